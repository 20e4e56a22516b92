// k_decode_persist1m_each: the multi-sequence form (t2s_persist1m.hip) with its sampler
// workgroups reading the per-sequence table (PersistArgs::per, gsv_t2s_generate_each).  The
// code is in t2s_persist1.hip under PERSIST1_MULTI and PERSIST_SEQ_TABLE.
#define PERSIST_SEQ_TABLE
#define PERSIST1_MULTI
#include "t2s_persist1.hip"

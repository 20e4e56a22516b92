// k_decode_persistm_each: the batched persistent decode with its sampler workgroups reading
// the per-sequence table (PersistArgs::per, gsv_t2s_generate_each).  The code is in
// t2s_persistm.hip under PERSIST_SEQ_TABLE.
#define PERSIST_SEQ_TABLE
#include "t2s_persistm.hip"

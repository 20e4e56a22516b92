// k_decode_persist1_each: the single-sequence persistent decode with its sampler reading the
// per-sequence table (PersistArgs::per, gsv_t2s_generate_each).  Its own translation unit, so
// k_decode_persist1 keeps the code it has without the read.  The code is in t2s_persist1.hip
// under PERSIST_SEQ_TABLE.
#define PERSIST_SEQ_TABLE
#include "t2s_persist1.hip"

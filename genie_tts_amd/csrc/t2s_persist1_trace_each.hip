// k_decode_persist1_trace_each: k_decode_persist1_each (the sampler reading the per-sequence
// table) with the phase stamps compiled in.  The code is in t2s_persist1.hip under
// PERSIST_TRACE and PERSIST_SEQ_TABLE.
#define PERSIST_TRACE
#define PERSIST_SEQ_TABLE
#include "t2s_persist1.hip"

// k_decode_persist1_trace: the single-sequence persistent decode with its phase stamps
// compiled in (engine option "ptrace"; tools/ptrace2.py, tools/knob_sweep.py).  Its own
// translation unit, so k_decode_persist1 carries no stamp code and keeps the register
// allocation it has alone.  The code is in t2s_persist1.hip under PERSIST_TRACE.
#define PERSIST_TRACE
#include "t2s_persist1.hip"

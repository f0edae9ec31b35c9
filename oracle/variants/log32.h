/* variants/log32.h — slip variant (CPU tests only): log evaluated through float, what a single-precision temporary or a
 * call that resolves to the single-precision overload does.  tests/test_parity_bars_cpu.py proves the parity bars see it. */
#include "probe.h"

static inline double orcv_log32(double x) { return (double)logf((float)x); }
#define log(x) orcv_log32(x)

/* variants/exp32.h — slip variant (CPU tests only): exp evaluated through float, what a single-precision temporary or a
 * call that resolves to the single-precision overload does.  tests/test_parity_bars_cpu.py proves the parity bars see it. */
#include "probe.h"

static inline double orcv_exp32(double x) { return (double)expf((float)x); }
#define exp(x) orcv_exp32(x)

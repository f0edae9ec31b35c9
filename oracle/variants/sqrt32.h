/* variants/sqrt32.h — slip variant (CPU tests only): sqrt evaluated through float, what a single-precision temporary or a
 * call that resolves to the single-precision overload does.  tests/test_parity_bars_cpu.py proves the parity bars see it. */
#include "probe.h"

static inline double orcv_sqrt32(double x) { return (double)sqrtf((float)x); }
#define sqrt(x) orcv_sqrt32(x)

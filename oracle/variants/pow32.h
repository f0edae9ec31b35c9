/* variants/pow32.h — slip variant (CPU tests only): pow evaluated through float, what a single-precision temporary or a
 * call that resolves to the single-precision overload does.  tests/test_parity_bars_cpu.py proves the parity bars see it. */
#include "probe.h"

static inline double orcv_pow32(double x, double y) { return (double)powf((float)x, (float)y); }
#define pow(x, y) orcv_pow32(x, y)

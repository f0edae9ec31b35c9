/* variants/exp46.h — slip variant (CPU tests only): exp with the low 7 mantissa bits cleared, what a medium-precision
 * (46-bit) routine placed ahead of amplifying algebra looks like.  Reported by the CPU tests, not asserted. */
#include "probe.h"

static inline double orcv_exp46(double x)
{
    double r = exp(x);
    uint64_t b;
    memcpy(&b, &r, sizeof b);
    if (((b >> 52) & 0x7FF) != 0x7FF) b &= ~(uint64_t)0x7F;
    memcpy(&r, &b, sizeof r);
    return r;
}
#define exp(x) orcv_exp46(x)

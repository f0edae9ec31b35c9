/* variants/ulp.h — noise variant: every result of the libm calls for which the device uses a routine of its own or the
 * device library's (exp, log, pow, sqrt, sin, cos, tan, atan, acos, asin) moved by -2 .. +2 ulp.  The step is chosen by a
 * hash of the result's bits, so the build is still a function of its inputs and runs are reproducible.  +-2 ulp is the
 * accuracy class tests/test_math_gpu.py asserts for the lean device routines: this build is one more correct fp64
 * evaluation of the model, and its distance from the default build measures how far two correct evaluations may lie apart. */
#include "probe.h"

static inline double orcv_jitter(double r)
{
    uint64_t b, h;
    memcpy(&b, &r, sizeof b);
    uint64_t e = (b >> 52) & 0x7FF;
    if (e == 0 || e >= 0x7FE) return r;          /* zero, subnormal, top binade, inf, NaN: untouched */
    h = b * 0x9E3779B97F4A7C15ull;               /* splitmix64 finaliser */
    h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 27; h *= 0x94D049BB133111EBull;
    h ^= h >> 31;
    b += (uint64_t)((int64_t)(h % 5) - 2);       /* neighbouring doubles are neighbouring bit patterns */
    memcpy(&r, &b, sizeof r);
    return r;
}
static inline double orcv_exp(double x) { return orcv_jitter(exp(x)); }
static inline double orcv_log(double x) { return orcv_jitter(log(x)); }
static inline double orcv_pow(double x, double y) { return orcv_jitter(pow(x, y)); }
static inline double orcv_sqrt(double x) { return orcv_jitter(sqrt(x)); }
static inline double orcv_sin(double x) { return orcv_jitter(sin(x)); }
static inline double orcv_cos(double x) { return orcv_jitter(cos(x)); }
static inline double orcv_tan(double x) { return orcv_jitter(tan(x)); }
static inline double orcv_atan(double x) { return orcv_jitter(atan(x)); }
static inline double orcv_acos(double x) { return orcv_jitter(acos(x)); }
static inline double orcv_asin(double x) { return orcv_jitter(asin(x)); }
#define exp(x) orcv_exp(x)
#define log(x) orcv_log(x)
#define pow(x, y) orcv_pow(x, y)
#define sqrt(x) orcv_sqrt(x)
#define sin(x) orcv_sin(x)
#define cos(x) orcv_cos(x)
#define tan(x) orcv_tan(x)
#define atan(x) orcv_atan(x)
#define acos(x) orcv_acos(x)
#define asin(x) orcv_asin(x)

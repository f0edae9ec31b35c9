/* variants/probe.h — TEST INFRASTRUCTURE: every perturbed build of the oracle (oracle/Makefile, tests/parity_bars.py)
 * force-includes this ahead of oracle_unit.c.  <math.h> is read here, once, so that the macros a variant header lays over
 * libm names afterwards rename the oracle's calls and not libm's declarations; orc_variant_probe() lets the loader ask,
 * before any floating-point code of the library runs, whether this host can execute it. */
#ifndef ORC_VARIANT_PROBE_H
#define ORC_VARIANT_PROBE_H
#include <math.h>
#include <stdint.h>
#include <string.h>

int orc_variant_probe(void);
int orc_variant_probe(void)
{
#ifdef __FMA__                                   /* built with -mfma: needs a host with fused multiply-add */
    return __builtin_cpu_supports("fma") ? 1 : 0;
#else
    return 1;
#endif
}
#endif

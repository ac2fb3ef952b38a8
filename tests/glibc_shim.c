/* The CPU oracle in libm = glibc-2.35 mode (tests/glibc_oracle.py): oracle/*.c compiled with -DORACLE_USE_LIBM, which calls the C
 * library's sinf / cosf / acosf (and cos, reference random.cpp:134), linked with this object, which defines those functions -- with hidden
 * visibility, so only the oracle's own calls bind to them -- from include/ssx_glibc_math.h.  The oracle then computes what it computes
 * against glibc 2.35 on an x86-64 FMA host, on any host (tests/test_glibc_math_cpu.py checks that it does, where the host has that glibc).
 * sincosf: GCC merges the oracle's sinf / cosf pairs of one argument into it.  cos: the reference rounds cos((double)x) of a float x back
 * to float, which is ssx_cosf(x) for every x the integrator passes (0 <= x < pi; checked against glibc's cos on all floats in [0, 4]). */
#include "ssx_fmath.h"
#include "ssx_glibc_math.h"

#define SHIM __attribute__((visibility("hidden")))
SHIM float sinf(float x) { return ssx_glibc_sinf(x); }
SHIM float cosf(float x) { return ssx_glibc_cosf(x); }
SHIM void sincosf(float x, float* s, float* c) { ssx_glibc_sincosf(x, s, c); }
SHIM float acosf(float x) { return ssx_glibc_acosf(x); }
SHIM double cos(double x) { return (double)ssx_cosf((float)x); }

/* ssx_glibc_math.h -- glibc 2.35's x86-64 sinf / cosf / sincosf / acosf, restated bit for bit.
 *
 * Why this exists: include/ssx_fmath.h defines the transcendentals of the parity contract once, for the
 * build ("libm = build", the default).  The reference as users actually build it on x86-64 calls glibc
 * instead, and glibc's results differ from those in many ulp-level cases (tests/test_oracle_pins.py:
 * about 31 % of cornell-srgb samples change in at least one bit).  The run-time mode "libm = glibc-2.35"
 * evaluates the functions below on the GPU (and, through a shim, in the CPU oracle), so that an image can
 * be compared with a stock x86-64 build of the reference bit for bit.
 *
 * What is restated (glibc 2.35, x86-64):
 *   sinf, cosf, sincosf  glibc's sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, s_sincosf.c -- Arm's
 *                        optimized-routines algorithm (Szabolcs Nagy, 2018; MIT OR Apache-2.0 WITH
 *                        LLVM-exception): abstop12 range split, |x| < 0.75 direct, reduce_fast below 120,
 *                        reduce_large with the 2/pi bit table beyond, sinf_poly in binary64.  x86-64 glibc
 *                        selects an FMA build of these (an ifunc) on every AVX2 + FMA host; GCC contracted
 *                        the multiply-adds of that build, which is restated here with an explicit fma()
 *                        wherever it contracted and plain operations elsewhere.  sincosf returns exactly
 *                        (sinf(x), cosf(x)) for every x, so it shares their code.
 *   acosf                fdlibm's binary32 __ieee754_acosf (Copyright (C) 1993 by Sun Microsystems, Inc.
 *                        "Developed at SunPro, a Sun Microsystems, Inc. business.  Permission to use, copy,
 *                        modify, and distribute this software is freely granted, provided that this notice
 *                        is preserved."; float version by Ian Lance Taylor, Cygnus Support).  glibc 2.35 has
 *                        one, non-ifunc acosf, built for the x86-64 baseline: no contraction.
 * The constants were rebuilt from the published algorithms and checked against the tables of the
 * installed libm.so.6.  The arbiter is tests/test_glibc_math_cpu.py, which compares every function with the
 * host's glibc on all 2^32 inputs (NaN matches NaN).
 *
 * Plain C99 / C++17 / HIP.  Compile every user with -ffp-contract=off: the fma() calls below are the only
 * fused operations.  A HIP kernel may define SSX_GM_TABLE to an array of doubles filled from
 * SSX_GM_COEFF_INIT (same order) so that the binary64 coefficients are loaded where they are used instead of
 * being held in registers; the 2/pi bit table (only read for |x| >= 120) is always read from memory (device
 * memory in HIP code, which then calls these functions on the device only).
 */
#ifndef SSX_GLIBC_MATH_H
#define SSX_GLIBC_MATH_H

#if defined(SSX_GM_TABLE)
#define SSX_GM_FN static __device__ __forceinline__   /* the coefficients live in LDS: device code only */
#define SSX_GM_DATA __device__
#elif defined(__HIPCC__) || defined(__HIP__)
#define SSX_GM_FN static __host__ __device__ __forceinline__
#define SSX_GM_DATA __device__
#else
#define SSX_GM_FN static inline
#define SSX_GM_DATA
#endif
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#define SSX_GM_FMA(a, b, c) __builtin_fma((a), (b), (c))

/* sincos_t of sincosf.h, table 0 (table 1 is the same with c0..c4 negated: see ssx_gm_sinf_poly) */
#define SSX_GM_LIST(X) \
	X(HPI_INV, 0x1.45F306DC9C883p+23) /* 2/pi * 2^24 (the shift-based reduce_fast) */ \
	X(HPI, 0x1.921FB54442D18p0)       /* pi/2 */ \
	X(C0, 0x1p0) \
	X(C1, -0x1.ffffffd0c621cp-2) \
	X(C2, 0x1.55553e1068f19p-5) \
	X(C3, -0x1.6c087e89a359dp-10) \
	X(C4, 0x1.99343027bf8c3p-16) \
	X(S1, -0x1.555545995a603p-3) \
	X(S2, 0x1.1107605230bc4p-7) \
	X(S3, -0x1.994eb3774cf24p-13) \
	X(PI63, 0x1.921FB54442D18p-62)    /* pi/2 * 2^-62 (reduce_large) */
enum {
#define SSX_GM_ENUM(name, lit) SSX_GM_I_##name,
	SSX_GM_LIST(SSX_GM_ENUM)
#undef SSX_GM_ENUM
	SSX_GM_N_COEFF
};
#define SSX_GM_VALUE(name, lit) lit,
#define SSX_GM_COEFF_INIT { SSX_GM_LIST(SSX_GM_VALUE) }
#ifdef SSX_GM_TABLE
#define SSX_GM_C(name) (SSX_GM_TABLE[SSX_GM_I_##name])
#else
#define SSX_GM_LITERAL(name, lit) static const double ssx_gm_lit_##name = lit;
SSX_GM_LIST(SSX_GM_LITERAL)
#undef SSX_GM_LITERAL
#define SSX_GM_C(name) (ssx_gm_lit_##name)
#endif

/* __inv_pio4: 2/pi in overlapping 32-bit windows, 8 bits apart */
static SSX_GM_DATA const uint32_t ssx_gm_inv_pio4[24] = {
	0xa2,       0xa2f9,     0xa2f983,   0xa2f9836e,
	0xf9836e4e, 0x836e4e44, 0x6e4e4415, 0x4e441529,
	0x441529fc, 0x1529fc27, 0x29fc2757, 0xfc2757d1,
	0x2757d1f5, 0x57d1f534, 0xd1f534dd, 0xf534ddc0,
	0x34ddc0db, 0xddc0db62, 0xc0db6295, 0xdb629599,
	0x6295993c, 0x95993c43, 0x993c4390, 0x3c439041
};

SSX_GM_FN uint32_t ssx_gm_asuint(float f) { union { float f; uint32_t u; } v; v.f = f; return v.u; }
SSX_GM_FN float ssx_gm_asfloat(uint32_t u) { union { float f; uint32_t u; } v; v.u = u; return v.f; }
/* the top 12 bits of |x| (sign cleared) */
SSX_GM_FN uint32_t ssx_gm_abstop12(float x) { return (ssx_gm_asuint(x) >> 20) & 0x7ff; }
#define SSX_GM_TOP12_PIO4 0x3f4u   /* abstop12(0x1.921FB6p-1f): the direct range is |x| < 0.75 */
#define SSX_GM_TOP12_TINY 0x398u   /* abstop12(0x1p-12f) */
#define SSX_GM_TOP12_120 0x42fu    /* abstop12(120.0f) */
#define SSX_GM_TOP12_INF 0x7f8u    /* abstop12(INFINITY) */

/* sinf_poly with table 0 (neg = 0) or table 1 (neg = 1).  Table 1 differs from table 0 only in the sign of
 * c0..c4, and every operation of the cosine branch is odd in those coefficients (round to nearest even is
 * symmetric), so table 1's result is the negated table 0 result.  Contractions as in the FMA build. */
SSX_GM_FN double ssx_gm_sin_poly(double x, double x2) {
	const double x3 = x * x2;
	const double s1 = SSX_GM_FMA(x2, SSX_GM_C(S3), SSX_GM_C(S2));
	const double x7 = x3 * x2;
	const double s = SSX_GM_FMA(x3, SSX_GM_C(S1), x);
	return SSX_GM_FMA(x7, s1, s);
}
SSX_GM_FN double ssx_gm_cos_poly(double x2) {
	const double x4 = x2 * x2;
	const double c2 = SSX_GM_FMA(x2, SSX_GM_C(C4), SSX_GM_C(C3));
	const double c1 = SSX_GM_FMA(x2, SSX_GM_C(C1), SSX_GM_C(C0));
	const double x6 = x4 * x2;
	const double c = SSX_GM_FMA(x4, SSX_GM_C(C2), c1);
	return SSX_GM_FMA(x6, c2, c);
}
SSX_GM_FN float ssx_gm_sinf_poly(double x, double x2, int neg, int n) {
	if ((n & 1) == 0) return (float)ssx_gm_sin_poly(x, x2);
	const double c = ssx_gm_cos_poly(x2);
	return (float)(neg ? -c : c);
}

/* reduce_fast, shift-based (TOINT_INTRINSICS is 0 on x86-64): |x| < 120 */
SSX_GM_FN double ssx_gm_reduce_fast(double x, int* np) {
	const double r = x * SSX_GM_C(HPI_INV);
	const int n = ((int32_t)r + 0x800000) >> 24;
	*np = n;
	return SSX_GM_FMA(-(double)n, SSX_GM_C(HPI), x);
}

/* reduce_large: 120 <= |x| < inf; x reduced for |x| (the sign is applied by the caller) */
SSX_GM_FN double ssx_gm_reduce_large(uint32_t xi, int* np) {
	const uint32_t* arr = &ssx_gm_inv_pio4[(xi >> 26) & 15];
	const int shift = (xi >> 23) & 7;
	uint64_t n, res0, res1, res2;
	xi = (xi & 0xffffff) | 0x800000;
	xi <<= shift;
	res0 = (uint32_t)(xi * arr[0]);
	res1 = (uint64_t)xi * arr[4];
	res2 = (uint64_t)xi * arr[8];
	res0 = (res2 >> 32) | (res0 << 32);
	res0 += res1;
	n = (res0 + (1ULL << 61)) >> 62;
	res0 -= n << 62;
	const double x = (double)(int64_t)res0;
	*np = (int)n;
	return x * SSX_GM_C(PI63);
}

/* the shared part of sinf (cos_ = 0) and cosf (cos_ = 1) */
SSX_GM_FN float ssx_gm_sincos1(float y, int cos_) {
	double x = y;
	const uint32_t top = ssx_gm_abstop12(y);
	if (top < SSX_GM_TOP12_PIO4) {
		if (top < SSX_GM_TOP12_TINY) return cos_ ? 1.0f : y;
		return ssx_gm_sinf_poly(x, x * x, 0, cos_);
	}
	int n, q;
	if (top < SSX_GM_TOP12_120) {
		x = ssx_gm_reduce_fast(x, &n);
		q = n;
	} else if (top < SSX_GM_TOP12_INF) {
		const uint32_t xi = ssx_gm_asuint(y);
		x = ssx_gm_reduce_large(xi, &n);
		q = n + (int)(xi >> 31);
	} else {
		return y - y; /* NaN for inf and NaN */
	}
	const double s = ((q & 3) == 1 || (q & 3) == 2) ? -1.0 : 1.0; /* sign[] = { 1, -1, -1, 1 } */
	return ssx_gm_sinf_poly(x * s, x * x, (q & 2) != 0, n ^ cos_);
}

SSX_GM_FN float ssx_glibc_sinf(float x) { return ssx_gm_sincos1(x, 0); }
SSX_GM_FN float ssx_glibc_cosf(float x) { return ssx_gm_sincos1(x, 1); }

/* sincosf: one reduction, the sine and the cosine branch of the same polynomial pair */
SSX_GM_FN void ssx_glibc_sincosf(float y, float* sinp, float* cosp) {
	double x = y;
	const uint32_t top = ssx_gm_abstop12(y);
	if (top < SSX_GM_TOP12_PIO4) {
		if (top < SSX_GM_TOP12_TINY) { *sinp = y; *cosp = 1.0f; return; }
		const double x2 = x * x;
		*sinp = (float)ssx_gm_sin_poly(x, x2);
		*cosp = (float)ssx_gm_cos_poly(x2);
		return;
	}
	int n, q;
	if (top < SSX_GM_TOP12_120) {
		x = ssx_gm_reduce_fast(x, &n);
		q = n;
	} else if (top < SSX_GM_TOP12_INF) {
		const uint32_t xi = ssx_gm_asuint(y);
		x = ssx_gm_reduce_large(xi, &n);
		q = n + (int)(xi >> 31);
	} else {
		*sinp = *cosp = y - y;
		return;
	}
	const double s = ((q & 3) == 1 || (q & 3) == 2) ? -1.0 : 1.0;
	const double xs = x * s, x2 = x * x;
	const int neg = (q & 2) != 0;
	const float sv = (float)ssx_gm_sin_poly(xs, x2);
	const double c = ssx_gm_cos_poly(x2);
	const float cv = (float)(neg ? -c : c);
	*sinp = (n & 1) ? cv : sv;
	*cosp = (n & 1) ? sv : cv;
}

/* fdlibm __ieee754_acosf, binary32 throughout, no contraction */
SSX_GM_FN float ssx_gm_acosf_rat(float z) {
	const float pS0 = 1.6666667163e-01f, pS1 = -3.2556581497e-01f, pS2 = 2.0121252537e-01f,
	            pS3 = -4.0055535734e-02f, pS4 = 7.9153501429e-04f, pS5 = 3.4793309169e-05f,
	            qS1 = -2.4033949375e+00f, qS2 = 2.0209457874e+00f, qS3 = -6.8828397989e-01f,
	            qS4 = 7.7038154006e-02f;
	const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
	const float q = 1.0f + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
	return p / q;
}
SSX_GM_FN float ssx_glibc_acosf(float x) {
	const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
	const uint32_t hx = ssx_gm_asuint(x), ix = hx & 0x7fffffffu;
	if (ix == 0x3f800000u) return (hx >> 31) ? pi + 2.0f * pio2_lo : 0.0f;
	if (ix > 0x3f800000u) return (x - x) / (x - x);
	if (ix < 0x3f000000u) { /* |x| < 0.5 */
		if (ix <= 0x32800000u) return pio2_hi + pio2_lo;
		const float z = x * x;
		const float r = ssx_gm_acosf_rat(z);
		return pio2_hi - (x - (pio2_lo - x * r));
	}
	if (hx >> 31) { /* x <= -0.5 */
		const float z = (1.0f + x) * 0.5f;
		const float r = ssx_gm_acosf_rat(z);
		const float s = __builtin_sqrtf(z);
		const float w = r * s - pio2_lo;
		return pi - 2.0f * (s + w);
	}
	/* x >= 0.5 */
	const float z = (1.0f - x) * 0.5f;
	const float s = __builtin_sqrtf(z);
	const float df = ssx_gm_asfloat(ssx_gm_asuint(s) & 0xfffff000u);
	const float c = (z - df * df) / (s + df);
	const float r = ssx_gm_acosf_rat(z);
	const float w = r * s + c;
	return 2.0f * (df + w);
}

#endif /* SSX_GLIBC_MATH_H */

/* Exhaustive comparison of include/ssx_glibc_math.h with the host's glibc (tests/test_glibc_math_cpu.py).
 *
 *   glibc_math_check THREADS [LO HI]
 *   glibc_math_check digest THREADS
 *
 * Every binary32 pattern through sinf, cosf, sincosf and acosf of the C library and of the restatement
 * (NaN matches NaN, otherwise the bits must be equal), and (float)cos((double)x) against ssx_cosf(x) for
 * 0 <= x <= 4 (the argument of the reference's random.cpp:134 lies in [0, pi)).  Prints one JSON line.
 * "digest": the digests of ssx_debug_sweep's SSX_SWEEP_GLIBC_SIN / _COS / _ACOS (include/ssx.h), from the restatement alone (no libm call):
 * what the device's evaluation of the same header must reproduce (tests/test_glibc_mode_gpu.py).
 * Build with -fno-builtin (the calls must reach the library, not the compiler's constant folding) and
 * -ffp-contract=off. */
#define _GNU_SOURCE
#include <gnu/libc-version.h>
#include <inttypes.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssx_fmath.h"
#include "ssx_glibc_math.h"

enum { F_SIN, F_COS, F_SINCOS_S, F_SINCOS_C, F_ACOS, F_COSD, N_F };
static const char* names[N_F] = { "sinf", "cosf", "sincosf_sin", "sincosf_cos", "acosf", "cos_double_vs_ssx_cosf" };

typedef struct {
	uint64_t lo, hi;
	uint64_t bad[N_F];
	uint32_t first[N_F];
} Job;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static int same(float a, float b) { return (isnan(a) && isnan(b)) || bits(a) == bits(b); }

static void note(Job* j, int f, uint32_t u) {
	if (j->bad[f]++ == 0) j->first[f] = u;
}

static void* run(void* arg) {
	Job* j = (Job*)arg;
	for (uint64_t i = j->lo; i < j->hi; ++i) {
		const uint32_t u = (uint32_t)i;
		float x;
		memcpy(&x, &u, 4);
		if (!same(sinf(x), ssx_glibc_sinf(x))) note(j, F_SIN, u);
		if (!same(cosf(x), ssx_glibc_cosf(x))) note(j, F_COS, u);
		float s, c, s2, c2;
		sincosf(x, &s, &c);
		ssx_glibc_sincosf(x, &s2, &c2);
		if (!same(s, s2)) note(j, F_SINCOS_S, u);
		if (!same(c, c2)) note(j, F_SINCOS_C, u);
		if (!same(acosf(x), ssx_glibc_acosf(x))) note(j, F_ACOS, u);
		if (u <= 0x40800000u && !same((float)cos((double)x), ssx_cosf(x))) note(j, F_COSD, u);
	}
	return NULL;
}

/* splitmix64 of (x << 32 | result), any NaN result as 0x7FC00000: csrc/ssx_debug.hip glibc_digest_word */
static uint64_t digest_word(uint32_t x, float y) {
	uint64_t z = ((uint64_t)x << 32) | (isnan(y) ? 0x7FC00000u : bits(y));
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
typedef struct { uint64_t lo, hi, d[3]; } DigestJob;
static void* run_digest(void* arg) {
	DigestJob* j = (DigestJob*)arg;
	for (uint64_t i = j->lo; i < j->hi; ++i) {
		const uint32_t u = (uint32_t)i;
		float x;
		memcpy(&x, &u, 4);
		j->d[0] += digest_word(u, ssx_glibc_sinf(x));
		j->d[1] += digest_word(u, ssx_glibc_cosf(x));
		j->d[2] += digest_word(u, ssx_glibc_acosf(x));
	}
	return NULL;
}
static int digest_main(int nt) {
	DigestJob jobs[16];
	pthread_t th[16];
	const uint64_t total = 1ull << 32;
	for (int t = 0; t < nt; ++t) {
		memset(&jobs[t], 0, sizeof jobs[t]);
		jobs[t].lo = total * (uint64_t)t / (uint64_t)nt;
		jobs[t].hi = total * (uint64_t)(t + 1) / (uint64_t)nt;
		pthread_create(&th[t], NULL, run_digest, &jobs[t]);
	}
	uint64_t d[3] = { 0, 0, 0 };
	for (int t = 0; t < nt; ++t) {
		pthread_join(th[t], NULL);
		for (int k = 0; k < 3; ++k) d[k] += jobs[t].d[k];
	}
	printf("{\"sinf\": %" PRIu64 ", \"cosf\": %" PRIu64 ", \"acosf\": %" PRIu64 "}\n", d[0], d[1], d[2]);
	return 0;
}

int main(int argc, char** argv) {
	if (argc > 1 && strcmp(argv[1], "digest") == 0) {
		int nt = argc > 2 ? atoi(argv[2]) : 8;
		return digest_main(nt < 1 ? 1 : (nt > 16 ? 16 : nt));
	}
	int nt = argc > 1 ? atoi(argv[1]) : 8;
	if (nt < 1) nt = 1;
	if (nt > 16) nt = 16;
	const uint64_t total = 1ull << 32;
	uint64_t lo = argc > 2 ? strtoull(argv[2], NULL, 0) : 0, hi = argc > 3 ? strtoull(argv[3], NULL, 0) : total;
	pthread_t th[16];
	/* 64 rounds of one chunk per thread: the rounds are short, so a slow range (reduce_large) holds up one round only */
	const int chunks = nt * 64;
	Job* part = (Job*)calloc((size_t)chunks, sizeof(Job));
	for (int k = 0; k < chunks; ++k) {
		part[k].lo = lo + (hi - lo) * (uint64_t)k / (uint64_t)chunks;
		part[k].hi = lo + (hi - lo) * (uint64_t)(k + 1) / (uint64_t)chunks;
	}
	for (int round = 0; round < 64; ++round) {
		for (int t = 0; t < nt; ++t) pthread_create(&th[t], NULL, run, &part[round * nt + t]);
		for (int t = 0; t < nt; ++t) pthread_join(th[t], NULL);
	}
	uint64_t bad[N_F] = { 0 };
	uint32_t first[N_F] = { 0 };
	int have[N_F] = { 0 };
	for (int k = 0; k < chunks; ++k)
		for (int f = 0; f < N_F; ++f)
			if (part[k].bad[f]) {
				if (!have[f]) { have[f] = 1; first[f] = part[k].first[f]; }
				bad[f] += part[k].bad[f];
			}
	printf("{\"glibc\": \"%s\", \"inputs\": %" PRIu64, gnu_get_libc_version(), hi - lo);
	for (int f = 0; f < N_F; ++f) printf(", \"%s\": [%" PRIu64 ", \"0x%08x\"]", names[f], bad[f], first[f]);
	printf("}\n");
	free(part);
	return 0;
}

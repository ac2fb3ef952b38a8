// ssx_debug.hip -- device-side unit evaluation of the path megakernel's building blocks, for the
// parity tests (include/ssx.h: ssx_debug_eval, ssx_debug_samples).  Each op runs the SAME device
// function the megakernel inlines (this file is part of the same translation unit), one item per
// lane, on inputs the test supplies, so the tests can compare it with the oracle's unit-level
// functions on edge cases the renders reach rarely or never (degenerate spherical triangles, rays
// through shared vertices, the Lemire redraw, ...).  SSX_DBG_TRACE and SSX_DBG_TRACE_MASKED run the generic trace<0> whatever the
// context's topology; SSX_DBG_TRACE_TOPO (ssx_debug_trace_cornell_kernel / _plane_kernel below, and ssx_debug_trace_jit of csrc/ssx_kernels.hip for a scene's
// own pattern) runs the topology-specialised trace the context's renders run.  Nothing here runs during a render.
#include "../../include/ssx.h"
#include "ssx_ddmath.h" // the independent evaluation of sin / cos / acos that ssx_fmath.h is proved against (SSX_SWEEP_*_PROOF)

namespace {

__device__ __forceinline__ Rng load_rng(const uint32_t* w) {
	Rng r;
	r.state = ((uint64_t)w[1] << 32) | w[0];
	r.inc = ((uint64_t)w[3] << 32) | w[2];
	return r;
}
__device__ __forceinline__ float f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t u(float x) { return __float_as_uint(x); }

} // namespace

// Exhaustive / hashed sweeps on the device: for every 32-bit pattern x in [lo, lo + count) compare a cheaper
// function with the function that defines the result.  res[0] = mismatches, res[1] = a per-op maximum
// (rcp64: largest error in ulps), res[2] = stored examples, res[3..] = up to 8 mismatching inputs.
__device__ __forceinline__ uint32_t sweep_hash(uint32_t h) {
	h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
	return h;
}
__device__ __forceinline__ bool same_float(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
extern "C" __global__ void __launch_bounds__(256) ssx_debug_sweep_kernel(SsxKernelArgs a, uint32_t op, uint32_t lo, uint64_t count, unsigned long long* res) {
	Lds L; L.w = stage_lds(a);
	(void)L;
	unsigned long long bad = 0, mx = 0;
	uint32_t example = 0; bool have_example = false;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t bits = lo + (uint32_t)i;
		const float x = __uint_as_float(bits);
		bool ok = true;
		switch (op) {
		case SSX_SWEEP_RCP: ok = same_float(ssx_exact::rcp(x), 1.0f / x); break;
		case SSX_SWEEP_SQRT: ok = same_float(ssx_exact::sqrt_normal(x), __builtin_sqrtf(x)); break;
		case SSX_SWEEP_INVERSESQRT: ok = same_float(inversesqrt_(x), 1.0f / __builtin_sqrtf(x)); break;
		case SSX_SWEEP_SIN: ok = same_float(ssx_sinf_lds(x), ssx_sinf(x)); break;
		case SSX_SWEEP_COS: ok = same_float(ssx_cosf_lds(x), ssx_cosf(x)); break;
		case SSX_SWEEP_ACOS: ok = same_float(ssx_acosf_lds(x), ssx_acosf(x)); break;
		case SSX_SWEEP_DIV_PI: ok = same_float(SSX_DIV_CONST(x, SSX_PI_F), x / SSX_PI_F); break;
		case SSX_SWEEP_ACOS_SIN: { // the fused arc + sine of the spherical-triangle code, on its domain |x| <= 1
			if (!(__builtin_fabsf(x) <= 1.0f)) break;
			const float amax = __uint_as_float(0x40490FDAu);
			float sn; int sn_ok;
			const float arc = ssx_acos_sin_lds(x, amax, &sn, &sn_ok);
			const float arc_ref = clamp_glm(ssx_acosf(x), 0.0f, amax);
			ok = same_float(arc, arc_ref) && (!sn_ok || same_float(sn, ssx_sinf(arc_ref)));
			if (!sn_ok) mx += 1; // fallbacks (per thread; summed below)
			break;
		}
		case SSX_SWEEP_RCP64: { // accuracy of the binary64 reciprocal behind div64_*: error in ulps of the correctly rounded 1/x
			const double r = ssx_exact::div64_rcp_any(x), t = 1.0 / (double)x;
			if (r != r || t != t) { ok = (r != r) == (t != t); break; }
			const long long d = (long long)__double_as_longlong(r) - (long long)__double_as_longlong(t);
			const unsigned long long ad = (unsigned long long)(d < 0 ? -d : d);
			mx = ad > mx ? ad : mx;
			ok = ad <= 1ull;
			break;
		}
		case SSX_SWEEP_DIV_PAIRS: { // a = this pattern, b = hashes of it (arbitrary patterns, and the same exponent range as a)
			const uint32_t h = sweep_hash(bits ^ 0x9E3779B9u);
			const float b1 = __uint_as_float(h);
			const float b2 = __uint_as_float((bits & 0x7F800000u) | (h & 0x807FFFFFu)); // same exponent: quotients in [0.5, 2)
			const double r1 = ssx_exact::div64_rcp_any(b1), r2 = ssx_exact::div64_rcp_any(b2);
			ok = same_float(ssx_exact::div64_by(x, r1), x / b1) && same_float(ssx_exact::div64_by(x, r2), x / b2) &&
			     same_float(ssx_exact::div64_by(b1, ssx_exact::div64_rcp_any(x)), b1 / x);
			break;
		}
		case SSX_SWEEP_SIN_PROOF: case SSX_SWEEP_COS_PROOF: case SSX_SWEEP_ACOS_PROOF: { // ssx_fmath.h against csrc/ssx_ddmath.h
			const bool arc = op == SSX_SWEEP_ACOS_PROOF;
			const float got = op == SSX_SWEEP_SIN_PROOF ? ssx_sinf(x) : (arc ? ssx_acosf(x) : ssx_cosf(x));
			if (!arc) { // ssx_sincosf (what the samplers call) returns the same two floats as ssx_sinf and ssx_cosf, for every input
				float sc_s, sc_c;
				ssx_sincosf(x, &sc_s, &sc_c);
				if (!same_float(op == SSX_SWEEP_SIN_PROOF ? sc_s : sc_c, got)) {
					atomicAdd(&res[0], 1ull);
					const unsigned long long slot = atomicAdd(&res[2], 1ull);
					if (slot < 8ull) res[3 + slot] = bits;
				}
			}
			if (!(__builtin_fabsf(x) <= (arc ? 1.0f : 0x1p20f))) { ok = got != got; break; } // outside the domain (and NaN): NaN
			int decided = 1;
			const float want = op == SSX_SWEEP_SIN_PROOF ? ssx_dd::sin_f32(x, &decided) : (arc ? ssx_dd::acos_f32(x, acos((double)x), &decided) : ssx_dd::cos_f32(x, &decided));
			if (!decided) { // too close to a rounding boundary for ~100 bits: the host settles it (tests/test_fmath.py)
				++mx;
				const unsigned long long slot = atomicAdd(&res[2], 1ull);
				if (slot < 8ull) res[3 + slot] = (unsigned long long)bits | (1ull << 32);
				break;
			}
			if (__float_as_uint(got) != __float_as_uint(want)) { // every one of these is listed (the header's known exceptions: a handful)
				atomicAdd(&res[0], 1ull);
				const unsigned long long slot = atomicAdd(&res[2], 1ull);
				if (slot < 8ull) res[3 + slot] = bits;
			}
			break;
		}
		default: break;
		}
		if (!ok) { ++bad; if (!have_example) { example = bits; have_example = true; } }
	}
	if (bad) {
		atomicAdd(&res[0], bad);
		const unsigned long long slot = atomicAdd(&res[2], 1ull);
		if (slot < 8ull) res[3 + slot] = example;
	}
	if (mx) { if (op == SSX_SWEEP_ACOS_SIN || op >= SSX_SWEEP_SIN_PROOF) atomicAdd(&res[1], mx); else atomicMax(&res[1], mx); }
}

extern "C" __global__ void __launch_bounds__(256) ssx_debug_eval_kernel(SsxKernelArgs a, uint32_t op, const uint32_t* in, uint32_t in_words,
                                                                       uint32_t* out, uint32_t out_words, uint32_t n) {
	Lds L; L.w = stage_lds(a);
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	// every lane of a wave runs the op (trace() wants uniform control flow); lanes past the end redo item n-1
	const uint32_t item = gid < n ? gid : n - 1u;
	const uint32_t* x = in + (size_t)item * in_words;
	uint32_t o[12];
#pragma unroll
	for (int k = 0; k < 12; ++k) o[k] = 0u;
	switch (op) {
	case SSX_DBG_FMATH: { // in: x -> sin, cos, acos, sincos.s, sincos.c
		float s, c;
		ssx_sincosf(f(x[0]), &s, &c);
		o[0] = u(ssx_sinf(f(x[0]))); o[1] = u(ssx_cosf(f(x[0]))); o[2] = u(ssx_acosf(f(x[0]))); o[3] = u(s); o[4] = u(c);
		break;
	}
	case SSX_DBG_SPHTRI: { // in: A, B, C (unit vectors) -> b, cos_c, alpha, cos_alpha, area
		SphTri t;
		sphtri_make(mk(f(x[0]), f(x[1]), f(x[2])), mk(f(x[3]), f(x[4]), f(x[5])), mk(f(x[6]), f(x[7]), f(x[8])), t);
		o[0] = u(t.b); o[1] = u(t.cos_c); o[2] = u(t.alpha); o[3] = u(t.cos_alpha); o[4] = u(t.area);
		break;
	}
	case SSX_DBG_ARVO: { // in: A, B, C, b, cos_c, alpha, cos_alpha, area, rng[4] -> dir, rng state
		SphTri t;
		t.A = mk(f(x[0]), f(x[1]), f(x[2])); t.B = mk(f(x[3]), f(x[4]), f(x[5])); t.C = mk(f(x[6]), f(x[7]), f(x[8]));
		t.b = f(x[9]); t.cos_c = f(x[10]); t.alpha = f(x[11]); t.cos_alpha = f(x[12]); t.area = f(x[13]);
		t.sin_alpha = ssx_sinf_lds(t.alpha);
		Rng r = load_rng(x + 14);
		V3 d = rand_toward_sphericaltri(r, t);
		o[0] = u(d.x); o[1] = u(d.y); o[2] = u(d.z); o[3] = (uint32_t)r.state; o[4] = (uint32_t)(r.state >> 32);
		break;
	}
	case SSX_DBG_SAMPLE_LIGHT: { // in: from, rng[4] -> dir, light quad, pdf, rng state
		Rng r = load_rng(x + 3);
		V3 d; uint32_t lq; float pdf;
		sample_light(L, r, mk(f(x[0]), f(x[1]), f(x[2])), d, lq, pdf);
		o[0] = u(d.x); o[1] = u(d.y); o[2] = u(d.z); o[3] = lq; o[4] = u(pdf); o[5] = (uint32_t)r.state; o[6] = (uint32_t)(r.state >> 32);
		break;
	}
	case SSX_DBG_COSHEMI: { // in: normal, rng[4] -> w_i, pdf, rng state
		Rng r = load_rng(x + 3);
		float pdf;
		V3 w = get_rotated_to(rand_coshemi(r, pdf), mk(f(x[0]), f(x[1]), f(x[2])));
		o[0] = u(w.x); o[1] = u(w.y); o[2] = u(w.z); o[3] = u(pdf); o[4] = (uint32_t)r.state; o[5] = (uint32_t)(r.state >> 32);
		break;
	}
	case SSX_DBG_TRACE: { // in: orig, dir, ignore quad (int) -> hit quad (-1: none), tri of the quad, dist, st
		HitInfo h;
		trace<0>(L, mk(f(x[0]), f(x[1]), f(x[2])), mk(f(x[3]), f(x[4]), f(x[5])), (int)x[6], true, h);
		o[0] = h.tri < 0 ? 0xFFFFFFFFu : (uint32_t)h.tri >> 1;
		o[1] = h.tri < 0 ? 0u : (uint32_t)h.tri & 1u;
		o[2] = u(h.dist);
		if (h.tri >= 0) { float sx, sy; hit_st(L.quad((uint32_t)h.tri >> 1), (uint32_t)h.tri & 1u, h, sx, sy); o[3] = u(sx); o[4] = u(sy); }
		break;
	}
	case SSX_DBG_TRACE_MASKED: { // in: SSX_DBG_TRACE's row, mask[4] -> as SSX_DBG_TRACE
		// The masked pass 1 of ssx_generate_kernel's trace (there the mask is the tile's, ssx_tile_mask_kernel).  trace() reads the mask
		// through readfirstlane -- it is wave-uniform by contract -- so the wave works with the four words of its FIRST lane's row: the
		// caller lays its rows out in blocks of 64 that share one mask (include/ssx.h), and the lanes past the end redo item n - 1.
		HitInfo h;
		trace<0>(L, mk(f(x[0]), f(x[1]), f(x[2])), mk(f(x[3]), f(x[4]), f(x[5])), (int)x[6], true, h, 0, x + 7);
		o[0] = h.tri < 0 ? 0xFFFFFFFFu : (uint32_t)h.tri >> 1;
		o[1] = h.tri < 0 ? 0u : (uint32_t)h.tri & 1u;
		o[2] = u(h.dist);
		if (h.tri >= 0) { float sx, sy; hit_st(L.quad((uint32_t)h.tri >> 1), (uint32_t)h.tri & 1u, h, sx, sy); o[3] = u(sx); o[4] = u(sy); }
		break;
	}
	case SSX_DBG_RAND_CHOICE: { // in: rng[4], n -> choice, rng state
		Rng r = load_rng(x);
		o[0] = rand_choice(r, x[4]); o[1] = (uint32_t)r.state; o[2] = (uint32_t)(r.state >> 32);
		break;
	}
	case SSX_DBG_ALBEDO: { // in: quad, st, lambda_0 -> albedo at the four hero wavelengths
		Hero hh = material_albedo(L, L.quad(x[0]), f(x[1]), f(x[2]), f(x[3]));
		o[0] = u(hh.v[0]); o[1] = u(hh.v[1]); o[2] = u(hh.v[2]); o[3] = u(hh.v[3]);
		break;
	}
	case SSX_DBG_FLUX_TO_XYZ: { // in: flux[4], lambda_0 -> X, Y, Z
		Hero fl; fl.v[0] = f(x[0]); fl.v[1] = f(x[1]); fl.v[2] = f(x[2]); fl.v[3] = f(x[3]);
		float xyz[3];
		flux_to_xyz(L, fl, f(x[4]), xyz);
		o[0] = u(xyz[0]); o[1] = u(xyz[1]); o[2] = u(xyz[2]);
		break;
	}
	case SSX_DBG_RAND_1F: { // in: rng[4] -> rand_1f, rng state
		Rng r = load_rng(x);
		o[0] = u(rand_1f(r)); o[1] = (uint32_t)r.state; o[2] = (uint32_t)(r.state >> 32);
		break;
	}
	default: break;
	}
	if (gid < n)
		for (uint32_t k = 0; k < out_words && k < 12u; ++k) out[(size_t)gid * out_words + k] = o[k];
}

// SSX_DBG_TRACE_TOPO: the trace the context's renders run -- trace<1> (Cornell topology) or trace<2> (plane topology): the generated pass 1 of
// csrc/ssx_pass1_gen.h and the pass 2 that finds a candidate's vertices through triofs / vtab4 -- where SSX_DBG_TRACE above always runs the generic body.
// A kernel of its own: two more inlined traces in ssx_debug_eval_kernel's switch would change that kernel's registers for every other op.  It stages the
// whole blob, as ssx_debug_eval_kernel does, so one upload answers both ops.  (Topology 3: ssx_debug_trace_jit, csrc/ssx_kernels.hip, compiled at run time.)
#define SSX_DEBUG_TRACE_TOPO_KERNEL(name, topo) \
	extern "C" __global__ void __launch_bounds__(256) name(SsxKernelArgs a, const uint32_t* in, uint32_t in_words, uint32_t* out, uint32_t out_words, uint32_t n) { \
		debug_trace_rows<topo>(a, in, in_words, out, out_words, n); \
	}
SSX_DEBUG_TRACE_TOPO_KERNEL(ssx_debug_trace_cornell_kernel, 1)
SSX_DEBUG_TRACE_TOPO_KERNEL(ssx_debug_trace_plane_kernel, 2)
#undef SSX_DEBUG_TRACE_TOPO_KERNEL

// ssx_debug_fold (include/ssx.h): the path kernel's fold -- resolve_records, in the loop of unit_fold -- on levels the caller supplies.  One wave per 64
// pixels ("tile"), n_k samples per pixel, one cohort of SSX_COHORT_KS samples per pixel per pass.  The wave first writes the rows' levels into its own log
// regions, the way the path kernel's lanes do: through the store_* / *_word functions of csrc/ssx_kernels.hip that path_step, shadow_flush and the end of a
// path call, addressed through a LogRef as theirs; then it hands over to itself as the path kernel's lanes do (wave_release / wave_acquire and unit_fold's two
// fences) and folds cohort by cohort.  A kernel of its own per (queue entries, libm, flux) as the path kernels are: ssx_debug_eval_kernel keeps its registers.
//   rows [tile][pixel][k][SSX_FOLD_ROW_WORDS] (include/ssx.h); a.ray / a.st / a.flux: [tile][k][pixel] as a render's; a.accum [tile][component][pixel]
// Slots: the samples of a cohort take their level-entry and next-event slots one sample after the other in the order of a permutation of the cohort's 128
// places made from order_seed; bit 7 of the seed turns the order of a sample's own levels round.  Which slot an entry gets must not matter to the fold.
__device__ __forceinline__ uint32_t fold_rank(uint32_t rc, uint32_t seed) { return (rc * ((seed << 1) | 1u) + (seed >> 8)) & (SSX_COHORT_RECORDS - 1u); }
template <bool NARROW, bool GLIBC, bool FLUX>
__device__ __forceinline__ void debug_fold_body(const SsxKernelArgs& a, const uint32_t* rows, uint32_t n_tiles, uint32_t n_k, uint32_t order_seed, uint32_t parked) {
	static_assert((SSX_COHORT_RECORDS & (SSX_COHORT_RECORDS - 1u)) == 0u, "fold_rank permutes a power of two");
	uint32_t* const lds_words = stage_lds<GLIBC>(a);
	Lds L; L.w = lds_words;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t wave_slot = blockIdx.x * 4u + wave; // = the tile
	if (wave_slot >= n_tiles) return;
	uint32_t* const cnt = lds_words + a.blob_words + wave * SSX_WAVE_COUNTER_WORDS; // the wave's hand-over word lives behind 4 * SSX_UNIT_COHORTS counters, as in the path kernel
	const uint32_t rec_base = wave_slot * n_k * 64u;
	const uint32_t* const tile_rows = rows + (size_t)wave_slot * 64u * n_k * SSX_FOLD_ROW_WORDS;
	LogRef lg; lg.cnt = cnt; lg.wave_base = wave_slot * 2u * a.unit_cohorts;
	for (uint32_t kq = 0; kq < n_k; kq += SSX_COHORT_KS) {
		const uint32_t cohort = kq / SSX_COHORT_KS, ways = min(SSX_COHORT_KS, n_k - kq);
		for (uint32_t s = 0; s < ways; ++s) {
			const uint32_t rc = s * 64u + lane, my_rank = fold_rank(rc, order_seed);
			// slots in front of this sample's: the entries of the cohort's samples that come before it in the seed's order
			uint32_t fs0 = 0, ne0 = 0;
			for (uint32_t o = 0; o < ways * 64u; ++o) {
				if (fold_rank(o, order_seed) >= my_rank) continue;
				const uint32_t* y = tile_rows + ((size_t)(o & 63u) * n_k + kq + (o >> 6)) * SSX_FOLD_ROW_WORDS;
				const uint32_t on = min(y[SSX_FOLD_N], SSX_MAX_FRAMES);
				fs0 += on;
				for (uint32_t l = 0; l <= on; ++l) ne0 += (y[SSX_FOLD_LEVEL0 + l * SSX_FOLD_LEVEL_WORDS + SSX_FOLD_L_FLAGS] & SSX_FOLD_NEE) ? 1u : 0u;
			}
			const uint32_t* x = tile_rows + ((size_t)lane * n_k + kq + s) * SSX_FOLD_ROW_WORDS;
			const uint32_t n = min(x[SSX_FOLD_N], SSX_MAX_FRAMES), r = rec_base + (kq + s) * 64u + lane;
			uint32_t n_ne = 0;
			for (uint32_t l = 0; l <= n; ++l) n_ne += (x[SSX_FOLD_LEVEL0 + l * SSX_FOLD_LEVEL_WORDS + SSX_FOLD_L_FLAGS] & SSX_FOLD_NEE) ? 1u : 0u;
			lg.tagw = log_tag_word(cohort, 0u, a.unit_cohorts, s); // unit tag 0
			const bool turned = ((order_seed >> 7) & 1u) != 0u;
			uint32_t prev_slot = SSX_NO_SLOT, tail = 0u, ne_seen = 0u;
			for (uint32_t l = 0; l <= n; ++l) { // what path_step stores for level l, the flush for its shadow ray, and the path's end for the last level
				const uint32_t* v = x + SSX_FOLD_LEVEL0 + l * SSX_FOLD_LEVEL_WORDS;
				const uint32_t flags = v[SSX_FOLD_L_FLAGS];
				uint32_t level_word = level_word_none();
				if (flags & SSX_FOLD_EMISSION) {
					const float e[4] = { f(v[SSX_FOLD_L_EMISSION]), f(v[SSX_FOLD_L_EMISSION + 1]), f(v[SSX_FOLD_L_EMISSION + 2]), f(v[SSX_FOLD_L_EMISSION + 3]) };
					store_emission(a, lg, l, r, e);
					level_word = level_word_emission(level_word);
				}
				if (flags & SSX_FOLD_NEE) {
					const float c[4] = { f(v[SSX_FOLD_L_NEE]), f(v[SSX_FOLD_L_NEE + 1]), f(v[SSX_FOLD_L_NEE + 2]), f(v[SSX_FOLD_L_NEE + 3]) };
					const uint32_t nslot = ne0 + (turned ? n_ne - 1u - ne_seen : ne_seen);
					const uint32_t ni = nee_index(lg, nslot);
					if (NARROW) store_parked_term(a, ni, c);
					store_shadow_outcome<NARROW>(a, ni, (flags & SSX_FOLD_NEE_VISIBLE) != 0u, c[0], c[1], c[2], c[3]);
					level_word = level_word_nee(level_word, nslot);
					++ne_seen;
				}
				if (l < n) {
					const float fs[4] = { f(v[SSX_FOLD_L_FS]), f(v[SSX_FOLD_L_FS + 1]), f(v[SSX_FOLD_L_FS + 2]), f(v[SSX_FOLD_L_FS + 3]) };
					const uint32_t slot = fs0 + (turned ? n - 1u - l : l);
					store_level_entry(a, lg, slot, fs, f(v[SSX_FOLD_L_NDL]), f(v[SSX_FOLD_L_PDF]), prev_slot, level_word);
					prev_slot = slot;
				} else tail = tail_word(level_word, x[SSX_FOLD_HIT] ? 1u : 0u, n, prev_slot);
			}
			// the sample's records as the generate kernel and the path's end leave them: {camera ray, lambda_0}, {lambda_0, tail word, final stream}
			a.ray[r] = make_float4(f(x[SSX_FOLD_CAM_DIR]), f(x[SSX_FOLD_CAM_DIR + 1]), f(x[SSX_FOLD_CAM_DIR + 2]), f(x[SSX_FOLD_LAMBDA0]));
			a.st[r] = make_uint4(x[SSX_FOLD_LAMBDA0], tail, 0u, 0u);
			wave_release(cnt);
		}
	}
	// unit_fold from here on: the hand-over, then one cohort per pass
	wave_acquire(cnt);
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
	for (uint32_t kq = 0; kq < n_k; kq += SSX_COHORT_KS) {
		const uint32_t log_rec = log_region(a, wave_slot, 0u, kq / SSX_COHORT_KS);
		resolve_records<SSX_COHORT_KS, NARROW, FLUX>(L, a, rec_base + kq * 64u + lane, 64u, min(SSX_COHORT_KS, n_k - kq), log_rec * SSX_MAX_FRAMES, log_rec * SSX_MAX_LEVELS, lane, acc, parked != 0u);
	}
	// a parked unit's samples are added by the wave whose turn reaches them, in ascending k (sums_chain)
	if (parked)
		for (uint32_t kq = 0; kq < n_k; ++kq) add_staged_sample(a.rgb_mode != 0u, acc, a.ray + (rec_base + kq * 64u + lane));
	double* const px = a.accum + (size_t)wave_slot * 256u + lane;
	px[0] = acc[0]; px[64] = acc[1]; px[128] = acc[2]; px[192] = acc[3];
}
#define SSX_DEBUG_FOLD_KERNEL(name, narrow, glibc, flux) \
	extern "C" __global__ void __launch_bounds__(256) name(SsxKernelArgs a, const uint32_t* rows, uint32_t n_tiles, uint32_t n_k, uint32_t order_seed, uint32_t parked) { \
		debug_fold_body<narrow, glibc, flux>(a, rows, n_tiles, n_k, order_seed, parked); \
	}
SSX_DEBUG_FOLD_KERNEL(ssx_debug_fold_kernel, false, false, false)
SSX_DEBUG_FOLD_KERNEL(ssx_debug_fold_kernel_nq, true, false, false)
SSX_DEBUG_FOLD_KERNEL(ssx_debug_fold_kernel_glibc, false, true, false)
SSX_DEBUG_FOLD_KERNEL(ssx_debug_fold_kernel_nq_glibc, true, true, false)
SSX_DEBUG_FOLD_KERNEL(ssx_debug_fold_kernel_flux, false, false, true)
SSX_DEBUG_FOLD_KERNEL(ssx_debug_fold_kernel_nq_flux, true, false, true)
#undef SSX_DEBUG_FOLD_KERNEL

// ssx_debug_step (include/ssx.h): one iteration of render_body's loop per round, on paths the caller supplies -- a row is a lane's Path in front of step (4).
// One wave per tile; round k is sample k of the tile's 64 pixels, so rec_index, the tag word (log_tag_word), the cohort's counters and its log region
// (LogRef, log_region) are what a render's refill hands a lane.  Per round, in render_body's order: (4) trace<TOPO> with every lane taking part, a miss ends the
// path, a hit takes hit_st only where the quad's albedo is a texture; (1) path_step<NARROW, TOPO != 1, GLIBC> -- the instance the render kernel of this
// topology runs: BLACK compiled out of the Cornell topology's -- and the end of a path that does not continue (end_path's statement: tail_word, the final
// stream, wave_release); sq.count += popc(ballot(pushed)); (2) the flush loop of render_body's flush_fold (restated below), with drain only after the last round.
// Then the hand-over as the fold begins it (wave_acquire, unit_fold's two fences) and the read-back THROUGH WHAT THE FOLD READS: the tail word of an ended
// path (a.st[r].y, decoded as resolve_records decodes it), the entry of a continued one (log_fs, log_np, log_link at its slot), log_direct at the fold's
// index, nee_term<NARROW>.  LDS as a path kernel's workgroup: [coefficients][blob][4 queues][4 x counters].
// Topology 3 has no twin here: its path_step is the BLACK = true instance TOPO 0 and 2 run, its trace is ssx_debug_trace_jit's (SSX_DBG_TRACE_TOPO).
template <int TOPO, bool NARROW, bool GLIBC>
__device__ __forceinline__ void debug_step_body(const SsxKernelArgs& a, const uint32_t* rows, uint32_t n_tiles, uint32_t n_k, uint32_t* out) {
	uint32_t* const lds_words = stage_lds<GLIBC>(a);
	Lds L; L.w = lds_words;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t wave_slot = blockIdx.x * 4u + wave; // = the tile
	if (wave_slot >= n_tiles) return;
	constexpr uint32_t queue_words = SSX_QUEUE_ENTRIES * (NARROW ? SSX_QUEUE_WORDS_NARROW : SSX_QUEUE_WORDS_WIDE);
	uint32_t* const log_cnt = lds_words + a.blob_words + 4u * queue_words + wave * SSX_WAVE_COUNTER_WORDS;
	if (lane < SSX_WAVE_COUNTER_WORDS) log_cnt[lane] = 0u; // the logs of the unit's cohorts are empty (rotate_fetch)
	SsxTimer tm;
	ShadowQ sq;
	sq.e = reinterpret_cast<float4*>(lds_words + a.blob_words + wave * queue_words);
	sq.count = 0; sq.cnt = log_cnt;
	const uint32_t rec_base = wave_slot * n_k * 64u;
	for (uint32_t k = 0; k < n_k; ++k) {
		const uint32_t r = rec_base + k * 64u + lane;
		const uint32_t* x = rows + (size_t)r * SSX_STEP_ROW_WORDS;
		uint32_t* o = out + (size_t)r * SSX_STEP_OUT_WORDS;
		Path p;
		p.orig = mk(f(x[SSX_STEP_R_ORIG]), f(x[SSX_STEP_R_ORIG + 1]), f(x[SSX_STEP_R_ORIG + 2]));
		p.dir = mk(f(x[SSX_STEP_R_DIR]), f(x[SSX_STEP_R_DIR + 1]), f(x[SSX_STEP_R_DIR + 2]));
		p.ignore = (int)x[SSX_STEP_R_IGNORE]; p.depth = x[SSX_STEP_R_DEPTH]; p.lambda_0 = f(x[SSX_STEP_R_LAMBDA0]);
		p.rng = load_rng(x + SSX_STEP_R_RNG);
		p.prev_slot = x[SSX_STEP_R_PREV_SLOT];
		p.rec_index = r;
		LogRef lg;
		lg.cnt = log_cnt; lg.wave_base = wave_slot * 2u * a.unit_cohorts; lg.tagw = log_tag_word(k / SSX_COHORT_KS, 0u, a.unit_cohorts, k % SSX_COHORT_KS); // unit tag 0
		bool active = true;
		auto end_path = [&](uint32_t level_word, uint32_t hit_anything) { // render_body's, word for word
			const uint32_t tail = tail_word(level_word, hit_anything, p.depth, p.prev_slot);
			a.st[p.rec_index] = make_uint4(__float_as_uint(p.lambda_0), tail, (uint32_t)p.rng.state, (uint32_t)(p.rng.state >> 32));
			wave_release(log_cnt);
			active = false;
		};
		// (4)
		HitInfo hit;
		trace<TOPO>(L, p.orig, p.dir, p.ignore, true, hit);
		p.hit_tri = hit.tri; p.hit_dist = hit.dist;
		float st_x = 0.0f, st_y = 0.0f;
		if (hit.tri < 0) end_path(level_word_none(), p.depth ? 1u : 0u);
		else {
			const SsxBlobQuad& Q = L.quad((uint32_t)hit.tri >> 1);
			if (Q.albedo_mode != 0u) hit_st(Q, (uint32_t)hit.tri & 1u, hit, st_x, st_y);
		}
		p.hit_st_x = st_x; p.hit_st_y = st_y;
		o[SSX_STEP_O_HIT_TRI] = (uint32_t)hit.tri; o[SSX_STEP_O_HIT_DIST] = u(hit.dist); o[SSX_STEP_O_HIT_ST] = u(st_x); o[SSX_STEP_O_HIT_ST + 1] = u(st_y);
		// (1)
		bool pushed = false, cont = false;
		if (active) {
			uint32_t level_word;
			cont = path_step<NARROW, TOPO != 1, GLIBC>(L, sq, a, lg, p, pushed, level_word);
			if (!cont) end_path(level_word, 1u);
		}
		sq.count += (uint32_t)__popcll(__ballot(pushed));
		// the lane's path as the next iteration would find it
		o[SSX_STEP_O_FLAGS] = (hit.tri >= 0 ? SSX_STEP_HIT : 0u) | (cont ? SSX_STEP_CONTINUED : 0u);
		o[SSX_STEP_O_NEXT_ORIG] = u(p.orig.x); o[SSX_STEP_O_NEXT_ORIG + 1] = u(p.orig.y); o[SSX_STEP_O_NEXT_ORIG + 2] = u(p.orig.z);
		o[SSX_STEP_O_NEXT_DIR] = u(p.dir.x); o[SSX_STEP_O_NEXT_DIR + 1] = u(p.dir.y); o[SSX_STEP_O_NEXT_DIR + 2] = u(p.dir.z);
		o[SSX_STEP_O_NEXT_IGNORE] = (uint32_t)p.ignore; o[SSX_STEP_O_NEXT_DEPTH] = p.depth;
		o[SSX_STEP_O_RNG] = (uint32_t)p.rng.state; o[SSX_STEP_O_RNG + 1] = (uint32_t)(p.rng.state >> 32);
		o[SSX_STEP_O_SLOT] = cont ? p.prev_slot : SSX_NO_SLOT;
		// (2) the flush loop of render_body's flush_fold (csrc/ssx_kernels.hip), RESTATED: calling one function from both changed the code objects of all 19 path
		// kernels (same instruction counts, other instructions: profiles/r26/NOTES.md), and those stay as they are.  Keep the two loops the same.
		const bool drain = k + 1u == n_k;
		while (sq.count >= SSX_SQ_FLUSH_AT || (drain && sq.count)) {
			const uint32_t take = min(sq.count, 64u);
			sq.count -= take;
			shadow_flush<TOPO, NARROW>(L, a, sq, sq.count, take, tm);
		}
	}
	// the fold's side from here on
	wave_acquire(log_cnt);
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	for (uint32_t k = 0; k < n_k; ++k) {
		const uint32_t r = rec_base + k * 64u + lane, s = k % SSX_COHORT_KS;
		const uint32_t* x = rows + (size_t)r * SSX_STEP_ROW_WORDS;
		uint32_t* o = out + (size_t)r * SSX_STEP_OUT_WORDS;
		const uint32_t log_rec = log_region(a, wave_slot, 0u, k / SSX_COHORT_KS), fs_base = log_rec * SSX_MAX_FRAMES, nee_base = log_rec * SSX_MAX_LEVELS;
		uint32_t flags = o[SSX_STEP_O_FLAGS], ns, depth, has_em;
		const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		float4 F = zero4; float2 NP = make_float2(0.0f, 0.0f);
		uint32_t prev = 0u, tail_depth = 0u, tail_hit = 0u;
		if (flags & SSX_STEP_CONTINUED) { // the level's entry, as the level pass of resolve_records reads it
			const uint32_t i = fs_base + o[SSX_STEP_O_SLOT];
			F = log_fs(a, i); NP = log_np(a, i);
			const uint32_t K = log_link(a, i);
			prev = K & SSX_NO_SLOT; ns = (K >> 13) & SSX_NO_SLOT; has_em = (K >> 26) & 1u;
			depth = x[SSX_STEP_R_DEPTH];
		} else { // the tail word, as its first loop does
			const uint4 rec = a.st[r];
			const uint32_t y = rec.y;
			tail_depth = depth = (y >> 2) & 0xFu; tail_hit = y & 1u;
			prev = (y >> 6) & SSX_NO_SLOT; ns = y >> 19; has_em = (y >> 1) & 1u;
			o[SSX_STEP_O_RNG] = rec.z; o[SSX_STEP_O_RNG + 1] = rec.w; // the sample's final stream, where the path's end left it
		}
		const float4 em = has_em ? log_direct(a, nee_base + depth * SSX_COHORT_RECORDS + lane + s * 64u) : zero4;
		const bool parked = ns != SSX_NO_SLOT;
		const float4 raw = parked ? log_nee(a, nee_base + ns) : zero4;
		const float4 ne = nee_term<NARROW>(a, nee_base + ns, parked);
		// visible: the visibility byte (narrow entries); wide entries hold the finished term, and a parked term is never four zeros
		const bool visible = parked && (NARROW ? log_vis(a, nee_base + ns) != 0 : (raw.x != 0.0f || raw.y != 0.0f || raw.z != 0.0f || raw.w != 0.0f));
		flags |= (has_em ? SSX_STEP_EMISSION : 0u) | (parked ? SSX_STEP_PARKED : 0u) | (visible ? SSX_STEP_VISIBLE : 0u);
		o[SSX_STEP_O_FLAGS] = flags;
		o[SSX_STEP_O_EMISSION] = u(em.x); o[SSX_STEP_O_EMISSION + 1] = u(em.y); o[SSX_STEP_O_EMISSION + 2] = u(em.z); o[SSX_STEP_O_EMISSION + 3] = u(em.w);
		o[SSX_STEP_O_NEE] = u(raw.x); o[SSX_STEP_O_NEE + 1] = u(raw.y); o[SSX_STEP_O_NEE + 2] = u(raw.z); o[SSX_STEP_O_NEE + 3] = u(raw.w);
		o[SSX_STEP_O_NEE_TERM] = u(ne.x); o[SSX_STEP_O_NEE_TERM + 1] = u(ne.y); o[SSX_STEP_O_NEE_TERM + 2] = u(ne.z); o[SSX_STEP_O_NEE_TERM + 3] = u(ne.w);
		o[SSX_STEP_O_FS] = u(F.x); o[SSX_STEP_O_FS + 1] = u(F.y); o[SSX_STEP_O_FS + 2] = u(F.z); o[SSX_STEP_O_FS + 3] = u(F.w);
		o[SSX_STEP_O_NDL] = u(NP.x); o[SSX_STEP_O_PDF] = u(NP.y);
		o[SSX_STEP_O_PREV_SLOT] = prev; o[SSX_STEP_O_TAIL_DEPTH] = tail_depth; o[SSX_STEP_O_TAIL_HIT] = tail_hit;
	}
}
#define SSX_DEBUG_STEP_KERNEL(name, topo, narrow, glibc) \
	extern "C" __global__ void __launch_bounds__(256) name(SsxKernelArgs a, const uint32_t* rows, uint32_t n_tiles, uint32_t n_k, uint32_t* out) { \
		debug_step_body<topo, narrow, glibc>(a, rows, n_tiles, n_k, out); \
	}
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel, 0, false, false)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_nq, 0, true, false)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_cornell, 1, false, false)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_cornell_nq, 1, true, false)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_plane, 2, false, false)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_plane_nq, 2, true, false)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_glibc, 0, false, true)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_nq_glibc, 0, true, true)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_cornell_glibc, 1, false, true)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_cornell_nq_glibc, 1, true, true)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_plane_glibc, 2, false, true)
SSX_DEBUG_STEP_KERNEL(ssx_debug_step_kernel_plane_nq_glibc, 2, true, true)
#undef SSX_DEBUG_STEP_KERNEL

// ---- libm = glibc-2.35: the same diagnostics for the _glibc kernels, in kernels of their own (they stage the LDS table of the _glibc
// kernels, stage_lds<true>: the glibc coefficients over ssx_fmath.h's arc-cosine slots)
// Digest word of one input and its result (include/ssx.h SSX_SWEEP_GLIBC_*; tests/glibc_math_check.c computes the same on the host).
__device__ __forceinline__ unsigned long long glibc_digest_word(uint32_t x, float y) {
	unsigned long long z = ((unsigned long long)x << 32) | (y != y ? 0x7FC00000u : __float_as_uint(y));
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
extern "C" __global__ void __launch_bounds__(256) ssx_debug_sweep_glibc_kernel(SsxKernelArgs a, uint32_t op, uint32_t lo, uint64_t count, unsigned long long* res) {
	Lds L; L.w = stage_lds<true>(a);
	(void)L;
	unsigned long long bad = 0, digest = 0;
	uint32_t example = 0; bool have_example = false;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t bits = lo + (uint32_t)i;
		const float x = __uint_as_float(bits);
		bool ok = true;
		switch (op) {
		case SSX_SWEEP_GLIBC_SIN: case SSX_SWEEP_GLIBC_COS: {
			const bool c = op == SSX_SWEEP_GLIBC_COS;
			const float y = c ? ssx_glibc_cosf(x) : ssx_glibc_sinf(x);
			float s2, c2;
			ssx_glibc_sincosf(x, &s2, &c2);
			ok = same_float(c ? c2 : s2, y);
			digest += glibc_digest_word(bits, y);
			break;
		}
		case SSX_SWEEP_GLIBC_ACOS: digest += glibc_digest_word(bits, ssx_glibc_acosf(x)); break;
		case SSX_SWEEP_GLIBC_COS_LDS: ok = same_float(ssx_cosf_lds(x), ssx_cosf(x)); break;
		default: break;
		}
		if (!ok) { ++bad; if (!have_example) { example = bits; have_example = true; } }
	}
	if (bad) {
		atomicAdd(&res[0], bad);
		const unsigned long long slot = atomicAdd(&res[2], 1ull);
		if (slot < 8ull) res[3 + slot] = example;
	}
	if (digest) atomicAdd(&res[1], digest);
}

extern "C" __global__ void __launch_bounds__(256) ssx_debug_eval_glibc_kernel(SsxKernelArgs a, uint32_t op, const uint32_t* in, uint32_t in_words,
                                                                             uint32_t* out, uint32_t out_words, uint32_t n) {
	Lds L; L.w = stage_lds<true>(a);
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t item = gid < n ? gid : n - 1u;
	const uint32_t* x = in + (size_t)item * in_words;
	uint32_t o[12];
#pragma unroll
	for (int k = 0; k < 12; ++k) o[k] = 0u;
	switch (op) {
	case SSX_DBG_GLIBC_MATH: { // in: x -> sinf, cosf, acosf, sincosf.s, sincosf.c
		float s, c;
		ssx_glibc_sincosf(f(x[0]), &s, &c);
		o[0] = u(ssx_glibc_sinf(f(x[0]))); o[1] = u(ssx_glibc_cosf(f(x[0]))); o[2] = u(ssx_glibc_acosf(f(x[0]))); o[3] = u(s); o[4] = u(c);
		break;
	}
	case SSX_DBG_SPHTRI_GLIBC: {
		SphTri t;
		sphtri_make<true>(mk(f(x[0]), f(x[1]), f(x[2])), mk(f(x[3]), f(x[4]), f(x[5])), mk(f(x[6]), f(x[7]), f(x[8])), t);
		o[0] = u(t.b); o[1] = u(t.cos_c); o[2] = u(t.alpha); o[3] = u(t.cos_alpha); o[4] = u(t.area);
		break;
	}
	case SSX_DBG_ARVO_GLIBC: {
		SphTri t;
		t.A = mk(f(x[0]), f(x[1]), f(x[2])); t.B = mk(f(x[3]), f(x[4]), f(x[5])); t.C = mk(f(x[6]), f(x[7]), f(x[8]));
		t.b = f(x[9]); t.cos_c = f(x[10]); t.alpha = f(x[11]); t.cos_alpha = f(x[12]); t.area = f(x[13]);
		t.sin_alpha = ssx_glibc_sinf(t.alpha); // (what sphtri_make<true> stores: random.cpp:108)
		Rng r = load_rng(x + 14);
		V3 d = rand_toward_sphericaltri<true>(r, t);
		o[0] = u(d.x); o[1] = u(d.y); o[2] = u(d.z); o[3] = (uint32_t)r.state; o[4] = (uint32_t)(r.state >> 32);
		break;
	}
	case SSX_DBG_SAMPLE_LIGHT_GLIBC: {
		Rng r = load_rng(x + 3);
		V3 d; uint32_t lq; float pdf;
		sample_light<true>(L, r, mk(f(x[0]), f(x[1]), f(x[2])), d, lq, pdf);
		o[0] = u(d.x); o[1] = u(d.y); o[2] = u(d.z); o[3] = lq; o[4] = u(pdf); o[5] = (uint32_t)r.state; o[6] = (uint32_t)(r.state >> 32);
		break;
	}
	case SSX_DBG_COSHEMI_GLIBC: {
		Rng r = load_rng(x + 3);
		float pdf;
		V3 w = get_rotated_to(rand_coshemi<true>(r, pdf), mk(f(x[0]), f(x[1]), f(x[2])));
		o[0] = u(w.x); o[1] = u(w.y); o[2] = u(w.z); o[3] = u(pdf); o[4] = (uint32_t)r.state; o[5] = (uint32_t)(r.state >> 32);
		break;
	}
	default: break;
	}
	if (gid < n)
		for (uint32_t k = 0; k < out_words && k < 12u; ++k) out[(size_t)gid * out_words + k] = o[k];
}

// ssx_display.hip -- finishing a development for a display (include/ssx.h, "Finishing a development for a display"): METER counts an image's channels and its
// luminance into histograms of sixteen keys per octave, LOCAL makes a per-pixel gain from a self-guided filter of the integer log-luminance, TONE applies channel
// gains, a matrix and the caller's curve table.  Part of ssx_api.hip's translation unit, behind ssx_spectral.hip (carve) and ssx_denoise.hip (blocks_of,
// denoise_check_size).  Four kernels (LOCAL's two are each compiled for their first and second pass).  Every product is rounded before its add (the build's
// -ffp-contract=off); / is the compiler's correctly rounded division; no log, exp or pow.  A lane writes only its own output; the only atomics are integer adds.
//
// METER.  4 x 4096 counters are 64 KB, all a workgroup may allocate, and would leave two workgroups per CU.  Instead a workgroup counts ONE quantity (blockIdx.y)
// of 2048 pixels into 4096 + 4 counters, 16 KB: eight workgroups, 32 waves per CU.  The price is that the image is read four times -- three megabytes at 512^2,
// from the caches after the first -- against a flush (4100 counters read and cleared per workgroup) that is as long either way.  CONTENTION: a Cornell wall puts
// most lanes of a wave on one or two keys, and an LDS atomic takes its lanes' equal addresses one after the other, 64 turns for a flat wall.  So equal keys are
// counted in the wave before the atomic: the first live lane's key goes to all (v_readlane), a ballot counts the lanes that hold it, that lane adds the count,
// they retire; TWO such rounds, then whoever is left adds 1 for itself.  Two because that is what a wall and its edge hold; bounded because a wave of 64 distinct
// keys would otherwise take 64 rounds where 64 lanes' atomics on 64 addresses take one instruction.  A round is a handful of scalar and VALU operations, so the
// worst case (no two keys equal) pays two rounds for nothing, about a tenth of the loop.  Counts are integers: any order gives the same numbers.  The flush adds
// the non-zero counters only (integer global atomics): a rendered image fills a few hundred of 4096.
//
// LOCAL.  Every sum is taken from 0.0f in ascending order, so there is no running window: a lane adds its own 2 r + 1 values, and the kernels are LDS-bound at
// r = 32, launch-bound at r = 4 (profiles/r32/NOTES.md).  ROWS: a workgroup takes 64 x 4 pixels, one lane each, and stages 64 + 2 r values per row and plane
// (pitch 128), the column clamped while staging; the first pass makes L from the image here (and writes it), and squares it while summing, so it stages one plane.
// COLUMNS: a workgroup takes 64 x 16 pixels, four rows per lane (rows lq, lq + 4, ...), and stages 16 + 2 r rows of 64 for both planes, the row clamped while
// staging: 40 KB at r = 32 (statically: three workgroups per CU; the kernel is short of lanes, not of LDS, at the sizes a finish sees).  The pointwise m, v, a, b
// end the first column pass, base, Lo and the gain the second.  BANKS, from the rule (ds_read_b32 and ds_write_b32: two groups of 32 lanes, bank = word address
// mod 32): in both kernels a group of 32 lanes is 32 consecutive columns of one staged row and reads, at every step of its sum, 32 consecutive words: 32 banks, no
// conflicts, whatever the pitch.  The staging writes consecutive words from consecutive lanes.
//
// TONE.  One lane per pixel, 12 bytes in (16 with a local gain), 12 out.  The table is read by a per-lane index.  It stays in global memory and comes through the
// caches: the finish's own table is 258 floats (a kilobyte: sixteen lines), the largest one allowed 64 KB.  LDS would need the table staged per workgroup -- a
// kilobyte per 256 pixels is a third on top of the 3 KB those pixels move, and 64 KB would be one workgroup per CU -- and would not read better: by the rule a
// ds_read_b32 conflicts where lanes of a group hold DIFFERENT words on one bank, which is what a gather by value does whenever a group's pixels spread over more
// than 32 nodes.  Through the caches a wave's load costs one pass per distinct line, and neighbouring pixels fall on neighbouring nodes: a smooth region reads one or
// two lines per load.  idx + 1 is the next word, the same line fifteen times in sixteen.

#define SSX_METER_LANES 256u
#define SSX_METER_PER_LANE 8u
#define SSX_METER_SLOTS (SSX_METER_KEYS + 4u)               // a quantity's keys, then its four special classes
#define SSX_LOCAL_LANES 256u
#define SSX_LOCAL_TX 64u
#define SSX_LOCAL_ROWS_TY 4u
#define SSX_LOCAL_SW (SSX_LOCAL_TX + 2u * SSX_LOCAL_MAX_RADIUS)      // 128: the rows kernel's staged pitch
#define SSX_LOCAL_COLS_TY 16u
#define SSX_LOCAL_SH (SSX_LOCAL_COLS_TY + 2u * SSX_LOCAL_MAX_RADIUS) // 80: the columns kernel's staged rows

struct SsxMeterArgs {
	const float* img;         // [pixels][3]
	const uint8_t* mask;      // [pixels], or nullptr
	uint32_t* hist;           // [4][SSX_METER_KEYS], zeroed
	uint32_t* special;        // [4][4], zeroed
	uint32_t pixels;
	float luma[3];
};

struct SsxLocalArgs {
	const float* img;         // rows, first pass: [pixels][3]
	const float* p0;          // the two planes read: rows, second pass: a, b; columns: the row sums
	const float* p1;
	const float* L;           // columns, second pass
	float* o0;                // rows: the row sums; columns, first pass: a, b; second: gain, base (or nullptr)
	float* o1;
	float* oL;                // rows, first pass: L
	uint32_t width, height, tiles_x, r;
	float luma[3], exposure, y_lo, y_hi, n, eps, pivot, compress, boost;
};

struct SsxToneArgs {
	const float* img;         // [pixels][3]
	const float* local;       // [pixels], or nullptr
	const float* curve;       // [curve_len]
	float* out;               // [pixels][3]
	uint32_t pixels, shift, lo_bits;
	float lo, hi, unit;       // unit = 2^-shift
	float gains[3], matrix[9];
};

__device__ __forceinline__ float display_luminance(const float* x, const float* luma) { return ((0.0f + x[0] * luma[0]) + x[1] * luma[1]) + x[2] * luma[2]; }

// the counter of a value: its key, or SSX_METER_KEYS + the special class
__device__ __forceinline__ uint32_t meter_slot(float x) {
	const uint32_t u = __float_as_uint(x), m = u & 0x7FFFFFFFu;
	if (m == 0u) return SSX_METER_KEYS;
	if (m > 0x7F800000u) return SSX_METER_KEYS + 3u;
	if (u >> 31) return SSX_METER_KEYS + 1u;
	if (u == 0x7F800000u) return SSX_METER_KEYS + 2u;
	return u >> 19;
}

// h[slot] += 1 for every live lane; called by all lanes of the wave together
__device__ __forceinline__ void meter_add(uint32_t* h, uint32_t slot, bool live) {
#pragma unroll
	for (int round = 0; round < 2; ++round) {
		const uint64_t todo = __ballot(live);
		if (todo) { // (uniform)
			const uint32_t leader = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__ffsll((long long)todo) - 1));
			const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, (int)leader);
			const bool same = live && slot == s0;
			const uint32_t count = (uint32_t)__popcll(__ballot(same));
			if ((threadIdx.x & 63u) == leader) atomicAdd(&h[s0], count);
			live = live && !same;
		}
	}
	if (live) atomicAdd(&h[slot], 1u);
}

// blockIdx.x = chunk of SSX_METER_LANES * SSX_METER_PER_LANE pixels, blockIdx.y = quantity
extern "C" __global__ void __launch_bounds__(SSX_METER_LANES) ssx_meter_kernel(SsxMeterArgs a) {
	__shared__ uint32_t h[SSX_METER_SLOTS];
	const uint32_t t = threadIdx.x, k = blockIdx.y;
	for (uint32_t s = t; s < SSX_METER_SLOTS; s += SSX_METER_LANES) h[s] = 0u;
	__syncthreads();
	const uint32_t first = blockIdx.x * (SSX_METER_LANES * SSX_METER_PER_LANE);   // < 2^28
	for (uint32_t it = 0; it < SSX_METER_PER_LANE; ++it) {
		const uint32_t p = first + it * SSX_METER_LANES + t;
		const bool live = p < a.pixels && (!a.mask || a.mask[p] != 0u);
		uint32_t slot = 0u;
		if (live) {
			const float* const x = a.img + (size_t)p * 3u;
			slot = meter_slot(k < 3u ? x[k] : display_luminance(x, a.luma));
		}
		meter_add(h, slot, live);
	}
	__syncthreads();
	for (uint32_t s = t; s < SSX_METER_SLOTS; s += SSX_METER_LANES) {
		const uint32_t n = h[s];
		if (n) atomicAdd(s < SSX_METER_KEYS ? a.hist + k * SSX_METER_KEYS + s : a.special + k * 4u + (s - SSX_METER_KEYS), n);
	}
}

// L of the header for one pixel
__device__ __forceinline__ float local_log(const SsxLocalArgs& a, const float* x) {
	float yc = display_luminance(x, a.luma) * a.exposure;
	yc = yc > a.y_lo ? yc : a.y_lo;
	yc = yc < a.y_hi ? yc : a.y_hi;
	return (float)((int32_t)(__float_as_uint(yc) >> 7) - 8323072) * 0x1p-16f;
}

// E(d) of the header
__device__ __forceinline__ float local_exp(float d) {
	float f = floorf(d * 65536.0f);
	f = f > -16777216.0f ? f : -16777216.0f;
	f = f < 16777216.0f ? f : 16777216.0f;
	int32_t key = (int32_t)f + 8323072;
	key = key > 0x10000 ? key : 0x10000;
	key = key < 0xFEFFFF ? key : 0xFEFFFF;
	return __uint_as_float((uint32_t)key << 7);
}

__device__ __forceinline__ int local_clamp(int k, int n) { return k < 0 ? 0 : (k >= n ? n - 1 : k); }

// blockIdx.x = tile_y * tiles_x + tile_x, a tile 64 x 4 pixels
template <bool FIRST> __device__ __forceinline__ void local_rows(const SsxLocalArgs& a) {
	__shared__ float s0[SSX_LOCAL_ROWS_TY * SSX_LOCAL_SW];
	__shared__ float s1[FIRST ? 1u : SSX_LOCAL_ROWS_TY * SSX_LOCAL_SW];
	const uint32_t t = threadIdx.x, r = a.r, sw = SSX_LOCAL_TX + 2u * r;
	const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
	const uint32_t x0 = tx * SSX_LOCAL_TX, y0 = ty * SSX_LOCAL_ROWS_TY;
	for (uint32_t idx = t; idx < SSX_LOCAL_ROWS_TY * sw; idx += SSX_LOCAL_LANES) {
		const uint32_t row = idx / sw, sx = idx - row * sw, gy = y0 + row;
		float v0 = 0.0f, v1 = 0.0f;
		if (gy < a.height) {
			const uint32_t p = gy * a.width + (uint32_t)local_clamp((int)x0 + (int)sx - (int)r, (int)a.width);
			if (FIRST) v0 = local_log(a, a.img + (size_t)p * 3u);
			else { v0 = a.p0[p]; v1 = a.p1[p]; }
		}
		s0[row * SSX_LOCAL_SW + sx] = v0;
		if (!FIRST) s1[row * SSX_LOCAL_SW + sx] = v1;
	}
	__syncthreads();
	const uint32_t lx = t & (SSX_LOCAL_TX - 1u), ly = t / SSX_LOCAL_TX, gx = x0 + lx, gy = y0 + ly;
	if (gx >= a.width || gy >= a.height) return;
	const float* const w0 = s0 + ly * SSX_LOCAL_SW + lx;
	const float* const w1 = s1 + (FIRST ? 0u : ly * SSX_LOCAL_SW + lx);
	float h0 = 0.0f, h1 = 0.0f;
	for (uint32_t k = 0; k <= 2u * r; ++k) {
		const float v = w0[k];
		h0 = h0 + v;
		h1 = h1 + (FIRST ? v * v : w1[k]);
	}
	const uint32_t p = gy * a.width + gx;
	a.o0[p] = h0;
	a.o1[p] = h1;
	if (FIRST) a.oL[p] = w0[r];
}

// blockIdx.x = tile_y * tiles_x + tile_x, a tile 64 x 16 pixels
template <bool FIRST> __device__ __forceinline__ void local_columns(const SsxLocalArgs& a) {
	__shared__ float s0[SSX_LOCAL_SH * SSX_LOCAL_TX];
	__shared__ float s1[SSX_LOCAL_SH * SSX_LOCAL_TX];
	const uint32_t t = threadIdx.x, r = a.r, sh = SSX_LOCAL_COLS_TY + 2u * r;
	const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
	const uint32_t x0 = tx * SSX_LOCAL_TX, y0 = ty * SSX_LOCAL_COLS_TY;
	for (uint32_t idx = t; idx < sh * SSX_LOCAL_TX; idx += SSX_LOCAL_LANES) {
		const uint32_t sy = idx / SSX_LOCAL_TX, sx = idx & (SSX_LOCAL_TX - 1u), gx = x0 + sx;
		float v0 = 0.0f, v1 = 0.0f;
		if (gx < a.width) {
			const uint32_t p = (uint32_t)local_clamp((int)y0 + (int)sy - (int)r, (int)a.height) * a.width + gx;
			v0 = a.p0[p]; v1 = a.p1[p];
		}
		s0[idx] = v0; s1[idx] = v1;
	}
	__syncthreads();
	const uint32_t lx = t & (SSX_LOCAL_TX - 1u), lq = t / SSX_LOCAL_TX, gx = x0 + lx;
	if (gx >= a.width) return;
	for (uint32_t m = 0; m < SSX_LOCAL_COLS_TY / 4u; ++m) {
		const uint32_t ly = lq + 4u * m, gy = y0 + ly;
		if (gy >= a.height) break;
		const float* const w0 = s0 + ly * SSX_LOCAL_TX + lx;
		const float* const w1 = s1 + ly * SSX_LOCAL_TX + lx;
		float c0 = 0.0f, c1 = 0.0f;
		for (uint32_t k = 0; k <= 2u * r; ++k) { c0 = c0 + w0[k * SSX_LOCAL_TX]; c1 = c1 + w1[k * SSX_LOCAL_TX]; }
		const uint32_t p = gy * a.width + gx;
		if (FIRST) {
			const float mean = c0 / a.n;
			float v = c1 / a.n - mean * mean;
			v = v > 0.0f ? v : 0.0f;
			const float ga = v / (v + a.eps);
			a.o0[p] = ga;
			a.o1[p] = mean - ga * mean;
		} else {
			const float A = c0 / a.n, Bm = c1 / a.n, L = a.L[p];
			const float base = A * L + Bm;
			const float tt = (base - a.pivot) * a.compress + a.pivot;
			const float Lo = tt + (L - base) * a.boost;
			a.o0[p] = local_exp(Lo - L);
			if (a.o1) a.o1[p] = base;
		}
	}
}

extern "C" __global__ void __launch_bounds__(SSX_LOCAL_LANES) ssx_local_rows_log_kernel(SsxLocalArgs a) { local_rows<true>(a); }
extern "C" __global__ void __launch_bounds__(SSX_LOCAL_LANES) ssx_local_rows_kernel(SsxLocalArgs a) { local_rows<false>(a); }
extern "C" __global__ void __launch_bounds__(SSX_LOCAL_LANES) ssx_local_columns_ab_kernel(SsxLocalArgs a) { local_columns<true>(a); }
extern "C" __global__ void __launch_bounds__(SSX_LOCAL_LANES) ssx_local_columns_gain_kernel(SsxLocalArgs a) { local_columns<false>(a); }

extern "C" __global__ void __launch_bounds__(256) ssx_tone_kernel(SsxToneArgs a) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= a.pixels) return;
	const float* const x = a.img + (size_t)p * 3u;
	float v[3];
#pragma unroll
	for (int c = 0; c < 3; ++c) v[c] = x[c] * a.gains[c];
	if (a.local) { // (uniform)
		const float g = a.local[p];
#pragma unroll
		for (int c = 0; c < 3; ++c) v[c] = v[c] * g;
	}
	float* const o = a.out + (size_t)p * 3u;
	const uint32_t low = (1u << a.shift) - 1u;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		float xc = ((0.0f + v[0] * a.matrix[3 * c]) + v[1] * a.matrix[3 * c + 1]) + v[2] * a.matrix[3 * c + 2];
		xc = xc > a.lo ? xc : a.lo;
		xc = xc < a.hi ? xc : a.hi;
		const uint32_t k = __float_as_uint(xc) - a.lo_bits, idx = k >> a.shift;   // idx + 1 < curve_len: xc lies in [lo, hi]
		const float f = (float)(k & low) * a.unit;
		const float c0 = a.curve[idx], c1 = a.curve[idx + 1u];
		o[c] = c0 + (c1 - c0) * f;
	}
}

namespace {

bool display_positive_normal(float v) { return std::isnormal(v) && v > 0.0f; }

int display_check_luma(ssx_ctx* ctx, const char* what, const float* luma) {
	if (!luma) return fail(ctx, SSX_ERR_ARG, fmt("%s: luma must not be NULL", what));
	for (int c = 0; c < 3; ++c)
		if (!std::isfinite(luma[c])) return fail(ctx, SSX_ERR_ARG, fmt("%s: luma[%d] = %g: must be finite", what, c, (double)luma[c]));
	return SSX_OK;
}

int local_take_params(ssx_ctx* ctx, const char* what, const ssx_local_params* in) {
	if (!in) return fail(ctx, SSX_ERR_ARG, fmt("%s: local must not be NULL", what));
	if (in->struct_size != sizeof(ssx_local_params)) return fail(ctx, SSX_ERR_ARG, "ssx_local_params.struct_size mismatch");
	if (in->radius < 1u || in->radius > SSX_LOCAL_MAX_RADIUS) return fail(ctx, SSX_ERR_ARG, fmt("ssx_local_params.radius = %u: must be 1..%u", in->radius, SSX_LOCAL_MAX_RADIUS));
	const struct { const char* name; float v; } finite[] = { { "exposure", in->exposure }, { "pivot", in->pivot }, { "compress", in->compress }, { "boost", in->boost } };
	for (const auto& f : finite)
		if (!std::isfinite(f.v)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_local_params.%s = %g: must be finite", f.name, (double)f.v));
	if (!display_positive_normal(in->y_lo)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_local_params.y_lo = %g: must be a positive normal number", (double)in->y_lo));
	if (!display_positive_normal(in->y_hi)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_local_params.y_hi = %g: must be a positive normal number", (double)in->y_hi));
	if (in->y_lo > in->y_hi) return fail(ctx, SSX_ERR_ARG, fmt("ssx_local_params.y_lo = %g lies above y_hi = %g", (double)in->y_lo, (double)in->y_hi));
	if (!std::isfinite(in->eps) || !(in->eps > 0.0f)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_local_params.eps = %g: must be finite and positive", (double)in->eps));
	return SSX_OK;
}

uint32_t display_bits(float v) { uint32_t u; std::memcpy(&u, &v, sizeof u); return u; }

int tone_take_params(ssx_ctx* ctx, const char* what, const ssx_tone_params* in) {
	if (!in) return fail(ctx, SSX_ERR_ARG, fmt("%s: tone must not be NULL", what));
	if (in->struct_size != sizeof(ssx_tone_params)) return fail(ctx, SSX_ERR_ARG, "ssx_tone_params.struct_size mismatch");
	if (in->shift < 12u || in->shift > 23u) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.shift = %u: must be 12..23", in->shift));
	if (!display_positive_normal(in->lo)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.lo = %g: must be a positive normal number", (double)in->lo));
	if (!display_positive_normal(in->hi)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.hi = %g: must be a positive normal number", (double)in->hi));
	if (in->lo > in->hi) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.lo = %g lies above hi = %g", (double)in->lo, (double)in->hi));
	const uint32_t len = ((display_bits(in->hi) - display_bits(in->lo)) >> in->shift) + 2u;
	if (len > SSX_TONE_MAX_CURVE) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params: lo, hi and shift ask for a curve_len of %u, above %u", len, SSX_TONE_MAX_CURVE));
	if (in->curve_len != len) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.curve_len = %u: lo, hi and shift define %u", in->curve_len, len));
	for (int c = 0; c < 3; ++c)
		if (!std::isfinite(in->gains[c])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.gains[%d] = %g: must be finite", c, (double)in->gains[c]));
	for (int k = 0; k < 9; ++k)
		if (!std::isfinite(in->matrix[k])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.matrix[%d][%d] = %g: must be finite", k / 3, k % 3, (double)in->matrix[k]));
	if (!in->curve) return fail(ctx, SSX_ERR_ARG, "ssx_tone_params: curve must not be NULL");
	for (uint32_t k = 0; k < len; ++k)
		if (!std::isfinite(in->curve[k])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_tone_params.curve[%u] = %g: must be finite", k, (double)in->curve[k]));
	return SSX_OK;
}

// LOCAL on d_img (only read), queued on the context's stream: gain, base; plane[0..4]: L and two pairs of scratch planes
int local_device(ssx_ctx* ctx, const ssx_local_params& s, const float* luma, uint32_t width, uint32_t height, const float* d_img, float* const plane[5], float* gain, float* base) {
	SsxLocalArgs a{};
	a.width = width; a.height = height; a.r = s.radius;
	a.tiles_x = (width + SSX_LOCAL_TX - 1u) / SSX_LOCAL_TX;
	for (int c = 0; c < 3; ++c) a.luma[c] = luma[c];
	a.exposure = s.exposure; a.y_lo = s.y_lo; a.y_hi = s.y_hi; a.eps = s.eps; a.pivot = s.pivot; a.compress = s.compress; a.boost = s.boost;
	a.n = (float)((2u * s.radius + 1u) * (2u * s.radius + 1u));
	const dim3 rows(a.tiles_x * ((height + SSX_LOCAL_ROWS_TY - 1u) / SSX_LOCAL_ROWS_TY));    // < 2^27: at most 2^28 pixels, a tile holds 4 rows of some
	const dim3 cols(a.tiles_x * ((height + SSX_LOCAL_COLS_TY - 1u) / SSX_LOCAL_COLS_TY));
	float* const L = plane[0];
	a.img = d_img; a.oL = L; a.o0 = plane[1]; a.o1 = plane[2];
	hipLaunchKernelGGL(ssx_local_rows_log_kernel, rows, dim3(SSX_LOCAL_LANES), 0, ctx->stream, a);
	a.p0 = plane[1]; a.p1 = plane[2]; a.o0 = plane[3]; a.o1 = plane[4];
	hipLaunchKernelGGL(ssx_local_columns_ab_kernel, cols, dim3(SSX_LOCAL_LANES), 0, ctx->stream, a);
	a.p0 = plane[3]; a.p1 = plane[4]; a.o0 = plane[1]; a.o1 = plane[2];
	hipLaunchKernelGGL(ssx_local_rows_kernel, rows, dim3(SSX_LOCAL_LANES), 0, ctx->stream, a);
	a.p0 = plane[1]; a.p1 = plane[2]; a.L = L; a.o0 = gain; a.o1 = base;
	hipLaunchKernelGGL(ssx_local_columns_gain_kernel, cols, dim3(SSX_LOCAL_LANES), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_meter_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* img, const float* luma, const uint8_t* mask, uint32_t* hist, uint32_t* special) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_meter_images";
	if (!img || !hist || !special) return fail(ctx, SSX_ERR_ARG, fmt("%s: img, hist and special must not be NULL", what));
	int rc = display_check_luma(ctx, what, luma);
	if (rc) return rc;
	if ((rc = denoise_check_size(ctx, width, height, what))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	float* d_img = nullptr; uint32_t* d_counts = nullptr; uint8_t* d_mask = nullptr;
	if ((rc = carve(ctx, ctx->d_display, [&](Carver& c) {
		d_img = c.take<float>(pixels * 3u);
		d_counts = c.take<uint32_t>(4u * SSX_METER_KEYS + 16u);
		d_mask = c.take<uint8_t>(mask ? pixels : 0u);
	}))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d_img, img, pixels * 3u * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	if (mask) SSX_HIP(ctx, hipMemcpyAsync(d_mask, mask, pixels, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemsetAsync(d_counts, 0, (4u * SSX_METER_KEYS + 16u) * sizeof(uint32_t), ctx->stream));
	SsxMeterArgs a{};
	a.img = d_img; a.mask = mask ? d_mask : nullptr; a.hist = d_counts; a.special = d_counts + 4u * SSX_METER_KEYS; a.pixels = (uint32_t)pixels;
	for (int c = 0; c < 3; ++c) a.luma[c] = luma[c];
	const uint32_t per_block = SSX_METER_LANES * SSX_METER_PER_LANE;
	hipLaunchKernelGGL(ssx_meter_kernel, dim3((uint32_t)((pixels + per_block - 1u) / per_block), 4u), dim3(SSX_METER_LANES), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(hist, d_counts, 4u * SSX_METER_KEYS * sizeof(uint32_t), hipMemcpyDeviceToHost));
	SSX_HIP(ctx, hipMemcpy(special, d_counts + 4u * SSX_METER_KEYS, 16u * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_local_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* img, const float* luma, const ssx_local_params* local, float* gain, float* base) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_local_images";
	if (!img || !gain) return fail(ctx, SSX_ERR_ARG, fmt("%s: img and gain must not be NULL", what));
	int rc = display_check_luma(ctx, what, luma);
	if (rc) return rc;
	if ((rc = local_take_params(ctx, what, local))) return rc;
	if ((rc = denoise_check_size(ctx, width, height, what))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	float* d_img = nullptr; float* plane[5] = {}; float* d_gain = nullptr; float* d_base = nullptr;
	if ((rc = carve(ctx, ctx->d_display, [&](Carver& c) {
		d_img = c.take<float>(pixels * 3u);
		for (float*& p : plane) p = c.take<float>(pixels);
		d_gain = c.take<float>(pixels);
		d_base = c.take<float>(base ? pixels : 0u);
	}))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d_img, img, pixels * 3u * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	if ((rc = local_device(ctx, *local, luma, width, height, d_img, plane, d_gain, base ? d_base : nullptr))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(gain, d_gain, pixels * sizeof(float), hipMemcpyDeviceToHost));
	if (base) SSX_HIP(ctx, hipMemcpy(base, d_base, pixels * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_tone_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* img, const float* local, const ssx_tone_params* tone, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_tone_images";
	if (!img || !out) return fail(ctx, SSX_ERR_ARG, fmt("%s: img and out must not be NULL", what));
	int rc = tone_take_params(ctx, what, tone);
	if (rc) return rc;
	if ((rc = denoise_check_size(ctx, width, height, what))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	float* d_img = nullptr; float* d_local = nullptr; float* d_curve = nullptr; float* d_out = nullptr;
	if ((rc = carve(ctx, ctx->d_display, [&](Carver& c) {
		d_img = c.take<float>(pixels * 3u);
		d_out = c.take<float>(pixels * 3u);
		d_curve = c.take<float>(tone->curve_len);
		d_local = c.take<float>(local ? pixels : 0u);
	}))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d_img, img, pixels * 3u * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	if (local) SSX_HIP(ctx, hipMemcpyAsync(d_local, local, pixels * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d_curve, tone->curve, tone->curve_len * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	SsxToneArgs a{};
	a.img = d_img; a.local = local ? d_local : nullptr; a.curve = d_curve; a.out = d_out;
	a.pixels = (uint32_t)pixels; a.shift = tone->shift; a.lo_bits = display_bits(tone->lo);
	a.lo = tone->lo; a.hi = tone->hi; a.unit = std::ldexp(1.0f, -(int)tone->shift);
	for (int c = 0; c < 3; ++c) a.gains[c] = tone->gains[c];
	for (int k = 0; k < 9; ++k) a.matrix[k] = tone->matrix[k];
	hipLaunchKernelGGL(ssx_tone_kernel, blocks_of(pixels), dim3(256), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, d_out, pixels * 3u * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

} // extern "C"

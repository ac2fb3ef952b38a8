// ssx_spectral_stats.hip -- error bars for the spectral output: a per-pixel, per-bin second moment of the hero fluxes beside the sums S, the variance of every
// bin mean, and region probes (include/ssx.h, "Spectral moments and region probes").  Part of ssx_api.hip's translation unit, behind ssx_spectral.hip (whose
// state S, N it stands next to) and ssx_denoise.hip (blocks_of, denoise_check_size).  Everything here is binary64 with IEEE + - * /, no contraction (the build's
// -ffp-contract=off), in the order the header writes: a restatement in numpy gives the same bits (tests/spectral_stats_ref.py).

// What ssx_spectral_moment_kernel needs of a launch: what ssx_spectral_bin_kernel needs (SsxSpectralArgs), with Q[tile slot][bin][pixel of the tile] in place of S
// and no counts -- they are the bin kernel's N.
struct SsxMomentArgs {
	const float4* flux; const uint4* st;
	double* Q;
	SsxPixelGrid g;
	uint32_t n_k, M;
	float lambda_min, lambda_step;
};

// The bin kernel's lane mapping: one 256-lane workgroup per owned tile slot, lane = (pixel of the tile, hero slot i), lane (pixel, i) owns the pixel's bins
// i*M .. i*M + M-1 of Q: no atomics, no barriers.  The lane's M accumulators live in LDS as [M][256] binary64 (a run-time index; lane l of a row is at
// 8-byte address l: a ds_read_b64 / ds_write_b64 is served in two groups of 32 lanes over 64 four-byte banks, and 32 consecutive 8-byte addresses cover each
// bank pair once -- conflict-free).  32 KB at 64 bins: S and Q in one kernel would need more than 64 KB, and the bin kernel stays what it was.
//     m as there;  Q[i*M + m] += (double)f[i] * (double)f[i]      (the product of two binary32 values is exact in binary64)
// in ascending k.  Lanes outside a ragged image have no records and touch nothing.
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_moment_kernel(SsxMomentArgs a) {
	extern __shared__ double moment_lds[];
	const uint32_t tid = threadIdx.x, px = tid >> 2, i = tid & 3u, slot = blockIdx.x, M = a.M;
	uint32_t tx, ty;
	(void)tile_of_slot(a.g, slot, tx, ty);
	if (tx * 8u + (px & 7u) >= a.g.width || ty * 8u + (px >> 3) >= a.g.height) return;
	double* const acc = moment_lds + tid;                                                // [m * 256]
	double* const Q = a.Q + ((size_t)slot * 4u * M + (size_t)i * M) * 64u + px;          // [m * 64]
	for (uint32_t m = 0; m < M; ++m) acc[m * 256u] = Q[m * 64u];
	const float fM = (float)M;
	size_t r = (size_t)slot * a.n_k * 64u + px;
#pragma unroll 4
	for (uint32_t kk = 0; kk < a.n_k; ++kk, r += 64u) {
		const float f = reinterpret_cast<const float*>(a.flux + r)[i], lambda_0 = __uint_as_float(a.st[r].x);
		const float t = (lambda_0 - a.lambda_min) / a.lambda_step;
		const uint32_t m = min(M - 1u, (uint32_t)(t * fM));
		const double d = (double)f;
		acc[m * 256u] += d * d;
	}
	for (uint32_t m = 0; m < M; ++m) Q[m * 64u] = acc[m * 256u];
}

// q of the header: the sum of squared deviations of a sub-bin's n >= 2 samples from their mean, from Q, S and n; negative rounding residue is 0, a NaN stays one
__device__ __forceinline__ double moment_deviations(double Q, double S, uint32_t n) {
	const double q = Q - (S * S) / (double)n;
	return (q < 0.0) ? 0.0 : q;
}

// The estimate of one cell from Q, S and n >= 2: the variance of its mean, (q / (n - 1)) / n, and -- where the caller wants it -- the mean S / n
__device__ __forceinline__ double cell_variance(double Q, double S, uint32_t n, double* mean = nullptr) {
	const double e = (moment_deviations(Q, S, n) / (double)(n - 1u)) / (double)n;
	if (mean) *mean = S / (double)n;
	return e;
}

// S, Q, N -> row-major [height][width][B] var (binary32) and Q (either may be NULL); 0 for pixels the context does not own.
//     n = N[b % M];   n < 2: var = +inf;   else var = (float)((q / (double)(n-1)) / (double)n)
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_variance_kernel(const double* S, const double* Q, const uint32_t* N, float* var, double* q_out, SsxPixelGrid g, uint32_t M) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n_px = g.width * g.height, B = 4u * M;
	if (p >= n_px) return;
	const uint32_t i = p % g.width, j = p / g.width;
	const bool own = ssx_owns_pixel(g, i, j);
	const size_t slot = ssx_shared_tile(g, i, j) / g.tile_stride, lane = (j & 7u) * 8u + (i & 7u);
	for (uint32_t b = 0; b < B; ++b) {
		float v = 0.0f; double qq = 0.0;
		if (own) {
			const size_t at = (slot * B + b) * 64u + lane;
			const uint32_t n = N[(slot * M + b % M) * 64u + lane];
			qq = Q[at];
			v = n < 2u ? __uint_as_float(0x7F800000u) : (float)cell_variance(qq, S[at], n);
		}
		if (var) var[(size_t)p * B + b] = v;
		if (q_out) q_out[(size_t)p * B + b] = qq;
	}
}

// The inverse of the variance kernel's q for the tiles this context owns (ssx_spectral_moments_import): row-major whole-image q [height][width][B] (row 0 =
// bottom; whoever exported it may have owned other tiles) -> Q[tile slot][bin][pixel of the tile].  ssx_spectral_import_kernel's geometry for one array, one
// 256-lane workgroup per owned tile slot (slot -> tile by tile_of_slot), no atomics: a workgroup writes its own slot only.
//   in:   by tile_rows_to_lds (ssx_spectral.hip), into [64 pixels][B + 1] doubles of LDS (33 KB at B = 64).
//   out:  wave w stores bins w, w + 4, ...: per bin the 64 lanes' doubles are 512 consecutive bytes.  Lanes of pixels outside the image store +0.0, what the
//         memset of a fresh render leaves there.
// The check.  On the way out lane = pixel, wave = bin: the lane that stores Q[slot][b][px] reads the context's own S[slot][b][px] and N[slot][b % M][px] where
// they lie (coalesced, 512 and 256 consecutive bytes per wave) and holds q to what ssx_spectral_moment_kernel can produce -- Q += (double)f * (double)f from
// +0.0, every product exact:
//     rule 0   n == 0 :  q is +0.0, bit for bit
//     rule 1   n == 1 :  q == S * S, or both are NaN      (S is then (double)f, its square exact; -ffp-contract=off: one multiply)
//     rule 2   n >= 2 :  !(q < 0.0)                       (a sum of squares is non-negative, or NaN)
// An owned in-image pixel that breaks rule r stores 1 into bad[r] (a plain store; every writer of a word stores the same value).  Nothing inexact is held:
// values at n >= 2 are the file's checksum's business.
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_moments_import_kernel(const double* q, const double* S, const uint32_t* N, double* Q, uint32_t* bad, SsxPixelGrid g, uint32_t M) {
	extern __shared__ double moment_lds[];
	const uint32_t tid = threadIdx.x, slot = blockIdx.x, B = 4u * M, stride = B + 1u;
	uint32_t tx, ty;
	(void)tile_of_slot(g, slot, tx, ty);
	const uint32_t i0 = tx * 8u, j0 = ty * 8u, cols = min(8u, g.width - i0), rows = min(8u, g.height - j0);
	tile_rows_to_lds(q, moment_lds, g.width, i0, j0, cols, rows, B);
	__syncthreads();
	const uint32_t px = tid & 63u, w = tid >> 6;
	const bool inside = (px & 7u) < cols && (px >> 3) < rows;
	const size_t at0 = (size_t)slot * B * 64u + px;
	const uint32_t* const Np = N + (size_t)slot * M * 64u + px;
	for (uint32_t b = w; b < B; b += 4u) {
		const size_t at = at0 + (size_t)b * 64u;
		double v = 0.0;
		if (inside) {
			v = moment_lds[px * stride + b];
			const uint32_t n = Np[(size_t)(b % M) * 64u];
			if (n == 0u) { if (__double_as_longlong(v) != 0ll) bad[0] = 1u; }
			else if (n == 1u) { const double s = S[at], ss = s * s; if (!(v == ss) && !(v != v && ss != ss)) bad[1] = 1u; }
			else if (v < 0.0) bad[2] = 1u;
		}
		Q[at] = v;
	}
}

// Region probes on row-major device arrays: sums and q [height][width][B], counts [height][width][M], labels [height][width] (0..R-1, or 255: no region).
// Stage 1: one workgroup per image row and half h of the quantities (h = 0: SS | NN, h = 1: VV | UU), 2 B lanes, lane = (quantity, bin): the B lanes of a
// quantity read B consecutive elements of a pixel.  The pixel's label is a run-time index, so the accumulators live in LDS, [R][2 B] eight-byte words (lane l of a
// row at 8-byte address l: conflict-free, as above; 32 KB at R = 32, B = 64), each lane its own column: no atomics, no barriers.  The workgroup walks the row in
// ascending i, from +0.0 / 0, and writes its partials part[j][r][quantity 0..3][B]; a region without a pixel in the row leaves its +0.0.
struct SsxProbeArgs {
	const double* sums; const double* q; const uint32_t* counts; const uint8_t* labels;
	uint64_t* part;   // [height][R][4][B]: SS, NN, VV, UU -- binary64 or uint64 by quantity
	uint64_t* out;    // [4][R][B]
	uint32_t width, height, B, R;
};

extern "C" __global__ void __launch_bounds__(128) ssx_probe_rows_kernel(SsxProbeArgs a) {
	extern __shared__ uint64_t probe_lds[];
	const uint32_t t = threadIdx.x, B = a.B, M = B / 4u, j = blockIdx.x, half = blockIdx.y, second = t / B, b = t - second * B, lanes = 2u * B;
	uint64_t* const acc = probe_lds + t;                                                 // [r * lanes]
	for (uint32_t r = 0; r < a.R; ++r) acc[r * lanes] = 0ull;
	const size_t row = (size_t)j * a.width;
	for (uint32_t i = 0; i < a.width; ++i) {
		const uint32_t r = a.labels[row + i];
		if (r >= a.R) continue;                                                          // 255: no region (other values never get here: the host refuses them)
		const size_t p = row + i;
		const uint32_t n = a.counts[p * M + b % M];
		uint64_t* const at = acc + r * lanes;
		if (second) *at += (half == 0u) ? (uint64_t)n : (n < 2u ? (uint64_t)n : 0ull);   // NN | UU
		else if (half == 0u) *reinterpret_cast<double*>(at) += a.sums[p * B + b];        // SS
		else if (n >= 2u) *reinterpret_cast<double*>(at) += (moment_deviations(a.q[p * B + b], a.sums[p * B + b], n) / (double)(n - 1u)) * (double)n; // VV
	}
	const uint32_t quantity = half * 2u + second;                                        // 0 SS, 1 NN, 2 VV, 3 UU
	for (uint32_t r = 0; r < a.R; ++r) a.part[(((size_t)j * a.R + r) * 4u + quantity) * B + b] = acc[r * lanes];
}

// Stage 2 is ssx_ordered_reduce_kernel (ssx_spectral.hip) with 4 quantities, NN and UU (1 and 3) the integers.

namespace {

// The state, row-major, into the arrays a pure call uploads (ssx_spectral_probe, ssx_spectral_compare): pixels of other contexts read as +0.0 and count 0 --
// they add nothing to a probe and are not comparable.
int state_to_rows(ssx_ctx* ctx, double* S, uint32_t* N, double* Q) {
	const ssx_render_params& p = ctx->cur;
	const uint32_t M = ctx->spectral_bins / 4u;
	hipLaunchKernelGGL(ssx_spectral_export_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_spectral_sums.as<const double>(), ctx->d_spectral_counts.as<const uint32_t>(),
	                   (float*)nullptr, S, N, pixel_grid(&p), M);
	SSX_HIP(ctx, hipGetLastError());
	hipLaunchKernelGGL(ssx_spectral_variance_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_spectral_sums.as<const double>(), ctx->d_spectral_moments.as<const double>(),
	                   ctx->d_spectral_counts.as<const uint32_t>(), (float*)nullptr, Q, pixel_grid(&p), M);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

size_t moment_bytes(const ssx_ctx* ctx, uint32_t tiles) { return (size_t)tiles * ctx->spectral_bins * 64u * sizeof(double); }

// Whether the sample walk about to start will keep the moments (what moments_begin decides once the walk runs): so that the allocation of Q precedes the plan
// of the sample arrays, which asks the device for its free memory.
int moments_reserve(ssx_ctx* ctx, uint32_t my_tiles, bool continuing) {
	if (!ctx->spectral_bins || !ctx->spectral_moments || continuing) return SSX_OK;
	SSX_HIP(ctx, ctx->d_spectral_moments.reserve(moment_bytes(ctx, my_tiles)));
	return SSX_OK;
}

// Start of a sample walk, behind spectral_begin (`spectral`: this walk bins its launches).  The moments follow the bins' rule: zeroed by ssx_render_start,
// carried on by a continue that finds them valid, otherwise left out -- the render is the same, the state stays invalid.
int moments_begin(ssx_ctx* ctx, uint32_t my_tiles, bool continuing, bool spectral, bool* active) {
	*active = spectral && ctx->spectral_moments && (!continuing || ctx->sums.moments_valid);
	if (!*active || continuing || !my_tiles) return SSX_OK;
	SSX_HIP(ctx, hipMemsetAsync(ctx->d_spectral_moments.ptr, 0, moment_bytes(ctx, my_tiles), ctx->stream));
	return SSX_OK;
}

// The one launch of ssx_spectral_moment_kernel, dynamic-LDS size included: a render's (moments_batch) and ssx_debug_spectral_accumulate's.
int launch_spectral_moment(ssx_ctx* ctx, const SsxMomentArgs& a, uint32_t tiles, hipStream_t stream) {
	const size_t lds = (size_t)a.M * 256u * sizeof(double); // <= 32 KB at 64 bins
	hipLaunchKernelGGL(ssx_spectral_moment_kernel, dim3(tiles), dim3(256), lds, stream, a);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

// after the launch of samples [k0, k0 + n_k), next to spectral_batch: the same records, read again
int moments_batch(ssx_ctx* ctx, const ssx_render_params* p, const LaunchPlan& pl, uint32_t n_k, hipStream_t stream) {
	if (pl.args.my_tiles == 0 || n_k == 0) return SSX_OK;
	SsxKernelArgs bound = pl.args;
	bind_arrays(bound, ctx->d_samples.as<uint8_t>(), (uint64_t)pl.args.my_tiles * n_k * 64u, nullptr, 0, true);
	SsxMomentArgs a{};
	a.flux = bound.flux; a.st = bound.st;
	a.Q = ctx->d_spectral_moments.as<double>();
	a.g = pixel_grid(p);
	a.n_k = n_k; a.M = ctx->spectral_bins / 4u;
	a.lambda_min = ctx->lambda_min; a.lambda_step = ctx->lambda_step;
	return launch_spectral_moment(ctx, a, pl.args.my_tiles, stream);
}

// the end of a sample walk: the moments of the launches that ran, or why there are none
void moments_publish(ssx_ctx* ctx, bool active) {
	ctx->sums.moments_valid = active;
	if (!active && ctx->spectral_moments) ctx->moments_note = "the render that made these bins ran without them (it continued bins that had none)";
}

void moments_invalidate(ssx_ctx* ctx, const char* why) { ctx->sums.moments_valid = false; ctx->moments_note = why; }
void moments_drop(ssx_ctx* ctx) { ctx->d_spectral_moments.release(); }

// what every read-out of the moments asks first
int moments_ready(ssx_ctx* ctx, const char* what) { return spectral_ready(ctx, what, true); }

// d_probe: sums and q [pixels][B] binary64, part [height][R][4][B], out [4][R][B], counts [pixels][M], labels [pixels]
struct ProbeBuffers { double* sums; double* q; uint64_t* part; uint64_t* out; uint32_t* counts; uint8_t* labels; };
int probe_buffers(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t B, uint32_t R, ProbeBuffers* d) {
	const size_t pixels = (size_t)width * height;
	return carve(ctx, ctx->d_probe, [&](Carver& c) {
		d->sums = c.take<double>(pixels * B);
		d->q = c.take<double>(pixels * B);
		d->part = c.take<uint64_t>((size_t)height * R * 4u * B);
		d->out = c.take<uint64_t>((size_t)4u * R * B);
		d->counts = c.take<uint32_t>(pixels * (B / 4u));
		d->labels = c.take<uint8_t>(pixels);
	});
}

int probe_check(ssx_ctx* ctx, const char* what, uint32_t width, uint32_t height, const uint8_t* labels, uint32_t R, const void* SS, const void* NN, const void* VV, const void* UU) {
	if (!labels || !SS || !NN || !VV || !UU) return fail(ctx, SSX_ERR_ARG, fmt("%s: labels and the four outputs must not be NULL", what));
	if (R < 1u || R > 32u) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u regions: need 1..32", what, R));
	const size_t pixels = (size_t)width * height;
	for (size_t p = 0; p < pixels; ++p)
		if (labels[p] != 255u && labels[p] >= R)
			return fail(ctx, SSX_ERR_ARG, fmt("%s: labels[%zu][%zu] = %u: need a region 0..%u, or 255 for none", what, p / width, p % width, (unsigned)labels[p], R - 1u));
	return SSX_OK;
}

// The one body of both probes: sums, q and counts are in d already; the labels go up, the two kernels run, the four [R][B] arrays come back.
int probe_device(ssx_ctx* ctx, const ProbeBuffers& d, uint32_t width, uint32_t height, uint32_t B, const uint8_t* labels, uint32_t R, double* SS, uint64_t* NN, double* VV, uint64_t* UU) {
	SSX_HIP(ctx, hipMemcpyAsync(d.labels, labels, (size_t)width * height, hipMemcpyHostToDevice, ctx->stream));
	SsxProbeArgs a{};
	a.sums = d.sums; a.q = d.q; a.counts = d.counts; a.labels = d.labels; a.part = d.part; a.out = d.out;
	a.width = width; a.height = height; a.B = B; a.R = R;
	const size_t lds = (size_t)R * 2u * B * sizeof(uint64_t); // <= 32 KB
	hipLaunchKernelGGL(ssx_probe_rows_kernel, dim3(height, 2), dim3(2u * B), lds, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	hipLaunchKernelGGL(ssx_ordered_reduce_kernel, blocks_of((size_t)4u * R * B), dim3(256), 0, ctx->stream, d.part, d.out, height, R, B, 4u, 0xAu);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return copy_planes(ctx, d.out, (size_t)R * B, { SS, NN, VV, UU });
}

} // namespace

extern "C" {

int ssx_set_spectral_moments(ssx_ctx* ctx, int enable) {
	if (!ctx) return SSX_ERR_ARG;
	const bool on = enable != 0;
	if (on && !ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, "ssx_set_spectral_moments: spectral output is off (ssx_set_spectral_bins first)");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (on == ctx->spectral_moments) return SSX_OK;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if (const int rc = wait_device_pending(ctx)) return rc;
	ctx->spectral_moments = on;
	moments_invalidate(ctx, "they were switched on after the render that made these bins (valid from zero samples or not at all: ssx_render_start first)");
	if (!on) moments_drop(ctx);
	return SSX_OK;
}

int ssx_spectral_variance(ssx_ctx* ctx, ssx_spectral_info_t* info, float* var, double* q) {
	if (!ctx || !info) return SSX_ERR_ARG;
	if (const int rc = moments_ready(ctx, "ssx_spectral_variance")) return rc;
	spectral_info_of(ctx, info);
	if (!var && !q) return SSX_OK;
	const ssx_render_params& p = ctx->cur;
	const uint32_t B = ctx->spectral_bins, M = B / 4u;
	const size_t n = (size_t)p.width * p.height * B;
	double* d_q; float* d_var;
	if (const int rc = carve(ctx, ctx->d_stage, [&](Carver& c) { d_q = c.take<double>(n); d_var = c.take<float>(n); })) return rc;
	hipLaunchKernelGGL(ssx_spectral_variance_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_spectral_sums.as<const double>(), ctx->d_spectral_moments.as<const double>(),
	                   ctx->d_spectral_counts.as<const uint32_t>(), var ? d_var : nullptr, q ? d_q : nullptr, pixel_grid(&p), M);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (q) SSX_HIP(ctx, hipMemcpy(q, d_q, n * sizeof(double), hipMemcpyDeviceToHost));
	if (var) SSX_HIP(ctx, hipMemcpy(var, d_var, n * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_spectral_moments_import(ssx_ctx* ctx, const ssx_spectral_info_t* info, const double* q) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_moments_import";
	if (!ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, fmt("%s: spectral output is off (ssx_set_spectral_bins)", what));
	if (!ctx->spectral_moments) return fail(ctx, SSX_ERR_STATE, fmt("%s: spectral moments are off (ssx_set_spectral_moments)", what));
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (!ctx->sums.continuable || !ctx->sums.spectral_valid || !ctx->sums.spectral_imported)
		return fail(ctx, SSX_ERR_STATE, fmt("%s: the moments go on top of the bins of a successful ssx_spectral_import, directly: the context holds none, or has rendered since", what));
	// from here on a refusal leaves the moments invalid; bins and pixel sums stay what the two imports made them
	auto refuse = [&](const std::string& why) {
		moments_invalidate(ctx, "an ssx_spectral_moments_import on top of ssx_spectral_import was refused or failed (ssx_spectral_import itself does not carry them)");
		return fail(ctx, SSX_ERR_ARG, why);
	};
	if (!info || !q) return refuse(fmt("%s: info and q must not be NULL", what));
	const std::string why = spectral_info_mismatch(ctx, what, "these moments", "the imported bins", info);
	if (!why.empty()) return refuse(why);
	const ssx_render_params& p = ctx->cur;
	const uint32_t B = ctx->spectral_bins, M = B / 4u;
	moments_invalidate(ctx, "an ssx_spectral_moments_import on top of ssx_spectral_import was refused or failed (ssx_spectral_import itself does not carry them)");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if (const int rc = wait_device_pending(ctx)) return rc;
	const uint32_t tiles = owned_tiles(p);
	const size_t n = (size_t)p.width * p.height * B;
	SSX_HIP(ctx, ctx->d_spectral_moments.reserve(moment_bytes(ctx, tiles))); // (before the kernel; ssx_scratch_info counts it from here on)
	uint32_t bad[3] = { 0u, 0u, 0u };
	if (tiles) {
		double* d_q; uint32_t* d_bad; // d_stage: q and the three flags of the check
		if (const int rc = carve(ctx, ctx->d_stage, [&](Carver& c) { d_q = c.take<double>(n); d_bad = c.take<uint32_t>(3); })) return rc;
		SSX_HIP(ctx, hipMemcpyAsync(d_q, q, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		SSX_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof bad, ctx->stream));
		const size_t lds = 64u * (size_t)(B + 1u) * sizeof(double); // <= 33 KB at 64 bins
		hipLaunchKernelGGL(ssx_spectral_moments_import_kernel, dim3(tiles), dim3(256), lds, ctx->stream, d_q, ctx->d_spectral_sums.as<const double>(),
		                   ctx->d_spectral_counts.as<const uint32_t>(), ctx->d_spectral_moments.as<double>(), d_bad, pixel_grid(&p), M);
		SSX_HIP(ctx, hipGetLastError());
		SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		SSX_HIP(ctx, hipMemcpy(bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
	}
	const char* const tail = "these are not the second moments of the imported bins (another render's, one rank's unmerged export -- merge the ranks' by ownership first -- or the sums S)";
	if (bad[0]) return fail(ctx, SSX_ERR_ARG, fmt("%s: q: rule n == 0: a sub-bin this context owns holds no sample, and its Q is not +0.0: %s", what, tail));
	if (bad[1]) return fail(ctx, SSX_ERR_ARG, fmt("%s: q: rule n == 1: a sub-bin this context owns holds one sample, and its Q is not S * S: %s", what, tail));
	if (bad[2]) return fail(ctx, SSX_ERR_ARG, fmt("%s: q: rule n >= 2: a sub-bin this context owns holds a negative Q, and a sum of squares has none: %s", what, tail));
	ctx->sums.moments_valid = true; ctx->moments_note.clear();
	return SSX_OK;
}

int ssx_spectral_probe(ssx_ctx* ctx, const uint8_t* labels, uint32_t regions, double* SS, uint64_t* NN, double* VV, uint64_t* UU) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_probe";
	int rc = moments_ready(ctx, what);
	if (rc) return rc;
	const ssx_render_params& p = ctx->cur;
	if ((rc = probe_check(ctx, what, p.width, p.height, labels, regions, SS, NN, VV, UU))) return rc;
	ProbeBuffers d;
	if ((rc = probe_buffers(ctx, p.width, p.height, ctx->spectral_bins, regions, &d))) return rc;
	if ((rc = state_to_rows(ctx, d.sums, d.counts, d.q))) return rc;
	return probe_device(ctx, d, p.width, p.height, ctx->spectral_bins, labels, regions, SS, NN, VV, UU);
}

int ssx_probe_arrays(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const double* sums, const double* q, const uint32_t* counts, const uint8_t* labels, uint32_t regions,
                     double* SS, uint64_t* NN, double* VV, uint64_t* UU) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_probe_arrays";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if (!sums || !q || !counts) return fail(ctx, SSX_ERR_ARG, fmt("%s: sums, q and counts must not be NULL", what));
	int rc = denoise_check_size(ctx, width, height, what);
	if (rc) return rc;
	if ((rc = probe_check(ctx, what, width, height, labels, regions, SS, NN, VV, UU))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	ProbeBuffers d;
	if ((rc = probe_buffers(ctx, width, height, bins, regions, &d))) return rc;
	const size_t pixels = (size_t)width * height;
	SSX_HIP(ctx, hipMemcpyAsync(d.sums, sums, pixels * bins * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.q, q, pixels * bins * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.counts, counts, pixels * (bins / 4u) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	return probe_device(ctx, d, width, height, bins, labels, regions, SS, NN, VV, UU);
}

// ssx_spectral_bin_kernel and ssx_spectral_moment_kernel on the caller's records (include/ssx.h): the records of each launch go up in the path kernels' layout
// [tile slot][k - k0][pixel of the tile] -- slot and lane of a pixel by ssx_shared_tile, as the export kernel finds them --, the two kernels run through the launch
// helpers a render uses, on S, N, Q of the call's own, and the export and variance kernels bring the state back row-major.  Everything lives in d_probe, the
// temporaries of one pure call: the context's bins, moments, sums and flags are not looked at.
int ssx_debug_spectral_accumulate(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, uint32_t tile_first, uint32_t tile_stride, uint32_t tile_skew,
                                  float lambda_min, float lambda_step, uint32_t launches, const uint32_t* n_k, const float* flux, const float* lambda_0,
                                  double* sums, uint32_t* counts, double* q) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_debug_spectral_accumulate";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	int rc = denoise_check_size(ctx, width, height, what);
	if (rc) return rc;
	if (tile_stride == 0u || tile_first >= tile_stride) return fail(ctx, SSX_ERR_ARG, fmt("%s: need tile_first < tile_stride", what));
	if (!std::isfinite(lambda_min) || !std::isfinite(lambda_step) || !(lambda_step > 0.0f)) return fail(ctx, SSX_ERR_ARG, fmt("%s: lambda_min must be finite, lambda_step finite and positive", what));
	if (!n_k || !flux || !lambda_0 || !sums || !counts) return fail(ctx, SSX_ERR_ARG, fmt("%s: n_k, flux, lambda_0, sums and counts must not be NULL", what));
	if (launches == 0u) return fail(ctx, SSX_ERR_ARG, fmt("%s: launches must be positive", what));
	ssx_render_params p{};
	p.struct_size = sizeof p; p.width = width; p.height = height; p.tile_first = tile_first; p.tile_stride = tile_stride; p.tile_skew = tile_skew;
	const uint64_t all_tiles = (uint64_t)tiles_across(width) * tiles_across(height);
	uint64_t K = 0; uint32_t max_nk = 0;
	for (uint32_t l = 0; l < launches; ++l) {
		if (n_k[l] == 0u) return fail(ctx, SSX_ERR_ARG, fmt("%s: n_k[%u] = 0: every launch needs a sample", what, l));
		K += n_k[l]; max_nk = n_k[l] > max_nk ? n_k[l] : max_nk;
		if (all_tiles * 64u * K > (1ull << 30)) return fail(ctx, SSX_ERR_ARG, fmt("%s: too many records (tiles * 64 * samples per pixel: at most 2^30)", what));
	}
	if ((rc = idle_on_device(ctx))) return rc;
	const SsxPixelGrid g = pixel_grid(&p);
	const uint32_t tiles = owned_tiles(p), B = bins, M = bins / 4u;
	const size_t pixels = (size_t)width * height, records = (size_t)tiles * max_nk * 64u, cells = (size_t)tiles * B * 64u;
	float4* d_flux; uint4* d_st; double* d_S; double* d_Q; uint32_t* d_N; double* d_sums; double* d_q; uint32_t* d_counts;
	if ((rc = carve(ctx, ctx->d_probe, [&](Carver& c) {
		d_flux = c.take<float4>(records); d_st = c.take<uint4>(records);
		d_S = c.take<double>(cells); d_Q = c.take<double>(cells); d_N = c.take<uint32_t>((size_t)tiles * M * 64u);
		d_sums = c.take<double>(pixels * B); d_q = c.take<double>(pixels * B); d_counts = c.take<uint32_t>(pixels * M);
	}))) return rc;
	if (tiles) { // as spectral_begin and moments_begin leave a fresh render
		SSX_HIP(ctx, hipMemsetAsync(d_S, 0, cells * sizeof(double), ctx->stream));
		SSX_HIP(ctx, hipMemsetAsync(d_Q, 0, cells * sizeof(double), ctx->stream));
		SSX_HIP(ctx, hipMemsetAsync(d_N, 0, (size_t)tiles * M * 64u * sizeof(uint32_t), ctx->stream));
	}
	std::vector<float4> fl; std::vector<uint4> st;
	uint64_t k0 = 0;
	for (uint32_t l = 0; l < launches && tiles; k0 += n_k[l], ++l) {
		const uint32_t n = n_k[l];
		const size_t n_rec = (size_t)tiles * n * 64u;
		fl.assign(n_rec, float4{ 0.0f, 0.0f, 0.0f, 0.0f }); st.assign(n_rec, uint4{ 0u, 0u, 0u, 0u });
		for (uint32_t j = 0; j < height; ++j) for (uint32_t i = 0; i < width; ++i) {
			if (!ssx_owns_pixel(g, i, j)) continue;
			const size_t slot = ssx_shared_tile(g, i, j) / g.tile_stride, lane = (j & 7u) * 8u + (i & 7u);
			for (uint32_t kk = 0; kk < n; ++kk) {
				const size_t r = (slot * n + kk) * 64u + lane, o = ((size_t)j * width + i) * K + k0 + kk;
				memcpy(&fl[r], flux + 4u * o, sizeof(float4)); // (bits, not values: a signalling NaN stays what the caller wrote)
				memcpy(&st[r].x, lambda_0 + o, sizeof(float));
			}
		}
		SSX_HIP(ctx, hipMemcpy(d_flux, fl.data(), n_rec * sizeof(float4), hipMemcpyHostToDevice)); // (synchronous: the host vectors are refilled for the next launch)
		SSX_HIP(ctx, hipMemcpy(d_st, st.data(), n_rec * sizeof(uint4), hipMemcpyHostToDevice));
		SsxSpectralArgs a{};
		a.flux = d_flux; a.st = d_st; a.S = d_S; a.N = d_N; a.g = g; a.n_k = n; a.M = M; a.lambda_min = lambda_min; a.lambda_step = lambda_step;
		if ((rc = launch_spectral_bin(ctx, a, tiles, ctx->stream))) return rc;
		if (q) {
			SsxMomentArgs b{};
			b.flux = d_flux; b.st = d_st; b.Q = d_Q; b.g = g; b.n_k = n; b.M = M; b.lambda_min = lambda_min; b.lambda_step = lambda_step;
			if ((rc = launch_spectral_moment(ctx, b, tiles, ctx->stream))) return rc;
		}
		SSX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the records are overwritten by the next launch's
	}
	hipLaunchKernelGGL(ssx_spectral_export_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, (const double*)d_S, (const uint32_t*)d_N, (float*)nullptr, d_sums, d_counts, g, M);
	SSX_HIP(ctx, hipGetLastError());
	if (q) {
		hipLaunchKernelGGL(ssx_spectral_variance_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, (const double*)d_S, (const double*)d_Q, (const uint32_t*)d_N, (float*)nullptr, d_q, g, M);
		SSX_HIP(ctx, hipGetLastError());
	}
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(sums, d_sums, pixels * B * sizeof(double), hipMemcpyDeviceToHost));
	SSX_HIP(ctx, hipMemcpy(counts, d_counts, pixels * M * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (q) SSX_HIP(ctx, hipMemcpy(q, d_q, pixels * B * sizeof(double), hipMemcpyDeviceToHost));
	return SSX_OK;
}

} // extern "C"

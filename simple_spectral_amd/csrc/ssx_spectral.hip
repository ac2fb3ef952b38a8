// ssx_spectral.hip -- spectral radiance output: per-pixel wavelength bins of the hero fluxes (include/ssx.h, "Spectral radiance output").  Part of
// ssx_api.hip's translation unit (included behind its context and launch helpers, like ssx_progressive.hip).  The path kernels' part is one store:
// the fold of the _flux twins leaves every sample's hero flux in flux[] (ssx_kernels.hip resolve_records).  Everything else is here: the kernel that
// bins a launch's samples, run after each launch of the sample walk next to the noise estimate's, the export kernel, its inverse (ssx_spectral_import: the bins
// of a checkpoint taken up again) and the entry points.

// What ssx_spectral_bin_kernel needs of a launch: the records [tile slot][k - k0][pixel of the tile] of its flux[] and st[] arrays (st[r].x is lambda_0
// once the path has ended), and the persistent state S[tile slot][bin][pixel of the tile] (binary64) and N[tile slot][m][pixel of the tile].
struct SsxSpectralArgs {
	const float4* flux; const uint4* st;
	double* S; uint32_t* N;
	SsxPixelGrid g;          // the device's tile list: slot -> tile by tile_of_slot (ssx_kernels.hip), as the path kernels walk it
	uint32_t n_k, M;         // samples per pixel of the launch; bins per hero slot (B / 4)
	float lambda_min, lambda_step;
};

// One 256-lane workgroup per owned tile slot; lane = (pixel of the tile, hero slot i): the four lanes of a pixel read one 16-byte flux record, and
// lane (pixel, i) owns the pixel's bins i*M .. i*M + M-1 -- no two lanes share an accumulator, so there are no atomics and no barriers.  The lane's M
// accumulators live in LDS as [M][256] binary64 (the bin of a sample is a run-time index: registers would go to scratch; 8 bytes per lane and row:
// conflict-free), the pixel's M counts behind them as [M][64], kept by the i = 0 lanes.  A lane walks the launch's samples in ascending k, as the pixel
// sums are added (binary64 addition is not associative): the result does not depend on launch size, partition or device count.
//     t = (lambda_0 - lambda_min) / lambda_step;  m = min(M-1, (uint32)(t * (float)M));  S[i*M + m] += (double)f[i];  N[m] += 1
// (binary32, IEEE division, no contraction: the build's -ffp-contract=off).  Lanes outside a ragged image have no records and touch nothing.
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_bin_kernel(SsxSpectralArgs a) {
	extern __shared__ double spectral_lds[];
	const uint32_t tid = threadIdx.x, px = tid >> 2, i = tid & 3u, slot = blockIdx.x, M = a.M;
	uint32_t tx, ty;
	(void)tile_of_slot(a.g, slot, tx, ty);
	if (tx * 8u + (px & 7u) >= a.g.width || ty * 8u + (px >> 3) >= a.g.height) return;
	double* const acc = spectral_lds + tid;                                              // [m * 256]
	uint32_t* const cnt = reinterpret_cast<uint32_t*>(spectral_lds + (size_t)M * 256u) + px; // [m * 64]
	double* const S = a.S + ((size_t)slot * 4u * M + (size_t)i * M) * 64u + px;          // [m * 64]
	uint32_t* const N = a.N + (size_t)slot * M * 64u + px;                               // [m * 64]
	for (uint32_t m = 0; m < M; ++m) { acc[m * 256u] = S[m * 64u]; if (i == 0u) cnt[m * 64u] = N[m * 64u]; }
	const float fM = (float)M;
	size_t r = (size_t)slot * a.n_k * 64u + px;
#pragma unroll 4
	for (uint32_t kk = 0; kk < a.n_k; ++kk, r += 64u) {
		const float f = reinterpret_cast<const float*>(a.flux + r)[i], lambda_0 = __uint_as_float(a.st[r].x);
		const float t = (lambda_0 - a.lambda_min) / a.lambda_step;
		const uint32_t m = min(M - 1u, (uint32_t)(t * fM));
		acc[m * 256u] += (double)f;
		if (i == 0u) cnt[m * 64u] += 1u;
	}
	for (uint32_t m = 0; m < M; ++m) { S[m * 64u] = acc[m * 256u]; if (i == 0u) N[m * 64u] = cnt[m * 64u]; }
}

// S, N -> row-major [height][width][B] means and sums and [height][width][M] counts (any may be NULL); 0 for pixels the context does not own.
// mean[b] = N[b % M] ? (float)(S[b] / (double)N[b % M]) : 0.0f
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_export_kernel(const double* S, const uint32_t* N, float* mean, double* sums, uint32_t* counts, SsxPixelGrid g, uint32_t M) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n = g.width * g.height, B = 4u * M;
	if (p >= n) return;
	const uint32_t i = p % g.width, j = p / g.width;
	const bool own = ssx_owns_pixel(g, i, j);
	const size_t slot = ssx_shared_tile(g, i, j) / g.tile_stride, lane = (j & 7u) * 8u + (i & 7u);
	for (uint32_t b = 0; b < B; ++b) {
		const double s = own ? S[(slot * B + b) * 64u + lane] : 0.0;
		const uint32_t c = own ? N[(slot * M + b % M) * 64u + lane] : 0u;
		if (sums) sums[(size_t)p * B + b] = s;
		if (mean) mean[(size_t)p * B + b] = c ? (float)(s / (double)c) : 0.0f;
		if (counts && b < M) counts[(size_t)p * M + b] = c;
	}
}

// Rows into LDS, the first half of both import kernels (this one and ssx_spectral_moments_import_kernel): the tile at (i0, j0) of a row-major whole-image
// binary64 array src [height][width][B] -> lds [64 pixels][B + 1], by the 256 lanes of a workgroup (the caller's barrier follows).
//   in:   the 8 pixel rows of a tile are 8 runs of cols * B consecutive doubles in the source (cols = 8, fewer in the image's last tile column; 4 KB at B = 64).
//         Consecutive lanes read consecutive 16-byte pairs of a run -- B is a multiple of 4, so every run starts 32-byte aligned in an array that is.  Rows and
//         columns outside a ragged image are never read.
//   LDS:  the stride B + 1 is an ODD number of elements: on the way out lane = pixel reads element b of its row, i.e. 8-byte address (B + 1) * pixel + b.  A
//         ds_read_b64 is served in two groups of 32 lanes over 64 four-byte banks, bank = (address / 4) mod 64, so the 32 lanes of a group need 32 distinct even
//         bank pairs: 2 * (B + 1) * pixel mod 64 distinct for 32 consecutive pixels, which holds exactly when the stride is odd (one element of padding: the
//         access width); the unpadded stride B -- 4, ..., 64 doubles -- would put 2, ..., 32 lanes on one bank pair.  The price is on the way in: with an odd
//         stride a pixel's row starts 8-byte aligned only, so a pair is stored as two 8-byte writes (16 lanes a group, 32 banks, lanes l and l + 8 on the same
//         ones: 2-way), which the write's own register transfer mostly covers.  33 KB at B = 64.
__device__ __forceinline__ void tile_rows_to_lds(const double* src, double* lds, uint32_t width, uint32_t i0, uint32_t j0, uint32_t cols, uint32_t rows, uint32_t B) {
	const uint32_t pairs = cols * (B / 2u);                                                        // 16-byte pairs of one run
	for (uint32_t e = threadIdx.x; e < rows * pairs; e += 256u) {
		const uint32_t r = e / pairs, v = e - r * pairs, c = (2u * v) / B, b = 2u * v - c * B;       // (B is even: a pair never straddles two pixels)
		const double2 d = reinterpret_cast<const double2*>(src + ((size_t)(j0 + r) * width + i0) * B)[v];
		double* const o = lds + (r * 8u + c) * (B + 1u) + b;
		o[0] = d.x; o[1] = d.y;
	}
}

// The inverse of the export for the tiles this context owns: row-major whole-image sums [height][width][B] and counts [height][width][M] (row 0 = bottom; whoever
// exported them may have owned other tiles) -> S[tile slot][bin][pixel of the tile], N[tile slot][m][pixel of the tile].  A transposition through LDS, one
// 256-lane workgroup per owned tile slot (slot -> tile by tile_of_slot), no atomics: a workgroup writes its own slot only.
//   in:   the sums by tile_rows_to_lds; the counts' runs of cols * M words word by word (M may be odd: such a run has no alignment to speak of).
//   LDS:  [64 pixels][B + 1] doubles, then [64 pixels][M | 1] words.  The counts' ds_read_b32 has 32 banks for 32 lanes: an odd word stride again, M + 1 for an
//         even M, M itself for an odd one.  33 KB + 4 KB at B = 64.
//   out:  wave w stores bins w, w + 4, ...: per bin the 64 lanes' doubles are 512 consecutive bytes, per m 256.  Lanes of pixels outside the image store +0 / 0,
//         what the memset of a fresh render leaves there.
// The check: every sample is counted exactly once, misses included (ssx_spectral_bin_kernel), so for an in-image pixel the sum of its M counts is done_spp --
// after a finished render, a stopped one (the walk stops between launches, after the launch's bins) and a levelled one alike.  A pixel that breaks it stores
// 1 into *bad (a plain store; every writer stores the same value).
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_import_kernel(const double* sums, const uint32_t* counts, double* S, uint32_t* N, uint32_t* bad, SsxPixelGrid g, uint32_t M, uint32_t done_spp) {
	extern __shared__ double spectral_lds[];
	const uint32_t tid = threadIdx.x, slot = blockIdx.x, B = 4u * M, s_stride = B + 1u, n_stride = M | 1u;
	uint32_t tx, ty;
	(void)tile_of_slot(g, slot, tx, ty);
	const uint32_t i0 = tx * 8u, j0 = ty * 8u, cols = min(8u, g.width - i0), rows = min(8u, g.height - j0);
	double* const ls = spectral_lds;                                                               // [pixel * s_stride + b]
	uint32_t* const ln = reinterpret_cast<uint32_t*>(spectral_lds + 64u * s_stride);               // [pixel * n_stride + m]
	tile_rows_to_lds(sums, ls, g.width, i0, j0, cols, rows, B);
	const uint32_t words = cols * M;
	for (uint32_t e = tid; e < rows * words; e += 256u) {
		const uint32_t r = e / words, v = e - r * words, c = v / M, m = v - c * M;
		ln[(r * 8u + c) * n_stride + m] = counts[((size_t)(j0 + r) * g.width + i0) * M + v];
	}
	__syncthreads();
	const uint32_t px = tid & 63u, w = tid >> 6;
	const bool inside = (px & 7u) < cols && (px >> 3) < rows;
	double* const So = S + (size_t)slot * B * 64u + px;
	uint32_t* const No = N + (size_t)slot * M * 64u + px;
	for (uint32_t b = w; b < B; b += 4u) So[(size_t)b * 64u] = inside ? ls[px * s_stride + b] : 0.0;
	for (uint32_t m = w; m < M; m += 4u) No[(size_t)m * 64u] = inside ? ln[px * n_stride + m] : 0u;
	if (w == 0u && inside) {
		uint32_t n = 0u;
		for (uint32_t m = 0; m < M; ++m) n += ln[px * n_stride + m];
		if (n != done_spp) *bad = 1u;
	}
}

// The ordered reduce behind the probes and the comparison: part [rows][R][K][B] -> out [K][R][B], one lane per (quantity, r, b) adds the rows' partials in
// ascending row order, from +0.0 / 0; bit q of integer_mask says that quantity q is uint64, not binary64.  The additions stay in order; the loads do not depend
// on them, so the loop is unrolled to keep 16 of them in flight.  (ssx_spectral_noise_reduce_kernel stays its own: its partials are four arrays of two widths
// in a [tiles][B] layout that the ABI hands out; a width parameter and an indirection would cost more than its 15 lines.)
extern "C" __global__ void __launch_bounds__(256) ssx_ordered_reduce_kernel(const uint64_t* part, uint64_t* out, uint32_t rows, uint32_t R, uint32_t B, uint32_t K, uint32_t integer_mask) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= K * R * B) return;
	const uint32_t quantity = e / (R * B), rb = e - quantity * (R * B), r = rb / B, b = rb - r * B;
	const uint64_t* const src = part + ((size_t)r * K + quantity) * B + b;
	const size_t stride = (size_t)R * K * B;
	if ((integer_mask >> quantity) & 1u) {
		uint64_t total = 0ull;
#pragma unroll 16
		for (uint32_t j = 0; j < rows; ++j) total += src[j * stride];
		out[e] = total;
	} else {
		double total = 0.0;
#pragma unroll 16
		for (uint32_t j = 0; j < rows; ++j) total += reinterpret_cast<const double*>(src)[j * stride];
		reinterpret_cast<double*>(out)[e] = total;
	}
}

namespace {

size_t spectral_sum_bytes(const ssx_ctx* ctx, uint32_t tiles) { return (size_t)tiles * ctx->spectral_bins * 64u * sizeof(double); }
size_t spectral_count_bytes(const ssx_ctx* ctx, uint32_t tiles) { return (size_t)tiles * (ctx->spectral_bins / 4u) * 64u * sizeof(uint32_t); }

// What a context with spectral output on cannot render (out of scope so far, not a limit of the design: include/ssx.h).
int spectral_refuses(ssx_ctx* ctx, const ssx_render_params& p, bool tile_walk) {
	if (!ctx->spectral_bins) return SSX_OK;
	if (ctx->rgb_mode) return fail(ctx, SSX_ERR_ARG, "spectral output is on (ssx_set_spectral_bins): a scene in SSX_MODE_RGB carries no wavelengths");
	if (p.libm != SSX_LIBM_BUILD) return fail(ctx, SSX_ERR_ARG, "spectral output is on (ssx_set_spectral_bins): libm = glibc-2.35 is not supported with it");
	if (tile_walk) return fail(ctx, SSX_ERR_ARG, "spectral output is on (ssx_set_spectral_bins): tile_major renders are not supported with it");
	return SSX_OK;
}

// Start of a sample walk.  ssx_render_start: zeroed state for the device's tiles.  A continued render carries valid state on; without it (sums that were
// imported without their bins, or rendered with spectral output off or another bin count) it renders normally and the state stays invalid.  *active: bin this walk's launches.
int spectral_begin(ssx_ctx* ctx, uint32_t my_tiles, bool continuing, bool* active) {
	*active = ctx->spectral_bins != 0u && (!continuing || ctx->sums.spectral_valid);
	if (!*active || continuing) return SSX_OK;
	SSX_HIP(ctx, ctx->d_spectral_sums.reserve(spectral_sum_bytes(ctx, my_tiles)));
	SSX_HIP(ctx, ctx->d_spectral_counts.reserve(spectral_count_bytes(ctx, my_tiles)));
	if (my_tiles) {
		SSX_HIP(ctx, hipMemsetAsync(ctx->d_spectral_sums.ptr, 0, spectral_sum_bytes(ctx, my_tiles), ctx->stream));
		SSX_HIP(ctx, hipMemsetAsync(ctx->d_spectral_counts.ptr, 0, spectral_count_bytes(ctx, my_tiles), ctx->stream));
	}
	return SSX_OK;
}

// The one launch of ssx_spectral_bin_kernel, dynamic-LDS size included: a render's (spectral_batch) and ssx_debug_spectral_accumulate's (ssx_spectral_stats.hip).
int launch_spectral_bin(ssx_ctx* ctx, const SsxSpectralArgs& a, uint32_t tiles, hipStream_t stream) {
	const size_t lds = (size_t)a.M * (256u * sizeof(double) + 64u * sizeof(uint32_t)); // <= 36 KB at 64 bins
	hipLaunchKernelGGL(ssx_spectral_bin_kernel, dim3(tiles), dim3(256), lds, stream, a);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

// after the launch of samples [k0, k0 + n_k) of every owned pixel, in stream order: its records are in the sample arrays until the next launch
int spectral_batch(ssx_ctx* ctx, const ssx_render_params* p, const LaunchPlan& pl, uint32_t n_k, hipStream_t stream) {
	if (pl.args.my_tiles == 0 || n_k == 0) return SSX_OK;
	SsxKernelArgs bound = pl.args;
	bind_arrays(bound, ctx->d_samples.as<uint8_t>(), (uint64_t)pl.args.my_tiles * n_k * 64u, nullptr, 0, true); // where make_batch put the launch's arrays
	SsxSpectralArgs a{};
	a.flux = bound.flux; a.st = bound.st;
	a.S = ctx->d_spectral_sums.as<double>(); a.N = ctx->d_spectral_counts.as<uint32_t>();
	a.g = pixel_grid(p);
	a.n_k = n_k; a.M = ctx->spectral_bins / 4u;
	a.lambda_min = ctx->lambda_min; a.lambda_step = ctx->lambda_step;
	return launch_spectral_bin(ctx, a, pl.args.my_tiles, stream);
}

void spectral_drop(ssx_ctx* ctx) { ctx->d_spectral_sums.release(); ctx->d_spectral_counts.release(); }

// ---- what the four spectral fragments share on the host ----

bool valid_bins(uint32_t bins) { return bins >= 4u && bins <= 64u && !(bins & 3u); } // a multiple of 4 up to 64

// One DeviceBuffer carved into typed arrays, each aligned for its type whatever the order: `layout` runs once to size the reservation and once to hand out pointers.
struct Carver {
	uint8_t* base; size_t at;
	template <class T> T* take(size_t count) {
		at = (at + alignof(T) - 1u) / alignof(T) * alignof(T);
		T* const p = base ? reinterpret_cast<T*>(base + at) : nullptr;
		at += count * sizeof(T);
		return p;
	}
};
template <class Layout> int carve(ssx_ctx* ctx, DeviceBuffer& buf, Layout layout) {
	Carver c{nullptr, 0};
	layout(c);
	SSX_HIP(ctx, buf.reserve(c.at));
	c = Carver{buf.as<uint8_t>(), 0};
	layout(c);
	return SSX_OK;
}

// planes of n eight-byte words, one behind the other on the device, back to their host pointers
int copy_planes(ssx_ctx* ctx, const uint64_t* d_out, size_t n, std::initializer_list<void*> outs) {
	for (void* const o : outs) { SSX_HIP(ctx, hipMemcpy(o, d_out, n * 8u, hipMemcpyDeviceToHost)); d_out += n; }
	return SSX_OK;
}

// What every spectral read-out asks first: bins on, (moments on,) no render, valid bins (and valid moments); then the device is the context's.
int spectral_ready(ssx_ctx* ctx, const char* what, bool moments) {
	if (!ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, fmt("%s: spectral output is off (ssx_set_spectral_bins)", what));
	if (moments && !ctx->spectral_moments) return fail(ctx, SSX_ERR_STATE, fmt("%s: spectral moments are off (ssx_set_spectral_moments)", what));
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (!ctx->sums.continuable || !ctx->sums.spectral_valid)
		return fail(ctx, SSX_ERR_STATE, fmt("%s: the context holds no spectral bins: ", what) + (ctx->sums.continuable ? ctx->spectral_note : std::string("no render has accumulated any (ssx_render_start first)")));
	if (moments && !ctx->sums.moments_valid) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context holds no spectral moments: ", what) + ctx->moments_note);
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	return wait_device_pending(ctx);
}

void spectral_info_of(const ssx_ctx* ctx, ssx_spectral_info_t* info) {
	const ssx_render_params& p = ctx->cur;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info;
	info->width = p.width; info->height = p.height; info->bins = ctx->spectral_bins; info->done_spp = ctx->done_spp.load();
	info->lambda_min = ctx->lambda_min; info->bin_width = ctx->lambda_step / (float)(ctx->spectral_bins / 4u);
}

// Whether `info` (`whose`: "these bins", "the other render") belongs to what the context holds: the refusal's text, or nothing.  done_against names what done_spp
// is held against; NULL: it is not.  The floats are compared as bits.
std::string spectral_info_mismatch(const ssx_ctx* ctx, const char* what, const char* whose, const char* done_against, const ssx_spectral_info_t* info) {
	ssx_spectral_info_t own;
	spectral_info_of(ctx, &own);
	if (info->struct_size != sizeof *info) return fmt("%s: ssx_spectral_info_t.struct_size mismatch", what);
	if (info->width != own.width || info->height != own.height)
		return fmt("%s: size differs (%s: %u x %u, this render: %u x %u)", what, whose, info->width, info->height, own.width, own.height);
	if (info->bins != own.bins) return fmt("%s: bins differs (%s: %u, this context: %u)", what, whose, info->bins, own.bins);
	if (done_against && info->done_spp != own.done_spp) return fmt("%s: done_spp differs (%s: %u, %s: %u)", what, whose, info->done_spp, done_against, own.done_spp);
	if (memcmp(&info->lambda_min, &own.lambda_min, sizeof(float)) != 0)
		return fmt("%s: lambda_min differs (%s: %.9g, the uploaded scene: %.9g)", what, whose, (double)info->lambda_min, (double)own.lambda_min);
	if (memcmp(&info->bin_width, &own.bin_width, sizeof(float)) != 0)
		return fmt("%s: bin_width differs (%s: %.9g, the uploaded scene: %.9g)", what, whose, (double)info->bin_width, (double)own.bin_width);
	return std::string();
}

} // namespace

extern "C" {

int ssx_set_spectral_bins(ssx_ctx* ctx, uint32_t bins) {
	if (!ctx) return SSX_ERR_ARG;
	if (bins && !valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_set_spectral_bins: %u bins: need 0 (off) or a multiple of 4 up to 64", bins));
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (bins == ctx->spectral_bins) return SSX_OK;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if (const int rc = wait_device_pending(ctx)) return rc; // (a queued ssx_render_device uses the sample arrays in the layout without flux[])
	ctx->spectral_bins = bins;
	ctx->sums.spectral_valid = ctx->sums.spectral_imported = false; ctx->spectral_note = "the bin count changed after the last render";
	moments_invalidate(ctx, "the bin count changed after the last render"); // (whatever clears the bins clears their moments)
	if (!bins) { spectral_drop(ctx); ctx->spectral_moments = false; moments_drop(ctx); }
	return SSX_OK;
}

int ssx_spectral_read(ssx_ctx* ctx, ssx_spectral_info_t* info, float* mean, double* sums, uint32_t* counts) {
	if (!ctx || !info) return SSX_ERR_ARG;
	if (const int rc = spectral_ready(ctx, "ssx_spectral_read", false)) return rc;
	spectral_info_of(ctx, info);
	if (!mean && !sums && !counts) return SSX_OK;
	const ssx_render_params& p = ctx->cur;
	const uint32_t B = ctx->spectral_bins, M = B / 4u;
	const size_t pixels = (size_t)p.width * p.height;
	double* d_sums; float* d_mean; uint32_t* d_counts;
	if (const int rc = carve(ctx, ctx->d_stage, [&](Carver& c) { d_sums = c.take<double>(pixels * B); d_mean = c.take<float>(pixels * B); d_counts = c.take<uint32_t>(pixels * M); })) return rc;
	hipLaunchKernelGGL(ssx_spectral_export_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_spectral_sums.as<const double>(), ctx->d_spectral_counts.as<const uint32_t>(),
	                   mean ? d_mean : nullptr, sums ? d_sums : nullptr, counts ? d_counts : nullptr, pixel_grid(&p), M);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (sums) SSX_HIP(ctx, hipMemcpy(sums, d_sums, pixels * B * sizeof(double), hipMemcpyDeviceToHost));
	if (mean) SSX_HIP(ctx, hipMemcpy(mean, d_mean, pixels * B * sizeof(float), hipMemcpyDeviceToHost));
	if (counts) SSX_HIP(ctx, hipMemcpy(counts, d_counts, pixels * M * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_spectral_import(ssx_ctx* ctx, const ssx_spectral_info_t* info, const double* sums, const uint32_t* counts) {
	if (!ctx || !info || !sums || !counts) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_import";
	if (info->struct_size != sizeof *info) return fail(ctx, SSX_ERR_ARG, fmt("%s: ssx_spectral_info_t.struct_size mismatch", what)); // (before the state is looked at)
	if (!ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, "ssx_spectral_import: spectral output is off (ssx_set_spectral_bins)");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (!ctx->sums.continuable || !ctx->sums.imported)
		return fail(ctx, SSX_ERR_STATE, "ssx_spectral_import: the bins go on top of the pixel sums of an ssx_sums_import, directly: the context holds none, or has rendered since");
	const std::string why = spectral_info_mismatch(ctx, what, "these bins", "the imported sums", info);
	if (!why.empty()) return fail(ctx, SSX_ERR_ARG, why);
	const ssx_render_params& p = ctx->cur;
	const uint32_t B = ctx->spectral_bins, M = B / 4u, done = ctx->done_spp.load();
	if (const int rc = spectral_refuses(ctx, p, false)) return rc; // (what a continue with the bins would be refused for)
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if (const int rc = wait_device_pending(ctx)) return rc;
	const uint32_t tiles = owned_tiles(p);
	const size_t pixels = (size_t)p.width * p.height;
	double* d_sums; uint32_t* d_counts; uint32_t* d_bad; // d_stage: the sums, the counts and the flag of the check
	if (const int rc = carve(ctx, ctx->d_stage, [&](Carver& c) { d_sums = c.take<double>(pixels * B); d_counts = c.take<uint32_t>(pixels * M); d_bad = c.take<uint32_t>(1); })) return rc;
	SSX_HIP(ctx, ctx->d_spectral_sums.reserve(spectral_sum_bytes(ctx, tiles)));
	SSX_HIP(ctx, ctx->d_spectral_counts.reserve(spectral_count_bytes(ctx, tiles)));
	// from here on the device state is being replaced: it is valid again only once the check has passed
	ctx->sums.spectral_valid = ctx->sums.spectral_imported = false; ctx->spectral_note = "an ssx_spectral_import on top of ssx_sums_import was refused or failed";
	uint32_t bad = 0;
	if (tiles) {
		SSX_HIP(ctx, hipMemcpyAsync(d_sums, sums, pixels * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		SSX_HIP(ctx, hipMemcpyAsync(d_counts, counts, pixels * M * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		SSX_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(uint32_t), ctx->stream));
		const size_t lds = 64u * ((size_t)(B + 1u) * sizeof(double) + (size_t)(M | 1u) * sizeof(uint32_t)); // <= 37 KB at 64 bins
		hipLaunchKernelGGL(ssx_spectral_import_kernel, dim3(tiles), dim3(256), lds, ctx->stream, d_sums, d_counts, ctx->d_spectral_sums.as<double>(),
		                   ctx->d_spectral_counts.as<uint32_t>(), d_bad, pixel_grid(&p), M, done);
		SSX_HIP(ctx, hipGetLastError());
		SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		SSX_HIP(ctx, hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
	}
	if (bad) return fail(ctx, SSX_ERR_ARG, fmt("ssx_spectral_import: counts: a pixel this context owns does not hold done_spp = %u samples over its %u counts (every sample is counted once; "
	                                           "one rank's unmerged export holds zeros where it owned nothing: merge the ranks' exports by ownership first)", done, M));
	ctx->sums.spectral_valid = ctx->sums.spectral_imported = true; ctx->spectral_note.clear();
	moments_invalidate(ctx, "the bins came from ssx_spectral_import, which does not carry their second moments (hand the checkpoint's Q to ssx_spectral_moments_import on top of it, or render from ssx_render_start)");
	return SSX_OK;
}

int ssx_debug_sample_flux(ssx_ctx* ctx, const ssx_render_params* p_in, float* flux, float* lambda_0) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = begin_render(ctx, p_in, &pp, "render in progress");
	if (rc) return rc;
	const ssx_render_params* const p = &pp;
	if (!ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, "ssx_debug_sample_flux: spectral output is off (ssx_set_spectral_bins): the sample arrays hold no flux");
	if ((rc = spectral_refuses(ctx, pp, false))) return rc;
	if (p->tile_first != 0 || p->tile_stride != 1) return fail(ctx, SSX_ERR_ARG, "ssx_debug_sample_flux renders the whole image");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	if ((rc = ready_to_launch(ctx, p, false))) return rc;
	LaunchPlan pl = make_plan(ctx, p);
	if (p->spp > pl.max_spp_per_launch) return fail(ctx, SSX_ERR_ARG, "ssx_debug_sample_flux: too many samples for one launch");
	if ((rc = ensure_samples(ctx, pl, p->spp))) return rc;
	sums_invalidate(ctx);
	if ((rc = clear_sums(ctx, p->width, p->height, ctx->stream))) return rc;
	Batch b = make_batch(ctx, pl, 0, p->spp);
	if ((rc = launch_batch(ctx, b, ctx->stream))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<float4> fl((size_t)b.n_rec);
	std::vector<uint4> st((size_t)b.n_rec);
	SSX_HIP(ctx, hipMemcpy(fl.data(), b.a.flux, fl.size() * sizeof(float4), hipMemcpyDeviceToHost));
	SSX_HIP(ctx, hipMemcpy(st.data(), b.a.st, st.size() * sizeof(uint4), hipMemcpyDeviceToHost));
	const uint32_t spp = p->spp, tiles_x = tiles_across(p->width);
	for (uint32_t j = 0; j < p->height; ++j) for (uint32_t i = 0; i < p->width; ++i) {
		const uint32_t tile = (j >> 3) * tiles_x + (i >> 3), lane = (j & 7u) * 8u + (i & 7u);
		for (uint32_t k = 0; k < spp; ++k) {
			const size_t r = ((size_t)tile * spp + k) * 64u + lane, o = ((size_t)j * p->width + i) * spp + k;
			if (flux) { flux[4 * o + 0] = fl[r].x; flux[4 * o + 1] = fl[r].y; flux[4 * o + 2] = fl[r].z; flux[4 * o + 3] = fl[r].w; }
			if (lambda_0) memcpy(&lambda_0[o], &st[r].x, 4);
		}
	}
	return SSX_OK;
}

} // extern "C"

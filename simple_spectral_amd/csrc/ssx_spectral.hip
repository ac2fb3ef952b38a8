// ssx_spectral.hip -- spectral radiance output: per-pixel wavelength bins of the hero fluxes (include/ssx.h, "Spectral radiance output").  Part of
// ssx_api.hip's translation unit (included behind its context and launch helpers, like ssx_progressive.hip).  The path kernels' part is one store:
// the fold of the _flux twins leaves every sample's hero flux in flux[] (ssx_kernels.hip resolve_records).  Everything else is here: the kernel that
// bins a launch's samples, run after each launch of the sample walk next to the noise estimate's, the export kernel and the entry points.

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
// imported, or rendered with spectral output off or another bin count) it renders normally and the state stays invalid.  *active: bin this walk's launches.
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
	const size_t lds = (size_t)a.M * (256u * sizeof(double) + 64u * sizeof(uint32_t)); // <= 36 KB at 64 bins
	hipLaunchKernelGGL(ssx_spectral_bin_kernel, dim3(pl.args.my_tiles), dim3(256), lds, stream, a);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

void spectral_drop(ssx_ctx* ctx) { ctx->d_spectral_sums.release(); ctx->d_spectral_counts.release(); }

} // namespace

extern "C" {

int ssx_set_spectral_bins(ssx_ctx* ctx, uint32_t bins) {
	if (!ctx) return SSX_ERR_ARG;
	if (bins > 64u || (bins & 3u)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_set_spectral_bins: %u bins: need 0 (off) or a multiple of 4 up to 64", bins));
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (bins == ctx->spectral_bins) return SSX_OK;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if (const int rc = wait_device_pending(ctx)) return rc; // (a queued ssx_render_device uses the sample arrays in the layout without flux[])
	ctx->spectral_bins = bins;
	ctx->sums.spectral_valid = false; ctx->spectral_note = "the bin count changed after the last render";
	if (!bins) spectral_drop(ctx);
	return SSX_OK;
}

int ssx_spectral_read(ssx_ctx* ctx, ssx_spectral_info_t* info, float* mean, double* sums, uint32_t* counts) {
	if (!ctx || !info) return SSX_ERR_ARG;
	if (!ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, "ssx_spectral_read: spectral output is off (ssx_set_spectral_bins)");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (!ctx->sums.continuable || !ctx->sums.spectral_valid)
		return fail(ctx, SSX_ERR_STATE, "ssx_spectral_read: the context holds no spectral bins: " + (ctx->sums.continuable ? ctx->spectral_note : std::string("no render has accumulated any (ssx_render_start first)")));
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if (const int rc = wait_device_pending(ctx)) return rc;
	const ssx_render_params& p = ctx->cur;
	const uint32_t B = ctx->spectral_bins, M = B / 4u;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info;
	info->width = p.width; info->height = p.height; info->bins = B; info->done_spp = ctx->done_spp.load();
	info->lambda_min = ctx->lambda_min; info->bin_width = ctx->lambda_step / (float)M;
	if (!mean && !sums && !counts) return SSX_OK;
	const size_t pixels = (size_t)p.width * p.height, b_sums = pixels * B * sizeof(double), b_mean = pixels * B * sizeof(float), b_counts = pixels * M * sizeof(uint32_t);
	DeviceBuffer& stage = ctx->d_stage;
	SSX_HIP(ctx, stage.reserve(b_sums + b_mean + b_counts));
	double* const d_sums = stage.as<double>();
	float* const d_mean = reinterpret_cast<float*>(stage.as<uint8_t>() + b_sums);
	uint32_t* const d_counts = reinterpret_cast<uint32_t*>(stage.as<uint8_t>() + b_sums + b_mean);
	hipLaunchKernelGGL(ssx_spectral_export_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_spectral_sums.as<const double>(), ctx->d_spectral_counts.as<const uint32_t>(),
	                   mean ? d_mean : nullptr, sums ? d_sums : nullptr, counts ? d_counts : nullptr, pixel_grid(&p), M);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (sums) SSX_HIP(ctx, hipMemcpy(sums, d_sums, b_sums, hipMemcpyDeviceToHost));
	if (mean) SSX_HIP(ctx, hipMemcpy(mean, d_mean, b_mean, hipMemcpyDeviceToHost));
	if (counts) SSX_HIP(ctx, hipMemcpy(counts, d_counts, b_counts, hipMemcpyDeviceToHost));
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

// ssx_progressive.hip -- continue / export / import of the binary64 pixel sums and the noise estimate by batch means (include/ssx.h,
// "Progressive rendering").  Part of ssx_api.hip's translation unit (included behind its context and launch helpers).  Nothing here touches
// the path, generate or finalize kernels: the kernels below are small per-pixel ones that run between the launches of a render, or on request.

// accumulator -> row-major [height][width][4] (+0 for foreign pixels); s2_out (optional) <- S2 of the noise state (or zeros)
extern "C" __global__ void __launch_bounds__(256) ssx_sums_export_kernel(const double* accum, const double* noise, double* sums, double* s2_out, SsxPixelGrid g) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n = g.width * g.height;
	if (p >= n) return;
	const uint32_t i = p % g.width, j = p / g.width;
	const bool own = ssx_owns_pixel(g, i, j);
	const double* const px = accum + ssx_sum_slot(i, j, g.tiles_x);
	double4 o = make_double4(0.0, 0.0, 0.0, 0.0);
	if (own) o = make_double4(px[0], px[64], px[128], px[192]);
	reinterpret_cast<double4*>(sums)[p] = o;
	if (s2_out) s2_out[p] = (own && noise) ? noise[(size_t)n + p] : 0.0;
}

// row-major sums -> the owned pixels' accumulators (the accumulator was cleared before: foreign tiles stay 0).  With a noise state:
// A_prev = the imported Y sum; S2 = the exporter's, or -- none given -- the imported sum as ONE batch of done_spp samples: A*A / done_spp.
extern "C" __global__ void __launch_bounds__(256) ssx_sums_import_kernel(double* accum, double* noise, const double* sums, const double* s2_in, SsxPixelGrid g, uint32_t done_spp) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n = g.width * g.height;
	if (p >= n) return;
	const uint32_t i = p % g.width, j = p / g.width;
	if (!ssx_owns_pixel(g, i, j)) {
		if (noise) { noise[p] = 0.0; noise[(size_t)n + p] = 0.0; }
		return;
	}
	double* const px = accum + ssx_sum_slot(i, j, g.tiles_x);
	const double4 v = reinterpret_cast<const double4*>(sums)[p];
	px[0] = v.x; px[64] = v.y; px[128] = v.z; px[192] = v.w;
	if (noise) {
		noise[p] = v.y;
		noise[(size_t)n + p] = s2_in ? s2_in[p] : (done_spp ? v.y * v.y / (double)done_spp : 0.0);
	}
}

// the noise state of sums that exist already (the estimate switched on before a continue): they count as one batch
extern "C" __global__ void __launch_bounds__(256) ssx_noise_adopt_kernel(const double* accum, double* noise, SsxPixelGrid g, uint32_t done_spp) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n = g.width * g.height;
	if (p >= n) return;
	const uint32_t i = p % g.width, j = p / g.width;
	const bool own = ssx_owns_pixel(g, i, j);
	const double a = own ? accum[ssx_sum_slot(i, j, g.tiles_x) + 64u] : 0.0;
	noise[p] = a;
	noise[(size_t)n + p] = done_spp ? a * a / (double)done_spp : 0.0;
}

// one batch of n_k samples per pixel has been added to the sums: d = A_now - A_prev; S2 += d*d / n_k; A_prev = A_now
extern "C" __global__ void __launch_bounds__(256) ssx_noise_kernel(const double* accum, double* noise, SsxPixelGrid g, double n_k) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n = g.width * g.height;
	if (p >= n) return;
	const uint32_t i = p % g.width, j = p / g.width;
	if (!ssx_owns_pixel(g, i, j)) return;
	const double a = accum[ssx_sum_slot(i, j, g.tiles_x) + 64u];
	const double d = a - noise[p];
	noise[(size_t)n + p] += d * d / n_k;
	noise[p] = a;
}

// v = ((S2 - A*A/N) / (B-1)) / N, clamped at 0; a_out = A (0 for foreign pixels)
extern "C" __global__ void __launch_bounds__(256) ssx_noise_variance_kernel(const double* accum, const double* noise, double* v_out, double* a_out, SsxPixelGrid g, double N, double B) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n = g.width * g.height;
	if (p >= n) return;
	const uint32_t i = p % g.width, j = p / g.width;
	double v = 0.0, a = 0.0;
	if (ssx_owns_pixel(g, i, j)) {
		a = accum[ssx_sum_slot(i, j, g.tiles_x) + 64u];
		v = ((noise[(size_t)n + p] - a * a / N) / (B - 1.0)) / N;
		if (!(v > 0.0)) v = 0.0;
	}
	v_out[p] = v; a_out[p] = a;
}

namespace {

size_t noise_bytes(const ssx_render_params* p) { return (size_t)p->width * p->height * 2 * sizeof(double); }

// Start of a sample walk: ssx_render_start resets the estimate; a continued render carries it on, or adopts the k_begin samples it finds as one batch.
int noise_begin(ssx_ctx* ctx, const ssx_render_params* p, uint32_t k_begin, bool continuing) {
	if (!ctx->noise_on) { ctx->sums.noise_valid = false; return SSX_OK; }
	if (continuing && ctx->sums.noise_valid) return SSX_OK;
	SSX_HIP(ctx, ctx->d_noise.reserve(noise_bytes(p)));
	const uint32_t done = continuing ? k_begin : 0u;
	if (!done) SSX_HIP(ctx, hipMemsetAsync(ctx->d_noise.ptr, 0, noise_bytes(p), ctx->stream));
	else {
		hipLaunchKernelGGL(ssx_noise_adopt_kernel, pixel_blocks(p), dim3(256), 0, ctx->stream, ctx->d_accum.as<const double>(), ctx->d_noise.as<double>(), pixel_grid(p), done);
		SSX_HIP(ctx, hipGetLastError());
	}
	ctx->sums.noise_batches = done ? 1u : 0u;
	ctx->sums.noise_valid = true;
	return SSX_OK;
}

// after the launch of a sample range of n_k samples per pixel, in stream order
int noise_batch(ssx_ctx* ctx, const ssx_render_params* p, uint32_t n_k, hipStream_t stream) {
	hipLaunchKernelGGL(ssx_noise_kernel, pixel_blocks(p), dim3(256), 0, stream, ctx->d_accum.as<const double>(), ctx->d_noise.as<double>(), pixel_grid(p), (double)n_k);
	SSX_HIP(ctx, hipGetLastError());
	++ctx->sums.noise_batches;
	return SSX_OK;
}

// the estimate switched off: its state goes, the sums stay what they are
void noise_drop(ssx_ctx* ctx) { if (hipSetDevice(ctx->device) == hipSuccess) ctx->d_noise.release(); ctx->sums.noise_valid = false; ctx->sums.noise_batches = 0; }

// entry points that read or replace the sums: a context with continuable sums and no render running, its device current
int sums_ready(ssx_ctx* ctx, const char* what) {
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (!ctx->sums.continuable) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context holds no sums that can be continued (render with ssx_render_start, or ssx_sums_import, first)", what));
	SSX_HIP(ctx, hipSetDevice(ctx->device)); // (the worker of the last render has left the device idle: `rendering` is its last word)
	return wait_device_pending(ctx);
}

} // namespace

extern "C" {

uint64_t ssx_scene_digest(ssx_ctx* ctx) { return (ctx && ctx->have_scene) ? ctx->scene_digest : 0u; }

int ssx_render_continue(ssx_ctx* ctx, uint32_t spp_more) {
	if (!ctx) return SSX_ERR_ARG;
	int rc = sums_ready(ctx, "ssx_render_continue");
	if (rc) return rc;
	const uint32_t done = ctx->done_spp.load();
	if (spp_more == 0) return fail(ctx, SSX_ERR_ARG, "spp_more must be positive");
	if ((uint64_t)done + spp_more > 0xFFFFFFFFull) return fail(ctx, SSX_ERR_ARG, "more than 2^32 - 1 samples per pixel in all");
	ssx_render_params p = ctx->cur;
	p.spp = done + spp_more;
	return start_worker(ctx, p, done, true, spp_more);
}

int ssx_sums_export(ssx_ctx* ctx, ssx_sums_info_t* info, double* sums, double* noise_s2) {
	if (!ctx || !info || !sums) return SSX_ERR_ARG;
	int rc = sums_ready(ctx, "ssx_sums_export");
	if (rc) return rc;
	const ssx_render_params& p = ctx->cur;
	const bool have_noise = ctx->noise_on && ctx->sums.noise_valid;
	memset(info, 0, sizeof *info);
	info->struct_size = sizeof *info;
	info->width = p.width; info->height = p.height; info->done_spp = ctx->done_spp.load(); info->seed = p.seed;
	info->indirect_only = p.indirect_only ? 1u : 0u; info->no_explicit_light_sampling = p.no_explicit_light_sampling ? 1u : 0u;
	info->no_flat_field_correction = p.no_flat_field_correction ? 1u : 0u; info->libm = p.libm; info->rgb_mode = ctx->rgb_mode ? 1u : 0u;
	info->tile_first = p.tile_first; info->tile_stride = p.tile_stride; info->tile_skew = p.tile_skew;
	info->noise_batches = have_noise ? ctx->sums.noise_batches : 0u;
	info->scene_digest = ctx->scene_digest;
	const size_t pixels = (size_t)p.width * p.height;
	DeviceBuffer& stage = ctx->d_stage;
	SSX_HIP(ctx, stage.reserve(pixels * 5 * sizeof(double)));
	double* const d_sums = stage.as<double>(), * const d_s2 = noise_s2 ? d_sums + pixels * 4 : nullptr;
	hipLaunchKernelGGL(ssx_sums_export_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_accum.as<const double>(),
	                   have_noise ? ctx->d_noise.as<const double>() : nullptr, d_sums, d_s2, pixel_grid(&p));
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(sums, d_sums, pixels * 4 * sizeof(double), hipMemcpyDeviceToHost));
	if (noise_s2) SSX_HIP(ctx, hipMemcpy(noise_s2, d_s2, pixels * sizeof(double), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_sums_import(ssx_ctx* ctx, const ssx_render_params* params, const ssx_sums_info_t* info, const double* sums, const double* noise_s2) {
	if (!ctx || !info || !sums) return SSX_ERR_ARG;
	if (info->struct_size != sizeof *info) return fail(ctx, SSX_ERR_ARG, "ssx_sums_info_t.struct_size mismatch");
	ssx_render_params given;
	if (params && params->struct_size == sizeof given && params->spp == 0) { given = *params; given.spp = 1; params = &given; } // (spp is ignored)
	ssx_render_params pp;
	int rc = begin_render(ctx, params, &pp, "render in progress");
	if (rc) return rc;
	auto differs = [&](const char* field, uint64_t mine, uint64_t theirs) {
		return fail(ctx, SSX_ERR_ARG, fmt("ssx_sums_import: %s differs (these sums: %llu, this render: %llu)", field, (unsigned long long)theirs, (unsigned long long)mine));
	};
	if (pp.width != info->width || pp.height != info->height)
		return fail(ctx, SSX_ERR_ARG, fmt("ssx_sums_import: size differs (these sums: %u x %u, this render: %u x %u)", info->width, info->height, pp.width, pp.height));
	if (pp.seed != info->seed) return differs("seed", pp.seed, info->seed);
	if ((pp.indirect_only != 0) != (info->indirect_only != 0)) return differs("indirect_only", pp.indirect_only, info->indirect_only);
	if ((pp.no_explicit_light_sampling != 0) != (info->no_explicit_light_sampling != 0)) return differs("no_explicit_light_sampling", pp.no_explicit_light_sampling, info->no_explicit_light_sampling);
	if ((pp.no_flat_field_correction != 0) != (info->no_flat_field_correction != 0)) return differs("no_flat_field_correction", pp.no_flat_field_correction, info->no_flat_field_correction);
	if (pp.libm != info->libm) return differs("libm", pp.libm, info->libm);
	if ((ctx->rgb_mode ? 1u : 0u) != (info->rgb_mode ? 1u : 0u)) return differs("rgb_mode", ctx->rgb_mode ? 1u : 0u, info->rgb_mode);
	{ // The sums are +0 where their exporter owned nothing: every tile this context is to own must have been the exporter's (a merged
	  // checkpoint: all of them; one rank's export: only a partition inside its own).
		const uint32_t tiles_x = tiles_across(pp.width), n_tiles = tiles_x * tiles_across(pp.height);
		if (info->tile_stride == 0 || info->tile_first >= info->tile_stride) return fail(ctx, SSX_ERR_ARG, "ssx_sums_import: tile_first / tile_stride of these sums are invalid");
		const SsxPixelGrid mine = pixel_grid(&pp), theirs{ pp.width, pp.height, tiles_x, info->tile_first, info->tile_stride, info->tile_skew % tiles_x };
		for (uint32_t t = 0; info->tile_stride > 1u && t < n_tiles; ++t) {
			const uint32_t i = (t % tiles_x) * 8u, j = (t / tiles_x) * 8u;
			if (ssx_owns_pixel(mine, i, j) && !ssx_owns_pixel(theirs, i, j))
				return fail(ctx, SSX_ERR_ARG, fmt("ssx_sums_import: tile ownership differs: these sums hold the tiles of tile_first %u / tile_stride %u / tile_skew %u only, this render "
				                                  "owns tile %u outside them (merge the ranks' exports by ownership first)", info->tile_first, info->tile_stride, info->tile_skew, t));
		}
	}
	if (ctx->scene_digest != info->scene_digest)
		return fail(ctx, SSX_ERR_ARG, fmt("ssx_sums_import: scene_digest differs (these sums: %016llx, the uploaded scene: %016llx)", (unsigned long long)info->scene_digest, (unsigned long long)ctx->scene_digest));
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	pp.spp = info->done_spp ? info->done_spp : 1u;
	if ((rc = ready_to_launch(ctx, &pp, true))) return rc;
	sums_invalidate(ctx);
	ctx->spectral_note = "the sums came from ssx_sums_import, which carries no spectral state (ssx_spectral_import puts the bins of the same samples next to them)";
	const size_t pixels = (size_t)pp.width * pp.height;
	const bool s2_given = noise_s2 && info->noise_batches;
	DeviceBuffer& stage = ctx->d_stage;
	SSX_HIP(ctx, stage.reserve(pixels * 5 * sizeof(double)));
	double* const d_sums = stage.as<double>(), * const d_s2 = s2_given ? d_sums + pixels * 4 : nullptr;
	SSX_HIP(ctx, hipMemcpyAsync(d_sums, sums, pixels * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (d_s2) SSX_HIP(ctx, hipMemcpyAsync(d_s2, noise_s2, pixels * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	if (ctx->noise_on) SSX_HIP(ctx, ctx->d_noise.reserve(noise_bytes(&pp)));
	if ((rc = clear_sums(ctx, pp.width, pp.height, ctx->stream))) return rc;
	hipLaunchKernelGGL(ssx_sums_import_kernel, pixel_blocks(&pp), dim3(256), 0, ctx->stream, ctx->d_accum.as<double>(),
	                   ctx->noise_on ? ctx->d_noise.as<double>() : nullptr, d_sums, d_s2, pixel_grid(&pp), info->done_spp);
	SSX_HIP(ctx, hipGetLastError());
	if ((rc = launch_finalize(ctx, &pp, pp.spp, ctx->d_out.as<float>(), ctx->stream))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	ctx->cur = pp;
	ctx->total_spp = 0; ctx->k_begin = 0;
	ctx->done_tiles.store(0);
	sums_publish(ctx, info->done_spp, !ctx->noise_on ? -1 : s2_given ? (int64_t)info->noise_batches : (info->done_spp ? 1 : 0)); // (the kernel made one batch of sums without S2)
	ctx->sums.imported = true;
	return SSX_OK;
}

int ssx_set_noise_estimate(ssx_ctx* ctx, int enable) {
	if (!ctx) return SSX_ERR_ARG;
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	ctx->noise_on = enable != 0;
	if (!ctx->noise_on) noise_drop(ctx);
	return SSX_OK;
}

int ssx_noise_info(ssx_ctx* ctx, double* v_out, double summary[4]) {
	if (!ctx || !summary) return SSX_ERR_ARG;
	if (!ctx->noise_on) return fail(ctx, SSX_ERR_STATE, "ssx_noise_info: the noise estimate is off (ssx_set_noise_estimate)");
	int rc = sums_ready(ctx, "ssx_noise_info");
	if (rc) return rc;
	if (!ctx->sums.noise_valid || ctx->sums.noise_batches < 2u) return fail(ctx, SSX_ERR_STATE, fmt("ssx_noise_info: %u batch(es) so far; the between-batch variance needs two", ctx->sums.noise_valid ? ctx->sums.noise_batches : 0u));
	const ssx_render_params& p = ctx->cur;
	const size_t pixels = (size_t)p.width * p.height;
	const double N = (double)ctx->done_spp.load(), B = (double)ctx->sums.noise_batches;
	DeviceBuffer& stage = ctx->d_stage;
	SSX_HIP(ctx, stage.reserve(pixels * 2 * sizeof(double)));
	hipLaunchKernelGGL(ssx_noise_variance_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_accum.as<const double>(), ctx->d_noise.as<const double>(),
	                   stage.as<double>(), stage.as<double>() + pixels, pixel_grid(&p), N, B);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<double> va(pixels * 2);
	SSX_HIP(ctx, hipMemcpy(va.data(), stage.ptr, pixels * 2 * sizeof(double), hipMemcpyDeviceToHost));
	const SsxPixelGrid g = pixel_grid(&p);
	double sum_v = 0.0, sum_mean = 0.0, owned = 0.0;
	for (uint32_t j = 0; j < p.height; ++j) for (uint32_t i = 0; i < p.width; ++i) { // one after the other, row-major
		if (!ssx_owns_pixel(g, i, j)) continue;
		const size_t q = (size_t)j * p.width + i;
		sum_v += va[q]; sum_mean += va[pixels + q] / N; owned += 1.0;
	}
	if (v_out) memcpy(v_out, va.data(), pixels * sizeof(double));
	summary[0] = sum_v; summary[1] = sum_mean; summary[2] = owned; summary[3] = B;
	return SSX_OK;
}

} // extern "C"

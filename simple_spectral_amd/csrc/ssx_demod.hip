// ssx_demod.hip -- demodulated denoising (include/ssx.h, "Demodulated denoising"): the filter of ssx_denoise.hip run on illumination -- radiance divided by the
// first-hit albedo, bin by bin -- with the albedo multiplied back afterwards.  Part of ssx_api.hip's translation unit (included behind ssx_denoise.hip and
// ssx_develop.hip, whose state, buffers and launch helpers it uses).  The three a-trous kernels are launched as they are, on other inputs: launch_atrous gets
// the demodulated image, variance and channels and an all-zero albedo guide.  Nothing here touches the generate, path or finalize kernels, and nothing here
// runs or is allocated unless one of the entry points at the end is called.

// The albedo bins rho[p][b] (include/ssx.h "ALBEDO BINS").  One lane per pixel and pair of sub-bins, the scene tables staged as ssx_guides_kernel stages them;
// K x K rays through the pixel (rows outer, columns inner), each traced by the generic trace with no quad ignored -- every lane of a wave runs it (it wants
// uniform control flow): lanes past the end redo the last pixel and store nothing, and the ray loop's bounds are a kernel argument.  Per ray and sub-bin m one
// call of material_albedo gives the four bins i * M + m.  blockIdx.y selects the MC consecutive sub-bins m0 .. m0 + MC - 1 a workgroup handles (one m0 per
// workgroup: uniform); MC is a template parameter and both loops over the 4 MC sums are unrolled, so every index is static and the sums are registers (a
// run-time m would send the array to scratch).  MC = 2 for an even M, 1 for an odd one.  Every pair traces the pixel's rays again: keeping all B sums of a
// pixel in one lane (MC = M) was tried first and does not fit -- at four waves per SIMD (128 registers) the instances MC = 4, 8 and 16 spilled 23, 71 and more
// registers to 96 .. 288 bytes of scratch, MC = 2 takes exactly 128 and MC = 1 115 (tools/kernel_resources.py; profiles/r16/NOTES.md) -- and the bins are
// computed once per scene and size.  amdgpu_waves_per_eu(4) holds both instances to those 128 registers.
// Output: planar in groups of four, rho[group][pixel] as float4 -- the layout of the filter's channel buffers, group g = bins 4 g .. 4 g + 3; a lane stores its
// 4 MC floats into four of those groups.
template <int MC>
__device__ __forceinline__ void albedo_bins_body(const SsxKernelArgs& a, float* __restrict__ rho, uint32_t K, uint32_t M) {
	Lds L; L.w = stage_lds(a);
	const SsxBlobHeader& h = L.hdr();
	const uint32_t n = a.width * a.height, gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t p = gid < n ? gid : n - 1u;
	const uint32_t i = p % a.width, j = p / a.width;
	const V3 cam = mk(h.cam_pos[0], h.cam_pos[1], h.cam_pos[2]);
	const uint32_t m0 = blockIdx.y * (uint32_t)MC;
	const float sub_step = h.lambda_step / (float)M;
	float acc[4 * MC];
#pragma unroll
	for (int b = 0; b < 4 * MC; ++b) acc[b] = 0.0f;
	for (uint32_t ry = 0; ry < K; ++ry) {
		for (uint32_t rx = 0; rx < K; ++rx) {
			double dx, dy, dz;
			camera_dir(h, a, (double)i + ((double)rx + 0.5) / (double)K, (double)j + ((double)ry + 0.5) / (double)K, dx, dy, dz);
			const double inv = 1.0 / __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
			const V3 dir = mk((float)(dx * inv), (float)(dy * inv), (float)(dz * inv));
			HitInfo hit;
			trace<0>(L, cam, dir, -1, true, hit);
			const bool got = hit.tri >= 0;
			const uint32_t quad = got ? (uint32_t)hit.tri >> 1 : 0u, which = got ? (uint32_t)hit.tri & 1u : 0u; // (a miss looks quad 0 up and adds +0)
			const SsxBlobQuad& Q = L.quad(quad);
			float st_x, st_y;
			hit_st(Q, which, hit, st_x, st_y);
			if (!got) { st_x = 0.0f; st_y = 0.0f; }
#pragma unroll
			for (int m = 0; m < MC; ++m) {
				const float lambda_0 = h.lambda_min + ((float)(m0 + (uint32_t)m) + 0.5f) * sub_step;
				const Hero al = material_albedo(L, Q, st_x, st_y, lambda_0);
#pragma unroll
				for (int s = 0; s < 4; ++s) acc[s * MC + m] = acc[s * MC + m] + (got ? al.v[s] : 0.0f);
			}
		}
	}
	if (gid >= n) return;
	const float rays = (float)(K * K);
#pragma unroll
	for (int s = 0; s < 4; ++s) {
#pragma unroll
		for (int m = 0; m < MC; ++m) {
			const uint32_t b = (uint32_t)s * M + m0 + (uint32_t)m; // component b & 3 of group b / 4
			rho[((size_t)(b >> 2) * n + p) * 4u + (b & 3u)] = acc[s * MC + m] / rays;
		}
	}
}
#define SSX_ALBEDO_BINS_KERNEL(M) \
	extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) ssx_albedo_bins_kernel_m##M(SsxKernelArgs a, float* rho, uint32_t K, uint32_t sub_bins) { albedo_bins_body<M>(a, rho, K, sub_bins); }
SSX_ALBEDO_BINS_KERNEL(1)
SSX_ALBEDO_BINS_KERNEL(2)
#undef SSX_ALBEDO_BINS_KERNEL

__device__ __forceinline__ float4 ssx_floor4(const float4 r, float f) { return make_float4(r.x > f ? r.x : f, r.y > f ? r.y : f, r.z > f ? r.z : f, r.w > f ? r.w : f); }

// What the per-pixel kernels below share: the render's image and variance (they decide which pixels are valid, and are never written), the albedo bins and
// the channel albedo r~_c (x, y, z; w is 1).
struct SsxDemodArgs {
	const float4* c; const float* var;   // the inputs of the filter before demodulation
	const float4* rho;                   // [B / 4][pixels]
	const float4* rc;                    // [pixels]: max(rho_c, floor) (ssx_demod_channel_albedo_kernel)
	uint32_t pixels, M;
	float floor;
};

// e0'[b] = e0[b] / max(rho[p][b], floor) for the B sum channels, in place on the first B / 4 groups; the count channels behind them and invalid pixels stay as
// they are.  One lane per float4: 16-byte coalesced loads of e and rho, one store.
extern "C" __global__ void __launch_bounds__(256) ssx_demod_channels_kernel(SsxDemodArgs a, float4* e) {
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= a.pixels * a.M) return;
	const uint32_t p = idx % a.pixels;
	if (!ssx_denoise_valid(a.c[p], a.var[p])) return;
	const float4 r = ssx_floor4(a.rho[idx], a.floor), v = e[idx];
	e[idx] = make_float4(v.x / r.x, v.y / r.y, v.z / r.z, v.w / r.w);
}

// r~_c[p] = max(num[p][k] / den[k], floor) for k = X, Y, Z (num by the develop images kernel from the row-major albedo bins), w = 1.  One lane per pixel.  It
// depends on the albedo bins, Wc and the floor only, so it runs when one of them changes, not per call (demod_channel_albedo).
extern "C" __global__ void __launch_bounds__(256) ssx_demod_channel_albedo_kernel(const float* num, float den_x, float den_y, float den_z, float floor, float4* rc, uint32_t pixels) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= pixels) return;
	const float4 r = ssx_floor4(make_float4(num[3u * (size_t)p] / den_x, num[3u * (size_t)p + 1u] / den_y, num[3u * (size_t)p + 2u] / den_z, 1.0f), floor);
	rc[p] = make_float4(r.x, r.y, r.z, 1.0f);
}

// c'[k] = c[k] / r~_c[k] for X, Y, Z, alpha as it is; var' = var / (r~_c[1] * r~_c[1]).  An invalid pixel keeps c and var.  One lane per pixel.
extern "C" __global__ void __launch_bounds__(256) ssx_demod_image_kernel(SsxDemodArgs a, float4* c_out, float* var_out) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= a.pixels) return;
	const float4 r = a.rc[p];
	const float4 c = a.c[p];
	const float v = a.var[p];
	const bool valid = ssx_denoise_valid(c, v);
	c_out[p] = valid ? make_float4(c.x / r.x, c.y / r.y, c.z / r.z, c.w) : c;
	var_out[p] = valid ? v / (r.y * r.y) : v;
}

// The remodulating twin of ssx_spectral_ratio_kernel: out[p][b] = eL[B + b % M] > 0 ? (eL[b] / eL[B + b % M]) * max(rho[p][b], floor) : 0, row-major
// [height][width][B]; a pixel that was invalid on input was not divided and is not multiplied.  One lane per float.
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_ratio_remod_kernel(SsxDemodArgs a, const float4* e, float* out) {
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x, B = 4u * a.M;
	if (idx >= a.pixels * B) return;
	const uint32_t p = idx / B, b = idx % B;
	const float den = ssx_channel(e, a.pixels, p, B + b % a.M);
	const float rho = ssx_channel(a.rho, a.pixels, p, b);
	const float r = ssx_denoise_valid(a.c[p], a.var[p]) ? (rho > a.floor ? rho : a.floor) : 1.0f;
	out[idx] = den > 0.0f ? (ssx_channel(e, a.pixels, p, b) / den) * r : 0.0f;
}

// c_out[k] = cL[k] * r~_c[k], alpha as it is; var_out = varL * (r~_c[1] * r~_c[1]); a pixel that was invalid on input keeps cL and varL.  One lane per pixel.
extern "C" __global__ void __launch_bounds__(256) ssx_remod_image_kernel(SsxDemodArgs a, const float4* cL, const float* varL, float4* c_out, float* var_out) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= a.pixels) return;
	const float4 c = cL[p], r = a.rc[p];
	const float v = varL[p];
	const bool valid = ssx_denoise_valid(a.c[p], a.var[p]);
	c_out[p] = valid ? make_float4(c.x * r.x, c.y * r.y, c.z * r.z, c.w) : c;
	var_out[p] = valid ? v * (r.y * r.y) : v;
}

namespace {

// supersample in {1, 2, 4}, the floor finite and positive; a NULL pointer gives the defaults
constexpr uint32_t kDemodDefaultSupersample = 2;
constexpr float kDemodDefaultFloor = SSX_DEMOD_DEFAULT_FLOOR, kDemodDefaultSigmaL = SSX_DEMOD_DEFAULT_SIGMA_L;
int demod_check_supersample(ssx_ctx* ctx, const char* what, uint32_t K) {
	return (K == 1u || K == 2u || K == 4u) ? SSX_OK : fail(ctx, SSX_ERR_ARG, fmt("%s: supersample = %u: need 1, 2 or 4", what, K));
}
int demod_take_params(ssx_ctx* ctx, const ssx_demod_params* in, ssx_demod_params* out) {
	out->struct_size = sizeof *out; out->supersample = kDemodDefaultSupersample; out->albedo_floor = kDemodDefaultFloor;
	if (!in) return SSX_OK;
	if (in->struct_size != sizeof *out) return fail(ctx, SSX_ERR_ARG, "ssx_demod_params.struct_size mismatch");
	*out = *in;
	if (const int rc = demod_check_supersample(ctx, "ssx_demod_params", out->supersample)) return rc;
	if (!(out->albedo_floor > 0.0f) || !std::isfinite(out->albedo_floor)) return fail(ctx, SSX_ERR_ARG, "ssx_demod_params.albedo_floor must be finite and positive");
	return SSX_OK;
}
// The filter's parameters in this mode: sigma_a is ignored (the albedo guide is zero: wa is exactly 1), and a NULL pointer gives the mode's own sigma_l.
int demod_take_denoise_params(ssx_ctx* ctx, const ssx_denoise_params* in, ssx_denoise_params* out) {
	if (!in) { const int rc = denoise_take_params(ctx, nullptr, out); out->sigma_l = kDemodDefaultSigmaL; return rc; }
	if (in->struct_size != sizeof *out) return fail(ctx, SSX_ERR_ARG, "ssx_denoise_params.struct_size mismatch");
	ssx_denoise_params p = *in;
	p.sigma_a = 1.0f;
	return denoise_take_params(ctx, &p, out);
}

// d_albedo_bins: rho planar [B / 4][pixels] float4 | the same row-major [pixels][B] (what ssx_albedo_bins returns and the develop images kernel reads)
struct AlbedoBins { float4* planar; float* rows; };
AlbedoBins albedo_bins_of(const ssx_ctx* ctx, size_t pixels, uint32_t B) {
	float4* const base = ctx->d_albedo_bins.as<float4>();
	return AlbedoBins{ base, reinterpret_cast<float*>(base + pixels * (B / 4u)) };
}

// The albedo bins of the uploaded scene at width x height, B bins, K x K rays per pixel, on the device (the context's device current, nothing queued by
// ssx_render_device): computed once per (scene upload, size, B, K) -- they depend on nothing else -- and kept until ssx_upload_scene or another request.
int ensure_albedo_bins(ssx_ctx* ctx, const char* what, uint32_t width, uint32_t height, uint32_t B, uint32_t K) {
	if (ctx->rgb_mode) return fail(ctx, SSX_ERR_STATE, fmt("%s: the scene is in SSX_MODE_RGB: there are no wavelength bins", what));
	if (ctx->abins_width == width && ctx->abins_height == height && ctx->abins_bins == B && ctx->abins_supersample == K) return SSX_OK;
	const size_t pixels = (size_t)width * height;
	int rc = channels_check_size(ctx, pixels, B, what);
	if (rc) return rc;
	ctx->abins_width = ctx->abins_height = 0;
	SSX_HIP(ctx, ctx->d_albedo_bins.reserve(pixels * B * 2u * sizeof(float)));
	const AlbedoBins ab = albedo_bins_of(ctx, pixels, B);
	SsxKernelArgs a{};
	a.blob = ctx->d_blob.as<uint32_t>(); a.blob_words = ctx->blob_words; a.rgb_mode = 0u;
	a.width = width; a.height = height;
	a.inv_width = 1.0 / (double)width; a.inv_height = 1.0 / (double)height;
	const dim3 grid = blocks_of(pixels), block(256);
	const size_t lds = staged_blob_lds(ctx->blob_words);
	float* const rho = reinterpret_cast<float*>(ab.planar);
	const uint32_t M = B / 4u;
	if (M & 1u) hipLaunchKernelGGL(ssx_albedo_bins_kernel_m1, dim3(grid.x, M), block, lds, ctx->stream, a, rho, K, M);
	else hipLaunchKernelGGL(ssx_albedo_bins_kernel_m2, dim3(grid.x, M / 2u), block, lds, ctx->stream, a, rho, K, M);
	SSX_HIP(ctx, hipGetLastError());
	hipLaunchKernelGGL(ssx_channels_unpack_kernel, blocks_of(pixels * B), block, 0, ctx->stream, ab.planar, ab.rows, (uint32_t)pixels, B);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	ctx->abins_width = width; ctx->abins_height = height; ctx->abins_bins = B; ctx->abins_supersample = K;
	++ctx->abins_serial;
	return SSX_OK;
}

// d_demod: W_dev (4 KB: the channel weights as the develop kernels read them) | rc | c' | zero albedo | c_out (float4 [pixels] each) | var' | var_out | num [pixels][3]
struct DemodBuffers { float* W; float4* rc; float4* c; float4* zero; float4* c_out; float* var; float* var_out; float* num; };
int demod_buffers(ssx_ctx* ctx, size_t pixels, DemodBuffers* d) {
	SSX_HIP(ctx, ctx->d_demod.reserve(kDevelopWeightBytes + pixels * (4u * 16u + 5u * 4u)));
	uint8_t* const base = ctx->d_demod.as<uint8_t>();
	d->W = reinterpret_cast<float*>(base);
	float4* const f4 = reinterpret_cast<float4*>(base + kDevelopWeightBytes);
	d->rc = f4; d->c = f4 + pixels; d->zero = f4 + 2u * pixels; d->c_out = f4 + 3u * pixels;
	float* const f1 = reinterpret_cast<float*>(f4 + 4u * pixels);
	d->var = f1; d->var_out = f1 + pixels; d->num = f1 + 2u * pixels;
	return SSX_OK;
}

// den[c] = the develop accumulation of all ones with Wc[c][.]: acc = 0.0f; acc = acc + (1.0f * Wc[c][b]) for ascending b
int demod_denominators(ssx_ctx* ctx, const char* what, const float* weights_xyz, uint32_t B, float den[3]) {
	for (uint32_t c = 0; c < 3u; ++c) {
		volatile float acc = 0.0f;
		for (uint32_t b = 0; b < B; ++b) acc = acc + weights_xyz[(size_t)c * B + b];
		den[c] = acc;
		if (!(den[c] > 0.0f)) return fail(ctx, SSX_ERR_ARG, fmt("%s: weights_xyz row %u sums to %g: the channel albedo needs a positive denominator", what, c, (double)den[c]));
	}
	return SSX_OK;
}

// d.rc = r~_c and d.zero = the all-zero albedo guide.  Both depend on (albedo bins, Wc, floor, size) only, so they are made when one of those changes -- the
// upload of Wc as the develop kernels read it, the develop of the row-major bins into num, the division and the floor, the memset -- and kept in d_demod for the
// calls that follow (ctx->demod_rc_*: what they were made from; a new allocation of d_demod or newly computed albedo bins drop them).
int demod_channel_albedo(ssx_ctx* ctx, const float* weights_xyz, const float den[3], float floor, size_t pixels, uint32_t B, const AlbedoBins& ab, const DemodBuffers& d) {
	const std::vector<float> wc(weights_xyz, weights_xyz + (size_t)3u * B);
	if (ctx->demod_rc_base == ctx->d_demod.ptr && ctx->demod_rc_bins_serial == ctx->abins_serial && ctx->demod_rc_floor == floor && ctx->demod_rc_weights == wc) return SSX_OK;
	ctx->demod_rc_base = nullptr;
	std::vector<float> w((size_t)B * 4u, 0.0f); // W_dev[b][4], the fourth channel zero (develop_buffers' layout at G = 1)
	for (uint32_t c = 0; c < 3u; ++c) for (uint32_t k = 0; k < B; ++k) w[(size_t)k * 4u + c] = wc[(size_t)c * B + k];
	SSX_HIP(ctx, hipMemcpy(d.W, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice)); // (blocking: `w` goes out of scope)
	SsxDevelopArgs da{};
	da.q = ab.rows; da.W = d.W; da.out = d.num;
	da.B = B; da.C = 3u; da.pixels = (uint32_t)pixels;
	if (const int rc = launch_develop_images(ctx, da)) return rc;
	hipLaunchKernelGGL(ssx_demod_channel_albedo_kernel, blocks_of(pixels), dim3(256), 0, ctx->stream, d.num, den[0], den[1], den[2], floor, d.rc, (uint32_t)pixels);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipMemsetAsync(d.zero, 0, pixels * sizeof(float4), ctx->stream));
	ctx->demod_rc_base = ctx->d_demod.ptr; ctx->demod_rc_bins_serial = ctx->abins_serial; ctx->demod_rc_floor = floor; ctx->demod_rc_weights = wc;
	return SSX_OK;
}

// The device part of ssx_denoise_spectral_demod, shared with ssx_spectral_develop_demod, after denoise_own_state_ready(.., true): albedo bins, channel albedo,
// the divide, the L levels on the demodulated inputs with a zero albedo guide, the multiply; all queued on the context's stream.  On return (not yet waited
// for) the image and variance are in d->c_out / d->var_out and out[p][b], row-major [height][width][B], in cb->stage.
int denoise_spectral_demod_device(ssx_ctx* ctx, const char* what, const ssx_denoise_params& dp, const ssx_demod_params& dm, const float* weights_xyz, DemodBuffers* d, ChannelBuffers* cb) {
	const ssx_render_params& p = ctx->cur;
	const size_t pixels = (size_t)p.width * p.height;
	const uint32_t B = ctx->spectral_bins, M = B / 4u;
	float den[3];
	int rc = demod_denominators(ctx, what, weights_xyz, B, den);
	if (rc) return rc;
	if ((rc = channels_check_size(ctx, pixels, B + M, what))) return rc;
	if ((rc = ensure_albedo_bins(ctx, what, p.width, p.height, B, dm.supersample))) return rc;
	DenoiseBuffers b;
	if ((rc = denoise_own_inputs(ctx, &b))) return rc;
	if ((rc = channel_buffers(ctx, pixels, B + M, B, cb))) return rc;
	if ((rc = demod_buffers(ctx, pixels, d))) return rc;
	const AlbedoBins ab = albedo_bins_of(ctx, pixels, B);
	if ((rc = demod_channel_albedo(ctx, weights_xyz, den, dm.albedo_floor, pixels, B, ab, *d))) return rc;
	hipLaunchKernelGGL(ssx_spectral_channels_kernel, blocks_of(pixels * cb->groups), dim3(256), 0, ctx->stream, ctx->d_spectral_sums.as<const double>(),
	                   ctx->d_spectral_counts.as<const uint32_t>(), cb->e[0], pixel_grid(&p), M, (double)ctx->done_spp.load());
	SSX_HIP(ctx, hipGetLastError());
	const SsxDemodArgs a{ ctx->d_out.as<const float4>(), b.var_in, ab.planar, d->rc, (uint32_t)pixels, M, dm.albedo_floor };
	hipLaunchKernelGGL(ssx_demod_channels_kernel, blocks_of(pixels * M), dim3(256), 0, ctx->stream, a, cb->e[0]);
	SSX_HIP(ctx, hipGetLastError());
	hipLaunchKernelGGL(ssx_demod_image_kernel, blocks_of(pixels), dim3(256), 0, ctx->stream, a, d->c, d->var);
	SSX_HIP(ctx, hipGetLastError());
	const SsxGuides g = guides_of(ctx, pixels);
	if ((rc = launch_atrous(ctx, dp, p.width, p.height, d->c, d->var, g.prim, d->zero, b, cb))) return rc;
	const uint32_t last = (dp.levels - 1u) & 1u;
	hipLaunchKernelGGL(ssx_spectral_ratio_remod_kernel, blocks_of(pixels * B), dim3(256), 0, ctx->stream, a, cb->e[dp.levels & 1u], cb->stage);
	SSX_HIP(ctx, hipGetLastError());
	hipLaunchKernelGGL(ssx_remod_image_kernel, blocks_of(pixels), dim3(256), 0, ctx->stream, a, b.c[last], b.var[last], d->c_out, d->var_out);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

// What both state entry points check and take before they touch the device
int demod_begin(ssx_ctx* ctx, const char* what, const ssx_denoise_params* params, const ssx_demod_params* demod, const float* weights_xyz, ssx_denoise_params* dp, ssx_demod_params* dm) {
	int rc = demod_take_denoise_params(ctx, params, dp);
	if (rc) return rc;
	if ((rc = demod_take_params(ctx, demod, dm))) return rc;
	if (!weights_xyz) return fail(ctx, SSX_ERR_ARG, fmt("%s: weights_xyz must not be NULL", what));
	return denoise_own_state_ready(ctx, what, true);
}

} // namespace

extern "C" {

int ssx_albedo_bins(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, uint32_t supersample, float* rho_out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_albedo_bins";
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	int rc = idle_on_device(ctx);
	if (rc) return rc;
	if (bins < 4u || bins > 64u || (bins & 3u)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if ((rc = demod_check_supersample(ctx, what, supersample))) return rc;
	if ((rc = denoise_check_size(ctx, width, height, what))) return rc;
	if ((rc = ensure_albedo_bins(ctx, what, width, height, bins, supersample))) return rc;
	const size_t pixels = (size_t)width * height;
	if (rho_out) SSX_HIP(ctx, hipMemcpy(rho_out, albedo_bins_of(ctx, pixels, bins).rows, pixels * bins * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_denoise_spectral_demod(ssx_ctx* ctx, const ssx_denoise_params* params, const ssx_demod_params* demod, const float* weights_xyz, float* mean_out, float* xyza_out, float* var_out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_denoise_spectral_demod";
	ssx_denoise_params dp;
	ssx_demod_params dm;
	int rc = demod_begin(ctx, what, params, demod, weights_xyz, &dp, &dm);
	if (rc) return rc;
	const size_t pixels = (size_t)ctx->cur.width * ctx->cur.height;
	DemodBuffers d;
	ChannelBuffers cb;
	if ((rc = denoise_spectral_demod_device(ctx, what, dp, dm, weights_xyz, &d, &cb))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (xyza_out) SSX_HIP(ctx, hipMemcpy(xyza_out, d.c_out, pixels * sizeof(float4), hipMemcpyDeviceToHost));
	if (var_out) SSX_HIP(ctx, hipMemcpy(var_out, d.var_out, pixels * sizeof(float), hipMemcpyDeviceToHost));
	if (mean_out) SSX_HIP(ctx, hipMemcpy(mean_out, cb.stage, pixels * ctx->spectral_bins * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_spectral_develop_demod(ssx_ctx* ctx, const ssx_denoise_params* denoise, const ssx_demod_params* demod, const float* weights_xyz, const float* weights, uint32_t channels, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_develop_demod";
	int rc = develop_check(ctx, what, channels, weights);
	if (rc) return rc;
	ssx_denoise_params dp;
	ssx_demod_params dm;
	if ((rc = demod_begin(ctx, what, denoise, demod, weights_xyz, &dp, &dm))) return rc;
	const size_t pixels = (size_t)ctx->cur.width * ctx->cur.height;
	const uint32_t B = ctx->spectral_bins;
	DevelopBuffers dv;
	if ((rc = develop_buffers(ctx, pixels, B, channels, weights, 0, &dv))) return rc;
	DemodBuffers d;
	ChannelBuffers cb;
	if ((rc = denoise_spectral_demod_device(ctx, what, dp, dm, weights_xyz, &d, &cb))) return rc;
	SsxDevelopArgs a{};
	a.q = cb.stage; a.W = dv.W; a.out = dv.out; // the remodulated ratio, developed where it lies
	a.B = B; a.C = channels; a.pixels = (uint32_t)pixels;
	if ((rc = launch_develop_images(ctx, a))) return rc;
	return develop_read_back(ctx, dv, pixels, channels, out);
}

} // extern "C"

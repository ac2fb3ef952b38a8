// ssx_denoise.hip -- first-hit guide buffers and the variance-guided edge-stopping a-trous filter (include/ssx.h, "Denoising").  Part of ssx_api.hip's
// translation unit (included behind its context and launch helpers, like ssx_progressive.hip and ssx_spectral.hip).  Nothing here touches the generate,
// path or finalize kernels, and nothing here runs or is allocated unless one of the three entry points at the end is called.

// What the per-pixel kernels below write and read: one array per quantity, pixel p = j * width + i (row 0 = bottom).
struct SsxGuides { uint32_t* prim; float* depth; float* normal /* [p][3] */; float4* albedo; };

// One lane per pixel of the whole image: the camera ray through the pixel centre (camera_dir and the normalisation of generate_sample, no random number),
// its closest hit by the generic trace (the device function behind SSX_DBG_TRACE, no quad ignored) and the albedo there (the one behind SSX_DBG_ALBEDO) at
// lambda_g = lambda_min + 0.5f * lambda_step (0 in RGB mode).  The scene tables are staged as ssx_debug_eval stages them.  Every lane of a wave runs the
// trace (it wants uniform control flow): lanes past the end redo the last pixel and store nothing.
extern "C" __global__ void __launch_bounds__(256) ssx_guides_kernel(SsxKernelArgs a, SsxGuides out) {
	Lds L; L.w = stage_lds(a);
	const SsxBlobHeader& h = L.hdr();
	const uint32_t n = a.width * a.height, gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t p = gid < n ? gid : n - 1u;
	const uint32_t i = p % a.width, j = p / a.width;
	double dx, dy, dz;
	camera_dir(h, a, (double)i + 0.5, (double)j + 0.5, dx, dy, dz);
	const double inv = 1.0 / __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
	const V3 dir = mk((float)(dx * inv), (float)(dy * inv), (float)(dz * inv));
	HitInfo hit;
	trace<0>(L, mk(h.cam_pos[0], h.cam_pos[1], h.cam_pos[2]), dir, -1, true, hit);
	const bool got = hit.tri >= 0;
	const uint32_t quad = got ? (uint32_t)hit.tri >> 1 : 0u, which = got ? (uint32_t)hit.tri & 1u : 0u; // (a miss looks quad 0 up and drops the result)
	const SsxBlobQuad& Q = L.quad(quad);
	float st_x, st_y;
	hit_st(Q, which, hit, st_x, st_y);
	const float lambda_g = a.rgb_mode ? 0.0f : h.lambda_min + 0.5f * h.lambda_step;
	const Hero al = material_albedo(L, Q, got ? st_x : 0.0f, got ? st_y : 0.0f, lambda_g);
	if (gid >= n) return;
	out.prim[p] = got ? quad : 0xFFFFFFFFu;
	out.depth[p] = got ? hit.dist : 0.0f;
	out.normal[3u * (size_t)p + 0u] = got ? Q.normal[which][0] : 0.0f;
	out.normal[3u * (size_t)p + 1u] = got ? Q.normal[which][1] : 0.0f;
	out.normal[3u * (size_t)p + 2u] = got ? Q.normal[which][2] : 0.0f;
	out.albedo[p] = got ? make_float4(al.v[0], al.v[1], al.v[2], al.v[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// v = ((S2 - A*A/N) / (B-1)) / N, clamped at 0, of owned pixel (i, j) = p: the expression of ssx_noise_variance_kernel (ssx_progressive.hip), which stays as it
// is; tests/test_denoise_gpu.py holds ssx_denoise against ssx_denoise_images fed with ssx_noise_info's v, bit for bit.
__device__ __forceinline__ double ssx_noise_variance(const double* accum, const double* noise, const SsxPixelGrid& g, uint32_t i, uint32_t j, uint32_t p, double N, double B) {
	const double a = accum[ssx_sum_slot(i, j, g.tiles_x) + 64u];
	double v = ((noise[(size_t)g.width * g.height + p] - a * a / N) / (B - 1.0)) / N;
	if (!(v > 0.0)) v = 0.0;
	return v;
}

// The noise estimate's variance of the pixel mean in image units: var = (float)(v * scale2), scale2 = s * s with s
// the factor ssx_finalize_kernel applies to A / N (1000, or 1 in RGB mode); the product is binary64.  The whole image is owned (ssx_denoise checks).
extern "C" __global__ void __launch_bounds__(256) ssx_denoise_var_kernel(const double* accum, const double* noise, float* var, SsxPixelGrid g, double N, double B, double scale2) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= g.width * g.height) return;
	const double v = ssx_noise_variance(accum, noise, g, p % g.width, p / g.width, p, N, B);
	var[p] = (float)(v * scale2);
}

// One level of the filter.
struct SsxAtrousArgs {
	const float4* c; const float* var; const uint32_t* prim; const float4* albedo; // what the level reads: the previous level's c and var, the guides
	float4* c_out; float* var_out;
	uint32_t width, height, step;   // step = 2^level
	float sigma_l, inv_sa2;         // inv_sa2 = 1.0f / (sigma_a * sigma_a), by the host (the same float division)
};

__device__ __forceinline__ bool ssx_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool ssx_denoise_valid(const float4 c, float var) { return ssx_finite(c.x) && ssx_finite(c.y) && ssx_finite(c.z) && ssx_finite(var); }

// A 16x16-pixel workgroup (4 waves), one lane per pixel, plain gather: a tap reads c and albedo as one 16-byte load each, prim and var as 4 bytes (40 bytes
// per tap, 25 taps and the 9 variance taps of g per pixel).  Neighbouring lanes read neighbouring pixels at every step, so a wave's tap is four 256-byte runs
// (c, albedo) and four 64-byte ones; the working set of a level -- 40 bytes per pixel, 10 MB at 512^2 -- stays in the L2 / MALL from one level to the next.
// No atomics, no barriers, no LDS.  Every operation is binary32 in the order include/ssx.h writes it, divisions and the square root IEEE, nothing contracted:
// tests/denoise_ref.py restates it in numpy and the results are compared bit for bit.
extern "C" __global__ void __launch_bounds__(256) ssx_atrous_kernel(SsxAtrousArgs a) {
	const int W = (int)a.width, H = (int)a.height;
	const int x = (int)(blockIdx.x * 16u + threadIdx.x), y = (int)(blockIdx.y * 16u + threadIdx.y);
	if (x >= W || y >= H) return;
	const size_t p = (size_t)y * a.width + (size_t)x;
	const float4 cp = a.c[p];
	const float vp = a.var[p];
	if (!ssx_denoise_valid(cp, vp)) { a.c_out[p] = cp; a.var_out[p] = vp; return; } // an invalid pixel keeps what it has, at every level
	// g: the 3x3 Gaussian of the variance over the valid neighbours at distance 1 (not `step`), centre included
	float gs = 0.0f, ks = 0.0f;
#pragma unroll
	for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
		for (int dx = -1; dx <= 1; ++dx) {
			const int qx = x + dx, qy = y + dy;
			if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
			const size_t q = (size_t)qy * a.width + (size_t)qx;
			const float vq = a.var[q];
			if (!ssx_denoise_valid(a.c[q], vq)) continue;
			const float k3 = (dy == 0 ? 2.0f : 1.0f) * (dx == 0 ? 2.0f : 1.0f);
			gs += k3 * vq; ks += k3;
		}
	}
	const float g = gs / ks;
	const float den = a.sigma_l * __builtin_sqrtf(g) + 1e-6f;
	const uint32_t prim_p = a.prim[p];
	const float4 al_p = a.albedo[p];
	const int step = (int)a.step;
	float sw = 0.0f, scx = 0.0f, scy = 0.0f, scz = 0.0f, sv = 0.0f;
	for (int dy = -2; dy <= 2; ++dy) {
		const int qy = y + step * dy;
		if (qy < 0 || qy >= H) continue;
		const float hy = dy == 0 ? 0.375f : ((dy == -1 || dy == 1) ? 0.25f : 0.0625f);
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + step * dx;
			if (qx < 0 || qx >= W) continue;
			const size_t q = (size_t)qy * a.width + (size_t)qx;
			if (a.prim[q] != prim_p) continue;
			const float4 cq = a.c[q];
			const float vq = a.var[q];
			if (!ssx_denoise_valid(cq, vq)) continue;
			const float4 al_q = a.albedo[q];
			const float hx = dx == 0 ? 0.375f : ((dx == -1 || dx == 1) ? 0.25f : 0.0625f);
			const float k = hy * hx;
			const float xl = __builtin_fabsf(cq.y - cp.y) / den;
			const float wl = 1.0f / (1.0f + xl * xl);
			const float d0 = al_q.x - al_p.x, d1 = al_q.y - al_p.y, d2 = al_q.z - al_p.z, d3 = al_q.w - al_p.w;
			const float da2 = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
			const float wa = 1.0f / (1.0f + da2 * a.inv_sa2);
			const float w = (k * wl) * wa;
			sw += w;
			scx += w * cq.x; scy += w * cq.y; scz += w * cq.z;
			sv += (w * w) * vq;
		}
	}
	a.c_out[p] = make_float4(scx / sw, scy / sw, scz / sw, cp.w); // (the centre tap always counts: sw >= 9/64)
	a.var_out[p] = sv / (sw * sw);
}

namespace {

constexpr uint32_t kDenoiseMaxLevels = 6;

// levels in 1..6, both sigmas finite and positive; a NULL pointer gives the defaults
int denoise_take_params(ssx_ctx* ctx, const ssx_denoise_params* in, ssx_denoise_params* out) {
	out->struct_size = sizeof *out; out->levels = 5u; out->sigma_l = 1.0f; out->sigma_a = 0.1f;
	if (!in) return SSX_OK;
	if (in->struct_size != sizeof *out) return fail(ctx, SSX_ERR_ARG, "ssx_denoise_params.struct_size mismatch");
	*out = *in;
	if (out->levels < 1u || out->levels > kDenoiseMaxLevels) return fail(ctx, SSX_ERR_ARG, fmt("ssx_denoise_params.levels = %u: need 1..%u", out->levels, kDenoiseMaxLevels));
	if (!(out->sigma_l > 0.0f) || !std::isfinite(out->sigma_l)) return fail(ctx, SSX_ERR_ARG, "ssx_denoise_params.sigma_l must be finite and positive");
	if (!(out->sigma_a > 0.0f) || !std::isfinite(out->sigma_a)) return fail(ctx, SSX_ERR_ARG, "ssx_denoise_params.sigma_a must be finite and positive");
	return SSX_OK;
}

int denoise_check_size(ssx_ctx* ctx, uint32_t width, uint32_t height, const char* what) {
	if (width == 0 || height == 0) return fail(ctx, SSX_ERR_ARG, fmt("%s: width and height must be positive", what));
	if ((uint64_t)width * height > (1ull << 28)) return fail(ctx, SSX_ERR_ARG, fmt("%s: image too large", what));
	return SSX_OK;
}

// d_guides: prim | depth | albedo | normal, `pixels` entries each (16-byte quantities at multiples of 16: pixels * 8 bytes precede albedo)
size_t guides_bytes(size_t pixels) { return ((pixels * 8u + 15u) & ~(size_t)15u) + pixels * 16u + pixels * 12u; }
SsxGuides guides_of(const ssx_ctx* ctx, size_t pixels) {
	uint8_t* const base = ctx->d_guides.as<uint8_t>();
	SsxGuides g;
	g.prim = reinterpret_cast<uint32_t*>(base);
	g.depth = reinterpret_cast<float*>(base + pixels * 4u);
	g.albedo = reinterpret_cast<float4*>(base + ((pixels * 8u + 15u) & ~(size_t)15u));
	g.normal = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(g.albedo) + pixels * 16u);
	return g;
}

// The guide buffers of the uploaded scene at width x height, on the device (the context's device current, nothing queued by ssx_render_device): computed
// once per (scene upload, size) -- they depend on nothing else -- and kept until ssx_upload_scene or another size.
int ensure_guides(ssx_ctx* ctx, uint32_t width, uint32_t height) {
	if (ctx->guides_width == width && ctx->guides_height == height) return SSX_OK;
	const size_t pixels = (size_t)width * height;
	ctx->guides_width = ctx->guides_height = 0;
	SSX_HIP(ctx, ctx->d_guides.reserve(guides_bytes(pixels)));
	SsxKernelArgs a{};
	a.blob = ctx->d_blob.as<uint32_t>(); a.blob_words = ctx->blob_words; a.rgb_mode = ctx->rgb_mode ? 1u : 0u;
	a.width = width; a.height = height;
	a.inv_width = 1.0 / (double)width; a.inv_height = 1.0 / (double)height;
	const size_t lds = ((size_t)ctx->blob_words + SSX_LDS_PREFIX_WORDS) * 4;
	hipLaunchKernelGGL(ssx_guides_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), lds, ctx->stream, a, guides_of(ctx, pixels));
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	ctx->guides_width = width; ctx->guides_height = height;
	return SSX_OK;
}

// d_denoise: the filter's working set, `pixels` entries per array: c_in | albedo_in | c[0] | c[1] (float4) | var_in | prim_in | var[0] | var[1] (4 bytes)
struct DenoiseBuffers { float4* c_in; float4* albedo_in; float4* c[2]; float* var_in; uint32_t* prim_in; float* var[2]; };
int denoise_buffers(ssx_ctx* ctx, size_t pixels, DenoiseBuffers* b) {
	SSX_HIP(ctx, ctx->d_denoise.reserve(pixels * 80u));
	float4* const f4 = ctx->d_denoise.as<float4>();
	b->c_in = f4; b->albedo_in = f4 + pixels; b->c[0] = f4 + 2u * pixels; b->c[1] = f4 + 3u * pixels;
	float* const f1 = reinterpret_cast<float*>(f4 + 4u * pixels);
	b->var_in = f1; b->prim_in = reinterpret_cast<uint32_t*>(f1 + pixels); b->var[0] = f1 + 2u * pixels; b->var[1] = f1 + 3u * pixels;
	return SSX_OK;
}

// The levels, one launch each, ping-pong between b.c / b.var[0] and [1]; none of the four inputs is written.  The result is in b.c / b.var[(levels - 1) & 1]
// once the stream has been waited for.
int launch_atrous(ssx_ctx* ctx, const ssx_denoise_params& dp, uint32_t width, uint32_t height, const float4* c, const float* var, const uint32_t* prim, const float4* albedo, const DenoiseBuffers& b) {
	SsxAtrousArgs a{};
	a.prim = prim; a.albedo = albedo;
	a.width = width; a.height = height;
	a.sigma_l = dp.sigma_l; a.inv_sa2 = 1.0f / (dp.sigma_a * dp.sigma_a);
	const dim3 grid((width + 15u) / 16u, (height + 15u) / 16u), block(16, 16);
	for (uint32_t l = 0; l < dp.levels; ++l) {
		a.c = l ? b.c[(l - 1u) & 1u] : c; a.var = l ? b.var[(l - 1u) & 1u] : var;
		a.c_out = b.c[l & 1u]; a.var_out = b.var[l & 1u];
		a.step = 1u << l;
		hipLaunchKernelGGL(ssx_atrous_kernel, grid, block, 0, ctx->stream, a);
		SSX_HIP(ctx, hipGetLastError());
	}
	return SSX_OK;
}

int denoise_read_back(ssx_ctx* ctx, const ssx_denoise_params& dp, size_t pixels, const DenoiseBuffers& b, float* xyza_out, float* var_out) {
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const uint32_t last = (dp.levels - 1u) & 1u;
	if (xyza_out) SSX_HIP(ctx, hipMemcpy(xyza_out, b.c[last], pixels * sizeof(float4), hipMemcpyDeviceToHost));
	if (var_out) SSX_HIP(ctx, hipMemcpy(var_out, b.var[last], pixels * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_guides(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t* prim, float* depth, float* normal, float* albedo) {
	if (!ctx) return SSX_ERR_ARG;
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	int rc = denoise_check_size(ctx, width, height, "ssx_guides");
	if (rc) return rc;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	if ((rc = ensure_guides(ctx, width, height))) return rc;
	const size_t pixels = (size_t)width * height;
	const SsxGuides g = guides_of(ctx, pixels);
	if (prim) SSX_HIP(ctx, hipMemcpy(prim, g.prim, pixels * 4u, hipMemcpyDeviceToHost));
	if (depth) SSX_HIP(ctx, hipMemcpy(depth, g.depth, pixels * 4u, hipMemcpyDeviceToHost));
	if (normal) SSX_HIP(ctx, hipMemcpy(normal, g.normal, pixels * 12u, hipMemcpyDeviceToHost));
	if (albedo) SSX_HIP(ctx, hipMemcpy(albedo, g.albedo, pixels * 16u, hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_denoise_images(ssx_ctx* ctx, const ssx_denoise_params* params, uint32_t width, uint32_t height, const float* xyza, const float* var,
                       const uint32_t* prim, const float* albedo, float* xyza_out, float* var_out) {
	if (!ctx) return SSX_ERR_ARG;
	if (!xyza || !var || !prim || !albedo || !xyza_out) return fail(ctx, SSX_ERR_ARG, "ssx_denoise_images: xyza, var, prim, albedo and xyza_out must not be NULL");
	ssx_denoise_params dp;
	int rc = denoise_take_params(ctx, params, &dp);
	if (rc) return rc;
	if ((rc = denoise_check_size(ctx, width, height, "ssx_denoise_images"))) return rc;
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	DenoiseBuffers b;
	if ((rc = denoise_buffers(ctx, pixels, &b))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(b.c_in, xyza, pixels * 16u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(b.albedo_in, albedo, pixels * 16u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(b.var_in, var, pixels * 4u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(b.prim_in, prim, pixels * 4u, hipMemcpyHostToDevice, ctx->stream));
	if ((rc = launch_atrous(ctx, dp, width, height, b.c_in, b.var_in, b.prim_in, b.albedo_in, b))) return rc;
	return denoise_read_back(ctx, dp, pixels, b, xyza_out, var_out);
}

int ssx_denoise(ssx_ctx* ctx, const ssx_denoise_params* params, float* xyza_out, float* var_out) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_denoise_params dp;
	int rc = denoise_take_params(ctx, params, &dp);
	if (rc) return rc;
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if ((rc = sums_ready(ctx, "ssx_denoise"))) return rc;
	if (!ctx->noise_on) return fail(ctx, SSX_ERR_STATE, "ssx_denoise: the noise estimate is off (ssx_set_noise_estimate): the filter is guided by its variance");
	if (!ctx->sums.noise_valid || ctx->sums.noise_batches < 2u)
		return fail(ctx, SSX_ERR_STATE, fmt("ssx_denoise: %u batch(es) so far; the between-batch variance needs two", ctx->sums.noise_valid ? ctx->sums.noise_batches : 0u));
	const ssx_render_params& p = ctx->cur;
	if (p.tile_stride != 1u) return fail(ctx, SSX_ERR_STATE, fmt("ssx_denoise: the context owns a part of the image only (tile_stride = %u): combine the ranks and use ssx_denoise_images", p.tile_stride));
	if (!ctx->d_out.ptr) return fail(ctx, SSX_ERR_STATE, "ssx_denoise: the context holds no image");
	if ((rc = ensure_guides(ctx, p.width, p.height))) return rc;
	const size_t pixels = (size_t)p.width * p.height;
	DenoiseBuffers b;
	if ((rc = denoise_buffers(ctx, pixels, &b))) return rc;
	const double s = ctx->rgb_mode ? 1.0 : 1000.0; // what ssx_finalize_kernel multiplies A / N by
	hipLaunchKernelGGL(ssx_denoise_var_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_accum.as<const double>(), ctx->d_noise.as<const double>(), b.var_in,
	                   pixel_grid(&p), (double)ctx->done_spp.load(), (double)ctx->sums.noise_batches, s * s);
	SSX_HIP(ctx, hipGetLastError());
	const SsxGuides g = guides_of(ctx, pixels);
	if ((rc = launch_atrous(ctx, dp, p.width, p.height, ctx->d_out.as<const float4>(), b.var_in, g.prim, g.albedo, b))) return rc;
	return denoise_read_back(ctx, dp, pixels, b, xyza_out, var_out);
}

} // extern "C"

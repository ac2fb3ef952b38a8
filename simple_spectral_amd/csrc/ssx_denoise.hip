// ssx_denoise.hip -- first-hit guide buffers and the variance-guided edge-stopping a-trous filter (include/ssx.h, "Denoising").  Part of ssx_api.hip's
// translation unit (included behind its context and launch helpers, like ssx_progressive.hip and ssx_spectral.hip).  Nothing here touches the generate,
// path or finalize kernels, and nothing here runs or is allocated unless one of the entry points at the end is called.
// The filter is stated once: ssx_atrous_den (the 3x3 Gaussian of the variance), ssx_atrous_tap_weight (a tap's w), ssx_atrous_weights (a pixel's 25 weights,
// masks and sw) and ssx_atrous_apply (the 25 taps of one group of channels).  ssx_atrous_kernel (image and variance) loops over the first two; the two shapes
// of the extra channels' kernel, plain gather and LDS-staged, take their weights from the third; the gather sums through the fourth, the LDS kernel keeps that loop in its own text.

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

// What one level of the filter reads, the same for its three kernels: the previous level's c and var and the guides.  launch_atrous fills it once per level.
struct SsxAtrousInput {
	const float4* c; const float* var; const uint32_t* prim; const float4* albedo;
	uint32_t width, height, step;   // step = 2^level; width * height <= 2^28 (denoise_check_size): a pixel's index fits 32 bits
	float sigma_l, inv_sa2;         // inv_sa2 = 1.0f / (sigma_a * sigma_a), by the host (the same float division)
};
struct SsxAtrousArgs { SsxAtrousInput in; float4* c_out; float* var_out; };
// (e, e_out: [groups][height][width], see "extra channels" below)
struct SsxAtrousChannelsArgs { SsxAtrousInput in; const float4* e; float4* e_out; uint32_t groups; };

__device__ __forceinline__ bool ssx_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool ssx_denoise_valid(const float4 c, float var) { return ssx_finite(c.x) && ssx_finite(c.y) && ssx_finite(c.z) && ssx_finite(var); }

// den = sigma_l * sqrt(g) + 1e-6f of the valid pixel (x, y) (include/ssx.h FILTER), g the 3x3 Gaussian of the variance over the valid neighbours at distance 1
// (not `step`), centre included: rows outer, columns inner.
__device__ __forceinline__ float ssx_atrous_den(const SsxAtrousInput& in, int x, int y) {
	const int W = (int)in.width, H = (int)in.height;
	float gs = 0.0f, ks = 0.0f;
#pragma unroll
	for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
		for (int dx = -1; dx <= 1; ++dx) {
			const int qx = x + dx, qy = y + dy;
			if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
			const uint32_t q = (uint32_t)qy * in.width + (uint32_t)qx;
			const float vq = in.var[q];
			if (!ssx_denoise_valid(in.c[q], vq)) continue;
			const float k3 = (dy == 0 ? 2.0f : 1.0f) * (dx == 0 ? 2.0f : 1.0f);
			gs += k3 * vq; ks += k3;
		}
	}
	return in.sigma_l * __builtin_sqrtf(gs / ks) + 1e-6f;
}

// The 5-tap B3 spline h = (1/16, 1/4, 3/8, 1/4, 1/16) at offset d in -2 .. 2; a tap's k = ssx_atrous_h(dy) * ssx_atrous_h(dx).
__device__ __forceinline__ float ssx_atrous_h(int d) { return d == 0 ? 0.375f : ((d == -1 || d == 1) ? 0.25f : 0.0625f); }

// w = (k * wl) * wa of one tap (include/ssx.h FILTER): the one statement of the weight, for the image and for the extra channels.
__device__ __forceinline__ float ssx_atrous_tap_weight(float k, float y_q, float y_p, float den, const float4 al_q, const float4 al_p, float inv_sa2) {
	const float xl = __builtin_fabsf(y_q - y_p) / den;
	const float wl = 1.0f / (1.0f + xl * xl);
	const float d0 = al_q.x - al_p.x, d1 = al_q.y - al_p.y, d2 = al_q.z - al_p.z, d3 = al_q.w - al_p.w;
	const float da2 = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
	const float wa = 1.0f / (1.0f + da2 * inv_sa2);
	return (k * wl) * wa;
}

// A 16x16-pixel workgroup (4 waves), one lane per pixel, plain gather: a tap reads c and albedo as one 16-byte load each, prim and var as 4 bytes (40 bytes
// per tap, 25 taps and the 9 variance taps of g per pixel).  Neighbouring lanes read neighbouring pixels at every step, so a wave's tap is four 256-byte runs
// (c, albedo) and four 64-byte ones; the working set of a level -- 40 bytes per pixel, 10 MB at 512^2 -- stays in the L2 / MALL from one level to the next.
// No atomics, no barriers, no LDS.  Every operation is binary32 in the order include/ssx.h writes it, divisions and the square root IEEE, nothing contracted:
// tests/denoise_ref.py restates it in numpy and the results are compared bit for bit.  The rows stay a rolled loop that skips a row outside the image as a
// whole, and the sums are five scalars: that is what keeps the kernel at its registers (profiles/r15/NOTES.md).
extern "C" __global__ void __launch_bounds__(256) ssx_atrous_kernel(SsxAtrousArgs a) {
	const SsxAtrousInput& in = a.in;
	const int W = (int)in.width, H = (int)in.height;
	const int x = (int)(blockIdx.x * 16u + threadIdx.x), y = (int)(blockIdx.y * 16u + threadIdx.y);
	if (x >= W || y >= H) return;
	const size_t p = (size_t)y * in.width + (size_t)x;
	const float4 cp = in.c[p];
	const float vp = in.var[p];
	if (!ssx_denoise_valid(cp, vp)) { a.c_out[p] = cp; a.var_out[p] = vp; return; } // an invalid pixel keeps what it has, at every level
	const float den = ssx_atrous_den(in, x, y);
	const uint32_t prim_p = in.prim[p];
	const float4 al_p = in.albedo[p];
	const int step = (int)in.step;
	float sw = 0.0f, scx = 0.0f, scy = 0.0f, scz = 0.0f, sv = 0.0f;
	for (int dy = -2; dy <= 2; ++dy) {
		const int qy = y + step * dy;
		if (qy < 0 || qy >= H) continue;
		const float hy = ssx_atrous_h(dy);
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const int qx = x + step * dx;
			if (qx < 0 || qx >= W) continue;
			const size_t q = (size_t)qy * in.width + (size_t)qx;
			if (in.prim[q] != prim_p) continue;
			const float4 cq = in.c[q];
			const float vq = in.var[q];
			if (!ssx_denoise_valid(cq, vq)) continue;
			const float w = ssx_atrous_tap_weight(hy * ssx_atrous_h(dx), cq.y, cp.y, den, in.albedo[q], al_p, in.inv_sa2);
			sw += w;
			scx += w * cq.x; scy += w * cq.y; scz += w * cq.z;
			sv += (w * w) * vq;
		}
	}
	a.c_out[p] = make_float4(scx / sw, scy / sw, scz / sw, cp.w); // (the centre tap always counts: sw >= 9/64)
	a.var_out[p] = sv / (sw * sw);
}

// ---- extra channels (include/ssx.h "EXTRA CHANNELS", "SPECTRAL CHANNELS") ---------------------------------------------------------------------------------
// The E extra channels of a pixel lie on the device planar in groups of four: e[group][pixel] as float4, groups = ceil(E / 4), the spare components of the
// last group +0 (they are filtered like the rest and never leave the device).  A tap is then one 16-byte load per group, neighbouring lanes reading
// neighbouring pixels: the access pattern of c in ssx_atrous_kernel, `groups` times.  groups * width * height <= 2^27 (channels_check_size): 32-bit indices.
__device__ __forceinline__ float ssx_channel(const float4* e, uint32_t plane, uint32_t p, uint32_t ch) {
	return reinterpret_cast<const float*>(e + (size_t)(ch >> 2) * plane + p)[ch & 3u];
}

// The level's 25 weights of the valid pixel (x, y) with image cp, for the extra channels: the expressions of ssx_atrous_kernel in its order (ssx_atrous_den,
// ssx_atrous_tap_weight), tap t = (dy + 2) * 5 + (dx + 2).  Returns sw; w[t] is +0 for a tap that does not take part; two 25-bit masks: `inside` (the tap is
// in the image: its address may be read) and `counted` (it takes part: inside, valid, same primitive).  Both loops are unrolled, so every index into w is
// static and w stays in registers.
__device__ __forceinline__ float ssx_atrous_weights(const SsxAtrousInput& in, int x, int y, const float4 cp, float (&w)[25], uint32_t& inside, uint32_t& counted) {
	const int W = (int)in.width, H = (int)in.height, step = (int)in.step;
	const float den = ssx_atrous_den(in, x, y);
	const uint32_t p = (uint32_t)y * in.width + (uint32_t)x;
	const uint32_t prim_p = in.prim[p];
	const float4 al_p = in.albedo[p];
	float sw = 0.0f;
	inside = 0u; counted = 0u;
#pragma unroll
	for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const int t = (dy + 2) * 5 + (dx + 2);
			w[t] = 0.0f;
			const int qx = x + step * dx, qy = y + step * dy;
			if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
			inside |= 1u << t;
			const uint32_t q = (uint32_t)qy * in.width + (uint32_t)qx;
			if (in.prim[q] != prim_p) continue;
			const float4 cq = in.c[q];
			if (!ssx_denoise_valid(cq, in.var[q])) continue;
			w[t] = ssx_atrous_tap_weight(ssx_atrous_h(dy) * ssx_atrous_h(dx), cq.y, cp.y, den, in.albedo[q], al_p, in.inv_sa2);
			counted |= 1u << t;
			sw += w[t];
		}
	}
	return sw;
}

// One group of four channels of one pixel: the 25 taps fetch(t) in the order of t, a select per component that adds w[t] * tap for a counted tap and leaves
// the sum alone for any other -- skipped, not added with weight 0 --, and the four divisions by sw.  Unrolled: t is static in w[t] and in fetch(t).
template <class Fetch>
__device__ __forceinline__ float4 ssx_atrous_apply(const float (&w)[25], uint32_t counted, float sw, Fetch fetch) {
	float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
	for (int t = 0; t < 25; ++t) {
		const float4 v = fetch(t);
		const bool on = ((counted >> t) & 1u) != 0u;
		s0 = on ? s0 + w[t] * v.x : s0; s1 = on ? s1 + w[t] * v.y : s1; s2 = on ? s2 + w[t] * v.z : s2; s3 = on ? s3 + w[t] * v.w : s3;
	}
	return make_float4(s0 / sw, s1 / sw, s2 / sw, s3 / sw);
}

// One level for the extra channels, launched next to ssx_atrous_kernel on the same input: the same 16x16-pixel workgroup, one lane per pixel.  The lane
// computes the level's weights once (ssx_atrous_weights: 25 registers and the two masks), then walks the groups (ssx_atrous_apply): 25 loads of 16 bytes, from
// the tap where it is inside the image and from the lane's own pixel where it is not.  The offsets (dy * width + dx) * step are the same for every lane
// (scalar registers).  No atomics, no LDS, no barriers; a lane writes its own pixel only.
extern "C" __global__ void __launch_bounds__(256) ssx_atrous_channels_kernel(SsxAtrousChannelsArgs a) {
	const SsxAtrousInput& in = a.in;
	const int W = (int)in.width, H = (int)in.height;
	const int x = (int)(blockIdx.x * 16u + threadIdx.x), y = (int)(blockIdx.y * 16u + threadIdx.y);
	if (x >= W || y >= H) return;
	const uint32_t plane = in.width * in.height, p = (uint32_t)y * in.width + (uint32_t)x;
	const float4 cp = in.c[p];
	const float vp = in.var[p];
	if (!ssx_denoise_valid(cp, vp)) { // an invalid pixel keeps what it has, at every level
		for (uint32_t g = 0; g < a.groups; ++g) a.e_out[(size_t)g * plane + p] = a.e[(size_t)g * plane + p];
		return;
	}
	const int step = (int)in.step;
	float w[25];
	uint32_t inside, counted;
	const float sw = ssx_atrous_weights(in, x, y, cp, w, inside, counted); // (the centre tap always counts: sw >= 9/64)
	for (uint32_t g = 0; g < a.groups; ++g) {
		const float4* const eg = a.e + (size_t)g * plane + p;
		a.e_out[(size_t)g * plane + p] = ssx_atrous_apply(w, counted, sw, [&](int t) {
			const ptrdiff_t off = (ptrdiff_t)((t / 5 - 2) * W + (t % 5 - 2)) * step; // inside the planes wherever `inside` says so
			return eg[(inside >> t) & 1u ? off : (ptrdiff_t)0];
		});
	}
}

// The same level with the taps staged in LDS, for the steps at which a workgroup's taps overlap: at step s the 25 taps of its 16x16 pixels lie in a tile of
// T x T pixels, T = 16 + 4 s (20 at step 1, 24 at step 2), so a value that the plain gather fetches up to 25 times is fetched T^2 / 256 = 1.6 or 2.3 times.
// Per group of four channels the 256 lanes copy the tile (zeros outside the image) into one of two LDS buffers of 576 float4, one barrier, and every lane
// takes its 25 taps from there at the static offsets (dy T + dx) s from its own place; the next group goes to the other buffer, so one barrier per group is
// enough (a lane that writes buffer b for group g + 2 has passed the barrier of group g + 1, which every lane reaches after its reads of group g).  All 256
// lanes stay to the end for the barriers: lanes outside the image and invalid pixels compute no weights; the former store nothing, the latter store the
// centre of the tile, i.e. what they had.  Weights are those of ssx_atrous_channels_kernel by the same function, the sums by the same loop: the same bits.
// Only for step <= 2 (launch_atrous).
constexpr uint32_t kChannelsLdsTileMax = 24u * 24u;
extern "C" __global__ void __launch_bounds__(256) ssx_atrous_channels_lds_kernel(SsxAtrousChannelsArgs a) {
	__shared__ float4 tile[2][kChannelsLdsTileMax];
	const SsxAtrousInput& in = a.in;
	const int W = (int)in.width, H = (int)in.height, step = (int)in.step, T = 16 + 4 * step;
	const int x = (int)(blockIdx.x * 16u + threadIdx.x), y = (int)(blockIdx.y * 16u + threadIdx.y);
	const bool in_image = x < W && y < H;
	const uint32_t plane = in.width * in.height, p = in_image ? (uint32_t)y * in.width + (uint32_t)x : 0u;
	float4 cp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	float vp = 0.0f;
	if (in_image) { cp = in.c[p]; vp = in.var[p]; }
	const bool valid = in_image && ssx_denoise_valid(cp, vp);
	float w[25];
#pragma unroll
	for (int t = 0; t < 25; ++t) w[t] = 0.0f;
	uint32_t inside = 0u, counted = 0u; // (`inside` is not used here: every tap is in the tile)
	float sw = 1.0f; // (a lane without weights divides nothing it stores)
	if (valid) sw = ssx_atrous_weights(in, x, y, cp, w, inside, counted);
	const int tid = (int)(threadIdx.y * 16u + threadIdx.x), cells = T * T;
	const int ox = (int)(blockIdx.x * 16u) - 2 * step, oy = (int)(blockIdx.y * 16u) - 2 * step;       // the tile's corner in the image
	const int mine = ((int)threadIdx.y + 2 * step) * T + ((int)threadIdx.x + 2 * step);            // the lane's own pixel in the tile: taps at mine + (dy T + dx) step, in 0 .. T^2 - 1
	int src[3]; // the up to three cells tid + 256 k the lane copies per group: its pixel in the plane, -1 outside the image (zeros), -2 past the tile (nothing)
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const int cell = tid + 256 * k, gx = ox + cell % T, gy = oy + cell / T;
		src[k] = cell >= cells ? -2 : ((gx >= 0 && gx < W && gy >= 0 && gy < H) ? gy * W + gx : -1);
	}
	for (uint32_t g = 0; g < a.groups; ++g) {
		const float4* const eg = a.e + (size_t)g * plane;
		float4* const buf = tile[g & 1u];
#pragma unroll
		for (int k = 0; k < 3; ++k)
			if (src[k] != -2) buf[tid + 256 * k] = src[k] >= 0 ? eg[src[k]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		__syncthreads();
		// The loop of ssx_atrous_apply with buf[mine + ...] as its fetch(t), spelled out: called through the function, with the tap as a lambda (captures by
		// reference or by value), this kernel lost 2 % at 64 bins and two levels, measured; with a functor it needed 124 VGPRs (profiles/r15/NOTES.md).
		float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
		for (int t = 0; t < 25; ++t) {
			const float4 v = buf[mine + ((t / 5 - 2) * T + (t % 5 - 2)) * step];
			const bool on = ((counted >> t) & 1u) != 0u;
			s0 = on ? s0 + w[t] * v.x : s0; s1 = on ? s1 + w[t] * v.y : s1; s2 = on ? s2 + w[t] * v.z : s2; s3 = on ? s3 + w[t] * v.w : s3;
		}
		if (in_image) a.e_out[(size_t)g * plane + p] = valid ? make_float4(s0 / sw, s1 / sw, s2 / sw, s3 / sw) : buf[mine];
	}
}

// Which levels take their taps from LDS: the one place that decides.  0: none (every level is the plain gather); at most 2 (the tile buffers hold step <= 2).
#ifndef SSX_CHANNELS_LDS_LEVELS
#define SSX_CHANNELS_LDS_LEVELS 2
#endif
static_assert(SSX_CHANNELS_LDS_LEVELS >= 0 && SSX_CHANNELS_LDS_LEVELS <= 2, "the LDS tile of ssx_atrous_channels_lds_kernel holds steps 1 and 2 only");
constexpr bool ssx_channels_level_in_lds(uint32_t level) { return level < (uint32_t)SSX_CHANNELS_LDS_LEVELS; }

// The C ABI's interleaved [height][width][E] <-> the groups of four; one lane per float4 on the way in, per float on the way out.
extern "C" __global__ void __launch_bounds__(256) ssx_channels_pack_kernel(const float* in, float4* e, uint32_t pixels, uint32_t E, uint32_t groups) {
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= pixels * groups) return;
	const uint32_t ch = 4u * (idx / pixels), p = idx % pixels;
	const float* const src = in + (size_t)p * E;
	e[idx] = make_float4(src[ch], ch + 1u < E ? src[ch + 1u] : 0.0f, ch + 2u < E ? src[ch + 2u] : 0.0f, ch + 3u < E ? src[ch + 3u] : 0.0f);
}
extern "C" __global__ void __launch_bounds__(256) ssx_channels_unpack_kernel(const float4* e, float* out, uint32_t pixels, uint32_t E) {
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= pixels * E) return;
	out[idx] = ssx_channel(e, pixels, idx / E, idx % E);
}

// e0 of the spectral bins (include/ssx.h "SPECTRAL CHANNELS") from the persistent S[tile slot][bin][pixel of the tile] and N[tile slot][m][pixel of the tile]
// of a context that owns the whole image: channels 0..B-1 = (float)(S / n), B..B+M-1 = (float)((double)N / n), both divisions binary64; one lane per float4.
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_channels_kernel(const double* S, const uint32_t* N, float4* e, SsxPixelGrid g, uint32_t M, double n) {
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x, pixels = g.width * g.height, B = 4u * M, groups = (B + M + 3u) / 4u;
	if (idx >= pixels * groups) return;
	const uint32_t ch0 = 4u * (idx / pixels), p = idx % pixels, i = p % g.width, j = p / g.width;
	const size_t slot = ssx_shared_tile(g, i, j) / g.tile_stride, lane = (j & 7u) * 8u + (i & 7u);
	float v[4];
#pragma unroll
	for (uint32_t k = 0; k < 4u; ++k) {
		const uint32_t ch = ch0 + k;
		v[k] = ch < B ? (float)(S[(slot * B + ch) * 64u + lane] / n) : (ch < B + M ? (float)((double)N[(slot * M + (ch - B)) * 64u + lane] / n) : 0.0f);
	}
	e[idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// out[p][b] = eL[p][B + b % M] > 0 ? eL[p][b] / eL[p][B + b % M] : 0.0f, row-major [height][width][B]; one lane per float
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_ratio_kernel(const float4* e, float* out, uint32_t pixels, uint32_t M) {
	const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x, B = 4u * M;
	if (idx >= pixels * B) return;
	const uint32_t p = idx / B, b = idx % B;
	const float den = ssx_channel(e, pixels, p, B + b % M);
	out[idx] = den > 0.0f ? ssx_channel(e, pixels, p, b) / den : 0.0f;
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
	hipLaunchKernelGGL(ssx_guides_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), staged_blob_lds(ctx->blob_words), ctx->stream, a, guides_of(ctx, pixels));
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
// ... with the caller's four filter inputs in c_in, albedo_in, var_in and prim_in (queued on the context's stream)
int denoise_upload_inputs(ssx_ctx* ctx, size_t pixels, const float* xyza, const float* var, const uint32_t* prim, const float* albedo, DenoiseBuffers* b) {
	if (const int rc = denoise_buffers(ctx, pixels, b)) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(b->c_in, xyza, pixels * 16u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(b->albedo_in, albedo, pixels * 16u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(b->var_in, var, pixels * 4u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(b->prim_in, prim, pixels * 4u, hipMemcpyHostToDevice, ctx->stream));
	return SSX_OK;
}

// d_denoise_channels: the extra channels' ping-pong buffers e[0] | e[1] (groups x pixels float4 each) and, behind them, the row-major staging of what the
// entry point takes or returns ([pixels][stage_channels] floats).  Allocated by the two entry points that filter extra channels, by nothing else.
struct ChannelBuffers { float4* e[2]; float* stage; uint32_t groups; };
constexpr uint32_t kDenoiseMaxChannels = 80;
constexpr uint64_t kChannelBufferLimit = 1ull << 31; // bytes of one ping-pong buffer: the kernels index them with 32 bits
int channels_check_size(ssx_ctx* ctx, size_t pixels, uint32_t channels, const char* what) {
	if ((uint64_t)pixels * ((channels + 3u) / 4u) * 16u > kChannelBufferLimit)
		return fail(ctx, SSX_ERR_ARG, fmt("%s: %u channels at this size need channel buffers of more than 2 GiB each", what, channels));
	return SSX_OK;
}
int channel_buffers(ssx_ctx* ctx, size_t pixels, uint32_t channels, uint32_t stage_channels, ChannelBuffers* cb) {
	cb->groups = (channels + 3u) / 4u;
	const size_t plane = pixels * cb->groups;
	SSX_HIP(ctx, ctx->d_denoise_channels.reserve(plane * 32u + pixels * stage_channels * sizeof(float)));
	cb->e[0] = ctx->d_denoise_channels.as<float4>(); cb->e[1] = cb->e[0] + plane;
	cb->stage = reinterpret_cast<float*>(cb->e[1] + plane);
	return SSX_OK;
}
dim3 blocks_of(size_t lanes) { return dim3((uint32_t)((lanes + 255u) / 256u)); }

// The levels, one launch each, ping-pong between b.c / b.var[0] and [1]; none of the four inputs is written.  The result is in b.c / b.var[(levels - 1) & 1]
// once the stream has been waited for.  With extra channels (cb; NULL: none, and nothing more is launched) every level also runs ssx_atrous_channels_kernel (or, where ssx_channels_level_in_lds says so, its LDS-staged twin) on
// the same input, from cb->e[l & 1] to cb->e[(l + 1) & 1]: the caller has put the channels into cb->e[0] and finds them in cb->e[levels & 1].
int launch_atrous(ssx_ctx* ctx, const ssx_denoise_params& dp, uint32_t width, uint32_t height, const float4* c, const float* var, const uint32_t* prim, const float4* albedo, const DenoiseBuffers& b,
                  const ChannelBuffers* cb = nullptr) {
	SsxAtrousInput in{};
	in.prim = prim; in.albedo = albedo;
	in.width = width; in.height = height;
	in.sigma_l = dp.sigma_l; in.inv_sa2 = 1.0f / (dp.sigma_a * dp.sigma_a);
	const dim3 grid((width + 15u) / 16u, (height + 15u) / 16u), block(16, 16);
	for (uint32_t l = 0; l < dp.levels; ++l) {
		in.c = l ? b.c[(l - 1u) & 1u] : c; in.var = l ? b.var[(l - 1u) & 1u] : var;
		in.step = 1u << l;
		hipLaunchKernelGGL(ssx_atrous_kernel, grid, block, 0, ctx->stream, SsxAtrousArgs{ in, b.c[l & 1u], b.var[l & 1u] });
		SSX_HIP(ctx, hipGetLastError());
		if (!cb) continue;
		const SsxAtrousChannelsArgs ca{ in, cb->e[l & 1u], cb->e[(l + 1u) & 1u], cb->groups };
		if (ssx_channels_level_in_lds(l)) hipLaunchKernelGGL(ssx_atrous_channels_lds_kernel, grid, block, 0, ctx->stream, ca);
		else hipLaunchKernelGGL(ssx_atrous_channels_kernel, grid, block, 0, ctx->stream, ca);
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

// What ssx_denoise and ssx_denoise_spectral ask of the context's own state before they touch the device (the reasons as ssx_last_error gives them); on
// return the context's device is current and idle, and the guide buffers of the render's size exist.
int denoise_own_state_ready(ssx_ctx* ctx, const char* what, bool spectral) {
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if (spectral && !ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, fmt("%s: spectral output is off (ssx_set_spectral_bins)", what));
	if (const int rc = sums_ready(ctx, what)) return rc;
	if (spectral && !ctx->sums.spectral_valid) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context holds no spectral bins: ", what) + ctx->spectral_note);
	if (!ctx->noise_on) return fail(ctx, SSX_ERR_STATE, fmt("%s: the noise estimate is off (ssx_set_noise_estimate): the filter is guided by its variance", what));
	if (!ctx->sums.noise_valid || ctx->sums.noise_batches < 2u)
		return fail(ctx, SSX_ERR_STATE, fmt("%s: %u batch(es) so far; the between-batch variance needs two", what, ctx->sums.noise_valid ? ctx->sums.noise_batches : 0u));
	const ssx_render_params& p = ctx->cur;
	if (p.tile_stride != 1u)
		return fail(ctx, SSX_ERR_STATE, fmt("%s: the context owns a part of the image only (tile_stride = %u): combine the ranks and use %s", what, p.tile_stride, spectral ? "ssx_denoise_channels" : "ssx_denoise_images"));
	if (!ctx->d_out.ptr) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context holds no image", what));
	return ensure_guides(ctx, p.width, p.height);
}

// ... and the filter's buffers with the variance in image units in b->var_in (queued on the context's stream)
int denoise_own_inputs(ssx_ctx* ctx, DenoiseBuffers* b) {
	const ssx_render_params& p = ctx->cur;
	if (const int rc = denoise_buffers(ctx, (size_t)p.width * p.height, b)) return rc;
	const double s = ctx->rgb_mode ? 1.0 : 1000.0; // what ssx_finalize_kernel multiplies A / N by
	hipLaunchKernelGGL(ssx_denoise_var_kernel, pixel_blocks(&p), dim3(256), 0, ctx->stream, ctx->d_accum.as<const double>(), ctx->d_noise.as<const double>(), b->var_in,
	                   pixel_grid(&p), (double)ctx->done_spp.load(), (double)ctx->sums.noise_batches, s * s);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

// The device part of ssx_denoise_spectral, shared with ssx_spectral_develop (ssx_develop.hip), after denoise_own_state_ready(.., true): the channels e0 of the
// bins, the L levels and the ratio, all queued on the context's stream.  On return (not yet waited for) the filtered image and variance are in b->c / b->var
// [(levels - 1) & 1] and out[p][b], row-major [height][width][B], in cb->stage.
int denoise_spectral_device(ssx_ctx* ctx, const ssx_denoise_params& dp, DenoiseBuffers* b, ChannelBuffers* cb) {
	const ssx_render_params& p = ctx->cur;
	const size_t pixels = (size_t)p.width * p.height;
	const uint32_t B = ctx->spectral_bins, M = B / 4u;
	int rc = channels_check_size(ctx, pixels, B + M, "ssx_denoise_spectral");
	if (rc) return rc;
	if ((rc = denoise_own_inputs(ctx, b))) return rc;
	if ((rc = channel_buffers(ctx, pixels, B + M, B, cb))) return rc;
	hipLaunchKernelGGL(ssx_spectral_channels_kernel, blocks_of(pixels * cb->groups), dim3(256), 0, ctx->stream, ctx->d_spectral_sums.as<const double>(),
	                   ctx->d_spectral_counts.as<const uint32_t>(), cb->e[0], pixel_grid(&p), M, (double)ctx->done_spp.load());
	SSX_HIP(ctx, hipGetLastError());
	const SsxGuides g = guides_of(ctx, pixels);
	if ((rc = launch_atrous(ctx, dp, p.width, p.height, ctx->d_out.as<const float4>(), b->var_in, g.prim, g.albedo, *b, cb))) return rc;
	hipLaunchKernelGGL(ssx_spectral_ratio_kernel, blocks_of(pixels * B), dim3(256), 0, ctx->stream, cb->e[dp.levels & 1u], cb->stage, (uint32_t)pixels, M);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_guides(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t* prim, float* depth, float* normal, float* albedo) {
	if (!ctx) return SSX_ERR_ARG;
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	int rc = idle_on_device(ctx); // (before the size check, so that a running render is refused first, as it was; a bad size is now refused with the device current)
	if (rc) return rc;
	if ((rc = denoise_check_size(ctx, width, height, "ssx_guides"))) return rc;
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
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	DenoiseBuffers b;
	if ((rc = denoise_upload_inputs(ctx, pixels, xyza, var, prim, albedo, &b))) return rc;
	if ((rc = launch_atrous(ctx, dp, width, height, b.c_in, b.var_in, b.prim_in, b.albedo_in, b))) return rc;
	return denoise_read_back(ctx, dp, pixels, b, xyza_out, var_out);
}

int ssx_denoise(ssx_ctx* ctx, const ssx_denoise_params* params, float* xyza_out, float* var_out) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_denoise_params dp;
	int rc = denoise_take_params(ctx, params, &dp);
	if (rc) return rc;
	if ((rc = denoise_own_state_ready(ctx, "ssx_denoise", false))) return rc;
	const ssx_render_params& p = ctx->cur;
	const size_t pixels = (size_t)p.width * p.height;
	DenoiseBuffers b;
	if ((rc = denoise_own_inputs(ctx, &b))) return rc;
	const SsxGuides g = guides_of(ctx, pixels);
	if ((rc = launch_atrous(ctx, dp, p.width, p.height, ctx->d_out.as<const float4>(), b.var_in, g.prim, g.albedo, b))) return rc;
	return denoise_read_back(ctx, dp, pixels, b, xyza_out, var_out);
}

int ssx_denoise_channels(ssx_ctx* ctx, const ssx_denoise_params* params, uint32_t width, uint32_t height, const float* xyza, const float* var,
                         const uint32_t* prim, const float* albedo, uint32_t channels, const float* extra, float* xyza_out, float* var_out, float* extra_out) {
	if (!ctx) return SSX_ERR_ARG;
	if (channels < 1u || channels > kDenoiseMaxChannels) return fail(ctx, SSX_ERR_ARG, fmt("ssx_denoise_channels: channels = %u: need 1..%u", channels, kDenoiseMaxChannels));
	if (!xyza || !var || !prim || !albedo || !extra || !extra_out)
		return fail(ctx, SSX_ERR_ARG, "ssx_denoise_channels: xyza, var, prim, albedo, extra and extra_out must not be NULL");
	ssx_denoise_params dp;
	int rc = denoise_take_params(ctx, params, &dp);
	if (rc) return rc;
	if ((rc = denoise_check_size(ctx, width, height, "ssx_denoise_channels"))) return rc;
	const size_t pixels = (size_t)width * height;
	if ((rc = channels_check_size(ctx, pixels, channels, "ssx_denoise_channels"))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	DenoiseBuffers b;
	ChannelBuffers cb;
	if ((rc = denoise_upload_inputs(ctx, pixels, xyza, var, prim, albedo, &b))) return rc;
	if ((rc = channel_buffers(ctx, pixels, channels, channels, &cb))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(cb.stage, extra, pixels * channels * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(ssx_channels_pack_kernel, blocks_of(pixels * cb.groups), dim3(256), 0, ctx->stream, cb.stage, cb.e[0], (uint32_t)pixels, channels, cb.groups);
	SSX_HIP(ctx, hipGetLastError());
	if ((rc = launch_atrous(ctx, dp, width, height, b.c_in, b.var_in, b.prim_in, b.albedo_in, b, &cb))) return rc;
	hipLaunchKernelGGL(ssx_channels_unpack_kernel, blocks_of(pixels * channels), dim3(256), 0, ctx->stream, cb.e[dp.levels & 1u], cb.stage, (uint32_t)pixels, channels);
	SSX_HIP(ctx, hipGetLastError());
	if ((rc = denoise_read_back(ctx, dp, pixels, b, xyza_out, var_out))) return rc; // (waits for the stream)
	SSX_HIP(ctx, hipMemcpy(extra_out, cb.stage, pixels * channels * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_denoise_spectral(ssx_ctx* ctx, const ssx_denoise_params* params, float* mean_out, float* xyza_out, float* var_out) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_denoise_params dp;
	int rc = denoise_take_params(ctx, params, &dp);
	if (rc) return rc;
	if ((rc = denoise_own_state_ready(ctx, "ssx_denoise_spectral", true))) return rc;
	const ssx_render_params& p = ctx->cur;
	const size_t pixels = (size_t)p.width * p.height;
	DenoiseBuffers b;
	ChannelBuffers cb;
	if ((rc = denoise_spectral_device(ctx, dp, &b, &cb))) return rc;
	if ((rc = denoise_read_back(ctx, dp, pixels, b, xyza_out, var_out))) return rc; // (waits for the stream)
	if (mean_out) SSX_HIP(ctx, hipMemcpy(mean_out, cb.stage, pixels * ctx->spectral_bins * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

} // extern "C"

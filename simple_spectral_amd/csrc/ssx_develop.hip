// ssx_develop.hip -- developing the spectral bins (include/ssx.h, "Developing the spectral bins"): out[p][c] = sum_b q[p][b] * W[c][b], one linear map per
// pixel from B bins to C channels.  Part of ssx_api.hip's translation unit (included behind ssx_spectral.hip and ssx_denoise.hip, whose state and helpers it
// uses).  Two kernels, both memory bound: they read every q once and write C floats per pixel; no atomics, no barriers, a lane writes only its own pixel.
//
// The weights: every lane of a wave needs W[.][b] at the same time, so they are read at wave-uniform addresses from a small device buffer -- the compiler
// turns those into scalar loads served by the scalar cache -- rather than staged in LDS, which would cost a barrier and buy nothing: no lane indexes the table
// by anything of its own.  The buffer is bin-major, W_dev[b][4 G], G = ceil(C / 4) groups of four channels, the padding channels zero (at most 64 x 16 floats =
// 4 KB): one bin's weights are 16 G consecutive bytes.  G is a template parameter, so the 4 G accumulators are registers with static indices; the padding
// accumulators are computed and never stored.

struct SsxDevelopArgs {
	const double* S;          // state kernel: S[tile slot][bin][pixel of the tile] (ssx_spectral.hip)
	const float* q;           // images kernel: row-major [pixels][B]
	const float* W;           // [B][4 G]
	float* out;               // row-major [pixels][C]
	SsxPixelGrid g;           // state kernel: the device's tile list, slot -> tile by tile_of_slot
	uint32_t B, C, pixels;
	double M, n;              // state kernel: q = (float)((S * M) / n), both binary64
};

// acc[k] = acc[k] + (q * w[k]): the product rounded before the add (the build's -ffp-contract=off), bins in ascending order at the caller
template <int G>
__device__ __forceinline__ void develop_bin(float (&acc)[4 * G], float q, const float* __restrict__ w) {
#pragma unroll
	for (int k = 0; k < 4 * G; ++k) acc[k] = acc[k] + q * w[k];
}
template <int G>
__device__ __forceinline__ void develop_store(const float (&acc)[4 * G], float* __restrict__ o, uint32_t C) {
#pragma unroll
	for (int k = 0; k < 4 * G; ++k) if ((uint32_t)k < C) o[k] = acc[k];
}

// One 64-lane workgroup (one wave) per owned tile slot; lane = pixel of the tile, so that per bin the wave reads 512 consecutive bytes of S.  Lanes outside a
// ragged image touch nothing.  Pixels the context does not own are not visited: the entry point has zeroed the output.
template <int G>
__device__ __forceinline__ void develop_state_body(const SsxDevelopArgs& a) {
	const uint32_t px = threadIdx.x, slot = blockIdx.x;
	uint32_t tx, ty;
	(void)tile_of_slot(a.g, slot, tx, ty);
	const uint32_t i = tx * 8u + (px & 7u), j = ty * 8u + (px >> 3);
	if (i >= a.g.width || j >= a.g.height) return;
	const double* const S = a.S + (size_t)slot * a.B * 64u + px;
	float acc[4 * G];
#pragma unroll
	for (int k = 0; k < 4 * G; ++k) acc[k] = 0.0f;
#pragma unroll 4
	for (uint32_t b = 0; b < a.B; ++b) develop_bin<G>(acc, (float)((S[(size_t)b * 64u] * a.M) / a.n), a.W + (size_t)b * (4 * G));
	develop_store<G>(acc, a.out + ((size_t)j * a.g.width + i) * a.C, a.C);
}

// One lane per pixel; a lane reads its B consecutive floats in float4s (B is a multiple of 4, the array 16-byte aligned).
template <int G>
__device__ __forceinline__ void develop_images_body(const SsxDevelopArgs& a) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= a.pixels) return;
	const float4* const q = reinterpret_cast<const float4*>(a.q + (size_t)p * a.B);
	float acc[4 * G];
#pragma unroll
	for (int k = 0; k < 4 * G; ++k) acc[k] = 0.0f;
#pragma unroll 2
	for (uint32_t b4 = 0; b4 < a.B / 4u; ++b4) {
		const float4 v = q[b4];
		const float* const w = a.W + (size_t)b4 * (16 * G);
		develop_bin<G>(acc, v.x, w); develop_bin<G>(acc, v.y, w + 4 * G); develop_bin<G>(acc, v.z, w + 8 * G); develop_bin<G>(acc, v.w, w + 12 * G);
	}
	develop_store<G>(acc, a.out + (size_t)p * a.C, a.C);
}

extern "C" {
__global__ void __launch_bounds__(64) ssx_develop_state_kernel_g1(SsxDevelopArgs a) { develop_state_body<1>(a); }
__global__ void __launch_bounds__(64) ssx_develop_state_kernel_g2(SsxDevelopArgs a) { develop_state_body<2>(a); }
__global__ void __launch_bounds__(64) ssx_develop_state_kernel_g3(SsxDevelopArgs a) { develop_state_body<3>(a); }
__global__ void __launch_bounds__(64) ssx_develop_state_kernel_g4(SsxDevelopArgs a) { develop_state_body<4>(a); }
__global__ void __launch_bounds__(256) ssx_develop_images_kernel_g1(SsxDevelopArgs a) { develop_images_body<1>(a); }
__global__ void __launch_bounds__(256) ssx_develop_images_kernel_g2(SsxDevelopArgs a) { develop_images_body<2>(a); }
__global__ void __launch_bounds__(256) ssx_develop_images_kernel_g3(SsxDevelopArgs a) { develop_images_body<3>(a); }
__global__ void __launch_bounds__(256) ssx_develop_images_kernel_g4(SsxDevelopArgs a) { develop_images_body<4>(a); }
}

namespace {

constexpr uint32_t kDevelopMaxChannels = 16;
constexpr size_t kDevelopWeightBytes = 64u * kDevelopMaxChannels * sizeof(float); // 4 KB: the largest W_dev

int develop_check(ssx_ctx* ctx, const char* what, uint32_t channels, const float* weights) {
	if (channels < 1u || channels > kDevelopMaxChannels) return fail(ctx, SSX_ERR_ARG, fmt("%s: channels = %u: need 1..%u", what, channels, kDevelopMaxChannels));
	if (!weights) return fail(ctx, SSX_ERR_ARG, fmt("%s: weights must not be NULL", what));
	return SSX_OK;
}

// d_develop: W_dev (4 KB) | out [pixels][C] | q [pixels][B] (ssx_develop_images only; q_floats = 0 otherwise), the arrays at multiples of 16 bytes.  The caller's
// [C][B] weights go up as W_dev[b][4 G] with zero padding, on the context's stream.
struct DevelopBuffers { float* W; float* out; float* q; };
int develop_buffers(ssx_ctx* ctx, size_t pixels, uint32_t B, uint32_t C, const float* weights, size_t q_floats, DevelopBuffers* d) {
	const size_t out_bytes = (pixels * C * sizeof(float) + 15u) & ~(size_t)15u;
	SSX_HIP(ctx, ctx->d_develop.reserve(kDevelopWeightBytes + out_bytes + q_floats * sizeof(float)));
	uint8_t* const base = ctx->d_develop.as<uint8_t>();
	d->W = reinterpret_cast<float*>(base);
	d->out = reinterpret_cast<float*>(base + kDevelopWeightBytes);
	d->q = reinterpret_cast<float*>(base + kDevelopWeightBytes + out_bytes);
	const uint32_t G4 = 4u * ((C + 3u) / 4u);
	std::vector<float> w((size_t)B * G4, 0.0f);
	for (uint32_t c = 0; c < C; ++c) for (uint32_t b = 0; b < B; ++b) w[(size_t)b * G4 + c] = weights[(size_t)c * B + b];
	SSX_HIP(ctx, hipMemcpy(d->W, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice)); // (blocking: `w` goes out of scope)
	return SSX_OK;
}

int launch_develop_images(ssx_ctx* ctx, const SsxDevelopArgs& a) {
	const dim3 grid = blocks_of(a.pixels), block(256);
	switch ((a.C + 3u) / 4u) {
	case 1: hipLaunchKernelGGL(ssx_develop_images_kernel_g1, grid, block, 0, ctx->stream, a); break;
	case 2: hipLaunchKernelGGL(ssx_develop_images_kernel_g2, grid, block, 0, ctx->stream, a); break;
	case 3: hipLaunchKernelGGL(ssx_develop_images_kernel_g3, grid, block, 0, ctx->stream, a); break;
	default: hipLaunchKernelGGL(ssx_develop_images_kernel_g4, grid, block, 0, ctx->stream, a); break;
	}
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

int launch_develop_state(ssx_ctx* ctx, const SsxDevelopArgs& a, uint32_t my_tiles) {
	if (my_tiles == 0) return SSX_OK;
	const dim3 grid(my_tiles), block(64);
	switch ((a.C + 3u) / 4u) {
	case 1: hipLaunchKernelGGL(ssx_develop_state_kernel_g1, grid, block, 0, ctx->stream, a); break;
	case 2: hipLaunchKernelGGL(ssx_develop_state_kernel_g2, grid, block, 0, ctx->stream, a); break;
	case 3: hipLaunchKernelGGL(ssx_develop_state_kernel_g3, grid, block, 0, ctx->stream, a); break;
	default: hipLaunchKernelGGL(ssx_develop_state_kernel_g4, grid, block, 0, ctx->stream, a); break;
	}
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

int develop_read_back(ssx_ctx* ctx, const DevelopBuffers& d, size_t pixels, uint32_t C, float* out) {
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (out) SSX_HIP(ctx, hipMemcpy(out, d.out, pixels * C * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

// What a develop from the context's own state asks first (ssx_spectral_develop, ssx_spectral_delta_e): the refusals, then the device is the context's.
int develop_state_ready(ssx_ctx* ctx, const char* what, bool denoised) {
	if (!ctx->spectral_bins) return fail(ctx, SSX_ERR_STATE, fmt("%s: spectral output is off (ssx_set_spectral_bins)", what));
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (!ctx->sums.continuable || !ctx->sums.spectral_valid)
		return fail(ctx, SSX_ERR_STATE, fmt("%s: the context holds no spectral bins: ", what) + (ctx->sums.continuable ? ctx->spectral_note : std::string("no render has accumulated any (ssx_render_start first)")));
	if (ctx->done_spp.load() == 0u) return fail(ctx, SSX_ERR_STATE, fmt("%s: no sample has been accumulated yet (ssx_done_spp is 0)", what));
	if (denoised) { if (const int rc = denoise_own_state_ready(ctx, what, true)) return rc; }
	else if (const int rc = sums_ready(ctx, what)) return rc;
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_develop_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q, const float* weights, uint32_t channels, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	int rc = develop_check(ctx, "ssx_develop_images", channels, weights);
	if (rc) return rc;
	if (bins < 4u || bins > 64u || (bins & 3u)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_develop_images: %u bins: need a multiple of 4 up to 64", bins));
	if (!q || !out) return fail(ctx, SSX_ERR_ARG, "ssx_develop_images: q and out must not be NULL");
	if ((rc = denoise_check_size(ctx, width, height, "ssx_develop_images"))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	DevelopBuffers d;
	if ((rc = develop_buffers(ctx, pixels, bins, channels, weights, pixels * bins, &d))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d.q, q, pixels * bins * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	SsxDevelopArgs a{};
	a.q = d.q; a.W = d.W; a.out = d.out;
	a.B = bins; a.C = channels; a.pixels = (uint32_t)pixels;
	if ((rc = launch_develop_images(ctx, a))) return rc;
	return develop_read_back(ctx, d, pixels, channels, out);
}

int ssx_spectral_develop(ssx_ctx* ctx, const ssx_denoise_params* denoise, const float* weights, uint32_t channels, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_develop";
	int rc = develop_check(ctx, what, channels, weights);
	if (rc) return rc;
	ssx_denoise_params dp;
	if (denoise && (rc = denoise_take_params(ctx, denoise, &dp))) return rc;
	if ((rc = develop_state_ready(ctx, what, denoise != nullptr))) return rc;
	const uint32_t done = ctx->done_spp.load();
	const ssx_render_params& p = ctx->cur;
	const size_t pixels = (size_t)p.width * p.height;
	const uint32_t B = ctx->spectral_bins;
	DevelopBuffers d;
	if ((rc = develop_buffers(ctx, pixels, B, channels, weights, 0, &d))) return rc;
	SsxDevelopArgs a{};
	a.W = d.W; a.out = d.out;
	a.B = B; a.C = channels; a.pixels = (uint32_t)pixels;
	if (denoise) { // the filter as ssx_denoise_spectral runs it; its ratio, row-major in the channel buffers' staging area, is q
		DenoiseBuffers b;
		ChannelBuffers cb;
		if ((rc = denoise_spectral_device(ctx, dp, &b, &cb))) return rc;
		a.q = cb.stage;
		if ((rc = launch_develop_images(ctx, a))) return rc;
	} else {
		a.S = ctx->d_spectral_sums.as<const double>();
		a.g = pixel_grid(&p);
		a.M = (double)(B / 4u); a.n = (double)done;
		if (p.tile_stride != 1u) SSX_HIP(ctx, hipMemsetAsync(d.out, 0, pixels * channels * sizeof(float), ctx->stream)); // pixels of other contexts: +0
		if ((rc = launch_develop_state(ctx, a, owned_tiles(p)))) return rc;
	}
	return develop_read_back(ctx, d, pixels, channels, out);
}

} // extern "C"

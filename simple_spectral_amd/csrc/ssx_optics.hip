// ssx_optics.hip -- developing through a lens (include/ssx.h, "Developing through a lens"): per wavelength bin a bilinear resampling about the optical centre
// (WARP) and a separable blur (BLUR) on q [height][width][B], row-major.  Part of ssx_api.hip's translation unit, behind ssx_develop.hip (develop_state_ready,
// develop_buffers, launch_develop_images), ssx_spectral.hip (carve, valid_bins) and ssx_denoise.hip (blocks_of, denoise_check_size, denoise_spectral_device).
// Four kernels, all memory bound, no atomics, a lane writes only its own output.  Every product is rounded before its add (the build's -ffp-contract=off).
//
// The lanes of the warp and blur kernels run along the INTERLEAVED (pixel, bin) axis, element e = i * B + b of a row: a wave stores 256 consecutive bytes, and
// reads them wherever the source is aligned with the destination (every blur tap; the warp's four corners are four such runs per bin, shifted per bin).
//
// The per-bin tables -- s_b, r_b and the taps -- are indexed by the bin only, and with this lane order a wave holds up to 64 different bins: the addresses are
// not wave-uniform, so scalar loads (the develop kernels' way) are out.  The warp kernel reads s_b from the parameter block in global memory: lane -> b is
// consecutive modulo B, one 256-byte read per wave that stays in the vector L1.  The blur kernels copy r_b and the taps into LDS once per workgroup, next to the
// barrier the staging needs anyway, laid out [b][2 R + 1] as the caller gives them.  The blur walk is uniform in d across the wave (see the kernels), so at
// step d a group of 32 lanes reads words b * (2 R + 1) + d + R for consecutive b (modulo B) -- an ODD stride, so 32 distinct b with b mod 32 distinct land on 32
// distinct banks, and lanes with the same b read one address (a broadcast).  Only B in {36, ..., 60} can put two different b of one group on a bank, a two-way
// conflict on the tap read.

#define SSX_OPTICS_LANES 256u
#define SSX_OPTICS_MAX_TAPS (2u * SSX_OPTICS_MAX_RADIUS + 1u)

struct SsxOpticsArgs {
	const double* S;          // unpack kernel: S[tile slot][bin][pixel of the tile] (ssx_spectral.hip)
	const float* src;         // warp and blur kernels: row-major [height][width][B]
	float* dst;               // row-major [height][width][B]
	const float* scale;       // [B]
	const uint32_t* radius;   // [B]
	const float* taps;        // [B][2 R + 1]
	SsxPixelGrid g;           // unpack kernel: the device's tile list, slot -> tile by tile_of_slot
	uint32_t width, height, B, R, Rmax;   // Rmax: the largest r_b (<= R): how far the blur kernels' wave-uniform walk goes
	float cx, cy;
	double M, n;              // unpack kernel: q = (float)((S * M) / n), both binary64
};

// One 64-lane workgroup (one wave) per owned tile slot, lane = pixel of the tile as in develop_state_body: per bin the wave reads 512 consecutive bytes of S.  A
// lane gathers four bins and stores them as one float4 (B is a multiple of 4, the row-major array 16-byte aligned): over its B / 4 stores a lane fills its own
// 4 B consecutive bytes, so every cache line is written whole by one lane within four consecutive stores.  Lanes outside a ragged image touch nothing.
extern "C" __global__ void __launch_bounds__(64) ssx_optics_unpack_kernel(SsxOpticsArgs a) {
	const uint32_t px = threadIdx.x, slot = blockIdx.x;
	uint32_t tx, ty;
	(void)tile_of_slot(a.g, slot, tx, ty);
	const uint32_t i = tx * 8u + (px & 7u), j = ty * 8u + (px >> 3);
	if (i >= a.width || j >= a.height) return;
	const double* const S = a.S + (size_t)slot * a.B * 64u + px;
	float4* const o = reinterpret_cast<float4*>(a.dst + ((size_t)j * a.width + i) * a.B);
#pragma unroll 2
	for (uint32_t b4 = 0; b4 < a.B / 4u; ++b4) {
		const double* const s = S + (size_t)b4 * 256u;
		float4 v;
		v.x = (float)((s[0] * a.M) / a.n); v.y = (float)((s[64] * a.M) / a.n); v.z = (float)((s[128] * a.M) / a.n); v.w = (float)((s[192] * a.M) / a.n);
		o[b4] = v;
	}
}

// WARP's coordinate along one axis: the source position of destination index k, split into the two clamped neighbours and the weight of the second
__device__ __forceinline__ void optics_axis(uint32_t k, float c, float s, uint32_t extent, uint32_t& ka, uint32_t& kb, float& f) {
	const float d = ((float)k + 0.5f) - c;
	float x = (c + d * s) - 0.5f;
	x = x > -1.0f ? x : -1.0f;                                                           // max(x, -1.0f): a NaN gives -1
	const float top = (float)extent;
	x = x < top ? x : top;                                                               // min(x, (float)extent)
	const float x0 = floorf(x);
	f = x - x0;
	const int k0 = (int)x0, last = (int)extent - 1;                                      // -1 .. extent
	ka = (uint32_t)min(max(k0, 0), last);
	kb = (uint32_t)min(max(k0 + 1, 0), last);
}

// One lane per element of the image, e = (j * width + i) * B + b.
extern "C" __global__ void __launch_bounds__(SSX_OPTICS_LANES) ssx_optics_warp_kernel(SsxOpticsArgs a) {
	const size_t e = (size_t)blockIdx.x * SSX_OPTICS_LANES + threadIdx.x;
	const size_t pixels = (size_t)a.width * a.height;
	if (e >= pixels * a.B) return;
	const uint32_t p = pixels * a.B <= 0xFFFFFFFFull ? (uint32_t)e / a.B : (uint32_t)(e / a.B);   // (uniform) 32-bit division wherever the image allows it
	const uint32_t b = (uint32_t)(e - (size_t)p * a.B);
	const uint32_t j = p / a.width, i = p - j * a.width;
	const float s = a.scale[b];
	if (s == 1.0f) { a.dst[e] = a.src[e]; return; }
	uint32_t ia, ib, ja, jb;
	float fx, fy;
	optics_axis(i, a.cx, s, a.width, ia, ib, fx);
	optics_axis(j, a.cy, s, a.height, ja, jb, fy);
	const float* const ra = a.src + (size_t)ja * a.width * a.B + b;
	const float* const rb = a.src + (size_t)jb * a.width * a.B + b;
	const float gx = 1.0f - fx, gy = 1.0f - fy;
	const float lo = ra[(size_t)ia * a.B] * gx + ra[(size_t)ib * a.B] * fx;
	const float hi = rb[(size_t)ia * a.B] * gx + rb[(size_t)ib * a.B] * fx;
	a.dst[e] = lo * gy + hi * fy;
}

// The per-bin tables into LDS (the header comment of this file): r_b and the 2 R + 1 taps of every bin
__device__ __forceinline__ void optics_stage_tables(const SsxOpticsArgs& a, uint32_t* radius, float* taps) {
	const uint32_t K = 2u * a.R + 1u;
	for (uint32_t t = threadIdx.x; t < a.B; t += SSX_OPTICS_LANES) radius[t] = a.radius[t];
	for (uint32_t t = threadIdx.x; t < a.B * K; t += SSX_OPTICS_LANES) taps[t] = a.taps[t];
}

// BLUR along i.  One 256-lane workgroup takes a SEGMENT of SSX_OPTICS_SEG = 2048 consecutive elements of one row (eight per lane, 32 pixels at B = 64) and
// stages it with an apron of R pixels = R * B elements either side in LDS -- at most 2048 + 2 * 12 * 64 = 3584 floats, 14 KB -- the pixel index clamped to the
// row while staging, so the walk needs no clamp.  At the worst case (B = 64, R = 12) the apron is 1536 elements for 2048 outputs and the tables are 1664 words
// for 2048 outputs; a global read is saved per tap beyond what the apron costs: 25 reads per output become 1.75.  The staging reads consecutive global
// addresses (except where the clamp repeats the border pixel) and writes consecutive LDS words.
// THE WALK IS WAVE-UNIFORM IN d: every lane steps d = -Rmax .. Rmax (Rmax: the largest r_b of the call, from the host) and takes a step only where |d| <= its
// own r_b, so its additions are still those of -r_b .. r_b in ascending order.  At step d the lanes that take it read word R * B + o + d * B for consecutive o:
// the 32 lanes of a ds_read_b32 group cover 32 consecutive words, 32 banks, whatever B and however the radii are mixed -- with a per-lane start at -r_b the
// lanes of a group would sit at different d and collide for every B that is no multiple of 32.  The tap read at step d is word b * (2 R + 1) + R + d, an odd
// stride over the bins of the group (this file's header).
#define SSX_OPTICS_SEG 2048u
extern "C" __global__ void __launch_bounds__(SSX_OPTICS_LANES) ssx_optics_blur_h_kernel(SsxOpticsArgs a, uint32_t segs) {
	__shared__ float stage[SSX_OPTICS_SEG + 2u * SSX_OPTICS_MAX_RADIUS * 64u];
	__shared__ float taps[64u * SSX_OPTICS_MAX_TAPS];
	__shared__ uint32_t radius[64u];
	const uint32_t t = threadIdx.x, B = a.B, R = a.R, K = 2u * R + 1u;
	const uint32_t j = blockIdx.x / segs, seg = blockIdx.x - j * segs;
	const size_t row_elems = (size_t)a.width * B, e0 = (size_t)seg * SSX_OPTICS_SEG;
	const float* const row = a.src + (size_t)j * row_elems;
	optics_stage_tables(a, radius, taps);
	const uint32_t n_e = (uint32_t)min((size_t)SSX_OPTICS_SEG, row_elems - e0), staged = n_e + 2u * R * B;
	const int last = (int)a.width - 1;
	const bool narrow = row_elems + 2u * R * B <= 0xFFFFFFFFull;                         // (uniform) the element index fits 32 bits: no 64-bit division
	for (uint32_t s = t; s < staged; s += SSX_OPTICS_LANES) {
		const size_t u = e0 + s;                                                         // the element, R * B ahead of where it lies
		const uint32_t up = narrow ? (uint32_t)u / B : (uint32_t)(u / B);
		const uint32_t b = (uint32_t)(u - (size_t)up * B);
		const int pi = (int)up - (int)R;
		stage[s] = row[(size_t)min(max(pi, 0), last) * B + b];
	}
	__syncthreads();
	const int Rm = (int)a.Rmax;
	const uint32_t b0 = narrow ? (uint32_t)e0 % B : (uint32_t)(e0 % B);
	for (uint32_t o = t; o < n_e; o += SSX_OPTICS_LANES) {
		const uint32_t b = (b0 + o) % B;
		const int r = (int)radius[b];
		const float* const mine = stage + R * B + o;
		const float* const k = taps + b * K + R;
		float acc = r ? 0.0f : mine[0];
		for (int d = -Rm; d <= Rm; ++d)
			if (d >= -r && d <= r && r) acc = acc + mine[d * (int)B] * k[d];
		a.dst[(size_t)j * row_elems + e0 + o] = acc;
	}
}

// BLUR along j.  One workgroup takes 256 consecutive elements of a row and a STRIP of SSX_OPTICS_ROWS = 8 output rows: the tables are staged once for 2048
// outputs, a lane's bin, radius and taps are the same for its eight rows, and the 2 r + 1 source rows of consecutive output rows overlap inside one workgroup.
// Lane t reads element e of rows clamp(j + d): every read of a wave is 256 consecutive bytes.  The walk is uniform in d as in the horizontal pass.
#define SSX_OPTICS_ROWS 8u
extern "C" __global__ void __launch_bounds__(SSX_OPTICS_LANES) ssx_optics_blur_v_kernel(SsxOpticsArgs a, uint32_t chunks) {
	__shared__ float taps[64u * SSX_OPTICS_MAX_TAPS];
	__shared__ uint32_t radius[64u];
	const uint32_t t = threadIdx.x, B = a.B, R = a.R, K = 2u * R + 1u;
	const uint32_t strip = blockIdx.x / chunks, chunk = blockIdx.x - strip * chunks;
	const size_t row_elems = (size_t)a.width * B, e = (size_t)chunk * SSX_OPTICS_LANES + t;
	optics_stage_tables(a, radius, taps);
	__syncthreads();
	if (e >= row_elems) return;
	const uint32_t b = row_elems <= 0xFFFFFFFFull ? (uint32_t)e % B : (uint32_t)(e % B);
	const int r = (int)radius[b], Rm = (int)a.Rmax, last = (int)a.height - 1;
	const float* const col = a.src + e;
	const float* const k = taps + b * K + R;
	const uint32_t j0 = strip * SSX_OPTICS_ROWS, j1 = min(j0 + SSX_OPTICS_ROWS, a.height);
	for (uint32_t j = j0; j < j1; ++j) {
		float acc = r ? 0.0f : col[(size_t)j * row_elems];
		for (int d = -Rm; d <= Rm; ++d)
			if (d >= -r && d <= r && r) acc = acc + col[(size_t)min(max((int)j + d, 0), last) * row_elems] * k[d];
		a.dst[(size_t)j * row_elems + e] = acc;
	}
}

namespace {

// The caller's parameters, checked and copied: what the kernels take (scale, radius and taps still the caller's host pointers)
struct OpticsParams { float cx, cy; uint32_t R, Rmax; const float* scale; const uint32_t* radius; const float* taps; bool warps, blurs; };

int optics_take_params(ssx_ctx* ctx, const char* what, const ssx_optics_params* in, uint32_t B, OpticsParams* o) {
	if (!in) return fail(ctx, SSX_ERR_ARG, fmt("%s: optics must not be NULL", what));
	if (in->struct_size != sizeof(ssx_optics_params)) return fail(ctx, SSX_ERR_ARG, "ssx_optics_params.struct_size mismatch");
	if (in->max_radius > SSX_OPTICS_MAX_RADIUS) return fail(ctx, SSX_ERR_ARG, fmt("ssx_optics_params.max_radius = %u: need 0..%u", in->max_radius, SSX_OPTICS_MAX_RADIUS));
	if (!in->scale || !in->radius || !in->taps) return fail(ctx, SSX_ERR_ARG, "ssx_optics_params: scale, radius and taps must not be NULL");
	if (!std::isfinite(in->cx) || !std::isfinite(in->cy)) return fail(ctx, SSX_ERR_ARG, "ssx_optics_params: cx and cy must be finite");
	o->cx = in->cx; o->cy = in->cy; o->R = in->max_radius; o->scale = in->scale; o->radius = in->radius; o->taps = in->taps;
	o->warps = o->blurs = false; o->Rmax = 0u;
	for (uint32_t b = 0; b < B; ++b) {
		if (in->radius[b] > in->max_radius) return fail(ctx, SSX_ERR_ARG, fmt("ssx_optics_params.radius[%u] = %u: above max_radius = %u", b, in->radius[b], in->max_radius));
		if (!(in->scale[b] > 0.0f) || !std::isfinite(in->scale[b])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_optics_params.scale[%u] = %g: a magnification must be finite and > 0", b, (double)in->scale[b]));
		o->warps = o->warps || in->scale[b] != 1.0f;
		o->blurs = o->blurs || in->radius[b] != 0u;
		o->Rmax = std::max(o->Rmax, in->radius[b]);
	}
	return SSX_OK;
}

// d_optics: two images [pixels][B] (16-byte aligned: the unpack kernel stores float4s) and the parameter block scale [B] | radius [B] | taps [B][2 R + 1]
struct OpticsBuffers { float* img[2]; float* scale; uint32_t* radius; float* taps; };
int optics_buffers(ssx_ctx* ctx, size_t pixels, uint32_t B, const OpticsParams& o, OpticsBuffers* d) {
	const size_t K = 2u * o.R + 1u;
	if (const int rc = carve(ctx, ctx->d_optics, [&](Carver& c) {
		for (int x = 0; x < 2; ++x) d->img[x] = reinterpret_cast<float*>(c.take<float4>(pixels * B / 4u));
		d->scale = c.take<float>(B);
		d->radius = c.take<uint32_t>(B);
		d->taps = c.take<float>((size_t)B * K);
	})) return rc;
	SSX_HIP(ctx, hipMemcpy(d->scale, o.scale, B * sizeof(float), hipMemcpyHostToDevice));          // (blocking: the caller's arrays)
	SSX_HIP(ctx, hipMemcpy(d->radius, o.radius, B * sizeof(uint32_t), hipMemcpyHostToDevice));
	SSX_HIP(ctx, hipMemcpy(d->taps, o.taps, (size_t)B * K * sizeof(float), hipMemcpyHostToDevice));
	return SSX_OK;
}

// WARP and BLUR on `src` (one of d.img, or a buffer of somebody else's that is only read): the passes some bin needs, each from where the last one wrote into
// the image of d that is not being read.  *result: where the bins behind the lens lie -- `src` itself when no pass ran.
int optics_device(ssx_ctx* ctx, const OpticsBuffers& d, const OpticsParams& o, uint32_t width, uint32_t height, uint32_t B, const float* src, const float** result) {
	SsxOpticsArgs a{};
	a.scale = d.scale; a.radius = d.radius; a.taps = d.taps;
	a.width = width; a.height = height; a.B = B; a.R = o.R; a.Rmax = o.Rmax; a.cx = o.cx; a.cy = o.cy;
	const size_t pixels = (size_t)width * height;
	auto free_image = [&d](const float* busy) { return busy == d.img[0] ? d.img[1] : d.img[0]; };
	if (o.warps) {
		a.src = src; a.dst = free_image(src);
		hipLaunchKernelGGL(ssx_optics_warp_kernel, blocks_of(pixels * B), dim3(SSX_OPTICS_LANES), 0, ctx->stream, a);
		SSX_HIP(ctx, hipGetLastError());
		src = a.dst;
	}
	if (o.blurs) {
		const size_t row_elems = (size_t)width * B;
		const uint32_t segs = (uint32_t)((row_elems + SSX_OPTICS_SEG - 1u) / SSX_OPTICS_SEG), chunks = (uint32_t)((row_elems + SSX_OPTICS_LANES - 1u) / SSX_OPTICS_LANES);
		const uint32_t strips = (height + SSX_OPTICS_ROWS - 1u) / SSX_OPTICS_ROWS;
		a.src = src; a.dst = free_image(src);
		hipLaunchKernelGGL(ssx_optics_blur_h_kernel, dim3((uint32_t)((size_t)segs * height)), dim3(SSX_OPTICS_LANES), 0, ctx->stream, a, segs);
		SSX_HIP(ctx, hipGetLastError());
		a.src = a.dst; a.dst = free_image(a.src);
		hipLaunchKernelGGL(ssx_optics_blur_v_kernel, dim3((uint32_t)((size_t)chunks * strips)), dim3(SSX_OPTICS_LANES), 0, ctx->stream, a, chunks);
		SSX_HIP(ctx, hipGetLastError());
		src = a.dst;
	}
	*result = src;
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_optics_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q, const ssx_optics_params* optics, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_optics_images";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if (!q || !out) return fail(ctx, SSX_ERR_ARG, fmt("%s: q and out must not be NULL", what));
	int rc = denoise_check_size(ctx, width, height, what);
	if (rc) return rc;
	OpticsParams o;
	if ((rc = optics_take_params(ctx, what, optics, bins, &o))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	OpticsBuffers d;
	if ((rc = optics_buffers(ctx, pixels, bins, o, &d))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d.img[0], q, pixels * bins * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	const float* result = nullptr;
	if ((rc = optics_device(ctx, d, o, width, height, bins, d.img[0], &result))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, result, pixels * bins * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_spectral_develop_optics(ssx_ctx* ctx, const ssx_denoise_params* denoise, const ssx_optics_params* optics, const float* weights, uint32_t channels,
                                float* out, float* bins_out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_develop_optics";
	const bool develops = out || weights;
	int rc = SSX_OK;
	if (develops && (rc = develop_check(ctx, what, channels, weights))) return rc;
	ssx_denoise_params dp;
	if (denoise && (rc = denoise_take_params(ctx, denoise, &dp))) return rc;
	if ((rc = develop_state_ready(ctx, what, denoise != nullptr))) return rc;
	const ssx_render_params& p = ctx->cur;
	if (p.tile_stride != 1u) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context owns one tile in %u (tile_stride): a blur needs its neighbours -- gather the bins and use ssx_optics_images", what, p.tile_stride));
	const uint32_t B = ctx->spectral_bins;
	OpticsParams o;
	if ((rc = optics_take_params(ctx, what, optics, B, &o))) return rc;
	const size_t pixels = (size_t)p.width * p.height;
	OpticsBuffers d;
	if ((rc = optics_buffers(ctx, pixels, B, o, &d))) return rc;
	const float* src = nullptr;
	if (denoise) { // the filter as ssx_denoise_spectral runs it; its ratio, row-major in the channel buffers' staging area, is q
		DenoiseBuffers b;
		ChannelBuffers cb;
		if ((rc = denoise_spectral_device(ctx, dp, &b, &cb))) return rc;
		src = cb.stage;
	} else {
		SsxOpticsArgs a{};
		a.S = ctx->d_spectral_sums.as<const double>(); a.dst = d.img[0];
		a.g = pixel_grid(&p);
		a.width = p.width; a.height = p.height; a.B = B;
		a.M = (double)(B / 4u); a.n = (double)ctx->done_spp.load();
		hipLaunchKernelGGL(ssx_optics_unpack_kernel, dim3(owned_tiles(p)), dim3(64), 0, ctx->stream, a);
		SSX_HIP(ctx, hipGetLastError());
		src = d.img[0];
	}
	const float* result = nullptr;
	if ((rc = optics_device(ctx, d, o, p.width, p.height, B, src, &result))) return rc;
	if (develops) {
		DevelopBuffers dv;
		if ((rc = develop_buffers(ctx, pixels, B, channels, weights, 0, &dv))) return rc;
		SsxDevelopArgs a{};
		a.q = result; a.W = dv.W; a.out = dv.out;
		a.B = B; a.C = channels; a.pixels = (uint32_t)pixels;
		if ((rc = launch_develop_images(ctx, a))) return rc;
		if ((rc = develop_read_back(ctx, dv, pixels, channels, out))) return rc;
	} else SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (bins_out) SSX_HIP(ctx, hipMemcpy(bins_out, result, pixels * B * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

} // extern "C"

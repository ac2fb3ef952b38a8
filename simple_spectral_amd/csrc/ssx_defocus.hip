// ssx_defocus.hip -- depth of field after the render (include/ssx.h, "Depth of field after the render"): per (pixel, bin) a circle-of-confusion gather over a
// disc of up to 25 x 25 sources on q [height][width][B], row-major, steered by the depth guide.  Part of ssx_api.hip's translation unit, behind ssx_optics.hip
// (the unpack kernel, optics_take_params, optics_buffers, optics_device), ssx_develop.hip, ssx_spectral.hip (carve, valid_bins) and ssx_denoise.hip (blocks_of,
// denoise_check_size, ensure_guides, guides_of, denoise_spectral_device).  Two kernels, no atomics, a lane writes only its own output.  Every product is rounded
// before its add (the build's -ffp-contract=off); 1.0f / x and x / y are the compiler's correctly rounded divisions.
//
// PREPARE is one lane per element: inv[p] and a[p][b].  c[p][b] is not stored: it is three operations on inv[p] and f_b -- a subtraction, a product with |.| as
// an operand modifier, a min -- and the gather, whose lane keeps f_b in a register for its whole life, redoes them to the same bits.  That keeps a staged source
// at 8 bytes per bin instead of 12, which is what lets a second workgroup onto the CU at R = 12 (below).  a is stored because it costs a division.
//
// GATHER is the hot path: up to (2 R + 1)^2 taps per output, each a handful of VALU operations on three LDS words.  It is not separable (ce depends on source
// and destination), so ssx_optics_blur_* cannot serve it.  One 256-lane workgroup takes a TILE of 16 x 16 pixels and a CHUNK of 4 consecutive bins and stages
// the tile with its apron of R pixels on every side in LDS: per staged pixel {a, q} for the 4 bins (8 floats) and inv (1 float), 36 bytes; plus the 289
// distances sqrtf(d2), d2 = 0 .. 2 * 12^2, which the host makes (correctly rounded) and every workgroup copies.  (16 + 2 R)^2 * 36 + 1156 bytes: 18.6 KB at
// R = 3, 38 KB at R = 8, 58.8 KB at R = 12 -- 8, 4 and 2 workgroups on a CU's 160 KB.  The chunk is 4 bins because the apron is paid per bin: at R = 12 the
// staged area is 6.25 times the tile, and 8 bins would leave one workgroup -- one wave per SIMD -- on the CU.  Every B is a multiple of 4, so no chunk is ragged.
//
// Lanes run along the interleaved (pixel, bin) axis of a tile row, as in ssx_optics.hip: lane t has bin t & 3 of the chunk, pixel (t >> 2) & 15 of the row, and
// rows (t >> 6) + 4 k, k = 0..3 -- a wave is one tile row, 16 pixels x 4 bins, and a lane carries four outputs through one walk, so that four independent
// chains of additions hide the LDS latency that two waves per SIMD cannot.  A wave's store is 16 runs of 16 bytes, B * 4 bytes apart: whole lines at B = 4, a
// quarter of each line at B = 64, the other chunks' workgroups -- neighbours in the grid -- filling the rest in the L2.  Against 45 to 517 taps per output the
// store is noise; the chunk size is set by LDS, not by the store.
//
// THE WALK IS WAVE-UNIFORM IN (dy, dx): the loop counters are scalars, the distance is one broadcast LDS word, and a tap with dx^2 + dy^2 >= (R + 1)^2 -- dist >=
// R + 1 >= ce + 1, never covered -- is skipped for the whole wave (21 % of the square).  The per-lane `taken` test is a select on the two sums, not a branch.
// BANKS, from the rule (ds_read_b64: two groups of 32 lanes, bank = word address mod 64; ds_read_b32: two groups of 32, bank = word mod 32): at a tap the 32
// lanes of a group read {a, q} at 8-byte words (row * SW + col0 + dx) * 4 + 0 .. 31 -- 32 consecutive float2, 64 consecutive words, 64 banks; and inv at words
// row * SW + col0 + dx + 0 .. 7, each by four lanes (a broadcast), 8 banks.  Neither depends on R, B or the tile's position: no conflicts.  The staging writes
// consecutive words from consecutive lanes.
// OUTSIDE THE IMAGE a staged source has a = 0 and q = 0, and the test is w > 0.0f with w = cover * a instead of cover > 0.0f.  Inside the image the two are
// the same test: a is finite and >= 1 / (pi * 156.34) > 0.002, and a positive cover is a difference of two binary32 numbers in [1, 14), a multiple of 2^-23,
// so w neither underflows nor is NaN (c is in [0, R] whatever inv is: K > 0 here, and inf * K = inf gives R).  Outside, w is 0 and the tap is skipped.

#define SSX_DEFOCUS_LANES 256u
#define SSX_DEFOCUS_TILE 16u
#define SSX_DEFOCUS_CHUNK 4u
#define SSX_DEFOCUS_DIST (2u * SSX_DEFOCUS_MAX_RADIUS * SSX_DEFOCUS_MAX_RADIUS + 1u)   // 289: every dx^2 + dy^2 of the walk

struct SsxDefocusArgs {
	const float* q;           // [height][width][B]
	const float* depth;       // prepare kernel: [height][width]
	float* inv;               // [height][width]: written by the prepare kernel, read by the gather
	float* a;                 // [height][width][B]: likewise
	float* dst;               // gather kernel: [height][width][B]
	const float* focus;       // [B]
	const float* dist;        // [SSX_DEFOCUS_DIST]: sqrtf((float)d2)
	uint32_t width, height, B, R;
	float K;
};

// c[s][b] of the header from inv[s]: min(fabsf(inv - f) * K, (float)R)
__device__ __forceinline__ float defocus_coc(float inv, float f, float K, float Rf) {
	const float c = fabsf(inv - f) * K;
	return c < Rf ? c : Rf;
}

// One lane per element e = p * B + b; the lane of bin 0 also writes its pixel's inv.
extern "C" __global__ void __launch_bounds__(SSX_DEFOCUS_LANES) ssx_defocus_prepare_kernel(SsxDefocusArgs a) {
	const size_t e = (size_t)blockIdx.x * SSX_DEFOCUS_LANES + threadIdx.x;
	const size_t pixels = (size_t)a.width * a.height;
	if (e >= pixels * a.B) return;
	const uint32_t p = pixels * a.B <= 0xFFFFFFFFull ? (uint32_t)e / a.B : (uint32_t)(e / a.B);   // (uniform) 32-bit division wherever the image allows it
	const uint32_t b = (uint32_t)(e - (size_t)p * a.B);
	const float d = a.depth[p];
	const float inv = d > 0.0f ? 1.0f / d : 0.0f;
	const float c = defocus_coc(inv, a.focus[b], a.K, (float)a.R);
	a.a[e] = 1.0f / (3.14159274f * ((c * c + c) + 0.333333343f));
	if (b == 0u) a.inv[p] = inv;
}

extern __shared__ __attribute__((aligned(16))) float defocus_lds[];

// blockIdx.x = (tile_y * tiles_x + tile_x) * (B / 4) + chunk: the chunks of a tile are neighbours in the grid and share the tile's lines of a, q and dst.
extern "C" __global__ void __launch_bounds__(SSX_DEFOCUS_LANES) ssx_defocus_gather_kernel(SsxDefocusArgs a, uint32_t tiles_x) {
	const uint32_t t = threadIdx.x, B = a.B, chunks = B / SSX_DEFOCUS_CHUNK;
	const int R = (int)a.R, SW = (int)SSX_DEFOCUS_TILE + 2 * R;                          // the staged square's side
	const uint32_t n_s = (uint32_t)(SW * SW);
	float2* const aq = reinterpret_cast<float2*>(defocus_lds);                            // [SW][SW][4] {a, q}
	float* const inv_l = defocus_lds + (size_t)n_s * 2u * SSX_DEFOCUS_CHUNK;              // [SW][SW]
	float* const dist_l = inv_l + n_s;                                                   // [SSX_DEFOCUS_DIST]
	const uint32_t tile = blockIdx.x / chunks, b0 = (blockIdx.x - tile * chunks) * SSX_DEFOCUS_CHUNK;
	const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
	const int x0 = (int)(tx * SSX_DEFOCUS_TILE), y0 = (int)(ty * SSX_DEFOCUS_TILE), W = (int)a.width, H = (int)a.height;
	for (uint32_t idx = t; idx < n_s * SSX_DEFOCUS_CHUNK; idx += SSX_DEFOCUS_LANES) {
		const uint32_t s = idx / SSX_DEFOCUS_CHUNK, bl = idx % SSX_DEFOCUS_CHUNK;
		const int sy = (int)(s / (uint32_t)SW), sx = (int)s - sy * SW;
		const int gx = x0 + sx - R, gy = y0 + sy - R;
		float2 v = make_float2(0.0f, 0.0f);
		float iv = 0.0f;
		if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
			const size_t pix = (size_t)gy * a.width + (uint32_t)gx, e = pix * B + b0 + bl;
			v.x = a.a[e]; v.y = a.q[e];
			iv = a.inv[pix];
		}
		aq[idx] = v;
		if (bl == 0u) inv_l[s] = iv;
	}
	for (uint32_t k = t; k < SSX_DEFOCUS_DIST; k += SSX_DEFOCUS_LANES) dist_l[k] = a.dist[k];
	__syncthreads();
	const uint32_t bl = t & 3u, col = (t >> 2) & 15u, row0 = t >> 6;
	const float f = a.focus[b0 + bl], K = a.K, Rf = (float)R;
	int centre[4];
	float invp[4], cp[4], sw[4], sq[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		centre[k] = ((int)row0 + 4 * k + R) * SW + (int)col + R;
		invp[k] = inv_l[centre[k]];
		cp[k] = defocus_coc(invp[k], f, K, Rf);
		sw[k] = 0.0f; sq[k] = 0.0f;
	}
	const int lim = (R + 1) * (R + 1);
	for (int dy = -R; dy <= R; ++dy)
		for (int dx = -R; dx <= R; ++dx) {
			const int d2 = dx * dx + dy * dy;
			if (d2 >= lim) continue;                                                     // (uniform) never covered
			const float dist = dist_l[d2];
			const int off = dy * SW + dx;
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const int s = centre[k] + off;
				const float invs = inv_l[s];
				const float2 v = aq[s * (int)SSX_DEFOCUS_CHUNK + (int)bl];
				const float cs = defocus_coc(invs, f, K, Rf);
				const float cm = cs < cp[k] ? cs : cp[k];
				const float ce = invs < invp[k] ? cm : cs;
				float cover = (ce + 1.0f) - dist;
				cover = cover > 0.0f ? cover : 0.0f;
				cover = cover < 1.0f ? cover : 1.0f;
				const float w = cover * v.x;
				const bool taken = w > 0.0f;                                             // cover > 0 and inside the image (this file's header)
				const float sw1 = sw[k] + w, sq1 = sq[k] + w * v.y;
				sw[k] = taken ? sw1 : sw[k];
				sq[k] = taken ? sq1 : sq[k];
			}
		}
	const int gx = x0 + (int)col;
	if (gx >= W) return;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int gy = y0 + (int)row0 + 4 * k;
		if (gy < H) a.dst[((size_t)gy * a.width + (uint32_t)gx) * B + b0 + bl] = sq[k] / sw[k];
	}
}

namespace {

size_t defocus_lds_bytes(uint32_t R) {
	const size_t side = SSX_DEFOCUS_TILE + 2u * R;
	return (side * side * (2u * SSX_DEFOCUS_CHUNK + 1u) + SSX_DEFOCUS_DIST) * sizeof(float);
}

// The caller's parameters, checked and copied (focus still the caller's host pointer); active: DEFOCUS is not the identity
struct DefocusParams { uint32_t R; float K; const float* focus; bool active; };

int defocus_take_params(ssx_ctx* ctx, const char* what, const ssx_defocus_params* in, uint32_t B, DefocusParams* o) {
	if (!in) return fail(ctx, SSX_ERR_ARG, fmt("%s: defocus must not be NULL", what));
	if (in->struct_size != sizeof(ssx_defocus_params)) return fail(ctx, SSX_ERR_ARG, "ssx_defocus_params.struct_size mismatch");
	if (in->max_radius > SSX_DEFOCUS_MAX_RADIUS) return fail(ctx, SSX_ERR_ARG, fmt("ssx_defocus_params.max_radius = %u: need 0..%u", in->max_radius, SSX_DEFOCUS_MAX_RADIUS));
	if (!(in->gain >= 0.0f) || !std::isfinite(in->gain)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_defocus_params.gain = %g: must be finite and >= 0", (double)in->gain));
	if (!in->focus) return fail(ctx, SSX_ERR_ARG, "ssx_defocus_params: focus must not be NULL");
	for (uint32_t b = 0; b < B; ++b)
		if (!(in->focus[b] >= 0.0f) || !std::isfinite(in->focus[b]))
			return fail(ctx, SSX_ERR_ARG, fmt("ssx_defocus_params.focus[%u] = %g: an inverse focus distance must be finite and >= 0", b, (double)in->focus[b]));
	o->R = in->max_radius; o->K = in->gain; o->focus = in->focus;
	o->active = in->max_radius != 0u && in->gain != 0.0f;
	return SSX_OK;
}

// d_defocus: out | a ([pixels][B] each) | inv [pixels] | focus [B] | dist [289], and for the pure entry the caller's q [pixels][B] and depth [pixels]
struct DefocusBuffers { float* out; float* a; float* inv; float* focus; float* dist; float* q; float* depth; };
int defocus_buffers(ssx_ctx* ctx, size_t pixels, uint32_t B, const DefocusParams& o, bool pure, DefocusBuffers* d) {
	if (const int rc = carve(ctx, ctx->d_defocus, [&](Carver& c) {
		d->out = reinterpret_cast<float*>(c.take<float4>(pixels * B / 4u));
		d->a = reinterpret_cast<float*>(c.take<float4>(pixels * B / 4u));
		d->inv = c.take<float>(pixels);
		d->focus = c.take<float>(B);
		d->dist = c.take<float>(SSX_DEFOCUS_DIST);
		d->q = pure ? reinterpret_cast<float*>(c.take<float4>(pixels * B / 4u)) : nullptr;
		d->depth = pure ? c.take<float>(pixels) : nullptr;
	})) return rc;
	float dist[SSX_DEFOCUS_DIST];
	for (uint32_t k = 0; k < SSX_DEFOCUS_DIST; ++k) dist[k] = std::sqrt((float)k);                 // binary32 sqrt: correctly rounded
	SSX_HIP(ctx, hipMemcpy(d->focus, o.focus, B * sizeof(float), hipMemcpyHostToDevice));          // (blocking: the caller's array, and `dist`)
	SSX_HIP(ctx, hipMemcpy(d->dist, dist, sizeof dist, hipMemcpyHostToDevice));
	return SSX_OK;
}

// DEFOCUS on `src` with `depth` (both only read), queued on the context's stream; the result is in d.out.  Only for o.active.
int defocus_device(ssx_ctx* ctx, const DefocusBuffers& d, const DefocusParams& o, uint32_t width, uint32_t height, uint32_t B, const float* src, const float* depth) {
	SsxDefocusArgs a{};
	a.q = src; a.depth = depth; a.inv = d.inv; a.a = d.a; a.dst = d.out; a.focus = d.focus; a.dist = d.dist;
	a.width = width; a.height = height; a.B = B; a.R = o.R; a.K = o.K;
	const size_t pixels = (size_t)width * height;
	hipLaunchKernelGGL(ssx_defocus_prepare_kernel, blocks_of(pixels * B), dim3(SSX_DEFOCUS_LANES), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	const uint32_t tiles_x = (width + SSX_DEFOCUS_TILE - 1u) / SSX_DEFOCUS_TILE, tiles_y = (height + SSX_DEFOCUS_TILE - 1u) / SSX_DEFOCUS_TILE;
	const size_t blocks = (size_t)tiles_x * tiles_y * (B / SSX_DEFOCUS_CHUNK);                     // <= 2^28: at most 2^24 tiles (denoise_check_size; an image one pixel wide) times 16 chunks
	hipLaunchKernelGGL(ssx_defocus_gather_kernel, dim3((uint32_t)blocks), dim3(SSX_DEFOCUS_LANES), defocus_lds_bytes(o.R), ctx->stream, a, tiles_x);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_defocus_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q, const float* depth, const ssx_defocus_params* defocus, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_defocus_images";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if (!q || !depth || !out) return fail(ctx, SSX_ERR_ARG, fmt("%s: q, depth and out must not be NULL", what));
	int rc = denoise_check_size(ctx, width, height, what);
	if (rc) return rc;
	DefocusParams o;
	if ((rc = defocus_take_params(ctx, what, defocus, bins, &o))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	if (!o.active) { // a copy, bit for bit; nothing is allocated or launched
		if (out != q) std::memmove(out, q, pixels * bins * sizeof(float));
		return SSX_OK;
	}
	DefocusBuffers d;
	if ((rc = defocus_buffers(ctx, pixels, bins, o, true, &d))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d.q, q, pixels * bins * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.depth, depth, pixels * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	if ((rc = defocus_device(ctx, d, o, width, height, bins, d.q, d.depth))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, d.out, pixels * bins * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_spectral_develop_lens(ssx_ctx* ctx, const ssx_denoise_params* denoise, const ssx_defocus_params* defocus, const ssx_optics_params* optics, const float* weights,
                              uint32_t channels, float* out, float* bins_out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_develop_lens";
	const bool develops = out || weights;
	int rc = SSX_OK;
	if (develops && (rc = develop_check(ctx, what, channels, weights))) return rc;
	ssx_denoise_params dp;
	if (denoise && (rc = denoise_take_params(ctx, denoise, &dp))) return rc;
	if ((rc = develop_state_ready(ctx, what, denoise != nullptr))) return rc;
	const ssx_render_params& p = ctx->cur;
	if (p.tile_stride != 1u) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context owns one tile in %u (tile_stride): a blur needs its neighbours -- gather the bins and use ssx_defocus_images and ssx_optics_images", what, p.tile_stride));
	const uint32_t B = ctx->spectral_bins;
	DefocusParams f{};
	if (defocus && (rc = defocus_take_params(ctx, what, defocus, B, &f))) return rc;
	// without a lens: the identity's tables, so that the unpack kernel has its image (optics_buffers) and no pass runs (optics_device)
	const std::vector<float> one(B, 1.0f);
	const std::vector<uint32_t> zero(B, 0u);
	OpticsParams o{ 0.0f, 0.0f, 0u, 0u, one.data(), zero.data(), one.data(), false, false };
	if (optics && (rc = optics_take_params(ctx, what, optics, B, &o))) return rc;
	if (f.active && !ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
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
	if (f.active) { // DEFOCUS first: the depth guide is registered to the unwarped pixels
		if ((rc = ensure_guides(ctx, p.width, p.height))) return rc;
		DefocusBuffers fb;
		if ((rc = defocus_buffers(ctx, pixels, B, f, false, &fb))) return rc;
		if ((rc = defocus_device(ctx, fb, f, p.width, p.height, B, src, guides_of(ctx, pixels).depth))) return rc;
		src = fb.out;
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

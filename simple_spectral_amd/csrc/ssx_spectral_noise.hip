// ssx_spectral_noise.hip -- the spectral noise figure: per 8x8 tile and bin, the summed variance of the pixels' bin means, their summed means and the numbers of
// estimable and unestimated pixels, reduced from the native S, Q, N state in a fixed order, and the totals over the tiles (include/ssx.h, "Spectral noise
// figure").  Part of ssx_api.hip's translation unit, behind ssx_spectral_stats.hip (moments_ready, moment_deviations; the state S, Q, N it reads).  Everything
// here is binary64 with IEEE + - * /, no contraction (the build's -ffp-contract=off), in the order the header writes: a restatement in numpy gives the same bits
// (tests/spectral_noise_ref.py).

struct SsxNoiseArgs {
	const double* S; const double* Q; const uint32_t* N;   // [tile slot][bin][64], [tile slot][bin][64], [tile slot][m][64]: the device layout, read where it lies
	const uint8_t* mask;                                   // [height][width], row 0 = bottom; NULL: every pixel
	double* tEV; double* tEM; uint32_t* tPP; uint32_t* tPU; // [tiles][B], indexed by the tile's image index t = ty * tiles_x + tx
	SsxPixelGrid g;
	uint32_t M;
};

// Stage 1: one 256-lane workgroup per owned tile slot; the bins go through LDS in chunks of 32.
//   in:   lane = (pixel of the tile, wave w); wave w takes bins w, w + 4, ... of the chunk.  Per bin the wave reads S and Q at [slot][b][pixel] -- 512 consecutive
//         bytes each, the layout's fastest index across the lanes: fully coalesced, every byte of S and Q read once -- and N at [slot][b % M][pixel], 256
//         consecutive bytes (read 4 times over the b of one m: from the cache after the first).  The divisions -- two for e, one inside q, one for mu -- run here,
//         64 x 4 wide, not in the sequential walk.  A pixel outside the image or the mask, or with n < 2, stores e = mu = +0.0: the walk then adds +0.0, which
//         leaves a partial that started from +0.0 as it is (the header's bit-neutrality argument; a NaN stays a NaN), so the walk needs no branch.
//   LDS:  e and mu as [32 bins][65] binary64, the pixel's class (0 out, 1 estimable, 2 unestimated) as [32 bins][68] bytes: 33,280 + 2,176 = 35,456 bytes whatever
//         the bin count (four workgroups per CU).  On the way in lane = pixel writes 8-byte address 65 * bin + pixel: 16 consecutive lanes of a ds_write_b64 group
//         cover 32 consecutive banks.  On the way out lane = (quantity, bin) reads 65 * bin + pixel at step `pixel`: a ds_read_b64 is served in two groups of 32
//         lanes over 64 four-byte banks, and a group is the 32 bins of ONE quantity, so it needs 32 distinct bank pairs -- (65 * bin + pixel) mod 32 = (bin + pixel)
//         mod 32, distinct for 32 consecutive bins: the ODD stride is the whole argument; the unpadded 64 would put all 32 lanes on one pair.  The class bytes have a
//         row stride of 17 words, odd again: the 32 lanes of a count quantity read 32 distinct banks, and the two quantities of the wave read the same byte.
//   out:  wave 0 = the lanes of EV | EM, wave 1 = PP | PU (no divergence inside a wave: the quantity selects a pointer or a constant).  Each lane walks the 64
//         pixels in ascending order -- ascending row, then ascending column: the layout's fastest index -- from +0.0 / 0 and stores at [t][b]: 32 consecutive
//         8-byte (4-byte) words per quantity.  No atomics; nothing spills.
#define SSX_NOISE_CHUNK 32u
#define SSX_NOISE_STRIDE 65u       // binary64 elements between the bins' rows
#define SSX_NOISE_CLASS_STRIDE 68u // bytes between the bins' class rows (17 words)
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_noise_tiles_kernel(SsxNoiseArgs a) {
	__shared__ double noise_e[SSX_NOISE_CHUNK * SSX_NOISE_STRIDE], noise_mu[SSX_NOISE_CHUNK * SSX_NOISE_STRIDE];
	__shared__ uint8_t noise_class[SSX_NOISE_CHUNK * SSX_NOISE_CLASS_STRIDE];
	const uint32_t tid = threadIdx.x, px = tid & 63u, w = tid >> 6, slot = blockIdx.x, M = a.M, B = 4u * M;
	uint32_t tx, ty;
	const uint32_t t = tile_of_slot(a.g, slot, tx, ty);
	const uint32_t i = tx * 8u + (px & 7u), j = ty * 8u + (px >> 3);
	bool in = i < a.g.width && j < a.g.height;
	if (in && a.mask) in = a.mask[(size_t)j * a.g.width + i] != 0u;
	for (uint32_t b0 = 0; b0 < B; b0 += SSX_NOISE_CHUNK) {
		const uint32_t nb = min(SSX_NOISE_CHUNK, B - b0);
		for (uint32_t bl = w; bl < nb; bl += 4u) {
			const uint32_t b = b0 + bl;
			double e = 0.0, mu = 0.0;
			uint8_t cls = 0u;
			if (in) {
				const uint32_t n = a.N[((size_t)slot * M + b % M) * 64u + px];
				cls = n >= 2u ? 1u : 2u;
				if (n >= 2u) {
					const size_t at = ((size_t)slot * B + b) * 64u + px;
					e = cell_variance(a.Q[at], a.S[at], n, &mu);
				}
			}
			noise_e[bl * SSX_NOISE_STRIDE + px] = e;
			noise_mu[bl * SSX_NOISE_STRIDE + px] = mu;
			noise_class[bl * SSX_NOISE_CLASS_STRIDE + px] = cls;
		}
		__syncthreads();
		const uint32_t quantity = tid >> 5, bl = tid & 31u;                                  // 0 EV, 1 EM, 2 PP, 3 PU (tid < 128: waves 0 and 1)
		if (tid < 128u && bl < nb) {
			const size_t o = (size_t)t * B + b0 + bl;
			if (quantity < 2u) {
				const double* const src = (quantity ? noise_mu : noise_e) + bl * SSX_NOISE_STRIDE;
				double acc = 0.0;
				for (uint32_t p = 0; p < 64u; ++p) acc += src[p];
				(quantity ? a.tEM : a.tEV)[o] = acc;
			} else {
				const uint8_t* const src = noise_class + bl * SSX_NOISE_CLASS_STRIDE;
				const uint32_t want = quantity - 1u;                                          // PP counts class 1, PU class 2
				uint32_t count = 0u;
				for (uint32_t p = 0; p < 64u; ++p) count += (uint32_t)src[p] == want ? 1u : 0u;
				(quantity == 2u ? a.tPP : a.tPU)[o] = count;
			}
		}
		__syncthreads();                                                                     // (the next chunk overwrites what the walk reads)
	}
}

// Stage 2: one lane per (quantity, bin) -- 4 B <= 256 lanes, one workgroup -- adds the tiles' partials in ascending t, from +0.0 / 0.  The B lanes of a quantity
// read B consecutive words of a tile.  The additions stay in order; the loads do not depend on them, so the loop is unrolled to keep 16 of them in flight (a
// 512 x 512 image has 4096 tiles: one dependent load per addition would cost a memory latency each).  out: EV | EM | PP | PU, [B] eight-byte words each.
extern "C" __global__ void __launch_bounds__(256) ssx_spectral_noise_reduce_kernel(const double* tEV, const double* tEM, const uint32_t* tPP, const uint32_t* tPU, uint64_t* out, uint32_t tiles, uint32_t B) {
	const uint32_t e = threadIdx.x;
	if (e >= 4u * B) return;
	const uint32_t quantity = e / B, b = e - quantity * B;
	if (quantity < 2u) {
		const double* const src = (quantity ? tEM : tEV) + b;
		double total = 0.0;
#pragma unroll 16
		for (uint32_t t = 0; t < tiles; ++t) total += src[(size_t)t * B];
		reinterpret_cast<double*>(out)[e] = total;
	} else {
		const uint32_t* const src = (quantity == 2u ? tPP : tPU) + b;
		uint64_t total = 0ull;
#pragma unroll 16
		for (uint32_t t = 0; t < tiles; ++t) total += src[(size_t)t * B];
		out[e] = total;
	}
}

namespace {

// d_stage: tEV and tEM [tiles][B] binary64, out [4][B], tPP and tPU [tiles][B] uint32, mask [pixels]: nothing of the image's size but the mask (S, Q, N are read where they lie)
struct NoiseBuffers { double* tEV; double* tEM; uint64_t* out; uint32_t* tPP; uint32_t* tPU; uint8_t* mask; size_t partial_bytes; };
int noise_buffers(ssx_ctx* ctx, size_t tiles, uint32_t B, size_t pixels, NoiseBuffers* d) {
	const size_t n = tiles * B;
	return carve(ctx, ctx->d_stage, [&](Carver& c) {
		d->tEV = c.take<double>(n);
		d->tEM = c.take<double>(n);
		d->out = c.take<uint64_t>((size_t)4u * B);
		d->tPP = c.take<uint32_t>(n);
		d->tPU = c.take<uint32_t>(n);
		d->partial_bytes = c.at;                                                             // (from tEV on: what ssx_spectral_noise zeroes in one go)
		d->mask = c.take<uint8_t>(pixels);
	});
}

// The one body of both entry points: the partials are in d already; the second kernel runs, the four [B] arrays come back.
int noise_reduce_device(ssx_ctx* ctx, const NoiseBuffers& d, uint32_t tiles, uint32_t B, double* EV, double* EM, uint64_t* PP, uint64_t* PU) {
	hipLaunchKernelGGL(ssx_spectral_noise_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, d.tEV, d.tEM, d.tPP, d.tPU, d.out, tiles, B);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return copy_planes(ctx, d.out, B, { EV, EM, PP, PU });
}

} // namespace

extern "C" {

int ssx_spectral_noise(ssx_ctx* ctx, const uint8_t* mask, double* EV, double* EM, uint64_t* PP, uint64_t* PU, double* tEV, double* tEM, uint32_t* tPP, uint32_t* tPU) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_noise";
	int rc = moments_ready(ctx, what);
	if (rc) return rc;
	if (!EV || !EM || !PP || !PU) return fail(ctx, SSX_ERR_ARG, fmt("%s: the four [bins] outputs must not be NULL", what));
	const ssx_render_params& p = ctx->cur;
	const uint32_t B = ctx->spectral_bins, tiles = tiles_across(p.width) * tiles_across(p.height), owned = owned_tiles(p);
	const size_t pixels = (size_t)p.width * p.height;
	NoiseBuffers d;
	if ((rc = noise_buffers(ctx, tiles, B, mask ? pixels : 0u, &d))) return rc;
	SSX_HIP(ctx, hipMemsetAsync(d.tEV, 0, d.partial_bytes, ctx->stream));                   // a tile the context does not own: +0.0 and 0
	if (mask) SSX_HIP(ctx, hipMemcpyAsync(d.mask, mask, pixels, hipMemcpyHostToDevice, ctx->stream));
	if (owned) {
		SsxNoiseArgs a{};
		a.S = ctx->d_spectral_sums.as<const double>(); a.Q = ctx->d_spectral_moments.as<const double>(); a.N = ctx->d_spectral_counts.as<const uint32_t>();
		a.mask = mask ? d.mask : nullptr;
		a.tEV = d.tEV; a.tEM = d.tEM; a.tPP = d.tPP; a.tPU = d.tPU;
		a.g = pixel_grid(&p); a.M = B / 4u;
		hipLaunchKernelGGL(ssx_spectral_noise_tiles_kernel, dim3(owned), dim3(256), 0, ctx->stream, a);
		SSX_HIP(ctx, hipGetLastError());
	}
	if ((rc = noise_reduce_device(ctx, d, tiles, B, EV, EM, PP, PU))) return rc;
	const size_t n = (size_t)tiles * B;
	if (tEV) SSX_HIP(ctx, hipMemcpy(tEV, d.tEV, n * 8u, hipMemcpyDeviceToHost));
	if (tEM) SSX_HIP(ctx, hipMemcpy(tEM, d.tEM, n * 8u, hipMemcpyDeviceToHost));
	if (tPP) SSX_HIP(ctx, hipMemcpy(tPP, d.tPP, n * 4u, hipMemcpyDeviceToHost));
	if (tPU) SSX_HIP(ctx, hipMemcpy(tPU, d.tPU, n * 4u, hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_spectral_noise_reduce(ssx_ctx* ctx, uint32_t tiles, uint32_t bins, const double* tEV, const double* tEM, const uint32_t* tPP, const uint32_t* tPU,
                              double* EV, double* EM, uint64_t* PP, uint64_t* PU) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_noise_reduce";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if (tiles < 1u || tiles > (1u << 22)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u tiles: need 1..2^22 (an image of at most 2^28 pixels)", what, tiles));
	if (!tEV || !tEM || !tPP || !tPU || !EV || !EM || !PP || !PU) return fail(ctx, SSX_ERR_ARG, fmt("%s: the partials and the four outputs must not be NULL", what));
	int rc = idle_on_device(ctx);
	if (rc) return rc;
	NoiseBuffers d;
	if ((rc = noise_buffers(ctx, tiles, bins, 0u, &d))) return rc;
	const size_t n = (size_t)tiles * bins;
	SSX_HIP(ctx, hipMemcpyAsync(d.tEV, tEV, n * 8u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.tEM, tEM, n * 8u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.tPP, tPP, n * 4u, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.tPU, tPU, n * 4u, hipMemcpyHostToDevice, ctx->stream));
	return noise_reduce_device(ctx, d, tiles, bins, EV, EM, PP, PU);
}

} // extern "C"

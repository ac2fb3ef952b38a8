// ssx_sensor.hip -- developing onto a sensor (include/ssx.h, "Developing onto a sensor"): SENSOR takes q [height][width][B] to a mosaic raw [height][width]
// (one filter of a 2 x 2 colour filter array per photosite, electrons, noise, ADC), DEMOSAIC takes raw to out [height][width][3] with a 5 x 5 table per
// (phase, channel) and a 3 x 3 matrix.  Part of ssx_api.hip's translation unit, behind ssx_defocus.hip (defocus_take_params, defocus_buffers, defocus_device),
// ssx_optics.hip (the unpack kernel, optics_take_params, optics_buffers, optics_device), ssx_develop.hip (develop_state_ready), ssx_spectral.hip (carve,
// valid_bins) and ssx_denoise.hip (blocks_of, denoise_check_size, ensure_guides, guides_of, denoise_spectral_device).  Two kernels, no atomics, a lane writes
// only its own output.  Every product is rounded before its add (the build's -ffp-contract=off); sqrtf is the compiler's correctly rounded square root.
//
// SENSOR is ssx_develop_images_kernel_g1 with a tail: one lane per pixel, its B floats read once in float4s, memory bound (256 bytes in, 4 or 8 out per pixel
// at B = 64).  The weight row depends on the lane's photosite, and a per-lane row would turn the develop's scalar loads into a gather.  Instead every lane
// accumulates all three channels from W_dev[b][4] -- one 16-byte load at a wave-uniform address per bin, served by the scalar cache, as in ssx_develop.hip --
// and selects its own at the end.  The three chains are independent, so the selected one has the bits of "the accumulation for that one channel".  The cost is
// 6 VALU operations per bin and lane instead of 2: 384 per pixel at B = 64 against 256 bytes of HBM, an eighth of what the memory takes (2.5 us against 17 us
// at 512^2 on paper), so the row's two channels were not singled out (a wave does not stay inside an image row when W is odd).  LDS would cost a barrier and
// buy nothing: no lane indexes the weights by anything of its own.  The noise is 10 rounds of a 32-bit integer hash per pixel, a few dozen VALU operations.
//
// DEMOSAIC: 75 taps per pixel on a one-float image -- at 512^2 one megabyte in, three out; the arithmetic (150 VALU operations per pixel) is nothing.  What
// decides the shape is that the table depends on the pixel's phase.  One lane per 2 x 2 QUAD sees all four phases, every lane the same four: all 300 taps and
// the 9 matrix entries are read at wave-uniform addresses with compile-time offsets (scalar loads again; the loops are unrolled completely), and the lanes
// never diverge.  A 256-lane workgroup takes 32 x 8 quads, a TILE of 64 x 16 pixels, and stages it with its apron of 2 in LDS: 68 x 20 floats = 5440 bytes,
// mirrored while staging (m(k, n) of the header; a staged pixel whose mirror image lies outside the image -- possible only past a ragged tile's end, where no
// lane stores -- is 0).  Tiles start at even coordinates, so a quad's parity is the image's.  A lane then reads its 6 x 6 window as 18 ds_read_b64 (the
// window starts at an even column: 8-byte aligned) into registers and runs the twelve chains of 25 from there.
// BANKS, from the rule (ds_read_b64: two groups of 32 lanes, bank = word address mod 64): a group of 32 lanes is one row of 32 quads, and at each of the 18
// reads it takes 32 consecutive float2 -- 64 consecutive words, 64 banks: no conflicts, whatever the pitch; that is why the tile is 32 quads wide.  The
// staging writes consecutive words from consecutive lanes.  OCCUPANCY: the kernel compiles to 117 VGPRs (allocated 120): four waves per SIMD, four workgroups
// per CU; its 5.4 KB of LDS would allow many more.  512^2 has only 256 workgroups, one per CU, so at that size the kernel's time is the latency of one
// workgroup (stage, barrier, window, 600 VALU operations behind scalar loads, store: 9 us measured, 2.7 times a float4 copy of its bytes), not bandwidth;
// larger images fill the CUs (profiles/r29/NOTES.md).
// The store: a lane writes 6 consecutive floats in each of two rows, a wave 768 consecutive bytes per row: whole lines.

#define SSX_SENSOR_LANES 256u
#define SSX_DEMOSAIC_QX 32u                                  // quads per tile row: one group of 32 lanes
#define SSX_DEMOSAIC_QY 8u
#define SSX_DEMOSAIC_SW (2u * SSX_DEMOSAIC_QX + 4u)          // 68: the staged tile's pitch
#define SSX_DEMOSAIC_SH (2u * SSX_DEMOSAIC_QY + 4u)          // 20
#define SSX_DEMOSAIC_TABLE 312u                              // taps [4][3][25] | ccm [3][3] | padding to 16 bytes

struct SsxSensorArgs {
	const float* q;           // [pixels][B]
	const float* W;           // [B][4]: the three filters' weights per bin, the fourth 0 and never read
	float* raw;               // [pixels]
	float* dn;                // [pixels], or nullptr
	uint32_t width, pixels, B;
	uint32_t cfa;             // two bits per phase
	uint32_t noise, base;     // base = h(h(seed) + frame): the same for every pixel, so the host makes it
	float exposure, inv_exposure, read_var, dn_per_e, e_per_dn, black, white;
};

struct SsxDemosaicArgs {
	const float* raw;         // [height][width]
	const float* table;       // [SSX_DEMOSAIC_TABLE]
	float* out;               // [height][width][3]
	uint32_t width, height, tiles_x;
};

// h(x) of the header
__host__ __device__ __forceinline__ uint32_t sensor_hash(uint32_t x) {
	x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
	return x;
}

extern "C" __global__ void __launch_bounds__(SSX_SENSOR_LANES) ssx_sensor_kernel(SsxSensorArgs a) {
	const uint32_t p = blockIdx.x * SSX_SENSOR_LANES + threadIdx.x;
	if (p >= a.pixels) return;
	const float4* const q = reinterpret_cast<const float4*>(a.q + (size_t)p * a.B);
	float acc[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll 2
	for (uint32_t b4 = 0; b4 < a.B / 4u; ++b4) {
		const float4 v = q[b4];
		const float* const w = a.W + (size_t)b4 * 16u;
#pragma unroll
		for (int k = 0; k < 3; ++k) acc[k] = acc[k] + v.x * w[k];
#pragma unroll
		for (int k = 0; k < 3; ++k) acc[k] = acc[k] + v.y * w[4 + k];
#pragma unroll
		for (int k = 0; k < 3; ++k) acc[k] = acc[k] + v.z * w[8 + k];
#pragma unroll
		for (int k = 0; k < 3; ++k) acc[k] = acc[k] + v.w * w[12 + k];
	}
	const uint32_t j = p / a.width, i = p - j * a.width;
	const uint32_t c = (a.cfa >> (2u * ((j & 1u) * 2u + (i & 1u)))) & 3u;
	float e = (c == 0u ? acc[0] : (c == 1u ? acc[1] : acc[2])) * a.exposure;
	if (a.noise) { // (uniform)
		const uint32_t hp = sensor_hash(a.base + p);
		uint32_t S = 0u;
#pragma unroll
		for (uint32_t k = 0; k < 6u; ++k) {
			const uint32_t u = sensor_hash(hp + k);
			S += (u & 0xFFFFu) + (u >> 16);
		}
		const float z = ((float)S - 393210.0f) * 1.52587890625e-05f;
		const float sd = sqrtf((e > 0.0f ? e : 0.0f) + a.read_var);
		e = e + sd * z;
	}
	if (a.white > 0.0f) { // (uniform)
		float d = floorf((e * a.dn_per_e + a.black) + 0.5f);
		d = d > 0.0f ? d : 0.0f;
		d = d < a.white ? d : a.white;
		if (a.dn) a.dn[p] = d;
		e = (d - a.black) * a.e_per_dn;
	}
	a.raw[p] = e * a.inv_exposure;
}

// m(k, n) of the header for k in -2 .. n + 1 and beyond: negative where the mirror image lies outside the image (only past a ragged tile's end)
__device__ __forceinline__ int demosaic_mirror(int k, int n) { return k < 0 ? -k : (k >= n ? 2 * (n - 1) - k : k); }

// blockIdx.x = tile_y * tiles_x + tile_x
extern "C" __global__ void __launch_bounds__(SSX_SENSOR_LANES) ssx_demosaic_kernel(SsxDemosaicArgs a) {
	__shared__ __attribute__((aligned(16))) float tile[SSX_DEMOSAIC_SH * SSX_DEMOSAIC_SW];
	const uint32_t t = threadIdx.x;
	const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
	const int W = (int)a.width, H = (int)a.height, x0 = (int)(tx * 2u * SSX_DEMOSAIC_QX), y0 = (int)(ty * 2u * SSX_DEMOSAIC_QY);
	for (uint32_t idx = t; idx < SSX_DEMOSAIC_SH * SSX_DEMOSAIC_SW; idx += SSX_SENSOR_LANES) {
		const uint32_t sy = idx / SSX_DEMOSAIC_SW, sx = idx - sy * SSX_DEMOSAIC_SW;
		const int mx = demosaic_mirror(x0 + (int)sx - 2, W), my = demosaic_mirror(y0 + (int)sy - 2, H);
		tile[idx] = (mx >= 0 && my >= 0) ? a.raw[(size_t)my * a.width + (uint32_t)mx] : 0.0f;
	}
	__syncthreads();
	const uint32_t qx = t & (SSX_DEMOSAIC_QX - 1u), qy = t / SSX_DEMOSAIC_QX;
	float w[6][6];                                            // the quad's window: staged rows 2 qy .. 2 qy + 5, columns 2 qx .. 2 qx + 5
#pragma unroll
	for (int r = 0; r < 6; ++r) {
		const float2* const row = reinterpret_cast<const float2*>(tile + (2u * qy + (uint32_t)r) * SSX_DEMOSAIC_SW + 2u * qx);
#pragma unroll
		for (int k = 0; k < 3; ++k) { const float2 v = row[k]; w[r][2 * k] = v.x; w[r][2 * k + 1] = v.y; }
	}
	const float* const taps = a.table;
	const float* const ccm = a.table + 300;
#pragma unroll
	for (int pj = 0; pj < 2; ++pj)
#pragma unroll
		for (int pi = 0; pi < 2; ++pi) {
			float rgb[3];
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				const float* const k = taps + ((pj * 2 + pi) * 3 + c) * 25;
				float acc = 0.0f;
#pragma unroll
				for (int dy = 0; dy < 5; ++dy)
#pragma unroll
					for (int dx = 0; dx < 5; ++dx) acc = acc + w[pj + dy][pi + dx] * k[dy * 5 + dx];
				rgb[c] = acc;
			}
			const int gx = x0 + 2 * (int)qx + pi, gy = y0 + 2 * (int)qy + pj;
			if (gx < W && gy < H) {
				float* const o = a.out + ((size_t)gy * a.width + (uint32_t)gx) * 3u;
#pragma unroll
				for (int c = 0; c < 3; ++c) o[c] = ((0.0f + rgb[0] * ccm[3 * c]) + rgb[1] * ccm[3 * c + 1]) + rgb[2] * ccm[3 * c + 2];
			}
		}
}

namespace {

// The caller's parameters, checked (the tables still the caller's host pointers)
int sensor_take_params(ssx_ctx* ctx, const char* what, const ssx_sensor_params* in, bool senses, bool demosaics, bool wants_dn) {
	if (!in) return fail(ctx, SSX_ERR_ARG, fmt("%s: sensor must not be NULL", what));
	if (in->struct_size != sizeof(ssx_sensor_params)) return fail(ctx, SSX_ERR_ARG, "ssx_sensor_params.struct_size mismatch");
	for (int k = 0; k < 4; ++k)
		if (in->cfa[k] > 2u) return fail(ctx, SSX_ERR_ARG, fmt("ssx_sensor_params.cfa[%d] = %u: a channel is 0..2", k, in->cfa[k]));
	const struct { const char* name; float v; bool non_negative; } fields[] = {
		{ "exposure", in->exposure, true }, { "inv_exposure", in->inv_exposure, false }, { "read_var", in->read_var, true }, { "dn_per_e", in->dn_per_e, false },
		{ "e_per_dn", in->e_per_dn, false }, { "black", in->black, false }, { "white", in->white, true } };
	for (const auto& f : fields) {
		if (!std::isfinite(f.v)) return fail(ctx, SSX_ERR_ARG, fmt("ssx_sensor_params.%s = %g: must be finite", f.name, (double)f.v));
		if (f.non_negative && f.v < 0.0f) return fail(ctx, SSX_ERR_ARG, fmt("ssx_sensor_params.%s = %g: must not be negative", f.name, (double)f.v));
	}
	if (in->white > 0.0f && in->black > in->white) return fail(ctx, SSX_ERR_ARG, fmt("ssx_sensor_params.black = %g lies above white = %g", (double)in->black, (double)in->white));
	if (wants_dn && !(in->white > 0.0f)) return fail(ctx, SSX_ERR_ARG, fmt("%s: dn needs an ADC (ssx_sensor_params.white > 0)", what));
	if (senses && !in->weights) return fail(ctx, SSX_ERR_ARG, "ssx_sensor_params: weights must not be NULL");
	if (demosaics) {
		if (!in->taps) return fail(ctx, SSX_ERR_ARG, "ssx_sensor_params: taps must not be NULL");
		if (!in->ccm) return fail(ctx, SSX_ERR_ARG, "ssx_sensor_params: ccm must not be NULL");
		for (int k = 0; k < 300; ++k)
			if (!std::isfinite(in->taps[k])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_sensor_params.taps[%d][%d][%d] = %g: must be finite", k / 75, k / 25 % 3, k % 25, (double)in->taps[k]));
		for (int k = 0; k < 9; ++k)
			if (!std::isfinite(in->ccm[k])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_sensor_params.ccm[%d][%d] = %g: must be finite", k / 3, k % 3, (double)in->ccm[k]));
	}
	return SSX_OK;
}

int sensor_check_size(ssx_ctx* ctx, uint32_t width, uint32_t height, const char* what) {
	if (width < 3u || height < 3u) return fail(ctx, SSX_ERR_ARG, fmt("%s: width = %u, height = %u: the mirrored border needs at least 3 x 3", what, width, height));
	return denoise_check_size(ctx, width, height, what);
}

// d_sensor: W_dev [64][4] | table [312] | raw | dn [pixels] | out [pixels][3] | the pure SENSOR's q [q_floats]; the caller's tables go up here (blocking)
struct SensorBuffers { float* W; float* table; float* raw; float* dn; float* out; float* q; };
int sensor_buffers(ssx_ctx* ctx, size_t pixels, uint32_t B, const ssx_sensor_params& s, bool senses, bool demosaics, size_t q_floats, SensorBuffers* d) {
	if (const int rc = carve(ctx, ctx->d_sensor, [&](Carver& c) {
		d->W = reinterpret_cast<float*>(c.take<float4>(64u));
		d->table = reinterpret_cast<float*>(c.take<float4>(SSX_DEMOSAIC_TABLE / 4u));
		d->raw = reinterpret_cast<float*>(c.take<float4>((pixels + 3u) / 4u));
		d->dn = c.take<float>(pixels);
		d->out = c.take<float>(pixels * 3u);
		d->q = reinterpret_cast<float*>(c.take<float4>(q_floats / 4u));
	})) return rc;
	if (senses) {
		std::vector<float> w((size_t)B * 4u, 0.0f);
		for (uint32_t c = 0; c < 3u; ++c) for (uint32_t b = 0; b < B; ++b) w[(size_t)b * 4u + c] = s.weights[(size_t)c * B + b];
		SSX_HIP(ctx, hipMemcpy(d->W, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
	}
	if (demosaics) {
		float table[SSX_DEMOSAIC_TABLE] = {};
		std::memcpy(table, s.taps, 300u * sizeof(float));
		std::memcpy(table + 300, s.ccm, 9u * sizeof(float));
		SSX_HIP(ctx, hipMemcpy(d->table, table, sizeof table, hipMemcpyHostToDevice));
	}
	return SSX_OK;
}

// SENSOR on `src` (only read), queued on the context's stream: d.raw, and d.dn with an ADC
int sensor_device(ssx_ctx* ctx, const SensorBuffers& d, const ssx_sensor_params& s, uint32_t width, uint32_t height, uint32_t B, const float* src) {
	SsxSensorArgs a{};
	a.q = src; a.W = d.W; a.raw = d.raw; a.dn = s.white > 0.0f ? d.dn : nullptr;
	a.width = width; a.pixels = width * height; a.B = B;
	a.cfa = s.cfa[0] | s.cfa[1] << 2 | s.cfa[2] << 4 | s.cfa[3] << 6;
	a.noise = s.noise; a.base = sensor_hash(sensor_hash(s.seed) + s.frame);
	a.exposure = s.exposure; a.inv_exposure = s.inv_exposure; a.read_var = s.read_var;
	a.dn_per_e = s.dn_per_e; a.e_per_dn = s.e_per_dn; a.black = s.black; a.white = s.white;
	hipLaunchKernelGGL(ssx_sensor_kernel, blocks_of(a.pixels), dim3(SSX_SENSOR_LANES), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

// DEMOSAIC on d.raw, queued on the context's stream: d.out
int demosaic_device(ssx_ctx* ctx, const SensorBuffers& d, uint32_t width, uint32_t height) {
	SsxDemosaicArgs a{};
	a.raw = d.raw; a.table = d.table; a.out = d.out;
	a.width = width; a.height = height;
	a.tiles_x = (width + 2u * SSX_DEMOSAIC_QX - 1u) / (2u * SSX_DEMOSAIC_QX);
	const uint32_t tiles_y = (height + 2u * SSX_DEMOSAIC_QY - 1u) / (2u * SSX_DEMOSAIC_QY);
	const size_t blocks = (size_t)a.tiles_x * tiles_y;                                           // < 2^25: at most 2^28 pixels, at least 3 x 16 of them per tile
	hipLaunchKernelGGL(ssx_demosaic_kernel, dim3((uint32_t)blocks), dim3(SSX_SENSOR_LANES), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_sensor_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q, const ssx_sensor_params* sensor, float* raw, float* dn) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_sensor_images";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if (!q || !raw) return fail(ctx, SSX_ERR_ARG, fmt("%s: q and raw must not be NULL", what));
	int rc = sensor_check_size(ctx, width, height, what);
	if (rc) return rc;
	if ((rc = sensor_take_params(ctx, what, sensor, true, false, dn != nullptr))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	SensorBuffers d;
	if ((rc = sensor_buffers(ctx, pixels, bins, *sensor, true, false, pixels * bins, &d))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d.q, q, pixels * bins * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	if ((rc = sensor_device(ctx, d, *sensor, width, height, bins, d.q))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(raw, d.raw, pixels * sizeof(float), hipMemcpyDeviceToHost));
	if (dn) SSX_HIP(ctx, hipMemcpy(dn, d.dn, pixels * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_demosaic_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* raw, const ssx_sensor_params* sensor, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_demosaic_images";
	if (!raw || !out) return fail(ctx, SSX_ERR_ARG, fmt("%s: raw and out must not be NULL", what));
	int rc = sensor_check_size(ctx, width, height, what);
	if (rc) return rc;
	if ((rc = sensor_take_params(ctx, what, sensor, false, true, false))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	SensorBuffers d;
	if ((rc = sensor_buffers(ctx, pixels, 4u, *sensor, false, true, 0, &d))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d.raw, raw, pixels * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	if ((rc = demosaic_device(ctx, d, width, height))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, d.out, pixels * 3u * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

// The front is ssx_spectral_develop_lens's, statement by statement (that entry stays as it is); behind it SENSOR and DEMOSAIC take the develop kernels' place.
int ssx_spectral_develop_sensor(ssx_ctx* ctx, const ssx_denoise_params* denoise, const ssx_defocus_params* defocus, const ssx_optics_params* optics,
                                const ssx_sensor_params* sensor, float* out, float* raw_out, float* dn_out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_develop_sensor";
	int rc = sensor_take_params(ctx, what, sensor, true, true, dn_out != nullptr);
	if (rc) return rc;
	ssx_denoise_params dp;
	if (denoise && (rc = denoise_take_params(ctx, denoise, &dp))) return rc;
	if ((rc = develop_state_ready(ctx, what, denoise != nullptr))) return rc;
	const ssx_render_params& p = ctx->cur;
	if (p.tile_stride != 1u) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context owns one tile in %u (tile_stride): a demosaic needs its neighbours -- gather the bins and use ssx_sensor_images and ssx_demosaic_images", what, p.tile_stride));
	if ((rc = sensor_check_size(ctx, p.width, p.height, what))) return rc;
	const uint32_t B = ctx->spectral_bins;
	DefocusParams f{};
	if (defocus && (rc = defocus_take_params(ctx, what, defocus, B, &f))) return rc;
	const std::vector<float> one(B, 1.0f);
	const std::vector<uint32_t> zero(B, 0u);
	OpticsParams o{ 0.0f, 0.0f, 0u, 0u, one.data(), zero.data(), one.data(), false, false };
	if (optics && (rc = optics_take_params(ctx, what, optics, B, &o))) return rc;
	if (f.active && !ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	const size_t pixels = (size_t)p.width * p.height;
	OpticsBuffers d;
	if ((rc = optics_buffers(ctx, pixels, B, o, &d))) return rc;
	const float* src = nullptr;
	if (denoise) {
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
	if (f.active) {
		if ((rc = ensure_guides(ctx, p.width, p.height))) return rc;
		DefocusBuffers fb;
		if ((rc = defocus_buffers(ctx, pixels, B, f, false, &fb))) return rc;
		if ((rc = defocus_device(ctx, fb, f, p.width, p.height, B, src, guides_of(ctx, pixels).depth))) return rc;
		src = fb.out;
	}
	const float* result = nullptr;
	if ((rc = optics_device(ctx, d, o, p.width, p.height, B, src, &result))) return rc;
	SensorBuffers s;
	if ((rc = sensor_buffers(ctx, pixels, B, *sensor, true, true, 0, &s))) return rc;
	if ((rc = sensor_device(ctx, s, *sensor, p.width, p.height, B, result))) return rc;
	if ((rc = demosaic_device(ctx, s, p.width, p.height))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (out) SSX_HIP(ctx, hipMemcpy(out, s.out, pixels * 3u * sizeof(float), hipMemcpyDeviceToHost));
	if (raw_out) SSX_HIP(ctx, hipMemcpy(raw_out, s.raw, pixels * sizeof(float), hipMemcpyDeviceToHost));
	if (dn_out) SSX_HIP(ctx, hipMemcpy(dn_out, s.dn, pixels * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

} // extern "C"

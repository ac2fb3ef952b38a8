// ssx_delta_e.hip -- the colour difference of two developments (include/ssx.h, "Colour difference of two developments"): per pixel the CIELAB coordinates of two
// XYZ triples under their whites, dE*ab and CIEDE2000 as a two-channel map, and per labelled region and metric SUM, SSQ, MAX, NF, NX, EX reduced in a fixed
// order.  Part of ssx_api.hip's translation unit, behind ssx_develop.hip (develop_state_ready, the develop kernels and their launches), ssx_spectral.hip
// (carve, copy_planes) and ssx_denoise.hip (blocks_of, denoise_check_size, denoise_spectral_device).  The per-pixel part is binary64 with the device library's cbrt,
// atan2, sin, cos, exp and sqrt: its results are held to the numpy restatement (tests/delta_e_ref.py) WITHIN A BOUND, not bit for bit.  The region part is IEEE
// + and * on the map's floats in the order the header writes: a numpy walk over the returned map gives the same bits.

struct SsxDeltaEArgs {
	const float* xyz_a; const float* xyz_b;   // [height][width][3], row-major
	const uint8_t* labels;                    // [height][width], or NULL: every pixel is region 0
	float* de;                                // [height][width][2], or NULL
	float* lab;                               // [height][width][6], or NULL
	uint64_t* part;                           // [height][R][6][2]: SUM, SSQ (binary64), MAX (binary32 in the low word), NF, NX, EX (uint64)
	SsxPixelGrid g;                           // whose pixels: a pixel the grid does not own writes +0 and belongs to no region (tile_stride 1: all owned)
	double rw_a[3], rw_b[3];                  // the whites
	double t[2];                              // the thresholds
	uint32_t R;
};

// f of the header: the cube root above the knee (6/29)^3, the tangent's line below it.  A NaN takes the line and stays a NaN.
__device__ __forceinline__ double delta_e_f(double t) { return t > 216.0 / 24389.0 ? cbrt(t) : t / (108.0 / 841.0) + 4.0 / 29.0; }

struct SsxLab { double L, a, b; };
// delta_e_lab and delta_e_00 are NOT inlined: inlined next to each other, the binary64 constants of the library's cbrt, atan2, sin, cos and exp do not fit the
// wave's 106 scalar registers (11 spilled to VGPR lanes, 167 VGPRs); as two calls the kernel needs 93 SGPRs and 107 VGPRs and spills nothing.  By value in, by
// value out: nothing goes through memory (no scratch), and one copy of the three cube roots serves both sides.
__device__ __noinline__ SsxLab delta_e_lab(float X, float Y, float Z, double w0, double w1, double w2) {
	const double fx = delta_e_f((double)X / w0), fy = delta_e_f((double)Y / w1), fz = delta_e_f((double)Z / w2);
	return SsxLab{ 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz) };
}

#define SSX_DE_RAD 0.017453292519943295   /* pi / 180 */
#define SSX_DE_DEG 57.29577951308232      /* 180 / pi */
#define SSX_DE_25_7 6103515625.0          /* 25^7 */

__device__ __forceinline__ double delta_e_pow7(double c) { const double c2 = c * c, c4 = c2 * c2; return (c4 * c2) * c; }
__device__ __forceinline__ double delta_e_hue(double b, double ap) {
	if (ap == 0.0 && b == 0.0) return 0.0;
	const double h = atan2(b, ap) * SSX_DE_DEG;
	return h < 0.0 ? h + 360.0 : h;
}

// CIEDE2000 of the header, kL = kC = kH = 1, statement by statement (not inlined: see delta_e_lab)
__device__ __noinline__ double delta_e_00(double L1, double a1, double b1, double L2, double a2, double b2) {
	const double C1 = sqrt(a1 * a1 + b1 * b1), C2 = sqrt(a2 * a2 + b2 * b2);
	const double Cm7 = delta_e_pow7(0.5 * (C1 + C2));
	const double G = 0.5 * (1.0 - sqrt(Cm7 / (Cm7 + SSX_DE_25_7)));
	const double ap1 = (1.0 + G) * a1, ap2 = (1.0 + G) * a2;
	const double Cp1 = sqrt(ap1 * ap1 + b1 * b1), Cp2 = sqrt(ap2 * ap2 + b2 * b2);
	const double h1 = delta_e_hue(b1, ap1), h2 = delta_e_hue(b2, ap2);
	const double dL = L2 - L1, dC = Cp2 - Cp1, CC = Cp1 * Cp2, dh0 = h2 - h1, hs = h1 + h2;
	const bool grey = CC == 0.0, far = fabs(h1 - h2) > 180.0;
	const double dh = grey ? 0.0 : !far ? dh0 : dh0 > 180.0 ? dh0 - 360.0 : dh0 + 360.0;
	const double dH = (2.0 * sqrt(CC)) * sin((0.5 * dh) * SSX_DE_RAD);
	const double Lm = 0.5 * (L1 + L2), Cm = 0.5 * (Cp1 + Cp2);
	const double hm = grey ? hs : !far ? 0.5 * hs : hs < 360.0 ? 0.5 * (hs + 360.0) : 0.5 * (hs - 360.0);
	const double T = (((1.0 - 0.17 * cos((hm - 30.0) * SSX_DE_RAD)) + 0.24 * cos((2.0 * hm) * SSX_DE_RAD)) + 0.32 * cos((3.0 * hm + 6.0) * SSX_DE_RAD)) - 0.20 * cos((4.0 * hm - 63.0) * SSX_DE_RAD);
	const double u = (hm - 275.0) / 25.0, dtheta = 30.0 * exp(-(u * u));
	const double Cp7 = delta_e_pow7(Cm), RC = 2.0 * sqrt(Cp7 / (Cp7 + SSX_DE_25_7));
	const double l50 = (Lm - 50.0) * (Lm - 50.0);
	const double SL = 1.0 + (0.015 * l50) / sqrt(20.0 + l50), SC = 1.0 + 0.045 * Cm, SH = 1.0 + (0.015 * Cm) * T;
	const double RT = -sin((2.0 * dtheta) * SSX_DE_RAD) * RC;
	const double tl = dL / SL, tc = dC / SC, th = dH / SH;
	return sqrt(((tl * tl + tc * tc) + th * th) + (RT * tc) * th);
}

// Stage 1, the structure of ssx_compare_rows_kernel: one 256-lane workgroup per image row takes the row in chunks of SSX_DE_CHUNK = 256 pixels, one lane per
// pixel -- the per-pixel part is some hundreds of binary64 operations (six cube roots, two arc tangents, a dozen roots, seven sines and cosines, an
// exponential) at a quarter of the binary32 rate or less, so a lane has one pixel's worth of registers live and a chunk is as wide as the workgroup; the
// walk's 12 lanes then cost 256 dependent LDS reads per chunk, which the other workgroups of the CU hide.
//   pixel: lane t reads its two triples (24 bytes: the wave reads 768 consecutive bytes of each array), writes de as one float2 and lab as six floats, and
//         stages its two floats and its label.  A pixel of another context (state entry with an owner mask) writes +0 and stages label 255.
//   LDS:  v as two rows of floats, ROW STRIDE 257; the labels as 256 bytes.  The LDS of gfx950 has 64 banks of 4 bytes; a ds_write_b32 and a ds_read_b32 are
//         served per group of 32 lanes and take the bank as (byte address / 4) mod 32, the wider reads as mod 64.  On the way in lane t writes row k at word k *
//         257 + t: the 32 lanes of a group cover 32 consecutive words, 32 distinct banks.  On the way out lane t = q * 2 + k (q: the quantity, k: the metric)
//         reads word k * 257 + i at pixel step i: the 12 lanes, all in one group, ask for two distinct addresses, words i and i + 257 -- banks i and i + 1
//         under either modulus (257 mod 32 = 257 mod 64 = 1), each address a broadcast.  THE PAD OF ONE WORD is the whole argument: a stride of 256 (0 mod 32
//         and mod 64) would put both addresses on one bank and make every step of the serial walk a two-way conflict.  The label is one byte for the
//         whole workgroup.
//   walk: as in the compare kernel the accumulators of the 12 lanes live in LDS, [R][12] eight-byte words (lane t of region r at word r * 12 + t: consecutive
//         lanes, consecutive bank pairs), and the lane keeps those of the CURRENT region in a register, going to LDS where the label changes.  Ascending i from
//         +0.0 / 0, the accumulators carried from chunk to chunk; no atomics.
#define SSX_DE_CHUNK 256u
#define SSX_DE_STRIDE 257u
#define SSX_DE_QUANTITIES 6u
#define SSX_DE_NO_REGION 255u
extern "C" __global__ void __launch_bounds__(256) ssx_delta_e_rows_kernel(SsxDeltaEArgs a) {
	__shared__ float stage[2u * SSX_DE_STRIDE];
	__shared__ uint64_t acc[32u * 12u];
	__shared__ uint8_t lab[SSX_DE_CHUNK];
	const uint32_t t = threadIdx.x, j = blockIdx.x, R = a.R, width = a.g.width;
	for (uint32_t e = t; e < R * 12u; e += 256u) acc[e] = 0ull;                          // +0.0, +0.0f and 0 are all-zero words
	const uint32_t q = t >> 1, k = t & 1u;                                               // the walk's lanes: t < 12
	const float* const mine = stage + k * SSX_DE_STRIDE;
	const double tk = a.t[k];
	uint32_t cur = SSX_DE_NO_REGION;
	uint64_t au = 0ull;
	const size_t row = (size_t)j * width;
	__syncthreads();
	for (uint32_t i0 = 0; i0 < width; i0 += SSX_DE_CHUNK) {
		const uint32_t n_px = min(SSX_DE_CHUNK, width - i0);
		if (t < n_px) {
			const size_t p = row + i0 + t;
			float v_ab = 0.0f, v_00 = 0.0f, l6[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
			uint32_t r = SSX_DE_NO_REGION;
			if (ssx_owns_pixel(a.g, i0 + t, j)) {
				const float* const xa = a.xyz_a + p * 3u;
				const float* const xb = a.xyz_b + p * 3u;
				const SsxLab A = delta_e_lab(xa[0], xa[1], xa[2], a.rw_a[0], a.rw_a[1], a.rw_a[2]), B = delta_e_lab(xb[0], xb[1], xb[2], a.rw_b[0], a.rw_b[1], a.rw_b[2]);
				const double L1 = A.L, a1 = A.a, b1 = A.b, L2 = B.L, a2 = B.a, b2 = B.b;
				const double dL = L1 - L2, da = a1 - a2, db = b1 - b2;
				v_ab = (float)sqrt((dL * dL + da * da) + db * db);
				v_00 = (float)delta_e_00(L1, a1, b1, L2, a2, b2);
				l6[0] = (float)L1; l6[1] = (float)a1; l6[2] = (float)b1; l6[3] = (float)L2; l6[4] = (float)a2; l6[5] = (float)b2;
				r = a.labels ? a.labels[p] : 0u;
			}
			stage[t] = v_ab; stage[SSX_DE_STRIDE + t] = v_00;
			lab[t] = (uint8_t)r;
			if (a.de) *reinterpret_cast<float2*>(a.de + p * 2u) = make_float2(v_ab, v_00);
			if (a.lab) {
				float2* const o = reinterpret_cast<float2*>(a.lab + p * 6u);
				o[0] = make_float2(l6[0], l6[1]); o[1] = make_float2(l6[2], l6[3]); o[2] = make_float2(l6[4], l6[5]);
			}
		}
		__syncthreads();
		if (t < 12u) {
			for (uint32_t i = 0; i < n_px; ++i) {
				const uint32_t r = lab[i];
				if (r >= R) continue;                                                        // 255: no region (other values never get here: the host refuses them)
				if (r != cur) {
					if (cur != SSX_DE_NO_REGION) acc[cur * 12u + t] = au;
					cur = r; au = acc[r * 12u + t];
				}
				const float v = mine[i];
				const bool finite = fabsf(v) <= 3.4028234663852886e38f;                      // false for a NaN
				const double x = (double)v;
				switch (q) {
				case 0u: if (finite) au = (uint64_t)__double_as_longlong(__longlong_as_double((long long)au) + x); break;              // SUM
				case 1u: if (finite) au = (uint64_t)__double_as_longlong(__longlong_as_double((long long)au) + x * x); break;          // SSQ: the product is exact
				case 2u: if (finite && v > __uint_as_float((uint32_t)au)) au = (uint64_t)__float_as_uint(v); break;                      // MAX
				case 3u: au += finite ? 1ull : 0ull; break;                                                                              // NF
				case 4u: au += finite ? 0ull : 1ull; break;                                                                              // NX
				default: au += x > tk ? 1ull : 0ull; break;                                                                              // EX: strict, a NaN does not count
				}
			}
		}
		__syncthreads();                                                                     // (the next chunk overwrites what the walk reads)
	}
	if (t < 12u && cur != SSX_DE_NO_REGION) acc[cur * 12u + t] = au;
	__syncthreads();
	for (uint32_t e = t; e < R * 12u; e += 256u) a.part[(size_t)j * R * 12u + e] = acc[e];   // [j][r][q][k]
}

// Stage 2: part [rows][R][6][2] -> out [6][R][2], one lane per (quantity, r, k) takes the rows' partials in ascending row order from +0.0 / 0.  A sibling of
// ssx_ordered_reduce_kernel (ssx_spectral.hip), which adds every quantity: MAX (quantity 2) takes the larger instead.
extern "C" __global__ void __launch_bounds__(256) ssx_delta_e_reduce_kernel(const uint64_t* part, uint64_t* out, uint32_t rows, uint32_t R) {
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= SSX_DE_QUANTITIES * R * 2u) return;
	const uint32_t quantity = e / (R * 2u), rk = e - quantity * (R * 2u), r = rk >> 1, k = rk & 1u;
	const uint64_t* const src = part + ((size_t)r * SSX_DE_QUANTITIES + quantity) * 2u + k;
	const size_t stride = (size_t)R * SSX_DE_QUANTITIES * 2u;
	if (quantity < 2u) {
		double total = 0.0;
#pragma unroll 16
		for (uint32_t j = 0; j < rows; ++j) total += reinterpret_cast<const double*>(src)[j * stride];
		reinterpret_cast<double*>(out)[e] = total;
	} else if (quantity == 2u) {
		float most = 0.0f;
#pragma unroll 16
		for (uint32_t j = 0; j < rows; ++j) most = fmaxf(most, __uint_as_float((uint32_t)src[j * stride]));   // the partials are finite and >= +0
		out[e] = (uint64_t)__float_as_uint(most);
	} else {
		uint64_t total = 0ull;
#pragma unroll 16
		for (uint32_t j = 0; j < rows; ++j) total += src[j * stride];
		out[e] = total;
	}
}

namespace {

// d_probe (a temporary of one call, shared with the probes and the comparison): xyz of A and B [pixels][3], de [pixels][2], lab [pixels][6], part
// [height][R][6][2], out [6][R][2], the two sides' develop weights (4 KB each, the develop kernels' W_dev), labels [pixels]
struct DeltaEBuffers { float* xyz[2]; float* de; float* lab; uint64_t* part; uint64_t* out; float* W[2]; uint8_t* labels; };
int delta_e_buffers(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t R, DeltaEBuffers* d) {
	const size_t pixels = (size_t)width * height;
	return carve(ctx, ctx->d_probe, [&](Carver& c) {
		d->part = c.take<uint64_t>((size_t)height * R * 12u);
		d->out = c.take<uint64_t>((size_t)12u * R);
		for (int x = 0; x < 2; ++x) d->W[x] = reinterpret_cast<float*>(c.take<float4>(kDevelopWeightBytes / sizeof(float4)));
		d->de = reinterpret_cast<float*>(c.take<float2>(pixels));                          // (the kernel stores de and lab as float2)
		d->lab = reinterpret_cast<float*>(c.take<float2>(pixels * 3u));
		for (int x = 0; x < 2; ++x) d->xyz[x] = c.take<float>(pixels * 3u);
		d->labels = c.take<uint8_t>(pixels);
	});
}

bool delta_e_positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

int delta_e_check(ssx_ctx* ctx, const char* what, uint32_t width, uint32_t height, const double* white_a, const double* white_b, const uint8_t* labels, uint32_t R, const double* t,
                  const void* SUM, const void* SSQ, const void* MAX, const void* NF, const void* NX, const void* EX) {
	if (!white_a || !white_b) return fail(ctx, SSX_ERR_ARG, fmt("%s: white_a and white_b must not be NULL", what));
	if (!t) return fail(ctx, SSX_ERR_ARG, fmt("%s: t must not be NULL", what));
	if (!SUM || !SSQ || !MAX || !NF || !NX || !EX) return fail(ctx, SSX_ERR_ARG, fmt("%s: the six outputs SUM, SSQ, MAX, NF, NX, EX must not be NULL", what));
	for (int c = 0; c < 3; ++c) {
		if (!delta_e_positive_finite(white_a[c])) return fail(ctx, SSX_ERR_ARG, fmt("%s: white_a[%d] = %g: a white's components must be finite and > 0", what, c, white_a[c]));
		if (!delta_e_positive_finite(white_b[c])) return fail(ctx, SSX_ERR_ARG, fmt("%s: white_b[%d] = %g: a white's components must be finite and > 0", what, c, white_b[c]));
	}
	for (int k = 0; k < 2; ++k)
		if (!(t[k] >= 0.0) || t[k] > 1.7976931348623157e308) return fail(ctx, SSX_ERR_ARG, fmt("%s: t[%d] = %g: a threshold must be finite and >= 0", what, k, t[k]));
	if (R < 1u || R > 32u) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u regions: need 1..32", what, R));
	if (!labels) {
		if (R != 1u) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u regions with labels NULL: the whole image is region 0, regions must be 1", what, R));
		return SSX_OK;
	}
	const size_t pixels = (size_t)width * height;
	for (size_t p = 0; p < pixels; ++p)
		if (labels[p] != 255u && labels[p] >= R)
			return fail(ctx, SSX_ERR_ARG, fmt("%s: labels[%zu][%zu] = %u: need a region 0..%u, or 255 for none", what, p / width, p % width, (unsigned)labels[p], R - 1u));
	return SSX_OK;
}

// The one body of both entry points: the two XYZ images are in d already; the labels go up, the two kernels run, the six [R][2] arrays and the maps come back.
int delta_e_device(ssx_ctx* ctx, const DeltaEBuffers& d, const SsxPixelGrid& g, const double* white_a, const double* white_b, const uint8_t* labels, uint32_t R, const double* t,
                   float* de, float* lab, double* SUM, double* SSQ, float* MAX, uint64_t* NF, uint64_t* NX, uint64_t* EX) {
	const size_t pixels = (size_t)g.width * g.height;
	if (labels) SSX_HIP(ctx, hipMemcpyAsync(d.labels, labels, pixels, hipMemcpyHostToDevice, ctx->stream));
	SsxDeltaEArgs a{};
	a.xyz_a = d.xyz[0]; a.xyz_b = d.xyz[1]; a.labels = labels ? d.labels : nullptr; a.de = de ? d.de : nullptr; a.lab = lab ? d.lab : nullptr; a.part = d.part;
	a.g = g; a.R = R;
	for (int c = 0; c < 3; ++c) { a.rw_a[c] = white_a[c]; a.rw_b[c] = white_b[c]; }
	for (int k = 0; k < 2; ++k) a.t[k] = t[k];
	hipLaunchKernelGGL(ssx_delta_e_rows_kernel, dim3(g.height), dim3(256), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	hipLaunchKernelGGL(ssx_delta_e_reduce_kernel, blocks_of((size_t)12u * R), dim3(256), 0, ctx->stream, d.part, d.out, g.height, R);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<uint64_t> most((size_t)R * 2u);
	if (const int rc = copy_planes(ctx, d.out, (size_t)R * 2u, { SUM, SSQ, most.data(), NF, NX, EX })) return rc;
	for (size_t e = 0; e < most.size(); ++e) { const uint32_t w = (uint32_t)most[e]; memcpy(&MAX[e], &w, sizeof w); }
	if (de) SSX_HIP(ctx, hipMemcpy(de, d.de, pixels * 2u * sizeof(float), hipMemcpyDeviceToHost));
	if (lab) SSX_HIP(ctx, hipMemcpy(lab, d.lab, pixels * 6u * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

// the caller's [3][B] weights as the develop kernels' W_dev[b][4], the fourth channel zero
int delta_e_weights(ssx_ctx* ctx, float* W_dev, uint32_t B, const float* weights) {
	std::vector<float> w((size_t)B * 4u, 0.0f);
	for (uint32_t c = 0; c < 3u; ++c) for (uint32_t b = 0; b < B; ++b) w[(size_t)b * 4u + c] = weights[(size_t)c * B + b];
	SSX_HIP(ctx, hipMemcpy(W_dev, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice)); // (blocking: `w` goes out of scope)
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_delta_e_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* xyz_a, const float* xyz_b, const double* white_a, const double* white_b,
                       const uint8_t* labels, uint32_t regions, const double* t, float* de, float* lab,
                       double* SUM, double* SSQ, float* MAX, uint64_t* NF, uint64_t* NX, uint64_t* EX) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_delta_e_images";
	if (!xyz_a || !xyz_b) return fail(ctx, SSX_ERR_ARG, fmt("%s: xyz_a and xyz_b must not be NULL", what));
	int rc = denoise_check_size(ctx, width, height, what);
	if (rc) return rc;
	if ((rc = delta_e_check(ctx, what, width, height, white_a, white_b, labels, regions, t, SUM, SSQ, MAX, NF, NX, EX))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	DeltaEBuffers d;
	if ((rc = delta_e_buffers(ctx, width, height, regions, &d))) return rc;
	const size_t bytes = (size_t)width * height * 3u * sizeof(float);
	SSX_HIP(ctx, hipMemcpyAsync(d.xyz[0], xyz_a, bytes, hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.xyz[1], xyz_b, bytes, hipMemcpyHostToDevice, ctx->stream));
	const SsxPixelGrid whole{ width, height, tiles_across(width), 0u, 1u, 0u };
	return delta_e_device(ctx, d, whole, white_a, white_b, labels, regions, t, de, lab, SUM, SSQ, MAX, NF, NX, EX);
}

int ssx_spectral_delta_e(ssx_ctx* ctx, const ssx_denoise_params* denoise, int denoised_a, int denoised_b, const float* weights_a, const float* weights_b,
                         const double* white_a, const double* white_b, const uint8_t* labels, uint32_t regions, const double* t, float* de, float* lab,
                         double* SUM, double* SSQ, float* MAX, uint64_t* NF, uint64_t* NX, uint64_t* EX) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_delta_e";
	if (!weights_a || !weights_b) return fail(ctx, SSX_ERR_ARG, fmt("%s: weights_a and weights_b must not be NULL", what));
	if ((denoised_a || denoised_b) && !denoise) return fail(ctx, SSX_ERR_ARG, fmt("%s: denoised_%s != 0 needs the filter's parameters: denoise must not be NULL", what, denoised_a ? "a" : "b"));
	const bool filtered = denoised_a || denoised_b;
	ssx_denoise_params dp;
	int rc = SSX_OK;
	if (filtered && (rc = denoise_take_params(ctx, denoise, &dp))) return rc;
	if ((rc = develop_state_ready(ctx, what, filtered))) return rc;
	const ssx_render_params& p = ctx->cur;
	if ((rc = delta_e_check(ctx, what, p.width, p.height, white_a, white_b, labels, regions, t, SUM, SSQ, MAX, NF, NX, EX))) return rc;
	const size_t pixels = (size_t)p.width * p.height;
	const uint32_t B = ctx->spectral_bins;
	DeltaEBuffers d;
	if ((rc = delta_e_buffers(ctx, p.width, p.height, regions, &d))) return rc;
	ChannelBuffers cb{};
	if (filtered) {                                                                      // the filter once, whichever sides ask for it: its ratio stays where it lies
		DenoiseBuffers b;
		if ((rc = denoise_spectral_device(ctx, dp, &b, &cb))) return rc;
	}
	for (int x = 0; x < 2; ++x) {                                                        // each side as ssx_spectral_develop develops it, into the call's staging
		if ((rc = delta_e_weights(ctx, d.W[x], B, x ? weights_b : weights_a))) return rc;
		SsxDevelopArgs a{};
		a.W = d.W[x]; a.out = d.xyz[x];
		a.B = B; a.C = 3u; a.pixels = (uint32_t)pixels;
		if (x ? denoised_b : denoised_a) {
			a.q = cb.stage;
			if ((rc = launch_develop_images(ctx, a))) return rc;
		} else {
			a.S = ctx->d_spectral_sums.as<const double>();
			a.g = pixel_grid(&p);
			a.M = (double)(B / 4u); a.n = (double)ctx->done_spp.load();
			if (p.tile_stride != 1u) SSX_HIP(ctx, hipMemsetAsync(d.xyz[x], 0, pixels * 3u * sizeof(float), ctx->stream));
			if ((rc = launch_develop_state(ctx, a, owned_tiles(p)))) return rc;
		}
	}
	return delta_e_device(ctx, d, pixel_grid(&p), white_a, white_b, labels, regions, t, de, lab, SUM, SSQ, MAX, NF, NX, EX);
}

} // extern "C"

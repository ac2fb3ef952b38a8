// ssx_spectral_compare.hip -- two spectral renders compared pixel by pixel and bin by bin: the difference of the bin means with its variance as two maps, and
// per labelled region and bin the pooled signed difference, its variance, a chi-square sum and the numbers of comparable, not-comparable and exceeding cells,
// reduced in a fixed order (include/ssx.h, "Comparing two spectral renders").  Part of ssx_api.hip's translation unit, behind ssx_spectral_stats.hip
// (moments_ready, moment_deviations, probe_check, the export and variance kernels that make the context's own A) and ssx_denoise.hip (blocks_of,
// denoise_check_size).  Everything here is binary64 with IEEE + - * /, no contraction (the build's -ffp-contract=off), in the order the header writes: a
// restatement in numpy gives the same bits (tests/spectral_compare_ref.py).

struct SsxCompareArgs {
	const double* SA; const double* QA; const uint32_t* NA;   // [height][width][B], [height][width][B], [height][width][M], row-major
	const double* SB; const double* QB; const uint32_t* NB;
	const uint8_t* labels;                                    // [height][width]
	float* diff; float* var;                                  // [height][width][B]; either may be NULL
	uint64_t* part;                                           // [height][R][6][B]: DD, VV, X2 (binary64), CC, NC, EX (uint64)
	uint64_t* out;                                            // [6][R][B]
	double t2;
	uint32_t width, height, B, R;
};

// Stage 1, FUSED: one 256-lane workgroup per image row does the elementwise part and the ordered walk, a chunk of the row at a time, so that d, v and z2 never
// leave the CU (a separate elementwise pass would write and read three binary64 temporaries of the image's size -- 1.5 times the six inputs again -- to win
// nothing the chunks do not give: the divisions run 256 wide here too).  A chunk is SSX_COMPARE_CELLS = 1024 cells = floor(1024 / B) whole pixels.
//   classify: lane t takes cells t, t + 256, ... of the chunk; a cell is (pixel, bin), the bin fastest, as the arrays lie: the 64 lanes of a wave read 512
//         consecutive bytes of SA, QA, SB and QB and write 256 consecutive bytes of diff and var -- every byte of the four once.  NA and NB are read at [p][b % M], B
//         / 4 words per pixel, four times over the b of one m: from the cache after the first.  The nine divisions of a comparable cell run here.  A cell that is
//         not comparable stages d = v = z2 = +0.0: the walk then adds +0.0, which leaves a partial that started from +0.0 as it is (such a partial is never -0.0,
//         and x + (+0.0) == x for every other x; a NaN stays a NaN), so the walk has no branch on the class.
//   LDS:  d, v, z2 as three rows of binary64, row stride 1024 + B; the class (1 comparable, 2 not) as 1024 bytes; the chunk's labels as up to 256 bytes.  On the
//         way in lane t writes 8-byte address row + t (+ 256 u): 16 consecutive lanes of a ds_write_b64 group cover 32 consecutive banks.  On the way out lane
//         t = k * B + b (k = 0 DD | CC, 1 VV | NC, 2 X2 | EX) reads 8-byte address k * (1024 + B) + i * B + b at pixel step i: a ds_read_b64 is served in two
//         groups of 32 lanes over 64 four-byte banks, bank pair = address mod 32, and since 1024 + B == B (mod 32) the address is t + i * B (mod 32) --
//         consecutive lanes, consecutive pairs, 32 distinct ones per group whatever B is: the PAD OF B WORDS is the whole argument; the unpadded 1024 would put
//         the lanes (k, b) of a group with 3 B <= 32 three deep on one pair.  The class is read as a byte at i * B + b, the same for the three k (one address: a
//         broadcast), consecutive b in consecutive bytes.  The label is one byte for the whole workgroup.
//   walk: the label is a run-time index, so the accumulators of the 3 B walking lanes live in LDS, [R][3 B] binary64 and [R][3 B] uint32 (a row holds fewer
//         than 2^32 pixels), lane t of region r at word r * 3 B + t: consecutive lanes, consecutive words, conflict-free at either width.  The lane keeps the
//         accumulators of the CURRENT region in registers and goes to LDS only where the label changes (labels come in runs: a rectangle costs two exchanges per
//         row); the additions and their order are the same.  Ascending i from +0.0 / 0; no atomics.
// LDS per workgroup: 27,392 bytes of staging + 36 CAP bytes of accumulators, CAP >= R * B: two instances, CAP = 256 (36 KB: four workgroups per CU) and CAP = 2048
// (R = 32 at B = 64; 99 KB, static: one workgroup per CU).
#define SSX_COMPARE_CELLS 1024u
#define SSX_COMPARE_NO_REGION 255u
template <uint32_t CAP>
__device__ __forceinline__ void compare_rows(const SsxCompareArgs& a) {
	__shared__ double stage[3u * (SSX_COMPARE_CELLS + 64u)];
	__shared__ double acc_d[3u * CAP];
	__shared__ uint32_t acc_n[3u * CAP];
	__shared__ uint8_t cls[SSX_COMPARE_CELLS];
	__shared__ uint8_t lab[256];
	const uint32_t t = threadIdx.x, B = a.B, M = B / 4u, R = a.R, j = blockIdx.x, lanes = 3u * B, stride = SSX_COMPARE_CELLS + B;
	const uint32_t chunk_px = SSX_COMPARE_CELLS / B;                                     // whole pixels per chunk: 16 (B = 64) .. 256 (B = 4)
	for (uint32_t e = t; e < R * lanes; e += 256u) { acc_d[e] = 0.0; acc_n[e] = 0u; }
	const uint32_t k = t / B, b = t - k * B;                                             // the walk's lanes: t < 3 B
	const double* const mine = stage + k * stride + b;
	uint32_t cur = SSX_COMPARE_NO_REGION, an = 0u;
	double ad = 0.0;
	const size_t row = (size_t)j * a.width;
	__syncthreads();
	for (uint32_t i0 = 0; i0 < a.width; i0 += chunk_px) {
		const uint32_t n_px = min(chunk_px, a.width - i0), n_cells = n_px * B;
		if (t < n_px) lab[t] = a.labels[row + i0 + t];
		const size_t g0 = (row + i0) * B;
		for (uint32_t e = t; e < n_cells; e += 256u) {
			const uint32_t pi = e / B, eb = e - pi * B;
			const size_t g = g0 + e, at_n = (row + i0 + pi) * M + eb % M;
			const uint32_t nA = a.NA[at_n], nB = a.NB[at_n];
			const double sA = a.SA[g], qA = a.QA[g], sB = a.SB[g], qB = a.QB[g];
			const bool comparable = nA >= 2u && nB >= 2u;
			double d = 0.0, v = 0.0, z2 = 0.0;
			float fd = 0.0f, fv = __uint_as_float(0x7F800000u);
			if (comparable) {
				double muA, muB;
				const double eA = cell_variance(qA, sA, nA, &muA), eB = cell_variance(qB, sB, nB, &muB);
				d = muA - muB;
				v = eA + eB;
				z2 = (v == 0.0 && d == 0.0) ? 0.0 : (d * d) / v;
				fd = (float)d; fv = (float)v;
			}
			stage[e] = d; stage[stride + e] = v; stage[2u * stride + e] = z2;
			cls[e] = comparable ? 1u : 2u;
			if (a.diff) a.diff[g] = fd;
			if (a.var) a.var[g] = fv;
		}
		__syncthreads();
		if (t < lanes) {
			for (uint32_t i = 0; i < n_px; ++i) {
				const uint32_t r = lab[i];
				if (r >= R) continue;                                                        // 255: no region (other values never get here: the host refuses them)
				if (r != cur) {
					if (cur != SSX_COMPARE_NO_REGION) { acc_d[cur * lanes + t] = ad; acc_n[cur * lanes + t] = an; }
					cur = r; ad = acc_d[r * lanes + t]; an = acc_n[r * lanes + t];
				}
				const double x = mine[i * B];
				const uint32_t c = cls[i * B + b];
				ad += x;
				an += (k == 0u) ? (c == 1u ? 1u : 0u) : (k == 1u) ? (c == 2u ? 1u : 0u) : ((c == 1u && x > a.t2) ? 1u : 0u);
			}
		}
		__syncthreads();                                                                     // (the next chunk overwrites what the walk reads)
	}
	if (t < lanes && cur != SSX_COMPARE_NO_REGION) { acc_d[cur * lanes + t] = ad; acc_n[cur * lanes + t] = an; }
	__syncthreads();
	for (uint32_t e = t; e < R * lanes; e += 256u) {
		const uint32_t r = e / lanes, tt = e - r * lanes, kk = tt / B, bb = tt - kk * B;
		uint64_t* const o = a.part + (((size_t)j * R + r) * 6u + kk) * B + bb;
		o[0] = (uint64_t)__double_as_longlong(acc_d[e]);
		o[3u * B] = (uint64_t)acc_n[e];
	}
}

extern "C" __global__ void __launch_bounds__(256) ssx_compare_rows_kernel(SsxCompareArgs a) { compare_rows<256u>(a); }         // R * B <= 256
extern "C" __global__ void __launch_bounds__(256) ssx_compare_rows_wide_kernel(SsxCompareArgs a) { compare_rows<2048u>(a); }  // R * B <= 2048: any legal R and B

// Stage 2 is ssx_ordered_reduce_kernel (ssx_spectral.hip) with 6 quantities, CC, NC and EX (3, 4 and 5) the integers.

namespace {

// d_probe (shared with the probes: both are temporaries of one call): S and Q of A and B [pixels][B] binary64, part [height][R][6][B], out [6][R][B], NA and NB [pixels][M], diff and var [pixels][B] binary32, labels [pixels]
struct CompareBuffers { double* S[2]; double* Q[2]; uint64_t* part; uint64_t* out; uint32_t* N[2]; float* diff; float* var; uint8_t* labels; };
int compare_buffers(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t B, uint32_t R, CompareBuffers* d) {
	const size_t pixels = (size_t)width * height;
	return carve(ctx, ctx->d_probe, [&](Carver& c) {
		for (int x = 0; x < 2; ++x) { d->S[x] = c.take<double>(pixels * B); d->Q[x] = c.take<double>(pixels * B); }
		d->part = c.take<uint64_t>((size_t)height * R * 6u * B);
		d->out = c.take<uint64_t>((size_t)6u * R * B);
		for (int x = 0; x < 2; ++x) d->N[x] = c.take<uint32_t>(pixels * (B / 4u));
		d->diff = c.take<float>(pixels * B);
		d->var = c.take<float>(pixels * B);
		d->labels = c.take<uint8_t>(pixels);
	});
}

int compare_check(ssx_ctx* ctx, const char* what, uint32_t width, uint32_t height, const double* SB, const double* QB, const uint32_t* NB, const uint8_t* labels, uint32_t R, double t2,
                  const void* DD, const void* VV, const void* X2, const void* CC, const void* NC, const void* EX) {
	if (!SB || !QB || !NB) return fail(ctx, SSX_ERR_ARG, fmt("%s: SB, QB and NB must not be NULL", what));
	if (!labels || !DD || !VV || !X2 || !CC || !NC || !EX) return fail(ctx, SSX_ERR_ARG, fmt("%s: labels and the six outputs DD, VV, X2, CC, NC, EX must not be NULL", what));
	if (!(t2 >= 0.0) || t2 > 1.7976931348623157e308) return fail(ctx, SSX_ERR_ARG, fmt("%s: t2 = %g: the squared threshold must be finite and >= 0", what, t2));
	return probe_check(ctx, what, width, height, labels, R, DD, VV, X2, CC);             // regions and labels, with the probe's words
}

// The one body of both entry points: the six arrays are in d already; the labels go up, the two kernels run, the six [R][B] arrays and the maps come back.
int compare_device(ssx_ctx* ctx, const CompareBuffers& d, uint32_t width, uint32_t height, uint32_t B, const uint8_t* labels, uint32_t R, double t2,
                   double* DD, double* VV, double* X2, uint64_t* CC, uint64_t* NC, uint64_t* EX, float* diff, float* var) {
	SSX_HIP(ctx, hipMemcpyAsync(d.labels, labels, (size_t)width * height, hipMemcpyHostToDevice, ctx->stream));
	SsxCompareArgs a{};
	a.SA = d.S[0]; a.QA = d.Q[0]; a.NA = d.N[0]; a.SB = d.S[1]; a.QB = d.Q[1]; a.NB = d.N[1];
	a.labels = d.labels; a.diff = diff ? d.diff : nullptr; a.var = var ? d.var : nullptr; a.part = d.part; a.out = d.out;
	a.t2 = t2; a.width = width; a.height = height; a.B = B; a.R = R;
	if (R * B <= 256u) hipLaunchKernelGGL(ssx_compare_rows_kernel, dim3(height), dim3(256), 0, ctx->stream, a);
	else hipLaunchKernelGGL(ssx_compare_rows_wide_kernel, dim3(height), dim3(256), 0, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	hipLaunchKernelGGL(ssx_ordered_reduce_kernel, blocks_of((size_t)6u * R * B), dim3(256), 0, ctx->stream, d.part, d.out, height, R, B, 6u, 0x38u);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (const int rc = copy_planes(ctx, d.out, (size_t)R * B, { DD, VV, X2, CC, NC, EX })) return rc;
	const size_t b_map = (size_t)width * height * B * sizeof(float);
	if (diff) SSX_HIP(ctx, hipMemcpy(diff, d.diff, b_map, hipMemcpyDeviceToHost));
	if (var) SSX_HIP(ctx, hipMemcpy(var, d.var, b_map, hipMemcpyDeviceToHost));
	return SSX_OK;
}

int compare_upload(ssx_ctx* ctx, const CompareBuffers& d, int x, size_t pixels, uint32_t B, const double* S, const double* Q, const uint32_t* N) {
	SSX_HIP(ctx, hipMemcpyAsync(d.S[x], S, pixels * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.Q[x], Q, pixels * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	SSX_HIP(ctx, hipMemcpyAsync(d.N[x], N, pixels * (B / 4u) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_spectral_compare_arrays(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const double* SA, const double* QA, const uint32_t* NA,
                                const double* SB, const double* QB, const uint32_t* NB, const uint8_t* labels, uint32_t regions, double t2,
                                double* DD, double* VV, double* X2, uint64_t* CC, uint64_t* NC, uint64_t* EX, float* diff, float* var) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_compare_arrays";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if (!SA || !QA || !NA) return fail(ctx, SSX_ERR_ARG, fmt("%s: SA, QA and NA must not be NULL", what));
	int rc = denoise_check_size(ctx, width, height, what);
	if (rc) return rc;
	if ((rc = compare_check(ctx, what, width, height, SB, QB, NB, labels, regions, t2, DD, VV, X2, CC, NC, EX))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	CompareBuffers d;
	if ((rc = compare_buffers(ctx, width, height, bins, regions, &d))) return rc;
	const size_t pixels = (size_t)width * height;
	if ((rc = compare_upload(ctx, d, 0, pixels, bins, SA, QA, NA))) return rc;
	if ((rc = compare_upload(ctx, d, 1, pixels, bins, SB, QB, NB))) return rc;
	return compare_device(ctx, d, width, height, bins, labels, regions, t2, DD, VV, X2, CC, NC, EX, diff, var);
}

int ssx_spectral_compare(ssx_ctx* ctx, const ssx_spectral_info_t* other_info, const double* SB, const double* QB, const uint32_t* NB, const uint8_t* labels, uint32_t regions, double t2,
                         double* DD, double* VV, double* X2, uint64_t* CC, uint64_t* NC, uint64_t* EX, float* diff, float* var) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_compare";
	int rc = moments_ready(ctx, what);
	if (rc) return rc;
	const ssx_render_params& p = ctx->cur;
	const uint32_t B = ctx->spectral_bins;
	if (!other_info) return fail(ctx, SSX_ERR_ARG, fmt("%s: other_info must not be NULL", what));
	const std::string why = spectral_info_mismatch(ctx, what, "the other render", nullptr, other_info);
	if (!why.empty()) return fail(ctx, SSX_ERR_ARG, why);
	if ((rc = compare_check(ctx, what, p.width, p.height, SB, QB, NB, labels, regions, t2, DD, VV, X2, CC, NC, EX))) return rc;
	CompareBuffers d;
	if ((rc = compare_buffers(ctx, p.width, p.height, B, regions, &d))) return rc;
	if ((rc = state_to_rows(ctx, d.S[0], d.N[0], d.Q[0]))) return rc;                        // the context's own render is A
	if ((rc = compare_upload(ctx, d, 1, (size_t)p.width * p.height, B, SB, QB, NB))) return rc;
	return compare_device(ctx, d, p.width, p.height, B, labels, regions, t2, DD, VV, X2, CC, NC, EX, diff, var);
}

} // extern "C"

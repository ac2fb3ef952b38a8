// ssx_glare.hip -- veiling glare and diffraction (include/ssx.h, "Glare: per-bin convolution by FFT"): per wavelength bin a 2-D convolution of
// q [height][width][B] with a (2 R + 1)^2 point spread function, by a padded power-of-two FFT written as its radix-2 butterfly graph.  Part of ssx_api.hip's
// translation unit, behind ssx_defocus.hip (defocus_take_params, defocus_buffers, defocus_device), ssx_optics.hip (the unpack kernel, optics_take_params,
// optics_buffers, optics_device), ssx_develop.hip (develop_check, develop_state_ready, develop_buffers, launch_develop_images), ssx_spectral.hip (carve,
// valid_bins) and ssx_denoise.hip (denoise_check_size, denoise_spectral_device).  Three kernels, no atomics, a lane writes only its own outputs, no library FFT.
// Every product is rounded before its add (the build's -ffp-contract=off): the bits are the header's.
//
// THE SCHEDULE.  The header's graph is decimation in time on y[k] = x[bitrev(k)].  A FORWARD line is loaded in its natural order and node k of the graph is
// kept at address bitrev(k): stage s then pairs addresses D = P >> s apart (a = hi * 2 D + lo, b = a + D with lo < D), the twiddle T[k * step] depends on hi
// alone, and frequency k ends up at address bitrev(k).  Nothing undoes that: the planes in global memory hold the spectrum at [bitrev(ky)][bitrev(kx)], the
// psf's transform goes through the same code so MULTIPLY is pointwise on equal addresses, and an INVERSE line -- whose input is by definition the spectrum in
// bit-reversed order -- reads its addresses as they are, runs the stages in the textbook layout (D = 2^(s - 1), twiddle by lo) and leaves the natural order.
// No lane ever computes a bit reversal, and no load or store is a bit-reversed scatter.  The same butterflies with the same operands in the same roles: the
// same bits.  The twiddles arrive per axis as two stage-packed tables made by the host from the caller's table (copies and sign flips only): entry h + x is
// the twiddle of stage h = 2^(s - 1) for hi = x (forward) or lo = x (inverse, imaginary part negated), so that a stage reads consecutive entries.
//
// THE PASSES, per chunk of bins (a chunk is whole groups of four consecutive bins; the planes of a chunk are X and Kf, [py][px] complex each per bin):
//   rows      PAD (or KERNEL, for the psf) fused with the forward rows.  One workgroup per (row, group of four bins); up to four lines in LDS, so that the
//             clamped reads of q are runs of 16 bytes per pixel, 64 consecutive lanes covering 16 pixels.  Rows that PAD leaves zero are neither made nor stored.
//   columns   forward columns, MULTIPLY, inverse columns without leaving LDS (for the psf: the forward columns alone).  SEVERAL ADJACENT COLUMNS PER WORKGROUP
//             rather than a transposing store in the row kernels: a transpose would have to be undone in front of the inverse rows (a fourth and fifth pass
//             over the planes), and eight float2 columns are already runs of 64 bytes.  Eight columns up to py = 1024, four at 2048, two at 4096, so that lines
//             and both twiddle tables stay below 160 KiB.  The rows the first pass skipped are taken as zero without being read; only rows < height are stored.
//   rows back inverse rows fused with CROP: out[j][i][b] = re * inv for the `on` bins, the copy of the `off` bins of the group folded in.
// SCRATCH: 16 px py bytes per bin of a chunk; a chunk is as many groups of four bins as fit SSX_GLARE_SCRATCH = 256 MiB, at least one: 64 px py bytes, 1 GiB at
// the largest plan, 256 MiB or less wherever px py <= 2^22.  Beside the planes d_glare holds the two packed twiddle tables (16 (px + py) bytes), the psf
// (4 B (2 R + 1)^2 bytes: 67 MB at B = 64, R = 256), out (4 B width height bytes) and, for the pure entry, q (as much again): at 512^2 with 64 bins and R = 256
// that is 256 MiB + 67 MB + 67 MB (+ 67 MB).  Like the other stages' buffers it stays allocated until the context is destroyed.
//
// LDS BANKS, argued from the rule, not counted.  A line is float2[P]; a butterfly reads a and b with ds_read_b64 (groups of 32 lanes, bank = word mod 64, so a
// float2 element e sits on banks 2 (e mod 32), + 1).  Consecutive lanes have consecutive lo.  For D >= 32 a group reads 32 consecutive elements: 64 banks, no
// conflict.  For D < 32 a group's a-addresses are the elements of one aligned run of 64 whose bit log2 D is clear (the b-addresses: set), and e and e + 32 of
// that run would meet on a bank: a two-way conflict in the five closest stages, the power-of-two stride case.  The layout is therefore SWIZZLED: element e
// lives at e ^ 31 where bit 5 of e is set, i.e. every odd run of 32 is stored backwards.  The even half of the group's run keeps bit log2 D clear, the odd half
// has it flipped to set, so the 32 addresses fall on 32 different element banks for every D < 32, and for D >= 32 a run of 32 is still a permutation of
// itself.  The stores (ds_write_b64: 16 contiguous lanes, bank = word mod 32, element mod 16) are conflict-free for D >= 16 and two-way for D < 16, which
// raises a store from 6 to 8 LDS cycles in four stages -- accepted.  The twiddle reads: an inverse stage reads consecutive entries; a forward stage reads one entry per D consecutive lanes, so a group takes max(1, 32 / D) consecutive entries, each a broadcast to its D lanes: distinct banks.  Staging is argued no further than the pitch below.  Lines of one workgroup are
// pitched P + 4 elements apart so that staging (lanes across the lines first) spreads over the banks; with P < 64 a group straddles lines and conflicts are
// not argued: those transforms are tiny.

#define SSX_GLARE_LANES 1024u
#define SSX_GLARE_SCRATCH (256ull << 20)

struct SsxGlareArgs {
	const float* q;           // [height][width][B]
	float* out;               // [height][width][B]
	const float* psf;         // [B][K][K]
	float2* X;                // [bins of the chunk][py][px]
	float2* Kf;               // [bins of the chunk][py][px]
	const float2* twx_f; const float2* twx_i;   // [px] stage-packed, forward and inverse (this file's header)
	const float2* twy_f; const float2* twy_i;   // [py]
	uint64_t on;              // bit b: bin b is on
	uint32_t width, height, B, R, px, py, nx, ny;   // nx = log2 px
	uint32_t b0;              // the chunk's first bin
	uint32_t lines;           // rows kernels: lines per pass of a workgroup (4, 2 or 1); columns kernel: columns per workgroup
	uint32_t psf_pass;        // 1: the rows kernel does KERNEL on psf, the columns kernel the forward columns of Kf alone
	float inv;                // 1 / (px py)
};

__device__ __forceinline__ uint32_t glare_at(uint32_t e) { return e ^ ((e & 32u) ? 31u : 0u); }   // the swizzle of this file's header

// All stages of `nl` lines of P = 2^n elements, `pitch` apart; tw: the stage-packed table in LDS.  Ends behind a barrier.
template <bool FWD> __device__ __forceinline__ void glare_fft(float2* lines, uint32_t pitch, uint32_t nl, uint32_t n, const float2* tw) {
	const uint32_t half = 1u << (n - 1u), total = nl << (n - 1u);
	for (uint32_t s = 1; s <= n; ++s) {
		const uint32_t h = 1u << (s - 1u), ld = FWD ? n - s : s - 1u, D = 1u << ld;
		for (uint32_t u = threadIdx.x; u < total; u += blockDim.x) {
			const uint32_t line = u >> (n - 1u), t = u & (half - 1u);
			const uint32_t lo = t & (D - 1u), hi = t >> ld;
			const uint32_t ea = (hi << (ld + 1u)) + lo;
			const float2 w = tw[h + (FWD ? hi : lo)];
			float2* const L = lines + line * pitch;
			float2* const pa = L + glare_at(ea);
			float2* const pb = L + glare_at(ea + D);
			const float2 a = *pa, b = *pb;
			const float tre = (w.x * b.x) - (w.y * b.y);
			const float tim = (w.x * b.y) + (w.y * b.x);
			*pa = make_float2(a.x + tre, a.y + tim);
			*pb = make_float2(a.x - tre, a.y - tim);
		}
		__syncthreads();
	}
}

extern __shared__ __attribute__((aligned(16))) float2 glare_lds[];

// PAD + forward rows (psf_pass: KERNEL + forward rows).  blockIdx.x: the non-zero row, blockIdx.y: the group of four bins within the chunk.
// LDS: tw [px] | lines [a.lines][px + 4]
extern "C" __global__ void __launch_bounds__(SSX_GLARE_LANES) ssx_glare_rows_kernel(SsxGlareArgs a) {
	const uint32_t P = a.px, n = a.nx, pitch = P + 4u, NL = a.lines, R = a.R;
	float2* const tw = glare_lds;
	float2* const lines = glare_lds + P;
	const uint32_t group_on = (uint32_t)(a.on >> (a.b0 + 4u * blockIdx.y)) & 15u;
	if (!group_on) return;                                                                    // (uniform)
	for (uint32_t t = threadIdx.x; t < P; t += blockDim.x) tw[t] = a.twx_f[t];
	// the row: PAD's rows are 0 .. height + R - 1 and py - R .. py - 1, KERNEL's are 0 .. R and py - R .. py - 1
	const uint32_t r = blockIdx.x, low = a.psf_pass ? R + 1u : a.height + R;
	const uint32_t jj = r < low ? r : a.py - (low + R - r);
	const int jrel = jj < low ? (int)jj : (int)jj - (int)a.py;                                 // j' (PAD), dy (KERNEL)
	const uint32_t K = 2u * R + 1u, lb = NL == 4u ? 2u : NL == 2u ? 1u : 0u;
	for (uint32_t c0 = 0; c0 < 4u; c0 += NL) {
		if (!((group_on >> c0) & ((1u << NL) - 1u))) continue;                                // (uniform)
		for (uint32_t idx = threadIdx.x; idx < (P << lb); idx += blockDim.x) {
			const uint32_t c = idx & (NL - 1u), ii = idx >> lb;
			const uint32_t b = a.b0 + 4u * blockIdx.y + c0 + c;
			float v = 0.0f;
			if ((group_on >> (c0 + c)) & 1u) {
				if (a.psf_pass) {
					const int dx = ii <= R ? (int)ii : (ii >= P - R ? (int)ii - (int)P : 0x7fffffff);
					if (dx != 0x7fffffff) v = a.psf[((size_t)b * K + (uint32_t)(jrel + (int)R)) * K + (uint32_t)(dx + (int)R)];
				} else {
					const int irel = ii < a.width + R ? (int)ii : (int)ii - (int)P;
					if (irel >= -(int)R) {                                                    // (irel < width + R holds on both branches: px >= width + 2 R)
						const uint32_t si = (uint32_t)min(max(irel, 0), (int)a.width - 1), sj = (uint32_t)min(max(jrel, 0), (int)a.height - 1);
						v = a.q[((size_t)sj * a.width + si) * a.B + b];
					}
				}
			}
			lines[c * pitch + glare_at(ii)] = make_float2(v, 0.0f);
		}
		__syncthreads();
		glare_fft<true>(lines, pitch, NL, n, tw);
		for (uint32_t idx = threadIdx.x; idx < (P << lb); idx += blockDim.x) {
			const uint32_t ii = idx & (P - 1u), c = idx >> n;
			if (!((group_on >> (c0 + c)) & 1u)) continue;
			float2* const plane = (a.psf_pass ? a.Kf : a.X) + (size_t)(4u * blockIdx.y + c0 + c) * a.py * P;
			plane[(size_t)jj * P + ii] = lines[c * pitch + glare_at(ii)];
		}
		__syncthreads();
	}
}

// Forward columns, MULTIPLY, inverse columns (psf_pass: the forward columns of Kf).  blockIdx.x: a.lines adjacent columns, blockIdx.y: the bin within the chunk.
// LDS: tw forward [py] | tw inverse [py] | lines [a.lines][py + 4]
extern "C" __global__ void __launch_bounds__(SSX_GLARE_LANES) ssx_glare_columns_kernel(SsxGlareArgs a) {
	const uint32_t P = a.py, n = a.ny, pitch = P + 4u, NC = a.lines, R = a.R;
	if (!((a.on >> (a.b0 + blockIdx.y)) & 1u)) return;                                        // (uniform)
	float2* const twf = glare_lds;
	float2* const twi = glare_lds + P;
	float2* const lines = glare_lds + 2u * P;
	for (uint32_t t = threadIdx.x; t < P; t += blockDim.x) { twf[t] = a.twy_f[t]; twi[t] = a.twy_i[t]; }
	const uint32_t lb = NC == 8u ? 3u : NC == 4u ? 2u : NC == 2u ? 1u : 0u;
	const uint32_t i0 = blockIdx.x * NC;
	const size_t plane_at = (size_t)blockIdx.y * P * a.px;
	float2* const plane = (a.psf_pass ? a.Kf : a.X) + plane_at;
	const uint32_t low = a.psf_pass ? R + 1u : a.height + R;                                   // rows low .. py - R - 1 were never written: zero
	for (uint32_t idx = threadIdx.x; idx < (P << lb); idx += blockDim.x) {
		const uint32_t c = idx & (NC - 1u), jj = idx >> lb;
		const bool made = jj < low || jj + R >= P;
		lines[c * pitch + glare_at(jj)] = made ? plane[(size_t)jj * a.px + i0 + c] : make_float2(0.0f, 0.0f);
	}
	__syncthreads();
	glare_fft<true>(lines, pitch, NC, n, twf);
	uint32_t stored = P;
	if (!a.psf_pass) {
		const float2* const kf = a.Kf + plane_at;
		for (uint32_t idx = threadIdx.x; idx < (P << lb); idx += blockDim.x) {
			const uint32_t c = idx & (NC - 1u), jj = idx >> lb;
			float2* const p = lines + c * pitch + glare_at(jj);
			const float2 w = *p, b = kf[(size_t)jj * a.px + i0 + c];
			*p = make_float2((w.x * b.x) - (w.y * b.y), (w.x * b.y) + (w.y * b.x));
		}
		__syncthreads();
		glare_fft<false>(lines, pitch, NC, n, twi);
		stored = a.height;                                                                      // CROP reads rows < height only
	}
	for (uint32_t idx = threadIdx.x; idx < (stored << lb); idx += blockDim.x) {
		const uint32_t c = idx & (NC - 1u), jj = idx >> lb;
		plane[(size_t)jj * a.px + i0 + c] = lines[c * pitch + glare_at(jj)];
	}
}

// Inverse rows + CROP, and the copy of the group's `off` bins.  blockIdx.x: the image row, blockIdx.y: the group of four bins within the chunk.
// LDS: tw [px] | lines [a.lines][px + 4]
extern "C" __global__ void __launch_bounds__(SSX_GLARE_LANES) ssx_glare_rows_back_kernel(SsxGlareArgs a) {
	const uint32_t P = a.px, n = a.nx, pitch = P + 4u, NL = a.lines;
	float2* const tw = glare_lds;
	float2* const lines = glare_lds + P;
	const uint32_t group_on = (uint32_t)(a.on >> (a.b0 + 4u * blockIdx.y)) & 15u;
	if (group_on) for (uint32_t t = threadIdx.x; t < P; t += blockDim.x) tw[t] = a.twx_i[t];
	const uint32_t j = blockIdx.x, lb = NL == 4u ? 2u : NL == 2u ? 1u : 0u;
	for (uint32_t c0 = 0; c0 < 4u; c0 += NL) {
		const bool any = (group_on >> c0) & ((1u << NL) - 1u);                                 // (uniform)
		if (any) {
			for (uint32_t idx = threadIdx.x; idx < (P << lb); idx += blockDim.x) {
				const uint32_t ii = idx & (P - 1u), c = idx >> n;
				float2 v = make_float2(0.0f, 0.0f);
				if ((group_on >> (c0 + c)) & 1u) v = a.X[((size_t)(4u * blockIdx.y + c0 + c) * a.py + j) * P + ii];
				lines[c * pitch + glare_at(ii)] = v;
			}
			__syncthreads();
			glare_fft<false>(lines, pitch, NL, n, tw);
		}
		for (uint32_t idx = threadIdx.x; idx < (a.width << lb); idx += blockDim.x) {
			const uint32_t c = idx & (NL - 1u), i = idx >> lb;
			const size_t e = ((size_t)j * a.width + i) * a.B + a.b0 + 4u * blockIdx.y + c0 + c;
			a.out[e] = ((group_on >> (c0 + c)) & 1u) ? lines[c * pitch + glare_at(i)].x * a.inv : a.q[e];
		}
		__syncthreads();
	}
}

namespace {

uint32_t glare_extent(uint32_t n, uint32_t R) { // the smallest power of two >= max(2, n + 2 R)
	uint32_t p = 2u;
	while (p < n + 2u * R) p <<= 1;
	return p;
}

// The caller's parameters, checked (the tables still the caller's host pointers); active: some bin is on
struct GlareParams { uint32_t R, px, py; uint64_t on; const float* psf; const float* twx; const float* twy; bool active; };

int glare_take_params(ssx_ctx* ctx, const char* what, const ssx_glare_params* in, uint32_t width, uint32_t height, uint32_t B, GlareParams* g) {
	if (!in) return fail(ctx, SSX_ERR_ARG, fmt("%s: glare must not be NULL", what));
	if (in->struct_size != sizeof(ssx_glare_params)) return fail(ctx, SSX_ERR_ARG, "ssx_glare_params.struct_size mismatch");
	if (in->radius > SSX_GLARE_MAX_RADIUS) return fail(ctx, SSX_ERR_ARG, fmt("ssx_glare_params.radius = %u: need 0..%u", in->radius, SSX_GLARE_MAX_RADIUS));
	if (!in->on || !in->psf || !in->twiddle_x || !in->twiddle_y) return fail(ctx, SSX_ERR_ARG, "ssx_glare_params: on, psf, twiddle_x and twiddle_y must not be NULL");
	if (width > SSX_GLARE_MAX_EXTENT || height > SSX_GLARE_MAX_EXTENT) return fail(ctx, SSX_ERR_ARG, fmt("%s: image too large: a padded extent would exceed %u", what, SSX_GLARE_MAX_EXTENT));
	const uint32_t px = glare_extent(width, in->radius), py = glare_extent(height, in->radius);
	if (px > SSX_GLARE_MAX_EXTENT || in->px != px) return fail(ctx, SSX_ERR_ARG, fmt("ssx_glare_params.px = %u: need %u, the smallest power of two >= max(2, width + 2 radius), and at most %u", in->px, px, SSX_GLARE_MAX_EXTENT));
	if (py > SSX_GLARE_MAX_EXTENT || in->py != py) return fail(ctx, SSX_ERR_ARG, fmt("ssx_glare_params.py = %u: need %u, the smallest power of two >= max(2, height + 2 radius), and at most %u", in->py, py, SSX_GLARE_MAX_EXTENT));
	g->R = in->radius; g->px = px; g->py = py; g->psf = in->psf; g->twx = in->twiddle_x; g->twy = in->twiddle_y; g->on = 0;
	const size_t KK = (size_t)(2u * in->radius + 1u) * (2u * in->radius + 1u);
	for (uint32_t b = 0; b < B; ++b) {
		if (!in->on[b]) continue;
		g->on |= 1ull << b;
		for (size_t k = 0; k < KK; ++k)
			if (!std::isfinite(in->psf[b * KK + k]))
				return fail(ctx, SSX_ERR_ARG, fmt("ssx_glare_params.psf[%u][%u][%u] = %g: must be finite", b, (uint32_t)(k / (2u * in->radius + 1u)), (uint32_t)(k % (2u * in->radius + 1u)), (double)in->psf[b * KK + k]));
	}
	g->active = g->on != 0;
	if (g->active) {
		for (uint32_t m = 0; m < px; ++m)
			if (!std::isfinite(in->twiddle_x[m])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_glare_params.twiddle_x[%u][%u] = %g: must be finite", m / 2u, m & 1u, (double)in->twiddle_x[m]));
		for (uint32_t m = 0; m < py; ++m)
			if (!std::isfinite(in->twiddle_y[m])) return fail(ctx, SSX_ERR_ARG, fmt("ssx_glare_params.twiddle_y[%u][%u] = %g: must be finite", m / 2u, m & 1u, (double)in->twiddle_y[m]));
	}
	return SSX_OK;
}

// The stage-packed tables of this file's header from the caller's T [P / 2][2]: forward | inverse, P entries each (entry 0 is not read)
void glare_pack_twiddles(const float* T, uint32_t P, float2* out) {
	float2* const f = out;
	float2* const i = out + P;
	f[0] = i[0] = make_float2(0.0f, 0.0f);
	uint32_t n = 0;
	while ((1u << n) < P) ++n;
	for (uint32_t s = 1; s <= n; ++s) {
		const uint32_t h = 1u << (s - 1u), D = P >> s;
		for (uint32_t k = 0; k < h; ++k) {
			uint32_t rev = 0;
			for (uint32_t bit = 0; bit + 1u < s; ++bit) rev |= ((k >> bit) & 1u) << (s - 2u - bit);
			const float re = T[2u * k * D], im = T[2u * k * D + 1u];
			f[h + rev] = make_float2(re, im);
			i[h + k] = make_float2(re, -im);
		}
	}
}

uint32_t glare_chunk_bins(uint32_t px, uint32_t py, uint32_t B) { // whole groups of four bins within SSX_GLARE_SCRATCH, at least one
	const uint64_t group = 64ull * px * py;
	const uint64_t groups = std::max<uint64_t>(1u, SSX_GLARE_SCRATCH / group);
	return (uint32_t)std::min<uint64_t>(B, 4u * groups);
}

// d_glare: X | Kf ([chunk bins][py][px] complex each) | the packed twiddles x, y | psf [B][K][K] | out [pixels][B] (| the pure entry's q [pixels][B])
struct GlareBuffers { float2* X; float2* Kf; float2* twx; float2* twy; float* psf; float* out; float* q; };
int glare_buffers(ssx_ctx* ctx, size_t pixels, uint32_t B, const GlareParams& g, bool pure, GlareBuffers* d) {
	const size_t KK = (size_t)(2u * g.R + 1u) * (2u * g.R + 1u), plane = (size_t)g.px * g.py, cb = glare_chunk_bins(g.px, g.py, B);
	if (const int rc = carve(ctx, ctx->d_glare, [&](Carver& c) {
		d->X = reinterpret_cast<float2*>(c.take<float4>(cb * plane / 2u));
		d->Kf = reinterpret_cast<float2*>(c.take<float4>(cb * plane / 2u));
		d->twx = reinterpret_cast<float2*>(c.take<float4>(g.px));
		d->twy = reinterpret_cast<float2*>(c.take<float4>(g.py));
		d->psf = c.take<float>((size_t)B * KK);
		d->out = reinterpret_cast<float*>(c.take<float4>(pixels * B / 4u));
		d->q = pure ? reinterpret_cast<float*>(c.take<float4>(pixels * B / 4u)) : nullptr;
	})) return rc;
	std::vector<float2> tw(2u * (size_t)std::max(g.px, g.py));
	glare_pack_twiddles(g.twx, g.px, tw.data());
	SSX_HIP(ctx, hipMemcpy(d->twx, tw.data(), 2u * (size_t)g.px * sizeof(float2), hipMemcpyHostToDevice));   // (blocking: a local, and the caller's arrays)
	glare_pack_twiddles(g.twy, g.py, tw.data());
	SSX_HIP(ctx, hipMemcpy(d->twy, tw.data(), 2u * (size_t)g.py * sizeof(float2), hipMemcpyHostToDevice));
	uint32_t first = 0, last = B - 1u;   // one copy over the span of the `on` bins (only for g.active); what it carries of `off` bins in between no kernel reads
	while (!((g.on >> first) & 1u)) ++first;
	while (!((g.on >> last) & 1u)) --last;
	SSX_HIP(ctx, hipMemcpy(d->psf + first * KK, g.psf + first * KK, (size_t)(last - first + 1u) * KK * sizeof(float), hipMemcpyHostToDevice));
	return SSX_OK;
}

template <class Kernel> int glare_launch(ssx_ctx* ctx, Kernel kernel, dim3 grid, uint32_t butterflies, size_t lds, const SsxGlareArgs& a) {
	uint32_t lanes = 64u;
	while (lanes < butterflies && lanes < SSX_GLARE_LANES) lanes <<= 1;
	if (lds > 65536u) SSX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	hipLaunchKernelGGL(kernel, grid, dim3(lanes), lds, ctx->stream, a);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

// GLARE on `src` (only read), queued on the context's stream: d.out.  Only for g.active.
int glare_device(ssx_ctx* ctx, const GlareBuffers& d, const GlareParams& g, uint32_t width, uint32_t height, uint32_t B, const float* src) {
	SsxGlareArgs a{};
	a.q = src; a.out = d.out; a.psf = d.psf; a.X = d.X; a.Kf = d.Kf;
	a.twx_f = d.twx; a.twx_i = d.twx + g.px; a.twy_f = d.twy; a.twy_i = d.twy + g.py;
	a.on = g.on; a.width = width; a.height = height; a.B = B; a.R = g.R; a.px = g.px; a.py = g.py;
	while ((1u << a.nx) < g.px) ++a.nx;
	while ((1u << a.ny) < g.py) ++a.ny;
	a.inv = 1.0f / ((float)g.px * (float)g.py);                                                // a power of two: exact
	const uint32_t row_lines = g.px <= 2048u ? 4u : 2u;
	const uint32_t col_lines = std::min(g.px, g.py <= 1024u ? 8u : g.py <= 2048u ? 4u : 2u);
	const size_t row_lds = ((size_t)g.px + (size_t)row_lines * (g.px + 4u)) * sizeof(float2);
	const size_t col_lds = (2u * (size_t)g.py + (size_t)col_lines * (g.py + 4u)) * sizeof(float2);
	const uint32_t cb = glare_chunk_bins(g.px, g.py, B);
	int rc = SSX_OK;
	for (uint32_t b0 = 0; b0 < B; b0 += cb) {
		const uint32_t nb = std::min(cb, B - b0);
		a.b0 = b0;
		for (uint32_t psf_pass = 2; psf_pass-- > 0;) { // Kf first, then X through MULTIPLY
			a.psf_pass = psf_pass;
			const uint32_t rows = (psf_pass ? 1u : height) + 2u * g.R;
			a.lines = row_lines;
			if ((rc = glare_launch(ctx, ssx_glare_rows_kernel, dim3(rows, nb / 4u), row_lines * (g.px / 2u), row_lds, a))) return rc;
			a.lines = col_lines;
			if ((rc = glare_launch(ctx, ssx_glare_columns_kernel, dim3(g.px / col_lines, nb), col_lines * (g.py / 2u), col_lds, a))) return rc;
		}
		a.lines = row_lines;
		if ((rc = glare_launch(ctx, ssx_glare_rows_back_kernel, dim3(height, nb / 4u), row_lines * (g.px / 2u), row_lds, a))) return rc;
	}
	return SSX_OK;
}

} // namespace

extern "C" {

int ssx_glare_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q, const ssx_glare_params* glare, float* out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_glare_images";
	if (!valid_bins(bins)) return fail(ctx, SSX_ERR_ARG, fmt("%s: %u bins: need a multiple of 4 up to 64", what, bins));
	if (!q || !out) return fail(ctx, SSX_ERR_ARG, fmt("%s: q and out must not be NULL", what));
	int rc = denoise_check_size(ctx, width, height, what);
	if (rc) return rc;
	GlareParams g;
	if ((rc = glare_take_params(ctx, what, glare, width, height, bins, &g))) return rc;
	if ((rc = idle_on_device(ctx))) return rc;
	const size_t pixels = (size_t)width * height;
	if (!g.active) { // a copy, bit for bit; nothing is allocated or launched
		if (out != q) std::memmove(out, q, pixels * bins * sizeof(float));
		return SSX_OK;
	}
	GlareBuffers d;
	if ((rc = glare_buffers(ctx, pixels, bins, g, true, &d))) return rc;
	SSX_HIP(ctx, hipMemcpyAsync(d.q, q, pixels * bins * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	if ((rc = glare_device(ctx, d, g, width, height, bins, d.q))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, d.out, pixels * bins * sizeof(float), hipMemcpyDeviceToHost));
	return SSX_OK;
}

// The front is ssx_spectral_develop_lens's, statement by statement (that entry stays as it is); GLARE stands between the lens and the develop kernels.
int ssx_spectral_develop_glare(ssx_ctx* ctx, const ssx_denoise_params* denoise, const ssx_defocus_params* defocus, const ssx_optics_params* optics,
                               const ssx_glare_params* glare, const float* weights, uint32_t channels, float* out, float* bins_out) {
	if (!ctx) return SSX_ERR_ARG;
	const char* const what = "ssx_spectral_develop_glare";
	const bool develops = out || weights;
	int rc = SSX_OK;
	if (develops && (rc = develop_check(ctx, what, channels, weights))) return rc;
	ssx_denoise_params dp;
	if (denoise && (rc = denoise_take_params(ctx, denoise, &dp))) return rc;
	if ((rc = develop_state_ready(ctx, what, denoise != nullptr))) return rc;
	const ssx_render_params& p = ctx->cur;
	if (p.tile_stride != 1u) return fail(ctx, SSX_ERR_STATE, fmt("%s: the context owns one tile in %u (tile_stride): a blur needs its neighbours -- gather the bins and use ssx_defocus_images, ssx_optics_images and ssx_glare_images", what, p.tile_stride));
	const uint32_t B = ctx->spectral_bins;
	DefocusParams f{};
	if (defocus && (rc = defocus_take_params(ctx, what, defocus, B, &f))) return rc;
	const std::vector<float> one(B, 1.0f);
	const std::vector<uint32_t> zero(B, 0u);
	OpticsParams o{ 0.0f, 0.0f, 0u, 0u, one.data(), zero.data(), one.data(), false, false };
	if (optics && (rc = optics_take_params(ctx, what, optics, B, &o))) return rc;
	GlareParams g{};
	if (glare && (rc = glare_take_params(ctx, what, glare, p.width, p.height, B, &g))) return rc;
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
	if (g.active) {
		GlareBuffers gb;
		if ((rc = glare_buffers(ctx, pixels, B, g, false, &gb))) return rc;
		if ((rc = glare_device(ctx, gb, g, p.width, p.height, B, result))) return rc;
		result = gb.out;
	}
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

// ssx_pack.h -- ssx_scene_desc -> the blob layout of ssx_blob.h (host arithmetic only: no device call, no context).
// pack_blob = validate the description, lay the tables out (header + offsets), fill them.  Included by ssx_api.hip (one translation
// unit), behind its helpers debug_env / env_on / fmt and csrc/ssx_jit.h.
#pragma once

namespace {

uint32_t align4(uint32_t words) { return (words + 3u) & ~3u; }

// p = kz of geometry.cpp:19-24; (kx, ky) = the other two axes in the table's fixed order (ssx_blob.h: the reference's two orders per
// kz give the same hits)
const uint32_t kPermAxes[3][2] = SSX_PERM_AXES;

// Every check of the caller's description; the first that fails names the error.
int validate_scene(const ssx_scene_desc* s, std::string& err) {
	auto bad = [&](int code, const std::string& msg) { err = msg; return code; };
	if (s->n_quads == 0 || s->n_quads > SSX_MAX_QUADS) return bad(SSX_ERR_SCENE, fmt("n_quads=%u outside 1..%u", s->n_quads, SSX_MAX_QUADS));
	if (s->n_lights == 0) return bad(SSX_ERR_SCENE, "scene has no lights (reference asserts !lights.empty(), scene.cpp:30)");
	if (s->n_textures > SSX_MAX_TEXTURES) return bad(SSX_ERR_SCENE, "too many textures");
	const uint32_t spec_ids[6] = { s->spec_xbar, s->spec_ybar, s->spec_zbar, s->spec_basis_r, s->spec_basis_g, s->spec_basis_b };
	for (uint32_t id : spec_ids) if (id >= s->n_spectra) return bad(SSX_ERR_ARG, "observer/basis spectrum index out of range");
	for (uint32_t i = 0; i < s->n_spectra; ++i) {
		const ssx_spectrum& sp = s->spectra[i];
		if (sp.n < 2) return bad(SSX_ERR_DATA, "Must have at-least two elements in sampled spectrum!"); // spectrum.cpp:17-20
		if ((uint64_t)sp.offset + sp.n > s->n_samples) return bad(SSX_ERR_ARG, "spectrum samples out of range");
	}
	if (s->uplift == SSX_MODE_RGB) {
		// the RGB build's "spectra" are triples: every table must be {r,g,b,0} on the grid 0,1,2,3 and the
		// "wavelengths" 0,1,2,3 (lambda_min 0, step 1), so that lookups return the components exactly
		if (s->lambda_min != 0.0f || s->lambda_step != 1.0f) return bad(SSX_ERR_ARG, "RGB mode needs lambda_min = 0, lambda_step = 1");
		for (uint32_t i = 0; i < s->n_spectra; ++i)
			if (s->spectra[i].n != 4u || s->spectra[i].low != 0.0f || s->spectra[i].delta_recip != 1.0f || s->samples[s->spectra[i].offset + 3u] != 0.0f)
				return bad(SSX_ERR_ARG, "RGB mode needs every spectrum as {r,g,b,0} with low = 0, delta_recip = 1");
	}
	for (uint32_t i = 0; i < s->n_materials; ++i) {
		const ssx_material& m = s->materials[i];
		if (m.kind > SSX_MTL_MIRROR || m.albedo_mode > SSX_ALBEDO_TEXTURE) return bad(SSX_ERR_ARG, "bad material kind/mode");
		if (m.emission_spectrum >= s->n_spectra) return bad(SSX_ERR_ARG, "material emission spectrum out of range");
		if (m.albedo_mode == SSX_ALBEDO_CONSTANT && m.albedo_spectrum >= s->n_spectra) return bad(SSX_ERR_ARG, "material albedo spectrum out of range");
		if (m.albedo_mode == SSX_ALBEDO_TEXTURE && m.albedo_texture >= s->n_textures) return bad(SSX_ERR_ARG, "material texture out of range");
	}
	for (uint32_t i = 0; i < s->n_quads; ++i) if (s->quads[i].material >= s->n_materials) return bad(SSX_ERR_ARG, "quad material out of range");
	for (uint32_t i = 0; i < s->n_quads; ++i) if (s->quads[i].flags & ~(uint32_t)(SSX_PRIM_LIGHT | SSX_PRIM_TRI)) return bad(SSX_ERR_ARG, "unknown primitive flags");
	// ssx_exact::rcp is exact for |x| <= 2^126 (determinants of the watertight test are products of two coordinate differences):
	// refuse coordinates that could leave the range instead of losing bit parity silently
	for (uint32_t i = 0; i < s->n_quads; ++i) {
		const ssx_vertex* vs[4] = { &s->quads[i].v00, &s->quads[i].v10, &s->quads[i].v11, &s->quads[i].v01 };
		const int nv = (s->quads[i].flags & SSX_PRIM_TRI) ? 3 : 4; // (a triangle's v01 is not part of the scene)
		for (int v = 0; v < nv; ++v) for (float c : vs[v]->pos) if (!(std::fabs(c) <= 0x1p30f)) return bad(SSX_ERR_SCENE, "vertex coordinate beyond 2^30 (or not a number)");
	}
	for (float c : s->cam_pos) if (!(std::fabs(c) <= 0x1p30f)) return bad(SSX_ERR_SCENE, "camera position beyond 2^30 (or not a number)");
	for (uint32_t i = 0; i < s->n_lights; ++i) if (s->lights[i] >= s->n_quads) return bad(SSX_ERR_ARG, "light index out of range");
	return SSX_OK;
}

// What the scene's sharing pattern of corners is (ssx_upload_scene decides about run-time specialisation).
struct PackInfo { bool candidate = false; ssx_jit::VidTable vid; };

// Where everything goes: the header with its offsets, and what the fill needs besides the description.
struct BlobLayout {
	SsxBlobHeader h{};
	std::vector<uint32_t> sample_pos;   // per spectrum: word offset of its first sample; 0 = the kernels read no table of its own
	ssx_jit::VidTable vid;              // per quad: ids of its corners among the distinct vertices (scenes that may run a specialised pass 1)
	std::vector<const float*> distinct; // positions of the distinct vertices, numbered by first occurrence
};

// the header's scene constants (everything but the topology and the offsets)
void scene_constants(const ssx_scene_desc* s, SsxBlobHeader& h) {
	memcpy(h.pv_inv, s->pv_inv, sizeof h.pv_inv);
	memcpy(h.cam_pos, s->cam_pos, sizeof h.cam_pos);
	std::memcpy(h.cam_dir, s->cam_dir, sizeof h.cam_dir);
	h.lambda_min = s->lambda_min; h.lambda_step = s->lambda_step;
	h.n_quads = s->n_quads; h.n_lights = s->n_lights; h.n_materials = s->n_materials; h.n_spectra = s->n_spectra;
	h.spec_xbar = s->spec_xbar; h.spec_ybar = s->spec_ybar; h.spec_zbar = s->spec_zbar;
	h.spec_basis_r = s->spec_basis_r; h.spec_basis_g = s->spec_basis_g; h.spec_basis_b = s->spec_basis_b;
	h.n_textures = s->n_textures;
	h.uplift = s->uplift;
	h.n_lights_recip = 1.0 / (double)(float)s->n_lights;
	for (int r = 0; r < 4; ++r) { volatile double z = 0.0, one = 1.0; h.q_const[r] = h.pv_inv[2 * 4 + r] * z + h.pv_inv[3 * 4 + r] * one; } // (volatile: the two products and the sum as written, whatever the host compiler would like to fold)
	for (int k = 0; k < 3; ++k) h.cam_pos_d[k] = (double)s->cam_pos[k];
	// a black surface ends its path on the random draws alone (ssx_kernels.hip path_step) -- provided (emitted * n_dot_l) * 0 is 0: no NaN / inf / huge emission sample
	h.black_ends_path = 1u;
	for (uint32_t i = 0; i < s->n_lights; ++i) {
		const ssx_spectrum& es = s->spectra[s->materials[s->quads[s->lights[i]].material].emission_spectrum];
		for (uint32_t k = 0; k < es.n; ++k) if (!(std::fabs(s->samples[es.offset + k]) <= 0x1p60f)) h.black_ends_path = 0u;
	}
	if (const char* e = debug_env("SSX_BLACK_SHORTCUT")) { if (e[0] == '0') h.black_ends_path = 0u; } // A/B runs and tests: evaluate everything
	for (int i = 0; i < 4; ++i) { volatile float fi = (float)i; h.lambda_steps[i] = fi * s->lambda_step; } // one IEEE float multiply each, as spectrum.cpp:63
	const ssx_spectrum &r = s->spectra[s->spec_basis_r], &g = s->spectra[s->spec_basis_g], &b = s->spectra[s->spec_basis_b];
	const ssx_spectrum &ox = s->spectra[s->spec_xbar], &oy = s->spectra[s->spec_ybar], &oz = s->spectra[s->spec_zbar];
	h.observer_one_grid = (ox.n == oy.n && ox.n == oz.n && ox.low == oy.low && ox.low == oz.low && ox.delta_recip == oy.delta_recip && ox.delta_recip == oz.delta_recip) ? 1u : 0u;
	h.basis_one_grid = (r.n == g.n && r.n == b.n && r.low == g.low && r.low == b.low && r.delta_recip == g.delta_recip && r.delta_recip == b.delta_recip) ? 1u : 0u;
	for (uint32_t q = 0; q < s->n_quads; ++q) h.tri_valid[q >> 5] |= ((s->quads[q].flags & SSX_PRIM_TRI) ? 1ull : 3ull) << (2u * (q & 31u));
}

// force_topology: -1 = the built-in topology the scene's sharing pattern matches, else 0 (generic); 3 = the tables of a kernel
// compiled for the scene's own pattern.  d_jh: the uplift's table in HBM (an address the header carries).
int layout_blob(const ssx_scene_desc* s, const void* d_jh, int force_topology, PackInfo* info, BlobLayout& L, std::string& err) {
	SsxBlobHeader& h = L.h;
	scene_constants(s, h);

	// Which corners coincide?  Distinct vertices numbered by first occurrence of their position (bitwise); if the pattern is
	// that of one of the reference's built-in meshes (csrc/ssx_pass1_gen.h) the kernel with that topology's pass 1 runs.
	L.vid.assign(s->n_quads, std::array<uint8_t, 4>{});
	bool any_tri = false;
	for (uint32_t q = 0; q < s->n_quads; ++q) any_tri = any_tri || (s->quads[q].flags & SSX_PRIM_TRI);
	const bool topo_candidate = s->n_quads <= 32u && !any_tri; // the built-in topologies: at most 32 primitives, all quads
	for (uint32_t q = 0; topo_candidate && q < s->n_quads; ++q) {
		const ssx_vertex* vs[4] = { &s->quads[q].v00, &s->quads[q].v10, &s->quads[q].v11, &s->quads[q].v01 };
		for (int v = 0; v < 4; ++v) {
			size_t k = 0;
			while (k < L.distinct.size() && memcmp(L.distinct[k], vs[v]->pos, 12) != 0) ++k;
			if (k == L.distinct.size()) L.distinct.push_back(vs[v]->pos);
			L.vid[q][v] = (uint8_t)k; // n_quads <= 32: at most 128 distinct vertices
		}
	}
	h.topology = 0; h.n_verts = (uint32_t)L.distinct.size();
	for (const SsxTopology& t : ssx_topologies) {
		if (!topo_candidate || t.n_quads != s->n_quads || t.n_verts != L.distinct.size()) continue;
		bool same = true;
		for (uint32_t q = 0; q < s->n_quads && same; ++q) for (int v = 0; v < 4; ++v) same = same && t.vid[q][v] == L.vid[q][v];
		if (same) h.topology = t.id;
	}
	if (env_on("SSX_GENERIC_KERNEL")) h.topology = 0; // A/B measurements and tests of the generic loop on the built-in scenes
	if (info) { info->candidate = topo_candidate && h.topology == 0 && !env_on("SSX_GENERIC_KERNEL"); info->vid = L.vid; }
	if (force_topology == 3 && topo_candidate) h.topology = 3; // (the caller holds, or waits for, kernels compiled for this pattern: csrc/ssx_jit.h)

	uint32_t off = (uint32_t)(sizeof(SsxBlobHeader) / 4);
	h.off_quads = off;     off = align4(off + s->n_quads * (uint32_t)(sizeof(SsxBlobQuad) / 4));
	h.off_lights = off;    off = align4(off + s->n_lights);
	h.off_spectra = off;   off = align4(off + s->n_spectra * (uint32_t)(sizeof(SsxBlobSpectrum) / 4));
	// every table gets two zero samples in front and two behind (hero_index in ssx_kernels.hip)
	// A table gets LDS space only if the kernels read it as a table of its own: a material's emission /
	// constant albedo, or a basis / observer table that is not covered by its interleaved copy below.
	std::vector<uint8_t> table_needed(s->n_spectra, 0);
	for (uint32_t i = 0; i < s->n_materials; ++i) {
		table_needed[s->materials[i].emission_spectrum] = 1;
		if (s->materials[i].albedo_mode == SSX_ALBEDO_CONSTANT) table_needed[s->materials[i].albedo_spectrum] = 1;
	}
	if (!h.basis_one_grid) table_needed[s->spec_basis_r] = table_needed[s->spec_basis_g] = table_needed[s->spec_basis_b] = 1;
	if (!h.observer_one_grid) table_needed[s->spec_xbar] = table_needed[s->spec_ybar] = table_needed[s->spec_zbar] = 1;
	L.sample_pos.assign(s->n_spectra, 0u); // (a descriptor without samples keeps (low, delta_recip, n) for the shared index)
	for (uint32_t i = 0; i < s->n_spectra; ++i) if (table_needed[i]) { L.sample_pos[i] = off + 2u; off += s->spectra[i].n + 4u; }
	off = align4(off);
	auto one_grid4 = [&](uint32_t ia, uint32_t flag) -> uint32_t { // interleaved float4 copy of three tables on one grid
		if (!flag) return 0u;
		const uint32_t at = off + 8u; // elements -2, -1 sit at `off`
		off = align4(off + 4u * (s->spectra[ia].n + 4u));
		return at;
	};
	h.off_basis4 = one_grid4(s->spec_basis_r, h.basis_one_grid);
	h.off_observer4 = one_grid4(s->spec_xbar, h.observer_one_grid);
	h.off_lut = off;       off = align4(off + 256u);
	h.off_tex = off;       off = align4(off + s->n_textures * (uint32_t)(sizeof(SsxBlobTexture) / 4));
	if (s->uplift == SSX_UPLIFT_JH) {
		h.jh_res = s->jh_res;
		h.off_jh_scale = off;  off = align4(off + s->jh_res);
	}
	if (s->uplift == SSX_UPLIFT_JH || s->uplift == SSX_UPLIFT_MENG) { // the uplift's table in HBM (JH coefficients / Meng grid)
		h.jh_data_lo = (uint32_t)(uintptr_t)d_jh; h.jh_data_hi = (uint32_t)((uint64_t)(uintptr_t)d_jh >> 32);
	}
	if (h.topology) { // distinct-vertex table per axis permutation + vertex ids per quad
		h.vtab_stride = (3u * h.n_verts + 1u) & ~1u; // even: the {x,y} pairs stay 8-byte aligned
		h.off_vtab = off;  off = align4(off + SSX_PERM_COUNT * h.vtab_stride);
		h.off_vid = off;   off = align4(off + s->n_quads);
		h.off_vtab4 = off; off = align4(off + SSX_PERM_COUNT * 4u * h.n_verts);   // 16-byte aligned (align4)
		h.off_triofs = off; off = align4(off + 4u * s->n_quads);                    // 8-byte aligned entries
	}
	h.words_without_perm = off;
	h.off_perm = off;      off = align4(off + s->n_quads * SSX_PERM_WORDS_PER_QUAD); // last: not staged by the specialised kernels
	h.total_words = off;
	// prefix + blob + the four waves' shadow-ray queues is what a path-kernel workgroup allocates (<= 64 KiB); the
	// calibration render stages the whole blob also where the scene's own kernel stops before the per-quad table.
	// A scene whose tables exceed that with the permuted vertex table (288 bytes per primitive) keeps that table in HBM
	// (generic kernels read it from there: SsxBlobHeader::perm_hbm; ssx_upload_scene fills in the address).
	h.perm_hbm = ((size_t)off * 4 > SSX_BLOB_MAX_BYTES) ? 1u : 0u;
	const uint32_t staged = h.perm_hbm ? h.words_without_perm : off;
	if ((size_t)staged * 4 > SSX_BLOB_MAX_BYTES) { err = fmt("scene tables need %u bytes of LDS (max %u)", staged * 4, SSX_BLOB_MAX_BYTES); return SSX_ERR_SCENE; }
	return SSX_OK;
}

// d_tex: the textures' texels on the device (addresses the texture table carries)
void fill_blob(const ssx_scene_desc* s, const std::vector<const void*>& d_tex, const BlobLayout& L, std::vector<uint32_t>& blob) {
	const SsxBlobHeader& h = L.h;
	blob.assign(h.total_words, 0u);
	memcpy(blob.data(), &h, sizeof h);
	auto desc = [&](uint32_t id) {
		SsxBlobSpectrum d;
		d.offset = L.sample_pos[id]; d.n = s->spectra[id].n;
		d.low = s->spectra[id].low; d.delta_recip = s->spectra[id].delta_recip;
		return d;
	};
	float* perm = reinterpret_cast<float*>(blob.data() + h.off_perm);
	SsxBlobQuad* bq = reinterpret_cast<SsxBlobQuad*>(blob.data() + h.off_quads);
	for (uint32_t q = 0; q < s->n_quads; ++q) {
		const ssx_quad& Q = s->quads[q];
		const ssx_vertex* vs[4] = { &Q.v00, &Q.v10, &Q.v11, (Q.flags & SSX_PRIM_TRI) ? &Q.v00 : &Q.v01 }; // a triangle's v01 is not part of the scene
		for (uint32_t p = 0; p < SSX_PERM_COUNT; ++p) {
			const uint32_t kz = p, kx = kPermAxes[p][0], ky = kPermAxes[p][1];
			float* dst = perm + q * SSX_PERM_WORDS_PER_QUAD + p * 12u;
			for (int v = 0; v < 4; ++v) { dst[2 * v + 0] = vs[v]->pos[kx]; dst[2 * v + 1] = vs[v]->pos[ky]; dst[8 + v] = vs[v]->pos[kz]; } // x0 y0 .. x3 y3 | z0..z3
		}
		for (int v = 0; v < 4; ++v) {
			memcpy(bq[q].pos[v], vs[v]->pos, 12);
			memcpy(bq[q].st[v], vs[v]->st, 8);
		}
		memcpy(bq[q].normal[0], Q.normal0, 12);
		memcpy(bq[q].normal[1], Q.normal1, 12);
		const ssx_material& m = s->materials[Q.material];
		bq[q].kind = m.kind; bq[q].albedo_mode = m.albedo_mode; bq[q].albedo_tex = m.albedo_texture;
		bq[q].albedo = desc(m.albedo_mode == SSX_ALBEDO_CONSTANT ? m.albedo_spectrum : m.emission_spectrum);
		bq[q].emission = desc(m.emission_spectrum);
		// any nonzero emission sample?  (all-zero tables evaluate to exactly +0 at every wavelength)
		const ssx_spectrum& es = s->spectra[m.emission_spectrum];
		bq[q].is_tri = (Q.flags & SSX_PRIM_TRI) ? 1u : 0u;
		bq[q].is_emissive = 0;
		for (uint32_t k = 0; k < es.n; ++k) if (s->samples[es.offset + k] != 0.0f) bq[q].is_emissive = 1;
	}
	if (h.topology) {
		float* vt = reinterpret_cast<float*>(blob.data() + h.off_vtab);
		float* vt4 = reinterpret_cast<float*>(blob.data() + h.off_vtab4);
		for (uint32_t p = 0; p < SSX_PERM_COUNT; ++p) {
			const uint32_t kz = p, kx = kPermAxes[p][0], ky = kPermAxes[p][1];
			float* dst = vt + p * h.vtab_stride;
			for (uint32_t k = 0; k < h.n_verts; ++k) { dst[2 * k] = L.distinct[k][kx]; dst[2 * k + 1] = L.distinct[k][ky]; dst[2 * h.n_verts + k] = L.distinct[k][kz]; }
			float* d4 = vt4 + p * 4u * h.n_verts;
			for (uint32_t k = 0; k < h.n_verts; ++k) { d4[4 * k] = L.distinct[k][kx]; d4[4 * k + 1] = L.distinct[k][ky]; d4[4 * k + 2] = L.distinct[k][kz]; d4[4 * k + 3] = 0.0f; }
		}
		for (uint32_t q = 0; q < s->n_quads; ++q) {
			const std::array<uint8_t, 4>& id = L.vid[q];
			blob[h.off_vid + q] = (uint32_t)id[0] | ((uint32_t)id[1] << 8) | ((uint32_t)id[2] << 16) | ((uint32_t)id[3] << 24);
			// triangle `which` of quad q = vertices (v00, v10 | v11, v11 | v01): byte offsets of their 16-byte records (n_verts <= 128: below 2^16)
			for (uint32_t which = 0; which < 2u; ++which) {
				const uint32_t a = 16u * id[0], b = 16u * id[1 + which], c = 16u * id[2 + which];
				blob[h.off_triofs + 2u * (2u * q + which)] = a | (b << 16);
				blob[h.off_triofs + 2u * (2u * q + which) + 1u] = c;
			}
		}
	}
	memcpy(blob.data() + h.off_lights, s->lights, 4 * s->n_lights);
	SsxBlobSpectrum* bs = reinterpret_cast<SsxBlobSpectrum*>(blob.data() + h.off_spectra);
	for (uint32_t i = 0; i < s->n_spectra; ++i) {
		bs[i] = desc(i);
		if (L.sample_pos[i]) memcpy(blob.data() + L.sample_pos[i], s->samples + s->spectra[i].offset, 4 * (size_t)s->spectra[i].n); // blob is zero-filled: the guards stay 0
	}
	auto fill4 = [&](uint32_t at, uint32_t ia, uint32_t ib, uint32_t ic) {
		if (!at) return;
		float* dst = reinterpret_cast<float*>(blob.data() + at);
		for (uint32_t k = 0; k < s->spectra[ia].n; ++k) {
			dst[4 * k + 0] = s->samples[s->spectra[ia].offset + k];
			dst[4 * k + 1] = s->samples[s->spectra[ib].offset + k];
			dst[4 * k + 2] = s->samples[s->spectra[ic].offset + k];
		}
	};
	fill4(h.off_basis4, s->spec_basis_r, s->spec_basis_g, s->spec_basis_b);
	fill4(h.off_observer4, s->spec_xbar, s->spec_ybar, s->spec_zbar);
	memcpy(blob.data() + h.off_lut, s->srgb_to_linear, 4 * 256);
	if (s->uplift == SSX_UPLIFT_JH) memcpy(blob.data() + h.off_jh_scale, s->jh_scale, 4 * (size_t)s->jh_res);
	SsxBlobTexture* bt = reinterpret_cast<SsxBlobTexture*>(blob.data() + h.off_tex);
	for (uint32_t i = 0; i < s->n_textures; ++i) {
		uint64_t p = (uint64_t)(uintptr_t)d_tex[i];
		bt[i].ptr_lo = (uint32_t)p; bt[i].ptr_hi = (uint32_t)(p >> 32);
		bt[i].w = s->textures[i].width; bt[i].h = s->textures[i].height;
	}
}

// Packs ssx_scene_desc into the blob layout of ssx_blob.h; on failure `err` says why and `blob` is untouched.
int pack_blob(const ssx_scene_desc* s, const std::vector<const void*>& d_tex, const void* d_jh, std::vector<uint32_t>& blob, std::string& err, int force_topology = -1, PackInfo* info = nullptr) {
	int rc = validate_scene(s, err);
	BlobLayout L;
	if (!rc) rc = layout_blob(s, d_jh, force_topology, info, L, err);
	if (!rc) fill_blob(s, d_tex, L, blob);
	return rc;
}

} // namespace

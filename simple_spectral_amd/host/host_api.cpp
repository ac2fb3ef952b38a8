// host_api.cpp -- C entry points of libssx_host.so (include/ssx_host.h).
#include "../../include/ssx_host.h"

#include "checkpoint.hpp"
#include "color.hpp"
#include "develop.hpp"
#include "image_io.hpp"
#include "scene.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

struct ssh_scene {
	std::unique_ptr<ssx::ColorData> color;
	std::unique_ptr<ssx::JHModel> jh;
	std::unique_ptr<ssx::MengGrid> meng;
	std::unique_ptr<ssx::Scene> scene;
};

namespace {
thread_local std::string g_error;
int report(const ssx::HostError& e) { g_error = e.message; return e.code; }
} // namespace

extern "C" {

const char* ssh_last_error(void) { return g_error.c_str(); }

int ssh_scene_create_ex(const char* scene_name, const char* data_dir, int observer,
                        const uint8_t* tex_rgb, uint32_t tex_w, uint32_t tex_h, const char* texture_path,
                        float light_scale, uint32_t uplift, const char* jh_coeff_path, uint32_t jh_res,
                        ssh_scene** out) {
	if (!scene_name || !data_dir || !out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	*out = nullptr;
	try {
		auto s = std::make_unique<ssh_scene>();
		s->color = std::make_unique<ssx::ColorData>(data_dir, observer);
		const bool els = (uplift & 0x100u) == 0u; // bit 8 of `uplift`: scene built for the non-ELS integrator
		const bool rgb_mode = (uplift & 0x200u) != 0u; // bit 9: RENDER_MODE_RGB (then the low byte is ignored)
		uplift &= 0xFFu;
		if (rgb_mode) { uplift = SSX_UPLIFT_OURS; s->color->rgb_output_transform = true; }
		if (uplift == SSX_UPLIFT_JH) {
			if (observer != 1931) throw ssx::HostError{ -3, "Only our algorithm currently implements support for the newest CIE standard observer!" };
			const std::string path = jh_coeff_path ? jh_coeff_path : "";
			bool loaded = false;
			if (!path.empty()) {
				try { s->jh = std::make_unique<ssx::JHModel>(ssx::jh_load(path)); loaded = true; } catch (const ssx::HostError&) {}
			}
			if (!loaded) {
				s->jh = std::make_unique<ssx::JHModel>(ssx::jh_optimize(*s->color, jh_res ? jh_res : 64u));
				if (!path.empty()) ssx::jh_save(*s->jh, path);
			}
		} else if (uplift == SSX_UPLIFT_MENG) { // jh_coeff_path names the grid file (meng2015.hpp)
			if (observer != 1931) throw ssx::HostError{ -3, "Only our algorithm currently implements support for the newest CIE standard observer!" };
			s->meng = std::make_unique<ssx::MengGrid>(ssx::meng_load(jh_coeff_path ? jh_coeff_path : ""));
			s->color->meng_output_transform = true;
		} else if (uplift != SSX_UPLIFT_OURS) {
			throw ssx::HostError{ -3, "unsupported uplift variant" };
		}
		ssx::Texture tex;
		const ssx::Texture* texp = nullptr;
		if (tex_rgb && tex_w && tex_h) {
			tex.width = tex_w; tex.height = tex_h;
			tex.rgb.assign(tex_rgb, tex_rgb + (size_t)3 * tex_w * tex_h);
			texp = &tex;
		} else if (texture_path && *texture_path) {
			tex = ssx::load_texture(texture_path);
			texp = &tex;
		}
		s->scene = std::make_unique<ssx::Scene>(*s->color, scene_name, data_dir, texp, light_scale, s->jh.get(), els, s->meng.get(), rgb_mode);
		*out = s.release();
		return SSX_OK;
	} catch (const ssx::HostError& e) {
		return report(e);
	} catch (const std::exception& e) {
		g_error = e.what();
		return SSX_ERR_DATA;
	}
}

int ssh_scene_create(const char* scene_name, const char* data_dir, int observer,
                     const uint8_t* tex_rgb, uint32_t tex_w, uint32_t tex_h, const char* texture_path,
                     float light_scale, ssh_scene** out) {
	return ssh_scene_create_ex(scene_name, data_dir, observer, tex_rgb, tex_w, tex_h, texture_path, light_scale, SSX_UPLIFT_OURS, nullptr, 0, out);
}

void ssh_scene_destroy(ssh_scene* scene) { delete scene; }

const ssx_scene_desc* ssh_scene_desc(const ssh_scene* scene) { return scene ? &scene->scene->desc() : nullptr; }

int ssh_xyza_to_srgba(const ssh_scene* scene, const float* xyza, float* srgba, size_t n) {
	if (!scene || !xyza || !srgba) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	scene->color->xyza_to_srgba(xyza, srgba, n);
	return SSX_OK;
}

int ssh_save_image(const char* path, const float* srgba, uint32_t width, uint32_t height) {
	if (!path || !srgba) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try { ssx::save_image(path, srgba, width, height); return SSX_OK; }
	catch (const ssx::HostError& e) { return report(e); }
}

int ssh_load_png_rgb8(const char* path, uint8_t** rgb_out, uint32_t* width, uint32_t* height) {
	if (!path || !rgb_out || !width || !height) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try {
		ssx::Texture t = ssx::load_png_rgb8(path);
		*rgb_out = static_cast<uint8_t*>(malloc(t.rgb.size()));
		memcpy(*rgb_out, t.rgb.data(), t.rgb.size());
		*width = t.width; *height = t.height;
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
}
void ssh_free(void* p) { free(p); }

int ssh_checkpoint_save_moments(const char* path, const ssx_sums_info_t* info, const char* scene_name, const char* options_text, const double* sums, const double* noise_s2,
                                const ssx_spectral_info_t* spectral_info, const double* spectral_sums, const uint32_t* spectral_counts, const double* q) {
	if (!path || !info || !sums || (spectral_info && (!spectral_sums || !spectral_counts))) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (q && !spectral_info) { g_error = "ssh_checkpoint_save_moments: q without the wavelength bins it belongs to (spectral_info is NULL)"; return SSX_ERR_ARG; }
	try {
		ssx::Checkpoint c;
		c.info = *info;
		c.scene_name = scene_name ? scene_name : ""; c.options_text = options_text ? options_text : "";
		const size_t pixels = (size_t)info->width * info->height;
		c.sums.assign(sums, sums + pixels * 4);
		if (noise_s2) c.s2.assign(noise_s2, noise_s2 + pixels);
		if (spectral_info) {
			if (spectral_info->bins < 4u || spectral_info->bins > 64u || spectral_info->bins % 4u) { g_error = "ssh_checkpoint_save_spectral: bins must be a multiple of 4 in 4..64"; return SSX_ERR_ARG; }
			c.spectral = *spectral_info;
			c.spectral_sums.assign(spectral_sums, spectral_sums + pixels * spectral_info->bins);
			c.spectral_counts.assign(spectral_counts, spectral_counts + pixels * (spectral_info->bins / 4u));
			if (q) c.moments.assign(q, q + pixels * spectral_info->bins);
		}
		ssx::checkpoint_save(path, c);
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
	catch (const std::exception& e) { g_error = e.what(); return SSX_ERR_DATA; }
}

int ssh_checkpoint_save_spectral(const char* path, const ssx_sums_info_t* info, const char* scene_name, const char* options_text, const double* sums, const double* noise_s2,
                                 const ssx_spectral_info_t* spectral_info, const double* spectral_sums, const uint32_t* spectral_counts) {
	return ssh_checkpoint_save_moments(path, info, scene_name, options_text, sums, noise_s2, spectral_info, spectral_sums, spectral_counts, nullptr);
}

int ssh_checkpoint_save(const char* path, const ssx_sums_info_t* info, const char* scene_name, const char* options_text,
                        const double* sums, const double* noise_s2) {
	return ssh_checkpoint_save_moments(path, info, scene_name, options_text, sums, noise_s2, nullptr, nullptr, nullptr, nullptr);
}

int ssh_checkpoint_load_moments(const char* path, ssx_sums_info_t* info, char* scene_name, size_t scene_name_size, char* options_text, size_t options_text_size,
                                double** sums_out, double** noise_s2_out, ssx_spectral_info_t* spectral_info, double** spectral_sums_out, uint32_t** spectral_counts_out,
                                double** q_out) {
	if (!path || !info || !sums_out || (spectral_info && (!spectral_sums_out || !spectral_counts_out)) || (q_out && !spectral_info)) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	*sums_out = nullptr;
	if (q_out) *q_out = nullptr;
	if (noise_s2_out) *noise_s2_out = nullptr;
	if (spectral_info) { memset(spectral_info, 0, sizeof *spectral_info); *spectral_sums_out = nullptr; *spectral_counts_out = nullptr; }
	double* s2 = nullptr; double* bins = nullptr; uint32_t* counts = nullptr;
	try {
		const ssx::Checkpoint c = ssx::checkpoint_load(path);
		auto text = [](const std::string& s, char* out, size_t n) { if (out && n) { const size_t k = s.size() < n - 1 ? s.size() : n - 1; memcpy(out, s.data(), k); out[k] = '\0'; } };
		auto copy = [](const auto& v) { // (a malloc'ed copy: ssh_free releases it)
			using T = typename std::decay_t<decltype(v)>::value_type;
			T* p = static_cast<T*>(malloc(v.size() * sizeof(T)));
			if (!p) throw std::bad_alloc();
			memcpy(p, v.data(), v.size() * sizeof(T));
			return p;
		};
		*info = c.info;
		text(c.scene_name, scene_name, scene_name_size);
		text(c.options_text, options_text, options_text_size);
		*sums_out = copy(c.sums);
		if (noise_s2_out && !c.s2.empty()) *noise_s2_out = s2 = copy(c.s2);
		if (spectral_info && c.spectral.bins) {
			*spectral_sums_out = bins = copy(c.spectral_sums);
			*spectral_counts_out = counts = copy(c.spectral_counts);
			if (q_out && !c.moments.empty()) *q_out = copy(c.moments);
			*spectral_info = c.spectral;
		}
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
	catch (const std::exception& e) { // (out of memory half-way: nothing is handed out)
		free(*sums_out); *sums_out = nullptr; free(s2); free(bins); free(counts);
		if (q_out) *q_out = nullptr; // (the last copy made: when it throws nothing of it exists)
		if (noise_s2_out) *noise_s2_out = nullptr;
		if (spectral_info) { *spectral_sums_out = nullptr; *spectral_counts_out = nullptr; }
		g_error = e.what(); return SSX_ERR_DATA;
	}
}

int ssh_checkpoint_load_spectral(const char* path, ssx_sums_info_t* info, char* scene_name, size_t scene_name_size, char* options_text, size_t options_text_size,
                                 double** sums_out, double** noise_s2_out, ssx_spectral_info_t* spectral_info, double** spectral_sums_out, uint32_t** spectral_counts_out) {
	return ssh_checkpoint_load_moments(path, info, scene_name, scene_name_size, options_text, options_text_size, sums_out, noise_s2_out, spectral_info, spectral_sums_out, spectral_counts_out, nullptr);
}

int ssh_checkpoint_load(const char* path, ssx_sums_info_t* info, char* scene_name, size_t scene_name_size, char* options_text, size_t options_text_size,
                        double** sums_out, double** noise_s2_out) {
	return ssh_checkpoint_load_moments(path, info, scene_name, scene_name_size, options_text, options_text_size, sums_out, noise_s2_out, nullptr, nullptr, nullptr, nullptr);
}

int ssh_sums_merge(double* dst, double* dst_s2, const double* src, const double* src_s2, const ssx_sums_info_t* src_info) {
	if (!dst || !src || !src_info || src_info->struct_size != sizeof *src_info) { g_error = "NULL argument or ssx_sums_info_t.struct_size mismatch"; return SSX_ERR_ARG; }
	ssx::sums_merge(dst, dst_s2, src, src_s2, *src_info);
	return SSX_OK;
}

int ssh_spectral_merge(double* dst_sums, uint32_t* dst_counts, const double* src_sums, const uint32_t* src_counts, uint32_t bins, const ssx_sums_info_t* src_sums_info) {
	if (!src_sums_info || src_sums_info->struct_size != sizeof *src_sums_info) { g_error = "NULL argument or ssx_sums_info_t.struct_size mismatch"; return SSX_ERR_ARG; }
	if (bins < 4u || bins > 64u || bins % 4u) { g_error = "ssh_spectral_merge: bins must be a multiple of 4 in 4..64"; return SSX_ERR_ARG; }
	if ((!dst_sums) != (!src_sums) || (!dst_counts) != (!src_counts)) { g_error = "ssh_spectral_merge: sums and counts come in pairs of dst and src"; return SSX_ERR_ARG; }
	ssx::spectral_merge(dst_sums, dst_counts, src_sums, src_counts, bins, *src_sums_info);
	return SSX_OK;
}

int ssh_moments_merge(double* dst_q, const double* src_q, uint32_t bins, const ssx_sums_info_t* src_sums_info) {
	if (!dst_q || !src_q || !src_sums_info || src_sums_info->struct_size != sizeof *src_sums_info) { g_error = "NULL argument or ssx_sums_info_t.struct_size mismatch"; return SSX_ERR_ARG; }
	if (bins < 4u || bins > 64u || bins % 4u) { g_error = "ssh_moments_merge: bins must be a multiple of 4 in 4..64"; return SSX_ERR_ARG; }
	ssx::moments_merge(dst_q, src_q, bins, *src_sums_info);
	return SSX_OK;
}

int ssh_save_npy_f32(const char* path, const float* data, const uint32_t* shape, uint32_t ndim) {
	if (!path || !data || !shape || ndim == 0 || ndim > 8) { g_error = "NULL argument or ndim outside 1..8"; return SSX_ERR_ARG; }
	try {
		size_t dims[8];
		for (uint32_t d = 0; d < ndim; ++d) dims[d] = shape[d];
		ssx::save_npy_f32(path, data, dims, ndim);
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
}

int ssh_probe_derive(uint32_t regions, uint32_t bins, const double* SS, const uint64_t* NN, const double* VV, const uint64_t* UU, double* mean, double* std_err) {
	if (!SS || !NN || !VV || !UU) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	ssx::probe_derive(regions, bins, SS, NN, VV, UU, mean, std_err);
	return SSX_OK;
}

int ssh_probe_save_csv(const char* path, uint32_t regions, uint32_t bins, float lambda_min, float bin_width, const double* SS, const uint64_t* NN, const double* VV, const uint64_t* UU) {
	if (!path || !SS || !NN || !VV || !UU) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try { ssx::save_probe_csv(path, regions, bins, lambda_min, bin_width, SS, NN, VV, UU); return SSX_OK; }
	catch (const ssx::HostError& e) { return report(e); }
}

int ssh_spectral_noise_derive(uint32_t bins, const double* EV, const double* EM, const uint64_t* PP, const uint64_t* PU, double* noise, double* coverage, double* rel) {
	if (!EV || !EM || !PP || !PU) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	ssx::spectral_noise_derive(bins, EV, EM, PP, PU, noise, coverage, rel);
	return SSX_OK;
}

int ssh_spectral_noise_save_csv(const char* path, uint32_t bins, float lambda_min, float bin_width, const double* EV, const double* EM, const uint64_t* PP, const uint64_t* PU) {
	if (!path || !EV || !EM || !PP || !PU) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try { ssx::save_spectral_noise_csv(path, bins, lambda_min, bin_width, EV, EM, PP, PU); return SSX_OK; }
	catch (const ssx::HostError& e) { return report(e); }
}

int ssh_compare_derive(uint32_t regions, uint32_t bins, const double* DD, const double* VV, const double* X2, const uint64_t* CC, const uint64_t* NC, const uint64_t* EX,
                       double* mean_diff, double* std_err, double* z, double* chi2, double* exceed, double* coverage) {
	if (!DD || !VV || !X2 || !CC || !NC || !EX) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	ssx::compare_derive(regions, bins, DD, VV, X2, CC, NC, EX, mean_diff, std_err, z, chi2, exceed, coverage);
	return SSX_OK;
}

int ssh_compare_save_csv(const char* path, uint32_t regions, uint32_t bins, float lambda_min, float bin_width, const double* DD, const double* VV, const double* X2,
                         const uint64_t* CC, const uint64_t* NC, const uint64_t* EX) {
	if (!path || !DD || !VV || !X2 || !CC || !NC || !EX) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try { ssx::save_compare_csv(path, regions, bins, lambda_min, bin_width, DD, VV, X2, CC, NC, EX); return SSX_OK; }
	catch (const ssx::HostError& e) { return report(e); }
}

int ssh_delta_e_derive(uint32_t regions, const double* SUM, const double* SSQ, const float* MAX, const uint64_t* NF, const uint64_t* NX, const uint64_t* EX,
                       double* mean, double* rms, double* max, double* exceed, double* coverage) {
	if (!SUM || !SSQ || !MAX || !NF || !NX || !EX) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	ssx::delta_e_derive(regions, SUM, SSQ, MAX, NF, NX, EX, mean, rms, max, exceed, coverage);
	return SSX_OK;
}

int ssh_delta_e_save_csv(const char* path, uint32_t regions, const double* SUM, const double* SSQ, const float* MAX, const uint64_t* NF, const uint64_t* NX, const uint64_t* EX) {
	if (!path || !SUM || !SSQ || !MAX || !NF || !NX || !EX) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try { ssx::save_delta_e_csv(path, regions, SUM, SSQ, MAX, NF, NX, EX); return SSX_OK; }
	catch (const ssx::HostError& e) { return report(e); }
}

int ssh_develop_white(const float* weights, uint32_t bins, float lambda_min, float lambda_step, const ssh_spectrum_t* illuminant, double* out) {
	if (!weights || !out || (illuminant && !illuminant->samples)) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try {
		ssx::Spectrum e;
		if (illuminant) e = ssx::Spectrum(std::vector<float>(illuminant->samples, illuminant->samples + illuminant->n), illuminant->low, illuminant->high);
		ssx::develop_white(weights, bins, lambda_min, lambda_step, illuminant ? &e : nullptr, out);
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
	catch (const std::exception& e) { g_error = e.what(); return SSX_ERR_DATA; }
}

int ssh_develop_weights(const char* data_dir, int observer, const ssh_spectrum_t* responses, uint32_t channels, const ssh_spectrum_t* filter, const double* gain,
                        int space, uint32_t bins, float lambda_min, float lambda_step, float* weights, double* weights64) {
	if (!weights) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (space != SSH_SPACE_XYZ && space != SSH_SPACE_LRGB) { g_error = "ssh_develop_weights: space must be SSH_SPACE_XYZ or SSH_SPACE_LRGB"; return SSX_ERR_ARG; }
	if ((!responses || space == SSH_SPACE_LRGB) && !data_dir) { g_error = "ssh_develop_weights: the observer's tables need data_dir"; return SSX_ERR_ARG; }
	if (!responses && channels != 3) { g_error = "ssh_develop_weights: an observer has three channels"; return SSX_ERR_ARG; }
	try {
		std::unique_ptr<ssx::ColorData> color;
		if (!responses || space == SSH_SPACE_LRGB) color = std::make_unique<ssx::ColorData>(data_dir, observer);
		auto table = [](const ssh_spectrum_t& t) {
			if (!t.samples) throw ssx::HostError{ SSX_ERR_ARG, "a spectrum table without samples" };
			return ssx::Spectrum(std::vector<float>(t.samples, t.samples + t.n), t.low, t.high);
		};
		std::vector<ssx::Spectrum> r;
		if (responses) for (uint32_t c = 0; c < channels; ++c) r.push_back(table(responses[c]));
		else r = { color->std_obs_xbar, color->std_obs_ybar, color->std_obs_zbar };
		ssx::Spectrum g;
		if (filter) g = table(*filter);
		const std::vector<double> w = ssx::develop_weights(r, filter ? &g : nullptr, gain, space == SSH_SPACE_LRGB ? &color->matr_xyz_to_lrgb.m[0][0] : nullptr,
		                                                   bins, lambda_min, lambda_step);
		for (size_t i = 0; i < w.size(); ++i) { weights[i] = static_cast<float>(w[i]); if (weights64) weights64[i] = w[i]; }
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
	catch (const std::exception& e) { g_error = e.what(); return SSX_ERR_DATA; }
}

int ssh_relight_gain(const ssh_spectrum_t* from_spectrum, const ssh_spectrum_t* to_spectrum, uint32_t bins, float lambda_min, float lambda_step, double* gain) {
	if (!from_spectrum || !to_spectrum || !from_spectrum->samples || !to_spectrum->samples || !gain) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try {
		const ssx::Spectrum a(std::vector<float>(from_spectrum->samples, from_spectrum->samples + from_spectrum->n), from_spectrum->low, from_spectrum->high);
		const ssx::Spectrum b(std::vector<float>(to_spectrum->samples, to_spectrum->samples + to_spectrum->n), to_spectrum->low, to_spectrum->high);
		const std::vector<double> g = ssx::relight_gain(a, b, bins, lambda_min, lambda_step);
		memcpy(gain, g.data(), g.size() * sizeof(double));
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
	catch (const std::exception& e) { g_error = e.what(); return SSX_ERR_DATA; }
}

int ssh_optics_lens(uint32_t bins, float lambda_min, float lambda_step, double lambda_ref, double lateral, double sigma_ref, double axial, uint32_t max_radius,
                    float* scale_out, uint32_t* radius_out, float* taps_out) {
	if (!scale_out || !radius_out || !taps_out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (bins < 4u || bins > 64u || (bins & 3u)) { g_error = "ssh_optics_lens: bins must be a multiple of 4 up to 64"; return SSX_ERR_ARG; }
	if (max_radius > SSX_OPTICS_MAX_RADIUS) { g_error = "ssh_optics_lens: max_radius must be 0..12"; return SSX_ERR_ARG; }
	if (!std::isfinite(lambda_min) || !std::isfinite(lambda_step) || !(lambda_step > 0.0f)) { g_error = "ssh_optics_lens: lambda_min must be finite, lambda_step finite and positive"; return SSX_ERR_ARG; }
	if (!std::isfinite(lambda_ref) || !(lambda_ref > 0.0)) { g_error = "ssh_optics_lens: lambda_ref must be finite and positive"; return SSX_ERR_ARG; }
	if (!std::isfinite(lateral) || !std::isfinite(axial) || !std::isfinite(sigma_ref) || sigma_ref < 0.0) { g_error = "ssh_optics_lens: lateral and axial must be finite, sigma_ref finite and >= 0"; return SSX_ERR_ARG; }
	const uint32_t R = max_radius, K = 2u * R + 1u;
	const double width = static_cast<double>(lambda_step) / (bins / 4u);
	for (uint32_t b = 0; b < bins; ++b) {
		const double lc = static_cast<double>(lambda_min) + (b + 0.5) * width;
		const double u = (lc - lambda_ref) / lambda_ref;
		const float s = static_cast<float>(1.0 + lateral * u);
		if (!(s > 0.0f) || !std::isfinite(s)) { g_error = "ssh_optics_lens: the lateral coefficient gives bin " + std::to_string(b) + " a magnification that is not finite and > 0"; return SSX_ERR_ARG; }
		scale_out[b] = s;
		const double sd = sigma_ref * lc / lambda_ref, ax = axial * u;
		const double sigma = std::sqrt(sd * sd + ax * ax);
		for (uint32_t k = 0; k < K; ++k) taps_out[b * K + k] = 0.0f;
		radius_out[b] = 0u;
		if (sigma * sigma == 0.0) continue; // (sigma 0, or so small that its square underflows: no blur, not 0 / 0)
		const uint32_t r = static_cast<uint32_t>(std::fmin(static_cast<double>(R), std::ceil(3.0 * sigma)));
		radius_out[b] = r;
		double k[2u * SSX_OPTICS_MAX_RADIUS + 1u], total = 0.0;
		for (int d = -static_cast<int>(r); d <= static_cast<int>(r); ++d) k[d + static_cast<int>(r)] = std::exp(-static_cast<double>(d * d) / (2.0 * (sigma * sigma)));
		for (uint32_t t = 0; t < 2u * r + 1u; ++t) total = total + k[t];
		for (uint32_t t = 0; t < 2u * r + 1u; ++t) taps_out[b * K + (R - r) + t] = static_cast<float>(k[t] / total);
	}
	return SSX_OK;
}

int ssh_glare_plan(uint32_t width, uint32_t height, uint32_t radius, uint32_t* px, uint32_t* py) {
	if (!px || !py) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (width == 0u || height == 0u) { g_error = "ssh_glare_plan: width and height must be positive"; return SSX_ERR_ARG; }
	if (radius > SSX_GLARE_MAX_RADIUS) { g_error = "ssh_glare_plan: radius must be 0..256"; return SSX_ERR_ARG; }
	if (width > SSX_GLARE_MAX_EXTENT || height > SSX_GLARE_MAX_EXTENT) { g_error = "ssh_glare_plan: a padded extent would exceed 4096"; return SSX_ERR_ARG; }
	uint32_t x = 2u, y = 2u;
	while (x < width + 2u * radius) x <<= 1;
	while (y < height + 2u * radius) y <<= 1;
	if (x > SSX_GLARE_MAX_EXTENT || y > SSX_GLARE_MAX_EXTENT) { g_error = "ssh_glare_plan: a padded extent would exceed 4096"; return SSX_ERR_ARG; }
	*px = x; *py = y;
	return SSX_OK;
}

int ssh_glare_twiddles(uint32_t P, float* out) {
	if (!out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (P < 2u || P > SSX_GLARE_MAX_EXTENT || (P & (P - 1u))) { g_error = "ssh_glare_twiddles: P must be a power of two in 2..4096"; return SSX_ERR_ARG; }
	for (uint32_t m = 0; m < P / 2u; ++m) {
		const double x = (2.0 * 3.14159265358979323846 * static_cast<double>(m)) / static_cast<double>(P);
		out[2u * m] = static_cast<float>(std::cos(x));
		out[2u * m + 1u] = static_cast<float>(-std::sin(x));
	}
	out[0] = 1.0f; out[1] = 0.0f;
	if (P >= 4u) { out[2u * (P / 4u)] = 0.0f; out[2u * (P / 4u) + 1u] = -1.0f; }
	return SSX_OK;
}

namespace {

// in-place binary64 radix-2 FFT of n = 2^k values with stride `stride` (decimation in time, libm twiddles): ssh_glare_aperture's own
void glare_fft64(double* re, double* im, uint32_t n, size_t stride, const std::vector<double>& c, const std::vector<double>& s) {
	for (uint32_t i = 1, j = 0; i < n; ++i) {
		uint32_t bit = n >> 1;
		for (; j & bit; bit >>= 1) j ^= bit;
		j ^= bit;
		if (i < j) { std::swap(re[i * stride], re[j * stride]); std::swap(im[i * stride], im[j * stride]); }
	}
	for (uint32_t h = 1; h < n; h <<= 1) {
		const uint32_t step = n / (2u * h);
		for (uint32_t g = 0; g < n; g += 2u * h)
			for (uint32_t k = 0; k < h; ++k) {
				const double wr = c[k * step], wi = -s[k * step];
				double& ar = re[(g + k) * stride]; double& ai = im[(g + k) * stride];
				double& br = re[(g + k + h) * stride]; double& bi = im[(g + k + h) * stride];
				const double tr = wr * br - wi * bi, ti = wr * bi + wi * br;
				br = ar - tr; bi = ai - ti; ar = ar + tr; ai = ai + ti;
			}
	}
}

} // namespace

int ssh_glare_aperture(uint32_t bins, float lambda_min, float lambda_step, double lambda_ref, int blades, double rotation, double ring_px, double strength,
                       uint32_t radius, float* psf_out, uint8_t* on_out) {
	if (!psf_out || !on_out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (bins < 4u || bins > 64u || (bins & 3u)) { g_error = "ssh_glare_aperture: bins must be a multiple of 4 up to 64"; return SSX_ERR_ARG; }
	if (radius > SSX_GLARE_MAX_RADIUS) { g_error = "ssh_glare_aperture: radius must be 0..256"; return SSX_ERR_ARG; }
	if (!std::isfinite(lambda_min) || !(lambda_min > 0.0f) || !std::isfinite(lambda_step) || !(lambda_step > 0.0f)) { g_error = "ssh_glare_aperture: lambda_min and lambda_step must be finite and positive"; return SSX_ERR_ARG; }
	if (!std::isfinite(lambda_ref) || !(lambda_ref > 0.0)) { g_error = "ssh_glare_aperture: lambda_ref must be finite and positive"; return SSX_ERR_ARG; }
	if (!std::isfinite(rotation)) { g_error = "ssh_glare_aperture: rotation must be finite"; return SSX_ERR_ARG; }
	if (!std::isfinite(ring_px) || !(ring_px > 0.0)) { g_error = "ssh_glare_aperture: ring_px must be finite and positive"; return SSX_ERR_ARG; }
	if (!(strength >= 0.0) || !(strength <= 1.0)) { g_error = "ssh_glare_aperture: strength must be 0..1"; return SSX_ERR_ARG; }
	if (blades > 64) { g_error = "ssh_glare_aperture: at most 64 blades"; return SSX_ERR_ARG; }
	const uint32_t R = radius, K = 2u * R + 1u;
	const size_t KK = static_cast<size_t>(K) * K;
	for (uint32_t b = 0; b < bins; ++b) {
		on_out[b] = strength != 0.0;
		for (size_t k = 0; k < KK; ++k) psf_out[b * KK + k] = 0.0f;
		psf_out[b * KK + static_cast<size_t>(R) * K + R] = 1.0f;
	}
	if (strength == 0.0) return SSX_OK;
	constexpr uint32_t N = SSH_GLARE_GRID, SUB = SSH_GLARE_SUBSAMPLES;
	constexpr double A = SSH_GLARE_PUPIL, pi = 3.14159265358979323846;
	// the aperture: coverage of each cell by the polygon (circumradius A about the grid's centre), SUB x SUB samples per cell
	std::vector<double> re(static_cast<size_t>(N) * N, 0.0), im(static_cast<size_t>(N) * N, 0.0);
	const bool disc = blades < 3;
	std::vector<double> nx, ny;
	const double apothem = disc ? A : A * std::cos(pi / blades);
	for (int k = 0; !disc && k < blades; ++k) {
		const double t = rotation + (2.0 * k + 1.0) * pi / blades;
		nx.push_back(std::cos(t)); ny.push_back(std::sin(t));
	}
	const int lo = static_cast<int>(N / 2u) - static_cast<int>(A) - 2, hi = static_cast<int>(N / 2u) + static_cast<int>(A) + 2;
	for (int y = lo; y < hi; ++y)
		for (int x = lo; x < hi; ++x) {
			uint32_t inside = 0;
			for (uint32_t v = 0; v < SUB; ++v)
				for (uint32_t u = 0; u < SUB; ++u) {
					const double sx = (x + (u + 0.5) / SUB) - N / 2.0, sy = (y + (v + 0.5) / SUB) - N / 2.0;
					bool in = true;
					if (disc) in = sx * sx + sy * sy <= A * A;
					else for (size_t k = 0; k < nx.size() && in; ++k) in = sx * nx[k] + sy * ny[k] <= apothem;
					inside += in;
				}
			re[static_cast<size_t>(y) * N + x] = static_cast<double>(inside) / (SUB * SUB);
		}
	std::vector<double> c(N / 2u), s(N / 2u);
	for (uint32_t m = 0; m < N / 2u; ++m) { c[m] = std::cos(2.0 * pi * m / N); s[m] = std::sin(2.0 * pi * m / N); }
	for (uint32_t y = 0; y < N; ++y) glare_fft64(&re[static_cast<size_t>(y) * N], &im[static_cast<size_t>(y) * N], N, 1, c, s);
	for (uint32_t x = 0; x < N; ++x) glare_fft64(&re[x], &im[x], N, N, c, s);
	for (size_t k = 0; k < re.size(); ++k) re[k] = re[k] * re[k] + im[k] * im[k];             // the far-field intensity, frequency (fy, fx) at [fy mod N][fx mod N]
	auto at = [&re](int fy, int fx) { return re[static_cast<size_t>((fy + static_cast<int>(N)) % static_cast<int>(N)) * N + static_cast<size_t>((fx + static_cast<int>(N)) % static_cast<int>(N))]; };
	const double ring0 = SSH_GLARE_AIRY_ZERO * N / (2.0 * A);                                   // a disc's first dark ring, in frequency samples
	const double width = static_cast<double>(lambda_step) / (bins / 4u), limit = N / 2.0 - 1.0;
	std::vector<double> pat(KK);
	for (uint32_t b = 0; b < bins; ++b) {
		const double lc = static_cast<double>(lambda_min) + (b + 0.5) * width;
		const double kappa = (ring0 / ring_px) * (lambda_ref / lc);
		double total = 0.0;
		for (uint32_t j = 0; j < K; ++j)
			for (uint32_t i = 0; i < K; ++i) {
				const double fy = (static_cast<double>(j) - R) * kappa, fx = (static_cast<double>(i) - R) * kappa;
				double v = 0.0;
				if (std::fabs(fy) < limit && std::fabs(fx) < limit) {
					const double y0 = std::floor(fy), x0 = std::floor(fx), ty = fy - y0, tx = fx - x0;
					const int iy = static_cast<int>(y0), ix = static_cast<int>(x0);
					const double l = at(iy, ix) * (1.0 - tx) + at(iy, ix + 1) * tx, h = at(iy + 1, ix) * (1.0 - tx) + at(iy + 1, ix + 1) * tx;
					v = l * (1.0 - ty) + h * ty;
				}
				pat[static_cast<size_t>(j) * K + i] = v;
				total = total + v;
			}
		for (size_t k = 0; k < KK; ++k) {
			const double delta = k == static_cast<size_t>(R) * K + R ? 1.0 : 0.0;
			psf_out[b * KK + k] = static_cast<float>((1.0 - strength) * delta + strength * (pat[k] / total));
		}
	}
	return SSX_OK;
}

int ssh_sensor_bayer(const char* pattern, int method, uint32_t* cfa_out, float* taps_out) {
	if (!pattern || !cfa_out || !taps_out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (method != SSH_DEMOSAIC_BILINEAR && method != SSH_DEMOSAIC_MHC) { g_error = "ssh_sensor_bayer: method must be SSH_DEMOSAIC_BILINEAR or SSH_DEMOSAIC_MHC"; return SSX_ERR_ARG; }
	const std::string name(pattern);
	if (name != "RGGB" && name != "BGGR" && name != "GRBG" && name != "GBRG") { g_error = "ssh_sensor_bayer: pattern must be RGGB, BGGR, GRBG or GBRG"; return SSX_ERR_ARG; }
	uint32_t cfa[4];
	for (int k = 0; k < 4; ++k) cfa[k] = name[k] == 'R' ? 0u : (name[k] == 'G' ? 1u : 2u);
	const bool mhc = method == SSH_DEMOSAIC_MHC;
	for (int phase = 0; phase < 4; ++phase) {
		const uint32_t own = cfa[phase];
		for (uint32_t c = 0; c < 3u; ++c) {
			double k[5][5] = {};                                    // [dy + 2][dx + 2], in eighths
			auto at = [&](int dx, int dy) -> double& { return k[dy + 2][dx + 2]; };
			if (c == own) at(0, 0) = 8.0;
			else if (c == 1u) {                                      // G at an R or B site
				at(-1, 0) = at(1, 0) = at(0, -1) = at(0, 1) = 2.0;
				if (mhc) { at(0, 0) = 4.0; at(-2, 0) = at(2, 0) = at(0, -2) = at(0, 2) = -1.0; }
			} else if (own == 1u) {                                  // R or B at a G site: its sites are this row's neighbours, or this column's
				const bool in_row = cfa[phase ^ 1] == c;
				auto along = [&](int d) -> double& { return in_row ? at(d, 0) : at(0, d); };
				auto across = [&](int d) -> double& { return in_row ? at(0, d) : at(d, 0); };
				along(-1) = along(1) = 4.0;
				if (mhc) { at(0, 0) = 5.0; at(-1, -1) = at(1, -1) = at(-1, 1) = at(1, 1) = -1.0; along(-2) = along(2) = -1.0; across(-2) = across(2) = 0.5; }
			} else {                                                 // R at B, B at R
				at(-1, -1) = at(1, -1) = at(-1, 1) = at(1, 1) = 2.0;
				if (mhc) { at(0, 0) = 6.0; at(-2, 0) = at(2, 0) = at(0, -2) = at(0, 2) = -1.5; }
			}
			for (int t = 0; t < 25; ++t) taps_out[(phase * 3 + static_cast<int>(c)) * 25 + t] = static_cast<float>(k[t / 5][t % 5] / 8.0);
		}
	}
	for (int k = 0; k < 4; ++k) cfa_out[k] = cfa[k];
	return SSX_OK;
}

int ssh_sensor_exposure(double full_well, double white_level, uint32_t bits, double black, double read_e, float* out) {
	if (!out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (!std::isfinite(full_well) || !(full_well > 0.0)) { g_error = "ssh_sensor_exposure: full_well must be finite and positive"; return SSX_ERR_ARG; }
	if (!std::isfinite(white_level) || !(white_level > 0.0)) { g_error = "ssh_sensor_exposure: white_level must be finite and positive"; return SSX_ERR_ARG; }
	if (bits > 24u) { g_error = "ssh_sensor_exposure: bits must be 0..24 (a binary32 holds every integer up to 2^24)"; return SSX_ERR_ARG; }
	if (!std::isfinite(read_e) || read_e < 0.0) { g_error = "ssh_sensor_exposure: read_e must be finite and >= 0"; return SSX_ERR_ARG; }
	const double white = bits ? static_cast<double>((1u << bits) - 1u) : 0.0;
	if (!std::isfinite(black) || black < 0.0 || (bits && !(black < white))) { g_error = "ssh_sensor_exposure: black must be finite, >= 0 and below 2^bits - 1"; return SSX_ERR_ARG; }
	const double exposure = full_well / white_level;
	out[0] = static_cast<float>(exposure);
	out[1] = static_cast<float>(1.0 / exposure);
	out[2] = static_cast<float>(read_e * read_e);
	out[3] = bits ? static_cast<float>((white - black) / full_well) : 1.0f;
	out[4] = bits ? static_cast<float>(full_well / (white - black)) : 1.0f;
	out[5] = static_cast<float>(black);
	out[6] = static_cast<float>(white);
	for (int k = 0; k < 7; ++k) if (!std::isfinite(out[k])) { g_error = "ssh_sensor_exposure: a result is not finite in binary32"; return SSX_ERR_ARG; }
	return SSX_OK;
}

int ssh_sensor_ccm(const float* cam, const float* target, uint32_t bins, float* ccm_out) {
	if (!cam || !target || !ccm_out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (bins == 0u) { g_error = "ssh_sensor_ccm: bins must be positive"; return SSX_ERR_ARG; }
	double G[3][3] = {}, M[3][3] = {};
	for (int r = 0; r < 3; ++r)
		for (int c = 0; c < 3; ++c)
			for (uint32_t b = 0; b < bins; ++b) {
				G[r][c] = G[r][c] + static_cast<double>(cam[r * bins + b]) * static_cast<double>(cam[c * bins + b]);
				M[r][c] = M[r][c] + static_cast<double>(target[r * bins + b]) * static_cast<double>(cam[c * bins + b]);
			}
	double adj[3][3];                                               // the adjugate of the symmetric G: adj[r][c] = cofactor(c, r)
	for (int r = 0; r < 3; ++r)
		for (int c = 0; c < 3; ++c) {
			const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
			adj[r][c] = G[r1][c1] * G[r2][c2] - G[r1][c2] * G[r2][c1];
		}
	const double det = (G[0][0] * adj[0][0] + G[0][1] * adj[1][0]) + G[0][2] * adj[2][0];
	const double scale = G[0][0] * G[1][1] * G[2][2];               // Hadamard: det <= scale for a Gram matrix
	if (!std::isfinite(det) || !std::isfinite(scale) || !(det > 1e-12 * scale)) { g_error = "ssh_sensor_ccm: cam * cam^T is singular (the three curves are not linearly independent over these bins)"; return SSX_ERR_ARG; }
	for (int r = 0; r < 3; ++r)
		for (int c = 0; c < 3; ++c) {
			const double v = ((M[r][0] * adj[0][c] + M[r][1] * adj[1][c]) + M[r][2] * adj[2][c]) / det;
			ccm_out[r * 3 + c] = static_cast<float>(v);
			if (!std::isfinite(ccm_out[r * 3 + c])) { g_error = "ssh_sensor_ccm: a result is not finite in binary32"; return SSX_ERR_ARG; }
		}
	return SSX_OK;
}

int ssh_sensor_standin_curve(uint32_t channel, float* samples, float* low, float* high) {
	if (!samples || !low || !high) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (channel > 2u) { g_error = "ssh_sensor_standin_curve: channel must be 0..2"; return SSX_ERR_ARG; }
	const double peak = channel == 0u ? 600.0 : (channel == 1u ? 540.0 : 460.0);
	for (uint32_t k = 0; k < SSH_SENSOR_STANDIN_SAMPLES; ++k) {
		const double t = ((380.0 + 5.0 * k) - peak) / 35.0;
		samples[k] = static_cast<float>(std::exp(-0.5 * (t * t)));
	}
	*low = 380.0f; *high = 730.0f;
	return SSX_OK;
}

int ssh_scene_vfov(const ssh_scene* scene, float* vfov_deg) {
	if (!scene || !vfov_deg) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	*vfov_deg = scene->scene->camera.vfov_deg;
	return SSX_OK;
}

int ssh_defocus_thin_lens(float vfov_deg, uint32_t height, uint32_t bins, float lambda_min, float lambda_step, double aperture, double focus_distance, double axial,
                          double lambda_ref, float* gain_out, float* focus_out) {
	if (!gain_out || !focus_out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (!(vfov_deg > 0.0f) || !(vfov_deg < 180.0f)) { g_error = "ssh_defocus_thin_lens: vfov_deg must lie in (0, 180)"; return SSX_ERR_ARG; }
	if (!std::isfinite(lambda_min) || !std::isfinite(lambda_step) || !(lambda_step > 0.0f)) { g_error = "ssh_defocus_thin_lens: lambda_min must be finite, lambda_step finite and positive"; return SSX_ERR_ARG; }
	if (bins < 4u || bins > 64u || (bins & 3u)) { g_error = "ssh_defocus_thin_lens: bins must be a multiple of 4 up to 64"; return SSX_ERR_ARG; }
	if (height == 0u) { g_error = "ssh_defocus_thin_lens: height must be positive"; return SSX_ERR_ARG; }
	if (!std::isfinite(aperture) || aperture < 0.0) { g_error = "ssh_defocus_thin_lens: aperture must be finite and >= 0"; return SSX_ERR_ARG; }
	if (!std::isfinite(focus_distance) || !(focus_distance > 0.0)) { g_error = "ssh_defocus_thin_lens: focus_distance must be finite and positive"; return SSX_ERR_ARG; }
	if (!std::isfinite(axial)) { g_error = "ssh_defocus_thin_lens: axial must be finite"; return SSX_ERR_ARG; }
	if (!std::isfinite(lambda_ref) || !(lambda_ref > 0.0)) { g_error = "ssh_defocus_thin_lens: lambda_ref must be finite and positive"; return SSX_ERR_ARG; }
	const double vfov = static_cast<double>(vfov_deg) * (3.14159265358979323846 / 180.0);
	const double v_px = (static_cast<double>(height) / 2.0) / std::tan(vfov / 2.0);
	const float K = static_cast<float>(0.5 * aperture * v_px);
	if (!std::isfinite(K)) { g_error = "ssh_defocus_thin_lens: the aperture gives a gain that is not finite"; return SSX_ERR_ARG; }
	*gain_out = K;
	const double width = static_cast<double>(lambda_step) / (bins / 4u);
	for (uint32_t b = 0; b < bins; ++b) {
		const double lc = static_cast<double>(lambda_min) + (b + 0.5) * width;
		const double u = (lc - lambda_ref) / lambda_ref;
		const double f = 1.0 / focus_distance + axial * u;
		focus_out[b] = static_cast<float>(f > 0.0 ? f : 0.0);
		if (!std::isfinite(focus_out[b])) { g_error = "ssh_defocus_thin_lens: bin " + std::to_string(b) + " gets an inverse focus distance that is not finite"; return SSX_ERR_ARG; }
	}
	return SSX_OK;
}

namespace {
float display_frombits(uint32_t u) { float v; memcpy(&v, &u, sizeof v); return v; }
uint32_t display_bits(float v) { uint32_t u; memcpy(&u, &v, sizeof u); return u; }
// percentile(k, p) of ssx_host.h on one quantity's histogram
double meter_percentile(const uint32_t* h, double p) {
	uint64_t N = 0;
	for (uint32_t k = 0; k < SSX_METER_KEYS; ++k) N += h[k];
	if (!N) return 0.0;
	double rank = std::ceil(p * static_cast<double>(N));
	rank = std::min(std::max(rank, 1.0), static_cast<double>(N));
	uint64_t cum = 0;
	for (uint32_t k = 0; k < SSX_METER_KEYS; ++k) {
		cum += h[k];
		if (static_cast<double>(cum) >= rank) return static_cast<double>(display_frombits(k << 19));
	}
	return 0.0;
}
double meter_mean(const uint32_t* h) {
	uint64_t N = 0; double s = 0.0;
	for (uint32_t k = 0; k < 4080u; ++k) if (h[k]) { N += h[k]; s += static_cast<double>(h[k]) * static_cast<double>(display_frombits((k << 19) + (1u << 18))); }
	return N ? s / static_cast<double>(N) : 0.0;
}
double srgb_oetf(double v) { return v <= 0.0031308 ? 12.92 * v : 1.055 * std::pow(v, 1.0 / 2.4) - 0.055; }
double hable(double x) { const double A = 0.15, B = 0.50, C = 0.10, D = 0.20, E = 0.02, F = 0.30; return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - E / F; }
} // namespace

int ssh_meter_derive(const uint32_t* hist, const uint32_t* special, double key_value, double white_percentile, const double* percentiles, uint32_t n_percentiles,
                     float* percentile_out, float* out) {
	if (!hist || !special || !out || (n_percentiles && (!percentiles || !percentile_out))) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (!std::isfinite(key_value) || !(key_value > 0.0)) { g_error = "ssh_meter_derive: key_value must be finite and positive"; return SSX_ERR_ARG; }
	if (!(white_percentile >= 0.0) || !(white_percentile <= 1.0)) { g_error = "ssh_meter_derive: white_percentile must lie in 0..1"; return SSX_ERR_ARG; }
	for (uint32_t i = 0; i < n_percentiles; ++i)
		if (!(percentiles[i] >= 0.0) || !(percentiles[i] <= 1.0)) { g_error = "ssh_meter_derive: percentiles[" + std::to_string(i) + "] must lie in 0..1"; return SSX_ERR_ARG; }
	for (uint32_t k = 0; k < 4u; ++k)
		for (uint32_t i = 0; i < n_percentiles; ++i) percentile_out[k * n_percentiles + i] = static_cast<float>(meter_percentile(hist + k * SSX_METER_KEYS, percentiles[i]));
	const uint32_t* const hy = hist + 3u * SSX_METER_KEYS;
	uint64_t N = 0, S = 0;
	for (uint32_t k = 0; k < SSX_METER_KEYS; ++k) { N += hy[k]; S += static_cast<uint64_t>(hy[k]) * (2u * k + 1u); }
	double log_average = 0.0;
	if (N) {
		const uint64_t q = S / (2u * N);
		const double f = static_cast<double>(S % (2u * N)) / static_cast<double>(2u * N);
		log_average = std::ldexp(1.0 + (static_cast<double>(q & 15u) + f) / 16.0, static_cast<int>(q >> 4) - 127);
	}
	const double exposure = log_average > 0.0 ? key_value / log_average : 1.0;
	const double white = meter_percentile(hy, white_percentile);
	for (uint32_t i = 0; i < SSH_METER_OUT; ++i) out[i] = 0.0f;
	out[SSH_METER_LOG_AVERAGE] = static_cast<float>(log_average);
	out[SSH_METER_EXPOSURE] = static_cast<float>(exposure);
	out[SSH_METER_WHITE] = static_cast<float>(white);
	out[SSH_METER_WHITE_EXPOSED] = static_cast<float>(white * exposure);
	const float kf = static_cast<float>(key_value);
	out[SSH_METER_PIVOT] = std::isnormal(kf) ? static_cast<float>(static_cast<int32_t>(display_bits(kf) >> 7) - 8323072) * 0x1p-16f : 0.0f;
	double mean[3], patch[3];
	for (uint32_t c = 0; c < 3u; ++c) { mean[c] = meter_mean(hist + c * SSX_METER_KEYS); patch[c] = meter_percentile(hist + c * SSX_METER_KEYS, white_percentile); }
	for (uint32_t c = 0; c < 3u; ++c) {
		out[SSH_METER_GREY + c] = static_cast<float>(mean[1] > 0.0 && mean[c] > 0.0 ? mean[1] / mean[c] : 1.0);
		out[SSH_METER_PATCH + c] = static_cast<float>(patch[1] > 0.0 && patch[c] > 0.0 ? patch[1] / patch[c] : 1.0);
	}
	out[SSH_METER_COUNT] = static_cast<float>(N);
	for (uint32_t i = 0; i < SSH_METER_OUT; ++i) if (!std::isfinite(out[i])) { g_error = "ssh_meter_derive: a result is not finite in binary32"; return SSX_ERR_ARG; }
	return SSX_OK;
}

int ssh_tone_curve(int kind, double white, float lo, float hi, uint32_t shift, float* curve_out, uint32_t curve_len) {
	if (!curve_out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	if (kind != SSH_TONE_CLIP && kind != SSH_TONE_REINHARD && kind != SSH_TONE_FILMIC) { g_error = "ssh_tone_curve: kind must be SSH_TONE_CLIP, SSH_TONE_REINHARD or SSH_TONE_FILMIC"; return SSX_ERR_ARG; }
	if (!std::isfinite(white) || !(white > 0.0)) { g_error = "ssh_tone_curve: white must be finite and positive"; return SSX_ERR_ARG; }
	if (shift < 12u || shift > 23u) { g_error = "ssh_tone_curve: shift must be 12..23"; return SSX_ERR_ARG; }
	if (!std::isnormal(lo) || !std::isnormal(hi) || !(lo > 0.0f) || !(hi >= lo)) { g_error = "ssh_tone_curve: lo and hi must be positive normal numbers, lo <= hi"; return SSX_ERR_ARG; }
	const uint32_t len = ((display_bits(hi) - display_bits(lo)) >> shift) + 2u;
	if (len > SSX_TONE_MAX_CURVE || curve_len != len) { g_error = "ssh_tone_curve: lo, hi and shift define a curve_len of " + std::to_string(len) + " (at most " + std::to_string(SSX_TONE_MAX_CURVE) + ")"; return SSX_ERR_ARG; }
	const double hw = hable(white);
	for (uint32_t idx = 0; idx < len; ++idx) {
		const uint32_t u = display_bits(lo) + (idx << shift);
		const double x = u < 0x7F800000u ? static_cast<double>(display_frombits(u)) : static_cast<double>(hi);
		double t = x;
		if (kind == SSH_TONE_REINHARD) t = x * (1.0 + x / (white * white)) / (1.0 + x);
		else if (kind == SSH_TONE_FILMIC) t = hable(2.0 * x) / hw;
		curve_out[idx] = static_cast<float>(srgb_oetf(std::min(std::max(t, 0.0), 1.0)));
	}
	return SSX_OK;
}

int ssh_display_matrix(const char* data_dir, int observer, float* out) {
	if (!data_dir || !out) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try {
		const ssx::ColorData color(data_dir, observer);
		for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) out[3 * r + c] = color.matr_xyz_to_lrgb.m[c][r];
		return SSX_OK;
	} catch (const ssx::HostError& e) { return report(e); }
	catch (const std::exception& e) { g_error = e.what(); return SSX_ERR_DATA; }
}

int ssh_emitter_spectrum(const ssx_scene_desc* desc, uint32_t* spectrum) {
	if (!desc || !spectrum) { g_error = "NULL argument"; return SSX_ERR_ARG; }
	try { *spectrum = ssx::emitter_spectrum(*desc); return SSX_OK; }
	catch (const ssx::HostError& e) { return report(e); }
}

int ssh_color_values(const ssh_scene* scene, const char* name, float* out, int capacity) {
	if (!scene || !name || !out) return SSX_ERR_ARG;
	const ssx::ColorData& c = *scene->color;
	const float* src = nullptr; int n = 0;
	if (!strcmp(name, "D65_rad_XYZ")) { src = c.D65_rad_XYZ; n = 3; }
	else if (!strcmp(name, "xyz_to_lrgb")) { src = &c.matr_xyz_to_lrgb.m[0][0]; n = 9; }
	else if (!strcmp(name, "lrgb_to_xyz")) { src = &c.matr_lrgb_to_xyz.m[0][0]; n = 9; }
	else return SSX_ERR_ARG;
	if (capacity < n) return SSX_ERR_ARG;
	memcpy(out, src, sizeof(float) * (size_t)n);
	return n;
}

} // extern "C"

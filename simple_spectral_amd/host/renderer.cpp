#include "renderer.hpp"

#include "checkpoint.hpp"
#include "develop.hpp"
#include "image_io.hpp"
#include "../../include/ssx_host.h"

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <thread>

namespace ssx {

Framebuffer::Framebuffer(const size_t r[2]) : res{ r[0], r[1] }, pixels_(4 * r[0] * r[1]) {
	for (size_t j = 0; j < res[1]; ++j) for (size_t i = 0; i < res[0]; ++i) {
		const float v = (((i / 8) ^ (j / 8)) % 2 == 0) ? 0.7f : 0.3f;
		float* p = (*this)(i, j);
		p[0] = p[1] = p[2] = v; p[3] = 1.0f;
	}
}
void Framebuffer::save(const std::string& path) const { save_image(path, pixels_.data(), res[0], res[1]); }

// The C ABI, resolved from libssx_hip.so at run time so that libssx_host.so itself has no HIP
// dependency (it must load on machines without a GPU for table/scene/image work).
// Every entry point the host calls, named once: X(name) stands for ssx_<name> of include/ssx.h.  The member's type is the header's own declaration
// (decltype of a declared function does not use it: no link dependency), so a prototype that changes there is a compile error at the call here.
#define SSX_HOST_API(X) \
	X(create) X(destroy) X(upload_scene) X(render_start) X(render_stop) X(is_rendering) X(progress) X(render_wait) X(last_error) \
	X(device_framebuffer) X(device_index) X(read_framebuffer) X(accumulate_peer) X(done_spp) X(done_tiles) X(reduce_rccl) \
	X(render_continue) X(sums_export) X(sums_import) X(set_noise_estimate) X(noise_info) \
	X(set_spectral_bins) X(spectral_read) X(spectral_import) X(set_spectral_moments) X(spectral_variance) X(spectral_moments_import) X(spectral_probe) X(probe_arrays) X(spectral_noise) X(spectral_noise_reduce) X(spectral_compare) X(spectral_compare_arrays) X(delta_e_images) X(spectral_delta_e) \
	X(guides) X(denoise_images) X(denoise) X(denoise_channels) X(denoise_spectral) \
	X(develop_images) X(spectral_develop) X(albedo_bins) X(denoise_spectral_demod) X(spectral_develop_demod) X(optics_images) X(spectral_develop_optics) X(defocus_images) X(spectral_develop_lens) X(sensor_images) X(demosaic_images) X(spectral_develop_sensor) X(glare_images) X(spectral_develop_glare) \
	X(meter_images) X(local_images) X(tone_images)

struct Renderer::Api {
	void* handle = nullptr;
#define X(name) decltype(&::ssx_##name) name = nullptr;
	SSX_HOST_API(X)
#undef X

	explicit Api(const std::string& path) {
		handle = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
		if (!handle) throw HostError{ SSX_ERR_DEVICE, std::string("cannot load the HIP library (no CPU fallback exists): ") + dlerror() };
		auto sym = [&](const char* name) {
			void* p = dlsym(handle, name);
			if (!p) throw HostError{ SSX_ERR_DEVICE, std::string("libssx_hip.so lacks symbol ") + name };
			return p;
		};
		// one interface version on both sides of the boundary (include/ssx.h: what changed between versions)
		const int abi = reinterpret_cast<decltype(&::ssx_abi_version)>(sym("ssx_abi_version"))();
		if (abi != SSX_ABI_VERSION) throw HostError{ SSX_ERR_DEVICE, "libssx_hip.so implements ABI version " + std::to_string(abi) + ", this host was built against version " + std::to_string(SSX_ABI_VERSION) + " (include/ssx.h)" };
#define X(name) name = reinterpret_cast<decltype(name)>(sym("ssx_" #name));
		SSX_HOST_API(X)
#undef X
	}
	~Api() { if (handle) dlclose(handle); }
};

namespace {
std::string default_hip_library() {
	Dl_info info;
	if (dladdr(reinterpret_cast<void*>(&default_hip_library), &info) && info.dli_fname) {
		std::string self = info.dli_fname;
		const size_t slash = self.rfind('/');
		return (slash == std::string::npos ? std::string(".") : self.substr(0, slash)) + "/libssx_hip.so";
	}
	return "libssx_hip.so";
}
bool file_exists(const std::string& p) { return std::ifstream(p).good(); }

// Scene selection and its warnings (src/renderer.cpp:17-38, EXPLICIT_LIGHT_SAMPLING build)
void check_scene_name(const Renderer::Options& options) {
	if (options.scene_name == "plane-srgb") {
		if (options.explicit_light_sampling) std::fprintf(stderr, "Warning: Plane converges much faster without explicit light sampling!  (See \"stdafx.hpp\" to disable.)\n");
	} else if (options.scene_name == "cornell" || options.scene_name == "cornell-srgb") {
		if (!options.explicit_light_sampling) std::fprintf(stderr, "Warning: Cornell converges much faster with explicit light sampling!  (See \"stdafx.hpp\" to enable.)\n");
	} else {
		std::fprintf(stderr, "Unrecognized scene \"%s\"!  (Supported scenes: \"cornell\", \"cornell-srgb\", \"plane-srgb\")\n", options.scene_name.c_str());
		throw HostError{ -3, "Unrecognized scene" };
	}
}

// The parameter structs of the C ABI from the host's, each in this one place.  demodulated: the mode's filter runs with a zero albedo guide, which sigma_a
// cannot weigh -- any valid value serves, and the library's own demodulated calls take 1 as well.
ssx_denoise_params to_abi(const Renderer::DenoiseParams& p, bool demodulated = false) {
	ssx_denoise_params dp{};
	dp.struct_size = sizeof dp; dp.levels = p.levels; dp.sigma_l = p.sigma_l; dp.sigma_a = demodulated ? 1.0f : p.sigma_a;
	return dp;
}
ssx_demod_params to_abi(const Renderer::DemodParams& p) {
	ssx_demod_params dm{};
	dm.struct_size = sizeof dm; dm.supersample = p.supersample; dm.albedo_floor = p.albedo_floor;
	return dm;
}

// ---- The several-device route of denoise_spectral on host arrays: include/ssx.h's formulas restated, every operation in the header's type and order (the tests
// hold them against the one-device calls bit for bit).  pixels x B bins, M = B / 4 count channels, E = B + M filter channels.

// e0: the channels the filter takes -- per-bin sums and sample counts over the sample count n, divided in binary64 and rounded to binary32 once
std::vector<float> spectral_channels(const std::vector<double>& sums, const std::vector<uint32_t>& counts, size_t pixels, size_t B, double n) {
	const size_t M = B / 4, E = B + M;
	std::vector<float> e0(pixels * E);
	for (size_t p = 0; p < pixels; ++p) {
		for (size_t b = 0; b < B; ++b) e0[p * E + b] = static_cast<float>(sums[p * B + b] / n);
		for (size_t m = 0; m < M; ++m) e0[p * E + B + m] = static_cast<float>(static_cast<double>(counts[p * M + m]) / n);
	}
	return e0;
}

// What DEMODULATE leaves for REMODULATE: the albedo bins rho [pixels][B], the floored channel albedo rc [pixels][3], and which pixels were divided at all.
struct Demodulation {
	float floor;
	std::vector<float> rho, rc;
	std::vector<uint8_t> valid;
	float floored(float r) const { return r > floor ? r : floor; }
};

// The denominators of the channel albedo: the develop's accumulation of all ones over each row of weights_xyz [3][B].
void channel_denominators(const std::vector<float>& wc, size_t B, float den[3]) {
	for (size_t c = 0; c < 3; ++c) {
		volatile float acc = 0.0f;
		for (size_t b = 0; b < B; ++b) acc = acc + wc[c * B + b];
		den[c] = acc;
		if (!(den[c] > 0.0f)) throw HostError{ SSX_ERR_ARG, "denoise_spectral: a row of weights_xyz does not sum to a positive denominator" };
	}
}

// DEMODULATE, in binary32.  d.rho holds the albedo bins and d.rc their develop by weights_xyz (not yet normalised); bins (of e0), image and variance of
// every pixel with a finite image and variance are divided by the floored albedo -- the others pass through as they are and stay out of REMODULATE.
void demodulate(Demodulation& d, const float den[3], size_t B, std::vector<float>& e0, std::vector<float>& image, std::vector<float>& var) {
	const size_t pixels = var.size(), E = B + B / 4;
	d.valid.resize(pixels);
	for (size_t p = 0; p < pixels; ++p) {
		for (size_t c = 0; c < 3; ++c) d.rc[p * 3 + c] = d.floored(d.rc[p * 3 + c] / den[c]);
		d.valid[p] = std::isfinite(image[p * 4]) && std::isfinite(image[p * 4 + 1]) && std::isfinite(image[p * 4 + 2]) && std::isfinite(var[p]);
		if (!d.valid[p]) continue;
		for (size_t b = 0; b < B; ++b) e0[p * E + b] = e0[p * E + b] / d.floored(d.rho[p * B + b]);
		for (size_t c = 0; c < 3; ++c) image[p * 4 + c] = image[p * 4 + c] / d.rc[p * 3 + c];
		var[p] = var[p] / (d.rc[p * 3 + 1] * d.rc[p * 3 + 1]);
	}
}

// The filtered bins: the ratio of the filtered per-bin sums to the filtered counts of their sub-bin (0 where nothing was counted); d (the demodulated mode):
// times the floored albedo bin, REMODULATE -- and the filtered image `out` times the channel albedo.
std::vector<float> ratio(const std::vector<float>& eL, size_t pixels, size_t B, const Demodulation* d, std::vector<float>& out) {
	const size_t M = B / 4, E = B + M;
	std::vector<float> mean(pixels * B);
	for (size_t p = 0; p < pixels; ++p) for (size_t b = 0; b < B; ++b) {
		const float den = eL[p * E + B + b % M];
		const float r = d && d->valid[p] ? d->floored(d->rho[p * B + b]) : 1.0f;
		mean[p * B + b] = den > 0.0f ? (d ? (eL[p * E + b] / den) * r : eL[p * E + b] / den) : 0.0f;
	}
	if (d) for (size_t p = 0; p < pixels; ++p) if (d->valid[p]) for (size_t c = 0; c < 3; ++c) out[p * 4 + c] = out[p * 4 + c] * d->rc[p * 3 + c];
	return mean;
}
} // namespace

Renderer::Renderer(const Options& opts) : options(opts), framebuffer(opts.res), xyza(4 * opts.res[0] * opts.res[1], 0.0f) {
	check_scene_name(options);
	color = std::make_unique<ColorData>(options.data_dir, options.observer);
	Texture tex;
	const Texture* texp = nullptr;
	if (options.scene_name != "cornell") {
		std::string path = options.texture_path;
		if (path.empty()) { // the reference opens the 4096^2 blob; fall back to its own listed alternative
			path = options.data_dir + "/scenes/crystal-lizard-4096.png";
			if (!file_exists(path)) path = options.data_dir + "/scenes/crystal-lizard-512.png";
		}
		tex = load_texture(path);
		texp = &tex;
	}
	if (options.rgb_mode) {
		color->rgb_output_transform = true;
	} else if (options.uplift == SSX_UPLIFT_JH) {
		const std::string path = options.jh_coeff_path.empty() ? options.data_dir + "/jakob-and-hanika-2019-srgb.coeff" : options.jh_coeff_path;
		try { jh = std::make_unique<JHModel>(jh_load(path)); }
		catch (const HostError&) { // the authors' table is not in the repository: fit our own once and keep it
			std::fprintf(stderr, "Fitting Jakob-Hanika coefficients (\"%s\" not found) ...\n", path.c_str());
			jh = std::make_unique<JHModel>(jh_optimize(*color, 64));
			try { jh_save(*jh, path); } catch (const HostError&) {}
		}
	} else if (options.uplift == SSX_UPLIFT_MENG) {
		meng = std::make_unique<MengGrid>(meng_load(options.meng_grid_path.empty() ? options.data_dir + "/meng-et-al-2015-grid.bin" : options.meng_grid_path));
		color->meng_output_transform = true;
	} else if (options.uplift != SSX_UPLIFT_OURS) {
		throw HostError{ -3, "unsupported uplift variant" };
	}
	scene = std::make_unique<Scene>(*color, options.scene_name, options.data_dir, texp, options.light_scale, jh.get(), options.explicit_light_sampling, meng.get(), options.rgb_mode);

	api_ = std::make_unique<Api>(options.hip_library.empty() ? default_hip_library() : options.hip_library);
	const int n = options.gpus < 1 ? 1 : options.gpus;
	// SSX_TEST_ONE_GPU=1: plumbing test of the multi-device path on a 1-GPU box (all contexts on device 0)
	const char* one_gpu = std::getenv("SSX_TEST_ONE_GPU");
	for (int d = 0; d < n; ++d) {
		ssx_ctx* ctx = nullptr;
		int rc = api_->create((one_gpu && *one_gpu == '1') ? 0 : d, &ctx);
		if (rc) throw HostError{ rc, std::string("ssx_create: ") + api_->last_error(nullptr) };
		ctxs_.push_back(ctx);
		rc = api_->upload_scene(ctx, &scene->desc());
		if (rc) throw HostError{ rc, std::string("ssx_upload_scene: ") + api_->last_error(ctx) };
	}
}

Renderer::~Renderer() {
	for (ssx_ctx* c : ctxs_) api_->destroy(c);
}

ssx_render_params Renderer::params_for_(size_t d, size_t spp, size_t spp_per_launch) const {
	ssx_render_params p{};
	p.struct_size = sizeof p;
	p.width = w32_(); p.height = h32_();
	p.spp = static_cast<uint32_t>(spp);
	p.indirect_only = options.indirect_only ? 1u : 0u;
	p.no_explicit_light_sampling = options.explicit_light_sampling ? 0u : 1u;
	p.no_flat_field_correction = options.flat_field_correction ? 0u : 1u;
	p.tile_first = static_cast<uint32_t>(d); p.tile_stride = static_cast<uint32_t>(ctxs_.size());
	p.tile_skew = ctxs_.size() > 1 ? 1u : 0u; // several devices: diagonals instead of vertical stripes of the image (include/ssx.h)
	p.spp_per_launch = static_cast<uint32_t>(spp_per_launch);
	p.tile_major = options.tile_major ? 1u : 0u;
	p.seed = options.seed;
	p.libm = options.libm;
	return p;
}

// whose pixels device d's arrays hold: the description sums_owner / merge_owned (host/checkpoint.hpp) decide by
ssx_sums_info_t Renderer::owner_(size_t d) const {
	const ssx_render_params p = params_for_(d, 1, 0); // (what the devices rendered with)
	ssx_sums_info_t o{};
	o.struct_size = sizeof o; o.width = p.width; o.height = p.height;
	o.tile_first = p.tile_first; o.tile_stride = p.tile_stride; o.tile_skew = p.tile_skew;
	return o;
}

void Renderer::check_(int rc, const char* what, ssx_ctx* c) const {
	if (rc) throw HostError{ rc, std::string(what) + ": " + api_->last_error(c) };
}

void Renderer::start_(size_t spp, size_t spp_per_launch) {
	time_start_ = std::chrono::steady_clock::now();
	for (size_t d = 0; d < ctxs_.size(); ++d) {
		const ssx_render_params p = params_for_(d, spp, spp_per_launch);
		check_(api_->render_start(ctxs_[d], &p), "ssx_render_start", ctxs_[d]);
	}
	started_ = need_join_ = true;
	expected_spp_ = spp;
}

void Renderer::render_start() { start_(options.spp, options.spp_per_launch); }

// Starts ssx_render_continue on every (context, samples more) pair; should one refuse, the ones already started are stopped and joined
// before the error leaves (no worker is left behind unjoined).
void Renderer::continue_each_(const std::vector<std::pair<ssx_ctx*, uint32_t>>& more) {
	for (size_t n = 0; n < more.size(); ++n) {
		const int rc = api_->render_continue(more[n].first, more[n].second);
		if (!rc) continue;
		const std::string why = std::string("ssx_render_continue: ") + api_->last_error(more[n].first);
		for (size_t b = 0; b < n; ++b) { api_->render_stop(more[b].first); (void)api_->render_wait(more[b].first, nullptr); }
		throw HostError{ rc, why };
	}
}

// the devices that are short of `target` render up to it (blocking)
void Renderer::continue_to_(size_t target) {
	std::vector<std::pair<ssx_ctx*, uint32_t>> more;
	for (ssx_ctx* c : ctxs_) {
		const size_t mine = api_->done_spp(c);
		if (mine < target) more.emplace_back(c, static_cast<uint32_t>(target - mine));
	}
	continue_each_(more);
	for (const auto& m : more) check_(api_->render_wait(m.first, nullptr), "ssx_render_wait", m.first);
}

void Renderer::level_devices() {
	wait_workers_();
	size_t top = 0;
	for (ssx_ctx* c : ctxs_) { const size_t n = api_->done_spp(c); if (n > top) top = n; }
	continue_to_(top);
}

void Renderer::render_continue(size_t spp) {
	level_devices(); // devices that stopped at different counts: the laggards catch up first, then all render `spp` more
	const size_t done = done_spp();
	std::vector<std::pair<ssx_ctx*, uint32_t>> more;
	for (ssx_ctx* c : ctxs_) more.emplace_back(c, static_cast<uint32_t>(spp));
	continue_each_(more);
	started_ = need_join_ = true;
	expected_spp_ = done + spp;
}

size_t Renderer::done_spp() const {
	size_t done = SIZE_MAX;
	for (ssx_ctx* c : ctxs_) { const size_t n = api_->done_spp(c); if (n < done) done = n; }
	return ctxs_.empty() ? 0 : done;
}

void Renderer::wait_workers_() {
	if (!need_join_) return;
	need_join_ = false;
	for (ssx_ctx* c : ctxs_) check_(api_->render_wait(c, nullptr), "ssx_render_wait", c);
}

void Renderer::set_noise_estimate(bool on) {
	for (ssx_ctx* c : ctxs_) check_(api_->set_noise_estimate(c, on ? 1 : 0), "ssx_set_noise_estimate", c);
}

double Renderer::noise(std::vector<double>* v_map) {
	wait_workers_();
	const size_t pixels = options.res[0] * options.res[1];
	double total[3] = { 0.0, 0.0, 0.0 };
	std::vector<double> v(v_map ? pixels : 0);
	if (v_map) v_map->assign(pixels, 0.0);
	for (ssx_ctx* c : ctxs_) { // the ranks' partial sums add up; every pixel's v is nonzero on its owner alone
		double s[4];
		check_(api_->noise_info(c, v_map ? v.data() : nullptr, s), "ssx_noise_info", c);
		for (int k = 0; k < 3; ++k) total[k] += s[k];
		if (v_map) for (size_t p = 0; p < pixels; ++p) (*v_map)[p] += v[p];
	}
	return std::sqrt(total[0] / total[2]) / (total[1] / total[2]);
}

void Renderer::set_spectral_bins(size_t bins) {
	wait_workers_();
	for (ssx_ctx* c : ctxs_) check_(api_->set_spectral_bins(c, static_cast<uint32_t>(bins)), "ssx_set_spectral_bins", c);
	spectral_bins_ = bins;
	if (!bins) spectral_moments_ = false; // (the library switches the moments off with the bins)
}

// One loop over the contexts for every reader of the bins: ssx_spectral_read on each, the shares merged by ownership into whichever of the three arrays are
// asked for (sized here) -- every pixel from the device that owns it, bit for bit (merge_owned: the one merge by ownership mask).  Returns device 0's info.
// The raw sums mean something under ONE sample count only: with `sums` the devices must be level (level_devices), and devices that are not are refused.
ssx_spectral_info_t Renderer::gather_bins_(std::vector<float>* mean, std::vector<double>* sums, std::vector<uint32_t>* counts) {
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_, M = B / 4;
	if (mean) mean->assign(pixels * B, 0.0f);
	if (sums) sums->assign(pixels * B, 0.0);
	if (counts) counts->assign(pixels * M, 0u);
	std::vector<float> part_mean(mean ? pixels * B : 0);
	std::vector<double> part_sums(sums ? pixels * B : 0);
	std::vector<uint32_t> part_counts(counts ? pixels * M : 0);
	ssx_spectral_info_t first{};
	for (size_t d = 0; d < ctxs_.size(); ++d) {
		ssx_spectral_info_t info{};
		check_(api_->spectral_read(ctxs_[d], &info, mean ? part_mean.data() : nullptr, sums ? part_sums.data() : nullptr, counts ? part_counts.data() : nullptr), "ssx_spectral_read", ctxs_[d]);
		if (d == 0) first = info;
		if (sums && info.done_spp != first.done_spp) throw HostError{ SSX_ERR_STATE, "the devices' wavelength bins hold different sample counts (level_devices was not run)" };
		if (mean) merge_owned(mean->data(), part_mean.data(), B, owner_(d));
		if (sums) merge_owned(sums->data(), part_sums.data(), B, owner_(d));
		if (counts) merge_owned(counts->data(), part_counts.data(), M, owner_(d));
	}
	return first;
}

void Renderer::spectral_image(std::vector<float>* mean, std::vector<uint32_t>* counts, std::vector<float>* centres) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "spectral_image: spectral output is off (set_spectral_bins)" };
	const ssx_spectral_info_t info = gather_bins_(mean, nullptr, counts); // (the library's means, not means recomputed here)
	if (centres) {
		centres->resize(spectral_bins_);
		for (size_t b = 0; b < spectral_bins_; ++b) (*centres)[b] = info.lambda_min + (static_cast<float>(b) + 0.5f) * info.bin_width;
	}
}

void Renderer::save_spectral_image(const std::string& path) {
	std::vector<float> mean;
	spectral_image(&mean);
	save_spectral_image(path, mean);
}

void Renderer::save_spectral_image(const std::string& path, const std::vector<float>& bins) {
	const size_t shape[3] = { options.res[1], options.res[0], spectral_bins_ };
	if (bins.size() != shape[0] * shape[1] * shape[2]) throw HostError{ SSX_ERR_ARG, "save_spectral_image: the array is not [height][width][bins]" };
	save_npy_f32(path, bins.data(), shape, 3);
}

void Renderer::set_spectral_moments(bool on) {
	wait_workers_();
	for (ssx_ctx* c : ctxs_) check_(api_->set_spectral_moments(c, on ? 1 : 0), "ssx_set_spectral_moments", c);
	spectral_moments_ = on;
}

std::vector<double> Renderer::gather_moments_() {
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	std::vector<double> q(pixels * B, 0.0), part(pixels * B);
	for (size_t d = 0; d < ctxs_.size(); ++d) { // every pixel from the device that owns it, bit for bit (merge_owned: the one merge by ownership mask)
		ssx_spectral_info_t qi{};
		check_(api_->spectral_variance(ctxs_[d], &qi, nullptr, part.data()), "ssx_spectral_variance", ctxs_[d]);
		merge_owned(q.data(), part.data(), B, owner_(d));
	}
	return q;
}

std::vector<float> Renderer::spectral_variance() {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "spectral_variance: spectral output is off (set_spectral_bins)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	std::vector<float> var(pixels * B, 0.0f), part(ctxs_.size() > 1 ? pixels * B : 0);
	for (size_t d = 0; d < ctxs_.size(); ++d) { // every pixel from the device that owns it (merge_owned: the one merge by ownership mask)
		ssx_spectral_info_t info{};
		check_(api_->spectral_variance(ctxs_[d], &info, ctxs_.size() > 1 ? part.data() : var.data(), nullptr), "ssx_spectral_variance", ctxs_[d]);
		if (ctxs_.size() > 1) merge_owned(var.data(), part.data(), B, owner_(d));
	}
	return var;
}

void Renderer::save_spectral_variance(const std::string& path) { save_spectral_image(path, spectral_variance()); }

Renderer::Probe Renderer::probe(const std::vector<uint8_t>& labels, size_t regions) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "probe: spectral output is off (set_spectral_bins)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	if (labels.size() != pixels) throw HostError{ SSX_ERR_ARG, "probe: labels is not [height][width]" };
	if (regions < 1 || regions > 32) throw HostError{ SSX_ERR_ARG, "probe: need 1..32 regions" };
	Probe r;
	r.regions = regions; r.bins = B;
	r.SS.resize(regions * B); r.VV.resize(regions * B); r.NN.resize(regions * B); r.UU.resize(regions * B);
	ssx_ctx* root = ctxs_[0];
	const uint32_t r32 = static_cast<uint32_t>(regions);
	ssx_spectral_info_t info{};
	if (ctxs_.size() == 1) {
		check_(api_->spectral_variance(root, &info, nullptr, nullptr), "ssx_spectral_variance", root);
		check_(api_->spectral_probe(root, labels.data(), r32, r.SS.data(), r.NN.data(), r.VV.data(), r.UU.data()), "ssx_spectral_probe", root);
	} else { // S, N (gather_bins_) and Q from the device that owns the pixel, bit for bit; then the pure probe on device 0
		level_devices(); // (a stopped render: one sample count behind every pixel)
		std::vector<double> sums;
		std::vector<uint32_t> counts;
		info = gather_bins_(nullptr, &sums, &counts);
		const std::vector<double> q = gather_moments_();
		check_(api_->probe_arrays(root, w32_(), h32_(), static_cast<uint32_t>(B), sums.data(), q.data(), counts.data(), labels.data(), r32, r.SS.data(), r.NN.data(), r.VV.data(), r.UU.data()),
		       "ssx_probe_arrays", root);
	}
	r.lambda_min = info.lambda_min; r.bin_width = info.bin_width;
	r.mean.resize(regions * B); r.std_err.resize(regions * B);
	probe_derive(regions, B, r.SS.data(), r.NN.data(), r.VV.data(), r.UU.data(), r.mean.data(), r.std_err.data());
	return r;
}

void Renderer::save_probe_csv(const std::string& path, const Probe& p) const {
	ssx::save_probe_csv(path, p.regions, p.bins, p.lambda_min, p.bin_width, p.SS.data(), p.NN.data(), p.VV.data(), p.UU.data());
}

std::vector<uint8_t> Renderer::labels_from_rects(const std::vector<std::array<size_t, 4>>& rects) const {
	const size_t W = options.res[0], H = options.res[1];
	if (rects.empty() || rects.size() > 32) throw HostError{ SSX_ERR_ARG, "labels_from_rects: need 1..32 rectangles" };
	std::vector<uint8_t> labels(W * H, 255u);
	for (size_t r = 0; r < rects.size(); ++r) {
		const std::array<size_t, 4>& q = rects[r];
		if (q[0] >= q[2] || q[1] >= q[3] || q[2] > W || q[3] > H) throw HostError{ SSX_ERR_ARG, "labels_from_rects: rectangle " + std::to_string(r) + " is empty or leaves the image" };
		for (size_t j = q[1]; j < q[3]; ++j) for (size_t i = q[0]; i < q[2]; ++i) labels[j * W + i] = static_cast<uint8_t>(r);
	}
	return labels;
}

Renderer::SpectralNoise Renderer::spectral_noise(const std::vector<uint8_t>& mask) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "spectral_noise: spectral output is off (set_spectral_bins)" };
	const size_t W = options.res[0], H = options.res[1], B = spectral_bins_, tiles_x = (W + 7) / 8, tiles = tiles_x * ((H + 7) / 8);
	if (!mask.empty() && mask.size() != W * H) throw HostError{ SSX_ERR_ARG, "spectral_noise: mask is not [height][width]" };
	const uint8_t* const m = mask.empty() ? nullptr : mask.data();
	SpectralNoise r;
	r.bins = B;
	r.EV.resize(B); r.EM.resize(B); r.PP.resize(B); r.PU.resize(B); r.rel.resize(B);
	ssx_ctx* root = ctxs_[0];
	if (ctxs_.size() == 1) {
		check_(api_->spectral_noise(root, m, r.EV.data(), r.EM.data(), r.PP.data(), r.PU.data(), nullptr, nullptr, nullptr, nullptr), "ssx_spectral_noise", root);
	} else { // every tile's partials from the device that owns the tile, bit for bit; then the pure reduction on device 0
		level_devices(); // (a stopped render: one sample count behind every pixel)
		std::vector<double> tEV(tiles * B, 0.0), tEM(tiles * B, 0.0), pEV(tiles * B), pEM(tiles * B);
		std::vector<uint32_t> tPP(tiles * B, 0u), tPU(tiles * B, 0u), pPP(tiles * B), pPU(tiles * B);
		for (size_t d = 0; d < ctxs_.size(); ++d) {
			check_(api_->spectral_noise(ctxs_[d], m, r.EV.data(), r.EM.data(), r.PP.data(), r.PU.data(), pEV.data(), pEM.data(), pPP.data(), pPU.data()), "ssx_spectral_noise", ctxs_[d]);
			const ssx_sums_info_t owner = owner_(d);
			for (size_t t = 0; t < tiles; ++t) {
				if (!sums_owner(owner, (t % tiles_x) * 8, (t / tiles_x) * 8)) continue;
				std::memcpy(&tEV[t * B], &pEV[t * B], B * sizeof(double)); std::memcpy(&tEM[t * B], &pEM[t * B], B * sizeof(double));
				std::memcpy(&tPP[t * B], &pPP[t * B], B * sizeof(uint32_t)); std::memcpy(&tPU[t * B], &pPU[t * B], B * sizeof(uint32_t));
			}
		}
		check_(api_->spectral_noise_reduce(root, static_cast<uint32_t>(tiles), static_cast<uint32_t>(B), tEV.data(), tEM.data(), tPP.data(), tPU.data(),
		                                   r.EV.data(), r.EM.data(), r.PP.data(), r.PU.data()), "ssx_spectral_noise_reduce", root);
	}
	ssx_spectral_info_t info{};
	check_(api_->spectral_variance(root, &info, nullptr, nullptr), "ssx_spectral_variance", root);
	r.lambda_min = info.lambda_min; r.bin_width = info.bin_width;
	spectral_noise_derive(B, r.EV.data(), r.EM.data(), r.PP.data(), r.PU.data(), &r.noise, &r.coverage, r.rel.data());
	return r;
}

void Renderer::save_spectral_noise_csv(const std::string& path, const SpectralNoise& n) const {
	ssx::save_spectral_noise_csv(path, n.bins, n.lambda_min, n.bin_width, n.EV.data(), n.EM.data(), n.PP.data(), n.PU.data());
}

std::vector<uint8_t> Renderer::mask_from_rects(const std::vector<std::array<size_t, 4>>& rects) const {
	const size_t W = options.res[0], H = options.res[1];
	std::vector<uint8_t> mask(W * H, 0u);
	for (size_t r = 0; r < rects.size(); ++r) {
		const std::array<size_t, 4>& q = rects[r];
		if (q[0] >= q[2] || q[1] >= q[3] || q[2] > W || q[3] > H) throw HostError{ SSX_ERR_ARG, "mask_from_rects: rectangle " + std::to_string(r) + " is empty or leaves the image" };
		for (size_t j = q[1]; j < q[3]; ++j) for (size_t i = q[0]; i < q[2]; ++i) mask[j * W + i] = 1u;
	}
	return mask;
}

Renderer::UntilSpectral Renderer::render_until_spectral(double target, size_t step, size_t max_spp, const std::vector<uint8_t>& mask, double min_coverage, const std::function<bool()>& tick,
                                                        bool resume) {
	if (step == 0 || max_spp == 0) throw HostError{ SSX_ERR_ARG, "render_until_spectral: step and max_spp must be positive" };
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "render_until_spectral: spectral output is off (set_spectral_bins)" };
	if (!mask.empty() && mask.size() != options.res[0] * options.res[1]) throw HostError{ SSX_ERR_ARG, "render_until_spectral: mask is not [height][width]" };
	UntilSpectral r;
	r.noise = r.coverage = NAN;
	if (resume) { // what the devices hold is taken up: no ssx_render_start, and the figure first -- it may already meet the target
		const SpectralNoise now = spectral_noise(mask); // (throws SSX_ERR_STATE with the library's reason when the moments are not valid)
		r.noise = now.noise; r.coverage = now.coverage;
		if ((r.noise <= target && r.coverage >= min_coverage) || done_spp() >= max_spp) { r.spp = done_spp(); return r; }
	} else set_spectral_moments(true);
	bool stopped = false;
	for (size_t n = 0;; ++n) {
		if (n == 0 && !resume) start_(step, step); else render_continue(step);
		while (tick && is_rendering()) {
			if (!stopped && tick()) { render_stop(); stopped = true; }
			std::this_thread::sleep_for(std::chrono::milliseconds(10));
		}
		wait_workers_();
		if (!stopped) { const SpectralNoise now = spectral_noise(mask); r.noise = now.noise; r.coverage = now.coverage; }
		if (stopped || (r.noise <= target && r.coverage >= min_coverage) || done_spp() >= max_spp) break;
	}
	r.spp = done_spp();
	return r;
}

Renderer::Compare Renderer::compare_spectral(const Checkpoint& other, const std::vector<uint8_t>& labels, size_t regions, double t2, bool maps) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "compare_spectral: spectral output is off (set_spectral_bins)" };
	const size_t W = options.res[0], H = options.res[1], pixels = W * H, B = spectral_bins_;
	if (labels.size() != pixels) throw HostError{ SSX_ERR_ARG, "compare_spectral: labels is not [height][width]" };
	if (regions < 1 || regions > 32) throw HostError{ SSX_ERR_ARG, "compare_spectral: need 1..32 regions" };
	if (!other.spectral.bins || other.moments.empty()) throw HostError{ SSX_ERR_ARG, "compare_spectral: the other render carries no wavelength bins with their second moments" };
	if (other.spectral.width != W || other.spectral.height != H || other.spectral.bins != B) // (so that the arrays are as large as the library will read them)
		throw HostError{ SSX_ERR_ARG, "compare_spectral: the other render's size or bin count differs from this render's" };
	Compare r;
	r.regions = regions; r.bins = B;
	r.DD.resize(regions * B); r.VV.resize(regions * B); r.X2.resize(regions * B); r.CC.resize(regions * B); r.NC.resize(regions * B); r.EX.resize(regions * B);
	if (maps) { r.diff.resize(pixels * B); r.var.resize(pixels * B); }
	float* const diff = maps ? r.diff.data() : nullptr, * const var = maps ? r.var.data() : nullptr;
	ssx_ctx* root = ctxs_[0];
	const uint32_t r32 = static_cast<uint32_t>(regions);
	ssx_spectral_info_t info{};
	if (ctxs_.size() == 1) {
		check_(api_->spectral_variance(root, &info, nullptr, nullptr), "ssx_spectral_variance", root);
		check_(api_->spectral_compare(root, &other.spectral, other.spectral_sums.data(), other.moments.data(), other.spectral_counts.data(), labels.data(), r32, t2,
		                              r.DD.data(), r.VV.data(), r.X2.data(), r.CC.data(), r.NC.data(), r.EX.data(), diff, var), "ssx_spectral_compare", root);
	} else { // S, N (gather_bins_) and Q from the device that owns the pixel, bit for bit; then the pure comparison on device 0, as the probe does
		level_devices(); // (a stopped render: one sample count behind every pixel)
		std::vector<double> sums;
		std::vector<uint32_t> counts;
		info = gather_bins_(nullptr, &sums, &counts);
		const std::vector<double> q = gather_moments_();
		if (std::memcmp(&info.lambda_min, &other.spectral.lambda_min, sizeof(float)) != 0 || std::memcmp(&info.bin_width, &other.spectral.bin_width, sizeof(float)) != 0)
			throw HostError{ SSX_ERR_ARG, "compare_spectral: lambda_min or bin_width of the other render differs from this render's" };
		check_(api_->spectral_compare_arrays(root, w32_(), h32_(), static_cast<uint32_t>(B), sums.data(), q.data(), counts.data(), other.spectral_sums.data(), other.moments.data(),
		                                     other.spectral_counts.data(), labels.data(), r32, t2, r.DD.data(), r.VV.data(), r.X2.data(), r.CC.data(), r.NC.data(), r.EX.data(), diff, var),
		       "ssx_spectral_compare_arrays", root);
	}
	r.lambda_min = info.lambda_min; r.bin_width = info.bin_width;
	const size_t n = regions * B;
	r.mean_diff.resize(n); r.std_err.resize(n); r.z.resize(n); r.chi2.resize(n); r.exceed.resize(n); r.coverage.resize(n);
	compare_derive(regions, B, r.DD.data(), r.VV.data(), r.X2.data(), r.CC.data(), r.NC.data(), r.EX.data(), r.mean_diff.data(), r.std_err.data(), r.z.data(), r.chi2.data(),
	               r.exceed.data(), r.coverage.data());
	return r;
}

void Renderer::save_compare_csv(const std::string& path, const Compare& c) const {
	ssx::save_compare_csv(path, c.regions, c.bins, c.lambda_min, c.bin_width, c.DD.data(), c.VV.data(), c.X2.data(), c.CC.data(), c.NC.data(), c.EX.data());
}

namespace {
// the outputs of a colour difference, sized; what both routes hand to the library
Renderer::DeltaE delta_e_result(size_t pixels, size_t regions, bool maps) {
	Renderer::DeltaE r;
	r.regions = regions;
	const size_t n = regions * 2;
	r.SUM.resize(n); r.SSQ.resize(n); r.MAX.resize(n); r.NF.resize(n); r.NX.resize(n); r.EX.resize(n);
	if (maps) r.de.resize(pixels * 2);
	return r;
}
void delta_e_finish(Renderer::DeltaE& r) {
	const size_t n = r.regions * 2;
	r.mean.resize(n); r.rms.resize(n); r.max.resize(n); r.exceed.resize(n); r.coverage.resize(n);
	delta_e_derive(r.regions, r.SUM.data(), r.SSQ.data(), r.MAX.data(), r.NF.data(), r.NX.data(), r.EX.data(), r.mean.data(), r.rms.data(), r.max.data(), r.exceed.data(), r.coverage.data());
}
void delta_e_check_labels(const char* what, const std::vector<uint8_t>& labels, size_t pixels, size_t regions) {
	if (!labels.empty() && labels.size() != pixels) throw HostError{ SSX_ERR_ARG, std::string(what) + ": labels is not [height][width]" };
	if (regions < 1 || regions > 32 || (labels.empty() && regions != 1)) throw HostError{ SSX_ERR_ARG, std::string(what) + ": need 1..32 regions (1 without labels)" };
}
} // namespace

Renderer::DeltaE Renderer::delta_e_images(const float* xyz_a, const float* xyz_b, const double white_a[3], const double white_b[3], const std::vector<uint8_t>& labels, size_t regions,
                                          const double t[2], bool maps) {
	wait_workers_();
	const size_t pixels = options.res[0] * options.res[1];
	delta_e_check_labels("delta_e_images", labels, pixels, regions);
	DeltaE r = delta_e_result(pixels, regions, maps);
	ssx_ctx* root = ctxs_[0];
	check_(api_->delta_e_images(root, w32_(), h32_(), xyz_a, xyz_b, white_a, white_b, labels.empty() ? nullptr : labels.data(), static_cast<uint32_t>(regions), t,
	                            maps ? r.de.data() : nullptr, nullptr, r.SUM.data(), r.SSQ.data(), r.MAX.data(), r.NF.data(), r.NX.data(), r.EX.data()), "ssx_delta_e_images", root);
	delta_e_finish(r);
	return r;
}

Renderer::DeltaE Renderer::delta_e(const DeltaESide& side_a, const DeltaESide& side_b, const double white_a[3], const double white_b[3], const std::vector<uint8_t>& labels,
                                   size_t regions, const double t[2], bool maps, const DenoiseParams* denoise, const DemodParams* demod) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "delta_e: spectral output is off (set_spectral_bins)" };
	if (!side_a.weights || !side_b.weights) throw HostError{ SSX_ERR_ARG, "delta_e: a side without weights" };
	const bool filtered = side_a.denoised || side_b.denoised;
	if (filtered && !denoise) throw HostError{ SSX_ERR_ARG, "delta_e: a denoised side needs the filter's parameters (pass denoise)" };
	if (demod && !filtered) throw HostError{ SSX_ERR_ARG, "delta_e: the demodulated mode is a mode of a denoised side" };
	const size_t pixels = options.res[0] * options.res[1];
	delta_e_check_labels("delta_e", labels, pixels, regions);
	if (ctxs_.size() == 1 && !demod && !side_a.optics && !side_b.optics && !side_a.defocus && !side_b.defocus && !side_a.glare && !side_b.glare) {
		DeltaE r = delta_e_result(pixels, regions, maps);
		ssx_ctx* root = ctxs_[0];
		const ssx_denoise_params dp = denoise ? to_abi(*denoise, false) : ssx_denoise_params{};
		check_(api_->spectral_delta_e(root, filtered ? &dp : nullptr, side_a.denoised ? 1 : 0, side_b.denoised ? 1 : 0, side_a.weights, side_b.weights, white_a, white_b,
		                              labels.empty() ? nullptr : labels.data(), static_cast<uint32_t>(regions), t, maps ? r.de.data() : nullptr, nullptr,
		                              r.SUM.data(), r.SSQ.data(), r.MAX.data(), r.NF.data(), r.NX.data(), r.EX.data()), "ssx_spectral_delta_e", root);
		delta_e_finish(r);
		return r;
	}
	// each side by the develop's own route (several devices: every pixel from its owner; the demodulated filter), then the pure entry on device 0
	auto side = [&](const DeltaESide& x) {
		const DenoiseParams* const dn = x.denoised ? denoise : nullptr;
		const DemodParams* const dm = x.denoised ? demod : nullptr;
		return x.glare ? develop_glare(x.weights, 3, *x.glare, dn, dm, x.optics, x.defocus) : develop(x.weights, 3, dn, dm, x.optics, x.defocus);
	};
	const std::vector<float> xyz_a = side(side_a), xyz_b = side(side_b);
	return delta_e_images(xyz_a.data(), xyz_b.data(), white_a, white_b, labels, regions, t, maps);
}

void Renderer::save_delta_e_csv(const std::string& path, const DeltaE& d) const {
	ssx::save_delta_e_csv(path, d.regions, d.SUM.data(), d.SSQ.data(), d.MAX.data(), d.NF.data(), d.NX.data(), d.EX.data());
}

void Renderer::save_delta_e_map(const std::string& path, const DeltaE& d) {
	if (d.de.empty()) throw HostError{ SSX_ERR_ARG, "save_delta_e_map: the colour difference was made without its map" };
	const size_t shape[3] = { options.res[1], options.res[0], 2 };
	save_npy_f32(path, d.de.data(), shape, 3);
}

void Renderer::save_compare_map(const std::string& path, const Compare& c) {
	if (c.diff.empty()) throw HostError{ SSX_ERR_ARG, "save_compare_map: the comparison was made without its maps" };
	std::vector<float> zmap(c.diff.size());
	compare_zmap(zmap.size(), c.diff.data(), c.var.data(), zmap.data());
	save_spectral_image(path, zmap);
}

Renderer::Guides Renderer::guides() {
	wait_workers_();
	const size_t W = options.res[0], H = options.res[1];
	Guides g;
	g.prim.assign(W * H, 0u); g.depth.assign(W * H, 0.0f); g.normal.assign(W * H * 3, 0.0f); g.albedo.assign(W * H * 4, 0.0f);
	check_(api_->guides(ctxs_[0], w32_(), h32_(), g.prim.data(), g.depth.data(), g.normal.data(), g.albedo.data()), "ssx_guides", ctxs_[0]);
	return g;
}

void Renderer::save_guides(const std::string& path) {
	const Guides g = guides();
	const size_t pixels = options.res[0] * options.res[1];
	std::vector<float> all(pixels * 9);
	for (size_t p = 0; p < pixels; ++p) {
		float* o = &all[p * 9];
		o[0] = g.prim[p] == 0xFFFFFFFFu ? -1.0f : static_cast<float>(g.prim[p]);
		o[1] = g.depth[p];
		std::memcpy(o + 2, &g.normal[p * 3], 3 * sizeof(float));
		std::memcpy(o + 5, &g.albedo[p * 4], 4 * sizeof(float));
	}
	const size_t shape[3] = { options.res[1], options.res[0], 9 };
	save_npy_f32(path, all.data(), shape, 3);
}

// What the pure filter calls take from several devices besides the image (render_wait combined it: xyza): the devices are brought level (a stopped render: one
// sample count behind every pixel's v), the variances are combined (each pixel's v is nonzero on its owner alone) and put into image units --
// var = (float)(v * (s * s)) in binary64, s = what the image multiplies the mean by -- and the guides, which do not depend on ownership.
Renderer::FilterInputs Renderer::filter_inputs_() {
	level_devices();
	std::vector<double> v;
	(void)noise(&v);
	const double s = options.rgb_mode ? 1.0 : 1000.0;
	FilterInputs in;
	in.var.resize(v.size());
	for (size_t p = 0; p < v.size(); ++p) in.var[p] = static_cast<float>(v[p] * (s * s));
	in.guides = guides();
	return in;
}

Framebuffer Renderer::denoise(const DenoiseParams& params, std::vector<float>* xyza_out) {
	wait_workers_();
	const size_t pixels = options.res[0] * options.res[1];
	const ssx_denoise_params dp = to_abi(params);
	std::vector<float> out(pixels * 4);
	ssx_ctx* root = ctxs_[0];
	if (ctxs_.size() == 1) check_(api_->denoise(root, &dp, out.data(), nullptr), "ssx_denoise", root);
	else { // every device holds its own tiles: image and variance combined by ownership, then the pure filter on device 0
		const FilterInputs in = filter_inputs_();
		check_(api_->denoise_images(root, &dp, w32_(), h32_(), xyza.data(), in.var.data(), in.guides.prim.data(), in.guides.albedo.data(), out.data(), nullptr), "ssx_denoise_images", root);
	}
	Framebuffer fb(options.res);
	color->xyza_to_srgba(out.data(), fb.data(), pixels);
	if (xyza_out) xyza_out->swap(out);
	return fb;
}

std::vector<float> Renderer::albedo_bins(size_t bins, uint32_t supersample) {
	wait_workers_();
	std::vector<float> rho(options.res[0] * options.res[1] * bins);
	check_(api_->albedo_bins(ctxs_[0], w32_(), h32_(), static_cast<uint32_t>(bins), supersample, rho.data()), "ssx_albedo_bins", ctxs_[0]);
	return rho;
}

void Renderer::save_albedo_bins(const std::string& path, size_t bins, uint32_t supersample) {
	const std::vector<float> rho = albedo_bins(bins, supersample);
	const size_t shape[3] = { options.res[1], options.res[0], bins };
	save_npy_f32(path, rho.data(), shape, 3);
}

std::vector<float> Renderer::demod_weights_(const DemodParams& demod) const {
	const size_t B = spectral_bins_;
	if (!demod.weights_xyz.empty()) {
		if (demod.weights_xyz.size() != 3 * B) throw HostError{ SSX_ERR_ARG, "DemodParams.weights_xyz is not [3][bins]" };
		return demod.weights_xyz;
	}
	const ssx_scene_desc& d = scene->desc();
	const std::vector<double> w = develop_weights({ color->std_obs_xbar, color->std_obs_ybar, color->std_obs_zbar }, nullptr, nullptr, nullptr, static_cast<uint32_t>(B), d.lambda_min, d.lambda_step);
	return std::vector<float>(w.begin(), w.end()); // (rounded to binary32 here, once)
}

Framebuffer Renderer::denoise_spectral(const DenoiseParams& params, std::vector<float>* bins, std::vector<float>* xyza_out, const DemodParams* demod) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "denoise_spectral: spectral output is off (set_spectral_bins)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	const ssx_denoise_params dp = to_abi(params, demod != nullptr);
	const ssx_demod_params dm = demod ? to_abi(*demod) : ssx_demod_params{};
	const std::vector<float> wc = demod ? demod_weights_(*demod) : std::vector<float>();
	std::vector<float> out(pixels * 4), mean(ctxs_.size() == 1 ? pixels * B : 0);
	ssx_ctx* root = ctxs_[0];
	if (ctxs_.size() > 1) mean = denoise_spectral_devices_(dp, demod, wc, out);
	else if (demod) check_(api_->denoise_spectral_demod(root, &dp, &dm, wc.data(), mean.data(), out.data(), nullptr), "ssx_denoise_spectral_demod", root);
	else check_(api_->denoise_spectral(root, &dp, mean.data(), out.data(), nullptr), "ssx_denoise_spectral", root);
	Framebuffer fb(options.res);
	color->xyza_to_srgba(out.data(), fb.data(), pixels);
	if (bins) bins->swap(mean);
	if (xyza_out) xyza_out->swap(out);
	return fb;
}

// denoise_spectral's several-device route (renderer.hpp): as denoise() combines image and variance; the sums S and counts N come from the device that owns
// the pixel, bit for bit.  The demodulated mode: DEMODULATE and REMODULATE of include/ssx.h on the host around the same pure filter with a zero albedo guide.
// Returns the filtered bins; out: the filtered image.
std::vector<float> Renderer::denoise_spectral_devices_(const ssx_denoise_params& dp, const DemodParams* demod, const std::vector<float>& wc, std::vector<float>& out) {
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_, E = B + B / 4;
	ssx_ctx* root = ctxs_[0];
	FilterInputs in = filter_inputs_();
	std::vector<double> sums;
	std::vector<uint32_t> counts;
	const ssx_spectral_info_t info = gather_bins_(nullptr, &sums, &counts);
	std::vector<float> e0 = spectral_channels(sums, counts, pixels, B, static_cast<double>(info.done_spp)), eL(pixels * E), image(xyza);
	Demodulation d{ demod ? demod->albedo_floor : 0.0f, {}, {}, {} };
	if (demod) {
		if (!(d.floor > 0.0f) || !std::isfinite(d.floor)) throw HostError{ SSX_ERR_ARG, "DemodParams.albedo_floor must be finite and positive" };
		float den[3];
		channel_denominators(wc, B, den);
		d.rho = albedo_bins(B, demod->supersample);
		d.rc.resize(pixels * 3);
		check_(api_->develop_images(root, w32_(), h32_(), static_cast<uint32_t>(B), d.rho.data(), wc.data(), 3, d.rc.data()), "ssx_develop_images", root);
		demodulate(d, den, B, e0, image, in.var);
		in.guides.albedo.assign(pixels * 4, 0.0f);
	}
	check_(api_->denoise_channels(root, &dp, w32_(), h32_(), image.data(), in.var.data(), in.guides.prim.data(), in.guides.albedo.data(),
	                              static_cast<uint32_t>(E), e0.data(), out.data(), nullptr, eL.data()), "ssx_denoise_channels", root);
	return ratio(eL, pixels, B, demod ? &d : nullptr, out);
}

namespace {
// the lens as the C ABI takes it; a NaN centre is the middle of the image
ssx_optics_params to_abi(const Renderer::Optics& o, size_t width, size_t height, size_t B) {
	if (o.max_radius <= SSX_OPTICS_MAX_RADIUS && (o.scale.size() != B || o.radius.size() != B || o.taps.size() != B * (2u * o.max_radius + 1u)))
		throw HostError{ SSX_ERR_ARG, "Optics: scale and radius must hold one entry per wavelength bin, taps 2 * max_radius + 1 per bin" };
	ssx_optics_params p{};
	p.struct_size = sizeof p;
	p.cx = std::isnan(o.cx) ? static_cast<float>(width) / 2.0f : o.cx;
	p.cy = std::isnan(o.cy) ? static_cast<float>(height) / 2.0f : o.cy;
	p.max_radius = o.max_radius;
	p.scale = o.scale.data(); p.radius = o.radius.data(); p.taps = o.taps.data();
	return p;
}
// the aperture as the C ABI takes it
ssx_defocus_params to_abi(const Renderer::Defocus& f, size_t B) {
	if (f.focus.size() != B) throw HostError{ SSX_ERR_ARG, "Defocus: focus must hold one entry per wavelength bin" };
	ssx_defocus_params p{};
	p.struct_size = sizeof p;
	p.max_radius = f.max_radius; p.gain = f.gain; p.focus = f.focus.data();
	return p;
}
} // namespace

std::vector<float> Renderer::defocus_images(const float* q, const float* depth, const Defocus& defocus) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "defocus_images: spectral output is off (set_spectral_bins)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	const ssx_defocus_params df = to_abi(defocus, B);
	std::vector<float> out(pixels * B);
	check_(api_->defocus_images(ctxs_[0], w32_(), h32_(), static_cast<uint32_t>(B), q, depth, &df, out.data()), "ssx_defocus_images", ctxs_[0]);
	return out;
}

std::vector<float> Renderer::optics_images(const float* q, const Optics& optics) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "optics_images: spectral output is off (set_spectral_bins)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	const ssx_optics_params op = to_abi(optics, options.res[0], options.res[1], B);
	std::vector<float> out(pixels * B);
	check_(api_->optics_images(ctxs_[0], w32_(), h32_(), static_cast<uint32_t>(B), q, &op, out.data()), "ssx_optics_images", ctxs_[0]);
	return out;
}

std::vector<float> Renderer::source_bins_(const DenoiseParams* denoise, const DemodParams* demod) {
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	std::vector<float> bins;
	if (denoise) (void)denoise_spectral(*denoise, &bins, nullptr, demod);
	else {
		level_devices(); // (a stopped render: one sample count behind every pixel)
		std::vector<double> sums;
		const ssx_spectral_info_t info = gather_bins_(nullptr, &sums, nullptr);
		const double M = static_cast<double>(B / 4), n = static_cast<double>(info.done_spp);
		bins.resize(pixels * B);
		for (size_t e = 0; e < bins.size(); ++e) bins[e] = static_cast<float>((sums[e] * M) / n); // the raw source of include/ssx.h
	}
	return bins;
}

namespace {
// the sensor as the C ABI takes it (B == 0: the weights are not needed)
ssx_sensor_params to_abi(const Renderer::Sensor& s, size_t B, bool demosaics) {
	if (B && s.weights.size() != 3 * B) throw HostError{ SSX_ERR_ARG, "Sensor: weights must hold three rows of one entry per wavelength bin" };
	if (demosaics && (s.taps.size() != 300 || s.ccm.size() != 9)) throw HostError{ SSX_ERR_ARG, "Sensor: taps must hold [4][3][25] entries and ccm [3][3]" };
	ssx_sensor_params p{};
	p.struct_size = sizeof p;
	for (int k = 0; k < 4; ++k) p.cfa[k] = s.cfa[k];
	p.noise = s.noise; p.seed = s.seed; p.frame = s.frame;
	p.exposure = s.exposure; p.inv_exposure = s.inv_exposure; p.read_var = s.read_var;
	p.dn_per_e = s.dn_per_e; p.e_per_dn = s.e_per_dn; p.black = s.black; p.white = s.white;
	p.weights = B ? s.weights.data() : nullptr;
	p.taps = demosaics ? s.taps.data() : nullptr; p.ccm = demosaics ? s.ccm.data() : nullptr;
	return p;
}
} // namespace

std::vector<float> Renderer::sensor_images(const float* q, const Sensor& sensor, std::vector<float>* dn) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "sensor_images: spectral output is off (set_spectral_bins)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	const ssx_sensor_params sp = to_abi(sensor, B, false);
	std::vector<float> raw(pixels);
	const bool adc = dn && sensor.white > 0.0f;
	if (dn) dn->assign(adc ? pixels : 0, 0.0f);
	check_(api_->sensor_images(ctxs_[0], w32_(), h32_(), static_cast<uint32_t>(B), q, &sp, raw.data(), adc ? dn->data() : nullptr), "ssx_sensor_images", ctxs_[0]);
	return raw;
}

std::vector<float> Renderer::demosaic_images(const float* raw, const Sensor& sensor) {
	wait_workers_();
	const size_t pixels = options.res[0] * options.res[1];
	const ssx_sensor_params sp = to_abi(sensor, 0, true);
	std::vector<float> out(pixels * 3);
	check_(api_->demosaic_images(ctxs_[0], w32_(), h32_(), raw, &sp, out.data()), "ssx_demosaic_images", ctxs_[0]);
	return out;
}

Renderer::SensorImage Renderer::develop_sensor(const Sensor& sensor, const DenoiseParams* denoise, const DemodParams* demod, const Optics* optics, const Defocus* defocus,
                                               const Glare* glare) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "develop_sensor: spectral output is off (set_spectral_bins)" };
	if (demod && !denoise) throw HostError{ SSX_ERR_ARG, "develop_sensor: the demodulated mode is a mode of the denoised source (pass denoise)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	SensorImage r;
	if (glare) { // the bins behind the glare, then the pure entries on device 0
		std::vector<float> bins;
		(void)develop_glare(nullptr, 0, *glare, denoise, demod, optics, defocus, &bins);
		r.raw = sensor_images(bins.data(), sensor, &r.dn);
		r.out = demosaic_images(r.raw.data(), sensor);
		return r;
	}
	if (ctxs_.size() == 1 && !demod) {
		ssx_ctx* root = ctxs_[0];
		const ssx_sensor_params sp = to_abi(sensor, B, true);
		const ssx_denoise_params dp = denoise ? to_abi(*denoise, false) : ssx_denoise_params{};
		const ssx_defocus_params df = defocus ? to_abi(*defocus, B) : ssx_defocus_params{};
		const ssx_optics_params op = optics ? to_abi(*optics, options.res[0], options.res[1], B) : ssx_optics_params{};
		r.out.resize(pixels * 3); r.raw.resize(pixels);
		if (sensor.white > 0.0f) r.dn.resize(pixels);
		check_(api_->spectral_develop_sensor(root, denoise ? &dp : nullptr, defocus ? &df : nullptr, optics ? &op : nullptr, &sp, r.out.data(), r.raw.data(),
		                                     r.dn.empty() ? nullptr : r.dn.data()), "ssx_spectral_develop_sensor", root);
		return r;
	}
	std::vector<float> bins = source_bins_(denoise, demod); // then the pure entries on device 0
	if (defocus) bins = defocus_images(bins.data(), guides().depth.data(), *defocus);
	if (optics) bins = optics_images(bins.data(), *optics);
	r.raw = sensor_images(bins.data(), sensor, &r.dn);
	r.out = demosaic_images(r.raw.data(), sensor);
	return r;
}

namespace {
// the glare as the C ABI takes it
ssx_glare_params to_abi(const Renderer::Glare& g, size_t B) {
	const size_t K = 2u * static_cast<size_t>(g.radius) + 1u;
	if (g.on.size() != B || (g.radius <= SSX_GLARE_MAX_RADIUS && g.psf.size() != B * K * K))
		throw HostError{ SSX_ERR_ARG, "Glare: on must hold one entry per wavelength bin, psf (2 * radius + 1)^2 per bin" };
	if ((g.px && g.px <= SSX_GLARE_MAX_EXTENT && g.twiddle_x.size() != g.px) || (g.py && g.py <= SSX_GLARE_MAX_EXTENT && g.twiddle_y.size() != g.py))
		throw HostError{ SSX_ERR_ARG, "Glare: twiddle_x must hold [px / 2][2] entries and twiddle_y [py / 2][2]" };
	ssx_glare_params p{};
	p.struct_size = sizeof p;
	p.radius = g.radius; p.px = g.px; p.py = g.py;
	p.on = g.on.data(); p.psf = g.psf.data(); p.twiddle_x = g.twiddle_x.data(); p.twiddle_y = g.twiddle_y.data();
	return p;
}
} // namespace

Renderer::Meter Renderer::meter_images(const float* img, const float luma[3], const uint8_t* mask) {
	wait_workers_();
	Meter m;
	m.hist.assign(4u * SSX_METER_KEYS, 0u); m.special.assign(16u, 0u);
	check_(api_->meter_images(ctxs_[0], w32_(), h32_(), img, luma, mask, m.hist.data(), m.special.data()), "ssx_meter_images", ctxs_[0]);
	return m;
}

std::vector<float> Renderer::local_images(const float* img, const float luma[3], const Local& local, std::vector<float>* base) {
	wait_workers_();
	const size_t pixels = options.res[0] * options.res[1];
	ssx_local_params p{};
	p.struct_size = sizeof p; p.radius = local.radius; p.exposure = local.exposure; p.y_lo = local.y_lo; p.y_hi = local.y_hi; p.eps = local.eps;
	p.pivot = local.pivot; p.compress = local.compress; p.boost = local.boost;
	std::vector<float> gain(pixels);
	if (base) base->assign(pixels, 0.0f);
	check_(api_->local_images(ctxs_[0], w32_(), h32_(), img, luma, &p, gain.data(), base ? base->data() : nullptr), "ssx_local_images", ctxs_[0]);
	return gain;
}

std::vector<float> Renderer::tone_images(const float* img, const Tone& tone, const float* local) {
	wait_workers_();
	const size_t pixels = options.res[0] * options.res[1];
	ssx_tone_params p{};
	p.struct_size = sizeof p; p.shift = tone.shift; p.curve_len = static_cast<uint32_t>(tone.curve.size()); p.lo = tone.lo; p.hi = tone.hi;
	for (int c = 0; c < 3; ++c) p.gains[c] = tone.gains[c];
	for (int k = 0; k < 9; ++k) p.matrix[k] = tone.matrix[k];
	p.curve = tone.curve.data();
	std::vector<float> out(pixels * 3);
	check_(api_->tone_images(ctxs_[0], w32_(), h32_(), img, local, &p, out.data()), "ssx_tone_images", ctxs_[0]);
	return out;
}

void Renderer::display_luma(const float matrix[9], float luma[3]) {
	for (int c = 0; c < 3; ++c)
		luma[c] = static_cast<float>((0.2126 * static_cast<double>(matrix[c]) + 0.7152 * static_cast<double>(matrix[3 + c])) + 0.0722 * static_cast<double>(matrix[6 + c]));
}

std::vector<float> Renderer::finish(const float* img, const Display& d, Meter* meter) {
	float luma[3];
	display_luma(d.matrix, luma);
	Meter m = meter_images(img, luma);
	float out[SSH_METER_OUT];
	if (ssh_meter_derive(m.hist.data(), m.special.data(), d.key, d.white_percentile, nullptr, 0, nullptr, out) != SSX_OK) throw HostError{ SSX_ERR_ARG, std::string("finish: ") + ssh_last_error() };
	Tone tone;
	for (int c = 0; c < 3; ++c) {
		const float wb = d.wb == WhiteBalance::Grey ? out[SSH_METER_GREY + c] : (d.wb == WhiteBalance::WhitePatch ? out[SSH_METER_PATCH + c] : 1.0f);
		tone.gains[c] = out[SSH_METER_EXPOSURE] * wb;
	}
	for (int k = 0; k < 9; ++k) tone.matrix[k] = d.matrix[k];
	std::vector<float> gain;
	if (d.local) {
		Local l;
		l.radius = d.radius; l.compress = d.compress; l.boost = d.boost; l.eps = d.eps; l.exposure = out[SSH_METER_EXPOSURE]; l.pivot = out[SSH_METER_PIVOT];
		gain = local_images(img, luma, l);
	}
	uint32_t lo_bits, hi_bits;
	std::memcpy(&lo_bits, &tone.lo, 4); std::memcpy(&hi_bits, &tone.hi, 4);
	tone.curve.assign(((hi_bits - lo_bits) >> tone.shift) + 2u, 0.0f);
	const double white = out[SSH_METER_WHITE_EXPOSED] > 0.0f ? static_cast<double>(out[SSH_METER_WHITE_EXPOSED]) : 1.0;
	if (ssh_tone_curve(d.curve, white, tone.lo, tone.hi, tone.shift, tone.curve.data(), static_cast<uint32_t>(tone.curve.size())) != SSX_OK)
		throw HostError{ SSX_ERR_ARG, std::string("finish: ") + ssh_last_error() };
	std::vector<float> result = tone_images(img, tone, d.local ? gain.data() : nullptr);
	if (meter) *meter = std::move(m);
	return result;
}

std::vector<float> Renderer::glare_images(const float* q, const Glare& glare) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "glare_images: spectral output is off (set_spectral_bins)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_;
	const ssx_glare_params gp = to_abi(glare, B);
	std::vector<float> out(pixels * B);
	check_(api_->glare_images(ctxs_[0], w32_(), h32_(), static_cast<uint32_t>(B), q, &gp, out.data()), "ssx_glare_images", ctxs_[0]);
	return out;
}

std::vector<float> Renderer::develop_glare(const float* weights, size_t channels, const Glare& glare, const DenoiseParams* denoise, const DemodParams* demod, const Optics* optics,
                                           const Defocus* defocus, std::vector<float>* bins_out) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "develop_glare: spectral output is off (set_spectral_bins)" };
	if (demod && !denoise) throw HostError{ SSX_ERR_ARG, "develop_glare: the demodulated mode is a mode of the denoised source (pass denoise)" };
	if (!weights != !channels) throw HostError{ SSX_ERR_ARG, "develop_glare: weights and channels go together (NULL and 0: the bins alone)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_, C = channels;
	const uint32_t c32 = static_cast<uint32_t>(C);
	std::vector<float> out(pixels * C);
	ssx_ctx* root = ctxs_[0];
	if (ctxs_.size() == 1 && !demod) {
		const ssx_glare_params gp = to_abi(glare, B);
		const ssx_denoise_params dp = denoise ? to_abi(*denoise, false) : ssx_denoise_params{};
		const ssx_defocus_params df = defocus ? to_abi(*defocus, B) : ssx_defocus_params{};
		const ssx_optics_params op = optics ? to_abi(*optics, options.res[0], options.res[1], B) : ssx_optics_params{};
		if (bins_out) bins_out->assign(pixels * B, 0.0f);
		check_(api_->spectral_develop_glare(root, denoise ? &dp : nullptr, defocus ? &df : nullptr, optics ? &op : nullptr, &gp, weights, c32, C ? out.data() : nullptr,
		                                    bins_out ? bins_out->data() : nullptr), "ssx_spectral_develop_glare", root);
		return out;
	}
	std::vector<float> bins = source_bins_(denoise, demod); // then the pure entries on device 0 (the depth guide does not depend on ownership)
	if (defocus) bins = defocus_images(bins.data(), guides().depth.data(), *defocus);
	if (optics) bins = optics_images(bins.data(), *optics);
	bins = glare_images(bins.data(), glare);
	if (C) check_(api_->develop_images(root, w32_(), h32_(), static_cast<uint32_t>(B), bins.data(), weights, c32, out.data()), "ssx_develop_images", root);
	if (bins_out) *bins_out = std::move(bins);
	return out;
}

std::vector<float> Renderer::develop(const float* weights, size_t channels, const DenoiseParams* denoise, const DemodParams* demod, const Optics* optics, const Defocus* defocus) {
	wait_workers_();
	if (!spectral_bins_) throw HostError{ SSX_ERR_STATE, "develop: spectral output is off (set_spectral_bins)" };
	if (demod && !denoise) throw HostError{ SSX_ERR_ARG, "develop: the demodulated mode is a mode of the denoised source (pass denoise)" };
	const size_t pixels = options.res[0] * options.res[1], B = spectral_bins_, C = channels, n_dev = ctxs_.size();
	const uint32_t c32 = static_cast<uint32_t>(C);
	std::vector<float> out(pixels * (C ? C : 1));
	ssx_ctx* root = ctxs_[0];
	const ssx_denoise_params dp = denoise ? to_abi(*denoise, demod != nullptr) : ssx_denoise_params{};
	if (defocus && n_dev == 1 && !demod) {
		const ssx_defocus_params df = to_abi(*defocus, B);
		const ssx_optics_params op = optics ? to_abi(*optics, options.res[0], options.res[1], B) : ssx_optics_params{};
		check_(api_->spectral_develop_lens(root, denoise ? &dp : nullptr, &df, optics ? &op : nullptr, weights, c32, out.data(), nullptr), "ssx_spectral_develop_lens", root);
	} else if (optics && n_dev == 1 && !demod) {
		const ssx_optics_params op = to_abi(*optics, options.res[0], options.res[1], B);
		check_(api_->spectral_develop_optics(root, denoise ? &dp : nullptr, &op, weights, c32, out.data(), nullptr), "ssx_spectral_develop_optics", root);
	} else if (optics || defocus) { // q by the host's gather, then the pure entries on device 0 (the depth guide does not depend on ownership)
		std::vector<float> bins = source_bins_(denoise, demod);
		if (defocus) bins = defocus_images(bins.data(), guides().depth.data(), *defocus);
		const std::vector<float> behind = optics ? optics_images(bins.data(), *optics) : std::move(bins);
		check_(api_->develop_images(root, w32_(), h32_(), static_cast<uint32_t>(B), behind.data(), weights, c32, out.data()), "ssx_develop_images", root);
	} else if (n_dev == 1 && demod) {
		const ssx_demod_params dm = to_abi(*demod);
		const std::vector<float> wc = demod_weights_(*demod);
		check_(api_->spectral_develop_demod(root, &dp, &dm, wc.data(), weights, c32, out.data()), "ssx_spectral_develop_demod", root);
	} else if (n_dev == 1) check_(api_->spectral_develop(root, denoise ? &dp : nullptr, weights, c32, out.data()), "ssx_spectral_develop", root);
	else if (denoise) {
		std::vector<float> bins;
		(void)denoise_spectral(*denoise, &bins, nullptr, demod);
		check_(api_->develop_images(root, w32_(), h32_(), static_cast<uint32_t>(B), bins.data(), weights, c32, out.data()), "ssx_develop_images", root);
	} else {
		level_devices(); // (a stopped render: one sample count behind every pixel)
		std::vector<float> part(out.size());
		for (size_t d = 0; d < n_dev; ++d) { // every pixel from the device that owns it, bit for bit (merge_owned: the one merge by ownership mask)
			check_(api_->spectral_develop(ctxs_[d], nullptr, weights, c32, part.data()), "ssx_spectral_develop", ctxs_[d]);
			merge_owned(out.data(), part.data(), C, owner_(d));
		}
	}
	return out;
}

std::pair<size_t, double> Renderer::render_until(double target, size_t step, size_t max_spp, const std::function<bool()>& tick) {
	if (step == 0 || max_spp == 0) throw HostError{ SSX_ERR_ARG, "render_until: step and max_spp must be positive" };
	set_noise_estimate(true);
	double level = INFINITY;
	bool stopped = false;
	for (size_t n = 0;; ++n) {
		if (n == 0) start_(step, step); else render_continue(step);
		while (tick && is_rendering()) {
			if (!stopped && tick()) { render_stop(); stopped = true; }
			std::this_thread::sleep_for(std::chrono::milliseconds(10));
		}
		wait_workers_();
		if (n >= 1 && !stopped) level = noise();
		if (stopped || level <= target || done_spp() >= max_spp) break;
	}
	return { done_spp(), level };
}

void Renderer::save_checkpoint(const std::string& path) {
	level_devices(); // a stopped multi-device render: one count for the file
	const size_t pixels = options.res[0] * options.res[1];
	Checkpoint ck;
	ck.sums.assign(pixels * 4, 0.0);
	std::vector<double> sums(pixels * 4), s2(pixels);
	bool have_s2 = true;
	uint32_t batches = 0;
	for (size_t d = 0; d < ctxs_.size(); ++d) {
		ssx_sums_info_t info{};
		check_(api_->sums_export(ctxs_[d], &info, sums.data(), s2.data()), "ssx_sums_export", ctxs_[d]);
		if (d == 0) { ck.info = info; batches = info.noise_batches; ck.s2.assign(pixels, 0.0); }
		have_s2 = have_s2 && info.noise_batches != 0 && info.noise_batches == batches; // (devices brought level apart have taken different batches: not one estimate)
		sums_merge(ck.sums.data(), ck.s2.data(), sums.data(), s2.data(), info);
	}
	ck.info.tile_first = 0; ck.info.tile_stride = 1; ck.info.tile_skew = 0; // the merged array is the whole image
	if (!have_s2) { ck.s2.clear(); ck.info.noise_batches = 0; }
	// the wavelength bins, when every device holds valid ones (a render with spectral output, or a resume that took them up): merged by ownership like the sums
	bool have_bins = spectral_bins_ != 0;
	for (size_t d = 0; have_bins && d < ctxs_.size(); ++d) {
		ssx_spectral_info_t si{};
		have_bins = api_->spectral_read(ctxs_[d], &si, nullptr, nullptr, nullptr) == SSX_OK; // (SSX_ERR_STATE: continuable sums without bins)
	}
	if (have_bins) ck.spectral = gather_bins_(nullptr, &ck.spectral_sums, &ck.spectral_counts);
	// their second moments, when every device holds valid ones: the same merge
	bool have_moments = have_bins && spectral_moments_;
	for (size_t d = 0; have_moments && d < ctxs_.size(); ++d) {
		ssx_spectral_info_t si{};
		have_moments = api_->spectral_variance(ctxs_[d], &si, nullptr, nullptr) == SSX_OK; // (SSX_ERR_STATE: valid bins without moments)
	}
	if (have_moments) ck.moments = gather_moments_();
	ck.scene_name = options.scene_name;
	ck.options_text = "observer=" + std::to_string(options.observer) + "\ntexture=" + options.texture_path + "\nlight_scale=" + std::to_string(options.light_scale) +
	                  "\nuplift=" + std::to_string(options.uplift) + "\nrgb=" + (options.rgb_mode ? "1" : "0") +
	                  "\nexplicit_light_sampling=" + (options.explicit_light_sampling ? "1" : "0") + "\n";
	checkpoint_save(path, ck);
}

bool Renderer::load_checkpoint(const std::string& path) {
	wait_workers_();
	const Checkpoint ck = checkpoint_load(path);
	const bool take_bins = ck.spectral.bins != 0u && spectral_bins_ == ck.spectral.bins;
	const bool take_moments = take_bins && spectral_moments_ && !ck.moments.empty();
	moments_resumed_ = false;
	for (size_t d = 0; d < ctxs_.size(); ++d) {
		const ssx_render_params p = params_for_(d, ck.info.done_spp ? ck.info.done_spp : 1u, 0);
		check_(api_->sums_import(ctxs_[d], &p, &ck.info, ck.sums.data(), ck.s2.empty() ? nullptr : ck.s2.data()), "ssx_sums_import", ctxs_[d]);
		// every device takes its own tiles from the whole array, however many devices wrote it
		if (take_bins) check_(api_->spectral_import(ctxs_[d], &ck.spectral, ck.spectral_sums.data(), ck.spectral_counts.data()), "ssx_spectral_import", ctxs_[d]);
		if (take_moments) check_(api_->spectral_moments_import(ctxs_[d], &ck.spectral, ck.moments.data()), "ssx_spectral_moments_import", ctxs_[d]);
	}
	moments_resumed_ = take_moments;
	time_start_ = std::chrono::steady_clock::now();
	started_ = true; need_join_ = false;
	expected_spp_ = ck.info.done_spp;
	return take_bins;
}

void Renderer::render_stop() { for (ssx_ctx* c : ctxs_) api_->render_stop(c); }

bool Renderer::is_rendering() const {
	for (ssx_ctx* c : ctxs_) if (api_->is_rendering(c)) return true;
	return false;
}

double Renderer::progress() const {
	double s = 0;
	for (ssx_ctx* c : ctxs_) s += api_->progress(c);
	return ctxs_.empty() ? 0.0 : s / static_cast<double>(ctxs_.size());
}

void Renderer::print_progress() const {
	auto pretty = [](double secs) {
		const double days = std::floor(secs / 86400.0); secs -= 86400.0 * days;
		const double hours = std::floor(secs / 3600.0); secs -= 3600.0 * hours;
		const double mins = std::floor(secs / 60.0); secs -= 60.0 * mins;
		if (days > 0.0) std::printf("%d days + ", static_cast<int>(days));
		std::printf("%02d:%02d:%06.3f", static_cast<int>(hours), static_cast<int>(mins), secs);
	};
	const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - time_start_).count();
	const double part = is_rendering() ? progress() : 1.0;
	if (part < 1.0) {
		if (part > 0.0) {
			std::printf("\rRender %.3f%% (ETA ", part * 100.0);
			pretty(elapsed / part - elapsed);
			std::printf(")           ");
			std::fflush(stdout);
		} else {
			std::printf("\rRender started                               ");
		}
	} else {
		std::printf("\rRender completed in ");
		pretty(elapsed);
		std::printf("             \n");
	}
}

void Renderer::render_wait() {
	if (!started_) return;
	wait_workers_();
	// Every device's share stays in its own HBM (ssx_render_wait without a host buffer).  The combine is
	// the path's one exchange step (north_star: reduce of the per-GPU framebuffers over xGMI): device 0
	// pulls each peer's framebuffer with a device-to-device copy and adds it with a kernel.  Every pixel
	// is nonzero in exactly one device's buffer and x + 0 is exact, so the sum is bit for bit the image
	// a single device produces (the multi-process path, bench.py, does the same with one RCCL reduce).
	// a stopped render: every device's share is the mean over the samples IT accumulated (ssx.h: ssx_done_spp); say so when the
	// counts differ from the request, as the image then is not what the reference would have left (finished tiles next to
	// untouched ones, src/renderer.cpp:388-394)
	const size_t tiles_x = (options.res[0] + 7) / 8, n_tiles = tiles_x * ((options.res[1] + 7) / 8);
	std::vector<uint32_t> done_tiles(ctxs_.size());
	bool partial_tiles = false;
	for (size_t d = 0; d < ctxs_.size(); ++d) {
		const uint32_t done = api_->done_spp(ctxs_[d]);
		done_tiles[d] = api_->done_tiles(ctxs_[d]);
		const size_t owned = n_tiles > d ? (n_tiles - d + ctxs_.size() - 1) / ctxs_.size() : 0;
		if (options.tile_major) {
			if (done_tiles[d] < owned) { partial_tiles = true; std::fprintf(stderr, "Render stopped: device %d finished %u of its %zu tiles; the others keep the checkerboard.\n", api_->device_index(ctxs_[d]), done_tiles[d], owned); }
		} else if (done != static_cast<uint32_t>(expected_spp_))
			std::fprintf(stderr, "Render stopped: device %d accumulated %u of %zu samples per pixel; its tiles hold the mean over those.\n", api_->device_index(ctxs_[d]), done, expected_spp_);
	}
	ssx_ctx* root = ctxs_[0];
	if (options.reduce_rccl) { // one RCCL reduce over all devices (a single context: RCCL with one rank)
		int rc = api_->reduce_rccl(ctxs_.data(), static_cast<int>(ctxs_.size()), w32_(), h32_());
		if (rc) throw HostError{ rc, std::string("ssx_reduce_rccl: ") + api_->last_error(root) };
	} else
	for (size_t d = 1; d < ctxs_.size(); ++d) {
		int rc = api_->accumulate_peer(root, api_->device_framebuffer(root), api_->device_index(ctxs_[d]), api_->device_framebuffer(ctxs_[d]),
		                               w32_(), h32_(), nullptr);
		if (rc) throw HostError{ rc, std::string("ssx_accumulate_peer: ") + api_->last_error(root) };
	}
	{
		int rc = api_->read_framebuffer(root, xyza.data());
		if (rc) throw HostError{ rc, std::string("ssx_read_framebuffer: ") + api_->last_error(root) };
	}
	started_ = false;
	// framebuffer(i,j) = sRGB_A_F32(ciexyz_to_srgb(XYZ), alpha)  (src/renderer.cpp:298)
	if (!partial_tiles) color->xyza_to_srgba(xyza.data(), framebuffer.data(), options.res[0] * options.res[1]);
	else { // a stopped tile-major render: like the reference's, the framebuffer keeps its checkerboard where no tile was finished (src/framebuffer.cpp:15-32)
		std::vector<float> all(xyza.size());
		color->xyza_to_srgba(xyza.data(), all.data(), options.res[0] * options.res[1]);
		const size_t skew = params_for_(0, 1, 0).tile_skew; // (what the devices rendered with)
		for (size_t j = 0; j < options.res[1]; ++j) for (size_t i = 0; i < options.res[0]; ++i) {
			const size_t tile = shared_tile(options.res[0], skew, i, j), d = tile % ctxs_.size();
			if (tile / ctxs_.size() < done_tiles[d]) std::memcpy(framebuffer(i, j), &all[4 * (j * options.res[0] + i)], 4 * sizeof(float));
		}
	}
	print_progress();
	if (!options.output_path.empty()) framebuffer.save(options.output_path); // src/renderer.cpp:393
}

} // namespace ssx

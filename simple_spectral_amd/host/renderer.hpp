// renderer.hpp -- C++ host mirror of the reference's Renderer (src/renderer.hpp:14-82) and
// Framebuffer (src/framebuffer.hpp:7-43).  Same verbs -- render_start / render_stop / render_wait
// / is_rendering, public `framebuffer` and `scene` -- but the worker threads and their tile loop
// (src/renderer.cpp:309-395) are replaced by the HIP path behind the C ABI (include/ssx.h),
// loaded from libssx_hip.so at construction.  There is no CPU rendering path: if the library or a
// gfx950 device is missing, the constructor throws.
#pragma once
#include "color.hpp"
#include "scene.hpp"

#include <cmath>
#include <array>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <vector>

struct ssx_ctx;

namespace ssx {

struct Checkpoint; // host/checkpoint.hpp

class Framebuffer { // sRGB + linear alpha, float, rows bottom to top (src/framebuffer.hpp:26-34)
public:
	explicit Framebuffer(const size_t res[2]); // 8x8 checkerboard 0.7/0.3, alpha 1 (src/framebuffer.cpp:15-32)
	const size_t res[2];
	float* operator()(size_t i, size_t j) { return &pixels_[4 * (j * res[0] + i)]; }
	const float* operator()(size_t i, size_t j) const { return &pixels_[4 * (j * res[0] + i)]; }
	float* data() { return pixels_.data(); }
	const float* data() const { return pixels_.data(); }
	void save(const std::string& path) const; // src/framebuffer.cpp:39-176
private:
	std::vector<float> pixels_;
};

class Renderer {
public:
	struct Options { // src/renderer.hpp:16-29, then the additive options of this build
		std::string scene_name;
		size_t res[2] = { 0, 0 };
		size_t spp = 0;
		bool indirect_only = false;
		std::string output_path;
		int observer = 1931;         // CIE_OBSERVER (src/stdafx.hpp:82-86), a compile-time switch in the reference
		uint64_t seed = 0;           // seeding contract of include/ssx.h
		int gpus = 1;                // devices 0..gpus-1, 8x8 tiles dealt round-robin
		std::string texture_path;    // default: data/scenes/crystal-lizard-4096.png, else the 512 version
		float light_scale = 30.0f;   // lightsc (src/scene.cpp:291-293)
		bool explicit_light_sampling = true; // EXPLICIT_LIGHT_SAMPLING (src/stdafx.hpp:44)
		bool reduce_rccl = false;            // --reduce=rccl: combine the devices' framebuffers with one RCCL reduce instead of peer copies + adds
		bool flat_field_correction = true;   // FLAT_FIELD_CORRECTION (src/stdafx.hpp:55); false: flux = radiance * dot(ray dir, camera.dir) (src/renderer.cpp:264-265)
		bool tile_major = false;     // --tile-major: walk through the tiles like the reference (src/renderer.cpp:340-409), so that a stopped render holds finished
		                             // tiles at the full sample count next to the untouched checkerboard (src/renderer.cpp:388-394) instead of a noisier whole image
		uint32_t libm = 0;           // --libm: ssx_render_params.libm (SSX_LIBM_BUILD | SSX_LIBM_GLIBC_2_35: glibc 2.35's x86-64 sinf / cosf / acosf)
		bool rgb_mode = false;       // RENDER_MODE_RGB (src/stdafx.hpp:91-93) instead of spectral rendering; `uplift` is then unused
		int uplift = 1;              // RENDER_MODE_SPECTRAL_ALGNUM: 1 = basis (ours), 2 = Meng et al. 2015, 3 = Jakob-Hanika 2019
		std::string meng_grid_path;  // default data/meng-et-al-2015-grid.bin (converted from the authors' header, meng2015.hpp)
		std::string jh_coeff_path;   // default data/jakob-and-hanika-2019-srgb.coeff (src/util/color.cpp:144); fitted and written when absent
		std::string data_dir = "data"; // CWD-relative like the reference's paths
		std::string hip_library;     // default: libssx_hip.so next to libssx_host.so
		size_t spp_per_launch = 0;   // render_start: samples per pixel of one launch (0: the library's choice); one launch is one batch of the noise estimate
	};
	const Options options;
	Framebuffer framebuffer;
	std::unique_ptr<ColorData> color;
	std::unique_ptr<JHModel> jh;
	std::unique_ptr<MengGrid> meng;
	std::unique_ptr<Scene> scene;
	std::vector<float> xyza; // per-pixel mean XYZ + alpha before the sRGB store (the parity metric)

	explicit Renderer(const Options& options);
	~Renderer();

	void render_start();            // src/renderer.cpp:396-422
	void render_stop();             // src/renderer.hpp:77
	void render_wait();             // src/renderer.cpp:423-430 (+ XYZ->sRGB store of :298 and save of :393)
	bool is_rendering() const;      // src/renderer.hpp:81
	double progress() const;        // the `part` of _print_progress (src/renderer.cpp:75)
	void print_progress() const;    // src/renderer.cpp:53-101

	// Progressive rendering (include/ssx.h: the sums of a render that walked through the samples can be taken up again, bit for bit).
	void render_continue(size_t spp);        // `spp` more samples per pixel onto what exists; asynchronous like render_start (then render_wait)
	size_t done_spp() const;                 // samples per pixel accumulated over the whole history (the smallest count among the devices)
	// After render_stop the devices of a multi-GPU render may hold different counts: the laggards render the missing samples (blocking; a
	// few launches at most), so that image, checkpoint and whatever follows speak of ONE count.  render_continue and save_checkpoint do it
	// themselves; call it BEFORE render_wait when the image written there is to be the checkpoint's.
	void level_devices();
	// One file with the sums of all devices, merged by ownership (host/checkpoint.hpp), after level_devices().  Not while rendering.  When every device holds
	// valid wavelength bins (set_spectral_bins before the render, or a load_checkpoint that took them up) the file carries them too, merged the same way
	// ("SSXCKPT2"); otherwise it is the file it always was.  When every device also holds valid second moments (set_spectral_moments before the render, or a
	// load_checkpoint that took them up) their Q follows the bins, read through ssx_spectral_variance's q and merged the same way ("SSXCKPT3").
	void save_checkpoint(const std::string& path);
	// Every device takes its own tiles from the file's array; render_wait() then yields the checkpointed image, render_continue goes on from it.
	// Throws HostError with the library's reason when the file belongs to another scene, size, seed or set of flags.
	// A file with wavelength bins, read with set_spectral_bins(its count) in force: every device also takes the bins of its tiles (ssx_spectral_import; the
	// number of devices may differ from the writer's), and spectral_image, denoise_spectral, develop and a later save_checkpoint go on as after a render of
	// those samples.  Returns whether the bins were taken up; when not (no bins in the file, spectral output off, another bin count) the resume is the plain one.
	// A file with the second moments, read with set_spectral_moments(true) in force and the bins taken up: every device also takes the Q of its tiles
	// (ssx_spectral_moments_import), and spectral_variance, probe, spectral_noise and render_until_spectral(resume) go on as after a render of those samples with
	// the moments on; moments_resumed() says whether.
	bool load_checkpoint(const std::string& path);
	bool moments_resumed() const { return moments_resumed_; }
	void set_noise_estimate(bool on);        // ssx_set_noise_estimate on every device
	// sqrt(sum v / n) / (sum A/N / n) over all devices (include/ssx.h ssx_noise_info); v_map: the per-pixel variances [height][width]
	double noise(std::vector<double>* v_map = nullptr);
	// Renders in steps of `step` samples per pixel (one launch, one batch of the estimate, each) until noise() <= target -- checked after every step
	// from the second on -- or done_spp() >= max_spp; returns {done_spp, noise}.  Blocking; `tick` (optional) is called every 10 ms meanwhile
	// and stops the render by returning true.  The decision reads only the sums: the same call gives the same count.  Then render_wait().
	std::pair<size_t, double> render_until(double target, size_t step, size_t max_spp, const std::function<bool()>& tick = {});

	// Spectral radiance output (include/ssx.h ssx_set_spectral_bins): `bins` wavelength bins per pixel (a multiple of 4 up to 64; 0 = off) on every
	// device, for the renders that follow.  Not while rendering.
	void set_spectral_bins(size_t bins);
	// The bins of the last render, the devices' shares combined by ownership mask: mean [height][width][bins] (row 0 = bottom), counts
	// [height][width][bins / 4] (optional), centres [bins] (optional): lambda_min + (b + 0.5) * bin_width in binary32.  After render_wait().
	void spectral_image(std::vector<float>* mean, std::vector<uint32_t>* counts = nullptr, std::vector<float>* centres = nullptr);
	void save_spectral_image(const std::string& path); // spectral_image's mean as a .npy file (image_io.hpp save_npy_f32)

	// Error bars for the bins (include/ssx.h "Spectral moments and region probes").  set_spectral_moments: every device also keeps the second moments of the hero
	// fluxes, for the renders that follow (after set_spectral_bins; not while rendering).
	void set_spectral_moments(bool on);
	// The variance of every bin mean, [height][width][bins] (row 0 = bottom; +inf where a sub-bin holds fewer than two samples), the devices' shares combined by
	// ownership mask.  After render_wait() of a render that started with the moments on.
	std::vector<float> spectral_variance();
	void save_spectral_variance(const std::string& path); // ... as a .npy file in spectral_image's layout
	// The pooled spectra of labelled sets of pixels: labels [height][width] (row 0 = bottom), 0..regions-1 a region (at most 32), 255 none.  SS, NN, VV, UU
	// [regions][bins] as the header defines them, reduced on the device in a fixed order; mean and std_err derived from them (image_io.hpp probe_derive).  One
	// device: ssx_spectral_probe.  Several: S, Q and N of the levelled devices merged by ownership, then ssx_probe_arrays on device 0 -- the same bits.
	struct Probe { size_t regions = 0, bins = 0; float lambda_min = 0.0f, bin_width = 0.0f; std::vector<double> SS, VV, mean, std_err; std::vector<uint64_t> NN, UU; };
	Probe probe(const std::vector<uint8_t>& labels, size_t regions);
	void save_probe_csv(const std::string& path, const Probe& probe) const; // image_io.hpp save_probe_csv
	// labels for probe(): region r = the half-open rectangle rects[r] = {x0, y0, x1, y1} (row 0 = bottom); where two overlap the later one wins.  Throws for an
	// empty rectangle or one that leaves the image, and for more than 32.
	std::vector<uint8_t> labels_from_rects(const std::vector<std::array<size_t, 4>>& rects) const;

	// The spectral noise figure (include/ssx.h "Spectral noise figure"): mask [height][width] (row 0 = bottom; nonzero = in), empty = every pixel.  EV, EM, PP, PU
	// [bins] as the header defines them, reduced on the device in a fixed order; noise, coverage and rel derived from them (image_io.hpp spectral_noise_derive).
	// One device: ssx_spectral_noise.  Several: level_devices(), every device's tile partials merged by ownership, then ssx_spectral_noise_reduce on device 0 --
	// the same bits.  After render_wait() of a render that started with the moments on.
	struct SpectralNoise { size_t bins = 0; float lambda_min = 0.0f, bin_width = 0.0f; std::vector<double> EV, EM, rel; std::vector<uint64_t> PP, PU; double noise = 0.0, coverage = 0.0; };
	SpectralNoise spectral_noise(const std::vector<uint8_t>& mask = {});
	void save_spectral_noise_csv(const std::string& path, const SpectralNoise& n) const; // image_io.hpp save_spectral_noise_csv
	// a mask for spectral_noise(): the union of the half-open rectangles {x0, y0, x1, y1} (row 0 = bottom).  Throws for an empty one or one that leaves the image.
	std::vector<uint8_t> mask_from_rects(const std::vector<std::array<size_t, 4>>& rects) const;
	// Renders until the bins are converged: switches the moments on (spectral output must be on: set_spectral_bins), starts with `step` samples per pixel and
	// continues `step` at a time, reads spectral_noise(mask) after EVERY step, the first included, and stops at the first noise <= target && coverage >=
	// min_coverage, at max_spp, or when tick() returns true (render_until's tick).  min_coverage is the user's parameter, not a tolerance: it keeps a render with
	// many bins from stopping on the few sub-bins that happen to hold two samples after one step; 1.0 is legal but slow to reach -- it needs two samples in every
	// sub-bin of every pixel.  A NaN figure (a non-finite flux, an empty mask) never stops the render: it runs to max_spp.  Returns the count and the last
	// figure read (NaN when the first step was stopped by tick).  Deterministic: the decision reads only S, Q and N.
	// resume: the render goes on from what the devices hold -- a load_checkpoint that took the moments up (moments_resumed()), or an earlier run of this loop --
	// instead of starting over: nothing is reset, valid moments are required (HostError SSX_ERR_STATE otherwise), and the figure is read BEFORE the first step: a
	// resumed render that already meets the target renders nothing.  Then `step` at a time as above: from a count that is a multiple of `step` the loop reads the
	// figure at the counts an uninterrupted run reads it at, and ends on the same bits.
	struct UntilSpectral { size_t spp = 0; double noise = 0.0, coverage = 0.0; };
	UntilSpectral render_until_spectral(double target, size_t step, size_t max_spp, const std::vector<uint8_t>& mask = {}, double min_coverage = 0.99, const std::function<bool()>& tick = {},
	                                    bool resume = false);

	// Comparing this render with another, bin by bin (include/ssx.h "Comparing two spectral renders"): A is what the devices hold, B the bins, counts and second
	// moments of `other` (checkpoint_load of a file written with the moments on: "SSXCKPT3"); labels and regions as probe() takes them; t2 the squared z
	// threshold.  DD, VV, X2, CC, NC, EX [regions][bins] as the header defines them, reduced on the device in a fixed order, and the figures derived from them
	// (image_io.hpp compare_derive); with `maps` also diff and var [height][width][bins].  One device: ssx_spectral_compare.  Several: level_devices(), S, Q and N
	// merged by ownership, then ssx_spectral_compare_arrays on device 0 -- the same bits.  After render_wait() of a render that started with the moments on.  The
	// two renders must have independent samples (different seeds) for z to mean anything.
	struct Compare {
		size_t regions = 0, bins = 0; float lambda_min = 0.0f, bin_width = 0.0f;
		std::vector<double> DD, VV, X2, mean_diff, std_err, z, chi2, exceed, coverage; std::vector<uint64_t> CC, NC, EX;
		std::vector<float> diff, var;
	};
	Compare compare_spectral(const Checkpoint& other, const std::vector<uint8_t>& labels, size_t regions, double t2, bool maps = false);
	void save_compare_csv(const std::string& path, const Compare& c) const; // image_io.hpp save_compare_csv
	void save_compare_map(const std::string& path, const Compare& c);       // zmap = diff / sqrt(var) (image_io.hpp compare_zmap) as a .npy file in spectral_image's layout


	// Denoising (include/ssx.h: first-hit guide buffers and the variance-guided a-trous filter).
	struct Guides { std::vector<uint32_t> prim; std::vector<float> depth, normal, albedo; }; // [height][width] x {1, 1, 3, 4}, row 0 = bottom; prim 0xFFFFFFFF = miss
	Guides guides();                                  // ssx_guides of device 0 at the options' resolution (they depend on the scene and the size only)
	void save_guides(const std::string& path);        // float32 [height][width][9] = {prim (-1: miss), depth, normal xyz, albedo 0..3} as a .npy file
	struct DenoiseParams { uint32_t levels = 5; float sigma_l = 1.0f, sigma_a = 0.1f; };
	// The image of the render so far, filtered.  Needs set_noise_estimate(true) before a render of at least two launches; after render_wait().  One device:
	// ssx_denoise, all on the device.  Several: the devices' images and variances combined by ownership (render_wait, noise), then ssx_denoise_images on
	// device 0 -- the same bits.  xyza_out (optional): the filtered XYZ + alpha behind the returned sRGB framebuffer.  Nothing the devices hold changes.
	Framebuffer denoise(const DenoiseParams& params, std::vector<float>* xyza_out = nullptr);
	// The wavelength bins of the render so far, filtered with the weights denoise() applies to the image (include/ssx.h "Denoising the spectral bins"):
	// *bins [height][width][B], the ratio of the filtered per-bin sums to the filtered sample counts.  Needs what denoise() needs, and set_spectral_bins before
	// the render.  One device: ssx_denoise_spectral, all on the device.  Several: the devices' sums, counts, images and variances combined by ownership, the
	// channels e0 built here by the header's formula, ssx_denoise_channels on device 0, the ratio formed here -- the same bits.  Returns the filtered image,
	// which is denoise()'s (xyza_out as there).  Nothing the devices hold changes.
	// demod (optional): the demodulated mode (include/ssx.h "Demodulated denoising") -- bins, image and variance divided by the first-hit albedo before the filter
	// and multiplied by it afterwards; params.sigma_a is ignored then.  One device: ssx_denoise_spectral_demod, all on the device.  Several: as above, with the
	// albedo bins of device 0 (ssx_albedo_bins; they do not depend on ownership), the channel albedo through ssx_develop_images, the divide and the multiply here by
	// the header's formulas and ssx_denoise_channels with a zero albedo guide between them -- the same bits.
	struct DemodParams { uint32_t supersample = 2; float albedo_floor = SSX_DEMOD_DEFAULT_FLOOR; std::vector<float> weights_xyz; }; // weights_xyz [3][B]; empty: the develop weights of the render's own observer
	Framebuffer denoise_spectral(const DenoiseParams& params, std::vector<float>* bins, std::vector<float>* xyza_out = nullptr, const DemodParams* demod = nullptr);
	// ssx_albedo_bins of device 0 at the options' resolution: [height][width][bins], row 0 = bottom; supersample x supersample rays per pixel (1, 2 or 4)
	std::vector<float> albedo_bins(size_t bins, uint32_t supersample = 2);
	void save_albedo_bins(const std::string& path, size_t bins, uint32_t supersample = 2); // ... as a .npy file
	void save_spectral_image(const std::string& path, const std::vector<float>& bins); // a [height][width][B] array, e.g. denoise_spectral's, in spectral_image's .npy layout

	// Developing the bins (include/ssx.h "Developing the spectral bins"): weights [channels][B] (host/develop.hpp builds them) -> [height][width][channels], row 0 =
	// bottom.  denoise == nullptr: the raw source -- every device develops its own pixels (ssx_spectral_develop) and the shares are combined by ownership mask.
	// Otherwise the denoised source: one device runs ssx_spectral_develop with the parameters, all on the device; several follow denoise_spectral's path and
	// then ssx_develop_images on device 0.  Either way the same bits as one device.  After render_wait(); nothing the devices hold changes.
	// demod (with denoise): the bins filtered in the demodulated mode -- one device: ssx_spectral_develop_demod; several: denoise_spectral's path as above.
	// optics (include/ssx.h "Developing through a lens"): the source goes through the lens before it is developed.  One device and no demodulated source:
	// ssx_spectral_develop_optics, all on the device.  Otherwise the host gathers q by its existing gather (every pixel's sums from the device that owns it, q = (float)((S *
	// M) / n); the denoised source by denoise_spectral's path), then ssx_optics_images and ssx_develop_images on device 0: the same bits.
	struct Optics { float cx = NAN, cy = NAN; uint32_t max_radius = 0; std::vector<float> scale; std::vector<uint32_t> radius; std::vector<float> taps; }; // a NaN centre: the image's middle; scale, radius [B], taps [B][2 R + 1]
	// defocus (include/ssx.h "Depth of field after the render"): the source is defocused with the depth guide first, then goes through the lens if there is one.
	// One device and no demodulated source: ssx_spectral_develop_lens.  Otherwise q by the same gather, then ssx_defocus_images with guides().depth (the guides
	// do not depend on ownership), ssx_optics_images and ssx_develop_images on device 0: the same bits.
	struct Defocus { uint32_t max_radius = 0; float gain = 0.0f; std::vector<float> focus; }; // R, K and f_b [B] of ssx_defocus_params (ssh_defocus_thin_lens makes them)
	std::vector<float> develop(const float* weights, size_t channels, const DenoiseParams* denoise = nullptr, const DemodParams* demod = nullptr, const Optics* optics = nullptr,
	                           const Defocus* defocus = nullptr);
	// the aperture as a pure function on q [height][width][B] and depth [height][width] of the options' size (ssx_defocus_images on device 0)
	std::vector<float> defocus_images(const float* q, const float* depth, const Defocus& defocus);
	// the lens as a pure function on q [height][width][B] of the options' size (ssx_optics_images on device 0)
	std::vector<float> optics_images(const float* q, const Optics& optics);
	// Glare (include/ssx.h "Glare: per-bin convolution by FFT"): behind the aperture and the lens every `on` bin is convolved with its own point spread function,
	// then developed.  One device and no demodulated source: ssx_spectral_develop_glare, all on the device.  Otherwise q by develop()'s gather, then
	// ssx_defocus_images, ssx_optics_images, ssx_glare_images and ssx_develop_images on device 0: the same bits.  weights NULL with channels 0: no development,
	// the result is empty.  bins_out: the bins behind the glare [height][width][B].
	struct Glare { // ssx_glare_params (ssh_glare_aperture, ssh_glare_plan, ssh_glare_twiddles make them); on [B], psf [B][2 R + 1][2 R + 1], twiddles [px / 2][2], [py / 2][2]
		uint32_t radius = 0, px = 0, py = 0;
		std::vector<uint8_t> on;
		std::vector<float> psf, twiddle_x, twiddle_y;
	};
	std::vector<float> develop_glare(const float* weights, size_t channels, const Glare& glare, const DenoiseParams* denoise = nullptr, const DemodParams* demod = nullptr,
	                                 const Optics* optics = nullptr, const Defocus* defocus = nullptr, std::vector<float>* bins_out = nullptr);
	// the glare as a pure function on q [height][width][B] of the options' size (ssx_glare_images on device 0)
	std::vector<float> glare_images(const float* q, const Glare& glare);
	// Developing onto a sensor (include/ssx.h "Developing onto a sensor"): behind the aperture and the lens the bins fall on a colour filter array, are counted,
	// digitised and demosaiced.  One device and no demodulated source: ssx_spectral_develop_sensor, all on the device.  Otherwise q by develop()'s gather, then
	// ssx_defocus_images, ssx_optics_images, ssx_sensor_images and ssx_demosaic_images on device 0: the same bits.
	struct Sensor { // ssx_sensor_params (ssh_sensor_bayer, ssh_sensor_exposure, ssh_sensor_ccm make them); weights [3][B], taps [4][3][25], ccm [3][3]
		uint32_t cfa[4] = { 0, 1, 1, 2 }; uint32_t noise = 0, seed = 0, frame = 0;
		float exposure = 1.0f, inv_exposure = 1.0f, read_var = 0.0f, dn_per_e = 1.0f, e_per_dn = 1.0f, black = 0.0f, white = 0.0f;
		std::vector<float> weights, taps, ccm;
	};
	struct SensorImage { std::vector<float> out, raw, dn; }; // [height][width][3], the mosaic [height][width], the ADC's numbers [height][width] (empty without an ADC)
	// glare: the bins behind the glare (develop_glare's bins_out) fall on the sensor by way of ssx_sensor_images and ssx_demosaic_images on device 0
	SensorImage develop_sensor(const Sensor& sensor, const DenoiseParams* denoise = nullptr, const DemodParams* demod = nullptr, const Optics* optics = nullptr,
	                           const Defocus* defocus = nullptr, const Glare* glare = nullptr);
	// the two stages as pure functions on arrays of the options' size (ssx_sensor_images, ssx_demosaic_images on device 0); dn may be NULL
	std::vector<float> sensor_images(const float* q, const Sensor& sensor, std::vector<float>* dn = nullptr);
	std::vector<float> demosaic_images(const float* raw, const Sensor& sensor);
	// Finishing a development for a display (include/ssx.h "Finishing a development for a display"): the three stages as pure functions on images [height][width][3]
	// of the options' size (ssx_meter_images, ssx_local_images, ssx_tone_images on device 0), and finish(), which chains them with the host's policy
	// (ssh_meter_derive, ssh_tone_curve) exactly as the Python Renderer.finish does: the same bits.
	struct Meter { std::vector<uint32_t> hist, special; };     // [4][SSX_METER_KEYS], [4][4]
	struct Local { uint32_t radius = 4; float exposure = 1.0f, y_lo = 0x1p-20f, y_hi = 0x1p20f, eps = 0.25f, pivot = 0.0f, compress = 1.0f, boost = 1.0f; };
	struct Tone { uint32_t shift = 19; float lo = 0x1p-12f, hi = 16.0f; float gains[3] = { 1.0f, 1.0f, 1.0f }; float matrix[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }; std::vector<float> curve; };
	enum class WhiteBalance { None, Grey, WhitePatch };
	struct Display { // what --develop-display and its companions say; matrix [c'][c]: the image's channels -> linear sRGB
		int curve = 1;                                         // SSH_TONE_CLIP / _REINHARD / _FILMIC
		double key = 0.18, white_percentile = 0.99;
		WhiteBalance wb = WhiteBalance::None;
		bool local = false; uint32_t radius = 4; float compress = 0.5f, boost = 1.0f, eps = 0.25f;
		float matrix[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
	};
	// the luminance the display sees: the BT.709 row times the matrix, binary64, rounded once (simple_spectral_amd/renderer.py display_luma)
	static void display_luma(const float matrix[9], float luma[3]);
	Meter meter_images(const float* img, const float luma[3], const uint8_t* mask = nullptr);
	std::vector<float> local_images(const float* img, const float luma[3], const Local& local, std::vector<float>* base = nullptr);
	std::vector<float> tone_images(const float* img, const Tone& tone, const float* local = nullptr);
	// display-encoded [height][width][3] in 0..1 (the curve holds the sRGB transfer function: nothing further is to be applied); meter: what was metered
	std::vector<float> finish(const float* img, const Display& display, Meter* meter = nullptr);

	// The colour difference of two developments of this render (include/ssx.h "Colour difference of two developments"): the six [regions][2] arrays (metric 0
	// dE*ab, 1 dE00), the five derived figures (image_io.hpp delta_e_derive) and, with `maps`, de [height][width][2].  A side is its [3][bins] weights (xyz space)
	// and whether the bins are filtered first (then `denoise`, and `demod` for the demodulated mode, say how -- for both sides alike).  labels empty: the whole
	// image is region 0 and regions must be 1.  One device and no demodulated side: ssx_spectral_delta_e.  Otherwise each side through develop() -- every pixel
	// from the device that owns it -- then ssx_delta_e_images on device 0: the same bits.  The whites are the caller's (they set the absolute size of every dE).
	struct DeltaESide { const float* weights = nullptr; bool denoised = false; const Optics* optics = nullptr; const Defocus* defocus = nullptr; const Glare* glare = nullptr; }; // optics, defocus, glare: the side seen through a lens, with an aperture (develop), behind a glare (develop_glare)
	struct DeltaE {
		size_t regions = 0;
		std::vector<double> SUM, SSQ, mean, rms, max, exceed, coverage; std::vector<float> MAX; std::vector<uint64_t> NF, NX, EX;
		std::vector<float> de;
	};
	DeltaE delta_e(const DeltaESide& side_a, const DeltaESide& side_b, const double white_a[3], const double white_b[3], const std::vector<uint8_t>& labels, size_t regions,
	               const double t[2], bool maps = false, const DenoiseParams* denoise = nullptr, const DemodParams* demod = nullptr);
	// ... of two XYZ images [height][width][3] of the options' size, as a pure function (ssx_delta_e_images on device 0)
	DeltaE delta_e_images(const float* xyz_a, const float* xyz_b, const double white_a[3], const double white_b[3], const std::vector<uint8_t>& labels, size_t regions,
	                      const double t[2], bool maps = false);
	void save_delta_e_csv(const std::string& path, const DeltaE& d) const; // image_io.hpp save_delta_e_csv
	void save_delta_e_map(const std::string& path, const DeltaE& d);       // de as a float32 .npy file [height][width][2], row 0 = bottom

private:
	struct Api;
	std::unique_ptr<Api> api_;
	std::vector<ssx_ctx*> ctxs_;
	std::chrono::steady_clock::time_point time_start_;
	bool started_ = false;
	bool need_join_ = false;    // a worker of every context is running or waits to be joined
	size_t spectral_bins_ = 0;
	bool spectral_moments_ = false; // set_spectral_moments is in force (switching the bins off switches it off)
	bool moments_resumed_ = false;  // the last load_checkpoint took the second moments up
	// ssx_spectral_variance's q of every device merged by ownership (the devices level): Q [height][width][bins]
	std::vector<double> gather_moments_();
	std::vector<float> source_bins_(const DenoiseParams* denoise, const DemodParams* demod); // q [height][width][B] on the host: the raw source from every pixel's owner, or denoise_spectral's
	std::vector<float> demod_weights_(const DemodParams& demod) const; // demod.weights_xyz, or the render's own observer's develop weights over the bins
	size_t expected_spp_ = 0;   // the count the running (or last) call renders to: what render_wait compares ssx_done_spp with
	ssx_render_params params_for_(size_t d, size_t spp, size_t spp_per_launch) const;
	ssx_sums_info_t owner_(size_t d) const; // device d's ownership (tile_first / tile_stride / tile_skew), as the merges by ownership take it
	uint32_t w32_() const { return static_cast<uint32_t>(options.res[0]); } // the options' resolution as the C ABI takes it
	uint32_t h32_() const { return static_cast<uint32_t>(options.res[1]); }
	// The two gathers of the several-device routes (renderer.cpp).  What the pure filter calls take besides the image, after level_devices(): the
	// devices' variances combined and in image units, and the guides.
	struct FilterInputs { std::vector<float> var; Guides guides; };
	FilterInputs filter_inputs_();
	// ssx_spectral_read of every device merged by ownership into the arrays asked for (the library's means | the raw sums | the counts); device 0's info
	ssx_spectral_info_t gather_bins_(std::vector<float>* mean, std::vector<double>* sums, std::vector<uint32_t>* counts);
	// denoise_spectral's several-device route: the filtered bins, and the filtered image in `out`
	std::vector<float> denoise_spectral_devices_(const ssx_denoise_params& dp, const DemodParams* demod, const std::vector<float>& wc, std::vector<float>& out);
	void start_(size_t spp, size_t spp_per_launch);
	void wait_workers_();
	void continue_each_(const std::vector<std::pair<ssx_ctx*, uint32_t>>& more);
	void continue_to_(size_t target);
	void check_(int rc, const char* what, ssx_ctx* c) const;
};

} // namespace ssx

// main.cpp -- the reference's command line (src/main.cpp:33-162) over the MI355X core.
//   simple-spectral --scene=cornell-srgb -w=512 -h=512 -spp=256 --output=out.png [--indirect-only]
// Flags, aliases, defaults and messages follow the reference (note: -h is HEIGHT, there is no
// --help; `name=value` or bare flags; unknown arguments produce a warning).  Additive options,
// long names only so that none collides: --gpus=N --seed=S --observer=1931|2006 --texture=PATH
// --light-scale=X --data-dir=DIR --uplift=ours|meng|jh --jh-coeff=FILE --meng-grid=FILE --no-explicit-light-sampling --no-flat-field-correction --tile-major --reduce=peer|rccl --rgb.
// Progressive rendering (not with --tile-major): --checkpoint=PATH writes the pixel sums at the end of the render and on abort -- and, with --spectral-output,
// --develop-output or --spectral-denoise, the wavelength bins behind them; --resume=PATH
// takes them up again, -spp then being the TOTAL wanted (at or below the checkpoint's count: the image is written as it is);
// --noise-target=X --max-samples=N [--noise-step=S] renders in steps of S samples until the noise estimate falls to X or N samples are done.
// Spectral output: --spectral-output=PATH.npy [--spectral-bins=N, default 16] also writes the per-pixel wavelength bins (include/ssx.h), a NumPy file of
// shape (height, width, N), row 0 = bottom, after the image.  Not with --tile-major, --rgb or --libm=glibc-2.35.  With --resume the checkpoint must hold the bins
// (it was written with one of the spectral options): N then defaults to the checkpoint's count, and another N, a checkpoint without bins or an unreadable one is
// refused before anything renders.
// Denoising: --denoise [--denoise-levels=N, 1..6, default 5] [--denoise-sigma=L,A, default 1,0.1] writes the image filtered by the variance-guided a-trous filter
// of include/ssx.h to --output instead of the plain one.  It switches the noise estimate on and renders in launches of --noise-step samples (ceil(spp / 8) when
// that is not given), so that the estimate has its two batches; not with -spp=1 or --tile-major.  --guides-output=PATH.npy writes the first-hit guide buffers,
// float32 (height, width, 9) = {primitive (-1: none), depth, normal xyz, albedo 0..3}, row 0 = bottom.
// --spectral-denoise (with --spectral-output): the file holds the bins filtered with the weights of that filter (include/ssx.h "Denoising the spectral bins").  It
// renders as --denoise does (noise estimate on, the same launch rule and refusals) and takes --denoise-levels and --denoise-sigma; the output image is the
// filtered one only if --denoise is given too.
// Developing the bins (include/ssx.h "Developing the spectral bins"): --develop-output=PATH with --spectral-bins=N writes the image developed from the bins on the
// device -- through the same XYZ -> sRGB store and writers as --output -- under --develop-observer=1931|2006 (default: the render's), through --develop-filter=FILE.csv
// (--develop-lens=lateral,sigma,axial[,lambda_ref] with --develop-lens-radius=R puts a lens in front: include/ssx.h "Developing through a lens";
// --develop-defocus=aperture,focus_distance[,axial[,lambda_ref]] with --develop-defocus-radius=R gives it an aperture: "Depth of field after the render";
// --develop-glare=blades,ring_px,strength[,rotation[,lambda_ref]] with --develop-glare-radius=R puts an iris's diffraction behind the lens: "Glare: per-bin convolution by FFT";
// --develop-sensor=PATTERN[,mhc|bilinear] with --develop-sensor-curves / -exposure / -noise / -bits and --sensor-raw-output puts a sensor behind both: "Developing
// onto a sensor")
// (a spectrum in the format of data/*.csv, its range in the name: NAME-LOW+STEP+HIGH.csv) and relit by --develop-relight=NEW.csv (the emitters' spectrum replaced by
// NEW; refused unless all emissive materials share one spectrum up to a scale).  With --spectral-denoise the filtered bins are developed.  It does not need
// --spectral-output, and has its refusals (--tile-major, --rgb, --libm=glibc-2.35; --resume of a checkpoint without the bins).  With --resume, --spectral-bins may
// be left out: the checkpoint's count.
// Demodulated denoising (include/ssx.h "Demodulated denoising"): --demodulate[=K] with --spectral-denoise runs that filter on illumination -- bins, image and
// variance divided by the first-hit albedo per bin (K x K rays per pixel, K = 1, 2 or 4; default 2) before it and multiplied by it afterwards; the albedo part of
// --denoise-sigma is ignored then.  --albedo-output=PATH.npy (needs --spectral-bins=N) writes those albedo bins, [height][width][N] float32.
// Colour difference of two developments (include/ssx.h "Colour difference of two developments"), with --spectral-bins=N: --delta-e-output=PATH.npy writes the map
// float32 [height][width][2] (dE*ab, dE00), --delta-e-csv=PATH.csv one line per region and metric "region,metric,mean,rms,max,exceed,coverage,finite,nonfinite".
// Side A is the development --develop-observer / --develop-filter / --develop-relight / --spectral-denoise / --demodulate describe (these then do not need
// --develop-output), side B the one --delta-e-observer / --delta-e-filter / --delta-e-relight / --delta-e-denoise describe.  The whites are host policy and a
// viewing decision, like exposure -- they set the absolute size of every dE: chromaticity = the side's weights applied to its illuminant (the relight's, else the
// scene's emitter spectrum, else D65), one scale for both so that side A's mean finite Y is 0.18 of its white's Y, or --delta-e-white-y=Y as side A's white's Y.
// --delta-e-threshold=ab,00 (default 2.3,1): what "exceed" counts beyond.  Regions: the --probe rectangles, else the whole image.  Refused before anything
// renders with --rgb, --tile-major, --libm=glibc-2.35, --resume, or without --spectral-bins.
// Error bars for the bins (include/ssx.h "Spectral moments and region probes"), all with --spectral-bins=N: --spectral-variance-output=PATH.npy writes the variance
// of every bin mean, float32 [height][width][N] (+inf where a sub-bin holds fewer than two samples); --probe=x0,y0,x1,y1 (half-open, row 0 = bottom; up to 32 of
// them, region r = the r-th) with --probe-output=PATH.csv writes the pooled mean spectrum of each rectangle with its standard error, one line per region and bin:
// region, bin, centre wavelength, mean, stderr, samples, unestimated.  Not with --tile-major, --rgb or --libm=glibc-2.35.  --checkpoint then also keeps the bins'
// second moments behind them ("SSXCKPT3"), and --resume needs a checkpoint that holds them for the bin count in force (default: the checkpoint's count): one that
// cannot be read, has no bins, no moments or another count is refused before anything renders.
// A spectral stopping rule (include/ssx.h "Spectral noise figure"): --spectral-noise-target=X with --spectral-bins=N and --max-samples=K renders --noise-step
// samples per pixel at a time until the RMS standard error of the pixels' bin means, relative to the mean bin flux, is at most X and the share of sub-bins that
// hold two samples is at least --spectral-noise-coverage=C (default 0.99; 1.0 is legal but slow to reach), or K samples are done.  --spectral-noise-region=
// x0,y0,x1,y1 (half-open, row 0 = bottom, repeatable) restricts the figure to the union of the rectangles; --spectral-noise-output=PATH.csv writes it per bin:
// bin, centre wavelength, rel, EV, EM, estimable, unestimated.  One stopping rule per run: not with --noise-target; not with --tile-major, --rgb or
// --libm=glibc-2.35.  With --resume of a checkpoint that holds the second moments (as above) the rule goes on from the checkpoint's samples: the figure is read
// first -- a render that already meets the target renders nothing -- -spp is ignored as before and --max-samples caps the total.
// Comparing with another render (include/ssx.h "Comparing two spectral renders"): --compare-to=FILE.ckpt with --spectral-bins=N holds the finished render against
// the bins, counts and second moments of that checkpoint, pixel by pixel and bin by bin.  --compare-output=PATH.csv writes one line per region and bin: region, bin,
// centre wavelength, mean_diff, stderr, z, chi2, exceed, comparable, not_comparable; --compare-map-output=PATH.npy the signed per-pixel map diff / sqrt(var),
// float32 [height][width][N] (0 where a cell is not comparable); --compare-threshold=Z (default 3) is the z beyond which a cell counts into `exceed`.  The regions
// are the --probe rectangles (which then do not need --probe-output); without any the whole image is region 0.  It switches the second moments on.  Refused before
// anything renders: a checkpoint that cannot be read, holds no second moments, or has another size, bin count, lambda_min or bin width; --tile-major, --rgb or
// --libm=glibc-2.35.  A checkpoint of the same seed only draws a warning: the samples are then not independent and z is not calibrated.
#include "renderer.hpp"

#include "checkpoint.hpp"
#include "develop.hpp"
#include "image_io.hpp"
#include "../../include/ssx_host.h"

#include <array>
#include <chrono>
#include <csignal>
#include <cmath>
#include <cstring>
#include <memory>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

namespace {

void print_usage() {
	std::printf(
		"Simple Spectral: a simple spectral renderer for demonstration purposes\n"
		"  Required arguments:\n"
		"    `--scene=<name>`/`-s=<name>`\n"
		"          Render the given built-in scene (valid scenes: \"cornell\", \"cornell-srgb\", \"plane-srgb\").\n"
		"    `--width=<width>`/`-w=<width>`\n"
		"          Set the width of the render.\n"
		"    `--height=<height>`/`-h=<height>`\n"
		"          Set the height of the render.\n"
		"    `--samples=<samples>`/`-spp=<samples>`\n"
		"          Set the number of samples per pixel.\n"
		"    `--output=<output-image-path>`/`-o=<output-image-path>`\n"
		"          Set the path to the output image (.csv, .hdr, .pfm, else PNG).\n"
		"  Optional arguments:\n"
		"    `--indirect-only`/`-io`\n"
		"          Render only indirect illumination.\n"
		"  MI355X build:\n"
		"    `--gpus=<n>` `--seed=<n>` `--observer=1931|2006` `--uplift=ours|meng|jh` `--jh-coeff=<file>` `--meng-grid=<file>` `--rgb` `--no-explicit-light-sampling` `--no-flat-field-correction` `--tile-major` `--reduce=peer|rccl` `--libm=build|glibc-2.35`\n"
		"    `--texture=<png>` `--light-scale=<x>` `--data-dir=<dir>`\n"
		"    `--checkpoint=<file>` `--resume=<file>` (`-spp` is then the total) `--noise-target=<x> --max-samples=<n> [--noise-step=<s>]`\n"
		"    `--spectral-output=<file.npy>` [`--spectral-bins=<n>`: 4, 8, ..., 64; default 16, with `--resume` the checkpoint's]\n"
		"          (`--checkpoint` then also keeps the wavelength bins, and `--resume` needs a checkpoint that holds <n> of them)\n"
		"    `--denoise` [`--denoise-levels=<n>`: 1..6; default 5] [`--denoise-sigma=<l>,<a>`; default 1,0.1] (the output image is the filtered one; not with `-spp=1`)\n"
		"    `--guides-output=<file.npy>` (first hit per pixel: primitive, depth, normal, albedo)\n"
		"    `--spectral-denoise` (with `--spectral-output`: the file holds the bins filtered with `--denoise`'s weights, levels and sigmas; not with `-spp=1`)\n"
		"    `--develop-output=<image>` (needs `--spectral-bins=<n>`) [`--develop-observer=1931|2006`] [`--develop-filter=<name-low+step+high.csv>`] [`--develop-relight=<new.csv>`]\n"
		"          (the image developed from the wavelength bins; with `--spectral-denoise` from the filtered bins)\n"
		"    [`--develop-lens=<lateral>,<sigma>,<axial>[,<lambda_ref=550>]`] [`--develop-lens-radius=<0..12, default 8>`] [`--delta-e-lens=...`]\n"
		"          (the bins through a lens before they are developed: lateral chromatic aberration, a blur of <sigma> pixels at <lambda_ref> growing with the\n"
		"           wavelength, <axial> pixels of defocus per relative wavelength offset; for `--develop-output` and side A of `--delta-e-*`, `--delta-e-lens` for side B)\n"
		"    [`--develop-glare=<blades>,<ring_px>,<strength>[,<rotation=0>[,<lambda_ref=550>]]`] [`--develop-glare-radius=<0..256, default 64>`] [`--delta-e-glare=...`]\n"
		"          (veiling glare and diffraction behind the lens: every bin convolved with the far-field pattern of an iris of <blades> blades (fewer than 3: a\n"
		"           disc), a disc's first dark ring <ring_px> pixels out at <lambda_ref> and growing with the wavelength, <strength> of the light leaving the\n"
		"           geometric image, the iris turned by <rotation> radians; sides as for `--develop-lens`)\n"
		"    [`--develop-display=clip|reinhard|filmic[,<key=0.18>[,<white_percentile=0.99>]]`] [`--develop-display-local=<radius 1..32>,<compress>[,<boost=1>[,<eps=0.25>]]`]\n"
		"    [`--develop-display-wb=none|grey|white-patch`] [`--meter-output=<hist.csv>`]\n"
		"          (finish `--develop-output` for a display: the image is metered, exposed for a log-average of <key>, its <white_percentile> taken as white, large-scale\n"
		"           contrast compressed about the key with detail kept, and a tone curve with the sRGB transfer function applied; `--meter-output` writes the metering)\n"
		"    [`--develop-defocus=<aperture>,<focus_distance>[,<axial=0>[,<lambda_ref=550>]]`] [`--develop-defocus-radius=<0..12, default 8>`] [`--delta-e-defocus=...`]\n"
		"          (depth of field from the depth guide before the lens: an aperture of diameter <aperture> focused at <focus_distance>, both in scene units, the\n"
		"           inverse focus distance moving by <axial> per relative wavelength offset; sides as for `--develop-lens`)\n"
		"    [`--develop-sensor=<RGGB|BGGR|GRBG|GBRG>[,mhc|bilinear]`] [`--develop-sensor-curves=<R.csv>,<G.csv>,<B.csv>`] [`--develop-sensor-exposure=<full_well=15000>,<white_level=1>`]\n"
		"    [`--develop-sensor-noise=<read_e>[,<seed=0>]`] [`--develop-sensor-bits=<1..24>[,<black=0>]`] [`--sensor-raw-output=<raw.npy>`]\n"
		"          (behind the aperture and the lens the bins fall on a Bayer sensor -- the pattern's first two letters are the bottom row -- are counted with shot and\n"
		"           read noise, digitised and demosaiced; `--develop-output` then writes the demosaiced image.  Without curves: three Gaussian stand-ins, no camera's.\n"
		"           `--develop-sensor-curves` on its own: an ordinary develop with the camera's curves in the observer's place)\n"
		"    `--demodulate[=1|2|4]` (with `--spectral-denoise`: filter illumination -- divide by the first-hit albedo per bin, <k> x <k> rays per pixel, before; multiply after)\n"
		"    `--albedo-output=<file.npy>` (needs `--spectral-bins=<n>`: the first-hit albedo per wavelength bin)\n"
		"    `--spectral-variance-output=<file.npy>` (needs `--spectral-bins=<n>`: the variance of every bin mean)\n"
		"          (with this, `--probe` or `--spectral-noise-target`, `--checkpoint` also keeps the bins' second moments, and `--resume` needs a checkpoint that holds them)\n"
		"    `--probe=<x0>,<y0>,<x1>,<y1>` (up to 32) `--probe-output=<file.csv>` (need `--spectral-bins=<n>`: each rectangle's pooled spectrum with its standard error)\n"
		"    `--spectral-noise-target=<x> --spectral-bins=<n> --max-samples=<k> [--noise-step=<s>]` [`--spectral-noise-coverage=<c>`; default 0.99]\n"
		"          [`--spectral-noise-region=<x0>,<y0>,<x1>,<y1>` ...] [`--spectral-noise-output=<file.csv>`] (render until the wavelength bins are converged)\n"
		"    `--compare-to=<file.ckpt>` (needs `--spectral-bins=<n>`) [`--compare-output=<file.csv>`] [`--compare-map-output=<file.npy>`] [`--compare-threshold=<z>`; default 3]\n"
		"          (the render against another one's checkpoint, bin by bin, with error bars and z-scores; regions: the `--probe` rectangles, else the whole image)\n"
		"    `--delta-e-output=<file.npy>` `--delta-e-csv=<file.csv>` (need `--spectral-bins=<n>`) [`--delta-e-observer=1931|2006`] [`--delta-e-filter=<file.csv>`] [`--delta-e-relight=<file.csv>`]\n"
		"          [`--delta-e-denoise`] [`--delta-e-threshold=<ab>,<00>`; default 2.3,1] [`--delta-e-white-y=<Y>`; default: side A's mean Y is 0.18 of it]\n"
		"          (CIELAB dE*ab and CIEDE2000 between two developments of the render: side A as `--develop-*`, `--spectral-denoise` and `--demodulate` say, side B as these say;\n"
		"           the whites set the absolute size of every dE: a viewing decision, like exposure; regions: the `--probe` rectangles, else the whole image)\n");
}

struct ArgList {
	std::vector<std::string> args;
	// Finds `name=value` / `shortname=value` (returns value) or a bare flag (returns name) and
	// removes it from the list; false when absent.
	bool take(const std::string& name, const std::string& shortname, std::string* out) {
		for (auto it = args.begin(); it != args.end(); ++it) {
			const size_t eq = it->find('=');
			if (eq != std::string::npos) {
				const std::string key = it->substr(0, eq);
				if (key == name || (!shortname.empty() && key == shortname)) { *out = it->substr(eq + 1); args.erase(it); return true; }
			} else if (*it == name || (!shortname.empty() && *it == shortname)) {
				*out = name; args.erase(it); return true;
			}
		}
		return false;
	}
	std::string require(const std::string& name, const std::string& shortname) {
		std::string v;
		if (take(name, shortname, &v)) return v;
		std::fprintf(stderr, "Required argument `%s`", name.c_str());
		if (!shortname.empty()) std::fprintf(stderr, "/`%s`", shortname.c_str());
		std::fprintf(stderr, " not found!\n");
		throw -2;
	}
};

unsigned to_pos(const std::string& s) { // Str::to_pos (src/util/string.hpp:43-57)
	size_t used = 0;
	int v = 0;
	try { v = std::stoi(s, &used); } catch (...) { throw -1; }
	if (used != s.size()) throw -1;
	if (v <= 0) throw -2;
	return static_cast<unsigned>(v);
}

// `--probe` and `--spectral-noise-region`: a half-open rectangle x0,y0,x1,y1 inside a width x height image
std::array<size_t, 4> to_rect(const char* flag, const std::string& v, size_t width, size_t height) {
	std::array<size_t, 4> q{};
	bool ok = true;
	try {
		size_t at = 0;
		for (int k = 0; k < 4 && ok; ++k) {
			const size_t comma = k < 3 ? v.find(',', at) : v.size();
			if (comma == std::string::npos) { ok = false; break; }
			const std::string part = v.substr(at, comma - at);
			size_t used = 0;
			const long long n = std::stoll(part, &used);
			ok = used == part.size() && n >= 0;
			q[k] = static_cast<size_t>(n); at = comma + 1;
		}
	} catch (...) { ok = false; }
	if (!ok) { std::fprintf(stderr, "Invalid value for %s (<x0>,<y0>,<x1>,<y1>)!\n", flag); throw -2; }
	if (q[0] >= q[2] || q[1] >= q[3] || q[2] > width || q[3] > height) {
		std::fprintf(stderr, "`%s=%s` is empty or leaves the image: a rectangle is half-open, x0 < x1 <= width and y0 < y1 <= height (row 0 = bottom)!\n", flag, v.c_str());
		throw -2;
	}
	return q;
}

struct Progressive;
// `--resume` with an option that needs the second moments of the samples already rendered: the checkpoint has to hold them, for as many bins as are asked for
// (default: as many as it holds).  Refuses (throws -2) with the reason; otherwise the bin count in force is the file's.
void resume_needs_moments(const char* flag, Progressive* g);

struct Progressive { // the flags of the progressive modes
	std::string checkpoint, resume;
	double noise_target = -1.0; // < 0: none
	size_t max_samples = 0, noise_step = 16;
	std::string spectral_output; // --spectral-output: "" = none
	size_t spectral_bins = 16;
	bool denoise = false;        // --denoise
	bool spectral_denoise = false; // --spectral-denoise
	bool noise_step_given = false;
	ssx::Renderer::DenoiseParams denoise_params;
	std::string guides_output;   // --guides-output: "" = none
	std::string develop_output, develop_filter, develop_relight; // --develop-output / --develop-filter / --develop-relight: "" = none
	int develop_observer = 0;    // --develop-observer: 0 = the render's
	// the lens in front of the development (include/ssx.h "Developing through a lens"; ssh_optics_lens): --develop-lens=lateral,sigma,axial[,lambda_ref] for
	// --develop-output and side A of --delta-e-*, --delta-e-lens=... for side B, --develop-lens-radius=R (the largest blur radius, for both)
	struct Lens { bool on = false; double lateral = 0.0, sigma = 0.0, axial = 0.0, lambda_ref = 550.0; };
	Lens develop_lens, delta_e_lens;
	unsigned develop_lens_radius = 8;
	// the aperture (include/ssx.h "Depth of field after the render"; ssh_defocus_thin_lens): --develop-defocus=aperture,focus_distance[,axial[,lambda_ref]] and
	// --delta-e-defocus=... for the same sides, --develop-defocus-radius=R (the largest circle of confusion, for both)
	struct Aperture { bool on = false; double aperture = 0.0, focus_distance = 1.0, axial = 0.0, lambda_ref = 550.0; };
	Aperture develop_defocus, delta_e_defocus;
	unsigned develop_defocus_radius = 8;
	// the glare behind the lens (include/ssx.h "Glare: per-bin convolution by FFT"; ssh_glare_aperture): --develop-glare=blades,ring_px,strength[,rotation[,lambda_ref]]
	// and --delta-e-glare=... for the same sides, --develop-glare-radius=R (the psf's radius, for both)
	struct Iris { bool on = false; int blades = 0; double ring_px = 1.0, strength = 0.0, rotation = 0.0, lambda_ref = 550.0; };
	Iris develop_glare, delta_e_glare;
	unsigned develop_glare_radius = 64;
	// the finish for a display (include/ssx.h "Finishing a development for a display"): --develop-display=clip|reinhard|filmic[,key[,white_percentile]],
	// --develop-display-local=radius,compress[,boost[,eps]], --develop-display-wb=none|grey|white-patch, --meter-output=hist.csv
	bool display_on = false;
	ssx::Renderer::Display display;
	std::string meter_output;
	// the sensor (include/ssx.h "Developing onto a sensor"): --develop-sensor=PATTERN[,mhc|bilinear], --develop-sensor-curves=R.csv,G.csv,B.csv (also on its own: an
	// ordinary develop with a camera's curves), --develop-sensor-exposure=full_well,white_level, --develop-sensor-noise=read_e[,seed], --develop-sensor-bits=N[,black],
	// --sensor-raw-output=raw.npy
	struct SensorFlags {
		bool on = false, noise = false, exposure_given = false, bits_given = false;
		std::string pattern; int method = SSH_DEMOSAIC_MHC;
		std::vector<std::string> curves;                     // three paths, or none: the stand-in curves of ssx_host.h
		double full_well = 15000.0, white_level = 1.0, read_e = 0.0, black = 0.0;
		unsigned bits = 0, seed = 0;
		std::string raw_output;
	} sensor;
	bool spectral_bins_given = false;
	bool demodulate = false;     // --demodulate[=K]
	ssx::Renderer::DemodParams demod_params;
	std::string albedo_output;   // --albedo-output: "" = none
	std::string variance_output; // --spectral-variance-output: "" = none
	std::vector<std::array<size_t, 4>> probes; // --probe=x0,y0,x1,y1, in the order given
	std::string probe_output;    // --probe-output: "" = none
	bool moments() const { return !variance_output.empty() || !probe_output.empty() || !compare_to.empty(); } // what needs the second moments
	double spectral_noise_target = -1.0;   // --spectral-noise-target: < 0 = none
	double spectral_noise_coverage = 0.99; // --spectral-noise-coverage
	std::vector<std::array<size_t, 4>> spectral_noise_regions; // --spectral-noise-region=x0,y0,x1,y1: the mask is their union; none = every pixel
	std::string spectral_noise_output;     // --spectral-noise-output: "" = none
	std::string compare_to, compare_output, compare_map_output; // --compare-to / --compare-output / --compare-map-output: "" = none
	double compare_threshold = 3.0;        // --compare-threshold: Z; the library takes t2 = Z * Z
	// the colour difference of two developments (include/ssx.h "Colour difference of two developments"): side A is what --develop-*, --spectral-denoise and
	// --demodulate describe, side B what these do
	std::string delta_e_output, delta_e_csv, delta_e_filter, delta_e_relight; // --delta-e-output / --delta-e-csv / --delta-e-filter / --delta-e-relight: "" = none
	int delta_e_observer = 0;              // --delta-e-observer: 0 = the render's
	bool delta_e_denoise = false;          // --delta-e-denoise: side B from the filtered bins
	double delta_e_threshold[2] = { 2.3, 1.0 }; // --delta-e-threshold=ab,00: the customary just-noticeable differences; user parameters
	double delta_e_white_y = 0.0;          // --delta-e-white-y: 0 = side A's mean finite Y is 0.18 of the white's
	bool delta_e() const { return !delta_e_output.empty() || !delta_e_csv.empty(); }
	std::shared_ptr<ssx::Checkpoint> compare_other; // --compare-to's file, read when the arguments are checked
};

void resume_needs_moments(const char* flag, Progressive* g) {
	const char* const head = "`%s` cannot be combined with `--resume`: \"%s\" does not carry the second moments of the samples already rendered";
	ssx::Checkpoint ck;
	try { ck = ssx::checkpoint_load(g->resume); }
	catch (const ssx::HostError& e) {
		std::fprintf(stderr, head, flag, g->resume.c_str());
		std::fprintf(stderr, ": the checkpoint cannot be read: %s\n", e.message.c_str());
		throw -2;
	}
	const uint32_t held = ck.spectral.bins;
	if (!held || ck.moments.empty()) {
		std::fprintf(stderr, head, flag, g->resume.c_str());
		std::fprintf(stderr, !held ? ": it holds the pixel sums only, no wavelength bins (write it with `--checkpoint` and this option)!\n"
		                           : ": it holds %u wavelength bins without their second moments (write it with `--checkpoint` and this option)!\n", held);
		throw -2;
	}
	if (g->spectral_bins_given && g->spectral_bins != held) {
		std::fprintf(stderr, head, flag, g->resume.c_str());
		std::fprintf(stderr, " for another bin count: it holds %u wavelength bins, `--spectral-bins=%zu` was asked for!\n", held, g->spectral_bins);
		throw -2;
	}
	g->spectral_bins = held; g->spectral_bins_given = true;
}

void parse_arguments(int argc, char* argv[], ssx::Renderer::Options* o, Progressive* g) {
	ArgList a;
	for (int i = 0; i < argc; ++i) a.args.emplace_back(argv[i]);
	o->scene_name = a.require("--scene", "-s");
	if (o->scene_name != "cornell" && o->scene_name != "cornell-srgb" && o->scene_name != "plane-srgb") {
		std::fprintf(stderr, "Unrecognized scene \"%s\"!  (Supported scenes: \"cornell\", \"cornell-srgb\", \"plane-srgb\")\n", o->scene_name.c_str());
		throw -3;
	}
	const std::string sw = a.require("--width", "-w"), sh = a.require("--height", "-h");
	try { o->res[0] = to_pos(sw); o->res[1] = to_pos(sh); }
	catch (int) { std::fprintf(stderr, "Invalid width or height!\n"); throw; }
	const std::string sspp = a.require("--samples", "-spp");
	try { o->spp = to_pos(sspp); }
	catch (int) { std::fprintf(stderr, "Invalid number of samples!\n"); throw; }
	std::string v;
	o->indirect_only = a.take("--indirect-only", "-io", &v);
	if (o->indirect_only && v != "--indirect-only") { std::fprintf(stderr, "`--indirect-only`/`-io` does not take a value!\n"); throw -1; }
	o->output_path = a.require("--output", "-o");
	try {
		if (a.take("--gpus", "", &v)) o->gpus = static_cast<int>(to_pos(v));
		if (a.take("--seed", "", &v)) o->seed = std::stoull(v);
		if (a.take("--observer", "", &v)) o->observer = static_cast<int>(to_pos(v));
		if (a.take("--light-scale", "", &v)) o->light_scale = std::stof(v);
	} catch (...) { std::fprintf(stderr, "Invalid value for --gpus/--seed/--observer/--light-scale!\n"); throw -2; }
	if (a.take("--uplift", "", &v)) {
		if (v == "ours") o->uplift = 1; else if (v == "meng") o->uplift = 2; else if (v == "jh") o->uplift = 3;
		else { std::fprintf(stderr, "Invalid value for --uplift (ours|meng|jh)!\n"); throw -2; }
	}
	if (a.take("--jh-coeff", "", &v)) o->jh_coeff_path = v;
	if (a.take("--meng-grid", "", &v)) o->meng_grid_path = v;
	if (a.take("--rgb", "", &v)) o->rgb_mode = true;
	if (a.take("--no-explicit-light-sampling", "", &v)) o->explicit_light_sampling = false;
	if (a.take("--no-flat-field-correction", "", &v)) o->flat_field_correction = false;
	if (a.take("--tile-major", "", &v)) o->tile_major = true;
	if (a.take("--libm", "", &v)) {
		if (v == "build") o->libm = SSX_LIBM_BUILD; else if (v == "glibc-2.35") o->libm = SSX_LIBM_GLIBC_2_35;
		else { std::fprintf(stderr, "Invalid value for --libm (build|glibc-2.35)!\n"); throw -2; }
	}
	if (a.take("--reduce", "", &v)) {
		if (v == "rccl") o->reduce_rccl = true;
		else if (v != "peer") { std::fprintf(stderr, "Unrecognized --reduce \"%s\" (peer | rccl)\n", v.c_str()); throw -2; }
	}
	if (a.take("--checkpoint", "", &v)) g->checkpoint = v;
	if (a.take("--resume", "", &v)) g->resume = v;
	try {
		if (a.take("--noise-target", "", &v)) { size_t used = 0; g->noise_target = std::stod(v, &used); if (used != v.size() || !(g->noise_target >= 0.0)) throw -2; }
		if (a.take("--max-samples", "", &v)) g->max_samples = to_pos(v);
		if (a.take("--noise-step", "", &v)) { g->noise_step = to_pos(v); g->noise_step_given = true; }
	} catch (...) { std::fprintf(stderr, "Invalid value for --noise-target/--max-samples/--noise-step!\n"); throw -2; }
	if (o->tile_major && (!g->resume.empty() || !g->checkpoint.empty() || g->noise_target >= 0.0)) {
		std::fprintf(stderr, "`--resume`, `--checkpoint` and `--noise-target` cannot be combined with `--tile-major`: only a render that walks through the samples can be continued!\n");
		throw -2;
	}
	if (g->noise_target >= 0.0 && g->max_samples == 0) { std::fprintf(stderr, "`--noise-target` needs `--max-samples=<n>`!\n"); throw -2; }
	if (g->noise_target >= 0.0 && !g->resume.empty()) { std::fprintf(stderr, "`--noise-target` cannot be combined with `--resume`!\n"); throw -2; }
	if (a.take("--spectral-output", "", &v)) g->spectral_output = v;
	if (a.take("--develop-output", "", &v)) g->develop_output = v;
	if (a.take("--develop-filter", "", &v)) g->develop_filter = v;
	if (a.take("--develop-relight", "", &v)) g->develop_relight = v;
	if (a.take("--develop-observer", "", &v)) {
		if (v == "1931") g->develop_observer = 1931; else if (v == "2006") g->develop_observer = 2006;
		else { std::fprintf(stderr, "Invalid value for --develop-observer (1931|2006)!\n"); throw -2; }
	}
	auto take_lens = [&](const char* flag, Progressive::Lens* lens) {
		if (!a.take(flag, "", &v)) return;
		double x[4] = { 0.0, 0.0, 0.0, 550.0 };
		size_t n = 0, at = 0;
		bool ok = true;
		try {
			while (ok && n < 4) {
				const size_t comma = v.find(',', at);
				const std::string part = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
				size_t used = 0;
				x[n++] = std::stod(part, &used);
				ok = used == part.size() && std::isfinite(x[n - 1]);
				if (comma == std::string::npos) break;
				at = comma + 1;
				if (n == 4) ok = false;
			}
		} catch (...) { ok = false; }
		if (!ok || n < 3 || x[1] < 0.0 || !(x[3] > 0.0)) { std::fprintf(stderr, "Invalid value for %s (<lateral>,<sigma>,<axial>[,<lambda_ref>]: finite, sigma >= 0, lambda_ref > 0)!\n", flag); throw -2; }
		lens->on = true; lens->lateral = x[0]; lens->sigma = x[1]; lens->axial = x[2]; lens->lambda_ref = x[3];
	};
	take_lens("--develop-lens", &g->develop_lens);
	take_lens("--delta-e-lens", &g->delta_e_lens);
	bool lens_radius_given = false;
	if (a.take("--develop-lens-radius", "", &v)) {
		size_t r = 99;
		try { r = v == "0" ? 0 : to_pos(v); } catch (int) { r = 99; }
		if (r > SSX_OPTICS_MAX_RADIUS) { std::fprintf(stderr, "Invalid value for --develop-lens-radius (0..12)!\n"); throw -2; }
		g->develop_lens_radius = static_cast<unsigned>(r);
		lens_radius_given = true;
	}
	auto take_aperture = [&](const char* flag, Progressive::Aperture* ap) {
		if (!a.take(flag, "", &v)) return;
		double x[4] = { 0.0, 1.0, 0.0, 550.0 };
		size_t n = 0, at = 0;
		bool ok = true;
		try {
			while (ok && n < 4) {
				const size_t comma = v.find(',', at);
				const std::string part = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
				size_t used = 0;
				x[n++] = std::stod(part, &used);
				ok = used == part.size() && std::isfinite(x[n - 1]);
				if (comma == std::string::npos) break;
				at = comma + 1;
				if (n == 4) ok = false;
			}
		} catch (...) { ok = false; }
		if (!ok || n < 2 || x[0] < 0.0 || !(x[1] > 0.0) || !(x[3] > 0.0)) { std::fprintf(stderr, "Invalid value for %s (<aperture>,<focus_distance>[,<axial>[,<lambda_ref>]]: finite, aperture >= 0, focus_distance > 0, lambda_ref > 0)!\n", flag); throw -2; }
		ap->on = true; ap->aperture = x[0]; ap->focus_distance = x[1]; ap->axial = x[2]; ap->lambda_ref = x[3];
	};
	take_aperture("--develop-defocus", &g->develop_defocus);
	take_aperture("--delta-e-defocus", &g->delta_e_defocus);
	bool defocus_radius_given = false;
	if (a.take("--develop-defocus-radius", "", &v)) {
		size_t r = 99;
		try { r = v == "0" ? 0 : to_pos(v); } catch (int) { r = 99; }
		if (r > SSX_DEFOCUS_MAX_RADIUS) { std::fprintf(stderr, "Invalid value for --develop-defocus-radius (0..12)!\n"); throw -2; }
		g->develop_defocus_radius = static_cast<unsigned>(r);
		defocus_radius_given = true;
	}
	auto take_glare = [&](const char* flag, Progressive::Iris* iris) {
		if (!a.take(flag, "", &v)) return;
		double x[5] = { 0.0, 1.0, 0.0, 0.0, 550.0 };
		size_t n = 0, at = 0;
		bool ok = true;
		try {
			while (ok && n < 5) {
				const size_t comma = v.find(',', at);
				const std::string part = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
				size_t used = 0;
				x[n++] = std::stod(part, &used);
				ok = used == part.size() && std::isfinite(x[n - 1]);
				if (comma == std::string::npos) break;
				at = comma + 1;
				if (n == 5) ok = false;
			}
		} catch (...) { ok = false; }
		if (!ok || n < 3 || x[0] < 0.0 || x[0] > 64.0 || x[0] != std::floor(x[0]) || !(x[1] > 0.0) || x[2] < 0.0 || x[2] > 1.0 || !(x[4] > 0.0)) {
			std::fprintf(stderr, "Invalid value for %s (<blades>,<ring_px>,<strength>[,<rotation>[,<lambda_ref>]]: finite, blades an integer 0..64, ring_px > 0, strength 0..1, lambda_ref > 0)!\n", flag);
			throw -2;
		}
		iris->on = true; iris->blades = static_cast<int>(x[0]); iris->ring_px = x[1]; iris->strength = x[2]; iris->rotation = x[3]; iris->lambda_ref = x[4];
	};
	take_glare("--develop-glare", &g->develop_glare);
	take_glare("--delta-e-glare", &g->delta_e_glare);
	bool glare_radius_given = false;
	if (a.take("--develop-glare-radius", "", &v)) {
		size_t r = 999;
		try { r = v == "0" ? 0 : to_pos(v); } catch (int) { r = 999; }
		if (r > SSX_GLARE_MAX_RADIUS) { std::fprintf(stderr, "Invalid value for --develop-glare-radius (0..256)!\n"); throw -2; }
		g->develop_glare_radius = static_cast<unsigned>(r);
		glare_radius_given = true;
	}
	{ // the display's options
		auto numbers = [&](const std::string& text, double* x, size_t most) { // comma-separated finite numbers: how many, or 0 for a malformed list
			size_t n = 0, at = 0;
			try {
				for (;;) {
					if (n == most) return static_cast<size_t>(0);
					const size_t comma = text.find(',', at);
					const std::string part = text.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
					size_t used = 0;
					x[n++] = std::stod(part, &used);
					if (used != part.size() || !std::isfinite(x[n - 1])) return static_cast<size_t>(0);
					if (comma == std::string::npos) return n;
					at = comma + 1;
				}
			} catch (...) { return static_cast<size_t>(0); }
		};
		bool local_given = false, wb_given = false;
		if (a.take("--develop-display", "", &v)) {
			const size_t comma = v.find(',');
			const std::string kind = v.substr(0, comma);
			double x[2] = { 0.18, 0.99 };
			const bool ok = comma == std::string::npos || numbers(v.substr(comma + 1), x, 2) != 0;
			if (!ok || (kind != "clip" && kind != "reinhard" && kind != "filmic") || !(x[0] > 0.0) || x[1] < 0.0 || x[1] > 1.0) {
				std::fprintf(stderr, "Invalid value for --develop-display (clip|reinhard|filmic[,<key>[,<white_percentile>]]: key finite and > 0, white_percentile 0..1)!\n");
				throw -2;
			}
			g->display_on = true;
			g->display.curve = kind == "clip" ? SSH_TONE_CLIP : (kind == "reinhard" ? SSH_TONE_REINHARD : SSH_TONE_FILMIC);
			g->display.key = x[0]; g->display.white_percentile = x[1];
		}
		if (a.take("--develop-display-local", "", &v)) {
			double x[4] = { 0.0, 0.0, 1.0, 0.25 };
			const size_t n = numbers(v, x, 4);
			if (n < 2 || x[0] < 1.0 || x[0] > static_cast<double>(SSX_LOCAL_MAX_RADIUS) || x[0] != std::floor(x[0]) || !std::isfinite(static_cast<float>(x[1])) ||
			    !std::isfinite(static_cast<float>(x[2])) || !std::isfinite(static_cast<float>(x[3])) || !(static_cast<float>(x[3]) > 0.0f)) {
				std::fprintf(stderr, "Invalid value for --develop-display-local (<radius>,<compress>[,<boost>[,<eps>]]: finite, radius an integer 1..32, eps > 0)!\n");
				throw -2;
			}
			g->display.local = true; g->display.radius = static_cast<uint32_t>(x[0]);
			g->display.compress = static_cast<float>(x[1]); g->display.boost = static_cast<float>(x[2]); g->display.eps = static_cast<float>(x[3]);
			local_given = true;
		}
		if (a.take("--develop-display-wb", "", &v)) {
			if (v == "none") g->display.wb = ssx::Renderer::WhiteBalance::None;
			else if (v == "grey") g->display.wb = ssx::Renderer::WhiteBalance::Grey;
			else if (v == "white-patch") g->display.wb = ssx::Renderer::WhiteBalance::WhitePatch;
			else { std::fprintf(stderr, "Invalid value for --develop-display-wb (none|grey|white-patch)!\n"); throw -2; }
			wb_given = true;
		}
		if (a.take("--meter-output", "", &v)) g->meter_output = v;
		if ((local_given || wb_given) && !g->display_on) { std::fprintf(stderr, "`--develop-display-local` and `--develop-display-wb` need `--develop-display=clip|reinhard|filmic`!\n"); throw -2; }
	}
	{ // the sensor's options
		auto split = [](const std::string& s) {
			std::vector<std::string> parts;
			size_t at = 0;
			for (;;) {
				const size_t comma = s.find(',', at);
				parts.push_back(s.substr(at, comma == std::string::npos ? std::string::npos : comma - at));
				if (comma == std::string::npos) break;
				at = comma + 1;
			}
			return parts;
		};
		auto number = [](const std::string& part, double* x) {
			try { size_t used = 0; *x = std::stod(part, &used); return used == part.size() && std::isfinite(*x); } catch (...) { return false; }
		};
		Progressive::SensorFlags& s = g->sensor;
		bool any = false;
		if (a.take("--develop-sensor", "", &v)) {
			const std::vector<std::string> p = split(v);
			const bool pattern_ok = p[0] == "RGGB" || p[0] == "BGGR" || p[0] == "GRBG" || p[0] == "GBRG";
			if (!pattern_ok || p.size() > 2 || (p.size() == 2 && p[1] != "mhc" && p[1] != "bilinear")) { std::fprintf(stderr, "Invalid value for --develop-sensor (RGGB|BGGR|GRBG|GBRG[,mhc|bilinear])!\n"); throw -2; }
			s.on = true; s.pattern = p[0]; s.method = p.size() == 2 && p[1] == "bilinear" ? SSH_DEMOSAIC_BILINEAR : SSH_DEMOSAIC_MHC;
		}
		if (a.take("--develop-sensor-curves", "", &v)) {
			s.curves = split(v);
			if (s.curves.size() != 3 || s.curves[0].empty() || s.curves[1].empty() || s.curves[2].empty()) { std::fprintf(stderr, "Invalid value for --develop-sensor-curves (<R.csv>,<G.csv>,<B.csv>)!\n"); throw -2; }
		}
		if (a.take("--develop-sensor-exposure", "", &v)) {
			const std::vector<std::string> p = split(v);
			if (p.size() != 2 || !number(p[0], &s.full_well) || !number(p[1], &s.white_level) || !(s.full_well > 0.0) || !(s.white_level > 0.0)) { std::fprintf(stderr, "Invalid value for --develop-sensor-exposure (<full_well>,<white_level>: finite and > 0)!\n"); throw -2; }
			s.exposure_given = any = true;
		}
		if (a.take("--develop-sensor-noise", "", &v)) {
			const std::vector<std::string> p = split(v);
			double seed = 0.0;
			if (p.size() > 2 || !number(p[0], &s.read_e) || s.read_e < 0.0 || (p.size() == 2 && (!number(p[1], &seed) || seed < 0.0 || seed > 4294967295.0 || seed != std::floor(seed)))) { std::fprintf(stderr, "Invalid value for --develop-sensor-noise (<read_e>[,<seed>]: read_e >= 0, seed a 32-bit number)!\n"); throw -2; }
			s.noise = any = true; s.seed = static_cast<unsigned>(seed);
		}
		if (a.take("--develop-sensor-bits", "", &v)) {
			const std::vector<std::string> p = split(v);
			double bits = 0.0;
			if (p.size() > 2 || !number(p[0], &bits) || bits < 1.0 || bits > 24.0 || bits != std::floor(bits) || (p.size() == 2 && (!number(p[1], &s.black) || s.black < 0.0))) { std::fprintf(stderr, "Invalid value for --develop-sensor-bits (<1..24>[,<black>= 0>])!\n"); throw -2; }
			s.bits = static_cast<unsigned>(bits); s.bits_given = any = true;
		}
		if (a.take("--sensor-raw-output", "", &v)) { s.raw_output = v; any = true; }
		if (any && !s.on) { std::fprintf(stderr, "`--develop-sensor-exposure`, `--develop-sensor-noise`, `--develop-sensor-bits` and `--sensor-raw-output` need `--develop-sensor=<pattern>`!\n"); throw -2; }
	}
	if (a.take("--delta-e-output", "", &v)) g->delta_e_output = v;
	if (a.take("--delta-e-csv", "", &v)) g->delta_e_csv = v;
	if (a.take("--delta-e-filter", "", &v)) g->delta_e_filter = v;
	if (a.take("--delta-e-relight", "", &v)) g->delta_e_relight = v;
	bool delta_e_side = !g->delta_e_filter.empty() || !g->delta_e_relight.empty();
	if (a.take("--delta-e-observer", "", &v)) {
		if (v == "1931") g->delta_e_observer = 1931; else if (v == "2006") g->delta_e_observer = 2006;
		else { std::fprintf(stderr, "Invalid value for --delta-e-observer (1931|2006)!\n"); throw -2; }
		delta_e_side = true;
	}
	if (a.take("--delta-e-denoise", "", &v)) {
		if (v != "--delta-e-denoise") { std::fprintf(stderr, "`--delta-e-denoise` does not take a value!\n"); throw -2; }
		g->delta_e_denoise = delta_e_side = true;
	}
	if (a.take("--delta-e-threshold", "", &v)) {
		bool ok = false;
		try {
			const size_t comma = v.find(',');
			if (comma != std::string::npos) {
				const std::string x = v.substr(0, comma), y = v.substr(comma + 1);
				size_t u0 = 0, u1 = 0;
				g->delta_e_threshold[0] = std::stod(x, &u0); g->delta_e_threshold[1] = std::stod(y, &u1);
				ok = u0 == x.size() && u1 == y.size() && g->delta_e_threshold[0] >= 0.0 && g->delta_e_threshold[1] >= 0.0 && g->delta_e_threshold[0] < 1e300 && g->delta_e_threshold[1] < 1e300;
			}
		} catch (...) { ok = false; }
		if (!ok) { std::fprintf(stderr, "Invalid value for --delta-e-threshold (<ab>,<00>, both finite and >= 0)!\n"); throw -2; }
		delta_e_side = true;
	}
	if (a.take("--delta-e-white-y", "", &v)) {
		try { size_t used = 0; g->delta_e_white_y = std::stod(v, &used); if (used != v.size() || !(g->delta_e_white_y > 0.0) || g->delta_e_white_y > 1e300) throw -2; }
		catch (...) { std::fprintf(stderr, "Invalid value for --delta-e-white-y (finite and > 0)!\n"); throw -2; }
		delta_e_side = true;
	}
	if (g->delta_e_lens.on || g->delta_e_defocus.on) delta_e_side = true;
	if (glare_radius_given && !g->develop_glare.on && !g->delta_e_glare.on) { std::fprintf(stderr, "`--develop-glare-radius` needs `--develop-glare` or `--delta-e-glare`!\n"); throw -2; }
	if (g->delta_e_glare.on && !g->delta_e()) { std::fprintf(stderr, "`--delta-e-glare` needs `--delta-e-output=<file.npy>` or `--delta-e-csv=<file.csv>`!\n"); throw -2; }
	if (defocus_radius_given && !g->develop_defocus.on && !g->delta_e_defocus.on) { std::fprintf(stderr, "`--develop-defocus-radius` needs `--develop-defocus` or `--delta-e-defocus`!\n"); throw -2; }
	if (lens_radius_given && !g->develop_lens.on && !g->delta_e_lens.on) { std::fprintf(stderr, "`--develop-lens-radius` needs `--develop-lens` or `--delta-e-lens`!\n"); throw -2; }
	if (delta_e_side && !g->delta_e()) {
		std::fprintf(stderr, "`--delta-e-observer`, `--delta-e-filter`, `--delta-e-relight`, `--delta-e-denoise`, `--delta-e-threshold`, `--delta-e-white-y`, `--delta-e-lens` and `--delta-e-defocus` need `--delta-e-output=<file.npy>` or `--delta-e-csv=<file.csv>`!\n");
		throw -2;
	}
	if (a.take("--spectral-bins", "", &v)) {
		g->spectral_bins_given = true;
		try { g->spectral_bins = to_pos(v); } catch (int) { g->spectral_bins = 0; }
		if (g->spectral_bins == 0 || g->spectral_bins > 64 || g->spectral_bins % 4) { std::fprintf(stderr, "Invalid value for --spectral-bins (a multiple of 4 up to 64)!\n"); throw -2; }
	}
	if (!g->resume.empty() && (!g->spectral_output.empty() || !g->develop_output.empty())) {
		// the bins of the samples already rendered must come from the checkpoint: it has to hold them, as many as are asked for (default: as many as it holds)
		const char* const flag = !g->spectral_output.empty() ? "--spectral-output" : "--develop-output";
		uint32_t held = 0;
		try { held = ssx::checkpoint_load(g->resume).spectral.bins; }
		catch (const ssx::HostError& e) {
			std::fprintf(stderr, "`%s` cannot be combined with `--resume` of a checkpoint that cannot be read: %s\n", flag, e.message.c_str());
			throw -2;
		}
		if (!held) {
			std::fprintf(stderr, "`%s` cannot be combined with `--resume` of a checkpoint without wavelength bins: \"%s\" holds the pixel sums only (write it with `--checkpoint` and a spectral option)!\n", flag, g->resume.c_str());
			throw -2;
		}
		if (g->spectral_bins_given && g->spectral_bins != held) {
			std::fprintf(stderr, "`%s` cannot be combined with `--resume` of a checkpoint with another bin count: \"%s\" holds %u wavelength bins, `--spectral-bins=%zu` was asked for!\n", flag, g->resume.c_str(), held, g->spectral_bins);
			throw -2;
		}
		g->spectral_bins = held; g->spectral_bins_given = true;
	}
	if (!g->spectral_output.empty() && (o->tile_major || o->rgb_mode || o->libm != SSX_LIBM_BUILD)) {
		std::fprintf(stderr, "`--spectral-output` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`!\n");
		throw -2;
	}
	if (g->develop_output.empty() && !g->delta_e() && (!g->develop_filter.empty() || !g->develop_relight.empty() || g->develop_observer || g->develop_lens.on || g->develop_defocus.on || !g->sensor.curves.empty())) {
		std::fprintf(stderr, "`--develop-observer`, `--develop-filter`, `--develop-relight`, `--develop-lens`, `--develop-defocus` and `--develop-sensor-curves` need `--develop-output=<image>`!\n");
		throw -2;
	}
	if ((g->display_on || !g->meter_output.empty()) && g->develop_output.empty()) {
		std::fprintf(stderr, "`--develop-display` and `--meter-output` need `--develop-output=<image>`: they finish and meter the image written there!\n");
		throw -2;
	}
	if (g->develop_glare.on && g->develop_output.empty() && !g->delta_e()) { std::fprintf(stderr, "`--develop-glare` needs `--develop-output=<image>`!\n"); throw -2; }
	if (g->sensor.on && g->develop_output.empty()) { std::fprintf(stderr, "`--develop-sensor` needs `--develop-output=<image>`: it writes the demosaiced image there!\n"); throw -2; }
	if (g->sensor.on && g->delta_e()) { std::fprintf(stderr, "`--develop-sensor` cannot be combined with `--delta-e-output` or `--delta-e-csv`: compare two developments with Renderer.delta_e_images instead!\n"); throw -2; }
	if (g->delta_e() && !g->spectral_bins_given) {
		std::fprintf(stderr, "`--delta-e-output` and `--delta-e-csv` need `--spectral-bins=<n>`: they compare two developments of the render's wavelength bins!\n");
		throw -2;
	}
	if (g->delta_e() && (o->tile_major || o->rgb_mode || o->libm != SSX_LIBM_BUILD)) {
		std::fprintf(stderr, "`--delta-e-output` and `--delta-e-csv` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`: such a render has no wavelength bins!\n");
		throw -2;
	}
	if (g->delta_e() && !g->resume.empty()) { std::fprintf(stderr, "`--delta-e-output` and `--delta-e-csv` cannot be combined with `--resume`!\n"); throw -2; }
	if (!g->develop_output.empty() && !g->spectral_bins_given) {
		std::fprintf(stderr, "`--develop-output` needs `--spectral-bins=<n>`: it develops the wavelength bins of the render!\n");
		throw -2;
	}
	if (!g->develop_output.empty() && (o->tile_major || o->rgb_mode || o->libm != SSX_LIBM_BUILD)) {
		std::fprintf(stderr, "`--develop-output` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`: such a render has no wavelength bins!\n");
		throw -2;
	}
	if (a.take("--denoise", "", &v)) {
		if (v != "--denoise") { std::fprintf(stderr, "`--denoise` does not take a value!\n"); throw -2; }
		g->denoise = true;
	}
	if (a.take("--denoise-levels", "", &v)) {
		unsigned n = 0;
		try { n = to_pos(v); } catch (int) { n = 0; }
		if (n < 1 || n > 6) { std::fprintf(stderr, "Invalid value for --denoise-levels (1..6)!\n"); throw -2; }
		g->denoise_params.levels = n;
	}
	if (a.take("--denoise-sigma", "", &v)) {
		bool ok = false;
		try {
			const size_t comma = v.find(',');
			if (comma != std::string::npos) {
				size_t u0 = 0, u1 = 0;
				const std::string l = v.substr(0, comma), s2 = v.substr(comma + 1);
				g->denoise_params.sigma_l = std::stof(l, &u0); g->denoise_params.sigma_a = std::stof(s2, &u1);
				ok = u0 == l.size() && u1 == s2.size() && g->denoise_params.sigma_l > 0.0f && g->denoise_params.sigma_a > 0.0f &&
				     g->denoise_params.sigma_l < 1e30f && g->denoise_params.sigma_a < 1e30f;
			}
		} catch (...) { ok = false; }
		if (!ok) { std::fprintf(stderr, "Invalid value for --denoise-sigma (<l>,<a>, both positive)!\n"); throw -2; }
	}
	if (a.take("--spectral-denoise", "", &v)) {
		if (v != "--spectral-denoise") { std::fprintf(stderr, "`--spectral-denoise` does not take a value!\n"); throw -2; }
		if (g->spectral_output.empty() && g->develop_output.empty() && !g->delta_e()) { std::fprintf(stderr, "`--spectral-denoise` needs `--spectral-output=<file.npy>`: it filters the bins written there!\n"); throw -2; }
		g->spectral_denoise = true;
	}
	if (a.take("--demodulate", "", &v)) {
		if (!g->spectral_denoise) { std::fprintf(stderr, "`--demodulate` needs `--spectral-denoise`: it is a mode of that filter!\n"); throw -2; }
		if (v != "--demodulate") {
			if (v != "1" && v != "2" && v != "4") { std::fprintf(stderr, "Invalid value for --demodulate (1, 2 or 4 rays per pixel axis)!\n"); throw -2; }
			g->demod_params.supersample = static_cast<uint32_t>(v[0] - '0');
		}
		g->demodulate = true;
	}
	if (a.take("--albedo-output", "", &v)) {
		if (!g->spectral_bins_given || o->rgb_mode) { std::fprintf(stderr, "`--albedo-output` needs `--spectral-bins=<n>` and a spectral render: it writes the albedo of those bins!\n"); throw -2; }
		g->albedo_output = v;
	}
	const bool filters = g->denoise || g->spectral_denoise || g->delta_e_denoise; // both render for the filter: the noise estimate on, two batches at least
	const char* const flag = g->denoise ? "--denoise" : g->spectral_denoise ? "--spectral-denoise" : "--delta-e-denoise";
	if (filters && o->spp < 2) { std::fprintf(stderr, "`%s` needs at least two samples per pixel: its variance estimate compares batches of samples!\n", flag); throw -2; }
	if (filters && o->tile_major) { std::fprintf(stderr, "`%s` cannot be combined with `--tile-major`: only a render that walks through the samples takes batches!\n", flag); throw -2; }
	if (filters) o->spp_per_launch = g->noise_step_given ? g->noise_step : (o->spp + 7) / 8; // at least two launches = two batches
	if (filters && o->spp_per_launch >= o->spp) { std::fprintf(stderr, "`%s` needs `--noise-step` below the number of samples (two batches at least)!\n", flag); throw -2; }
	if (a.take("--guides-output", "", &v)) g->guides_output = v;
	if (a.take("--spectral-variance-output", "", &v)) g->variance_output = v;
	while (a.take("--probe", "", &v)) {
		const std::array<size_t, 4> q = to_rect("--probe", v, o->res[0], o->res[1]);
		if (g->probes.size() == 32) { std::fprintf(stderr, "`--probe` can be given 32 times at most!\n"); throw -2; }
		g->probes.push_back(q);
	}
	if (a.take("--probe-output", "", &v)) g->probe_output = v;
	if (a.take("--compare-to", "", &v)) g->compare_to = v;
	if (a.take("--compare-output", "", &v)) g->compare_output = v;
	if (a.take("--compare-map-output", "", &v)) g->compare_map_output = v;
	if (a.take("--compare-threshold", "", &v)) {
		try { size_t used = 0; g->compare_threshold = std::stod(v, &used); if (used != v.size() || !(g->compare_threshold >= 0.0) || g->compare_threshold > 1e150) throw -2; }
		catch (...) { std::fprintf(stderr, "Invalid value for --compare-threshold (a finite number >= 0)!\n"); throw -2; }
	}
	if (g->compare_to.empty() && (!g->compare_output.empty() || !g->compare_map_output.empty())) {
		std::fprintf(stderr, "`--compare-output` and `--compare-map-output` need `--compare-to=<file.ckpt>`: they write that comparison!\n");
		throw -2;
	}
	if ((g->probes.empty() != g->probe_output.empty()) && ((g->compare_to.empty() && !g->delta_e()) || g->probes.empty())) { // (--compare-to and --delta-e-* take their regions from --probe alone)
		std::fprintf(stderr, "`--probe=<x0>,<y0>,<x1>,<y1>` and `--probe-output=<file.csv>` need each other!\n"); throw -2; }
	if (g->moments()) {
		const char* const flag = !g->variance_output.empty() ? "--spectral-variance-output" : !g->probe_output.empty() ? "--probe" : "--compare-to";
		if (!g->resume.empty()) resume_needs_moments(flag, g);
		if (!g->spectral_bins_given) { std::fprintf(stderr, "`%s` needs `--spectral-bins=<n>`: it speaks of the wavelength bins of the render!\n", flag); throw -2; }
		if (o->tile_major || o->rgb_mode || o->libm != SSX_LIBM_BUILD) {
			std::fprintf(stderr, "`%s` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`: such a render has no wavelength bins!\n", flag);
			throw -2;
		}
	}
	if (a.take("--spectral-noise-target", "", &v)) {
		try { size_t used = 0; g->spectral_noise_target = std::stod(v, &used); if (used != v.size() || !(g->spectral_noise_target >= 0.0)) throw -2; }
		catch (...) { std::fprintf(stderr, "Invalid value for --spectral-noise-target (a number >= 0)!\n"); throw -2; }
	}
	if (!g->compare_to.empty()) { // the other render is read now: what cannot be compared is refused before anything renders
		const char* const head = "`--compare-to` cannot compare with \"%s\": ";
		ssx::Checkpoint ck;
		try { ck = ssx::checkpoint_load(g->compare_to); }
		catch (const ssx::HostError& e) {
			std::fprintf(stderr, head, g->compare_to.c_str());
			std::fprintf(stderr, "the checkpoint cannot be read: %s\n", e.message.c_str());
			throw -2;
		}
		if (!ck.spectral.bins || ck.moments.empty()) {
			std::fprintf(stderr, head, g->compare_to.c_str());
			if (!ck.spectral.bins) std::fprintf(stderr, "it holds the pixel sums only, no wavelength bins and no second moments Q (write it with `--checkpoint` and `--spectral-variance-output`, `--probe` or `--compare-to`)!\n");
			else std::fprintf(stderr, "it holds %u wavelength bins without their second moments Q (write it with `--checkpoint` and `--spectral-variance-output`, `--probe` or `--compare-to`)!\n", ck.spectral.bins);
			throw -2;
		}
		if (ck.spectral.width != o->res[0] || ck.spectral.height != o->res[1]) {
			std::fprintf(stderr, head, g->compare_to.c_str());
			std::fprintf(stderr, "the size differs: it holds %u x %u pixels, this render has %zu x %zu!\n", ck.spectral.width, ck.spectral.height, static_cast<size_t>(o->res[0]), static_cast<size_t>(o->res[1]));
			throw -2;
		}
		if (ck.spectral.bins != g->spectral_bins) {
			std::fprintf(stderr, head, g->compare_to.c_str());
			std::fprintf(stderr, "the bin count differs: it holds %u wavelength bins, `--spectral-bins=%zu` is in force!\n", ck.spectral.bins, g->spectral_bins);
			throw -2;
		}
		if (ck.info.seed == o->seed) std::fprintf(stderr, "Warning: `--compare-to`: same seed: the samples are not independent; z is not calibrated\n");
		g->compare_other = std::make_shared<ssx::Checkpoint>(std::move(ck));
	}
	const bool spectral_stop = g->spectral_noise_target >= 0.0;
	if (a.take("--spectral-noise-coverage", "", &v)) {
		try { size_t used = 0; g->spectral_noise_coverage = std::stod(v, &used); if (used != v.size() || !(g->spectral_noise_coverage >= 0.0 && g->spectral_noise_coverage <= 1.0)) throw -2; }
		catch (...) { std::fprintf(stderr, "Invalid value for --spectral-noise-coverage (0..1)!\n"); throw -2; }
		if (!spectral_stop) { std::fprintf(stderr, "`--spectral-noise-coverage` needs `--spectral-noise-target=<x>`: it is part of that stopping rule!\n"); throw -2; }
	}
	while (a.take("--spectral-noise-region", "", &v)) {
		if (!spectral_stop) { std::fprintf(stderr, "`--spectral-noise-region` needs `--spectral-noise-target=<x>`: it is part of that stopping rule!\n"); throw -2; }
		g->spectral_noise_regions.push_back(to_rect("--spectral-noise-region", v, o->res[0], o->res[1]));
	}
	if (a.take("--spectral-noise-output", "", &v)) {
		if (!spectral_stop) { std::fprintf(stderr, "`--spectral-noise-output` needs `--spectral-noise-target=<x>`: it writes the figure that rule stopped on!\n"); throw -2; }
		g->spectral_noise_output = v;
	}
	if (spectral_stop) {
		const char* const flag = "--spectral-noise-target";
		if (g->noise_target >= 0.0) { std::fprintf(stderr, "`%s` cannot be combined with `--noise-target`: one stopping rule per run!\n", flag); throw -2; }
		if (!g->resume.empty()) resume_needs_moments(flag, g);
		if (!g->spectral_bins_given) { std::fprintf(stderr, "`%s` needs `--spectral-bins=<n>`: it speaks of the wavelength bins of the render!\n", flag); throw -2; }
		if (g->max_samples == 0) { std::fprintf(stderr, "`%s` needs `--max-samples=<n>`!\n", flag); throw -2; }
		if (o->tile_major || o->rgb_mode || o->libm != SSX_LIBM_BUILD) {
			std::fprintf(stderr, "`%s` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`: such a render has no wavelength bins!\n", flag);
			throw -2;
		}
	}
	if (a.take("--texture", "", &v)) o->texture_path = v;
	if (a.take("--data-dir", "", &v)) o->data_dir = v;
	if (a.args.size() > 1) {
		std::fprintf(stderr, "Warning: ignoring extraneous argument(s):\n");
		for (size_t i = 1; i < a.args.size(); ++i) std::fprintf(stderr, "  \"%s\"\n", a.args[i].c_str());
	}
}

} // namespace

namespace {
// The reference aborts a render by closing its window (src/main.cpp:318-327: render_stop, then the
// last worker saves what exists).  Without a window the same path hangs off Ctrl-C.
volatile std::sig_atomic_t g_abort = 0;
void on_sigint(int) { g_abort = 1; }
} // namespace

// --meter-output: the line "quantity,key,lower_edge,count", then one line per non-zero counter -- quantity 0..2 the channels, 3 the luminance; key 0..4095 with
// its lower edge frombits(key << 19) (%.9g), or one of zero, negative, inf, nan with an empty edge
static void save_meter_csv(const std::string& path, const ssx::Renderer::Meter& m) {
	FILE* const f = std::fopen(path.c_str(), "w");
	if (!f) throw ssx::HostError{ SSX_ERR_DATA, "cannot write " + path };
	std::fprintf(f, "quantity,key,lower_edge,count\n");
	static const char* const classes[4] = { "zero", "negative", "inf", "nan" };
	for (uint32_t k = 0; k < 4u; ++k) {
		for (uint32_t key = 0; key < SSX_METER_KEYS; ++key) {
			const uint32_t n = m.hist[k * SSX_METER_KEYS + key];
			if (!n) continue;
			const uint32_t u = key << 19; float edge; std::memcpy(&edge, &u, sizeof edge);
			std::fprintf(f, "%u,%u,%.9g,%u\n", k, key, static_cast<double>(edge), n);
		}
		for (uint32_t c = 0; c < 4u; ++c) if (m.special[k * 4u + c]) std::fprintf(f, "%u,%s,,%u\n", k, classes[c], m.special[k * 4u + c]);
	}
	std::fclose(f);
}

int main(int argc, char* argv[]) {
	ssx::Renderer::Options options;
	Progressive prog;
	try {
		parse_arguments(argc, argv, &options, &prog);
	} catch (int) {
		print_usage();
		return -1;
	}
	try {
		const std::string denoised_path = options.output_path;
		if (prog.denoise) options.output_path.clear(); // (render_wait writes the plain image there; the filtered one is written below)
		ssx::Renderer renderer(options);
		std::signal(SIGINT, on_sigint);
		if (prog.denoise || prog.spectral_denoise || prog.delta_e_denoise) renderer.set_noise_estimate(true);
		const bool spectral_stop = prog.spectral_noise_target >= 0.0;
		if (!prog.spectral_output.empty() || !prog.develop_output.empty() || prog.delta_e() || prog.moments() || spectral_stop) renderer.set_spectral_bins(prog.spectral_bins);
		if (prog.moments() || (spectral_stop && !prog.resume.empty())) renderer.set_spectral_moments(true); // (before load_checkpoint: it takes Q up only with the moments on)
		// what --develop-output applies, built (and refused) before the render: the observer's tables over the bins, times the filter, times the relighting gain
		std::vector<float> develop_weights;
		std::unique_ptr<ssx::ColorData> develop_color;
		// one development's weights: the observer's tables over the bins, times the filter, times the relighting gain (`relit` false: without the gain)
		// (`responses`: a camera's three curves in the observer's place)
		auto weights_of = [&](const ssx::ColorData& color, const std::string& filter_path, const std::string& relight_path, bool relit, const std::vector<ssx::Spectrum>* responses = nullptr) {
			const ssx_scene_desc& d = renderer.scene->desc();
			const uint32_t B = static_cast<uint32_t>(prog.spectral_bins);
			ssx::Spectrum filter;
			if (!filter_path.empty()) filter = ssx::load_spectrum_csv(filter_path);
			std::vector<double> gain;
			if (relit && !relight_path.empty()) {
				const ssx_spectrum& e = d.spectra[ssx::emitter_spectrum(d)];
				const ssx::Spectrum from(std::vector<float>(d.samples + e.offset, d.samples + e.offset + e.n), e.low, e.high);
				gain = ssx::relight_gain(from, ssx::load_spectrum_csv(relight_path), B, d.lambda_min, d.lambda_step);
			}
			const std::vector<double> w = ssx::develop_weights(responses ? *responses : std::vector<ssx::Spectrum>{ color.std_obs_xbar, color.std_obs_ybar, color.std_obs_zbar },
			                                                   filter_path.empty() ? nullptr : &filter, gain.empty() ? nullptr : gain.data(), nullptr, B, d.lambda_min, d.lambda_step);
			return std::vector<float>(w.begin(), w.end()); // (rounded to binary32 here, once)
		};
		if (!prog.develop_output.empty() || prog.delta_e()) {
			develop_color = std::make_unique<ssx::ColorData>(options.data_dir, prog.develop_observer ? prog.develop_observer : options.observer);
			develop_color->meng_output_transform = renderer.color->meng_output_transform;
			develop_weights = weights_of(*develop_color, prog.develop_filter, prog.develop_relight, true);
		}
		// the sensor, built (and refused) before the render; --develop-sensor-curves on its own: an ordinary develop with the camera's curves in the observer's place
		ssx::Renderer::Sensor sensor;
		if (prog.sensor.on || !prog.sensor.curves.empty()) {
			std::vector<ssx::Spectrum> curves;
			for (const std::string& path : prog.sensor.curves) curves.push_back(ssx::load_spectrum_csv(path));
			for (uint32_t c = 0; curves.size() < 3; ++c) { // the stand-in curves of include/ssx_host.h: no camera's
				std::vector<float> samples(SSH_SENSOR_STANDIN_SAMPLES);
				float low = 0.0f, high = 0.0f;
				if (ssh_sensor_standin_curve(c, samples.data(), &low, &high) != SSX_OK) throw ssx::HostError{ SSX_ERR_ARG, std::string("--develop-sensor: ") + ssh_last_error() };
				curves.emplace_back(std::move(samples), low, high);
			}
			const std::vector<float> cam = weights_of(*develop_color, prog.develop_filter, prog.develop_relight, true, &curves);
			if (!prog.sensor.on) develop_weights = cam;
			else {
				const Progressive::SensorFlags& f = prog.sensor;
				const uint32_t B = static_cast<uint32_t>(prog.spectral_bins);
				sensor.weights = cam; sensor.taps.resize(300); sensor.ccm.resize(9);
				float scales[7];
				if (ssh_sensor_bayer(f.pattern.c_str(), f.method, sensor.cfa, sensor.taps.data()) != SSX_OK ||
				    ssh_sensor_exposure(f.full_well, f.white_level, f.bits, f.black, f.read_e, scales) != SSX_OK ||
				    ssh_sensor_ccm(cam.data(), develop_weights.data(), B, sensor.ccm.data()) != SSX_OK) // to the space --develop-output writes: the observer's X, Y, Z
					throw ssx::HostError{ SSX_ERR_ARG, std::string("--develop-sensor: ") + ssh_last_error() };
				sensor.exposure = scales[0]; sensor.inv_exposure = scales[1]; sensor.read_var = scales[2]; sensor.dn_per_e = scales[3]; sensor.e_per_dn = scales[4];
				sensor.black = scales[5]; sensor.white = scales[6];
				sensor.noise = f.noise ? 1u : 0u; sensor.seed = f.seed;
			}
		}
		// the lenses, built (and refused) before the render
		ssx::Renderer::Optics lens_a, lens_b;
		auto make_lens = [&](const Progressive::Lens& l, ssx::Renderer::Optics* o) {
			if (!l.on) return;
			const ssx_scene_desc& d = renderer.scene->desc();
			const uint32_t B = static_cast<uint32_t>(prog.spectral_bins), R = prog.develop_lens_radius;
			o->max_radius = R; o->scale.resize(B); o->radius.resize(B); o->taps.resize(static_cast<size_t>(B) * (2u * R + 1u));
			if (ssh_optics_lens(B, d.lambda_min, d.lambda_step, l.lambda_ref, l.lateral, l.sigma, l.axial, R, o->scale.data(), o->radius.data(), o->taps.data()) != SSX_OK)
				throw ssx::HostError{ SSX_ERR_ARG, std::string("--develop-lens / --delta-e-lens: ") + ssh_last_error() };
		};
		make_lens(prog.develop_lens, &lens_a);
		make_lens(prog.delta_e_lens, &lens_b);
		const ssx::Renderer::Optics* const optics_a = prog.develop_lens.on ? &lens_a : nullptr;
		const ssx::Renderer::Optics* const optics_b = prog.delta_e_lens.on ? &lens_b : nullptr;
		// ... and the apertures
		ssx::Renderer::Defocus aperture_a, aperture_b;
		auto make_aperture = [&](const Progressive::Aperture& ap, ssx::Renderer::Defocus* f) {
			if (!ap.on) return;
			const ssx_scene_desc& d = renderer.scene->desc();
			const uint32_t B = static_cast<uint32_t>(prog.spectral_bins);
			f->max_radius = prog.develop_defocus_radius; f->focus.resize(B);
			if (ssh_defocus_thin_lens(renderer.scene->camera.vfov_deg, static_cast<uint32_t>(options.res[1]), B, d.lambda_min, d.lambda_step, ap.aperture, ap.focus_distance, ap.axial,
			                          ap.lambda_ref, &f->gain, f->focus.data()) != SSX_OK)
				throw ssx::HostError{ SSX_ERR_ARG, std::string("--develop-defocus / --delta-e-defocus: ") + ssh_last_error() };
		};
		make_aperture(prog.develop_defocus, &aperture_a);
		make_aperture(prog.delta_e_defocus, &aperture_b);
		const ssx::Renderer::Defocus* const defocus_a = prog.develop_defocus.on ? &aperture_a : nullptr;
		const ssx::Renderer::Defocus* const defocus_b = prog.delta_e_defocus.on ? &aperture_b : nullptr;
		// ... and the glares, with the plan and the twiddles of this image
		ssx::Renderer::Glare glare_store_a, glare_store_b;
		auto make_glare = [&](const Progressive::Iris& iris, ssx::Renderer::Glare* gl) {
			if (!iris.on) return;
			const ssx_scene_desc& d = renderer.scene->desc();
			const uint32_t B = static_cast<uint32_t>(prog.spectral_bins), R = prog.develop_glare_radius, K = 2u * R + 1u;
			gl->radius = R; gl->on.resize(B); gl->psf.resize(static_cast<size_t>(B) * K * K);
			if (ssh_glare_plan(static_cast<uint32_t>(options.res[0]), static_cast<uint32_t>(options.res[1]), R, &gl->px, &gl->py) != SSX_OK)
				throw ssx::HostError{ SSX_ERR_ARG, std::string("--develop-glare / --delta-e-glare: ") + ssh_last_error() };
			gl->twiddle_x.resize(gl->px); gl->twiddle_y.resize(gl->py);
			if (ssh_glare_twiddles(gl->px, gl->twiddle_x.data()) != SSX_OK || ssh_glare_twiddles(gl->py, gl->twiddle_y.data()) != SSX_OK ||
			    ssh_glare_aperture(B, d.lambda_min, d.lambda_step, iris.lambda_ref, iris.blades, iris.rotation, iris.ring_px, iris.strength, R, gl->psf.data(), gl->on.data()) != SSX_OK)
				throw ssx::HostError{ SSX_ERR_ARG, std::string("--develop-glare / --delta-e-glare: ") + ssh_last_error() };
		};
		make_glare(prog.develop_glare, &glare_store_a);
		make_glare(prog.delta_e_glare, &glare_store_b);
		const ssx::Renderer::Glare* const glare_a = prog.develop_glare.on ? &glare_store_a : nullptr;
		const ssx::Renderer::Glare* const glare_b = prog.delta_e_glare.on ? &glare_store_b : nullptr;
		// side B of --delta-e-*, and both sides' whites up to the common scale (host policy: the chromaticity is the development, by the side's weights without a
		// relighting gain, of the side's illuminant -- the relight's new one, else the scene's emitter spectrum where it has one, else D65)
		std::vector<float> delta_e_weights;
		double delta_e_white[2][3] = {};
		if (prog.delta_e()) {
			const ssx_scene_desc& d = renderer.scene->desc();
			const uint32_t B = static_cast<uint32_t>(prog.spectral_bins);
			const ssx::ColorData color_b(options.data_dir, prog.delta_e_observer ? prog.delta_e_observer : options.observer);
			delta_e_weights = weights_of(color_b, prog.delta_e_filter, prog.delta_e_relight, true);
			ssx::Spectrum scene_light;
			try {
				const ssx_spectrum& e = d.spectra[ssx::emitter_spectrum(d)];
				scene_light = ssx::Spectrum(std::vector<float>(d.samples + e.offset, d.samples + e.offset + e.n), e.low, e.high);
			} catch (const ssx::HostError&) { scene_light = ssx::load_spectrum_csv(options.data_dir + "/d65-300+5+780.csv"); }
			const struct { const ssx::ColorData* color; const std::string* filter; const std::string* relight; } sides[2] = {
				{ develop_color.get(), &prog.develop_filter, &prog.develop_relight }, { &color_b, &prog.delta_e_filter, &prog.delta_e_relight } };
			for (int x = 0; x < 2; ++x) {
				const std::vector<float> plain = weights_of(*sides[x].color, *sides[x].filter, *sides[x].relight, false);
				const ssx::Spectrum light = sides[x].relight->empty() ? scene_light : ssx::load_spectrum_csv(*sides[x].relight);
				ssx::develop_white(plain.data(), B, d.lambda_min, d.lambda_step, &light, delta_e_white[x]);
				for (int c = 0; c < 3; ++c)
					if (!(delta_e_white[x][c] > 0.0)) throw ssx::HostError{ SSX_ERR_ARG, "--delta-e: a side's white has a component that is not positive (its filter or illuminant leaves a channel dark)" };
			}
		}
		if (prog.compare_other) { // the last refusal of --compare-to needs the scene: still before anything renders
			const ssx_scene_desc& d = renderer.scene->desc();
			const float bin_width = d.lambda_step / static_cast<float>(prog.spectral_bins / 4);
			const ssx_spectral_info_t& other = prog.compare_other->spectral;
			if (std::memcmp(&other.lambda_min, &d.lambda_min, sizeof(float)) != 0 || std::memcmp(&other.bin_width, &bin_width, sizeof(float)) != 0) {
				std::fprintf(stderr, "`--compare-to` cannot compare with \"%s\": lambda_min or bin_width differs: its bins start at %.9g nm and are %.9g nm wide, this render's start at %.9g nm and are %.9g nm wide!\n",
				             prog.compare_to.c_str(), static_cast<double>(other.lambda_min), static_cast<double>(other.bin_width), static_cast<double>(d.lambda_min), static_cast<double>(bin_width));
				return -1;
			}
		}
		bool stop_sent = false;
		const bool needs_moments = prog.moments() || spectral_stop;
		if (!prog.resume.empty()) {
			try {
				const bool bins = renderer.load_checkpoint(prog.resume);
				if (!bins && (!prog.spectral_output.empty() || !prog.develop_output.empty())) // (checked when the arguments were read; the file has changed since)
					throw ssx::HostError{ SSX_ERR_DATA, "it holds no wavelength bins of the count asked for" };
				if (needs_moments && !renderer.moments_resumed()) throw ssx::HostError{ SSX_ERR_DATA, "it holds no second moments for the bin count asked for" };
			}
			catch (const ssx::HostError& e) { // not this render's checkpoint (or no checkpoint at all): bad data, as the reference exits on it
				std::fprintf(stderr, "Cannot resume from \"%s\": %s\n", prog.resume.c_str(), e.message.c_str());
				return -1;
			}
		}
		if (prog.noise_target >= 0.0) {
			const auto r = renderer.render_until(prog.noise_target, prog.noise_step, prog.max_samples, [&]() {
				renderer.print_progress();
				if (!g_abort || stop_sent) return false;
				stop_sent = true; std::fprintf(stderr, "\nAborting: saving the partial render ...\n");
				return true;
			});
			std::fprintf(stderr, "Noise %.6g after %zu samples per pixel (target %.6g).\n", r.second, r.first, prog.noise_target);
		} else if (spectral_stop) {
			const std::vector<uint8_t> mask = prog.spectral_noise_regions.empty() ? std::vector<uint8_t>() : renderer.mask_from_rects(prog.spectral_noise_regions);
			if (!prog.resume.empty()) std::fprintf(stderr, "Resuming \"%s\": %zu samples per pixel done, at most %zu wanted.\n", prog.resume.c_str(), renderer.done_spp(), prog.max_samples);
			const auto r = renderer.render_until_spectral(prog.spectral_noise_target, prog.noise_step, prog.max_samples, mask, prog.spectral_noise_coverage, [&]() {
				renderer.print_progress();
				if (!g_abort || stop_sent) return false;
				stop_sent = true; std::fprintf(stderr, "\nAborting: saving the partial render ...\n");
				return true;
			}, !prog.resume.empty());
			std::fprintf(stderr, "Spectral noise %.6g (coverage %.6g) after %zu samples per pixel (target %.6g).\n", r.noise, r.coverage, r.spp, prog.spectral_noise_target);
			if (!prog.spectral_noise_output.empty()) renderer.save_spectral_noise_csv(prog.spectral_noise_output, renderer.spectral_noise(mask));
		} else {
			if (!prog.resume.empty()) {
				const size_t done = renderer.done_spp();
				std::fprintf(stderr, "Resuming \"%s\": %zu samples per pixel done, %zu wanted.\n", prog.resume.c_str(), done, options.spp);
				if (options.spp > done) renderer.render_continue(options.spp - done);
			} else renderer.render_start();
			while (renderer.is_rendering()) { // the reference prints from its workers every 10 ms (src/renderer.cpp:352-358)
				if (g_abort && !stop_sent) { renderer.render_stop(); stop_sent = true; std::fprintf(stderr, "\nAborting: saving the partial render ...\n"); }
				renderer.print_progress();
				std::this_thread::sleep_for(std::chrono::milliseconds(10));
			}
		}
		// An aborted multi-GPU render: the devices stopped at different counts.  With a checkpoint asked for they are brought level first (the
		// laggards finish the launches the others had done), so that the image written now is the one the checkpoint resumes from.
		if (!prog.checkpoint.empty()) renderer.level_devices();
		renderer.render_wait();
		std::vector<float> filtered_bins;
		if (prog.spectral_denoise && (prog.denoise || !prog.spectral_output.empty())) { // (one run of the filter serves both outputs)
			const ssx::Framebuffer fb = renderer.denoise_spectral(prog.denoise_params, &filtered_bins, nullptr, prog.demodulate ? &prog.demod_params : nullptr);
			if (prog.denoise) fb.save(denoised_path);
		} else if (prog.denoise) renderer.denoise(prog.denoise_params).save(denoised_path);
		if (!prog.guides_output.empty()) renderer.save_guides(prog.guides_output);
		if (!prog.albedo_output.empty()) renderer.save_albedo_bins(prog.albedo_output, prog.spectral_bins, prog.demod_params.supersample);
		if (prog.spectral_denoise && !prog.spectral_output.empty()) renderer.save_spectral_image(prog.spectral_output, filtered_bins);
		else if (!prog.spectral_output.empty()) renderer.save_spectral_image(prog.spectral_output);
		if (!prog.variance_output.empty()) renderer.save_spectral_variance(prog.variance_output);
		if (!prog.probe_output.empty()) renderer.save_probe_csv(prog.probe_output, renderer.probe(renderer.labels_from_rects(prog.probes), prog.probes.size()));
		if (prog.compare_other) {
			const size_t regions = prog.probes.empty() ? 1 : prog.probes.size();
			const std::vector<uint8_t> labels = prog.probes.empty() ? std::vector<uint8_t>(options.res[0] * options.res[1], 0u) : renderer.labels_from_rects(prog.probes);
			const ssx::Renderer::Compare c = renderer.compare_spectral(*prog.compare_other, labels, regions, prog.compare_threshold * prog.compare_threshold, !prog.compare_map_output.empty());
			if (!prog.compare_output.empty()) renderer.save_compare_csv(prog.compare_output, c);
			if (!prog.compare_map_output.empty()) renderer.save_compare_map(prog.compare_map_output, c);
			for (size_t r = 0; r < regions; ++r) { // one line per region, the bins added up: the CSV has the figures
				uint64_t cc = 0, ex = 0;
				for (size_t b = 0; b < c.bins; ++b) { cc += c.CC[r * c.bins + b]; ex += c.EX[r * c.bins + b]; }
				std::fprintf(stderr, "Compared with \"%s\", region %zu: %llu comparable cells, %llu beyond z = %.6g.\n", prog.compare_to.c_str(), r, static_cast<unsigned long long>(cc),
				             static_cast<unsigned long long>(ex), prog.compare_threshold);
			}
		}
		if (prog.delta_e()) {
			const size_t regions = prog.probes.empty() ? 1 : prog.probes.size(), pixels = options.res[0] * options.res[1];
			const std::vector<uint8_t> labels = prog.probes.empty() ? std::vector<uint8_t>() : renderer.labels_from_rects(prog.probes);
			const ssx::Renderer::DenoiseParams* const dn = (prog.spectral_denoise || prog.delta_e_denoise) ? &prog.denoise_params : nullptr;
			const ssx::Renderer::DemodParams* const dm = prog.demodulate ? &prog.demod_params : nullptr;
			// the whites' common scale: --delta-e-white-y is side A's white's Y; without it side A's mean finite Y is 0.18 of its white's Y
			double scale = 0.0;
			if (prog.delta_e_white_y > 0.0) scale = prog.delta_e_white_y / delta_e_white[0][1];
			else {
				const std::vector<float> xyz = glare_a ? renderer.develop_glare(develop_weights.data(), 3, *glare_a, prog.spectral_denoise ? dn : nullptr, prog.spectral_denoise ? dm : nullptr, optics_a, defocus_a)
				                                       : renderer.develop(develop_weights.data(), 3, prog.spectral_denoise ? dn : nullptr, prog.spectral_denoise ? dm : nullptr, optics_a, defocus_a);
				double sum = 0.0; size_t n = 0;
				for (size_t p = 0; p < pixels; ++p) if (std::isfinite(xyz[3 * p + 1])) { sum += static_cast<double>(xyz[3 * p + 1]); ++n; }
				const double mean = n ? sum / static_cast<double>(n) : 0.0;
				if (!(mean > 0.0)) throw ssx::HostError{ SSX_ERR_ARG, "--delta-e: side A's development has no positive mean Y to scale the whites by; give `--delta-e-white-y=<Y>`" };
				scale = (mean / 0.18) / delta_e_white[0][1];
			}
			for (int x = 0; x < 2; ++x) for (int c = 0; c < 3; ++c) delta_e_white[x][c] *= scale;
			const ssx::Renderer::DeltaESide side_a{ develop_weights.data(), prog.spectral_denoise, optics_a, defocus_a, glare_a }, side_b{ delta_e_weights.data(), prog.delta_e_denoise, optics_b, defocus_b, glare_b };
			const ssx::Renderer::DeltaE e = renderer.delta_e(side_a, side_b, delta_e_white[0], delta_e_white[1], labels, regions, prog.delta_e_threshold, !prog.delta_e_output.empty(), dn,
			                                                 (prog.spectral_denoise || prog.delta_e_denoise) ? dm : nullptr);
			if (!prog.delta_e_csv.empty()) renderer.save_delta_e_csv(prog.delta_e_csv, e);
			if (!prog.delta_e_output.empty()) renderer.save_delta_e_map(prog.delta_e_output, e);
			for (size_t r = 0; r < regions; ++r)
				std::fprintf(stderr, "Colour difference, region %zu: mean dE*ab %.4g, mean dE00 %.4g, max dE00 %.4g (whites' Y %.6g).\n", r, e.mean[2 * r], e.mean[2 * r + 1], e.max[2 * r + 1], delta_e_white[0][1]);
		}
		if (!prog.develop_output.empty()) { // X, Y, Z from the bins, the alpha of the render's image, then the store of --output
			std::vector<float> xyz;
			if (prog.sensor.on) { // through the sensor: the ccm has taken the demosaiced image to X, Y, Z
				ssx::Renderer::SensorImage img = renderer.develop_sensor(sensor, prog.spectral_denoise ? &prog.denoise_params : nullptr, prog.demodulate ? &prog.demod_params : nullptr, optics_a, defocus_a, glare_a);
				if (!prog.sensor.raw_output.empty()) {
					const size_t shape[2] = { options.res[1], options.res[0] };
					ssx::save_npy_f32(prog.sensor.raw_output, img.raw.data(), shape, 2);
				}
				xyz = std::move(img.out);
			} else if (glare_a) xyz = renderer.develop_glare(develop_weights.data(), 3, *glare_a, prog.spectral_denoise ? &prog.denoise_params : nullptr, prog.demodulate ? &prog.demod_params : nullptr, optics_a, defocus_a);
			else xyz = renderer.develop(develop_weights.data(), 3, prog.spectral_denoise ? &prog.denoise_params : nullptr, prog.demodulate ? &prog.demod_params : nullptr, optics_a, defocus_a);
			const size_t pixels = options.res[0] * options.res[1];
			ssx::Framebuffer fb(options.res);
			if (prog.display_on || !prog.meter_output.empty()) { // X, Y, Z -> linear sRGB is the finish's matrix (row-major [c'][c]; Mat3 is m[col][row])
				ssx::Renderer::Display display = prog.display;
				for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) display.matrix[3 * r + c] = develop_color->matr_xyz_to_lrgb.m[c][r];
				if (prog.display_on) { // already display-encoded: it goes to the store of --output as it is, past the observer's matrix and transfer function
					ssx::Renderer::Meter meter;
					const std::vector<float> finished = renderer.finish(xyz.data(), display, &meter);
					if (!prog.meter_output.empty()) save_meter_csv(prog.meter_output, meter);
					for (size_t p = 0; p < pixels; ++p) {
						for (int c = 0; c < 3; ++c) fb.data()[4 * p + c] = finished[3 * p + c];
						fb.data()[4 * p + 3] = renderer.xyza[4 * p + 3];
					}
					fb.save(prog.develop_output);
				} else { // --meter-output alone: the metering a finish would start with, nothing else
					float luma[3];
					ssx::Renderer::display_luma(display.matrix, luma);
					save_meter_csv(prog.meter_output, renderer.meter_images(xyz.data(), luma));
				}
			}
			if (!prog.display_on) {
				std::vector<float> xyza(pixels * 4);
				for (size_t p = 0; p < pixels; ++p) { xyza[4 * p] = xyz[3 * p]; xyza[4 * p + 1] = xyz[3 * p + 1]; xyza[4 * p + 2] = xyz[3 * p + 2]; xyza[4 * p + 3] = renderer.xyza[4 * p + 3]; }
				develop_color->xyza_to_srgba(xyza.data(), fb.data(), pixels);
				fb.save(prog.develop_output);
			}
		}
		if (!prog.checkpoint.empty()) renderer.save_checkpoint(prog.checkpoint);
	} catch (const ssx::HostError& e) {
		std::fprintf(stderr, "%s\n", e.message.c_str());
		return e.code;
	}
	return 0;
}

/* ssx_host.h -- C entry points of the host-side library (libssx_host.so): table and scene
 * preparation that stays on the CPU, exactly as in the reference (Color::init, src/util/color.cpp:
 * 72-155; Scene::get_new_*, src/scene.cpp:32-415; the XYZ->sRGB store of src/renderer.cpp:298).
 * It produces the ssx_scene_desc that ssx_upload_scene (ssx.h) consumes.  Used by the Python
 * binding; the C++ host (simple_spectral_amd/host/) uses the classes directly.
 */
#ifndef SSX_HOST_H
#define SSX_HOST_H

#include "ssx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssh_scene ssh_scene;

/* scene_name: "cornell" | "cornell-srgb" | "plane-srgb" (else -3, as src/renderer.cpp:32-38).
 * observer: 1931 | 2006 (CIE_OBSERVER, src/stdafx.hpp:82-86).
 * tex_rgb: decoded RGB8 texture (rows top to bottom) for the -srgb scenes, or NULL to load
 * texture_path (PNG) with the library's own decoder.  light_scale: `lightsc` (src/scene.cpp:291-293). */
int ssh_scene_create(const char* scene_name, const char* data_dir, int observer,
                     const uint8_t* tex_rgb, uint32_t tex_w, uint32_t tex_h, const char* texture_path,
                     float light_scale, ssh_scene** out);
/* Bit 9 (0x200) of `uplift`: RENDER_MODE_RGB (SSX_MODE_RGB in ssx.h; the low byte is then ignored):
 * the scene carries linear-RGB triples, ssh_xyza_to_srgba applies only the sRGB transfer function.
 * As ssh_scene_create, plus the uplift variant (SSX_UPLIFT_OURS | SSX_UPLIFT_MENG | SSX_UPLIFT_JH).
 * For MENG, jh_coeff_path names the grid file ("SSXMENG1", simple_spectral_amd/host/meng2015.hpp;
 * -1 when missing) and ssh_xyza_to_srgba applies the Meng output transform (src/util/color.cpp:
 * 243-254); like JH it requires the CIE 1931 observer.  For JH the model is
 * loaded from jh_coeff_path when that file exists ("SPEC" format of rgb2spec_load), otherwise
 * fitted by the library's own optimiser at resolution jh_res (and written to jh_coeff_path when one
 * is given).  JH requires the CIE 1931 observer (src/stdafx.hpp:107-109).  Bit 8 (0x100) of `uplift`
 * builds the scene for the integrator without EXPLICIT_LIGHT_SAMPLING (plane-srgb's textured quad
 * becomes a MaterialMirror, src/scene.cpp:346-355). */
int ssh_scene_create_ex(const char* scene_name, const char* data_dir, int observer,
                        const uint8_t* tex_rgb, uint32_t tex_w, uint32_t tex_h, const char* texture_path,
                        float light_scale, uint32_t uplift, const char* jh_coeff_path, uint32_t jh_res,
                        ssh_scene** out);
void ssh_scene_destroy(ssh_scene* scene);
const ssx_scene_desc* ssh_scene_desc(const ssh_scene* scene);

/* Color::ciexyz_to_srgb on n float4 {X,Y,Z,alpha} pixels -> {sR,sG,sB,alpha} (src/renderer.cpp:298) */
int ssh_xyza_to_srgba(const ssh_scene* scene, const float* xyza, float* srgba, size_t n);

/* Framebuffer::save (src/framebuffer.cpp:39-176): format from the extension (.csv/.hdr/.pfm,
 * anything else PNG); srgba is width*height float4, row 0 = bottom. */
int ssh_save_image(const char* path, const float* srgba, uint32_t width, uint32_t height);

/* PNG -> RGB8 rows top to bottom (what lodepng::decode(..., LCT_RGB) gives, src/material.cpp:11-14).
 * *rgb_out is malloc'ed; release with ssh_free. */
int ssh_load_png_rgb8(const char* path, uint8_t** rgb_out, uint32_t* width, uint32_t* height);
void ssh_free(void* p);

/* Colour-table introspection for tests: name in {D65_rad_XYZ (3), xyz_to_lrgb (9, column-major),
 * lrgb_to_xyz (9)}; returns the number of floats written. */
int ssh_color_values(const ssh_scene* scene, const char* name, float* out, int capacity);

/* The checkpoint file of a render: what ssx_sums_export hands out (ssx.h), in one file -- magic "SSXCKPT1", the ssx_sums_info_t, the scene's
 * name and an options text ("key=value" lines: what rebuilds the scene), the [height][width][4] sums, the [height][width] S2 of the noise
 * estimate when noise_s2 is not NULL, and a trailing 64-bit checksum.  Written next to `path` and renamed over it. */
int ssh_checkpoint_save(const char* path, const ssx_sums_info_t* info, const char* scene_name, const char* options_text,
                        const double* sums, const double* noise_s2);
/* Reads one.  *sums_out and *noise_s2_out (NULL in the file without S2) are malloc'ed: release with ssh_free.  scene_name / options_text
 * (optional) receive the terminated texts, cut to their buffers.  A truncated or altered file, or one with another magic: SSX_ERR_DATA. */
int ssh_checkpoint_load(const char* path, ssx_sums_info_t* info, char* scene_name, size_t scene_name_size, char* options_text, size_t options_text_size,
                        double** sums_out, double** noise_s2_out);
/* The combine of the ranks' exports: dst's pixels that src_info's exporter owns (tile_first / tile_stride / tile_skew) <- src's, bit for bit
 * -- by ownership mask, not by adding (-0.0 stays -0.0).  dst_s2 / src_s2: the same for S2, or NULL. */
int ssh_sums_merge(double* dst, double* dst_s2, const double* src, const double* src_s2, const ssx_sums_info_t* src_info);
/* A checkpoint that also carries the wavelength bins of a render with spectral output -- what ssx_spectral_read hands out as sums and counts and
 * ssx_spectral_import takes back (ssx.h) -- so that a resumed render keeps them.  Such a file has the magic "SSXCKPT2": the fields of "SSXCKPT1" up to
 * and including S2, then the ssx_spectral_info_t preceded by its byte count, the sums [height][width][bins] (binary64), the counts [height][width][bins / 4]
 * (uint32), then the checksum (host/checkpoint.hpp has the layout).  spectral_info == NULL: exactly ssh_checkpoint_save, byte for byte.  SSX_ERR_ARG:
 * bins no multiple of 4 in 4..64; a width, height or done_spp that differs from info's; a NULL array. */
int ssh_checkpoint_save_spectral(const char* path, const ssx_sums_info_t* info, const char* scene_name, const char* options_text, const double* sums, const double* noise_s2,
                                 const ssx_spectral_info_t* spectral_info, const double* spectral_sums, const uint32_t* spectral_counts);
/* Reads either kind (so does ssh_checkpoint_load, which passes over the bins).  From an "SSXCKPT1" file spectral_info->bins is 0 and both array outputs
 * are NULL; otherwise they are malloc'ed like *sums_out: release with ssh_free.  SSX_ERR_DATA also: a bin count outside {4, ..., 64}, arrays whose size does
 * not follow from the header. */
int ssh_checkpoint_load_spectral(const char* path, ssx_sums_info_t* info, char* scene_name, size_t scene_name_size, char* options_text, size_t options_text_size,
                                 double** sums_out, double** noise_s2_out, ssx_spectral_info_t* spectral_info, double** spectral_sums_out, uint32_t** spectral_counts_out);
/* ssh_sums_merge's rule for the bins: dst's pixels that src_sums_info's exporter owns <- src's, bit for bit, sums [height][width][bins] and counts
 * [height][width][bins / 4] (either pair may be NULL).  The merged arrays of all ranks are what a context of any ownership imports. */
int ssh_spectral_merge(double* dst_sums, uint32_t* dst_counts, const double* src_sums, const uint32_t* src_counts, uint32_t bins, const ssx_sums_info_t* src_sums_info);
/* A checkpoint that also carries the bins' second moments -- what ssx_spectral_variance hands out as q and ssx_spectral_moments_import takes back (ssx.h) -- so
 * that a resumed render keeps its error bars and its spectral stopping rule.  Such a file has the magic "SSXCKPT3": the "SSXCKPT2" layout up to and including
 * the counts, then q [height][width][bins] (binary64), then the checksum over every byte before it.  q == NULL: exactly ssh_checkpoint_save_spectral, byte for
 * byte.  SSX_ERR_ARG also: q without bins (spectral_info == NULL). */
int ssh_checkpoint_save_moments(const char* path, const ssx_sums_info_t* info, const char* scene_name, const char* options_text, const double* sums, const double* noise_s2,
                                const ssx_spectral_info_t* spectral_info, const double* spectral_sums, const uint32_t* spectral_counts, const double* q);
/* Reads all three kinds (so do ssh_checkpoint_load and ssh_checkpoint_load_spectral, which pass over what they do not return).  *q_out is NULL from a file
 * without the moments, otherwise malloc'ed like *sums_out: release with ssh_free.  SSX_ERR_DATA also: truncation or an altered bit anywhere in q, one byte
 * more or less, the "SSXCKPT2" or "SSXCKPT1" magic on the longer file, the "SSXCKPT3" magic on a file without q. */
int ssh_checkpoint_load_moments(const char* path, ssx_sums_info_t* info, char* scene_name, size_t scene_name_size, char* options_text, size_t options_text_size,
                                double** sums_out, double** noise_s2_out, ssx_spectral_info_t* spectral_info, double** spectral_sums_out, uint32_t** spectral_counts_out,
                                double** q_out);
/* ssh_sums_merge's rule for the second moments: dst_q's pixels that src_sums_info's exporter owns <- src_q's, bit for bit, [height][width][bins]. */
int ssh_moments_merge(double* dst_q, const double* src_q, uint32_t bins, const ssx_sums_info_t* src_sums_info);

/* A NumPy .npy file (format version 1.0, '<f4', C order) of `data` with the given shape: what np.load reads, and the bytes np.save writes for the
 * same array.  The CLI's --spectral-output writes the spectral image with it: shape (height, width, bins), row 0 = bottom. */
int ssh_save_npy_f32(const char* path, const float* data, const uint32_t* shape, uint32_t ndim);

/* The region probes' results (ssx.h "Spectral moments and region probes"; SS, NN, VV, UU: [regions][bins] of ssx_spectral_probe / ssx_probe_arrays) as their
 * readers take them: mean = NN ? SS / NN : 0 and stderr = sqrt(VV * NN / (NN - UU)) / NN (NaN when NN - UU == 0), binary64, in this order; either output may be NULL. */
int ssh_probe_derive(uint32_t regions, uint32_t bins, const double* SS, const uint64_t* NN, const double* VV, const uint64_t* UU, double* mean, double* std_err);
/* ... and as a text file, what the CLI's --probe-output writes: the line "region,bin,wavelength,mean,stderr,samples,unestimated", then one line per region and bin
 * in that order -- the bin's centre lambda_min + (b + 0.5) * bin_width in binary32 ("%.9g"), mean and stderr ("%.17g", "nan" for a NaN), NN and UU. */
int ssh_probe_save_csv(const char* path, uint32_t regions, uint32_t bins, float lambda_min, float bin_width, const double* SS, const uint64_t* NN, const double* VV, const uint64_t* UU);

/* The comparison of two spectral renders (ssx.h "Comparing two spectral renders"; DD, VV, X2, CC, NC, EX: [regions][bins] of ssx_spectral_compare /
 * ssx_spectral_compare_arrays) as its readers take it: mean_diff, stderr, z, chi2, exceed and coverage [regions][bins] as DERIVED BY THE HOSTS defines them,
 * binary64, each NaN where its denominator is 0; any of the six outputs may be NULL. */
int ssh_compare_derive(uint32_t regions, uint32_t bins, const double* DD, const double* VV, const double* X2, const uint64_t* CC, const uint64_t* NC, const uint64_t* EX,
                       double* mean_diff, double* std_err, double* z, double* chi2, double* exceed, double* coverage);
/* ... and as a text file, what the CLI's --compare-output writes: the line "region,bin,wavelength,mean_diff,stderr,z,chi2,exceed,comparable,not_comparable", then
 * one line per region and bin -- the bin's centre as ssh_probe_save_csv writes it, the five figures ("%.17g", "nan" for a NaN), CC and NC. */
int ssh_compare_save_csv(const char* path, uint32_t regions, uint32_t bins, float lambda_min, float bin_width, const double* DD, const double* VV, const double* X2,
                         const uint64_t* CC, const uint64_t* NC, const uint64_t* EX);

/* The colour difference of two developments (ssx.h "Colour difference of two developments"; SUM, SSQ, MAX, NF, NX, EX: [regions][2] of ssx_delta_e_images /
 * ssx_spectral_delta_e, metric 0 dE*ab, 1 dE00) as its readers take it: mean, rms, max, exceed and coverage [regions][2] as DERIVED BY THE HOSTS defines them,
 * binary64, each NaN where its denominator is 0; any of the five outputs may be NULL. */
int ssh_delta_e_derive(uint32_t regions, const double* SUM, const double* SSQ, const float* MAX, const uint64_t* NF, const uint64_t* NX, const uint64_t* EX,
                       double* mean, double* rms, double* max, double* exceed, double* coverage);
/* ... and as a text file: the line "region,metric,mean,rms,max,exceed,coverage,finite,nonfinite", then one line per region and metric ("ab", then "00") -- the
 * five figures ("%.17g", "nan" for a NaN), NF and NX. */
int ssh_delta_e_save_csv(const char* path, uint32_t regions, const double* SUM, const double* SSQ, const float* MAX, const uint64_t* NF, const uint64_t* NX, const uint64_t* EX);

/* The spectral noise figure's totals (ssx.h "Spectral noise figure"; EV, EM, PP, PU: [bins] of ssx_spectral_noise / ssx_spectral_noise_reduce) as their readers
 * take them: *noise, *coverage and rel[bins] as DERIVED BY THE HOSTS defines them, binary64, in that order; any of the three outputs may be NULL. */
int ssh_spectral_noise_derive(uint32_t bins, const double* EV, const double* EM, const uint64_t* PP, const uint64_t* PU, double* noise, double* coverage, double* rel);
/* ... and as a text file, what the CLI's --spectral-noise-output writes: the line "bin,wavelength,rel,EV,EM,estimable,unestimated", then one line per bin -- the
 * bin's centre as ssh_probe_save_csv writes it, rel, EV and EM ("%.17g", "nan" for a NaN), PP and PU. */
int ssh_spectral_noise_save_csv(const char* path, uint32_t bins, float lambda_min, float bin_width, const double* EV, const double* EM, const uint64_t* PP, const uint64_t* PU);

/* ---- Developing the spectral bins (ssx.h "Developing the spectral bins": the definitions are there, operation by operation) ----------------------------------- */
typedef struct ssh_spectrum_t { const float* samples; uint32_t n; float low, high; } ssh_spectrum_t; /* n >= 2 uniform samples over [low, high] */
enum { SSH_SPACE_XYZ = 0, SSH_SPACE_LRGB = 1 };
/* The weight matrix W[channels][bins] of ssx_develop_images / ssx_spectral_develop for bins of a render with this lambda_min and lambda_step (ssx_scene_desc).
 * responses: `channels` response curves (a camera's, 1..16), or NULL for the x-bar, y-bar, z-bar tables of `observer` (1931 | 2006, from data_dir; channels must
 * then be 3).  filter: an optional spectrum in front of the lens (NULL: none).  gain: an optional factor per bin, e.g. ssh_relight_gain's (NULL: none).  space:
 * SSH_SPACE_XYZ -- the weights as integrated; SSH_SPACE_LRGB -- three rows, taken to linear BT.709 by the XYZ -> lRGB matrix of `observer`'s colour tables (needs
 * observer and data_dir also with responses given).  weights: float [channels][bins]; weights64 (optional): the same before the final rounding. */
int ssh_develop_weights(const char* data_dir, int observer, const ssh_spectrum_t* responses, uint32_t channels, const ssh_spectrum_t* filter, const double* gain,
                        int space, uint32_t bins, float lambda_min, float lambda_step, float* weights, double* weights64);
/* gain[b] = integral of to_spectrum over bin b / integral of from_spectrum, 0 where the latter is 0.  As a gain it turns a render lit by from_spectrum into one lit
 * by to_spectrum -- exactly only when every emitter of the scene carries from_spectrum up to a scale (ssh_emitter_spectrum), and up to the variation of the ratio
 * inside a bin. */
int ssh_relight_gain(const ssh_spectrum_t* from_spectrum, const ssh_spectrum_t* to_spectrum, uint32_t bins, float lambda_min, float lambda_step, double* gain);
/* A reference white for the colour difference: the development, by weights [3][bins] (ssh_develop_weights, xyz space), of the illuminant's mean over each bin --
 * out[c] = sum over b of (double)weights[c][b] * (integral of the illuminant over bin b / the bin's width), binary64, ascending b, integrated as ssh_relight_gain
 * integrates.  illuminant NULL: equal energy.  Which white a comparison uses is the caller's viewing decision, like exposure: it sets the absolute size of every dE. */
int ssh_develop_white(const float* weights, uint32_t bins, float lambda_min, float lambda_step, const ssh_spectrum_t* illuminant, double out[3]);
/* A lens for ssx_optics_images / ssx_spectral_develop_optics (ssx.h "Developing through a lens"): the per-bin tables of ssx_optics_params for bins of a render
 * with this lambda_min and lambda_step, from a lateral chromatic coefficient, a blur sigma_ref (pixels) at lambda_ref and an axial coefficient (pixels of defocus
 * blur per unit of relative wavelength offset).  Binary64, IEEE operations in the order written, rounded to binary32 once at the end.  M = bins / 4:
 *     lc_b = (double)lambda_min + (b + 0.5) * ((double)lambda_step / M)        the bin's centre;        u = (lc_b - lambda_ref) / lambda_ref
 *     s_b = (float)(1.0 + lateral * u)                                         refused unless finite and > 0
 *     sd = sigma_ref * lc_b / lambda_ref   (diffraction grows with lambda);    ax = axial * u;    sigma_b = sqrt(sd * sd + ax * ax)
 *     r_b = min(max_radius, ceil(3.0 * sigma_b)), 0 where sigma_b * sigma_b == 0 (sigma_b is 0 or its square underflows; the bin's taps are then all 0 and never read)
 *     k_b[d] = exp(-(double)(d * d) / (2.0 * (sigma_b * sigma_b))) for d = -r_b .. r_b;  total = their sum in ascending d from 0.0;  taps[b][d + R] = (float)(k_b[d] / total)
 * taps outside |d| <= r_b are 0.  lateral = axial = sigma_ref = 0 gives identity parameters.  scale_out [bins], radius_out [bins], taps_out [bins][2 max_radius + 1].
 * SSX_ERR_ARG: NULL pointers, bins not a multiple of 4 in 4..64, max_radius above 12, a non-finite argument, lambda_step or lambda_ref not positive, sigma_ref < 0. */
int ssh_optics_lens(uint32_t bins, float lambda_min, float lambda_step, double lambda_ref, double lateral, double sigma_ref, double axial, uint32_t max_radius,
                    float* scale_out, uint32_t* radius_out, float* taps_out);
/* A thin lens for ssx_defocus_images / ssx_spectral_develop_lens (ssx.h "Depth of field after the render"): the gain K and the per-bin inverse focus distances of
 * ssx_defocus_params for a render with this vertical field of view (ssh_scene_vfov), `height` rows and `bins` bins of this lambda_min and lambda_step, from an aperture diameter and a focus distance in scene units and an axial
 * coefficient (inverse scene units per unit of relative wavelength offset: longitudinal chromatic aberration).  Binary64, IEEE operations in the order written,
 * libm's tan, rounded to binary32 once at the end.  M = bins / 4:
 *     vfov = (double)vfov_deg * (3.14159265358979323846 / 180.0);     v_px = ((double)height / 2.0) / tan(vfov / 2.0)     the image distance in pixels
 *     gain = (float)(0.5 * aperture * v_px)                                                  the blur RADIUS in pixels per unit of inverse-depth offset
 *     lc_b = (double)lambda_min + (b + 0.5) * ((double)lambda_step / M);   u = (lc_b - lambda_ref) / lambda_ref
 *     focus_b = (float)max(0.0, 1.0 / focus_distance + axial * u)
 * A point at distance z then has the circle of confusion 0.5 * aperture * v_px * |1 / z - focus_b| pixels: the thin lens focused far beyond its focal length.  The
 * depth guide is a RAY LENGTH from the eye, so the surface in focus is a sphere about the eye of radius 1 / focus_b, not a plane; a planar focus is out of scope.
 * aperture = 0 gives gain 0: the identity.  focus_out [bins].  SSX_ERR_ARG: NULL pointers, a vfov_deg outside (0, 180), bins not a multiple of 4 in 4..64, height 0, a lambda_step not positive, an aperture that is not
 * finite or negative, a focus_distance or lambda_ref not finite and positive, an axial that is not finite, a result that is not finite in binary32. */
int ssh_defocus_thin_lens(float vfov_deg, uint32_t height, uint32_t bins, float lambda_min, float lambda_step, double aperture, double focus_distance, double axial,
                          double lambda_ref, float* gain_out, float* focus_out);
/* *vfov_deg = the vertical field of view of the scene's camera in degrees (what ssh_defocus_thin_lens takes; the scene description carries only the matrix). */
int ssh_scene_vfov(const ssh_scene* scene, float* vfov_deg);
/* ---- Glare for ssx_glare_images / ssx_spectral_develop_glare (ssx.h "Glare: per-bin convolution by FFT").  All of it binary64, rounded to binary32 once at
 * the end.  The library itself takes any psf and any twiddles. */
/* *px, *py = the padded extents of ssx_glare_params: the smallest powers of two >= max(2, width + 2 radius) and max(2, height + 2 radius).  SSX_ERR_ARG: NULL, an
 * empty image, a radius above SSX_GLARE_MAX_RADIUS, an extent above SSX_GLARE_MAX_EXTENT. */
int ssh_glare_plan(uint32_t width, uint32_t height, uint32_t radius, uint32_t* px, uint32_t* py);
/* out [P / 2][2]: T[m] = ((float)cos(x), (float)-sin(x)) with x = (2.0 * 3.14159265358979323846 * m) / P in binary64 and libm's cos and sin; T[0] = (1, 0) and
 * T[P / 4] = (0, -1) exactly.  SSX_ERR_ARG: NULL, a P that is no power of two in 2..SSX_GLARE_MAX_EXTENT. */
int ssh_glare_twiddles(uint32_t P, float* out);
/* psf_out [bins][2 radius + 1][2 radius + 1] and on_out [bins] of ssx_glare_params for an iris of `blades` straight blades (fewer than 3: a disc), for bins of a
 * render with this lambda_min and lambda_step.  THE MODEL: Fraunhofer diffraction of a uniformly lit aperture, whose pattern grows linearly with the wavelength.
 *   - The aperture is a regular polygon of circumradius SSH_GLARE_PUPIL cells about the centre of a SSH_GLARE_GRID^2 grid, first vertex at `rotation` radians; a
 *     cell's value is the fraction of its SSH_GLARE_SUBSAMPLES^2 regularly placed samples that lie inside (anti-aliased edges on a fixed grid).
 *   - I = |DFT|^2 of that grid, by a binary64 radix-2 FFT of this library's own (libm's cos and sin).
 *   - A disc of radius a on a grid of N has its first dark ring at SSH_GLARE_AIRY_ZERO * N / (2 a) frequency samples; the pattern is scaled so that this ring lies
 *     ring_px pixels out at lambda_ref: bin b, centre lc_b = (double)lambda_min + (b + 0.5) * ((double)lambda_step / (bins / 4)), samples I bilinearly at
 *     (dy, dx) * kappa_b, kappa_b = (ring0 / ring_px) * (lambda_ref / lc_b); beyond the grid's Nyquist range (about SSH_GLARE_PUPIL / 1.22 rings) the pattern is 0.
 *   - Each bin's pattern is divided by its sum over the K x K window (ascending dy, dx from 0.0), and psf_b = (1 - strength) * delta + strength * pattern:
 *     `strength` is the share of the light that leaves the geometric image.
 * strength == 0: on_out[b] = 0 for every bin and psf_b = delta.  SSX_ERR_ARG: NULL, bins not a multiple of 4 in 4..64, a radius above SSX_GLARE_MAX_RADIUS, more
 * than 64 blades, a strength outside 0..1, a ring_px, lambda_ref, lambda_min or lambda_step not finite and positive, a rotation not finite. */
#define SSH_GLARE_GRID 1024u
#define SSH_GLARE_PUPIL 128.0
#define SSH_GLARE_SUBSAMPLES 4u
#define SSH_GLARE_AIRY_ZERO 1.2196698912665045
int ssh_glare_aperture(uint32_t bins, float lambda_min, float lambda_step, double lambda_ref, int blades, double rotation, double ring_px, double strength,
                       uint32_t radius, float* psf_out, uint8_t* on_out);
/* ---- A sensor for ssx_sensor_images / ssx_demosaic_images / ssx_spectral_develop_sensor (ssx.h "Developing onto a sensor").  All of it binary64, rounded to
 * binary32 once at the end. */
enum { SSH_DEMOSAIC_BILINEAR = 0, SSH_DEMOSAIC_MHC = 1 };
/* cfa_out [4] and taps_out [4][3][25] of ssx_sensor_params for a 2 x 2 Bayer pattern, "RGGB", "BGGR", "GRBG" or "GBRG": the first two letters are row j = 0, THE
 * BOTTOM ROW, at i = 0 and i = 1, the last two row j = 1; channels R = 0, G = 1, B = 2.  SSH_DEMOSAIC_MHC: the 5 x 5 filters of Malvar, He and Cutler
 * ("High-quality linear interpolation for demosaicing of Bayer-patterned color images", ICASSP 2004), all over 8:
 *     G at an R or B site: centre 4, the four edge neighbours 2, the four axis taps at distance two -1;
 *     R or B at a G site whose row neighbours carry that colour: centre 5, the two row neighbours 4, the four diagonals -1, the two row taps at distance two -1,
 *       the two column taps at distance two 1/2; at a G site of the other kind the transpose;
 *     R at a B site and B at an R site: centre 6, the four diagonals 2, the four axis taps at distance two -3/2;
 *     a site's own colour: the centre tap alone.
 * SSH_DEMOSAIC_BILINEAR: the same without the centre and the distance-two corrections (the neighbours' mean).  Every coefficient is dyadic, every (phase,
 * channel) sums to 1.  Other colour filter arrays are out of scope here (the library takes any tables).  SSX_ERR_ARG: NULL, another pattern, another method. */
int ssh_sensor_bayer(const char* pattern, int method, uint32_t* cfa_out, float* taps_out);
/* The scales of ssx_sensor_params, out[7] = { exposure, inv_exposure, read_var, dn_per_e, e_per_dn, black, white } in the struct's order:
 *     exposure = full_well / white_level      a development that gives white_level fills the well;      inv_exposure = 1 / exposure;      read_var = read_e * read_e
 *     white = 2^bits - 1;   dn_per_e = (white - black) / full_well;   e_per_dn = full_well / (white - black)          a full well lands on white
 * bits = 0: no ADC (white = 0, dn_per_e = e_per_dn = 1, unused).  SSX_ERR_ARG: NULL, a full_well or white_level not finite and positive, bits above 24, a black
 * that is not finite, negative or (with an ADC) not below white, a read_e not finite or negative, a result that is not finite in binary32. */
int ssh_sensor_exposure(double full_well, double white_level, uint32_t bits, double black, double read_e, float* out);
/* The least-squares 3 x 3 that takes the camera's channels to a target's: ccm = target * cam^T * (cam * cam^T)^-1 for cam, target [3][bins] (the weights of
 * ssh_develop_weights: the camera's curves, and the observer's in the space --develop-output writes), by the adjugate.  It is a fit over equal-energy bins, not a
 * white balance.  SSX_ERR_ARG: NULL, bins 0, a singular cam * cam^T (det <= 1e-12 * the product of its diagonal), a result not finite in binary32. */
int ssh_sensor_ccm(const float* cam, const float* target, uint32_t bins, float* ccm_out);
/* STAND-IN response curves for a sensor whose curves nobody supplied (the CLI's --develop-sensor without --develop-sensor-curves).  THEY ARE NO CAMERA'S: three
 * Gaussians, channel 0 (R) peaking at 600 nm, 1 (G) at 540 nm, 2 (B) at 460 nm, each with a standard deviation of 35 nm and a peak of 1, sampled every 5 nm from
 * 380 to 730 nm: samples[k] = (float)exp(-0.5 * ((380 + 5 k - peak) / 35)^2), k = 0 .. 70, binary64 with libm's exp.  samples [SSH_SENSOR_STANDIN_SAMPLES];
 * *low = 380, *high = 730: an ssh_spectrum_t for ssh_develop_weights.  SSX_ERR_ARG: NULL, a channel above 2. */
#define SSH_SENSOR_STANDIN_SAMPLES 71u
int ssh_sensor_standin_curve(uint32_t channel, float* samples, float* low, float* high);
/* ---- The policy of a display for ssx_meter_images / ssx_local_images / ssx_tone_images (ssx.h "Finishing a development for a display").  All of it binary64,
 * rounded to binary32 once at the end. */
/* What a metering says, from hist [4][SSX_METER_KEYS] and special [4][4] of ssx_meter_images.  Quantity 3 is the luminance.  Only the finite positive values (the
 * histogram) are looked at; N_k is their number.
 *   percentile(k, p): with rank = min(max(ceil(p * N_k), 1), N_k), the smallest key whose cumulative count reaches rank, as that key's LOWER EDGE
 *     frombits(key << 19): at most one key (a sixteenth of its octave's start: 6.25 %) below the value a sort of the data finds at that rank.  N_k == 0 gives 0.
 *     percentile_out [4][n_percentiles] for percentiles [n_percentiles] (each in 0..1); both may be NULL with n_percentiles == 0.
 *   out [SSH_METER_OUT]:
 *     [SSH_METER_LOG_AVERAGE]   the log-average of the luminance IN THE PIECEWISE-LINEAR LOGARITHM OF LOCAL, every value taken at its key's centre: with the
 *                               integer S = sum of count * (2 key + 1), q = S div 2N, f = (S mod 2N) / 2N:  2^((q >> 4) - 127) * (1 + ((q & 15) + f) / 16) -- 127 + 1/32 less
 *                               than the mean key over 16 is the mean L.  An image scaled by 2^k has every key moved by 16 k, so q moves by 16 k and f stays: its
 *                               log-average is 2^k times this one EXACTLY (while nothing leaves the normal range).  0 without a finite positive luminance.
 *     [SSH_METER_EXPOSURE]      key_value / log-average (1 where that is 0): the factor that puts the log-average on key_value, 0.18 by convention
 *     [SSH_METER_WHITE]         percentile(3, white_percentile): the highlight that is to reach white;   [SSH_METER_WHITE_EXPOSED] the same times the exposure
 *     [SSH_METER_PIVOT]         L(key_value) as LOCAL defines it: ssx_local_params.pivot
 *     [SSH_METER_GREY + c]      grey-world channel gains: mean_1 / mean_c, the means taken with every value at its key's centre frombits((key << 19) + (1 << 18))
 *     [SSH_METER_PATCH + c]     white-patch channel gains: percentile(1, white_percentile) / percentile(c, white_percentile)
 *                               a gain whose numerator or denominator is 0 is 1; the gains multiply the image's own channels (TONE's gains): a white balance proper
 *                               wants a development in linear RGB
 *     [SSH_METER_COUNT]         N_3 as a float; the rest 0
 * SSX_ERR_ARG: NULL, a key_value that is not finite and positive, a percentile outside 0..1, a result that is not finite in binary32. */
enum { SSH_METER_LOG_AVERAGE = 0, SSH_METER_EXPOSURE = 1, SSH_METER_WHITE = 2, SSH_METER_WHITE_EXPOSED = 3, SSH_METER_PIVOT = 4, SSH_METER_GREY = 5, SSH_METER_PATCH = 8,
       SSH_METER_COUNT = 11 };
#define SSH_METER_OUT 16u
int ssh_meter_derive(const uint32_t* hist, const uint32_t* special, double key_value, double white_percentile, const double* percentiles, uint32_t n_percentiles,
                     float* percentile_out, float* out);
/* curve_out [curve_len] of ssx_tone_params for lo, hi and shift: node idx stands at x = frombits(bits(lo) + (idx << shift)) (the last node may lie beyond hi) and holds
 * oetf(min(max(t(x), 0), 1)), oetf the sRGB transfer function (v <= 0.0031308 ? 12.92 v : 1.055 v^(1/2.4) - 0.055, libm's pow), and t
 *   SSH_TONE_CLIP      t = x
 *   SSH_TONE_REINHARD  t = x (1 + x / white^2) / (1 + x)                      Reinhard et al. 2002, eq. 4: x == white gives 1
 *   SSH_TONE_FILMIC    t = h(2 x) / h(white), h(x) = (x (A x + C B) + D E) / (x (A x + B) + D F) - E / F with A .15, B .5, C .1, D .2, E .02, F .3    (Hable 2010)
 *                      HERE `white` IS HABLE'S W, the linear white of his curve, NOT the value that reaches 1: with his exposure bias of 2 that is x = white / 2, and
 *                      everything above it is clipped.  Renderer.finish and the CLI pass the metered white point all the same: filmic gives its top octave to the clip.
 * SSX_ERR_ARG: NULL, another kind, a white that is not finite and positive, lo, hi, shift or curve_len that ssx_tone_images would refuse. */
enum { SSH_TONE_CLIP = 0, SSH_TONE_REINHARD = 1, SSH_TONE_FILMIC = 2 };
int ssh_tone_curve(int kind, double white, float lo, float hi, uint32_t shift, float* curve_out, uint32_t curve_len);
/* out [3][3], row-major: ssx_tone_params.matrix for an image in CIE XYZ -- the observer's XYZ -> linear sRGB (BT.709 primaries, the project's D65), the matrix
 * ssh_xyza_to_srgba applies.  SSX_ERR_ARG: NULL; SSX_ERR_DATA / SSX_ERR_SCENE: the tables of data_dir. */
int ssh_display_matrix(const char* data_dir, int observer, float* out);
/* *spectrum = index (in desc->spectra) of the emission spectrum that all emissive materials of the scene share up to a scale.  SSX_ERR_SCENE, with the reason in
 * ssh_last_error, when two of them differ or none is emissive: what the CLI's --develop-relight refuses. */
int ssh_emitter_spectrum(const ssx_scene_desc* desc, uint32_t* spectrum);

const char* ssh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

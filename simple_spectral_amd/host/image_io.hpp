// image_io.hpp -- texture decode and framebuffer writers of the host side.
//   load_png_rgb8  : what the reference gets from lodepng::decode(out,w,h,path,LCT_RGB)
//                    (src/material.cpp:10-29): 8-bit RGB, rows top to bottom.
//   save_image     : Framebuffer::save (src/framebuffer.cpp:39-176): .csv / .hdr / .pfm by
//                    extension, anything else PNG (RGBA8, rows flipped to top-to-bottom).
// PNG (de)compression uses zlib; the container code (chunks, CRC, filters) is written here.
#pragma once
#include "scene.hpp"

#include <string>

namespace ssx {

Texture load_png_rgb8(const std::string& path);

// Seeded procedural RGB8 texture, n x n (SURVEY.md section 8(d) "synthetic inputs (iii)"): stands in for the
// reference's data/scenes/crystal-lizard-4096.png (src/scene.cpp:292,357), a 48 MiB blob missing from its
// repository, to reproduce its memory footprint (beyond the 32 MiB of aggregate L2).  Integer arithmetic
// only; simple_spectral_amd/textures.py computes the same bytes.
Texture procedural_texture(uint32_t n, uint32_t seed);
// "procedural:N" or "procedural:N:SEED" -> procedural_texture, anything else -> load_png_rgb8
Texture load_texture(const std::string& path);

// srgba: width*height float4 {sR,sG,sB,alpha}, index j*width+i, row 0 = bottom
// (src/framebuffer.hpp:26-34).
void save_image(const std::string& path, const float* srgba, size_t width, size_t height);

// A NumPy .npy file, format version 1.0: little-endian float32 ('<f4'), C order, the given shape -- the header np.save writes (padded to a
// multiple of 64 bytes), then the values as they lie in memory.  The spectral image: shape (height, width, bins), row 0 = bottom.
void save_npy_f32(const std::string& path, const float* data, const size_t* shape, size_t ndim);

// The region probes' results for their readers (include/ssx.h "Spectral moments and region probes"), [regions][bins] each:
//     mean = NN ? SS / NN : 0        stderr = sqrt(VV * NN / (NN - UU)) / NN   (NaN when NN - UU == 0)
// in binary64, the operations in this order.
void probe_derive(size_t regions, size_t bins, const double* SS, const uint64_t* NN, const double* VV, const uint64_t* UU, double* mean, double* std_err);
// ... as a text file: the line "region,bin,wavelength,mean,stderr,samples,unestimated", then one line per region and bin in that order -- the bin's centre
// wavelength lambda_min + (b + 0.5) * bin_width in binary32 (%.9g), mean and stderr (%.17g: they read back to the same binary64; "nan" for a NaN), the counts.
void save_probe_csv(const std::string& path, size_t regions, size_t bins, float lambda_min, float bin_width, const double* SS, const uint64_t* NN, const double* VV, const uint64_t* UU);

// The spectral noise figure for its readers (include/ssx.h "Spectral noise figure"), from the totals EV, EM, PP, PU [bins]: with P, U, EVs, EMs their sums over
// ascending b and mean = EMs / P,
//     noise = sqrt(EVs / P) / mean  (NaN when P == 0 or mean == 0)     coverage = P / (P + U)  (NaN when P + U == 0)
//     rel[b] = sqrt(EV[b] / PP[b]) / (EM[b] / PP[b])                    (NaN when PP[b] == 0 or the bin's mean is 0)
// in binary64, the operations in this order; any output may be NULL.
void spectral_noise_derive(size_t bins, const double* EV, const double* EM, const uint64_t* PP, const uint64_t* PU, double* noise, double* coverage, double* rel);
// ... as a text file: the line "bin,wavelength,rel,EV,EM,estimable,unestimated", then one line per bin -- the bin's centre wavelength as save_probe_csv writes it,
// rel, EV and EM (%.17g: they read back to the same binary64; "nan" for a NaN), PP and PU.
void save_spectral_noise_csv(const std::string& path, size_t bins, float lambda_min, float bin_width, const double* EV, const double* EM, const uint64_t* PP, const uint64_t* PU);

// The comparison of two spectral renders for its readers (include/ssx.h "Comparing two spectral renders"), from the six [regions][bins] arrays:
//     mean_diff = DD / CC     stderr = sqrt(VV) / CC     z = DD / sqrt(VV)     chi2 = X2 / CC     exceed = EX / CC     coverage = CC / (CC + NC)
// in binary64, each NaN where its denominator is 0; any output may be NULL.
void compare_derive(size_t regions, size_t bins, const double* DD, const double* VV, const double* X2, const uint64_t* CC, const uint64_t* NC, const uint64_t* EX,
                    double* mean_diff, double* std_err, double* z, double* chi2, double* exceed, double* coverage);
// the per-pixel signed map of n cells: zmap = diff / sqrt(var) in binary32, 0 where var is +inf (a cell that is not comparable)
void compare_zmap(size_t n, const float* diff, const float* var, float* zmap);
// ... as a text file: the line "region,bin,wavelength,mean_diff,stderr,z,chi2,exceed,comparable,not_comparable", then one line per region and bin -- the bin's
// centre wavelength as save_probe_csv writes it, the five derived figures (%.17g; "nan" for a NaN, "inf" for an infinity), CC and NC.
void save_compare_csv(const std::string& path, size_t regions, size_t bins, float lambda_min, float bin_width, const double* DD, const double* VV, const double* X2,
                      const uint64_t* CC, const uint64_t* NC, const uint64_t* EX);

// The colour difference's region arrays (ssx.h "Colour difference of two developments"; [regions][2]: metric 0 dE*ab, 1 dE00) as their readers take them: mean =
// SUM / NF, rms = sqrt(SSQ / NF), max = MAX, exceed = EX / NF, coverage = NF / (NF + NX), each NaN where its denominator is 0; any output may be nullptr.
void delta_e_derive(size_t regions, const double* SUM, const double* SSQ, const float* MAX, const uint64_t* NF, const uint64_t* NX, const uint64_t* EX,
                    double* mean, double* rms, double* max, double* exceed, double* coverage);
// ... as a text file: the line "region,metric,mean,rms,max,exceed,coverage,finite,nonfinite", then one line per region and metric ("ab", "00"), the figures as
// save_compare_csv writes them.
void save_delta_e_csv(const std::string& path, size_t regions, const double* SUM, const double* SSQ, const float* MAX, const uint64_t* NF, const uint64_t* NX, const uint64_t* EX);

} // namespace ssx

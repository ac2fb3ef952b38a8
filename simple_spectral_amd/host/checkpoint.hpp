// checkpoint.hpp -- the checkpoint file of a render: the raw binary64 pixel sums ssx_sums_export hands out (include/ssx.h), what they
// belong to, and -- when the render kept it -- the noise estimate's S2.  Little-endian, one file:
//     "SSXCKPT1"
//     u32 info_bytes, ssx_sums_info_t
//     u32 n, scene name | u32 n, options text ("key=value" lines: what rebuilds the scene; for the reader's information)
//     u32 has_s2, u32 0
//     f64 sums[height][width][4] | f64 s2[height][width] (has_s2)
//     u64 checksum of every byte before it
// A checkpoint that also carries the wavelength bins of a render with spectral output (ssx_spectral_read's sums and counts) has another magic and one
// more section; without bins the file is, byte for byte, the one above:
//     "SSXCKPT2"
//     u32 info_bytes, ssx_sums_info_t | the two texts | u32 has_s2, u32 0 | f64 sums[height][width][4] | f64 s2[height][width] (has_s2)      as above
//     u32 spectral_info_bytes, ssx_spectral_info_t        (width, height and done_spp those of the ssx_sums_info_t; bins B in {4, 8, ..., 64}, M = B / 4)
//     f64 S[height][width][B] | u32 N[height][width][M]
//     u64 checksum of every byte before it
// A checkpoint that also carries the bins' second moments (ssx_spectral_variance's q) has a third magic and one more array behind the counts; without valid
// moments the file is, byte for byte, one of the two above:
//     "SSXCKPT3"
//     the "SSXCKPT2" layout up to and including N
//     f64 Q[height][width][B]
//     u64 checksum of every byte before it
// A file that is truncated, altered or of another kind, a bin count outside {4, ..., 64} and arrays whose size does not follow from the header are
// refused with SSX_ERR_DATA.
#pragma once
#include "../../include/ssx.h"
#include "spectrum.hpp"

#include <cstring>
#include <string>
#include <vector>

namespace ssx {

struct Checkpoint {
	ssx_sums_info_t info{};
	std::string scene_name, options_text;
	std::vector<double> sums; // [height][width][4]
	std::vector<double> s2;   // [height][width], or empty
	// the wavelength bins (SSXCKPT2), or spectral.bins == 0 and both arrays empty (SSXCKPT1)
	ssx_spectral_info_t spectral{};
	std::vector<double> spectral_sums;     // [height][width][B]
	std::vector<uint32_t> spectral_counts; // [height][width][B / 4]
	std::vector<double> moments;           // the second moments Q [height][width][B] (SSXCKPT3), or empty
};

void checkpoint_save(const std::string& path, const Checkpoint& c); // throws HostError
Checkpoint checkpoint_load(const std::string& path);               // throws HostError{SSX_ERR_DATA}; any of the three kinds of file

// The ownership rule of this library (the kernels': include/ssx.h tile_first / tile_stride / tile_skew): the place of pixel (i, j)'s 8x8 tile in the
// list the devices share out -- row-major, tile row ty rotated by ty * tile_skew columns.  Tile t belongs to the device with tile_first == t % tile_stride,
// as the (t / tile_stride)-th of its tiles.
inline size_t shared_tile(size_t width, size_t tile_skew, size_t i, size_t j) {
	const size_t tiles_x = (width + 7u) / 8u;
	return (j / 8) * tiles_x + (i / 8 + ((j / 8) * (tile_skew % tiles_x)) % tiles_x) % tiles_x;
}
// Does the exporter described by `info` own pixel (i, j)?
bool sums_owner(const ssx_sums_info_t& info, size_t i, size_t j);
// dst's pixels that `src_info` owns <- src's, bit for bit (a merge by ownership mask, not a sum: -0.0 stays -0.0); s2 likewise where both are given
void sums_merge(double* dst, double* dst_s2, const double* src, const double* src_s2, const ssx_sums_info_t& src_info);
// The same rule for arrays with n values per pixel: dst[p][0..n) <- src[p][0..n) for every pixel p that `src_info` owns.  Every combine of the devices' shares
// by ownership goes through here (spectral_merge; Renderer::spectral_image, denoise_spectral and develop).
template <class T>
void merge_owned(T* dst, const T* src, size_t n, const ssx_sums_info_t& src_info) {
	for (size_t j = 0; j < src_info.height; ++j) for (size_t i = 0; i < src_info.width; ++i) {
		if (!sums_owner(src_info, i, j)) continue;
		const size_t p = (j * src_info.width + i) * n;
		std::memcpy(dst + p, src + p, n * sizeof(T)); // (the bytes: -0.0 and a NaN's payload stay what they are)
	}
}
// ... for the wavelength bins: sums [height][width][bins] and counts [height][width][bins / 4] (either pair may be NULL)
void spectral_merge(double* dst_sums, uint32_t* dst_counts, const double* src_sums, const uint32_t* src_counts, size_t bins, const ssx_sums_info_t& src_info);
// ... and for their second moments: q [height][width][bins]
void moments_merge(double* dst_q, const double* src_q, size_t bins, const ssx_sums_info_t& src_info);

} // namespace ssx

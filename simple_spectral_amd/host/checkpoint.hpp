// checkpoint.hpp -- the checkpoint file of a render: the raw binary64 pixel sums ssx_sums_export hands out (include/ssx.h), what they
// belong to, and -- when the render kept it -- the noise estimate's S2.  Little-endian, one file:
//     "SSXCKPT1"
//     u32 info_bytes, ssx_sums_info_t
//     u32 n, scene name | u32 n, options text ("key=value" lines: what rebuilds the scene; for the reader's information)
//     u32 has_s2, u32 0
//     f64 sums[height][width][4] | f64 s2[height][width] (has_s2)
//     u64 checksum of every byte before it
// A file that is truncated, altered or of another kind is refused with SSX_ERR_DATA.
#pragma once
#include "../../include/ssx.h"
#include "spectrum.hpp"

#include <string>
#include <vector>

namespace ssx {

struct Checkpoint {
	ssx_sums_info_t info{};
	std::string scene_name, options_text;
	std::vector<double> sums; // [height][width][4]
	std::vector<double> s2;   // [height][width], or empty
};

void checkpoint_save(const std::string& path, const Checkpoint& c); // throws HostError
Checkpoint checkpoint_load(const std::string& path);               // throws HostError{SSX_ERR_DATA}

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

} // namespace ssx

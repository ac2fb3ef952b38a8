// ssx_pixel_grid.h -- which device owns pixel (i, j), and where its sums are: the one statement of that rule for the per-pixel kernels
// (ssx_finalize_kernel in ssx_kernels.hip, the five of ssx_progressive.hip) and the host code of ssx_api.hip's translation unit.  Not among the
// sources the run-time compiler is given (build.py EMBED): the path and generate kernels go the other way, tile_of_slot (ssx_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// an image and one device's share of its 8x8 tiles (ssx_render_params); tile_skew already reduced modulo tiles_x (pixel_grid, ssx_api.hip)
struct SsxPixelGrid { uint32_t width, height, tiles_x, tile_first, tile_stride, tile_skew; };

// The place of the pixel's tile in the list the devices share out: row-major, tile row ty rotated by ty * tile_skew columns.  Tile t of
// that list is the (t / tile_stride)-th tile of the device with tile_first == t % tile_stride.
__host__ __device__ inline uint32_t ssx_shared_tile(const SsxPixelGrid& g, uint32_t i, uint32_t j) {
	return (j >> 3) * g.tiles_x + ((i >> 3) + ((j >> 3) * g.tile_skew) % g.tiles_x) % g.tiles_x;
}
__host__ __device__ inline bool ssx_owns_pixel(const SsxPixelGrid& g, uint32_t i, uint32_t j) { return ssx_shared_tile(g, i, j) % g.tile_stride == g.tile_first; }

// the pixel's X sum in the accumulator's [tile (row-major)][component][pixel of the tile] layout (components 64 doubles apart: unit_fold)
__device__ __forceinline__ size_t ssx_sum_slot(uint32_t i, uint32_t j, uint32_t tiles_x) {
	return (size_t)((j >> 3) * tiles_x + (i >> 3)) * 256u + ((j & 7u) * 8u + (i & 7u));
}

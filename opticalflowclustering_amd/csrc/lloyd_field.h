// lloyd_field.h -- how the Lloyd tile sweeps cut a stack of (u,v) fields (n_fields x H x W x 2 f32) into 2-D tiles.
// One place for the tile -> sample map: k_tile_probe, k_tile_meta, the walk and the label stores of lloyd_tiles.hip's
// field kernels use it, and so does the host (ofc_lloyd_field_origin, tests/test_lloyd_field_layout_host.py).
//
//   tile   FIELD_TW x FIELD_TH pixels = 64 samples.  Lane r16 of the 16 lanes that walk a tile takes the quad (4
//          consecutive pixels, 32 B) number r16 % FIELD_QPR of tile row r16 / FIELD_QPR.
//   group  64 x 8 pixels = 8 tiles (FIELD_GTX across, FIELD_GTY down), index g over (field, band of 8 rows, 64-px column).
//          H % 8 == 0, so the fields stack into one image of n_fields * H rows and g = band * (W / 64) + column.
//   tile records are group-major: t = g * 8 + ty * FIELD_GTX + tx, a group's 8 records are contiguous.
// The shape is a build-time decision ("2-D tiles"): 16 x 4 shipped, 8 x 8 measured against it.
#pragma once
#include <cstdint>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace ofc {

#ifndef OFC_FIELD_TW
#define OFC_FIELD_TW 16
#endif
constexpr int FIELD_TW = OFC_FIELD_TW, FIELD_TH = 64 / FIELD_TW;    // tile, pixels
constexpr int FIELD_GW = 64, FIELD_GH = 8;                          // group, pixels
constexpr int FIELD_GTX = FIELD_GW / FIELD_TW, FIELD_GTY = FIELD_GH / FIELD_TH;
constexpr int FIELD_QPR = FIELD_TW / 4;                             // quads per tile row
static_assert(FIELD_TW * FIELD_TH == 64 && FIELD_GTX * FIELD_GTY == 8 && FIELD_QPR >= 1 && FIELD_TH <= FIELD_GH, "tile shape");

// can a stack of W x H fields be cut this way?  (sample indices / 4 are kept in 32 bits)
__host__ __device__ inline bool field_geometry_ok(int64_t W, int64_t H, int64_t n_fields)
{
    return W > 0 && H > 0 && n_fields > 0 && W % FIELD_GW == 0 && H % FIELD_GH == 0 && W <= (1 << 24) &&
           n_fields * H <= (int64_t)0x7fffffff / W * 4;
}
// first sample (index into the stack's n_fields * H * W samples) of group g
__host__ __device__ inline int64_t field_group_origin(int64_t g, int W)
{
    const int64_t gx_n = W / FIELD_GW, band = g / gx_n;
    return band * FIELD_GH * W + (g - band * gx_n) * FIELD_GW;
}
// offset of tile ti (0..7) of a group from the group's origin, samples
__host__ __device__ inline int field_tile_offset(int ti, int W)
{
    return (ti / FIELD_GTX) * FIELD_TH * W + (ti % FIELD_GTX) * FIELD_TW;
}
// offset of lane r16's quad (0..15) from its tile's origin, samples
__host__ __device__ inline int field_quad_offset(int r16, int W)
{
    return (r16 / FIELD_QPR) * W + (r16 % FIELD_QPR) * 4;
}
// first sample of quad r16 of tile t
__host__ __device__ inline int64_t field_quad_origin(int64_t t, int r16, int W)
{
    return field_group_origin(t >> 3, W) + field_tile_offset((int)(t & 7), W) + field_quad_offset(r16, W);
}

}  // namespace ofc

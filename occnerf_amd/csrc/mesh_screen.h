// What the two resolves of mesh_raster's keys share (mesh_raster.hip mesh_resolve, mesh_texture.hip mesh_resolve_textured;
// DESIGN.md sections 7j, 7o): the key of an empty pixel, the image-size test, the background and the byte a weighted sum of
// bytes is stored as.  The screen-space triangle itself is stated by each resolve; see DESIGN.md section 7o for why.
#pragma once

#include "common.h"

namespace occ {

constexpr unsigned long long kRasterEmpty = ~0ull;        // the key of a pixel no triangle covers

// H and W in 1..kRasterMaxSide and at most 2^28 pixels (mesh_raster.hip, beside the rasteriser's other limits).
bool raster_size_ok(int32_t H, int32_t W);

struct RasterBg {
    uint8_t c[3];
};

// rint, then clamped to a byte (a NaN gives 0).
__device__ __forceinline__ uint8_t raster_byte(double s) {
    const double r = rint(s);
    return (uint8_t)(r > 0.0 ? (r < 255.0 ? r : 255.0) : 0.0);
}

}  // namespace occ

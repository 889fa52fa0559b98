// The distance arithmetic of farthest point sampling, shared by every FPS kernel over C-dimensional rows (staging.hip: equal-sized
// clouds; scene_stage.hip: ragged voxels) so that they select the same rows bit for bit: squared differences accumulated in COLUMN
// order from 0.f, fp32, no contraction (the library is built with -ffp-contract=off).
#pragma once

namespace fc {

// |row - ref|^2 over the first C <= 8 columns; ref[c] = 0 for c >= C.  `row` may point into global memory or LDS.
__device__ __forceinline__ float fps_row_dist2(const float* __restrict__ row, const float (&ref)[8], int C) {
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < C) { const float t = row[c] - ref[c]; d += t * t; }
    return d;
}

}  // namespace fc

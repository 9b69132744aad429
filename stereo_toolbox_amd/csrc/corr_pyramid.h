// Pixel-major pyramids and their linear-interpolation windows, shared by geo_lookup.hip (IGEV family) and corr1d.hip (RAFT
// family): level i of a pyramid over `rows` rows of `len` positions with C channels is [rows][len >> i][C], the levels one
// behind the other in one buffer (avg_pool2d([1, 2]) of the level before along `len`, an odd tail dropped).
#pragma once
#include "stx_common.h"

constexpr int CP_MAX_LEVELS = 4;      // the all-pairs row correlation kernels (corr1d.hip) write up to four levels

__device__ __host__ inline size_t geo_level_offset(long long rows, int len, int C, int lvl) {
    size_t off = 0;
    for (int j = 0; j < lvl; ++j) off += (size_t)rows * (size_t)(len >> j) * (size_t)C;
    return off;
}

// position of the window's first tap: floor(x) - r as an integer that cannot overflow, and the fraction all 2r+1 samples share
__device__ __forceinline__ int geo_window(float x, int radius, float& frac) {
    const float xf = floorf(x);
    frac = x - xf;
    return (int)fminf(fmaxf(xf, -1.0e6f), 1.0e6f) - radius;
}

__device__ __forceinline__ float geo_tap1(const float* row, int t, int len) { return (t < 0 || t >= len) ? 0.f : row[t]; }

__device__ __forceinline__ float geo_lerp(float a, float b, float f) { return fmaf(f, b, (1.f - f) * a); }

// The all-pairs row correlation on the matrix cores with its pooled levels, and its backward (kernels in corr1d.hip):
//   cpyr level 0 [B*H*W1][W2] = scale * sum_c fmap1[b][c][h][w1] * fmap2[b][c][h][w2], levels 1 .. levels - 1 pooled from it.
// A scale of 1.0f is exact (the IGEV form).  The callers check pointers and shapes (levels <= CP_MAX_LEVELS); `what` names
// the entry point in launch errors.  gfmap1 / gfmap2 may be NULL.
int corr_pyramid_fwd_launch(const float* fmap1, const float* fmap2, float* cpyr, int B, int C, int H, int W1, int W2, int levels,
                            float scale, void* stream, const char* what);
int corr_pyramid_bwd_launch(const float* gcpyr, const float* fmap1, const float* fmap2, float* gfmap1, float* gfmap2, int B, int C,
                            int H, int W1, int W2, int levels, float scale, void* stream, const char* what);

// All-pairs 1-D correlation pyramid and its per-iteration lookup of the RAFT family (reference models/RAFTStereo/corr.py:31-61,
// 110-156 with utils/utils.py:59-74 -- RAFT-Stereo and Selective-RAFT use the classes unchanged -- and the disparity-indexed
// variant with its "scale" lookups, models/DEFOMStereo/corr.py:113-181); run once per GRU iteration (32 in validation).
//
//   corr[b,h,w1,w2] = scale * sum_c fmap1[b,c,h,w1] * fmap2[b,c,h,w2],  scale = 1 / sqrt(C)              corr.py:148-156
//   level i+1 = avg_pool2d(level i, [1,2], [1,2]) along w2 (floor: an odd tail is dropped), up to four levels     :122-125
//   lookup: a call is a table of JOBS (level l, radius r, alpha, m); per pixel p a job gives the 2r+1 samples of that pixel's
//           row of level l at x = (base[p] - alpha * disp[p]) * m + k, k = -r .. r; linear interpolation between floor(x) and
//           floor(x) + 1, taps outside [0, len_l - 1] are zero (grid_sample, align_corners=True, zero padding).
//             RAFT          (i, r, 0, 2^-i)  base = coords[:, 0]                                              corr.py:127-146
//             DEFOM         (i, r, 1, 2^-i)  base = the pixel's column                              DEFOMStereo/corr.py:160-168
//             DEFOM scaling (0, rs, s, 1) for every s of scale_list                                                   :150-158
//
// Layout.  The pyramid is PIXEL-MAJOR (corr_pyramid.h), level i [B*H*W1][W2 >> i], so a pixel's lookup touches only its own
// rows, forward and backward: the backward adds into them with plain loads and stores -- no atomics, bitwise reproducible --
// and because it ADDS, the lookups of one training step accumulate into one gradient buffer (ops.py Corr1dLookupFn).
//
// Kernels.
//   corr_pyramid_fwd  one GEMM W1 x C x W2 per image row on v_mfma_f32_16x16x4_f32 (operands straight from the NCHW rows, one
//                     dword per lane, 64-byte segments); the pooled levels come out of the accumulators (neighbouring lanes
//                     hold neighbouring w2) in the same launch.  Also serves stx_geo_corr_fwd (scale 1, at most 3 levels).
//   corr_pyramid_bwd  g_fmap1 = scale * G . fmap2, g_fmap2 = scale * G^T . fmap1 on the same instruction, G = the gradient of
//                     level 0 plus the pooled levels' gradients (0.5 / 0.25 / 0.125 of the parent element), formed while the
//                     operand is loaded.
//   corr1d_lookup_fwd one lane per pixel and job, all jobs of a call in ONE launch (grid.y = job): the stores of a wave are
//                     256-byte runs along w of the NCHW output, the loads the lane's own window of 2r+2 floats.
//   corr1d_lookup_bwd one lane per pixel and LEVEL (grid.y = level): the lane walks the jobs of its level in table order --
//                     several jobs may read one row (the eight scale lookups all read level 0), so they must not run
//                     side by side -- and every tap is one read-modify-write of the row the pixel owns.
#include "corr_pyramid.h"

namespace {

constexpr int GC_THREADS = 256;       // correlation: four waves
constexpr int CL_THREADS = 128;       // lookup kernels: lanes (pixels) per workgroup
constexpr int CL_MAX_JOBS = 8;
constexpr int CL_MAX_RADIUS = 8;

// ------------------------------------------------------------------------------------------------ all-pairs row correlation
// grid (cdiv(W1, 16), H, B), four waves; a wave owns the w2 tiles 4 g .. 4 g + 3 of the groups g = wave, wave + 4, ...
// MFMA 16x16x4 f32: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D[row = 4 (l >> 4) + r][col = l & 15].
__global__ __launch_bounds__(GC_THREADS) void corr_pyramid_fwd_kernel(const float* __restrict__ f1, const float* __restrict__ f2,
                                                                      float* __restrict__ cpyr, int B, int C, int H, int W1, int W2,
                                                                      int levels, float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int w1_0 = (int)blockIdx.x * 16, h = (int)blockIdx.y, b = (int)blockIdx.z;
    const size_t HW1 = (size_t)H * W1, HW2 = (size_t)H * W2;
    const float* a_row = f1 + (size_t)b * C * HW1 + (size_t)h * W1;
    const float* b_row = f2 + (size_t)b * C * HW2 + (size_t)h * W2;
    const size_t rows = (size_t)B * H * W1;
    const int len1 = W2 >> 1, len2 = W2 >> 2, len3 = W2 >> 3;
    float* l0 = cpyr;
    float* l1 = cpyr + geo_level_offset((long long)rows, W2, 1, 1);
    float* l2 = cpyr + geo_level_offset((long long)rows, W2, 1, 2);
    float* l3 = cpyr + geo_level_offset((long long)rows, W2, 1, 3);
    const bool a_ok = w1_0 + li < W1;
    for (int w2_0 = wave * 64; w2_0 < W2; w2_0 += 256) {
        f32x4 acc[4];
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < C; c0 += 4) {
            const int c = c0 + lk;
            const bool c_ok = c < C;
            const float a = (a_ok && c_ok) ? a_row[(size_t)c * HW1 + w1_0 + li] : 0.f;
            float bv[4];
            for (int n = 0; n < 4; ++n) {
                const int w2 = w2_0 + 16 * n + li;
                bv[n] = (c_ok && w2 < W2) ? b_row[(size_t)c * HW2 + w2] : 0.f;
            }
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[n], acc[n], 0, 0, 0);
        }
        for (int n = 0; n < 4; ++n) {
            const int w2 = w2_0 + 16 * n + li;
            for (int r = 0; r < 4; ++r) {
                const int w1 = w1_0 + 4 * lk + r;
                const size_t row = ((size_t)b * H + h) * W1 + w1;
                // rounded on its own: contracted into the pooling sum below, level 1 would not be the average of the
                // level-0 values that are stored
                float v0 = acc[n][r] * scale;
                STX_OPAQUE_VGPR(v0);
                const float v1 = (v0 + __shfl_xor(v0, 1)) * 0.5f;          // avg_pool of lanes (w2, w2 + 1), w2 even
                const float v2 = (v1 + __shfl_xor(v1, 2)) * 0.5f;          // ... of level-1 elements (w2/2, w2/2 + 1), w2 % 4 == 0
                const float v3 = (v2 + __shfl_xor(v2, 4)) * 0.5f;          // ... of level-2 elements, w2 % 8 == 0
                if (w1 < W1) {
                    if (w2 < W2) l0[row * W2 + w2] = v0;
                    if (levels > 1 && !(li & 1) && (w2 >> 1) < len1) l1[row * len1 + (w2 >> 1)] = v1;
                    if (levels > 2 && !(li & 3) && (w2 >> 2) < len2) l2[row * len2 + (w2 >> 2)] = v2;
                    if (levels > 3 && !(li & 7) && (w2 >> 3) < len3) l3[row * len3 + (w2 >> 3)] = v3;
                }
            }
        }
    }
}

// gradient of corr level 0 at (row, w2) with the pooled levels folded in
struct CorrGrad {
    const float *l0, *l1, *l2, *l3;
    int W2, len1, len2, len3;
    __device__ __forceinline__ float at(size_t row, int w2) const {
        float v = l0[row * W2 + w2];
        if (l1 && (w2 >> 1) < len1) v = fmaf(0.5f, l1[row * len1 + (w2 >> 1)], v);
        if (l2 && (w2 >> 2) < len2) v = fmaf(0.25f, l2[row * len2 + (w2 >> 2)], v);
        if (l3 && (w2 >> 3) < len3) v = fmaf(0.125f, l3[row * len3 + (w2 >> 3)], v);
        return v;
    }
};

// which = 0: g_fmap1[c][w1] = scale * sum_w2 G[w1][w2] fmap2[c][w2]   (grid.x over w1 tiles, the sum runs over w2)
// which = 1: g_fmap2[c][w2] = scale * sum_w1 G[w1][w2] fmap1[c][w1]   (grid.x over w2 tiles, the sum runs over w1)
// D[row = c][col = the output column]; the k index of step s of a 16-wide slab is 4 (l >> 4) + s for both operands.
__global__ __launch_bounds__(GC_THREADS) void corr_pyramid_bwd_kernel(const float* __restrict__ gcpyr, const float* __restrict__ fother,
                                                                      float* __restrict__ gf, int B, int C, int H, int W1, int W2,
                                                                      int levels, int which, float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int o0 = (int)blockIdx.x * 16, h = (int)blockIdx.y, b = (int)blockIdx.z;
    const int Wo = which ? W2 : W1, Wk = which ? W1 : W2;              // output columns, summed columns
    const size_t rows = (size_t)B * H * W1;
    CorrGrad G;
    G.W2 = W2; G.len1 = W2 >> 1; G.len2 = W2 >> 2; G.len3 = W2 >> 3;
    G.l0 = gcpyr;
    G.l1 = levels > 1 ? gcpyr + geo_level_offset((long long)rows, W2, 1, 1) : nullptr;
    G.l2 = levels > 2 ? gcpyr + geo_level_offset((long long)rows, W2, 1, 2) : nullptr;
    G.l3 = levels > 3 ? gcpyr + geo_level_offset((long long)rows, W2, 1, 3) : nullptr;
    const size_t HWk = (size_t)H * Wk, HWo = (size_t)H * Wo;
    const float* frow = fother + (size_t)b * C * HWk + (size_t)h * Wk;
    float* grow = gf + (size_t)b * C * HWo + (size_t)h * Wo;
    const size_t row0 = ((size_t)b * H + h) * W1;
    const int oc = o0 + li;                                             // this lane's output column (B operand)
    for (int c0 = wave * 16; c0 < C; c0 += 64) {
        f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        const int ca = c0 + li;                                         // this lane's channel (A operand)
        for (int k0 = 0; k0 < Wk; k0 += 16) {
            float av[4], bv[4];
            for (int sidx = 0; sidx < 4; ++sidx) {
                const int k = k0 + 4 * lk + sidx;
                const bool k_ok = k < Wk;
                av[sidx] = (k_ok && ca < C) ? frow[(size_t)ca * HWk + k] : 0.f;
                bv[sidx] = (k_ok && oc < Wo) ? (which ? G.at(row0 + k, oc) : G.at(row0 + oc, k)) : 0.f;
            }
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], acc1, 0, 0, 0);
        }
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + 4 * lk + r;
            if (c < C && oc < Wo) grow[(size_t)c * HWo + oc] = (acc0[r] + acc1[r]) * scale;
        }
    }
}

// ------------------------------------------------------------------------------------------------ lookup
struct Corr1dJobs {
    int n, channels;                  // jobs of the call; output channels = sum of (2 radius + 1)
    int level[CL_MAX_JOBS], radius[CL_MAX_JOBS], chan0[CL_MAX_JOBS];
    float alpha[CL_MAX_JOBS], mult[CL_MAX_JOBS];
};

struct Corr1dShape {
    int H, W1, W2, levels;
    long long npix;                   // B * H * W1
};

__device__ __forceinline__ float corr1d_position(const float* base, const float* disp, long long p, float alpha, float mult) {
    const float d = (disp && alpha != 0.f) ? disp[p] : 0.f;
    return (base[p] - alpha * d) * mult;
}

// grid (cdiv(npix, CL_THREADS), jobs)
__global__ __launch_bounds__(CL_THREADS) void corr1d_lookup_fwd_kernel(const float* __restrict__ cpyr, const float* __restrict__ base,
                                                                       const float* __restrict__ disp, float* __restrict__ out,
                                                                       Corr1dShape s, Corr1dJobs jobs) {
    const long long p = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (p >= s.npix) return;
    const int j = (int)blockIdx.y;
    const int lvl = jobs.level[j], radius = jobs.radius[j];
    const int K = 2 * radius + 1, len = s.W2 >> lvl;
    const size_t HW = (size_t)s.H * s.W1;
    const size_t b = (size_t)(p / (long long)HW), hw = (size_t)(p % (long long)HW);
    float f;
    const int x0 = geo_window(corr1d_position(base, disp, p, jobs.alpha[j], jobs.mult[j]), radius, f);
    const float* row = cpyr + geo_level_offset(s.npix, s.W2, 1, lvl) + (size_t)p * len;
    float* o = out + (b * (size_t)jobs.channels + (size_t)jobs.chan0[j]) * HW + hw;
    float prev = geo_tap1(row, x0, len);
    for (int k = 0; k < K; ++k) {
        const float cur = geo_tap1(row, x0 + k + 1, len);
        o[(size_t)k * HW] = geo_lerp(prev, cur, f);
        prev = cur;
    }
}

// grid (cdiv(npix, CL_THREADS), levels).  Gradient of a window: tap t (0 .. K) receives (1 - f) * g[k = t] + f * g[k = t - 1];
// ADDED to the owner's row.
__global__ __launch_bounds__(CL_THREADS) void corr1d_lookup_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ base,
                                                                       const float* __restrict__ disp, float* __restrict__ gcpyr,
                                                                       Corr1dShape s, Corr1dJobs jobs) {
    const long long p = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (p >= s.npix) return;
    const int lvl = (int)blockIdx.y;
    const int len = s.W2 >> lvl;
    const size_t HW = (size_t)s.H * s.W1;
    const size_t b = (size_t)(p / (long long)HW), hw = (size_t)(p % (long long)HW);
    float* row = gcpyr + geo_level_offset(s.npix, s.W2, 1, lvl) + (size_t)p * len;
    for (int j = 0; j < jobs.n; ++j) {
        if (jobs.level[j] != lvl) continue;
        const int radius = jobs.radius[j], K = 2 * radius + 1;
        float f;
        const int x0 = geo_window(corr1d_position(base, disp, p, jobs.alpha[j], jobs.mult[j]), radius, f);
        const float* g = gout + (b * (size_t)jobs.channels + (size_t)jobs.chan0[j]) * HW + hw;
        float carry = 0.f;                                              // f * g[k = t - 1]
        for (int t = 0; t <= K; ++t) {
            const float gk = t < K ? g[(size_t)t * HW] : 0.f;
            const int x = x0 + t;
            if (x >= 0 && x < len) row[x] += fmaf(1.f - f, gk, carry);
            carry = f * gk;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
int corr_shape_ok(int B, int C, int H, int W1, int W2, int levels, const char* what) {
    STX_REQUIRE(B > 0 && C > 0 && H > 0 && W1 > 0 && W2 > 0 && B < 65536 && H < 65536, "%s: bad shape B=%d C=%d H=%d W1=%d W2=%d", what, B,
                C, H, W1, W2);
    STX_REQUIRE(levels >= 1 && levels <= CP_MAX_LEVELS, "%s: num_levels %d outside 1..%d", what, levels, CP_MAX_LEVELS);
    // the reference's grid normalisation divides by (length - 1) of every level it samples
    STX_REQUIRE((W2 >> (levels - 1)) >= 2, "%s: W2=%d leaves level %d shorter than 2", what, W2, levels - 1);
    STX_REQUIRE((long long)B * H * W1 * (long long)W2 < (1ll << 40), "%s: tensor too large", what);
    return STX_OK;
}

// jobs: njobs x (level, radius, alpha, mult) floats in HOST memory
int corr1d_jobs(Corr1dJobs& t, const float* jobs, int njobs, int levels, const char* what) {
    STX_REQUIRE(jobs && njobs >= 1 && njobs <= CL_MAX_JOBS, "%s: %d lookup jobs outside 1..%d", what, njobs, CL_MAX_JOBS);
    t.n = njobs;
    t.channels = 0;
    for (int j = 0; j < CL_MAX_JOBS; ++j) {
        t.level[j] = 0; t.radius[j] = 0; t.chan0[j] = 0; t.alpha[j] = 0.f; t.mult[j] = 0.f;
    }
    for (int j = 0; j < njobs; ++j) {
        const float lv = jobs[4 * j], r = jobs[4 * j + 1];
        STX_REQUIRE(lv >= 0.f && lv < (float)levels && lv == (float)(int)lv, "%s: job %d reads level %g of %d", what, j, (double)lv, levels);
        STX_REQUIRE(r >= 1.f && r <= (float)CL_MAX_RADIUS && r == (float)(int)r, "%s: job %d: radius %g outside 1..%d", what, j, (double)r,
                    CL_MAX_RADIUS);
        t.level[j] = (int)lv;
        t.radius[j] = (int)r;
        t.alpha[j] = jobs[4 * j + 2];
        t.mult[j] = jobs[4 * j + 3];
        t.chan0[j] = t.channels;
        t.channels += 2 * t.radius[j] + 1;
    }
    return STX_OK;
}

int corr1d_lookup_shape(Corr1dShape& s, int B, int H, int W1, int W2, int levels, const char* what) {
    if (int rc = corr_shape_ok(B, 1, H, W1, W2, levels, what)) return rc;
    s.H = H; s.W1 = W1; s.W2 = W2; s.levels = levels;
    s.npix = (long long)B * H * W1;
    STX_REQUIRE(s.npix / CL_THREADS < (1ll << 31) - 1, "%s: too many pixels", what);
    return STX_OK;
}

}  // namespace

int corr_pyramid_fwd_launch(const float* fmap1, const float* fmap2, float* cpyr, int B, int C, int H, int W1, int W2, int levels,
                            float scale, void* stream, const char* what) {
    hipLaunchKernelGGL(corr_pyramid_fwd_kernel, dim3(stx_cdiv(W1, 16), H, B), dim3(GC_THREADS), 0, (hipStream_t)stream, fmap1, fmap2, cpyr,
                       B, C, H, W1, W2, levels, scale);
    return stx_check_launch(what);
}

int corr_pyramid_bwd_launch(const float* gcpyr, const float* fmap1, const float* fmap2, float* gfmap1, float* gfmap2, int B, int C,
                            int H, int W1, int W2, int levels, float scale, void* stream, const char* what) {
    if (gfmap1) {
        hipLaunchKernelGGL(corr_pyramid_bwd_kernel, dim3(stx_cdiv(W1, 16), H, B), dim3(GC_THREADS), 0, (hipStream_t)stream, gcpyr, fmap2,
                           gfmap1, B, C, H, W1, W2, levels, 0, scale);
        if (int rc = stx_check_launch(what)) return rc;
    }
    if (gfmap2) {
        hipLaunchKernelGGL(corr_pyramid_bwd_kernel, dim3(stx_cdiv(W2, 16), H, B), dim3(GC_THREADS), 0, (hipStream_t)stream, gcpyr, fmap1,
                           gfmap2, B, C, H, W1, W2, levels, 1, scale);
        if (int rc = stx_check_launch(what)) return rc;
    }
    return STX_OK;
}

extern "C" long long stx_corr1d_pyramid_floats(long long rows, int W2, int levels) {
    if (rows <= 0 || W2 <= 0 || levels < 1 || levels > CP_MAX_LEVELS) return 0;
    return (long long)geo_level_offset(rows, W2, 1, levels);
}

extern "C" int stx_corr1d_pyramid_fwd(const float* fmap1, const float* fmap2, float* cpyr, int B, int C, int H, int W1, int W2,
                                      int levels, float scale, void* stream) {
    stx_begin();
    STX_REQUIRE(fmap1 && fmap2 && cpyr, "corr1d_pyramid_fwd: null pointer");
    if (int rc = corr_shape_ok(B, C, H, W1, W2, levels, "corr1d_pyramid_fwd")) return rc;
    return corr_pyramid_fwd_launch(fmap1, fmap2, cpyr, B, C, H, W1, W2, levels, scale, stream, "corr1d_pyramid_fwd");
}

extern "C" int stx_corr1d_pyramid_bwd(const float* gcpyr, const float* fmap1, const float* fmap2, float* gfmap1, float* gfmap2, int B,
                                      int C, int H, int W1, int W2, int levels, float scale, void* stream) {
    stx_begin();
    STX_REQUIRE(gcpyr && fmap1 && fmap2 && (gfmap1 || gfmap2), "corr1d_pyramid_bwd: null pointer");
    if (int rc = corr_shape_ok(B, C, H, W1, W2, levels, "corr1d_pyramid_bwd")) return rc;
    return corr_pyramid_bwd_launch(gcpyr, fmap1, fmap2, gfmap1, gfmap2, B, C, H, W1, W2, levels, scale, stream, "corr1d_pyramid_bwd");
}

extern "C" int stx_corr1d_lookup_fwd(const float* cpyr, const float* base, const float* disp, const float* jobs, int njobs, float* out,
                                     int B, int H, int W1, int W2, int levels, void* stream) {
    stx_begin();
    STX_REQUIRE(cpyr && base && out, "corr1d_lookup_fwd: null pointer");
    Corr1dShape s;
    Corr1dJobs t;
    if (int rc = corr1d_lookup_shape(s, B, H, W1, W2, levels, "corr1d_lookup_fwd")) return rc;
    if (int rc = corr1d_jobs(t, jobs, njobs, levels, "corr1d_lookup_fwd")) return rc;
    hipLaunchKernelGGL(corr1d_lookup_fwd_kernel, dim3((unsigned)((s.npix + CL_THREADS - 1) / CL_THREADS), t.n), dim3(CL_THREADS), 0,
                       (hipStream_t)stream, cpyr, base, disp, out, s, t);
    return stx_check_launch("corr1d_lookup_fwd");
}

extern "C" int stx_corr1d_lookup_bwd(const float* gout, const float* base, const float* disp, const float* jobs, int njobs,
                                     float* gcpyr, int B, int H, int W1, int W2, int levels, void* stream) {
    stx_begin();
    STX_REQUIRE(gout && base && gcpyr, "corr1d_lookup_bwd: null pointer");
    Corr1dShape s;
    Corr1dJobs t;
    if (int rc = corr1d_lookup_shape(s, B, H, W1, W2, levels, "corr1d_lookup_bwd")) return rc;
    if (int rc = corr1d_jobs(t, jobs, njobs, levels, "corr1d_lookup_bwd")) return rc;
    hipLaunchKernelGGL(corr1d_lookup_bwd_kernel, dim3((unsigned)((s.npix + CL_THREADS - 1) / CL_THREADS), levels), dim3(CL_THREADS), 0,
                       (hipStream_t)stream, gout, base, disp, gcpyr, s, t);
    return stx_check_launch("corr1d_lookup_bwd");
}

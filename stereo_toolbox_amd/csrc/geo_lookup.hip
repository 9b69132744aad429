// Combined geometry-encoding lookup and convex upsampling of the IGEV family (reference models/IGEVStereo/geometry.py:7-70,
// models/IGEVStereo/submodule.py:243-255; the same two pieces serve MonSter, Selective-IGEV and FoundationStereo): the part of
// those models that runs once per GRU iteration (22 in training, 32 in validation, igev_stereo.py:101-102).
//
//   corr[b,h,w1,w2] = sum_c fmap1[b,c,h,w1] * fmap2[b,c,h,w2]                                   geometry.py:62-70
//   level i+1 = avg_pool2d(level i, [1,2], [1,2]) along the last axis (floor: an odd tail is dropped)     :24-30
//   lookup: per pixel p, level i, k in [-r, r]:  geo level at x = disp[p] / 2^i + k (all C channels),
//           that pixel's correlation row at x = (coords[p] - disp[p]) / 2^i + k; linear interpolation between floor(x) and
//           floor(x) + 1, taps outside [0, len_i - 1] are zero (grid_sample, align_corners=True, zero padding)      :35-59
//   context_upsample: out[4y+j][4x+i] = sum_{t<9} w[t][4y+j][4x+i] * disp[y + t/3 - 1][x + t%3 - 1]     submodule.py:243-255
//
// Layout.  Both pyramids are PIXEL-MAJOR, the levels one behind the other in one buffer:
//   geometry level i   [B*H*W][D >> i][C]      (one pixel's search window = 2r+2 taps x C floats = ONE contiguous run:
//                                               10 x 32 B at radius 4, C = 8)
//   correlation level i [B*H*W1][W2 >> i]
// so the lookup of a pixel touches nothing but that pixel's own rows, forward and backward: the backward pass adds into the
// rows its pixel owns with plain loads and stores -- no atomics, bitwise reproducible -- and because it ADDS, the 22-32
// lookups of one training step accumulate into one gradient buffer per pyramid (ops.py GeoLookupFn).
//
// Kernels.
//   geo_corr_fwd      (the kernels of corr1d.hip at scale 1, corr_pyramid.h)
//                     one GEMM W1 x C x W2 per image row on v_mfma_f32_16x16x4_f32 (operands straight from the NCHW rows, one
//                     dword per lane, 64-byte segments); the pooled levels come out of the accumulators (neighbouring lanes
//                     hold neighbouring w2) in the same launch.
//   geo_corr_bwd      g_fmap1 = G . fmap2, g_fmap2 = G^T . fmap1 on the same instruction, G = the gradient of level 0 plus
//                     the pooled levels' gradients (0.5 / 0.25 of the parent element), formed while the operand is loaded.
//   geo_pyramid_fwd   dense [B][D][H][W][C] volume -> every level, one launch: a (16-pixel x D x C) tile is read in memory
//                     order, turned in LDS, and written in runs of D_i * C floats per pixel.  _bwd: the inverse.
//   geo_lookup_fwd    one lane per pixel and job (a job = one channel quad of one level, or one level's correlation row):
//                     the stores of a wave are 256-byte runs along w of the NCHW output, the loads 16-byte pieces of the
//                     lane's own window.  A gather with 32-byte granules out of two pyramids (about 130 MB at 576x960) that
//                     fit the Infinity Cache.
//   geo_lookup_bwd    the same decomposition; every tap of the window is one read-modify-write of the owner's row.
//   context_upsample  one lane per four output pixels (they share the low-resolution cell): 9 x float4 of weights, 9 taps.
//                     Backward: the weights' gradient in the same shape; the disparity's gradient as a GATHER over the 9 x 16
//                     output pixels a low-resolution pixel feeds (fixed order, no atomics).
#include "corr_pyramid.h"

namespace {

constexpr int GL_THREADS = 128;       // lookup kernels: lanes (pixels) per workgroup
constexpr int GL_MAX_LEVELS = 3;
constexpr int GL_MAX_RADIUS = 8;
constexpr int GP_THREADS = 256;       // pyramid build
constexpr size_t GP_LDS_BYTES = STX_LDS_DEFAULT;   // (no grant needed)
constexpr int CU_THREADS = 256;

struct GeoShape {
    int B, H, W, D, C, W2, levels, radius;
    long long npix;                   // B * H * W
};

// ------------------------------------------------------------------------------------------------ pyramid addressing
// (geo_level_offset, geo_window, geo_tap1, geo_lerp: corr_pyramid.h)
__device__ __forceinline__ float4 geo_tap4(const float* row, int t, int len, int C) {
    if (t < 0 || t >= len) return make_float4(0.f, 0.f, 0.f, 0.f);
    return stx_ld4(row + (size_t)t * C);
}

// ------------------------------------------------------------------------------------------------ lookup
// grid: (cdiv(npix, GL_THREADS), levels * (C/4 + 1)); blockIdx.y = level * (C/4 + 1) + job, job < C/4: channel quad, else correlation
__global__ __launch_bounds__(GL_THREADS) void geo_lookup_fwd_kernel(const float* __restrict__ gpyr, const float* __restrict__ cpyr,
                                                                    const float* __restrict__ disp, const float* __restrict__ coords,
                                                                    float* __restrict__ out, GeoShape s) {
    const long long p = (long long)blockIdx.x * GL_THREADS + threadIdx.x;
    if (p >= s.npix) return;
    const int Q = s.C >> 2;
    const int lvl = (int)blockIdx.y / (Q + 1), job = (int)blockIdx.y % (Q + 1);
    const int K = 2 * s.radius + 1;
    const size_t HW = (size_t)s.H * s.W;
    const size_t b = (size_t)(p / (long long)HW), hw = (size_t)(p % (long long)HW);
    const float scale = 1.f / (float)(1 << lvl);
    float* o = out + (b * (size_t)(s.levels * (s.C + 1) * K) + (size_t)lvl * (s.C + 1) * K) * HW + hw;
    const float d = disp[p];
    float f;
    if (job < Q) {
        const int len = s.D >> lvl;
        const int x0 = geo_window(d * scale, s.radius, f);
        const float* row = gpyr + geo_level_offset(s.npix, s.D, s.C, lvl) + (size_t)p * len * s.C + 4 * job;
        float* oq = o + (size_t)(4 * job) * K * HW;
        float4 prev = geo_tap4(row, x0, len, s.C);
        for (int k = 0; k < K; ++k) {
            const float4 cur = geo_tap4(row, x0 + k + 1, len, s.C);
            oq[(size_t)(0 * K + k) * HW] = geo_lerp(prev.x, cur.x, f);
            oq[(size_t)(1 * K + k) * HW] = geo_lerp(prev.y, cur.y, f);
            oq[(size_t)(2 * K + k) * HW] = geo_lerp(prev.z, cur.z, f);
            oq[(size_t)(3 * K + k) * HW] = geo_lerp(prev.w, cur.w, f);
            prev = cur;
        }
    } else {
        const int len = s.W2 >> lvl;
        const int x0 = geo_window(coords[p] * scale - d * scale, s.radius, f);
        const float* row = cpyr + geo_level_offset(s.npix, s.W2, 1, lvl) + (size_t)p * len;
        float* oc = o + (size_t)s.C * K * HW;
        float prev = geo_tap1(row, x0, len);
        for (int k = 0; k < K; ++k) {
            const float cur = geo_tap1(row, x0 + k + 1, len);
            oc[(size_t)k * HW] = geo_lerp(prev, cur, f);
            prev = cur;
        }
    }
}

// gradient of the window: tap j (0 .. K) receives (1 - f) * g[k = j] + f * g[k = j - 1]; ADDED to the owner's row
__global__ __launch_bounds__(GL_THREADS) void geo_lookup_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ disp,
                                                                    const float* __restrict__ coords, float* __restrict__ ggpyr,
                                                                    float* __restrict__ gcpyr, GeoShape s) {
    const long long p = (long long)blockIdx.x * GL_THREADS + threadIdx.x;
    if (p >= s.npix) return;
    const int Q = s.C >> 2;
    const int lvl = (int)blockIdx.y / (Q + 1), job = (int)blockIdx.y % (Q + 1);
    const int K = 2 * s.radius + 1;
    const size_t HW = (size_t)s.H * s.W;
    const size_t b = (size_t)(p / (long long)HW), hw = (size_t)(p % (long long)HW);
    const float scale = 1.f / (float)(1 << lvl);
    const float* g = gout + (b * (size_t)(s.levels * (s.C + 1) * K) + (size_t)lvl * (s.C + 1) * K) * HW + hw;
    const float d = disp[p];
    float f;
    if (job < Q) {
        if (ggpyr == nullptr) return;
        const int len = s.D >> lvl;
        const int x0 = geo_window(d * scale, s.radius, f);
        float* row = ggpyr + geo_level_offset(s.npix, s.D, s.C, lvl) + (size_t)p * len * s.C + 4 * job;
        const float* gq = g + (size_t)(4 * job) * K * HW;
        float4 carry = make_float4(0.f, 0.f, 0.f, 0.f);                 // f * g[k = j - 1]
        for (int j = 0; j <= K; ++j) {
            float4 gk = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < K)
                gk = make_float4(gq[(size_t)(0 * K + j) * HW], gq[(size_t)(1 * K + j) * HW], gq[(size_t)(2 * K + j) * HW],
                                 gq[(size_t)(3 * K + j) * HW]);
            const int t = x0 + j;
            if (t >= 0 && t < len) {
                float* q = row + (size_t)t * s.C;
                float4 v = stx_ld4(q);
                v.x += fmaf(1.f - f, gk.x, carry.x);
                v.y += fmaf(1.f - f, gk.y, carry.y);
                v.z += fmaf(1.f - f, gk.z, carry.z);
                v.w += fmaf(1.f - f, gk.w, carry.w);
                stx_st4(q, v);
            }
            carry = make_float4(f * gk.x, f * gk.y, f * gk.z, f * gk.w);
        }
    } else {
        if (gcpyr == nullptr) return;
        const int len = s.W2 >> lvl;
        const int x0 = geo_window(coords[p] * scale - d * scale, s.radius, f);
        float* row = gcpyr + geo_level_offset(s.npix, s.W2, 1, lvl) + (size_t)p * len;
        const float* gc = g + (size_t)s.C * K * HW;
        float carry = 0.f;
        for (int j = 0; j <= K; ++j) {
            const float gk = j < K ? gc[(size_t)j * HW] : 0.f;
            const int t = x0 + j;
            if (t >= 0 && t < len) row[t] += fmaf(1.f - f, gk, carry);
            carry = f * gk;
        }
    }
}

// ------------------------------------------------------------------------------------------------ geometry pyramid
// grid (cdiv(W, WT), H, B).  LDS image [D][WT * C + C] (the pad spreads a wave's (d, c) reads over all banks).
__global__ __launch_bounds__(GP_THREADS) void geo_pyramid_kernel(const float* __restrict__ vol_in, float* __restrict__ vol_out,
                                                                 const float* __restrict__ pyr_in, float* __restrict__ pyr_out,
                                                                 GeoShape s, int WT) {
    STX_DYN_SMEM(smem);
    float* img = reinterpret_cast<float*>(smem);
    const int C = s.C, D = s.D, rowf = WT * C, ldr = rowf + C;
    const int w0 = (int)blockIdx.x * WT, h = (int)blockIdx.y, b = (int)blockIdx.z;
    const int npx = s.W - w0 < WT ? s.W - w0 : WT;
    const size_t pix0 = ((size_t)b * s.H + h) * s.W + w0;
    if (vol_in) {                                                       // forward: volume -> levels
        for (int i = threadIdx.x; i < D * rowf; i += GP_THREADS) {
            const int d = i / rowf, r = i - d * rowf;
            if (r < npx * C) img[d * ldr + r] = vol_in[(((size_t)b * D + d) * s.H + h) * s.W * C + (size_t)w0 * C + r];
        }
        __syncthreads();
        for (int lvl = 0; lvl < s.levels; ++lvl) {
            const int len = D >> lvl, run = len * C;
            float* dst = pyr_out + geo_level_offset(s.npix, D, C, lvl) + pix0 * run;
            for (int i = threadIdx.x; i < npx * run; i += GP_THREADS) {
                const int px = i / run, r = i - px * run, dd = r / C, c = r - dd * C;
                const float* q = img + px * C + c;
                float v;
                if (lvl == 0) {
                    v = q[dd * ldr];
                } else if (lvl == 1) {
                    v = (q[(2 * dd) * ldr] + q[(2 * dd + 1) * ldr]) * 0.5f;
                } else {
                    const float a0 = (q[(4 * dd) * ldr] + q[(4 * dd + 1) * ldr]) * 0.5f;
                    const float a1 = (q[(4 * dd + 2) * ldr] + q[(4 * dd + 3) * ldr]) * 0.5f;
                    v = (a0 + a1) * 0.5f;
                }
                dst[i] = v;
            }
        }
    } else {                                                            // backward: level gradients -> volume gradient
        const int len1 = D >> 1, len2 = D >> 2;
        const float* l0 = pyr_in + pix0 * ((size_t)D * C);
        const float* l1 = s.levels > 1 ? pyr_in + geo_level_offset(s.npix, D, C, 1) + pix0 * ((size_t)len1 * C) : nullptr;
        const float* l2 = s.levels > 2 ? pyr_in + geo_level_offset(s.npix, D, C, 2) + pix0 * ((size_t)len2 * C) : nullptr;
        const int run = D * C;
        for (int i = threadIdx.x; i < npx * run; i += GP_THREADS) {
            const int px = i / run, r = i - px * run, d = r / C, c = r - d * C;
            float v = l0[i];
            if (l1 && (d >> 1) < len1) v = fmaf(0.5f, l1[(size_t)px * len1 * C + (d >> 1) * C + c], v);
            if (l2 && (d >> 2) < len2) v = fmaf(0.25f, l2[(size_t)px * len2 * C + (d >> 2) * C + c], v);
            img[d * ldr + px * C + c] = v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < D * rowf; i += GP_THREADS) {
            const int d = i / rowf, r = i - d * rowf;
            if (r < npx * C) vol_out[(((size_t)b * D + d) * s.H + h) * s.W * C + (size_t)w0 * C + r] = img[d * ldr + r];
        }
    }
}

// ------------------------------------------------------------------------------------------------ context_upsample
// one lane per (b, Y, x): the four output pixels X = 4x .. 4x + 3 of row Y share the low-resolution cell (Y / 4, x)
__global__ __launch_bounds__(CU_THREADS) void context_upsample_kernel(const float* __restrict__ disp, const float* __restrict__ wts,
                                                                      const float* __restrict__ g, float* __restrict__ out,
                                                                      float* __restrict__ gw, int B, int h, int w) {
    const long long idx = (long long)blockIdx.x * CU_THREADS + threadIdx.x;
    const int H4 = 4 * h;
    if (idx >= (long long)B * H4 * w) return;
    const int x = (int)(idx % w), Y = (int)((idx / w) % H4), b = (int)(idx / ((long long)w * H4));
    const int y = Y >> 2;
    const size_t plane = (size_t)H4 * 4 * w, pos = (size_t)Y * 4 * w + 4 * (size_t)x;
    const float* dl = disp + (size_t)b * h * w;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g) gv = stx_ld4(g + (size_t)b * plane + pos);
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const float dv = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? dl[(size_t)yy * w + xx] : 0.f;
        const size_t o = ((size_t)b * 9 + t) * plane + pos;
        if (g) {
            stx_st4(gw + o, make_float4(gv.x * dv, gv.y * dv, gv.z * dv, gv.w * dv));
        } else {
            const float4 wv = stx_ld4(wts + o);
            acc.x = fmaf(wv.x, dv, acc.x);
            acc.y = fmaf(wv.y, dv, acc.y);
            acc.z = fmaf(wv.z, dv, acc.z);
            acc.w = fmaf(wv.w, dv, acc.w);
        }
    }
    if (!g) stx_st4(out + (size_t)b * plane + pos, acc);
}

// g_disp[y][x] = sum over the cells (y - dy, x - dx) that read this pixel as tap t = 3 (dy + 1) + (dx + 1), over their 16 outputs
__global__ __launch_bounds__(CU_THREADS) void context_upsample_bwd_disp_kernel(const float* __restrict__ g, const float* __restrict__ wts,
                                                                               float* __restrict__ gdisp, int B, int h, int w) {
    const long long idx = (long long)blockIdx.x * CU_THREADS + threadIdx.x;
    if (idx >= (long long)B * h * w) return;
    const int x = (int)(idx % w), y = (int)((idx / w) % h), b = (int)(idx / ((long long)w * h));
    const size_t plane = (size_t)16 * h * w;
    float acc = 0.f;                                                    // summed as a tree (4 -> 16 -> 144 terms): shorter rounding chains
    for (int t = 0; t < 9; ++t) {
        const int cy = y - (t / 3 - 1), cx = x - (t % 3 - 1);
        if (cy < 0 || cy >= h || cx < 0 || cx >= w) continue;
        float cell = 0.f;
        for (int j = 0; j < 4; ++j) {
            const size_t pos = (size_t)(4 * cy + j) * 4 * w + 4 * (size_t)cx;
            const float4 wv = stx_ld4(wts + ((size_t)b * 9 + t) * plane + pos);
            const float4 gv = stx_ld4(g + (size_t)b * plane + pos);
            cell += fmaf(wv.w, gv.w, fmaf(wv.z, gv.z, fmaf(wv.y, gv.y, wv.x * gv.x)));
        }
        acc += cell;
    }
    gdisp[idx] = acc;
}

// ------------------------------------------------------------------------------------------------ host side
int geo_shape(GeoShape& s, int B, int H, int W, int D, int C, int W2, int levels, int radius, const char* what) {
    STX_REQUIRE(B > 0 && H > 0 && W > 0 && D > 0 && C > 0 && W2 > 0, "%s: bad shape B=%d H=%d W=%d D=%d C=%d W2=%d", what, B, H, W, D,
                C, W2);
    STX_REQUIRE(levels >= 1 && levels <= GL_MAX_LEVELS, "%s: num_levels %d outside 1..%d", what, levels, GL_MAX_LEVELS);
    STX_REQUIRE(radius >= 1 && radius <= GL_MAX_RADIUS, "%s: radius %d outside 1..%d", what, radius, GL_MAX_RADIUS);
    STX_REQUIRE(C % 4 == 0, "%s: geometry channels C (%d) must be a multiple of 4", what, C);
    STX_REQUIRE((D >> (levels - 1)) >= 1 && (W2 >> (levels - 1)) >= 1, "%s: D=%d / W2=%d too short for %d levels", what, D, W2, levels);
    STX_REQUIRE(H < 65536 && B < 65536, "%s: H / B exceed the launch grid", what);
    STX_REQUIRE((long long)B * H * W * (long long)(D > W2 ? D : W2) * C < (1ll << 40), "%s: tensor too large", what);
    s.B = B; s.H = H; s.W = W; s.D = D; s.C = C; s.W2 = W2; s.levels = levels; s.radius = radius;
    s.npix = (long long)B * H * W;
    STX_REQUIRE(s.npix / GL_THREADS < (1ll << 31) - 1, "%s: too many pixels", what);
    return STX_OK;
}

int geo_pyramid_launch(const float* vol_in, float* vol_out, const float* pyr_in, float* pyr_out, int B, int D, int H, int W, int C,
                       int levels, void* stream, const char* what) {
    GeoShape s;
    if (int rc = geo_shape(s, B, H, W, D, C, 1 << (GL_MAX_LEVELS - 1), levels, 1, what)) return rc;
    int WT = 16;
    while (WT > 1 && (size_t)D * (WT * C + C) * sizeof(float) > GP_LDS_BYTES) WT >>= 1;
    const size_t lds = (size_t)D * (WT * C + C) * sizeof(float);
    STX_REQUIRE(lds <= GP_LDS_BYTES, "%s: D * C = %d does not fit the LDS tile", what, D * C);
    hipLaunchKernelGGL(geo_pyramid_kernel, dim3(stx_cdiv(W, WT), H, B), dim3(GP_THREADS), lds, (hipStream_t)stream, vol_in, vol_out,
                       pyr_in, pyr_out, s, WT);
    return stx_check_launch(what);
}

}  // namespace

extern "C" long long stx_geo_pyramid_floats(long long rows, int len, int C, int levels) {
    if (rows <= 0 || len <= 0 || C <= 0 || levels < 1 || levels > GL_MAX_LEVELS) return 0;
    return (long long)geo_level_offset(rows, len, C, levels);
}

extern "C" int stx_geo_corr_fwd(const float* fmap1, const float* fmap2, float* cpyr, int B, int C, int H, int W1, int W2, int levels,
                                void* stream) {
    stx_begin();
    STX_REQUIRE(fmap1 && fmap2 && cpyr, "geo_corr_fwd: null pointer");
    STX_REQUIRE(B > 0 && C > 0 && H > 0 && W1 > 0 && W2 > 0 && B < 65536 && H < 65536, "geo_corr_fwd: bad shape B=%d C=%d H=%d W1=%d W2=%d",
                B, C, H, W1, W2);
    STX_REQUIRE(levels >= 1 && levels <= GL_MAX_LEVELS && (W2 >> (levels - 1)) >= 1, "geo_corr_fwd: %d levels on W2=%d", levels, W2);
    return corr_pyramid_fwd_launch(fmap1, fmap2, cpyr, B, C, H, W1, W2, levels, 1.0f, stream, "geo_corr_fwd");
}

extern "C" int stx_geo_corr_bwd(const float* gcpyr, const float* fmap1, const float* fmap2, float* gfmap1, float* gfmap2, int B, int C,
                                int H, int W1, int W2, int levels, void* stream) {
    stx_begin();
    STX_REQUIRE(gcpyr && fmap1 && fmap2, "geo_corr_bwd: null pointer");
    STX_REQUIRE(B > 0 && C > 0 && H > 0 && W1 > 0 && W2 > 0 && B < 65536 && H < 65536, "geo_corr_bwd: bad shape B=%d C=%d H=%d W1=%d W2=%d",
                B, C, H, W1, W2);
    STX_REQUIRE(levels >= 1 && levels <= GL_MAX_LEVELS && (W2 >> (levels - 1)) >= 1, "geo_corr_bwd: %d levels on W2=%d", levels, W2);
    return corr_pyramid_bwd_launch(gcpyr, fmap1, fmap2, gfmap1, gfmap2, B, C, H, W1, W2, levels, 1.0f, stream, "geo_corr_bwd");
}

extern "C" int stx_geo_pyramid_fwd(const float* vol, float* gpyr, int B, int D, int H, int W, int C, int levels, void* stream) {
    stx_begin();
    STX_REQUIRE(vol && gpyr, "geo_pyramid_fwd: null pointer");
    return geo_pyramid_launch(vol, nullptr, nullptr, gpyr, B, D, H, W, C, levels, stream, "geo_pyramid_fwd");
}

extern "C" int stx_geo_pyramid_bwd(const float* ggpyr, float* gvol, int B, int D, int H, int W, int C, int levels, void* stream) {
    stx_begin();
    STX_REQUIRE(ggpyr && gvol, "geo_pyramid_bwd: null pointer");
    return geo_pyramid_launch(nullptr, gvol, ggpyr, nullptr, B, D, H, W, C, levels, stream, "geo_pyramid_bwd");
}

extern "C" int stx_geo_lookup_fwd(const float* gpyr, const float* cpyr, const float* disp, const float* coords, float* out, int B,
                                  int H, int W, int D, int C, int W2, int levels, int radius, void* stream) {
    stx_begin();
    STX_REQUIRE(gpyr && cpyr && disp && coords && out, "geo_lookup_fwd: null pointer");
    GeoShape s;
    if (int rc = geo_shape(s, B, H, W, D, C, W2, levels, radius, "geo_lookup_fwd")) return rc;
    hipLaunchKernelGGL(geo_lookup_fwd_kernel, dim3((unsigned)((s.npix + GL_THREADS - 1) / GL_THREADS), levels * (C / 4 + 1)),
                       dim3(GL_THREADS), 0, (hipStream_t)stream, gpyr, cpyr, disp, coords, out, s);
    return stx_check_launch("geo_lookup_fwd");
}

extern "C" int stx_geo_lookup_bwd(const float* gout, const float* disp, const float* coords, float* ggpyr, float* gcpyr, int B, int H,
                                  int W, int D, int C, int W2, int levels, int radius, void* stream) {
    stx_begin();
    STX_REQUIRE(gout && disp && coords && (ggpyr || gcpyr), "geo_lookup_bwd: null pointer");
    GeoShape s;
    if (int rc = geo_shape(s, B, H, W, D, C, W2, levels, radius, "geo_lookup_bwd")) return rc;
    hipLaunchKernelGGL(geo_lookup_bwd_kernel, dim3((unsigned)((s.npix + GL_THREADS - 1) / GL_THREADS), levels * (C / 4 + 1)),
                       dim3(GL_THREADS), 0, (hipStream_t)stream, gout, disp, coords, ggpyr, gcpyr, s);
    return stx_check_launch("geo_lookup_bwd");
}

extern "C" int stx_context_upsample_fwd(const float* disp_low, const float* up_weights, float* out, int B, int h, int w, void* stream) {
    stx_begin();
    STX_REQUIRE(disp_low && up_weights && out && B > 0 && h > 0 && w > 0, "context_upsample_fwd: bad arguments B=%d h=%d w=%d", B, h, w);
    const long long n = (long long)B * 4 * h * w;
    STX_REQUIRE(n * 36 < (1ll << 40) && (n + CU_THREADS - 1) / CU_THREADS < (1ll << 31), "context_upsample_fwd: tensor too large");
    hipLaunchKernelGGL(context_upsample_kernel, dim3((unsigned)((n + CU_THREADS - 1) / CU_THREADS)), dim3(CU_THREADS), 0,
                       (hipStream_t)stream, disp_low, up_weights, (const float*)nullptr, out, (float*)nullptr, B, h, w);
    return stx_check_launch("context_upsample_fwd");
}

extern "C" int stx_context_upsample_bwd(const float* g, const float* disp_low, const float* up_weights, float* gdisp, float* gweights,
                                        int B, int h, int w, void* stream) {
    stx_begin();
    STX_REQUIRE(g && B > 0 && h > 0 && w > 0 && (gdisp || gweights), "context_upsample_bwd: bad arguments B=%d h=%d w=%d", B, h, w);
    STX_REQUIRE((!gweights || disp_low) && (!gdisp || up_weights), "context_upsample_bwd: a saved forward operand is missing");
    const long long n = (long long)B * 4 * h * w;
    STX_REQUIRE(n * 36 < (1ll << 40) && (n + CU_THREADS - 1) / CU_THREADS < (1ll << 31), "context_upsample_bwd: tensor too large");
    if (gweights) {
        hipLaunchKernelGGL(context_upsample_kernel, dim3((unsigned)((n + CU_THREADS - 1) / CU_THREADS)), dim3(CU_THREADS), 0,
                           (hipStream_t)stream, disp_low, (const float*)nullptr, g, (float*)nullptr, gweights, B, h, w);
        if (int rc = stx_check_launch("context_upsample_bwd (weights)")) return rc;
    }
    if (gdisp) {
        const long long m = (long long)B * h * w;
        hipLaunchKernelGGL(context_upsample_bwd_disp_kernel, dim3((unsigned)((m + CU_THREADS - 1) / CU_THREADS)), dim3(CU_THREADS), 0,
                           (hipStream_t)stream, g, up_weights, gdisp, B, h, w);
        if (int rc = stx_check_launch("context_upsample_bwd (disp)")) return rc;
    }
    return STX_OK;
}

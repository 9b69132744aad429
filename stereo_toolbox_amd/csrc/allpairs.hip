// StereoAnywhere's volume stage on a row-wise all-pairs volume vol[B][H][W1][W2] (reference models/StereoAnywhere):
//   * disparity and confidence regressed from the volume in BOTH directions (utils/utils.py:112-170; the model calls the set
//     two to three times per forward, stereoanywhere.py:285-331):
//       p_l = softmax over w2,  disp_l[b,h,w1] = w1 - sum_w2 p_l w2,  conf_l = 1 + sum_w2 p_l log2(p_l + 1e-6) / log2(W2)
//       p_r = softmax over w1,  disp_r[b,h,w2] = sum_w1 p_r w1 - w2,  conf_r = 1 + sum_w1 p_r log2(p_r + 1e-6) / log2(W1)
//     Stock that is four volume-sized softmaxes and about a dozen volume-sized temporaries; here the volume is read once per
//     direction from HBM (the further passes of the column direction re-read a workgroup's own 64-column strip from L2).
//   * the correlation block that takes a VOLUME (corr.py:75-132): the pixel-major pyramid of corr1d.hip with level 0 = the
//     volume -- optionally times the truncation factor of truncate_corr_volume_v2 (utils/utils.py:216-238), formed on the fly
//     -- so stx_corr1d_lookup_fwd / _bwd serve the lookups unchanged; and the mask volume itself for callers that want it.
//
// Kernels.
//   allpairs_rows   one WAVE per volume row (b, h, w1), four rows per workgroup: the row (W2 <= 512) lives in eight registers
//                   per lane, so max, sum and the weighted sums are wave reductions over ONE read.  B*H*W1 / 4 workgroups.
//   allpairs_cols   one workgroup per image row (b, h) and 64-column strip, lanes along w2 (256-byte coalesced rows), the four
//                   waves interleaved down w1; the waves' partial results are combined in LDS in wave order.  Pass 1 the max,
//                   pass 2 sum and first moment (disp_r needs no more), pass 3 -- only for the confidence or the backward's
//                   statistics, which need the NORMALISED p because of the + 1e-6 -- the entropy sums.
//   allpairs_bwd    one wave per row again: gvol = row-direction softmax Jacobian term + column-direction term from the saved
//                   statistics, every element written once, no atomics.
//   Sums are accumulated in double (the exponentials are fp32): what is left is the error of expf / log2f on each term.
//   volume_pyramid_fwd / _bwd, truncate_mask   one wave per row, the pooled levels from neighbouring lanes as in corr1d.hip.
//
// Statistics (`stats`, 4 * (B*H*W1 + B*H*W2) floats): per row, then per column (b, h, w2), the four floats
//   max, sum_k exp(v_k - max), E = sum_k p_k k, F = sum_k p_k f'(p_k)   with f(p) = p log2(p + 1e-6),
// which make the backward one pass:  d disp_l / d v_j = -p_j (j - E),  d sum_k f(p_k) / d v_j = p_j (f'(p_j) - F).
#include "corr_pyramid.h"

namespace {

constexpr int AP_THREADS = 256;       // four waves
constexpr int AP_WAVES = AP_THREADS / 64;
constexpr int AP_MAX_W = 512;         // estimators: a row of W2 floats in AP_MAX_W / 64 registers per lane
constexpr int AP_ROW_REGS = AP_MAX_W / 64;
constexpr float AP_EPS = 1e-6f;       // utils/utils.py:159,168
constexpr float AP_INV_LN2 = 1.4426950408889634f;
constexpr float AP_NEG = -3.402823466e38f;

enum { AP_DISP_L = 1, AP_CONF_L = 2, AP_DISP_R = 4, AP_CONF_R = 8 };

__device__ __forceinline__ float ap_wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// butterfly sum of a double through two fp32 shuffles (hi + lo carries 48 bits); every lane ends with the same bits
__device__ __forceinline__ double ap_wave_sum(double x) {
    for (int off = 32; off > 0; off >>= 1) {
        const float hi = (float)x, lo = (float)(x - (double)hi);
        const float ohi = __shfl_xor(hi, off), olo = __shfl_xor(lo, off);
        x = ((double)hi + (double)lo) + ((double)ohi + (double)olo);
    }
    return x;
}

// f'(p) for f(p) = p log2(p + eps); `l` returns log2(p + eps)
__device__ __forceinline__ float ap_entropy_slope(float p, float& l) {
    const float x = p + AP_EPS;
    l = log2f(x);
    return l + (p / x) * AP_INV_LN2;
}

// ------------------------------------------------------------------------------------------------ row direction (left)
// grid cdiv(R, AP_WAVES); stats may be NULL (no backward), disp / conf may be NULL
__global__ __launch_bounds__(AP_THREADS) void allpairs_rows_kernel(const float* __restrict__ vol, float* __restrict__ disp,
                                                                   float* __restrict__ conf, float* __restrict__ stats,
                                                                   long long R, int W1, int W2, double inv_log) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * AP_WAVES + wave;
    if (r >= R) return;                                                  // (the whole wave)
    const float* row = vol + (size_t)r * W2;
    float v[AP_ROW_REGS];
    float m = AP_NEG;
#pragma unroll
    for (int k = 0; k < AP_ROW_REGS; ++k) {
        const int w2 = 64 * k + lane;
        v[k] = w2 < W2 ? row[w2] : AP_NEG;
        m = fmaxf(m, v[k]);
    }
    m = ap_wave_max(m);
    double s = 0.0, n1 = 0.0;
#pragma unroll
    for (int k = 0; k < AP_ROW_REGS; ++k) {
        const int w2 = 64 * k + lane;
        v[k] = w2 < W2 ? expf(v[k] - m) : 0.f;
        s += (double)v[k];
        n1 += (double)v[k] * (double)w2;
    }
    s = ap_wave_sum(s);
    n1 = ap_wave_sum(n1);
    const double E = n1 / s;
    double h = 0.0, f = 0.0;
    if (conf || stats) {
        const double inv = 1.0 / s;
#pragma unroll
        for (int k = 0; k < AP_ROW_REGS; ++k) {
            const float p = (float)((double)v[k] * inv);                 // 0 past the row end: contributes 0 * log2(eps)
            float l;
            const float slope = ap_entropy_slope(p, l);
            h += (double)p * (double)l;
            f += (double)p * (double)slope;
        }
        h = ap_wave_sum(h);
        if (stats) f = ap_wave_sum(f);
    }
    if (lane == 0) {
        const int w1 = (int)(r % W1);
        if (disp) disp[r] = (float)((double)w1 - E);
        if (conf) conf[r] = (float)(1.0 + h * inv_log);
        if (stats) {
            float* st = stats + 4 * (size_t)r;
            st[0] = m; st[1] = (float)s; st[2] = (float)E; st[3] = (float)f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ column direction (right)
// grid nstrips * B*H (strip fastest); dynamic LDS 2 * AP_WAVES * 64 doubles; cstats = the column part of `stats` or NULL
__global__ __launch_bounds__(AP_THREADS) void allpairs_cols_kernel(const float* __restrict__ vol, float* __restrict__ disp,
                                                                   float* __restrict__ conf, float* __restrict__ cstats, int W1,
                                                                   int W2, int nstrips, double inv_log) {
    STX_DYN_SMEM(smem);
    double* part0 = reinterpret_cast<double*>(smem);
    double* part1 = part0 + AP_WAVES * 64;
    float* partm = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = (int)(blockIdx.x % (unsigned)nstrips);
    const size_t bh = blockIdx.x / (unsigned)nstrips;
    const int w2 = strip * 64 + lane;
    const bool ok = w2 < W2;
    const float* col = vol + bh * (size_t)W1 * W2 + (ok ? w2 : 0);
    // pass 1: the column's max
    float m = AP_NEG;
    if (ok)
        for (int w1 = wave; w1 < W1; w1 += AP_WAVES) m = fmaxf(m, col[(size_t)w1 * W2]);
    partm[wave * 64 + lane] = m;
    __syncthreads();
    for (int w = 0; w < AP_WAVES; ++w) m = fmaxf(m, partm[w * 64 + lane]);
    __syncthreads();
    // pass 2: sum and first moment of exp(v - max)
    double s = 0.0, n1 = 0.0;
    if (ok)
        for (int w1 = wave; w1 < W1; w1 += AP_WAVES) {
            const double e = (double)expf(col[(size_t)w1 * W2] - m);
            s += e;
            n1 += e * (double)w1;
        }
    part0[wave * 64 + lane] = s;
    part1[wave * 64 + lane] = n1;
    __syncthreads();
    s = 0.0; n1 = 0.0;
    for (int w = 0; w < AP_WAVES; ++w) { s += part0[w * 64 + lane]; n1 += part1[w * 64 + lane]; }
    __syncthreads();
    const double E = ok ? n1 / s : 0.0;
    // pass 3: the entropy sums on the normalised p
    double h = 0.0, f = 0.0;
    if (conf || cstats) {
        if (ok) {
            const double inv = 1.0 / s;
            for (int w1 = wave; w1 < W1; w1 += AP_WAVES) {
                const float p = (float)((double)expf(col[(size_t)w1 * W2] - m) * inv);
                float l;
                const float slope = ap_entropy_slope(p, l);
                h += (double)p * (double)l;
                f += (double)p * (double)slope;
            }
        }
        part0[wave * 64 + lane] = h;
        part1[wave * 64 + lane] = f;
        __syncthreads();
        h = 0.0; f = 0.0;
        for (int w = 0; w < AP_WAVES; ++w) { h += part0[w * 64 + lane]; f += part1[w * 64 + lane]; }
    }
    if (wave == 0 && ok) {
        const size_t c = bh * (size_t)W2 + w2;
        if (disp) disp[c] = (float)(E - (double)w2);
        if (conf) conf[c] = (float)(1.0 + h * inv_log);
        if (cstats) {
            float* st = cstats + 4 * c;
            st[0] = m; st[1] = (float)s; st[2] = (float)E; st[3] = (float)f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
struct ApGrads {
    const float *disp_l, *conf_l, *disp_r, *conf_r;                      // any may be NULL
    float k_l, k_r;                                                      // 1 / log2(W2), 1 / log2(W1)
};

// p (a disp (k - E) + c (f'(p) - F)) for one direction; st = (max, sum, E, F)
__device__ __forceinline__ float ap_direction_grad(float v, const float* st, float k, float a, float c) {
    const float p = expf(v - st[0]) / st[1];
    float l;
    const float slope = ap_entropy_slope(p, l);
    return p * (a * (k - st[2]) + c * (slope - st[3]));
}

// grid cdiv(R, AP_WAVES): one wave per row, lanes along w2
__global__ __launch_bounds__(AP_THREADS) void allpairs_bwd_kernel(ApGrads g, const float* __restrict__ vol,
                                                                  const float* __restrict__ stats, float* __restrict__ gvol,
                                                                  long long R, int W1, int W2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * AP_WAVES + wave;
    if (r >= R) return;
    const int w1 = (int)(r % W1);
    const size_t bh = (size_t)(r / W1);
    const bool left = g.disp_l || g.conf_l, right = g.disp_r || g.conf_r;
    const float* rst = stats + 4 * (size_t)r;
    const float* cst = stats + 4 * (size_t)R + 4 * bh * (size_t)W2;
    const float a_l = g.disp_l ? -g.disp_l[r] : 0.f;                     // disp_l = w1 - E
    const float c_l = g.conf_l ? g.conf_l[r] * g.k_l : 0.f;
    for (int w2 = lane; w2 < W2; w2 += 64) {
        const float v = vol[(size_t)r * W2 + w2];
        float out = 0.f;
        if (left) out = ap_direction_grad(v, rst, (float)w2, a_l, c_l);
        if (right) {
            const size_t c = bh * (size_t)W2 + w2;
            const float a_r = g.disp_r ? g.disp_r[c] : 0.f;
            const float c_r = g.conf_r ? g.conf_r[c] * g.k_r : 0.f;
            out += ap_direction_grad(v, cst + 4 * (size_t)w2, (float)w1, a_r, c_r);
        }
        gvol[(size_t)r * W2 + w2] = out;
    }
}

// ------------------------------------------------------------------------------------------------ truncation, pyramid
// truncate_corr_volume_v2 (utils/utils.py:229-236): (1 - c) + c (sigmoid((w1 - disp) - w2) (1 - atten) + atten)
__device__ __forceinline__ float ap_truncation(float center, int w2, float c, float atten) {
    const float x = center - (float)w2;
    const float sg = 1.f / (1.f + expf(-x));
    return (1.f - c) + c * (sg * (1.f - atten) + atten);
}

struct ApTruncate {
    const float *disp, *conf;                                            // [R] each; disp NULL = no truncation
    float atten, conf_th;
    int has_th;                                                          // conf := conf > conf_th
    __device__ __forceinline__ bool on() const { return disp != nullptr; }
    __device__ __forceinline__ float confidence(long long r) const {
        const float c = conf[r];
        return has_th ? (c > conf_th ? 1.f : 0.f) : c;
    }
};

// grid cdiv(R, AP_WAVES): one wave per row; w2 = 64 k + lane, so neighbouring lanes hold neighbouring w2 and a pooled
// element's children sit in one aligned group of 2 / 4 / 8 lanes
__global__ __launch_bounds__(AP_THREADS) void volume_pyramid_fwd_kernel(const float* __restrict__ vol, ApTruncate t,
                                                                        float* __restrict__ cpyr, long long R, int W1, int W2,
                                                                        int levels) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * AP_WAVES + wave;
    if (r >= R) return;
    const int len1 = W2 >> 1, len2 = W2 >> 2, len3 = W2 >> 3;
    float* l0 = cpyr + (size_t)r * W2;
    float* l1 = cpyr + geo_level_offset(R, W2, 1, 1) + (size_t)r * len1;
    float* l2 = cpyr + geo_level_offset(R, W2, 1, 2) + (size_t)r * len2;
    float* l3 = cpyr + geo_level_offset(R, W2, 1, 3) + (size_t)r * len3;
    const float center = t.on() ? (float)(int)(r % W1) - t.disp[r] : 0.f;
    const float c = t.on() ? t.confidence(r) : 0.f;
    for (int k0 = 0; k0 < W2; k0 += 64) {                                // (uniform trip count: every lane shuffles)
        const int w2 = k0 + lane;
        float v0 = w2 < W2 ? vol[(size_t)r * W2 + w2] : 0.f;
        if (t.on()) v0 *= ap_truncation(center, w2, c, t.atten);
        // rounded on its own: contracted into the pooling sum, level 1 would not be the average of the stored level 0
        STX_OPAQUE_VGPR(v0);
        const float v1 = (v0 + __shfl_xor(v0, 1)) * 0.5f;
        const float v2 = (v1 + __shfl_xor(v1, 2)) * 0.5f;
        const float v3 = (v2 + __shfl_xor(v2, 4)) * 0.5f;
        if (w2 < W2) l0[w2] = v0;
        if (levels > 1 && !(lane & 1) && (w2 >> 1) < len1) l1[w2 >> 1] = v1;
        if (levels > 2 && !(lane & 3) && (w2 >> 2) < len2) l2[w2 >> 2] = v2;
        if (levels > 3 && !(lane & 7) && (w2 >> 3) < len3) l3[w2 >> 3] = v3;
    }
}

// gvol = factor * (g0 + g1 / 2 + g2 / 4 + g3 / 8 of the elements this one was pooled into); every element written
__global__ __launch_bounds__(AP_THREADS) void volume_pyramid_bwd_kernel(const float* __restrict__ gcpyr, ApTruncate t,
                                                                        float* __restrict__ gvol, long long R, int W1, int W2,
                                                                        int levels) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * AP_WAVES + wave;
    if (r >= R) return;
    const int len1 = W2 >> 1, len2 = W2 >> 2, len3 = W2 >> 3;
    const float* l0 = gcpyr + (size_t)r * W2;
    const float* l1 = gcpyr + geo_level_offset(R, W2, 1, 1) + (size_t)r * len1;
    const float* l2 = gcpyr + geo_level_offset(R, W2, 1, 2) + (size_t)r * len2;
    const float* l3 = gcpyr + geo_level_offset(R, W2, 1, 3) + (size_t)r * len3;
    const float center = t.on() ? (float)(int)(r % W1) - t.disp[r] : 0.f;
    const float c = t.on() ? t.confidence(r) : 0.f;
    for (int w2 = lane; w2 < W2; w2 += 64) {
        float v = l0[w2];
        if (levels > 1 && (w2 >> 1) < len1) v = fmaf(0.5f, l1[w2 >> 1], v);
        if (levels > 2 && (w2 >> 2) < len2) v = fmaf(0.25f, l2[w2 >> 2], v);
        if (levels > 3 && (w2 >> 3) < len3) v = fmaf(0.125f, l3[w2 >> 3], v);
        if (t.on()) v *= ap_truncation(center, w2, c, t.atten);
        gvol[(size_t)r * W2 + w2] = v;
    }
}

// mask [R][W2]
__global__ __launch_bounds__(AP_THREADS) void truncate_mask_kernel(ApTruncate t, float* __restrict__ mask, long long R, int W1,
                                                                   int W2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * AP_WAVES + wave;
    if (r >= R) return;
    const float center = (float)(int)(r % W1) - t.disp[r];
    const float c = t.confidence(r);
    for (int w2 = lane; w2 < W2; w2 += 64) mask[(size_t)r * W2 + w2] = ap_truncation(center, w2, c, t.atten);
}

// ------------------------------------------------------------------------------------------------ host side
int ap_shape_ok(int B, int H, int W1, int W2, const char* what) {
    STX_REQUIRE(B > 0 && H > 0 && W1 > 0 && W2 > 0, "%s: bad shape B=%d H=%d W1=%d W2=%d", what, B, H, W1, W2);
    STX_REQUIRE((long long)B * H * W1 * (long long)W2 < (1ll << 40), "%s: tensor too large", what);
    STX_REQUIRE((long long)B * H * W1 / AP_WAVES < (1ll << 31) - 1, "%s: too many rows", what);
    return STX_OK;
}

int ap_estimates_shape_ok(int B, int H, int W1, int W2, const char* what) {
    if (int rc = ap_shape_ok(B, H, W1, W2, what)) return rc;
    STX_REQUIRE(W1 >= 2 && W1 <= AP_MAX_W && W2 >= 2 && W2 <= AP_MAX_W, "%s: W1=%d / W2=%d outside 2..%d", what, W1, W2, AP_MAX_W);
    STX_REQUIRE((long long)B * H * stx_cdiv(W2, 64) < (1ll << 31) - 1, "%s: too many column strips", what);
    return STX_OK;
}

int ap_pyramid_shape_ok(int B, int H, int W1, int W2, int levels, const char* what) {
    if (int rc = ap_shape_ok(B, H, W1, W2, what)) return rc;
    STX_REQUIRE(levels >= 1 && levels <= CP_MAX_LEVELS, "%s: num_levels %d outside 1..%d", what, levels, CP_MAX_LEVELS);
    STX_REQUIRE((W2 >> (levels - 1)) >= 2, "%s: W2=%d leaves level %d shorter than 2", what, W2, levels - 1);
    return STX_OK;
}

inline unsigned ap_row_grid(long long R) { return (unsigned)((R + AP_WAVES - 1) / AP_WAVES); }

}  // namespace

extern "C" int stx_allpairs_estimates_fwd(const float* vol, int which, float* disp_l, float* conf_l, float* disp_r, float* conf_r,
                                          float* stats, int B, int H, int W1, int W2, void* stream) {
    stx_begin();
    const char* what = "allpairs_estimates_fwd";
    STX_REQUIRE(vol, "%s: null pointer", what);
    STX_REQUIRE(which > 0 && which < 16, "%s: `which` (%d) is a mask of bits 1 (disp_l), 2 (conf_l), 4 (disp_r), 8 (conf_r)", what, which);
    STX_REQUIRE(!(which & AP_DISP_L) == !disp_l && !(which & AP_CONF_L) == !conf_l && !(which & AP_DISP_R) == !disp_r &&
                    !(which & AP_CONF_R) == !conf_r,
                "%s: exactly the outputs named by `which` (%d) must be non-null", what, which);
    if (int rc = ap_estimates_shape_ok(B, H, W1, W2, what)) return rc;
    const long long R = (long long)B * H * W1;
    if (which & (AP_DISP_L | AP_CONF_L)) {
        hipLaunchKernelGGL(allpairs_rows_kernel, dim3(ap_row_grid(R)), dim3(AP_THREADS), 0, (hipStream_t)stream, vol, disp_l, conf_l, stats,
                           R, W1, W2, 1.0 / log2((double)W2));
        if (int rc = stx_check_launch(what)) return rc;
    }
    if (which & (AP_DISP_R | AP_CONF_R)) {
        const int nstrips = stx_cdiv(W2, 64);
        const size_t lds = 2 * AP_WAVES * 64 * sizeof(double);
        if (int rc = stx_lds_require((const void*)allpairs_cols_kernel, lds, what)) return rc;
        hipLaunchKernelGGL(allpairs_cols_kernel, dim3((unsigned)(nstrips * B * H)), dim3(AP_THREADS), lds, (hipStream_t)stream, vol, disp_r,
                           conf_r, stats ? stats + 4 * (size_t)R : nullptr, W1, W2, nstrips, 1.0 / log2((double)W1));
        if (int rc = stx_check_launch(what)) return rc;
    }
    return STX_OK;
}

extern "C" int stx_allpairs_estimates_bwd(const float* g_disp_l, const float* g_conf_l, const float* g_disp_r, const float* g_conf_r,
                                          const float* vol, const float* stats, float* gvol, int B, int H, int W1, int W2,
                                          void* stream) {
    stx_begin();
    const char* what = "allpairs_estimates_bwd";
    STX_REQUIRE(vol && stats && gvol, "%s: null pointer", what);
    STX_REQUIRE(g_disp_l || g_conf_l || g_disp_r || g_conf_r, "%s: no gradient given", what);
    if (int rc = ap_estimates_shape_ok(B, H, W1, W2, what)) return rc;
    const long long R = (long long)B * H * W1;
    ApGrads g{g_disp_l, g_conf_l, g_disp_r, g_conf_r, 1.f / log2f((float)W2), 1.f / log2f((float)W1)};
    hipLaunchKernelGGL(allpairs_bwd_kernel, dim3(ap_row_grid(R)), dim3(AP_THREADS), 0, (hipStream_t)stream, g, vol, stats, gvol, R, W1, W2);
    return stx_check_launch(what);
}

extern "C" int stx_corr1d_volume_pyramid_fwd(const float* vol, const float* tdisp, const float* tconf, float atten, float* cpyr, int B,
                                             int H, int W1, int W2, int levels, void* stream) {
    stx_begin();
    const char* what = "corr1d_volume_pyramid_fwd";
    STX_REQUIRE(vol && cpyr && !tdisp == !tconf, "%s: null pointer (tdisp and tconf go together)", what);
    if (int rc = ap_pyramid_shape_ok(B, H, W1, W2, levels, what)) return rc;
    const long long R = (long long)B * H * W1;
    ApTruncate t{tdisp, tconf, atten, 0.f, 0};
    hipLaunchKernelGGL(volume_pyramid_fwd_kernel, dim3(ap_row_grid(R)), dim3(AP_THREADS), 0, (hipStream_t)stream, vol, t, cpyr, R, W1, W2,
                       levels);
    return stx_check_launch(what);
}

extern "C" int stx_corr1d_volume_pyramid_bwd(const float* gcpyr, const float* tdisp, const float* tconf, float atten, float* gvol,
                                             int B, int H, int W1, int W2, int levels, void* stream) {
    stx_begin();
    const char* what = "corr1d_volume_pyramid_bwd";
    STX_REQUIRE(gcpyr && gvol && !tdisp == !tconf, "%s: null pointer (tdisp and tconf go together)", what);
    if (int rc = ap_pyramid_shape_ok(B, H, W1, W2, levels, what)) return rc;
    const long long R = (long long)B * H * W1;
    ApTruncate t{tdisp, tconf, atten, 0.f, 0};
    hipLaunchKernelGGL(volume_pyramid_bwd_kernel, dim3(ap_row_grid(R)), dim3(AP_THREADS), 0, (hipStream_t)stream, gcpyr, t, gvol, R, W1,
                       W2, levels);
    return stx_check_launch(what);
}

extern "C" int stx_truncate_mask_fwd(const float* disp, const float* conf, int has_th, float conf_th, float atten, float* mask, int B,
                                     int H, int W, void* stream) {
    stx_begin();
    const char* what = "truncate_mask_fwd";
    STX_REQUIRE(disp && conf && mask, "%s: null pointer", what);
    if (int rc = ap_shape_ok(B, H, W, W, what)) return rc;
    const long long R = (long long)B * H * W;
    ApTruncate t{disp, conf, atten, conf_th, has_th ? 1 : 0};
    hipLaunchKernelGGL(truncate_mask_kernel, dim3(ap_row_grid(R)), dim3(AP_THREADS), 0, (hipStream_t)stream, t, mask, R, W, W);
    return stx_check_launch(what);
}

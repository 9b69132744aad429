// StereoAnywhere's mono-stereo alignment stage (reference models/StereoAnywhere/stereoanywhere.py:167-235, utils/utils.py:48-54,
// 172-198, 255-269, 345-384): what the reference runs between its aggregation networks and the GRU loop.
//   * generate_masks / the masked N-channel volume  volume * left_masks.unsqueeze(4) * right_masks.unsqueeze(3): the masks are
//     one-hot in N, so at most one channel of out[b, :, h, w2, w3] is non-zero.  Stock: a 2 N-iteration mask loop and two
//     broadcast multiplies (the N-fold volume written, read back and written again); here the volume row is read once and the N
//     output rows are written once, the all-zero rows without touching the volume.  The backward reads ONE channel row.
//   * softlrc: both left-right-consistency maps from one launch; the backward (direct term, sampled value, sample coordinate
//     through relu) in two launches without float atomics: per-source coefficients first, then every target pixel GATHERS what
//     the stock grid_sample backward scatters -- the bilinear weight of source column x on target column x' is the hat function
//     max(0, 1 - |ix(x) - x'|) -- in a fixed order, so the result is bitwise reproducible.
//   * weighted_lsq: per image ONE workgroup selects the four order statistics torch.quantile would read off a sorted copy
//     (radix select on the bit pattern of relu(disp) >= 0, 8 bits a pass, integer LDS histograms), forms torch.quantile's own
//     fp32 `lerp`, accumulates the five weighted sums in double in a fixed order and solves the 2 x 2 normal equations.  No sort,
//     no compaction, nothing read back by the host.  One elementwise launch for the three gradients.
//   * handcrafted_mirror_detector: one elementwise kernel forward, one backward for the four gradients.
// Coordinates, sums and the transcendental functions of the map-sized kernels are formed in double (the maps are a few ten
// thousand pixels); the volume kernels only move fp32 values.
#include "stx_common.h"

namespace {

constexpr int MA_THREADS = 256;       // four waves
constexpr int MA_WAVES = MA_THREADS / 64;
constexpr int MA_MAX_N = 64;          // mask channels
constexpr int MA_MAX_W = 2048;        // masked volume: bins of one right row in LDS (one byte each)
constexpr int MA_ROWS = 16;           // masked volume: volume rows (b, h, w2) per workgroup, four per wave
constexpr int MA_LRC_MAX_W = 1024;    // softlrc backward: one source row in LDS (four doubles per column)
constexpr int MA_LSQ_THREADS = 512;   // weighted_lsq: one workgroup per image
constexpr int MA_LSQ_WAVES = MA_LSQ_THREADS / 64;
constexpr int MA_LSQ_STATS = 8;       // doubles per image: S_wmm, S_wm, S_w, S_wms, S_ws, min threshold, max threshold, 0

__device__ __forceinline__ unsigned ma_bits(float f) {
    union { float f; unsigned u; } c;
    c.f = f;
    return c.u;
}
__device__ __forceinline__ float ma_float(unsigned u) {
    union { float f; unsigned u; } c;
    c.u = u;
    return c.f;
}

// ------------------------------------------------------------------------------------------------ the bin rule
// generate_masks (utils/utils.py:48-54): channel i where f32(i / N) <= v < f32((i + 1) / N) -- the thresholds are python's double
// quotients rounded to fp32 by the comparison with an fp32 tensor, the comparison itself is fp32.  -1: no bin (v >= 1, v < 0, NaN).
__device__ __forceinline__ float ma_threshold(int i, int N) { return (float)((double)i / (double)N); }

__device__ __forceinline__ int ma_bin(float v, int N) {
    if (!(v >= 0.f) || !(v < ma_threshold(N, N))) return -1;
    int i = (int)(v * (float)N);                                         // a guess, off by one at most; then the rule itself
    i = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
    while (i > 0 && v < ma_threshold(i, N)) --i;
    while (i < N - 1 && !(v < ma_threshold(i + 1, N))) ++i;
    return i;
}

// masks [B][N][H][W] as fp16 bit patterns (1.0 = 0x3C00); one thread per pixel, every channel written
__global__ __launch_bounds__(MA_THREADS) void generate_masks_kernel(const float* __restrict__ mde, unsigned short* __restrict__ masks,
                                                                    long long pixels, long long HW, int N) {
    const long long p = (long long)blockIdx.x * MA_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const int bin = ma_bin(mde[p], N);
    const long long b = p / HW, hw = p % HW;
    unsigned short* out = masks + (size_t)b * N * HW + hw;
    for (int n = 0; n < N; ++n) out[(size_t)n * HW] = n == bin ? (unsigned short)0x3C00 : (unsigned short)0;
}

// ------------------------------------------------------------------------------------------------ masked volume
// grid B*H * cdiv(W2, MA_ROWS) (chunk fastest).  BWD = false: out[b][n][h][w2][:] = vol row where n == bin_left(w2) and
// bin_right(w3) == n, else 0.  BWD = true: `wide` is the gradient of that tensor and `flat` [B][H][W2][W3] receives
// g[b][bin_left][h][w2][w3] where the bins agree, else 0.  VEC: W3 % 4 == 0, every row 16-byte aligned.
template <bool BWD, bool VEC>
__global__ __launch_bounds__(MA_THREADS) void masked_volume_kernel(float* __restrict__ flat, const float* __restrict__ mde_l,
                                                                   const float* __restrict__ mde_r, float* __restrict__ wide, int N,
                                                                   int H, int W2, int W3, int chunks) {
    __shared__ signed char rbin[MA_MAX_W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const size_t bh = blockIdx.x / (unsigned)chunks;
    const size_t b = bh / (unsigned)H, h = bh % (unsigned)H;
    for (int w3 = threadIdx.x; w3 < W3; w3 += MA_THREADS) rbin[w3] = (signed char)ma_bin(mde_r[bh * W3 + w3], N);
    __syncthreads();
    for (int row = wave; row < MA_ROWS; row += MA_WAVES) {
        const int w2 = chunk * MA_ROWS + row;
        if (w2 >= W2) break;                                             // (the whole wave)
        const int lbin = ma_bin(mde_l[bh * W2 + w2], N);                 // wave-uniform
        float* frow = flat + (bh * W2 + w2) * (size_t)W3;
        if (BWD) {
            const float* grow = lbin < 0 ? nullptr : wide + (((b * N + lbin) * H + h) * W2 + w2) * (size_t)W3;
            if (VEC) {
                for (int c = 4 * lane; c < W3; c += 256) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (grow) {
                        v = stx_ld4(grow + c);
                        v.x = rbin[c] == lbin ? v.x : 0.f;
                        v.y = rbin[c + 1] == lbin ? v.y : 0.f;
                        v.z = rbin[c + 2] == lbin ? v.z : 0.f;
                        v.w = rbin[c + 3] == lbin ? v.w : 0.f;
                    }
                    stx_st4(frow + c, v);
                }
            } else {
                for (int c = lane; c < W3; c += 64) frow[c] = (grow && rbin[c] == lbin) ? grow[c] : 0.f;
            }
            continue;
        }
        for (int n = 0; n < N; ++n) {
            float* orow = wide + (((b * N + n) * H + h) * W2 + w2) * (size_t)W3;
            const bool live = n == lbin;                                 // a row of zeros otherwise: the volume is not read
            if (VEC) {
                for (int c = 4 * lane; c < W3; c += 256) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (live) {
                        v = stx_ld4(frow + c);
                        v.x = rbin[c] == n ? v.x : 0.f;
                        v.y = rbin[c + 1] == n ? v.y : 0.f;
                        v.z = rbin[c + 2] == n ? v.z : 0.f;
                        v.w = rbin[c + 3] == n ? v.w : 0.f;
                    }
                    stx_st4(orow + c, v);
                }
            } else {
                for (int c = lane; c < W3; c += 64) orow[c] = (live && rbin[c] == n) ? frow[c] : 0.f;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ softlrc
// disp_warping (utils/utils.py:172-187): grid 2 (x -+ d) / W - 1, 2 y / H - 1, align_corners=True, zeros padding, i.e. the sample
// column (x -+ d) (W - 1) / W and the fractional row y (H - 1) / H.
__device__ __forceinline__ double lrc_column(int x, float d, double sign, int W) {
    const double r = d > 0.f ? (double)d : 0.0;                          // relu
    return ((double)x + sign * r) * (double)(W - 1) / (double)W;
}
// rows y0 and y0 + 1 with weights 1 - wy1 and wy1 (row y0 + 1 may lie outside only with weight 0)
__device__ __forceinline__ void lrc_rows(int y, int H, int& y0, double& wy1) {
    const double iy = (double)y * (double)(H - 1) / (double)H;
    const double f = floor(iy);
    y0 = (int)f;
    wy1 = iy - f;
}
// bilinear sample of img [H][W] at (column ix, the rows of y) and its derivative along ix
__device__ __forceinline__ double lrc_sample(const float* __restrict__ img, int y, double ix, int H, int W, double& d_ix) {
    int y0;
    double wy1;
    lrc_rows(y, H, y0, wy1);
    const double fx = floor(ix);
    const double wx1 = ix - fx;
    double v = 0.0;
    d_ix = 0.0;
    if (fx >= -1.0 && fx <= (double)(W - 1)) {                           // otherwise both taps lie outside
        const int x0 = (int)fx, x1 = x0 + 1;
        for (int k = 0; k < 2; ++k) {
            const int yy = y0 + k;
            const double wy = k ? wy1 : 1.0 - wy1;
            if (yy >= H) continue;
            const double a = x0 >= 0 ? (double)img[(size_t)yy * W + x0] : 0.0;
            const double c = x1 < W ? (double)img[(size_t)yy * W + x1] : 0.0;
            v += wy * (a * (1.0 - wx1) + c * wx1);
            d_ix += wy * (c - a);
        }
    }
    return v;
}
// softplus(th - |u|) / log(1 + e^th) and its derivative along u; th <= 20: below the threshold of F.softplus throughout
__device__ __forceinline__ double lrc_soft(double u, double th, double inv_div, double& d_u) {
    const double x = th - fabs(u);
    const double e = exp(x);
    d_u = -(e / (1.0 + e)) * (u > 0.0 ? 1.0 : (u < 0.0 ? -1.0 : 0.0)) * inv_div;
    return log1p(e) * inv_div;
}

// one thread per pixel, both outputs.  COEF (backward, pass 1): ws = four planes of `pixels` doubles,
//   0 / 1  dL/d disp2 and dL/d disp3 without the sampled-value path: the direct term and the sample coordinate through relu
//   2 / 3  dL/d(warped disp3) of out2's pixel, dL/d(warped disp2) of out3's pixel (what grid_sample's backward scatters)
template <bool COEF>
__global__ __launch_bounds__(MA_THREADS) void softlrc_kernel(const float* __restrict__ disp2, const float* __restrict__ disp3,
                                                             const float* __restrict__ g2, const float* __restrict__ g3,
                                                             float* __restrict__ out2, float* __restrict__ out3,
                                                             double* __restrict__ ws, long long pixels, int H, int W, double th,
                                                             double inv_div) {
    const long long p = (long long)blockIdx.x * MA_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const size_t img = (size_t)(p / ((long long)H * W)) * H * W;
    const float d2 = disp2[p], d3 = disp3[p];
    double s3, s2, e2, e3;
    const double w3 = lrc_sample(disp3 + img, y, lrc_column(x, d2, -1.0, W), H, W, s3);   // warped_disp3 (utils.py:193)
    const double w2 = lrc_sample(disp2 + img, y, lrc_column(x, d3, 1.0, W), H, W, s2);    // warped_disp2 (utils.py:192)
    const double o2 = lrc_soft((double)d2 - w3, th, inv_div, e2);
    const double o3 = lrc_soft((double)d3 - w2, th, inv_div, e3);
    if (!COEF) {
        out2[p] = (float)o2;
        out3[p] = (float)o3;
        return;
    }
    const double c2 = g2 ? (double)g2[p] * e2 : 0.0, c3 = g3 ? (double)g3[p] * e3 : 0.0;
    const double k = (double)(W - 1) / (double)W;
    ws[p] = c2 * (1.0 + (d2 > 0.f ? s3 * k : 0.0));                      // u2 = d2 - warped3((x - relu d2) k)
    ws[pixels + p] = c3 * (1.0 - (d3 > 0.f ? s2 * k : 0.0));             // u3 = d3 - warped2((x + relu d3) k)
    ws[2 * pixels + p] = -c2;
    ws[3 * pixels + p] = -c3;
}

// backward, pass 2: grid B * H (one workgroup per target row y'), the source rows y' - 1 .. y' + 1 staged one at a time:
// col[0 / 1][x] the sample column of out2's / out3's pixel (y, x), cw[0 / 1][x] its coefficient times the row weight on y'.
// g_disp3[y'][x'] = ws0-plane-1 + sum over out2's pixels, g_disp2[y'][x'] = plane 0 + sum over out3's pixels; x ascending.
__global__ __launch_bounds__(MA_THREADS) void softlrc_gather_kernel(const float* __restrict__ disp2, const float* __restrict__ disp3,
                                                                    const double* __restrict__ ws, float* __restrict__ gd2,
                                                                    float* __restrict__ gd3, long long pixels, int H, int W) {
    STX_DYN_SMEM(smem);
    double* col0 = reinterpret_cast<double*>(smem);
    double* col1 = col0 + W;
    double* cw0 = col1 + W;
    double* cw1 = cw0 + W;
    const int yt = (int)(blockIdx.x % (unsigned)H);
    const size_t img = (size_t)(blockIdx.x / (unsigned)H) * H * W;
    double acc2[MA_LRC_MAX_W / MA_THREADS], acc3[MA_LRC_MAX_W / MA_THREADS];
#pragma unroll
    for (int k = 0; k < MA_LRC_MAX_W / MA_THREADS; ++k) acc2[k] = acc3[k] = 0.0;
    for (int y = yt > 0 ? yt - 1 : 0; y <= yt + 1 && y < H; ++y) {       // (block-uniform)
        int y0;
        double wy1;
        lrc_rows(y, H, y0, wy1);
        const double wy = (y0 == yt ? 1.0 - wy1 : 0.0) + (y0 + 1 == yt ? wy1 : 0.0);
        if (wy == 0.0) continue;
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += MA_THREADS) {
            const size_t s = img + (size_t)y * W + x;
            col0[x] = lrc_column(x, disp2[s], -1.0, W);
            col1[x] = lrc_column(x, disp3[s], 1.0, W);
            cw0[x] = ws[2 * pixels + s] * wy;
            cw1[x] = ws[3 * pixels + s] * wy;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MA_LRC_MAX_W / MA_THREADS; ++k) {
            const int xt = k * MA_THREADS + (int)threadIdx.x;
            if (xt >= W) continue;
            double a3 = acc3[k], a2 = acc2[k];
            for (int x = 0; x < W; ++x) {
                const double h0 = 1.0 - fabs(col0[x] - (double)xt), h1 = 1.0 - fabs(col1[x] - (double)xt);
                a3 += cw0[x] * (h0 > 0.0 ? h0 : 0.0);                    // out2 samples disp3
                a2 += cw1[x] * (h1 > 0.0 ? h1 : 0.0);                    // out3 samples disp2
            }
            acc3[k] = a3;
            acc2[k] = a2;
        }
    }
#pragma unroll
    for (int k = 0; k < MA_LRC_MAX_W / MA_THREADS; ++k) {
        const int xt = k * MA_THREADS + (int)threadIdx.x;
        if (xt >= W) continue;
        const size_t t = img + (size_t)yt * W + xt;
        gd2[t] = (float)(ws[t] + acc2[k]);
        gd3[t] = (float)(ws[pixels + t] + acc3[k]);
    }
}

// ------------------------------------------------------------------------------------------------ weighted_lsq
struct LsqRanks {
    unsigned k[4];                                                       // 0-based ranks: floor / ceil of q_min (n - 1), of q_max (n - 1)
    float w_min, w_max;                                                  // the fractions
};

// torch.quantile's interpolation: at::lerp in fp32, one fused multiply-add
__device__ __forceinline__ float lsq_lerp(float a, float b, float w) {
    const float diff = b - a;
    return w < 0.5f ? fmaf(w, diff, a) : fmaf(-diff, 1.f - w, b);
}
__device__ __forceinline__ float lsq_relu(float d) { return d > 0.f ? d : 0.f; }   // +0 for -0: bit order = value order

// fixed-order tree over the workgroup; every thread returns the total
__device__ __forceinline__ double lsq_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MA_LSQ_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// the 2 x 2 normal equations; det == 0 (one distinct |mde| under the mask): scale 0, shift the weighted mean
__device__ __forceinline__ bool lsq_solve(const double* S, double& scale, double& shift, double& det) {
    det = S[0] * S[2] - S[1] * S[1];
    if (det == 0.0) {
        scale = 0.0;
        shift = S[4] / S[2];
        return false;
    }
    scale = (S[3] * S[2] - S[1] * S[4]) / det;
    shift = (S[0] * S[4] - S[1] * S[3]) / det;
    return true;
}

// grid B, MA_LSQ_THREADS threads: image b's n elements
__global__ __launch_bounds__(MA_LSQ_THREADS) void weighted_lsq_kernel(const float* __restrict__ mde, const float* __restrict__ disp,
                                                                      const float* __restrict__ conf, float* __restrict__ scale,
                                                                      float* __restrict__ shift, double* __restrict__ stats,
                                                                      unsigned n, LsqRanks ranks) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned prefix[4], krem[4];
    __shared__ int rep[4];
    __shared__ double red[MA_LSQ_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)blockIdx.x * n;
    const float* d = disp + base;
    if (tid < 4) {
        prefix[tid] = 0u;
        krem[tid] = ranks.k[tid];
        rep[tid] = 0;                                                    // pass 0: one histogram serves the four targets
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int sh = 24 - 8 * pass;
        for (int i = tid; i < 4 * 256; i += MA_LSQ_THREADS) (&hist[0][0])[i] = 0u;
        __syncthreads();
        const unsigned p0 = prefix[0], p1 = prefix[1], p2 = prefix[2], p3 = prefix[3];
        const bool own1 = rep[1] == 1, own2 = rep[2] == 2, own3 = rep[3] == 3;
        for (unsigned i = tid; i < n; i += MA_LSQ_THREADS) {
            const unsigned key = ma_bits(lsq_relu(d[i]));
            const unsigned digit = (key >> sh) & 255u;
            const unsigned long long hi = (unsigned long long)key >> (sh + 8);   // the digits of the earlier passes
            if (hi == ((unsigned long long)p0 >> (sh + 8))) atomicAdd(&hist[0][digit], 1u);
            if (own1 && hi == ((unsigned long long)p1 >> (sh + 8))) atomicAdd(&hist[1][digit], 1u);
            if (own2 && hi == ((unsigned long long)p2 >> (sh + 8))) atomicAdd(&hist[2][digit], 1u);
            if (own3 && hi == ((unsigned long long)p3 >> (sh + 8))) atomicAdd(&hist[3][digit], 1u);
        }
        __syncthreads();
        if (wave < 4) {                                                  // wave t: the digit of target t; counts < 2^24 are exact floats
            const unsigned* hrow = hist[rep[wave]];
            const unsigned c0 = hrow[4 * lane], c1 = hrow[4 * lane + 1], c2 = hrow[4 * lane + 2], c3 = hrow[4 * lane + 3];
            const unsigned k = krem[wave];                               // read by every lane before the scan, written after it
            const float mine = (float)(c0 + c1 + c2 + c3);
            float incl = mine;
            for (int off = 1; off < 64; off <<= 1) {
                const float o = __shfl(incl, lane >= off ? lane - off : lane);
                if (lane >= off) incl += o;
            }
            const unsigned below = (unsigned)(incl - mine), upto = (unsigned)incl;
            if (below <= k && k < upto) {                                // exactly one lane
                unsigned digit = 4u * lane, acc = below;
                if (k >= acc + c0) { acc += c0; ++digit;
                    if (k >= acc + c1) { acc += c1; ++digit;
                        if (k >= acc + c2) { acc += c2; ++digit; } } }
                prefix[wave] |= digit << sh;
                krem[wave] = k - acc;
            }
        }
        __syncthreads();
        if (tid < 4) {
            int r = tid;
            for (int t = tid - 1; t >= 0; --t)
                if (prefix[t] == prefix[tid]) r = t;
            rep[tid] = r;
        }
        __syncthreads();
    }
    const float t_min = lsq_lerp(ma_float(prefix[0]), ma_float(prefix[1]), ranks.w_min);
    const float t_max = lsq_lerp(ma_float(prefix[2]), ma_float(prefix[3]), ranks.w_max);
    double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned i = tid; i < n; i += MA_LSQ_THREADS) {
        const float sf = lsq_relu(d[i]);
        if (!(t_min <= sf && sf <= t_max)) continue;
        const double m = fabs((double)mde[base + i]), s = (double)sf, w = 0.9 * fabs((double)conf[base + i]) + 0.1;
        S[0] += w * m * m;
        S[1] += w * m;
        S[2] += w;
        S[3] += w * m * s;
        S[4] += w * s;
    }
    for (int j = 0; j < 5; ++j) S[j] = lsq_block_sum(S[j], red);
    if (tid == 0) {
        double sc, shf, det;
        lsq_solve(S, sc, shf, det);
        scale[blockIdx.x] = (float)sc;
        shift[blockIdx.x] = (float)shf;
        double* st = stats + (size_t)blockIdx.x * MA_LSQ_STATS;
        for (int j = 0; j < 5; ++j) st[j] = S[j];
        st[5] = (double)t_min;
        st[6] = (double)t_max;
        st[7] = 0.0;
    }
}

// grid (cdiv(n, MA_THREADS), B).  With M = [[S0, S1], [S1, S2]], theta = (scale, shift) = M^-1 (S3, S4) and lambda = M^-1 g:
//   dL/dw = -(l1 m + l2) e,  dL/dm = -w (l1 e + scale (l1 m + l2)),  dL/ds = w (l1 m + l2),   e = scale m + shift - s
// under the mask, then the signs of |mde|, |conf| (times 0.9) and the gate of relu.  The thresholds carry no gradient.
__global__ __launch_bounds__(MA_THREADS) void weighted_lsq_bwd_kernel(const float* __restrict__ g_scale, const float* __restrict__ g_shift,
                                                                      const float* __restrict__ mde, const float* __restrict__ disp,
                                                                      const float* __restrict__ conf, const double* __restrict__ stats,
                                                                      float* __restrict__ g_mde, float* __restrict__ g_disp,
                                                                      float* __restrict__ g_conf, unsigned n) {
    const unsigned i = blockIdx.x * MA_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t at = (size_t)blockIdx.y * n + i;
    const double* S = stats + (size_t)blockIdx.y * MA_LSQ_STATS;
    const float sf = lsq_relu(disp[at]);
    float om = 0.f, od = 0.f, oc = 0.f;
    if ((float)S[5] <= sf && sf <= (float)S[6]) {
        const double ga = g_scale ? (double)g_scale[blockIdx.y] : 0.0, gb = g_shift ? (double)g_shift[blockIdx.y] : 0.0;
        const double mv = (double)mde[at], cv = (double)conf[at];
        const double m = fabs(mv), s = (double)sf, w = 0.9 * fabs(cv) + 0.1;
        double sc, shf, det, dw, dm, ds;
        if (lsq_solve(S, sc, shf, det)) {
            const double l1 = (S[2] * ga - S[1] * gb) / det, l2 = (S[0] * gb - S[1] * ga) / det;
            const double e = sc * m + shf - s, lm = l1 * m + l2;
            dw = -lm * e;
            dm = -w * (l1 * e + sc * lm);
            ds = w * lm;
        } else {                                                         // shift = S4 / S2 alone
            dw = gb * (s - shf) / S[2];
            dm = 0.0;
            ds = gb * w / S[2];
        }
        om = (float)(mv > 0.0 ? dm : (mv < 0.0 ? -dm : 0.0));
        oc = (float)(cv > 0.0 ? 0.9 * dw : (cv < 0.0 ? -0.9 * dw : 0.0));
        od = sf > 0.f ? (float)ds : 0.f;
    }
    g_mde[at] = om;
    g_disp[at] = od;
    g_conf[at] = oc;
}

// ------------------------------------------------------------------------------------------------ mirror detector
// utils/utils.py:255-269: a = sc mc sigmoid(gain (md - sd)), b = (1 - sc) mc, out = sigmoid(gain (a + b - a b - th))
struct MirrorGrads {
    float *sd, *md, *sc, *mc;
};
template <bool BWD>
__global__ __launch_bounds__(MA_THREADS) void mirror_kernel(const float* __restrict__ go, const float* __restrict__ sd,
                                                            const float* __restrict__ md, const float* __restrict__ sc,
                                                            const float* __restrict__ mc, double th, double gain, float* __restrict__ out,
                                                            MirrorGrads g, long long n) {
    const long long i = (long long)blockIdx.x * MA_THREADS + threadIdx.x;
    if (i >= n) return;
    const double s = (double)sc[i], m = (double)mc[i];
    const double near = 1.0 / (1.0 + exp(-gain * ((double)md[i] - (double)sd[i])));
    const double both = s * m, a = both * near, b = (1.0 - s) * m;
    const double o = 1.0 / (1.0 + exp(-gain * (a + b - a * b - th)));
    if (!BWD) {
        out[i] = (float)o;
        return;
    }
    const double gm = (double)go[i] * o * (1.0 - o) * gain;
    const double ga = gm * (1.0 - b), gb = gm * (1.0 - a);
    const double gboth = ga * near, gmd = ga * both * near * (1.0 - near) * gain;
    g.md[i] = (float)gmd;
    g.sd[i] = (float)-gmd;
    g.sc[i] = (float)(gboth * m - gb * m);
    g.mc[i] = (float)(gboth * s + gb * (1.0 - s));
}

// ------------------------------------------------------------------------------------------------ host side
inline unsigned ma_grid(long long n) { return (unsigned)((n + MA_THREADS - 1) / MA_THREADS); }

int ma_map_ok(long long n, const char* what) {
    STX_REQUIRE(n > 0 && n < (1ll << 31) * MA_THREADS, "%s: %lld elements outside 1..2^39", what, n);
    return STX_OK;
}

int ma_volume_ok(int B, int N, int H, int W2, int W3, const char* what) {
    STX_REQUIRE(B > 0 && H > 0 && W2 > 0 && W3 > 0, "%s: bad shape B=%d H=%d W2=%d W3=%d", what, B, H, W2, W3);
    STX_REQUIRE(N >= 1 && N <= MA_MAX_N, "%s: n_masks %d outside 1..%d", what, N, MA_MAX_N);
    STX_REQUIRE(W3 <= MA_MAX_W, "%s: W3=%d above %d", what, W3, MA_MAX_W);
    STX_REQUIRE((long long)B * N * H * W2 * (long long)W3 < (1ll << 40), "%s: tensor too large", what);
    STX_REQUIRE((long long)B * H * stx_cdiv(W2, MA_ROWS) < (1ll << 31) - 1, "%s: too many rows", what);
    return STX_OK;
}

int ma_lrc_ok(int B, int H, int W, float lrc_th, const char* what) {
    STX_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", what, B, H, W);
    STX_REQUIRE((long long)B * H * W < (1ll << 31), "%s: tensor too large", what);
    STX_REQUIRE(lrc_th <= 20.f, "%s: lrc_th %g above 20 (the linear branch of softplus) is not supported", what, (double)lrc_th);
    return STX_OK;
}

int ma_lsq_ok(int B, long long n, const char* what) {
    STX_REQUIRE(B > 0 && n > 0, "%s: bad shape B=%d n=%lld", what, B, n);
    STX_REQUIRE(n < (1ll << 24), "%s: %lld elements per image; torch.quantile's own limit is 2^24", what, n);
    STX_REQUIRE(B <= 65535, "%s: B=%d above 65535", what, B);
    return STX_OK;
}

template <bool BWD>
int ma_masked_volume(float* flat, const float* mde_l, const float* mde_r, float* wide, int B, int N, int H, int W2, int W3,
                     void* stream, const char* what) {
    STX_REQUIRE(flat && mde_l && mde_r && wide, "%s: null pointer", what);
    if (int rc = ma_volume_ok(B, N, H, W2, W3, what)) return rc;
    const int chunks = stx_cdiv(W2, MA_ROWS);
    const dim3 grid((unsigned)((long long)B * H * chunks));
    if (W3 % 4 == 0)
        hipLaunchKernelGGL((masked_volume_kernel<BWD, true>), grid, dim3(MA_THREADS), 0, (hipStream_t)stream, flat, mde_l, mde_r, wide, N,
                           H, W2, W3, chunks);
    else
        hipLaunchKernelGGL((masked_volume_kernel<BWD, false>), grid, dim3(MA_THREADS), 0, (hipStream_t)stream, flat, mde_l, mde_r, wide,
                           N, H, W2, W3, chunks);
    return stx_check_launch(what);
}

}  // namespace

extern "C" int stx_generate_masks_fwd(const float* mde, void* masks, int B, int N, int H, int W, void* stream) {
    stx_begin();
    const char* what = "generate_masks_fwd";
    STX_REQUIRE(mde && masks, "%s: null pointer", what);
    STX_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", what, B, H, W);
    STX_REQUIRE(N >= 1 && N <= MA_MAX_N, "%s: N %d outside 1..%d", what, N, MA_MAX_N);
    const long long pixels = (long long)B * H * W;
    STX_REQUIRE(pixels * N < (1ll << 40), "%s: tensor too large", what);
    hipLaunchKernelGGL(generate_masks_kernel, dim3(ma_grid(pixels)), dim3(MA_THREADS), 0, (hipStream_t)stream, mde,
                       (unsigned short*)masks, pixels, (long long)H * W, N);
    return stx_check_launch(what);
}

extern "C" int stx_masked_volume_fwd(const float* vol, const float* mde_l, const float* mde_r, float* out, int B, int N, int H, int W2,
                                     int W3, void* stream) {
    stx_begin();
    return ma_masked_volume<false>(const_cast<float*>(vol), mde_l, mde_r, out, B, N, H, W2, W3, stream, "masked_volume_fwd");
}

extern "C" int stx_masked_volume_bwd(const float* g, const float* mde_l, const float* mde_r, float* gvol, int B, int N, int H, int W2,
                                     int W3, void* stream) {
    stx_begin();
    return ma_masked_volume<true>(gvol, mde_l, mde_r, const_cast<float*>(g), B, N, H, W2, W3, stream, "masked_volume_bwd");
}

extern "C" int stx_softlrc_fwd(const float* disp2, const float* disp3, float lrc_th, float* out2, float* out3, int B, int H, int W,
                               void* stream) {
    stx_begin();
    const char* what = "softlrc_fwd";
    STX_REQUIRE(disp2 && disp3 && out2 && out3, "%s: null pointer", what);
    if (int rc = ma_lrc_ok(B, H, W, lrc_th, what)) return rc;
    const long long pixels = (long long)B * H * W;
    hipLaunchKernelGGL(softlrc_kernel<false>, dim3(ma_grid(pixels)), dim3(MA_THREADS), 0, (hipStream_t)stream, disp2, disp3,
                       (const float*)nullptr, (const float*)nullptr, out2, out3, (double*)nullptr, pixels, H, W, (double)lrc_th,
                       1.0 / log1p(exp((double)lrc_th)));
    return stx_check_launch(what);
}

extern "C" long long stx_softlrc_bwd_workspace_floats(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 ? 8ll * B * H * W : 0;                // four planes of doubles
}

extern "C" int stx_softlrc_bwd(const float* g2, const float* g3, const float* disp2, const float* disp3, float lrc_th, void* workspace,
                               float* gdisp2, float* gdisp3, int B, int H, int W, void* stream) {
    stx_begin();
    const char* what = "softlrc_bwd";
    STX_REQUIRE(disp2 && disp3 && workspace && gdisp2 && gdisp3, "%s: null pointer", what);
    STX_REQUIRE(g2 || g3, "%s: no gradient given", what);
    STX_REQUIRE(((size_t)workspace & 7) == 0, "%s: the workspace must be 8-byte aligned", what);
    if (int rc = ma_lrc_ok(B, H, W, lrc_th, what)) return rc;
    STX_REQUIRE(W <= MA_LRC_MAX_W, "%s: W=%d above %d", what, W, MA_LRC_MAX_W);
    const long long pixels = (long long)B * H * W;
    double* ws = (double*)workspace;
    const size_t lds = 4 * (size_t)W * sizeof(double);
    if (int rc = stx_lds_require((const void*)softlrc_gather_kernel, lds, what)) return rc;
    hipLaunchKernelGGL(softlrc_kernel<true>, dim3(ma_grid(pixels)), dim3(MA_THREADS), 0, (hipStream_t)stream, disp2, disp3, g2, g3,
                       (float*)nullptr, (float*)nullptr, ws, pixels, H, W, (double)lrc_th, 1.0 / log1p(exp((double)lrc_th)));
    if (int rc = stx_check_launch(what)) return rc;
    hipLaunchKernelGGL(softlrc_gather_kernel, dim3((unsigned)(B * H)), dim3(MA_THREADS), lds, (hipStream_t)stream, disp2, disp3,
                       (const double*)ws, gdisp2, gdisp3, pixels, H, W);
    return stx_check_launch(what);
}

extern "C" int stx_weighted_lsq_fwd(const float* mde, const float* disp, const float* conf, float min_quantile, float max_quantile,
                                    float* scale, float* shift, void* stats, int B, long long n, void* stream) {
    stx_begin();
    const char* what = "weighted_lsq_fwd";
    STX_REQUIRE(mde && disp && conf && scale && shift && stats, "%s: null pointer", what);
    STX_REQUIRE(((size_t)stats & 7) == 0, "%s: stats must be 8-byte aligned", what);
    if (int rc = ma_lsq_ok(B, n, what)) return rc;
    STX_REQUIRE(min_quantile >= 0.f && min_quantile <= 1.f && max_quantile >= 0.f && max_quantile <= 1.f,
                "%s: quantiles %g / %g outside 0..1", what, (double)min_quantile, (double)max_quantile);
    // torch.quantile: rank = q (n - 1) as an fp32 product, the value interpolated between floor and ceil
    LsqRanks ranks;
    const float last = (float)(n - 1);
    volatile float r_min = min_quantile * last, r_max = max_quantile * last;   // rounded products: never fused into the fractions
    ranks.k[0] = (unsigned)r_min;
    ranks.k[1] = (unsigned)ceilf(r_min);
    ranks.k[2] = (unsigned)r_max;
    ranks.k[3] = (unsigned)ceilf(r_max);
    ranks.w_min = r_min - (float)ranks.k[0];
    ranks.w_max = r_max - (float)ranks.k[2];
    hipLaunchKernelGGL(weighted_lsq_kernel, dim3((unsigned)B), dim3(MA_LSQ_THREADS), 0, (hipStream_t)stream, mde, disp, conf, scale,
                       shift, (double*)stats, (unsigned)n, ranks);
    return stx_check_launch(what);
}

extern "C" int stx_weighted_lsq_bwd(const float* g_scale, const float* g_shift, const float* mde, const float* disp, const float* conf,
                                    const void* stats, float* g_mde, float* g_disp, float* g_conf, int B, long long n, void* stream) {
    stx_begin();
    const char* what = "weighted_lsq_bwd";
    STX_REQUIRE(mde && disp && conf && stats && g_mde && g_disp && g_conf, "%s: null pointer", what);
    STX_REQUIRE(g_scale || g_shift, "%s: no gradient given", what);
    if (int rc = ma_lsq_ok(B, n, what)) return rc;
    hipLaunchKernelGGL(weighted_lsq_bwd_kernel, dim3(ma_grid(n), (unsigned)B), dim3(MA_THREADS), 0, (hipStream_t)stream, g_scale, g_shift,
                       mde, disp, conf, (const double*)stats, g_mde, g_disp, g_conf, (unsigned)n);
    return stx_check_launch(what);
}

extern "C" int stx_mirror_detector_fwd(const float* stereo_disp, const float* mono_disp, const float* stereo_conf, const float* mono_conf,
                                       float conf_th, float step_gain, float* out, long long n, void* stream) {
    stx_begin();
    const char* what = "mirror_detector_fwd";
    STX_REQUIRE(stereo_disp && mono_disp && stereo_conf && mono_conf && out, "%s: null pointer", what);
    if (int rc = ma_map_ok(n, what)) return rc;
    hipLaunchKernelGGL(mirror_kernel<false>, dim3(ma_grid(n)), dim3(MA_THREADS), 0, (hipStream_t)stream, (const float*)nullptr, stereo_disp,
                       mono_disp, stereo_conf, mono_conf, (double)conf_th, (double)step_gain, out, MirrorGrads{}, n);
    return stx_check_launch(what);
}

extern "C" int stx_mirror_detector_bwd(const float* g_out, const float* stereo_disp, const float* mono_disp, const float* stereo_conf,
                                       const float* mono_conf, float conf_th, float step_gain, float* g_stereo_disp, float* g_mono_disp,
                                       float* g_stereo_conf, float* g_mono_conf, long long n, void* stream) {
    stx_begin();
    const char* what = "mirror_detector_bwd";
    STX_REQUIRE(g_out && stereo_disp && mono_disp && stereo_conf && mono_conf && g_stereo_disp && g_mono_disp && g_stereo_conf &&
                    g_mono_conf,
                "%s: null pointer", what);
    if (int rc = ma_map_ok(n, what)) return rc;
    hipLaunchKernelGGL(mirror_kernel<true>, dim3(ma_grid(n)), dim3(MA_THREADS), 0, (hipStream_t)stream, g_out, stereo_disp, mono_disp,
                       stereo_conf, mono_conf, (double)conf_th, (double)step_gain, (float*)nullptr,
                       MirrorGrads{g_stereo_disp, g_mono_disp, g_stereo_conf, g_mono_conf}, n);
    return stx_check_launch(what);
}

// Convex upsampling with the soft-max fused, and the trainer's sequence loss: the two steps every iteration of the iterative
// families ends with.
//
//   RAFT layout  (upsample_flow, models/RAFTStereo/raft_stereo.py:81-93, models/DEFOMStereo/defom_stereo.py; convex_upflow,
//                 models/StereoAnywhere/utils/utils.py:97-110; upsample_disp, models/SelectiveStereo/SelectiveRAFT/raft.py:72-84)
//     mask [N][9 f f][H][W], channel c = (t f + j) f + i;  flow [N][D][H][W]
//     out[n][d][f y + j][f x + i] = sum_t softmax_t(mask[n][t][j][i][y][x]) * s * flow[n][d][y + t/3 - 1][x + t%3 - 1]   (0 outside)
//   pixel layout (F.softmax(spx_pred, 1) in front of context_upsample, models/IGEVStereo/igev_stereo.py:158-166)
//     logits [B][9][4h][4w];  disp_low [B][1][h][w]
//     out[b][Y][X] = sum_t softmax_t(logits[b][t][Y][X]) * s * disp_low[b][Y/4 + t/3 - 1][X/4 + t%3 - 1]
//   The two differ only in where element (t, j, i) of cell p = y W + x lives, so one set of kernels (template PIX) serves both.
//
// Mapping.  A workgroup is 64 cells x f sub-rows: lane (p, j) = (threadIdx.x, threadIdx.y) owns the f outputs i = 0 .. f-1 of
// output row f y + j, f consecutive floats (one 16-byte store at f = 4, two at f = 8, 8 bytes at f = 2).  In the RAFT layout every
// mask plane (t, j, i) is contiguous over p, so the 9 f loads of a wave are 256-byte runs at any W; in the pixel layout a lane
// loads 9 x float4.  The nine flow taps per d are read once per lane.  No LDS in the forward, no transposition anywhere.
//
// Numerics.  The soft-max (maximum subtracted: logits of magnitude 90 are fine), the nine-term sums and the gradient algebra are
// formed in double, as allpairs.hip and selfsup_loss.hip do; results are rounded to fp32 once.
//
// Backward, no atomics, bitwise reproducible.  cvx_bwd_kernel has the forward's mapping, re-forms the soft-max from the logits
// (nothing mask-sized is saved) and writes g_mask[t] = s_t (a_t - sum_t' s_t' a_t'), a_t = sum_d g[d] * s * flow tap, every element
// once.  When the flow needs a gradient it also leaves c[n][d][t][y][x] = sum_{j, i} s_t g[d] (doubles): the sum over i in the lane,
// the sum over j through LDS in the fixed order j = 0 .. f-1.  cvx_gather_kernel then forms
// g_flow[n][d][y][x] = s * sum_t c[n][d][t][y - (t/3 - 1)][x - (t%3 - 1)] over the in-image neighbours, t ascending.
// D is walked in chunks of two (registers), one launch per chunk; the soft-max is re-formed per chunk, so D <= 2 -- every model
// here -- is one launch that forms it once.
//
// Sequence loss (trainer/trainer_torchrun.py:272-284): loss = sum_k w_k * (sum_valid smooth_l1(pred_k - gt)) / max(1, #valid),
// valid = (gt > 0) & (gt < maxdisp - 1) -- a NaN / inf gt compares false and is selected away.  The K prediction pointers and
// weights travel BY VALUE in the kernel arguments (SeqArgs): no device-side pointer table, no copy.  seq_fwd_kernel leaves one
// double partial and one integer count per workgroup, seq_final_kernel (one workgroup) combines them in a fixed order and divides on
// the device; seq_bwd_kernel writes the K gradients w_k clamp(pred_k - gt, -1, 1) g / max(1, #valid), exact zeros where excluded.
#include "stx_common.h"

namespace {

constexpr int CV_LANES = 64;          // cells per workgroup (one wave per sub-row j)
constexpr int CV_DC = 2;              // flow channels held in registers at a time
constexpr int CVG_THREADS = 256;
constexpr int SQ_THREADS = 256;
constexpr int SQ_MAX_BLOCKS = 1024;
constexpr int SQ_MAX_K = 48;          // predictions per launch (valid_iters = 32 plus the initial disparity = 33)

struct CvxShape {
    int N, D, H, W;
    double scale;
};

// element (t, j, i = 0 .. F-1) of cell (y, x), p = y W + x, of image n
template <int F, bool PIX>
__device__ __forceinline__ size_t cvx_mask_offset(const CvxShape& s, int n, int t, int j, int y, int x, size_t p) {
    const size_t HW = (size_t)s.H * s.W;
    if (PIX) return (((size_t)n * 9 + t) * (F * s.H) + (size_t)(F * y + j)) * ((size_t)F * s.W) + (size_t)F * x;
    return (((size_t)n * 9 + t) * F + j) * F * HW + p;         // + i * HW
}

// pixel layout: the lane's 9 x float4 of logits, loaded up front
__device__ __forceinline__ void cvx_load_mask_pix(const float* __restrict__ mask, const CvxShape& s, int n, int j, int y, int x,
                                                  float (&m)[9][4]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float4 v = stx_ld4(mask + cvx_mask_offset<4, true>(s, n, t, j, y, x, 0));
        m[t][0] = v.x; m[t][1] = v.y; m[t][2] = v.z; m[t][3] = v.w;
    }
}

// the nine logits of output i: out of the preloaded float4s (pixel layout), or nine coalesced loads (RAFT layout; q = the
// wave-uniform address of plane (t = 0, j, i = 0): plane (t, j, i) lies (t F F + i) H W floats further, the lane adds its cell p --
// a scalar base and a 32-bit lane offset per load, no 64-bit address per lane)
template <int F, bool PIX>
__device__ __forceinline__ void cvx_mask_column(const float (&m)[PIX ? 9 : 1][PIX ? F : 1], const float* __restrict__ q, size_t HW,
                                                unsigned p, int i, float (&mi)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) mi[t] = PIX ? m[PIX ? t : 0][PIX ? i : 0] : (q + ((size_t)t * F * F + i) * HW)[p];
}

// F consecutive floats of an output row
template <int F>
__device__ __forceinline__ void cvx_load_row(const float* __restrict__ q, float (&v)[F]) {
    if (F == 2) {
        const float2 a = *reinterpret_cast<const float2*>(q);
        v[0] = a.x; v[1] = a.y;
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) {
            const float4 a = stx_ld4(q + k);
            v[k] = a.x; v[k + 1] = a.y; v[k + 2] = a.z; v[k + 3] = a.w;
        }
    }
}

template <int F>
__device__ __forceinline__ void cvx_store_row(float* __restrict__ q, const float (&v)[F]) {
    if (F == 2) {
        *reinterpret_cast<float2*>(q) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) stx_st4(q + k, make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]));
    }
}

__device__ __forceinline__ float cvx_tap(const float* __restrict__ plane, const CvxShape& s, int y, int x, int t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    return (yy >= 0 && yy < s.H && xx >= 0 && xx < s.W) ? plane[(size_t)yy * s.W + xx] : 0.f;
}

// e[t] = exp(mi[t] - max_t mi[t]) in double; returns 1 / sum_t e[t]
__device__ __forceinline__ double cvx_softmax(const float (&mi)[9], double (&e)[9]) {
    float mx = mi[0];
#pragma unroll
    for (int t = 1; t < 9; ++t) mx = fmaxf(mx, mi[t]);
    double sum = 0.0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        e[t] = exp((double)mi[t] - (double)mx);
        sum += e[t];
    }
    return 1.0 / sum;
}

// block (CV_LANES, F), grid (cdiv(H W, CV_LANES), N)
template <int F, bool PIX>
__global__ __launch_bounds__(CV_LANES * F) void cvx_fwd_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                                float* __restrict__ out, CvxShape s, int d0) {
    const size_t HW = (size_t)s.H * s.W;
    const size_t p = (size_t)blockIdx.x * CV_LANES + threadIdx.x;
    if (p >= HW) return;
    const int j = __builtin_amdgcn_readfirstlane((int)threadIdx.y), n = (int)blockIdx.y;   // (a wave is one sub-row)
    const int y = (int)(p / s.W), x = (int)(p % s.W);
    float m[PIX ? 9 : 1][PIX ? F : 1];
    if constexpr (PIX) cvx_load_mask_pix(mask, s, n, j, y, x, m);
    const float* mq = mask + cvx_mask_offset<F, false>(s, n, 0, j, 0, 0, 0);
    {                                                           // flow channels d0, d0 + 1 (one launch per chunk: see the launchers)
        float fv[CV_DC][9];
#pragma unroll
        for (int dd = 0; dd < CV_DC; ++dd)
#pragma unroll
            for (int t = 0; t < 9; ++t) fv[dd][t] = d0 + dd < s.D ? cvx_tap(flow + ((size_t)n * s.D + d0 + dd) * HW, s, y, x, t) : 0.f;
        float o[CV_DC][F];
#pragma unroll
        for (int i = 0; i < F; ++i) {
            double e[9];
            STX_SCHED_BARRIER();                                // keeps the outputs in order in the schedule: loads of output i + 1 stay behind output i
            float mi[9];
            cvx_mask_column<F, PIX>(m, mq, HW, (unsigned)p, i, mi);
            const double inv = cvx_softmax(mi, e);
#pragma unroll
            for (int dd = 0; dd < CV_DC; ++dd) {
                double acc = 0.0;
#pragma unroll
                for (int t = 0; t < 9; ++t) acc += e[t] * (double)fv[dd][t];
                o[dd][i] = (float)(acc * inv * s.scale);
            }
        }
#pragma unroll
        for (int dd = 0; dd < CV_DC; ++dd)
            if (d0 + dd < s.D)
                cvx_store_row<F>(out + (((size_t)n * s.D + d0 + dd) * (F * s.H) + (size_t)(F * y + j)) * ((size_t)F * s.W) + (size_t)F * x, o[dd]);
    }
}

// block (CV_LANES, F), grid (cdiv(H W, CV_LANES), N).  gmask and / or coef (doubles [N][D][9][H][W]) may be null.
template <int F, bool PIX>
__global__ __launch_bounds__(CV_LANES * F) void cvx_bwd_kernel(const float* __restrict__ g, const float* __restrict__ flow,
                                                                const float* __restrict__ mask, float* __restrict__ gmask,
                                                                double* __restrict__ coef, CvxShape s, int d0) {
    __shared__ double red[F * 9 * CV_LANES];
    const size_t HW = (size_t)s.H * s.W;
    const size_t p0 = (size_t)blockIdx.x * CV_LANES + threadIdx.x;
    const bool active = p0 < HW;
    const size_t p = active ? p0 : HW - 1;                     // idle lanes shadow the last cell and write nothing
    const int lane = (int)threadIdx.x, j = __builtin_amdgcn_readfirstlane((int)threadIdx.y), n = (int)blockIdx.y;
    const int y = (int)(p / s.W), x = (int)(p % s.W);
    const size_t orow = (size_t)(F * y + j) * ((size_t)F * s.W) + (size_t)F * x, oplane = (size_t)F * s.H * F * s.W;
    float m[PIX ? 9 : 1][PIX ? F : 1];
    if constexpr (PIX) cvx_load_mask_pix(mask, s, n, j, y, x, m);
    const float* mq = mask + cvx_mask_offset<F, false>(s, n, 0, j, 0, 0, 0);
    {                                                           // flow channels d0, d0 + 1 (one launch per chunk: see the launchers)
        float fv[CV_DC][9], gv[CV_DC][F];
#pragma unroll
        for (int dd = 0; dd < CV_DC; ++dd) {
            const bool has = d0 + dd < s.D;
#pragma unroll
            for (int t = 0; t < 9; ++t) fv[dd][t] = has ? cvx_tap(flow + ((size_t)n * s.D + d0 + dd) * HW, s, y, x, t) : 0.f;
            if (has) {
                cvx_load_row<F>(g + ((size_t)n * s.D + d0 + dd) * oplane + orow, gv[dd]);
            } else {
#pragma unroll
                for (int i = 0; i < F; ++i) gv[dd][i] = 0.f;
            }
        }
        double c[CV_DC][9];
#pragma unroll
        for (int dd = 0; dd < CV_DC; ++dd)
#pragma unroll
            for (int t = 0; t < 9; ++t) c[dd][t] = 0.0;
        float gm[PIX ? 9 : 1][F];
#pragma unroll
        for (int i = 0; i < F; ++i) {
            double e[9];
            STX_SCHED_BARRIER();                                // keeps the outputs in order in the schedule: loads of output i + 1 stay behind output i
            float mi[9];
            cvx_mask_column<F, PIX>(m, mq, HW, (unsigned)p, i, mi);
            const double inv = cvx_softmax(mi, e);
#pragma unroll
            for (int t = 0; t < 9; ++t) e[t] *= inv;            // s_t
            if (d0 == 0 && gmask) {
                double a[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    a[t] = 0.0;
#pragma unroll
                    for (int dd = 0; dd < CV_DC; ++dd) a[t] += (double)gv[dd][i] * (double)fv[dd][t];
                }
                for (int d = CV_DC; d < s.D; ++d) {            // channels beyond the register chunk (D > 2): plain loads
                    const double gd = (double)g[((size_t)n * s.D + d) * oplane + orow + i];
                    for (int t = 0; t < 9; ++t) a[t] += gd * (double)cvx_tap(flow + ((size_t)n * s.D + d) * HW, s, y, x, t);
                }
                double dot = 0.0;
#pragma unroll
                for (int t = 0; t < 9; ++t) dot += e[t] * a[t];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const float v = (float)(e[t] * (a[t] - dot) * s.scale);
                    if (PIX) {
                        gm[PIX ? t : 0][i] = v;
                    } else if (active) {
                        gmask[cvx_mask_offset<F, PIX>(s, n, t, j, y, x, p) + (size_t)i * HW] = v;
                    }
                }
            }
#pragma unroll
            for (int dd = 0; dd < CV_DC; ++dd)
#pragma unroll
                for (int t = 0; t < 9; ++t) c[dd][t] += e[t] * (double)gv[dd][i];
        }
        if (PIX && d0 == 0 && gmask && active) {
#pragma unroll
            for (int t = 0; t < 9; ++t) cvx_store_row<F>(gmask + cvx_mask_offset<F, PIX>(s, n, t, j, y, x, p), gm[PIX ? t : 0]);
        }
        if (coef) {
#pragma unroll
            for (int dd = 0; dd < CV_DC; ++dd) {
                if (d0 + dd >= s.D) break;                     // (uniform over the workgroup)
#pragma unroll
                for (int t = 0; t < 9; ++t) red[(j * 9 + t) * CV_LANES + lane] = c[dd][t];
                __syncthreads();
                for (int t = j; t < 9; t += F) {               // the sum over the sub-rows, j = 0 .. F-1 in this order
                    double sum = 0.0;
                    for (int jj = 0; jj < F; ++jj) sum += red[(jj * 9 + t) * CV_LANES + lane];
                    if (active) coef[(((size_t)n * s.D + d0 + dd) * 9 + t) * HW + p] = sum;
                }
                __syncthreads();
            }
        }
    }
}

// one lane per element of g_flow
__global__ __launch_bounds__(CVG_THREADS) void cvx_gather_kernel(const double* __restrict__ coef, float* __restrict__ gflow, CvxShape s) {
    const size_t HW = (size_t)s.H * s.W;
    const size_t idx = (size_t)blockIdx.x * CVG_THREADS + threadIdx.x;
    if (idx >= (size_t)s.N * s.D * HW) return;
    const size_t nd = idx / HW, p = idx % HW;
    const int y = (int)(p / s.W), x = (int)(p % s.W);
    double sum = 0.0;
    for (int t = 0; t < 9; ++t) {
        const int cy = y - (t / 3 - 1), cx = x - (t % 3 - 1);
        if (cy >= 0 && cy < s.H && cx >= 0 && cx < s.W) sum += coef[(nd * 9 + t) * HW + (size_t)cy * s.W + cx];
    }
    gflow[idx] = (float)(sum * s.scale);
}

// ------------------------------------------------------------------------------------------------ sequence loss
struct SeqArgs {
    const float* pred[SQ_MAX_K];
    double w[SQ_MAX_K];
};
struct SeqGrads {
    float* g[SQ_MAX_K];
};

__device__ __forceinline__ bool seq_valid(float gt, float hi) { return gt > 0.f && gt < hi; }

// grid nblk (<= SQ_MAX_BLOCKS): psum[nblk] doubles, pcnt[nblk] ints
__global__ __launch_bounds__(SQ_THREADS) void seq_fwd_kernel(SeqArgs a, int K, const float* __restrict__ gt, float hi, long long n,
                                                             double* __restrict__ psum, int* __restrict__ pcnt) {
    __shared__ double red[SQ_THREADS];
    __shared__ int redc[SQ_THREADS];
    double acc = 0.0;
    int cnt = 0;
    const long long step = (long long)gridDim.x * SQ_THREADS;
    for (long long i = (long long)blockIdx.x * SQ_THREADS + threadIdx.x; i < n; i += step) {
        const float t = gt[i];
        if (!seq_valid(t, hi)) continue;
        ++cnt;
        double px = 0.0;
        for (int k = 0; k < K; ++k) {
            const double d = fabs((double)a.pred[k][i] - (double)t);
            px += a.w[k] * (d < 1.0 ? 0.5 * d * d : d - 0.5);
        }
        acc += px;
    }
    red[threadIdx.x] = acc;
    redc[threadIdx.x] = cnt;
    __syncthreads();
    for (int h = SQ_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[threadIdx.x] += red[threadIdx.x + h];
            redc[threadIdx.x] += redc[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = red[0];
        pcnt[blockIdx.x] = redc[0];
    }
}

// one workgroup: loss[0] = sum / max(1, count), count[0] = the number of valid pixels
__global__ __launch_bounds__(SQ_THREADS) void seq_final_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt, int nblk,
                                                               float* __restrict__ loss, int* __restrict__ count) {
    __shared__ double red[SQ_THREADS];
    __shared__ int redc[SQ_THREADS];
    double acc = 0.0;
    int cnt = 0;
    for (int k = threadIdx.x; k < nblk; k += SQ_THREADS) {
        acc += psum[k];
        cnt += pcnt[k];
    }
    red[threadIdx.x] = acc;
    redc[threadIdx.x] = cnt;
    __syncthreads();
    for (int h = SQ_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[threadIdx.x] += red[threadIdx.x + h];
            redc[threadIdx.x] += redc[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(red[0] / (double)(redc[0] > 1 ? redc[0] : 1));
        count[0] = redc[0];
    }
}

__global__ __launch_bounds__(SQ_THREADS) void seq_bwd_kernel(SeqArgs a, SeqGrads o, int K, const float* __restrict__ gt, float hi,
                                                             long long n, const float* __restrict__ gloss, const int* __restrict__ count) {
    const long long i = (long long)blockIdx.x * SQ_THREADS + threadIdx.x;
    if (i >= n) return;
    const int cnt = count[0];
    const double f = (double)gloss[0] / (double)(cnt > 1 ? cnt : 1);
    const float t = gt[i];
    const bool ok = seq_valid(t, hi);
    for (int k = 0; k < K; ++k) {
        if (o.g[k] == nullptr) continue;
        float v = 0.f;
        if (ok) {
            const double d = (double)a.pred[k][i] - (double)t;
            v = (float)(a.w[k] * (d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d)) * f);
        }
        o.g[k][i] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline bool cvx_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

int cvx_shape(CvxShape& s, int N, int D, int H, int W, int f, float scale, const char* what) {
    STX_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && N < 65536, "%s: bad shape N=%d D=%d H=%d W=%d", what, N, D, H, W);
    STX_REQUIRE(f == 2 || f == 4 || f == 8, "%s: factor %d is not one of 2, 4, 8", what, f);
    STX_REQUIRE((long long)N * (D > 9 ? D : 9) * f * f * H * (long long)W < (1ll << 40), "%s: tensor too large", what);
    STX_REQUIRE((long long)H * W < (1ll << 30), "%s: too many cells", what);
    s.N = N; s.D = D; s.H = H; s.W = W;
    s.scale = (double)scale;
    return STX_OK;
}

template <bool PIX>
int cvx_fwd_launch(const float* flow, const float* mask, float* out, const CvxShape& s, int f, void* stream, const char* what) {
    const dim3 grid((unsigned)(((long long)s.H * s.W + CV_LANES - 1) / CV_LANES), s.N), block(CV_LANES, f);
    for (int d0 = 0; d0 < s.D; d0 += CV_DC) {
        if (f == 2) hipLaunchKernelGGL((cvx_fwd_kernel<2, false>), grid, block, 0, (hipStream_t)stream, flow, mask, out, s, d0);
        else if (f == 4) hipLaunchKernelGGL((cvx_fwd_kernel<4, PIX>), grid, block, 0, (hipStream_t)stream, flow, mask, out, s, d0);
        else hipLaunchKernelGGL((cvx_fwd_kernel<8, false>), grid, block, 0, (hipStream_t)stream, flow, mask, out, s, d0);
        if (int rc = stx_check_launch(what)) return rc;
    }
    return STX_OK;
}

template <bool PIX>
int cvx_bwd_launch(const float* g, const float* flow, const float* mask, float* gflow, float* gmask, double* coef, const CvxShape& s,
                   int f, void* stream, const char* what) {
    const dim3 grid((unsigned)(((long long)s.H * s.W + CV_LANES - 1) / CV_LANES), s.N), block(CV_LANES, f);
    double* cf = gflow ? coef : nullptr;
    for (int d0 = 0; d0 < (cf ? s.D : 1); d0 += CV_DC) {       // the mask's gradient comes out of the first launch
        if (f == 2) hipLaunchKernelGGL((cvx_bwd_kernel<2, false>), grid, block, 0, (hipStream_t)stream, g, flow, mask, gmask, cf, s, d0);
        else if (f == 4) hipLaunchKernelGGL((cvx_bwd_kernel<4, PIX>), grid, block, 0, (hipStream_t)stream, g, flow, mask, gmask, cf, s, d0);
        else hipLaunchKernelGGL((cvx_bwd_kernel<8, false>), grid, block, 0, (hipStream_t)stream, g, flow, mask, gmask, cf, s, d0);
        if (int rc = stx_check_launch(what)) return rc;
    }
    if (gflow) {
        const long long m = (long long)s.N * s.D * s.H * s.W;
        hipLaunchKernelGGL(cvx_gather_kernel, dim3((unsigned)((m + CVG_THREADS - 1) / CVG_THREADS)), dim3(CVG_THREADS), 0,
                           (hipStream_t)stream, (const double*)coef, gflow, s);
        if (int rc = stx_check_launch(what)) return rc;
    }
    return STX_OK;
}

int seq_args(SeqArgs& a, const float* const* preds, const double* weights, int K, const float* gt, long long n, const char* what) {
    STX_REQUIRE(preds && weights && gt, "%s: null pointer", what);
    STX_REQUIRE(K >= 1 && K <= SQ_MAX_K, "%s: %d predictions outside 1..%d", what, K, SQ_MAX_K);
    STX_REQUIRE(n > 0 && n < (1ll << 31), "%s: %lld pixels outside 1..2^31-1", what, n);
    for (int k = 0; k < SQ_MAX_K; ++k) {
        a.pred[k] = k < K ? preds[k] : nullptr;
        a.w[k] = k < K ? weights[k] : 0.0;
        STX_REQUIRE(k >= K || preds[k], "%s: prediction %d is a null pointer", what, k);
    }
    return STX_OK;
}

int seq_blocks(long long n) {
    const long long b = (n + SQ_THREADS - 1) / SQ_THREADS;
    return (int)(b < SQ_MAX_BLOCKS ? b : SQ_MAX_BLOCKS);
}

}  // namespace

extern "C" long long stx_convex_upsample_bwd_workspace_floats(int N, int D, int H, int W) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return 2ll * N * D * 9 * H * W;                            // the tap coefficients, doubles
}

extern "C" int stx_convex_upsample_fwd(const float* flow, const float* mask, float* out, int N, int D, int H, int W, int mask_channels,
                                       int f, float scale, void* stream) {
    stx_begin();
    const char* what = "convex_upsample_fwd";
    STX_REQUIRE(flow && mask && out, "%s: null pointer", what);
    CvxShape s;
    if (int rc = cvx_shape(s, N, D, H, W, f, scale, what)) return rc;
    STX_REQUIRE(mask_channels == 9 * f * f, "%s: mask has %d channels, factor %d wants %d", what, mask_channels, f, 9 * f * f);
    STX_REQUIRE(cvx_aligned(out), "%s: out must be 16-byte aligned", what);
    return cvx_fwd_launch<false>(flow, mask, out, s, f, stream, what);
}

extern "C" int stx_convex_upsample_bwd(const float* g, const float* flow, const float* mask, float* gflow, float* gmask,
                                       float* workspace, int N, int D, int H, int W, int mask_channels, int f, float scale,
                                       void* stream) {
    stx_begin();
    const char* what = "convex_upsample_bwd";
    STX_REQUIRE(g && flow && mask && (gflow || gmask), "%s: null pointer", what);
    CvxShape s;
    if (int rc = cvx_shape(s, N, D, H, W, f, scale, what)) return rc;
    STX_REQUIRE(mask_channels == 9 * f * f, "%s: mask has %d channels, factor %d wants %d", what, mask_channels, f, 9 * f * f);
    STX_REQUIRE(!gflow || (workspace && ((uintptr_t)workspace & 7) == 0), "%s: g_flow needs the 8-byte aligned workspace", what);
    STX_REQUIRE(cvx_aligned(g), "%s: g must be 16-byte aligned", what);
    return cvx_bwd_launch<false>(g, flow, mask, gflow, gmask, reinterpret_cast<double*>(workspace), s, f, stream, what);
}

extern "C" int stx_softmax_context_upsample_fwd(const float* disp_low, const float* logits, float* out, int B, int h, int w, float scale,
                                                void* stream) {
    stx_begin();
    const char* what = "softmax_context_upsample_fwd";
    STX_REQUIRE(disp_low && logits && out, "%s: null pointer", what);
    CvxShape s;
    if (int rc = cvx_shape(s, B, 1, h, w, 4, scale, what)) return rc;
    STX_REQUIRE(cvx_aligned(out) && cvx_aligned(logits), "%s: logits and out must be 16-byte aligned", what);
    return cvx_fwd_launch<true>(disp_low, logits, out, s, 4, stream, what);
}

extern "C" int stx_softmax_context_upsample_bwd(const float* g, const float* disp_low, const float* logits, float* gdisp, float* glogits,
                                                float* workspace, int B, int h, int w, float scale, void* stream) {
    stx_begin();
    const char* what = "softmax_context_upsample_bwd";
    STX_REQUIRE(g && disp_low && logits && (gdisp || glogits), "%s: null pointer", what);
    CvxShape s;
    if (int rc = cvx_shape(s, B, 1, h, w, 4, scale, what)) return rc;
    STX_REQUIRE(!gdisp || (workspace && ((uintptr_t)workspace & 7) == 0), "%s: g_disp needs the 8-byte aligned workspace", what);
    STX_REQUIRE(cvx_aligned(g) && cvx_aligned(logits) && cvx_aligned(glogits), "%s: g, logits and g_logits must be 16-byte aligned", what);
    return cvx_bwd_launch<true>(g, disp_low, logits, gdisp, glogits, reinterpret_cast<double*>(workspace), s, 4, stream, what);
}

extern "C" int stx_sequence_loss_max_predictions() { return SQ_MAX_K; }

extern "C" long long stx_sequence_loss_workspace_floats(long long n) {
    if (n <= 0 || n >= (1ll << 31)) return 0;
    return 3ll * seq_blocks(n);                                // per workgroup one double and one int
}

extern "C" int stx_sequence_loss_fwd(const float* const* preds, const double* weights, int K, const float* gt, float maxdisp, float* loss,
                                     int* count, float* workspace, long long n, void* stream) {
    stx_begin();
    const char* what = "sequence_loss_fwd";
    SeqArgs a;
    if (int rc = seq_args(a, preds, weights, K, gt, n, what)) return rc;
    STX_REQUIRE(loss && count && workspace && ((uintptr_t)workspace & 7) == 0, "%s: loss, count and the 8-byte aligned workspace", what);
    const int nblk = seq_blocks(n);
    double* psum = reinterpret_cast<double*>(workspace);
    int* pcnt = reinterpret_cast<int*>(psum + nblk);
    hipLaunchKernelGGL(seq_fwd_kernel, dim3(nblk), dim3(SQ_THREADS), 0, (hipStream_t)stream, a, K, gt, maxdisp - 1.f, n, psum, pcnt);
    if (int rc = stx_check_launch(what)) return rc;
    hipLaunchKernelGGL(seq_final_kernel, dim3(1), dim3(SQ_THREADS), 0, (hipStream_t)stream, (const double*)psum, (const int*)pcnt, nblk,
                       loss, count);
    return stx_check_launch(what);
}

extern "C" int stx_sequence_loss_bwd(const float* gloss, const float* const* preds, const double* weights, int K, const float* gt,
                                     float maxdisp, const int* count, float* const* gpreds, long long n, void* stream) {
    stx_begin();
    const char* what = "sequence_loss_bwd";
    SeqArgs a;
    if (int rc = seq_args(a, preds, weights, K, gt, n, what)) return rc;
    STX_REQUIRE(gloss && count && gpreds, "%s: null pointer", what);
    SeqGrads o;
    bool any = false;
    for (int k = 0; k < SQ_MAX_K; ++k) {
        o.g[k] = k < K ? gpreds[k] : nullptr;
        any = any || o.g[k];
    }
    STX_REQUIRE(any, "%s: no gradient asked for", what);
    hipLaunchKernelGGL(seq_bwd_kernel, dim3((unsigned)((n + SQ_THREADS - 1) / SQ_THREADS)), dim3(SQ_THREADS), 0, (hipStream_t)stream, a, o,
                       K, gt, maxdisp - 1.f, n, gloss, count);
    return stx_check_launch(what);
}

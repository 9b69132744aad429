// STTR's matching head (reference models/STTR/regression_head.py) on the raw cross-attention attn[N][H][W][W] (left position i,
// right position j; -inf where j > i):
//   * S = attn with a dustbin row and column holding phi, M = W + 1;
//   * OT mode: `iters` log-space Sinkhorn iterations per image row (u_0 = 0, log mu = log nu = log([1..1, W] / 2W)),
//       v_k[j] = log nu[j] - LSE_i(S_ij + u_{k-1}[i]),   u_k[i] = log mu[i] - LSE_j(S_ij + v_k[j]),
//     transported matrix P_ij = exp(S_ij + u_K[i] + v_K[j] + log 2W);  softmax mode: P = row softmax of S;
//   * the regression on P[:W, :W]: first arg-max m over j, the window {m-1, m, m+1} (0 outside [0, W)), norm = its sum (forced
//     to 1 -- a constant -- where the occlusion mask is set or, without a mask, where it is below 0.1),
//     disp = sum P_j max(i - j, 0) / norm, occ = 1 - norm, the response at the ground-truth location (linear between the
//     clamped floor and ceil of `target`, weight_r = target - clamped floor) and the dustbin responses P[:W, W], P[W, :W].
// Stock that is 20 matrix-sized temporaries kept for autograd plus the cats, the exp, a padded copy and three gathers.  Here
// nothing matrix-sized is written by the fused head: the forward keeps the 2 * iters scaling vectors, the backward re-forms
// every exponential from them.
//
// Layout.  ONE workgroup owns one (n, h) matrix and reads it from L2 / Infinity Cache once per half-iteration (at W = 320 the
// matrix is 412 KB: it does not fit the LDS); lanes always run along j, so both directions are coalesced:
//   LSE_j  one wave per matrix row, the row (M <= 432) in seven (double) registers per lane: max and sum are wave reductions of ONE read;
//   LSE_i  lanes along the columns of a 64-column strip, the waves interleaved down the rows, a running (max, sum) per lane;
//          the waves' partial results are combined through LDS in wave order.
// Precision.  Exponents and sums are formed in double -- u and v are kept and saved as doubles -- and each exponential is one
// fp32 expf of the rounded exponent times (1 + the rounding's remainder): the 1e-6 that rounding an exponent of size 16 to
// fp32 costs is gone, what is left is expf's own error; the entries of P themselves (once per element) take a double exp.
// Nothing uses float atomics: every result is bitwise reproducible.
//
// Backward (unrolled like autograd through the iterations).  With G = dL/dP and Gamma = G o P:
//   gu = sum_j Gamma, gv = sum_i Gamma;  for k = K..1:  a_k = gu;  gv[j] -= sum_i gu[i] R_ij,  R = exp(S + v_k[j] + u_k[i] - log mu[i]);
//   b_k = gv;  gu[i] = -sum_j gv[j] C_ij,  C = exp(S + u_{k-1}[i] + v_k[j] - log nu[j]);  gv = 0
// -- 2K read-only matrix-vector passes -- and then ONE pass that writes gS = Gamma - sum_k (a_k[i] R^k_ij + b_k[j] C^k_ij):
// g_attn = gS[:W, :W] written once, g_phi = the sum of gS over the dustbin row and column, one partial per (n, h), added up in a
// fixed order by a one-workgroup kernel.  The fused head's Gamma has at most five entries per row (the window and the two
// ground-truth taps) plus the dustbins: it lives in LDS; the dense pair takes a dense G.  Softmax mode: gS = Gamma - P gu.
#include "stx_common.h"

namespace {

constexpr int ST_MAX_W = 431;          // M = W + 1 <= 432: the backward's vectors of 10 iterations fit the LDS (st_bwd_lds_floats)
constexpr int ST_REGS = 7;             // a matrix row in ST_REGS registers per lane
constexpr int ST_MAX_ITERS = 10;
constexpr int ST_SLOTS = 5;            // sparse Gamma entries per row: the window (3) and the ground-truth taps (2)
constexpr int ST_SMALL_M = 128;        // up to this M a workgroup has 256 threads, above it 1024
constexpr float ST_NEG = -3.402823466e38f;
constexpr int ST_FORCED = 1 << 16;     // bit of `arg`: norm was forced to 1

__device__ __forceinline__ float st_ninf() { return -__builtin_huge_valf(); }

__device__ __forceinline__ float st_wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// butterfly sum of a double through two fp32 shuffles (hi + lo carries 48 bits); every lane ends with the same bits
__device__ __forceinline__ double st_wave_sum(double x) {
    for (int off = 32; off > 0; off >>= 1) {
        const float hi = (float)x, lo = (float)(x - (double)hi);
        const float ohi = __shfl_xor(hi, off), olo = __shfl_xor(lo, off);
        x = ((double)hi + (double)lo) + ((double)ohi + (double)olo);
    }
    return x;
}

// exp(x) for a double x: expf of x rounded to fp32, corrected by the remainder of that rounding (|lo| <= 2^-24 |x|)
__device__ __forceinline__ float st_exp(double x) {
    const float hi = (float)x;
    const float lo = hi > ST_NEG ? (float)(x - (double)hi) : 0.f;        // (x = -inf: exp = 0, no inf - inf)
    return expf(hi) * (1.f + lo);
}

// one (n, h) matrix: S_ij and the marginals
struct StMat {
    const float* attn;                 // [W][W]
    float phi;
    int W, M, mode;                    // mode 1 = optimal transport, 0 = softmax
    float log_one, log_bin, log_2w;    // log(1 / 2W), log(W / 2W), log(2W): fp32 values formed on the host
    __device__ __forceinline__ float s(int i, int j) const { return (i < W && j < W) ? attn[(size_t)i * W + j] : phi; }
    __device__ __forceinline__ double lm(int i) const { return (double)(i < W ? log_one : log_bin); }   // log mu = log nu
    // P_ij.  OT: a = u_K (by row), b = v_K (by column).  Softmax: a = the row max, b = the row sum, both by row.  A double exp,
    // rounded once: the reference's fp32 error on the largest entries (the dustbin corner, ~W / 2) is one ulp, and expf alone costs that.
    __device__ __forceinline__ float p(int i, int j, const double* a, const double* b) const {
        const double x = (double)s(i, j);
        return (float)(mode ? exp(((x + a[i]) + b[j]) + (double)log_2w) : exp(x - a[i]) / b[i]);
    }
};

// LSE_j(S_ij + v[j]) of row i as (max, sum of exp(. - max)); v NULL = 0.  Called by a whole wave.
__device__ __forceinline__ void st_row_lse(const StMat& q, int i, const double* v, int lane, float& m, double& acc) {
    double x[ST_REGS];
    m = ST_NEG;
#pragma unroll
    for (int k = 0; k < ST_REGS; ++k) {
        const int j = 64 * k + lane;
        x[k] = (double)st_ninf();
        if (j < q.M) x[k] = (double)q.s(i, j) + (v ? v[j] : 0.0);
        m = fmaxf(m, (float)x[k]);
    }
    m = st_wave_max(m);                                                  // finite: the dustbin entry is.  (Any common shift near the max serves.)
    acc = 0.0;
#pragma unroll
    for (int k = 0; k < ST_REGS; ++k) acc += (double)st_exp(x[k] - (double)m);   // exp(-inf) = 0: masked entries and the row's tail
    acc = st_wave_sum(acc);
}

// a running (max, sum): x = -inf adds nothing, also while m is still ST_NEG
__device__ __forceinline__ void st_online(double x, double& m, double& acc) {
    if (x > m) {
        acc *= (double)st_exp(m - x);
        m = x;
    }
    acc += (double)st_exp(x - m);
}

// v[j] = log nu[j] - LSE_i(S_ij + u[i]) for every column; pm / ps [nwaves][M] partial (max, sum).  Called by the workgroup;
// ends with a barrier.  `save` (NULL or [M]) receives a copy.
__device__ void st_col_step(const StMat& q, const double* u, double* v, double* pm, double* ps, double* save) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6, M = q.M;
    for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        if (j >= M) continue;
        double m = (double)ST_NEG;
        double acc = 0.0;
        int i = wave;
        for (; i + 3 * nwaves < M; i += 4 * nwaves) {                    // four loads in flight
            const double x0 = (double)q.s(i, j) + u[i], x1 = (double)q.s(i + nwaves, j) + u[i + nwaves];
            const double x2 = (double)q.s(i + 2 * nwaves, j) + u[i + 2 * nwaves], x3 = (double)q.s(i + 3 * nwaves, j) + u[i + 3 * nwaves];
            st_online(x0, m, acc);
            st_online(x1, m, acc);
            st_online(x2, m, acc);
            st_online(x3, m, acc);
        }
        for (; i < M; i += nwaves) st_online((double)q.s(i, j) + u[i], m, acc);
        pm[wave * M + j] = m;
        ps[wave * M + j] = acc;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < M; j += blockDim.x) {
        double m = (double)ST_NEG;
        for (int w = 0; w < nwaves; ++w) m = fmax(m, pm[w * M + j]);
        double acc = 0.0;
        for (int w = 0; w < nwaves; ++w) acc += ps[w * M + j] * (double)st_exp(pm[w * M + j] - m);   // (a wave without rows: 0)
        const double r = q.lm(j) - (m + log(acc));
        v[j] = r;
        if (save) save[j] = r;
    }
    __syncthreads();
}

// u[i] = log mu[i] - LSE_j(S_ij + v[j]) for every row; ends with a barrier
__device__ void st_row_step(const StMat& q, double* u, const double* v, double* save) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int i = wave; i < q.M; i += nwaves) {
        float m;
        double acc;
        st_row_lse(q, i, v, lane, m, acc);
        if (lane == 0) {
            const double r = q.lm(i) - ((double)m + log(acc));
            u[i] = r;
            if (save) save[i] = r;
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ forward
struct StFwd {
    const float *attn, *phi;
    int W, iters, mode;
    float log_one, log_bin, log_2w;
    double *us, *vs;                   // OT: [NH][iters][M] each; softmax: row max / row sum [NH][M]; NULL = not kept
    float* P;                          // dense [NH][M][M] or NULL
    // the fused head (disp NULL = not run): outputs [NH][W]
    const unsigned char* mask;         // NULL = the 0.1 threshold
    const float* target;               // NULL = no gt_response
    float *disp, *occ, *norm, *gt, *bin_l, *bin_r;
    int* arg;
};

// grid N*H; dynamic LDS st_fwd_lds(M, nwaves)
__global__ __launch_bounds__(1024) void sttr_fwd_kernel(StFwd a) {
    STX_DYN_SMEM(smem);
    const int W = a.W, M = W + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    double* ps = reinterpret_cast<double*>(smem);
    double* pm = ps + (size_t)nwaves * M;
    double* u = pm + (size_t)nwaves * M;
    double* v = u + M;
    const size_t nh = blockIdx.x;
    const StMat q{a.attn + nh * (size_t)W * W, *a.phi, W, M, a.mode, a.log_one, a.log_bin, a.log_2w};
    if (a.mode) {
        for (int j = threadIdx.x; j < M; j += blockDim.x) u[j] = 0.0;
        __syncthreads();
        for (int k = 0; k < a.iters; ++k) {
            const size_t at = (nh * a.iters + k) * (size_t)M;
            st_col_step(q, u, v, pm, ps, a.vs ? a.vs + at : nullptr);
            st_row_step(q, u, v, a.us ? a.us + at : nullptr);
        }
    } else {
        for (int i = wave; i < M; i += nwaves) {
            float m;
            double acc;
            st_row_lse(q, i, nullptr, lane, m, acc);
            if (lane == 0) {
                u[i] = (double)m;
                v[i] = acc;
                if (a.us) a.us[nh * M + i] = (double)m;
                if (a.vs) a.vs[nh * M + i] = acc;
            }
        }
        __syncthreads();
    }
    for (int i = wave; i < M; i += nwaves) {
        if (a.P) {
            float* row = a.P + (nh * M + i) * (size_t)M;
            for (int j = lane; j < M; j += 64) row[j] = q.p(i, j, u, v);
        }
        if (!a.disp) continue;
        if (i == W) {                                                    // the dustbin row
            for (int j = lane; j < W; j += 64) a.bin_r[nh * W + j] = q.p(W, j, u, v);
            continue;
        }
        // first arg-max over j < W
        float best = -1.f, bidx = 0.f;
        for (int j = lane; j < W; j += 64) {
            const float pj = q.p(i, j, u, v);
            if (pj > best) {
                best = pj;
                bidx = (float)j;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off), oi = __shfl_xor(bidx, off);
            if (ob > best || (ob == best && oi < bidx)) {
                best = ob;
                bidx = oi;
            }
        }
        const int am = (int)bidx;
        // lanes 0..2 the window, 3..4 the ground-truth taps, 5 the dustbin column
        const size_t r = nh * W + i;
        const float t = a.target ? a.target[r] : 0.f;
        const float hi = (float)(W - 1);
        const int il = (int)fminf(fmaxf(floorf(t), 0.f), hi), ir = (int)fminf(fmaxf(ceilf(t), 0.f), hi);
        int col = -1;
        if (lane < 3) col = am - 1 + lane;
        if (lane == 3) col = il;
        if (lane == 4) col = ir;
        if (lane == 5) col = W;
        float pv = 0.f;
        if (col >= 0 && (col < W || lane == 5) && (a.target || lane < 3 || lane == 5)) pv = q.p(i, col, u, v);
        const float p0 = __shfl(pv, 0), p1 = __shfl(pv, 1), p2 = __shfl(pv, 2), pl = __shfl(pv, 3), pr = __shfl(pv, 4);
        if (lane == 5) a.bin_l[r] = pv;
        if (lane == 0) {
            const double raw = ((double)p0 + (double)p1) + (double)p2;
            const bool forced = a.mask ? a.mask[r] != 0 : (float)raw < 0.1f;
            const double n = forced ? 1.0 : raw;
            const double s0 = (double)(i - (am - 1) > 0 ? i - (am - 1) : 0), s1 = (double)(i - am > 0 ? i - am : 0),
                         s2 = (double)(i - (am + 1) > 0 ? i - (am + 1) : 0);
            a.disp[r] = (float)(((double)p0 * s0 + (double)p1 * s1 + (double)p2 * s2) / n);
            a.occ[r] = (float)(1.0 - n);
            a.norm[r] = (float)n;
            a.arg[r] = am | (forced ? ST_FORCED : 0);
            if (a.target) {
                const double wr = (double)t - (double)il;
                a.gt[r] = (float)((double)pl * (1.0 - wr) + (double)pr * wr);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
struct StBwd {
    const float *attn, *phi;
    const double *us, *vs;
    int W, iters, mode;
    float log_one, log_bin, log_2w;
    // the fused head: gradients [NH][W] (any may be NULL) and what the forward gave
    const float *g_disp, *g_occ, *g_gt, *g_bin_l, *g_bin_r;
    const float *disp, *norm, *target;
    const int* arg;
    const float* G;                    // the dense pair: [NH][M][M]
    float* g_attn;                     // [NH][W][W]
    double* phi_part;                  // [NH]
};

// LDS of the backward: the doubles U [(K+1)][M] (u_0 = 0 first), V [K][M] (softmax: K = 0 and U = row max, V = row sum, one row
// each), then the floats A [K][M], B [K][M], gu [M], gv [M], part [nwaves][M], then the sparse Gamma: sval [SLOTS][M], dl [M],
// dr [M], scol (int) [SLOTS][M].  92 M floats for 10 iterations and 16 waves: M <= 432.
struct StLds {
    double *U, *V;
    float *A, *B, *gu, *gv, *part, *sval, *dl, *dr;
    int* scol;
};

__host__ __device__ inline size_t st_bwd_lds_floats(int M, int K, int nwaves, bool dense) {
    return (size_t)M * ((K ? 6 * K + 2 : 4) + 2 + nwaves + (dense ? 0 : 2 * ST_SLOTS + 2)) + 2 * 64;
}

template <bool DENSE>
struct StGamma {
    const StMat& q;
    const StLds& l;
    const double *a, *b;               // the arguments of q.p
    const float* G;                    // this matrix's dense gradient
    // Gamma_ij; the sparse form sums the row's slots in slot order
    __device__ __forceinline__ float at(int i, int j) const {
        if (DENSE) return G[(size_t)i * q.M + j] * q.p(i, j, a, b);
        if (i == q.W) return j < q.W ? l.dr[j] : 0.f;
        if (j == q.W) return l.dl[i];
        float g = 0.f;
#pragma unroll
        for (int s = 0; s < ST_SLOTS; ++s) g += l.scol[s * q.M + i] == j ? l.sval[s * q.M + i] : 0.f;
        return g;
    }
};

// grid N*H
template <bool DENSE>
__global__ __launch_bounds__(1024) void sttr_bwd_kernel(StBwd a) {
    STX_DYN_SMEM(smem);
    const int W = a.W, M = W + 1, K = a.mode ? a.iters : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const size_t nh = blockIdx.x;
    const StMat q{a.attn + nh * (size_t)W * W, *a.phi, W, M, a.mode, a.log_one, a.log_bin, a.log_2w};
    double* wsum = reinterpret_cast<double*>(smem);                      // [64] (16 used)
    StLds l;
    l.U = wsum + 64;
    l.V = l.U + (size_t)(K ? K + 1 : 1) * M;
    l.A = reinterpret_cast<float*>(l.V + (size_t)(K ? K : 1) * M);
    l.B = l.A + (size_t)K * M;
    l.gu = l.B + (size_t)K * M;
    l.gv = l.gu + M;
    l.part = l.gv + M;
    l.sval = l.part + (size_t)nwaves * M;
    l.dl = l.sval + (size_t)ST_SLOTS * M;
    l.dr = l.dl + M;
    l.scol = reinterpret_cast<int*>(l.dr + M);
    // the scaling vectors
    if (K) {
        for (int j = threadIdx.x; j < M; j += blockDim.x) l.U[j] = 0.0;
        for (int e = threadIdx.x; e < K * M; e += blockDim.x) {
            l.U[M + e] = a.us[nh * (size_t)K * M + e];
            l.V[e] = a.vs[nh * (size_t)K * M + e];
        }
    } else {
        for (int j = threadIdx.x; j < M; j += blockDim.x) {
            l.U[j] = a.us[nh * M + j];
            l.V[j] = a.vs[nh * M + j];
        }
    }
    __syncthreads();
    const double* pa = l.U + (size_t)K * M;                              // u_K | row max
    const double* pb = K ? l.V + (size_t)(K - 1) * M : l.V;               // v_K | row sum
    const StGamma<DENSE> gam{q, l, pa, pb, DENSE ? a.G + nh * (size_t)M * M : nullptr};
    if (!DENSE) {
        // the sparse Gamma of the fused head: G times P, entry by entry
        for (int i = threadIdx.x; i < W; i += blockDim.x) {
            const size_t r = nh * W + i;
            const int code = a.arg[r], am = code & (ST_FORCED - 1);
            const bool forced = (code & ST_FORCED) != 0;
            const float gd = a.g_disp ? a.g_disp[r] : 0.f, go = a.g_occ ? a.g_occ[r] : 0.f;
            const float d = a.disp[r], n = a.norm[r];
            for (int s = 0; s < 3; ++s) {
                const int j = am - 1 + s;
                const bool in = j >= 0 && j < W;
                float val = 0.f;
                if (in && (a.g_disp || a.g_occ)) {
                    const float shift = (float)(i - j > 0 ? i - j : 0);
                    const float g = forced ? gd * shift : gd * ((shift - d) / n) - go;
                    val = g * q.p(i, j, pa, pb);
                }
                l.scol[s * M + i] = in ? j : -1;
                l.sval[s * M + i] = val;
            }
            int il = -1, ir = -1;
            float vl = 0.f, vr = 0.f;
            if (a.g_gt) {
                const float t = a.target[r], hi = (float)(W - 1), gg = a.g_gt[r];
                il = (int)fminf(fmaxf(floorf(t), 0.f), hi);
                ir = (int)fminf(fmaxf(ceilf(t), 0.f), hi);
                const double wr = (double)t - (double)il;
                if (il == ir) {                                          // a clamped target: weights of size |t| that sum to 1
                    vl = (float)((double)gg * ((1.0 - wr) + wr) * (double)q.p(i, il, pa, pb));
                    ir = -1;
                } else {
                    vl = (float)((double)gg * (1.0 - wr) * (double)q.p(i, il, pa, pb));
                    vr = (float)((double)gg * wr * (double)q.p(i, ir, pa, pb));
                }
            }
            l.scol[3 * M + i] = il;
            l.sval[3 * M + i] = vl;
            l.scol[4 * M + i] = ir;
            l.sval[4 * M + i] = vr;
            l.dl[i] = a.g_bin_l ? a.g_bin_l[r] * q.p(i, W, pa, pb) : 0.f;
            l.dr[i] = a.g_bin_r ? a.g_bin_r[r] * q.p(W, i, pa, pb) : 0.f;
        }
        if (threadIdx.x == 0) {                                          // (never read as a row entry: `at` tests i == W first)
            l.dl[W] = 0.f;
            l.dr[W] = 0.f;
        }
        __syncthreads();
    }
    // gu = sum_j Gamma (one wave per row), gv = sum_i Gamma (lanes along j, the waves' partial sums combined in wave order)
    for (int i = wave; i < M; i += nwaves) {
        double acc = 0.0;
        for (int j = lane; j < M; j += 64) acc += (double)gam.at(i, j);
        acc = st_wave_sum(acc);
        if (lane == 0) l.gu[i] = (float)acc;
    }
    if (K) {
        for (int j0 = 0; j0 < M; j0 += 64) {
            const int j = j0 + lane;
            if (j >= M) continue;
            double acc = 0.0;
            for (int i = wave; i < M; i += nwaves) acc += (double)gam.at(i, j);
            l.part[wave * M + j] = (float)acc;
        }
    }
    __syncthreads();
    if (K) {
        for (int j = threadIdx.x; j < M; j += blockDim.x) {
            double acc = 0.0;
            for (int w = 0; w < nwaves; ++w) acc += (double)l.part[w * M + j];
            l.gv[j] = (float)acc;
        }
        __syncthreads();
    }
    // the reverse sweep
    for (int k = K; k >= 1; --k) {
        const double *uk = l.U + (size_t)k * M, *up = uk - M, *vk = l.V + (size_t)(k - 1) * M;
        float *ak = l.A + (size_t)(k - 1) * M, *bk = l.B + (size_t)(k - 1) * M;
        for (int j0 = 0; j0 < M; j0 += 64) {
            const int j = j0 + lane;
            if (j >= M) continue;
            const double vj = vk[j];
            double acc = 0.0;
            for (int i = wave; i < M; i += nwaves) acc += (double)l.gu[i] * (double)st_exp((((double)q.s(i, j) + vj) + uk[i]) - q.lm(i));
            l.part[wave * M + j] = (float)acc;
        }
        for (int j = threadIdx.x; j < M; j += blockDim.x) ak[j] = l.gu[j];
        __syncthreads();
        for (int j = threadIdx.x; j < M; j += blockDim.x) {
            double acc = k == K ? (double)l.gv[j] : 0.0;
            for (int w = 0; w < nwaves; ++w) acc -= (double)l.part[w * M + j];
            bk[j] = (float)acc;
        }
        __syncthreads();
        for (int i = wave; i < M; i += nwaves) {
            const double ui = up[i];
            double acc = 0.0;
            for (int j = lane; j < M; j += 64) acc += (double)bk[j] * (double)st_exp((((double)q.s(i, j) + ui) + vk[j]) - q.lm(j));
            acc = st_wave_sum(acc);
            if (lane == 0) l.gu[i] = (float)-acc;
        }
        __syncthreads();
    }
    // gS, written once; the dustbin row and column summed for g_phi
    double gphi = 0.0;
    for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        if (j >= M) continue;
        double vk[ST_MAX_ITERS];
        float bv[ST_MAX_ITERS];
#pragma unroll
        for (int k = 0; k < ST_MAX_ITERS; ++k) {
            vk[k] = k < K ? l.V[(size_t)k * M + j] : 0.0;
            bv[k] = k < K ? l.B[(size_t)k * M + j] : 0.f;
        }
        const double lnu = q.lm(j);
        for (int i = wave; i < M; i += nwaves) {
            const double sij = (double)q.s(i, j);
            double g = (double)gam.at(i, j);
            if (K) {
                const double lmu = q.lm(i);
#pragma unroll
                for (int k = 0; k < ST_MAX_ITERS; ++k)
                    if (k < K) {
                        const double sv = sij + vk[k];
                        g -= (double)l.A[(size_t)k * M + i] * (double)st_exp((sv + l.U[(size_t)(k + 1) * M + i]) - lmu);
                        g -= (double)bv[k] * (double)st_exp((sv + l.U[(size_t)k * M + i]) - lnu);
                    }
            } else {
                g -= (double)q.p(i, j, pa, pb) * (double)l.gu[i];
            }
            if (i < W && j < W)
                a.g_attn[(nh * W + i) * (size_t)W + j] = (float)g;
            else
                gphi += g;
        }
    }
    gphi = st_wave_sum(gphi);
    if (lane == 0) wsum[wave] = gphi;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int w = 0; w < nwaves; ++w) acc += wsum[w];
        a.phi_part[nh] = acc;
    }
}

// g_phi[0] = the sum of part[0..n) in a fixed order; one workgroup of 256
__global__ __launch_bounds__(256) void sttr_phi_sum_kernel(const double* __restrict__ part, float* __restrict__ g_phi, int n) {
    __shared__ double acc[256];
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) s += part[e];
    acc[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int e = 0; e < 256; ++e) t += acc[e];
        g_phi[0] = (float)t;
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline int st_threads(int M) { return M <= ST_SMALL_M ? 256 : 1024; }

inline size_t st_fwd_lds(int M, int nwaves) { return (size_t)M * (2 * nwaves + 2) * sizeof(double); }

int st_shape_ok(int N, int H, int W, int mode, int iters, const char* what) {
    STX_REQUIRE(N > 0 && H > 0, "%s: bad shape N=%d H=%d", what, N, H);
    STX_REQUIRE(W >= 2 && W <= ST_MAX_W, "%s: W=%d outside 2..%d", what, W, ST_MAX_W);
    STX_REQUIRE((long long)N * H < (1ll << 31) - 1 && (long long)N * H * (W + 1) * (long long)(W + 1) < (1ll << 40),
                "%s: tensor too large", what);
    STX_REQUIRE(mode == 0 || mode == 1, "%s: mode %d is neither 1 (optimal transport) nor 0 (softmax)", what, mode);
    STX_REQUIRE(!mode || (iters >= 1 && iters <= ST_MAX_ITERS), "%s: iters=%d outside 1..%d", what, iters, ST_MAX_ITERS);
    return STX_OK;
}

int st_launch_fwd(const StFwd& a, int N, int H, void* stream, const char* what) {
    const int M = a.W + 1, threads = st_threads(M);
    const size_t lds = st_fwd_lds(M, threads / 64);
    if (int rc = stx_lds_require((const void*)sttr_fwd_kernel, lds, what)) return rc;
    hipLaunchKernelGGL(sttr_fwd_kernel, dim3((unsigned)(N * H)), dim3(threads), lds, (hipStream_t)stream, a);
    return stx_check_launch(what);
}

template <bool DENSE>
int st_launch_bwd(const StBwd& a, float* g_phi, int N, int H, void* stream, const char* what) {
    const int M = a.W + 1, threads = st_threads(M);
    const size_t lds = st_bwd_lds_floats(M, a.mode ? a.iters : 0, threads / 64, DENSE) * sizeof(float);
    if (int rc = stx_lds_require((const void*)sttr_bwd_kernel<DENSE>, lds, what)) return rc;
    hipLaunchKernelGGL(sttr_bwd_kernel<DENSE>, dim3((unsigned)(N * H)), dim3(threads), lds, (hipStream_t)stream, a);
    if (int rc = stx_check_launch(what)) return rc;
    hipLaunchKernelGGL(sttr_phi_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)a.phi_part, g_phi, N * H);
    return stx_check_launch(what);
}

}  // namespace

extern "C" int stx_sttr_head_fwd(const float* attn, const float* phi, int mode, int iters, float log_one, float log_bin, float log_2w,
                                 const unsigned char* occ_mask, const float* target, float* disp, float* occ, float* norm, int* arg,
                                 float* gt_response, float* bin_left, float* bin_right, double* us, double* vs, int N, int H, int W,
                                 void* stream) {
    stx_begin();
    const char* what = "sttr_head_fwd";
    STX_REQUIRE(attn && phi && disp && occ && norm && arg && bin_left && bin_right, "%s: null pointer", what);
    STX_REQUIRE(!target == !gt_response, "%s: target and gt_response go together", what);
    STX_REQUIRE(!us == !vs, "%s: us and vs go together", what);
    if (int rc = st_shape_ok(N, H, W, mode, iters, what)) return rc;
    const StFwd a{attn, phi, W, iters, mode, log_one, log_bin, log_2w, us, vs, nullptr, occ_mask, target, disp, occ, norm, gt_response,
                  bin_left, bin_right, arg};
    return st_launch_fwd(a, N, H, stream, what);
}

extern "C" int stx_sttr_head_bwd(const float* g_disp, const float* g_occ, const float* g_gt, const float* g_bin_left,
                                 const float* g_bin_right, const float* attn, const float* phi, int mode, int iters, float log_one,
                                 float log_bin, float log_2w, const float* target, const float* disp, const float* norm, const int* arg,
                                 const double* us, const double* vs, float* g_attn, double* phi_partials, float* g_phi, int N, int H, int W,
                                 void* stream) {
    stx_begin();
    const char* what = "sttr_head_bwd";
    STX_REQUIRE(attn && phi && disp && norm && arg && us && vs && g_attn && phi_partials && g_phi, "%s: null pointer", what);
    STX_REQUIRE(g_disp || g_occ || g_gt || g_bin_left || g_bin_right, "%s: no gradient given", what);
    STX_REQUIRE(!g_gt || target, "%s: the gradient of gt_response needs the forward's target", what);
    if (int rc = st_shape_ok(N, H, W, mode, iters, what)) return rc;
    const StBwd a{attn, phi, us, vs, W, iters, mode, log_one, log_bin, log_2w, g_disp, g_occ, g_gt, g_bin_left, g_bin_right, disp, norm,
                  target, arg, nullptr, g_attn, phi_partials};
    return st_launch_bwd<false>(a, g_phi, N, H, stream, what);
}

extern "C" int stx_sttr_transport_fwd(const float* attn, const float* phi, int mode, int iters, float log_one, float log_bin,
                                      float log_2w, float* P, double* us, double* vs, int N, int H, int W, void* stream) {
    stx_begin();
    const char* what = "sttr_transport_fwd";
    STX_REQUIRE(attn && phi && P, "%s: null pointer", what);
    STX_REQUIRE(!us == !vs, "%s: us and vs go together", what);
    if (int rc = st_shape_ok(N, H, W, mode, iters, what)) return rc;
    StFwd a{};
    a.attn = attn; a.phi = phi; a.W = W; a.iters = iters; a.mode = mode;
    a.log_one = log_one; a.log_bin = log_bin; a.log_2w = log_2w;
    a.us = us; a.vs = vs; a.P = P;
    return st_launch_fwd(a, N, H, stream, what);
}

extern "C" int stx_sttr_transport_bwd(const float* G, const float* attn, const float* phi, int mode, int iters, float log_one,
                                      float log_bin, float log_2w, const double* us, const double* vs, float* g_attn, double* phi_partials,
                                      float* g_phi, int N, int H, int W, void* stream) {
    stx_begin();
    const char* what = "sttr_transport_bwd";
    STX_REQUIRE(G && attn && phi && us && vs && g_attn && phi_partials && g_phi, "%s: null pointer", what);
    if (int rc = st_shape_ok(N, H, W, mode, iters, what)) return rc;
    StBwd a{};
    a.attn = attn; a.phi = phi; a.us = us; a.vs = vs; a.W = W; a.iters = iters; a.mode = mode;
    a.log_one = log_one; a.log_bin = log_bin; a.log_2w = log_2w;
    a.G = G; a.g_attn = g_attn; a.phi_part = phi_partials;
    return st_launch_bwd<true>(a, g_phi, N, H, stream, what);
}

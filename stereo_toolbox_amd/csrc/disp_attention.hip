// FoundationStereo's disparity transformer (reference FoundationStereo/submodule.py `CostVolumeDisparityAttention`: a sinusoid
// table added once, then `num_transformer` post-norm encoder layers over the D tokens of every pixel), forward and backward.
//
// A sequence is the L = D tokens of one pixel, C channels each (the model: L 26, C 28, four heads of 7, feed-forward 28, four
// layers; 2160 sequences per image).  One sequence with every intermediate of a layer fits in a few KB of LDS, so a WAVE owns a
// sequence and nothing but the layer inputs (training) and the result ever reaches HBM.
//
// Layout.  Sequences are read from and written to the caller's memory through one address function,
//   offset(n, t) = (n / hw) * sb + (n % hw) * sp + t * st   (floats; the C channels of a token are contiguous),
// which is the dense channels-last volume [B][D][H][W][C] with hw = H W, sb = D H W C, sp = C, st = H W C, and a plain
// [N][L][C] tensor with hw = 1, sb = L C, sp = 0, st = C.  No permuted copy exists.
//
// Arithmetic of a layer, on x [L][C] in LDS (row stride SA with SA % 8 == 4: the 16 rows an MFMA operand reads fall into 16
// different bank groups):
//   Q, K, V = x Wq^T + bq, ...                              v_mfma_f32_16x16x4_f32, M = L and N = C in one or two 16-tiles each
//   per head: S = Q_h K_h^T / sqrt(hd); e = exp(S - rowmax) (formed in double, rounded once); O_h = (e V_h) / rowsum
//   z1 = x + drop1(O Wo^T + bo);  x1 = LayerNorm(z1)        moments, rsqrt and the affine map in double, rounded once
//   h = drop(gelu(x1 W1^T + b1))                            erf in double
//   z2 = x1 + drop2(h W2^T + b2); y = LayerNorm(z2)
// Out-of-range rows / columns / contraction indices of a tile are zeros made by the operand loaders: buffers hold L rows only.
//
// Forward: ONE launch for all layers.  One workgroup per CU with as many waves as the LDS holds (at most 12; nine at the model's
// size, so that the 2160 sequences of an image are one round of 256 x 9 waves), a static persistent grid: wave gw of nw takes the
// sequences gw, gw + nw, ...  The weights of one layer (4 C C + 2 C F + 9 C + F floats; 19.9 KB for the model) are staged into
// LDS per layer and round, all loads of a layer in flight together; per wave 4 buffers of L x SA floats and one L x SP score
// tile (14.5 KB for the model).  In training the input of every layer is written out: that is all the backward keeps.
//
// Backward: one launch per layer, from the last to the first, plus a small reduction launch.  A wave re-runs the layer's forward
// on the saved input in LDS (11 buffers + two score tiles, 38 KB for the model; one to four waves per workgroup, whatever fits
// into the CU's 160 KB), then walks it backwards.  The running gradient lives in one dense [N][L][C] buffer that every wave
// updates in place for its own sequences.  Parameter gradients: sequences are grouped into UNITS of four consecutive sequences
// -- a function of N only, not of the grid -- a wave takes whole units, adds the unit's sequences in order into the unit's row
// of a workspace slab (the first one stores), and the reduction launch adds the rows in unit order: no float atomics, and the
// bits do not depend on the grid.  Frozen parameters (NULL gradient pointer) skip their products; the walk stops at the lowest
// layer that anything is wanted from.
//
// Dropout (three sites per layer: 0 after out_proj, 1 after GELU, 2 after linear2): Philox4x32-10 with the 64-bit seed as key
// (low word, high word), read from DEVICE memory, and the counter
//   (sequence n, token >> 2, 4 * layer + site, channel);  word (token & 3) of the result decides the element:
//   keep iff word >= floor(p * 2^32), kept values are scaled by 1 / (1 - p).
// A function of the element's index and the seed only; the backward draws it again, nothing is stored.  With p = 0 or no seed
// nothing is drawn.
#include "stx_common.h"
#include <math.h>

extern "C" int stx_get_tuning(const char* name);

namespace {

constexpr int DA_MAX_L = 32, DA_MAX_C = 32, DA_MAX_HD = 8, DA_MAX_LAYERS = 8, DA_NPRM = 16, DA_UNIT = 4, DA_MAX_WAVES = 4;
constexpr int DA_CUS = 256;
constexpr int DA_FWD_BUFS = 4, DA_BWD_BUFS = 11;
constexpr int DA_FWD_MAX_WAVES = 12;                                    // three per SIMD: the forward kernel's registers allow it

// the 16 tensors of a layer in state-dict order
enum { P_QW, P_QB, P_KW, P_KB, P_VW, P_VB, P_OW, P_OB, P_W1, P_B1, P_W2, P_B2, P_G1, P_E1, P_G2, P_E2 };

#ifdef STX_HIPEMU
#define DA_WAVE_SYNC() hipemu::wave_sync_()
#else
// LDS hand-over inside one wave: its LDS accesses complete in order; the statement keeps the compiler from moving them across
#define DA_WAVE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif

struct DaDims { int N, L, C, F, E, hd; };
struct DaView { int hw; long long sb, sp, st; };

__host__ __device__ inline long long da_off(const DaView& v, int n, int t) {
    return (long long)(n / v.hw) * v.sb + (long long)(n % v.hw) * v.sp + (long long)t * v.st;
}

__host__ __device__ inline int da_stride(int n) { return (n & 7) == 4 ? n : n + 4; }      // n a multiple of 4

// off: the tensors packed one after the other (a slab row); lds: the same with every matrix row padded to da_stride(columns)
struct DaLay { int off[DA_NPRM + 1], lds[DA_NPRM + 1], rows[DA_NPRM], cols[DA_NPRM], sC, sF; };

__host__ __device__ inline DaLay da_layout(int C, int F) {
    DaLay l;
    const int rows[DA_NPRM] = {C, 1, C, 1, C, 1, C, 1, F, 1, C, 1, 1, 1, 1, 1};
    const int cols[DA_NPRM] = {C, C, C, C, C, C, C, C, C, F, F, C, C, C, C, C};
    l.off[0] = l.lds[0] = 0;
    for (int i = 0; i < DA_NPRM; ++i) {
        l.rows[i] = rows[i];
        l.cols[i] = cols[i];
        l.off[i + 1] = l.off[i] + rows[i] * cols[i];
        l.lds[i + 1] = l.lds[i] + (rows[i] > 1 ? rows[i] * da_stride(cols[i]) : cols[i]);
    }
    l.sC = da_stride(C);
    l.sF = da_stride(F);
    return l;
}

// ------------------------------------------------------------------------------------------------ dropout
struct DaDrop { unsigned k0, k1, thr; float scale; int on; };
struct DaWords { unsigned w[4]; };

__device__ inline DaWords da_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    return DaWords{{c0, c1, c2, c3}};
}

__device__ inline DaWords da_draw(const DaDrop& d, int n, int tgroup, int layer, int site, int ch) {
    return da_philox((unsigned)n, (unsigned)tgroup, (unsigned)(4 * layer + site), (unsigned)ch, d.k0, d.k1);
}

__device__ inline DaDrop da_drop_setup(const long long* seed, unsigned thr, float scale) {
    DaDrop d{0u, 0u, thr, scale, 0};
    if (seed && thr) {
        const unsigned long long s = (unsigned long long)seed[0];
        d.k0 = (unsigned)s;
        d.k1 = (unsigned)(s >> 32);
        d.on = 1;
    }
    return d;
}

// ------------------------------------------------------------------------------------------------ device helpers
__device__ __forceinline__ f32x4 da_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ inline double da_gelu(double u) { return 0.5 * u * (1.0 + erf(u * 0.70710678118654752440)); }
__device__ inline double da_gelu_grad(double u) {
    return 0.5 * (1.0 + erf(u * 0.70710678118654752440)) + u * exp(-0.5 * u * u) * 0.39894228040143267794;
}

// D[m][n] = sum_k fa(m, k) fb(k, n), M, N <= 32, any K: up to 2 x 2 tiles of 16 x 16, one pass over K.  fa / fb are called for
// in-range indices only (everything else is a zero operand); fd(m4, n, v) receives rows m4 .. m4 + 3 of column n < N and checks
// the rows itself.  All 64 lanes of the wave call it together.
template <class FA, class FB, class FD>
__device__ __forceinline__ void da_gemm(int M, int N, int K, int lane, FA fa, FB fb, FD fd) {
    STX_OPAQUE_VGPR(lane);                                               // keeps the address math of the ~40 inlined products local to each
    const int a = lane & 15, g = lane >> 4;
    const bool m1 = M > 16, n1 = N > 16;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 c00 = z, c01 = z, c10 = z, c11 = z;
    DA_WAVE_SYNC();
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + g;
        const bool kin = k < K;
        const float a0 = (kin && a < M) ? fa(a, k) : 0.f;
        const float b0 = (kin && a < N) ? fb(k, a) : 0.f;
        float b1 = 0.f;
        c00 = da_mfma(a0, b0, c00);
        if (n1) {
            b1 = (kin && 16 + a < N) ? fb(k, 16 + a) : 0.f;
            c01 = da_mfma(a0, b1, c01);
        }
        if (m1) {
            const float a1 = (kin && 16 + a < M) ? fa(16 + a, k) : 0.f;
            c10 = da_mfma(a1, b0, c10);
            if (n1) c11 = da_mfma(a1, b1, c11);
        }
    }
    if (a < N) {
        fd(4 * g, a, c00);
        if (m1) fd(16 + 4 * g, a, c10);
    }
    if (n1 && 16 + a < N) {
        fd(4 * g, 16 + a, c01);
        if (m1) fd(16 + 4 * g, 16 + a, c11);
    }
    DA_WAVE_SYNC();
}

// the buffers of one wave ([L][SA] each, P and P2 [L][SP]); in the forward kernel O, X1 and HD alias Q, K and V, the rest is unused
struct DaBufs {
    float *X, *Q, *K, *V, *O, *X1, *XH1, *U, *HD, *XH2, *G, *P, *P2, *rs1, *rs2;
    double* dsc;
};

struct DaCtx {
    DaDims d;
    DaLay lay;
    const float* wl;       // the layer's weights in LDS
    DaBufs b;
    DaDrop dr;
    int SA, SP, n, layer, lane;
    double eps;
};

__device__ inline void da_load(float* buf, int SA, const float* src, const DaView& v, int n, int L, int C, const float* pe, int lane) {
    const int c4n = C >> 2;
    DA_WAVE_SYNC();
    for (int e = lane; e < L * c4n; e += 64) {
        const int t = e / c4n, c = (e - t * c4n) * 4;
        float4 x = stx_ld4(src + da_off(v, n, t) + c);
        if (pe) {
            const float4 q = stx_ld4(pe + t * C + c);
            x.x += q.x; x.y += q.y; x.z += q.z; x.w += q.w;
        }
        stx_st4(buf + t * SA + c, x);
    }
    DA_WAVE_SYNC();
}

__device__ inline void da_store(float* dst, const DaView& v, int n, const float* buf, int SA, int L, int C, int lane) {
    const int c4n = C >> 2;
    DA_WAVE_SYNC();
    for (int e = lane; e < L * c4n; e += 64) {
        const int t = e / c4n, c = (e - t * c4n) * 4;
        stx_st4(dst + da_off(v, n, t) + c, stx_ld4(buf + t * SA + c));
    }
    DA_WAVE_SYNC();
}

// P [L][L] holds scores; afterwards e = exp(score - row max) (float) and dsc[i] = 1 / sum_j e[i][j] (double).  Lane (i = lane & 31,
// half = lane >> 5) takes the columns half, half + 2, ... of row i; the two partial sums are added in the order (half 0) + (half 1).
__device__ inline void da_softmax(float* P, int SP, int L, double* dsc, int lane) {
    const int i = lane & 31, half = lane >> 5;
    DA_WAVE_SYNC();
    float m = -__builtin_huge_valf();
    if (i < L)
        for (int j = half; j < L; j += 2) m = fmaxf(m, P[i * SP + j]);
    m = fmaxf(m, __shfl_xor(m, 32));
    double s = 0.0;
    if (i < L)
        for (int j = half; j < L; j += 2) {
            const float e = (float)exp((double)P[i * SP + j] - (double)m);
            P[i * SP + j] = e;
            s += (double)e;
        }
    dsc[lane] = s;
    DA_WAVE_SYNC();
    double tot = 1.0;
    if (lane < 32) tot = dsc[lane] + dsc[lane + 32];
    DA_WAVE_SYNC();
    if (lane < 32) dsc[lane] = lane < L ? 1.0 / tot : 0.0;
    DA_WAVE_SYNC();
}

// LayerNorm of the rows of Z over C channels: Y = xhat * gamma + beta, XH = xhat, rs = rstd; Y / XH may be NULL or Z itself
__device__ inline void da_layernorm(const float* Z, float* Y, float* XH, float* rs, const float* gam, const float* bet, int L, int C, int SA,
                                    double eps, int lane) {
    DA_WAVE_SYNC();
    if (lane < L) {
        const float* z = Z + lane * SA;
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += (double)z[c];
        const double mean = s / C;
        double v = 0.0;
        for (int c = 0; c < C; ++c) {
            const double dlt = (double)z[c] - mean;
            v += dlt * dlt;
        }
        const double rstd = 1.0 / sqrt(v / C + eps);
        for (int c = 0; c < C; ++c) {
            const double xh = ((double)z[c] - mean) * rstd;
            if (XH) XH[lane * SA + c] = (float)xh;
            if (Y) Y[lane * SA + c] = (float)(xh * (double)gam[c] + (double)bet[c]);
        }
        if (rs) rs[lane] = (float)rstd;
    }
    DA_WAVE_SYNC();
}

// scores of head h into P: Q_h K_h^T / sqrt(hd)
__device__ inline void da_scores(const DaCtx& c, int h) {
    const DaBufs& b = c.b;
    const int L = c.d.L, hd = c.d.hd, SA = c.SA, SP = c.SP, c0 = h * hd;
    const float sq = (float)sqrt((double)hd);
    da_gemm(L, L, hd, c.lane, [&](int m, int k) { return b.Q[m * SA + c0 + k]; }, [&](int k, int n) { return b.K[n * SA + c0 + k]; },
            [&](int m4, int n, f32x4 v) {
                for (int r = 0; r < 4; ++r)
                    if (m4 + r < L) b.P[(m4 + r) * SP + n] = v[r] / sq;
            });
}

// One layer forward on c.b.X.  BWD = false: the result replaces X (O, X1, HD may alias Q, K, V).  BWD = true: everything the
// backward walk needs stays: Q, K, V, O, X1, XH1 / rs1, U (the GELU's argument), HD, XH2 / rs2.
template <bool BWD>
__device__ inline void da_layer_fwd(const DaCtx& c) {
    const DaBufs& b = c.b;
    const DaLay& lay = c.lay;
    const DaDrop& dr = c.dr;
    const int L = c.d.L, C = c.d.C, F = c.d.F, hd = c.d.hd, SA = c.SA, SP = c.SP, lane = c.lane, sC = lay.sC, sF = lay.sF;
    for (int j = 0; j < 3; ++j) {
        const float *W = c.wl + lay.lds[2 * j], *bias = c.wl + lay.lds[2 * j + 1];
        float* out = j == 0 ? b.Q : (j == 1 ? b.K : b.V);
        da_gemm(L, C, C, lane, [&](int m, int k) { return b.X[m * SA + k]; }, [&](int k, int n) { return W[n * sC + k]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) out[(m4 + r) * SA + n] = v[r] + bias[n];
                });
    }
    for (int h = 0; h < c.d.E; ++h) {
        const int c0 = h * hd;
        da_scores(c, h);
        da_softmax(b.P, SP, L, b.dsc, lane);
        da_gemm(L, hd, L, lane, [&](int m, int k) { return b.P[m * SP + k]; }, [&](int k, int n) { return b.V[k * SA + c0 + n]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) b.O[(m4 + r) * SA + c0 + n] = (float)((double)v[r] * b.dsc[m4 + r]);
                });
    }
    {
        const float *W = c.wl + lay.lds[P_OW], *bias = c.wl + lay.lds[P_OB];
        da_gemm(L, C, C, lane, [&](int m, int k) { return b.O[m * SA + k]; }, [&](int k, int n) { return W[n * sC + k]; },
                [&](int m4, int n, f32x4 v) {
                    DaWords w{};
                    if (dr.on) w = da_draw(dr, c.n, m4 >> 2, c.layer, 0, n);
                    for (int r = 0; r < 4; ++r) {
                        const int t = m4 + r;
                        if (t >= L) continue;
                        float y = v[r] + bias[n];
                        if (dr.on) y = w.w[r] >= dr.thr ? y * dr.scale : 0.f;
                        b.X1[t * SA + n] = b.X[t * SA + n] + y;
                    }
                });
    }
    da_layernorm(b.X1, b.X1, BWD ? b.XH1 : nullptr, BWD ? b.rs1 : nullptr, c.wl + lay.lds[P_G1], c.wl + lay.lds[P_E1], L, C, SA, c.eps, lane);
    {
        const float *W = c.wl + lay.lds[P_W1], *bias = c.wl + lay.lds[P_B1];
        da_gemm(L, F, C, lane, [&](int m, int k) { return b.X1[m * SA + k]; }, [&](int k, int n) { return W[n * sC + k]; },
                [&](int m4, int n, f32x4 v) {
                    DaWords w{};
                    if (dr.on) w = da_draw(dr, c.n, m4 >> 2, c.layer, 1, n);
                    for (int r = 0; r < 4; ++r) {
                        const int t = m4 + r;
                        if (t >= L) continue;
                        const float u = v[r] + bias[n];
                        if (BWD) b.U[t * SA + n] = u;
                        float y = (float)da_gelu((double)u);
                        if (dr.on) y = w.w[r] >= dr.thr ? y * dr.scale : 0.f;
                        b.HD[t * SA + n] = y;
                    }
                });
    }
    {
        const float *W = c.wl + lay.lds[P_W2], *bias = c.wl + lay.lds[P_B2];
        float* Z = BWD ? b.XH2 : b.X;
        da_gemm(L, C, F, lane, [&](int m, int k) { return b.HD[m * SA + k]; }, [&](int k, int n) { return W[n * sF + k]; },
                [&](int m4, int n, f32x4 v) {
                    DaWords w{};
                    if (dr.on) w = da_draw(dr, c.n, m4 >> 2, c.layer, 2, n);
                    for (int r = 0; r < 4; ++r) {
                        const int t = m4 + r;
                        if (t >= L) continue;
                        float y = v[r] + bias[n];
                        if (dr.on) y = w.w[r] >= dr.thr ? y * dr.scale : 0.f;
                        Z[t * SA + n] = b.X1[t * SA + n] + y;
                    }
                });
        da_layernorm(Z, BWD ? nullptr : Z, BWD ? Z : nullptr, BWD ? b.rs2 : nullptr, c.wl + lay.lds[P_G2], c.wl + lay.lds[P_E2], L, C, SA, c.eps,
                     lane);
    }
}

__device__ inline void da_stage_weights(float* wl, const DaLay& lay, const float* const* prm) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (2 * nt >= lay.rows[P_W1] * lay.cols[P_W1] && 2 * nt >= lay.rows[P_QW] * lay.cols[P_QW]) {
        // a workgroup that covers every matrix in two elements per thread (the forward's): all 22 loads are issued before the
        // first LDS store, so a layer's staging costs one trip to L2, not one per tensor
        float v[22];
        int k = 0;
#pragma unroll
        for (int i = 0; i < DA_NPRM; ++i) {
            const int n = lay.rows[i] * lay.cols[i];
#pragma unroll
            for (int s = 0; s < ((i < P_G1 && !(i & 1)) ? 2 : 1); ++s) {
                const int e = tid + s * nt;
                v[k++] = e < n ? prm[i][e] : 0.f;
            }
        }
        k = 0;
#pragma unroll
        for (int i = 0; i < DA_NPRM; ++i) {
            const int cols = lay.cols[i], n = lay.rows[i] * cols, ld = lay.rows[i] > 1 ? da_stride(cols) : cols;
#pragma unroll
            for (int s = 0; s < ((i < P_G1 && !(i & 1)) ? 2 : 1); ++s) {
                const int e = tid + s * nt, r = e / cols;
                if (e < n) wl[lay.lds[i] + r * ld + (e - r * cols)] = v[k];
                ++k;
            }
        }
        return;
    }
    for (int i = 0; i < DA_NPRM; ++i) {
        const int cols = lay.cols[i], n = lay.rows[i] * cols, ld = lay.rows[i] > 1 ? da_stride(cols) : cols;
        const float* src = prm[i];
        float* dst = wl + lay.lds[i];
        for (int e = threadIdx.x; e < n; e += blockDim.x) {
            const int r = e / cols;
            dst[r * ld + (e - r * cols)] = src[e];
        }
    }
}

__device__ inline DaBufs da_carve(float* base, int L, int SA, int SP, bool bwd) {
    DaBufs b;
    b.dsc = reinterpret_cast<double*>(base);
    base += 128;
    b.rs1 = base;
    b.rs2 = base + 32;
    base += 64;
    const int nb = L * SA;
    b.X = base;
    b.Q = base + nb;
    b.K = base + 2 * nb;
    b.V = base + 3 * nb;
    if (bwd) {
        b.O = base + 4 * nb;
        b.X1 = base + 5 * nb;
        b.XH1 = base + 6 * nb;
        b.U = base + 7 * nb;
        b.HD = base + 8 * nb;
        b.XH2 = base + 9 * nb;
        b.G = base + 10 * nb;
        b.P = base + 11 * nb;
        b.P2 = b.P + L * SP;
    } else {
        b.O = b.Q;
        b.X1 = b.K;
        b.HD = b.V;
        b.XH1 = b.U = b.XH2 = b.G = b.P2 = nullptr;
        b.P = base + 4 * nb;
    }
    return b;
}

__host__ __device__ inline int da_wave_floats(int L, int SA, int SP, bool bwd) {
    return 192 + (bwd ? DA_BWD_BUFS : DA_FWD_BUFS) * L * SA + (bwd ? 2 : 1) * L * SP;
}

__host__ __device__ inline int da_weight_floats(const DaLay& lay) { return (lay.lds[DA_NPRM] + 3) & ~3; }

// ------------------------------------------------------------------------------------------------ forward
struct DaPrm { const float* p[DA_NPRM]; };

struct DaFwdArgs {
    const float *x, *pe;
    float *y, *saved;
    const long long* seed;
    DaPrm prm[DA_MAX_LAYERS];
    DaDims d;
    DaView v;
    int layers;
    unsigned thr;
    float scale, eps;
};

__global__ __launch_bounds__(64 * DA_FWD_MAX_WAVES) void disp_attention_fwd_kernel(DaFwdArgs A) {
    STX_DYN_SMEM(smem);
    float* wl = reinterpret_cast<float*>(smem);
    const DaDims d = A.d;
    DaCtx c;
    c.d = d;
    c.lay = da_layout(d.C, d.F);
    c.wl = wl;
    c.SA = da_stride(d.C > d.F ? d.C : d.F);
    c.SP = da_stride((d.L + 3) & ~3);
    c.lane = threadIdx.x & 63;
    c.eps = (double)A.eps;
    c.dr = da_drop_setup(A.seed, A.thr, A.scale);
    const int wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    c.b = da_carve(wl + da_weight_floats(c.lay) + wave * da_wave_floats(d.L, c.SA, c.SP, false), d.L, c.SA, c.SP, false);
    const int nw = gridDim.x * nwv, gw = blockIdx.x * nwv + wave;
    const DaView dense{1, (long long)d.L * d.C, 0, (long long)d.C};
    const size_t per_layer = (size_t)d.N * d.L * d.C;
    for (int base = 0; base < d.N; base += nw) {
        const int n = base + gw;
        const bool live = n < d.N;
        c.n = n;
        if (live) da_load(c.b.X, c.SA, A.x, A.v, n, d.L, d.C, A.pe, c.lane);
        for (int l = 0; l < A.layers; ++l) {
            __syncthreads();                                             // every wave is done with the previous layer's weights
            da_stage_weights(wl, c.lay, A.prm[l].p);
            __syncthreads();
            if (!live) continue;
            c.layer = l;
            if (A.saved) da_store(A.saved + l * per_layer, dense, n, c.b.X, c.SA, d.L, d.C, c.lane);
            da_layer_fwd<false>(c);
        }
        if (live) da_store(A.y, A.v, n, c.b.X, c.SA, d.L, d.C, c.lane);
    }
}

// ------------------------------------------------------------------------------------------------ backward
struct DaBwdArgs {
    const float *xin, *gout;       // the layer's saved input [N][L][C]; the gradient of its output through gv
    float* gin;                    // the gradient of its input through iv, or NULL
    float* slab;                   // [units][lay.off[16]]
    const long long* seed;
    DaPrm prm;
    DaDims d;
    DaView gv, iv;
    int layer;
    unsigned want, thr;            // bit i: the gradient of tensor i is wanted
    float scale, eps;
};

__device__ __forceinline__ void da_acc(float* row, int idx, float v, bool first) { row[idx] = first ? v : row[idx] + v; }

// row[off + c] (+)= sum_t A[t][c] (* B[t][c]): lane c
__device__ inline void da_colsum(float* row, int off, const float* A, const float* B, int L, int n, int SA, bool first, int lane) {
    DA_WAVE_SYNC();
    if (lane < n) {
        float s = 0.f;
        for (int t = 0; t < L; ++t) s += B ? A[t * SA + lane] * B[t * SA + lane] : A[t * SA + lane];
        da_acc(row, off + lane, s, first);
    }
    DA_WAVE_SYNC();
}

// row[off + m * N + n] (+)= sum_t A[t][m] B[t][n]
__device__ inline void da_wgrad(float* row, int off, const float* A, const float* B, int M, int N, int L, int SA, bool first, int lane) {
    da_gemm(M, N, L, lane, [&](int m, int k) { return A[k * SA + m]; }, [&](int k, int n) { return B[k * SA + n]; },
            [&](int m4, int n, f32x4 v) {
                for (int r = 0; r < 4; ++r)
                    if (m4 + r < M) da_acc(row, off + (m4 + r) * N + n, v[r], first);
            });
}

// G <- the gradient in front of a LayerNorm whose output's gradient is G; xhat and rstd as saved
__device__ inline void da_layernorm_bwd(float* G, const float* XH, const float* rs, const float* gam, int L, int C, int SA, int lane) {
    DA_WAVE_SYNC();
    if (lane < L) {
        float* g = G + lane * SA;
        const float* xh = XH + lane * SA;
        double m1 = 0.0, m2 = 0.0;
        for (int c = 0; c < C; ++c) {
            const double dx = (double)g[c] * (double)gam[c];
            m1 += dx;
            m2 += dx * (double)xh[c];
        }
        m1 /= C;
        m2 /= C;
        const double rstd = (double)rs[lane];
        for (int c = 0; c < C; ++c) g[c] = (float)(rstd * ((double)g[c] * (double)gam[c] - m1 - (double)xh[c] * m2));
    }
    DA_WAVE_SYNC();
}

// D[t][ch] = G[t][ch] * (kept ? scale : 0) for site `site` of this sequence
__device__ inline void da_drop_copy(float* D, const float* G, const DaCtx& c, int site, int width) {
    const int L = c.d.L, SA = c.SA, groups = (L + 3) >> 2;
    DA_WAVE_SYNC();
    for (int e = c.lane; e < groups * width; e += 64) {
        const int tg = e / width, ch = e - tg * width;
        const DaWords w = da_draw(c.dr, c.n, tg, c.layer, site, ch);
        for (int r = 0; r < 4; ++r) {
            const int t = 4 * tg + r;
            if (t < L) D[t * SA + ch] = w.w[r] >= c.dr.thr ? G[t * SA + ch] * c.dr.scale : 0.f;
        }
    }
    DA_WAVE_SYNC();
}

__device__ inline void da_layer_bwd(const DaCtx& c, unsigned want, float* row, bool first, bool need_gin) {
    const DaBufs& b = c.b;
    const DaLay& lay = c.lay;
    const int L = c.d.L, C = c.d.C, F = c.d.F, hd = c.d.hd, SA = c.SA, SP = c.SP, lane = c.lane, sC = lay.sC, sF = lay.sF;
    auto wants = [&](int i) { return (want >> i) & 1u; };
    // ---- LayerNorm 2
    if (wants(P_G2)) da_colsum(row, lay.off[P_G2], b.G, b.XH2, L, C, SA, first, lane);
    if (wants(P_E2)) da_colsum(row, lay.off[P_E2], b.G, nullptr, L, C, SA, first, lane);
    da_layernorm_bwd(b.G, b.XH2, b.rs2, c.wl + lay.lds[P_G2], L, C, SA, lane);                   // G = d z2
    // ---- linear2, behind dropout 2
    float* DY = b.G;
    if (c.dr.on) {
        DY = b.XH2;
        da_drop_copy(DY, b.G, c, 2, C);
    }
    if (wants(P_B2)) da_colsum(row, lay.off[P_B2], DY, nullptr, L, C, SA, first, lane);
    if (wants(P_W2)) da_wgrad(row, lay.off[P_W2], DY, b.HD, C, F, L, SA, first, lane);
    {
        const float* W = c.wl + lay.lds[P_W2];
        da_gemm(L, F, C, lane, [&](int m, int k) { return DY[m * SA + k]; }, [&](int k, int n) { return W[k * sF + n]; },
                [&](int m4, int n, f32x4 v) {
                    DaWords w{};
                    if (c.dr.on) w = da_draw(c.dr, c.n, m4 >> 2, c.layer, 1, n);
                    for (int r = 0; r < 4; ++r) {
                        const int t = m4 + r;
                        if (t >= L) continue;
                        float dh = v[r];
                        if (c.dr.on) dh = w.w[r] >= c.dr.thr ? dh * c.dr.scale : 0.f;
                        b.U[t * SA + n] = (float)((double)dh * da_gelu_grad((double)b.U[t * SA + n]));    // U = d u
                    }
                });
    }
    // ---- linear1
    if (wants(P_B1)) da_colsum(row, lay.off[P_B1], b.U, nullptr, L, F, SA, first, lane);
    if (wants(P_W1)) da_wgrad(row, lay.off[P_W1], b.U, b.X1, F, C, L, SA, first, lane);
    {
        const float* W = c.wl + lay.lds[P_W1];
        da_gemm(L, C, F, lane, [&](int m, int k) { return b.U[m * SA + k]; }, [&](int k, int n) { return W[k * sC + n]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) b.G[(m4 + r) * SA + n] += v[r];                          // G = d x1
                });
    }
    // ---- LayerNorm 1
    if (wants(P_G1)) da_colsum(row, lay.off[P_G1], b.G, b.XH1, L, C, SA, first, lane);
    if (wants(P_E1)) da_colsum(row, lay.off[P_E1], b.G, nullptr, L, C, SA, first, lane);
    da_layernorm_bwd(b.G, b.XH1, b.rs1, c.wl + lay.lds[P_G1], L, C, SA, lane);                   // G = d z1, also the residual's share of d x
    // ---- out_proj, behind dropout 1
    float* DA = b.G;
    if (c.dr.on) {
        DA = b.XH1;
        da_drop_copy(DA, b.G, c, 0, C);
    }
    if (wants(P_OB)) da_colsum(row, lay.off[P_OB], DA, nullptr, L, C, SA, first, lane);
    if (wants(P_OW)) da_wgrad(row, lay.off[P_OW], DA, b.O, C, C, L, SA, first, lane);
    float* dO = b.XH2;
    {
        const float* W = c.wl + lay.lds[P_OW];
        da_gemm(L, C, C, lane, [&](int m, int k) { return DA[m * SA + k]; }, [&](int k, int n) { return W[k * sC + n]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) dO[(m4 + r) * SA + n] = v[r];
                });
    }
    // ---- attention: dQ, dK, dV go where X1, U and HD were
    float *dQ = b.X1, *dK = b.U, *dV = b.HD;
    const float sq = (float)sqrt((double)hd);
    for (int h = 0; h < c.d.E; ++h) {
        const int c0 = h * hd;
        da_scores(c, h);
        da_softmax(b.P, SP, L, b.dsc, lane);
        const int i = lane & 31, half = lane >> 5;
        if (i < L)
            for (int j = half; j < L; j += 2) b.P[i * SP + j] = (float)((double)b.P[i * SP + j] * b.dsc[i]);
        da_gemm(L, hd, L, lane, [&](int m, int k) { return b.P[k * SP + m]; }, [&](int k, int n) { return dO[k * SA + c0 + n]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) dV[(m4 + r) * SA + c0 + n] = v[r];
                });
        da_gemm(L, L, hd, lane, [&](int m, int k) { return dO[m * SA + c0 + k]; }, [&](int k, int n) { return b.V[n * SA + c0 + k]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) b.P2[(m4 + r) * SP + n] = v[r];                          // d P
                });
        // d S = P (d P - sum_j P d P): the row sum over the very products it is subtracted from, so that one key gives exact zeros
        {
            double s = 0.0;
            if (i < L)
                for (int j = half; j < L; j += 2) s += (double)b.P[i * SP + j] * (double)b.P2[i * SP + j];
            b.dsc[lane] = s;
            DA_WAVE_SYNC();
            const double dl = b.dsc[i] + b.dsc[i + 32];
            if (i < L)
                for (int j = half; j < L; j += 2)
                    b.P[i * SP + j] = (float)((double)b.P[i * SP + j] * ((double)b.P2[i * SP + j] - dl)) / sq;   // d (Q K^T)
        }
        da_gemm(L, hd, L, lane, [&](int m, int k) { return b.P[m * SP + k]; }, [&](int k, int n) { return b.K[k * SA + c0 + n]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) dQ[(m4 + r) * SA + c0 + n] = v[r];
                });
        da_gemm(L, hd, L, lane, [&](int m, int k) { return b.P[k * SP + m]; }, [&](int k, int n) { return b.Q[k * SA + c0 + n]; },
                [&](int m4, int n, f32x4 v) {
                    for (int r = 0; r < 4; ++r)
                        if (m4 + r < L) dK[(m4 + r) * SA + c0 + n] = v[r];
                });
    }
    // ---- the three projections
    for (int j = 0; j < 3; ++j) {
        const float* D = j == 0 ? dQ : (j == 1 ? dK : dV);
        if (wants(2 * j + 1)) da_colsum(row, lay.off[2 * j + 1], D, nullptr, L, C, SA, first, lane);
        if (wants(2 * j)) da_wgrad(row, lay.off[2 * j], D, b.X, C, C, L, SA, first, lane);
        if (need_gin) {
            const float* W = c.wl + lay.lds[2 * j];
            da_gemm(L, C, C, lane, [&](int m, int k) { return D[m * SA + k]; }, [&](int k, int n) { return W[k * sC + n]; },
                    [&](int m4, int n, f32x4 v) {
                        for (int r = 0; r < 4; ++r)
                            if (m4 + r < L) b.G[(m4 + r) * SA + n] += v[r];                      // G = d x
                    });
        }
    }
}

__global__ __launch_bounds__(256) void disp_attention_bwd_kernel(DaBwdArgs A) {
    STX_DYN_SMEM(smem);
    float* wl = reinterpret_cast<float*>(smem);
    const DaDims d = A.d;
    DaCtx c;
    c.d = d;
    c.lay = da_layout(d.C, d.F);
    c.wl = wl;
    c.SA = da_stride(d.C > d.F ? d.C : d.F);
    c.SP = da_stride((d.L + 3) & ~3);
    c.lane = threadIdx.x & 63;
    c.eps = (double)A.eps;
    c.dr = da_drop_setup(A.seed, A.thr, A.scale);
    c.layer = A.layer;
    const int wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    c.b = da_carve(wl + da_weight_floats(c.lay) + wave * da_wave_floats(d.L, c.SA, c.SP, true), d.L, c.SA, c.SP, true);
    da_stage_weights(wl, c.lay, A.prm.p);
    __syncthreads();
    const int nw = gridDim.x * nwv, gw = blockIdx.x * nwv + wave, units = (d.N + DA_UNIT - 1) / DA_UNIT;
    const DaView dense{1, (long long)d.L * d.C, 0, (long long)d.C};
    for (int u = gw; u < units; u += nw) {
        float* row = A.slab + (size_t)u * c.lay.off[DA_NPRM];
        for (int s = 0; s < DA_UNIT; ++s) {
            const int n = u * DA_UNIT + s;
            if (n >= d.N) break;
            c.n = n;
            da_load(c.b.X, c.SA, A.xin, dense, n, d.L, d.C, nullptr, c.lane);
            da_load(c.b.G, c.SA, A.gout, A.gv, n, d.L, d.C, nullptr, c.lane);
            da_layer_fwd<true>(c);
            da_layer_bwd(c, A.want, row, s == 0, A.gin != nullptr);
            if (A.gin) da_store(A.gin, A.iv, n, c.b.G, c.SA, d.L, d.C, c.lane);
        }
    }
}

// out[j] = sum over the units, in order, of slab[u][j].  256 threads = 64 elements x 4 chunks of units; the four chunk sums are
// added in chunk order.  Tensors with a NULL pointer are skipped.
struct DaOut { float* p[DA_NPRM]; };

__global__ __launch_bounds__(256) void disp_attention_reduce_kernel(const float* __restrict__ slab, int units, int C, int F, DaOut out) {
    __shared__ float part[4][64];
    const DaLay lay = da_layout(C, F);
    const int total = lay.off[DA_NPRM], e = threadIdx.x & 63, q = threadIdx.x >> 6, j = blockIdx.x * 64 + e;
    const int chunk = (units + 3) / 4, lo = q * chunk, hi = lo + chunk < units ? lo + chunk : units;
    int which = 0;
    while (which < DA_NPRM - 1 && j >= lay.off[which + 1]) ++which;
    const bool live = j < total && out.p[which] != nullptr;
    float s = 0.f;
    if (live)
        for (int u = lo; u < hi; ++u) s += slab[(size_t)u * total + j];
    part[q][e] = s;
    __syncthreads();
    if (live && q == 0) out.p[which][j - lay.off[which]] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
}

// masks [layers][3][N][L][Cm] bytes, Cm = max(C, F): 1 = kept
__global__ __launch_bounds__(256) void disp_attention_masks_kernel(const long long* seed, unsigned thr, unsigned char* __restrict__ masks, int N,
                                                                   int L, int Cm, int layers) {
    const DaDrop dr = da_drop_setup(seed, thr, 1.f);
    const int groups = (L + 3) >> 2;
    const size_t total = (size_t)layers * 3 * N * groups * Cm, id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int ch = (int)(id % Cm), tg = (int)((id / Cm) % groups), n = (int)((id / ((size_t)Cm * groups)) % N);
    const int ls = (int)(id / ((size_t)Cm * groups * N)), layer = ls / 3, site = ls - 3 * layer;
    DaWords w{};
    if (dr.on) w = da_draw(dr, n, tg, layer, site, ch);
    for (int r = 0; r < 4; ++r) {
        const int t = 4 * tg + r;
        if (t < L) masks[(((size_t)ls * N + n) * L + t) * Cm + ch] = (!dr.on || w.w[r] >= dr.thr) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ host side
int da_supported(int L, int C, int nhead, int F, int layers) {
    if (L < 1 || L > DA_MAX_L) return 0;
    if (C < 4 || C > DA_MAX_C || (C & 3)) return 0;
    if (nhead < 1 || C % nhead || C / nhead > DA_MAX_HD) return 0;
    if (F < 4 || F > DA_MAX_C || (F & 3)) return 0;
    if (layers < 1 || layers > DA_MAX_LAYERS) return 0;
    return 1;
}

int da_check(const char* what, int N, int L, int C, int nhead, int F, int layers, float p, int hw, long long sb, long long sp, long long st) {
    STX_REQUIRE(da_supported(L, C, nhead, F, layers),
                "%s: L=%d C=%d heads=%d ff=%d layers=%d is not served (L 1..32; C, ff multiples of 4 up to 32; head dim <= 8; 1..8 layers)", what, L,
                C, nhead, F, layers);
    STX_REQUIRE(N >= 1 && (long long)N * L * C < (1ll << 31), "%s: N=%d sequences: N L C must stay below 2^31", what, N);
    STX_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout probability %g outside [0, 1)", what, (double)p);
    STX_REQUIRE(hw >= 1 && N % hw == 0 && !(sb & 3) && !(sp & 3) && !(st & 3) && sb >= 0 && sp >= 0 && st >= 0,
                "%s: strides (hw %d, %lld, %lld, %lld) must be non-negative multiples of 4 floats, N a multiple of hw", what, hw, sb, sp, st);
    return STX_OK;
}

// the test switch STX_DA_GRID (csrc/stx_runtime.hip), read by name
int da_grid_override() { return stx_get_tuning("STX_DA_GRID"); }

unsigned da_threshold(float p) { return (unsigned)floor((double)p * 4294967296.0); }

size_t da_lds_bytes(int L, int C, int F, int waves, bool bwd) {
    const int SA = da_stride(C > F ? C : F), SP = da_stride((L + 3) & ~3);
    return sizeof(float) * ((size_t)da_weight_floats(da_layout(C, F)) + (size_t)waves * da_wave_floats(L, SA, SP, bwd));
}

}  // namespace

extern "C" int stx_disp_attention_supported(int L, int C, int nhead, int F, int layers) { return da_supported(L, C, nhead, F, layers); }

extern "C" long long stx_disp_attention_bwd_workspace_floats(int N, int L, int C, int F) {
    if (N < 1 || L < 1 || L > DA_MAX_L || C < 4 || C > DA_MAX_C || (C & 3) || F < 4 || F > DA_MAX_C || (F & 3)) return 0;
    return (long long)((N + DA_UNIT - 1) / DA_UNIT) * da_layout(C, F).off[DA_NPRM];
}

extern "C" int stx_disp_attention_fwd(const float* x, const float* pe, const float* const* params, float* y, float* saved, const long long* seed,
                                      float p, float eps, int N, int L, int C, int nhead, int F, int layers, int hw, long long sb, long long sp,
                                      long long st, void* stream) {
    stx_begin();
    const char* what = "disp_attention_fwd";
    STX_REQUIRE(x && params && y, "%s: null pointer", what);
    if (int rc = da_check(what, N, L, C, nhead, F, layers, p, hw, sb, sp, st)) return rc;
    DaFwdArgs A;
    A.x = x; A.pe = pe; A.y = y; A.saved = saved; A.seed = seed;
    for (int l = 0; l < layers; ++l)
        for (int i = 0; i < DA_NPRM; ++i) {
            STX_REQUIRE(params[l * DA_NPRM + i], "%s: parameter %d of layer %d is NULL", what, i, l);
            A.prm[l].p[i] = params[l * DA_NPRM + i];
        }
    A.d = DaDims{N, L, C, F, nhead, C / nhead};
    A.v = DaView{hw, sb, sp, st};
    A.layers = layers;
    A.thr = seed ? da_threshold(p) : 0u;
    A.scale = (float)(1.0 / (1.0 - (double)p));
    A.eps = eps;
    // one workgroup per CU, as many waves as its LDS holds (nine at the model's size: 2304 sequences in flight, one round per image)
    int waves = DA_FWD_MAX_WAVES;
    while (waves > 1 && da_lds_bytes(L, C, F, waves, false) > STX_LDS_MAX) --waves;
    const size_t lds = da_lds_bytes(L, C, F, waves, false);
    if (int rc = stx_lds_require((const void*)disp_attention_fwd_kernel, lds, what)) return rc;
    int grid = stx_cdiv(N, waves);
    if (grid > DA_CUS) grid = DA_CUS;
    if (da_grid_override() > 0) grid = da_grid_override();
    hipLaunchKernelGGL(disp_attention_fwd_kernel, dim3((unsigned)grid), dim3(64 * waves), lds, (hipStream_t)stream, A);
    return stx_check_launch(what);
}

extern "C" int stx_disp_attention_bwd(const float* gy, const float* saved, const float* const* params, float* const* gparams, float* gx,
                                      float* gbuf, float* workspace, long long workspace_floats, const long long* seed, float p, float eps, int N,
                                      int L, int C, int nhead, int F, int layers, int hw, long long sb, long long sp, long long st, void* stream) {
    stx_begin();
    const char* what = "disp_attention_bwd";
    STX_REQUIRE(gy && saved && params && gparams, "%s: null pointer", what);
    if (int rc = da_check(what, N, L, C, nhead, F, layers, p, hw, sb, sp, st)) return rc;
    unsigned want[DA_MAX_LAYERS];
    int lowest = gx ? 0 : layers;
    for (int l = 0; l < layers; ++l) {
        want[l] = 0;
        for (int i = 0; i < DA_NPRM; ++i) {
            STX_REQUIRE(params[l * DA_NPRM + i], "%s: parameter %d of layer %d is NULL", what, i, l);
            if (gparams[l * DA_NPRM + i]) want[l] |= 1u << i;
        }
        if (want[l] && l < lowest) lowest = l;
    }
    STX_REQUIRE(lowest < layers, "%s: no gradient is wanted", what);
    STX_REQUIRE(layers == 1 || lowest == layers - 1 || gbuf, "%s: gbuf is NULL", what);
    const DaLay lay = da_layout(C, F);
    const int units = stx_cdiv(N, DA_UNIT);
    const long long need = (long long)units * lay.off[DA_NPRM];
    STX_REQUIRE(workspace && workspace_floats >= need, "%s: workspace of %lld floats, %lld needed", what, workspace_floats, need);
    int waves = DA_MAX_WAVES;
    while (waves > 1 && da_lds_bytes(L, C, F, waves, true) > STX_LDS_MAX) --waves;
    const size_t lds = da_lds_bytes(L, C, F, waves, true);
    if (int rc = stx_lds_require((const void*)disp_attention_bwd_kernel, lds, what)) return rc;
    int grid = stx_cdiv(units, waves);
    if (grid > DA_CUS) grid = DA_CUS;
    if (da_grid_override() > 0) grid = da_grid_override();
    const DaView view{hw, sb, sp, st}, dense{1, (long long)L * C, 0, (long long)C};
    const size_t per_layer = (size_t)N * L * C;
    for (int l = layers - 1; l >= lowest; --l) {
        DaBwdArgs A;
        A.xin = saved + l * per_layer;
        A.gout = l == layers - 1 ? gy : gbuf;
        A.gv = l == layers - 1 ? view : dense;
        A.gin = l == 0 ? gx : (l > lowest ? gbuf : nullptr);
        A.iv = l == 0 ? view : dense;
        A.slab = workspace;
        A.seed = seed;
        for (int i = 0; i < DA_NPRM; ++i) A.prm.p[i] = params[l * DA_NPRM + i];
        A.d = DaDims{N, L, C, F, nhead, C / nhead};
        A.layer = l;
        A.want = want[l];
        A.thr = seed ? da_threshold(p) : 0u;
        A.scale = (float)(1.0 / (1.0 - (double)p));
        A.eps = eps;
        hipLaunchKernelGGL(disp_attention_bwd_kernel, dim3((unsigned)grid), dim3(64 * waves), lds, (hipStream_t)stream, A);
        if (int rc = stx_check_launch(what)) return rc;
        if (want[l]) {
            DaOut out;
            for (int i = 0; i < DA_NPRM; ++i) out.p[i] = gparams[l * DA_NPRM + i];
            hipLaunchKernelGGL(disp_attention_reduce_kernel, dim3((unsigned)stx_cdiv(lay.off[DA_NPRM], 64)), dim3(256), 0, (hipStream_t)stream,
                               (const float*)workspace, units, C, F, out);
            if (int rc = stx_check_launch(what)) return rc;
        }
    }
    return STX_OK;
}

extern "C" int stx_disp_attention_masks(const long long* seed, float p, unsigned char* masks, int N, int L, int C, int F, int layers,
                                        void* stream) {
    stx_begin();
    const char* what = "disp_attention_masks";
    STX_REQUIRE(masks, "%s: null pointer", what);
    STX_REQUIRE(N >= 1 && L >= 1 && L <= DA_MAX_L && C >= 1 && C <= DA_MAX_C && F >= 1 && F <= DA_MAX_C && layers >= 1 && layers <= DA_MAX_LAYERS,
                "%s: N=%d L=%d C=%d ff=%d layers=%d outside the served range", what, N, L, C, F, layers);
    STX_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout probability %g outside [0, 1)", what, (double)p);
    const int Cm = C > F ? C : F;
    const size_t total = (size_t)layers * 3 * N * ((L + 3) / 4) * Cm;
    STX_REQUIRE(total < (1ull << 31), "%s: too many elements", what);
    hipLaunchKernelGGL(disp_attention_masks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed,
                       seed ? da_threshold(p) : 0u, masks, N, L, Cm, layers);
    return stx_check_launch(what);
}

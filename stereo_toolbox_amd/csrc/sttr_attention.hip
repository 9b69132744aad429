// STTR's attention with relative positional encoding (reference models/STTR/attention.py, `MultiheadAttentionRelative`), the
// core between the q/k/v projection and the output projection, forward and backward.
//
// The reference gathers the [2W-1, C] sine table into [W, W, C], projects it and forms three [B, E, W, W] einsums.  Because
// pos_indexes[w, v] = (W-1-w) + v, the projected rows are rows of two tables Qr, Kr [2W-1][E][16] and
//   S[b,e,w,v] = q[w].k[v] + q[w].Kr[r] + k[v].Qr[r],   r = W-1-w+v,   head dim 16,
// followed by the optional causal mask (v > w: -inf), the softmax over v and o = P v.  Nothing W x W exists here except the
// optional outputs raw = sum_e S (heads added in the order e = 0, 1, ...) and avg = mean_e P.
//
// Tiling.  One wave owns a 16 x 16 tile of S at a time; every product is v_mfma_f32_16x16x4_f32 (four per 16 x 16 x 16).  A lane
// is (a = lane & 15, g = lane >> 4): `a` indexes the OWNER side of the tile (the side the wave keeps: the 16 queries in the
// forward, dq and the table kernels; the 16 keys in the dk/dv kernel), its four registers r the other side, y = 4 g + r.  That is
// the MFMA's D layout with the owner along the columns, so a tile of P or dS is, register for register, the B operand of the
// next product (P v, dS k, ...) -- no transposition ever happens.  Operands are read straight from global memory as one float4
// per lane (row = lane & 15, columns 4 g .. 4 g + 3: the contraction index c is split as c = 4 g + step, the same on both
// operands), 16 rows of 64 contiguous bytes; k, v and the tables of one (row, head) are 27 KB at most and live in L1 / L2.
//   The positional terms are Toeplitz in the tile: with t = 15 - i + j (i the query, j the key inside the tile), r = Rb + t,
// Rb = W - 16 - w0 + v0, t in [0, 31).  The wave multiplies its query tile with the 32-row window Kr[Rb ..] and its key tile with
// Qr[Rb ..] (two 16 x 16 products each), leaves the results in its own LDS slab and reads them back skewed: [i][t], [j][t].
// LDS: 1376 floats per wave (two 16 x 32 products at strides 34 / 35 and a 16 x 16 tile of dS at stride 17), 22 KB per
// workgroup of four waves, static -- no dynamic LDS, and no limit on W from the LDS; W <= 431 is the matching head's limit.
//   Waves never wait for each other (no workgroup barrier): a causal wave stops at its diagonal tile.
//
// Forward: grid (ceil(W / 64), B), four waves of 16 queries; the heads are a loop INSIDE the wave so that raw / avg are added up
// by the one lane that owns the element, in head order.  Online softmax over the key tiles (the first tile holds key 0, never
// masked, so the running max is finite from the start); saved: row max and row sum per (b, e, w).
// Backward: S and P are recomputed from q, k, Qr, Kr and the saved statistics, dS = P o (dP - delta) + dRaw with
// delta = dO . o per row (a small kernel of its own), exactly 0 at masked entries.  Three sweeps, none of which uses an atomic:
//   dq      query-owner waves, as the forward;
//   dk, dv  key-owner waves (the tile transposed: the same code with the roles swapped);
//   dKr, dQr   query-owner waves over (query tile, head, chunk of rows b), the key tiles OUTSIDE the row loop: the two 16-row
//           chunks of each table a tile touches stay in registers across the rows; moving to the next key tile shifts the window
//           by 16, so the lower chunk is stored (once) and the upper becomes the lower.  Per wave that is one partial window of
//           (W16 + 1) x 16 rows per table; a last kernel adds the partials of every (chunk of rows, query tile) in a fixed order.
// Every result is bitwise reproducible.
#include "stx_common.h"

namespace {

constexpr int SA_MAX_W = 431;          // the matching head's limit (csrc/sttr_head.hip ST_MAX_W)
constexpr int SA_MAX_E = 8;
constexpr int SA_HD = 16;
constexpr int SA_WAVES = 4;
constexpr int SA_S1 = 34, SA_S2 = 35, SA_S3 = 17;                         // LDS row strides (floats): owner product, other product, dS
constexpr int SA_SLAB = 16 * SA_S1 + 16 * SA_S2 + 16 * SA_S3;

// LDS hand-over inside ONE wave (its own slab): the wave's LDS accesses complete in order; the statement keeps the compiler from
// moving them across it.  (The emulator runs lanes one after the other: there it is a rendezvous of the wave.)
#ifdef STX_HIPEMU
#define SA_WAVE_SYNC() hipemu::wave_sync_()
#else
#define SA_WAVE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif

__device__ __forceinline__ float sa_ninf() { return -__builtin_huge_valf(); }

__device__ __forceinline__ f32x4 sa_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct SaRow {
    float c[4];
};

// columns 4 g .. 4 g + 3 of row `row` (zeros outside [0, nrows)); base is 16-byte aligned, stride a multiple of 16 floats
__device__ __forceinline__ SaRow sa_row4(const float* base, int row, int nrows, size_t stride, int g) {
    SaRow o{{0.f, 0.f, 0.f, 0.f}};
    if (base && row >= 0 && row < nrows) {
        const float4 x = *reinterpret_cast<const float4*>(base + (size_t)row * stride + 4 * g);
        o.c[0] = x.x; o.c[1] = x.y; o.c[2] = x.z; o.c[3] = x.w;
    }
    return o;
}

__device__ __forceinline__ float sa_at(const float* base, int row, int nrows, size_t stride, int c) {
    return (row >= 0 && row < nrows) ? base[(size_t)row * stride + c] : 0.f;
}

// product of two 16 x 16 operand tiles: D[y = 4 g + r][a] = sum_c A[y][c] B[a][c]
__device__ __forceinline__ f32x4 sa_dot(const SaRow& A, const SaRow& B) {
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) d = sa_mfma(A.c[kk], B.c[kk], d);
    return d;
}

struct SaArgs {
    const float *q, *k, *v, *Qr, *Kr;  // q, k, v [W][B][E][16]; Qr, Kr [2W-1][E][16] or both NULL
    int W, B, E, causal;
};

// The 16 x 16 tile of S at queries w0 .., keys v0 .. of (b, e).  KEYS = false: the owner side (lane & 15) is the query, the
// registers the keys; KEYS = true: the other way round.  Masked entries (key >= W, causal key > query) and rows of queries
// >= W are -inf.  `slab` is the wave's LDS.  own / oth: the owner's and the other side's operand rows.
template <bool KEYS>
__device__ __forceinline__ f32x4 sa_scores(const SaArgs& p, int e, int w0, int v0, const SaRow& own, const SaRow& oth, float* slab, int lane) {
    const int a = lane & 15, g = lane >> 4;
    f32x4 s = sa_dot(oth, own);
    if (p.Qr) {
        const int nR = 2 * p.W - 1, Rb = p.W - 16 - w0 + v0;
        const size_t ts = (size_t)p.E * SA_HD;
        const float* tabO = (KEYS ? p.Qr : p.Kr) + (size_t)e * SA_HD;    // pairs with the owner: q . Kr, k . Qr
        const float* tabR = (KEYS ? p.Kr : p.Qr) + (size_t)e * SA_HD;
        float *TO = slab, *TR = slab + 16 * SA_S1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const SaRow to = sa_row4(tabO, Rb + 16 * h + a, nR, ts, g), tr = sa_row4(tabR, Rb + 16 * h + a, nR, ts, g);
            const f32x4 dO = sa_dot(to, own);                            // [t' = 4 g + r][owner a]
            const f32x4 dR = sa_dot(oth, tr);                            // [other 4 g + r][t' = a]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                TO[a * SA_S1 + 16 * h + 4 * g + r] = dO[r];
                TR[(4 * g + r) * SA_S2 + 16 * h + a] = dR[r];
            }
        }
        SA_WAVE_SYNC();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = 4 * g + r, t = KEYS ? 15 - y + a : 15 - a + y;
            const float fo = TO[a * SA_S1 + t], fr = TR[y * SA_S2 + t];
            s[r] = KEYS ? (s[r] + fr) + fo : (s[r] + fo) + fr;           // (q.k + q.Kr) + k.Qr, the reference's order
        }
        SA_WAVE_SYNC();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int w = w0 + (KEYS ? 4 * g + r : a), v = v0 + (KEYS ? a : 4 * g + r);
        if (w >= p.W || v >= p.W || (p.causal && v > w)) s[r] = sa_ninf();
    }
    return s;
}

__device__ __forceinline__ float sa_group_max(float x) {                  // over the four lanes that share lane & 15
    x = fmaxf(x, __shfl_xor(x, 16));
    return fmaxf(x, __shfl_xor(x, 32));
}

__device__ __forceinline__ float sa_group_sum(float x) {                  // every lane of the group ends with the same bits
    x += __shfl_xor(x, 16);
    return x + __shfl_xor(x, 32);
}

// ------------------------------------------------------------------------------------------------ forward
// grid (ceil(W / 64), B), 256 threads
__global__ __launch_bounds__(256) void sttr_attn_fwd_kernel(SaArgs p, float* __restrict__ o, float* raw, float* avg, float* __restrict__ stats) {
    __shared__ float lds[SA_WAVES * SA_SLAB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, g = lane >> 4;
    const int W = p.W, b = blockIdx.y, w0 = (blockIdx.x * SA_WAVES + wave) * 16;
    if (w0 >= W) return;
    float* slab = lds + wave * SA_SLAB;
    const size_t rs = (size_t)p.B * p.E * SA_HD;
    const int w = w0 + a, vend = (p.causal && w0 + 16 < W) ? w0 + 16 : W;
    for (int e = 0; e < p.E; ++e) {
        const size_t he = ((size_t)b * p.E + e) * SA_HD;
        const float *qh = p.q + he, *kh = p.k + he, *vh = p.v + he;
        const SaRow own = sa_row4(qh, w, W, rs, g);
        float m = sa_ninf(), lsum = 0.f;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};                                // o^T [c = 4 g + r][query a]
        for (int v0 = 0; v0 < vend; v0 += 16) {
            const SaRow oth = sa_row4(kh, v0 + a, W, rs, g);
            const f32x4 s = sa_scores<false>(p, e, w0, v0, own, oth, slab, lane);
            if (raw && w < W) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int v = v0 + 4 * g + r;
                    if (v < W) {
                        float* at = raw + ((size_t)b * W + w) * W + v;
                        *at = e ? *at + s[r] : s[r];
                    }
                }
            }
            const float mn = fmaxf(m, sa_group_max(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]))));
            const bool live = mn > sa_ninf();                            // (only rows of queries >= W are not)
            const float scale = live ? expf(m - mn) : 0.f;
            float pr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[r] = live ? expf(s[r] - mn) : 0.f;
            lsum = lsum * scale + sa_group_sum((pr[0] + pr[1]) + (pr[2] + pr[3]));
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] *= scale;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc = sa_mfma(sa_at(vh, v0 + 4 * g + kk, W, rs, a), pr[kk], acc);
            m = mn;
        }
        if (raw && w < W && e == 0)                                      // the tiles a causal wave never visits
            for (int v = vend + 4 * g; v < W; v += 16)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (v + r < W) raw[((size_t)b * W + w) * W + v + r] = sa_ninf();
        if (w < W) {
            const float inv = 1.f / lsum;
            *reinterpret_cast<float4*>(o + (size_t)w * rs + he + 4 * g) = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
            if (stats && g == 0) {
                stats[((size_t)b * p.E + e) * W + w] = m;
                stats[((size_t)p.B * p.E + (size_t)b * p.E + e) * W + w] = lsum;
            }
        }
        if (avg) {                                                       // the debugging output: a second sweep with the final statistics
            for (int v0 = 0; v0 < W; v0 += 16) {
                f32x4 s = {sa_ninf(), sa_ninf(), sa_ninf(), sa_ninf()};
                if (v0 < vend) s = sa_scores<false>(p, e, w0, v0, own, sa_row4(kh, v0 + a, W, rs, g), slab, lane);
                if (w >= W) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int v = v0 + 4 * g + r;
                    if (v >= W) continue;
                    float* at = avg + ((size_t)b * W + w) * W + v;
                    float x = expf(s[r] - m) / lsum;
                    if (e) x += *at;
                    *at = e == p.E - 1 ? x / (float)p.E : x;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
struct SaBwd {
    SaArgs p;
    const float *dO, *dRaw, *stats, *delta;                             // dO [W][B][E][16] or NULL, dRaw [B][W][W] or NULL
};

// delta[b][e][w] = dO[w][b][e] . o[w][b][e]
__global__ __launch_bounds__(256) void sttr_attn_delta_kernel(const float* __restrict__ dO, const float* __restrict__ o, float* __restrict__ delta,
                                                               int W, int B, int E) {
    const size_t n = (size_t)W * B * E, id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const int w = (int)(id % W);
    const size_t be = id / W;
    float acc = 0.f;
    if (dO) {
        const float *x = dO + ((size_t)w * B * E + be) * SA_HD, *y = o + ((size_t)w * B * E + be) * SA_HD;
#pragma unroll
        for (int c = 0; c < SA_HD; ++c) acc = fmaf(x[c], y[c], acc);
    }
    delta[id] = acc;
}

// dS of the tile whose scores are s.  dOq: the queries' rows of dO, vk: the keys' rows of v, given as (owner, other) like the
// scores' operands.  P is returned in pr.
template <bool KEYS>
__device__ __forceinline__ f32x4 sa_dscores(const SaBwd& d, int b, int e, int w0, int v0, const f32x4& s, const SaRow& ownG, const SaRow& othG,
                                             int lane, float* pr) {
    const int a = lane & 15, g = lane >> 4, W = d.p.W;
    f32x4 dp = {0.f, 0.f, 0.f, 0.f};
    if (d.dO) dp = sa_dot(othG, ownG);                                   // dO[w] . v[v]
    const size_t st = ((size_t)b * d.p.E + e) * W, half = (size_t)d.p.B * d.p.E * W;
    f32x4 ds;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int w = w0 + (KEYS ? 4 * g + r : a), v = v0 + (KEYS ? a : 4 * g + r);
        float x = 0.f, pp = 0.f;
        if (s[r] > sa_ninf()) {                                          // (masked entries, keys and queries >= W: exactly 0)
            pp = expf(s[r] - d.stats[st + w]) / d.stats[half + st + w];
            x = pp * (dp[r] - d.delta[st + w]);
            if (d.dRaw) x += d.dRaw[((size_t)b * W + w) * W + v];
        }
        pr[r] = pp;
        ds[r] = x;
    }
    return ds;
}

// acc[c = 4 g + r][owner a] += sum_t tab[Rb + t][c] dS(owner a, t): the positional half of dq (KEYS = false, tab = Kr) and of
// dk (KEYS = true, tab = Qr); dS of the tile goes through the wave's slab.
template <bool KEYS>
__device__ __forceinline__ f32x4 sa_pos_grad(const SaArgs& p, const float* tab, int Rb, const f32x4& ds, float* slab, int lane, f32x4 acc) {
    const int a = lane & 15, g = lane >> 4, nR = 2 * p.W - 1;
    const size_t ts = (size_t)p.E * SA_HD;
    float* D = slab + 16 * SA_S1 + 16 * SA_S2;
#pragma unroll
    for (int r = 0; r < 4; ++r) D[a * SA_S3 + 4 * g + r] = ds[r];
    SA_WAVE_SYNC();
#pragma unroll
    for (int step = 0; step < 8; ++step) {
        const int t = 4 * step + g, y = KEYS ? 15 + a - t : t - 15 + a;
        const float bv = (y >= 0 && y < 16) ? D[a * SA_S3 + y] : 0.f;
        acc = sa_mfma(sa_at(tab, Rb + t, nR, ts, a), bv, acc);
    }
    SA_WAVE_SYNC();
    return acc;
}

// dq: grid (ceil(W / 64), B)
__global__ __launch_bounds__(256) void sttr_attn_dq_kernel(SaBwd d, float* __restrict__ dq) {
    __shared__ float lds[SA_WAVES * SA_SLAB];
    const SaArgs& p = d.p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, g = lane >> 4;
    const int W = p.W, b = blockIdx.y, w0 = (blockIdx.x * SA_WAVES + wave) * 16;
    if (w0 >= W) return;
    float* slab = lds + wave * SA_SLAB;
    const size_t rs = (size_t)p.B * p.E * SA_HD;
    const int w = w0 + a, vend = (p.causal && w0 + 16 < W) ? w0 + 16 : W;
    for (int e = 0; e < p.E; ++e) {
        const size_t he = ((size_t)b * p.E + e) * SA_HD;
        const float *kh = p.k + he, *vh = p.v + he;
        const SaRow own = sa_row4(p.q + he, w, W, rs, g), ownG = sa_row4(d.dO ? d.dO + he : nullptr, w, W, rs, g);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};                                // dq^T [c = 4 g + r][query a]
        for (int v0 = 0; v0 < vend; v0 += 16) {
            const SaRow oth = sa_row4(kh, v0 + a, W, rs, g), othG = sa_row4(vh, v0 + a, W, rs, g);
            const f32x4 s = sa_scores<false>(p, e, w0, v0, own, oth, slab, lane);
            float pr[4];
            const f32x4 ds = sa_dscores<false>(d, b, e, w0, v0, s, ownG, othG, lane, pr);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc = sa_mfma(sa_at(kh, v0 + 4 * g + kk, W, rs, a), ds[kk], acc);
            if (p.Qr) acc = sa_pos_grad<false>(p, p.Kr + (size_t)e * SA_HD, W - 16 - w0 + v0, ds, slab, lane, acc);
        }
        if (w < W) *reinterpret_cast<float4*>(dq + (size_t)w * rs + he + 4 * g) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// dk, dv: grid (ceil(W / 64), B), a wave owns 16 keys
__global__ __launch_bounds__(256) void sttr_attn_dkv_kernel(SaBwd d, float* __restrict__ dk, float* __restrict__ dv) {
    __shared__ float lds[SA_WAVES * SA_SLAB];
    const SaArgs& p = d.p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, g = lane >> 4;
    const int W = p.W, b = blockIdx.y, v0 = (blockIdx.x * SA_WAVES + wave) * 16;
    if (v0 >= W) return;
    float* slab = lds + wave * SA_SLAB;
    const size_t rs = (size_t)p.B * p.E * SA_HD;
    const int v = v0 + a;
    for (int e = 0; e < p.E; ++e) {
        const size_t he = ((size_t)b * p.E + e) * SA_HD;
        const float *qh = p.q + he, *gh = d.dO ? d.dO + he : nullptr;
        const SaRow own = sa_row4(p.k + he, v, W, rs, g), ownG = sa_row4(p.v + he, v, W, rs, g);
        f32x4 ak = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};      // dk^T, dv^T [c = 4 g + r][key a]
        for (int w0 = p.causal ? v0 : 0; w0 < W; w0 += 16) {             // (causal: the queries of earlier tiles are all < v0)
            const SaRow oth = sa_row4(qh, w0 + a, W, rs, g), othG = sa_row4(gh, w0 + a, W, rs, g);
            const f32x4 s = sa_scores<true>(p, e, w0, v0, own, oth, slab, lane);
            float pr[4];
            const f32x4 ds = sa_dscores<true>(d, b, e, w0, v0, s, ownG, othG, lane, pr);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                ak = sa_mfma(sa_at(qh, w0 + 4 * g + kk, W, rs, a), ds[kk], ak);
                if (gh) av = sa_mfma(sa_at(gh, w0 + 4 * g + kk, W, rs, a), pr[kk], av);
            }
            if (p.Qr) ak = sa_pos_grad<true>(p, p.Qr + (size_t)e * SA_HD, W - 16 - w0 + v0, ds, slab, lane, ak);
        }
        if (v < W) {
            *reinterpret_cast<float4*>(dk + (size_t)v * rs + he + 4 * g) = make_float4(ak[0], ak[1], ak[2], ak[3]);
            *reinterpret_cast<float4*>(dv + (size_t)v * rs + he + 4 * g) = make_float4(av[0], av[1], av[2], av[3]);
        }
    }
}

// The partial windows of dKr (table 0) and dQr (table 1): part[task][table][(W16 + 1) * 16][16], task = (chunk of rows * E + e) *
// W16 + query tile; row x of a window of query tile qt is table row W - 16 - 16 qt + x.  One wave per task, four per workgroup.
__global__ __launch_bounds__(256) void sttr_attn_dtab_kernel(SaBwd d, float* __restrict__ part, int nb) {
    __shared__ float lds[SA_WAVES * SA_SLAB];
    const SaArgs& p = d.p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, g = lane >> 4;
    const int W = p.W, W16 = (W + 15) / 16;
    const long long task = (long long)blockIdx.x * SA_WAVES + wave;
    if (task >= (long long)nb * p.E * W16) return;
    const int qt = (int)(task % W16), e = (int)((task / W16) % p.E), bc = (int)(task / ((long long)W16 * p.E));
    const int b_lo = (int)((long long)bc * p.B / nb), b_hi = (int)((long long)(bc + 1) * p.B / nb), w0 = 16 * qt;
    float* slab = lds + wave * SA_SLAB;
    float* D = slab + 16 * SA_S1 + 16 * SA_S2;
    const size_t rs = (size_t)p.B * p.E * SA_HD;
    float* win = part + (size_t)task * 2 * (W16 + 1) * 256;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 kLo = zero, kHi = zero, qLo = zero, qHi = zero;                 // [t = 4 g + r][c = a] of the chunks Rb .. and Rb + 16 ..
    for (int vt = 0; vt < W16; ++vt) {
        const int v0 = 16 * vt;
        if (!(p.causal && v0 > w0 + 15)) {
            for (int b = b_lo; b < b_hi; ++b) {
                const size_t he = ((size_t)b * p.E + e) * SA_HD;
                const float *qh = p.q + he, *kh = p.k + he;
                const SaRow own = sa_row4(qh, w0 + a, W, rs, g), ownG = sa_row4(d.dO ? d.dO + he : nullptr, w0 + a, W, rs, g);
                const SaRow oth = sa_row4(kh, v0 + a, W, rs, g), othG = sa_row4(p.v + he, v0 + a, W, rs, g);
                const f32x4 s = sa_scores<false>(p, e, w0, v0, own, oth, slab, lane);
                float pr[4];
                const f32x4 ds = sa_dscores<false>(d, b, e, w0, v0, s, ownG, othG, lane, pr);
#pragma unroll
                for (int r = 0; r < 4; ++r) D[a * SA_S3 + 4 * g + r] = ds[r];        // [query a][key 4 g + r]
                SA_WAVE_SYNC();
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int x = 4 * kk + g;                            // the contraction index: a query for dKr, a key for dQr
                    const float bq = sa_at(qh, w0 + x, W, rs, a), bk = sa_at(kh, v0 + x, W, rs, a);
                    const int jl = a - 15 + x, jh = jl + 16;             // dKr[t] += dS[i = x][j = t - 15 + x] q[x]
                    const int il = 15 + x - a, ih = il - 16;             // dQr[t] += dS[i = 15 + x - t][j = x] k[x]
                    kLo = sa_mfma((jl >= 0 && jl < 16) ? D[x * SA_S3 + jl] : 0.f, bq, kLo);
                    kHi = sa_mfma((jh >= 0 && jh < 16) ? D[x * SA_S3 + jh] : 0.f, bq, kHi);
                    qLo = sa_mfma((il >= 0 && il < 16) ? D[il * SA_S3 + x] : 0.f, bk, qLo);
                    qHi = sa_mfma((ih >= 0 && ih < 16) ? D[ih * SA_S3 + x] : 0.f, bk, qHi);
                }
                SA_WAVE_SYNC();
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            win[(size_t)(16 * vt + 4 * g + r) * 16 + a] = kLo[r];
            win[(size_t)((W16 + 1) * 16 + 16 * vt + 4 * g + r) * 16 + a] = qLo[r];
        }
        kLo = kHi; kHi = zero;
        qLo = qHi; qHi = zero;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        win[(size_t)(16 * W16 + 4 * g + r) * 16 + a] = kLo[r];
        win[(size_t)((W16 + 1) * 16 + 16 * W16 + 4 * g + r) * 16 + a] = qLo[r];
    }
}

// dKr / dQr [2W-1][E][16] = the partial windows added in the order (chunk of rows, query tile); one thread per element
__global__ __launch_bounds__(256) void sttr_attn_tab_sum_kernel(const float* __restrict__ part, float* __restrict__ dKr, float* __restrict__ dQr,
                                                                 int W, int E, int nb) {
    const int nR = 2 * W - 1, W16 = (W + 15) / 16, rows = (W16 + 1) * 16;
    const size_t n = (size_t)2 * nR * E * SA_HD, id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const int c = (int)(id % SA_HD), e = (int)((id / SA_HD) % E), r = (int)((id / ((size_t)SA_HD * E)) % nR), tab = (int)(id / ((size_t)SA_HD * E * nR));
    float acc = 0.f;
    for (int bc = 0; bc < nb; ++bc)
        for (int qt = 0; qt < W16; ++qt) {
            const int x = r - (W - 16 - 16 * qt);
            if (x < 0 || x >= rows) continue;
            const size_t task = ((size_t)bc * E + e) * W16 + qt;
            acc += part[((task * 2 + tab) * rows + x) * 16 + c];
        }
    (tab ? dQr : dKr)[((size_t)r * E + e) * SA_HD + c] = acc;
}

// ------------------------------------------------------------------------------------------------ host side
int sa_shape_ok(int W, int B, int E, int head_dim, const char* what) {
    STX_REQUIRE(head_dim == SA_HD, "%s: head dim %d is not supported, only %d (embed_dim / num_heads)", what, head_dim, SA_HD);
    STX_REQUIRE(W >= 2 && W <= SA_MAX_W, "%s: W=%d outside 2..%d", what, W, SA_MAX_W);
    STX_REQUIRE(E >= 1 && E <= SA_MAX_E, "%s: %d heads outside 1..%d", what, E, SA_MAX_E);
    STX_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d rows outside 1..65535", what, B);
    return STX_OK;
}

long long sa_scratch_floats(int W, int B, int E, int nb, bool tables) {
    const long long W16 = (W + 15) / 16;
    return (long long)B * E * W + (tables ? (long long)nb * E * W16 * 2 * (W16 + 1) * 256 : 0);
}

}  // namespace

extern "C" int stx_sttr_attn_fwd(const float* q, const float* k, const float* v, const float* Qr, const float* Kr, int causal, float* o,
                                 float* raw, float* avg, float* stats, int W, int B, int E, int head_dim, void* stream) {
    stx_begin();
    const char* what = "sttr_attn_fwd";
    STX_REQUIRE(q && k && v && o, "%s: null pointer", what);
    STX_REQUIRE(!Qr == !Kr, "%s: Qr and Kr go together", what);
    if (int rc = sa_shape_ok(W, B, E, head_dim, what)) return rc;
    const SaArgs p{q, k, v, Qr, Kr, W, B, E, causal ? 1 : 0};
    hipLaunchKernelGGL(sttr_attn_fwd_kernel, dim3((unsigned)stx_cdiv(W, 64), (unsigned)B), dim3(256), 0, (hipStream_t)stream, p, o, raw, avg,
                       stats);
    return stx_check_launch(what);
}

extern "C" int stx_sttr_attn_bwd(const float* dO, const float* dRaw, const float* q, const float* k, const float* v, const float* Qr,
                                 const float* Kr, const float* o, const float* stats, int causal, float* dq, float* dk, float* dv, float* dQr,
                                 float* dKr, float* scratch, long long scratch_floats, int nb, int W, int B, int E, int head_dim,
                                 void* stream) {
    stx_begin();
    const char* what = "sttr_attn_bwd";
    STX_REQUIRE(q && k && v && o && stats && dq && dk && dv && scratch, "%s: null pointer", what);
    STX_REQUIRE(dO || dRaw, "%s: no gradient given", what);
    STX_REQUIRE(!Qr == !Kr && !Qr == !dQr && !Qr == !dKr, "%s: Qr, Kr, dQr and dKr go together", what);
    if (int rc = sa_shape_ok(W, B, E, head_dim, what)) return rc;
    STX_REQUIRE(nb >= 1 && nb <= B, "%s: %d chunks of rows outside 1..B=%d", what, nb, B);
    const long long need = sa_scratch_floats(W, B, E, nb, Qr != nullptr);
    STX_REQUIRE(scratch_floats >= need, "%s: scratch of %lld floats, %lld needed", what, scratch_floats, need);
    const SaBwd d{{q, k, v, Qr, Kr, W, B, E, causal ? 1 : 0}, dO, dRaw, stats, scratch};
    const hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)B * E * W;
    hipLaunchKernelGGL(sttr_attn_delta_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, dO, o, scratch, W, B, E);
    if (int rc = stx_check_launch(what)) return rc;
    const dim3 grid((unsigned)stx_cdiv(W, 64), (unsigned)B);
    hipLaunchKernelGGL(sttr_attn_dq_kernel, grid, dim3(256), 0, st, d, dq);
    if (int rc = stx_check_launch(what)) return rc;
    hipLaunchKernelGGL(sttr_attn_dkv_kernel, grid, dim3(256), 0, st, d, dk, dv);
    if (int rc = stx_check_launch(what)) return rc;
    if (Qr) {
        float* part = scratch + rows;
        const long long tasks = (long long)nb * E * ((W + 15) / 16);
        hipLaunchKernelGGL(sttr_attn_dtab_kernel, dim3((unsigned)((tasks + SA_WAVES - 1) / SA_WAVES)), dim3(256), 0, st, d, part, nb);
        if (int rc = stx_check_launch(what)) return rc;
        const size_t n = (size_t)2 * (2 * W - 1) * E * SA_HD;
        hipLaunchKernelGGL(sttr_attn_tab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)part, dKr, dQr, W, E,
                           nb);
        if (int rc = stx_check_launch(what)) return rc;
    }
    return STX_OK;
}

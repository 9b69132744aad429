// Selective recurrent unit of SelectiveStereo (reference SelectiveStereo/SelectiveRAFT/update.py:15-71, the same text in
// SelectiveIGEV/update.py) for gfx950: the 1x1 RaftConvGRU cell and the attention-weighted blend of the two cells,
//   h' = att h_s + (1 - att) h_l,   h_s = small_gru(h, x) (1x1),   h_l = large_gru(h, x) (3x3: convgru.hip, unchanged),
// forward and backward, on the exact fp32 MFMA v_mfma_f32_16x16x4_f32.
//
// Layout and source lists are those of convgru.hip: channels-last fp32 [B][H][W][C], the K axis a virtual concatenation of up
// to 4 sources (pointer, channels, pixel pitch); served: hidden a multiple of 16 up to 128, sources multiples of 4 channels,
// K = hidden + sum x up to 512.  A 1x1 convolution sees no neighbours, so pixels are one flat axis of P = B H W.
//
// GEMM kernel (stx_selgru_gemm): a plain [P x K] x [K x N] product.  A workgroup (4 waves) owns MT x 16 consecutive pixels
//   (MT = 8; 4 when the 8-row grid would leave compute units idle) and 4 N tiles of 16 channels, one per wave; further N slices
//   are grid.y.  K is walked in chunks of 32 channels staged in LDS as [MT x 16][40] (the pad keeps the ds_read_b128 operand
//   reads conflict-free and takes the over-read of a ragged last chunk).  Every chunk is one MFMA chain of 32 products from
//   zero, added to the running total on the VALU: an output is K / 32 short chains, as in the 3x3 kernel.
//   Epilogues: 0 raw: out = (acc + addend) + addend2;  1 zr: writes z, r h (and r);  2 q: writes h' (and q).  Pre-activations,
//   sigmoid, tanh and the convex update are formed in double and rounded once.  The q epilogue may blend with the other
//   cell's output in place: blend 1: out = att mine + (1 - att) other;  blend 2: out = att other + (1 - att) mine -- the
//   unrounded state of this cell, the blend in double, one rounding.
// Blend backward (stx_selgru_blend_bwd): g_s = att g, g_l = (1 - att) g and g_att[pixel] = sum_c g (h_s - h_l) with h_s, h_l
//   re-formed from the saved z, q and h; the channel sum runs in double in channel order.
// Weight gradient (stx_selgru_wgrad): dW[co][ci] = sum_pix src[pix][ci] g[pix][co]: 64-pixel tiles, 32 x 32 channel block
//   pairs, one 16 x 16 block per wave, partial sums of a pixel range in a slab, reduced in a fixed order in double.
// Bias gradients (stx_selgru_col_sum): column sums of gq, gz, gr in double, per-workgroup partials combined in block order.
// No float atomics anywhere: every result is bitwise reproducible.
#include "stx_common.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_CK = 32;          // concatenated channels per K chunk
constexpr int SG_PS = 40;          // floats per pixel slot of the LDS image (chunk + 8 pad)
constexpr int SG_MAX_SRC = 4;
constexpr int SG_MAX_HIDDEN = 128;
constexpr int SG_MAX_K = 512;
constexpr int SG_WPT = 64;         // pixels per tile of the weight gradient
constexpr int SG_WLS = 48;         // floats per pixel of its LDS tiles (16 mod 64 dwords: the 4 pixel rows of an operand read miss each other's banks)

struct SgSrc { const float* p; int c; int pitch; };
struct SgSrcs { SgSrc s[SG_MAX_SRC]; int n; int K; };

// source and channel offset of concatenated channel `vc` (< K)
__device__ __forceinline__ const float* sg_src_at(const SgSrcs& S, int vc, int& pitch) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < SG_MAX_SRC - 1; ++k)
        if (s == k && vc >= S.s[k].c) { vc -= S.s[k].c; s = k + 1; }
    pitch = S.s[s].pitch;
    return S.s[s].p + vc;
}

__device__ __forceinline__ f32x4 sg_zero4() {
    f32x4 z;
    z[0] = 0.f; z[1] = 0.f; z[2] = 0.f; z[3] = 0.f;
    return z;
}

int sg_groups(int K) { return (K + 15) / 16; }

// wp[group][nt][lane][j]: element kk = 4 (lane >> 4) + j of the group -> concatenated channel c = 16 group + kk (zero behind K),
// n = 16 nt + (lane & 15).  From one or two torch weights w[A][Bd] (1x1) stacked along A:
//   mode 0 (forward):       K = Bd,    N = nw A,  Wk[c][n] = w_{n / A}[n % A][c]
//   mode 1 (data gradient): K = nw A,  N = Bd,    Wk[c][n] = w_{c / A}[c % A][n]
__global__ __launch_bounds__(SG_THREADS) void sg_pack_kernel(const float* __restrict__ w0, const float* __restrict__ w1,
                                                             float* __restrict__ wp, int A, int Bd, int K, int N, int mode,
                                                             int NTall, long long total) {
    const long long idx = (long long)blockIdx.x * SG_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const long long r = idx >> 8;
    const int nt = (int)(r % NTall), g = (int)(r / NTall);
    const int c = 16 * g + 4 * (lane >> 4) + j, n = 16 * nt + (lane & 15);
    float v = 0.f;
    if (c < K && n < N) {
        if (mode == 0) {
            const float* w = n / A ? w1 : w0;
            v = w[(size_t)(n % A) * Bd + c];
        } else {
            const float* w = c / A ? w1 : w0;
            v = w[(size_t)(c % A) * Bd + n];
        }
    }
    wp[idx] = v;
}

struct SgGemmArgs {
    SgSrcs S;
    const float* wp;
    const float* bias0;     // channels [0, split)      (gate epilogues)
    const float* bias1;     // channels [split, N)      (zr)
    const float* add0;      // raw: addends [pix][add_pitch], added in this order (or null)
    const float* add1;
    const float* h;         // gate epilogues: the state
    const float* z;         // q epilogue
    const float* att;       // q epilogue with a blend: [pix]
    const float* other;     // ... the other cell's state [pix][split] (may be out0)
    float* out0;            // raw: out [pix][out_pitch]; zr: z; q: h'
    float* out1;            // zr: r h; q: q (or null)
    float* out2;            // zr: r (or null)
    int add0_pitch, add1_pitch, h_pitch, out_pitch;
    int N, split, epi, blend, NTall;
    long long P;
};

template <int MT>
__global__ __launch_bounds__(SG_THREADS, 2) void selgru_gemm_kernel(SgGemmArgs a) {
    STX_DYN_SMEM(smem);
    float* tile = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int nt = (int)blockIdx.y * 4 + wave;
    const bool active = nt < a.NTall;                                   // (wave-uniform; an idle wave still stages and syncs)
    const long long p0 = (long long)blockIdx.x * (MT * 16);
    const int K = a.S.K;
    const int nchunk = (K + SG_CK - 1) / SG_CK;
    const size_t wstep = (size_t)a.NTall * 256;
    const float* wl = a.wp + (size_t)(active ? nt : 0) * 256 + (size_t)lane * 4;

    f32x4 tot[MT];
#pragma unroll
    for (int mm = 0; mm < MT; ++mm) tot[mm] = sg_zero4();
    const int abase = i * SG_PS + 4 * kq;

    for (int ch = 0; ch < nchunk; ++ch) {
        const int c0 = ch * SG_CK;
        const int ck = K - c0 < SG_CK ? K - c0 : SG_CK;
        const int ng = (ck + 15) / 16;
        __syncthreads();                                                // every wave is done reading the previous chunk
        for (int e = tid; e < MT * 16 * (SG_PS / 4); e += SG_THREADS) {
            const int f = e % (SG_PS / 4), px = e / (SG_PS / 4);
            const int c = 4 * f;
            const long long pix = p0 + px;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < ck && pix < a.P) {
                int pitch;
                const float* p = sg_src_at(a.S, c0 + c, pitch);
                val = stx_ld4(p + (size_t)pix * pitch);
            }
            stx_st4(tile + px * SG_PS + c, val);
        }
        __syncthreads();
        if (active) {
            f32x4 acc[MT];
#pragma unroll
            for (int mm = 0; mm < MT; ++mm) acc[mm] = sg_zero4();
            for (int g = 0; g < ng; ++g) {
                const float4 bv = stx_ld4(wl + (size_t)(ch * 2 + g) * wstep);
                const float* tr = tile + 16 * g + abase;
#pragma unroll
                for (int mm = 0; mm < MT; ++mm) {
                    const float4 av = stx_ld4(tr + mm * 16 * SG_PS);
                    acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[mm], 0, 0, 0);
                    acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[mm], 0, 0, 0);
                    acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[mm], 0, 0, 0);
                    acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[mm], 0, 0, 0);
                }
            }
#pragma unroll
            for (int mm = 0; mm < MT; ++mm) tot[mm] += acc[mm];
        }
    }
    if (!active) return;

    // epilogue: accumulator register r of a lane = pixel 16 mm + 4 kq + r of the tile, channel 16 nt + i
    const int n = nt * 16 + i;
    if (n >= a.N) return;
    const bool second = n >= a.split;                                   // (wave-uniform: split is a multiple of 16)
    const int m = second ? n - a.split : n;
    const float* bias = second ? a.bias1 : a.bias0;
    const double bs = (a.epi != 0 && bias) ? (double)bias[m] : 0.0;
#pragma unroll
    for (int mm = 0; mm < MT; ++mm) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long pix = p0 + mm * 16 + 4 * kq + r;
            if (pix < a.P) {
                float v = tot[mm][r];
                if (a.epi == 0) {
                    if (a.add0) v = v + a.add0[(size_t)pix * a.add0_pitch + n];
                    if (a.add1) v = v + a.add1[(size_t)pix * a.add1_pitch + n];
                    a.out0[(size_t)pix * a.out_pitch + n] = v;
                } else {
                    const double pre = (double)v + bs;
                    const float hv = a.h[(size_t)pix * a.h_pitch + m];
                    const size_t o = (size_t)pix * a.split + m;
                    if (a.epi == 1) {
                        const float gate = (float)(1.0 / (1.0 + exp(-pre)));
                        if (!second) {
                            a.out0[o] = gate;
                        } else {
                            a.out1[o] = gate * hv;
                            if (a.out2) a.out2[o] = gate;
                        }
                    } else {
                        const float qv = (float)tanh(pre);
                        const float zv = a.z[o];
                        double mine = (1.0 - (double)zv) * (double)hv + (double)zv * (double)qv;
                        if (a.blend) {
                            const double av = (double)a.att[pix], ov = (double)a.other[o];
                            mine = a.blend == 1 ? av * mine + (1.0 - av) * ov : av * ov + (1.0 - av) * mine;
                        }
                        a.out0[o] = (float)mine;
                        if (a.out1) a.out1[o] = qv;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ blend backward
// Pixels [blockIdx.x * per_block, + per_block) by rpb = 256 / hidden pixel rows of `hidden` threads.
struct SgBlendArgs {
    const float* g; const float* att; const float* zs; const float* qs; const float* zl; const float* ql; const float* h;
    float* gs; float* gl; float* gatt;      // gatt null: att needs no gradient
    long long P, per_block;
    int g_pitch, h_pitch, hidden, rpb;
};

__global__ __launch_bounds__(SG_THREADS) void selgru_blend_bwd_kernel(SgBlendArgs a) {
    __shared__ double red[SG_THREADS];
    const int t = threadIdx.x, c = t % a.hidden, pr = t / a.hidden;
    const long long p_lo = (long long)blockIdx.x * a.per_block;
    const long long p_hi = p_lo + a.per_block < a.P ? p_lo + a.per_block : a.P;
    for (long long pb = p_lo; pb < p_hi; pb += a.rpb) {                 // (uniform over the workgroup)
        const long long p = pb + pr;
        const bool live = pr < a.rpb && p < p_hi;
        double d = 0.0;
        if (live) {
            const size_t o = (size_t)p * a.hidden + c;
            const float gv = a.g[(size_t)p * a.g_pitch + c], av = a.att[p];
            a.gs[o] = av * gv;
            a.gl[o] = (1.f - av) * gv;
            if (a.gatt) {
                const double hv = (double)a.h[(size_t)p * a.h_pitch + c];
                const double zs = (double)a.zs[o], zl = (double)a.zl[o];
                const double hs = (1.0 - zs) * hv + zs * (double)a.qs[o];
                const double hl = (1.0 - zl) * hv + zl * (double)a.ql[o];
                d = (double)gv * (hs - hl);
            }
        }
        if (a.gatt) {
            red[t] = d;
            __syncthreads();
            if (t < a.rpb && pb + t < p_hi) {
                double s = 0.0;
                for (int k = 0; k < a.hidden; ++k) s += red[t * a.hidden + k];
                a.gatt[pb + t] = (float)s;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------ weight gradient
struct SgWArgs {
    SgSrcs S;
    const float* g0; const float* g1;   // dense [pix][CG] each; g1 null: one map
    float* slab;                        // [pair][chunk][32 ci][32 co]
    int CG, CC;                         // channels of one map, of the stacked maps
    int ntiles, nchunks, ncfb;
    long long P;
};

__global__ __launch_bounds__(SG_THREADS, 2) void selgru_wgrad_kernel(SgWArgs a) {
    __shared__ __attribute__((aligned(16))) float xt[SG_WPT * SG_WLS];
    __shared__ __attribute__((aligned(16))) float gt[SG_WPT * SG_WLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int mi = wave >> 1, nj = wave & 1;                            // the wave's 16 x 16 block of the 32 ci x 32 co pair
    const int chunk = blockIdx.x, pair = blockIdx.y;
    const int cfb = pair % a.ncfb, ccb = pair / a.ncfb;
    const int t_lo = (int)((long long)a.ntiles * chunk / a.nchunks), t_hi = (int)((long long)a.ntiles * (chunk + 1) / a.nchunks);

    f32x4 acc[2];                                                       // even and odd pixel quads: two chains
    acc[0] = sg_zero4();
    acc[1] = sg_zero4();
    for (int t = t_lo; t < t_hi; ++t) {
        const long long p0 = (long long)t * SG_WPT;
        __syncthreads();                                                // every wave is done with the previous tile
        for (int e = tid; e < SG_WPT * 8 * 2; e += SG_THREADS) {
            const int which = e / (SG_WPT * 8), ee = e % (SG_WPT * 8);
            const int f = ee & 7, px = ee >> 3;
            const long long pix = p0 + px;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (which == 0) {
                const int c = cfb * 32 + 4 * f;
                if (c < a.S.K && pix < a.P) {
                    int pitch;
                    const float* p = sg_src_at(a.S, c, pitch);
                    val = stx_ld4(p + (size_t)pix * pitch);
                }
                stx_st4(xt + px * SG_WLS + 4 * f, val);
            } else {
                const int c = ccb * 32 + 4 * f;
                if (c < a.CC && pix < a.P) {
                    const float* gp = c >= a.CG ? a.g1 + (c - a.CG) : a.g0 + c;
                    val = stx_ld4(gp + (size_t)pix * a.CG);
                }
                stx_st4(gt + px * SG_WLS + 4 * f, val);
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SG_WPT / 4; ++s) {
            const float av = xt[(4 * s + kq) * SG_WLS + 16 * mi + i];
            const float bv = gt[(4 * s + kq) * SG_WLS + 16 * nj + i];
            acc[s & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[s & 1], 0, 0, 0);
        }
    }
    // accumulator register r: ci = 16 mi + 4 kq + r, co = 16 nj + i
    float* dst = a.slab + ((size_t)pair * a.nchunks + chunk) * 1024;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(16 * mi + 4 * kq + r) * 32 + 16 * nj + i] = acc[0][r] + acc[1][r];
}

// dW[co][ci] = sum over the chunks of the slab, in chunk order, in double
__global__ __launch_bounds__(SG_THREADS) void selgru_wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                                        int K, int CC, int nchunks, int ncfb, long long total) {
    const long long idx = (long long)blockIdx.x * SG_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int e = (int)(idx & 1023), pair = (int)(idx >> 10);
    const float* p = slab + (size_t)pair * nchunks * 1024 + e;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += (double)p[(size_t)c * 1024];
    const int co = (pair / ncfb) * 32 + (e & 31), ci = (pair % ncfb) * 32 + (e >> 5);
    if (co < CC && ci < K) dw[(size_t)co * K + ci] = (float)s;
}

// ------------------------------------------------------------------------------------------ bias gradients
// part[map][block][n] = sum over the block's pixels of map[pix][n], in double; thread = (pixel row, column)
struct SgColArgs {
    const float* m[3];
    double* part;
    long long P, per_block;
    int n, rpb;
};

__global__ __launch_bounds__(SG_THREADS) void selgru_col_sum_kernel(SgColArgs a) {
    __shared__ double red[SG_THREADS];
    const int t = threadIdx.x, c = t % a.n, pr = t / a.n;
    const float* src = a.m[blockIdx.y];
    const long long p_lo = (long long)blockIdx.x * a.per_block;
    const long long p_hi = p_lo + a.per_block < a.P ? p_lo + a.per_block : a.P;
    double s = 0.0;
    if (pr < a.rpb)
        for (long long p = p_lo + pr; p < p_hi; p += a.rpb) s += (double)src[(size_t)p * a.n + c];
    red[t] = s;
    __syncthreads();
    if (t < a.n) {
        for (int k = 1; k < a.rpb; ++k) s += red[k * a.n + t];
        a.part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.n + t] = s;
    }
}

// out[map][j] = (float) sum over the blocks of part[map][block][j], in block order
__global__ __launch_bounds__(SG_THREADS) void selgru_col_finish_kernel(const double* __restrict__ part, float* __restrict__ out,
                                                                      int blocks, int n, int total) {
    const int idx = blockIdx.x * SG_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int j = idx % n, map = idx / n;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[((size_t)map * blocks + b) * n + j];
    out[idx] = (float)s;
}

void sg_col_plan(long long P, int n, int* rpb, long long* per_block, int* blocks) {
    *rpb = SG_THREADS / n;
    long long pb = (P + 255) / 256;                                     // at most 256 workgroups per map
    const long long least = (long long)*rpb * 16;
    pb = pb < least ? least : pb;
    pb = (pb + *rpb - 1) / *rpb * *rpb;
    *per_block = pb;
    *blocks = (int)((P + pb - 1) / pb);
}

struct SgWPlan { int ncfb, npairs, nchunks; long long ntiles; };
SgWPlan sg_wplan(long long P, int K, int CC) {
    SgWPlan p;
    p.ntiles = (P + SG_WPT - 1) / SG_WPT;
    p.ncfb = stx_cdiv(K, 32);
    p.npairs = p.ncfb * stx_cdiv(CC, 32);
    long long n = 1024 / p.npairs;
    n = n < 1 ? 1 : n;
    p.nchunks = (int)(n > p.ntiles ? p.ntiles : n);
    return p;
}

// ------------------------------------------------------------------------------------------ host side
bool sg_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fills S from the flat C-ABI form; false: a malformed list
bool sg_sources(SgSrcs& S, const float* const* ptr, const int* ch, const int* pitch) {
    S.n = 0;
    S.K = 0;
    bool ended = false;
    for (int k = 0; k < SG_MAX_SRC; ++k) {
        S.s[k].p = nullptr; S.s[k].c = 0; S.s[k].pitch = 0;
        if (ch[k] == 0 && !ptr[k]) { ended = true; continue; }
        if (ended || !ptr[k] || ch[k] < 4 || ch[k] % 4 || pitch[k] < ch[k] || pitch[k] % 4 || !sg_aligned(ptr[k])) return false;
        S.s[k].p = ptr[k]; S.s[k].c = ch[k]; S.s[k].pitch = pitch[k];
        S.n = k + 1;
        S.K += ch[k];
    }
    return S.n >= 1 && S.K <= SG_MAX_K;
}

bool sg_hidden_ok(int hidden) { return hidden >= 16 && hidden <= SG_MAX_HIDDEN && hidden % 16 == 0; }

template <typename Kern, typename A>
int sg_launch(Kern kernel, dim3 grid, size_t lds, hipStream_t st, const A& args, const char* what) {
    if (int rc = stx_lds_require((const void*)kernel, lds, what)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(SG_THREADS), lds, st, args);
    return 0;
}

}  // namespace

// Whether the 1x1 cell serves hidden channels with nx x sources of cx0, cx1, cx2 channels (the limits of the 3x3 cell).
extern "C" int stx_selgru_supported(int hidden, int nx, int cx0, int cx1, int cx2) {
    stx_begin();
    if (!sg_hidden_ok(hidden) || nx < 1 || nx > SG_MAX_SRC - 1) return 0;
    const int cx[3] = {cx0, cx1, cx2};
    int K = hidden;
    for (int k = 0; k < 3; ++k) {
        if (k < nx) {
            if (cx[k] < 4 || cx[k] % 4) return 0;
            K += cx[k];
        } else if (cx[k] != 0) {
            return 0;
        }
    }
    return K <= SG_MAX_K ? 1 : 0;
}

// Floats of the packed 1x1 weights for GEMM-K = K concatenated channels and N output channels (0: unsupported).
extern "C" long long stx_selgru_packed_floats(int K, int N) {
    stx_begin();
    if (K < 4 || K > SG_MAX_K || K % 4 || N < 1 || N > SG_MAX_K) return 0;
    return (long long)sg_groups(K) * stx_cdiv(N, 16) * 256;
}

extern "C" int stx_selgru_pack_weight(const float* w0, const float* w1, float* wp, int A, int Bd, int mode, void* stream) {
    stx_begin();
    STX_REQUIRE(w0 && wp && A > 0 && Bd > 0, "selgru_pack_weight: bad args");
    STX_REQUIRE(mode == 0 || mode == 1, "selgru_pack_weight: mode %d", mode);
    const int nw = w1 ? 2 : 1;
    const int K = mode == 0 ? Bd : nw * A, N = mode == 0 ? nw * A : Bd;
    STX_REQUIRE(K >= 4 && K <= SG_MAX_K && K % 4 == 0 && N <= SG_MAX_K, "selgru_pack_weight: K=%d (a multiple of 4, <= %d) N=%d (<= %d)",
                K, SG_MAX_K, N, SG_MAX_K);
    const int NTall = stx_cdiv(N, 16);
    const long long total = (long long)sg_groups(K) * NTall * 256;
    hipLaunchKernelGGL(sg_pack_kernel, dim3((unsigned)((total + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0,
                       (hipStream_t)stream, w0, w1, wp, A, Bd, K, N, mode, NTall, total);
    return stx_check_launch("selgru_pack_weight");
}

extern "C" int stx_selgru_gemm(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                               const float* s3, int c3, int p3, const float* wp, int N, int epi, int split, const float* bias0,
                               const float* bias1, const float* add0, int add0_pitch, const float* add1, int add1_pitch,
                               const float* h, int h_pitch, const float* z, const float* att, const float* other, int blend,
                               float* out0, float* out1, float* out2, int out_pitch, long long P, void* stream) {
    stx_begin();
    STX_REQUIRE(wp && out0 && P > 0 && N > 0 && N <= SG_MAX_K, "selgru_gemm: bad shape");
    STX_REQUIRE(P < (1ll << 31), "selgru_gemm: %lld pixels too many", P);
    SgGemmArgs a;
    const float* ptr[4] = {s0, s1, s2, s3};
    const int ch[4] = {c0, c1, c2, c3}, pitch[4] = {p0, p1, p2, p3};
    STX_REQUIRE(sg_sources(a.S, ptr, ch, pitch), "selgru_gemm: sources must be 1..4 in a row, each 16-byte aligned with channels a "
                "multiple of 4, a pitch >= channels that is a multiple of 4, and at most %d channels together", SG_MAX_K);
    STX_REQUIRE(epi >= 0 && epi <= 2, "selgru_gemm: epilogue code %d", epi);
    STX_REQUIRE(blend >= 0 && blend <= 2 && (blend == 0 || (epi == 2 && att && other)),
                "selgru_gemm: blend %d needs the q epilogue, att and the other cell's state", blend);
    if (epi == 0) {
        split = N;
        STX_REQUIRE(out_pitch >= N && (!add0 || add0_pitch >= N) && (!add1 || add1_pitch >= N),
                    "selgru_gemm: raw epilogue, output / addend pitch below N=%d", N);
    } else {
        STX_REQUIRE(sg_hidden_ok(split) && N == (epi == 1 ? 2 * split : split),
                    "selgru_gemm: gate epilogue %d with N=%d hidden=%d (a multiple of 16, <= %d)", epi, N, split, SG_MAX_HIDDEN);
        STX_REQUIRE(h && h_pitch >= split, "selgru_gemm: gate epilogue needs h and a pitch >= hidden");
        STX_REQUIRE(epi == 1 ? out1 != nullptr : z != nullptr, "selgru_gemm: gate epilogue %d, missing operand", epi);
        STX_REQUIRE(out0 != h && out1 != h, "selgru_gemm: the output must not alias h");
    }
    a.wp = wp; a.bias0 = bias0; a.bias1 = bias1; a.add0 = add0; a.add1 = add1; a.h = h; a.z = z; a.att = att; a.other = other;
    a.out0 = out0; a.out1 = out1; a.out2 = out2;
    a.add0_pitch = add0_pitch; a.add1_pitch = add1_pitch; a.h_pitch = h_pitch; a.out_pitch = out_pitch;
    a.N = N; a.split = split; a.epi = epi; a.blend = blend; a.NTall = stx_cdiv(N, 16);
    a.P = P;
    const int slices = stx_cdiv(a.NTall, 4);
    // 8-row tiles unless they would leave most compute units without a workgroup
    const bool small = (P + 127) / 128 * slices < 256;
    const int MT = small ? 4 : 8;
    const long long tiles = (P + MT * 16 - 1) / (MT * 16);
    const size_t lds = (size_t)MT * 16 * SG_PS * 4;
    const dim3 grid((unsigned)tiles, slices);
    int rc;
    if (small) rc = sg_launch(selgru_gemm_kernel<4>, grid, lds, (hipStream_t)stream, a, "selgru_gemm");
    else rc = sg_launch(selgru_gemm_kernel<8>, grid, lds, (hipStream_t)stream, a, "selgru_gemm");
    if (rc) return rc;
    return stx_check_launch("selgru_gemm");
}

// g_s = att g, g_l = (1 - att) g [P][hidden] and, with gatt, gatt[P] = sum_c g (h_s - h_l)
extern "C" int stx_selgru_blend_bwd(const float* g, int g_pitch, const float* att, const float* zs, const float* qs, const float* zl,
                                    const float* ql, const float* h, int h_pitch, float* gs, float* gl, float* gatt, long long P,
                                    int hidden, void* stream) {
    stx_begin();
    STX_REQUIRE(g && att && gs && gl && P > 0, "selgru_blend_bwd: bad args");
    STX_REQUIRE(!gatt || (zs && qs && zl && ql && h), "selgru_blend_bwd: the gradient of att needs z, q of both cells and h");
    STX_REQUIRE(sg_hidden_ok(hidden) && g_pitch >= hidden && (!gatt || h_pitch >= hidden),
                "selgru_blend_bwd: hidden=%d (a multiple of 16, <= %d), pitches >= hidden", hidden, SG_MAX_HIDDEN);
    SgBlendArgs a = {};
    a.g = g; a.att = att; a.zs = zs; a.qs = qs; a.zl = zl; a.ql = ql; a.h = h; a.gs = gs; a.gl = gl; a.gatt = gatt;
    a.P = P; a.g_pitch = g_pitch; a.h_pitch = h_pitch; a.hidden = hidden;
    a.rpb = SG_THREADS / hidden;
    long long pb = (P + 1023) / 1024;                                   // at most 1024 workgroups
    const long long least = (long long)a.rpb * 8;
    pb = pb < least ? least : pb;
    a.per_block = (pb + a.rpb - 1) / a.rpb * a.rpb;
    const long long blocks = (P + a.per_block - 1) / a.per_block;
    hipLaunchKernelGGL(selgru_blend_bwd_kernel, dim3((unsigned)blocks), dim3(SG_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("selgru_blend_bwd");
}

extern "C" long long stx_selgru_wgrad_workspace_floats(long long P, int K, int CC) {
    stx_begin();
    if (P < 1 || P >= (1ll << 31) || K < 4 || K > SG_MAX_K || K % 4 || CC < 16 || CC > 2 * SG_MAX_HIDDEN || CC % 16) return 0;
    const SgWPlan p = sg_wplan(P, K, CC);
    return (long long)p.npairs * p.nchunks * 1024;
}

// dw[ng CG][K] from the source list (K concatenated channels) against the dense maps g0 (and g1) [P][CG]; workspace of
// stx_selgru_wgrad_workspace_floats(P, K, ng CG) floats.
extern "C" int stx_selgru_wgrad(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                                const float* s3, int c3, int p3, const float* g0, const float* g1, int CG, float* dw,
                                float* workspace, long long P, void* stream) {
    stx_begin();
    STX_REQUIRE(g0 && dw && workspace && P > 0, "selgru_wgrad: bad args");
    STX_REQUIRE(sg_hidden_ok(CG), "selgru_wgrad: %d gradient channels (a multiple of 16, <= %d)", CG, SG_MAX_HIDDEN);
    STX_REQUIRE(sg_aligned(g0) && sg_aligned(g1), "selgru_wgrad: gradient maps must be 16-byte aligned");
    STX_REQUIRE(P < (1ll << 31), "selgru_wgrad: %lld pixels too many", P);
    SgWArgs a;
    const float* ptr[4] = {s0, s1, s2, s3};
    const int ch[4] = {c0, c1, c2, c3}, pitch[4] = {p0, p1, p2, p3};
    STX_REQUIRE(sg_sources(a.S, ptr, ch, pitch), "selgru_wgrad: sources must be 1..4 in a row, each 16-byte aligned with channels a "
                "multiple of 4, a pitch >= channels that is a multiple of 4, and at most %d channels together", SG_MAX_K);
    a.g0 = g0; a.g1 = g1; a.slab = workspace; a.CG = CG; a.CC = g1 ? 2 * CG : CG;
    const SgWPlan p = sg_wplan(P, a.S.K, a.CC);
    a.ntiles = (int)p.ntiles; a.nchunks = p.nchunks; a.ncfb = p.ncfb; a.P = P;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(selgru_wgrad_kernel, dim3(p.nchunks, p.npairs), dim3(SG_THREADS), 0, st, a);
    const long long nout = (long long)p.npairs * 1024;
    hipLaunchKernelGGL(selgru_wgrad_reduce_kernel, dim3((unsigned)((nout + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, st,
                       (const float*)workspace, dw, a.S.K, a.CC, p.nchunks, p.ncfb, nout);
    return stx_check_launch("selgru_wgrad");
}

// Floats of the workspace of stx_selgru_col_sum (the kernels keep doubles there: 8-byte aligned; 0: unsupported).
extern "C" long long stx_selgru_col_sum_workspace_floats(long long P, int n) {
    stx_begin();
    if (P < 1 || P >= (1ll << 31) || !sg_hidden_ok(n)) return 0;
    int rpb, blocks;
    long long pb;
    sg_col_plan(P, n, &rpb, &pb, &blocks);
    return (long long)3 * blocks * n * 2;
}

// out[k][n] = the column sums of the dense maps m0, m1, m2 [P][n] (trailing ones may be NULL: fewer rows of out), summed in
// double in a fixed order and rounded once: the bias gradients of a cell from gq, gz, gr.
extern "C" int stx_selgru_col_sum(const float* m0, const float* m1, const float* m2, float* out, double* workspace, long long P, int n,
                                  void* stream) {
    stx_begin();
    STX_REQUIRE(m0 && out && workspace && P > 0 && P < (1ll << 31) && ((uintptr_t)workspace & 7) == 0 && (m1 || !m2), "selgru_col_sum: bad args");
    STX_REQUIRE(sg_hidden_ok(n), "selgru_col_sum: %d columns (a multiple of 16, <= %d)", n, SG_MAX_HIDDEN);
    SgColArgs a;
    a.m[0] = m0; a.m[1] = m1; a.m[2] = m2; a.part = workspace; a.P = P; a.n = n;
    const int maps = m2 ? 3 : (m1 ? 2 : 1);
    int blocks;
    sg_col_plan(P, n, &a.rpb, &a.per_block, &blocks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(selgru_col_sum_kernel, dim3(blocks, maps), dim3(SG_THREADS), 0, st, a);
    hipLaunchKernelGGL(selgru_col_finish_kernel, dim3(stx_cdiv(maps * n, SG_THREADS)), dim3(SG_THREADS), 0, st, (const double*)workspace,
                       out, blocks, n, maps * n);
    return stx_check_launch("selgru_col_sum");
}

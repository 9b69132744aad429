// ConvGRU cell of the iterative families (reference IGEVStereo/update.py:25-40; the same class in RAFTStereo, DEFOMStereo,
// StereoAnywhere and FoundationStereo) for gfx950: fused gates, forward and backward, on the exact fp32 MFMA
// v_mfma_f32_16x16x4_f32.
//
//   z = sigmoid(conv_z([h, x..]) + cz)   r = sigmoid(conv_r([h, x..]) + cr)   q = tanh(conv_q([r h, x..]) + cq)
//   h' = (1 - z) h + z q                 (3x3, padding 1, stride 1, with bias)
//
// Layout: channels-last fp32 [B][H][W][C].  The K axis of a convolution is a VIRTUAL concatenation: a launch takes up to 4
// "sources" (device pointer, channels, pixel pitch in floats); no cat is materialised, and a channel slice of a wider
// map (pitch > channels) is consumed as it is.  Served (stx_convgru_supported): hidden a multiple of 16 up to 128, every
// source a multiple of 4 channels, at most 4 sources (h / r h and up to three x), K = hidden + sum x up to 512, kernel 3x3.
//
// GEMM kernel (stx_convgru_gemm): M = pixels, N = output channels, K = 9 taps x concatenated channels.
//   A workgroup (4 waves) owns a tile of MT x 16 pixels (MT = 8; 4 when the 8-row grid would leave compute units idle) and
//   4 N tiles of 16 channels, one per wave; further N slices are grid.y.  Each wave multiplies all MT pixel rows with its own
//   N tile, so a packed-weight float is fetched once per workgroup; weights stream from L2 one K group ahead.
//   K is walked in chunks of 32 concatenated channels: the chunk's halo image [MT + 2][18][40] sits in LDS -- 32 channels and
//   8 pad floats per pixel, the pad makes the ds_read_b128 operand reads (16 pixels x 4 k-quarters) conflict-free and takes
//   the over-read of a ragged last chunk (zero weights meet zeroed pad).  A chunk is 9 taps x (1 or 2) groups of 16 floats.
//   Sums are blocked: every (chunk, tap row) is one MFMA chain of at most 96 products from zero, added to the running total
//   on the VALU -- an output is K / 32 x 3 short chains, not one chain of 9 K products (3456 for hidden 128 + 256).
//   Epilogues: 0 raw: out = acc (+ addend);  1 zr: N = 2 hidden, z | r stacked, writes z, r h (and r);  2 q: writes h' (and
//   q).  Pre-activations are summed and the sigmoid / tanh formed in double: the final rounding is the only error left.
//   The data gradients are the same kernel with the raw epilogue on mode-1 weights (flipped taps, transposed channels).
// Streaming kernels: gate backward (gq, gz), reset backward (gr and the running dL/dh), both with per-workgroup partial rows
//   of the bias gradients, and a fixed-order row reduction.
// Weight gradient: dW[co][ci][tap] = sum_pix src[pix + tap - 1][ci] g[pix][co] over the source list against one or two dense
//   gradient maps (gz | gr stacked), the scheme of conv3d_axial.hip's planar weight gradient: 16 x 16 pixel tiles, 32 x 32
//   channel block pairs, taps dealt to the waves, partial sums in a slab, reduced in a fixed order.
// No float atomics anywhere: every result is bitwise reproducible.
#include "stx_common.h"

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_CK = 32;          // concatenated channels per K chunk
constexpr int CG_PS = 40;          // floats per pixel slot of the LDS image (chunk + 8 pad)
constexpr int CG_LV = 18;          // pixels per line (16 + halo)
constexpr int CG_GPC = 18;         // K groups of a full chunk (9 taps x 2)
constexpr int CG_MAX_SRC = 4;
constexpr int CG_MAX_HIDDEN = 128;
constexpr int CG_MAX_K = 512;

struct CgSrc { const float* p; int c; int pitch; };
struct CgSrcs { CgSrc s[CG_MAX_SRC]; int n; int K; };

// source and channel offset of concatenated channel `vc` (< K)
__device__ __forceinline__ const float* cg_src_at(const CgSrcs& S, int vc, int& pitch) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < CG_MAX_SRC - 1; ++k)
        if (s == k && vc >= S.s[k].c) { vc -= S.s[k].c; s = k + 1; }
    pitch = S.s[s].pitch;
    return S.s[s].p + vc;
}

__device__ __forceinline__ f32x4 cg_zero4() {
    f32x4 z;
    z[0] = 0.f; z[1] = 0.f; z[2] = 0.f; z[3] = 0.f;
    return z;
}

int cg_groups(int K) {             // K groups of the packed weights: full chunks, then the ragged one
    const int full = K / CG_CK, rest = K % CG_CK;
    return full * CG_GPC + 9 * ((rest + 15) / 16);
}

// wp[group][nt][lane][j]: group = chunk * 18 + tap * ng + g (ng = groups of 16 in the chunk), element kk = 16 g + 4 (lane >> 4) + j
// -> concatenated channel c = 32 chunk + kk (zero behind the chunk's end), n = 16 nt + (lane & 15).  From one or two torch
// weights w[A][Bd][3][3] stacked along A:
//   mode 0 (forward):       K = Bd,    N = nw A,  Wk[tap][c][n] = w_{n / A}[n % A][c][tap]
//   mode 1 (data gradient): K = nw A,  N = Bd,    Wk[tap][c][n] = w_{c / A}[c % A][n][8 - tap]
__global__ __launch_bounds__(CG_THREADS) void cg_pack_kernel(const float* __restrict__ w0, const float* __restrict__ w1,
                                                             float* __restrict__ wp, int A, int Bd, int K, int N, int mode,
                                                             int NTall, long long total) {
    const long long idx = (long long)blockIdx.x * CG_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    const long long r = idx >> 8;
    const int nt = (int)(r % NTall), gs = (int)(r / NTall);
    const int chunk = gs / CG_GPC, within = gs - chunk * CG_GPC;
    const int ck = K - chunk * CG_CK < CG_CK ? K - chunk * CG_CK : CG_CK;
    const int ng = (ck + 15) / 16;
    const int tap = within / ng, g = within - tap * ng;
    const int kk = 16 * g + 4 * (lane >> 4) + j, c = chunk * CG_CK + kk, n = 16 * nt + (lane & 15);
    float v = 0.f;
    if (kk < ck && n < N) {
        if (mode == 0) {
            const float* w = n / A ? w1 : w0;
            v = w[((size_t)(n % A) * Bd + c) * 9 + tap];
        } else {
            const float* w = c / A ? w1 : w0;
            v = w[((size_t)(c % A) * Bd + n) * 9 + (8 - tap)];
        }
    }
    wp[idx] = v;
}

struct CgGemmArgs {
    CgSrcs S;
    const float* wp;
    const float* bias0;     // channels [0, split)      (gate epilogues)
    const float* bias1;     // channels [split, N)      (zr)
    const float* add0;      // raw: addend [pix][add0_pitch]; zr: cz; q: cq  (or null)
    const float* add1;      // zr: cr (or null)
    const float* h;         // gate epilogues: the state at the centre pixel
    const float* z;         // q epilogue
    float* out0;            // raw: out [pix][out_pitch]; zr: z; q: h'
    float* out1;            // zr: r h; q: q (or null)
    float* out2;            // zr: r (or null)
    int add0_pitch, add1_pitch, h_pitch, out_pitch;
    int N, split, epi, NTall;
    int H, W, nTH, nTW;
};

template <int MT>
__global__ __launch_bounds__(CG_THREADS, 2) void convgru_gemm_kernel(CgGemmArgs a) {
    STX_DYN_SMEM(smem);
    float* tile = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int nt = (int)blockIdx.y * 4 + wave;
    const bool active = nt < a.NTall;                                   // (wave-uniform; an idle wave still stages and syncs)
    int b, h0, w0;
    {
        const int t = blockIdx.x;
        const int tw = t % a.nTW, th = (t / a.nTW) % a.nTH;
        b = t / (a.nTW * a.nTH);
        h0 = th * MT;
        w0 = tw * 16;
    }
    constexpr int NL = MT + 2;
    const int K = a.S.K;
    const int nchunk = (K + CG_CK - 1) / CG_CK;
    const int total_groups = (K / CG_CK) * CG_GPC + 9 * (((K % CG_CK) + 15) / 16);
    const size_t wstep = (size_t)a.NTall * 256;
    const float* wl = a.wp + (size_t)(active ? nt : 0) * 256 + (size_t)lane * 4;

    f32x4 tot[MT];
#pragma unroll
    for (int mm = 0; mm < MT; ++mm) tot[mm] = cg_zero4();
    const int abase = i * CG_PS + 4 * kq;

    for (int ch = 0; ch < nchunk; ++ch) {
        const int c0 = ch * CG_CK;
        const int ck = K - c0 < CG_CK ? K - c0 : CG_CK;
        const int ng = (ck + 15) / 16;
        __syncthreads();                                                // every wave is done reading the previous chunk
        for (int e = tid; e < NL * CG_LV * (CG_PS / 4); e += CG_THREADS) {
            const int f = e % (CG_PS / 4), lv = e / (CG_PS / 4);
            const int px = lv % CG_LV, l = lv / CG_LV;
            const int hh = h0 - 1 + l, ww = w0 - 1 + px, c = 4 * f;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < ck && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) {
                int pitch;
                const float* p = cg_src_at(a.S, c0 + c, pitch);
                val = stx_ld4(p + ((size_t)b * a.H + hh) * a.W * pitch + (size_t)ww * pitch);
            }
            stx_st4(tile + lv * CG_PS + c, val);
        }
        __syncthreads();
        if (active) {
            int gs = ch * CG_GPC;                                       // this chunk's first K group
            float4 bcur = stx_ld4(wl + (size_t)gs * wstep);
#pragma unroll 1
            for (int kh = 0; kh < 3; ++kh) {
                f32x4 acc[MT];
#pragma unroll
                for (int mm = 0; mm < MT; ++mm) acc[mm] = cg_zero4();
                for (int s = 0; s < 3 * ng; ++s) {
                    const int kw = s / ng, g = s - kw * ng;
                    ++gs;                                               // the next group's weights (behind the last: the last again)
                    const float4 bnxt = stx_ld4(wl + (size_t)(gs < total_groups ? gs : total_groups - 1) * wstep);
                    const float* tr = tile + (kh * CG_LV + kw) * CG_PS + 16 * g + abase;
#pragma unroll
                    for (int mm = 0; mm < MT; ++mm) {
                        const float4 av = stx_ld4(tr + mm * CG_LV * CG_PS);
                        acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bcur.x, acc[mm], 0, 0, 0);
                        acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bcur.y, acc[mm], 0, 0, 0);
                        acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bcur.z, acc[mm], 0, 0, 0);
                        acc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bcur.w, acc[mm], 0, 0, 0);
                    }
                    bcur = bnxt;
                }
#pragma unroll
                for (int mm = 0; mm < MT; ++mm) tot[mm] += acc[mm];
            }
        }
    }
    if (!active) return;

    // epilogue: accumulator register r of a lane = pixel 4 kq + r of row mm, channel 16 nt + i
    const int n = nt * 16 + i;
    if (n >= a.N) return;
    const bool second = n >= a.split;                                   // (wave-uniform: split is a multiple of 16)
    const int m = second ? n - a.split : n;
    const float* bias = second ? a.bias1 : a.bias0;
    const float* add = second ? a.add1 : a.add0;
    const int add_pitch = second ? a.add1_pitch : a.add0_pitch;
    const double bs = (a.epi != 0 && bias) ? (double)bias[m] : 0.0;
#pragma unroll
    for (int mm = 0; mm < MT; ++mm) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int hh = h0 + mm, ww = w0 + 4 * kq + r;
            if (hh < a.H && ww < a.W) {
                const size_t pix = ((size_t)b * a.H + hh) * a.W + ww;
                const float v = tot[mm][r];
                if (a.epi == 0) {
                    a.out0[pix * a.out_pitch + n] = a.add0 ? v + a.add0[pix * a.add0_pitch + n] : v;
                } else {
                    const double pre = (double)v + bs + (add ? (double)add[pix * add_pitch + m] : 0.0);
                    const float hv = a.h[pix * a.h_pitch + m];
                    const size_t o = pix * a.split + m;
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
                        a.out0[o] = (float)((1.0 - (double)zv) * (double)hv + (double)zv * (double)qv);
                        if (a.out1) a.out1[o] = qv;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ streaming backward
// Pixels [blockIdx.x * per_block, + per_block) by rpb = 256 / hidden pixel rows of `hidden` threads; bias partials of the
// workgroup are summed over its pixel rows in a fixed order.
struct CgGateArgs {
    const float* g; const float* z; const float* q; const float* r; const float* h;
    float* buf;        // reset backward: running [dL/dh | g_x] rows of buf_pitch floats, first `hidden` = g_rh on entry
    float* o0;         // gate: gq; reset: gr
    float* o1;         // gate: gz
    float* rows;       // gate: [blocks][2][hidden] (gq | gz); reset: [blocks][hidden]; or null
    long long P, per_block;
    int g_pitch, h_pitch, buf_pitch, hidden, rpb;
};

template <int RESET>
__global__ __launch_bounds__(CG_THREADS) void convgru_gate_bwd_kernel(CgGateArgs a) {
    __shared__ float red[2 * CG_THREADS];
    const int t = threadIdx.x, c = t % a.hidden, pr = t / a.hidden;
    const long long p_lo = (long long)blockIdx.x * a.per_block;
    const long long p_hi = p_lo + a.per_block < a.P ? p_lo + a.per_block : a.P;
    float s0 = 0.f, s1 = 0.f;
    if (pr < a.rpb) {
        for (long long p = p_lo + pr; p < p_hi; p += a.rpb) {
            const size_t o = (size_t)p * a.hidden + c;
            const float gv = a.g[(size_t)p * a.g_pitch + c], zv = a.z[o], hv = a.h[(size_t)p * a.h_pitch + c];
            if (RESET) {
                float* bp = a.buf + (size_t)p * a.buf_pitch + c;
                const float grh = *bp, rv = a.r[o];
                const float gr = grh * hv * rv * (1.f - rv);
                a.o0[o] = gr;
                *bp = gv * (1.f - zv) + grh * rv;
                s0 += gr;
            } else {
                const float qv = a.q[o];
                const float gq = gv * zv * (1.f - qv * qv);
                const float gz = gv * (qv - hv) * zv * (1.f - zv);
                a.o0[o] = gq;
                a.o1[o] = gz;
                s0 += gq;
                s1 += gz;
            }
        }
    }
    if (!a.rows) return;                                                // (uniform over the launch)
    red[t] = s0;
    red[CG_THREADS + t] = s1;
    __syncthreads();
    if (t < a.hidden) {
        float t0 = 0.f, t1 = 0.f;
        for (int k = 0; k < a.rpb; ++k) {
            t0 += red[k * a.hidden + t];
            t1 += red[CG_THREADS + k * a.hidden + t];
        }
        if (RESET) {
            a.rows[(size_t)blockIdx.x * a.hidden + t] = t0;
        } else {
            a.rows[((size_t)blockIdx.x * 2) * a.hidden + t] = t0;
            a.rows[((size_t)blockIdx.x * 2 + 1) * a.hidden + t] = t1;
        }
    }
}

// out[j] = sum over the rows of rows[row][n], in row order
__global__ __launch_bounds__(CG_THREADS) void convgru_row_sum_kernel(const float* __restrict__ rows, float* __restrict__ out,
                                                                    int nrows, int n) {
    const int j = blockIdx.x * CG_THREADS + threadIdx.x;
    if (j >= n) return;
    float s = 0.f;
    for (int r = 0; r < nrows; ++r) s += rows[(size_t)r * n + j];
    out[j] = s;
}

void cg_stream_plan(long long P, int hidden, int* rpb, long long* per_block, int* blocks) {
    *rpb = CG_THREADS / hidden;
    long long pb = (P + 511) / 512;                                     // at most 512 workgroups
    const long long least = (long long)*rpb * 16;
    pb = pb < least ? least : pb;
    pb = (pb + *rpb - 1) / *rpb * *rpb;
    *per_block = pb;
    *blocks = (int)((P + pb - 1) / pb);
}

// ------------------------------------------------------------------------------------------ weight gradient
constexpr int CG_WXLS = 18 * 32 + 16;   // x tile: 18 lines of 18 pixels x 32 channels, line stride = 16 mod 32 dwords
constexpr int CG_WGLS = 16 * 32 + 16;   // g tile: 16 lines of 16 pixels x 32 channels

struct CgWArgs {
    CgSrcs S;
    const float* g0; const float* g1;   // dense [pix][CG] each; g1 null: one map
    float* slab;                        // [pair][chunk][tap][32 ci][32 co]
    int CG, CC;                         // channels of one map, of the stacked maps
    int H, W, nA, nB, ntiles, nchunks, ncfb;
};

__global__ __launch_bounds__(CG_THREADS, 2) void convgru_wgrad_kernel(CgWArgs a) {
    STX_DYN_SMEM(smem);
    float* xt = reinterpret_cast<float*>(smem);
    float* gt = xt + 18 * CG_WXLS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x, pair = blockIdx.y;
    const int cfb = pair % a.ncfb, ccb = pair / a.ncfb;
    const int t_lo = (int)((long long)a.ntiles * chunk / a.nchunks), t_hi = (int)((long long)a.ntiles * (chunk + 1) / a.nchunks);

    f32x4 acc[3][2][2];                                                 // tap = wave + 4 k
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) acc[k][mi][nj] = cg_zero4();

    for (int t = t_lo; t < t_hi; ++t) {
        const int tb = t % a.nB, ta = (t / a.nB) % a.nA, b = t / (a.nB * a.nA);
        const int o1 = ta * 16, o2 = tb * 16;
        __syncthreads();                                                // every wave is done with the previous tile
        for (int e = tid; e < 18 * 18 * 8; e += CG_THREADS) {
            const int f = e & 7, lv = e >> 3;
            const int v = lv % 18, l = lv / 18;
            const int c = cfb * 32 + 4 * f;
            const int hh = o1 - 1 + l, ww = o2 - 1 + v;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < a.S.K && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) {
                int pitch;
                const float* p = cg_src_at(a.S, c, pitch);
                val = stx_ld4(p + (((size_t)b * a.H + hh) * a.W + ww) * pitch);
            }
            stx_st4(xt + l * CG_WXLS + v * 32 + 4 * f, val);
        }
        for (int e = tid; e < 16 * 16 * 8; e += CG_THREADS) {
            const int f = e & 7, lv = e >> 3;
            const int v = lv & 15, l = lv >> 4;
            const int c = ccb * 32 + 4 * f;
            const int hh = o1 + l, ww = o2 + v;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < a.CC && hh < a.H && ww < a.W) {
                const float* gp = c >= a.CG ? a.g1 + (c - a.CG) : a.g0 + c;
                val = stx_ld4(gp + (((size_t)b * a.H + hh) * a.W + ww) * a.CG);
            }
            stx_st4(gt + l * CG_WGLS + v * 32 + 4 * f, val);
        }
        __syncthreads();
        for (int pos = 0; pos < 16; ++pos) {
#pragma unroll
            for (int lg = 0; lg < 4; ++lg) {
                const float* gp = gt + (4 * lg + kq) * CG_WGLS + pos * 32 + i;
                const float b0 = gp[0], b1 = gp[16];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int tap = wave + 4 * k;                       // (wave-uniform)
                    if (tap < 9) {
                        const int dl = tap / 3, dp = tap % 3;
                        const float* xp = xt + (4 * lg + kq + dl) * CG_WXLS + (pos + dp) * 32 + i;
                        const float a0 = xp[0], a1 = xp[16];
                        acc[k][0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[k][0][0], 0, 0, 0);
                        acc[k][0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[k][0][1], 0, 0, 0);
                        acc[k][1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[k][1][0], 0, 0, 0);
                        acc[k][1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[k][1][1], 0, 0, 0);
                    }
                }
            }
        }
    }
    // accumulator register r: ci = 16 mi + 4 kq + r, co = 16 nj + i
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int tap = wave + 4 * k;
        if (tap < 9) {
            float* dst = a.slab + (((size_t)pair * a.nchunks + chunk) * 9 + tap) * 1024;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(16 * mi + 4 * kq + r) * 32 + 16 * nj + i] = acc[k][mi][nj][r];
        }
    }
}

// dW[co][ci][tap] = sum over the chunks of the slab in a fixed order: a workgroup owns 64 consecutive elements of
// [pair][tap][32 ci][32 co]; its four waves take every fourth chunk, then one LDS round.
__global__ __launch_bounds__(CG_THREADS) void convgru_wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                                         int K, int CC, int nchunks, int ncfb) {
    __shared__ float red[4][64];
    const int part = threadIdx.x >> 6, o = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * 64 + o;
    const int e = (int)(idx & 1023);
    const int tap = (int)((idx >> 10) % 9), pair = (int)((idx >> 10) / 9);
    const float* p = slab + ((size_t)pair * nchunks * 9 + tap) * 1024 + e;
    float s = 0.f;
    for (int c = part; c < nchunks; c += 4) s += p[(size_t)c * 9 * 1024];
    red[part][o] = s;
    __syncthreads();
    if (part == 0) {
        const float t = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
        const int co = (pair / ncfb) * 32 + (e & 31), ci = (pair % ncfb) * 32 + (e >> 5);
        if (co < CC && ci < K) dw[((size_t)co * K + ci) * 9 + tap] = t;
    }
}

struct CgWPlan { int nA, nB, ncfb, npairs, nchunks; long long ntiles; };
CgWPlan cg_wplan(int B, int H, int W, int K, int CC) {
    CgWPlan p;
    p.nA = stx_cdiv(H, 16);
    p.nB = stx_cdiv(W, 16);
    p.ntiles = (long long)B * p.nA * p.nB;
    p.ncfb = stx_cdiv(K, 32);
    p.npairs = p.ncfb * stx_cdiv(CC, 32);
    long long n = 1024 / p.npairs;
    n = n < 1 ? 1 : n;
    p.nchunks = (int)(n > p.ntiles ? p.ntiles : n);
    return p;
}

// ------------------------------------------------------------------------------------------ host side
bool cg_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fills S from the flat C-ABI form; false: a malformed list
bool cg_sources(CgSrcs& S, const float* const* ptr, const int* ch, const int* pitch) {
    S.n = 0;
    S.K = 0;
    bool ended = false;
    for (int k = 0; k < CG_MAX_SRC; ++k) {
        S.s[k].p = nullptr; S.s[k].c = 0; S.s[k].pitch = 0;
        if (ch[k] == 0 && !ptr[k]) { ended = true; continue; }
        if (ended || !ptr[k] || ch[k] < 4 || ch[k] % 4 || pitch[k] < ch[k] || pitch[k] % 4 || !cg_aligned(ptr[k])) return false;
        S.s[k].p = ptr[k]; S.s[k].c = ch[k]; S.s[k].pitch = pitch[k];
        S.n = k + 1;
        S.K += ch[k];
    }
    return S.n >= 1 && S.K <= CG_MAX_K;
}

bool cg_supported(int hidden, int nx, int cx0, int cx1, int cx2, int ksize) {
    if (ksize != 3 || hidden < 16 || hidden > CG_MAX_HIDDEN || hidden % 16) return false;
    if (nx < 1 || nx > CG_MAX_SRC - 1) return false;
    const int cx[3] = {cx0, cx1, cx2};
    int K = hidden;
    for (int k = 0; k < 3; ++k) {
        if (k < nx) {
            if (cx[k] < 4 || cx[k] % 4) return false;
            K += cx[k];
        } else if (cx[k] != 0) {
            return false;
        }
    }
    return K <= CG_MAX_K;
}

template <typename Kern, typename A>
int cg_launch(Kern kernel, dim3 grid, size_t lds, hipStream_t st, const A& args, const char* what) {
    if (int rc = stx_lds_require((const void*)kernel, lds, what)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(CG_THREADS), lds, st, args);
    return 0;
}

}  // namespace

extern "C" int stx_convgru_supported(int hidden, int nx, int cx0, int cx1, int cx2, int ksize) {
    stx_begin();
    return cg_supported(hidden, nx, cx0, cx1, cx2, ksize) ? 1 : 0;
}

// Floats of the packed weights for GEMM-K = K concatenated channels and N output channels (0: unsupported).
extern "C" long long stx_convgru_packed_floats(int K, int N) {
    stx_begin();
    if (K < 4 || K > CG_MAX_K || K % 4 || N < 1 || N > CG_MAX_K) return 0;
    return (long long)cg_groups(K) * stx_cdiv(N, 16) * 256;
}

extern "C" int stx_convgru_pack_weight(const float* w0, const float* w1, float* wp, int A, int Bd, int mode, void* stream) {
    stx_begin();
    STX_REQUIRE(w0 && wp && A > 0 && Bd > 0, "convgru_pack_weight: bad args");
    STX_REQUIRE(mode == 0 || mode == 1, "convgru_pack_weight: mode %d", mode);
    const int nw = w1 ? 2 : 1;
    const int K = mode == 0 ? Bd : nw * A, N = mode == 0 ? nw * A : Bd;
    STX_REQUIRE(K >= 4 && K <= CG_MAX_K && K % 4 == 0 && N <= CG_MAX_K, "convgru_pack_weight: K=%d (a multiple of 4, <= %d) N=%d (<= %d)",
                K, CG_MAX_K, N, CG_MAX_K);
    const int NTall = stx_cdiv(N, 16);
    const long long total = (long long)cg_groups(K) * NTall * 256;
    hipLaunchKernelGGL(cg_pack_kernel, dim3((unsigned)((total + CG_THREADS - 1) / CG_THREADS)), dim3(CG_THREADS), 0,
                       (hipStream_t)stream, w0, w1, wp, A, Bd, K, N, mode, NTall, total);
    return stx_check_launch("convgru_pack_weight");
}

extern "C" int stx_convgru_gemm(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                                const float* s3, int c3, int p3, const float* wp, int N, int epi, int split,
                                const float* bias0, const float* bias1, const float* add0, int add0_pitch, const float* add1,
                                int add1_pitch, const float* h, int h_pitch, const float* z, float* out0, float* out1, float* out2,
                                int out_pitch, int B, int H, int W, void* stream) {
    stx_begin();
    STX_REQUIRE(wp && out0 && B > 0 && H > 0 && W > 0 && N > 0 && N <= CG_MAX_K, "convgru_gemm: bad shape");
    STX_REQUIRE((long long)B * H * W < (1ll << 31), "convgru_gemm: %d x %d x %d pixels too many", B, H, W);
    CgGemmArgs a;
    const float* ptr[4] = {s0, s1, s2, s3};
    const int ch[4] = {c0, c1, c2, c3}, pitch[4] = {p0, p1, p2, p3};
    STX_REQUIRE(cg_sources(a.S, ptr, ch, pitch), "convgru_gemm: sources must be 1..4 in a row, each 16-byte aligned with channels a "
                "multiple of 4, a pitch >= channels that is a multiple of 4, and at most %d channels together", CG_MAX_K);
    STX_REQUIRE(epi >= 0 && epi <= 2, "convgru_gemm: epilogue code %d", epi);
    if (epi == 0) {
        split = N;
        STX_REQUIRE(out_pitch >= N && (!add0 || add0_pitch >= N), "convgru_gemm: raw epilogue, output / addend pitch below N=%d", N);
    } else {
        STX_REQUIRE(split >= 16 && split <= CG_MAX_HIDDEN && split % 16 == 0 && N == (epi == 1 ? 2 * split : split),
                    "convgru_gemm: gate epilogue %d with N=%d hidden=%d (a multiple of 16, <= %d)", epi, N, split, CG_MAX_HIDDEN);
        STX_REQUIRE(h && h_pitch >= split && (!add0 || add0_pitch >= split) && (!add1 || add1_pitch >= split),
                    "convgru_gemm: gate epilogue needs h and pitches >= hidden");
        STX_REQUIRE(epi == 1 ? out1 != nullptr : z != nullptr, "convgru_gemm: gate epilogue %d, missing operand", epi);
        STX_REQUIRE(out0 != h && out1 != h, "convgru_gemm: the output must not alias h");
    }
    a.wp = wp; a.bias0 = bias0; a.bias1 = bias1; a.add0 = add0; a.add1 = add1; a.h = h; a.z = z;
    a.out0 = out0; a.out1 = out1; a.out2 = out2;
    a.add0_pitch = add0_pitch; a.add1_pitch = add1_pitch; a.h_pitch = h_pitch; a.out_pitch = out_pitch;
    a.N = N; a.split = split; a.epi = epi; a.NTall = stx_cdiv(N, 16);
    a.H = H; a.W = W; a.nTW = stx_cdiv(W, 16);
    const int slices = stx_cdiv(a.NTall, 4);
    // 8-row tiles unless they would leave most compute units without a workgroup (the 1/16-resolution level)
    const bool small = (long long)B * stx_cdiv(H, 8) * a.nTW * slices < 256;
    const int MT = small ? 4 : 8;
    a.nTH = stx_cdiv(H, MT);
    const long long tiles = (long long)B * a.nTH * a.nTW;
    STX_REQUIRE(tiles < (1ll << 31), "convgru_gemm: %lld tiles exceed the grid", tiles);
    const size_t lds = (size_t)(MT + 2) * CG_LV * CG_PS * 4;
    const dim3 grid((unsigned)tiles, slices);
    int rc;
    if (small) rc = cg_launch(convgru_gemm_kernel<4>, grid, lds, (hipStream_t)stream, a, "convgru_gemm");
    else rc = cg_launch(convgru_gemm_kernel<8>, grid, lds, (hipStream_t)stream, a, "convgru_gemm");
    if (rc) return rc;
    return stx_check_launch("convgru_gemm");
}

// Rows of the bias-gradient partials the two streaming backward kernels write for P pixels (0: unsupported).
extern "C" int stx_convgru_gate_rows(long long P, int hidden) {
    stx_begin();
    if (P < 1 || hidden < 16 || hidden > CG_MAX_HIDDEN || hidden % 16) return 0;
    int rpb, blocks;
    long long pb;
    cg_stream_plan(P, hidden, &rpb, &pb, &blocks);
    return blocks;
}

extern "C" int stx_convgru_gate_bwd(const float* g, int g_pitch, const float* z, const float* q, const float* h, int h_pitch,
                                    float* gq, float* gz, float* rows, long long P, int hidden, void* stream) {
    stx_begin();
    STX_REQUIRE(g && z && q && h && gq && gz && P > 0, "convgru_gate_bwd: bad args");
    STX_REQUIRE(hidden >= 16 && hidden <= CG_MAX_HIDDEN && hidden % 16 == 0 && g_pitch >= hidden && h_pitch >= hidden,
                "convgru_gate_bwd: hidden=%d (a multiple of 16, <= %d), pitches >= hidden", hidden, CG_MAX_HIDDEN);
    CgGateArgs a = {};
    a.g = g; a.z = z; a.q = q; a.h = h; a.o0 = gq; a.o1 = gz; a.rows = rows;
    a.P = P; a.g_pitch = g_pitch; a.h_pitch = h_pitch; a.hidden = hidden;
    int blocks;
    cg_stream_plan(P, hidden, &a.rpb, &a.per_block, &blocks);
    hipLaunchKernelGGL(convgru_gate_bwd_kernel<0>, dim3(blocks), dim3(CG_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("convgru_gate_bwd");
}

extern "C" int stx_convgru_reset_bwd(float* buf, int buf_pitch, const float* g, int g_pitch, const float* z, const float* r,
                                     const float* h, int h_pitch, float* gr, float* rows, long long P, int hidden, void* stream) {
    stx_begin();
    STX_REQUIRE(buf && g && z && r && h && gr && P > 0, "convgru_reset_bwd: bad args");
    STX_REQUIRE(hidden >= 16 && hidden <= CG_MAX_HIDDEN && hidden % 16 == 0 && g_pitch >= hidden && h_pitch >= hidden && buf_pitch >= hidden,
                "convgru_reset_bwd: hidden=%d (a multiple of 16, <= %d), pitches >= hidden", hidden, CG_MAX_HIDDEN);
    CgGateArgs a = {};
    a.g = g; a.z = z; a.r = r; a.h = h; a.buf = buf; a.o0 = gr; a.rows = rows;
    a.P = P; a.g_pitch = g_pitch; a.h_pitch = h_pitch; a.buf_pitch = buf_pitch; a.hidden = hidden;
    int blocks;
    cg_stream_plan(P, hidden, &a.rpb, &a.per_block, &blocks);
    hipLaunchKernelGGL(convgru_gate_bwd_kernel<1>, dim3(blocks), dim3(CG_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("convgru_reset_bwd");
}

extern "C" int stx_convgru_row_sum(const float* rows, float* out, int nrows, int n, void* stream) {
    stx_begin();
    STX_REQUIRE(rows && out && nrows > 0 && n > 0, "convgru_row_sum: bad args");
    hipLaunchKernelGGL(convgru_row_sum_kernel, dim3(stx_cdiv(n, CG_THREADS)), dim3(CG_THREADS), 0, (hipStream_t)stream, rows, out, nrows, n);
    return stx_check_launch("convgru_row_sum");
}

extern "C" long long stx_convgru_wgrad_workspace_floats(int B, int H, int W, int K, int CC) {
    stx_begin();
    if (B < 1 || H < 1 || W < 1 || K < 4 || K > CG_MAX_K || K % 4 || CC < 16 || CC > 2 * CG_MAX_HIDDEN || CC % 16) return 0;
    const CgWPlan p = cg_wplan(B, H, W, K, CC);
    return (long long)p.npairs * p.nchunks * 9 * 1024;
}

// dw[ng CG][K][9] from the source list (K concatenated channels) against the dense maps g0 (and g1) [B][H][W][CG];
// workspace of stx_convgru_wgrad_workspace_floats(B, H, W, K, ng CG) floats.
extern "C" int stx_convgru_wgrad(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                                 const float* s3, int c3, int p3, const float* g0, const float* g1, int CG, float* dw,
                                 float* workspace, int B, int H, int W, void* stream) {
    stx_begin();
    STX_REQUIRE(g0 && dw && workspace && B > 0 && H > 0 && W > 0, "convgru_wgrad: bad args");
    STX_REQUIRE(CG >= 16 && CG <= CG_MAX_HIDDEN && CG % 16 == 0, "convgru_wgrad: %d gradient channels (a multiple of 16, <= %d)", CG,
                CG_MAX_HIDDEN);
    STX_REQUIRE(cg_aligned(g0) && cg_aligned(g1), "convgru_wgrad: gradient maps must be 16-byte aligned");
    STX_REQUIRE((long long)B * H * W < (1ll << 31), "convgru_wgrad: %d x %d x %d pixels too many", B, H, W);
    CgWArgs a;
    const float* ptr[4] = {s0, s1, s2, s3};
    const int ch[4] = {c0, c1, c2, c3}, pitch[4] = {p0, p1, p2, p3};
    STX_REQUIRE(cg_sources(a.S, ptr, ch, pitch), "convgru_wgrad: sources must be 1..4 in a row, each 16-byte aligned with channels a "
                "multiple of 4, a pitch >= channels that is a multiple of 4, and at most %d channels together", CG_MAX_K);
    a.g0 = g0; a.g1 = g1; a.slab = workspace; a.CG = CG; a.CC = g1 ? 2 * CG : CG;
    const CgWPlan p = cg_wplan(B, H, W, a.S.K, a.CC);
    STX_REQUIRE(p.ntiles < (1ll << 31), "convgru_wgrad: %lld tiles", p.ntiles);
    a.H = H; a.W = W; a.nA = p.nA; a.nB = p.nB; a.ntiles = (int)p.ntiles; a.nchunks = p.nchunks; a.ncfb = p.ncfb;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)18 * CG_WXLS + (size_t)16 * CG_WGLS) * 4;
    if (int rc = cg_launch(convgru_wgrad_kernel, dim3(p.nchunks, p.npairs), lds, st, a, "convgru_wgrad")) return rc;
    const long long nout = (long long)p.npairs * 9 * 1024;
    hipLaunchKernelGGL(convgru_wgrad_reduce_kernel, dim3((unsigned)(nout / 64)), dim3(CG_THREADS), 0, st, (const float*)workspace, dw,
                       a.S.K, a.CC, p.nchunks, p.ncfb);
    return stx_check_launch("convgru_wgrad");
}

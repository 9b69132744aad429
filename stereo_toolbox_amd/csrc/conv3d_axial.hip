// Axial-planar Conv3d for gfx950: the (1,3,3) "planar" and (kd,1,1) "axial" stride-1 convolutions of FoundationStereo's
// Conv3dNormActReduced (reference FoundationStereo/submodule.py:89-114), forward / data gradient / weight gradient, as
// implicit GEMM on the exact fp32 MFMA v_mfma_f32_16x16x4_f32 (the model's widths 28 / 56 / 112 / 168 are multiples of 4
// but not of 8 or 32: the 16-wide form needs no channel padding of K and wastes the least N).
//
// Layout: dense channels-last fp32 [B][D][H][W][C], "same" zero padding.
//
// Forward (and data gradient = the same kernel on flipped / transposed weights, pack mode 1).
//   GEMM view: M = output voxels, N = Cout in tiles of 16, K = taps x Cin.
//   A workgroup (4 waves) stages a halo tile of one CK-channel chunk into LDS as NL "lines" of LV voxels x CK floats:
//     axial : line = one of 16 consecutive (h,w) columns, voxels = a D-run of 16 outputs + kd-1 halo planes;
//     planar: line = one of 18 input rows h of a D-plane, voxels = 18 consecutive w (16 x 16 outputs + halo).
//   Inside a line (voxel, channel) is contiguous, so the taps that run ALONG a line (all kd of the axial kernel, the
//   three kw of the planar one) and the chunk's channels form ONE contiguous run of taps x CK floats per output voxel:
//   K is walked in 16-float groups through that run (one ds_read_b128 per lane and four MFMAs), without regard to
//   where a tap ends; the packed weights follow the same order and carry zeros behind the run's end (K padded to 16
//   per run, not per tap: 17 x 28 = 476 -> 480).  The planar kernel has three such runs (kh), one line apart.
//   A lane's float4 holds run elements 16 g + 4 (lane >> 4) + j, j = 0..3: MFMA j of the group takes component j, the
//   weights are packed to match (stx_conv3d_axial_pack_weight).  Lines end in >= 12 zeroed pad floats, so the
//   over-read of the last group meets zeros x zero weights; the pad also makes the line stride an odd multiple of 4
//   dwords (axial A reads, lane = line: conflict-free).
//   A wave owns 4 M tiles (16 voxels each) x up to 4 N tiles; wider outputs are further workgroups (grid.y) of the same
//   launch, all in stx_conv3d_axial_fwd.  Packed weights stream from L2 one group ahead.
//   Epilogue as stx_conv3d_fwd: scale / bias / residual / activation code, and per-workgroup BatchNorm partial rows
//   stats[rows][2][Cout] of the raw output (row = workgroup tile; every row x channel written once, no atomics).
//
// Weight gradient: dW[co][ci][t] = sum_vox x[vox + t - pad][ci] gz[vox][co].
//   MFMA view: D[16 ci][16 co] += A[ci][k = 4 voxels] B[k][co].  A workgroup owns one (32 ci, 32 co) block pair and a
//   contiguous run of spatial tiles; x (with halo) and gz tiles of 32 channels sit in LDS, the four voxels of an MFMA are
//   the same position of four neighbouring lines (line stride = 16 mod 32 dwords: conflict-free ds_read_b32).  The taps
//   are dealt round-robin to the 4 waves, each keeps its taps' 32 x 32 partial sums in registers.  Partials go to a slab
//   [pair][chunk][tap][32][32]; a second kernel sums the chunks in a fixed order (bitwise reproducible, no atomics).
#include "stx_common.h"

namespace {

constexpr int AX_THREADS = 256;
constexpr int AX_MT = 4;            // M tiles (16 voxels) per wave
constexpr int AX_ROWS = 4 * AX_MT;  // M tiles per workgroup: the D-run (axial) / the H rows (planar) of a tile
constexpr int AX_NT = 4;            // N tiles (16 channels) per workgroup at most
constexpr int AX_WTD = 8;           // weight gradient, axial: D-run of a tile

// Geometry of a kernel shape, shared by the pack routine, the launchers and the *_stat_rows / *_floats queries.
struct AxGeom {
    int planar;      // 1: (1,3,3); 0: (kd,1,1)
    int kd;          // axial taps (1 for planar)
    int T;           // taps
    int tpr;         // taps per run (along a line)
    int nrun;        // runs (lines apart)
    int CK, nchunk;  // channel chunk, chunks
    int ng;          // 16-float groups per run
    int NL, LV, LS;  // lines, voxels per line, line stride (floats)
};

bool ax_shape_ok(int kd, int kh, int kw) {
    if (kd == 1 && kh == 3 && kw == 3) return true;
    return kh == 1 && kw == 1 && kd >= 3 && kd <= 17 && (kd & 1);
}
bool ax_supported(int Cin, int Cout, int kd, int kh, int kw) {
    return ax_shape_ok(kd, kh, kw) && Cin >= 4 && Cin <= 192 && Cin % 4 == 0 && Cout >= 1 && Cout <= 192;
}
// line stride: voxels x chunk + a zeroed pad of >= 12 floats that makes the stride an odd multiple of 4 dwords
int ax_line_stride(int LV, int CK) { return LV * CK + (((LV * CK / 4) & 1) ? 16 : 12); }
AxGeom ax_geom(int Cin, int kd, int kh, int kw) {
    AxGeom g;
    g.planar = (kd == 1 && kh == 3);
    g.kd = g.planar ? 1 : kd;
    g.T = g.planar ? 9 : kd;
    g.tpr = g.planar ? 3 : kd;
    g.nrun = g.planar ? 3 : 1;
    g.CK = 4;
    for (int c = 32; c >= 4; c -= 4)       // the largest multiple of 4 up to 32 that divides Cin (28 for the model's widths)
        if (Cin % c == 0) { g.CK = c; break; }
    g.nchunk = Cin / g.CK;
    g.ng = (g.tpr * g.CK + 15) / 16;
    g.NL = g.planar ? AX_ROWS + 2 : 16;
    g.LV = g.planar ? 18 : AX_ROWS + g.kd - 1;
    g.LS = ax_line_stride(g.LV, g.CK);
    return g;
}

// wp[chunk][run][group][nt][lane][j] = Wk[tap][c][n]: run element kk = 16 group + 4 (lane >> 4) + j -> tap = run * tpr + kk / CK,
// c = chunk * CK + kk % CK (zero behind the run's end), n = 16 nt + (lane & 15).  From a torch weight w[A][Bd][T]:
//   mode 0 (forward):       K = Bd, N = A, Wk[tap][c][n] = w[n][c][tap]
//   mode 1 (data gradient): K = A, N = Bd, Wk[tap][c][n] = w[c][n][T-1-tap]
__global__ __launch_bounds__(AX_THREADS) void ax_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Bd, int N,
                                                             int mode, AxGeom g, int NTall, long long total) {
    const long long idx = (long long)blockIdx.x * AX_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    long long r = idx >> 8;
    const int nt = (int)(r % NTall); r /= NTall;
    const int grp = (int)(r % g.ng); r /= g.ng;
    const int run = (int)(r % g.nrun);
    const int ch = (int)(r / g.nrun);
    const int kk = 16 * grp + 4 * (lane >> 4) + j, n = 16 * nt + (lane & 15);
    float v = 0.f;
    if (kk < g.tpr * g.CK && n < N) {
        const int tap = run * g.tpr + kk / g.CK, c = ch * g.CK + kk % g.CK;
        v = mode == 0 ? w[((size_t)n * Bd + c) * g.T + tap] : w[((size_t)c * Bd + n) * g.T + (g.T - 1 - tap)];
    }
    wp[idx] = v;
}

struct AxArgs {
    const float* x;         // [B][D][H][W][Cin]
    const float* wp;        // packed weights
    float* out;             // [B][D][H][W][Cout]
    const float* scale;     // [Cout] or null
    const float* bias;      // [Cout] or null
    const float* residual;  // like out, or null
    float* stats;           // [gridDim.x][2][Cout] partial sums of the raw output, or null
    int D, H, W, Cin, Cout, act;
    int nA, nB;             // tiles: axial (D runs, column groups), planar (H, W)
    int nt0, NTall;         // first N tile of this launch (grid.y adds AX_NT each), N tiles of the packed weights
    AxGeom g;
};

__device__ __forceinline__ f32x4 ax_zero4() {
    f32x4 z;
    z[0] = 0.f; z[1] = 0.f; z[2] = 0.f; z[3] = 0.f;
    return z;
}

// NS: accumulator sets.  K group s adds into set s % NS and the sets are summed in the epilogue: an output is the sum of NS
// fp32 chains of K / NS products instead of one chain of K (476 for the 17-tap kernel at 28 channels), whose rounding error
// grows with its length (the blocked sums of conv3d.hip's march kernel; on the emulator the eval-mode block at 28 channels went
// from 2.8 x to 0.8 x the reference's own fp32-vs-fp64 distance).  NS = 4 at 1-2 N tiles, NS = 2 at 3-4 (128 accumulator
// registers either way).  The MFMA stream is unchanged; the epilogue adds NS - 1 VALU adds per output.
template <int NT, int NS>
__global__ __launch_bounds__(AX_THREADS, 2) void conv3d_axial_kernel(AxArgs a) {
    STX_DYN_SMEM(smem);
    float* tile = reinterpret_cast<float*>(smem);
    const AxGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int nt0 = a.nt0 + (int)blockIdx.y * AX_NT;
    const int P = a.H * a.W;
    // tile origin.  axial: lines = columns p0 + l of (h,w), voxels = planes d0 - pad + v; planar: lines = rows h0 - 1 + l of
    // plane `bd` (= b * D + d), voxels = w0 - 1 + v
    int bd, o1, o2;
    {
        const int t = blockIdx.x;
        const int tb = t % a.nB, ta = (t / a.nB) % a.nA;
        bd = t / (a.nB * a.nA);
        o1 = ta * AX_ROWS;
        o2 = tb * 16;
    }
    const int pad = g.kd / 2;
    const int LS = g.LS, CK = g.CK;

    // zero the pad behind every line once (never overwritten by the staging)
    for (int e = tid; e < g.NL * (LS - g.LV * CK); e += AX_THREADS) {
        const int np = LS - g.LV * CK, l = e / np;
        tile[l * LS + g.LV * CK + (e - l * np)] = 0.f;
    }

    f32x4 acc[NS][AX_MT][NT];
    int abase[AX_MT];
#pragma unroll
    for (int mm = 0; mm < AX_MT; ++mm) {
        const int m = wave * AX_MT + mm;
        abase[mm] = (g.planar ? m * LS + i * CK : i * LS + m * CK) + 4 * kq;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int k = 0; k < NS; ++k) acc[k][mm][nt] = ax_zero4();
    }

    const int NF4 = CK / 4;
    const int nelem = g.NL * g.LV * NF4;
    const int steps = g.nrun * g.ng;                                    // K groups of a chunk
    const size_t wstep = (size_t)a.NTall * 256;
    const float* wl = a.wp + (size_t)nt0 * 256 + (size_t)lane * 4;      // group s of chunk ch: wl + (ch * steps + s) * wstep
    const long long last = (long long)g.nchunk * steps - 1;

    for (int ch = 0; ch < g.nchunk; ++ch) {
        __syncthreads();                                                // every wave is done reading the previous chunk
        const int c0 = ch * CK;
        for (int e = tid; e < nelem; e += AX_THREADS) {
            const int f = e % NF4, lv = e / NF4;
            const int v = lv % g.LV, l = lv / g.LV;
            bool ok;
            size_t vox;
            if (g.planar) {
                const int h = o1 - 1 + l, w = o2 - 1 + v;
                ok = h >= 0 && h < a.H && w >= 0 && w < a.W;
                vox = ((size_t)bd * a.H + h) * a.W + w;
            } else {
                const int p = o2 + l, d = o1 - pad + v;
                ok = p < P && d >= 0 && d < a.D;
                vox = ((size_t)bd * a.D + d) * P + p;
            }
            const float4 val = ok ? stx_ld4(a.x + vox * a.Cin + c0 + 4 * f) : make_float4(0.f, 0.f, 0.f, 0.f);
            stx_st4(tile + l * LS + v * CK + 4 * f, val);
        }
        __syncthreads();
        const float* wq = wl + (size_t)ch * steps * wstep;
        float4 bcur[NT], bnxt[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bcur[nt] = stx_ld4(wq + (size_t)nt * 256);
        // (steps are walked NS at a time so that the set index is a compile-time constant; the sets rotate on across chunks
        //  only through the order of the additions, which stays fixed)
        for (int s0 = 0; s0 < steps; s0 += NS) {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int s = s0 + k;
                if (s < steps) {                                        // (wave-uniform)
                    const int r = s / g.ng, grp = s - r * g.ng;
                    const float* tr = tile + r * LS + 16 * grp;
                    // the next group's weights (behind the very last group: the last group again)
                    const long long sn = (long long)ch * steps + s + 1;
                    const float* wn = wl + (size_t)(sn > last ? last : sn) * wstep;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bnxt[nt] = stx_ld4(wn + (size_t)nt * 256);
                    float4 av[AX_MT];
#pragma unroll
                    for (int mm = 0; mm < AX_MT; ++mm) av[mm] = stx_ld4(tr + abase[mm]);
#pragma unroll
                    for (int mm = 0; mm < AX_MT; ++mm)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            acc[k][mm][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mm].x, bcur[nt].x, acc[k][mm][nt], 0, 0, 0);
                            acc[k][mm][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mm].y, bcur[nt].y, acc[k][mm][nt], 0, 0, 0);
                            acc[k][mm][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mm].z, bcur[nt].z, acc[k][mm][nt], 0, 0, 0);
                            acc[k][mm][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mm].w, bcur[nt].w, acc[k][mm][nt], 0, 0, 0);
                        }
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bcur[nt] = bnxt[nt];
                }
            }
        }
    }

    // epilogue: accumulator register r of a lane = voxel 4 kq + r of the M tile, channel 16 (nt0 + nt) + i
    float s1[NT], s2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { s1[nt] = 0.f; s2[nt] = 0.f; }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = (nt0 + nt) * 16 + i;
        const bool nok = n < a.Cout;
        const float sc = (a.scale && nok) ? a.scale[n] : 1.f;
        const float bs = (a.bias && nok) ? a.bias[n] : 0.f;
#pragma unroll
        for (int mm = 0; mm < AX_MT; ++mm) {
            const int m = wave * AX_MT + mm;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 4 * kq + r;
                bool ok;
                size_t vox;
                if (g.planar) {
                    ok = o1 + m < a.H && o2 + q < a.W;
                    vox = ((size_t)bd * a.H + o1 + m) * a.W + o2 + q;
                } else {
                    ok = o1 + m < a.D && o2 + q < P;
                    vox = ((size_t)bd * a.D + o1 + m) * P + o2 + q;
                }
                if (ok && nok) {
                    const size_t idx = vox * a.Cout + n;
                    float v = acc[0][mm][nt][r];
                    if constexpr (NS == 2) v += acc[1][mm][nt][r];
                    if constexpr (NS == 4) v = (v + acc[1][mm][nt][r]) + (acc[2][mm][nt][r] + acc[3][mm][nt][r]);
                    s1[nt] += v;
                    s2[nt] = fmaf(v, v, s2[nt]);
                    v = fmaf(v, sc, bs);
                    if (a.residual) v += a.residual[idx];
                    a.out[idx] = stx_act(v, a.act);
                }
            }
        }
    }
    if (a.stats) {
        // lanes of one channel (kq = 0..3), then the four waves, in a fixed order
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            s1[nt] += __shfl_xor(s1[nt], 16);
            s1[nt] += __shfl_xor(s1[nt], 32);
            s2[nt] += __shfl_xor(s2[nt], 16);
            s2[nt] += __shfl_xor(s2[nt], 32);
        }
        __syncthreads();                                                // the tile is no longer read
        if (lane < 16) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                tile[((wave * NT + nt) * 16 + lane) * 2 + 0] = s1[nt];
                tile[((wave * NT + nt) * 16 + lane) * 2 + 1] = s2[nt];
            }
        }
        __syncthreads();
        if (tid < NT * 16) {
            const int n = nt0 * 16 + tid;
            if (n < a.Cout) {
                float t1 = 0.f, t2 = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    t1 += tile[((w * NT) * 16 + tid) * 2 + 0];
                    t2 += tile[((w * NT) * 16 + tid) * 2 + 1];
                }
                float* row = a.stats + (size_t)blockIdx.x * 2 * a.Cout;
                row[n] = t1;
                row[a.Cout + n] = t2;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ weight gradient
struct AxWArgs {
    const float* x;    // [B][D][H][W][CF]
    const float* gz;   // [B][D][H][W][CC]
    float* slab;       // [pair][chunk][tap][32 ci][32 co]
    int D, H, W, CF, CC;
    int planar, kd, T;
    int nA, nB, ntiles, nchunks, ncfb;
    int XNL, XLV, XLS, GLV, GLS;   // x tile: lines, voxels per line, line stride; gz tile: 16 lines of GLV voxels
};

// TPW: taps per wave at most (tap t belongs to wave t % 4)
template <int TPW>
__global__ __launch_bounds__(AX_THREADS, 2) void conv3d_axial_wgrad_kernel(AxWArgs a) {
    STX_DYN_SMEM(smem);
    float* xt = reinterpret_cast<float*>(smem);
    float* gt = xt + a.XNL * a.XLS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x, pair = blockIdx.y;
    const int cfb = pair % a.ncfb, ccb = pair / a.ncfb;
    const int P = a.H * a.W, pad = a.kd / 2;
    const int t_lo = (int)((long long)a.ntiles * chunk / a.nchunks), t_hi = (int)((long long)a.ntiles * (chunk + 1) / a.nchunks);

    // the 16 floats behind every line's voxels are never read (reads stay inside the voxels); nothing to zero

    f32x4 acc[TPW][2][2];
#pragma unroll
    for (int k = 0; k < TPW; ++k)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) acc[k][mi][nj] = ax_zero4();

    const int nxe = a.XNL * a.XLV * 8, nge = 16 * a.GLV * 8;
    for (int t = t_lo; t < t_hi; ++t) {
        const int tb = t % a.nB, ta = (t / a.nB) % a.nA, bd = t / (a.nB * a.nA);
        const int o1 = ta * (a.planar ? 16 : AX_WTD), o2 = tb * 16;
        __syncthreads();                                                // every wave is done with the previous tile
        for (int e = tid; e < nxe; e += AX_THREADS) {
            const int f = e & 7, lv = e >> 3;
            const int v = lv % a.XLV, l = lv / a.XLV;
            const int c = cfb * 32 + 4 * f;
            bool ok;
            size_t vox;
            if (a.planar) {
                const int h = o1 - 1 + l, w = o2 - 1 + v;
                ok = h >= 0 && h < a.H && w >= 0 && w < a.W;
                vox = ((size_t)bd * a.H + h) * a.W + w;
            } else {
                const int p = o2 + l, d = o1 - pad + v;
                ok = p < P && d >= 0 && d < a.D;
                vox = ((size_t)bd * a.D + d) * P + p;
            }
            const float4 val = (ok && c < a.CF) ? stx_ld4(a.x + vox * a.CF + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            stx_st4(xt + l * a.XLS + v * 32 + 4 * f, val);
        }
        for (int e = tid; e < nge; e += AX_THREADS) {
            const int f = e & 7, lv = e >> 3;
            const int v = lv % a.GLV, l = lv / a.GLV;
            const int c = ccb * 32 + 4 * f;
            bool ok;
            size_t vox;
            if (a.planar) {
                const int h = o1 + l, w = o2 + v;
                ok = h < a.H && w < a.W;
                vox = ((size_t)bd * a.H + h) * a.W + w;
            } else {
                const int p = o2 + l, d = o1 + v;
                ok = p < P && d < a.D;
                vox = ((size_t)bd * a.D + d) * P + p;
            }
            const float4 val = (ok && c < a.CC) ? stx_ld4(a.gz + vox * a.CC + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            stx_st4(gt + l * a.GLS + v * 32 + 4 * f, val);
        }
        __syncthreads();
        for (int pos = 0; pos < a.GLV; ++pos) {
#pragma unroll
            for (int lg = 0; lg < 4; ++lg) {
                const float* gp = gt + (4 * lg + kq) * a.GLS + pos * 32 + i;
                const float b0 = gp[0], b1 = gp[16];
#pragma unroll
                for (int k = 0; k < TPW; ++k) {
                    const int tap = wave + 4 * k;                       // (wave-uniform)
                    if (tap < a.T) {
                        const int dl = a.planar ? tap / 3 : 0, dp = a.planar ? tap % 3 : tap;
                        const float* xp = xt + (4 * lg + kq + dl) * a.XLS + (pos + dp) * 32 + i;
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
    for (int k = 0; k < TPW; ++k) {
        const int tap = wave + 4 * k;
        if (tap < a.T) {
            float* dst = a.slab + (((size_t)pair * a.nchunks + chunk) * a.T + tap) * 1024;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(16 * mi + 4 * kq + r) * 32 + 16 * nj + i] = acc[k][mi][nj][r];
        }
    }
}

// dW[co][ci][tap] = sum over the chunks of the slab, in a fixed order: a workgroup owns 64 consecutive outputs of
// [pair][tap][32 ci][32 co]; its four waves take every fourth chunk, then one LDS round.
__global__ __launch_bounds__(AX_THREADS) void conv3d_axial_wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                                                int CF, int CC, int T, int nchunks, int ncfb) {
    __shared__ float red[4][64];
    const int part = threadIdx.x >> 6, o = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * 64 + o;
    const int e = (int)(idx & 1023);
    const int tap = (int)((idx >> 10) % T), pair = (int)((idx >> 10) / T);
    const float* p = slab + ((size_t)pair * nchunks * T + tap) * 1024 + e;
    float s = 0.f;
    for (int c = part; c < nchunks; c += 4) s += p[(size_t)c * T * 1024];
    red[part][o] = s;
    __syncthreads();
    if (part == 0) {
        const float t = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
        const int co = (pair / ncfb) * 32 + (e & 31), ci = (pair % ncfb) * 32 + (e >> 5);
        if (co < CC && ci < CF) dw[((size_t)co * CF + ci) * T + tap] = t;
    }
}

struct AxWPlan { int planar, T, nA, nB, ncfb, npairs, nchunks; long long ntiles; int XNL, XLV, XLS, GLV, GLS; size_t lds; };
AxWPlan ax_wplan(int B, int D, int H, int W, int CF, int CC, int kd, int kh, int kw) {
    AxWPlan p;
    p.planar = (kd == 1 && kh == 3);
    p.T = p.planar ? 9 : kd;
    if (p.planar) { p.nA = stx_cdiv(H, 16); p.nB = stx_cdiv(W, 16); p.ntiles = (long long)B * D * p.nA * p.nB; }
    else { p.nA = stx_cdiv(D, AX_WTD); p.nB = stx_cdiv(H * W, 16); p.ntiles = (long long)B * p.nA * p.nB; }
    p.ncfb = stx_cdiv(CF, 32);
    p.npairs = p.ncfb * stx_cdiv(CC, 32);
    long long n = 1024 / p.npairs;
    n = n < 1 ? 1 : n;
    p.nchunks = (int)(n > p.ntiles ? p.ntiles : n);
    p.XNL = p.planar ? 18 : 16;
    p.XLV = p.planar ? 18 : AX_WTD + kd - 1;
    p.GLV = p.planar ? 16 : AX_WTD;
    p.XLS = p.XLV * 32 + 16;
    p.GLS = p.GLV * 32 + 16;
    p.lds = ((size_t)p.XNL * p.XLS + (size_t)16 * p.GLS) * 4;
    return p;
}

template <typename K, typename A>
int ax_launch(K kernel, dim3 grid, size_t lds, hipStream_t st, const A& args, const char* what) {
    if (int rc = stx_lds_require((const void*)kernel, lds, what)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(AX_THREADS), lds, st, args);
    return 0;
}

int ax_fwd_launch(const AxArgs& a, int NT, dim3 grid, size_t lds, hipStream_t st) {
    switch (NT) {
    case 1: return ax_launch(conv3d_axial_kernel<1, 4>, grid, lds, st, a, "conv3d_axial_fwd");
    case 2: return ax_launch(conv3d_axial_kernel<2, 4>, grid, lds, st, a, "conv3d_axial_fwd");
    case 3: return ax_launch(conv3d_axial_kernel<3, 2>, grid, lds, st, a, "conv3d_axial_fwd");
    default: return ax_launch(conv3d_axial_kernel<4, 2>, grid, lds, st, a, "conv3d_axial_fwd");
    }
}

// tiles of the forward launch = rows of its BatchNorm partial slab
long long ax_fwd_tiles(const AxGeom& g, int B, int D, int H, int W, int* nA, int* nB) {
    if (g.planar) { *nA = stx_cdiv(H, AX_ROWS); *nB = stx_cdiv(W, 16); return (long long)B * D * *nA * *nB; }
    *nA = stx_cdiv(D, AX_ROWS); *nB = stx_cdiv(H * W, 16);
    return (long long)B * *nA * *nB;
}

}  // namespace

extern "C" int stx_conv3d_axial_supported(int Cin, int Cout, int kd, int kh, int kw) {
    stx_begin();
    return ax_supported(Cin, Cout, kd, kh, kw) ? 1 : 0;
}

// Floats of the packed weights for GEMM-K = K channels, N output channels (0: unsupported shape).
extern "C" long long stx_conv3d_axial_packed_floats(int K, int N, int kd, int kh, int kw) {
    stx_begin();
    if (!ax_supported(K, N, kd, kh, kw)) return 0;
    const AxGeom g = ax_geom(K, kd, kh, kw);
    return (long long)g.nchunk * g.nrun * g.ng * stx_cdiv(N, 16) * 256;
}

extern "C" int stx_conv3d_axial_pack_weight(const float* w, float* wp, int A, int Bd, int kd, int kh, int kw, int mode, void* stream) {
    stx_begin();
    STX_REQUIRE(w && wp && A > 0 && Bd > 0, "conv3d_axial_pack_weight: bad args");
    STX_REQUIRE(mode == 0 || mode == 1, "conv3d_axial_pack_weight: mode %d", mode);
    const int K = mode == 0 ? Bd : A, N = mode == 0 ? A : Bd;
    STX_REQUIRE(ax_supported(K, N, kd, kh, kw), "conv3d_axial_pack_weight: K=%d N=%d kernel (%d,%d,%d) unsupported", K, N, kd, kh, kw);
    const AxGeom g = ax_geom(K, kd, kh, kw);
    const int NTall = stx_cdiv(N, 16);
    const long long total = (long long)g.nchunk * g.nrun * g.ng * NTall * 256;
    hipLaunchKernelGGL(ax_pack_kernel, dim3((unsigned)((total + AX_THREADS - 1) / AX_THREADS)), dim3(AX_THREADS), 0,
                       (hipStream_t)stream, w, wp, Bd, N, mode, g, NTall, total);
    return stx_check_launch("conv3d_axial_pack_weight");
}

// Rows of the `stats` slab stx_conv3d_axial_fwd writes ([rows][2][Cout], every row written, nothing beyond).
extern "C" long long stx_conv3d_axial_fwd_stat_rows(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw) {
    stx_begin();
    if (B < 1 || D < 1 || H < 1 || W < 1 || !ax_supported(Cin, Cout, kd, kh, kw)) return 0;
    int nA, nB;
    return ax_fwd_tiles(ax_geom(Cin, kd, kh, kw), B, D, H, W, &nA, &nB);
}

extern "C" int stx_conv3d_axial_fwd(const float* x, const float* wp, float* out, const float* scale, const float* bias,
                                    const float* residual, float* stats, int B, int D, int H, int W, int Cin, int Cout,
                                    int kd, int kh, int kw, int act, void* stream) {
    stx_begin();
    STX_REQUIRE(x && wp && out && B > 0 && D > 0 && H > 0 && W > 0, "conv3d_axial_fwd: bad shape");
    STX_REQUIRE(ax_supported(Cin, Cout, kd, kh, kw), "conv3d_axial_fwd: Cin=%d (multiple of 4, <= 192) Cout=%d (<= 192) kernel (%d,%d,%d): "
                "served are (1,3,3) and (kd,1,1) with kd odd, 3..17", Cin, Cout, kd, kh, kw);
    STX_REQUIRE(act >= 0 && act <= 3, "conv3d_axial_fwd: activation code %d", act);
    STX_REQUIRE((long long)H * W < (1ll << 30), "conv3d_axial_fwd: plane of %d x %d voxels too large", H, W);
    AxArgs a;
    a.x = x; a.wp = wp; a.out = out; a.scale = scale; a.bias = bias; a.residual = residual; a.stats = stats;
    a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.act = act;
    a.g = ax_geom(Cin, kd, kh, kw);
    const long long tiles = ax_fwd_tiles(a.g, B, D, H, W, &a.nA, &a.nB);
    STX_REQUIRE(tiles < (1ll << 31), "conv3d_axial_fwd: %lld tiles exceed the grid", tiles);
    a.NTall = stx_cdiv(Cout, 16);
    const size_t lds = (size_t)a.g.NL * a.g.LS * 4;
    hipStream_t st = (hipStream_t)stream;
    // N in slices of AX_NT tiles: the whole slices are one launch (grid.y), a narrower last slice a second one
    const int nfull = a.NTall / AX_NT, rem = a.NTall % AX_NT;
    if (nfull) {
        a.nt0 = 0;
        if (int rc = ax_fwd_launch(a, AX_NT, dim3((unsigned)tiles, nfull), lds, st)) return rc;
    }
    if (rem) {
        a.nt0 = nfull * AX_NT;
        if (int rc = ax_fwd_launch(a, rem, dim3((unsigned)tiles, 1), lds, st)) return rc;
    }
    return stx_check_launch("conv3d_axial_fwd");
}

extern "C" long long stx_conv3d_axial_wgrad_workspace_floats(int B, int D, int H, int W, int CF, int CC, int kd, int kh, int kw) {
    stx_begin();
    if (B < 1 || D < 1 || H < 1 || W < 1 || !ax_supported(CF, CC, kd, kh, kw) || CC % 4) return 0;
    const AxWPlan p = ax_wplan(B, D, H, W, CF, CC, kd, kh, kw);
    return (long long)p.npairs * p.nchunks * p.T * 1024;
}

// dw[CC][CF][taps] from x [B][D][H][W][CF] and gz [B][D][H][W][CC]; workspace of stx_conv3d_axial_wgrad_workspace_floats floats.
extern "C" int stx_conv3d_axial_wgrad(const float* x, const float* gz, float* dw, float* workspace, int B, int D, int H, int W,
                                      int CF, int CC, int kd, int kh, int kw, void* stream) {
    stx_begin();
    STX_REQUIRE(x && gz && dw && workspace && B > 0 && D > 0 && H > 0 && W > 0, "conv3d_axial_wgrad: bad shape");
    STX_REQUIRE(ax_supported(CF, CC, kd, kh, kw) && CC % 4 == 0, "conv3d_axial_wgrad: CF=%d CC=%d (multiples of 4, <= 192) kernel (%d,%d,%d) "
                "unsupported", CF, CC, kd, kh, kw);
    STX_REQUIRE((long long)H * W < (1ll << 30), "conv3d_axial_wgrad: plane of %d x %d voxels too large", H, W);
    const AxWPlan p = ax_wplan(B, D, H, W, CF, CC, kd, kh, kw);
    STX_REQUIRE(p.ntiles < (1ll << 31), "conv3d_axial_wgrad: %lld tiles", p.ntiles);
    AxWArgs a;
    a.x = x; a.gz = gz; a.slab = workspace;
    a.D = D; a.H = H; a.W = W; a.CF = CF; a.CC = CC;
    a.planar = p.planar; a.kd = p.planar ? 1 : kd; a.T = p.T;
    a.nA = p.nA; a.nB = p.nB; a.ntiles = (int)p.ntiles; a.nchunks = p.nchunks; a.ncfb = p.ncfb;
    a.XNL = p.XNL; a.XLV = p.XLV; a.XLS = p.XLS; a.GLV = p.GLV; a.GLS = p.GLS;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.nchunks, p.npairs);
    int rc;
    if (p.T <= 12) rc = ax_launch(conv3d_axial_wgrad_kernel<3>, grid, p.lds, st, a, "conv3d_axial_wgrad");
    else rc = ax_launch(conv3d_axial_wgrad_kernel<5>, grid, p.lds, st, a, "conv3d_axial_wgrad");
    if (rc) return rc;
    const long long nout = (long long)p.npairs * p.T * 1024;
    hipLaunchKernelGGL(conv3d_axial_wgrad_reduce_kernel, dim3((unsigned)(nout / 64)), dim3(AX_THREADS), 0, st,
                       (const float*)workspace, dw, CF, CC, p.T, p.nchunks, p.ncfb);
    return stx_check_launch("conv3d_axial_wgrad");
}

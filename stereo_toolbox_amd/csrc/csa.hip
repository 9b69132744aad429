// Contextual spatial attention of SelectiveStereo (reference SelectiveStereo/SelectiveRAFT/update.py:106-135, the same text in
// SelectiveIGEV; used as `inp = cam(x) * x; att = sam(inp)`, SelectiveIGEV/igev_stereo.py:225-226) for gfx950, forward and backward.
//
//   ChannelAttentionEnhancement:  gate = sigmoid(W2 relu(W1 avg) + W2 relu(W1 max)),  avg / max = global pools of x per (b, c),
//                                 W1 [C/16][C], W2 [C][C/16] (1x1 convolutions without bias)
//   SpatialAttentionExtractor:    att = sigmoid(conv_kxk([mean_c x' | max_c x'])),  Conv2d(2, 1, k, padding k / 2) without bias
//
// Layout: channels-last fp32 x [B][H][W][pitch >= C].  Served (stx_csa_supported): C a multiple of 16 up to 256, k odd up to 7,
// any H, W >= 1.  Forward:
//   pass 1 (stx_csa_pool):   per-workgroup partial sum (double), max and arg max over a pixel range, per (b, c);
//   pass 2 (stx_csa_apply):  every workgroup combines the partials in block order and recomputes the tiny MLP in double
//                            (C x C/16 products, twice), writes x' = gate x and, in the same sweep, the per-pixel channel mean
//                            and max of x' as a 2-channel map (and the arg max channel); workgroup 0 of a batch item leaves the
//                            gate, the pooled vectors and the arg max pixels for the backward pass;
//   pass 3 (stx_csa_sam):    the k x k convolution of the map and the sigmoid, in double, rounded once.
//   The gate alone (stx_csa_gate) is pass 1 and a one-workgroup finish; the spatial attention alone is pass 2 without a gate.
// Every product the reference forms in fp32 is formed in double and rounded once (the reference's own fp32-vs-fp64 distance on
// x' is one rounding).  Ties: a global max pool sends its gradient to the lowest pixel index, a per-pixel channel max to the
// lowest channel.  Backward without atomics: per-workgroup partials in double, combined in a fixed order.
#include "stx_common.h"

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_MAX_C = 256;
constexpr int CS_MAX_CR = CS_MAX_C / 16;
constexpr int CS_MAX_K = 7;
constexpr int CS_MAX_BLOCKS = 256;       // workgroups of a pixel sweep per batch item

bool cs_c_ok(int C) { return C >= 16 && C <= CS_MAX_C && C % 16 == 0; }
bool cs_k_ok(int k) { return k >= 1 && k <= CS_MAX_K && (k & 1); }

// pixels per workgroup of a sweep over HW pixels by rows of `rows` pixels
void cs_plan(long long HW, int rows, long long* per_block, int* blocks) {
    long long pb = (HW + CS_MAX_BLOCKS - 1) / CS_MAX_BLOCKS;
    const long long least = (long long)rows * 4;
    pb = pb < least ? least : pb;
    pb = (pb + rows - 1) / rows * rows;
    *per_block = pb;
    *blocks = (int)((HW + pb - 1) / pb);
}

// ------------------------------------------------------------------------------------------ pass 1: pooled partials
struct CsPoolArgs {
    const float* x;
    double* psum; float* pmax; int* pidx;      // [B][blocks][C]
    long long HW, per_block;
    int pitch, C, rpb;
};

__global__ __launch_bounds__(CS_THREADS) void csa_pool_kernel(CsPoolArgs a) {
    __shared__ double rs[CS_THREADS];
    __shared__ float rm[CS_THREADS];
    __shared__ int ri[CS_THREADS];
    const int t = threadIdx.x, c = t % a.C, pr = t / a.C, b = blockIdx.y;
    const long long p_lo = (long long)blockIdx.x * a.per_block;
    const long long p_hi = p_lo + a.per_block < a.HW ? p_lo + a.per_block : a.HW;
    double s = 0.0;
    float m = 0.f;
    int mi = -1;
    if (pr < a.rpb) {
        const float* xb = a.x + (size_t)b * a.HW * a.pitch + c;
        for (long long p = p_lo + pr; p < p_hi; p += a.rpb) {
            const float v = xb[(size_t)p * a.pitch];
            s += (double)v;
            if (mi < 0 || v > m) { m = v; mi = (int)p; }
        }
    }
    rs[t] = s; rm[t] = m; ri[t] = mi;
    __syncthreads();
    if (t < a.C) {
        for (int k = 1; k < a.rpb; ++k) {
            const int o = k * a.C + t;
            s += rs[o];
            if (ri[o] >= 0 && (mi < 0 || rm[o] > m || (rm[o] == m && ri[o] < mi))) { m = rm[o]; mi = ri[o]; }
        }
        const size_t o = ((size_t)b * gridDim.x + blockIdx.x) * a.C + t;
        a.psum[o] = s; a.pmax[o] = m; a.pidx[o] = mi;
    }
}

// The gate of batch item b from the pooled partials, by the whole workgroup: gate[c] (rounded to float) in `gate`; pooled
// avg | max in `pool` [2][C], the hidden pre-activations in `hid` [2][C / 16] (all LDS, double).  Returns thread c's arg max pixel.
struct CsMlp {
    const double* psum; const float* pmax; const int* pidx; const float* w1; const float* w2;
    int nblk, C; long long HW;
};

__device__ __forceinline__ int cs_gate(const CsMlp& m, int b, float* gate, double* pool, double* hid) {
    const int t = threadIdx.x, C = m.C, Cr = C / 16;
    int mi = -1;
    if (t < C) {
        double s = 0.0;
        float mx = 0.f;
        for (int k = 0; k < m.nblk; ++k) {                              // block order = pixel order: the first maximum wins
            const size_t o = ((size_t)b * m.nblk + k) * C + t;
            s += m.psum[o];
            if (mi < 0 || m.pmax[o] > mx) { mx = m.pmax[o]; mi = m.pidx[o]; }
        }
        pool[t] = s / (double)m.HW;
        pool[C + t] = (double)mx;
    }
    __syncthreads();
    if (t < 2 * Cr) {
        const int j = t % Cr, which = t / Cr;
        const float* w = m.w1 + (size_t)j * C;
        const double* v = pool + which * C;
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += (double)w[c] * v[c];
        hid[t] = s;
    }
    __syncthreads();
    if (t < C) {
        double s = 0.0;
        for (int j = 0; j < Cr; ++j) {
            const double ha = hid[j] > 0.0 ? hid[j] : 0.0, hm = hid[Cr + j] > 0.0 ? hid[Cr + j] : 0.0;
            s += (double)m.w2[(size_t)t * Cr + j] * (ha + hm);
        }
        gate[t] = (float)(1.0 / (1.0 + exp(-s)));
    }
    __syncthreads();
    return mi;
}

struct CsGateArgs {
    CsMlp m;
    float* gate; double* pooled; int* argp;    // [B][C], [B][2][C], [B][C]
};

__global__ __launch_bounds__(CS_THREADS) void csa_gate_kernel(CsGateArgs a) {
    __shared__ float gate[CS_MAX_C];
    __shared__ double pool[2 * CS_MAX_C];
    __shared__ double hid[2 * CS_MAX_CR];
    const int t = threadIdx.x, b = blockIdx.x, C = a.m.C;
    const int mi = cs_gate(a.m, b, gate, pool, hid);
    if (t < C) {
        a.gate[(size_t)b * C + t] = gate[t];
        a.pooled[((size_t)b * 2) * C + t] = pool[t];
        a.pooled[((size_t)b * 2 + 1) * C + t] = pool[C + t];
        a.argp[(size_t)b * C + t] = mi;
    }
}

// ------------------------------------------------------------------------------------------ pass 2: x' and the 2-channel map
struct CsApplyArgs {
    CsMlp m;                                   // m.w1 null: no gate (the spatial attention of x itself)
    const float* x;
    float* xp;                                 // x' [B][HW][C] dense (null without a gate)
    float* map;                                // [B][HW][2]: channel mean | channel max of x'
    int* argc;                                 // [B][HW] arg max channel (or null)
    float* gate; double* pooled; int* argp;    // written by workgroup 0 of each batch item (or null)
    long long HW, per_block;
    int pitch, C;
};

__global__ __launch_bounds__(CS_THREADS) void csa_apply_kernel(CsApplyArgs a) {
    __shared__ float gate[CS_MAX_C];
    __shared__ double pool[2 * CS_MAX_C];
    __shared__ double hid[2 * CS_MAX_CR];
    __shared__ double rs[CS_THREADS];
    __shared__ float rm[CS_THREADS];
    __shared__ int ri[CS_THREADS];
    const int t = threadIdx.x, b = blockIdx.y, C = a.C;
    const bool gated = a.m.w1 != nullptr;
    if (gated) {
        const int mi = cs_gate(a.m, b, gate, pool, hid);
        if (blockIdx.x == 0 && a.gate && t < C) {
            a.gate[(size_t)b * C + t] = gate[t];
            a.pooled[((size_t)b * 2) * C + t] = pool[t];
            a.pooled[((size_t)b * 2 + 1) * C + t] = pool[C + t];
            a.argp[(size_t)b * C + t] = mi;
        }
    }
    // 16 lanes per pixel, lane l takes the channels l, l + 16, ..; 16 pixels per round
    const int l = t & 15, pr = t >> 4;
    const long long p_lo = (long long)blockIdx.x * a.per_block;
    const long long p_hi = p_lo + a.per_block < a.HW ? p_lo + a.per_block : a.HW;
    for (long long pb = p_lo; pb < p_hi; pb += 16) {                    // (uniform over the workgroup)
        const long long p = pb + pr;
        double s = 0.0;
        float m = 0.f;
        int mi = -1;
        if (p < p_hi) {
            const float* xr = a.x + ((size_t)b * a.HW + p) * a.pitch;
            float* xo = gated ? a.xp + ((size_t)b * a.HW + p) * C : nullptr;
            for (int c = l; c < C; c += 16) {
                float v = xr[c];
                if (gated) {
                    v = (float)((double)gate[c] * (double)v);
                    xo[c] = v;
                }
                s += (double)v;
                if (mi < 0 || v > m) { m = v; mi = c; }
            }
        }
        rs[t] = s; rm[t] = m; ri[t] = mi;
        __syncthreads();
        if (l == 0 && p < p_hi) {
            for (int k = 1; k < 16; ++k) {
                s += rs[t + k];
                if (rm[t + k] > m || (rm[t + k] == m && ri[t + k] < mi)) { m = rm[t + k]; mi = ri[t + k]; }
            }
            const size_t o = (size_t)b * a.HW + p;
            a.map[o * 2] = (float)(s / (double)C);
            a.map[o * 2 + 1] = m;
            if (a.argc) a.argc[o] = mi;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ pass 3: k x k convolution + sigmoid
__global__ __launch_bounds__(CS_THREADS) void csa_sam_kernel(const float* __restrict__ map, const float* __restrict__ w,
                                                            float* __restrict__ att, int B, int H, int W, int k) {
    const long long idx = (long long)blockIdx.x * CS_THREADS + threadIdx.x;
    if (idx >= (long long)B * H * W) return;
    const int x0 = (int)(idx % W), y0 = (int)((idx / W) % H), b = (int)(idx / ((long long)W * H));
    const int pad = k / 2;
    double s = 0.0;
    for (int dy = 0; dy < k; ++dy) {
        const int yy = y0 + dy - pad;
        if (yy < 0 || yy >= H) continue;
        for (int dx = 0; dx < k; ++dx) {
            const int xx = x0 + dx - pad;
            if (xx < 0 || xx >= W) continue;
            const float* mp = map + (((size_t)b * H + yy) * W + xx) * 2;
            s += (double)w[dy * k + dx] * (double)mp[0] + (double)w[k * k + dy * k + dx] * (double)mp[1];
        }
    }
    att[idx] = (float)(1.0 / (1.0 + exp(-s)));
}

// ------------------------------------------------------------------------------------------ backward of pass 3
// gpre = g att (1 - att)
__global__ __launch_bounds__(CS_THREADS) void csa_sam_bwd_pre_kernel(const float* __restrict__ g, const float* __restrict__ att,
                                                                    float* __restrict__ gpre, long long n) {
    const long long idx = (long long)blockIdx.x * CS_THREADS + threadIdx.x;
    if (idx >= n) return;
    const double av = (double)att[idx];
    gpre[idx] = (float)((double)g[idx] * av * (1.0 - av));
}

// gmap[pix][ch] = sum_taps w[ch][tap] gpre[pix - (tap - pad)]
__global__ __launch_bounds__(CS_THREADS) void csa_sam_bwd_data_kernel(const float* __restrict__ gpre, const float* __restrict__ w,
                                                                     float* __restrict__ gmap, int B, int H, int W, int k) {
    const long long idx = (long long)blockIdx.x * CS_THREADS + threadIdx.x;
    if (idx >= (long long)B * H * W) return;
    const int x0 = (int)(idx % W), y0 = (int)((idx / W) % H), b = (int)(idx / ((long long)W * H));
    const int pad = k / 2;
    double s0 = 0.0, s1 = 0.0;
    for (int dy = 0; dy < k; ++dy) {
        const int yy = y0 - (dy - pad);
        if (yy < 0 || yy >= H) continue;
        for (int dx = 0; dx < k; ++dx) {
            const int xx = x0 - (dx - pad);
            if (xx < 0 || xx >= W) continue;
            const double gv = (double)gpre[((size_t)b * H + yy) * W + xx];
            s0 += (double)w[dy * k + dx] * gv;
            s1 += (double)w[k * k + dy * k + dx] * gv;
        }
    }
    gmap[idx * 2] = (float)s0;
    gmap[idx * 2 + 1] = (float)s1;
}

// part[block][ch k k] = sum over the block's pixels of map[pix + tap - pad][ch] gpre[pix]; thread = (ch, tap)
__global__ __launch_bounds__(128) void csa_sam_bwd_weight_kernel(const float* __restrict__ gpre, const float* __restrict__ map,
                                                                double* __restrict__ part, int B, int H, int W, int k,
                                                                long long per_block) {
    const int t = threadIdx.x, kk = k * k;
    if (t >= 2 * kk) return;
    const int ch = t / kk, tap = t % kk, dy = tap / k - k / 2, dx = tap % k - k / 2;
    const long long n = (long long)B * H * W;
    const long long p_lo = (long long)blockIdx.x * per_block;
    const long long p_hi = p_lo + per_block < n ? p_lo + per_block : n;
    double s = 0.0;
    for (long long p = p_lo; p < p_hi; ++p) {
        const int x0 = (int)(p % W), y0 = (int)((p / W) % H);
        const int yy = y0 + dy, xx = x0 + dx;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        s += (double)map[(p + (long long)dy * W + dx) * 2 + ch] * (double)gpre[p];
    }
    part[(size_t)blockIdx.x * 2 * kk + t] = s;
}

// out[j] = (float) sum over the rows of rows[row][n] in row order
__global__ __launch_bounds__(CS_THREADS) void csa_row_sum_kernel(const double* __restrict__ rows, float* __restrict__ out,
                                                                int nrows, int n) {
    const int j = blockIdx.x * CS_THREADS + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int r = 0; r < nrows; ++r) s += rows[(size_t)r * n + j];
    out[j] = (float)s;
}

// ------------------------------------------------------------------------------------------ backward of pass 2
// g_x'[pix][c] = gxp[pix][c] + gmap[pix][0] / C + (c == argc[pix]) gmap[pix][1];  gx = gate g_x' (or g_x' without a gate);
// pgate[b][block][c] = sum over the block's pixels of g_x' x
struct CsApplyBwdArgs {
    const float* x; const float* gate; const float* gxp; const float* gmap; const int* argc;
    float* gx; double* pgate;
    long long HW, per_block;
    int pitch, gxp_pitch, C, rpb;
};

__global__ __launch_bounds__(CS_THREADS) void csa_apply_bwd_kernel(CsApplyBwdArgs a) {
    __shared__ double rs[CS_THREADS];
    const int t = threadIdx.x, c = t % a.C, pr = t / a.C, b = blockIdx.y;
    const long long p_lo = (long long)blockIdx.x * a.per_block;
    const long long p_hi = p_lo + a.per_block < a.HW ? p_lo + a.per_block : a.HW;
    const double gt = a.gate ? (double)a.gate[(size_t)b * a.C + c] : 1.0;
    double s = 0.0;
    if (pr < a.rpb) {
        for (long long p = p_lo + pr; p < p_hi; p += a.rpb) {
            const size_t o = (size_t)b * a.HW + p;
            double g = a.gxp ? (double)a.gxp[o * a.gxp_pitch + c] : 0.0;
            if (a.gmap) {
                g += (double)a.gmap[o * 2] / (double)a.C;
                if (a.argc[o] == c) g += (double)a.gmap[o * 2 + 1];
            }
            a.gx[o * a.C + c] = (float)(gt * g);
            if (a.pgate) s += g * (double)a.x[o * a.pitch + c];
        }
    }
    if (!a.pgate) return;                                               // (uniform over the launch)
    rs[t] = s;
    __syncthreads();
    if (t < a.C) {
        for (int k = 1; k < a.rpb; ++k) s += rs[k * a.C + t];
        a.pgate[((size_t)b * gridDim.x + blockIdx.x) * a.C + t] = s;
    }
}

// ------------------------------------------------------------------------------------------ backward of the MLP
// One workgroup, the batch items in order.  ggate[b][c] = sum of the pgate partials in block order, or the float map gg.
struct CsGateBwdArgs {
    const double* pgate; const float* gg; const double* pooled; const float* w1; const float* w2;
    float* dw1; float* dw2;                    // [C/16][C], [C][C/16] (or null)
    float* gavg; float* gmx;                   // [B][C]: gradient to every pixel of the mean path (1 / HW folded in), to the arg max
    int B, C, nblk; long long HW;
};

__global__ __launch_bounds__(CS_THREADS) void csa_gate_bwd_kernel(CsGateBwdArgs a) {
    __shared__ double pool[2 * CS_MAX_C];
    __shared__ double hid[2 * CS_MAX_CR];
    __shared__ double go[CS_MAX_C];
    __shared__ double gh[2 * CS_MAX_CR];
    const int t = threadIdx.x, C = a.C, Cr = C / 16;
    double d1[CS_MAX_CR], d2[CS_MAX_CR];                                 // thread c: dW1[j][c], dW2[c][j]
#pragma unroll
    for (int j = 0; j < CS_MAX_CR; ++j) { d1[j] = 0.0; d2[j] = 0.0; }
    for (int b = 0; b < a.B; ++b) {
        __syncthreads();
        if (t < C) {
            pool[t] = a.pooled[((size_t)b * 2) * C + t];
            pool[C + t] = a.pooled[((size_t)b * 2 + 1) * C + t];
        }
        __syncthreads();
        if (t < 2 * Cr) {
            const int j = t % Cr, which = t / Cr;
            const float* w = a.w1 + (size_t)j * C;
            const double* v = pool + which * C;
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += (double)w[c] * v[c];
            hid[t] = s;
        }
        __syncthreads();
        if (t < C) {
            double s = 0.0;
            for (int j = 0; j < Cr; ++j) {
                const double ha = hid[j] > 0.0 ? hid[j] : 0.0, hm = hid[Cr + j] > 0.0 ? hid[Cr + j] : 0.0;
                s += (double)a.w2[(size_t)t * Cr + j] * (ha + hm);
            }
            const double gate = 1.0 / (1.0 + exp(-s));
            double g = 0.0;
            if (a.pgate) {
                for (int k = 0; k < a.nblk; ++k) g += a.pgate[((size_t)b * a.nblk + k) * C + t];
            } else {
                g = (double)a.gg[(size_t)b * C + t];
            }
            go[t] = g * gate * (1.0 - gate);
            for (int j = 0; j < Cr; ++j) {
                const double ha = hid[j] > 0.0 ? hid[j] : 0.0, hm = hid[Cr + j] > 0.0 ? hid[Cr + j] : 0.0;
                d2[j] += go[t] * (ha + hm);
            }
        }
        __syncthreads();
        if (t < 2 * Cr) {
            const int j = t % Cr;
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += (double)a.w2[(size_t)c * Cr + j] * go[c];
            gh[t] = hid[t] > 0.0 ? s : 0.0;
        }
        __syncthreads();
        if (t < C) {
            double ga = 0.0, gm = 0.0;
            for (int j = 0; j < Cr; ++j) {
                const double w = (double)a.w1[(size_t)j * C + t];
                ga += w * gh[j];
                gm += w * gh[Cr + j];
                d1[j] += gh[j] * pool[t] + gh[Cr + j] * pool[C + t];
            }
            a.gavg[(size_t)b * C + t] = (float)(ga / (double)a.HW);
            a.gmx[(size_t)b * C + t] = (float)gm;
        }
    }
    if (t < C) {
        for (int j = 0; j < Cr; ++j) {
            if (a.dw1) a.dw1[(size_t)j * C + t] = (float)d1[j];
            if (a.dw2) a.dw2[(size_t)t * Cr + j] = (float)d2[j];
        }
    }
}

// gx[pix][c] (+)= gavg[b][c] + (pix == argp[b][c]) gmx[b][c]
__global__ __launch_bounds__(CS_THREADS) void csa_pool_bwd_kernel(float* __restrict__ gx, const float* __restrict__ gavg,
                                                                 const float* __restrict__ gmx, const int* __restrict__ argp,
                                                                 int accumulate, long long HW, int C, long long total) {
    const long long idx = (long long)blockIdx.x * CS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long p = (idx / C) % HW, b = idx / ((long long)C * HW);
    const size_t o = (size_t)b * C + c;
    double g = (double)gavg[o];
    if ((long long)argp[o] == p) g += (double)gmx[o];
    if (accumulate) g += (double)gx[idx];
    gx[idx] = (float)g;
}

bool cs_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" int stx_csa_supported(int C, int ksize) {
    stx_begin();
    return cs_c_ok(C) && cs_k_ok(ksize) ? 1 : 0;
}

// Workgroups per batch item of the pixel sweeps over HW pixels with C channels: the rows of psum / pmax / pidx and of pgate
// (0: unsupported).
extern "C" int stx_csa_blocks(long long HW, int C) {
    stx_begin();
    if (HW < 1 || HW >= (1ll << 31) || !cs_c_ok(C)) return 0;
    long long pb;
    int blocks;
    cs_plan(HW, CS_THREADS / C, &pb, &blocks);
    return blocks;
}

extern "C" int stx_csa_pool(const float* x, int pitch, double* psum, float* pmax, int* pidx, int B, long long HW, int C, void* stream) {
    stx_begin();
    STX_REQUIRE(x && psum && pmax && pidx && B > 0 && HW > 0 && cs_aligned8(psum), "csa_pool: bad args");
    STX_REQUIRE(cs_c_ok(C) && pitch >= C, "csa_pool: C=%d (a multiple of 16, <= %d), pitch >= C", C, CS_MAX_C);
    STX_REQUIRE(HW < (1ll << 31) && B < 65536, "csa_pool: %d x %lld pixels too many", B, HW);
    CsPoolArgs a;
    a.x = x; a.psum = psum; a.pmax = pmax; a.pidx = pidx; a.HW = HW; a.pitch = pitch; a.C = C; a.rpb = CS_THREADS / C;
    int blocks;
    cs_plan(HW, a.rpb, &a.per_block, &blocks);
    hipLaunchKernelGGL(csa_pool_kernel, dim3(blocks, B), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("csa_pool");
}

extern "C" int stx_csa_gate(const double* psum, const float* pmax, const int* pidx, int nblk, const float* w1, const float* w2,
                            float* gate, double* pooled, int* argp, int B, long long HW, int C, void* stream) {
    stx_begin();
    STX_REQUIRE(psum && pmax && pidx && w1 && w2 && gate && pooled && argp && B > 0 && HW > 0 && nblk > 0 && cs_aligned8(psum) &&
                cs_aligned8(pooled), "csa_gate: bad args");
    STX_REQUIRE(cs_c_ok(C), "csa_gate: C=%d (a multiple of 16, <= %d)", C, CS_MAX_C);
    CsGateArgs a;
    a.m.psum = psum; a.m.pmax = pmax; a.m.pidx = pidx; a.m.w1 = w1; a.m.w2 = w2; a.m.nblk = nblk; a.m.C = C; a.m.HW = HW;
    a.gate = gate; a.pooled = pooled; a.argp = argp;
    hipLaunchKernelGGL(csa_gate_kernel, dim3(B), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("csa_gate");
}

// w1 NULL: no gate -- map / argc of x itself, xp unused.  Otherwise psum / pmax / pidx [B][nblk][C] of stx_csa_pool, and gate,
// pooled, argp (all three or none) receive what the backward pass needs.
extern "C" int stx_csa_apply(const float* x, int pitch, const double* psum, const float* pmax, const int* pidx, int nblk,
                             const float* w1, const float* w2, float* xp, float* map, int* argc, float* gate, double* pooled,
                             int* argp, int B, long long HW, int C, void* stream) {
    stx_begin();
    STX_REQUIRE(x && map && B > 0 && HW > 0, "csa_apply: bad args");
    STX_REQUIRE(cs_c_ok(C) && pitch >= C, "csa_apply: C=%d (a multiple of 16, <= %d), pitch >= C", C, CS_MAX_C);
    STX_REQUIRE(HW < (1ll << 31) && B < 65536, "csa_apply: %d x %lld pixels too many", B, HW);
    if (w1) {
        STX_REQUIRE(psum && pmax && pidx && w2 && xp && nblk > 0 && cs_aligned8(psum), "csa_apply: the gate needs the pooled partials, w2 and xp");
        STX_REQUIRE((gate && pooled && argp && cs_aligned8(pooled)) || (!gate && !pooled && !argp), "csa_apply: gate, pooled and argp go together");
    }
    CsApplyArgs a;
    a.m.psum = psum; a.m.pmax = pmax; a.m.pidx = pidx; a.m.w1 = w1; a.m.w2 = w2; a.m.nblk = nblk; a.m.C = C; a.m.HW = HW;
    a.x = x; a.xp = xp; a.map = map; a.argc = argc; a.gate = gate; a.pooled = pooled; a.argp = argp;
    a.HW = HW; a.pitch = pitch; a.C = C;
    int blocks;
    cs_plan(HW, 16, &a.per_block, &blocks);
    hipLaunchKernelGGL(csa_apply_kernel, dim3(blocks, B), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("csa_apply");
}

extern "C" int stx_csa_sam(const float* map, const float* w, float* att, int B, int H, int W, int ksize, void* stream) {
    stx_begin();
    STX_REQUIRE(map && w && att && B > 0 && H > 0 && W > 0, "csa_sam: bad args");
    STX_REQUIRE(cs_k_ok(ksize), "csa_sam: kernel %d (odd, <= %d)", ksize, CS_MAX_K);
    const long long n = (long long)B * H * W;
    STX_REQUIRE(n < (1ll << 31), "csa_sam: %lld pixels too many", n);
    hipLaunchKernelGGL(csa_sam_kernel, dim3((unsigned)((n + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0, (hipStream_t)stream,
                       map, w, att, B, H, W, ksize);
    return stx_check_launch("csa_sam");
}

// Floats of the workspace of stx_csa_sam_bwd (the kernels keep doubles there: 8-byte aligned; 0: unsupported).
extern "C" long long stx_csa_sam_bwd_workspace_floats(int B, int H, int W, int ksize) {
    stx_begin();
    if (B < 1 || H < 1 || W < 1 || !cs_k_ok(ksize) || (long long)B * H * W >= (1ll << 31)) return 0;
    return (long long)CS_MAX_BLOCKS * 2 * ksize * ksize * 2;
}

// gpre [B][H][W] (scratch), gmap [B][H][W][2] and dw [2][k][k] (may be NULL, else with the workspace) from g = dL/d att.
extern "C" int stx_csa_sam_bwd(const float* g, const float* att, const float* map, const float* w, float* gpre, float* gmap,
                               float* dw, double* workspace, int B, int H, int W, int ksize, void* stream) {
    stx_begin();
    STX_REQUIRE(g && att && map && w && gpre && gmap && B > 0 && H > 0 && W > 0, "csa_sam_bwd: bad args");
    STX_REQUIRE(cs_k_ok(ksize), "csa_sam_bwd: kernel %d (odd, <= %d)", ksize, CS_MAX_K);
    STX_REQUIRE(!dw || (workspace && cs_aligned8(workspace)), "csa_sam_bwd: the weight gradient needs the workspace");
    const long long n = (long long)B * H * W;
    STX_REQUIRE(n < (1ll << 31), "csa_sam_bwd: %lld pixels too many", n);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((n + CS_THREADS - 1) / CS_THREADS);
    hipLaunchKernelGGL(csa_sam_bwd_pre_kernel, dim3(grid), dim3(CS_THREADS), 0, st, g, att, gpre, n);
    hipLaunchKernelGGL(csa_sam_bwd_data_kernel, dim3(grid), dim3(CS_THREADS), 0, st, (const float*)gpre, w, gmap, B, H, W, ksize);
    if (dw) {
        const long long per_block = (n + CS_MAX_BLOCKS - 1) / CS_MAX_BLOCKS;
        const int blocks = (int)((n + per_block - 1) / per_block);
        hipLaunchKernelGGL(csa_sam_bwd_weight_kernel, dim3(blocks), dim3(128), 0, st, (const float*)gpre, map, workspace, B, H, W, ksize,
                           per_block);
        const int nn = 2 * ksize * ksize;
        hipLaunchKernelGGL(csa_row_sum_kernel, dim3(stx_cdiv(nn, CS_THREADS)), dim3(CS_THREADS), 0, st, (const double*)workspace, dw,
                           blocks, nn);
    }
    return stx_check_launch("csa_sam_bwd");
}

// gate NULL: no gate.  gxp (gradient arriving at x', pitch gxp_pitch) and gmap (with argc) may each be NULL, not both.
// pgate (may be NULL) [B][stx_csa_blocks(HW, C)][C] doubles.
extern "C" int stx_csa_apply_bwd(const float* x, int pitch, const float* gate, const float* gxp, int gxp_pitch, const float* gmap,
                                 const int* argc, float* gx, double* pgate, int B, long long HW, int C, void* stream) {
    stx_begin();
    STX_REQUIRE(gx && (gxp || gmap) && (!gmap || argc) && (!pgate || (x && cs_aligned8(pgate))) && B > 0 && HW > 0, "csa_apply_bwd: bad args");
    STX_REQUIRE(cs_c_ok(C) && (!pgate || pitch >= C) && (!gxp || gxp_pitch >= C), "csa_apply_bwd: C=%d (a multiple of 16, <= %d), pitches >= C",
                C, CS_MAX_C);
    STX_REQUIRE(HW < (1ll << 31) && B < 65536, "csa_apply_bwd: %d x %lld pixels too many", B, HW);
    CsApplyBwdArgs a;
    a.x = x; a.gate = gate; a.gxp = gxp; a.gmap = gmap; a.argc = argc; a.gx = gx; a.pgate = pgate;
    a.HW = HW; a.pitch = pitch; a.gxp_pitch = gxp_pitch; a.C = C; a.rpb = CS_THREADS / C;
    int blocks;
    cs_plan(HW, a.rpb, &a.per_block, &blocks);
    hipLaunchKernelGGL(csa_apply_bwd_kernel, dim3(blocks, B), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("csa_apply_bwd");
}

// Exactly one of pgate ([B][nblk][C] doubles) and gg ([B][C] floats) is given.
extern "C" int stx_csa_gate_bwd(const double* pgate, int nblk, const float* gg, const double* pooled, const float* w1, const float* w2,
                                float* dw1, float* dw2, float* gavg, float* gmx, int B, long long HW, int C, void* stream) {
    stx_begin();
    STX_REQUIRE((pgate != nullptr) != (gg != nullptr) && pooled && w1 && w2 && gavg && gmx && B > 0 && HW > 0 && (!pgate || nblk > 0) &&
                cs_aligned8(pgate) && cs_aligned8(pooled), "csa_gate_bwd: bad args");
    STX_REQUIRE(cs_c_ok(C), "csa_gate_bwd: C=%d (a multiple of 16, <= %d)", C, CS_MAX_C);
    CsGateBwdArgs a;
    a.pgate = pgate; a.gg = gg; a.pooled = pooled; a.w1 = w1; a.w2 = w2; a.dw1 = dw1; a.dw2 = dw2; a.gavg = gavg; a.gmx = gmx;
    a.B = B; a.C = C; a.nblk = nblk; a.HW = HW;
    hipLaunchKernelGGL(csa_gate_bwd_kernel, dim3(1), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
    return stx_check_launch("csa_gate_bwd");
}

extern "C" int stx_csa_pool_bwd(float* gx, const float* gavg, const float* gmx, const int* argp, int accumulate, int B, long long HW,
                                int C, void* stream) {
    stx_begin();
    STX_REQUIRE(gx && gavg && gmx && argp && B > 0 && HW > 0, "csa_pool_bwd: bad args");
    STX_REQUIRE(cs_c_ok(C), "csa_pool_bwd: C=%d (a multiple of 16, <= %d)", C, CS_MAX_C);
    const long long total = (long long)B * HW * C;
    STX_REQUIRE(total < (1ll << 40), "csa_pool_bwd: %lld elements too many", total);
    hipLaunchKernelGGL(csa_pool_bwd_kernel, dim3((unsigned)((total + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0,
                       (hipStream_t)stream, gx, gavg, gmx, argp, accumulate, HW, C, total);
    return stx_check_launch("csa_pool_bwd");
}

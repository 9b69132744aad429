// MonSter's mono / stereo mutual refinement (reference models/MonSter/monster.py:456-494, warp.py, refinement.py:403-407), NCHW fp32.
//
//   * flaw = disp_warp(right, d)[0] - left for one or two disparities from one launch.  The sample coordinate is the reference's
//     (`normalize_coords` divides by W - 1 / H - 1, grid_sample runs with align_corners=False):
//         ix = (x - d) W / (W - 1) - 1/2,   iy = y H / (H - 1) - 1/2        (formed in double; the sample is rounded to fp32 once)
//     padding 'border' clips ix to [0, W - 1] and iy to [0, H - 1] (a clipped ix has no gradient to d, a corner index past the edge
//     contributes nothing); padding 'zeros' drops the corners outside the image.  The validity map is formed from the weights of
//     the corners inside the image (1 everywhere under 'border'; under 'zeros' the reference's `< 0.9999 -> 0`, `> 0 -> 1`): no
//     tensor of ones, no second sampling pass.
//   * backward, two launches, no float atomics, no memset: a per-pixel kernel (g_left = -(g_a + g_b), g_disp = -W / (W - 1)
//     sum_c g d out / d ix, the channel sum in double in a fixed order) and a GATHER for g_right: a workgroup owns (b, source row r,
//     8 channels).  The output rows y whose {y0, y0 + 1} hold r lie in [r - 1, r + 1]; for each of them, ascending, a's rows before
//     b's, the row's (x0, fx) are inverted into per-source-column lists in LDS -- counted and placed with INTEGER LDS atomics, then
//     every lane puts its own list in order of x (up to 8 entries by insertion; a longer one -- the band x < d that 'border' clips
//     onto column 0 is tens of entries in real data -- is written again by one in-order scan of the row) -- and walked once per
//     channel.  The order of the additions is therefore fixed, every g_right element is written exactly once, cells that receive
//     nothing are exact zeros.  Worst case: a whole row clipped onto one column puts W entries on one lane, which walks them
//     alone: legal and correct, not optimised.
//   * scale / shift fit (monster.py:31-66): per image ONE workgroup selects the k-th smallest mono value exactly (radix select on
//     the order-preserving bit pattern, 8 bits a pass, integer LDS histograms -- the method of weighted_lsq in mono_align.hip,
//     restated here with negative values ordered), masks with the strict comparisons of the reference, accumulates the five sums
//     in double in a fixed order, solves (X^T X + 1e-6 I) p = X^T y in double and rounds once.  Nothing is read back by the host.
#include "stx_common.h"

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_CCHUNK = 8;                   // channels of one forward / gather workgroup
constexpr int MS_PX = 64, MS_CG = 4;           // pixel backward: 64 pixels x 4 channel groups
constexpr int MS_MAX_W = 2048;                 // gather: W (9 + MS_CCHUNK) floats of LDS
constexpr int MS_SORT_MAX = 8;                 // gather: lists up to this length are sorted in place, longer ones rebuilt by a scan
constexpr int MS_FIT_THREADS = 1024;
constexpr int MS_FIT_STATS = 8;                // doubles per image: S_mm, S_m, N, S_mg, S_g, threshold, k, 0
constexpr double MS_RIDGE = 1e-6;              // monster.py:60
constexpr float MS_MIN_MONO = 1e-2f;           // monster.py:51 (compared in fp32, as torch compares an fp32 tensor with a scalar)
constexpr float MS_VALID_TH = 0.9999f;         // warp.py:77

struct MsGeom {
    int C, H, W, zeros;
    double sx, sy;                             // W / (W - 1), H / (H - 1)
};

// One axis of the sample: the top-left index i0 (border: in [0, n - 1]; zeros: in [-2, n]), the fraction, whether the two corners lie
// inside, whether the coordinate was clipped (border only).  A NaN coordinate lands on index 0 / -2: never out of bounds.
struct MsAxis {
    int i0;
    double f;
    bool a, b, clipped;
};

__device__ __forceinline__ MsAxis ms_axis(double v, int n, int zeros) {
    MsAxis t;
    if (zeros) {
        t.clipped = false;
        v = !(v >= -2.0) ? -2.0 : (v > (double)n ? (double)n : v);      // (outside [-1, n) both corners are outside anyway)
    } else {
        const double hi = (double)(n - 1);
        t.clipped = !(v > 0.0) || !(v < hi);
        v = v > 0.0 ? (v < hi ? v : hi) : 0.0;
    }
    const double fl = floor(v);
    t.i0 = (int)fl;
    t.f = v - fl;
    t.a = t.i0 >= 0 && t.i0 < n;
    t.b = t.i0 + 1 >= 0 && t.i0 + 1 < n;
    return t;
}

__device__ __forceinline__ MsAxis ms_axis_x(int x, float d, const MsGeom& g) { return ms_axis(((double)x - (double)d) * g.sx - 0.5, g.W, g.zeros); }
__device__ __forceinline__ MsAxis ms_axis_y(int y, const MsGeom& g) { return ms_axis((double)y * g.sy - 0.5, g.H, g.zeros); }

// bilinear sample of one plane; ddx = d value / d ix.  The four products are formed in double (the weights are the double
// fractions) and the caller rounds once: a streaming kernel does not feel the conversions, and the result is the nearest fp32
// value to the exact sample whatever the contraction of the build.
__device__ __forceinline__ double ms_sample(const float* __restrict__ plane, const MsAxis& tx, const MsAxis& ty, int W, double* ddx) {
    const float* r0 = plane + (ptrdiff_t)ty.i0 * W + tx.i0;
    const double v00 = tx.a && ty.a ? (double)r0[0] : 0.0, v01 = tx.b && ty.a ? (double)r0[1] : 0.0;
    const double v10 = tx.a && ty.b ? (double)r0[W] : 0.0, v11 = tx.b && ty.b ? (double)r0[W + 1] : 0.0;
    const double wx0 = 1.0 - tx.f, wy0 = 1.0 - ty.f;
    if (ddx) *ddx = wy0 * (v01 - v00) + ty.f * (v11 - v10);
    return wy0 * (wx0 * v00 + tx.f * v01) + ty.f * (wx0 * v10 + tx.f * v11);
}

__device__ __forceinline__ float ms_valid(const MsAxis& tx, const MsAxis& ty, int zeros) {
    if (!zeros) return 1.f;
    const double vx = (tx.a ? 1.0 - tx.f : 0.0) + (tx.b ? tx.f : 0.0);
    const double vy = (ty.a ? 1.0 - ty.f : 0.0) + (ty.b ? ty.f : 0.0);
    return (float)(vx * vy) < MS_VALID_TH ? 0.f : 1.f;
}

// ------------------------------------------------------------------------------------------------ flaw forward
// grid (cdiv(B H W, 256), cdiv(C, MS_CCHUNK)): lane = pixel, the taps of both disparities reused over the chunk's channels;
// out = sample - left (left NULL: the sample itself)
__global__ __launch_bounds__(MS_THREADS) void ms_flaw_fwd_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                                 const float* __restrict__ da, const float* __restrict__ db,
                                                                 float* __restrict__ oa, float* __restrict__ ob, float* __restrict__ valid,
                                                                 MsGeom g, long long npix) {
    const long long i = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= npix) return;
    const size_t hw = (size_t)g.H * g.W;
    const size_t b = (size_t)(i / (long long)hw), k = (size_t)(i % (long long)hw);
    const int y = (int)(k / g.W), x = (int)(k % g.W);
    const MsAxis ty = ms_axis_y(y, g), ta = ms_axis_x(x, da[i], g);
    MsAxis tb = ta;
    if (db) tb = ms_axis_x(x, db[i], g);
    if (valid && blockIdx.y == 0) valid[i] = ms_valid(ta, ty, g.zeros);
    const int c0 = (int)blockIdx.y * MS_CCHUNK, c1 = c0 + MS_CCHUNK < g.C ? c0 + MS_CCHUNK : g.C;
    for (int c = c0; c < c1; ++c) {
        const size_t plane = (b * g.C + c) * hw;
        const double l = left ? (double)left[plane + k] : 0.0;
        oa[plane + k] = (float)(ms_sample(right + plane, ta, ty, g.W, nullptr) - l);
        if (db) ob[plane + k] = (float)(ms_sample(right + plane, tb, ty, g.W, nullptr) - l);
    }
}

// ------------------------------------------------------------------------------------------------ flaw backward, per pixel
// grid cdiv(B H W, 64), block (64, 4): thread (p, q) walks the channels q, q + 4, ... of pixel p: g_left = -(g_a + g_b) and its
// share of sum_c g d out / d ix in double; the four shares are added in the order q = 0..3.
__global__ __launch_bounds__(MS_THREADS) void ms_flaw_bwd_pixel_kernel(const float* __restrict__ ga, const float* __restrict__ gb,
                                                                       const float* __restrict__ right, const float* __restrict__ da,
                                                                       const float* __restrict__ db, float* __restrict__ g_left,
                                                                       float* __restrict__ g_da, float* __restrict__ g_db, MsGeom g,
                                                                       long long npix) {
    __shared__ double red[2][MS_CG][MS_PX];
    const int p = threadIdx.x, q = threadIdx.y;
    const long long i = (long long)blockIdx.x * MS_PX + p;
    const bool live = i < npix;
    const bool want_a = g_da != nullptr && ga != nullptr, want_b = g_db != nullptr && gb != nullptr && db != nullptr;
    double sa = 0.0, sb = 0.0;
    bool clip_a = false, clip_b = false;
    if (live) {
        const size_t hw = (size_t)g.H * g.W;
        const size_t b = (size_t)(i / (long long)hw), k = (size_t)(i % (long long)hw);
        const int y = (int)(k / g.W), x = (int)(k % g.W);
        const MsAxis ty = ms_axis_y(y, g), ta = ms_axis_x(x, da[i], g);
        MsAxis tb = ta;
        if (db) tb = ms_axis_x(x, db[i], g);
        clip_a = ta.clipped;
        clip_b = tb.clipped;
        for (int c = q; c < g.C; c += MS_CG) {
            const size_t plane = (b * g.C + c) * hw;
            const float va = ga ? ga[plane + k] : 0.f, vb = gb ? gb[plane + k] : 0.f;
            if (g_left) g_left[plane + k] = -(va + vb);
            double ddx;
            if (want_a && !clip_a) {
                ms_sample(right + plane, ta, ty, g.W, &ddx);
                sa += (double)va * ddx;
            }
            if (want_b && !clip_b) {
                ms_sample(right + plane, tb, ty, g.W, &ddx);
                sb += (double)vb * ddx;
            }
        }
    }
    red[0][q][p] = sa;
    red[1][q][p] = sb;
    __syncthreads();
    if (q == 0 && live) {
        if (g_da) g_da[i] = clip_a || !want_a ? 0.f : (float)(-g.sx * (((red[0][0][p] + red[0][1][p]) + red[0][2][p]) + red[0][3][p]));
        if (g_db) g_db[i] = clip_b || !want_b ? 0.f : (float)(-g.sx * (((red[1][0][p] + red[1][1][p]) + red[1][2][p]) + red[1][3][p]));
    }
}

// ------------------------------------------------------------------------------------------------ flaw backward, g_right
// grid (H, cdiv(C, MS_CCHUNK), B), 256 threads, LDS ms_gather_lds(W).  See the head of the file.
__global__ __launch_bounds__(MS_THREADS) void ms_flaw_bwd_gather_kernel(const float* __restrict__ ga, const float* __restrict__ gb,
                                                                        const float* __restrict__ da, const float* __restrict__ db,
                                                                        float* __restrict__ g_right, MsGeom g) {
    STX_DYN_SMEM(smem);
    __shared__ int part[MS_THREADS];
    const int W = g.W, H = g.H, tid = threadIdx.x;
    int* x0s = reinterpret_cast<int*>(smem);                             // [W]     top-left column of output pixel x
    float* fxs = reinterpret_cast<float*>(x0s + W);                      // [W]     its fraction
    int* off = reinterpret_cast<int*>(fxs + W);                          // [W + 1] counts, then list starts, per source column
    int* cur = off + (W + 1);                                            // [W]     fill cursors
    int* ex = cur + W;                                                   // [2 W]   entries: the output column ...
    float* ew = reinterpret_cast<float*>(ex + 2 * W);                    // [2 W]   ... and its x weight
    float* acc = ew + 2 * W;                                             // [MS_CCHUNK][W]
    const int r = blockIdx.x, c0 = (int)blockIdx.y * MS_CCHUNK, b = blockIdx.z;
    const int nc = c0 + MS_CCHUNK < g.C ? MS_CCHUNK : g.C - c0;
    const size_t hw = (size_t)H * W;
    for (int i = tid; i < MS_CCHUNK * W; i += MS_THREADS) acc[i] = 0.f;
    const int per = (W + 1 + MS_THREADS - 1) / MS_THREADS;
    for (int set = 0; set < 2; ++set) {
        const float* disp = set ? db : da;
        const float* gq = set ? gb : ga;
        if (!disp || !gq) continue;                                      // (uniform)
        const int ylo = r - 2 > 0 ? r - 2 : 0, yhi = r + 2 < H - 1 ? r + 2 : H - 1;
        for (int y = ylo; y <= yhi; ++y) {
            const MsAxis ty = ms_axis_y(y, g);
            double wy;
            if (ty.a && ty.i0 == r) wy = 1.0 - ty.f;
            else if (ty.b && ty.i0 + 1 == r) wy = ty.f;
            else continue;                                               // (uniform: y and r only)
            __syncthreads();                                             // the lists of the row before are done with
            const float* drow = disp + (size_t)b * hw + (size_t)y * W;
            for (int x = tid; x < W; x += MS_THREADS) {
                const MsAxis tx = ms_axis_x(x, drow[x], g);
                x0s[x] = tx.i0;
                fxs[x] = (float)tx.f;
                off[x] = 0;
            }
            if (tid == 0) off[W] = 0;
            __syncthreads();
            for (int x = tid; x < W; x += MS_THREADS) {
                const int x0 = x0s[x];
                if (x0 >= 0 && x0 < W) atomicAdd(&off[x0], 1);
                if (x0 + 1 >= 0 && x0 + 1 < W) atomicAdd(&off[x0 + 1], 1);
            }
            __syncthreads();
            {                                                            // exclusive scan of off[0 .. W]
                const int lo = tid * per, hi = lo + per < W + 1 ? lo + per : W + 1;
                int s = 0;
                for (int j = lo; j < hi; ++j) s += off[j];
                part[tid] = s;
                __syncthreads();
                if (tid == 0) {
                    int run = 0;
                    for (int j = 0; j < MS_THREADS; ++j) {
                        const int v = part[j];
                        part[j] = run;
                        run += v;
                    }
                }
                __syncthreads();
                int run = part[tid];
                for (int j = lo; j < hi; ++j) {
                    const int v = off[j];
                    off[j] = run;
                    if (j < W) cur[j] = run;
                    run += v;
                }
            }
            __syncthreads();
            for (int x = tid; x < W; x += MS_THREADS) {
                const int x0 = x0s[x];
                const float fx = fxs[x];
                if (x0 >= 0 && x0 < W) {
                    const int pos = atomicAdd(&cur[x0], 1);
                    ex[pos] = x;
                    ew[pos] = 1.f - fx;
                }
                if (x0 + 1 >= 0 && x0 + 1 < W) {
                    const int pos = atomicAdd(&cur[x0 + 1], 1);
                    ex[pos] = x;
                    ew[pos] = fx;
                }
            }
            __syncthreads();
            for (int xs = tid; xs < W; xs += MS_THREADS) {               // a lane owns source column xs and its list
                const int beg = off[xs], end = off[xs + 1];
                if (beg == end) continue;
                if (end - beg > MS_SORT_MAX) {                           // a long list (the clipped band lands on column 0 / W - 1):
                    int at = beg;                                        // written again in order by one scan of the row
                    for (int x = 0; x < W; ++x) {
                        const int x0 = x0s[x];
                        if (x0 == xs) {
                            ex[at] = x;
                            ew[at++] = 1.f - fxs[x];
                        } else if (x0 + 1 == xs) {
                            ex[at] = x;
                            ew[at++] = fxs[x];
                        }
                    }
                } else
                for (int i = beg + 1; i < end; ++i) {                    // by x, ascending (the x of one list are distinct)
                    const int kx = ex[i];
                    const float kw = ew[i];
                    int j = i - 1;
                    while (j >= beg && ex[j] > kx) {
                        ex[j + 1] = ex[j];
                        ew[j + 1] = ew[j];
                        --j;
                    }
                    ex[j + 1] = kx;
                    ew[j + 1] = kw;
                }
                for (int c = 0; c < nc; ++c) {
                    const float* grow = gq + ((size_t)b * g.C + c0 + c) * hw + (size_t)y * W;
                    double s = 0.0;
                    for (int i = beg; i < end; ++i) s += (double)grow[ex[i]] * (double)ew[i];
                    acc[c * W + xs] = (float)((double)acc[c * W + xs] + wy * s);
                }
            }
        }
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
        float* out = g_right + ((size_t)b * g.C + c0 + c) * hw + (size_t)r * W;
        for (int xs = tid; xs < W; xs += MS_THREADS) out[xs] = acc[c * W + xs];
    }
}

// ------------------------------------------------------------------------------------------------ scale / shift
// bit pattern whose unsigned order is the order of the floats (negative values below the positive ones, -0 below +0)
__device__ __forceinline__ unsigned ms_key(float f) {
    union { float f; unsigned u; } c;
    c.f = f;
    return c.u & 0x80000000u ? ~c.u : c.u | 0x80000000u;
}
__device__ __forceinline__ float ms_unkey(unsigned k) {
    union { float f; unsigned u; } c;
    c.u = k & 0x80000000u ? k & 0x7fffffffu : ~k;
    return c.f;
}

// fixed-order tree over the workgroup; every thread returns the total
__device__ __forceinline__ double ms_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MS_FIT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// grid B, MS_FIT_THREADS threads: image b's n elements; k = the 0-based rank of the threshold
__global__ __launch_bounds__(MS_FIT_THREADS) void ms_scale_shift_kernel(const float* __restrict__ mono, const float* __restrict__ gt,
                                                                        const unsigned char* __restrict__ mask, float* __restrict__ out,
                                                                        double* __restrict__ stats, unsigned n, unsigned k) {
    __shared__ unsigned hist[256];
    __shared__ unsigned prefix, krem;
    __shared__ double red[MS_FIT_THREADS];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * n;
    const float* m = mono + base;
    if (tid == 0) {
        prefix = 0u;
        krem = k;
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int sh = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned long long want = (unsigned long long)prefix >> (sh + 8);   // the digits of the earlier passes
        for (unsigned i = tid; i < n; i += MS_FIT_THREADS) {
            const unsigned key = ms_key(m[i]);
            if (((unsigned long long)key >> (sh + 8)) == want) atomicAdd(&hist[(key >> sh) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned accum = 0u, digit = 0u;
            const unsigned kk = krem;
            while (digit < 255u && kk >= accum + hist[digit]) accum += hist[digit++];
            prefix |= digit << sh;
            krem = kk - accum;
        }
        __syncthreads();
    }
    const float thr = ms_unkey(prefix);
    double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned i = tid; i < n; i += MS_FIT_THREADS) {
        const float mf = m[i], gf = gt[base + i];
        const bool ok = mask ? mask[base + i] != 0 : (gf > 0.f && mf > MS_MIN_MONO && mf > thr);
        if (!ok) continue;
        const double mv = (double)mf, gv = (double)gf;
        S[0] += mv * mv;
        S[1] += mv;
        S[2] += 1.0;
        S[3] += mv * gv;
        S[4] += gv;
    }
    for (int j = 0; j < 5; ++j) S[j] = ms_block_sum(S[j], red);
    if (tid == 0) {
        const double a = S[0] + MS_RIDGE, d = S[2] + MS_RIDGE;
        const double det = a * d - S[1] * S[1];
        out[2 * blockIdx.x] = (float)((S[3] * d - S[1] * S[4]) / det);
        out[2 * blockIdx.x + 1] = (float)((a * S[4] - S[1] * S[3]) / det);
        double* st = stats + (size_t)blockIdx.x * MS_FIT_STATS;
        for (int j = 0; j < 5; ++j) st[j] = S[j];
        st[5] = (double)thr;
        st[6] = (double)k;
        st[7] = 0.0;
    }
}

// grid (cdiv(n, 256), B): out = scale x + shift (with_shift == 0: scale x, the backward)
__global__ __launch_bounds__(MS_THREADS) void ms_apply_kernel(const float* __restrict__ x, const float* __restrict__ ss,
                                                              float* __restrict__ out, unsigned n, int with_shift) {
    const unsigned i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t at = (size_t)blockIdx.y * n + i;
    const float sc = ss[2 * blockIdx.y], sh = with_shift ? ss[2 * blockIdx.y + 1] : 0.f;
    out[at] = sc * x[at] + sh;
}

// ------------------------------------------------------------------------------------------------ host side
int ms_shape_ok(int B, int C, int H, int W, const char* what) {
    STX_REQUIRE(B >= 1 && C >= 1 && H >= 2 && W >= 2, "%s: B, C >= 1 and H, W >= 2 (the sample grid divides by H - 1 and W - 1) required, got %d x %d x %d x %d",
                what, B, C, H, W);
    STX_REQUIRE((long long)B * C * H * W < (1ll << 31), "%s: %d x %d x %d x %d elements are not served (2^31 and above)", what, B, C, H, W);
    STX_REQUIRE((C + MS_CCHUNK - 1) / MS_CCHUNK <= 65535 && B <= 65535, "%s: more than 65535 channel chunks or images", what);
    return STX_OK;
}

int ms_fit_ok(int B, long long n, const char* what) {
    STX_REQUIRE(B >= 1 && B <= 65535, "%s: 1 <= B <= 65535 required, got %d", what, B);
    STX_REQUIRE(n >= 1 && n < (1ll << 24), "%s: %lld elements per image outside 1 .. 2^24 - 1", what, n);
    return STX_OK;
}

inline MsGeom ms_geom(int C, int H, int W, int zeros) {
    MsGeom g;
    g.C = C;
    g.H = H;
    g.W = W;
    g.zeros = zeros != 0;
    g.sx = (double)W / (double)(W - 1);
    g.sy = (double)H / (double)(H - 1);
    return g;
}

inline size_t ms_gather_lds(int W) { return ((size_t)(9 + MS_CCHUNK) * W + 1) * sizeof(float); }

}  // namespace

extern "C" int stx_monster_flaw_fwd(const float* left, const float* right, const float* disp_a, const float* disp_b, int zeros_pad,
                                    float* out_a, float* out_b, float* valid, int B, int C, int H, int W, void* stream) {
    stx_begin();
    const char* what = "monster_flaw_fwd";
    STX_REQUIRE(right && disp_a && out_a, "%s: null pointer", what);
    STX_REQUIRE((disp_b != nullptr) == (out_b != nullptr), "%s: disp_b and out_b go together", what);
    if (int rc = ms_shape_ok(B, C, H, W, what)) return rc;
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(ms_flaw_fwd_kernel, dim3((unsigned)((npix + MS_THREADS - 1) / MS_THREADS), (unsigned)stx_cdiv(C, MS_CCHUNK)),
                       dim3(MS_THREADS), 0, (hipStream_t)stream, left, right, disp_a, disp_b, out_a, out_b, valid,
                       ms_geom(C, H, W, zeros_pad), npix);
    return stx_check_launch(what);
}

extern "C" int stx_monster_flaw_bwd(const float* g_a, const float* g_b, const float* right, const float* disp_a, const float* disp_b,
                                    int zeros_pad, float* g_left, float* g_right, float* g_disp_a, float* g_disp_b, int B, int C, int H,
                                    int W, void* stream) {
    stx_begin();
    const char* what = "monster_flaw_bwd";
    STX_REQUIRE(right && disp_a && (g_a || g_b), "%s: null pointer", what);
    STX_REQUIRE(disp_b || (!g_b && !g_disp_b), "%s: g_b / g_disp_b without disp_b", what);
    STX_REQUIRE(g_left || g_right || g_disp_a || g_disp_b, "%s: no gradient asked for", what);
    if (int rc = ms_shape_ok(B, C, H, W, what)) return rc;
    const MsGeom g = ms_geom(C, H, W, zeros_pad);
    size_t lds = 0;
    if (g_right) {                                                       // (checked before anything is launched)
        STX_REQUIRE(W <= MS_MAX_W, "%s: W = %d above the %d the gradient to the sampled map serves", what, W, MS_MAX_W);
        lds = ms_gather_lds(W);
        if (int rc = stx_lds_require((const void*)ms_flaw_bwd_gather_kernel, lds, what)) return rc;
    }
    if (g_left || g_disp_a || g_disp_b) {
        const long long npix = (long long)B * H * W;
        hipLaunchKernelGGL(ms_flaw_bwd_pixel_kernel, dim3((unsigned)((npix + MS_PX - 1) / MS_PX)), dim3(MS_PX, MS_CG), 0,
                           (hipStream_t)stream, g_a, g_b, right, disp_a, disp_b, g_left, g_disp_a, g_disp_b, g, npix);
        if (int rc = stx_check_launch(what)) return rc;
    }
    if (g_right) {
        hipLaunchKernelGGL(ms_flaw_bwd_gather_kernel, dim3((unsigned)H, (unsigned)stx_cdiv(C, MS_CCHUNK), (unsigned)B), dim3(MS_THREADS),
                           lds, (hipStream_t)stream, g_a, g_b, disp_a, disp_b, g_right, g);
        return stx_check_launch(what);
    }
    return STX_OK;
}

extern "C" int stx_monster_scale_shift(const float* mono, const float* gt, const unsigned char* mask, long long k, float* out,
                                       void* stats, int B, long long n, void* stream) {
    stx_begin();
    const char* what = "monster_scale_shift";
    STX_REQUIRE(mono && gt && out && stats, "%s: null pointer", what);
    STX_REQUIRE(((size_t)stats & 7) == 0, "%s: stats must be 8-byte aligned", what);
    if (int rc = ms_fit_ok(B, n, what)) return rc;
    STX_REQUIRE(k >= 0 && k < n, "%s: rank %lld outside 0 .. n - 1 = %lld", what, k, n - 1);
    hipLaunchKernelGGL(ms_scale_shift_kernel, dim3((unsigned)B), dim3(MS_FIT_THREADS), 0, (hipStream_t)stream, mono, gt, mask, out,
                       (double*)stats, (unsigned)n, (unsigned)k);
    return stx_check_launch(what);
}

extern "C" int stx_monster_apply_scale_shift(const float* x, const float* scale_shift, int with_shift, float* out, int B, long long n,
                                             void* stream) {
    stx_begin();
    const char* what = "monster_apply_scale_shift";
    STX_REQUIRE(x && scale_shift && out, "%s: null pointer", what);
    if (int rc = ms_fit_ok(B, n, what)) return rc;
    hipLaunchKernelGGL(ms_apply_kernel, dim3((unsigned)((n + MS_THREADS - 1) / MS_THREADS), (unsigned)B), dim3(MS_THREADS), 0,
                       (hipStream_t)stream, x, scale_shift, out, (unsigned)n, with_shift);
    return stx_check_launch(what);
}

// The self-supervised objective of reference loss_functions/ (photometric_loss.py, auto_mask.py, smoothness_loss.py) on NCHW fp32
// images: the reference's own bilinear warp, the SSIM distance, the fused photometric loss, the auto-mask and the edge-aware
// smoothness loss, each with the backward the trainers need (to `disp`; to both images for the stand-alone SSIM).  Stock that is
// two grid_samples, two reflect pads, five avg_pool2ds and about twenty elementwise passes per prediction, and again in backward.
//
// Warp (photometric_loss.py:5-37).  The reference feeds a linspace(0, 1) grid to grid_sample with align_corners=False, so output
// pixel (h, w) samples the right image at
//     x = (w - disp) W / (W - 1) - 1/2,        y = h H / (H - 1) - 1/2
// bilinearly in BOTH directions with zeros outside; valid_mask is the sum of the weights of the corners inside the image.  The
// coordinates are formed in double (one multiply-add per pixel), the interpolation in fp32.
//
// SSIM distance (:40-77).  A workgroup owns a 16 x 64 tile of outputs and stages the two images with their reflected halo in LDS;
// every output sums its window's five moments in DOUBLE straight from LDS (the products of two floats are exact there), so
// sigma^2 = E[x^2] - mu^2 keeps its digits on flat regions.  Windows 3 .. 11.
//
// Backward of the windowed part, two launches, no atomics: `coef` computes per window q the three coefficients of
//     d dist_q / d y_r = (1 / n) (dS/dmu_y + 2 dS/dE[yy] y_r + dS/dE[xy] x_r) (-1/2) [0 <= dist_q <= 1]
// times the upstream gradient -- stored centred on the window's own centre pixel (a^ = a + 2 b y_q + c x_q, so that the gather
// adds small numbers) -- and `gather` sums them over the windows that contain pixel r OR one of its reflections: all of those lie
// in [r - p, r + p], a window counts once per padded position it holds (1, 2 or 3 times per direction).  Every gradient element is
// written once.
//
// Fused photometric loss (:80-104): the same tile kernel with the second tile filled by the warp at the reflected pixel positions
// (each with its own disparity), the channels looped inside, loss = mean_C((w dist + (1 - w) |L - warped|) valid).  Backward:
// `coef` (which also leaves the warped image in the workspace) and `gather`, whose epilogue adds the L1 term and multiplies by
// d warped / d x * (-W / (W - 1)), summed over the channels.  auto_mask is one forward launch with three tiles.
//
// Smoothness (smoothness_loss.py:5-44): `stats` (per-image sum of disp, max of img; per-block partials in double), `terms` (every
// block re-adds the partials in a fixed order, then sums its share of |dx norm| exp(-mean_C |dx img|) and the dy twin) and a
// one-block `final`.  Backward is one launch: d loss / d disp_k = |inv| sum_edges sign w / N - L_b inv / (H W), inv = 1 / (mean_b +
// 1e-7), L_b the image's share of the loss (saved by the forward) -- the second term is the path through the per-image mean.
#include "stx_common.h"

namespace {

constexpr int SL_TW = 64, SL_TH = 16;          // outputs of one workgroup
constexpr int SL_THREADS = 256;                // lane = column, wave + 4 k = row
constexpr int SL_ROWS = SL_TH / 4;
constexpr int SL_MAX_PAD = 5;                  // window 11
constexpr int SL_PHOTO_WINDOW = 7;             // photometric_loss calls ssim() with its default
constexpr int SL_SMOOTH_MAX_BLOCKS = 128;
constexpr double SL_C1 = 0.01 * 0.01, SL_C2 = 0.03 * 0.03;
constexpr double SL_MEAN_EPS = 1e-7;           // smoothness_loss.py:24

struct SlGeom {
    int C, H, W, p, tilesX;
    double sx, sy;                             // W / (W - 1), H / (H - 1)
};

__device__ __forceinline__ int sl_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// ------------------------------------------------------------------------------------------------ the reference's warp
struct SlTap {
    int x0, y0;                                // top-left corner, clamped to [-2, W] / [-2, H] (outside: zeros anyway)
    float fx, fy;
};

__device__ __forceinline__ int sl_corner(double f, int n) { return !(f >= -2.0) ? -2 : (f > (double)n ? n : (int)f); }

__device__ __forceinline__ SlTap sl_tap(int h, int w, float d, const SlGeom& g) {
    const double x = ((double)w - (double)d) * g.sx - 0.5, y = (double)h * g.sy - 0.5;
    const double xf = floor(x), yf = floor(y);
    SlTap t;
    t.x0 = sl_corner(xf, g.W);
    t.y0 = sl_corner(yf, g.H);
    t.fx = (float)(x - xf);
    t.fy = (float)(y - yf);
    return t;
}

__device__ __forceinline__ float sl_tap_valid(const SlTap& t, int H, int W) {
    const float vx = (t.x0 >= 0 && t.x0 < W ? 1.f - t.fx : 0.f) + (t.x0 + 1 >= 0 && t.x0 + 1 < W ? t.fx : 0.f);
    const float vy = (t.y0 >= 0 && t.y0 < H ? 1.f - t.fy : 0.f) + (t.y0 + 1 >= 0 && t.y0 + 1 < H ? t.fy : 0.f);
    return vx * vy;
}

// bilinear sample of one plane; ddx = d value / d x
__device__ __forceinline__ float sl_tap_sample(const float* __restrict__ plane, const SlTap& t, int H, int W, float* ddx) {
    const bool xa = t.x0 >= 0 && t.x0 < W, xb = t.x0 + 1 >= 0 && t.x0 + 1 < W;
    const bool ya = t.y0 >= 0 && t.y0 < H, yb = t.y0 + 1 >= 0 && t.y0 + 1 < H;
    const float* r0 = plane + (ptrdiff_t)t.y0 * W + t.x0;
    const float v00 = xa && ya ? r0[0] : 0.f, v01 = xb && ya ? r0[1] : 0.f;
    const float v10 = xa && yb ? r0[W] : 0.f, v11 = xb && yb ? r0[W + 1] : 0.f;
    const float wx0 = 1.f - t.fx, wy0 = 1.f - t.fy;
    if (ddx) *ddx = wy0 * (v01 - v00) + t.fy * (v11 - v10);
    return wy0 * (wx0 * v00 + t.fx * v01) + t.fy * (wx0 * v10 + t.fx * v11);
}

// grid cdiv(B*H*W, 256): warped [B][C][H][W], valid [B][H][W]
__global__ __launch_bounds__(SL_THREADS) void sl_warp_fwd_kernel(const float* __restrict__ right, const float* __restrict__ disp,
                                                                 float* __restrict__ warped, float* __restrict__ valid, SlGeom g,
                                                                 long long npix) {
    const long long i = (long long)blockIdx.x * SL_THREADS + threadIdx.x;
    if (i >= npix) return;
    const size_t hw = (size_t)g.H * g.W;
    const size_t b = (size_t)(i / (long long)hw), k = (size_t)(i % (long long)hw);
    const int h = (int)(k / g.W), w = (int)(k % g.W);
    const SlTap t = sl_tap(h, w, disp[i], g);
    valid[i] = sl_tap_valid(t, g.H, g.W);
    for (int c = 0; c < g.C; ++c) warped[(b * g.C + c) * hw + k] = sl_tap_sample(right + (b * g.C + c) * hw, t, g.H, g.W, nullptr);
}

// gdisp [B][H][W] = -sx sum_c g d warped / d x
__global__ __launch_bounds__(SL_THREADS) void sl_warp_bwd_kernel(const float* __restrict__ gw, const float* __restrict__ right,
                                                                 const float* __restrict__ disp, float* __restrict__ gdisp, SlGeom g,
                                                                 long long npix) {
    const long long i = (long long)blockIdx.x * SL_THREADS + threadIdx.x;
    if (i >= npix) return;
    const size_t hw = (size_t)g.H * g.W;
    const size_t b = (size_t)(i / (long long)hw), k = (size_t)(i % (long long)hw);
    const int h = (int)(k / g.W), w = (int)(k % g.W);
    const SlTap t = sl_tap(h, w, disp[i], g);
    double acc = 0.0;
    for (int c = 0; c < g.C; ++c) {
        float ddx;
        sl_tap_sample(right + (b * g.C + c) * hw, t, g.H, g.W, &ddx);
        acc += (double)gw[(b * g.C + c) * hw + k] * (double)ddx;
    }
    gdisp[i] = (float)(-g.sx * acc);
}

// ------------------------------------------------------------------------------------------------ tiles
__device__ __forceinline__ void sl_tile_origin(const SlGeom& g, int& h0, int& w0) {
    h0 = (int)(blockIdx.x / (unsigned)g.tilesX) * SL_TH;
    w0 = (int)(blockIdx.x % (unsigned)g.tilesX) * SL_TW;
}

__device__ __forceinline__ int sl_tile_stride(const SlGeom& g) { return SL_TW + 2 * g.p; }
__device__ __forceinline__ int sl_tile_floats(const SlGeom& g) { return (SL_TH + 2 * g.p) * (SL_TW + 2 * g.p); }

// tile[r][c] = value(h, w) of pixel (h0 - p + r, w0 - p + c): `reflect` = of the reflect-padded image (0 past the padding),
// otherwise of the zero-extended one
template <typename F>
__device__ __forceinline__ void sl_fill(float* tile, const SlGeom& g, int h0, int w0, bool reflect, F value) {
    const int TS = sl_tile_stride(g), n = sl_tile_floats(g);
    for (int i = threadIdx.x; i < n; i += SL_THREADS) {
        const int r = i / TS, c = i - r * TS;
        const int h = h0 - g.p + r, w = w0 - g.p + c;
        float v = 0.f;
        if (reflect) {
            if (h >= -g.p && h < g.H + g.p && w >= -g.p && w < g.W + g.p) v = value(sl_reflect(h, g.H), sl_reflect(w, g.W));
        } else if (h >= 0 && h < g.H && w >= 0 && w < g.W) {
            v = value(h, w);
        }
        tile[i] = v;
    }
}

struct SlMoments {
    double mx, my, vx, vy, cxy;
};

// the window whose top-left tile element is (r, c)
__device__ __forceinline__ SlMoments sl_moments(const float* tx, const float* ty, int TS, int r, int c, int ws) {
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int i = 0; i < ws; ++i) {
        const float* px = tx + (r + i) * TS + c;
        const float* py = ty + (r + i) * TS + c;
        for (int j = 0; j < ws; ++j) {
            const double a = (double)px[j], b = (double)py[j];
            sx += a;
            sy += b;
            sxx += a * a;
            syy += b * b;
            sxy += a * b;
        }
    }
    const double inv = 1.0 / (double)(ws * ws);
    SlMoments m;
    m.mx = sx * inv;
    m.my = sy * inv;
    m.vx = sxx * inv - m.mx * m.mx;
    m.vy = syy * inv - m.my * m.my;
    m.cxy = sxy * inv - m.mx * m.my;
    return m;
}

struct SlSsim {
    double A, Bt, Cc, D, S;                    // S = A Bt / (Cc D)
};

__device__ __forceinline__ SlSsim sl_ssim(const SlMoments& m) {
    SlSsim s;
    s.A = 2.0 * m.mx * m.my + SL_C1;
    s.Bt = 2.0 * m.cxy + SL_C2;
    s.Cc = m.mx * m.mx + m.my * m.my + SL_C1;
    s.D = m.vx + m.vy + SL_C2;
    s.S = (s.A * s.Bt) / (s.Cc * s.D);
    return s;
}

__device__ __forceinline__ double sl_clamp01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

__device__ __forceinline__ double sl_distance(const float* tx, const float* ty, int TS, int r, int c, int ws) {
    return sl_clamp01(0.5 * (1.0 - sl_ssim(sl_moments(tx, ty, TS, r, c, ws)).S));
}

// ------------------------------------------------------------------------------------------------ forward
// grid (tiles, B*C); dynamic LDS two tiles
__global__ __launch_bounds__(SL_THREADS) void sl_ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 float* __restrict__ out, SlGeom g) {
    STX_DYN_SMEM(smem);
    float* tx = reinterpret_cast<float*>(smem);
    float* ty = tx + sl_tile_floats(g);
    const int TS = sl_tile_stride(g), ws = 2 * g.p + 1;
    const size_t plane = (size_t)blockIdx.y * g.H * g.W;
    int h0, w0;
    sl_tile_origin(g, h0, w0);
    const float *px = x + plane, *py = y + plane;
    sl_fill(tx, g, h0, w0, true, [&](int h, int w) { return px[h * g.W + w]; });
    sl_fill(ty, g, h0, w0, true, [&](int h, int w) { return py[h * g.W + w]; });
    __syncthreads();
    const int col = threadIdx.x & 63, w = w0 + col;
    for (int k = 0; k < SL_ROWS; ++k) {
        const int row = (int)(threadIdx.x >> 6) + 4 * k, h = h0 + row;
        if (h < g.H && w < g.W) out[plane + (size_t)h * g.W + w] = (float)sl_distance(tx, ty, TS, row, col, ws);
    }
}

struct SlDenorm {
    float mean[3], std[3];
    int on;
};

// MASK = false: loss [B][1][H][W] = mean_C((w dist(L, Y) + (1 - w) |L - Y|) valid), Y = warp(right, disp) or right (disp NULL)
// MASK = true:  mask [B][1][H][W] = loss(disp) < loss(NULL), both without valid
// grid (tiles, B); dynamic LDS two / three tiles
template <bool MASK>
__global__ __launch_bounds__(SL_THREADS) void sl_photo_fwd_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                                  const float* __restrict__ disp, double w_ssim, int use_valid,
                                                                  SlDenorm dn, float* __restrict__ loss,
                                                                  unsigned char* __restrict__ mask, SlGeom g) {
    STX_DYN_SMEM(smem);
    float* tl = reinterpret_cast<float*>(smem);
    float* tw = tl + sl_tile_floats(g);
    float* tr = tw + sl_tile_floats(g);        // MASK only
    const int TS = sl_tile_stride(g), ws = 2 * g.p + 1;
    const size_t hw = (size_t)g.H * g.W, b = blockIdx.y;
    int h0, w0;
    sl_tile_origin(g, h0, w0);
    const float* pd = disp ? disp + b * hw : nullptr;
    const int col = threadIdx.x & 63, w = w0 + col;
    double acc[SL_ROWS], acc_id[SL_ROWS];
    float valid[SL_ROWS];
    for (int k = 0; k < SL_ROWS; ++k) {
        const int h = h0 + (int)(threadIdx.x >> 6) + 4 * k;
        acc[k] = acc_id[k] = 0.0;
        valid[k] = 1.f;
        if (!MASK && use_valid && pd && h < g.H && w < g.W) valid[k] = sl_tap_valid(sl_tap(h, w, pd[h * g.W + w], g), g.H, g.W);
    }
    for (int c = 0; c < g.C; ++c) {
        const float *pl = left + (b * g.C + c) * hw, *pr = right + (b * g.C + c) * hw;
        const float sc = dn.on ? dn.std[c] : 1.f, sh = dn.on ? dn.mean[c] : 0.f;
        sl_fill(tl, g, h0, w0, true, [&](int h, int w_) { return pl[h * g.W + w_] * sc + sh; });
        if (pd)
            sl_fill(tw, g, h0, w0, true, [&](int h, int w_) {
                const SlTap t = sl_tap(h, w_, pd[h * g.W + w_], g);
                const float v = sl_tap_sample(pr, t, g.H, g.W, nullptr);
                return dn.on ? v * sc + sh * sl_tap_valid(t, g.H, g.W) : v;      // the zeros outside are zeros of the de-normalised image
            });
        if (MASK || !pd) sl_fill(MASK ? tr : tw, g, h0, w0, true, [&](int h, int w_) { return pr[h * g.W + w_] * sc + sh; });
        __syncthreads();
        for (int k = 0; k < SL_ROWS; ++k) {
            const int row = (int)(threadIdx.x >> 6) + 4 * k;
            if (h0 + row >= g.H || w >= g.W) continue;
            const int centre = (row + g.p) * TS + col + g.p;
            const double l = (double)tl[centre];
            acc[k] += (w_ssim * sl_distance(tl, tw, TS, row, col, ws) + (1.0 - w_ssim) * fabs(l - (double)tw[centre])) * (double)valid[k];
            if (MASK) acc_id[k] += w_ssim * sl_distance(tl, tr, TS, row, col, ws) + (1.0 - w_ssim) * fabs(l - (double)tr[centre]);
        }
        __syncthreads();
    }
    for (int k = 0; k < SL_ROWS; ++k) {
        const int h = h0 + (int)(threadIdx.x >> 6) + 4 * k;
        if (h >= g.H || w >= g.W) continue;
        const size_t o = b * hw + (size_t)h * g.W + w;
        if (MASK)
            mask[o] = (float)(acc[k] / g.C) < (float)(acc_id[k] / g.C) ? 1 : 0;
        else
            loss[o] = (float)(acc[k] / g.C);
    }
}

// ------------------------------------------------------------------------------------------------ backward: coefficients
// The per-window coefficient maps [B][C][H][W] each: a^y, b, c (and a^x for the stand-alone SSIM), see the head of the file.
// PHOTO: up = gloss w valid / C, Y = the warp, which is also written to `warped`.
// grid (tiles, B*C); dynamic LDS two tiles
template <bool PHOTO>
__global__ __launch_bounds__(SL_THREADS) void sl_coef_kernel(const float* __restrict__ up, const float* __restrict__ x,
                                                             const float* __restrict__ y, const float* __restrict__ disp, double w_ssim,
                                                             int use_valid, float* __restrict__ ay, float* __restrict__ ax,
                                                             float* __restrict__ cb, float* __restrict__ cc, float* __restrict__ warped,
                                                             SlGeom g) {
    STX_DYN_SMEM(smem);
    float* tx = reinterpret_cast<float*>(smem);
    float* ty = tx + sl_tile_floats(g);
    const int TS = sl_tile_stride(g), ws = 2 * g.p + 1;
    const size_t hw = (size_t)g.H * g.W, plane = (size_t)blockIdx.y * hw, b = blockIdx.y / (unsigned)g.C;
    int h0, w0;
    sl_tile_origin(g, h0, w0);
    const float *px = x + plane, *py = y + plane;
    const float* pd = PHOTO ? disp + b * hw : nullptr;
    sl_fill(tx, g, h0, w0, true, [&](int h, int w) { return px[h * g.W + w]; });
    if (PHOTO)
        sl_fill(ty, g, h0, w0, true, [&](int h, int w) { return sl_tap_sample(py, sl_tap(h, w, pd[h * g.W + w], g), g.H, g.W, nullptr); });
    else
        sl_fill(ty, g, h0, w0, true, [&](int h, int w) { return py[h * g.W + w]; });
    __syncthreads();
    const int col = threadIdx.x & 63, w = w0 + col;
    const double inv_n = 1.0 / (double)(ws * ws);
    for (int k = 0; k < SL_ROWS; ++k) {
        const int row = (int)(threadIdx.x >> 6) + 4 * k, h = h0 + row;
        if (h >= g.H || w >= g.W) continue;
        const size_t o = plane + (size_t)h * g.W + w;
        const int centre = (row + g.p) * TS + col + g.p;
        const double xq = (double)tx[centre], yq = (double)ty[centre];
        double u;
        if (PHOTO) {
            u = (double)up[b * hw + (size_t)h * g.W + w] * w_ssim / (double)g.C;
            if (use_valid) u *= (double)sl_tap_valid(sl_tap(h, w, pd[h * g.W + w], g), g.H, g.W);
            warped[o] = ty[centre];
        } else {
            u = (double)up[o];
        }
        const SlMoments m = sl_moments(tx, ty, TS, row, col, ws);
        const SlSsim s = sl_ssim(m);
        const double dist = 0.5 * (1.0 - s.S);
        const double G = dist >= 0.0 && dist <= 1.0 ? -0.5 * u * inv_n : 0.0;       // torch's clamp passes the gradient at the ends
        const double icd = 1.0 / (s.Cc * s.D);
        const double dS_dmy = 2.0 * m.mx * (s.Bt - s.A) * icd - s.S * 2.0 * m.my * (1.0 / s.Cc - 1.0 / s.D);
        const double dS_dmx = 2.0 * m.my * (s.Bt - s.A) * icd - s.S * 2.0 * m.mx * (1.0 / s.Cc - 1.0 / s.D);
        const double dS_dee = -s.S / s.D;                                            // d / dE[xx] = d / dE[yy]
        const double dS_dexy = 2.0 * s.A * icd;
        ay[o] = (float)(G * (dS_dmy + 2.0 * dS_dee * yq + dS_dexy * xq));
        if (!PHOTO) ax[o] = (float)(G * (dS_dmx + 2.0 * dS_dee * xq + dS_dexy * yq));
        cb[o] = (float)(G * dS_dee);
        cc[o] = (float)(G * dS_dexy);
    }
}

// ------------------------------------------------------------------------------------------------ backward: gather
// how many padded positions of source index i window q holds (q in [i - p, i + p], inside the image)
__device__ __forceinline__ int sl_multiplicity(int q, int i, int n, int p) {
    return 1 + (i >= 1 && i <= p && q <= p - i) + (i <= n - 2 && i >= n - 1 - p && q >= 2 * (n - 1) - i - p);
}

struct SlGrad {
    double gx, gy;
};

// tile element (row + p, col + p) is the pixel (h, w); the coefficient tiles are zero outside the image
__device__ __forceinline__ SlGrad sl_gather(const float* ta_y, const float* ta_x, const float* tb, const float* tc, const float* tx,
                                            const float* ty, const SlGeom& g, int row, int col, int h, int w) {
    const int TS = sl_tile_stride(g), ws = 2 * g.p + 1;
    const int centre = (row + g.p) * TS + col + g.p;
    const float xr = tx[centre], yr = ty[centre];
    SlGrad out{0.0, 0.0};
    for (int i = 0; i < ws; ++i) {
        const int qh = h - g.p + i;
        if (qh < 0 || qh >= g.H) continue;
        const int mh = sl_multiplicity(qh, h, g.H, g.p);
        for (int j = 0; j < ws; ++j) {
            const int qw = w - g.p + j;
            if (qw < 0 || qw >= g.W) continue;
            const double m = (double)(mh * sl_multiplicity(qw, w, g.W, g.p));
            const int e = (row + i) * TS + col + j;
            const double dx = (double)(xr - tx[e]), dy = (double)(yr - ty[e]);
            const double bq = (double)tb[e], cq = (double)tc[e];
            out.gy += m * ((double)ta_y[e] + 2.0 * bq * dy + cq * dx);
            if (ta_x) out.gx += m * ((double)ta_x[e] + 2.0 * bq * dx + cq * dy);
        }
    }
    return out;
}

// grid (tiles, B*C); dynamic LDS six tiles; gx / gy may be NULL (not both)
__global__ __launch_bounds__(SL_THREADS) void sl_ssim_gather_kernel(const float* __restrict__ ay, const float* __restrict__ ax,
                                                                    const float* __restrict__ cb, const float* __restrict__ cc,
                                                                    const float* __restrict__ x, const float* __restrict__ y,
                                                                    float* __restrict__ gx, float* __restrict__ gy, SlGeom g) {
    STX_DYN_SMEM(smem);
    const int nt = sl_tile_floats(g);
    float* t_ay = reinterpret_cast<float*>(smem);
    float *t_ax = t_ay + nt, *t_b = t_ax + nt, *t_c = t_b + nt, *t_x = t_c + nt, *t_y = t_x + nt;
    const size_t plane = (size_t)blockIdx.y * g.H * g.W;
    int h0, w0;
    sl_tile_origin(g, h0, w0);
    const float* src[6] = {ay + plane, ax + plane, cb + plane, cc + plane, x + plane, y + plane};
    float* dst[6] = {t_ay, t_ax, t_b, t_c, t_x, t_y};
    for (int t = 0; t < 6; ++t) {
        const float* p = src[t];
        sl_fill(dst[t], g, h0, w0, false, [&](int h, int w) { return p[h * g.W + w]; });
    }
    __syncthreads();
    const int col = threadIdx.x & 63, w = w0 + col;
    for (int k = 0; k < SL_ROWS; ++k) {
        const int row = (int)(threadIdx.x >> 6) + 4 * k, h = h0 + row;
        if (h >= g.H || w >= g.W) continue;
        const SlGrad r = sl_gather(t_ay, t_ax, t_b, t_c, t_x, t_y, g, row, col, h, w);
        const size_t o = plane + (size_t)h * g.W + w;
        if (gx) gx[o] = (float)r.gx;
        if (gy) gy[o] = (float)r.gy;
    }
}

// gdisp [B][1][H][W] = -sx sum_c (gathered d / d warped + gloss (1 - w) valid / C sign(warped - L)) d warped / d x
// grid (tiles, B); dynamic LDS five tiles
__global__ __launch_bounds__(SL_THREADS) void sl_photo_gather_kernel(const float* __restrict__ gloss, const float* __restrict__ ay,
                                                                     const float* __restrict__ cb, const float* __restrict__ cc,
                                                                     const float* __restrict__ left, const float* __restrict__ warped,
                                                                     const float* __restrict__ right, const float* __restrict__ disp,
                                                                     double w_ssim, int use_valid, float* __restrict__ gdisp, SlGeom g) {
    STX_DYN_SMEM(smem);
    const int nt = sl_tile_floats(g), TS = sl_tile_stride(g);
    float* t_ay = reinterpret_cast<float*>(smem);
    float *t_b = t_ay + nt, *t_c = t_b + nt, *t_x = t_c + nt, *t_y = t_x + nt;
    const size_t hw = (size_t)g.H * g.W, b = blockIdx.y;
    int h0, w0;
    sl_tile_origin(g, h0, w0);
    const int col = threadIdx.x & 63, w = w0 + col;
    const float* pd = disp + b * hw;
    double acc[SL_ROWS], l1[SL_ROWS];
    SlTap tap[SL_ROWS];
    for (int k = 0; k < SL_ROWS; ++k) {
        const int h = h0 + (int)(threadIdx.x >> 6) + 4 * k;
        acc[k] = l1[k] = 0.0;
        tap[k] = SlTap{-2, -2, 0.f, 0.f};
        if (h >= g.H || w >= g.W) continue;
        tap[k] = sl_tap(h, w, pd[h * g.W + w], g);
        l1[k] = (double)gloss[b * hw + (size_t)h * g.W + w] * (1.0 - w_ssim) / (double)g.C;
        if (use_valid) l1[k] *= (double)sl_tap_valid(tap[k], g.H, g.W);
    }
    for (int c = 0; c < g.C; ++c) {
        const size_t plane = (b * g.C + c) * hw;
        const float* src[5] = {ay + plane, cb + plane, cc + plane, left + plane, warped + plane};
        float* dst[5] = {t_ay, t_b, t_c, t_x, t_y};
        for (int t = 0; t < 5; ++t) {
            const float* p = src[t];
            sl_fill(dst[t], g, h0, w0, false, [&](int h, int w_) { return p[h * g.W + w_]; });
        }
        __syncthreads();
        for (int k = 0; k < SL_ROWS; ++k) {
            const int row = (int)(threadIdx.x >> 6) + 4 * k, h = h0 + row;
            if (h >= g.H || w >= g.W) continue;
            double gw = sl_gather(t_ay, nullptr, t_b, t_c, t_x, t_y, g, row, col, h, w).gy;
            const int centre = (row + g.p) * TS + col + g.p;
            const float d = t_y[centre] - t_x[centre];
            gw += d > 0.f ? l1[k] : (d < 0.f ? -l1[k] : 0.0);
            float ddx;
            sl_tap_sample(right + plane, tap[k], g.H, g.W, &ddx);
            acc[k] += gw * (double)ddx;
        }
        __syncthreads();
    }
    for (int k = 0; k < SL_ROWS; ++k) {
        const int h = h0 + (int)(threadIdx.x >> 6) + 4 * k;
        if (h < g.H && w < g.W) gdisp[b * hw + (size_t)h * g.W + w] = (float)(-g.sx * acc[k]);
    }
}

// ------------------------------------------------------------------------------------------------ smoothness
// fixed-order tree over the workgroup; every thread returns the total
__device__ __forceinline__ double sl_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = SL_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

struct SlSmoothWs {
    double* psum;                              // [B][nblk]     sum of disp
    double* pterm;                             // [B][nblk][2]  x / y terms
    float* pmax;                               // [B][nblk]     max of img
};

// grid (nblk, B)
__global__ __launch_bounds__(SL_THREADS) void sl_smooth_stats_kernel(const float* __restrict__ disp, const float* __restrict__ img,
                                                                     SlSmoothWs ws, int C, long long hw) {
    __shared__ double red[SL_THREADS];
    __shared__ float redm[SL_THREADS];
    const size_t b = blockIdx.y;
    const long long step = (long long)gridDim.x * SL_THREADS, first = (long long)blockIdx.x * SL_THREADS + threadIdx.x;
    double s = 0.0;
    for (long long i = first; i < hw; i += step) s += (double)disp[b * hw + i];
    float m = -3.402823466e38f;
    for (long long i = first; i < hw * C; i += step) m = fmaxf(m, img[b * C * hw + i]);
    s = sl_block_sum(s, red);
    redm[threadIdx.x] = m;
    __syncthreads();
    for (int k = SL_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) redm[threadIdx.x] = fmaxf(redm[threadIdx.x], redm[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ws.psum[b * gridDim.x + blockIdx.x] = s;
        ws.pmax[b * gridDim.x + blockIdx.x] = redm[0];
    }
}

// exp(-mean_C |img_i - img_j|), j = i + step
__device__ __forceinline__ double sl_edge_weight(const float* __restrict__ img, int C, long long hw, long long i, long long step) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += fabs((double)img[c * hw + i] - (double)img[c * hw + i + step]);
    return exp(-s / (double)C);
}

__device__ __forceinline__ double sl_image_mean(const double* psum, int nblk, long long hw) {
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += psum[k];
    return s / (double)hw;
}

// grid (nblk, B)
__global__ __launch_bounds__(SL_THREADS) void sl_smooth_terms_kernel(const float* __restrict__ disp, const float* __restrict__ img,
                                                                     SlSmoothWs ws, int C, int H, int W) {
    __shared__ double red[SL_THREADS];
    const size_t b = blockIdx.y;
    const long long hw = (long long)H * W;
    const double ainv = fabs(1.0 / (sl_image_mean(ws.psum + b * gridDim.x, (int)gridDim.x, hw) + SL_MEAN_EPS));
    const float* d = disp + b * hw;
    const float* im = img + b * C * hw;
    const long long step = (long long)gridDim.x * SL_THREADS;
    double tx = 0.0, ty = 0.0;
    for (long long i = (long long)blockIdx.x * SL_THREADS + threadIdx.x; i < hw; i += step) {
        const int h = (int)(i / W), w = (int)(i % W);
        if (w + 1 < W) tx += fabs((double)d[i] - (double)d[i + 1]) * ainv * sl_edge_weight(im, C, hw, i, 1);
        if (h + 1 < H) ty += fabs((double)d[i] - (double)d[i + W]) * ainv * sl_edge_weight(im, C, hw, i, W);
    }
    tx = sl_block_sum(tx, red);
    ty = sl_block_sum(ty, red);
    if (threadIdx.x == 0) {
        ws.pterm[2 * (b * gridDim.x + blockIdx.x)] = tx;
        ws.pterm[2 * (b * gridDim.x + blockIdx.x) + 1] = ty;
    }
}

// one workgroup: out = (loss, max of img); stats = per image (mean, share of the loss), doubles
__global__ __launch_bounds__(SL_THREADS) void sl_smooth_final_kernel(SlSmoothWs ws, float* __restrict__ out, double* __restrict__ stats,
                                                                     int B, int nblk, int H, int W) {
    const long long hw = (long long)H * W;
    const double nx = (double)B * H * (W - 1), ny = (double)B * (H - 1) * W;
    for (int b = threadIdx.x; b < B; b += SL_THREADS) {
        double tx = 0.0, ty = 0.0;
        for (int k = 0; k < nblk; ++k) {
            tx += ws.pterm[2 * ((size_t)b * nblk + k)];
            ty += ws.pterm[2 * ((size_t)b * nblk + k) + 1];
        }
        stats[b] = sl_image_mean(ws.psum + (size_t)b * nblk, nblk, hw);
        stats[B + b] = tx / nx + ty / ny;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double loss = 0.0;
        float m = -3.402823466e38f;
        for (int b = 0; b < B; ++b) loss += stats[B + b];
        for (int k = 0; k < B * nblk; ++k) m = fmaxf(m, ws.pmax[k]);
        out[0] = (float)loss;
        out[1] = m;
    }
}

// grid cdiv(B*H*W, 256)
__global__ __launch_bounds__(SL_THREADS) void sl_smooth_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ disp,
                                                                   const float* __restrict__ img, const double* __restrict__ stats,
                                                                   float* __restrict__ gdisp, int B, int C, int H, int W, long long npix) {
    const long long idx = (long long)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= npix) return;
    const long long hw = (long long)H * W;
    const size_t b = (size_t)(idx / hw);
    const long long i = idx % hw;
    const int h = (int)(i / W), w = (int)(i % W);
    const float* d = disp + b * hw;
    const float* im = img + b * C * hw;
    const double inv = 1.0 / (stats[b] + SL_MEAN_EPS);
    const double nx = (double)B * H * (W - 1), ny = (double)B * (H - 1) * W;
    const float di = d[i];
    double tx = 0.0, ty = 0.0;
    auto sign = [](float a, float c) { return a > c ? 1.0 : (a < c ? -1.0 : 0.0); };
    if (w + 1 < W) tx += sign(di, d[i + 1]) * sl_edge_weight(im, C, hw, i, 1);
    if (w > 0) tx += sign(di, d[i - 1]) * sl_edge_weight(im, C, hw, i - 1, 1);
    if (h + 1 < H) ty += sign(di, d[i + W]) * sl_edge_weight(im, C, hw, i, W);
    if (h > 0) ty += sign(di, d[i - W]) * sl_edge_weight(im, C, hw, i - W, W);
    gdisp[idx] = (float)((double)gout[0] * (fabs(inv) * (tx / nx + ty / ny) - stats[B + b] * inv / (double)hw));
}

// ------------------------------------------------------------------------------------------------ host side
int sl_shape_ok(int B, int C, int H, int W, const char* what) {
    STX_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape B=%d C=%d H=%d W=%d", what, B, C, H, W);
    STX_REQUIRE((long long)H * W < (1ll << 30), "%s: image of %d x %d pixels too large", what, H, W);
    STX_REQUIRE((long long)B * C <= 65535, "%s: B * C = %lld planes exceed the grid's 65535", what, (long long)B * C);
    STX_REQUIRE((long long)B * C * H * W < (1ll << 38), "%s: tensor too large", what);
    return STX_OK;
}

int sl_warp_shape_ok(int B, int C, int H, int W, const char* what) {
    if (int rc = sl_shape_ok(B, C, H, W, what)) return rc;
    STX_REQUIRE(H >= 2 && W >= 2, "%s: the reference's grid needs H, W >= 2, got %d x %d", what, H, W);
    return STX_OK;
}

int sl_window_ok(int H, int W, int window, const char* what) {
    STX_REQUIRE(window >= 3 && window <= 2 * SL_MAX_PAD + 1 && (window & 1), "%s: window_size %d is not an odd size 3..%d", what, window,
                2 * SL_MAX_PAD + 1);
    STX_REQUIRE(H > window / 2 && W > window / 2, "%s: reflect padding by %d needs H, W > %d, got %d x %d", what, window / 2, window / 2, H,
                W);
    return STX_OK;
}

SlGeom sl_geom(int C, int H, int W, int window) {
    SlGeom g;
    g.C = C;
    g.H = H;
    g.W = W;
    g.p = window / 2;
    g.tilesX = stx_cdiv(W, SL_TW);
    g.sx = W > 1 ? (double)W / (double)(W - 1) : 1.0;
    g.sy = H > 1 ? (double)H / (double)(H - 1) : 1.0;
    return g;
}

inline unsigned sl_tiles(const SlGeom& g) { return (unsigned)(g.tilesX * stx_cdiv(g.H, SL_TH)); }
inline size_t sl_lds(const SlGeom& g, int tiles) { return (size_t)tiles * (SL_TH + 2 * g.p) * (SL_TW + 2 * g.p) * sizeof(float); }
inline unsigned sl_pixel_grid(long long npix) { return (unsigned)((npix + SL_THREADS - 1) / SL_THREADS); }

inline int sl_smooth_blocks(int H, int W) {
    const long long n = ((long long)H * W + 8 * SL_THREADS - 1) / (8 * SL_THREADS);
    return (int)(n < 1 ? 1 : (n > SL_SMOOTH_MAX_BLOCKS ? SL_SMOOTH_MAX_BLOCKS : n));
}

}  // namespace

extern "C" int stx_photo_warp_fwd(const float* right, const float* disp, float* warped, float* valid, int B, int C, int H, int W,
                                  void* stream) {
    stx_begin();
    const char* what = "photo_warp_fwd";
    STX_REQUIRE(right && disp && warped && valid, "%s: null pointer", what);
    if (int rc = sl_warp_shape_ok(B, C, H, W, what)) return rc;
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(sl_warp_fwd_kernel, dim3(sl_pixel_grid(npix)), dim3(SL_THREADS), 0, (hipStream_t)stream, right, disp, warped, valid,
                       sl_geom(C, H, W, 1), npix);
    return stx_check_launch(what);
}

extern "C" int stx_photo_warp_bwd(const float* gwarped, const float* right, const float* disp, float* gdisp, int B, int C, int H, int W,
                                  void* stream) {
    stx_begin();
    const char* what = "photo_warp_bwd";
    STX_REQUIRE(gwarped && right && disp && gdisp, "%s: null pointer", what);
    if (int rc = sl_warp_shape_ok(B, C, H, W, what)) return rc;
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(sl_warp_bwd_kernel, dim3(sl_pixel_grid(npix)), dim3(SL_THREADS), 0, (hipStream_t)stream, gwarped, right, disp, gdisp,
                       sl_geom(C, H, W, 1), npix);
    return stx_check_launch(what);
}

extern "C" int stx_ssim_fwd(const float* x, const float* y, float* out, int B, int C, int H, int W, int window, void* stream) {
    stx_begin();
    const char* what = "ssim_fwd";
    STX_REQUIRE(x && y && out, "%s: null pointer", what);
    if (int rc = sl_shape_ok(B, C, H, W, what)) return rc;
    if (int rc = sl_window_ok(H, W, window, what)) return rc;
    const SlGeom g = sl_geom(C, H, W, window);
    const size_t lds = sl_lds(g, 2);
    if (int rc = stx_lds_require((const void*)sl_ssim_fwd_kernel, lds, what)) return rc;
    hipLaunchKernelGGL(sl_ssim_fwd_kernel, dim3(sl_tiles(g), (unsigned)(B * C)), dim3(SL_THREADS), lds, (hipStream_t)stream, x, y, out, g);
    return stx_check_launch(what);
}

extern "C" long long stx_ssim_bwd_workspace_floats(int B, int C, int H, int W) { return 4ll * B * C * H * W; }

extern "C" int stx_ssim_bwd(const float* g_out, const float* x, const float* y, float* gx, float* gy, float* workspace, int B, int C,
                            int H, int W, int window, void* stream) {
    stx_begin();
    const char* what = "ssim_bwd";
    STX_REQUIRE(g_out && x && y && workspace && (gx || gy), "%s: null pointer", what);
    if (int rc = sl_shape_ok(B, C, H, W, what)) return rc;
    if (int rc = sl_window_ok(H, W, window, what)) return rc;
    const SlGeom g = sl_geom(C, H, W, window);
    const size_t n = (size_t)B * C * H * W;
    float *ay = workspace, *ax = ay + n, *cb = ax + n, *cc = cb + n;
    const dim3 grid(sl_tiles(g), (unsigned)(B * C));
    size_t lds = sl_lds(g, 2);
    if (int rc = stx_lds_require((const void*)sl_coef_kernel<false>, lds, what)) return rc;
    hipLaunchKernelGGL(sl_coef_kernel<false>, grid, dim3(SL_THREADS), lds, (hipStream_t)stream, g_out, x, y, (const float*)nullptr, 1.0, 0,
                       ay, ax, cb, cc, (float*)nullptr, g);
    if (int rc = stx_check_launch(what)) return rc;
    lds = sl_lds(g, 6);
    if (int rc = stx_lds_require((const void*)sl_ssim_gather_kernel, lds, what)) return rc;
    hipLaunchKernelGGL(sl_ssim_gather_kernel, grid, dim3(SL_THREADS), lds, (hipStream_t)stream, (const float*)ay, (const float*)ax,
                       (const float*)cb, (const float*)cc, x, y, gx, gy, g);
    return stx_check_launch(what);
}

extern "C" int stx_photometric_fwd(const float* left, const float* right, const float* disp, double ssim_weight, int enable_mask,
                                   float* loss, int B, int C, int H, int W, void* stream) {
    stx_begin();
    const char* what = "photometric_fwd";
    STX_REQUIRE(left && right && loss, "%s: null pointer", what);
    STX_REQUIRE(disp || !enable_mask, "%s: enable_mask needs a disparity (there is no valid_mask without a warp)", what);
    if (int rc = disp ? sl_warp_shape_ok(B, C, H, W, what) : sl_shape_ok(B, C, H, W, what)) return rc;
    if (int rc = sl_window_ok(H, W, SL_PHOTO_WINDOW, what)) return rc;
    const SlGeom g = sl_geom(C, H, W, SL_PHOTO_WINDOW);
    const size_t lds = sl_lds(g, 2);
    if (int rc = stx_lds_require((const void*)sl_photo_fwd_kernel<false>, lds, what)) return rc;
    const SlDenorm dn{{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, 0};
    hipLaunchKernelGGL(sl_photo_fwd_kernel<false>, dim3(sl_tiles(g), (unsigned)B), dim3(SL_THREADS), lds, (hipStream_t)stream, left, right,
                       disp, ssim_weight, enable_mask ? 1 : 0, dn, loss, (unsigned char*)nullptr, g);
    return stx_check_launch(what);
}

extern "C" long long stx_photometric_bwd_workspace_floats(int B, int C, int H, int W) { return 4ll * B * C * H * W; }

extern "C" int stx_photometric_bwd(const float* gloss, const float* left, const float* right, const float* disp, double ssim_weight,
                                   int enable_mask, float* gdisp, float* workspace, int B, int C, int H, int W, void* stream) {
    stx_begin();
    const char* what = "photometric_bwd";
    STX_REQUIRE(gloss && left && right && disp && gdisp && workspace, "%s: null pointer", what);
    if (int rc = sl_warp_shape_ok(B, C, H, W, what)) return rc;
    if (int rc = sl_window_ok(H, W, SL_PHOTO_WINDOW, what)) return rc;
    const SlGeom g = sl_geom(C, H, W, SL_PHOTO_WINDOW);
    const size_t n = (size_t)B * C * H * W;
    float *ay = workspace, *cb = ay + n, *cc = cb + n, *warped = cc + n;
    size_t lds = sl_lds(g, 2);
    if (int rc = stx_lds_require((const void*)sl_coef_kernel<true>, lds, what)) return rc;
    hipLaunchKernelGGL(sl_coef_kernel<true>, dim3(sl_tiles(g), (unsigned)(B * C)), dim3(SL_THREADS), lds, (hipStream_t)stream, gloss, left,
                       right, disp, ssim_weight, enable_mask ? 1 : 0, ay, (float*)nullptr, cb, cc, warped, g);
    if (int rc = stx_check_launch(what)) return rc;
    lds = sl_lds(g, 5);
    if (int rc = stx_lds_require((const void*)sl_photo_gather_kernel, lds, what)) return rc;
    hipLaunchKernelGGL(sl_photo_gather_kernel, dim3(sl_tiles(g), (unsigned)B), dim3(SL_THREADS), lds, (hipStream_t)stream, gloss,
                       (const float*)ay, (const float*)cb, (const float*)cc, left, (const float*)warped, right, disp, ssim_weight,
                       enable_mask ? 1 : 0, gdisp, g);
    return stx_check_launch(what);
}

extern "C" int stx_auto_mask_fwd(const float* left, const float* right, const float* disp, int denorm, unsigned char* mask, int B, int C,
                                 int H, int W, void* stream) {
    stx_begin();
    const char* what = "auto_mask_fwd";
    STX_REQUIRE(left && right && disp && mask, "%s: null pointer", what);
    STX_REQUIRE(!denorm || C == 3, "%s: denorm is defined for 3 channels, got %d", what, C);
    if (int rc = sl_warp_shape_ok(B, C, H, W, what)) return rc;
    if (int rc = sl_window_ok(H, W, SL_PHOTO_WINDOW, what)) return rc;
    const SlGeom g = sl_geom(C, H, W, SL_PHOTO_WINDOW);
    const size_t lds = sl_lds(g, 3);
    if (int rc = stx_lds_require((const void*)sl_photo_fwd_kernel<true>, lds, what)) return rc;
    const SlDenorm dn{{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, denorm ? 1 : 0};      // auto_mask.py:9-10
    hipLaunchKernelGGL(sl_photo_fwd_kernel<true>, dim3(sl_tiles(g), (unsigned)B), dim3(SL_THREADS), lds, (hipStream_t)stream, left, right,
                       disp, 0.85, 0, dn, (float*)nullptr, mask, g);
    return stx_check_launch(what);
}

extern "C" long long stx_smoothness_workspace_floats(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 7ll * B * sl_smooth_blocks(H, W);
}

extern "C" int stx_smoothness_fwd(const float* disp, const float* img, float* out, float* stats, float* workspace, int B, int C, int H,
                                  int W, void* stream) {
    stx_begin();
    const char* what = "smoothness_fwd";
    STX_REQUIRE(disp && img && out && stats && workspace, "%s: null pointer", what);
    if (int rc = sl_shape_ok(B, C, H, W, what)) return rc;
    STX_REQUIRE(H >= 2 && W >= 2, "%s: the differences need H, W >= 2, got %d x %d", what, H, W);
    STX_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "%s: workspace and stats hold doubles (8-byte aligned)", what);
    const int nblk = sl_smooth_blocks(H, W);
    SlSmoothWs ws;
    ws.psum = reinterpret_cast<double*>(workspace);
    ws.pterm = ws.psum + (size_t)B * nblk;
    ws.pmax = reinterpret_cast<float*>(ws.pterm + 2 * (size_t)B * nblk);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    hipLaunchKernelGGL(sl_smooth_stats_kernel, grid, dim3(SL_THREADS), 0, (hipStream_t)stream, disp, img, ws, C, (long long)H * W);
    if (int rc = stx_check_launch(what)) return rc;
    hipLaunchKernelGGL(sl_smooth_terms_kernel, grid, dim3(SL_THREADS), 0, (hipStream_t)stream, disp, img, ws, C, H, W);
    if (int rc = stx_check_launch(what)) return rc;
    hipLaunchKernelGGL(sl_smooth_final_kernel, dim3(1), dim3(SL_THREADS), 0, (hipStream_t)stream, ws, out, reinterpret_cast<double*>(stats),
                       B, nblk, H, W);
    return stx_check_launch(what);
}

extern "C" int stx_smoothness_bwd(const float* gout, const float* disp, const float* img, const float* stats, float* gdisp, int B, int C,
                                  int H, int W, void* stream) {
    stx_begin();
    const char* what = "smoothness_bwd";
    STX_REQUIRE(gout && disp && img && stats && gdisp, "%s: null pointer", what);
    if (int rc = sl_shape_ok(B, C, H, W, what)) return rc;
    STX_REQUIRE(H >= 2 && W >= 2, "%s: the differences need H, W >= 2, got %d x %d", what, H, W);
    STX_REQUIRE(((uintptr_t)stats & 7) == 0, "%s: stats hold doubles (8-byte aligned)", what);
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(sl_smooth_bwd_kernel, dim3(sl_pixel_grid(npix)), dim3(SL_THREADS), 0, (hipStream_t)stream, gout, disp, img,
                       reinterpret_cast<const double*>(stats), gdisp, B, C, H, W, npix);
    return stx_check_launch(what);
}

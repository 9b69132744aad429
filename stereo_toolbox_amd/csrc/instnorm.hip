// Instance normalisation with the activation and the residual tail fused, forward and backward, fp32 planes.
//
// nn.InstanceNorm2d / nn.InstanceNorm3d as the reference's feature and context networks build them (affine=False,
// track_running_stats=False, eps 1e-5, biased variance; train = eval): IGEV's BasicConv_IN / Conv2x_IN
// (models/IGEVStereo/submodule.py:82-150) and the ResidualBlock of the RAFT-family extractors (models/RAFTStereo/extractor.py:6-60).
// Per plane p = (b, c) of S contiguous floats:
//     xhat = (x - mean) rsqrt(var + eps),   y = act(xhat)   or, with a skip tensor,   y = relu(skip + act(xhat))
// act: 0 none, 1 ReLU, 3 LeakyReLU(0.01) -- the codes of stx_act (stx_common.h).
//
//   * B C is small (24-128 planes at B = 1) and the planes are large (35k-550k floats), so a plane is cut into chunks by a rule
//     of the shape alone (in_plan) and a workgroup owns one chunk.  Two launches, no grid barrier, no spin-wait:
//       (a) every workgroup leaves (sum x, sum x^2) of its chunk as two doubles;
//       (b) every workgroup adds its plane's partials in a fixed tree, in double, forms mean and rstd, evaluates the expression
//           above in double from the fp32 input and rounds once.  Chunk 0 of a plane writes (mean, rstd) for the backward.
//     Workgroup index = plane * chunks + chunk in both launches: the second read of x finds the tensor in L2 / Infinity Cache in
//     the order the first one left it.  A plane of one chunk takes ONE launch (IN_PATH_FUSED): the workgroup reduces and applies.
//   * backward, the same shape: g' = gy [y > 0 in the tail] act'(xhat), (a) per-chunk doubles of sum g' and sum g' xhat,
//     (b) gx = rstd (g' - sum g' / S - xhat sum g' xhat / S), gskip = gy [y > 0].  xhat and the masks are re-formed from x, skip,
//     mean and rstd by the forward's own expression (in_eval): y is never stored.  ReLU passes where its input is > 0, LeakyReLU
//     multiplies by 0.01 where xhat <= 0 (torch's conventions).
//   * 16-byte loads and stores.  The tensor base is 16-byte aligned (checked); a plane base is not when S is odd, so a chunk
//     is walked as scalar head (up to the next 16-byte boundary), vector body, scalar tail.  Which thread adds which element
//     follows from (plane, S) alone: no float atomics, the bits do not depend on anything but the shape and the data.
//   * the statistics are kept as doubles ([planes][2], 16 bytes a plane).  An fp32 mean would move every xhat of a plane by up to
//     rstd 2^-21 at |mean| ~ 10, three times the rounding of the result itself.
#include "stx_common.h"

namespace {

constexpr int IN_THREADS = 256;
constexpr long long IN_CHUNK_MIN = 1024;       // elements: one 16-byte vector per thread
constexpr long long IN_TARGET_WG = 1024;       // workgroups asked for (4 per CU)
constexpr int IN_MAX_CHUNKS = IN_THREADS;      // the partials of a plane are added by one tree of the workgroup
constexpr int IN_PATH_FUSED = 0, IN_PATH_SPLIT = 1;
constexpr double IN_SLOPE = 0.01;
constexpr size_t IN_LDS = 2 * IN_THREADS * sizeof(double);   // the reduction tree of in_block_sum2

struct InPlan {
    int chunks;            // per plane
    int len;               // elements of a chunk (a multiple of 4; the last one holds the rest)
    int path;
};

// The chunk rule: a function of (planes, S) only.
inline InPlan in_plan(long long planes, long long S) {
    long long n = (IN_TARGET_WG + planes - 1) / planes;
    const long long most = (S + IN_CHUNK_MIN - 1) / IN_CHUNK_MIN;
    if (n > most) n = most;
    if (n > IN_MAX_CHUNKS) n = IN_MAX_CHUNKS;
    if (n < 1) n = 1;
    long long len = ((S + n - 1) / n + 3) & ~3ll;
    InPlan p;
    p.len = (int)len;
    p.chunks = (int)((S + len - 1) / len);
    p.path = p.chunks == 1 ? IN_PATH_FUSED : IN_PATH_SPLIT;
    return p;
}

// Fixed-order tree over the workgroup for two values at once; every thread returns the totals.
__device__ __forceinline__ void in_block_sum2(double& a, double& b, double (*red)[IN_THREADS]) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[0][tid] = a;
    red[1][tid] = b;
    __syncthreads();
    for (int s = IN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    a = red[0][0];
    b = red[1][0];
}

// The walk of one chunk: f(i, n) for n = 4 (16-byte aligned offset i of the chunk) or n = 1.  `a0` = the chunk's first element,
// counted from the tensor base.
template <typename F>
__device__ __forceinline__ void in_walk(size_t a0, int len, F f) {
    const int tid = threadIdx.x;
    int head = (int)((4u - (unsigned)(a0 & 3u)) & 3u);
    if (head > len) head = len;
    const int nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    for (int v = tid; v < nvec; v += IN_THREADS) f(head + 4 * v, 4);
    if (tid < head) f(tid, 1);
    if (tid < len - tail0) f(tail0 + tid, 1);
}

__device__ __forceinline__ void in_ld(const float* p, int n, float* v) {
    if (n == 4) {
        const float4 t = stx_ld4(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

__device__ __forceinline__ void in_st(float* p, int n, const float* v) {
    if (n == 4) stx_st4(p, make_float4(v[0], v[1], v[2], v[3]));
    else p[0] = v[0];
}

// One element, in double: xhat, the output, and d y / d xhat (the activation's slope times the tail's mask) with `pass` = the
// tail's mask alone.  Forward and backward share it, so the masks of the backward are the forward's.
struct InVal {
    double xh, y, slope;
    bool pass;
};

__device__ __forceinline__ InVal in_eval(float x, const float* skip, double mean, double rstd, int act) {
    InVal r;
    r.xh = ((double)x - mean) * rstd;
    const bool pos = r.xh > 0.0;
    double a = r.xh, d = 1.0;
    if (act == 1) {
        a = pos ? r.xh : 0.0;
        d = pos ? 1.0 : 0.0;
    } else if (act == 3) {
        a = pos ? r.xh : IN_SLOPE * r.xh;
        d = pos ? 1.0 : IN_SLOPE;
    }
    r.pass = true;
    if (skip) {
        a += (double)*skip;
        r.pass = a > 0.0;
        a = r.pass ? a : 0.0;
    }
    r.y = a;
    r.slope = r.pass ? d : 0.0;
    return r;
}

__device__ __forceinline__ void in_moments(double sx, double sxx, long long S, float eps, double& mean, double& rstd) {
    mean = sx / (double)S;
    double var = sxx / (double)S - mean * mean;
    var = var > 0.0 ? var : 0.0;
    rstd = 1.0 / sqrt(var + (double)eps);
}

// MODE 0: the chunk's partial sums.  MODE 1: apply from the plane's partials.  MODE 2: one chunk per plane, both in one launch.
// grid planes * chunks, workgroup (plane, chunk) = (blockIdx.x / chunks, blockIdx.x % chunks).
template <int MODE>
__global__ __launch_bounds__(IN_THREADS) void in_fwd_kernel(const float* __restrict__ x, const float* __restrict__ skip,
                                                            float* __restrict__ y, double* __restrict__ stats,
                                                            double* __restrict__ part, long long S, int clen, int chunks, int act,
                                                            float eps) {
    STX_DYN_SMEM(smem);
    double(*red)[IN_THREADS] = reinterpret_cast<double(*)[IN_THREADS]>(smem);
    const int tid = threadIdx.x;
    const size_t plane = blockIdx.x / (unsigned)chunks;
    const int c = (int)(blockIdx.x % (unsigned)chunks);
    const long long lo = (long long)c * clen;
    const int len = (int)(S - lo < clen ? S - lo : clen);
    const size_t a0 = plane * (size_t)S + (size_t)lo;
    const float* xp = x + a0;
    double sx = 0.0, sxx = 0.0;
    if (MODE != 1) {
        in_walk(a0, len, [&](int i, int n) {
            float v[4];
            in_ld(xp + i, n, v);
            for (int j = 0; j < n; ++j) {
                const double d = (double)v[j];
                sx += d;
                sxx += d * d;
            }
        });
        in_block_sum2(sx, sxx, red);
        if (MODE == 0) {
            if (tid == 0) {
                part[2 * (size_t)blockIdx.x] = sx;
                part[2 * (size_t)blockIdx.x + 1] = sxx;
            }
            return;
        }
    } else {
        if (tid < chunks) {
            sx = part[2 * (plane * chunks + tid)];
            sxx = part[2 * (plane * chunks + tid) + 1];
        }
        in_block_sum2(sx, sxx, red);
    }
    double mean, rstd;
    in_moments(sx, sxx, S, eps, mean, rstd);
    if (stats && c == 0 && tid == 0) {
        stats[2 * plane] = mean;
        stats[2 * plane + 1] = rstd;
    }
    const float* sp = skip ? skip + a0 : nullptr;
    float* yp = y + a0;
    in_walk(a0, len, [&](int i, int n) {
        float v[4], s[4], o[4];
        in_ld(xp + i, n, v);
        if (sp) in_ld(sp + i, n, s);
        for (int j = 0; j < n; ++j) o[j] = (float)in_eval(v[j], sp ? &s[j] : nullptr, mean, rstd, act).y;
        in_st(yp + i, n, o);
    });
}

// The backward in the same three modes.  gx NULL: nothing is summed, gskip alone is written (MODE 1 / 2).
template <int MODE>
__global__ __launch_bounds__(IN_THREADS) void in_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                            const float* __restrict__ skip, const double* __restrict__ stats,
                                                            float* __restrict__ gx, float* __restrict__ gskip,
                                                            double* __restrict__ part, long long S, int clen, int chunks, int act) {
    STX_DYN_SMEM(smem);
    double(*red)[IN_THREADS] = reinterpret_cast<double(*)[IN_THREADS]>(smem);
    const int tid = threadIdx.x;
    const size_t plane = blockIdx.x / (unsigned)chunks;
    const int c = (int)(blockIdx.x % (unsigned)chunks);
    const long long lo = (long long)c * clen;
    const int len = (int)(S - lo < clen ? S - lo : clen);
    const size_t a0 = plane * (size_t)S + (size_t)lo;
    const float* xp = x + a0;
    const float* gp = gy + a0;
    const float* sp = skip ? skip + a0 : nullptr;
    const double mean = stats[2 * plane], rstd = stats[2 * plane + 1];
    double s1 = 0.0, s2 = 0.0;
    if (MODE != 1) {
        if (gx) {                                                        // (uniform)
            in_walk(a0, len, [&](int i, int n) {
                float v[4], s[4], g[4];
                in_ld(xp + i, n, v);
                in_ld(gp + i, n, g);
                if (sp) in_ld(sp + i, n, s);
                for (int j = 0; j < n; ++j) {
                    const InVal e = in_eval(v[j], sp ? &s[j] : nullptr, mean, rstd, act);
                    const double gd = (double)g[j] * e.slope;
                    s1 += gd;
                    s2 += gd * e.xh;
                }
            });
            in_block_sum2(s1, s2, red);
        }
        if (MODE == 0) {
            if (tid == 0) {
                part[2 * (size_t)blockIdx.x] = s1;
                part[2 * (size_t)blockIdx.x + 1] = s2;
            }
            return;
        }
    } else if (gx) {
        if (tid < chunks) {
            s1 = part[2 * (plane * chunks + tid)];
            s2 = part[2 * (plane * chunks + tid) + 1];
        }
        in_block_sum2(s1, s2, red);
    }
    const double m1 = s1 / (double)S, m2 = s2 / (double)S;
    float* gxp = gx ? gx + a0 : nullptr;
    float* gsp = gskip ? gskip + a0 : nullptr;
    in_walk(a0, len, [&](int i, int n) {
        float v[4], s[4], g[4], o[4], os[4];
        in_ld(xp + i, n, v);
        in_ld(gp + i, n, g);
        if (sp) in_ld(sp + i, n, s);
        for (int j = 0; j < n; ++j) {
            const InVal e = in_eval(v[j], sp ? &s[j] : nullptr, mean, rstd, act);
            o[j] = (float)(rstd * (((double)g[j] * e.slope - m1) - e.xh * m2));
            os[j] = e.pass ? g[j] : 0.f;
        }
        if (gxp) in_st(gxp + i, n, o);
        if (gsp) in_st(gsp + i, n, os);
    });
}

int in_args_ok(long long planes, long long S, int layout, int act, const char* what) {
    STX_REQUIRE(layout == 0, "%s: layout %d is not served by the kernels (0 = planes of S contiguous floats, NCHW / NCDHW; a "
                "channels-last tensor goes through one layout copy in the binding)", what, layout);
    STX_REQUIRE(planes >= 1 && S >= 2, "%s: at least one plane of at least 2 elements required (one value per plane has no variance: "
                "torch refuses it in training), got %lld planes of %lld", what, planes, S);
    STX_REQUIRE(S < (1ll << 31), "%s: %lld elements per plane are not served (2^31 and above)", what, S);
    STX_REQUIRE(act == 0 || act == 1 || act == 3, "%s: activation code %d (0 none, 1 ReLU, 3 LeakyReLU)", what, act);
    STX_REQUIRE(planes * (long long)in_plan(planes, S).chunks < (1ll << 31), "%s: %lld planes are too many workgroups", what, planes);
    return STX_OK;
}

inline bool in_aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" int stx_instnorm_plan(long long planes, long long S, int layout, int* chunks, int* path) {
    if (int rc = in_args_ok(planes, S, layout, 0, "instnorm_plan")) return rc;
    const InPlan p = in_plan(planes, S);
    if (chunks) *chunks = p.chunks;
    if (path) *path = p.path;
    return STX_OK;
}

extern "C" long long stx_instnorm_ws_bytes(long long planes, long long S, int layout) {
    if (in_args_ok(planes, S, layout, 0, "instnorm_ws_bytes")) return -1;
    const InPlan p = in_plan(planes, S);
    return p.path == IN_PATH_FUSED ? 0 : planes * (long long)p.chunks * 2 * (long long)sizeof(double);
}

extern "C" int stx_instnorm_fwd(const float* x, const float* skip, float* y, void* stats, void* ws, long long planes, long long S,
                                int layout, int act, float eps, void* stream) {
    stx_begin();
    const char* what = "instnorm_fwd";
    STX_REQUIRE(x && y, "%s: null pointer", what);
    if (int rc = in_args_ok(planes, S, layout, act, what)) return rc;
    STX_REQUIRE(in_aligned16(x) && in_aligned16(y) && in_aligned16(skip), "%s: x, skip and y must be 16-byte aligned", what);
    STX_REQUIRE(((size_t)stats & 7) == 0 && ((size_t)ws & 7) == 0, "%s: stats and workspace must be 8-byte aligned", what);
    STX_REQUIRE(eps >= 0.f, "%s: eps %g", what, (double)eps);
    const InPlan p = in_plan(planes, S);
    const dim3 grid((unsigned)(planes * p.chunks)), block(IN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (p.path == IN_PATH_FUSED) {
        if (int rc = stx_lds_require((const void*)in_fwd_kernel<2>, IN_LDS, what)) return rc;
        hipLaunchKernelGGL(in_fwd_kernel<2>, grid, block, IN_LDS, st, x, skip, y, (double*)stats, (double*)nullptr, S, p.len, p.chunks, act, eps);
        return stx_check_launch(what);
    }
    STX_REQUIRE(ws, "%s: %lld planes of %lld need a workspace (stx_instnorm_ws_bytes)", what, planes, S);
    if (int rc = stx_lds_require((const void*)in_fwd_kernel<0>, IN_LDS, what)) return rc;
    if (int rc = stx_lds_require((const void*)in_fwd_kernel<1>, IN_LDS, what)) return rc;
    hipLaunchKernelGGL(in_fwd_kernel<0>, grid, block, IN_LDS, st, x, skip, y, (double*)stats, (double*)ws, S, p.len, p.chunks, act, eps);
    if (int rc = stx_check_launch(what)) return rc;
    hipLaunchKernelGGL(in_fwd_kernel<1>, grid, block, IN_LDS, st, x, skip, y, (double*)stats, (double*)ws, S, p.len, p.chunks, act, eps);
    return stx_check_launch(what);
}

extern "C" int stx_instnorm_bwd(const float* gy, const float* x, const float* skip, const void* stats, float* gx, float* gskip, void* ws,
                                long long planes, long long S, int layout, int act, void* stream) {
    stx_begin();
    const char* what = "instnorm_bwd";
    STX_REQUIRE(gy && x && stats, "%s: null pointer", what);
    STX_REQUIRE(gx || gskip, "%s: no gradient asked for", what);
    STX_REQUIRE(!gskip || skip, "%s: gskip without skip", what);
    if (int rc = in_args_ok(planes, S, layout, act, what)) return rc;
    STX_REQUIRE(in_aligned16(gy) && in_aligned16(x) && in_aligned16(skip) && in_aligned16(gx) && in_aligned16(gskip),
                "%s: gy, x, skip, gx and gskip must be 16-byte aligned", what);
    STX_REQUIRE(((size_t)stats & 7) == 0 && ((size_t)ws & 7) == 0, "%s: stats and workspace must be 8-byte aligned", what);
    const InPlan p = in_plan(planes, S);
    const dim3 grid((unsigned)(planes * p.chunks)), block(IN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const double* sd = (const double*)stats;
    if (p.path == IN_PATH_FUSED) {
        if (int rc = stx_lds_require((const void*)in_bwd_kernel<2>, IN_LDS, what)) return rc;
        hipLaunchKernelGGL(in_bwd_kernel<2>, grid, block, IN_LDS, st, gy, x, skip, sd, gx, gskip, (double*)nullptr, S, p.len, p.chunks, act);
        return stx_check_launch(what);
    }
    if (gx) {
        STX_REQUIRE(ws, "%s: %lld planes of %lld need a workspace (stx_instnorm_ws_bytes)", what, planes, S);
        if (int rc = stx_lds_require((const void*)in_bwd_kernel<0>, IN_LDS, what)) return rc;
        hipLaunchKernelGGL(in_bwd_kernel<0>, grid, block, IN_LDS, st, gy, x, skip, sd, gx, gskip, (double*)ws, S, p.len, p.chunks, act);
        if (int rc = stx_check_launch(what)) return rc;
    }
    if (int rc = stx_lds_require((const void*)in_bwd_kernel<1>, IN_LDS, what)) return rc;
    hipLaunchKernelGGL(in_bwd_kernel<1>, grid, block, IN_LDS, st, gy, x, skip, sd, gx, gskip, (double*)ws, S, p.len, p.chunks, act);
    return stx_check_launch(what);
}

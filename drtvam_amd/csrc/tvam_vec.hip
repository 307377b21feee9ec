// tvam_vec.hip — fused vector kernels of the linear L-BFGS step
// (lbfgs.py:146-275 of the reference, restated in drtvam_amd/lbfgs.py).
//
// The two-loop recursion only ever needs dot products between the current
// gradient g and the history pairs (s_i, y_i); written in terms of the Gram
// entries s_i.y_j, y_i.y_j, s_i.g, y_i.g, g.g it becomes scalar work, and the
// search direction is one linear combination of g, s_i, y_i.  So one step
// touches the n-vectors in three passes instead of ~4m + 10:
//   tvam_lbfgs_history   : s_new = p - p_old, y_new = g - g_old and every dot
//                          the recursion needs, in one read of p, p_old, g,
//                          g_old and the retained history;
//   tvam_lbfgs_direction : d = cg g + sum cs_j s_j + sum cy_j y_j;
//   tvam_axpy_clamp      : p_new = max(p + alpha d, lo) (update + clamp,
//                          optimize.py:316-318).
// Dot products accumulate in fp64 per thread, then per block, then over a
// fixed number of blocks in a fixed order (deterministic).
// tests/test_gpu_vec_kernels.py pins the dots layout, the fp64 accumulation and that determinism.
// The update passes of the first-order optimisers (SGD, Adam; the config's 'optimizer' entry) are
// at the end of the file: tvam_optim_kernel.
#include "tvam_plan.h"

#define TVAM_VB 256       // threads per block
#define TVAM_VGRID_MAX 2048  // most blocks of the reduction kernels (work[] holds grid * ndots doubles)
#define TVAM_HMAX 8
#define TVAM_VU 1  // grid-stride elements per loop trip (2 and 4: no faster, profiles/r06/vec/)

#include <algorithm>
#include <cstdlib>

// launch geometry knobs (read once): blocks of the history pass and of the direction pass
static int vec_knob(const char* name, int def) {
    const int x = tvam_knob(name, def);
    return x > 0 ? x : def;
}
static int hist_grid() {
    static const int g = std::min(vec_knob("TVAM_VEC_HGRID", 768), TVAM_VGRID_MAX);
    return g;
}
static int dir_grid() {
    static const int g = vec_knob("TVAM_VEC_DGRID", 1024);
    return g;
}

// a streamed float4, loaded non-temporal: every pass reads a history vector once, gigabytes before the
// next pass reads it again (direction pass 0.75 -> 0.65 ms at config 2's size, profiles/r06/vec/)
__device__ __forceinline__ float4 vld(const float* p, uint64_t i) {
    typedef float vf4 __attribute__((ext_vector_type(4)));
    const vf4 v = __builtin_nontemporal_load(reinterpret_cast<const vf4*>(p) + i);
    return make_float4(v.x, v.y, v.z, v.w);
}

struct VecPtrs {
    const float* s[TVAM_HMAX];
    const float* y[TVAM_HMAX];
};

// Segments of the vectors (tvam_lbfgs_history_rows / tvam_lbfgs_direction_rows): float4 index t
// of the part -> segment t / len4, float4 off4 + segment * stride4 + t % len4 (a band of DMD rows
// of every angle)
struct VecSeg {
    uint32_t len4;
    uint64_t stride4, off4;
};

__device__ __forceinline__ uint64_t vec_seg_index(const VecSeg& sg, uint64_t t) {
    const uint64_t a = t / sg.len4;
    return sg.off4 + a * sg.stride4 + (t - a * sg.len4);
}

__device__ __forceinline__ double warp_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Block-reduce ND accumulators and write this block's partials.
template <int ND>
__device__ __forceinline__ void block_partials(double (&acc)[ND], double* __restrict__ work) {
    __shared__ double red[TVAM_VB / 64][ND > 0 ? ND : 1];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const double v = warp_sum(acc[d]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][d] = v;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < ND; d += TVAM_VB) {
        double s = 0.0;
        for (int w = 0; w < TVAM_VB / 64; ++w) s += red[w][d];
        work[(size_t)blockIdx.x * ND + d] = s;
    }
}

// Dots written (H = retained pairs, NEW = a new pair is formed; index j runs
// over the retained pairs, then the new one):
//   [0, HT)        s_j . g          HT = H + NEW
//   [HT, 2HT)      y_j . g
//   if NEW:
//   [2HT, 3HT)     s_new . y_j
//   [3HT, 4HT)     s_j . y_new
//   [4HT, 5HT)     y_new . y_j
//   last           g . g
template <int H, bool NEW>
struct HistLayout {
    static constexpr int HT = H + (NEW ? 1 : 0);
    static constexpr int ND = (NEW ? 5 * HT : 2 * HT) + 1;
};

// SPRE: s_new already holds p - p_old (written by the previous step's update, tvam_axpy_clamp_dev's
// s_out): read instead of formed from p and p_old (two vector reads and a write fewer)
template <int H, bool NEW, bool SEG = false, bool SPRE = false>
__global__ __launch_bounds__(TVAM_VB) void tvam_lbfgs_hist_kernel(uint64_t n, const float* __restrict__ p,
                                                                   const float* __restrict__ p_old,
                                                                   const float* __restrict__ g,
                                                                   const float* __restrict__ g_old, VecPtrs hv,
                                                                   float* __restrict__ s_new,
                                                                   float* __restrict__ y_new,
                                                                   double* __restrict__ work, VecSeg sg) {
    using L = HistLayout<H, NEW>;
    constexpr int HT = L::HT, ND = L::ND;
    double acc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) acc[d] = 0.0;

    auto visit = [&](float pv, float pov, float gv, float gov, const float (&sv)[TVAM_HMAX],
                     const float (&yv)[TVAM_HMAX], float& sn, float& yn) {
        sn = NEW ? pv - pov : 0.0f;
        yn = NEW ? gv - gov : 0.0f;
#pragma unroll
        for (int j = 0; j < HT; ++j) {
            const float sj = j < H ? sv[j] : sn, yj = j < H ? yv[j] : yn;
            acc[j] = fma((double)sj, (double)gv, acc[j]);
            acc[HT + j] = fma((double)yj, (double)gv, acc[HT + j]);
            if (NEW) {
                acc[2 * HT + j] = fma((double)sn, (double)yj, acc[2 * HT + j]);
                acc[3 * HT + j] = fma((double)sj, (double)yn, acc[3 * HT + j]);
                acc[4 * HT + j] = fma((double)yn, (double)yj, acc[4 * HT + j]);
            }
        }
        acc[ND - 1] = fma((double)gv, (double)gv, acc[ND - 1]);
    };

    const uint64_t n4 = n / 4, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // VU grid-stride elements per trip, all their loads issued before the first is summed (more bytes
    // in flight per wave); each thread still sums its elements in grid-stride order (the same dots)
    struct El {
        float4 g4, p4, po4, go4, s4[H > 0 ? H : 1], y4[H > 0 ? H : 1];
    };
    for (uint64_t t0 = tid; t0 < n4; t0 += (uint64_t)TVAM_VU * stride) {
        El el[TVAM_VU];
#pragma unroll
        for (int u = 0; u < TVAM_VU; ++u) {
            const uint64_t t = t0 + (uint64_t)u * stride;
            if (t >= n4) break;
            const uint64_t i = SEG ? vec_seg_index(sg, t) : t;
            el[u].g4 = vld(g, i);
            el[u].p4 = el[u].po4 = el[u].go4 = make_float4(0, 0, 0, 0);
            if (NEW) {
                if (SPRE) {
                    el[u].p4 = vld(s_new, i);  // s_new = p - p_old, with p_old = 0 below
                } else {
                    el[u].p4 = vld(p, i);
                    el[u].po4 = vld(p_old, i);
                }
                el[u].go4 = vld(g_old, i);
            }
#pragma unroll
            for (int j = 0; j < H; ++j) {
                el[u].s4[j] = vld(hv.s[j], i);
                el[u].y4[j] = vld(hv.y[j], i);
            }
        }
#pragma unroll
        for (int u = 0; u < TVAM_VU; ++u) {
            const uint64_t t = t0 + (uint64_t)u * stride;
            if (t >= n4) break;
            const uint64_t i = SEG ? vec_seg_index(sg, t) : t;
            const El& e = el[u];
            float sv[TVAM_HMAX], yv[TVAM_HMAX];
            float4 sn4, yn4;
#define TVAM_LANE(c)                                                    \
            _Pragma("unroll") for (int j = 0; j < H; ++j) {             \
                sv[j] = e.s4[j].c;                                      \
                yv[j] = e.y4[j].c;                                      \
            }                                                           \
            visit(e.p4.c, e.po4.c, e.g4.c, e.go4.c, sv, yv, sn4.c, yn4.c);
            TVAM_LANE(x) TVAM_LANE(y) TVAM_LANE(z) TVAM_LANE(w)
#undef TVAM_LANE
            if (NEW) {
                if (!SPRE) reinterpret_cast<float4*>(s_new)[i] = sn4;
                reinterpret_cast<float4*>(y_new)[i] = yn4;
            }
        }
    }
    for (uint64_t i = 4 * n4 + tid; !SEG && i < n; i += stride) {  // tail
        float sv[TVAM_HMAX], yv[TVAM_HMAX];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            sv[j] = hv.s[j][i];
            yv[j] = hv.y[j][i];
        }
        float sn, yn;
        visit(NEW ? (SPRE ? s_new[i] : p[i]) : 0.0f, NEW && !SPRE ? p_old[i] : 0.0f, g[i], NEW ? g_old[i] : 0.0f, sv,
              yv, sn, yn);
        if (NEW) {
            if (!SPRE) s_new[i] = sn;
            y_new[i] = yn;
        }
    }
    block_partials<ND>(acc, work);
}

// Sum the per-block partials of dot d over the blocks, in block order.
__global__ __launch_bounds__(TVAM_VB) void tvam_partials_kernel(int nd, int nblocks, const double* __restrict__ work,
                                                                double* __restrict__ dots) {
    __shared__ double red[TVAM_VB / 64];
    const int d = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += TVAM_VB) s += work[(size_t)b * nd + d];
    s = warp_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < TVAM_VB / 64; ++w) t += red[w];
        dots[d] = t;
    }
}

template <int H, bool NEW>
static hipError_t launch_hist(uint64_t n, const float* p, const float* p_old, const float* g, const float* g_old,
                              const VecPtrs& hv, float* s_new, float* y_new, double* work, double* dots,
                              hipStream_t stream, const VecSeg& sg) {
    // a band of rows (sg.len4 > 0): fewer blocks, the rest of the GPU keeps the neighbouring band's adjoint
    const int nb = sg.len4 ? std::max(64, (int)std::min<uint64_t>(hist_grid(), (n / 4 + TVAM_VB - 1) / TVAM_VB))
                           : hist_grid();
    if (sg.len4)
        hipLaunchKernelGGL((tvam_lbfgs_hist_kernel<H, NEW, true>), dim3(nb), dim3(TVAM_VB), 0, stream, n, p, p_old, g,
                           g_old, hv, s_new, y_new, work, sg);
    else if (NEW && !p_old)  // s_new precomputed (tvam_lbfgs_history: g_old given, p_old NULL)
        hipLaunchKernelGGL((tvam_lbfgs_hist_kernel<H, NEW, false, true>), dim3(nb), dim3(TVAM_VB), 0, stream, n, p,
                           p_old, g, g_old, hv, s_new, y_new, work, sg);
    else
        hipLaunchKernelGGL((tvam_lbfgs_hist_kernel<H, NEW>), dim3(nb), dim3(TVAM_VB), 0, stream, n, p, p_old, g,
                           g_old, hv, s_new, y_new, work, sg);
    hipLaunchKernelGGL(tvam_partials_kernel, dim3(HistLayout<H, NEW>::ND), dim3(TVAM_VB), 0, stream,
                       HistLayout<H, NEW>::ND, nb, work, dots);
    return hipGetLastError();
}

template <bool NEW>
static hipError_t dispatch_hist(int h, uint64_t n, const float* p, const float* p_old, const float* g,
                                const float* g_old, const VecPtrs& hv, float* s_new, float* y_new, double* work,
                                double* dots, hipStream_t stream, const VecSeg& sg) {
    switch (h) {
#define TVAM_H(H) \
    case H: return launch_hist<H, NEW>(n, p, p_old, g, g_old, hv, s_new, y_new, work, dots, stream, sg);
        TVAM_H(0) TVAM_H(1) TVAM_H(2) TVAM_H(3) TVAM_H(4) TVAM_H(5) TVAM_H(6) TVAM_H(7)
#undef TVAM_H
        default: return hipErrorInvalidValue;
    }
}

static hipError_t tvam_launch_lbfgs_history(uint64_t n, const float* p, const float* p_old, const float* g,
                                            const float* g_old, int h, const float* const* S, const float* const* Y,
                                            float* s_new, float* y_new, double* work, double* dots, hipStream_t stream,
                                            uint64_t nseg = 0, uint64_t seg_len = 0, uint64_t seg_stride = 0,
                                            uint64_t seg_off = 0) {
    VecPtrs hv{};
    for (int j = 0; j < h; ++j) {
        hv.s[j] = S[j];
        hv.y[j] = Y[j];
    }
    VecSeg sg{};
    if (nseg > 0) {
        n = nseg * seg_len;
        sg.len4 = (uint32_t)(seg_len / 4);
        sg.stride4 = seg_stride / 4;
        sg.off4 = seg_off / 4;
    }
    if (p_old || g_old) return dispatch_hist<true>(h, n, p, p_old, g, g_old, hv, s_new, y_new, work, dots, stream, sg);
    return dispatch_hist<false>(h, n, p, p_old, g, g_old, hv, s_new, y_new, work, dots, stream, sg);
}

// ---------------------------------------------------------------------------
struct DirCoef {
    float cg;
    float cs[TVAM_HMAX], cy[TVAM_HMAX];
};

// DEV: the coefficients come from device memory (tvam_lbfgs_coef_kernel's output: cg, cs[8], cy[8]).
// SEG: n = the part's elements (segments x length), indices through VecSeg.
template <int H, bool DEV = false, bool SEG = false>
__global__ __launch_bounds__(TVAM_VB) void tvam_lbfgs_dir_kernel(uint64_t n, const float* __restrict__ g, VecPtrs hv,
                                                                  DirCoef c, const float* __restrict__ cdev,
                                                                  float* __restrict__ d, VecSeg sg = VecSeg{}) {
    if (DEV) {
        c.cg = cdev[0];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            c.cs[j] = cdev[1 + j];
            c.cy[j] = cdev[1 + TVAM_HMAX + j];
        }
    }
    const uint64_t n4 = n / 4, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t t0 = tid; t0 < n4; t0 += (uint64_t)TVAM_VU * stride) {
        float4 g4[TVAM_VU], s4[TVAM_VU][H > 0 ? H : 1], y4[TVAM_VU][H > 0 ? H : 1];
#pragma unroll
        for (int u = 0; u < TVAM_VU; ++u) {  // every load of the trip first (bytes in flight)
            const uint64_t t = t0 + (uint64_t)u * stride;
            if (t >= n4) break;
            const uint64_t i = SEG ? vec_seg_index(sg, t) : t;
            g4[u] = vld(g, i);
#pragma unroll
            for (int j = 0; j < H; ++j) {
                s4[u][j] = vld(hv.s[j], i);
                y4[u][j] = vld(hv.y[j], i);
            }
        }
#pragma unroll
        for (int u = 0; u < TVAM_VU; ++u) {
            const uint64_t t = t0 + (uint64_t)u * stride;
            if (t >= n4) break;
            const uint64_t i = SEG ? vec_seg_index(sg, t) : t;
            float4 r = make_float4(c.cg * g4[u].x, c.cg * g4[u].y, c.cg * g4[u].z, c.cg * g4[u].w);
#pragma unroll
            for (int j = 0; j < H; ++j) {
                r.x = fmaf(c.cs[j], s4[u][j].x, fmaf(c.cy[j], y4[u][j].x, r.x));
                r.y = fmaf(c.cs[j], s4[u][j].y, fmaf(c.cy[j], y4[u][j].y, r.y));
                r.z = fmaf(c.cs[j], s4[u][j].z, fmaf(c.cy[j], y4[u][j].z, r.z));
                r.w = fmaf(c.cs[j], s4[u][j].w, fmaf(c.cy[j], y4[u][j].w, r.w));
            }
            reinterpret_cast<float4*>(d)[i] = r;
        }
    }
    for (uint64_t i = 4 * n4 + tid; !SEG && i < n; i += stride) {
        float r = c.cg * g[i];
#pragma unroll
        for (int j = 0; j < H; ++j) r = fmaf(c.cs[j], hv.s[j][i], fmaf(c.cy[j], hv.y[j][i], r));
        d[i] = r;
    }
}

static hipError_t tvam_launch_lbfgs_direction(uint64_t n, const float* g, int h, const float* const* S,
                                       const float* const* Y, float cg, const float* cs, const float* cy, float* d,
                                       hipStream_t stream) {
    VecPtrs hv{};
    DirCoef c{};
    c.cg = cg;
    for (int j = 0; j < h; ++j) {
        hv.s[j] = S[j];
        hv.y[j] = Y[j];
        c.cs[j] = cs[j];
        c.cy[j] = cy[j];
    }
    const dim3 grid(dir_grid()), block(TVAM_VB);
    switch (h) {
#define TVAM_H(H) \
    case H: hipLaunchKernelGGL(tvam_lbfgs_dir_kernel<H>, grid, block, 0, stream, n, g, hv, c, nullptr, d, VecSeg{}); break;
        TVAM_H(0) TVAM_H(1) TVAM_H(2) TVAM_H(3) TVAM_H(4) TVAM_H(5) TVAM_H(6) TVAM_H(7) TVAM_H(8)
#undef TVAM_H
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The two-loop recursion on the device (lbfgs.py:221-243 in Gram form, as the host recursion of
// drtvam_amd/lbfgs.py evaluated it before): one lane, so the direction pass follows the history
// pass and its all-reduce on the stream without a host round trip.  gram[] keeps the retained
// pairs' entries between steps, indexed by ring slot: s_a.y_b at [a][b], y_a.y_b at 64 + [a][b];
// a new pair's entries come from the history pass's dots.  The same fp64 operations in the same
// order as that host code (no contraction), so the f32-rounded coefficients -- and the
// direction -- are bit-identical to it.  coef: cg | cs[8] | cy[8]; gdz: g.d (the Armijo slope).
struct LbfgsOrder {
    int slot[TVAM_HMAX];
};

__global__ void tvam_lbfgs_coef_kernel(int H, int is_new, int first, LbfgsOrder o, const double* __restrict__ dots,
                                       double* __restrict__ gram, float* __restrict__ coef,
                                       double* __restrict__ gdz) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double* SY = gram;
    double* YY = gram + TVAM_HMAX * TVAM_HMAX;
    const double* Sg = dots;
    const double* Yg = dots + H;
    const double gg = dots[(is_new ? 5 * H : 2 * H)];
    if (is_new) {
        const int sl = o.slot[H - 1];
        for (int j = 0; j < H; ++j) {
            const int sj = o.slot[j];
            SY[sl * TVAM_HMAX + sj] = dots[2 * H + j];  // s_new . y_j
            SY[sj * TVAM_HMAX + sl] = dots[3 * H + j];  // s_j . y_new
            YY[sl * TVAM_HMAX + sj] = dots[4 * H + j];
            YY[sj * TVAM_HMAX + sl] = dots[4 * H + j];
        }
    }
    double a[TVAM_HMAX], b[TVAM_HMAX];
    for (int i = H - 1; i >= 0; --i) {
        const int si = o.slot[i];
        double s = 0.0;
        for (int j = i + 1; j < H; ++j) s = s + a[j] * SY[si * TVAM_HMAX + o.slot[j]];
        a[i] = (Sg[i] - s) / SY[si * TVAM_HMAX + si];
    }
    const int last = H > 0 ? o.slot[H - 1] : 0;
    const double gamma = (first || H == 0) ? 1.0 : SY[last * TVAM_HMAX + last] / YY[last * TVAM_HMAX + last];
    for (int i = 0; i < H; ++i) {
        const int yi = o.slot[i];
        double s1 = 0.0;
        for (int j = 0; j < H; ++j) s1 = s1 + a[j] * YY[yi * TVAM_HMAX + o.slot[j]];
        double yz = gamma * (Yg[i] - s1);
        double s2 = 0.0;
        for (int j = 0; j < i; ++j) s2 = s2 + (a[j] - b[j]) * SY[o.slot[j] * TVAM_HMAX + yi];
        yz = yz + s2;
        b[i] = yz / SY[yi * TVAM_HMAX + yi];
    }
    // d = -z, z = gamma (g - sum a_j y_j) + sum (a_j - b_j) s_j
    const double cg = -gamma;
    double r = cg * gg, rs = 0.0, ry = 0.0;
    coef[0] = (float)cg;
    for (int j = 0; j < H; ++j) {
        const double cs = -(a[j] - b[j]), cy = gamma * a[j];
        coef[1 + j] = (float)cs;
        coef[1 + TVAM_HMAX + j] = (float)cy;
        rs = rs + cs * Sg[j];
        ry = ry + cy * Yg[j];
    }
    gdz[0] = r + rs + ry;
}

static hipError_t tvam_launch_lbfgs_coef(int h, int is_new, int first, const int* order, const double* dots, double* gram,
                                  float* coef, double* gdz, hipStream_t stream) {
    LbfgsOrder o{};
    for (int j = 0; j < h; ++j) o.slot[j] = order[j];
    hipLaunchKernelGGL(tvam_lbfgs_coef_kernel, dim3(1), dim3(64), 0, stream, h, is_new, first, o, dots, gram, coef, gdz);
    return hipGetLastError();
}

static hipError_t tvam_launch_lbfgs_direction_dev(uint64_t n, const float* g, int h, const float* const* S,
                                                  const float* const* Y, const float* coef, float* d,
                                                  hipStream_t stream, uint64_t nseg = 0, uint64_t seg_len = 0,
                                                  uint64_t seg_stride = 0, uint64_t seg_off = 0) {
    VecPtrs hv{};
    for (int j = 0; j < h; ++j) {
        hv.s[j] = S[j];
        hv.y[j] = Y[j];
    }
    const DirCoef c{};
    VecSeg sg{};
    const bool seg = nseg > 0;
    if (seg) {
        n = nseg * seg_len;
        sg.len4 = (uint32_t)(seg_len / 4);
        sg.stride4 = seg_stride / 4;
        sg.off4 = seg_off / 4;
    }
    // a part of the vector: fewer blocks, so that the rest of the GPU keeps the forward of the
    // previous part (tvam_lbfgs_direction_rows)
    const int nb = seg ? std::max(64, (int)std::min<uint64_t>(dir_grid(), (n / 4 + TVAM_VB - 1) / TVAM_VB)) : dir_grid();
    const dim3 grid(nb), block(TVAM_VB);
    switch (h) {
#define TVAM_H(H)                                                                                                 \
    case H:                                                                                                       \
        if (seg)                                                                                                  \
            hipLaunchKernelGGL((tvam_lbfgs_dir_kernel<H, true, true>), grid, block, 0, stream, n, g, hv, c, coef, \
                               d, sg);                                                                            \
        else                                                                                                      \
            hipLaunchKernelGGL((tvam_lbfgs_dir_kernel<H, true>), grid, block, 0, stream, n, g, hv, c, coef, d,    \
                               sg);                                                                               \
        break;
        TVAM_H(0) TVAM_H(1) TVAM_H(2) TVAM_H(3) TVAM_H(4) TVAM_H(5) TVAM_H(6) TVAM_H(7) TVAM_H(8)
#undef TVAM_H
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// alpha_dev (tvam_axpy_clamp_dev): the step size read from device memory, tvam_armijo_kernel's pick
// s_out (optional): the next history pair's s = out - p (the fp32 difference tvam_lbfgs_history forms
// from p_new and p_old, so that pass reads it instead of both vectors)
__global__ __launch_bounds__(TVAM_VB) void tvam_axpy_clamp_kernel(uint64_t n, const float* __restrict__ p, float alpha,
                                                                  const float* __restrict__ d, float lo,
                                                                  float* __restrict__ out,
                                                                  const float* __restrict__ alpha_dev,
                                                                  float* __restrict__ s_out) {
    if (alpha_dev) alpha = alpha_dev[0];
    const uint64_t n4 = n / 4, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = tid; i < n4; i += stride) {
        const float4 p4 = reinterpret_cast<const float4*>(p)[i];
        const float4 d4 = reinterpret_cast<const float4*>(d)[i];
        const float4 o = make_float4(fmaxf(fmaf(alpha, d4.x, p4.x), lo), fmaxf(fmaf(alpha, d4.y, p4.y), lo),
                                     fmaxf(fmaf(alpha, d4.z, p4.z), lo), fmaxf(fmaf(alpha, d4.w, p4.w), lo));
        reinterpret_cast<float4*>(out)[i] = o;
        if (s_out) reinterpret_cast<float4*>(s_out)[i] = make_float4(o.x - p4.x, o.y - p4.y, o.z - p4.z, o.w - p4.w);
    }
    for (uint64_t i = 4 * n4 + tid; i < n; i += stride) {
        const float o = fmaxf(fmaf(alpha, d[i], p[i]), lo);
        out[i] = o;
        if (s_out) s_out[i] = o - p[i];
    }
}

static hipError_t tvam_launch_axpy_clamp(uint64_t n, const float* p, float alpha, const float* d, float lo, float* out,
                                         hipStream_t stream, const float* alpha_dev = nullptr,
                                         float* s_out = nullptr) {
    hipLaunchKernelGGL(tvam_axpy_clamp_kernel, dim3(2048), dim3(TVAM_VB), 0, stream, n, p, alpha, d, lo, out,
                       alpha_dev, s_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The first batch of Armijo probes decided on the device (FusedLinearLBFGS.step), so that the
// update p + alpha d can follow the probes on the stream while the host reads them: alpha[0] =
// a_j for the first probe j with f_j <= loss + c1 a_j g.d, a_j = a0 / 2^j (lbfgs.py:256-266), in
// the host loop's fp64 operations and order (no contraction); 0 when no probe passes (the host
// then discards the update launched behind it).  loss = loss_dev[0] / loss_div, or loss_host.
// report (optional, e.g. pinned host memory the host polls, no copy kernel and no event): the undivided
// loss, g.d, the probes and the chosen alpha, as f64, then 1.0 once they are visible system-wide.
__global__ void tvam_armijo_kernel(int nprobe, double a0, const double* __restrict__ probes,
                                   const double* __restrict__ loss_dev, double loss_host, double loss_div,
                                   const double* __restrict__ gdz, double c1, float* __restrict__ alpha,
                                   double* __restrict__ report) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double l0 = loss_dev ? loss_dev[0] : loss_host;
    const double lv = loss_dev ? l0 / loss_div : loss_host;
    const double gd = 0.0 + gdz[0];
    float r = 0.0f;
    for (int j = 0; j < nprobe; ++j) {
        const double a = a0 * ldexp(1.0, -j);
        if (probes[j] <= lv + c1 * a * gd) {
            r = (float)a;
            break;
        }
    }
    alpha[0] = r;
    if (report) {
        report[0] = l0;
        report[1] = gdz[0];
        for (int j = 0; j < nprobe; ++j) report[2 + j] = probes[j];
        report[2 + nprobe] = (double)r;
        __threadfence_system();
        report[3 + nprobe] = 1.0;
        __threadfence_system();
    }
}

static hipError_t tvam_launch_armijo(int nprobe, double a0, const double* probes, const double* loss_dev, double loss_host,
                              double loss_div, const double* gdz, double c1, float* alpha, double* report,
                              hipStream_t stream) {
    hipLaunchKernelGGL(tvam_armijo_kernel, dim3(1), dim3(64), 0, stream, nprobe, a0, probes, loss_dev, loss_host,
                       loss_div, gdz, c1, alpha, report);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// First-order optimisers (drtvam_amd/optimizers.py: Mitsuba's mi.ad.SGD / mi.ad.Adam for one
// parameter and a scalar learning rate), one fused pass over the pattern vector with the loop's
// clamp folded in.  Per element, every operation a separate once-rounded fp32 operation in this
// order (no contraction), keep = mask && g == 0:
//   SGD       w = p - lr g
//   SGDM      s' = mu s + g; w = p - lr s'; keep: s' = s
//   ADAM      m' = b1 m + c1 g; v' = b2 v + c2 (g g); keep: m' = m, v' = v;
//             den = sqrt(v') + e; w = p - (lr_t m') / den
//   MOMENTS   ADAM's m', v' only, and S = sum v' (fp64: per thread, per block, then
//             tvam_partials_kernel over the blocks in block order)
//   APPLY     den = fl32(sqrt(S / N)) + e (fp64 quotient and root, S and N from device memory);
//             w = p - (lr_t m') / den
//   all       keep: w = p; p' = w < lo ? lo : w
// p, s, m, v are updated in place.  A float4 main path from the 16-byte grid on, a scalar head up
// to it and a scalar tail; vectors that do not share one offset from that grid go through the
// scalar path whole.  tests/test_gpu_optimizers.py pins every output to the fp32 model of
// tests/optim_model.py bit for bit.
enum { TVAM_OPT_SGD, TVAM_OPT_SGDM, TVAM_OPT_ADAM, TVAM_OPT_MOMENTS, TVAM_OPT_APPLY };
#define TVAM_OPT_GRID 2048

struct OptimArgs {
    uint64_t n, head;  // head: leading entries of the scalar path
    float* p;
    const float* g;
    float* a;  // s | m
    float* b;  // v
    float lr, k1, c1, k2, c2, eps, lo;
    const double* S;
    const double* count;
    double* work;
};

template <int KIND, bool MASK>
__device__ __forceinline__ void optim_elem(float& p, float g, float& a, float& b, const OptimArgs& q, float den_u,
                                           double& acc) {
#pragma clang fp contract(off)
    const bool keep = MASK && g == 0.0f;
    float w;
    if (KIND == TVAM_OPT_SGD) {
        w = p - q.lr * g;
    } else if (KIND == TVAM_OPT_SGDM) {
        const float s1 = q.k1 * a + g;
        w = p - q.lr * s1;
        if (!keep) a = s1;
    } else {
        float den = den_u;
        if (KIND != TVAM_OPT_APPLY) {
            const float m1 = q.k1 * a + q.c1 * g;
            const float v1 = q.k2 * b + q.c2 * (g * g);
            if (!keep) {
                a = m1;
                b = v1;
            }
            den = __builtin_sqrtf(b) + q.eps;
        }
        if (KIND == TVAM_OPT_MOMENTS) {
            acc += (double)b;
            return;
        }
        w = p - (q.lr * a) / den;
    }
    if (keep) w = p;
    p = w < q.lo ? q.lo : w;
}

template <int KIND, bool MASK>
__global__ __launch_bounds__(TVAM_VB) void tvam_optim_kernel(OptimArgs q) {
    constexpr bool HP = KIND != TVAM_OPT_MOMENTS;            // p read and written
    constexpr bool HG = KIND != TVAM_OPT_APPLY || MASK;      // g read
    constexpr bool HA = KIND != TVAM_OPT_SGD;                // s | m read
    constexpr bool WA = HA && KIND != TVAM_OPT_APPLY;        //       and written
    constexpr bool HB = KIND == TVAM_OPT_ADAM || KIND == TVAM_OPT_MOMENTS;  // v read and written
    float den_u = 0.0f;
    if (KIND == TVAM_OPT_APPLY) den_u = (float)sqrt(q.S[0] / q.count[0]) + q.eps;
    double acc[1] = {0.0};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto scalar = [&](uint64_t i) {
        float p = 0.0f, g = 0.0f, a = 0.0f, b = 0.0f;
        if (HP) p = q.p[i];
        if (HG) g = q.g[i];
        if (HA) a = q.a[i];
        if (HB) b = q.b[i];
        optim_elem<KIND, MASK>(p, g, a, b, q, den_u, acc[0]);
        if (HP) q.p[i] = p;
        if (WA) q.a[i] = a;
        if (HB) q.b[i] = b;
    };
    for (uint64_t i = tid; i < q.head; i += stride) scalar(i);
    const uint64_t n4 = (q.n - q.head) / 4;
    for (uint64_t i = tid; i < n4; i += stride) {
        const float4 z = make_float4(0, 0, 0, 0);
        float4 p4 = z, g4 = z, a4 = z, b4 = z;
        if (HP) p4 = vld(q.p + q.head, i);
        if (HG) g4 = vld(q.g + q.head, i);
        if (HA) a4 = vld(q.a + q.head, i);
        if (HB) b4 = vld(q.b + q.head, i);
        optim_elem<KIND, MASK>(p4.x, g4.x, a4.x, b4.x, q, den_u, acc[0]);
        optim_elem<KIND, MASK>(p4.y, g4.y, a4.y, b4.y, q, den_u, acc[0]);
        optim_elem<KIND, MASK>(p4.z, g4.z, a4.z, b4.z, q, den_u, acc[0]);
        optim_elem<KIND, MASK>(p4.w, g4.w, a4.w, b4.w, q, den_u, acc[0]);
        if (HP) reinterpret_cast<float4*>(q.p + q.head)[i] = p4;
        if (WA) reinterpret_cast<float4*>(q.a + q.head)[i] = a4;
        if (HB) reinterpret_cast<float4*>(q.b + q.head)[i] = b4;
    }
    for (uint64_t i = q.head + 4 * n4 + tid; i < q.n; i += stride) scalar(i);
    if constexpr (KIND == TVAM_OPT_MOMENTS) block_partials<1>(acc, q.work);
}

// Entries up to the 16-byte grid when every vector in use sits at the same offset from it, else all n.
static uint64_t optim_head(uint64_t n, const void* const* v, int nv) {
    uintptr_t off = 0;
    bool first = true;
    for (int j = 0; j < nv; ++j) {
        if (!v[j]) continue;
        const uintptr_t o = (uintptr_t)v[j] & 15u;
        if (first) off = o;
        else if (o != off) return n;
        first = false;
    }
    if (off & 3u) return n;
    return std::min<uint64_t>(n, ((16u - off) & 15u) / 4);
}

template <int KIND>
static hipError_t launch_optim(bool mask, OptimArgs q, double* S_out, hipStream_t stream) {
    const void* v[4] = {q.p, q.g, q.a, q.b};
    q.head = optim_head(q.n, v, 4);
    const dim3 grid(TVAM_OPT_GRID), block(TVAM_VB);
    if (mask)
        hipLaunchKernelGGL((tvam_optim_kernel<KIND, true>), grid, block, 0, stream, q);
    else
        hipLaunchKernelGGL((tvam_optim_kernel<KIND, false>), grid, block, 0, stream, q);
    if (KIND == TVAM_OPT_MOMENTS)
        hipLaunchKernelGGL(tvam_partials_kernel, dim3(1), dim3(TVAM_VB), 0, stream, 1, TVAM_OPT_GRID, q.work, S_out);
    return hipGetLastError();
}

static hipError_t tvam_launch_sgd_step(uint64_t n, float* p, const float* g, float* s, float lr, float mu, bool mask,
                                float lo, hipStream_t stream) {
    OptimArgs q{};
    q.n = n, q.p = p, q.g = g, q.a = s, q.lr = lr, q.k1 = mu, q.lo = lo;
    return s ? launch_optim<TVAM_OPT_SGDM>(mask, q, nullptr, stream) : launch_optim<TVAM_OPT_SGD>(mask, q, nullptr, stream);
}

static hipError_t tvam_launch_adam_step(uint64_t n, float* p, const float* g, float* m, float* v, float lr_t, float b1,
                                 float c1, float b2, float c2, float eps, bool mask, float lo, hipStream_t stream) {
    OptimArgs q{};
    q.n = n, q.p = p, q.g = g, q.a = m, q.b = v, q.lr = lr_t, q.k1 = b1, q.c1 = c1, q.k2 = b2, q.c2 = c2;
    q.eps = eps, q.lo = lo;
    return launch_optim<TVAM_OPT_ADAM>(mask, q, nullptr, stream);
}

static hipError_t tvam_launch_adam_moments(uint64_t n, const float* g, float* m, float* v, float b1, float c1, float b2,
                                    float c2, bool mask, double* work, double* S, hipStream_t stream) {
    OptimArgs q{};
    q.n = n, q.g = g, q.a = m, q.b = v, q.k1 = b1, q.c1 = c1, q.k2 = b2, q.c2 = c2, q.work = work;
    return launch_optim<TVAM_OPT_MOMENTS>(mask, q, S, stream);
}

static hipError_t tvam_launch_adam_apply(uint64_t n, float* p, const float* g, const float* m, const double* S,
                                  const double* count, float lr_t, float eps, bool mask, float lo,
                                  hipStream_t stream) {
    OptimArgs q{};
    q.n = n, q.p = p, q.g = mask ? g : nullptr, q.a = const_cast<float*>(m), q.S = S, q.count = count;
    q.lr = lr_t, q.eps = eps, q.lo = lo;
    return launch_optim<TVAM_OPT_APPLY>(mask, q, nullptr, stream);
}

// The extern "C" boundary of these kernels (include/tvam.h).
static bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

extern "C" int tvam_lbfgs_history(uint64_t n, const float* p, const float* p_old, const float* g, const float* g_old,
                                  int32_t h, const float* const* S, const float* const* Y, float* s_new,
                                  float* y_new, double* work, double* dots, void* stream) {
    if (!g || !work || !dots || (h > 0 && (!S || !Y))) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (h < 0 || h > 7) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_history: 0 <= h <= 7 retained pairs");
    if (p_old && (!p || !g_old || !s_new || !y_new)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    // p_old NULL with g_old given: a new pair whose s_new already holds p - p_old (read, not written)
    const bool spre = !p_old && g_old;
    if (spre && (!s_new || !y_new)) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_history: precomputed s_new needs s_new, y_new");
    bool ok = aligned16(g) && (!p_old || (aligned16(p) && aligned16(p_old) && aligned16(g_old) &&
                                          aligned16(s_new) && aligned16(y_new))) &&
              (!spre || (aligned16(g_old) && aligned16(s_new) && aligned16(y_new)));
    for (int j = 0; j < h; ++j) ok = ok && S[j] && Y[j] && aligned16(S[j]) && aligned16(Y[j]);
    if (!ok) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_history: vectors must be 16-byte aligned");
    hipError_t e = tvam_launch_lbfgs_history(n, p, p_old, g, g_old, h, S, Y, s_new, y_new, work, dots,
                                             (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "lbfgs history launch");
}

extern "C" int tvam_lbfgs_history_rows(uint64_t nseg, uint64_t seg_len, uint64_t seg_stride, uint64_t seg_off,
                                       const float* p, const float* p_old, const float* g, const float* g_old,
                                       int32_t h, const float* const* S, const float* const* Y, float* s_new,
                                       float* y_new, double* work, double* dots, void* stream) {
    if (!g || !work || !dots || (h > 0 && (!S || !Y))) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (h < 0 || h > 7) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_history_rows: 0 <= h <= 7 retained pairs");
    if (p_old && (!p || !g_old || !s_new || !y_new)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (!p_old && g_old) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_history_rows: g_old without p_old");
    if (nseg == 0 || seg_len == 0 || seg_len % 4 || seg_stride % 4 || seg_off % 4 || seg_len > seg_stride ||
        seg_len / 4 > 0xffffffffull)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_history_rows: segments of a multiple of 4 entries, 4-aligned");
    bool ok = aligned16(g) && (!p_old || (aligned16(p) && aligned16(p_old) && aligned16(g_old) &&
                                          aligned16(s_new) && aligned16(y_new)));
    for (int j = 0; j < h; ++j) ok = ok && S[j] && Y[j] && aligned16(S[j]) && aligned16(Y[j]);
    if (!ok) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_history_rows: vectors must be 16-byte aligned");
    hipError_t e = tvam_launch_lbfgs_history(0, p, p_old, g, g_old, h, S, Y, s_new, y_new, work, dots,
                                             (hipStream_t)stream, nseg, seg_len, seg_stride, seg_off);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "lbfgs history launch");
}

extern "C" int tvam_lbfgs_direction(uint64_t n, const float* g, int32_t h, const float* const* S,
                                    const float* const* Y, float cg, const float* cs, const float* cy, float* d,
                                    void* stream) {
    if (!g || !d || (h > 0 && (!S || !Y || !cs || !cy))) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (h < 0 || h > 8) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_direction: 0 <= h <= 8 pairs");
    bool ok = aligned16(g) && aligned16(d);
    for (int j = 0; j < h; ++j) ok = ok && S[j] && Y[j] && aligned16(S[j]) && aligned16(Y[j]);
    if (!ok) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_direction: vectors must be 16-byte aligned");
    hipError_t e = tvam_launch_lbfgs_direction(n, g, h, S, Y, cg, cs, cy, d, (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "lbfgs direction launch");
}

extern "C" int tvam_lbfgs_coef(int32_t h, int32_t is_new, int32_t first, const int32_t* order, const double* dots,
                               double* gram, float* coef, double* gdz, void* stream) {
    if (h < 0 || h > 8) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_coef: 0 <= h <= 8 pairs");
    if (!dots || !gram || !coef || !gdz || (h > 0 && !order)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (is_new && h == 0) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_coef: a new pair needs h >= 1");
    for (int j = 0; j < h; ++j)
        if (order[j] < 0 || order[j] >= 8) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_coef: ring slots are 0..7");
    hipError_t e = tvam_launch_lbfgs_coef(h, is_new ? 1 : 0, first ? 1 : 0, order, dots, gram, coef, gdz,
                                          (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "lbfgs coefficient launch");
}

extern "C" int tvam_lbfgs_direction_dev(uint64_t n, const float* g, int32_t h, const float* const* S,
                                        const float* const* Y, const float* coef, float* d, void* stream) {
    if (!g || !d || !coef || (h > 0 && (!S || !Y))) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (h < 0 || h > 8) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_direction_dev: 0 <= h <= 8 pairs");
    bool ok = aligned16(g) && aligned16(d);
    for (int j = 0; j < h; ++j) ok = ok && S[j] && Y[j] && aligned16(S[j]) && aligned16(Y[j]);
    if (!ok) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_direction_dev: vectors must be 16-byte aligned");
    hipError_t e = tvam_launch_lbfgs_direction_dev(n, g, h, S, Y, coef, d, (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "lbfgs direction launch");
}

extern "C" int tvam_lbfgs_direction_rows(uint64_t nseg, uint64_t seg_len, uint64_t seg_stride, uint64_t seg_off,
                                         const float* g, int32_t h, const float* const* S, const float* const* Y,
                                         const float* coef, float* d, void* stream) {
    if (!g || !d || !coef || (h > 0 && (!S || !Y))) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (h < 0 || h > 8) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_direction_rows: 0 <= h <= 8 pairs");
    if (nseg == 0 || seg_len == 0 || seg_len % 4 || seg_stride % 4 || seg_off % 4 || seg_len > seg_stride ||
        seg_len / 4 > 0xffffffffull)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_direction_rows: segments of a multiple of 4 entries, 4-aligned");
    bool ok = aligned16(g) && aligned16(d);
    for (int j = 0; j < h; ++j) ok = ok && S[j] && Y[j] && aligned16(S[j]) && aligned16(Y[j]);
    if (!ok) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_direction_rows: vectors must be 16-byte aligned");
    hipError_t e = tvam_launch_lbfgs_direction_dev(0, g, h, S, Y, coef, d, (hipStream_t)stream, nseg, seg_len,
                                                   seg_stride, seg_off);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "lbfgs direction launch");
}

extern "C" int tvam_axpy_clamp(uint64_t n, const float* p, float alpha, const float* d, float lo, float* out,
                               void* stream) {
    if (!p || !d || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (!aligned16(p) || !aligned16(d) || !aligned16(out))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_axpy_clamp: vectors must be 16-byte aligned");
    hipError_t e = tvam_launch_axpy_clamp(n, p, alpha, d, lo, out, (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "axpy launch");
}

extern "C" int tvam_axpy_clamp_dev(uint64_t n, const float* p, const float* alpha, const float* d, float lo,
                                   float* out, float* s_out, void* stream) {
    if (!p || !alpha || !d || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (!aligned16(p) || !aligned16(d) || !aligned16(out) || (s_out && !aligned16(s_out)))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_axpy_clamp_dev: vectors must be 16-byte aligned");
    if (s_out && (s_out == p || s_out == out || s_out == d))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_axpy_clamp_dev: s_out must not alias p, d or out");
    hipError_t e = tvam_launch_axpy_clamp(n, p, 0.0f, d, lo, out, (hipStream_t)stream, alpha, s_out);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "axpy launch");
}

extern "C" int tvam_lbfgs_armijo(int32_t nprobe, double alpha0, const double* probes, const double* loss_dev,
                                 double loss_host, double loss_div, const double* gdz, double c1, float* alpha,
                                 double* report, void* stream) {
    if (!probes || !gdz || !alpha) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (nprobe < 1 || nprobe > 64) return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_armijo: 1 <= nprobe <= 64");
    if (!(alpha0 > 0.0) || !(loss_div > 0.0))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_lbfgs_armijo: alpha0 and loss_div must be positive");
    hipError_t e = tvam_launch_armijo(nprobe, alpha0, probes, loss_dev, loss_host, loss_div, gdz, c1, alpha, report,
                                      (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "armijo launch");
}

// First-order optimiser updates.  The hyper-parameters arrive as doubles and are rounded here:
// lr, beta and epsilon to fp32, 1 - beta in double and then to fp32.
extern "C" int tvam_sgd_step(uint64_t n, float* p, const float* g, float* s, double lr, double momentum, int32_t mask,
                             float lo, void* stream) {
    if (!p || !g) return tvam_fail(TVAM_ERR_INVALID, "tvam_sgd_step: null argument");
    if (!s && momentum != 0.0) return tvam_fail(TVAM_ERR_INVALID, "tvam_sgd_step: momentum needs the state vector s");
    if (n == 0) return 0;
    hipError_t e = tvam_launch_sgd_step(n, p, g, s, (float)lr, (float)momentum, mask != 0, lo, (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "sgd step launch");
}

extern "C" int tvam_adam_step(uint64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta_1,
                              double beta_2, double epsilon, int32_t mask, float lo, void* stream) {
    if (!p || !g || !m || !v) return tvam_fail(TVAM_ERR_INVALID, "tvam_adam_step: null argument");
    if (n == 0) return 0;
    hipError_t e = tvam_launch_adam_step(n, p, g, m, v, (float)lr_t, (float)beta_1, (float)(1.0 - beta_1),
                                         (float)beta_2, (float)(1.0 - beta_2), (float)epsilon, mask != 0, lo,
                                         (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "adam step launch");
}

extern "C" int tvam_adam_moments(uint64_t n, const float* g, float* m, float* v, double beta_1, double beta_2,
                                 int32_t mask, double* work, double* S, void* stream) {
    if (!g || !m || !v || !work || !S) return tvam_fail(TVAM_ERR_INVALID, "tvam_adam_moments: null argument");
    if (n == 0) return 0;
    hipError_t e = tvam_launch_adam_moments(n, g, m, v, (float)beta_1, (float)(1.0 - beta_1), (float)beta_2,
                                            (float)(1.0 - beta_2), mask != 0, work, S, (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "adam moments launch");
}

extern "C" int tvam_adam_apply(uint64_t n, float* p, const float* g, const float* m, const double* S,
                               const double* count, double lr_t, double epsilon, int32_t mask, float lo,
                               void* stream) {
    if (!p || !m || !S || !count || (mask && !g)) return tvam_fail(TVAM_ERR_INVALID, "tvam_adam_apply: null argument");
    if (n == 0) return 0;
    hipError_t e = tvam_launch_adam_apply(n, p, g, m, S, count, (float)lr_t, (float)epsilon, mask != 0, lo,
                                          (hipStream_t)stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "adam apply launch");
}

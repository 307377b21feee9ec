// tvam_loss.hip — the fused losses beside tvam_loss_threshold* (tvam_kernels.hip): L2Loss over a
// one-channel target, and ThresholdedLoss / L2Loss over a surface-aware (two-channel) film
// (loss.py:28-59, :62-79, :82-132).  One pass gives the f64 value and dL/ddose, a second kind of pass
// the value at up to TVAM_MAX_PROBES step sizes (the Armijo probes of lbfgs.py:255-268).
//
// Per voxel, fp32, one rounding per written operation (no contraction: the gradient is held bit for
// bit to this order by tests/loss_model.py), x = fmaf(alpha, ddose, dose) when ddose is given:
//
//   L2, one channel          d = x - t;  element d d;  gradient (2 d) scale
//   two channels             x0, x1 and t0 = V_in, t1 = V_out interleaved per voxel;
//                            s = t0 + t1, w_in = t0 / s, w_out = t1 / s (IEEE divisions; s = 0 is
//                            outside the contract, 0 / 0 as in the reference);
//                            element w_in e_in + w_out e_out;
//                            gradient (w_in g_in) scale to channel 0, (w_out g_out) scale to channel 1
//     threshold              e_in = w_object relu(tu - x0)^K + w_limit relu(x0 - 1)^K,
//                            e_out = w_void relu(x1 - tl)^K, g_in / g_out as tvam_loss_grad_elem
//     L2                     e_in = (x0 - 1)^2, e_out = x1^2, g_in = 2 (x0 - 1), g_out = 2 x1
//
// Kernels: 256 threads, grid-stride, at most 2048 workgroups.  A float4 holds four one-channel
// voxels or two whole two-channel voxels; it is used when every pointer is 16-byte aligned (an
// 8-byte aligned two-channel array would split voxel pairs across float4s: it takes the scalar
// path, like a 4-byte aligned one), the tail and the unaligned case run one voxel per trip.  The
// reduction counts voxels: per-thread f64 sum, wave shuffle, red[4], one f64 atomicAdd(out, s scale)
// per workgroup.  Pure HBM streams: 12 B (one channel) / 24 B (two) per voxel with the gradient,
// 8 B / 16 B without; the probes read 8 B / 24 B.
#include "tvam_plan.h"

#pragma clang fp contract(off)

#define TVAM_LW_BLOCK 256
#define TVAM_LW_GRID 2048
#define TVAM_LW_THRESHOLD 0  // tvam.h: TVAM_LOSS_KIND_THRESHOLD
#define TVAM_LW_L2 1         // tvam.h: TVAM_LOSS_KIND_L2

namespace {

struct LwParams {
    int K;
    float tl, tu, w_object, w_void, w_limit;
};

__device__ __forceinline__ float lw_relu(float z) { return z > 0.0f ? z : 0.0f; }

// e_in, e_out of one two-channel voxel (and g_in, g_out when GRAD)
template <int KIND, int KC, bool GRAD>
__device__ __forceinline__ void lw_inout(float x0, float x1, const LwParams& p, float& e_in, float& e_out, float& g_in,
                                         float& g_out) {
    if (KIND == TVAM_LW_THRESHOLD) {
        const int K = KC ? KC : p.K;
        const float zo = p.tu - x0, zl = x0 - 1.0f, zv = x1 - p.tl;
        const float ro = lw_relu(zo), rl = lw_relu(zl), rv = lw_relu(zv);
        e_in = p.w_object * tvam_powi(ro, K) + p.w_limit * tvam_powi(rl, K);
        e_out = p.w_void * tvam_powi(rv, K);
        if (GRAD) {
            g_in = (zo > 0.0f ? -p.w_object * (float)K * tvam_powi(ro, K - 1) : 0.0f) +
                   (zl > 0.0f ? p.w_limit * (float)K * tvam_powi(rl, K - 1) : 0.0f);
            g_out = zv > 0.0f ? p.w_void * (float)K * tvam_powi(rv, K - 1) : 0.0f;
        }
    } else {
        const float d0 = x0 - 1.0f;
        e_in = d0 * d0;
        e_out = x1 * x1;
        if (GRAD) {
            g_in = 2.0f * d0;
            g_out = 2.0f * x1;
        }
    }
}

// one two-channel voxel: the element; g0, g1 = the gradient before scale
template <int KIND, int KC>
__device__ __forceinline__ float lw_surface_grad(float x0, float x1, float t0, float t1, const LwParams& p, float& g0,
                                                 float& g1) {
    const float s = t0 + t1;
    const float w_in = t0 / s, w_out = t1 / s;
    float e_in, e_out, g_in, g_out;
    lw_inout<KIND, KC, true>(x0, x1, p, e_in, e_out, g_in, g_out);
    g0 = w_in * g_in;
    g1 = w_out * g_out;
    return w_in * e_in + w_out * e_out;
}

template <int KIND, int KC>
__device__ __forceinline__ float lw_surface_elem(float x0, float x1, float w_in, float w_out, const LwParams& p) {
    float e_in, e_out, g_in, g_out;
    lw_inout<KIND, KC, false>(x0, x1, p, e_in, e_out, g_in, g_out);
    return w_in * e_in + w_out * e_out;
}

// sum of acc over the workgroup, out += sum * scale (one atomic per workgroup)
__device__ __forceinline__ void lw_reduce(double acc, double* red, float scale, double* __restrict__ out) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < TVAM_LW_BLOCK / 64; ++w) s += red[w];
        atomicAdd(out, s * (double)scale);
    }
}

template <int NA_MAX>
__device__ __forceinline__ void lw_reduce_probes(const double (&acc)[NA_MAX], double (*red)[TVAM_LW_BLOCK / 64], int na,
                                                 float scale, double* __restrict__ out) {
#pragma unroll
    for (int j = 0; j < NA_MAX; ++j) {
        double v = acc[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[j][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < na) {
        double s = 0.0;
        for (int w = 0; w < TVAM_LW_BLOCK / 64; ++w) s += red[threadIdx.x][w];
        atomicAdd(out + threadIdx.x, s * (double)scale);
    }
}

// ---------------------------------------------------------------------------
// L2, one channel.  n4: voxels / 4 when dose, ddose, target and grad allow float4 accesses, else 0
__global__ __launch_bounds__(TVAM_LW_BLOCK) void lw_l2_kernel(const float* __restrict__ dose,
                                                              const float* __restrict__ ddose, float alpha,
                                                              const float* __restrict__ target, uint64_t n, uint64_t n4,
                                                              float scale, double* __restrict__ out,
                                                              float* __restrict__ grad) {
    __shared__ double red[TVAM_LW_BLOCK / 64];
    double acc = 0.0;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = tid; t < n4; t += stride) {
        float4 x = reinterpret_cast<const float4*>(dose)[t];
        if (ddose) {  // vol + alpha * dvol (lbfgs.py:258)
            const float4 dx = reinterpret_cast<const float4*>(ddose)[t];
            x = make_float4(fmaf(alpha, dx.x, x.x), fmaf(alpha, dx.y, x.y), fmaf(alpha, dx.z, x.z), fmaf(alpha, dx.w, x.w));
        }
        const float4 tg = reinterpret_cast<const float4*>(target)[t];
        const float4 d = make_float4(x.x - tg.x, x.y - tg.y, x.z - tg.z, x.w - tg.w);
        acc += (double)(d.x * d.x);
        acc += (double)(d.y * d.y);
        acc += (double)(d.z * d.z);
        acc += (double)(d.w * d.w);
        if (grad)
            reinterpret_cast<float4*>(grad)[t] =
                make_float4((2.0f * d.x) * scale, (2.0f * d.y) * scale, (2.0f * d.z) * scale, (2.0f * d.w) * scale);
    }
    for (uint64_t i = 4 * n4 + tid; i < n; i += stride) {
        float x = dose[i];
        if (ddose) x = fmaf(alpha, ddose[i], x);
        const float d = x - target[i];
        acc += (double)(d * d);
        if (grad) grad[i] = (2.0f * d) * scale;
    }
    lw_reduce(acc, red, scale, out);
}

__global__ __launch_bounds__(TVAM_LW_BLOCK) void lw_l2_probes_kernel(const float* __restrict__ dose,
                                                                     const float* __restrict__ ddose, TvamProbeAlphas al,
                                                                     int na, const float* __restrict__ target, uint64_t n,
                                                                     uint64_t n4, float scale, double* __restrict__ out) {
    __shared__ double red[TVAM_MAX_PROBES][TVAM_LW_BLOCK / 64];
    double acc[TVAM_MAX_PROBES];
#pragma unroll
    for (int j = 0; j < TVAM_MAX_PROBES; ++j) acc[j] = 0.0;
    auto elem = [&](float x0, float dx, float t) {
#pragma unroll
        for (int j = 0; j < TVAM_MAX_PROBES; ++j)
            if (j < na) {
                const float d = fmaf(al.a[j], dx, x0) - t;
                acc[j] += (double)(d * d);
            }
    };
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = tid; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(dose)[i], dx = reinterpret_cast<const float4*>(ddose)[i];
        const float4 tg = reinterpret_cast<const float4*>(target)[i];
        elem(x.x, dx.x, tg.x);
        elem(x.y, dx.y, tg.y);
        elem(x.z, dx.z, tg.z);
        elem(x.w, dx.w, tg.w);
    }
    for (uint64_t i = 4 * n4 + tid; i < n; i += stride) elem(dose[i], ddose[i], target[i]);
    lw_reduce_probes(acc, red, na, scale, out);
}

// ---------------------------------------------------------------------------
// Two channels.  n: voxels; n2: voxels / 2 (float4s of two whole voxels) when dose, ddose, target and
// grad are 16-byte aligned, else 0
template <int KIND, int KC>
__global__ __launch_bounds__(TVAM_LW_BLOCK) void lw_surface_kernel(const float* __restrict__ dose,
                                                                   const float* __restrict__ ddose, float alpha,
                                                                   const float* __restrict__ target, uint64_t n,
                                                                   uint64_t n2, LwParams p, float scale,
                                                                   double* __restrict__ out, float* __restrict__ grad) {
    __shared__ double red[TVAM_LW_BLOCK / 64];
    double acc = 0.0;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = tid; t < n2; t += stride) {
        float4 x = reinterpret_cast<const float4*>(dose)[t];
        if (ddose) {
            const float4 dx = reinterpret_cast<const float4*>(ddose)[t];
            x = make_float4(fmaf(alpha, dx.x, x.x), fmaf(alpha, dx.y, x.y), fmaf(alpha, dx.z, x.z), fmaf(alpha, dx.w, x.w));
        }
        const float4 tg = reinterpret_cast<const float4*>(target)[t];
        float4 g;
        acc += (double)lw_surface_grad<KIND, KC>(x.x, x.y, tg.x, tg.y, p, g.x, g.y);
        acc += (double)lw_surface_grad<KIND, KC>(x.z, x.w, tg.z, tg.w, p, g.z, g.w);
        if (grad)
            reinterpret_cast<float4*>(grad)[t] = make_float4(g.x * scale, g.y * scale, g.z * scale, g.w * scale);
    }
    for (uint64_t i = 2 * n2 + tid; i < n; i += stride) {
        float x0 = dose[2 * i], x1 = dose[2 * i + 1];
        if (ddose) {
            x0 = fmaf(alpha, ddose[2 * i], x0);
            x1 = fmaf(alpha, ddose[2 * i + 1], x1);
        }
        float g0, g1;
        acc += (double)lw_surface_grad<KIND, KC>(x0, x1, target[2 * i], target[2 * i + 1], p, g0, g1);
        if (grad) {
            grad[2 * i] = g0 * scale;
            grad[2 * i + 1] = g1 * scale;
        }
    }
    lw_reduce(acc, red, scale, out);
}

template <int KIND, int KC>
__global__ __launch_bounds__(TVAM_LW_BLOCK) void lw_surface_probes_kernel(const float* __restrict__ dose,
                                                                          const float* __restrict__ ddose,
                                                                          TvamProbeAlphas al, int na,
                                                                          const float* __restrict__ target, uint64_t n,
                                                                          uint64_t n2, LwParams p, float scale,
                                                                          double* __restrict__ out) {
    __shared__ double red[TVAM_MAX_PROBES][TVAM_LW_BLOCK / 64];
    double acc[TVAM_MAX_PROBES];
#pragma unroll
    for (int j = 0; j < TVAM_MAX_PROBES; ++j) acc[j] = 0.0;
    auto voxel = [&](float x0, float x1, float dx0, float dx1, float t0, float t1) {
        const float s = t0 + t1;
        const float w_in = t0 / s, w_out = t1 / s;  // the value kernel's weights, once for every step size
#pragma unroll
        for (int j = 0; j < TVAM_MAX_PROBES; ++j)
            if (j < na)
                acc[j] += (double)lw_surface_elem<KIND, KC>(fmaf(al.a[j], dx0, x0), fmaf(al.a[j], dx1, x1), w_in, w_out, p);
    };
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = tid; i < n2; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(dose)[i], dx = reinterpret_cast<const float4*>(ddose)[i];
        const float4 tg = reinterpret_cast<const float4*>(target)[i];
        voxel(x.x, x.y, dx.x, dx.y, tg.x, tg.y);
        voxel(x.z, x.w, dx.z, dx.w, tg.z, tg.w);
    }
    for (uint64_t i = 2 * n2 + tid; i < n; i += stride)
        voxel(dose[2 * i], dose[2 * i + 1], ddose[2 * i], ddose[2 * i + 1], target[2 * i], target[2 * i + 1]);
    lw_reduce_probes(acc, red, na, scale, out);
}

bool lw_al16(const void* a, const void* b, const void* c, const void* d) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// workgroups for `work` grid-stride trips
unsigned lw_grid(uint64_t work) {
    const uint64_t g = (work + TVAM_LW_BLOCK - 1) / TVAM_LW_BLOCK;
    return g > TVAM_LW_GRID ? TVAM_LW_GRID : (g == 0 ? 1u : (unsigned)g);
}

// KC of a two-channel launch: K = 1..4 as a compile-time constant, else 0 (K at run time); the L2 kind has no K
#define TVAM_LW_DISPATCH(LAUNCH)                        \
    if (kind == TVAM_LW_L2) {                           \
        LAUNCH(TVAM_LW_L2, 0);                          \
    } else {                                            \
        switch (p.K) {                                  \
            case 1: LAUNCH(TVAM_LW_THRESHOLD, 1); break; \
            case 2: LAUNCH(TVAM_LW_THRESHOLD, 2); break; \
            case 3: LAUNCH(TVAM_LW_THRESHOLD, 3); break; \
            case 4: LAUNCH(TVAM_LW_THRESHOLD, 4); break; \
            default: LAUNCH(TVAM_LW_THRESHOLD, 0); break; \
        }                                               \
    }

// the argument checks the value and the probe entries share; 0: fine
int lw_check_surface(const char* fn, int32_t kind, int32_t K) {
    if (kind != TVAM_LW_THRESHOLD && kind != TVAM_LW_L2)
        return tvam_fail(TVAM_ERR_INVALID, std::string(fn) + ": unknown kind " + std::to_string(kind) +
                                               " (0: threshold, 1: l2)");
    if (kind == TVAM_LW_THRESHOLD && (K < 1 || K > 16))
        return tvam_fail(TVAM_ERR_INVALID, std::string(fn) + ": integer K in [1, 16] required (got " + std::to_string(K) + ")");
    return 0;
}

int lw_check_ptrs(const char* fn, const void* dose, const void* target, const void* out) {
    const char* which = !dose ? "dose" : !target ? "target" : !out ? "out" : nullptr;
    return which ? tvam_fail(TVAM_ERR_INVALID, std::string(fn) + ": null " + which) : 0;
}

int lw_check_probes(const char* fn, const void* ddose, const void* alphas, int32_t n_alpha) {
    if (!ddose || !alphas) return tvam_fail(TVAM_ERR_INVALID, std::string(fn) + ": null " + (!ddose ? "ddose" : "alphas"));
    if (n_alpha < 1 || n_alpha > TVAM_MAX_PROBES)
        return tvam_fail(TVAM_ERR_INVALID, std::string(fn) + ": 1 <= n_alpha <= 8 (got " + std::to_string(n_alpha) + ")");
    return 0;
}

}  // namespace

// The extern "C" boundary of these kernels (include/tvam.h).
extern "C" int tvam_loss_square(const float* dose, const float* ddose, float alpha, const float* target, uint64_t n,
                                float scale, double* out, float* grad, void* stream) {
    if (int rc = lw_check_ptrs("tvam_loss_square", dose, target, out)) return rc;
    if (n == 0) return 0;
    const uint64_t n4 = lw_al16(dose, ddose, target, grad) ? n / 4 : 0;
    hipLaunchKernelGGL(lw_l2_kernel, dim3(lw_grid(n4 ? n4 : n)), dim3(TVAM_LW_BLOCK), 0, (hipStream_t)stream, dose, ddose,
                       alpha, target, n, n4, scale, out, grad);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "tvam_loss_square: launch");
}

extern "C" int tvam_loss_square_probes(const float* dose, const float* ddose, const float* alphas, int32_t n_alpha,
                                       const float* target, uint64_t n, float scale, double* out, void* stream) {
    if (int rc = lw_check_ptrs("tvam_loss_square_probes", dose, target, out)) return rc;
    if (int rc = lw_check_probes("tvam_loss_square_probes", ddose, alphas, n_alpha)) return rc;
    if (n == 0) return 0;
    TvamProbeAlphas al{};
    for (int j = 0; j < n_alpha; ++j) al.a[j] = alphas[j];
    const uint64_t n4 = lw_al16(dose, ddose, target, nullptr) ? n / 4 : 0;
    hipLaunchKernelGGL(lw_l2_probes_kernel, dim3(lw_grid(n4 ? n4 : n)), dim3(TVAM_LW_BLOCK), 0, (hipStream_t)stream, dose,
                       ddose, al, (int)n_alpha, target, n, n4, scale, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "tvam_loss_square_probes: launch");
}

extern "C" int tvam_loss_surface(int32_t kind, const float* dose, const float* ddose, float alpha, const float* target,
                                 uint64_t n_vox, int32_t K, float tl, float tu, float w_object, float w_void,
                                 float w_limit, float scale, double* out, float* grad, void* stream) {
    if (int rc = lw_check_ptrs("tvam_loss_surface", dose, target, out)) return rc;
    if (int rc = lw_check_surface("tvam_loss_surface", kind, K)) return rc;
    if (n_vox == 0) return 0;
    const LwParams p{K, tl, tu, w_object, w_void, w_limit};
    const uint64_t n2 = lw_al16(dose, ddose, target, grad) ? n_vox / 2 : 0;
    const unsigned g = lw_grid(n2 ? n2 : n_vox);
#define TVAM_LW_VALUE(KIND, KC)                                                                                      \
    hipLaunchKernelGGL((lw_surface_kernel<KIND, KC>), dim3(g), dim3(TVAM_LW_BLOCK), 0, (hipStream_t)stream, dose, ddose, \
                       alpha, target, n_vox, n2, p, scale, out, grad)
    TVAM_LW_DISPATCH(TVAM_LW_VALUE)
#undef TVAM_LW_VALUE
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "tvam_loss_surface: launch");
}

extern "C" int tvam_loss_surface_probes(int32_t kind, const float* dose, const float* ddose, const float* alphas,
                                        int32_t n_alpha, const float* target, uint64_t n_vox, int32_t K, float tl,
                                        float tu, float w_object, float w_void, float w_limit, float scale, double* out,
                                        void* stream) {
    if (int rc = lw_check_ptrs("tvam_loss_surface_probes", dose, target, out)) return rc;
    if (int rc = lw_check_probes("tvam_loss_surface_probes", ddose, alphas, n_alpha)) return rc;
    if (int rc = lw_check_surface("tvam_loss_surface_probes", kind, K)) return rc;
    if (n_vox == 0) return 0;
    const LwParams p{K, tl, tu, w_object, w_void, w_limit};
    TvamProbeAlphas al{};
    for (int j = 0; j < n_alpha; ++j) al.a[j] = alphas[j];
    const uint64_t n2 = lw_al16(dose, ddose, target, nullptr) ? n_vox / 2 : 0;
    const unsigned g = lw_grid(n2 ? n2 : n_vox);
#define TVAM_LW_PROBES(KIND, KC)                                                                                       \
    hipLaunchKernelGGL((lw_surface_probes_kernel<KIND, KC>), dim3(g), dim3(TVAM_LW_BLOCK), 0, (hipStream_t)stream, dose, \
                       ddose, al, (int)n_alpha, target, n_vox, n2, p, scale, out)
    TVAM_LW_DISPATCH(TVAM_LW_PROBES)
#undef TVAM_LW_PROBES
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "tvam_loss_surface_probes: launch");
}

// Extinction derivatives: d dose / d sigma_t of a non-scattering medium, the
// reference's g_st (sensor.py:377-440, volume.py:274-280) in forward and reverse mode.
//
//   tvam_dsigma_kernel<FWD>  the tangent film T[v] = d dose[v] / d sigma_t: the forward render with
//                            the visit weight w'(T0, dt) of tvam_dsigma.h, global float atomics
//   tvam_dsigma_kernel<ADJ>  the scalar g = sum_v G[v] T[v]: per ray a gather of w' G inv_vol in
//                            fp32, the rays summed in fp64 by wave shuffles, then the workgroup's 4
//                            waves through LDS; one partial per workgroup, no atomics
//   tvam_dsigma_sum_kernel   one workgroup: the partials in a fixed order into the caller's double
// One thread per (ray, sample).  The segment is the one the plan's own forward marches: SEG =
// DS_PATH for the collimated plans of tvam_plan_create (tvam_path_first_segment: index-matched,
// cylindrical or square, occluders), else the ConeMesh of a 3-D ray plan (cn_ray_at).  The march is
// cn_dda's own stepping (cn_dda_steps), so T0 is the DDA's t, measured from the segment origin o2.
#include "tvam_plan.h"

#include "tvam_cone_ray.h"
#include "tvam_dsigma.h"

namespace {

enum { DS_PATH = 4 };  // SEG beyond the ConeMesh values: the planar first segment of tvam_path.h

extern __shared__ float4 ds_mesh_lds[];  // CN_MESH_LDS: the workgroup's copy of the meshes

template <int MODE, int SEG>
__global__ __launch_bounds__(256) void tvam_dsigma_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ pat,
                                                          const int32_t* __restrict__ idxmap,
                                                          const float* __restrict__ gin, float* __restrict__ tangent,
                                                          double* __restrict__ partials) {
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * (int)tp.spp;
    const bool f32 = tvam_path_fits32(n);
    constexpr int MESH = SEG == DS_PATH ? (int)CN_NO_MESH : SEG;
    const TvamMeshView mesh = cn_mesh_view<MESH>(k, ds_mesh_lds);
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        // FWD: em = pattern * wscale * inv_vol; ADJ: pattern * wscale (inv_vol goes with the gathered gradient)
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_FWD>(k, pat, idxmap, ix.local, k.wscale, MODE == TVAM_MODE_FWD ? k.inv_vol : 1.0f,
                                           em, act))
            continue;
        tvam_path_pixel(k, f32, ix);
        const uint64_t stream = tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp);
        ConeRay r;
        if constexpr (SEG == DS_PATH) {
            TvamPcg rng;
            const TvamPathDraws dr = tvam_path_draws<false, false>(k, tp, ix.al, stream, rng);
            TvamPathSeg s;
            if (!tvam_path_first_segment(k, ix, dr, s)) continue;
            r.o2[0] = s.o2x, r.o2[1] = s.o2y, r.o2[2] = s.oz;
            r.d2[0] = s.d2x, r.d2[1] = s.d2y, r.d2[2] = 0.0f;
            r.maxt = s.maxt;
            r.att = s.wgt;
        } else {
            if (!cn_ray_at<MESH>(k, tp, ix.al, ix.colc, ix.rowc, stream, r, &mesh)) continue;
            if (SEG == CN_NO_MESH) {  // (index matched: the ray's own direction, no interface)
                r.d2[0] = r.d[0], r.d2[1] = r.d[1], r.d2[2] = r.d[2];
                r.att = 1.0f;
            }
        }
        const float emw = em * r.att;
        float acc = 0.0f;
        cn_dda_steps(k, r.o2, r.d2, r.maxt, [&](int64_t idx, float t, float dt) {
            const float w = tvam_dsig_weight(k.sig_t, t, dt);
            if (MODE == TVAM_MODE_FWD) atomicAdd(&tangent[idx], emw * w);
            else acc = fmaf(w, gin[idx] * k.inv_vol, acc);
        });
        if (MODE == TVAM_MODE_ADJ) sum += (double)emw * (double)acc;
    }
    if (MODE == TVAM_MODE_ADJ) {
        __shared__ double s_wave[4];
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) partials[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
    }
}

// The n partials into out[0]: thread t sums partials t, t + 256, ... in that order, thread 0 the 256
// sums in index order.
__global__ __launch_bounds__(256) void tvam_dsigma_sum_kernel(const double* __restrict__ partials, int n,
                                                              double* __restrict__ out) {
    __shared__ double s_part[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    s_part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double g = 0.0;
        for (int i = 0; i < 256; ++i) g += s_part[i];
        out[0] = g;
    }
}

template <int SEG>
void ds_launch(int mode, const TvamConsts& k, const TvamTiles& t, const float* pat, const int32_t* idxmap,
               const float* gin, float* tangent, double* partials, unsigned grid, hipStream_t stream) {
    const dim3 g(grid), b(256);
    const size_t lds = SEG == CN_MESH_LDS ? cn_lds(k) : 0;
    if (mode == TVAM_MODE_FWD)
        hipLaunchKernelGGL((tvam_dsigma_kernel<TVAM_MODE_FWD, SEG>), g, b, lds, stream, k, t, pat, idxmap, gin, tangent,
                           partials);
    else
        hipLaunchKernelGGL((tvam_dsigma_kernel<TVAM_MODE_ADJ, SEG>), g, b, lds, stream, k, t, pat, idxmap, gin, tangent,
                           partials);
}

}  // namespace

unsigned tvam_dsigma_grid(int64_t n_rays) { return tvam_grid_1d(n_rays, 2048); }

hipError_t tvam_launch_partial_sum(const double* partials, int n, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(tvam_dsigma_sum_kernel, dim3(1), dim3(256), 0, stream, partials, n, out);
    return hipGetLastError();
}

hipError_t tvam_launch_dsigma(int mode, bool cone, const TvamConsts& k, const TvamTiles& t, const float* pat,
                              const int32_t* idxmap, const float* gin, float* tangent, double* partials,
                              double* g_sigma, hipStream_t stream) {
    const unsigned grid = tvam_dsigma_grid((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp);
    if (!cone) {
        ds_launch<DS_PATH>(mode, k, t, pat, idxmap, gin, tangent, partials, grid, stream);
    } else {
        switch (cn_mesh_mode(k)) {
            case CN_NO_MESH: ds_launch<CN_NO_MESH>(mode, k, t, pat, idxmap, gin, tangent, partials, grid, stream); break;
            case CN_MESH_LDS: ds_launch<CN_MESH_LDS>(mode, k, t, pat, idxmap, gin, tangent, partials, grid, stream); break;
            case CN_GLASS: ds_launch<CN_GLASS>(mode, k, t, pat, idxmap, gin, tangent, partials, grid, stream); break;
            default: ds_launch<CN_MESH_GLOBAL>(mode, k, t, pat, idxmap, gin, tangent, partials, grid, stream);
        }
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && mode == TVAM_MODE_ADJ) e = tvam_launch_partial_sum(partials, (int)grid, g_sigma, stream);
    return e;
}

extern "C" int tvam_dsigma_weights(float sigma_t, const float* T0, const float* dt, int64_t n, float* w) {
    if (n < 0 || (n > 0 && (!T0 || !dt || !w))) return tvam_fail(TVAM_ERR_INVALID, "tvam_dsigma_weights: null argument");
    for (int64_t i = 0; i < n; ++i) w[i] = tvam_dsig_weight(sigma_t, T0[i], dt[i]);
    return 0;
}

// Corner filter ('filter_corner'; integrators/filter_corner.py:17-66, optimize.py:166-185): one
// thread per active entry sends the ray through its pixel's centre (regular sampling, spp 1,
// seed 0, no time sample, whatever the plan's own sampling is), finds the first surface it meets
// (tvam_firsthit.h) and keeps the pixel unless the ray misses the scene or lands within `radius`
// of a vial corner.  The telecentric / lens projectors still take their aperture draw from the
// sampler stream of the entry's position in the whole active set (cn_ray_at, tvam_cone_ray.h:
// the ray tvam_plan_rays exports for such a plan); the collimated projector draws nothing.
// Setup-time work: no LDS, no atomics; one 4-byte and one 16-byte store per entry.
#include "tvam_cone_ray.h"
#include "tvam_firsthit.h"

namespace {

// active == nullptr: entry i is dense shard entry i ([angle][crop row][crop col]; stream = the
// global dense index).  Else active[i] is a full-DMD index angle * H * W + row * W + col (any
// pixel of the DMD, the crop does not restrict it) and the stream is k.stream_base + i; an entry
// whose angle lies outside the plan's shard is dropped (keep 0, t = -1).
// The caller passes k with regular = 1, sample_time = 0 and tp with seed = 0, spp = 1.
template <int PROJ>
__global__ __launch_bounds__(256) void tvam_corner_kernel(TvamConsts k, TvamTiles tp,
                                                          const uint32_t* __restrict__ active, int64_t n, float dist,
                                                          float radius, float* __restrict__ keep,
                                                          float4* __restrict__ hits) {
    const uint32_t hw = (uint32_t)k.res_x * (uint32_t)k.res_y;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int al, colc, rowc;
        uint64_t stream;
        if (active) {
            const uint32_t p = active[i];
            const uint32_t a = p / hw, rem = p - a * hw;
            const uint32_t row = rem / (uint32_t)k.res_x, col = rem - row * (uint32_t)k.res_x;
            al = (int)a - k.a0;
            rowc = (int)row - k.crop_off_y;
            colc = (int)col - k.crop_off_x;
            stream = (uint64_t)(k.stream_base + i);
        } else {
            tvam_path_pixel(k, i, tvam_path_fits32(n), al, rowc, colc);
            stream = (uint64_t)(i + k.shard_base);
        }
        TvamFirstHit h;
        h.t = -1.0f;
        h.px = h.py = h.pz = 0.0f;
        if (al >= 0 && al < tp.n_shard) {
            float ox, oy, oz, dx, dy, dz;
            if (PROJ == TVAM_PROJECTOR_COLLIMATED) {
                TvamPcg rng;  // (k.regular: nothing is drawn)
                const TvamPathDraws dr = tvam_path_draws<false, false>(k, tp, al, stream, rng);
                tvam_path_ray(k, colc, rowc, dr, ox, oy, oz, dx, dy);
                dz = 0.0f;
            } else {
                ConeRay r;
                (void)cn_ray_at(k, tp, al, colc, rowc, stream, r);
                ox = r.o[0];
                oy = r.o[1];
                oz = r.o[2];
                dx = r.d[0];
                dy = r.d[1];
                dz = r.d[2];
            }
            h = tvam_first_hit(k, ox, oy, oz, dx, dy, dz);
        }
        keep[i] = tvam_corner_keep(h, dist, radius) ? 1.0f : 0.0f;
        if (hits) hits[i] = make_float4(h.px, h.py, h.pz, h.t);
    }
}

}  // namespace

hipError_t tvam_launch_corner(const TvamConsts& k, const TvamTiles& t, const uint32_t* active, int64_t n, float dist,
                              float radius, float* keep, float* hits, hipStream_t stream) {
    const dim3 grid(tvam_grid_1d(n)), block(256);
    float4* h4 = reinterpret_cast<float4*>(hits);
    switch (k.proj_type) {
        case TVAM_PROJECTOR_COLLIMATED:
            hipLaunchKernelGGL(tvam_corner_kernel<TVAM_PROJECTOR_COLLIMATED>, grid, block, 0, stream, k, t, active, n,
                               dist, radius, keep, h4);
            break;
        case TVAM_PROJECTOR_TELECENTRIC:
            hipLaunchKernelGGL(tvam_corner_kernel<TVAM_PROJECTOR_TELECENTRIC>, grid, block, 0, stream, k, t, active, n,
                               dist, radius, keep, h4);
            break;
        default:
            hipLaunchKernelGGL(tvam_corner_kernel<TVAM_PROJECTOR_LENS>, grid, block, 0, stream, k, t, active, n, dist,
                               radius, keep, h4);
    }
    return hipGetLastError();
}

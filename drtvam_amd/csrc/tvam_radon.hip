// Radon filter (integrators/radon.py:47-106, optimize.py:143-163):
// one thread per DMD pixel of the plan's shard, summing its samples'
// weighted target-and-medium absorption (tvam_radon_ray).  The optimiser
// keeps the pixels with radon > 0 ('filter_radon').  Setup-time work: the
// target mesh is tested triangle by triangle (no BVH).
#include "tvam_path.h"

namespace {

__global__ __launch_bounds__(256) void tvam_radon_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ tgt,
                                                         int ntgt, int max_depth, float wray,
                                                         float* __restrict__ radon) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x;
    for (int64_t local = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; local < n;
         local += (int64_t)gridDim.x * blockDim.x) {
        int al, rowc, colc;
        tvam_path_pixel(k, local, false, al, rowc, colc);  // (64-bit: the second decode costs the 7th wave/SIMD)
        float acc = 0.0f;
        for (int smp = 0; smp < spp; ++smp) {
            TvamPcg rng;  // the dense set's stream (no idxmap)
            const TvamPathDraws dr = tvam_path_draws<false, false>(k, tp, al, tvam_stream(k, nullptr, local, tp.spp, smp), rng);
            float ox, oy, oz, dx, dy;
            tvam_path_ray(k, colc, rowc, dr, ox, oy, oz, dx, dy);
            acc += tvam_radon_ray(k, tgt, ntgt, max_depth, ox, oy, oz, dx, dy);
        }
        radon[local] = wray * acc;
    }
}

}  // namespace

hipError_t tvam_launch_radon(const TvamConsts& k, const TvamTiles& t, const float* tgt, int ntgt, int max_depth,
                             float wray, float* radon, hipStream_t stream) {
    const int64_t n = (int64_t)t.n_shard * k.crop_y * k.crop_x;
    hipLaunchKernelGGL(tvam_radon_kernel, dim3(tvam_grid_1d(n)), dim3(256), 0, stream, k, t, tgt, ntgt, max_depth, wray,
                       radon);
    return hipGetLastError();
}

// Telecentric and lens projectors (projector.py:199-296): projector rays with a finite
// etendue.  Every ray starts on the aperture disk and passes its pixel's point of the focus
// plane, so its first medium segment is a 3-D ray: it leaves its z-slice, and none of the
// planar / tile kernels (d.z = 0) applies.  The pieces are the scattered segments' own
// (tvam_seg3d.h, tvam_bricks.h): the open tube's 3-D hit, the 3-D DDA and the brick bins.
//
//   cn_ray            sampler draws (common.py:92-108: position next_2d if jittered, time
//                     next_1d under sample_time, aperture next_2d), get_ray of the plan's
//                     projector, CircularMotion's to_world (motion.py:26-36), the medium
//                     segment behind the index-matched vial (volume.py:191-216, :268)
//   tvam_cone_kernel  one thread per (ray, sample) marching cn_dda (the oracle's or_dda op for
//                     op): forward with global float atomics, adjoint as a gather (a plain
//                     store per active entry when spp == 1), visit count
//   tvam_cone_emit_kernel   one brick-bin record per ray for tvam_scatter_binned (the binned
//                     forward: bin fill, sort, tvam_bin_march_kernel and the bin cache)
//   tvam_cone_export_kernel the rays themselves (tvam_plan_rays)
//
// A 'custom' vial (mesh interfaces, tvam_mesh.h) runs the same kernels for all three projectors,
// instantiated with MESH: the segment comes from cn_segment_mesh (closest hits through the
// hierarchy, from global memory or from the workgroup's LDS copy), the march takes the refracted
// direction d2 and the weight em * att.  The index-matched instantiations (MESH = CN_NO_MESH) read
// d and em as before.  A traced 'cylindrical' / 'square' vial (tvam_plan_create_traced) is one more
// instantiation, CN_GLASS: the segment comes from tvam_glass.h's analytic tracer, the rest is the
// mesh instantiations' (d2, em * att); it reads no table.
#include "tvam_internal.h"

#include <algorithm>

#include "tvam_cone_ray.h"

namespace {

// The ray of flat index ix (cn_ray_at, tvam_cone_ray.h).
template <int MESH>
__device__ __forceinline__ bool cn_ray(const TvamConsts& k, const TvamTiles& tp, const int32_t* idxmap,
                                       const TvamPathIndex& ix, ConeRay& r, const TvamMeshView& mesh) {
    return cn_ray_at<MESH>(k, tp, ix.al, ix.colc, ix.rowc, tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp), r, &mesh);
}

// the workgroup's LDS copy of the meshes (CN_MESH_LDS launches pass cn_mesh_lds_bytes of dynamic LDS)
extern __shared__ float4 cn_mesh_lds[];

template <int MODE, int MESH>
__global__ __launch_bounds__(256) void tvam_cone_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ pat,
                                                        const int32_t* __restrict__ idxmap,
                                                        const float* __restrict__ gin, float* __restrict__ out,
                                                        unsigned long long* __restrict__ counter) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    uint64_t nvis = 0;
    const bool f32 = false;  // (the 64-bit decode alone: the second one costs this kernel its 7th wave/SIMD)
    const TvamMeshView mesh = cn_mesh_view<MESH>(k, cn_mesh_lds);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<MODE>(k, pat, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        if (!cn_ray<MESH>(k, tp, idxmap, ix, r, mesh)) continue;
        if (MESH == CN_NO_MESH) {
            const float acc = cn_dda<MODE>(k, r.o2, r.d, r.maxt, em, out, gin, nvis);
            if (MODE == TVAM_MODE_ADJ) {
                if (spp == 1) out[act] = acc * k.wscale;  // the entry's only ray: no atomic
                else if (acc != 0.0f) atomicAdd(&out[act], acc * k.wscale);
            }
        } else {
            const float acc = cn_dda<MODE>(k, r.o2, r.d2, r.maxt, em * r.att, out, gin, nvis) * r.att;
            if (MODE == TVAM_MODE_ADJ) {
                if (spp == 1) out[act] = acc * k.wscale;
                else if (acc != 0.0f) atomicAdd(&out[act], acc * k.wscale);
            }
        }
    }
    if (MODE == TVAM_MODE_COUNT) tvam_count_reduce(nvis, counter);
}

// One brick-bin record per ray of paths [sb.p0, sb.p1) (sb.slots = 1; the layout of
// tvam_scatter_kernel<EMIT>'s records: weight em, attenuation 1 for the cached forward's rescale,
// 0 in slots without a segment), its brick count and the chunk's largest |weight|.
template <int MESH>
__global__ __launch_bounds__(256) void tvam_cone_emit_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ pat,
                                                             const int32_t* __restrict__ idxmap, TvamSegBuf sb) {
    float wmax = 0.0f;
    const bool f32 = tvam_path_fits32(sb.p1);
    const TvamMeshView mesh = cn_mesh_view<MESH>(k, cn_mesh_lds);
    for (int64_t i = sb.p0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < sb.p1;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = i - sb.p0;
        reinterpret_cast<float*>(&sb.r[TVAM_REC_F4 * slot + 2])[2] = 0.0f;
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_FWD>(k, pat, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        if (!cn_ray<MESH>(k, tp, idxmap, ix, r, mesh)) continue;
        SegDda q;
        if (!sc_dda_init(k, r.o2, MESH == CN_NO_MESH ? r.d : r.d2, r.maxt, q)) continue;
        const float att = MESH == CN_NO_MESH ? 1.0f : r.att;  // (.z: the cached forward's rescale)
        if (MESH != CN_NO_MESH) em = em * att;
        sb.r[TVAM_REC_F4 * slot] = make_float4(q.t_start, q.tau_end, q.dtm0[0], q.dtm0[1]);
        sb.r[TVAM_REC_F4 * slot + 1] = make_float4(q.dtm0[2], q.ts[0] * (float)q.step[0], q.ts[1] * (float)q.step[1],
                                                   q.ts[2] * (float)q.step[2]);
        sb.r[TVAM_REC_F4 * slot + 2] = make_float4(__int_as_float(q.sv[0] | (q.sv[1] << 11) | (q.sv[2] << 22)), em, att, 0.0f);
        sb.m[slot] = (uint32_t)sc_brick_count(k, q);
        wmax = fmaxf(wmax, fabsf(em));
    }
    sc_block_max(wmax, sb.wmax);
}

// tvam_plan_rays: row act * spp + smp = o[3], d[3], hit, o2[3], maxt, d2[3], weight, 0
template <int MESH>
__global__ __launch_bounds__(256) void tvam_cone_export_kernel(TvamConsts k, TvamTiles tp,
                                                               const int32_t* __restrict__ idxmap,
                                                               float* __restrict__ rays) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    const bool f32 = tvam_path_fits32(n);
    const TvamMeshView mesh = cn_mesh_view<MESH>(k, cn_mesh_lds);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_ADJ>(k, nullptr, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        r.o2[0] = r.o2[1] = r.o2[2] = 0.0f;
        r.maxt = 0.0f;
        const bool hit = cn_ray<MESH>(k, tp, idxmap, ix, r, mesh);
        if (MESH == CN_NO_MESH || !hit) {  // (a ray that never reaches the medium keeps its own direction)
            r.d2[0] = r.d[0], r.d2[1] = r.d[1], r.d2[2] = r.d[2];
            r.att = 1.0f;
        }
        float4* row = reinterpret_cast<float4*>(rays + 16 * (act * spp + ix.smp));
        row[0] = make_float4(r.o[0], r.o[1], r.o[2], r.d[0]);
        row[1] = make_float4(r.d[1], r.d[2], hit ? 1.0f : 0.0f, hit ? r.o2[0] : 0.0f);
        row[2] = make_float4(hit ? r.o2[1] : 0.0f, hit ? r.o2[2] : 0.0f, hit ? r.maxt : 0.0f, r.d2[0]);
        row[3] = make_float4(r.d2[1], r.d2[2], MESH == CN_NO_MESH ? k.wscale : k.wscale * r.att, 0.0f);
    }
}

}  // namespace

template <int MESH>
static void cn_launch_rays(int mode, const TvamConsts& k, const TvamTiles& t, const float* pat, const int32_t* idxmap,
                           const float* gin, float* out, unsigned long long* counter, hipStream_t stream) {
    const dim3 g(tvam_grid_1d((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp, 262144)), b(256);
    const size_t lds = cn_lds(k);
    switch (mode) {
        case TVAM_MODE_FWD:
            tvam_kt_begin(stream, TVAM_KT_CONE);
            hipLaunchKernelGGL((tvam_cone_kernel<TVAM_MODE_FWD, MESH>), g, b, lds, stream, k, t, pat, idxmap, gin, out,
                               counter);
            tvam_kt_end(stream, TVAM_KT_CONE);
            break;
        case TVAM_MODE_ADJ:
            hipLaunchKernelGGL((tvam_cone_kernel<TVAM_MODE_ADJ, MESH>), g, b, lds, stream, k, t, pat, idxmap, gin, out,
                               counter);
            break;
        default:
            hipLaunchKernelGGL((tvam_cone_kernel<TVAM_MODE_COUNT, MESH>), g, b, lds, stream, k, t, pat, idxmap, gin, out,
                               counter);
    }
}

hipError_t tvam_launch_cone_rays(int mode, const TvamConsts& k, const TvamTiles& t, const float* pat,
                                 const int32_t* idxmap, const float* gin, float* out, unsigned long long* counter,
                                 hipStream_t stream) {
    switch (cn_mesh_mode(k)) {
        case CN_NO_MESH: cn_launch_rays<CN_NO_MESH>(mode, k, t, pat, idxmap, gin, out, counter, stream); break;
        case CN_MESH_LDS: cn_launch_rays<CN_MESH_LDS>(mode, k, t, pat, idxmap, gin, out, counter, stream); break;
        case CN_GLASS: cn_launch_rays<CN_GLASS>(mode, k, t, pat, idxmap, gin, out, counter, stream); break;
        default: cn_launch_rays<CN_MESH_GLOBAL>(mode, k, t, pat, idxmap, gin, out, counter, stream);
    }
    return hipGetLastError();
}

void tvam_cone_write_records(const TvamConsts& k, const TvamTiles& t, const float* pat, const int32_t* idxmap,
                             const TvamSegBuf& sb, unsigned grid, hipStream_t stream) {
    const dim3 g(grid), b(256);
    switch (cn_mesh_mode(k)) {
        case CN_NO_MESH:
            hipLaunchKernelGGL(tvam_cone_emit_kernel<CN_NO_MESH>, g, b, 0, stream, k, t, pat, idxmap, sb);
            break;
        case CN_MESH_LDS:
            hipLaunchKernelGGL(tvam_cone_emit_kernel<CN_MESH_LDS>, g, b, cn_lds(k), stream, k, t, pat, idxmap, sb);
            break;
        case CN_GLASS:
            hipLaunchKernelGGL(tvam_cone_emit_kernel<CN_GLASS>, g, b, 0, stream, k, t, pat, idxmap, sb);
            break;
        default:
            hipLaunchKernelGGL(tvam_cone_emit_kernel<CN_MESH_GLOBAL>, g, b, 0, stream, k, t, pat, idxmap, sb);
    }
}

hipError_t tvam_launch_cone_export(const TvamConsts& k, const TvamTiles& t, const int32_t* idxmap, float* rays,
                                   hipStream_t stream) {
    const dim3 g(tvam_grid_1d((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp, 262144)), b(256);
    switch (cn_mesh_mode(k)) {
        case CN_NO_MESH: hipLaunchKernelGGL(tvam_cone_export_kernel<CN_NO_MESH>, g, b, 0, stream, k, t, idxmap, rays); break;
        case CN_MESH_LDS:
            hipLaunchKernelGGL(tvam_cone_export_kernel<CN_MESH_LDS>, g, b, cn_lds(k), stream, k, t, idxmap, rays);
            break;
        case CN_GLASS: hipLaunchKernelGGL(tvam_cone_export_kernel<CN_GLASS>, g, b, 0, stream, k, t, idxmap, rays); break;
        default: hipLaunchKernelGGL(tvam_cone_export_kernel<CN_MESH_GLOBAL>, g, b, 0, stream, k, t, idxmap, rays);
    }
    return hipGetLastError();
}

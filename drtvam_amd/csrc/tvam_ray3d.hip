// 3-D ray plans: projector rays with a finite etendue (telecentric and lens projectors,
// projector.py:199-296) and vials traced per ray in 3-D ('custom' meshes, traced 'cylindrical' /
// 'square' glass, 'double_cylindrical', dielectric occluders, reflected paths).  Such a ray leaves its z-slice, so
// none of the planar / tile kernels (d.z = 0) applies.  The pieces are the scattered segments' own
// (tvam_seg3d.h, tvam_bricks.h: the 3-D DDA and the brick bins), the ray generation of
// tvam_cone_ray.h and, for what tells the plans apart, the walk policies of tvam_ray3d.h.
//
//   tvam_ray3d_kernel<MODE, WALK>   one thread per (ray, sample): each segment marched by cn_dda (the
//                       oracle's or_dda op for op) with weight em * att as the walk finds it (one
//                       copy of the DDA, never two segments in registers).  Forward: global float
//                       atomics; adjoint: a gather summed over the segments (a plain store per
//                       active entry when spp == 1); visit count
//   tvam_ray3d_emit_kernel<WALK>    SLOTS brick-bin records per path for tvam_scatter_binned (the
//                       binned forward: bin fill, sort, tvam_bin_march_kernel and the bin cache)
//   tvam_ray3d_export_kernel<WALK>  the rays themselves (tvam_plan_rays: the first segment) and
//                       their segments (tvam_plan_segments, tvam_plan_insert_segments)
// DESIGN.md section 4m has the register figures these shapes were chosen for.
#include "tvam_internal.h"

#include "tvam_ray3d.h"

namespace {

template <int MODE, typename WALK>
__global__ __launch_bounds__(256) void tvam_ray3d_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ aux,
                                                         const float* __restrict__ pat,
                                                         const int32_t* __restrict__ idxmap,
                                                         const float* __restrict__ gin, float* __restrict__ out,
                                                         unsigned long long* __restrict__ counter) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    uint64_t nvis = 0;
    const bool f32 = false;  // (the 64-bit decode alone: the second one costs this kernel its 7th wave/SIMD)
    const WALK walk(k, aux);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<MODE>(k, pat, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        typename WALK::State st;
        walk.start(k, tp, idxmap, ix, r, st);
        float acc = 0.0f;
        if (WALK::SLOTS == 1) {
            if (!walk.next(k, r, st)) continue;
            acc = cn_dda<MODE>(k, r.o2, r.d2, r.maxt, em * r.att, out, gin, nvis) * r.att;
        } else {
            // (a counted loop where the walk is bounded: as a `while`, the two-segment forward took
            // 76 VGPRs for 67 and lost a wave per SIMD)
#pragma unroll 1
            for (int s = 0; WALK::SLOTS == 0 || s < WALK::SLOTS; ++s) {
                if (!walk.next(k, r, st)) break;
                acc = acc + cn_dda<MODE>(k, r.o2, r.d2, r.maxt, em * r.att, out, gin, nvis) * r.att;
            }
        }
        if (MODE == TVAM_MODE_ADJ) {
            if (spp == 1) out[act] = acc * k.wscale;  // the entry's only ray: no atomic
            else if (acc != 0.0f) atomicAdd(&out[act], acc * k.wscale);
        }
    }
    if (MODE == TVAM_MODE_COUNT) tvam_count_reduce(nvis, counter);
}

// SLOTS brick-bin records per path of [sb.p0, sb.p1) (sb.slots = SLOTS; sc_pack: weight em * att,
// .z = att for the cached forward's rescale; a slot without a segment keeps .z = 0 and m = 0),
// their brick counts and the chunk's largest |weight|.
template <typename WALK>
__global__ __launch_bounds__(256) void tvam_ray3d_emit_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ aux,
                                                              const float* __restrict__ pat,
                                                              const int32_t* __restrict__ idxmap, TvamSegBuf sb) {
    float wmax = 0.0f;
    const bool f32 = tvam_path_fits32(sb.p1);
    const WALK walk(k, aux);
    for (int64_t i = sb.p0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < sb.p1;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot0 = (i - sb.p0) * WALK::SLOTS;
#pragma unroll
        for (int s = 0; s < WALK::SLOTS; ++s) reinterpret_cast<float*>(&sb.r[TVAM_REC_F4 * (slot0 + s) + 2])[2] = 0.0f;
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_FWD>(k, pat, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        typename WALK::State st;
        walk.start(k, tp, idxmap, ix, r, st);
#pragma unroll 1
        for (int s = 0; s < WALK::SLOTS; ++s) {
            if (!walk.next(k, r, st)) break;
            SegDda q;
            if (!sc_dda_init(k, r.o2, r.d2, r.maxt, q)) continue;
            const float wgt = em * r.att;
            sc_pack(sb, slot0 + s, q, wgt, r.att);
            sb.m[slot0 + s] = (uint32_t)sc_brick_count(k, q);
            wmax = fmaxf(wmax, fabsf(wgt));
        }
    }
    sc_block_max(wmax, sb.wmax);
}

// rays (tvam_plan_rays, may be null): row act * spp + smp = o[3], d[3], hit, o2[3], maxt, d2[3],
// weight, 0 of the first segment (a ray that never reaches the medium keeps its own direction);
// segs (tvam_plan_segments / tvam_plan_insert_segments, may be null): [row][max_segments] = o2[3],
// maxt, d2[3], weight, zeros past the row's segments; nseg (may be null): the row's segments.
template <typename WALK>
__global__ __launch_bounds__(256) void tvam_ray3d_export_kernel(TvamConsts k, TvamTiles tp,
                                                                const float* __restrict__ aux,
                                                                const int32_t* __restrict__ idxmap,
                                                                float* __restrict__ rays, float* __restrict__ segs,
                                                                int max_segments, int32_t* __restrict__ nseg) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    const bool f32 = tvam_path_fits32(n);
    const WALK walk(k, aux);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_ADJ>(k, nullptr, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        typename WALK::State st;
        walk.start(k, tp, idxmap, ix, r, st);
        const int64_t row = act * spp + ix.smp;
        int s = 0;
#pragma unroll 1
        while ((WALK::SLOTS == 0 || s < WALK::SLOTS) && walk.next(k, r, st)) {
            if (segs && s < max_segments) {
                float4* sg = reinterpret_cast<float4*>(segs + 8 * (row * max_segments + s));
                sg[0] = make_float4(r.o2[0], r.o2[1], r.o2[2], r.maxt);
                sg[1] = make_float4(r.d2[0], r.d2[1], r.d2[2], k.wscale * r.att);
            }
            if (rays && s == 0) {
                float4* rw = reinterpret_cast<float4*>(rays + 16 * row);
                rw[0] = make_float4(r.o[0], r.o[1], r.o[2], r.d[0]);
                rw[1] = make_float4(r.d[1], r.d[2], 1.0f, r.o2[0]);
                rw[2] = make_float4(r.o2[1], r.o2[2], r.maxt, r.d2[0]);
                rw[3] = make_float4(r.d2[1], r.d2[2], k.wscale * r.att, 0.0f);
            }
            ++s;
            if (!segs) break;  // the rays hold the first segment alone
        }
        if (rays && s == 0) {
            float4* rw = reinterpret_cast<float4*>(rays + 16 * row);
            rw[0] = make_float4(r.o[0], r.o[1], r.o[2], r.d[0]);
            rw[1] = make_float4(r.d[1], r.d[2], 0.0f, 0.0f);
            rw[2] = make_float4(0.0f, 0.0f, 0.0f, r.d[0]);
            rw[3] = make_float4(r.d[1], r.d[2], k.wscale, 0.0f);
        }
        if (segs)
            for (int q = s < max_segments ? s : max_segments; q < max_segments; ++q) {
                float4* sg = reinterpret_cast<float4*>(segs + 8 * (row * max_segments + q));
                sg[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                sg[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        if (nseg) nseg[row] = s;
    }
}

// The policy that serves (walk, k) and its dynamic LDS: f(R3Walk<WALK>{}, bytes).
template <typename W>
struct R3Walk {
    typedef W type;
};
template <typename F>
void r3_dispatch(int walk, const TvamConsts& k, F&& f) {
    if (walk == TVAM_WALK_INSERT) {
        if (k.mesh.lds_bytes > 0) f(R3Walk<WalkInsert<CN_MESH_LDS>>{}, cn_mesh_lds_bytes(k.mesh));
        else f(R3Walk<WalkInsert<CN_MESH_GLOBAL>>{}, (size_t)0);
    } else if (walk == TVAM_WALK_REFLECT) {
        if (k.mesh.n_tris <= 0) f(R3Walk<WalkReflect<CN_NO_MESH>>{}, (size_t)0);
        else if (k.mesh.lds_bytes > 0) f(R3Walk<WalkReflect<CN_MESH_LDS>>{}, cn_mesh_lds_bytes(k.mesh));
        else f(R3Walk<WalkReflect<CN_MESH_GLOBAL>>{}, (size_t)0);
    } else if (walk == TVAM_WALK_DOUBLE) {
        f(R3Walk<WalkDouble>{}, (size_t)0);
    } else {
        switch (cn_mesh_mode(k)) {
            case CN_NO_MESH: f(R3Walk<WalkOne<CN_NO_MESH>>{}, (size_t)0); break;
            case CN_MESH_LDS: f(R3Walk<WalkOne<CN_MESH_LDS>>{}, cn_lds(k)); break;
            case CN_GLASS: f(R3Walk<WalkOne<CN_GLASS>>{}, (size_t)0); break;
            default: f(R3Walk<WalkOne<CN_MESH_GLOBAL>>{}, (size_t)0);
        }
    }
}

inline dim3 r3_grid(const TvamConsts& k, const TvamTiles& t) {
    return dim3(tvam_grid_1d((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp, 262144));
}

}  // namespace

hipError_t tvam_launch_ray3d(int mode, int walk, const TvamConsts& k, const TvamTiles& t, const float* aux,
                             const float* pat, const int32_t* idxmap, const float* gin, float* out,
                             unsigned long long* counter, hipStream_t stream) {
    const dim3 g = r3_grid(k, t), b(256);
    r3_dispatch(walk, k, [&](auto w, size_t lds) {
        typedef typename decltype(w)::type W;
        switch (mode) {
            case TVAM_MODE_FWD:
                tvam_kt_begin(stream, TVAM_KT_CONE);
                hipLaunchKernelGGL((tvam_ray3d_kernel<TVAM_MODE_FWD, W>), g, b, lds, stream, k, t, aux, pat, idxmap, gin,
                                   out, counter);
                tvam_kt_end(stream, TVAM_KT_CONE);
                break;
            case TVAM_MODE_ADJ:
                hipLaunchKernelGGL((tvam_ray3d_kernel<TVAM_MODE_ADJ, W>), g, b, lds, stream, k, t, aux, pat, idxmap, gin,
                                   out, counter);
                break;
            default:
                hipLaunchKernelGGL((tvam_ray3d_kernel<TVAM_MODE_COUNT, W>), g, b, lds, stream, k, t, aux, pat, idxmap,
                                   gin, out, counter);
        }
    });
    return hipGetLastError();
}

void tvam_ray3d_write_records(int walk, const TvamConsts& k, const TvamTiles& t, const float* pat,
                              const int32_t* idxmap, const TvamSegBuf& sb, unsigned grid, hipStream_t stream) {
    r3_dispatch(walk, k, [&](auto w, size_t lds) {
        typedef typename decltype(w)::type W;
        if constexpr (W::SLOTS > 0)  // (tvam_scatter_binned takes no walk without slots)
            hipLaunchKernelGGL(tvam_ray3d_emit_kernel<W>, dim3(grid), dim3(256), lds, stream, k, t, nullptr, pat, idxmap,
                               sb);
    });
}

hipError_t tvam_launch_ray3d_export(int walk, const TvamConsts& k, const TvamTiles& t, const float* aux,
                                    const int32_t* idxmap, float* rays, float* segs, int32_t max_segments,
                                    int32_t* nseg, hipStream_t stream) {
    r3_dispatch(walk, k, [&](auto w, size_t lds) {
        typedef typename decltype(w)::type W;
        hipLaunchKernelGGL(tvam_ray3d_export_kernel<W>, r3_grid(k, t), dim3(256), lds, stream, k, t, aux, idxmap, rays,
                           segs, max_segments, nseg);
    });
    return hipGetLastError();
}

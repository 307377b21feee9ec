// Dielectric occluders (geometry.py:55-72 with a 'bsdf' entry; tvam_insert.h): transparent inserts
// inside the resin.  Every ray is traced in 3-D through the container, the black occluders and the
// inserts' triangles and deposits along every stretch it runs in the resin, for all three projectors
// and the 'index_matched', 'cylindrical' and 'square' vials.  The pieces are those of tvam_cone.hip
// and tvam_double.hip: cn_ray_at for the projector ray (whose generator the walk goes on drawing
// from for the Russian roulette), cn_mesh_view for the hierarchy (staged in LDS when it fits),
// cn_dda for a segment's march.
//
//   tvam_insert_kernel         one thread per (ray, sample): the resumable walk of tvam_insert.h,
//                              each segment marched by cn_dda with weight em * att_s as it is
//                              found (one copy of the DDA).  Forward: global float atomics; adjoint:
//                              a gather summed over the segments (a plain store per active entry
//                              when spp == 1); count.
//   tvam_insert_export_kernel  the rays (tvam_plan_rays: the first segment) and every segment
//                              (tvam_plan_insert_segments)
// and, on the host, the validation of the inserts.
#include "tvam_plan.h"

#include <cmath>

#include "tvam_cone_ray.h"
#include "tvam_insert.h"

namespace {

// The draws of a device walk: the ray's own generator, four numbers per surface iteration in the
// order of tvam_path.h (roulette, then the BSDF's next_1d + next_2d, ignored).
struct InsDraws {
    TvamPcg rng;
    __device__ __forceinline__ float rr(int) { return rng.next_float(); }
    __device__ __forceinline__ void bsdf() {
        (void)rng.next_float();
        (void)rng.next_float();
        (void)rng.next_float();
    }
};

// The projector ray of flat index ix and the start of its walk.
__device__ __forceinline__ void in_ray(const TvamConsts& k, const TvamTiles& tp, const int32_t* idxmap,
                                       const TvamPathIndex& ix, ConeRay& r, InsDraws& dr, TvamInsertWalk& w) {
    (void)cn_ray_at<CN_NO_MESH, true>(k, tp, ix.al, ix.colc, ix.rowc, tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp), r,
                                      dr.rng);
    tvam_insert_start(w, r.o, r.d);
}

__device__ __forceinline__ bool in_next(const TvamConsts& k, const TvamInsertScene& sc, bool rr, InsDraws& dr,
                                        TvamInsertWalk& w, ConeRay& r) {
    return tvam_insert_next(k, sc, rr, dr, w, r.o2, r.d2, r.maxt, r.att);
}

// the workgroup's LDS copy of the hierarchy (CN_MESH_LDS launches pass cn_mesh_lds_bytes of dynamic LDS)
extern __shared__ __attribute__((aligned(16))) float4 in_mesh_lds[];

// MESH: CN_MESH_LDS or CN_MESH_GLOBAL (how the hierarchy is read)
template <int MODE, int MESH>
__global__ __launch_bounds__(256) void tvam_insert_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ tri_eta,
                                                          const float* __restrict__ pat,
                                                          const int32_t* __restrict__ idxmap,
                                                          const float* __restrict__ gin, float* __restrict__ out,
                                                          unsigned long long* __restrict__ counter) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    uint64_t nvis = 0;
    const bool f32 = false;  // (the 64-bit decode alone, as in tvam_cone_kernel)
    TvamInsertScene sc;
    sc.mesh = cn_mesh_view<MESH>(k, in_mesh_lds);
    sc.tri_eta = tri_eta;
    const bool rr = tvam_insert_roulette_on(k.rr_depth, k.max_depth);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<MODE>(k, pat, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        InsDraws dr;
        TvamInsertWalk w;
        in_ray(k, tp, idxmap, ix, r, dr, w);
        float acc = 0.0f;
#pragma unroll 1
        while (in_next(k, sc, rr, dr, w, r))
            acc = acc + cn_dda<MODE>(k, r.o2, r.d2, r.maxt, em * r.att, out, gin, nvis) * r.att;
        if (MODE == TVAM_MODE_ADJ) {
            if (spp == 1) out[act] = acc * k.wscale;  // the entry's only ray: no atomic
            else if (acc != 0.0f) atomicAdd(&out[act], acc * k.wscale);
        }
    }
    if (MODE == TVAM_MODE_COUNT) tvam_count_reduce(nvis, counter);
}

// rays (tvam_plan_rays, may be null): row act * spp + smp = o[3], d[3], hit, o2[3], maxt, d2[3],
// weight, 0 of the first segment (the traced plans' layout); segs / nseg (tvam_plan_insert_segments,
// may be null): [row][max_segments] = o2[3], maxt, d2[3], weight, zeros past the row's nseg segments.
template <int MESH>
__global__ __launch_bounds__(256) void tvam_insert_export_kernel(TvamConsts k, TvamTiles tp,
                                                                 const float* __restrict__ tri_eta,
                                                                 const int32_t* __restrict__ idxmap,
                                                                 float* __restrict__ rays, float* __restrict__ segs,
                                                                 int max_segments, int32_t* __restrict__ nseg) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    const bool f32 = tvam_path_fits32(n);
    TvamInsertScene sc;
    sc.mesh = cn_mesh_view<MESH>(k, in_mesh_lds);
    sc.tri_eta = tri_eta;
    const bool rr = tvam_insert_roulette_on(k.rr_depth, k.max_depth);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_ADJ>(k, nullptr, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        InsDraws dr;
        TvamInsertWalk w;
        in_ray(k, tp, idxmap, ix, r, dr, w);
        const int64_t row = act * spp + ix.smp;
        int s = 0;
#pragma unroll 1
        while (in_next(k, sc, rr, dr, w, r)) {
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
        if (segs) {
            for (int q = s < max_segments ? s : max_segments; q < max_segments; ++q) {
                float4* sg = reinterpret_cast<float4*>(segs + 8 * (row * max_segments + q));
                sg[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                sg[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            nseg[row] = s;
        }
    }
}

inline bool in_lds(const TvamConsts& k) { return k.mesh.lds_bytes > 0; }

}  // namespace

hipError_t tvam_launch_insert_rays(int mode, const TvamConsts& k, const TvamTiles& t, const float* tri_eta,
                                   const float* pat, const int32_t* idxmap, const float* gin, float* out,
                                   unsigned long long* counter, hipStream_t stream) {
    const dim3 g(tvam_grid_1d((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp, 262144)), b(256);
    const bool lds = in_lds(k);
    const size_t nb = lds ? cn_mesh_lds_bytes(k.mesh) : 0;
#define TVAM_INS_LAUNCH(M)                                                                                              \
    do {                                                                                                                \
        if (lds)                                                                                                        \
            hipLaunchKernelGGL((tvam_insert_kernel<M, CN_MESH_LDS>), g, b, nb, stream, k, t, tri_eta, pat, idxmap, gin, \
                               out, counter);                                                                           \
        else                                                                                                            \
            hipLaunchKernelGGL((tvam_insert_kernel<M, CN_MESH_GLOBAL>), g, b, 0, stream, k, t, tri_eta, pat, idxmap,    \
                               gin, out, counter);                                                                      \
    } while (0)
    switch (mode) {
        case TVAM_MODE_FWD:
            tvam_kt_begin(stream, TVAM_KT_CONE);
            TVAM_INS_LAUNCH(TVAM_MODE_FWD);
            tvam_kt_end(stream, TVAM_KT_CONE);
            break;
        case TVAM_MODE_ADJ: TVAM_INS_LAUNCH(TVAM_MODE_ADJ); break;
        default: TVAM_INS_LAUNCH(TVAM_MODE_COUNT);
    }
#undef TVAM_INS_LAUNCH
    return hipGetLastError();
}

hipError_t tvam_launch_insert_export(const TvamConsts& k, const TvamTiles& t, const float* tri_eta,
                                     const int32_t* idxmap, float* rays, float* segs, int32_t max_segments,
                                     int32_t* nseg, hipStream_t stream) {
    const dim3 g(tvam_grid_1d((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp, 262144)), b(256);
    if (in_lds(k))
        hipLaunchKernelGGL(tvam_insert_export_kernel<CN_MESH_LDS>, g, b, cn_mesh_lds_bytes(k.mesh), stream, k, t, tri_eta,
                           idxmap, rays, segs, max_segments, nseg);
    else
        hipLaunchKernelGGL(tvam_insert_export_kernel<CN_MESH_GLOBAL>, g, b, 0, stream, k, t, tri_eta, idxmap, rays, segs,
                           max_segments, nseg);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

// The inserts of tvam_plan_create_inserts / tvam_insert_segments against the container of k:
// TVAM_ERR_INVALID naming the insert and the triangle or vertex, 0 if sound.  No device call.
int tvam_inserts_validate(const TvamConsts& k, const tvam_insert* ins, int32_t n) {
    if (!ins || n <= 0) return tvam_fail(TVAM_ERR_INVALID, "dielectric occluders: no insert given");
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) {
        const std::string who = "insert " + std::to_string(i);
        const tvam_insert& s = ins[i];
        if (!s.tris || s.n_tris <= 0) return tvam_fail(TVAM_ERR_INVALID, who + ": the mesh is null or empty");
        if (!(s.int_ior > 0.0f && s.ext_ior > 0.0f) || !std::isfinite(s.int_ior) || !std::isfinite(s.ext_ior))
            return tvam_fail(TVAM_ERR_INVALID, who + ": int_ior and ext_ior must be positive");
        total += s.n_tris;
        if (total >= (1 << 27)) return tvam_fail(TVAM_ERR_TOO_LARGE, "the inserts have too many triangles");
        for (int32_t j = 0; j < s.n_tris; ++j) {
            const float* v = s.tris + 9 * (size_t)j;
            for (int q = 0; q < 9; ++q)
                if (!std::isfinite(v[q]))
                    return tvam_fail(TVAM_ERR_INVALID, who + ": triangle " + std::to_string(j) + " vertex " +
                                                           std::to_string(q / 3) + " is not finite");
            float nx, ny, nz;
            tvam_tri_normal(v, nx, ny, nz);  // the kernels' own normal: it must exist
            if (!(std::isfinite(nx) && std::isfinite(ny) && std::isfinite(nz)))
                return tvam_fail(TVAM_ERR_INVALID, who + ": triangle " + std::to_string(j) + " has zero area");
            for (int c = 0; c < 3; ++c) {
                const float x = v[3 * c], y = v[3 * c + 1], z = v[3 * c + 2];
                const bool out = k.vial_type == TVAM_VIAL_SQUARE
                                     ? (std::fabs(x) > k.vial_r || std::fabs(y) > k.vial_r || std::fabs(z) > k.vial_hz_int)
                                     : (std::sqrt(x * x + y * y) >= k.vial_r || std::fabs(z) > k.vial_half_h);
                if (out)
                    return tvam_fail(TVAM_ERR_INVALID, who + ": triangle " + std::to_string(j) + " vertex " +
                                                           std::to_string(c) + " lies outside the resin");
            }
        }
    }
    return 0;
}

// All inserts' triangles in the caller's order, and each triangle's eta = int_ior / ext_ior.
void tvam_inserts_flatten(const tvam_insert* ins, int32_t n, std::vector<float>& tris, std::vector<float>& tri_eta) {
    tris.clear(), tri_eta.clear();
    for (int32_t i = 0; i < n; ++i) {
        tris.insert(tris.end(), ins[i].tris, ins[i].tris + 9 * (size_t)ins[i].n_tris);
        tri_eta.insert(tri_eta.end(), (size_t)ins[i].n_tris, ins[i].int_ior / ins[i].ext_ior);
    }
}

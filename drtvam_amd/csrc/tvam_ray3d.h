// tvam_ray3d.h -- the walk policies of the 3-D ray kernels (tvam_ray3d.hip; device only).  A 3-D ray
// plan differs from another only in how a ray's next medium segment is found; a policy is that
// difference, and the march, record and export kernels are written once over it.
//
//   SLOTS               the most segments a ray can have, 0: any number
//   WALK(k, aux)        once per thread, before the ray loop (every thread of the workgroup: the
//                       CN_MESH_LDS views stage the hierarchy and synchronise); it holds what is
//                       constant for the kernel, and the kernel keeps the object const
//   State               what the walk carries from one segment to the next: a local of the ray
//                       loop's body (as members of the policy object, alive across grid-stride
//                       iterations, it cost a prototype's insert forward a wave per SIMD)
//   start(k, tp, idxmap, ix, r, st)   the projector ray of flat index ix into r.o / r.d
//   next(k, r, st)      the next segment into r.o2 / r.d2 / r.maxt / r.att, false: no more
#pragma once
#include "tvam_cone_ray.h"
#include "tvam_double.h"
#include "tvam_insert.h"

namespace {

// the workgroup's LDS copy of the hierarchy (CN_MESH_LDS launches pass cn_mesh_lds_bytes of dynamic LDS)
extern __shared__ __attribute__((aligned(16))) float4 r3_mesh_lds[];

// One segment: behind the index-matched vial, the meshes of a 'custom' vial or the analytic glass of
// a traced vial (cn_ray_at<MESH>).  Index matched, the segment runs along the ray itself with
// weight 1, which the compiler folds out of the kernels again.
template <int MESH>
struct WalkOne {
    static constexpr int SLOTS = 1;
    TvamMeshView mesh;
    struct State {
        bool hit;
    };
    __device__ __forceinline__ WalkOne(const TvamConsts& k, const float*) : mesh(cn_mesh_view<MESH>(k, r3_mesh_lds)) {}
    __device__ __forceinline__ void start(const TvamConsts& k, const TvamTiles& tp, const int32_t* idxmap,
                                          const TvamPathIndex& ix, ConeRay& r, State& st) const {
        st.hit = cn_ray_at<MESH>(k, tp, ix.al, ix.colc, ix.rowc, tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp), r,
                                 &mesh);
        if (MESH == CN_NO_MESH) {
            r.d2[0] = r.d[0], r.d2[1] = r.d[1], r.d2[2] = r.d[2];
            r.att = 1.0f;
        }
    }
    __device__ __forceinline__ bool next(const TvamConsts&, ConeRay&, State& st) const {
        const bool hit = st.hit;
        st.hit = false;
        return hit;
    }
};

// 'double_cylindrical' vial: the resumable walk of tvam_double.h, in front of the inner vial and behind it.
struct WalkDouble {
    static constexpr int SLOTS = 2;
    typedef TvamDoubleWalk State;
    __device__ __forceinline__ WalkDouble(const TvamConsts&, const float*) {}
    __device__ __forceinline__ void start(const TvamConsts& k, const TvamTiles& tp, const int32_t* idxmap,
                                          const TvamPathIndex& ix, ConeRay& r, State& st) const {
        cn_projector_ray(k, tp, ix.al, ix.colc, ix.rowc, tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp), r);
        tvam_double_start(st, r.o, r.d);
    }
    __device__ __forceinline__ bool next(const TvamConsts& k, ConeRay& r, State& st) const {
        return tvam_double_next(k.dbl, k.vial_half_h, k.sig_t, k.max_depth, st, r.o2, r.d2, r.maxt, r.att);
    }
};

// The draws of a device walk through inserts: the ray's own generator, four numbers per surface
// iteration in the order of tvam_path.h (roulette, then the BSDF's next_1d + next_2d, ignored).
struct InsDraws {
    TvamPcg rng;
    __device__ __forceinline__ float rr(int) { return rng.next_float(); }
    __device__ __forceinline__ void bsdf() {
        (void)rng.next_float();
        (void)rng.next_float();
        (void)rng.next_float();
    }
    // (a reflecting walk uses the first of the BSDF's three: next_1d)
    __device__ __forceinline__ float s1(int) {
        const float s = rng.next_float();
        (void)rng.next_float();
        (void)rng.next_float();
        return s;
    }
};

// Dielectric occluders: the resumable walk of tvam_insert.h, which goes on drawing from the ray's
// generator for the Russian roulette.  MESH: CN_MESH_LDS or CN_MESH_GLOBAL (how the hierarchy is
// read); aux: tri_eta.
template <int MESH>
struct WalkInsert {
    static constexpr int SLOTS = 0;
    TvamInsertScene sc;
    bool rr;
    struct State {
        InsDraws dr;
        TvamInsertWalk w;
    };
    __device__ __forceinline__ WalkInsert(const TvamConsts& k, const float* tri_eta)
        : sc{cn_mesh_view<MESH>(k, r3_mesh_lds), tri_eta}, rr(tvam_insert_roulette_on(k.rr_depth, k.max_depth)) {}
    __device__ __forceinline__ void start(const TvamConsts& k, const TvamTiles& tp, const int32_t* idxmap,
                                          const TvamPathIndex& ix, ConeRay& r, State& st) const {
        (void)cn_ray_at<CN_NO_MESH, true>(k, tp, ix.al, ix.colc, ix.rowc,
                                          tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp), r, st.dr.rng);
        tvam_insert_start(st.w, r.o, r.d);
    }
    __device__ __forceinline__ bool next(const TvamConsts& k, ConeRay& r, State& st) const {
        return tvam_insert_next(k, sc, rr, st.dr, st.w, r.o2, r.d2, r.maxt, r.att);
    }
};

// transmission_only = 0 (tvam_plan_create_reflect): the same walk with reflection sampled against
// refraction at every dielectric interface after the first (tvam_insert_next<true>).  It always
// draws its four numbers per surface iteration.  MESH: CN_MESH_LDS, CN_MESH_GLOBAL, or CN_NO_MESH
// for a plan without inserts (no hierarchy is read); aux: tri_eta.
template <int MESH>
struct WalkReflect {
    static constexpr int SLOTS = 0;
    TvamInsertScene sc;
    struct State {
        InsDraws dr;
        TvamInsertWalk w;
    };
    __device__ __forceinline__ WalkReflect(const TvamConsts& k, const float* tri_eta)
        : sc{cn_mesh_view<MESH>(k, r3_mesh_lds), tri_eta} {}
    __device__ __forceinline__ void start(const TvamConsts& k, const TvamTiles& tp, const int32_t* idxmap,
                                          const TvamPathIndex& ix, ConeRay& r, State& st) const {
        (void)cn_ray_at<CN_NO_MESH, true>(k, tp, ix.al, ix.colc, ix.rowc,
                                          tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp), r, st.dr.rng);
        tvam_insert_start(st.w, r.o, r.d);
    }
    __device__ __forceinline__ bool next(const TvamConsts& k, ConeRay& r, State& st) const {
        return tvam_insert_next<true, MESH != CN_NO_MESH>(k, sc, true, st.dr, st.w, r.o2, r.d2, r.maxt, r.att);
    }
};

}  // namespace

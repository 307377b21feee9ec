// tvam_plan.h — struct tvam_plan and the error helpers of the extern "C" boundary, shared by
// tvam_plan.hip (construction) and tvam_calls.hip (the per-call entry points).
//
// Ownership: every device table of a plan is a TvamDevBuf member, freed with the plan.  The structs
// the kernels take by value (k, tiles, pl) hold raw pointers only, filled from those owners in one
// place, tvam_plan::bind().  What the destructor itself releases is what is not device memory: the
// ray slots' events and the bin scratch's event and pinned word.
#pragma once

#include <string>

#include "tvam_internal.h"

// the calling thread's tvam_last_error() message; return `code`
int tvam_fail(int code, const std::string& msg);
int tvam_hip_fail(hipError_t e, const char* what);

template <typename T>
int tvam_upload(TvamDevBuf<T>& b, const std::vector<T>& v) {
    const hipError_t e = b.upload(v);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, b.get() ? "hipMemcpy" : "hipMalloc");
}

#define TVAM_FROZEN_CAP (1 << 20)
#define TVAM_STRAY_CAP (1 << 22)  // stray rays per record set (more: the tile kernels use the full row lists)

// The seven sorts of plan: the create entry point a plan came through and, for tvam_plan_create, its
// projector.  Every kind but Plain runs the 3-D ray kernels (tvam_ray3d.hip).  What a kind's descriptor
// may ask for is stated once, in validate() (tvam_plan.hip); what a per-call entry refuses of a kind,
// in that entry's switch (tvam_calls.hip).
enum class TvamPlanKind {
    Plain,    // tvam_plan_create, collimated: index-matched, 'cylindrical' or 'square' vial (planar / tile kernels)
    Cone,     // tvam_plan_create, telecentric / lens: 3-D first segments behind an index-matched vial
    Traced,   // tvam_plan_create_traced: 'cylindrical' / 'square' vial traced per ray in 3-D (tvam_glass.h)
    Mesh,     // tvam_plan_create_mesh: 'custom' vial, mesh interfaces traced per ray (tvam_mesh.h)
    Double,   // tvam_plan_create_double: four tubes traced per ray, two segments (tvam_double.h)
    Inserts,  // tvam_plan_create_inserts: dielectric occluders walked per ray (tvam_insert.h)
    Reflect,  // tvam_plan_create_reflect: transmission_only = 0, the insert walk with sampled reflections
};

// runs the 3-D ray kernels (tvam_ray3d.hip), not the planar, tile and per-path kernels / walks inserts (tvam_insert.h:
// any number of segments per ray) / has TvamConsts::mesh live (a vial's or the inserts' hierarchy; Double: TvamConsts::dbl)
inline bool tvam_kind_ray3d(TvamPlanKind kind) { return kind != TvamPlanKind::Plain; }
inline bool tvam_kind_inserts(TvamPlanKind kind) { return kind == TvamPlanKind::Inserts || kind == TvamPlanKind::Reflect; }
inline bool tvam_kind_mesh(TvamPlanKind kind) { return kind == TvamPlanKind::Mesh || tvam_kind_inserts(kind); }

struct tvam_plan {
    tvam_desc desc;
    const TvamPlanKind kind;
    const int device;
    TvamConsts k{};
    TvamTiles tiles{};
    int32_t ntiles = 0;
    size_t lds_bytes = 0;
    int32_t max_rows_per_slice = 0;
    int64_t n_slots_all = 0;  // (angle, column) slots over every tile (tvam_plan_tile_stats)
    int64_t n_main_rows = 0;  // main-row list entries over every slice (0: no main-row lists)
    int64_t n_rows_all = 0;   // row list entries over every slice
    const bool empty;    // (route decisions: the constructor's)  max_depth too small for any ray to reach the medium
    const bool cyl;      // refracting (cylindrical / square) vial of a Plain plan: per-ray directions and weights
    const bool surface;  // surface-aware film (2 channels): per-path kernels cut at the target mesh
    const bool general;  // sample_time, a ratio / delta sensor or a 3-D ray kind: the general per-path kernel
    const float* vols = nullptr;  // caller's compute_volume() output (tvam_plan_set_volumes)
    TvamDevBuf<float> tgt, occ;   // target mesh (surface-aware films) and occluder triangles
    TvamDevBuf<float> ins_eta;      // dielectric occluders: eta of each insert triangle, caller order (the hierarchy: mesh_*)
    TvamDevBuf<float4> mesh_nodes;  // 'custom' vial: the hierarchy over both meshes (TvamMesh)
    TvamDevBuf<float> mesh_tris;
    TvamDevBuf<int32_t> mesh_ids;
    // device tables (TvamTiles)
    TvamDevBuf<float2> cs;
    TvamDevBuf<int32_t> slice_off, slice_rows;
    TvamDevBuf<int32_t> slice_moff, slice_mrows, row_main;  // main-row lists
    TvamDevBuf<uint32_t> slots;
    TvamDevBuf<int64_t> slot_off;
    TvamDevBuf<unsigned long long> counter;
    TvamDevBuf<float4> ang;
    // per-ray records (tvam_ray_setup_kernel), cached: regular sampling makes
    // them call-independent; otherwise they are keyed on (spp, seed).  Two slots (LRU) when memory
    // allows: an optimiser iteration renders seed i, back-projects seed i', renders seed i again
    struct RaySlot {
        TvamDevBuf<float4> f, g;
        TvamDevBuf<int2> i;
        TvamDevBuf<int64_t> frozen;  // frozen-axis rays of the ray records (tvam_frozen_kernel)
        TvamDevBuf<unsigned long long> frozen_n;
        TvamDevBuf<uint32_t> stray;  // stray rays (TvamTiles::stray_*): [cap] appended, [cap] by slice,
        TvamDevBuf<uint32_t> stray_cs;  // [2 (nz + 1)] counts / cursors, offsets
        TvamDevBuf<unsigned long long> stray_n;
        uint64_t cap = 0;  // rays f, i (and g) hold
        bool valid = false;
        uint32_t spp = 0, seed = 0;
        bool sparse = false;  // records built for a sparse active set (streams by active position)
        const void* pix = nullptr;  // ... that set (active_pixels pointer and count: the records'
        uint64_t npix = 0;          // key; tvam_plan_set_active drops them after in-place changes)
        hipEvent_t ready = nullptr;
        uint64_t used = 0;
    };
    RaySlot rs[2];
    uint64_t ray_tick = 0;
    // planar fast path (regular sampling; tvam_planar.hip)
    bool planar = false;      // planar adjoint
    bool planar_fwd = false;  // voxel-driven planar forward (straight rays only)
    int32_t planar_fz = 16, planar_az = 4;
    TvamPlanar pl{};
    TvamDevBuf<int32_t> pl_slice_off, pl_slice_rows, pl_fwd_cb, pl_rec_i;
    TvamDevBuf<float4> pl_vox, pl_fwd_ang, pl_rec_f, pl_rec_g;
    TvamDevBuf<float> pl_part;  // voxel-driven forward: partial doses of the angle parts
    TvamDevBuf<float> pl_bin;   // voxel-driven forward: slice-binned patterns
    TvamDevBuf<float4> pl_vox2;       // refracted voxel-driven forward: per-column 1/d, flags, weight
    TvamDevBuf<float4> pl_fwd_model;  // refracted voxel-driven forward: per-(tile, angle) chord-index models
    TvamDevBuf<unsigned> amax;  // ray-driven forward: per-angle max |pattern|, fixed-point scale
    TvamDevBuf<float> fscale;
    int32_t planar_rz = 4;
    TvamAdjListBufs adjl{};  // planar adjoint: slice-invariant visit lists (tvam_adjlist.hip)
    bool adjl_pending = false;  // the lists are to be built by the first adjoint call
    int adjl_parts = 1;
    TvamBinScratch bins{};  // scattering media: brick-binned forward scratch
    // sparse scratch (dense crop layout), allocated on first sparse call
    TvamDevBuf<float> dense;
    TvamDevBuf<int32_t> idxmap;
    TvamDevBuf<double> dsig_part;  // tvam_adjoint_dsigma / tvam_adjoint_dprojector: one partial per workgroup, allocated on the first call

    // the kernel structs' table pointers (k, tiles, pl) from their owners; an owner that holds
    // nothing gives nullptr.  (pl.chord and the visit lists' pl.adjl_* are set by their builders.)
    void bind() {
        k.tgt = tgt.get(), k.occ = occ.get();
        if (tvam_kind_mesh(kind))  // (else k.dbl may have k.mesh's bytes)
            k.mesh.nodes = mesh_nodes.get(), k.mesh.tris = mesh_tris.get(), k.mesh.ids = mesh_ids.get();
        tiles.cs = cs.get(), tiles.ang = ang.get();
        tiles.slice_off = slice_off.get(), tiles.slice_rows = slice_rows.get();
        tiles.slots = slots.get(), tiles.slot_off = slot_off.get();
        tiles.slice_moff = slice_moff.get(), tiles.slice_mrows = slice_mrows.get(), tiles.row_main = row_main.get();
        pl.cs = cs.get();
        pl.slice_off = pl_slice_off.get(), pl.slice_rows = pl_slice_rows.get();
        pl.vox = pl_vox.get(), pl.vox2 = pl_vox2.get();
        pl.rec_f = pl_rec_f.get(), pl.rec_i = pl_rec_i.get(), pl.rec_g = pl_rec_g.get();
        pl.fwd_ang = pl_fwd_ang.get(), pl.fwd_cb = pl_fwd_cb.get();
        pl.fwd_part = pl_part.get(), pl.fwd_bin = pl_bin.get();
        pl.fwd_model = pl_fwd_model.get();
    }
    // How a plan of (kind, descriptor) is served, decided once.  empty: two glass surfaces + the medium segment (volume.py:179,
    // :271-272; a double vial's first deposit is at loop iteration 2), index matched: entry bounce + medium segment
    tvam_plan(TvamPlanKind kind_, const tvam_desc& d, int device_)
        : desc(d), kind(kind_), device(device_),
          empty(d.max_depth < (glass(d) || kind_ == TvamPlanKind::Mesh || kind_ == TvamPlanKind::Double ? 3 : 2)),
          cyl(glass(d) && kind_ == TvamPlanKind::Plain), surface(d.film_channels == 2),
          general(!surface && (d.sample_time || d.sensor_type != TVAM_SENSOR_DDA || tvam_kind_ray3d(kind_))) {}
    static bool glass(const tvam_desc& d) { return d.vial_type == TVAM_VIAL_CYLINDRICAL || d.vial_type == TVAM_VIAL_SQUARE; }
    tvam_plan(const tvam_plan&) = delete;
    ~tvam_plan() {
        for (auto& r : rs)
            if (r.ready) (void)hipEventDestroy(r.ready);
        tvam_bin_scratch_free(bins);
    }
};

// the forward of a telecentric / lens plan: the brick bins by flag, else the plan's default
inline bool tvam_cone_binned(const tvam_plan* p) {
    const int fl = p->desc.flags;
    return (fl & TVAM_FLAG_BIN_FIRST) || (!(fl & TVAM_FLAG_SCATTER_ATOMIC) && TVAM_CONE_BINNED_DEFAULT);
}

// the walk of a 3-D ray plan (tvam_kind_ray3d; tvam_ray3d.h)
inline int tvam_plan_walk(const tvam_plan* p) {
    switch (p->kind) {
    case TvamPlanKind::Plain: case TvamPlanKind::Cone: case TvamPlanKind::Traced: case TvamPlanKind::Mesh: break;
    case TvamPlanKind::Double: return TVAM_WALK_DOUBLE;
    case TvamPlanKind::Inserts: return TVAM_WALK_INSERT;
    case TvamPlanKind::Reflect: return TVAM_WALK_REFLECT;
    }
    return TVAM_WALK_ONE;
}

// one medium segment as the host segment dumpers write it: o2[3], maxt, d2[3], att
inline void seg_row(float* sg, const float o2[3], const float d2[3], float maxt, float att) {
    sg[0] = o2[0], sg[1] = o2[1], sg[2] = o2[2], sg[3] = maxt;
    sg[4] = d2[0], sg[5] = d2[1], sg[6] = d2[2], sg[7] = att;
}

// rays of the shard at one sample per pixel: a dense active set's length
inline uint64_t shard_pixels(const tvam_plan* p) {
    return (uint64_t)(p->k.a1 - p->k.a0) * p->desc.crop_y * p->desc.crop_x;
}

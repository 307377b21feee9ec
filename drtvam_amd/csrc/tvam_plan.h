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

struct tvam_plan {
    tvam_desc desc;
    int device;
    TvamConsts k;
    TvamTiles tiles;
    int32_t ntiles;
    size_t lds_bytes;
    int32_t max_rows_per_slice;
    int64_t n_slots_all = 0;  // (angle, column) slots over every tile (tvam_plan_tile_stats)
    int64_t n_main_rows = 0;  // main-row list entries over every slice (0: no main-row lists)
    int64_t n_rows_all = 0;   // row list entries over every slice
    bool empty;  // max_depth too small for any ray to reach the medium
    bool cyl;    // refracting (cylindrical / square) vial: per-ray directions and weights
    bool surface = false;    // surface-aware film (2 channels): per-path kernels cut at the target mesh
    bool general = false;    // sample_time or a ratio / delta sensor: the general per-path kernel
    bool cone = false;       // telecentric / lens projector: 3-D first segments (tvam_ray3d.hip); implies general
    bool mesh = false;       // 'custom' vial: mesh interfaces traced per ray (tvam_mesh.h); implies cone
    const float* vols = nullptr;  // caller's compute_volume() output (tvam_plan_set_volumes)
    TvamDevBuf<float> tgt, occ;   // target mesh (surface-aware films) and occluder triangles
    bool dbl = false;        // 'double_cylindrical' vial: four tubes traced per ray, two segments (tvam_double.h); implies cone
    bool traced = false;     // 'cylindrical' / 'square' vial traced per ray in 3-D (tvam_plan_create_traced, tvam_glass.h); implies cone
    bool ins = false;        // dielectric occluders walked per ray (tvam_plan_create_inserts, tvam_insert.h); implies cone
    bool refl = false;       // transmission_only = 0 (tvam_plan_create_reflect): the insert walk with sampled reflections; implies ins
    TvamDevBuf<float> ins_eta;      // ... eta of each insert triangle, caller order (the hierarchy: mesh_*)
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
    TvamAdjListBufs adjl;  // planar adjoint: slice-invariant visit lists (tvam_adjlist.hip)
    bool adjl_pending = false;  // the lists are to be built by the first adjoint call
    int adjl_parts = 1;
    TvamBinScratch bins;  // scattering media: brick-binned forward scratch
    // sparse scratch (dense crop layout), allocated on first sparse call
    TvamDevBuf<float> dense;
    TvamDevBuf<int32_t> idxmap;
    TvamDevBuf<double> dsig_part;  // tvam_adjoint_dsigma / tvam_adjoint_dprojector: one partial per workgroup, allocated on the first call

    // the kernel structs' table pointers (k, tiles, pl) from their owners; an owner that holds
    // nothing gives nullptr.  (pl.chord and the visit lists' pl.adjl_* are set by their builders.)
    void bind() {
        k.tgt = tgt.get(), k.occ = occ.get();
        if (!dbl)  // (k.dbl shares k.mesh's bytes)
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
    tvam_plan() = default;
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

// the walk of a 3-D ray plan (p->cone; tvam_ray3d.h)
inline int tvam_plan_walk(const tvam_plan* p) {
    return p->refl ? TVAM_WALK_REFLECT : p->ins ? TVAM_WALK_INSERT : (p->dbl ? TVAM_WALK_DOUBLE : TVAM_WALK_ONE);
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

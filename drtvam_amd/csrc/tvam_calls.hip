// tvam_calls.hip — the per-call entry points of a plan (include/tvam.h): forward, adjoint, visit
// count, ray export, Radon and corner filters, volumes, discretize and the plan's statistics.
// Caller buffers are never allocated or copied here on the hot path; only the sparse active-set
// path uses a lazily allocated dense scratch, and the per-ray kernels their cached ray records.
#include "tvam_plan.h"

#include "tvam_dproj.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using K = TvamPlanKind;

// tvam_scatter_binned found brick walks that disagree with the record writer's counts
static int bin_mismatch_fail(tvam_plan* p) {
    uint32_t bad = 0;
    if (p->bins.bad.get()) (void)hipMemcpy(&bad, p->bins.bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost);
    return tvam_fail(TVAM_ERR_HIP, "brick bins: " + std::to_string(bad) +
                                  " scattered segments' brick walks disagree with their closed-form brick counts "
                                  "(entries would be lost); rerun with TVAM_FLAG_SCATTER_ATOMIC");
}

// ray weight inv_pdf / n_samples * print_time over n_all pixels (projector.py:164-165, :187; common.py:111)
static float ray_weight(const tvam_desc& d, uint64_t n_all, uint32_t spp) {
    float area = d.pixel_size_x * d.pixel_size_y * (float)n_all;
    float w = area / (float)(n_all * (uint64_t)spp);
    return w * d.print_time;
}

// per-call constants: spp forced to 1 under regular sampling (common.py:49-51) and the ray weight
static int call_setup(tvam_plan* p, uint64_t n_active, const uint32_t* active_pixels, uint32_t& spp, TvamConsts& k) {
    const tvam_desc& d = p->desc;
    if (!active_pixels && n_active != shard_pixels(p))
        return tvam_fail(TVAM_ERR_INVALID, "active_data and active_pixels must have the same length.");  // projector.py:137-138
    if (d.regular_sampling) spp = 1;
    if (spp == 0) spp = 4;  // optimize.py:96
    if ((d.active_total > 0 ? (uint64_t)d.active_total : n_active) * (uint64_t)spp > (1ull << 32))
        return tvam_fail(TVAM_ERR_TOO_LARGE,
                    "The total number of Monte Carlo samples required by this rendering task exceeds 2^32 = "
                    "4294967296. Please use fewer samples per pixel or render using multiple passes.");  // common.py:60-65
    k = p->k;
    // inv_pdf / n_samples over the whole active set (projector.py:164-165, :187): a shard's
    // call carries its own n_active, the reference's len(active_data) is desc.active_total
    const uint64_t n_all = d.active_total > 0 ? (uint64_t)d.active_total : n_active;
    float w = ray_weight(d, n_all, spp);
    float ss = d.albedo * d.sigma_t;
    float sa_st = d.sigma_t != 0.0f ? (float)(((double)d.sigma_t - (double)ss) / (double)d.sigma_t) : 0.0f;
    k.wscale = w * sa_st;
    hipError_t e = hipSetDevice(p->device);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipSetDevice");
    return 0;
}

// the sparse scratch, both buffers or (after a failure) neither
static int ensure_dense(tvam_plan* p) {
    const uint64_t n = shard_pixels(p);
    if (p->dense.get() && p->idxmap.get()) return 0;
    hipError_t e;
    if ((e = p->dense.alloc(n)) != hipSuccess || (e = p->idxmap.alloc(n)) != hipSuccess) {
        (void)p->dense.reset();
        return tvam_hip_fail(e, "hipMalloc");
    }
    return 0;
}

// Make the per-ray records of (spp, seed) available on `stream`.  The
// buffer grows on demand (first call with a larger spp); the pre-pass runs
// only when the cached records do not match the call.
static int ensure_rays(tvam_plan* p, const TvamConsts& k, TvamTiles& t, const int32_t* idxmap, hipStream_t stream,
                       const uint32_t* active_pixels = nullptr, uint64_t n_active = 0) {
    const uint64_t n = (uint64_t)(k.a1 - k.a0) * k.crop_y * k.crop_x * t.spp;
    if (n > 0xFFFFFFFFull) {  // stray lists hold 32-bit record indices: every slice walks its full row list
        t.slice_moff = nullptr;
        t.row_main = nullptr;
    }
    hipError_t e;
    auto bind = [&](tvam_plan::RaySlot& r) {
        t.ray_f = r.f.get();
        t.ray_i = r.i.get();
        t.ray_g = r.g.get();
        t.frozen = r.frozen.get();
        t.frozen_n = r.frozen_n.get();
        t.frozen_cap = TVAM_FROZEN_CAP;
        if (t.slice_moff) {
            t.stray_idx = r.stray.get();
            t.stray_list = r.stray.get() + TVAM_STRAY_CAP;
            t.stray_cnt = r.stray_cs.get();
            t.stray_off = r.stray_cs.get() + (k.nz + 1);
            t.stray_n = r.stray_n.get();
            t.stray_cap = TVAM_STRAY_CAP;
        }
        r.used = ++p->ray_tick;
    };
    // jittered records of a sparse active set depend on the set (sampler streams by active
    // position): reused for the same set (pointer and count; the slice ranges of one forward,
    // the line-search forward of the same seed), like a dense set's for the same seed and spp
    auto same_set = [&](const tvam_plan::RaySlot& r) {
        return idxmap ? (r.sparse && r.pix == (const void*)active_pixels && r.npix == n_active) : !r.sparse;
    };
    for (auto& r : p->rs)
        if (r.valid && r.spp == t.spp && (k.regular || (r.seed == t.seed && same_set(r)))) {
            bind(r);
            e = hipStreamWaitEvent(stream, r.ready, 0);
            return e == hipSuccess ? 0 : tvam_hip_fail(e, "hipStreamWaitEvent");
        }
    const size_t per_ray = sizeof(float4) + sizeof(int2) + (p->cyl ? sizeof(float4) : 0);
    auto alloc = [&](tvam_plan::RaySlot& r) -> int {
        const size_t n1 = (size_t)std::max<uint64_t>(n, 1);
        r.cap = 0;
        r.valid = false;
        (void)r.f.reset();  // all three released before the first is allocated anew
        (void)r.i.reset();
        (void)r.g.reset();
        if ((e = r.f.alloc(n1)) != hipSuccess || (e = r.i.alloc(n1)) != hipSuccess ||
            (p->cyl && (e = r.g.alloc(n1)) != hipSuccess))
            return tvam_hip_fail(e, "hipMalloc (ray records)");
        if ((e = r.frozen.grow(TVAM_FROZEN_CAP)) != hipSuccess || (e = r.frozen_n.grow(1)) != hipSuccess)
            return tvam_hip_fail(e, "hipMalloc (frozen-ray list)");
        if (t.slice_moff &&
            ((e = r.stray.grow((size_t)2 * TVAM_STRAY_CAP)) != hipSuccess ||
             (e = r.stray_cs.grow((size_t)2 * (k.nz + 1))) != hipSuccess || (e = r.stray_n.grow(1)) != hipSuccess))
            return tvam_hip_fail(e, "hipMalloc (stray-ray lists)");
        r.cap = n;
        return 0;
    };
    // the slot to fill: the first one; a second only for jittered records and while a quarter
    // of the device memory stays free after it; else the least recently used one that holds n
    tvam_plan::RaySlot* r = &p->rs[0];
    if (p->rs[0].cap > 0) {
        bool second = p->rs[1].cap >= n;
        if (!second && !k.regular && p->rs[1].cap == 0) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > (size_t)n * per_ray + tot / 4 + ((size_t)16 << 20)) {
                int rc;
                if ((rc = alloc(p->rs[1]))) return rc;
                second = true;
            }
        }
        if (second && (p->rs[1].used < p->rs[0].used || !p->rs[1].valid)) r = &p->rs[1];
    }
    if (r->cap < n) {
        int rc;
        if ((rc = alloc(*r))) return rc;
    }
    bind(*r);
    if ((e = hipMemsetAsync(t.frozen_n, 0, sizeof(unsigned long long), stream)) != hipSuccess)
        return tvam_hip_fail(e, "hipMemsetAsync");
    if (t.slice_moff && ((e = hipMemsetAsync(t.stray_n, 0, sizeof(unsigned long long), stream)) != hipSuccess ||
                         (e = hipMemsetAsync(t.stray_cnt, 0, (size_t)(k.nz + 1) * sizeof(uint32_t), stream)) != hipSuccess))
        return tvam_hip_fail(e, "hipMemsetAsync");
    if ((e = tvam_launch_ray_setup(k, t, r->f.get(), r->i.get(), r->g.get(), idxmap, stream)) != hipSuccess)
        return tvam_hip_fail(e, "ray setup launch");
    if (t.slice_moff && (e = tvam_launch_stray_lists(k, t, stream)) != hipSuccess)
        return tvam_hip_fail(e, "stray list launch");
    if ((e = hipEventRecord(r->ready, stream)) != hipSuccess) return tvam_hip_fail(e, "hipEventRecord");
    r->valid = true;
    r->spp = t.spp;
    r->seed = t.seed;
    r->sparse = idxmap != nullptr;
    r->pix = idxmap ? (const void*)active_pixels : nullptr;
    r->npix = idxmap ? n_active : 0;
    return 0;
}

extern "C" int tvam_plan_set_active(tvam_plan* p, int64_t active_base, int64_t active_total) {
    if (!p) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (active_base < 0 || active_total < 0) return tvam_fail(TVAM_ERR_INVALID, "active_base / active_total must be >= 0");
    p->desc.active_base = active_base;
    p->desc.active_total = active_total;
    p->k.stream_base = active_base;
    for (auto& r : p->rs) r.valid = false;
    return 0;
}

// Slice granularity of tvam_forward_slices: the voxel-driven forward's Z, 1 for the per-ray tile
// kernels, 0 when the plan's forward cannot be split by slices (scattered paths and per-path
// kernels add into every slice; the ray-driven planar forward).
static int fwd_chunk(const tvam_plan* p) {
    if (p->surface || p->general || p->desc.albedo != 0.0f) return 0;
    if (p->planar_fwd) return p->planar_fz;
    return p->planar ? 0 : 1;
}

extern "C" int tvam_plan_fwd_chunk(const tvam_plan* p) { return p ? fwd_chunk(p) : 0; }

// The TvamTiles of a call: the plan's tables with the call's spp and seed.
static TvamTiles call_tiles(const tvam_plan* p, uint32_t spp, uint32_t seed) {
    TvamTiles t = p->tiles;
    t.spp = spp;
    t.seed = seed;
    return t;
}

// A sparse active set (active_pixels): the dense (angle,row,col) -> active index map (the adjoint
// kernels add each ray's gradient straight into grad_active[active index]); with active_data (the
// forward) also the data scattered into the zeroed dense patterns, *pat.  A dense set binds nothing.
static int bind_active(tvam_plan* p, const TvamConsts& k, const float* active_data, const uint32_t* active_pixels,
                       uint64_t n_active, hipStream_t stream, const float** pat, const int32_t** idxmap) {
    if (!active_pixels) return 0;
    int rc;
    hipError_t e = hipSuccess;
    if ((rc = ensure_dense(p))) return rc;
    const size_t n = p->dense.capacity();
    if ((active_data && (e = hipMemsetAsync(p->dense.get(), 0, n * sizeof(float), stream)) != hipSuccess) ||
        (e = hipMemsetAsync(p->idxmap.get(), 0xff, n * sizeof(int32_t), stream)) != hipSuccess)
        return tvam_hip_fail(e, "hipMemsetAsync");
    if ((e = tvam_launch_scatter(k, active_data, active_pixels, n_active, p->dense.get(), p->idxmap.get(), stream)) !=
        hipSuccess)
        return tvam_hip_fail(e, "scatter launch");
    if (active_data) *pat = p->dense.get();
    *idxmap = p->idxmap.get();
    return 0;
}

// A 3-D ray plan's per-ray kernels (tvam_ray3d.hip) over the plan's walk.
static hipError_t launch_ray3d(int mode, const tvam_plan* p, const TvamConsts& k, const TvamTiles& t, const float* pat,
                               const int32_t* idxmap, const float* gin, float* out, unsigned long long* counter,
                               hipStream_t stream) {
    return tvam_launch_ray3d(mode, tvam_plan_walk(p), k, t, p->ins_eta.get(), pat, idxmap, gin, out, counter, stream);
}

// Segments of a call that cross slices -- the scattered segments after each path's first medium
// segment (walk = TVAM_WALK_NONE), or the 3-D segments of a 3-D ray plan's forward (its walk): through
// the brick bins when `binned`, else (or on a grid beyond the packed records' range) the per-ray
// atomics / gathers.
static int scattered_segments(int mode, tvam_plan* p, const TvamConsts& k, const TvamTiles& t, const float* pat,
                              const int32_t* idxmap, const float* gin, float* out, hipStream_t stream, bool binned,
                              int walk, const char* what) {
    hipError_t e = hipErrorNotSupported;
    if (mode == TVAM_MODE_FWD) p->bins.acc_float = tvam_knob("TVAM_BIN_FLOAT", 0);
    if (binned)
        e = tvam_scatter_binned(mode, k, t, pat, idxmap, gin, out, p->bins, stream, walk);
    else
        for (auto& v : p->bins.st) v = 0;  // nothing binned
    if (e == hipErrorNotSupported)
        e = walk == TVAM_WALK_NONE ? tvam_launch_scatter_paths(mode, k, t, pat, idxmap, gin, out, nullptr, stream)
                                   : launch_ray3d(mode, p, k, t, pat, idxmap, gin, out, nullptr, stream);
    if (e == hipErrorIllegalState) return bin_mismatch_fail(p);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, what);
}

// TVAM_FLAG_FWD_STATS: the forward's counter (tvam_plan_stats), zeroed on `stream`; else nullptr
static int fwd_stats_counter(tvam_plan* p, hipStream_t stream, unsigned long long** counter) {
    *counter = nullptr;
    if (!(p->desc.flags & TVAM_FLAG_FWD_STATS)) return 0;
    const hipError_t e = hipMemsetAsync(p->counter.get(), 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemsetAsync");
    *counter = p->counter.get();
    return 0;
}

static int forward_impl(tvam_plan* p, const float* active_data, const uint32_t* active_pixels, uint64_t n_active,
                        uint32_t spp, uint32_t seed, float* dose, void* stream_, int zb, int ze);

extern "C" int tvam_forward(tvam_plan* p, const float* active_data, const uint32_t* active_pixels, uint64_t n_active,
                            uint32_t spp, uint32_t seed, float* dose, void* stream_) {
    return forward_impl(p, active_data, active_pixels, n_active, spp, seed, dose, stream_, 0, -1);
}

// What tvam_forward_slices and tvam_adjoint_slices (`who`) refuse by name (the other 3-D ray kinds: the entries' own checks)
static int slices_refuse(const tvam_plan* p, const char* who) {
    switch (p->kind) {
    case K::Reflect: return tvam_fail(TVAM_ERR_UNSUPPORTED, std::string(who) + ": reflected paths (transmission_only = 0) take rays out of their slice (no slice ranges)");
    case K::Inserts: return tvam_fail(TVAM_ERR_UNSUPPORTED, std::string(who) + ": dielectric occluders take rays out of their slice (no slice ranges)");
    case K::Plain: case K::Cone: case K::Traced: case K::Mesh: case K::Double: break;
    }
    return 0;
}

extern "C" int tvam_forward_slices(tvam_plan* p, const float* active_data, const uint32_t* active_pixels,
                                   uint64_t n_active, uint32_t spp, uint32_t seed, int32_t z_begin, int32_t z_end,
                                   float* dose, void* stream) {
    if (!p) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (const int rc = slices_refuse(p, "tvam_forward_slices")) return rc;
    const int ch = fwd_chunk(p), nz = p->k.nz;
    if (ch == 0) return tvam_fail(TVAM_ERR_UNSUPPORTED, "this plan's forward cannot be split into slice ranges");
    if (z_begin < 0 || z_end > nz || z_begin >= z_end || z_begin % ch != 0 || (z_end % ch != 0 && z_end != nz))
        return tvam_fail(TVAM_ERR_INVALID, "slice range must lie in the film and on the forward's slice chunks");
    return forward_impl(p, active_data, active_pixels, n_active, spp, seed, dose, stream, z_begin, z_end);
}

static int forward_impl(tvam_plan* p, const float* active_data, const uint32_t* active_pixels, uint64_t n_active,
                        uint32_t spp, uint32_t seed, float* dose, void* stream_, int zb, int ze) {
    if (!p || !dose || (!active_data && n_active)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    int rc = call_setup(p, n_active, active_pixels, spp, k);
    if (rc) return rc;
    const TvamConsts& kc = k;
    size_t V = (size_t)kc.res[0] * kc.res[1] * kc.nz * (p->surface ? 2 : 1);
    const bool ranged = ze >= 0;  // tvam_forward_slices: only slices [zb, ze) of dose are written
    hipError_t e;
    if (p->surface && !p->vols) return tvam_fail(TVAM_ERR_INVALID, "surface-aware film: call tvam_plan_set_volumes first");
    if (p->empty || n_active == 0 || p->surface || p->general) {
        const size_t plane = (size_t)kc.res[0] * kc.res[1];
        e = ranged ? hipMemsetAsync(dose + (size_t)zb * plane, 0, (size_t)(ze - zb) * plane * sizeof(float), stream)
                   : hipMemsetAsync(dose, 0, V * sizeof(float), stream);
        if (e != hipSuccess) return tvam_hip_fail(e, "hipMemsetAsync");
        if (p->empty || n_active == 0) return 0;
    }
    const float* pat = active_data;
    const int32_t* idxmap = nullptr;
    if ((rc = bind_active(p, kc, active_data, active_pixels, n_active, stream, &pat, &idxmap))) return rc;
    if (p->general) {
        TvamTiles t = call_tiles(p, spp, seed);
        if (tvam_kind_ray3d(p->kind)) {  // a record slot per possible segment; any number of them: the per-ray atomics alone
            const int walk = tvam_plan_walk(p);
            return scattered_segments(TVAM_MODE_FWD, p, kc, t, pat, idxmap, nullptr, dose, stream,
                                      tvam_walk_slots(walk) > 0 && tvam_cone_binned(p), walk,
                                      p->kind == K::Reflect   ? "reflected-path forward launch"
                                      : p->kind == K::Inserts ? "dielectric-occluder forward launch"
                                      : p->kind == K::Double  ? "double-vial forward launch"
                                                                         : "projector-ray forward launch");
        }
        e = tvam_launch_general_paths(TVAM_MODE_FWD, kc, t, pat, idxmap, nullptr, dose, nullptr, stream);
        return e == hipSuccess ? 0 : tvam_hip_fail(e, "path forward launch");
    }
    if (p->surface) {
        TvamTiles t = call_tiles(p, spp, seed);
        e = tvam_launch_surface_paths(TVAM_MODE_FWD, kc, t, pat, idxmap, nullptr, p->vols, dose, nullptr, stream);
        if (e == hipSuccess) e = tvam_launch_scale_volumes((int64_t)V, p->vols, dose, stream);
        return e == hipSuccess ? 0 : tvam_hip_fail(e, "surface-aware forward launch");
    }
    unsigned long long* stats = nullptr;
    if (p->planar_fwd) {
        if ((rc = fwd_stats_counter(p, stream, &stats))) return rc;
        TvamPlanar pl = p->pl;
        if (ranged) {
            pl.fwd_zc0 = zb / p->planar_fz;
            pl.fwd_nzc = (ze - zb + p->planar_fz - 1) / p->planar_fz;
        }
        e = tvam_launch_fwd_planar(kc, pl, p->planar_fz, pat, dose, stream);
        if (e != hipSuccess) return tvam_hip_fail(e, "planar forward launch");
    } else if (p->planar) {
        e = tvam_launch_fwd_rays_planar(kc, p->pl, p->tiles, p->planar_rz, pat, p->amax.get(), p->fscale.get(), dose,
                                        stream);
        if (e != hipSuccess) return tvam_hip_fail(e, "planar ray forward launch");
    } else {
        TvamTiles t = call_tiles(p, spp, seed);
        if (ranged) {
            t.kz0 = zb;
            t.kz1 = ze;
        }
        if ((rc = ensure_rays(p, kc, t, idxmap, stream, active_pixels, n_active))) return rc;
        if ((rc = fwd_stats_counter(p, stream, &stats))) return rc;
        tvam_kt_begin(stream, TVAM_KT_TILE);
        e = tvam_launch_tiles(TVAM_MODE_FWD, kc, t, p->lds_bytes, pat, idxmap, nullptr, dose, stats, stream);
        tvam_kt_end(stream, TVAM_KT_TILE);
        if (e == hipSuccess) e = tvam_launch_frozen(TVAM_MODE_FWD, kc, t, pat, idxmap, nullptr, dose, nullptr, stream);
        if (e != hipSuccess) return tvam_hip_fail(e, "forward launch");
    }
    if (p->desc.albedo != 0.0f) {  // scattered segments (after each path's first medium segment)
        return scattered_segments(TVAM_MODE_FWD, p, kc, call_tiles(p, spp, seed), pat, idxmap, nullptr, dose, stream,
                                  !(p->desc.flags & TVAM_FLAG_SCATTER_ATOMIC), TVAM_WALK_NONE, "scatter forward launch");
    }
    return 0;
}

// The planar adjoint of film slices [z_begin, z_end) alone, into the DMD rows [row_begin, row_end) of every
// angle of grad_active (dense crop order; those rows zeroed first, the others untouched): the caller's rows
// are exactly the rows whose rays lie in those slices (tvam_row_slices), so the rows hold their whole
// gradient.  Regular-sampling planar plans of a dense set; slices on the adjoint's Z-slice chunks.
// The planar adjoint's visit lists, built at the plan's first adjoint call when they fit in a
// quarter of the free device memory (else the tile adjoint serves).  16 slices per workgroup where
// the tile's 4 planes fit in LDS, else 8 (the weights are the same; the adjoint's chunk reported
// before the build, max(8, adjl_z), stays a multiple of the one the kernel then runs).
// Slice granularity of tvam_adjoint_slices: the list adjoint's slices per workgroup while the
// lists serve or are still to be built, else the tile adjoint's.
static int adj_chunk(const tvam_plan* p) {
    return p->pl.adjl_ngroups > 0 || p->adjl_pending ? std::max(p->planar_az, p->pl.adjl_z) : p->planar_az;
}

static int ensure_adj_lists(tvam_plan* p) {
    if (!p->adjl_pending) return 0;
    p->adjl_pending = false;
    size_t fr = 0, tot = 0;
    hipError_t e = hipMemGetInfo(&fr, &tot);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemGetInfo");
    e = tvam_build_adj_lists(p->k, p->pl, p->tiles, p->adjl_parts, fr / 4, p->adjl, nullptr);
    if (e == hipSuccess && p->pl.adjl_z == 16 && tvam_adjl_lds(p->pl, p->tiles, 16) > 160 * 1024) p->pl.adjl_z = 8;
    if (e == hipSuccess && tvam_adjl_lds(p->pl, p->tiles, p->pl.adjl_z) > 160 * 1024) e = hipErrorOutOfMemory;
    if (e != hipSuccess) {
        p->adjl = TvamAdjListBufs{};
        p->pl.adjl_ngroups = 0;
        if (e != hipErrorOutOfMemory) return tvam_hip_fail(e, "adjoint visit lists");
        (void)hipGetLastError();
    }
    return 0;
}

extern "C" int tvam_adjoint_slices(tvam_plan* p, const float* grad_dose, uint64_t n_active, int32_t z_begin,
                                   int32_t z_end, int32_t row_begin, int32_t row_end, float* grad_active,
                                   void* stream_) {
    if (!p || !grad_dose || !grad_active) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (const int rc = slices_refuse(p, "tvam_adjoint_slices")) return rc;
    if (!p->planar || p->general || p->surface || p->desc.albedo != 0.0f || p->empty)
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_adjoint_slices: planar plans only");
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    uint32_t spp = 1;
    int rc = call_setup(p, n_active, nullptr, spp, k);
    if (rc) return rc;
    const int Z = adj_chunk(p), nz = k.nz;
    if ((rc = ensure_adj_lists(p))) return rc;
    const int64_t R = k.crop_y, C = k.crop_x, A = (int64_t)p->tiles.n_shard;
    if (z_begin < 0 || z_end > nz || z_begin >= z_end || z_begin % Z != 0 || (z_end % Z != 0 && z_end != nz) ||
        row_begin < 0 || row_end > R || row_begin > row_end || (int64_t)n_active != A * R * C)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_adjoint_slices: slices on the adjoint's chunks, rows in the crop, dense set");
    hipError_t e = hipSuccess;
    if (row_end > row_begin)
        e = hipMemset2DAsync(grad_active + (size_t)row_begin * C, (size_t)(R * C) * sizeof(float), 0,
                             (size_t)(row_end - row_begin) * C * sizeof(float), (size_t)A, stream);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemset2DAsync");
    TvamPlanar pl = p->pl;
    pl.adj_zc0 = z_begin / p->planar_az;  // (in the tile adjoint's chunks; the list adjoint converts)
    pl.adj_nzc = (z_end - z_begin + p->planar_az - 1) / p->planar_az;
    e = tvam_launch_adj_planar(k, pl, p->tiles, p->planar_az, nullptr, grad_dose, grad_active, stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "planar adjoint launch");
}

extern "C" int tvam_plan_adj_chunk(const tvam_plan* p) {
    if (!p || !p->planar || p->general || p->surface || p->desc.albedo != 0.0f) return 0;
    return adj_chunk(p);
}

extern "C" int tvam_adjoint(tvam_plan* p, const float* grad_dose, const uint32_t* active_pixels, uint64_t n_active,
                            uint32_t spp, uint32_t seed, float* grad_active, void* stream_) {
    if (!p || !grad_dose || (!grad_active && n_active)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    int rc = call_setup(p, n_active, active_pixels, spp, k);
    if (rc) return rc;
    hipError_t e;
    if (n_active == 0) return 0;
    const int32_t* idxmap = nullptr;
    if ((rc = bind_active(p, k, nullptr, active_pixels, n_active, stream, nullptr, &idxmap))) return rc;
    if ((rc = ensure_adj_lists(p))) return rc;
    if ((e = hipMemsetAsync(grad_active, 0, n_active * sizeof(float), stream)) != hipSuccess)
        return tvam_hip_fail(e, "hipMemsetAsync");
    if (p->general) {
        if (p->empty) return 0;
        TvamTiles t = call_tiles(p, spp, seed);
        e = tvam_kind_ray3d(p->kind)
                ? launch_ray3d(TVAM_MODE_ADJ, p, k, t, nullptr, idxmap, grad_dose, grad_active, nullptr, stream)
                : tvam_launch_general_paths(TVAM_MODE_ADJ, k, t, nullptr, idxmap, grad_dose, grad_active, nullptr, stream);
        return e == hipSuccess ? 0 : tvam_hip_fail(e, "path adjoint launch");
    }
    if (p->surface) {
        if (!p->vols) return tvam_fail(TVAM_ERR_INVALID, "surface-aware film: call tvam_plan_set_volumes first");
        if (p->empty) return 0;
        TvamTiles t = call_tiles(p, spp, seed);
        e = tvam_launch_surface_paths(TVAM_MODE_ADJ, k, t, nullptr, idxmap, grad_dose, p->vols, grad_active, nullptr,
                                      stream);
        return e == hipSuccess ? 0 : tvam_hip_fail(e, "surface-aware adjoint launch");
    }
    if (p->planar) {
        e = tvam_launch_adj_planar(k, p->pl, p->tiles, p->planar_az, idxmap, grad_dose, grad_active, stream);
        if (e != hipSuccess) return tvam_hip_fail(e, "planar adjoint launch");
    } else if (!p->empty) {
        TvamTiles t = call_tiles(p, spp, seed);
        if ((rc = ensure_rays(p, k, t, idxmap, stream, active_pixels, n_active))) return rc;
        e = tvam_launch_tiles(TVAM_MODE_ADJ, k, t, p->lds_bytes, nullptr, idxmap, grad_dose, grad_active, nullptr,
                              stream);
        if (e == hipSuccess)
            e = tvam_launch_frozen(TVAM_MODE_ADJ, k, t, nullptr, idxmap, grad_dose, grad_active, nullptr, stream);
        if (e != hipSuccess) return tvam_hip_fail(e, "adjoint launch");
    }
    if (p->desc.albedo != 0.0f && !p->empty) {
        return scattered_segments(TVAM_MODE_ADJ, p, k, call_tiles(p, spp, seed), nullptr, idxmap, grad_dose, grad_active,
                                  stream, !(p->desc.flags & TVAM_FLAG_SCATTER_ATOMIC), TVAM_WALK_NONE,
                                  "scatter adjoint launch");
    }
    return 0;
}

// Extinction derivatives (tvam_dsigma.hip).  What both entries refuse, from the descriptor and the
// plan's kind alone: no device call, nothing allocated.
static int dsigma_refuse(const tvam_plan* p, const char* who) {
    const tvam_desc& d = p->desc;
    const char* why = nullptr;
    if (d.albedo > 0.0f) why = "albedo > 0 (the free-flight terms of a scattering medium are not built)";
    else if (d.sensor_type != TVAM_SENSOR_DDA) why = "the 'ratio' / 'delta' sensors are not differentiated";
    else if (p->surface) why = "a surface-aware (two-channel) film is not differentiated";
    else if (p->k.z0 != 0 || p->k.nz != p->k.res[2]) why = "a film slab is not differentiated (render the whole film)";
    else if (d.sample_time) why = "sample_time is not differentiated";
    else
        switch (p->kind) {
        case K::Double: why = "a 'double_cylindrical' plan is not differentiated (its second segment starts at the first one's path length)"; break;
        case K::Reflect: why = "a plan with reflected paths (transmission_only = 0) is not differentiated (its sampled branches do not depend smoothly on the extinction's path)"; break;
        case K::Inserts: why = "a plan with dielectric occluders is not differentiated (its later segments start at the earlier ones' path length)"; break;
        case K::Plain: case K::Cone: case K::Traced: case K::Mesh: break;  // one medium segment per ray: differentiated
        }
    return why ? tvam_fail(TVAM_ERR_UNSUPPORTED, std::string(who) + ": " + why) : 0;
}

extern "C" int tvam_forward_dsigma(tvam_plan* p, const float* active_data, const uint32_t* active_pixels,
                                   uint64_t n_active, uint32_t spp, uint32_t seed, float* tangent, void* stream_) {
    if (!p || !tangent || (!active_data && n_active)) return tvam_fail(TVAM_ERR_INVALID, "tvam_forward_dsigma: null argument");
    int rc = dsigma_refuse(p, "tvam_forward_dsigma");
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    if ((rc = call_setup(p, n_active, active_pixels, spp, k))) return rc;
    const size_t V = (size_t)k.res[0] * k.res[1] * k.nz;
    hipError_t e = hipMemsetAsync(tangent, 0, V * sizeof(float), stream);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemsetAsync");
    if (p->empty || n_active == 0) return 0;
    const float* pat = active_data;
    const int32_t* idxmap = nullptr;
    if ((rc = bind_active(p, k, active_data, active_pixels, n_active, stream, &pat, &idxmap))) return rc;
    e = tvam_launch_dsigma(TVAM_MODE_FWD, tvam_kind_ray3d(p->kind), k, call_tiles(p, spp, seed), pat, idxmap, nullptr, tangent, nullptr,
                           nullptr, stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "extinction tangent launch");
}

extern "C" int tvam_adjoint_dsigma(tvam_plan* p, const float* active_data, const float* grad_dose,
                                   const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                                   double* g_sigma, void* stream_) {
    if (!p || !grad_dose || !g_sigma || (!active_data && n_active))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_adjoint_dsigma: null argument");
    int rc = dsigma_refuse(p, "tvam_adjoint_dsigma");
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    if ((rc = call_setup(p, n_active, active_pixels, spp, k))) return rc;
    hipError_t e;
    if (p->empty || n_active == 0) {
        e = hipMemsetAsync(g_sigma, 0, sizeof(double), stream);
        return e == hipSuccess ? 0 : tvam_hip_fail(e, "hipMemsetAsync");
    }
    const float* pat = active_data;
    const int32_t* idxmap = nullptr;
    if ((rc = bind_active(p, k, active_data, active_pixels, n_active, stream, &pat, &idxmap))) return rc;
    const TvamTiles t = call_tiles(p, spp, seed);
    // (the grid, and with it the order of the sum, depends on the ray count alone)
    if ((e = p->dsig_part.grow(tvam_dsigma_grid((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp))) != hipSuccess)
        return tvam_hip_fail(e, "hipMalloc (extinction partials)");
    e = tvam_launch_dsigma(TVAM_MODE_ADJ, tvam_kind_ray3d(p->kind), k, t, pat, idxmap, grad_dose, nullptr, p->dsig_part.get(), g_sigma,
                           stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "extinction gradient launch");
}

// Projector derivatives (tvam_dproj.hip).  What both entries refuse, from the descriptor and the
// plan's kind alone: no device call, nothing allocated.
static int dproj_check(const tvam_plan* p, int32_t param, const char* who) {
    const tvam_desc& d = p->desc;
    const char* why = nullptr;
    std::string vial;
    switch (p->kind) {  // index-matched vials only
    case K::Reflect: why = "a plan with reflected paths (transmission_only = 0)"; break;
    case K::Inserts: why = "a plan with dielectric occluders (inserts)"; break;
    case K::Double: why = "a 'double_cylindrical' vial"; break;
    case K::Mesh: why = "a 'custom' vial"; break;
    case K::Traced: case K::Plain: case K::Cone:
        if (d.vial_type == TVAM_VIAL_INDEX_MATCHED) break;
        vial = std::string(p->kind == K::Traced ? "a traced '" : "a '") +
               (d.vial_type == TVAM_VIAL_SQUARE ? "square" : "cylindrical") + "' vial";
        why = vial.c_str();
        break;
    }
    if (why) return tvam_fail(TVAM_ERR_UNSUPPORTED, std::string(who) + ": " + why);
    if (d.albedo > 0.0f) why = "albedo > 0 (a scattering medium)";
    else if (d.sensor_type != TVAM_SENSOR_DDA) why = "the 'ratio' / 'delta' sensors are not differentiated";
    else if (p->surface) why = "a surface-aware (two-channel) film is not differentiated";
    else if (p->k.z0 != 0 || p->k.nz != p->k.res[2]) why = "a film slab is not differentiated (render the whole film)";
    else if (d.n_occluder_tris > 0) why = "occluders";
    else if (d.projector_type != TVAM_PROJECTOR_TELECENTRIC && d.projector_type != TVAM_PROJECTOR_LENS)
        why = "a collimated projector (telecentric and lens projectors only)";
    if (why) return tvam_fail(TVAM_ERR_UNSUPPORTED, std::string(who) + ": " + why);
    if (param < TVAM_DPROJ_DISTANCE || param > TVAM_DPROJ_PIXEL_SIZE)
        return tvam_fail(TVAM_ERR_INVALID, std::string(who) + ": param must be one of TVAM_DPROJ_*");
    return 0;
}

static TvamDproj dproj_of(const tvam_plan* p, int32_t param) {
    return TvamDproj{param, p->desc.pixel_size_x, p->desc.pixel_size_y};
}

extern "C" int tvam_forward_dprojector(tvam_plan* p, int32_t param, const float* active_data,
                                       const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                                       float* tangent, void* stream_) {
    if (!p || !tangent || (!active_data && n_active))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_forward_dprojector: null argument");
    int rc = dproj_check(p, param, "tvam_forward_dprojector");
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    if ((rc = call_setup(p, n_active, active_pixels, spp, k))) return rc;
    const size_t V = (size_t)k.res[0] * k.res[1] * k.nz;
    hipError_t e = hipMemsetAsync(tangent, 0, V * sizeof(float), stream);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemsetAsync");
    if (p->empty || n_active == 0) return 0;
    const float* pat = active_data;
    const int32_t* idxmap = nullptr;
    if ((rc = bind_active(p, k, active_data, active_pixels, n_active, stream, &pat, &idxmap))) return rc;
    e = tvam_launch_dproj(TVAM_MODE_FWD, k, call_tiles(p, spp, seed), dproj_of(p, param), pat, idxmap, nullptr, tangent,
                          nullptr, nullptr, stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "projector tangent launch");
}

extern "C" int tvam_adjoint_dprojector(tvam_plan* p, int32_t param, const float* active_data, const float* grad_dose,
                                       const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                                       double* g, void* stream_) {
    if (!p || !grad_dose || !g || (!active_data && n_active))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_adjoint_dprojector: null argument");
    int rc = dproj_check(p, param, "tvam_adjoint_dprojector");
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    if ((rc = call_setup(p, n_active, active_pixels, spp, k))) return rc;
    hipError_t e;
    if (p->empty || n_active == 0) {
        e = hipMemsetAsync(g, 0, sizeof(double), stream);
        return e == hipSuccess ? 0 : tvam_hip_fail(e, "hipMemsetAsync");
    }
    const float* pat = active_data;
    const int32_t* idxmap = nullptr;
    if ((rc = bind_active(p, k, active_data, active_pixels, n_active, stream, &pat, &idxmap))) return rc;
    const TvamTiles t = call_tiles(p, spp, seed);
    // (the grid, and with it the order of the sum, depends on the ray count alone)
    if ((e = p->dsig_part.grow(tvam_dsigma_grid((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp))) != hipSuccess)
        return tvam_hip_fail(e, "hipMalloc (projector partials)");
    e = tvam_launch_dproj(TVAM_MODE_ADJ, k, t, dproj_of(p, param), pat, idxmap, grad_dose, nullptr, p->dsig_part.get(), g,
                          stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "projector gradient launch");
}

// The rays of a call (tvam_ray3d.hip's export serves every projector kind); `segs`: the medium
// segments of a 'double_cylindrical' plan (tvam_plan_segments, two per ray) or of a plan with
// dielectric occluders (tvam_plan_insert_segments, max_segments per ray and their count) instead.
static int export_rays(tvam_plan* p, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                       float* rays, float* segs, void* stream_, int32_t max_segments = 0, int32_t* nseg = nullptr);

extern "C" int tvam_plan_rays(tvam_plan* p, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp,
                              uint32_t seed, float* rays, void* stream_) {
    if (!p || (!rays && n_active)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    const tvam_desc& d = p->desc;
    bool served = d.albedo == 0.0f && (d.n_occluder_tris == 0 || tvam_kind_inserts(p->kind));  // (the insert walk meets them)
    switch (p->kind) {
    case K::Plain: served = served && d.vial_type == TVAM_VIAL_INDEX_MATCHED; break;  // (planar refraction: not these rays)
    case K::Cone: case K::Traced: case K::Mesh: case K::Double: case K::Inserts: case K::Reflect: break;
    }
    if (!served)
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_plan_rays: index-matched, 'custom', 'double_cylindrical' and traced glass vial plans without scattering or occluders only");
    return export_rays(p, active_pixels, n_active, spp, seed, rays, nullptr, stream_);
}

extern "C" int tvam_plan_segments(tvam_plan* p, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp,
                                  uint32_t seed, float* segs, void* stream_) {
    if (!p || (!segs && n_active)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    switch (p->kind) {
    case K::Reflect: return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_plan_segments: a plan with reflected paths (transmission_only = 0) has any number of segments per ray (tvam_plan_insert_segments)");
    case K::Inserts: return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_plan_segments: a plan with dielectric occluders has any number of segments per ray (tvam_plan_insert_segments)");
    case K::Plain: case K::Cone: case K::Traced: case K::Mesh: return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_plan_segments: 'double_cylindrical' vial plans only");
    case K::Double: break;
    }
    if (((uintptr_t)segs & 15u) != 0) return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_segments: segs must be 16-byte aligned");
    return export_rays(p, active_pixels, n_active, spp, seed, nullptr, segs, stream_, 2);
}

extern "C" int tvam_plan_insert_segments(tvam_plan* p, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp,
                                         uint32_t seed, int32_t max_segments, float* segs, int32_t* nseg,
                                         void* stream_) {
    if (!p || ((!segs || !nseg) && n_active)) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    switch (p->kind) {
    case K::Plain: case K::Cone: case K::Traced: case K::Mesh: case K::Double: return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_plan_insert_segments: plans with dielectric occluders only (tvam_plan_create_inserts; reflected paths: tvam_plan_create_reflect)");
    case K::Inserts: case K::Reflect: break;
    }
    if (max_segments <= 0) return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_insert_segments: max_segments must be positive");
    if (((uintptr_t)segs & 15u) != 0) return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_insert_segments: segs must be 16-byte aligned");
    return export_rays(p, active_pixels, n_active, spp, seed, nullptr, segs, stream_, max_segments, nseg);
}

static int export_rays(tvam_plan* p, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                       float* rays, float* segs, void* stream_, int32_t max_segments, int32_t* nseg) {
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k;
    int rc = call_setup(p, n_active, active_pixels, spp, k);
    if (rc) return rc;
    if (n_active == 0) return 0;
    hipError_t e;
    const int32_t* idxmap = nullptr;
    if ((rc = bind_active(p, k, nullptr, active_pixels, n_active, stream, nullptr, &idxmap))) return rc;
    TvamTiles t = call_tiles(p, spp, seed);
    e = tvam_launch_ray3d_export(tvam_plan_walk(p), k, t, p->ins_eta.get(), idxmap, rays, segs, max_segments, nseg, stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "ray export launch");
}

extern "C" int tvam_count_visits(tvam_plan* p, uint32_t spp, uint32_t seed, uint64_t* visits) {
    if (!p || !visits) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    TvamConsts k;
    int rc = call_setup(p, shard_pixels(p), nullptr, spp, k);
    if (rc) return rc;
    *visits = 0;
    if (p->empty) return 0;
    hipError_t e = hipMemset(p->counter.get(), 0, sizeof(unsigned long long));
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemset");
    TvamTiles t = call_tiles(p, spp, seed);
    if (p->general) {
        e = tvam_kind_ray3d(p->kind)
                ? launch_ray3d(TVAM_MODE_COUNT, p, k, t, nullptr, nullptr, nullptr, nullptr, p->counter.get(), nullptr)
                : tvam_launch_general_paths(TVAM_MODE_COUNT, k, t, nullptr, nullptr, nullptr, nullptr, p->counter.get(), nullptr);
    } else if (p->surface) {
        e = tvam_launch_surface_paths(TVAM_MODE_COUNT, k, t, nullptr, nullptr, nullptr, nullptr, nullptr, p->counter.get(),
                                      nullptr);
    } else {
        if ((rc = ensure_rays(p, k, t, nullptr, nullptr))) return rc;
        e = tvam_launch_tiles(TVAM_MODE_COUNT, k, t, p->lds_bytes, nullptr, nullptr, nullptr, nullptr, p->counter.get(),
                              nullptr);
        if (e == hipSuccess)
            e = tvam_launch_frozen(TVAM_MODE_COUNT, k, t, nullptr, nullptr, nullptr, nullptr, p->counter.get(), nullptr);
    }
    if (e != hipSuccess) return tvam_hip_fail(e, "count launch");
    if (p->desc.albedo != 0.0f && !p->general && !p->surface) {  // (the surface kernel runs whole paths)
        e = tvam_launch_scatter_paths(TVAM_MODE_COUNT, k, t, nullptr, nullptr, nullptr, nullptr, p->counter.get(), nullptr);
        if (e != hipSuccess) return tvam_hip_fail(e, "scatter count launch");
    }
    unsigned long long h = 0;
    e = hipMemcpy(&h, p->counter.get(), sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemcpy");
    *visits = h;
    return 0;
}

extern "C" int tvam_radon(tvam_plan* p, const float* target_tris, int32_t n_target_tris, uint32_t spp, uint32_t seed,
                          int32_t max_depth, float* radon, void* stream_) {
    if (!p || !radon || n_target_tris < 0 || (n_target_tris > 0 && !target_tris))
        return tvam_fail(TVAM_ERR_INVALID, "null argument");
    switch (p->kind) {  // the Radon path is a planar ray (tvam_radon_ray)
    case K::Reflect: return tvam_fail(TVAM_ERR_UNSUPPORTED, "transmission_only = 0 with filter_radon (the Radon pass's own reflection sampling) is not implemented on the GPU path");
    case K::Inserts: return tvam_fail(TVAM_ERR_UNSUPPORTED, "dielectric occluders with filter_radon are not implemented on the GPU path");
    case K::Mesh: return tvam_fail(TVAM_ERR_UNSUPPORTED, "a 'custom' vial with filter_radon is not implemented on the GPU path");
    case K::Double: return tvam_fail(TVAM_ERR_UNSUPPORTED, "a 'double_cylindrical' vial with filter_radon is not implemented on the GPU path");
    case K::Traced: return tvam_fail(TVAM_ERR_UNSUPPORTED, "a traced 'cylindrical' / 'square' vial with filter_radon is not implemented on the GPU path");
    case K::Cone: return tvam_fail(TVAM_ERR_UNSUPPORTED, "the 'telecentric' / 'lens' projectors with filter_radon are not implemented on the GPU path");
    case K::Plain: break;
    }
    TvamConsts k;
    int rc = call_setup(p, shard_pixels(p), nullptr, spp, k);
    if (rc) return rc;
    const float wray = ray_weight(p->desc, shard_pixels(p), spp);
    hipStream_t stream = (hipStream_t)stream_;
    TvamDevBuf<float> dt;
    hipError_t e = hipSuccess;
    if (n_target_tris > 0) {
        const size_t n = (size_t)n_target_tris * 9;
        if ((e = dt.alloc(n)) != hipSuccess) return tvam_hip_fail(e, "hipMalloc (target mesh)");
        if ((e = hipMemcpy(dt.get(), target_tris, n * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
            return tvam_hip_fail(e, "hipMemcpy (target mesh)");
    }
    TvamTiles t = call_tiles(p, spp, seed);
    e = tvam_launch_radon(k, t, dt.get(), n_target_tris, max_depth, wray, radon, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "radon launch");
}

// 'filter_corner' (tvam_corner.hip): reads only the projector, motion, vial and occluder fields, so
// every plan kind serves it (an `empty` plan too: the pass does not depend on max_depth).
extern "C" int tvam_corner(tvam_plan* p, const uint32_t* active_pixels, uint64_t n_active, float dist, float radius,
                           float* keep, float* hits, void* stream_) {
    if (!p) return tvam_fail(TVAM_ERR_INVALID, "tvam_corner: null plan");
    switch (p->kind) {
    case K::Double: return tvam_fail(TVAM_ERR_UNSUPPORTED, "a 'double_cylindrical' vial with filter_corner is not implemented on the GPU path");
    case K::Plain: case K::Cone: case K::Traced: case K::Mesh: case K::Inserts: case K::Reflect: break;
    }
    if (!keep) return tvam_fail(TVAM_ERR_INVALID, "tvam_corner: null keep");
    if (!(radius >= 0.0f)) return tvam_fail(TVAM_ERR_INVALID, "tvam_corner: radius must be >= 0");
    if (!std::isfinite(dist)) return tvam_fail(TVAM_ERR_INVALID, "tvam_corner: dist must be finite");
    if (((uintptr_t)hits & 15u) != 0) return tvam_fail(TVAM_ERR_INVALID, "tvam_corner: hits must be 16-byte aligned");
    if (!active_pixels && n_active != shard_pixels(p))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_corner: n_active must equal the shard's dense size when active_pixels is null");
    if (n_active > (uint64_t)INT64_MAX) return tvam_fail(TVAM_ERR_INVALID, "tvam_corner: n_active too large");
    if (n_active == 0) return 0;
    hipError_t e = hipSetDevice(p->device);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipSetDevice");
    TvamConsts k = p->k;  // the pass's own sampling (optimize.py:167-171): regular, spp 1, seed 0, no time sample
    k.regular = 1;
    k.sample_time = 0;
    TvamTiles t = p->tiles;
    t.spp = 1;
    t.seed = 0;
    e = tvam_launch_corner(k, t, active_pixels, (int64_t)n_active, dist, radius, keep, hits, (hipStream_t)stream_);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "corner launch");
}

extern "C" int tvam_compute_volume(tvam_plan* p, uint32_t sample_count, float* volumes, void* stream_) {
    if (!p || !volumes) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (!p->surface) return tvam_fail(TVAM_ERR_INVALID, "compute_volume needs a surface-aware film (film_channels 2)");
    if (sample_count == 0) return tvam_fail(TVAM_ERR_INVALID, "sample_count must be positive");
    hipError_t e = hipSetDevice(p->device);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipSetDevice");
    hipStream_t stream = (hipStream_t)stream_;
    e = tvam_launch_volumes(p->k, sample_count, volumes, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "compute_volume launch");
}

extern "C" int tvam_plan_set_volumes(tvam_plan* p, const float* volumes) {
    if (!p) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (!p->surface) return tvam_fail(TVAM_ERR_INVALID, "volumes apply to surface-aware films (film_channels 2)");
    p->vols = volumes;
    return 0;
}

extern "C" int tvam_discretize(const tvam_desc* desc, float* occ, void* stream_) {
    if (!desc || !occ) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    const tvam_desc& d = *desc;
    if (d.abi_version != TVAM_ABI_VERSION) return tvam_fail(TVAM_ERR_INVALID, "tvam_desc.abi_version mismatch");
    if (d.n_target_tris <= 0 || !d.target_tris) return tvam_fail(TVAM_ERR_INVALID, "No target shape found in the scene");
    for (int a = 0; a < 3; ++a)
        if (d.film_res[a] <= 0 || !(d.bbox_max[a] > d.bbox_min[a]))
            return tvam_fail(TVAM_ERR_INVALID, "film resolution and sensor bbox must be positive");
    if ((int64_t)d.film_res[0] * d.film_res[1] * d.film_res[2] > (int64_t)1 << 32)
        return tvam_fail(TVAM_ERR_TOO_LARGE, "discretize: more than 2^32 voxels");
    hipStream_t stream = (hipStream_t)stream_;
    TvamConsts k{};
    for (int a = 0; a < 3; ++a) {
        k.res[a] = d.film_res[a];
        k.bmin[a] = d.bbox_min[a];
        k.h[a] = (d.bbox_max[a] - d.bbox_min[a]) / (float)d.film_res[a];  // utils.py:104
    }
    const size_t nt = (size_t)d.n_target_tris * 9;
    TvamDevBuf<float> d_tris;
    hipError_t e = d_tris.alloc(nt);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMalloc");
    e = hipMemcpyAsync(d_tris.get(), d.target_tris, nt * sizeof(float), hipMemcpyHostToDevice, stream);
    k.tgt = d_tris.get();
    k.n_tgt = d.n_target_tris;
    if (e == hipSuccess) e = tvam_launch_discretize(k, d.target_tris, occ, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "discretize launch");
}

extern "C" int tvam_plan_fwd_scale(tvam_plan* p, float* scale) {
    if (!p || !scale) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (!p->planar || p->planar_fwd)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_fwd_scale: this plan's forward is not the ray-driven planar kernel");
    hipError_t e = hipSetDevice(p->device);
    if (e == hipSuccess) e = hipMemcpy(scale, p->fscale.get(), 2 * sizeof(float), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : tvam_hip_fail(e, "hipMemcpy");
}

// bit 0: planar adjoint (+ ray-driven planar forward unless bit 1), bit 1: voxel-driven planar forward
// bit 2: 3-D projector rays (telecentric / lens)
extern "C" int tvam_plan_path(const tvam_plan* p) {
    return p ? (p->planar ? 1 : 0) | (p->planar_fwd ? 2 : 0) | (tvam_kind_ray3d(p->kind) ? 4 : 0) : 0;
}

extern "C" int tvam_plan_fwd_variant(const tvam_plan* p, int32_t* v) {
    if (!p || !v) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (!p->planar_fwd)
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_plan_fwd_variant: the voxel-driven forward does not serve this plan");
    TvamFwdVariant fv;
    if (!tvam_planar_fwd_variant(p->pl, p->planar_fz, fv))
        return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_fwd_variant: no instantiated forward kernel serves the plan's tables");
    v[0] = fv.z;
    v[1] = fv.nc;
    v[2] = p->pl.fwd_nc;
    v[3] = p->pl.ncmax;
    v[4] = fv.ab;
    v[5] = fv.pf;
    v[6] = (fv.bin ? 1 : 0) | (fv.dma ? 2 : 0) | (fv.multi ? 4 : 0) | (fv.refr ? 8 : 0) | (fv.sconst ? 16 : 0);
    v[7] = p->pl.fwd_parts > 1 ? p->pl.fwd_parts : 1;
    return 0;
}

extern "C" int tvam_plan_stats(tvam_plan* p, uint64_t* fallback_tiles) {
    if (!p || !fallback_tiles) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    unsigned long long h = 0;
    hipError_t e = hipMemcpy(&h, p->counter.get(), sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemcpy");
    *fallback_tiles = h;
    return 0;
}

extern "C" int tvam_plan_bin_stats(tvam_plan* p, int64_t* stats) {
    if (!p || !stats) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    const TvamBinScratch& b = p->bins;
    for (int i = 0; i < 5; ++i) stats[i] = b.st[i];
    int64_t cache = 0;  // device bytes the forward bin cache holds
    for (const TvamBinChunk& c : b.fc)
        cache += (int64_t)(c.r.capacity() * sizeof(float4) + (c.vals.capacity() + c.bstart.capacity()) * sizeof(uint32_t));
    stats[5] = cache;
    // the chunk scratch: records, brick counts and offsets, sort keys / values, adjoint partials
    stats[6] = b.cap_slots * (TVAM_REC_F4 * (int64_t)sizeof(float4) + 2 * (int64_t)sizeof(uint32_t)) +
               b.cap_entries * (int64_t)(4 * sizeof(uint32_t) + sizeof(float)) + (int64_t)b.bstart.capacity() * 4 +
               (int64_t)b.temp.capacity();
    // slots whose bin-fill walk disagreed with the record writer's closed-form brick count
    // (sc_brick_count; 0 by construction, checked by the tests), summed over the calls since the
    // chunk scratch was allocated
    stats[7] = 0;
    if (b.bad.get()) {
        uint32_t bad = 0;
        if (hipMemcpy(&bad, b.bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return tvam_fail(TVAM_ERR_HIP, "tvam_plan_bin_stats: reading the count check");
        stats[7] = bad;
    }
    return 0;
}

// The per-ray tile kernels' row walks for the plan's most recent ray records (jittered plans):
// how many rays the ray setup listed as strays (rays outside their row's main slice) and what
// the (tile, slice) workgroups walk because of them -- every workgroup of a slice walks that
// slice's whole stray list, against its main rows' slots.
extern "C" int tvam_plan_tile_stats(tvam_plan* p, int64_t* stats) {
    if (!p || !stats) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    stats[0] = -1;
    const tvam_plan::RaySlot* r = nullptr;
    for (const auto& s : p->rs)
        if (s.valid && (!r || s.used > r->used)) r = &s;
    if (!r) return 0;
    unsigned long long ns = 0, nf = 0;
    hipError_t e = hipSuccess;
    const bool lists = r->stray_n.get() && p->n_main_rows > 0;
    if (lists) e = hipMemcpy(&ns, r->stray_n.get(), sizeof(ns), hipMemcpyDeviceToHost);
    if (e == hipSuccess && r->frozen_n.get()) e = hipMemcpy(&nf, r->frozen_n.get(), sizeof(nf), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipMemcpy");
    stats[0] = lists ? (int64_t)ns : -1;
    stats[1] = lists ? (int64_t)TVAM_STRAY_CAP : 0;
    // strays beyond the cap: the workgroups walk the full row lists instead (no stray walk)
    const bool used = lists && ns <= (unsigned long long)TVAM_STRAY_CAP;
    stats[2] = used ? (int64_t)ns * p->ntiles : 0;
    stats[3] = (used ? p->n_main_rows : p->n_rows_all) * p->n_slots_all * (int64_t)r->spp;
    stats[4] = (int64_t)nf;
    stats[5] = (int64_t)r->spp;
    stats[6] = p->ntiles;
    stats[7] = p->n_slots_all;
    return 0;
}

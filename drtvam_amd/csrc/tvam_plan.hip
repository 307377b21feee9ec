// tvam_plan.hip — descriptor validation, plan construction and destruction, tuning knobs and the
// kernel launch timer (the per-call entry points: tvam_calls.hip).
//
// The plan turns a tvam_desc (the reference's scene / plugin properties) into
// the small constant tables the tile kernels consume:
//   * per-angle (cos, sin) of the shard, computed like CircularMotion.eval
//     (motion.py:26-36: alpha = 2*pi*time, time = angle / n_patterns);
//   * per-z-slice list of DMD rows whose (planar) rays lie in that slice;
//   * per-(xy-tile, angle) range of DMD columns whose rays can cross the tile.
#include "tvam_plan.h"
#include "tvam_glass.h"
#include "tvam_insert.h"
#include "tvam_mesh.h"

#include <algorithm>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace {
thread_local std::string g_err;
}

int tvam_fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int tvam_hip_fail(hipError_t e, const char* what) {
    return tvam_fail(TVAM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

extern "C" void tvam_desc_init(tvam_desc* d) {
    std::memset(d, 0, sizeof(*d));
    d->abi_version = TVAM_ABI_VERSION;
    d->projector_type = TVAM_PROJECTOR_COLLIMATED;
    d->n_patterns = 1000;            // projector.py:73
    d->res_x = d->res_y = 256;       // projector.py:74-75
    d->crop_x = d->crop_y = 256;
    d->pixel_size_x = d->pixel_size_y = 1.0f;
    d->distance = 20.0f;
    d->sensor_type = TVAM_SENSOR_DDA;
    for (int a = 0; a < 3; ++a) {
        d->bbox_min[a] = -0.5f;
        d->bbox_max[a] = 0.5f;
        d->film_res[a] = 256;        // film.py:9-11
    }
    d->film_channels = 1;
    d->vial_type = TVAM_VIAL_INDEX_MATCHED;
    d->vial_height = 40.0f;          // geometry.py:80
    d->medium_ior = 1.0f;
    d->vial_ior = 1.5f;
    d->print_time = 1.0f;            // common.py:13
    d->regular_sampling = 0;         // common.py:22
    d->sample_time = 0;              // common.py:10
    d->max_depth = 6;                // optimize.py:99
    d->rr_depth = 6;                 // optimize.py:100
    d->transmission_only = 1;        // common.py:19
    d->angle_begin = 0;
    d->angle_end = -1;               // -1: all angles
    d->tile = 0;
    d->slab_begin = 0;
    d->slab_end = -1;                // -1: all slices
}

extern "C" const char* tvam_last_error(void) { return g_err.c_str(); }
extern "C" int tvam_abi_version(void) { return TVAM_ABI_VERSION; }
extern "C" int64_t tvam_device_bytes(void) { return g_tvam_device_bytes.load(); }

static void kt_plan_gone(const tvam_plan* p);  // the kernel timer's events go with their owning plan

extern "C" void tvam_plan_destroy(tvam_plan* p) {
    if (!p) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(p->device);
    kt_plan_gone(p);
    delete p;
    (void)hipSetDevice(cur);
}

// The kind of a descriptor handed to tvam_plan_create (or tvam_row_slices): no payload beside it.
static TvamPlanKind desc_kind(const tvam_desc& d) {
    if (d.vial_type == TVAM_VIAL_CUSTOM) return TvamPlanKind::Mesh;  // (tvam_plan_create refuses these two before it asks)
    if (d.vial_type == TVAM_VIAL_DOUBLE_CYLINDRICAL) return TvamPlanKind::Double;
    return d.projector_type != TVAM_PROJECTOR_COLLIMATED ? TvamPlanKind::Cone : TvamPlanKind::Plain;
}

static bool has_slab(const tvam_desc& d) {
    return d.slab_begin != 0 || (d.slab_end >= 0 && d.slab_end != d.film_res[2]);
}

// What the 3-D ray kernels (tvam_ray3d.hip) do not serve, kind by kind: every ray of such a plan is
// traced in 3-D and runs the per-ray kernels.  A refusal reads subject + limit + tail; the limits that
// kinds share are stated once, and each kind lists them, with its own, in the order of its refusals.
static int ray3d_limits(const tvam_desc& d, TvamPlanKind kind) {
    const char* pn = d.projector_type == TVAM_PROJECTOR_LENS ? "'lens'" : d.projector_type == TVAM_PROJECTOR_TELECENTRIC ? "'telecentric'" : "'collimated'";
    const std::string projector = std::string("the ") + pn + " projector with ";
    std::string subject;
    const char* tail = " is not implemented on the GPU path";
    switch (kind) {
    case TvamPlanKind::Plain: return 0;
    case TvamPlanKind::Cone: subject = projector; break;
    case TvamPlanKind::Traced: subject = projector, tail = " behind a traced glass vial is not implemented on the GPU path"; break;
    case TvamPlanKind::Mesh: subject = "a 'custom' vial with "; break;
    case TvamPlanKind::Double: subject = "a 'double_cylindrical' vial with "; break;
    case TvamPlanKind::Inserts: subject = "dielectric occluders with ", tail = " are not implemented on the GPU path"; break;
    case TvamPlanKind::Reflect: subject = "transmission_only = 0 with "; break;
    }
    int rc = 0;  // set by the first limit that refuses; each limit returns whether it refused
    auto no = [&](const std::string& what) { return (rc = tvam_fail(TVAM_ERR_UNSUPPORTED, subject + what + tail)) != 0; };
    auto invalid = [&](const char* msg) { return (rc = tvam_fail(TVAM_ERR_INVALID, msg)) != 0; };
    auto lens = [&] {
        return d.projector_type != TVAM_PROJECTOR_COLLIMATED &&
               ((!(d.focus_distance > 0.0f) && invalid("focus_distance must be positive")) ||
                (!(d.aperture_radius >= 0.0f) && invalid("aperture_radius must be >= 0")));
    };
    auto occluders = [&] { return d.n_occluder_tris > 0 && no("occluders"); };
    auto medium_sensor_film = [&] {  // absorbing medium, 'dda' sensor, one-channel film, the whole film
        return (d.albedo != 0.0f && no("a scattering medium (albedo > 0)")) ||
               (d.sensor_type == TVAM_SENSOR_RATIO && no("the 'ratio' sensor")) ||
               (d.sensor_type == TVAM_SENSOR_DELTA && no("the 'delta' sensor")) ||
               (d.film_channels == 2 && no("a surface-aware film")) || (has_slab(d) && no("film slabs"));
    };
    auto refraction_only = [&](const char* where) {
        return !d.transmission_only && no(std::string("transmission_only = 0 (reflected paths at the ") + where + ")");
    };
    auto rr2 = [&] { return d.rr_depth < 2 && no("rr_depth < 2 (Russian roulette before the medium segment)"); };
    bool refused = false;
    switch (kind) {  // each kind's limits, its own among them, in the order of its refusals
    case TvamPlanKind::Plain: break;
    case TvamPlanKind::Cone:  // index-matched vial (3-D refraction at the glass: the traced entry's, with its own limits)
        refused = lens() ||
                  (tvam_plan::glass(d) && (rc = tvam_fail(TVAM_ERR_UNSUPPORTED, subject + "a " + (d.vial_type == TVAM_VIAL_SQUARE ? "'square'" : "'cylindrical'") +
                                                                      " vial (3-D refraction) needs the traced path: create the plan with tvam_plan_create_traced"))) ||
                  occluders() || medium_sensor_film();
        break;
    case TvamPlanKind::Traced:  // the two analytic surfaces of tvam_glass.h
        refused = lens() ||
                  (!(d.vial_r > 0.0f && d.vial_r_ext > d.vial_r && d.vial_ior > 0.0f && d.medium_ior > 0.0f && d.vial_height > 0.0f) &&
                   invalid("glass vial: need r_ext > r_int > 0 (w_ext > w_int), a positive height and positive IORs")) ||
                  occluders() || medium_sensor_film() || refraction_only("glass interfaces") || rr2();
        break;
    case TvamPlanKind::Mesh:
        refused = lens() || occluders() || medium_sensor_film() || refraction_only("glass interfaces") || rr2() ||
                  (!(d.vial_ior > 0.0f && d.medium_ior > 0.0f) && invalid("a 'custom' vial needs positive IORs"));
        break;
    case TvamPlanKind::Double:
        // the last deposit is at loop iteration min(max_depth - 1, 6); Russian roulette acts at
        // iterations > rr_depth (volume.py:182-185)
        refused = lens() || occluders() || medium_sensor_film() || refraction_only("glass interfaces") ||
                  (d.rr_depth < std::min(d.max_depth, 7) - 1 && no("rr_depth < min(max_depth, 7) - 1 (Russian roulette on or before a deposit)")) ||
                  (!(d.vial_height > 0.0f) && invalid("a 'double_cylindrical' vial needs a positive height"));
        break;
    case TvamPlanKind::Inserts:  // black occluders are walked, and Russian roulette is honoured: no limit on either
    case TvamPlanKind::Reflect:
        refused = (kind == TvamPlanKind::Reflect && d.transmission_only &&
                   invalid("tvam_plan_create_reflect: transmission_only = 1 belongs to tvam_plan_create and its siblings")) ||
                  (d.vial_type == TVAM_VIAL_CUSTOM && no("a 'custom' vial")) ||
                  (d.vial_type == TVAM_VIAL_DOUBLE_CYLINDRICAL && no("a 'double_cylindrical' vial")) || lens() ||
                  (!(d.vial_height > 0.0f) && invalid("dielectric occluders need a positive vial height")) ||
                  medium_sensor_film() || (kind == TvamPlanKind::Inserts && refraction_only("interfaces"));
        break;
    }
    return refused ? rc : 0;
}

// The limits of a descriptor of `kind`, before any device call: the kind's own (ray3d_limits), then every kind's.
static int validate(const tvam_desc& d, TvamPlanKind kind) {
    if (d.abi_version != TVAM_ABI_VERSION) return tvam_fail(TVAM_ERR_INVALID, "tvam_desc.abi_version mismatch");
    if (d.projector_type != TVAM_PROJECTOR_COLLIMATED && d.projector_type != TVAM_PROJECTOR_TELECENTRIC &&
        d.projector_type != TVAM_PROJECTOR_LENS)
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "only the 'collimated', 'telecentric' and 'lens' projectors are implemented on the GPU path");
    if (kind == TvamPlanKind::Traced && d.vial_type != TVAM_VIAL_CYLINDRICAL && d.vial_type != TVAM_VIAL_SQUARE)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_create_traced: vial_type must be TVAM_VIAL_CYLINDRICAL or TVAM_VIAL_SQUARE (other vials: tvam_plan_create and its siblings)");
    if (const int rc = ray3d_limits(d, kind)) return rc;
    if (d.sensor_type != TVAM_SENSOR_DDA && d.sensor_type != TVAM_SENSOR_RATIO && d.sensor_type != TVAM_SENSOR_DELTA)
        return tvam_fail(TVAM_ERR_INVALID, "unknown sensor type");
    if (d.sensor_type == TVAM_SENSOR_DELTA && d.albedo == 0.0f)  // volume.py:160-161
        return tvam_fail(TVAM_ERR_INVALID, "Tried to render a purely absorptive volume with a delta tracking sensor. This is not supported.");
    if (d.sensor_type == TVAM_SENSOR_RATIO && !(d.majorant > 0.0f))
        return tvam_fail(TVAM_ERR_INVALID, "the 'ratio' sensor needs a positive majorant");
    if (d.sample_time && d.film_channels != 1)
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "sample_time needs a one-channel film");
    if ((d.sensor_type != TVAM_SENSOR_DDA || d.sample_time) && has_slab(d))
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "sample_time and the ratio / delta sensors need a film without slabs");
    if (d.vial_type != TVAM_VIAL_INDEX_MATCHED && d.vial_type != TVAM_VIAL_CYLINDRICAL &&
        d.vial_type != TVAM_VIAL_SQUARE && d.vial_type != TVAM_VIAL_CUSTOM &&
        d.vial_type != TVAM_VIAL_DOUBLE_CYLINDRICAL)
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "only the 'index_matched', 'cylindrical', 'square', 'custom' and 'double_cylindrical' containers are implemented on the GPU path");
    // transmission_only = False lets the reference sample reflection as well as refraction at every
    // dielectric interface after the first (volume.py:235-243, radon.py:87-95); the kernels only
    // refract.  An index-matched vial has no such interface; a Reflect plan's kernels sample both.
    if (d.vial_type != TVAM_VIAL_INDEX_MATCHED && !d.transmission_only && kind != TvamPlanKind::Reflect)
        return tvam_fail(TVAM_ERR_UNSUPPORTED,
                         std::string("transmission_only = 0 behind a ") +
                             (d.vial_type == TVAM_VIAL_SQUARE ? "'square'" : "'cylindrical'") +
                             " vial (reflected paths at the glass interfaces) is not implemented on the GPU path");
    if (d.n_occluder_tris < 0 || (d.n_occluder_tris > 0 && !d.occluder_tris))
        return tvam_fail(TVAM_ERR_INVALID, "occluder_tris is null");
    if (d.film_channels != 1 && d.film_channels != 2) return tvam_fail(TVAM_ERR_INVALID, "film_channels must be 1 or 2");
    if (d.film_channels == 2) {
        if (d.n_target_tris <= 0 || !d.target_tris)
            return tvam_fail(TVAM_ERR_INVALID, "No target shape found in the scene");  // sensor.py:60-61
        if (has_slab(d)) return tvam_fail(TVAM_ERR_UNSUPPORTED, "surface-aware films cannot be split into slabs");
    }
    if (!(d.albedo >= 0.0f && d.albedo <= 1.0f)) return tvam_fail(TVAM_ERR_INVALID, "medium albedo must lie in [0, 1]");
    if (d.albedo != 0.0f) {
        if (!(d.sigma_t > 0.0f)) return tvam_fail(TVAM_ERR_INVALID, "scattering medium: extinction must be positive");
        if (d.phase_type < TVAM_PHASE_ISOTROPIC || d.phase_type > TVAM_PHASE_HG)
            return tvam_fail(TVAM_ERR_UNSUPPORTED, "unknown phase function");
        if (has_slab(d))
            return tvam_fail(TVAM_ERR_UNSUPPORTED, "scattered paths leave their slice: film slabs need a non-scattering medium");
    }
    // the medium segment is path vertex 1 (index matched) or 2 (behind two glass
    // surfaces); Russian roulette starts at depth > rr_depth (volume.py:182-185)
    if (!tvam_kind_inserts(kind) && kind != TvamPlanKind::Double &&
        d.rr_depth < (d.vial_type == TVAM_VIAL_INDEX_MATCHED ? 1 : 2))
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "Russian roulette before the medium segment (rr_depth too small) is not implemented");
    if (d.n_patterns <= 0 || d.res_x <= 0 || d.res_y <= 0) return tvam_fail(TVAM_ERR_INVALID, "projector resolution and n_patterns must be positive");
    if (d.crop_x <= 0 || d.crop_y <= 0 || d.crop_x > d.res_x || d.crop_y > d.res_y)
        return tvam_fail(TVAM_ERR_INVALID, "Crop resolution must be smaller than the base resolution.");  // projector.py:81-82
    if (d.crop_offset_x < 0 || d.crop_offset_y < 0 || d.crop_offset_x + d.crop_x > d.res_x ||
        d.crop_offset_y + d.crop_y > d.res_y)
        return tvam_fail(TVAM_ERR_INVALID, "With the specified crop offset, the cropped region extends beyond the base resolution.");  // projector.py:87-88
    for (int a = 0; a < 3; ++a) {
        if (d.film_res[a] <= 0) return tvam_fail(TVAM_ERR_INVALID, "film resolution must be positive");
        if (!(d.bbox_max[a] > d.bbox_min[a])) return tvam_fail(TVAM_ERR_INVALID, "sensor bounding box is empty");
    }
    // (a 'custom' vial's surfaces are its meshes: vial_r, vial_r_ext and vial_height are unused; a
    // 'double_cylindrical' vial's radii are tvam_double_vial's)
    const bool own_surfaces = kind == TvamPlanKind::Mesh || kind == TvamPlanKind::Double;
    if (!own_surfaces && !(d.vial_r > 0.0f))
        return tvam_fail(TVAM_ERR_INVALID, "vial radius must be positive");
    if (d.vial_type != TVAM_VIAL_INDEX_MATCHED && !own_surfaces &&
        !(d.vial_r_ext > d.vial_r && d.vial_ior > 0.0f && d.medium_ior > 0.0f && d.vial_height > 0.0f))
        return tvam_fail(TVAM_ERR_INVALID, "glass vial: need r_ext > r_int > 0 (w_ext > w_int) and positive IORs");
    {
        const int z1 = d.slab_end < 0 ? d.film_res[2] : d.slab_end;
        if (d.slab_begin < 0 || z1 > d.film_res[2] || d.slab_begin >= z1)
            return tvam_fail(TVAM_ERR_INVALID, "invalid film slab [slab_begin, slab_end)");
    }
    if (!(d.pixel_size_x > 0.0f && d.pixel_size_y > 0.0f)) return tvam_fail(TVAM_ERR_INVALID, "pixel_size must be positive");
    if (d.active_base < 0 || d.active_total < 0) return tvam_fail(TVAM_ERR_INVALID, "active_base / active_total must be >= 0");
    return 0;
}

static TvamConsts make_consts(const tvam_desc& d, int a0, int a1) {
    TvamConsts k;
    std::memset(&k, 0, sizeof(k));
    for (int a = 0; a < 3; ++a) {
        k.bmin[a] = d.bbox_min[a];
        k.bmax[a] = d.bbox_max[a];
        k.res[a] = d.film_res[a];
        k.h[a] = (d.bbox_max[a] - d.bbox_min[a]) / (float)d.film_res[a];  // sensor.py:19
    }
    k.z0 = d.slab_begin;
    k.nz = (d.slab_end < 0 ? d.film_res[2] : d.slab_end) - d.slab_begin;
    float vol = k.h[0] * k.h[1] * k.h[2];
    k.inv_vol = vol != 0.0f ? 1.0f / vol : 0.0f;  // volume.py:41-42
    k.res_x = d.res_x;
    k.res_y = d.res_y;
    k.crop_x = d.crop_x;
    k.crop_y = d.crop_y;
    k.crop_off_x = d.crop_offset_x;
    k.crop_off_y = d.crop_offset_y;
    k.n_patterns = d.n_patterns;
    k.a0 = a0;
    k.a1 = a1;
    k.shard_base = (int64_t)a0 * d.crop_y * d.crop_x;
    k.stream_base = d.active_base;
    k.ex = (float)d.res_x * d.pixel_size_x;
    k.ey = (float)d.res_y * d.pixel_size_y;
    k.inv_w = 1.0f / (float)d.res_x;
    k.inv_h = 1.0f / (float)d.res_y;
    k.dist_m_zc = d.distance - 0.005f;
    k.clockwise = d.clockwise;
    k.regular = d.regular_sampling;
    k.sample_time = d.sample_time;
    k.skip_zero = (d.flags & TVAM_FLAG_NO_ZERO_SKIP) ? 0 : 1;
    k.vial_type = d.vial_type;
    k.max_depth = d.max_depth;
    k.vial_r = d.vial_r;
    k.vial_half_h = 0.5f * d.vial_height;
    k.vial_r_ext = d.vial_r_ext;
    k.vial_hz_int = (float)(0.5 * 0.9 * (double)d.vial_height);  // geometry.py:207 (inner cuboid)
    k.eta_ext = d.vial_ior / TVAM_IOR_AIR;   // int/ext IOR of the outer surface (geometry.py:160-170)
    k.eta_int = d.medium_ior / d.vial_ior;   // and of the inner one (geometry.py:171-183)
    k.nsig2 = -d.sigma_t * 1.44269504088896340736f;
    k.sig_t = d.sigma_t;
    k.sig_s = d.albedo * d.sigma_t;
    k.rr_depth = d.rr_depth;
    k.phase_type = d.phase_type;
    k.phase_g = d.phase_g;
    k.sensor_type = d.sensor_type;
    k.majorant = d.majorant;
    k.wscale = 0.0f;  // per call
    k.proj_type = d.projector_type;
    k.ap_r = d.aperture_radius;
    k.focus = d.focus_distance;
    k.dist = d.distance;
    {
        double hxy = std::max((double)k.h[0], (double)k.h[1]);
        k.vox_chord = (float)std::min(1.0, (double)d.sigma_t * std::sqrt(2.0) * hxy);
        k.rays_per_voxel = (float)((double)(a1 - a0) * (std::ceil(std::sqrt(2.0) * hxy / d.pixel_size_x) + 1.0));
    }
    return k;
}
// Tuning knobs (TVAM_<NAME> environment variables) are honoured only under TVAM_EXPERIMENTAL=1 --
// A/B runs and the tests that force a code path (work splits, slab depths, chunk sizes) -- and
// each honoured one is logged; production plans take the defaults whatever the environment holds.
int tvam_knob(const char* name, int def) {
    const char* x = std::getenv("TVAM_EXPERIMENTAL");  // read per call: a test process sets it per test
    if (!(x && std::atoi(x) == 1)) return def;
    const char* v = std::getenv(name);
    if (!(v && *v)) return def;
    const int r = std::atoi(v);
    std::fprintf(stderr, "[tvam] TVAM_EXPERIMENTAL: %s=%d (default %d)\n", name, r, def);
    return r;
}
// Launch timer of the dominant forward kernel (tvam_plan_kernel_time): event pairs recorded on the
// launching stream around each launch while enabled (up to 1024 launches per measurement).  One
// timer per process, owned by the plan that enabled it: launches on another device are not
// recorded, the state is guarded by a mutex (plans on other host threads may launch meanwhile),
// and the events are destroyed with the owning plan.
namespace {
struct KernelTimer {
    std::mutex mu;
    bool on = false;
    int kind = 0;  // TvamKtKind of the measured plan's dominant forward kernel
    int device = -1;
    const tvam_plan* owner = nullptr;
    std::vector<hipEvent_t> ev;
    size_t n = 0;
};
KernelTimer g_kt;

bool kt_here(int kind) {
    if (!g_kt.on || kind != g_kt.kind || g_kt.n + 2 > g_kt.ev.size()) return false;
    int cur = -1;
    return hipGetDevice(&cur) == hipSuccess && cur == g_kt.device;
}

// the owner's events (every recorded pair complete first); caller holds the mutex
void kt_release() {
    for (size_t i = 0; i < g_kt.n; ++i) (void)hipEventSynchronize(g_kt.ev[i]);
    for (hipEvent_t e : g_kt.ev) (void)hipEventDestroy(e);
    g_kt.ev.clear();
    g_kt.n = 0;
    g_kt.on = false;
    g_kt.owner = nullptr;
    g_kt.device = -1;
}
}  // namespace

static void kt_plan_gone(const tvam_plan* p) {
    std::lock_guard<std::mutex> lk(g_kt.mu);
    if (g_kt.owner == p) kt_release();
}

void tvam_kt_begin(hipStream_t stream, int kind) {
    std::lock_guard<std::mutex> lk(g_kt.mu);
    if (kt_here(kind)) (void)hipEventRecord(g_kt.ev[g_kt.n], stream);
}

bool tvam_kt_take(int kind, hipEvent_t* start, hipEvent_t* stop) {
    std::lock_guard<std::mutex> lk(g_kt.mu);
    if (!kt_here(kind)) return false;
    *start = g_kt.ev[g_kt.n];
    *stop = g_kt.ev[g_kt.n + 1];
    g_kt.n += 2;
    return true;
}

void tvam_kt_end(hipStream_t stream, int kind) {
    std::lock_guard<std::mutex> lk(g_kt.mu);
    if (!kt_here(kind)) return;
    (void)hipEventRecord(g_kt.ev[g_kt.n + 1], stream);
    g_kt.n += 2;
}

// Planar fast path: regular sampling and rows whose vial entry offset is
// row-independent (|z| <= 0.7 r < r / sqrt(2) <= max(|p_x|, |p_y|) on the
// vial wall).  Builds the row -> slice CSR of valid rows and the per-(angle,
// column) ray table (computed once, here).
static bool planar_fwd_setup(tvam_plan* p, const std::vector<float2>& cs, const std::vector<int32_t>& off,
                             std::vector<float4>& fwd_ang_h, std::vector<int32_t>& fwd_cb_h);
static int fwd_buffers(tvam_plan* p);
static int choose_fwd_z(tvam_plan* p);
static int refr_fwd_setup(tvam_plan* p, const std::vector<int32_t>& off);

// Regular sampling: the slab-local slice of crop row rc's rays (the DDA start voxel z of its
// height yc, tvam_slice_of; outside [0, nz): the row misses the slab).
static int regular_row_slice(const tvam_desc& d, const TvamConsts& k, int rc, float& yc) {
    float xc;
    tvam_ray_camera(k, 0, d.crop_offset_y + rc, 0.5f, 0.5f, xc, yc);
    return tvam_slice_of(k, yc) - k.z0;
}

// The CSR (off, rows) of per-slice row lists; returns the longest list.
static int32_t rows_csr(const std::vector<std::vector<int32_t>>& rows_of, std::vector<int32_t>& off,
                        std::vector<int32_t>& rows) {
    int32_t most = 0;
    off.assign(rows_of.size() + 1, 0);
    for (size_t s = 0; s < rows_of.size(); ++s) {
        off[s] = (int32_t)rows.size();
        rows.insert(rows.end(), rows_of[s].begin(), rows_of[s].end());
        most = std::max(most, (int32_t)rows_of[s].size());
    }
    off[rows_of.size()] = (int32_t)rows.size();
    return most;
}

// chord: the medium chords of the columns (pl.chord), needed only while the plan is built
static int planar_tables(tvam_plan* p, const std::vector<float2>& cs, TvamDevBuf<float4>& chord) {
    const tvam_desc& d = p->desc;
    const TvamConsts& k = p->k;
    // occluders end segments at z-dependent points: rows no longer share a path
    if (!d.regular_sampling || (d.flags & TVAM_FLAG_NO_PLANAR) || p->empty || d.n_occluder_tris > 0) return 0;
    std::vector<std::vector<int32_t>> rows_of(k.nz);
    // a square vial's inner cuboid is lower than its outer one (vial_hz_int): a planar ray between
    // the two heights crosses glass alone and deposits nothing (tvam_segment_square's inner hit
    // fails its z test), so such a row shares no column chord
    const float row_half = d.vial_type == TVAM_VIAL_SQUARE ? std::min(k.vial_half_h, k.vial_hz_int) : k.vial_half_h;
    for (int rc = 0; rc < d.crop_y; ++rc) {
        float yc;
        const int s = regular_row_slice(d, k, rc, yc);
        if (s < 0 || s >= k.nz || !(yc >= -row_half && yc <= row_half)) continue;  // misses grid / vial / slab
        if (!(std::fabs(yc) <= 0.7f * d.vial_r)) return 0;  // spawn offset would depend on z
        rows_of[s].push_back(rc);
    }
    std::vector<int32_t> off, rows;
    p->pl.max_rows_slice = rows_csr(rows_of, off, rows);
    p->planar_fz = tvam_knob("TVAM_PLANAR_FWD_Z", 0);  // 0: chosen from the slab depth (planar_fwd_setup)
    // adjoint slices per workgroup: 8 (one march gathers 8 slices: measured 5.2 -> 3.9 ms on
    // config 2 with 1024-thread workgroups and 45 x 45 tiles), 4 for films under 8 slices
    // (TVAM_PLANAR_ADJ_Z: 4 = the tile adjoint at 4 slices, 8 / 16 = the list adjoint's slices per workgroup)
    const int az_knob = tvam_knob("TVAM_PLANAR_ADJ_Z", 0);
    p->planar_az = az_knob == 4 || k.nz < 8 ? 4 : 8;
    if (p->planar_fz != 8 && p->planar_fz != 16 && p->planar_fz != 24 && p->planar_fz != 28 && p->planar_fz != 32 &&
        p->planar_fz != 40 && p->planar_fz != 48 && p->planar_fz != 52 && p->planar_fz != 60)
        p->planar_fz = 0;
    const int ns = (int)cs.size();
    int32_t mrc = 0;
    for (int z0 = 0; z0 < k.nz; z0 += p->planar_az)
        mrc = std::max<int32_t>(mrc, off[std::min(z0 + p->planar_az, k.nz)] - off[z0]);
    p->pl.ns = ns;
    p->pl.max_rows_chunk = mrc;
    p->planar_rz = 4;
    p->pl.adj_pitch = p->tiles.tsx + 2;
    p->pl.rayfwd_pitch = p->pl.adj_pitch;
    // Refracted rays are not parallel, and a DMD much finer than the voxels
    // overflows the voxel-driven forward's column window: there the forward
    // is ray-driven like the adjoint (one record per (angle, column), shared
    // by all slices).
    p->planar_fwd = !p->cyl && !(d.flags & TVAM_FLAG_RAY_FWD);
    std::vector<float4> fwd_ang_h;  // host staging of the forward tables
    std::vector<int32_t> fwd_cb_h;
    if (p->planar_fwd && !planar_fwd_setup(p, cs, off, fwd_ang_h, fwd_cb_h)) p->planar_fwd = false;
    if (tvam_planar_adj_lds(p->pl, p->tiles, p->planar_az) > 160 * 1024) p->planar_az = 4;
    if (tvam_planar_adj_lds(p->pl, p->tiles, p->planar_az) > 160 * 1024) return 0;  // tile too large: general path
    {
        // Split each tile's ray list over up to 8 workgroups until there are >= ~16K in
        // all: a thin slab (z-slab sharding) leaves few (tile, chunk) workgroups for 256
        // CUs, and even the full film (10K at 400^3) ends with a ragged last round
        // (measured 5.30 -> 5.20 ms at split 2 on config 2).  1024-thread workgroups each
        // reload a 71 KB gradient tile, so they aim at half as many: >= ~8K (config 2:
        // split 3 instead of 5, adjoint 3.98 -> 3.72 ms; split 8: 4.29 ms).  At most 4: the thin
        // slabs of 4 / 8 z-slab ranks (split 8 by the rule) measured adjoint 1.15 / 0.63 ms at
        // split 8, 1.01 / 0.57 ms at 4, 1.00 / 0.59 ms at 2 (profiles/r03/s2/slab_split_ab.jsonl)
        // 1024 threads at Z = 8: the 71 KB tile admits 2 workgroups per CU = 8 waves per SIMD
        const int ant = tvam_knob("TVAM_ADJ_NT", p->planar_az >= 8 ? 1024 : 512);
        p->pl.adj_nt = ant == 1024 ? 1024 : 512;
        const int64_t want = p->pl.adj_nt >= 1024 ? 8192 : 16384;
        const int64_t nwg = (int64_t)p->tiles.ntx * p->tiles.nty * ((k.nz + p->planar_az - 1) / p->planar_az);
        int split = (int)std::min<int64_t>(4, std::max<int64_t>(1, (want + nwg - 1) / std::max<int64_t>(nwg, 1)));
        const int es = tvam_knob("TVAM_ADJ_SPLIT", 0);
        if (es >= 1 && es <= 64) split = es;
        p->pl.adj_split = split;
        p->pl.rayfwd_nt = 512;
    }
    if (tvam_planar_rayfwd_lds(p->pl, p->tiles, p->planar_rz) > 160 * 1024) p->planar_rz = 4;
    if (tvam_planar_rayfwd_lds(p->pl, p->tiles, p->planar_rz) > 160 * 1024) return 0;
    int rc;
    const size_t nrec = (size_t)std::max(ns, 1) * d.crop_x;
    hipError_t e;
    if ((rc = tvam_upload(p->pl_slice_off, off)) || (rc = tvam_upload(p->pl_slice_rows, rows))) return rc;
    if (p->planar_fwd) {
        // the forward's scalar loads read two angles' constants at a time: pad both tables so the pair
        // of the last angle stays inside its allocation
        fwd_ang_h.resize(fwd_ang_h.size() + 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        fwd_cb_h.resize(fwd_cb_h.size() + 2, 0);
        if ((rc = tvam_upload(p->pl_fwd_ang, fwd_ang_h)) || (rc = tvam_upload(p->pl_fwd_cb, fwd_cb_h))) return rc;
    }
    p->pl.fwd_parts = 1;
    if (p->planar_fwd && (rc = fwd_buffers(p))) return rc;
    if ((e = p->pl_vox.alloc(nrec)) != hipSuccess || (e = p->pl_rec_f.alloc(nrec)) != hipSuccess ||
        (e = p->pl_rec_i.alloc(nrec)) != hipSuccess || (p->cyl && (e = p->pl_rec_g.alloc(nrec)) != hipSuccess) ||
        (e = p->amax.alloc((size_t)std::max(ns, 1))) != hipSuccess || (e = p->fscale.alloc(2)) != hipSuccess)
        return tvam_hip_fail(e, "hipMalloc (planar tables)");
    // refracting vial: the voxel-driven forward over per-column chords (tvam_refr_model_kernel)
    const bool try_refr = p->cyl && !(d.flags & TVAM_FLAG_RAY_FWD) && ns > 0;
    if (try_refr && ((e = p->pl_vox2.alloc(nrec)) != hipSuccess || (e = chord.alloc(nrec)) != hipSuccess))
        return tvam_hip_fail(e, "hipMalloc (refracted forward tables)");
    p->bind();
    p->pl.chord = chord.get();
    if (ns > 0) {
        if ((e = tvam_launch_planar_rays(k, p->pl, nullptr)) != hipSuccess) return tvam_hip_fail(e, "planar ray table");
        if ((e = hipDeviceSynchronize()) != hipSuccess) return tvam_hip_fail(e, "planar ray table");
        // A column whose DDA starts with a frozen axis (sensor.py:358, see tvam_frozen_kernel) leaves
        // its chord; the planar kernels cannot follow it, so such a plan runs the per-ray tile path
        // (none occurs in the BASELINE configs under regular sampling).
        std::vector<int32_t> ri((size_t)ns * k.crop_x);
        if ((e = hipMemcpy(ri.data(), p->pl.rec_i, ri.size() * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess)
            return tvam_hip_fail(e, "hipMemcpy");
        for (int32_t v : ri)
            if (v == -2) return 0;
    }
    if (try_refr && (rc = refr_fwd_setup(p, off))) return rc;
    // the adjoint over slice-invariant visit lists (tvam_adjlist.hip), when they fit in a quarter of
    // the free device memory (config 2: ~0.5 GB); else the tile adjoint re-derives the visits.
    // Groups = (tile, step quadrant, part), parts until the grid holds >= 8K workgroups.
    p->pl.adjl_ngroups = 0;
    if (p->planar_az == 8 && ns > 0 && tvam_knob("TVAM_ADJ_LISTS", 1)) {
        // 16 slices per workgroup (one per CU) on deep films, 8 (two per CU) on thin ones: the
        // 50-slice slabs of 8 ranks ran 0.68 ms at 16 (four chunks, the last 2 slices deep) and
        // 0.47 ms at 8; 400 slices 3.20 ms at 16, 3.29 at 8 (profiles/r05/slab_adjoint_z/)
        p->pl.adjl_z = tvam_knob("TVAM_ADJL_Z", az_knob == 8 || k.nz < 256 ? 8 : 16) == 8 ? 8 : 16;
        const int64_t nwg4 = (int64_t)p->tiles.ntx * p->tiles.nty * 4 * ((k.nz + p->pl.adjl_z - 1) / p->pl.adjl_z);
        // built by the first adjoint call (ensure_adj_lists): a forward-only plan (final_render) never
        // pays for them
        p->adjl_parts = (int)std::min<int64_t>(4, std::max<int64_t>(1, (4096 + nwg4 - 1) / std::max<int64_t>(nwg4, 1)));
        p->adjl_pending = true;
    }
    p->planar = true;
    return 0;
}

static int planar_setup(tvam_plan* p, const std::vector<float2>& cs) {
    TvamDevBuf<float4> chord;
    const int rc = planar_tables(p, cs, chord);
    p->pl.chord = nullptr;
    if (!p->planar) p->planar_fwd = false;  // the planar path was given up after the forward's tables were chosen
    return rc;
}


// Buffers of the voxel-driven forward (straight or refracted): angle parts of thin slabs and
// the slice-binned patterns.
static int fwd_buffers(tvam_plan* p) {
    const tvam_desc& d = p->desc;
    const TvamConsts& k = p->k;
    const int ns = p->pl.ns;
    hipError_t e;
    // A thin slab leaves few (16x16 tile, slice chunk) workgroups, each running
    // every angle: at 3 resident workgroups per CU, 1250 of them (400^2 film,
    // 50 slices) fill 1.6 rounds of the 768 slots.  Split the angles into parts
    // until >= 4 rounds; the partial doses are summed in fixed order.
    const int tw = 16;
    const int64_t nwg = (int64_t)((k.res[0] + tw - 1) / tw) * ((k.res[1] + 15) / 16) *
                        ((k.nz + p->planar_fz - 1) / p->planar_fz);
    int parts = (int)std::min<int64_t>(4, std::max<int64_t>(1, (4 * 768 + nwg - 1) / std::max<int64_t>(nwg, 1)));
    const int ep = tvam_knob("TVAM_FWD_PARTS", 0);
    if (ep >= 1 && ep <= 16) parts = ep;
    parts = std::max(1, std::min(parts, ns));
    if (parts > 1) {
        const size_t n = (size_t)parts * k.nz * k.res[0] * k.res[1];
        if ((e = p->pl_part.alloc(n)) != hipSuccess) return tvam_hip_fail(e, "hipMalloc (forward parts)");
    }
    p->pl.fwd_parts = parts;
    // Slice-binned patterns ([angle][pad + column][slice], tvam_slice_bin_kernel): the
    // forward stages each window column's Z slices with 16-byte loads and stores
    const int Z = p->planar_fz;
    const int nq = (p->pl.ncmax * (Z / 4) + 255) / 256;
    if (tvam_knob("TVAM_FWD_BIN", 1) && nq <= 2 && ns > 0) {
        if (p->pl.fwd_ab > 2 || (nq == 2 && p->pl.fwd_ab != 2)) p->pl.fwd_ab = 2;  // the instantiated variants
        p->pl.bin_pad = p->pl.ncmax;
        p->pl.bin_nz = (k.nz + Z - 1) / Z * Z;
        const size_t n = (size_t)ns * (d.crop_x + 2 * p->pl.bin_pad) * p->pl.bin_nz;
        if ((e = p->pl_bin.alloc(n)) != hipSuccess) return tvam_hip_fail(e, "hipMalloc (binned patterns)");
        if ((e = hipMemset(p->pl_bin.get(), 0, n * sizeof(float))) != hipSuccess)
            return tvam_hip_fail(e, "hipMemset (binned patterns)");
        p->pl.fwd_pf = nq;
    }
    // binned slabs staged by LDS-DMA where the window fits (tvam_planar_fwd_dma_ok; wider windows
    // keep the register staging)
    p->bind();
    p->pl.fwd_dma = tvam_planar_fwd_dma_ok(p->pl, Z) ? 1 : 0;
    return 0;
}


// Slices per workgroup of the voxel-driven forward: the fewest padded slice-passes
// ceil(nz / Z) * (Z + 12) (the +12 prices the per-angle candidate geometry and staging shared by
// the Z slices), register-staged depths (windows the LDS-DMA staging cannot take) priced 25 %
// higher, among the depths whose staging fits.  With the DMA staging, Z = 52 on 400-slice films
// (8 chunks; Z = 60, 7 chunks, measured a tie: kernel 2294 against 2306 us, its 420-slice binning
// 110 against 93 us, profiles/r06/; round 5: Z = 52 2.68, 40 2.72, 32 2.81 ms, profiles/r05/fwd_depth/),
// and Z = 60 / 48 on films of <= 60 / 48 slices (the slabs of 8 ranks, 48-57 slices: one chunk).
// Returns false when none fits.
static int choose_fwd_z(tvam_plan* p) {
    const TvamConsts& k = p->k;
    if (p->planar_fz == 0) {
        int best = 8;
        int64_t bcost = INT64_MAX;
        const bool deep = tvam_knob("TVAM_FWD_BIN", 1) != 0;
        for (int Z : {60, 52, 48, 40, 32, 28, 24, 16, 8}) {
            if ((Z > 32 && !deep) || !tvam_planar_fwd_fits(p->pl, Z)) continue;
            if (Z == 60 && k.nz > 60) continue;  // one-chunk slabs only (400 slices: a tie with 52, binning +15 %)
            const int64_t cost =
                (int64_t)((k.nz + Z - 1) / Z) * (Z + 12) * (deep && tvam_planar_fwd_dma_window(p->pl, Z) ? 4 : 5);
            if (cost < bcost) bcost = cost, best = Z;
        }
        p->planar_fz = best;
    }
    for (int Z : {60, 52, 48, 40, 32, 28, 24, 16, 8})  // the deepest instantiated depth <= the choice that fits
        if (Z <= p->planar_fz && tvam_planar_fwd_fits(p->pl, Z)) {
            p->planar_fz = Z;
            break;
        }
    return tvam_planar_fwd_fits(p->pl, p->planar_fz) ? 1 : 0;
}

// Refracted voxel-driven forward (after the planar ray table, with pl.chord filled): the
// per-angle run of columns whose chords reach the medium (contiguous, else no voxel-driven
// forward), the per-(tile, angle) chord-index models and the staged window width.  Leaves
// planar_fwd false (the ray-driven forward serves) when the tables do not fit.
static int refr_fwd_setup(tvam_plan* p, const std::vector<int32_t>& off) {
    const tvam_desc& d = p->desc;
    const TvamConsts& k = p->k;
    const int ns = p->pl.ns;
    hipError_t e;
    std::vector<float4> vox((size_t)ns * d.crop_x);
    if ((e = hipMemcpy(vox.data(), p->pl.vox, vox.size() * sizeof(float4), hipMemcpyDeviceToHost)) != hipSuccess)
        return tvam_hip_fail(e, "hipMemcpy");
    std::vector<int2> range(ns);
    for (int a = 0; a < ns; ++a) {
        int c0 = -1, c1 = -2;
        for (int c = 0; c < d.crop_x; ++c)
            if (vox[(size_t)a * d.crop_x + c].z >= 0.0f) {
                if (c0 < 0) c0 = c;
                if (c1 >= 0 && c1 != c - 1) return 0;  // a gap in the run: the bisection needs one
                c1 = c;
            }
        range[a] = make_int2(c0, c1);
    }
    // The chord-index model needs chords that do not cross inside the grid: every chord's end
    // points must lie on one side of its predecessor's line, the same side for the whole angle
    // (strong refraction can fold the beam; the ray-driven forward then serves).
    {
        std::vector<float4> chord((size_t)ns * d.crop_x);
        if ((e = hipMemcpy(chord.data(), p->pl.chord, chord.size() * sizeof(float4), hipMemcpyDeviceToHost)) != hipSuccess)
            return tvam_hip_fail(e, "hipMemcpy");
        for (int a = 0; a < ns; ++a) {
            int orient = 0;
            for (int c = range[a].x; c < range[a].y; ++c) {
                const float4 A = chord[(size_t)a * d.crop_x + c], B = chord[(size_t)a * d.crop_x + c + 1];
                const double tb = vox[(size_t)a * d.crop_x + c + 1].z;
                const double pts[2][2] = {{B.x, B.y}, {B.x + tb * B.z, B.y + tb * B.w}};
                for (const auto& q : pts) {
                    const double sd = (q[0] - A.x) * (double)A.w - (q[1] - A.y) * (double)A.z;
                    const int sg = sd > 0.0 ? 1 : (sd < 0.0 ? -1 : 0);
                    if (sg == 0 || (orient != 0 && sg != orient)) return 0;
                    orient = sg;
                }
            }
        }
    }
    const int ntiles = ((k.res[0] + 15) / 16) * ((k.res[1] + 15) / 16);
    const size_t nm = (size_t)ntiles * ns;
    TvamDevBuf<int2> d_range;
    TvamDevBuf<int32_t> d_need;
    int rc = tvam_upload(d_range, range);
    if (rc) return rc;
    if ((e = p->pl_fwd_model.alloc(2 * nm)) != hipSuccess || (e = d_need.alloc(nm)) != hipSuccess)
        return tvam_hip_fail(e, "hipMalloc (refracted forward models)");
    float4* d_model = p->pl_fwd_model.get();
    e = tvam_launch_refr_model(k, p->pl, d_range.get(), d_model, d_need.get(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<int32_t> need(nm);
    std::vector<float4> mdl(2 * nm);
    if (e == hipSuccess) e = hipMemcpy(need.data(), d_need.get(), nm * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(mdl.data(), d_model, 2 * nm * sizeof(float4), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return tvam_hip_fail(e, "refracted forward models");
    int ncm = 1, ncmax_c = 1;
    for (size_t i = 0; i < nm; ++i) {
        int nc;
        std::memcpy(&nc, &mdl[2 * i + 1].y, sizeof(int));
        ncm = std::max(ncm, need[i]);
        ncmax_c = std::max(ncmax_c, nc);
        // windows wholly outside the crop stage only the binned patterns' zero pads
        int cb;
        std::memcpy(&cb, &mdl[2 * i + 1].z, sizeof(int));
        (void)cb;
    }
    TvamPlanar save = p->pl;
    p->pl.fwd_refr = 1;
    p->pl.ncmax = ncm;
    p->pl.fwd_nc = ncmax_c;
    p->pl.fwd_ab = 2;
    p->pl.fwd_model = d_model;
    {
        bool multi = false;
        for (int z = 0; z < k.nz; ++z) multi |= off[z + 1] - off[z] > 1;
        p->pl.fwd_multi = multi ? 1 : 0;
    }
    // clamp windows into the binned patterns' zero pads (bin_pad = ncmax on either side)
    bool changed = false;
    for (size_t i = 0; i < nm; ++i) {
        int cb;
        std::memcpy(&cb, &mdl[2 * i + 1].z, sizeof(int));
        const int cl = std::min(std::max(cb, -ncm), (int)d.crop_x);
        if (cl != cb) {
            std::memcpy(&mdl[2 * i + 1].z, &cl, sizeof(int));
            changed = true;
        }
    }
    if (changed && (e = hipMemcpy(d_model, mdl.data(), 2 * nm * sizeof(float4), hipMemcpyHostToDevice)) !=
                       hipSuccess)
        return tvam_hip_fail(e, "hipMemcpy");
    if (!choose_fwd_z(p)) {
        p->pl = save;
        (void)p->pl_fwd_model.reset();
        return 0;
    }
    const int nq = (p->pl.ncmax * (p->planar_fz / 4) + 255) / 256;
    p->pl.fwd_pf = nq;
    p->planar_fwd = true;
    if ((rc = fwd_buffers(p))) return rc;
    if (!p->pl.fwd_bin) return tvam_fail(TVAM_ERR_INVALID, "refracted voxel-driven forward needs the binned patterns");
    return 0;
}

// Voxel-driven forward tables (straight rays); false when the DMD is too fine
// for the staged column window.
static bool planar_fwd_setup(tvam_plan* p, const std::vector<float2>& cs, const std::vector<int32_t>& off,
                             std::vector<float4>& fwd_ang_h, std::vector<int32_t>& fwd_cb_h) {
    const tvam_desc& d = p->desc;
    const TvamConsts& k = p->k;
    const int ns = (int)cs.size();
    // Forward (voxel-driven) tables.  Per angle, in the kernel's fp32 ops:
    // u(X, Y) = X * (s du) + Y * (-c du) + u0 is the crop column whose ray has
    // lateral coordinate X s - Y c (common.py:96-99: x_c = W a (0.5 - u));
    // w = half the voxel's lateral width in columns + the spawn-offset margin.
    // A voxel's candidates are the NC columns from ceil(u - w) on; every
    // (16x16 tile, angle) stages a window of ncmax columns from fwd_cb.
    // The spawn offset moves a planar ray's line sideways by at most its length
    // (1 + max|p|) * RayEpsilon, max|p| = r on the vial wall (|p_z| <= 0.7 r here).
    const double marg_u = 1.5 * (1.0 + (double)d.vial_r) * (double)TVAM_RAY_EPS * (double)d.res_x / (double)k.ex + 1e-3;
    const float du = -(float)d.res_x / k.ex;
    const float u0 = 0.5f * (float)d.res_x - 0.5f - (float)d.crop_offset_x;
    std::vector<float4> fang(2 * (size_t)std::max(ns, 1));
    double wmax = 0.0;
    for (int i = 0; i < ns; ++i) {
        const float c = cs[i].x, sn = cs[i].y, dxr = -c, dyr = -sn;
        const int fl = (std::fabs(dxr) > 1e-8f ? 1 : 0) | (std::fabs(dyr) > 1e-8f ? 2 : 0);
        const float w = 0.5f * (k.h[0] * std::fabs(sn) + k.h[1] * std::fabs(c)) * std::fabs(du) + (float)marg_u;
        int32_t flb = fl;
        float flf;
        std::memcpy(&flf, &flb, sizeof(flf));
        fang[2 * (size_t)i] = make_float4(sn * du, -c * du, 1.0f / dxr, 1.0f / dyr);
        fang[2 * (size_t)i + 1] = make_float4(w, flf, 0.0f, 0.0f);
        wmax = std::max(wmax, (double)w);
    }
    const int nc = (int)std::floor(2.0 * wmax + 1e-3) + 1;
    // per (16 px x 16 tile, angle): the first staged column and the window width that holds every
    // voxel's candidates (px = 2: 32 x 16 tiles of voxel pairs)
    auto windows = [&](std::vector<int32_t>& fcb) {
        const int tw = 16;
        const int ntx = (k.res[0] + tw - 1) / tw, nty = (k.res[1] + 15) / 16;
        fcb.assign((size_t)ntx * nty * std::max(ns, 1), 0);
        int need = 0;
        for (int t = 0; t < ntx * nty; ++t) {
            const int bx = t % ntx, by = t / ntx;
            const double xc0 = (double)k.bmin[0] + (bx * tw + 0.5) * k.h[0], xc1 = xc0 + (tw - 1.0) * k.h[0];
            const double yc0 = (double)k.bmin[1] + (by * 16 + 0.5) * k.h[1], yc1 = yc0 + 15.0 * k.h[1];
            for (int i = 0; i < ns; ++i) {
                const double A = fang[2 * (size_t)i].x, B = fang[2 * (size_t)i].y, w = fang[2 * (size_t)i + 1].x;
                const double uc[4] = {xc0 * A + yc0 * B, xc1 * A + yc0 * B, xc0 * A + yc1 * B, xc1 * A + yc1 * B};
                const double umin = *std::min_element(uc, uc + 4) + u0, umax = *std::max_element(uc, uc + 4) + u0;
                const int cb = (int)std::floor(umin - w) - 1;  // 1 column of slack for fp32 rounding in the kernel
                fcb[(size_t)t * ns + i] = cb;
                need = std::max(need, (int)std::ceil(umax - w) + 1 + nc - cb);
            }
        }
        // a window wholly outside the crop stages only zero columns: clamp it into the
        // slice-binned patterns' zero pads (ncmax columns either side)
        for (auto& cb : fcb) cb = std::min(std::max(cb, -need), (int)d.crop_x);
        return need;
    };
    std::vector<int32_t> fcb;
    const int need = windows(fcb);
    p->pl.marg_u = (float)marg_u;
    p->pl.u0 = u0;
    p->pl.fwd_nc = nc;
    p->pl.ncmax = need;
    {
        bool multi = false;
        for (int z = 0; z < k.nz; ++z) multi |= off[z + 1] - off[z] > 1;
        p->pl.fwd_multi = multi ? 1 : 0;
    }
    p->pl.fwd_ab = 2;  // two angles per barrier (4.34 -> 3.80 ms on config 2)
    if (!choose_fwd_z(p)) return false;
    p->pl.fwd_pf = (p->pl.ncmax * p->planar_fz + 255) / 256 <= 2 ? 2 : 4;
    fwd_ang_h = std::move(fang);
    fwd_cb_h = std::move(fcb);
    return true;
}


// Slot lists behind a refracting (cylindrical) vial.  A column's rays are no
// longer one straight line per angle: each sub-pixel position u is traced
// through the glass (tvam_segment, the kernels' own fp32 code) to its medium
// chord, and the tiles within `marg` of that chord are marked.  Jittered
// sampling covers u in [0, 1] by bisection until neighbouring chords' end
// points are within a quarter voxel (or their hit status flips at a grazing /
// total-internal-reflection boundary, refined to 2^-12 of a pixel), and marks
// each pair with their end-point distance as extra margin: the chords of the
// rays in between lie in the quadrilateral the pair spans.
namespace {
struct CylChord {
    bool hit;
    double ax, ay, bx, by;
    float w;  // interface weight
};

CylChord cyl_chord(const TvamConsts& k, float c, float s, int col, float u) {
    CylChord ch{false, 0, 0, 0, 0, 0.0f};
    float xc, yc, ox, oy, oz, dx, dy, o2x, o2y, d2x, d2y, maxt, w;
    tvam_ray_camera(k, col, 0, u, 0.5f, xc, yc);
    tvam_ray_world(k, c, s, xc, 0.0f, ox, oy, oz, dx, dy);
    if (!tvam_segment(k, ox, oy, 0.0f, dx, dy, o2x, o2y, d2x, d2y, maxt, w)) return ch;
    ch.hit = true;
    ch.ax = o2x;
    ch.ay = o2y;
    ch.bx = (double)o2x + (double)maxt * d2x;
    ch.by = (double)o2y + (double)maxt * d2y;
    ch.w = w;
    return ch;
}

double chord_dist(const CylChord& a, const CylChord& b) {
    return std::max(std::hypot(a.ax - b.ax, a.ay - b.ay), std::hypot(a.bx - b.bx, a.by - b.by));
}

struct TileGrid {
    double x0, y0, wx, wy;  // origin and tile size
    int ntx, nty;
};

// Mark the tiles whose box, grown by m, meets the segment a -> b (slab clip), with the length of
// the segment inside the tile itself (0 where only the grown box meets it).  (The length in the
// grown box made a chord pair at a square vial's corner, marked with a margin of their millimetre
// apart end points, the longest of the tile, and the length classes of the other slots collapsed:
// config 5's waves held whole within-angle length ramps, 0.57 of the march lanes busy.)
template <typename F>
void mark_tiles(const TileGrid& g, const CylChord& ch, double m, F&& mark) {
    const double lox = std::min(ch.ax, ch.bx) - m, hix = std::max(ch.ax, ch.bx) + m;
    const double loy = std::min(ch.ay, ch.by) - m, hiy = std::max(ch.ay, ch.by) + m;
    const int tx0 = std::max(0, (int)std::floor((lox - g.x0) / g.wx)), tx1 = std::min(g.ntx - 1, (int)std::floor((hix - g.x0) / g.wx));
    const int ty0 = std::max(0, (int)std::floor((loy - g.y0) / g.wy)), ty1 = std::min(g.nty - 1, (int)std::floor((hiy - g.y0) / g.wy));
    const double dx = ch.bx - ch.ax, dy = ch.by - ch.ay;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const double bx0 = g.x0 + tx * g.wx - m, bx1 = g.x0 + (tx + 1) * g.wx + m;
            const double by0 = g.y0 + ty * g.wy - m, by1 = g.y0 + (ty + 1) * g.wy + m;
            double t0 = 0.0, t1 = 1.0;
            auto clip = [&](double o, double d, double lo, double hi) {
                if (std::fabs(d) < 1e-300) return o >= lo && o <= hi;
                double a = (lo - o) / d, b = (hi - o) / d;
                if (a > b) std::swap(a, b);
                t0 = std::max(t0, a);
                t1 = std::min(t1, b);
                return t0 <= t1;
            };
            if (clip(ch.ax, dx, bx0, bx1) && clip(ch.ay, dy, by0, by1)) {
                t0 = 0.0;
                t1 = 1.0;
                const bool in = clip(ch.ax, dx, bx0 + m, bx1 - m) && clip(ch.ay, dy, by0 + m, by1 - m);
                mark(ty * g.ntx + tx, in ? (t1 - t0) * std::hypot(dx, dy) : 0.0);  // the chord's length in the tile
            }
        }
}
}  // namespace

// Fixed-point bound behind a refracting vial (replaces TvamConsts::rays_per_voxel):
// the beam converges, and a cuboid splits it into sub-beams that cross, so
// more than one ray per pixel pitch of one angle may cross a voxel.  From the
// chords of an angle at 1 (regular) or 8 (jittered) positions per column, in
// column order, split into runs of neighbours that keep one side of each
// other along the whole chord (the distance of a point moving along one chord
// to the other's line is linear, so checking both end points suffices; a miss,
// a crossing or a change of side starts a new run).  A run whose least
// neighbour spacing is s contributes at most ceil(sqrt2 h / s) + 2 columns'
// rays to a voxel (a factor 2 covers the approximation); the runs add up.
// The largest interface weight scales the bound.  A tube is rotation
// invariant (one angle); a cuboid is not (every angle, the largest sum).
static float cyl_rays_per_voxel(const tvam_desc& d, const TvamConsts& k, const std::vector<float2>& cs) {
    const int sub = d.regular_sampling ? 1 : 8;
    const int ns = (int)cs.size();
    const int nang = d.vial_type == TVAM_VIAL_SQUARE ? ns : std::min(ns, 1);
    const double hxy = std::max((double)k.h[0], (double)k.h[1]);
    const double D = 2.0 * std::sqrt(2.0) * hxy;
    double wmax = 1.0, worst = 0.0;
    std::vector<CylChord> ch;
    for (int ai = 0; ai < nang; ++ai) {
        const bool sq = d.vial_type == TVAM_VIAL_SQUARE;
        const float c = sq ? cs[ai].x : 1.0f, sn = sq ? cs[ai].y : 0.0f;
        ch.clear();
        for (int col = 0; col < d.crop_x; ++col)
            for (int j = 0; j < sub; ++j)
                ch.push_back(cyl_chord(k, c, sn, d.crop_offset_x + col, ((float)j + 0.5f) / (float)sub));
        double total = 0.0, run_s = INFINITY;
        int run_sign = 0;
        bool in_run = false;
        auto close_run = [&]() {
            if (in_run) total += (run_s < INFINITY ? std::ceil(D / run_s) : 0.0) + 2.0;
            in_run = false;
            run_s = INFINITY;
            run_sign = 0;
        };
        for (size_t i = 0; i < ch.size(); ++i) {
            if (!ch[i].hit) {
                close_run();
                continue;
            }
            wmax = std::max(wmax, (double)ch[i].w);
            in_run = true;
            if (i + 1 == ch.size() || !ch[i + 1].hit) continue;
            const double dx = ch[i].bx - ch[i].ax, dy = ch[i].by - ch[i].ay, L = std::hypot(dx, dy);
            if (!(L > 1e-12)) continue;
            const double nx = -dy / L, ny = dx / L;
            const double da = (ch[i + 1].ax - ch[i].ax) * nx + (ch[i + 1].ay - ch[i].ay) * ny;
            const double db = (ch[i + 1].bx - ch[i].ax) * nx + (ch[i + 1].by - ch[i].ay) * ny;
            const int sg = da > 0.0 ? 1 : -1;
            if (!(da * db > 0.0) || (run_sign != 0 && sg != run_sign)) {
                close_run();  // the next chord crosses (or turns): a new run starts with it
                in_run = false;
                continue;
            }
            run_sign = sg;
            run_s = std::min(run_s, std::min(std::fabs(da), std::fabs(db)) * sub);
        }
        close_run();
        worst = std::max(worst, total);
    }
    if (!(worst > 0.0)) return k.rays_per_voxel;  // no chord: the straight-ray bound
    return (float)((double)ns * worst * wmax * 1.01);
}

// Within each angle a tile's slots are ordered by decreasing predicted in-tile chord length
// (the longest of the column's traced sub-pixel chords): the per-ray tile kernels' waves take 64
// consecutive slots of one angle, which then march similar lengths (the columns of an angle
// crossing a tile have a trapezoid of lengths; in column order every wave held both ramps and the
// long middle), while neighbouring lanes still read neighbouring columns' records.
static void cyl_slot_lists(const tvam_desc& d, const TvamConsts& k, const std::vector<float2>& cs, int tsx, int tsy,
                           int ntx, int nty, double marg, std::vector<std::vector<uint32_t>>& per_tile) {
    const TileGrid g{(double)k.bmin[0], (double)k.bmin[1], tsx * (double)k.h[0], tsy * (double)k.h[1], ntx, nty};
    const double hmin = std::min(k.h[0], k.h[1]);
    per_tile.assign((size_t)ntx * nty, {});
    std::vector<std::vector<float>> len_of((size_t)ntx * nty);
    std::vector<uint32_t> last((size_t)ntx * nty, 0xffffffffu);
    std::vector<size_t> angle_start((size_t)ntx * nty, 0);
    const int ns = (int)cs.size();
    const int sort_mode = tvam_knob("TVAM_SLOT_SORT", 3);
    const bool sort_len = sort_mode != 0;
    for (int i = 0; i < ns; ++i) {
        for (size_t t = 0; t < per_tile.size(); ++t) angle_start[t] = per_tile[t].size();
        for (int col = 0; col < d.crop_x; ++col) {
            const uint32_t key = ((uint32_t)i << 16) | (uint32_t)col;
            auto mark = [&](int t, double len) {
                if (last[t] != key) {
                    last[t] = key;
                    per_tile[t].push_back(key);
                    len_of[t].push_back((float)len);
                } else {
                    len_of[t].back() = std::max(len_of[t].back(), (float)len);
                }
            };
            const float c = cs[i].x, s = cs[i].y;
            const int colg = d.crop_offset_x + col;
            if (d.regular_sampling) {
                const CylChord ch = cyl_chord(k, c, s, colg, 0.5f);
                if (ch.hit) mark_tiles(g, ch, marg, mark);
                continue;
            }
            struct Iv {
                float u0, u1;
                CylChord a, b;
                int depth;
            };
            std::vector<Iv> st;
            st.push_back({0.0f, 1.0f, cyl_chord(k, c, s, colg, 0.0f), cyl_chord(k, c, s, colg, 1.0f), 0});
            while (!st.empty()) {
                Iv v = st.back();
                st.pop_back();
                if (!v.a.hit && !v.b.hit && v.depth >= 4) continue;  // both miss on a 1/16 pixel: between them too
                const bool mixed = v.a.hit != v.b.hit;
                const double dd = (v.a.hit && v.b.hit) ? chord_dist(v.a, v.b) : 0.0;
                if ((mixed || dd > 0.25 * hmin || v.depth < 4) && v.depth < 12) {
                    const float um = 0.5f * (v.u0 + v.u1);
                    const CylChord cm = cyl_chord(k, c, s, colg, um);
                    st.push_back({v.u0, um, v.a, cm, v.depth + 1});
                    st.push_back({um, v.u1, cm, v.b, v.depth + 1});
                    continue;
                }
                const double m = marg + (mixed ? hmin : dd);
                if (v.a.hit) mark_tiles(g, v.a, m, mark);
                if (v.b.hit) mark_tiles(g, v.b, m, mark);
            }
        }
        if (!sort_len) continue;
        for (size_t t = 0; t < per_tile.size(); ++t) {  // this angle's slots of tile t, longest first
            const size_t b = angle_start[t], e = per_tile[t].size();
            if (e - b < 2) continue;
            std::vector<size_t> ord(e - b);
            for (size_t j = 0; j < ord.size(); ++j) ord[j] = b + j;
            std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return len_of[t][x] > len_of[t][y]; });
            std::vector<uint32_t> keys(ord.size());
            std::vector<float> lens(ord.size());
            for (size_t j = 0; j < ord.size(); ++j) {
                keys[j] = per_tile[t][ord[j]];
                lens[j] = len_of[t][ord[j]];
            }
            std::copy(keys.begin(), keys.end(), per_tile[t].begin() + (std::ptrdiff_t)b);
            std::copy(lens.begin(), lens.end(), len_of[t].begin() + (std::ptrdiff_t)b);
        }
    }
    // TVAM_SLOT_SORT=2: length classes (eighths of the tile's longest chord) over all angles,
    // longest class first; angle order and the within-angle order are kept inside a class, so a
    // wave's lanes march similar lengths without mixing far-apart angles (config 4 first segments,
    // 40-angle shard: forward 32.0 -> 28.7 ms, adjoint 35.4 -> 30.8 ms; config 5 unchanged)
    // TVAM_SLOT_SORT=3 (default): the same classes within blocks of 16 angles, so the tiles of a
    // slice (one XCD's, tvam_tile_kernel) walk the angles in step and re-read each other's ray
    // records from L2 (config 5, 200-angle shard: adjoint 211 -> 206 ms, forward -0.5 %; config 4
    // unchanged; profiles/r05/ab_slot_blocks/)
    const int ablk = sort_mode == 3 ? std::max(1, tvam_knob("TVAM_SLOT_BLOCK", 16)) : (1 << 30);
    if ((sort_mode == 2 || sort_mode == 3) && !d.regular_sampling)  // (the planar adjoint keeps the per-angle order: 3.9 -> 8.2 ms)
        for (size_t t = 0; t < per_tile.size(); ++t) {
            const size_t n = per_tile[t].size();
            if (n < 2) continue;
            const float lmax = *std::max_element(len_of[t].begin(), len_of[t].end());
            if (!(lmax > 0.0f)) continue;
            std::vector<int> cls(n);
            for (size_t j = 0; j < n; ++j)
                cls[j] = std::min(7, (int)(8.0f * len_of[t][j] / lmax)) - 8 * (int)((per_tile[t][j] >> 16) / (uint32_t)ablk);
            std::vector<size_t> ord(n);
            for (size_t j = 0; j < n; ++j) ord[j] = j;
            std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return cls[x] > cls[y]; });
            std::vector<uint32_t> keys(n);
            for (size_t j = 0; j < n; ++j) keys[j] = per_tile[t][ord[j]];
            per_tile[t].swap(keys);
        }
    for (auto& v : len_of) std::vector<float>().swap(v);
}

// n_occ and the bounding box of the occluder triangles `tri` (TvamConsts::occ itself is the caller's).
static void occ_bounds(TvamConsts& k, const float* tri, int32_t n) {
    k.n_occ = n;
    for (int a = 0; a < 3; ++a) {
        k.occ_lo[a] = TVAM_INF;
        k.occ_hi[a] = -TVAM_INF;
    }
    for (size_t i = 0; i < 9 * (size_t)n; ++i) {
        k.occ_lo[i % 3] = std::min(k.occ_lo[i % 3], tri[i]);
        k.occ_hi[i % 3] = std::max(k.occ_hi[i % 3], tri[i]);
    }
}

// Plan creation, step by step.  Mesh upload: the target mesh (surface-aware films, TvamConsts::tgt)
// and the occluder triangles with their bounding box (TvamConsts::occ).
static int upload_meshes(tvam_plan* p) {
    const tvam_desc& d = p->desc;
    int rc;
    if (p->surface) {
        std::vector<float> tri(d.target_tris, d.target_tris + 9 * (size_t)d.n_target_tris);
        if ((rc = tvam_upload(p->tgt, tri))) return rc;
        p->k.n_tgt = d.n_target_tris;
    }
    if (d.n_occluder_tris > 0) {
        std::vector<float> tri(d.occluder_tris, d.occluder_tris + 9 * (size_t)d.n_occluder_tris);
        if ((rc = tvam_upload(p->occ, tri))) return rc;
        occ_bounds(p->k, tri.data(), d.n_occluder_tris);
    }
    p->bind();
    return 0;
}

// Tile geometry: the LDS-resident xy tile of one z-slice.
static int tile_geometry(tvam_plan* p) {
    const tvam_desc& d = p->desc;
    const TvamConsts& k = p->k;
    TvamTiles& t = p->tiles;
    auto pick = [&](int res) {
        // measured optima: the planar adjoint (regular sampling, 8 interleaved slices in LDS) at
        // <= 48 (45 at 400^3: two 71 KB tiles per CU); the per-ray tile kernels of the jittered
        // configs at 73 (config 5, 800^3: 11 tiles of 73 -> 3.15 s per iteration vs 3.35 s at 13
        // tiles of 62, 3.24 s at 80, 3.50 s at 89; config 4: 6 tiles of 67 within 1 % of 5 of 80)
        int ts = d.tile > 0 ? d.tile : (d.regular_sampling && !(d.flags & TVAM_FLAG_NO_PLANAR) ? 48 : 73);
        int nt = (res + ts - 1) / ts;
        return (res + nt - 1) / nt;
    };
    t.tsx = pick(k.res[0]), t.tsy = pick(k.res[1]);
    t.ntx = (k.res[0] + t.tsx - 1) / t.tsx, t.nty = (k.res[1] + t.tsy - 1) / t.tsy;
    t.n_shard = k.a1 - k.a0;
    p->ntiles = t.ntx * t.nty;
    // tile (+ guard band) + reduction scratch + per-angle max |p|
    p->lds_bytes = (size_t)TVAM_TILE_PITCH(t.tsx) * (t.tsy + 2) * sizeof(float) + 16 * sizeof(float) +
                   (size_t)t.n_shard * sizeof(float);
    if (p->lds_bytes > 160 * 1024) return tvam_fail(TVAM_ERR_INVALID, "tile too large for LDS; lower tvam_desc.tile");
    return 0;
}

// Per-angle tables: the rotation (motion.py:26-36) and the DDA stepping of d = (-c, -s)
// (sensor.py:343, :357-360).
static void angle_tables(const tvam_desc& d, const TvamConsts& k, std::vector<float2>& cs, std::vector<float4>& ang) {
    const int ns = k.a1 - k.a0;
    cs.resize(ns);
    ang.resize(ns);
    for (int i = 0; i < ns; ++i) {
        float time = (float)(k.a0 + i) / (float)d.n_patterns;
        float alpha = TVAM_TWO_PI * time;
        if (d.clockwise) alpha = -alpha;
        cs[i] = make_float2(cosf(alpha), sinf(alpha));
        float dir[2] = {-cs[i].x, -cs[i].y}, ts[2], st[2];
        for (int a = 0; a < 2; ++a) {
            int step = dir[a] > 0.0f ? 1 : -1;
            bool valid = fabsf(dir[a]) > 1e-8f;
            ts[a] = valid ? (k.h[a] / dir[a]) * (float)step : TVAM_INF;
            st[a] = (float)step;
        }
        ang[i] = make_float4(ts[0], ts[1], st[0], st[1]);
    }
}

// Row lists: the DMD rows feeding each slice.  A ray's height is y_c of its row (+ jitter); its
// slice is the DDA start voxel z (tvam_slice_of); local slice s of the slab = global slice k.z0 + s.
static std::vector<std::vector<int32_t>> row_lists(const tvam_desc& d, const TvamConsts& k) {
    std::vector<std::vector<int32_t>> rows_of(k.nz);
    for (int rc = 0; rc < d.crop_y; ++rc) {
        if (d.regular_sampling) {
            float yc;
            const int s = regular_row_slice(d, k, rc, yc);
            if (s >= 0 && s < k.nz) rows_of[s].push_back(rc);
        } else {
            const int row = d.crop_offset_y + rc;
            // jittered rows: a ray's height yc(jy) is monotone in jy in fp32 (tvam_ray_camera), and so is
            // its slice (int)((yc - bmin) / h) (tvam_slice_of), so the slices of the sampler's jy in
            // [0, 1 - 2^-23] (TvamPcg::next_float) lie between those of its two ends, computed with the
            // kernels' own fp32 expressions (a slice list with a +-1 margin made two of every three row
            // slots of the tile kernels idle at 1:1 rows; jy = 1 itself, never drawn, listed a row in
            // the next slice wherever row and slice boundaries coincide)
            float xc, ytop, ybot;
            tvam_ray_camera(k, 0, row, 0.5f, 0.0f, xc, ytop);
            tvam_ray_camera(k, 0, row, 0.5f, 0.99999988f, xc, ybot);
            if (!(ytop > k.bmin[2] && ybot < k.bmax[2])) continue;  // every jittered ray misses the grid
            const float zlo = ybot > k.bmin[2] ? ybot : k.bmin[2], zhi = ytop < k.bmax[2] ? ytop : k.bmax[2];
            int s0 = (int)((zlo - k.bmin[2]) / k.h[2]), s1 = (int)((zhi - k.bmin[2]) / k.h[2]);
            s0 = std::max(k.z0, std::max(s0, 0));
            s1 = std::min(k.z0 + k.nz - 1, std::min(s1, k.res[2] - 1));
            for (int s = s0; s <= s1; ++s) rows_of[s - k.z0].push_back(rc);
        }
    }
    return rows_of;
}

// Main rows of jittered plans (TvamTiles::slice_moff): a row's main slice is its centre ray's;
// used when the row lists hold rows that only the extreme jitters take into a slice (config 5:
// 1:1 rows list two per slice, and half of the tile kernels' slots were rays of the other
// slice, tools/tile_diag.py) and 32 interior jitters of every row stay in its main slice.
// Returns false (no main-row lists) where they gain nothing or a row's interior jitters split.
static bool main_row_lists(const tvam_desc& d, const TvamConsts& k, const std::vector<std::vector<int32_t>>& rows_of,
                           std::vector<int32_t>& row_main, std::vector<int32_t>& slice_moff,
                           std::vector<int32_t>& slice_mrows) {
    if (d.regular_sampling || tvam_knob("TVAM_TILE_MAIN", 1) == 0) return false;
    row_main.assign(d.crop_y, -1);
    std::vector<std::vector<int32_t>> mrows(k.nz);
    bool split = false;
    for (int rc = 0; rc < d.crop_y && !split; ++rc) {
        float xc, yc;
        tvam_ray_camera(k, 0, d.crop_offset_y + rc, 0.5f, 0.5f, xc, yc);
        const int sg = tvam_slice_of(k, yc);
        for (int j = 0; j < 32 && !split; ++j) {
            tvam_ray_camera(k, 0, d.crop_offset_y + rc, 0.5f, ((float)j + 0.5f) / 32.0f, xc, yc);
            split = tvam_slice_of(k, yc) != sg;
        }
        if (sg >= k.z0 && sg < k.z0 + k.nz) {
            row_main[rc] = sg - k.z0;
            mrows[sg - k.z0].push_back(rc);
        }
    }
    bool gain = false;
    for (int z = 0; z < k.nz; ++z) gain = gain || mrows[z].size() < rows_of[z].size();
    if (!gain || split) return false;
    rows_csr(mrows, slice_moff, slice_mrows);
    return true;
}

// Per-tile slot lists: every (angle, DMD column) whose ray crosses the
// tile, in (angle, column) order so that consecutive lanes read
// consecutive ray records.  A collimated ray's lateral coordinate is
// l = dot(o, (s,-c,0)) = x_c; the spawn offset moves it by less than
// (1+max|p|)*RayEpsilon, covered by the margin.  (Sorting the slots by
// predicted in-tile length balances the lanes of a wave — 0.98 instead of
// 0.64 of the lanes busy in the march loop — but scatters the record reads
// and the adjoint's atomics over angles, which costs more than it gains.)
// Returns the most slots of one tile.
static int64_t slot_lists(tvam_plan* p, const std::vector<float2>& cs, std::vector<int64_t>& slot_off,
                          std::vector<uint32_t>& slots) {
    const tvam_desc& d = p->desc;
    const TvamConsts& k = p->k;
    const int tsx = p->tiles.tsx, tsy = p->tiles.tsy, ntx = p->tiles.ntx, nty = p->tiles.nty, ns = p->tiles.n_shard;
    double rmax = std::max({std::fabs((double)k.bmin[0]), std::fabs((double)k.bmax[0]), std::fabs((double)k.bmin[1]),
                            std::fabs((double)k.bmax[1]), (double)d.vial_r, (double)k.vial_half_h});
    double marg_l = 4.0 * (1.0 + rmax) * (double)TVAM_RAY_EPS;
    const double W = d.res_x, ex = k.ex;
    const double vr = d.vial_r;
    slot_off.assign((size_t)p->ntiles + 1, 0);
    int64_t max_nrt = 0;
    if (p->cyl) {
        std::vector<std::vector<uint32_t>> per_tile;
        // host tracing without occluders (device memory; they only shorten chords: a superset)
        TvamConsts kh = k;
        kh.occ = nullptr;
        kh.n_occ = 0;
        cyl_slot_lists(d, kh, cs, tsx, tsy, ntx, nty, marg_l + 1e-3 * std::min(k.h[0], k.h[1]), per_tile);
        p->k.rays_per_voxel = cyl_rays_per_voxel(d, kh, cs);
        for (int t = 0; t < p->ntiles; ++t) {
            slots.insert(slots.end(), per_tile[t].begin(), per_tile[t].end());
            slot_off[(size_t)t + 1] = (int64_t)slots.size();
            max_nrt = std::max<int64_t>(max_nrt, (int64_t)per_tile[t].size());
        }
        return max_nrt;
    }
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            int tile = ty * ntx + tx;
            double X0 = (double)k.bmin[0] + (double)(tx * tsx) * k.h[0];
            double X1 = (double)k.bmin[0] + (double)std::min((tx + 1) * tsx, k.res[0]) * k.h[0];
            double Y0 = (double)k.bmin[1] + (double)(ty * tsy) * k.h[1];
            double Y1 = (double)k.bmin[1] + (double)std::min((ty + 1) * tsy, k.res[1]) * k.h[1];
            const size_t first = slots.size();
            for (int i = 0; i < ns; ++i) {
                double c = cs[i].x, s = cs[i].y;
                double l[4] = {X0 * s - Y0 * c, X1 * s - Y0 * c, X0 * s - Y1 * c, X1 * s - Y1 * c};
                double L0 = *std::min_element(l, l + 4) - marg_l, L1 = *std::max_element(l, l + 4) + marg_l;
                L0 = std::max(L0, -vr - marg_l);
                L1 = std::min(L1, vr + marg_l);
                if (!(L0 <= L1)) continue;
                double c_lo = W * (0.5 - L1 / ex) - 1.0, c_hi = W * (0.5 - L0 / ex);
                int cl = std::max((int)std::floor(c_lo) - 1 - d.crop_offset_x, 0);
                int ch = std::min((int)std::ceil(c_hi) + 1 - d.crop_offset_x, d.crop_x - 1);
                // (column order: ordering by in-tile chord length, as behind refracting vials, made the
                // planar adjoint slower, 3.82 -> 3.96 ms on config 2)
                for (int col = cl; col <= ch; ++col) slots.push_back(((uint32_t)i << 16) | (uint32_t)col);
            }
            slot_off[(size_t)tile + 1] = (int64_t)slots.size();
            max_nrt = std::max<int64_t>(max_nrt, (int64_t)(slots.size() - first));
        }
    return max_nrt;
}

// The hierarchy over both meshes of a 'custom' vial (inner mesh first: a tie in t between the two
// goes to the inner one, tvam_segment_square's `ti <= te`), uploaded through the plan's owners.
static int upload_vial_meshes(tvam_plan* p, const float* outer, int32_t n_outer, const float* inner, int32_t n_inner) {
    std::vector<float> all(inner, inner + 9 * (size_t)n_inner);
    all.insert(all.end(), outer, outer + 9 * (size_t)n_outer);
    TvamMeshHost h;
    tvam_mesh_build(all.data(), n_inner + n_outer, h);
    // whole 16-byte rows: the kernels' LDS staging copies the tables as float4 (cn_mesh_view)
    h.tris.resize((h.tris.size() + 3) / 4 * 4, 0.0f);
    h.ids.resize((h.ids.size() + 3) / 4 * 4, 0);
    int rc;
    if ((rc = tvam_upload(p->mesh_nodes, h.nodes)) || (rc = tvam_upload(p->mesh_tris, h.tris)) ||
        (rc = tvam_upload(p->mesh_ids, h.ids)))
        return rc;
    TvamMesh& m = p->k.mesh;
    m.n_nodes = (int32_t)(h.nodes.size() / 2);
    m.n_tris = n_inner + n_outer;
    m.n_inner = n_inner;
    const size_t bytes = h.nodes.size() * sizeof(float4) + h.tris.size() * sizeof(float) + h.ids.size() * sizeof(int32_t);
    m.lds_bytes = bytes <= TVAM_MESH_LDS_BUDGET ? (int32_t)bytes : 0;
    p->bind();
    return 0;
}

// tvam_double.hip
int tvam_double_validate(const tvam_double_vial* v, float medium_ior);
TvamDouble tvam_double_consts(const tvam_double_vial& v, float medium_ior);
// tvam_insert.hip
int tvam_inserts_validate(const TvamConsts& k, const tvam_insert* ins, int32_t n);
void tvam_inserts_flatten(const tvam_insert* ins, int32_t n, std::vector<float>& tris, std::vector<float>& tri_eta);

// Dielectric occluders: one hierarchy over every insert's triangles and each triangle's eta,
// uploaded through the plan's owners.
static int upload_inserts(tvam_plan* p, const tvam_insert* inserts, int32_t n_inserts) {
    std::vector<float> tris, tri_eta;
    tvam_inserts_flatten(inserts, n_inserts, tris, tri_eta);
    int rc;
    if ((rc = upload_vial_meshes(p, tris.data(), (int32_t)tri_eta.size(), nullptr, 0))) return rc;
    return tvam_upload(p->ins_eta, tri_eta);
}

// What a create entry point or a host segment dumper was handed beside the descriptor: the kind and its payload.
struct PlanInputs {
    TvamPlanKind kind;
    const float *outer = nullptr, *inner = nullptr;  // Mesh: the two vial meshes
    int32_t n_outer = 0, n_inner = 0;
    const tvam_double_vial* dbl = nullptr;  // Double
    const tvam_insert* inserts = nullptr;   // Inserts, Reflect (which may have none)
    int32_t n_inserts = 0;
};

// The descriptor's limits (validate), then the payload's: no device call.
static int inputs_validate(const tvam_desc& d, const PlanInputs& in) {
    int rc = validate(d, in.kind);
    if (rc) return rc;
    switch (in.kind) {
    case TvamPlanKind::Plain: case TvamPlanKind::Cone: case TvamPlanKind::Traced: break;
    case TvamPlanKind::Mesh:
        if ((rc = tvam_mesh_validate("outer", in.outer, in.n_outer)) || (rc = tvam_mesh_validate("inner", in.inner, in.n_inner)))
            return rc;
        if ((int64_t)in.n_outer + in.n_inner >= (1 << 27))
            return tvam_fail(TVAM_ERR_TOO_LARGE, "the vial meshes have too many triangles");
        break;
    case TvamPlanKind::Double: return tvam_double_validate(in.dbl, d.medium_ior);
    case TvamPlanKind::Reflect:  // a glass vial needs no insert; the index-matched tube has no interface of its own and needs one
        if (in.n_inserts < 0 || (in.n_inserts > 0 && !in.inserts))
            return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_create_reflect: inserts is null");
        if (in.n_inserts == 0 && d.vial_type == TVAM_VIAL_INDEX_MATCHED)
            return tvam_fail(TVAM_ERR_INVALID, "transmission_only = 0 behind an 'index_matched' vial without inserts has no dielectric interface: create the plan with tvam_plan_create");
        if (in.n_inserts == 0) break;
        [[fallthrough]];
    case TvamPlanKind::Inserts: return tvam_inserts_validate(make_consts(d, 0, 0), in.inserts, in.n_inserts);
    }
    return 0;
}

static int plan_create(const tvam_desc& d_in, const PlanInputs& in, int device, tvam_plan** out) {
    int rc = inputs_validate(d_in, in);
    if (rc) return rc;
    tvam_desc d = d_in;
    if (in.dbl) {  // the host tables (tiles, slots) are sized by the medium's tube and the outermost one
        d.vial_r = in.dbl->r_int_outer;
        d.vial_r_ext = in.dbl->r_ext_outer;
    }
    int a0 = d.angle_begin, a1 = d.angle_end < 0 ? d.n_patterns : d.angle_end;
    if (a0 < 0 || a1 > d.n_patterns || a0 > a1) return tvam_fail(TVAM_ERR_INVALID, "invalid angle shard");

    if (a1 - a0 > 65536 || d.crop_x > 65536)  // slot entries pack (angle << 16 | column)
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "more than 65536 angles per shard or DMD columns");

    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return tvam_hip_fail(e, "hipSetDevice");

    std::unique_ptr<tvam_plan> p(new tvam_plan(in.kind, d, device));  // (an error exit destroys it on `device`)
    p->k = make_consts(d, a0, a1);
    if (in.dbl) p->k.dbl = tvam_double_consts(*in.dbl, d.medium_ior);
    if ((rc = upload_meshes(p.get())) || (rc = tile_geometry(p.get()))) return rc;
    if (in.kind == TvamPlanKind::Mesh && (rc = upload_vial_meshes(p.get(), in.outer, in.n_outer, in.inner, in.n_inner)))
        return rc;
    if (in.n_inserts > 0 && (rc = upload_inserts(p.get(), in.inserts, in.n_inserts))) return rc;

    std::vector<float2> cs;
    std::vector<float4> ang;
    angle_tables(d, p->k, cs, ang);
    const std::vector<std::vector<int32_t>> rows_of = row_lists(d, p->k);
    std::vector<int32_t> row_main, slice_moff, slice_mrows, slice_off, slice_rows;
    const bool main_rows = main_row_lists(d, p->k, rows_of, row_main, slice_moff, slice_mrows);
    p->max_rows_per_slice = rows_csr(rows_of, slice_off, slice_rows);
    std::vector<int64_t> slot_off;
    std::vector<uint32_t> slots;
    const int64_t max_nrt = slot_lists(p.get(), cs, slot_off, slots);
    // flat slot count per workgroup must fit int32 (rows * slots * spp)
    if ((int64_t)p->max_rows_per_slice * max_nrt * 64 > (int64_t)0x7fffffff)
        return tvam_fail(TVAM_ERR_TOO_LARGE, "too many rays per tile for one launch");

    if ((rc = tvam_upload(p->cs, cs)) || (rc = tvam_upload(p->slice_off, slice_off)) ||
        (rc = tvam_upload(p->slice_rows, slice_rows)) || (rc = tvam_upload(p->slots, slots)) ||
        (rc = tvam_upload(p->slot_off, slot_off)) || (rc = tvam_upload(p->ang, ang)))
        return rc;
    if ((e = p->counter.alloc(1)) != hipSuccess) return tvam_hip_fail(e, "hipMalloc");
    p->n_slots_all = (int64_t)slots.size();
    p->n_main_rows = main_rows ? (int64_t)slice_mrows.size() : 0;
    p->n_rows_all = (int64_t)slice_rows.size();
    if (main_rows && ((rc = tvam_upload(p->slice_moff, slice_moff)) || (rc = tvam_upload(p->slice_mrows, slice_mrows)) ||
                      (rc = tvam_upload(p->row_main, row_main))))
        return rc;
    p->bind();
    for (auto& r : p->rs)
        if ((e = hipEventCreateWithFlags(&r.ready, hipEventDisableTiming)) != hipSuccess)
            return tvam_hip_fail(e, "hipEventCreate");
    if (!p->surface && !p->general && (rc = planar_setup(p.get(), cs))) return rc;
    *out = p.release();
    return 0;
}

extern "C" int tvam_plan_create(const tvam_desc* desc, int device, tvam_plan** out) {
    if (!desc || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (desc->abi_version == TVAM_ABI_VERSION && desc->vial_type == TVAM_VIAL_CUSTOM)
        return tvam_fail(TVAM_ERR_INVALID, "a 'custom' vial needs its meshes: create the plan with tvam_plan_create_mesh");
    if (desc->abi_version == TVAM_ABI_VERSION && desc->vial_type == TVAM_VIAL_DOUBLE_CYLINDRICAL)
        return tvam_fail(TVAM_ERR_INVALID, "a 'double_cylindrical' vial needs its radii and IORs: create the plan with tvam_plan_create_double");
    return plan_create(*desc, PlanInputs{desc_kind(*desc)}, device, out);
}

extern "C" int tvam_plan_create_traced(const tvam_desc* desc, int device, tvam_plan** out) {
    if (!desc || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    *out = nullptr;
    return plan_create(*desc, PlanInputs{TvamPlanKind::Traced}, device, out);
}

extern "C" int tvam_plan_create_mesh(const tvam_desc* desc, const float* outer_tris, int32_t n_outer,
                                     const float* inner_tris, int32_t n_inner, int device, tvam_plan** out) {
    if (!desc || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (desc->abi_version == TVAM_ABI_VERSION && desc->vial_type != TVAM_VIAL_CUSTOM)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_create_mesh: vial_type must be TVAM_VIAL_CUSTOM");
    PlanInputs in{TvamPlanKind::Mesh};
    in.outer = outer_tris, in.n_outer = n_outer, in.inner = inner_tris, in.n_inner = n_inner;
    return plan_create(*desc, in, device, out);
}

extern "C" int tvam_plan_create_double(const tvam_desc* desc, const tvam_double_vial* vial, int device,
                                       tvam_plan** out) {
    if (!desc || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (desc->abi_version == TVAM_ABI_VERSION && desc->vial_type != TVAM_VIAL_DOUBLE_CYLINDRICAL)
        return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_create_double: vial_type must be TVAM_VIAL_DOUBLE_CYLINDRICAL");
    PlanInputs in{TvamPlanKind::Double};
    in.dbl = vial;
    return plan_create(*desc, in, device, out);
}

// Inserts: dielectric occluders walked per ray.  Reflect (transmission_only = 0): the same walk with reflection
// sampled against refraction at every dielectric interface after a path's first (tvam_insert_next<true>).
static PlanInputs insert_inputs(TvamPlanKind kind, const tvam_insert* inserts, int32_t n_inserts) {
    PlanInputs in{kind};
    in.inserts = inserts, in.n_inserts = n_inserts;
    return in;
}

extern "C" int tvam_plan_create_inserts(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts,
                                        int device, tvam_plan** out) {
    if (!desc || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    *out = nullptr;
    return plan_create(*desc, insert_inputs(TvamPlanKind::Inserts, inserts, n_inserts), device, out);
}

extern "C" int tvam_plan_create_reflect(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts,
                                        int device, tvam_plan** out) {
    if (!desc || !out) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    *out = nullptr;
    return plan_create(*desc, insert_inputs(TvamPlanKind::Reflect, inserts, n_inserts), device, out);
}

// The host tracer of a Traced plan (tvam_glass.h), ray by ray: no device call.
extern "C" int tvam_traced_segments(const tvam_desc* desc, const float* o, const float* d, int64_t n_rays,
                                    float* segs) {
    if (!desc || n_rays < 0 || (n_rays > 0 && (!o || !d || !segs))) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (validate(*desc, TvamPlanKind::Traced)) return TVAM_ERR_INVALID;  // (the message is the plan entry's)
    const TvamConsts k = make_consts(*desc, 0, 0);
    for (int64_t i = 0; i < n_rays; ++i) {
        float o2[3], d2[3], maxt, att;
        float* s = segs + 8 * i;
        if (tvam_segment_traced(k, o + 3 * i, d + 3 * i, o2, d2, maxt, att)) {
            seg_row(s, o2, d2, maxt, att);
        } else {
            for (int j = 0; j < 8; ++j) s[j] = 0.0f;
        }
    }
    return 0;
}

// The host walk of an Inserts or Reflect plan (tvam_insert.h), ray by ray: no device call.  Its scene: the descriptor's
// constants with the caller's occluder triangles, the inserts' flat tables and their hierarchy (none: an empty scene).
namespace {
struct HostInsertScene {
    TvamConsts k;
    std::vector<float> tris, tri_eta;
    TvamMeshHost mesh;
    TvamInsertScene view{};
    HostInsertScene(const tvam_desc& d, const tvam_insert* inserts, int32_t n_inserts) : k(make_consts(d, 0, 0)) {
        if (d.n_occluder_tris > 0) {
            k.occ = d.occluder_tris;
            occ_bounds(k, d.occluder_tris, d.n_occluder_tris);
        }
        if (n_inserts <= 0) return;
        tvam_inserts_flatten(inserts, n_inserts, tris, tri_eta);
        tvam_mesh_build(tris.data(), (int32_t)tri_eta.size(), mesh);
        view.mesh.nodes = mesh.nodes.data(), view.mesh.tris = mesh.tris.data(), view.mesh.ids = mesh.ids.data();
        view.mesh.n_nodes = (int32_t)(mesh.nodes.size() / 2), view.mesh.n_tris = (int32_t)tri_eta.size(), view.mesh.n_inner = 0;
        view.tri_eta = tri_eta.data();
    }
};

// u [n_rays][max_depth][4]: each loop iteration's draws (null: none, Russian roulette never acts)
template <bool REFLECT, bool MESHES>
void host_walk(const HostInsertScene& sc, const float* o, const float* d, int64_t n_rays, const float* u,
               int32_t max_segments, float* segs, int32_t* nseg) {
    for (int64_t i = 0; i < n_rays; ++i) {
        TvamInsertWalk w;
        tvam_insert_start(w, o + 3 * i, d + 3 * i);
        TvamInsertHostDraws dr{u ? u + 4 * (size_t)sc.k.max_depth * (size_t)i : nullptr};
        float* row = segs + 8 * (size_t)max_segments * (size_t)i;
        if (max_segments > 0) std::fill(row, row + 8 * (size_t)max_segments, 0.0f);
        int32_t s = 0;
        float o2[3], d2[3], maxt, att;
        while (tvam_insert_next<REFLECT, MESHES>(sc.k, sc.view, u != nullptr, dr, w, o2, d2, maxt, att)) {
            if (s < max_segments) seg_row(row + 8 * s, o2, d2, maxt, att);
            ++s;
        }
        nseg[i] = s;
    }
}
}  // namespace

extern "C" int tvam_insert_segments(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts,
                                    const float* o, const float* d, int64_t n_rays, const float* u,
                                    int32_t max_segments, float* segs, int32_t* nseg) {
    if (!desc || n_rays < 0 || max_segments < 0 || (n_rays > 0 && (!o || !d || !nseg || (max_segments > 0 && !segs))))
        return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (const int rc = inputs_validate(*desc, insert_inputs(TvamPlanKind::Inserts, inserts, n_inserts))) return rc;
    host_walk<false, true>(HostInsertScene(*desc, inserts, n_inserts), o, d, n_rays, u, max_segments, segs, nseg);
    return 0;
}

// u is required: a reflecting walk always draws.
extern "C" int tvam_reflect_segments(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts,
                                     const float* o, const float* d, int64_t n_rays, const float* u,
                                     int32_t max_segments, float* segs, int32_t* nseg) {
    if (!desc || n_rays < 0 || max_segments < 0 || (n_rays > 0 && (!o || !d || !nseg || (max_segments > 0 && !segs))))
        return tvam_fail(TVAM_ERR_INVALID, "null argument");
    if (n_rays > 0 && !u) return tvam_fail(TVAM_ERR_INVALID, "tvam_reflect_segments: u is required (a reflecting walk always draws)");
    if (const int rc = inputs_validate(*desc, insert_inputs(TvamPlanKind::Reflect, inserts, n_inserts))) return rc;
    const HostInsertScene sc(*desc, inserts, n_inserts);
    if (n_inserts > 0)
        host_walk<true, true>(sc, o, d, n_rays, u, max_segments, segs, nseg);
    else
        host_walk<true, false>(sc, o, d, n_rays, u, max_segments, segs, nseg);
    return 0;
}

extern "C" int tvam_plan_kernel_time(tvam_plan* p, int32_t enable, double* total_ms, int64_t* launches) {
    if (!p || !total_ms || !launches) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    *total_ms = 0.0;
    *launches = 0;
    std::lock_guard<std::mutex> lk(g_kt.mu);
    if (g_kt.owner && g_kt.owner != p) return tvam_fail(TVAM_ERR_INVALID, "tvam_plan_kernel_time: another plan owns the timer");
    hipError_t e = hipSuccess;
    for (size_t i = 0; e == hipSuccess && i < g_kt.n; i += 2) {  // each pair's end complete before it is read
        float ms = 0.0f;
        e = hipEventSynchronize(g_kt.ev[i + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_kt.ev[i], g_kt.ev[i + 1]);
        *total_ms += ms;
    }
    *launches = (int64_t)(g_kt.n / 2);
    if (e != hipSuccess) return tvam_hip_fail(e, "tvam_plan_kernel_time");
    g_kt.n = 0;
    g_kt.on = false;
    if (!enable) {  // measurement read: the events go with it
        kt_release();
        return 0;
    }
    {
        g_kt.owner = p;
        g_kt.device = p->device;
        while (g_kt.ev.size() < 2048) {
            hipEvent_t ev;
            if ((e = hipEventCreate(&ev)) != hipSuccess) return tvam_hip_fail(e, "hipEventCreate");
            g_kt.ev.push_back(ev);
        }
        // the plan's dominant forward kernel: the brick march of a scattering medium, else the
        // voxel-driven planar forward where it serves, else the per-ray tile forward
        // (telecentric / lens: the brick march of the binned forward, else the per-ray atomic forward)
        // (dielectric occluders: the per-ray atomic forward alone)
        g_kt.kind = tvam_kind_ray3d(p->kind)
                        ? (tvam_cone_binned(p) && !tvam_kind_inserts(p->kind) ? TVAM_KT_BRICK : TVAM_KT_CONE)
                        : (p->desc.albedo != 0.0f ? TVAM_KT_BRICK : (p->planar_fwd ? TVAM_KT_PLANAR : TVAM_KT_TILE));
        g_kt.on = true;
    }
    return 0;
}

extern "C" int tvam_row_slices(const tvam_desc* desc, int32_t* slice_of_row) {
    if (!desc || !slice_of_row) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    int rc = validate(*desc, desc_kind(*desc));
    if (rc) return rc;
    const tvam_desc& d = *desc;
    if (d.projector_type != TVAM_PROJECTOR_COLLIMATED)  // 3-D rays cross slices: no row <-> slice map
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_row_slices: the 'telecentric' / 'lens' projectors' rays leave their slice (no film slabs)");
    if (d.vial_type == TVAM_VIAL_CUSTOM)  // refracted at tilted faces, they leave it too
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_row_slices: a 'custom' vial's rays leave their slice (no film slabs)");
    if (d.vial_type == TVAM_VIAL_DOUBLE_CYLINDRICAL)  // per-ray 3-D kernels: no film slabs
        return tvam_fail(TVAM_ERR_UNSUPPORTED, "tvam_row_slices: a 'double_cylindrical' vial runs the 3-D per-ray path (no film slabs)");
    // (a descriptor meant for tvam_plan_create_traced is a planar one here when collimated, and is
    // refused above with the projector's message otherwise: that path has no film slabs either)
    const TvamConsts k = make_consts(d, 0, d.n_patterns);
    for (int r = 0; r < d.crop_y; ++r) {
        float xc, yc;
        tvam_ray_camera(k, 0, d.crop_offset_y + r, 0.5f, 0.5f, xc, yc);
        const int s = tvam_slice_of(k, yc);
        slice_of_row[r] = (s >= 0 && yc >= -k.vial_half_h && yc <= k.vial_half_h) ? s : -1;
    }
    return 0;
}

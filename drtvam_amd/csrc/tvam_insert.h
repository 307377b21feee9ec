// tvam_insert.h -- the medium segments of a ray through a resin that holds dielectric occluders
// (geometry.py:55-72 with a 'bsdf' entry: transparent inserts, the overprinting case), host and
// device.
//
// The scene: the container ('index_matched': one open tube with a null BSDF; 'cylindrical' /
// 'square': the two analytic glass surfaces of tvam_glass.h), the descriptor's black occluders, and
// the inserts: closed 'ply' meshes with face normals, wound outwards, whose exterior is the printing
// medium and which have no interior medium.  Every insert triangle carries its insert's
// eta = int_ior / ext_ior (the BSDF's own numbers, whatever the resin's IOR is).
//
// The path loop is volume.py:179-272 in transmission-only mode with a non-scattering medium, in the
// statement order of tvam_double_next.  Per iteration:
//   Russian roulette (volume.py:181-186): one draw before the intersection; it acts when
//     depth > rr_depth with q = min(0.99, attenuation): the path ends unless u < q, and the
//     attenuation takes 1 / q.  (tvam_path.h's sc_roulette, restated here for the host.)
//   the nearest hit t >= 0 over the container's surfaces (a tie of the two glass surfaces goes to the
//     inner one), then the black occluders, then the insert triangles; a later candidate wins only
//     when it is strictly nearer.  None: the path ends and a segment in progress deposits nothing
//     (cn_segment's open-end rule).
//   in the medium: the segment (p, v, [0, t]) with the current attenuation.
//   a black occluder ends the path after that deposit.
//   else the interface's transmission (tvam_transmit_world with the surface's eta; the index-matched
//     tube passes the ray unchanged; weight 0 = total internal reflection ends the path), e^{-sigma_t t}
//     after a medium segment (volume.py:263), the spawn_ray offset (1 + max|h|) RayEpsilon along the
//     normal on the side of wo, and the medium flag of si.target_medium(wo): the container's medium
//     boundary crossed inwards turns it on, an insert face crossed inwards (n . wo < 0) turns it off,
//     crossed outwards turns it on; any other crossing turns it off.
//   the BSDF's next_1d + next_2d are drawn and ignored: four draws per iteration.
// Every surface counts as depth; the loop runs while depth < max_depth.
//
// transmission_only = 0 (tvam_insert_next<REFLECT>, tvam_plan_create_reflect): the same loop with the
// BSDF's next_1d used.  At depth 0 the transmission is forced as above; at every later dielectric
// surface s1 <= F reflects (weight 1) and s1 > F refracts with weight eta_ti^2
// (tvam_dielectric_sample), so total internal reflection reflects instead of ending the path.  The
// index-matched tube and the black occluders are as above, and so is everything after the BSDF: a
// reflection off the inner wall from the resin side keeps the medium flag and starts a new segment.
// Such a walk draws its four numbers in every iteration, whether or not the roulette can act.
//
// The walk is resumable: its state is the point, the direction, the attenuation, the depth and the
// flag, and tvam_insert_next advances it to the next medium segment.  A kernel marches one segment
// at a time with one copy of its DDA.  All state is scalars: no per-thread array is indexed at run
// time (tvam_seg3d.h).
#pragma once
#include "tvam_firsthit.h"
#include "tvam_mesh.h"

struct TvamInsertWalk {
    float px, py, pz, vx, vy, vz;
    float att;
    int depth;
    bool in_medium;
};

// What a walk reads beside the plan's constants (k.mesh: the hierarchy over every insert's
// triangles; k.occ: the black occluders).
struct TvamInsertScene {
    TvamMeshView mesh;     // global memory, or a workgroup's LDS copy
    const float* tri_eta;  // [n_tris] by the triangle's index in the caller's order (TvamMeshView::ids)
};

TVAM_HD void tvam_insert_start(TvamInsertWalk& w, const float o[3], const float d[3]) {
    w.px = o[0], w.py = o[1], w.pz = o[2];
    w.vx = d[0], w.vy = d[1], w.vz = d[2];
    w.att = 1.0f;
    w.depth = 0;
    w.in_medium = false;
}

// Whether Russian roulette can act on a path of these limits at all (depth <= max_depth - 1); a
// walk that it cannot touch draws nothing.
TVAM_HD bool tvam_insert_roulette_on(int rr_depth, int max_depth) { return rr_depth < max_depth - 1; }

// The draws of a host walk: u[depth][4] of the caller, or none (roulette never acts).
struct TvamInsertHostDraws {
    const float* u;
    TVAM_HD float rr(int depth) const { return u[4 * depth]; }
    TVAM_HD float s1(int depth) const { return u[4 * depth + 1]; }  // the BSDF's next_1d (a reflecting walk)
    TVAM_HD void bsdf() const {}
};

// surface kinds of a hit
#define TVAM_INS_OUTER 0   // glass vials: air | glass
#define TVAM_INS_MEDIUM 1  // the container's medium boundary (index-matched tube, or glass | medium)
#define TVAM_INS_BLACK 2   // a black occluder
#define TVAM_INS_INSERT 3  // an insert face

// Mitsuba's dielectric::sample with both lobes enabled and TransportMode::Radiance, in world space:
// s1 <= F reflects (wo = d - 2 (d . n) n, weight 1), else the refraction of tvam_transmit_world with
// weight eta_ti^2 (the lobe's probability 1 - F cancels the Fresnel factor).  F = 1 always reflects.
TVAM_HD float tvam_dielectric_sample(float nx, float ny, float nz, float dx, float dy, float dz, float eta, float s1,
                                     float& wx, float& wy, float& wz) {
    const float cos_i = -(dx * nx + dy * ny + dz * nz);
    float cos_t, eta_ti;
    const float r = tvam_fresnel(cos_i, eta, cos_t, eta_ti);
    if (s1 <= r) {
        const float c = 2.0f * cos_i;
        wx = dx + c * nx;
        wy = dy + c * ny;
        wz = dz + c * nz;
        return 1.0f;
    }
    const float c = eta_ti * cos_i + cos_t;
    wx = eta_ti * dx + c * nx;
    wy = eta_ti * dy + c * ny;
    wz = eta_ti * dz + c * nz;
    return eta_ti * eta_ti;
}

// The walk to its next medium segment (o2, d2, [0, maxt]) of weight `weight` (the attenuation the
// segment starts with); false: the path has ended.  rr: Russian roulette is drawn (draws.rr(depth)
// per iteration, draws.bsdf() after a valid hit).  `iter` (host checks): the loop iteration of the
// deposit.
//
// REFLECT (tvam_plan_create_reflect, transmission_only = 0): after the path's first surface every
// dielectric interface samples reflection against refraction with draws.s1(depth), the BSDF's
// next_1d (tvam_dielectric_sample); total internal reflection reflects instead of ending the path.
// Such a walk always draws (rr = true).  MESHES = false: a scene without inserts, no hierarchy read.
template <bool REFLECT = false, bool MESHES = true, typename DRAWS>
TVAM_HD bool tvam_insert_next(const TvamConsts& k, const TvamInsertScene& sc, bool rr, DRAWS& draws, TvamInsertWalk& w,
                              float o2[3], float d2[3], float& maxt, float& weight, int* iter = nullptr) {
    const bool brute = MESHES && sc.mesh.n_tris <= TVAM_MESH_BRUTE_MAX;
    while (w.depth < k.max_depth) {
        if (rr) {  // volume.py:181-186
            const float q = fminf(0.99f, w.att);
            const float u_rr = draws.rr(w.depth);
            if (w.depth > k.rr_depth) {
                if (!(u_rr < q)) break;
                w.att = w.att * (1.0f / q);
            }
            if (!(w.att != 0.0f)) break;
        }
        // the container (surfaces and components in scalars: no indexed per-thread array)
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        float t, eta;
        int kind;
        if (k.vial_type == 2 /* TVAM_VIAL_SQUARE */) {
            float ex = 0.0f, ey = 0.0f, ez = 0.0f;
            const float te = tvam_box_hit(w.px, w.py, w.pz, w.vx, w.vy, w.vz, k.vial_r_ext, k.vial_r_ext, k.vial_half_h,
                                          ex, ey, ez);
            const float ti = tvam_box_hit(w.px, w.py, w.pz, w.vx, w.vy, w.vz, k.vial_r, k.vial_r, k.vial_hz_int, nx, ny,
                                          nz);
            const bool inner = ti <= te;
            t = inner ? ti : te;
            if (!inner) nx = ex, ny = ey, nz = ez;
            eta = inner ? k.eta_int : k.eta_ext;
            kind = inner ? TVAM_INS_MEDIUM : TVAM_INS_OUTER;
        } else if (k.vial_type == 1 /* TVAM_VIAL_CYLINDRICAL */) {
            const float te = tvam_tube_hit3(w.px, w.py, w.pz, w.vx, w.vy, w.vz, k.vial_r_ext, k.vial_half_h);
            const float ti = tvam_tube_hit3(w.px, w.py, w.pz, w.vx, w.vy, w.vz, k.vial_r, k.vial_half_h);
            const bool inner = ti <= te;
            t = inner ? ti : te;
            eta = inner ? k.eta_int : k.eta_ext;
            kind = inner ? TVAM_INS_MEDIUM : TVAM_INS_OUTER;
        } else {  // index matched: the null BSDF passes the ray on
            t = tvam_tube_hit3(w.px, w.py, w.pz, w.vx, w.vy, w.vz, k.vial_r, k.vial_half_h);
            eta = 1.0f;
            kind = TVAM_INS_MEDIUM;
        }
        if (k.n_occ) {
            const float tb = tvam_occ_hit(k, w.px, w.py, w.pz, w.vx, w.vy, w.vz);
            if (tb < t) t = tb, kind = TVAM_INS_BLACK;
        }
        int slot = 0;
        if constexpr (MESHES) {
            const float tm = brute ? tvam_mesh_closest_brute(sc.mesh, TVAM_MESH_BOTH, w.px, w.py, w.pz, w.vx, w.vy, w.vz, slot)
                                   : tvam_mesh_closest(sc.mesh, TVAM_MESH_BOTH, w.px, w.py, w.pz, w.vx, w.vy, w.vz, slot);
            if (tm < t) t = tm, kind = TVAM_INS_INSERT;
        }
        if (!(t < TVAM_INF)) break;
        float s1 = 0.0f;
        if constexpr (REFLECT) s1 = draws.s1(w.depth);
        else if (rr) draws.bsdf();
        const bool seg = w.in_medium;
        if (seg) {
            o2[0] = w.px, o2[1] = w.py, o2[2] = w.pz;
            d2[0] = w.vx, d2[1] = w.vy, d2[2] = w.vz;
            maxt = t;
            weight = w.att;
            if (iter) *iter = w.depth;
        }
        if (kind == TVAM_INS_BLACK) {  // a black diffuse BSDF: weight 0
            w.depth = k.max_depth;
            return seg;
        }
        const float hx = fmaf(w.vx, t, w.px), hy = fmaf(w.vy, t, w.py), hz = fmaf(w.vz, t, w.pz);
        if (kind == TVAM_INS_INSERT) {
            tvam_tri_normal(sc.mesh.tris + 9 * slot, nx, ny, nz);
            eta = sc.tri_eta[sc.mesh.ids[slot]];
        } else if (k.vial_type != 2) {
            const float rp = sqrtf(hx * hx + hy * hy);
            nx = hx / rp, ny = hy / rp, nz = 0.0f;
        }
        float wx = w.vx, wy = w.vy, wz = w.vz, tw = 1.0f;
        if (k.vial_type != 0 || kind == TVAM_INS_INSERT) {
            if (REFLECT && w.depth > 0) tw = tvam_dielectric_sample(nx, ny, nz, w.vx, w.vy, w.vz, eta, s1, wx, wy, wz);
            else tw = tvam_transmit_world(nx, ny, nz, w.vx, w.vy, w.vz, eta, wx, wy, wz);
        }
        if (!(tw > 0.0f)) {
            w.depth = k.max_depth;
            return seg;
        }
        w.att = w.att * tw;
        if (seg) w.att = w.att * expf(-k.sig_t * t);
        const float m = fmaxf(fmaxf(fabsf(hx), fabsf(hy)), fabsf(hz));
        float mag = (1.0f + m) * TVAM_RAY_EPS;
        const float nwo = nx * wx + ny * wy + nz * wz;
        if (__builtin_signbit(nwo)) mag = -mag;
        w.px = fmaf(mag, nx, hx);
        w.py = fmaf(mag, ny, hy);
        w.pz = fmaf(mag, nz, hz);
        w.vx = wx;
        w.vy = wy;
        w.vz = wz;
        w.in_medium = (kind == TVAM_INS_MEDIUM && nwo < 0.0f) || (kind == TVAM_INS_INSERT && nwo > 0.0f);
        ++w.depth;
        if (seg) return true;
    }
    w.depth = k.max_depth;
    return false;
}

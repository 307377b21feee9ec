// tvam_firsthit.h -- the first surface a projector ray meets, and the 'filter_corner' decision
// (integrators/filter_corner.py:60-66, optimize.py:166-185): scene.ray_intersect of a world ray
// with a fully 3-D direction against the container's outer surface and the occluder triangles,
// then norm(abs(si.p.xy) - dist) < radius.  Host and device (fp32, the divisions and square roots
// of tvam_quadratic / tvam_box_hit / tvam_tri_hit, which this header calls and does not restate).
//
//   vial            outer surface
//   index_matched   open tube of radius vial_r, |z| <= vial_half_h
//   cylindrical     open tube of radius vial_r_ext, |z| <= vial_half_h
//   square          closed cuboid vial_r_ext x vial_r_ext x vial_half_h (all six faces)
//   custom          the outer mesh, from either side (tvam_mesh.h)
//
// A tube is hit from either side (si.is_valid() does not look at the orientation): a ray that
// came in through an open end and meets the inside wall has a valid hit.  The reference's scene
// also holds the target mesh during this pass; it lies inside the container and never comes first,
// so it is left out here (the one deviation).
#pragma once
#include "tvam_common.h"
#include "tvam_mesh.h"

struct TvamFirstHit {
    float t;            // distance along the ray, -1: no surface
    float px, py, pz;   // the hit point o + t d (0 on a miss)
};

// Nearest hit t >= 0 of the open tube (radius r, |z| <= half) for a 3-D ray (Mitsuba cylinder
// restated; tvam_seg3d.h's sc_tube_hit, here for the host too).
TVAM_HD float tvam_tube_hit3(float ox, float oy, float oz, float dx, float dy, float dz, float r, float half) {
    float t0, t1;
    if (!tvam_cyl_roots(ox, oy, dx, dy, r, t0, t1)) return TVAM_INF;
    if (!(t1 >= 0.0f)) return TVAM_INF;
    const float zn = fmaf(dz, t0, oz), zf = fmaf(dz, t1, oz);
    if (t0 >= 0.0f && zn >= -half && zn <= half) return t0;
    if (zf >= -half && zf <= half) return t1;
    return TVAM_INF;
}

// The container's outer surface alone.
TVAM_HD float tvam_outer_hit(const TvamConsts& k, float ox, float oy, float oz, float dx, float dy, float dz) {
    if (k.vial_type == 3 /* TVAM_VIAL_CUSTOM */) {
        int slot;
        return tvam_mesh_closest(tvam_mesh_view(k.mesh), TVAM_MESH_OUTER, ox, oy, oz, dx, dy, dz, slot);
    }
    if (k.vial_type == 2 /* TVAM_VIAL_SQUARE */) {
        float nx, ny, nz;
        return tvam_box_hit(ox, oy, oz, dx, dy, dz, k.vial_r_ext, k.vial_r_ext, k.vial_half_h, nx, ny, nz);
    }
    const float r = k.vial_type == 1 /* TVAM_VIAL_CYLINDRICAL */ ? k.vial_r_ext : k.vial_r;
    return tvam_tube_hit3(ox, oy, oz, dx, dy, dz, r, k.vial_half_h);
}

// scene.ray_intersect: the nearer of the outer surface and the occluders.
TVAM_HD TvamFirstHit tvam_first_hit(const TvamConsts& k, float ox, float oy, float oz, float dx, float dy, float dz) {
    float t = tvam_outer_hit(k, ox, oy, oz, dx, dy, dz);
    if (k.n_occ) t = fminf(t, tvam_occ_hit(k, ox, oy, oz, dx, dy, dz));
    TvamFirstHit h;
    if (!(t < TVAM_INF)) {
        h.t = -1.0f;
        h.px = h.py = h.pz = 0.0f;
        return h;
    }
    h.t = t;
    h.px = fmaf(dx, t, ox);
    h.py = fmaf(dy, t, oy);
    h.pz = fmaf(dz, t, oz);
    return h;
}

// filter_corner.py:63: the hit lies within `radius` of a vertical edge at (+-dist, +-dist).
TVAM_HD bool tvam_hits_corner(float px, float py, float dist, float radius) {
    const float ax = fabsf(px) - dist, ay = fabsf(py) - dist;
    return sqrtf(ax * ax + ay * ay) < radius;
}

// The pixel stays active: its ray meets the scene and not near a corner.
TVAM_HD bool tvam_corner_keep(const TvamFirstHit& h, float dist, float radius) {
    return h.t >= 0.0f && !tvam_hits_corner(h.px, h.py, dist, radius);
}

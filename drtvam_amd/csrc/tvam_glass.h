// tvam_glass.h -- the medium segment of a 3-D ray behind a 'cylindrical' or 'square' glass vial
// (geometry.py:142-219), host and device, fp32: the tracer of the plans of tvam_plan_create_traced.
//
// Two analytic dielectric surfaces, the outer one (air | glass) and the inner one (glass | medium):
//   cylindrical   open tubes of radius vial_r_ext and vial_r, |z| <= vial_half_h, no end caps
//                 (geometry.py:153), outward normal (hx, hy, 0) / sqrt(hx^2 + hy^2)
//   square        closed cuboids (vial_r_ext, vial_r_ext, vial_half_h) and (vial_r, vial_r,
//                 vial_hz_int), all six faces, tvam_box_hit's normals
// The path loop is volume.py:179-272 in transmission-only mode with a non-scattering medium, in the
// statement order of tvam_segment_square / tvam_segment_mesh with all three components: per surface
// the nearest hit t >= 0 of the two (a tie goes to the inner one; none: the ray deposits nothing,
// which also ends a ray that leaves the medium through a tube's open end, cn_segment's rule), the
// medium segment (p, v, [0, t]) of weight att once the ray is in the medium, else the dielectric
// transmission (tvam_transmit_world; weight 0 = total internal reflection ends the ray), the
// spawn_ray offset (1 + max|h|) RayEpsilon along the normal on the side of wo, and the medium flag.
// A ray may come in through a tube's open end and meet a wall from inside.
//
// A planar ray (d.z = 0) gives tvam_segment_square's bits; behind the tubes it agrees with
// tvam_segment_cyl to rounding (that one refracts in the tube's shading frame, tvam_transmit).
// No per-thread array is indexed dynamically here: surfaces and components are scalars.
#pragma once
#include "../../include/tvam.h"
#include "tvam_firsthit.h"

// `square`: the cuboids, else the tubes.  Returns whether the ray deposits.
TVAM_HD bool tvam_segment_glass(bool square, float r_ext, float r_int, float half, float hz_int, float eta_ext,
                                float eta_int, int max_depth, const float o[3], const float d[3], float o2[3],
                                float d2[3], float& maxt, float& weight) {
    float px = o[0], py = o[1], pz = o[2], vx = d[0], vy = d[1], vz = d[2], att = 1.0f;
    bool in_medium = false;
    for (int depth = 0; depth < max_depth; ++depth) {
        float nex = 0.0f, ney = 0.0f, nez = 0.0f, nix = 0.0f, niy = 0.0f, niz = 0.0f;
        float te, ti;
        if (square) {
            te = tvam_box_hit(px, py, pz, vx, vy, vz, r_ext, r_ext, half, nex, ney, nez);
            ti = tvam_box_hit(px, py, pz, vx, vy, vz, r_int, r_int, hz_int, nix, niy, niz);
        } else {
            te = tvam_tube_hit3(px, py, pz, vx, vy, vz, r_ext, half);
            ti = tvam_tube_hit3(px, py, pz, vx, vy, vz, r_int, half);
        }
        const bool inner = ti <= te;
        const float t = inner ? ti : te;
        if (!(t < TVAM_INF)) return false;
        if (in_medium) {
            o2[0] = px, o2[1] = py, o2[2] = pz;
            d2[0] = vx, d2[1] = vy, d2[2] = vz;
            maxt = t;
            weight = att;
            return true;
        }
        const float hx = fmaf(vx, t, px), hy = fmaf(vy, t, py), hz = fmaf(vz, t, pz);
        float nx, ny, nz;
        if (square) {
            nx = inner ? nix : nex, ny = inner ? niy : ney, nz = inner ? niz : nez;
        } else {
            const float rp = sqrtf(hx * hx + hy * hy);
            nx = hx / rp, ny = hy / rp, nz = 0.0f;
        }
        float wx, wy, wz;
        const float w = tvam_transmit_world(nx, ny, nz, vx, vy, vz, inner ? eta_int : eta_ext, wx, wy, wz);
        if (!(w > 0.0f)) return false;
        att = att * w;
        const float m = fmaxf(fmaxf(fabsf(hx), fabsf(hy)), fabsf(hz));
        float mag = (1.0f + m) * TVAM_RAY_EPS;
        const float nwo = nx * wx + ny * wy + nz * wz;
        if (__builtin_signbit(nwo)) mag = -mag;
        px = fmaf(mag, nx, hx);
        py = fmaf(mag, ny, hy);
        pz = fmaf(mag, nz, hz);
        vx = wx;
        vy = wy;
        vz = wz;
        in_medium = inner && nwo < 0.0f;
    }
    return false;
}

// ... of a plan's constants (vial_type TVAM_VIAL_CYLINDRICAL or TVAM_VIAL_SQUARE).
TVAM_HD bool tvam_segment_traced(const TvamConsts& k, const float o[3], const float d[3], float o2[3], float d2[3],
                                 float& maxt, float& weight) {
    return tvam_segment_glass(k.vial_type == TVAM_VIAL_SQUARE, k.vial_r_ext, k.vial_r, k.vial_half_h,
                              k.vial_hz_int, k.eta_ext, k.eta_int, k.max_depth, o, d, o2, d2, maxt, weight);
}

// tvam_double.h -- the medium segments of a ray behind a 'double_cylindrical' vial
// (geometry.py:222-308), host and device.
//
// Four concentric open tubes around z (|z| <= half, outward normals), outermost first:
//   S0  r0  air          | outer glass
//   S1  r1  outer glass  | medium        crossed inwards: in the medium
//   S2  r2  medium       | inner glass   crossed outwards: in the medium
//   S3  r3  inner glass  | core          (the core holds no resin)
// The path loop is volume.py:179-272 in transmission-only mode with a non-scattering medium, in the
// statement order of tvam_segment_mesh: per surface the nearest hit t >= 0 over the four tubes
// (tvam_tube_hit3's rule; none: the ray left through an open end, nothing more is deposited), a
// medium segment (p, v, [0, t]) with the current attenuation when the ray is in the medium, the
// dielectric transmission (tvam_transmit_world with the tube's eta; weight 0 = total internal
// reflection ends the path), e^{-sigma_t t} after a medium segment (volume.py:263), the spawn_ray
// offset (1 + max|h|) RayEpsilon along the normal on the side of wo, the medium flag.  At most
// max_depth surfaces, so a ray deposits along 0, 1 or 2 segments: in front of the inner vial and
// behind it.
//
// The walk is resumable: its state is the point, the direction, the attenuation, the depth and the
// flag, and tvam_double_next advances it to the next medium segment.  A kernel marches one segment
// at a time with one copy of its DDA and never holds both.
#pragma once
#include "tvam_firsthit.h"

struct TvamDoubleWalk {
    float px, py, pz, vx, vy, vz;
    float att;
    int depth;
    bool in_medium;
};

TVAM_HD void tvam_double_start(TvamDoubleWalk& w, const float o[3], const float d[3]) {
    w.px = o[0], w.py = o[1], w.pz = o[2];
    w.vx = d[0], w.vy = d[1], w.vz = d[2];
    w.att = 1.0f;
    w.depth = 0;
    w.in_medium = false;
}

// The walk to its next medium segment (o2, d2, [0, maxt]) of weight `weight` (the attenuation the
// segment starts with); false: the path has ended.  `iter` (host checks): the loop iteration of
// the deposit.
TVAM_HD bool tvam_double_next(const TvamDouble& v, float half, float sig_t, int max_depth, TvamDoubleWalk& w,
                              float o2[3], float d2[3], float& maxt, float& weight, int* iter = nullptr) {
    while (w.depth < max_depth) {
        // nearest of the four tubes (axes and surfaces in scalars: no indexed per-thread array)
        float t = tvam_tube_hit3(w.px, w.py, w.pz, w.vx, w.vy, w.vz, v.r0, half);
        float eta = v.eta0;
        int s = 0;
        const float t1 = tvam_tube_hit3(w.px, w.py, w.pz, w.vx, w.vy, w.vz, v.r1, half);
        if (t1 < t) t = t1, eta = v.eta1, s = 1;
        const float t2 = tvam_tube_hit3(w.px, w.py, w.pz, w.vx, w.vy, w.vz, v.r2, half);
        if (t2 < t) t = t2, eta = v.eta2, s = 2;
        const float t3 = tvam_tube_hit3(w.px, w.py, w.pz, w.vx, w.vy, w.vz, v.r3, half);
        if (t3 < t) t = t3, eta = v.eta3, s = 3;
        if (!(t < TVAM_INF)) break;
        const bool seg = w.in_medium;
        if (seg) {
            o2[0] = w.px, o2[1] = w.py, o2[2] = w.pz;
            d2[0] = w.vx, d2[1] = w.vy, d2[2] = w.vz;
            maxt = t;
            weight = w.att;
            if (iter) *iter = w.depth;
        }
        const float hx = fmaf(w.vx, t, w.px), hy = fmaf(w.vy, t, w.py), hz = fmaf(w.vz, t, w.pz);
        const float rp = sqrtf(hx * hx + hy * hy);
        const float nx = hx / rp, ny = hy / rp;
        float wx, wy, wz;
        const float tw = tvam_transmit_world(nx, ny, 0.0f, w.vx, w.vy, w.vz, eta, wx, wy, wz);
        if (!(tw > 0.0f)) {
            w.depth = max_depth;
            return seg;
        }
        w.att = w.att * tw;
        if (seg) w.att = w.att * expf(-sig_t * t);
        const float m = fmaxf(fmaxf(fabsf(hx), fabsf(hy)), fabsf(hz));
        float mag = (1.0f + m) * TVAM_RAY_EPS;
        const float nwo = nx * wx + ny * wy + 0.0f * wz;
        if (__builtin_signbit(nwo)) mag = -mag;
        w.px = fmaf(mag, nx, hx);
        w.py = fmaf(mag, ny, hy);
        w.pz = hz;
        w.vx = wx;
        w.vy = wy;
        w.vz = wz;
        w.in_medium = (s == 1 && nwo < 0.0f) || (s == 2 && nwo > 0.0f);
        ++w.depth;
        if (seg) return true;
    }
    w.depth = max_depth;
    return false;
}

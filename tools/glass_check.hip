// Stand-alone host run of the traced glass vials' tracer (drtvam_amd/csrc/tvam_glass.h: the code the
// CN_GLASS kernels of tvam_ray3d.hip run), for a sanitizer build without a GPU or an interpreter:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude tools/glass_check.hip -o glass_check && ./glass_check
// Vials: the tests' tube (r_ext 6.5 / r_int 6.0) and cuvette (w_ext 13 / w_int 12), height 4, glass
// 1.54 around a resin of 1.347.  Rays: through the axis (the chord is the inner diameter less two
// spawn offsets), then random rays from outside and from inside the glass and the medium,
// axis-parallel rays (a zero component: tvam_box_hit's slab test), rays along z (through a tube's
// open ends, through the cuvette's four horizontal faces), grazing rays (tangent to a tube, within a
// few ulp of a cuboid's face plane and of its edges), at every max_depth from 0 to 8.  Checks: finite
// values, a unit direction, a weight in (0, 1.4] (a ray that starts in the glass gains up to
// (1.54 / 1.347)^2), a segment no longer than the inner surface's diagonal, nothing deposited at
// max_depth < 1.  Prints one line per part; exit status 1 on a failure.
#include <cmath>
#include <cstdio>

#include "../drtvam_amd/csrc/tvam_glass.h"

static uint32_t g_state = 2463534242u;
static float uni() {  // xorshift32 in [0, 1)
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

static const float R_EXT = 6.5f, R_INT = 6.0f, HALF = 2.0f, HZ_INT = 1.8f;
static const float ETA_EXT = 1.54f / TVAM_IOR_AIR, ETA_INT = 1.347f / 1.54f;

// One ray; returns whether it deposits, `bad` set on a broken invariant.
static bool run(bool square, int max_depth, const float o[3], const float d[3], float& maxt, int& bad) {
    float o2[3] = {NAN, NAN, NAN}, d2[3] = {NAN, NAN, NAN}, w = NAN;
    maxt = NAN;
    if (!tvam_segment_glass(square, R_EXT, R_INT, HALF, HZ_INT, ETA_EXT, ETA_INT, max_depth, o, d, o2, d2, maxt, w))
        return false;
    const float len = sqrtf(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
    const float diag = 2.0f * sqrtf(2.0f * R_INT * R_INT + HALF * HALF) + 1.0f;
    if (!(std::isfinite(maxt) && maxt >= 0.0f && maxt <= diag && w > 0.0f && w <= 1.4f && fabsf(len - 1.0f) < 1e-4f &&
          std::isfinite(o2[0]) && std::isfinite(o2[1]) && std::isfinite(o2[2]) && max_depth >= 1))
        bad = 1;
    return true;
}

int main() {
    int bad = 0;
    // 1. through the axis
    for (int sq = 0; sq < 2; ++sq) {
        const float o[3] = {20.0f, 0.0f, 0.5f}, d[3] = {-1.0f, 0.0f, 0.0f};
        float maxt;
        const bool hit = run(sq != 0, 6, o, d, maxt, bad);
        printf("%s, through the axis: chord %.6f (inner width %.1f)\n", sq ? "cuvette" : "tube", hit ? maxt : -1.0f,
               2.0f * R_INT);
        bad |= !hit || !(fabsf(maxt - 2.0f * R_INT) < 4.0f * (1.0f + R_EXT) * TVAM_RAY_EPS);
        float m2;
        bad |= run(sq != 0, 2, o, d, m2, bad);  // two surfaces before the segment: max_depth 3 at least
    }
    // 2. random, axis-parallel, along z and grazing rays at every max_depth
    for (int sq = 0; sq < 2; ++sq) {
        long long segs = 0, rays = 0, zsegs = 0;
        for (int max_depth = 0; max_depth <= 8; ++max_depth)
            for (int r = 0; r < 40000; ++r) {
                const float R = (r % 4 == 0) ? 7.0f * uni() : 25.0f;  // from inside a shell, or from outside
                const float phi = 6.2831853f * uni();
                float o[3] = {R * cosf(phi), R * sinf(phi), (r % 3 == 0 ? 6.0f : 50.0f) * (uni() - 0.5f)};
                float d[3];
                for (int a = 0; a < 3; ++a) d[a] = 14.0f * uni() - 7.0f - o[a];
                const int kind = r % 11;
                if (kind == 1) {  // along z, from above or below: open ends / horizontal faces
                    o[0] = 13.0f * uni() - 6.5f, o[1] = 13.0f * uni() - 6.5f, o[2] = r % 2 ? 10.0f : -10.0f;
                    d[0] = 0.0f, d[1] = 0.0f, d[2] = -o[2];
                } else if (kind == 2) {  // axis-parallel in the plane
                    d[(r / 11) % 2] = 0.0f, d[2] = 0.0f;
                } else if (kind == 3) {  // grazing: tangent to a tube / in a face plane, to a few ulp
                    const float rr = (r / 11) % 2 ? R_EXT : R_INT;
                    const float off = rr * (1.0f + ((float)(r % 5) - 2.0f) * 1.1920929e-7f);
                    o[0] = 20.0f, o[1] = off, o[2] = 4.0f * uni() - 2.0f;
                    d[0] = -1.0f, d[1] = 0.0f, d[2] = 0.0f;
                } else if (kind == 4) {  // grazing a horizontal face / an open end's rim
                    const float hz = (r / 11) % 2 ? HALF : HZ_INT;
                    o[0] = 20.0f, o[1] = 13.0f * uni() - 6.5f, o[2] = hz * (1.0f + ((float)(r % 5) - 2.0f) * 1.1920929e-7f);
                    d[0] = -1.0f, d[1] = 0.0f, d[2] = 0.0f;
                } else if (kind == 5) {  // at a vertical edge of the cuboids / the same line on the tubes
                    const float rr = (r / 11) % 2 ? R_EXT : R_INT;
                    o[0] = 20.0f, o[1] = 20.0f - rr + rr, o[2] = 4.0f * uni() - 2.0f;
                    d[0] = rr - 20.0f, d[1] = rr - o[1], d[2] = 0.0f;
                } else if (kind == 6) {  // in through an open end / the top face at a slope
                    o[0] = 12.0f * uni() - 6.0f, o[1] = 0.0f, o[2] = 4.0f;
                    d[0] = 4.0f * uni() - 2.0f, d[1] = 4.0f * uni() - 2.0f, d[2] = -1.0f;
                }
                float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                if (!(len > 0.0f)) d[0] = 1.0f, d[1] = 0.0f, d[2] = 0.0f, len = 1.0f;
                for (int a = 0; a < 3; ++a) d[a] /= len;
                float maxt;
                const bool hit = run(sq != 0, max_depth, o, d, maxt, bad);
                if (hit && kind == 1) {
                    ++zsegs;
                    if (!sq) bad = 1;  // along z no tube is ever met
                }
                segs += hit;
                ++rays;
            }
        printf("%s: %lld segments of %lld rays, %lld of them along z\n", sq ? "cuvette" : "tube", segs, rays, zsegs);
        bad |= segs == 0 || (sq && zsegs == 0);
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad;
}

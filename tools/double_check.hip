// Stand-alone host run of the double vial's tracer (drtvam_amd/csrc/tvam_double.h: the resumable
// walk the kernels run), for a sanitizer build without a GPU or an interpreter:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude tools/double_check.hip -o double_check && ./double_check
// Rays: the reference config's tubes (7 / 6 / 3 / 2; 1.53, 1.48, 1.553, 1.33) under collimated rays
// at its 24 impact parameters, whose medium chords Bouguer's invariant gives in closed form, then
// random 3-D rays from outside, from inside every shell, axis-parallel and along z, at every
// max_depth from 0 to 12.  Checks: at most two segments, finite values, unit directions, weights in
// (0, 1.25] (a ray that starts inside the inner glass gains (1.553 / 1.48)^2), a walk that has
// ended stays ended.  Prints one line per part; exit status 1 on a failure.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../drtvam_amd/csrc/tvam_double.h"

static uint32_t g_state = 2463534242u;
static float uni() {  // xorshift32 in [0, 1)
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

static TvamDouble reference_vial() {
    TvamDouble v;
    v.r0 = 7.0f, v.r1 = 6.0f, v.r2 = 3.0f, v.r3 = 2.0f;
    v.eta0 = 1.53f / TVAM_IOR_AIR, v.eta1 = 1.48f / 1.53f, v.eta2 = 1.553f / 1.48f, v.eta3 = 1.33f / 1.553f;
    return v;
}

struct Seg {
    float o2[3], d2[3], maxt, w;
    int iter;
};

static int walk(const TvamDouble& v, int max_depth, const float o[3], const float d[3], Seg out[2], int& bad) {
    TvamDoubleWalk w;
    tvam_double_start(w, o, d);
    int n = 0;
    for (int s = 0; s < 3; ++s) {  // a third call must find nothing
        Seg g;
        if (!tvam_double_next(v, 20.0f, 0.05f, max_depth, w, g.o2, g.d2, g.maxt, g.w, &g.iter)) break;
        if (n == 2) {
            bad = 1;
            break;
        }
        const float len = sqrtf(g.d2[0] * g.d2[0] + g.d2[1] * g.d2[1] + g.d2[2] * g.d2[2]);
        if (!(std::isfinite(g.maxt) && g.maxt >= 0.0f && g.w > 0.0f && g.w <= 1.25f && fabsf(len - 1.0f) < 1e-4f &&
              std::isfinite(g.o2[0]) && std::isfinite(g.o2[1]) && std::isfinite(g.o2[2]) && g.iter < max_depth))
            bad = 1;
        out[n++] = g;
    }
    float o2[3], d2[3], maxt, wt;
    if (tvam_double_next(v, 20.0f, 0.05f, max_depth, w, o2, d2, maxt, wt)) bad = 1;  // ended stays ended
    return n;
}

int main() {
    int bad = 0;
    const TvamDouble v = reference_vial();
    // 1. collimated rays against the closed form
    double worst = 0.0;
    int counts[3] = {0, 0, 0};
    for (int i = 0; i < 24; ++i) {
        const float b = 0.15f + 0.3f * (float)i;
        const float o[3] = {-20.0f, b, 0.0f}, d[3] = {1.0f, 0.0f, 0.0f};
        Seg s[2];
        const int n = walk(v, 10, o, d, s, bad);
        ++counts[n];
        const double bm = (double)b * (double)TVAM_IOR_AIR / 1.48;
        const bool two = bm < 3.0;
        const double chord = two ? std::sqrt(36.0 - bm * bm) - std::sqrt(9.0 - bm * bm) : 2.0 * std::sqrt(36.0 - bm * bm);
        const int expect = b > 7.0f ? 0 : (i == 9 ? 1 : (two ? 2 : 1));  // i == 9 (b = 2.85): totally reflected at S3
        if (n != expect) bad = 1;
        for (int k = 0; k < n; ++k) {
            worst = std::fmax(worst, std::fabs((double)s[k].maxt - chord));
            if (s[k].iter != (k == 0 ? 2 : (b > 3.0f ? 4 : 6))) bad = 1;
        }
    }
    // (the spawn offsets keep the walk within a few 1e-3 of the closed form, tests/test_double_vial.py)
    printf("closed form: %d / %d / %d rays with 0 / 1 / 2 segments, largest |maxt - chord| %.3e\n", counts[0], counts[1],
           counts[2], worst);
    bad |= !(worst < 5e-3) || counts[0] != 1 || counts[1] != 9 || counts[2] != 14;
    // 2. random rays at every max_depth
    long long segs = 0, rays = 0;
    for (int max_depth = 0; max_depth <= 12; ++max_depth)
        for (int r = 0; r < 20000; ++r) {
            const float R = (r % 4 == 0) ? 6.5f * uni() : 25.0f;  // from inside a shell, or from outside
            const float phi = 6.2831853f * uni();
            float o[3] = {R * cosf(phi), R * sinf(phi), 50.0f * uni() - 25.0f};
            float d[3];
            for (int a = 0; a < 3; ++a) d[a] = 16.0f * uni() - 8.0f - o[a];
            if (r % 7 == 0) d[0] = 0.0f, d[1] = 0.0f, d[2] = 1.0f;               // along the axis: no tube is met
            else if (r % 5 == 0) d[(r / 5) % 2] = 0.0f, d[2] = 0.0f;             // axis-parallel in the plane
            float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (!(len > 0.0f)) d[0] = 1.0f, len = 1.0f;
            for (int a = 0; a < 3; ++a) d[a] /= len;
            Seg s[2];
            const int n = walk(v, max_depth, o, d, s, bad);
            if (max_depth < 2 && n != 0 && R > 7.0f) bad = 1;
            segs += n;
            ++rays;
        }
    printf("random rays: %lld segments of %lld rays\n", segs, rays);
    bad |= segs == 0;
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad;
}

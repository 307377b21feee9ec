// CPU run of the 'filter_corner' geometry (drtvam_amd/csrc/tvam_firsthit.h: first hit of a 3-D ray
// against the container's outer surface and the occluders, and the corner predicate), so that
// tests/test_corner_model.py can compare it with the float64 model without a GPU.  Host code only.
// Build and run: tools/corner_check.sh INPUT [INPUT ...]
//
// INPUT (text): vial_type vial_r vial_r_ext half_height dist radius n_occ n_rays
//               n_occ x 9 floats (triangles [3 vertices][x, y, z])
//               n_rays x 6 floats (o.x o.y o.z d.x d.y d.z; fp32 values)
// Output per INPUT: a line "case <index> <n_rays>", then one line per ray: keep t p.x p.y p.z
// (t = -1 on a miss)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../drtvam_amd/csrc/tvam_firsthit.h"

static int run_case(int index, const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "corner_check: cannot open %s\n", path);
        return 2;
    }
    TvamConsts k{};
    float dist, radius;
    int n_occ;
    long n_rays;
    if (fscanf(f, "%d %f %f %f %f %f %d %ld", &k.vial_type, &k.vial_r, &k.vial_r_ext, &k.vial_half_h, &dist, &radius,
               &n_occ, &n_rays) != 8 || n_occ < 0 || n_rays < 0) {
        fprintf(stderr, "corner_check: bad header in %s\n", path);
        fclose(f);
        return 2;
    }
    std::vector<float> occ((size_t)n_occ * 9);
    for (float& v : occ)
        if (fscanf(f, "%f", &v) != 1) {
            fprintf(stderr, "corner_check: bad triangle list in %s\n", path);
            fclose(f);
            return 2;
        }
    k.occ = occ.data();
    k.n_occ = n_occ;
    for (int a = 0; a < 3; ++a) {  // the occluders' bounding box, as tvam_plan_create forms it
        k.occ_lo[a] = TVAM_INF;
        k.occ_hi[a] = -TVAM_INF;
    }
    for (size_t i = 0; i < occ.size(); ++i) {
        k.occ_lo[i % 3] = std::min(k.occ_lo[i % 3], occ[i]);
        k.occ_hi[i % 3] = std::max(k.occ_hi[i % 3], occ[i]);
    }
    printf("case %d %ld\n", index, n_rays);
    for (long i = 0; i < n_rays; ++i) {
        float r[6];
        for (float& v : r)
            if (fscanf(f, "%f", &v) != 1) {
                fprintf(stderr, "corner_check: bad ray %ld in %s\n", i, path);
                fclose(f);
                return 2;
            }
        const TvamFirstHit h = tvam_first_hit(k, r[0], r[1], r[2], r[3], r[4], r[5]);
        printf("%d %.9g %.9g %.9g %.9g\n", tvam_corner_keep(h, dist, radius) ? 1 : 0, h.t, h.px, h.py, h.pz);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: corner_check INPUT [INPUT ...]\n");
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        const int rc = run_case(i - 1, argv[i]);
        if (rc) return rc;
    }
    return 0;
}

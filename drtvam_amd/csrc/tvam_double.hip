// 'double_cylindrical' vial (geometry.py:222-308; tvam_double.h): two nested glass tubes with the
// printing medium between them.  Every ray is traced in 3-D through the four dielectric tubes and
// deposits along at most two medium segments, in front of the inner vial and behind it, for all
// three projectors.  The kernels are tvam_ray3d.hip's over WalkDouble (tvam_ray3d.h); here, on the
// host, the validation of the vial, its constants and tvam_double_segments.
#include "tvam_plan.h"

#include <algorithm>
#include <cmath>

#include "tvam_double.h"

int tvam_double_validate(const tvam_double_vial* v, float medium_ior) {
    if (!v) return tvam_fail(TVAM_ERR_INVALID, "a 'double_cylindrical' vial needs its tvam_double_vial");
    if (!(v->r_ext_outer > v->r_int_outer && v->r_int_outer > v->r_ext_inner && v->r_ext_inner > v->r_int_inner &&
          v->r_int_inner > 0.0f) ||
        !std::isfinite(v->r_ext_outer))
        return tvam_fail(TVAM_ERR_INVALID,
                         "a 'double_cylindrical' vial needs r_ext_outer > r_int_outer > r_ext_inner > r_int_inner > 0");
    if (!(v->ior_outer > 0.0f && v->ior_inner > 0.0f && v->ior_inside_inner > 0.0f && medium_ior > 0.0f))
        return tvam_fail(TVAM_ERR_INVALID, "a 'double_cylindrical' vial needs positive IORs");
    return 0;
}

// eta = int_ior / ext_ior of each tube's dielectric (geometry.py:259-305; 'outer_vial' has Mitsuba's
// default ext_ior, air)
TvamDouble tvam_double_consts(const tvam_double_vial& v, float medium_ior) {
    TvamDouble c;
    c.r0 = v.r_ext_outer, c.r1 = v.r_int_outer, c.r2 = v.r_ext_inner, c.r3 = v.r_int_inner;
    c.eta0 = v.ior_outer / TVAM_IOR_AIR;
    c.eta1 = medium_ior / v.ior_outer;
    c.eta2 = v.ior_inner / medium_ior;
    c.eta3 = v.ior_inside_inner / v.ior_inner;
    return c;
}

extern "C" int tvam_double_segments(const tvam_double_vial* vial, float medium_ior, float sigma_t, float height,
                                    int32_t max_depth, const float* o, const float* d, int64_t n_rays, float* segs) {
    if (n_rays < 0 || (n_rays > 0 && (!o || !d || !segs))) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    const int rc = tvam_double_validate(vial, medium_ior);
    if (rc) return rc;
    if (!(height > 0.0f)) return tvam_fail(TVAM_ERR_INVALID, "a 'double_cylindrical' vial needs a positive height");
    const TvamDouble c = tvam_double_consts(*vial, medium_ior);
    const float half = 0.5f * height;
    for (int64_t i = 0; i < n_rays; ++i) {
        TvamDoubleWalk w;
        tvam_double_start(w, o + 3 * i, d + 3 * i);
        float* row = segs + 16 * i;
        std::fill(row, row + 16, 0.0f);
        for (int s = 0; s < 2; ++s) {
            float o2[3], d2[3], maxt, att;
            if (!tvam_double_next(c, half, sigma_t, max_depth, w, o2, d2, maxt, att)) break;
            seg_row(row + 8 * s, o2, d2, maxt, att);
        }
    }
    return 0;
}

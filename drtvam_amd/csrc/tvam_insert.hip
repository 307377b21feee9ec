// Dielectric occluders (geometry.py:55-72 with a 'bsdf' entry; tvam_insert.h): transparent inserts
// inside the resin.  Every ray is traced in 3-D through the container, the black occluders and the
// inserts' triangles and deposits along every stretch it runs in the resin, for all three projectors
// and the 'index_matched', 'cylindrical' and 'square' vials.  The kernels are tvam_ray3d.hip's over
// WalkInsert (tvam_ray3d.h); here, on the host, the validation of the inserts and their flat tables.
#include "tvam_plan.h"

#include <cmath>

#include "tvam_insert.h"

// The inserts of tvam_plan_create_inserts / tvam_insert_segments against the container of k:
// TVAM_ERR_INVALID naming the insert and the triangle or vertex, 0 if sound.  No device call.
int tvam_inserts_validate(const TvamConsts& k, const tvam_insert* ins, int32_t n) {
    if (!ins || n <= 0) return tvam_fail(TVAM_ERR_INVALID, "dielectric occluders: no insert given");
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) {
        const std::string who = "insert " + std::to_string(i);
        const tvam_insert& s = ins[i];
        if (!s.tris || s.n_tris <= 0) return tvam_fail(TVAM_ERR_INVALID, who + ": the mesh is null or empty");
        if (!(s.int_ior > 0.0f && s.ext_ior > 0.0f) || !std::isfinite(s.int_ior) || !std::isfinite(s.ext_ior))
            return tvam_fail(TVAM_ERR_INVALID, who + ": int_ior and ext_ior must be positive");
        total += s.n_tris;
        if (total >= (1 << 27)) return tvam_fail(TVAM_ERR_TOO_LARGE, "the inserts have too many triangles");
        for (int32_t j = 0; j < s.n_tris; ++j) {
            const float* v = s.tris + 9 * (size_t)j;
            for (int q = 0; q < 9; ++q)
                if (!std::isfinite(v[q]))
                    return tvam_fail(TVAM_ERR_INVALID, who + ": triangle " + std::to_string(j) + " vertex " +
                                                           std::to_string(q / 3) + " is not finite");
            float nx, ny, nz;
            tvam_tri_normal(v, nx, ny, nz);  // the kernels' own normal: it must exist
            if (!(std::isfinite(nx) && std::isfinite(ny) && std::isfinite(nz)))
                return tvam_fail(TVAM_ERR_INVALID, who + ": triangle " + std::to_string(j) + " has zero area");
            for (int c = 0; c < 3; ++c) {
                const float x = v[3 * c], y = v[3 * c + 1], z = v[3 * c + 2];
                const bool out = k.vial_type == TVAM_VIAL_SQUARE
                                     ? (std::fabs(x) > k.vial_r || std::fabs(y) > k.vial_r || std::fabs(z) > k.vial_hz_int)
                                     : (std::sqrt(x * x + y * y) >= k.vial_r || std::fabs(z) > k.vial_half_h);
                if (out)
                    return tvam_fail(TVAM_ERR_INVALID, who + ": triangle " + std::to_string(j) + " vertex " +
                                                           std::to_string(c) + " lies outside the resin");
            }
        }
    }
    return 0;
}

// All inserts' triangles in the caller's order, and each triangle's eta = int_ior / ext_ior.
void tvam_inserts_flatten(const tvam_insert* ins, int32_t n, std::vector<float>& tris, std::vector<float>& tri_eta) {
    tris.clear(), tri_eta.clear();
    for (int32_t i = 0; i < n; ++i) {
        tris.insert(tris.end(), ins[i].tris, ins[i].tris + 9 * (size_t)ins[i].n_tris);
        tri_eta.insert(tri_eta.end(), (size_t)ins[i].n_tris, ins[i].int_ior / ins[i].ext_ior);
    }
}

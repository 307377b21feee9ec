// tvam_mesh.hip -- host side of the 'custom' vial's meshes: validation, the bounding volume
// hierarchy of tvam_mesh.h (built once per plan, on the host) and tvam_mesh_hit, the host-only
// closest-hit entry that runs the kernels' own traversal (tvam_mesh.h is host and device).
#include "tvam_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "tvam_mesh.h"

namespace {

struct Builder {
    const float* tris;
    std::vector<float> cen;      // [n][3] centroids
    std::vector<int32_t> order;  // triangle indices, partitioned in place
    float pad;
    TvamMeshHost* out;

    void bounds(int b, int e, float lo[3], float hi[3]) const {
        for (int a = 0; a < 3; ++a) lo[a] = TVAM_INF, hi[a] = -TVAM_INF;
        for (int j = b; j < e; ++j)
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) {
                    const float x = tris[9 * (size_t)order[j] + 3 * v + a];
                    lo[a] = std::min(lo[a], x);
                    hi[a] = std::max(hi[a], x);
                }
    }

    // Emits the subtree over order[b, e) depth first; recursion depth <= log2(n) + 1 (median splits).
    void node(int b, int e) {
        const size_t me = out->nodes.size() / 2;
        float lo[3], hi[3];
        bounds(b, e, lo, hi);
        out->nodes.push_back(make_float4(lo[0] - pad, lo[1] - pad, lo[2] - pad, 0.0f));
        out->nodes.push_back(make_float4(hi[0] + pad, hi[1] + pad, hi[2] + pad, 0.0f));
        int32_t meta = 0;
        if (e - b <= TVAM_MESH_LEAF) {
            meta = (int32_t)(out->ids.size()) | ((e - b) << 28);
            for (int j = b; j < e; ++j) {
                out->ids.push_back(order[j]);
                out->tris.insert(out->tris.end(), tris + 9 * (size_t)order[j], tris + 9 * (size_t)order[j] + 9);
            }
        } else {
            // median split of the centroids along their widest axis (ties by index: deterministic)
            float clo[3] = {TVAM_INF, TVAM_INF, TVAM_INF}, chi[3] = {-TVAM_INF, -TVAM_INF, -TVAM_INF};
            for (int j = b; j < e; ++j)
                for (int a = 0; a < 3; ++a) {
                    clo[a] = std::min(clo[a], cen[3 * (size_t)order[j] + a]);
                    chi[a] = std::max(chi[a], cen[3 * (size_t)order[j] + a]);
                }
            int ax = 0;
            for (int a = 1; a < 3; ++a)
                if (chi[a] - clo[a] > chi[ax] - clo[ax]) ax = a;
            const int mid = b + (e - b) / 2;
            std::nth_element(order.begin() + b, order.begin() + mid, order.begin() + e, [&](int32_t x, int32_t y) {
                const float cx = cen[3 * (size_t)x + ax], cy = cen[3 * (size_t)y + ax];
                return cx < cy || (cx == cy && x < y);
            });
            node(b, mid);
            node(mid, e);
        }
        const int32_t skip = (int32_t)(out->nodes.size() / 2);
        std::memcpy(&out->nodes[2 * me].w, &skip, sizeof(skip));
        std::memcpy(&out->nodes[2 * me + 1].w, &meta, sizeof(meta));
    }
};

}  // namespace

// "mesh `name`: ..." for null / empty meshes, non-finite vertices and zero-area triangles; 0 if sound.
int tvam_mesh_validate(const char* name, const float* tris, int32_t n) {
    if (!tris || n <= 0)
        return tvam_fail(TVAM_ERR_INVALID, std::string("the ") + name + " vial mesh is null or empty");
    if (n >= (1 << 27))
        return tvam_fail(TVAM_ERR_TOO_LARGE, std::string("the ") + name + " vial mesh has too many triangles");
    for (int32_t i = 0; i < n; ++i) {
        const float* v = tris + 9 * (size_t)i;
        for (int q = 0; q < 9; ++q)
            if (!std::isfinite(v[q]))
                return tvam_fail(TVAM_ERR_INVALID, std::string("the ") + name + " vial mesh: triangle " +
                                                       std::to_string(i) + " has a non-finite vertex");
        float nx, ny, nz;
        tvam_tri_normal(v, nx, ny, nz);  // the kernels' own normal: it must exist
        if (!(std::isfinite(nx) && std::isfinite(ny) && std::isfinite(nz)))
            return tvam_fail(TVAM_ERR_INVALID, std::string("the ") + name + " vial mesh: triangle " +
                                                   std::to_string(i) + " has zero area");
    }
    return 0;
}

// The hierarchy over validated triangles [n][3][3].
void tvam_mesh_build(const float* tris, int32_t n, TvamMeshHost& out) {
    Builder b;
    b.tris = tris;
    b.out = &out;
    b.cen.resize(3 * (size_t)n);
    b.order.resize(n);
    std::iota(b.order.begin(), b.order.end(), 0);
    float big = 0.0f;
    for (int32_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float* v = tris + 9 * (size_t)i;
            b.cen[3 * (size_t)i + a] = (v[a] + v[3 + a] + v[6 + a]) / 3.0f;
            big = std::max({big, std::fabs(v[a]), std::fabs(v[3 + a]), std::fabs(v[6 + a])});
        }
    b.pad = TVAM_MESH_PAD * (1.0f + big);
    out.nodes.clear(), out.tris.clear(), out.ids.clear();
    out.nodes.reserve(4 * (size_t)n);
    out.tris.reserve(9 * (size_t)n);
    out.ids.reserve(n);
    b.node(0, n);
}

extern "C" int tvam_mesh_hit(const float* tris, int32_t n, const float* o, const float* d, int64_t n_rays,
                             int32_t use_bvh, float* t, int32_t* tri) {
    if ((n_rays > 0 && (!o || !d || !t || !tri)) || n_rays < 0) return tvam_fail(TVAM_ERR_INVALID, "null argument");
    int rc = tvam_mesh_validate("queried", tris, n);
    if (rc) return rc;
    TvamMeshHost h;
    tvam_mesh_build(tris, n, h);
    TvamMeshView m;
    m.nodes = h.nodes.data();
    m.tris = h.tris.data();
    m.ids = h.ids.data();
    m.n_nodes = (int32_t)(h.nodes.size() / 2);
    m.n_tris = n;
    m.n_inner = 0;
    for (int64_t i = 0; i < n_rays; ++i) {
        const float* oo = o + 3 * i;
        const float* dd = d + 3 * i;
        int slot;
        t[i] = use_bvh ? tvam_mesh_closest(m, TVAM_MESH_BOTH, oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], slot)
                       : tvam_mesh_closest_brute(m, TVAM_MESH_BOTH, oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], slot);
        tri[i] = slot < 0 ? -1 : m.ids[slot];
    }
    return 0;
}

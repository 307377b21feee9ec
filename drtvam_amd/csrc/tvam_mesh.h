// tvam_mesh.h -- closest hit of a ray with the triangle meshes of a 'custom' vial
// (geometry.py:98-138), host and device: the traversal of the bounding volume hierarchy that
// tvam_mesh.hip builds, and the brute-force loop it must agree with bit for bit.
//
// Layout (TvamMesh): a binary tree over the triangles of both meshes (inner mesh first), at most
// TVAM_MESH_LEAF triangles per leaf, stored depth first.  Node i is two float4: {lo.xyz, skip}
// and {hi.xyz, first | count << 28}; count = 0 marks an inner node, whose first child is node
// i + 1; `skip` is the node that follows i's subtree.  The triangles are stored in leaf order
// (a leaf's run is contiguous) with ids[] = their index in the caller's order.
//
// Traversal: i = (the ray meets node i's box) ? i + 1 : skip[i], from i = 0 until i = n_nodes;
// a leaf tests its triangles with tvam_tri_hit (t >= 0) on the way.  There is no stack, so no
// dynamically indexed per-thread array (which would live in scratch memory, see tvam_seg3d.h).
// The loop runs at most n_nodes times, and every index it follows (skip, first, count) was
// written by the host builder from validated input, never by a caller.
//
// Agreement with the brute-force loop: both keep the hit of least t and, among equal t, of least
// id, so the order of the tests does not matter; the hierarchy only has to test every triangle
// the loop would accept.  tvam_tri_hit's t is an fp32 result while the box test is exact about
// the box, so the builder grows every box by TVAM_MESH_PAD (1 + the meshes' largest |coordinate|):
// a triangle that tvam_tri_hit accepts at t has the ray within that rounding of it, inside the
// grown box, and the box's entry time lies below t by at least the pad, so the cut `entry <=
// best t` never drops a nearer or equal hit.
#pragma once
#include <vector>

#include "tvam_common.h"

#define TVAM_MESH_LEAF 4
#define TVAM_MESH_PAD 1e-3f
// LDS staging budget of the per-ray kernels: nodes, triangles and ids of
// both meshes are staged per workgroup when they take at most this many bytes
#define TVAM_MESH_LDS_BUDGET 16384
// Meshes of at most this many triangles (both surfaces together) are looped over instead: the
// reference's 16-triangle cuvette measured 7 % faster that way (adjoint 2.77 against 2.96 ms,
// DESIGN.md section 4f); the next size measured, 4096 triangles, is 13 x faster through the
// hierarchy.  Both give the same bits.
#define TVAM_MESH_BRUTE_MAX 16

// The three tables, wherever they live (global memory, or a workgroup's LDS copy).
struct TvamMeshView {
    const float4* nodes;
    const float* tris;
    const int32_t* ids;
    int32_t n_nodes, n_tris, n_inner;
};

TVAM_HD TvamMeshView tvam_mesh_view(const TvamMesh& m) {
    TvamMeshView v;
    v.nodes = m.nodes;
    v.tris = m.tris;
    v.ids = m.ids;
    v.n_nodes = m.n_nodes;
    v.n_tris = m.n_tris;
    v.n_inner = m.n_inner;
    return v;
}

// which: 0 = both meshes, 1 = the outer mesh alone (the first-hit pass of 'filter_corner')
#define TVAM_MESH_BOTH 0
#define TVAM_MESH_OUTER 1

// One triangle against the best hit so far: nearer wins, equal t goes to the lower id.
TVAM_HD void tvam_mesh_test(const TvamMeshView& m, int j, int which, float ox, float oy, float oz, float dx, float dy,
                            float dz, float& best, int& best_id, int& best_j) {
    const int id = m.ids[j];
    if (which == TVAM_MESH_OUTER && id < m.n_inner) return;
    const float t = tvam_tri_hit(m.tris + 9 * j, ox, oy, oz, dx, dy, dz);
    if (t < best || (t == best && t < TVAM_INF && id < best_id)) {
        best = t;
        best_id = id;
        best_j = j;
    }
}

// Closest hit through the hierarchy: the distance (TVAM_INF: none), slot = the triangle's
// position in m.tris (its vertices: m.tris + 9 * slot; its caller-order index: m.ids[slot]).
TVAM_HD float tvam_mesh_closest(const TvamMeshView& m, int which, float ox, float oy, float oz, float dx, float dy,
                                float dz, int& slot) {
    float best = TVAM_INF;
    int best_id = 0x7fffffff, best_j = -1;
    int i = 0;
    for (int it = 0; it < m.n_nodes && i < m.n_nodes; ++it) {
        const float4 lo = m.nodes[2 * i], hi = m.nodes[2 * i + 1];
        // slab test; a ray parallel to an axis gives +-inf, or NaN (0 / 0) on a box plane itself,
        // which fminf / fmaxf drop: such a ray runs in the grown box's boundary, the pad away
        // from every triangle inside
        const float ax = (lo.x - ox) / dx, bx = (hi.x - ox) / dx;
        const float ay = (lo.y - oy) / dy, by = (hi.y - oy) / dy;
        const float az = (lo.z - oz) / dz, bz = (hi.z - oz) / dz;
        const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
        const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
        const bool in = tn <= tf && tn <= best;
        const int meta = __builtin_bit_cast(int, hi.w);
        const int count = meta >> 28;
        if (in && count > 0) {
            const int first = meta & 0x0fffffff;
            for (int j = first; j < first + count; ++j)
                tvam_mesh_test(m, j, which, ox, oy, oz, dx, dy, dz, best, best_id, best_j);
        }
        i = in ? i + 1 : __builtin_bit_cast(int, lo.w);
    }
    slot = best_j;
    return best;
}

// The same over every triangle in storage order.
TVAM_HD float tvam_mesh_closest_brute(const TvamMeshView& m, int which, float ox, float oy, float oz, float dx,
                                      float dy, float dz, int& slot) {
    float best = TVAM_INF;
    int best_id = 0x7fffffff, best_j = -1;
    for (int j = 0; j < m.n_tris; ++j) tvam_mesh_test(m, j, which, ox, oy, oz, dx, dy, dz, best, best_id, best_j);
    slot = best_j;
    return best;
}

// Mitsuba's face normal of a 'ply' shape with face_normals = true: normalize((v1 - v0) x (v2 - v0)).
TVAM_HD void tvam_tri_normal(const float* v, float& nx, float& ny, float& nz) {
    const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
    const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const float len = sqrtf(cx * cx + cy * cy + cz * cz);
    nx = cx / len;
    ny = cy / len;
    nz = cz / len;
}

// The medium segment behind a 'custom' vial (volume.py:179-272 in transmission-only mode, the
// statement order of tvam_segment_square with all three components): from (o, d) the nearest hit
// over both meshes, the face normal, the dielectric transmission (eta_int behind an inner-mesh
// face, eta_ext behind an outer one; weight 0 = total internal reflection ends the ray), the
// spawn_ray offset along the normal on the side of wo, until a hit on the inner mesh leaves the
// ray running against the normal (n . wo < 0): it is in the medium, and the next nearest hit ends
// the segment.  No hit (an open end): no deposit, the rule of cn_segment.  At most max_depth
// surfaces.  BRUTE: the loop over every triangle whatever the size (the measurement build of
// DESIGN.md section 4f).
template <bool BRUTE = false>
TVAM_HD bool tvam_segment_mesh(const TvamMeshView& m, int max_depth, float eta_ext, float eta_int, const float o[3],
                               const float d[3], float o2[3], float d2[3], float& maxt, float& weight) {
    float px = o[0], py = o[1], pz = o[2], vx = d[0], vy = d[1], vz = d[2], att = 1.0f;
    bool in_medium = false;
    const bool loop = BRUTE || m.n_tris <= TVAM_MESH_BRUTE_MAX;
    for (int depth = 0; depth < max_depth; ++depth) {
        int slot;
        const float t = loop ? tvam_mesh_closest_brute(m, TVAM_MESH_BOTH, px, py, pz, vx, vy, vz, slot)
                              : tvam_mesh_closest(m, TVAM_MESH_BOTH, px, py, pz, vx, vy, vz, slot);
        if (!(t < TVAM_INF)) return false;
        if (in_medium) {
            o2[0] = px, o2[1] = py, o2[2] = pz;
            d2[0] = vx, d2[1] = vy, d2[2] = vz;
            maxt = t;
            weight = att;
            return true;
        }
        const bool inner = m.ids[slot] < m.n_inner;
        float nx, ny, nz;
        tvam_tri_normal(m.tris + 9 * slot, nx, ny, nz);
        const float hx = fmaf(vx, t, px), hy = fmaf(vy, t, py), hz = fmaf(vz, t, pz);
        float wx, wy, wz;
        const float w = tvam_transmit_world(nx, ny, nz, vx, vy, vz, inner ? eta_int : eta_ext, wx, wy, wz);
        if (!(w > 0.0f)) return false;
        att = att * w;
        const float mx = fmaxf(fmaxf(fabsf(hx), fabsf(hy)), fabsf(hz));
        float mag = (1.0f + mx) * TVAM_RAY_EPS;
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

// Host side (tvam_mesh.hip): the hierarchy over `n` triangles ([n][3][3], caller order).
struct TvamMeshHost {
    std::vector<float4> nodes;  // [2 n_nodes]
    std::vector<float> tris;    // leaf order
    std::vector<int32_t> ids;
};
// 0, or TVAM_ERR_INVALID with "the <name> vial mesh ..." as the calling thread's error
int tvam_mesh_validate(const char* name, const float* tris, int32_t n);
void tvam_mesh_build(const float* tris, int32_t n, TvamMeshHost& out);

// tvam_cone_ray.h -- ray generation of the telecentric / lens projectors (projector.py:199-296),
// shared by tvam_cone.hip (forward, adjoint, export) and tvam_corner.hip (the 'filter_corner'
// first-hit pass): the sampler draws, get_ray, CircularMotion's to_world and the medium segment
// behind the index-matched vial, or behind the mesh interfaces of a 'custom' vial (device only).
#pragma once
#include "tvam_mesh.h"
#include "tvam_path.h"
#include "tvam_seg3d.h"

namespace {

struct ConeRay {
    float o[3], d[3];  // world-space projector ray
    float o2[3];       // medium segment (o2, d2, [0, maxt])
    float maxt;
    float d2[3], att;  // 'custom' vial: the refracted direction and the interfaces' transmission weight
                       // (index matched: d and 1, and the kernels read d itself)
};

// How a kernel reads the meshes of a 'custom' vial.
enum ConeMesh { CN_NO_MESH = 0, CN_MESH_GLOBAL = 1, CN_MESH_LDS = 2 };

// The kernel's view of the meshes: global memory, or the workgroup's LDS copy (the three tables
// back to back in 16-byte rows; every thread of the workgroup calls this, before its ray loop).
template <int MESH>
__device__ __forceinline__ TvamMeshView cn_mesh_view(const TvamConsts& k, float4* lds) {
    TvamMeshView m = tvam_mesh_view(k.mesh);
    if (MESH == CN_MESH_LDS) {
        const int n4 = 2 * m.n_nodes, t4 = (9 * m.n_tris + 3) / 4, i4 = (m.n_tris + 3) / 4;
        const float4* gt = reinterpret_cast<const float4*>(k.mesh.tris);
        const float4* gi = reinterpret_cast<const float4*>(k.mesh.ids);
        for (int i = threadIdx.x; i < n4; i += blockDim.x) lds[i] = k.mesh.nodes[i];
        for (int i = threadIdx.x; i < t4; i += blockDim.x) lds[n4 + i] = gt[i];
        for (int i = threadIdx.x; i < i4; i += blockDim.x) lds[n4 + t4 + i] = gi[i];
        __syncthreads();
        m.nodes = lds;
        m.tris = reinterpret_cast<const float*>(lds + n4);
        m.ids = reinterpret_cast<const int32_t*>(lds + n4 + t4);
    }
    return m;
}

// Bytes of that copy (the launch's dynamic LDS; tvam_plan.hip's TvamMesh::lds_bytes bounds it).
inline size_t cn_mesh_lds_bytes(const TvamMesh& m) {
    return sizeof(float4) * ((size_t)2 * m.n_nodes + (9 * (size_t)m.n_tris + 3) / 4 + ((size_t)m.n_tris + 3) / 4);
}

#ifndef TVAM_MESH_BRUTE
#define TVAM_MESH_BRUTE 0  // 1: a measurement build whose kernels loop over every triangle
#endif

// 'custom' vial: the medium segment of the world ray (r.o, r.d) through the mesh interfaces.
__device__ __forceinline__ bool cn_segment_mesh(const TvamConsts& k, const TvamMeshView& m, ConeRay& r) {
    return tvam_segment_mesh<TVAM_MESH_BRUTE != 0>(m, k.max_depth, k.eta_ext, k.eta_int, r.o, r.d, r.o2, r.d2, r.maxt,
                                                   r.att);
}

// Mitsuba warp::square_to_uniform_disk_concentric (Shirley & Chiu), restated
__device__ __forceinline__ void cn_disk(float u1, float u2, float& x, float& y) {
    const float sx = 2.0f * u1 - 1.0f, sy = 2.0f * u2 - 1.0f;
    const bool q = fabsf(sx) < fabsf(sy);
    const float r = q ? sy : sx, rp = q ? sx : sy;
    float phi = 0.78539816339744830962f * rp / r;
    if (q) phi = 1.57079632679489661923f - phi;
    if (sx == 0.0f && sy == 0.0f) phi = 0.0f;
    x = r * cosf(phi);
    y = r * sinf(phi);
}

// Index-matched vial, 3-D ray (Mitsuba's open cylinder with a null BSDF, volume.py:191-216):
// the first tube hit is the entry only when it is front-facing (else the ray came in through an
// open end and never enters the medium through the interface: no deposit); o2 is the hit offset
// inward by spawn_ray's (1 + max|p|) eps (or_segment_index_matched's rule); the segment ends at
// the next tube hit from o2, and a ray that leaves through an open end has no valid si there
// (volume.py:268): no deposit either.
__device__ __forceinline__ bool cn_segment(const TvamConsts& k, ConeRay& r) {
    const float t0 = sc_tube_hit(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], k.vial_r, k.vial_half_h);
    if (!(t0 < TVAM_INF)) return false;
    const float px = fmaf(r.d[0], t0, r.o[0]), py = fmaf(r.d[1], t0, r.o[1]), pz = fmaf(r.d[2], t0, r.o[2]);
    const float rp = sqrtf(px * px + py * py);
    const float nx = px / rp, ny = py / rp;
    const float ndd = nx * r.d[0] + ny * r.d[1] + 0.0f * r.d[2];
    if (!(ndd < 0.0f)) return false;
    const float m = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
    const float mag = -((1.0f + m) * TVAM_RAY_EPS);
    r.o2[0] = fmaf(mag, nx, px);
    r.o2[1] = fmaf(mag, ny, py);
    r.o2[2] = pz;
    const float t1 = sc_tube_hit(r.o2[0], r.o2[1], r.o2[2], r.d[0], r.d[1], r.d[2], k.vial_r, k.vial_half_h);
    if (!(t1 < TVAM_INF)) return false;
    r.maxt = t1;
    return true;
}

// The ray of shard angle `al`, crop pixel (colc, rowc), drawn from sampler stream `stream` of seed
// tp.seed, and its medium segment.  Returns whether it deposits.  The collimated projector takes
// tvam_ray_world / tvam_segment_im (the ray records' own expressions), so that the export of such
// a plan is the oracle's ray bit for bit.
template <int MESH = CN_NO_MESH>
__device__ __forceinline__ bool cn_ray_at(const TvamConsts& k, const TvamTiles& tp, int al, int colc, int rowc,
                                          uint64_t stream, ConeRay& r, const TvamMeshView* mesh = nullptr) {
    TvamPcg rng;
    const TvamPathDraws dr = tvam_path_draws<true, true>(k, tp, al, stream, rng);
    const float c = dr.c, sn = dr.sn;
    float xc, yc;
    tvam_ray_camera(k, k.crop_off_x + colc, k.crop_off_y + rowc, dr.jx, dr.jy, xc, yc);
    if (k.proj_type == TVAM_PROJECTOR_COLLIMATED) {
        tvam_ray_world(k, c, sn, xc, yc, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1]);
        r.d[2] = 0.0f;
        if (MESH != CN_NO_MESH) return cn_segment_mesh(k, *mesh, r);
        r.o2[2] = r.o[2];
        return tvam_segment_im(k, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.o2[0], r.o2[1], r.maxt);
    }
    float ax, ay;
    cn_disk(dr.u1, dr.u2, ax, ay);
    ax = k.ap_r * ax;
    ay = k.ap_r * ay;
    // camera space: origin (X, Y, 0) on the aperture plane, direction towards the pixel's point of
    // the focus plane
    float X, Y, vx, vy, vz;
    if (k.proj_type == TVAM_PROJECTOR_TELECENTRIC) {  // projector.py:220-234
        X = xc + ax;
        Y = yc + ay;
        vx = -ax;
        vy = -ay;
        vz = 0.005f + k.focus;  // the pixel's point sits on the near plane z_c = 0.005
    } else {  // projector.py:273-286: focus_p = near_p (focus_distance / near_p.z) = (xc, yc, focus)
        X = ax;
        Y = ay;
        vx = xc - ax;
        vy = yc - ay;
        vz = k.focus;
    }
    const float inv = 1.0f / sqrtf(vx * vx + vy * vy + vz * vz);
    vx = vx * inv;
    vy = vy * inv;
    vz = vz * inv;
    // to_world (motion.py:26-36; tvam_ray_world with a general camera point and direction):
    // (X, Y, Z) -> (c (D - Z) + s X, s (D - Z) - c X, Y), Z = 0
    const float D = k.dist;
    r.o[0] = c * D + sn * X;
    r.o[1] = sn * D - c * X;
    r.o[2] = Y;
    r.d[0] = sn * vx - c * vz;
    r.d[1] = -sn * vz - c * vx;
    r.d[2] = vy;
    if (MESH != CN_NO_MESH) return cn_segment_mesh(k, *mesh, r);
    return cn_segment(k, r);
}

}  // namespace

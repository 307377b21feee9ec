// tvam_cone_ray.h -- ray generation of the telecentric / lens projectors (projector.py:199-296),
// shared by tvam_ray3d.hip (forward, adjoint, export) and tvam_corner.hip (the 'filter_corner'
// first-hit pass): the sampler draws, get_ray, CircularMotion's to_world and the medium segment
// behind the index-matched vial, behind the mesh interfaces of a 'custom' vial or behind the two
// analytic glass surfaces of a traced 'cylindrical' / 'square' vial (tvam_glass.h), and the per-ray
// DDA of a 3-D segment (cn_dda), which tvam_ray3d.hip marches (device only).
#pragma once
#include "tvam_glass.h"
#include "tvam_mesh.h"
#include "tvam_path.h"
#include "tvam_seg3d.h"

namespace {

struct ConeRay {
    float o[3], d[3];  // world-space projector ray
    float o2[3];       // medium segment (o2, d2, [0, maxt])
    float maxt;
    float d2[3], att;  // 'custom' and traced glass vials: the refracted direction and the interfaces' transmission weight
                       // (index matched: d and 1, and the kernels read d itself)
};

// How a kernel finds the medium segment: behind the index-matched vial, through the meshes of a
// 'custom' vial (and how it reads them), or through the analytic glass surfaces of a traced
// 'cylindrical' / 'square' vial (tvam_plan_create_traced).
enum ConeMesh { CN_NO_MESH = 0, CN_MESH_GLOBAL = 1, CN_MESH_LDS = 2, CN_GLASS = 3 };

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

// MESH of a launch over a 3-D ray plan and its dynamic LDS.
inline int cn_mesh_mode(const TvamConsts& k) {
    // (a glass vial reaches these kernels only through a traced plan: tvam_plan_create's plans of
    // such a vial are planar)
    if (k.vial_type == TVAM_VIAL_CYLINDRICAL || k.vial_type == TVAM_VIAL_SQUARE) return CN_GLASS;
    return k.vial_type != TVAM_VIAL_CUSTOM ? CN_NO_MESH : (k.mesh.lds_bytes > 0 ? CN_MESH_LDS : CN_MESH_GLOBAL);
}
inline size_t cn_lds(const TvamConsts& k) { return cn_mesh_mode(k) == CN_MESH_LDS ? cn_mesh_lds_bytes(k.mesh) : 0; }

#ifndef TVAM_MESH_BRUTE
#define TVAM_MESH_BRUTE 0  // 1: a measurement build whose kernels loop over every triangle
#endif

// 'custom' vial: the medium segment of the world ray (r.o, r.d) through the mesh interfaces.
__device__ __forceinline__ bool cn_segment_mesh(const TvamConsts& k, const TvamMeshView& m, ConeRay& r) {
    return tvam_segment_mesh<TVAM_MESH_BRUTE != 0>(m, k.max_depth, k.eta_ext, k.eta_int, r.o, r.d, r.o2, r.d2, r.maxt,
                                                   r.att);
}

// traced 'cylindrical' / 'square' vial: the medium segment through the two analytic glass surfaces.
__device__ __forceinline__ bool cn_segment_glass(const TvamConsts& k, ConeRay& r) {
    return tvam_segment_traced(k, r.o, r.d, r.o2, r.d2, r.maxt, r.att);
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
// a plan is the oracle's ray bit for bit.  RAY_ONLY: the world-space projector ray (r.o, r.d) alone,
// for a caller that traces the vial itself (WalkDouble, tvam_ray3d.h).  rng: the ray's generator, left after
// the prefix for a caller whose path loop goes on drawing (WalkInsert, tvam_ray3d.h).
template <int MESH = CN_NO_MESH, bool RAY_ONLY = false>
__device__ __forceinline__ bool cn_ray_at(const TvamConsts& k, const TvamTiles& tp, int al, int colc, int rowc,
                                          uint64_t stream, ConeRay& r, TvamPcg& rng,
                                          const TvamMeshView* mesh = nullptr) {
    const TvamPathDraws dr = tvam_path_draws<true, true>(k, tp, al, stream, rng);
    const float c = dr.c, sn = dr.sn;
    float xc, yc;
    tvam_ray_camera(k, k.crop_off_x + colc, k.crop_off_y + rowc, dr.jx, dr.jy, xc, yc);
    if (k.proj_type == TVAM_PROJECTOR_COLLIMATED) {
        tvam_ray_world(k, c, sn, xc, yc, r.o[0], r.o[1], r.o[2], r.d[0], r.d[1]);
        r.d[2] = 0.0f;
        if (RAY_ONLY) return true;
        if (MESH == CN_GLASS) return cn_segment_glass(k, r);
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
    if (RAY_ONLY) return true;
    if (MESH == CN_GLASS) return cn_segment_glass(k, r);
    if (MESH != CN_NO_MESH) return cn_segment_mesh(k, *mesh, r);
    return cn_segment(k, r);
}

// ... for a caller that draws nothing after the prefix.
template <int MESH = CN_NO_MESH, bool RAY_ONLY = false>
__device__ __forceinline__ bool cn_ray_at(const TvamConsts& k, const TvamTiles& tp, int al, int colc, int rowc,
                                          uint64_t stream, ConeRay& r, const TvamMeshView* mesh = nullptr) {
    TvamPcg rng;
    return cn_ray_at<MESH, RAY_ONLY>(k, tp, al, colc, rowc, stream, r, rng, mesh);
}

// The projector ray alone.
__device__ __forceinline__ void cn_projector_ray(const TvamConsts& k, const TvamTiles& tp, int al, int colc, int rowc,
                                                 uint64_t stream, ConeRay& r) {
    (void)cn_ray_at<CN_NO_MESH, true>(k, tp, al, colc, rowc, stream, r);
}

// The segment's DDA (sensor.py:327-438), stepped like the oracle's or_dda op for op in fp32: the
// box clip, start / end voxel, dtmax / tstep per axis, then per visit dt = min(dtmax, remaining),
// dtmax -= dt (an axis at its crossing restarts from tstep), so a ray visits exactly the oracle's
// voxels (sc_dda's closed-form crossing times fmaf(n, ts, dtm0) can split a near-tie the other
// way).  cn_dda_steps is the stepping alone, shared by cn_dda and the extinction derivative
// (tvam_dsigma.hip): visit(film index, t, dt) per voxel visit, t the in-medium path length from o
// at which the visit starts.
template <typename F>
__device__ __forceinline__ void cn_dda_steps(const TvamConsts& k, const float o[3], const float d[3], float maxt,
                                             F&& visit) {
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float tb0 = (k.bmin[a] - o[a]) / d[a];
        const float tb1 = (k.bmax[a] - o[a]) / d[a];
        lo[a] = fminf(tb0, tb1);
        hi[a] = fmaxf(tb0, tb1);
    }
    const float t_start = fmaxf(fmaxf(fmaxf(fmaxf(lo[0], lo[1]), lo[2]), 0.0f), 0.0f);
    const float t_end = fminf(fminf(fminf(hi[0], hi[1]), hi[2]), maxt);
    if (!(isfinite(t_start) && isfinite(t_end) && t_start < t_end)) return;
    // axes in scalars (dynamically indexed arrays would be promoted to scratch)
    int cur[3], endv[3], step[3];
    float dtm[3], ts[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float gs = fmaf(d[a], t_start, o[a]), ge = fmaf(d[a], t_end, o[a]);
        step[a] = d[a] > 0.0f ? 1 : -1;
        int sv = (int)((gs - k.bmin[a]) / k.h[a]);
        int ev = (int)((ge - k.bmin[a]) / k.h[a]);
        sv = sv < 0 ? 0 : (sv > k.res[a] - 1 ? k.res[a] - 1 : sv);
        ev = ev < 0 ? 0 : (ev > k.res[a] - 1 ? k.res[a] - 1 : ev);
        cur[a] = sv;
        endv[a] = ev;
        float next = k.bmin[a] + (float)(sv + step[a]) * k.h[a];
        if (d[a] < 0.0f) next = next + k.h[a];
        const bool valid = fabsf(d[a]) > 1e-8f;
        float dt0 = valid ? (next - gs) / d[a] : TVAM_INF;
        if (dt0 < 0.0f) dt0 = TVAM_INF;  // sensor.py:358: the axis never steps
        dtm[a] = dt0;
        ts[a] = valid ? (k.h[a] / d[a]) * (float)step[a] : TVAM_INF;
    }
    const int64_t sy = k.res[0], sz = (int64_t)k.res[0] * k.res[1];
    float t = t_start, remaining = t_end - t_start;
    // a ray steps at most res - 1 times per axis (the guard only bounds the loop)
    const int nmax = k.res[0] + k.res[1] + k.res[2] + 1;
    for (int it = 0; it < nmax; ++it) {
        const float dt = fminf(fminf(fminf(dtm[0], dtm[1]), dtm[2]), remaining);
        remaining = remaining - dt;
        const int64_t idx = cur[0] + cur[1] * sy + cur[2] * sz;
        visit(idx, t, dt);
        const bool alive = (cur[0] != endv[0] || cur[1] != endv[1] || cur[2] != endv[2]) && remaining > 1e-6f;
        if (!alive) break;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const bool m = dtm[a] == dt;
            dtm[a] = m ? ts[a] : dtm[a] - dt;
            cur[a] += m ? step[a] : 0;
        }
        if (cur[0] < 0 || cur[1] < 0 || cur[2] < 0 || cur[0] >= k.res[0] || cur[1] >= k.res[1] || cur[2] >= k.res[2])
            break;
        t = t + dt;
    }
}

// The visit weight e^{-st t} (1 - e^{-st dt}) without cancellation (tvam_omexp).  FWD adds
// em * weight into dose, ADJ returns sum weight * grad * inv_vol, COUNT counts visits.
template <int MODE>
__device__ __forceinline__ float cn_dda(const TvamConsts& k, const float o[3], const float d[3], float maxt, float em,
                                        float* __restrict__ dose, const float* __restrict__ gin, uint64_t& nvis) {
    float acc = 0.0f;
    cn_dda_steps(k, o, d, maxt, [&](int64_t idx, float t, float dt) {
        if (MODE != TVAM_MODE_COUNT) {
            const float c = sc_exp2(k.nsig2 * t) * tvam_omexp(k.sig_t * fmaxf(dt, 0.0f));
            if (MODE == TVAM_MODE_FWD) atomicAdd(&dose[idx], em * c);
            else acc = fmaf(c, gin[idx] * k.inv_vol, acc);
        }
        ++nvis;
    });
    return acc;
}

}  // namespace

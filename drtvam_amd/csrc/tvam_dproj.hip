// Projector derivatives: d dose / d theta for one parameter theta of a
// telecentric / lens projector behind the index-matched vial (distance, focus_distance,
// aperture_radius, pixel size), pathwise: the sampler draws, the (ray, sample) -> voxel bookkeeping
// and every discrete decision are held fixed.
//
//   tvam_dproj_kernel<FWD>  the tangent film T[v] = d dose[v] / d theta, global float atomics
//   tvam_dproj_kernel<ADJ>  the scalar g = sum_v G[v] T[v]: per ray a gather in fp32, the rays summed
//                           in fp64 by wave shuffles, then the workgroup's 4 waves through LDS; one
//                           partial per workgroup, summed in a fixed order (tvam_launch_partial_sum)
// One thread per (ray, sample).  The ray and its segment are cn_ray_at's own; dp_ray_tangent forms
// the tangent of (o2, d, maxt) in fp64 from the same draws, and dp_dda_steps is cn_dda_steps' stepping
// with the tangent of every visit's two end times.
#include "tvam_plan.h"

#include "tvam_cone_ray.h"
#include "tvam_dproj.h"

namespace {

// What dp_dda_steps needs of the fp64 segment and its tangent: face j of axis a (the plane
// bmin_a + j h_a) is crossed at t = (bmin_a + j h_a - o2_a) / d_a = P_a + j Q_a, which moves by
// t' = -(o2'_a + t d'_a) / d_a = A_a + t B_a; the segment ends at maxt, which moves by maxt_p.
// Doubles: near the focus A_a and t B_a cancel, and an axis the ray hardly moves along divides by a
// small d_a.
struct DpTan {
    double P[3], Q[3], A[3], B[3], maxt, maxt_p;
};

// The nearer root t >= 0 of |o_xy + t d_xy| = r whose z lies in the tube (sc_tube_hit's choice).
__device__ __forceinline__ double dp_tube_hit(const double o[3], const double d[3], double r, double half) {
    const double a = d[0] * d[0] + d[1] * d[1], b = 2.0 * (d[0] * o[0] + d[1] * o[1]);
    const double c = o[0] * o[0] + o[1] * o[1] - r * r;
    const double sq = sqrt(fmax(b * b - 4.0 * a * c, 0.0));
    const double q = -0.5 * (b + copysign(sq, b));
    const double r0 = q / a, r1 = c / q;
    const double t0 = fmin(r0, r1), t1 = fmax(r0, r1);
    const double zn = fma(d[2], t0, o[2]);
    return t0 >= 0.0 && zn >= -half && zn <= half ? t0 : t1;
}

// The tangent of cn_ray_at's ray (telecentric / lens, index-matched vial; a ray that deposits) under
// the draws dr.  The ray is formed again in fp64 from the draws by cn_ray_at's and cn_segment's
// expressions, and its tangent beside it: a ray that is nearly parallel to a voxel face has a
// direction component that is the small difference of two camera-space lengths, the crossing times of
// that axis' faces move by 1 / that component, and the fp32 component is good to 1e-5 of itself only.
__device__ __forceinline__ void dp_ray_tangent(const TvamConsts& k, const TvamDproj& dp, const TvamPathDraws& dr,
                                               int colc, int rowc, DpTan& g) {
    // tvam_ray_camera: ((0.5 - u) W p_x, (0.5 - v) H p_y), u = (col + jx) / W
    const double W = k.res_x, H = k.res_y, p_x = dp.px, p_y = dp.py;
    const double xc = (0.5 - ((double)(k.crop_off_x + colc) + (double)dr.jx) / W) * W * p_x;
    const double yc = (0.5 - ((double)(k.crop_off_y + rowc) + (double)dr.jy) / H) * H * p_y;
    // cn_disk
    double ux, uy;
    {
        const double sx = 2.0 * (double)dr.u1 - 1.0, sy = 2.0 * (double)dr.u2 - 1.0;
        const bool q = fabs(sx) < fabs(sy);
        const double r = q ? sy : sx, rp = q ? sx : sy;
        double phi = 0.78539816339744830962 * rp / r;
        if (q) phi = 1.57079632679489661923 - phi;
        if (sx == 0.0 && sy == 0.0) phi = 0.0;
        ux = r * cos(phi);
        uy = r * sin(phi);
    }
    const double R = k.ap_r, F = k.focus, D = k.dist;
    const double ax = R * ux, ay = R * uy;
    const bool tele = k.proj_type == TVAM_PROJECTOR_TELECENTRIC;
    // camera space: origin (X, Y, 0), unnormalised direction v; their tangents and the distance's
    const double X = tele ? xc + ax : ax, Y = tele ? yc + ay : ay;
    const double vx = tele ? -ax : xc - ax, vy = tele ? -ay : yc - ay, vz = tele ? 0.005 + F : F;
    double Xp = 0.0, Yp = 0.0, Dp = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
    if (dp.param == TVAM_DPROJ_DISTANCE) {
        Dp = 1.0;
    } else if (dp.param == TVAM_DPROJ_FOCUS_DISTANCE) {
        wz = 1.0;
    } else if (dp.param == TVAM_DPROJ_APERTURE_RADIUS) {
        Xp = ux, Yp = uy;
        wx = -ux, wy = -uy;
    } else {  // TVAM_DPROJ_PIXEL_SIZE: xc = (0.5 - u) W p_x
        const double sx = xc / p_x, sy = yc / p_y;
        if (tele) Xp = sx, Yp = sy;
        else wx = sx, wy = sy;
    }
    // normalisation: d^' = (v' - d^ (d^ . v')) / |v|
    const double inv = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
    const double hx = vx * inv, hy = vy * inv, hz = vz * inv;
    const double hw = hx * wx + hy * wy + hz * wz;
    const double hxp = (wx - hx * hw) * inv, hyp = (wy - hy * hw) * inv, hzp = (wz - hz * hw) * inv;
    // to_world at the ray's own angle: (X, Y, 0) -> (c D + s X, s D - c X, Y), direction alike
    const double c = dr.c, sn = dr.sn;
    const double o[3] = {c * D + sn * X, sn * D - c * X, Y};
    const double d[3] = {sn * hx - c * hz, -sn * hz - c * hx, hy};
    const double op[3] = {c * Dp + sn * Xp, sn * Dp - c * Xp, Yp};
    const double dq[3] = {sn * hxp - c * hzp, -sn * hzp - c * hxp, hyp};
    // cn_segment: entry time t0, entry point p, normal n, spawn offset, exit time maxt
    const double rv = k.vial_r, half = k.vial_half_h, eps = TVAM_RAY_EPS;
    const double t0 = dp_tube_hit(o, d, rv, half);
    const double px = fma(d[0], t0, o[0]), py = fma(d[1], t0, o[1]), pz = fma(d[2], t0, o[2]);
    const double rp = sqrt(px * px + py * py);
    const double nx = px / rp, ny = py / rp;
    const double ndd = nx * d[0] + ny * d[1];
    const double t0p = -(nx * fma(t0, dq[0], op[0]) + ny * fma(t0, dq[1], op[1])) / ndd;
    const double ppx = fma(t0, dq[0], fma(t0p, d[0], op[0]));
    const double ppy = fma(t0, dq[1], fma(t0p, d[1], op[1]));
    const double ppz = fma(t0, dq[2], fma(t0p, d[2], op[2]));
    // o2 = p - mag n, mag = (1 + max |p|) eps: n turns with p, mag moves with the largest |component|
    const double apx = fabs(px), apy = fabs(py), apz = fabs(pz);
    const double m = fmax(fmax(apx, apy), apz);
    const double mp = apx == m ? (px < 0.0 ? -ppx : ppx) : (apy == m ? (py < 0.0 ? -ppy : ppy) : (pz < 0.0 ? -ppz : ppz));
    const double mag = (1.0 + m) * eps;
    const double npp = nx * ppx + ny * ppy;
    const double npx = (ppx - nx * npp) / rp, npy = (ppy - ny * npp) / rp;
    const double o2[3] = {px - mag * nx, py - mag * ny, pz};
    const double o2p[3] = {ppx - (eps * mp) * nx - mag * npx, ppy - (eps * mp) * ny - mag * npy, ppz};
    // exit: |q_xy| = r at q = o2 + maxt d
    const double maxt = dp_tube_hit(o2, d, rv, half);
    const double qx = fma(d[0], maxt, o2[0]), qy = fma(d[1], maxt, o2[1]);
    g.maxt_p = -(qx * fma(maxt, dq[0], o2p[0]) + qy * fma(maxt, dq[1], o2p[1])) / (qx * d[0] + qy * d[1]);
    g.maxt = maxt;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool moves = d[a] != 0.0;  // (an axis the ray does not move along crosses no face)
        const double lo = k.bmin[a], hv = ((double)k.bmax[a] - lo) / (double)k.res[a];
        g.P[a] = moves ? (lo - o2[a]) / d[a] : 0.0;
        g.Q[a] = moves ? hv / d[a] : 0.0;
        g.A[a] = moves ? -o2p[a] / d[a] : 0.0;
        g.B[a] = moves ? -dq[a] / d[a] : 0.0;
    }
}

// An event of the march: the in-medium path length at which the fp64 ray reaches it, and its tangent.
struct DpEvent {
    float t, tp;
};

// cn_dda_steps' stepping, op for op: it decides which voxels a ray visits and which face ends each
// visit.  Beside it, the two events that bound every visit, from the fp64 ray (DpTan):
// visit(film index, event a, event b).  The segment's start t = 0 does not move; its end maxt moves
// by g.maxt_p; face j of axis a (the plane bmin_a + j h_a) is crossed at t = P_a + j Q_a and moves
// by t' = A_a + t B_a.  (The stepping's own fp32 times accumulate dtm - dt over the visits: good for
// the dose, which is continuous in them, but the tangent of a ray that is nearly parallel to a face
// multiplies them by 1 / d_a.)
template <typename F>
__device__ __forceinline__ void dp_dda_steps(const TvamConsts& k, const float o[3], const float d[3], float maxt,
                                             const DpTan& g, F&& visit) {
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
    // face j of axis a
    auto face = [&](int a, int j) {
        const double tc = fma((double)j, g.Q[a], g.P[a]);
        return DpEvent{(float)tc, (float)fma(tc, g.B[a], g.A[a])};
    };
    // the box faces a ray enters and leaves through: plane 0 or res of the axis
    auto box_in = [&](int a) { return face(a, d[a] > 0.0f ? 0 : k.res[a]); };
    auto box_out = [&](int a) { return face(a, d[a] > 0.0f ? k.res[a] : 0); };
    const DpEvent ev_start = !(t_start > 0.0f) ? DpEvent{0.0f, 0.0f}
                                               : (lo[0] == t_start ? box_in(0) : (lo[1] == t_start ? box_in(1) : box_in(2)));
    const DpEvent ev_end = t_end == maxt ? DpEvent{(float)g.maxt, (float)g.maxt_p}
                                         : (hi[0] == t_end ? box_out(0) : (hi[1] == t_end ? box_out(1) : box_out(2)));
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
        if (dt0 < 0.0f) dt0 = TVAM_INF;
        dtm[a] = dt0;
        ts[a] = valid ? (k.h[a] / d[a]) * (float)step[a] : TVAM_INF;
    }
    const int64_t sy = k.res[0], sz = (int64_t)k.res[0] * k.res[1];
    float remaining = t_end - t_start;
    DpEvent ea = ev_start;
    const int nmax = k.res[0] + k.res[1] + k.res[2] + 1;
    for (int it = 0; it < nmax; ++it) {
        const float dmin = fminf(fminf(dtm[0], dtm[1]), dtm[2]);
        const float dt = fminf(dmin, remaining);
        // the visit ends at the segment's end, or at the face of the first axis that steps: the far
        // face of the voxel along that axis
        const DpEvent eb = !(dmin < remaining) ? ev_end
                           : (dtm[0] == dt ? face(0, cur[0] + (step[0] > 0))
                                           : (dtm[1] == dt ? face(1, cur[1] + (step[1] > 0)) : face(2, cur[2] + (step[2] > 0))));
        remaining = remaining - dt;
        const int64_t idx = cur[0] + cur[1] * sy + cur[2] * sz;
        visit(idx, ea, eb);
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
        ea = eb;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void tvam_dproj_kernel(TvamConsts k, TvamTiles tp, TvamDproj dp,
                                                         const float* __restrict__ pat,
                                                         const int32_t* __restrict__ idxmap,
                                                         const float* __restrict__ gin, float* __restrict__ tangent,
                                                         double* __restrict__ partials) {
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * (int)tp.spp;
    const bool f32 = tvam_path_fits32(n);
    // the ray weight ~ p_x p_y: w' / w
    const float wrel = dp.param == TVAM_DPROJ_PIXEL_SIZE ? 1.0f / dp.px + 1.0f / dp.py : 0.0f;
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        // FWD: em = pattern * wscale * inv_vol; ADJ: pattern * wscale (inv_vol goes with the gathered gradient)
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_FWD>(k, pat, idxmap, ix.local, k.wscale, MODE == TVAM_MODE_FWD ? k.inv_vol : 1.0f,
                                           em, act))
            continue;
        tvam_path_pixel(k, f32, ix);
        const uint64_t stream = tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp);
        ConeRay r;
        if (!cn_ray_at<CN_NO_MESH>(k, tp, ix.al, ix.colc, ix.rowc, stream, r)) continue;
        TvamPcg rng;  // (cn_ray_at's draws again: the same stream, the same numbers)
        const TvamPathDraws dr = tvam_path_draws<true, true>(k, tp, ix.al, stream, rng);
        DpTan g;
        dp_ray_tangent(k, dp, dr, ix.colc, ix.rowc, g);
        float acc = 0.0f;
        dp_dda_steps(k, r.o2, r.d, r.maxt, g, [&](int64_t idx, const DpEvent& a, const DpEvent& b) {
            // d / d theta of e^{-st t_a} - e^{-st t_b}, and the weight's share of the deposit itself
            const float ea = sc_exp2(k.nsig2 * a.t), eb = sc_exp2(k.nsig2 * b.t);
            float w = k.sig_t * (eb * b.tp - ea * a.tp);
            if (wrel != 0.0f) w = fmaf(wrel, ea * tvam_omexp(k.sig_t * fmaxf(b.t - a.t, 0.0f)), w);
            if (MODE == TVAM_MODE_FWD) atomicAdd(&tangent[idx], em * w);
            else acc = fmaf(w, gin[idx] * k.inv_vol, acc);
        });
        if (MODE == TVAM_MODE_ADJ) sum += (double)em * (double)acc;
    }
    if (MODE == TVAM_MODE_ADJ) {
        __shared__ double s_wave[4];
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) partials[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
    }
}

}  // namespace

hipError_t tvam_launch_dproj(int mode, const TvamConsts& k, const TvamTiles& t, const TvamDproj& dp, const float* pat,
                             const int32_t* idxmap, const float* gin, float* tangent, double* partials, double* g,
                             hipStream_t stream) {
    const unsigned grid = tvam_dsigma_grid((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp);
    if (mode == TVAM_MODE_FWD)
        hipLaunchKernelGGL(tvam_dproj_kernel<TVAM_MODE_FWD>, dim3(grid), dim3(256), 0, stream, k, t, dp, pat, idxmap, gin,
                           tangent, partials);
    else
        hipLaunchKernelGGL(tvam_dproj_kernel<TVAM_MODE_ADJ>, dim3(grid), dim3(256), 0, stream, k, t, dp, pat, idxmap, gin,
                           tangent, partials);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && mode == TVAM_MODE_ADJ) e = tvam_launch_partial_sum(partials, (int)grid, g, stream);
    return e;
}

// tvam_seg3d.h -- the 3-D medium segment shared by the scattered segments (tvam_scatter.hip) and the
// segments of the 3-D ray plans (tvam_ray3d.hip): the open-tube hit of a 3-D ray, the per-ray DDA
// march and the brick-bin record of a segment (device only).
#pragma once
#include "tvam_bricks.h"

namespace {

__device__ __forceinline__ float sc_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Nearest hit t >= 0 of the open tube (radius r, |z| <= half) for a 3-D ray
// (Mitsuba cylinder restated; oracle or_tube_hit).
__device__ __forceinline__ float sc_tube_hit(float ox, float oy, float oz, float dx, float dy, float dz, float r,
                                             float half) {
    float t0, t1;
    if (!tvam_cyl_roots(ox, oy, dx, dy, r, t0, t1)) return TVAM_INF;
    if (!(t1 >= 0.0f)) return TVAM_INF;
    const float zn = fmaf(dz, t0, oz), zf = fmaf(dz, t1, oz);
    if (t0 >= 0.0f && zn >= -half && zn <= half) return t0;
    if (zf >= -half && zf <= half) return t1;
    return TVAM_INF;
}

// The visits of a segment inside the voxel box [lo, hi) (a brick), resumed in
// closed form at the box entry: per axis the step count n at the entry time,
// the next crossing at t = dtm0 + n ts (fmaf from the count, so a visit splits
// at a brick face exactly where the neighbouring brick resumes), one axis per
// visit (ties: x before y before z).  Axes are kept in scalars (dynamically
// indexed arrays would be promoted to LDS).  F(local x, y, z, weight
// e^{-st t0} - e^{-st t1}).
template <typename F>
__device__ __forceinline__ void sc_box_march(const TvamConsts& k, const SegDda& q, const int lo[3], const int hi[3],
                                             F&& f) {
    float tin[3], tout[3];
    int nin[3], nout[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        tvam_axis_window(q.sv[a], q.step[a], q.dtm0[a], q.ts[a], lo[a], hi[a], tin[a], tout[a], nin[a], nout[a]);
    const float tau_e = fmaxf(fmaxf(fmaxf(tin[0], tin[1]), tin[2]), 0.0f);
    const float tau_x = fminf(fminf(fminf(tout[0], tout[1]), tout[2]), q.tau_end);
    if (!(tau_e < tau_x)) return;
    int n0 = tvam_axis_steps(tau_e, q.dtm0[0], q.ts[0], nin[0], nout[0]);
    int n1 = tvam_axis_steps(tau_e, q.dtm0[1], q.ts[1], nin[1], nout[1]);
    int n2 = tvam_axis_steps(tau_e, q.dtm0[2], q.ts[2], nin[2], nout[2]);
    int x = q.sv[0] + q.step[0] * n0 - lo[0];
    int y = q.sv[1] + q.step[1] * n1 - lo[1];
    int z = q.sv[2] + q.step[2] * n2 - lo[2];
    const float ts0 = q.ts[0], ts1 = q.ts[1], ts2 = q.ts[2];
    const float d0 = q.dtm0[0], d1 = q.dtm0[1], d2 = q.dtm0[2];
    float T0 = d0 < TVAM_INF ? fmaf((float)n0, ts0, d0) : TVAM_INF;
    float T1 = d1 < TVAM_INF ? fmaf((float)n1, ts1, d1) : TVAM_INF;
    float T2 = d2 < TVAM_INF ? fmaf((float)n2, ts2, d2) : TVAM_INF;
    const int s0 = q.step[0], s1 = q.step[1], s2 = q.step[2];
    const float stop = tau_x - 1e-6f;
    const float base = k.nsig2 * q.t_start;
    float ea = sc_exp2(fmaf(k.nsig2, tau_e, base)), tp = tau_e;
    for (int guard = 0; guard < 3 * 4096; ++guard) {
        const bool m0 = T0 <= T1 && T0 <= T2;
        const bool m1 = !m0 && T1 <= T2;
        const float tmin = m0 ? T0 : (m1 ? T1 : T2);
        const float tn = tmin < tau_x ? tmin : tau_x;
        // e^{-st t} (1 - e^{-st dt}) without cancellation (tvam_omexp); ea tracks e^{-st t}
        const float c = ea * tvam_omexp(k.sig_t * fmaxf(tn - tp, 0.0f));
        const float eb = ea - c;
        tp = tn;
        f(x, y, z, c);
        if (!(tn < stop)) break;
        if (m0) {
            x += s0;
            ++n0;
            T0 = fmaf((float)n0, ts0, d0);
        } else if (m1) {
            y += s1;
            ++n1;
            T1 = fmaf((float)n1, ts1, d1);
        } else {
            z += s2;
            ++n2;
            T2 = fmaf((float)n2, ts2, d2);
        }
        ea = eb;
    }
}

// The whole segment, brick by brick (the binned forward's visits exactly).
template <typename F>
__device__ __forceinline__ void sc_seg_march(const TvamConsts& k, const SegDda& q, F&& f) {
    const int B[3] = {TVAM_BX, TVAM_BY, TVAM_BZ};
    const int nb[3] = {sc_nbr(k, 0), sc_nbr(k, 1), sc_nbr(k, 2)};
    sc_walk_bricks(k, q, [&](int bid, float, float) {
        const int bx = bid % nb[0], by = (bid / nb[0]) % nb[1], bz = bid / (nb[0] * nb[1]);
        const int lo[3] = {bx * B[0], by * B[1], bz * B[2]};
        const int hi[3] = {min(lo[0] + B[0], k.res[0]), min(lo[1] + B[1], k.res[1]), min(lo[2] + B[2], k.res[2])};
        sc_box_march(k, q, lo, hi, [&](int x, int y, int z, float c) { f(lo[0] + x, lo[1] + y, lo[2] + z, c); });
    });
}

// One medium segment's 3-D DDA (sensor.py:327-438, op for op like the oracle's
// or_dda): MODE FWD adds em * (e^{-st t} - e^{-st (t + dt)}) * inv_vol into the
// dose, ADJ returns sum (...) * grad * inv_vol, COUNT counts visits.
template <int MODE>
__device__ float sc_dda(const TvamConsts& k, float ox, float oy, float oz, float dx, float dy, float dz, float maxt,
                        float em, float* __restrict__ dose, const float* __restrict__ gin, uint64_t& nvis) {
    const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    SegDda q;
    if (!sc_dda_init(k, o, d, maxt, q)) return 0.0f;
    float acc = 0.0f;
    const int64_t sy = k.res[0], sz = (int64_t)k.res[0] * k.res[1];
    sc_seg_march(k, q, [&](int x, int y, int z, float c) {
        const int64_t idx = x + y * sy + z * sz;
        if (MODE == TVAM_MODE_FWD) atomicAdd(&dose[idx], em * c);
        else if (MODE == TVAM_MODE_ADJ) acc = fmaf(c, gin[idx] * k.inv_vol, acc);
        ++nvis;
    });
    return acc;
}

// The brick-bin record of a segment (TvamSegBuf: 3 float4 per slot), written by the record writers
// (tvam_scatter_kernel<EMIT>, tvam_ray3d_emit_kernel) and read back by the bin fill and the brick
// march.  wgt: the record's weight; att: the path attenuation alone (.z, for the cached forward's
// rescale, tvam_bin_reweight_kernel).
__device__ __forceinline__ void sc_pack(const TvamSegBuf& sb, int64_t slot, const SegDda& q, float wgt, float att) {
    sb.r[TVAM_REC_F4 * slot] = make_float4(q.t_start, q.tau_end, q.dtm0[0], q.dtm0[1]);
    sb.r[TVAM_REC_F4 * slot + 1] = make_float4(q.dtm0[2], q.ts[0] * (float)q.step[0], q.ts[1] * (float)q.step[1],
                                               q.ts[2] * (float)q.step[2]);
    sb.r[TVAM_REC_F4 * slot + 2] = make_float4(__int_as_float(q.sv[0] | (q.sv[1] << 11) | (q.sv[2] << 22)), wgt, att, 0.0f);
}

__device__ __forceinline__ void sc_unpack(const float4 a, const float4 b, const float4 cf, SegDda& q, float& w) {
    const int2 c = make_int2(__float_as_int(cf.x), __float_as_int(cf.y));
    q.t_start = a.x;
    q.tau_end = a.y;
    q.dtm0[0] = a.z;
    q.dtm0[1] = a.w;
    q.dtm0[2] = b.x;
    const float tsv[3] = {b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        q.step[i] = tsv[i] < 0.0f ? -1 : 1;
        q.ts[i] = fabsf(tsv[i]);
    }
    q.sv[0] = c.x & 0x7ff;
    q.sv[1] = (c.x >> 11) & 0x7ff;
    q.sv[2] = (c.x >> 22) & 0x3ff;
    w = __int_as_float(c.y);
}

// The largest of a 256-thread workgroup's non-negative values into *dst (float bits, which order
// like the floats): one device atomic per workgroup (one per wave put ~10^6 atomics on a single
// address per chunk)
__device__ __forceinline__ void sc_block_max(float v, uint32_t* dst) {
    __shared__ float s_max[4];
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
        if (v > 0.0f) atomicMax(dst, __float_as_uint(v));
    }
}

}  // namespace

// 'double_cylindrical' vial (geometry.py:222-308; tvam_double.h): two nested glass tubes with the
// printing medium between them.  Every ray is traced in 3-D through the four dielectric tubes and
// deposits along at most two medium segments, in front of the inner vial and behind it, for all
// three projectors.  The pieces are those of tvam_cone.hip: cn_projector_ray for the ray, cn_dda
// for a segment's march, the brick-bin records of tvam_scatter_binned with two slots per path.
//
//   tvam_double_kernel         one thread per (ray, sample): the resumable walk of tvam_double.h,
//                              each segment marched by cn_dda with weight em * att_s as it is
//                              found (one copy of the DDA, never both segments in registers).
//                              Forward: global float atomics; adjoint: a gather summed over both
//                              segments (a plain store per active entry when spp == 1); count.
//   tvam_double_emit_kernel    two brick-bin records per path (record weight em * att_s, .z =
//                              att_s for the cached forward's rescale; a slot without a segment
//                              keeps .z = 0 and m = 0)
//   tvam_double_export_kernel  the rays (tvam_plan_rays: the first segment) and both segments
//                              (tvam_plan_segments)
// and, on the host, the validation of the vial, its constants and tvam_double_segments.
#include "tvam_plan.h"

#include <algorithm>

#include "tvam_cone_ray.h"
#include "tvam_double.h"

namespace {

// The projector ray of flat index ix and the start of its walk.
__device__ __forceinline__ void dv_ray(const TvamConsts& k, const TvamTiles& tp, const int32_t* idxmap,
                                       const TvamPathIndex& ix, ConeRay& r, TvamDoubleWalk& w) {
    cn_projector_ray(k, tp, ix.al, ix.colc, ix.rowc, tvam_stream(k, idxmap, ix.local, tp.spp, ix.smp), r);
    tvam_double_start(w, r.o, r.d);
}

__device__ __forceinline__ bool dv_next(const TvamConsts& k, TvamDoubleWalk& w, ConeRay& r) {
    return tvam_double_next(k.dbl, k.vial_half_h, k.sig_t, k.max_depth, w, r.o2, r.d2, r.maxt, r.att);
}

template <int MODE>
__global__ __launch_bounds__(256) void tvam_double_kernel(TvamConsts k, TvamTiles tp, const float* __restrict__ pat,
                                                          const int32_t* __restrict__ idxmap,
                                                          const float* __restrict__ gin, float* __restrict__ out,
                                                          unsigned long long* __restrict__ counter) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    uint64_t nvis = 0;
    const bool f32 = false;  // (the 64-bit decode alone, as in tvam_cone_kernel)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<MODE>(k, pat, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        TvamDoubleWalk w;
        dv_ray(k, tp, idxmap, ix, r, w);
        float acc = 0.0f;
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            if (!dv_next(k, w, r)) break;
            acc = acc + cn_dda<MODE>(k, r.o2, r.d2, r.maxt, em * r.att, out, gin, nvis) * r.att;
        }
        if (MODE == TVAM_MODE_ADJ) {
            if (spp == 1) out[act] = acc * k.wscale;  // the entry's only ray: no atomic
            else if (acc != 0.0f) atomicAdd(&out[act], acc * k.wscale);
        }
    }
    if (MODE == TVAM_MODE_COUNT) tvam_count_reduce(nvis, counter);
}

// Two brick-bin records per path of [sb.p0, sb.p1) (sb.slots = 2; the layout of
// tvam_scatter_kernel<EMIT>'s records), their brick counts and the chunk's largest |weight|.
__global__ __launch_bounds__(256) void tvam_double_emit_kernel(TvamConsts k, TvamTiles tp,
                                                               const float* __restrict__ pat,
                                                               const int32_t* __restrict__ idxmap, TvamSegBuf sb) {
    float wmax = 0.0f;
    const bool f32 = tvam_path_fits32(sb.p1);
    for (int64_t i = sb.p0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < sb.p1;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot0 = (i - sb.p0) * 2;
        reinterpret_cast<float*>(&sb.r[TVAM_REC_F4 * slot0 + 2])[2] = 0.0f;
        reinterpret_cast<float*>(&sb.r[TVAM_REC_F4 * (slot0 + 1) + 2])[2] = 0.0f;
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_FWD>(k, pat, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        TvamDoubleWalk w;
        dv_ray(k, tp, idxmap, ix, r, w);
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            if (!dv_next(k, w, r)) break;
            SegDda q;
            if (!sc_dda_init(k, r.o2, r.d2, r.maxt, q)) continue;
            const int64_t slot = slot0 + s;
            const float wgt = em * r.att;
            sb.r[TVAM_REC_F4 * slot] = make_float4(q.t_start, q.tau_end, q.dtm0[0], q.dtm0[1]);
            sb.r[TVAM_REC_F4 * slot + 1] = make_float4(q.dtm0[2], q.ts[0] * (float)q.step[0],
                                                       q.ts[1] * (float)q.step[1], q.ts[2] * (float)q.step[2]);
            sb.r[TVAM_REC_F4 * slot + 2] = make_float4(__int_as_float(q.sv[0] | (q.sv[1] << 11) | (q.sv[2] << 22)), wgt,
                                                       r.att, 0.0f);
            sb.m[slot] = (uint32_t)sc_brick_count(k, q);
            wmax = fmaxf(wmax, fabsf(wgt));
        }
    }
    sc_block_max(wmax, sb.wmax);
}

// rays (tvam_plan_rays, may be null): row act * spp + smp = o[3], d[3], hit, o2[3], maxt, d2[3],
// weight, 0 of the first segment; segs (tvam_plan_segments, may be null): [row][2] = o2[3], maxt,
// d2[3], weight, zeros where there is no segment.
__global__ __launch_bounds__(256) void tvam_double_export_kernel(TvamConsts k, TvamTiles tp,
                                                                 const int32_t* __restrict__ idxmap,
                                                                 float* __restrict__ rays, float* __restrict__ segs) {
    const int spp = (int)tp.spp;
    const int64_t n = (int64_t)tp.n_shard * k.crop_y * k.crop_x * spp;
    const bool f32 = tvam_path_fits32(n);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        TvamPathIndex ix = tvam_path_index<false>(k, tp, i, f32);
        float em;
        int64_t act;
        if (!tvam_path_gate<TVAM_MODE_ADJ>(k, nullptr, idxmap, ix.local, k.wscale, k.inv_vol, em, act)) continue;
        tvam_path_pixel(k, f32, ix);
        ConeRay r;
        TvamDoubleWalk w;
        dv_ray(k, tp, idxmap, ix, r, w);
        const int64_t row = act * spp + ix.smp;
        bool more = true;
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            more = more && dv_next(k, w, r);
            if (segs) {
                float4* sg = reinterpret_cast<float4*>(segs + 16 * row + 8 * s);
                sg[0] = more ? make_float4(r.o2[0], r.o2[1], r.o2[2], r.maxt) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                sg[1] = more ? make_float4(r.d2[0], r.d2[1], r.d2[2], k.wscale * r.att)
                             : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            if (rays && s == 0) {
                float4* rw = reinterpret_cast<float4*>(rays + 16 * row);
                rw[0] = make_float4(r.o[0], r.o[1], r.o[2], r.d[0]);
                rw[1] = make_float4(r.d[1], r.d[2], more ? 1.0f : 0.0f, more ? r.o2[0] : 0.0f);
                rw[2] = make_float4(more ? r.o2[1] : 0.0f, more ? r.o2[2] : 0.0f, more ? r.maxt : 0.0f,
                                    more ? r.d2[0] : r.d[0]);
                rw[3] = make_float4(more ? r.d2[1] : r.d[1], more ? r.d2[2] : r.d[2],
                                    more ? k.wscale * r.att : k.wscale, 0.0f);
            }
        }
    }
}

}  // namespace

hipError_t tvam_launch_double_rays(int mode, const TvamConsts& k, const TvamTiles& t, const float* pat,
                                   const int32_t* idxmap, const float* gin, float* out, unsigned long long* counter,
                                   hipStream_t stream) {
    const dim3 g(tvam_grid_1d((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp, 262144)), b(256);
    switch (mode) {
        case TVAM_MODE_FWD:
            tvam_kt_begin(stream, TVAM_KT_CONE);
            hipLaunchKernelGGL(tvam_double_kernel<TVAM_MODE_FWD>, g, b, 0, stream, k, t, pat, idxmap, gin, out, counter);
            tvam_kt_end(stream, TVAM_KT_CONE);
            break;
        case TVAM_MODE_ADJ:
            hipLaunchKernelGGL(tvam_double_kernel<TVAM_MODE_ADJ>, g, b, 0, stream, k, t, pat, idxmap, gin, out, counter);
            break;
        default:
            hipLaunchKernelGGL(tvam_double_kernel<TVAM_MODE_COUNT>, g, b, 0, stream, k, t, pat, idxmap, gin, out,
                               counter);
    }
    return hipGetLastError();
}

void tvam_double_write_records(const TvamConsts& k, const TvamTiles& t, const float* pat, const int32_t* idxmap,
                               const TvamSegBuf& sb, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL(tvam_double_emit_kernel, dim3(grid), dim3(256), 0, stream, k, t, pat, idxmap, sb);
}

hipError_t tvam_launch_double_export(const TvamConsts& k, const TvamTiles& t, const int32_t* idxmap, float* rays,
                                     float* segs, hipStream_t stream) {
    const dim3 g(tvam_grid_1d((int64_t)t.n_shard * k.crop_y * k.crop_x * t.spp, 262144)), b(256);
    hipLaunchKernelGGL(tvam_double_export_kernel, g, b, 0, stream, k, t, idxmap, rays, segs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

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
            float* sg = row + 8 * s;
            sg[0] = o2[0], sg[1] = o2[1], sg[2] = o2[2], sg[3] = maxt;
            sg[4] = d2[0], sg[5] = d2[1], sg[6] = d2[2], sg[7] = att;
        }
    }
    return 0;
}

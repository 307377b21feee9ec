// tvam_path.h -- the one definition of what every per-ray kernel restates of a path (device only):
// the decode of a thread's ray, the pattern / active-set gate, the sampler prefix, the collimated
// projector's first medium segment, the events of the path loops of tvam_scatter.hip and the
// visit-count epilogue.  The draws are those of oracle/tvam_oracle.c and of the reference
// (common.py:92-108, volume.py:179-272), number for number and in their order: a change to a draw
// is made here and nowhere else.
#pragma once
#include "tvam_internal.h"

namespace {

// A thread's ray: dense shard entry `local` = ([shard angle al][crop row rowc][crop column colc]),
// sample smp.
struct TvamPathIndex {
    int64_t local;
    int smp, al, rowc, colc;
};

// Dense shard entry -> (shard angle, crop row, crop column).  fits32: the entry count fits in 32
// bits (32-bit index arithmetic: a 64-bit division is ~3x the code).
__device__ __forceinline__ void tvam_path_pixel(const TvamConsts& k, int64_t local, bool fits32, int& al, int& rowc,
                                                int& colc) {
    const int64_t per_angle = (int64_t)k.crop_y * k.crop_x;
    if (fits32) {
        const uint32_t l32 = (uint32_t)local, pa = (uint32_t)per_angle, cx = (uint32_t)k.crop_x;
        const uint32_t a32 = l32 / pa, p32 = l32 - a32 * pa, r32 = p32 / cx;
        al = (int)a32;
        rowc = (int)r32;
        colc = (int)(p32 - r32 * cx);
    } else {
        al = (int)(local / per_angle);
        const int64_t pix = local - (int64_t)al * per_angle;
        rowc = (int)(pix / k.crop_x);
        colc = (int)(pix - (int64_t)rowc * k.crop_x);
    }
}

// Whether a launch over n rays may decode them in 32 bits.
__device__ __forceinline__ bool tvam_path_fits32(int64_t n) { return n <= (int64_t)0xffffffff; }

// Flat ray index of a launch over the shard's n_local * spp rays -> its entry and sample.  Pixel-major:
// i = local * spp + smp.  Sample-major: i = smp * n_local + local, the ray records' order (the
// tile kernels' lanes, which enumerate the sample slowest, read consecutive records of
// neighbouring pixels).  fits32: tvam_path_fits32 of the launch's ray count, or false in a kernel
// whose registers the second decode would push over an occupancy step.
template <bool SAMPLE_MAJOR>
__device__ __forceinline__ TvamPathIndex tvam_path_index(const TvamConsts& k, const TvamTiles& tp, int64_t i,
                                                         bool fits32) {
    const int64_t n_local = (int64_t)tp.n_shard * k.crop_y * k.crop_x;
    TvamPathIndex ix;
    if (fits32) {
        const uint32_t ii = (uint32_t)i, d = SAMPLE_MAJOR ? (uint32_t)n_local : tp.spp;
        const uint32_t q = ii / d, r = ii - q * d;
        ix.local = (int64_t)(SAMPLE_MAJOR ? r : q);
        ix.smp = (int)(SAMPLE_MAJOR ? q : r);
    } else {
        const int64_t d = SAMPLE_MAJOR ? n_local : (int64_t)(int)tp.spp;
        const int64_t q = i / d, r = i - q * d;
        ix.local = SAMPLE_MAJOR ? r : q;
        ix.smp = (int)(SAMPLE_MAJOR ? q : r);
    }
    return ix;
}

// The pixel of ix.local (tvam_path_pixel), decoded after the gate: the coordinates are not live
// across its loads, and dropped entries skip the divisions.
__device__ __forceinline__ void tvam_path_pixel(const TvamConsts& k, bool fits32, TvamPathIndex& ix) {
    tvam_path_pixel(k, ix.local, fits32, ix.al, ix.rowc, ix.colc);
}

// Pattern / active-set gate of dense entry `local`; false: the entry casts no ray.  FWD: em = the
// entry's pattern value * wscale * inv_vol (zero entries dropped under skip_zero; a caller adding
// into an unscaled film passes inv_vol = 1).  Else em = 1 and act = the entry's position in the
// sparse active set (idxmap; entries outside it dropped), or `local` for a dense set.
template <int MODE>
__device__ __forceinline__ bool tvam_path_gate(const TvamConsts& k, const float* __restrict__ pat,
                                               const int32_t* __restrict__ idxmap, int64_t local, float wscale,
                                               float inv_vol, float& em, int64_t& act) {
    em = 1.0f;
    act = local;
    if (MODE == TVAM_MODE_FWD) {
        const float p = pat[local];
        if (p == 0.0f && k.skip_zero) return false;
        em = p * wscale * inv_vol;
    } else if (idxmap) {
        act = idxmap[local];
        if (act < 0) return false;
    }
    return true;
}

// The sampler prefix of a ray (common.py:92-108): position next_2d if jittered, time next_1d under
// sample_time, aperture next_2d; (c, sn) = the rotation the ray is cast under.
struct TvamPathDraws {
    float jx, jy, c, sn, u1, u2;
};

// Seeds rng with `stream` (tvam_stream) and draws the prefix; rng is left after the aperture pair.
// MORE: the caller goes on drawing from rng.  Without it the generator is seeded only for a
// jittered position, and the aperture pair is not drawn (u1 = u2 = 0).
// TIME: sample_time is honoured (common.py:101-104: time = (angle + u) / n_patterns); without it
// the rotation is the shard angle's own.
template <bool MORE, bool TIME>
__device__ __forceinline__ TvamPathDraws tvam_path_draws(const TvamConsts& k, const TvamTiles& tp, int al,
                                                         uint64_t stream, TvamPcg& rng) {
    TvamPathDraws d;
    d.jx = d.jy = 0.5f;
    d.u1 = d.u2 = 0.0f;
    if (MORE || !k.regular) {
        rng.seed(tp.seed, stream);
        if (!k.regular) {
            d.jx = rng.next_float();
            d.jy = rng.next_float();
        }
    }
    if (TIME && k.sample_time) {
        float time = (float)(k.a0 + al);
        time = time + rng.next_float();
        time = time / (float)k.n_patterns;
        float alpha = TVAM_TWO_PI * time;
        if (k.clockwise) alpha = -alpha;
        d.c = cosf(alpha);
        d.sn = sinf(alpha);
    } else {
        const float2 csv = tp.cs[al];
        d.c = csv.x;
        d.sn = csv.y;
    }
    if (MORE) {  // aperture sample (projector.py:160)
        d.u1 = rng.next_float();
        d.u2 = rng.next_float();
    }
    return d;
}

// The collimated projector's ray through crop pixel (colc, rowc) under the draws d.
__device__ __forceinline__ void tvam_path_ray(const TvamConsts& k, int colc, int rowc, const TvamPathDraws& d,
                                              float& ox, float& oy, float& oz, float& dx, float& dy) {
    float xc, yc;
    tvam_ray_camera(k, k.crop_off_x + colc, k.crop_off_y + rowc, d.jx, d.jy, xc, yc);
    tvam_ray_world(k, d.c, d.sn, xc, yc, ox, oy, oz, dx, dy);
}

// A path's first medium segment (o2, d2, [0, maxt]) in the plane z = oz, and the weight wgt its
// interfaces leave it.
struct TvamPathSeg {
    float oz, o2x, o2y, d2x, d2y, maxt, wgt;
};

// tvam_path_ray, then the vial (tvam_segment).  false: the ray never reaches the medium.
__device__ __forceinline__ bool tvam_path_first_segment(const TvamConsts& k, const TvamPathIndex& ix,
                                                        const TvamPathDraws& d, TvamPathSeg& s) {
    float ox, oy, dx, dy;
    tvam_path_ray(k, ix.colc, ix.rowc, d, ox, oy, s.oz, dx, dy);
    return tvam_segment(k, ox, oy, s.oz, dx, dy, s.o2x, s.o2y, s.d2x, s.d2y, s.maxt, s.wgt);
}

// ---------------------------------------------------------------------------
// Events of the path loops (tvam_scatter.hip; oracle or_trace_scatter, or_trace_surface_scatter,
// or_trace_estimator).
// ---------------------------------------------------------------------------

// Surfaces before the medium (glass vials: two): the depth a path enters the medium with.
__device__ __forceinline__ int sc_nsurf(const TvamConsts& k) { return k.vial_type == 0 ? 1 : 2; }

// Skips the draws of the surface iterations before the medium: RR, the medium's (scattering
// media), BSDF next_1d + next_2d.
__device__ __forceinline__ void sc_skip_surface_draws(TvamPcg& rng, int nsurf, bool has_sc) {
    for (int q = 0; q < (has_sc ? 5 : 4) * nsurf; ++q) (void)rng.next_float();
}

// Russian roulette (volume.py:182-185); false: the path ends (killed, or its attenuation is 0).
__device__ __forceinline__ bool sc_roulette(const TvamConsts& k, TvamPcg& rng, int depth, float& att) {
    const float q = fminf(0.99f, att);
    const float u_rr = rng.next_float();
    if (depth > k.rr_depth) {
        if (!(u_rr < q)) return false;
        att = att * (1.0f / q);
    }
    return att != 0.0f;
}

// Mitsuba coordinate_system() (Duff et al. 2017) and the phase functions'
// sample(): isotropic (square_to_uniform_sphere, world space), rayleigh (cbrt
// inversion of the (3/8)(1 + mu^2) CDF), hg (-cos_theta in the frame of wi).
__device__ __forceinline__ void sc_phase(const TvamConsts& k, float dx, float dy, float dz, float u1, float u2,
                                         float& wx, float& wy, float& wz) {
    float lx, ly, lz;
    if (k.phase_type == TVAM_PHASE_ISOTROPIC) {  // square_to_uniform_sphere(u): z = 1 - 2 u.y, phi = 2 pi u.x
        const float z = 1.0f - 2.0f * u2;
        const float r = sqrtf(fmaxf(1.0f - z * z, 0.0f));
        const float sp = sinf(TVAM_TWO_PI * u1), cp = cosf(TVAM_TWO_PI * u1);
        wx = r * cp;
        wy = r * sp;
        wz = z;
        return;
    }
    if (k.phase_type == TVAM_PHASE_RAYLEIGH) {
        const float z = 2.0f * (2.0f * u1 - 1.0f);
        const float tmp = sqrtf(z * z + 1.0f);
        const float ct = cbrtf(z + tmp) + cbrtf(z - tmp);
        const float st = sqrtf(fmaxf(1.0f - ct * ct, 0.0f));
        const float sp = sinf(TVAM_TWO_PI * u2), cp = cosf(TVAM_TWO_PI * u2);
        lx = st * cp;
        ly = st * sp;
        lz = ct;
    } else {
        const float g = k.phase_g;
        float ct;
        if (fabsf(g) < 5.9604644775390625e-08f) {
            ct = 1.0f - 2.0f * u1;
        } else {
            const float sq = (1.0f - g * g) / (1.0f - g + 2.0f * g * u1);
            ct = (1.0f + g * g - sq * sq) / (2.0f * g);
        }
        const float st = sqrtf(fmaxf(1.0f - ct * ct, 0.0f));
        const float sp = sinf(TVAM_TWO_PI * u2), cp = cosf(TVAM_TWO_PI * u2);
        lx = st * cp;
        ly = st * sp;
        lz = -ct;
    }
    const float nx = -dx, ny = -dy, nz = -dz;  // Frame3f(wi = -d)
    const float sg = copysignf(1.0f, nz);
    const float a = -1.0f / (sg + nz);
    const float b = nx * ny * a;
    const float sx = sg * (nx * nx * a) + 1.0f, sy = sg * b, sz = -sg * nx;
    const float tx = b, ty = fmaf(ny, ny * a, sg), tz = -ny;
    wx = sx * lx + tx * ly + nx * lz;
    wy = sy * lx + ty * ly + ny * lz;
    wz = sz * lx + tz * ly + nz * lz;
}

// A medium event at free-flight distance tmi: weight tr / pdf * sigma_s, the phase function's
// next_1d + next_2d, the path moved to the event and turned into the sampled direction.
// false: the path has reached max_depth.
__device__ __forceinline__ bool sc_medium_event(const TvamConsts& k, TvamPcg& rng, float tmi, float& px, float& py,
                                                float& pz, float& vx, float& vy, float& vz, float& att, int& depth) {
    const float tr = expf(-tmi * k.sig_t);
    const float pdf = tr * k.sig_t;
    const float inv = pdf > 0.0f ? 1.0f / pdf : 0.0f;
    float w = tr * inv;
    w = w * k.sig_s;
    (void)rng.next_float();  // phase next_1d
    const float u1 = rng.next_float(), u2 = rng.next_float();
    float wx, wy, wz;
    sc_phase(k, vx, vy, vz, u1, u2, wx, wy, wz);
    px = fmaf(vx, tmi, px);
    py = fmaf(vy, tmi, py);
    pz = fmaf(vz, tmi, pz);
    vx = wx;
    vy = wy;
    vz = wz;
    att = att * w;
    ++depth;
    return depth < k.max_depth;
}

// The 'ratio' sensor along a segment [0, tsi) (sensor.py:193-295): deposits at t stepping by
// -log(1 - u) / majorant (draws inside accumulate), weight att (1 - st / mu)^k st / mu.
// deposit(t, weight).
template <typename F>
__device__ __forceinline__ void sc_ratio_track(const TvamConsts& k, TvamPcg& rng, float tsi, float att, F&& deposit) {
    const float mj = k.majorant;
    const float ratio = k.sig_t / mj, keep = 1.0f - ratio;
    float t = 0.0f, pk = 1.0f;
    for (int it = 0; it < (1 << 20); ++it) {
        t = t + (-logf(1.0f - rng.next_float()) / mj);
        if (!(t < tsi)) break;
        deposit(t, att * pk * ratio);
        pk = pk * keep;
    }
}

// The voxel of a point deposit of the ratio / delta sensors (sensor.py:143-151, :248-260):
// floor((p - bbox.min) / h) as x + y res.x + z res.x res.y, or -1 outside the grid (skipped).
__device__ __forceinline__ int64_t sc_point_voxel(const TvamConsts& k, float px, float py, float pz) {
    const int vx = (int)floorf((px - k.bmin[0]) / k.h[0]);
    const int vy = (int)floorf((py - k.bmin[1]) / k.h[1]);
    const int vz = (int)floorf((pz - k.bmin[2]) / k.h[2]);
    if (vx < 0 || vy < 0 || vz < 0 || vx >= k.res[0] || vy >= k.res[1] || vz >= k.res[2]) return -1;
    return vx + (int64_t)vy * k.res[0] + (int64_t)vz * k.res[0] * k.res[1];
}

// COUNT epilogue: a wave's visits summed into its first lane, one atomic per wave.
__device__ __forceinline__ void tvam_count_reduce(unsigned long long nvis, unsigned long long* counter) {
    for (int off = 32; off > 0; off >>= 1) nvis += __shfl_down(nvis, off, 64);
    if ((threadIdx.x & 63) == 0 && nvis) atomicAdd(counter, nvis);
}

}  // namespace

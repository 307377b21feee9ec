"""Float64 NumPy model of the projector derivatives (test helper, no GPU):
d dose / d theta for theta in distance, focus_distance, aperture_radius, pixel_size of a telecentric /
lens projector behind the index-matched vial.

The rays are projector_model's (its sampler, disk warp, to_world and medium segment), generated here
from float64 parameter values `vals` so that a finite difference in theta is not rounded through the
descriptor's float32 fields.  The tangents are the analytic pathwise ones: camera-space tangent of
the origin and of the unnormalised direction, normalisation, to_world at the ray's own angle, the
implicit derivatives of the tube entry / exit times, the spawn offset, and per voxel visit the
derivative of the two face-crossing times that bound it.  The DDA is analytic: the times at which the
segment crosses the box and every interior voxel face, sorted; a visit lies between two consecutive
times and its voxel is that of the midpoint.

trace() returns per ray the visit sequence (film indices), the deposits e^{-s t_a} - e^{-s t_b}, their
tangents s (e^{-s t_b} t_b' - e^{-s t_a} t_a'), and a margin: the least gap between two consecutive
event times of the DDA (box entry, face crossings, end) in units of the voxel size, joined with
projector_model's tube margin.  A ray whose margin is below MARGIN may visit other voxels in fp32."""
import numpy as np

import projector_model as pm

MARGIN = 1e-4
PARAMS = ("distance", "focus_distance", "aperture_radius", "pixel_size")  # index = TVAM_DPROJ_*


def base_vals(desc):
    """The descriptor's own (float32) parameter values, as float64."""
    f = lambda v: float(np.float32(v))
    return dict(distance=f(desc.distance), focus_distance=f(desc.focus_distance),
                aperture_radius=f(desc.aperture_radius), pixel_size_x=f(desc.pixel_size_x),
                pixel_size_y=f(desc.pixel_size_y))


def moved(vals, param, delta):
    """vals with parameter `param` moved by delta ('pixel_size' moves both pixel sizes together)."""
    v = dict(vals)
    if param == "pixel_size":
        v["pixel_size_x"] += delta
        v["pixel_size_y"] += delta
    else:
        v[param] += delta
    return v


def theta_of(vals, param):
    return vals["pixel_size_x"] if param == "pixel_size" else vals[param]


def _dot(a, b):
    return np.sum(a * b, -1)


def _rays(desc, pixels, streams, spp, seed, vals, param):
    """World rays and segments (projector_model.model_rays with float64 parameters) and, for `param`,
    the tangents of o2, d and maxt."""
    pixels = np.repeat(np.asarray(pixels, dtype=np.int64), spp)
    st = np.repeat(np.asarray(streams, dtype=np.uint64), spp) * np.uint64(spp) + \
        np.tile(np.arange(spp, dtype=np.uint64), len(streams))
    hw = desc.res_x * desc.res_y
    angle, pix = pixels // hw, pixels % hw
    row, col = pix // desc.res_x, pix % desc.res_x
    smp = pm.Sampler(seed, st)
    jx = jy = np.full(pixels.shape, 0.5)
    if not desc.regular_sampling:
        jx, jy = smp.next_float(), smp.next_float()
    ut = smp.next_float() if desc.sample_time else None
    u1, u2 = smp.next_float(), smp.next_float()
    alpha = pm.angle_alpha(desc, angle, ut)
    px, py = vals["pixel_size_x"], vals["pixel_size_y"]
    D, F, R = vals["distance"], vals["focus_distance"], vals["aperture_radius"]
    W, H = desc.res_x, desc.res_y
    xc, yc = (0.5 - (col + jx) / W) * W * px, (0.5 - (row + jy) / H) * H * py
    ux, uy = pm.square_to_uniform_disk_concentric(u1, u2)
    ax, ay = R * ux, R * uy
    z = np.zeros_like(xc)
    tele = desc.projector_type == 1
    assert desc.projector_type in (1, 2)
    if tele:
        oc = np.stack([xc + ax, yc + ay, z], -1)
        v = np.stack([-ax, -ay, z + (pm.ZC + F)], -1)
    else:
        oc = np.stack([ax, ay, z], -1)
        v = np.stack([xc - ax, yc - ay, z + F], -1)
    nv = np.linalg.norm(v, axis=-1, keepdims=True)
    dc = v / nv
    c, s = np.cos(alpha), np.sin(alpha)

    def world(o_c, d_c, Dv):
        ow = np.stack([c * (Dv - o_c[..., 2]) + s * o_c[..., 0], s * (Dv - o_c[..., 2]) - c * o_c[..., 0], o_c[..., 1]], -1)
        dw = np.stack([-c * d_c[..., 2] + s * d_c[..., 0], -s * d_c[..., 2] - c * d_c[..., 0], d_c[..., 1]], -1)
        return ow, dw

    o, d = world(oc, dc, D)
    r, half = float(np.float32(desc.vial_r)), 0.5 * float(np.float32(desc.vial_height))
    n = o.shape[0]
    t0, m0 = pm._tube_hit(o, d, r, half)
    hit = np.isfinite(t0)
    t0 = np.where(hit, t0, 0.0)
    p = o + d * t0[:, None]
    rp = np.hypot(p[:, 0], p[:, 1])
    nrm = np.stack([p[:, 0] / rp, p[:, 1] / rp, np.zeros(n)], -1)
    ndd = _dot(nrm, d)
    hit &= ndd < 0.0
    amax = np.argmax(np.abs(p), -1)
    mag = (1.0 + np.abs(p)[np.arange(n), amax]) * pm.RAY_EPS
    o2 = p - mag[:, None] * nrm
    t1, m1 = pm._tube_hit(o2, d, r, half)
    margin = np.where(hit, np.minimum(m0, m1), m0)
    hit &= np.isfinite(t1)
    maxt = np.where(hit, t1, 0.0)
    out = dict(o=o, d=d, hit=hit, o2=o2, maxt=maxt, tube_margin=margin)
    if param is None:
        return out
    # camera-space tangents of the origin, the unnormalised direction and the distance
    ocp, vp, Dp = np.zeros_like(oc), np.zeros_like(v), 0.0
    if param == "distance":
        Dp = 1.0
    elif param == "focus_distance":
        vp[:, 2] = 1.0
    elif param == "aperture_radius":
        ocp[:, 0], ocp[:, 1] = ux, uy
        vp[:, 0], vp[:, 1] = -ux, -uy
    else:
        assert param == "pixel_size"
        tgt = ocp if tele else vp
        tgt[:, 0], tgt[:, 1] = xc / px, yc / py
    dcp = (vp - dc * _dot(dc, vp)[:, None]) / nv
    # to_world is linear in (origin, D) and in the direction; the derivative of a point at Z = 0
    op, dp = world(ocp, dcp, Dp)
    with np.errstate(invalid="ignore", divide="ignore"):
        t0p = -_dot(nrm, op + t0[:, None] * dp) / ndd
        pp = op + t0p[:, None] * d + t0[:, None] * dp
        mp = np.sign(p[np.arange(n), amax]) * pp[np.arange(n), amax]
        npx = (pp - nrm * _dot(nrm, pp)[:, None]) / rp[:, None]
        npx[:, 2] = 0.0
        o2p = pp - pm.RAY_EPS * mp[:, None] * nrm - mag[:, None] * npx
        q = o2 + maxt[:, None] * d
        q[:, 2] = 0.0
        maxtp = -_dot(q, o2p + maxt[:, None] * dp) / _dot(q, d)
    out.update(o2p=o2p, dp=dp, maxtp=maxtp)
    return out


def trace(desc, pixels, streams, spp, seed, vals=None, param=None):
    """Per ray (row i * spp + k of active entry i): hit, vox [n, K] film indices (-1 past the ray's
    visits), ev [n, K + 1] the axis of the face at each event time (3: the segment's own start or end;
    -1 past the ray's events), dep [n, K], tan [n, K] (param given; the geometric part, without the ray
    weight's share), margin [n]."""
    vals = base_vals(desc) if vals is None else vals
    R = _rays(desc, pixels, streams, spp, seed, vals, param)
    o2, d, maxt, hit = R["o2"], R["d"], R["maxt"], R["hit"]
    n = o2.shape[0]
    bmin = np.array([float(np.float32(v)) for v in desc.bbox_min])
    bmax = np.array([float(np.float32(v)) for v in desc.bbox_max])
    res = np.array([int(v) for v in desc.film_res])
    h = (bmax - bmin) / res
    sig = float(np.float32(desc.sigma_t))
    have = param is not None
    with np.errstate(invalid="ignore", divide="ignore"):
        tb0, tb1 = (bmin - o2) / d, (bmax - o2) / d
        lo, hi = np.minimum(tb0, tb1), np.maximum(tb0, tb1)
        a_in, a_out = np.argmax(lo, -1), np.argmin(hi, -1)
        rows = np.arange(n)
        t_in, t_out = lo[rows, a_in], hi[rows, a_out]
        t_start, t_end = np.maximum(t_in, 0.0), np.minimum(t_out, maxt)
        ok = hit & np.isfinite(t_start) & np.isfinite(t_end) & (t_start < t_end)

        def face_tan(t, axis):  # t' = -(o2'_a + t d'_a) / d_a
            return -(R["o2p"][rows, axis] + t * R["dp"][rows, axis]) / d[rows, axis]

        times = [np.where(ok, t_start, np.inf)[:, None]]
        axes = [np.where(t_in > 0.0, a_in, 3)[:, None]]  # 3: the segment's own start or end
        tans = []
        if have:
            tans.append(np.where(t_in > 0.0, face_tan(t_start, a_in), 0.0)[:, None])
        for a in range(3):
            planes = bmin[a] + h[a] * np.arange(1, res[a])
            t = (planes[None, :] - o2[:, a:a + 1]) / d[:, a:a + 1]
            good = ok[:, None] & np.isfinite(t) & (t > t_start[:, None]) & (t < t_end[:, None])
            times.append(np.where(good, t, np.inf))
            axes.append(np.full(t.shape, a))
            if have:
                tans.append(np.where(good, -(R["o2p"][:, a:a + 1] + t * R["dp"][:, a:a + 1]) / d[:, a:a + 1], 0.0))
        times.append(np.where(ok, t_end, np.inf)[:, None])
        axes.append(np.where(maxt <= t_out, 3, a_out)[:, None])
        if have:
            tans.append(np.where(maxt <= t_out, R["maxtp"], face_tan(t_end, a_out))[:, None])
    T = np.concatenate(times, 1)
    order = np.argsort(T, 1, kind="stable")
    T = np.take_along_axis(T, order, 1)
    cnt = np.isfinite(T).sum(1)          # events of the ray: visits + 1
    K = max(int(cnt.max()) - 1, 1)
    ta, tb = T[:, :K], T[:, 1:K + 1]
    live = np.isfinite(tb)
    ta, tb = np.where(live, ta, 0.0), np.where(live, tb, 0.0)
    mid = 0.5 * (ta + tb)
    vox = np.zeros((n, K), dtype=np.int64)
    stride = 1
    for a in range(3):
        ia = np.floor((o2[:, a:a + 1] + mid * d[:, a:a + 1] - bmin[a]) / h[a]).astype(np.int64)
        vox += np.clip(ia, 0, res[a] - 1) * stride
        stride *= res[a]
    vox = np.where(live, vox, -1)
    ea, eb = np.exp(-sig * ta), np.exp(-sig * tb)
    dep = np.where(live, ea - eb, 0.0)
    gaps = np.where(live, tb - ta, np.inf).min(1) / h.min()
    with np.errstate(invalid="ignore"):
        miss = np.where(hit & np.isfinite(t_start) & np.isfinite(t_end), np.abs(t_end - t_start) / h.min(), np.inf)
    margin = np.minimum(R["tube_margin"], np.where(ok, gaps, miss))
    ev = np.where(np.isfinite(T), np.take_along_axis(np.concatenate(axes, 1), order, 1), -1)[:, :K + 1]
    out = dict(hit=hit, ok=ok, vox=vox, ev=ev, dep=dep, margin=margin, n_visits=np.where(ok, cnt - 1, 0))
    if have:
        Tp = np.take_along_axis(np.concatenate(tans, 1), order, 1)
        out["tan"] = np.where(live, sig * (eb * Tp[:, 1:K + 1] - ea * Tp[:, :K]), 0.0)
    return out


def weight_rel(vals, param):
    """w' / w of the ray weight ~ p_x p_y."""
    return 1.0 / vals["pixel_size_x"] + 1.0 / vals["pixel_size_y"] if param == "pixel_size" else 0.0


def ray_em(desc, pat, spp, n_total, vals=None):
    """Per ray: pattern value * ray weight * sigma_a / sigma_t * inv_vol, float64 from the float32
    inputs (pat: one value per active entry)."""
    vals = base_vals(desc) if vals is None else vals
    w = vals["pixel_size_x"] * vals["pixel_size_y"] / spp * float(np.float32(desc.print_time))
    sa_st = 1.0 - float(np.float32(desc.albedo))
    bmin = np.array([float(np.float32(v)) for v in desc.bbox_min])
    bmax = np.array([float(np.float32(v)) for v in desc.bbox_max])
    vol = np.prod((bmax - bmin) / np.array([int(v) for v in desc.film_res]))
    del n_total  # (area / n_samples = p_x p_y n / (n spp): the count cancels)
    return np.repeat(np.asarray(pat, np.float64), spp) * (w * sa_st / vol)


def film_shape(desc):
    rx, ry, rz = desc.film_res
    return (rz, ry, rx)


def scatter(desc, tr, per_visit):
    """The film of per-visit values [n, K] (already weighted per ray)."""
    out = np.zeros(int(np.prod(film_shape(desc))))
    live = tr["vox"] >= 0
    np.add.at(out, tr["vox"][live], per_visit[live])
    return out.reshape(film_shape(desc))


def dose_film(desc, tr, em):
    return scatter(desc, tr, em[:, None] * tr["dep"])


def tangent_film(desc, tr, em, vals, param):
    """T_theta = sum over rays em (tangent + (w' / w) deposit)."""
    return scatter(desc, tr, em[:, None] * (tr["tan"] + weight_rel(vals, param) * tr["dep"]))


def fov_chain(desc, vals):
    """A lens configured by fov: (p / F, d p / d fov in degrees) with p = 2 F tan(fov / 2) / res_x."""
    F, p = vals["focus_distance"], vals["pixel_size_x"]
    half = np.arctan(p * desc.res_x / 2.0 / F)
    return p / F, (np.pi / 180.0) * F / np.cos(half) ** 2 / desc.res_x


def same_sequence(trs):
    """Rays whose discrete decisions agree in every trace of `trs`: the voxels visited and the face
    that ends each visit (the box face a ray enters or leaves through included)."""
    K = max(t["vox"].shape[1] for t in trs)
    pad = lambda a, k: np.pad(a, ((0, 0), (0, k - a.shape[1])), constant_values=-1)
    same = np.ones(trs[0]["vox"].shape[0], bool)
    for t in trs[1:]:
        same &= (pad(t["vox"], K) == pad(trs[0]["vox"], K)).all(1) & (pad(t["ev"], K + 1) == pad(trs[0]["ev"], K + 1)).all(1)
    return same


def padded(a, K):
    """[n, k] per-visit values as [n, K], zero filled."""
    return np.pad(a, ((0, 0), (0, K - a.shape[1])))


def keep_pixels(tr, spp):
    """Active entries all of whose rays have margin > MARGIN."""
    return (tr["margin"] > MARGIN).reshape(-1, spp).all(1)


# --------------------------------------------------------------------------- scenes and the calibration fit
def projector_config(kind="telecentric", lens_fov=False):
    """The config of projector_model.projector_scene(kind, lens_fov=lens_fov), for the tests that need
    the scene itself (traverse / update) rather than its descriptor."""
    F = 20.0
    proj = {"type": kind, "n_patterns": 6, "resx": 24, "resy": 20, "motion": "circular", "distance": F,
            "aperture_radius": 2.0, "focus_distance": F}
    if kind == "lens" and lens_fov:
        proj["fov"] = float(np.rad2deg(2 * np.arctan(0.15 * 24 / 2 / F)))
    else:
        proj["pixel_size"] = 0.15
    return {
        "vial": {"type": "index_matched", "r": 2.9, "height": 40.0,
                 "medium": {"ior": 1.0, "extinction": 1.0, "albedo": 0.0}},
        "projector": proj,
        "sensor": {"type": "dda", "scalex": 4.0, "scaley": 3.6, "scalez": 2.0,
                   "film": {"type": "vfilm", "resx": 36, "resy": 40, "resz": 20}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.9, "tu": 0.95},
        "regular_sampling": False,
    }


FIT_SPP = 64
FIT_PARAMS = ("aperture_radius", "focus_distance", "distance")


def fit_pixels(desc):
    """The calibration pattern: 8 lit pixels of angle 0 (flat full-DMD indices), two columns of four
    rows around the DMD's centre."""
    return np.array([r * desc.res_x + c for r in (7, 9, 11, 13) for c in (9, 14)], dtype=np.int64)


def fit_model(desc, name, start, steps, by_fov=False, seed=0):
    """One-parameter Gauss-Newton theta <- theta - <D - D*, T> / <T, T> on the float64 model, D* the
    model's dose at the descriptor's own parameters: theta after each step.  by_fov: a lens configured
    by fov, whose pixel size follows focus_distance (p = 2 F tan(fov / 2) / res_x)."""
    pix = fit_pixels(desc)
    st = np.arange(pix.size)
    pat = np.ones(pix.size, np.float32)
    v0 = base_vals(desc)

    def vals_at(theta):
        v = dict(v0)
        v[name] = theta
        if by_fov and name == "focus_distance":
            v["pixel_size_x"] = v0["pixel_size_x"] * theta / v0["focus_distance"]
            v["pixel_size_y"] = v0["pixel_size_y"] * theta / v0["focus_distance"]
        return v

    def dose_and_tangent(theta, want_T=True):
        v = vals_at(theta)
        em = ray_em(desc, pat, FIT_SPP, pix.size, v)
        tr = trace(desc, pix, st, FIT_SPP, seed, v, name if want_T else None)
        D = dose_film(desc, tr, em)
        if not want_T:
            return D, None
        T = tangent_film(desc, tr, em, v, name)
        if by_fov and name == "focus_distance":
            trp = trace(desc, pix, st, FIT_SPP, seed, v, "pixel_size")
            T = T + v["pixel_size_x"] / theta * tangent_film(desc, trp, em, v, "pixel_size")
        return D, T

    target, _ = dose_and_tangent(v0[name], False)
    theta, out = float(start), []
    for _ in range(steps):
        D, T = dose_and_tangent(theta)
        theta = theta - float(np.vdot(D - target, T) / np.vdot(T, T))
        out.append(theta)
    return out

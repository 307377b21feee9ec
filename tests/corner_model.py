"""Float64 NumPy model of the 'filter_corner' pass (test helper, no GPU; filter_corner.py:17-66,
optimize.py:166-185), next to projector_model.py, whose rays it takes: the first surface a
projector ray meets -- the container's outer surface (index_matched: open tube r, cylindrical: open
tube r_ext, both |z| <= height / 2 and hit from either side; square: the closed cuboid w_ext x
w_ext x height) or an occluder triangle -- and the decision

    dropped  iff  no hit  or  sqrt((|p.x| - dist)^2 + (|p.y| - dist)^2) < radius.

The fp32 code is compared with it under one rule.  With

    delta = 64 * 2^-24 * (distance + sqrt(2) * outer half-width)

(an absolute length: a few dozen fp32 roundings on coordinates of that magnitude) a pixel is
*undecided* when its verdict (hit / miss, corner / not) changes if the ray is displaced by +-delta
along either transverse direction, or `radius` or the height changes by +-delta.  (The lateral
displacement also covers near-tangent rays on a tube, whose hit point is ill-conditioned.)  On
every other pixel the fp32 verdict must equal the model's exactly, and the hit point must lie
within delta + max over those variations of |p(varied) - p|."""
import copy

import numpy as np

import projector_model as pm


def surface(desc, dheight=0.0):
    """(kind, half-width or radius, half height) of the container's outer surface."""
    half = 0.5 * (float(np.float32(desc.vial_height)) + dheight)
    if desc.vial_type == 2:
        return "box", float(np.float32(desc.vial_r_ext)), half
    r = float(np.float32(desc.vial_r_ext)) if desc.vial_type == 1 else float(np.float32(desc.vial_r))
    return "tube", r, half


def delta(desc):
    _, w, _ = surface(desc)
    return 64.0 * 2.0 ** -24 * (float(np.float32(desc.distance)) + np.sqrt(2.0) * w)


def _tube(o, d, r, half):
    """Nearest t >= 0 on the open tube, from either side (inf: none)."""
    A = d[:, 0] ** 2 + d[:, 1] ** 2
    B = 2.0 * (d[:, 0] * o[:, 0] + d[:, 1] * o[:, 1])
    C = o[:, 0] ** 2 + o[:, 1] ** 2 - r * r
    disc = B * B - 4.0 * A * C
    ok = (disc >= 0.0) & (A > 0.0)
    sq = np.sqrt(np.where(ok, disc, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        t0 = (-B - sq) / (2.0 * A)
        t1 = (-B + sq) / (2.0 * A)
        z0, z1 = o[:, 2] + d[:, 2] * t0, o[:, 2] + d[:, 2] * t1
    near = ok & (t0 >= 0.0) & (np.abs(z0) <= half)
    far = ok & ~near & (t1 >= 0.0) & (np.abs(z1) <= half)
    return np.where(near, t0, np.where(far, t1, np.inf))


def _box(o, d, h):
    """Nearest t >= 0 on the closed cuboid [-h, h] (slab method; inf: none)."""
    tn = np.full(o.shape[0], -np.inf)
    tf = np.full(o.shape[0], np.inf)
    ok = np.ones(o.shape[0], dtype=bool)
    for a in range(3):
        par = d[:, a] == 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            ta = (-h[a] - o[:, a]) / d[:, a]
            tb = (h[a] - o[:, a]) / d[:, a]
        lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
        ok &= ~par | (np.abs(o[:, a]) <= h[a])
        tn = np.where(par, tn, np.maximum(tn, lo))
        tf = np.where(par, tf, np.minimum(tf, hi))
    ok &= tn <= tf
    return np.where(ok & (tn >= 0.0), tn, np.where(ok & (tf >= 0.0), tf, np.inf))


def _tris(o, d, tris):
    """Nearest t >= 0 over the triangles [m, 3, 3] (Moller-Trumbore; inf: none)."""
    best = np.full(o.shape[0], np.inf)
    for v in np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3):
        e1, e2 = v[1] - v[0], v[2] - v[0]
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(invalid="ignore", divide="ignore"):
            inv = 1.0 / det
            tv = o - v[0]
            u = np.sum(tv * pv, -1) * inv
            q = np.cross(tv, e1)
            w = np.sum(d * q, -1) * inv
            t = (q @ e2) * inv
        hit = (det != 0.0) & (u >= 0.0) & (u <= 1.0) & (w >= 0.0) & (u + w <= 1.0) & (t >= 0.0)
        best = np.where(hit & (t < best), t, best)
    return best


def first_hit(desc, o, d, occluders=None, dheight=0.0):
    """(t, p) of world rays [n, 3]: t = inf and p = 0 on a miss."""
    kind, w, half = surface(desc, dheight)
    t = _box(o, d, (w, w, half)) if kind == "box" else _tube(o, d, w, half)
    if occluders is not None and len(occluders):
        t = np.minimum(t, _tris(o, d, occluders))
    hit = np.isfinite(t)
    p = np.where(hit[:, None], o + d * np.where(hit, t, 0.0)[:, None], 0.0)
    return t, p


def verdict(desc, o, d, dist, radius, occluders=None, dheight=0.0):
    """(hit, corner, p): corner only where hit."""
    t, p = first_hit(desc, o, d, occluders, dheight)
    hit = np.isfinite(t)
    corner = hit & (np.hypot(np.abs(p[:, 0]) - dist, np.abs(p[:, 1]) - dist) < radius)
    return hit, corner, p


def evaluate(desc, o, d, dist, radius, occluders=None):
    """The model's answer for world rays [n, 3] (float64): dict of keep, hit, t, p, undecided
    (the rule above), ptol (the hit-point tolerance) and delta."""
    dist, radius = float(np.float32(dist)), float(np.float32(radius))
    dl = delta(desc)
    t, p = first_hit(desc, o, d, occluders)
    hit, corner, _ = verdict(desc, o, d, dist, radius, occluders)
    dn = d / np.linalg.norm(d, axis=-1, keepdims=True)
    e1 = np.stack([dn[:, 1], -dn[:, 0], np.zeros(len(dn))], -1)  # horizontal, perpendicular to d
    e1 /= np.linalg.norm(e1, axis=-1, keepdims=True)
    e2 = np.cross(dn, e1)
    undecided = np.zeros(len(o), dtype=bool)
    spread = np.zeros(len(o))
    variations = [dict(o=o + s * dl * e) for e in (e1, e2) for s in (1.0, -1.0)]
    variations += [dict(radius=radius + s * dl) for s in (1.0, -1.0)]
    variations += [dict(dheight=s * dl) for s in (1.0, -1.0)]
    for v in variations:
        h2, c2, p2 = verdict(desc, v.get("o", o), d, dist, v.get("radius", radius), occluders, v.get("dheight", 0.0))
        undecided |= (h2 != hit) | (c2 != corner)
        both = hit & h2
        spread = np.maximum(spread, np.where(both, np.linalg.norm(p2 - p, axis=-1), 0.0))
    return dict(keep=hit & ~corner, hit=hit, corner=corner, t=t, p=p, undecided=undecided, ptol=dl + spread, delta=dl)


def pass_desc(desc):
    """The descriptor the corner pass samples with: regular, no time sample (spp 1, seed 0)."""
    d = copy.copy(desc) if not hasattr(desc, "copy") else desc.copy()
    d.regular_sampling = 1
    d.sample_time = 0
    return d


def corner_rays(desc, pixels, streams=None):
    """World rays (float64 o, d) of the pass for active entries `pixels` (full-DMD indices) whose
    sampler streams are `streams` (default: the positions 0..n-1)."""
    pixels = np.asarray(pixels, dtype=np.int64)
    streams = np.arange(len(pixels)) if streams is None else streams
    r = pm.model_rays(pass_desc(desc), pixels, streams, 1, 0)
    return r["o"], r["d"]


def corner_model(desc, pixels, dist, radius, streams=None, occluders=None):
    o, d = corner_rays(desc, pixels, streams)
    return evaluate(desc, o, d, dist, radius, occluders)


def compare(model, keep, hits=None):
    """Assert the rule: at most 0.5 % undecided (the model's own condition), exact verdicts on the
    rest, hit points within ptol.  keep: 0 / 1 array; hits: [n, 4] = p, t (t = -1: miss) or None.
    Returns the number of undecided pixels."""
    und = model["undecided"]
    n = len(und)
    assert und.sum() <= 0.005 * n, f"test case leaves {und.sum()} of {n} pixels undecided"
    dec = ~und
    got = np.asarray(keep) > 0
    bad = dec & (got != model["keep"])
    assert not bad.any(), f"{bad.sum()} decided pixels differ, first at entry {np.nonzero(bad)[0][:5]}"
    if hits is not None:
        hits = np.asarray(hits, dtype=np.float64)
        ghit = hits[:, 3] >= 0.0
        badh = dec & (ghit != model["hit"])
        assert not badh.any(), f"{badh.sum()} decided pixels differ in hit / miss"
        m = dec & model["hit"]
        err = np.linalg.norm(hits[m, :3] - model["p"][m], axis=-1)
        over = err > model["ptol"][m]
        assert not over.any(), f"hit points off by up to {err.max():.3e} (delta {model['delta']:.3e})"
        assert np.all(hits[dec & ~model["hit"], :3] == 0.0)
    return int(und.sum())


def plate(angle_rad, at=10.0, half_w=0.6, half_h=0.45):
    """Occluder plate (two triangles, [2, 3, 3] float32) facing the projector of rotation angle
    `angle_rad`, `at` mm from the axis.  Its diagonal passes no pixel centre of the test DMDs (0.5 mm
    pixels: lateral and z offsets of +-0.25, +-0.75), where fp32 could slip between the triangles."""
    c, s = np.cos(angle_rad), np.sin(angle_rad)
    ctr = at * np.array([c, s, 0.0])
    u = half_w * np.array([s, -c, 0.0])
    v = np.array([0.0, 0.0, half_h])
    q = [ctr - u - v, ctr + u - v, ctr + u + v, ctr - u + v]
    return np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], dtype=np.float32)


def corner_scene(vial="square", n_patterns=8, clockwise=False, crop=None, height=2.0, resx=48, resy=6, pixel=0.5):
    """The small scene of the corner tests: the vial of box_hole_square_sparsity_loss.json (w_ext
    12.408 / w_int 10.191) or a tube of radius 6.5, height 2 mm, a DMD of 48 x 6 px of 0.5 mm (wider
    than the square's diagonal, taller than the vial), a 16^3 film; 8 patterns look straight at the
    corners at 45, 135, ... degrees.  crop = (cropx, cropy, offset_x, offset_y).  Returns the config."""
    medium = {"ior": 1.347, "extinction": 0.03, "albedo": 0.0}
    if vial == "square":
        v = {"type": "square", "w_int": 10.191, "w_ext": 12.408, "ior": 1.54, "height": height, "medium": medium}
    elif vial == "cylindrical":
        v = {"type": "cylindrical", "r_int": 5.5, "r_ext": 6.5, "ior": 1.54, "height": height, "medium": medium}
    else:
        v = {"type": "index_matched", "r": 6.5, "height": height, "medium": medium}
    proj = {"type": "collimated", "n_patterns": n_patterns, "resx": resx, "resy": resy, "pixel_size": pixel,
            "motion": "circular", "distance": 20.0, "clockwise": clockwise}
    if crop is not None:
        proj |= {"cropx": crop[0], "cropy": crop[1], "crop_offset_x": crop[2], "crop_offset_y": crop[3]}
    return {
        "vial": v,
        "projector": proj,
        "sensor": {"type": "dda", "scalex": 4.0, "scaley": 4.0, "scalez": 1.6,
                   "film": {"type": "vfilm", "resx": 16, "resy": 16, "resz": 16}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.85, "tu": 0.95},
        "regular_sampling": True,
        "n_steps": 3,
    }


def outer_radius(desc):
    return surface(desc)[1]

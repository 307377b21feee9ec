"""Float64 NumPy model of a 'cylindrical' / 'square' glass vial traced per ray in 3-D (test helper,
no GPU): the path loop of volume.py:179-272 in transmission-only mode with a non-scattering medium
through the two analytic dielectric surfaces (the formulas of tvam_segment_glass,
drtvam_amd/csrc/tvam_glass.h, in exact-arithmetic form), and the scenes of the tests.

    cylindrical   open tubes r_ext, r_int around z, |z| <= half, no end caps, outward normals
    square        closed cuboids (r_ext, r_ext, half) and (r_int, r_int, 0.9 half), six faces each

trace() also returns a per-ray margin: the least relative distance of any discrete decision of the
path from going the other way (tangency, root signs, the z window, which face of a cuboid is hit,
inner-vs-outer ties, total internal reflection).  An fp32 tracer can only be compared with this
model on rays whose margin is well above fp32 rounding; the tests use 1e-4 and check that at most
1 % of their rays fall below it.  The conditioning of a segment (kappa_d, kappa_w) is that of
tests/double_vial_model.py (compare_segments there explains it)."""
import numpy as np

from double_vial_model import IOR_AIR, MARGIN, RAY_EPS, _fresnel, _tube

# the tests' vials: glass of IOR 1.54 around a resin of IOR 1.347, sigma_t 0.1; tube r_ext 6.5 /
# r_int 6.0, cuvette w_ext 13 / w_int 12, both 4 high (the cuvette's inner half height is 1.8)
IOR_GLASS, IOR_MEDIUM, SIGMA_T, HEIGHT = 1.54, 1.347, 0.1, 4.0
R_EXT, R_INT = 6.5, 6.0

LABELS = ("miss", "end_entry", "inside_first", "left_open", "horizontal", "tir", "deposit")


def _box(p, v, h, crossed, scale):
    """Nearest hit t >= 0 of the closed box [-h, h] (inf: none), its outward face normal, and the
    margin of tvam_box_hit's decisions, in units of `scale`: an axis the ray is parallel to against
    its slab, entry before exit, the signs of the entry and the exit, and which axis gives each.
    crossed: the ray has just crossed a face of this very box, so the root nearer its origin sits at
    the spawn offset, whose sign the offset settles by design: not counted as a decision."""
    n = p.shape[0]
    h = np.asarray(h, np.float64)
    par = v == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-h - p) / v, (h - p) / v
    lo = np.where(par, -np.inf, np.minimum(t0, t1))
    hi = np.where(par, np.inf, np.maximum(t0, t1))
    outside = (par & ~((p >= -h) & (p <= h))).any(1)
    m_par = np.where(par, np.abs(np.abs(p) - h) / h, np.inf).min(1)
    an, af = np.argmax(lo, 1), np.argmin(hi, 1)  # (first of equals, like the strict compares)
    tn, tf = lo.max(1), hi.min(1)
    ar = np.arange(n)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[ar, an], hi2[ar, af] = -np.inf, np.inf
    gap_n, gap_f = (tn - lo2.max(1)) / scale, (hi2.min(1) - tf) / scale
    cross = tn <= tf
    use_n = cross & (tn >= 0.0)
    use_f = cross & ~use_n & (tf >= 0.0)
    t = np.where(outside, np.inf, np.where(use_n, tn, np.where(use_f, tf, np.inf)))
    near_n = np.abs(tn) <= np.abs(tf)
    s_n = np.where(crossed & near_n, np.inf, np.abs(tn) / scale)
    s_f = np.where(crossed & ~near_n, np.inf, np.abs(tf) / scale)
    margin = np.minimum(m_par, np.abs(tf - tn) / scale)
    margin = np.minimum(margin, np.where(cross, s_n, np.inf))
    margin = np.minimum(margin, np.where(use_n, gap_n, np.inf))
    margin = np.minimum(margin, np.where(cross & ~use_n, s_f, np.inf))
    margin = np.minimum(margin, np.where(use_f, gap_f, np.inf))
    margin = np.where(outside, m_par, margin)
    ax = np.where(use_n, an, af)
    vd = v[ar, ax]
    sgn = np.where(use_n, np.where(vd > 0.0, -1.0, 1.0), np.where(vd > 0.0, 1.0, -1.0))
    nrm = np.zeros((n, 3))
    nrm[ar, ax] = sgn
    nrm[~np.isfinite(t)] = 0.0
    return t, nrm, margin


def trace(o, d, square, r_ext, r_int, half, hz_int, eta_ext, eta_int, max_depth):
    """The medium segment of world rays (o, d: [n, 3]): dict of
      hit     the ray deposits
      seg     [n, 8]: o2[0:3], maxt [3], d2[4:7], att [7] (the interfaces' transmission); zeros else
      margin  see the module text
      c2      the least of cos_theta_i^2 and cos_theta_t^2 over the interfaces crossed
      and one bool array per label:
        miss          no surface is met at all
        end_entry     the first surface met is a horizontal face (square) / a tube met from inside
                      after the ray came in through an open end (cylindrical)
        inside_first  the first surface met is met from inside (n . d > 0)
        left_open     in the medium, no further hit: left through an open end, deposits nothing
        horizontal    the segment starts or ends on a horizontal face
        tir           ended by total internal reflection
        deposit       = hit"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = o.shape[0]
    p, v = o.copy(), d.copy()
    att = np.ones(n)
    alive = np.ones(n, bool)
    in_medium = np.zeros(n, bool)
    last = np.full(n, -1)  # 0: outer, 1: inner
    seg = np.zeros((n, 8))
    hit = np.zeros(n, bool)
    margin = np.full(n, np.inf)
    c2 = np.ones(n)
    lab = {k: np.zeros(n, bool) for k in LABELS}
    start_h = np.zeros(n, bool)
    for depth in range(max_depth):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        pi, vi = p[idx], v[idx]
        if square:
            te, ne, me = _box(pi, vi, (r_ext, r_ext, half), last[idx] == 0, r_ext)
            ti, ni, mi = _box(pi, vi, (r_int, r_int, hz_int), last[idx] == 1, r_ext)
        else:
            te, me = _tube(pi, vi, r_ext, half, last[idx] == 0)
            ti, mi = _tube(pi, vi, r_int, half, last[idx] == 1)
        margin[idx] = np.minimum(margin[idx], np.minimum(me, mi))
        both = np.isfinite(te) & np.isfinite(ti)
        with np.errstate(invalid="ignore"):
            margin[idx] = np.minimum(margin[idx], np.where(both, np.abs(ti - te) / r_ext, np.inf))
        inner = ti <= te
        t = np.where(inner, ti, te)
        found = np.isfinite(t)
        gone = idx[~found]
        if depth == 0:
            lab["miss"][gone] = True
        lab["left_open"][gone[in_medium[gone]]] = True
        alive[gone] = False
        idx, t, inner = idx[found], t[found], inner[found]
        hpt = p[idx] + v[idx] * t[:, None]
        if square:
            nn = np.where(inner[:, None], ni[found], ne[found])
        else:
            rp = np.hypot(hpt[:, 0], hpt[:, 1])
            nn = np.stack([hpt[:, 0] / rp, hpt[:, 1] / rp, np.zeros(idx.size)], -1)
        horiz = nn[:, 2] != 0.0
        dep = in_medium[idx]
        di = idx[dep]
        seg[di, 0:3], seg[di, 3], seg[di, 4:7], seg[di, 7] = p[di], t[dep], v[di], att[di]
        hit[di] = True
        lab["horizontal"][di] = start_h[di] | horiz[dep]
        alive[di] = False
        idx, t, inner, hpt, nn, horiz = idx[~dep], t[~dep], inner[~dep], hpt[~dep], nn[~dep], horiz[~dep]
        cos_i = -np.sum(v[idx] * nn, -1)
        if depth == 0:
            lab["inside_first"][idx] = cos_i < 0.0
            lab["end_entry"][idx] = horiz if square else cos_i < 0.0
        r, cos_t, eta_ti, ct2 = _fresnel(cos_i, np.where(inner, eta_int, eta_ext))
        T = 1.0 - r
        margin[idx] = np.minimum(margin[idx], np.where(ct2 < 0.0, -ct2, T))
        c2[idx] = np.minimum(c2[idx], np.minimum(np.abs(ct2), cos_i * cos_i))
        wo = eta_ti[:, None] * v[idx] + (eta_ti * cos_i + cos_t)[:, None] * nn
        att[idx] *= T * eta_ti * eta_ti
        nwo = np.sum(nn * wo, -1)
        mag = (1.0 + np.max(np.abs(hpt), -1)) * RAY_EPS * np.where(nwo < 0.0, -1.0, 1.0)
        p[idx] = hpt + mag[:, None] * nn
        v[idx] = wo
        in_medium[idx] = inner & (nwo < 0.0)
        start_h[idx] = in_medium[idx] & horiz
        last[idx] = np.where(inner, 1, 0)
        dead = ~(T > 0.0)
        lab["tir"][idx[dead]] = True
        alive[idx[dead]] = False
    lab["deposit"] = hit
    return dict(hit=hit, seg=seg, margin=margin, c2=c2, **lab)


# --------------------------------------------------------------------------- scenes
def traced_config(vial="cylindrical", kind="telecentric", regular=False, angles=12, resx=48, resy=16, pitch=0.3,
                  max_depth=6, **kw):
    """The tests' scene as a config: 12 angles, DMD 48 x 16 at pitch 0.3 (rows out to +-2.4, beyond the
    vials' half height 2 and the cuvette's inner 1.8), distance = focus_distance = 20 with aperture 2
    (cone slopes up to 0.1; lens: 2.5, see below), film 40 x 40 x 24 over 13 x 13 x 4.8 (more than one 32 x 32 x 16 brick on
    x and y, a multiple on none)."""
    proj = {"type": kind, "n_patterns": angles, "resx": resx, "resy": resy, "pixel_size": pitch,
            "motion": "circular", "distance": 20.0}
    if kind != "collimated":
        # A lens ray starts on the aperture and aims at its pixel's point of the focus plane, on the
        # axis: it can come down onto the cuvette's top face only from an aperture point above that
        # face, so the lens scenes take an aperture of 2.5 > the half height 2 (slopes up to 0.125).
        proj |= {"aperture_radius": 2.5 if kind == "lens" else 2.0, "focus_distance": 20.0}
    medium = {"ior": IOR_MEDIUM, "extinction": SIGMA_T, "albedo": 0.0}
    if vial == "cylindrical":
        v = {"type": "cylindrical", "r_int": R_INT, "r_ext": R_EXT, "height": HEIGHT, "ior": IOR_GLASS, "medium": medium}
    else:
        v = {"type": "square", "w_int": 2 * R_INT, "w_ext": 2 * R_EXT, "height": HEIGHT, "ior": IOR_GLASS,
             "medium": medium}
    return {
        "vial": v, "projector": proj,
        "sensor": {"type": "dda", "scalex": 13.0, "scaley": 13.0, "scalez": 4.8,
                   "film": {"type": "vfilm", "resx": 40, "resy": 40, "resz": 24}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.9, "tu": 0.95},
        "regular_sampling": regular, "max_depth": max_depth, **kw,
    }


def traced_scene(vial="cylindrical", kind="telecentric", regular=False, **kw):
    """The descriptor of traced_config, marked for the traced entry (collimated ones too: the oracle
    cross-check of the 3-D path)."""
    from drtvam_amd.configs import desc_from_config
    d = desc_from_config(traced_config(vial, kind, regular, **kw))
    assert tuple(d.film_res) == (40, 40, 24), tuple(d.film_res)
    d.set_traced_vial()
    return d


def vial_of(desc):
    """trace()'s vial arguments of a descriptor, as the library forms them in fp32 (make_consts)."""
    f = np.float32
    half = float(f(0.5) * f(desc.vial_height))
    hz_int = float(f(0.5 * 0.9 * float(f(desc.vial_height))))
    eta_ext = float(f(desc.vial_ior) / f(IOR_AIR))
    eta_int = float(f(desc.medium_ior) / f(desc.vial_ior))
    return dict(square=int(desc.vial_type) == 2, r_ext=float(f(desc.vial_r_ext)), r_int=float(f(desc.vial_r)), half=half,
                hz_int=hz_int, eta_ext=eta_ext, eta_int=eta_int, max_depth=int(desc.max_depth))


def trace_desc(desc, o, d):
    return trace(o, d, **vial_of(desc))


_MODEL = {}


def scene_model(vial, kind, regular, spp=2, seed=3, **kw):
    """The model's rays and segments of traced_scene(vial, kind, regular), dense set (computed once;
    callers do not change it)."""
    key = (vial, kind, regular, spp, seed, tuple(sorted(kw.items())))
    if key not in _MODEL:
        import projector_model as pm
        d = traced_scene(vial, kind, regular, **kw)
        pix = pm.dense_pixels(d)
        m = pm.model_rays(d, pix, np.arange(pix.size), 1 if regular else spp, seed)
        _MODEL[key] = dict(desc=d, o=m["o"], d=m["d"], **trace_desc(d, m["o"], m["d"]))
    return _MODEL[key]


def compare_segments(got, model):
    """got [n, 8] (an fp32 tracer's segments, weight = the interfaces' transmission) against trace()'s
    dict on the rays above the margin: which rays deposit must agree.  Returns the largest |do2|,
    |dmaxt|, |dd2| and relative weight error over the segments, each divided by its segment's
    condition number kappa_d = max(1, 1 / (2 sqrt(c2))) (points, lengths, directions) or kappa_w =
    max(1, 1 / (2 c2)) (weights), and the share of rays below the margin."""
    ok = model["margin"] > MARGIN
    got = np.asarray(got, np.float64)
    has = got[:, 3] != 0.0
    assert np.array_equal(has[ok], model["hit"][ok])
    assert not got[~has].any()  # no deposit: all zeros
    ref = model["seg"]
    sel = ok & model["hit"]
    kd = np.maximum(1.0, 0.5 / np.sqrt(model["c2"][sel]))
    kw = np.maximum(1.0, 0.5 / model["c2"][sel])
    e_o = (np.abs(got[sel][:, 0:3] - ref[sel][:, 0:3]).max(1) / kd).max()
    e_t = (np.abs(got[sel][:, 3] - ref[sel][:, 3]) / kd).max()
    e_d = (np.abs(got[sel][:, 4:7] - ref[sel][:, 4:7]).max(1) / kd).max()
    e_w = (np.abs(got[sel][:, 7] / ref[sel][:, 7] - 1.0) / kw).max()
    return dict(e_o=float(e_o), e_t=float(e_t), e_d=float(e_d), e_w=float(e_w), low=float((~ok).mean()),
                compared=int(sel.sum()), kappa_w=float(kw.max()), kappa_d=float(kd.max()))

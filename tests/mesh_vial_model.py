"""Float64 NumPy model of a 'custom' vial (test helper, no GPU): mesh builders with outward
winding, and a brute-force tracer of a world ray through the two dielectric meshes to its medium
segment (volume.py:179-272 in transmission-only mode; the formulas of tvam_segment_mesh,
drtvam_amd/csrc/tvam_mesh.h, in exact-arithmetic form).

The tracer also returns a per-ray margin: how far every discrete decision of the path was from
going the other way (see trace).  An fp32 tracer can only be compared with this model on rays whose
margin is well above fp32 rounding; the tests use 1e-4 and check that at most 1 % of their rays
fall below it."""
import os

import numpy as np

RAY_EPS = 1500.0 * 2.0 ** -24   # math::RayEpsilon<float>
IOR_AIR = float(np.float32(1.000277))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-4


# --------------------------------------------------------------------------- meshes [n, 3, 3]
def _quad(a, b, c, d):
    """Two triangles of the quad a b c d (counter-clockwise seen from outside)."""
    return [[a, b, c], [a, c, d]]


def _oriented(tris):
    """Asserts the winding: every face normal points away from the z axis (side faces) or away
    from the origin (caps)."""
    t = np.asarray(tris, np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    c = t.mean(1)
    side = np.abs(n[:, 2]) < 0.999 * np.linalg.norm(n, axis=1)
    out = np.where(side, n[:, 0] * c[:, 0] + n[:, 1] * c[:, 1], n[:, 2] * c[:, 2])
    assert (out > 0).all()
    return t.astype(np.float32)


def box_tube(hx, hy, hz, closed=False):
    """Rectangular tube [-hx, hx] x [-hy, hy] x [-hz, hz]: 8 triangles, 12 with both caps."""
    p = lambda sx, sy, sz: [sx * hx, sy * hy, sz * hz]
    t = []
    t += _quad(p(1, -1, -1), p(1, 1, -1), p(1, 1, 1), p(1, -1, 1))        # +x
    t += _quad(p(-1, 1, -1), p(-1, -1, -1), p(-1, -1, 1), p(-1, 1, 1))    # -x
    t += _quad(p(1, 1, -1), p(-1, 1, -1), p(-1, 1, 1), p(1, 1, 1))        # +y
    t += _quad(p(-1, -1, -1), p(1, -1, -1), p(1, -1, 1), p(-1, -1, 1))    # -y
    if closed:
        t += _quad(p(-1, -1, 1), p(1, -1, 1), p(1, 1, 1), p(-1, 1, 1))    # +z
        t += _quad(p(-1, 1, -1), p(1, 1, -1), p(1, -1, -1), p(-1, -1, -1))  # -z
    return _oriented(t)


def square_vial_meshes(w_int, w_ext, height):
    """The closed cuboids of a SquareVial (geometry.py:186-219): outer w_ext x w_ext x height,
    inner w_int x w_int x 0.9 height."""
    return box_tube(0.5 * w_ext, 0.5 * w_ext, 0.5 * height, True), box_tube(0.5 * w_int, 0.5 * w_int, 0.45 * height, True)


def tessellated_tube(r, hz, n_phi=32, n_z=32, phase=0.0):
    """Open tube of radius r (vertices on the cylinder), n_phi x n_z quads = 2 n_phi n_z triangles."""
    phi = phase + 2.0 * np.pi * np.arange(n_phi + 1) / n_phi
    z = np.linspace(-hz, hz, n_z + 1)
    t = []
    for i in range(n_phi):
        for j in range(n_z):
            a = [r * np.cos(phi[i]), r * np.sin(phi[i]), z[j]]
            b = [r * np.cos(phi[i + 1]), r * np.sin(phi[i + 1]), z[j]]
            c = [r * np.cos(phi[i + 1]), r * np.sin(phi[i + 1]), z[j + 1]]
            d = [r * np.cos(phi[i]), r * np.sin(phi[i]), z[j + 1]]
            t += _quad(a, b, c, d)
    return _oriented(t)


def prism(r, hz, n=7, tilt_deg=8.0, phase=0.3):
    """Open n-sided prism of circumradius r, then rotated about the x axis by tilt_deg so that no
    face is vertical: a collimated ray (d.z = 0) leaves its slice at the first interface."""
    t = np.asarray(tessellated_tube(r, hz, n, 1, phase), np.float64)
    a = np.deg2rad(tilt_deg)
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    return (t @ R.T).astype(np.float32)


def cuvette():
    """The golden PLYs (the reference's open rectangular cuvette): (outer, inner)."""
    from drtvam_amd.utils import read_ply
    out = []
    for name in ("cuvette_outer.ply", "cuvette_inner.ply"):
        v, f = read_ply(os.path.join(GOLDEN, name))
        out.append(np.asarray(v, np.float32)[np.asarray(f)])
    return out[0], out[1]


def scene_meshes(name):
    """(outer, inner) of the GPU scenes: around projector_model.projector_scene's 4 x 3.6 x 2 mm film."""
    if name == "cuvette":
        return cuvette()
    if name == "prism":
        return prism(3.9, 6.0), prism(3.25, 6.0)
    if name == "tube":  # 2048 triangles per surface
        return tessellated_tube(3.4, 5.0), tessellated_tube(2.95, 5.0, phase=0.05)
    raise KeyError(name)


# --------------------------------------------------------------------------- tracer
def _closest(tris, o, d):
    """Brute force Moller-Trumbore of rays [n, 3] against triangles [m, 3, 3] in float64: nearest
    t >= 0 (inf: none), its triangle, the gap to the second nearest hit, and the least distance of
    any triangle from changing its answer, |min(u, w, 1 - u - w)| over the triangles whose plane
    the ray meets at t >= 0 (for a triangle the ray misses this is its largest violated edge test).
    Only (ray, triangle) pairs whose ray passes the triangle's bounding sphere, grown by 5 % and
    1e-3, are evaluated: the others miss by more than that and decide nothing."""
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    n = o.shape[0]
    cen = tris.mean(1)
    rad = np.linalg.norm(tris - cen[:, None], axis=-1).max(1)
    along = d @ cen.T - np.sum(o * d, -1)[:, None]                       # (c - o) . d
    dist2 = np.sum(o * o, -1)[:, None] + np.sum(cen * cen, -1)[None] - 2.0 * (o @ cen.T) - along ** 2
    ri, tj = np.nonzero(dist2 <= (1.05 * rad[None] + 1e-3) ** 2)
    oo, dd = o[ri], d[ri]
    p = np.cross(dd, e2[tj])
    det = np.sum(e1[tj] * p, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = oo - v0[tj]
        u = np.sum(tv * p, -1) * inv
        q = np.cross(tv, e1[tj])
        w = np.sum(dd * q, -1) * inv
        t = np.sum(e2[tj] * q, -1) * inv
        bary = np.minimum(np.minimum(u, w), 1.0 - u - w)
    ok = np.isfinite(u) & np.isfinite(w) & np.isfinite(t) & (np.abs(det) > 1e-300)
    front = ok & (t >= 0.0)
    th = np.where(front & (bary >= 0.0), t, np.inf)
    t_best, i_best = np.full(n, np.inf), np.full(n, -1)
    gap, edge = np.full(n, np.inf), np.full(n, np.inf)
    np.minimum.at(edge, ri, np.where(front, np.abs(bary), np.inf))
    order = np.lexsort((th, ri))
    rs, ts, js = ri[order], th[order], tj[order]
    pos = np.nonzero(np.r_[True, rs[1:] != rs[:-1]])[0] if rs.size else np.zeros(0, np.int64)
    rays = rs[pos]
    t_best[rays] = ts[pos]
    i_best[rays] = np.where(np.isfinite(ts[pos]), js[pos], -1)
    nxt = np.minimum(pos + 1, rs.size - 1)
    second = np.where((pos + 1 < rs.size) & (rs[nxt] == rays), ts[nxt], np.inf)
    with np.errstate(invalid="ignore"):
        gap[rays] = np.where(np.isfinite(ts[pos]), second - ts[pos], np.inf)
    return t_best, i_best, gap, edge


def _fresnel(cos_i, eta):
    """Mitsuba fresnel(): reflectance, signed cos_theta_t, eta_ti (and cos_theta_t^2 before its clamp:
    negative = total internal reflection)."""
    outside = cos_i >= 0.0
    eta_it = np.where(outside, eta, 1.0 / eta)
    eta_ti = np.where(outside, 1.0 / eta, eta)
    ct2 = 1.0 - (1.0 - cos_i * cos_i) * (eta_ti * eta_ti)
    ci, ct = np.abs(cos_i), np.sqrt(np.maximum(ct2, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        a_s = (ci - eta_it * ct) / (ci + eta_it * ct)
        a_p = (ct - eta_it * ci) / (ct + eta_it * ci)
    r = 0.5 * (a_s * a_s + a_p * a_p)
    r = np.where(ci == 0.0, 1.0, r)
    r = np.where(eta == 1.0, 0.0, r)
    return r, np.where(outside, -ct, ct), eta_ti, ct2


def trace(o, d, outer, inner, eta_ext, eta_int, max_depth):
    """Medium segments of world rays (o, d: [n, 3]) behind the dielectric meshes outer / inner
    ([m, 3, 3], wound outwards): dict of hit (the ray deposits), o2, d2, maxt, weight (product of
    the interfaces' transmission weights) and margin.

    Per surface: the nearest hit over both meshes (none: the ray ends, nothing deposited), the
    face normal n = normalize((v1 - v0) x (v2 - v0)), transmission wo = eta_ti d + (eta_ti cos_i +
    cos_t) n with weight (1 - F) eta_ti^2 (0: the ray ends), the spawn offset (1 + max|h|) RayEpsilon
    along n on wo's side; in_medium = inner mesh and n . wo < 0; once in the medium the next
    nearest hit ends the segment.  At most max_depth surfaces.

    margin = the minimum over the ray's surfaces of: the distance of every triangle plane the ray
    meets ahead from an edge decision (barycentric), the gap in t between the nearest and the
    second nearest hit, and the distance of the Fresnel transmission 1 - F from 0 (under total
    internal reflection, where 1 - F = 0 identically: of cos_theta_t^2 from 0)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    tris = np.concatenate([np.asarray(outer, np.float64), np.asarray(inner, np.float64)])
    n_outer = len(outer)
    nrm = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    n = o.shape[0]
    p, v = o.copy(), d.copy()
    att = np.ones(n)
    alive = np.ones(n, bool)
    in_medium = np.zeros(n, bool)
    hit = np.zeros(n, bool)
    o2, d2, maxt = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    margin = np.full(n, np.inf)
    for _ in range(max_depth):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, tri, gap, edge = _closest(tris, p[idx], v[idx])
        margin[idx] = np.minimum(margin[idx], np.minimum(gap, edge))
        found = np.isfinite(t)
        alive[idx[~found]] = False
        done = found & in_medium[idx]
        di = idx[done]
        hit[di], o2[di], d2[di], maxt[di] = True, p[di], v[di], t[done]
        alive[di] = False
        go = found & ~in_medium[idx]
        gi = idx[go]
        if gi.size == 0:
            continue
        tg, trg = t[go], tri[go]
        is_inner = trg >= n_outer
        nn = nrm[trg]
        h = p[gi] + v[gi] * tg[:, None]
        cos_i = -np.sum(v[gi] * nn, -1)
        r, cos_t, eta_ti, ct2 = _fresnel(cos_i, np.where(is_inner, eta_int, eta_ext))
        T = 1.0 - r
        margin[gi] = np.minimum(margin[gi], np.where(ct2 < 0.0, -ct2, T))
        wo = eta_ti[:, None] * v[gi] + (eta_ti * cos_i + cos_t)[:, None] * nn
        passed = T > 0.0
        att[gi] *= T * eta_ti * eta_ti
        nwo = np.sum(nn * wo, -1)
        mag = (1.0 + np.max(np.abs(h), -1)) * RAY_EPS * np.where(nwo < 0.0, -1.0, 1.0)
        p[gi] = h + mag[:, None] * nn
        v[gi] = wo
        in_medium[gi] = is_inner & (nwo < 0.0)
        alive[gi[~passed]] = False
    return dict(hit=hit, o2=o2, d2=d2, maxt=maxt, weight=np.where(hit, att, 0.0), margin=margin)


# --------------------------------------------------------------------------- GPU scenes
VIAL_IOR, MEDIUM_IOR = 1.4702, 1.33


def custom_scene(kind, mesh, **kw):
    """projector_model.projector_scene(kind) behind the 'custom' vial `mesh` (scene_meshes)."""
    import projector_model as pm
    from drtvam_amd import _abi
    d = pm.projector_scene(kind, **kw)
    d.vial_type = _abi.VIAL_CUSTOM
    d.vial_ior, d.medium_ior = VIAL_IOR, MEDIUM_IOR
    d.vial_r = d.vial_r_ext = d.vial_height = 0.0  # unused by this vial type
    outer, inner = scene_meshes(mesh)
    d.set_vial_meshes(outer, inner)
    return d


def etas(desc):
    """(eta_ext, eta_int) as make_consts forms them in fp32."""
    return (float(np.float32(desc.vial_ior) / np.float32(IOR_AIR)),
            float(np.float32(desc.medium_ior) / np.float32(desc.vial_ior)))


_MODEL = {}


def scene_model(kind, mesh, spp, seed):
    """The model's rays of custom_scene(kind, mesh), dense set (computed once): projector_model's
    (o, d) traced through the meshes."""
    key = (kind, mesh, spp, seed)
    if key not in _MODEL:
        import projector_model as pm
        d = custom_scene(kind, mesh)
        pix = pm.dense_pixels(d)
        m = pm.model_rays(d, pix, np.arange(pix.size), spp, seed)
        e_ext, e_int = etas(d)
        tr = trace(m["o"], m["d"], d._vial_outer, d._vial_inner, e_ext, e_int, d.max_depth)
        _MODEL[key] = dict(desc=d, o=m["o"], d=m["d"], **tr)
    return _MODEL[key]

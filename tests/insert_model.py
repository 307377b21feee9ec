"""Float64 NumPy model of dielectric occluders inside the resin (test helper, no GPU): the path loop
of volume.py:179-272 in transmission-only mode with a non-scattering medium through the container,
the black occluders and the inserts' triangles (the formulas of tvam_insert_next,
drtvam_amd/csrc/tvam_insert.h, in exact-arithmetic form), the test meshes, and the scenes of the
tests.

    surface                       medium flag after crossing
    container's outer glass       off
    container's medium boundary   inwards (n . wo < 0): on, outwards: off
    black occluder                the path ends after the deposit
    insert face                   inwards (n . wo < 0): off, outwards: on

Per iteration: one roulette draw (acts when depth > rr_depth, q = min(0.99, attenuation)), the
nearest hit over container, black occluders, inserts (a later candidate wins only when strictly
nearer), a segment (p, v, [0, t]) of weight attenuation when in the medium, the Fresnel
transmission, e^{-sigma_t t} after a medium segment, the spawn offset.

trace() also returns a per-ray margin: the least relative distance of any discrete decision of the
path from going the other way: the container's own decisions (double_vial_model._tube,
traced_vial_model._box), which candidate is nearest, per triangle the barycentric edge distance
and the sign of t, total internal reflection, and the roulette's u < q.  An fp32 tracer can only be
compared with this model on rays whose margin is well above fp32 rounding; the tests use 1e-4 and
check that at most 1 % of their rays fall below it."""
import os

import numpy as np

from double_vial_model import IOR_AIR, MARGIN, RAY_EPS, _fresnel, _tube, compare_segments  # noqa: F401
from traced_vial_model import _box

MAX_SEGMENTS = 6
CHUNK = 2048  # rays per block of the triangle tests (memory)

# the documented example's numbers (container.rst, "Occlusions")
INT_IOR, EXT_IOR = 1.58, 1.4849
IOR_GLASS, IOR_MEDIUM, SIGMA_T = 1.54, 1.4849, 1.0


# --------------------------------------------------------------------------- meshes
def _rot(rz=0.0, rx=0.0):
    cz, sz, cx, sx = np.cos(rz), np.sin(rz), np.cos(rx), np.sin(rx)
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    return Rz @ Rx


def _place(tris, rz=0.0, rx=0.0, shift=(0.0, 0.0, 0.0)):
    """Rotate about x then z, shift, and round to what a PLY file holds (float32)."""
    t = np.asarray(tris, np.float64) @ _rot(rz, rx).T + np.asarray(shift, np.float64)
    return t.astype(np.float32)


def _quad(a, b, c, d, n=1):
    """The quad a b c d (counter-clockwise seen from outside) as 2 n^2 triangles."""
    a, b, c, d = (np.asarray(x, np.float64) for x in (a, b, c, d))
    out = []
    for i in range(n):
        for j in range(n):
            def pt(s, t):
                s, t = s / n, t / n
                return (1 - s) * (1 - t) * a + s * (1 - t) * b + s * t * c + (1 - s) * t * d
            p00, p10, p11, p01 = pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)
            out += [[p00, p10, p11], [p00, p11, p01]]
    return out


def box_tris(lo, hi, n=1):
    """A closed box wound outwards, 12 n^2 triangles."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    t = []
    t += _quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), n)  # +x
    t += _quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), n)  # -x
    t += _quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), n)  # +y
    t += _quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), n)  # -y
    t += _quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), n)  # +z
    t += _quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0), n)  # -z
    return np.asarray(t, np.float64)


def prism_tris(n=7, radius=0.6, z0=-0.5, z1=0.5):
    """A closed n-gon prism around z wound outwards: 2 n side triangles and 2 (n - 2) cap triangles."""
    a = 2.0 * np.pi * np.arange(n) / n
    lo = np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z0)], -1)
    hi = lo.copy()
    hi[:, 2] = z1
    t = []
    for i in range(n):
        j = (i + 1) % n
        t += _quad(lo[i], lo[j], hi[j], hi[i])
    for i in range(1, n - 1):
        t.append([hi[0], hi[i], hi[i + 1]])
        t.append([lo[0], lo[i + 1], lo[i]])
    return np.asarray(t, np.float64)


def u_tris(w=1.6, d=1.2, arm=0.4, base=0.4, z0=-0.5, z1=0.5):
    """A non-convex U-piece (open towards +y): two arms of width `arm` on a base of depth `base`, as
    three boxes' outer faces: a ray along x above the base crosses both arms and the gap."""
    x0, x1, y0, y1 = -0.5 * w, 0.5 * w, -0.5 * d, 0.5 * d
    yb = y0 + base
    xa, xb = x0 + arm, x1 - arm
    poly = [(x0, y0), (x1, y0), (x1, y1), (xb, y1), (xb, yb), (xa, yb), (xa, y1), (x0, y1)]  # counter-clockwise
    t = []
    for i in range(len(poly)):
        (ax, ay), (bx, by) = poly[i], poly[(i + 1) % len(poly)]
        t += _quad((ax, ay, z0), (bx, by, z0), (bx, by, z1), (ax, ay, z1))
    for (ax, ay, bx, by) in ((x0, y0, x1, yb), (x0, yb, xa, y1), (xb, yb, x1, y1)):  # caps: base, left arm, right arm
        t += _quad((ax, ay, z1), (bx, ay, z1), (bx, by, z1), (ax, by, z1))
        t += _quad((ax, ay, z0), (ax, by, z0), (bx, by, z0), (bx, ay, z0))
    return np.asarray(t, np.float64)


def check_closed(tris):
    """A closed mesh wound outwards (its caps may be split along inner lines, so edges are not paired up):
    the area vectors sum to zero and the signed volume is positive."""
    t = np.asarray(tris, np.float64)
    cr = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    vol = np.sum(t[:, 0] * cr) / 6.0
    return vol > 0.0 and np.abs(cr.sum(0)).max() < 1e-5 * np.abs(cr).sum()


# The tests' meshes, posed inside the film of the scenes below (|x| < 2, |y| < 1.8, |z| < 1) and
# away from the pixel grid's symmetry (odd angles, shifts that are no multiple of the pixel pitch).
def mesh(name):
    if name == "box":          # 12 triangles: the brute-force loop
        return _place(box_tris((-0.55, -0.45, -0.4), (0.55, 0.45, 0.4)), rz=0.31, rx=0.0, shift=(0.233, -0.171, 0.047))
    if name == "prism":        # tilted: its faces take rays out of their z-plane (24 triangles: the hierarchy)
        return _place(prism_tris(7, 0.62, -0.45, 0.45), rz=0.2, rx=0.37, shift=(-0.187, 0.263, -0.031))
    if name == "u":            # non-convex: up to three medium segments (28 triangles)
        return _place(u_tris(), rz=0.43, rx=0.11, shift=(0.127, 0.091, 0.023))
    if name == "fine":         # 432 triangles: the hierarchy exceeds the LDS budget
        return _place(box_tris((-0.55, -0.45, -0.4), (0.55, 0.45, 0.4), n=6), rz=0.31, rx=0.23,
                      shift=(0.233, -0.171, 0.047))
    if name == "far":          # above every lit ray (DMD rows reach |z| <= 1.5) and inside the cuvette's resin (|z| <= 1.8)
        return _place(box_tris((-0.5, -0.5, -0.09), (0.5, 0.5, 0.09)), shift=(0.0, 0.0, 1.69))
    if name == "black":        # a black occluder behind the inserts
        return _place(box_tris((-0.25, -0.3, -0.5), (0.25, 0.3, 0.5)), rz=0.17, shift=(-1.31, 0.93, 0.013))
    raise KeyError(name)


MESHES = ("box", "prism", "u", "fine", "far", "black")


def write_ply(path, tris):
    """Triangles [n][3][3] as a binary little-endian PLY with float32 vertices, three per triangle in
    their order (utils.read_ply reads it; the winding is kept)."""
    t = np.ascontiguousarray(tris, dtype="<f4").reshape(-1, 3, 3)
    n = t.shape[0]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nelement face %d\nproperty list uchar uint vertex_indices\nend_header\n" % (3 * n, n))
    faces = np.zeros(n, dtype=[("c", "u1"), ("i", "<u4", 3)])
    faces["c"] = 3
    faces["i"] = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(t.tobytes())
        f.write(faces.tobytes())


def write_meshes(dirpath):
    """Every test mesh as <dirpath>/<name>.ply; returns {name: path}."""
    out = {}
    for name in MESHES:
        out[name] = os.path.join(str(dirpath), name + ".ply")
        if not os.path.exists(out[name]):
            write_ply(out[name], mesh(name))
    return out


# --------------------------------------------------------------------------- triangles
def _tri_hits(p, v, tris, crossed, scale):
    """Nearest hit t >= 0 (inf: none) of rays (p, v: [n, 3]) with triangles [m, 3, 3] (Moller-Trumbore,
    tvam_tri_hit's tests: 0 <= u <= 1, w >= 0, u + w <= 1, t >= 0), its triangle, and the margin of
    those decisions: per triangle the barycentric distance b = min(u, w, 1 - u - w) from an edge and
    |t| / scale from the origin, combined by whether each alone decides; plus the gap between the
    nearest and the second nearest hit.  crossed [n]: the triangle the ray has just crossed (-1:
    none), whose sign of t the spawn offset settles by design."""
    n, m = p.shape[0], tris.shape[0]
    tbest, slot, margin = np.full(n, np.inf), np.full(n, -1), np.full(n, np.inf)
    if m == 0:
        return tbest, slot, margin
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    for a in range(0, n, CHUNK):
        sl = slice(a, min(n, a + CHUNK))
        pp, vv = p[sl], v[sl]
        k = pp.shape[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            pv = np.cross(vv[:, None, :], e2[None])
            inv = 1.0 / np.sum(e1[None] * pv, -1)
            tv = pp[:, None, :] - v0[None]
            u = np.sum(tv * pv, -1) * inv
            q = np.cross(tv, e1[None])
            w = np.sum(vv[:, None, :] * q, -1) * inv
            t = np.sum(e2[None] * q, -1) * inv
            b = np.minimum(np.minimum(u, w), 1.0 - u - w)
        ok = np.isfinite(b) & np.isfinite(t)
        hit = ok & (b >= 0.0) & (t >= 0.0)
        ts = np.abs(t) / scale
        mg = np.where(b >= 0.0, np.where(t >= 0.0, np.minimum(b, ts), ts),
                      np.where(t >= 0.0, -b, np.maximum(-b, ts)))
        mg = np.where(ok, mg, np.inf)  # an exactly parallel ray: 0 / 0 on both sides
        cr = crossed[sl]
        has = cr >= 0
        mg[np.nonzero(has)[0], cr[has]] = np.inf
        th = np.where(hit, t, np.inf)
        j = np.argmin(th, 1)
        ar = np.arange(k)
        t1 = th[ar, j]
        th2 = th.copy()
        th2[ar, j] = np.inf
        t2 = th2.min(1)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(t2), (t2 - t1) / scale, np.inf)
        tbest[sl] = t1
        slot[sl] = np.where(np.isfinite(t1), j, -1)
        margin[sl] = np.minimum(mg.min(1), gap)
    return tbest, slot, margin


def tri_normals(tris):
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


# --------------------------------------------------------------------------- the walk
def trace(o, d, cont, tris, tri_eta, sigma_t, max_depth, black=None, rr_depth=None, u=None,
          max_segments=MAX_SEGMENTS, flaw=None):
    """Medium segments of world rays (o, d: [n, 3]).
      cont     the container: dict(square, r_ext, r_int, half, hz_int, eta_ext, eta_int) of a glass vial
               (traced_vial_model.vial_of) or dict(r, half) of an index-matched one
      tris     [m, 3, 3] every insert's triangles, tri_eta [m] their eta = int_ior / ext_ior
      black    [k, 3, 3] black occluder triangles or None
      u        [n, max_depth, 4] the four draws of each iteration, or None: roulette never acts
      flaw     a planted error (the tests of the checker): 'flag' (the medium flag is not cleared inside
               an insert), 'exp' (e^{-sigma_t t} is applied inside an insert too), 'eta' (the inserts'
               eta inverted)
    Returns a dict of
      n       segments deposited
      segs    [n, max_segments, 8]: o2[0:3], maxt [3], d2[4:7], weight [7] (the attenuation the segment
              starts with); zeros where there is no segment
      iters   [n, max_segments] loop iteration of each deposit (-1: none)
      margin  see the module text
      ct2     [n, max_segments] the least of cos_theta_i^2 and cos_theta_t^2 over the interfaces crossed
              before each segment (double_vial_model.compare_segments) and of cos_theta_i^2 at the surface
              the segment ends on
      ends    [n] why the path ended: 'none' (no further hit), 'black', 'tir', 'depth', 'rr'"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    tri_eta = np.asarray(tri_eta, np.float64)
    if flaw == "eta":
        tri_eta = 1.0 / tri_eta
    black = np.zeros((0, 3, 3)) if black is None else np.asarray(black, np.float64).reshape(-1, 3, 3)
    nrm_ins, nrm_blk = tri_normals(tris), (tri_normals(black) if len(black) else np.zeros((0, 3)))
    glass = "r_ext" in cont
    square = bool(cont.get("square", False))
    scale = cont["r_ext"] if glass else cont["r"]
    n = o.shape[0]
    p, v = o.copy(), d.copy()
    att = np.ones(n)
    alive = np.ones(n, bool)
    in_medium = np.zeros(n, bool)
    inside_ins = np.zeros(n, bool)   # (flaw 'exp')
    last = np.full(n, -1)            # container surface just crossed: 0 outer, 1 medium boundary
    last_tri = np.full(n, -1)        # insert triangle just crossed
    nseg = np.zeros(n, np.int64)
    segs = np.zeros((n, max_segments, 8))
    iters = np.full((n, max_segments), -1)
    margin = np.full(n, np.inf)
    ct2min = np.ones(n)
    ct2seg = np.ones((n, max_segments))
    ends = np.full(n, "depth", dtype=object)
    for depth in range(max_depth):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        if u is not None:
            q = np.minimum(0.99, att[idx])
            if depth > rr_depth:
                ur = np.asarray(u, np.float64)[idx, depth, 0]
                margin[idx] = np.minimum(margin[idx], np.abs(ur - q))
                keep = ur < q
                att[idx] = att[idx] / q
                ends[idx[~keep]] = "rr"
                alive[idx[~keep]] = False
                idx = idx[keep]
        pi, vi = p[idx], v[idx]
        k = idx.size
        # the container
        if glass and square:
            te, ne, me = _box(pi, vi, (cont["r_ext"], cont["r_ext"], cont["half"]), last[idx] == 0, scale)
            ti, ni, mi = _box(pi, vi, (cont["r_int"], cont["r_int"], cont["hz_int"]), last[idx] == 1, scale)
        elif glass:
            te, me = _tube(pi, vi, cont["r_ext"], cont["half"], last[idx] == 0)
            ti, mi = _tube(pi, vi, cont["r_int"], cont["half"], last[idx] == 1)
        else:
            ti, mi = _tube(pi, vi, cont["r"], cont["half"], last[idx] == 1)
            te, me = np.full(k, np.inf), np.full(k, np.inf)
        margin[idx] = np.minimum(margin[idx], np.minimum(me, mi))
        inner = ti <= te
        t = np.where(inner, ti, te)
        kind = np.where(inner, 1, 0)  # 0 outer glass, 1 medium boundary, 2 black, 3 insert
        tb, sb, mb = _tri_hits(pi, vi, black, np.full(k, -1), scale)
        tm, sm, mm = _tri_hits(pi, vi, tris, last_tri[idx], scale)
        margin[idx] = np.minimum(margin[idx], np.minimum(mb, mm))
        # which candidate is nearest: the gap between the two nearest of the four
        cand = np.sort(np.stack([te, ti, tb, tm], -1), -1)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(cand[:, 1]), (cand[:, 1] - cand[:, 0]) / scale, np.inf)
        margin[idx] = np.minimum(margin[idx], gap)
        use_b = tb < t
        t, kind = np.where(use_b, tb, t), np.where(use_b, 2, kind)
        use_m = tm < t
        t, kind = np.where(use_m, tm, t), np.where(use_m, 3, kind)
        found = np.isfinite(t)
        ends[idx[~found]] = "none"
        alive[idx[~found]] = False
        sel = np.nonzero(found)[0]
        idx, t, kind, inner, sm, sb = idx[sel], t[sel], kind[sel], inner[sel], sm[sel], sb[sel]
        # the surface met: hit point, normal, cos_theta_i
        h = p[idx] + v[idx] * t[:, None]
        if glass and square:
            nn = np.where(inner[:, None], ni[sel], ne[sel])
        else:
            rp = np.hypot(h[:, 0], h[:, 1])
            nn = np.stack([h[:, 0] / rp, h[:, 1] / rp, np.zeros(idx.size)], -1)
        isi, isb = kind == 3, kind == 2
        nn[isi] = nrm_ins[sm[isi]]
        nn[isb] = nrm_blk[sb[isb]]
        cos_i = -np.sum(v[idx] * nn, -1)
        # the deposit.  Its length is the distance to that surface, (plane - p) . n / cos_i on a flat face: an fp32
        # rounding of cos_i moves it by that over |cos_i|, so the segment's conditioning takes the end surface's
        # cos_i^2 beside those of the interfaces crossed before it (a tube met at grazing incidence is a tangency:
        # _tube's margin)
        dep = in_medium[idx]
        di, ks = idx[dep], nseg[idx[dep]]
        fits = ks < max_segments
        dj, kj = di[fits], ks[fits]
        segs[dj, kj, 0:3], segs[dj, kj, 3], segs[dj, kj, 4:7], segs[dj, kj, 7] = p[dj], t[dep][fits], v[dj], att[dj]
        iters[dj, kj] = depth
        ct2seg[dj, kj] = np.minimum(ct2min[dj], (cos_i * cos_i)[dep][fits])
        nseg[di] += 1
        ends[idx[isb]] = "black"
        alive[idx[isb]] = False
        go = ~isb
        idx, t, kind, sm, dep, h, nn, isi, cos_i = (idx[go], t[go], kind[go], sm[go], dep[go], h[go], nn[go], isi[go],
                                                    cos_i[go])
        if glass:
            eta = np.where(kind == 1, cont["eta_int"], cont["eta_ext"])
        else:
            eta = np.ones(idx.size)
        eta = np.where(isi, tri_eta[np.maximum(sm, 0)], eta)
        r, cos_t, eta_ti, ct2 = _fresnel(cos_i, eta)
        T = 1.0 - r
        margin[idx] = np.minimum(margin[idx], np.where(ct2 < 0.0, -ct2, T))
        ct2min[idx] = np.minimum(ct2min[idx], np.minimum(np.abs(ct2), cos_i * cos_i))
        wo = eta_ti[:, None] * v[idx] + (eta_ti * cos_i + cos_t)[:, None] * nn
        att[idx] *= T * eta_ti * eta_ti
        damp = dep | (inside_ins[idx] if flaw == "exp" else False)
        att[idx] *= np.where(damp, np.exp(-sigma_t * t), 1.0)
        nwo = np.sum(nn * wo, -1)
        mag = (1.0 + np.max(np.abs(h), -1)) * RAY_EPS * np.where(nwo < 0.0, -1.0, 1.0)
        p[idx] = h + mag[:, None] * nn
        v[idx] = wo
        new_flag = ((kind == 1) & (nwo < 0.0)) | (isi & (nwo > 0.0))
        if flaw == "flag":  # (the planted error: an insert face crossed inwards leaves the flag as it was)
            new_flag = np.where(isi & (nwo < 0.0), in_medium[idx], new_flag)
        in_medium[idx] = new_flag
        inside_ins[idx] = isi & (nwo < 0.0)
        last[idx] = np.where(isi, -1, kind)
        last_tri[idx] = np.where(isi, sm, -1)
        dead = ~(T > 0.0)
        ends[idx[dead]] = "tir"
        alive[idx[dead]] = False
    return dict(n=nseg, segs=segs, iters=iters, margin=margin, ct2=ct2seg, ends=ends)


def slab_closed_form(n1, n2, sigma_t, t1):
    """A slab of IOR n2 in a resin of IOR n1 at normal incidence: the two faces' transmission (1 - F)^2,
    F = ((n1 - n2) / (n1 + n2))^2 (the eta_ti^2 factors cancel), and the attenuation e^{-sigma_t t1} of the
    resin path t1 in front of it alone."""
    F = ((n1 - n2) / (n1 + n2)) ** 2
    return (1.0 - F) ** 2, np.exp(-sigma_t * t1)


# --------------------------------------------------------------------------- scenes
def insert_config(vial="index_matched", kind="collimated", regular=True, inserts=("box",), black=False, paths=None,
                  max_depth=8, rr_depth=8, int_ior=INT_IOR, ext_ior=EXT_IOR, extinction=SIGMA_T, **kw):
    """The tests' scene as a config, at the size of projector_model.projector_scene: DMD 24 x 20 px of
    0.15 mm, 6 patterns, film 40 x 36 x 20 voxels of 0.1 mm, sigma_t 1 / mm (`extinction`), distance = focus_distance =
    20 with aperture 2; the vial index matched (r 2.9), cylindrical (2.9 / 3.2) or square (5.8 / 6.4),
    4 mm high; the named meshes (write_meshes: `paths`) as dielectric occluders, 'black' as a black one."""
    proj = {"type": kind, "n_patterns": 6, "resx": 24, "resy": 20, "pixel_size": 0.15, "motion": "circular",
            "distance": 20.0}
    if kind != "collimated":
        proj |= {"aperture_radius": 2.0, "focus_distance": 20.0}
    occ = [{"filename": paths[m], "bsdf": {"type": "dielectric", "int_ior": int_ior, "ext_ior": ext_ior}} for m in inserts]
    if black:
        occ.append({"filename": paths["black"]})
    medium = {"ior": IOR_MEDIUM, "extinction": extinction, "albedo": 0.0}
    if vial == "index_matched":
        v = {"type": "index_matched", "r": 2.9, "height": 4.0, "medium": medium}
    elif vial == "cylindrical":
        v = {"type": "cylindrical", "r_int": 2.9, "r_ext": 3.2, "height": 4.0, "ior": IOR_GLASS, "medium": medium}
    else:
        v = {"type": "square", "w_int": 5.8, "w_ext": 6.4, "height": 4.0, "ior": IOR_GLASS, "medium": medium}
    if occ:
        v["occlusions"] = occ
    return {
        "vial": v, "projector": proj,
        "sensor": {"type": "dda", "scalex": 4.0, "scaley": 3.6, "scalez": 2.0,
                   "film": {"type": "vfilm", "resx": 36, "resy": 40, "resz": 20}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.9, "tu": 0.95},
        "regular_sampling": regular, "max_depth": max_depth, "rr_depth": rr_depth, **kw,
    }


def insert_scene(dirpath, vial="index_matched", kind="collimated", regular=True, inserts=("box",), black=False, **kw):
    from drtvam_amd.configs import desc_from_config
    d = desc_from_config(insert_config(vial, kind, regular, inserts, black, write_meshes(dirpath), **kw))
    assert tuple(d.film_res) == (40, 36, 20), tuple(d.film_res)
    return d


def container_of(desc):
    """trace()'s container of a descriptor, as the library forms it in fp32 (make_consts)."""
    import traced_vial_model as tv
    if int(desc.vial_type) == 0:
        f = np.float32
        return dict(r=float(f(desc.vial_r)), half=float(f(0.5) * f(desc.vial_height)))
    c = tv.vial_of(desc)
    c.pop("max_depth")
    return c


def inserts_of(desc):
    """(tris [m, 3, 3], tri_eta [m], black [k, 3, 3] or None) of a descriptor, eta formed in fp32."""
    f = np.float32
    ins = desc.inserts
    tris = np.concatenate([t for t, _, _ in ins]).astype(np.float64) if ins else np.zeros((0, 3, 3))
    eta = np.concatenate([np.full(t.shape[0], float(f(ni) / f(ne))) for t, ni, ne in ins]) if ins else np.zeros(0)
    black = getattr(desc, "_occluders", None)
    return tris, eta, (None if black is None or not black.size else black.astype(np.float64))


def trace_desc(desc, o, d, u=None, **kw):
    tris, eta, black = inserts_of(desc)
    return trace(o, d, container_of(desc), tris, eta, float(np.float32(desc.sigma_t)), int(desc.max_depth), black=black,
                 rr_depth=int(desc.rr_depth), u=u, **kw)


def roulette_on(desc):
    """tvam_insert_roulette_on: whether roulette can act on a path of the descriptor's limits."""
    return int(desc.rr_depth) < int(desc.max_depth) - 1


def path_draws(desc, streams, spp, seed):
    """The four draws of each loop iteration of the rays model_rays(desc, pixels, streams, spp, seed) casts:
    [n * spp, max_depth, 4], drawn from each ray's own generator after its prefix (position pair when
    jittered, time under sample_time, aperture pair)."""
    import projector_model as pm
    st = np.repeat(np.asarray(streams, dtype=np.uint64), spp) * np.uint64(spp) + \
        np.tile(np.arange(spp, dtype=np.uint64), len(streams))
    smp = pm.Sampler(seed, st)
    for _ in range((0 if desc.regular_sampling else 2) + (1 if desc.sample_time else 0) + 2):
        smp.next_float()
    u = np.empty((st.size, int(desc.max_depth), 4))
    for it in range(int(desc.max_depth)):
        for c in range(4):
            u[:, it, c] = smp.next_float()
    return u


_MODEL = {}


def scene_model(dirpath, vial, kind, regular, spp=2, seed=3, **kw):
    """The model's rays and segments of insert_scene(...), dense set (computed once; callers do not
    change it)."""
    key = (vial, kind, regular, spp, seed, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _MODEL:
        import projector_model as pm
        d = insert_scene(dirpath, vial, kind, regular, **kw)
        pix = pm.dense_pixels(d)
        spp_ = 1 if regular else spp
        m = pm.model_rays(d, pix, np.arange(pix.size), spp_, seed)
        u = path_draws(d, np.arange(pix.size), spp_, seed) if roulette_on(d) else None
        _MODEL[key] = dict(desc=d, spp=spp_, o=m["o"], d=m["d"], u=u, **trace_desc(d, m["o"], m["d"], u=u))
    return _MODEL[key]


# The scenes of the GPU film-parity tests (tests/test_gpu_inserts.py): name -> (vial, kind, regular, keywords).
FILM_VARIANTS = {
    "im-collimated-box": ("index_matched", "collimated", True, dict(inserts=("box",))),               # brute force, LDS
    "cyl-telecentric-u-black": ("cylindrical", "telecentric", False, dict(inserts=("u",), black=True)),  # hierarchy in LDS
    "square-lens-fine": ("square", "lens", False, dict(inserts=("fine",))),                           # hierarchy in global memory
    "square-collimated-u-black-rr": ("square", "collimated", False,                                   # roulette acts
                                     dict(inserts=("u",), black=True, max_depth=16, rr_depth=2, extinction=0.2)),
}
FILM_SPP, FILM_SEED = 3, 3


def film_keep(m):
    """The pixels a film comparison keeps: every sample's ray above the margin.  A pixel is left out whole (its
    pattern value is one number), so the rays left out are spp per such pixel."""
    spp = m["spp"]
    return (m["margin"] > MARGIN).reshape(-1, spp).all(1)

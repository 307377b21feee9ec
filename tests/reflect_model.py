"""Float64 NumPy model of reflected paths (test helper, no GPU): the path loop of volume.py:179-272
with transmission_only = False and a non-scattering medium, through the container, the black
occluders and the inserts' triangles (the formulas of tvam_insert_next<REFLECT>,
drtvam_amd/csrc/tvam_insert.h, in exact-arithmetic form), and the scenes of the tests.  It is
insert_model.trace with the BSDF's first draw used:

    loop depth 0          the transmission is forced: weight (1 - F) eta_ti^2
    depth >= 1,           s1 = u[:, depth, 1] (the draws are roulette, s1, then the two of s2);
    dielectric surface    s1 <= F reflects, wo = d - 2 (d . n) n, weight 1; otherwise the refraction's
                          direction with weight eta_ti^2.  F = 1 (total internal reflection) reflects.
    index-matched tube    passes the ray on; a black occluder ends the path after its deposit

After either branch, as insert_model: e^{-sigma_t t} after a medium segment, the spawn offset on the
side of wo, the medium flag (kind == MEDIUM and n . wo < 0, or kind == INSERT and n . wo > 0),
++depth.  Roulette is drawn in every iteration and acts when depth > rr_depth.

The per-ray margin is insert_model's (geometry decisions, the roulette's u < q) plus the new
decision, |s1 - F|, and |cos_theta_t^2| at every sampled interface: F has a square-root singularity
at the critical angle, where an fp32 rounding of cos_theta_t^2 moves it by far more than an ulp."""
import numpy as np

import insert_model as im
from double_vial_model import MARGIN, RAY_EPS, _fresnel, _tube, compare_segments  # noqa: F401
from insert_model import _tri_hits, tri_normals
from traced_vial_model import _box

# strong contrasts: at the documented IORs F is about 0.2 % at normal incidence and a test would be vacuous
IOR_GLASS, IOR_MEDIUM, INT_IOR, EXT_IOR = 1.9, 1.2, 2.2, 1.2


def trace(o, d, cont, tris, tri_eta, sigma_t, max_depth, u, rr_depth, black=None, max_segments=None, flaw=None):
    """insert_model.trace with reflections (see the module text); u [n, max_depth, 4] is required.
      flaw   a planted error (the tests of the checker): 'lt' (s1 < F in place of s1 <= F), 'keepT' ((1 - F) kept
             on the refracted branch), 'spawn' (the reflected ray's spawn offset on the wrong side)
    Returns insert_model.trace's dict, and
      refl      [n] sampled reflections of the path
      refl_seg  [n] the path has a sampled reflection followed by a medium segment"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    u = np.asarray(u, np.float64)
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    tri_eta = np.asarray(tri_eta, np.float64)
    black = np.zeros((0, 3, 3)) if black is None else np.asarray(black, np.float64).reshape(-1, 3, 3)
    nrm_ins = tri_normals(tris) if len(tris) else np.zeros((0, 3))
    nrm_blk = tri_normals(black) if len(black) else np.zeros((0, 3))
    glass = "r_ext" in cont
    square = bool(cont.get("square", False))
    scale = cont["r_ext"] if glass else cont["r"]
    max_segments = max_depth if max_segments is None else max_segments
    n = o.shape[0]
    p, v = o.copy(), d.copy()
    att = np.ones(n)
    alive = np.ones(n, bool)
    in_medium = np.zeros(n, bool)
    last = np.full(n, -1)
    last_tri = np.full(n, -1)
    nseg = np.zeros(n, np.int64)
    segs = np.zeros((n, max_segments, 8))
    iters = np.full((n, max_segments), -1)
    margin = np.full(n, np.inf)
    ct2min = np.ones(n)
    ct2seg = np.ones((n, max_segments))
    ends = np.full(n, "depth", dtype=object)
    nrefl = np.zeros(n, np.int64)
    refl_seg = np.zeros(n, bool)
    for depth in range(max_depth):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        if depth > rr_depth:
            q = np.minimum(0.99, att[idx])
            ur = u[idx, depth, 0]
            margin[idx] = np.minimum(margin[idx], np.abs(ur - q))
            keep = ur < q
            att[idx] = att[idx] / q
            ends[idx[~keep]] = "rr"
            alive[idx[~keep]] = False
            idx = idx[keep]
        pi, vi = p[idx], v[idx]
        k = idx.size
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
        dep = in_medium[idx]
        di, ks = idx[dep], nseg[idx[dep]]
        fits = ks < max_segments
        dj, kj = di[fits], ks[fits]
        segs[dj, kj, 0:3], segs[dj, kj, 3], segs[dj, kj, 4:7], segs[dj, kj, 7] = p[dj], t[dep][fits], v[dj], att[dj]
        iters[dj, kj] = depth
        ct2seg[dj, kj] = np.minimum(ct2min[dj], (cos_i * cos_i)[dep][fits])
        nseg[di] += 1
        refl_seg[di] |= nrefl[di] > 0
        ends[idx[isb]] = "black"
        alive[idx[isb]] = False
        go = ~isb
        idx, t, kind, sm, dep, h, nn, isi, cos_i = (idx[go], t[go], kind[go], sm[go], dep[go], h[go], nn[go], isi[go],
                                                    cos_i[go])
        if glass:
            eta = np.where(kind == 1, cont["eta_int"], cont["eta_ext"])
        else:
            eta = np.ones(idx.size)
        eta = np.where(isi, tri_eta[np.maximum(sm, 0)], eta) if len(tri_eta) else eta
        F, cos_t, eta_ti, ct2 = _fresnel(cos_i, eta)
        T = 1.0 - F
        diel = glass | isi  # (the index-matched tube's null BSDF samples nothing)
        s1 = u[idx, depth, 1]
        if depth == 0:
            refl = np.zeros(idx.size, bool)
            margin[idx] = np.minimum(margin[idx], np.where(ct2 < 0.0, -ct2, T))
            wgt = T * eta_ti * eta_ti
        else:
            refl = diel & ((s1 < F) if flaw == "lt" else (s1 <= F))
            margin[idx] = np.minimum(margin[idx], np.where(diel, np.minimum(np.abs(s1 - F), np.abs(ct2)), np.inf))
            wgt = np.where(refl, 1.0, eta_ti * eta_ti * (T if flaw == "keepT" else 1.0))
        # conditioning (compare_segments): the refraction's through cos_theta_t^2, both branches' through cos_i^2
        ct2min[idx] = np.minimum(ct2min[idx], np.where(refl, cos_i * cos_i, np.minimum(np.abs(ct2), cos_i * cos_i)))
        wo_t = eta_ti[:, None] * v[idx] + (eta_ti * cos_i + cos_t)[:, None] * nn
        wo_r = v[idx] + (2.0 * cos_i)[:, None] * nn
        wo = np.where(refl[:, None], wo_r, wo_t)
        att[idx] *= wgt
        att[idx] *= np.where(dep, np.exp(-sigma_t * t), 1.0)
        nwo = np.sum(nn * wo, -1)
        side = np.where(nwo < 0.0, -1.0, 1.0)
        if flaw == "spawn":
            side = np.where(refl, -side, side)
        mag = (1.0 + np.max(np.abs(h), -1)) * RAY_EPS * side
        p[idx] = h + mag[:, None] * nn
        v[idx] = wo
        in_medium[idx] = ((kind == 1) & (nwo < 0.0)) | (isi & (nwo > 0.0))
        last[idx] = np.where(isi, -1, kind)
        last_tri[idx] = np.where(isi, sm, -1)
        nrefl[idx] += refl
        dead = ~(wgt > 0.0)  # (depth 0 alone: a first surface met under total internal reflection)
        ends[idx[dead]] = "tir"
        alive[idx[dead]] = False
    return dict(n=nseg, segs=segs, iters=iters, margin=margin, ct2=ct2seg, ends=ends, refl=nrefl, refl_seg=refl_seg)


# --------------------------------------------------------------------------- scenes
def reflect_config(vial="cylindrical", kind="collimated", regular=True, inserts=(), black=False, paths=None,
                   ior_glass=IOR_GLASS, ior_medium=IOR_MEDIUM, int_ior=INT_IOR, ext_ior=EXT_IOR, **kw):
    """insert_model.insert_config with transmission_only = false and the strong IOR contrasts above."""
    kw.setdefault("transmission_only", False)
    cfg = im.insert_config(vial, kind, regular, inserts, black, paths, int_ior=int_ior, ext_ior=ext_ior, **kw)
    cfg["vial"]["medium"]["ior"] = ior_medium
    if vial != "index_matched":
        cfg["vial"]["ior"] = ior_glass
    return cfg


def reflect_scene(dirpath, vial="cylindrical", kind="collimated", regular=True, inserts=(), black=False, **kw):
    from drtvam_amd.configs import desc_from_config
    d = desc_from_config(reflect_config(vial, kind, regular, inserts, black, im.write_meshes(dirpath), **kw))
    assert tuple(d.film_res) == (40, 36, 20), tuple(d.film_res)
    return d


def trace_desc(desc, o, d, u, **kw):
    tris, eta, black = im.inserts_of(desc)
    return trace(o, d, im.container_of(desc), tris, eta, float(np.float32(desc.sigma_t)), int(desc.max_depth), u,
                 int(desc.rr_depth), black=black, **kw)


_MODEL = {}


def scene_model(dirpath, vial, kind, regular, spp=3, seed=3, **kw):
    """The model's rays, draws and segments of reflect_scene(...), dense set (computed once; callers do not
    change it).  The draws are float32 values, as the kernels' generator and the host walk take them."""
    key = (vial, kind, regular, spp, seed, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _MODEL:
        import projector_model as pm
        d = reflect_scene(dirpath, vial, kind, regular, **kw)
        pix = pm.dense_pixels(d)
        spp_ = 1 if regular else spp
        m = pm.model_rays(d, pix, np.arange(pix.size), spp_, seed)
        u = im.path_draws(d, np.arange(pix.size), spp_, seed)
        _MODEL[key] = dict(desc=d, spp=spp_, o=m["o"], d=m["d"], u=u, **trace_desc(d, m["o"], m["d"], u))
    return _MODEL[key]


# The scenes of the GPU tests (tests/test_gpu_reflect.py), which the CPU tests walk on the host too:
# name -> (vial, kind, regular, keywords).  3 vials x 3 projectors, index matched only with inserts.
SCENES = {
    "cyl-collimated": ("cylindrical", "collimated", True, dict()),                                   # no hierarchy
    "cyl-telecentric-box": ("cylindrical", "telecentric", False, dict(inserts=("box",))),            # brute force, LDS
    "cyl-lens-fine": ("cylindrical", "lens", False, dict(inserts=("fine",))),                        # hierarchy in global memory
    "square-collimated-u-black": ("square", "collimated", True, dict(inserts=("u",), black=True)),    # hierarchy in LDS
    "square-telecentric": ("square", "telecentric", False, dict()),                                  # no hierarchy
    "square-lens-prism-u-black-rr": ("square", "lens", False,                                        # roulette acts
                                     dict(inserts=("prism", "u"), black=True, max_depth=16, rr_depth=2, extinction=0.2)),
    "im-collimated-prism-u": ("index_matched", "collimated", True, dict(inserts=("prism", "u"))),
    "im-telecentric-prism-u-black": ("index_matched", "telecentric", False, dict(inserts=("prism", "u"), black=True)),
    "im-lens-u": ("index_matched", "lens", False, dict(inserts=("u",))),
}
# the dose / gradient scenes: one per hierarchy mode, a black occluder, the roulette
FILM_SCENES = ("cyl-collimated", "cyl-lens-fine", "square-collimated-u-black", "square-lens-prism-u-black-rr")
SPP, SEED = 3, 3


def model_of(dirpath, name):
    vial, kind, regular, kw = SCENES[name]
    return scene_model(dirpath, vial, kind, regular, SPP, SEED, **kw)


def film_keep(m):
    return im.film_keep(m)

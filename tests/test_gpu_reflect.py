"""Reflected paths (transmission_only = 0) on the GPU: tvam_plan_create_reflect's plans run
tvam_ray3d.hip's kernels over WalkReflect (tvam_insert_next<REFLECT>): at every dielectric surface
after a path's first, the ray's own generator picks reflection or refraction.

The oracle knows no reflections, so the path is pinned by the float64 model of tests/reflect_model.py
(which tests/test_reflect.py pins to closed forms and to the host walk on the CPU):
  1. the device export (Projection.insert_segments) against the model on every ray whose decisions
     the model finds at least 1e-4 from flipping, the s1-versus-F choice among them;
  2. dose and gradient against the oracle's DDA (oracle.dda_ray) marched over the model's segments;
  3. the adjoint as the forward's transpose, angle shards, the sparse set, the ray-generation options;
  4. the anchor to the oracle itself: with every IOR equal no path reflects, and the plan gives the
     oracle's forward, adjoint and exact visit count of the transmission-only scene.
Scenes are insert_model.insert_scene's size: DMD 24 x 20, 6 angles, film 40 x 36 x 20; 2880 rays at
spp 1 and 8640 at spp 3, no multiple of 256."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config
from drtvam_amd.engine import Projection

import insert_model as im
import projector_model as pm
import reflect_model as rm

RTOL = 1e-4  # the project's parity bar
DEV = "cuda:0"
SPP, SEED = rm.SPP, rm.SEED
# section 4l's export-vs-model bounds (tests/test_gpu_inserts.py), times the segment's condition number
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("reflect_meshes")
    im.write_meshes(d)
    return d


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def film_shape(d):
    rx, ry, rz = d.film_res
    return (rz, ry, rx)


# --------------------------------------------------------------------------- 1. the export
@pytest.mark.parametrize("name", list(rm.SCENES))
def test_segments_match_model(meshdir, name):
    """3 vials x 3 projectors (index matched only with inserts), with and without inserts, a black occluder, the
    hierarchy in LDS, in global memory and absent, and max_depth 16 / rr_depth 2 with the roulette acting."""
    m = rm.model_of(meshdir, name)
    d, spp = m["desc"], m["spp"]
    S = m["segs"].shape[1]
    n = d.n_patterns * d.crop_y * d.crop_x
    assert d.reflected and (n * spp) % 256 != 0
    proj = Projection(d, DEV)
    assert proj.cone and not proj.planar and proj.fwd_chunk == 0
    segs, nseg = proj.insert_segments(None, None, spp, SEED, S)
    rays = proj.rays(None, None, spp, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    segs, nseg = segs.cpu().numpy().astype(np.float64), nseg.cpu().numpy()
    assert segs.shape == (n * spp, S, 8) and nseg.shape == (n * spp,) and rays.shape == (n * spp, 16)
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    assert np.abs(rays[:, 0:3] - m["o"]).max() <= tol_o and np.abs(rays[:, 3:6] - m["d"]).max() <= tol_d
    hit = rays[:, 6] != 0.0  # tvam_plan_rays serves the first segment
    assert np.array_equal(hit, nseg > 0)
    assert np.array_equal(rays[hit, 7:11], segs[hit, 0, 0:4]) and np.array_equal(rays[hit, 11:15], segs[hit, 0, 4:8])
    ok = m["margin"] > rm.MARGIN
    assert np.array_equal(nseg[ok], m["n"][ok]) and nseg.max() <= S
    w = float(pm.ray_weight(d, n, spp))
    att = segs.copy()
    att[:, :, 7] /= w
    r = rm.compare_segments(att, m)
    hist = np.bincount(m["n"][ok], minlength=4)
    ends = dict(zip(*np.unique(m["ends"][ok], return_counts=True)))
    print(f"{name}: rays {len(segs)} segments per ray {hist.tolist()} ends {ends} reflected-then-deposited "
          f"{int(m['refl_seg'][ok].sum())} compared {r['compared']} below margin {r['low']:.4f} |do2| {r['e_o']:.3e} "
          f"|dmaxt| {r['e_t']:.3e} (tol {TOL_O:.3e}) |dd2| {r['e_d']:.3e} |dw|/w {r['e_w']:.3e} (tol {TOL_D:.3e}), "
          f"each / kappa")
    assert r["low"] <= 0.01 and m["refl_seg"][ok].sum() >= 50 and hist[3:].sum() > 0
    assert r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D
    if "rr_depth" in rm.SCENES[name][3]:
        assert ends.get("rr", 0) > 0
    # the host walk is the kernels' own code: on the device's own rays it gives the device's segments
    if m["spp"] == 1 and d.projector_type == _abi.PROJECTOR_COLLIMATED:
        hs, hn = _abi.reflect_segments(d, rays[:, 0:3], rays[:, 3:6], m["u"], S)
        same = hn == nseg
        assert same.mean() >= 0.99 and np.allclose(hs[same][:, :, 0:7], segs[same][:, :, 0:7], rtol=0, atol=TOL_O)


# --------------------------------------------------------------------------- 2. dose and gradient
_REF = {}


def reference(oracle, meshdir, name):
    """Per scene, computed once: the oracle's DDA over the model's segments (fp32 rows, as the kernels' segments
    are), weights = ray weight x attenuation x inv_vol.  Pixels with a ray below the margin are left out: their
    pattern values are 0 (the forward skips them) and `keep` marks the gradient entries that are compared."""
    if name in _REF:
        return _REF[name]
    m = rm.model_of(meshdir, name)
    d, spp = m["desc"], m["spp"]
    n = d.n_patterns * d.crop_y * d.crop_x
    keep = rm.film_keep(m)
    assert keep.shape == (n,) and (~keep).mean() <= 0.01 * spp
    rng = np.random.default_rng(11)
    pat = rng.uniform(0.02, 0.1, n).astype(np.float32) * keep
    G = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    w0 = float(pm.ray_weight(d, n, spp)) * float(pm.inv_vol(d))
    dose = np.zeros(film_shape(d), np.float64)
    refl = np.zeros(film_shape(d), np.float64)  # the part deposited after a sampled reflection
    grad = np.zeros(n, np.float64)
    segs = m["segs"].astype(np.float32)
    seen = np.zeros(len(segs), bool)
    for i in np.nonzero(np.repeat(keep, spp))[0]:
        for s in range(int(m["n"][i])):
            sg = segs[i, s]
            film, _ = oracle.dda_ray(d, sg[0:3], sg[4:7], float(sg[3]))
            w = float(sg[7]) * w0
            dose += (w * float(pat[i // spp])) * film
            if m["refl_seg"][i] and s > 0:
                refl += (w * float(pat[i // spp])) * film
            grad[i // spp] += w * float(np.vdot(film, G))
    _REF[name] = dict(desc=d, spp=spp, n=n, pat=pat, G=G, dose=dose, refl=refl, grad=grad, keep=keep, m=m)
    return _REF[name]


@pytest.mark.parametrize("name", rm.FILM_SCENES)
def test_dose_and_gradient_match_oracle_dda_over_model_segments(oracle, meshdir, name):
    ref = reference(oracle, meshdir, name)
    proj = Projection(ref["desc"], DEV)
    dose = proj.forward(dev(ref["pat"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
    grad = proj.adjoint(dev(ref["G"]), ref["n"], None, ref["spp"], SEED).cpu().numpy()
    proj.close()
    e_f = rel_l2(dose, ref["dose"])
    e_a = rel_l2(grad[ref["keep"]], ref["grad"][ref["keep"]])
    share = float(np.linalg.norm(ref["refl"]) / np.linalg.norm(ref["dose"]))
    print(f"{name}: dose rel-L2 {e_f:.3e} gradient rel-L2 {e_a:.3e}; later segments of reflected paths carry "
          f"{share:.4f} of the dose norm; pixels left out {int((~ref['keep']).sum())} of {ref['n']}")
    assert np.linalg.norm(ref["dose"]) > 0 and share > 0.0 and np.linalg.norm(ref["grad"]) > 0
    assert e_f < RTOL and e_a < RTOL


# --------------------------------------------------------------------------- 3. properties
def test_adjoint_is_transpose(meshdir):
    d = rm.reflect_scene(meshdir, "cylindrical", "telecentric", False, inserts=("prism", "u"), black=True)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, n).astype(np.float32)
    y = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(d, DEV)
    Ax = proj.forward(dev(x), None, SPP, SEED).cpu().numpy()[..., 0].astype(np.float64)
    Aty = proj.adjoint(dev(y), n, None, SPP, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    lhs, rhs = float(np.vdot(Ax, y)), float(np.vdot(x, Aty))
    print(f"<Ax, y> {lhs:.9e} <x, Aty> {rhs:.9e}")
    assert lhs > 0 and abs(lhs - rhs) <= RTOL * abs(lhs)


def test_angle_shards_sum_to_full_render(meshdir):
    d = rm.reflect_scene(meshdir, "square", "lens", False, inserts=("u",), black=True, max_depth=16, rr_depth=2,
                         extinction=0.2)
    per = d.crop_y * d.crop_x
    n = d.n_patterns * per
    rng = np.random.default_rng(8)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = dev(rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32))
    full = Projection(d, DEV)
    dose = full.forward(dev(pat), None, SPP, SEED).cpu().numpy().astype(np.float64)
    grad = full.adjoint(G, n, None, SPP, SEED).cpu().numpy()
    full.close()
    total, parts = np.zeros_like(dose), []
    for a0, a1 in ((0, 2), (2, 6)):
        ds = d.copy()
        ds.angle_begin, ds.angle_end = a0, a1
        ds.active_base, ds.active_total = a0 * per, n
        sh = Projection(ds, DEV)
        total += sh.forward(dev(pat[a0 * per:a1 * per]), None, SPP, SEED).cpu().numpy()
        parts.append(sh.adjoint(G, (a1 - a0) * per, None, SPP, SEED).cpu().numpy())
        sh.close()
    assert np.linalg.norm(dose) > 0
    assert rel_l2(total, dose) < RTOL
    assert rel_l2(np.concatenate(parts), grad) < RTOL


def test_sparse_set_agrees_with_dense(meshdir):
    """A ray's draws come from its sampler stream, which is its position in the active set: the sparse set that
    lists every pixel in dense order has the dense set's streams, and a lit subset of it gives the dense forward
    of the same patterns and the dense gradient's entries."""
    d = rm.reflect_scene(meshdir, "square", "collimated", True, inserts=("prism", "u"), black=True)
    pix = pm.dense_pixels(d)
    n = pix.size
    rng = np.random.default_rng(3)
    sel = np.sort(rng.choice(n, n // 3, replace=False))
    pat = np.zeros(n, np.float32)
    pat[sel] = rng.uniform(0.01, 0.1, sel.size).astype(np.float32)
    G = dev(rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32))
    proj = Projection(d, DEV)
    dense = proj.forward(dev(pat), None, 1, SEED).cpu().numpy().astype(np.float64)
    gd = proj.adjoint(G, n, None, 1, SEED).cpu().numpy()
    proj.close()
    ds = d.copy()
    ds.active_base, ds.active_total = 0, n
    sp = Projection(ds, DEV)
    allpix = dev(pix.astype(np.int32), torch.int32)
    sparse = sp.forward(dev(pat), allpix, 1, SEED).cpu().numpy()
    gs = sp.adjoint(G, n, allpix, 1, SEED).cpu().numpy()
    sp.close()
    assert np.linalg.norm(dense) > 0 and rel_l2(sparse, dense) < RTOL
    assert np.array_equal(gs, gd)


def test_crop_clockwise_sample_time_and_sparse_set(meshdir):
    """Every ray-generation option at once: every third pixel of a cropped DMD, clockwise, a time sample."""
    d = rm.reflect_scene(meshdir, "cylindrical", "telecentric", False, inserts=("u",), black=True)
    d.crop_x, d.crop_y, d.crop_offset_x, d.crop_offset_y = 19, 14, 3, 2
    d.clockwise, d.sample_time = 1, 1
    sub = np.ascontiguousarray(pm.dense_pixels(d)[::3]).astype(np.int32)
    d.active_base, d.active_total = 0, sub.size
    S = int(d.max_depth)
    proj = Projection(d, DEV)
    segs, nseg = proj.insert_segments(None, dev(sub, torch.int32), 2, SEED, S)
    proj.close()
    segs, nseg = segs.cpu().numpy().astype(np.float64), nseg.cpu().numpy()
    r = pm.model_rays(d, sub, np.arange(sub.size), 2, SEED)
    u = im.path_draws(d, np.arange(sub.size), 2, SEED)
    m = rm.trace_desc(d, r["o"], r["d"], u)
    ok = m["margin"] > rm.MARGIN
    assert np.array_equal(nseg[ok], m["n"][ok]) and (m["n"] >= 2).any() and m["refl_seg"].sum() > 0
    segs[:, :, 7] /= float(pm.ray_weight(d, sub.size, 2))
    c = rm.compare_segments(segs, m)
    assert c["low"] <= 0.01 and c["e_o"] <= TOL_O and c["e_t"] <= TOL_O and c["e_d"] <= TOL_D and c["e_w"] <= TOL_D


# --------------------------------------------------------------------------- 4. the anchor
@pytest.mark.parametrize("vial", ["cylindrical", "square"])
def test_equal_iors_match_oracle_transmission_only_scene(oracle, meshdir, vial):
    """Glass and resin of the air's IOR: F = 0 at every interface, no path reflects, and the plan gives the oracle's
    forward, adjoint and visit count of the same scene with transmission_only = true."""
    n_air = float(np.float32(1.000277))
    kw = dict(ior_glass=n_air, ior_medium=n_air)
    d = rm.reflect_scene(meshdir, vial, "collimated", True, **kw)
    dc = rm.reflect_scene(meshdir, vial, "collimated", True, transmission_only=True, **kw)
    assert d.reflected and not dc.reflected
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(0)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(-1.0, 1.0, film_shape(d)).astype(np.float32)
    want, visits = oracle.forward(dc, pat, spp=1, seed=5, nthreads=8)
    gref, _ = oracle.adjoint(dc, G, spp=1, seed=5, nthreads=8)
    proj = Projection(d, DEV)
    dose = proj.forward(dev(pat), None, 1, 5).cpu().numpy()[..., 0]
    grad = proj.adjoint(dev(G), n, None, 1, 5).cpu().numpy()
    got_visits = proj.count_visits(1, 5)
    _, nseg = proj.insert_segments(None, None, 1, 5, 2)
    proj.close()
    e_f, e_a = rel_l2(dose, want), rel_l2(grad, gref)
    print(f"{vial}: dose rel-L2 {e_f:.3e} gradient rel-L2 {e_a:.3e} visits {got_visits} (oracle {visits})")
    assert int(nseg.max()) == 1
    assert np.linalg.norm(want) > 0 and e_f <= RTOL and e_a <= RTOL
    assert got_visits == visits


# --------------------------------------------------------------------------- refusals on the device
def test_other_calls_serve_or_refuse_the_plan_by_name(meshdir):
    d = rm.reflect_scene(meshdir, "cylindrical", "collimated", True)
    proj = Projection(d, DEV)
    n = d.n_patterns * d.crop_y * d.crop_x
    pat = torch.zeros(n, device=DEV)
    G = torch.zeros(film_shape(d) + (1,), device=DEV)
    with pytest.raises(ValueError, match="transmission_only = 0 with filter_radon"):
        proj.radon(np.zeros((0, 3, 3), np.float32))
    with pytest.raises(ValueError, match=r"tvam_forward_dsigma: a plan with reflected paths \(transmission_only = 0\)"):
        proj.forward_dsigma(pat, None, 1, 0)
    with pytest.raises(ValueError, match="tvam_adjoint_dsigma: a plan with reflected paths"):
        proj.adjoint_dsigma(pat, G, None, 1, 0)
    with pytest.raises(ValueError, match="tvam_forward_dprojector: a plan with reflected paths"):
        proj.forward_dprojector("distance", pat, None, 1, 0)
    with pytest.raises(ValueError, match="tvam_forward_slices: reflected paths"):
        proj.forward_slices(pat, None, 1, 0, 0, 4, G.clone())
    with pytest.raises(ValueError, match="tvam_adjoint_slices: reflected paths"):
        proj.adjoint_slices(G, n, 0, 4, 0, 2, pat.clone())
    with pytest.raises(ValueError, match="tvam_plan_segments: a plan with reflected paths"):
        proj.segments(None, None, 1, 0)
    # the corner filter reads the projector and the vial alone: the transmission-only plan's answer
    keep, hits = proj.corner(2.9, 0.3, hits=True)
    plain = Projection(rm.reflect_scene(meshdir, "cylindrical", "collimated", True, transmission_only=True), DEV)
    keep0, hits0 = plain.corner(2.9, 0.3, hits=True)
    assert torch.equal(keep, keep0) and torch.equal(hits, hits0) and int(keep.sum()) > 0
    assert plain.planar and proj.count_visits(1, 0) > 0
    plain.close()
    proj.close()

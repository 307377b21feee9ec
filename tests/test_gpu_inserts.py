"""Dielectric occluders on the GPU (tvam_insert.h, tvam_ray3d.hip): every ray walked through the
container, the black occluders and the inserts' triangles, any number of medium segments per ray.

The oracle knows only black occluders, so the path is pinned by the float64 model of
tests/insert_model.py:
  1. tvam_plan_insert_segments (Projection.insert_segments) against the model on every ray whose
     decisions the model finds at least 1e-4 from flipping (at most 1 % are not:
     tests/test_insert_model.py checks that on the CPU);
  2. dose and gradient against the oracle's DDA (oracle.dda_ray) marched over the model's segments,
     with the rays below the margin left out (their pixels carry pattern 0, their gradient entries are
     not compared);
  3. anchors to the oracle itself: an insert no lit ray meets gives the oracle's forward, adjoint and
     visit count of the scene without it; a black occluder behind an insert cuts the model's rays there.
Scenes (insert_model.insert_scene) are at the size of projector_model.projector_scene: DMD 24 x 20,
6 angles, film 40 x 36 x 20; 2880 rays at spp 1 and 8640 at spp 3, no multiple of 256."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config
from drtvam_amd.engine import Projection

import insert_model as im
import projector_model as pm

RTOL = 1e-4  # the project's parity bar
DEV = "cuda:0"
SPP, SEED = 3, 3
# tests/test_gpu_mesh_vial.py's export-vs-model bounds (times the segment's condition number,
# double_vial_model.compare_segments)
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("insert_meshes")
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
SCENES = [(v, k, reg) for v in ("index_matched", "cylindrical", "square")
          for (k, reg) in (("collimated", True), ("telecentric", False), ("lens", False))]
EXTRA = [
    ("index_matched", "collimated", True, dict(inserts=("box",))),                    # brute force
    ("cylindrical", "lens", False, dict(inserts=("fine",))),                          # hierarchy in global memory
    ("square", "lens", False, dict(inserts=("prism", "u"), black=True, max_depth=16, rr_depth=2, extinction=0.2)),  # roulette acts
    ("square", "telecentric", False, dict(inserts=("u",), max_depth=4)),              # ended inside the piece
]


def check_segments(meshdir, vial, kind, regular, kw):
    m = im.scene_model(meshdir, vial, kind, regular, SPP, SEED, **kw)
    d, spp = m["desc"], m["spp"]
    n = d.n_patterns * d.crop_y * d.crop_x
    proj = Projection(d, DEV)
    assert proj.cone and not proj.planar and proj.fwd_chunk == 0
    segs, nseg = proj.insert_segments(None, None, spp, SEED, im.MAX_SEGMENTS)
    rays = proj.rays(None, None, spp, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    segs, nseg = segs.cpu().numpy().astype(np.float64), nseg.cpu().numpy()
    assert segs.shape == (n * spp, im.MAX_SEGMENTS, 8) and nseg.shape == (n * spp,) and rays.shape == (n * spp, 16)
    assert (n * spp) % 256 != 0
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    assert np.abs(rays[:, 0:3] - m["o"]).max() <= tol_o and np.abs(rays[:, 3:6] - m["d"]).max() <= tol_d
    # tvam_plan_rays serves the first segment in the traced plans' layout
    hit = rays[:, 6] != 0.0
    assert np.array_equal(hit, nseg > 0)
    assert np.array_equal(rays[hit, 7:11], segs[hit, 0, 0:4]) and np.array_equal(rays[hit, 11:15], segs[hit, 0, 4:8])
    assert not rays[~hit, 7:11].any() and np.array_equal(rays[~hit, 11:14], rays[~hit, 3:6])
    w = float(pm.ray_weight(d, n, spp))
    assert np.all(rays[~hit, 14] == w)
    ok = m["margin"] > im.MARGIN
    assert np.array_equal(nseg[ok], m["n"][ok]) and nseg.max() <= im.MAX_SEGMENTS
    att = segs.copy()
    att[:, :, 7] /= w
    r = im.compare_segments(att, m)
    hist = np.bincount(m["n"][ok], minlength=4)
    ends = dict(zip(*np.unique(m["ends"][ok], return_counts=True)))
    print(f"{vial} {kind} {kw}: rays {len(segs)} segments per ray {hist.tolist()} ends {ends} compared {r['compared']} "
          f"below margin {r['low']:.4f} |do2| {r['e_o']:.3e} |dmaxt| {r['e_t']:.3e} (tol {TOL_O:.3e}) |dd2| {r['e_d']:.3e} "
          f"|dw|/w {r['e_w']:.3e} (tol {TOL_D:.3e}), each / kappa; largest kappa_d {r['kappa_d']:.1f} kappa_w "
          f"{r['kappa_w']:.1f}")
    assert r["low"] <= 0.01
    assert r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D
    present = segs[:, :, 3] != 0.0
    assert np.abs(np.linalg.norm(segs[present][:, 4:7], axis=1) - 1.0).max() <= 16 * tol_d
    return m, hist, ends


@pytest.mark.parametrize("vial,kind,regular", SCENES, ids=[f"{v}-{k}" for v, k, _ in SCENES])
def test_segments_match_model(meshdir, vial, kind, regular):
    """Each projector behind each vial, spp 1 (regular) and 3 (jittered): the tilted prism, the U-piece and a
    black occluder; rays of 1, 2, 3 and more segments."""
    m, hist, ends = check_segments(meshdir, vial, kind, regular, dict(inserts=("prism", "u"), black=True))
    assert hist[1] > 0 and hist[2] > 0 and hist[3] > 0 and ends.get("black", 0) > 0 and ends.get("tir", 0) > 0


@pytest.mark.parametrize("vial,kind,regular,kw", EXTRA, ids=["brute", "global", "roulette", "max_depth"])
def test_segments_match_model_more(meshdir, vial, kind, regular, kw):
    m, hist, ends = check_segments(meshdir, vial, kind, regular, kw)
    if "rr_depth" in kw:
        assert m["u"] is not None and ends.get("rr", 0) > 0
    if kw.get("max_depth") == 4:
        assert ends.get("depth", 0) > 0 and hist[2] == 0


def test_crop_clockwise_sample_time_and_sparse_set(meshdir):
    """Every ray-generation option at once: every third pixel of a cropped DMD, clockwise, a time sample."""
    d = im.insert_scene(meshdir, "cylindrical", "telecentric", False, inserts=("u",), black=True)
    d.crop_x, d.crop_y, d.crop_offset_x, d.crop_offset_y = 19, 14, 3, 2
    d.clockwise, d.sample_time = 1, 1
    sub = np.ascontiguousarray(pm.dense_pixels(d)[::3]).astype(np.int32)
    d.active_base, d.active_total = 0, sub.size
    proj = Projection(d, DEV)
    segs, nseg = proj.insert_segments(None, dev(sub, torch.int32), 2, SEED, im.MAX_SEGMENTS)
    proj.close()
    segs, nseg = segs.cpu().numpy().astype(np.float64), nseg.cpu().numpy()
    r = pm.model_rays(d, sub, np.arange(sub.size), 2, SEED)
    m = im.trace_desc(d, r["o"], r["d"])
    ok = m["margin"] > im.MARGIN
    assert np.array_equal(nseg[ok], m["n"][ok]) and (m["n"] >= 2).any()
    segs[:, :, 7] /= float(pm.ray_weight(d, sub.size, 2))
    c = im.compare_segments(segs, m)
    assert c["low"] <= 0.01 and c["e_o"] <= TOL_O and c["e_t"] <= TOL_O and c["e_d"] <= TOL_D and c["e_w"] <= TOL_D


# --------------------------------------------------------------------------- 2. dose and gradient
VARIANTS = im.FILM_VARIANTS  # a full pattern set each: brute force / LDS / global hierarchies, a black occluder, roulette
_REF = {}


def reference(oracle, meshdir, name):
    """Per variant, computed once: the model's segments and the oracle's DDA over them (fp32 rows, as the
    kernels' segments are), weights = ray weight x attenuation x inv_vol.  Rays below the margin are left
    out: their pixels' pattern values are 0 (the forward skips them) and `keep` marks the gradient entries
    that are compared."""
    if name in _REF:
        return _REF[name]
    vial, kind, regular, kw = VARIANTS[name]
    m = im.scene_model(meshdir, vial, kind, regular, im.FILM_SPP, im.FILM_SEED, **kw)
    d, spp = m["desc"], m["spp"]
    n = d.n_patterns * d.crop_y * d.crop_x
    keep = im.film_keep(m)
    assert keep.shape == (n,) and (~keep).mean() <= 0.01  # at most 1 % of the rays (spp per pixel left out)
    rng = np.random.default_rng(11)
    pat = rng.uniform(0.02, 0.1, n).astype(np.float32) * keep
    G = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    w0 = float(pm.ray_weight(d, n, spp)) * float(pm.inv_vol(d))
    dose = np.zeros(film_shape(d), np.float64)
    later = np.zeros(film_shape(d), np.float64)  # the part from second and later segments
    grad = np.zeros(n, np.float64)
    visits = 0
    segs = m["segs"].astype(np.float32)
    for i in np.nonzero(np.repeat(keep, spp))[0]:
        for s in range(min(int(m["n"][i]), im.MAX_SEGMENTS)):
            sg = segs[i, s]
            film, v = oracle.dda_ray(d, sg[0:3], sg[4:7], float(sg[3]))
            visits += v
            w = float(sg[7]) * w0
            dose += (w * float(pat[i // spp])) * film
            if s > 0:
                later += (w * float(pat[i // spp])) * film
            grad[i // spp] += w * float(np.vdot(film, G))
    assert m["n"].max() <= im.MAX_SEGMENTS
    _REF[name] = dict(desc=d, spp=spp, n=n, pat=pat, G=G, dose=dose, later=later, grad=grad, keep=keep, visits=visits, m=m)
    return _REF[name]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_dose_and_gradient_match_oracle_dda_over_model_segments(oracle, meshdir, name):
    ref = reference(oracle, meshdir, name)
    proj = Projection(ref["desc"], DEV)
    dose = proj.forward(dev(ref["pat"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
    grad = proj.adjoint(dev(ref["G"]), ref["n"], None, ref["spp"], SEED).cpu().numpy()
    proj.close()
    e_f = rel_l2(dose, ref["dose"])
    e_a = rel_l2(grad[ref["keep"]], ref["grad"][ref["keep"]])
    share = float(np.linalg.norm(ref["later"]) / np.linalg.norm(ref["dose"]))
    print(f"{name}: dose rel-L2 {e_f:.3e} gradient rel-L2 {e_a:.3e}; later segments carry {share:.3f} of the dose norm; "
          f"pixels left out {int((~ref['keep']).sum())} of {ref['n']}")
    assert np.linalg.norm(ref["dose"]) > 0 and share > 0.02 and np.linalg.norm(ref["grad"]) > 0
    assert e_f < RTOL and e_a < RTOL


def test_one_lit_pixel(oracle, meshdir):
    """A single pixel whose rays cross the U-piece: the dose is those rays' segments alone."""
    ref = reference(oracle, meshdir, "cyl-telecentric-u-black")
    d, spp, m = ref["desc"], ref["spp"], ref["m"]
    per_pixel = m["n"].reshape(ref["n"], spp)
    cand = np.nonzero(ref["keep"] & (per_pixel >= 2).all(1))[0]
    assert cand.size > 0
    px = int(cand[len(cand) // 2])
    pat = np.zeros(ref["n"], np.float32)
    pat[px] = 0.07
    w0 = float(pm.ray_weight(d, ref["n"], spp)) * float(pm.inv_vol(d))
    want = np.zeros(film_shape(d), np.float64)
    segs = m["segs"].astype(np.float32)
    for i in range(px * spp, (px + 1) * spp):
        for s in range(int(m["n"][i])):
            film, _ = oracle.dda_ray(d, segs[i, s, 0:3], segs[i, s, 4:7], float(segs[i, s, 3]))
            want += (float(segs[i, s, 7]) * w0 * 0.07) * film
    proj = Projection(d, DEV)
    dose = proj.forward(dev(pat), None, spp, SEED).cpu().numpy()[..., 0]
    G = np.zeros(film_shape(d), np.float32)
    G[want > 0] = 1.0
    grad = proj.adjoint(dev(G), ref["n"], None, spp, SEED).cpu().numpy()
    proj.close()
    e = rel_l2(dose, want)
    print(f"pixel {px}: dose rel-L2 {e:.3e}, lit voxels {int((want > 0).sum())}")
    assert e < RTOL and np.count_nonzero(dose) <= np.count_nonzero(want) + 8
    assert abs(float(grad[px]) * 0.07 / want.sum() - 1.0) < RTOL  # the pixel's own gradient entry: its dose per unit pattern


def test_visit_count(oracle, meshdir):
    """Regular sampling: count_visits equals the oracle's DDA over the plan's own exported segments exactly (the
    traced-vial tests' scheme), and, in a scene all of whose rays lie above the margin, the oracle's DDA over the
    model's segments exactly too (measured: 89595 visits on all three counts)."""
    ref = reference(oracle, meshdir, "im-collimated-box")
    d, m = ref["desc"], ref["m"]
    proj = Projection(d, DEV)
    got = proj.count_visits(1, SEED)
    segs, nseg = proj.insert_segments(None, None, 1, SEED, im.MAX_SEGMENTS)
    proj.close()
    segs, nseg = segs.cpu().numpy(), nseg.cpu().numpy()
    own = 0
    for i in range(len(segs)):
        for s in range(int(nseg[i])):
            own += oracle.dda_ray(d, segs[i, s, 0:3], segs[i, s, 4:7], float(segs[i, s, 3]))[1]
    model = 0
    ms = m["segs"].astype(np.float32)
    for i in range(len(ms)):
        for s in range(int(m["n"][i])):
            model += oracle.dda_ray(d, ms[i, s, 0:3], ms[i, s, 4:7], float(ms[i, s, 3]))[1]
    print(f"visits: kernel {got}, DDA over its own segments {own}, over the model's {model}")
    assert int((m["margin"] <= im.MARGIN).sum()) == 0  # no ray of this scene is left out
    assert got == own and got > 0
    assert got == model


# --------------------------------------------------------------------------- 3. anchors
@pytest.mark.parametrize("vial", ["cylindrical", "square", "index_matched"])
def test_missed_insert_matches_oracle_scene_without_it(oracle, meshdir, vial):
    """The 'far' insert sits above every lit ray: forward, adjoint and visit count are the oracle's of the
    same scene without inserts: the 3-D vial walk, the weights and the DDA of the new kernels against the
    oracle itself."""
    d = im.insert_scene(meshdir, vial, "collimated", True, inserts=("far",))
    dc = desc_from_config(im.insert_config(vial, "collimated", True, inserts=(), paths=im.write_meshes(meshdir)))
    assert len(d.inserts) == 1 and not dc.inserts
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


def test_black_occluder_behind_an_insert_cuts_the_rays(meshdir):
    """The same scene with and without the black piece: rays that meet it keep their segments up to it and
    lose what lies behind, as the model's do."""
    kw = dict(inserts=("prism", "u"))
    with_b = im.scene_model(meshdir, "index_matched", "collimated", True, SPP, SEED, black=True, **kw)
    without = im.scene_model(meshdir, "index_matched", "collimated", True, SPP, SEED, black=False, **kw)
    ok = (with_b["margin"] > im.MARGIN) & (without["margin"] > im.MARGIN)
    cut = ok & (with_b["ends"] == "black")
    behind = cut & (with_b["n"] >= 2)  # met the black piece after an insert
    assert behind.sum() > 0
    proj = Projection(with_b["desc"], DEV)
    segs, nseg = proj.insert_segments(None, None, 1, SEED, im.MAX_SEGMENTS)
    proj.close()
    segs, nseg = segs.cpu().numpy().astype(np.float64), nseg.cpu().numpy()
    proj = Projection(without["desc"], DEV)
    segs0, nseg0 = proj.insert_segments(None, None, 1, SEED, im.MAX_SEGMENTS)
    proj.close()
    segs0, nseg0 = segs0.cpu().numpy().astype(np.float64), nseg0.cpu().numpy()
    assert np.array_equal(nseg[ok], with_b["n"][ok]) and np.array_equal(nseg0[ok], without["n"][ok])
    for i in np.nonzero(behind)[0]:
        k = int(nseg[i])
        assert k <= nseg0[i]
        assert np.array_equal(segs[i, :k - 1], segs0[i, :k - 1])           # untouched in front of it
        assert np.array_equal(segs[i, k - 1, [0, 1, 2, 4, 5, 6, 7]], segs0[i, k - 1, [0, 1, 2, 4, 5, 6, 7]])
        assert segs[i, k - 1, 3] < segs0[i, k - 1, 3]                       # the last one ends on the black piece
    same = ok & (with_b["ends"] != "black")
    assert np.array_equal(segs[same], segs0[same])


# --------------------------------------------------------------------------- 4. properties
def test_adjoint_is_transpose(meshdir):
    d = im.insert_scene(meshdir, "cylindrical", "telecentric", False, inserts=("prism", "u"), black=True)
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
    d = im.insert_scene(meshdir, "square", "lens", False, inserts=("u",), black=True, max_depth=16, rr_depth=2,
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
    """Collimated rays at regular sampling do not depend on their sampler stream: the sparse set's forward is the
    dense one with zeros elsewhere, and its gradient the dense one's entries."""
    d = im.insert_scene(meshdir, "square", "collimated", True, inserts=("prism", "u"), black=True)
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
    ds.active_base, ds.active_total = 0, n  # the ray weight of the whole set
    sp = Projection(ds, DEV)
    sub = dev(pix[sel].astype(np.int32), torch.int32)
    sparse = sp.forward(dev(pat[sel]), sub, 1, SEED).cpu().numpy()
    gs = sp.adjoint(G, sel.size, sub, 1, SEED).cpu().numpy()
    sp.close()
    assert np.linalg.norm(dense) > 0 and rel_l2(sparse, dense) < RTOL
    assert np.array_equal(gs, gd[sel])


# --------------------------------------------------------------------------- refusals on the device
def test_refusals_allocate_nothing_and_name_the_entry(meshdir):
    base = im.insert_scene(meshdir, "cylindrical", "collimated", True, inserts=("box",))
    Projection(base, DEV).close()  # the runtime is up
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    d = base.copy()
    d.albedo = 0.5
    with pytest.raises(ValueError, match="dielectric occluders with a scattering medium"):
        Projection(d, DEV)
    d = base.copy()
    bad = im.mesh("box").copy()
    bad[0, 0] = [3.5, 0.0, 0.0]
    d.set_inserts([(bad, 1.58, 1.4849)])
    with pytest.raises(ValueError, match="insert 0: triangle 0 vertex 0 lies outside the resin"):
        Projection(d, DEV)
    d = base.copy()
    d.set_inserts([(im.mesh("box"), 1.58, 0.0)])
    with pytest.raises(ValueError, match="insert 0: int_ior and ext_ior must be positive"):
        Projection(d, DEV)
    assert torch.cuda.mem_get_info(0)[0] == free0
    proj = Projection(base, DEV)
    n = base.n_patterns * base.crop_y * base.crop_x
    pat = torch.zeros(n, device=DEV)
    G = torch.zeros(film_shape(base) + (1,), device=DEV)
    with pytest.raises(ValueError, match="dielectric occluders with filter_radon"):
        proj.radon(np.zeros((0, 3, 3), np.float32))
    with pytest.raises(ValueError, match="tvam_forward_dsigma: a plan with dielectric occluders"):
        proj.forward_dsigma(pat, None, 1, 0)
    with pytest.raises(ValueError, match="tvam_adjoint_dsigma: a plan with dielectric occluders"):
        proj.adjoint_dsigma(pat, G, None, 1, 0)
    with pytest.raises(ValueError, match="tvam_forward_slices: dielectric occluders"):
        proj.forward_slices(pat, None, 1, 0, 0, 4, G.clone())
    with pytest.raises(ValueError, match="tvam_adjoint_slices: dielectric occluders"):
        proj.adjoint_slices(G, n, 0, 4, 0, 2, pat.clone())
    with pytest.raises(ValueError, match="tvam_plan_segments: a plan with dielectric occluders"):
        proj.segments(None, None, 1, 0)
    # the corner filter serves such a plan: inserts lie inside the resin and never come first
    keep, hits = proj.corner(2.9, 0.3, hits=True)
    plain = Projection(desc_from_config(im.insert_config("cylindrical", "collimated", True, inserts=(),
                                                         paths=im.write_meshes(meshdir))), DEV)
    keep0, hits0 = plain.corner(2.9, 0.3, hits=True)
    assert torch.equal(keep, keep0) and torch.equal(hits, hits0) and int(keep.sum()) > 0
    with pytest.raises(ValueError, match="tvam_plan_insert_segments: plans with dielectric occluders only"):
        plain.insert_segments(None, None, 1, 0)
    # the same refusals at the C entries with every buffer made beforehand (the wrappers above make their outputs
    # first, and torch keeps what it once took): free device memory is the same before and after
    film, vec, segs = G.clone(), pat.clone(), torch.zeros((n, 2, 8), device=DEV)
    nseg = torch.zeros(n, dtype=torch.int32, device=DEV)
    one = torch.zeros((), dtype=torch.float64, device=DEV)
    tri = np.zeros((1, 3, 3), np.float32)
    lib, P, Q = proj.lib, proj._plan, plain._plan
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    U = _abi.TVAM_ERR_UNSUPPORTED
    assert lib.tvam_radon(P, tri.ctypes.data, 1, 4, 0, 5, vec.data_ptr(), None) == U
    assert lib.tvam_forward_dsigma(P, pat.data_ptr(), None, n, 1, 0, film.data_ptr(), None) == U
    assert lib.tvam_adjoint_dsigma(P, pat.data_ptr(), G.data_ptr(), None, n, 1, 0, one.data_ptr(), None) == U
    assert lib.tvam_forward_slices(P, pat.data_ptr(), None, n, 1, 0, 0, 4, film.data_ptr(), None) == U
    assert lib.tvam_adjoint_slices(P, G.data_ptr(), n, 0, 4, 0, 2, vec.data_ptr(), None) == U
    assert lib.tvam_plan_segments(P, None, n, 1, 0, segs.data_ptr(), None) == U
    assert lib.tvam_plan_insert_segments(Q, None, n, 1, 0, 2, segs.data_ptr(), nseg.data_ptr(), None) == U
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free1
    plain.close()
    proj.close()

"""The 'custom' vial on the GPU (tvam_mesh.h, tvam_ray3d.hip): two dielectric triangle meshes, every
ray traced through them in 3-D by closest-hit queries against a bounding volume hierarchy.

The oracle has no mesh vial, so the path is pinned the way tests/test_gpu_projectors.py pins the
3-D projector rays:
  1. tvam_plan_rays (Projection.rays) against the float64 model of tests/mesh_vial_model.py on
     every ray whose decisions the model finds at least 1e-4 from flipping (at most 1 % are not:
     tests/test_mesh_vial.py checks that on the CPU);
  2. dose, gradient and visit count against the oracle's DDA (oracle.dda_ray) marched over those
     exported segments;
  3. closed cube meshes against the oracle's own square vial, end to end.
Shapes: projector_model.projector_scene's (6 angles, 24 x 20 DMD, 40 x 36 x 20 film, spp 2).  The
cuvette and the prism are staged in LDS, the 4096-triangle tube is read through the caches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config, square_vial
from drtvam_amd.engine import Projection

import mesh_vial_model as mv
import projector_model as pm
from parity_util import flip_protocol

RTOL = 1e-4
DEV = "cuda:0"
SPP, SEED = 2, 3
KINDS = ("collimated", "telecentric", "lens")
MESHES = ("cuvette", "prism", "tube")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def with_flags(d, flags):
    d = d.copy()
    d.flags = int(flags)
    return d


def film_shape(d):
    rx, ry, rz = d.film_res
    return (rz, ry, rx)


# --------------------------------------------------------------------------- 1. the export
@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("kind", KINDS)
def test_export_matches_model(kind, mesh):
    m = mv.scene_model(kind, mesh, SPP, SEED)
    d = m["desc"]
    proj = Projection(d, DEV)
    assert proj.cone and not proj.planar and proj.fwd_chunk == 0
    rays = proj.rays(None, None, SPP, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    n = d.n_patterns * d.crop_y * d.crop_x
    assert rays.shape == (n * SPP, 16)
    ok = m["margin"] > mv.MARGIN
    assert (~ok).mean() <= 0.01
    # the projector's own bounds (test_gpu_projectors.py) for the ray itself
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    assert np.abs(rays[:, 0:3] - m["o"]).max() <= tol_o and np.abs(rays[:, 3:6] - m["d"]).max() <= tol_d
    hit = rays[:, 6] != 0.0
    assert np.array_equal(hit[ok], m["hit"][ok])
    assert not rays[~hit, 7:11].any()
    sel = ok & hit
    assert sel.mean() > 0.5
    # three chained closest hits and refractions on top of the projector's own arithmetic: 4 x
    e_o = np.abs(rays[sel, 7:10] - m["o2"][sel]).max()
    e_t = np.abs(rays[sel, 10] - m["maxt"][sel]).max()
    e_d = np.abs(rays[sel, 11:14] - m["d2"][sel]).max()
    w = float(pm.ray_weight(d, n, SPP))
    e_w = np.abs(rays[sel, 14] / (w * m["weight"][sel]) - 1.0).max()
    print(f"{kind} {mesh}: hits {hit.mean():.3f} below margin {(~ok).mean():.4f} |do2| {e_o:.3e} |dmaxt| {e_t:.3e} "
          f"(tol {4 * tol_o:.3e}) |dd2| {e_d:.3e} |dw|/w {e_w:.3e} (tol {4 * tol_d:.3e})")
    assert e_o <= 4 * tol_o and e_t <= 4 * tol_o and e_d <= 4 * tol_d and e_w <= 4 * tol_d
    assert np.abs(np.linalg.norm(rays[hit, 11:14], axis=1) - 1.0).max() <= 16 * tol_d
    assert np.all(rays[~hit, 14] == w) and np.array_equal(rays[~hit, 11:14], rays[~hit, 3:6])
    if mesh == "prism":  # refraction is really there, out of the slice too
        assert np.abs(rays[sel, 11:14] - rays[sel, 3:6]).max() > 1e-2
        if kind == "collimated":
            assert np.all(rays[:, 5] == 0.0) and np.abs(rays[sel, 13]).min() > 1e-3


# --------------------------------------------------------------------------- 2. dose, gradient, visits
VARIANTS = {
    "collimated-prism": ("collimated", "prism", {}),
    "telecentric-cuvette": ("telecentric", "cuvette", {}),
    "lens-tube": ("lens", "tube", {}),
    "collimated-cuvette-regular": ("collimated", "cuvette", dict(regular=True)),
}
_REF = {}


def reference(oracle, name):
    """Per variant, computed once: the exported segments of the per-ray plan and the oracle's DDA
    over them (the pattern of test_gpu_projectors.reference)."""
    if name in _REF:
        return _REF[name]
    kind, mesh, kw = VARIANTS[name]
    d = mv.custom_scene(kind, mesh, **kw)
    spp = 1 if d.regular_sampling else SPP
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(11)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(with_flags(d, _abi.FLAG_SCATTER_ATOMIC), DEV)
    rays = proj.rays(n, None, spp, SEED).cpu().numpy()
    proj.close()
    iv = float(pm.inv_vol(d))
    dose = np.zeros(film_shape(d), np.float64)
    grad = np.zeros(n, np.float64)
    visits = 0
    for i, r in enumerate(rays):
        if r[6] == 0.0:
            continue
        film, v = oracle.dda_ray(d, r[7:10], r[11:14], float(r[10]))
        visits += v
        w = float(r[14]) * iv
        dose += (w * float(pat[i // spp])) * film
        grad[i // spp] += w * float(np.vdot(film, G))
    _REF[name] = dict(desc=d, spp=spp, n=n, pat=pat, G=G, dose=dose, grad=grad, visits=visits)
    return _REF[name]


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_dose_matches_oracle_dda(oracle, name, fwd):
    ref = reference(oracle, name)
    d = with_flags(ref["desc"], _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST)
    proj = Projection(d, DEV)
    dose = proj.forward(dev(ref["pat"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
    err = rel_l2(dose, ref["dose"])
    st = proj.bin_stats()
    print(f"{name} {fwd}: dose rel-L2 {err:.3e}, bins {st}")
    assert np.linalg.norm(ref["dose"]) > 0
    assert err < RTOL
    if fwd == "binned":
        assert st["chunks"] >= 1 and st["entries"] > 0 and st["count_mismatch"] == 0
    else:
        assert st["chunks"] == 0
        assert proj.count_visits(ref["spp"], SEED) == ref["visits"]
    proj.close()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_gradient_matches_oracle_dda(oracle, name):
    ref = reference(oracle, name)
    proj = Projection(ref["desc"], DEV)
    grad = proj.adjoint(dev(ref["G"]), ref["n"], None, ref["spp"], SEED).cpu().numpy()
    proj.close()
    err = rel_l2(grad, ref["grad"])
    print(f"{name}: gradient rel-L2 {err:.3e}")
    assert np.linalg.norm(ref["grad"]) > 0 and err < RTOL


# --------------------------------------------------------------------------- 3. the oracle's square vial
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
def test_closed_cubes_match_oracle_square_vial(oracle, regular):
    """A SquareVial's two cuboids as closed meshes: the same scene, so the oracle's square-vial
    forward and adjoint are the reference for ray generation, weights and the whole chain."""
    spp = 1 if regular else 2
    cfg = square_vial(N=24, angles=12, regular_sampling=regular, spp=spp)
    dsq = desc_from_config(cfg)
    d = dsq.copy()
    d.vial_type = _abi.VIAL_CUSTOM
    outer, inner = mv.square_vial_meshes(cfg["vial"]["w_int"], cfg["vial"]["w_ext"], float(dsq.vial_height))
    d.set_vial_meshes(outer, inner)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(0)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(-1.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(d, DEV)
    assert proj.cone
    out = flip_protocol(oracle, proj, dsq, pat, G, spp, 5, nthreads=8, dev=DEV)
    proj.close()
    assert out["visits"] > 0


# --------------------------------------------------------------------------- 4. - 6. properties
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_adjoint_is_transpose(fwd):
    d = with_flags(mv.custom_scene("telecentric", "prism"),
                   _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, n).astype(np.float32)
    y = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(d, DEV)
    Ax = proj.forward(dev(x), None, SPP, SEED).cpu().numpy()[..., 0].astype(np.float64)
    Aty = proj.adjoint(dev(y), n, None, SPP, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    lhs, rhs = float(np.vdot(Ax, y)), float(np.vdot(x, Aty))
    print(f"{fwd}: <Ax, y> {lhs:.9e} <x, Aty> {rhs:.9e}")
    assert lhs > 0 and abs(lhs - rhs) <= RTOL * abs(lhs)


@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_angle_shards_sum_to_full_render(fwd):
    flag = _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST
    d = with_flags(mv.custom_scene("lens", "cuvette"), flag)
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
    for a0, a1 in ((0, 3), (3, 6)):
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


@pytest.mark.parametrize("mesh", ["cuvette", "tube"])
def test_second_forward_is_served_from_the_bin_cache(mesh):
    d = with_flags(mv.custom_scene("telecentric", mesh), _abi.FLAG_BIN_FIRST | _abi.FLAG_NO_ZERO_SKIP)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(4)
    p1, p2 = (dev(rng.uniform(0.0, 0.1, n).astype(np.float32)) for _ in range(2))
    proj = Projection(d, DEV)
    a = proj.forward(p1, None, SPP, SEED).clone()
    s1 = proj.bin_stats()
    b = proj.forward(p1, None, SPP, SEED).clone()
    s2 = proj.bin_stats()
    assert s1["cached"] == 0 and s1["stored"] == s1["chunks"] >= 1
    assert s2["cached"] == s2["chunks"] >= 1
    assert float(a.abs().max()) > 0 and torch.equal(a, b)
    # another pattern from the cache (the records' weights rescaled by the kept attenuation) equals
    # an uncached plan's forward
    c = proj.forward(p2, None, SPP, SEED).clone()
    assert proj.bin_stats()["cached"] >= 1
    proj.close()
    fresh = Projection(d, DEV)
    c2 = fresh.forward(p2, None, SPP, SEED)
    assert fresh.bin_stats()["cached"] == 0 and torch.equal(c, c2)
    fresh.close()


# --------------------------------------------------------------------------- 7. filter_corner
@pytest.mark.parametrize("kind", ["collimated", "telecentric"])
def test_filter_corner_on_the_cuvette(kind):
    """The first-hit pass takes the nearest hit of the outer mesh, from either side; the pixel stays
    unless its ray misses or lands within `radius` of a vertical edge (+-dist, +-dist).  The model:
    the pass's own rays (pixel centres, spp 1, seed 0) against the outer mesh in float64."""
    d = mv.custom_scene(kind, "cuvette")
    outer = np.asarray(d._vial_outer, np.float64)
    dist, radius = float(np.abs(outer[..., 0]).max()), 0.5
    dr = d.copy()
    dr.regular_sampling = 1
    pix = pm.dense_pixels(d)
    m = pm.model_rays(dr, pix, np.arange(pix.size), 1, 0)
    t, _, _, edge = mv._closest(outer, m["o"], m["d"])
    hit = np.isfinite(t)
    p = m["o"] + m["d"] * np.where(hit, t, 0.0)[:, None]
    rr = np.hypot(np.abs(p[:, 0]) - dist, np.abs(p[:, 1]) - dist)
    keep = hit & ~(rr < radius)
    decided = (edge > mv.MARGIN) & (np.abs(rr - radius) > mv.MARGIN)
    proj = Projection(d, DEV)
    got, hits = proj.corner(dist, radius, hits=True)
    got, hits = got.cpu().numpy(), hits.cpu().numpy().astype(np.float64)
    proj.close()
    print(f"{kind}: kept {int(got.sum())} of {got.size}, model {int(keep.sum())}, undecided {int((~decided).sum())}")
    assert (~decided).mean() <= 0.01
    assert np.array_equal(got[decided] != 0.0, keep[decided])
    assert 0 < keep.sum() < hit.sum() <= hit.size  # corners are dropped, not only misses
    sel = decided & hit
    tol = 4 * 64 * float(np.spacing(np.float32(d.distance)))
    assert np.abs(hits[sel, :3] - p[sel]).max() <= tol and np.abs(hits[sel, 3] - t[sel]).max() <= tol
    assert np.all(hits[decided & ~hit, 3] == -1.0)


# --------------------------------------------------------------------------- refusals on the device
def test_refusals_allocate_nothing():
    Projection(mv.custom_scene("collimated", "cuvette"), DEV).close()  # the runtime is up
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    d = mv.custom_scene("telecentric", "cuvette")
    d.albedo = 0.5
    with pytest.raises(ValueError, match="a 'custom' vial with a scattering medium"):
        Projection(d, DEV)
    d = mv.custom_scene("collimated", "cuvette")
    bad = np.array(d._vial_inner)
    bad[2, 2] = bad[2, 1]
    d.set_vial_meshes(d._vial_outer, bad)
    with pytest.raises(ValueError, match="the inner vial mesh: triangle 2 has zero area"):
        Projection(d, DEV)
    assert torch.cuda.mem_get_info(0)[0] == free0
    proj = Projection(mv.custom_scene("collimated", "cuvette"), DEV)
    with pytest.raises(ValueError, match="a 'custom' vial with filter_radon"):
        proj.radon(np.zeros((0, 3, 3), np.float32))
    proj.close()

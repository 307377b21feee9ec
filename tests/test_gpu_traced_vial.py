"""The 'cylindrical' and 'square' vials traced per ray in 3-D on the GPU (tvam_glass.h, the CN_GLASS
instantiations of tvam_ray3d.hip; plans of tvam_plan_create_traced).

  1. tvam_plan_rays (Projection.rays) against the float64 model of tests/traced_vial_model.py on
     every ray whose decisions the model finds at least 1e-4 from flipping (at most 1 % are not:
     tests/test_traced_vial.py checks that on the CPU), with that file's bounds;
  2. dose (atomic, binned, and the cached second call with new pattern values), gradient and visit
     count against the oracle's DDA (oracle.dda_ray) marched over those exported segments;
  3. a collimated descriptor through the traced entry against the oracle's own cylindrical / square
     vial (parity_util.flip_protocol) and against the planar plan of tvam_plan_create;
  4. the transpose identity, angle shards, filter_corner, refusals.
Shapes: traced_vial_model.traced_config's (12 angles, 48 x 16 DMD, 40 x 40 x 24 film, spp 2)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.engine import Projection

import corner_model as cm
import projector_model as pm
import traced_vial_model as tv
from parity_util import flip_protocol

RTOL = 1e-4
DEV = "cuda:0"
SPP, SEED = 2, 3
VIALS = ("cylindrical", "square")
KINDS = ("collimated", "telecentric", "lens")
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))


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
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("vial", VIALS)
def test_export_matches_model(vial, kind, regular):
    m = tv.scene_model(vial, kind, regular, SPP, SEED)
    d = m["desc"]
    spp = 1 if regular else SPP
    proj = Projection(d, DEV)
    assert proj.cone and not proj.planar and not proj.planar_forward and proj.fwd_chunk == 0
    rays = proj.rays(None, None, spp, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    n = d.n_patterns * d.crop_y * d.crop_x
    assert rays.shape == (n * spp, 16)
    assert (m["margin"] <= tv.MARGIN).mean() <= 0.01
    # the projector's own bounds (test_gpu_projectors.py) for the ray itself
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    assert np.abs(rays[:, 0:3] - m["o"]).max() <= tol_o and np.abs(rays[:, 3:6] - m["d"]).max() <= tol_d
    # the segment against the model traced from the exported (fp32) ray
    ref = tv.trace_desc(d, rays[:, 0:3], rays[:, 3:6])
    hit = rays[:, 6] != 0.0
    w = float(pm.ray_weight(d, n, spp))
    got = np.zeros((len(rays), 8))
    got[hit, 0:4] = rays[hit, 7:11]
    got[hit, 4:7] = rays[hit, 11:14]
    got[hit, 7] = rays[hit, 14] / w
    assert not rays[~hit, 7:11].any()
    r = tv.compare_segments(got, ref)
    print(f"{vial} {kind} {'regular' if regular else 'jittered'}: hits {hit.mean():.3f} compared {r['compared']} below "
          f"margin {r['low']:.4f} |do2| {r['e_o']:.3e} |dmaxt| {r['e_t']:.3e} (tol {TOL_O:.3e}) |dd2| {r['e_d']:.3e} "
          f"|dw|/w {r['e_w']:.3e} (tol {TOL_D:.3e}), each / kappa")
    assert r["low"] <= 0.01
    assert r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D
    assert np.abs(np.linalg.norm(rays[hit, 11:14], axis=1) - 1.0).max() <= 16 * tol_d
    # a ray that never reaches the medium keeps its own direction and the plain weight
    assert np.all(rays[~hit, 14] == np.float32(w)) and np.array_equal(rays[~hit, 11:14], rays[~hit, 3:6])
    assert np.abs(rays[hit, 11:14] - rays[hit, 3:6]).max() > 1e-2  # refracted at all
    # the host tracer is the kernels' code: the same bits from the same rays
    host = _abi.traced_segments(d, rays[:, 0:3].astype(np.float32), rays[:, 3:6].astype(np.float32))
    assert np.array_equal(host[:, 3] != 0.0, hit)
    assert np.array_equal(host[hit, 0:7].astype(np.float64), got[hit, 0:7])


# --------------------------------------------------------------------------- 2. dose, gradient, visits
VARIANTS = {
    "cylindrical-telecentric": ("cylindrical", "telecentric", False),
    "square-lens": ("square", "lens", False),
    "square-telecentric-regular": ("square", "telecentric", True),
    "cylindrical-lens-regular": ("cylindrical", "lens", True),
}
_REF = {}


def reference(oracle, name):
    """Per variant, computed once and left unchanged: the exported segments of the per-ray plan and
    the oracle's DDA over them (the pattern of test_gpu_mesh_vial.reference)."""
    if name in _REF:
        return _REF[name]
    vial, kind, regular = VARIANTS[name]
    d = tv.traced_scene(vial, kind, regular)
    spp = 1 if regular else SPP
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(11)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    pat2 = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(with_flags(d, _abi.FLAG_SCATTER_ATOMIC), DEV)
    rays = proj.rays(n, None, spp, SEED).cpu().numpy()
    proj.close()
    iv = float(pm.inv_vol(d))
    dose = np.zeros(film_shape(d), np.float64)
    dose2 = np.zeros(film_shape(d), np.float64)
    grad = np.zeros(n, np.float64)
    visits = 0
    for i, r in enumerate(rays):
        if r[6] == 0.0:
            continue
        film, v = oracle.dda_ray(d, r[7:10], r[11:14], float(r[10]))
        visits += v
        w = float(r[14]) * iv
        nz = np.nonzero(film)
        dose[nz] += (w * float(pat[i // spp])) * film[nz]
        dose2[nz] += (w * float(pat2[i // spp])) * film[nz]
        grad[i // spp] += w * float(np.vdot(film[nz], G[nz]))
    _REF[name] = dict(desc=d, spp=spp, n=n, pat=pat, pat2=pat2, G=G, dose=dose, dose2=dose2, grad=grad, visits=visits)
    return _REF[name]


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_dose_matches_oracle_dda(oracle, name, fwd):
    ref = reference(oracle, name)
    flags = _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST | _abi.FLAG_NO_ZERO_SKIP
    proj = Projection(with_flags(ref["desc"], flags), DEV)
    dose = proj.forward(dev(ref["pat"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
    err = rel_l2(dose, ref["dose"])
    st = proj.bin_stats()
    print(f"{name} {fwd}: dose rel-L2 {err:.3e}, bins {st}")
    assert np.linalg.norm(ref["dose"]) > 0
    assert err < RTOL
    if fwd == "binned":
        assert st["chunks"] >= 1 and st["entries"] > 0 and st["count_mismatch"] == 0
        assert st["cached"] == 0 and st["stored"] == st["chunks"]
        # the second call, with new pattern values, is served from the bin cache (the records'
        # weights rescaled by the kept attenuation)
        dose2 = proj.forward(dev(ref["pat2"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
        st2 = proj.bin_stats()
        err2 = rel_l2(dose2, ref["dose2"])
        print(f"{name} cached: dose rel-L2 {err2:.3e}, bins {st2}")
        assert st2["cached"] == st2["chunks"] >= 1
        assert err2 < RTOL
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


# --------------------------------------------------------------------------- 3. the oracle's own vials
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
@pytest.mark.parametrize("vial", VIALS)
def test_collimated_traced_plan_matches_oracle_and_planar_plan(oracle, vial, regular):
    """A collimated descriptor through the traced entry is the oracle's scene: its forward and adjoint
    are the reference for ray generation, weights and the whole chain; the planar plan of
    tvam_plan_create computes the same from the same inputs."""
    spp = 1 if regular else 2
    d = tv.traced_scene(vial, "collimated", regular)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(0)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(-1.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(d, DEV)
    assert proj.cone and not proj.planar
    out = flip_protocol(oracle, proj, d, pat, G, spp, 5, nthreads=8, dev=DEV)
    assert out["visits"] > 0
    dose = proj.forward(dev(pat), None, spp, 5).cpu().numpy()
    grad = proj.adjoint(dev(G), n, None, spp, 5).cpu().numpy()
    proj.close()
    dp = d.copy()
    dp.set_traced_vial(False)
    plan = Projection(dp, DEV)
    assert not plan.cone
    with pytest.raises(ValueError, match="tvam_plan_rays"):  # a planar plan's rays() stays refused
        plan.rays(None, None, spp, 5)
    dose_p = plan.forward(dev(pat), None, spp, 5).cpu().numpy()
    grad_p = plan.adjoint(dev(G), n, None, spp, 5).cpu().numpy()
    plan.close()
    e_d, e_g = rel_l2(dose, dose_p), rel_l2(grad, grad_p)
    print(f"{vial} {'regular' if regular else 'jittered'}: traced vs planar plan dose {e_d:.3e} gradient {e_g:.3e}")
    assert e_d < RTOL and e_g < RTOL


def test_planar_cuvette_plan_matches_oracle_between_the_heights(oracle):
    """The planar plan of tvam_plan_create on the 4-high cuvette under regular sampling, directly
    against the oracle: DMD rows between the inner cuboid's height (1.8) and the outer one's (2)
    cross glass alone and deposit nothing, so the planar row lists must leave them out."""
    d = tv.traced_scene("square", "collimated", True)
    d.set_traced_vial(False)
    yc = (0.5 * d.res_y - 0.5 - np.arange(d.res_y)) * d.pixel_size_y
    band = (np.abs(yc) > 0.45 * d.vial_height) & (np.abs(yc) <= 0.5 * d.vial_height)
    assert band.sum() == 2  # rows at +-1.95
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(2)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(-1.0, 1.0, film_shape(d)).astype(np.float32)
    plan = Projection(d, DEV)
    assert plan.planar and not plan.cone
    out = flip_protocol(oracle, plan, d, pat, G, 1, 5, nthreads=8, dev=DEV)
    assert out["visits"] > 0 and out["flipped"] == 0
    # those rows' pixels have no gradient at all
    g = plan.adjoint(dev(np.abs(G)), n, None, 1, 5).cpu().numpy().reshape(d.n_patterns, d.crop_y, d.crop_x)
    plan.close()
    assert not g[:, band].any() and g[:, ~band & (np.abs(yc) < 1.8)].any()


def test_slice_calls_refuse_a_traced_plan():
    """forward_slices / adjoint_slices serve planar plans only: a traced plan has no slice chunks."""
    d = tv.traced_scene("square", "collimated", True)
    n = d.n_patterns * d.crop_y * d.crop_x
    proj = Projection(d, DEV)
    assert proj.fwd_chunk == 0 and proj.adj_chunk == 0
    dose = torch.zeros(proj.film_shape, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="cannot be split into slice ranges"):
        proj.forward_slices(dev(np.zeros(n, np.float32)), None, 1, 0, 0, 8, dose)
    with pytest.raises(ValueError, match="planar plans only"):
        proj.adjoint_slices(dose, n, 0, 8, 0, d.crop_y, torch.zeros(n, dtype=torch.float32, device=DEV))
    proj.close()


# --------------------------------------------------------------------------- 4. properties
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
@pytest.mark.parametrize("vial", VIALS)
def test_adjoint_is_transpose(vial, fwd):
    d = with_flags(tv.traced_scene(vial, "telecentric"),
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
    print(f"{vial} {fwd}: <Ax, y> {lhs:.9e} <x, Aty> {rhs:.9e}")
    assert lhs > 0 and abs(lhs - rhs) <= RTOL * abs(lhs)


@pytest.mark.parametrize("vial", VIALS)
def test_angle_shards_sum_to_full_render(vial):
    d = tv.traced_scene(vial, "lens")
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
    for a0, a1 in ((0, 5), (5, 12)):
        ds = d.copy()
        ds.angle_begin, ds.angle_end = a0, a1
        ds.active_base, ds.active_total = a0 * per, n
        assert ds.traced_vial
        sh = Projection(ds, DEV)
        total += sh.forward(dev(pat[a0 * per:a1 * per]), None, SPP, SEED).cpu().numpy()
        parts.append(sh.adjoint(G, (a1 - a0) * per, None, SPP, SEED).cpu().numpy())
        sh.close()
    assert np.linalg.norm(dose) > 0
    assert rel_l2(total, dose) < RTOL
    assert rel_l2(np.concatenate(parts), grad) < RTOL


def test_sparse_active_set_and_crop():
    """Every third pixel of a cropped DMD: the sparse set's rays are the dense set's."""
    d = tv.traced_scene("square", "telecentric")
    d.crop_x, d.crop_y, d.crop_offset_x, d.crop_offset_y = 40, 12, 5, 3
    d.clockwise = 1
    pix = pm.dense_pixels(d)
    proj = Projection(d, DEV)
    dense = proj.rays(None, None, SPP, SEED).cpu().numpy()
    proj.close()
    sub = np.ascontiguousarray(pix[::3]).astype(np.int32)
    ds = d.copy()
    ds.active_base, ds.active_total = 0, sub.size
    sp = Projection(ds, DEV)
    rays = sp.rays(None, dev(sub, torch.int32), SPP, SEED).cpu().numpy()
    m = pm.model_rays(ds, sub, np.arange(sub.size), SPP, SEED)
    sp.close()
    assert rays.shape == (sub.size * SPP, 16) and dense.shape == (pix.size * SPP, 16)
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    assert np.abs(rays[:, 0:3] - m["o"]).max() <= tol_o
    host = _abi.traced_segments(ds, rays[:, 0:3], rays[:, 3:6])
    hit = rays[:, 6] != 0
    assert 0 < hit.sum() < hit.size and np.array_equal(host[:, 3] != 0, hit)
    assert np.array_equal(host[hit, 0:4], rays[hit, 7:11]) and np.array_equal(host[hit, 4:7], rays[hit, 11:14])


def test_sample_time_rays():
    """sample_time draws the angle per sample: the rays are the model's, the segments the host tracer's."""
    d = tv.traced_scene("cylindrical", "lens")
    d.sample_time = 1
    pix = pm.dense_pixels(d)
    m = pm.model_rays(d, pix, np.arange(pix.size), SPP, SEED)
    proj = Projection(d, DEV)
    rays = proj.rays(None, None, SPP, SEED).cpu().numpy()
    proj.close()
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    assert np.abs(rays[:, 0:3] - m["o"]).max() <= tol_o and np.abs(rays[:, 3:6] - m["d"]).max() <= tol_d
    d0 = d.copy()
    d0.sample_time = 0
    m0 = pm.model_rays(d0, pix, np.arange(pix.size), SPP, SEED)
    assert np.abs(m["o"] - m0["o"]).max() > 0.1  # the time sample moves the projector
    host = _abi.traced_segments(d, rays[:, 0:3], rays[:, 3:6])
    hit = rays[:, 6] != 0
    assert 0 < hit.sum() < hit.size and np.array_equal(host[:, 3] != 0, hit)
    assert np.array_equal(host[hit, 0:4], rays[hit, 7:11]) and np.array_equal(host[hit, 4:7], rays[hit, 11:14])


# --------------------------------------------------------------------------- filter_corner
def test_filter_corner_lens_square():
    """The first-hit pass on a traced plan: the outer cuboid from the lens projector's 3-D rays,
    against tests/corner_model.py."""
    d = tv.traced_scene("square", "lens")
    dist, radius = float(d.vial_r_ext), 0.8
    pix = pm.dense_pixels(d)
    model = cm.corner_model(d, pix, dist, radius)
    proj = Projection(d, DEV)
    keep, hits = proj.corner(dist, radius, hits=True)
    proj.close()
    und = cm.compare(model, keep.cpu().numpy(), hits.cpu().numpy())
    k = model["keep"]
    print(f"lens square: kept {int(k.sum())} of {k.size}, hits {int(model['hit'].sum())}, undecided {und}")
    assert 0 < k.sum() < model["hit"].sum() <= k.size  # corners are dropped, not only misses


# --------------------------------------------------------------------------- refusals on the device
def test_refusals_allocate_nothing():
    Projection(tv.traced_scene("square", "lens"), DEV).close()  # the runtime is up
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for vial in VIALS:
        d = tv.traced_scene(vial, "telecentric")
        d.albedo = 0.5
        with pytest.raises(ValueError, match="the 'telecentric' projector with a scattering medium"):
            Projection(d, DEV)
        d = tv.traced_scene(vial, "lens")
        d.vial_r_ext = d.vial_r
        with pytest.raises(ValueError, match="r_ext > r_int"):
            Projection(d, DEV)
        d = tv.traced_scene(vial, "lens")
        d.set_traced_vial(False)  # tvam_plan_create keeps refusing the combination
        with pytest.raises(ValueError, match=f"the 'lens' projector with a '{vial}' vial"):
            Projection(d, DEV)
    assert torch.cuda.mem_get_info(0)[0] == free0
    proj = Projection(tv.traced_scene("cylindrical", "telecentric"), DEV)
    with pytest.raises(ValueError, match="filter_radon"):
        proj.radon(np.zeros((0, 3, 3), np.float32))
    proj.close()

"""The 'double_cylindrical' vial on the GPU (tvam_double.h, tvam_ray3d.hip): every ray traced
through four dielectric tubes, up to two medium segments per ray.

The oracle has no such vial, so the path is pinned the way tests/test_gpu_mesh_vial.py pins the
mesh vial:
  1. tvam_plan_segments (Projection.segments) against the float64 model of
     tests/double_vial_model.py on every ray whose decisions the model finds at least 1e-4 from
     flipping (at most 1 % are not: tests/test_double_vial.py checks that on the CPU);
  2. dose, gradient and visit count against the oracle's DDA (oracle.dda_ray) marched over those
     exported segments, for the atomic forward, the binned forward and its cached second call;
  3. an inner tube too thin for any pixel-centre ray to meet against the oracle's own cylindrical
     vial, end to end.
Scene (double_vial_model.double_scene): radii 7 / 6 / 3 / 2 with the reference's IORs, sigma_t 0.05,
12 angles, DMD 48 x 8 at pitch 0.3, film 40 x 40 x 20 over 14 x 14 x 3 (more than one 32 x 32 x 16
brick on every axis)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config
from drtvam_amd.engine import Projection

import double_vial_model as dv
import projector_model as pm

RTOL = 1e-4  # the project's parity bar
DEV = "cuda:0"
SPP, SEED = 2, 3
KINDS = ("collimated", "telecentric", "lens")
# tests/test_gpu_mesh_vial.py's export-vs-model bounds (times the segment's condition number,
# double_vial_model.compare_segments)
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def with_flags(d, flags, **fields):
    d = d.copy()
    d.flags = int(flags)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def film_shape(d):
    rx, ry, rz = d.film_res
    return (rz, ry, rx)


# --------------------------------------------------------------------------- 1. the export
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
@pytest.mark.parametrize("kind", KINDS)
def test_segments_match_model(kind, regular):
    m = dv.scene_model(kind, regular, SPP, SEED)
    d = m["desc"]
    spp = 1 if regular else SPP
    proj = Projection(d, DEV)
    assert proj.cone and not proj.planar and proj.fwd_chunk == 0
    segs = proj.segments(None, None, spp, SEED).cpu().numpy().astype(np.float64)
    rays = proj.rays(None, None, spp, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    n = d.n_patterns * d.crop_y * d.crop_x
    assert segs.shape == (n * spp, 2, 8) and rays.shape == (n * spp, 16)
    # the projector's own bounds (test_gpu_projectors.py) for the ray itself
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    assert np.abs(rays[:, 0:3] - m["o"]).max() <= tol_o and np.abs(rays[:, 3:6] - m["d"]).max() <= tol_d
    # tvam_plan_rays serves the first segment in its own layout
    hit = rays[:, 6] != 0.0
    assert np.array_equal(hit, segs[:, 0, 3] != 0.0)
    assert np.array_equal(rays[hit, 7:11], segs[hit, 0, 0:4]) and np.array_equal(rays[hit, 11:15], segs[hit, 0, 4:8])
    assert not rays[~hit, 7:11].any() and np.array_equal(rays[~hit, 11:14], rays[~hit, 3:6])
    w = float(pm.ray_weight(d, n, spp))
    assert np.all(rays[~hit, 14] == w)
    att = segs.copy()
    att[:, :, 7] /= w
    r = dv.compare_segments(att, m)
    print(f"{kind} {'regular' if regular else 'jittered'}: rays {len(segs)} segments compared {r['compared']} "
          f"below margin {r['low']:.4f} |do2| {r['e_o']:.3e} |dmaxt| {r['e_t']:.3e} (tol {TOL_O:.3e}) "
          f"|dd2| {r['e_d']:.3e} |dw|/w {r['e_w']:.3e} (tol {TOL_D:.3e}), each / kappa; largest kappa_d "
          f"{r['kappa_d']:.1f} kappa_w {r['kappa_w']:.1f}")
    assert r["low"] <= 0.01
    assert r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D
    present = segs[:, :, 3] != 0.0
    assert np.abs(np.linalg.norm(segs[present][:, 4:7], axis=1) - 1.0).max() <= 16 * tol_d
    counts = np.bincount(present.sum(1), minlength=3)
    assert counts[1] > 0 and counts[2] > 0
    assert counts[0] > 0 or kind == "lens"  # (the lens projector's rays converge: none passes the vial by)
    assert not present[:, 1][~present[:, 0]].any()  # never a second segment without a first


# --------------------------------------------------------------------------- 2. dose, gradient, visits
VARIANTS = {
    "collimated-regular": ("collimated", True),
    "telecentric-jittered": ("telecentric", False),
    "lens-jittered": ("lens", False),
}
_REF = {}


def reference(oracle, name):
    """Per variant, computed once: the exported segments of the plan and the oracle's DDA over them,
    first and second segments apart (the pattern of test_gpu_mesh_vial.reference)."""
    if name in _REF:
        return _REF[name]
    kind, regular = VARIANTS[name]
    d = dv.double_scene(kind, regular)
    spp = 1 if regular else SPP
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(11)
    pat, pat2 = (rng.uniform(0.0, 0.1, n).astype(np.float32) for _ in range(2))
    G = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(with_flags(d, _abi.FLAG_SCATTER_ATOMIC), DEV)
    segs = proj.segments(n, None, spp, SEED).cpu().numpy()
    proj.close()
    iv = float(pm.inv_vol(d))
    dose = np.zeros((2, 2) + film_shape(d), np.float64)  # [pattern][segment slot]
    grad = np.zeros(n, np.float64)
    visits = [0, 0]
    for i, row in enumerate(segs):
        for s in range(2):
            sg = row[s]
            if sg[3] == 0.0:
                continue
            film, v = oracle.dda_ray(d, sg[0:3], sg[4:7], float(sg[3]))
            visits[s] += v
            w = float(sg[7]) * iv
            dose[0, s] += (w * float(pat[i // spp])) * film
            dose[1, s] += (w * float(pat2[i // spp])) * film
            grad[i // spp] += w * float(np.vdot(film, G))
    _REF[name] = dict(desc=d, spp=spp, n=n, pat=pat, pat2=pat2, G=G, dose=dose, grad=grad, visits=visits, segs=segs)
    return _REF[name]


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_dose_matches_oracle_dda(oracle, name, fwd):
    ref = reference(oracle, name)
    flags = _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST | _abi.FLAG_NO_ZERO_SKIP
    proj = Projection(with_flags(ref["desc"], flags), DEV)
    want = ref["dose"][0].sum(0)
    dose = proj.forward(dev(ref["pat"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
    err = rel_l2(dose, want)
    st = proj.bin_stats()
    second = float(np.linalg.norm(ref["dose"][0, 1]) / np.linalg.norm(want))
    print(f"{name} {fwd}: dose rel-L2 {err:.3e} (second segments carry {second:.3f} of the norm), bins {st}")
    assert np.linalg.norm(ref["dose"][0, 0]) > 0 and second > 0.05
    assert err < RTOL
    if fwd == "binned":
        assert st["chunks"] >= 1 and st["entries"] > 0 and st["count_mismatch"] == 0 and st["cached"] == 0
        # the cached second call, new pattern values: the records' weights rescaled by the kept attenuation
        dose2 = proj.forward(dev(ref["pat2"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
        st2 = proj.bin_stats()
        err2 = rel_l2(dose2, ref["dose"][1].sum(0))
        print(f"{name} cached: dose rel-L2 {err2:.3e}, bins {st2}")
        assert st2["cached"] == st2["chunks"] >= 1
        assert err2 < RTOL
    else:
        assert st["chunks"] == 0
        assert proj.count_visits(ref["spp"], SEED) == sum(ref["visits"])
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


@pytest.mark.parametrize("name", ["collimated-regular", "lens-jittered"])
def test_max_depth_3_gives_first_segments_only(oracle, name):
    """The reference's `progressive` runs its first steps at max_depth 3: the first deposit (loop
    iteration 2) alone.  Against the same export."""
    ref = reference(oracle, name)
    d3 = with_flags(ref["desc"], _abi.FLAG_BIN_FIRST, max_depth=3)
    proj = Projection(d3, DEV)
    segs = proj.segments(ref["n"], None, ref["spp"], SEED).cpu().numpy()
    assert np.array_equal(segs[:, 0], ref["segs"][:, 0]) and not segs[:, 1].any() and ref["segs"][:, 1].any()
    dose = proj.forward(dev(ref["pat"]), None, ref["spp"], SEED).cpu().numpy()[..., 0]
    assert proj.count_visits(ref["spp"], SEED) == ref["visits"][0]
    proj.close()
    err = rel_l2(dose, ref["dose"][0, 0])
    print(f"{name} max_depth 3: dose rel-L2 {err:.3e} against the first segments")
    assert err < RTOL
    d2 = with_flags(ref["desc"], 0, max_depth=2)  # no deposit at all
    proj = Projection(d2, DEV)
    assert float(proj.forward(dev(ref["pat"]), None, ref["spp"], SEED).abs().max()) == 0.0
    assert float(proj.adjoint(dev(ref["G"]), ref["n"], None, ref["spp"], SEED).abs().max()) == 0.0
    proj.close()


# --------------------------------------------------------------------------- 3. the oracle's cylindrical vial
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_thin_inner_tube_matches_oracle_cylindrical_vial(oracle, fwd):
    """Inner tube 0.05 / 0.02: no pixel-centre ray reaches it (|b| min 0.15 against 0.074), so the
    scene is the oracle's cylindrical vial r_int_outer / r_ext_outer / ior_outer: its forward, adjoint
    and visit count are the reference for ray generation, weights and the whole chain."""
    radii = (7.0, 6.0, 0.05, 0.02)
    flag = _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST
    d = with_flags(dv.double_scene("collimated", True, radii=radii), flag)
    cfg = dv.double_config("collimated", True)
    cfg["vial"] = {"type": "cylindrical", "r_int": radii[1], "r_ext": radii[0], "ior": dv.IOR_OUTER,
                   "medium": cfg["vial"]["medium"]}
    dc = desc_from_config(cfg)
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
    assert not proj.segments(n, None, 1, 5)[:, 1].any()
    proj.close()
    e_f, e_a = rel_l2(dose, want), rel_l2(grad, gref)
    print(f"{fwd}: dose rel-L2 {e_f:.3e} gradient rel-L2 {e_a:.3e} visits {got_visits} (oracle {visits})")
    assert np.linalg.norm(want) > 0 and e_f <= RTOL and e_a <= RTOL
    assert got_visits == visits


# --------------------------------------------------------------------------- 4. - 5. properties
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_adjoint_is_transpose(fwd):
    d = with_flags(dv.double_scene("telecentric"), _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, n).astype(np.float32)
    y = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    proj = Projection(d, DEV)
    Ax = proj.forward(dev(x), None, SPP, SEED).cpu().numpy()[..., 0].astype(np.float64)
    Aty = proj.adjoint(dev(y), n, None, SPP, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    lhs, rhs = float(np.vdot(Ax, y.astype(np.float64))), float(np.vdot(x.astype(np.float64), Aty))
    print(f"{fwd}: <Ax, y> {lhs:.9e} <x, Aty> {rhs:.9e}")
    assert lhs > 0 and abs(lhs - rhs) <= RTOL * abs(lhs)


@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_angle_shards_sum_to_full_render(fwd):
    flag = _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST
    d = with_flags(dv.double_scene("lens"), flag)
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
        sh = Projection(ds, DEV)
        total += sh.forward(dev(pat[a0 * per:a1 * per]), None, SPP, SEED).cpu().numpy()
        parts.append(sh.adjoint(G, (a1 - a0) * per, None, SPP, SEED).cpu().numpy())
        sh.close()
    assert np.linalg.norm(dose) > 0
    assert rel_l2(total, dose) < RTOL
    assert rel_l2(np.concatenate(parts), grad) < RTOL


# --------------------------------------------------------------------------- refusals on the device
def test_refusals_allocate_nothing_and_name_the_filter():
    Projection(dv.double_scene("collimated"), DEV).close()  # the runtime is up
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    d = dv.double_scene("telecentric")
    d.albedo = 0.5
    with pytest.raises(ValueError, match="a 'double_cylindrical' vial with a scattering medium"):
        Projection(d, DEV)
    d = dv.double_scene("collimated")
    d.set_double_vial(7, 6, 6.5, 2, 1.5, 1.5, 1.3)
    with pytest.raises(ValueError, match="r_ext_outer > r_int_outer > r_ext_inner > r_int_inner > 0"):
        Projection(d, DEV)
    assert torch.cuda.mem_get_info(0)[0] == free0
    proj = Projection(dv.double_scene("collimated"), DEV)
    with pytest.raises(ValueError, match="a 'double_cylindrical' vial with filter_radon"):
        proj.radon(np.zeros((0, 3, 3), np.float32))
    with pytest.raises(ValueError, match="a 'double_cylindrical' vial with filter_corner"):
        proj.corner(7.0, 0.5)
    proj.close()
    other = Projection(pm.projector_scene("collimated"), DEV)
    with pytest.raises(ValueError, match="tvam_plan_segments: 'double_cylindrical' vial plans only"):
        other.segments(None, None, 1, 0)
    other.close()

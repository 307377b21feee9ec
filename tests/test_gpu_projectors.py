"""Telecentric and lens projectors on the GPU (tvam_ray3d.hip): the 3-D projector rays, their
medium segments, the per-ray forward / adjoint / visit count and the brick-binned forward.

The oracle restates only the collimated projector, so the new path is pinned in two steps:
  1. tvam_plan_rays (Projection.rays) is the oracle's ray bit for bit on a collimated plan, and for
     the new projectors agrees with the float64 model of tests/projector_model.py;
  2. dose, gradient and visit count are compared with the oracle's DDA (oracle.dda_ray) marched
     over those exported rays: both sides march the same rays, so no path is excluded.
RTOL = 1e-4 relative L2 is the project's parity bar."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.engine import Projection

import projector_model as pm

RTOL = 1e-4
DEV = "cuda:0"
SPP, SEED = 2, 3


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def with_flags(d, flags):
    d = d.copy()
    d.flags = int(flags)
    return d


VARIANTS = {
    "telecentric": dict(kind="telecentric"),
    "lens": dict(kind="lens"),
    "telecentric_short": dict(kind="telecentric", height=2.4),
    "sample_time": dict(kind="telecentric", sample_time=True),
    "regular": dict(kind="lens", regular=True),
    "sparse": dict(kind="telecentric", height=2.4),
}
_REF = {}


def reference(oracle, name):
    """Per variant, computed once: the exported rays of the per-ray plan and the oracle's DDA over them --
    dose for the pattern `pat`, per-entry gradient for the film gradient `G`, visit count."""
    if name in _REF:
        return _REF[name]
    d = pm.projector_scene(**VARIANTS[name])
    spp = 1 if d.regular_sampling else SPP
    n_dense = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(11)
    pix = None
    n = n_dense
    if name == "sparse":  # every third pixel; streams by position in the set
        pix = pm.dense_pixels(d)[::3].astype(np.int32)
        n = pix.size
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(0.0, 1.0, pm_film_shape(d)).astype(np.float32)
    proj = Projection(with_flags(d, _abi.FLAG_SCATTER_ATOMIC), DEV)
    rays = proj.rays(n, None if pix is None else dev(pix, torch.int32), spp, SEED).cpu().numpy()
    proj.close()
    iv = float(pm.inv_vol(d))
    dose = np.zeros(pm_film_shape(d), np.float64)
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
    _REF[name] = dict(desc=d, spp=spp, n=n, pix=pix, pat=pat, G=G, rays=rays, dose=dose, grad=grad, visits=visits)
    return _REF[name]


def pm_film_shape(d):
    rx, ry, rz = d.film_res
    return (rz, ry, rx)


# --------------------------------------------------------------------------- 1. the export
def test_export_is_oracle_ray_on_collimated_plan(oracle):
    d = pm.projector_scene("collimated", height=2.4)
    proj = Projection(d, DEV)
    assert not proj.cone
    rays = proj.rays(None, None, SPP, SEED).cpu().numpy()
    proj.close()
    pix = pm.dense_pixels(d)
    assert rays.shape == (pix.size * SPP, 16)
    w = pm.ray_weight(d, pix.size, SPP)
    hits = 0
    for i in range(rays.shape[0]):
        r = oracle.ray(d, int(pix[i // SPP]), i, SEED)
        g = rays[i]
        assert np.array_equal(g[0:3], r["o"]) and np.array_equal(g[3:6], r["d"]), i
        assert bool(g[6]) == r["hit"], i
        if r["hit"]:
            hits += 1
            assert np.array_equal(g[7:10], r["o2"]) and g[10] == np.float32(r["maxt"]), i
        else:
            assert not g[7:11].any()
        assert np.array_equal(g[11:14], r["d2"]) and g[14] == w and g[15] == 0.0
    assert 0 < hits < rays.shape[0]  # rows above / below the short vial miss


def test_export_with_sample_time_on_collimated_plan(oracle):
    """sample_time draws each ray's own angle (position, time, aperture: common.py:92-108) and takes
    its sine and cosine on the device, whose libm may differ from the host's in the last place: the
    oracle's ray to 64 ulp of the distance / of 1 instead of bit for bit."""
    d = pm.projector_scene("collimated", height=2.4, sample_time=True)
    proj = Projection(d, DEV)
    rays = proj.rays(None, None, SPP, SEED).cpu().numpy()
    proj.close()
    pix = pm.dense_pixels(d)
    tol_o, tol_d = 64 * np.spacing(np.float32(d.distance)), 64 * np.spacing(np.float32(1.0))
    for i in range(0, rays.shape[0], 7):
        r = oracle.ray(d, int(pix[i // SPP]), i, SEED)
        g = rays[i]
        assert np.abs(g[0:3] - r["o"]).max() <= tol_o and np.abs(g[3:6] - r["d"]).max() <= tol_d, i
        assert bool(g[6]) == r["hit"], i
        if r["hit"]:
            assert np.abs(g[7:10] - r["o2"]).max() <= tol_o and abs(g[10] - r["maxt"]) <= tol_o, i


# --------------------------------------------------------------------------- 2. the ray models
@pytest.mark.parametrize("kind,fov,seed", [("telecentric", False, 67), ("lens", False, 7), ("lens", True, 7)])
@pytest.mark.parametrize("height", [40.0, 2.4])
def test_ray_models_match_float64_model(kind, fov, seed, height):
    d = pm.projector_scene(kind, height=height, lens_fov=fov)
    proj = Projection(d, DEV)
    assert proj.cone and proj.fwd_chunk == 0 and proj.adj_chunk == 0
    rays = proj.rays(None, None, SPP, seed).cpu().numpy().astype(np.float64)
    proj.close()
    pix = pm.dense_pixels(d)
    m = pm.model_rays(d, pix, np.arange(pix.size), SPP, seed)
    assert m["margin"].min() > 1e-4  # no ray within 1e-4 of an open-end decision (CPU check)
    # ~20 fp32 operations (sincos included) at <= 2 ulp each; a convention error is O(1)
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    eo, ed = np.abs(rays[:, 0:3] - m["o"]).max(), np.abs(rays[:, 3:6] - m["d"]).max()
    en = np.abs(np.linalg.norm(rays[:, 3:6], axis=1) - 1.0).max()
    print(f"{kind} fov={fov} h={height}: |do| {eo:.3e} (tol {tol_o:.3e}) |dd| {ed:.3e} (tol {tol_d:.3e}) ||d|-1| {en:.3e}")
    assert eo <= tol_o and ed <= tol_d
    assert en <= 4 * float(np.spacing(np.float32(1.0)))
    hit = rays[:, 6] != 0.0
    assert np.array_equal(hit, m["hit"])
    if height > 10:
        assert hit.all()
    else:
        assert 0.5 < hit.mean() < 0.9
    e2 = np.abs(rays[hit, 7:10] - m["o2"][hit]).max()
    et = np.abs(rays[hit, 10] - m["maxt"][hit]).max()
    print(f"  |do2| {e2:.3e} |dmaxt| {et:.3e}")
    assert e2 <= tol_o and et <= tol_o
    assert not rays[~hit, 7:11].any()
    assert np.array_equal(rays[:, 11:14], rays[:, 3:6])
    assert np.all(rays[:, 14] == float(pm.ray_weight(d, pix.size, SPP)))


def test_lens_neighbouring_chief_rays():
    """Chief rays (aperture 0, regular sampling) of neighbouring pixels are pixel_size * s /
    focus_distance apart at axial distance s from the lens."""
    d = pm.projector_scene("lens", aperture=0.0, regular=True)
    proj = Projection(d, DEV)
    rays = proj.rays().cpu().numpy().astype(np.float64)
    proj.close()
    r = rays.reshape(d.n_patterns, d.crop_y, d.crop_x, 16)[0]  # angle 0: the axis is -x, the lens at x = distance
    tol = 64 * float(np.spacing(np.float32(d.distance)))
    assert np.abs(r[..., 0:3] - [d.distance, 0.0, 0.0]).max() <= tol  # every chief ray leaves the lens centre
    ps, F = float(np.float32(d.pixel_size_x)), float(d.focus_distance)
    for s in (17.0, 20.0, 23.0):
        p = r[..., 0:3] + r[..., 3:6] * (s / -r[..., 3])[..., None]
        assert np.abs(np.linalg.norm(p[:, 1:] - p[:, :-1], axis=-1) - ps * s / F).max() <= 2 * tol
        assert np.abs(np.linalg.norm(p[1:] - p[:-1], axis=-1) - ps * s / F).max() <= 2 * tol


# --------------------------------------------------------------------------- 3. dose
@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_dose_matches_oracle_dda(oracle, name, fwd):
    ref = reference(oracle, name)
    d = with_flags(ref["desc"], _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST)
    proj = Projection(d, DEV)
    pix = None if ref["pix"] is None else dev(ref["pix"], torch.int32)
    dose = proj.forward(dev(ref["pat"]), pix, ref["spp"], SEED).cpu().numpy()[..., 0]
    err = rel_l2(dose, ref["dose"])
    st = proj.bin_stats()
    print(f"{name} {fwd}: dose rel-L2 {err:.3e}, bins {st}")
    assert np.linalg.norm(ref["dose"]) > 0
    assert err < RTOL
    if fwd == "binned":
        assert st["chunks"] >= 1 and st["entries"] > 0 and st["count_mismatch"] == 0
    else:
        assert st["chunks"] == 0
        if ref["pix"] is None:  # tvam_count_visits counts the dense set
            assert proj.count_visits(ref["spp"], SEED) == ref["visits"]
    proj.close()


# --------------------------------------------------------------------------- 4. adjoint
@pytest.mark.parametrize("name", list(VARIANTS))
def test_gradient_matches_oracle_dda(oracle, name):
    ref = reference(oracle, name)
    proj = Projection(ref["desc"], DEV)
    pix = None if ref["pix"] is None else dev(ref["pix"], torch.int32)
    grad = proj.adjoint(dev(ref["G"]), ref["n"], pix, ref["spp"], SEED).cpu().numpy()
    proj.close()
    err = rel_l2(grad, ref["grad"])
    print(f"{name}: gradient rel-L2 {err:.3e}")
    assert np.linalg.norm(ref["grad"]) > 0 and err < RTOL


@pytest.mark.parametrize("kind", ["telecentric", "lens"])
@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_adjoint_is_transpose(kind, fwd):
    d = with_flags(pm.projector_scene(kind, height=2.4),
                   _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, n).astype(np.float32)
    y = rng.uniform(0.0, 1.0, pm_film_shape(d)).astype(np.float32)
    proj = Projection(d, DEV)
    Ax = proj.forward(dev(x), None, SPP, SEED).cpu().numpy()[..., 0].astype(np.float64)
    Aty = proj.adjoint(dev(y), n, None, SPP, SEED).cpu().numpy().astype(np.float64)
    proj.close()
    lhs, rhs = float(np.vdot(Ax, y)), float(np.vdot(x, Aty))
    print(f"{kind} {fwd}: <Ax, y> {lhs:.9e} <x, Aty> {rhs:.9e}")
    assert lhs > 0 and abs(lhs - rhs) <= RTOL * abs(lhs)


# --------------------------------------------------------------------------- 5. limits and properties
def test_zero_aperture_telecentric_is_collimated():
    dt = pm.projector_scene("telecentric", aperture=0.0)
    dc = pm.projector_scene("collimated")
    n = dt.n_patterns * dt.crop_y * dt.crop_x
    rng = np.random.default_rng(2)
    pat = dev(rng.uniform(0.0, 0.1, n).astype(np.float32))
    G = dev(rng.uniform(0.0, 1.0, pm_film_shape(dt)).astype(np.float32))
    out = {}
    for key, d in (("t", dt), ("c", dc)):
        proj = Projection(d, DEV)
        out[key] = (proj.forward(pat, None, SPP, SEED).cpu().numpy(), proj.adjoint(G, n, None, SPP, SEED).cpu().numpy())
        proj.close()
    ed, eg = rel_l2(out["t"][0], out["c"][0]), rel_l2(out["t"][1], out["c"][1])
    print(f"aperture 0 vs collimated: dose {ed:.3e} gradient {eg:.3e}")
    assert ed < RTOL and eg < RTOL


def test_binned_forward_repeatable_and_cached():
    d = with_flags(pm.projector_scene("telecentric", height=2.4), _abi.FLAG_BIN_FIRST | _abi.FLAG_NO_ZERO_SKIP)
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(4)
    p1, p2 = (dev(rng.uniform(0.0, 0.1, n).astype(np.float32)) for _ in range(2))
    proj = Projection(d, DEV)
    a = proj.forward(p1, None, SPP, SEED).clone()
    s1 = proj.bin_stats()
    b = proj.forward(p1, None, SPP, SEED).clone()
    s2 = proj.bin_stats()
    assert s1["cached"] == 0 and s1["stored"] == s1["chunks"] >= 1
    assert s2["cached"] == s2["chunks"] >= 1  # the second forward of the seed: no record writer, fill or sort
    assert torch.equal(a, b)
    # the line-search forward: the same seed with another pattern, from the cache, equals an uncached plan's
    c = proj.forward(p2, None, SPP, SEED).clone()
    assert proj.bin_stats()["cached"] >= 1
    proj.close()
    fresh = Projection(d, DEV)
    c2 = fresh.forward(p2, None, SPP, SEED)
    assert fresh.bin_stats()["cached"] == 0
    assert torch.equal(c, c2)
    # and without the cache (zero skipping on) two runs are bitwise identical too
    plain = Projection(with_flags(d, _abi.FLAG_BIN_FIRST), DEV)
    e1 = plain.forward(p1, None, SPP, SEED).clone()
    e2 = plain.forward(p1, None, SPP, SEED)
    assert plain.bin_stats()["cached"] == 0 and torch.equal(e1, e2)
    assert rel_l2(e1.cpu().numpy(), a.cpu().numpy()) < RTOL
    for p in (fresh, plain):
        p.close()


@pytest.mark.parametrize("fwd", ["atomic", "binned"])
def test_angle_shards_sum_to_full_render(fwd):
    flag = _abi.FLAG_SCATTER_ATOMIC if fwd == "atomic" else _abi.FLAG_BIN_FIRST
    d = with_flags(pm.projector_scene("lens", height=2.4), flag)
    per = d.crop_y * d.crop_x
    n = d.n_patterns * per
    rng = np.random.default_rng(8)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = dev(rng.uniform(0.0, 1.0, pm_film_shape(d)).astype(np.float32))
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
    assert rel_l2(total, dose) < RTOL
    assert rel_l2(np.concatenate(parts), grad) < RTOL


@pytest.mark.parametrize("kind", ["telecentric", "lens"])
def test_single_pixel_stays_in_its_cone(kind):
    """One lit pixel at spp 256 deposits only within aperture_radius |1 - s / F| + pixel / 2 + one
    voxel diagonal of its chief ray (s: axial distance from the aperture plane; F = focus_distance
    + z_c for telecentric, focus_distance for lens)."""
    d = pm.projector_scene(kind)
    n = d.n_patterns * d.crop_y * d.crop_x
    row, col = 7, 15
    pat = np.zeros(n, np.float32)
    pat[row * d.crop_x + col] = 1.0  # angle 0
    proj = Projection(d, DEV)
    dose = proj.forward(dev(pat), None, 256, SEED).cpu().numpy()[..., 0]
    proj.close()
    z, y, x = np.nonzero(dose)
    assert z.size > 50
    h = [(d.bbox_max[a] - d.bbox_min[a]) / d.film_res[a] for a in range(3)]
    centres = np.stack([d.bbox_min[0] + (x + 0.5) * h[0], d.bbox_min[1] + (y + 0.5) * h[1],
                        d.bbox_min[2] + (z + 0.5) * h[2]], -1)
    cam = pm.to_camera(d, np.zeros(1), centres)
    xc, yc = pm.camera_xy(d, col, row, 0.5, 0.5)
    s = cam[:, 2]
    F = d.focus_distance + (pm.ZC if kind == "telecentric" else 0.0)
    chief = np.stack([np.full_like(s, xc), np.full_like(s, yc)], -1) if kind == "telecentric" else \
        np.stack([xc * s / F, yc * s / F], -1)
    off = np.linalg.norm(cam[:, :2] - chief, axis=-1)
    bound = d.aperture_radius * np.abs(1.0 - s / F) + 0.5 * d.pixel_size_x + float(np.linalg.norm(h))
    print(f"{kind}: {z.size} voxels, max offset / bound {np.max(off / bound):.3f}")
    assert np.all(off <= bound)
    # the cone is really there: off the focus plane the deposit is wider than a pixel
    assert off[np.abs(s - F) > 1.5].max() > 0.1


# --------------------------------------------------------------------------- 6. refusals
def _refused(d, match):
    with pytest.raises(ValueError, match=match):
        Projection(d, DEV)


def test_refusals_name_the_combination():
    Projection(pm.projector_scene("telecentric"), DEV).close()  # the runtime is up: refusals allocate nothing
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    for kind in ("telecentric", "lens"):
        base = pm.projector_scene(kind)
        pat = f"the '{kind}' projector with "
        d = base.copy()
        d.vial_type, d.vial_r_ext, d.vial_r = _abi.VIAL_CYLINDRICAL, 3.2, 2.9
        _refused(d, pat + "a 'cylindrical' vial")
        d.vial_type = _abi.VIAL_SQUARE
        _refused(d, pat + "a 'square' vial")
        d = base.copy()
        d.set_occluders(tri)
        _refused(d, pat + "occluders")
        d = base.copy()
        d.albedo = 0.5
        _refused(d, pat + "a scattering medium")
        d = base.copy()
        d.sensor_type, d.majorant = _abi.SENSOR_RATIO, 3.0
        _refused(d, pat + "the 'ratio' sensor")
        d = base.copy()
        d.sensor_type = _abi.SENSOR_DELTA
        _refused(d, pat + "the 'delta' sensor")
        d = base.copy()
        d.film_channels = 2
        d.set_target(tri)
        _refused(d, pat + "a surface-aware film")
        d = base.copy()
        d.slab_begin, d.slab_end = 0, 10
        _refused(d, pat + "film slabs")
        d = base.copy()
        d.focus_distance = 0.0
        _refused(d, "focus_distance must be positive")
        d = base.copy()
        d.aperture_radius = -1.0
        _refused(d, "aperture_radius must be >= 0")
    d = pm.projector_scene("lens")
    d.projector_type = 7
    _refused(d, "only the 'collimated', 'telecentric' and 'lens' projectors")
    assert torch.cuda.mem_get_info(0)[0] == free0


def test_unsupported_entry_points():
    d = pm.projector_scene("telecentric")
    proj = Projection(d, DEV)
    n = d.n_patterns * d.crop_y * d.crop_x
    out = torch.zeros(proj.film_shape, device=DEV)
    with pytest.raises(ValueError, match="cannot be split into slice ranges"):
        proj.forward_slices(torch.zeros(n, device=DEV), None, SPP, SEED, 0, 4, out)
    with pytest.raises(ValueError, match="planar plans only"):
        proj.adjoint_slices(out, n, 0, 4, 0, 4, torch.zeros(n, device=DEV))
    with pytest.raises(ValueError, match="filter_radon"):
        proj.radon(np.zeros((0, 3, 3), np.float32))
    m = np.empty(d.crop_y, np.int32)
    import ctypes
    assert proj.lib.tvam_row_slices(ctypes.byref(d), m.ctypes.data_as(ctypes.c_void_p)) == _abi.TVAM_ERR_UNSUPPORTED
    proj.close()
    # the export serves index-matched, non-scattering plans only
    from drtvam_amd.configs import cylindrical_refraction, desc_from_config
    cyl = Projection(desc_from_config(cylindrical_refraction(N=16, angles=4)), DEV)
    with pytest.raises(ValueError, match="tvam_plan_rays"):
        cyl.rays()
    cyl.close()


def test_kernel_time_records_the_forward():
    for flag, launches in ((_abi.FLAG_SCATTER_ATOMIC, 1), (_abi.FLAG_BIN_FIRST, 1)):
        d = with_flags(pm.projector_scene("telecentric"), flag)
        n = d.n_patterns * d.crop_y * d.crop_x
        proj = Projection(d, DEV)
        pat = torch.full((n,), 0.05, device=DEV)
        proj.kernel_time(True)
        proj.forward(pat, None, SPP, SEED)
        ms, k = proj.kernel_time(False)
        assert k == launches and ms > 0.0
        proj.close()

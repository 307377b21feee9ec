"""Projector derivatives on the GPU (tvam_dproj.hip): the tangent film
T = d dose / d theta (Projection.forward_dprojector) and the reverse-mode scalar g = <G, T>
(Projection.adjoint_dprojector) for theta in distance, focus_distance, aperture_radius, pixel_size,
against the float64 model's analytic tangents (dprojector_model.py, itself checked against central
differences in test_dprojector_model.py).

Active entries holding a ray whose margin is below dprojector_model.MARGIN (the ray may visit other
voxels in fp32 than in float64; at most 1 % of the rays) carry the pattern value 0 on both sides: they
cast no ray that counts.  Bars: dsigma_model's (relative L2 < 1e-4 and per voxel |dT| <= 1e-4
max |T_ref| for the film, |g - <G, T_ref>| <= 1e-4 <|G|, |T_ref|> for the scalar) and the dot-test
bar 1e-6 sum |G T_gpu| between the two GPU results."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.engine import Projection

import double_vial_model as dv
import dprojector_model as dpm
import dsigma_model as dm
import insert_model as im
import mesh_vial_model as mv
import projector_model as pm
import traced_vial_model as tv

DEV = "cuda:0"
SEED = 3


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _mixed():
    d = pm.projector_scene("telecentric", sample_time=True)
    d.clockwise = 1
    d.crop_x, d.crop_y, d.crop_offset_x, d.crop_offset_y = 19, 14, 3, 2
    return d


# name -> (descriptor, every k-th dense entry active (1: the dense set))
SCENES = {
    "telecentric": (lambda: pm.projector_scene("telecentric"), 1),
    "lens": (lambda: pm.projector_scene("lens"), 1),
    "lens-fov": (lambda: pm.projector_scene("lens", lens_fov=True), 1),
    "lens-regular": (lambda: pm.projector_scene("lens", regular=True), 1),
    "mixed-sparse": (_mixed, 3),
}
_REF = {}


def reference(name):
    """Per scene, computed once and left unchanged: the descriptor, the active set, the patterns
    (zero at the entries left out), the model's rays and a film gradient."""
    if name in _REF:
        return _REF[name]
    make, every = SCENES[name]
    d = make()
    spp = 1 if d.regular_sampling else 2
    n_dense = d.n_patterns * d.crop_y * d.crop_x
    keep = np.arange(0, n_dense, every)
    pix = pm.dense_pixels(d)[keep]
    streams = np.arange(keep.size)  # (a dense set's position is its dense index)
    tr = dpm.trace(d, pix, streams, spp, SEED)
    ok = dpm.keep_pixels(tr, spp)
    low = float((tr["margin"] < dpm.MARGIN).mean())
    assert low <= 0.01, low
    rng = np.random.default_rng(11)
    pat = rng.uniform(0.0, 0.1, keep.size).astype(np.float32)
    pat2 = rng.uniform(0.0, 0.1, keep.size).astype(np.float32)
    pat[~ok] = 0.0
    pat2[~ok] = 0.0
    G = rng.uniform(0.0, 1.0, dpm.film_shape(d)).astype(np.float32)
    _REF[name] = dict(desc=d, spp=spp, n=keep.size, pix=pix, streams=streams, sparse=every != 1, pat=pat, pat2=pat2,
                      G=G, low=low, vals=dpm.base_vals(d), T={})
    return _REF[name]


def model_tangent(R, param):
    """The model's tangent film of R's first pattern set (cached per scene and parameter)."""
    if param not in R["T"]:
        d = R["desc"]
        tr = dpm.trace(d, R["pix"], R["streams"], R["spp"], SEED, None, param)
        em = dpm.ray_em(d, R["pat"], R["spp"], R["n"])
        R["T"][param] = dpm.tangent_film(d, tr, em, R["vals"], param)
    return R["T"][param]


def gpu_pixels(R):
    return dev(R["pix"].astype(np.int32), torch.int32) if R["sparse"] else None


def gpu_film(proj, R, param, pat=None, seed=SEED):
    T = proj.forward_dprojector(param, dev(R["pat"] if pat is None else pat), gpu_pixels(R), R["spp"], seed)
    assert T.shape == proj.film_shape and T.dtype == torch.float32
    return T.cpu().numpy()[..., 0].astype(np.float64)


def check_film_and_scalar(R, T, T_ref, g, label):
    G64 = R["G"].astype(np.float64)
    l2, mx = dm.film_errors(T, T_ref)
    ref, scale = float(np.vdot(G64, T_ref)), float(np.vdot(np.abs(G64), np.abs(T_ref)))
    own, own_scale = float(np.vdot(G64, T)), float(np.abs(G64 * T).sum())
    print(f"{label}: {R['low']:.4%} of the rays left out; film rel L2 {l2:.3e} max / max {mx:.3e}; "
          f"g {g:.9e} <G, T_ref> {ref:.9e} (|diff| / <|G|,|T_ref|> {abs(g - ref) / scale:.2e}), "
          f"against the GPU film {abs(g - own) / own_scale:.2e}")
    assert np.abs(T_ref).max() > 0
    assert dm.film_ok(T, T_ref), (l2, mx)
    assert dm.scalar_ok(g, R["G"], T_ref)
    assert abs(g - own) <= 1e-6 * own_scale


# --------------------------------------------------------------------------- 1-2. film and scalar
@pytest.mark.parametrize("param", dpm.PARAMS)
@pytest.mark.parametrize("name", ["telecentric", "lens"])
def test_tangent_and_scalar_match_model(name, param):
    R = reference(name)
    proj = Projection(R["desc"], DEV)
    try:
        T = gpu_film(proj, R, param)
        g = proj.adjoint_dprojector(param, dev(R["pat"]), dev(R["G"]), None, R["spp"], SEED)
        g2 = proj.adjoint_dprojector(_abi.DPROJ_DISTANCE + dpm.PARAMS.index(param), dev(R["pat"]), dev(R["G"]), None,
                                     R["spp"], SEED)
        assert g.dim() == 0 and g.dtype == torch.float64
        assert g.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes()  # the same 8 bytes
        check_film_and_scalar(R, T, model_tangent(R, param), float(g), f"{name} {param}")
    finally:
        proj.close()


def test_lens_by_fov_chain_rule():
    """d / dF at fixed fov = T_F + (p / F) T_p, and d / dfov = (dp / dfov) T_p, from the entries'
    films and scalars against the model's."""
    R = reference("lens-fov")
    d = R["desc"]
    p_over_F, dp_dfov = dpm.fov_chain(d, R["vals"])
    proj = Projection(d, DEV)
    try:
        data, G = dev(R["pat"]), dev(R["G"])
        TF, Tp = gpu_film(proj, R, "focus_distance"), gpu_film(proj, R, "pixel_size")
        gF = float(proj.adjoint_dprojector("focus_distance", data, G, None, R["spp"], SEED))
        gp = float(proj.adjoint_dprojector("pixel_size", data, G, None, R["spp"], SEED))
        ref_F = model_tangent(R, "focus_distance") + p_over_F * model_tangent(R, "pixel_size")
        check_film_and_scalar(R, TF + p_over_F * Tp, ref_F, gF + p_over_F * gp, "lens by fov, focus_distance")
        check_film_and_scalar(R, dp_dfov * Tp, dp_dfov * model_tangent(R, "pixel_size"), dp_dfov * gp,
                              "lens by fov, fov")
    finally:
        proj.close()


# --------------------------------------------------------------------------- 3. linearity in the patterns
@pytest.mark.parametrize("name,param", [("telecentric", "aperture_radius"), ("lens", "pixel_size")])
def test_linear_in_the_patterns(name, param):
    R = reference(name)
    a, b = 0.75, -1.5  # (exact in fp32; a negative weight too)
    proj = Projection(R["desc"], DEV)
    try:
        T1, T2 = gpu_film(proj, R, param), gpu_film(proj, R, param, R["pat2"])
        mix = (np.float32(a) * R["pat"] + np.float32(b) * R["pat2"]).astype(np.float32)
        T12 = gpu_film(proj, R, param, mix)
        # per ray the products differ by one rounding of the mixed pattern and one of em * w; the rest
        # is the order of the float atomics
        assert np.abs(T12 - (a * T1 + b * T2)).max() <= 1e-5 * max(np.abs(T1).max(), np.abs(T2).max())
    finally:
        proj.close()


# --------------------------------------------------------------------------- 4-5. aperture_radius = 0
def test_zero_aperture():
    """aperture_radius = 0: the aperture draws move no ray, yet d / d aperture_radius is finite (and
    not zero: it is the derivative at R = 0 along each ray's disk sample).  With every ray parallel to
    the projector axis, moving the telecentric projector along that axis moves no deposit:
    d / d distance is zero to rounding.

    The bound.  Exactly, o' = -d, t0' = 1 and p' = o2' = 0, so every t' = 0.  If the tangent were
    formed in fp32, t0' would be 1 within 3 roundings and p' = o' + t0' d within 2 more, |p'| <= 5 U; the
    spawn offset adds less than U; a face's or the exit's t' divides by a direction cosine >= 0.5 (the
    angles are multiples of 60 degrees; axes the ray does not move along cross no face) or by the
    exit's >= 0.78 (|y| <= 1.8 inside r = 2.9): |t'| <= 16 U.  A visit's tangent s (e_b t_b' - e_a t_a')
    is then at most 2 s 16 U, a ray has at most rx + ry + rz visits, so
    sum_v |T[v]| <= 32 s U (rx + ry + rz) sum em.  (The kernel forms the tangent in fp64 and stays far
    below that.)"""
    d = pm.projector_scene("telecentric", aperture=0.0)
    spp = 2
    n = d.n_patterns * d.crop_y * d.crop_x
    pat = np.random.default_rng(11).uniform(0.0, 0.1, n).astype(np.float32)
    proj = Projection(d, DEV)
    try:
        data = dev(pat)
        TR = proj.forward_dprojector("aperture_radius", data, None, spp, SEED)
        assert bool(torch.isfinite(TR).all()) and float(TR.abs().max()) > 0
        gR = proj.adjoint_dprojector("aperture_radius", data, dev(np.ones(dpm.film_shape(d), np.float32)), None, spp, SEED)
        assert np.isfinite(float(gR))
        TD = proj.forward_dprojector("distance", data, None, spp, SEED).cpu().numpy().astype(np.float64)
        TF = proj.forward_dprojector("focus_distance", data, None, spp, SEED).cpu().numpy().astype(np.float64)
        em = dpm.ray_em(d, pat, spp, n)
        sig = float(np.float32(d.sigma_t))
        bound = 32 * sig * dm.U * sum(int(v) for v in d.film_res) * float(em.sum())
        print(f"aperture 0: sum |T_distance| {np.abs(TD).sum():.3e} <= {bound:.3e}; sum |T_aperture| "
              f"{float(TR.abs().sum()):.3e}; sum |T_focus| {np.abs(TF).sum():.3e}")
        assert np.abs(TD).sum() <= bound
        # (focus_distance moves nothing either at R = 0: its direction tangent is along the ray)
        assert float(TR.abs().sum()) > 100 * bound
    finally:
        proj.close()


# --------------------------------------------------------------------------- 6. crop, clockwise, sample_time, sparse
def test_crop_clockwise_sample_time_and_sparse_set():
    R = reference("mixed-sparse")
    assert R["sparse"] and R["desc"].sample_time and R["desc"].clockwise
    proj = Projection(R["desc"], DEV)
    try:
        for param in ("focus_distance", "aperture_radius"):
            T = gpu_film(proj, R, param)
            g = float(proj.adjoint_dprojector(param, dev(R["pat"]), dev(R["G"]), gpu_pixels(R), R["spp"], SEED))
            check_film_and_scalar(R, T, model_tangent(R, param), g, f"mixed-sparse {param}")
    finally:
        proj.close()


# --------------------------------------------------------------------------- 7. angle shards
@pytest.mark.parametrize("name,param", [("telecentric", "distance"), ("lens", "focus_distance")])
def test_angle_shards_sum_to_the_whole(name, param):
    R = reference(name)
    d, spp, n = R["desc"], R["spp"], R["n"]
    per = d.crop_y * d.crop_x
    T_ref = model_tangent(R, param)
    total, g = np.zeros(dpm.film_shape(d)), 0.0
    for a0, a1 in ((0, 3), (3, 6)):
        ds = d.copy()
        ds.angle_begin, ds.angle_end = a0, a1
        ds.active_base, ds.active_total = a0 * per, n
        sh = Projection(ds, DEV)
        data = dev(R["pat"][a0 * per:a1 * per])
        total += sh.forward_dprojector(param, data, None, spp, SEED).cpu().numpy()[..., 0]
        g += float(sh.adjoint_dprojector(param, data, dev(R["G"]), None, spp, SEED))
        sh.close()
    check_film_and_scalar(R, total, T_ref, g, f"{name} {param}, shards 0-3 + 3-6")


# --------------------------------------------------------------------------- 8. regular sampling
def test_regular_sampling():
    R = reference("lens-regular")
    assert R["spp"] == 1
    proj = Projection(R["desc"], DEV)
    try:
        T = gpu_film(proj, R, "aperture_radius")
        g = float(proj.adjoint_dprojector("aperture_radius", dev(R["pat"]), dev(R["G"]), None, 1, SEED))
        check_film_and_scalar(R, T, model_tangent(R, "aperture_radius"), g, "lens-regular aperture_radius")
    finally:
        proj.close()


# --------------------------------------------------------------------------- 9. refusals
def test_refusals_name_the_entry_and_allocate_nothing(tmp_path):
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    base = pm.projector_scene("collimated", regular=True)
    plans = [(base.copy(), "a collimated projector")]
    d = base.copy()
    d.albedo, d.phase_type = 0.5, _abi.PHASE_RAYLEIGH
    plans.append((d, "albedo > 0"))
    d = base.copy()
    d.sensor_type, d.majorant = _abi.SENSOR_RATIO, 3.0
    plans.append((d, "'ratio' / 'delta' sensors"))
    d = base.copy()
    d.film_channels = 2
    d.set_target(tri)
    plans.append((d, "surface-aware"))
    d = base.copy()
    d.slab_begin, d.slab_end = 0, 10
    plans.append((d, "film slab"))
    plans.append((dv.double_scene("collimated", regular=True), "a 'double_cylindrical' vial"))
    plans.append((tv.traced_scene("cylindrical", "telecentric"), "a traced 'cylindrical' vial"))
    plans.append((tv.traced_scene("square", "lens", regular=True), "a traced 'square' vial"))
    plans.append((mv.custom_scene("lens", "cuvette"), "a 'custom' vial"))
    plans.append((im.insert_scene(tmp_path, "index_matched", "telecentric", True), "dielectric occluders"))
    projs = [(Projection(d, DEV), why) for d, why in plans]
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for proj, why in projs:
            lib = proj.lib
            nd = proj.desc.n_patterns * proj.desc.crop_y * proj.desc.crop_x
            data = torch.zeros(nd, dtype=torch.float32, device=DEV)
            G = torch.zeros(proj.film_shape, dtype=torch.float32, device=DEV)
            T = torch.zeros(proj.film_shape, dtype=torch.float32, device=DEV)
            g = torch.zeros((), dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(0)[0]
            for param in range(4):
                with pytest.raises(ValueError) as e:
                    _abi.check(lib.tvam_forward_dprojector(proj._plan, param, data.data_ptr(), None, nd, 1, 0,
                                                           T.data_ptr(), stream))
                assert str(e.value).startswith("tvam_forward_dprojector: ") and why in str(e.value), str(e.value)
                with pytest.raises(ValueError) as e:
                    _abi.check(lib.tvam_adjoint_dprojector(proj._plan, param, data.data_ptr(), G.data_ptr(), None, nd,
                                                           1, 0, g.data_ptr(), stream))
                assert str(e.value).startswith("tvam_adjoint_dprojector: ") and why in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info(0)[0] == free0
    finally:
        for proj, _ in projs:
            proj.close()


def test_invalid_arguments():
    R = reference("telecentric")
    proj = Projection(R["desc"], DEV)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        data, G = dev(R["pat"]), dev(R["G"])
        T = torch.zeros(proj.film_shape, dtype=torch.float32, device=DEV)
        g = torch.zeros((), dtype=torch.float64, device=DEV)
        for param in (-1, 4):
            assert proj.lib.tvam_forward_dprojector(proj._plan, param, data.data_ptr(), None, R["n"], 2, 0, T.data_ptr(),
                                                    stream) == _abi.TVAM_ERR_INVALID
            assert b"tvam_forward_dprojector: param" in proj.lib.tvam_last_error()
            assert proj.lib.tvam_adjoint_dprojector(proj._plan, param, data.data_ptr(), G.data_ptr(), None, R["n"], 2, 0,
                                                    g.data_ptr(), stream) == _abi.TVAM_ERR_INVALID
            assert b"tvam_adjoint_dprojector: param" in proj.lib.tvam_last_error()
        assert proj.lib.tvam_forward_dprojector(proj._plan, 0, data.data_ptr(), None, R["n"], 2, 0, None,
                                                stream) == _abi.TVAM_ERR_INVALID
        assert proj.lib.tvam_adjoint_dprojector(proj._plan, 0, data.data_ptr(), None, None, R["n"], 2, 0, g.data_ptr(),
                                                stream) == _abi.TVAM_ERR_INVALID
        assert proj.lib.tvam_adjoint_dprojector(proj._plan, 0, data.data_ptr(), G.data_ptr(), None, R["n"], 2, 0, None,
                                                stream) == _abi.TVAM_ERR_INVALID
        with pytest.raises(KeyError):
            proj.forward_dprojector("fov", data, None, 2, 0)
    finally:
        proj.close()

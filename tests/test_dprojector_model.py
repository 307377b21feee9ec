"""The float64 model of the projector derivatives (dprojector_model.py) against
itself, on the CPU: its analytic per-ray, per-voxel tangents against central differences of its own
deposits in theta, the ray weight's share of the pixel-size derivative, the chain rule of a lens
configured by fov, the share of rays the GPU tests leave out, and the wiring of the two entries."""
import ctypes
import os

import numpy as np
import pytest

from drtvam_amd import _abi

import dprojector_model as dpm
import dsigma_model as dm
import projector_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3
SPP = 2
SCENES = {
    "telecentric": lambda: pm.projector_scene("telecentric"),
    "lens": lambda: pm.projector_scene("lens"),
    "lens-fov": lambda: pm.projector_scene("lens", lens_fov=True),
}
_TR = {}
# The finite-difference step: dsigma_model.fd_step's power of two, 2^-8 smaller.  At fd_step itself
# (2e-4 of theta) a ray's lateral shift is ~4e-3 of a voxel, and with ~60 face crossings per ray one
# ray in six changes the order of two crossings somewhere; at 2^-8 of it fewer than 0.1 % do, and the
# differences at h and 2 h still agree to better than 1e-8 (float64 deposits).
H_SCALE = 2.0 ** -8


def dense(d):
    return pm.dense_pixels(d), np.arange(d.n_patterns * d.crop_y * d.crop_x)


def traced(name, param=None):
    """The scene's dense rays at its own parameters, computed once per (scene, param)."""
    if (name, param) not in _TR:
        d = SCENES[name]()
        pix, st = dense(d)
        _TR[name, param] = (d, dpm.trace(d, pix, st, SPP, SEED, None, param))
    return _TR[name, param]


# --------------------------------------------------------------------------- 1. analytic tangents against FD
@pytest.mark.parametrize("param", dpm.PARAMS)
@pytest.mark.parametrize("name", ["telecentric", "lens"])
def test_analytic_tangents_match_central_differences(name, param):
    """Per ray and voxel visit, over the rays whose visit sequence is the same at theta, theta +- h and
    theta +- 2 h (at most 1 % are left out).  The step (H_SCALE) is accepted by dsigma_model's two-step
    check, the central differences at h and 2 h agreeing to 1e-5; the analytic tangent then has to
    agree with the one at h to the same 1e-5 (its truncation error is a third of that)."""
    d, tr = traced(name, param)
    assert tr["hit"].all() and tr["ok"].mean() > 0.5
    pix, st = dense(d)
    v0 = dpm.base_vals(d)
    h = dm.fd_step(dpm.theta_of(v0, param)) * H_SCALE
    at = {m: dpm.trace(d, pix, st, SPP, SEED, dpm.moved(v0, param, m * h)) for m in (-2, -1, 1, 2)}
    K = max(t["vox"].shape[1] for t in list(at.values()) + [tr])
    same = dpm.same_sequence([tr] + list(at.values()))
    left_out = 1.0 - same.mean()
    T_h = (dpm.padded(at[1]["dep"], K) - dpm.padded(at[-1]["dep"], K))[same] / (2 * h)
    T_2h = (dpm.padded(at[2]["dep"], K) - dpm.padded(at[-2]["dep"], K))[same] / (4 * h)
    conv = dm.assert_converged(T_h, T_2h)
    T = dpm.padded(tr["tan"], K)[same]
    l2, mx = dm.film_errors(T, T_h)
    print(f"{name} {param}: h {h:.3e}, {left_out:.4%} of the rays left out, FD convergence {conv:.2e}, "
          f"analytic against FD rel L2 {l2:.2e} max / max {mx:.2e}")
    assert left_out <= 0.01
    assert np.abs(T).max() > 0
    assert l2 <= 1e-5 and mx <= 1e-5


# --------------------------------------------------------------------------- 2. the weight term
@pytest.mark.parametrize("name", ["telecentric", "lens"])
def test_pixel_size_weight_term(name):
    d, tr = traced(name, "pixel_size")
    n = d.n_patterns * d.crop_y * d.crop_x
    pat = np.random.default_rng(5).uniform(0.0, 0.1, n).astype(np.float32)
    v0 = dpm.base_vals(d)
    em = dpm.ray_em(d, pat, SPP, n)
    T = dpm.tangent_film(d, tr, em, v0, "pixel_size")
    geometric = dpm.scatter(d, tr, em[:, None] * tr["tan"])
    dose = dpm.dose_film(d, tr, em)
    want = (1.0 / v0["pixel_size_x"] + 1.0 / v0["pixel_size_y"]) * dose.sum()
    assert want > 0 and abs((T.sum() - geometric.sum()) - want) <= 1e-12 * want
    # ... and the whole film derivative against the FD of the dose, the ray weight included
    pix, st = dense(d)
    h = dm.fd_step(v0["pixel_size_x"]) * H_SCALE

    def dose_at(m):
        v = dpm.moved(v0, "pixel_size", m * h)
        return dpm.dose_film(d, dpm.trace(d, pix, st, SPP, SEED, v), dpm.ray_em(d, pat, SPP, n, v))

    fd = (dose_at(1) - dose_at(-1)) / (2 * h)
    # (rays that change their visit sequence between theta - h and theta + h move dose from a voxel
    # to its neighbour: the sum over the film sees the derivative alone)
    assert abs(T.sum() - fd.sum()) <= 1e-5 * np.abs(fd).sum()


# --------------------------------------------------------------------------- 3. lens by fov
def test_lens_fov_chain_rule_matches_fd_in_focus_with_fov_held():
    """d / dF at fixed fov = d_F + (p / F) d_p, per ray and visit, against the FD of the deposits at
    F +- h with p = 2 F tan(fov / 2) / res_x re-derived."""
    d, trF = traced("lens-fov", "focus_distance")
    _, trp = traced("lens-fov", "pixel_size")
    pix, st = dense(d)
    v0 = dpm.base_vals(d)
    p_over_F, dp_dfov = dpm.fov_chain(d, v0)
    assert abs(dp_dfov - (np.pi / 180) * (v0["focus_distance"] + (v0["pixel_size_x"] * d.res_x / 2) ** 2
                                          / v0["focus_distance"]) / d.res_x) <= 1e-12
    h = dm.fd_step(v0["focus_distance"]) * H_SCALE

    def at(m):
        F = v0["focus_distance"] + m * h
        v = dict(v0, focus_distance=F, pixel_size_x=v0["pixel_size_x"] * F / v0["focus_distance"],
                 pixel_size_y=v0["pixel_size_y"] * F / v0["focus_distance"])
        return dpm.trace(d, pix, st, SPP, SEED, v)

    tr = {m: at(m) for m in (-2, -1, 1, 2)}
    K = max(t["vox"].shape[1] for t in list(tr.values()) + [trF])
    same = dpm.same_sequence([trF] + list(tr.values()))
    assert 1.0 - same.mean() <= 0.01
    T_h = (dpm.padded(tr[1]["dep"], K) - dpm.padded(tr[-1]["dep"], K))[same] / (2 * h)
    T_2h = (dpm.padded(tr[2]["dep"], K) - dpm.padded(tr[-2]["dep"], K))[same] / (4 * h)
    dm.assert_converged(T_h, T_2h)
    T = dpm.padded(trF["tan"] + p_over_F * trp["tan"], K)[same]
    l2, mx = dm.film_errors(T, T_h)
    print(f"lens by fov: chain rule against FD rel L2 {l2:.2e} max / max {mx:.2e}")
    assert l2 <= 1e-5 and mx <= 1e-5


# --------------------------------------------------------------------------- 4. the rays the GPU tests leave out
@pytest.mark.parametrize("name", list(SCENES))
def test_few_rays_are_near_a_decision(name):
    d, tr = traced(name)
    low = float((tr["margin"] < dpm.MARGIN).mean())
    half = 0.5 * float(np.float32(d.vial_height))
    print(f"{name}: {low:.4%} of {tr['margin'].size} rays below margin {dpm.MARGIN}")
    assert tr["margin"].size == 5760 and tr["hit"].all()
    assert low <= 0.01
    pix, st = dense(d)
    m = pm.model_rays(d, pix, st, SPP, SEED)
    assert m["hit"].all() and m["margin"].min() > 18.0 and half == 20.0
    # the model's rays are projector_model's
    R = dpm._rays(d, pix, st, SPP, SEED, dpm.base_vals(d), None)
    assert np.abs(R["o2"] - m["o2"]).max() <= 1e-12 and np.abs(R["maxt"] - m["maxt"]).max() <= 1e-12


# --------------------------------------------------------------------------- 5. wiring
def test_entries_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "tvam.h")).read()
    lib = _abi.load_library()
    for name in ("tvam_forward_dprojector", "tvam_adjoint_dprojector"):
        assert f"int {name}(" in header
        assert name in _abi.EXPORTS
        assert getattr(lib, name) is not None
    for i, name in enumerate(("DISTANCE", "FOCUS_DISTANCE", "APERTURE_RADIUS", "PIXEL_SIZE")):
        assert getattr(_abi, "DPROJ_" + name) == i
        assert any(line.split() == ["#define", "TVAM_DPROJ_" + name, str(i)] for line in header.splitlines())
        assert dpm.PARAMS[i] == name.lower()
    assert "#define TVAM_ABI_VERSION 13" in header
    assert _abi.ABI_VERSION == 13 and lib.tvam_abi_version() == 13
    # null pointers are refused by message, without touching a GPU
    assert lib.tvam_forward_dprojector(None, 0, None, None, 0, 1, 0, None, None) == _abi.TVAM_ERR_INVALID
    assert b"tvam_forward_dprojector" in lib.tvam_last_error()
    assert lib.tvam_adjoint_dprojector(None, 0, None, None, None, 0, 1, 0, None, None) == _abi.TVAM_ERR_INVALID
    assert b"tvam_adjoint_dprojector" in lib.tvam_last_error()


# --------------------------------------------------------------------------- 6. scenes
@pytest.mark.parametrize("kind,fov", [("telecentric", False), ("lens", False), ("lens", True)])
def test_projector_config_is_the_projector_scene(kind, fov):
    from drtvam_amd.configs import desc_from_config
    a, b = desc_from_config(dpm.projector_config(kind, fov)), pm.projector_scene(kind, lens_fov=fov)
    assert bytes(memoryview(a).cast("B")) == bytes(memoryview(b).cast("B"))


def _scene(kind, fov):
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict
    cfg = dpm.projector_config(kind, fov)
    cfg["projector"]["device"] = "cpu"
    return load_dict(load_scene(cfg))


@pytest.mark.parametrize("kind,fov", [("telecentric", False), ("lens", False), ("lens", True)])
def test_traverse_exposes_the_calibration_and_update_writes_it_back(kind, fov):
    import torch
    from drtvam_amd.scene import traverse
    scene = _scene(kind, fov)
    p = scene.projector
    before = (p.motion.distance, p.focus_distance, p.aperture_radius, p.pixel_size, getattr(p, "fov", None))
    params = traverse(scene)
    last = "projector.fov" if fov else "projector.pixel_size"
    assert set(params) == {"projector.active_data", "projector.active_pixels", "printing_medium.sigma_t",
                           "projector.distance", "projector.focus_distance", "projector.aperture_radius", last}
    params.update()  # the projector's own values, rounded to float32: nothing moves
    assert before == (p.motion.distance, p.focus_distance, p.aperture_radius, p.pixel_size, getattr(p, "fov", None))
    params["projector.distance"] = torch.tensor(21.0)
    params["projector.focus_distance"] = 19.0
    params["projector.aperture_radius"] = torch.tensor(1.5, requires_grad=True)
    params.update()
    assert (p.motion.distance, p.focus_distance, p.aperture_radius) == (21.0, 19.0, 1.5)
    assert scene.projector_params["aperture_radius"].requires_grad
    if kind == "telecentric":
        assert p.pixel_size == before[3]
        params[last] = 0.2
        params.update()
        assert p.pixel_size == (float(np.float32(0.2)),) * 2 and p.emitter_size == (24 * p.pixel_size[0], 20 * p.pixel_size[1])
    elif fov:  # the pixel size follows focus_distance at the fov held
        assert abs(p.pixel_size - before[3] * 19.0 / 20.0) <= 1e-12 and p.fov == before[4]
        assert p.dproj_terms("focus_distance") == [("focus_distance", 1.0), ("pixel_size", p.pixel_size / 19.0)]
        (name, c), = p.dproj_terms("fov")
        assert name == "pixel_size" and abs(c - dpm.fov_chain(scene.integrator.desc(scene, scene.sensor_by_id("sensor")),
                                                              dict(focus_distance=19.0, pixel_size_x=p.pixel_size))[1]) <= 1e-12
    else:  # the fov follows
        assert p.pixel_size == before[3] and p.fov != before[4]
        assert p.dproj_terms("focus_distance") == [("focus_distance", 1.0)]
    with pytest.raises(ValueError, match="0-dim"):
        params["projector.distance"] = torch.ones(1)
        params.update()


def test_collimated_scene_keeps_its_three_keys():
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict, traverse
    cfg = dm.collimated_config()
    cfg["projector"]["device"] = "cpu"
    scene = load_dict(load_scene(cfg))
    assert set(traverse(scene)) == {"projector.active_data", "projector.active_pixels", "printing_medium.sigma_t"}
    assert scene.projector_params == {}


def test_fit_model_converges_from_the_starts_the_gpu_test_uses():
    """The starts of test_gpu_dprojector_fit.py: 0.9 / 1.1 theta* for aperture_radius, narrowed to
    0.99 / 1.01 theta* for focus_distance and distance (from 0.9 / 1.1 the loop does not converge)."""
    for kind, fov in (("telecentric", False), ("lens", True)):
        d = pm.projector_scene(kind, lens_fov=fov)
        v0 = dpm.base_vals(d)
        for name, fs in (("aperture_radius", (0.9, 1.1)), ("focus_distance", (0.99, 1.01)), ("distance", (0.99, 1.01))):
            for f in fs:
                err = [abs(t / v0[name] - 1.0) for t in dpm.fit_model(d, name, f * v0[name], 8, by_fov=fov)]
                assert min(err) <= 1e-5, (kind, name, f, err)
        err = [abs(t / v0["distance"] - 1.0) for t in dpm.fit_model(d, "distance", 0.9 * v0["distance"], 8, by_fov=fov)]
        assert err[-1] > 1e-2

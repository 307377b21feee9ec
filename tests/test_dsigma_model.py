"""Extinction derivative, CPU side: the fp32 visit weight of the library's host entry against float64
with a derived bound (dsigma_model.weight_bound), the finite-difference checker and its tolerance
applied to a stand-in with one deliberate defect each (they must fail), and the wiring of the three
entries through the header, the binding and traverse()."""
import ctypes
import os

import numpy as np
import pytest

from drtvam_amd import _abi

import dsigma_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tvam_forward_dsigma", "tvam_adjoint_dsigma", "tvam_dsigma_weights")


# --------------------------------------------------------------------------- the weight
@pytest.mark.parametrize("s", [0.03, 1.0, 7.5])
def test_weight_within_derived_bound(s):
    """s dt over [1e-7, 5] (both branches of tvam_omexp, and its threshold from both sides), s T0
    over [0, 20], and dt = 0."""
    sdt = np.concatenate([np.geomspace(1e-7, 5.0, 400), [0.05, np.nextafter(np.float32(0.05), np.float32(0)), 0.0]])
    sT0 = np.concatenate([[0.0], np.geomspace(1e-3, 20.0, 300), [1.0]])
    dt, T0 = np.meshgrid((sdt / s).astype(np.float32), (sT0 / s).astype(np.float32))
    w = _abi.dsigma_weights(s, T0, dt).astype(np.float64)
    ref = dm.w_exact(s, T0, dt)
    bound = dm.weight_bound(s, T0, dt)
    err = np.abs(w - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"sigma {s}: max |w - w64| / bound = {worst:.3f}, max relative error {float(np.max(err[ref != 0] / np.abs(ref[ref != 0]))):.3e}")
    assert np.all(err <= bound), worst
    assert not np.any(w[dt == 0])  # a visit of no length deposits nothing


def test_weight_sign_change_and_entry_value():
    s = np.float32(1.0)
    dt = np.float32(0.01)
    # w'(0, dt) = dt e^{-s dt}
    w0 = float(_abi.dsigma_weights(s, np.float32(0.0), dt))
    ref0 = float(dt) * np.exp(-float(s) * float(dt))
    assert abs(w0 - ref0) <= float(dm.weight_bound(s, 0.0, dt))
    # the sign changes where (T0 + dt) e^{-s dt} = T0, i.e. s T0 = s dt / (e^{s dt} - 1) ~ 1 - s dt / 2
    T0 = np.linspace(0.9, 1.1, 2001).astype(np.float32)
    w = _abi.dsigma_weights(s, T0, dt)
    root = float(dt) / np.expm1(float(s) * float(dt))
    assert np.all(w[T0 < root - 1e-4] > 0) and np.all(w[T0 > root + 1e-4] < 0)
    assert abs(root - (1.0 - 0.005)) < 1e-4


def test_weights_broadcast_and_empty():
    w = _abi.dsigma_weights(1.0, np.zeros((3, 1), np.float32), np.full((1, 4), 0.1, np.float32))
    assert w.shape == (3, 4) and w.dtype == np.float32
    assert _abi.dsigma_weights(1.0, np.zeros(0, np.float32), np.zeros(0, np.float32)).shape == (0,)


# --------------------------------------------------------------------------- the checker checks
def _stand_in_reference(sigma):
    st = dm.StandIn()
    T_h, T_2h = dm.fd_tangent(st.dose, sigma)
    dm.assert_converged(T_h, T_2h)
    return st, T_h


def test_checker_accepts_the_correct_stand_in():
    st, T_ref = _stand_in_reference(1.0)
    assert (T_ref > 0).any() and (T_ref < 0).any()
    T = st.tangent(1.0)
    print("stand-in errors (rel L2, max / max):", dm.film_errors(T, T_ref))
    assert dm.film_ok(T, T_ref)
    G = np.random.default_rng(3).uniform(0, 1, T.shape)
    assert dm.scalar_ok(np.vdot(G, T), G, T_ref)


@pytest.mark.parametrize("defect", ["grid_entry", "no_T0q", "no_E0"])
def test_checker_rejects_each_defect(defect):
    st, T_ref = _stand_in_reference(1.0)
    T = st.tangent(1.0, defect)
    print(defect, dm.film_errors(T, T_ref))
    assert not dm.film_ok(T, T_ref)
    G = np.random.default_rng(3).uniform(0, 1, T.shape)
    assert not dm.scalar_ok(np.vdot(G, T), G, T_ref)


def test_unconverged_reference_is_refused():
    """A step too coarse for the 1e-5 bar must not pass as ground truth."""
    st = dm.StandIn()
    h = 2.0 ** -3
    T = [(st.dose(1.0 + m * h) - st.dose(1.0 - m * h)) / (2 * m * h) for m in (1, 2)]
    with pytest.raises(AssertionError):
        dm.assert_converged(T[0], T[1])


def test_fd_step_is_exact_in_fp32():
    for sigma, h in ((1.0, 2.0 ** -12), (1.75, 2.0 ** -12), (0.5, 2.0 ** -13), (0.06, 2.0 ** -17)):
        assert dm.fd_step(np.float32(sigma)) == h


# --------------------------------------------------------------------------- ABI and wiring
def test_entries_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "tvam.h")).read()
    lib = _abi.load_library()
    for name in NAMES:
        assert f"int {name}(" in header
        assert name in _abi.EXPORTS
        assert getattr(lib, name) is not None
    assert "#define TVAM_ABI_VERSION 13" in header
    assert _abi.ABI_VERSION == 13 and lib.tvam_abi_version() == 13
    # the host entry refuses null arrays by message, without touching a GPU
    assert lib.tvam_dsigma_weights(ctypes.c_float(1.0), None, None, 4, None) == _abi.TVAM_ERR_INVALID
    assert b"tvam_dsigma_weights" in lib.tvam_last_error()


def _scene(sigma=1.0):
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict
    cfg = dm.collimated_config()
    cfg["projector"]["device"] = "cpu"
    cfg["vial"]["medium"]["extinction"] = sigma
    return load_dict(load_scene(cfg))


def test_collimated_config_is_the_projector_scene():
    import projector_model as pm
    from drtvam_amd.configs import desc_from_config
    a, b = desc_from_config(dm.collimated_config(True)), pm.projector_scene("collimated", regular=True)
    assert bytes(memoryview(a).cast("B")) == bytes(memoryview(b).cast("B"))


def test_traverse_exposes_sigma_t_and_update_writes_it_back():
    import torch
    from drtvam_amd.integrators import VolumeIntegrator
    from drtvam_amd.scene import traverse
    scene = _scene(0.75)
    params = traverse(scene)
    assert set(params) == {"projector.active_data", "projector.active_pixels", "printing_medium.sigma_t"}
    s = params["printing_medium.sigma_t"]
    assert s.dim() == 0 and s.dtype == torch.float32 and float(s) == 0.75
    integ = VolumeIntegrator({"regular_sampling": True})
    sensor = scene.sensor_by_id("sensor")
    assert integ.desc(scene, sensor).sigma_t == 0.75
    params["printing_medium.sigma_t"] = torch.tensor(1.25, dtype=torch.float32)
    params.update()
    assert scene.container.sigma_t == 1.25 and integ.desc(scene, sensor).sigma_t == 1.25
    params.update({"printing_medium.sigma_t": torch.tensor(0.5)})
    assert integ.desc(scene, sensor).sigma_t == 0.5
    with pytest.raises(ValueError, match="0-dim"):
        params.update({"printing_medium.sigma_t": torch.ones(2)})

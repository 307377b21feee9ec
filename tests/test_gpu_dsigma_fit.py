"""Fitting the resin's extinction to a dose, end to end: D* = forward(p) at sigma* = 1 / mm on
projector_model.projector_scene('collimated', regular=True), then Gauss-Newton on sigma alone,
    sigma <- fp32(sigma - <D - D*, T> / <T, T>),   T = d dose / d sigma_t (render_forward's sigma tangent),
through traverse / update and the integrator's plan cache: every step renders at a new sigma, so it
builds a new plan, and the plans of earlier steps are evicted.

The same loop on the float64 oracle with a finite-difference tangent reaches sigma* exactly in fp32
from 1.75 in 4 steps (errors 0.21, 7.7e-3, 1.8e-5, 0) and from 0.5 in 3.  A step maps the error e to
O(e^2) + eps_T e with eps_T <= 1e-4, the tangent's bar (test_gpu_dsigma.py), so 6 steps leave two
steps of margin for |sigma - sigma*| <= 1e-5 sigma*."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dsigma_model as dm

DEV = "cuda:0"
SIGMA_STAR = 1.0


def _scene():
    from drtvam_amd.integrators import VolumeIntegrator
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict
    cfg = dm.collimated_config(regular=True)
    cfg["projector"]["device"] = DEV
    scene = load_dict(load_scene(cfg))
    return scene, scene.sensor_by_id("sensor"), VolumeIntegrator({"regular_sampling": True, "max_depth": 6, "rr_depth": 6})


def test_scene_level_gradient_and_tangent():
    """scene.render differentiates with respect to traverse()'s sigma_t, render_backward accumulates
    the same scalar into its .grad, and render_forward adds the sigma tangent to the pattern tangent:
    each against the Projection's own entries."""
    from drtvam_amd.scene import render, traverse
    scene, sensor, integ = _scene()
    params = traverse(scene)
    n = scene.projector.active_size()
    rng = np.random.default_rng(9)
    pat = torch.as_tensor(rng.uniform(0.0, 0.1, n).astype(np.float32), device=DEV)
    tan = torch.as_tensor(rng.uniform(-1.0, 1.0, n).astype(np.float32), device=DEV)
    params["projector.active_data"] = pat
    sig = torch.tensor(1.0, dtype=torch.float32, requires_grad=True)
    params["printing_medium.sigma_t"] = sig
    params.update()
    proj = integ.projection(scene, sensor)
    G = torch.as_tensor(rng.uniform(0.0, 1.0, proj.film_shape).astype(np.float32), device=DEV)
    want = float(proj.adjoint_dsigma(pat, G, None, 1, 0))

    dose = render(scene, params, integrator=integ, sensor=sensor, spp=1, seed=0, seed_grad=0)
    assert dose.requires_grad and not pat.requires_grad
    (dose * G).sum().backward()
    assert sig.grad.dtype == torch.float32 and sig.grad.dim() == 0
    assert abs(float(sig.grad) - want) <= 2.0 ** -23 * abs(want)  # the f64 scalar rounded to the parameter's fp32

    sig.grad = None
    params["projector.active_data"] = pat.clone().requires_grad_(True)
    params.update()
    integ.render_backward(scene, params, G, sensor, seed=0, spp=1)
    integ.render_backward(scene, params, G, sensor, seed=0, spp=1)  # accumulates
    assert abs(float(sig.grad) - 2 * want) <= 2.0 ** -22 * abs(want)
    g_pat = 2 * proj.adjoint(G, n, None, 1, 0).double()
    assert float(torch.linalg.norm(scene.projector.active_data.grad.double() - g_pat) / torch.linalg.norm(g_pat)) < 1e-6

    T = proj.forward_dsigma(pat, None, 1, 0).double()
    A = proj.forward(tan, None, 1, 0).double()
    scene.projector.active_data.grad = None
    only_sigma = integ.render_forward(scene, params, sensor, seed=0, spp=1, tangent_sigma_t=0.5).double()
    both = integ.render_forward(scene, params, sensor, seed=0, spp=1, tangent=tan, tangent_sigma_t=0.5).double()
    only_pattern = integ.render_forward(scene, params, sensor, seed=0, spp=1, tangent=tan).double()
    scale = float(T.abs().max())
    assert float((only_sigma - 0.5 * T).abs().max()) <= 1e-5 * scale  # (the atomics' order differs between calls)
    assert float((both - (A + 0.5 * T)).abs().max()) <= 1e-5 * max(scale, float(A.abs().max()))
    assert float((only_pattern - A).abs().max()) <= 1e-6 * float(A.abs().max())
    assert len(integ._plans) == 1


@pytest.mark.parametrize("start", [1.75, 0.5])
def test_gauss_newton_recovers_sigma(start):
    from drtvam_amd.scene import traverse
    scene, sensor, integ = _scene()
    params = traverse(scene)
    assert float(params["printing_medium.sigma_t"]) == SIGMA_STAR
    n = scene.projector.active_size()
    pat = np.random.default_rng(5).uniform(0.0, 0.1, n).astype(np.float32)
    params["projector.active_data"] = torch.as_tensor(pat, device=DEV)
    params.update()
    target = integ.render(scene, sensor, seed=0, spp=1).double().clone()
    assert float(target.abs().max()) > 0

    sigma = np.float32(start)
    errors = []
    for _ in range(6):
        params["printing_medium.sigma_t"] = torch.tensor(float(sigma), dtype=torch.float32)
        params.update()
        dose = integ.render(scene, sensor, seed=0, spp=1).double()
        T = integ.render_forward(scene, params, sensor, seed=0, spp=1, tangent_sigma_t=1.0).double()
        step = float(((dose - target) * T).sum() / (T * T).sum())
        sigma = np.float32(float(sigma) - step)
        errors.append(abs(float(sigma) - SIGMA_STAR))
        assert len(integ._plans) == 1  # the plans of earlier sigmas are closed, not kept
    print(f"from {start}: errors {['%.2e' % e for e in errors]}")
    assert errors[-1] <= 1e-5 * SIGMA_STAR
    assert len(integ._plans) == 1

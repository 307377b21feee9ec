"""Projector derivatives at the scene level, and calibrating a projector with them.

1. traverse / update / render / render_backward / render_forward on the shared projector scenes
   (dprojector_model.projector_config), each against the Projection's own entries.

2. Calibration as the reference's tutorial sets it up: one pattern with 8 lit pixels (a sparse active
   set), spp 64, D* = render at theta*.  Then one-parameter Gauss-Newton
       theta <- fp32(theta - <D - D*, T> / <T, T>),   T = d dose / d theta (render_forward's projector tangent),
   for aperture_radius, focus_distance and distance in turn, through traverse / update and the
   integrator's plan cache, on the telecentric scene and on the lens configured by fov (whose pixel
   size follows focus_distance).

   The same loop on the float64 model (dprojector_model.fit_model), |theta / theta* - 1| per step:
     telecentric aperture_radius  from 0.9: 6.2e-2 3.0e-2 7.8e-3 6.6e-4 2.8e-6;  from 1.1: 6.0e-2 2.7e-2 5.4e-3 7.3e-5 8.3e-9
     lens        aperture_radius  from 0.9: 7.3e-2 4.3e-2 1.9e-2 5.4e-3 6.6e-4 7.3e-6;
                                  from 1.1: 6.7e-2 3.4e-2 1.4e-2 5.3e-3 5.2e-3 5.0e-3 4.9e-4 2.5e-6
   From 0.9 theta* and 1.1 theta* the loop does not converge for focus_distance and distance on either
   projector (2 mm is 20 voxels: the eight beams no longer overlap their targets, and the error creeps by
   ~3e-3 per step).  Their starts are narrowed to 0.99 theta* and 1.01 theta* (0.2 mm, two voxels):
     telecentric focus_distance   from 0.99: 6.1e-3 2.9e-3 7.0e-4 4.6e-5 8.1e-8;  from 1.01: 6.3e-3 3.2e-3 8.1e-4 3.8e-5 1.3e-7
     telecentric distance         from 0.99: 6.7e-3 3.7e-3 1.2e-3 1.4e-4 9.8e-7;  from 1.01: 6.2e-3 3.2e-3 9.0e-4 7.4e-5 4.6e-7
     lens by fov focus_distance   from 0.99: 6.7e-3 4.2e-3 2.0e-3 6.3e-4 4.1e-5 6.2e-7;  from 1.01: 7.7e-3 4.8e-3 2.6e-3 2.0e-3 6.0e-4 8.5e-5 1.0e-6
     lens by fov distance         from 0.99: 6.6e-3 3.7e-3 1.1e-3 1.4e-4 5.8e-7;  from 1.01: 6.5e-3 3.4e-3 9.9e-4 8.3e-5 9.3e-7
   The test runs the model's loop itself: the number of steps is the model's first with
   |theta - theta*| <= 1e-5 theta*, the GPU gets two more, and has to meet the same bar."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dprojector_model as dpm
import projector_model as pm

DEV = "cuda:0"
BAR = 1e-5


def _scene(kind, lens_fov=False):
    from drtvam_amd.integrators import VolumeIntegrator
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict
    cfg = dpm.projector_config(kind, lens_fov)
    cfg["projector"]["device"] = DEV
    scene = load_dict(load_scene(cfg))
    return scene, scene.sensor_by_id("sensor"), VolumeIntegrator({"max_depth": 6, "rr_depth": 6})


def test_traverse_keys():
    from drtvam_amd.scene import traverse
    base = {"projector.active_data", "projector.active_pixels", "printing_medium.sigma_t"}
    cal = {"projector.distance", "projector.focus_distance", "projector.aperture_radius"}
    for kind, fov, last in (("telecentric", False, "projector.pixel_size"), ("lens", False, "projector.pixel_size"),
                            ("lens", True, "projector.fov")):
        params = traverse(_scene(kind, fov)[0])
        assert set(params) == base | cal | {last}
        for k in cal | {last}:
            assert params[k].dim() == 0 and params[k].dtype == torch.float32 and params[k].device.type == "cpu"
        assert float(params["projector.distance"]) == 20.0 and float(params["projector.aperture_radius"]) == 2.0
    import dsigma_model as dm
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict
    cfg = dm.collimated_config()
    cfg["projector"]["device"] = DEV
    assert set(traverse(load_dict(load_scene(cfg)))) == base


@pytest.mark.parametrize("kind,fov", [("telecentric", False), ("lens", True)])
def test_scene_level_gradient_and_tangent(kind, fov):
    """scene.render differentiates with respect to traverse()'s projector parameters, render_backward
    accumulates the same scalars into their .grad, and render_forward adds the projector tangents to
    the pattern tangent: each against the Projection's own entries (a lens by fov through the chain
    rule d / dF = d_F + (p / F) d_p, d / dfov = (pi / 180) F sec^2(fov / 2) / res_x d_p)."""
    from drtvam_amd.scene import render, traverse
    scene, sensor, integ = _scene(kind, fov)
    params = traverse(scene)
    n = scene.projector.active_size()
    rng = np.random.default_rng(9)
    pat = torch.as_tensor(rng.uniform(0.0, 0.1, n).astype(np.float32), device=DEV)
    tan = torch.as_tensor(rng.uniform(-1.0, 1.0, n).astype(np.float32), device=DEV)
    params["projector.active_data"] = pat
    last = "fov" if fov else "pixel_size"
    names = ("distance", "focus_distance", "aperture_radius", last)
    for name in names:
        params["projector." + name] = params["projector." + name].clone().requires_grad_(True)
    params.update()
    proj = integ.projection(scene, sensor)
    desc = pm.projector_scene(kind, lens_fov=fov)
    for field in ("distance", "focus_distance", "aperture_radius", "pixel_size_x", "pixel_size_y"):
        assert getattr(proj.desc, field) == getattr(desc, field)  # update() moved nothing
    G = torch.as_tensor(rng.uniform(0.0, 1.0, proj.film_shape).astype(np.float32), device=DEV)
    raw = {p: float(proj.adjoint_dprojector(p, pat, G, None, 2, 0)) for p in dpm.PARAMS}
    p_over_F, dp_dfov = dpm.fov_chain(desc, dpm.base_vals(desc))
    want = {"distance": raw["distance"], "aperture_radius": raw["aperture_radius"]}
    if fov:
        want["focus_distance"] = raw["focus_distance"] + p_over_F * raw["pixel_size"]
        want["fov"] = dp_dfov * raw["pixel_size"]
    else:
        want["focus_distance"], want["pixel_size"] = raw["focus_distance"], raw["pixel_size"]
    # (the chain's coefficients come from the projector's float64 fov and the model's float32 pixel size)
    tol = lambda name: (1e-6 if fov else 2.0 ** -22) * (abs(raw["focus_distance"]) + abs(p_over_F * raw["pixel_size"])
                                                      if name == "focus_distance" else abs(want[name]))

    dose = render(scene, params, integrator=integ, sensor=sensor, spp=2, seed=0, seed_grad=0)
    assert dose.requires_grad and not pat.requires_grad
    (dose * G).sum().backward()
    for name in names:
        g = params["projector." + name].grad
        assert g.dtype == torch.float32 and g.dim() == 0
        assert abs(float(g) - want[name]) <= tol(name), (name, float(g), want[name])
        params["projector." + name].grad = None

    params["projector.active_data"] = pat.clone().requires_grad_(True)
    params.update()
    integ.render_backward(scene, params, G, sensor, seed=0, spp=2)
    integ.render_backward(scene, params, G, sensor, seed=0, spp=2)  # accumulates
    for name in names:
        assert abs(float(params["projector." + name].grad) - 2 * want[name]) <= 2 * tol(name)
    g_pat = 2 * proj.adjoint(G, n, None, 2, 0).double()
    assert float(torch.linalg.norm(scene.projector.active_data.grad.double() - g_pat) / torch.linalg.norm(g_pat)) < 1e-6

    T = {p: proj.forward_dprojector(p, pat, None, 2, 0).double() for p in dpm.PARAMS}
    TF = T["focus_distance"] + p_over_F * T["pixel_size"] if fov else T["focus_distance"]
    Tl = dp_dfov * T["pixel_size"] if fov else T["pixel_size"]
    A = proj.forward(tan, None, 2, 0).double()
    scene.projector.active_data.grad = None
    only = integ.render_forward(scene, params, sensor, seed=0, spp=2, tangent_projector={"focus_distance": 0.5}).double()
    both = integ.render_forward(scene, params, sensor, seed=0, spp=2, tangent=tan,
                                tangent_projector={"aperture_radius": -2.0, last: 0.25}).double()
    mix = A - 2.0 * T["aperture_radius"] + 0.25 * Tl
    # (the atomics' order differs between calls)
    assert float((only - 0.5 * TF).abs().max()) <= 1e-5 * float(TF.abs().max())
    assert float((both - mix).abs().max()) <= 1e-5 * max(float(A.abs().max()), 2 * float(T["aperture_radius"].abs().max()),
                                                         float(Tl.abs().max()))
    assert len(integ._plans) == 1


FITS = [(kind, fov, name, f) for kind, fov in (("telecentric", False), ("lens", True))
        for name, fs in (("aperture_radius", (0.9, 1.1)), ("focus_distance", (0.99, 1.01)), ("distance", (0.99, 1.01)))
        for f in fs]


@pytest.mark.parametrize("kind,fov,name,f", FITS, ids=[f"{k}{'-fov' if v else ''}-{n}-{f}" for k, v, n, f in FITS])
def test_gauss_newton_recovers_the_parameter(kind, fov, name, f):
    from drtvam_amd.scene import traverse
    desc = pm.projector_scene(kind, lens_fov=fov)
    star = dpm.base_vals(desc)[name]
    model = dpm.fit_model(desc, name, f * star, 10, by_fov=fov)
    m_err = [abs(t / star - 1.0) for t in model]
    n_model = next(i + 1 for i, e in enumerate(m_err) if e <= BAR)  # (StopIteration: the model does not converge)

    scene, sensor, integ = _scene(kind, fov)
    params = traverse(scene)
    assert float(params["projector." + name]) == star
    pix = dpm.fit_pixels(desc)
    params["projector.active_pixels"] = torch.as_tensor(pix.astype(np.int32), device=DEV)
    params["projector.active_data"] = torch.ones(pix.size, dtype=torch.float32, device=DEV)
    params.update()
    assert not scene.projector.dense
    target = integ.render(scene, sensor, seed=0, spp=dpm.FIT_SPP).double().clone()
    assert float(target.abs().max()) > 0

    theta = np.float32(f * star)
    errors = []
    for _ in range(n_model + 2):
        params["projector." + name] = torch.tensor(float(theta), dtype=torch.float32)
        params.update()
        dose = integ.render(scene, sensor, seed=0, spp=dpm.FIT_SPP).double()
        T = integ.render_forward(scene, params, sensor, seed=0, spp=dpm.FIT_SPP, tangent_projector={name: 1.0}).double()
        theta = np.float32(float(theta) - float(((dose - target) * T).sum() / (T * T).sum()))
        errors.append(abs(float(theta) / star - 1.0))
        assert len(integ._plans) == 1  # the plans of earlier values are closed, not kept
    print(f"{kind}{' by fov' if fov else ''} {name} from {f}: model {['%.1e' % e for e in m_err[:n_model]]}, "
          f"GPU {['%.1e' % e for e in errors]}")
    assert errors[-1] <= BAR

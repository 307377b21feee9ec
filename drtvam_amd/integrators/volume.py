"""Volume integrator (mirror of drtvam/integrators/volume.py).

``render`` = VolumeIntegrator.render (volume.py:18-56): one forward
projection (HIP tile kernel) returning the dose tensor [Z, Y, X, C].
``render_backward`` = volume.py:97-134: the adjoint projection of ``grad_in``
accumulated into ``projector.active_data.grad``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .common import TVAMIntegrator
from ..engine import derive_seed_grad, render as engine_render


def _sigma_param(scene):
    """The medium's extinction as traverse(scene) exposes it ('printing_medium.sigma_t'), or None."""
    return getattr(scene, 'sigma_t_param', None)


def _projector_params(scene):
    """[(name, tensor, [(parameter, coefficient)])] of traverse(scene)'s projector calibration that
    requires grad (telecentric / lens projectors): the tensor and the library derivatives that sum to
    d / d name (TVAMProjector.dproj_terms)."""
    return [(name, t, scene.projector.dproj_terms(name))
            for name, t in getattr(scene, 'projector_params', {}).items() if t.requires_grad]


def _check_projectors(scene):
    if scene.projector is None:
        raise Exception("No projector found in the scene")
    if getattr(scene, 'n_projectors', 1) > 1:
        raise Exception("The scene contains more than one projector. Only one is supported")


class VolumeIntegrator(TVAMIntegrator):

    def to_string(self):
        return ('VolumeIntegrator[\n'
                f'    self.print_time={self.print_time},\n'
                f'    self.transmission_only={self.transmission_only},\n'
                f'    self.sample_time={self.sample_time},\n'
                f'    self.max_depth={self.max_depth},\n'
                f'    self.rr_depth={self.rr_depth},\n'
                ']')

    def _sensor(self, scene, sensor):
        if isinstance(sensor, int):
            return scene.sensors()[sensor]
        if isinstance(sensor, str):
            return scene.sensor_by_id(sensor)
        return sensor

    def render(self, scene, sensor=0, seed: int = 0, spp: int = 0, develop: bool = True,
               evaluate: bool = True) -> torch.Tensor:
        _check_projectors(scene)
        sensor = self._sensor(scene, sensor)
        projector = scene.projector
        seed, spp = self.prepare(projector, seed, spp)
        proj = self.projection(scene, sensor)
        pix = None if projector.dense else projector.active_pixels
        with torch.no_grad():
            dose = proj.forward(projector.active_data.detach().contiguous(), pix, spp, seed)
        sensor.film().data = dose
        return dose

    def render_differentiable(self, scene, sensor=0, spp: int = 0, spp_grad: Optional[int] = None, seed: int = 0,
                              seed_grad: Optional[int] = None, active_data: Optional[torch.Tensor] = None):
        """mi.render with AD: dose depends differentiably on active_data (default: projector.active_data)
        and, when traverse(scene)'s 'printing_medium.sigma_t' or 'projector.<calibration>' require grad, on
        the medium's extinction and the projector's parameters."""
        _check_projectors(scene)
        sensor = self._sensor(scene, sensor)
        projector = scene.projector
        seed, spp = self.prepare(projector, seed, spp)
        spp_grad = spp if not spp_grad else (1 if self.regular_sampling else spp_grad)
        proj = self.projection(scene, sensor)
        pix = None if projector.dense else projector.active_pixels
        x = projector.active_data if active_data is None else active_data
        sig = _sigma_param(scene)
        if sig is not None and not sig.requires_grad:
            sig = None
        return engine_render(proj, x, pix, spp, spp_grad, seed, derive_seed_grad(seed) if seed_grad is None else seed_grad,
                             sigma_t=sig, projector=[(t, terms) for _, t, terms in _projector_params(scene)])

    def render_forward(self, scene, params=None, sensor=0, seed: int = 0, spp: int = 0,
                       tangent: Optional[torch.Tensor] = None,
                       tangent_sigma_t: Optional[float] = None,
                       tangent_projector: Optional[dict] = None) -> torch.Tensor:
        """Forward-mode derivative (volume.py:58-95): the dose tangent [Z, Y, X, C] produced by a
        tangent of projector.active_data.  The render is linear in the patterns, so this is the
        forward projection of the tangent (the reference propagates dr.grad(active_data) through
        Le in ADMode.Forward and scales by inv_vol, as the forward kernel does).  `tangent`
        defaults to projector.active_data.grad, the slot the reference reads it from.
        `tangent_sigma_t`: a tangent of the medium's extinction (sensor.py:371-375); the result is
        A tangent + tangent_sigma_t T with T = d dose / d sigma_t of projector.active_data
        (Projection.forward_dsigma).  `tangent_projector`: tangents of traverse(scene)'s projector
        calibration by name, e.g. {'focus_distance': 1.0}; each adds its tangent times
        d dose / d name (Projection.forward_dprojector; a lens given by fov through the chain rule of
        TVAMProjector.dproj_terms).  Any tangent alone is allowed."""
        _check_projectors(scene)
        sensor = self._sensor(scene, sensor)
        projector = scene.projector
        if tangent is None:
            tangent = projector.active_data.grad
        if tangent is None and tangent_sigma_t is None and not tangent_projector:
            raise ValueError("render_forward: no tangent (set projector.active_data.grad or pass `tangent`)")
        if tangent is not None and tangent.numel() != projector.active_size():
            raise ValueError("render_forward: the tangent must have one entry per active pixel")
        seed, spp = self.prepare(projector, seed, spp)
        proj = self.projection(scene, sensor)
        pix = None if projector.dense else projector.active_pixels
        with torch.no_grad():
            out = None
            if tangent is not None:
                out = proj.forward(tangent.detach().to(dtype=torch.float32).contiguous(), pix, spp, seed)
            if tangent_sigma_t is not None:
                T = proj.forward_dsigma(projector.active_data.detach().contiguous(), pix, spp, seed)
                T *= float(tangent_sigma_t)
                out = T if out is None else out.add_(T)
            for name, tv in (tangent_projector or {}).items():
                for param, c in projector.dproj_terms(name):
                    T = proj.forward_dprojector(param, projector.active_data.detach().contiguous(), pix, spp, seed)
                    T *= float(tv) * c
                    out = T if out is None else out.add_(T)
            return out

    def render_backward(self, scene, params, grad_in: torch.Tensor, sensor=0, seed: int = 0, spp: int = 0) -> None:
        _check_projectors(scene)
        sensor = self._sensor(scene, sensor)
        projector = scene.projector
        seed, spp = self.prepare(projector, seed, spp)
        proj = self.projection(scene, sensor)
        pix = None if projector.dense else projector.active_pixels
        g = proj.adjoint(grad_in.contiguous(), projector.active_size(), pix, spp, seed)
        x = projector.active_data
        if x.grad is None:
            x.grad = g
        else:
            x.grad += g
        sig = _sigma_param(scene)
        if sig is not None and sig.requires_grad:  # st_grad into sigma_t (volume.py:274-280)
            gs = proj.adjoint_dsigma(x.detach().contiguous(), grad_in.contiguous(), pix, spp, seed)
            gs = gs.to(device=sig.device, dtype=sig.dtype)
            if sig.grad is None:
                sig.grad = gs
            else:
                sig.grad += gs
        for _, t, terms in _projector_params(scene):
            gt = sum(c * proj.adjoint_dprojector(param, x.detach().contiguous(), grad_in.contiguous(), pix, spp, seed)
                     for param, c in terms).to(device=t.device, dtype=t.dtype)
            if t.grad is None:
                t.grad = gt
            else:
                t.grad += gt


integrators = {'volume': VolumeIntegrator}

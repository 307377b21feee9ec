"""Corner integrator (mirror of drtvam/integrators/filter_corner.py).

``render`` sends one ray through every active pixel, intersects it with the scene's first surface
(the container's outer surface or an occluder) and reports which pixels stay active: those whose
ray meets the scene and does not land within ``radius`` of a vial corner at (+-dist, +-dist).
The optimiser's 'filter_corner' (optimize.py:166-185) compacts the active set to them.
"""
from __future__ import annotations

import torch

from .common import TVAMIntegrator
from .volume import _check_projectors, integrators


class CornerIntegrator(TVAMIntegrator):
    def __init__(self, props):
        super().__init__(props)
        self.dist = props['dist']
        self.radius = props.get('radius', 0.1)

    def to_string(self):
        return 'CornerIntegrator'

    def _sensor(self, scene, sensor):
        if isinstance(sensor, int):
            return scene.sensors()[sensor]
        if isinstance(sensor, str):
            return scene.sensor_by_id(sensor)
        return sensor

    def render(self, scene, sensor=0, seed: int = 0, spp: int = 0, develop: bool = True,
               evaluate: bool = True) -> torch.Tensor:
        """Tensor of projector.size() ([n_patterns, h, w]): 1 at the active pixels that are kept, 0
        elsewhere.  The reference's values are the emitter weight of each kept ray; only their sign
        is ever read (optimize.py:173), so 1 stands for it.  The pass samples as the optimiser runs
        it (regular, one sample, seed 0) whatever ``seed`` / ``spp`` say; the target mesh, which
        lies inside the container, is not intersected."""
        _check_projectors(scene)
        projector = scene.projector
        proj = self.projection(scene, self._sensor(scene, sensor))
        pix = projector.active_pixels.to(device=proj.device, dtype=torch.int32).contiguous()
        with torch.no_grad():
            keep = proj.corner(self.dist, self.radius, active_pixels=pix)
        n, h, w = projector.size()
        imgs = torch.zeros(n * h * w, dtype=torch.float32, device=proj.device)
        imgs[pix.long()] = keep
        return imgs.reshape(n, h, w)


integrators['corner'] = CornerIntegrator

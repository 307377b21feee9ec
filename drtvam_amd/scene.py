"""Scene assembly and the ``render`` / ``traverse`` entry points.

Mirrors the pieces of Mitsuba that drtvam relies on around the hot path:
``load_dict`` (optimize.py:90), ``traverse`` (optimize.py:91, the
'projector.active_data' / 'projector.active_pixels' parameters) and
``render(scene, params, integrator, sensor, spp, spp_grad, seed)``
(optimize.py:216, :294, :328).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .geometry import CustomVial, CylindricalVial, DoubleCylindricalVial, IndexMatchedVial, Container
from .integrators import integrators, VolumeIntegrator
from .projector import TVAMProjector, emitters
from .sensor import VolumetricSensor, sensors


class Scene:
    def __init__(self):
        self.projector: Optional[TVAMProjector] = None
        self.n_projectors = 0
        self._sensors: list[tuple[str, VolumetricSensor]] = []
        self.container: Optional[Container] = None
        self.target = None
        self.integrator = None
        self.shapes = {}
        self.sigma_t_param = None  # traverse()'s 'printing_medium.sigma_t', once traversed
        self.projector_params = {}  # traverse()'s 'projector.<name>' of a telecentric / lens projector, by name

    def emitters(self):
        return [self.projector] if self.projector is not None else []

    def sensors(self):
        return [s for _, s in self._sensors]

    def sensor_by_id(self, sid):
        for k, s in self._sensors:
            if k == sid:
                return s
        raise KeyError(sid)

    def sensor_ids(self):
        return [k for k, _ in self._sensors]


def _medium_from(d, ior):
    m = {'ior': ior, 'extinction': d.get('sigma_t', 1.0), 'albedo': d.get('albedo', 0.0)}
    if 'phase' in d:
        m['phase'] = d['phase']
    return m


def _container_from_shapes(scene_dict):
    media = {k: v for k, v in scene_dict.items() if isinstance(v, dict) and v.get('type') == 'homogeneous'}
    shapes = {k: v for k, v in scene_dict.items() if isinstance(v, dict) and v.get('type') in ('cylinder', 'cube', 'ply')}
    # Container.add_occlusions: 'ply' shapes whose exterior is the medium; their 'bsdf' (black diffuse or
    # dielectric) and 'face_normals' go back into the container's 'occlusions'
    occl = {k: v for k, v in shapes.items() if k.startswith('occlusion') and v['type'] == 'ply' and 'exterior' in v
            and 'interior' not in v}
    shapes = {k: v for k, v in shapes.items() if k not in occl}
    occlusions = [{'filename': v['filename'], 'face_normals': v.get('face_normals', True),
                   **({'bsdf': v['bsdf']} if 'bsdf' in v else {})} for v in occl.values()]
    extra = {'occlusions': occlusions} if occlusions else {}
    holder = [(k, v) for k, v in shapes.items() if 'interior' in v]
    if not holder:
        return None
    if len(holder) > 1:
        raise ValueError("There is more than one medium in the scene. Only one is supported")
    name, shp = holder[0]
    interior = shp['interior']
    if interior.get('type') == 'ref':
        interior = media[interior['id']]
    bsdf = shp.get('bsdf', {'type': 'diffuse'})
    if shp['type'] == 'cylinder' and bsdf.get('type') == 'null':
        p0, p1 = np.asarray(shp.get('p0', [0, 0, 0]), float), np.asarray(shp.get('p1', [0, 0, 1]), float)
        if abs(p0[0]) + abs(p0[1]) + abs(p1[0]) + abs(p1[1]) > 0 or abs(p0[2] + p1[2]) > 1e-9:
            raise NotImplementedError("only vials centred on the z axis are supported")
        return IndexMatchedVial({'r': shp['radius'], 'height': float(abs(p1[2] - p0[2])),
                                 'medium': _medium_from(interior, 1.0), **extra})
    if shp['type'] == 'cylinder' and bsdf.get('type') == 'dielectric':
        outer = [v for k, v in shapes.items() if k != name and v['type'] == 'cylinder']
        if len(outer) == 1:
            p0, p1 = np.asarray(shp['p0'], float), np.asarray(shp['p1'], float)
            return CylindricalVial({'r_int': shp['radius'], 'r_ext': outer[0]['radius'],
                                    'height': float(abs(p1[2] - p0[2])),
                                    'ior': bsdf.get('ext_ior', 1.5),
                                    'medium': _medium_from(interior, bsdf.get('int_ior', 1.0)), **extra})
        if len(outer) == 3:  # DoubleCylindricalVial.to_dict: four nested dielectric tubes
            by_r = sorted(outer + [shp], key=lambda v: -v['radius'])
            if by_r[1] is shp and 'exterior' in by_r[2] and all(v.get('bsdf', {}).get('type') == 'dielectric' for v in by_r):
                p0, p1 = np.asarray(shp['p0'], float), np.asarray(shp['p1'], float)
                return DoubleCylindricalVial({
                    'r_ext_outer': by_r[0]['radius'], 'r_int_outer': by_r[1]['radius'],
                    'r_ext_inner': by_r[2]['radius'], 'r_int_inner': by_r[3]['radius'],
                    'height': float(abs(p1[2] - p0[2])), 'ior_outer': bsdf.get('ext_ior', 1.5),
                    'ior_inner': by_r[2]['bsdf'].get('int_ior', 1.5),
                    'ior_inside_inner': by_r[3]['bsdf'].get('int_ior', 1.0),
                    'medium': _medium_from(interior, bsdf.get('int_ior', 1.0)), **extra})
    if shp['type'] == 'ply' and bsdf.get('type') == 'dielectric':  # CustomVial.to_dict: two dielectric meshes
        outer = [v for k, v in shapes.items() if k != name and v['type'] == 'ply'
                 and v.get('bsdf', {}).get('type') == 'dielectric']
        if len(outer) == 1:
            return CustomVial({'filename_vial_outer': outer[0]['filename'], 'filename_vial_inner': shp['filename'],
                               'ior': bsdf.get('ext_ior', outer[0]['bsdf'].get('int_ior', 1.5)),
                               'medium': _medium_from(interior, bsdf.get('int_ior', 1.0)), **extra})
    raise NotImplementedError(f"container shape '{name}' is not supported by the GPU engine")


def load_dict(scene_dict: dict) -> Scene:
    """Instantiate the plugins of a scene dictionary (Mitsuba ``load_dict`` for the TVAM plugin set)."""
    if scene_dict.get('type', 'scene') != 'scene':
        raise ValueError("expected a dictionary of type 'scene'")
    scene = Scene()
    for key, v in scene_dict.items():
        if key == 'type':
            continue
        if isinstance(v, TVAMProjector):
            scene.projector = v
            scene.n_projectors += 1
            continue
        if isinstance(v, VolumetricSensor):
            scene._sensors.append((key, v))
            continue
        if not isinstance(v, dict) or 'type' not in v:
            continue
        t = v['type']
        if t in emitters:
            scene.projector = emitters[t](v)
            scene.n_projectors += 1
        elif t in sensors:
            scene._sensors.append((key, sensors[t](v)))
        elif t in integrators:
            scene.integrator = integrators[t](v)
        else:
            scene.shapes[key] = v
    scene.container = scene_dict.get('_container') or _container_from_shapes(scene_dict)
    scene.target = scene_dict.get('target')
    if scene.integrator is None:
        scene.integrator = VolumeIntegrator({})
    return scene


class SceneParameters(dict):
    """``mi.traverse(scene)`` equivalent for the differentiable projector data and the printing
    medium's extinction ('printing_medium.sigma_t': a 0-dim float32 tensor on the host holding the
    container's value; ``update`` writes it back, so the next plan is built with it).  A telecentric
    or lens projector adds its calibration, 0-dim float32 host tensors as well: 'projector.distance',
    'projector.focus_distance', 'projector.aperture_radius' and 'projector.pixel_size', or
    'projector.fov' for a lens configured by fov."""

    def __init__(self, scene: Scene):
        super().__init__()
        self.scene = scene
        p = scene.projector
        dict.__setitem__(self, 'projector.active_data', p.active_data)
        dict.__setitem__(self, 'projector.active_pixels', p.active_pixels)
        if scene.container is not None:
            sig = torch.tensor(float(scene.container.sigma_t), dtype=torch.float32)
            dict.__setitem__(self, 'printing_medium.sigma_t', sig)
            scene.sigma_t_param = sig
        self._calibration = ()
        if hasattr(p, 'calibration'):
            cal = p.calibration()
            self._calibration = tuple(cal)
            for name, v in cal.items():
                dict.__setitem__(self, 'projector.' + name, torch.tensor(float(v), dtype=torch.float32))
            scene.projector_params = {name: self['projector.' + name] for name in cal}

    def update(self, values=None):
        if values is not None:
            for k in ('projector.active_data', 'projector.active_pixels', 'printing_medium.sigma_t') + \
                    tuple('projector.' + name for name in self._calibration):
                if k in values:
                    dict.__setitem__(self, k, values[k])
        self.scene.projector.set_active(self['projector.active_data'], self['projector.active_pixels'])
        sig = self.get('printing_medium.sigma_t')
        if sig is not None:
            if not isinstance(sig, torch.Tensor):
                sig = torch.tensor(float(sig), dtype=torch.float32)
                dict.__setitem__(self, 'printing_medium.sigma_t', sig)
            if sig.dim() != 0:
                raise ValueError("'printing_medium.sigma_t' must be a 0-dim tensor")
            self.scene.container.sigma_t = float(sig.detach().to(torch.float32))
            self.scene.sigma_t_param = sig
        if self._calibration:
            cal = {}
            for name in self._calibration:
                v = self['projector.' + name]
                if not isinstance(v, torch.Tensor):
                    v = torch.tensor(float(v), dtype=torch.float32)
                    dict.__setitem__(self, 'projector.' + name, v)
                if v.dim() != 0:
                    raise ValueError(f"'projector.{name}' must be a 0-dim tensor")
                cal[name] = v
            # (a value that still is the projector's own, rounded to float32, leaves it as it is)
            own = self.scene.projector.calibration()
            new = {name: float(v.detach().to(torch.float32)) for name, v in cal.items()}
            self.scene.projector.set_calibration(
                {name: own[name] if np.float32(own[name]) == np.float32(v) else v for name, v in new.items()})
            self.scene.projector_params = cal


def traverse(scene: Scene) -> SceneParameters:
    return SceneParameters(scene)


def render(scene: Scene, params=None, integrator=None, sensor=0, spp: int = 0, spp_grad: int = 0, seed: int = 0,
           seed_grad: Optional[int] = None) -> torch.Tensor:
    """Differentiable render (``mi.render``): gradients flow to projector.active_data, and to
    traverse(scene)'s 'printing_medium.sigma_t' and 'projector.<calibration>', when they require grad."""
    integrator = integrator or scene.integrator
    x = scene.projector.active_data
    sig = getattr(scene, 'sigma_t_param', None)
    cal = any(v.requires_grad for v in getattr(scene, 'projector_params', {}).values())
    if (x.requires_grad or (sig is not None and sig.requires_grad) or cal) and torch.is_grad_enabled():
        return integrator.render_differentiable(scene, sensor, spp=spp, spp_grad=spp_grad or None, seed=seed,
                                                seed_grad=seed_grad)
    return integrator.render(scene, sensor, seed=seed, spp=spp)

"""Device-side projection engine: owns a tvam_plan and exposes the forward /
adjoint projections as torch operations.

``TvamRender`` plays the role of Mitsuba's ``mi.render`` custom op
(optimize.py:216, :294): its forward is VolumeIntegrator.render
(integrators/volume.py:18-56) and its backward is render_backward
(integrators/volume.py:97-134).  Both run the HIP kernels of libtvam.so; there
is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _abi


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def device_bytes() -> int:
    """Bytes of device memory libtvam.so owns in this process (tvam_device_bytes): 0 without plans."""
    return int(_abi.load_library().tvam_device_bytes())


def derive_seed_grad(seed: int) -> int:
    """Seed of the adjoint pass when none is given (decorrelated from the primal)."""
    v0, v1 = seed & 0xFFFFFFFF, 1
    s = 0
    for _ in range(4):
        s = (s + 0x9E3779B9) & 0xFFFFFFFF
        v0 = (v0 + ((((v1 << 4) & 0xFFFFFFFF) + 0xA341316C) ^ ((v1 + s) & 0xFFFFFFFF) ^ ((v1 >> 5) + 0xC8013EA4))) & 0xFFFFFFFF
        v1 = (v1 + ((((v0 << 4) & 0xFFFFFFFF) + 0xAD90777D) ^ ((v0 + s) & 0xFFFFFFFF) ^ ((v0 >> 5) + 0x7E95761E))) & 0xFFFFFFFF
    return v0


DPROJ_PARAMS = {'distance': _abi.DPROJ_DISTANCE, 'focus_distance': _abi.DPROJ_FOCUS_DISTANCE,
                'aperture_radius': _abi.DPROJ_APERTURE_RADIUS, 'pixel_size': _abi.DPROJ_PIXEL_SIZE}


def dproj_id(param) -> int:
    """A projector parameter (its name or _abi.DPROJ_*) as the id the library takes."""
    return DPROJ_PARAMS[param] if isinstance(param, str) else int(param)


class Projection:
    """One tvam_plan (scene tables) bound to one GPU."""

    def __init__(self, desc: _abi.TvamDesc, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise _abi.TvamError("the TVAM projection engine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = _abi.load_library()
        self.desc = desc.copy()
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        plan = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            if self.desc.reflected:  # transmission_only = 0: reflections sampled at the glass and the inserts
                ins = self.desc.inserts
                _abi.check(self.lib.tvam_plan_create_reflect(ctypes.byref(self.desc), _abi.insert_array(ins), len(ins),
                                                             self.device.index, ctypes.byref(plan)))
            elif self.desc.inserts:  # dielectric occluders travel beside the struct (set_inserts)
                ins = self.desc.inserts
                _abi.check(self.lib.tvam_plan_create_inserts(ctypes.byref(self.desc), _abi.insert_array(ins), len(ins),
                                                             self.device.index, ctypes.byref(plan)))
            elif self.desc.vial_type == _abi.VIAL_CUSTOM:  # the meshes travel beside the struct (set_vial_meshes)
                outer = getattr(self.desc, "_vial_outer", None)
                inner = getattr(self.desc, "_vial_inner", None)
                _abi.check(self.lib.tvam_plan_create_mesh(
                    ctypes.byref(self.desc), None if outer is None or not outer.size else outer.ctypes.data,
                    0 if outer is None else int(outer.shape[0]),
                    None if inner is None or not inner.size else inner.ctypes.data,
                    0 if inner is None else int(inner.shape[0]), self.device.index, ctypes.byref(plan)))
            elif self.desc.vial_type == _abi.VIAL_DOUBLE_CYLINDRICAL:  # radii and IORs beside the struct
                vial = getattr(self.desc, "_double_vial", None)
                _abi.check(self.lib.tvam_plan_create_double(
                    ctypes.byref(self.desc), None if vial is None else ctypes.byref(vial), self.device.index,
                    ctypes.byref(plan)))
            elif self.desc.traced_vial:  # glass tube / cuvette traced per ray in 3-D (set_traced_vial)
                _abi.check(self.lib.tvam_plan_create_traced(ctypes.byref(self.desc), self.device.index,
                                                            ctypes.byref(plan)))
            else:
                _abi.check(self.lib.tvam_plan_create(ctypes.byref(self.desc), self.device.index, ctypes.byref(plan)))
        self._plan = plan
        rx, ry, rz = self.desc.film_res
        if self.desc.slab_end >= 0:  # film slab of this plan (z-slab sharding)
            rz = self.desc.slab_end - self.desc.slab_begin
        self.film_shape = (rz, ry, rx, self.desc.film_channels)
        self.n_dense = self.desc.n_patterns * self.desc.crop_y * self.desc.crop_x

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self.lib.tvam_plan_destroy(self._plan)
            self._plan = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_tensor(self, t: torch.Tensor, dtype, name):
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor on {self.device}")

    def _check_pixels(self, active_pixels: torch.Tensor):
        """The plan keeps a sparse set's ray records keyed on the active_pixels pointer and count.
        A pointer alone does not name a set: a freed tensor's address can be handed to a new one.
        So the projection holds the last tensor it was given (its storage cannot be reused while
        held) and drops the records (tvam_plan_set_active) whenever a call brings another tensor
        object, or the same tensor changed in place (new torch version)."""
        self._check_tensor(active_pixels, torch.int32, "active_pixels")
        ver = active_pixels._version
        last = getattr(self, "_pix_last", None)
        if last is not None and (last[0] is not active_pixels or last[1] != ver):
            self.set_active(self.desc.active_base, self.desc.active_total)
        self._pix_last = (active_pixels, ver)

    def forward(self, active_data: torch.Tensor, active_pixels: Optional[torch.Tensor] = None, spp: int = 1,
                seed: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_tensor(active_data, torch.float32, "active_data")
        if active_pixels is not None:
            self._check_pixels(active_pixels)
        if out is None:
            out = torch.empty(self.film_shape, dtype=torch.float32, device=self.device)
        self._check_tensor(out, torch.float32, "dose")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_forward(
                self._plan, active_data.data_ptr(), None if active_pixels is None else active_pixels.data_ptr(),
                active_data.numel(), spp, seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def forward_slices(self, active_data: torch.Tensor, active_pixels: Optional[torch.Tensor], spp: int, seed: int,
                       z_begin: int, z_end: int, out: torch.Tensor) -> torch.Tensor:
        """The forward of film slices [z_begin, z_end) into out (the other slices untouched)."""
        self._check_tensor(active_data, torch.float32, "active_data")
        if active_pixels is not None:
            self._check_pixels(active_pixels)
        self._check_tensor(out, torch.float32, "dose")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_forward_slices(
                self._plan, active_data.data_ptr(), None if active_pixels is None else active_pixels.data_ptr(),
                active_data.numel(), spp, seed & 0xFFFFFFFF, int(z_begin), int(z_end), out.data_ptr(),
                _stream_ptr(self.device)))
        return out

    @property
    def fwd_chunk(self) -> int:
        """Slice granularity of forward_slices (0: not splittable)."""
        return int(self.lib.tvam_plan_fwd_chunk(self._plan))

    def adjoint(self, grad_dose: torch.Tensor, n_active: int, active_pixels: Optional[torch.Tensor] = None,
                spp: int = 1, seed: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        grad_dose = grad_dose.contiguous()
        self._check_tensor(grad_dose, torch.float32, "grad_dose")
        if grad_dose.numel() != self.film_shape[0] * self.film_shape[1] * self.film_shape[2] * self.film_shape[3]:
            raise ValueError("grad_dose has the wrong number of elements")
        if active_pixels is not None:
            self._check_pixels(active_pixels)
        if out is None:
            out = torch.empty(n_active, dtype=torch.float32, device=self.device)
        self._check_tensor(out, torch.float32, "grad_active")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_adjoint(
                self._plan, grad_dose.data_ptr(), None if active_pixels is None else active_pixels.data_ptr(),
                n_active, spp, seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def forward_dsigma(self, active_data: torch.Tensor, active_pixels: Optional[torch.Tensor] = None, spp: int = 1,
                       seed: int = 0) -> torch.Tensor:
        """The tangent film d dose / d sigma_t of forward(active_data, ...) (tvam_forward_dsigma), film
        shaped.  Non-scattering media; ValueError names what the entry refuses."""
        self._check_tensor(active_data, torch.float32, "active_data")
        if active_pixels is not None:
            self._check_pixels(active_pixels)
        out = torch.empty(self.film_shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_forward_dsigma(
                self._plan, active_data.data_ptr(), None if active_pixels is None else active_pixels.data_ptr(),
                active_data.numel(), spp, seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def adjoint_dsigma(self, active_data: torch.Tensor, grad_dose: torch.Tensor,
                       active_pixels: Optional[torch.Tensor] = None, spp: int = 1, seed: int = 0) -> torch.Tensor:
        """d <grad_dose, forward(active_data, ...)> / d sigma_t (tvam_adjoint_dsigma): a 0-dim float64
        tensor, the same bits for the same call."""
        self._check_tensor(active_data, torch.float32, "active_data")
        grad_dose = grad_dose.contiguous()
        self._check_tensor(grad_dose, torch.float32, "grad_dose")
        if grad_dose.numel() != self.film_shape[0] * self.film_shape[1] * self.film_shape[2] * self.film_shape[3]:
            raise ValueError("grad_dose has the wrong number of elements")
        if active_pixels is not None:
            self._check_pixels(active_pixels)
        out = torch.empty((), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_adjoint_dsigma(
                self._plan, active_data.data_ptr(), grad_dose.data_ptr(),
                None if active_pixels is None else active_pixels.data_ptr(), active_data.numel(), spp,
                seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def forward_dprojector(self, param, active_data: torch.Tensor, active_pixels: Optional[torch.Tensor] = None,
                           spp: int = 1, seed: int = 0) -> torch.Tensor:
        """The tangent film d dose / d theta of forward(active_data, ...) in one projector parameter
        (tvam_forward_dprojector), film shaped.  param: _abi.DPROJ_* or its name ('distance',
        'focus_distance', 'aperture_radius', 'pixel_size').  Telecentric / lens plans behind the
        index-matched vial; ValueError names what the entry refuses."""
        self._check_tensor(active_data, torch.float32, "active_data")
        if active_pixels is not None:
            self._check_pixels(active_pixels)
        out = torch.empty(self.film_shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_forward_dprojector(
                self._plan, dproj_id(param), active_data.data_ptr(),
                None if active_pixels is None else active_pixels.data_ptr(), active_data.numel(), spp,
                seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def adjoint_dprojector(self, param, active_data: torch.Tensor, grad_dose: torch.Tensor,
                           active_pixels: Optional[torch.Tensor] = None, spp: int = 1, seed: int = 0) -> torch.Tensor:
        """d <grad_dose, forward(active_data, ...)> / d theta (tvam_adjoint_dprojector): a 0-dim float64
        tensor, the same bits for the same call."""
        self._check_tensor(active_data, torch.float32, "active_data")
        grad_dose = grad_dose.contiguous()
        self._check_tensor(grad_dose, torch.float32, "grad_dose")
        if grad_dose.numel() != self.film_shape[0] * self.film_shape[1] * self.film_shape[2] * self.film_shape[3]:
            raise ValueError("grad_dose has the wrong number of elements")
        if active_pixels is not None:
            self._check_pixels(active_pixels)
        out = torch.empty((), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_adjoint_dprojector(
                self._plan, dproj_id(param), active_data.data_ptr(), grad_dose.data_ptr(),
                None if active_pixels is None else active_pixels.data_ptr(), active_data.numel(), spp,
                seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def adjoint_slices(self, grad_dose: torch.Tensor, n_active: int, z_begin: int, z_end: int, row_begin: int,
                       row_end: int, out: torch.Tensor) -> torch.Tensor:
        """The planar adjoint of film slices [z_begin, z_end) into DMD rows [row_begin, row_end) of every
        angle of out (dense set; those rows zeroed first, the rest untouched; tvam_adjoint_slices).
        An empty row range (row_begin == row_end) zeroes nothing: the slices' contributions are added
        to out as it stands (a caller that zeroed the whole vector once)."""
        self._check_tensor(grad_dose, torch.float32, "grad_dose")
        self._check_tensor(out, torch.float32, "grad_active")
        if out.numel() != n_active:
            raise ValueError("adjoint_slices: out must hold n_active entries")
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_adjoint_slices(self._plan, grad_dose.data_ptr(), n_active, int(z_begin),
                                                    int(z_end), int(row_begin), int(row_end), out.data_ptr(),
                                                    _stream_ptr(self.device)))
        return out

    @property
    def adj_chunk(self) -> int:
        """Slice granularity of adjoint_slices (0: not available)."""
        return int(self.lib.tvam_plan_adj_chunk(self._plan))

    def set_active(self, active_base: int, active_total: int) -> None:
        """Position of this plan's first active entry in the whole active set and that set's
        size (desc.active_base / active_total): sampler streams and the ray weight of later
        calls follow the reference's whole projector.active_pixels (common.py:57-67)."""
        _abi.check(self.lib.tvam_plan_set_active(self._plan, int(active_base), int(active_total)))
        self.desc.active_base = int(active_base)
        self.desc.active_total = int(active_total)

    def compute_volume(self, sample_count: int = 2 ** 14) -> torch.Tensor:
        """Surface-aware voxel volumes [Z, Y, X, 2] (inside, outside the target mesh) of this plan's
        film (VolumetricSensor.compute_volume, sensor.py:47-110)."""
        out = torch.empty(self.film_shape[:3] + (2,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_compute_volume(self._plan, int(sample_count), out.data_ptr(),
                                                    _stream_ptr(self.device)))
        return out

    def set_volumes(self, volumes: torch.Tensor) -> None:
        """Per-(voxel, channel) volumes of a surface-aware film (the forward divides by them,
        volume.py:41-42); the projection keeps the tensor alive."""
        self._check_tensor(volumes, torch.float32, "volumes")
        if tuple(volumes.shape) != tuple(self.film_shape):
            raise ValueError(f"volumes must have the film shape {self.film_shape}")
        _abi.check(self.lib.tvam_plan_set_volumes(self._plan, volumes.data_ptr()))
        self._volumes = volumes

    def radon(self, target_tris, spp: int = 4, seed: int = 0, max_depth: int = 5) -> torch.Tensor:
        """Radon filter image of this plan's DMD pixels (dense crop order of its shard):
        positive where a ray crosses the target inside the medium (radon.py:47-106)."""
        import numpy as np
        tris = np.ascontiguousarray(target_tris, dtype=np.float32).reshape(-1, 9)
        a0, a1 = self.desc.angle_begin, (self.desc.angle_end if self.desc.angle_end >= 0 else self.desc.n_patterns)
        out = torch.empty((a1 - a0) * self.desc.crop_y * self.desc.crop_x, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_radon(self._plan, tris.ctypes.data if tris.size else None, tris.shape[0], spp,
                                           seed & 0xFFFFFFFF, max_depth, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def corner(self, dist: float, radius: float = 0.1, active_pixels: Optional[torch.Tensor] = None,
               n_active: Optional[int] = None, hits: bool = False):
        """Corner filter mask of the active entries (tvam_corner; filter_corner.py:17-66): float32
        1 where the ray through the pixel's centre meets the scene's first surface at p and not
        sqrt((|p.x| - dist)^2 + (|p.y| - dist)^2) < radius, else 0.  active_pixels: int32 full-DMD
        indices (None: this plan's dense shard order).  With hits=True returns (keep, hits), hits
        [n, 4] = p.x, p.y, p.z, t (t = -1 on a miss)."""
        if active_pixels is not None:
            self._check_tensor(active_pixels, torch.int32, "active_pixels")
            n_active = int(active_pixels.numel())
        elif n_active is None:
            a0, a1 = self.desc.angle_begin, (self.desc.angle_end if self.desc.angle_end >= 0 else self.desc.n_patterns)
            n_active = (a1 - a0) * self.desc.crop_y * self.desc.crop_x
        keep = torch.empty(int(n_active), dtype=torch.float32, device=self.device)
        h = torch.empty((int(n_active), 4), dtype=torch.float32, device=self.device) if hits else None
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_corner(
                self._plan, None if active_pixels is None else active_pixels.data_ptr(), int(n_active), float(dist),
                float(radius), keep.data_ptr(), None if h is None else h.data_ptr(), _stream_ptr(self.device)))
        return (keep, h) if hits else keep

    def rays(self, n_active: Optional[int] = None, active_pixels: Optional[torch.Tensor] = None, spp: int = 1,
             seed: int = 0) -> torch.Tensor:
        """The projector rays of a call (tvam_plan_rays), [n_active * spp, 16] float32 in sampler-stream
        order (row = active entry * spp + sample): o[0:3], d[3:6], hit [6], o2[7:10], maxt [10],
        d2[11:14], weight [14] (the whole per-ray weight), 0.  The diagnostic counterpart of the
        oracle's ray(); index-matched plans with a non-scattering medium, and 'custom',
        'double_cylindrical' and traced glass vial plans (d2: the refracted direction; the weight carries the
        interfaces' transmission; double_cylindrical: the first of the two segments, see segments())."""
        if active_pixels is not None:
            self._check_pixels(active_pixels)
            n_active = int(active_pixels.numel())
        elif n_active is None:
            a0, a1 = self.desc.angle_begin, (self.desc.angle_end if self.desc.angle_end >= 0 else self.desc.n_patterns)
            n_active = (a1 - a0) * self.desc.crop_y * self.desc.crop_x
        if self.desc.regular_sampling:
            spp = 1  # common.py:49-51
        out = torch.zeros((int(n_active) * int(spp), 16), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_plan_rays(
                self._plan, None if active_pixels is None else active_pixels.data_ptr(), int(n_active), int(spp),
                seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def segments(self, n_active: Optional[int] = None, active_pixels: Optional[torch.Tensor] = None, spp: int = 1,
                 seed: int = 0) -> torch.Tensor:
        """Both medium segments of a call's rays behind a 'double_cylindrical' vial (tvam_plan_segments),
        [n_active * spp, 2, 8] float32 in sampler-stream order: o2[0:3], maxt [3], d2[4:7], weight [7]
        (the whole per-ray weight times the attenuation the segment starts with); a slot without a
        segment is all zeros."""
        if active_pixels is not None:
            self._check_pixels(active_pixels)
            n_active = int(active_pixels.numel())
        elif n_active is None:
            a0, a1 = self.desc.angle_begin, (self.desc.angle_end if self.desc.angle_end >= 0 else self.desc.n_patterns)
            n_active = (a1 - a0) * self.desc.crop_y * self.desc.crop_x
        if self.desc.regular_sampling:
            spp = 1  # common.py:49-51
        out = torch.zeros((int(n_active) * int(spp), 2, 8), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_plan_segments(
                self._plan, None if active_pixels is None else active_pixels.data_ptr(), int(n_active), int(spp),
                seed & 0xFFFFFFFF, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def insert_segments(self, n_active: Optional[int] = None, active_pixels: Optional[torch.Tensor] = None,
                        spp: int = 1, seed: int = 0, max_segments: int = 8):
        """Every medium segment of a call's rays through a resin with dielectric occluders
        (tvam_plan_insert_segments): (segs [n_active * spp, max_segments, 8] float32 in sampler-stream order:
        o2[0:3], maxt [3], d2[4:7], weight [7] (the whole per-ray weight times the attenuation the segment
        starts with), zeros past a ray's segments; nseg [n_active * spp] int32, the segments each ray has).
        A transmission_only = 0 plan (tvam_plan_create_reflect) is served too: its reflected segments are among
        them, in path order."""
        if active_pixels is not None:
            self._check_pixels(active_pixels)
            n_active = int(active_pixels.numel())
        elif n_active is None:
            a0, a1 = self.desc.angle_begin, (self.desc.angle_end if self.desc.angle_end >= 0 else self.desc.n_patterns)
            n_active = (a1 - a0) * self.desc.crop_y * self.desc.crop_x
        if self.desc.regular_sampling:
            spp = 1  # common.py:49-51
        rows = int(n_active) * int(spp)
        segs = torch.zeros((rows, int(max_segments), 8), dtype=torch.float32, device=self.device)
        nseg = torch.zeros((rows,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_plan_insert_segments(
                self._plan, None if active_pixels is None else active_pixels.data_ptr(), int(n_active), int(spp),
                seed & 0xFFFFFFFF, int(max_segments), segs.data_ptr(), nseg.data_ptr(), _stream_ptr(self.device)))
        return segs, nseg

    @property
    def cone(self) -> bool:
        """True for the 3-D per-ray path: a telecentric / lens projector, a 'custom' or
        'double_cylindrical' vial, or a traced 'cylindrical' / 'square' vial (set_traced_vial)."""
        return bool(self.lib.tvam_plan_path(self._plan) & 4)

    @property
    def planar(self) -> bool:
        """True when the planar fast path (regular sampling) serves this plan's adjoint."""
        return bool(self.lib.tvam_plan_path(self._plan) & 1)

    @property
    def planar_forward(self) -> bool:
        """True when the voxel-driven planar forward serves this plan (straight rays)."""
        return bool(self.lib.tvam_plan_path(self._plan) & 2)

    def fwd_variant(self) -> dict:
        """The voxel-driven forward kernel this plan launches (tvam_plan_fwd_variant): Z slices per
        workgroup, NC candidate columns instantiated, the plan's candidate count nc, the staged window
        ncmax, AB angles per barrier, PF staged values per thread, the flags BIN / DMA / MULTI / REFR /
        SCONST and the angle parts.  ValueError when the voxel-driven forward does not serve the plan."""
        import numpy as np
        v = np.zeros(8, dtype=np.int32)
        _abi.check(self.lib.tvam_plan_fwd_variant(self._plan, v.ctypes.data))
        out = dict(zip(("Z", "NC", "nc", "ncmax", "AB", "PF"), (int(x) for x in v[:6])))
        for bit, name in enumerate(("BIN", "DMA", "MULTI", "REFR", "SCONST")):
            out[name] = bool(int(v[6]) >> bit & 1)
        out["parts"] = int(v[7])
        return out

    def fallback_tiles(self) -> int:
        """Workgroups of the last forward that used float LDS atomics (needs FLAG_FWD_STATS)."""
        v = ctypes.c_uint64(0)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _abi.check(self.lib.tvam_plan_stats(self._plan, ctypes.byref(v)))
        return int(v.value)

    def fwd_scale(self):
        """(scale, fixed) of the last ray-driven planar forward: the int32 fixed-point scale 2^e and
        whether fixed point was used (False: the overflow bound was not finite, float adds)."""
        import numpy as np
        v = np.zeros(2, dtype=np.float32)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _abi.check(self.lib.tvam_plan_fwd_scale(self._plan, v.ctypes.data))
        return float(v[0]), bool(v[1] != 0.0)

    def bin_stats(self):
        """Chunking of the last brick-binned call (scattering media): a dict with the chunks of
        paths, those served from / stored into the forward bin cache, the brick entries marched,
        the paths per chunk, the device bytes of the bin cache and scratch, and the slots whose bin-fill
        walk disagreed with the record writer's closed-form brick count (0; tvam_plan_bin_stats)."""
        import numpy as np
        v = np.zeros(8, dtype=np.int64)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _abi.check(self.lib.tvam_plan_bin_stats(self._plan, v.ctypes.data))
        return dict(zip(("chunks", "cached", "stored", "entries", "chunk_paths", "cache_bytes", "scratch_bytes",
                         "count_mismatch"), (int(x) for x in v)))

    def tile_stats(self):
        """Row walks of the per-ray tile kernels for the most recent ray records (jittered plans):
        the rays listed as strays (-1: no stray lists), the list capacity, the (tile, slice)
        workgroups' stray walk and main-row slot walk summed over a launch, the frozen-axis rays,
        spp, tiles and slots (tvam_plan_tile_stats)."""
        import numpy as np
        v = np.zeros(8, dtype=np.int64)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _abi.check(self.lib.tvam_plan_tile_stats(self._plan, v.ctypes.data))
        return dict(zip(("strays", "stray_cap", "stray_walk", "main_walk", "frozen", "spp", "tiles", "slots"),
                        (int(x) for x in v)))

    def kernel_time(self, enable: bool):
        """Launch time of the dominant forward kernel from HIP events on its stream
        (tvam_plan_kernel_time): (total ms, launches) recorded since the previous call; enable
        starts a new measurement."""
        t = ctypes.c_double(0.0)
        n = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.tvam_plan_kernel_time(self._plan, 1 if enable else 0, ctypes.byref(t), ctypes.byref(n)))
        return float(t.value), int(n.value)

    def count_visits(self, spp: int = 1, seed: int = 0) -> int:
        v = ctypes.c_uint64(0)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _abi.check(self.lib.tvam_count_visits(self._plan, spp, seed & 0xFFFFFFFF, ctypes.byref(v)))
        return int(v.value)


class TvamRender(torch.autograd.Function):
    """dose = render(active_data); d loss / d active_data via the adjoint kernel, d loss / d sigma_t via
    the extinction-gradient kernel when the medium's sigma_t is an input that requires grad, and
    d loss / d (a projector parameter) via the projector-gradient kernel for the inputs `thetas`:
    dproj[i] = [(parameter, coefficient)], the library's derivatives that make up d / d thetas[i]."""

    @staticmethod
    def forward(ctx, active_data, proj: Projection, active_pixels, spp: int, spp_grad: int, seed: int,
                seed_grad: int, sigma_t=None, dproj=(), *thetas):
        ctx.proj = proj
        ctx.active_pixels = active_pixels
        ctx.spp_grad = spp_grad
        ctx.seed_grad = seed_grad
        ctx.n_active = active_data.numel()
        ctx.dproj = dproj
        ctx.theta_like = [(t.device, t.dtype) for t in thetas]
        data = active_data.detach().contiguous()
        need_sigma = sigma_t is not None and sigma_t.requires_grad
        if need_sigma or any(t.requires_grad for t in thetas):  # these gradients render the patterns again
            ctx.save_for_backward(data)
        if need_sigma:
            ctx.sigma_like = (sigma_t.device, sigma_t.dtype)
        return proj.forward(data, active_pixels, spp, seed)

    @staticmethod
    def backward(ctx, grad_dose):
        grad_dose = grad_dose.contiguous()
        g = None
        if ctx.needs_input_grad[0]:
            g = ctx.proj.adjoint(grad_dose, ctx.n_active, ctx.active_pixels, ctx.spp_grad, ctx.seed_grad)
        gs = None
        if ctx.needs_input_grad[7]:
            (data,) = ctx.saved_tensors
            gs = ctx.proj.adjoint_dsigma(data, grad_dose, ctx.active_pixels, ctx.spp_grad, ctx.seed_grad)
            gs = gs.to(device=ctx.sigma_like[0], dtype=ctx.sigma_like[1])
        gt = []
        for i, terms in enumerate(ctx.dproj):
            if not ctx.needs_input_grad[9 + i]:
                gt.append(None)
                continue
            (data,) = ctx.saved_tensors
            gi = sum(c * ctx.proj.adjoint_dprojector(param, data, grad_dose, ctx.active_pixels, ctx.spp_grad, ctx.seed_grad)
                     for param, c in terms)
            gt.append(gi.to(device=ctx.theta_like[i][0], dtype=ctx.theta_like[i][1]))
        return (g, None, None, None, None, None, None, gs, None, *gt)


def render(proj: Projection, active_data: torch.Tensor, active_pixels: Optional[torch.Tensor] = None,
           spp: int = 1, spp_grad: Optional[int] = None, seed: int = 0, seed_grad: Optional[int] = None,
           sigma_t: Optional[torch.Tensor] = None, projector=()):
    """sigma_t: the medium's extinction as a 0-dim tensor, an input of the render when it requires
    grad.  The plan bakes sigma_t in, so the tensor must hold the plan's own value (as float32).
    projector: [(theta, [(parameter, coefficient), ...])], 0-dim tensors that are inputs of the render
    when they require grad, each with the projector derivatives (Projection.adjoint_dprojector) whose
    weighted sum is d / d theta; the plan bakes the projector in as well, the caller keeps the two in step."""
    spp_grad = spp if spp_grad is None else spp_grad
    seed_grad = derive_seed_grad(seed) if seed_grad is None else seed_grad
    if sigma_t is not None:
        if sigma_t.dim() != 0:
            raise ValueError("render: sigma_t must be a 0-dim tensor")
        have = ctypes.c_float(float(sigma_t.detach())).value
        if have != ctypes.c_float(proj.desc.sigma_t).value:
            raise ValueError(f"render: sigma_t = {have!r} is not the plan's extinction {proj.desc.sigma_t!r}; "
                             "build the Projection from a descriptor with this sigma_t")
    for theta, _ in projector:
        if theta.dim() != 0:
            raise ValueError("render: a projector parameter must be a 0-dim tensor")
    return TvamRender.apply(active_data, proj, active_pixels, spp, spp_grad, seed, seed_grad, sigma_t,
                            tuple(terms for _, terms in projector), *[theta for theta, _ in projector])


def target_mask(target: torch.Tensor) -> torch.Tensor:
    """Bit mask of a contiguous f32 target (tvam_target_mask): int32 words, bit j of word w =
    target[32 w + j] > 0, the loss kernels' object test from 1/32 of the bytes."""
    if target.dtype != torch.float32 or not target.is_contiguous() or not target.is_cuda:
        raise ValueError("target_mask: a contiguous float32 CUDA tensor")
    n = target.numel()
    mask = torch.empty((n + 31) // 32, dtype=torch.int32, device=target.device)
    with torch.cuda.device(target.device):
        _abi.check(_abi.load_library().tvam_target_mask(target.data_ptr(), n, mask.data_ptr(),
                                                        _stream_ptr(target.device)))
    return mask


def _check_mask(mask, mask_bit0, n, dev):
    if mask.dtype != torch.int32 or not mask.is_contiguous() or mask.device != dev:
        raise ValueError(f"mask must be a contiguous int32 tensor on {dev}")
    if mask_bit0 < 0 or mask_bit0 + n > 32 * mask.numel():
        raise ValueError("mask: bits [mask_bit0, mask_bit0 + n) out of range")


def loss_threshold_probes(dose: torch.Tensor, ddose: torch.Tensor, alphas, target: torch.Tensor, K: int, tl: float,
                          tu: float, w_object: float, w_void: float, w_limit: float, scale: float,
                          mask: Optional[torch.Tensor] = None, mask_bit0: int = 0) -> torch.Tensor:
    """Fused ThresholdedLoss of dose + a * ddose for each a in alphas (<= 8): f64 device vector, one pass.
    ``mask``: target_mask() of a tensor whose elements [mask_bit0, mask_bit0 + n) are this target
    (the object test read from it instead of the f32 target)."""
    lib = _abi.load_library()
    na = len(alphas)
    if not 1 <= na <= 8:
        raise ValueError("loss_threshold_probes: 1 to 8 step sizes")
    for name, t in (("dose", dose), ("ddose", ddose), ("target", target)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dose.device:
            raise ValueError(f"{name} must be a contiguous float32 tensor on {dose.device}")
    n = dose.numel()
    if target.numel() != n or ddose.numel() != n:
        raise ValueError("loss_threshold_probes: size mismatch")
    out = torch.zeros(na, dtype=torch.float64, device=dose.device)
    a = (ctypes.c_float * na)(*[float(v) for v in alphas])
    with torch.cuda.device(dose.device):
        if mask is not None:
            _check_mask(mask, mask_bit0, n, dose.device)
            _abi.check(lib.tvam_loss_threshold_probes_mask(
                dose.data_ptr(), ddose.data_ptr(), a, na, mask.data_ptr(), int(mask_bit0), n, int(K), float(tl),
                float(tu), float(w_object), float(w_void), float(w_limit), float(scale), out.data_ptr(),
                _stream_ptr(dose.device)))
        else:
            _abi.check(lib.tvam_loss_threshold_probes(
                dose.data_ptr(), ddose.data_ptr(), a, na, target.data_ptr(), n, int(K), float(tl), float(tu),
                float(w_object), float(w_void), float(w_limit), float(scale), out.data_ptr(), _stream_ptr(dose.device)))
    return out


def loss_threshold(dose: torch.Tensor, target: torch.Tensor, K: int, tl: float, tu: float, w_object: float,
                   w_void: float, w_limit: float, scale: float, ddose: Optional[torch.Tensor] = None,
                   alpha: float = 0.0, grad: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                   mask_bit0: int = 0) -> torch.Tensor:
    """Fused ThresholdedLoss value (f64 device scalar) and optional dL/dx (HIP kernel); ``mask`` as in
    loss_threshold_probes."""
    lib = _abi.load_library()
    out = torch.zeros(1, dtype=torch.float64, device=dose.device)
    for name, t in (("dose", dose), ("target", target), ("ddose", ddose), ("grad", grad)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dose.device):
            raise ValueError(f"{name} must be a contiguous float32 tensor on {dose.device}")
    n = dose.numel()
    if target.numel() != n or (ddose is not None and ddose.numel() != n) or (grad is not None and grad.numel() != n):
        raise ValueError("loss_threshold: size mismatch")
    with torch.cuda.device(dose.device):
        if mask is not None:
            _check_mask(mask, mask_bit0, n, dose.device)
            _abi.check(lib.tvam_loss_threshold_mask(
                dose.data_ptr(), None if ddose is None else ddose.data_ptr(), float(alpha), mask.data_ptr(),
                int(mask_bit0), n, int(K), float(tl), float(tu), float(w_object), float(w_void), float(w_limit),
                float(scale), out.data_ptr(), None if grad is None else grad.data_ptr(), _stream_ptr(dose.device)))
        else:
            _abi.check(lib.tvam_loss_threshold(
                dose.data_ptr(), None if ddose is None else ddose.data_ptr(), float(alpha), target.data_ptr(), n,
                int(K), float(tl), float(tu), float(w_object), float(w_void), float(w_limit), float(scale),
                out.data_ptr(), None if grad is None else grad.data_ptr(), _stream_ptr(dose.device)))
    return out[0]


def _check_loss_tensors(what, dose, n_floats, **tensors):
    """The loss wrappers' checks: contiguous float32 tensors on dose's device, n_floats each."""
    for name, t in (("dose", dose),) + tuple(tensors.items()):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dose.device):
            raise ValueError(f"{name} must be a contiguous float32 tensor on {dose.device}")
        if t is not None and t.numel() != n_floats:
            raise ValueError(f"{what}: size mismatch")


def _probe_alphas(what, alphas):
    na = len(alphas)
    if not 1 <= na <= 8:
        raise ValueError(f"{what}: 1 to 8 step sizes")
    return na, (ctypes.c_float * na)(*[float(v) for v in alphas])


def _ptr(t):
    return None if t is None else t.data_ptr()


def loss_square(dose: torch.Tensor, target: torch.Tensor, scale: float, ddose: Optional[torch.Tensor] = None,
                alpha: float = 0.0, grad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused L2Loss over a one-channel target (tvam_loss_square): scale * sum (x - target)^2 with x = dose +
    alpha * ddose as an f64 device scalar, and optionally dL/dx = 2 (x - target) scale into grad."""
    lib = _abi.load_library()
    n = dose.numel()
    _check_loss_tensors("loss_square", dose, n, target=target, ddose=ddose, grad=grad)
    out = torch.zeros(1, dtype=torch.float64, device=dose.device)
    with torch.cuda.device(dose.device):
        _abi.check(lib.tvam_loss_square(dose.data_ptr(), _ptr(ddose), float(alpha), target.data_ptr(), n, float(scale),
                                        out.data_ptr(), _ptr(grad), _stream_ptr(dose.device)))
    return out[0]


def loss_square_probes(dose: torch.Tensor, ddose: torch.Tensor, alphas, target: torch.Tensor,
                       scale: float) -> torch.Tensor:
    """loss_square of dose + a * ddose for each a in alphas (<= 8): f64 device vector, one pass."""
    lib = _abi.load_library()
    na, a = _probe_alphas("loss_square_probes", alphas)
    n = dose.numel()
    _check_loss_tensors("loss_square_probes", dose, n, ddose=ddose, target=target)
    out = torch.zeros(na, dtype=torch.float64, device=dose.device)
    with torch.cuda.device(dose.device):
        _abi.check(lib.tvam_loss_square_probes(dose.data_ptr(), ddose.data_ptr(), a, na, target.data_ptr(), n,
                                               float(scale), out.data_ptr(), _stream_ptr(dose.device)))
    return out


def _surface_voxels(what, dose):
    if dose.numel() % 2:
        raise ValueError(f"{what}: a two-channel dose has an even number of floats")
    return dose.numel() // 2


def loss_surface(kind: int, dose: torch.Tensor, target: torch.Tensor, scale: float, K: int = 2, tl: float = 0.0,
                 tu: float = 0.0, w_object: float = 1.0, w_void: float = 1.0, w_limit: float = 1.0,
                 ddose: Optional[torch.Tensor] = None, alpha: float = 0.0,
                 grad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused loss over a surface-aware film (tvam_loss_surface): dose, target, ddose, grad hold the two
    channels interleaved per voxel ([..., 2]); kind _abi.LOSS_KIND_THRESHOLD (K, tl, tu and the weights
    of ThresholdedLoss) or _abi.LOSS_KIND_L2.  f64 device scalar; dL/dx per channel into grad."""
    lib = _abi.load_library()
    nv = _surface_voxels("loss_surface", dose)
    _check_loss_tensors("loss_surface", dose, 2 * nv, target=target, ddose=ddose, grad=grad)
    out = torch.zeros(1, dtype=torch.float64, device=dose.device)
    with torch.cuda.device(dose.device):
        _abi.check(lib.tvam_loss_surface(
            int(kind), dose.data_ptr(), _ptr(ddose), float(alpha), target.data_ptr(), nv, int(K), float(tl), float(tu),
            float(w_object), float(w_void), float(w_limit), float(scale), out.data_ptr(), _ptr(grad),
            _stream_ptr(dose.device)))
    return out[0]


def loss_surface_probes(kind: int, dose: torch.Tensor, ddose: torch.Tensor, alphas, target: torch.Tensor,
                        scale: float, K: int = 2, tl: float = 0.0, tu: float = 0.0, w_object: float = 1.0,
                        w_void: float = 1.0, w_limit: float = 1.0) -> torch.Tensor:
    """loss_surface of dose + a * ddose for each a in alphas (<= 8): f64 device vector, one pass."""
    lib = _abi.load_library()
    na, a = _probe_alphas("loss_surface_probes", alphas)
    nv = _surface_voxels("loss_surface_probes", dose)
    _check_loss_tensors("loss_surface_probes", dose, 2 * nv, ddose=ddose, target=target)
    out = torch.zeros(na, dtype=torch.float64, device=dose.device)
    with torch.cuda.device(dose.device):
        _abi.check(lib.tvam_loss_surface_probes(
            int(kind), dose.data_ptr(), ddose.data_ptr(), a, na, target.data_ptr(), nv, int(K), float(tl), float(tu),
            float(w_object), float(w_void), float(w_limit), float(scale), out.data_ptr(), _stream_ptr(dose.device)))
    return out


def _check_edges(edges, side: int) -> None:
    """tvam_class_hist's argument checks, for the torch path (the CUDA path leaves them to the library)."""
    import numpy as np
    k = int(edges.size)
    if not 1 <= k <= 2048:
        raise ValueError(f"class_hist: 1 <= n_edges <= 2048 (got {k})")
    if side not in (0, 1):
        raise ValueError(f"class_hist: side must be 0 or 1 (got {side})")
    bad = np.flatnonzero(~np.isfinite(edges))
    if bad.size:
        raise ValueError(f"class_hist: edge {int(bad[0])} is not finite")
    bad = np.flatnonzero(~(edges[:-1] < edges[1:]))
    if bad.size:
        raise ValueError(f"class_hist: edges must be strictly increasing (edge {int(bad[0]) + 1} <= edge {int(bad[0])})")


def class_hist(x: torch.Tensor, target: torch.Tensor, edges, side: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Class-split histogram of x over the sorted edge table `edges` (host, float32, 1 to 2048 strictly
    increasing finite values): int64 [2, n_edges + 2], row c = target > 0 (0 empty, 1 object), column
    j = #{k : edges[k] < x} (side 0) or #{k : edges[k] <= x} (side 1) for j <= n_edges; the last
    column counts the NaN entries of x, which take no slot.  Exact integer counts.

    CUDA tensors run the HIP kernel (tvam_class_hist; `out`, an int64 CUDA tensor of that shape, is
    overwritten); CPU tensors take a torch path (bucketize + bincount), the one way this module works
    without a GPU.  target is brought to x's device."""
    import numpy as np
    x = torch.as_tensor(x)
    target = torch.as_tensor(target).to(device=x.device)
    if x.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("class_hist: x and target must be float32")
    if x.numel() != target.numel():
        raise ValueError("class_hist: x and target must have the same number of elements")
    x = x.detach().contiguous().reshape(-1)
    target = target.detach().contiguous().reshape(-1)
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float32).reshape(-1))
    k, n, side = int(e.size), x.numel(), int(side)
    if x.is_cuda:
        if out is None:
            out = torch.empty((2, k + 2), dtype=torch.int64, device=x.device)
        elif out.dtype != torch.int64 or not out.is_contiguous() or out.device != x.device or out.numel() != 2 * (k + 2):
            raise ValueError(f"class_hist: out must be a contiguous int64 tensor of shape (2, {k + 2}) on {x.device}")
        with torch.cuda.device(x.device):
            _abi.check(_abi.load_library().tvam_class_hist(
                x.data_ptr() if n else None, target.data_ptr() if n else None, n, e.ctypes.data, k, side,
                out.data_ptr(), _stream_ptr(x.device)))
        return out.view(2, k + 2)
    _check_edges(e, side)
    nan = torch.isnan(x)
    slot = torch.bucketize(x, torch.from_numpy(e), right=(side == 1))
    slot = torch.where(nan, torch.full_like(slot, k + 1), slot)
    key = slot + (target > 0).to(slot.dtype) * (k + 2)
    counts = torch.bincount(key, minlength=2 * (k + 2)).to(torch.int64).view(2, k + 2)
    if out is not None:
        out.copy_(counts)
        return out
    return counts

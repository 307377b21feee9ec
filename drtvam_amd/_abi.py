"""ctypes binding of libtvam.so (include/tvam.h).

The GPU path has no fallback: if the HIP library is missing or fails to load,
every call raises.  ``TvamDesc`` mirrors ``struct tvam_desc`` field for field.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TVAM_LIB") or os.path.join(_HERE, "libtvam.so")  # TVAM_LIB: a variant build

ABI_VERSION = 13

TVAM_OK = 0
TVAM_ERR_INVALID = -1
TVAM_ERR_UNSUPPORTED = -2
TVAM_ERR_HIP = -3
TVAM_ERR_TOO_LARGE = -4

PROJECTOR_COLLIMATED = 0
PROJECTOR_TELECENTRIC = 1
PROJECTOR_LENS = 2
VIAL_INDEX_MATCHED = 0
VIAL_CYLINDRICAL = 1
VIAL_SQUARE = 2
VIAL_CUSTOM = 3
VIAL_DOUBLE_CYLINDRICAL = 4
PHASE_ISOTROPIC = 0
PHASE_RAYLEIGH = 1
PHASE_HG = 2
SENSOR_DDA = 0
SENSOR_RATIO = 1
SENSOR_DELTA = 2

FLAG_NO_ZERO_SKIP = 1
FLAG_FWD_STATS = 2
FLAG_NO_PLANAR = 4
FLAG_RAY_FWD = 8
FLAG_SCATTER_ATOMIC = 16
FLAG_BIN_FIRST = 32
LBFGS_WORK_DOUBLES = 2048 * 64
LOSS_KIND_THRESHOLD = 0
LOSS_KIND_L2 = 1
DPROJ_DISTANCE = 0
DPROJ_FOCUS_DISTANCE = 1
DPROJ_APERTURE_RADIUS = 2
DPROJ_PIXEL_SIZE = 3


class TvamDoubleVial(ctypes.Structure):
    """tvam_double_vial: the four radii (outermost first) and the glass / core IORs of a
    'double_cylindrical' vial."""
    _fields_ = [
        ("r_ext_outer", ctypes.c_float),
        ("r_int_outer", ctypes.c_float),
        ("r_ext_inner", ctypes.c_float),
        ("r_int_inner", ctypes.c_float),
        ("ior_outer", ctypes.c_float),
        ("ior_inner", ctypes.c_float),
        ("ior_inside_inner", ctypes.c_float),
    ]


class TvamInsert(ctypes.Structure):
    """tvam_insert: one dielectric occluder, its triangles (host) and the BSDF's IORs."""
    _fields_ = [
        ("tris", ctypes.c_void_p),
        ("n_tris", ctypes.c_int32),
        ("int_ior", ctypes.c_float),
        ("ext_ior", ctypes.c_float),
    ]


class TvamDesc(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("projector_type", ctypes.c_int32),
        ("n_patterns", ctypes.c_int32),
        ("res_x", ctypes.c_int32),
        ("res_y", ctypes.c_int32),
        ("crop_x", ctypes.c_int32),
        ("crop_y", ctypes.c_int32),
        ("crop_offset_x", ctypes.c_int32),
        ("crop_offset_y", ctypes.c_int32),
        ("pixel_size_x", ctypes.c_float),
        ("pixel_size_y", ctypes.c_float),
        ("distance", ctypes.c_float),
        ("clockwise", ctypes.c_int32),
        ("sensor_type", ctypes.c_int32),
        ("bbox_min", ctypes.c_float * 3),
        ("bbox_max", ctypes.c_float * 3),
        ("film_res", ctypes.c_int32 * 3),
        ("film_channels", ctypes.c_int32),
        ("vial_type", ctypes.c_int32),
        ("vial_r", ctypes.c_float),
        ("vial_r_ext", ctypes.c_float),
        ("vial_height", ctypes.c_float),
        ("vial_ior", ctypes.c_float),
        ("medium_ior", ctypes.c_float),
        ("sigma_t", ctypes.c_float),
        ("albedo", ctypes.c_float),
        ("print_time", ctypes.c_float),
        ("regular_sampling", ctypes.c_int32),
        ("sample_time", ctypes.c_int32),
        ("max_depth", ctypes.c_int32),
        ("rr_depth", ctypes.c_int32),
        ("transmission_only", ctypes.c_int32),
        ("angle_begin", ctypes.c_int32),
        ("angle_end", ctypes.c_int32),
        ("tile", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("slab_begin", ctypes.c_int32),
        ("slab_end", ctypes.c_int32),
        ("phase_type", ctypes.c_int32),
        ("phase_g", ctypes.c_float),
        ("occluder_tris", ctypes.c_void_p),
        ("n_occluder_tris", ctypes.c_int32),
        ("target_tris", ctypes.c_void_p),
        ("n_target_tris", ctypes.c_int32),
        ("majorant", ctypes.c_float),
        ("reserved0", ctypes.c_int32),
        ("active_base", ctypes.c_int64),
        ("active_total", ctypes.c_int64),
        ("aperture_radius", ctypes.c_float),
        ("focus_distance", ctypes.c_float),
    ]

    def copy(self) -> "TvamDesc":
        d = TvamDesc()
        ctypes.pointer(d)[0] = self
        # the triangle arrays and the double vial go with the copy
        for keep in ("_occluders", "_targets", "_vial_outer", "_vial_inner", "_double_vial", "_traced_vial",
                     "_inserts"):
            if hasattr(self, keep):
                setattr(d, keep, getattr(self, keep))
        return d

    def set_target(self, tris) -> None:
        """Target mesh triangles [n][3][3] (float32, host, world space) for surface-aware films."""
        import numpy as np
        t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3, 3)
        self._targets = t
        self.target_tris = t.ctypes.data if t.size else None
        self.n_target_tris = int(t.shape[0])

    def set_occluders(self, tris) -> None:
        """Occluder triangles [n][3][3] (float32, host); the desc keeps the array alive."""
        import numpy as np
        t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3, 3)
        self._occluders = t
        self.occluder_tris = t.ctypes.data if t.size else None
        self.n_occluder_tris = int(t.shape[0])

    def set_vial_meshes(self, outer, inner) -> None:
        """Outer and inner surface of a 'custom' vial, triangles [n][3][3] (float32, host, world space,
        wound outwards).  They are not part of the C struct: engine.Projection hands them to
        tvam_plan_create_mesh."""
        import numpy as np
        self._vial_outer = np.ascontiguousarray(outer, dtype=np.float32).reshape(-1, 3, 3)
        self._vial_inner = np.ascontiguousarray(inner, dtype=np.float32).reshape(-1, 3, 3)

    def set_double_vial(self, r_ext_outer, r_int_outer, r_ext_inner, r_int_inner, ior_outer, ior_inner,
                        ior_inside_inner) -> None:
        """Radii and IORs of a 'double_cylindrical' vial.  They are not part of the C struct:
        engine.Projection hands them to tvam_plan_create_double."""
        self._double_vial = TvamDoubleVial(float(r_ext_outer), float(r_int_outer), float(r_ext_inner),
                                           float(r_int_inner), float(ior_outer), float(ior_inner),
                                           float(ior_inside_inner))

    def set_traced_vial(self, traced: bool = True) -> None:
        """Mark a 'cylindrical' / 'square' vial descriptor as "trace every ray in 3-D through the glass":
        engine.Projection then creates its plan through tvam_plan_create_traced (the telecentric and
        lens projectors need it; a collimated descriptor runs the same per-ray path instead of the
        planar kernels).  The mark is not part of the C struct."""
        self._traced_vial = bool(traced)

    def set_inserts(self, inserts) -> None:
        """Dielectric occluders inside the resin: a sequence of (tris [n][3][3], int_ior, ext_ior), world
        space, wound outwards.  They are not part of the C struct: engine.Projection hands them to
        tvam_plan_create_inserts."""
        import numpy as np
        self._inserts = [(np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 3, 3), float(ni), float(ne))
                         for t, ni, ne in inserts]

    @property
    def inserts(self) -> list:
        return list(getattr(self, "_inserts", []))

    @property
    def reflected(self) -> bool:
        """transmission_only = 0 in a scene with a dielectric interface (a 'cylindrical' / 'square' vial or
        inserts): reflection is sampled there, and engine.Projection creates the plan through
        tvam_plan_create_reflect, for collimated projectors too (their paths are stochastic and leave the
        planar kernels).  An index-matched vial without inserts has no interface and is no such scene."""
        return not self.transmission_only and (self.vial_type in (VIAL_CYLINDRICAL, VIAL_SQUARE) or bool(self.inserts))

    @property
    def traced_vial(self) -> bool:
        return bool(getattr(self, "_traced_vial", False))

    def as_dict(self) -> dict:
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if isinstance(v, ctypes.Array) else v
        return out


# Entry points declared in include/tvam.h, with their ctypes signatures.
_P = ctypes.c_void_p
EXPORTS = {
    "tvam_desc_init": (None, [ctypes.POINTER(TvamDesc)]),
    "tvam_plan_create": (ctypes.c_int, [ctypes.POINTER(TvamDesc), ctypes.c_int, ctypes.POINTER(_P)]),
    "tvam_plan_create_mesh": (ctypes.c_int, [ctypes.POINTER(TvamDesc), _P, ctypes.c_int32, _P, ctypes.c_int32,
                                             ctypes.c_int, ctypes.POINTER(_P)]),
    "tvam_mesh_hit": (ctypes.c_int, [_P, ctypes.c_int32, _P, _P, ctypes.c_int64, ctypes.c_int32, _P, _P]),
    "tvam_plan_create_double": (ctypes.c_int, [ctypes.POINTER(TvamDesc), ctypes.POINTER(TvamDoubleVial), ctypes.c_int,
                                               ctypes.POINTER(_P)]),
    "tvam_plan_create_traced": (ctypes.c_int, [ctypes.POINTER(TvamDesc), ctypes.c_int, ctypes.POINTER(_P)]),
    "tvam_traced_segments": (ctypes.c_int, [ctypes.POINTER(TvamDesc), _P, _P, ctypes.c_int64, _P]),
    "tvam_plan_create_inserts": (ctypes.c_int, [ctypes.POINTER(TvamDesc), ctypes.POINTER(TvamInsert), ctypes.c_int32,
                                                ctypes.c_int, ctypes.POINTER(_P)]),
    "tvam_insert_segments": (ctypes.c_int, [ctypes.POINTER(TvamDesc), ctypes.POINTER(TvamInsert), ctypes.c_int32, _P, _P,
                                            ctypes.c_int64, _P, ctypes.c_int32, _P, _P]),
    "tvam_plan_insert_segments": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_int32, _P, _P, _P]),
    "tvam_plan_create_reflect": (ctypes.c_int, [ctypes.POINTER(TvamDesc), ctypes.POINTER(TvamInsert), ctypes.c_int32,
                                                ctypes.c_int, ctypes.POINTER(_P)]),
    "tvam_reflect_segments": (ctypes.c_int, [ctypes.POINTER(TvamDesc), ctypes.POINTER(TvamInsert), ctypes.c_int32, _P, _P,
                                             ctypes.c_int64, _P, ctypes.c_int32, _P, _P]),
    "tvam_plan_segments": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    "tvam_double_segments": (ctypes.c_int, [ctypes.POINTER(TvamDoubleVial), ctypes.c_float, ctypes.c_float,
                                            ctypes.c_float, ctypes.c_int32, _P, _P, ctypes.c_int64, _P]),
    "tvam_plan_destroy": (None, [_P]),
    "tvam_forward": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    "tvam_adjoint": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    "tvam_forward_dsigma": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    "tvam_adjoint_dsigma": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    "tvam_dsigma_weights": (ctypes.c_int, [ctypes.c_float, _P, _P, ctypes.c_int64, _P]),
    "tvam_forward_dprojector": (ctypes.c_int, [_P, ctypes.c_int32, _P, _P, ctypes.c_uint64, ctypes.c_uint32,
                                                ctypes.c_uint32, _P, _P]),
    "tvam_adjoint_dprojector": (ctypes.c_int, [_P, ctypes.c_int32, _P, _P, _P, ctypes.c_uint64, ctypes.c_uint32,
                                                ctypes.c_uint32, _P, _P]),
    "tvam_forward_slices": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_int32, ctypes.c_int32, _P, _P]),
    "tvam_plan_fwd_chunk": (ctypes.c_int, [_P]),
    "tvam_lbfgs_history": (ctypes.c_int, [ctypes.c_uint64, _P, _P, _P, _P, ctypes.c_int32, _P, _P, _P, _P, _P, _P,
                                          _P]),
    "tvam_lbfgs_direction": (ctypes.c_int, [ctypes.c_uint64, _P, ctypes.c_int32, _P, _P, ctypes.c_float, _P, _P, _P,
                                            _P]),
    "tvam_lbfgs_coef": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, _P, _P]),
    "tvam_lbfgs_direction_dev": (ctypes.c_int, [ctypes.c_uint64, _P, ctypes.c_int32, _P, _P, _P, _P, _P]),
    "tvam_lbfgs_history_rows": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _P,
                                               _P, _P, _P, ctypes.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "tvam_lbfgs_direction_rows": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _P,
                                                 ctypes.c_int32, _P, _P, _P, _P, _P]),
    "tvam_axpy_clamp": (ctypes.c_int, [ctypes.c_uint64, _P, ctypes.c_float, _P, ctypes.c_float, _P, _P]),
    "tvam_axpy_clamp_dev": (ctypes.c_int, [ctypes.c_uint64, _P, _P, _P, ctypes.c_float, _P, _P, _P]),
    "tvam_lbfgs_armijo": (ctypes.c_int, [ctypes.c_int32, ctypes.c_double, _P, _P, ctypes.c_double, ctypes.c_double,
                                         _P, ctypes.c_double, _P, _P, _P]),
    "tvam_sgd_step": (ctypes.c_int, [ctypes.c_uint64, _P, _P, _P, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                     ctypes.c_float, _P]),
    "tvam_adam_step": (ctypes.c_int, [ctypes.c_uint64, _P, _P, _P, _P, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_float, _P]),
    "tvam_adam_moments": (ctypes.c_int, [ctypes.c_uint64, _P, _P, _P, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_int32, _P, _P, _P]),
    "tvam_adam_apply": (ctypes.c_int, [ctypes.c_uint64, _P, _P, _P, _P, _P, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_int32, ctypes.c_float, _P]),
    "tvam_row_slices": (ctypes.c_int, [ctypes.POINTER(TvamDesc), _P]),
    "tvam_plan_path": (ctypes.c_int, [_P]),
    "tvam_plan_fwd_variant": (ctypes.c_int, [_P, _P]),
    "tvam_adjoint_slices": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_int32, _P, _P]),
    "tvam_plan_adj_chunk": (ctypes.c_int, [_P]),
    "tvam_plan_set_active": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64]),
    "tvam_compute_volume": (ctypes.c_int, [_P, ctypes.c_uint32, _P, _P]),
    "tvam_plan_set_volumes": (ctypes.c_int, [_P, _P]),
    "tvam_radon": (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, _P, _P]),
    "tvam_corner": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_float, ctypes.c_float, _P, _P, _P]),
    "tvam_plan_rays": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    "tvam_count_visits": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]),
    "tvam_plan_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "tvam_discretize": (ctypes.c_int, [ctypes.POINTER(TvamDesc), _P, _P]),
    "tvam_plan_fwd_scale": (ctypes.c_int, [_P, _P]),
    "tvam_plan_bin_stats": (ctypes.c_int, [_P, _P]),
    "tvam_plan_tile_stats": (ctypes.c_int, [_P, _P]),
    "tvam_plan_kernel_time": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_int64)]),
    "tvam_loss_threshold": (
        ctypes.c_int,
        [_P, _P, ctypes.c_float, _P, ctypes.c_uint64, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P, _P],
    ),
    "tvam_loss_threshold_probes": (
        ctypes.c_int,
        [_P, _P, _P, ctypes.c_int32, _P, ctypes.c_uint64, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P],
    ),
    "tvam_target_mask": (ctypes.c_int, [_P, ctypes.c_uint64, _P, _P]),
    "tvam_loss_threshold_mask": (
        ctypes.c_int,
        [_P, _P, ctypes.c_float, _P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P, _P],
    ),
    "tvam_loss_threshold_probes_mask": (
        ctypes.c_int,
        [_P, _P, _P, ctypes.c_int32, _P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_float,
         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P],
    ),
    "tvam_loss_square": (ctypes.c_int, [_P, _P, ctypes.c_float, _P, ctypes.c_uint64, ctypes.c_float, _P, _P, _P]),
    "tvam_loss_square_probes": (
        ctypes.c_int, [_P, _P, _P, ctypes.c_int32, _P, ctypes.c_uint64, ctypes.c_float, _P, _P]),
    "tvam_loss_surface": (
        ctypes.c_int,
        [ctypes.c_int32, _P, _P, ctypes.c_float, _P, ctypes.c_uint64, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P, _P],
    ),
    "tvam_loss_surface_probes": (
        ctypes.c_int,
        [ctypes.c_int32, _P, _P, _P, ctypes.c_int32, _P, ctypes.c_uint64, ctypes.c_int32, ctypes.c_float,
         ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P],
    ),
    "tvam_class_hist": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _P, ctypes.c_int32, ctypes.c_int32, _P, _P]),
    "tvam_last_error": (ctypes.c_char_p, []),
    "tvam_abi_version": (ctypes.c_int, []),
    "tvam_device_bytes": (ctypes.c_int64, []),
}

_lib = None
_lock = threading.Lock()


class TvamError(RuntimeError):
    pass


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load libtvam.so (no fallback: raises if it is absent)."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise TvamError(
                f"libtvam.so not found at {p}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or drtvam_amd/csrc/build.sh (there is no CPU fallback)"
            )
        lib = ctypes.CDLL(p)
        # the version first: a library built before an export was added fails with this message,
        # not an AttributeError from the binding loop
        ver = getattr(lib, "tvam_abi_version", None)
        if ver is None:
            raise TvamError(f"{p} exports no tvam_abi_version; rebuild it")
        ver.restype, ver.argtypes = ctypes.c_int, []
        if ver() != ABI_VERSION:
            raise TvamError(f"libtvam.so ABI version mismatch ({ver()} != {ABI_VERSION}); rebuild it")
        for name, (res, args) in EXPORTS.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise TvamError(f"libtvam.so lacks {name} (ABI {ABI_VERSION}); rebuild it")
            fn.restype = res
            fn.argtypes = args
        if path is None:
            _lib = lib
        return lib


def check(rc: int) -> None:
    if rc == TVAM_OK:
        return
    msg = load_library().tvam_last_error().decode(errors="replace")
    if rc in (TVAM_ERR_INVALID, TVAM_ERR_UNSUPPORTED):
        raise ValueError(msg)
    if rc == TVAM_ERR_TOO_LARGE:
        raise Exception(msg)
    raise TvamError(msg)


def mesh_hit(tris, o, d, use_bvh: bool = True):
    """Closest hit of rays (o, d: [n, 3]) with the triangles [m][3][3] on the host (tvam_mesh_hit):
    (t float32 [n], +inf where none; tri int32 [n], -1 where none).  No GPU is touched."""
    import numpy as np
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("mesh_hit: o and d must have the same shape")
    t = np.empty(o.shape[0], np.float32)
    tri = np.empty(o.shape[0], np.int32)
    check(load_library().tvam_mesh_hit(tris.ctypes.data if tris.size else None, tris.shape[0], o.ctypes.data,
                                       d.ctypes.data, o.shape[0], 1 if use_bvh else 0, t.ctypes.data, tri.ctypes.data))
    return t, tri


def double_segments(vial: TvamDoubleVial, medium_ior, sigma_t, height, max_depth, o, d):
    """Medium segments of world rays (o, d: [n, 3]) behind a 'double_cylindrical' vial on the host
    (tvam_double_segments, the kernels' own tracer): float32 [n, 2, 8] = o2[0:3], maxt [3],
    d2[4:7], attenuation [7]; a slot without a segment is all zeros.  No GPU is touched."""
    import numpy as np
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("double_segments: o and d must have the same shape")
    segs = np.empty((o.shape[0], 2, 8), np.float32)
    check(load_library().tvam_double_segments(ctypes.byref(vial), float(medium_ior), float(sigma_t), float(height),
                                              int(max_depth), o.ctypes.data, d.ctypes.data, o.shape[0],
                                              segs.ctypes.data))
    return segs


def traced_segments(desc: TvamDesc, o, d):
    """Medium segments of world rays (o, d: [n, 3]) behind the 'cylindrical' / 'square' vial of `desc`
    on the host (tvam_traced_segments, the kernels' own tracer): float32 [n, 8] = o2[0:3], maxt [3],
    d2[4:7], transmission weight [7]; all zeros where the ray deposits nothing.  No GPU is touched."""
    import numpy as np
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("traced_segments: o and d must have the same shape")
    segs = np.empty((o.shape[0], 8), np.float32)
    check(load_library().tvam_traced_segments(ctypes.byref(desc), o.ctypes.data, d.ctypes.data, o.shape[0],
                                              segs.ctypes.data))
    return segs


def insert_array(inserts):
    """The tvam_insert array of a descriptor's inserts (TvamDesc.inserts; the triangle arrays stay theirs),
    or None when there are none."""
    if not inserts:
        return None
    arr = (TvamInsert * len(inserts))()
    for i, (t, ni, ne) in enumerate(inserts):
        arr[i] = TvamInsert(t.ctypes.data if t.size else None, int(t.shape[0]), ni, ne)
    return arr


def insert_segments(desc: TvamDesc, o, d, u=None, max_segments: int = 8):
    """Medium segments of world rays (o, d: [n, 3]) through the container, black occluders and dielectric
    inserts of `desc` on the host (tvam_insert_segments, the kernels' own walk): (segs float32
    [n, max_segments, 8] = o2[0:3], maxt [3], d2[4:7], attenuation [7], zeros past a ray's segments; nseg int32
    [n]).  u: [n, max_depth, 4], the four draws of each loop iteration, or None: roulette never acts.  No GPU
    is touched."""
    import numpy as np
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("insert_segments: o and d must have the same shape")
    if u is not None:
        u = np.ascontiguousarray(u, dtype=np.float32)
        if u.shape != (o.shape[0], int(desc.max_depth), 4):
            raise ValueError("insert_segments: u must be [n_rays, max_depth, 4]")
    ins = desc.inserts
    arr = insert_array(ins)
    segs = np.empty((o.shape[0], int(max_segments), 8), np.float32)
    nseg = np.empty(o.shape[0], np.int32)
    check(load_library().tvam_insert_segments(ctypes.byref(desc), arr, len(ins), o.ctypes.data, d.ctypes.data,
                                              o.shape[0], None if u is None else u.ctypes.data, int(max_segments),
                                              segs.ctypes.data, nseg.ctypes.data))
    return segs, nseg


def reflect_segments(desc: TvamDesc, o, d, u, max_segments: int = 8):
    """insert_segments for a transmission_only = 0 descriptor (tvam_reflect_segments, the reflecting kernels'
    own walk): after a path's first surface, the iteration's second draw u[:, depth, 1] picks reflection
    (u <= F) or refraction at every dielectric interface.  u [n, max_depth, 4] is required.  No GPU is touched."""
    import numpy as np
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("reflect_segments: o and d must have the same shape")
    if u is None:
        raise ValueError("reflect_segments: u is required (a reflecting walk always draws)")
    u = np.ascontiguousarray(u, dtype=np.float32)
    if u.shape != (o.shape[0], int(desc.max_depth), 4):
        raise ValueError("reflect_segments: u must be [n_rays, max_depth, 4]")
    ins = desc.inserts
    arr = insert_array(ins)
    segs = np.empty((o.shape[0], int(max_segments), 8), np.float32)
    nseg = np.empty(o.shape[0], np.int32)
    check(load_library().tvam_reflect_segments(ctypes.byref(desc), arr, len(ins), o.ctypes.data, d.ctypes.data,
                                               o.shape[0], u.ctypes.data, int(max_segments), segs.ctypes.data,
                                               nseg.ctypes.data))
    return segs, nseg


def dsigma_weights(sigma_t, T0, dt):
    """The extinction derivative's visit weight w'(T0, dt) = e^{-s T0} (dt (1 - q) - T0 q), q = 1 - e^{-s dt},
    on the host in the kernels' own float32 expression (tvam_dsigma_weights): float32, T0's shape (T0 and dt
    broadcast).  No GPU is touched."""
    import numpy as np
    T0, dt = np.broadcast_arrays(np.asarray(T0, dtype=np.float32), np.asarray(dt, dtype=np.float32))
    shape = T0.shape
    T0 = np.ascontiguousarray(T0).reshape(-1)
    dt = np.ascontiguousarray(dt).reshape(-1)
    w = np.empty(T0.size, np.float32)
    check(load_library().tvam_dsigma_weights(float(sigma_t), T0.ctypes.data if T0.size else None,
                                             dt.ctypes.data if dt.size else None, T0.size,
                                             w.ctypes.data if w.size else None))
    return w.reshape(shape)


def default_desc() -> TvamDesc:
    d = TvamDesc()
    load_library().tvam_desc_init(ctypes.byref(d))
    return d

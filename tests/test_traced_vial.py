"""The 'cylindrical' and 'square' vials traced per ray in 3-D, without a GPU: the float64 model of
tests/traced_vial_model.py and the kernels' own tracer compiled for the host (tvam_traced_segments)
anchored to the oracle's planar segment, the host tracer against the model for every projector and
both vials, the coverage the scenes must have, the refusals of tvam_plan_create_traced, and the
Python mark (set_traced_vial) from the config down to the descriptor."""
import ctypes
import os
import re

import numpy as np
import pytest

from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config

import projector_model as pm
import traced_vial_model as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VIALS = ("cylindrical", "square")
KINDS = ("collimated", "telecentric", "lens")

# the project's bounds for a chain of hits, refractions and offsets (tests/test_double_vial.py):
# 4 x 64 ulp of the distance for points and lengths, 4 x 64 ulp of 1 for directions and, relatively,
# weights, each times the segment's condition number (traced_vial_model.compare_segments)
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))
# the oracle anchor: 64 ulp
ULP_O = 64 * float(np.spacing(np.float32(20.0)))
ULP_D = 64 * float(np.spacing(np.float32(1.0)))


# --------------------------------------------------------------------------- planar anchor
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
@pytest.mark.parametrize("vial", VIALS)
def test_planar_rays_reproduce_the_oracle(oracle, vial, regular):
    """On the oracle's collimated rays (d.z = 0) the host tracer and the model give the oracle's
    segment to 64 ulp, the bound of tests/test_double_vial.py's oracle anchor, asserted the same way:
    the raw errors, every ray, the hit mask equal on every ray, no conditioning factor and no
    exclusion.  (The square vial's host tracer: equal bits, it is tvam_segment_square's arithmetic;
    the tube's 2-D code refracts in the shading frame.)  The float64 model cannot be held to that:
    it is an exact-arithmetic tracer, and what separates it from the oracle is the oracle's own fp32
    rounding, which near grazing incidence the problem amplifies by kappa_d / kappa_w
    (traced_vial_model.compare_segments; measured raw on the tube: |dw|/w 3.5e-4, |dd2| 1.6e-5, and
    2.9e-5 / 4.6e-6 under regular sampling); within 1e-4 of a decision it may also rightly take the
    other branch.  So the model alone keeps 64 ulp x kappa on the rays above the margin, and the
    test asserts that those are all but 1 %."""
    spp = 1 if regular else 2
    d = tv.traced_scene(vial, "collimated", regular, angles=5)
    pix = pm.dense_pixels(d)
    rays = [oracle.ray(d, int(pix[i // spp]), i, 5) for i in range(pix.size * spp)]
    o = np.array([r["o"] for r in rays], np.float32)
    dd = np.array([r["d"] for r in rays], np.float32)
    hit = np.array([r["hit"] for r in rays])
    ref = np.array([np.r_[r["o2"], r["maxt"], r["d2"], r["weight"]] for r in rays], np.float64)
    assert np.all(dd[:, 2] == 0.0) and 0 < hit.sum() < hit.size
    m = tv.trace_desc(d, o, dd)
    ok = m["margin"] > tv.MARGIN
    assert (~ok).mean() <= 0.01
    host = _abi.traced_segments(d, o, dd).astype(np.float64)
    everything = np.ones(len(rays), bool)
    for name, got, has, rays_of in (("host", host, host[:, 3] != 0.0, everything), ("model", m["seg"], m["hit"], ok)):
        assert np.array_equal(has[rays_of], hit[rays_of])
        sel = rays_of & hit
        kd = kw = 1.0  # the host tracer: raw errors
        if name == "model":
            kd = np.maximum(1.0, 0.5 / np.sqrt(m["c2"][sel]))
            kw = np.maximum(1.0, 0.5 / m["c2"][sel])
        e_o = (np.abs(got[sel, 0:2] - ref[sel, 0:2]).max(1) / kd).max()
        e_t = (np.abs(got[sel, 3] - ref[sel, 3]) / kd).max()
        e_d = (np.abs(got[sel, 4:6] - ref[sel, 4:6]).max(1) / kd).max()
        e_w = (np.abs(got[sel, 7] / ref[sel, 7] - 1.0) / kw).max()
        print(f"{vial} {name}: compared {int(sel.sum())} of {int(hit.sum())} |do2| {e_o:.3e} |dmaxt| {e_t:.3e} (tol "
              f"{ULP_O:.3e}) |dd2| {e_d:.3e} |dw|/w {e_w:.3e} (tol {ULP_D:.3e})"
              + (f", each / kappa (largest kappa_w {np.max(kw):.1f})" if name == "model" else ", raw, every ray"))
        assert e_o <= ULP_O and e_t <= ULP_O and e_d <= ULP_D and e_w <= ULP_D
        assert np.all(got[sel, 2] == o[sel, 2]) and np.all(got[sel, 6] == 0.0)  # the ray stays in its slice
    if vial == "square":  # the same fp32 statements as the oracle's or_segment_square
        assert np.array_equal(host[hit][:, [0, 1, 3, 4, 5, 7]], ref[hit][:, [0, 1, 3, 4, 5, 7]])


# --------------------------------------------------------------------------- host tracer vs model
def _labels(m):
    return {k: int(m[k].sum()) for k in tv.LABELS}


@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("vial", VIALS)
def test_host_tracer_matches_model(vial, kind, regular):
    m = tv.scene_model(vial, kind, regular)
    d = m["desc"]
    low = float((m["margin"] <= tv.MARGIN).mean())
    assert low <= 0.01  # on the model alone
    o32, d32 = m["o"].astype(np.float32), m["d"].astype(np.float32)
    segs = _abi.traced_segments(d, o32, d32)
    ref = tv.trace_desc(d, o32, d32)  # the model traced from the rays the host tracer was given
    r = tv.compare_segments(segs, ref)
    print(f"{vial} {kind} {'regular' if regular else 'jittered'}: rays {len(segs)} compared {r['compared']} below "
          f"margin {low:.4f} |do2| {r['e_o']:.3e} |dmaxt| {r['e_t']:.3e} (tol {TOL_O:.3e}) |dd2| {r['e_d']:.3e} "
          f"|dw|/w {r['e_w']:.3e} (tol {TOL_D:.3e}), each / kappa; largest kappa_d {r['kappa_d']:.1f} kappa_w "
          f"{r['kappa_w']:.1f}; labels {_labels(m)}")
    assert r["low"] <= 0.01
    assert r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D


@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("vial", VIALS)
def test_scenes_cover_the_cases(vial, kind, regular):
    """From the model's labels alone."""
    m = tv.scene_model(vial, kind, regular)
    n = _labels(m)
    print(f"{vial} {kind} {'regular' if regular else 'jittered'}: {n} (totally reflected: {n['tir']})")
    assert n["miss"] > 0 and n["deposit"] > 0
    cone = kind != "collimated"
    if vial == "square" and cone:
        assert n["horizontal"] > 0  # a segment that starts or ends on a horizontal face
        assert n["end_entry"] > 0   # in through the outer top or bottom face
    if vial == "cylindrical" and cone:
        assert n["left_open"] > 0 and not (m["left_open"] & m["hit"]).any()  # out through an open end: no deposit
    if vial == "cylindrical" and kind == "telecentric":
        assert n["inside_first"] > 0  # in through an open end, a tube met from inside first
    if not cone:  # planar rays never leave their slice
        assert n["horizontal"] == n["end_entry"] == n["left_open"] == 0


def test_special_rays_on_the_host():
    """Single rays with known fates, host tracer and model alike."""
    d = tv.traced_scene("cylindrical", "telecentric")
    sq = tv.traced_scene("square", "telecentric")
    s = np.float32(1.0 / np.sqrt(2.0))
    o = np.array([[20, 0, 0], [20, 0, 3], [0, 0, 10], [0, 0, -5], [20, 7, 0], [20, 0, 0.5]], np.float32)
    v = np.array([[-1, 0, 0], [-1, 0, 0], [0, 0, -1], [s, 0, s], [-1, 0, 0], [-1, 0, 0]], np.float32)
    cyl = _abi.traced_segments(d, o, v)
    box = _abi.traced_segments(sq, o, v)
    mc, mb = tv.trace_desc(d, o, v), tv.trace_desc(sq, o, v)
    assert np.array_equal(cyl[:, 3] != 0, mc["hit"]) and np.array_equal(box[:, 3] != 0, mb["hit"])
    # through the axis: the chord is the inner diameter less two spawn offsets; straight on
    for segs, width in ((cyl, 2 * tv.R_INT), (box, 2 * tv.R_INT)):
        assert abs(segs[0, 3] - width) < 4 * (1 + tv.R_EXT) * tv.RAY_EPS and np.array_equal(segs[0, 4:7], [-1, 0, 0])
        # normal incidence twice: (1 - F) eta_ti^2 per interface (radiance mode), F = ((n1 - n2) / (n1 + n2))^2
        na, ng, nm = tv.IOR_AIR, tv.IOR_GLASS, tv.IOR_MEDIUM
        want = (1 - ((na - ng) / (na + ng)) ** 2) * (1 - ((ng - nm) / (ng + nm)) ** 2) * (na / nm) ** 2
        assert abs(segs[0, 7] / want - 1.0) < 1e-5
    assert not cyl[1].any() and not box[1].any()  # above both vials
    # down the axis: through the tube's open end, never a wall; through the cuvette's four
    # horizontal faces, a segment between the inner ones
    assert not cyl[2].any()
    assert abs(box[2, 3] - 2 * 1.8) < 1e-3 and np.array_equal(box[2, 4:7], [0, 0, -1]) and abs(box[2, 2] - 1.8) < 1e-3
    # up through the open end at 45 degrees, a wall from inside first: glass, then air
    assert not cyl[3].any() and mc["inside_first"][3]
    assert not cyl[4].any() and not box[4].any()  # passes beside
    assert cyl[5, 3] > 0 and cyl[5, 2] == np.float32(0.5)


# --------------------------------------------------------------------------- the C interface
def test_header_and_loader():
    hdr = open(os.path.join(ROOT, "include", "tvam.h")).read()
    assert re.search(r"#define\s+TVAM_ABI_VERSION\s+13\b", hdr)
    for name in ("tvam_plan_create_traced", "tvam_traced_segments"):
        assert re.search(r"\bint\s+%s\(" % name, hdr) and name in _abi.EXPORTS
    lib = _abi.load_library()
    assert lib.tvam_plan_create_traced.restype is ctypes.c_int and lib.tvam_traced_segments.restype is ctypes.c_int
    assert ctypes.sizeof(_abi.TvamDesc) == ctypes.sizeof(_abi.default_desc())


def _create(d, entry="tvam_plan_create_traced"):
    lib = _abi.load_library()
    plan = ctypes.c_void_p()
    rc = getattr(lib, entry)(ctypes.byref(d), 0, ctypes.byref(plan))
    assert not plan.value
    return rc, lib.tvam_last_error().decode()


def _segments_rc(d):
    lib = _abi.load_library()
    o = np.array([[20, 0, 0]], np.float32)
    v = np.array([[-1, 0, 0]], np.float32)
    out = np.full((1, 8), 7.0, np.float32)
    return lib.tvam_traced_segments(ctypes.byref(d), o.ctypes.data, v.ctypes.data, 1, out.ctypes.data)


@pytest.mark.parametrize("vial", VIALS)
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_name_the_combination(vial, kind):
    """Every refusal comes from validation, before any HIP call: it holds on a machine without a GPU."""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    base = tv.traced_scene(vial, kind)
    pat = f"the '{kind}' projector with "

    def unsupported(d, what):
        rc, msg = _create(d)
        assert rc == _abi.TVAM_ERR_UNSUPPORTED and (pat + what) in msg, (rc, msg)
        assert _segments_rc(d) == _abi.TVAM_ERR_INVALID

    def invalid(d, what):
        rc, msg = _create(d)
        assert rc == _abi.TVAM_ERR_INVALID and what in msg, (rc, msg)
        assert _segments_rc(d) == _abi.TVAM_ERR_INVALID

    d = base.copy()
    d.set_occluders(tri)
    unsupported(d, "occluders")
    d = base.copy()
    d.albedo = 0.5
    unsupported(d, "a scattering medium")
    d = base.copy()
    d.sensor_type, d.majorant = _abi.SENSOR_RATIO, 3.0
    unsupported(d, "the 'ratio' sensor")
    d = base.copy()
    d.sensor_type = _abi.SENSOR_DELTA
    unsupported(d, "the 'delta' sensor")
    d = base.copy()
    d.film_channels = 2
    d.set_target(tri)
    unsupported(d, "a surface-aware film")
    d = base.copy()
    d.slab_begin, d.slab_end = 0, 10
    unsupported(d, "film slabs")
    d = base.copy()
    d.transmission_only = 0
    unsupported(d, "transmission_only = 0")
    d = base.copy()
    d.rr_depth = 1
    unsupported(d, "rr_depth < 2")
    for vt in (_abi.VIAL_INDEX_MATCHED, _abi.VIAL_CUSTOM, _abi.VIAL_DOUBLE_CYLINDRICAL):
        d = base.copy()
        d.vial_type = vt
        invalid(d, "tvam_plan_create")
    d = base.copy()
    d.vial_r_ext = d.vial_r
    invalid(d, "r_ext > r_int")
    for field in ("vial_r", "vial_height", "vial_ior", "medium_ior"):
        d = base.copy()
        setattr(d, field, 0.0)
        invalid(d, "glass vial")
    if kind != "collimated":
        d = base.copy()
        d.focus_distance = 0.0
        invalid(d, "focus_distance must be positive")
        d = base.copy()
        d.aperture_radius = -1.0
        invalid(d, "aperture_radius must be >= 0")
        # tvam_plan_create keeps refusing the combination, with its old prefix, and names the new entry
        rc, msg = _create(base, "tvam_plan_create")
        assert rc == _abi.TVAM_ERR_UNSUPPORTED and f"{pat}a '{vial}' vial" in msg and "tvam_plan_create_traced" in msg
    assert _segments_rc(base) == 0


def test_row_slices_refuse_3d_descriptors():
    """tvam_row_slices takes a descriptor, not a plan: a telecentric / lens descriptor with a glass
    vial (the ones the config path marks for the traced entry) has no row <-> slice map and is
    refused, with the message that names the traced entry; a collimated glass-vial descriptor is a
    planar one there whatever entry later creates its plan (TvamProblem refuses slab sharding for a
    traced plan before it asks)."""
    lib = _abi.load_library()
    for vial in VIALS:
        for kind in ("telecentric", "lens"):
            d = tv.traced_scene(vial, kind)
            rows = np.zeros(d.crop_y, np.int32)
            assert lib.tvam_row_slices(ctypes.byref(d), rows.ctypes.data) == _abi.TVAM_ERR_UNSUPPORTED
            msg = lib.tvam_last_error().decode()
            assert f"the '{kind}' projector with a '{vial}' vial" in msg and "tvam_plan_create_traced" in msg
        d = tv.traced_scene(vial, "collimated", True)
        rows = np.full(d.crop_y, -7, np.int32)
        assert lib.tvam_row_slices(ctypes.byref(d), rows.ctypes.data) == 0 and rows.max() >= 0 and rows.min() >= -1


def test_null_arguments():
    lib = _abi.load_library()
    d = tv.traced_scene("square", "lens")
    assert lib.tvam_plan_create_traced(None, 0, None) == _abi.TVAM_ERR_INVALID
    assert lib.tvam_traced_segments(ctypes.byref(d), None, None, 1, None) == _abi.TVAM_ERR_INVALID
    assert lib.tvam_traced_segments(ctypes.byref(d), None, None, 0, None) == 0


# --------------------------------------------------------------------------- Python
def test_mark_travels_with_the_descriptor():
    d = _abi.default_desc()
    assert not d.traced_vial and not d.copy().traced_vial
    d.set_traced_vial()
    assert d.traced_vial and d.copy().traced_vial and d.copy().copy().traced_vial
    d.set_traced_vial(False)
    assert not d.traced_vial and not d.copy().traced_vial


@pytest.mark.parametrize("vial", VIALS)
def test_config_marks_telecentric_and_lens_only(vial):
    for kind in KINDS:
        d = desc_from_config(tv.traced_config(vial, kind))
        assert d.traced_vial == (kind != "collimated"), (vial, kind)
        assert d.vial_type == (_abi.VIAL_CYLINDRICAL if vial == "cylindrical" else _abi.VIAL_SQUARE)
    # other vials are never marked
    from double_vial_model import double_scene
    assert not pm.projector_scene("telecentric").traced_vial and not double_scene("lens").traced_vial

"""The 'double_cylindrical' vial without a GPU: the float64 model of tests/double_vial_model.py
against the closed form of the medium chords and against the oracle where the two coincide, the
kernels' own tracer compiled for the host (tvam_double_segments) against the model, the C entry
points' refusals, DoubleCylindricalVial's to_dict / fill_desc, and the margin cap the GPU tests of
tests/test_gpu_double_vial.py rely on."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest

from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config

import double_vial_model as dv
import projector_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the bounds of tests/test_gpu_mesh_vial.py's export-vs-model comparison (the same operations: tube
# hit, transmit, offset, chained): 4 x 64 ulp of the distance for points and lengths, 4 x 64 ulp of 1
# for directions and, relatively, weights -- each times the segment's condition number towards
# grazing incidence and total internal reflection (double_vial_model.compare_segments), which is 1
# for all but a few rays
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))


def ref_vial():
    return _abi.TvamDoubleVial(*dv.RADII, dv.IOR_OUTER, dv.IOR_INNER, dv.IOR_CORE)


# --------------------------------------------------------------------------- model vs closed form
def test_model_matches_closed_form_chords():
    """The reference config's radii and IORs at its 24 impact parameters: 0 / 1 / 2 segments, the
    totally reflected ray, the loop iteration of each deposit, and the chords of Bouguer's invariant.
    The model's segments are shorter than the closed form's only by the spawn offsets at their two
    ends, (1 + max|h|) RayEpsilon along the normal, i.e. / cos(incidence) along the ray."""
    b = dv.IMPACT
    o, d = dv.planar_rays(b)
    m = dv.trace(o, d, max_depth=10)
    chord, nsegs = dv.chords(b)
    tir = np.isclose(b, 2.85)
    assert np.array_equal(m["n"], np.where(tir, 1, nsegs))
    assert m["n"][-1] == 0 and b[-1] == pytest.approx(7.05)                      # misses the vial
    assert np.all(m["n"][(b > 4.5) & (b < 7.0)] == 1)                            # the medium alone
    assert np.all(m["n"][(b > 3.0) & (b < 4.5)] == 2)                            # the inner glass alone
    assert np.all(m["n"][b < 2.7] == 2)                                          # through the core
    it = m["iters"]
    assert np.all(it[m["n"] >= 1, 0] == 2)
    assert np.all(it[(b > 3.0) & (b < 4.5), 1] == 4) and np.all(it[b < 2.7, 1] == 6)
    assert it[tir, 1] == -1
    for k in range(2):
        sel = m["n"] > k
        seg = m["segs"][sel, k]
        got = seg[:, 3]
        # The spawn offsets, off = (1 + max|h|) RayEpsilon <= (1 + r0) RayEpsilon along the normal, are
        # all that separates the model from the closed form, to first order in two ways.  (1) Both
        # ends of a segment sit an offset inside their tubes: the segment is shorter by off /
        # cos(incidence) per end, cos = sqrt(1 - (b_m / r)^2) on r1 (outer end) and on r2 (inner
        # end of a two-segment ray) or r1 again.  (2) Every crossing before the segment moves the
        # ray's line sideways by off sin(theta) <= off, i.e. the invariant b_m by at most
        # off n / n_medium <= 1.05 off per crossing (2 before the first segment, up to 6 before the
        # second), and the chord follows with slope |dc / db_m| = b_m |1 / sqrt(r1^2 - b_m^2) -
        # 1 / sqrt(r2^2 - b_m^2)| (two segments) or 2 b_m / sqrt(r1^2 - b_m^2) (one).
        bm = b[sel] * dv.IOR_AIR / float(np.float32(dv.IOR_MEDIUM))
        two = nsegs[sel] == 2
        r1, r2 = dv.RADII[1], dv.RADII[2]
        off = (1.0 + dv.RADII[0]) * dv.RAY_EPS
        c1 = np.sqrt(1.0 - (bm / r1) ** 2)
        c2 = np.sqrt(1.0 - np.minimum(bm / r2, 0.999) ** 2)
        ends = off / c1 + np.where(two, off / c2, off / c1)
        slope = np.where(two, bm * np.abs(1.0 / (r1 * c1) - 1.0 / (r2 * c2)), 2.0 * bm / (r1 * c1))
        slack = ends + slope * (2 if k == 0 else 6) * 1.05 * off
        err = chord[sel] - got
        print(f"segment {k}: chord - model in [{err.min():.3e}, {err.max():.3e}], bound from {slack.min():.3e} to "
              f"{slack.max():.3e}")
        assert np.all(np.abs(err) <= slack)
        assert np.allclose(np.linalg.norm(seg[:, 4:7], axis=1), 1.0, atol=1e-12)
    # the second segment starts with the first one's absorption
    two = m["n"] == 2
    s0, s1 = m["segs"][two, 0], m["segs"][two, 1]
    assert np.all(s1[:, 7] < s0[:, 7] * np.exp(-dv.SIGMA_T * s0[:, 3]) * (1 + 1e-12))
    assert np.all(s1[:, 7] > 0.5 * s0[:, 7] * np.exp(-dv.SIGMA_T * s0[:, 3]))


@pytest.mark.parametrize("max_depth,expect", [(2, (0, 0, 0)), (3, (1, 1, 1)), (5, (1, 2, 1)), (7, (2, 2, 1)),
                                              (10, (2, 2, 1))])
def test_max_depth_bounds_the_deposits(max_depth, expect):
    """Segments per class of ray (through the core, through the inner glass alone, the medium alone):
    the first deposit is loop iteration 2, the second 4 or 6.  Model and host tracer."""
    b = dv.IMPACT
    o, d = dv.planar_rays(b)
    core, glass, medium = b < 2.7, (b > 3.0) & (b < 4.5), (b > 4.5) & (b < 7.0)
    m = dv.trace(o, d, max_depth=max_depth)
    segs = _abi.double_segments(ref_vial(), dv.IOR_MEDIUM, dv.SIGMA_T, dv.HEIGHT, max_depth, o, d)
    n_host = (segs[:, :, 3] != 0).sum(1)
    for n in (m["n"], n_host):
        assert np.all(n[core] == expect[0]) and np.all(n[glass] == expect[1]) and np.all(n[medium] == expect[2])
        assert n[-1] == 0 and n[np.isclose(b, 2.85)] == min(1, expect[2])


# --------------------------------------------------------------------------- host tracer vs model
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
@pytest.mark.parametrize("kind", ["collimated", "telecentric", "lens"])
def test_host_tracer_matches_model(kind, regular):
    m = dv.scene_model(kind, regular, 2, 3)
    d = m["desc"]
    segs = _abi.double_segments(d._double_vial, d.medium_ior, d.sigma_t, d.vial_height, d.max_depth,
                                m["o"].astype(np.float32), m["d"].astype(np.float32))
    # the model traced from the rays the host tracer was given (fp32-rounded o, d)
    radii, eta, st, height = dv.vial_of(d)
    ref = dv.trace(m["o"].astype(np.float32), m["d"].astype(np.float32), radii, eta, st, height, d.max_depth)
    low = float((m["margin"] <= dv.MARGIN).mean())
    assert low <= 0.01  # on the model alone
    r = dv.compare_segments(segs, ref)
    print(f"{kind} {'regular' if regular else 'jittered'}: rays {len(segs)} segments compared {r['compared']} "
          f"below margin {low:.4f} |do2| {r['e_o']:.3e} |dmaxt| {r['e_t']:.3e} (tol {TOL_O:.3e}) "
          f"|dd2| {r['e_d']:.3e} |dw|/w {r['e_w']:.3e} (tol {TOL_D:.3e}), each / kappa; largest kappa_d "
          f"{r['kappa_d']:.1f} kappa_w {r['kappa_w']:.1f}")
    assert r["low"] <= 0.01
    assert r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D
    counts = np.bincount(ref["n"], minlength=3)
    assert counts[1] > 0 and counts[2] > 0  # one- and two-segment rays both occur


def test_margin_shares():
    """Regular sampling at pitch 0.3 keeps every ray well away from a decision; uniformly jittered
    impact parameters put well under 1 % below the margin (model alone)."""
    m = dv.trace(*dv.planar_rays(dv.IMPACT))
    assert m["margin"].min() > 5e-3
    rng = np.random.default_rng(0)
    b = rng.uniform(0.0, 7.2, 200000)
    mj = dv.trace(*dv.planar_rays(b))
    low = float((mj["margin"] <= dv.MARGIN).mean())
    print(f"regular: least margin {m['margin'].min():.4f}; jittered: {low:.5f} below {dv.MARGIN}")
    assert low <= 0.01


# --------------------------------------------------------------------------- oracle anchors
def _oracle_rays(oracle, d, seed=5):
    pix = pm.dense_pixels(d)
    return [oracle.ray(d, int(pix[i]), i, seed) for i in range(pix.size)]


def _cyl_desc(radii, ior_outer, regular=True):
    """The oracle's cylindrical vial r_int_outer / r_ext_outer / ior_outer on the double scene's
    projector and film."""
    cfg = dv.double_config("collimated", regular, max_depth=10)
    cfg["vial"] = {"type": "cylindrical", "r_int": radii[1], "r_ext": radii[0], "ior": ior_outer,
                   "medium": cfg["vial"]["medium"]}
    return desc_from_config(cfg)


def test_anchor_thin_inner_tube_equals_oracle_cylindrical(oracle):
    """(a) inner tube 0.05 / 0.02: no pixel-centre ray reaches it at an even DMD width and pitch 0.3
    (|b| min 0.15, beyond r_ext_inner n_medium / n_air = 0.074), so every ray's single segment is the
    oracle's ray of the cylindrical vial r_int_outer / r_ext_outer / ior_outer."""
    radii = (7.0, 6.0, 0.05, 0.02)
    d = dv.double_scene("collimated", True, radii=radii)
    dc = _cyl_desc(radii, dv.IOR_OUTER)
    rays = _oracle_rays(oracle, dc)
    o = np.array([r["o"] for r in rays], np.float32)
    dd = np.array([r["d"] for r in rays], np.float32)
    segs = _abi.double_segments(d._double_vial, d.medium_ior, d.sigma_t, d.vial_height, d.max_depth, o, dd)
    hit = np.array([r["hit"] for r in rays])
    assert np.array_equal(segs[:, 0, 3] != 0, hit) and not segs[:, 1].any() and 0 < hit.sum() < hit.size
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    e_o = np.abs(segs[hit, 0, 0:3] - np.array([r["o2"] for r in rays])[hit]).max()
    e_t = np.abs(segs[hit, 0, 3] - np.array([r["maxt"] for r in rays])[hit]).max()
    e_d = np.abs(segs[hit, 0, 4:7] - np.array([r["d2"] for r in rays])[hit]).max()
    e_w = np.abs(segs[hit, 0, 7] / np.array([r["weight"] for r in rays])[hit] - 1.0).max()
    print(f"|do2| {e_o:.3e} |dmaxt| {e_t:.3e} (tol {tol_o:.3e}) |dd2| {e_d:.3e} |dw|/w {e_w:.3e} (tol {tol_d:.3e})")
    assert e_o <= tol_o and e_t <= tol_o and e_d <= tol_d and e_w <= tol_d


def test_anchor_invisible_inner_tube(oracle):
    """(b) ior_inner = ior_inside_inner = the medium's: the inner tube refracts nothing.  d2 of both
    segments is the oracle's direction, the second segment ends where the oracle's segment ends, and
    the two weights differ by exactly exp(-sigma_t len1)."""
    d = dv.double_scene("collimated", True, ior_inner=dv.IOR_MEDIUM, core=dv.IOR_MEDIUM)
    dc = _cyl_desc(dv.RADII, dv.IOR_OUTER)
    rays = _oracle_rays(oracle, dc)
    o = np.array([r["o"] for r in rays], np.float32)
    dd = np.array([r["d"] for r in rays], np.float32)
    segs = _abi.double_segments(d._double_vial, d.medium_ior, d.sigma_t, d.vial_height, d.max_depth, o, dd)
    hit = np.array([r["hit"] for r in rays])
    n = (segs[:, :, 3] != 0).sum(1)
    assert np.array_equal(n > 0, hit) and (n == 2).sum() > 0 and (n == 1).sum() > 0
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    o2 = np.array([r["o2"] for r in rays], np.float64)
    d2 = np.array([r["d2"] for r in rays], np.float64)
    end = o2 + d2 * np.array([r["maxt"] for r in rays])[:, None]
    two = n == 2
    s0, s1 = segs[two, 0].astype(np.float64), segs[two, 1].astype(np.float64)
    # four more offsets lie between the oracle's entry and the second segment's end: 4 x the bound
    e_d = max(np.abs(s0[:, 4:7] - d2[two]).max(), np.abs(s1[:, 4:7] - d2[two]).max())
    e_end = np.abs(s1[:, 0:3] + s1[:, 4:7] * s1[:, 3:4] - end[two]).max()
    e_o = np.abs(s0[:, 0:3] - o2[two]).max()
    print(f"|dd2| {e_d:.3e} (tol {tol_d:.3e}) |dend| {e_end:.3e} |do2| {e_o:.3e} (tol {4 * tol_o:.3e})")
    assert e_d <= tol_d and e_o <= tol_o and e_end <= 4 * tol_o
    # eta = 1 interfaces transmit with weight exactly 1 (Mitsuba's fresnel: r = 0 at eta == 1)
    w0, w1, len1 = segs[two, 0, 7], segs[two, 1, 7], segs[two, 0, 3]
    # and the second weight is the first times e^{-sigma_t len1}, to the rounding of one fp32 expf and product
    ratio = w1 / (w0.astype(np.float64) * np.exp(-float(np.float32(d.sigma_t)) * len1.astype(np.float64)))
    assert np.abs(ratio - 1.0).max() <= 2 * float(np.spacing(np.float32(1.0)))
    one = n == 1
    e_t = np.abs(segs[one, 0, 3] - np.array([r["maxt"] for r in rays])[one]).max()
    assert e_t <= tol_o


# --------------------------------------------------------------------------- the C ABI
def test_header_and_loader():
    hdr = open(os.path.join(ROOT, "include", "tvam.h")).read()
    assert re.search(r"#define\s+TVAM_VIAL_DOUBLE_CYLINDRICAL\s+4\b", hdr)
    assert re.search(r"#define\s+TVAM_ABI_VERSION\s+13\b", hdr)
    names = {"tvam_plan_create_double", "tvam_plan_segments", "tvam_double_segments"}
    assert all(n in hdr for n in names) and "typedef struct tvam_double_vial" in hdr
    assert _abi.VIAL_DOUBLE_CYLINDRICAL == 4 and _abi.ABI_VERSION == 13
    assert names <= set(_abi.EXPORTS)
    lib = _abi.load_library()
    assert lib.tvam_abi_version() == 13
    assert ctypes.sizeof(_abi.TvamDoubleVial) == 28


def _create(d, vial):
    lib = _abi.load_library()
    plan = ctypes.c_void_p()
    rc = lib.tvam_plan_create_double(ctypes.byref(d), None if vial is None else ctypes.byref(vial), 0,
                                     ctypes.byref(plan))
    assert not plan.value  # no plan was created
    return rc, lib.tvam_last_error().decode()


def test_refusals_name_the_combination():
    """Every refusal comes from validation, before any HIP call: it holds on a machine without a GPU."""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    lib = _abi.load_library()

    def base():
        return dv.double_scene("telecentric")

    plan = ctypes.c_void_p()
    d = base()
    assert lib.tvam_plan_create(ctypes.byref(d), 0, ctypes.byref(plan)) == _abi.TVAM_ERR_INVALID
    assert "tvam_plan_create_double" in lib.tvam_last_error().decode() and not plan.value

    def unsupported(d, what):
        rc, msg = _create(d, d._double_vial)
        assert rc == _abi.TVAM_ERR_UNSUPPORTED and msg.startswith("a 'double_cylindrical' vial with " + what), msg

    d = base()
    d.set_occluders(tri)
    unsupported(d, "occluders")
    d = base()
    d.albedo = 0.5
    unsupported(d, "a scattering medium (albedo > 0)")
    d = base()
    d.sensor_type, d.majorant = _abi.SENSOR_RATIO, 3.0
    unsupported(d, "the 'ratio' sensor")
    d = base()
    d.sensor_type = _abi.SENSOR_DELTA
    unsupported(d, "the 'delta' sensor")
    d = base()
    d.film_channels = 2
    d.set_target(tri)
    unsupported(d, "a surface-aware film")
    d = base()
    d.slab_begin, d.slab_end = 0, 10
    unsupported(d, "film slabs")
    d = base()
    d.transmission_only = 0
    unsupported(d, "transmission_only = 0")
    d = base()
    d.rr_depth = 5  # max_depth 10: the last deposit is at iteration 6
    unsupported(d, "rr_depth < min(max_depth, 7) - 1")
    d = base()
    d.max_depth, d.rr_depth = 3, 1
    unsupported(d, "rr_depth < min(max_depth, 7) - 1")

    def invalid(vial, what, d=None):
        rc, msg = _create(base() if d is None else d, vial)
        assert rc == _abi.TVAM_ERR_INVALID and what in msg, msg

    order = "r_ext_outer > r_int_outer > r_ext_inner > r_int_inner > 0"
    invalid(None, "needs its tvam_double_vial")
    invalid(_abi.TvamDoubleVial(7, 7, 3, 2, 1.5, 1.5, 1.3), order)
    invalid(_abi.TvamDoubleVial(7, 6, 6.5, 2, 1.5, 1.5, 1.3), order)
    invalid(_abi.TvamDoubleVial(7, 6, 3, 0, 1.5, 1.5, 1.3), order)
    invalid(_abi.TvamDoubleVial(7, 6, 3, float("nan"), 1.5, 1.5, 1.3), order)
    invalid(_abi.TvamDoubleVial(7, 6, 3, 2, 0.0, 1.5, 1.3), "positive IORs")
    invalid(_abi.TvamDoubleVial(7, 6, 3, 2, 1.5, -1.0, 1.3), "positive IORs")
    invalid(_abi.TvamDoubleVial(7, 6, 3, 2, 1.5, 1.5, 0.0), "positive IORs")
    d = base()
    d.medium_ior = 0.0
    invalid(d._double_vial, "positive IORs", d)
    # the other vial types cannot take the entry, and the host tracer refuses the same vials
    invalid(ref_vial(), "TVAM_VIAL_DOUBLE_CYLINDRICAL", pm.projector_scene("collimated"))
    o = np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match=order):
        _abi.double_segments(_abi.TvamDoubleVial(7, 6, 3, 4, 1.5, 1.5, 1.3), 1.48, 0.05, 40.0, 10, o, o)
    # a descriptor with valid settings passes validation: the refusal is then the missing GPU's or none
    assert lib.tvam_row_slices(ctypes.byref(dv.double_scene("collimated")), (ctypes.c_int32 * 8)()) == \
        _abi.TVAM_ERR_UNSUPPORTED
    assert "'double_cylindrical'" in lib.tvam_last_error().decode()


# --------------------------------------------------------------------------- Python
def reference_config():
    with open(os.path.join(GOLDEN, "double_cylindrical.json")) as f:
        cfg = json.load(f)
    cfg["target"]["filename"] = os.path.join(GOLDEN, "hollow_gear.ply")
    return cfg


def test_double_vial_fills_the_descriptor():
    cfg = reference_config()
    d = desc_from_config(cfg)
    assert d.vial_type == _abi.VIAL_DOUBLE_CYLINDRICAL and d.projector_type == _abi.PROJECTOR_COLLIMATED
    v = d._double_vial
    assert (v.r_ext_outer, v.r_int_outer, v.r_ext_inner, v.r_int_inner) == (7.0, 6.0, 3.0, 2.0)
    assert (v.ior_outer, v.ior_inner, v.ior_inside_inner) == (np.float32(1.53), np.float32(1.553), np.float32(1.33))
    assert d.medium_ior == np.float32(1.48) and d.sigma_t == np.float32(0.05) and d.albedo == 0.0
    assert d.vial_height == 40.0 and d.max_depth == 10 and d.rr_depth == 6
    assert (tuple(d.film_res), d.n_patterns, d.res_x, d.res_y) == ((50, 50, 1), 200, 200, 10)
    c = d.copy()
    assert c._double_vial is d._double_vial and c.vial_type == _abi.VIAL_DOUBLE_CYLINDRICAL
    named = copy.deepcopy(cfg)
    named["vial"] |= {"ior_outer": "bk7", "ior_inside_inner": "air"}
    v = desc_from_config(named)._double_vial
    assert v.ior_outer == np.float32(1.5046) and v.ior_inside_inner == np.float32(1.000277)


def test_double_vial_dict_and_scene_round_trip():
    from drtvam_amd.geometry import DoubleCylindricalVial
    from drtvam_amd.scene import _container_from_shapes
    cfg = reference_config()
    v = DoubleCylindricalVial(cfg["vial"])
    sd = v.to_dict()
    ref = {"type": "ref", "id": "printing_medium"}
    expect = {
        "outer_vial": (7, {"int_ior": 1.53}, {}),
        "outer_vial_interior": (6, {"ext_ior": 1.53, "int_ior": 1.48}, {"interior": ref}),
        "inner_vial": (3, {"ext_ior": 1.48, "int_ior": 1.553}, {"exterior": ref}),
        "inner_vial_interior": (2, {"ext_ior": 1.553, "int_ior": 1.33}, {}),
    }
    assert set(sd) == set(expect) | {"printing_medium"}
    assert sd["printing_medium"] == {"type": "homogeneous", "sigma_t": 0.05, "albedo": 0.0}
    for key, (r, ior, medium) in expect.items():
        assert sd[key] == {"type": "cylinder", "p0": [0.0, 0.0, -20.0], "p1": [0.0, 0.0, 20.0], "radius": r,
                           "bsdf": {"type": "dielectric", **ior}, **medium}
    back = _container_from_shapes(sd)
    assert isinstance(back, DoubleCylindricalVial)
    assert (back.r_ext_outer, back.r_int_outer, back.r_ext_inner, back.r_int_inner) == (7, 6, 3, 2)
    assert (back.vial_ior_outer, back.vial_ior_inner, back.inside_inner_ior, back.medium_ior) == (1.53, 1.553, 1.33, 1.48)
    assert back.height == 40.0 and back.sigma_t == 0.05
    # the reference's own medium parsing: albedo is required, a scattering medium needs its phase
    bad = copy.deepcopy(cfg["vial"])
    del bad["medium"]["albedo"]
    with pytest.raises(KeyError):
        DoubleCylindricalVial(bad)
    bad = copy.deepcopy(cfg["vial"])
    bad["medium"]["albedo"] = 0.5
    with pytest.raises(ValueError, match="without specifying a phase function"):
        DoubleCylindricalVial(bad)
    occ = copy.deepcopy(cfg["vial"])
    occ["occlusions"] = [{"filename": os.path.join(GOLDEN, "occlusion.ply")}]
    with pytest.raises(NotImplementedError, match="a 'double_cylindrical' vial with occluders"):
        DoubleCylindricalVial(occ).fill_desc(_abi.default_desc())


def test_load_scene_of_the_reference_config():
    from drtvam_amd.geometry import DoubleCylindricalVial
    from discretize_util import scene_of
    scene, sensor = scene_of(reference_config())
    assert isinstance(scene.container, DoubleCylindricalVial)
    assert tuple(sensor.resolution()) == (50, 50, 1)
    assert scene.projector is not None and scene.target is not None

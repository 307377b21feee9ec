"""Reflected paths (transmission_only = 0) at the C ABI, without a GPU: tvam_reflect_segments, the
walk the reflecting kernels run (tvam_insert_next<REFLECT>), against closed forms and the float64
model of tests/reflect_model.py on every scene the GPU tests use; the anchor to the transmission-only
walk where every Fresnel reflectance is 0; the statistics of the sampled branch; the checker's own
sensitivity (planted errors); and tvam_plan_create_reflect's refusals, which all come before any
device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from drtvam_amd import _abi

import insert_model as im
import projector_model as pm
import reflect_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tvam_plan_create_reflect", "tvam_reflect_segments"}
# tests/test_gpu_inserts.py's export-vs-model bounds (times the segment's condition number,
# double_vial_model.compare_segments)
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))
F32 = np.float32
N_AIR = float(F32(1.000277))


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("reflect_meshes")
    im.write_meshes(d)
    return d


def test_header_and_loader():
    hdr = open(ROOT + "/include/tvam.h").read()
    assert re.search(r"#define\s+TVAM_ABI_VERSION\s+13\b", hdr) and _abi.ABI_VERSION == 13  # additions only
    assert all(n in hdr for n in NAMES) and NAMES <= set(_abi.EXPORTS)
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES)


# --------------------------------------------------------------------------- 1. closed forms
def square_desc(meshdir, **kw):
    """The cuvette of the scenes: inner half width 2.9, outer 3.2, glass 1.9, resin 1.2, sigma_t 1."""
    return rm.reflect_scene(meshdir, "square", "collimated", True, **kw)


def draws(desc, n=1, s1=0.9):
    """Draws that never reflect (s1 = 0.9 exceeds every F below 0.9) and never stop at the roulette."""
    u = np.zeros((n, int(desc.max_depth), 4), np.float32)
    u[:, :, 1] = s1
    return u


CENTRE_O = np.array([[20.0, 0.0, 0.0]], np.float32)
CENTRE_D = np.array([[-1.0, 0.0, 0.0]], np.float32)


def normal_F(n1, n2):
    return ((n1 - n2) / (n1 + n2)) ** 2


def test_closed_form_forced_reflection_at_the_far_inner_face(meshdir):
    """Normal incidence through the centre.  Surfaces: 0 outer face (forced transmission), 1 inner face,
    2 the far inner face met from the resin (first deposit), 3 the near inner face met from the resin."""
    d = square_desc(meshdir)
    sig = float(F32(d.sigma_t))
    u = draws(d)
    u[0, 2, 1] = 0.0  # s1 = 0 <= F: the path reflects at the far inner face
    segs, nseg = _abi.reflect_segments(d, CENTRE_O, CENTRE_D, u, 8)
    assert nseg[0] >= 2
    s0, s1 = segs[0, 0].astype(np.float64), segs[0, 1].astype(np.float64)
    ng, nr = float(F32(rm.IOR_GLASS)), float(F32(rm.IOR_MEDIUM))
    # first segment: forced transmission (1 - F) eta_ti^2 at the outer face, eta_ti^2 alone at the sampled inner one
    w0 = (1.0 - normal_F(N_AIR, ng)) * (N_AIR / ng) ** 2 * (ng / nr) ** 2
    assert abs(s0[7] / w0 - 1.0) < 1e-5
    assert abs(s0[0] - 2.9) < 1e-3 and np.allclose(s0[4:7], [-1, 0, 0], atol=1e-6) and abs(s0[3] - 5.8) < 2e-3
    # second segment: starts at the far face, reversed, attenuation (the first segment's) e^{-sigma L}, weight 1
    assert abs(s1[0] + 2.9) < 1e-3 and s1[0] > -2.9 and np.allclose(s1[4:7], [1, 0, 0], atol=1e-6)
    assert abs(s1[0] - (s0[0] - s0[3])) < 1e-3
    assert abs(s1[7] / (s0[7] * np.exp(-sig * s0[3])) - 1.0) < 1e-5
    # the same ray without that reflection: one refraction out, the path leaves the vial
    segs_t, nseg_t = _abi.reflect_segments(d, CENTRE_O, CENTRE_D, draws(d), 8)
    assert nseg_t[0] == 1 and np.array_equal(segs_t[0, 0], segs[0, 0])


def test_closed_form_refraction_weight_has_no_fresnel_factor(meshdir):
    d = square_desc(meshdir)
    segs, nseg = _abi.reflect_segments(d, CENTRE_O, CENTRE_D, draws(d), 8)
    ng, nr = float(F32(rm.IOR_GLASS)), float(F32(rm.IOR_MEDIUM))
    first = (1.0 - normal_F(N_AIR, ng)) * (N_AIR / ng) ** 2  # the forced transmission of depth 0
    ratio = float(segs[0, 0, 7]) / first
    assert abs(ratio / (ng / nr) ** 2 - 1.0) < 1e-5          # eta_ti^2
    assert abs(ratio / ((1.0 - normal_F(ng, nr)) * (ng / nr) ** 2) - 1.0) > 0.04  # and not (1 - F) eta_ti^2 (F = 5.1 %)
    # the transmission-only walk of the same scene keeps the factor
    dt = d.copy()
    dt.transmission_only = 1
    dt.set_inserts([(im.mesh("far"), 1.5, 1.5)])
    st, _ = _abi.insert_segments(dt, CENTRE_O, CENTRE_D, None, 8)
    assert abs(float(st[0, 0, 7]) / (first * (1.0 - normal_F(ng, nr)) * (ng / nr) ** 2) - 1.0) < 1e-5


def test_depth_0_transmission_is_forced_whatever_s1_is(meshdir):
    d = square_desc(meshdir)
    a, na = _abi.reflect_segments(d, CENTRE_O, CENTRE_D, draws(d), 8)
    u = draws(d)
    u[0, 0, 1] = 0.0  # would reflect off the outer face if depth 0 sampled
    b, nb = _abi.reflect_segments(d, CENTRE_O, CENTRE_D, u, 8)
    assert nb[0] == na[0] == 1 and np.array_equal(a, b)
    # at depth 1 the same draw does reflect: the path turns back inside the glass and never reaches the resin
    u = draws(d)
    u[0, 1, 1] = 0.0
    c, nc = _abi.reflect_segments(d, CENTRE_O, CENTRE_D, u, 8)
    assert nc[0] == 0 and not c.any()


def test_total_internal_reflection_reflects(meshdir):
    """A slab insert (2.2 in 1.2) met obliquely: inside it the ray meets the side face beyond the critical angle.
    The transmission-only walk ends there ('tir'); the reflecting walk reflects whatever s1 is, as the model does."""
    slab = im.box_tris((-1.0, -0.25, -0.5), (1.0, 0.25, 0.5)).astype(np.float32)
    d = square_desc(meshdir)
    d.set_inserts([(slab, rm.INT_IOR, rm.EXT_IOR)])
    dt = d.copy()
    dt.transmission_only = 1
    a = np.deg2rad(40.0)
    ys = np.linspace(-17.0, -13.0, 161)
    o = np.stack([np.full_like(ys, 20.0), ys, np.full_like(ys, 0.013)], -1)
    v = np.tile([-np.cos(a), np.sin(a), 0.0], (ys.size, 1))
    old = im.trace_desc(dt, o, v)
    u = draws(d, ys.size, s1=0.99)  # only F > 0.99 reflects: total internal reflection
    new = rm.trace_desc(d, o, v, u.astype(np.float64))
    pick = np.nonzero((old["ends"] == "tir") & (old["margin"] > 1e-3) & (new["margin"] > 1e-3) & (old["n"] == 1))[0]
    assert pick.size > 0
    i = int(pick[pick.size // 2])
    so, no = _abi.insert_segments(dt, o[i:i + 1], v[i:i + 1], None, 8)
    sr, nr = _abi.reflect_segments(d, o[i:i + 1], v[i:i + 1], u[i:i + 1], 8)
    assert no[0] == 1 and old["n"][i] == 1          # today: the path ends inside the slab
    assert new["refl"][i] >= 1 and new["n"][i] >= 2  # reflected at least once, and out into the resin again
    assert nr[0] == new["n"][i]
    sub = {k: (x[i:i + 1] if isinstance(x, np.ndarray) else x) for k, x in new.items()}
    r = rm.compare_segments(sr, sub)
    assert r["compared"] >= 2 and r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D


# --------------------------------------------------------------------------- 2. the host walk against the model
def host_walk(m):
    return _abi.reflect_segments(m["desc"], m["o"], m["d"], m["u"], m["segs"].shape[1])


@pytest.mark.parametrize("name", list(rm.SCENES))
def test_host_walk_matches_model(meshdir, name):
    m = rm.model_of(meshdir, name)
    ok = m["margin"] > rm.MARGIN
    n = ok.size
    assert n % 256 != 0 and n == (2880 if m["spp"] == 1 else 8640)
    # what the scene has to hold (change the scene, not these)
    assert (~ok).mean() <= 0.01
    assert m["refl_seg"].sum() >= max(50, 0.02 * n)  # a sampled reflection followed by a medium segment
    assert (m["n"] >= 3).any()
    if "rr_depth" in rm.SCENES[name][3]:
        assert (m["ends"] == "rr").any()
    assert m["n"].max() <= m["segs"].shape[1]
    segs, nseg = host_walk(m)
    assert np.array_equal(nseg[ok], m["n"][ok])
    r = rm.compare_segments(segs, m)
    print(f"{name}: rays {n} reflected-then-deposited {int(m['refl_seg'].sum())} 3+ segments {int((m['n'] >= 3).sum())} "
          f"below margin {r['low']:.4f} compared {r['compared']} |do2| {r['e_o']:.3e} |dmaxt| {r['e_t']:.3e} "
          f"(tol {TOL_O:.3e}) |dd2| {r['e_d']:.3e} |dw|/w {r['e_w']:.3e} (tol {TOL_D:.3e}), each / kappa")
    assert r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D


# --------------------------------------------------------------------------- 3. anchor without reflections
@pytest.mark.parametrize("vial,inserts", [("cylindrical", ("prism", "u")), ("square", ("far",)),
                                          ("index_matched", ("box",))])
def test_equal_iors_give_the_transmission_only_segments_bit_for_bit(meshdir, vial, inserts):
    """Every IOR equal to the air's: eta = 1 at every interface, F = 0, no draw s1 > 0 reflects, and the sampled
    refraction is tvam_transmit_world's.  ('far' is met by no ray: the walk of a vial without inserts.)"""
    kw = dict(inserts=inserts, black=True, ior_glass=N_AIR, ior_medium=N_AIR, int_ior=1.7, ext_ior=1.7,
              max_depth=12, rr_depth=3, extinction=0.2)
    d = rm.reflect_scene(meshdir, vial, "lens", False, **kw)
    pix = pm.dense_pixels(d)
    rays = pm.model_rays(d, pix, np.arange(pix.size), 1, 7)
    u = im.path_draws(d, np.arange(pix.size), 1, 7).astype(np.float32)
    assert u[:, :, 1].min() > 0.0
    dt = d.copy()
    dt.transmission_only = 1
    want, nw = _abi.insert_segments(dt, rays["o"], rays["d"], u, 12)
    got, ng = _abi.reflect_segments(d, rays["o"], rays["d"], u, 12)
    assert nw.max() >= (1 if inserts == ("far",) else 2)
    assert np.array_equal(ng, nw) and np.array_equal(got, want)


# --------------------------------------------------------------------------- 4. the sampled branch's statistics
def test_binomial_share_of_paths_entering_the_resin(meshdir):
    """One ray, 20 000 draw sets of the sampler: it enters the resin when it refracts at the glass | resin face
    (surface 1), with probability 1 - F, and then deposits at the far face."""
    d = square_desc(meshdir)
    n = 20000
    u = im.path_draws(d, np.arange(n), 1, 11).astype(np.float32)
    o, v = np.repeat(CENTRE_O, n, 0), np.repeat(CENTRE_D, n, 0)
    _, nseg = _abi.reflect_segments(d, o, v, u, 2)
    one = rm.trace_desc(d, CENTRE_O.astype(np.float64), CENTRE_D.astype(np.float64), draws(d).astype(np.float64))
    assert one["n"][0] == 1
    F = normal_F(float(F32(rm.IOR_GLASS)), float(F32(rm.IOR_MEDIUM)))  # the model's reflectance there (5.1 %)
    entered = int((nseg >= 1).sum())
    print(f"entered {entered} of {n}, expected {n * (1 - F):.1f} +- {np.sqrt(n * F * (1 - F)):.1f}")
    assert abs(entered - n * (1.0 - F)) <= 5.0 * np.sqrt(n * F * (1.0 - F))


# --------------------------------------------------------------------------- 5. planted errors
def rejected(segs, model):
    """Whether the comparison refuses `segs` as the model's: segment counts or a bound."""
    try:
        r = rm.compare_segments(segs, model)
    except AssertionError:
        return True
    return not (r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D)


def test_checker_rejects_lt_in_place_of_le_at_s1_equal_F(meshdir):
    """An insert of eta = 3 met at normal incidence has F = ((1 - 3) / (1 + 3))^2 = 0.25 exactly, in float32
    and float64 alike (cos_i = 1, every intermediate a dyadic number): s1 = 0.25 reflects under <= and refracts
    under <.  The ray's margin is 0 by construction, so the comparison takes it regardless."""
    slab = im.box_tris((-1.0, -0.5, -0.5), (1.0, 0.5, 0.5)).astype(np.float32)
    d = rm.reflect_scene(meshdir, "index_matched", "collimated", True, inserts=("box",))
    d.set_inserts([(slab, 3.0, 1.0)])
    o = np.array([[20.0, 0.125, 0.0625]], np.float32)
    u = draws(d)
    u[0, 1, 1] = 0.25  # surface 0 is the tube (null BSDF), surface 1 the slab's +x face
    segs, nseg = _abi.reflect_segments(d, o, CENTRE_D, u, 8)
    good = rm.trace_desc(d, o, CENTRE_D, u)
    bad = rm.trace_desc(d, o, CENTRE_D, u, flaw="lt")
    assert good["margin"][0] == 0.0 and good["refl"][0] == 1 and bad["refl"][0] == 0
    for m in (good, bad):
        m["margin"] = np.full(1, np.inf)
    assert nseg[0] == 2 and segs[0, 1, 4] == 1.0  # reflected: the second segment runs back along +x
    assert not rejected(segs, good)
    assert rejected(segs, bad)


@pytest.mark.parametrize("flaw", ["keepT", "spawn"])
def test_checker_rejects_planted_errors(meshdir, flaw):
    """(1 - F) kept on the refracted branch; the reflected ray's spawn offset on the wrong side."""
    m = rm.model_of(meshdir, "square-collimated-u-black")
    segs, _ = host_walk(m)
    assert not rejected(segs, m)
    bad = rm.trace_desc(m["desc"], m["o"], m["d"], m["u"], flaw=flaw)
    assert rejected(segs, bad)


# --------------------------------------------------------------------------- 6. refusals
def _create(d, inserts, entry="tvam_plan_create_reflect"):
    lib = _abi.load_library()
    plan = ctypes.c_void_p()
    arr = _abi.insert_array(inserts)
    rc = getattr(lib, entry)(ctypes.byref(d), arr, len(inserts), 0, ctypes.byref(plan))
    assert not plan.value  # no plan was created
    return rc, lib.tvam_last_error().decode()


def test_refusals_name_the_cause_and_make_no_plan(meshdir):
    """Every refusal comes from validation, before any HIP call: it holds on a machine without a GPU."""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    o = np.array([[20.0, 0.1, 0.0]], np.float32)

    def base(vial="cylindrical", kind="telecentric", inserts=("box",)):
        return rm.reflect_scene(meshdir, vial, kind, False, inserts=inserts)

    def unsupported(d, what):
        rc, msg = _create(d, d.inserts)
        assert rc == _abi.TVAM_ERR_UNSUPPORTED and msg.startswith("transmission_only = 0 with " + what), msg
        with pytest.raises(ValueError, match=re.escape("transmission_only = 0 with " + what)):  # the host walk too
            _abi.reflect_segments(d, o, CENTRE_D, draws(d), 4)

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
    d.vial_type = _abi.VIAL_CUSTOM
    unsupported(d, "a 'custom' vial")
    d = base()
    d.vial_type = _abi.VIAL_DOUBLE_CYLINDRICAL
    unsupported(d, "a 'double_cylindrical' vial")
    # transmission_only = 1 belongs to the other entries
    d = base()
    d.transmission_only = 1
    rc, msg = _create(d, d.inserts)
    assert rc == _abi.TVAM_ERR_INVALID and "transmission_only = 1 belongs to tvam_plan_create and its siblings" in msg
    # an index-matched vial needs an insert; a glass vial does not (the host walk runs)
    d = base("index_matched", inserts=())
    rc, msg = _create(d, [])
    assert rc == _abi.TVAM_ERR_INVALID and "'index_matched' vial without inserts" in msg
    d = base("square", inserts=())
    assert not d.inserts and d.reflected
    _, nseg = _abi.reflect_segments(d, o, CENTRE_D, draws(d), 4)
    assert nseg[0] == 1
    # the inserts' own validation is tvam_plan_create_inserts'
    d = base()
    bad = im.mesh("box").copy()
    bad[3, 0] = [2.9, 0.0, 0.0]
    rc, msg = _create(d, [(bad, 1.5, 1.4)])
    assert rc == _abi.TVAM_ERR_INVALID and "insert 0: triangle 3 vertex 0 lies outside the resin" in msg
    rc, msg = _create(d, [(im.mesh("box"), 0.0, 1.4)])
    assert rc == _abi.TVAM_ERR_INVALID and "insert 0: int_ior and ext_ior must be positive" in msg
    # u is required
    lib = _abi.load_library()
    segs, nseg = np.zeros((1, 4, 8), np.float32), np.zeros(1, np.int32)
    d = base()
    rc = lib.tvam_reflect_segments(ctypes.byref(d), _abi.insert_array(d.inserts), 1, o.ctypes.data, CENTRE_D.ctypes.data, 1,
                                   None, 4, segs.ctypes.data, nseg.ctypes.data)
    assert rc == _abi.TVAM_ERR_INVALID and "u is required" in lib.tvam_last_error().decode()
    with pytest.raises(ValueError, match="u is required"):
        _abi.reflect_segments(d, o, CENTRE_D, None, 4)
    # the old entries' refusals are unchanged
    rc, msg = _create(d, d.inserts, "tvam_plan_create_inserts")
    assert rc == _abi.TVAM_ERR_UNSUPPORTED and msg.startswith("dielectric occluders with transmission_only = 0")
    dt = d.copy()
    dt.transmission_only = 1
    rc, msg = _create(dt, [], "tvam_plan_create_inserts")
    assert rc == _abi.TVAM_ERR_INVALID and "no insert given" in msg
    plan = ctypes.c_void_p()
    dc = base("cylindrical", "collimated", inserts=())
    rc = lib.tvam_plan_create(ctypes.byref(dc), 0, ctypes.byref(plan))
    assert rc == _abi.TVAM_ERR_UNSUPPORTED and not plan.value
    assert "transmission_only = 0 behind a 'cylindrical' vial" in lib.tvam_last_error().decode()
    rc = lib.tvam_plan_create_traced(ctypes.byref(dc), 0, ctypes.byref(plan))
    assert rc == _abi.TVAM_ERR_UNSUPPORTED and not plan.value and "transmission_only = 0" in lib.tvam_last_error().decode()


def test_descriptor_names_the_reflecting_scenes(meshdir):
    """TvamDesc.reflected: what engine.Projection sends to tvam_plan_create_reflect."""
    assert rm.reflect_scene(meshdir, "cylindrical", "collimated", True).reflected       # collimated configs too
    assert rm.reflect_scene(meshdir, "index_matched", "lens", False, inserts=("u",)).reflected
    assert not rm.reflect_scene(meshdir, "index_matched", "collimated", True).reflected  # no dielectric interface
    assert not rm.reflect_scene(meshdir, "square", "lens", False, transmission_only=True).reflected

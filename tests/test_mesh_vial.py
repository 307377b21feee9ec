"""The 'custom' vial without a GPU: the float64 model of tests/mesh_vial_model.py anchored to the
oracle's square vial, the host bounding volume hierarchy against the brute-force loop
(tvam_mesh_hit: the kernels' own traversal, compiled for the host), the C entry points' refusals,
CustomVial.fill_desc, and the margin cap the GPU tests of tests/test_gpu_mesh_vial.py rely on."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from drtvam_amd import _abi
from drtvam_amd.configs import BOX_HOLE_CUSTOM_CUVETTE, desc_from_config, square_vial

import mesh_vial_model as mv
import projector_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# --------------------------------------------------------------------------- the model and the oracle
@pytest.mark.parametrize("regular", [True, False], ids=["regular", "jittered"])
def test_model_reproduces_oracle_square_vial(oracle, regular):
    """Closed box meshes of a SquareVial's cuboids: the tracer, fed with the oracle's own (o, d),
    gives the oracle's hit, o2, d2, maxt and weight -- 64 ulp of the distance for points, 64 ulp of
    1 for directions and (relatively) the weight -- on every ray whose margin exceeds 1e-4."""
    spp = 1 if regular else 2
    cfg = square_vial(N=24, angles=12, regular_sampling=regular, spp=spp)
    d = desc_from_config(cfg)
    outer, inner = mv.square_vial_meshes(cfg["vial"]["w_int"], cfg["vial"]["w_ext"], float(d.vial_height))
    pix = pm.dense_pixels(d)
    rays = [oracle.ray(d, int(pix[i // spp]), i, 5) for i in range(pix.size * spp)]
    o = np.array([r["o"] for r in rays], np.float64)
    dd = np.array([r["d"] for r in rays], np.float64)
    e_ext = float(np.float32(d.vial_ior) / np.float32(mv.IOR_AIR))
    e_int = float(np.float32(d.medium_ior) / np.float32(d.vial_ior))
    m = mv.trace(o, dd, outer, inner, e_ext, e_int, d.max_depth)
    ok = m["margin"] > mv.MARGIN
    hit = np.array([r["hit"] for r in rays])
    assert ok.mean() > 0.95 and 0 < hit[ok].sum()
    assert np.array_equal(hit[ok], m["hit"][ok])
    sel = ok & hit
    tol_o = 64 * float(np.spacing(np.float32(d.distance)))
    tol_d = 64 * float(np.spacing(np.float32(1.0)))
    e_o = np.abs(np.array([r["o2"] for r in rays], np.float64)[sel] - m["o2"][sel]).max()
    e_t = np.abs(np.array([r["maxt"] for r in rays])[sel] - m["maxt"][sel]).max()
    e_d = np.abs(np.array([r["d2"] for r in rays], np.float64)[sel] - m["d2"][sel]).max()
    e_w = np.abs(np.array([r["weight"] for r in rays])[sel] / m["weight"][sel] - 1.0).max()
    print(f"rays {len(rays)} compared {int(sel.sum())}: |do2| {e_o:.3e} |dmaxt| {e_t:.3e} (tol {tol_o:.3e}) "
          f"|dd2| {e_d:.3e} |dw|/w {e_w:.3e} (tol {tol_d:.3e})")
    assert e_o <= tol_o and e_t <= tol_o and e_d <= tol_d and e_w <= tol_d
    assert np.abs(m["d2"][sel] - dd[sel]).max() > 1e-2  # refracted at all


def test_mesh_builders_are_wound_outwards():
    for outer, inner in (mv.cuvette(), mv.scene_meshes("prism"), mv.scene_meshes("tube"),
                         mv.square_vial_meshes(7.0, 8.0, 20.0)):
        for t in (outer, inner):
            t = np.asarray(t, np.float64)
            n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
            c = t.mean(1)
            assert (np.linalg.norm(n, axis=1) > 0).all()
            side = np.abs(n[:, 2]) < 0.9 * np.linalg.norm(n, axis=1)
            assert (np.sum(n[side, :2] * c[side, :2], -1) > 0).all()
            assert (n[~side, 2] * c[~side, 2] > 0).all()
    assert mv.scene_meshes("tube")[0].shape == (2048, 3, 3) and mv.cuvette()[0].shape == (8, 3, 3)


# --------------------------------------------------------------------------- the hierarchy
def _test_rays(tris, n=10000, seed=0):
    """Random rays around the mesh: towards it from outside, from inside it, axis-parallel ones
    (exact zeros in d) and ones aimed past it."""
    rng = np.random.default_rng(seed)
    ext = float(np.abs(tris).max())
    o = rng.uniform(-2.0 * ext, 2.0 * ext, (n, 3))
    o[: n // 4] *= 0.2  # from inside
    tgt = rng.uniform(-ext, ext, (n, 3))
    tgt[n // 2: n // 2 + n // 8] *= 4.0  # mostly misses
    d = tgt - o
    ax = np.arange(n - n // 5, n)  # axis-parallel: one component +-1
    d[ax] = 0.0
    d[ax, rng.integers(0, 3, ax.size)] = rng.choice([-1.0, 1.0], ax.size)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("name", ["tube", "prism", "cuvette"])
def test_bvh_equals_brute_force_on_the_host(name):
    outer, inner = mv.scene_meshes(name)
    for tris in (outer, np.concatenate([inner, outer])):
        o, d = _test_rays(tris, seed=len(tris))
        t1, i1 = _abi.mesh_hit(tris, o, d, use_bvh=True)
        t0, i0 = _abi.mesh_hit(tris, o, d, use_bvh=False)
        hits = np.isfinite(t0)
        print(f"{name} {len(tris)} triangles: {hits.mean():.3f} of {len(o)} rays hit")
        assert 0.2 < hits.mean() < 0.98
        assert np.array_equal(t1.view(np.uint32), t0.view(np.uint32)) and np.array_equal(i1, i0)
        assert np.all(i0[~hits] == -1) and np.all((i0[hits] >= 0) & (i0[hits] < len(tris)))
        assert np.all(t0[hits] >= 0.0)
        # and the hits are the model's, wherever its decisions are clear
        tm, im, gap, edge = mv._closest(np.asarray(tris, np.float64), o.astype(np.float64), d.astype(np.float64))
        ok = (edge > mv.MARGIN) & (gap > mv.MARGIN)
        assert ok.mean() > 0.9
        assert np.array_equal(hits[ok], np.isfinite(tm[ok])) and np.array_equal(i0[ok & hits], im[ok & hits])
        # t = (e2 . q) / det with det = |e1 x e2| (n . d): the fp32 rounding of the products (64 ulp of
        # the scene's extent, origins included) is divided by the cosine of incidence
        sel = ok & hits
        t64 = np.asarray(tris, np.float64)[im[sel]]
        nrm = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
        cos = np.abs(np.sum(nrm * d[sel], -1)) / np.linalg.norm(nrm, axis=1)
        tol = 64 * float(np.spacing(np.float32(4.0 * np.abs(tris).max()))) / cos
        worst = float((np.abs(t0[sel] - tm[sel]) / tol).max())
        print(f"  |dt| / tol: {worst:.3f}")
        assert worst <= 1.0


def test_mesh_hit_refuses_bad_meshes():
    o = np.zeros((1, 3), np.float32)
    d = np.array([[1.0, 0.0, 0.0]], np.float32)
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], np.float32)
    t, i = _abi.mesh_hit(tri, o, d)
    assert t[0] == 1.0 and i[0] == 0
    with pytest.raises(ValueError, match="null or empty"):
        _abi.mesh_hit(np.zeros((0, 3, 3), np.float32), o, d)
    bad = tri.copy()
    bad[0, 2] = bad[0, 0]
    with pytest.raises(ValueError, match="triangle 0 has zero area"):
        _abi.mesh_hit(bad, o, d)
    bad = tri.copy()
    bad[0, 1, 2] = np.nan
    with pytest.raises(ValueError, match="triangle 0 has a non-finite vertex"):
        _abi.mesh_hit(bad, o, d)


# --------------------------------------------------------------------------- the C ABI
def _create_mesh(d, outer, inner):
    lib = _abi.load_library()
    plan = ctypes.c_void_p()
    rc = lib.tvam_plan_create_mesh(ctypes.byref(d), None if outer is None else outer.ctypes.data,
                                   0 if outer is None else len(outer), None if inner is None else inner.ctypes.data,
                                   0 if inner is None else len(inner), 0, ctypes.byref(plan))
    assert not plan.value  # no plan was created
    return rc, lib.tvam_last_error().decode()


def test_header_and_loader():
    hdr = open(os.path.join(ROOT, "include", "tvam.h")).read()
    assert re.search(r"#define\s+TVAM_VIAL_CUSTOM\s+3\b", hdr)
    assert re.search(r"#define\s+TVAM_ABI_VERSION\s+13\b", hdr)
    assert "tvam_plan_create_mesh" in hdr and "tvam_mesh_hit" in hdr
    assert _abi.VIAL_CUSTOM == 3 and _abi.ABI_VERSION == 13
    assert {"tvam_plan_create_mesh", "tvam_mesh_hit"} <= set(_abi.EXPORTS)
    lib = _abi.load_library()
    assert lib.tvam_plan_create_mesh.restype is ctypes.c_int and lib.tvam_mesh_hit.restype is ctypes.c_int


def test_refusals_name_the_combination():
    """Every refusal comes from validation, before any HIP call: it holds on a machine without a GPU."""
    outer, inner = (np.ascontiguousarray(t) for t in mv.cuvette())
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    lib = _abi.load_library()

    def base():
        return mv.custom_scene("telecentric", "cuvette")

    # tvam_plan_create names the entry that takes the meshes
    plan = ctypes.c_void_p()
    d = base()
    assert lib.tvam_plan_create(ctypes.byref(d), 0, ctypes.byref(plan)) == _abi.TVAM_ERR_INVALID
    assert "tvam_plan_create_mesh" in lib.tvam_last_error().decode() and not plan.value

    def unsupported(d, what):
        rc, msg = _create_mesh(d, outer, inner)
        assert rc == _abi.TVAM_ERR_UNSUPPORTED and msg.startswith("a 'custom' vial with " + what), msg

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
    d.rr_depth = 1
    unsupported(d, "rr_depth < 2")

    def invalid(o, i, what):
        rc, msg = _create_mesh(base(), o, i)
        assert rc == _abi.TVAM_ERR_INVALID and what in msg, msg

    invalid(None, inner, "the outer vial mesh is null or empty")
    invalid(outer, None, "the inner vial mesh is null or empty")
    bad = inner.copy()
    bad[5, 0, 1] = np.inf
    invalid(outer, bad, "the inner vial mesh: triangle 5 has a non-finite vertex")
    bad = outer.copy()
    bad[3, 1] = bad[3, 0]
    invalid(bad, inner, "the outer vial mesh: triangle 3 has zero area")
    # the radius check does not reject the type (vial_r = vial_r_ext = vial_height = 0 above), and
    # the other vial types cannot take the entry
    d = pm.projector_scene("collimated")
    rc, msg = _create_mesh(d, outer, inner)
    assert rc == _abi.TVAM_ERR_INVALID and "TVAM_VIAL_CUSTOM" in msg


# --------------------------------------------------------------------------- Python
def _cuvette_config():
    cfg = copy.deepcopy(BOX_HOLE_CUSTOM_CUVETTE)
    cfg["vial"]["filename_vial_outer"] = os.path.join(GOLDEN, "cuvette_outer.ply")
    cfg["vial"]["filename_vial_inner"] = os.path.join(GOLDEN, "cuvette_inner.ply")
    return cfg


def test_custom_vial_fills_the_descriptor():
    cfg = _cuvette_config()
    d = desc_from_config(cfg)
    assert d.vial_type == _abi.VIAL_CUSTOM and d.projector_type == _abi.PROJECTOR_TELECENTRIC
    assert d.vial_ior == np.float32(1.4702) and d.medium_ior == np.float32(1.33)
    assert d.sigma_t == np.float32(0.06) and d.albedo == 0.0 and d.n_occluder_tris == 0
    outer, inner = mv.cuvette()
    assert np.array_equal(d._vial_outer, outer) and np.array_equal(d._vial_inner, inner)
    assert d._vial_outer.dtype == np.float32 and d._vial_outer.flags["C_CONTIGUOUS"]
    c = d.copy()
    assert c._vial_outer is d._vial_outer and c._vial_inner is d._vial_inner and c.vial_type == _abi.VIAL_CUSTOM
    assert (tuple(d.film_res), d.n_patterns, d.res_x, d.res_y) == ((100, 100, 50), 200, 200, 20)


def test_custom_vial_dict_and_scene_round_trip():
    from drtvam_amd.geometry import CustomVial
    from drtvam_amd.scene import _container_from_shapes
    cfg = _cuvette_config()
    v = CustomVial(cfg["vial"])
    sd = v.to_dict()
    for key, ior in (("vial_exterior", {"int_ior": 1.4702, "ext_ior": "air"}),
                     ("vial_interior", {"ext_ior": 1.4702, "int_ior": 1.33})):
        assert sd[key]["type"] == "ply" and sd[key]["face_normals"] is True
        assert sd[key]["bsdf"] == {"type": "dielectric", **ior}
    assert sd["vial_interior"]["interior"] == {"type": "ref", "id": "printing_medium"}
    back = _container_from_shapes(sd)
    assert isinstance(back, CustomVial)
    assert back.filename_vial_outer == v.filename_vial_outer and back.filename_vial_inner == v.filename_vial_inner
    assert back.vial_ior == 1.4702 and back.medium_ior == 1.33 and back.sigma_t == 0.06
    occ = copy.deepcopy(cfg["vial"])
    occ["occlusions"] = [{"filename": os.path.join(GOLDEN, "occlusion.ply")}]
    with pytest.raises(NotImplementedError, match="a 'custom' vial with occluders"):
        CustomVial(occ).fill_desc(_abi.default_desc())


# --------------------------------------------------------------------------- the GPU tests' cap
@pytest.mark.parametrize("mesh", ["cuvette", "prism", "tube"])
@pytest.mark.parametrize("kind", ["collimated", "telecentric", "lens"])
def test_gpu_scenes_keep_their_rays_clear_of_decisions(kind, mesh):
    """At most 1 % of a GPU scene's rays lie within 1e-4 of a discrete decision (an edge, a second
    surface, total internal reflection): the cap tests/test_gpu_mesh_vial.py relies on."""
    m = mv.scene_model(kind, mesh, 2, 3)
    low = float((m["margin"] <= mv.MARGIN).mean())
    print(f"{kind} {mesh}: {low:.4f} of {m['margin'].size} rays below the margin, {m['hit'].mean():.3f} deposit")
    assert low <= 0.01
    assert m["hit"].mean() > 0.5

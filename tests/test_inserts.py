"""Dielectric occluders at the C ABI and in the Python layer, without a GPU: the new entries are
exported and the ABI is unchanged, every validation and refusal message of
tvam_plan_create_inserts comes before any device call, and the documented config builds the inserts
beside the descriptor."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config
from drtvam_amd.geometry import IOR_TABLE, geometries
from drtvam_amd.optimize import load_scene
from drtvam_amd.scene import load_dict

import insert_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvam.h")
NAMES = {"tvam_plan_create_inserts", "tvam_insert_segments", "tvam_plan_insert_segments"}


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("insert_meshes")
    im.write_meshes(d)
    return d


# --------------------------------------------------------------------------- the C ABI
def test_header_and_loader():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+TVAM_ABI_VERSION\s+13\b", hdr) and _abi.ABI_VERSION == 13
    assert all(n in hdr for n in NAMES) and "typedef struct tvam_insert" in hdr
    assert NAMES <= set(_abi.EXPORTS)
    lib = _abi.load_library()
    assert lib.tvam_abi_version() == 13 and all(hasattr(lib, n) for n in NAMES)
    assert ctypes.sizeof(_abi.TvamInsert) == 24 and _abi.TvamInsert.n_tris.offset == 8


def test_insert_layout_matches_header(tmp_path):
    """The ctypes mirror has the C struct's size and field offsets (compiled with gcc, as tests/test_capi.py
    compiles tvam_desc)."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tvam.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(tvam_insert), offsetof(tvam_insert, tris), '
                   'offsetof(tvam_insert, n_tris), offsetof(tvam_insert, int_ior), offsetof(tvam_insert, ext_ior));\n'
                   'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _abi.TvamInsert
    assert vals == [ctypes.sizeof(T), T.tris.offset, T.n_tris.offset, T.int_ior.offset, T.ext_ior.offset]


def _create(d, inserts):
    lib = _abi.load_library()
    plan = ctypes.c_void_p()
    arr = _abi.insert_array(inserts)
    rc = lib.tvam_plan_create_inserts(ctypes.byref(d), arr, len(inserts), 0, ctypes.byref(plan))
    assert not plan.value  # no plan was created
    return rc, lib.tvam_last_error().decode()


def test_refusals_and_validation_name_the_cause(meshdir):
    """Every refusal comes from validation, before any HIP call: it holds on a machine without a GPU."""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    box = im.mesh("box")

    def base(vial="cylindrical", kind="telecentric"):
        return im.insert_scene(meshdir, vial, kind, False, inserts=("box",))

    def unsupported(d, what):
        rc, msg = _create(d, d.inserts)
        assert rc == _abi.TVAM_ERR_UNSUPPORTED and msg.startswith("dielectric occluders with " + what), msg

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
    d.vial_type = _abi.VIAL_CUSTOM
    unsupported(d, "a 'custom' vial")
    d = base()
    d.vial_type = _abi.VIAL_DOUBLE_CYLINDRICAL
    unsupported(d, "a 'double_cylindrical' vial")

    def invalid(inserts, what, d=None):
        rc, msg = _create(base() if d is None else d, inserts)
        assert rc == _abi.TVAM_ERR_INVALID and what in msg, msg

    good = (box, 1.58, 1.4849)
    invalid([], "no insert given")
    invalid([good, (np.zeros((0, 3, 3), np.float32), 1.5, 1.4)], "insert 1: the mesh is null or empty")
    bad = box.copy()
    bad[5, 2, 1] = np.nan
    invalid([good, (bad, 1.5, 1.4)], "insert 1: triangle 5 vertex 2 is not finite")
    bad = box.copy()
    bad[7, 1] = bad[7, 0]
    invalid([(bad, 1.5, 1.4)], "insert 0: triangle 7 has zero area")
    invalid([(box, 0.0, 1.4)], "insert 0: int_ior and ext_ior must be positive")
    invalid([good, (box, 1.5, -1.0)], "insert 1: int_ior and ext_ior must be positive")
    bad = box.copy()
    bad[3, 0] = [2.9, 0.0, 0.0]  # radius >= vial_r
    invalid([(bad, 1.5, 1.4)], "insert 0: triangle 3 vertex 0 lies outside the resin")
    bad = box.copy()
    bad[4, 1] = [0.0, 0.0, 2.01]  # |z| > half height
    invalid([(bad, 1.5, 1.4)], "insert 0: triangle 4 vertex 1 lies outside the resin")
    bad = box.copy()
    bad[2, 2] = [0.0, 0.0, 1.9]  # square: the inner cuboid is 0.9 of the height (1.8)
    invalid([(bad, 1.5, 1.4)], "insert 0: triangle 2 vertex 2 lies outside the resin", base("square"))
    d = base("cylindrical")  # (the same vertex lies inside the tube's resin: half height 2)
    d.set_inserts([(bad, 1.5, 1.4)])
    _abi.insert_segments(d, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), None, 4)
    d = base()
    d.focus_distance = 0.0
    invalid(d.inserts, "focus_distance must be positive", d)
    # Russian roulette is honoured: no refusal on rr_depth (the host walk runs, with and without draws)
    d = base()
    d.rr_depth, d.max_depth = 0, 16
    o = np.array([[20.0, 0.1, 0.0]], np.float32)
    v = np.array([[-1.0, 0.0, 0.0]], np.float32)
    segs, nseg = _abi.insert_segments(d, o, v, None, 4)
    assert nseg[0] == 2
    # the host walk refuses what the plan entry refuses
    d = base()
    d.albedo = 0.5
    with pytest.raises(ValueError, match="dielectric occluders with a scattering medium"):
        _abi.insert_segments(d, o, v, None, 4)
    d = base()
    d.set_inserts([(box, 0.0, 1.0)])
    with pytest.raises(ValueError, match="insert 0: int_ior and ext_ior must be positive"):
        _abi.insert_segments(d, o, v, None, 4)
    # the other plan entries know nothing of inserts, and the black occluders next to them stay legal
    d = im.insert_scene(meshdir, "square", "collimated", True, inserts=("box",), black=True)
    assert d.n_occluder_tris == 12 and len(d.inserts) == 1
    segs, nseg = _abi.insert_segments(d, o, v, None, 4)
    assert nseg[0] == 2


# --------------------------------------------------------------------------- Python
def documented_config(meshdir, **bsdf):
    """container.rst, "Occlusions": a transparent plastic piece and a fully absorptive one."""
    paths = im.write_meshes(meshdir)
    cfg = im.insert_config("cylindrical", "collimated", True, inserts=(), paths=paths)
    cfg["vial"]["occlusions"] = [
        {"filename": paths["box"], "bsdf": {"type": "dielectric", "int_ior": 1.58, "ext_ior": 1.4849} | bsdf},
        {"filename": paths["black"]},
    ]
    return json.loads(json.dumps(cfg))


def test_documented_config_builds_the_inserts(meshdir):
    d = desc_from_config(documented_config(meshdir))
    assert d.n_occluder_tris == 12 and np.array_equal(d._occluders, im.mesh("black"))
    (t, ni, ne), = d.inserts
    assert np.array_equal(t, im.mesh("box")) and (ni, ne) == (1.58, 1.4849)
    assert d.copy().inserts[0][0] is t  # the arrays go with a copy
    # Mitsuba's defaults and names
    cfg = documented_config(meshdir)
    cfg["vial"]["occlusions"][0]["bsdf"] = {"type": "dielectric"}
    (_, ni, ne), = desc_from_config(cfg).inserts
    assert (ni, ne) == (IOR_TABLE["bk7"], IOR_TABLE["air"])
    cfg["vial"]["occlusions"][0]["bsdf"] = {"type": "dielectric", "int_ior": "diamond", "ext_ior": "water"}
    (_, ni, ne), = desc_from_config(cfg).inserts
    assert (ni, ne) == (IOR_TABLE["diamond"], IOR_TABLE["water"])
    # an explicit black diffuse BSDF is a black occluder, as before
    cfg["vial"]["occlusions"][0]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "spectrum", "value": 0.0}}
    d = desc_from_config(cfg)
    assert not d.inserts and d.n_occluder_tris == 24


def test_other_bsdfs_are_refused_by_name(meshdir):
    cfg = documented_config(meshdir)
    cfg["vial"]["occlusions"][0]["bsdf"] = {"type": "roughdielectric", "alpha": 0.1}
    with pytest.raises(NotImplementedError, match="'roughdielectric'"):
        desc_from_config(cfg)
    cfg["vial"]["occlusions"][0]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "spectrum", "value": 0.5}}
    with pytest.raises(NotImplementedError, match="'diffuse'.*black"):
        desc_from_config(cfg)
    cfg = documented_config(meshdir)
    cfg["vial"]["occlusions"][0]["face_normals"] = False
    with pytest.raises(NotImplementedError, match="face_normals: false"):
        desc_from_config(cfg)
    for vial in ("custom", "double_cylindrical"):
        assert vial in geometries  # (their own refusal of occluders stands: tests/test_mesh_vial.py, test_double_vial.py)


def test_to_dict_and_load_dict_carry_the_bsdf(meshdir):
    cfg = documented_config(meshdir)
    sd = load_scene(cfg)
    occ = {k: v for k, v in sd.items() if k.startswith("occlusion")}
    assert len(occ) == 2
    diel = [v for v in occ.values() if v["bsdf"]["type"] == "dielectric"]
    assert len(diel) == 1 and diel[0]["bsdf"] == {"type": "dielectric", "int_ior": 1.58, "ext_ior": 1.4849}
    assert all(v["type"] == "ply" and v["face_normals"] is True and v["exterior"] == {"type": "ref", "id": "printing_medium"}
               for v in occ.values())
    black = [v for v in occ.values() if v["bsdf"]["type"] == "diffuse"]
    assert black[0]["bsdf"]["reflectance"]["value"] == 0.0
    # a scene dictionary without the container object: load_dict rebuilds it from the shapes, occlusions included
    plain = {k: v for k, v in sd.items() if k != "_container"}
    scene = load_dict(plain)
    got = scene.container.occlusions
    assert [o["filename"] for o in got] == [o["filename"] for o in cfg["vial"]["occlusions"]]
    assert got[0]["bsdf"] == cfg["vial"]["occlusions"][0]["bsdf"]
    from drtvam_amd.integrators import VolumeIntegrator
    d = VolumeIntegrator({"regular_sampling": True}).desc(scene, scene.sensor_by_id("sensor"))
    assert len(d.inserts) == 1 and d.n_occluder_tris == 12 and d.vial_type == _abi.VIAL_CYLINDRICAL

"""Telecentric / lens projectors without a GPU: the plugin classes (props, error strings, fill_desc,
fov <-> pixel_size), the ABI additions of version 13, and the float64 ray model the GPU tests
compare the kernels with (tests/projector_model.py), checked here against known answers and,
for the collimated projector, against the oracle's ray."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from drtvam_amd import _abi
from drtvam_amd.projector import LensProjector, TelecentricProjector, emitters

import projector_model as pm

BASE = {"n_patterns": 6, "resx": 24, "resy": 20, "motion": "circular", "distance": 20.0, "device": "cpu"}


def test_emitters_registered():
    assert emitters["telecentric"] is TelecentricProjector and emitters["lens"] is LensProjector


def test_telecentric_props_and_desc():
    p = TelecentricProjector(BASE | {"pixel_size": 0.15, "aperture_radius": 2.0, "focus_distance": 18.0})
    assert p.pixel_size == (0.15, 0.15) and p.emitter_size == (24 * 0.15, 20 * 0.15)
    assert p.to_string() == "TelecentricProjector"
    d = _abi.TvamDesc()
    p.fill_desc(d)
    assert d.projector_type == _abi.PROJECTOR_TELECENTRIC == 1
    assert (d.n_patterns, d.res_x, d.res_y, d.crop_x, d.crop_y) == (6, 24, 20, 24, 20)
    assert d.pixel_size_x == d.pixel_size_y == np.float32(0.15)
    assert d.aperture_radius == np.float32(2.0) and d.focus_distance == np.float32(18.0)
    assert d.distance == 20.0 and d.clockwise == 0
    p2 = TelecentricProjector(BASE | {"pixel_size": (0.1, 0.2), "aperture_radius": 0.0, "focus_distance": 1.0})
    p2.fill_desc(d)
    assert (d.pixel_size_x, d.pixel_size_y) == (np.float32(0.1), np.float32(0.2))


def test_telecentric_props_errors():
    with pytest.raises(ValueError, match="pixel_size must be a float or a Point2f"):
        TelecentricProjector(BASE | {"pixel_size": "wide", "aperture_radius": 1.0, "focus_distance": 1.0})
    for missing in ("pixel_size", "aperture_radius", "focus_distance"):
        props = BASE | {"pixel_size": 0.1, "aperture_radius": 1.0, "focus_distance": 1.0}
        del props[missing]
        with pytest.raises(KeyError, match=missing):
            TelecentricProjector(props)
    with pytest.raises(ValueError, match="Missing field 'motion'"):
        TelecentricProjector({k: v for k, v in BASE.items() if k != "motion"} |
                             {"pixel_size": 0.1, "aperture_radius": 1.0, "focus_distance": 1.0})


def test_lens_props_errors():
    lens = {"aperture_radius": 1.0, "focus_distance": 20.0}
    with pytest.raises(AssertionError, match="Specify either 'fov' or 'pixel_size', not both."):
        LensProjector(BASE | lens | {"fov": 10.0, "pixel_size": 0.1})
    with pytest.raises(AssertionError, match="Either 'fov' or 'pixel_size' must be specified."):
        LensProjector(BASE | lens)
    with pytest.raises(KeyError, match="focus_distance"):
        LensProjector(BASE | {"aperture_radius": 1.0, "pixel_size": 0.1})


def test_lens_fov_pixel_size_consistency():
    lens = {"aperture_radius": 0.5, "focus_distance": 20.0}
    a = LensProjector(BASE | lens | {"pixel_size": 0.15})
    # pixel_size * N_x = tan(fov / 2) * 2 * focus_distance (projector.py:254-262)
    assert a.fov == pytest.approx(np.rad2deg(2 * np.arctan(0.15 * 24 / 2 / 20.0)), rel=1e-14)
    b = LensProjector(BASE | lens | {"fov": a.fov})
    assert b.pixel_size == pytest.approx(0.15, rel=1e-13)
    assert b.pixel_size == np.tan(np.deg2rad(a.fov) / 2) * 2 * 20.0 / 24  # host double
    # image rectangle on the plane z = 1
    assert a.area == pytest.approx((24 * 0.15 / 20.0) * (20 * 0.15 / 20.0), rel=1e-12)
    da, db = _abi.TvamDesc(), _abi.TvamDesc()
    a.fill_desc(da)
    b.fill_desc(db)
    assert da.projector_type == db.projector_type == _abi.PROJECTOR_LENS == 2
    assert da.pixel_size_x == da.pixel_size_y == db.pixel_size_x == db.pixel_size_y == np.float32(0.15)
    assert da.aperture_radius == np.float32(0.5) and da.focus_distance == 20.0
    assert a.to_string().startswith("LensProjector[\n    fov = ") and "aperture radius = 0.5" in a.to_string()


def test_desc_from_config_all_kinds():
    for kind, t in (("collimated", 0), ("telecentric", 1), ("lens", 2)):
        d = pm.projector_scene(kind)
        assert d.projector_type == t and d.abi_version == _abi.ABI_VERSION == 13
        assert tuple(d.film_res) == (40, 36, 20)
    d = pm.projector_scene("lens", lens_fov=True)
    assert d.pixel_size_x == np.float32(0.15)


def test_abi_symbols_and_flags():
    assert _abi.FLAG_BIN_FIRST == 32 and _abi.FLAG_SCATTER_ATOMIC == 16
    assert "tvam_plan_rays" in _abi.EXPORTS
    names = [n for n, _ in _abi.TvamDesc._fields_]
    assert names[-2:] == ["aperture_radius", "focus_distance"]
    lib = _abi.load_library()  # binds every entry of EXPORTS or raises
    assert lib.tvam_abi_version() == 13
    assert hasattr(lib, "tvam_plan_rays")
    hdr = open(os.path.join(ROOT, "include", "tvam.h")).read()
    for tok in ("#define TVAM_ABI_VERSION 13", "#define TVAM_PROJECTOR_TELECENTRIC 1", "#define TVAM_PROJECTOR_LENS        2",
                "#define TVAM_FLAG_BIN_FIRST    32", "int tvam_plan_rays("):
        assert tok in hdr, tok


def test_desc_size_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tvam.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(tvam_desc), offsetof(tvam_desc, aperture_radius), '
                   'offsetof(tvam_desc, focus_distance)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(_abi.TvamDesc) == vals[0]
    assert _abi.TvamDesc.aperture_radius.offset == vals[1] and _abi.TvamDesc.focus_distance.offset == vals[2]


def test_desc_init_defaults():
    d = _abi.default_desc()
    assert d.projector_type == 0 and d.aperture_radius == 0.0 and d.focus_distance == 0.0


# --------------------------------------------------------------------------- the float64 model
def test_warp_known_answers():
    w = pm.square_to_uniform_disk_concentric
    for (u, v), (x, y) in (((0.5, 0.5), (0.0, 0.0)), ((1.0, 0.5), (1.0, 0.0)), ((0.5, 1.0), (0.0, 1.0)),
                           ((0.0, 0.5), (-1.0, 0.0)), ((0.5, 0.0), (0.0, -1.0))):
        gx, gy = w(u, v)
        assert abs(gx - x) < 1e-15 and abs(gy - y) < 1e-15, (u, v, gx, gy)
    g = np.random.default_rng(0).random((2, 4096))
    x, y = w(g[0], g[1])
    assert np.all(x * x + y * y <= 1.0 + 1e-15)
    # the warp preserves area: mean r^2 of a stratified 64 x 64 grid (midpoints) is the disk's 1/2,
    # to the midpoint rule's error.  r^2 = max(x^2, y^2) on the square [-1, 1]^2 with cells of
    # width h = 2 / 64: the smooth part is low by h^2 / 12 (midpoint rule for a square), the cells on
    # the two diagonals (kink of the max) by another h^2 / 6 (E max(a, b) = h / 6 per cell, summed):
    # h^2 / 4 = 1 / 64^2 to leading order; half as much again is allowed for the next order.
    c = (np.arange(64) + 0.5) / 64
    uu, vv = np.meshgrid(c, c, indexing="ij")
    x, y = w(uu, vv)
    assert abs(np.mean(x * x + y * y) - 0.5) <= 1.5 / 64 ** 2


def test_sampler_and_collimated_ray_match_oracle(oracle):
    """The model's sampler, camera mapping, to_world and segment against the oracle's collimated ray
    (fp32): origins to 64 ulp of the distance, directions to 64 ulp of 1."""
    d = pm.projector_scene("collimated")
    pix = pm.dense_pixels(d)
    spp, seed = 2, 3
    m = pm.model_rays(d, pix, np.arange(len(pix)), spp, seed)
    tol_o, tol_d = 64 * np.spacing(np.float32(d.distance)), 64 * np.spacing(np.float32(1.0))
    for i in range(0, len(pix) * spp, 37):
        r = oracle.ray(d, int(pix[i // spp]), i, seed)
        assert np.abs(r["o"] - m["o"][i]).max() <= tol_o and np.abs(r["d"] - m["d"][i]).max() <= tol_d
        assert r["hit"] == bool(m["hit"][i])
        if r["hit"]:
            assert np.abs(r["o2"] - m["o2"][i]).max() <= tol_o and abs(r["maxt"] - m["maxt"][i]) <= tol_o


def test_model_limits():
    """aperture 0: the telecentric ray is the collimated ray's line (origin on the aperture plane);
    every ray of a pixel passes that pixel's point of the focus plane; lens chief rays of
    neighbouring pixels are pixel_size * s / focus_distance apart at axial distance s."""
    xc, yc = np.array([0.3, -1.1]), np.array([-0.2, 0.7])
    u = np.array([0.21, 0.93]), np.array([0.77, 0.08])
    for kind in ("telecentric", "lens"):
        d = pm.projector_scene(kind)
        o, dr = pm.get_ray(d, xc, yc, *u)
        assert np.allclose(np.linalg.norm(dr, axis=-1), 1.0, atol=1e-15)
        F = d.focus_distance + (pm.ZC if kind == "telecentric" else 0.0)
        p = o + dr * (F / dr[:, 2])[:, None]   # where the ray meets the plane z = F
        assert np.allclose(p[:, 0], xc, atol=1e-13) and np.allclose(p[:, 1], yc, atol=1e-13)
        assert np.all(np.hypot(o[:, 0] - (xc if kind == "telecentric" else 0), o[:, 1] - (yc if kind == "telecentric" else 0))
                      <= d.aperture_radius + 1e-12)
    d = pm.projector_scene("telecentric", aperture=0.0)
    o, dr = pm.get_ray(d, xc, yc, *u)
    assert np.array_equal(dr, np.array([[0, 0, 1.0]] * 2)) and np.array_equal(o[:, :2], np.stack([xc, yc], -1))
    d = pm.projector_scene("lens", aperture=0.0)
    x0, y0 = pm.camera_xy(d, np.array([5, 6]), np.array([4, 4]), 0.5, 0.5)
    o, dr = pm.get_ray(d, x0, y0, np.array([0.5, 0.5]), np.array([0.5, 0.5]))
    for s in (5.0, 20.0, 23.0):
        p = o + dr * (s / dr[:, 2])[:, None]
        assert np.linalg.norm(p[0] - p[1]) == pytest.approx(float(np.float32(0.15)) * s / 20.0, rel=1e-12)


def test_to_world_matches_collimated_convention():
    """The general camera -> world map reduces to tvam_ray_world for (xc, yc, zc), direction +z."""
    d = pm.projector_scene("collimated")
    a = np.array([0.3])
    o, dr = pm.to_world(d, a, np.array([[0.4, -0.2, pm.ZC]]), np.array([[0.0, 0.0, 1.0]]))
    c, s, D = np.cos(a), np.sin(a), 20.0 - pm.ZC
    assert np.allclose(o[0], [c[0] * D + s[0] * 0.4, s[0] * D - c[0] * 0.4, -0.2], atol=1e-14)
    assert np.allclose(dr[0], [-c[0], -s[0], 0.0], atol=1e-15)
    back = pm.to_camera(d, a, o)
    assert np.allclose(back[0], [0.4, -0.2, pm.ZC], atol=1e-13)


def test_short_vial_margins():
    """The seeds the GPU hit test uses keep every ray 1e-4 away from an open-end decision."""
    pix = None
    for kind, fov, seed in (("telecentric", False, 67), ("lens", False, 7), ("lens", True, 7)):
        d = pm.projector_scene(kind, height=2.4, lens_fov=fov)
        pix = pm.dense_pixels(d) if pix is None else pix
        m = pm.model_rays(d, pix, np.arange(len(pix)), 2, seed)
        assert m["margin"].min() > 1e-4
        assert 0.5 < m["hit"].mean() < 0.9  # some rays enter or leave through the open ends

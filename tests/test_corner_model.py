"""'filter_corner' without a GPU: known answers of the float64 model (tests/corner_model.py), the
fp32 geometry of drtvam_amd/csrc/tvam_firsthit.h host-compiled (tools/corner_check.sh) against that
model, and the plumbing (integrator registry, ABI entry, argument validation before any HIP call)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import corner_model as cm
import projector_model as pm
from drtvam_amd import _abi
from drtvam_amd.configs import desc_from_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_EXT = 12.408


def _angle(desc, pixels, a):
    return np.asarray(pixels)[np.asarray(pixels) // (desc.res_x * desc.res_y) == a]


def _lateral(desc, pixels):
    """Camera-space x (lateral offset) and y (height) of the pixels' centres."""
    pix = np.asarray(pixels) % (desc.res_x * desc.res_y)
    return pm.camera_xy(desc, pix % desc.res_x, pix // desc.res_x, 0.5, 0.5)


# --------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("radius", [0.2, 0.6])
def test_square_at_angle_zero_drops_the_edge_columns(radius):
    """Pattern 0 looks along -x at the face x = w_ext / 2: with dist = w_ext / 2 the dropped
    columns are those with lateral offset in (dist - radius, dist] and those beyond w_ext / 2."""
    d = desc_from_config(cm.corner_scene("square", 8, resx=200, pixel=0.13))
    pix = _angle(d, pm.dense_pixels(d), 0)
    dist = float(np.float32(W_EXT / 2))
    m = cm.corner_model(d, pix, dist, radius)
    lat, y = _lateral(d, pix)
    inside = np.abs(y) <= 1.0
    expect_drop = ~inside | (np.abs(lat) > dist - float(np.float32(radius)))
    assert m["undecided"].sum() == 0
    assert np.array_equal(~m["keep"], expect_drop)
    assert (~m["keep"]).sum() == expect_drop.sum() and 0 < m["corner"].sum() < inside.sum()
    assert np.array_equal(m["corner"], inside & (np.abs(lat) > dist - float(np.float32(radius))) & (np.abs(lat) <= dist))


@pytest.mark.parametrize("vial", ["cylindrical", "index_matched"])
def test_tube_drops_the_chords_around_the_45_degree_points(vial):
    """Radius R, dist = R / sqrt(2): a hit at azimuth phi is dropped iff its chord distance
    2 R sin(|phi' - 45 deg| / 2) from the 45-degree point of its quadrant is below radius."""
    d = desc_from_config(cm.corner_scene(vial, 8, resx=200, pixel=0.13))
    R = cm.outer_radius(d)
    assert R == 6.5
    radius = 0.6
    for a in (0, 1, 3):
        pix = _angle(d, pm.dense_pixels(d), a)
        m = cm.corner_model(d, pix, R / np.sqrt(2.0), radius)
        lat, y = _lateral(d, pix)
        hit = (np.abs(y) <= 1.0) & (np.abs(lat) <= R)
        assert np.array_equal(m["hit"], hit)
        # azimuth of the entry point: the projector sits at azimuth alpha, the entry at alpha - asin(lat / R)
        alpha = 2.0 * np.pi * a / 8
        with np.errstate(invalid="ignore"):
            phi = alpha - np.arcsin(np.clip(lat / R, -1, 1))
        fold = np.arctan2(np.abs(np.sin(phi)), np.abs(np.cos(phi)))
        chord = 2.0 * R * np.sin(np.abs(fold - np.pi / 4) / 2.0)
        near = np.abs(chord - float(np.float32(radius))) < 1e-3  # fp32 dist / radius vs. the closed form's
        assert np.array_equal(m["corner"][~near], (hit & (chord < radius))[~near])
        assert m["corner"].sum() > 0


def test_rows_above_the_vial_are_dropped():
    for vial in ("square", "cylindrical", "index_matched"):
        d = desc_from_config(cm.corner_scene(vial, 8))
        pix = pm.dense_pixels(d)
        m = cm.corner_model(d, pix, 6.204, 0.2)
        _, y = _lateral(d, pix)
        assert set(np.round(np.abs(y), 6)) == {0.25, 0.75, 1.25}
        assert not m["hit"][np.abs(y) > 1.0].any() and not m["keep"][np.abs(y) > 1.0].any()
        assert m["hit"][np.abs(y) < 1.0].any()


def test_occluder_plate_takes_the_hit():
    """A plate 10 mm out, in front of the corner pattern 1 looks at: its rays end on the plate (p . n
    = 10), away from the corner, so the pixels the corner would drop stay active."""
    d = desc_from_config(cm.corner_scene("square", 8))
    pix = _angle(d, pm.dense_pixels(d), 1)
    alpha = float(pm.angle_alpha(d, 1))
    occ = cm.plate(alpha)
    m0 = cm.corner_model(d, pix, 6.204, 0.6)
    m1 = cm.corner_model(d, pix, 6.204, 0.6, occluders=occ)
    lat, y = _lateral(d, pix)
    behind = (np.abs(lat) < 0.6) & (np.abs(y) < 0.45)
    n = np.array([np.cos(alpha), np.sin(alpha), 0.0])
    assert behind.sum() == 4
    assert np.allclose(m1["p"][behind] @ n, 10.0, atol=1e-5) and np.allclose(m0["p"][behind] @ n, 8.774 - 0.25, atol=2e-3)
    assert m0["corner"][behind].all() and m1["keep"][behind].all()
    assert np.array_equal(m0["keep"][~behind], m1["keep"][~behind])
    assert m1["undecided"].sum() == 0


def test_undecided_marks_the_threshold():
    """A ray displaced across a decision by less than delta is undecided; one farther away is not."""
    d = desc_from_config(cm.corner_scene("square", 8))
    dl = cm.delta(d)
    assert dl == pytest.approx(64 * 2.0 ** -24 * (20.0 + np.sqrt(2.0) * float(np.float32(6.204))))
    o = np.array([[19.0, 6.004 + s * f * dl, 0.0] for s in (1, -1) for f in (0.5, 3.0)])
    dd = np.tile([-1.0, 0.0, 0.0], (4, 1))
    m = cm.evaluate(d, o, dd, float(np.float32(6.204)), 0.2)
    r = float(np.float32(6.204)) - float(np.float32(0.2))
    assert list(m["undecided"]) == [abs(y - r) < dl for y in o[:, 1]] and m["undecided"].sum() == 2


# --------------------------------------------------------------------------- fp32 geometry on the host
def _case_file(path, desc, o, d, dist, radius, occ):
    occ = np.zeros((0, 3, 3), np.float32) if occ is None else np.asarray(occ, np.float32)
    with open(path, "w") as f:
        f.write("%d %.9g %.9g %.9g %.9g %.9g %d %d\n" % (desc.vial_type, desc.vial_r, desc.vial_r_ext,
                                                      0.5 * desc.vial_height, np.float32(dist), np.float32(radius),
                                                      len(occ), len(o)))
        np.savetxt(f, occ.reshape(-1, 9), fmt="%.9g")
        np.savetxt(f, np.concatenate([o, d], 1), fmt="%.9g")


def host_cases():
    """(name, desc, pixels, streams, dist, radius, occluders): the GPU tests' scenes."""
    cases = []
    for vial in ("square", "cylindrical", "index_matched"):
        for A in (8, 7):
            d = desc_from_config(cm.corner_scene(vial, A))
            dist = 6.204 if vial == "square" else cm.outer_radius(d) / np.sqrt(2.0)
            for radius in (0.2, 0.6):
                cases.append((f"{vial}-{A}-{radius}", d, pm.dense_pixels(d), None, dist, radius, None))
    d = desc_from_config(cm.corner_scene("square", 8))
    cases.append(("plate", d, pm.dense_pixels(d), None, 6.204, 0.6, cm.plate(float(pm.angle_alpha(d, 1)))))
    for kind, height in (("telecentric", 40.0), ("telecentric", 3.0), ("lens", 3.0)):
        d = pm.projector_scene(kind, height=height)
        cases.append((f"{kind}-{height}", d, pm.dense_pixels(d), None, 2.9 / np.sqrt(2.0), 0.3, None))
    return cases


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_firsthit_header_matches_the_model(tmp_path):
    """tvam_firsthit.h, host-compiled, on the fp32 rays of every GPU test scene: exact verdicts on
    the decided pixels, hit points within the model's tolerance (corner_model.compare)."""
    cases = host_cases()
    files, models = [], []
    for i, (name, d, pix, streams, dist, radius, occ) in enumerate(cases):
        o, dd = cm.corner_rays(d, pix, streams)
        o32, d32 = o.astype(np.float32), dd.astype(np.float32)  # the rays the fp32 code is given
        path = tmp_path / f"case{i}.txt"
        _case_file(path, d, o32, d32, dist, radius, occ)
        files.append(str(path))
        models.append(cm.evaluate(d, o32.astype(np.float64), d32.astype(np.float64), dist, radius, occ))
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run([os.path.join(ROOT, "tools", "corner_check.sh")] + files, capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    blocks = re.split(r"^case \d+ \d+\n", r.stdout, flags=re.M)[1:]
    assert len(blocks) == len(cases)
    for (name, d, *_), m, blk in zip(cases, models, blocks):
        out = np.array(blk.split(), dtype=np.float64).reshape(-1, 5)
        assert len(out) == len(m["keep"]), name
        hits = np.concatenate([out[:, 2:5], out[:, 1:2]], 1)
        print(name, "undecided", cm.compare(m, out[:, 0], hits), "of", len(out), "kept", int(out[:, 0].sum()))
        assert 0 < out[:, 0].sum() < len(out), name
    # the short telecentric / lens vials: some rays come in through an open end and meet the inside wall
    for name, d, pix, streams, dist, radius, occ in cases:
        if name.endswith("-3.0"):
            o, dd = cm.corner_rays(d, pix, streams)
            t, p = cm.first_hit(d, o, dd)
            inside_wall = np.isfinite(t) & (np.sum(p[:, :2] * dd[:, :2], -1) > 0)
            assert inside_wall.any(), name


# --------------------------------------------------------------------------- plumbing
def test_corner_integrator_is_registered():
    from drtvam_amd.integrators import CornerIntegrator, integrators
    assert integrators["corner"] is CornerIntegrator
    with pytest.raises(KeyError):
        CornerIntegrator({"regular_sampling": True})
    c = CornerIntegrator({"dist": 6.204})
    assert c.radius == 0.1 and c.dist == 6.204 and c.to_string() == "CornerIntegrator"
    assert CornerIntegrator({"dist": 1.0, "radius": 0.25}).radius == 0.25


def test_tvam_corner_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "tvam.h")).read()
    assert re.search(r"\bint\s+tvam_corner\s*\(tvam_plan\*\s*plan,\s*const uint32_t\*\s*active_pixels,\s*uint64_t n_active,"
                     r"\s*float dist,\s*float radius,\s*float\*\s*keep,\s*float\*\s*hits,\s*void\*\s*hip_stream\)", header)
    assert "tvam_corner" in _abi.EXPORTS
    assert hasattr(_abi.load_library(), "tvam_corner")
    assert _abi.load_library().tvam_abi_version() == 13


def test_tvam_corner_validates_before_hip():
    """Null plan / keep, radius < 0, non-finite dist, misaligned hits and a dense count that is not
    the shard's return TVAM_ERR_INVALID with a message, before any HIP call (no GPU here).  The plan
    is a zeroed stand-in: validation reads only its descriptor and constants."""
    lib = _abi.load_library()
    buf = (ctypes.c_float * 64)()
    q = ctypes.addressof(buf)
    fake = ctypes.create_string_buffer(1 << 16)  # larger than struct tvam_plan; zeros: an empty shard
    p = ctypes.addressof(fake)
    cases = [
        lib.tvam_corner(None, None, 0, 1.0, 0.1, q, None, None),              # null plan
        lib.tvam_corner(p, None, 0, 1.0, 0.1, None, None, None),              # null keep
        lib.tvam_corner(p, None, 0, 1.0, -0.1, q, None, None),                # radius < 0
        lib.tvam_corner(p, None, 0, 1.0, float("nan"), q, None, None),        # radius NaN
        lib.tvam_corner(p, None, 0, float("inf"), 0.1, q, None, None),        # dist not finite
        lib.tvam_corner(p, None, 0, float("nan"), 0.1, q, None, None),
        lib.tvam_corner(p, None, 0, 1.0, 0.1, q, ((q + 15) & ~15) + 4, None),  # hits not 16-byte aligned
        lib.tvam_corner(p, None, 5, 1.0, 0.1, q, None, None),                 # dense count != shard size (0)
    ]
    for i, rc in enumerate(cases):
        assert rc == _abi.TVAM_ERR_INVALID, (i, rc)
        assert lib.tvam_last_error().decode().startswith("tvam_corner:")
    # a valid empty call returns before touching the device
    assert lib.tvam_corner(p, None, 0, 1.0, 0.1, q, None, None) == 0

"""The float64 model of dielectric occluders (tests/insert_model.py) on its own, and against the
library's host walk (tvam_insert_segments, the code the kernels run): no GPU.

  1. the meshes are closed and wound outwards, and PLY files keep them bit for bit;
  2. the model reproduces the closed forms of a slab at normal incidence;
  3. the host walk agrees with the model on rays of 0, 1, 2 and 3 segments: total internal reflection
     inside an insert, a path ended by max_depth inside an insert, an open-end exit, the brute-force
     and the hierarchy sizes, a black occluder behind an insert, and Russian roulette acting;
  4. the comparison rejects three planted errors of the model;
  5. at most 1 % of any GPU test scene's rays lie below the 1e-4 margin."""
import numpy as np
import pytest

from drtvam_amd import _abi
from drtvam_amd.utils import read_ply

import insert_model as im
import projector_model as pm

# tests/test_gpu_mesh_vial.py's export-vs-model bounds (times the segment's condition number,
# double_vial_model.compare_segments)
TOL_O = 4 * 64 * float(np.spacing(np.float32(20.0)))
TOL_D = 4 * 64 * float(np.spacing(np.float32(1.0)))


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("insert_meshes")
    im.write_meshes(d)
    return d


def within(r):
    return r["e_o"] <= TOL_O and r["e_t"] <= TOL_O and r["e_d"] <= TOL_D and r["e_w"] <= TOL_D


# --------------------------------------------------------------------------- 1. meshes
@pytest.mark.parametrize("name", im.MESHES)
def test_meshes_are_closed_and_survive_ply(name, meshdir):
    t = im.mesh(name)
    assert t.dtype == np.float32 and im.check_closed(t)
    v, f = read_ply(str(meshdir / (name + ".ply")))
    back = np.asarray(v, np.float32)[np.asarray(f)]
    assert np.array_equal(back, t)  # vertices, order and winding
    assert np.abs(t[..., 0]).max() < 2.0 and np.abs(t[..., 1]).max() < 1.8 and np.abs(t[..., 2]).max() < 2.0
    want = {"box": 12, "prism": 24, "u": 28, "fine": 432, "far": 12, "black": 12}[name]
    assert t.shape == (want, 3, 3)


def test_fine_box_exceeds_the_lds_budget_and_box_is_brute():
    """TVAM_MESH_BRUTE_MAX 16 and TVAM_MESH_LDS_BUDGET 16384 (tvam_mesh.h): 36 bytes of vertices and 4 of
    id per triangle alone put 432 triangles past the budget, before any node."""
    assert len(im.mesh("box")) <= 16 < len(im.mesh("prism"))
    assert len(im.mesh("fine")) > 300 and 40 * len(im.mesh("fine")) > 16384
    assert 40 * len(im.mesh("prism")) + 32 * 2 * len(im.mesh("prism")) < 16384


# --------------------------------------------------------------------------- 2. closed forms
def slab_scene(t_slab=0.8, x_face=0.5):
    """An axis-aligned slab x in [x_face - t_slab, x_face] inside an index-matched vial of radius 2.9; rays
    along -x at normal incidence."""
    tris = im.box_tris((x_face - t_slab, -1.0, -1.0), (x_face, 1.0, 1.0)).astype(np.float32).astype(np.float64)
    cont = dict(r=2.9, half=2.0)
    y = np.array([-0.3, 0.0123, 0.41])
    o = np.stack([np.full(3, 20.0), y, np.array([0.1, -0.2, 0.05])], -1)
    d = np.tile([-1.0, 0.0, 0.0], (3, 1))
    return cont, tris, o, d


def test_model_reproduces_the_slab_closed_forms():
    n1, n2, st, t_slab, x_face = im.EXT_IOR, im.INT_IOR, 0.7, 0.8, 0.5
    cont, tris, o, d = slab_scene(t_slab, x_face)
    m = im.trace(o, d, cont, tris, np.full(len(tris), n2 / n1), st, 8)
    assert np.array_equal(m["n"], [2, 2, 2]) and m["margin"].min() > 1e-3
    for i in range(3):
        s0, s1 = m["segs"][i, 0], m["segs"][i, 1]
        x_in = np.sqrt(2.9 ** 2 - o[i, 1] ** 2)
        t1 = x_in - x_face  # the resin path in front of the slab
        T2, A = im.slab_closed_form(n1, n2, st, t1)
        assert abs(s0[7] - 1.0) < 1e-15                      # index matched: nothing lost at the vial
        assert abs(s0[3] - t1) < 1e-3                        # up to the spawn offset
        assert abs(s1[7] / (T2 * np.exp(-st * s0[3])) - 1.0) < 1e-12   # (1 - F)^2 e^{-st t1}: no loss inside
        assert abs(np.exp(-st * s0[3]) / A - 1.0) < 1e-3
        # the second segment starts one slab thickness later, on the far face
        assert abs((s0[0] - s0[3]) - s1[0] - t_slab) < 1e-3 and abs(s1[0] - (x_face - t_slab)) < 1e-3
        assert np.allclose(s1[4:7], [-1.0, 0.0, 0.0], atol=1e-15)
    # and the weights the library's own walk gives
    desc = pm.projector_scene("collimated")
    desc.vial_r, desc.vial_height, desc.sigma_t, desc.max_depth = 2.9, 4.0, st, 8
    desc.set_inserts([(tris.astype(np.float32), n2, n1)])
    segs, nseg = _abi.insert_segments(desc, o, d, None, 4)
    assert np.array_equal(nseg, [2, 2, 2])
    F = ((n1 - n2) / (n1 + n2)) ** 2
    assert np.abs(segs[:, 1, 7] / ((1 - F) ** 2 * np.exp(-st * segs[:, 0, 3].astype(np.float64))) - 1.0).max() < 1e-5


# --------------------------------------------------------------------------- 3. host walk against the model
def host_and_model(desc, o, d, u=None, **kw):
    m = im.trace_desc(desc, o, d, u=u, **kw)
    segs, nseg = _abi.insert_segments(desc, o, d, None if u is None else u.astype(np.float32), im.MAX_SEGMENTS)
    ok = m["margin"] > im.MARGIN
    assert np.array_equal(nseg[ok], m["n"][ok])
    return segs, nseg, m


CASES = [
    # vial, kind, regular, inserts, black, extra
    ("index_matched", "collimated", True, ("box",), False, {}),
    ("index_matched", "telecentric", False, ("prism", "u"), True, {}),
    ("cylindrical", "lens", False, ("fine",), False, {}),
    ("cylindrical", "collimated", True, ("u", "box"), True, {}),
    ("square", "telecentric", False, ("prism",), False, {}),
    ("square", "collimated", False, ("fine", "u"), True, {}),
    ("square", "lens", False, ("u",), False, {"max_depth": 4}),           # ended by max_depth inside the piece
    ("index_matched", "lens", False, ("box",), False, {"int_ior": 2.419}),  # 'diamond': total internal reflection
]


@pytest.mark.parametrize("vial,kind,regular,inserts,black,extra", CASES,
                         ids=[f"{c[0]}-{c[1]}-{'+'.join(c[3])}{'-black' if c[4] else ''}{''.join('-%s%s' % kv for kv in c[5].items())}"
                              for c in CASES])
def test_host_walk_matches_model(meshdir, vial, kind, regular, inserts, black, extra):
    m = im.scene_model(meshdir, vial, kind, regular, inserts=inserts, black=black, **extra)
    d = m["desc"]
    assert not im.roulette_on(d)
    segs, nseg = _abi.insert_segments(d, m["o"], m["d"], None, im.MAX_SEGMENTS)
    r = im.compare_segments(segs, m)
    ok = m["margin"] > im.MARGIN
    assert np.array_equal(nseg[ok], m["n"][ok])
    hist = np.bincount(m["n"][ok], minlength=4)
    ends = dict(zip(*np.unique(m["ends"][ok], return_counts=True)))
    print(f"{vial} {kind} {inserts}: rays {len(nseg)} segments per ray {hist.tolist()} ends {ends} below margin "
          f"{r['low']:.4f} |do2| {r['e_o']:.2e} |dmaxt| {r['e_t']:.2e} |dd2| {r['e_d']:.2e} |dw|/w {r['e_w']:.2e}")
    assert r["low"] <= 0.01 and within(r)
    assert hist[1] > 0
    if "max_depth" not in extra:
        assert hist[2] > 0
        if "u" in inserts:
            assert hist[3] > 0                  # both arms and the gap
    if black:
        assert ends.get("black", 0) > 0
    if "max_depth" in extra:
        assert ends.get("depth", 0) > 0
    if "int_ior" in extra:
        assert ends.get("tir", 0) > len(nseg) // 50


def test_segment_counts_zero_to_three_and_the_path_ends(meshdir):
    """Hand-placed rays through the U-piece in a short index-matched tube: no segment (the ray passes above
    the vial), one (beside the piece), two (through one arm), three (through both arms and the gap), an
    open-end exit behind the piece (the segment in progress deposits nothing), a path ended by max_depth
    inside the piece, total internal reflection inside a 'diamond' piece."""
    d = im.insert_scene(meshdir, "index_matched", "collimated", True, inserts=("u",), max_depth=10, rr_depth=10)
    u_mesh = d.inserts[0][0].astype(np.float64)
    c = u_mesh.reshape(-1, 3).mean(0)
    R = im._rot(0.43, 0.11)
    ex, ey, ez = R[:, 0], R[:, 1], R[:, 2]

    def ray(through, direction, back=10.0):
        direction = direction / np.linalg.norm(direction)
        return through - back * direction, direction

    rays = [
        ray(np.array([0.0, 0.0, 2.5]), np.array([-1.0, 0.02, 0.0])),        # 0: above the vial
        ray(c + 1.4 * ey + 0.03 * ez, -ex + 0.013 * ey),                     # 1: beside the piece
        ray(c - 0.45 * ey + 0.03 * ez, -ex + 0.013 * ey),                    # 2: through the base
        ray(c + 0.35 * ey + 0.03 * ez, -ex + 0.013 * ey),                    # 3: both arms and the gap
        ray(c + 0.35 * ey + 0.3 * ez, -ex + 0.013 * ey + 0.7 * ez, 3.5),    # in through the wall, up and out of the open end
    ]
    o, dd = (np.array(x) for x in zip(*rays))
    segs, nseg, m = host_and_model(d, o, dd)
    assert m["margin"].min() > im.MARGIN
    assert m["n"].tolist() == [0, 1, 2, 3, m["n"][4]] and m["ends"][4] == "none" and m["ends"][0] == "none"
    assert m["n"][4] >= 1  # it deposited in front of the piece, and nothing on its way out through the open end
    r = im.compare_segments(segs, m)
    assert within(r)
    # max_depth 2: the vial, then the first arm's face: the path ends inside the piece after one segment
    d2 = d.copy()
    d2.max_depth = 2
    segs, nseg, m = host_and_model(d2, o[3:4], dd[3:4])
    assert m["n"].tolist() == [1] and m["ends"][0] == "depth" and nseg.tolist() == [1]
    # a 'diamond' box met at 45 degrees near its corner: total internal reflection at the adjacent face
    dt = im.insert_scene(meshdir, "index_matched", "collimated", True, inserts=("box",), int_ior=2.419)
    box = dt.inserts[0][0].astype(np.float64)
    Rb = im._rot(0.31, 0.0)
    corner = np.array([0.233, -0.171, 0.047]) + Rb @ np.array([0.55, 0.45, 0.0])
    through = corner - 0.12 * Rb[:, 1]  # on the +x face, 0.12 below the corner
    o1, d1 = ray(through, -(Rb[:, 0] - Rb[:, 1]), back=8.0)
    segs, nseg, m = host_and_model(dt, o1[None], d1[None])
    assert m["margin"][0] > im.MARGIN and m["ends"][0] == "tir" and m["n"].tolist() == [1] and nseg.tolist() == [1]
    assert box.shape == (12, 3, 3)


def test_roulette_acts_with_supplied_draws(meshdir):
    """rr_depth 1, max_depth 8 and the caller's u: from iteration 2 on q = min(0.99, attenuation) decides, and the
    survivors' weights take 1 / q."""
    m0 = im.scene_model(meshdir, "cylindrical", "telecentric", False, inserts=("u", "prism"), black=True)
    d = m0["desc"].copy()
    d.rr_depth, d.max_depth = 1, 8
    assert im.roulette_on(d)
    rng = np.random.default_rng(21)
    u = rng.uniform(0.0, 1.0, (len(m0["o"]), 8, 4)).astype(np.float32).astype(np.float64)
    segs, nseg, m = host_and_model(d, m0["o"], m0["d"], u=u)
    r = im.compare_segments(segs, m)
    ends = dict(zip(*np.unique(m["ends"], return_counts=True)))
    print(f"roulette: ends {ends} below margin {r['low']:.4f} |dw|/w {r['e_w']:.2e}")
    assert r["low"] <= 0.01 and within(r)
    assert ends.get("rr", 0) > len(nseg) // 20
    # survivors carry 1 / q: some later segment starts with more than its predecessor's attenuation allows without it
    plain = im.trace_desc(m0["desc"], m0["o"], m0["d"])
    both = (m["n"] >= 2) & (plain["n"] >= 2) & (m["margin"] > im.MARGIN)
    assert both.any() and (m["segs"][both, 1, 7] > plain["segs"][both, 1, 7] * (1 + 1e-9)).any()
    # without u roulette never acts, whatever rr_depth says
    segs0, nseg0 = _abi.insert_segments(d, m0["o"], m0["d"], None, im.MAX_SEGMENTS)
    r0 = im.compare_segments(segs0, dict(plain))
    assert within(r0)
    with pytest.raises(ValueError, match="u must be"):
        _abi.insert_segments(d, m0["o"], m0["d"], u[:, :4], im.MAX_SEGMENTS)


# --------------------------------------------------------------------------- 4. planted errors
@pytest.mark.parametrize("flaw", ["flag", "exp", "eta"])
def test_checker_rejects_planted_errors(meshdir, flaw):
    """The same comparison with one error planted in the model: the medium flag not cleared inside the insert
    (an extra segment), e^{-sigma_t t} applied inside the insert (later weights low), eta inverted (directions
    and weights off)."""
    m = im.scene_model(meshdir, "index_matched", "collimated", True, inserts=("box",))
    d = m["desc"]
    segs, nseg = _abi.insert_segments(d, m["o"], m["d"], None, im.MAX_SEGMENTS)
    assert within(im.compare_segments(segs, m))
    bad = im.trace_desc(d, m["o"], m["d"], flaw=flaw)
    try:
        r = im.compare_segments(segs, bad)
    except AssertionError:
        return  # the segment counts disagree
    assert not within(r), r


# --------------------------------------------------------------------------- 5. the exclusion cap
GPU_SCENES = [(v, k, reg, ins, blk)
              for v in ("index_matched", "cylindrical", "square")
              for (k, reg) in (("collimated", True), ("telecentric", False), ("lens", False))
              for (ins, blk) in ((("box",), False), (("prism", "u"), True), (("fine",), False))]


def test_at_most_one_percent_of_any_scene_lies_below_the_margin(meshdir):
    worst = 0.0
    for vial, kind, regular, ins, blk in GPU_SCENES:
        for spp in ((1,) if regular else (1, 3)):
            m = im.scene_model(meshdir, vial, kind, regular, spp=spp, inserts=ins, black=blk)
            low = int((m["margin"] <= im.MARGIN).sum())
            worst = max(worst, low / len(m["margin"]))
            assert low <= 0.01 * len(m["margin"]), (vial, kind, ins, spp, low, len(m["margin"]))
    m = im.scene_model(meshdir, "square", "lens", False, spp=3, inserts=("prism", "u"), black=True, max_depth=16, rr_depth=2,
                       extinction=0.2)
    low = int((m["margin"] <= im.MARGIN).sum())
    assert m["u"] is not None and low <= 0.01 * len(m["margin"])
    print(f"largest share below the margin: {worst:.4f}; with roulette {low / len(m['margin']):.4f}")
    # the film comparisons leave out whole pixels: spp rays for every pixel with a ray below the margin
    for name, (vial, kind, regular, kw) in im.FILM_VARIANTS.items():
        m = im.scene_model(meshdir, vial, kind, regular, im.FILM_SPP, im.FILM_SEED, **kw)
        out = int((~im.film_keep(m)).sum()) * m["spp"]
        print(f"{name}: {out} of {len(m['margin'])} rays left out")
        assert out <= 0.01 * len(m["margin"]), name

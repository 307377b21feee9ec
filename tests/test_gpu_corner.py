"""GPU: 'filter_corner' (tvam_corner, the `corner` integrator, TvamProblem._filter_corner) against
the float64 model of tests/corner_model.py under its rule: at most 0.5 % of a case's pixels
undecided by the model alone, exact verdicts on all others, hit points within delta + the model's
own spread.  Shapes are the smallest that can go wrong: a 48 x 6 px DMD wider than the square's
diagonal and taller than the 2 mm vial, 8 patterns (45, 135, ... degrees look straight at a corner)
and 7, more than one workgroup (2304 entries), crops, shards and compacted sets."""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import corner_model as cm
import projector_model as pm
from drtvam_amd.configs import desc_from_config
from drtvam_amd.engine import Projection

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
DIST = 6.204


def _t(a, dtype=None):
    return torch.as_tensor(a if dtype is None else np.asarray(a).astype(dtype), device=DEV).contiguous()


def _run(proj, dist, radius, pixels=None):
    keep, hits = proj.corner(dist, radius, active_pixels=None if pixels is None else _t(pixels, np.int32), hits=True)
    torch.cuda.synchronize()
    return keep.cpu().numpy(), hits.cpu().numpy()


CASES = {
    # name: (vial, patterns, clockwise, crop, plate, jittered plan)
    "square-8": ("square", 8, False, None, False, False),
    "square-7-jittered-plan": ("square", 7, False, None, False, True),
    "cylindrical-8": ("cylindrical", 8, False, None, False, False),
    "index-matched-8": ("index_matched", 8, False, None, False, False),
    "square-8-clockwise": ("square", 8, True, None, False, False),
    "square-8-crop": ("square", 8, False, (41, 4, 5, 1), False, False),
    "square-8-plate": ("square", 8, False, None, True, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mask_and_hits_match_the_model(name):
    vial, A, cw, crop, plate, jitter = CASES[name]
    cfg = cm.corner_scene(vial, A, clockwise=cw, crop=crop)
    cfg["regular_sampling"] = not jitter  # the pass samples regularly whatever the plan does
    d = desc_from_config(cfg)
    occ = None
    if plate:
        occ = cm.plate(float(pm.angle_alpha(d, 1)))
        d.set_occluders(occ)
    dist = DIST if vial == "square" else cm.outer_radius(d) / np.sqrt(2.0)
    proj = Projection(d, DEV)
    pix = pm.dense_pixels(d)
    for radius in (0.2, 0.6):
        m = cm.corner_model(d, pix, dist, radius, occluders=occ)
        keep, hits = _run(proj, dist, radius)
        und = cm.compare(m, keep, hits)
        print(name, radius, "undecided", und, "kept", int(keep.sum()), "of", keep.size)
        assert 0 < keep.sum() <= m["hit"].sum()
        if radius == 0.6:  # corners are dropped, not only misses
            assert m["corner"].any() and keep.sum() < m["hit"].sum()
        assert np.array_equal(proj.corner(dist, radius).cpu().numpy(), keep)  # without hits: the same mask
    proj.close()


@pytest.mark.parametrize("kind,height", [("telecentric", 40.0), ("telecentric", 3.0), ("lens", 3.0)])
def test_telecentric_and_lens(kind, height):
    """3-D rays with the aperture draws of streams = positions in the active set; the short vial
    lets rays in through an open end, where the inside wall is a valid hit."""
    d = pm.projector_scene(kind, height=height)  # jittered plan: the pass still samples regularly
    dist, radius = 2.9 / np.sqrt(2.0), 0.3
    proj = Projection(d, DEV)
    pix = pm.dense_pixels(d)
    m = cm.corner_model(d, pix, dist, radius)
    keep, hits = _run(proj, dist, radius)
    cm.compare(m, keep, hits)
    assert 0 < keep.sum() < m["hit"].sum()
    if height < 40.0:
        o, dd = cm.corner_rays(d, pix)
        inside_wall = m["hit"] & (np.sum(m["p"][:, :2] * dd[:, :2], -1) > 0)
        assert inside_wall.any() and (hits[inside_wall & ~m["undecided"], 3] > 0).all()
    # a compacted set: every third pixel, streams = positions (not pixel indices), then offset by
    # a lower rank's entries (tvam_plan_set_active)
    sub = pix[::3]
    o_pos, _ = cm.corner_rays(d, sub)
    o_idx, _ = cm.corner_rays(d, sub, streams=np.arange(len(pix))[::3])
    assert not np.allclose(o_pos, o_idx)  # the two seedings give different rays
    for base in (0, 5):
        proj.set_active(base, len(sub) + base)
        ms = cm.corner_model(d, sub, dist, radius, streams=base + np.arange(len(sub)))
        ks, hs = _run(proj, dist, radius, sub)
        cm.compare(ms, ks, hs)
        # the hit points tell the seedings apart: those of the pixel-index streams are farther off
        mi = cm.corner_model(d, sub, dist, radius, streams=np.arange(len(pix))[::3])
        both = ms["hit"] & mi["hit"] & ~ms["undecided"]
        assert np.linalg.norm(hs[both, :3] - mi["p"][both], axis=-1).max() > 100 * ms["delta"]
    proj.close()


def test_sparse_input_equals_dense():
    d = desc_from_config(cm.corner_scene("square", 8))
    proj = Projection(d, DEV)
    pix = pm.dense_pixels(d)
    keep, hits = _run(proj, DIST, 0.6)
    rng = np.random.default_rng(3)
    sel = np.sort(rng.permutation(len(pix))[: len(pix) // 3])
    ks, hs = _run(proj, DIST, 0.6, pix[sel])
    assert np.array_equal(ks, keep[sel]) and np.array_equal(hs, hits[sel])
    assert 0 < ks.sum() < ks.size
    proj.close()


def test_shards_tile_the_whole_plan():
    cfg = cm.corner_scene("square", 8)
    d = desc_from_config(cfg)
    proj = Projection(d, DEV)
    whole, _ = _run(proj, DIST, 0.6)
    whole = whole.reshape(8, 6, 48)
    proj.close()
    parts = []
    for a0, a1 in ((0, 3), (3, 8)):  # angle shards
        p = Projection(desc_from_config(cfg, angle_range=(a0, a1)), DEV)
        parts.append(_run(p, DIST, 0.6)[0].reshape(a1 - a0, 6, 48))
        # full-DMD indices of the whole plan on a shard: entries of other angles are dropped
        k, h = _run(p, DIST, 0.6, pm.dense_pixels(d))
        k = k.reshape(8, 6, 48)
        assert np.array_equal(k[a0:a1], whole[a0:a1]) and not k[:a0].any() and not k[a1:].any()
        p.close()
    assert np.array_equal(np.concatenate(parts, 0), whole)
    bands = []
    # z-slabs: row bands of every angle (rows 0-2 look into slices 10 and 15, rows 3-5 into 5 and 0)
    for (r0, r1), (z0, z1) in (((0, 3), (8, 16)), ((3, 6), (0, 8))):
        ds = d.copy()
        ds.crop_offset_y += r0
        ds.crop_y = r1 - r0
        ds.slab_begin, ds.slab_end = z0, z1
        p = Projection(ds, DEV)
        bands.append(_run(p, DIST, 0.6)[0].reshape(8, r1 - r0, 48))
        p.close()
    assert np.array_equal(np.concatenate(bands, 1), whole)


def test_corner_integrator_render():
    from drtvam_amd.integrators import integrators
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict
    cfg = cm.corner_scene("square", 8, crop=(41, 4, 5, 1))
    cfg["projector"]["device"] = DEV
    scene = load_dict(load_scene(cfg))
    integ = integrators["corner"]({"regular_sampling": True, "dist": DIST, "radius": 0.6})
    img = integ.render(scene, spp=1)
    assert tuple(img.shape) == scene.projector.size() == (8, 6, 48)
    d = desc_from_config(cm.corner_scene("square", 8, crop=(41, 4, 5, 1)))
    pix = pm.dense_pixels(d)
    m = cm.corner_model(d, pix, DIST, 0.6)
    assert m["undecided"].sum() == 0
    expect = np.zeros(8 * 6 * 48, dtype=np.float32)
    expect[pix[m["keep"]]] = 1.0
    assert np.array_equal(img.cpu().numpy().ravel(), expect)


def _problem_cfg(radius=0.6, **extra):
    cfg = cm.corner_scene("square", 8)
    cfg["filter_corner"] = {"dist": DIST, "radius": radius}
    cfg.update(extra)
    return cfg


def test_problem_compacts_to_the_models_set():
    from drtvam_amd.optimize import TvamProblem
    cfg = _problem_cfg()
    d = desc_from_config(cfg)
    pix = pm.dense_pixels(d)
    m = cm.corner_model(d, pix, DIST, 0.6)
    assert m["undecided"].sum() == 0
    prob = TvamProblem(cfg, device=torch.device(DEV))
    assert np.array_equal(prob.active_pixels.cpu().numpy(), pix[m["keep"]])
    assert prob.n_filtered == prob.n_local == int(m["keep"].sum()) == prob.n_active_global()
    assert prob.x0.numel() == prob.n_local and float(prob.x0.abs().max()) == 0.0
    assert prob.proj.desc.active_total == prob.n_local
    # L-BFGS on the compacted set
    losses = [prob.iteration(i) for i in range(3)]
    assert np.all(np.isfinite(losses)) and losses[1] <= losses[0] and losses[2] <= losses[1]
    assert prob.patterns_local().numel() == prob.n_local
    dense = prob.gather_patterns(prob.patterns_local().float()).cpu().numpy()
    assert dense.size == prob.n_global and not dense[~m["keep"]].any() and dense[m["keep"]].any()
    # Adam on the compacted set
    adam = TvamProblem(_problem_cfg(optimizer={"type": "adam", "lr": 0.05}), device=torch.device(DEV))
    la = [adam.iteration(i) for i in range(3)]
    assert np.all(np.isfinite(la)) and adam.patterns_local().numel() == prob.n_local
    # filter_pixels=False (patterns_fwd given): nothing is filtered
    off = TvamProblem(cfg, device=torch.device(DEV), filter_pixels=False)
    assert off.active_pixels is None and off.n_local == off.n_global


def test_problem_default_radius_and_missing_dist():
    from drtvam_amd.optimize import TvamProblem
    cfg = _problem_cfg()
    cfg["filter_corner"] = {"dist": DIST}
    d = desc_from_config(cfg)
    m = cm.corner_model(d, pm.dense_pixels(d), DIST, 0.1)
    assert m["undecided"].sum() == 0
    prob = TvamProblem(cfg, device=torch.device(DEV))
    assert prob.n_local == int(m["keep"].sum())
    cfg["filter_corner"] = {"radius": 0.2}
    with pytest.raises(KeyError):
        TvamProblem(cfg, device=torch.device(DEV))


def test_problem_with_radon_is_the_intersection():
    from drtvam_amd.optimize import TvamProblem
    base = _problem_cfg(filter_radon=True, spp_filter_radon=2)
    both = TvamProblem(base, device=torch.device(DEV))
    only = copy.deepcopy(base)
    del only["filter_corner"]
    radon = TvamProblem(only, device=torch.device(DEV))
    d = desc_from_config(base)
    pix = pm.dense_pixels(d)
    m = cm.corner_model(d, pix, DIST, 0.6)
    rset = radon.active_pixels.cpu().numpy()
    expect = np.intersect1d(rset, pix[m["keep"]])
    assert 0 < expect.size < rset.size
    assert np.array_equal(both.active_pixels.cpu().numpy(), expect)
    assert both.n_filtered == expect.size and float(both.x0.abs().max()) == 0.0 and both.x0.numel() == expect.size
    assert np.array_equal(pix[both.active_dense.cpu().numpy()], expect)
    losses = [both.iteration(i) for i in range(2)]
    assert np.all(np.isfinite(losses))


def test_problem_empty_result_raises():
    from drtvam_amd.optimize import TvamProblem
    with pytest.raises(ValueError, match="corner filter"):
        TvamProblem(_problem_cfg(radius=30.0), device=torch.device(DEV))


def test_reference_config_end_to_end(tmp_path):
    """tests/files/box_hole_square_sparsity_loss.json of the reference (the one shipped config with
    'filter_corner'), as given and with the key removed: the filtered run's exported patterns are
    exactly 0 outside the model's kept set, the unfiltered run lights some of those pixels (what the
    parent commit did for the config as given), both loss histories are finite.  No accuracy bar:
    no reference test runs this config; the voxels-correct figures are printed."""
    from discretize_util import box_hole_reference
    from drtvam_amd.optimize import optimize
    cfg = json.load(open(os.path.join(GOLDEN, "box_hole_square_sparsity_loss.json")))
    cfg["target"]["filename"] = os.path.join(GOLDEN, "box_hole.ply")
    fc = cfg["filter_corner"]
    d = desc_from_config(cfg)
    pix = pm.dense_pixels(d)
    m = cm.corner_model(d, pix, fc["dist"], fc["radius"])
    assert m["undecided"].sum() <= 0.005 * len(pix)
    outside = np.ones(d.n_patterns * d.res_y * d.res_x, dtype=bool)
    outside[pix[m["keep"] | m["undecided"]]] = False
    assert outside.any()
    th = (cfg["loss"]["tl"] + cfg["loss"]["tu"]) / 2
    lit = {}
    for name in ("filtered", "unfiltered"):
        c = copy.deepcopy(cfg)
        if name == "unfiltered":
            del c["filter_corner"]
        c["output"] = str(tmp_path / name)
        vol = optimize(c, device=DEV).cpu().numpy()[..., 0]
        loss = np.load(tmp_path / name / "loss.npy")
        assert loss.size and np.all(np.isfinite(loss))
        pats = np.load(tmp_path / name / "patterns.npz")
        pats = pats[pats.files[0]].reshape(-1)
        assert pats.size == outside.size
        lit[name] = int(np.count_nonzero(pats[outside]))
        correct = np.mean(np.isclose(box_hole_reference(), vol > th)) * 100
        print(f"{name}: voxels correct {correct:.3f} %, loss {loss[0]:.4e} -> {loss[-1]:.4e}, "
              f"lit pixels outside the kept set {lit[name]} of {int(outside.sum())}")
    assert lit["filtered"] == 0
    assert lit["unfiltered"] > 0

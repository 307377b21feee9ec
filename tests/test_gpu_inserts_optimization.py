"""Optimisation through dielectric occluders on the GPU: the reference's overprinting scene
(tests/files/box_hole_occlusion.json, restated as configs.BOX_HOLE_OCCLUSION) with its occlusion.ply
made transparent, {"type": "dielectric", "int_ior": 1.58, "ext_ior": <the resin's IOR>}, judged as
tests/test_gpu_optimization.py judges the black piece: voxels at (tl + tu) / 2 against
box - piece - hole (no resin inside the piece: no dose there), at the reference's own bar of 97.0 %
(tests/test_optimization.py:99).  And the model matters: patterns optimised without the piece score
strictly lower when projected through the scene that has it."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from drtvam_amd.configs import BOX_HOLE_OCCLUSION
from drtvam_amd.optimize import TvamProblem, optimize

import insert_model as im
from discretize_util import box_hole_reference

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def transparent_config(out, piece=True):
    cfg = copy.deepcopy(BOX_HOLE_OCCLUSION)
    cfg["target"]["filename"] = os.path.join(GOLDEN, "box_hole.ply")
    cfg["output"] = str(out)
    if piece:
        cfg["vial"]["occlusions"] = [{"filename": os.path.join(GOLDEN, "occlusion.ply"),
                                      "bsdf": {"type": "dielectric", "int_ior": 1.58,
                                               "ext_ior": cfg["vial"]["medium"]["ior"]}}]
    else:
        del cfg["vial"]["occlusions"]
    return cfg


def score(cfg, vol):
    reference = np.zeros((50, 100, 100))
    reference[5:45, 10:90, 10:90] = 1
    piece = np.zeros((50, 100, 100))
    piece[15:35, 40:60, 30:70] = 1
    ref = (reference - piece - (reference - box_hole_reference())) > 0  # box - piece - hole
    th = (cfg["loss"]["tl"] + cfg["loss"]["tu"]) / 2
    return float(np.mean(np.isclose(ref, vol > th)) * 100)


def test_transparent_piece_optimization_and_the_model_matters(tmp_path):
    with_piece = transparent_config(tmp_path / "with")
    vol = optimize(with_piece, device="cuda:0").cpu().numpy()[..., 0]
    got = score(with_piece, vol)
    # the same optimisation with the piece left out of the scene, then its patterns projected (--forward_mode)
    # through the scene that has it
    blind = transparent_config(tmp_path / "blind", piece=False)
    optimize(blind, device="cuda:0")
    patterns = np.load(tmp_path / "blind" / "patterns.npz")["patterns"]
    through = transparent_config(tmp_path / "through")
    vol2 = optimize(through, patterns_fwd=patterns, device="cuda:0").cpu().numpy()[..., 0]
    got2 = score(through, vol2)
    print(f"percentage correct: optimised with the transparent piece {got:.3f}, optimised without it and projected "
          f"through it {got2:.3f}")
    assert got > 97.0
    assert got2 < got
    loss = np.load(tmp_path / "with" / "loss.npy")
    assert loss[-1] < loss[0]


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("insert_meshes")
    im.write_meshes(d)
    return d


def small_config(meshdir, out, **kw):
    cfg = im.insert_config("cylindrical", "collimated", False, inserts=("box",), black=True, paths=im.write_meshes(meshdir),
                           extinction=0.1)
    cfg |= {"output": str(out), "n_steps": 3, "spp": 2, "spp_ref": 2, "spp_grad": 2} | kw
    return cfg


def test_problem_is_a_3d_ray_scene(meshdir, tmp_path):
    from drtvam_amd._abi import FLAG_NO_ZERO_SKIP
    prob = TvamProblem(small_config(meshdir, tmp_path), device="cuda:0")
    assert prob.shard == "angle" and prob.proj.cone and not prob.proj.planar
    assert int(prob.proj.desc.flags) & FLAG_NO_ZERO_SKIP and len(prob.proj.desc.inserts) == 1
    with pytest.raises(ValueError, match="dielectric occluders.*shard 'angle'"):
        TvamProblem(small_config(meshdir, tmp_path, shard="slab", regular_sampling=True), device="cuda:0")
    with pytest.raises(NotImplementedError, match="filter_radon with dielectric occluders"):
        TvamProblem(small_config(meshdir, tmp_path, filter_radon=True), device="cuda:0")


def test_filter_corner_forward_mode_and_psf_analysis_run(meshdir, tmp_path):
    cfg = small_config(meshdir, tmp_path / "a", filter_corner={"dist": 2.26, "radius": 0.4})
    vol = optimize(cfg, device="cuda:0")
    assert float(vol.sum()) > 0 and (tmp_path / "a" / "patterns.npz").exists()
    # the default final render (max_depth_ref 16, rr_depth_ref 8) ran: Russian roulette is honoured, not refused
    patterns = np.load(tmp_path / "a" / "patterns.npz")["patterns"]
    vol2 = optimize(small_config(meshdir, tmp_path / "b"), patterns_fwd=patterns, device="cuda:0")
    assert vol2.shape == vol.shape and float(vol2.sum()) > 0
    cfg = small_config(meshdir, tmp_path / "c", psf_analysis=[{"index_pattern": 1, "x": 12, "y": 9, "intensity": 1.0}])
    out = optimize(cfg, device="cuda:0")
    assert float(out.sum()) > 0


def test_plan_cache_tells_a_moved_piece_apart(meshdir, tmp_path):
    """Two scenes whose inserts have the same triangle count and IORs but other vertices are two plans; the same
    scene asked twice is one."""
    from drtvam_amd.integrators import VolumeIntegrator
    from drtvam_amd.optimize import load_scene
    from drtvam_amd.scene import load_dict
    paths = im.write_meshes(meshdir)
    integ = VolumeIntegrator({"regular_sampling": True, "max_depth": 8, "rr_depth": 8})
    projs = []
    for name in ("box", "far", "box"):
        cfg = im.insert_config("cylindrical", "collimated", True, inserts=(name,), paths=paths)
        cfg["projector"]["device"] = "cuda:0"
        scene = load_dict(load_scene(cfg))
        projs.append(integ.projection(scene, scene.sensor_by_id("sensor")))
    assert len(im.mesh("box")) == len(im.mesh("far"))
    assert projs[0] is projs[2] and projs[0] is not projs[1]
    assert np.array_equal(projs[1].desc.inserts[0][0], im.mesh("far"))

"""Optimisation with transmission_only = false on the GPU: the reference's square-cuvette scene
(tests/files/box_hole_square.json, restated as configs.BOX_HOLE_SQUARE) with reflections sampled at
the glass, judged as tests/test_gpu_optimization.py judges the transmission-only run and held to the
bar the reference grants its stochastic-path scenes (test_optimization.py:152-155): more than 99.0 %.
And the optimiser's side of a reflecting scene: angle shards only, filter_radon refused by name,
filter_corner, --forward_mode, psf_analysis and the final render at max_depth_ref 16 / rr_depth_ref 8."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from drtvam_amd.configs import BOX_HOLE_SQUARE
from drtvam_amd.optimize import TvamProblem, optimize

import insert_model as im
import reflect_model as rm
from discretize_util import box_hole_reference

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_box_hole_square_optimization_with_reflections(tmp_path):
    cfg = copy.deepcopy(BOX_HOLE_SQUARE)
    cfg["target"]["filename"] = os.path.join(GOLDEN, "box_hole.ply")
    cfg["output"] = str(tmp_path)
    cfg["transmission_only"] = False
    vol = optimize(cfg, device="cuda:0").cpu().numpy()[..., 0]
    th = (cfg["loss"]["tl"] + cfg["loss"]["tu"]) / 2
    correct = np.mean(np.isclose(box_hole_reference(), vol > th)) * 100
    print("percentage correct", correct)
    assert correct > 99.0
    loss = np.load(tmp_path / "loss.npy")
    assert loss[-1] < loss[0]


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("reflect_meshes")
    im.write_meshes(d)
    return d


def small_config(meshdir, out, **kw):
    cfg = rm.reflect_config("cylindrical", "collimated", False, inserts=("box",), black=True,
                            paths=im.write_meshes(meshdir), extinction=0.1)
    cfg |= {"output": str(out), "n_steps": 3, "spp": 2, "spp_ref": 2, "spp_grad": 2} | kw
    return cfg


def test_problem_is_a_3d_ray_scene(meshdir, tmp_path):
    from drtvam_amd._abi import FLAG_NO_ZERO_SKIP
    prob = TvamProblem(small_config(meshdir, tmp_path), device="cuda:0")
    assert prob.shard == "angle" and prob.proj.cone and not prob.proj.planar and prob.proj.desc.reflected
    assert int(prob.proj.desc.flags) & FLAG_NO_ZERO_SKIP
    # without inserts too, and for a collimated projector under regular sampling: no planar kernels
    plain = small_config(meshdir, tmp_path, regular_sampling=True)
    del plain["vial"]["occlusions"]
    prob = TvamProblem(plain, device="cuda:0")
    assert prob.shard == "angle" and prob.proj.cone and not prob.proj.planar and not prob.proj.desc.inserts
    # (with inserts the inserts' own refusals come first: tests/test_gpu_inserts_optimization.py)
    with pytest.raises(ValueError, match="transmission_only = false.*shard 'angle'"):
        TvamProblem(plain | {"shard": "slab"}, device="cuda:0")
    with pytest.raises(NotImplementedError, match="filter_radon with transmission_only = false"):
        TvamProblem(plain | {"filter_radon": True}, device="cuda:0")
    with pytest.raises(ValueError, match="dielectric occluders.*shard 'angle'"):
        TvamProblem(small_config(meshdir, tmp_path, shard="slab", regular_sampling=True), device="cuda:0")


def test_filter_corner_forward_mode_and_psf_analysis_run(meshdir, tmp_path):
    cfg = small_config(meshdir, tmp_path / "a", filter_corner={"dist": 2.26, "radius": 0.4})
    vol = optimize(cfg, device="cuda:0")
    assert float(vol.sum()) > 0 and (tmp_path / "a" / "patterns.npz").exists()
    # patterns of a transmission-only run projected (--forward_mode) through the reflecting scene; the default final
    # render (max_depth_ref 16, rr_depth_ref 8) runs with the roulette acting
    optimize(small_config(meshdir, tmp_path / "t", transmission_only=True), device="cuda:0")
    patterns = np.load(tmp_path / "t" / "patterns.npz")["patterns"]
    vol2 = optimize(small_config(meshdir, tmp_path / "b"), patterns_fwd=patterns, device="cuda:0")
    assert vol2.shape == vol.shape and float(vol2.sum()) > 0
    cfg = small_config(meshdir, tmp_path / "c", psf_analysis=[{"index_pattern": 1, "x": 12, "y": 9, "intensity": 1.0}])
    out = optimize(cfg, device="cuda:0")
    assert float(out.sum()) > 0

"""End-to-end optimisation with the telecentric and lens projectors.

The index-matched box-with-hole config of test_gpu_optimization.py's first test
(tests/files/box_hole_index_matched.json of the reference) with "type": "telecentric",
aperture_radius 0.001 and focus_distance = distance: at that etendue the beam radius across the
film (aperture_radius * |1 - s / F| <= 0.001 * 2.5 / 20 mm over the 5 mm film) stays below 1 / 50 of
the 0.05 mm voxel, so the collimated run's bar applies: > 99.4 % of the voxels thresholded at
(tl + tu) / 2 match the voxelised reference.  A lens config of the same pixel size at the focus
plane runs the same loop, and both run under two-rank angle sharding (test_gpu_distributed.py's
pattern: two ranks on the one GPU, gloo), where the sharded run must reproduce the single-rank one."""
import copy
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from drtvam_amd.configs import BOX_HOLE_INDEX_MATCHED
from drtvam_amd.optimize import optimize

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from discretize_util import box_hole_reference  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def box_hole_config(kind, tmp_path=None):
    cfg = copy.deepcopy(BOX_HOLE_INDEX_MATCHED)
    proj = cfg["projector"]
    proj["type"] = kind
    proj["aperture_radius"] = 0.001
    proj["focus_distance"] = proj["distance"]
    cfg["target"]["filename"] = os.path.join(GOLDEN, "box_hole.ply")
    if tmp_path is not None:
        cfg["output"] = str(tmp_path)
    return cfg


def test_box_hole_telecentric_optimization(tmp_path):
    cfg = box_hole_config("telecentric", tmp_path)
    vol = optimize(cfg, device="cuda:0").cpu().numpy()[..., 0]
    th = (cfg["loss"]["tl"] + cfg["loss"]["tu"]) / 2
    correct = np.mean(np.isclose(box_hole_reference(), vol > th)) * 100
    print("percentage correct", correct)
    assert correct > 99.4
    loss = np.load(tmp_path / "loss.npy")
    assert loss[-1] < 0.05 * loss[0]
    assert (tmp_path / "patterns.npz").exists() and (tmp_path / "final.npy").exists()


def test_box_hole_lens_optimization(tmp_path):
    """The lens form of the same projector: pixel_size is the pixel at the focus plane (the film
    centre), and the film spans s / focus_distance in [0.875, 1.125].  24 DMD rows instead of 20,
    so that the image still covers the target's height (1 mm) on the near side of the film
    (24 * 0.05 * 0.875 = 1.05 mm).  The run must converge like the collimated one (the loss falls
    to a twentieth) and meet the lowest bar the reference holds a box_hole config to (97 %,
    test_optimization.py:43-99): the collimated 99.4 % does not carry over, the magnification
    changes the pixel footprint by an eighth across the film."""
    cfg = box_hole_config("lens", tmp_path)
    cfg["projector"]["resy"] = 24
    vol = optimize(cfg, device="cuda:0").cpu().numpy()[..., 0]
    th = (cfg["loss"]["tl"] + cfg["loss"]["tu"]) / 2
    correct = np.mean(np.isclose(box_hole_reference(), vol > th)) * 100
    loss = np.load(tmp_path / "loss.npy")
    print("percentage correct", correct, "loss ratio", loss[-1] / loss[0])
    assert loss[-1] < 0.05 * loss[0]
    assert correct > 97.0


def test_slab_sharding_and_filter_radon_are_refused():
    from drtvam_amd.optimize import TvamProblem
    cfg = box_hole_config("telecentric")
    cfg["shard"] = "slab"
    with pytest.raises(ValueError, match="leave their slice"):
        TvamProblem(cfg, device=torch.device("cuda", 0))
    cfg = box_hole_config("lens")
    cfg["filter_radon"] = True
    with pytest.raises(NotImplementedError, match="filter_radon"):
        TvamProblem(cfg, device=torch.device("cuda", 0))


# --------------------------------------------------------------------------- two ranks, one GPU
def _run(rank, world, steps, kind):
    from drtvam_amd.optimize import TvamProblem
    cfg = box_hole_config(kind)
    cfg["projector"] |= {"n_patterns": 12, "resx": 40, "resy": 8, "pixel_size": 0.125, "aperture_radius": 1.0}
    cfg["sensor"]["film"] = {"type": "vfilm", "resx": 24, "resy": 24, "resz": 10}
    cfg["target"] = {"analytic": "box_hole"}
    cfg["progressive"] = False
    cfg["spp"] = 2
    prob = TvamProblem(cfg, device=torch.device("cuda", 0), rank=rank, world_size=world)
    assert prob.shard == "angle" and prob.proj.cone  # 'auto': never slab for 3-D projector rays
    g = torch.Generator().manual_seed(0)
    prob.x0 = prob.local_from_global(torch.rand(prob.n_global, generator=g) * 0.1)
    for i in range(steps):
        prob.iteration(i)
    x = prob.gather_patterns(prob.patterns_local().float())
    dose = prob.final_render(spp=2)
    return np.asarray(prob.loss_hist), x.cpu().numpy(), dose.cpu().numpy()


def _worker(rank, world, port, steps, kind, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = _run(rank, world, steps, kind)
        if rank == 0:
            q.put(res)
    except BaseException:  # report instead of leaving the parent waiting
        import traceback
        q.put(("error", rank, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("kind", ["telecentric", "lens"])
def test_two_rank_angle_sharding_matches_single_rank(kind):
    steps = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()

    def result(procs):
        try:
            res = q.get(timeout=240)
        finally:
            for p in procs:
                p.join(timeout=60)
                if p.is_alive():
                    p.kill()
        assert not (isinstance(res[0], str) and res[0] == "error"), res[2]
        assert all(p.exitcode == 0 for p in procs)
        return res

    p1 = ctx.Process(target=_worker, args=(0, 1, _free_port(), steps, kind, q))
    p1.start()
    ref_loss, ref_x, ref_dose = result([p1])
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, steps, kind, q)) for r in range(2)]
    for p in procs:
        p.start()
    loss, x, dose = result(procs)
    assert ref_loss[-1] < ref_loss[0]
    # the same sums in a different order (partial doses): fp32 rounding only
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    np.testing.assert_allclose(x, ref_x, rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(dose, ref_dose, rtol=1e-3, atol=1e-6)

"""End-to-end optimisation behind a 'custom' vial: the reference's box_hole_custom_cuvette case
(tests/files/box_hole_custom_cuvette.json, restated as configs.BOX_HOLE_CUSTOM_CUVETTE) -- the
telecentric projector through the rectangular glass cuvette of tests/golden/cuvette_*.ply, the
box-with-hole target -- held to the reference's own bar (test_optimization.py:152-153): more than
99.0 % of the voxels thresholded at (tl + tu) / 2 match the voxelised target."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from drtvam_amd.configs import BOX_HOLE_CUSTOM_CUVETTE
from drtvam_amd.optimize import optimize

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from discretize_util import box_hole_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def cuvette_config(out=None):
    cfg = copy.deepcopy(BOX_HOLE_CUSTOM_CUVETTE)
    cfg["vial"]["filename_vial_outer"] = os.path.join(GOLDEN, "cuvette_outer.ply")
    cfg["vial"]["filename_vial_inner"] = os.path.join(GOLDEN, "cuvette_inner.ply")
    cfg["target"]["filename"] = os.path.join(GOLDEN, "box_hole.ply")
    if out is not None:
        cfg["output"] = str(out)
    return cfg


def test_box_hole_custom_cuvette_optimization(tmp_path):
    cfg = cuvette_config(tmp_path)
    vol = optimize(cfg, device="cuda:0").cpu().numpy()[..., 0]
    th = (cfg["loss"]["tl"] + cfg["loss"]["tu"]) / 2
    correct = np.mean(np.isclose(box_hole_reference(), vol > th)) * 100
    loss = np.load(tmp_path / "loss.npy")
    print("percentage correct", correct, "loss", loss[0], "->", loss[-1])
    assert correct > 99.0
    assert loss[-1] < 0.05 * loss[0]
    assert (tmp_path / "patterns.npz").exists() and (tmp_path / "final.npy").exists()


def test_custom_vial_refuses_slab_shards_and_filter_radon():
    cfg = cuvette_config()
    with pytest.raises(ValueError, match="a 'custom' vial's rays"):
        optimize(cfg | {"shard": "slab", "regular_sampling": True}, device="cuda:0")
    with pytest.raises(NotImplementedError, match="filter_radon with a 'custom' vial"):
        optimize(cfg | {"filter_radon": True}, device="cuda:0")


def test_command_line_runs_a_custom_vial_config(tmp_path):
    """python -m drtvam_amd.optimize on a JSON config that names a custom vial (a short run: the
    command line is what this test is about)."""
    cfg = cuvette_config(tmp_path / "out")
    cfg["n_steps"] = 3
    cfg["projector"]["n_patterns"] = 40
    path = tmp_path / "cuvette.json"
    path.write_text(json.dumps(cfg))
    r = subprocess.run([sys.executable, "-m", "drtvam_amd.optimize", str(path)], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    loss = np.load(tmp_path / "out" / "loss.npy")
    assert loss.size == 3 and np.all(np.isfinite(loss)) and loss[-1] < loss[0]

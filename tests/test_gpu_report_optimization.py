"""GPU: optimize() ends with the print report (optimize.py:362-366 of the reference): histogram.npz and
report.json next to final.npy, equal to the model of tests/report_model.py evaluated on the run's
own final.npy and target, for an optimisation, a forward-mode run and a surface-aware run (whose
report compares with target_binary.npy).  The config is tests/files/box_hole_index_matched.json cut
to 40 angles, a 50 x 50 x 25 film and 3 steps."""
import copy
import json
import os

import numpy as np
import pytest

import report_model as rm
from drtvam_amd.configs import BOX_HOLE_INDEX_MATCHED
from drtvam_amd.optimize import optimize

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _config(out):
    cfg = copy.deepcopy(BOX_HOLE_INDEX_MATCHED)
    cfg["target"]["filename"] = os.path.join(GOLDEN, "box_hole.ply")
    cfg["projector"]["n_patterns"] = 40
    cfg["sensor"]["film"].update(resx=50, resy=50, resz=25)
    cfg["n_steps"] = 3
    cfg["output"] = str(out)
    return cfg


def _check(out, printed, target_file):
    """The report files against the model on the run's own outputs; the printed lines."""
    final = np.load(os.path.join(out, "final.npy"))
    target = np.load(os.path.join(out, target_file))
    assert final.shape == target.shape == (25, 50, 50, 1)
    pats = np.load(os.path.join(out, "patterns.npz"))["patterns"]
    h, rep = rm.check_report_files(out, final, target, max_intensity=float(pats.max()))
    lines = printed.splitlines()
    assert "Pattern efficiency {:.4f}".format(rep["efficiency"]) in lines
    assert rep["efficiency"] == float(np.sum(pats / pats.max() / pats.size))
    assert "Best IoU: {:.4f}".format(rep["best_iou"]) in lines
    assert "Best threshold: {:4f}".format(rep["best_threshold"]) in lines
    assert lines.index("Pattern efficiency {:.4f}".format(rep["efficiency"])) < lines.index(
        "Best IoU: {:.4f}".format(rep["best_iou"]))
    assert rep["n_object"] == int((target > 0).sum()) > 0
    assert h["object"].sum() + h["above"][1] + h["nan"][1] + h["below"][1] == rep["n_object"]
    return rep


def test_optimisation_and_forward_mode_write_the_report(tmp_path, capsys):
    cfg = _config(tmp_path / "opt")
    vol = optimize(cfg, device="cuda:0")
    rep = _check(tmp_path / "opt", capsys.readouterr().out, "target.npy")
    np.testing.assert_array_equal(vol.cpu().numpy(), np.load(tmp_path / "opt" / "final.npy"))
    assert 0.0 < rep["best_iou"] <= 1.0
    # --forward_mode: the saved patterns rendered again, the same report
    pats = np.load(tmp_path / "opt" / "patterns.npz")["patterns"]
    fwd = _config(tmp_path / "fwd")
    optimize(fwd, patterns_fwd=pats, device="cuda:0")
    rep_fwd = _check(tmp_path / "fwd", capsys.readouterr().out, "target.npy")
    assert rep_fwd["efficiency"] == rep["efficiency"]
    # all patterns zero: no efficiency line today, and no report
    zero = _config(tmp_path / "zero")
    optimize(zero, patterns_fwd=np.zeros_like(pats), device="cuda:0")
    out = capsys.readouterr().out
    assert "Pattern efficiency" not in out and "Best IoU" not in out and "All patterns are zero" in out
    assert not (tmp_path / "zero" / "report.json").exists() and (tmp_path / "zero" / "final.npy").exists()


def test_surface_aware_run_reports_against_target_binary(tmp_path, capsys):
    cfg = _config(tmp_path)
    cfg["final_sensor"] = copy.deepcopy(cfg["sensor"])
    cfg["sensor"]["film"]["surface_aware"] = True
    optimize(cfg, device="cuda:0")
    assert np.load(tmp_path / "target.npy").shape == (25, 50, 50, 2)  # the fractional volumes: not the report's target
    _check(tmp_path, capsys.readouterr().out, "target_binary.npy")


def test_final_sensor_of_another_resolution(tmp_path, capsys):
    """A final sensor finer than the optimisation's: the report's target is discretised on its grid."""
    cfg = _config(tmp_path)
    cfg["final_sensor"] = copy.deepcopy(cfg["sensor"])
    cfg["sensor"]["film"].update(resx=25, resy=25, resz=13)
    cfg["n_steps"] = 1
    optimize(cfg, device="cuda:0")
    from drtvam_amd.optimize import TvamProblem
    from drtvam_amd.utils import discretize
    prob = TvamProblem(copy.deepcopy(cfg), device="cuda:0")
    target = discretize(prob.scene, sensor=prob.final_sensor).numpy()
    final = np.load(tmp_path / "final.npy")
    assert final.shape == target.shape == (25, 50, 50, 1) and np.load(tmp_path / "target.npy").shape == (13, 25, 25, 1)
    pats = np.load(tmp_path / "patterns.npz")["patterns"]
    rm.check_report_files(tmp_path, final, target, max_intensity=float(pats.max()))
    assert json.load(open(tmp_path / "report.json"))["n_object"] == int((target > 0).sum())

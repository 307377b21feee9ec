"""The print report without a GPU: the torch path of engine.class_hist, utils.iou_sweep and
utils.save_histogram on CPU tensors against the model of tests/report_model.py (the reference's
300-pass sweep and searchsorted + bincount).  Counts are compared for equality and the IoU array bit
for bit."""
import json
import sys

import numpy as np
import pytest
import torch

import report_model as rm
from drtvam_amd import engine, utils


def _volume(seed=0, n=24 ** 3, nan=True):
    """A bimodal dose around tl / tu with mistakes on both sides, a 20 % object target whose void
    values are 0, -0, -1 and whose object values are 1 and 0.5, and NaN doses in both classes."""
    rng = np.random.default_rng(seed)
    obj = rng.random(n) < 0.2
    x = np.where(obj, rng.normal(0.97, 0.05, n), rng.normal(0.80, 0.10, n)).astype(np.float32)
    t = np.where(obj, rng.choice(np.float32([1.0, 0.5]), n), rng.choice(np.float32([0.0, -0.0, -1.0]), n))
    if nan:
        x[np.flatnonzero(obj)[:2]] = np.nan
        x[np.flatnonzero(~obj)[:3]] = np.nan
    return x, t.astype(np.float32)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n_edges", [1, 2, 300, 501, 2048])
def test_torch_class_hist_equals_model(n_edges, side):
    edges = np.linspace(0, 1.3, n_edges).astype(np.float32) if n_edges > 1 else np.float32([0.9])
    x, t = _volume(n_edges)
    x = np.concatenate([x, rm.special_values(edges)])
    t = np.concatenate([t, np.resize(np.float32([1.0, 0.0, 0.5, -1.0, -0.0]), x.size - t.size)])
    got = engine.class_hist(torch.from_numpy(x), torch.from_numpy(t), edges, side)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, n_edges + 2)
    np.testing.assert_array_equal(got.numpy(), rm.class_hist(x, t, edges, side))
    assert int(got.sum()) == x.size


def test_torch_class_hist_empty_and_invalid():
    z = torch.zeros(0)
    assert not engine.class_hist(z, z, np.float32([0.0, 1.0]), 0).any()
    x = torch.zeros(4)
    for edges, side, msg in (([0.5, 0.25], 0, "strictly increasing"), ([0.5, 0.5], 0, "strictly increasing"),
                             ([0.0, np.nan], 0, "edge 1 is not finite"), ([], 0, "1 <= n_edges <= 2048"),
                             (np.arange(2049), 0, "1 <= n_edges <= 2048"), ([0.0, 1.0], 2, "side must be 0 or 1")):
        with pytest.raises(ValueError, match=msg):
            engine.class_hist(x, x, np.asarray(edges, np.float32), side)


def test_library_refuses_before_it_touches_the_runtime():
    """tvam_class_hist validates on the host: every refusal returns TVAM_ERR_INVALID with its cause
    in a process without a GPU."""
    from drtvam_amd import _abi
    lib = _abi.load_library()
    x = np.zeros(8, np.float32)      # host memory: never read, the call is refused first
    counts = np.zeros(2 * 2051, np.uint64)

    def call(edges, n_edges, side, xp=x.ctypes.data, cp=counts.ctypes.data):
        e = np.asarray(edges, np.float32)
        rc = lib.tvam_class_hist(xp, xp, 8, e.ctypes.data if edges is not None else None, n_edges, side, cp, None)
        return rc, lib.tvam_last_error().decode()

    for args, msg in (((None, 3, 0), "null argument"), (([0.0, 1.0], 2, 0, None), "null argument"),
                      (([0.0, 1.0], 2, 0, x.ctypes.data, None), "null argument"),
                      (([0.0, 1.0], 0, 0), "1 <= n_edges <= 2048 (got 0)"),
                      ((np.arange(2049), 2049, 0), "1 <= n_edges <= 2048 (got 2049)"),
                      (([0.0, 1.0], 2, -1), "side must be 0 or 1 (got -1)"),
                      (([0.0, 1.0, 1.0], 3, 1), "edges must be strictly increasing (edge 2 <= edge 1)"),
                      (([1.0, 0.0], 2, 0), "edges must be strictly increasing (edge 1 <= edge 0)"),
                      (([0.0, -np.inf], 2, 0), "edge 1 is not finite"), (([np.nan], 1, 0), "edge 0 is not finite")):
        rc, err = call(*args)
        assert rc == _abi.TVAM_ERR_INVALID and err == "tvam_class_hist: " + msg, (args, rc, err)


def test_iou_sweep_equals_the_300_pass_model():
    x, t = _volume(1)
    got = utils.iou_sweep(torch.from_numpy(x), torch.from_numpy(t))
    iou, best = rm.iou_sweep(x, t)
    assert got["iou"].dtype == np.float32
    np.testing.assert_array_equal(got["thresholds"], rm.THRESHOLDS)
    np.testing.assert_array_equal(got["iou"].view(np.uint32), iou.view(np.uint32))
    assert got["best_index"] == best and 0 < best < 299
    assert got["best_threshold"] == float(rm.THRESHOLDS[best]) and got["best_iou"] == float(iou[best])
    obj = t > 0
    assert got["n_object"] == int(obj.sum()) and got["n_empty"] == int((~obj).sum())
    # numpy inputs and a volume-shaped tensor give the same
    again = utils.iou_sweep(x.reshape(24, 24, 24, 1), t.reshape(24, 24, 24, 1))
    np.testing.assert_array_equal(again["iou"].view(np.uint32), iou.view(np.uint32))


def test_iou_sweep_tie_takes_the_first_threshold():
    """Doses on two values only: the IoU is constant between them, a plateau of equal maxima; the
    reference's np.argmax takes its first threshold."""
    t = np.float32([1, 1, 1, 0, 0, 0, 0, 1])
    x = np.float32([0.9, 0.9, 0.9, 0.5, 0.5, 0.5, 0.9, 0.5])
    got = utils.iou_sweep(torch.from_numpy(x), torch.from_numpy(t))
    iou, best = rm.iou_sweep(x, t)
    np.testing.assert_array_equal(got["iou"].view(np.uint32), iou.view(np.uint32))
    assert np.count_nonzero(iou == iou.max()) > 1
    assert got["best_index"] == best == int(np.flatnonzero(iou == iou.max())[0])
    assert rm.THRESHOLDS[best - 1] < np.float32(0.5) <= rm.THRESHOLDS[best]
    # a user's own thresholds, two of them with the same IoU
    got = utils.iou_sweep(x, t, thresholds=[0.1, 0.6, 0.7, 0.95])
    np.testing.assert_array_equal(got["iou"], np.float32([0.5, 0.6, 0.6, 0.0]))
    assert got["best_index"] == 1 and got["best_threshold"] == float(np.float32(0.6))


def test_empty_union_gives_zero():
    x = np.full(10, 0.5, np.float32)
    got = utils.iou_sweep(x, np.zeros(10, np.float32))
    iou, best = rm.iou_sweep(x, np.zeros(10, np.float32))
    assert got["iou"][-1] == 0.0 and not got["iou"][rm.THRESHOLDS >= 0.5].any()
    np.testing.assert_array_equal(got["iou"], iou)
    got = utils.iou_sweep(np.full(10, -1.0, np.float32), np.zeros(10, np.float32))  # empty at every threshold
    assert not got["iou"].any() and got["best_index"] == 0 and got["best_iou"] == 0.0 and got["n_object"] == 0


def test_save_histogram_files_match_the_model(tmp_path, capsys, monkeypatch):
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # import matplotlib raises ImportError
    x, t = _volume(2)
    x[:3] = [-0.25, 1.3, 7.0]  # below the first edge, on the last edge, far above
    png = tmp_path / "out" / "histogram.png"
    rep = utils.save_histogram(torch.from_numpy(x).reshape(24, 24, 24, 1), torch.from_numpy(t).reshape(24, 24, 24, 1),
                               str(png), 0.125, 2.5)
    h, on_disk = rm.check_report_files(tmp_path / "out", x, t, efficiency=0.125, max_intensity=2.5)
    assert on_disk == json.loads(json.dumps(rep)) and not png.exists()
    assert set(on_disk) == {"best_iou", "best_threshold", "best_threshold_normalized", "efficiency", "n_object",
                            "n_empty"}
    assert h["object"].shape == h["empty"].shape == (500,) and h["above"].sum() == 2
    total = h["object"].sum() + h["empty"].sum() + h["above"].sum() + h["nan"].sum() + h["below"].sum()
    assert total == x.size and h["below"].sum() >= 1
    iou, best = rm.iou_sweep(x, t)
    lines = capsys.readouterr().out.splitlines()
    assert "Best IoU: {:.4f}".format(iou[best]) in lines
    assert "Best threshold: {:4f}".format(rm.THRESHOLDS[best]) in lines


def test_save_histogram_plots_when_matplotlib_is_there(tmp_path):
    """The PNG is best effort: written with matplotlib, and no error without it."""
    try:
        import matplotlib  # noqa: F401
        have = True
    except ImportError:
        have = False
    x, t = _volume(3, nan=False)
    utils.save_histogram(x, t, str(tmp_path / "histogram.png"), 0.5, 1.0)
    assert (tmp_path / "histogram.npz").exists() and (tmp_path / "report.json").exists()
    assert (tmp_path / "histogram.png").exists() == have

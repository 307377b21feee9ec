"""Model of the print report (drtvam_amd/utils.py: iou_sweep, save_histogram; engine.class_hist): the
reference's own method in numpy.  The IoU sweep is one compare / and / or / count pass over the
volume per threshold (utils.py:8-11, :59-62); the class-split histogram is np.searchsorted +
np.bincount per class with the NaN doses masked out first.  Everything is an integer count or the
fp32 quotient of two: the tests compare for equality."""
import numpy as np

THRESHOLDS = np.linspace(0, 1.3, 300).astype(np.float32)   # utils.py:59 as the fp32 compare sees them
HIST_EDGES = np.linspace(0, 1.3, 501).astype(np.float32)   # save_histogram's fixed bins


def class_hist(x, target, edges, side):
    """int64 [2, n_edges + 2]: row = target > 0, column = searchsorted slot ('left' for side 0,
    'right' for side 1), last column = NaN entries of x."""
    x = np.asarray(x, np.float32).reshape(-1)
    obj = np.asarray(target).reshape(-1) > 0
    edges = np.asarray(edges, np.float32)
    k = edges.size
    nan = np.isnan(x)
    out = np.zeros((2, k + 2), np.int64)
    for c in (0, 1):
        m = obj == bool(c)
        j = np.searchsorted(edges, x[m & ~nan], side="left" if side == 0 else "right")
        out[c, :k + 1] = np.bincount(j, minlength=k + 1)
        out[c, k + 1] = np.count_nonzero(m & nan)
    return out


def iou_sweep(x, target, thresholds=THRESHOLDS):
    """One pass per threshold: (iou float32 [n], index of the first maximum)."""
    x = np.asarray(x, np.float32).reshape(-1)
    obj = np.asarray(target).reshape(-1) > 0
    iou = np.zeros(len(thresholds), np.float32)
    for k, t in enumerate(np.asarray(thresholds, np.float32)):
        th = x > t
        union = np.count_nonzero(th | obj)
        if union:
            iou[k] = np.float32(np.count_nonzero(th & obj)) / np.float32(union)
    return iou, int(np.argmax(iou))


def histogram(x, target, edges=HIST_EDGES):
    """save_histogram's arrays: object, empty [n_edges - 1] (half-open bins), above, nan [2] = (empty, object)."""
    c = class_hist(x, target, edges, 1)
    k = len(edges)
    return {"object": c[1, 1:k], "empty": c[0, 1:k], "above": c[:, k], "nan": c[:, k + 1]}


def special_values(edges):
    """Every edge, its fp32 neighbours, +-0, a denormal of either sign, +-inf and NaN."""
    e = np.asarray(edges, np.float32)
    tiny = np.float32(1e-45)
    extra = np.array([0.0, -0.0, tiny, -tiny, np.float32(1e-39), np.inf, -np.inf, np.nan, np.nan], np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf)), extra])


def check_report_files(out_dir, x, target, efficiency=None, max_intensity=None):
    """histogram.npz and report.json of out_dir against the model on (x, target)."""
    import json
    import os
    h = np.load(os.path.join(out_dir, "histogram.npz"))
    rep = json.load(open(os.path.join(out_dir, "report.json")))
    iou, best = iou_sweep(x, target)
    np.testing.assert_array_equal(h["thresholds"], THRESHOLDS)
    np.testing.assert_array_equal(h["edges"], HIST_EDGES)
    assert h["iou"].dtype == np.float32
    np.testing.assert_array_equal(h["iou"].view(np.uint32), iou.view(np.uint32))
    for name, want in histogram(x, target).items():
        np.testing.assert_array_equal(h[name], want, err_msg=name)
    obj = np.asarray(target).reshape(-1) > 0
    assert rep["best_threshold"] == float(THRESHOLDS[best])
    assert rep["best_iou"] == float(iou[best])
    assert rep["n_object"] == int(obj.sum()) and rep["n_empty"] == int((~obj).sum())
    if efficiency is not None:
        assert rep["efficiency"] == float(efficiency)
    if max_intensity is not None:
        assert rep["best_threshold_normalized"] == float(THRESHOLDS[best]) / float(max_intensity)
    return h, rep

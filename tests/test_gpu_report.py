"""GPU: tvam_class_hist (engine.class_hist on CUDA tensors) and the report built on it
(utils.iou_sweep, utils.save_histogram) against the model of tests/report_model.py, the reference's
method in numpy.  Every count is compared for equality.

The shapes are the smallest at which the kernel can go wrong: sizes around the wave, the workgroup
and the float4 grid at every (x, target) offset from the 16-byte grid, the edge counts at which
the search length and the number of LDS counter copies change (1, 2, 300, 501; 2048: one copy per
wave pair), values on and next to every edge, and at 2^20 + 3 entries (more than one workgroup,
every workgroup's flush) the inputs that load the LDS counters most."""
import json

import numpy as np
import pytest
import torch

import report_model as rm
from drtvam_amd import engine, utils

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BIG = 2 ** 20 + 3
TARGET_VALUES = np.float32([0.0, 1.0, 0.5, -1.0, -0.0])


def _views(x, t, ox, ot):
    """x and t as views ox / ot floats into larger CUDA tensors (whose storage is 16-byte aligned)."""
    bx = torch.zeros(x.size + 8, dtype=torch.float32, device=DEV)
    bt = torch.zeros(t.size + 8, dtype=torch.float32, device=DEV)
    assert bx.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0
    vx, vt = bx[ox:ox + x.size], bt[ot:ot + t.size]
    vx.copy_(torch.from_numpy(x))
    vt.copy_(torch.from_numpy(t))
    return vx, vt


def _mixed(n, seed):
    """Doses over and beyond the edge range with special values among them, all five target values."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.5, n).astype(np.float32)
    sp = rm.special_values(rm.THRESHOLDS[::37])
    if n >= 64:
        pos = rng.choice(n, min(sp.size, n // 2), replace=False)
        x[pos] = sp[:pos.size]
    return x, rng.choice(TARGET_VALUES, n)


_ref_cache = {}


def _reference(n):
    """(x, target, model counts for side 0 over THRESHOLDS, for side 1 over HIST_EDGES), computed once."""
    if n not in _ref_cache:
        x, t = _mixed(n, n)
        _ref_cache[n] = (x, t, rm.class_hist(x, t, rm.THRESHOLDS, 0), rm.class_hist(x, t, rm.HIST_EDGES, 1))
    return _ref_cache[n]


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 4099, BIG])
def test_sizes_and_alignment(n):
    x, t, want0, want1 = _reference(n)
    for ox, ot in ((0, 0), (1, 1), (1, 2), (3, 0)):
        vx, vt = _views(x, t, ox, ot)
        got0 = engine.class_hist(vx, vt, rm.THRESHOLDS, 0)
        got1 = engine.class_hist(vx, vt, rm.HIST_EDGES, 1)
        assert got0.dtype == torch.int64 and tuple(got0.shape) == (2, 302) and got0.device == vx.device
        np.testing.assert_array_equal(got0.cpu().numpy(), want0, err_msg=f"side 0, offsets {ox}, {ot}")
        np.testing.assert_array_equal(got1.cpu().numpy(), want1, err_msg=f"side 1, offsets {ox}, {ot}")


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n_edges", [1, 2, 300, 501, 2048])
def test_edge_counts_and_special_values(n_edges, side):
    """Every edge itself, its two fp32 neighbours, +-0, denormals, +-inf and NaN (in both classes)
    among 4099 random doses."""
    edges = np.linspace(0, 1.3, n_edges).astype(np.float32) if n_edges > 1 else np.float32([0.0])
    rng = np.random.default_rng(n_edges)
    x = np.concatenate([rm.special_values(edges), rng.uniform(-0.2, 1.5, 4099).astype(np.float32)])
    t = np.resize(TARGET_VALUES, x.size)
    nan = np.isnan(x)
    t[np.flatnonzero(nan)] = [1.0, -1.0]  # one NaN dose in each class
    assert (nan & (t > 0)).any() and (nan & ~(t > 0)).any()
    want = rm.class_hist(x, t, edges, side)
    got = engine.class_hist(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), edges, side).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert got.sum() == x.size and got[:, -1].sum() == nan.sum()
    # the torch path on the same data: one definition on both devices
    np.testing.assert_array_equal(engine.class_hist(torch.from_numpy(x), torch.from_numpy(t), edges, side).numpy(), want)


def test_zero_signs_denormals_and_infinities():
    """Spelled out, edges (0, 1): -0 sits where +0 does, a denormal above 0 is above it (no flush
    in the compare), +-inf take the end slots, NaN takes none."""
    tiny = np.float32(1e-45)
    x = np.float32([0.0, -0.0, tiny, -tiny, np.inf, -np.inf, np.nan, 1.0])
    t = np.ones(8, np.float32)
    dx, dt = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    # side 0, #{e < x}: 0, -0, -tiny, -inf -> 0; tiny, 1 -> 1; inf -> 2
    np.testing.assert_array_equal(engine.class_hist(dx, dt, [0.0, 1.0], 0).cpu().numpy(), [[0, 0, 0, 0], [4, 2, 1, 1]])
    # side 1, #{e <= x}: -tiny, -inf -> 0; 0, -0, tiny -> 1; 1, inf -> 2
    np.testing.assert_array_equal(engine.class_hist(dx, dt, [0.0, 1.0], 1).cpu().numpy(), [[0, 0, 0, 0], [2, 3, 2, 1]])


def test_target_class_is_target_above_zero():
    t = np.float32([0.0, 1.0, 0.5, -1.0, -0.0, np.float32(1e-45), np.nan, np.inf])
    x = np.full(t.size, 0.5, np.float32)
    got = engine.class_hist(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), [0.25, 0.75], 0).cpu().numpy()
    np.testing.assert_array_equal(got, [[0, 4, 0, 0], [0, 4, 0, 0]])
    np.testing.assert_array_equal(got, rm.class_hist(x, t, np.float32([0.25, 0.75]), 0))


def _contention_inputs():
    rng = np.random.default_rng(7)
    obj = rng.random(BIG) < 0.2
    t = obj.astype(np.float32)
    return {
        # one slot for every entry: the worst case for the counters
        "equal": (np.full(BIG, 0.9, np.float32), np.ones(BIG, np.float32)),
        # two spikes, as a converged dose: empty just under tl, object just over tu
        "spikes": (np.where(obj, np.float32(0.96), np.float32(0.84)).astype(np.float32), t),
        # every slot in use in every workgroup: the flush of many slots from many workgroups
        "uniform": (rng.uniform(0.0, 1.3, BIG).astype(np.float32), t),
    }


@pytest.fixture(scope="module")
def contention():
    out = {}
    for name, (x, t) in _contention_inputs().items():
        out[name] = (torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), rm.class_hist(x, t, rm.THRESHOLDS, 0),
                     rm.class_hist(x, t, rm.HIST_EDGES, 1))
    return out


@pytest.mark.parametrize("fold", [1, 0, 2])
@pytest.mark.parametrize("name", ["equal", "spikes", "uniform"])
def test_contention_and_multi_workgroup_flush(contention, knobs, name, fold):
    """fold 1: the production kernel (a wave folds a key that 8 or more of its lanes share before it
    touches LDS); fold 0: every lane adds to LDS itself, fold 2: a wave always folds two keys -- the
    variants DESIGN.md 4h measures it against."""
    if fold != 1:
        knobs(TVAM_REPORT_FOLD=fold)
    x, t, want0, want1 = contention[name]
    np.testing.assert_array_equal(engine.class_hist(x, t, rm.THRESHOLDS, 0).cpu().numpy(), want0)
    np.testing.assert_array_equal(engine.class_hist(x, t, rm.HIST_EDGES, 1).cpu().numpy(), want1)
    if name == "equal":
        assert np.count_nonzero(want0) == 1 and want0.max() == BIG


def test_no_entries_gives_zeros():
    z = torch.zeros(0, dtype=torch.float32, device=DEV)
    out = torch.full((2, 302), 5, dtype=torch.int64, device=DEV)
    got = engine.class_hist(z, z, rm.THRESHOLDS, 0, out=out)
    assert got.data_ptr() == out.data_ptr() and not out.any()


def test_invalid_arguments_name_the_cause():
    x = torch.zeros(16, dtype=torch.float32, device=DEV)
    for edges, side, msg in (
            ([0.0, 0.5, 0.25], 0, r"tvam_class_hist: edges must be strictly increasing \(edge 2 <= edge 1\)"),
            ([0.0, 0.5, 0.5], 1, r"tvam_class_hist: edges must be strictly increasing \(edge 2 <= edge 1\)"),
            ([0.0, np.nan, 1.0], 0, "tvam_class_hist: edge 1 is not finite"),
            ([0.0, np.inf], 0, "tvam_class_hist: edge 1 is not finite"),
            ([], 0, r"tvam_class_hist: 1 <= n_edges <= 2048 \(got 0\)"),
            (np.arange(2049), 0, r"tvam_class_hist: 1 <= n_edges <= 2048 \(got 2049\)"),
            ([0.0, 1.0], 2, r"tvam_class_hist: side must be 0 or 1 \(got 2\)")):
        with pytest.raises(ValueError, match=msg):
            engine.class_hist(x, x, np.asarray(edges, np.float32), side)
    with pytest.raises(ValueError, match="same number of elements"):
        engine.class_hist(x, x[:8], [0.0], 0)
    with pytest.raises(ValueError, match="out must be a contiguous int64 tensor"):
        engine.class_hist(x, x, [0.0], 0, out=torch.zeros(2, 4, dtype=torch.int64, device=DEV))


def test_second_call_zeroes_the_buffer_and_memory_returns():
    """The call zeroes counts itself (a second call on the same buffer gives the same counts, not
    twice them), and what it allocates (the device copy of the edge table) is gone when it returns."""
    x, t, want0, want1 = _reference(4099)
    dx, dt = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    out0 = torch.full((2, 302), -1, dtype=torch.int64, device=DEV)
    out1 = torch.full((2, 503), -1, dtype=torch.int64, device=DEV)
    small = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    engine.class_hist(dx, dt, rm.THRESHOLDS, 0, out=out0)  # the runtime and the kernels are loaded
    torch.cuda.synchronize()
    free0, owned0 = torch.cuda.mem_get_info(0)[0], engine.device_bytes()
    for _ in range(2):
        engine.class_hist(dx, dt, rm.THRESHOLDS, 0, out=out0)
        engine.class_hist(dx, dt, rm.HIST_EDGES, 1, out=out1)
        with pytest.raises(ValueError, match="strictly increasing"):  # a refusal allocates nothing
            engine.class_hist(dx, dt, np.float32([1.0, 0.0]), 0, out=small)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free0 and engine.device_bytes() == owned0
    np.testing.assert_array_equal(out0.cpu().numpy(), want0)
    np.testing.assert_array_equal(out1.cpu().numpy(), want1)


def test_report_on_cuda_tensors(tmp_path, capsys):
    """iou_sweep and save_histogram on a 24^3 CUDA volume: the 300-pass model's IoU array bit for bit,
    its best threshold, and the histogram files."""
    rng = np.random.default_rng(11)
    n = 24 ** 3
    obj = rng.random(n) < 0.2
    x = np.where(obj, rng.normal(0.97, 0.05, n), rng.normal(0.80, 0.10, n)).astype(np.float32)
    x[:4] = [np.nan, -0.25, 1.3, 7.0]
    t = obj.astype(np.float32)
    vol = torch.from_numpy(x).to(DEV).reshape(24, 24, 24, 1)
    tgt = torch.from_numpy(t).reshape(24, 24, 24, 1)  # on the host, as optimize() holds it
    iou, best = rm.iou_sweep(x, t)
    got = utils.iou_sweep(vol, tgt.to(DEV))
    np.testing.assert_array_equal(got["iou"].view(np.uint32), iou.view(np.uint32))
    assert got["best_index"] == best and got["best_threshold"] == float(rm.THRESHOLDS[best])
    rep = utils.save_histogram(vol, tgt, str(tmp_path / "histogram.png"), 0.25, 4.0)
    _, on_disk = rm.check_report_files(tmp_path, x, t, efficiency=0.25, max_intensity=4.0)
    assert on_disk == json.loads(json.dumps(rep))
    lines = capsys.readouterr().out.splitlines()
    assert "Best IoU: {:.4f}".format(iou[best]) in lines and "Best threshold: {:4f}".format(rm.THRESHOLDS[best]) in lines

"""The fused L2 / surface-aware loss kernels without a GPU: tests/loss_model.py's level A against its
level B within the derived bounds, level B against the torch definitions (L2Loss / ThresholdedLoss
__call__ on float64 tensors), the checkers against numpy stand-ins with deliberate defects, and the
declaration of the new entry points (header, ctypes table, argument checks, Python methods)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loss_model as lm
import vec_model as vm
from drtvam_amd import _abi
from drtvam_amd.loss import L2Loss, ThresholdedLoss

TL, TU = 0.85, 0.95
WEIGHTS = (1.0, 1.3, 0.7)  # object, void, limit
KS = [1, 2, 3, 4, 5, 16]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tvam.h")
NEW = ["tvam_loss_square", "tvam_loss_square_probes", "tvam_loss_surface", "tvam_loss_surface_probes"]


def _params(scale):
    return (TL, TU) + WEIGHTS + (scale,)


def _ks(law):
    return KS if law == "surface_threshold" else [2]


# ---------------------------------------------------------------------------
# level A against level B
@pytest.mark.parametrize("law", lm.LAWS)
def test_level_a_within_the_derived_bound_of_level_b(law):
    for K in _ks(law):
        for n, scale in ((3073, 1.0), (65541, 1.0 / 65541)):
            x, t = lm.inputs(law, n, 11 + K, TL, TU)
            lm.check_level_a_against_b(law, x, t, K, *_params(scale))
            alphas = [1.0, 0.25, -0.5]
            x0, dx, t = lm.probe_inputs(law, n, 12 + K, alphas, TL, TU)
            for a in alphas:
                lm.check_level_a_against_b(law, vm.fma32(a, dx, x0), t, K, *_params(scale))


def test_inputs_cover_the_edge_cases():
    x, t = lm.inputs("l2", 3073, 1, TL, TU)
    assert np.any(t < 0) and np.any((t == 0) & np.signbit(t)) and np.any((t == 0) & ~np.signbit(t)) and np.any(x == t)
    for law in ("surface_threshold", "surface_l2"):
        x, t = lm.inputs(law, 3073, 1, TL, TU)
        t0, t1 = t[0::2], t[1::2]
        assert np.all(t0 + t1 > 0) and np.any(t0 == 0) and np.any(t1 == 0) and np.any((t0 > 0) & (t1 > 0))
        for k in vm.loss_thresholds(TL, TU):
            assert np.any(x[0::2] == k) and np.any(x[1::2] == k)
        assert np.any(x[1::2] == 0)


def test_model_refuses_subnormal_intermediates():
    x = np.float32([1.0 + 2.0 ** -20, 0.5])
    t = np.float32([1.0, 1.0])
    with pytest.raises(vm.SubnormalInput):
        lm.level_a("surface_threshold", x, t, 16, *_params(1.0))  # (2^-20)^16 underflows
    with pytest.raises(vm.SubnormalInput):
        lm.level_a("l2", np.float32([2.0 ** -70]), np.float32([0.0]), 2, *_params(1.0))


# ---------------------------------------------------------------------------
# level B against the torch definitions
def _f32_props(reduction, K=2):
    f = lambda v: float(np.float32(v))
    return {"reduction": reduction, "K": K, "tl": f(TL), "tu": f(TU), "weight_object": f(WEIGHTS[0]),
            "weight_void": f(WEIGHTS[1]), "weight_limit": f(WEIGHTS[2])}


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("law", lm.LAWS)
def test_level_b_equals_the_torch_mirror(law, reduction):
    n = 8 * 9 * 10
    for K in _ks(law):
        x, t = lm.inputs(law, n, 21 + K, TL, TU)
        scale = lm.mean_scale(reduction, n)
        vb, gb, _, _ = lm.level_b(law, x, t, K, *_params(1.0), scale64=scale)
        fn = (L2Loss if law != "surface_threshold" else ThresholdedLoss)(_f32_props(reduction, K))
        c = lm.channels(law)
        xt = torch.from_numpy(x.astype(np.float64)).reshape(8, 9, 10, c).requires_grad_(True)
        tt = torch.from_numpy(t.astype(np.float64)).reshape(8, 9, 10, c)
        loss = fn(xt, tt, torch.zeros(4, dtype=torch.float64))
        loss.backward()
        want = scale * math_fsum(vb)
        got = float(loss.detach())
        assert abs(got - want) <= 1e-12 * abs(want), (law, K, got, want)
        g = xt.grad.reshape(-1).numpy()
        assert np.all(np.abs(g - gb) <= 1e-12 * np.abs(gb)), (law, K)


def math_fsum(a):
    import math
    return math.fsum(np.asarray(a, dtype=np.float64).tolist())


def test_mean_counts_voxels_in_the_python_layer():
    """Loss._fused_scale: 1 / voxels, of the slab's film when a count is given; a two-channel voxel once."""
    for cls in (L2Loss, ThresholdedLoss):
        fn = cls({"reduction": "mean"})
        x1, x2 = torch.zeros(3, 4, 5, 1), torch.zeros(3, 4, 5, 2)
        assert fn._fused_scale(x1, x1, None) == 1.0 / 60 and fn._fused_scale(x2, x2, None) == 1.0 / 60
        assert fn._fused_scale(x2[:1], x2[:1], 60) == 1.0 / 60
        assert fn._fused_scale(x1, torch.zeros(3, 4, 5), None) == 1.0 / 60
        assert cls({})._fused_scale(x2, x2, None) == 1.0


# ---------------------------------------------------------------------------
# the checkers on stand-ins
@pytest.mark.parametrize("law", lm.LAWS)
def test_checkers_accept_the_faithful_stand_in(law):
    n, K = 257, 3
    x, t = lm.inputs(law, n, 31, TL, TU)
    for reduction in ("sum", "mean"):
        params = _params(lm.mean_scale(reduction, n))
        v, g = lm.standin(law, x, t, K, params)
        lm.check_loss(law, v, x, t, K, params, grad=g)
        lm.check_reduced(law, v, x, t, K, (TL, TU) + WEIGHTS, reduction, n, grad=g)


@pytest.mark.parametrize("law", ["surface_threshold", "surface_l2"])
@pytest.mark.parametrize("defect", ["swap_w", "split_pair"])
def test_checkers_reject_two_channel_defects(law, defect):
    n, K = 257, 2
    x, t = lm.inputs(law, n, 32, TL, TU)
    params = _params(1.0 / n)
    v, g = lm.standin(law, x, t, K, params, defect=defect)
    with pytest.raises(AssertionError):
        lm.check_loss(law, v, x, t, K, params)  # the value alone
    with pytest.raises(AssertionError):
        lm.check_loss(law, lm.standin(law, x, t, K, params)[0], x, t, K, params, grad=g)  # the gradient alone


@pytest.mark.parametrize("law", lm.LAWS)
def test_checkers_reject_a_gradient_without_scale(law):
    n, K = 257, 2
    x, t = lm.inputs(law, n, 33, TL, TU)
    params = _params(1.0 / n)
    v, g = lm.standin(law, x, t, K, params, defect="no_scale")
    lm.check_loss(law, v, x, t, K, params)  # the value is right
    with pytest.raises(AssertionError):
        lm.check_loss(law, v, x, t, K, params, grad=g)


@pytest.mark.parametrize("law", ["surface_threshold", "surface_l2"])
def test_checkers_reject_a_mean_over_the_float_count(law):
    n, K = 257, 2
    x, t = lm.inputs(law, n, 34, TL, TU)
    v, g = lm.standin(law, x, t, K, _params(1.0 / (2 * n)))  # 1 / x.numel()
    with pytest.raises(AssertionError):
        lm.check_reduced(law, v, x, t, K, (TL, TU) + WEIGHTS, "mean", n)
    with pytest.raises(AssertionError):
        lm.check_reduced(law, lm.standin(law, x, t, K, _params(1.0 / n))[0], x, t, K, (TL, TU) + WEIGHTS, "mean", n, grad=g)


def test_value_check_rejects_one_dropped_voxel():
    for law in lm.LAWS:
        x, t = lm.inputs(law, 257, 35, TL, TU)
        params = _params(1.0)
        va, _ = lm.level_a(law, x, t, 2, *params)
        k = int(np.argmax(va))
        with pytest.raises(AssertionError):
            lm.check_loss(law, math_fsum(np.delete(va, k)), x, t, 2, params)


# ---------------------------------------------------------------------------
# declaration
def test_new_entry_points_are_declared():
    """Fails before the fused L2 / surface-aware losses exist: the four entries in tvam.h, the ctypes
    table and the library, ABI version unchanged, and the three fused methods on L2Loss."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _abi.load_library()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in tvam.h"
        assert name in _abi.EXPORTS and hasattr(lib, name), name
    assert lib.tvam_abi_version() == 13 and _abi.ABI_VERSION == 13
    assert re.search(r"#define\s+TVAM_ABI_VERSION\s+13\b", open(HEADER).read())
    for m in ("fusable", "fused_value", "fused_values", "fused_value_grad"):
        assert callable(getattr(L2Loss, m, None)), m
    assert (_abi.LOSS_KIND_THRESHOLD, _abi.LOSS_KIND_L2) == (0, 1)
    assert "TVAM_LOSS_KIND_THRESHOLD 0" in src and "TVAM_LOSS_KIND_L2 1" in src


def test_argument_checks_name_the_cause():
    """Every refusal is TVAM_ERR_INVALID before any HIP call, with the entry and the cause in the message;
    n = 0 returns 0 and leaves out untouched."""
    lib = _abi.load_library()
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_double * 8)(*([7.0] * 8))
    al = (ctypes.c_float * 8)()
    p, o, a = ctypes.addressof(buf), ctypes.addressof(out), ctypes.addressof(al)
    w = (0.85, 0.95, 1.0, 1.0, 1.0, 1.0)
    cases = [
        (lib.tvam_loss_square, (None, None, 0.0, p, 4, 1.0, o, None, None), "tvam_loss_square: null dose"),
        (lib.tvam_loss_square, (p, None, 0.0, None, 4, 1.0, o, None, None), "tvam_loss_square: null target"),
        (lib.tvam_loss_square, (p, None, 0.0, p, 4, 1.0, None, None, None), "tvam_loss_square: null out"),
        (lib.tvam_loss_square_probes, (p, None, a, 1, p, 4, 1.0, o, None), "tvam_loss_square_probes: null ddose"),
        (lib.tvam_loss_square_probes, (p, p, None, 1, p, 4, 1.0, o, None), "tvam_loss_square_probes: null alphas"),
        (lib.tvam_loss_square_probes, (p, p, a, 0, p, 4, 1.0, o, None), "tvam_loss_square_probes: 1 <= n_alpha <= 8 (got 0)"),
        (lib.tvam_loss_square_probes, (p, p, a, 9, p, 4, 1.0, o, None), "tvam_loss_square_probes: 1 <= n_alpha <= 8 (got 9)"),
        (lib.tvam_loss_surface, (0, None, None, 0.0, p, 4, 2) + w + (o, None, None), "tvam_loss_surface: null dose"),
        (lib.tvam_loss_surface, (0, p, None, 0.0, None, 4, 2) + w + (o, None, None), "tvam_loss_surface: null target"),
        (lib.tvam_loss_surface, (0, p, None, 0.0, p, 4, 2) + w + (None, None, None), "tvam_loss_surface: null out"),
        (lib.tvam_loss_surface, (2, p, None, 0.0, p, 4, 2) + w + (o, None, None),
         "tvam_loss_surface: unknown kind 2 (0: threshold, 1: l2)"),
        (lib.tvam_loss_surface, (-1, p, None, 0.0, p, 4, 2) + w + (o, None, None),
         "tvam_loss_surface: unknown kind -1 (0: threshold, 1: l2)"),
        (lib.tvam_loss_surface, (0, p, None, 0.0, p, 4, 0) + w + (o, None, None),
         "tvam_loss_surface: integer K in [1, 16] required (got 0)"),
        (lib.tvam_loss_surface, (0, p, None, 0.0, p, 4, 17) + w + (o, None, None),
         "tvam_loss_surface: integer K in [1, 16] required (got 17)"),
        (lib.tvam_loss_surface_probes, (0, p, None, a, 1, p, 4, 2) + w + (o, None), "tvam_loss_surface_probes: null ddose"),
        (lib.tvam_loss_surface_probes, (0, p, p, a, 9, p, 4, 2) + w + (o, None),
         "tvam_loss_surface_probes: 1 <= n_alpha <= 8 (got 9)"),
        (lib.tvam_loss_surface_probes, (0, p, p, a, 0, p, 4, 2) + w + (o, None),
         "tvam_loss_surface_probes: 1 <= n_alpha <= 8 (got 0)"),
        (lib.tvam_loss_surface_probes, (3, p, p, a, 1, p, 4, 2) + w + (o, None),
         "tvam_loss_surface_probes: unknown kind 3 (0: threshold, 1: l2)"),
        (lib.tvam_loss_surface_probes, (0, p, p, a, 1, p, 4, 17) + w + (o, None),
         "tvam_loss_surface_probes: integer K in [1, 16] required (got 17)"),
        (lib.tvam_loss_surface_probes, (0, p, p, a, 1, p, 4, 2) + w + (None, None), "tvam_loss_surface_probes: null out"),
    ]
    for fn, args, msg in cases:
        rc = fn(*args)
        assert rc == _abi.TVAM_ERR_INVALID and lib.tvam_last_error().decode() == msg, (msg, rc, lib.tvam_last_error())
        with pytest.raises(ValueError, match=re.escape(msg)):
            _abi.check(rc)
    # n = 0: nothing launched (host pointers would fault a kernel), out untouched; the L2 kind ignores K
    assert lib.tvam_loss_square(p, None, 0.0, p, 0, 1.0, o, None, None) == 0
    assert lib.tvam_loss_square_probes(p, p, a, 8, p, 0, 1.0, o, None) == 0
    assert lib.tvam_loss_surface(0, p, None, 0.0, p, 0, 2, *w, o, None, None) == 0
    assert lib.tvam_loss_surface(1, p, None, 0.0, p, 0, 99, *w, o, None, None) == 0
    assert lib.tvam_loss_surface_probes(1, p, p, a, 8, p, 0, 2, *w, o, None) == 0
    assert list(out) == [7.0] * 8

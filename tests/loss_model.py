"""Reference models, bounds and checkers for the fused L2 and surface-aware loss kernels
(tvam_loss.hip: tvam_loss_square*, tvam_loss_surface*), in the manner of tests/vec_model.py, whose
helpers this module uses.  Numpy only, no GPU: tests/test_loss_model.py runs the checkers on numpy
stand-ins with deliberate defects, tests/test_gpu_loss_kernels.py on the HIP kernels.

Three laws, per voxel (x = fmaf(alpha, ddose, dose) where a step is given):

  'l2'                 one channel: d = x - t; element d d; gradient (2 d) scale
  'surface_threshold'  two channels interleaved (x0, x1), (t0, t1): s = t0 + t1, w_in = t0 / s, w_out =
                       t1 / s; e_in = w_object relu(tu - x0)^K + w_limit relu(x0 - 1)^K, e_out = w_void
                       relu(x1 - tl)^K; element w_in e_in + w_out e_out; gradient (w_in g_in) scale,
                       (w_out g_out) scale
  'surface_l2'         the same weights; e_in = (x0 - 1)^2, e_out = x1^2, g_in = 2 (x0 - 1), g_out = 2 x1

Level A restates the kernels' fp32 operations in their order (one rounding each, no contraction; numpy's
fp32 division is IEEE, like the kernels'), refusing inputs with a nonzero intermediate below 2^-126
(vec_model._guard).  Level B is the reference expression (loss.py:28-59, :62-79, :82-132) in float64.

Rounding counts (first order, u = 2^-24, relative to the sum M of the magnitudes of the terms that are
added; weights and targets >= 0, so the value's terms do not cancel and M is the value itself):

  weights   s rounds once, the division once: 2 each
  l2        value: d 1, the square carries it twice and rounds once: 3.  gradient: d 1, 2 d exact,
            scale 1: 2
  surface_threshold
            a power term w r^K: the relu's argument rounds once and the power carries that K times,
            K - 1 products, the weight 1: 2 K (the (2K + 2) u of vec_model.check_level_a_against_b);
            e_in: the sum of two 1: 2 K + 1; e_out 2 K.  value: 2 K + 1 + weight 2 + weight product 1
            + sum 1: 2 K + 5.  gradient 0: each term (w K) r^(K - 1): the argument carried K - 1
            times, K - 2 products, w K 1, product 1: 2 K - 1; their sum 1, weight 2, weight product 1,
            scale 1: 2 K + 4.  gradient 1: 2 K - 1 + 2 + 1 + 1: 2 K + 3
  surface_l2
            value: (x0 - 1)^2 3, weight 2, product 1 (x1^2: 1 + 2 + 1), sum 1: 7.  gradient 0: d0 1, 2 d0
            exact, weight 2, product 1, scale 1: 5.  gradient 1: 2 + 1 + 1: 4

The bound asserted is (count + 1) u M: the spare rounding covers the second-order terms ((1 + u)^n - 1 <
n u (1 + 2^-19) for n <= 32) and level B's own float64 roundings (a few v = 2^-53 each).
"""
import math

import numpy as np

import vec_model as vm
from vec_model import U, _f32, _guard, _powi32

LAWS = ("l2", "surface_threshold", "surface_l2")
KIND = {"surface_threshold": 0, "surface_l2": 1}  # tvam.h: TVAM_LOSS_KIND_*


def channels(law):
    return 1 if law == "l2" else 2


def roundings(law, K):
    """(value, gradient channel 0, gradient channel 1) first-order rounding counts, see the module text."""
    if law == "l2":
        return 3, 2, 2
    if law == "surface_threshold":
        return 2 * K + 5, 2 * K + 4, 2 * K + 3
    return 7, 5, 4


def mean_scale(reduction, n_vox):
    """The scale a caller passes: 1 / voxels for 'mean' (a two-channel voxel counts once), 1 for 'sum'."""
    return 1.0 / n_vox if reduction == "mean" else 1.0


# ---------------------------------------------------------------------------
# level A
def _split(a, name):
    a = _f32(a, name).reshape(-1)
    assert a.size % 2 == 0, f"{name}: two floats per voxel"
    return a[0::2], a[1::2]


def _weights_a(t0, t1):
    s = _guard(t0 + t1, "t0 + t1")
    return _guard(t0 / s, "w_in"), _guard(t1 / s, "w_out")


def level_a(law, x, target, K, tl, tu, w_object, w_void, w_limit, scale, want_grad=True):
    """The kernels' fp32 arithmetic.  x, target: flat fp32 (interleaved for the two-channel laws).
    Returns fp32 (elements per voxel, gradient per float or None)."""
    tl, tu, wo, wv, wl, sc = vm.loss_params32(tl, tu, w_object, w_void, w_limit, scale)
    one, two, zero, Kf = np.float32(1), np.float32(2), np.float32(0), np.float32(K)
    if law == "l2":
        d = _guard(_f32(x, "x") - _f32(target, "target"), "x - target")
        val = _guard(d * d, "d d")
        return val, (_guard((two * d) * sc, "gradient x scale") if want_grad else None)
    x0, x1 = _split(x, "x")
    t0, t1 = _split(target, "target")
    w_in, w_out = _weights_a(t0, t1)
    if law == "surface_threshold":
        zo, zl, zv = _guard(tu - x0, "tu - x0"), _guard(x0 - one, "x0 - 1"), _guard(x1 - tl, "x1 - tl")
        po, pl, pv = zo > 0, zl > 0, zv > 0
        ro, rl, rv = np.where(po, zo, zero), np.where(pl, zl, zero), np.where(pv, zv, zero)
        e_in = _guard(_guard(wo * _powi32(ro, K, "ro"), "w_object ro^K") + _guard(wl * _powi32(rl, K, "rl"), "w_limit rl^K"),
                      "e_in")
        e_out = _guard(wv * _powi32(rv, K, "rv"), "w_void rv^K")
        if want_grad:
            g_in = _guard(np.where(po, _guard((-wo * Kf) * _powi32(ro, K - 1, "ro"), "object gradient"), zero) +
                          np.where(pl, _guard((wl * Kf) * _powi32(rl, K - 1, "rl"), "limit gradient"), zero), "g_in")
            g_out = np.where(pv, _guard((wv * Kf) * _powi32(rv, K - 1, "rv"), "void gradient"), zero)
    else:
        assert law == "surface_l2", law
        d0 = _guard(x0 - one, "x0 - 1")
        e_in, e_out = _guard(d0 * d0, "d0 d0"), _guard(x1 * x1, "x1 x1")
        if want_grad:
            g_in, g_out = two * d0, two * x1
    val = _guard(_guard(w_in * e_in, "w_in e_in") + _guard(w_out * e_out, "w_out e_out"), "element")
    if not want_grad:
        return val.astype(np.float32), None
    grad = np.empty(2 * x0.size, dtype=np.float32)
    grad[0::2] = _guard(_guard(w_in * g_in.astype(np.float32), "w_in g_in") * sc, "gradient 0 x scale")
    grad[1::2] = _guard(_guard(w_out * g_out.astype(np.float32), "w_out g_out") * sc, "gradient 1 x scale")
    return val.astype(np.float32), grad


# ---------------------------------------------------------------------------
# level B
def level_b(law, x, target, K, tl, tu, w_object, w_void, w_limit, scale, scale64=None):
    """The reference expression in float64 with the fp32-rounded parameters (scale64: the scale itself in
    float64 instead).  Returns float64 (elements per voxel, gradient per float, M of the elements, M of
    the gradient): M = the sum of the magnitudes of the added terms, what the bounds are relative to."""
    tl, tu, wo, wv, wl, sc = (float(v) for v in vm.loss_params32(tl, tu, w_object, w_void, w_limit, scale))
    if scale64 is not None:
        sc = float(scale64)
    if law == "l2":
        d = _f32(x, "x").astype(np.float64) - _f32(target, "target").astype(np.float64)
        return d * d, 2.0 * d * sc, d * d, np.abs(2.0 * d * sc)
    x0, x1 = (a.astype(np.float64) for a in _split(x, "x"))
    t0, t1 = (a.astype(np.float64) for a in _split(target, "target"))
    w_in, w_out = t0 / (t0 + t1), t1 / (t0 + t1)
    if law == "surface_threshold":
        ro, rl, rv = np.maximum(tu - x0, 0.0), np.maximum(x0 - 1.0, 0.0), np.maximum(x1 - tl, 0.0)
        dpow = lambda r: np.where(r > 0, K * r ** (K - 1), 0.0)
        e_in, e_out = wo * ro ** K + wl * rl ** K, wv * rv ** K
        a_in = np.abs(wo * ro ** K) + np.abs(wl * rl ** K)
        g_in, g_out = -wo * dpow(ro) + wl * dpow(rl), wv * dpow(rv)
        ag_in = np.abs(wo * dpow(ro)) + np.abs(wl * dpow(rl))
    else:
        assert law == "surface_l2", law
        e_in, e_out = (x0 - 1.0) ** 2, x1 ** 2
        a_in = e_in
        g_in, g_out = 2.0 * (x0 - 1.0), 2.0 * x1
        ag_in = np.abs(g_in)
    val = w_in * e_in + w_out * e_out
    m_val = np.abs(w_in * a_in) + np.abs(w_out * e_out)
    grad, m_grad = np.empty(2 * x0.size), np.empty(2 * x0.size)
    grad[0::2], grad[1::2] = w_in * g_in * sc, w_out * g_out * sc
    m_grad[0::2], m_grad[1::2] = np.abs(w_in * ag_in * sc), np.abs(grad[1::2])
    return val, grad, m_val, m_grad


def check_level_a_against_b(law, x, target, K, *params):
    """Per element, level A within (count + 1) u M of level B (module text), value and gradient, with
    identical zero sets.  Returns level A."""
    va, ga = level_a(law, x, target, K, *params)
    vb, gb, mv, mg = level_b(law, x, target, K, *params)
    nv, n0, n1 = roundings(law, K)
    ng = np.empty(ga.size)
    ng[0::channels(law)] = n0
    if channels(law) == 2:
        ng[1::2] = n1
    for name, a, b, m, cnt in (("value", va, vb, mv, nv), ("gradient", ga, gb, mg, ng)):
        assert a.shape == b.shape, f"{law} {name}: shape {a.shape} != {b.shape}"
        assert np.array_equal(a == 0, b == 0), f"{law} K = {K}: zero sets of the {name} differ"
        tol = (cnt + 1) * U * m
        bad = np.flatnonzero(np.abs(a.astype(np.float64) - b) > tol)
        assert bad.size == 0, (f"{law} K = {K} {name}: {bad.size} of {a.size} off, first at {bad[0]}: {a[bad[0]]!r} vs "
                               f"{b[bad[0]]!r}")
    return va, ga


def value_bound_rel(law, K):
    """Relative bound of a fused value against the float64 mirror's (non-negative weights and targets:
    the elements do not cancel): every element within (count + 1) u of level B's, and the f64
    accumulation of n of them within n v (vec_model.check_sum), n v < u for n < 2^29."""
    return (roundings(law, K)[0] + 2) * U


# ---------------------------------------------------------------------------
# checkers
def check_loss(law, value, x, target, K, params, grad=None, what="loss", model=None):
    """A kernel's value (and gradient) for the floats x (fp32, after any fma).  value within n v scale
    sum|element| of scale sum(level-A elements) (vec_model.check_sum: an f64 accumulation in any order over
    the n voxels; scale x element is exact in float64); gradient bit for bit level A's."""
    sc = params[-1]
    va, ga = model if model is not None else level_a(law, x, target, K, *params, want_grad=grad is not None)
    terms = float(np.float32(sc)) * va.astype(np.float64)  # exact
    vm.check_sum(float(value), terms, f"{what}: value ({law}, K = {K}, {va.size} voxels)")
    if grad is not None:
        vm.assert_bits_equal(_f32(grad, "grad"), ga, f"{what}: gradient ({law}, K = {K})")


def check_reduced(law, value, x, target, K, weights, reduction, n_vox, grad=None, what="loss"):
    """check_loss for a caller that names its reduction: the scale is worked out here, 1 / n_vox voxels
    for 'mean'.  weights: (tl, tu, w_object, w_void, w_limit)."""
    check_loss(law, value, x, target, K, tuple(weights) + (mean_scale(reduction, n_vox),), grad=grad, what=what)


# ---------------------------------------------------------------------------
# numpy stand-in of the kernels, with deliberate defects
def standin(law, x, target, K, params, defect=None):
    """(value f64, gradient fp32) as the kernels give them, or with one defect: 'swap_w' (w_in and w_out
    exchanged), 'no_scale' (the gradient not multiplied by scale), 'split_pair' (voxel pairs taken one
    float late, as a float4 on an 8-byte aligned address would hold them)."""
    x, target = _f32(x).reshape(-1), _f32(target).reshape(-1)
    sc = np.float32(params[-1])
    if defect == "swap_w":
        assert channels(law) == 2
        target = target.reshape(-1, 2)[:, ::-1].reshape(-1).copy()
    if defect == "split_pair":
        assert channels(law) == 2
        x, target = np.roll(x, -1), np.roll(target, -1)
    with np.errstate(invalid="ignore", divide="ignore"):  # a split pair may divide by t0 + t1 = 0
        va, ga = level_a(law, x, target, K, *params)
    if defect == "split_pair":
        ga = np.roll(ga, 1)
    if defect == "no_scale":
        ga = level_a(law, x, target, K, *(tuple(params[:-1]) + (1.0,)))[1]
    return math.fsum((float(sc) * va.astype(np.float64)).tolist()), ga


# ---------------------------------------------------------------------------
# inputs
def surface_targets(n_vox, rng):
    """(t0, t1) interleaved, t0 + t1 > 0: inside-only (t1 = 0), outside-only (t0 = 0) and boundary voxels
    with both parts in [1 / 16, 1] (weights >= 2^-5: the K = 16 powers stay normal fp32 numbers)."""
    r = rng.random(n_vox)
    a = (0.0625 + 0.9375 * rng.random(n_vox)).astype(np.float32)
    b = (0.0625 + 0.9375 * rng.random(n_vox)).astype(np.float32)
    t = np.empty(2 * n_vox, dtype=np.float32)
    t[0::2] = np.where(r < 0.3, 0.0, a)
    t[1::2] = np.where((r >= 0.3) & (r < 0.6), 0.0, b)
    return t


def inputs(law, n_vox, seed, tl, tu):
    """x uniform in [0, 1.3), snapped to the kinks (vec_model.snap; for 'l2' some x equal their target,
    for 'surface_l2' some x1 are 0), and the law's target: greyscale with 0, -0 and negative values, or
    two-channel volumes."""
    rng = np.random.default_rng(seed)
    if law == "l2":
        x, target = vm.loss_inputs(n_vox, seed, tl, tu)
        x[::5] = target[::5]
        return x, target
    x = vm.snap((rng.random(2 * n_vox) * 1.3).astype(np.float32), tl, tu)
    x[1::14] = 0.0
    return x, surface_targets(n_vox, rng)


def probe_inputs(law, n_vox, seed, alphas, tl, tu):
    """dose, ddose on the 2^-12 grid of vec_model.probe_inputs (alpha dx + x0 exact in float64) and the
    law's target."""
    x0, dx, target = vm.probe_inputs(channels(law) * n_vox, seed, alphas, tl, tu)
    if law != "l2":
        target = surface_targets(n_vox, np.random.default_rng(seed + 7919))
    return x0, dx, target

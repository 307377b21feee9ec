"""CPU: the reference models of tests/vec_model.py against what the project already trusts
(ThresholdedLoss, LinearLBFGS, the Gram-form host recursion), and the checkers against numpy
stand-ins of the kernels with one deliberate defect each: every defect must be rejected, the clean
stand-in accepted, so the tolerances the GPU tests (tests/test_gpu_vec_kernels.py) use are sharp."""
import ctypes

import numpy as np
import pytest
import torch

import vec_model as vm
from drtvam_amd.lbfgs import LinearLBFGS
from drtvam_amd.loss import ThresholdedLoss
from test_lbfgs_fused import NumpyVecLib

TL, TU = 0.85, 0.95
WEIGHTS = (1.0, 1.3, 0.7)  # object, void, limit
N_ODD = 4 * 1031 + 3
HIST_SWEEP = 768 * 256 * 4  # elements of one grid sweep of the history pass (tvam_vec.hip)


def _params(scale=1.0):
    return (TL, TU) + WEIGHTS + (scale,)


# ---------------------------------------------------------------------------
# the models against what the project already trusts
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 16])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_level_b_is_thresholded_loss(K, reduction):
    n = 5003
    x, target = vm.loss_inputs(n, 1, TL, TU)
    tl32, tu32, wo, wv, wl, _ = (float(v) for v in vm.loss_params32(*_params()))
    lf = ThresholdedLoss({"K": K, "tl": tl32, "tu": tu32, "weight_object": wo, "weight_void": wv,
                          "weight_limit": wl, "reduction": reduction})
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    tt = torch.tensor(target.astype(np.float64))
    loss = lf(xt.reshape(n, 1, 1, 1), tt.reshape(n, 1, 1, 1), torch.zeros(1, dtype=torch.float64))
    loss.backward()
    scale = 1.0 / n if reduction == "mean" else 1.0
    vb, gb = vm.loss_level_b(x, target > 0, K, tl32, tu32, wo, wv, wl, np.float32(scale))
    s32 = float(np.float32(scale))
    np.testing.assert_allclose(loss.item() / scale, vb.sum(), rtol=1e-12)
    np.testing.assert_allclose(xt.grad.numpy() / scale * s32, gb, rtol=1e-12, atol=0)
    # the kinks: no gradient at x == tu (object) and x == tl (void)
    assert np.all(gb[(x == np.float32(TU)) & (target > 0)] == 0) and np.all(gb[(x == np.float32(TL)) & ~(target > 0)] == 0)
    assert np.any(x == np.float32(TU)) and np.any(x == np.float32(TL)) and np.any(x == 1)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 7, 16])
def test_level_a_within_bound_of_level_b(K):
    n = 1 << 20
    x, target = vm.loss_inputs(n, 2, TL, TU)
    for scale in (1.0, 1.0 / n):
        va, ga = vm.check_level_a_against_b(x, target > 0, K, *_params(scale))
        assert va.dtype == np.float32 and ga.dtype == np.float32


def test_loss_model_refuses_subnormal_intermediates():
    """Without the snap, K = 16 underflows next to a threshold: the model raises instead of deciding."""
    tu = np.float32(TU)
    x = np.array([np.nextafter(tu, np.float32(0))], dtype=np.float32)
    vm.loss_level_a(x, [True], 5, *_params())
    with pytest.raises(vm.SubnormalInput):
        vm.loss_level_a(x, [True], 16, *_params())
    with pytest.raises(AssertionError):  # 24-bit step size, inputs off the grid: the fma is not one rounding
        vm.fma32(np.float32(0.3), np.array([1.0 + 2.0 ** -23], np.float32), np.array([2.0 ** 30], np.float32))


def test_two_loop_is_linear_lbfgs_direction():
    n, k = 300, 60
    gen = torch.Generator().manual_seed(0)
    A = torch.randn(k, n, generator=gen, dtype=torch.float64) / n ** 0.5
    b = torch.randn(k, generator=gen, dtype=torch.float64)
    key = 'projector.active_data'
    seen = []

    def render(vars_):
        seen.append(vars_[key].detach().clone())
        return A @ vars_[key]

    opt = LinearLBFGS(render_fn=render, loss_step=lambda vol, dvol, alpha, p: ((vol + alpha * dvol - b) ** 2).sum(), m=5)
    opt[key] = torch.rand(n, generator=gen, dtype=torch.float64) * 0.1
    for it in range(9):  # past m + 1 steps: pairs are evicted
        x = opt[key]
        vol = A @ x.detach()
        r = vol - b
        x.grad = 2.0 * (A.t() @ r)
        opt.step(vol, (r * r).sum())
        S, Y = [s.numpy() for s in opt.s[key]], [y.numpy() for y in opt.y[key]]
        g = opt.g_old[key].numpy()
        d, gd, (cg, cs, cy) = vm.two_loop(g, S, Y, first=it == 0)
        ref = seen[-1].numpy()
        np.testing.assert_allclose(d, ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max())
        np.testing.assert_allclose(gd, float(g @ ref), rtol=1e-9)
        # the coefficients the recursion implies reproduce d
        lin = cg * g + sum(cs[j] * S[j] + cy[j] * Y[j] for j in range(len(S)))
        np.testing.assert_allclose(lin, d, rtol=1e-9, atol=1e-12 * np.abs(d).max())
    assert len(opt.s[key]) == 6 or len(opt.s[key]) == 5


# ---------------------------------------------------------------------------
# Gram form against vector form
def _gram_chain(g, S, Y, p, p_old, g_old, first, slots):
    """NumpyVecLib history (h = H - 1 retained pairs + the new one) + coef + direction_dev, the retained
    pairs' Gram entries stored by ring slot as earlier steps would have."""
    lib = NumpyVecLib()
    n, h = g.size, len(S)
    H = h + 1
    ptr = lambda a: a.ctypes.data
    s_new, y_new = np.empty(n, np.float32), np.empty(n, np.float32)
    dots = np.zeros(vm.hist_ndots(h, True))
    lib.tvam_lbfgs_history(n, ptr(p), ptr(p_old), ptr(g), ptr(g_old), h, [ptr(s) for s in S], [ptr(y) for y in Y],
                           ptr(s_new), ptr(y_new), None, ptr(dots), None)
    gram = np.zeros(128)
    for a in range(h):
        for b in range(h):
            gram[slots[a] * 8 + slots[b]] = S[a].astype(np.float64) @ Y[b].astype(np.float64)
            gram[64 + slots[a] * 8 + slots[b]] = Y[a].astype(np.float64) @ Y[b].astype(np.float64)
    coef, gdz, d = np.zeros(17, np.float32), np.zeros(1), np.empty(n, np.float32)
    order = (ctypes.c_int32 * 8)(*slots[:H])
    lib.tvam_lbfgs_coef(H, 1, first, order, ptr(dots), ptr(gram), ptr(coef), ptr(gdz), None)
    lib.tvam_lbfgs_direction_dev(n, ptr(g), H, [ptr(s) for s in S] + [ptr(s_new)], [ptr(y) for y in Y] + [ptr(y_new)],
                                 ptr(coef), ptr(d), None)
    return d, float(gdz[0]), S + [s_new], Y + [y_new]


CHAIN_SLOTS = [3, 0, 5, 1, 7, 2, 6, 4]  # ring slots out of order, oldest pair first


def measure_gram_vec_gap():
    worst_d = worst_gd = 0.0
    for H in (1, 4, 8):
        for first in (0, 1):
            g, S, Y, p, p_old, g_old = vm.chain_inputs(N_ODD, H)
            d, gdz, Sa, Ya = _gram_chain(g, S, Y, p, p_old, g_old, first, CHAIN_SLOTS)
            gap_d, gap_gd = vm.chain_gaps(d, gdz, g, Sa, Ya, first)
            worst_d, worst_gd = max(worst_d, gap_d), max(worst_gd, gap_gd)
    return worst_d, worst_gd


def test_gram_form_against_vector_form():
    """The recorded constant holds for a fresh measurement (reference against reference), and the Gram
    chain on the host passes the GPU chain's check."""
    gap_d, gap_gd = measure_gram_vec_gap()
    print(f"Gram against vector form: direction {gap_d:.3e} M_i, g.d {gap_gd:.3e} sum|terms|")
    assert gap_d <= vm.GRAM_VEC_GAP and gap_gd <= vm.GRAM_VEC_GAP
    g, S, Y, p, p_old, g_old = vm.chain_inputs(N_ODD, 4)
    d, gdz, Sa, Ya = _gram_chain(g, S, Y, p, p_old, g_old, 0, CHAIN_SLOTS)
    vm.check_chain(d, gdz, g, Sa, Ya, 0)
    with pytest.raises(AssertionError):  # gamma = 1 where the newest pair's scaling belongs
        vm.check_chain(d, gdz, g, Sa, Ya, 1)


# ---------------------------------------------------------------------------
# the checkers reject what they must: numpy stand-ins with one deliberate defect
_vectors = vm.hist_inputs


def standin_history(g, S, Y, p, p_old, g_old, defect=None, skip=None):
    """dots by float64 BLAS dot products (an order of its own), s_new and y_new in fp32."""
    s_new, y_new = p - p_old, g - g_old
    keep = np.ones(g.size, dtype=bool)
    if skip is not None:
        keep[skip] = False
    dots = []
    for _, a, b in vm.history_pairs(g, S, Y, s_new, y_new):
        if defect == "fp32":
            dots.append(float(np.sum((a[keep] * b[keep]).astype(np.float32), dtype=np.float32)))
        else:
            dots.append(float(a[keep].astype(np.float64) @ b[keep].astype(np.float64)))
    dots = np.array(dots)
    if defect == "swap_new_blocks":
        ht = len(S) + 1
        dots[2 * ht:3 * ht], dots[3 * ht:4 * ht] = dots[3 * ht:4 * ht].copy(), dots[2 * ht:3 * ht].copy()
    return s_new, y_new, dots


def _run_history(n, h, **kw):
    g, S, Y, p, p_old, g_old = _vectors(n, h)
    if kw.get("skip") is not None:  # the dropped element counts in every dot
        for v in [g, p, g_old] + S + Y:
            v[kw["skip"]] = 1.0
        p_old[kw["skip"]] = 0.25
    s_new, y_new, dots = standin_history(g, S, Y, p, p_old, g_old, **kw)
    vm.check_history(dots, g, S, Y, p=p, p_old=p_old, g_old=g_old, s_new=s_new, y_new=y_new)


def test_history_checker_accepts_the_clean_standin():
    for n, h in ((1, 0), (7, 7), (N_ODD, 3), (HIST_SWEEP + 4 * 300 + 3, 1)):
        _run_history(n, h)


@pytest.mark.parametrize("kw", [
    dict(n=N_ODD, h=3, skip=N_ODD - 1),                                  # last tail element skipped
    dict(n=HIST_SWEEP + 4 * 300 + 3, h=1, skip=HIST_SWEEP + 4 * 17 + 2),  # one element of the second sweep skipped
    dict(n=N_ODD, h=3, defect="fp32"),                                   # dots accumulated in fp32
    dict(n=N_ODD, h=3, defect="swap_new_blocks"),                        # s_new.y_j and s_j.y_new blocks swapped
], ids=["tail", "second_sweep", "fp32_accumulator", "new_pair_blocks"])
def test_history_checker_rejects(kw):
    with pytest.raises(AssertionError):
        _run_history(**kw)


def test_history_checker_rejects_wrong_new_pair_and_layout():
    g, S, Y, p, p_old, g_old = _vectors(N_ODD, 2)
    s_new, y_new, dots = standin_history(g, S, Y, p, p_old, g_old)
    bad = s_new.copy()
    bad[-1] = np.nextafter(bad[-1], np.float32(9))
    with pytest.raises(AssertionError):
        vm.check_history(dots, g, S, Y, p=p, p_old=p_old, g_old=g_old, s_new=bad, y_new=y_new)
    with pytest.raises(AssertionError):  # the layout without a new pair is 2 h + 1 dots
        vm.check_history(dots, g, S, Y)
    vm.check_history(dots, g, S, Y, s_pre=s_new, g_old=g_old, s_new=s_new, y_new=y_new)  # the SPRE form


def test_band_sums_and_band_writes():
    A, R, C, h = 7, 36, 44, 3
    n = A * R * C
    g, S, Y, p, p_old, g_old = _vectors(n, h, seed=3)
    total = np.zeros(vm.hist_ndots(h, True))
    s_full = np.full(n, np.nan, np.float32)
    for r0, r1 in ((0, 5), (5, 21), (21, 36)):
        idx = vm.band_index(A, (r1 - r0) * C, R * C, r0 * C)
        gi = lambda v: v[idx]
        s_b, y_b, dots = standin_history(gi(g), [gi(s) for s in S], [gi(y) for y in Y], gi(p), gi(p_old), gi(g_old))
        vm.check_history(dots, gi(g), [gi(s) for s in S], [gi(y) for y in Y], p=gi(p), p_old=gi(p_old),
                         g_old=gi(g_old), s_new=s_b, y_new=y_b)
        band_only = np.full(n, np.nan, np.float32)
        band_only[idx] = s_b
        vm.check_untouched(band_only, idx, "s_new")
        band_only[(idx[-1] + 1) % n] = 0.0  # a band write that also touches a row outside the band
        with pytest.raises(AssertionError):
            vm.check_untouched(band_only, idx, "s_new")
        s_full[idx] = s_b
        total += dots
    vm.check_history(total, g, S, Y, p=p, p_old=p_old, g_old=g_old, s_new=s_full)
    total[4] += (total[4] - dots[4]) * 1e-9  # a band's share lost to a careless sum
    with pytest.raises(AssertionError):
        vm.check_history(total, g, S, Y, p=p, p_old=p_old, g_old=g_old)


def standin_direction(g, S, Y, cg, cs, cy, defect=None):
    if defect == "swap":
        cs, cy = cy, cs
    r = np.float32(cg) * g
    for j in range(len(S)):  # two roundings per term where the kernel's fma has one
        r = (np.float32(cs[j]) * S[j] + (np.float32(cy[j]) * Y[j] + r)).astype(np.float32)
    if defect == "tail":
        r[-1] = 0.0
    return r


@pytest.mark.parametrize("h", [0, 1, 8])
def test_direction_checker(h):
    g, S, Y, _, _, _ = _vectors(N_ODD, h, seed=4)
    rng = np.random.default_rng(5)
    cg, cs, cy = -0.7, rng.standard_normal(8).astype(np.float32), rng.standard_normal(8).astype(np.float32)
    # exact products, then one rounding per term: within the bound's 2 h + 2 roundings
    d64 = np.float32(cg) * g.astype(np.float64)
    d = d64.astype(np.float32)
    for j in range(h):
        d = (float(cs[j]) * S[j].astype(np.float64) + (float(cy[j]) * Y[j].astype(np.float64) + d).astype(np.float32)
             ).astype(np.float32)
    vm.check_direction(d, g, S, Y, cg, cs, cy)
    with pytest.raises(AssertionError):
        vm.check_direction(standin_direction(g, S, Y, cg, cs, cy, "tail"), g, S, Y, cg, cs, cy)
    if h:
        with pytest.raises(AssertionError):  # cs and cy swapped
            vm.check_direction(standin_direction(g, S, Y, cg, cs, cy, "swap"), g, S, Y, cg, cs, cy)


def test_axpy_checker_and_guards():
    n = N_ODD
    rng = np.random.default_rng(6)
    p, d = rng.random(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    for alpha in (0.25, 0.3, 0.0):
        for lo in (0.0, -np.inf):
            exact = np.maximum(p.astype(np.float64) + float(np.float32(alpha)) * d.astype(np.float64), lo)
            out = exact.astype(np.float32)  # one rounding, as the fma
            vm.check_axpy(out, p, alpha, d, lo, s_out=out - p)
            with pytest.raises(AssertionError):  # s_out from the exact sum, not from the rounded out
                vm.check_axpy(out, p, alpha, d, lo, s_out=(exact - p).astype(np.float32) + np.float32(1e-7))
            bad = out.copy()
            bad[-1] = p[-1]  # last tail element skipped
            if alpha and d[-1] and (lo < 0 or exact[-1] > 0):
                with pytest.raises(AssertionError):
                    vm.check_axpy(bad, p, alpha, d, lo)
    whole = np.full(n + 2 * vm.GUARD, np.nan, np.float32)
    whole[vm.GUARD:vm.GUARD + n] = p
    vm.check_guards(whole, vm.GUARD, n, "out")
    whole[vm.GUARD + n] = 0.0  # one float written past the end of an output
    with pytest.raises(AssertionError):
        vm.check_guards(whole, vm.GUARD, n, "out")
    whole[vm.GUARD + n] = np.nan
    whole[vm.GUARD - 1] = 1.0
    with pytest.raises(AssertionError):
        vm.check_guards(whole, vm.GUARD, n, "out")


def standin_loss(x, obj, K, params, defect=None):
    """Level-A elements summed by numpy's float64 pairwise sum (an order of its own)."""
    va, ga = vm.loss_level_a(x, obj, K, *params)
    scale = float(np.float32(params[-1]))
    if defect == "K-1":
        va, _ = vm.loss_level_a(x, obj, K - 1, *params)
    if defect == "kink":  # gradient taken at zo >= 0: -w K r^(K - 1) scale at x == tu
        tl, tu, wo, wv, wl, sc = vm.loss_params32(*params)
        at = obj & (x == tu)
        ga = np.where(at, (-wo * np.float32(K)) * (np.float32(0) if K > 1 else np.float32(1)) * sc, ga).astype(np.float32)
    if defect == "tail":
        va = va[:-1]
    if defect == "second_sweep":
        va = np.delete(va, 2097152 + 77)
    return scale * float(np.sum(va.astype(np.float64))), ga


@pytest.mark.parametrize("K", [1, 2, 16])
def test_loss_checker(K):
    n = N_ODD
    x, target = vm.loss_inputs(n, 7, TL, TU)
    obj = target > 0
    x[-1], obj[-1] = 0.25, True  # an element that counts, last
    for scale in (1.0, 1.0 / n):
        params = _params(scale)
        v, g = standin_loss(x, obj, K, params)
        vm.check_loss(v, x, obj, K, params, grad=g)
        with pytest.raises(AssertionError):  # last tail element skipped
            vm.check_loss(standin_loss(x, obj, K, params, "tail")[0], x, obj, K, params)
        if K > 1:
            with pytest.raises(AssertionError):  # value computed with K - 1
                vm.check_loss(standin_loss(x, obj, K, params, "K-1")[0], x, obj, K, params)
        if K == 1:
            assert np.any(obj & (x == np.float32(TU)))
            with pytest.raises(AssertionError):  # gradient nonzero at x == tu
                vm.check_loss(v, x, obj, K, params, grad=standin_loss(x, obj, K, params, "kink")[1])
        with pytest.raises(AssertionError):  # an fp32 accumulator
            va, _ = vm.loss_level_a(x, obj, K, *params)
            vm.check_loss(float(np.float32(scale)) * float(np.sum(va, dtype=np.float32)), x, obj, K, params)


def test_loss_checker_rejects_a_dropped_element_of_the_second_sweep():
    n = 2097152 + 4 * 300 + 3
    x, target = vm.loss_inputs(n, 8, TL, TU)
    obj = target > 0
    x[2097152 + 77], obj[2097152 + 77] = 0.25, True
    params = _params(1.0 / n)
    vm.check_loss(standin_loss(x, obj, 2, params)[0], x, obj, 2, params)
    with pytest.raises(AssertionError):
        vm.check_loss(standin_loss(x, obj, 2, params, "second_sweep")[0], x, obj, 2, params)


def test_probe_inputs_make_the_fma_one_rounding():
    alphas = [1.0, 0.5, 0.25, 0.125, 2.0 ** -7, 3.0, 0.0, -0.5, 0.3125]
    x0, dx, target = vm.probe_inputs(N_ODD, 9, alphas, TL, TU)
    for a in alphas:
        x = vm.fma32(a, dx, x0)
        for K in (1, 5, 16):
            vm.loss_level_a(x, target > 0, K, *_params(1.0 / N_ODD))  # no SubnormalInput
    assert np.count_nonzero(dx) > N_ODD // 2


def test_mask_model_and_checker():
    rng = np.random.default_rng(10)
    for n in (1, 31, 32, 33, 64 * 1000 + 13):
        t = rng.standard_normal(n).astype(np.float32)
        t[::7] = 0.0
        t[3::11] = -0.0
        t[5::13] = 1e-45
        t[6::17] = -1e-45
        words = vm.mask_model(t)
        assert words.size == (n + 31) // 32
        loop = [sum(1 << j for j in range(32) if 32 * w + j < n and t[32 * w + j] > 0) for w in range(min(words.size, 40))]
        assert [int(w) for w in words[:40]] == loop
        vm.check_target_mask(words, t)
        for bit0 in (0, 1, 4, 31, 33):
            if bit0 < n:
                assert np.array_equal(vm.mask_bits(words, bit0, n - bit0), t[bit0:] > 0)
        if n >= 31:
            off = np.roll(np.unpackbits(words.view(np.uint8), bitorder="little"), 1)  # mask written one bit off
            with pytest.raises(AssertionError):
                vm.check_target_mask(np.packbits(off, bitorder="little").view("<u4"), t)
    # a loss that reads the mask one bit off
    n = N_ODD
    x, target = vm.loss_inputs(n, 11, TL, TU)
    words = vm.mask_model(np.concatenate([np.zeros(36, np.float32), target]))
    params = _params(1.0 / n)
    obj = vm.mask_bits(words, 36, n)
    assert np.array_equal(obj, target > 0)
    v, g = standin_loss(x, obj, 2, params)
    vm.check_loss(v, x, target > 0, 2, params, grad=g)
    v1, g1 = standin_loss(x, vm.mask_bits(words, 37, n), 2, params)
    with pytest.raises(AssertionError):
        vm.check_loss(v1, x, target > 0, 2, params)
    with pytest.raises(AssertionError):
        vm.check_loss(v, x, target > 0, 2, params, grad=g1)

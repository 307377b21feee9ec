"""CPU: the first-order optimisers' numpy models (tests/optim_model.py).  The checkers accept the
model and reject stand-ins with deliberate defects; level A lies within the derived bound of level
B; the first Adam step moves every entry by lr against its gradient's sign."""
import math

import numpy as np
import pytest

import optim_model as om

F = np.float32
N = 4 * 1031 + 3
LR = 0.01
CASES = [dict(mask=False, uniform=False), dict(mask=True, uniform=False), dict(mask=False, uniform=True),
         dict(mask=True, uniform=True)]


def adam_standin(p, g, m, v, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask=False, lo=-math.inf, defect=None):
    """Adam written out once more, with one deliberate defect."""
    t1 = t if defect == "t" else t + 1
    lr_t, b1, c1, b2, c2, e = om.adam_scalars(lr, beta_1, beta_2, epsilon, t1)
    if defect == "c1":
        c1 = F(1) - F(beta_1)
    keep = (g == 0) & mask
    m1 = b1 * m + c1 * g
    v1 = b2 * v + c2 * (g * g)
    if defect != "mask":
        m1, v1 = np.where(keep, m, m1), np.where(keep, v, v1)
    den = np.sqrt(v1) + e
    w = p - (lr_t * (m1 / den) if defect == "order" else (lr_t * m1) / den)
    w = np.where(keep, p, w)
    return (w if defect == "clamp" else om.clamp(w, lo)), m1, v1, t1


@pytest.mark.parametrize("defect", [None, "order", "c1", "mask", "t", "clamp"])
def test_adam_checker_rejects_defects(defect):
    p, g, m, v, _ = om.optim_inputs(N, seed=1)
    if defect == "clamp":
        g = np.abs(g)  # steps down, below the clamp at 0
    kw = dict(lr=LR, mask=True, lo=0.0)
    with np.errstate(under="ignore"):
        got = adam_standin(p, g, m, v, 3, defect=defect, **kw)
    if defect is None:
        om.check_adam(*got, p, g, m, v, 3, **kw)
    else:
        with pytest.raises(AssertionError):
            om.check_adam(*got, p, g, m, v, 3, **kw)


@pytest.mark.parametrize("case", CASES)
def test_adam_checker_accepts_model(case):
    p, g, m, v, _ = om.optim_inputs(N, seed=4)
    for lo in (0.0, -math.inf):
        got = om.adam_step32(p, g, m, v, 7, LR, lo=lo, **case)
        om.check_adam(*got, p, g, m, v, 7, LR, lo=lo, **case)
        if case["uniform"]:  # for an implementation's own S, given
            S = float(np.sum(got[2].astype(np.float64)))
            om.check_adam(*om.adam_step32(p, g, m, v, 7, LR, lo=lo, S=S, N=2 * N, **case), p, g, m, v, 7, LR, lo=lo,
                          S=S, N=2 * N, **case)


def test_sgd_checker_accepts_model_and_rejects_defects():
    p, g, _, _, s = om.optim_inputs(N, seed=2)
    for mom, st in ((0.0, None), (0.9, s)):
        for mask in (False, True):
            om.check_sgd(*om.sgd_step32(p, g, st, LR, mom, mask, 0.0), p, g, st, LR, mom, mask, 0.0)
    g = np.abs(g)
    lr32, mu = F(LR), F(0.9)
    s1 = mu * s + g
    with pytest.raises(AssertionError):  # the clamp missing
        om.check_sgd(p - lr32 * s1, s1, p, g, s, LR, 0.9, False, 0.0)
    with pytest.raises(AssertionError):  # the mask on w only
        om.check_sgd(om.clamp(np.where(g == 0, p, p - lr32 * s1), 0.0), s1, p, g, s, LR, 0.9, True, 0.0)
    with pytest.raises(AssertionError):  # lr (mu s + g) contracted: the double's product rounded once
        w = (p.astype(np.float64) - float(lr32) * s1.astype(np.float64)).astype(np.float32)
        om.check_sgd(om.clamp(w, 0.0), s1, p, g, s, LR, 0.9, False, 0.0)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("t", [0, 1, 999])
def test_adam_level_a_within_bound_of_level_b(case, t):
    """g over 2^-60 .. 2^20 with exact zeros, v at 0, p at the clamp."""
    p, g, m, v, _ = om.optim_inputs(N, seed=3 + t)
    assert np.any(g == 0) and np.any(v == 0) and np.any(p == 0)
    a = om.adam_step32(p, g, m, v, t, LR, lo=0.0, **case)
    b = om.adam_step64(p, g, m, v, t, LR, lo=0.0, **case)
    Ep, Em, Ev = om.adam_bound(p, g, m, v, t, LR, **case)
    om.check_within_bound(a[1], b[1], Em, "m'")
    om.check_within_bound(a[2], b[2], Ev, "v'")
    om.check_within_bound(a[0], b[0], Ep, "p'")
    assert a[3] == b[3] == t + 1


@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("mask", [False, True])
def test_sgd_level_a_within_bound_of_level_b(mom, mask):
    p, g, _, _, s = om.optim_inputs(N, seed=7)
    st = s if mom else None
    a = om.sgd_step32(p, g, st, LR, mom, mask, 0.0)
    b = om.sgd_step64(p, g, st, LR, mom, mask, 0.0)
    Ep, Es = om.sgd_bound(p, g, st, LR, mom, mask)
    om.check_within_bound(a[0], b[0], Ep, "p'")
    if mom:
        om.check_within_bound(a[1], b[1], Es, "s'")


def test_first_adam_step_is_lr_against_the_sign():
    p, g, _, _, _ = om.optim_inputs(N, seed=11)
    nz = g != 0
    p[nz] = 0.0  # w = -q exactly: the bound counts no rounding of p - q
    z = np.zeros_like(p)
    w, m1, v1, t1 = om.adam_step32(p, g, z, z, 0, LR)
    assert t1 == 1
    err = np.abs(w.astype(np.float64) - (p - LR * np.sign(g.astype(np.float64))))
    assert np.all(err[nz] <= om.first_step_bound(g, LR)[nz])
    assert np.array_equal(w[~nz], p[~nz]) and np.any(p[~nz] != 0)
    big = nz & (np.abs(g) > 1)  # there e / (sqrt(c2) |g|) < 3.2e-7: a step of lr, not just a bounded one
    assert np.any(big) and np.all(np.abs(np.abs(w[big]) / LR - 1) < 3.2e-7 + 8 * om.U)


def test_uniform_sum_and_scalars():
    p, g, m, v, _ = om.optim_inputs(N, seed=5)
    _, _, v1, _ = om.adam_step32(p, g, m, v, 0, LR, uniform=True)
    S = float(np.sum(v1.astype(np.float64)))
    om.check_uniform_sum(S, v1)
    with pytest.raises(AssertionError):
        om.check_uniform_sum(float(np.sum(v1, dtype=np.float32)), v1)  # an fp32 accumulation
    lr_t, b1, c1, b2, c2, e = om.adam_scalars(LR, 0.9, 0.999, 1e-8, 1)
    assert c1 == F(0.1) and c1 != F(1) - F(0.9) and c2 == F(0.001)
    assert lr_t == F(LR) * F(math.sqrt(1 - 0.999) / (1 - 0.9))

"""Reference models, bounds and checkers of the first-order optimisers (drtvam_amd/optimizers.py,
tvam_sgd_step / tvam_adam_step / tvam_adam_moments / tvam_adam_apply of tvam_vec.hip): Mitsuba 3's
mi.ad.SGD and mi.ad.Adam for one parameter and a scalar learning rate.  Numpy only, no GPU;
tests/test_optim_model.py runs the checkers on numpy stand-ins with deliberate defects,
tests/test_optimizers.py on the torch path, tests/test_gpu_optimizers.py on the HIP kernels.

Level A (``*_step32``): every elementwise operation a separate, once-rounded numpy float32
operation in the written order; keep = mask and g == 0:

  SGD   momentum 0: w = p - lr32 g.  Else s' = mu s + g; w = p - lr32 s'; keep: s' = s.
  Adam  t' = t + 1; lr_t = fl32(fl32(lr) fl32(sqrt(1 - beta_2^t') / (1 - beta_1^t'))) (the
        quotient in Python floats); b = fl32(beta), c = fl32(1 - beta) (subtraction in double);
        m' = b1 m + c1 g; v' = b2 v + c2 (g g); keep: m' = m, v' = v; den = sqrt(v') + e
        (uniform: fl32(sqrt(S / N)) + e, S the f64 sum of v', root and quotient in f64);
        w = p - (lr_t m') / den.
  both  keep: w = p; p' = w < lo ? lo : w  (max(w, lo) with the sign of a zero and a NaN of w kept).

Level B (``*_step64``): the same formulas on the same fp32 inputs and the same fp32-rounded
scalars, evaluated in float64.

The bound between the two (``sgd_bound`` / ``adam_bound``).  u = 2^-24, eta = 2^-150 (half the
spacing of the fp32 subnormals).  A product, quotient or root rounds as fl(x) = x (1 + d) + h with
|d| <= u, |h| <= eta; a sum or difference of two fp32 numbers as x (1 + d) (it is exact where it
lands among the subnormals).  Second-order terms -- at most 12 such factors meet in one element,
so less than 78 u^2 -- and level B's own at most 12 roundings at 2^-53 are covered by writing
u' = u (1 + 2^-10) for u throughout (78 u and 12 2^-29 are both far below 2^-10).  With the
level-B values on the right-hand sides:

  E_m   <= 2 u' (|b1 m| + |c1 g|) + 2 eta          two products (u each, eta each), one sum (u of both)
  E_v   <= 3 u' (|b2 v| + |c2 g^2|) + 3 eta        g g, c2 (g g) and b2 v (u, eta each; c2 <= 1), one sum
  E_rad  = E_v, or sum(E_v) / N for uniform        the root's argument
  E_sqrt <= u' sqrt(rad) + min(E_rad / sqrt(rad), sqrt(E_rad))
                                                   |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= sqrt|a - b|
  E_den <= E_sqrt + u' den                         the sum with e
  E_num <= |lr_t| E_m + u' |lr_t m'| + eta
  E_q   <= (1 + u') (E_num + |q| E_den) / (den - E_den) + u' |q| + eta,   q = num / den
  E_w   <= (1 + u') E_q + u' (|p| + |q|)
  E_p'  <= E_w (the clamp is 1-Lipschitz); kept entries: E_m = E_v = E_p' = 0.

  SGD:  E_s <= 2 u' (|mu s| + |g|) + eta; E_q <= |lr32| E_s + u' |lr32 s'| + eta; E_w as above
        (momentum 0: E_s = 0 and s' = g).
"""
import math

import numpy as np

from vec_model import U, _f32, assert_bits_equal, check_sum

ETA = 2.0 ** -150
U1 = U * (1 + 2.0 ** -10)
F = np.float32


# ---------------------------------------------------------------------------
# scalars
def adam_scalars(lr, beta_1, beta_2, epsilon, t):
    """(lr_t, b1, c1, b2, c2, e) of the step that raises the count to t, as np.float32."""
    scale = math.sqrt(1 - beta_2 ** t) / (1 - beta_1 ** t)
    return F(lr) * F(scale), F(beta_1), F(1.0 - beta_1), F(beta_2), F(1.0 - beta_2), F(epsilon)


def clamp(w, lo):
    return np.where(w < w.dtype.type(lo), w.dtype.type(lo), w)


# ---------------------------------------------------------------------------
# SGD
def _sgd(p, g, s, lr, momentum, mask, lo, T):
    lr, mu = T(F(lr)), T(F(momentum))
    keep = (g == 0) if mask else np.zeros(g.shape, dtype=bool)
    if s is None:
        assert momentum == 0
        s1 = None
        w = p - lr * g
    else:
        s1 = mu * s + g
        w = p - lr * s1
        s1 = np.where(keep, s, s1)
    return clamp(np.where(keep, p, w), lo), s1


def sgd_step32(p, g, s, lr, momentum=0.0, mask=False, lo=-math.inf):
    """Level A.  s: None without momentum.  Returns (p', s')."""
    return _sgd(_f32(p, "p"), _f32(g, "g"), None if s is None else _f32(s, "s"), lr, momentum, mask, lo, F)


def sgd_step64(p, g, s, lr, momentum=0.0, mask=False, lo=-math.inf):
    """Level B."""
    d = lambda a: None if a is None else _f32(a).astype(np.float64)
    return _sgd(d(p), d(g), d(s), lr, momentum, mask, lo, np.float64)


def sgd_bound(p, g, s, lr, momentum=0.0, mask=False):
    """(E_p', E_s') per element, from the module docstring."""
    p, g = _f32(p).astype(np.float64), _f32(g).astype(np.float64)
    lr, mu = float(F(lr)), float(F(momentum))
    if s is None:
        s1, Es = g, np.zeros_like(g)
    else:
        s = _f32(s).astype(np.float64)
        s1 = mu * s + g
        Es = 2 * U1 * (np.abs(mu * s) + np.abs(g)) + ETA
    q = lr * s1
    Eq = abs(lr) * Es + U1 * np.abs(q) + ETA
    Ew = (1 + U1) * Eq + U1 * (np.abs(p) + np.abs(q))
    if mask:
        Ew, Es = np.where(g == 0, 0.0, Ew), np.where(g == 0, 0.0, Es)
    return Ew, Es


# ---------------------------------------------------------------------------
# Adam
def _adam(p, g, m, v, t, lr, beta_1, beta_2, epsilon, mask, lo, uniform, S, N, T):
    t1 = t + 1
    lr_t, b1, c1, b2, c2, e = (T(x) for x in adam_scalars(lr, beta_1, beta_2, epsilon, t1))
    keep = (g == 0) if mask else np.zeros(g.shape, dtype=bool)
    m1 = b1 * m + c1 * g
    v1 = b2 * v + c2 * (g * g)
    m1, v1 = np.where(keep, m, m1), np.where(keep, v, v1)
    if uniform:
        if S is None:
            S = math.fsum(v1.astype(np.float64).tolist())
        N = g.size if N is None else N
        root = np.sqrt(np.float64(S) / np.float64(N))  # f64 quotient and root at both levels
        den = (F(root) if T is F else root) + e
    else:
        den = np.sqrt(v1) + e
    w = p - (lr_t * m1) / den
    return clamp(np.where(keep, p, w), lo), m1, v1, t1


def adam_step32(p, g, m, v, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask=False, lo=-math.inf, uniform=False,
                S=None, N=None):
    """Level A.  t: the step count before the step.  uniform: S (the f64 sum of v' over all entries;
    default: the exact sum of this call's v') and N (default: the size).  Returns (p', m', v', t')."""
    with np.errstate(under="ignore"):
        return _adam(_f32(p, "p"), _f32(g, "g"), _f32(m, "m"), _f32(v, "v"), t, lr, beta_1, beta_2, epsilon, mask, lo,
                     uniform, S, N, F)


def adam_step64(p, g, m, v, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask=False, lo=-math.inf, uniform=False,
                S=None, N=None):
    """Level B."""
    d = lambda a: _f32(a).astype(np.float64)
    return _adam(d(p), d(g), d(m), d(v), t, lr, beta_1, beta_2, epsilon, mask, lo, uniform, S, N, np.float64)


def adam_bound(p, g, m, v, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask=False, uniform=False, N=None):
    """(E_p', E_m', E_v') per element, from the module docstring (uniform: S summed from this
    call's v', as the models do by default)."""
    p, g, m, v = (_f32(a).astype(np.float64) for a in (p, g, m, v))
    lr_t, b1, c1, b2, c2, e = (float(x) for x in adam_scalars(lr, beta_1, beta_2, epsilon, t + 1))
    keep = (g == 0) if mask else np.zeros(g.shape, dtype=bool)
    Em = np.where(keep, 0.0, 2 * U1 * (np.abs(b1 * m) + np.abs(c1 * g)) + 2 * ETA)
    Ev = np.where(keep, 0.0, 3 * U1 * (np.abs(b2 * v) + np.abs(c2 * g * g)) + 3 * ETA)
    m1 = np.where(keep, m, b1 * m + c1 * g)
    v1 = np.where(keep, v, b2 * v + c2 * (g * g))
    if uniform:
        N = g.size if N is None else N
        rad, Erad = np.float64(v1.sum() / N), np.float64(Ev.sum() / N)
    else:
        rad, Erad = v1, Ev
    root = np.sqrt(rad)
    with np.errstate(divide="ignore", invalid="ignore"):
        Esqrt = U1 * root + np.minimum(np.where(root > 0, Erad / root, np.inf), np.sqrt(Erad))
    den = root + e
    Eden = Esqrt + U1 * den
    assert np.all(den - Eden > 0), "the denominator's error reaches the denominator"
    num = lr_t * m1
    Enum = abs(lr_t) * Em + U1 * np.abs(num) + ETA
    q = num / den
    Eq = (1 + U1) * (Enum + np.abs(q) * Eden) / (den - Eden) + U1 * np.abs(q) + ETA
    Ew = (1 + U1) * Eq + U1 * (np.abs(p) + np.abs(q))
    return np.where(keep, 0.0, Ew), Em, Ev


def first_step_bound(g, lr, beta_2=0.999, epsilon=1e-8):
    """With zero state, |w - (p - lr sign(g))| <= lr (e / (sqrt(c2) |g|) + 8 u) for g != 0: m' / sqrt(v')
    = c1 g / (sqrt(c2) |g|) and the bias scale sqrt(1 - beta_2) / (1 - beta_1) cancel to sign(g); e in
    the denominator lowers the step by the factor 1 / (1 + e / (sqrt(c2) |g|)) >= 1 - e / (sqrt(c2) |g|)."""
    g = np.abs(_f32(g).astype(np.float64))
    c2 = float(F(1.0 - beta_2))
    with np.errstate(divide="ignore"):
        return lr * (float(F(epsilon)) / (math.sqrt(c2) * g) + 8 * U)


# ---------------------------------------------------------------------------
# checkers (bit for bit against level A)
def check_sgd(got_p, got_s, p, g, s, lr, momentum=0.0, mask=False, lo=-math.inf, what="sgd"):
    wp, ws = sgd_step32(p, g, s, lr, momentum, mask, lo)
    assert_bits_equal(_f32(got_p, "p'"), wp, f"{what}: p'")
    if s is not None:
        assert_bits_equal(_f32(got_s, "s'"), ws, f"{what}: s'")


def check_adam(got_p, got_m, got_v, got_t, p, g, m, v, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask=False,
               lo=-math.inf, uniform=False, S=None, N=None, what="adam"):
    """p', m', v' bit for bit and the step count.  uniform with S given: the implementation's own
    sum (checked against the terms with check_uniform_sum), so that p' is compared for that S."""
    wp, wm, wv, wt = adam_step32(p, g, m, v, t, lr, beta_1, beta_2, epsilon, mask, lo, uniform, S, N)
    assert got_t == wt, f"{what}: step count {got_t} != {wt}"
    assert_bits_equal(_f32(got_m, "m'"), wm, f"{what}: m'")
    assert_bits_equal(_f32(got_v, "v'"), wv, f"{what}: v'")
    assert_bits_equal(_f32(got_p, "p'"), wp, f"{what}: p'")


def check_uniform_sum(S, v1, what="adam uniform S"):
    """S within n 2^-53 sum|v'| of the exact sum of the fp32 v' (vec_model.check_sum)."""
    return check_sum(float(S), _f32(v1, "v'").astype(np.float64), what)


def check_within_bound(a32, b64, bound, what):
    err = np.abs(np.asarray(a32, dtype=np.float64) - b64)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (f"{what}: {bad.size} of {err.size} entries outside the bound, first at {bad[0]}: error "
                           f"{err[bad[0]]:.3e} > {np.broadcast_to(bound, err.shape)[bad[0]]:.3e}")


# ---------------------------------------------------------------------------
# inputs
def optim_inputs(n, seed=0, lo=0.0):
    """p >= lo with entries at the clamp, g = +-2^k for k uniform in [-60, 20] times [1, 2) with exact
    zeros, m of g's size order, v >= 0 with exact zeros.  fp32."""
    rng = np.random.default_rng(seed)
    mag = lambda: np.ldexp(1.0 + rng.random(n), rng.integers(-60, 21, n)) * rng.choice([-1.0, 1.0], n)
    g = mag()
    g[rng.random(n) < 0.2] = 0.0
    if n > 2:
        g[1] = -0.0
    p = rng.random(n) + (lo if np.isfinite(lo) else 0.0)
    p[rng.random(n) < 0.25] = lo if np.isfinite(lo) else 0.0
    m = 0.1 * mag()
    v = (0.01 * mag()) ** 2
    v[rng.random(n) < 0.3] = 0.0
    s = 0.5 * mag()
    return tuple(a.astype(np.float32) for a in (p, g, m, v, s))

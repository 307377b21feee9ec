"""Reference models, tolerances and checkers for the optimiser's vector and loss kernels
(tvam_vec.hip: history, partials, direction, coefficient lane, update; tvam_kernels.hip:
tvam_loss_threshold*, tvam_target_mask).  Numpy only, no GPU: the checkers take a kernel's
inputs and outputs as arrays and raise AssertionError; tests/test_vec_model.py runs them on
numpy stand-ins with deliberate defects, tests/test_gpu_vec_kernels.py on the HIP kernels.

Number formats: inputs are fp32 arrays, u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64).
A product of two fp32 numbers has at most 48 significant bits, so it is exact in float64;
every model below that forms such products in float64 relies on that.
"""
import math

import numpy as np

U = 2.0 ** -24     # fp32 unit roundoff
V = 2.0 ** -53     # fp64 unit roundoff
TINY = 2.0 ** -126  # smallest normal fp32
GUARD = 64         # sentinel floats (NaN) on each side of an output
FSUM_MAX = 1 << 16  # longest sum taken with math.fsum (exact); longer ones by the pairwise tree

# max_i |d_gram - d_vec|_i / M_i between the Gram-form chain (NumpyVecLib history + coef +
# direction, tests/test_lbfgs_fused.py) and the vector-form two-loop recursion below, and the same
# for g.d relative to sum |terms|: reference against reference, over H in {1, 4, 8} x first in
# {0, 1} on chain_inputs().  Measured with
#   python -c "import sys; sys.path.insert(0, 'tests'); import test_vec_model as t; print(t.measure_gram_vec_gap())"
# -> (9.75e-08, 4.5e-16); the larger, rounded up, is recorded.  The GPU chain tolerance is
# (2h + 3) u M_i + 4 x this (the gap is the coefficients' fp32 rounding and the Gram solve's
# conditioning, which move by small factors with the draw).
GRAM_VEC_GAP = 1.0e-7


def _f32(a, name="input"):
    a = np.asarray(a)
    assert a.dtype == np.float32, f"{name}: fp32 array expected, got {a.dtype}"
    return a


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} entries differ bit for bit, first at {bad[0]}: "
                           f"{got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}")


# ---------------------------------------------------------------------------
# sums
def tree_sum(x):
    """Pairwise float64 sum over a balanced tree (zero-padded to a power of two): its error is at
    most ceil(log2 n) v sum|x| (every level rounds each partial once)."""
    x = np.asarray(x, dtype=np.float64)
    m = 1 << max(0, (x.size - 1).bit_length())
    if m != x.size:
        x = np.concatenate([x, np.zeros(m - x.size)])
    while x.size > 1:
        x = x[0::2] + x[1::2]
    return float(x[0]) if x.size else 0.0


def sum_error(value, terms):
    """|value - sum(terms)| and the slack of that figure itself.  Up to FSUM_MAX terms:
    math.fsum([value, -t_0, -t_1, ...]) is the correctly rounded difference (slack 0).  Longer:
    the tree sum, whose own bound ceil(log2 n) v sum|terms| is the slack."""
    terms = np.asarray(terms, dtype=np.float64)
    if terms.size <= FSUM_MAX:
        return abs(math.fsum([float(value)] + (-terms).tolist())), 0.0
    slack = math.ceil(math.log2(terms.size)) * V * float(np.abs(terms).sum())
    return abs(float(value) - tree_sum(terms)), slack


def check_sum(value, terms, what, n=None):
    """An fp64 accumulation of the n terms in any order (per thread, warp, block, then over blocks;
    or atomics): every one of its at most n roundings is at most v of a partial sum <= sum|terms|,
    so |value - sum| <= n v sum|terms|.  Returns that bound."""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.size if n is None else n
    bound = n * V * float(np.abs(terms).sum())
    assert np.isfinite(value), f"{what}: {value!r}"
    err, slack = sum_error(value, terms)
    assert err <= bound + slack, f"{what}: error {err:.3e} > bound {bound:.3e} (+ reference slack {slack:.1e})"
    return bound


# ---------------------------------------------------------------------------
# sentinels
def check_guards(whole, start, n, what):
    """An output of n floats at whole[start:start + n]; everything else of whole is NaN sentinel."""
    whole = np.asarray(whole).ravel()
    out = np.ones(whole.size, dtype=bool)
    out[start:start + n] = False
    bad = np.flatnonzero(out & ~np.isnan(whole))
    assert bad.size == 0, f"{what}: {bad.size} sentinel(s) overwritten, first at offset {bad[0] - start} of [0, {n})"


def check_untouched(vec, idx, what):
    """A band write into a NaN-filled vector: only the entries idx may have been written."""
    vec = np.asarray(vec).ravel()
    out = np.ones(vec.size, dtype=bool)
    out[idx] = False
    bad = np.flatnonzero(out & ~np.isnan(vec))
    assert bad.size == 0, f"{what}: {bad.size} entries outside the band written, first at {bad[0]}"


def band_index(nseg, seg_len, seg_stride, seg_off):
    """Entries seg_off + a seg_stride + [0, seg_len) of every a < nseg (tvam.h, the _rows entries)."""
    return (seg_off + np.arange(nseg)[:, None] * seg_stride + np.arange(seg_len)[None, :]).ravel()


# ---------------------------------------------------------------------------
# history
def hist_ndots(h, new):
    """HistLayout (tvam_vec.hip) / tvam.h: HT = h + new; 2 HT + 1 dots, or 5 HT + 1 with a new pair."""
    ht = h + (1 if new else 0)
    return (5 * ht if new else 2 * ht) + 1


def hist_inputs(n, h, seed=0):
    """g, h pairs S = 0.1 N(0, 1), Y = 0.5 S + 0.05 N(0, 1), and p, p_old, g_old of a new pair.  fp32."""
    rng = np.random.default_rng(seed)
    nrm = lambda: rng.standard_normal(n, dtype=np.float32)
    g = nrm()
    S = [np.float32(0.1) * nrm() for _ in range(h)]
    Y = [np.float32(0.5) * s + np.float32(0.05) * nrm() for s in S]
    p, p_old = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    return g, S, Y, p, p_old, nrm()


def history_pairs(g, S, Y, s_new=None, y_new=None):
    """The dots in the documented order, as (name, a, b) factor pairs: s_j.g | y_j.g | (with a new
    pair, j over the retained pairs then the new one) s_new.y_j | s_j.y_new | y_new.y_j | g.g."""
    new = s_new is not None
    Sv = list(S) + ([s_new] if new else [])
    Yv = list(Y) + ([y_new] if new else [])
    out = [(f"s_{j}.g", s, g) for j, s in enumerate(Sv)] + [(f"y_{j}.g", y, g) for j, y in enumerate(Yv)]
    if new:
        out += [(f"s_new.y_{j}", s_new, y) for j, y in enumerate(Yv)]
        out += [(f"s_{j}.y_new", s, y_new) for j, s in enumerate(Sv)]
        out += [(f"y_new.y_{j}", y_new, y) for j, y in enumerate(Yv)]
    out.append(("g.g", g, g))
    return out


def history_new_pair(g, p=None, p_old=None, g_old=None, s_pre=None):
    """s_new = fl32(p - p_old) (or the precomputed s), y_new = fl32(g - g_old); None, None without
    a new pair."""
    if g_old is None:
        assert p_old is None and s_pre is None
        return None, None
    s = _f32(s_pre, "s_pre") if p_old is None else _f32(p, "p") - _f32(p_old, "p_old")
    return s, _f32(g, "g") - _f32(g_old, "g_old")


def check_history(dots, g, S, Y, p=None, p_old=None, g_old=None, s_pre=None, s_new=None, y_new=None, what="history"):
    """tvam_lbfgs_history (p, p_old, g_old: a new pair from p - p_old; s_pre, g_old: the SPRE form;
    neither: no new pair), or a band of tvam_lbfgs_history_rows on its gathered entries.
    s_new / y_new (the kernel's, when given) bit for bit; every dot within n v sum|product_i| of the
    exact sum of the exact products (check_sum).  Returns the bounds, one per dot."""
    g = _f32(g, "g")
    S, Y = [_f32(s, "S") for s in S], [_f32(y, "Y") for y in Y]
    sm, ym = history_new_pair(g, p, p_old, g_old, s_pre)
    new = sm is not None
    if new:
        if s_new is not None:
            assert_bits_equal(s_new, sm, f"{what}: s_new")
        if y_new is not None:
            assert_bits_equal(y_new, ym, f"{what}: y_new")
    dots = np.asarray(dots)
    assert dots.dtype == np.float64 and dots.shape == (hist_ndots(len(S), new),), \
        f"{what}: {hist_ndots(len(S), new)} f64 dots expected, got {dots.dtype} {dots.shape}"
    bounds = []
    for k, (name, a, b) in enumerate(history_pairs(g, S, Y, sm, ym)):
        prod = a.astype(np.float64) * b.astype(np.float64)  # exact
        bounds.append(check_sum(dots[k], prod, f"{what}: dot {k} ({name}), n = {g.size}"))
    return np.array(bounds)


# ---------------------------------------------------------------------------
# direction
def direction_model(g, S, Y, cg, cs, cy):
    """float64 value of cg g + sum_j (cs_j s_j + cy_j y_j) and M_i = |cg g_i| + sum_j (|cs_j s_ij| +
    |cy_j y_ij|), coefficients rounded to fp32 as the kernel receives them."""
    g = _f32(g, "g").astype(np.float64)
    cg = float(np.float32(cg))
    d = cg * g
    M = np.abs(d)
    for j, (s, y) in enumerate(zip(S, Y)):
        a = float(np.float32(cs[j])) * _f32(s, "S").astype(np.float64)
        b = float(np.float32(cy[j])) * _f32(y, "Y").astype(np.float64)
        d = d + a + b
        M = M + np.abs(a) + np.abs(b)
    return d, M


def check_direction(d, g, S, Y, cg, cs, cy, what="direction"):
    """|d_i - exact_i| <= (2h + 2) (u + v) M_i: the kernel rounds the product cg g_i once and each of
    its 2h fmas once (2h + 1 roundings, every partial at most M_i in size, counted as 2h + 2); the
    float64 evaluation of the model rounds as often, at v."""
    h = len(S)
    ref, M = direction_model(g, S, Y, cg, cs, cy)
    d = _f32(d, "d").astype(np.float64)
    assert d.shape == ref.shape, f"{what}: shape {d.shape} != {ref.shape}"
    assert np.all(np.isfinite(d)), f"{what}: non-finite entries"
    tol = (2 * h + 2) * (U + V) * M
    bad = np.flatnonzero(np.abs(d - ref) > tol)
    assert bad.size == 0, (f"{what}: {bad.size} of {d.size} entries off, first at {bad[0]}: {d[bad[0]]!r} vs "
                           f"{ref[bad[0]]!r}, tolerance {tol[bad[0]]:.3e}")


# ---------------------------------------------------------------------------
# update
def check_axpy(out, p, alpha, d, lo, s_out=None, what="axpy_clamp"):
    """out within u max(|exact|, 2^-126) (+ v |exact| for the model's own sum) of exact = max(p +
    alpha d, lo): alpha d is exact in float64, the kernel's fma rounds p + alpha d once to fp32
    (half a spacing: u |exact|, and u 2^-126 below the normal range) and max() is exact.  s_out
    bit-equal to fl32(out - p) of the kernel's own out."""
    p, d, out = _f32(p, "p"), _f32(d, "d"), _f32(out, "out")
    assert out.shape == p.shape, f"{what}: shape {out.shape} != {p.shape}"
    exact = np.maximum(p.astype(np.float64) + float(np.float32(alpha)) * d.astype(np.float64), float(lo))
    tol = U * np.maximum(np.abs(exact), TINY) + V * np.abs(exact)
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(~(np.abs(out.astype(np.float64) - exact) <= tol))
    assert bad.size == 0, (f"{what}: {bad.size} of {out.size} entries off, first at {bad[0]}: {out[bad[0]]!r} vs "
                           f"{exact[bad[0]]!r}")
    if s_out is not None:
        assert_bits_equal(_f32(s_out, "s_out"), out - p, f"{what}: s_out")


# ---------------------------------------------------------------------------
# loss
class SubnormalInput(ValueError):
    """A nonzero intermediate of the fp32 loss model below 2^-126: fp32 subnormal handling would
    decide the comparison, so the model refuses the input."""


def _guard(a, name):
    bad = (a != 0) & (np.abs(a) < np.float32(TINY))
    if np.any(bad):
        i = int(np.flatnonzero(bad)[0])
        raise SubnormalInput(f"{name}: nonzero value {a.ravel()[i]!r} below 2^-126 at {i}")
    return a


def _powi32(x, K, name):
    """tvam_powi: r = 1; r *= x, K times (fp32)."""
    r = np.ones_like(x)
    for k in range(K):
        r = _guard(r * x, f"{name}^{k + 1}")
    return r


def loss_params32(tl, tu, w_object, w_void, w_limit, scale):
    return tuple(np.float32(v) for v in (tl, tu, w_object, w_void, w_limit, scale))


def loss_level_a(x, obj, K, tl, tu, w_object, w_void, w_limit, scale, want_grad=True):
    """Level A: the kernels' per-element fp32 arithmetic in their operation order, no contraction
    (tvam_loss_grad_elem / tvam_loss_elem): object (obj) w_object ro^K + w_limit rl^K with ro =
    relu(tu - x), rl = relu(x - 1); void w_void rv^K with rv = relu(x - tl); gradient
    ((-/+ w K) r^(K - 1)) scale where the relu's argument is > 0, else 0.  Returns fp32 (elements,
    gradient)."""
    x = _f32(x, "x")
    tl, tu, wo, wv, wl, sc = loss_params32(tl, tu, w_object, w_void, w_limit, scale)
    obj = np.asarray(obj, dtype=bool)
    one, zero, Kf = np.float32(1), np.float32(0), np.float32(K)
    zo, zl, zv = _guard(tu - x, "tu - x"), _guard(x - one, "x - 1"), _guard(x - tl, "x - tl")
    po, pl, pv = zo > 0, zl > 0, zv > 0
    ro, rl, rv = np.where(po, zo, zero), np.where(pl, zl, zero), np.where(pv, zv, zero)
    v_obj = _guard(wo * _powi32(ro, K, "ro"), "w_object ro^K") + _guard(wl * _powi32(rl, K, "rl"), "w_limit rl^K")
    v_void = _guard(wv * _powi32(rv, K, "rv"), "w_void rv^K")
    val = np.where(obj, _guard(v_obj, "object value"), v_void).astype(np.float32)
    if not want_grad:
        return val, None
    g_obj = (np.where(po, _guard((-wo * Kf) * _powi32(ro, K - 1, "ro"), "object gradient"), zero) +
             np.where(pl, _guard((wl * Kf) * _powi32(rl, K - 1, "rl"), "limit gradient"), zero))
    g_void = np.where(pv, _guard((wv * Kf) * _powi32(rv, K - 1, "rv"), "void gradient"), zero)
    grad = _guard(np.where(obj, g_obj, g_void).astype(np.float32) * sc, "gradient x scale")
    return val, grad.astype(np.float32)


def loss_level_b(x, obj, K, tl, tu, w_object, w_void, w_limit, scale):
    """Level B: ThresholdedLoss.eval (loss.py:82-132) in float64 with the fp32-rounded parameters:
    where(target > 0, w_object relu(tu - x)^K + w_limit relu(x - 1)^K, w_void relu(x - tl)^K) and its
    derivative times scale (0 at and below a relu's kink).  Returns float64 (elements, gradient)."""
    x = _f32(x, "x").astype(np.float64)
    tl, tu, wo, wv, wl, sc = (float(v) for v in loss_params32(tl, tu, w_object, w_void, w_limit, scale))
    obj = np.asarray(obj, dtype=bool)
    ro, rl, rv = np.maximum(tu - x, 0.0), np.maximum(x - 1.0, 0.0), np.maximum(x - tl, 0.0)
    val = np.where(obj, wo * ro ** K + wl * rl ** K, wv * rv ** K)
    dpow = lambda r: np.where(r > 0, K * r ** (K - 1), 0.0)
    grad = np.where(obj, -wo * dpow(ro) + wl * dpow(rl), wv * dpow(rv)) * sc
    return val, grad


def check_level_a_against_b(x, obj, K, *params):
    """Per element, level A within (2K + 2) u of level B, value and gradient, identical zero sets:
    the fp32 value takes one rounding for the relu's argument, K - 1 for the power, one for the
    weight (K + 1); the gradient one more for the scale."""
    va, ga = loss_level_a(x, obj, K, *params)
    vb, gb = loss_level_b(x, obj, K, *params)
    for name, a, b in (("value", va, vb), ("gradient", ga, gb)):
        assert np.array_equal(a == 0, b == 0), f"K = {K}: zero sets of the {name} differ"
        ratio = np.abs(a.astype(np.float64) - b) / np.where(b != 0, np.abs(b), 1.0)
        assert ratio.max() <= (2 * K + 2) * U, f"K = {K} {name}: {ratio.max() / ((2 * K + 2) * U):.3f} of the bound"
    return va, ga


def fma32(alpha, dx, x0):
    """fmaf(alpha, dx, x0) for inputs whose float64 alpha dx + x0 is exact (asserted: the product of
    two fp32 numbers always is; the sum by its TwoSum error term), so that the one rounding to fp32
    is the fma's."""
    a = float(np.float32(alpha))
    t = a * _f32(dx, "ddose").astype(np.float64)
    x0 = _f32(x0, "dose").astype(np.float64)
    s = t + x0
    bb = s - t
    err = (t - (s - bb)) + (x0 - bb)
    assert not np.any(err), "alpha dx + x0 is not exact in float64: choose inputs on a coarser grid"
    return s.astype(np.float32)


def loss_thresholds(tl, tu):
    return [np.float32(tl), np.float32(tu), np.float32(1.0)]


def snap(x, tl, tu):
    """Every x with 0 < |x - t| < 2^-7 for t in {tl, tu, 1} becomes t exactly (so that powers up to
    K = 16 of a relu's argument stay normal fp32 numbers, and the kinks themselves are hit)."""
    x = _f32(x).copy()
    for t in loss_thresholds(tl, tu):
        x[np.abs(x - t) < np.float32(2.0 ** -7)] = t
    return x


def loss_inputs(n, seed, tl, tu):
    """x uniform in [0, 1.3), snapped; a target with 0, -0, negative, positive and greyscale values."""
    rng = np.random.default_rng(seed)
    x = snap((rng.random(n) * 1.3).astype(np.float32), tl, tu)
    r = rng.random(n)
    target = np.select([r < 0.35, r < 0.45, r < 0.5, r < 0.75], [0.0, -0.0, -r, 1.0], r).astype(np.float32)
    return x, target


def probe_inputs(n, seed, alphas, tl, tu):
    """dose and ddose on a 2^-12 grid (step sizes of <= 11 significant bits: alpha dx + x0 exact in
    float64); an element whose x = fmaf(alpha, dx, x0) falls within 2^-7 of a threshold without
    hitting it, for any alpha, gets dose 0.5 and ddose 0 instead (snap() for the two-array form)."""
    rng = np.random.default_rng(seed)
    x0 = (np.floor(rng.random(n) * 1.3 * 4096) / 4096).astype(np.float32)
    dx = (np.round(rng.standard_normal(n) * 0.2 * 4096) / 4096).astype(np.float32)
    bad = np.zeros(n, dtype=bool)
    for a in alphas:
        x = fma32(a, dx, x0)
        for t in loss_thresholds(tl, tu):
            bad |= (x != t) & (np.abs(x - t) < np.float32(2.0 ** -7))
    x0[bad], dx[bad] = 0.5, 0.0
    r = rng.random(n)
    target = np.select([r < 0.35, r < 0.45, r < 0.5, r < 0.75], [0.0, -0.0, -r, 1.0], r).astype(np.float32)
    return x0, dx, target


def check_loss(value, x, obj, K, params, grad=None, what="loss", model=None):
    """A loss kernel's value (and gradient) for the elements x (fp32, after any fma) and object flags
    obj.  value within n v scale sum|element| of scale sum(level-A elements), the elements' sum being
    an fp64 accumulation in any order (scale x element is exact in float64); gradient bit for bit
    level A's.  model: loss_level_a's result for these inputs, when the caller already has it."""
    sc = params[-1]
    va, ga = model if model is not None else loss_level_a(x, obj, K, *params, want_grad=grad is not None)
    terms = float(np.float32(sc)) * va.astype(np.float64)  # exact
    check_sum(float(value), terms, f"{what}: value (K = {K}, n = {va.size})")
    if grad is not None:
        assert_bits_equal(_f32(grad, "grad"), ga, f"{what}: gradient (K = {K})")


# ---------------------------------------------------------------------------
# target mask
def mask_model(target):
    """Bit i % 32 of word i / 32 = target[i] > 0; bits past n are 0."""
    b = np.packbits(_f32(target, "target") > 0, bitorder="little")
    b = np.concatenate([b, np.zeros(-b.size % 4, dtype=np.uint8)])
    return b.view("<u4")


def mask_bits(words, bit0, n):
    """The object flags of n elements read from a mask at bit offset bit0."""
    w = np.ascontiguousarray(words).view(np.uint8)
    lo = bit0 // 8
    return np.unpackbits(w[lo:(bit0 + n + 7) // 8], bitorder="little")[bit0 - 8 * lo:bit0 - 8 * lo + n].astype(bool)


def check_target_mask(words, target, what="target mask"):
    want = mask_model(target)
    got = np.ascontiguousarray(words).view("<u4")
    assert got.shape == want.shape, f"{what}: {want.size} words expected, got {got.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[0]}: {got[bad[0]]:#010x} != {want[bad[0]]:#010x}"


# ---------------------------------------------------------------------------
# coefficients and the chain
def two_loop(g, S, Y, first):
    """The textbook two-loop recursion (lbfgs.py:221-243 of the reference) on the vectors themselves,
    float64: q = g; a_i = (s_i.q) / (y_i.s_i), q -= a_i y_i (newest first); z = gamma q with gamma =
    1 on the first step, else y.s / y.y of the newest pair; b_i = (y_i.z) / (y_i.s_i), z += (a_i - b_i)
    s_i (oldest first); d = -z.  Returns d, g.d and the coefficients (cg, cs, cy) of d = cg g +
    sum cs_j s_j + cy_j y_j that the recursion implies (cg = -gamma, cs_j = -(a_j - b_j), cy_j = gamma a_j)."""
    g = np.asarray(g, dtype=np.float64)
    S = [np.asarray(s, dtype=np.float64) for s in S]
    Y = [np.asarray(y, dtype=np.float64) for y in Y]
    h = len(S)
    q = g.copy()
    a, b = np.zeros(h), np.zeros(h)
    ys = [float(Y[i] @ S[i]) for i in range(h)]
    for i in range(h - 1, -1, -1):
        a[i] = float(S[i] @ q) / ys[i]
        q -= a[i] * Y[i]
    gamma = 1.0 if (first or h == 0) else ys[-1] / float(Y[-1] @ Y[-1])
    z = gamma * q
    for i in range(h):
        b[i] = float(Y[i] @ z) / ys[i]
        z += (a[i] - b[i]) * S[i]
    d = -z
    return d, float(g @ d), (-gamma, -(a - b), gamma * a)


def chain_inputs(n, H, seed=0):
    """The chain test's vectors: S = 0.1 N(0, 1), Y = 0.5 S + 0.05 N(0, 1) (s.y > 0) for H pairs, the
    newest given as p, p_old, g_old with p - p_old ~ S[-1], g - g_old ~ Y[-1].  fp32."""
    rng = np.random.default_rng(1000 + 10 * seed + H)
    g = rng.standard_normal(n).astype(np.float32)
    S = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(H)]
    Y = [(0.5 * s + 0.05 * rng.standard_normal(n)).astype(np.float32) for s in S]
    p_old = rng.random(n).astype(np.float32)
    p = p_old + S[-1]
    g_old = g - Y[-1]
    return g, S[:-1], Y[:-1], p, p_old, g_old


def chain_tolerance(h):
    """Relative to M_i (and, for g.d, to sum |terms|): 2h + 2 roundings of the direction pass and one
    of every coefficient to fp32 (each term of M_i once: 2h + 3 in all), plus 4 x the recorded gap
    between the Gram form and the vector form of the recursion."""
    return (2 * h + 3) * U + 4 * GRAM_VEC_GAP


def chain_model(g, S, Y, first):
    d, gd, (cg, cs, cy) = two_loop(g, S, Y, first)
    g64 = np.asarray(g, dtype=np.float64)
    M = np.abs(cg * g64)
    gd_terms = [cg * float(g64 @ g64)]
    for j in range(len(S)):
        s, y = np.asarray(S[j], dtype=np.float64), np.asarray(Y[j], dtype=np.float64)
        M = M + np.abs(cs[j] * s) + np.abs(cy[j] * y)
        gd_terms += [cs[j] * float(s @ g64), cy[j] * float(y @ g64)]
    return d, M, gd, float(np.abs(gd_terms).sum())


def chain_gaps(d, gdz, g, S, Y, first):
    """max_i |d - d_vec|_i / M_i and |gdz - g.d_vec| / sum|terms| against the two-loop model."""
    ref, M, gd, gd_abs = chain_model(g, S, Y, first)
    return float(np.max(np.abs(np.asarray(d, dtype=np.float64) - ref) / M)), abs(float(gdz) - gd) / gd_abs


def check_chain(d, gdz, g, S, Y, first, what="chain"):
    """history + coef + direction_dev against the two-loop model: d within chain_tolerance(h) M_i, gdz
    within chain_tolerance(h) sum|terms| of g.d."""
    h = len(S)
    assert np.all(np.isfinite(d)) and np.isfinite(gdz), f"{what}: non-finite output"
    gap_d, gap_gd = chain_gaps(_f32(d, "d"), gdz, g, S, Y, first)
    tol = chain_tolerance(h)
    assert gap_d <= tol, f"{what}: direction off by {gap_d:.3e} M_i, tolerance {tol:.3e}"
    assert gap_gd <= tol, f"{what}: g.d off by {gap_gd:.3e} of sum|terms|, tolerance {tol:.3e}"

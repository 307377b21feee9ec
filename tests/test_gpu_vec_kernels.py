"""GPU: the L-BFGS vector kernels (tvam_vec.hip: history, partials, direction, coefficient lane,
update) and the loss kernels (tvam_kernels.hip: tvam_loss_threshold*, tvam_target_mask) against the
float64 / level-A models of tests/vec_model.py, through the C entries.  Every output lies inside a
larger buffer with NaN sentinels on both sides, which must survive the call.  No TVAM_VEC_* knob is
set (they are read once per process): the second grid-stride trip is reached by size."""
import ctypes

import numpy as np
import pytest
import torch

import vec_model as vm
from drtvam_amd import _abi

pytestmark = pytest.mark.gpu

# launch geometry (defaults of tvam_vec.hip: hist_grid(), dir_grid(), tvam_launch_axpy_clamp; of
# tvam_kernels.hip: tvam_launch_loss_threshold / _probes, tvam_launch_target_mask), 256 threads each
HIST_SWEEP = 768 * 256 * 4         # elements of one sweep of the history pass
DIR_SWEEP = 1024 * 256 * 4         # of the direction pass
AXPY_SWEEP = 2048 * 256 * 4        # of the update and of the loss (float4 path)
LOSS_SCALAR_SWEEP = 2048 * 256     # of the loss's scalar path
MASK_SWEEP = 4096 * 256 * 32       # of the mask kernel (one word per thread)
N_ODD = 4 * 1031 + 3
SMALL = [1, 3, 4, 7, N_ODD]
WRAP = AXPY_SWEEP + 4 * 300 + 3    # past one sweep of every vector kernel, with a float4 remainder and a tail
assert WRAP > max(HIST_SWEEP, DIR_SWEEP, AXPY_SWEEP, LOSS_SCALAR_SWEEP) and WRAP % 4 == 3
MASK_LARGE = MASK_SWEEP + 45
G = vm.GUARD

TL, TU = 0.85, 0.95
WEIGHTS = (1.0, 1.3, 0.7)  # object, void, limit
ALPHAS = [1.0, 0.5, 0.25, 0.125, 2.0 ** -7, 3.0, 0.0, -0.5]  # <= 11 significant bits each


def _params(scale):
    return (TL, TU) + WEIGHTS + (scale,)


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """n entries at [G + off, G + off + n) of a NaN-filled device buffer (off: floats off the 16-byte grid)."""

    def __init__(self, n, off=0, dtype=torch.float32, init=None):
        self.n, self.start = n, G + off
        self.whole = torch.full((n + 2 * G + 4,), float("nan"), dtype=dtype, device="cuda")
        self.view = self.whole[self.start:self.start + n]
        if init is not None:
            self.view.copy_(torch.as_tensor(init))
        assert (self.whole.data_ptr() + 4 * G) % 16 == 0

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self, what):
        w = self.whole.cpu().numpy()
        vm.check_guards(w, self.start, self.n, what)
        return w[self.start:self.start + self.n].copy()


def ptrs(ts):
    return (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])


def _work():
    return torch.empty(_abi.LBFGS_WORK_DOUBLES, dtype=torch.float64, device="cuda")


# ---------------------------------------------------------------------------
# history
def run_history(lib, n, h, mode, seed=0):
    """mode: 'none' (no new pair), 'new' (from p, p_old), 'spre' (s_new precomputed)."""
    g, S, Y, p, p_old, g_old = vm.hist_inputs(n, h, seed)
    gd, Sd, Yd = dev(g), [dev(s) for s in S], [dev(y) for y in Y]
    new = mode != "none"
    s_pre = p - p_old
    nd = vm.hist_ndots(h, new)
    args = {}
    if new:
        pd, pod, god = dev(p), dev(p_old), dev(g_old)
        s_new = Guarded(n, init=s_pre if mode == "spre" else None)
        y_new = Guarded(n)
        args = dict(g_old=g_old, **(dict(s_pre=s_pre) if mode == "spre" else dict(p=p, p_old=p_old)))
    work = _work()
    got = []
    for _ in range(2):  # the same call twice: bit-identical dots
        dots = Guarded(nd, dtype=torch.float64)
        rc = lib.tvam_lbfgs_history(n, pd.data_ptr() if mode == "new" else None, pod.data_ptr() if mode == "new" else None,
                                    gd.data_ptr(), god.data_ptr() if new else None, h, ptrs(Sd), ptrs(Yd),
                                    s_new.ptr if new else None, y_new.ptr if new else None, work.data_ptr(), dots.ptr,
                                    _stream())
        _abi.check(rc)
        got.append(dots.get(f"dots (n = {n}, h = {h}, {mode})"))
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64)), "dots differ between two identical calls"
    vm.check_history(got[0], g, S, Y, s_new=s_new.get("s_new") if new else None,
                     y_new=y_new.get("y_new") if new else None, what=f"history n = {n}, h = {h}, {mode}", **args)


@pytest.mark.parametrize("mode", ["none", "new", "spre"])
@pytest.mark.parametrize("h", range(8))
def test_history_every_depth(lib, h, mode):
    run_history(lib, N_ODD, h, mode, seed=h)


@pytest.mark.parametrize("mode", ["new", "spre"])
@pytest.mark.parametrize("h", [0, 7])
def test_history_small_sizes(lib, h, mode):
    for n in SMALL[:-1]:
        run_history(lib, n, h, mode, seed=n)


@pytest.mark.parametrize("mode", ["new", "spre"])
@pytest.mark.parametrize("h", [0, 7])
def test_history_second_sweep(lib, h, mode):
    run_history(lib, WRAP, h, mode, seed=5)


# ---------------------------------------------------------------------------
# history rows and direction rows
ROWS = (7, 36, 44)  # segments (angles), rows, columns
BANDS = ((0, 5), (5, 21), (21, 36))


@pytest.mark.parametrize("new", [False, True])
@pytest.mark.parametrize("h", [0, 3, 7])
def test_history_rows(lib, h, new):
    A, R, C = ROWS
    n = A * R * C
    g, S, Y, p, p_old, g_old = vm.hist_inputs(n, h, seed=20 + h)
    gd, Sd, Yd, pd, pod, god = dev(g), [dev(s) for s in S], [dev(y) for y in Y], dev(p), dev(p_old), dev(g_old)
    nd = vm.hist_ndots(h, new)
    work = _work()
    total = np.zeros(nd)
    s_all, y_all = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    for r0, r1 in BANDS:
        idx = vm.band_index(A, (r1 - r0) * C, R * C, r0 * C)
        s_new, y_new, dots = Guarded(n), Guarded(n), Guarded(nd, dtype=torch.float64)
        _abi.check(lib.tvam_lbfgs_history_rows(A, (r1 - r0) * C, R * C, r0 * C, pd.data_ptr() if new else None,
                                               pod.data_ptr() if new else None, gd.data_ptr(),
                                               god.data_ptr() if new else None, h, ptrs(Sd), ptrs(Yd),
                                               s_new.ptr if new else None, y_new.ptr if new else None,
                                               work.data_ptr(), dots.ptr, _stream()))
        what = f"history_rows band {r0}:{r1}, h = {h}"
        sb, yb, db = s_new.get(what + " s_new"), y_new.get(what + " y_new"), dots.get(what + " dots")
        vm.check_untouched(sb, idx if new else [], what + " s_new")
        vm.check_untouched(yb, idx if new else [], what + " y_new")
        gi = lambda v: v[idx]
        vm.check_history(db, gi(g), [gi(s) for s in S], [gi(y) for y in Y], what=what,
                         **(dict(p=gi(p), p_old=gi(p_old), g_old=gi(g_old), s_new=sb[idx], y_new=yb[idx]) if new else {}))
        s_all[idx], y_all[idx] = sb[idx], yb[idx]
        total += db  # summed in band order, as the caller does before tvam_lbfgs_coef
    vm.check_history(total, g, S, Y, what=f"history_rows summed over the bands, h = {h}",
                     **(dict(p=p, p_old=p_old, g_old=g_old, s_new=s_all, y_new=y_all) if new else {}))


@pytest.mark.parametrize("h", [0, 3, 7, 8])
def test_direction_rows(lib, h):
    A, R, C = ROWS
    n = A * R * C
    g, S, Y, _, _, _ = vm.hist_inputs(n, h, seed=30 + h)
    gd, Sd, Yd = dev(g), [dev(s) for s in S], [dev(y) for y in Y]
    coef = np.random.default_rng(31).standard_normal(17).astype(np.float32)
    cd = dev(coef)
    for r0, r1 in BANDS:
        idx = vm.band_index(A, (r1 - r0) * C, R * C, r0 * C)
        d = Guarded(n)
        _abi.check(lib.tvam_lbfgs_direction_rows(A, (r1 - r0) * C, R * C, r0 * C, gd.data_ptr(), h, ptrs(Sd), ptrs(Yd),
                                                 cd.data_ptr(), d.ptr, _stream()))
        what = f"direction_rows band {r0}:{r1}, h = {h}"
        db = d.get(what)
        vm.check_untouched(db, idx, what)
        vm.check_direction(db[idx], g[idx], [s[idx] for s in S], [y[idx] for y in Y], coef[0], coef[1:9], coef[9:17], what)


# ---------------------------------------------------------------------------
# direction
def run_direction(lib, n, h, seed=0):
    g, S, Y, _, _, _ = vm.hist_inputs(n, h, seed)
    gd, Sd, Yd = dev(g), [dev(s) for s in S], [dev(y) for y in Y]
    coef = np.random.default_rng(seed + 1).standard_normal(17).astype(np.float32)
    cs, cy = coef[1:9], coef[9:17]
    d = Guarded(n)
    _abi.check(lib.tvam_lbfgs_direction(n, gd.data_ptr(), h, ptrs(Sd), ptrs(Yd), float(coef[0]),
                                        (ctypes.c_float * 8)(*cs.tolist()), (ctypes.c_float * 8)(*cy.tolist()), d.ptr,
                                        _stream()))
    by_value = d.get(f"direction n = {n}, h = {h}")
    vm.check_direction(by_value, g, S, Y, coef[0], cs, cy, f"direction n = {n}, h = {h}")
    d, cd = Guarded(n), dev(coef)
    _abi.check(lib.tvam_lbfgs_direction_dev(n, gd.data_ptr(), h, ptrs(Sd), ptrs(Yd), cd.data_ptr(), d.ptr, _stream()))
    vm.check_direction(d.get(f"direction_dev n = {n}, h = {h}"), g, S, Y, coef[0], cs, cy,
                       f"direction_dev n = {n}, h = {h}")


@pytest.mark.parametrize("h", range(9))
def test_direction_every_depth(lib, h):
    run_direction(lib, N_ODD, h, seed=40 + h)


@pytest.mark.parametrize("h", [0, 8])
def test_direction_sizes(lib, h):
    for n in SMALL[:-1] + [WRAP]:
        run_direction(lib, n, h, seed=n % 97)


# ---------------------------------------------------------------------------
# update
@pytest.mark.parametrize("lo", [0.0, -np.inf])
@pytest.mark.parametrize("alpha", [0.25, 0.3, 0.0])
def test_axpy_clamp(lib, alpha, lo):
    for n in SMALL + [WRAP]:
        rng = np.random.default_rng(n % 89)
        p, d = rng.random(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
        pd, dd, ad = dev(p), dev(d), dev(np.array([alpha], np.float32))
        what = f"n = {n}, alpha = {alpha}, lo = {lo}"
        out = Guarded(n)
        _abi.check(lib.tvam_axpy_clamp(n, pd.data_ptr(), alpha, dd.data_ptr(), lo, out.ptr, _stream()))
        vm.check_axpy(out.get("axpy_clamp " + what), p, alpha, d, lo, what="axpy_clamp " + what)
        out = Guarded(n)
        _abi.check(lib.tvam_axpy_clamp_dev(n, pd.data_ptr(), ad.data_ptr(), dd.data_ptr(), lo, out.ptr, None, _stream()))
        vm.check_axpy(out.get("axpy_clamp_dev " + what), p, alpha, d, lo, what="axpy_clamp_dev " + what)
        out, s_out = Guarded(n), Guarded(n)
        _abi.check(lib.tvam_axpy_clamp_dev(n, pd.data_ptr(), ad.data_ptr(), dd.data_ptr(), lo, out.ptr, s_out.ptr,
                                           _stream()))
        vm.check_axpy(out.get("axpy_clamp_dev out " + what), p, alpha, d, lo, s_out=s_out.get("s_out " + what),
                      what="axpy_clamp_dev with s_out " + what)


def test_axpy_clamp_in_place(lib):
    """out aliasing p (tvam.h allows it), both entries."""
    n = N_ODD
    rng = np.random.default_rng(3)
    p, d = rng.random(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    dd, ad = dev(d), dev(np.array([0.3], np.float32))
    io = Guarded(n, init=p)
    _abi.check(lib.tvam_axpy_clamp(n, io.ptr, 0.3, dd.data_ptr(), 0.0, io.ptr, _stream()))
    vm.check_axpy(io.get("in place"), p, 0.3, d, 0.0, what="axpy_clamp in place")
    io = Guarded(n, init=p)
    _abi.check(lib.tvam_axpy_clamp_dev(n, io.ptr, ad.data_ptr(), dd.data_ptr(), 0.0, io.ptr, None, _stream()))
    vm.check_axpy(io.get("in place"), p, 0.3, d, 0.0, what="axpy_clamp_dev in place")


# ---------------------------------------------------------------------------
# chain: history -> coef -> direction_dev against the two-loop recursion
CHAIN_SLOTS = [3, 0, 5, 1, 7, 2, 6, 4]  # ring slots out of order, oldest pair first


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("H", [1, 4, 8])
def test_chain_against_two_loop(lib, H, first):
    n, h = N_ODD, H - 1
    g, S, Y, p, p_old, g_old = vm.chain_inputs(n, H)
    gd, Sd, Yd, pd, pod, god = dev(g), [dev(s) for s in S], [dev(y) for y in Y], dev(p), dev(p_old), dev(g_old)
    s_new, y_new = Guarded(n), Guarded(n)
    dots = Guarded(vm.hist_ndots(h, True), dtype=torch.float64)
    work = _work()
    _abi.check(lib.tvam_lbfgs_history(n, pd.data_ptr(), pod.data_ptr(), gd.data_ptr(), god.data_ptr(), h, ptrs(Sd),
                                      ptrs(Yd), s_new.ptr, y_new.ptr, work.data_ptr(), dots.ptr, _stream()))
    gram = np.zeros(128)
    for a in range(h):  # the retained pairs' entries by ring slot, as earlier steps stored them
        for b in range(h):
            gram[CHAIN_SLOTS[a] * 8 + CHAIN_SLOTS[b]] = S[a].astype(np.float64) @ Y[b].astype(np.float64)
            gram[64 + CHAIN_SLOTS[a] * 8 + CHAIN_SLOTS[b]] = Y[a].astype(np.float64) @ Y[b].astype(np.float64)
    gram_d = dev(gram)
    coef = Guarded(17, init=np.zeros(17, np.float32))
    gdz = Guarded(1, dtype=torch.float64)
    order = (ctypes.c_int32 * 8)(*CHAIN_SLOTS[:H])
    _abi.check(lib.tvam_lbfgs_coef(H, 1, first, order, dots.ptr, gram_d.data_ptr(), coef.ptr, gdz.ptr, _stream()))
    d = Guarded(n)
    _abi.check(lib.tvam_lbfgs_direction_dev(n, gd.data_ptr(), H, ptrs(Sd + [s_new.view]), ptrs(Yd + [y_new.view]),
                                            coef.ptr, d.ptr, _stream()))
    sn, yn = s_new.get("s_new"), y_new.get("y_new")
    vm.assert_bits_equal(sn, p - p_old, "s_new")
    vm.assert_bits_equal(yn, g - g_old, "y_new")
    c = coef.get("coef")
    assert np.all(c[1 + H:9] == 0) and np.all(c[9 + H:] == 0), "coefficients past h written"
    vm.check_chain(d.get("d"), gdz.get("gdz")[0], g, S + [sn], Y + [yn], first, what=f"chain H = {H}, first = {first}")


def test_coef_without_history(lib):
    """H = 0: d = -g, g.d = -g.g."""
    n = N_ODD
    g = vm.hist_inputs(n, 0, seed=50)[0]
    gd, work, gram = dev(g), _work(), dev(np.zeros(128))
    dots = Guarded(1, dtype=torch.float64)
    _abi.check(lib.tvam_lbfgs_history(n, None, None, gd.data_ptr(), None, 0, None, None, None, None, work.data_ptr(),
                                      dots.ptr, _stream()))
    vm.check_history(dots.get("dots"), g, [], [])
    coef, gdz, d = Guarded(17, init=np.zeros(17, np.float32)), Guarded(1, dtype=torch.float64), Guarded(n)
    for first in (0, 1):
        _abi.check(lib.tvam_lbfgs_coef(0, 0, first, None, dots.ptr, gram.data_ptr(), coef.ptr, gdz.ptr, _stream()))
        _abi.check(lib.tvam_lbfgs_direction_dev(n, gd.data_ptr(), 0, None, None, coef.ptr, d.ptr, _stream()))
        assert coef.get("coef")[0] == -1.0
        vm.check_chain(d.get("d"), gdz.get("gdz")[0], g, [], [], first, what="chain H = 0")


# ---------------------------------------------------------------------------
# loss
def call_loss(lib, K, params, n, dose, target=None, mask=None, bit0=0, ddose=None, alpha=0.0, grad=None):
    """tvam_loss_threshold or its _mask form (pointers); returns the value."""
    tl, tu, wo, wv, wl, sc = params
    out = Guarded(1, dtype=torch.float64, init=np.zeros(1))
    if mask is not None:
        rc = lib.tvam_loss_threshold_mask(dose, ddose, alpha, mask, bit0, n, K, tl, tu, wo, wv, wl, sc, out.ptr, grad,
                                          _stream())
    else:
        rc = lib.tvam_loss_threshold(dose, ddose, alpha, target, n, K, tl, tu, wo, wv, wl, sc, out.ptr, grad, _stream())
    _abi.check(rc)
    return out.get("loss value")[0]


def call_probes(lib, K, params, n, dose, ddose, alphas, target=None, mask=None, bit0=0):
    tl, tu, wo, wv, wl, sc = params
    na = len(alphas)
    out = Guarded(na, dtype=torch.float64, init=np.zeros(na))
    a = (ctypes.c_float * na)(*alphas)
    if mask is not None:
        rc = lib.tvam_loss_threshold_probes_mask(dose, ddose, a, na, mask, bit0, n, K, tl, tu, wo, wv, wl, sc, out.ptr,
                                                 _stream())
    else:
        rc = lib.tvam_loss_threshold_probes(dose, ddose, a, na, target, n, K, tl, tu, wo, wv, wl, sc, out.ptr, _stream())
    _abi.check(rc)
    return out.get("probe values")


def mask_dev(target):
    """The model's mask of target on the device (int32 words)."""
    return dev(vm.mask_model(target).view(np.int32))


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 16])
def test_loss_value_and_gradient(lib, K):
    """Value only and value + gradient, f32 target and mask form, both reductions' scale."""
    for n in SMALL + [WRAP]:
        x, target = vm.loss_inputs(n, 60 + n % 7, TL, TU)
        obj = target > 0
        xd, td, md = dev(x), dev(target), mask_dev(target)
        for scale in (1.0, 1.0 / n):
            params = _params(scale)
            model = vm.loss_level_a(x, obj, K, *params)
            for form in ("f32", "mask"):
                kw = dict(target=td.data_ptr()) if form == "f32" else dict(mask=md.data_ptr())
                what = f"loss {form} n = {n}, scale = {scale:g}"
                v = call_loss(lib, K, params, n, xd.data_ptr(), **kw)
                vm.check_loss(v, x, obj, K, params, what=what, model=model)
                grad = Guarded(n)
                v = call_loss(lib, K, params, n, xd.data_ptr(), grad=grad.ptr, **kw)
                vm.check_loss(v, x, obj, K, params, grad=grad.get(what + " gradient"), what=what, model=model)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 16])
def test_loss_with_ddose_and_probes(lib, K):
    """x = fmaf(alpha, ddose, dose): the single-alpha value and the probes with 1, 3 and 8 step sizes."""
    for n in SMALL + [WRAP]:
        x0, dx, target = vm.probe_inputs(n, 70 + n % 7, ALPHAS + [0.3125], TL, TU)
        obj = target > 0
        xd, dxd, td, md = dev(x0), dev(dx), dev(target), mask_dev(target)
        params = _params(1.0 / n)
        models = {a: vm.loss_level_a(vm.fma32(a, dx, x0), obj, K, *params, want_grad=False) for a in ALPHAS + [0.3125]}
        for form in ("f32", "mask"):
            kw = dict(target=td.data_ptr()) if form == "f32" else dict(mask=md.data_ptr())
            what = f"{form} n = {n}"
            v = call_loss(lib, K, params, n, xd.data_ptr(), ddose=dxd.data_ptr(), alpha=0.3125, **kw)
            vm.check_loss(v, None, obj, K, params, what="loss with ddose " + what, model=models[0.3125])
            for na in (1, 3, 8):
                vals = call_probes(lib, K, params, n, xd.data_ptr(), dxd.data_ptr(), ALPHAS[:na], **kw)
                for a, v in zip(ALPHAS[:na], vals):
                    vm.check_loss(v, None, obj, K, params, what=f"probe alpha = {a} of {na}, {what}", model=models[a])


@pytest.mark.parametrize("which", ["dose", "ddose", "grad", "target"])
def test_loss_one_pointer_off_the_16_byte_grid(lib, which):
    """Each of dose, ddose, grad, target alone one float off selects the scalar path: the same results,
    also past one sweep of that path."""
    K = 2
    for n in (N_ODD, LOSS_SCALAR_SWEEP + 4 * 300 + 3):
        x0, dx, target = vm.probe_inputs(n, 80, [0.5, 0.25, 1.0], TL, TU)
        obj = target > 0
        params = _params(1.0 / n)
        off = lambda name: 1 if name == which else 0
        xd, dxd, td = Guarded(n, off("dose"), init=x0), Guarded(n, off("ddose"), init=dx), Guarded(n, off("target"), init=target)
        assert sum(t.ptr % 16 != 0 for t in (xd, dxd, td)) == (which != "grad")
        grad = Guarded(n, off("grad"))
        model = vm.loss_level_a(vm.fma32(0.5, dx, x0), obj, K, *params)
        v = call_loss(lib, K, params, n, xd.ptr, target=td.ptr, ddose=dxd.ptr, alpha=0.5, grad=grad.ptr)
        vm.check_loss(v, None, obj, K, params, grad=grad.get("gradient"), what=f"{which} off, n = {n}", model=model)
        if which != "grad":
            vals = call_probes(lib, K, params, n, xd.ptr, dxd.ptr, [0.5, 0.25, 1.0], target=td.ptr)
            for a, v in zip([0.5, 0.25, 1.0], vals):
                vm.check_loss(v, vm.fma32(a, dx, x0), obj, K, params, what=f"probe {a}, {which} off, n = {n}")
        for t in (xd, dxd, td):
            t.get("input")  # inputs untouched around their ends too


@pytest.mark.parametrize("bit0", [0, 4, 28, 32, 36, 1, 31, 33])
def test_loss_mask_offsets(lib, bit0):
    """A slab of the film at mask bit offsets on the float4 path (multiples of 4) and the scalar path,
    ending inside a word."""
    K = 3
    n = N_ODD - (4 if (bit0 + N_ODD) % 32 == 0 else 0)
    assert (bit0 + n) % 32 != 0 and n % 4 == 3
    x0, dx, target = vm.probe_inputs(n, 90 + bit0, [0.5, 0.25, 1.0], TL, TU)
    film = np.concatenate([np.ones(bit0, np.float32), target, np.ones(50, np.float32)])  # neighbours all object
    md = mask_dev(film)
    obj = target > 0
    assert np.array_equal(vm.mask_bits(vm.mask_model(film), bit0, n), obj)
    params = _params(1.0 / n)
    xd, dxd = dev(x0), dev(dx)
    grad = Guarded(n)
    v = call_loss(lib, K, params, n, xd.data_ptr(), mask=md.data_ptr(), bit0=bit0, grad=grad.ptr)
    vm.check_loss(v, x0, obj, K, params, grad=grad.get("gradient"), what=f"mask offset {bit0}")
    v = call_loss(lib, K, params, n, xd.data_ptr(), mask=md.data_ptr(), bit0=bit0, ddose=dxd.data_ptr(), alpha=0.25)
    vm.check_loss(v, vm.fma32(0.25, dx, x0), obj, K, params, what=f"mask offset {bit0} with ddose")
    vals = call_probes(lib, K, params, n, xd.data_ptr(), dxd.data_ptr(), [0.5, 0.25, 1.0], mask=md.data_ptr(), bit0=bit0)
    for a, v in zip([0.5, 0.25, 1.0], vals):
        vm.check_loss(v, vm.fma32(a, dx, x0), obj, K, params, what=f"mask offset {bit0}, probe {a}")


EDGE_TARGETS = np.array([0.0, -0.0, -1.0, 1e-45, -1e-45, 1.0, 0.3], dtype=np.float32)


def edge_inputs(K):
    """Every edge dose against every edge target: x at tl, tu, 1 and 0, below 0; the thresholds'
    nextafter neighbours on both sides where the model admits them (K <= 5: the K-th power of one
    spacing, 2^-24 or 2^-23, is a normal number; at K = 16 it underflows and the model refuses, see
    test_vec_model.test_loss_model_refuses_subnormal_intermediates)."""
    xs = [0.0, -0.5, -2.0 ** -10]
    for t in vm.loss_thresholds(TL, TU):
        xs.append(t)
        if K <= 5:
            xs += [np.nextafter(t, np.float32(-9)), np.nextafter(t, np.float32(9))]
    xs = np.array(xs, dtype=np.float32)
    x = np.repeat(xs, EDGE_TARGETS.size)
    target = np.tile(EDGE_TARGETS, xs.size)
    return np.append(x, np.float32(0.5)), np.append(target, np.float32(1.0))  # + 1: a scalar tail


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 16])
def test_loss_edge_inputs(lib, K):
    x, target = edge_inputs(K)
    n = x.size
    assert n % 4 == (1 if K <= 5 else 3)
    obj = target > 0
    assert obj.sum() == (n - 1) // 7 * 3 + 1  # 1e-45, 1, 0.3 are object; 0, -0, -1, -1e-45 are not
    xd, td = dev(x), dev(target)
    words = Guarded((n + 31) // 32)
    _abi.check(lib.tvam_target_mask(td.data_ptr(), n, words.ptr, _stream()))
    vm.check_target_mask(words.get("mask").view(np.uint32), target)
    for scale in (1.0, 1.0 / n):
        params = _params(scale)
        for kw in (dict(target=td.data_ptr()), dict(mask=words.ptr)):
            grad = Guarded(n)
            v = call_loss(lib, K, params, n, xd.data_ptr(), grad=grad.ptr, **kw)
            gr = grad.get("gradient")
            vm.check_loss(v, x, obj, K, params, grad=gr, what=f"edge inputs, {'mask' if 'mask' in kw else 'f32'}")
            # the kink convention: no gradient at the thresholds themselves
            assert np.all(gr[obj & (x == np.float32(TU))] == 0) and np.all(gr[~obj & (x == np.float32(TL))] == 0)
            assert np.all(gr[obj & (x == 1)] == 0)


# ---------------------------------------------------------------------------
# target mask
def _mask_target(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.random(n, dtype=np.float32) - np.float32(0.5)
    for k, v in enumerate(EDGE_TARGETS):
        t[k::29] = v
    return t


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64 * 1000 + 13, MASK_LARGE])
def test_target_mask(lib, n):
    t = _mask_target(n, n % 101)
    td = dev(t)
    words = Guarded((n + 31) // 32)  # f32 NaN sentinels around the int32 words
    _abi.check(lib.tvam_target_mask(td.data_ptr(), n, words.ptr, _stream()))
    vm.check_target_mask(words.get(f"mask n = {n}").view(np.uint32), t, f"target mask n = {n}")


# ---------------------------------------------------------------------------
# misaligned pointers: TVAM_ERR_INVALID, one pointer at a time
def test_lbfgs_entries_reject_misaligned_pointers(lib):
    n, h = 64, 2
    buf = torch.zeros(16, n + 4, device="cuda")
    al = [buf[k, :n].data_ptr() for k in range(16)]
    assert all(a % 16 == 0 for a in al)
    keep = (_work(), torch.zeros(64, dtype=torch.float64, device="cuda"), torch.zeros(17, device="cuda"))
    work, dots, coef = (t.data_ptr() for t in keep)
    st = _stream()
    INVALID = _abi.TVAM_ERR_INVALID

    vec = dict(p=al[0], p_old=al[1], g=al[2], g_old=al[3], s_new=al[4], y_new=al[5], d=al[6], out=al[7], s_out=al[8])
    S, Y = (al[9], al[10]), (al[11], al[12])

    def ptrs_raw(v):
        return (ctypes.c_void_p * 8)(*v)

    def run(fn, names, lists=True, **base):
        assert fn(ptrs_raw(S), ptrs_raw(Y), **base) == 0
        for name in names:
            kw = dict(base)
            kw[name] += 4
            assert fn(ptrs_raw(S), ptrs_raw(Y), **kw) == INVALID, f"{fn.__name__}: {name} misaligned was accepted"
        for j in range(h if lists else 0):
            for which in "SY":
                s = tuple(a + 4 if (which == "S" and k == j) else a for k, a in enumerate(S))
                y = tuple(a + 4 if (which == "Y" and k == j) else a for k, a in enumerate(Y))
                assert fn(ptrs_raw(s), ptrs_raw(y), **base) == INVALID, f"{fn.__name__}: {which}[{j}] misaligned was accepted"

    def history(Sp, Yp, p, p_old, g, g_old, s_new, y_new):
        return lib.tvam_lbfgs_history(n, p, p_old, g, g_old, h, Sp, Yp, s_new, y_new, work, dots, st)

    def history_spre(Sp, Yp, g, g_old, s_new, y_new):
        return lib.tvam_lbfgs_history(n, None, None, g, g_old, h, Sp, Yp, s_new, y_new, work, dots, st)

    def history_plain(Sp, Yp, g):
        return lib.tvam_lbfgs_history(n, None, None, g, None, h, Sp, Yp, None, None, work, dots, st)

    def history_rows(Sp, Yp, p, p_old, g, g_old, s_new, y_new):
        return lib.tvam_lbfgs_history_rows(2, 16, 32, 0, p, p_old, g, g_old, h, Sp, Yp, s_new, y_new, work, dots, st)

    def direction(Sp, Yp, g, d):
        c = (ctypes.c_float * 8)(*([0.5] * 8))
        return lib.tvam_lbfgs_direction(n, g, h, Sp, Yp, -1.0, c, c, d, st)

    def direction_dev(Sp, Yp, g, d):
        return lib.tvam_lbfgs_direction_dev(n, g, h, Sp, Yp, coef, d, st)

    def direction_rows(Sp, Yp, g, d):
        return lib.tvam_lbfgs_direction_rows(2, 16, 32, 0, g, h, Sp, Yp, coef, d, st)

    def axpy(Sp, Yp, p, d, out):
        return lib.tvam_axpy_clamp(n, p, 0.5, d, 0.0, out, st)

    def axpy_dev(Sp, Yp, p, d, out, s_out):
        return lib.tvam_axpy_clamp_dev(n, p, coef, d, 0.0, out, s_out, st)

    pick = lambda *names: {k: vec[k] for k in names}
    new = ("p", "p_old", "g", "g_old", "s_new", "y_new")
    run(history, new, **pick(*new))
    run(history_spre, ("g", "g_old", "s_new", "y_new"), **pick("g", "g_old", "s_new", "y_new"))
    run(history_plain, ("g",), **pick("g"))
    run(history_rows, new, **pick(*new))
    for fn in (direction, direction_dev, direction_rows):
        run(fn, ("g", "d"), **pick("g", "d"))
    run(axpy, ("p", "d", "out"), lists=False, **pick("p", "d", "out"))
    run(axpy_dev, ("p", "d", "out", "s_out"), lists=False, **pick("p", "d", "out", "s_out"))
    torch.cuda.synchronize()

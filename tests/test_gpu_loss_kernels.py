"""GPU: the fused L2 and surface-aware loss kernels (tvam_loss.hip: tvam_loss_square*,
tvam_loss_surface*) against level A of tests/loss_model.py, through the C entries.  The gradient is
held bit for bit, the value within vec_model.check_sum's n v sum|terms| of scale x sum(level A), each
probe to the value at its step size under the same bound.  Every output lies inside a larger buffer
with NaN sentinels on both sides, which must survive the call."""
import ctypes

import numpy as np
import pytest
import torch

import loss_model as lm
import vec_model as vm
from drtvam_amd import _abi

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 257, 3073, 65541]  # voxels
WRAP = 2048 * 256 * 4 + 4 * 300 + 3  # past one sweep of a one-channel float4 kernel, two of a two-channel one
G = vm.GUARD
TL, TU = 0.85, 0.95
WEIGHTS = (1.0, 1.3, 0.7)  # object, void, limit
ALPHAS = [1.0, 0.5, 0.25, 0.125, 2.0 ** -7, 3.0, 0.0, -0.5]  # <= 11 significant bits each
ALPHA1 = 0.3125
CASES = [("l2", 2)] + [("surface_threshold", K) for K in (1, 2, 3, 4, 5, 16)] + [("surface_l2", 2)]


def _params(scale):
    return (TL, TU) + WEIGHTS + (scale,)


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


def call_loss(lib, law, K, params, n_vox, dose, target, ddose=None, alpha=0.0, grad=None):
    """tvam_loss_square / tvam_loss_surface on device pointers; the value."""
    tl, tu, wo, wv, wl, sc = params
    out = Guarded(1, dtype=torch.float64, init=np.zeros(1))
    if law == "l2":
        rc = lib.tvam_loss_square(dose, ddose, alpha, target, n_vox, sc, out.ptr, grad, _stream())
    else:
        rc = lib.tvam_loss_surface(lm.KIND[law], dose, ddose, alpha, target, n_vox, K, tl, tu, wo, wv, wl, sc, out.ptr,
                                   grad, _stream())
    _abi.check(rc)
    return out.get("loss value")[0]


def call_probes(lib, law, K, params, n_vox, dose, ddose, alphas, target):
    tl, tu, wo, wv, wl, sc = params
    na = len(alphas)
    out = Guarded(na, dtype=torch.float64, init=np.zeros(na))
    a = (ctypes.c_float * na)(*alphas)
    if law == "l2":
        rc = lib.tvam_loss_square_probes(dose, ddose, a, na, target, n_vox, sc, out.ptr, _stream())
    else:
        rc = lib.tvam_loss_surface_probes(lm.KIND[law], dose, ddose, a, na, target, n_vox, K, tl, tu, wo, wv, wl, sc,
                                          out.ptr, _stream())
    _abi.check(rc)
    return out.get("probe values")


def run_case(lib, law, K, n, offs=(0, 0, 0, 0), seed=0, nas=(1, 8)):
    """Everything of one law at one size: value, value + gradient, both reductions, with and without a
    step, the probes.  offs: floats off the 16-byte grid of dose, ddose, target, grad."""
    c = lm.channels(law)
    what = f"{law} K = {K}, {n} voxels, offsets {offs}"
    x, target = lm.inputs(law, n, 100 + seed + n % 7, TL, TU)
    xd, td = Guarded(c * n, offs[0], init=x), Guarded(c * n, offs[2], init=target)
    for scale in (1.0, 1.0 / n):  # 'sum', 'mean'
        params = _params(scale)
        model = lm.level_a(law, x, target, K, *params)
        v = call_loss(lib, law, K, params, n, xd.ptr, td.ptr)
        lm.check_loss(law, v, x, target, K, params, what=what, model=model)
        grad = Guarded(c * n, offs[3])
        v = call_loss(lib, law, K, params, n, xd.ptr, td.ptr, grad=grad.ptr)
        lm.check_loss(law, v, x, target, K, params, grad=grad.get(what + " gradient"), what=what, model=model)
    for t in (xd, td):
        t.get(what + " input")  # inputs untouched around their ends
    # a step on the 2^-12 grid
    alphas = ALPHAS[:max(nas)] + [ALPHA1]
    x0, dx, target = lm.probe_inputs(law, n, 200 + seed + n % 7, alphas, TL, TU)
    xd, dxd, td = Guarded(c * n, offs[0], init=x0), Guarded(c * n, offs[1], init=dx), Guarded(c * n, offs[2], init=target)
    params = _params(1.0 / n)
    models = {a: lm.level_a(law, vm.fma32(a, dx, x0), target, K, *params) for a in alphas}
    grad = Guarded(c * n, offs[3])
    v = call_loss(lib, law, K, params, n, xd.ptr, td.ptr, ddose=dxd.ptr, alpha=ALPHA1, grad=grad.ptr)
    lm.check_loss(law, v, None, target, K, params, grad=grad.get(what + " gradient with a step"), what=what + " with a step",
                  model=models[ALPHA1])
    for na in nas:
        vals = call_probes(lib, law, K, params, n, xd.ptr, dxd.ptr, ALPHAS[:na], td.ptr)
        for a, pv in zip(ALPHAS[:na], vals):
            lm.check_loss(law, pv, None, target, K, params, what=f"{what}: probe {a} of {na}", model=(models[a][0], None))
            # the probe against the value call at that step size: two f64 accumulations of the same terms
            v = call_loss(lib, law, K, params, n, xd.ptr, td.ptr, ddose=dxd.ptr, alpha=a)
            terms = float(np.float32(params[-1])) * models[a][0].astype(np.float64)
            assert abs(pv - v) <= 2 * terms.size * vm.V * float(np.abs(terms).sum()), (what, a, pv, v)


@pytest.mark.parametrize("law,K", CASES)
def test_value_gradient_and_probes(lib, law, K):
    for n in SIZES:
        run_case(lib, law, K, n)


@pytest.mark.parametrize("which", ["dose", "ddose", "target", "grad"])
@pytest.mark.parametrize("law,K", [("l2", 2), ("surface_threshold", 2), ("surface_threshold", 5), ("surface_l2", 2)])
def test_one_pointer_off_the_16_byte_grid(lib, law, K, which):
    """Each pointer alone one float off (4-byte aligned) and, for two channels, one voxel off (8-byte
    aligned: a float4 there would split voxel pairs) selects the scalar path: the same results."""
    for off in (1, 2) if lm.channels(law) == 2 else (1,):
        offs = tuple(off if name == which else 0 for name in ("dose", "ddose", "target", "grad"))
        for n in (3, 257, 3073):
            run_case(lib, law, K, n, offs=offs, seed=3, nas=(8,))


def test_every_pointer_one_voxel_off(lib):
    """All four arrays 8-byte aligned, equally: still no float4 may be formed."""
    for law in ("surface_threshold", "surface_l2"):
        run_case(lib, law, 2, 3073, offs=(2, 2, 2, 2), seed=5, nas=(8,))


@pytest.mark.parametrize("law", lm.LAWS)
def test_past_one_grid_sweep(lib, law):
    """More float4s than one sweep of 2048 workgroups: the grid-stride trip and the tail after it."""
    n = WRAP // lm.channels(law)
    assert n % 2 == 1
    run_case(lib, law, 2, n, seed=9, nas=(3,))


def test_edge_doses_and_targets(lib):
    """Doses at the kinks and their neighbours against every kind of target; no gradient at a kink."""
    ks = [np.float32(v) for v in (TL, TU, 1.0)]
    xs = [np.float32(0.0), np.float32(-0.5)] + ks + [np.nextafter(k, np.float32(s)) for k in ks for s in (-9, 9)]
    # one channel: every dose against 0, -0, negative, positive targets and itself
    ts = np.float32([0.0, -0.0, -1.0, 1.0, 0.3])
    x = np.append(np.repeat(np.float32(xs), ts.size), np.float32(xs))
    t = np.append(np.tile(ts, len(xs)), np.float32(xs))
    params = _params(1.0 / x.size)
    grad = Guarded(x.size)
    xd, td = Guarded(x.size, init=x), Guarded(x.size, init=t)
    v = call_loss(lib, "l2", 2, params, x.size, xd.ptr, td.ptr, grad=grad.ptr)
    g = grad.get("l2 gradient")
    lm.check_loss("l2", v, x, t, 2, params, grad=g, what="l2 edges")
    assert np.all(g[x == t] == 0)
    # two channels: every (x0, x1) pair of edge doses against inside-only, outside-only and mixed voxels
    pairs = np.float32([(a, b) for a in xs for b in xs])
    tg = np.float32([(1.0, 0.0), (0.0, 1.0), (0.25, 0.75), (0.5, 0.0625)])
    x2 = np.repeat(pairs, len(tg), axis=0).reshape(-1)
    t2 = np.tile(tg, (len(pairs), 1)).reshape(-1)
    n = x2.size // 2
    xd, td = Guarded(2 * n, init=x2), Guarded(2 * n, init=t2)
    for law, K in (("surface_threshold", 1), ("surface_threshold", 2), ("surface_threshold", 5), ("surface_l2", 2)):
        params = _params(1.0 / n)
        grad = Guarded(2 * n)
        v = call_loss(lib, law, K, params, n, xd.ptr, td.ptr, grad=grad.ptr)
        g = grad.get(law + " gradient")
        lm.check_loss(law, v, x2, t2, K, params, grad=g, what=f"{law} K = {K} edges")
        g0, g1, x0, x1 = g[0::2], g[1::2], x2[0::2], x2[1::2]
        assert np.all(g0[t2[0::2] == 0] == 0) and np.all(g1[t2[1::2] == 0] == 0)  # a zero weight: no gradient
        if law == "surface_threshold":
            assert np.all(g0[(x0 == np.float32(TU)) | (x0 == 1)] == 0) and np.all(g1[x1 <= np.float32(TL)] == 0)
        else:
            assert np.all(g0[x0 == 1] == 0) and np.all(g1[x1 == 0] == 0)


def test_invalid_arguments_and_empty_input(lib):
    """TVAM_ERR_INVALID with the cause named; n = 0 launches nothing and leaves out untouched."""
    n = 8
    buf = Guarded(2 * n, init=np.full(2 * n, 0.5, np.float32))
    out = Guarded(8, dtype=torch.float64, init=np.full(8, 7.0))
    a = (ctypes.c_float * 8)(*ALPHAS)
    p, o, st = buf.ptr, out.ptr, _stream()
    w = _params(1.0)
    cases = [
        (lib.tvam_loss_square(None, None, 0.0, p, n, 1.0, o, None, st), "tvam_loss_square: null dose"),
        (lib.tvam_loss_square(p, None, 0.0, None, n, 1.0, o, None, st), "tvam_loss_square: null target"),
        (lib.tvam_loss_square(p, None, 0.0, p, n, 1.0, None, None, st), "tvam_loss_square: null out"),
        (lib.tvam_loss_square_probes(p, None, a, 1, p, n, 1.0, o, st), "tvam_loss_square_probes: null ddose"),
        (lib.tvam_loss_square_probes(p, p, a, 0, p, n, 1.0, o, st), "tvam_loss_square_probes: 1 <= n_alpha <= 8 (got 0)"),
        (lib.tvam_loss_square_probes(p, p, a, 9, p, n, 1.0, o, st), "tvam_loss_square_probes: 1 <= n_alpha <= 8 (got 9)"),
        (lib.tvam_loss_surface(0, None, None, 0.0, p, n, 2, *w, o, None, st), "tvam_loss_surface: null dose"),
        (lib.tvam_loss_surface(0, p, None, 0.0, None, n, 2, *w, o, None, st), "tvam_loss_surface: null target"),
        (lib.tvam_loss_surface(0, p, None, 0.0, p, n, 2, *w, None, None, st), "tvam_loss_surface: null out"),
        (lib.tvam_loss_surface(2, p, None, 0.0, p, n, 2, *w, o, None, st),
         "tvam_loss_surface: unknown kind 2 (0: threshold, 1: l2)"),
        (lib.tvam_loss_surface(0, p, None, 0.0, p, n, 0, *w, o, None, st),
         "tvam_loss_surface: integer K in [1, 16] required (got 0)"),
        (lib.tvam_loss_surface(0, p, None, 0.0, p, n, 17, *w, o, None, st),
         "tvam_loss_surface: integer K in [1, 16] required (got 17)"),
        (lib.tvam_loss_surface_probes(0, p, None, a, 1, p, n, 2, *w, o, st), "tvam_loss_surface_probes: null ddose"),
        (lib.tvam_loss_surface_probes(0, p, p, a, 9, p, n, 2, *w, o, st),
         "tvam_loss_surface_probes: 1 <= n_alpha <= 8 (got 9)"),
        (lib.tvam_loss_surface_probes(5, p, p, a, 1, p, n, 2, *w, o, st),
         "tvam_loss_surface_probes: unknown kind 5 (0: threshold, 1: l2)"),
        (lib.tvam_loss_surface_probes(0, p, p, a, 1, p, n, 17, *w, o, st),
         "tvam_loss_surface_probes: integer K in [1, 16] required (got 17)"),
    ]
    for rc, msg in cases:
        assert rc == _abi.TVAM_ERR_INVALID, (msg, rc)
    # the message of the last refusal (each call above overwrote the one before): checked call by call
    rc = lib.tvam_loss_surface(2, p, None, 0.0, p, n, 2, *w, o, None, st)
    assert lib.tvam_last_error().decode() == "tvam_loss_surface: unknown kind 2 (0: threshold, 1: l2)"
    rc = lib.tvam_loss_square_probes(p, None, a, 1, p, n, 1.0, o, st)
    assert rc == _abi.TVAM_ERR_INVALID and lib.tvam_last_error().decode() == "tvam_loss_square_probes: null ddose"
    assert lib.tvam_loss_square(p, None, 0.0, p, 0, 1.0, o, None, st) == 0
    assert lib.tvam_loss_square_probes(p, p, a, 8, p, 0, 1.0, o, st) == 0
    assert lib.tvam_loss_surface(0, p, None, 0.0, p, 0, 2, *w, o, None, st) == 0
    assert lib.tvam_loss_surface_probes(1, p, p, a, 8, p, 0, 2, *w, o, st) == 0
    torch.cuda.synchronize()
    assert np.all(out.get("out after refused and empty calls") == 7.0)
    buf.get("input")


def test_engine_wrappers_check_their_tensors():
    from drtvam_amd import engine
    x = torch.full((2, 3, 4, 2), 0.5, device="cuda")
    t = torch.full((2, 3, 4, 2), 0.5, device="cuda")
    v = float(engine.loss_surface(_abi.LOSS_KIND_L2, x.reshape(-1), t.reshape(-1), 1.0))
    assert v == 24 * (0.5 * 0.25 + 0.5 * 0.25)
    assert float(engine.loss_square(x.reshape(-1), t.reshape(-1), 1.0 / 48)) == 0.0
    with pytest.raises(ValueError, match="size mismatch"):
        engine.loss_square(x.reshape(-1), t.reshape(-1)[:8], 1.0)
    with pytest.raises(ValueError, match="contiguous float32"):
        engine.loss_square(x.reshape(-1), t.reshape(-1).double(), 1.0)
    with pytest.raises(ValueError, match="contiguous float32"):
        engine.loss_surface(0, x.reshape(-1), t.reshape(-1)[::2], 1.0)
    with pytest.raises(ValueError, match="even number"):
        engine.loss_surface(0, x.reshape(-1)[:7], t.reshape(-1)[:7], 1.0)
    with pytest.raises(ValueError, match="1 to 8 step sizes"):
        engine.loss_square_probes(x.reshape(-1), x.reshape(-1), [1.0] * 9, t.reshape(-1), 1.0)
    with pytest.raises(ValueError, match="1 to 8 step sizes"):
        engine.loss_surface_probes(0, x.reshape(-1), x.reshape(-1), [], t.reshape(-1), 1.0)
    with pytest.raises(ValueError, match="contiguous float32"):
        engine.loss_square(x.reshape(-1), t.reshape(-1).cpu(), 1.0)

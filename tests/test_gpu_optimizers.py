"""GPU: the first-order optimisers.  The update kernels (tvam_vec.hip: tvam_sgd_step,
tvam_adam_step, tvam_adam_moments + tvam_adam_apply) through the C entries against the fp32 model of
tests/optim_model.py, bit for bit, every vector inside a NaN-sentinel buffer; drtvam_amd.optimizers on
CUDA tensors against the same steps on CPU tensors; and the config's 'optimizer' entry through the
real loop (TvamProblem, optimize(), two ranks).  No TVAM_VEC_* knob is set: the second grid-stride
trip is reached by size."""
import copy
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optim_model as om
from drtvam_amd import SGD, Adam, _abi
from test_gpu_vec_kernels import Guarded, _stream

pytestmark = pytest.mark.gpu

# launch geometry (tvam_vec.hip, TVAM_OPT_GRID): 2048 blocks of 256 threads, one float4 per thread and
# trip; the moments pass writes one partial per block, summed by one block of tvam_partials_kernel
OPT_SWEEP = 2048 * 256 * 4
N_ODD = 4 * 1031 + 3
SMALL = [1, 3, 4, 7, N_ODD]
WRAP = OPT_SWEEP + 4 * 300 + 3  # past one sweep, with a float4 remainder and a tail
assert WRAP % 4 == 3
LR = 0.01
KEY = "projector.active_data"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def layouts():
    """(n, offsets of p / g / the state vectors in floats off the 16-byte grid): every small size at
    every shared offset, the second sweep at two, and vectors that do not share an offset (the
    scalar path whole)."""
    out = [(n, (o, o, o)) for n in SMALL for o in range(4)]
    out += [(WRAP, (0, 0, 0)), (WRAP, (3, 3, 3)), (N_ODD, (0, 1, 2)), (7, (2, 0, 0))]
    return out


# ---------------------------------------------------------------------------
# kernels
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_step(lib, momentum, mask):
    for n, (op, og, os_) in layouts():
        p, g, _, _, s = om.optim_inputs(n, seed=n, lo=0.0)
        P, Gd = Guarded(n, op, init=p), Guarded(n, og, init=g)
        S = Guarded(n, os_, init=s) if momentum else None
        what = f"sgd n = {n}, offsets {op}{og}{os_}, momentum {momentum}, mask {mask}"
        _abi.check(lib.tvam_sgd_step(n, P.ptr, Gd.ptr, S.ptr if S else None, LR, momentum, int(mask), 0.0, _stream()))
        om.check_sgd(P.get(what + ": p"), S.get(what + ": s") if S else None, p, g, s if momentum else None, LR, momentum,
                     mask, 0.0, what=what)
        om.assert_bits_equal(Gd.get(what + ": g"), g, what + ": g untouched")


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_step(lib, t, mask):
    lr_t = float(om.adam_scalars(LR, 0.9, 0.999, 1e-8, t)[0])
    for n, (op, og, os_) in layouts():
        p, g, m, v, _ = om.optim_inputs(n, seed=n + t, lo=0.0)
        P, Gd, M, Vd = Guarded(n, op, init=p), Guarded(n, og, init=g), Guarded(n, os_, init=m), Guarded(n, os_, init=v)
        what = f"adam n = {n}, offsets {op}{og}{os_}, t = {t}, mask {mask}"
        _abi.check(lib.tvam_adam_step(n, P.ptr, Gd.ptr, M.ptr, Vd.ptr, lr_t, 0.9, 0.999, 1e-8, int(mask), 0.0, _stream()))
        om.check_adam(P.get(what + ": p"), M.get(what + ": m"), Vd.get(what + ": v"), t, p, g, m, v, t - 1, LR,
                      mask=mask, lo=0.0, what=what)
        om.assert_bits_equal(Gd.get(what + ": g"), g, what + ": g untouched")


def test_adam_step_other_hyperparameters(lib):
    """beta, epsilon and the clamp as arguments: rounded inside (c = fl32(1 - beta) from the double)."""
    n, t, kw = N_ODD, 3, dict(beta_1=0.8, beta_2=0.99, epsilon=1e-6)
    lr_t = float(om.adam_scalars(0.3, t=t, **kw)[0])
    for lo in (0.25, -math.inf):
        p, g, m, v, _ = om.optim_inputs(n, seed=9, lo=0.25)
        P, Gd, M, Vd = (Guarded(n, init=a) for a in (p, g, m, v))
        _abi.check(lib.tvam_adam_step(n, P.ptr, Gd.ptr, M.ptr, Vd.ptr, lr_t, 0.8, 0.99, 1e-6, 1, lo, _stream()))
        om.check_adam(P.get("p"), M.get("m"), Vd.get("v"), t, p, g, m, v, t - 1, 0.3, mask=True, lo=lo, **kw)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("t", [1, 1000])
def test_adam_uniform_pair(lib, t, mask):
    lr_t = float(om.adam_scalars(LR, 0.9, 0.999, 1e-8, t)[0])
    work = torch.empty(_abi.LBFGS_WORK_DOUBLES, dtype=torch.float64, device="cuda")
    for n, (op, og, os_) in layouts():
        p, g, m, v, _ = om.optim_inputs(n, seed=n + 2 * t, lo=0.0)
        N = 3 * n + 5  # the entries of all ranks
        what = f"adam uniform n = {n}, offsets {op}{og}{os_}, t = {t}, mask {mask}"
        sums = []
        for _ in range(2):  # the same call twice: bit-identical S
            Gd, M, Vd = Guarded(n, og, init=g), Guarded(n, os_, init=m), Guarded(n, os_, init=v)
            S = Guarded(1, dtype=torch.float64)
            _abi.check(lib.tvam_adam_moments(n, Gd.ptr, M.ptr, Vd.ptr, 0.9, 0.999, int(mask), work.data_ptr(), S.ptr,
                                             _stream()))
            sums.append(S.get(what + ": S"))
        assert sums[0].view(np.uint64) == sums[1].view(np.uint64), what + ": S differs between two identical calls"
        P = Guarded(n, op, init=p)
        sn = torch.tensor([sums[0][0], float(N)], dtype=torch.float64, device="cuda")
        _abi.check(lib.tvam_adam_apply(n, P.ptr, Gd.ptr if mask else None, M.ptr, sn.data_ptr(), sn.data_ptr() + 8, lr_t,
                                       1e-8, int(mask), 0.0, _stream()))
        m1, v1 = M.get(what + ": m"), Vd.get(what + ": v")
        om.check_adam(P.get(what + ": p"), m1, v1, t, p, g, m, v, t - 1, LR, mask=mask, lo=0.0, uniform=True,
                      S=sums[0][0], N=N, what=what)
        om.check_uniform_sum(sums[0][0], v1, what + ": S")


def test_no_launch_cases(lib):
    n = 8
    p, g, m, v, s = om.optim_inputs(n, seed=1)
    bufs = [Guarded(n, init=a) for a in (p, g, m, v, s)]
    P, Gd, M, Vd, S = bufs
    work = torch.empty(_abi.LBFGS_WORK_DOUBLES, dtype=torch.float64, device="cuda")
    sn = torch.tensor([1.0, 8.0], dtype=torch.float64, device="cuda")
    st = _stream()
    zero = [lib.tvam_sgd_step(0, P.ptr, Gd.ptr, S.ptr, LR, 0.9, 0, 0.0, st),
            lib.tvam_adam_step(0, P.ptr, Gd.ptr, M.ptr, Vd.ptr, LR, 0.9, 0.999, 1e-8, 0, 0.0, st),
            lib.tvam_adam_moments(0, Gd.ptr, M.ptr, Vd.ptr, 0.9, 0.999, 0, work.data_ptr(), sn.data_ptr(), st),
            lib.tvam_adam_apply(0, P.ptr, None, M.ptr, sn.data_ptr(), sn.data_ptr() + 8, LR, 1e-8, 0, 0.0, st)]
    assert zero == [0, 0, 0, 0]
    null = [lambda: lib.tvam_sgd_step(n, None, Gd.ptr, S.ptr, LR, 0.9, 0, 0.0, st),
            lambda: lib.tvam_sgd_step(n, P.ptr, None, S.ptr, LR, 0.9, 0, 0.0, st),
            lambda: lib.tvam_sgd_step(n, P.ptr, Gd.ptr, None, LR, 0.9, 0, 0.0, st),  # momentum without s
            lambda: lib.tvam_adam_step(n, P.ptr, Gd.ptr, None, Vd.ptr, LR, 0.9, 0.999, 1e-8, 0, 0.0, st),
            lambda: lib.tvam_adam_step(n, P.ptr, Gd.ptr, M.ptr, None, LR, 0.9, 0.999, 1e-8, 0, 0.0, st),
            lambda: lib.tvam_adam_moments(n, Gd.ptr, M.ptr, Vd.ptr, 0.9, 0.999, 0, None, sn.data_ptr(), st),
            lambda: lib.tvam_adam_moments(n, Gd.ptr, M.ptr, Vd.ptr, 0.9, 0.999, 0, work.data_ptr(), None, st),
            lambda: lib.tvam_adam_apply(n, P.ptr, None, M.ptr, sn.data_ptr(), sn.data_ptr() + 8, LR, 1e-8, 1, 0.0, st),
            lambda: lib.tvam_adam_apply(n, P.ptr, None, M.ptr, None, sn.data_ptr() + 8, LR, 1e-8, 0, 0.0, st)]
    for i, call in enumerate(null):
        rc = call()
        assert rc == _abi.TVAM_ERR_INVALID, (i, rc)
        assert b"tvam_" in lib.tvam_last_error(), i
        with pytest.raises(ValueError):
            _abi.check(rc)
    torch.cuda.synchronize()
    for b, a in zip(bufs, (p, g, m, v, s)):
        om.assert_bits_equal(b.get("no launch"), a, "a refused or empty call changed a vector")
    assert sn.tolist() == [1.0, 8.0]


# ---------------------------------------------------------------------------
# the classes on CUDA tensors
@pytest.mark.parametrize("make", [
    lambda: Adam(lr=LR, lo=0.0), lambda: Adam(lr=LR, mask_updates=True, beta_1=0.8),
    lambda: SGD(lr=0.05, momentum=0.9, lo=0.0), lambda: SGD(lr=0.05, mask_updates=True),
])
def test_step_on_cuda_equals_cpu(make):
    n = N_ODD
    p = om.optim_inputs(n, seed=0, lo=0.0)[0]
    opts = {d: make() for d in ("cpu", "cuda")}
    for d, o in opts.items():
        o[KEY] = torch.from_numpy(p).to(d)
    for k in range(3):
        g = om.optim_inputs(n, seed=20 + k)[1]
        for d, o in opts.items():
            o[KEY].grad = torch.from_numpy(g).to(d)
            o.step()
        om.assert_bits_equal(opts["cuda"][KEY].detach().cpu().numpy(), opts["cpu"][KEY].detach().numpy(), f"step {k}: p'")
        for a, b in zip(opts["cuda"].state[KEY], opts["cpu"].state[KEY]):
            om.assert_bits_equal(a.cpu().numpy(), b.numpy(), f"step {k}: state")
        assert opts["cuda"].t[KEY] == opts["cpu"].t[KEY] == k + 1


def test_uniform_step_on_cuda(lib):
    """Adam(uniform=True).step() on CUDA: the model's step for the S the moments pass summed."""
    n = N_ODD
    p, g, _, _, _ = om.optim_inputs(n, seed=4, lo=0.0)
    opt = Adam(lr=LR, uniform=True, lo=0.0, count=2 * n)
    opt[KEY] = torch.from_numpy(p).cuda()
    z = np.zeros(n, np.float32)
    opt[KEY].grad = torch.from_numpy(g).cuda()
    opt.step()
    S = float(opt._sn[KEY][0])
    m1, v1 = (s.cpu().numpy() for s in opt.state[KEY])
    om.check_adam(opt[KEY].detach().cpu().numpy(), m1, v1, opt.t[KEY], p, g, z, z, 0, LR, lo=0.0, uniform=True, S=S,
                  N=2 * n)
    om.check_uniform_sum(S, v1)


# ---------------------------------------------------------------------------
# the loop
def snap(opt):
    return [s.cpu().numpy().copy() for s in opt.state[KEY]]


def record_steps(opt, log):
    inner = opt.step

    def step():
        x = opt[KEY]
        before = (x.detach().cpu().numpy().copy(), x.grad.cpu().numpy().copy(), snap(opt), opt.t[KEY])
        inner()
        log.append(before + (opt[KEY].detach().cpu().numpy().copy(), snap(opt), opt.t[KEY]))
    opt.step = step


def model_step(opt, p, g, state, t, S=None):
    if isinstance(opt, Adam):
        p1, m1, v1, t1 = om.adam_step32(p, g, state[0], state[1], t, opt.lr, opt.beta_1, opt.beta_2, opt.epsilon,
                                        opt.mask_updates, opt.lo, opt.uniform, S=S, N=opt.count)
        return p1, [m1, v1], t1
    p1, s1 = om.sgd_step32(p, g, state[0] if state else None, opt.lr, opt.momentum, opt.mask_updates, opt.lo)
    return p1, ([s1] if state else []), t + 1


def small_problem(optimizer=None, sparsity=0.0, x0=None):
    from drtvam_amd.configs import benchy_index_matched
    from drtvam_amd.optimize import TvamProblem
    cfg = benchy_index_matched(N=32, angles=16)
    if sparsity:
        cfg["loss"]["weight_sparsity"] = sparsity
    if optimizer is not None:
        cfg["optimizer"] = optimizer
    prob = TvamProblem(cfg, device=torch.device("cuda", 0))
    if x0 == "random":
        prob.x0 = prob.local_from_global(torch.rand(prob.n_global, generator=torch.Generator().manual_seed(0)) * 0.1)
    elif x0 == "zero":
        prob.x0 = torch.zeros_like(prob.x0)
    return prob


@pytest.mark.parametrize("optimizer", [{"type": "adam", "lr": 0.01}, {"type": "sgd", "lr": 0.01, "momentum": 0.9}])
def test_step_replay_through_the_loop(optimizer):
    """4 iterations of TvamProblem with the config's optimiser: every update is the model's one step
    of the x, x.grad (adjoint + sparsity gradient) and state captured before it, clamped at 0; t
    advances by one per iteration; one forward per iteration.  Fails where the entry is ignored."""
    prob = small_problem(optimizer, sparsity=0.01, x0="random")
    assert prob.fused
    opt = prob.make_optimizer()
    assert isinstance(opt, Adam if optimizer["type"] == "adam" else SGD) and opt.lo == 0.0
    log, forwards = [], []
    record_steps(opt, log)
    inner = prob.forward_local
    prob.forward_local = lambda x, seed: (forwards.append(seed), inner(x, seed))[1]
    for i in range(4):
        prob.iteration(i)
    assert forwards == [0, 1, 2, 3] and len(log) == 4 and len(prob.loss_hist) == 4
    for k, (p, g, state, t, p1, state1, t1) in enumerate(log):
        assert t == k and t1 == k + 1
        assert np.any(g > 0) and np.any(g < 0)  # the sparsity gradient is in: the adjoint alone is <= 0 here
        wp, ws, _ = model_step(opt, p, g, state, t)
        om.assert_bits_equal(p1, wp, f"iteration {k}: x")
        for a, b in zip(state1, ws):
            om.assert_bits_equal(a, b, f"iteration {k}: state")
        assert p1.min() >= 0.0
        if k:
            om.assert_bits_equal(p, log[k - 1][4], f"iteration {k}: x is the previous update's output")


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_first_step_lowers_the_loss(kind):
    """Patterns zero, regular sampling: the dose is 0, only the object term is active and the
    gradient is <= 0.  Adam's first step raises every pixel with a gradient to lr (within the
    first-step bound) and leaves the others at 0, so with lr = tl / max(forward(ones)) every dose is
    <= tl (1 + bound): the void and limit terms stay 0 (up to (tl bound)^2) and the object term falls
    wherever a ray passes.  SGD's first step is -lr g0: lr = tl / max(forward(-g0)) gives the same."""
    prob = small_problem(x0="zero")
    x0 = prob.x0
    tl = prob.loss_fn.tl
    if kind == "adam":
        lr = tl / float(prob.forward(torch.ones_like(x0), 0).max())
    else:
        _, gvol = prob.loss_value_grad(prob.forward(x0, 0), x0)
        g0 = prob.adjoint(gvol, 0)
        lr = tl / float(prob.forward((-g0).contiguous(), 0).max())
    prob.optimizer_cfg = {"type": kind, "lr": lr}
    opt = prob.make_optimizer()
    log = []
    record_steps(opt, log)
    prob.iteration(0)
    prob.iteration(1)
    p, g, _, _, p1, _, _ = log[0]
    assert not p.any() and np.all(g <= 0) and np.any(g < 0)
    assert prob.loss_hist[1] < prob.loss_hist[0]
    nz = g != 0
    assert not p1[~nz].any()
    if kind == "adam":
        err = np.abs(p1.astype(np.float64) - lr)
        assert np.all(err[nz] <= om.first_step_bound(g, lr)[nz])
    else:
        om.assert_bits_equal(p1, om.sgd_step32(p, g, None, lr, lo=0.0)[0], "sgd first step")
    # both doses are fp32 sums of non-negative terms, fewer than 800 per voxel (16 angles, a few rays
    # each): each within 800 u < 5e-5 of its exact value, and the exact ones obey the inequality
    dose = prob.forward(torch.from_numpy(p1).cuda(), 0)
    assert float(dose.max()) <= tl * (1 + 1e-4)


def test_optimize_end_to_end(tmp_path):
    """optimize() with 'optimizer' adam writes its outputs; the loss history differs from the run
    without the entry (the L-BFGS).  Fails where the entry is ignored."""
    from drtvam_amd.configs import BOX_HOLE_INDEX_MATCHED
    from drtvam_amd.optimize import optimize
    hist = {}
    for name, entry in (("adam", {"type": "adam", "lr": 0.01}), ("default", None)):
        cfg = copy.deepcopy(BOX_HOLE_INDEX_MATCHED)
        cfg["target"]["filename"] = os.path.join(GOLDEN, "box_hole.ply")
        cfg["n_steps"] = 6
        cfg["output"] = str(tmp_path / name)
        if entry:
            cfg["optimizer"] = entry
        optimize(cfg, device=torch.device("cuda", 0))
        hist[name] = np.load(tmp_path / name / "loss.npy")
    out = tmp_path / "adam"
    pats = np.load(out / "patterns.npz")["patterns"]
    assert (out / "final.npy").exists() and pats.shape == (200, 20, 200)
    assert np.all(np.isfinite(pats)) and pats.min() >= 0.0 and pats.max() > 0.0
    assert hist["adam"].shape == hist["default"].shape == (6,)
    assert np.isclose(hist["adam"][0], hist["default"][0], rtol=1e-4)  # the same first forward
    assert not np.allclose(hist["adam"][1:], hist["default"][1:], rtol=1e-3)


# ---------------------------------------------------------------------------
# two ranks
STEPS2 = 3


def _run2(rank, world, shard):
    from drtvam_amd.configs import benchy_index_matched
    from drtvam_amd.optimize import TvamProblem
    cfg = benchy_index_matched(N=24, angles=12)
    cfg["shard"] = shard
    cfg["optimizer"] = {"type": "adam", "lr": 0.01, "uniform": True}
    prob = TvamProblem(cfg, device=torch.device("cuda", 0), rank=rank, world_size=world)
    assert prob.shard == shard
    prob.x0 = prob.local_from_global(torch.rand(prob.n_global, generator=torch.Generator().manual_seed(0)) * 0.1)
    opt = prob.make_optimizer()
    assert opt.uniform and opt.count == prob.n_global and (opt.allreduce is not None) == (world > 1)
    log, sums = [], []
    record_steps(opt, log)
    for i in range(STEPS2):
        prob.iteration(i)
        sums.append(float(opt._sn[KEY][0]))
    # every step of this rank: the model's, for the all-reduced S and the global count
    for k, (p, g, state, t, p1, state1, t1) in enumerate(log):
        wp, ws, wt = model_step(opt, p, g, state, t, S=sums[k])
        om.assert_bits_equal(p1, wp, f"rank {rank}, step {k}: x")
        for a, b in zip(state1, ws):
            om.assert_bits_equal(a, b, f"rank {rank}, step {k}: state")
        assert t1 == wt == k + 1
    v = prob.gather_patterns(opt.state[KEY][1])  # the last v' of every rank
    om.check_uniform_sum(sums[-1], v.cpu().numpy())
    x = prob.gather_patterns(prob.patterns_local().float())
    return np.asarray(prob.loss_hist), x.cpu().numpy(), np.asarray(sums)


def _worker2(rank, world, port, shard, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = _run2(rank, world, shard)
        if rank == 0:
            q.put(res)
    except BaseException:  # report instead of leaving the parent waiting
        import traceback
        q.put(("error", rank, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("shard", ["angle", "slab"])
def test_two_rank_adam_uniform_matches_single_rank(shard):
    """Angle shards and z-slabs, Adam uniform: each rank's every step is the model's step bit for
    bit for the all-reduced S (one f64 scalar, the only new collective) and the global count, S is
    the sum of every rank's v', and the patterns agree with the one-rank run.  Between the two runs
    the fp32 partial doses (angle shards) or the slab losses are summed in another order, which is
    outside the optimiser's model; that comparison carries the tolerance
    tests/test_gpu_distributed.py sets for the same quantity."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()

    def result(procs):
        try:
            res = q.get(timeout=240)
        finally:
            for p in procs:
                p.join(timeout=60)
                if p.is_alive():
                    p.kill()
        assert not (isinstance(res[0], str) and res[0] == "error"), res[2]
        assert all(p.exitcode == 0 for p in procs)
        return res

    p1 = ctx.Process(target=_worker2, args=(0, 1, _free_port(), shard, q))
    p1.start()
    ref_loss, ref_x, ref_S = result([p1])
    port = _free_port()
    procs = [ctx.Process(target=_worker2, args=(r, 2, port, shard, q)) for r in range(2)]
    for p in procs:
        p.start()
    loss, x, S = result(procs)
    assert ref_loss[-1] < ref_loss[0]
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    np.testing.assert_allclose(S, ref_S, rtol=1e-4)
    np.testing.assert_allclose(x, ref_x, rtol=1e-3, atol=1e-5)

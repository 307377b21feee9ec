"""CPU: drtvam_amd.optimizers.SGD / Adam (the torch path) against the fp32 model of
tests/optim_model.py, their constructor checks, and their wiring into ShardedLoop (the config's
'optimizer' entry) on the dense CPU operator of tests/test_distributed.py, one rank and two (gloo)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optim_model as om
from drtvam_amd import SGD, Adam
from drtvam_amd.lbfgs import LinearLBFGS
from test_distributed import A, PER_ANGLE, MatrixShard, free_port

KEY = "projector.active_data"
N = 4 * 257 + 3


# ---------------------------------------------------------------------------
# the torch path, bit for bit
def model_state(opt):
    return [s.numpy().copy() for s in opt.state[KEY]]


def model_step(opt, p, g, state, t):
    """One step of the fp32 model with opt's settings.  Returns (p', state', t')."""
    if isinstance(opt, Adam):
        p1, m1, v1, t1 = om.adam_step32(p, g, state[0], state[1], t, opt.lr, opt.beta_1, opt.beta_2, opt.epsilon,
                                        opt.mask_updates, opt.lo, opt.uniform, N=opt.count)
        return p1, [m1, v1], t1
    p1, s1 = om.sgd_step32(p, g, state[0] if state else None, opt.lr, opt.momentum, opt.mask_updates, opt.lo)
    return p1, ([s1] if state else []), t + 1


OPTS = [
    lambda: SGD(lr=0.05),
    lambda: SGD(lr=0.05, momentum=0.9, mask_updates=True, lo=0.0),
    lambda: Adam(lr=0.01),
    lambda: Adam(lr=0.01, beta_1=0.8, beta_2=0.99, epsilon=1e-6, mask_updates=True, lo=0.0),
    lambda: Adam(lr=0.01, uniform=True, lo=0.0),
    lambda: Adam(lr=0.01, uniform=True, mask_updates=True),
]


@pytest.mark.parametrize("make", OPTS)
def test_torch_path_equals_model_over_steps(make):
    """5 steps; after the second the variable is re-assigned at the same size (state and t kept, as
    the reference loop's clamp re-assigns), after the fourth at another size (state and t zeroed)."""
    opt = make()
    p, _, _, _, _ = om.optim_inputs(N, seed=0, lo=0.0)
    opt[KEY] = torch.from_numpy(p)
    state, t = [np.zeros(N, np.float32) for _ in range(opt.n_state)], 0
    for k in range(5):
        n = p.size
        g = om.optim_inputs(n, seed=10 + k)[1]
        x = opt[KEY]
        x.grad = torch.from_numpy(g)
        opt.step()
        p, state, t = model_step(opt, p, g, state, t)
        om.assert_bits_equal(opt[KEY].detach().numpy(), p, f"step {k}: p'")
        for a, b in zip(model_state(opt), state):
            om.assert_bits_equal(a, b, f"step {k}: state")
        assert opt.t[KEY] == t
        if k == 1:
            p = np.maximum(p, np.float32(0.25))
            opt[KEY] = torch.from_numpy(p)
            assert opt.t[KEY] == t == 2
        if k == 3:
            p = p[:-1].copy()
            opt[KEY] = torch.from_numpy(p)
            state, t = [np.zeros(p.size, np.float32) for _ in range(opt.n_state)], 0
            assert opt.t[KEY] == 0 and all(not s.any() for s in opt.state[KEY])
    opt.reset(KEY)
    assert opt.t[KEY] == 0 and all(not s.any() for s in opt.state[KEY])


def test_access_and_learning_rate():
    opt = Adam(lr=0.01)
    opt[KEY] = torch.ones(5)
    assert list(opt.keys()) == [KEY] and [k for k, _ in opt.items()] == [KEY]
    assert opt[KEY].requires_grad and opt[KEY].dtype == torch.float32
    opt.set_learning_rate(0.5)
    assert opt.lr == 0.5
    opt.step()  # no gradient yet: nothing moves
    assert opt.t[KEY] == 0 and torch.equal(opt[KEY].detach(), torch.ones(5))


@pytest.mark.parametrize("cls,kw", [
    (SGD, dict(lr=-1.0)), (SGD, dict(lr=0.1, momentum=1.0)), (SGD, dict(lr=0.1, momentum=-0.1)),
    (Adam, dict(lr=-0.1)), (Adam, dict(lr=0.1, beta_1=1.0)), (Adam, dict(lr=0.1, beta_2=-0.5)),
    (Adam, dict(lr=0.1, epsilon=0.0)), (Adam, dict(lr=float("nan"))),
])
def test_constructor_validation(cls, kw):
    with pytest.raises(ValueError):
        cls(**kw)


def test_constructor_keywords():
    with pytest.raises(TypeError):
        Adam(lr=0.1, beta1=0.9)
    with pytest.raises(TypeError):
        SGD(lr=0.1, nesterov=True)
    with pytest.raises(TypeError):
        Adam()  # lr is required
    with pytest.raises(TypeError):
        SGD()
    with pytest.raises(NotImplementedError):
        Adam(lr=0.1, params={KEY: torch.zeros(3)})
    with pytest.raises(NotImplementedError):
        SGD(lr=0.1, params={KEY: torch.zeros(3)})
    a = Adam(lr=0.1)
    assert (a.beta_1, a.beta_2, a.epsilon, a.mask_updates, a.uniform, a.lo) == (0.9, 0.999, 1e-8, False, False, -math.inf)
    s = SGD(lr=0.1)
    assert (s.momentum, s.mask_updates, s.lo) == (0.0, False, -math.inf)


# ---------------------------------------------------------------------------
# the loop
CONFIGS = {
    "adam": {"type": "adam", "lr": 0.02},
    "adam_uniform": {"type": "adam", "lr": 0.02, "uniform": True},
    "sgd_momentum": {"type": "sgd", "lr": 0.5, "momentum": 0.9},
}
STEPS = 4


class OptShard(MatrixShard):
    """MatrixShard with fp32 patterns (the operator stays float64) and an 'optimizer' entry."""

    def __init__(self, rank, world, cfg):
        super().__init__(rank, world)
        self.optimizer_cfg = cfg
        self.x0 = self.x0.to(torch.float32)

    def forward_local(self, x, seed):
        return super().forward_local(x.detach().to(torch.float64), seed)

    def adjoint_local(self, grad_vol, seed):
        return super().adjoint_local(grad_vol, seed).to(torch.float32)


def run(rank, world, cfg, log=None):
    prob = OptShard(rank, world, cfg)
    opt = prob.make_optimizer()
    if log is not None:
        inner = opt.step

        def step():
            x = opt[KEY]
            log.append((x.detach().numpy().copy(), x.grad.to(torch.float32).numpy().copy(), model_state(opt), opt.t[KEY]))
            inner()
            log[-1] += (opt[KEY].detach().numpy().copy(), model_state(opt), opt.t[KEY])
        opt.step = step
    for i in range(STEPS):
        prob.iteration(i)
    x = prob.patterns_local()
    if world > 1:
        parts = [torch.empty_like(x) for _ in range(world)]
        dist.all_gather(parts, x)
        x = torch.cat(parts)
    return prob, np.asarray(prob.loss_hist), x.numpy()


def _worker(rank, world, port, name, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _, loss, x = run(rank, world, CONFIGS[name])
        if rank == 0:
            q.put((loss, x))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_loop_builds_the_configured_optimizer(name):
    """One rank: every step of the loop is the model's step of the recorded x, x.grad and state
    (the clamp at 0 fused, uniform's count the global entry count), t advances by one per
    iteration; two ranks (gloo, angle shards) reproduce the patterns within the model's bound:
    the sum over the steps of the one-step bound level A / level B at the one-rank run's inputs
    (the ranks' float64 dose sums differ in their last bits, which reaches an fp32 gradient entry
    only where it sits at a rounding boundary)."""
    log = []
    prob, ref_loss, ref_x = run(0, 1, CONFIGS[name], log)
    opt = prob.opt
    assert isinstance(opt, Adam if name.startswith("adam") else SGD) and opt.lo == 0.0
    assert len(log) == STEPS and ref_loss[-1] < ref_loss[0]
    tol = np.zeros(ref_x.size)
    for k, (p, g, state, t, p1, state1, t1) in enumerate(log):
        assert t == k and t1 == k + 1
        wp, ws, wt = model_step(opt, p, g, state, t)
        om.assert_bits_equal(p1, wp, f"step {k}: p'")
        for a, b in zip(state1, ws):
            om.assert_bits_equal(a, b, f"step {k}: state")
        assert p1.min() >= 0.0
        if isinstance(opt, Adam):
            tol += om.adam_bound(p, g, state[0], state[1], t, opt.lr, uniform=opt.uniform)[0]
        else:
            tol += om.sgd_bound(p, g, state[0], opt.lr, opt.momentum)[0]
    if name == "adam_uniform":
        assert opt.count == A * PER_ANGLE

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, name, q)) for r in range(2)]
    for p in procs:
        p.start()
    loss, x = q.get()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-6)
    om.check_within_bound(x, ref_x.astype(np.float64), tol, f"{name}: two ranks against one")


def test_cli_overrides_reach_the_optimizer_entry():
    """-D optimizer.type=adam -D optimizer.lr=0.01 on a config without the entry."""
    import argparse
    from drtvam_amd.optimize import OverrideAction, apply_overrides
    ap = argparse.ArgumentParser()
    ap.add_argument("-D", dest="overrides", action=OverrideAction)
    ns = ap.parse_args(["-D", "optimizer.type=adam", "-D", "optimizer.lr=0.01", "-D", "n_steps=3"])
    cfg = apply_overrides({"loss": {"type": "threshold"}}, ns.overrides)
    assert cfg == {"loss": {"type": "threshold"}, "optimizer": {"type": "adam", "lr": 0.01}, "n_steps": 3}
    prob = OptShard(0, 1, cfg["optimizer"])
    assert isinstance(prob.make_optimizer(), Adam) and prob.opt.lr == 0.01


def test_loop_without_optimizer_entry_builds_lbfgs():
    for cfg in (None, {"type": "lbfgs"}, {"type": "lbfgs", "m": 7}, {"type": "something"}):
        prob = OptShard(0, 1, cfg)
        prob.make_optimizer()
        assert isinstance(prob.opt, LinearLBFGS) and not isinstance(prob.opt, (Adam, SGD))
    prob = MatrixShard(0, 1)  # a loop that never heard of the entry
    prob.iteration(0)
    assert isinstance(prob.opt, LinearLBFGS)

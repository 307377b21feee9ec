"""First-order optimisers: Mitsuba 3's ``mi.ad.SGD`` and ``mi.ad.Adam`` for one learning rate
(the reference's ``"optimizer": {"type": "adam" | "sgd", ...}``, optimize.py:203-225).

Per element every operation is one once-rounded fp32 operation, in this order, no fma;
keep = mask_updates and g == 0; lo is the clamp fused into the update (-inf: none):

  SGD    momentum 0:  w = p - lr32 g
         else:        s' = mu s + g;  w = p - lr32 s';  keep: s' = s
  Adam   t += 1;  lr_t = fl32(fl32(lr) fl32(sqrt(1 - beta_2^t) / (1 - beta_1^t)))
         m' = b1 m + c1 g;  v' = b2 v + c2 (g g);  keep: m' = m, v' = v
         den = sqrt(v') + e   (uniform: fl32(sqrt(S / N)) + e, S = the fp64 sum of v' over all
                               entries of all ranks, N their number)
         w = p - (lr_t m') / den
  both   keep: w = p;  p' = w < lo ? lo : w

with lr32 = fl32(lr), mu = fl32(momentum), b = fl32(beta), c = fl32(1 - beta) (the subtraction in
double), e = fl32(epsilon).  On contiguous fp32 CUDA tensors ``step()`` is one fused HIP pass
(tvam_sgd_step / tvam_adam_step; tvam_adam_moments + tvam_adam_apply for uniform) on the current
stream, in place; on any other tensor the same formulas run as torch fp32 operations in the same
order.  tests/optim_model.py is the numpy model both are pinned to, bit for bit.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def _f32(x):
    return float(np.float32(x))


def adam_scalars(lr, beta_1, beta_2, epsilon, t):
    """(lr_t, b1, c1, b2, c2, e) of step t, each an fp32 value held in a Python float."""
    scale = math.sqrt(1 - beta_2 ** t) / (1 - beta_1 ** t)
    lr_t = float(np.float32(lr) * np.float32(scale))
    return lr_t, _f32(beta_1), _f32(1.0 - beta_1), _f32(beta_2), _f32(1.0 - beta_2), _f32(epsilon)


class _FirstOrder:
    def __init__(self, lr, mask_updates, params, lo):
        if params is not None:
            raise NotImplementedError("per-parameter settings (params) are not offered: assign with opt[key] = x")
        self.set_learning_rate(lr)
        self.mask_updates = bool(mask_updates)
        self.lo = float(lo)
        self.variables = {}
        self.state = {}
        self.t = {}

    # mi.ad.Optimizer-style access
    def __setitem__(self, key, value):
        v = value.detach().clone() if isinstance(value, torch.Tensor) else torch.as_tensor(value)
        old = self.variables.get(key)
        v.requires_grad_(True)
        self.variables[key] = v
        if old is None or old.numel() != v.numel() or old.device != v.device:
            self.reset(key)

    def __getitem__(self, key):
        return self.variables[key]

    def keys(self):
        return self.variables.keys()

    def items(self):
        return self.variables.items()

    def set_learning_rate(self, lr):
        if isinstance(lr, dict):
            raise NotImplementedError("per-parameter learning rates are not offered")
        if not float(lr) >= 0:
            raise ValueError("'lr' must be >= 0")
        self.lr = float(lr)

    def reset(self, key):
        """Zero the state of `key` (and its step count)."""
        x = self.variables[key]
        self.state[key] = [torch.zeros(x.numel(), dtype=torch.float32, device=x.device) for _ in range(self.n_state)]
        self.t[key] = 0

    @staticmethod
    def _fusable(x, g):
        return (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and g.is_cuda and g.dtype == torch.float32
                and g.numel() == x.numel())

    @torch.no_grad()
    def step(self):
        for key, x in self.variables.items():
            if x.grad is None:
                continue
            g = x.grad.detach()
            if self._fusable(x, g):
                self._step_fused(key, x, g.contiguous().reshape(-1))
            else:
                p = x.detach().reshape(-1).to(torch.float32)
                w = self._step_torch(key, p, g.reshape(-1).to(torch.float32))
                lo = torch.tensor(self.lo, dtype=torch.float32, device=w.device)
                x.copy_(torch.where(w < lo, lo, w).reshape(x.shape))

    def _keep(self, g):
        return (g == 0) if self.mask_updates else None


def _scalar(v, like):
    return torch.tensor(v, dtype=torch.float32, device=like.device)


class SGD(_FirstOrder):
    """mi.ad.SGD: gradient descent, with momentum when ``momentum != 0``."""

    def __init__(self, lr, momentum=0.0, mask_updates=False, params=None, lo=-math.inf):
        if not 0 <= momentum < 1:
            raise ValueError("'momentum' must be in [0, 1)")
        self.momentum = float(momentum)
        self.n_state = 1 if self.momentum != 0 else 0
        super().__init__(lr, mask_updates, params, lo)

    def _step_torch(self, key, p, g):
        lr = _scalar(_f32(self.lr), p)
        keep = self._keep(g)
        if self.momentum == 0:
            w = p - lr * g
        else:
            s = self.state[key][0]
            s1 = _scalar(_f32(self.momentum), p) * s + g
            w = p - lr * s1
            s.copy_(s1 if keep is None else torch.where(keep, s, s1))
        self.t[key] += 1
        return w if keep is None else torch.where(keep, p, w)

    def _step_fused(self, key, x, g):
        from . import _abi
        lib = _abi.load_library()
        s = self.state[key][0].data_ptr() if self.momentum != 0 else None
        _abi.check(lib.tvam_sgd_step(x.numel(), x.data_ptr(), g.data_ptr(), s, self.lr, self.momentum,
                                     int(self.mask_updates), self.lo, torch.cuda.current_stream(x.device).cuda_stream))
        self.t[key] += 1


class Adam(_FirstOrder):
    """mi.ad.Adam.  ``uniform``: one denominator sqrt(mean v) for every entry; under sharding
    ``allreduce`` (in place, e.g. ShardedLoop.allreduce_) sums the one f64 scalar over the ranks
    and ``count`` is the number of entries of all ranks."""

    n_state = 2

    def __init__(self, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask_updates=False, uniform=False, params=None,
                 lo=-math.inf, allreduce=None, count=None):
        if not 0 <= beta_1 < 1:
            raise ValueError("'beta_1' must be in [0, 1)")
        if not 0 <= beta_2 < 1:
            raise ValueError("'beta_2' must be in [0, 1)")
        if not epsilon > 0:
            raise ValueError("'epsilon' must be > 0")
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.uniform = bool(uniform)
        self.allreduce = allreduce
        self.count = count
        self._sn = {}    # uniform, fused: device f64 [S, N]
        self._work = {}
        super().__init__(lr, mask_updates, params, lo)

    def _step_torch(self, key, p, g):
        self.t[key] += 1
        lr_t, b1, c1, b2, c2, e = (_scalar(v, p) for v in adam_scalars(self.lr, self.beta_1, self.beta_2,
                                                                          self.epsilon, self.t[key]))
        m, v = self.state[key]
        keep = self._keep(g)
        m1 = b1 * m + c1 * g
        v1 = b2 * v + c2 * (g * g)
        if keep is not None:
            m1, v1 = torch.where(keep, m, m1), torch.where(keep, v, v1)
        m.copy_(m1)
        v.copy_(v1)
        if self.uniform:
            S = v1.sum(dtype=torch.float64).reshape(1)
            if self.allreduce is not None:
                S = self.allreduce(S)
            N = float(self.count if self.count is not None else p.numel())
            den = _scalar(_f32(math.sqrt(float(S) / N)), p) + e
        else:
            # the correctly rounded fp32 root: torch's own fp32 sqrt is not on every backend, and the
            # f64 root of an fp32 number rounds to it (53 >= 2 x 24 + 2 bits)
            den = torch.sqrt(v1.to(torch.float64)).to(torch.float32) + e
        w = p - (lr_t * m1) / den
        return w if keep is None else torch.where(keep, p, w)

    def _step_fused(self, key, x, g):
        from . import _abi
        lib = _abi.load_library()
        self.t[key] += 1
        lr_t = adam_scalars(self.lr, self.beta_1, self.beta_2, self.epsilon, self.t[key])[0]
        m, v = self.state[key]
        st = torch.cuda.current_stream(x.device).cuda_stream
        n, mask = x.numel(), int(self.mask_updates)
        if not self.uniform:
            _abi.check(lib.tvam_adam_step(n, x.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr_t, self.beta_1,
                                          self.beta_2, self.epsilon, mask, self.lo, st))
            return
        sn = self._sn.get(key)
        if sn is None or sn.device != x.device:
            N = float(self.count if self.count is not None else n)
            sn = self._sn[key] = torch.tensor([0.0, N], dtype=torch.float64, device=x.device)
            self._work[key] = torch.empty(_abi.LBFGS_WORK_DOUBLES, dtype=torch.float64, device=x.device)
        if n == 0:  # an empty shard: no launch, its term of the all-reduce is 0
            sn[0:1].zero_()
        _abi.check(lib.tvam_adam_moments(n, g.data_ptr(), m.data_ptr(), v.data_ptr(), self.beta_1, self.beta_2, mask,
                                         self._work[key].data_ptr(), sn.data_ptr(), st))
        if self.allreduce is not None:
            self.allreduce(sn[0:1])
        _abi.check(lib.tvam_adam_apply(n, x.data_ptr(), g.data_ptr(), m.data_ptr(), sn.data_ptr(), sn.data_ptr() + 8,
                                       lr_t, self.epsilon, mask, self.lo, st))

"""GPU: the fused L2 and surface-aware losses in the optimisation loop (drtvam_amd/optimize.py,
drtvam_amd/loss.py): which problems are fused, loss_value_grad / loss_step / loss_steps of a fused
problem against the model of tests/loss_model.py and the float64 torch mirror, z-slab shards under
the L2 loss, and a short optimisation against the torch path ('fused_loss': false).

Scenes: the index-matched 24^3 x 10 angles of tests/test_gpu_radon.py and a 20^3 x 10 surface-aware
film around the box-with-hole mesh (the scene of tests/test_gpu_surface.py's make).  The thresholds
are dyadic (0.875, 0.9375), so that the kernels' fp32 parameters are the float64 mirror's."""
import copy
import os

import numpy as np
import pytest
import torch

import loss_model as lm
import vec_model as vm
from drtvam_amd.configs import benchy_index_matched
from drtvam_amd.lbfgs import FusedLinearLBFGS
from drtvam_amd.optimize import TvamProblem, optimize

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
TL, TU = 0.875, 0.9375
ALPHAS = [1.0, 0.5, 0.25, 0.125]

# largest relative deviation of the fused run's loss history from the torch path's over the 6 steps of
# test_l2_optimization_matches_the_torch_path, measured on an MI355X (the test prints it)
HISTORY_DEVIATION = 7.3e-8
HISTORY_TOLERANCE = min(1e-3, 10 * HISTORY_DEVIATION)


def planar_config(loss, **extra):
    cfg = benchy_index_matched(N=24, angles=10, size_mm=5.0, r=2.9, n_steps=6)
    cfg["loss"] = loss
    return cfg | extra


def surface_config(loss, **extra):
    cfg = benchy_index_matched(N=20, angles=10, size_mm=4.0, r=2.9, n_steps=6)
    cfg["target"] = {"filename": os.path.join(GOLDEN, "box_hole.ply"), "size": 3.0}
    cfg["final_sensor"] = copy.deepcopy(cfg["sensor"])
    cfg["sensor"]["film"]["surface_aware"] = True
    cfg["loss"] = loss
    return cfg | extra


THRESHOLD = {"type": "threshold", "tl": TL, "tu": TU, "K": 2}
CONFIGS = {
    "l2": lambda **k: planar_config({"type": "l2"}, **k),
    "surface_threshold": lambda **k: surface_config(dict(THRESHOLD, reduction="mean"), **k),
    "surface_l2": lambda **k: surface_config({"type": "l2", "reduction": "mean"}, **k),
}


@pytest.fixture(scope="module")
def problems():
    """law -> (fused problem, torch-path problem), built once; the surface-aware target (compute_volume) is
    computed by the first problem and handed to the others."""
    out, vols = {}, None
    for law, make in CONFIGS.items():
        fused = TvamProblem(make(), device=DEV, target=vols if law != "l2" else None)
        if law != "l2":
            vols = fused.target_full
        out[law] = (fused, TvamProblem(make(fused_loss=False), device=DEV, target=fused.target_full))
    return out


def test_which_problems_are_fused(problems):
    for law, (fused, plain) in problems.items():
        assert fused.fused is True, law
        assert plain.fused is False, law
        assert fused.target.shape[-1] == lm.channels(law)
        opt = fused.make_optimizer()
        assert isinstance(opt, FusedLinearLBFGS) and opt.loss_steps is not None, law
        assert plain.make_optimizer().loss_steps is None
    assert TvamProblem(planar_config(THRESHOLD), device=DEV).fused is True
    assert TvamProblem(planar_config(dict(THRESHOLD, K=2.5)), device=DEV).fused is False
    with pytest.raises(ValueError, match="z-slab sharding needs regular sampling, a non-scattering medium and the fused "
                                         "thresholded loss"):
        TvamProblem(planar_config(dict(THRESHOLD, K=2.5), shard="slab"), device=DEV)
    with pytest.raises(ValueError, match="z-slab sharding needs"):
        TvamProblem(planar_config({"type": "l2"}, shard="slab", fused_loss=False), device=DEV)


def _mirror(prob, x):
    """The loss of the float64 torch definition on the fp32 dose x (flat numpy)."""
    xt = torch.from_numpy(x.astype(np.float64)).reshape(tuple(prob.target.shape))
    return float(prob.loss_fn(xt, prob.target.double().cpu(), torch.zeros(1, dtype=torch.float64)))


@pytest.mark.parametrize("law", lm.LAWS)
def test_fused_loss_against_the_model_and_the_torch_path(problems, law):
    fused, plain = problems[law]
    lf = fused.loss_fn
    shape = tuple(fused.proj.film_shape)
    n_vox = fused.n_vox
    assert int(np.prod(shape)) == n_vox * lm.channels(law) and shape == tuple(fused.target.shape)
    K = 2
    weights = (TL, TU, 1.0, 1.0, 1.0)
    reduction = lf.reduction_name
    assert reduction == ("sum" if law == "l2" else "mean")
    target = fused.target.cpu().numpy().reshape(-1)
    if law != "l2":
        assert np.all(target[0::2] + target[1::2] > 0) and np.any(target[0::2] == 0) and np.any(target[1::2] == 0)
    x0, dx, _ = lm.probe_inputs(law, n_vox, 5, ALPHAS, TL, TU)
    vol, dvol = (torch.from_numpy(a).reshape(shape).to(DEV) for a in (x0, dx))
    pats = fused.x0
    # one more rounding than the element's for 'mean': the kernels' scale is fl32(1 / voxels)
    bound = lm.value_bound_rel(law, K) + (vm.U if reduction == "mean" else 0.0)
    # value and gradient
    v, g = fused.loss_value_grad(vol, pats)
    want = _mirror(fused, x0)
    print(f"{law}: fused value {float(v)!r}, float64 mirror {want!r}, relative {abs(float(v) - want) / want:.3e}, bound {bound:.3e}")
    assert abs(float(v) - want) <= bound * want
    lm.check_reduced(law, float(v), x0, target, K, weights, reduction, n_vox, grad=g.cpu().numpy().reshape(-1),
                     what=f"{law} loss_value_grad")
    # the torch path on the same dose: an fp32 sum of n elements, each rounding at most u of a partial sum
    vp, gp = plain.loss_value_grad(vol, pats)
    print(f"{law}: torch-path value {float(vp)!r}, relative {abs(float(vp) - want) / want:.3e}")
    assert abs(float(vp) - want) <= (n_vox * vm.U + bound) * want
    assert gp.shape == g.shape
    # the probes: each against the mirror at the dose the fma gives, and against loss_step
    vals = fused.loss_steps(vol, dvol, ALPHAS, pats).cpu().numpy()
    for a, pv in zip(ALPHAS, vals):
        xa = vm.fma32(a, dx, x0)
        want = _mirror(fused, xa)
        assert abs(pv - want) <= bound * want, (law, a, pv, want)
        lm.check_reduced(law, pv, xa, target, K, weights, reduction, n_vox, what=f"{law} loss_steps at {a}")
        sv = float(fused.loss_step(vol, dvol, a, pats))
        lm.check_reduced(law, sv, xa, target, K, weights, reduction, n_vox, what=f"{law} loss_step at {a}")
        # the torch path forms vol + a dvol in two fp32 operations: exact for these power-of-two steps on the
        # 2^-12 grid, so it evaluates the same dose
        tv = float(plain.loss_step(vol, dvol, a, pats))
        assert abs(tv - want) <= (n_vox * vm.U + bound) * want, (law, a, tv, want)


def test_l2_slab_shards():
    """shard 'slab' under the L2 loss on two emulated ranks: the slab terms sum to the one-rank value and
    the slab gradients are the one-rank gradient's slices, bit for bit ('mean': every slab scales by
    the whole film's voxel count)."""
    cfg = planar_config({"type": "l2", "reduction": "mean"}, shard="slab")
    one = TvamProblem(cfg, device=DEV, rank=0, world_size=1)
    two = [TvamProblem(cfg, device=DEV, rank=r, world_size=2) for r in range(2)]
    auto = TvamProblem(planar_config({"type": "l2"}), device=DEV, rank=1, world_size=2)
    assert auto.shard == "slab" and auto.dose_sharded and auto.fused
    assert TvamProblem(planar_config({"type": "l2"}, fused_loss=False), device=DEV, rank=1, world_size=2).shard == "angle"
    assert all(p.shard == "slab" and p.fused for p in [one] + two)
    assert (two[0].z0, two[0].z1, two[1].z1) == (0, two[1].z0, one.res_z) and 0 < two[1].z0 < one.res_z
    x = torch.rand(one.n_global, generator=torch.Generator().manual_seed(1)) * 0.1
    vol = one.forward(one.local_from_global(x), 0)
    assert float(vol.max()) > 0
    v1, g1 = one.loss_value_grad(vol, one.x0, reduce=False)
    v1, g1 = float(v1), g1.clone()
    parts = []
    for p in two:
        slab = vol[p.z0:p.z1]
        assert tuple(slab.shape) == tuple(p.proj.film_shape) and slab.is_contiguous()
        v, g = p.loss_value_grad(slab, p.x0, reduce=False)
        parts.append(float(v))
        vm.assert_bits_equal(g.cpu().numpy(), g1[p.z0:p.z1].cpu().numpy(), f"slab gradient of rank {p.rank}")
    # two f64 accumulations of the same non-negative terms, each within n v sum|terms| (vec_model.check_sum)
    assert v1 > 0 and abs(sum(parts) - v1) <= 2 * one.n_vox * vm.V * v1, (parts, v1)


def test_l2_optimization_matches_the_torch_path(tmp_path):
    hist = {}
    for arm, fused in (("fused", True), ("torch", False)):
        out = tmp_path / arm
        optimize(planar_config({"type": "l2"}, regular_sampling=True, fused_loss=fused, output=str(out)), device=DEV)
        hist[arm] = np.load(out / "loss.npy")
    a, b = hist["fused"], hist["torch"]
    assert a.shape == b.shape == (6,)
    dev = float(np.max(np.abs(a - b) / np.abs(b)))
    print(f"l2 loss history: fused {a.tolist()}, torch {b.tolist()}, largest relative deviation {dev:.3e}")
    assert a[-1] < a[0] and b[-1] < b[0] and np.all(np.isfinite(a))
    assert dev <= HISTORY_TOLERANCE, dev

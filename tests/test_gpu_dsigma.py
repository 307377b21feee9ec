"""Extinction derivatives on the GPU (tvam_dsigma.hip): the tangent film T = d dose / d sigma_t
(Projection.forward_dsigma) and the reverse-mode scalar g = <G, T> (Projection.adjoint_dsigma)
against the central difference of the float64 oracle at sigma +- h (dsigma_model.fd_tangent, accepted
only once it has converged), on every kind of plan the entries serve.

Collimated plans of tvam_plan_create (any vial, occluders): the oracle's own forward at sigma +- h.
3-D ray plans (telecentric / lens, traced glass, 'custom'): oracle.dda_ray at sigma +- h over the
segments exported by Projection.rays (the pattern of test_gpu_traced_vial.reference), one Python loop
per variant, cached.

Patterns are U[0, 0.1); a second set is lit at one angle only, so that a per-ray error is not averaged
over the angles.  Bars: the project's forward bars for the film (relative L2 < 1e-4 and per voxel
|dT| <= 1e-4 max |T_ref|), |g - <G, T_ref>| <= 1e-4 <|G|, |T_ref|> for the scalar, and the dot-test bar
1e-6 sum |G T_gpu| between the two GPU results."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.engine import Projection, render

import double_vial_model as dv
import dsigma_model as dm
import mesh_vial_model as mv
import projector_model as pm
import test_gpu_square as sq
import traced_vial_model as tv

DEV = "cuda:0"
SEED = 3


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def no_planar(d):
    d = d.copy()
    d.flags |= _abi.FLAG_NO_PLANAR
    return d


# name -> (descriptor, True: the oracle restates the projector and the vial (oracle.forward))
CASES = {
    "collimated": (lambda: pm.projector_scene("collimated"), True),
    "collimated-regular": (lambda: pm.projector_scene("collimated", regular=True), True),
    "collimated-noplanar": (lambda: no_planar(pm.projector_scene("collimated", regular=True)), True),
    "telecentric": (lambda: pm.projector_scene("telecentric"), False),
    "lens": (lambda: pm.projector_scene("lens"), False),
    "square": (lambda: sq.make(), True),
    "square-occ": (lambda: sq.make(occ=True), True),
    "square-occ-jittered": (lambda: sq.make(occ=True, regular=False, spp=2), True),
    "index_matched-occ": (lambda: sq.make(vial="index_matched", occ=True), True),
    "cylindrical-occ": (lambda: sq.make(vial="cylindrical", occ=True), True),
    "traced-cylindrical-telecentric": (lambda: tv.traced_scene("cylindrical", "telecentric"), False),
    "traced-square-lens-regular": (lambda: tv.traced_scene("square", "lens", regular=True), False),
    "custom-lens-cuvette": (lambda: mv.custom_scene("lens", "cuvette"), False),
}
_REF = {}


def film_shape(d):
    rx, ry, rz = d.film_res
    return (rz, ry, rx)


def _rays_tangents(oracle, d, rays, spp, pats):
    """(T_h, T_2h) per pattern set from oracle.dda_ray at sigma +- h, +- 2 h over exported segments."""
    sigma = float(np.float32(d.sigma_t))
    h = dm.fd_step(sigma)
    descs = [dm.with_sigma(d, sigma + sg * m * h) for m in (1, 2) for sg in (1, -1)]
    iv = float(pm.inv_vol(d))
    Th = [np.zeros(film_shape(d)) for _ in pats]
    T2h = [np.zeros(film_shape(d)) for _ in pats]
    for i, r in enumerate(rays):
        if r[6] == 0.0:
            continue
        f = [oracle.dda_ray(dd, r[7:10], r[11:14], float(r[10]))[0] for dd in descs]
        nz = np.nonzero(f[0])
        d1 = (f[0][nz] - f[1][nz]) / (2 * h)
        d2 = (f[2][nz] - f[3][nz]) / (4 * h)
        w = float(r[14]) * iv
        for j, pat in enumerate(pats):
            c = w * float(pat[i // spp])
            if c != 0.0:
                Th[j][nz] += c * d1
                T2h[j][nz] += c * d2
    return Th, T2h


def reference(oracle, name):
    """Per case, computed once and left unchanged: the descriptor, the inputs and the converged
    finite-difference tangent films of both pattern sets."""
    if name in _REF:
        return _REF[name]
    make, restated = CASES[name]
    d = make()
    spp = 1 if d.regular_sampling else 2
    per = d.crop_y * d.crop_x
    n = d.n_patterns * per
    rng = np.random.default_rng(11)
    pat = rng.uniform(0.0, 0.1, n).astype(np.float32)
    one = pat.copy()  # lit at one angle only
    one[:2 * per] = 0.0
    one[3 * per:] = 0.0
    pats = (pat, one)
    if restated:
        Th, T2h = [], []
        for p in pats:
            a, b = dm.fd_tangent(lambda s, p=p: oracle.forward(dm.with_sigma(d, s), p, spp=spp, seed=SEED, nthreads=8)[0],
                                 float(np.float32(d.sigma_t)))
            Th.append(a)
            T2h.append(b)
    else:
        proj = Projection(d, DEV)
        rays = proj.rays(n, None, spp, SEED).cpu().numpy()
        proj.close()
        Th, T2h = _rays_tangents(oracle, d, rays, spp, pats)
    conv = [dm.assert_converged(a, b) for a, b in zip(Th, T2h)]
    G0 = rng.uniform(0.0, 1.0, film_shape(d)).astype(np.float32)
    G1 = rng.uniform(-1.0, 1.0, film_shape(d)).astype(np.float32)
    _REF[name] = dict(desc=d, spp=spp, n=n, per=per, pats=pats, T=Th, G=(G0, G1), conv=conv)
    return _REF[name]


def sentinel_call(fn, shape, dtype):
    """fn(out) writes a tensor of `shape` that sits between NaN sentinels; returns it after checking them."""
    n = int(np.prod(shape)) if len(shape) else 1
    pad = 64
    buf = torch.full((n + 2 * pad,), float("nan"), dtype=dtype, device=DEV)
    out = buf[pad:pad + n].view(shape)
    fn(out)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n:]).all()
    assert not torch.isnan(out).any()
    return out.clone()


def raw_forward_dsigma(proj, data, pix, spp, seed):
    return sentinel_call(lambda out: _abi.check(proj.lib.tvam_forward_dsigma(
        proj._plan, data.data_ptr(), None if pix is None else pix.data_ptr(), data.numel(), spp, seed, out.data_ptr(),
        torch.cuda.current_stream().cuda_stream)), proj.film_shape, torch.float32)


def raw_adjoint_dsigma(proj, data, G, pix, spp, seed):
    return sentinel_call(lambda out: _abi.check(proj.lib.tvam_adjoint_dsigma(
        proj._plan, data.data_ptr(), G.data_ptr(), None if pix is None else pix.data_ptr(), data.numel(), spp, seed,
        out.data_ptr(), torch.cuda.current_stream().cuda_stream)), (), torch.float64)


# --------------------------------------------------------------------------- 1-4. film, scalar, consistency, determinism
@pytest.mark.parametrize("name", list(CASES))
def test_tangent_and_scalar_match_oracle_fd(oracle, name):
    R = reference(oracle, name)
    d, spp = R["desc"], R["spp"]
    proj = Projection(d, DEV)
    try:
        for k, (pat, T_ref) in enumerate(zip(R["pats"], R["T"])):
            assert (T_ref > 0).any()
            if d.sigma_t >= 1.0:  # chords longer than 1 / sigma_t: the derivative changes sign along them
                assert (T_ref < 0).any()
            data = dev(pat)
            T = raw_forward_dsigma(proj, data, None, spp, SEED).cpu().numpy()[..., 0].astype(np.float64)
            l2, mx = dm.film_errors(T, T_ref)
            print(f"{name} set {k}: reference convergence {R['conv'][k]:.2e}, film rel L2 {l2:.3e}, max / max {mx:.3e}, "
                  f"negative {np.mean(T_ref < 0):.2f} positive {np.mean(T_ref > 0):.2f}")
            assert l2 < dm.RTOL and mx <= dm.RTOL
            for G in R["G"]:
                g = raw_adjoint_dsigma(proj, data, dev(G), None, spp, SEED)
                g2 = raw_adjoint_dsigma(proj, data, dev(G), None, spp, SEED)
                assert g.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes()  # the same 8 bytes
                g = float(g)
                G64 = G.astype(np.float64)
                ref, scale = float(np.vdot(G64, T_ref)), float(np.vdot(np.abs(G64), np.abs(T_ref)))
                own, own_scale = float(np.vdot(G64, T)), float(np.abs(G64 * T).sum())
                print(f"   g {g:.9e} <G, T_ref> {ref:.9e} (|diff| / <|G|,|T_ref|> {abs(g - ref) / scale:.2e}), "
                      f"against the GPU film {abs(g - own) / own_scale:.2e}")
                assert abs(g - ref) <= 1e-4 * scale
                assert abs(g - own) <= 1e-6 * own_scale
        # the wrappers return the same results
        T2 = proj.forward_dsigma(dev(R["pats"][0]), None, spp, SEED)
        assert T2.shape == proj.film_shape
        g3 = proj.adjoint_dsigma(dev(R["pats"][0]), dev(R["G"][0]), None, spp, SEED)
        assert g3.dim() == 0 and g3.dtype == torch.float64
    finally:
        proj.close()


# --------------------------------------------------------------------------- 5. angle shards
@pytest.mark.parametrize("name", ["collimated", "lens", "square-occ", "traced-cylindrical-telecentric"])
def test_angle_shards_sum_to_the_whole(oracle, name):
    R = reference(oracle, name)
    d, spp, per, n = R["desc"], R["spp"], R["per"], R["n"]
    pat, T_ref, G = R["pats"][0], R["T"][0], R["G"][0]
    total, g = np.zeros(film_shape(d)), 0.0
    half = d.n_patterns // 2
    for a0, a1 in ((0, half), (half, d.n_patterns)):
        ds = d.copy()
        ds.angle_begin, ds.angle_end = a0, a1
        ds.active_base, ds.active_total = a0 * per, n
        sh = Projection(ds, DEV)
        data = dev(pat[a0 * per:a1 * per])
        total += sh.forward_dsigma(data, None, spp, SEED).cpu().numpy()[..., 0]
        g += float(sh.adjoint_dsigma(data, dev(G), None, spp, SEED))
        sh.close()
    l2, mx = dm.film_errors(total, T_ref)
    print(f"{name}: shards' film rel L2 {l2:.3e} max / max {mx:.3e}")
    assert l2 < dm.RTOL and mx <= dm.RTOL
    assert dm.scalar_ok(g, G, T_ref)


# --------------------------------------------------------------------------- 6. sparse active set
@pytest.mark.parametrize("name", ["collimated-regular", "collimated-noplanar", "telecentric", "square-occ"])
def test_sparse_set_equals_dense_with_zeros(oracle, name):
    """Every 3rd entry active: regular sampling draws nothing from the sampler, so the sparse call is
    the dense call with the other patterns zeroed; jittered plans seed their streams by active
    position, so there the dense counterpart is the oracle-independent statement g = <G, T>."""
    R = reference(oracle, name)
    d, spp, n = R["desc"], R["spp"], R["n"]
    pat, G = R["pats"][0], R["G"][0]
    keep = np.arange(0, n, 3)
    pix = pm.dense_pixels(d)[keep].astype(np.int32)
    proj = Projection(d, DEV)
    try:
        Ts = proj.forward_dsigma(dev(pat[keep]), dev(pix, torch.int32), spp, SEED).cpu().numpy().astype(np.float64)
        gs = float(proj.adjoint_dsigma(dev(pat[keep]), dev(G), dev(pix, torch.int32), spp, SEED))
        assert abs(gs - float(np.vdot(G.astype(np.float64), Ts[..., 0]))) <= 1e-6 * float(np.abs(G * Ts[..., 0]).sum())
        if d.regular_sampling:
            zeroed = np.zeros_like(pat)
            zeroed[keep] = pat[keep]
            Td = proj.forward_dsigma(dev(zeroed), None, spp, SEED).cpu().numpy().astype(np.float64)
            gd = float(proj.adjoint_dsigma(dev(zeroed), dev(G), None, spp, SEED))
            # the same rays with the same weights; only the order of the float atomics differs
            assert np.abs(Ts - Td).max() <= 1e-5 * np.abs(Td).max()
            assert abs(gs - gd) <= 1e-6 * float(np.abs(G * Td[..., 0]).sum())
        else:
            assert np.abs(Ts).max() > 0
    finally:
        proj.close()


# --------------------------------------------------------------------------- 7. spp 2, jittered
@pytest.mark.parametrize("name", ["collimated", "lens"])
def test_jittered_streams_are_the_plans_own(oracle, name):
    """Covered against the oracle above at spp 2 (the reference uses the plan's sampler streams);
    here: the same seed gives the same scalar bits and the same film up to the atomics' order, another
    seed gives another film."""
    R = reference(oracle, name)
    d, spp = R["desc"], R["spp"]
    assert spp == 2 and not d.regular_sampling
    data, G = dev(R["pats"][0]), dev(R["G"][0])
    proj = Projection(d, DEV)
    try:
        a = proj.forward_dsigma(data, None, spp, SEED).cpu().numpy().astype(np.float64)
        b = proj.forward_dsigma(data, None, spp, SEED).cpu().numpy().astype(np.float64)
        c = proj.forward_dsigma(data, None, spp, SEED + 1).cpu().numpy().astype(np.float64)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()
        assert np.abs(a - c).max() > 1e-3 * np.abs(a).max()
        ga = proj.adjoint_dsigma(data, G, None, spp, SEED)
        gc = proj.adjoint_dsigma(data, G, None, spp, SEED + 1)
        assert float(ga) != float(gc)
    finally:
        proj.close()


# --------------------------------------------------------------------------- 8. autograd
@pytest.mark.parametrize("name", ["collimated-regular", "lens"])
def test_autograd_sigma_gradient(oracle, name):
    R = reference(oracle, name)
    d, spp = R["desc"], R["spp"]
    pat = R["pats"][0]
    sigma = float(np.float32(d.sigma_t))

    def loss_at(desc, p, s=None):
        proj = Projection(desc, DEV)
        try:
            dose = render(proj, p, None, spp, spp, SEED, SEED, sigma_t=s) if s is not None else \
                render(proj, p, None, spp, spp, SEED, SEED)
            loss = (dose.double() ** 2).mean()
            if p.requires_grad:
                loss.backward()
            return float(loss.detach())
        finally:
            proj.close()

    p = dev(pat).requires_grad_(True)
    s = torch.tensor(sigma, dtype=torch.float32, requires_grad=True)
    loss_at(d, p, s)
    p_plain = dev(pat).requires_grad_(True)
    loss_at(d, p_plain)
    assert torch.equal(p.grad, p_plain.grad)  # bit for bit
    h = 2.0 ** -8
    with torch.no_grad():
        fd = (loss_at(dm.with_sigma(d, sigma + h), dev(pat)) - loss_at(dm.with_sigma(d, sigma - h), dev(pat))) / (2 * h)
    ad = float(s.grad)
    print(f"{name}: AD {ad:.8e} FD {fd:.8e} |AD - FD| / |FD| {abs(ad - fd) / abs(fd):.2e}")
    assert abs(ad - fd) / abs(fd) < 2e-4
    proj = Projection(d, DEV)
    try:
        with pytest.raises(ValueError, match="sigma_t"):
            render(proj, dev(pat), None, spp, spp, SEED, SEED, sigma_t=torch.tensor(sigma + h, requires_grad=True))
        with pytest.raises(ValueError, match="0-dim"):
            render(proj, dev(pat), None, spp, spp, SEED, SEED, sigma_t=torch.full((1,), sigma))
    finally:
        proj.close()


# --------------------------------------------------------------------------- 9. refusals
def test_refusals_name_the_cause():
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    base = pm.projector_scene("collimated", regular=True)
    plans = []
    d = base.copy()
    d.albedo, d.phase_type = 0.5, _abi.PHASE_RAYLEIGH
    plans.append((d, "albedo > 0"))
    d = base.copy()
    d.sensor_type, d.majorant = _abi.SENSOR_RATIO, 3.0
    plans.append((d, "'ratio' / 'delta' sensors"))
    # (a 'delta' sensor needs albedo > 0 to build a plan at all, which is the first refusal)
    d = base.copy()
    d.film_channels = 2
    d.set_target(tri)
    plans.append((d, "surface-aware"))
    d = base.copy()
    d.slab_begin, d.slab_end = 0, 10
    plans.append((d, "film slab"))
    d = base.copy()
    d.sample_time = 1
    plans.append((d, "sample_time"))
    plans.append((dv.double_scene("collimated", regular=True), "'double_cylindrical' plan"))
    projs = [(Projection(d, DEV), why) for d, why in plans]
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for proj, why in projs:
            lib = proj.lib
            nd = proj.desc.n_patterns * proj.desc.crop_y * proj.desc.crop_x
            data = torch.zeros(nd, dtype=torch.float32, device=DEV)
            G = torch.zeros(proj.film_shape, dtype=torch.float32, device=DEV)
            T = torch.zeros(proj.film_shape, dtype=torch.float32, device=DEV)
            g = torch.zeros((), dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(0)[0]
            with pytest.raises(ValueError) as e:
                _abi.check(lib.tvam_forward_dsigma(proj._plan, data.data_ptr(), None, nd, 1, 0, T.data_ptr(), stream))
            assert str(e.value).startswith("tvam_forward_dsigma: ") and why in str(e.value), str(e.value)
            with pytest.raises(ValueError) as e:
                _abi.check(lib.tvam_adjoint_dsigma(proj._plan, data.data_ptr(), G.data_ptr(), None, nd, 1, 0,
                                                   g.data_ptr(), stream))
            assert str(e.value).startswith("tvam_adjoint_dsigma: ") and why in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info(0)[0] == free0
    finally:
        for proj, _ in projs:
            proj.close()

"""Voxel-driven forward: oracle parity for every kernel variant a plan can pick.

tvam_fwd_planar_kernel is instantiated per (Z, NC, MULTI, PF, AB, BIN, REFR, DMAP); the plan picks
one from the scene's geometry (candidate columns nc = floor(2 wmax) + 1 from the DMD pitch against
the voxel size, the staged window ncmax, the slab depth Z).  Every case below is there for one
variant, states it in `expect`, and asserts it through Projection.fwd_variant() before it compares
anything: a case cannot pass while testing another kernel than it names.

Bars (test_gpu_parity.py): relative L2 < 1e-4 of the oracle and, per voxel,
|got - ref| <= 1e-4 max|ref| + 1e-7, for U[0, 0.1) patterns and for patterns lit at one angle
only (the 45 degree one, then an axis-aligned one): there a dropped candidate column is a large
share of its voxel's dose instead of 1 / A of it.

Unreachable from any descriptor (straight rays): NC >= 3 at Z = 60.  A 16-voxel tile spans
15 (2 w - 2 marg_u) columns between its outer voxel centres and nc >= 3 needs 2 w >= 2, so
ncmax >= 36 (planar_fwd_setup), while tvam_planar_fwd_fits wants ncmax (Z / 4) <= 512, i.e.
ncmax <= 34 at Z = 60.  The Z = 60 case therefore runs nc = 2.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.configs import benchy_index_matched, desc_from_config
from drtvam_amd.engine import Projection
from parity_report import report
from parity_util import flipped_pixels, rel_l2

RTOL_L2 = 1e-4  # test_gpu_parity.py:100
DEV = "cuda:0"


def make(cols, film, A, crop=None, angle_range=None):
    """The index-matched 10 mm scene under a cols x cols DMD with film = (x, y, z) voxels;
    crop = (cropx, crop_offset_x)."""
    d = desc_from_config(benchy_index_matched(N=cols, angles=A), angle_range=angle_range)
    d.film_res[0], d.film_res[1], d.film_res[2] = film
    if crop is not None:
        d.crop_x, d.crop_offset_x = crop
    return d


def gt(x):
    return lambda v: v > x


# name -> scene (cols, film, A), knobs, the variant the case is there for (None: the plan must fall
# back to the ray-driven forward) and what the case runs
CASES = {
    # candidate count and staging
    "nc3_dma": dict(cols=64, film=(32, 32, 16), A=16, expect=dict(NC=3, nc=3, BIN=True, DMA=True, SCONST=True, AB=2)),
    "nc4_dma": dict(cols=64, film=(28, 28, 16), A=16, expect=dict(NC=4, nc=4, BIN=True, DMA=True, SCONST=True)),
    # window > 64 columns: no LDS-DMA, register-staged binned slabs, shallow Z
    "nc4_wide": dict(cols=64, film=(23, 23, 16), A=16,
                     expect=dict(NC=4, nc=4, ncmax=gt(64), BIN=True, DMA=False, PF=1, AB=2, Z=8)),
    # the same past one chunk of per-angle constants (TVAM_ACH = 64) with a remainder, one angle part
    "nc4_wide_A72": dict(cols=64, film=(23, 23, 16), A=72, knobs=dict(TVAM_FWD_PARTS=1),
                         expect=dict(NC=4, nc=4, ncmax=gt(64), BIN=True, DMA=False, parts=1)),
    "nc5_ray_driven": dict(cols=64, film=(22, 22, 16), A=16, expect=None),
    "nc1": dict(cols=32, film=(64, 64, 16), A=16, expect=dict(NC=2, nc=1, DMA=True), zeros=True),
    "aniso": dict(cols=48, film=(48, 32, 16), A=16, expect=dict(NC=2, nc=2, DMA=True)),
    # staged from the [row][col] patterns (TVAM_FWD_BIN=0): one row per slice, then two
    "nc3_unbinned": dict(cols=64, film=(32, 32, 64), A=16, knobs=dict(TVAM_FWD_BIN=0),
                         expect=dict(NC=3, nc=3, BIN=False, MULTI=False, PF=4, AB=1)),
    "nc3_unbinned_multi": dict(cols=64, film=(32, 32, 32), A=16, knobs=dict(TVAM_FWD_BIN=0),
                               expect=dict(NC=3, nc=3, BIN=False, MULTI=True, PF=4, AB=1)),
    "nc3_unbinned_pf2": dict(cols=64, film=(32, 32, 64), A=16, knobs=dict(TVAM_FWD_BIN=0, TVAM_PLANAR_FWD_Z=8),
                             expect=dict(NC=3, nc=3, BIN=False, MULTI=False, PF=2, AB=1, Z=8)),
    "nc2_unbinned_ab2": dict(cols=32, film=(32, 32, 32), A=16, knobs=dict(TVAM_FWD_BIN=0, TVAM_PLANAR_FWD_Z=32),
                             expect=dict(NC=2, nc=2, BIN=False, MULTI=False, PF=4, AB=2, Z=32)),
    # the unbinned kernel's per-angle constants past one LDS chunk with a remainder
    "nc2_unbinned_A67": dict(cols=16, film=(16, 16, 16), A=67, knobs=dict(TVAM_FWD_BIN=0, TVAM_FWD_PARTS=1),
                             expect=dict(NC=2, BIN=False, parts=1)),
    # forced depths, slice counts that are no multiple of the depth (nc = 3 does not fit Z = 60).  The
    # depths cap the window: ncmax Z <= 1024 up to Z = 32, ncmax Z / 4 <= 512 beyond, and ncmax is about
    # 15 x + 6 columns for a voxel x = 2 w columns wide.  So Z = 48 / 52 take x <= 2.4 / 2.2 (films
    # 40^2 / 42^2: the third candidate covers up to 0.26 / 0.16 of a column), and Z = 28 only
    # 2 <= x < 2.07 (film 28^2 under 40 columns, ncmax = 36): there the third candidate is a sliver of
    # 0.02 columns, and the case pins the depth and its staging more than the candidate
    "nc3_z8": dict(cols=64, film=(32, 32, 50), A=16, knobs=dict(TVAM_PLANAR_FWD_Z=8), expect=dict(NC=3, nc=3, Z=8)),
    "nc3_z28": dict(cols=40, film=(28, 28, 50), A=8, knobs=dict(TVAM_PLANAR_FWD_Z=28), expect=dict(NC=3, nc=3, Z=28)),
    "nc3_z48": dict(cols=64, film=(40, 40, 50), A=8, knobs=dict(TVAM_PLANAR_FWD_Z=48),
                    expect=dict(NC=3, nc=3, Z=48, BIN=True)),
    "nc3_z52": dict(cols=64, film=(42, 42, 57), A=8, knobs=dict(TVAM_PLANAR_FWD_Z=52),
                    expect=dict(NC=3, nc=3, Z=52, BIN=True)),
    # a window the LDS-DMA staging cannot take at this depth (49 columns x 11 slots > 512): the
    # register-staged binned kernel with two float4s per thread
    "nc3_z40_pf2": dict(cols=64, film=(32, 32, 50), A=16, knobs=dict(TVAM_PLANAR_FWD_Z=40),
                        expect=dict(NC=3, nc=3, Z=40, BIN=True, DMA=False, PF=2, AB=2)),
    "nc2_z60": dict(cols=40, film=(40, 40, 50), A=8, knobs=dict(TVAM_PLANAR_FWD_Z=60),
                    expect=dict(NC=2, nc=2, Z=60, BIN=True, DMA=True)),
    # slice ranges, slab plans, crops
    "nc3_slices": dict(cols=64, film=(32, 32, 50), A=16, expect=dict(NC=3, nc=3), run="slices"),
    "nc3_slab_band": dict(cols=64, film=(32, 32, 32), A=16, expect=dict(NC=3, nc=3), run="slab", slab=(9, 21)),
    # a quarter of the columns, off centre: some tiles' windows clamp into the binned patterns' zero pads
    "nc3_crop": dict(cols=64, film=(32, 32, 16), A=16, crop=(16, 30), expect=dict(NC=3, nc=3, DMA=True)),
    # tile order: 6 x 7 full tiles, then 6 x 7 with partial edge tiles (ragged 5 x 5 super-blocks)
    "tiles_6x7": dict(cols=96, film=(96, 112, 8), A=6, knobs=dict(TVAM_FWD_PARTS=1), expect=dict(NC=2, parts=1)),
    "tiles_6x7_parts3": dict(cols=96, film=(96, 112, 8), A=6, knobs=dict(TVAM_FWD_PARTS=3),
                             expect=dict(NC=2, parts=3)),
    "tiles_ragged": dict(cols=90, film=(90, 100, 8), A=6, knobs=dict(TVAM_FWD_PARTS=1), expect=dict(NC=2, parts=1)),
    "tiles_ragged_parts3": dict(cols=90, film=(90, 100, 8), A=6, knobs=dict(TVAM_FWD_PARTS=3),
                                expect=dict(NC=2, parts=3)),
    # angle counts on the production variant (LDS-DMA, constants loaded one angle pair ahead); one
    # angle part, so the pair look-ahead runs over the whole odd / > 64 count
    "A1": dict(cols=16, film=(16, 16, 16), A=1, expect=dict(NC=2, nc=2, DMA=True, SCONST=True, AB=2, parts=1)),
    "A3": dict(cols=16, film=(16, 16, 16), A=3, knobs=dict(TVAM_FWD_PARTS=1),
               expect=dict(NC=2, nc=2, DMA=True, SCONST=True, AB=2, parts=1)),
    "A67": dict(cols=16, film=(16, 16, 16), A=67, knobs=dict(TVAM_FWD_PARTS=1),
                expect=dict(NC=2, nc=2, DMA=True, SCONST=True, AB=2, parts=1)),
    "A130": dict(cols=16, film=(16, 16, 16), A=130, knobs=dict(TVAM_FWD_PARTS=1),
                 expect=dict(NC=2, nc=2, DMA=True, SCONST=True, AB=2, parts=1)),
    "A130_parts": dict(cols=16, film=(16, 16, 16), A=130, expect=dict(NC=2, nc=2, DMA=True, SCONST=True, parts=gt(1))),
    "A130_shard": dict(cols=16, film=(16, 16, 16), A=130, angle_range=(5, 72), knobs=dict(TVAM_FWD_PARTS=1),
                       expect=dict(NC=2, nc=2, DMA=True, SCONST=True, parts=1)),
}
# the geometries whose adjoint and operator pair are checked too
ADJOINT_CASES = ["nc3_dma", "nc4_dma", "nc4_wide", "nc5_ray_driven", "nc1", "aniso", "tiles_6x7", "tiles_ragged"]


def plan(case, knobs):
    """(descriptor, projection, reported variant or None) of a case, the variant asserted."""
    if case.get("knobs"):
        knobs(**case["knobs"])
    d = make(case["cols"], case["film"], case["A"], case.get("crop"), case.get("angle_range"))
    proj = Projection(d, DEV)
    assert proj.planar
    if case["expect"] is None:  # the DMD is too fine for the staged window: ray-driven forward
        assert not proj.planar_forward
        with pytest.raises(ValueError, match="voxel-driven forward does not serve"):
            proj.fwd_variant()
        return d, proj, None
    assert proj.planar_forward
    v = proj.fwd_variant()
    for key, want in case["expect"].items():
        assert want(v[key]) if callable(want) else v[key] == want, (key, v)
    return d, proj, v


def variant_text(v):
    if v is None:
        return "ray-driven"
    flags = "+".join(f for f in ("BIN", "DMA", "MULTI", "REFR", "SCONST") if v[f]) or "-"
    return f"Z{v['Z']} NC{v['NC']} nc{v['nc']} ncmax{v['ncmax']} AB{v['AB']} PF{v['PF']} {flags} parts{v['parts']}"


def lit_angles(A, a0, a1):
    """The shard's angle at 45 degrees to the axes (else its second angle) and its axis-aligned one."""
    diag = [i for i in range(a0, a1) if (8 * i) % A == 0 and (8 * i // A) % 2 == 1]
    out = [diag[0] if diag else min(a0 + 1, a1 - 1)]
    if a0 not in out:
        out.append(a0 if a0 == 0 else next((i for i in range(a0, a1) if (4 * i) % A == 0), a0))
    return out


def pattern_sets(d, rng):
    """[(label, patterns [A][rows][cols] of the whole angle set, zero outside the plan's shard)]."""
    A = d.n_patterns
    a0, a1 = d.angle_begin, (d.angle_end if d.angle_end >= 0 else A)
    full = np.zeros((A, d.crop_y, d.crop_x), np.float32)
    full[a0:a1] = rng.uniform(0.0, 0.1, (a1 - a0, d.crop_y, d.crop_x))
    sets = [("uniform", full)]
    for a in lit_angles(A, a0, a1):
        one = np.zeros_like(full)
        one[a] = full[a]
        sets.append((f"angle{a}", one))
    return sets, a0, a1


def forward(proj, pat):
    out = proj.forward(torch.as_tensor(np.ascontiguousarray(pat).reshape(-1), device=DEV), None, 1, 0)
    torch.cuda.synchronize()
    return out.cpu().numpy()[..., 0]


def forward_slices(proj, pat):
    """The forward assembled from two slice ranges on the plan's chunks."""
    zc, nz = proj.fwd_chunk, proj.film_shape[0]
    assert 0 < zc < nz
    x = torch.as_tensor(np.ascontiguousarray(pat).reshape(-1), device=DEV)
    out = torch.full(proj.film_shape, float("nan"), dtype=torch.float32, device=DEV)
    proj.forward_slices(x, None, 1, 0, 0, zc, out)
    proj.forward_slices(x, None, 1, 0, zc, nz, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()[..., 0]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_variant_matches_oracle(oracle, knobs, name):
    case = CASES[name]
    d, proj, v = plan(case, knobs)
    sets, a0, a1 = pattern_sets(d, np.random.default_rng(0))
    run, zs, rows = forward, slice(None), slice(None)
    if case.get("run") == "slices":
        run = forward_slices
    elif case.get("run") == "slab":
        # a plan of film slab [z0, z1) over the band of DMD rows that feed it, as a z-slab rank builds
        # it: the oracle's slices [z0, z1) of the whole film (the other rows' rays miss them)
        z0, z1 = case["slab"]
        m = np.empty(d.crop_y, dtype=np.int32)
        _abi.check(_abi.load_library().tvam_row_slices(ctypes.byref(d), m.ctypes.data_as(ctypes.c_void_p)))
        band = np.nonzero((m >= z0) & (m < z1))[0]
        r0, r1 = int(band.min()), int(band.max()) + 1
        ds = d.copy()
        ds.slab_begin, ds.slab_end = z0, z1
        ds.crop_offset_y, ds.crop_y = r0, r1 - r0
        proj = Projection(ds, DEV)
        assert proj.planar_forward
        vs = proj.fwd_variant()
        for key, want in case["expect"].items():
            assert vs[key] == want, (key, vs)
        v, zs, rows = vs, slice(z0, z1), slice(r0, r1)
    numbers, bad = {}, []
    for label, pat in sets:
        ref, _ = oracle.forward(d, pat.reshape(-1), nthreads=8)
        ref = ref[zs]
        got = run(proj, pat[a0:a1, rows])
        assert got.shape == ref.shape
        e, worst, top = rel_l2(got, ref), float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
        numbers[f"rel_l2_{label}"] = e
        numbers[f"worst_{label}"] = worst / top
        assert top > 0.0
        if not e < RTOL_L2:
            bad.append((label, "rel_l2", e))
        if not worst <= 1e-4 * top + 1e-7:
            bad.append((label, "worst voxel", worst, top))
        if case.get("zeros"):
            # voxels between the rays of a coarse DMD: exactly 0 where the oracle's are (and the
            # single-angle patterns leave some, or the check would be empty)
            zero = ref == 0.0
            numbers[f"zero_{label}"] = int(zero.sum())
            if label != "uniform":
                assert zero.any() and not zero.all()
            if np.any(got[zero] != 0.0):
                bad.append((label, "nonzero where the oracle is 0", int(np.count_nonzero(got[zero]))))
    print(name, variant_text(v), numbers)
    report(variant=variant_text(v), **numbers)
    assert not bad, (variant_text(v), bad)


@pytest.mark.parametrize("name", ADJOINT_CASES)
def test_adjoint_and_operator_pair(oracle, knobs, name):
    """The adjoint at the forward's geometries: relative L2 < 1e-4 of the oracle's, no entry beyond
    fp32 rounding (parity_util.flipped_pixels; regular sampling draws nothing and both sides take
    the angles' sines and cosines on the host, so none is expected), and <A p, G> = <p, A^T G>
    within 1e-6 sum|A p . G| (test_gpu_scattering.py::test_dot_product)."""
    case = CASES[name]
    d, proj, v = plan(case, knobs)
    fx, fy, fz = case["film"]
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(1)
    G = rng.uniform(-1, 1, (fz, fy, fx)).astype(np.float32)
    gref, _ = oracle.adjoint(d, G, nthreads=8)
    gabs, _ = oracle.adjoint(d, np.abs(G), nthreads=8)
    Gt = torch.as_tensor(G, device=DEV)
    AtG = proj.adjoint(Gt, n, None, 1, 0)
    g = AtG.cpu().numpy()
    flip = flipped_pixels(g, gref, gabs)
    e = rel_l2(g, gref)
    p = torch.as_tensor(rng.uniform(0, 1, n).astype(np.float32), device=DEV)
    Ap = proj.forward(p, None, 1, 0)[..., 0]
    terms = Ap.double() * Gt.double()
    lhs, rhs, scale = float(terms.sum()), float(torch.dot(p.double(), AtG.double())), float(terms.abs().sum())
    numbers = dict(rel_l2_adjoint=e, flagged=int(flip.sum()), of=int(n), dot_gap=abs(lhs - rhs) / scale)
    print(name, variant_text(v), numbers)
    report(variant=variant_text(v), **numbers)
    assert e < RTOL_L2, numbers
    assert int(flip.sum()) == 0, (numbers, np.nonzero(flip)[0][:8])
    assert abs(lhs - rhs) <= 1e-6 * scale, numbers

"""Device-memory ownership of a plan (TvamDevBuf, tvam_plan.h): everything a plan allocates -- its
tables at creation, the ray records, sparse scratch, visit lists, bin scratch and bin cache of its
calls -- is counted by tvam_device_bytes() while the plan lives and gone when it is destroyed, also
when the creation fails half way.  Only the library's own counter is read, so other users of the
device do not disturb the tests.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from drtvam_amd import _abi
from drtvam_amd.configs import benchy_index_matched, cylindrical_refraction, desc_from_config
from drtvam_amd.engine import Projection, device_bytes
from test_oracle_surface import cube_tris

DEV = "cuda:0"
SCATTER_CHUNK_SLOTS = 50000  # 12 * 32 * 32 pixels * 2 spp * 6 later segments = 147456 slots: 3 chunks


def scattering_desc():
    cfg = benchy_index_matched(N=32, angles=12, sigma_t=0.1, regular_sampling=False, spp=2)
    cfg["vial"]["medium"]["albedo"] = 0.5
    cfg["vial"]["medium"]["phase"] = {"type": "rayleigh"}
    cfg["max_depth"] = 8
    cfg["rr_depth"] = 8
    d = desc_from_config(cfg)
    d.flags |= _abi.FLAG_NO_ZERO_SKIP  # (the forward bin cache serves only plans that do not skip zero pixels)
    return d


def surface_desc():
    d = desc_from_config(benchy_index_matched(N=24, angles=12, size_mm=4.0, r=2.9, regular_sampling=False, spp=2))
    d.film_channels = 2
    d.set_target(cube_tris([-1.1, -0.7, -0.9], [0.8, 1.3, 0.6]))
    return d


def telecentric_desc():
    cfg = benchy_index_matched(N=24, angles=12, size_mm=4.0, r=2.9, regular_sampling=False, spp=2)
    cfg["projector"] |= {"type": "telecentric", "aperture_radius": 2.0, "focus_distance": 20.0}
    return desc_from_config(cfg)


# name -> (descriptor, spp, sparse active set)
KINDS = {
    "planar": (lambda: desc_from_config(benchy_index_matched(N=24, angles=12)), 1, False),
    "refracted_planar": (lambda: desc_from_config(cylindrical_refraction(N=32, angles=12)), 1, False),
    "jittered_tile": (lambda: desc_from_config(benchy_index_matched(N=24, angles=12, regular_sampling=False, spp=2)),
                      2, False),
    "sparse": (lambda: desc_from_config(benchy_index_matched(N=24, angles=12, regular_sampling=False, spp=2)), 2, True),
    "scattering_bins": (scattering_desc, 2, False),
    "surface_aware": (surface_desc, 2, False),
    "telecentric": (telecentric_desc, 2, False),
}


def _use(proj, d, spp, sparse):
    """One forward and one adjoint of the plan."""
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(0)
    pix = None
    if sparse:
        keep = np.sort(rng.choice(n, n // 4, replace=False))
        pix = torch.as_tensor(keep.astype(np.int32), device=DEV)
        n = keep.size
    if d.film_channels == 2:
        proj.set_volumes(proj.compute_volume(64))
    pat = torch.as_tensor(rng.uniform(0.0, 0.1, n).astype(np.float32), device=DEV)
    dose = proj.forward(pat, pix, spp, 5)
    G = torch.as_tensor(rng.uniform(-1, 1, tuple(dose.shape)).astype(np.float32), device=DEV)
    grad = proj.adjoint(G if d.film_channels == 2 else G[..., 0].contiguous(), n, pix, spp, 6)
    torch.cuda.synchronize()
    assert float(dose.sum()) > 0.0 and float(grad.abs().sum()) > 0.0


@pytest.mark.parametrize("kind", list(KINDS))
def test_create_use_destroy_returns_every_byte(kind, knobs):
    make, spp, sparse = KINDS[kind]
    if kind == "scattering_bins":
        knobs(TVAM_BIN_CHUNK_SLOTS=SCATTER_CHUNK_SLOTS)
    d = make()
    gc.collect()  # plans other tests left to the collector go now, not in the middle of this test
    start = device_bytes()
    peaks = []
    for cycle in range(2):
        proj = Projection(d, DEV)
        created = device_bytes()
        assert created > start
        _use(proj, d, spp, sparse)
        if kind == "planar":
            assert proj.planar and proj.planar_forward
        if kind == "refracted_planar":
            assert proj.planar
        if kind in ("jittered_tile", "sparse"):
            assert not proj.planar
        if kind == "scattering_bins":
            st = proj.bin_stats()
            assert st["chunks"] >= 3 and st["cache_bytes"] > 0 and st["scratch_bytes"] > 0, st
        if kind == "telecentric":
            assert proj.cone
        peaks.append(device_bytes())
        if kind != "surface_aware":  # (whose per-path kernels need no buffers of their own)
            assert peaks[-1] > created  # the calls' own buffers: ray records, scratch, visit lists
        proj.close()
        assert device_bytes() == start
    assert peaks[0] == peaks[1]  # nothing is kept between plans


def test_failing_create_returns_every_byte():
    """A creation that fails after device memory was taken: occluder triangles are uploaded, then a
    256 x 256 tile does not fit the LDS."""
    cfg = benchy_index_matched(N=24, angles=12)
    cfg["sensor"]["film"] |= {"resx": 256, "resy": 256}
    d = desc_from_config(cfg, tile=256)
    d.set_occluders(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32))
    assert tuple(d.film_res)[:2] == (256, 256) and d.tile == 256
    Projection(desc_from_config(benchy_index_matched(N=24, angles=12)), DEV).close()  # the runtime is up
    gc.collect()
    start = device_bytes()
    with pytest.raises(ValueError, match="tile too large for LDS"):
        Projection(d, DEV)
    assert device_bytes() == start


def test_grown_ray_records_are_replaced_not_leaked():
    """spp 1 twice (both record slots), then spp 3: a slot's records are reallocated, at 24 bytes
    per ray (float4 + int2) at least 2 n more than before; destroy returns everything."""
    d = desc_from_config(benchy_index_matched(N=24, angles=12, regular_sampling=False, spp=1))
    n = d.n_patterns * d.crop_y * d.crop_x
    pat = torch.full((n,), 0.05, device=DEV)
    gc.collect()
    start = device_bytes()
    proj = Projection(d, DEV)
    proj.forward(pat, None, 1, 1)
    proj.forward(pat, None, 1, 2)
    small = device_bytes()
    proj.forward(pat, None, 3, 1)
    torch.cuda.synchronize()
    assert device_bytes() >= small + 2 * n * 24
    assert proj.tile_stats()["spp"] == 3
    proj.close()
    assert device_bytes() == start


# bin_stats() of the three calls below at the parent of the change that introduced TvamDevBuf (read
# from a run of that commit on an MI355X): the capacities folded into the owners report the same bytes
BIN_STATS_PARENT = {
    "forward": dict(chunks=3, cached=0, stored=3, entries=28240, chunk_paths=8332, cache_bytes=7325956,
                    scratch_bytes=3112428, count_mismatch=0),
    "forward_cached": dict(chunks=3, cached=3, stored=0, entries=28240, chunk_paths=8332, cache_bytes=7325956,
                           scratch_bytes=3112428, count_mismatch=0),
    "adjoint": dict(chunks=3, cached=0, stored=0, entries=28975, chunk_paths=8332, cache_bytes=7325956,
                    scratch_bytes=3115516, count_mismatch=0),
}


def test_bin_stats_report_the_same_bytes(knobs):
    knobs(TVAM_BIN_CHUNK_SLOTS=SCATTER_CHUNK_SLOTS)
    d = scattering_desc()
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(0)
    pat = torch.as_tensor(rng.uniform(0.0, 0.1, n).astype(np.float32), device=DEV)
    G = torch.as_tensor(rng.uniform(-1, 1, (32, 32, 32)).astype(np.float32), device=DEV)
    proj = Projection(d, DEV)
    got = {}
    proj.forward(pat, None, 2, 5)
    got["forward"] = proj.bin_stats()
    proj.forward(pat, None, 2, 5)
    got["forward_cached"] = proj.bin_stats()
    proj.adjoint(G, n, None, 2, 6)
    got["adjoint"] = proj.bin_stats()
    proj.close()
    print("bin stats", got)
    assert got == BIN_STATS_PARENT

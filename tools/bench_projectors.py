"""Forward / adjoint times of the telecentric projector on config 2's geometry (N^3 voxels, N angles,
N x N DMD, index matched; default N = 400), against the collimated jittered (spp 1) per-ray tile
path on the same GPU in the same process.  The aperture / focus ratio is the reference docs'
telecentric example (aperture_radius 10 at focus_distance 150), focus_distance = distance.

One JSON line per variant (HIP-event times of whole calls, min and median of `reps` after a warm-up
call): the brick-binned forward (first call of a seed = record writer + fill + sort + march, and the
cached call = reweight + march), the per-ray atomic forward, the adjoint, tvam_plan_bin_stats and
the dominant kernel's launch time; then the collimated yardstick and a summary line with the ratios.
usage: python tools/bench_projectors.py [N] [reps]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drtvam_amd import _abi  # noqa: E402
from drtvam_amd.configs import benchy_index_matched, desc_from_config  # noqa: E402
from drtvam_amd.engine import Projection  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def config(N, kind):
    cfg = benchy_index_matched(N=N, angles=N, regular_sampling=False, spp=1)
    if kind != "collimated":
        F = cfg["projector"]["distance"]
        cfg["projector"] |= {"type": kind, "aperture_radius": F * 10.0 / 150.0, "focus_distance": F}
    return cfg


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    assert torch.cuda.is_available(), "bench_projectors.py needs a GPU"
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(N * N * N, generator=g) * 0.1).cuda()
    G = (torch.rand((N, N, N), generator=g) * 2 - 1).cuda()
    out = {}

    def run(name, kind, flags, cached=False):
        d = desc_from_config(config(N, kind))
        d.flags = flags
        proj = Projection(d, "cuda:0")
        dose = proj.forward(x, None, 1, 0)
        rec = {"variant": name, "N": N, "path": int(proj.lib.tvam_plan_path(proj._plan))}
        if cached:  # every call after the first is served from the bin cache
            fmin, fmed = timed(lambda: proj.forward(x, None, 1, 0, out=dose), reps)
        else:       # a new seed per call: nothing cached, ray records rebuilt
            seed = [0]

            def f():
                seed[0] += 1
                proj.forward(x, None, 1, seed[0], out=dose)
            fmin, fmed = timed(f, reps)
        rec |= {"fwd_ms_min": fmin, "fwd_ms_med": fmed, "bin_stats": proj.bin_stats()}
        proj.kernel_time(True)
        proj.forward(x, None, 1, 0, out=dose)
        kms, kn = proj.kernel_time(False)
        rec |= {"kernel_ms": kms, "kernel_launches": kn}
        grad = proj.adjoint(G, x.numel(), None, 1, 0)
        seed = [0]

        def a():
            seed[0] += 1
            proj.adjoint(G, x.numel(), None, 1, seed[0], out=grad)
        amin, amed = timed(a, reps)
        rec |= {"adj_ms_min": amin, "adj_ms_med": amed, "dose_sum": float(dose.double().sum()),
                "visits": proj.count_visits(1, 0)}
        print(json.dumps(rec), flush=True)
        out[name] = rec
        proj.close()

    nz = _abi.FLAG_NO_ZERO_SKIP
    run("telecentric_binned_first", "telecentric", _abi.FLAG_BIN_FIRST | nz)
    run("telecentric_binned_cached", "telecentric", _abi.FLAG_BIN_FIRST | nz, cached=True)
    run("telecentric_atomic", "telecentric", _abi.FLAG_SCATTER_ATOMIC | nz)
    run("collimated_tile_jitter", "collimated", nz)
    y = out["collimated_tile_jitter"]
    print(json.dumps({"summary": {k: {"fwd_vs_tile": v["fwd_ms_med"] / y["fwd_ms_med"],
                                      "adj_vs_tile": v["adj_ms_med"] / y["adj_ms_med"]}
                                  for k, v in out.items() if k != "collimated_tile_jitter"}}), flush=True)


if __name__ == "__main__":
    main()

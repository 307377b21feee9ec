"""Measurement of the extinction-derivative entries: tvam_forward_dsigma and
tvam_adjoint_dsigma beside the plan's own tvam_forward and tvam_adjoint, in one process and in this
order per repetition, by device events around each call (medians of --reps after --warmup).

Scene: bench.py's config 2 (index-matched, N^3 voxels, N x N DMD, `angles` patterns, regular
sampling, one ray per pixel), whose own forward and adjoint are the planar kernels; the derivative
entries march every ray with the per-ray DDA, the tangent film with global float atomics."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from drtvam_amd import _abi  # noqa: E402
from drtvam_amd.configs import benchy_index_matched, desc_from_config  # noqa: E402
from drtvam_amd.engine import Projection  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--angles", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    d = desc_from_config(benchy_index_matched(N=args.n, angles=args.angles))
    n = d.n_patterns * d.crop_y * d.crop_x
    rng = np.random.default_rng(0)
    pat = torch.as_tensor(rng.uniform(0.0, 0.1, n).astype(np.float32), device=dev)
    proj = Projection(d, dev)
    G = torch.as_tensor(rng.uniform(0.0, 1.0, proj.film_shape).astype(np.float32), device=dev)
    dose = torch.empty(proj.film_shape, dtype=torch.float32, device=dev)
    grad = torch.empty(n, dtype=torch.float32, device=dev)
    calls = {
        "forward_ms": lambda: proj.forward(pat, None, 1, 0, out=dose),
        "adjoint_ms": lambda: proj.adjoint(G, n, None, 1, 0, out=grad),
        "forward_dsigma_ms": lambda: proj.forward_dsigma(pat, None, 1, 0),
        "adjoint_dsigma_ms": lambda: proj.adjoint_dsigma(pat, G, None, 1, 0),
    }
    times = {k: [] for k in calls}
    for _ in range(args.warmup + args.reps):
        for k, fn in calls.items():
            times[k].append(event_ms(fn))
    rec = {"lib": os.path.basename(_abi.LIB_PATH), "n": args.n, "angles": args.angles, "rays": n,
           "visits": int(proj.count_visits(1, 0)), "planar": proj.planar, "planar_forward": proj.planar_forward}
    for k, v in times.items():
        v = v[args.warmup:]
        rec[k] = statistics.median(v)
        rec[k + "_min_max"] = [min(v), max(v)]
    T = proj.forward_dsigma(pat, None, 1, 0)
    g = float(proj.adjoint_dsigma(pat, G, None, 1, 0))
    own = float((G.double() * T.double()).sum())
    rec["g_sigma"] = g
    rec["g_vs_own_film"] = abs(g - own) / float((G.double() * T.double()).abs().sum())
    proj.close()
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Measurement of the 'custom' vial path: forward and adjoint of a mesh vial
against the same scene behind the index-matched vial, in one process.

Scene: telecentric projector, 200 angles x 200 x 200 pixels of 0.025 mm, spp 1, a 128^3 film of
4.6 mm.  Vials: the golden cuvette (16 triangles, staged in LDS), a tessellated tube of 2 x 2048
triangles (read through the caches), and an index-matched tube of the tessellated tube's inner
radius as the yardstick.

Numbers: the per-ray atomic forward kernel from tvam_plan_kernel_time (HIP events around the
launch), the adjoint and the brick-binned forward (a fresh seed per call: nothing served from the
bin cache) from torch events around the call, medians of --reps calls after --warmup.

A library built with -DTVAM_MESH_BRUTE=1 (TVAM_CXXFLAGS of csrc/build.sh), named by the TVAM_LIB
environment variable, runs the same kernels looping over every triangle: run this script once per
library and compare the lines."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from drtvam_amd import _abi  # noqa: E402
from drtvam_amd.configs import desc_from_config  # noqa: E402
from drtvam_amd.engine import Projection  # noqa: E402

import mesh_vial_model as mv  # noqa: E402


def scene(vial, angles, px, film):
    cfg = {
        "vial": {"type": "index_matched", "r": 3.4, "height": 10.0,
                 "medium": {"ior": 1.33, "extinction": 0.06, "albedo": 0.0}},
        "projector": {"type": "telecentric", "n_patterns": angles, "resx": px, "resy": px, "pixel_size": 5.0 / px,
                      "motion": "circular", "distance": 20.0, "aperture_radius": 0.01, "focus_distance": 20.0},
        "sensor": {"type": "dda", "scalex": 4.6, "scaley": 4.6, "scalez": 4.6,
                   "film": {"type": "vfilm", "resx": film, "resy": film, "resz": film}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.9, "tu": 0.95},
    }
    d = desc_from_config(cfg)
    if vial != "index_matched":
        d.vial_type = _abi.VIAL_CUSTOM
        d.vial_ior = 1.4702
        outer, inner = mv.cuvette() if vial == "cuvette" else (mv.tessellated_tube(3.9, 5.0),
                                                               mv.tessellated_tube(3.4, 5.0, phase=0.05))
        d.set_vial_meshes(outer, inner)
    return d


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--angles", type=int, default=200)
    ap.add_argument("--px", type=int, default=200)
    ap.add_argument("--film", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vials", default="index_matched,cuvette,tube")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    n = args.angles * args.px * args.px
    rng = np.random.default_rng(0)
    pat = torch.as_tensor(rng.uniform(0.0, 0.1, n).astype(np.float32), device=dev)
    G = torch.as_tensor(rng.uniform(0.0, 1.0, (args.film,) * 3).astype(np.float32), device=dev)
    lines = []
    for vial in args.vials.split(","):
        d = scene(vial, args.angles, args.px, args.film)
        rec = {"lib": os.path.basename(_abi.LIB_PATH), "vial": vial, "angles": args.angles, "px": args.px,
               "film": args.film, "spp": 1}
        d.flags = _abi.FLAG_SCATTER_ATOMIC
        proj = Projection(d, dev)
        kt = []
        for i in range(args.warmup + args.reps):
            proj.kernel_time(True)
            dose = proj.forward(pat, None, 1, 7)
            ms, launches = proj.kernel_time(False)
            assert launches == 1
            if i >= args.warmup:
                kt.append(ms)
        rec["forward_atomic_kernel_ms"] = statistics.median(kt)
        rec["forward_atomic_kernel_ms_all"] = kt
        rec["dose_sum"] = float(dose.double().sum())
        adj = timed(lambda: proj.adjoint(G, n, None, 1, 7), args.reps, args.warmup)
        rec["adjoint_call_ms"] = statistics.median(adj)
        rec["adjoint_call_ms_all"] = adj
        rec["grad_sum"] = float(proj.adjoint(G, n, None, 1, 7).double().sum())
        proj.close()
        d.flags = _abi.FLAG_BIN_FIRST
        proj = Projection(d, dev)
        seed = [100]

        def binned():
            seed[0] += 1
            proj.forward(pat, None, 1, seed[0])

        b = timed(binned, args.reps, args.warmup)
        rec["forward_binned_call_ms"] = statistics.median(b)
        rec["forward_binned_call_ms_all"] = b
        proj.close()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

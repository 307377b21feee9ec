"""Measurement of the traced 'cylindrical' and 'square' vials: forward and
adjoint of the analytic glass tube and cuvette beside their mesh forms and a yardstick in the same
process, alternating between the five per repetition:

    index_matched   the index-matched tube of radius 3.4 (the yardstick)
    cylindrical     glass tube r_ext 3.9 / r_int 3.4, traced analytically (tvam_plan_create_traced)
    tube_mesh       the same tube as a 'custom' vial of 2 x 2048 triangles (tools/bench_custom_vial.py's)
    square          glass cuvette w_ext 7.8 / w_int 6.8, traced analytically
    cuboid_mesh     the same cuboids as a 'custom' vial of 2 x 12 triangles

Scene: telecentric projector, 200 angles x 200 x 200 pixels of 0.025 mm, spp 1, a 128^3 film of
4.6 mm, glass 1.4702 around a resin of 1.33, height 10.

Numbers, by device events, medians of --reps after --warmup: the per-ray atomic forward kernel
(tvam_plan_kernel_time), the adjoint call, the brick-binned forward call with a fresh seed (nothing
served from the bin cache) and with a repeated seed (served from it)."""
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


VIALS = "index_matched,cylindrical,tube_mesh,square,cuboid_mesh"


def scene(vial, angles, px, film):
    medium = {"extinction": 0.06, "albedo": 0.0, "ior": 1.33}
    if vial == "cylindrical":
        v = {"type": "cylindrical", "r_ext": 3.9, "r_int": 3.4, "ior": 1.4702, "height": 10.0, "medium": medium}
    elif vial == "square":
        v = {"type": "square", "w_ext": 7.8, "w_int": 6.8, "ior": 1.4702, "height": 10.0, "medium": medium}
    else:
        v = {"type": "index_matched", "r": 3.4, "height": 10.0, "medium": medium}
    cfg = {
        "vial": v,
        "projector": {"type": "telecentric", "n_patterns": angles, "resx": px, "resy": px, "pixel_size": 5.0 / px,
                      "motion": "circular", "distance": 20.0, "aperture_radius": 0.01, "focus_distance": 20.0},
        "sensor": {"type": "dda", "scalex": 4.6, "scaley": 4.6, "scalez": 4.6,
                   "film": {"type": "vfilm", "resx": film, "resy": film, "resz": film}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.9, "tu": 0.95},
    }
    d = desc_from_config(cfg)
    if vial in ("cylindrical", "square"):
        assert d.traced_vial  # the config path marks a telecentric projector behind a glass vial
    if vial == "tube_mesh":
        d.vial_type = _abi.VIAL_CUSTOM
        d.vial_ior = 1.4702
        d.set_vial_meshes(mv.tessellated_tube(3.9, 5.0), mv.tessellated_tube(3.4, 5.0, phase=0.05))
    if vial == "cuboid_mesh":
        d.vial_type = _abi.VIAL_CUSTOM
        d.vial_ior = 1.4702
        d.set_vial_meshes(*mv.square_vial_meshes(6.8, 7.8, 10.0))
    return d


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--angles", type=int, default=200)
    ap.add_argument("--px", type=int, default=200)
    ap.add_argument("--film", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vials", default=VIALS)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    n = args.angles * args.px * args.px
    rng = np.random.default_rng(0)
    pat = torch.as_tensor(rng.uniform(0.0, 0.1, n).astype(np.float32), device=dev)
    G = torch.as_tensor(rng.uniform(0.0, 1.0, (args.film,) * 3).astype(np.float32), device=dev)
    vials = args.vials.split(",")
    plans, times = {}, {}
    for vial in vials:
        d = scene(vial, args.angles, args.px, args.film)
        d.flags = _abi.FLAG_SCATTER_ATOMIC
        atomic = Projection(d, dev)
        d.flags = _abi.FLAG_BIN_FIRST | _abi.FLAG_NO_ZERO_SKIP
        plans[vial] = (atomic, Projection(d, dev))
        times[vial] = {"forward_atomic_kernel_ms": [], "adjoint_call_ms": [], "forward_binned_fresh_call_ms": [],
                       "forward_binned_cached_call_ms": []}
    for i in range(args.warmup + args.reps):
        for vial in vials:  # alternating: every repetition visits every vial
            atomic, binned = plans[vial]
            atomic.kernel_time(True)
            atomic.forward(pat, None, 1, 7)
            ms, launches = atomic.kernel_time(False)
            assert launches == 1
            t = times[vial]
            t["forward_atomic_kernel_ms"].append(ms)
            t["adjoint_call_ms"].append(event_ms(lambda: atomic.adjoint(G, n, None, 1, 7)))
            t["forward_binned_fresh_call_ms"].append(event_ms(lambda: binned.forward(pat, None, 1, 100 + i)))
            t["forward_binned_cached_call_ms"].append(event_ms(lambda: binned.forward(pat, None, 1, 100 + i)))
            assert binned.bin_stats()["cached"] == binned.bin_stats()["chunks"] >= 1
    lines = []
    for vial in vials:
        atomic, binned = plans[vial]
        rec = {"lib": os.path.basename(_abi.LIB_PATH), "vial": vial, "angles": args.angles, "px": args.px,
               "film": args.film, "spp": 1}
        for key, v in times[vial].items():
            rec[key] = statistics.median(v[args.warmup:])
            rec[key + "_all"] = v[args.warmup:]
        rec["dose_sum"] = float(atomic.forward(pat, None, 1, 7).double().sum())
        rec["grad_sum"] = float(atomic.adjoint(G, n, None, 1, 7).double().sum())
        rec["visits"] = int(atomic.count_visits(1, 7))
        rec["bin_entries"] = int(binned.bin_stats()["entries"])
        atomic.close()
        binned.close()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

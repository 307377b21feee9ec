"""Time of one tvam_corner call ('filter_corner', a one-off setup pass) beside tvam_radon at spp 1
as the yardstick, at the sizes of BASELINE config 2 (400 angles x 400 x 400 px, index matched) and
config 5 (800 angles x 800 x 800 px, square vial with the occluder): HIP events on the current
stream, the median of 7 calls after a warm-up.  One JSON line per (config, pass).

usage: python tools/bench_corner.py [--out FILE] [--small]   (--small: 1/4-size scenes, a dry run)"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drtvam_amd import _abi  # noqa: E402
from drtvam_amd.configs import benchy_index_matched, desc_from_config, square_occluded  # noqa: E402
from drtvam_amd.engine import Projection  # noqa: E402
from drtvam_amd.utils import cuboid_triangles  # noqa: E402


def timed(fn, reps=7):
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    s = 4 if args.small else 1
    configs = [("config2", benchy_index_matched(N=400 // s), 8.0 / np.sqrt(2.0)),
               ("config5", square_occluded(N=800 // s), 3.8)]
    lines = []
    for name, cfg, dist in configs:
        d = desc_from_config(cfg)
        d.flags |= _abi.FLAG_NO_PLANAR  # setup passes need no planar tables
        proj = Projection(d, "cuda:0")
        n = d.n_patterns * d.crop_y * d.crop_x
        lo, hi = np.asarray(d.bbox_min, np.float64), np.asarray(d.bbox_max, np.float64)
        tris = cuboid_triangles(lo + 0.1 * (hi - lo), lo + 0.9 * (hi - lo))
        keep = proj.corner(dist, 0.2)
        for what, fn in (("tvam_corner", lambda: proj.corner(dist, 0.2)),
                         ("tvam_corner+hits", lambda: proj.corner(dist, 0.2, hits=True)),
                         ("tvam_radon spp 1", lambda: proj.radon(tris, spp=1, seed=0, max_depth=5))):
            med, ms = timed(fn)
            lines.append({"config": name, "pass": what, "entries": n, "median_ms": round(med, 4),
                          "all_ms": [round(x, 4) for x in ms], "kept": int(keep.sum().item()),
                          "device": torch.cuda.get_device_name(0)})
            print(json.dumps(lines[-1]), flush=True)
        proj.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

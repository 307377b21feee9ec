"""The first-order optimisers' update kernels and loops, measured.

Part 1, kernels at n entries (default 64e6, config 2's pattern vector): achieved bytes/s of
tvam_adam_step (28 B per entry), tvam_sgd_step (12 B, 20 B with momentum), the uniform pair
tvam_adam_moments + tvam_adam_apply (20 + 12 B) and, as the yardstick in the same process,
tvam_axpy_clamp (12 B), an existing float4 stream of the same shape.  HIP-event times of single
calls, a warm-up call, min and median of `reps`.

Part 2, iterations per second of TvamProblem over benchy_index_matched(N) (default 400: config 2)
with 'optimizer' adam, sgd (momentum 0.9) and none (the linear L-BFGS), in this process on this
GPU: 20 timed iterations after 5, wall clock around a device synchronisation.

One JSON line per measurement on stdout and appended to <out>/bench_optimizers.jsonl
(default out: profiles/optimizers).
usage: python tools/bench_optimizers.py [--n N_ENTRIES] [--N GRID] [--reps R] [--out DIR] [--no-loops]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drtvam_amd import _abi  # noqa: E402
from drtvam_amd.configs import benchy_index_matched  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64_000_000)
    ap.add_argument("--N", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "optimizers"))
    ap.add_argument("--no-loops", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optimizers.py needs a GPU"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "bench_optimizers.jsonl"), "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    lib = _abi.load_library()
    n = args.n
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda: torch.rand(n, generator=gen, device="cuda")
    p, g, m, v, d = rnd(), rnd() - 0.5, rnd() - 0.5, rnd(), rnd() - 0.5
    work = torch.empty(_abi.LBFGS_WORK_DOUBLES, dtype=torch.float64, device="cuda")
    sn = torch.tensor([0.0, float(n)], dtype=torch.float64, device="cuda")
    P = lambda t: t.data_ptr()

    def moments():
        _abi.check(lib.tvam_adam_moments(n, P(g), P(m), P(v), 0.9, 0.999, 0, P(work), P(sn), st))

    def apply():
        _abi.check(lib.tvam_adam_apply(n, P(p), None, P(m), P(sn), P(sn) + 8, 1e-3, 1e-8, 0, 0.0, st))

    def pair():
        moments()
        apply()

    kernels = [
        ("tvam_axpy_clamp", 12, lambda: _abi.check(lib.tvam_axpy_clamp(n, P(p), 1e-3, P(d), 0.0, P(p), st))),
        ("tvam_sgd_step", 12, lambda: _abi.check(lib.tvam_sgd_step(n, P(p), P(g), None, 1e-3, 0.0, 0, 0.0, st))),
        ("tvam_sgd_step_momentum", 20, lambda: _abi.check(lib.tvam_sgd_step(n, P(p), P(g), P(m), 1e-3, 0.9, 0, 0.0, st))),
        ("tvam_adam_step", 28, lambda: _abi.check(lib.tvam_adam_step(n, P(p), P(g), P(m), P(v), 1e-3, 0.9, 0.999, 1e-8, 0,
                                                                     0.0, st))),
        ("tvam_adam_step_mask", 28, lambda: _abi.check(lib.tvam_adam_step(n, P(p), P(g), P(m), P(v), 1e-3, 0.9, 0.999,
                                                                          1e-8, 1, 0.0, st))),
        ("tvam_adam_moments", 20, moments),
        ("tvam_adam_apply", 12, apply),
        ("tvam_adam_uniform_pair", 32, pair),
    ]
    rate = {}
    for name, bytes_per, fn in kernels:
        tmin, tmed = timed(fn, args.reps)
        rate[name] = bytes_per * n / (tmed * 1e-3)
        emit({"kernel": name, "n": n, "bytes_per_entry": bytes_per, "ms_min": tmin, "ms_med": tmed,
              "TBps_med": rate[name] / 1e12, "vs_axpy_clamp": rate[name] / rate["tvam_axpy_clamp"]})
    del p, g, m, v, d
    torch.cuda.empty_cache()
    if args.no_loops:
        return

    from drtvam_amd.optimize import TvamProblem
    loops = [("lbfgs", None), ("adam", {"type": "adam", "lr": 0.01}),
             ("sgd", {"type": "sgd", "lr": 0.01, "momentum": 0.9})]
    base = None
    for name, entry in loops:
        cfg = benchy_index_matched(N=args.N)
        if entry:
            cfg["optimizer"] = entry
        prob = TvamProblem(cfg, device=torch.device("cuda", 0))
        for i in range(5):
            prob.iteration(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(5, 25):
            prob.iteration(i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 20
        base = base or dt
        emit({"loop": name, "N": args.N, "ms_per_iteration": dt * 1e3, "it_per_s": 1.0 / dt, "vs_lbfgs": base / dt,
              "loss_first": prob.loss_hist[0], "loss_last": prob.loss_hist[-1]})
        del prob
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

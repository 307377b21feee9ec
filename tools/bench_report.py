"""tvam_class_hist, the print report's one pass over dose and target (8 B per entry), measured.

At n entries (default 64e6, a 400^3 film) with 300 edges (the IoU sweep, side 0) and 501 edges (the
dose histogram, side 1), on three inputs against a target that is 20 % object: a uniform U[0, 1.3)
dose; a bimodal one, empty voxels at 0.85 +- 0.02 and object voxels at 0.97 +- 0.01, where the lanes
of a wave want the same few LDS counters; and two exact spikes (0.84 / 0.96), where they want the
same one or two.  Beside it in the same process:
  * the kernel with the per-wave fold never taken (TVAM_REPORT_FOLD=0: every lane adds to LDS
    itself) and always taken (=2), the A/B of the contention remedy, and with half the workgroups;
  * the torch equivalent it replaces, torch.bucketize + torch.bincount per class, and the cheaper
    form with one bincount over slot + class * (n_edges + 2);
  * tvam_axpy_clamp at the same n (12 B per entry), the project's streaming yardstick;
  * one call at n = 1024: what a call costs besides the pass (the edge table's allocation, copy and
    release, the synchronisation).
HIP-event times of single calls, a warm-up call, min and median of `reps` (9).  The kernel's
counts are checked against the torch equivalent's before anything is timed.

One JSON line per measurement on stdout and appended to <out>/bench_report.jsonl (default out:
profiles/report).
usage: python tools/bench_report.py [--n N_ENTRIES] [--reps R] [--out DIR]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drtvam_amd import _abi  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "report"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_report.py needs a GPU"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "bench_report.jsonl"), "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    lib = _abi.load_library()
    n = args.n
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(0)
    P = lambda t: t.data_ptr()

    # the streaming yardstick
    p, d = torch.rand(n, generator=gen, device="cuda"), torch.rand(n, generator=gen, device="cuda") - 0.5
    tmin, axpy_ms = timed(lambda: _abi.check(lib.tvam_axpy_clamp(n, P(p), 1e-3, P(d), 0.0, P(p), st)), args.reps)
    emit({"kernel": "tvam_axpy_clamp", "n": n, "bytes_per_entry": 12, "ms_min": tmin, "ms_med": axpy_ms,
          "TBps_med": 12 * n / (axpy_ms * 1e-3) / 1e12})
    del p, d

    target = (torch.rand(n, generator=gen, device="cuda") < 0.2).float()
    obj = target > 0
    inputs = {"uniform": torch.rand(n, generator=gen, device="cuda") * 1.3}
    noise = torch.randn(n, generator=gen, device="cuda")
    inputs["bimodal"] = torch.where(obj, 0.97 + 0.01 * noise, 0.85 + 0.02 * noise)
    inputs["spikes"] = torch.where(obj, 0.96, 0.84)  # one counter per class
    del noise

    def knob(**kv):
        for name in ("TVAM_EXPERIMENTAL", "TVAM_REPORT_FOLD", "TVAM_REPORT_GRID"):
            os.environ.pop(name, None)
        if kv:
            os.environ["TVAM_EXPERIMENTAL"] = "1"
            for name, v in kv.items():
                os.environ[name] = str(v)

    for k, side in ((300, 0), (501, 1)):
        edges = np.linspace(0, 1.3, k).astype(np.float32)
        edges_dev = torch.from_numpy(edges).cuda()
        counts = torch.empty((2, k + 2), dtype=torch.int64, device="cuda")

        def hist(x, m=None):
            m = x.numel() if m is None else m
            _abi.check(lib.tvam_class_hist(P(x), P(target), m, edges.ctypes.data, k, side, P(counts), st))

        def torch_per_class(x):
            slot = torch.bucketize(x, edges_dev, right=(side == 1))
            return torch.stack([torch.bincount(slot[~obj], minlength=k + 1), torch.bincount(slot[obj], minlength=k + 1)])

        def torch_one_key(x):
            slot = torch.bucketize(x, edges_dev, right=(side == 1))
            return torch.bincount(slot + obj * (k + 2), minlength=2 * (k + 2)).view(2, k + 2)

        for name, x in inputs.items():
            hist(x)
            want = torch_per_class(x)
            assert torch.equal(counts[:, :k + 1], want) and int(counts[:, k + 1].sum()) == 0, "counts differ from torch"
            del want
            rec = {"input": name, "n": n, "n_edges": k, "side": side, "bytes_per_entry": 8}
            tmin, tmed = timed(lambda: hist(x), args.reps)
            emit(dict(rec, kernel="tvam_class_hist", ms_min=tmin, ms_med=tmed, TBps_med=8 * n / (tmed * 1e-3) / 1e12,
                      time_vs_axpy_clamp=tmed / axpy_ms, rate_vs_axpy_clamp=(8 * n / tmed) / (12 * n / axpy_ms)))
            for label, kv in (("fold never", {"TVAM_REPORT_FOLD": 0}), ("fold always", {"TVAM_REPORT_FOLD": 2}),
                              ("1024 workgroups", {"TVAM_REPORT_GRID": 1024})):
                knob(**kv)
                fmin, fmed = timed(lambda: hist(x), args.reps)
                knob()
                emit(dict(rec, kernel="tvam_class_hist, " + label, ms_min=fmin, ms_med=fmed, vs_default=fmed / tmed))
            for what, fn in (("torch bucketize + bincount per class", torch_per_class),
                             ("torch bucketize + one bincount", torch_one_key)):
                qmin, qmed = timed(lambda: fn(x), args.reps)
                emit(dict(rec, kernel=what, ms_min=qmin, ms_med=qmed, vs_tvam_class_hist=qmed / tmed))
                torch.cuda.empty_cache()
        omin, omed = timed(lambda: hist(inputs["uniform"], 1024), args.reps)
        emit({"kernel": "tvam_class_hist", "input": "uniform", "n": 1024, "n_edges": k, "side": side, "ms_min": omin,
              "ms_med": omed})


if __name__ == "__main__":
    main()

"""Time StreamEngine.reset_streams (one HIP launch) against the equivalent
four torch indexed assignments, at 1 / 64 / 4096 evicted streams of a
S=65536, C=10, G=4096 engine (31 GB of rings). Device-event times, both
variants alternating in the same process; prints one JSON line per size.

    python scripts/reset_streams_bench.py [--streams 65536] [--grid 4096]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tskd_amd.engine import StreamEngine  # noqa: E402


def torch_reset(e, idx):
    e.bsum[idx] = 0
    e.bcnt[idx] = 0
    e.proc[idx] = 0
    e.last_val[idx] = float("nan")


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)  # us
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--channels", type=int, default=10)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--evict", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: no CPU fall-back"
    e = StreamEngine(args.streams, args.channels, ring_grid=args.grid,
                     device="cuda")
    g = torch.Generator().manual_seed(0)
    for n in args.evict:
        ids = torch.randperm(args.streams, generator=g)[:n].sort().values
        idx = ids.to("cuda")
        lst = ids.tolist()
        # the launch path as the server uses it: host list in, range check,
        # id upload, one kernel
        kern = lambda: e.reset_streams(lst)       # noqa: E731
        ref = lambda: torch_reset(e, idx)         # noqa: E731
        for _ in range(3):
            kern()
            ref()
        torch.cuda.synchronize()
        tk, tt = [], []
        for _ in range(args.reps):                # alternate the variants
            tk += timed(kern, 1)
            tt += timed(ref, 1)
        nbytes = n * args.channels * (3 * args.grid + 1) * 4
        k50, t50 = statistics.median(tk), statistics.median(tt)
        print(json.dumps({
            "evicted": n, "S": args.streams, "C": args.channels,
            "G": args.grid, "packed": e._packed, "bytes": nbytes,
            "kernel_us_p50": round(k50, 1), "kernel_us_min": round(min(tk), 1),
            "kernel_us_max": round(max(tk), 1),
            "torch_us_p50": round(t50, 1), "torch_us_min": round(min(tt), 1),
            "torch_us_max": round(max(tt), 1),
            "kernel_GBps": round(nbytes / k50 / 1e3, 1),
            "torch_GBps": round(nbytes / t50 / 1e3, 1)}), flush=True)
        # same result, checked once per size on the wiped slots
        e.proc.fill_(1.0)
        e.last_val.fill_(1.0)
        kern()
        torch.cuda.synchronize()
        assert not e.proc[idx].any() and torch.isnan(e.last_val[idx]).all()
        assert int((e.proc[:, 0, 0] == 0).sum()) == n


if __name__ == "__main__":
    main()

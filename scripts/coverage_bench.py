"""Time StreamEngine.coverage (one HIP launch) against the equivalent torch
ops (index_select of the span, > 0, unfold(...).any, sums) on a S=65536,
C=10, G=4096 packed engine whose span wraps the ring end, and the p50 of a
FusedServer trigger with the coverage gate on against off. Device-event
times for the kernel part, both variants alternating in the same process;
prints one JSON line per part.

    python scripts/coverage_bench.py [--streams 65536] [--grid 4096]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tskd_amd.bus import Bus, Producer  # noqa: E402
from tskd_amd.cli.serve import FusedServer  # noqa: E402
from tskd_amd.config import get_global_config  # noqa: E402
from tskd_amd.engine import StreamEngine  # noqa: E402
from tskd_amd.store import PredictionStore  # noqa: E402


def torch_coverage(e):
    """The kernel's three numbers in torch ops (no restore floor)."""
    L, W = e.model_win, e.win_buckets
    span, lo = L + W - 1, e.nproc - L
    idx = (lo + torch.arange(span, device=e.device)) % e.G
    pres = e.bcnt.index_select(2, idx) > 0                   # (S, C, span)
    present = pres.sum(-1)
    imputed = (~pres.unfold(-1, W, 1).any(-1)).sum(-1)
    pos = torch.arange(1, span + 1, device=e.device)
    stale = span - (pres * pos).amax(-1)
    return torch.stack([present, imputed, stale], dim=-1).to(torch.int32)


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def stats(xs, unit):
    return {f"{unit}_p50": round(statistics.median(xs), 1),
            f"{unit}_min": round(min(xs), 1), f"{unit}_max": round(max(xs), 1)}


def bench_kernel(args):
    e = StreamEngine(args.streams, args.channels, ring_grid=args.grid,
                     device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    step = 4096
    for s0 in range(0, e.S, step):          # ~70 % of the buckets hold data
        blk = e.bcnt[s0:s0 + step]
        blk.copy_((torch.rand(blk.shape, device="cuda", generator=g)
                   < 0.7).float() * 12)
    e.bcnt[::7, 3] = 0                      # and some rows none at all
    e.nproc = e.G + 60                      # lo = G - 60: the span wraps
    e.head = e._cleared = e.nproc + e.win_buckets - 1
    span = e.model_win + e.win_buckets - 1
    kern = e.coverage
    ref = lambda: torch_coverage(e)         # noqa: E731
    for _ in range(3):
        got, want = kern(), ref()
    torch.cuda.synchronize()
    assert torch.equal(got, want), "kernel and torch ops disagree"
    tk, tt = [], []
    for _ in range(args.reps):              # alternate the variants
        tk.append(timed(kern))
        tt.append(timed(ref))
    # the (sum, cnt) pairs of the span: what the kernel's cache lines hold
    nbytes = e.S * e.C * span * 4 * e._bst
    k50 = statistics.median(tk)
    print(json.dumps({
        "part": "kernel", "S": e.S, "C": e.C, "G": e.G, "packed": e._packed,
        "span": span, "bytes": nbytes, "reps": args.reps,
        **{"kernel_" + k: v for k, v in stats(tk, "us").items()},
        **{"torch_" + k: v for k, v in stats(tt, "us").items()},
        "kernel_GBps": round(nbytes / k50 / 1e3, 1)}), flush=True)


def make_server(tmp, tag, n_patients, grid, min_coverage):
    cfg = get_global_config()
    bus = Bus(os.path.join(tmp, f"bus_{tag}"))
    store = PredictionStore(os.path.join(tmp, f"pred_{tag}.log"))
    srv = FusedServer(bus, cfg, store, device="cuda", max_streams=n_patients,
                      ring_grid=grid, starting="earliest",
                      min_coverage=min_coverage)
    topics = [cfg.topic_for_channel(c) for c in cfg.channel_names[:8]]
    for t in topics:
        bus.create_topic(t)
    return srv, Producer(bus), topics


def bench_trigger(args):
    """Each timed trigger consumes one 5-s sample of every patient on 8
    channels and produces one new grid point: poll, ingest, fill, score,
    (coverage,) persist — synchronous, host clock around it."""
    n = args.patients
    pids = [f"p{i:06d}" for i in range(n)]
    with tempfile.TemporaryDirectory() as tmp:
        servers = {tag: make_server(tmp, tag, n, args.serve_grid, f)
                   for tag, f in (("off", 0.0), ("on", 0.5))}

        def step(tag, t_s):
            srv, prod, topics = servers[tag]
            for ch, topic in enumerate(topics):
                for pid in pids:
                    prod.produce(topic, pid, f"[{ch}, {96.5 + ch}]",
                                 ts_us=int(t_s * 1e6))
            prod.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scored = srv.trigger()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, scored

        # 14 minutes of event time in 60-s steps bring both past the first
        # full model window (coverage needs nproc >= 120), then 5-s steps
        t_s = 0.0
        for _ in range(16):
            for tag in servers:
                step(tag, t_s)
            t_s += 60.0
        ms = {tag: [] for tag in servers}
        for _ in range(args.reps):
            for tag in servers:         # alternate the variants
                dt, scored = step(tag, t_s)
                assert scored == n, (tag, scored)
                ms[tag].append(dt)
            t_s += 5.0
        on = servers["on"][0]
        print(json.dumps({
            "part": "trigger", "patients": n, "G": args.serve_grid,
            "reps": args.reps,
            **{"off_" + k: v for k, v in stats(ms["off"], "ms").items()},
            **{"on_" + k: v for k, v in stats(ms["on"], "ms").items()},
            "withheld_total": on.timer.gauges.get("withheld_total"),
            "coverage_mean": on.timer.gauges.get("coverage_mean"),
            "coverage_unavailable":
                on.timer.gauges.get("coverage_unavailable", 0)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--channels", type=int, default=10)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--patients", type=int, default=1024,
                    help="FusedServer trigger part (0 skips it)")
    ap.add_argument("--serve-grid", type=int, default=4096)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: no CPU fall-back"
    bench_kernel(args)
    if args.patients:
        bench_trigger(args)


if __name__ == "__main__":
    main()

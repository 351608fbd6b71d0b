"""Cost of the signal-quality gate (docs/PARITY.md divergence 15) on the dense
bf16 ingest and on the whole captured trigger, at the production shape
(S=65536, C=10, G=4096, 60-s triggers at 125 Hz, 8 mapped channels).

Two engines, one built with ``valid_range`` and one without, read the same
raw tensor of N(0, 1) samples; the gated one runs with symmetric bounds
[-t, t] on the mapped channels chosen so that 0 %, 5 % and 50 % of the
samples are rejected (the bounds tensor is rewritten in place, so the same
captured graph serves all three). Gated and ungated launches alternate in one
process; times are device events, median (min-max) of ``--reps``. Prints one
JSON line per part and rejected share.

    python scripts/quality_bench.py [--streams 65536] [--grid 4096]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tskd_amd.engine import StreamEngine  # noqa: E402
from tskd_amd.engine.stream_engine import TriggerGraph  # noqa: E402
from tskd_amd.models import build_model  # noqa: E402
from tskd_amd.ops import GraphedForward, MyCNNEngine  # noqa: E402

# |x| <= t accepts 100 %, 95 %, 50 % of N(0, 1)
SHARES = ((0.0, 1e30), (0.05, 1.959964), (0.50, 0.674490))
CIN = 8


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def stats(xs):
    return {"us_p50": round(statistics.median(xs), 1),
            "us_min": round(min(xs), 1), "us_max": round(max(xs), 1)}


def set_share(eng, t):
    b = torch.tensor([[-t, t]] * CIN + [[-float("inf"), float("inf")]]
                     * (eng.C - CIN), dtype=torch.float32)
    eng.bounds.copy_(b)


def engines(args):
    kw = dict(ring_grid=args.grid, fs=125.0, device="cuda")
    plain = StreamEngine(args.streams, args.channels, **kw)
    gated = StreamEngine(args.streams, args.channels,
                         valid_range=[(None, None)] * args.channels, **kw)
    return plain, gated


def bench_ingest(args, raw):
    plain, gated = engines(args)
    cm = list(range(CIN))
    n = raw.numel()
    for share, t in SHARES:
        set_share(gated, t)
        gated.rej.zero_()
        for _ in range(3):
            plain._launch_ingest(raw, cm)
            gated._launch_ingest(raw, cm)
        torch.cuda.synchronize()
        seen = float(gated.rej.sum()) / (3 * n)
        tp, tg = [], []
        for _ in range(args.reps):          # alternate the variants
            tp.append(timed(lambda: plain._launch_ingest(raw, cm)))
            tg.append(timed(lambda: gated._launch_ingest(raw, cm)))
        print(json.dumps({
            "part": "ingest_dense_bf16", "streams": args.streams,
            "grid": args.grid, "rejected_share": share,
            "rejected_share_seen": round(seen, 4),
            "raw_gb": round(n * 2 / 1e9, 2),
            "ungated": stats(tp), "gated": stats(tg),
            "gated_over_ungated": round(statistics.median(tg)
                                        / statistics.median(tp), 4)}),
            flush=True)


def bench_trigger(args, raw):
    plain, gated = engines(args)
    cm = list(range(CIN))
    torch.manual_seed(0)
    me = MyCNNEngine(build_model("MyCNN5").eval(), device="cuda")
    graphs = []
    for e in (plain, gated):
        while e.nproc == 0 or e.nproc < e.head - e.win_buckets + 1:
            e.ingest_dense(raw, chan_map=cm)
        torch.cuda.synchronize()
        gf = GraphedForward(me, s=args.streams, n=1, dtype=torch.bfloat16,
                            timelast=True, capture=False)
        graphs.append(TriggerGraph(e, raw, cm, gf, stride=12))
    tgp, tgg = graphs
    for share, t in SHARES:
        set_share(gated, t)
        for _ in range(3):
            tgp.replay()
            tgg.replay()
        torch.cuda.synchronize()
        tp, tg = [], []
        for _ in range(args.reps):
            tp.append(timed(tgp.replay))
            tg.append(timed(tgg.replay))
        print(json.dumps({
            "part": "trigger_graph", "streams": args.streams,
            "grid": args.grid, "rejected_share": share,
            "ungated": stats(tp), "gated": stats(tg),
            "gated_over_ungated": round(statistics.median(tg)
                                        / statistics.median(tp), 4)}),
            flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--channels", type=int, default=10)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--part", default="both",
                    choices=["both", "ingest", "trigger"])
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    raw = torch.empty(args.streams, CIN, int(125.0 * 60), device="cuda",
                      dtype=torch.bfloat16)
    for s0 in range(0, args.streams, 4096):     # bounded fp32 staging
        blk = raw[s0:s0 + 4096]
        blk.copy_(torch.randn(blk.shape, device="cuda", generator=g))
    if args.part in ("both", "ingest"):
        bench_ingest(args, raw)
        torch.cuda.empty_cache()
    if args.part in ("both", "trigger"):
        bench_trigger(args, raw)


if __name__ == "__main__":
    main()

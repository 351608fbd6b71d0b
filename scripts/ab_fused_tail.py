#!/usr/bin/env python3
"""Fused serving tail A/B (TSKD_FUSED_TAIL=0 vs 1) at the bench shape.

Two StreamEngine + TriggerGraph pairs live in ONE process (about 16 GB of
rings each at S=65536, G=2048; the raw trigger chunk is shared): arm 0 is
captured with the knob at 0 (gather -> conv -> LSTM/head, the unfused
chain), arm 1 with the knob at 1 (serve_tail). Rounds interleave the arms
— one unmeasured replay after each switch, then a block of replays between
two synchronises — so clock and neighbour drift hit both arms alike.

Prints per-arm median and minimum step time, the per-round deltas, the
spread of the baseline arm's round times (the noise floor the delta has to
clear) and the largest output difference between the arms.

Usage: python scripts/ab_fused_tail.py [--streams 65536] [--rounds 10]
                                       [--reps 20]
Run it under a time limit of its own (e.g. `timeout -k 10 600 python ...`).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def build_arm(knob: str, S: int, me, raw, cm):
    from tskd_amd.engine import StreamEngine
    from tskd_amd.engine.stream_engine import TriggerGraph
    from tskd_amd.ops import GraphedForward
    os.environ["TSKD_FUSED_TAIL"] = knob  # read when the graph is captured
    se = StreamEngine(S, 10, ring_grid=2048, fs=125.0, device="cuda")
    while se.nproc == 0 or se.nproc < se.head - se.win_buckets + 1:
        se.ingest_dense(raw, chan_map=cm)
    torch.cuda.synchronize()
    gf = GraphedForward(me, s=S, n=1, dtype=torch.bfloat16, timelast=True,
                        capture=False)
    tg = TriggerGraph(se, raw, cm, gf, stride=12)
    assert tg.fused_tail == (knob != "0"), (knob, tg.fused_tail)
    return tg


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available()
    assert args.rounds >= 8 and args.reps >= 20, \
        "at least 8 rounds x 20 replays"
    from tskd_amd.models import build_model
    from tskd_amd.ops import MyCNNEngine

    S = args.streams
    torch.manual_seed(3)
    me = MyCNNEngine(build_model("MyCNN5").eval(), device="cuda")
    raw = torch.randn(S, 8, int(125.0 * 60), device="cuda",
                      dtype=torch.bfloat16)
    cm = list(range(8))
    arms = [build_arm("0", S, me, raw, cm), build_arm("1", S, me, raw, cm)]
    os.environ.pop("TSKD_FUSED_TAIL", None)

    # identical state and input in both arms: outputs must agree
    for _ in range(10):
        outs = [tg.replay() for tg in arms]
    torch.cuda.synchronize()
    max_diff = (outs[0] - outs[1]).abs().max().item()

    ms = [[], []]  # per arm: one mean step time per round
    for r in range(args.rounds):
        for a in ((0, 1) if r % 2 == 0 else (1, 0)):
            tg = arms[a]
            tg.replay()                      # unmeasured, after the switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                tg.replay()
            torch.cuda.synchronize()
            ms[a].append((time.perf_counter() - t0) / args.reps * 1e3)
    outs = [tg.replay() for tg in arms]
    torch.cuda.synchronize()
    max_diff = max(max_diff, (outs[0] - outs[1]).abs().max().item())

    med = [statistics.median(m) for m in ms]
    deltas = [(b - f) / b * 100.0 for b, f in zip(ms[0], ms[1])]
    spread = (max(ms[0]) - min(ms[0])) / med[0] * 100.0
    # informational only: the full range above is what the verdict uses,
    # and a single disturbed round on a shared host inflates it
    q = statistics.quantiles(ms[0], n=4)
    iqr = (q[2] - q[0]) / med[0] * 100.0
    gain = (med[0] - med[1]) / med[0] * 100.0
    print(json.dumps({
        "streams": S, "rounds": args.rounds, "reps": args.reps,
        "unfused_ms": {"median": round(med[0], 4),
                       "min": round(min(ms[0]), 4),
                       "rounds": [round(x, 4) for x in ms[0]]},
        "fused_ms": {"median": round(med[1], 4),
                     "min": round(min(ms[1]), 4),
                     "rounds": [round(x, 4) for x in ms[1]]},
        "round_delta_pct": [round(d, 2) for d in deltas],
        "median_gain_pct": round(gain, 2),
        "min_gain_pct": round((min(ms[0]) - min(ms[1])) / min(ms[0]) * 100.0,
                              2),
        "baseline_round_spread_pct": round(spread, 2),
        "baseline_round_iqr_pct": round(iqr, 2),
        "rounds_won_by_fused": sum(d > 0 for d in deltas),
        "ship_as_default": bool(gain >= 3.0 and gain >= 2.0 * spread),
        "max_abs_output_diff": max_diff,
    }), flush=True)


if __name__ == "__main__":
    main()

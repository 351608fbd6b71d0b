#!/usr/bin/env python3
"""Staged fill16 A/B (TSKD_FILL16_STAGED=0 vs 1) at the bench shape.

StreamEngine + TriggerGraph pairs live in ONE process (about 16 GB of rings
each at S=65536, G=2048; the raw trigger chunk is shared): a baseline arm is
captured with ``TSKD_FILL16_STAGED=0`` (the per-lane L1 fill loop), a
default arm with the knob unset (the LDS-staged fill). The knob is read when
a launch is captured, so each graph keeps its own setting afterwards.

``--arms 4`` builds [baseline, default, default, baseline] and reports the
two same-setting pairs as well: engines built at different times in one
process do not run equally fast at S=65536 (their 16 GB rings land in
different places), and with two arms that difference is indistinguishable
from the knob's effect. The verdict then uses the mean of each setting's
two arms per round.

Rounds interleave the arms — one unmeasured replay after each switch, then a
block of replays between two synchronises — so clock and neighbour drift hit
both arms alike. Prints per-arm median and minimum step time, the per-round
deltas, the spread of the baseline arm's round times (the noise floor the
delta has to clear) and the largest output difference between the arms.

Usage: python scripts/ab_fill_tail.py [--streams 65536] [--rounds 10]
                                      [--reps 20] [--arms 2|4]
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

KNOBS = ("TSKD_FILL16_STAGED",)
ARM_ENV = ({"TSKD_FILL16_STAGED": "0"}, {})


def build_arm(env: dict, S: int, me, raw, cm):
    from tskd_amd.engine import StreamEngine
    from tskd_amd.engine.stream_engine import TriggerGraph
    from tskd_amd.ops import GraphedForward
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)  # read when the graph's launches are captured
    se = StreamEngine(S, 10, ring_grid=2048, fs=125.0, device="cuda")
    while se.nproc == 0 or se.nproc < se.head - se.win_buckets + 1:
        se.ingest_dense(raw, chan_map=cm)
    torch.cuda.synchronize()
    gf = GraphedForward(me, s=S, n=1, dtype=torch.bfloat16, timelast=True,
                        capture=False)
    tg = TriggerGraph(se, raw, cm, gf, stride=12)
    assert tg.fused_tail
    for k in KNOBS:
        os.environ.pop(k, None)
    return tg


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--arms", type=int, default=2, choices=(2, 4))
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
    setting = [0, 1] if args.arms == 2 else [0, 1, 1, 0]
    arms = [build_arm(ARM_ENV[k], S, me, raw, cm) for k in setting]

    def max_diff_now(outs):
        return max((o - outs[0]).abs().max().item() for o in outs[1:])

    # identical state and input in every arm: outputs must agree
    for _ in range(10):
        outs = [tg.replay() for tg in arms]
    torch.cuda.synchronize()
    max_diff = max_diff_now(outs)

    ms = [[] for _ in arms]  # per arm: one mean step time per round
    order = list(range(len(arms)))
    for r in range(args.rounds):
        for a in (order if r % 2 == 0 else order[::-1]):
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
    max_diff = max(max_diff, max_diff_now(outs))

    # per setting and round: the mean over that setting's arms
    by = [[statistics.mean(ms[a][r] for a in order if setting[a] == k)
           for r in range(args.rounds)] for k in (0, 1)]
    med = [statistics.median(m) for m in by]
    deltas = [(b - f) / b * 100.0 for b, f in zip(by[0], by[1])]
    spread = (max(by[0]) - min(by[0])) / med[0] * 100.0
    # informational only: the full range above is what the verdict uses,
    # and a single disturbed round on a shared host inflates it
    q = statistics.quantiles(by[0], n=4)
    iqr = (q[2] - q[0]) / med[0] * 100.0
    gain = (med[0] - med[1]) / med[0] * 100.0
    print(json.dumps({
        "streams": S, "rounds": args.rounds, "reps": args.reps,
        "arm_setting": ["baseline" if k == 0 else "default" for k in setting],
        "arm_median_ms": [round(statistics.median(m), 4) for m in ms],
        "baseline_ms": {"median": round(med[0], 4),
                        "min": round(min(by[0]), 4),
                        "rounds": [round(x, 4) for x in by[0]]},
        "default_ms": {"median": round(med[1], 4),
                       "min": round(min(by[1]), 4),
                       "rounds": [round(x, 4) for x in by[1]]},
        "round_delta_pct": [round(d, 2) for d in deltas],
        "median_gain_pct": round(gain, 2),
        "min_gain_pct": round((min(by[0]) - min(by[1])) / min(by[0]) * 100.0,
                              2),
        "baseline_round_spread_pct": round(spread, 2),
        "baseline_round_iqr_pct": round(iqr, 2),
        "rounds_won_by_default": sum(d > 0 for d in deltas),
        "ship_as_default": bool(gain >= 3.0 and gain >= 2.0 * spread),
        "max_abs_output_diff": max_diff,
    }), flush=True)


if __name__ == "__main__":
    main()

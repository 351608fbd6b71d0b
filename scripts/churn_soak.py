#!/usr/bin/env python3
"""Churn soak of the stream lifecycle: ONE FusedServer (one process) is
driven through waves of synthetic patients whose total number is far larger
than --max-streams. Each wave streams for --stay-min stream-minutes and
falls silent; waves overlap so that slots are reused while other patients
are live. One trigger per stream-minute.

Prints one JSON line: triggers, admissions, evictions, rejections, the slot
high-water mark, predictions and per-trigger latency. Stops at the first
error (any exception is fatal; a rejection or a slot above --max-streams
fails the run). Launch it under a time limit of its own, e.g.

    timeout -k 10 600 python scripts/churn_soak.py --device cuda
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--device", default=None)
    ap.add_argument("--max-streams", type=int, default=256)
    ap.add_argument("--wave", type=int, default=96,
                    help="patients admitted per wave")
    ap.add_argument("--waves", type=int, default=12)
    ap.add_argument("--wave-every-min", type=int, default=10)
    ap.add_argument("--stay-min", type=int, default=16)
    ap.add_argument("--evict-idle-s", type=float, default=180.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--ring-grid", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    import torch

    from tskd_amd.bus import Bus, Producer
    from tskd_amd.cli.serve import FusedServer
    from tskd_amd.config import get_global_config
    from tskd_amd.store import PredictionStore

    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    tmp = tempfile.mkdtemp(prefix="churn_soak_")
    cfg = get_global_config()
    bus = Bus(os.path.join(tmp, "bus"))
    store = PredictionStore(os.path.join(tmp, "pred.log"))
    topics = [cfg.topic_for_channel(c)
              for c in cfg.channel_names[:args.channels]]
    for t in topics:
        bus.create_topic(t)
    prod = Producer(bus)
    torch.manual_seed(0)
    srv = FusedServer(bus, cfg, store, device=dev,
                      max_streams=args.max_streams, ring_grid=args.ring_grid,
                      starting="earliest", evict_idle_s=args.evict_idle_s)
    total_min = (args.waves - 1) * args.wave_every_min + args.stay_min + \
        int(args.evict_idle_s // 60) + 2
    lat_ms, n_pred = [], 0
    for minute in range(total_min):
        live = [w for w in range(args.waves)
                if 0 <= minute - w * args.wave_every_min < args.stay_min]
        for step in range(12):
            t_us = int((minute * 60 + step * 5) * 1e6)
            for w in live:
                for i in range(args.wave):
                    pid = f"p{w * args.wave + i + 1:06d}"
                    for ch, topic in enumerate(topics):
                        prod.produce(
                            topic, pid,
                            f"[{ch}, {60 + (w + i + ch + step) % 40}.0]",
                            ts_us=t_us)
        t0 = time.perf_counter()
        n = srv.trigger()
        if dev != "cpu":
            torch.cuda.synchronize()
        lat_ms.append((time.perf_counter() - t0) * 1e3)
        n_pred += n
        c = srv.consumer
        if c.n_rejected():
            raise RuntimeError(f"minute {minute}: {c.n_rejected()} "
                               "samples rejected (table full)")
        if c.sid_high_water() > args.max_streams:
            raise RuntimeError("slot above max_streams")
        if len(set(srv.pid_index.values())) != len(srv.pid_index):
            raise RuntimeError("two live patients share a slot")
    predicted = {p for p, _t, _r in store.tail(store.count())} \
        if store.count() else set()
    c = srv.consumer
    lat = sorted(lat_ms)
    rec = {
        "device": dev, "max_streams": args.max_streams,
        "distinct_patients": args.waves * args.wave,
        "triggers": len(lat_ms), "admitted": c.n_admitted(),
        "evicted": c.n_evicted(), "rejected": c.n_rejected(),
        "active_end": c.n_streams(), "sid_high_water": c.sid_high_water(),
        "predictions": n_pred, "patients_predicted": len(predicted),
        "trigger_ms": {"p50": round(statistics.median(lat), 3),
                       "p99": round(lat[min(len(lat) - 1,
                                            int(0.99 * len(lat)))], 3),
                       "max": round(lat[-1], 3)},
    }
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    ok = (c.n_admitted() == args.waves * args.wave and c.n_rejected() == 0
          and len(predicted) == args.waves * args.wave)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

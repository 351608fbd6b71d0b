"""Time StreamEngine.snapshot (one HIP launch + one copy into pinned memory)
against the torch equivalent (index_select over the wrapped index lists,
cat, copy) and StreamEngine.restore, at 1 / 1024 / 65536 streams of a
S=65536, C=10, G=4096 packed engine (31 GB of rings). Each call is timed
from the host id list to the payload in pinned host memory with device
events; both variants alternate in the same process; one JSON line per
size. ``GBps`` is payload bytes over the whole call, the copy to the host
included — not a kernel bandwidth.

``--daemon N`` instead measures FusedServer's trigger time with and without
a state file at N patients: two servers on two buses fed the same chunks,
triggered alternately.

    python scripts/snapshot_bench.py [--streams 65536] [--grid 4096]
    python scripts/snapshot_bench.py --daemon 1024
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tskd_amd.engine import StreamEngine  # noqa: E402


def torch_snapshot(e, idx, bidx, pidx, host):
    """The same record layout with torch ops only."""
    n = idx.numel()
    bkt, proc = e._bkt, e.proc
    if n * e.G < e.S * bidx.numel():      # cheaper to pick the streams first
        bkt, proc = bkt.index_select(0, idx), proc.index_select(0, idx)
        b = bkt.index_select(2, bidx)
        p = proc.index_select(2, pidx)
    else:
        b = bkt.index_select(2, bidx).index_select(0, idx)
        p = proc.index_select(2, pidx).index_select(0, idx)
    rec = torch.cat([b.reshape(n, e.C, -1), p,
                     e.last_val.index_select(0, idx).unsqueeze(-1)], dim=2)
    out = host[:rec.numel()]
    out.copy_(rec.reshape(-1), non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return out.numpy().reshape(rec.shape)


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def bench_engine(args):
    e = StreamEngine(args.streams, args.channels, ring_grid=args.grid,
                     device="cuda")
    assert e._packed
    for t in (e._bkt, e.proc, e.last_val):
        t.uniform_(1.0, 2.0)
    # a steady-state position whose bucket range and processed tail both wrap
    e.nproc = 3 * args.grid - 20
    e.head = e._cleared = e.nproc + 35
    nbk, keep = 35, e.model_win
    R = 2 * nbk + keep + 1
    bidx = ((e.nproc + torch.arange(nbk)) % e.G).cuda()
    pidx = ((e.nproc - keep + torch.arange(keep)) % e.G).cuda()
    host = torch.empty(args.streams * args.channels * R, pin_memory=True)
    g = torch.Generator().manual_seed(0)
    for n in args.sizes:
        ids = torch.randperm(args.streams, generator=g)[:n].sort().values
        lst = ids.numpy()

        def kern():
            return e.snapshot(lst)

        def ref():
            return torch_snapshot(e, ids.cuda(), bidx, pidx, host)

        snap = kern()
        assert snap.payload.shape == (n, args.channels, R)
        assert np.array_equal(snap.payload, ref())   # same result, once
        frozen = kern()
        frozen.payload = frozen.payload.copy()

        def rest():
            e.head = e.nproc = e._cleared = 0        # "fresh" for the check
            e.restore(frozen)

        for _ in range(2):
            kern(), ref(), rest()
        torch.cuda.synchronize()
        tk, tt, tr = [], [], []
        for _ in range(args.reps):                   # alternate the variants
            tk.append(timed(kern))
            tt.append(timed(ref))
            tr.append(timed(rest))
        assert np.array_equal(kern().payload, frozen.payload)  # round trip
        nbytes = n * args.channels * R * 4
        k50, t50, r50 = (statistics.median(x) for x in (tk, tt, tr))
        print(json.dumps({
            "streams": n, "S": args.streams, "C": args.channels,
            "G": args.grid, "packed": e._packed, "payload_bytes": nbytes,
            "snapshot_us_p50": round(k50, 1),
            "snapshot_us_min": round(min(tk), 1),
            "snapshot_us_max": round(max(tk), 1),
            "torch_us_p50": round(t50, 1), "torch_us_min": round(min(tt), 1),
            "torch_us_max": round(max(tt), 1),
            "restore_us_p50": round(r50, 1),
            "restore_us_min": round(min(tr), 1),
            "restore_us_max": round(max(tr), 1),
            "snapshot_GBps": round(nbytes / k50 / 1e3, 2),
            "torch_GBps": round(nbytes / t50 / 1e3, 2),
            "restore_GBps": round(nbytes / r50 / 1e3, 2)}), flush=True)


def bench_daemon(args):
    from tskd_amd.bus import Bus, Producer
    from tskd_amd.cli.serve import FusedServer
    from tskd_amd.config import get_global_config
    from tskd_amd.store import PredictionStore
    cfg = get_global_config()
    n, nch = args.daemon, 4
    pids = [f"p{i + 1:06d}" for i in range(n)]
    tmp = tempfile.mkdtemp(prefix="snapshot_bench_")
    sides = {}
    for tag in ("plain", "state"):
        bus = Bus(os.path.join(tmp, f"bus_{tag}"))
        topics = [cfg.topic_for_channel(c) for c in cfg.channel_names[:nch]]
        for t in topics:
            bus.create_topic(t)
        torch.manual_seed(7)
        srv = FusedServer(
            bus, cfg, PredictionStore(os.path.join(tmp, f"pred_{tag}.log")),
            device="cuda", max_streams=n, ring_grid=4096,
            starting="earliest", evict_idle_s=240.0,
            state_path=os.path.join(tmp, "serve.snap")
            if tag == "state" else None)
        sides[tag] = (srv, Producer(bus), topics, [])
    warm = 16                                 # triggers before every stream
    for m in range(warm + args.reps):         # is scored (13 min + margin)
        for tag, (srv, prod, topics, ms) in sides.items():
            for step in range(12):
                t = m * 60 + step * 5
                for i, pid in enumerate(pids):
                    for ch in range(nch):
                        prod.produce(topics[ch], pid,
                                     f"[{ch}, {60 + (i + ch + step) % 40}]",
                                     ts_us=int(t * 1e6))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scored = srv.trigger()
            torch.cuda.synchronize()
            if m >= warm:
                assert scored == n
                ms.append((time.perf_counter() - t0) * 1e3)
    plain, state = sides["plain"][3], sides["state"][3]
    size = os.path.getsize(os.path.join(tmp, "serve.snap"))
    print(json.dumps({
        "patients": n, "channels_sent": nch, "triggers": args.reps,
        "state_file_bytes": size,
        "trigger_ms_p50_plain": round(statistics.median(plain), 2),
        "trigger_ms_p50_state": round(statistics.median(state), 2),
        "trigger_ms_min_plain": round(min(plain), 2),
        "trigger_ms_min_state": round(min(state), 2),
        "trigger_ms_max_plain": round(max(plain), 2),
        "trigger_ms_max_state": round(max(state), 2)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--channels", type=int, default=10)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--sizes", type=int, nargs="*",
                    default=[1, 1024, 65536])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--daemon", type=int, default=0, metavar="N")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: no CPU fall-back"
    if args.daemon:
        bench_daemon(args)
    else:
        args.sizes = [min(n, args.streams) for n in args.sizes]
        bench_engine(args)


if __name__ == "__main__":
    main()

"""Time StreamEngine.score_history (one HIP launch) against the reference
path on the same ring (window gather of the K columns of all S streams, row
selection, conv and LSTM launches: StreamEngine.score_history_reference on
bf16 time-last windows) for n = 64, 1024 and 65536 listed streams of a
S=65536, C=10, G=4096 packed engine at nproc = G + 60, so that windows wrap
the ring end; K = 8 columns at stride 12, age given, sigmoid on. Device-event
times of the whole call, both variants alternating in the same process,
results compared first at the test's tolerance; prints one JSON line per n.

    python scripts/history_bench.py [--streams 65536] [--grid 4096]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tskd_amd.engine import StreamEngine  # noqa: E402
from tskd_amd.models import build_model  # noqa: E402
from tskd_amd.ops import MyCNNEngine  # noqa: E402

RTOL = ATOL = 2e-3      # tests/test_history_gpu.py


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--channels", type=int, default=10)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--listed", type=int, nargs="+",
                    default=[64, 1024, 65536])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--stride", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: no CPU fall-back"

    torch.manual_seed(0)
    me = MyCNNEngine(build_model("MyCNN5").eval(), device="cuda")
    e = StreamEngine(args.streams, args.channels, ring_grid=args.grid,
                     device="cuda")
    assert me.supports_history(e.C)
    g = torch.Generator(device="cuda").manual_seed(0)
    step = 4096
    for s0 in range(0, e.S, step):
        blk = e.proc[s0:s0 + step]
        blk.copy_(torch.randn(blk.shape, device="cuda", generator=g) * 2.0)
    e.nproc = e.G + 60                      # windows wrap the ring end
    age = torch.full((e.S, 1), 65.0, device="cuda")
    k, stride = args.k, args.stride
    for n in args.listed:
        n = min(n, e.S)
        # n distinct streams spread over the whole ring
        sids = (torch.arange(n, dtype=torch.int64) * (e.S // n)).numpy()
        kern = lambda: e.score_history(  # noqa: E731
            me, sids, k, stride, age, True)
        ref = lambda: e.score_history_reference(  # noqa: E731
            me, sids, k, stride, age, True, dtype=torch.bfloat16)
        for _ in range(3):
            got, want = kern(), ref()
        torch.cuda.synchronize()
        nan = torch.isnan(got)
        assert torch.equal(nan, torch.isnan(want))
        torch.testing.assert_close(got[~nan], want[~nan], rtol=RTOL,
                                   atol=ATOL)
        diff = (got[~nan] - want[~nan]).abs().max().item()
        tk, tr = [], []
        for _ in range(args.reps):          # alternate the variants
            tk.append(timed(kern))
            tr.append(timed(ref))
        print(json.dumps({
            "S": e.S, "C": e.C, "G": e.G, "packed": e._packed, "n": n,
            "k": k, "stride": stride, "nan_columns": int(nan[0].sum()),
            "reps": args.reps, "max_abs_diff": diff,
            **{"kernel_" + key: v for key, v in stats(tk, "us").items()},
            **{"reference_" + key: v for key, v in stats(tr, "us").items()}}),
            flush=True)


if __name__ == "__main__":
    main()

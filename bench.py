#!/usr/bin/env python3
"""Flagship benchmark: waveform windows/sec (whole node) + p50 step latency,
MyCNN5 8-ch serving on MI355X.

Two modes (BASELINE.json configs):
  --mode pipeline (default; config 4): full fused end-to-end serving step —
      synthetic raw 8-channel 125 Hz waveform chunks (one 60-s trigger per
      step) -> GPU ring-buffer ingest -> fused 180 s/5 s sliding-mean +
      gap-fill -> model-window gather -> fused MFMA conv + LSTM + head +
      sigmoid -> prediction all-gather over RCCL/xGMI (world > 1).
      One model window per stream per trigger (reference serving semantics:
      600 s window / 60 s slide, predictStream.py:248-263).
  --mode infer (config 2): model-path throughput — S sequences x B=1024-window
      batches through the fused conv+LSTM path (reference batch semantics
      incl. the LSTM batch-axis-as-time quirk).
  --mode train (config 5): training step — fused conv/LSTM forward-with-stash,
      BCEWithLogits(pos_weight), BPTT backward, DP gradient all-reduce over
      RCCL, fused Adam (fp32, reference recipe).

value = whole-job windows/s across all ranks. Data is synthetic (no network)
with random-init weights; the reference publishes no quantitative numbers
 so vs_baseline is null.

The driver launches N>1 via torch.distributed.run, one rank per GPU; we read
RANK/LOCAL_RANK/WORLD_SIZE from the env (RCCL over xGMI).

A plain run sets up, warms up, times --steps steps and prints the result
line. --full additionally probes the serialized per-trigger latency
(p50_trigger_latency_ms; null without it). --dump-outputs DIR writes what
the last timed step returned as DIR/<name>.npy (inputs are seeded, so two
builds can be compared output for output).
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


DUMP_BUDGET_BYTES = 64 * 1024 * 1024


def dump_outputs(out_dir, arrays):
    """Write {name: tensor} as out_dir/<name>.npy (float32, or float64 where
    the tensor already is), at most DUMP_BUDGET_BYTES in all: an array over
    its share of the budget is reduced to a fixed, seeded sample of its
    flattened elements (same indices on every run)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        t = torch.as_tensor(t).detach()
        t = t.to("cpu", torch.float64 if t.dtype == torch.float64
                 else torch.float32)
        host[name] = t.contiguous().numpy()
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > DUMP_BUDGET_BYTES:
            share = int(DUMP_BUDGET_BYTES * (a.nbytes / total))
            keep = max(1, share // a.itemsize)
            if keep < a.size:
                rng = np.random.default_rng(20240613)
                idx = np.sort(rng.integers(0, a.size, size=keep))
                a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def run_steps(step_fn, steps, warmup, dist, device, min_warm_s=None,
              extra_quantum=1):
    if min_warm_s is None:
        # TSKD_BENCH_MINWARM=0 disables the extension (rocprof runs: the
        # extra ~3k dispatches overflow the tracer)
        min_warm_s = float(os.environ.get("TSKD_BENCH_MINWARM", "6"))
    # W contract warmup steps, then extend warmup to ~min_warm_s wall time:
    # stabilizes clocks AND makes the run long enough for the driver's
    # rocm-smi busy sampler to see it (r1 timed region was 40 ms —
    # invisible at 1 Hz sampling). The extension count must be AGREED
    # across ranks (steps contain collectives): take the MAX of each
    # rank's estimate, then run exactly that many everywhere.
    w0 = time.perf_counter()
    for _ in range(warmup):
        step_fn()
    _sync()
    elapsed = time.perf_counter() - w0
    per_step = max(elapsed / max(warmup, 1), 1e-4)
    n_extra = max(0, int((min_warm_s - elapsed) / per_step) + 1) \
        if (warmup > 0 and elapsed < min_warm_s) else 0
    if dist:
        red_dev = device if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([n_extra], dtype=torch.int64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        n_extra = int(t.item())
    n_extra = min(n_extra, 100_000)
    # extra_quantum > 1: round the wall-clock-paced count up to a multiple,
    # for step functions whose state is periodic in the step count
    n_extra = -(-n_extra // extra_quantum) * extra_quantum
    for _ in range(n_extra):
        step_fn()
    _sync()
    if dist:
        dist.barrier()
    _sync()
    lat = []
    t0 = time.perf_counter()
    for _ in range(steps):
        s0 = time.perf_counter()
        step_fn()
        _sync()
        lat.append(time.perf_counter() - s0)
    if dist:
        dist.barrier()
    _sync()
    t1 = time.perf_counter()
    red_dev = device if (dist and dist.get_backend() == "nccl") else "cpu"
    elapsed = torch.tensor([t1 - t0], device=red_dev, dtype=torch.float64)
    if dist:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    return float(elapsed.item()), lat


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=15)
    p.add_argument("--mode", default="pipeline",
                   choices=["pipeline", "infer", "train"])
    p.add_argument("--streams", type=int, default=65536,
                   help="[pipeline] concurrent patient streams per GPU")
    p.add_argument("--seqs", type=int, default=8192,
                   help="[infer] concurrent sequences per GPU")
    p.add_argument("--batch", type=int, default=1024,
                   help="[infer] windows per sequence batch")
    p.add_argument("--variant", default="MyCNN5")
    p.add_argument("--overlap", action="store_true",
                   help="[pipeline] two-stream ingest/model software "
                        "pipelining (measured NEUTRAL in r1 at full grids "
                        "and NULL in the r2 CU-partition sweep with capped "
                        "ingest grids — kept as an A/B reference)")
    p.add_argument("--graph", action="store_true", default=True,
                   help="hipGraph-capture the model forward (pipeline mode)")
    p.add_argument("--no-graph", dest="graph", action="store_false")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure: [pipeline] the serialized per-trigger "
                        "latency probe (p50_trigger_latency_ms)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the arrays the last "
                        "timed step returned as DIR/<name>.npy")
    args = p.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        from tskd_amd.parallel.dist import pick_backend
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(pick_backend(world))
    assert torch.cuda.is_available(), "bench.py requires an MI355X"
    # one rank per GPU in production; mod by visible count so world=2 on a
    # 1-GPU box (RCCL-path validation) shares cuda:0
    dev_idx = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_idx)
    device = torch.device("cuda", dev_idx)

    from tskd_amd.models import build_model
    from tskd_amd.ops import MyCNNEngine

    torch.manual_seed(1234 + rank)
    model = build_model(args.variant).eval()
    eng = MyCNNEngine(model, device=device)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    last = {}  # what the most recent step returned to its caller
    min_warm_s = None
    extra_quantum = 1

    if args.mode == "train":
        from tskd_amd.train.hip_trainer import MyCNNHipTrainer
        S, B = max(args.seqs // 8, 1), 64  # reference batch size 64
        tr = MyCNNHipTrainer(model, device=device, lr=1e-5, pos_weight=3.0)
        x = torch.randn(S, B, 10, 120, device=device)
        x[:, :, 8:, :] = 0
        age = torch.full((S, B), 65.0, device=device)
        y = (torch.rand(S, B, device=device) < 0.3).float()

        def step():
            last["loss"] = tr.step(x, age, y)

        if args.dump_outputs:
            # every step updates the weights: keep the step count a function
            # of the arguments alone (no wall-clock-paced warmup extension)
            min_warm_s = 0.0

        windows_per_step = S * B
        cfg = {"model": args.variant, "global_batch": windows_per_step * world,
               "seq_len": 120, "batch_per_seq": B, "seqs_per_gpu": S,
               "parallelism": f"dp{world}", "mode": "train",
               "optimizer": "fused_adam", "loss": "bce_pos_weight"}
        args.dtype = "fp32"  # training runs fp32 like the reference
    elif args.mode == "infer":
        from tskd_amd.ops import alloc_windows
        S, B = args.seqs, args.batch
        if dtype == torch.bfloat16:
            # timelast layout: the serving engine's internal window format
            x = alloc_windows(S, B, 10, timelast=True, dtype=dtype,
                              device=device)
            x.copy_(torch.randn(S, B, 120, 10, device=device, dtype=dtype))
            x[:, :, :, 8:] = 0  # 8 active of 10 wire channels
        else:
            x = torch.randn(S, B, 10, 120, device=device, dtype=dtype)
            x[:, :, 8:, :] = 0
        age = torch.full((S, B), 65.0, device=device)

        def step():
            last["probs"] = eng.forward(x, age, apply_sigmoid=True)

        windows_per_step = S * B
        cfg = {"model": args.variant, "global_batch": windows_per_step * world,
               "seq_len": 120, "batch_per_seq": B, "seqs_per_gpu": S,
               "parallelism": f"dp{world}", "mode": "infer"}
    else:
        from tskd_amd.engine import StreamEngine
        S = args.streams
        fs = 125.0
        se = StreamEngine(S, 10, ring_grid=2048, fs=fs, device=device)
        chan_map = list(range(8))  # 8 active channels
        trigger_samples = int(fs * 60)  # one 60-s trigger per step
        if args.dump_outputs:
            # the rings' position repeats every G / gcd(G, NB) triggers and
            # the window sums are grouped by ring position (last-bit
            # differences): keep the last step's position a function of the
            # arguments alone, whatever the warmup extension comes to
            import math
            nb = trigger_samples // se.bucket_len
            extra_quantum = se.G // math.gcd(se.G, nb)
        # Pre-generate one trigger's worth of raw data (synthetic; in
        # production this arrives from the bus).
        raw = torch.randn(S, 8, trigger_samples, device=device, dtype=dtype)
        age = torch.full((S, 1), 65.0, device=device)
        gathered = [torch.empty(S, device=device) for _ in range(world)] \
            if dist else None
        graphed = None
        tg = None
        if args.graph and dtype == torch.bfloat16:
            # warm the rings to steady state, then capture the WHOLE trigger
            # (ingest -> fill -> gather -> conv -> LSTM -> advance) as ONE
            # hipGraph (BASELINE config 4: fused preprocess+inference graph).
            # Any capture failure falls back to the eager kernel path.
            try:
                from tskd_amd.engine.stream_engine import TriggerGraph
                from tskd_amd.ops import GraphedForward
                graphed = GraphedForward(eng, s=S, n=1, dtype=dtype,
                                         timelast=True, capture=False)
                while se.nproc < se.head - se.win_buckets + 1 or se.nproc == 0:
                    se.ingest_dense(raw, chan_map=chan_map)
                _sync()
                tg = TriggerGraph(se, raw, chan_map, graphed, stride=12,
                                  overlap=args.overlap)
            except Exception as e:  # pragma: no cover - fallback safety
                print(f"[bench] hipGraph capture unavailable ({e}); "
                      "running eager", file=sys.stderr)
                tg = None

        # END-TO-END trigger latency: with the overlapped two-stream graph,
        # per-step wall time is the completion INTERVAL, not the latency of
        # one trigger. Probe the true per-trigger latency (ingest -> model,
        # serialized by a sync after every replay) before the timed loop.
        # (--full only: not part of the headline figure.)
        trigger_latency_ms = None
        if tg is not None and args.full:
            lp = []
            for _ in range(20):
                _sync()
                t0 = time.perf_counter()
                tg.replay()
                _sync()
                lp.append((time.perf_counter() - t0) * 1e3)
            trigger_latency_ms = statistics.median(lp)

        def step():
            if tg is not None:
                probs = tg.replay()
            else:
                se.ingest_dense(raw, chan_map=chan_map)
                w = se.windows(batch=1, stride=12, dtype=dtype)
                probs = eng.forward(w, age, apply_sigmoid=True)
            last["probs"] = probs
            if dist:
                if dist.get_backend() == "nccl":
                    # predictions to every rank (RCCL all-gather over xGMI)
                    dist.all_gather(gathered, probs.reshape(S).contiguous())
                else:
                    # gloo validation topology (ranks sharing one GPU)
                    from tskd_amd.parallel.dist import all_gather_predictions
                    all_gather_predictions(probs.reshape(S))

        windows_per_step = S
        cfg = {"model": args.variant, "global_batch": S * world,
               "seq_len": 120, "streams_per_gpu": S,
               "trigger_s": 60, "fs_hz": 125, "hipgraph": graphed is not None,
               "overlap": tg is not None and tg.overlap,
               "parallelism": f"dp{world}", "mode": "pipeline"}

    if args.mode != "pipeline":
        trigger_latency_ms = None
    elapsed_s, lat = run_steps(step, args.steps, args.warmup, dist, device,
                               min_warm_s=min_warm_s,
                               extra_quantum=extra_quantum)
    total_windows = windows_per_step * args.steps * world
    value = total_windows / elapsed_s
    ms_per_step = elapsed_s / args.steps * 1000.0

    if args.dump_outputs and rank == 0:
        _sync()
        outs = dict(last)
        if args.mode == "train":
            outs["weights"] = tr.wpack  # the updated packed parameters
        dump_outputs(args.dump_outputs, outs)

    if rank == 0:
        print(json.dumps({
            "metric": "waveform_windows_per_sec",
            "value": value,
            "unit": "windows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "p50_step_ms": statistics.median(lat) * 1000.0,
            "p50_trigger_latency_ms": (None if args.mode != "pipeline"
                                       else trigger_latency_ms),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic 8-active-ch 125 Hz waveforms, random-init weights",
            "config": cfg,
        }), flush=True)

    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

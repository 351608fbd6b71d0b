"""Round-2 serving-edge features: native poll_samples_sid (C++ key->sid +
shard filter), wall-clock event-time fast-forward, force_ready, and the
serving-latency harness smoke (CPU).
"""
import json
import subprocess
import sys
import os

import numpy as np
import pytest
import torch

from tskd_amd.bus import Bus, Consumer, Producer
from tskd_amd.engine import StreamEngine
from tskd_amd.parallel.dist import shard_for_key

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bus(tmp_path):
    return Bus(str(tmp_path / "bus"))


class TestPollSamplesSid:
    def test_dense_sid_assignment_and_arrays(self, bus):
        bus.create_topic("HR")
        p = Producer(bus)
        c = Consumer(bus, starting="earliest")
        c.subscribe(["HR"])
        pids = [f"p{i:06d}" for i in range(5)]
        for rep in range(3):
            for pid in pids:
                p.produce("HR", pid, json.dumps([2, 70.0 + rep]),
                          ts_us=1_000_000 * (rep + 1))
        sa, ca, va, ta, nk = c.poll_samples_sid(max_msgs=100)
        assert list(dict(nk).keys()) == pids      # first-seen order
        assert list(dict(nk).values()) == [0, 1, 2, 3, 4]
        assert sa.dtype == np.int32 and len(sa) == 15
        assert (sa[:5] == np.arange(5)).all()
        assert (ca == 2).all() and va.dtype == np.float32
        assert ta.dtype == np.float64 and ta[0] == 1.0
        # second poll: no new keys, ids stable
        p.produce("HR", pids[3], json.dumps([2, 99.0]), ts_us=4_000_000)
        sa2, _, _, _, nk2 = c.poll_samples_sid(max_msgs=100)
        assert nk2 == [] and list(sa2) == [3]

    def test_shard_filter_matches_python_hash(self, bus):
        bus.create_topic("HR")
        p = Producer(bus)
        pids = [f"p{i:06d}" for i in range(64)]
        for pid in pids:
            p.produce("HR", pid, json.dumps([0, 1.0]), ts_us=1)
        world = 4
        seen = set()
        for rank in range(world):
            c = Consumer(bus, starting="earliest")
            c.subscribe(["HR"])
            sa, ca, va, ta, nk = c.poll_samples_sid(max_msgs=1000,
                                                    rank=rank, world=world)
            keys = [k for k, _ in nk]
            assert all(shard_for_key(k, world) == rank for k in keys)
            # dense per-rank ids
            assert [s for _, s in nk] == list(range(len(keys)))
            seen.update(keys)
        assert seen == set(pids)  # partition of the key space

    def test_max_streams_enforced(self, bus):
        bus.create_topic("HR")
        p = Producer(bus)
        for i in range(5):
            p.produce("HR", f"p{i}", json.dumps([0, 1.0]), ts_us=1)
        c = Consumer(bus, starting="earliest")
        c.subscribe(["HR"])
        with pytest.raises(RuntimeError, match="max_streams"):
            c.poll_samples_sid(max_msgs=100, max_streams=3)


class TestWallClockEventTime:
    def test_fresh_engine_fast_forwards(self):
        se = StreamEngine(4, 3, ring_grid=256, device="cpu")
        now = 1_787_000_000.0  # epoch seconds
        n = 16
        se.ingest_events(torch.zeros(n, dtype=torch.long),
                         torch.zeros(n, dtype=torch.long),
                         torch.tensor([now + 5 * i for i in range(n)],
                                      dtype=torch.float64),
                         torch.arange(n, dtype=torch.float32) + 1,
                         advance_to=now + 5 * n)
        # origin skipped ahead: nproc near the wall-clock bucket, bounded
        # catch-up (no multi-hundred-million-point refill)
        assert se._origin_nproc > 0
        # nproc may lag the first-event bucket by up to win-1 (sliding
        # window not yet complete) but never leads it by more than the ring
        assert -se.win_buckets <= se.nproc - se._origin_nproc <= se.G
        assert not se.ready  # < 780 s of data since the stream began
        se.force_ready()
        assert se.ready
        w = se.windows(batch=1, stride=12)
        assert w.shape == (4, 1, 3, 120)
        assert torch.isfinite(w).all()

    def test_ready_stays_origin_relative(self):
        se = StreamEngine(2, 2, ring_grid=512, device="cpu")
        now = 1_787_000_000.0
        # feed 800 s of data in 40 s chunks -> ready flips when >= 780 s
        # (600 s model window + 180 s sliding window) has accumulated
        became_ready_at = None
        for step in range(21):
            t0 = now + 40.0 * step
            ts = torch.tensor([t0 + 5 * i for i in range(8)],
                              dtype=torch.float64)
            se.ingest_events(torch.zeros(8, dtype=torch.long),
                             torch.zeros(8, dtype=torch.long),
                             ts, torch.ones(8), advance_to=t0 + 40.0)
            if se.ready and became_ready_at is None:
                became_ready_at = 40.0 * (step + 1)
        assert became_ready_at is not None
        assert 760.0 <= became_ready_at <= 840.0

    def test_zero_based_times_unaffected(self):
        se = StreamEngine(2, 2, ring_grid=256, device="cpu")
        raw = torch.randn(2, 2, 625 * 5)  # 5 buckets at fs=125, 5-s buckets
        for _ in range(40):
            se.ingest_dense(raw)
        assert se._origin_nproc == 0
        assert se.ready  # 200 buckets > 120 + 36


class TestServingLatencyHarness:
    def test_quick_cpu_run(self):
        r = subprocess.run(
            [sys.executable, os.path.join(REPO, "scripts",
                                          "serving_latency.py"),
             "--device", "cpu", "--quick"],
            capture_output=True, text=True, timeout=300, cwd=REPO)
        assert r.returncode == 0, r.stderr
        recs = [json.loads(ln) for ln in r.stdout.splitlines()
                if ln.startswith("{")]
        assert {x["scenario"] for x in recs} == {"drain", "live"}
        drain = next(x for x in recs if x["scenario"] == "drain")
        assert drain["events_drained"] == drain["n_events"]
        live = next(x for x in recs if x["scenario"] == "live")
        assert live["n_predictions"] > 0
        assert live["wire_to_store_ms"]["p50"] is not None


@pytest.mark.gpu
class TestServingLatencyGpu:
    def test_wire_to_store_quick(self):
        """Full bus->parse->H2D->ring->model->store path on the GPU: the
        quick live scenario must score predictions with single-digit-to-
        low-double-digit-ms wire->store latency (measured p50 ~8 ms at 20k
        events/s in profiles/r02_serving_capacity.md)."""
        r = subprocess.run(
            [sys.executable, os.path.join(REPO, "scripts",
                                          "serving_latency.py"),
             "--device", "cuda", "--quick"],
            capture_output=True, text=True, timeout=420, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        recs = [json.loads(ln) for ln in r.stdout.splitlines()
                if ln.startswith("{")]
        live = next(x for x in recs if x["scenario"] == "live")
        assert live["n_predictions"] > 0
        assert live["wire_to_store_ms"]["p50"] < 200.0
        drain = next(x for x in recs if x["scenario"] == "drain")
        assert drain["events_drained"] == drain["n_events"]
        assert drain["n_predictions"] > 0


def _bench_warmup_worker(rank, world, port, out_dir):
    import time

    import torch.distributed as dist
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                       "RANK": str(rank), "WORLD_SIZE": str(world)})
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    from bench import run_steps
    calls = [0]

    def step():
        calls[0] += 1
        # a collective per step + rank-dependent speed: if the warmup
        # extension were wall-clock-paced per rank (the r2 deadlock bug),
        # ranks would issue different collective counts and hang here
        t = torch.ones(1)
        dist.all_reduce(t)
        time.sleep(0.001 * (1 + 4 * rank))

    elapsed, lat = run_steps(step, steps=3, warmup=2, dist=dist,
                             device="cpu", min_warm_s=0.2)
    with open(os.path.join(out_dir, f"warm{rank}.txt"), "w") as f:
        f.write(f"{calls[0]} {elapsed:.4f} {len(lat)}")
    dist.barrier()
    dist.destroy_process_group()


class TestBenchWarmupAgreement:
    def test_ranks_agree_on_extension_count(self, tmp_path):
        """Regression: the SMI-visibility warmup extension must run the
        SAME number of steps on every rank (steps contain collectives)."""
        import socket
        import torch.multiprocessing as mp
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        ctx = mp.get_context("spawn")
        ps = [ctx.Process(target=_bench_warmup_worker,
                          args=(r, 2, port, str(tmp_path)))
              for r in range(2)]
        for p in ps:
            p.start()
        for p in ps:
            p.join(120)
            assert p.exitcode == 0, p.exitcode
        c0, e0, l0 = open(tmp_path / "warm0.txt").read().split()
        c1, e1, l1 = open(tmp_path / "warm1.txt").read().split()
        assert c0 == c1          # identical collective counts
        assert l0 == l1 == "3"   # timed steps as contracted
        assert int(c0) > 5       # warmup actually extended past W=2


class TestBenchDump:
    def _bench(self):
        sys.path.insert(0, REPO)
        import bench
        return bench

    def test_dump_outputs_float32_npy(self, tmp_path):
        import numpy as np
        bench = self._bench()
        out = str(tmp_path / "dump")
        bench.dump_outputs(out, {
            "probs": torch.arange(6, dtype=torch.bfloat16).reshape(3, 2),
            "loss": 0.25})
        probs = np.load(os.path.join(out, "probs.npy"))
        assert probs.dtype == np.float32 and probs.shape == (3, 2)
        np.testing.assert_array_equal(probs.ravel(), np.arange(6))
        assert np.load(os.path.join(out, "loss.npy")).dtype == np.float32

    def test_dump_outputs_budget_sample_is_fixed(self, tmp_path, monkeypatch):
        import numpy as np
        bench = self._bench()
        monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
        big = torch.arange(10_000, dtype=torch.float32)
        small = torch.ones(24)
        for d in ("a", "b"):
            bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
        a = np.load(tmp_path / "a" / "big.npy")
        b = np.load(tmp_path / "b" / "big.npy")
        s = np.load(tmp_path / "a" / "small.npy")
        assert a.nbytes + s.nbytes <= 4096 and 0 < a.size < 10_000
        np.testing.assert_array_equal(a, b)      # same indices every run
        assert (np.diff(a) >= 0).all()           # a sample of the original

    def test_warmup_extension_quantum(self):
        bench = self._bench()
        calls = [0]

        def step():
            calls[0] += 1

        _, lat = bench.run_steps(step, steps=3, warmup=2, dist=None,
                                 device="cpu", min_warm_s=0.01,
                                 extra_quantum=512)
        assert len(lat) == 3
        extra = calls[0] - 3 - 2
        assert extra > 0 and extra % 512 == 0


class TestSignalSurvey:
    def test_survey_committed_record(self, capsys):
        """Signal-availability survey (explore_fantasia analog) over the
        committed real p000194 numerics record."""
        from tskd_amd.cli.surveysignals import main
        main(["--wavef-path", os.path.join(REPO, "data", "waveform"),
              "--json"])
        rec = json.loads(capsys.readouterr().out)
        assert rec["n_records"] == 1
        assert rec["channel_counts"]["HR"] == 1
        r = rec["records"]["p000194-2112-05-23-14-34n"]
        assert r["sig_len"] == 1625
        assert abs(r["fs_hz"] - 1 / 60) < 1e-6
        # the reference's channel-name mismatch shows up here: record says
        # NBPSys, config says "NBP Sys"
        assert "NBPSys" in r["channels"] and r["channels"]["HR"] > 0


class TestPollThread:
    def test_background_poll_scores_identically(self, tmp_path):
        """serve with the background poll thread must produce the same
        predictions as inline polling over the same bus contents."""
        import time

        from tskd_amd.cli.serve import FusedServer
        from tskd_amd.config import get_global_config
        from tskd_amd.store import PredictionStore
        cfg = get_global_config()
        results = {}
        for mode in ("inline", "thread"):
            bus = Bus(str(tmp_path / f"bus_{mode}"))
            store = PredictionStore(str(tmp_path / f"pred_{mode}.log"))
            topics = [cfg.topic_for_channel(c)
                      for c in cfg.channel_names[:4]]
            for t in topics:
                bus.create_topic(t)
            prod = Producer(bus)
            for step in range(200):
                for pi in range(6):
                    for ch in range(4):
                        prod.produce(topics[ch], f"p{pi:06d}",
                                     json.dumps([ch, 50.0 + step % 9]),
                                     ts_us=int(step * 5e6))
            torch.manual_seed(7)  # identical random-init model weights
            srv = FusedServer(bus, cfg, store, device="cpu",
                              max_streams=8, starting="earliest")
            srv.watermark_s = 0.0
            if mode == "thread":
                srv.start_poll_thread(interval_s=0.005)
                time.sleep(0.5)  # drain the whole backlog before triggering
                # (the watermark advances at consume time, so chunks that
                # arrive after a trigger advanced past their event time are
                # dropped — correct event-time semantics, but the
                # equivalence check wants identical ring contents)
            srv.se.force_ready()
            n = 0
            for _ in range(6):
                n += srv.trigger()
                time.sleep(0.05)
            srv.stop_poll_thread()
            results[mode] = {
                "n": n, "pids": sorted(srv.pid_index),
                "preds": sorted((p, round(r, 6))
                                for p, _t, r in store.tail(100)),
            }
        assert results["inline"]["pids"] == results["thread"]["pids"]
        assert results["inline"]["n"] > 0
        assert results["inline"]["preds"] == results["thread"]["preds"]


class TestServeCliMain:
    def test_main_poll_thread_flow(self, tmp_path, monkeypatch):
        """serve.main() end-to-end through the CLI arg path: tmp bus with a
        replayed backlog, --poll-thread, --max-triggers, prediction store
        written, clean shutdown (poll thread joined, deferred flush)."""
        import time

        from tskd_amd.cli import serve
        from tskd_amd.config import get_global_config
        from tskd_amd.store import PredictionStore
        cfg = get_global_config()
        bus = Bus(str(tmp_path / "bus"))
        topics = [cfg.topic_for_channel(c) for c in cfg.channel_names[:4]]
        for t in topics:
            bus.create_topic(t)
        prod = Producer(bus)
        for step in range(200):
            for pi in range(4):
                for ch in range(4):
                    prod.produce(topics[ch], f"p{pi:06d}",
                                 json.dumps([ch, 60.0 + step % 7]),
                                 ts_us=int(step * 5e6))
        store_path = str(tmp_path / "pred.log")
        serve.main(["--bus-dir", str(tmp_path / "bus"),
                    "--store-path", store_path,
                    "--model-path", str(tmp_path / "nonexistent.pth"),
                    "--device", "cpu", "--max-streams", "8",
                    "--starting", "earliest", "--poll-thread",
                    "--pipelined", "--speed", "1e6",
                    "--max-triggers", "30"])
        store = PredictionStore(store_path)
        assert store.count() > 0
        pids = {r[0] for r in store.tail(100)}
        assert pids == {f"p{i:06d}" for i in range(4)}

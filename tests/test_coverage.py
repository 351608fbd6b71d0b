"""Window coverage (StreamEngine.coverage) and the serving gate built on it
(serve --min-coverage). CPU tests: bucket counts written by hand into the
ring against a brute force written from the definitions, a restored engine's
floor, the refusals, the id-list cases, an event-path run, and two patients
through FusedServer of whom one falls silent.

The case builders are shared with tests/test_coverage_gpu.py.
"""
import json

import numpy as np
import pytest
import torch

from tskd_amd.bus import Bus, Consumer, Producer
from tskd_amd.engine import StreamEngine
from tskd_amd.metrics import StageTimer, prometheus_text

L = 120                      # model window, grid points
G = 192                      # ring shorter than 2 spans: the span wraps
RUNS = (0, 1, 35, 36, 37, 63, 64, 65)   # trailing empty runs, + span-1, span


# ---------------------------------------------------------------- the oracle
def brute(is_present, n, C, nproc, W, model_win=L):
    """(n, C, 3) [present, imputed, stale] from the definitions, bucket by
    bucket: ``is_present(s, c, b)`` for absolute bucket ``b``."""
    lo, hi = nproc - model_win, nproc + W - 1
    out = np.zeros((n, C, 3), dtype=np.int32)
    for s in range(n):
        for c in range(C):
            p = [is_present(s, c, b) for b in range(lo, hi)]
            out[s, c, 0] = sum(p)
            out[s, c, 1] = sum(not any(p[g:g + W]) for g in range(model_win))
            stale = 0
            while stale < len(p) and not p[len(p) - 1 - stale]:
                stale += 1
            out[s, c, 2] = stale
    return out


def brute_ring(bcnt, nproc, W, floor=0):
    """The brute force over ring contents ``bcnt`` (n, C, G)."""
    n, C, g = bcnt.shape
    return brute(lambda s, c, b: b < floor or bcnt[s, c, b % g] > 0,
                 n, C, nproc, W)


# ------------------------------------------------------------- count patterns
def patterns(span):
    """[(name, counts of the span's buckets, override of the buckets just
    outside it or None)]. Without an override the ring slots outside the
    span hold the OPPOSITE state of the span's nearest end (sentinels: a read
    one bucket too far on either side changes a result)."""
    def row(sel=slice(0, 0), val=1.0, base=0.0):
        a = np.full(span, base, dtype=np.float32)
        a[sel] = val
        return a

    out = [("empty", row(), None), ("full", row(base=1.0), None),
           ("single_lo", row(0), None), ("single_hi-1", row(-1), None),
           # a present bucket just outside an empty span must not count
           ("outside_lo-1", row(), "lo-1"), ("outside_hi", row(), "hi"),
           ("alternating", row(slice(0, None, 2)), None),
           ("alternating_odd", row(slice(1, None, 2)), None),
           ("every37", row(slice(0, None, 37)), None)]
    for run in RUNS + (span - 1, span):
        out.append((f"tail{run}", row(slice(span - run, None), 0.0, 1.0),
                    None))
    out.append(("half_counts", row(base=0.5), None))
    a = row(slice(0, None, 3), 625.0)
    a[1::3] = 0.5
    out.append(("large_and_fractional", a, None))
    rng = np.random.default_rng(span)
    out.append(("random10", (rng.random(span) < 0.1).astype(np.float32),
                None))
    return out


N_PATTERNS = len(patterns(155))


def ring_counts(S, C, g, nproc, W):
    """(S, C, g) float32 bucket counts: row r holds pattern r % N_PATTERNS in
    the span [nproc - L, nproc + W - 1), sentinels in every other slot."""
    span, lo = L + W - 1, nproc - L
    pats = patterns(span)
    ring = np.zeros((S, C, g), dtype=np.float32)
    n_out = g - span
    for r in range(S * C):
        _name, inside, outside = pats[r % len(pats)]
        row = ring[r // C, r % C]
        row[(lo + np.arange(span)) % g] = inside
        # outside slots in grid order from hi on; the last one is lo - 1 + g
        out = np.zeros(n_out, dtype=np.float32)
        if outside is None:
            out[:(n_out + 1) // 2] = 0.0 if inside[-1] > 0 else 625.0
            out[(n_out + 1) // 2:] = 0.0 if inside[0] > 0 else 625.0
        elif outside == "hi":
            out[0] = 1.0
        else:
            out[-1] = 1.0
        row[(lo + span + np.arange(n_out)) % g] = out
    return ring


def hand_engine(device, S, C, nproc, W, g=G):
    """An engine whose ring positions and bucket counts are set by hand."""
    e = StreamEngine(S, C, ring_grid=g, win_buckets=W, device=device)
    counts = ring_counts(S, C, g, nproc, W)
    e.bcnt.copy_(torch.from_numpy(counts))
    e.nproc = nproc
    e.head = e._cleared = nproc + W - 1
    return e, counts


def cov(e, sids=None):
    out = e.coverage(sids)
    assert out.dtype == torch.int32 and out.device.type == e.device.type
    return out.cpu().numpy()


# -------------------------------------------------------------- event path
def dropout_events(S=3, C=3, n_buckets=240):
    """One sample per 5 s on every (stream, channel), ~30 % dropped, some
    NaN, with per-channel dropouts: (0, 1) falls silent at bucket 100,
    (1, 2) never arrives, (2, 0) has a gap over buckets [120, 170)."""
    rng = np.random.default_rng(5)
    si, ci, ts, vv = [], [], [], []
    for s in range(S):
        for c in range(C):
            if (s, c) == (1, 2):
                continue
            b = np.arange(n_buckets)
            keep = rng.random(n_buckets) >= 0.3
            if (s, c) == (0, 1):
                keep &= b < 100
            if (s, c) == (2, 0):
                keep &= (b < 120) | (b >= 170)
            v = rng.integers(1, 200, n_buckets).astype(np.float32)
            v[rng.random(n_buckets) < 0.05] = np.nan
            si.append(np.full(keep.sum(), s))
            ci.append(np.full(keep.sum(), c))
            ts.append(b[keep] * 5.0 + 1.0)
            vv.append(v[keep])
    return tuple(np.concatenate(x) for x in (si, ci, ts, vv))


def run_events(device, g=G, until=240):
    """Feed dropout_events in 60-s triggers; returns the engine."""
    e = StreamEngine(3, 3, ring_grid=g, device=device)
    si, ci, ts, vv = dropout_events()
    for t in np.arange(0.0, until * 5.0, 60.0):
        m = (ts >= t) & (ts < t + 60.0)
        e.ingest_events(torch.from_numpy(si[m]).long(),
                        torch.from_numpy(ci[m]).long(),
                        torch.from_numpy(ts[m]), torch.from_numpy(vv[m]),
                        advance_to=t + 60.0)
    return e


def restored_engine(device, S, C, g=G):
    """A fresh engine restored from a CPU engine's snapshot taken at grid
    point 133 (events of dropout_events up to bucket 168)."""
    src = run_events("cpu", until=168)
    assert src.nproc == 133
    snap = src.snapshot()
    e = StreamEngine(S, C, ring_grid=g, device=device)
    e.restore(snap)
    return e, snap


# ===================================================================== tests
class TestCoverageCounts:
    @pytest.mark.parametrize("W", [36, 1, 64])
    @pytest.mark.parametrize("nproc", [120, 158, 311])
    def test_hand_written_counts_match_the_brute_force(self, nproc, W):
        S, C = -(-N_PATTERNS // 3), 3
        e, counts = hand_engine("cpu", S, C, nproc, W)
        want = brute_ring(counts, nproc, W)
        assert np.array_equal(cov(e), want)
        assert np.array_equal(e.bcnt.numpy(), counts)   # reads only

    def test_the_cases_are_not_vacuous(self):
        W, span = 36, L + 36 - 1
        S, C = -(-N_PATTERNS // 3), 3
        _e, counts = hand_engine("cpu", S, C, 158, W)
        want = brute_ring(counts, 158, W).reshape(-1, 3)[:N_PATTERNS]
        imputed, stale = set(want[:, 1]), set(want[:, 2])
        assert 0 in imputed and L in imputed
        assert any(0 < v < L for v in imputed)
        assert set(RUNS + (span - 1, span)) <= stale
        names = [p[0] for p in patterns(span)]
        by = dict(zip(names, want.tolist()))
        assert by["empty"] == [0, L, span] and by["full"] == [span, 0, 0]
        assert by["outside_lo-1"] == by["outside_hi"] == [0, L, span]
        assert by["single_lo"] == [1, L - 1, span - 1]
        assert by["single_hi-1"] == [1, L - 1, 0]
        assert by["half_counts"] == [span, 0, 0]
        assert by["tail37"] == [span - 37, 2, 37]

    def test_sid_lists(self):
        e, counts = hand_engine("cpu", 4, 3, 200, 36)
        want = brute_ring(counts, 200, 36)
        full = cov(e)
        assert full.shape == (4, 3, 3) and np.array_equal(full, want)
        assert np.array_equal(cov(e, [2, 0, 2]), want[[2, 0, 2]])
        assert np.array_equal(cov(e, torch.tensor([3])), want[[3]])
        empty = e.coverage([])
        assert empty.shape == (0, 3, 3) and empty.dtype == torch.int32
        for bad in ([4], [-1], [0, 4]):
            with pytest.raises(ValueError):
                e.coverage(bad)

    def test_refusals(self):
        e = StreamEngine(2, 3, ring_grid=G)
        with pytest.raises(ValueError, match="no full model window"):
            e.coverage()
        e, _ = hand_engine("cpu", 2, 3, L - 1, 36)
        with pytest.raises(ValueError, match="no full model window"):
            e.coverage()
        # the ring was cleared ahead past the slots the span's first buckets
        # occupy: lo = 80, and bucket 80 + G is already written
        e, _ = hand_engine("cpu", 2, 3, 200, 36)
        e._cleared = 80 + G
        e.coverage()
        e._cleared = 80 + G + 1
        with pytest.raises(ValueError, match="no longer wholly in the ring"):
            e.coverage()
        # the same through the event path: one sample far ahead of the
        # watermark clears the slots of the window's oldest buckets
        e = run_events("cpu")
        e.coverage()
        far = (e.nproc + G - e.win_buckets - 1) * 5.0
        e.ingest_events(torch.tensor([0]), torch.tensor([0]),
                        torch.tensor([far], dtype=torch.float64),
                        torch.tensor([1.0]), advance_to=e.head * 5.0)
        with pytest.raises(ValueError, match="no longer wholly in the ring"):
            e.coverage()

    def test_not_inside_a_device_state_block(self):
        e, _ = hand_engine("cpu", 1, 3, 200, 36)
        with e.device_state(torch.zeros(2, dtype=torch.int64)):
            with pytest.raises(AssertionError):
                e.coverage()


class TestRestoredFloor:
    def test_fresh_engine_has_no_floor(self):
        assert StreamEngine(1, 3)._bucket_floor == 0

    def test_buckets_below_the_snapshot_count_as_present(self):
        e, snap = restored_engine("cpu", 3, 3)
        assert e._bucket_floor == snap.nproc == 133
        # right after the restore every grid point's window reaches below
        # the floor: nothing is imputed, nobody is withheld
        got = cov(e)
        assert (got[:, :, 1] == 0).all() and (got[:, :, 0] >= L).all()
        want = brute_ring(e.bcnt.numpy(), e.nproc, 36, floor=133)
        assert np.array_equal(got, want)
        assert got[1, 2].tolist() == [L, 0, 35]   # the channel never arrived

    @pytest.mark.parametrize("nproc", [170, 252, 253, 290])
    def test_floor_inside_the_span(self, nproc):
        """Hand-written counts on a restored engine: lo = nproc - 120 lies
        below the floor 133 up to nproc 252; from 253 on it has no effect."""
        e, _snap = restored_engine("cpu", -(-N_PATTERNS // 3), 3)
        counts = ring_counts(e.S, 3, G, nproc, 36)
        e.bcnt.copy_(torch.from_numpy(counts))
        e.nproc = nproc
        e.head = e._cleared = nproc + 35
        want = brute_ring(counts, nproc, 36, floor=133)
        assert np.array_equal(cov(e), want)
        plain = brute_ring(counts, nproc, 36)
        assert np.array_equal(want, plain) == (nproc >= 253)


class TestEventPath:
    def test_dropouts_against_the_event_list(self):
        e = run_events("cpu")
        assert e.head == 240 and e.nproc == 205 and e.head > G
        si, ci, ts, vv = dropout_events()
        ok = ~np.isnan(vv)
        have = set(zip(si[ok].tolist(), ci[ok].tolist(),
                       (ts[ok] // 5.0).astype(int).tolist()))
        want = brute(lambda s, c, b: (s, c, b) in have, 3, 3, e.nproc, 36)
        got = cov(e)
        assert np.array_equal(got, want)
        # (0, 1) silent since bucket 100 of span [85, 240); (1, 2) never came
        assert got[0, 1, 2] >= 140 and got[0, 1, 1] >= 205 - 100
        assert got[1, 2].tolist() == [0, L, 155]
        assert got[2, 0, 1] >= 50 - 35 and got[2, 0, 2] < 36


# ------------------------------------------------------------------- serving
N_TRIGGERS = 28
SILENT_FROM_S = 16 * 60      # the second patient's last sample: 955 s
PIDS = ("p000501", "p000502")


def run_gate(tmp_path, tag, device="cpu", pipelined=False, **kw):
    """Two patients stream one sample per 5 s on every named channel; the
    second falls silent after 16 minutes. One trigger per stream-minute.
    Returns (server, [(trigger, nproc, store rows, response payloads)])."""
    from tskd_amd.cli.serve import FusedServer
    from tskd_amd.config import get_global_config
    from tskd_amd.store import PredictionStore
    cfg = get_global_config()
    bus = Bus(str(tmp_path / f"bus_{tag}"))
    store = PredictionStore(str(tmp_path / f"pred_{tag}.log"))
    topics = [cfg.topic_for_channel(c) for c in cfg.channel_names]
    for t in topics:
        bus.create_topic(t)
    prod = Producer(bus)
    torch.manual_seed(7)     # identical random-init model weights
    srv = FusedServer(bus, cfg, store, device=device, max_streams=4,
                      ring_grid=256, starting="earliest",
                      response_topic="risk", pipelined=pipelined, **kw)
    reader = Consumer(bus, starting="earliest")
    reader.subscribe(["risk"])
    log = []
    for m in range(N_TRIGGERS):
        for step in range(12):
            t = m * 60 + step * 5
            for i, pid in enumerate(PIDS):
                if i == 1 and t >= SILENT_FROM_S:
                    continue
                for ch in range(cfg.n_channels):
                    prod.produce(topics[ch], pid, json.dumps(
                        [ch, float(60 + 5 * i + ch + (t // 5) % 7)]),
                        ts_us=int(t * 1e6))
        before = store.count()
        srv.trigger()
        if pipelined:
            srv.flush()
        rows = store.tail(store.count() - before) \
            if store.count() > before else []
        msgs = reader.poll(max_msgs=64, timeout_ms=0)
        log.append((m + 1, srv.se.nproc,
                    [(p, t.timestamp(), r) for p, t, r in rows],
                    [(x.key.decode(), x.value) for x in msgs]))
    return srv, log


def expected_q(m):
    """The silent patient's coverage at trigger m (ending at 60 m seconds):
    the watermark trails the newest sample (60 m - 5) by 10 s, so head =
    12 m - 3 and nproc = 12 m - 38; its last sample sits in bucket 191, so
    the grid points from 192 on are imputed on every channel."""
    return 1.0 - min(max(12 * m - 38 - 192, 0), L) / L


def check_gate(srv, log, F):
    """The gate's properties on a run_gate log (shared with the GPU run)."""
    withheld = 0
    seen_both = False
    for m, nproc, rows, msgs in log:
        assert nproc == max(0, 12 * m - 38)
        pids = sorted(p for p, _t, _r in rows)
        assert pids == sorted(k for k, _v in msgs)
        if nproc < L:
            assert pids == []
            continue
        q = expected_q(m)
        if q < F:
            assert pids == [PIDS[0]], (m, pids)
            withheld += 1
        else:
            assert pids == list(PIDS), (m, pids)
            seen_both = True
        for key, value in msgs:
            doc = json.loads(value)
            assert sorted(doc) == ["coverage", "risk", "t_us"]
            want = 1.0 if key == PIDS[0] else q
            assert doc["coverage"] == round(want, 4), (m, key)
    assert seen_both and withheld >= 3
    assert srv.timer.gauges["withheld_total"] == withheld
    last_q = expected_q(log[-1][0])
    assert srv.timer.gauges["coverage_mean"] == pytest.approx(
        (1.0 + last_q) / 2, abs=1e-12)
    assert "coverage_unavailable" not in srv.timer.gauges
    return withheld


@pytest.fixture(scope="module")
def gated(tmp_path_factory):
    return run_gate(tmp_path_factory.mktemp("gate"), "on", min_coverage=0.5)


class TestServingGate:
    def test_silent_patient_is_withheld_below_the_bound(self, gated):
        srv, log = gated
        # q passes 0.5 between triggers 24 (0.5167) and 25 (0.4167)
        assert expected_q(24) > 0.5 > expected_q(25)
        assert check_gate(srv, log, 0.5) == N_TRIGGERS - 24

    def test_gauges_reach_prometheus(self, gated):
        srv, _log = gated
        text = prometheus_text([srv.timer])
        assert 'tskd_streams{stage="serve",state="withheld_total"} 4' in text
        assert 'state="coverage_mean"' in text
        # and the ten-trigger JSON log line (plain Python numbers)
        streams = json.loads(srv.timer.log_line())["streams"]
        assert streams["withheld_total"] == 4
        assert type(srv.timer.gauges["withheld_total"]) is int
        assert type(srv.timer.gauges["coverage_mean"]) is float

    def test_default_is_byte_identical_to_no_argument(self, tmp_path):
        _a, plain = run_gate(tmp_path, "plain")
        b, off = run_gate(tmp_path, "off", min_coverage=0.0)
        assert plain == off
        assert any(len(rows) == 2 for _m, _n, rows, _msgs in plain[-3:])
        assert all(b"coverage" not in v
                   for _m, _n, _r, msgs in off for _k, v in msgs)
        for g in ("withheld_total", "coverage_mean", "coverage_unavailable"):
            assert g not in b.timer.gauges

    def test_gate_changes_only_who_is_persisted(self, gated, tmp_path):
        _srv, log = gated
        _a, plain = run_gate(tmp_path, "plain2")
        for (m, nproc, rows, _msgs), (_m, pnproc, prows, _pm) in zip(log,
                                                                     plain):
            assert nproc == pnproc
            kept = {p for p, _t, _r in rows}
            assert [x for x in prows if x[0] in kept] == rows

    def test_pipelined_withholds_the_same(self, gated, tmp_path):
        _srv, log = gated
        psrv, plog = run_gate(tmp_path, "pipe", pipelined=True,
                              min_coverage=0.5)
        assert [(m, sorted(p for p, _t, _r in rows))
                for m, _n, rows, _msgs in plog] == \
               [(m, sorted(p for p, _t, _r in rows))
                for m, _n, rows, _msgs in log]
        assert psrv.timer.gauges["withheld_total"] == N_TRIGGERS - 24

    def test_with_the_lifecycle_mask(self, tmp_path):
        srv, log = run_gate(tmp_path, "life", min_coverage=0.5,
                            evict_idle_s=3600.0)
        assert check_gate(srv, log, 0.5) == N_TRIGGERS - 24

    def test_span_out_of_the_ring_withholds_nothing(self, tmp_path, caplog):
        srv, _log = run_gate(tmp_path, "skip", min_coverage=0.5)
        n0 = srv.store.count()
        srv.se._cleared = srv.se.nproc - L + srv.se.G + 13   # as if cleared
        topic = srv.cfg.topic_for_channel(srv.cfg.channel_names[0])
        Producer(Bus(str(tmp_path / "bus_skip"))).produce(
            topic, PIDS[0], json.dumps([0, 1.0]),
            ts_us=int((N_TRIGGERS * 60 + 55) * 1e6))
        with caplog.at_level("WARNING", logger="serve"):
            srv.trigger()
        assert srv.timer.gauges["coverage_unavailable"] == 1
        assert srv.store.count() == n0 + 2       # both persisted
        assert sum("coverage unavailable" in r.message
                   for r in caplog.records) == 1

    def test_bounds_are_checked(self, tmp_path):
        from tskd_amd.cli import serve
        for bad in (-0.1, 1.5):
            with pytest.raises(ValueError):
                run_gate(tmp_path, f"bad{bad}", min_coverage=bad)
            with pytest.raises(SystemExit):
                serve.main(["--min-coverage", str(bad)])


def test_coverage_gauges_render_as_stream_states():
    t = StageTimer("serve", gauges={"coverage_mean": 0.75})
    assert 'state="coverage_mean"} 0.75' in prometheus_text([t])

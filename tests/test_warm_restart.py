"""Warm restart: the engine snapshot (live ring tail) and restore, the
snapshot file, the consumer's slot table hand-over, and FusedServer resuming
from its state file after being dropped mid-run. CPU tests; the scenario
helpers are shared with tests/test_warm_restart_gpu.py.

Shapes follow tests/test_stream_lifecycle.py: C=3, G=128, 60-s triggers of
integer samples, so after trigger k head = 12k and nproc = 12k - 35, bucket
sums are exact and restored state compares with torch.equal.
"""
import dataclasses
import json
import os
import struct

import numpy as np
import pytest
import torch

from tskd_amd.bus import Bus, Consumer, Producer
from tskd_amd.engine import EngineSnapshot, SnapshotError, StreamEngine

from test_stream_lifecycle import _send, feed, patient_events, same

S, C, G = 5, 3, 128
END = 29                 # triggers of the uninterrupted run (nproc 313)
RESEAT = 12              # after this trigger slot 1 is wiped and re-admitted
# snapshot points: short tail (nproc 25 < 120); the processed tail wraps
# (nproc 169, slot 1 still gated); the bucket range wraps too (nproc 241 =
# 113 mod 128, slot 1 open)
POINTS = (5, 17, 23)


def _events():
    ev = [patient_events(20 + s, s, 0, 12 * END) for s in (0, 2, 3, 4)]
    ev.append(patient_events(60, 1, 0, 12 * RESEAT))
    ev.append(patient_events(61, 1, 12 * RESEAT, 12 * END))
    return ev


def drive(eng, start, stop, events, after=None):
    """Triggers start+1 .. stop of the scenario on ``eng``; slot 1 changes
    hands after trigger RESEAT. ``after(i)`` runs after trigger i."""
    for i, _ in enumerate(feed(eng, events, start * 60.0, stop * 60.0),
                          start + 1):
        if i == RESEAT:
            eng.reset_streams([1])
            eng.admit([1])
        if after is not None:
            after(i)


def observe(eng):
    snap = eng.snapshot()
    return {"head": eng.head, "nproc": eng.nproc, "nbk": snap.nbk,
            "keep": snap.keep, "payload": snap.payload.copy(),
            "win": eng.windows(batch=1, stride=12).cpu().clone(),
            "ready": eng.stream_ready().copy()}


def reference_run(device):
    """The uninterrupted engine: what it shows after every trigger, and its
    snapshots at POINTS (payload copied out of the reused buffer)."""
    events = _events()
    eng = StreamEngine(S, C, ring_grid=G, device=device)
    seen, snaps = {}, {}

    def after(i):
        seen[i] = observe(eng)
        if i in POINTS:
            snap = eng.snapshot()
            snap.payload = snap.payload.copy()
            snaps[i] = snap

    drive(eng, 0, END, events, after)
    assert eng.head == 12 * END and eng.nproc == 12 * END - 35
    return events, seen, snaps


def check_resumed(ref, k, device, ring_grid=G):
    """A fresh engine restored from the snapshot at trigger k shows exactly
    what the uninterrupted one shows after every later trigger."""
    events, seen, snaps = ref
    snap = snaps[k]
    assert snap.nproc == 12 * k - 35 and snap.nbk == 35
    assert snap.keep == min(120, snap.nproc)
    eng = StreamEngine(S, C, ring_grid=ring_grid, device=device)
    eng.restore(snap)
    assert eng._proc_floor == snap.nproc - snap.keep
    n = [0]

    def after(i):
        got, want = observe(eng), seen[i]
        for key in ("head", "nproc", "nbk", "keep"):
            assert got[key] == want[key], (key, i)
        assert same(torch.from_numpy(got["payload"]),
                    torch.from_numpy(want["payload"])), i
        assert torch.equal(got["win"], want["win"]), i
        assert (got["ready"] == want["ready"]).all(), i
        n[0] += 1

    drive(eng, k, END, events, after)
    assert n[0] == END - k
    return eng


@pytest.fixture(scope="module")
def ref_cpu():
    return reference_run("cpu")


class TestEngineEquivalence:
    @pytest.mark.parametrize("k", POINTS)
    def test_restored_engine_continues_like_uninterrupted(self, ref_cpu, k):
        check_resumed(ref_cpu, k, "cpu")

    def test_restore_into_a_longer_ring(self, ref_cpu):
        check_resumed(ref_cpu, 23, "cpu", ring_grid=256)

    def test_gate_and_record_length(self, ref_cpu):
        _ev, seen, snaps = ref_cpu
        # slot 1 is gated at the second snapshot point, open at the third
        assert not seen[17]["ready"][1] and seen[23]["ready"][1]
        assert snaps[17].born[1] == 12 * RESEAT - 35
        # 3 * (2*35 + 120 + 1) floats: no multiple of 4
        assert snaps[17].payload[0].size == 573


def expected_payload(eng, sids, nproc, nbk, keep):
    """numpy gather of the live ranges, from the engine's public views."""
    bs, bc, pr, lv = (t.cpu().numpy() for t in
                      (eng.bsum, eng.bcnt, eng.proc, eng.last_val))
    bidx = (nproc + np.arange(nbk)) % eng.G
    pidx = (nproc - keep + np.arange(keep)) % eng.G
    out = np.empty((len(sids), eng.C, 2 * nbk + keep + 1), np.float32)
    for i, s in enumerate(sids):
        out[i, :, 0:2 * nbk:2] = bs[s][:, bidx]
        out[i, :, 1:2 * nbk:2] = bc[s][:, bidx]
        out[i, :, 2 * nbk:2 * nbk + keep] = pr[s][:, pidx]
        out[i, :, -1] = lv[s]
    return out


def check_isolation(src, make_target):
    """Snapshot sids [0, S-1] of a ring-filled engine ``src`` standing at
    nproc 241 (both ranges wrap at G=128), restore into a fresh engine:
    listed slots match on their live ranges and hold nothing else, the
    slots in between stay never-used."""
    src.head, src.nproc, src._cleared = 276, 241, 276
    sids = [0, src.S - 1]
    snap = src.snapshot(sids)
    snap.payload = snap.payload.copy()   # out of the reused host buffer
    assert (snap.nbk, snap.keep) == (35, 120)
    want = expected_payload(src, sids, 241, 35, 120)
    assert np.array_equal(snap.payload, want)
    assert np.array_equal(src.snapshot(sids + sids).payload,
                          np.concatenate([want, want]))   # duplicates
    assert src.snapshot([]).payload.shape == (0, src.C, 191)
    dst = make_target()
    dst.restore(snap)
    assert (dst.head, dst.nproc, dst._cleared) == (276, 241, 276)
    assert np.array_equal(dst.snapshot(sids).payload, want)
    bidx = (241 + np.arange(35)) % dst.G
    pidx = (121 + np.arange(120)) % dst.G
    for name, idx in (("bsum", bidx), ("bcnt", bidx), ("proc", pidx)):
        t = getattr(dst, name).cpu().numpy()
        mask = np.ones(dst.G, bool)
        mask[idx] = False
        assert not t[sids][:, :, mask].any(), name   # only the live range
        assert not t[1:src.S - 1].any(), name        # neighbours untouched
    assert torch.isnan(dst.last_val[1:src.S - 1]).all()
    return snap


def check_refusals(snap, make_target):
    """Every refused restore raises ValueError and leaves the target
    fresh; an empty snapshot moves the indices only."""
    for bad in ((0, S), (-1, 0), (2, 2), (0, None)):
        e = make_target()
        sid_map = {k: v for k, v in zip((0, S - 1), bad) if v is not None}
        with pytest.raises(ValueError):
            e.restore(snap, sid_map=sid_map)   # range, duplicate, missing
        assert e.head == e.nproc == 0 and not e.proc.any()
    e = make_target()
    e.restore(snap, sid_map={0: 3, S - 1: 1})      # dict form, remapped
    assert np.array_equal(e.snapshot([3, 1]).payload, snap.payload)
    with pytest.raises(ValueError):
        e.restore(snap)                            # no longer fresh
    with pytest.raises(ValueError):
        e.snapshot([S])
    with pytest.raises(ValueError):
        e.snapshot([0], keep=e.nproc - e._proc_floor + 1)
    dev = str(e.device)
    with pytest.raises(ValueError):                # geometry: channels
        StreamEngine(S, C + 1, ring_grid=G, device=dev).restore(snap)
    with pytest.raises(ValueError):                # geometry: window
        StreamEngine(S, C, ring_grid=G, win_buckets=24,
                     device=dev).restore(snap)
    with pytest.raises(ValueError):                # keep = 120 > G = 64
        StreamEngine(S, C, ring_grid=64, device=dev).restore(snap)
    with pytest.raises(ValueError):                # sid 4 >= S = 3
        StreamEngine(3, C, ring_grid=G, device=dev).restore(snap)
    e = make_target()
    empty = EngineSnapshot(**{**snap.__dict__, "sids": snap.sids[:0],
                              "born": snap.born[:0],
                              "payload": snap.payload[:0]})
    e.restore(empty)
    assert e.nproc == 241 and not e.proc.any() and not e.bsum.any()
    assert torch.isnan(e.last_val).all()


def _filled_cpu():
    e = StreamEngine(S, C, ring_grid=G, device="cpu")
    g = torch.Generator().manual_seed(5)
    for name in ("bsum", "bcnt", "proc", "last_val"):
        t = getattr(e, name)
        t.copy_(torch.rand(t.shape, generator=g) + 1.0)
    return e


class TestSnapshotRestoreCpu:
    def test_isolation_and_refusals(self):
        fresh = lambda: StreamEngine(S, C, ring_grid=G)  # noqa: E731
        snap = check_isolation(_filled_cpu(), fresh)
        check_refusals(snap, fresh)


class TestFloorCheck:
    # G=256: a batch of two windows (132 points back) fits the ring
    def test_windows_refuse_to_reach_below_the_floor(self, ref_cpu):
        _ev, _seen, snaps = ref_cpu
        e = StreamEngine(S, C, ring_grid=256)
        before = [e.windows(batch=b, stride=12).clone() for b in (1, 2)]
        e.restore(snaps[17])                       # nproc 169, keep 120
        assert e._proc_floor == 49
        with pytest.raises(ValueError, match="restored"):
            e.windows(batch=2, stride=12)
        assert e.windows(batch=1, stride=12).any()
        # a fresh engine behaves as before: floor 0, zeros, no error
        f = StreamEngine(S, C, ring_grid=256)
        assert f._proc_floor == 0
        for b, w in zip((1, 2), before):
            assert torch.equal(f.windows(batch=b, stride=12), w)
            assert not w.any()
        # the short-tail snapshot carries everything: no floor
        e5 = StreamEngine(S, C, ring_grid=256)
        e5.restore(snaps[5])
        assert e5._proc_floor == 0
        e5.windows(batch=2, stride=12)


# ------------------------------------------------------------------- file
class TestSnapshotFile:
    @pytest.fixture
    def saved(self, ref_cpu, tmp_path):
        snap = ref_cpu[2][17]
        payload = snap.payload.copy()
        payload[1, :, -1] = np.nan   # a stream that has no carry yet
        snap = dataclasses.replace(snap, payload=payload)
        path = str(tmp_path / "engine.snap")
        extra = {"positions": {"HR/0": 4096}, "hwm": 1019.999, "who": "x"}
        snap.save(path, extra)
        return snap, path, extra

    def test_round_trip_is_bit_equal(self, saved):
        snap, path, extra = saved
        back, got = EngineSnapshot.load(path)
        assert got == extra
        assert np.isnan(snap.payload).any()   # NaN carries survive as bits
        assert back.payload.tobytes() == snap.payload.tobytes()
        assert back.payload.dtype == np.float32
        assert (back.sids == snap.sids).all() and back.sids.dtype == np.int64
        assert (back.born == snap.born).all()
        assert back.geometry == snap.geometry
        for key in ("head", "nproc", "cleared", "origin_nproc",
                    "forced_ready", "nbk", "keep"):
            assert getattr(back, key) == getattr(snap, key), key
        e = StreamEngine(S, C, ring_grid=G)
        e.restore(back)
        assert e.snapshot().payload.tobytes() == snap.payload.tobytes()
        assert not os.path.exists(path + ".tmp")

    def test_damaged_files_raise_snapshot_error(self, saved, tmp_path):
        _snap, path, _extra = saved
        good = open(path, "rb").read()
        hlen = struct.unpack_from("<I", good, 12)[0]
        bad = str(tmp_path / "bad.snap")

        def refused(data):
            with open(bad, "wb") as fh:
                fh.write(data)
            with pytest.raises(SnapshotError):
                EngineSnapshot.load(bad)

        # cut inside the magic, the header, the id arrays, the payload, the
        # checksum; and an empty file
        for cut in (0, 5, 16 + hlen // 2, 16 + hlen + 20, len(good) // 2,
                    len(good) - 1000, len(good) - 1):
            refused(good[:cut])
        refused(good + b"\0")                      # trailing bytes
        flipped = bytearray(good)
        flipped[len(good) - 2000] ^= 0x10          # one payload bit
        refused(bytes(flipped))
        refused(b"TSKDSNAQ" + good[8:])            # magic
        refused(good[:8] + struct.pack("<I", 2) + good[12:])   # version
        assert issubclass(SnapshotError, ValueError)
        assert EngineSnapshot.load(path)[0].nproc == 169   # original intact

    def test_interrupted_save_keeps_the_old_file(self, saved, ref_cpu,
                                                 monkeypatch):
        snap, path, extra = saved
        newer = ref_cpu[2][23]

        def crash(*_a):
            raise OSError("killed before the rename")

        monkeypatch.setattr(os, "replace", crash)
        with pytest.raises(OSError):
            newer.save(path, {"who": "y"})
        monkeypatch.undo()
        back, got = EngineSnapshot.load(path)
        assert got == extra and back.nproc == snap.nproc == 169
        newer.save(path, {"who": "y"})             # and the next one lands
        back, got = EngineSnapshot.load(path)
        assert got == {"who": "y"} and back.nproc == 241


# ------------------------------------------------------------- slot table
@pytest.fixture
def bus(tmp_path):
    return Bus(str(tmp_path / "bus"))


class TestSlotTableHandOver:
    def _mk(self, bus):
        bus.create_topic("HR")
        c = Consumer(bus, starting="earliest")
        c.subscribe(["HR"])
        return c

    def test_successor_hands_out_the_same_sids(self, bus):
        p, a = Producer(bus), self._mk(bus)
        for i, key in enumerate("abcde"):
            _send(p, "HR", key, 10.0 * i)          # last seen 0, 10, .., 40
        a.poll_samples_sid(max_msgs=100, max_streams=8)
        assert sorted(a.evict_idle(15.0)) == [("a", 0), ("b", 1)]
        entries, high_water = a.slot_table()
        assert sorted(entries) == [("c", 2, 20.0), ("d", 3, 30.0),
                                   ("e", 4, 40.0)]
        assert high_water == 5
        b = self._mk(bus)
        b.restore_slots(entries, high_water)
        assert b.n_streams() == 3 and b.sid_high_water() == 5
        assert sorted(b.slot_table()[0]) == sorted(entries)
        for key, off in a.positions().items():
            topic, _, part = key.rpartition("/")
            b.seek(topic, int(part), off)
        for key in "xyz":
            _send(p, "HR", key, 50.0)
        _send(p, "HR", "d", 51.0)
        got = [c.poll_samples_sid(max_msgs=100, max_streams=8)
               for c in (a, b)]
        for sa, _ca, _va, _ta, nk in got:
            assert nk == [("x", 0), ("y", 1), ("z", 5)]   # lowest free first
            assert list(sa) == [0, 1, 5, 3]
        # the restored last-seen times decide who is idle: c (20) goes, d
        # (seen again at 51) and e (40) stay
        assert b.evict_idle(35.0) == a.evict_idle(35.0) == [("c", 2)]

    def test_only_before_the_first_poll_and_no_duplicates(self, bus):
        p, c = Producer(bus), self._mk(bus)
        for bad in ([("a", 0, 1.0), ("b", 0, 2.0)],     # sid twice
                    [("a", 0, 1.0), ("a", 1, 2.0)],     # key twice
                    [("a", 2, 1.0)], [("a", -1, 1.0)]):  # outside high water
            with pytest.raises(ValueError):
                c.restore_slots(bad, 2)
        assert c.n_streams() == 0 and c.sid_high_water() == 0
        c.restore_slots([], 0)
        _send(p, "HR", "k", 1.0)
        c.poll_samples_sid(max_msgs=10, max_streams=4)
        with pytest.raises(RuntimeError, match="first poll"):
            c.restore_slots([("a", 0, 1.0)], 1)
        d = self._mk(bus)
        d.poll(max_msgs=1)
        with pytest.raises(RuntimeError, match="first poll"):
            d.restore_slots([("a", 0, 1.0)], 1)


# ----------------------------------------------------------------- daemon
N_CH = 4
LAST = 34                 # triggers in the uninterrupted run
SNAP_EVERY, DROP_AFTER = 3, 17   # last snapshot at 15, dropped two later
IDLE_S = 240.0
# who streams during which triggers (one sample per 5 s and channel):
# p2 falls silent and is evicted at trigger 11, leaving slot 1 free; p4
# arrives in trigger 9 (warm-up counts from grid point 96, so it is still
# gated at the snapshot, nproc 142, and opens at trigger 22); p5 arrives
# after the restart and must be given slot 1
PATIENTS = {"p000001": (1, LAST), "p000002": (1, 6), "p000003": (1, LAST),
            "p000004": (9, LAST), "p000005": (20, LAST)}


def _value(pid, ch, t):
    return float(40 + 3 * int(pid[1:]) + 2 * ch + (int(t) // 5) % 9)


class Daemon:
    """A bus, a store and the per-minute chunks of the scenario; servers
    come and go (``serve``), the bus and the store stay."""

    def __init__(self, tmp_path, tag, device):
        from tskd_amd.config import get_global_config
        from tskd_amd.store import PredictionStore
        self.cfg = get_global_config()
        self.bus = Bus(str(tmp_path / f"bus_{tag}"))
        self.store = PredictionStore(str(tmp_path / f"pred_{tag}.log"))
        self.topics = [self.cfg.topic_for_channel(c)
                       for c in self.cfg.channel_names[:N_CH]]
        for t in self.topics:
            self.bus.create_topic(t)
        self.prod = Producer(self.bus)
        self.device = device
        self.state = str(tmp_path / f"state_{tag}" / "serve-rank0of1.snap")
        os.makedirs(os.path.dirname(self.state), exist_ok=True)

    def serve(self, state=True, **kw):
        from tskd_amd.cli.serve import FusedServer
        torch.manual_seed(7)   # identical random-init model weights
        kw.setdefault("evict_idle_s", IDLE_S)
        return FusedServer(self.bus, self.cfg, self.store,
                           device=self.device, max_streams=4, ring_grid=1024,
                           starting="earliest",
                           state_path=self.state if state else None,
                           snapshot_every=SNAP_EVERY, **kw)

    def produce(self, m):
        """The chunk of trigger m: event time [60 (m-1), 60 m)."""
        for step in range(12):
            t = (m - 1) * 60 + step * 5
            for pid, (first, last) in PATIENTS.items():
                if first <= m <= last:
                    for ch in range(N_CH):
                        self.prod.produce(
                            self.topics[ch], pid,
                            json.dumps([ch, _value(pid, ch, t)]),
                            ts_us=int(t * 1e6))

    def rows(self):
        return [(p, int(round(t.timestamp() * 1e6)), r)
                for p, t, r in self.store.tail(self.store.count())]


def run_daemon(tmp_path, device):
    """(uninterrupted, interrupted) runs of the scenario: per run the store
    rows, p5's sid, the final live count and the servers."""
    out = {}
    ref = Daemon(tmp_path, "ref", device)
    srv = ref.serve(state=False)
    for m in range(1, LAST + 1):
        ref.produce(m)
        srv.trigger()
    out["ref"] = (ref.rows(), dict(srv.pid_index), srv.consumer.n_streams(),
                  srv)
    cut = Daemon(tmp_path, "cut", device)
    first = cut.serve()
    for m in range(1, DROP_AFTER + 1):
        cut.produce(m)
        first.trigger()
        if m == 15:
            # the snapshot moment: slot 1 free, p4 (slot 3) still gated
            assert first.pids == ["p000001", None, "p000003", "p000004"]
            assert list(first.se.stream_ready()) == [True, True, True, False]
            at_snapshot = (first.se.nproc, len(cut.rows()))
    assert len(cut.rows()) > at_snapshot[1]    # scored since the snapshot
    del first                                  # dropped: no final snapshot
    second = cut.serve()
    assert second.load_state() is True
    assert second.se.nproc == at_snapshot[0] == 12 * 15 - 38
    assert second.pids == ["p000001", None, "p000003", "p000004"]
    assert "restore_failed" not in second.timer.gauges
    second.trigger()        # replays the chunks of triggers 16 and 17
    for m in range(DROP_AFTER + 1, LAST + 1):
        cut.produce(m)
        second.trigger()
    second.save_state()
    out["cut"] = (cut.rows(), dict(second.pid_index),
                  second.consumer.n_streams(), second)
    out["state"] = cut.state
    return out


def check_daemon(out):
    ref_rows, ref_index, ref_live, _ = out["ref"]
    cut_rows, cut_index, cut_live, _ = out["cut"]
    # the replay wrote trigger 17's predictions a second time, bit for bit
    assert len(cut_rows) > len(set(cut_rows))
    assert len(ref_rows) == len(set(ref_rows))
    assert sorted(set(cut_rows)) == sorted(ref_rows)
    first = lambda rows, pid: min(t for p, t, _r in rows   # noqa: E731
                                  if p == pid)
    # p4 was gated across the restart: same first prediction, trigger 22
    assert first(cut_rows, "p000004") == first(ref_rows, "p000004") \
        == int((22 * 60 - 5) * 1e6)
    assert {p for p, _t, _r in ref_rows} == set(PATIENTS) - {"p000002"}
    assert cut_index == ref_index and cut_index["p000005"] == 1
    assert cut_live == ref_live == 4


@pytest.fixture(scope="module")
def daemon_cpu(tmp_path_factory):
    return run_daemon(tmp_path_factory.mktemp("warm"), "cpu")


def check_cold_starts(tmp_path, state, device):
    """A corrupt file and a file of another world are refused: error line,
    restore_failed = 1, and the server serves from cold."""
    d = Daemon(tmp_path, "cold", device)
    data = bytearray(open(state, "rb").read())
    data[len(data) // 2] ^= 0x01
    with open(d.state, "wb") as fh:
        fh.write(bytes(data))
    srv = d.serve()
    assert srv.load_state() is False
    assert srv.timer.gauges["restore_failed"] == 1
    assert srv.se.nproc == 0 and srv.pids == [] and srv.hwm == 0.0
    d.produce(1)
    srv.trigger()                                  # cold start works
    assert sorted(srv.pid_index) == ["p000001", "p000002", "p000003"]
    other = d.serve(state=False, rank=0, world=2)
    assert other.load_state(state) is False        # intact, but world 1
    assert other.timer.gauges["restore_failed"] == 1
    assert other.se.nproc == 0 and other.consumer.n_streams() == 0
    missing = d.serve(state=False)
    assert missing.load_state(state + ".none") is False
    assert missing.timer.gauges["restore_failed"] == 1


class TestDaemonWarmRestart:
    def test_resumed_run_writes_the_uninterrupted_rows(self, daemon_cpu):
        check_daemon(daemon_cpu)

    def test_state_file_is_one_file_with_offsets_and_slots(self, daemon_cpu):
        state = daemon_cpu["state"]
        assert os.listdir(os.path.dirname(state)) == ["serve-rank0of1.snap"]
        snap, extra = EngineSnapshot.load(state)
        srv = daemon_cpu["cut"][3]
        assert sorted(extra) == ["high_water", "hwm", "model", "positions",
                                 "rank", "slots", "world"]
        assert extra["positions"] == srv.consumer.positions()
        assert (extra["rank"], extra["world"]) == (0, 1)
        assert extra["model"] == "MyCNN5" and extra["high_water"] == 4
        assert sorted(s for _k, s, _t in extra["slots"]) == \
            snap.sids.tolist() == [0, 1, 2, 3]     # live slots only
        assert extra["hwm"] == srv.hwm == (LAST - 1) * 60 + 55.0

    def test_pipelined_trigger_is_persisted_before_the_snapshot(
            self, tmp_path):
        d = Daemon(tmp_path, "pipe", "cpu")
        srv = d.serve(pipelined=True)
        for m in range(1, 16):
            d.produce(m)
            srv.trigger()
        # trigger 15 wrote the file: its own predictions are in the store
        assert srv._pending is None
        assert max(t for _p, t, _r in d.rows()) == int((15 * 60 - 5) * 1e6)

    def test_refused_files_mean_a_cold_start(self, daemon_cpu, tmp_path):
        check_cold_starts(tmp_path, daemon_cpu["state"], "cpu")

    def test_free_slots_need_the_lifecycle(self, tmp_path):
        """A file with a free slot (None in pids) goes to a server that
        gives slots back only; one that never reuses a slot refuses it. A
        file without free slots is fine for it."""
        d = Daemon(tmp_path, "free", "cpu")
        srv = d.serve()
        for m in range(1, 13):
            d.produce(m)
            srv.trigger()
            if m == 6:
                srv.save_state(d.state + ".full")      # nobody evicted yet
        assert srv.pids == ["p000001", None, "p000003", "p000004"]
        off = d.serve(state=False, evict_idle_s=0.0)
        assert off.load_state(d.state) is False
        assert off.timer.gauges["restore_failed"] == 1 and off.pids == []
        assert off.load_state(d.state + ".full") is True
        assert off.pids == ["p000001", "p000002", "p000003"]
        assert off.se.nproc == 12 * 6 - 38 and off.hwm == 355.0

    def test_state_dir_with_poll_thread_is_rejected(self, tmp_path, capsys):
        from tskd_amd.cli import serve
        with pytest.raises(SystemExit) as ei:
            serve.main(["--state-dir", str(tmp_path), "--poll-thread",
                        "--bus-dir", str(tmp_path / "bus")])
        assert ei.value.code == 2
        assert "--state-dir cannot be combined with --poll-thread" in \
            capsys.readouterr().err
        assert serve.state_file("d", 1, 4) == os.path.join(
            "d", "serve-rank1of4.snap")

    def test_save_state_refuses_a_running_poll_thread(self, tmp_path):
        d = Daemon(tmp_path, "thr", "cpu")
        srv = d.serve(state=False)
        srv.start_poll_thread(interval_s=0.001)
        try:
            with pytest.raises(RuntimeError, match="poll thread"):
                srv.save_state(d.state)
        finally:
            srv.stop_poll_thread()
        assert not os.path.exists(d.state)

    def test_supervisor_knows_the_stage(self):
        from tskd_amd.parallel import supervisor
        assert supervisor.STAGES["serve"] == "tskd_amd.cli.serve"

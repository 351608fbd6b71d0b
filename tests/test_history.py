"""Risk history on the CPU: ``StreamEngine.score_history`` takes the
reference path there (``windows(batch=k - jmin)`` -> every window its own
one-step sequence -> ``MyCNNEngine.forward``), which is also the GPU kernel's
oracle (tests/test_history_gpu.py). It is held against a hand-written loop
that calls the model once per (stream, column), against the scores a
trigger-by-trigger run produced, and the daemon's ``--reload-check`` /
``--reload-max-shift`` are run end to end.

Bound of the loop comparison: tests/test_attribution.py's between the engine
and its loop. Both sides run the same fp32 model on the same (1, C, 120)
input, one window at a time, so the expected difference is zero; rtol = atol
= 1e-6 allows a few fp32 ulps at the O(1) logits.
"""

import copy
import json
import os

import numpy as np
import pytest
import torch

from tskd_amd.bus import Bus, Consumer
from tskd_amd.engine import StreamEngine
from tskd_amd.metrics import prometheus_text

from test_attribution import N_TRIGGERS, PIDS, PLAIN, run_daemon

G = 192
L = 120
S = 4
TOL = 1e-6
K_STRIDES = ((1, 12), (2, 12), (5, 12), (7, 12), (8, 12), (3, 1), (4, 13),
             (2, 72), (6, 40))
RELOAD_GAUGES = ("reload_checked_windows", "reload_shift_max",
                 "reload_shift_mean", "reload_nonfinite",
                 "reload_rejected_total")


def _model_engine(name, seed):
    from tskd_amd.models import build_model
    from tskd_amd.ops import MyCNNEngine
    torch.manual_seed(seed)
    return MyCNNEngine(build_model(name).eval(), device="cpu")


@pytest.fixture(scope="module")
def engines():
    return {"MyCNN5": _model_engine("MyCNN5", 400),
            "MyCNN2": _model_engine("MyCNN2", 401)}


def _ring(C, seed, nproc):
    se = StreamEngine(S, C, ring_grid=G)
    gen = torch.Generator().manual_seed(seed)
    se.proc.copy_(torch.randn(S, C, G, generator=gen) * 2.0)
    se.nproc = nproc
    return se


def jmin_of(nproc, ring, k, stride, floor=0):
    """Number of unavailable columns, from the definition: column j ends at
    e_j = nproc - (k-1-j)*stride and is available iff e_j - 120 >= lo."""
    lo = max(0, nproc - ring, floor)
    return sum(nproc - (k - 1 - j) * stride - L < lo for j in range(k))


def _loop(se, me, sids, k, stride, age, sig):
    """One model call per (stream, column), written out by hand."""
    lo = max(0, se.nproc - se.G)
    out = torch.full((len(sids), k), float("nan"))
    with torch.no_grad():
        for r, s in enumerate(sids):
            a = torch.zeros(1) if age is None else age.reshape(-1)[s:s + 1]
            for j in range(k):
                e = se.nproc - (k - 1 - j) * stride
                if e - L < lo:
                    continue
                idx = torch.from_numpy(np.arange(e - L, e) % se.G)
                y = me.model(se.proc[s][:, idx].unsqueeze(0), a)
                out[r, j] = torch.sigmoid(y)[0] if sig else y[0]
    return out


class TestReferencePath:
    @pytest.mark.parametrize("nproc", [200, 372])
    @pytest.mark.parametrize("variant", ["MyCNN5", "MyCNN2"])
    def test_matches_a_loop_over_the_model(self, engines, variant, nproc):
        me = engines[variant]
        assert not me.supports_history(me.cin)       # a CPU engine
        se = _ring(me.cin, seed=17 + me.cin, nproc=nproc)
        age_t = (40.0 + 9.0 * torch.arange(S, dtype=torch.float32)
                 ).reshape(S, 1)
        n_nan = 0
        for k, stride in K_STRIDES:
            for sids, age, sig in (([2, 0, 2], None, False),
                                   (None, age_t, True)):
                listed = list(range(S)) if sids is None else sids
                got = se.score_history(me, sids, k, stride, age, sig)
                want = _loop(se, me, listed, k, stride, age, sig)
                assert got.shape == (len(listed), k)
                assert got.dtype == torch.float32
                nan = torch.isnan(got)
                jm = jmin_of(nproc, G, k, stride)
                assert jm < k
                assert nan[:, :jm].all() and not nan[:, jm:].any()
                assert torch.equal(nan, torch.isnan(want))
                torch.testing.assert_close(got[:, jm:], want[:, jm:],
                                           rtol=TOL, atol=TOL)
                n_nan += jm
        # the set holds both kinds: 200 keeps 80 points of room, 372 has 72
        assert n_nan > 0
        # not vacuous: neighbouring columns score different windows, and the
        # newest one is the plain score of the latest window
        got = se.score_history(me, None, 2, 12, age_t, True)
        assert (got[:, 0] != got[:, 1]).all()
        plain = me.forward(se.windows(batch=1), age_t, apply_sigmoid=True)
        torch.testing.assert_close(got[:, 1:], plain, rtol=TOL, atol=TOL)

    def test_nan_prefix_examples(self, engines):
        me = engines["MyCNN5"]
        for nproc, k, stride, want in ((120, 5, 12, 4), (120, 1, 12, 0),
                                       (372, 8, 12, 1), (372, 7, 12, 0)):
            se = _ring(10, seed=3, nproc=nproc)
            got = se.score_history(me, [1], k, stride)
            assert int(torch.isnan(got).sum()) == want
            assert jmin_of(nproc, G, k, stride) == want
            assert not torch.isnan(got[:, want:]).any()

    def test_refusals(self, engines):
        me = engines["MyCNN5"]
        se = _ring(10, seed=29, nproc=200)
        for bad in ([-1], [S], [0, S]):
            with pytest.raises(ValueError, match="out of range"):
                se.score_history(me, bad)
        with pytest.raises(ValueError, match="k=0"):
            se.score_history(me, [0], k=0)
        with pytest.raises(ValueError, match="stride=0"):
            se.score_history(me, [0], stride=0)
        se.nproc = 119
        with pytest.raises(ValueError, match="no full model window"):
            se.score_history(me, [0])
        se.nproc = 200
        se._proc_floor = 100            # as after a restore with keep=100
        with pytest.raises(ValueError, match="restored"):
            se.score_history(me, [0])
        se._proc_floor = 0
        out = se.score_history(me, [], k=5)
        assert out.shape == (0, 5) and out.dtype == torch.float32


@pytest.mark.parametrize("ring", [256, 192])
def test_history_is_what_each_trigger_scored(engines, ring):
    """Ingest dense random data one trigger (12 grid points) at a time and
    keep every trigger's score of the latest window: the history at the end
    is that sequence, exactly (same windows, same model, one at a time).
    With ring = 192 the last five triggers cross the ring's wrap."""
    me = engines["MyCNN5"]
    se = StreamEngine(3, 10, ring_grid=ring, fs=25.0)
    gen = torch.Generator().manual_seed(77)
    age = torch.tensor([[30.0], [55.0], [80.0]])
    kept = []
    for m in range(19):
        se.ingest_dense(torch.randn(3, 10, 12 * se.bucket_len,
                                    generator=gen))
        if se.nproc >= L:
            kept.append(me.forward(se.windows(batch=1), age,
                                   apply_sigmoid=True))
    assert se.nproc == 12 * 19 - 35 and len(kept) >= 6
    assert (se.nproc > ring) == (ring == 192)
    want = torch.cat(kept[-5:], dim=1)
    got = se.score_history(me, None, k=5, stride=12, age=age)
    assert not torch.isnan(got).any()
    assert torch.equal(got, want)
    assert (got[:, 1:] != got[:, :-1]).all()


# ---------------------------------------------------------------- the daemon
def _save(model, path, newer_than=None):
    from tskd_amd.models.checkpoint import save_checkpoint
    save_checkpoint(model, str(path))
    if newer_than is not None:
        os.utime(str(path), (newer_than + 10, newer_than + 10))


def _one_more_trigger(srv, tmp_path, tag):
    """Stream-minute N_TRIGGERS + 1 of run_daemon's feed, one trigger, and
    every response published so far."""
    cfg = srv.cfg
    topics = [cfg.topic_for_channel(c) for c in cfg.channel_names]
    for step in range(12):
        t = N_TRIGGERS * 60 + step * 5
        for i, pid in enumerate(PIDS):
            for ch in range(cfg.n_channels):
                srv.producer.produce(topics[ch], pid, json.dumps(
                    [ch, ((t // 5 + 11 * ch) % 120) / 60.0 - 1.0 + 0.3 * i]),
                    ts_us=int(t * 1e6))
    srv.trigger()
    reader = Consumer(Bus(str(tmp_path / f"bus_{tag}")), starting="earliest")
    reader.subscribe(["risk"])
    return [(x.key.decode(), x.value)
            for x in reader.poll(max_msgs=256, timeout_ms=0)]


class TestDaemonReloadCheck:
    def test_same_weights_are_accepted_with_zero_shift(self, tmp_path):
        srv, _log = run_daemon(tmp_path, "same", reload_check=4)
        path = tmp_path / "same.pth"
        _save(srv.me.model, path)
        srv.model_path = str(path)
        srv._model_mtime = os.path.getmtime(str(path))
        assert srv.maybe_reload_model() is False     # nothing changed
        assert not any(k in srv.timer.gauges for k in RELOAD_GAUGES)
        _save(srv.me.model, path, newer_than=srv._model_mtime)
        before = srv.me
        assert srv.maybe_reload_model() is True
        assert srv.me is not before
        g = srv.timer.gauges
        assert g["reload_shift_max"] == 0.0
        assert g["reload_shift_mean"] == 0.0
        assert g["reload_nonfinite"] == 0
        # both slots, all four triggers: nproc = 166 reaches back to 10
        assert g["reload_checked_windows"] == 8
        assert "reload_rejected_total" not in g
        text = prometheus_text([srv.timer])
        assert ('tskd_streams{stage="serve",state="reload_checked_windows"}'
                ' 8') in text
        assert 'state="reload_shift_max"} 0' in text

    def test_a_shifted_head_is_refused(self, tmp_path, monkeypatch):
        srv, _log = run_daemon(tmp_path, "shift", reload_check=4,
                               reload_max_shift=0.2)
        ref, _log = run_daemon(tmp_path, "never")
        bad = copy.deepcopy(srv.me.model)
        with torch.no_grad():
            bad.out.bias += 10.0
        path = tmp_path / "shift.pth"
        _save(bad, path)
        srv.model_path = str(path)
        before = srv.me
        assert srv.maybe_reload_model() is False
        assert srv.me is before
        g = srv.timer.gauges
        assert g["reload_rejected_total"] == 1
        assert g["reload_checked_windows"] == 8
        assert g["reload_shift_max"] > 0.2
        assert 0.0 < g["reload_shift_mean"] <= g["reload_shift_max"]
        assert g["reload_nonfinite"] == 0
        # the same file is not looked at again
        calls = []
        real = srv.se.score_history
        monkeypatch.setattr(srv.se, "score_history",
                            lambda *a, **kw: calls.append(1) or real(*a, **kw))
        assert srv.maybe_reload_model() is False
        assert calls == [] and g["reload_rejected_total"] == 1
        # and serving goes on as if the file had never been there
        got = _one_more_trigger(srv, tmp_path, "shift")
        want = _one_more_trigger(ref, tmp_path, "never")
        assert got == want and len(got) == 2 * (N_TRIGGERS - 13 + 1)
        # without the limit the same candidate is reported and goes live
        srv.reload_max_shift = None
        _save(bad, path, newer_than=os.path.getmtime(str(path)))
        assert srv.maybe_reload_model() is True
        assert srv.me is not before
        assert g["reload_rejected_total"] == 1
        assert g["reload_shift_max"] > 0.2

    def test_nan_weights_are_refused(self, tmp_path):
        srv, _log = run_daemon(tmp_path, "nan", reload_check=2,
                               reload_max_shift=1.0)
        bad = copy.deepcopy(srv.me.model)
        with torch.no_grad():
            bad.out.weight.fill_(float("nan"))
        path = tmp_path / "nan.pth"
        _save(bad, path)
        srv.model_path = str(path)
        assert srv.maybe_reload_model() is False
        g = srv.timer.gauges
        assert g["reload_nonfinite"] == g["reload_checked_windows"] == 4
        assert g["reload_rejected_total"] == 1

    def test_off_is_byte_identical(self, tmp_path):
        srv, log = run_daemon(tmp_path, "off")
        _ref, plain = run_daemon(tmp_path, "plain", reload_check=0,
                                 reload_max_shift=None)
        assert [(m, msgs) for m, msgs, _d in log] == \
            [(m, msgs) for m, msgs, _d in plain]
        payloads = [v for _m, msgs, _d in log for _k, v in msgs]
        assert payloads and all(PLAIN.match(v) for v in payloads)
        # a reload with the flags off swaps as before and sets no gauge
        path = tmp_path / "off.pth"
        _save(srv.me.model, path)
        srv.model_path = str(path)
        before = srv.me
        assert srv.maybe_reload_model() is True and srv.me is not before
        assert not any(k in srv.timer.gauges for k in RELOAD_GAUGES)
        assert "reload_" not in prometheus_text([srv.timer])

    def test_no_ready_slot_swaps_unchecked(self, tmp_path):
        from tskd_amd.cli.serve import FusedServer
        from tskd_amd.config import get_global_config
        torch.manual_seed(7)
        srv = FusedServer(Bus(str(tmp_path / "bus_empty")),
                          get_global_config(), None, max_streams=4,
                          ring_grid=256, reload_check=4, reload_max_shift=0.0)
        path = tmp_path / "empty.pth"
        _save(srv.me.model, path)
        srv.model_path = str(path)
        assert srv.maybe_reload_model() is True
        assert srv.timer.gauges["reload_checked_windows"] == 0
        assert "reload_rejected_total" not in srv.timer.gauges

    def test_arguments(self, tmp_path):
        from tskd_amd.cli import serve
        with pytest.raises(SystemExit):
            serve.main(["--reload-max-shift", "0.2"])
        with pytest.raises(SystemExit):
            serve.main(["--reload-check", "-1"])
        with pytest.raises(ValueError, match="reload_check"):
            run_daemon(tmp_path, "bare", reload_max_shift=0.2)
        with pytest.raises(ValueError, match="negative"):
            run_daemon(tmp_path, "neg", reload_check=-1)

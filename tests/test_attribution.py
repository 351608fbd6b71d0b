"""Channel attribution on the CPU: ``StreamEngine.attribute_latest`` takes
the reference path there (windows -> one channel overwritten per copy ->
``MyCNNEngine.forward``), which is also the GPU kernel's oracle
(tests/test_attribution_gpu.py). It is held against a hand-written loop that
calls the model once per (stream, variant), and the daemon's
``--explain-above`` is run end to end.

Bound of the loop comparison: both sides run the same fp32 model on the same
(1, C, 120) input, one window at a time, so the expected difference is zero;
rtol = atol = 1e-6 allows a few fp32 ulps at the O(1) logits.
"""

import json
import re

import numpy as np
import pytest
import torch

from tskd_amd.bus import Bus, Consumer, Producer
from tskd_amd.engine import StreamEngine
from tskd_amd.metrics import prometheus_text

G = 192
L = 120
S = 4
NPROC = 200          # the window straddles the ring's wrap
TOL = 1e-6


def _model_engine(name, seed):
    from tskd_amd.models import build_model
    from tskd_amd.ops import MyCNNEngine
    torch.manual_seed(seed)
    return MyCNNEngine(build_model(name).eval(), device="cpu")


@pytest.fixture(scope="module")
def engines():
    return {"MyCNN5": _model_engine("MyCNN5", 300),
            "MyCNN2": _model_engine("MyCNN2", 301)}


def _ring(C, seed, nproc=NPROC):
    se = StreamEngine(S, C, ring_grid=G)
    gen = torch.Generator().manual_seed(seed)
    se.proc.copy_(torch.randn(S, C, G, generator=gen) * 2.0)
    se.nproc = nproc
    return se


def _window_slots(nproc):
    return torch.from_numpy(np.arange(nproc - L, nproc) % G)


def _loop(se, me, sids, age, baseline, sig):
    """One model call per (stream, variant), written out by hand."""
    idx = _window_slots(se.nproc)
    rows = []
    with torch.no_grad():
        for s in sids:
            x = se.proc[s][:, idx]                       # (C, 120)
            a = torch.zeros(1) if age is None else age.reshape(-1)[s:s + 1]
            row = []
            for k in range(se.C + 1):
                v = x.clone()
                if k:
                    v[k - 1] = 0.0 if baseline == "zero" else x[k - 1, 0]
                y = me.model(v.unsqueeze(0), a)
                row.append(torch.sigmoid(y) if sig else y)
            rows.append(torch.cat(row))
    return torch.stack(rows)


class TestReferencePath:
    @pytest.mark.parametrize("baseline", ["hold", "zero"])
    @pytest.mark.parametrize("variant", ["MyCNN5", "MyCNN2"])
    def test_matches_a_loop_over_the_model(self, engines, variant, baseline):
        me = engines[variant]
        assert not me.supports_attribution(me.cin)   # a CPU engine
        se = _ring(me.cin, seed=11 + me.cin)
        age_t = (40.0 + 9.0 * torch.arange(S, dtype=torch.float32)
                 ).reshape(S, 1)
        for sids in ([2, 0, 2], None):
            listed = list(range(S)) if sids is None else sids
            for age in (None, age_t):
                for sig in (False, True):
                    got = se.attribute_latest(me, sids, age, baseline, sig)
                    want = _loop(se, me, listed, age, baseline, sig)
                    assert got.shape == (len(listed), me.cin + 1)
                    assert got.dtype == torch.float32
                    torch.testing.assert_close(got, want, rtol=TOL, atol=TOL)
        # column 0 is the plain score of the latest window
        got = se.attribute_latest(me, None, age_t, baseline, True)
        plain = me.forward(se.windows(batch=1), age_t, apply_sigmoid=True)
        torch.testing.assert_close(got[:, :1], plain, rtol=TOL, atol=TOL)
        # and an occluded channel moves the score
        assert not torch.equal(got[:, 1:], got[:, :1].expand(-1, me.cin))

    def test_default_baseline_is_hold(self, engines):
        me = engines["MyCNN5"]
        se = _ring(10, seed=5)
        assert torch.equal(se.attribute_latest(me, [1]),
                           se.attribute_latest(me, [1], baseline="hold"))
        assert not torch.equal(se.attribute_latest(me, [1]),
                               se.attribute_latest(me, [1], baseline="zero"))

    def test_structure(self, engines):
        """A channel that already is the baseline is not changed by its
        occlusion: that column equals column 0 bit for bit, and no other."""
        me = engines["MyCNN5"]
        se = _ring(10, seed=23)
        idx = _window_slots(NPROC)
        se.proc[:, 3, idx] = se.proc[:, 3, idx[0]].unsqueeze(-1)  # flat
        hold = se.attribute_latest(me, None, baseline="hold")
        same = [k for k in range(1, 11)
                if torch.equal(hold[:, k], hold[:, 0])]
        assert same == [4]
        se.proc[:, 6, :] = 0.0
        zero = se.attribute_latest(me, None, baseline="zero")
        assert torch.equal(zero[:, 7], zero[:, 0])
        assert not torch.equal(zero[:, 4], zero[:, 0])

    def test_refusals(self, engines):
        me = engines["MyCNN5"]
        se = _ring(10, seed=29)
        for bad in ([-1], [S], [0, S]):
            with pytest.raises(ValueError, match="out of range"):
                se.attribute_latest(me, bad)
        with pytest.raises(ValueError, match="baseline"):
            se.attribute_latest(me, [0], baseline="mean")
        se.nproc = 60
        with pytest.raises(ValueError, match="no full model window"):
            se.attribute_latest(me, [0])
        se.nproc = NPROC
        assert se.attribute_latest(me, []).shape == (0, 11)


# ---------------------------------------------------------------- the daemon
N_TRIGGERS = 17              # nproc = 12 m - 38: scored from trigger 14 on
PIDS = ("p000501", "p000502")
PLAIN = re.compile(rb'^\{"t_us": \d+, "risk": \d\.\d{6}\}$')


def run_daemon(tmp_path, tag, device="cpu", **kw):
    """Two patients stream one sample per 5 s on every named channel (a
    600-s sawtooth in [-1, 1.3], shifted per channel, so that the 180-s means
    have a course), one trigger per stream-minute. Returns (server, [(trigger, response
    payloads, attribution of both slots by a direct engine call)])."""
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
                      response_topic="risk", **kw)
    reader = Consumer(bus, starting="earliest")
    reader.subscribe(["risk"])
    age = torch.full((4, 1), 65.0, device=device)
    log = []
    for m in range(N_TRIGGERS):
        for step in range(12):
            t = m * 60 + step * 5
            for i, pid in enumerate(PIDS):
                for ch in range(cfg.n_channels):
                    prod.produce(topics[ch], pid, json.dumps(
                        [ch, ((t // 5 + 11 * ch) % 120) / 60.0 - 1.0 + 0.3 * i]),
                        ts_us=int(t * 1e6))
        srv.trigger()
        msgs = reader.poll(max_msgs=64, timeout_ms=0)
        direct = None
        if srv.se.nproc >= L:
            direct = srv.se.attribute_latest(
                srv.me, [srv.pid_index[p] for p in PIDS], age,
                kw.get("explain_baseline", "hold"), True)
        log.append((m + 1, [(x.key.decode(), x.value) for x in msgs],
                    direct))
    return srv, log


class TestDaemon:
    @pytest.mark.parametrize("baseline", ["hold", "zero"])
    def test_every_response_is_explained_at_zero(self, tmp_path, baseline):
        srv, log = run_daemon(tmp_path, baseline, explain_above=0.0,
                              explain_baseline=baseline)
        nc = srv.cfg.n_channels
        n = 0
        for _m, msgs, direct in log:
            for key, value in msgs:
                doc = json.loads(value)
                assert sorted(doc) == ["attribution", "risk", "t_us"]
                att = doc["attribution"]
                assert att["baseline"] == baseline
                row = direct[PIDS.index(key)]
                assert doc["risk"] == float(f"{float(row[0]):.6f}")
                want = [float(f"{float(row[0] - row[c + 1]):.6f}")
                        for c in range(nc)]
                assert att["delta"] == want
                n += 1
        assert n == 2 * (N_TRIGGERS - 13) > 0
        # not vacuous: occluding a channel moves the published score
        assert max(abs(d) for _m, msgs, _d in log for _k, v in msgs
                   for d in json.loads(v)["attribution"]["delta"]) > 1e-4
        assert srv.timer.gauges["explained_total"] == n
        assert type(srv.timer.gauges["explained_total"]) is int
        assert (f'tskd_streams{{stage="serve",state="explained_total"}} {n}'
                in prometheus_text([srv.timer]))
        assert srv.store.count() == n       # the store schema is unchanged

    def test_nothing_is_explained_above_one(self, tmp_path):
        srv, log = run_daemon(tmp_path, "high", explain_above=1.1)
        payloads = [v for _m, msgs, _d in log for _k, v in msgs]
        assert payloads and all(PLAIN.match(v) for v in payloads)
        assert "explained_total" not in srv.timer.gauges

    def test_threshold_selects_by_risk(self, tmp_path):
        _srv, log = run_daemon(tmp_path, "all", explain_above=0.0)
        risks = sorted(json.loads(v)["risk"]
                       for _m, msgs, _d in log for _k, v in msgs)
        assert risks[0] < risks[-1]
        R = (risks[0] + risks[-1]) / 2
        srv, log = run_daemon(tmp_path, "some", explain_above=R)
        docs = [json.loads(v) for _m, msgs, _d in log for _k, v in msgs]
        assert all(("attribution" in d) == (d["risk"] >= R) for d in docs)
        n = sum("attribution" in d for d in docs)
        assert 0 < n < len(docs)
        assert srv.timer.gauges["explained_total"] == n

    def test_off_is_byte_identical(self, tmp_path):
        a, plain = run_daemon(tmp_path, "plain")
        b, off = run_daemon(tmp_path, "off", explain_above=None)
        _c, on = run_daemon(tmp_path, "on", explain_above=0.0)
        strip = [(m, msgs) for m, msgs, _d in plain]
        assert strip == [(m, msgs) for m, msgs, _d in off]
        payloads = [v for _m, msgs in strip for _k, v in msgs]
        assert payloads and all(PLAIN.match(v) for v in payloads)
        assert "explained_total" not in a.timer.gauges
        assert "explained_total" not in b.timer.gauges
        # the flag adds to a response and changes nothing else of it
        cut = re.compile(rb', "attribution": \{[^}]*\}')
        assert [(m, [(k, cut.sub(b"", v)) for k, v in msgs])
                for m, msgs, _d in on] == strip

    def test_without_a_response_topic_it_only_counts(self, tmp_path):
        srv, _log = run_daemon(tmp_path, "count", explain_above=0.0)
        srv.response_topic = None
        before = srv.timer.gauges["explained_total"]
        probs = torch.tensor([0.25, 0.75])
        srv._persist(probs, 1, list(PIDS))
        assert srv.timer.gauges["explained_total"] == before + 2

    def test_arguments(self, tmp_path):
        from tskd_amd.cli import serve
        with pytest.raises(SystemExit):
            serve.main(["--explain-above", "0.5", "--pipelined"])
        with pytest.raises(SystemExit):
            serve.main(["--explain-above", "0.5", "--explain-baseline",
                        "mean"])
        with pytest.raises(ValueError, match="pipelined"):
            run_daemon(tmp_path, "pipe", explain_above=0.5, pipelined=True)
        with pytest.raises(ValueError, match="explain_baseline"):
            run_daemon(tmp_path, "mean", explain_above=0.5,
                       explain_baseline="mean")

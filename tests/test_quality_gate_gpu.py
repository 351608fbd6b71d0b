"""Signal-quality gate on the GPU: the gated instantiations of
ingest_dense_kernel<bf16|fp32> and ingest_events_kernel
(csrc/preprocess_kernels.hip) against the numpy oracle of
tests/test_quality_gate.py with ``==`` — sums, counts and the rejected
counter — over the launch sweep of tests/test_ingest_exact.py, then the gate
switched off against the ungated entry point, the GPU engine against the CPU
engine, and a captured trigger against its eager twin.

Every dense launch runs on sentinel-prefilled rings through
``StreamEngine._launch_ingest`` of a gated engine, on a misaligned view whose
slack holds ±2**20 and NaN: in range for the open and one-sided intervals,
out of range for the others, so a sample read from outside a bucket shows in
the sum, the count or the rejected counter.
"""
import numpy as np
import pytest
import torch

from test_ingest_exact import (C, G, MAXABS, OFFSETS, SENT, SLACK, TORCH_DT,
                               dense_cases, event_rings, heads_for, place)
from test_ingest_exact import EC as XC
from test_ingest_exact import EG as XG
from test_ingest_exact import ES as XS
from test_quality_gate import (BOUNDS, OPEN, bounds_array, chan_map_for,
                               check_daemon, events_gate_oracle,
                               expected_gated, gated_events, gen_gated_raw,
                               numerics, run_daemon, same)
from tskd_amd.engine import StreamEngine
from tskd_amd.ops import hip

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("packed", [True, False],
                                  ids=["packed", "split"])
DTYPES = pytest.mark.parametrize("dt", ["bf16", "fp32"])


class GatedRings:
    """SENT-prefilled gated GPU engines of one layout, one per (S,
    bucket_len); the rejected counter starts every launch at ``rej0``."""

    def __init__(self, monkeypatch, packed, valid_range=BOUNDS):
        monkeypatch.setenv("TSKD_PACKED_BUCKETS", "1" if packed else "0")
        self.packed, self.cache, self.vr = packed, {}, valid_range

    def engine(self, S, bl, rej0=0):
        eng = self.cache.get((S, bl))
        if eng is None:
            eng = self.cache[(S, bl)] = StreamEngine(
                S, C, ring_grid=G, fs=bl / 5.0, device="cuda",
                valid_range=self.vr)
            assert eng.bucket_len == bl and eng._packed == self.packed
            assert eng.rej.is_cuda and eng.bounds.is_cuda
        if self.packed:
            eng._bkt.fill_(SENT)
        else:
            eng.bsum.fill_(SENT)
            eng.bcnt.fill_(SENT)
        eng.rej.fill_(rej0)
        eng.head = eng.nproc = 0
        return eng

    def launch_and_check(self, raw_f64, bl, off, dt, head, cm, note, rej0=0):
        S = raw_f64.shape[0]
        eng = self.engine(S, bl, rej0)
        buf, view = place(raw_f64, off, dt)
        eng.head = head
        eng._launch_ingest(view, cm)
        got_s, got_c, got_r = eng.bsum.cpu(), eng.bcnt.cpu(), eng.rej.cpu()
        es, ec, er = expected_gated(S, raw_f64, bl, head, cm,
                                    valid_range=self.vr)
        assert same(got_s, es), f"bsum {note}"
        assert same(got_c, ec), f"bcnt {note}"
        # unmapped channels: er is 0 there, the counter still rej0
        assert torch.equal(got_r, er + rej0), \
            f"rej {note}: {got_r.tolist()} != {(er + rej0).tolist()}"
        return er


@LAYOUTS
@DTYPES
def test_dense_sweep_exact(packed, dt, monkeypatch):
    """Every bucket length x NB x tail of dense_cases(): written slots and
    the rejected counter == the oracle, every other ring element still the
    sentinel, the counter of unmapped channels untouched."""
    rings = GatedRings(monkeypatch, packed)
    bad, n_rej, seen = [], 0, set()
    for k in dense_cases():
        rng = np.random.default_rng(3000 + k["seed"])
        x = gen_gated_raw(rng, k["S"], k["CIN"], k["T"], k["bl"], MAXABS[dt])
        cm = chan_map_for(k)
        seen.update(cm)
        try:
            n_rej += int(rings.launch_and_check(
                x, k["bl"], k["off"], dt,
                heads_for(k["nb"])[k["head_kind"]], cm, k, rej0=5).sum())
        except AssertionError as e:     # go on: name every failing shape
            bad.append(str(e).splitlines()[0])
    assert not bad, f"{len(bad)} launches differ:\n" + "\n".join(bad[:20])
    assert seen == set(range(C)) and n_rej > 1000


@LAYOUTS
@DTYPES
def test_short_final_bucket_after_a_rejected_sample(packed, dt, monkeypatch):
    """One-row tensors whose final bucket sits ``mis`` elements into its
    16 B chunk, with and without ``mis + bucket_len < 8``, every sample of the
    final bucket in range and the sample right before it out of range: a
    scalar tail that started before the bucket would count that sample a
    second time. Channel 3 is [-7, 100]."""
    rings = GatedRings(monkeypatch, packed)
    seen = set()
    for off in OFFSETS:
        for bl, T in ((5, 15), (1, 3), (5, 5), (7, 17), (5, 10)):
            rng = np.random.default_rng(177 + off + bl)
            nb = T // bl
            x = rng.integers(1, 101, size=(1, 1, T)).astype(np.float64)
            x[0, 0, :(nb - 1) * bl] = -200.0      # all rejected, last too
            x[0, 0, nb * bl:] = 200.0             # trailing: in no bucket
            mis = (SLACK + off + (nb - 1) * bl) % 8
            seen.add(mis + bl < 8)
            er = rings.launch_and_check(x, bl, off, dt, 5, [3],
                                        (off, bl, T, mis))
            assert er[0, 3] == (nb - 1) * bl
    assert seen == {True, False}


@LAYOUTS
@DTYPES
def test_two_launches_accumulate(packed, dt, monkeypatch):
    monkeypatch.setenv("TSKD_PACKED_BUCKETS", "1" if packed else "0")
    eng = StreamEngine(2, C, ring_grid=G, fs=9 / 5.0, device="cuda",
                       valid_range=BOUNDS)
    rng = np.random.default_rng(55)
    total = torch.zeros(2, C, dtype=torch.int64)
    for cm, head in (([3, 0, 4], 3), ([1, 3, 2], G - 2)):
        x = gen_gated_raw(rng, 2, 3, 5 * 9 + 3, 9, MAXABS[dt])
        _buf, view = place(x, 3, dt)
        eng.head = head
        eng._launch_ingest(view, cm)
        total += expected_gated(2, x, 9, head, cm)[2]
        assert torch.equal(eng.rejected().cpu(), total)
    assert total[:, 3].min() > 0 and total[:, 4].min() > 0
    assert torch.equal(eng.rejected([1, 1, 0]).cpu(), total[[1, 1, 0]])
    eng.reset_streams([1])
    total[1] = 0
    assert torch.equal(eng.rejected().cpu(), total)


@LAYOUTS
@DTYPES
def test_open_bounds_equal_the_ungated_entry_point(packed, dt, monkeypatch):
    """All-open bounds: the gated kernels write the rings of the ungated
    entry point bit for bit (NaN sums of +inf and -inf included), on the
    same raw tensor, and reject nothing."""
    monkeypatch.setenv("TSKD_PACKED_BUCKETS", "1" if packed else "0")
    for k in [k for k in dense_cases() if k["seed"] % 6 == 0]:
        rng = np.random.default_rng(5000 + k["seed"])
        x = gen_gated_raw(rng, k["S"], k["CIN"], k["T"], k["bl"], MAXABS[dt])
        _buf, view = place(x, k["off"], dt)
        cm = chan_map_for(k)
        engines = []
        for vr in (None, OPEN):
            eng = StreamEngine(k["S"], C, ring_grid=G, fs=k["bl"] / 5.0,
                               device="cuda", valid_range=vr)
            eng.bsum.fill_(SENT)
            eng.bcnt.fill_(SENT)
            eng.head = heads_for(k["nb"])[k["head_kind"]]
            eng._launch_ingest(view, cm)
            engines.append(eng)
        plain, gated = engines
        assert plain.rej is None
        for name in ("bsum", "bcnt"):
            a = getattr(plain, name).contiguous().view(torch.int32)
            b = getattr(gated, name).contiguous().view(torch.int32)
            assert torch.equal(a, b), (name, k)
        assert (gated.rejected() == 0).all(), k


def launch_events_gated(si, ci, bi, vi, bsum, bcnt, bst, min_bucket, bounds,
                        rej):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
           for a in (si.astype(np.int32), ci.astype(np.int32),
                     bi.astype(np.int64), vi.astype(np.float32))]
    hip.check(hip.load(hip.PREPROC).tskd_preproc_ingest_events_gated(
        *(hip.ptr(t) for t in dev), hip.ptr(bsum), hip.ptr(bcnt), XC, XG,
        len(vi), min_bucket, bst, hip.ptr(bounds), hip.ptr(rej),
        hip.stream_ptr()), "tskd_preproc_ingest_events_gated")
    torch.cuda.synchronize()


@LAYOUTS
def test_events_exact(packed):
    """A few hundred integer-valued events, many per bucket, late ones
    included, accumulate ONTO the sentinel; a second launch adds to the
    counter. XC = 4 channels: the first four intervals of BOUNDS."""
    vr = BOUNDS[:3] + [BOUNDS[3]]
    assert XC == 4
    rng = np.random.default_rng(8)
    min_bucket = 75
    si, ci, bi, vi = gated_events(rng, 800, XS, XC, XG // 4, min_bucket)
    assert (bi < min_bucket).sum() >= 40
    bsum, bcnt, bst = event_rings(packed, SENT)
    bounds = torch.from_numpy(bounds_array(vr)).float().cuda()
    rej = torch.zeros(XS, XC, dtype=torch.int64, device="cuda")
    launch_events_gated(si, ci, bi, vi, bsum, bcnt, bst, min_bucket, bounds,
                        rej)
    es, ec, er = events_gate_oracle(si, ci, bi, vi, min_bucket, XS, XC, XG,
                                    SENT, vr)
    assert same(bsum.cpu(), es) and torch.equal(bcnt.cpu(), ec)
    assert torch.equal(rej.cpu(), er)
    assert er[:, 3].min() > 0 and er[:, 0].sum() == 0
    # only late events: nothing moves; none at all: nothing launches
    launch_events_gated(si[:40], ci[:40], bi[:40], vi[:40], bsum, bcnt, bst,
                        min_bucket, bounds, rej)
    empty = np.zeros(0)
    launch_events_gated(empty, empty, empty, empty, bsum, bcnt, bst, 0,
                        bounds, rej)
    assert torch.equal(rej.cpu(), er) and same(bsum.cpu(), es)
    # a null bounds or counter pointer is refused by the launcher
    lib = hip.load(hip.PREPROC)
    assert lib.tskd_preproc_ingest_events_gated(
        None, None, None, None, hip.ptr(bsum), hip.ptr(bcnt), XC, XG, 0, 0,
        bst, None, hip.ptr(rej), hip.stream_ptr()) == -4


def _dense_raw(S, CIN, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(S, CIN, T)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = np.nan
    return torch.from_numpy(x)


TEN = [(-1.0, 1.0), (None, 0.5), (-0.25, None), (0.0, 0.0)] + \
    [(-1.5, 2.0)] * 4 + [(None, None)] * 2


def test_gpu_engine_matches_cpu_engine():
    """The same gated input through both engines: the counters are equal,
    the processed points agree at the tolerance tests/test_engine.py uses for
    GPU against CPU (dense fp32: rtol 1e-4, atol 1e-5; events: rtol 1e-3,
    atol 1e-4)."""
    S, fs = 3, 25.0
    raw = _dense_raw(S, 8, int(fs * 60 * 6), seed=11)
    cpu = StreamEngine(S, 10, ring_grid=256, fs=fs, valid_range=TEN)
    gpu = StreamEngine(S, 10, ring_grid=256, fs=fs, device="cuda",
                       valid_range=TEN)
    cm = list(range(8))
    for lo in range(0, raw.shape[2], int(fs * 60)):
        chunk = raw[:, :, lo:lo + int(fs * 60)]
        cpu.ingest_dense(chunk, chan_map=cm)
        gpu.ingest_dense(chunk.cuda(), chan_map=cm)
    assert gpu.nproc == cpu.nproc > 30
    assert torch.equal(gpu.rejected().cpu(), cpu.rejected())
    assert cpu.rejected()[:, :8].min() > 0 and \
        (cpu.rejected()[:, 8:] == 0).all()
    np.testing.assert_allclose(gpu.bcnt.cpu().numpy(), cpu.bcnt.numpy())
    np.testing.assert_allclose(
        gpu.proc[:, :, :gpu.nproc].cpu().numpy(),
        cpu.proc[:, :, :cpu.nproc].numpy(), rtol=1e-4, atol=1e-5)
    # events
    rng = np.random.default_rng(17)
    n = 3000
    args = (torch.from_numpy(rng.integers(0, 2, n)),
            torch.from_numpy(rng.integers(0, 4, n)),
            torch.from_numpy(rng.uniform(0, 1000, n)),
            torch.from_numpy(rng.normal(size=n).astype(np.float32)))
    cpu = StreamEngine(2, 10, ring_grid=512, valid_range=TEN)
    gpu = StreamEngine(2, 10, ring_grid=512, device="cuda", valid_range=TEN)
    for e in (cpu, gpu):
        e.ingest_events(*args, advance_to=600)
        e.ingest_events(*args, advance_to=1000)     # half of it late now
    assert gpu.nproc == cpu.nproc
    assert torch.equal(gpu.rejected().cpu(), cpu.rejected())
    assert cpu.rejected()[:, :4].min() > 0
    np.testing.assert_allclose(
        gpu.proc[:, :, :gpu.nproc].cpu().numpy(),
        cpu.proc[:, :, :cpu.nproc].numpy(), rtol=1e-3, atol=1e-4)


def test_trigger_graph_on_a_gated_engine_matches_eager():
    """The captured trigger of a gated engine (S = 4, G = 144: the replays
    cross the ring's end) against an eager twin fed the same chunks: scores,
    rings and the rejected counter."""
    from tskd_amd.engine.stream_engine import TriggerGraph
    from tskd_amd.models import build_model
    from tskd_amd.ops import GraphedForward, MyCNNEngine
    fs, S, Gr = 25.0, 4, 144
    torch.manual_seed(6)
    me = MyCNNEngine(build_model("MyCNN5").eval(), device="cuda")
    n_triggers = 16
    chunks = [_dense_raw(S, 8, int(fs * 60), seed=100 + i).cuda()
              .to(torch.bfloat16) for i in range(n_triggers)]
    cm = list(range(8))
    e1 = StreamEngine(S, 10, ring_grid=Gr, fs=fs, device="cuda",
                      valid_range=TEN)
    eager = []
    for ch in chunks:
        e1.ingest_dense(ch, chan_map=cm)
        w = e1.windows(batch=1, stride=12, dtype=torch.bfloat16)
        eager.append(me.forward(w, None, apply_sigmoid=True).clone())
    e2 = StreamEngine(S, 10, ring_grid=Gr, fs=fs, device="cuda",
                      valid_range=TEN)
    raw_buf = chunks[0].clone()
    idx = 0
    while e2.head < 120:
        raw_buf.copy_(chunks[idx])
        e2.ingest_dense(raw_buf, chan_map=cm)
        idx += 1
    torch.cuda.synchronize()
    gf = GraphedForward(me, s=S, n=1, dtype=torch.bfloat16, timelast=True)
    gf.age.zero_()
    raw_buf.copy_(chunks[idx])
    tg = TriggerGraph(e2, raw_buf, cm, gf, stride=12)
    idx += 1
    assert e2.head < Gr
    while idx < n_triggers:
        raw_buf.copy_(chunks[idx])
        out = tg.replay()
        torch.cuda.synchronize()
        torch.testing.assert_close(out, eager[idx], rtol=2e-3, atol=2e-3)
        idx += 1
    assert e2.head == e1.head > Gr and e2.nproc == e1.nproc
    assert torch.equal(e2.rejected(), e1.rejected())
    assert e1.rejected()[:, :8].min() > 100
    assert torch.equal(e2.bcnt, e1.bcnt) and same(e2.proc.cpu(),
                                                  e1.proc.cpu())


def test_daemon_on_the_gpu(tmp_path):
    """The CPU suite's gated daemon run on the GPU engine."""
    srv, zeros, log = run_daemon(tmp_path, "gpu", device="cuda",
                                 valid_range=numerics())
    check_daemon(srv, zeros, log)

"""Signal-quality gate (docs/PARITY.md divergence 15): per-wire-channel
plausibility bounds at ingest, the cumulative rejected counter, the
configuration syntax and the serving daemon built on them. CPU tests.

The dense and event inputs follow tests/test_ingest_exact.py (nonzero
integers, ~15 % NaN, so every sum is exact in fp32 in any order) with a few
±inf added; the oracle is plain numpy and every comparison is ``==``. The
oracle, the bounds and the case builders are shared with
tests/test_quality_gate_gpu.py.
"""
import json
import os

import numpy as np
import pytest
import torch

from test_ingest_exact import (C, G, MAXABS, SENT, TORCH_DT, dense_cases,
                               gen_raw, heads_for)
from tskd_amd.bus import Bus, Consumer, Producer
from tskd_amd.config import (DEFAULT_CHANNEL_NAMES, get_global_config,
                             parse_valid_ranges, resolve_valid_ranges)
from tskd_amd.engine import StreamEngine
from tskd_amd.metrics import prometheus_text

INF = float("inf")

# One interval per wire channel of the C = 5 test engines, every bound exact
# in bf16: open, one-sided below, one-sided above, bounds that ARE sample
# values (the generator is made to emit -7 and 100: inclusivity), and one
# that accepts nothing (no sample is 0.5).
BOUNDS = [(None, None), (-20.0, None), (None, 50.0), (-7.0, 100.0),
          (0.5, 0.5)]
OPEN = [(None, None)] * C
# non-identity injections into C; a case takes one by its seed, so that every
# interval meets both row counts of the sweep
GATE_CHAN_MAPS = {1: ([3], [1], [4], [0], [2]),
                  3: ([3, 0, 4], [1, 3, 2], [4, 2, 0], [2, 1, 3])}


def bounds_array(valid_range=BOUNDS):
    """(C, 2) float64 [lo, hi] with ±inf for the open sides."""
    return np.array([[-INF if lo is None else lo, INF if hi is None else hi]
                     for lo, hi in valid_range], dtype=np.float64)


def chan_map_for(k):
    maps = GATE_CHAN_MAPS[k["CIN"]]
    return list(maps[k["seed"] % len(maps)])


def gen_gated_raw(rng, S, CIN, T, bl, maxabs):
    """gen_raw plus the gate's edge values: samples equal to the inclusive
    interval's bounds (-7, 100), a few ±inf, and — when the row has more than
    one bucket — an out-of-range sample (maxabs is above every finite hi and
    below every finite lo once negated) as the LAST sample of the bucket
    before the final one and as the first trailing sample."""
    x, _ = gen_raw(rng, S, CIN, T, bl, maxabs)
    flat = x.reshape(-1)
    n = flat.size
    for val, share in ((-7.0, 0.04), (100.0, 0.04), (INF, 0.01),
                       (-INF, 0.01)):
        flat[rng.random(n) < share] = val
    nb = T // bl
    for s in range(S):
        for r in range(CIN):
            if nb > 1:
                x[s, r, (nb - 1) * bl - 1] = -float(maxabs)
            if T > nb * bl:
                x[s, r, nb * bl] = float(maxabs)
    return x


def gate_oracle(raw_f64, bucket_len, chan_map, valid_range=BOUNDS):
    """(sum float64, cnt int64, rej int64), each (S, CIN, NB): per whole
    bucket the sum and the number of accepted samples (lo <= v <= hi, false
    for NaN) and the number of rejected ones (not accepted and not NaN).
    Trailing T % bucket_len samples belong to no bucket."""
    S, CIN, T = raw_f64.shape
    nb = T // bucket_len
    bnd = bounds_array(valid_range)[list(chan_map)]
    lo, hi = bnd[None, :, 0, None], bnd[None, :, 1, None]
    osum = np.zeros((S, CIN, nb))
    ocnt = np.zeros((S, CIN, nb), dtype=np.int64)
    orej = np.zeros((S, CIN, nb), dtype=np.int64)
    for b in range(nb):
        seg = raw_f64[:, :, b * bucket_len:(b + 1) * bucket_len]
        with np.errstate(invalid="ignore"):
            acc = (lo <= seg) & (seg <= hi)
            osum[:, :, b] = np.where(acc, seg, 0.0).sum(-1)   # inf - inf
        ocnt[:, :, b] = acc.sum(-1)
        orej[:, :, b] = (~acc & ~np.isnan(seg)).sum(-1)
    return osum, ocnt, orej


def expected_gated(S, raw_f64, bucket_len, head, chan_map, unmapped=SENT,
                   valid_range=BOUNDS):
    """fp32 (S, C, G) sum and count rings after one gated dense launch on
    SENT-prefilled rings (as test_ingest_exact.expected_rings) and the int64
    (S, C) rejected counts the launch adds."""
    osum, ocnt, orej = gate_oracle(raw_f64, bucket_len, chan_map, valid_range)
    slots = (head + np.arange(osum.shape[-1])) % G
    es = np.full((S, C, G), SENT, dtype=np.float64)
    ec = np.full((S, C, G), SENT, dtype=np.float64)
    es[:, :, slots] = unmapped
    ec[:, :, slots] = unmapped
    rej = np.zeros((S, C), dtype=np.int64)
    for ci, c in enumerate(chan_map):
        es[:, c, slots] = osum[:, ci]
        ec[:, c, slots] = ocnt[:, ci]
        rej[:, c] = orej[:, ci].sum(-1)
    return (torch.from_numpy(es).to(torch.float32),
            torch.from_numpy(ec).to(torch.float32), torch.from_numpy(rej))


def gated_events(rng, n, ES, EC, EG, min_bucket):
    """Integer-valued events with many duplicates per bucket over ~2 ring
    turns, ~10 % NaN, a few ±inf, some late (bucket < min_bucket)."""
    si = rng.integers(0, ES, size=n)
    ci = rng.integers(0, EC, size=n)
    bi = rng.integers(min_bucket - 6, min_bucket + 2 * EG, size=n)
    vi = rng.integers(-60, 121, size=n).astype(np.float64)
    vi[vi == 0] = 3.0
    vi[rng.random(n) < 0.1] = np.nan
    vi[rng.random(n) < 0.02] = INF
    vi[rng.random(n) < 0.02] = -INF
    vi[rng.random(n) < 0.05] = -7.0
    vi[rng.random(n) < 0.05] = 100.0
    bi[:40] = min_bucket - 1        # late AND (mostly) out of range
    vi[:40:2] = 4000.0
    return si, ci, bi, vi


def events_gate_oracle(si, ci, bi, vi, min_bucket, ES, EC, EG, fill,
                       valid_range):
    """(sum, cnt) fp32 rings starting from ``fill`` and int64 (ES, EC)
    rejected counts: late drop first, then the gate."""
    bnd = bounds_array(valid_range)[ci]
    live = bi >= min_bucket
    with np.errstate(invalid="ignore"):
        acc = (bnd[:, 0] <= vi) & (vi <= bnd[:, 1])
    keep = live & acc
    out = live & ~acc & ~np.isnan(vi)
    es = np.full((ES, EC, EG), fill, dtype=np.float64)
    ec = np.full((ES, EC, EG), fill, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        np.add.at(es, (si[keep], ci[keep], bi[keep] % EG), vi[keep])
    np.add.at(ec, (si[keep], ci[keep], bi[keep] % EG), 1.0)
    rej = np.zeros((ES, EC), dtype=np.int64)
    np.add.at(rej, (si[out], ci[out]), 1)
    return (torch.from_numpy(es).to(torch.float32),
            torch.from_numpy(ec).to(torch.float32), torch.from_numpy(rej))


def same(got, exp):
    nan = torch.isnan(exp)
    return torch.equal(torch.isnan(got), nan) and \
        torch.equal(got[~nan], exp[~nan])


# ------------------------------------------------------------ oracle itself
def test_oracle_and_generator():
    y = np.array([[[1.0, -7.0, 100.0, np.nan, 101.0, -8.0, INF, 5.0]]])
    s, c, r = gate_oracle(y, 4, [3])            # [-7, 100], inclusive
    assert s.tolist() == [[[94.0, 5.0]]]
    assert c.tolist() == [[[3, 1]]] and r.tolist() == [[[0, 3]]]
    s, c, r = gate_oracle(y, 4, [0])            # open: all but the NaN
    assert c.tolist() == [[[3, 4]]] and r.sum() == 0 and s[0, 0, 1] == INF
    s, c, r = gate_oracle(y, 4, [4])            # accepts nothing
    assert c.sum() == 0 and s.sum() == 0 and r.tolist() == [[[3, 4]]]
    s, c, r = gate_oracle(y, 4, [1])            # [-20, +inf]
    assert c.tolist() == [[[3, 4]]] and r.sum() == 0
    s, c, r = gate_oracle(y, 4, [2])            # [-inf, 50]
    assert c.tolist() == [[[2, 2]]] and r.tolist() == [[[1, 2]]]
    rng = np.random.default_rng(3)
    x = gen_gated_raw(rng, 2, 3, 6 * 9 + 3, 9, MAXABS["bf16"])
    ok = ~np.isnan(x)
    assert (x[ok] != 0).all() and 0.05 < 1 - ok.mean() < 0.5
    assert (x == -7).any() and (x == 100).any()
    assert np.isinf(x).sum() >= 2
    xt = torch.from_numpy(x[ok]).to(torch.bfloat16).double().numpy()
    assert (xt == x[ok]).all()                  # exact in bf16
    b = bounds_array()
    assert (torch.from_numpy(b).to(torch.bfloat16).double().numpy()
            == b).all()
    # every interval, both row counts
    for cin, maps in GATE_CHAN_MAPS.items():
        assert {c for m in maps for c in m} == set(range(C))
        assert all(len(m) == cin == len(set(m)) for m in maps)


# ------------------------------------------------------- CPU engine: dense
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_cpu_dense_matches_oracle(dt):
    cases = [k for k in dense_cases() if k["seed"] % 5 == 0]
    assert {k["bl"] for k in cases} >= {1, 5, 625} and len(cases) >= 20
    seen = set()
    for k in cases:
        rng = np.random.default_rng(3000 + k["seed"])
        x = gen_gated_raw(rng, k["S"], k["CIN"], k["T"], k["bl"], MAXABS[dt])
        eng = StreamEngine(k["S"], C, ring_grid=G, fs=k["bl"] / 5.0,
                           valid_range=BOUNDS)
        assert eng.rej.dtype == torch.int64 and eng.rej.shape == (k["S"], C)
        eng.bsum.fill_(SENT)
        eng.bcnt.fill_(SENT)
        eng._warned_partial = True
        eng.head = head = heads_for(k["nb"])[k["head_kind"]]
        cm = chan_map_for(k)
        seen.update(cm)
        assert eng.ingest_dense(torch.from_numpy(x).to(TORCH_DT[dt]),
                                chan_map=cm) == k["nb"]
        es, ec, er = expected_gated(k["S"], x, k["bl"], head, cm,
                                    unmapped=0.0)
        assert same(eng.bsum, es) and torch.equal(eng.bcnt, ec), k
        assert torch.equal(eng.rejected(), er), k
    assert seen == set(range(C))


def test_cpu_dense_accumulates_over_launches():
    rng = np.random.default_rng(11)
    eng = StreamEngine(2, C, ring_grid=G, fs=1.0, valid_range=BOUNDS)
    total = torch.zeros(2, C, dtype=torch.int64)
    for cm in ([3, 0, 4], [1, 3, 2]):
        x = gen_gated_raw(rng, 2, 3, 4 * 5, 5, 256)
        head = eng.head
        eng.ingest_dense(torch.from_numpy(x).float(), chan_map=cm)
        total += expected_gated(2, x, 5, head, cm)[2]
        assert torch.equal(eng.rejected(), total)
    assert total[:, 3].min() > 0 and (total[:, 0] == 0).all()


# ------------------------------------------------------ CPU engine: events
ES, EC, EG = 3, 5, 64


def _event_engine(valid_range, device="cpu"):
    return StreamEngine(ES, EC, ring_grid=EG, win_buckets=4, model_win=8,
                        device=device, valid_range=valid_range)


def feed_events(eng, si, ci, bi, vi):
    """Events by BUCKET (timestamp = mid-bucket), no watermark advance
    beyond the engine's current head."""
    eng.ingest_events(torch.from_numpy(si).long(), torch.from_numpy(ci).long(),
                      torch.from_numpy((bi + 0.5) * eng.bucket_s),
                      torch.from_numpy(vi.astype(np.float32)),
                      advance_to=eng.head * eng.bucket_s)


def test_cpu_events_match_oracle_and_late_is_not_rejected():
    rng = np.random.default_rng(21)
    eng = _event_engine(BOUNDS)
    # move the processed grid to 9: buckets below it are late
    eng.advance_watermark(12 * eng.bucket_s)
    assert eng.nproc == 9
    si, ci, bi, vi = gated_events(rng, 900, ES, EC, 20, eng.nproc)
    assert bi.max() - eng.nproc < EG - eng.win_buckets
    assert (bi < eng.nproc).sum() > 40
    feed_events(eng, si, ci, bi, vi)
    es, ec, er = events_gate_oracle(si, ci, bi, vi, 9, ES, EC, EG, 0.0,
                                    BOUNDS)
    assert same(eng.bsum, es) and torch.equal(eng.bcnt, ec)
    assert torch.equal(eng.rejected(), er)
    assert er[:, 3].min() > 0 and er[:, 0].sum() == 0
    # the 20 late events of 4000.0 would have been rejected on any bounded
    # channel had they not been late: count them as live and it shows
    _s, _c, er_live = events_gate_oracle(si, ci, np.maximum(bi, 9), vi, 9,
                                         ES, EC, EG, 0.0, BOUNDS)
    assert er_live.sum() > er.sum()
    # a batch of late events only: nothing moves
    before = eng.rejected()
    feed_events(eng, si[:40], ci[:40], bi[:40], vi[:40])
    assert torch.equal(eng.rejected(), before)


# --------------------------------------------------------------- gate off
@pytest.mark.parametrize("path", ["dense", "events"])
def test_open_bounds_equal_no_gate(path):
    rng = np.random.default_rng(31)
    if path == "dense":
        a = StreamEngine(2, C, ring_grid=G, fs=1.0, win_buckets=4)
        b = StreamEngine(2, C, ring_grid=G, fs=1.0, win_buckets=4,
                         valid_range=OPEN)
        for _ in range(3):
            x = torch.from_numpy(gen_gated_raw(rng, 2, 3, 6 * 5, 5, 4095))
            for e in (a, b):
                e.ingest_dense(x.float(), chan_map=[3, 0, 4])
    else:
        a, b = _event_engine(None), _event_engine(OPEN)
        for e in (a, b):
            e.advance_watermark(12 * e.bucket_s)
        si, ci, bi, vi = gated_events(rng, 600, ES, EC, 20, 9)
        for e in (a, b):
            feed_events(e, si, ci, bi, vi)
            e.advance_watermark(40 * e.bucket_s)
    assert a.rej is None and a.bounds is None
    assert a.nproc == b.nproc > 0
    for name in ("bsum", "bcnt", "proc"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert same(ta, tb), name
        assert torch.equal(torch.isnan(ta), torch.isnan(tb))
    assert torch.isinf(a.bsum).any()        # ±inf went through both
    assert (b.rejected() == 0).all()


# ------------------------------------------------------- reset / refusals
def test_reset_streams_zeroes_the_listed_rows_only():
    eng = StreamEngine(4, C, ring_grid=G, fs=1.0, valid_range=BOUNDS)
    x = np.full((4, 1, 10), 5.0)
    eng.ingest_dense(torch.from_numpy(x).float(), chan_map=[4])
    assert eng.rejected()[:, 4].tolist() == [10] * 4
    eng.reset_streams([2, 0, 2])
    assert eng.rejected()[:, 4].tolist() == [0, 10, 0, 10]
    assert eng.rejected([3, 0, 3])[:, 4].tolist() == [10, 0, 10]
    assert eng.rejected([]).shape == (0, C)
    eng.reset_streams([])
    assert eng.rejected().sum() == 20
    out = eng.rejected()
    out.zero_()                               # a copy, not the counter
    assert eng.rejected().sum() == 20
    for bad in ([4], [-1]):
        with pytest.raises(ValueError):
            eng.rejected(bad)


def test_bad_bounds_and_ungated_engine_raise():
    for bad in (BOUNDS[:4], BOUNDS + [(None, None)],
                [(float("nan"), 1.0)] + BOUNDS[1:],
                [(1.0, float("nan"))] + BOUNDS[1:],
                [(2.0, 1.0)] + BOUNDS[1:], [(1.0,)] + BOUNDS[1:]):
        with pytest.raises(ValueError):
            StreamEngine(1, C, valid_range=bad)
    StreamEngine(1, C, valid_range=[(1.0, 1.0)] * C)    # lo == hi is legal
    with pytest.raises(ValueError, match="no signal-quality gate"):
        StreamEngine(1, C).rejected()


def test_snapshot_does_not_carry_the_counter():
    src = _event_engine(BOUNDS)
    rng = np.random.default_rng(41)
    si, ci, bi, vi = gated_events(rng, 300, ES, EC, 20, 0)
    feed_events(src, si, ci, bi, vi)
    src.advance_watermark(30 * src.bucket_s)
    assert src.rejected().sum() > 0
    snap = src.snapshot()
    assert not any("rej" in k for k in vars(snap))
    # restored under other bounds (here: none at all) or the same: from 0
    plain = _event_engine(None)
    plain.restore(snap)
    assert same(plain.windows(), src.windows())
    again = _event_engine([(None, 10.0)] * EC)
    again.restore(snap)
    assert (again.rejected() == 0).all()


# ------------------------------------------------------------ real record
RECORD_DIR = os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data",
    "waveform", "physionet.org", "files", "mimic3wdb-matched", "1.0", "p00",
    "p000194")
RECORD = os.path.join(RECORD_DIR, "p000194-2112-05-23-14-34n")
# record signal name -> configured channel name
HOUR = 60
NBP = {"NBPSys": "NBP Sys", "NBPDias": "NBP Dias", "NBPMean": "NBP Mean"}


def decode_record():
    """The record decoded independently of the project's reader: format-16
    samples (little-endian int16, signals interleaved), physical = digital /
    gain (baseline 0), -32768 = invalid. Returns (names, (n, nsig) float64
    with NaN for invalid)."""
    with open(RECORD + ".hea", encoding="ascii") as fh:
        lines = [ln.split() for ln in fh if ln.strip() and ln[0] != "#"]
    nsig, nsamp = int(lines[0][1]), int(lines[0][3])
    specs = lines[1:1 + nsig]
    assert all(s[1] == "16" and s[0] == specs[0][0] for s in specs)
    gains = np.array([float(s[2].split("/")[0].split("(")[0])
                      for s in specs])
    d = np.fromfile(os.path.join(RECORD_DIR, specs[0][0]), dtype="<i2")
    d = d[:nsamp * nsig].reshape(nsamp, nsig).astype(np.float64)
    p = d / gains
    p[d == -32768] = np.nan
    return [s[-1] for s in specs], p


@pytest.fixture(scope="module")
def real_record():
    """The record through the project's reader and the event path, into a
    gated (numerics preset) and an ungated CPU engine, one event per sample
    at 60 s spacing, fed an hour (HOUR samples) at a time, on a ring long
    enough that nothing is late."""
    from tskd_amd.io import rdrecord
    rec = rdrecord(RECORD)
    names = [NBP.get(n, n) for n in rec.sig_name]
    wire = [DEFAULT_CHANNEL_NAMES.index(n) for n in names]
    n = rec.sig_len
    p = rec.p_signal
    t = np.arange(n) * 60.0
    si = np.zeros(n * len(wire), dtype=np.int64)
    ci = np.repeat(np.asarray(wire), n)
    ts = np.tile(t, len(wire))
    vv = p.T.reshape(-1)
    preset = parse_valid_ranges(["numerics"], DEFAULT_CHANNEL_NAMES)
    engines = []
    for vr in (preset, None):
        eng = StreamEngine(1, 10, ring_grid=32768, valid_range=vr)
        for t0 in range(0, n, HOUR):
            m = (ts >= t0 * 60.0) & (ts < (t0 + HOUR) * 60.0)
            eng.ingest_events(torch.from_numpy(si[m]), torch.from_numpy(ci[m]),
                              torch.from_numpy(ts[m]),
                              torch.from_numpy(vv[m].astype(np.float32)),
                              advance_to=float(min(t0 + HOUR, n) * 60.0))
        engines.append(eng)
    return rec, wire, engines[0], engines[1]


def test_real_record_rejected_counts(real_record):
    rec, wire, gated, _plain = real_record
    names, p = decode_record()
    assert names == list(rec.sig_name) and p.shape == rec.p_signal.shape
    lo = {"HR": 1, "PULSE": 1, "RESP": 1, "SpO2": 1}
    hi = {"HR": 350, "PULSE": 350, "RESP": 150, "SpO2": 100}
    want = []
    for j, name in enumerate(names):
        v = p[:, j][~np.isnan(p[:, j])].astype(np.float32)
        want.append(int(((v < lo.get(name, 1)) |
                         (v > hi.get(name, 400))).sum()))
    assert want == [69, 925, 119, 933, 0, 0, 0]
    got = gated.rejected()[0]
    assert got[wire].tolist() == want
    assert got.sum() == sum(want)             # nothing on the other channels


def test_real_record_gated_hr_is_the_mean_of_the_nonzero_samples(real_record):
    rec, wire, gated, plain = real_record
    assert gated.nproc == plain.nproc > 1600 * 12
    hr = rec.p_signal[:, rec.sig_name.index("HR")]
    c = DEFAULT_CHANNEL_NAMES.index("HR")
    bucket = (np.arange(len(hr)) * 60.0 // 5.0).astype(int)
    # Tolerance: a bucket holds one sample, so its sum is exact. The CPU
    # engine's window sum is the difference of two fp32 prefix sums over the
    # buckets of one call: at most HOUR + 3 nonzero additions each (adding an
    # empty bucket is exact), every partial sum below (HOUR + 3) * 93.3 <
    # 2**13, so each addition rounds by at most 2**-12. The mean divides the
    # difference by the window's count; 1e-5 covers its own rounding. A zero
    # among a window's three samples moves the mean by about 20.
    assert np.nanmax(hr) * (HOUR + 3) < 2 ** 13
    err_sum = 2 * (HOUR + 3) * 2.0 ** -12
    # grid points whose 36-bucket window holds a zero AND a nonzero sample
    checked = 0
    for i in np.flatnonzero(hr == 0):
        g = bucket[i] - 20                    # window [g, g + 36) holds it
        inside = (bucket >= g) & (bucket < g + 36)
        vals = hr[inside].astype(np.float32).astype(np.float64)
        if g < 0 or not (vals != 0).any():
            continue
        got_g, got_p = float(gated.proc[0, c, g]), float(plain.proc[0, c, g])
        nz = vals[vals != 0]
        assert abs(got_p - vals.mean()) <= err_sum / len(vals) + 1e-5
        assert abs(got_g - nz.mean()) <= err_sum / len(nz) + 1e-5
        assert abs(got_g - got_p) > 1.0
        checked += 1
    assert checked >= 3


def test_training_frame_valid_range():
    from tskd_amd.io import rdrecord
    from tskd_amd.train.data import record_to_training_frame
    rec = rdrecord(RECORD)
    names = DEFAULT_CHANNEL_NAMES
    preset = parse_valid_ranges(["numerics"], names)
    plain = record_to_training_frame(rec.p_signal, rec.fs, rec.sig_name,
                                     names)
    same_ = record_to_training_frame(rec.p_signal, rec.fs, rec.sig_name,
                                     names, valid_range=None)
    assert plain.equals(same_)
    gated = record_to_training_frame(rec.p_signal, rec.fs, rec.sig_name,
                                     names, valid_range=preset)
    assert gated.shape == plain.shape
    spo2 = rec.p_signal[:, rec.sig_name.index("SpO2")]
    # the rolling mean of the accepted samples never falls below the bound
    assert plain["SpO2"].min() == 0.0 and gated["SpO2"].min() >= 1.0
    assert gated["SpO2"].max() <= spo2.max() and gated["HR"].min() >= 1.0
    # channels the record lacks stay the constant 0 column, also when the
    # gate would reject a 0 there
    all_ = record_to_training_frame(
        rec.p_signal, rec.fs, rec.sig_name, names,
        valid_range=[(1.0, None)] * len(names))
    assert (all_["CVP"] == 0).all() and (gated["NBP Sys"] == 0).all()
    with pytest.raises(ValueError):
        record_to_training_frame(rec.p_signal, rec.fs, rec.sig_name, names,
                                 valid_range=preset[:3])


# ---------------------------------------------------------- configuration
class TestParseValidRanges:
    names = DEFAULT_CHANNEL_NAMES

    def test_preset(self):
        got = dict(zip(self.names, parse_valid_ranges(["numerics"],
                                                      self.names)))
        assert got["HR"] == got["PULSE"] == (1.0, 350.0)
        assert got["RESP"] == (1.0, 150.0) and got["SpO2"] == (1.0, 100.0)
        assert got["NBP Sys"] == got["NBP Dias"] == got["NBP Mean"] == \
            (1.0, 400.0)
        for open_ in ("CVP", "ST V", "PVC Rate per Minute"):
            assert got[open_] == (None, None)
        # a channel list without some of the preset's names
        assert parse_valid_ranges(["numerics"], ["HR", "CVP"]) == \
            [(1.0, 350.0), (None, None)]

    def test_specs(self):
        got = parse_valid_ranges(["HR=1:350", "ST V=:", "SpO2=50:",
                                  "CVP=:30.5", " RESP = -2 : 4 "], self.names)
        by = dict(zip(self.names, got))
        assert by["HR"] == (1.0, 350.0) and by["ST V"] == (None, None)
        assert by["SpO2"] == (50.0, None) and by["CVP"] == (None, 30.5)
        assert by["RESP"] == (-2.0, 4.0) and by["PULSE"] == (None, None)
        assert parse_valid_ranges([], self.names) == [(None, None)] * 10
        # later specs win, over the preset too
        by = dict(zip(self.names, parse_valid_ranges(
            ["numerics", "HR=20:300", "SpO2=:"], self.names)))
        assert by["HR"] == (20.0, 300.0) and by["SpO2"] == (None, None)
        assert by["PULSE"] == (1.0, 350.0)
        # what the parser gives is what the engine takes
        StreamEngine(1, 10, valid_range=got)

    @pytest.mark.parametrize("bad", ["EEG=1:2", "HR", "HR=1", "HR=1:2:3",
                                     "HR=a:2", "HR=2:1", "HR=nan:2",
                                     "vitals", "=1:2"])
    def test_refusals(self, bad):
        with pytest.raises(ValueError):
            parse_valid_ranges([bad], self.names)

    def test_config_key_and_flag_precedence(self, tmp_path, reference_dir):
        cfg = get_global_config(str(tmp_path / "missing.cfg"))
        assert cfg.valid_ranges == [] and resolve_valid_ranges(cfg) is None
        assert resolve_valid_ranges(cfg, ["HR=1:"])[0] == (1.0, None)
        # the reference's own file has no such key and parses as before
        ref = get_global_config(os.path.join(reference_dir, "config.cfg"))
        assert ref.valid_ranges == [] and ref.window_size == 120
        assert resolve_valid_ranges(ref) is None
        path = tmp_path / "config.cfg"
        path.write_text("[SETTINGS]\nWINDOWSIZE = 120\n"
                        "VALID_RANGES = numerics, HR=30:300\n")
        cfg = get_global_config(str(path))
        assert cfg.valid_ranges == ["numerics", "HR=30:300"]
        by = dict(zip(cfg.channel_names, resolve_valid_ranges(cfg)))
        assert by["HR"] == (30.0, 300.0) and by["SpO2"] == (1.0, 100.0)
        # the flag replaces the key as a whole
        by = dict(zip(cfg.channel_names,
                      resolve_valid_ranges(cfg, ["RESP=2:"])))
        assert by["RESP"] == (2.0, None) and by["HR"] == (None, None)
        assert resolve_valid_ranges(cfg, []) == resolve_valid_ranges(cfg)
        path.write_text("[SETTINGS]\nVALID_RANGES = EEG=1:2\n")
        with pytest.raises(ValueError):
            get_global_config(str(path))

    def test_cli_flags(self):
        from tskd_amd.cli import processstream, serve
        for mod in (serve, processstream):
            with pytest.raises(SystemExit):
                mod.main(["--valid-range", "EEG=1:2"])


# ------------------------------------------------------------------ daemon
N_TRIGGERS = 16
PIDS = ("p000601", "p000602")


def run_daemon(tmp_path, tag, device="cpu", pipelined=False, channels=None,
               **kw):
    """Two patients, one sample per 5 s on every named channel, one trigger
    per stream-minute. The first patient's HR alternates between 70 and 0;
    the second's SpO2 and PULSE are 0 throughout. Returns (server, zeros sent
    per patient [HR of the first, SpO2 + PULSE of the second], [(trigger,
    nproc, store rows, response payloads)]). ``channels``: the config's
    channel list when not the default ten."""
    from tskd_amd.cli.serve import FusedServer
    from tskd_amd.store import PredictionStore
    cfg = get_global_config()
    if channels is not None:
        cfg.channel_names = list(channels)
    bus = Bus(str(tmp_path / f"bus_{tag}"))
    store = PredictionStore(str(tmp_path / f"pred_{tag}.log"))
    topics = [cfg.topic_for_channel(c) for c in cfg.channel_names]
    for t in topics:
        bus.create_topic(t)
    prod = Producer(bus)
    torch.manual_seed(7)
    srv = FusedServer(bus, cfg, store, device=device, max_streams=4,
                      ring_grid=256, starting="earliest",
                      response_topic="risk", pipelined=pipelined, **kw)
    reader = Consumer(bus, starting="earliest")
    reader.subscribe(["risk"])
    hr, spo2, pulse = (cfg.channel_names.index(n)
                       for n in ("HR", "SpO2", "PULSE"))
    zeros = [0, 0]
    log = []
    for m in range(N_TRIGGERS):
        for step in range(12):
            k = m * 12 + step
            for i, pid in enumerate(PIDS):
                for ch in range(cfg.n_channels):
                    v = float(60 + 5 * i + ch + k % 7)
                    if i == 0 and ch == hr:
                        v = 70.0 if k % 2 == 0 else 0.0
                    if i == 1 and ch in (spo2, pulse):
                        v = 0.0
                    if v == 0.0:
                        zeros[i] += 1
                    prod.produce(topics[ch], pid, json.dumps([ch, v]),
                                 ts_us=int(k * 5 * 1e6))
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
    return srv, zeros, log


def numerics(names=None):
    return parse_valid_ranges(
        ["numerics"], names or get_global_config().channel_names)


def check_daemon(srv, zeros, log, lifecycle=False):
    """The gated daemon's properties (shared with the GPU run)."""
    cfg = srv.cfg
    g = srv.timer.gauges
    assert g["rejected_samples_total"] == sum(zeros)
    if lifecycle:   # the state keeps its older meaning: patients turned away
        assert g["rejected_total"] == srv.consumer.n_rejected() == 0
    else:
        assert g["rejected_total"] == sum(zeros)
    per = srv.timer.rejected_samples
    assert per["HR"] == zeros[0] and per["SpO2"] == per["PULSE"] == \
        zeros[1] // 2
    assert sum(per.values()) == sum(zeros)
    text = prometheus_text([srv.timer])
    assert f'tskd_rejected_samples_total{{stage="serve",channel="HR"}} ' \
           f'{zeros[0]}' in text
    assert f'state="rejected_samples_total"}} {sum(zeros)}' in text
    rej = srv.se.rejected().cpu()
    assert rej[0, cfg.channel_names.index("HR")] == zeros[0]
    assert rej.sum() == sum(zeros)
    # the processed HR of the first patient is 70, not the 35 of 70/0/70/0
    hr = cfg.channel_names.index("HR")
    last = srv.se.proc[0, hr, (srv.se.nproc - 1) % srv.se.G]
    assert float(last) == 70.0
    reported = {p: 0 for p in PIDS}
    n_msgs = 0
    for _m, _nproc, rows, msgs in log:
        assert sorted(p for p, _t, _r in rows) == sorted(k for k, _v in msgs)
        for key, value in msgs:
            doc = json.loads(value)
            assert sorted(doc) == ["rejected", "risk", "t_us"]
            assert type(doc["rejected"]) is int and doc["rejected"] >= 0
            reported[key] += doc["rejected"]
            n_msgs += 1
    assert n_msgs >= 6
    # every sample rejected up to a patient's last prediction is reported
    # exactly once; what came after waits in the slot's tally
    for i, pid in enumerate(PIDS):
        assert reported[pid] + int(srv._rej_since[i]) == zeros[i]
        assert 0 <= int(srv._rej_since[i]) <= 24
    # one trigger's worth per response once serving is steady
    steady = [json.loads(v)["rejected"] for _m, _n, _r, msgs in log[-2:]
              for k, v in msgs if k == PIDS[0]]
    assert steady == [6, 6]


@pytest.fixture(scope="module")
def gated_daemon(tmp_path_factory):
    return run_daemon(tmp_path_factory.mktemp("qgate"), "on",
                      valid_range=numerics())


@pytest.fixture(scope="module")
def plain_daemon(tmp_path_factory):
    return run_daemon(tmp_path_factory.mktemp("qplain"), "plain")


class TestDaemon:
    def test_gated_counts_and_responses(self, gated_daemon):
        srv, zeros, log = gated_daemon
        assert zeros == [N_TRIGGERS * 6, N_TRIGGERS * 24]
        check_daemon(srv, zeros, log)

    def test_without_the_flag_nothing_changes(self, plain_daemon, tmp_path):
        srv, _zeros, plain = plain_daemon
        _b, _z, none = run_daemon(tmp_path, "none", valid_range=None)
        assert plain == none                    # byte-identical responses
        assert any(msgs for _m, _n, _r, msgs in plain)
        assert all(b"rejected" not in v
                   for _m, _n, _r, msgs in plain for _k, v in msgs)
        assert "rejected_total" not in srv.timer.gauges
        assert "rejected_samples_total" not in srv.timer.gauges
        assert srv.timer.rejected_samples == {}
        assert "tskd_rejected_samples_total" not in \
            prometheus_text([srv.timer])
        assert "rejected_samples" not in json.loads(srv.timer.log_line())
        hr = srv.cfg.channel_names.index("HR")
        last = srv.se.proc[0, hr, (srv.se.nproc - 1) % srv.se.G]
        assert float(last) == 35.0              # what the zeros do today
        with pytest.raises(ValueError):
            srv.se.rejected()

    def test_gate_and_plain_persist_the_same_streams(self, gated_daemon,
                                                     plain_daemon):
        _a, _z, log = gated_daemon
        _b, _y, plain = plain_daemon
        assert [(m, n, sorted(p for p, _t, _r in rows))
                for m, n, rows, _ in log] == \
               [(m, n, sorted(p for p, _t, _r in rows))
                for m, n, rows, _ in plain]

    def test_min_coverage_withholds_the_lead_off_patient(self, tmp_path):
        """--min-coverage 0.5, a ward whose config names HR, PULSE and SpO2:
        every SpO2 and PULSE sample of the second patient is 0. With the gate
        those two channels are imputed throughout, coverage 1/3, withheld;
        without it the zeros count as present, coverage 1, published. The
        first patient (every other HR sample 0) is published either way."""
        three = ("HR", "PULSE", "SpO2")
        on, zeros, log = run_daemon(tmp_path, "cov_on", channels=three,
                                    valid_range=numerics(three),
                                    min_coverage=0.5)
        off, _y, plain = run_daemon(tmp_path, "cov_off", channels=three,
                                    min_coverage=0.5)
        served = [m for m, n, _r, _ in log if n >= 120]
        assert len(served) >= 3
        for (m, n, rows, msgs), (_m, _n, prows, _pm) in zip(log, plain):
            if n < 120:
                assert rows == prows == []
                continue
            assert sorted(p for p, _t, _r in rows) == [PIDS[0]]
            assert sorted(p for p, _t, _r in prows) == sorted(PIDS)
            (key, value), = msgs
            doc = json.loads(value)
            assert sorted(doc) == ["coverage", "rejected", "risk", "t_us"]
            assert doc["coverage"] == 1.0
        assert on.timer.gauges["withheld_total"] == len(served)
        assert off.timer.gauges["withheld_total"] == 0
        assert on.timer.gauges["coverage_mean"] == pytest.approx(
            (1.0 + 1.0 / 3.0) / 2)
        # a withheld prediction does not consume the patient's tally
        assert int(on._rej_since[1]) == zeros[1] == N_TRIGGERS * 24

    def test_pipelined_reports_the_same(self, gated_daemon, tmp_path):
        _srv, _z, log = gated_daemon
        psrv, zeros, plog = run_daemon(tmp_path, "pipe", pipelined=True,
                                       valid_range=numerics())
        assert [(m, sorted((k, json.loads(v)["rejected"]) for k, v in msgs))
                for m, _n, _r, msgs in plog] == \
               [(m, sorted((k, json.loads(v)["rejected"]) for k, v in msgs))
                for m, _n, _r, msgs in log]
        check_daemon(psrv, zeros, plog)

    def test_with_the_lifecycle(self, tmp_path):
        srv, zeros, log = run_daemon(tmp_path, "life", evict_idle_s=3600.0,
                                     valid_range=numerics())
        check_daemon(srv, zeros, log, lifecycle=True)
        # an evicted slot starts over: counter row, host copy and tally
        srv._drop_evicted([(PIDS[0], 0)])
        assert (srv.se.rejected([0]) == 0).all()
        assert srv._rej_prev[0].sum() == 0 and srv._rej_since[0] == 0
        assert srv.se.rejected([1]).sum() == zeros[1]

    def test_state_file_round_trip_counts_from_zero(self, tmp_path):
        srv, zeros, _log = run_daemon(tmp_path, "state", valid_range=numerics(),
                                      state_path=str(tmp_path / "s.snap"))
        from tskd_amd.cli.serve import FusedServer
        from tskd_amd.store import PredictionStore
        torch.manual_seed(7)
        nxt = FusedServer(Bus(str(tmp_path / "bus_state")), srv.cfg,
                          PredictionStore(str(tmp_path / "pred_next.log")),
                          max_streams=4, ring_grid=256, starting="earliest",
                          state_path=str(tmp_path / "s.snap"),
                          valid_range=numerics())
        assert nxt.load_state()
        assert nxt.se.nproc == srv.se.nproc
        assert (nxt.se.rejected() == 0).all()
        nxt.trigger()
        assert nxt.timer.gauges.get("rejected_samples_total", 0) == 0

    def test_wrong_length_is_refused(self, tmp_path):
        with pytest.raises(ValueError):
            run_daemon(tmp_path, "bad", valid_range=numerics()[:3])


def test_processstream_counts_by_channel(tmp_path):
    """The two-stage preprocessor with the gate: lead-off zeros are dropped
    from the emitted points and counted by channel name; an evicted slot's
    counts stay in the totals."""
    from tskd_amd.cli.processstream import ProcessStream
    cfg = get_global_config()
    bus = Bus(str(tmp_path / "bus"))
    topics = [cfg.topic_for_channel(c) for c in cfg.channel_names]
    for t in topics:
        bus.create_topic(t)
    prod = Producer(bus)
    ps = ProcessStream(bus, cfg, max_streams=2, starting="earliest",
                       valid_range=numerics())
    plain = ProcessStream(Bus(str(tmp_path / "bus")), cfg, max_streams=2,
                          starting="earliest", out_topic="call-plain")
    hr = cfg.channel_names.index("HR")
    for k in range(60):
        prod.produce(topics[hr], "p1", json.dumps(
            [hr, 70.0 if k % 2 == 0 else 0.0]), ts_us=int(k * 5 * 1e6))
    assert ps.trigger() > 0 and plain.trigger() > 0
    assert ps.rejected_samples["HR"] == 30
    assert sum(ps.rejected_samples.values()) == 30
    assert plain.rejected_samples == {}
    assert float(ps.engine.proc[0, hr, 0]) == 70.0
    assert float(plain.engine.proc[0, hr, 0]) == 35.0
    ps._drop_evicted([("p1", 0)])
    assert (ps.engine.rejected() == 0).all()
    prod.produce(topics[hr], "p1", json.dumps([hr, 0.0]),
                 ts_us=int(300 * 1e6))
    ps.trigger()
    assert ps.rejected_samples["HR"] == 31

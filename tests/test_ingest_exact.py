"""Bit-exact bucket sum/count tests of the ingest kernels.

ingest_dense_kernel<bf16|fp32>, ingest_events_kernel and
clear_buckets_kernel (csrc/preprocess_kernels.hip) are compared with ``==``
against plain numpy. What makes that legal is the input: nonzero integers
(|v| <= 256 for bf16, |v| <= 4095 for fp32) whose every partial sum stays
below 2**24, so a bucket sum is exact in fp32 under ANY association order —
the kernel's 16-lane tree today, a matrix-core reduction tomorrow. Because
no value is zero, one dropped or one extra sample always changes the sum,
and the count catches it as well.

Every dense launch runs on sentinel-prefilled rings through
``StreamEngine._launch_ingest`` (no fill runs, ``head`` is free), on a raw
tensor that is a misaligned view into a larger buffer whose slack holds
large values: the masked head/tail chunks of the bf16 path and the scalar
peels of the fp32 path see every alignment, and nothing outside
``[head, head + NB)`` of the mapped channels may change.
"""

import numpy as np
import pytest
import torch

from tskd_amd.engine import StreamEngine
from tskd_amd.ops import hip

SENT = -7.25                 # ring prefill: exact in fp32, never a result
BIG = float(2 ** 20)         # slack filler: exact in bf16, wrecks any sum
SLACK = 16                   # elements kept around every raw view
G, C = 64, 5
CHAN_MAPS = {1: [3], 3: [3, 0, 4]}      # non-identity injections into C
BUCKET_LENS = (1, 5, 7, 8, 9, 25, 125, 625)
OFFSETS = (1, 3, 5)          # view start, elements into the buffer's body
HEAD_KINDS = ("zero", "five", "last", "wrap", "turns")
MAXABS = {"bf16": 256, "fp32": 4095}
TORCH_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}

LAYOUTS = pytest.mark.parametrize("packed", [True, False],
                                  ids=["packed", "split"])
DTYPES = pytest.mark.parametrize("dt", ["bf16", "fp32"])


# --------------------------------------------------------------------------
# 1. Oracle and generator
# --------------------------------------------------------------------------
def bucket_oracle(raw_f64, bucket_len):
    """(sum float64, cnt int64), each (S, CIN, NB), of the whole buckets of
    ``raw_f64`` (S, CIN, T): NaN samples are missing, trailing
    ``T % bucket_len`` samples belong to no bucket."""
    S, CIN, T = raw_f64.shape
    nb = T // bucket_len
    bsum = np.zeros((S, CIN, nb), dtype=np.float64)
    bcnt = np.zeros((S, CIN, nb), dtype=np.int64)
    for b in range(nb):
        seg = raw_f64[:, :, b * bucket_len:(b + 1) * bucket_len]
        with np.errstate(invalid="ignore"):     # +inf + -inf
            bsum[:, :, b] = np.nansum(seg, axis=-1)
        bcnt[:, :, b] = np.count_nonzero(~np.isnan(seg), axis=-1)
    return bsum, bcnt


def gen_raw(rng, S, CIN, T, bucket_len, maxabs, nan_frac=0.15):
    """float64 (S, CIN, T) of nonzero integers in [-maxabs, maxabs], ~15%
    NaN, plus forced edge cases, and a dict naming them as (row, bucket):

    first/last   the bucket's first / last sample is NaN
    before/after the sample just outside the bucket is NaN (the neighbour's
                 edge sample or the row's trailing samples)
    allnan       one bucket of NaN only
    single       one bucket with exactly one non-NaN sample
    """
    x = rng.integers(1, maxabs + 1, size=(S, CIN, T)).astype(np.float64)
    x *= rng.choice([-1.0, 1.0], size=x.shape)
    x[rng.random(x.shape) < nan_frac] = np.nan
    flat = x.reshape(-1)                 # rows are contiguous: a view
    nb, L = T // bucket_len, bucket_len
    buckets = [(r, b) for r in range(S * CIN) for b in range(nb)]
    picks = [buckets[i] for i in rng.permutation(len(buckets))]
    info = {k: [] for k in ("first", "last", "before", "after",
                            "allnan", "single")}
    special, edges = picks[:2], picks[2:]
    # the two whole-bucket cases (one of them when there is one bucket)
    if len(special) == 2 or (special and rng.random() < 0.5):
        r, b = special[0]
        flat[r * T + b * L:r * T + (b + 1) * L] = np.nan
        info["allnan"].append((r, b))
    if len(special) == 2 or (special and not info["allnan"]):
        r, b = special[-1]
        start = r * T + b * L
        flat[start:start + L] = np.nan
        flat[start + rng.integers(0, L)] = float(
            rng.integers(1, maxabs + 1)) * rng.choice([-1.0, 1.0])
        info["single"].append((r, b))
    spans = [(r * T + b * L, r * T + (b + 1) * L) for r, b in special]
    for i, (r, b) in enumerate(edges):
        start = r * T + b * L
        kind = ("first", "last", "before", "after", None)[i % 5]
        pos = {"first": start, "last": start + L - 1, "before": start - 1,
               "after": start + L, None: -1}[kind]
        # an edge write never lands in one of the two whole-bucket cases
        if 0 <= pos < flat.size and \
                not any(lo <= pos < hi for lo, hi in spans):
            flat[pos] = np.nan
            info[kind].append((r, b))
    return x, info


def heads_for(nb):
    """Ring heads of a launch of nb buckets, by HEAD_KINDS name."""
    return {"zero": 0, "five": 5, "last": G - 1, "wrap": G - nb + 1,
            "turns": 3 * G + 2}


def dense_cases():
    """The launch shapes of the GPU sweep: every bucket length x NB 1..9 x
    tail {0, 3}; stream count, input rows, base offset and head are dealt
    over them (seeded for S/CIN, cycled for offset and head)."""
    rng = np.random.default_rng(20240607)
    cases, i = [], 0
    for bl in BUCKET_LENS:
        for nb in range(1, 10):
            for tail in (0, 3):
                T = nb * bl + tail      # bl = 1: tail is 3 more buckets
                cases.append(dict(
                    bl=bl, nb=T // bl, req=(nb, tail), T=T,
                    tail=T % bl, S=int(rng.integers(1, 3)),
                    CIN=(1, 3)[rng.integers(0, 2)],
                    off=OFFSETS[(i // 2) % 3], head_kind=HEAD_KINDS[i % 5],
                    seed=i))
                i += 1
    return cases


def alignment_table(dt):
    """What the sweep's launches exercise in ingest_dense_kernel<dt>, from
    the element offset of every bucket (the buffer is 16 B-aligned and the
    view starts SLACK + off elements in)."""
    tab = {"head": set(), "tail": set(), "end_mis": set(),
           "end_short": set()}
    for k in dense_cases():
        rows = k["S"] * k["CIN"]
        for r in range(rows):
            for b in range(k["nb"]):
                e = SLACK + k["off"] + r * k["T"] + b * k["bl"]
                at_end = r == rows - 1 and b == k["nb"] - 1
                if dt == "bf16":
                    mis = e % 8
                    if at_end:      # floors the chunk count: scalar tail
                        tab["end_mis"].add(mis)
                        if mis + k["bl"] < 8:
                            tab["end_short"].add((mis, k["bl"]))
                    else:           # masked first and last chunk
                        tab["head"].add(mis)
                        tab["tail"].add((mis + k["bl"]) % 8)
                else:               # scalar peel before / after the quads
                    pre = min((-e) % 4, k["bl"])
                    tab["head"].add(pre)
                    tab["tail"].add((k["bl"] - pre) % 4)
    return tab


def same(got, exp):
    """torch.equal, with NaN equal to NaN (exact everywhere else)."""
    nan = torch.isnan(exp)
    return torch.equal(torch.isnan(got), nan) and \
        torch.equal(got[~nan], exp[~nan])


def expected_rings(S, raw_f64, bucket_len, head, chan_map, unmapped=SENT):
    """fp32 (S, C, G) sum and count rings after one dense launch on
    SENT-prefilled rings; ``unmapped``: what the written slots of channels
    outside chan_map hold (the kernel leaves them alone)."""
    osum, ocnt = bucket_oracle(raw_f64, bucket_len)
    nb = osum.shape[-1]
    slots = (head + np.arange(nb)) % G
    es = np.full((S, C, G), SENT, dtype=np.float64)
    ec = np.full((S, C, G), SENT, dtype=np.float64)
    es[:, :, slots] = unmapped
    ec[:, :, slots] = unmapped
    for ci, c in enumerate(chan_map):
        es[:, c, slots] = osum[:, ci]
        ec[:, c, slots] = ocnt[:, ci]
    # every finite value is an integer below 2**24 (or SENT): exact in fp32
    return (torch.from_numpy(es).to(torch.float32),
            torch.from_numpy(ec).to(torch.float32))


def test_generator_and_oracle():
    rng = np.random.default_rng(5)
    for dt, bl in (("bf16", 9), ("fp32", 625), ("bf16", 1)):
        S, CIN, nb, tail = 2, 3, 6, 3 if bl > 3 else 0
        x, info = gen_raw(rng, S, CIN, nb * bl + tail, bl, MAXABS[dt])
        ok = ~np.isnan(x)
        assert (x[ok] == np.round(x[ok])).all() and (x[ok] != 0).all()
        assert np.abs(x[ok]).max() <= MAXABS[dt] and (x[ok] < 0).any()
        assert 0.05 < 1 - ok.mean() < 0.8
        # exact in the kernel's input type, sums exact in fp32
        xt = torch.from_numpy(x[ok]).to(TORCH_DT[dt]).double().numpy()
        assert (xt == x[ok]).all() and bl * MAXABS[dt] < 2 ** 24
        osum, ocnt = bucket_oracle(x, bl)
        assert osum.shape == ocnt.shape == (S, CIN, nb)
        assert osum.dtype == np.float64 and ocnt.dtype == np.int64
        rows = x.reshape(S * CIN, -1)
        fs, fc = osum.reshape(S * CIN, nb), ocnt.reshape(S * CIN, nb)
        assert all(info[k] for k in info), info
        (r, b), = info["allnan"]
        assert (fs[r, b], fc[r, b]) == (0.0, 0)
        (r, b), = info["single"]
        assert fc[r, b] == 1 and fs[r, b] != 0
        for r, b in info["first"]:
            assert np.isnan(rows[r, b * bl])
        for r, b in info["last"]:
            assert np.isnan(rows[r, (b + 1) * bl - 1])
        # a NaN just outside a bucket is not the bucket's business
        flat = x.reshape(-1)
        T = nb * bl + tail
        for r, b in info["before"]:
            assert np.isnan(flat[r * T + b * bl - 1])
        for r, b in info["after"]:
            assert np.isnan(flat[r * T + (b + 1) * bl])
        seg = rows[:, :nb * bl].reshape(S * CIN, nb, bl)
        assert (fc == bl - np.isnan(seg).sum(-1)).all()
    # non-finite samples: counted, and summed as float64 sums them
    y = np.array([[[1.0, np.inf, 2.0, np.inf, -np.inf, np.nan, 4.0]]])
    s, c = bucket_oracle(y, 3)
    assert s[0, 0, 0] == np.inf and np.isnan(s[0, 0, 1])
    assert c.tolist() == [[[3, 2]]]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_cpu_engine_matches_oracle(dt):
    """The numpy mode of StreamEngine.ingest_dense against the independent
    oracle, bit for bit, on a slice of the GPU sweep's shapes."""
    cases = [k for k in dense_cases() if k["seed"] % 7 == 0]
    assert {k["bl"] for k in cases} >= {1, 5, 625} and len(cases) >= 12
    for k in cases:
        rng = np.random.default_rng(1000 + k["seed"])
        x, _ = gen_raw(rng, k["S"], k["CIN"], k["T"], k["bl"], MAXABS[dt])
        eng = StreamEngine(k["S"], C, ring_grid=G, fs=k["bl"] / 5.0)
        assert eng.bucket_len == k["bl"]
        eng.bsum.fill_(SENT)
        eng.bcnt.fill_(SENT)
        eng._warned_partial = True
        eng.head = head = heads_for(k["nb"])[k["head_kind"]]
        cm = CHAN_MAPS[k["CIN"]]
        assert eng.ingest_dense(torch.from_numpy(x).to(TORCH_DT[dt]),
                                chan_map=cm) == k["nb"]
        es, ec = expected_rings(k["S"], x, k["bl"], head, cm, unmapped=0.0)
        assert torch.equal(eng.bsum, es) and torch.equal(eng.bcnt, ec), k


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_sweep_covers_every_alignment(dt):
    """Host-side: the union of the sweep's launches reaches every head
    misalignment and every tail residue of the kernel's boundary code, and
    (bf16) every misalignment of the tensor-final bucket, including the
    ones where bucket and misalignment together stay below one chunk."""
    cases = dense_cases()
    tab = alignment_table(dt)
    per = 8 if dt == "bf16" else 4
    shown = "\n".join(f"  {k}: {sorted(v)}" for k, v in tab.items())
    assert tab["head"] == set(range(per)), shown
    assert tab["tail"] == set(range(per)), shown
    if dt == "bf16":
        assert tab["end_mis"] == set(range(8)), shown
        assert tab["end_short"], shown
        assert {bl for _, bl in tab["end_short"]} >= {1, 5}, shown
    # and the sweep is the one the kernel's other paths need
    assert {k["bl"] for k in cases} == set(BUCKET_LENS)
    for bl in BUCKET_LENS:
        sub = [k for k in cases if k["bl"] == bl]
        assert {k["req"] for k in sub} == \
            {(n, t) for n in range(1, 10) for t in (0, 3)}
        if bl > 3:
            assert all((k["nb"], k["tail"]) == k["req"] for k in sub)
        assert {k["head_kind"] for k in sub} == set(HEAD_KINDS)
        assert {k["off"] for k in sub} == set(OFFSETS)
    assert {(k["S"], k["CIN"]) for k in cases} == \
        {(1, 1), (1, 3), (2, 1), (2, 3)}
    # a launch that wraps the ring between two of its buckets
    assert any(k["nb"] > 1 and heads_for(k["nb"])[k["head_kind"]] % G
               + k["nb"] > G for k in cases)


# --------------------------------------------------------------------------
# 2. Dense ingest on the GPU
# --------------------------------------------------------------------------
def place(raw_f64, off, dt):
    """``raw_f64`` as a contiguous device view of type ``dt`` that starts
    SLACK + off elements into a larger 1-D buffer and ends SLACK + 8 before
    its end; the slack holds BIG values and NaN. Returns (buffer, view)."""
    n, lead = raw_f64.size, SLACK + off
    host = torch.full((lead + n + SLACK + 8,), BIG, dtype=torch.float64)
    host[::2] = -BIG
    host[::5] = float("nan")
    host[lead:lead + n] = torch.from_numpy(raw_f64.reshape(-1))
    buf = host.to(TORCH_DT[dt]).cuda()
    view = buf[lead:lead + n].view(raw_f64.shape)
    assert buf.data_ptr() % 16 == 0 and view.is_contiguous()
    assert view.data_ptr() == buf.data_ptr() + lead * buf.element_size()
    return buf, view


class Rings:
    """SENT-prefilled GPU engines of one layout, one per (S, bucket_len)."""

    def __init__(self, monkeypatch, packed):
        monkeypatch.setenv("TSKD_PACKED_BUCKETS", "1" if packed else "0")
        self.packed, self.cache = packed, {}

    def engine(self, S, bl):
        eng = self.cache.get((S, bl))
        if eng is None:
            eng = self.cache[(S, bl)] = StreamEngine(
                S, C, ring_grid=G, fs=bl / 5.0, device="cuda")
            assert eng.bucket_len == bl and eng._packed == self.packed
        if self.packed:
            eng._bkt.fill_(SENT)
        else:
            eng.bsum.fill_(SENT)
            eng.bcnt.fill_(SENT)
        eng.head = eng.nproc = 0
        return eng

    def launch_and_check(self, raw_f64, bl, off, dt, head, note,
                         dstate_head=None):
        """One _launch_ingest at ``head`` (host value; ``dstate_head``: the
        device state block's, which then wins) and the full-ring check."""
        S, CIN, _ = raw_f64.shape
        eng = self.engine(S, bl)
        cm = CHAN_MAPS[CIN]
        buf, view = place(raw_f64, off, dt)
        eng.head = head
        if dstate_head is None:
            eng._launch_ingest(view, cm)
        else:
            dstate = torch.tensor([dstate_head, 12345], dtype=torch.int64,
                                  device="cuda")
            with eng.device_state(dstate):
                eng._launch_ingest(view, cm)
            head = dstate_head
        got_s, got_c = eng.bsum.cpu(), eng.bcnt.cpu()
        es, ec = expected_rings(S, raw_f64, bl, head, cm)
        assert same(got_s, es), f"bsum {note}"
        assert same(got_c, ec), f"bcnt {note}"
        if self.packed:     # the two views are both halves of every pair
            assert eng._bkt.numel() == 2 * es.numel()


@pytest.mark.gpu
@LAYOUTS
@DTYPES
def test_dense_sweep_exact(packed, dt, monkeypatch):
    """Every bucket length x NB x tail of dense_cases(): written slots ==
    the oracle, every other ring element still the sentinel."""
    rings = Rings(monkeypatch, packed)
    bad = []
    for k in dense_cases():
        rng = np.random.default_rng(1000 + k["seed"])
        x, _ = gen_raw(rng, k["S"], k["CIN"], k["T"], k["bl"], MAXABS[dt])
        try:
            rings.launch_and_check(x, k["bl"], k["off"], dt,
                                   heads_for(k["nb"])[k["head_kind"]], k)
        except AssertionError as e:     # go on: name every failing shape
            bad.append(str(e).splitlines()[0])
    assert not bad, f"{len(bad)} launches differ:\n" + "\n".join(bad[:20])


@pytest.mark.gpu
@LAYOUTS
@DTYPES
def test_dense_short_final_bucket(packed, dt, monkeypatch):
    """One-row tensors whose final bucket sits ``mis`` elements into its
    16 B chunk with and without ``mis + bucket_len < 8``: in the first case
    the bf16 kernel has no chunk at all for that bucket and its scalar tail
    must start at the bucket, not ``mis`` samples before it. No NaN, so
    every sample before the bucket (or the slack) would show."""
    rings = Rings(monkeypatch, packed)
    seen = set()
    for off in OFFSETS:
        for bl, T in ((5, 15), (1, 3), (5, 5), (7, 17)):
            rng = np.random.default_rng(77 + off + bl)
            x = rng.integers(1, MAXABS[dt] + 1, size=(1, 1, T)) \
                * rng.choice([-1.0, 1.0], size=(1, 1, T))
            mis = (SLACK + off + (T // bl - 1) * bl) % 8
            seen.add(mis + bl < 8)
            rings.launch_and_check(x, bl, off, dt, 5, (off, bl, T, mis))
    assert seen == {True, False}


@pytest.mark.gpu
@LAYOUTS
@DTYPES
def test_dense_head_from_device_state(packed, dt, monkeypatch):
    """Inside device_state the kernel takes head from the device block,
    not the (different) host value; the launch wraps the ring."""
    rings = Rings(monkeypatch, packed)
    rng = np.random.default_rng(31)
    x, _ = gen_raw(rng, 2, 3, 5 * 9 + 3, 9, MAXABS[dt])
    rings.launch_and_check(x, 9, 3, dt, 7, "dstate", dstate_head=2 * G - 2)


@pytest.mark.gpu
@LAYOUTS
@DTYPES
def test_dense_nonfinite_exact(packed, dt, monkeypatch):
    """+inf in a bucket: sum +inf, counted. +inf and -inf: NaN sum. ±inf
    and NaN just outside a bucket — neighbouring samples, the trailing
    samples, the next row — leave its finite sum exact (a reduction that
    multiplies by a 0/1 mask would turn it into NaN)."""
    rings = Rings(monkeypatch, packed)
    inf, nan = float("inf"), float("nan")
    for bl in (5, 9, 625):
        for off in OFFSETS:
            S, CIN, nb, tail = 1, 3, 5, 3
            T = nb * bl + tail
            rng = np.random.default_rng(900 + bl + off)
            x, _ = gen_raw(rng, S, CIN, T, bl, MAXABS[dt], nan_frac=0.05)
            for r in range(CIN):
                row = x[0, r]
                row[0 * bl + 1] = inf
                row[0 * bl + bl - 2] = -inf       # bucket 0: NaN sum
                row[1 * bl + bl - 1] = (-inf, nan, inf)[r]   # before bucket 2
                row[3 * bl] = (inf, -inf, nan)[r]            # after bucket 2
                if r == 0:
                    row[3 * bl + 2] = inf         # bucket 3: +inf twice
                row[nb * bl:] = (inf, nan, -inf)  # after bucket 4, before
                #                                   the next row's bucket 0
            x[0, 1, 1] = 3.0                      # row 1 bucket 0: -inf only
            osum, ocnt = bucket_oracle(x, bl)
            assert np.isnan(osum[0, 0, 0]) and osum[0, 1, 0] == -inf
            assert osum[0, 0, 3] == inf and osum[0, 0, 1] == -inf
            assert np.isfinite(osum[0, :, 2]).all() and \
                np.isfinite(osum[0, :, 4]).all()
            assert ocnt[0, 0, 3] >= 2
            rings.launch_and_check(x, bl, off, dt, G - 3, (bl, off))


@pytest.mark.gpu
@LAYOUTS
@DTYPES
def test_public_ingest_dense_noncontiguous(packed, dt, monkeypatch):
    """StreamEngine.ingest_dense itself, on a non-contiguous slice: the
    engine's copy is what the kernel reads, mapped channels == the oracle,
    the other channels' slots are cleared, the rest is untouched. bf16 runs
    bucket_len 5 with the final bucket 2 elements into its chunk; fp32 runs
    bucket_len 625."""
    monkeypatch.setenv("TSKD_PACKED_BUCKETS", "1" if packed else "0")
    bl, nb = (5, 4) if dt == "bf16" else (625, 2)
    S, CIN, T = 2, 3, nb * bl + 3
    if dt == "bf16":    # the engine's contiguous copy is 16 B-aligned
        assert ((S * CIN - 1) * T + (nb - 1) * bl) % 8 + bl < 8
    rng = np.random.default_rng(404)
    x, _ = gen_raw(rng, S, CIN, T, bl, MAXABS[dt])
    big = np.full((S, CIN, T + 9), BIG)
    big[:, :, 4:4 + T] = x
    dev = torch.from_numpy(big).to(TORCH_DT[dt]).cuda()
    sl = dev[:, :, 4:4 + T]
    assert not sl.is_contiguous()
    eng = StreamEngine(S, C, ring_grid=G, fs=bl / 5.0, device="cuda")
    assert eng.bucket_len == bl and eng._packed == packed
    eng.bsum.fill_(SENT)
    eng.bcnt.fill_(SENT)
    cm = CHAN_MAPS[CIN]
    with pytest.warns(UserWarning, match="dropping 3 trailing samples"):
        assert eng.ingest_dense(sl, chan_map=cm) == nb
    assert eng.head == nb and eng.nproc == 0
    es, ec = expected_rings(S, x, bl, 0, cm, unmapped=0.0)
    assert torch.equal(eng.bsum.cpu(), es)
    assert torch.equal(eng.bcnt.cpu(), ec)


# --------------------------------------------------------------------------
# 3. Events and clear on the GPU
# --------------------------------------------------------------------------
ES, EC, EG = 3, 4, 32


def event_rings(packed, fill):
    """(sum view, count view, element stride) of fresh (ES, EC, EG) rings."""
    if packed:
        bkt = torch.full((ES, EC, EG, 2), fill, device="cuda")
        return bkt[..., 0], bkt[..., 1], 2
    return (torch.full((ES, EC, EG), fill, device="cuda"),
            torch.full((ES, EC, EG), fill, device="cuda"), 1)


def launch_events(si, ci, bi, vi, bsum, bcnt, bst, min_bucket):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
           for a in (si.astype(np.int32), ci.astype(np.int32),
                     bi.astype(np.int64), vi.astype(np.float32))]
    hip.check(hip.load(hip.PREPROC).tskd_preproc_ingest_events(
        *(hip.ptr(t) for t in dev), hip.ptr(bsum), hip.ptr(bcnt), EC, EG,
        len(vi), min_bucket, bst, hip.stream_ptr()),
        "tskd_preproc_ingest_events")
    torch.cuda.synchronize()


def events_oracle(si, ci, bi, vi, min_bucket, fill):
    es = np.full((ES, EC, EG), fill, dtype=np.float64)
    ec = np.full((ES, EC, EG), fill, dtype=np.float64)
    keep = (bi >= min_bucket) & ~np.isnan(vi)
    at = (si[keep], ci[keep], bi[keep] % EG)
    np.add.at(es, at, vi[keep].astype(np.float64))
    np.add.at(ec, at, 1.0)
    return (torch.from_numpy(es).to(torch.float32),
            torch.from_numpy(ec).to(torch.float32))


@pytest.mark.gpu
@LAYOUTS
def test_events_random_exact(packed):
    """Integer-valued events over ~3 ring turns accumulate ONTO the
    sentinel (quarter-integers far below 2**22: exact in any atomic order).
    Late events (b < min_bucket) and NaN values are dropped and not
    counted, b == min_bucket is kept, stream 1 gets nothing."""
    rng = np.random.default_rng(8)
    n, min_bucket = 6000, 75
    si = rng.choice([0, 2], size=n)
    ci = rng.integers(0, EC, size=n)
    bi = rng.integers(min_bucket - 8, min_bucket + 3 * EG, size=n)
    vi = rng.integers(-40, 41, size=n).astype(np.float64)
    vi[rng.random(n) < 0.1] = np.nan
    bi[:60] = min_bucket            # on the watermark: kept
    bi[60:120] = min_bucket - 1     # just behind it: dropped
    vi[:60:6] = np.nan
    vi[1:120:6] = 17.0
    assert (bi < min_bucket).sum() > 200 and np.isnan(vi).sum() > 300
    bsum, bcnt, bst = event_rings(packed, SENT)
    launch_events(si, ci, bi, vi, bsum, bcnt, bst, min_bucket)
    es, ec = events_oracle(si, ci, bi, vi, min_bucket, SENT)
    assert (es[1] == SENT).all() and (ec[0] != SENT).all()
    assert torch.equal(bsum.cpu(), es)
    assert torch.equal(bcnt.cpu(), ec)


@pytest.mark.gpu
@LAYOUTS
def test_events_contention_exact(packed):
    """20 000 events of +1 / -1 into ONE (stream, channel, bucket): the
    count is exactly 20 000, the sum exact, nothing else moves."""
    rng = np.random.default_rng(9)
    n, min_bucket = 20000, 40
    vi = rng.choice([-1.0, 1.0], size=n)
    si, ci = np.full(n, 1), np.full(n, 2)
    bi = np.full(n, min_bucket + EG + 5)
    bsum, bcnt, bst = event_rings(packed, 0.0)
    launch_events(si, ci, bi, vi, bsum, bcnt, bst, min_bucket)
    es, ec = events_oracle(si, ci, bi, vi, min_bucket, 0.0)
    slot = (min_bucket + EG + 5) % EG
    assert ec[1, 2, slot] == 20000 and ec.sum() == 20000
    assert es[1, 2, slot] == vi.sum()
    assert torch.equal(bsum.cpu(), es)
    assert torch.equal(bcnt.cpu(), ec)


@pytest.mark.gpu
@LAYOUTS
def test_events_none_launches_nothing(packed):
    bsum, bcnt, bst = event_rings(packed, SENT)
    empty = np.zeros(0)
    launch_events(empty, empty, empty, empty, bsum, bcnt, bst, 0)
    assert (bsum == SENT).all() and (bcnt == SENT).all()


@pytest.mark.gpu
@LAYOUTS
def test_clear_buckets_exact_slots(packed):
    """clear_buckets zeroes exactly slots (head + j) % G, j < nb, of every
    (stream, channel), also when the range wraps or head is turns ahead."""
    lib = hip.load(hip.PREPROC)
    for head, nb in ((0, 5), (EG - 2, 5), (5 * EG + 30, EG), (7, 0)):
        bsum, bcnt, bst = event_rings(packed, SENT)
        hip.check(lib.tskd_preproc_clear_buckets(
            hip.ptr(bsum), hip.ptr(bcnt), ES, EC, EG, head, nb, bst,
            hip.stream_ptr()), "tskd_preproc_clear_buckets")
        torch.cuda.synchronize()
        exp = torch.full((ES, EC, EG), SENT)
        exp[:, :, [(head + j) % EG for j in range(nb)]] = 0.0
        assert torch.equal(bsum.cpu(), exp), (head, nb)
        assert torch.equal(bcnt.cpu(), exp), (head, nb)

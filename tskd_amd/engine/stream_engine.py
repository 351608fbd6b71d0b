"""StreamEngine — GPU-resident streaming window engine.

The MI355X-native replacement for the reference's Spark Structured Streaming
stage: per-(stream, channel) ring buffers in HBM3E hold 5-s
bucket aggregates and processed 180 s/5 s window averages; the fused HIP
kernels in csrc/preprocess_kernels.hip do ingest, sliding-mean + gap-fill and
model-window gather entirely on-GPU, so raw waveforms never round-trip to the
host between ingestion and inference.

Memory plan (SURVEY.md §5 long-context): state per (stream, channel) is
O(ring), never O(stream): 3 fp32 rings of G grid points. At G=4096 (5.7 h of
5-s history), 64k streams x 10 ch cost 64k*10*4096*12 B = 31 GB of the
288 GB HBM3E — BASELINE.json config 4's 64k-stream scenario fits one GPU.

CPU mode runs the same semantics in numpy (the tests' property oracle is
pandas-free windowing.py, itself tested against the kernels).
"""

from __future__ import annotations

import contextlib
import os
from typing import Optional, Sequence

import numpy as np
import torch

from tskd_amd.engine import windowing as W
from tskd_amd.engine.snapshot import GEOMETRY, EngineSnapshot
from tskd_amd.ops import hip

# longest window the GPU fill kernels take: FILL_MAXW in
# preprocess_kernels.hip (tests/test_engine.py holds the two together)
GPU_MAX_WIN_BUCKETS = 64


def check_valid_range(valid_range, n_channels: int) -> np.ndarray:
    """``valid_range`` — a length-C sequence of ``(lo, hi)``, None meaning
    open on that side — as fp32 ``(C, 2)`` bounds with ±inf for the open
    sides. ValueError: a wrong length, a NaN bound, or lo > hi."""
    rows = list(valid_range)
    if len(rows) != n_channels:
        raise ValueError(f"valid_range has {len(rows)} entries for "
                         f"{n_channels} channels")
    out = np.empty((n_channels, 2), dtype=np.float32)
    for c, row in enumerate(rows):
        try:
            lo, hi = row
        except (TypeError, ValueError):
            raise ValueError(f"valid_range[{c}]={row!r} is not a (lo, hi) "
                             f"pair") from None
        lo = -np.inf if lo is None else np.float32(lo)
        hi = np.inf if hi is None else np.float32(hi)
        if np.isnan(lo) or np.isnan(hi):
            raise ValueError(f"valid_range[{c}] has a NaN bound")
        if lo > hi:
            raise ValueError(f"valid_range[{c}]: lo={lo} > hi={hi}")
        out[c] = lo, hi
    return out


class StreamEngine:
    """Event-time sliding-window engine over S streams x C channels.

    Durations are expressed in GRID units internally; the reference constants
    (180 s window / 5 s slide / 600 s model window) map to win_buckets=36 and
    model_win=120. ``speed`` compresses wall-clock like the reference's
    --speed flag but does NOT change grid semantics.
    """

    def __init__(self, n_streams: int, n_channels: int = 10,
                 ring_grid: int = 4096, fs: float = 125.0,
                 bucket_s: float = W.BUCKET_S, win_buckets: int = W.WIN_BUCKETS,
                 model_win: int = W.MODEL_WIN, device: str = "cpu",
                 valid_range=None):
        self.S, self.C, self.G = n_streams, n_channels, ring_grid
        self.fs = fs
        self.bucket_s = bucket_s
        self.bucket_len = int(round(fs * bucket_s))  # dense samples per bucket
        self.win_buckets = win_buckets
        self.model_win = model_win
        self.device = torch.device(device)
        self.head = 0    # buckets ingested (dense path)
        self.nproc = 0   # processed grid points produced
        self._cleared = 0  # ring slots zeroed up to this bucket (event path)
        # grid point at which this engine's streams BEGAN: nonzero when the
        # first event carries a large (e.g. wall-clock) timestamp and the
        # grid origin skips ahead — `ready` counts data since here
        self._origin_nproc = 0
        dev = self.device
        # Packed layout (GPU): (sum, cnt) interleaved as adjacent floats so
        # window_fill reads each bucket with ONE f32x2 load. bsum/bcnt stay
        # the public (S, C, G) views; kernels take the element stride.
        self._gpu = dev.type == "cuda"
        if self._gpu and not 1 <= win_buckets <= GPU_MAX_WIN_BUCKETS:
            raise ValueError(
                f"win_buckets={win_buckets} outside [1, "
                f"{GPU_MAX_WIN_BUCKETS}]: the fill kernels' window limit")
        self._packed = self._gpu and \
            os.environ.get("TSKD_PACKED_BUCKETS", "1") != "0"
        if self._packed:
            self._bkt = torch.zeros(self.S, self.C, self.G, 2, device=dev)
            self.bsum = self._bkt[..., 0]
            self.bcnt = self._bkt[..., 1]
            self._bst = 2
        else:
            self.bsum = torch.zeros(self.S, self.C, self.G, device=dev)
            self.bcnt = torch.zeros(self.S, self.C, self.G, device=dev)
            self._bst = 1
        self.proc = torch.zeros(self.S, self.C, self.G, device=dev)
        self.last_val = torch.full((self.S, self.C), float("nan"), device=dev)
        self._dstate = None  # device [head, nproc] during graph capture/replay
        self._dstate_gather_extra = 0
        self._cm_cache = {}  # chan_map tuple -> int32 device tensor
        self._warned_partial = False
        self._forced_ready = False
        # stream lifecycle: grid point at which each slot's CURRENT occupant
        # was admitted (0 = since the engine began; see admit/stream_ready)
        self.born = np.zeros(self.S, dtype=np.int64)
        # warm restart: processed points below this grid point were not
        # carried over by restore() (0 on an engine that was never restored)
        self._proc_floor = 0
        # ... and buckets below this one neither: coverage() counts them as
        # present (their state is unknown)
        self._bucket_floor = 0
        self._snap_dev = self._snap_host = None  # reused staging buffers
        # signal-quality gate (opt-in, docs/PARITY.md divergence 15): per
        # wire channel a closed interval [lo, hi]; a sample outside it that
        # is not NaN is rejected at ingest (neither summed nor counted) and
        # adds 1 to the cumulative (S, C) int64 counter ``rej``. None: no
        # gate, nothing allocated, every launch the ungated one.
        self.bounds = self.rej = None
        if valid_range is not None:
            self.bounds = torch.from_numpy(
                check_valid_range(valid_range, self.C)).to(dev)
            self.rej = torch.zeros(self.S, self.C, dtype=torch.int64,
                                   device=dev)
        if self._gpu:
            hip.load(hip.PREPROC)  # fail here, not at the first launch

    def _dstate_ptr(self):
        return hip.ptr(self._dstate)

    @contextlib.contextmanager
    def device_state(self, dstate: torch.Tensor, gather_extra: int = 0):
        """Within the block every launch reads the ring position from the
        device int64[2] ``dstate`` = [head, nproc] block (graph capture and
        replay) instead of the host indices; the window gather and the
        fused tail end at ``nproc + gather_extra``."""
        self._dstate, self._dstate_gather_extra = dstate, gather_extra
        try:
            yield
        finally:
            self._dstate, self._dstate_gather_extra = None, 0

    def _chan_map_tensor(self, chan_map: Sequence[int]) -> torch.Tensor:
        key = tuple(chan_map)
        cm = self._cm_cache.get(key)
        if cm is None:
            cm = self._cm_cache[key] = torch.tensor(
                list(chan_map), dtype=torch.int32, device=self.device)
        return cm

    def _launch_ingest(self, raw: torch.Tensor, chan_map) -> None:
        """Dense bucket ingest of contiguous fp32/bf16 ``raw`` at head (the
        kernel takes the device state block's head when one is set)."""
        lib = hip.load(hip.PREPROC)
        args = (hip.ptr(raw), int(raw.dtype == torch.bfloat16),
                hip.ptr(self.bsum), hip.ptr(self.bcnt),
                hip.ptr(self._chan_map_tensor(chan_map)), self.S,
                raw.shape[1], self.C, raw.shape[2], self.G, self.bucket_len,
                self.head, self._dstate_ptr(), self._bst)
        if self.bounds is None:
            hip.check(lib.tskd_preproc_ingest_dense(*args, hip.stream_ptr()),
                      "tskd_preproc_ingest_dense")
        else:
            hip.check(lib.tskd_preproc_ingest_dense_gated(
                *args, hip.ptr(self.bounds), hip.ptr(self.rej),
                hip.stream_ptr()), "tskd_preproc_ingest_dense_gated")

    def _launch_fill(self, phead: int, np_new: int) -> None:
        """Window fill of ``np_new`` grid points from ``phead`` (or from the
        device state block's nproc when one is set)."""
        hip.check(hip.load(hip.PREPROC).tskd_preproc_window_fill(
            hip.ptr(self.bsum), hip.ptr(self.bcnt), hip.ptr(self.proc),
            hip.ptr(self.last_val), self.S, self.C, self.G, phead, np_new,
            self.win_buckets, self._dstate_ptr(), self._bst,
            hip.stream_ptr()), "tskd_preproc_window_fill")

    # ------------------------------------------------------------------ ingest
    def ingest_dense(self, raw: torch.Tensor,
                     chan_map: Optional[Sequence[int]] = None) -> int:
        """raw (S, CIN, T) contiguous samples at self.fs starting at the
        current head; returns number of new buckets per channel.

        Only whole buckets are ingested: trailing ``T % bucket_len`` samples
        are dropped (warned once) — callers should send bucket-aligned
        trigger chunks (60 s at fs=125 is always aligned)."""
        assert raw.shape[0] == self.S
        cin, t = raw.shape[1], raw.shape[2]
        nb = t // self.bucket_len
        if t % self.bucket_len and not self._warned_partial:
            import warnings
            warnings.warn(
                f"ingest_dense: dropping {t % self.bucket_len} trailing "
                f"samples (T={t} not a multiple of bucket_len="
                f"{self.bucket_len})", stacklevel=2)
            self._warned_partial = True
        if nb > self.G - self.win_buckets:
            raise ValueError(
                f"batch spans {nb} buckets > ring capacity "
                f"{self.G - self.win_buckets}; ingest in smaller chunks")
        if chan_map is None:
            chan_map = list(range(cin))
        if self._gpu:
            raw = raw.contiguous()
            if raw.dtype not in (torch.bfloat16, torch.float32):
                raw = raw.float()
            self._launch_ingest(raw, chan_map)
            self._clear_stale_channels(chan_map, nb)
        else:
            rawf = raw.float().cpu().numpy()
            if self.bounds is not None:
                bnd = self.bounds.numpy()[list(chan_map)]   # (CIN, 2)
                lo, hi = bnd[None, :, 0, None], bnd[None, :, 1, None]
            for j in range(nb):
                seg = rawf[:, :, j * self.bucket_len:(j + 1) * self.bucket_len]
                ok = ~np.isnan(seg)
                if self.bounds is not None:
                    acc = (lo <= seg) & (seg <= hi)     # False for NaN
                    nrej = (ok & ~acc).sum(-1)          # (S, CIN)
                    for ci, c in enumerate(chan_map):
                        self.rej[:, c] += torch.from_numpy(nrej[:, ci])
                    ok = acc
                g = (self.head + j) % self.G
                for ci, c in enumerate(chan_map):
                    self.bsum[:, c, g] = torch.from_numpy(
                        np.where(ok[:, ci], seg[:, ci], 0.0).sum(-1)).float()
                    self.bcnt[:, c, g] = torch.from_numpy(
                        ok[:, ci].sum(-1).astype(np.float64)).float()
                # channels not in chan_map get empty buckets at this grid
                other = [c for c in range(self.C) if c not in chan_map]
                if other:
                    self.bsum[:, other, g] = 0
                    self.bcnt[:, other, g] = 0
        self.head += nb
        self._cleared = max(self._cleared, self.head)
        self._refill()
        return nb

    def _clear_stale_channels(self, chan_map: Sequence[int], nb: int) -> None:
        """Channels with no data this trigger still need their (re-used) ring
        slots zeroed — GPU path (CPU path does it inline)."""
        other = [c for c in range(self.C) if c not in set(chan_map)]
        if not other or nb <= 0:
            return
        idx = torch.tensor([(self.head + j) % self.G for j in range(nb)],
                           dtype=torch.long, device=self.device)
        oth = torch.tensor(other, dtype=torch.long, device=self.device)
        self.bsum[:, oth[:, None], idx[None, :]] = 0
        self.bcnt[:, oth[:, None], idx[None, :]] = 0

    def ingest_events(self, stream_idx: torch.Tensor, chan_idx: torch.Tensor,
                      ts: torch.Tensor, vals: torch.Tensor,
                      advance_to: Optional[float] = None) -> None:
        """Irregular event batch (the real numerics-record path, fs=1/60 Hz).

        Event time ``ts`` is in seconds; buckets behind the already-processed
        grid (the watermark) are dropped, like Spark's withWatermark
        (processStream.py:196). ``advance_to``: event-time high-water mark in
        seconds (defaults to max ts) — buckets strictly before it become
        eligible for processing.
        """
        if len(ts) == 0 and advance_to is None:
            return  # nothing to ingest, no watermark advance
        if (len(ts) and self.head == 0 and self.nproc == 0
                and self._origin_nproc == 0):
            first_bucket = int(float(ts.min()) // self.bucket_s)
            if first_bucket > self.G:
                # wall-clock event times on a fresh engine: the stream
                # BEGINS at the first event's bucket — `ready` counts
                # 600 s + 180 s of event time from here, exactly like a
                # zero-based replay counts from t=0
                self._origin_nproc = first_bucket
        min_bucket = self.nproc  # processed grid is immutable
        if self._gpu:
            # Bucketing/min/max on the GPU: host float64 math over millions
            # of events was the event path's dominant cost (event_bench).
            tsd = ts.double().to(self.device) if not ts.is_cuda else ts.double()
            bucket_d = torch.floor(tsd / self.bucket_s).long()
            if len(bucket_d):
                bmax = int(bucket_d.max().item())
                bmin = int(bucket_d.min().item())
                if bmax - max(bmin, min_bucket) >= self.G - self.win_buckets:
                    raise ValueError(
                        "event batch spans more buckets than the ring "
                        "holds; ingest in smaller chunks")
                self._clear_ahead(bmax + 1)
            else:
                self._clear_ahead(0)
            si = stream_idx.to(torch.int32).contiguous().to(self.device)
            ci = chan_idx.to(torch.int32).contiguous().to(self.device)
            bi = bucket_d.contiguous()
            vi = vals.float().contiguous().to(self.device)
            lib = hip.load(hip.PREPROC)
            args = (hip.ptr(si), hip.ptr(ci), hip.ptr(bi), hip.ptr(vi),
                    hip.ptr(self.bsum), hip.ptr(self.bcnt), self.C, self.G,
                    len(vi), min_bucket, self._bst)
            if self.bounds is None:
                hip.check(lib.tskd_preproc_ingest_events(
                    *args, hip.stream_ptr()), "tskd_preproc_ingest_events")
            else:
                hip.check(lib.tskd_preproc_ingest_events_gated(
                    *args, hip.ptr(self.bounds), hip.ptr(self.rej),
                    hip.stream_ptr()), "tskd_preproc_ingest_events_gated")
            if advance_to is None and len(tsd):
                advance_to = float(tsd.max().item())
        else:
            bucket = torch.floor(ts.double() / self.bucket_s).long()
            if len(bucket) and int(bucket.max()) - max(int(bucket.min()),
                                                       min_bucket) \
                    >= self.G - self.win_buckets:
                raise ValueError("event batch spans more buckets than the "
                                 "ring holds; ingest in smaller chunks")
            self._clear_ahead(int(bucket.max().item()) + 1 if len(bucket)
                              else 0)
            ok = (~torch.isnan(vals)) & (bucket >= min_bucket)
            if self.bounds is not None:
                # late drop first: a late event is not counted as rejected
                v32 = vals.float()
                bnd = self.bounds[chan_idx.long()]
                acc = (bnd[:, 0] <= v32) & (v32 <= bnd[:, 1])
                out = ok & ~acc
                if out.any():
                    np.add.at(self.rej.numpy().reshape(-1),
                              stream_idx[out].numpy() * self.C
                              + chan_idx[out].numpy(), 1)
                ok = ok & acc
            if ok.any():
                flat = ((stream_idx[ok].numpy() * self.C
                         + chan_idx[ok].numpy()) * self.G
                        + (bucket[ok].numpy() % self.G))
                bs = self.bsum.numpy().reshape(-1)
                bc = self.bcnt.numpy().reshape(-1)
                np.add.at(bs, flat, vals[ok].numpy().astype(np.float64))
                np.add.at(bc, flat, 1.0)
        hwm = float(advance_to) if advance_to is not None else float(ts.max())
        new_head = int(np.floor(hwm / self.bucket_s))
        if new_head > self.head:
            self.head = new_head
        self._refill()

    def ingest_events_chunked(self, stream_idx, chan_idx, ts, vals,
                              advance_to=None) -> None:
        """ingest_events for arbitrarily large backlogs: events are
        processed in bucket-ordered chunks no wider than the ring allows
        (catch-up replay after a long outage). Grid history older than the
        ring is overwritten — only the last ~G points are retained."""
        cap = self.G - self.win_buckets - 1
        if len(ts) == 0:
            if advance_to is not None:
                self.ingest_events(stream_idx, chan_idx, ts, vals,
                                   advance_to=advance_to)
            return
        bucket = torch.floor(ts.double() / self.bucket_s).long()
        span = int(bucket.max()) - max(int(bucket.min()), self.nproc)
        if span < cap:
            self.ingest_events(stream_idx, chan_idx, ts, vals,
                               advance_to=advance_to)
            return
        order = torch.argsort(bucket)
        b_sorted = bucket[order]
        lo = 0
        n = len(order)
        while lo < n:
            start_bucket = max(int(b_sorted[lo]), self.nproc)
            hi = int(torch.searchsorted(b_sorted,
                                        torch.tensor(start_bucket + cap)))
            hi = max(hi, lo + 1)
            idx = order[lo:hi]
            chunk_adv = float((int(b_sorted[min(hi, n) - 1]) + 1)
                              * self.bucket_s)
            self.ingest_events(stream_idx[idx], chan_idx[idx], ts[idx],
                               vals[idx], advance_to=chunk_adv)
            lo = hi
        if advance_to is not None:
            self.advance_watermark(advance_to)

    def advance_watermark(self, seconds: float) -> None:
        """Advance the event-time watermark to ``seconds`` without events:
        buckets before it become eligible and are processed."""
        if seconds / self.bucket_s > self.head:
            self._clear_ahead(int(seconds / self.bucket_s))
            self.head = int(seconds / self.bucket_s)
            self._refill()

    def _clear_ahead(self, upto_bucket: int) -> None:
        """Zero ring slots about to be re-used (stale data from G buckets
        ago). No-op until the ring wraps."""
        if upto_bucket <= self._cleared:
            return
        start = max(self._cleared, upto_bucket - self.G)
        nb = upto_bucket - start
        if self._gpu:
            hip.check(hip.load(hip.PREPROC).tskd_preproc_clear_buckets(
                hip.ptr(self.bsum), hip.ptr(self.bcnt), self.S, self.C,
                self.G, start, nb, self._bst, hip.stream_ptr()),
                "tskd_preproc_clear_buckets")
        else:
            idx = np.arange(start, start + nb) % self.G
            self.bsum[:, :, idx] = 0
            self.bcnt[:, :, idx] = 0
        self._cleared = upto_bucket

    def ingest_graph_kernel(self, raw: torch.Tensor, chan_map) -> None:
        """Capture-safe dense ingest only (bucket writes; head from dstate).
        Writes buckets [head, head+NB) — DISJOINT from anything the fill
        stage of the PREVIOUS trigger reads, which is what makes the
        two-stream overlapped TriggerGraph legal."""
        self._launch_ingest(raw, chan_map)

    def fill_graph_kernel(self, nb: int) -> None:
        """Capture-safe window fill of nb new grid points (nproc from
        dstate; reads buckets [nproc, nproc+nb+win-1) = through the buckets
        the SAME trigger's ingest just wrote)."""
        self._launch_fill(self.nproc, nb)

    def ingest_dense_graph_body(self, raw: torch.Tensor, chan_map, nb: int
                                 ) -> None:
        """Capture-safe ingest + fill: kernels only, indices from dstate."""
        self.ingest_graph_kernel(raw, chan_map)
        self.fill_graph_kernel(nb)

    # ----------------------------------------------------------------- process
    def _refill(self) -> None:
        """Produce newly-complete processed grid points (window starts)."""
        navail = max(0, self.head - self.win_buckets + 1)
        np_new = navail - self.nproc
        if np_new <= 0:
            return
        # The ring retains only the last G buckets: grid points further back
        # than that were overwritten and cannot be produced. Skip ahead —
        # this is both the catch-up-after-long-outage semantics the chunked
        # ingest documents AND what makes wall-clock (epoch-seconds) event
        # times work on a fresh engine (the stream "begins mid-history").
        max_np = self.G - self.win_buckets
        if np_new > max_np:
            self.nproc = navail - max_np
            np_new = max_np
        if self._gpu:
            self._launch_fill(self.nproc, np_new)
        else:
            bs = self.bsum.numpy()
            bc = self.bcnt.numpy()
            pr = self.proc.numpy()
            lv = self.last_val.numpy()
            # vectorized sliding sums via cumsum over the gathered bucket
            # range [nproc, nproc + np_new + win - 1)
            span = np_new + self.win_buckets - 1
            gidx = (self.nproc + np.arange(span)) % self.G
            pidx = (self.nproc + np.arange(np_new)) % self.G
            for s in range(self.S):
                for c in range(self.C):
                    vals = W.window_averages(bs[s, c, gidx], bc[s, c, gidx],
                                             self.win_buckets)
                    filled, carry = W.fill_series(vals, lv[s, c])
                    pr[s, c, pidx] = filled
                    lv[s, c] = carry
        self.nproc = navail

    # ------------------------------------------------------------------ gather
    def windows(self, batch: int = 1, stride: int = 12,
                dtype: torch.dtype = torch.float32,
                out: Optional[torch.Tensor] = None,
                timelast: bool = False,
                znormalize: bool = False, zeps: float = 1e-6) -> torch.Tensor:
        """Assemble (S, batch, C, model_win) model inputs ending at the latest
        processed grid point; window b ends at nproc - (batch-1-b)*stride.
        Early windows that would reach before grid 0 are all-zero.
        ``out``: optional pre-allocated destination (e.g. a GraphedForward's
        static input buffer) — every element is overwritten."""
        B, WIN = batch, self.model_win
        assert (B - 1) * stride + WIN <= self.G, (
            f"windows(batch={B}, stride={stride}) reaches back "
            f"{(B - 1) * stride + WIN} grid points but the ring holds only "
            f"G={self.G} — older slots are already overwritten")
        self._check_floor((B - 1) * stride + WIN)
        shape = (self.S, B, WIN, self.C) if timelast \
            else (self.S, B, self.C, WIN)
        provided = out is not None
        if out is not None:
            assert out.shape == shape and out.dtype == dtype
            assert out.is_contiguous()
        out = out if out is not None else torch.zeros(
            shape, dtype=dtype, device=self.device)
        if self._gpu:
            lib = hip.load(hip.PREPROC)
            is_bf16 = 1 if dtype == torch.bfloat16 else 0
            assert dtype in (torch.bfloat16, torch.float32)
            hip.check(lib.tskd_preproc_window_gather(
                hip.ptr(self.proc), hip.ptr(out), is_bf16, int(timelast),
                self.S, self.C, self.G, B, WIN, stride, self.nproc,
                self._dstate_ptr(), self._dstate_gather_extra,
                hip.stream_ptr()), "tskd_preproc_window_gather")
            if znormalize:
                # opt-in z-normalize per (stream, batch, channel) window row
                # (NOT reference semantics — see SURVEY.md §7 fidelity note).
                assert not timelast, "znormalize needs channel-major windows"
                hip.check(lib.tskd_preproc_window_znorm(
                    hip.ptr(out), is_bf16, self.S * B * self.C, WIN, zeps,
                    hip.stream_ptr()), "tskd_preproc_window_znorm")
        else:
            pr = self.proc.numpy()
            if provided:
                out.zero_()  # pre-grid-0 windows must read zero, not stale
            for b in range(B):
                wend = self.nproc - (B - 1 - b) * stride
                if wend - WIN < 0:
                    continue
                idx = (np.arange(wend - WIN, wend)) % self.G
                w = torch.from_numpy(pr[:, :, idx]).to(dtype)
                out[:, b] = w.transpose(-1, -2) if timelast else w
            if znormalize:
                assert not timelast
                m = out.float().mean(dim=-1, keepdim=True)
                sd = out.float().std(dim=-1, unbiased=False, keepdim=True)
                out.copy_(((out.float() - m) / sd.clamp_min(zeps)).to(dtype))
        return out

    def score_latest(self, model_engine, age: Optional[torch.Tensor] = None,
                     apply_sigmoid: bool = True) -> torch.Tensor:
        """(S, 1) scores of every stream's latest model window, computed by
        the fused serving-tail kernel straight from the ``proc`` ring (no
        window tensor is materialised). Same result as ``windows(batch=1,
        dtype=bf16, timelast=True)`` + ``model_engine.forward``; capture-
        safe (ring position from the device state block when one is set)."""
        assert self._gpu and self.model_win == 120
        self._check_floor(self.model_win)
        return model_engine.score_ring(
            self.proc, self.G, self.nproc, self._dstate_ptr(),
            self._dstate_gather_extra, age, apply_sigmoid)

    # ------------------------------------------------------------- attribution
    def attribute_latest(self, model_engine, sids=None,
                         age: Optional[torch.Tensor] = None,
                         baseline: str = "hold",
                         apply_sigmoid: bool = True) -> torch.Tensor:
        """Occlusion scores of the listed streams' latest model windows (all
        S streams when ``sids`` is None): fp32 ``(n, C + 1)``, one row per
        listed id. Column 0 is the score of the window as it stands (what
        ``score_latest`` returns); column k is the score with channel k - 1
        replaced for all ``model_win`` points by a constant: the window's
        oldest point (``baseline="hold"``: a flat line, the forward-fill
        carry of a lead that fell off ten minutes ago) or +0.0 (``"zero"``:
        the ``fillna(0)`` of a channel that never arrived). ``out[:, 0] -
        out[:, c + 1]`` is channel c's attribution: positive when its actual
        course raised the score. Occlusion against the pipeline's own two
        imputation baselines, not a causal claim.

        ``age``: ``(S, 1)`` / ``(S,)`` indexed by stream id, or None.
        Duplicate ids are harmless, an empty list launches nothing. Runs the
        fused kernel when ``model_engine.supports_attribution(C)``, else
        :meth:`attribute_reference` in fp32. The ring position is passed by
        value (legal between graph replays, not captured). ValueError: an id
        outside [0, S), an unknown baseline, no full model window yet, or a
        window that reaches below the restore floor."""
        assert self._dstate is None, "not inside a device_state block"
        if not model_engine.supports_attribution(self.C):
            return self.attribute_reference(model_engine, sids, age, baseline,
                                            apply_sigmoid)
        ids, age = self._attribution_args(sids, age, baseline)
        dids = torch.from_numpy(ids.astype(np.int32)).to(self.device)
        return model_engine.attribute_ring(
            self.proc, self.G, self.nproc, dids, age, baseline, apply_sigmoid)

    def _attribution_args(self, sids, age, baseline):
        """Checked arguments of an attribution call: (int64 ids, age rows of
        those ids as (n, 1) or None)."""
        from tskd_amd.ops import BASELINES
        assert self.model_win == 120
        if baseline not in BASELINES:
            raise ValueError(f"baseline {baseline!r} not in {list(BASELINES)}")
        ids = np.arange(self.S, dtype=np.int64) if sids is None \
            else self._check_sids(sids)
        if self.nproc < self.model_win:
            raise ValueError(f"no full model window yet: {self.nproc} of "
                             f"{self.model_win} grid points")
        self._check_floor(self.model_win)
        if age is not None:
            age = age.reshape(self.S, 1)[
                torch.from_numpy(ids).to(age.device)]
        return ids, age

    def attribute_reference(self, model_engine, sids=None,
                            age: Optional[torch.Tensor] = None,
                            baseline: str = "hold",
                            apply_sigmoid: bool = True,
                            dtype: torch.dtype = torch.float32
                            ) -> torch.Tensor:
        """:meth:`attribute_latest` from existing pieces only: gather the
        windows, copy each listed stream's C + 1 times with one channel
        overwritten per copy, score the copies as independent one-window
        sequences with ``model_engine.forward``. The fallback for engines
        the kernel does not cover (CPU, MyCNN2/3) and the kernel's oracle:
        with ``dtype=torch.bfloat16`` the windows are the time-last bf16
        ones the serving path scores, and the constant overwrites bf16
        values, which is what converting a flat fp32 channel gives."""
        ids, age = self._attribution_args(sids, age, baseline)
        timelast = dtype == torch.bfloat16
        w = self.windows(batch=1, dtype=dtype, timelast=timelast)
        x = w[torch.from_numpy(ids).to(w.device)]       # (n, 1, ...)
        if timelast:
            x = x.transpose(-1, -2)                      # (n, 1, C, WIN) view
        n, C = len(ids), self.C
        v = x.unsqueeze(1).repeat(1, C + 1, 1, 1, 1)     # (n, C+1, 1, C, WIN)
        for k in range(1, C + 1):
            v[:, k, 0, k - 1, :] = 0.0 if baseline == "zero" \
                else x[:, 0, k - 1, :1]
        if timelast:
            v = v.transpose(-1, -2).contiguous()
        v = v.reshape(n * (C + 1), 1, *v.shape[-2:])
        if age is not None:
            age = age.to(torch.float32).repeat_interleave(C + 1, dim=0)
        if n == 0:
            return torch.empty(0, C + 1, device=self.device)
        out = model_engine.forward(v, age, apply_sigmoid=apply_sigmoid)
        return out.reshape(n, C + 1).to(torch.float32)

    # ------------------------------------------------------------ risk history
    def score_history(self, model_engine, sids=None, k: int = 8,
                      stride: int = 12, age: Optional[torch.Tensor] = None,
                      apply_sigmoid: bool = True) -> torch.Tensor:
        """Scores of the listed streams (all S when ``sids`` is None) at the
        last ``k`` trigger positions the ring still holds: fp32 ``(n, k)``,
        one row per listed id, oldest first (the order of ``windows()``'
        batch axis). Column j is the window ending at ``e_j = nproc -
        (k-1-j)*stride``, scored as serving scores it (``score_latest`` at
        ``nproc = e_j``): every window is its own one-step sequence, not a
        step of an LSTM scan over the batch. A processed point never changes
        once written, so this is the score a daemon that triggers every
        ``stride`` grid points produced there.

        With ``lo = max(0, nproc - G, restore floor)``, column j is
        available iff ``e_j - model_win >= lo``; the unavailable columns are
        a prefix and come back NaN. Per-occupant validity is not the
        engine's business: a slot reused after ``reset_streams`` holds zeros
        below its new occupant's ``born``, and the caller masks the columns
        with ``e_j - model_win < born[sid]``.

        ``age``: ``(S, 1)`` / ``(S,)`` indexed by stream id, or None; one age
        serves all columns of a stream. Duplicate ids are harmless, an empty
        list launches nothing. Runs the fused kernel when
        ``model_engine.supports_history(C)``, else
        :meth:`score_history_reference` in fp32. The ring position is passed
        by value (legal between graph replays, not captured). ValueError: an
        id outside [0, S), ``k < 1``, ``stride < 1``, no full model window
        yet, or a newest window that reaches below the restore floor."""
        assert self._dstate is None, "not inside a device_state block"
        if not model_engine.supports_history(self.C):
            return self.score_history_reference(
                model_engine, sids, k, stride, age, apply_sigmoid)
        ids, age, jmin = self._history_args(sids, k, stride, age)
        dids = torch.from_numpy(ids.astype(np.int32)).to(self.device)
        return model_engine.history_ring(
            self.proc, self.G, self.nproc, dids, k, stride, jmin, age,
            apply_sigmoid)

    def _history_args(self, sids, k, stride, age):
        """Checked arguments of a history call: (int64 ids, age rows of those
        ids as (n, 1) or None, number of unavailable leading columns)."""
        assert self.model_win == 120
        k, stride = int(k), int(stride)
        if k < 1:
            raise ValueError(f"k={k}: at least one column")
        if stride < 1:
            raise ValueError(f"stride={stride}: at least one grid point")
        ids = np.arange(self.S, dtype=np.int64) if sids is None \
            else self._check_sids(sids)
        if self.nproc < self.model_win:
            raise ValueError(f"no full model window yet: {self.nproc} of "
                             f"{self.model_win} grid points")
        self._check_floor(self.model_win)
        lo = max(0, self.nproc - self.G, self._proc_floor)
        room = self.nproc - self.model_win - lo
        if room < 0:
            raise ValueError(f"the ring (G={self.G}) is shorter than a "
                             f"model window of {self.model_win}")
        jmin = k - min(k, room // stride + 1)
        if age is not None:
            age = age.reshape(self.S, 1)[
                torch.from_numpy(ids).to(age.device)]
        return ids, age, jmin

    def score_history_reference(self, model_engine, sids=None, k: int = 8,
                                stride: int = 12,
                                age: Optional[torch.Tensor] = None,
                                apply_sigmoid: bool = True,
                                dtype: torch.dtype = torch.float32
                                ) -> torch.Tensor:
        """:meth:`score_history` from existing pieces only: gather the
        available columns of every stream with ``windows(batch=k - jmin)``
        (by construction within that method's ring and floor bounds), take
        the listed rows, score each window as its own one-window sequence
        with ``model_engine.forward`` and prefix the NaN columns. The
        fallback for engines the kernel does not cover (CPU, MyCNN2/3) and
        the kernel's oracle: with ``dtype=torch.bfloat16`` the windows are
        the time-last bf16 ones the serving path scores."""
        ids, age, jmin = self._history_args(sids, k, stride, age)
        n, nav = len(ids), int(k) - jmin
        out = torch.full((n, int(k)), float("nan"), dtype=torch.float32,
                         device=self.device)
        if n == 0:
            return out
        w = self.windows(batch=nav, stride=int(stride), dtype=dtype,
                         timelast=dtype == torch.bfloat16)
        x = w[torch.from_numpy(ids).to(w.device)]        # (n, nav, ...)
        x = x.reshape(n * nav, 1, *x.shape[-2:])
        if age is not None:
            age = age.to(torch.float32).repeat_interleave(nav, dim=0)
        y = model_engine.forward(x, age, apply_sigmoid=apply_sigmoid)
        out[:, jmin:] = y.reshape(n, nav).to(torch.float32)
        return out

    @property
    def ready(self) -> bool:
        """A full model window exists (>= 600 s + 180 s of data SINCE THE
        STREAM BEGAN, matching the reference's ~10-minutes-to-first-
        prediction behavior — origin-relative so wall-clock event times
        behave the same as zero-based replay times)."""
        return self._forced_ready or \
            self.nproc - self._origin_nproc >= self.model_win

    # --------------------------------------------------------------- lifecycle
    def _check_sids(self, sids) -> np.ndarray:
        """``sids`` as an int64 array, every id in [0, S) — else ValueError
        (an out-of-range id must never reach a kernel)."""
        ids = np.asarray(
            sids.cpu() if isinstance(sids, torch.Tensor) else sids)
        if ids.size == 0:
            return np.empty(0, dtype=np.int64)
        if ids.dtype.kind not in "iu":
            raise ValueError(f"stream ids must be integers, got {ids.dtype}")
        ids = ids.astype(np.int64).reshape(-1)
        if ids.min() < 0 or ids.max() >= self.S:
            raise ValueError(
                f"stream id out of range [0, {self.S}): "
                f"{int(ids.min())}..{int(ids.max())}")
        return ids

    def reset_streams(self, sids) -> None:
        """Return the listed stream slots to the never-used state: bucket
        sums, bucket counts and processed points 0, fill carry NaN — what a
        slot holds before any patient has used it, so the next occupant
        inherits nothing. Duplicates are harmless; an empty list is a no-op.
        Reads no ring position (legal between graph replays). Does not
        touch ``born``: a slot may sit free long before it is re-admitted."""
        ids = self._check_sids(sids)
        if ids.size == 0:
            return
        if self._gpu:
            dids = torch.from_numpy(ids.astype(np.int32)).to(self.device)
            hip.check(hip.load(hip.PREPROC).tskd_preproc_reset_streams(
                hip.ptr(dids), int(ids.size), hip.ptr(self.bsum),
                hip.ptr(self.bcnt), hip.ptr(self.proc),
                hip.ptr(self.last_val), self.S, self.C, self.G, self._bst,
                hip.stream_ptr()), "tskd_preproc_reset_streams")
        else:
            idx = torch.from_numpy(np.unique(ids))
            self.bsum[idx] = 0
            self.bcnt[idx] = 0
            self.proc[idx] = 0
            self.last_val[idx] = float("nan")
        if self.rej is not None:
            self.rej[torch.from_numpy(ids).to(self.device)] = 0

    def rejected(self, sids=None) -> torch.Tensor:
        """Samples the signal-quality gate rejected since the engine began
        (or since the slot's last ``reset_streams``): int64 ``(n, C)`` per
        listed stream (all S when ``sids`` is None) and wire channel, on the
        engine's device. Rows follow the list order, duplicates are
        harmless. NaN samples and late events are not in it. The counter is
        not part of a snapshot: a restored engine counts from 0. ValueError:
        an engine built without ``valid_range``, or an id outside [0, S)."""
        if self.rej is None:
            raise ValueError("this engine has no signal-quality gate "
                             "(built without valid_range)")
        if sids is None:
            return self.rej.clone()
        ids = self._check_sids(sids)
        return self.rej[torch.from_numpy(ids).to(self.device)]

    def admit(self, sids, at=None) -> None:
        """A new occupant takes the listed slots now: ``stream_ready`` for
        them counts a full model window from the current grid point.
        ``at``: optional per-slot grid point (the bucket of the occupant's
        first sample) to count from instead when it lies AHEAD of the
        current one — the warm-up then holds 120 points of the occupant's
        own data however long the grid stood still before it arrived."""
        ids = self._check_sids(sids)
        if ids.size:
            born = np.full(ids.shape, self.nproc, dtype=np.int64)
            if at is not None:
                born = np.maximum(born, np.asarray(at, dtype=np.int64))
            self.born[ids] = born

    def stream_ready(self, sids=None) -> np.ndarray:
        """Per-stream ``ready``: bool mask over ``sids`` (all S streams when
        None) — a full model window has been produced since the stream's
        occupant was admitted (the reference's per-key "waiting until there
        are 120 signals" gate, predictStream.py:117-127). With ``admit``
        never called every entry equals ``ready``."""
        born = self.born if sids is None else self.born[self._check_sids(sids)]
        if self._forced_ready:
            return np.ones(born.shape, dtype=bool)
        return self.nproc - np.maximum(born, self._origin_nproc) \
            >= self.model_win

    def force_ready(self) -> None:
        """Declare the engine warm (steady-state serving): benchmarks that
        measure per-trigger latency of a long-running server call this to
        skip the reference's ~13-minute first-window ramp (windows shorter
        than 600 s are zero-padded, exactly as mid-history windows are)."""
        self._forced_ready = True

    # ---------------------------------------------------------------- coverage
    def coverage(self, sids=None) -> torch.Tensor:
        """How much of the latest model window rests on samples: int32
        ``(n, C, 3)`` = ``[present, imputed, stale]`` per listed stream (all
        S when ``sids`` is None) and channel, on the engine's device.

        The window's ``model_win`` grid points ``[lo, nproc)``, ``lo = nproc
        - model_win``, average the ``span = model_win + win_buckets - 1``
        buckets ``[lo, hi)``, ``hi = nproc + win_buckets - 1``. A bucket
        ``b`` is present iff its count is > 0 or ``b`` lies below the restore
        floor (the snapshot's ``nproc`` on a restored engine: buckets below
        it were not carried over, and unknown counts as present).

        - ``present``: present buckets in ``[lo, hi)``;
        - ``imputed``: grid points ``g`` in ``[lo, nproc)`` with no present
          bucket in ``[g, g + win_buckets)`` — model inputs that are a
          forward-filled carry, a back-filled prefix or a literal 0;
        - ``stale``: length of the run of non-present buckets ending at
          ``hi - 1`` (0 when that bucket is present, ``span`` when none is);
          ``stale * bucket_s`` bounds the newest sample's age from below.

        The numbers describe the buckets as they stand at the call: a late
        event accepted into a bucket >= ``nproc`` after an earlier grid
        point already consumed that bucket shows as present.

        Raises ValueError before the first full model window (``nproc <
        model_win``) and when the span is no longer wholly in the ring (a
        catch-up skip, or samples far ahead of the watermark, cleared the
        slots of its oldest buckets). Duplicate ids are harmless, rows
        follow the list order, an empty list launches nothing. Ring
        positions are passed by value (legal between graph replays, not
        captured)."""
        assert self._dstate is None, "not inside a device_state block"
        ids = None if sids is None else self._check_sids(sids)
        L, Wb = self.model_win, self.win_buckets
        if self.nproc < L:
            raise ValueError(
                f"no full model window yet: {self.nproc} of {L} grid points")
        lo, span = self.nproc - L, L + Wb - 1
        if max(self.head, self._cleared) - lo > self.G:
            raise ValueError(
                f"the window's buckets [{lo}, {lo + span}) are no longer "
                f"wholly in the ring (G={self.G}, written up to bucket "
                f"{max(self.head, self._cleared)})")
        n = self.S if ids is None else int(ids.size)
        out = torch.empty((n, self.C, 3), dtype=torch.int32,
                          device=self.device)
        if n == 0:
            return out
        if self._gpu:
            dids = None if ids is None else \
                torch.from_numpy(ids.astype(np.int32)).to(self.device)
            hip.check(hip.load(hip.PREPROC).tskd_preproc_window_coverage(
                hip.ptr(self.bcnt), self._bst, hip.ptr(dids), n, self.S,
                self.C, self.G, self.nproc, L, Wb, self._bucket_floor,
                hip.ptr(out), hip.stream_ptr()),
                "tskd_preproc_window_coverage")
            return out
        bidx = (lo + np.arange(span)) % self.G
        cnt = self.bcnt.numpy()[:, :, bidx]
        pres = (cnt if ids is None else cnt[ids]) > 0        # (n, C, span)
        pres[:, :, :min(max(self._bucket_floor - lo, 0), span)] = True
        # present buckets per window [g, g + Wb): differences of a prefix sum
        cs = np.zeros(pres.shape[:2] + (span + 1,), dtype=np.int64)
        np.cumsum(pres, axis=-1, out=cs[:, :, 1:])
        rev = pres[:, :, ::-1]
        res = np.stack([
            cs[:, :, -1],
            (cs[:, :, Wb:] == cs[:, :, :L]).sum(-1),
            np.where(rev.any(-1), rev.argmax(-1), span)], axis=-1)
        out.copy_(torch.from_numpy(res.astype(np.int32)))
        return out

    # ------------------------------------------------------------ warm restart
    def _geometry(self) -> dict:
        return {"C": self.C, "fs": self.fs, "bucket_s": self.bucket_s,
                "win_buckets": self.win_buckets, "model_win": self.model_win}

    def _check_floor(self, reach: int) -> None:
        """A gather reaching ``reach`` grid points back from the latest one
        must stay above the restore floor: below it a restored engine holds
        zeros where an uninterrupted one holds data."""
        end = self.nproc + self._dstate_gather_extra
        if max(end - reach, 0) < self._proc_floor:
            raise ValueError(
                f"window reaches back to grid point {max(end - reach, 0)} "
                f"but this engine was restored with processed points from "
                f"{self._proc_floor} on only (snapshot with a larger keep)")

    def _snap_buffers(self, numel: int):
        """The reused device staging and pinned host buffers, grown to hold
        ``numel`` floats."""
        if self._snap_dev is None or self._snap_dev.numel() < numel:
            cap = numel + numel // 4
            self._snap_dev = torch.empty(cap, device=self.device)
            self._snap_host = torch.empty(cap, pin_memory=True)
        return self._snap_dev[:numel], self._snap_host[:numel]

    def snapshot(self, sids=None, keep: Optional[int] = None
                 ) -> EngineSnapshot:
        """The live tail of the listed streams' rings (all S streams when
        ``sids`` is None) with the ring indices and geometry: per stream and
        channel the ``nbk`` = max(head, cleared) - nproc (sum, cnt) bucket
        pairs from ``nproc`` on, the last ``keep`` processed points and the
        fill carry, each ring range unwrapped to linear grid order. That is
        all ``restore`` needs to continue on a fresh engine exactly as this
        one would.

        ``keep`` defaults to ``model_win`` (or the points produced so far,
        if fewer): enough for ``windows(batch=1)``. Raise it, up to
        ``G - win_buckets`` (one model window is always allowed), when the
        restored engine must serve batched windows reaching further back.

        GPU: one launch into a reused device buffer and one copy into a
        reused pinned host buffer; the returned ``payload`` is a view of
        that host buffer, valid until this engine's next ``snapshot``.
        Duplicate ids are harmless. Reads host ring positions only (legal
        between graph replays)."""
        assert self._dstate is None, "not inside a device_state block"
        ids = np.arange(self.S, dtype=np.int64) if sids is None \
            else self._check_sids(sids)
        have = self.nproc - self._proc_floor
        if keep is None:
            keep = min(self.model_win, have,
                       max(0, self.nproc - self._origin_nproc))
        keep = int(keep)
        # one model window always fits (windows() needs model_win <= G)
        cap = min(max(self.G - self.win_buckets, min(self.model_win, self.G)),
                  have)
        if not 0 <= keep <= cap:
            raise ValueError(
                f"keep={keep} outside [0, {cap}]: G - win_buckets (or one "
                f"model window) at the most, and this engine holds {have} "
                f"processed points")
        nbk = max(self.head, self._cleared) - self.nproc
        assert 0 <= nbk <= self.G, (self.head, self._cleared, self.nproc)
        n, R = int(ids.size), 2 * nbk + keep + 1
        if n == 0:
            payload = np.empty((0, self.C, R), dtype=np.float32)
        elif self._gpu:
            dids = torch.from_numpy(ids.astype(np.int32)).to(self.device)
            dev, host = self._snap_buffers(n * self.C * R)
            hip.check(hip.load(hip.PREPROC).tskd_preproc_snapshot_streams(
                hip.ptr(dids), n, hip.ptr(self.bsum), hip.ptr(self.bcnt),
                hip.ptr(self.proc), hip.ptr(self.last_val), self.S, self.C,
                self.G, self._bst, self.nproc, nbk, keep, hip.ptr(dev),
                hip.stream_ptr()), "tskd_preproc_snapshot_streams")
            host.copy_(dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            payload = host.numpy().reshape(n, self.C, R)
        else:
            payload = np.empty((n, self.C, R), dtype=np.float32)
            ch = np.arange(self.C)
            bidx = (self.nproc + np.arange(nbk)) % self.G
            pidx = (self.nproc - keep + np.arange(keep)) % self.G
            payload[:, :, 0:2 * nbk:2] = \
                self.bsum.numpy()[np.ix_(ids, ch, bidx)]
            payload[:, :, 1:2 * nbk:2] = \
                self.bcnt.numpy()[np.ix_(ids, ch, bidx)]
            payload[:, :, 2 * nbk:2 * nbk + keep] = \
                self.proc.numpy()[np.ix_(ids, ch, pidx)]
            payload[:, :, -1] = self.last_val.numpy()[ids]
        return EngineSnapshot(
            geometry=self._geometry(), head=self.head, nproc=self.nproc,
            cleared=self._cleared, origin_nproc=self._origin_nproc,
            forced_ready=self._forced_ready, nbk=nbk, keep=keep, sids=ids,
            born=self.born[ids].copy(), payload=payload)

    def restore(self, snap: EngineSnapshot, sid_map=None) -> None:
        """Continue where ``snap`` was taken: scatter its records into the
        rings and take over its ring indices and ``born``. Only on a fresh
        engine (nothing ingested yet) of the same geometry; ring length,
        stream count and bucket packing may differ from the source's.
        ``sid_map``: {source stream id: target slot} for every snapshot
        stream (default: the same ids). Every check runs before anything is written, so a
        ValueError leaves the engine fresh. Processed points older than
        ``nproc - keep`` are not carried over: ``windows`` refuses to reach
        below that floor."""
        if self.head or self.nproc or self._cleared:
            raise ValueError("restore needs a fresh engine "
                             f"(head={self.head}, nproc={self.nproc})")
        mine = self._geometry()
        for k in GEOMETRY:
            if snap.geometry.get(k) != mine[k]:
                raise ValueError(f"geometry mismatch: {k} is "
                                 f"{snap.geometry.get(k)} in the snapshot, "
                                 f"{mine[k]} here")
        nbk, keep, nproc = int(snap.nbk), int(snap.keep), int(snap.nproc)
        if not (0 <= keep <= nproc and nbk >= 0
                and nbk == max(snap.head, snap.cleared) - nproc):
            raise ValueError("inconsistent snapshot indices")
        if keep > self.G or nbk > self.G:
            raise ValueError(
                f"snapshot tail (nbk={nbk}, keep={keep}) does not fit a ring "
                f"of G={self.G}")
        src = np.asarray(snap.sids, dtype=np.int64).reshape(-1)
        if sid_map is None:
            dst = src
        else:
            try:
                dst = np.asarray([sid_map[int(s)] for s in src])
            except KeyError as e:
                raise ValueError(f"sid_map lacks source stream {e}") from e
        n, R = int(src.size), 2 * nbk + keep + 1
        payload = np.asarray(snap.payload)
        if payload.shape != (n, self.C, R) \
                or payload.dtype != np.float32 or len(snap.born) != n:
            raise ValueError("snapshot arrays do not match its stream list")
        dst = self._check_sids(dst)
        if np.unique(dst).size != n:
            raise ValueError("duplicate target stream ids")
        if n and self._gpu:
            dids = torch.from_numpy(dst.astype(np.int32)).to(self.device)
            rec = torch.from_numpy(np.ascontiguousarray(payload)) \
                .to(self.device)
            hip.check(hip.load(hip.PREPROC).tskd_preproc_restore_streams(
                hip.ptr(dids), n, hip.ptr(self.bsum), hip.ptr(self.bcnt),
                hip.ptr(self.proc), hip.ptr(self.last_val), self.S, self.C,
                self.G, self._bst, nproc, nbk, keep, hip.ptr(rec),
                hip.stream_ptr()), "tskd_preproc_restore_streams")
        elif n:
            ch = np.arange(self.C)
            bidx = (nproc + np.arange(nbk)) % self.G
            pidx = (nproc - keep + np.arange(keep)) % self.G
            self.bsum.numpy()[np.ix_(dst, ch, bidx)] = \
                payload[:, :, 0:2 * nbk:2]
            self.bcnt.numpy()[np.ix_(dst, ch, bidx)] = \
                payload[:, :, 1:2 * nbk:2]
            self.proc.numpy()[np.ix_(dst, ch, pidx)] = \
                payload[:, :, 2 * nbk:2 * nbk + keep]
            self.last_val.numpy()[dst] = payload[:, :, -1]
        self.head, self.nproc = int(snap.head), nproc
        self._cleared = int(snap.cleared)
        self._origin_nproc = int(snap.origin_nproc)
        self._forced_ready = self._forced_ready or bool(snap.forced_ready)
        self.born[dst] = np.asarray(snap.born, dtype=np.int64)
        self._proc_floor = nproc - keep
        self._bucket_floor = nproc


class TriggerGraph:
    """ONE hipGraph for the whole serving trigger — fused preprocess +
    inference (BASELINE config 4: "fused preprocess+inference hipGraph"):
    ingest -> window_fill -> window_gather (into the model graph's static
    input) -> MFMA conv -> LSTM/head/sigmoid -> device ring-index advance.

    Ring indices live in a device int64[2] state block the captured kernels
    read, so one replay per 60-s trigger advances the rings with ZERO host
    work besides the replay call. Requires steady state (every trigger
    produces exactly NB new grid points) and a stable channel map.

    Fused tail (default; ``TSKD_FUSED_TAIL=0`` at capture time turns it
    off): when the model graph's input is a bf16 timelast buffer with one
    window per stream and the variant supports it (even channel count equal
    to the engine's: MyCNN5, MyCNN4), gather -> conv -> LSTM/head collapse
    into ONE kernel that reads the ``proc`` ring (``score_latest``). In
    that mode ``graphed_forward.x`` is NOT written; only ``.age`` is read.
    """

    def __init__(self, engine: "StreamEngine", raw: torch.Tensor,
                 chan_map, graphed_forward, stride: int = 12,
                 overlap: bool = False):
        assert engine._gpu, "TriggerGraph needs a CUDA StreamEngine"
        cin, t = raw.shape[1], raw.shape[2]
        self.nb = t // engine.bucket_len
        assert engine.nproc == engine.head - engine.win_buckets + 1, \
            "engine must be in steady state (warm up with eager triggers)"
        self.engine = engine
        self.raw = raw.contiguous()
        self.gf = graphed_forward
        self.stride = stride
        self.chan_map = list(chan_map)
        self.overlap = overlap
        gf = graphed_forward
        self.fused_tail = (
            os.environ.get("TSKD_FUSED_TAIL", "1") != "0"
            and gf.x.dtype == torch.bfloat16
            and getattr(gf, "timelast", False) and gf.x.shape[1] == 1
            and engine.model_win == 120
            and gf.engine.supports_fused_tail(engine.C))
        dev = engine.device
        self.dstate = torch.tensor([engine.head, engine.nproc],
                                   dtype=torch.int64, device=dev)
        if overlap:
            self._init_overlap()
            return
        # warm side-stream run, then capture
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            self._body(True, True)
        torch.cuda.current_stream().wait_stream(stream)
        # the warm run advanced device state AND rings once; mirror it
        engine.head += self.nb
        engine.nproc += self.nb
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._body(True, True)

    def _body(self, ingest: bool, model: bool) -> Optional[torch.Tensor]:
        """The capturable launch sequence: the ingest stage, the model
        stage (fill + score), or both, then ONE ring-index advance of the
        stage(s) run. The gather/fused tail runs AFTER the fill and BEFORE
        the advance, hence window end = nproc + nb."""
        engine, nb, out = self.engine, self.nb, None
        with engine.device_state(self.dstate, nb if model else 0):
            if ingest:
                engine.ingest_graph_kernel(self.raw, self.chan_map)
            if model:
                engine.fill_graph_kernel(nb)
                out = self._score()
            hip.check(hip.load(hip.PREPROC).tskd_preproc_advance_state(
                hip.ptr(self.dstate), nb if ingest else 0,
                nb if model else 0, hip.stream_ptr()),
                "tskd_preproc_advance_state")
        return out

    def _score(self) -> torch.Tensor:
        """Latest-window scores inside a trigger body (after the fill):
        the fused tail kernel, or gather into gf.x + conv + LSTM/head."""
        gf = self.gf
        if self.fused_tail:
            return self.engine.score_latest(gf.engine, gf.age,
                                            apply_sigmoid=True)
        self.engine.windows(batch=1, stride=self.stride, dtype=gf.x.dtype,
                            out=gf.x,
                            timelast=getattr(gf, "timelast", False))
        return gf.engine.forward(gf.x, gf.age, apply_sigmoid=True)

    def _init_overlap(self) -> None:
        """Two-stream software-pipelined trigger: ingest(T+1) overlaps the
        fill/gather/model chain of trigger T on a second HIP stream.

        Legality: ingest(T+1) writes buckets [head_T, head_T + NB) while
        fill(T) reads [nproc_T, nproc_T + NB + win - 1) = up to head_T - 1
        — disjoint ring regions (and G >> the combined span). The device
        ring indices split: the ingest graph advances dstate[0] (head)
        only, the model graph advances dstate[1] (nproc) only, so each
        stream owns its own index. A CUDA event orders model(T) after
        ingest(T); nothing orders ingest(T+1) after model(T).

        Raises per-trigger latency not at all (probe with replay()+sync);
        raises steady-state throughput by overlapping the HBM-bound ingest
        with the compute-bound model chain.
        """
        engine, nb = self.engine, self.nb
        self._sA = torch.cuda.Stream()
        self._sB = torch.cuda.Stream()
        # warm one full trigger (ingest then model), mirroring host indices
        with torch.cuda.stream(self._sA):
            self._body(True, False)
        self._sB.wait_stream(self._sA)
        with torch.cuda.stream(self._sB):
            self._body(False, True)
        torch.cuda.current_stream().wait_stream(self._sB)
        engine.head += nb
        engine.nproc += nb
        self.graph_i = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_i, stream=self._sA):
            self._body(True, False)
        self.graph_m = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_m, stream=self._sB):
            self.out = self._body(False, True)
        self._evA = torch.cuda.Event()

    def replay(self, raw_refresh: bool = False) -> torch.Tensor:
        """One serving trigger: caller refreshed self.raw in place."""
        if self.overlap:
            # ingest(T) launches on stream A; model(T) on stream B waits it
            # (event). The NEXT call's ingest(T+1) waits only stream A's own
            # order — it overlaps model(T). Pass raw_refresh=True when the
            # caller rewrote self.raw since the previous call: it orders
            # ingest(T) after the caller's stream (serializing the pipeline
            # but keeping the refresh race-free).
            cur = torch.cuda.current_stream()
            if raw_refresh:
                self._sA.wait_stream(cur)
            with torch.cuda.stream(self._sA):
                self.graph_i.replay()
                self._evA.record(self._sA)
            self._sB.wait_event(self._evA)
            self._sB.wait_stream(cur)   # previous output consumed on cur
            with torch.cuda.stream(self._sB):
                self.graph_m.replay()
            cur.wait_stream(self._sB)   # consumers on cur see trigger T
            self.engine.head += self.nb
            self.engine.nproc += self.nb
            return self.out
        self.graph.replay()
        self.engine.head += self.nb      # host mirrors (bookkeeping only)
        self.engine.nproc += self.nb
        return self.out

"""Fused serving daemon — the production deployment mode.

Collapses processStream + predictStream into ONE process per GPU: raw
channel topics are drained from the bus (native wire parse), ingested into
the GPU StreamEngine ring buffers, and every trigger runs the fused
preprocess -> window-gather -> MFMA conv -> LSTM -> sigmoid path; risk
scores land in the prediction store (and optionally a response topic).
The two-stage CLIs (processstream | predictstream) remain available for the
reference's exact topology including the `call-stream` wire contract; this
daemon is the latency/throughput-optimal arrangement.

Scale-out: under torchrun (one rank per GPU), patient streams are sharded
by consistent hash (tskd_amd.parallel.shard_for_key) — each rank ignores
messages outside its shard — and per-trigger predictions are all-gathered
over RCCL/xGMI; rank 0 writes the store.

Usage:
    python -m tskd_amd.cli.serve --bus-dir ... --store-path predictions.log
    python -m torch.distributed.run --nproc-per-node 8 --master-addr \
        127.0.0.1 -m tskd_amd.cli.serve ...
"""

from __future__ import annotations

import argparse
import logging
import os
import signal
import time
from typing import Dict, Optional

import torch

from tskd_amd.bus import Bus, Consumer, Producer
from tskd_amd.config import (engine_valid_range, get_global_config,
                             resolve_valid_ranges)
from tskd_amd.engine import EngineSnapshot, StreamEngine
from tskd_amd.metrics import StageTimer
from tskd_amd.models import build_model
from tskd_amd.ops import MyCNNEngine
from tskd_amd.parallel import (all_gather_predictions, init_distributed,
                               shard_for_key)
from tskd_amd.store import AgeTable, PredictionStore

log = logging.getLogger("serve")


class FusedServer:
    def __init__(self, bus: Bus, cfg, store: Optional[PredictionStore],
                 ages: Optional[AgeTable] = None, model=None,
                 device: str = "cpu", max_streams: int = 1024,
                 ring_grid: int = 4096, starting: str = "latest",
                 response_topic: Optional[str] = None,
                 emit_processed: Optional[str] = None,
                 rank: int = 0, world: int = 1,
                 pipelined: bool = False, evict_idle_s: float = 0.0,
                 state_path: Optional[str] = None, snapshot_every: int = 1,
                 min_coverage: float = 0.0,
                 explain_above: Optional[float] = None,
                 explain_baseline: str = "hold", reload_check: int = 0,
                 reload_max_shift: Optional[float] = None,
                 valid_range=None):
        self.cfg = cfg
        # hot-reload vetting (opt-in; 0 = off): before a changed checkpoint
        # goes live, the last reload_check triggers of the live ready slots
        # are scored from the ring under the current and the candidate model
        # (se.score_history) and the shift of the scores is exported; with
        # reload_max_shift a candidate that moves any of them further, or
        # gives a non-finite one, is refused
        self.reload_check = int(reload_check)
        self.reload_max_shift = None if reload_max_shift is None \
            else float(reload_max_shift)
        if self.reload_check < 0:
            raise ValueError(f"reload_check={reload_check} is negative")
        if self.reload_max_shift is not None and self.reload_check < 1:
            raise ValueError("reload_max_shift needs reload_check >= 1")
        # channel attribution (opt-in; None = off, so that a threshold of 0
        # explains every prediction): a persisted prediction with risk >=
        # explain_above is attributed in the same trigger, before
        # the ring moves (se.attribute_latest), and its response-topic JSON
        # carries the per-channel occlusion deltas. Choosing the streams
        # needs the scores on the host, which the pipelined mode defers.
        self.explain_above = None if explain_above is None \
            else float(explain_above)
        self.explain_baseline = explain_baseline
        if explain_baseline not in ("hold", "zero"):
            raise ValueError(f"explain_baseline={explain_baseline!r} is "
                             f"neither 'hold' nor 'zero'")
        if self.explain_above is not None and pipelined:
            raise ValueError("explain_above needs the scores on the host in "
                             "the trigger that made them: not with pipelined")
        # coverage gate (opt-in; 0 = off): a stream whose latest model window
        # holds less than this fraction of inputs that rest on samples (the
        # rest being a carried, back-filled or zero value: se.coverage) is
        # still scored, but its prediction goes neither to the store nor to
        # the response topic
        self.min_coverage = float(min_coverage)
        if not 0.0 <= self.min_coverage <= 1.0:
            raise ValueError(f"min_coverage={min_coverage} outside [0, 1]")
        # warm restart: every snapshot_every-th trigger ends by writing ONE
        # file (save_state) that a successor process resumes from
        # (load_state); None = off
        self.state_path = state_path
        self.snapshot_every = max(1, int(snapshot_every))
        self._n_triggers = 0
        self.store = store
        self.ages = ages or AgeTable()
        self.rank, self.world = rank, world
        self.device = device
        self.me = MyCNNEngine(model or build_model("MyCNN5").eval(),
                              device=device)
        # ring channel space = the MODEL's wire space (config may name fewer
        # channels; the rest stay zero, like the reference's fixed (1,10,120))
        # signal-quality gate (opt-in; None = off): per config channel a
        # closed plausibility interval (lo, hi); a sample outside it that is
        # not NaN is rejected at ingest and the engine counts it (se.rej).
        # Each trigger copies the counter to the host once and feeds the
        # per-channel counters, the gauges and the responses' "rejected"
        # from the delta against the previous copy.
        n_ring = max(cfg.n_channels, self.me.cin)
        if valid_range is not None and len(valid_range) != cfg.n_channels:
            raise ValueError(f"valid_range has {len(valid_range)} entries "
                             f"for {cfg.n_channels} config channels")
        self.se = StreamEngine(max_streams, n_ring,
                               ring_grid=ring_grid, device=device,
                               valid_range=engine_valid_range(valid_range,
                                                              n_ring))
        self._gated = self.se.rej is not None
        if self._gated:
            import numpy as _np
            self._rej_prev = _np.zeros((max_streams, n_ring), _np.int64)
            # per slot: rejected since the slot's last published prediction
            self._rej_since = _np.zeros(max_streams, _np.int64)
        self.consumer = Consumer(bus, starting=starting)
        topics = [cfg.topic_for_channel(c) for c in cfg.channel_names]
        for t in topics:
            bus.create_topic(t)
        self.consumer.subscribe(topics)
        self.producer = Producer(bus) if (response_topic or emit_processed) \
            else None
        self.response_topic = response_topic
        if response_topic:
            bus.create_topic(response_topic)
        # optional call-stream emission so the dashboard's processed plots
        # work in fused mode too (the two-stage wire contract)
        self.emit_processed = emit_processed
        if emit_processed:
            bus.create_topic(emit_processed)
        self.pid_index: Dict[str, int] = {}
        self.pids: list = []
        self.max_streams = max_streams
        # stream lifecycle (opt-in; 0 = off, ids are then never given back):
        # a patient silent for more than evict_idle_s of EVENT time is
        # evicted after a trigger, its ring slot wiped on the GPU and handed
        # to the next new patient. self.pids is then indexed by slot (None =
        # free) and predictions are gated per stream (se.stream_ready).
        # A patient is evicted only once its newest sample also lies behind
        # the processed grid, so nothing of it that is still on its way (a
        # chunk the poll thread holds, a late message) can land in the
        # wiped slot: the engine drops such samples as late.
        self.evict_idle_s = float(evict_idle_s)
        self._lifecycle = self.evict_idle_s > 0.0
        self._slot_version = 0   # bumped whenever pids/pid_index change
        self._poll_kw = dict(max_msgs=131072, timeout_ms=0, rank=rank,
                             world=world, max_streams=max_streams)
        if self._lifecycle:
            self._poll_kw.update(drop_when_full=True)
        self.hwm = 0.0
        self.watermark_s = cfg.watermark_s
        self.timer = StageTimer("serve")
        self.n_predictions = 0
        self.model_path: Optional[str] = None   # set to enable hot reload
        self._model_mtime = 0.0
        # pipelined mode: the bus poll of trigger T+1 overlaps trigger T's
        # asynchronously-launched GPU work; T's predictions persist at the
        # START of trigger T+1 (or at flush()). One trigger of persistence
        # lag bought for consume/compute overlap (north-star: "inference
        # overlapped with Kafka consume").
        self.pipelined = pipelined
        self._pending = None  # (probs_dev, t_us, pids_snapshot)
        # opt-in per-stage decomposition (poll/ingest/model/persist): adds
        # a device sync at each boundary, so ONLY for latency studies
        self.stage_profile = False
        self.stage_ms: Dict[str, list] = {k: [] for k in
                                          ("poll", "ingest", "model",
                                           "persist")}
        # background poll thread (north-star "inference overlapped with
        # consume"): a daemon thread drains+parses the bus continuously so
        # the trigger only ingests/scores — at saturating rates the poll
        # was ~90% of the trigger (profiles/r02 §1). Enable via
        # start_poll_thread(); the Consumer is then owned by that thread.
        import threading as _threading
        self._poll_lock = _threading.Lock()
        self._poll_pending: list = []
        self._poll_thread = None
        self._poll_stop = _threading.Event()

    def start_poll_thread(self, interval_s: float = 0.01) -> None:
        import threading as _threading
        self._poll_error: Optional[BaseException] = None

        def loop():
            try:
                while not self._poll_stop.is_set():
                    chunk = self.consumer.poll_samples_sid(**self._poll_kw)
                    if len(chunk[0]) or chunk[4] or (
                            len(chunk) > 5 and chunk[5] > 0.0):
                        with self._poll_lock:
                            self._poll_pending.append(chunk)
                    else:
                        self._poll_stop.wait(interval_s)
            except BaseException as e:  # surface at the next trigger —
                # a silently-dead poll thread would stall serving
                self._poll_error = e
                log.error("poll thread died: %s", e)

        self._poll_thread = _threading.Thread(target=loop, daemon=True)
        self._poll_thread.start()

    def stop_poll_thread(self) -> None:
        if self._poll_thread is not None:
            self._poll_stop.set()
            self._poll_thread.join(timeout=5)
            self._poll_thread = None

    def _take_polled(self):
        """Concatenate the background thread's pending chunks (or poll
        inline when the thread isn't running)."""
        if self._poll_thread is None:
            return self.consumer.poll_samples_sid(**self._poll_kw)
        if getattr(self, "_poll_error", None) is not None:
            raise RuntimeError("poll thread died") from self._poll_error
        with self._poll_lock:
            chunks, self._poll_pending = self._poll_pending, []
        # lifecycle chunks carry a sixth element (newest rejected time)
        tail = (max((c[5] for c in chunks), default=0.0),) \
            if self._lifecycle else ()
        if not chunks:
            import numpy as _np
            return (_np.empty(0, _np.int32), _np.empty(0, _np.int32),
                    _np.empty(0, _np.float32), _np.empty(0, _np.float64),
                    []) + tail
        if len(chunks) == 1:
            return chunks[0]
        import numpy as _np
        sa = _np.concatenate([c[0] for c in chunks])
        ca = _np.concatenate([c[1] for c in chunks])
        va = _np.concatenate([c[2] for c in chunks])
        ta = _np.concatenate([c[3] for c in chunks])
        nk = [kv for c in chunks for kv in c[4]]
        return (sa, ca, va, ta, nk) + tail

    def _stamp(self, key: Optional[str], t0: float) -> float:
        import time as _time
        if not self.stage_profile:
            return t0
        if self.device != "cpu":
            torch.cuda.synchronize()
        t1 = _time.perf_counter()
        if key is not None:
            self.stage_ms[key].append((t1 - t0) * 1e3)
        return t1

    def maybe_reload_model(self) -> bool:
        """Hot-reload the checkpoint when the file changes (the reference
        loads once at process start and never again — predictStream.py:36).
        Weight repack is ~6 KB; the engine swaps atomically between triggers.
        """
        if not self.model_path or not os.path.exists(self.model_path):
            return False
        mtime = os.path.getmtime(self.model_path)
        if mtime <= self._model_mtime:
            return False
        from tskd_amd.models import load_checkpoint
        try:
            model = load_checkpoint(self.model_path)
        except Exception as e:  # partial write etc. — retry next trigger
            log.warning("hot reload failed (%s); keeping current model", e)
            return False
        cand = MyCNNEngine(model, device=self.device)
        # the file is dealt with either way: a refused one is not vetted
        # again at every trigger
        self._model_mtime = mtime
        if self.reload_check > 0 and not self._vet_reload(cand):
            return False
        self.me = cand
        log.info("hot-reloaded model from %s", self.model_path)
        return True

    def _vet_reload(self, cand: MyCNNEngine) -> bool:
        """Score the last reload_check triggers of the live ready slots
        under the current and the candidate engine, export how far the
        scores move (gauges reload_*) and say whether the candidate may go
        live. Kept entries: columns the ring still holds (not NaN under the
        current model) that lie wholly within the slot's current occupancy.
        The shift figures are taken over the kept entries whose candidate
        score is finite; the others are counted in reload_nonfinite. With
        nothing to compare the swap goes ahead unchecked."""
        import numpy as _np
        se, K = self.se, self.reload_check
        g = self.timer.gauges
        ready = se.stream_ready()
        slots = [i for i, p in enumerate(self.pids)
                 if p is not None and bool(ready[i])]
        cur = new = None
        if slots:
            age = torch.full((se.S, 1), 65.0, device=se.device)
            col = self._age_column()
            age[:col.shape[0]] = col
            try:
                cur = se.score_history(self.me, slots, k=K, stride=12,
                                       age=age, apply_sigmoid=True).cpu()
                new = se.score_history(cand, slots, k=K, stride=12,
                                       age=age, apply_sigmoid=True).cpu()
            except ValueError as e:
                log.warning("reload check unavailable, swapping unchecked: "
                            "%s", e)
                cur = None
        n_kept = 0
        if cur is not None:
            ends = se.nproc - 12 * _np.arange(K - 1, -1, -1)
            since = _np.maximum(se.born[slots], se._origin_nproc)
            keep = torch.from_numpy(
                ends[None, :] - se.model_win >= since[:, None]) \
                & ~torch.isnan(cur)
            n_kept = int(keep.sum())
        if n_kept == 0:
            g["reload_checked_windows"] = 0
            return True
        finite = torch.isfinite(new) & keep
        shift = (new - cur).abs()[finite].double()
        nonfinite = n_kept - int(finite.sum())
        smax = float(shift.max()) if shift.numel() else 0.0
        smean = float(shift.mean()) if shift.numel() else 0.0
        g.update(reload_checked_windows=n_kept, reload_shift_max=smax,
                 reload_shift_mean=smean, reload_nonfinite=nonfinite)
        log.info("reload check: %d windows, shift max %.6f mean %.6f, "
                 "%d non-finite", n_kept, smax, smean, nonfinite)
        if self.reload_max_shift is not None and (
                nonfinite > 0 or smax > self.reload_max_shift):
            g["reload_rejected_total"] = g.get("reload_rejected_total", 0) + 1
            log.warning("hot reload of %s refused: shift max %.6f (limit "
                        "%.6f), %d non-finite; keeping current model",
                        self.model_path, smax, self.reload_max_shift,
                        nonfinite)
            return False
        return True

    def _age_column(self) -> torch.Tensor:
        """(slots in use, 1) ages on the device, cached: the column only
        changes when the slot table does (version counter)."""
        if getattr(self, "_age_ver", -1) != self._slot_version:
            self._age_dev = torch.tensor(
                [[self.ages.get(p) if p is not None else 65.0]
                 for p in self.pids], device=self.se.device)
            self._age_ver = self._slot_version
        return self._age_dev

    def _sid(self, pid: str) -> Optional[int]:
        """Host-side mirror of the native key->sid map (poll_samples_sid
        owns id assignment during serving; this exists for callers that
        query a pid outside a trigger — ids match because both assign
        densely in first-seen order and filter by the same FNV-1a shard)."""
        if self.world > 1 and shard_for_key(pid, self.world) != self.rank:
            return None  # another rank's patient
        if self._lifecycle:
            # the native slot table is the only allocator: look up only
            return self.pid_index.get(pid)
        if pid not in self.pid_index:
            if len(self.pid_index) >= self.max_streams:
                raise RuntimeError("max_streams exceeded")
            self.pid_index[pid] = len(self.pid_index)
            self.pids.append(pid)
            self._slot_version += 1
        return self.pid_index[pid]

    def _drop_evicted(self, pairs) -> None:
        """Forget evicted (key, sid) pairs and wipe their ring slots (one
        reset launch) so the next occupant inherits nothing."""
        if not pairs:
            return
        for key, sid in pairs:
            if self.pid_index.get(key) == sid:
                del self.pid_index[key]
            if sid < len(self.pids) and self.pids[sid] == key:
                self.pids[sid] = None
        self._slot_version += 1
        sids = [sid for _k, sid in pairs]
        self.se.reset_streams(sids)     # zeroes the slots' rej rows too
        if self._gated:
            self._rej_prev[sids] = 0
            self._rej_since[sids] = 0

    def _admit(self, new_keys, sa, ta) -> None:
        """Admit the trigger's new patients: each one's warm-up counts from
        the bucket of its first sample that the engine will accept (one
        behind the processed grid is dropped as late), never from before
        the current grid point."""
        import numpy as _np
        live = ta >= self.se.nproc * self.se.bucket_s
        first = _np.full(self.se.S, _np.inf)
        _np.minimum.at(first, sa[live], ta[live])
        sids = _np.asarray([sid for _k, sid in new_keys], dtype=_np.int64)
        t_first = first[sids]
        t_first[~_np.isfinite(t_first)] = 0.0   # no live sample: from now
        self.se.admit(sids, at=(t_first // self.se.bucket_s).astype(
            _np.int64))

    def _count_rejected(self) -> None:
        """One device-to-host copy of the engine's rejected counter; its
        delta against the previous copy goes to the per-channel counters
        (tskd_rejected_samples_total), the gauges and the per-slot tally
        that the next published prediction of the slot reports."""
        n = len(self.pids)
        nc = self.cfg.n_channels
        cur = self.se.rej[:n].cpu().numpy()
        delta = cur - self._rej_prev[:n]
        self._rej_prev[:n] = cur
        self._rej_since[:n] += delta[:, :nc].sum(axis=1)
        per = self.timer.rejected_samples
        for c, name in enumerate(self.cfg.channel_names):
            per[name] = per.get(name, 0) + int(delta[:, c].sum())
        g = self.timer.gauges
        total = g.get("rejected_samples_total", 0) + int(delta[:, :nc].sum())
        g["rejected_samples_total"] = total
        if not self._lifecycle:
            # with --evict-idle-s this state counts the samples of patients
            # turned away at a full slot table (_update_gauges)
            g["rejected_total"] = total

    def _update_gauges(self) -> None:
        c = self.consumer
        self.timer.gauges.update(
            active=c.n_streams(), admitted_total=c.n_admitted(),
            evicted_total=c.n_evicted(), rejected_total=c.n_rejected())

    def trigger(self) -> int:
        """Drain bus -> ingest -> fused preprocess+infer -> store."""
        with self.timer:
            import time as _time
            t0 = _time.perf_counter() if self.stage_profile else 0.0
            # native edge: poll + wire parse + key->sid + shard filter in
            # one C++ pass (no per-message Python — VERDICT r1 item #3);
            # with the poll thread running this just swaps buffers
            sa, ca, va, ta, new_keys, *rejected_ts = self._take_polled()
            t0 = self._stamp("poll", t0)
            if self._lifecycle:
                # event time passes even while every arriving patient is
                # turned away (a ward turning over all at once would
                # otherwise never reach the idle cut)
                for r in rejected_ts:
                    self.hwm = max(self.hwm, float(r))
                for k, sid in new_keys:
                    if sid >= len(self.pids):
                        self.pids.extend([None] * (sid + 1 - len(self.pids)))
                    self.pid_index[k] = sid
                    self.pids[sid] = k
                if new_keys:
                    self._admit(new_keys, sa, ta)
            else:
                for k, sid in new_keys:
                    self.pid_index[k] = sid
                    self.pids.append(k)
            if new_keys:
                self._slot_version += 1
            self.flush()  # pipelined: persist trigger T-1 AFTER the poll
                          # overlapped its GPU tail (no-op otherwise)
            if len(ta):
                self.hwm = max(self.hwm, float(ta.max()))
            advance = max(0.0, self.hwm - self.watermark_s)
            nproc_before = self.se.nproc
            if len(sa):
                import numpy as _np
                self.se.ingest_events_chunked(
                    torch.from_numpy(sa.astype(_np.int64)),
                    torch.from_numpy(ca.astype(_np.int64)),
                    torch.from_numpy(ta),
                    torch.from_numpy(va),
                    advance_to=advance)
            else:
                self.se.advance_watermark(advance)
            if self._gated and self.pids:
                self._count_rejected()
            t0 = self._stamp("ingest", t0)
            np_new = self.se.nproc - nproc_before
            if self.emit_processed and np_new > 0 and self.pids:
                import json as _json
                max_emit = self.se.G - self.se.win_buckets - 1
                if np_new > max_emit:  # catch-up: only the retained tail
                    nproc_emit = self.se.nproc - max_emit
                    np_emit = max_emit
                else:
                    nproc_emit, np_emit = nproc_before, np_new
                gidx = torch.tensor([(nproc_emit + j) % self.se.G
                                     for j in range(np_emit)],
                                    dtype=torch.long, device=self.se.device)
                block = self.se.proc.index_select(2, gidx).cpu()
                for pid, sid in self.pid_index.items():
                    rows = block[sid].tolist()
                    for c in range(self.cfg.n_channels):
                        self.producer.produce(self.emit_processed,
                                              f"{pid}_{c}",
                                              _json.dumps(rows[c]),
                                              ts_us=int(self.hwm * 1e6))
            n = self._score(np_new, t0)
            if self._lifecycle:
                # event time, like the watermark: --speed-invariant. The
                # slots are wiped in THIS trigger, before the next poll is
                # consumed.
                self._drop_evicted(self.consumer.evict_idle(min(
                    self.hwm - self.evict_idle_s,
                    self.se.nproc * self.se.bucket_s)))
                self._update_gauges()
            self._n_triggers += 1
            if self.state_path and \
                    self._n_triggers % self.snapshot_every == 0:
                self.save_state(self.state_path)
            return n

    def _score(self, np_new: int, t0: float) -> int:
        """Score the latest window of every slot in use and persist the
        predictions of the live, ready streams; returns their number."""
        if np_new <= 0 or not self.pids:
            return 0
        mask = None
        if self._lifecycle:
            ready = self.se.stream_ready()
            mask = [p is not None and bool(ready[i])
                    for i, p in enumerate(self.pids)]
            if not any(mask):
                return 0
        elif not self.se.ready:
            return 0
        dtype = torch.bfloat16 if self.device != "cpu" else torch.float32
        n_active = len(self.pids)
        # cached device buffers: the age column only changes when the
        # slot table does (version counter), and the gather overwrites every
        # window element — rebuilding these per trigger cost ~13 ms of
        # Python at 16k live patients (serving_latency_big.json)
        age = self._age_column()
        if getattr(self, "_win_buf", None) is None or \
                self._win_buf.dtype != dtype:
            tl = self.device != "cpu"
            shape = (self.se.S, 1, self.se.model_win, self.se.C) if tl \
                else (self.se.S, 1, self.se.C, self.se.model_win)
            self._win_buf = torch.zeros(shape, dtype=dtype,
                                        device=self.se.device)
        w = self.se.windows(batch=1, stride=12, dtype=dtype,
                            timelast=self.device != "cpu",
                            out=self._win_buf)
        probs_all = self.me.forward(w[:n_active].contiguous()
                                    if n_active < self.se.S else w,
                                    age, apply_sigmoid=True)
        probs = probs_all.reshape(-1)[:n_active]
        t_us = int(self.hwm * 1e6)
        if self.world > 1:
            # every rank sees the full per-trigger prediction set
            # (monitoring/router hook) — tiny direct all-gather on xGMI
            pad = torch.zeros(self.max_streams, device=probs.device)
            pad[:n_active] = probs
            self.last_gathered = all_gather_predictions(pad)
        imputed = self._imputed_inputs(n_active) \
            if self.min_coverage > 0.0 else None
        t0 = self._stamp("model", t0)
        rejected = self._rej_since[:n_active].copy() if self._gated else None
        if self.pipelined:
            # defer the device sync: persist at the next trigger start,
            # after the bus poll has overlapped this trigger's GPU work
            self._pending = (probs, t_us, list(self.pids), mask, imputed,
                             rejected)
        else:
            self._persist(probs, t_us, self.pids, mask, imputed, rejected)
        self._stamp("persist", t0)
        n_scored = n_active if mask is None else sum(mask)
        self.timer.add_items(n_scored)
        return n_scored

    def _imputed_inputs(self, n_active: int) -> Optional[torch.Tensor]:
        """Per slot in use, the number of fabricated inputs of its latest
        model window over the channels the config names (ring channels beyond
        them are zero by construction): one coverage launch, left on the
        device. None when the engine refuses (the window's buckets are no
        longer wholly in the ring): that trigger withholds nothing."""
        try:
            cov = self.se.coverage()
        except ValueError as e:
            log.warning("coverage unavailable, nothing withheld: %s", e)
            g = self.timer.gauges
            g["coverage_unavailable"] = g.get("coverage_unavailable", 0) + 1
            return None
        return cov[:n_active, :self.cfg.n_channels, 1].sum(dim=1)

    def _coverage_gate(self, imputed, n: int, mask):
        """(q per slot, mask without the streams whose q < min_coverage);
        counts the withheld ones."""
        q = 1.0 - imputed.cpu().numpy()[:n].astype("float64") / (
            self.se.model_win * self.cfg.n_channels)
        base = [True] * n if mask is None else mask
        held = [bool(b and q[i] < self.min_coverage)
                for i, b in enumerate(base)]
        g = self.timer.gauges
        g["withheld_total"] = g.get("withheld_total", 0) + sum(held)
        if any(base):
            g["coverage_mean"] = float(
                sum(q[i] for i, b in enumerate(base) if b) / sum(base))
        return q, [b and not h for b, h in zip(base, held)]

    def _explain(self, vals, slots) -> Dict[int, str]:
        """Attribute the predictions with risk >= explain_above in one call:
        {position in ``vals``: the response's attribution fragment}, deltas
        over the channels the config names, in its order. ``slots`` are the
        ring slots of ``vals``. Empty when the engine refuses (a restored
        ring's window reaches below the restore floor)."""
        pick = [j for j in range(len(slots))
                if float(vals[j]) >= self.explain_above]
        if not pick:
            return {}
        age = torch.full((self.se.S, 1), 65.0, device=self.se.device)
        age[:self._age_dev.shape[0]] = self._age_dev
        try:
            out = self.se.attribute_latest(
                self.me, [slots[j] for j in pick], age=age,
                baseline=self.explain_baseline, apply_sigmoid=True).cpu()
        except ValueError as e:
            log.warning("attribution unavailable: %s", e)
            return {}
        delta = (out[:, :1] - out[:, 1:1 + self.cfg.n_channels]).tolist()
        g = self.timer.gauges
        g["explained_total"] = g.get("explained_total", 0) + len(pick)
        return {j: ', "attribution": {"baseline": "%s", "delta": [%s]}' % (
                    self.explain_baseline,
                    ", ".join(f"{d:.6f}" for d in delta[r]))
                for r, j in enumerate(pick)}

    def _persist(self, probs, t_us: int, pids, mask=None,
                 imputed=None, rejected=None) -> None:
        q = None
        slots = range(len(pids))
        if imputed is not None:
            q, mask = self._coverage_gate(imputed, len(pids), mask)
            if not any(mask):
                return
        if mask is not None:
            # lifecycle: only live, ready slots are persisted and published
            keep = [i for i, m in enumerate(mask) if m]
            probs = probs.reshape(-1)[:len(pids)][
                torch.tensor(keep, dtype=torch.long, device=probs.device)]
            pids = [pids[i] for i in keep]
            slots = keep
            if q is not None:
                q = q[keep]
        n = len(pids)
        attr = self._explain(probs.reshape(-1)[:n].cpu(), slots) \
            if self.explain_above is not None else {}
        if self.store is not None:
            # the mmap store is multi-process safe: each rank persists
            # its own shard directly (no gather needed for durability)
            local = probs.reshape(-1)[:n].cpu()
            self.store.insert_batch(pids, [t_us] * n, local.tolist())
            self.n_predictions += n
        rej = None
        if rejected is not None:
            # what each published slot's tally held when it was scored; the
            # tally keeps what was rejected since (a pipelined persist runs
            # one trigger later) and restarts from there
            sl = list(slots)
            rej = rejected[sl]
            self._rej_since[sl] = (self._rej_since[sl] - rej).clip(min=0)
        if self.producer and self.response_topic:
            vals = probs.reshape(-1)[:n].cpu()
            for i, pid in enumerate(pids):
                cov = "" if q is None else f', "coverage": {q[i]:.4f}'
                rj = "" if rej is None else f', "rejected": {int(rej[i])}'
                self.producer.produce(
                    self.response_topic, pid,
                    f'{{"t_us": {t_us}, "risk": {float(vals[i]):.6f}{cov}'
                    f'{rj}{attr.get(i, "")}}}')

    def flush(self) -> None:
        """Persist the deferred trigger (pipelined mode; call on shutdown
        or whenever durability must catch up to compute)."""
        if self._pending is not None:
            pending, self._pending = self._pending, None
            self._persist(*pending)

    # ------------------------------------------------------------ warm restart
    def save_state(self, path: Optional[str] = None) -> None:
        """Write everything a successor needs to continue from this trigger
        into ONE file, replaced atomically: the live slots' ring tails
        (StreamEngine.snapshot) and, beside them, the bus positions, the
        slot table, the event-time high-water mark, rank/world and the model
        variant. Offsets, slot ids and ring contents can therefore never
        disagree. A deferred pipelined trigger is persisted first. Ring
        state is exactly-once; predictions made after the last snapshot are
        written again by the successor with the same (pid, t_us, risk)."""
        if self._poll_thread is not None:
            raise RuntimeError("save_state with the poll thread running: "
                               "bus positions run ahead of the rings")
        self.flush()
        entries, high_water = self.consumer.slot_table()
        snap = self.se.snapshot(sorted(sid for _k, sid, _t in entries))
        snap.save(path or self.state_path, extra={
            "positions": self.consumer.positions(),
            "slots": [[k, sid, t] for k, sid, t in entries],
            "high_water": high_water, "hwm": self.hwm,
            "rank": self.rank, "world": self.world,
            "model": type(self.me.model).__name__})

    def load_state(self, path: Optional[str] = None) -> bool:
        """Resume from a save_state file: restore the rings, the slot table
        (engine and consumer), ``hwm`` and the bus positions, so the next
        trigger consumes exactly what the writer had not yet put into the
        snapshot. Call before the first trigger. A file that is corrupt, of
        another rank/world or that does not fit this server is refused: one
        error line, ``restore_failed`` + 1, and a cold start as without a
        file (returns False)."""
        path = path or self.state_path
        try:
            snap, extra = EngineSnapshot.load(path)
            if (extra["rank"], extra["world"]) != (self.rank, self.world):
                raise ValueError(
                    f"written by rank {extra['rank']} of {extra['world']}, "
                    f"this is rank {self.rank} of {self.world}")
            slots = [(str(k), int(sid), float(t))
                     for k, sid, t in extra["slots"]]
            high_water = int(extra["high_water"])
            positions = {str(k): int(v)
                         for k, v in extra["positions"].items()}
            hwm = float(extra["hwm"])
            if high_water > self.max_streams:
                raise ValueError(f"{high_water} slots in the file, "
                                 f"max_streams={self.max_streams}")
            if not self._lifecycle and len(slots) != high_water:
                raise ValueError("the file has free slots (written with "
                                 "--evict-idle-s), this server never "
                                 "reuses a slot")
            if sorted(sid for _k, sid, _t in slots) != snap.sids.tolist() \
                    or len({k for k, _s, _t in slots}) != len(slots) \
                    or any(not 0 <= sid < high_water for _k, sid, _t in slots):
                raise ValueError("slot table and ring snapshot disagree")
            self.se.restore(snap)  # checks everything before it writes
        except (OSError, ValueError, KeyError, TypeError) as e:
            log.error("state file %s refused (%s): cold start", path, e)
            self.timer.gauges["restore_failed"] = \
                self.timer.gauges.get("restore_failed", 0) + 1
            return False
        if extra.get("model") != type(self.me.model).__name__:
            log.warning("state written under model %s, serving %s",
                        extra.get("model"), type(self.me.model).__name__)
        self.consumer.restore_slots(slots, high_water)
        for key, off in positions.items():
            topic, _, part = key.rpartition("/")
            self.consumer.seek(topic, int(part), off)
        self.pids = [None] * high_water
        self.pid_index = {}
        for k, sid, _t in slots:
            self.pids[sid] = k
            self.pid_index[k] = sid
        self.hwm = hwm
        self._slot_version += 1
        log.info("resumed %d streams at grid point %d from %s", len(slots),
                 self.se.nproc, path)
        return True


def state_file(state_dir: str, rank: int, world: int) -> str:
    return os.path.join(state_dir, f"serve-rank{rank}of{world}.snap")


def start_metrics_server(timers, port: int):
    """Serve the Prometheus text exposition on 127.0.0.1:port/metrics in a
    daemon thread (stdlib only; scrape target for production serving)."""
    import threading
    from http.server import BaseHTTPRequestHandler, HTTPServer

    from tskd_amd.metrics import prometheus_text

    class H(BaseHTTPRequestHandler):
        def do_GET(self):
            if self.path != "/metrics":
                self.send_response(404)
                self.end_headers()
                return
            body = prometheus_text(timers).encode()
            self.send_response(200)
            self.send_header("Content-Type", "text/plain; version=0.0.4")
            self.send_header("Content-Length", str(len(body)))
            self.end_headers()
            self.wfile.write(body)

        def log_message(self, *a):  # quiet
            pass

    srv = HTTPServer(("127.0.0.1", port), H)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    return srv


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO,
                        format="%(asctime)s %(name)s %(levelname)s %(message)s")
    cfg = get_global_config()
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--speed", type=float, default=5.0)
    ap.add_argument("--bus-dir", default=None)
    ap.add_argument("--store-path", default="predictions.log")
    ap.add_argument("--model-path", default=cfg.model_path)
    ap.add_argument("--age-table", default=None)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available()
                    else "cpu")
    ap.add_argument("--max-streams", type=int, default=1024)
    ap.add_argument("--starting", default="latest",
                    choices=["latest", "earliest"])
    ap.add_argument("--model-response-topic", default=None)
    ap.add_argument("--emit-processed", default=None, metavar="TOPIC",
                    help="also publish processed grid points to TOPIC "
                         "(e.g. call-stream) for the dashboard")
    ap.add_argument("--max-triggers", type=int, default=0)
    ap.add_argument("--hot-reload", action="store_true",
                    help="reload the checkpoint when the file changes")
    ap.add_argument("--metrics-port", type=int, default=0,
                    help="expose Prometheus /metrics on 127.0.0.1:PORT")
    ap.add_argument("--pipelined", action="store_true",
                    help="overlap the bus poll of trigger T+1 with trigger "
                         "T's GPU work (persistence lags one trigger)")
    ap.add_argument("--evict-idle-s", type=float, default=0.0,
                    help="stream lifecycle: evict a patient silent for more "
                         "than this many seconds of event time and reuse "
                         "its ring slot (0 = off: ids are never given back "
                         "and patient --max-streams+1 is fatal)")
    ap.add_argument("--poll-thread", action="store_true",
                    help="drain+parse the bus continuously on a background "
                         "thread (C++ releases the GIL); the trigger only "
                         "ingests/scores — removes the poll from the "
                         "latency path at saturating rates")
    ap.add_argument("--state-dir", default=None, metavar="DIR",
                    help="warm restart: resume from DIR/serve-rank{r}of{w}"
                         ".snap when it exists (ring tails, slot table and "
                         "bus offsets in one atomically replaced file) and "
                         "keep it up to date; a file that is refused means "
                         "a cold start")
    ap.add_argument("--snapshot-every", type=int, default=1, metavar="N",
                    help="with --state-dir: write the state file every N "
                         "triggers (and once more on SIGTERM)")
    ap.add_argument("--min-coverage", type=float, default=0.0, metavar="F",
                    help="coverage gate: withhold the prediction of a stream "
                         "whose latest model window has less than this "
                         "fraction of inputs resting on samples, the rest "
                         "being carried, back-filled or zero (0 = off)")
    ap.add_argument("--explain-above", type=float, default=None, metavar="R",
                    help="channel attribution: a published prediction with "
                         "risk >= R carries per-channel occlusion deltas "
                         "(score minus the score with that channel held "
                         "flat or zeroed) in the response topic (off "
                         "unless given)")
    ap.add_argument("--explain-baseline", default="hold",
                    choices=["hold", "zero"],
                    help="with --explain-above: what replaces a channel, "
                         "its oldest point in the window (a lead that fell "
                         "off) or 0 (a channel that never arrived)")
    ap.add_argument("--reload-check", type=int, default=0, metavar="K",
                    help="with --hot-reload: before a changed checkpoint "
                         "goes live, score the last K triggers of every "
                         "live ready stream from the ring under both models "
                         "and export how far the scores move (0 = off)")
    ap.add_argument("--reload-max-shift", type=float, default=None,
                    metavar="D",
                    help="with --reload-check: keep the current model when "
                         "the candidate moves any of those scores by more "
                         "than D or gives a non-finite one")
    ap.add_argument("--valid-range", action="append", default=None,
                    metavar="SPEC",
                    help="signal-quality gate (repeatable): NAME=LO:HI keeps "
                         "only samples of channel NAME inside [LO, HI] "
                         "(either side empty = open), 'numerics' selects "
                         "the preset that drops the monitors' no-reading "
                         "code 0; rejected samples count as missing and are "
                         "exported as tskd_rejected_samples_total. "
                         "Overrides the config's VALID_RANGES (off unless "
                         "either is given)")
    args = ap.parse_args(argv)
    try:
        valid_range = resolve_valid_ranges(cfg, args.valid_range)
    except ValueError as e:
        ap.error(str(e))
    if args.reload_check < 0:
        ap.error("--reload-check must not be negative")
    if args.reload_max_shift is not None and args.reload_check < 1:
        ap.error("--reload-max-shift needs --reload-check")
    if not 0.0 <= args.min_coverage <= 1.0:
        ap.error("--min-coverage must lie in [0, 1]")
    if args.explain_above is not None and args.pipelined:
        ap.error("--explain-above cannot be combined with --pipelined: "
                 "choosing the streams needs the scores on the host in the "
                 "trigger that made them, and --pipelined defers them")
    if args.state_dir and args.poll_thread:
        ap.error("--state-dir cannot be combined with --poll-thread: the "
                 "poll thread owns the consumer, so the bus positions run "
                 "ahead of the rings a snapshot would pair them with")
    if args.snapshot_every < 1:
        ap.error("--snapshot-every must be at least 1")

    rank, world = init_distributed()
    from tskd_amd.cli.predictstream import load_model_for_serving
    bus = Bus(args.bus_dir)
    store = PredictionStore(args.store_path)  # multi-process safe: all ranks
    ages = AgeTable()
    if args.age_table and os.path.exists(args.age_table):
        try:
            ages.load_cohort_csv(args.age_table)
        except (ValueError, IndexError):
            ages.load(args.age_table)
    srv = FusedServer(bus, cfg, store, ages,
                      model=load_model_for_serving(args.model_path),
                      device=args.device, max_streams=args.max_streams,
                      starting=args.starting,
                      response_topic=args.model_response_topic,
                      emit_processed=args.emit_processed,
                      rank=rank, world=world, pipelined=args.pipelined,
                      evict_idle_s=args.evict_idle_s,
                      snapshot_every=args.snapshot_every,
                      min_coverage=args.min_coverage,
                      explain_above=args.explain_above,
                      explain_baseline=args.explain_baseline,
                      reload_check=args.reload_check,
                      reload_max_shift=args.reload_max_shift,
                      valid_range=valid_range)
    if args.state_dir:
        os.makedirs(args.state_dir, exist_ok=True)
        srv.state_path = state_file(args.state_dir, rank, world)
        if os.path.exists(srv.state_path):
            srv.load_state()
    if args.poll_thread:
        srv.start_poll_thread()
    if args.hot_reload and args.model_path:
        srv.model_path = args.model_path
        if os.path.exists(args.model_path):
            srv._model_mtime = os.path.getmtime(args.model_path)
    metrics_srv = None
    if args.metrics_port:
        metrics_srv = start_metrics_server([srv.timer],
                                           args.metrics_port + rank)
        log.info("metrics on 127.0.0.1:%d/metrics", args.metrics_port + rank)
    period = cfg.predict_slide_s / args.speed
    stop = []
    signal.signal(signal.SIGTERM, lambda *a: stop.append(1))
    n = 0
    while not stop:
        t0 = time.time()
        srv.maybe_reload_model()
        srv.trigger()
        n += 1
        if n % 10 == 0:
            log.info("metrics %s", srv.timer.log_line())
        if args.max_triggers and n >= args.max_triggers:
            break
        time.sleep(max(0.0, period - (time.time() - t0)))
    srv.stop_poll_thread()
    srv.flush()  # pipelined mode: persist the final deferred trigger
    if srv.state_path:
        srv.save_state()  # SIGTERM / --max-triggers: nothing to replay


if __name__ == "__main__":
    main()

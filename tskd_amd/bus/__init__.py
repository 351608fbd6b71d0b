"""Keyed topic bus — python API over the C++ broker-less bus (_tskd_bus).

Drop-in functional analog of the reference's confluent-kafka usage
(reference sendStream.py:41-72, utils.py:409-428): keyed topics, acks=all,
retries=5, startingOffsets latest/earliest, replay via seek. Topics are
mmap'd partition logs under a shared directory (tmpfs by default), so the
pipeline stages remain separate OS processes like the reference's
docker-compose services — without a broker.
"""

from __future__ import annotations

import json
import time
from typing import List, Optional, Sequence

from tskd_amd import _tskd_bus as _C
from tskd_amd.config import GlobalConfig, get_global_config

Message = _C.Message


def default_bus_dir(cfg: Optional[GlobalConfig] = None) -> str:
    cfg = cfg or get_global_config()
    d = cfg.bus_dir
    if not d.startswith("/"):
        import os
        base = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
        d = f"{base}/{d}"
    return d


class Bus:
    def __init__(self, directory: Optional[str] = None, default_parts: int = 1):
        self._c = _C.Bus(directory or default_bus_dir(), default_parts)

    @property
    def dir(self) -> str:
        return self._c.dir

    def create_topic(self, topic: str, nparts: int = 1) -> None:
        self._c.create_topic(topic, nparts)

    def list_topics(self) -> List[str]:
        return self._c.list_topics()

    def end_offset(self, topic: str, partition: int = 0) -> int:
        return self._c.end_offset(topic, partition)

    def partition_for(self, topic: str, key: str) -> int:
        return self._c.partition_for(topic, key)

    def trim_offset(self, topic: str, partition: int = 0) -> int:
        return self._c.trim_offset(topic, partition)

    def trim_topic(self, topic: str, partition: int = 0,
                   before_offset: int = 0) -> int:
        """Retention: reclaim storage for messages before ``before_offset``
        (hole punch; offsets stay absolute — reads below the trim point are
        a consumer-visible gap, like Kafka retention). Returns the applied
        page-aligned trim offset."""
        return self._c.trim_topic(topic, partition, before_offset)


class Producer:
    """acks=all, retries=5 producer (reference utils.py:417-422)."""

    def __init__(self, bus: Bus, retries: int = 5):
        self._c = _C.Producer(bus._c, retries)

    def produce(self, topic: str, key: bytes | str, value: bytes | str,
                partition: int = -1, ts_us: int = -1,
                callback=None) -> None:
        k = key.decode() if isinstance(key, bytes) else key
        v = value.decode() if isinstance(value, bytes) else value
        try:
            self._c.produce(topic, k, v, partition, ts_us)
        except Exception as e:
            if callback:
                callback(e, None)  # reference `acked` error path (utils.py:409)
                return
            raise
        if callback:
            callback(None, (topic, k))

    def produce_sample(self, topic: str, patient_id: str, channel_index: int,
                       value: float, ts_us: int = -1) -> None:
        """The reference wire format: key=patientid,
        value=JSON [channel_index, float] (sendStream.py:59-64)."""
        self.produce(topic, patient_id,
                     json.dumps([channel_index, value]), ts_us=ts_us)

    def flush(self, topic: str = "") -> None:
        self._c.flush(topic)

    @property
    def produced(self) -> int:
        return self._c.produced


class Consumer:
    """startingOffsets latest|earliest; poll; seek for replay-from-offset."""

    def __init__(self, bus: Bus, starting: str = "latest"):
        assert starting in ("latest", "earliest")
        self._c = _C.Consumer(bus._c, starting)

    def subscribe(self, topics: Sequence[str]) -> None:
        self._c.subscribe(list(topics))

    def poll(self, max_msgs: int = 256, timeout_ms: int = 0) -> List[Message]:
        return self._c.poll(max_msgs, timeout_ms)

    def poll_samples(self, max_msgs: int = 4096, timeout_ms: int = 0):
        """Poll + parse the reference "[chan, value]" wire format natively
        (C++): returns (keys, topics, chan int32[], value float32[],
        ts float64[] seconds). Unparseable messages are skipped (their
        offsets still advance)."""
        return self._c.poll_samples(max_msgs, timeout_ms)

    def poll_samples_sid(self, max_msgs: int = 4096, timeout_ms: int = 0,
                         rank: int = 0, world: int = 1,
                         max_streams: int = 0,
                         drop_when_full: bool = False):
        """The fully-native serving ingest edge: poll + wire parse + key->
        dense-stream-id mapping + DP shard filter (FNV-1a % world == rank,
        same hash as parallel.shard_for_key) in one C++ pass. Returns
        (sid int32[], chan int32[], value float32[], ts float64[] seconds,
        new_keys [(key, sid), ...] in admission order).

        A new key takes the lowest sid freed by ``evict_idle``/``release``
        before the table grows. With the table full and nothing free an
        unknown key raises ``max_streams exceeded``; ``drop_when_full=True``
        skips its samples instead and counts them in ``n_rejected()``; the
        tuple then has a sixth element, the newest event time (seconds)
        among the samples rejected in this batch (0.0 if none), so that
        event time passes for the caller even while every arriving patient
        is turned away."""
        return self._c.poll_samples_sid(max_msgs, timeout_ms, rank, world,
                                        max_streams, drop_when_full)

    def evict_idle(self, before_ts: float):
        """Remove every key whose last-seen event time (seconds, updated at
        poll time) is ``< before_ts`` and free its sid for reuse. Returns
        the removed [(key, sid), ...]."""
        return self._c.evict_idle(float(before_ts))

    def release(self, key: bytes | str) -> int:
        """Explicit discharge of one key: the freed sid, or -1 if the key
        is not live."""
        return self._c.release(key.decode() if isinstance(key, bytes)
                               else key)

    def slot_table(self):
        """The key -> sid table as it stands: ([(key, sid, last_seen), ...],
        high_water). With ``positions()`` it is what a successor needs to
        take over this consumer's patients under the same ids."""
        entries, high_water = self._c.slot_table()
        return list(entries), high_water

    def restore_slots(self, entries, high_water: int) -> None:
        """Rebuild the slot table from a ``slot_table()`` of an earlier
        consumer: every sid below ``high_water`` that no entry uses is free,
        so new keys take the same lowest-free sids as the original. Legal
        only before the first poll (RuntimeError after it); a duplicate key
        or sid, or a sid outside [0, high_water), raises ValueError."""
        self._c.restore_slots(
            [(k.decode() if isinstance(k, bytes) else str(k), int(s),
              float(t)) for k, s, t in entries], int(high_water))

    def n_streams(self) -> int:
        """Number of live keys."""
        return self._c.n_streams()

    def sid_high_water(self) -> int:
        """Slots ever handed out (1 + the highest sid assigned)."""
        return self._c.sid_high_water()

    def n_rejected(self) -> int:
        """Samples skipped because the table was full (drop_when_full)."""
        return self._c.n_rejected()

    def n_admitted(self) -> int:
        return self._c.n_admitted()

    def n_evicted(self) -> int:
        return self._c.n_evicted()

    def seek(self, topic: str, partition: int, offset: int) -> None:
        self._c.seek(topic, partition, offset)

    def positions(self):
        return self._c.positions()


def wait_for_topic(bus: Bus, topic: str, timeout_s: float = 10.0) -> bool:
    t0 = time.time()
    while time.time() - t0 < timeout_s:
        if topic in bus.list_topics():
            return True
        time.sleep(0.05)
    return False

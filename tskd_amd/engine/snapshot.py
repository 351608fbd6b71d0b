"""EngineSnapshot — the live tail of a StreamEngine's rings, and its file.

A snapshot holds, per listed stream and channel, the buckets the window fill
has not consumed yet, the last ``keep`` processed points and the fill carry,
in linear grid order (see ``StreamEngine.snapshot``), plus the ring indices
and the geometry they were taken under. It restores into a fresh engine of
the same geometry whose ring length, stream count or bucket packing may
differ.

File layout (little-endian)::

    magic "TSKDSNAP" | version u32 | header length u32 | JSON header
    | sids int64[n] | born int64[n] | payload fp32[n, C, R] | crc32 u32

The CRC covers every byte before it. ``save`` writes a temporary file next
to the target, fsyncs it and renames it over the target, so a reader finds
either the old snapshot or the new one, never a mixture.
"""

from __future__ import annotations

import json
import os
import struct
import zlib
from dataclasses import dataclass, field
from typing import Tuple

import numpy as np

MAGIC = b"TSKDSNAP"
VERSION = 1
GEOMETRY = ("C", "fs", "bucket_s", "win_buckets", "model_win")
INDICES = ("head", "nproc", "cleared", "origin_nproc", "forced_ready", "nbk",
           "keep")
_PRE = struct.Struct("<8sII")


class SnapshotError(ValueError):
    """A snapshot file that cannot be trusted: truncated, corrupt, or of
    another format or version."""


@dataclass
class EngineSnapshot:
    geometry: dict            # C, fs, bucket_s, win_buckets, model_win
    head: int
    nproc: int
    cleared: int
    origin_nproc: int
    forced_ready: bool
    nbk: int                  # buckets [nproc, nproc + nbk) per channel
    keep: int                 # processed points [nproc - keep, nproc)
    sids: np.ndarray          # int64 (n,)
    born: np.ndarray          # int64 (n,) = engine.born[sids]
    payload: np.ndarray = field(repr=False)  # fp32 (n, C, 2*nbk + keep + 1)

    @property
    def record_len(self) -> int:
        return 2 * self.nbk + self.keep + 1

    def _header(self, extra: dict) -> dict:
        h = {k: getattr(self, k) for k in INDICES}
        h["forced_ready"] = bool(h["forced_ready"])
        h.update(geometry=self.geometry, n=int(self.sids.size),
                 extra=extra or {})
        return h

    def save(self, path: str, extra: dict = None) -> None:
        """Write the snapshot and the JSON-serialisable ``extra`` to
        ``path`` atomically (temporary file, fsync, rename)."""
        n, c = int(self.sids.size), int(self.geometry["C"])
        payload = np.ascontiguousarray(self.payload, dtype="<f4")
        assert payload.shape == (n, c, self.record_len), payload.shape
        hdr = json.dumps(self._header(extra), sort_keys=True).encode()
        parts = [_PRE.pack(MAGIC, VERSION, len(hdr)), hdr,
                 np.ascontiguousarray(self.sids, dtype="<i8").data,
                 np.ascontiguousarray(self.born, dtype="<i8").data,
                 payload.reshape(-1).data]
        tmp = f"{path}.tmp"
        crc = 0
        with open(tmp, "wb") as fh:
            for p in parts:
                crc = zlib.crc32(p, crc)
                fh.write(p)
            fh.write(struct.pack("<I", crc))
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, path)
        dfd = os.open(os.path.dirname(os.path.abspath(path)), os.O_RDONLY)
        try:
            os.fsync(dfd)  # the rename itself
        finally:
            os.close(dfd)

    @staticmethod
    def load(path: str) -> Tuple["EngineSnapshot", dict]:
        """(snapshot, extra) from ``path``; SnapshotError unless the file is
        complete and intact."""
        with open(path, "rb") as fh:
            buf = fh.read()
        if len(buf) < _PRE.size:
            raise SnapshotError(f"{path}: truncated before the header")
        magic, version, hlen = _PRE.unpack_from(buf)
        if magic != MAGIC:
            raise SnapshotError(f"{path}: not an engine snapshot")
        if version != VERSION:
            raise SnapshotError(f"{path}: version {version}, not {VERSION}")
        off = _PRE.size
        if len(buf) < off + hlen + 4:
            raise SnapshotError(f"{path}: truncated header")
        try:
            h = json.loads(buf[off:off + hlen])
            n, c = int(h["n"]), int(h["geometry"]["C"])
            rlen = 2 * int(h["nbk"]) + int(h["keep"]) + 1
            if min(n, c, int(h["nbk"]), int(h["keep"])) < 0:
                raise ValueError("negative size")
        except (ValueError, KeyError, TypeError) as e:
            raise SnapshotError(f"{path}: unreadable header ({e})") from e
        off += hlen
        body = 16 * n + 4 * n * c * rlen
        if len(buf) != off + body + 4:
            raise SnapshotError(
                f"{path}: {len(buf)} bytes, expected {off + body + 4}")
        (crc,) = struct.unpack_from("<I", buf, off + body)
        if zlib.crc32(memoryview(buf)[:off + body]) != crc:
            raise SnapshotError(f"{path}: checksum mismatch")
        sids = np.frombuffer(buf, "<i8", n, off).astype(np.int64)
        born = np.frombuffer(buf, "<i8", n, off + 8 * n).astype(np.int64)
        payload = np.frombuffer(buf, "<f4", n * c * rlen, off + 16 * n) \
            .astype(np.float32).reshape(n, c, rlen)
        snap = EngineSnapshot(
            geometry=h["geometry"], sids=sids, born=born, payload=payload,
            **{k: h[k] for k in INDICES})
        return snap, h["extra"]

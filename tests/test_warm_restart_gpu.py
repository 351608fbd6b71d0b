"""Warm restart on the GPU: the snapshot_streams / restore_streams kernels
(packed and split bucket layout on either side, wrapping ranges, a record
length that is no multiple of 4), restored-engine equivalence on device
rings for the event and the dense path, and FusedServer resuming on cuda.
"""
import contextlib
import os

import pytest
import torch

from tskd_amd.engine import StreamEngine

from test_stream_lifecycle_gpu import _filled_engine
from test_warm_restart import (C, G, POINTS, S, _filled_cpu,
                               check_cold_starts, check_daemon,
                               check_isolation, check_refusals, check_resumed,
                               reference_run, run_daemon)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def packing(packed):
    """Engines built inside use the packed or the split bucket layout."""
    old = os.environ.get("TSKD_PACKED_BUCKETS")
    os.environ["TSKD_PACKED_BUCKETS"] = "1" if packed else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["TSKD_PACKED_BUCKETS"]
        else:
            os.environ["TSKD_PACKED_BUCKETS"] = old


@pytest.fixture(scope="module", params=[True, False],
                ids=["from-packed", "from-unpacked"])
def ref_gpu(request):
    with packing(request.param):
        return request.param, reference_run("cuda")


class TestEngineEquivalenceGpu:
    @pytest.mark.parametrize("k", POINTS)
    def test_restored_into_the_other_layout(self, ref_gpu, k):
        """Integer samples: bucket sums are exact in fp32 whatever order the
        atomics land in, so the restored engine must match bit for bit."""
        src_packed, ref = ref_gpu
        with packing(not src_packed):
            eng = check_resumed(ref, k, "cuda")
        assert eng._packed == (not src_packed)

    def test_restored_into_a_longer_ring(self, ref_gpu):
        src_packed, ref = ref_gpu
        with packing(src_packed):
            eng = check_resumed(ref, 23, "cuda", ring_grid=256)
        assert eng._packed == src_packed and eng.G == 256


class TestSnapshotKernels:
    @pytest.mark.parametrize("dst_packed", [True, False],
                             ids=["to-packed", "to-unpacked"])
    @pytest.mark.parametrize("src_packed", [True, False],
                             ids=["from-packed", "from-unpacked"])
    def test_listed_slots_only_and_refusals(self, src_packed, dst_packed,
                                            monkeypatch):
        src = _filled_engine(S, C, G, src_packed, monkeypatch)
        monkeypatch.setenv("TSKD_PACKED_BUCKETS", "1" if dst_packed else "0")

        def fresh():
            e = StreamEngine(S, C, ring_grid=G, device="cuda")
            assert e._packed == dst_packed
            return e

        snap = check_isolation(src, fresh)
        if src_packed == dst_packed:
            check_refusals(snap, fresh)

    @pytest.mark.parametrize("src,dst", [("cpu", "cuda"), ("cuda", "cpu")])
    def test_records_cross_between_cpu_and_cuda(self, src, dst, monkeypatch):
        """A snapshot taken by one implementation (numpy gather or kernel)
        restored by the other: check_isolation compares both payloads with
        the same numpy gather of the source's views, bit for bit."""
        filled = _filled_cpu() if src == "cpu" \
            else _filled_engine(S, C, G, True, monkeypatch)
        check_isolation(filled,
                        lambda: StreamEngine(S, C, ring_grid=G, device=dst))

    def test_snapshot_reuses_its_buffers(self, monkeypatch):
        e = _filled_engine(S, C, G, True, monkeypatch)
        e.head, e.nproc, e._cleared = 276, 241, 276
        first = e.snapshot()
        dev, host = e._snap_dev, e._snap_host
        assert host.is_pinned() and dev.is_cuda
        kept = first.payload.copy()
        again = e.snapshot([1, 2])
        assert e._snap_dev is dev and e._snap_host is host
        assert (again.payload == kept[1:3]).all()


class TestDensePath:
    def test_restored_engine_fills_the_same_windows(self):
        """The same kernels on the same inputs: exact equality."""
        s, c, chunk = 4, 2, 7500                   # 60 s at 125 Hz
        g = torch.Generator().manual_seed(11)
        chunks = [torch.randn(s, c, chunk, generator=g).cuda()
                  for _ in range(20)]
        a = StreamEngine(s, c, ring_grid=G, device="cuda")
        b = StreamEngine(s, c, ring_grid=G, device="cuda")
        for raw in chunks[:15]:
            a.ingest_dense(raw)
            b.ingest_dense(raw)
        snap = b.snapshot()
        assert (snap.head, snap.nproc, snap.nbk, snap.keep) == \
            (180, 145, 35, 120)
        r = StreamEngine(s, c, ring_grid=G, device="cuda")
        r.restore(snap)
        for raw in chunks[15:]:
            a.ingest_dense(raw)
            r.ingest_dense(raw)
            assert a.nproc == r.nproc and a.head == r.head
            assert torch.equal(a.windows(batch=1, stride=12),
                               r.windows(batch=1, stride=12)), a.nproc
        assert a.nproc == 205 and a.windows().any()
        assert torch.equal(a.last_val, r.last_val)


@pytest.fixture(scope="module")
def daemon_gpu(tmp_path_factory):
    out = run_daemon(tmp_path_factory.mktemp("warm_gpu"), "cuda")
    torch.cuda.synchronize()
    return out


class TestDaemonWarmRestartGpu:
    def test_resumed_run_writes_the_uninterrupted_rows(self, daemon_gpu):
        check_daemon(daemon_gpu)

    def test_refused_files_mean_a_cold_start(self, daemon_gpu, tmp_path):
        check_cold_starts(tmp_path, daemon_gpu["state"], "cuda")

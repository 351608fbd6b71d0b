"""Window coverage on the GPU: the window_coverage kernel against the CPU
engine on identical ring contents (exact, torch.equal), over a ring the span
wraps in, both bucket layouts, the three window lengths the mask extraction
distinguishes, the id-list cases, a restored engine's floor, the event path,
and the serving gate on cuda against the cpu run.
"""
import functools

import numpy as np
import pytest
import torch

from tskd_amd.engine import StreamEngine

from test_coverage import (G, L, N_PATTERNS, N_TRIGGERS, check_gate,
                           hand_engine, restored_engine, ring_counts,
                           run_events, run_gate)

pytestmark = pytest.mark.gpu

# lo = nproc - 120 in a ring of 192: 157 ends the span (W=36) on the ring's
# last slot, 158 wraps it by one, 311 starts it on the last slot, 312 on
# slot 0 again
NPROCS = (120, 157, 158, 192, 200, 311, 312, 372)


@functools.lru_cache(maxsize=None)
def cpu_reference(S, C, nproc, W):
    """The CPU engine's result on the hand-written counts, computed once."""
    e, _counts = hand_engine("cpu", S, C, nproc, W)
    return e.coverage()


def set_packing(monkeypatch, packed):
    monkeypatch.setenv("TSKD_PACKED_BUCKETS", "1" if packed else "0")


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("W", [36, 1, 64])
@pytest.mark.parametrize("C", [10, 3])
@pytest.mark.parametrize("S", [1, 3, 9])
def test_kernel_equals_cpu_engine(S, C, W, packed, monkeypatch):
    set_packing(monkeypatch, packed)
    for nproc in NPROCS:
        e, counts = hand_engine("cuda", S, C, nproc, W)
        assert e._packed == packed
        got = e.coverage()
        assert got.is_cuda and got.dtype == torch.int32
        assert torch.equal(got.cpu(), cpu_reference(S, C, nproc, W)), nproc
        assert np.array_equal(e.bcnt.cpu().numpy(), counts)   # reads only


def test_every_pattern_is_covered():
    assert 9 * 3 >= N_PATTERNS


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_sid_lists(packed, monkeypatch):
    set_packing(monkeypatch, packed)
    e, _ = hand_engine("cuda", 9, 3, 200, 36)
    want = cpu_reference(9, 3, 200, 36)
    assert torch.equal(e.coverage().cpu(), want)
    assert torch.equal(e.coverage([2, 0, 2]).cpu(), want[[2, 0, 2]])
    assert torch.equal(e.coverage(torch.tensor([8])).cpu(), want[[8]])
    empty = e.coverage([])
    assert empty.shape == (0, 3, 3) and empty.is_cuda
    for bad in ([9], [-1], [0, 9]):
        with pytest.raises(ValueError):
            e.coverage(bad)


def test_refusals():
    e = StreamEngine(2, 3, ring_grid=G, device="cuda")
    with pytest.raises(ValueError, match="no full model window"):
        e.coverage()
    e, _ = hand_engine("cuda", 2, 3, 200, 36)
    e._cleared = 80 + G + 1
    with pytest.raises(ValueError, match="no longer wholly in the ring"):
        e.coverage()
    # a span above the kernel's 192-bit mask is refused before any launch
    e = StreamEngine(2, 3, ring_grid=256, win_buckets=64, model_win=130,
                     device="cuda")
    e.nproc, e.head = 130, 193
    e._cleared = e.head
    with pytest.raises(RuntimeError, match="code -4"):
        e.coverage()


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("nproc", [133, 170, 252, 253])
def test_floor_inside_the_span(nproc, packed, monkeypatch):
    set_packing(monkeypatch, packed)
    S = -(-N_PATTERNS // 3)
    pair = []
    for device in ("cpu", "cuda"):
        e, _snap = restored_engine(device, S, 3)
        assert e._bucket_floor == 133
        if nproc > 133:       # else: the rings as the restore left them
            e.bcnt.copy_(torch.from_numpy(ring_counts(S, 3, G, nproc, 36)))
            e.nproc = nproc
            e.head = e._cleared = nproc + 35
        pair.append(e.coverage().cpu())
    assert torch.equal(pair[0], pair[1])
    if nproc == 133:
        assert not pair[1][:, :, 1].any()


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_event_path_equal_on_both_devices(packed, monkeypatch):
    set_packing(monkeypatch, packed)
    gpu, cpu = run_events("cuda"), run_events("cpu")
    assert gpu._packed == packed
    assert (gpu.head, gpu.nproc) == (cpu.head, cpu.nproc) == (240, 205)
    got = gpu.coverage()
    assert torch.equal(got.cpu(), cpu.coverage())
    assert got[1, 2].tolist() == [0, L, 155]


class TestServingGateGpu:
    def test_withheld_set_equals_the_cpu_run(self, tmp_path):
        srv, log = run_gate(tmp_path, "gpu", device="cuda", min_coverage=0.5)
        torch.cuda.synchronize()
        assert srv.se.S == 4 and srv.se.G == 256
        assert check_gate(srv, log, 0.5) == N_TRIGGERS - 24
        csrv, clog = run_gate(tmp_path, "cpu", device="cpu", min_coverage=0.5)
        for (m, nproc, rows, msgs), (_m, cnproc, crows, cmsgs) in zip(log,
                                                                      clog):
            assert nproc == cnproc
            assert sorted(p for p, _t, _r in rows) == \
                sorted(p for p, _t, _r in crows), m
            assert sorted(k for k, _v in msgs) == \
                sorted(k for k, _v in cmsgs), m
        assert srv.timer.gauges["withheld_total"] == \
            csrv.timer.gauges["withheld_total"]
        assert srv.timer.gauges["coverage_mean"] == \
            csrv.timer.gauges["coverage_mean"]

    def test_default_is_byte_identical_to_no_argument(self, tmp_path):
        _a, plain = run_gate(tmp_path, "plain", device="cuda")
        b, off = run_gate(tmp_path, "off", device="cuda", min_coverage=0.0)
        torch.cuda.synchronize()
        assert plain == off
        assert any(len(rows) == 2 for _m, _n, rows, _msgs in plain[-3:])
        assert "withheld_total" not in b.timer.gauges

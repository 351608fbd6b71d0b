"""Risk history on the GPU: ``serve_tail_history_kernel`` against the
reference path (``StreamEngine.score_history_reference`` on bf16 time-last
windows: ``windows(batch=k - jmin)`` -> every window its own one-step
sequence -> ``MyCNNEngine.forward``), kernel vs unfused chain in the same
process on the same ring.

The construction is tests/test_attribution_gpu.py's: G = 192, S = 9, C = 10,
a seeded ``randn * 2`` ring, ``nproc`` set by hand, no ingest. Hard gate: rtol
= atol = 2e-3, that file's and tests/test_fused_tail.py's tolerance between
fused and unfused results; the expected difference is zero (same bf16 images,
same operation order for every kept term), and each test prints the maximum
it saw. NaN positions are compared with ``isnan`` and must be equal; values
are compared at the gate elsewhere.
"""

import pytest
import torch

from tskd_amd.engine import StreamEngine

from test_history import K_STRIDES, jmin_of

G = 192
S = 9
L = 120
# 120: first full window; 191: ends one short of the ring end; 192: exactly
# at it; 200: straddles the wrap; 372: a steady-state position after a wrap
NPROCS = (120, 191, 192, 200, 372)
# a single wave's stream; the last stream; a duplicate, out of order; an odd
# count; all nine
SID_LISTS = ([0], [8], [2, 0, 2], [5, 1, 7], list(range(S)))
RTOL = ATOL = 2e-3
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def engines():
    from tskd_amd.models import build_model
    from tskd_amd.ops import MyCNNEngine
    out = {}
    for i, name in enumerate(("MyCNN5", "MyCNN4", "MyCNN2")):
        torch.manual_seed(500 + i)
        out[name] = MyCNNEngine(build_model(name).eval(), device="cuda")
    return out


def _ring(n_streams, C, seed, ring=G):
    se = StreamEngine(n_streams, C, ring_grid=ring, fs=25.0, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    se.proc.copy_(torch.randn(n_streams, C, ring, device="cuda",
                              generator=gen) * 2.0)
    return se


def _age():
    return (40.0 + 7.0 * torch.arange(S, device="cuda",
                                      dtype=torch.float32)).reshape(S, 1)


def _close(got, want, jm, what):
    """NaN prefix of exactly jm columns on both sides, the rest at the gate;
    returns the largest difference."""
    nan = torch.isnan(got)
    assert torch.equal(nan, torch.isnan(want)), what
    assert nan[:, :jm].all() and not nan[:, jm:].any(), what
    torch.testing.assert_close(got[:, jm:], want[:, jm:], rtol=RTOL,
                               atol=ATOL, msg=lambda m: f"{what}: {m}")
    return (got[:, jm:] - want[:, jm:]).abs().max().item()


@pytest.mark.gpu
class TestHistoryKernel:
    @pytest.mark.parametrize("variant", ["MyCNN5", "MyCNN4"])
    def test_matches_reference_path(self, engines, variant):
        me = engines[variant]
        assert me.supports_history(10)
        se = _ring(S, 10, seed=7 * len(variant))
        worst = 0.0
        for nproc in NPROCS:
            se.nproc = nproc
            for k, stride in K_STRIDES:
                jm = jmin_of(nproc, G, k, stride)
                assert 0 <= jm < k
                for age in (None, _age()):
                    for sig in (False, True):
                        # the reference scores streams independently:
                        # computed once for all nine, a list's rows are its
                        ref = se.score_history_reference(
                            me, None, k, stride, age, sig, dtype=BF16)
                        assert ref.shape == (S, k)
                        for sids in SID_LISTS:
                            got = se.score_history(me, sids, k, stride, age,
                                                   sig)
                            torch.cuda.synchronize()
                            assert got.shape == (len(sids), k)
                            assert got.dtype == torch.float32
                            want = ref[torch.tensor(sids, device="cuda")]
                            worst = max(worst, _close(
                                got, want, jm,
                                f"nproc={nproc} k={k} stride={stride} sids="
                                f"{sids} age={age is not None} sig={sig}"))
        # not vacuous: every column of a stream differs from its neighbour
        se.nproc = 372
        got = se.score_history(me, None, 7, 12, None, False)
        assert not torch.isnan(got).any()
        assert (got[:, 1:] != got[:, :-1]).all()
        print(f"[history] {variant}: max |kernel - reference| = {worst:.3e}")

    def test_nan_prefix_is_exact(self, engines):
        me = engines["MyCNN5"]
        se = _ring(S, 10, seed=13)
        for nproc, k, stride, want in ((120, 5, 12, 4), (120, 1, 12, 0),
                                       (372, 8, 12, 1), (372, 7, 12, 0)):
            assert jmin_of(nproc, G, k, stride) == want
        for nproc in NPROCS:
            se.nproc = nproc
            for k, stride in K_STRIDES:
                got = se.score_history(me, [5, 1, 7], k, stride)
                nan = torch.isnan(got)
                jm = jmin_of(nproc, G, k, stride)
                assert nan[:, :jm].all() and not nan[:, jm:].any(), \
                    (nproc, k, stride)
                assert int(nan.sum()) == 3 * jm

    @pytest.mark.parametrize("variant", ["MyCNN5", "MyCNN4"])
    def test_newest_column_is_score_latest(self, engines, variant):
        me = engines[variant]
        se = _ring(S, 10, seed=61)
        worst = 0.0
        for nproc in NPROCS:
            se.nproc = nproc
            for age in (None, _age()):
                for sig in (False, True):
                    score = se.score_latest(me, age, apply_sigmoid=sig)
                    for k, stride in ((1, 12), (2, 12), (5, 12), (8, 12),
                                      (4, 13)):
                        for sids in SID_LISTS:
                            got = se.score_history(me, sids, k, stride, age,
                                                   sig)
                            torch.cuda.synchronize()
                            want = score[torch.tensor(sids, device="cuda")]
                            worst = max(worst, (got[:, -1:] - want).abs()
                                        .max().item())
                            torch.testing.assert_close(
                                got[:, -1:], want, rtol=RTOL, atol=ATOL)
        print(f"[history] {variant}: max |newest column - score_latest| = "
              f"{worst:.3e}")

    @pytest.mark.parametrize("nproc", [192, 200])
    @pytest.mark.parametrize("variant", ["MyCNN5", "MyCNN4"])
    def test_structure_is_exact(self, engines, variant, nproc):
        """A ring periodic in the slot index with period 12 (G is a multiple
        of 12) shows the same image to every window at stride 12, whichever
        round, image slot or wave scores it: the available columns of a row
        are bit-equal. A wrong start slot or unwrap shows as a difference,
        as stride 13 does."""
        me = engines[variant]
        se = _ring(S, 10, seed=71)
        se.proc.copy_(se.proc[:, :, :12].repeat(1, 1, G // 12))
        se.nproc = nproc
        for k in (7, 8):
            got = se.score_history(me, None, k, 12, None, False)
            jm = jmin_of(nproc, G, k, 12)
            assert jm == k - 7
            assert torch.isnan(got[:, :jm]).all()
            assert torch.equal(got[:, jm:],
                               got[:, -1:].expand(-1, k - jm))
        assert not torch.equal(got[0, jm:], got[1, jm:])   # streams differ
        got = se.score_history(me, None, 4, 13, None, False)
        assert not torch.isnan(got).any()
        assert not torch.equal(got, got[:, -1:].expand(-1, 4))

    @pytest.mark.parametrize("k,stride", [(5, 12), (5, 40)])
    def test_reads_stay_inside_the_windows(self, engines, k, stride):
        """NaN in every ring slot outside [e_jmin - 120, nproc) of the listed
        streams, and in all slots of the others, changes nothing. (5, 40) has
        three unavailable columns, one of them in a round with a live one."""
        me = engines["MyCNN5"]
        se = _ring(S, 10, seed=83)
        se.nproc = nproc = 200
        sids = [5, 1, 7]
        jm = jmin_of(nproc, G, k, stride)
        assert jm == {12: 0, 40: 3}[stride]
        clean = se.score_history(me, sids, k, stride, _age(), False)
        first = nproc - (k - 1 - jm) * stride - L
        assert first >= nproc - G
        inside = torch.zeros(G, dtype=torch.bool, device="cuda")
        inside[torch.arange(first, nproc, device="cuda") % G] = True
        assert 0 < int((~inside).sum()) < G
        keep = torch.zeros(S, dtype=torch.bool, device="cuda")
        keep[sids] = True
        se.proc[~keep] = float("nan")
        se.proc[:, :, ~inside] = float("nan")
        got = se.score_history(me, sids, k, stride, _age(), False)
        assert not torch.isnan(got[:, jm:]).any()
        assert torch.equal(torch.isnan(got), torch.isnan(clean))
        assert torch.equal(got[:, jm:], clean[:, jm:])

    @pytest.mark.parametrize("ring", [256, 192])
    def test_history_is_what_serving_produced(self, engines, ring):
        """Dense random data, one trigger (12 grid points) at a time: the
        scores ``score_latest`` gave at the last five triggers are the
        history at the end. With ring = 192 those triggers cross the wrap."""
        me = engines["MyCNN5"]
        se = StreamEngine(3, 10, ring_grid=ring, fs=25.0, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(77)
        age = torch.tensor([[30.0], [55.0], [80.0]], device="cuda")
        kept = []
        for _m in range(19):
            se.ingest_dense(torch.randn(3, 10, 12 * se.bucket_len,
                                        device="cuda", generator=gen))
            if se.nproc >= L:
                kept.append(se.score_latest(me, age).clone())
        assert se.nproc == 12 * 19 - 35 and len(kept) >= 6
        assert (se.nproc > ring) == (ring == 192)
        want = torch.cat(kept[-5:], dim=1)
        got = se.score_history(me, None, k=5, stride=12, age=age)
        torch.cuda.synchronize()
        assert not torch.isnan(got).any()
        print(f"[history] ring={ring}: max |history - served| = "
              f"{(got - want).abs().max().item():.3e}")
        torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)
        assert (got[:, 1:] != got[:, :-1]).all()

    def test_restored_engine(self, engines):
        me = engines["MyCNN5"]
        src = _ring(S, 10, seed=87)
        src.nproc = 200
        src.head = src._cleared = 200 + src.win_buckets - 1
        dst = StreamEngine(S, 10, ring_grid=G, fs=25.0, device="cuda")
        dst.restore(src.snapshot(keep=150))
        assert dst.nproc == 200 and dst._proc_floor == 50
        full = src.score_history(me, None, 5, 12, _age())
        got = dst.score_history(me, None, 5, 12, _age())
        assert not torch.isnan(full).any()
        # e_j - 120 = 32, 44, 56, 68, 80 against a floor of 50
        jm = jmin_of(200, G, 5, 12, floor=50)
        assert jm == 2
        worst = _close(got, torch.cat(
            [torch.full_like(full[:, :jm], float("nan")), full[:, jm:]],
            dim=1), jm, "restored")
        one = dst.score_history(me, None, 1, 12, _age())
        torch.testing.assert_close(one, dst.score_latest(me, _age()),
                                   rtol=RTOL, atol=ATOL)
        print(f"[history] restored vs source: max diff = {worst:.3e}")
        # a newest window below the floor is refused like attribute_latest's
        dst._proc_floor = 100
        with pytest.raises(ValueError, match="restored"):
            dst.score_history(me, [0])

    def test_launcher_and_host_edge_cases(self, engines):
        from tskd_amd.ops import hip
        me = engines["MyCNN5"]
        se = _ring(S, 10, seed=81)
        se.nproc = 200
        with pytest.raises(ValueError, match="k=0"):
            se.score_history(me, [0], k=0)
        with pytest.raises(ValueError, match="stride=0"):
            se.score_history(me, [0], stride=0)
        for bad in ([-1], [S]):
            with pytest.raises(ValueError, match="out of range"):
                se.score_history(me, bad)
        se.nproc = 119
        with pytest.raises(ValueError, match="no full model window"):
            se.score_history(me, [0])
        se.nproc = 200
        out = se.score_history(me, [], k=5)
        assert out.shape == (0, 5) and out.device.type == "cuda"
        assert out.dtype == torch.float32
        # the raw binding refuses, launching nothing: jmin = k, and a jmin one
        # too small for the ring (k = 8 at nproc = 200: column 0 would start
        # at grid point -4, the true jmin is 1)
        ids = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
        lib = hip.load(hip.MYCNN)
        assert jmin_of(200, G, 8, 12) == 1

        def raw(k, stride, jmin, proc=se.proc, c=10, eng=me):
            out = torch.full((2, k), -7.0, device="cuda")
            rc = lib.tskd_serve_tail_history_fwd(
                hip.ptr(proc), S, c, G, 200, hip.ptr(ids), 2, hip.ptr(None),
                k, stride, jmin, hip.ptr(out), hip.ptr(eng.wpack),
                hip.ptr(eng.bfrag), eng.age_eps, 0, eng.variant,
                hip.stream_ptr())
            torch.cuda.synchronize()
            return rc, out
        for k, stride, jmin in ((8, 12, 8), (8, 12, 0), (8, 12, -1),
                                (0, 12, 0), (8, 0, 1), (2, 2 ** 30, 1)):
            rc, out = raw(k, stride, jmin)
            assert rc == -5, (k, stride, jmin)
            assert (out == -7.0).all()
        rc, out = raw(8, 12, 1)
        assert rc == 0
        assert torch.isnan(out[:, 0]).all() and not torch.isnan(
            out[:, 1:]).any()
        # a ring of another channel count, an odd-CIN variant
        rc, out = raw(8, 12, 1, proc=se.proc[:, :8].contiguous(), c=8)
        assert rc == -6 and (out == -7.0).all()
        rc, out = raw(8, 12, 1, proc=se.proc[:, :7].contiguous(), c=7,
                      eng=engines["MyCNN2"])
        assert rc == -6 and (out == -7.0).all()

    def test_uncovered_variant_takes_the_reference_path(self, engines):
        me = engines["MyCNN2"]
        assert not me.supports_history(7)
        se = _ring(S, 7, seed=95)
        for nproc in (120, 200):
            se.nproc = nproc
            for sids in ([2, 0, 2], None):
                got = se.score_history(me, sids, 5, 12, _age())
                want = se.score_history_reference(me, sids, 5, 12, _age())
                jm = jmin_of(nproc, G, 5, 12)
                assert torch.equal(torch.isnan(got), torch.isnan(want))
                assert torch.equal(got[:, jm:], want[:, jm:])
                assert int(torch.isnan(got[0]).sum()) == jm

    def test_daemon_vets_a_reload_with_the_kernel(self, tmp_path):
        """serve --reload-check on the GPU: the same weights move nothing,
        a head bias raised by 10 is refused."""
        import copy
        from test_attribution import run_daemon
        from test_history import _save
        srv, _log = run_daemon(tmp_path, "gpu", device="cuda",
                               reload_check=4, reload_max_shift=0.2)
        assert srv.me.supports_history(srv.se.C)
        path = tmp_path / "gpu.pth"
        _save(srv.me.model, path)
        srv.model_path = str(path)
        before = srv.me
        assert srv.maybe_reload_model() is True and srv.me is not before
        g = srv.timer.gauges
        assert g["reload_checked_windows"] == 8
        assert g["reload_shift_max"] == 0.0 and g["reload_nonfinite"] == 0
        bad = copy.deepcopy(srv.me.model)
        with torch.no_grad():
            bad.out.bias += 10.0
        _save(bad, path, newer_than=srv._model_mtime)
        before = srv.me
        assert srv.maybe_reload_model() is False and srv.me is before
        assert g["reload_rejected_total"] == 1
        assert g["reload_shift_max"] > 0.2

    def test_offsets_past_2_31(self, engines):
        """The last stream of an (S, 10, 16384) ring of 2.16e9 elements lies
        past a 32-bit element offset: its row equals the same data scored in
        a one-stream ring, by the kernel bit for bit and by the reference
        path at the gate."""
        me = engines["MyCNN5"]
        big_s, big_g = 13200, 16384
        assert (big_s - 1) * 10 * big_g > 2 ** 31
        one = _ring(1, 10, seed=91, ring=big_g)
        one.nproc = end = big_g + 40                 # the windows wrap
        proc = torch.zeros(big_s, 10, big_g, device="cuda")
        proc[big_s - 1] = one.proc[0]
        sid = torch.tensor([big_s - 1, 0], dtype=torch.int32, device="cuda")
        got = me.history_ring(proc, big_g, end, sid, 3, 12, 0)
        same = me.history_ring(
            one.proc, big_g, end,
            torch.zeros(1, dtype=torch.int32, device="cuda"), 3, 12, 0)
        want = one.score_history_reference(me, [0], 3, 12, None, False,
                                           dtype=BF16)
        torch.cuda.synchronize()
        assert torch.equal(got[:1], same)
        assert not torch.equal(got[1:], same)        # stream 0 holds zeros
        torch.testing.assert_close(got[:1], want, rtol=RTOL, atol=ATOL)
        print(f"[history] past 2^31: max |kernel - reference| = "
              f"{(got[:1] - want).abs().max().item():.3e}")

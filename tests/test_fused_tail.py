"""Fused serving tail (window gather + conv + one LSTM step + head in one
kernel) against the unfused chain it replaces, kernel vs kernel, in the same
process on the same ring: ``windows(batch=1, bf16, timelast)`` followed by
``MyCNNEngine.forward``.

The ring is filled with seeded random fp32 values and ``nproc`` is set by
hand (no ingest). Hard gate: rtol = atol = 2e-3, the tolerance
tests/test_engine.py::TestTriggerGraph uses between graphed and eager
results; the expected difference is zero (same bf16 window, same operation
order for every kept term), and each test prints the maximum it saw.
"""

import pytest
import torch

from tskd_amd.engine import StreamEngine

G = 192  # small ring so the 120-point window can straddle the wrap
# 60: end < 120 -> all-zero window; 120: first full window; 191: ends one
# short of the ring end; 192: ends exactly at it; 200: straddles the wrap;
# 372 = 12 * 31: a steady-state position after a wrap
NPROCS = (60, 120, 191, 192, 200, 372)
RTOL = ATOL = 2e-3


@pytest.fixture(scope="module")
def engines():
    from tskd_amd.models import build_model
    from tskd_amd.ops import MyCNNEngine
    out = {}
    for i, name in enumerate(("MyCNN5", "MyCNN4", "MyCNN2")):
        torch.manual_seed(100 + i)
        out[name] = MyCNNEngine(build_model(name).eval(), device="cuda")
    return out


def _ring(S, C, seed):
    se = StreamEngine(S, C, ring_grid=G, fs=25.0, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    se.proc.copy_(torch.randn(S, C, G, device="cuda", generator=gen) * 2.0)
    return se


@pytest.mark.gpu
class TestFusedTail:
    # S = 3: odd pair tail; S = 9: a wave's second pair (4 waves x 2 windows
    # per workgroup, grid sized like the conv's) on reused LDS
    @pytest.mark.parametrize("S", [1, 3, 9])
    @pytest.mark.parametrize("variant", ["MyCNN5", "MyCNN4"])
    def test_matches_unfused_chain(self, engines, variant, S):
        me = engines[variant]
        assert me.supports_fused_tail(10)
        se = _ring(S, 10, seed=7 * S + len(variant))
        age_t = (40.0 + 7.0 * torch.arange(S, device="cuda",
                                           dtype=torch.float32)).reshape(S, 1)
        worst = 0.0
        seen = {}
        for nproc in NPROCS:
            se.nproc = nproc
            w = se.windows(batch=1, stride=12, dtype=torch.bfloat16,
                           timelast=True)
            if nproc < 120:
                assert not w.any()  # the reference window is all zeros
            for age in (None, age_t):
                for sig in (False, True):
                    ref = me.forward(w, age, apply_sigmoid=sig)
                    got = se.score_latest(me, age, apply_sigmoid=sig)
                    torch.cuda.synchronize()
                    assert got.shape == (S, 1) and ref.shape == (S, 1)
                    d = (got - ref).abs().max().item()
                    worst = max(worst, d)
                    torch.testing.assert_close(
                        got, ref, rtol=RTOL, atol=ATOL,
                        msg=lambda m: f"nproc={nproc} age={age is not None} "
                                      f"sigmoid={sig}: {m}")
                    if age is None and not sig:
                        seen[nproc] = got.clone()
        # the comparison is not vacuous: each ring position scores another
        # window, so the logits move with it
        for a, b in zip(NPROCS, NPROCS[1:]):
            assert not torch.equal(seen[a], seen[b]), (a, b)
        print(f"[fused tail] {variant} S={S}: max |fused - unfused| = "
              f"{worst:.3e}")

    def test_device_state_block_position(self, engines):
        """Ring position read from the device state block (+ extra), as a
        captured trigger does, equals the host-side position."""
        me = engines["MyCNN5"]
        se = _ring(3, 10, seed=31)
        se.nproc = 200
        ref = se.score_latest(me, None, apply_sigmoid=True).clone()
        dstate = torch.tensor([0, 188], dtype=torch.int64, device="cuda")
        se.nproc = 0  # must be ignored when the state block is set
        with se.device_state(dstate, gather_extra=12):
            got = se.score_latest(me, None, apply_sigmoid=True)
            torch.cuda.synchronize()
        assert torch.equal(got, ref)

    def test_unsupported_variant(self, engines):
        """MyCNN2 (7 channels, odd): not supported; the launcher refuses
        with its own code and TriggerGraph keeps the unfused path."""
        from tskd_amd.engine.stream_engine import TriggerGraph
        from tskd_amd.ops import GraphedForward
        me = engines["MyCNN2"]
        assert not me.supports_fused_tail(7)
        assert not me.supports_fused_tail(10)
        # MyCNN5 on a ring with another channel count is refused as well
        assert not engines["MyCNN5"].supports_fused_tail(8)
        se = _ring(4, 7, seed=41)
        se.nproc = 200
        with pytest.raises(RuntimeError, match="code -6"):
            se.score_latest(me, None)
        with pytest.raises(RuntimeError, match="code -6"):
            _ring(2, 8, seed=42).score_latest(engines["MyCNN5"], None)

        fs, S = 25.0, 4
        cm = list(range(7))
        gen = torch.Generator(device="cuda").manual_seed(43)
        chunks = [torch.randn(S, 7, int(fs * 60), device="cuda",
                              generator=gen).to(torch.bfloat16)
                  for _ in range(16)]
        e1 = StreamEngine(S, 7, ring_grid=G, fs=fs, device="cuda")
        eager = []
        for ch in chunks:
            e1.ingest_dense(ch, chan_map=cm)
            w = e1.windows(batch=1, stride=12, dtype=torch.bfloat16)
            eager.append(me.forward(w, None, apply_sigmoid=True).clone())
        e2 = StreamEngine(S, 7, ring_grid=G, fs=fs, device="cuda")
        raw = chunks[0].clone()
        idx = 0
        while e2.nproc == 0 or e2.nproc < e2.head - e2.win_buckets + 1:
            raw.copy_(chunks[idx])
            e2.ingest_dense(raw, chan_map=cm)
            idx += 1
        torch.cuda.synchronize()
        gf = GraphedForward(me, s=S, n=1, dtype=torch.bfloat16,
                            timelast=True, capture=False)
        gf.age.zero_()
        raw.copy_(chunks[idx])
        tg = TriggerGraph(e2, raw, cm, gf, stride=12)
        assert tg.fused_tail is False
        idx += 1
        while idx < len(chunks):
            raw.copy_(chunks[idx])
            out = tg.replay()
            torch.cuda.synchronize()
            torch.testing.assert_close(out, eager[idx], rtol=RTOL, atol=ATOL)
            idx += 1

    def test_trigger_graph_knob(self, engines, monkeypatch):
        """TriggerGraph fuses by default for MyCNN5 and leaves gf.x alone;
        TSKD_FUSED_TAIL=0 at capture time restores the unfused chain. Both
        graphs score the same trigger identically."""
        from tskd_amd.engine.stream_engine import TriggerGraph
        from tskd_amd.ops import GraphedForward
        me = engines["MyCNN5"]
        fs, S = 25.0, 5
        cm = list(range(8))
        gen = torch.Generator(device="cuda").manual_seed(51)
        chunk = torch.randn(S, 8, int(fs * 60), device="cuda",
                            generator=gen).to(torch.bfloat16)
        outs, flags, xs = [], [], []
        for knob in ("0", "1"):
            monkeypatch.setenv("TSKD_FUSED_TAIL", knob)
            se = StreamEngine(S, 10, ring_grid=G, fs=fs, device="cuda")
            while se.nproc == 0 or se.nproc < se.head - se.win_buckets + 1:
                se.ingest_dense(chunk, chan_map=cm)
            torch.cuda.synchronize()
            gf = GraphedForward(me, s=S, n=1, dtype=torch.bfloat16,
                                timelast=True, capture=False)
            tg = TriggerGraph(se, chunk, cm, gf, stride=12)
            for _ in range(12):  # past nproc = 120: a full, nonzero window
                out = tg.replay()
            assert se.nproc >= 120
            torch.cuda.synchronize()
            outs.append(out.clone())
            flags.append(tg.fused_tail)
            xs.append(bool(gf.x.any()))
        assert flags == [False, True]
        assert xs == [True, False]  # fused mode never writes gf.x
        d = (outs[0] - outs[1]).abs().max().item()
        print(f"[fused tail] graph knob 0 vs 1: max diff = {d:.3e}")
        torch.testing.assert_close(outs[1], outs[0], rtol=RTOL, atol=ATOL)

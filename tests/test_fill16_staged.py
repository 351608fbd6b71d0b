"""Staged steady-state window fill (``TSKD_FILL16_STAGED=1``, the default:
each 16-lane group loads its row's bucket span once into LDS) against the
per-lane L1 loop it replaces (``=0``), kernel vs kernel, in one process.

Two ``StreamEngine``s get identical seeded packed bucket rings and
``last_val`` carries; ``_launch_fill`` runs under each knob value and ``proc``
and ``last_val`` must be BITWISE equal (int32 views: NaN carries occur). The
staged kernel keeps the loop's association — segment 1 up to the ring end
dealt round-robin into four accumulators with the < 4 remainder into the
first, segment 2 again from the first, ``(a0 + a1) + (a2 + a3)`` — so there
is no tolerance: any difference is a bug.

Ring positions are given as ``phead % G`` relative to the span
``np + win_buckets - 1`` of bucket pairs a row reads.

The TriggerGraph parity runs at G = 192, not 64: the model window is 120
grid points, so neither the gather nor the fused tail accepts a ring shorter
than that. 40 triggers of 12 points are 2.5 turns of that ring.
"""

import pytest
import torch

from tskd_amd.engine import StreamEngine

WIN = 36
SENTINEL = 7.25  # proc outside the filled points must keep it


def _s0(pos: str, G: int, npn: int, win: int = WIN) -> int:
    span = npn + win - 1
    return {
        "nowrap": 5,                            # span well inside the ring
        "exact": G - span,                      # span ends exactly at G
        "last": G - span + 1,                   # only the last window wraps
        "middle": G - span + max(1, npn // 2),  # wrap from a middle window on
        "first": G - win + 2,                   # first window: 34 + 2 elements
        "before": G - 2,                        # windows 2.. start past the end
        "before1": G - 1,
    }[pos]


POSITIONS = ("nowrap", "exact", "last", "middle", "first", "before", "before1")
FILLS = ("dense", "empty", "bfill", "ffill")


def _make(S, C, G, npn, pos, fill, win=WIN, seed=0):
    """Seeded bucket ring, carries and ring position for one case."""
    s0 = _s0(pos, G, npn, win)
    phead = 3 * G + s0
    gen = torch.Generator(device="cuda").manual_seed(
        seed + 1000 * S + 100 * C + G + 7 * npn + s0)
    cnt = torch.randint(0, 5, (S, C, G), device="cuda",
                        generator=gen).float()
    val = torch.randn(S, C, G, device="cuda", generator=gen) * 30.0 + 80.0
    carry = torch.randn(S, C, device="cuda", generator=gen)
    # every third row starts without a carry (NaN)
    rows = torch.arange(S * C, device="cuda").reshape(S, C)
    carry[rows % 3 == 0] = float("nan")
    slot = (torch.arange(G, device="cuda") - s0) % G  # ring elem -> span slot
    if fill == "empty":
        cnt.zero_()
    elif fill == "bfill":
        # NaN carry; windows 0..p-1 empty, window p the first with data
        p = min(3, npn - 1)
        carry.fill_(float("nan"))
        cnt[:, :, slot < p + win - 1] = 0.0
        cnt[:, :, slot == p + win - 1] = 2.0
    elif fill == "ffill":
        # carry set; windows lo..hi-1 empty in the interior of the batch
        lo, hi = min(4, npn - 1), min(7, npn)
        carry.copy_(torch.randn(S, C, device="cuda", generator=gen))
        cnt[:, :, (slot >= lo) & (slot < hi + win - 1)] = 0.0
        cnt[:, :, slot < lo] = 3.0
        cnt[:, :, slot == hi + win - 1] = 1.0
    bkt = torch.stack((val * cnt, cnt), dim=-1)
    return bkt, carry, phead


def _run(knob, monkeypatch, S, C, G, npn, bkt, carry, phead, win=WIN):
    monkeypatch.delenv("TSKD_PACKED_BUCKETS", raising=False)
    monkeypatch.setenv("TSKD_FILL16_STAGED", knob)
    se = StreamEngine(S, C, ring_grid=G, fs=25.0, win_buckets=win,
                      device="cuda")
    assert se._packed
    se._bkt.copy_(bkt)
    se.last_val.copy_(carry)
    se.proc.fill_(SENTINEL)
    se._launch_fill(phead, npn)
    torch.cuda.synchronize()
    return se.proc.clone(), se.last_val.clone()


def _check(monkeypatch, S, C, G, npn, pos, fill, win=WIN):
    bkt, carry, phead = _make(S, C, G, npn, pos, fill, win)
    p0, l0 = _run("0", monkeypatch, S, C, G, npn, bkt, carry, phead, win)
    p1, l1 = _run("1", monkeypatch, S, C, G, npn, bkt, carry, phead, win)
    nbad = (p0.view(torch.int32) != p1.view(torch.int32)).sum().item()
    lbad = (l0.view(torch.int32) != l1.view(torch.int32)).sum().item()
    print(f"[fill16 staged] S={S} C={C} G={G} np={npn} {pos} {fill}: "
          f"{nbad} proc / {lbad} last_val words differ")
    assert nbad == 0 and lbad == 0
    # not vacuous: exactly the np new points were written, with no NaN left
    idx = (phead + torch.arange(npn, device="cuda")) % G
    mask = torch.zeros(G, dtype=torch.bool, device="cuda")
    mask[idx] = True
    assert (p1[:, :, ~mask] == SENTINEL).all()
    assert not torch.isnan(p1[:, :, mask]).any()
    if fill == "dense":
        assert (p1[:, :, mask] != SENTINEL).all()
    if fill == "empty":
        # all-empty rows: the carry where there is one, else fillna(0)
        want = torch.where(torch.isnan(carry), torch.zeros_like(carry), carry)
        assert torch.equal(p1[:, :, mask],
                           want[:, :, None].expand(S, C, npn))
        assert (l1.view(torch.int32) == carry.view(torch.int32)).all()


@pytest.mark.gpu
class TestFill16Staged:
    # S * C not a multiple of 4: the last wave has dead 16-lane groups
    @pytest.mark.parametrize("C", [10, 3])
    @pytest.mark.parametrize("S", [1, 3, 9])
    def test_rows(self, monkeypatch, S, C):
        _check(monkeypatch, S, C, 64, 12, "nowrap", "dense")
        _check(monkeypatch, S, C, 64, 12, "first", "dense")

    @pytest.mark.parametrize("pos", POSITIONS)
    @pytest.mark.parametrize("npn", [1, 12, 16])
    @pytest.mark.parametrize("G", [64, 2048])
    def test_ring_positions(self, monkeypatch, G, npn, pos):
        _check(monkeypatch, 9, 10, G, npn, pos, "dense")

    @pytest.mark.parametrize("pos", POSITIONS)
    @pytest.mark.parametrize("fill", FILLS[1:])
    def test_fill_states(self, monkeypatch, fill, pos):
        _check(monkeypatch, 9, 10, 64, 12, pos, fill)

    @pytest.mark.parametrize("pos", ["nowrap", "first", "before"])
    def test_other_window_length(self, monkeypatch, pos):
        """win_buckets != 36 takes the kernel's run-time-length instance."""
        _check(monkeypatch, 9, 10, 64, 12, pos, "dense", win=22)

    def test_trigger_graph_parity(self, monkeypatch):
        """One graph captured under each knob value scores 40 triggers
        (2.5 ring turns) identically."""
        from tskd_amd.engine.stream_engine import TriggerGraph
        from tskd_amd.models import build_model
        from tskd_amd.ops import GraphedForward, MyCNNEngine
        torch.manual_seed(100)
        me = MyCNNEngine(build_model("MyCNN5").eval(), device="cuda")
        fs, S, G = 25.0, 9, 192
        cm = list(range(8))  # channels 8, 9 never fed: all-empty rows

        def chunk(i):
            gen = torch.Generator(device="cuda").manual_seed(500 + i)
            # a level per (stream, channel, trigger) of the size the model's
            # tanh layers resolve, so the scores move from trigger to trigger
            x = torch.randn(S, 8, int(fs * 60), device="cuda",
                            generator=gen) * 10.0 + \
                torch.randn(S, 8, 1, device="cuda", generator=gen) * 1.5
            if 10 <= i < 15:       # 300 s of silence: empty windows, ffill
                x[: S // 2, 3] = float("nan")
            return x.to(torch.bfloat16)

        probs = []
        for knob in ("0", "1"):
            monkeypatch.setenv("TSKD_FILL16_STAGED", knob)
            se = StreamEngine(S, 10, ring_grid=G, fs=fs, device="cuda")
            raw = chunk(0).clone()
            while se.nproc == 0 or se.nproc < se.head - se.win_buckets + 1:
                se.ingest_dense(raw, chan_map=cm)
            torch.cuda.synchronize()
            gf = GraphedForward(me, s=S, n=1, dtype=torch.bfloat16,
                                timelast=True, capture=False)
            tg = TriggerGraph(se, raw, cm, gf, stride=12)
            outs = []
            for i in range(40):
                raw.copy_(chunk(i))
                outs.append(tg.replay().clone())
            torch.cuda.synchronize()
            assert se.nproc > 2 * G
            probs.append(torch.stack(outs))
        d = (probs[0] - probs[1]).abs().max().item()
        print(f"[fill16 staged] graph knob 0 vs 1, 40 triggers: "
              f"max diff = {d:.3e}")
        assert torch.equal(probs[0].view(torch.int32),
                           probs[1].view(torch.int32))
        assert not torch.equal(probs[0][12], probs[0][39])

"""HIP op dispatch for the MyCNN inference path.

GPU tensors run on the hand-written CDNA4 kernels (csrc/mycnn_kernels.hip)
— REQUIRED on a GPU box: if the extension .so is missing we raise instead of
silently falling back to eager PyTorch. CPU tensors use the PyTorch-eager
model itself (the numerics oracle the kernels are tested against).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from tskd_amd.ops import hip
from tskd_amd.ops.pack import (VARIANT_IDS, pack_conv1_mfma_bfrags,  # noqa: F401
                               pack_weights)


def hip_available() -> bool:
    try:
        hip.load(hip.MYCNN)
        return True
    except Exception:
        return False


def _age_ptr(age: Optional[torch.Tensor], s: int, n: int) -> Tuple:
    """``age`` as a contiguous fp32 (s, n) tensor and its device pointer
    (None -> null). Returns (pointer, tensor): hold the tensor until the
    launch."""
    if age is not None and (age.dtype != torch.float32 or age.shape != (s, n)
                            or not age.is_contiguous()):
        age = age.to(torch.float32).expand(s, n).contiguous()
    return hip.ptr(age), age


# trailing elements the timelast conv kernel may overread: they must be
# addressable, their contents never reach a result
TLAST_SLACK = 256

# channel-attribution baselines -> OCCLUDE_* in csrc/mycnn_kernels.hip
BASELINES = {"hold": 0, "zero": 1}


def alloc_windows(s: int, n: int, cin: int, win: int = 120,
                  timelast: bool = False, dtype=torch.bfloat16,
                  device="cuda") -> torch.Tensor:
    """Allocate a window tensor with the trailing slack the timelast
    (LDS-free) conv kernel requires; returns a (s, n, cin, win) or
    (s, n, win, cin) view tagged slack-safe."""
    numel = s * n * cin * win
    buf = torch.zeros(numel + TLAST_SLACK, dtype=dtype, device=device)
    shape = (s, n, win, cin) if timelast else (s, n, cin, win)
    t = buf[:numel].view(*shape)
    t._tskd_slack = True  # type: ignore[attr-defined]
    t._tskd_buf = buf  # keep storage alive  # type: ignore[attr-defined]
    return t


class MyCNNEngine:
    """Device-resident packed-weight inference engine for one MyCNN model.

    forward semantics == the reference model in eval mode,
    including the LSTM batch-axis-as-time quirk: ``x`` is (S, N, C, 120) —
    S independent sequences whose N windows each form one LSTM "batch".
    A reference-style single call is S=1.
    """

    def __init__(self, model, device: str = "cuda"):
        from tskd_amd.models.mycnn import _MyCNNBase
        assert isinstance(model, _MyCNNBase)
        self.variant = VARIANT_IDS[type(model).__name__]
        self.age_eps = float(model.AGE_EPS)
        self.cin = int(model.IN_CHANNELS)
        self.device = torch.device(device)
        self.model = model  # CPU oracle / fallback
        self.wpack = pack_weights(model).to(self.device)
        self.bfrag = pack_conv1_mfma_bfrags(model).to(self.device)
        if self.device.type == "cuda":
            lib = hip.load(hip.MYCNN)  # raises loudly if unavailable
            expect = lib.tskd_pack_size(self.variant)
            if expect != self.wpack.numel():
                raise RuntimeError(
                    f"weight pack size mismatch: py={self.wpack.numel()} "
                    f"hip={expect}")
            self.feat_len = lib.tskd_feat_len(self.variant)
        else:
            self.feat_len = int(model.MAGICNUM)

    def conv_features(self, x: torch.Tensor) -> torch.Tensor:
        """(..., C, 120) or timelast (..., 120, C) -> (..., LIN) features.

        The timelast layout runs the LDS-free MFMA kernel (even channel
        counts, bf16); its fragment reads may overrun the tensor by up to
        TLAST_SLACK elements, so non-slack-tagged inputs are copied into a
        padded buffer (allocate with :func:`alloc_windows` to avoid that).
        What the overrun reads, the slack or the next window, reaches no
        result: the kernel clears those fragment words.
        """
        timelast = (x.shape[-1] == self.cin and x.shape[-2] == 120
                    and self.cin != 120)
        lead = x.shape[:-2]
        xf = x.reshape(-1, x.shape[-2], x.shape[-1]).contiguous()
        sn = xf.shape[0]
        if xf.device.type != "cuda":
            raise RuntimeError("conv_features is the GPU path; use the model on CPU")
        lib = hip.load(hip.MYCNN)
        if timelast and (self.cin % 2 != 0 or xf.dtype != torch.bfloat16):
            # odd-CIN / fp32: transpose back to the staged layout
            xf = xf.transpose(-1, -2).contiguous()
            timelast = False
        if xf.dtype == torch.bfloat16:
            is_bf16 = 1
        elif xf.dtype == torch.float32:
            is_bf16 = 0
        else:
            xf = xf.to(torch.float32)
            is_bf16 = 0
        if timelast and not getattr(x, "_tskd_slack", False):
            pad = alloc_windows(1, sn, self.cin, 120, timelast=True,
                                dtype=xf.dtype, device=xf.device)
            pad.reshape(-1).copy_(xf.reshape(-1))
            xf = pad.reshape(sn, 120, self.cin)
        feat = torch.empty(sn, self.feat_len, dtype=torch.float32, device=xf.device)
        hip.check(lib.tskd_conv_fwd(
            hip.ptr(xf), is_bf16, int(timelast), hip.ptr(feat),
            hip.ptr(self.wpack), hip.ptr(self.bfrag), sn, self.variant,
            hip.stream_ptr()), "tskd_conv_fwd")
        return feat.reshape(*lead, self.feat_len)

    def lstm_head(self, feat: torch.Tensor, age: Optional[torch.Tensor],
                  apply_sigmoid: bool = False) -> torch.Tensor:
        """(S, N, LIN) features -> (S, N) logits (or probabilities)."""
        assert feat.dim() == 3 and feat.shape[-1] == self.feat_len
        s, n = feat.shape[0], feat.shape[1]
        feat = feat.contiguous()
        lib = hip.load(hip.MYCNN)
        out = torch.empty(s, n, dtype=torch.float32, device=feat.device)
        age_ptr, age = _age_ptr(age, s, n)
        hip.check(lib.tskd_lstm_head_fwd(
            hip.ptr(feat), age_ptr, hip.ptr(out), hip.ptr(self.wpack), s, n,
            self.age_eps, int(apply_sigmoid), self.variant,
            hip.stream_ptr()), "tskd_lstm_head_fwd")
        return out

    def supports_fused_tail(self, n_channels: int) -> bool:
        """True when :meth:`score_ring` applies: a GPU engine whose model
        has an even channel count equal to the ring's (MyCNN5, MyCNN4)."""
        return (self.device.type == "cuda" and self.cin % 2 == 0
                and self.cin == int(n_channels))

    def score_ring(self, proc: torch.Tensor, G: int, end: int,
                   dstate_ptr=None, end_extra: int = 0,
                   age: Optional[torch.Tensor] = None,
                   apply_sigmoid: bool = False) -> torch.Tensor:
        """Score the latest window of every stream straight from a
        StreamEngine's (S, C, G) fp32 ``proc`` ring: window gather + conv +
        one LSTM step + head in ONE kernel (B = 1, N = 1). The window ends
        at ``end`` (or at ``dstate[1] + end_extra`` when ``dstate_ptr`` is a
        device int64[2] state block, as in the window gather). Returns
        (S, 1) fp32; equals ``windows(batch=1, bf16, timelast)`` followed by
        :meth:`forward`. Raises for variants the kernel does not cover."""
        assert proc.dim() == 3 and proc.dtype == torch.float32 \
            and proc.is_contiguous() and proc.shape[2] == G
        s, c = proc.shape[0], proc.shape[1]
        lib = hip.load(hip.MYCNN)
        out = torch.empty(s, 1, dtype=torch.float32, device=proc.device)
        age_ptr, age = _age_ptr(age, s, 1)
        hip.check(lib.tskd_serve_tail_fwd(
            hip.ptr(proc), s, c, int(G), int(end),
            dstate_ptr if dstate_ptr is not None else hip.ptr(None),
            int(end_extra), age_ptr, hip.ptr(out), hip.ptr(self.wpack),
            hip.ptr(self.bfrag), self.age_eps, int(apply_sigmoid),
            self.variant, hip.stream_ptr()), "tskd_serve_tail_fwd")
        return out

    def supports_attribution(self, n_channels: int) -> bool:
        """True when :meth:`attribute_ring` applies: the coverage of
        :meth:`score_ring`."""
        return self.supports_fused_tail(n_channels)

    def attribute_ring(self, proc: torch.Tensor, G: int, end: int, sids,
                       age: Optional[torch.Tensor] = None,
                       baseline: str = "hold",
                       apply_sigmoid: bool = False) -> torch.Tensor:
        """Occlusion scores of the listed streams' latest windows straight
        from a StreamEngine's (S, C, G) fp32 ``proc`` ring, in ONE kernel:
        (n, C + 1) fp32, column 0 the score of the window ending at ``end``
        as :meth:`score_ring` gives it, column k the score with channel
        k - 1 replaced for all 120 points by a constant — the window's
        oldest point (``baseline="hold"``: a flat line, what the forward-fill
        carry makes of a lead that fell off) or +0.0 (``"zero"``: a channel
        that never arrived). ``sids``: int32 device tensor of n stream ids
        (rows follow it, duplicates are harmless, an id outside [0, S) is
        skipped and its row left unwritten); ``age``: (n,) / (n, 1) per
        listed stream, or None. The ring position is passed by value: legal
        between graph replays, not captured. Raises for variants the kernel
        does not cover and for an unknown baseline."""
        if baseline not in BASELINES:
            raise ValueError(f"baseline {baseline!r} not in {list(BASELINES)}")
        assert proc.dim() == 3 and proc.dtype == torch.float32 \
            and proc.is_contiguous() and proc.shape[2] == G
        assert sids.dtype == torch.int32 and sids.dim() == 1 \
            and sids.is_contiguous() and sids.device == proc.device
        s, c, n = proc.shape[0], proc.shape[1], sids.numel()
        out = torch.empty(n, c + 1, dtype=torch.float32, device=proc.device)
        if n == 0:
            return out
        age_ptr, age = _age_ptr(
            None if age is None else age.reshape(n, 1), n, 1)
        hip.check(hip.load(hip.MYCNN).tskd_serve_tail_occlude_fwd(
            hip.ptr(proc), s, c, int(G), int(end), hip.ptr(sids), n, age_ptr,
            BASELINES[baseline], hip.ptr(out), hip.ptr(self.wpack),
            hip.ptr(self.bfrag), self.age_eps, int(apply_sigmoid),
            self.variant, hip.stream_ptr()), "tskd_serve_tail_occlude_fwd")
        return out

    def supports_history(self, n_channels: int) -> bool:
        """True when :meth:`history_ring` applies: the coverage of
        :meth:`score_ring`."""
        return self.supports_fused_tail(n_channels)

    def history_ring(self, proc: torch.Tensor, G: int, end: int, sids,
                     k: int, stride: int, jmin: int,
                     age: Optional[torch.Tensor] = None,
                     apply_sigmoid: bool = False) -> torch.Tensor:
        """Scores of the listed streams at ``k`` window positions straight
        from a StreamEngine's (S, C, G) fp32 ``proc`` ring, in ONE kernel:
        (n, k) fp32, column j the score of the window ending at ``end -
        (k-1-j)*stride`` as :meth:`score_ring` gives it at that end (every
        window its own one-step sequence), oldest first. Columns below
        ``jmin`` are NaN and nothing of them is read; column ``jmin`` must
        neither start before grid point 0 nor reach slots the ring has
        already overwritten (``end - G``), else the launcher refuses with
        code -5. ``sids``: int32 device tensor of n stream ids (rows follow
        it, duplicates are harmless, an id outside [0, S) is skipped and its
        row left unwritten); ``age``: (n,) / (n, 1) per listed stream, one
        age for all of its columns, or None. The ring position is passed by
        value: legal between graph replays, not captured. Raises for
        variants the kernel does not cover."""
        assert proc.dim() == 3 and proc.dtype == torch.float32 \
            and proc.is_contiguous() and proc.shape[2] == G
        assert sids.dtype == torch.int32 and sids.dim() == 1 \
            and sids.is_contiguous() and sids.device == proc.device
        s, c, n = proc.shape[0], proc.shape[1], sids.numel()
        out = torch.empty(n, int(k), dtype=torch.float32, device=proc.device)
        if n == 0:
            return out
        age_ptr, age = _age_ptr(
            None if age is None else age.reshape(n, 1), n, 1)
        hip.check(hip.load(hip.MYCNN).tskd_serve_tail_history_fwd(
            hip.ptr(proc), s, c, int(G), int(end), hip.ptr(sids), n, age_ptr,
            int(k), int(stride), int(jmin), hip.ptr(out),
            hip.ptr(self.wpack), hip.ptr(self.bfrag), self.age_eps,
            int(apply_sigmoid), self.variant, hip.stream_ptr()),
            "tskd_serve_tail_history_fwd")
        return out

    def forward(self, x: torch.Tensor, age: Optional[torch.Tensor] = None,
                apply_sigmoid: bool = False) -> torch.Tensor:
        """x: (N, C, 120) single sequence, or (S, N, C, 120).

        Returns (N,) or (S, N) logits (probabilities if apply_sigmoid).
        """
        squeeze = x.dim() == 3
        if squeeze:
            x = x.unsqueeze(0)
            if age is not None and age.dim() == 1:
                age = age.unsqueeze(0)
        assert x.dim() == 4 and (
            (x.shape[-1] == 120 and x.shape[-2] == self.cin)
            or (x.shape[-2] == 120 and x.shape[-1] == self.cin))
        if x.device.type == "cuda":
            s, n = x.shape[0], x.shape[1]
            feat = self.conv_features(x).reshape(s, n, self.feat_len)
            out = self.lstm_head(feat, age, apply_sigmoid)
        else:
            s, n = x.shape[0], x.shape[1]
            if x.shape[-1] == self.cin and x.shape[-2] == 120:
                x = x.transpose(-1, -2)  # timelast input on the CPU path
            with torch.no_grad():
                outs = []
                for i in range(s):
                    a = age[i] if age is not None else torch.zeros(n)
                    y = self.model(x[i].float(), a.float())
                    outs.append(torch.sigmoid(y) if apply_sigmoid else y)
                out = torch.stack(outs)
        return out[0] if squeeze else out

    __call__ = forward


class GraphedForward:
    """hipGraph-captured micro-batch inference (BASELINE.json north star).

    Captures the fused conv+LSTM+head+sigmoid kernel sequence for a fixed
    (S, N) shape into a hipGraph (torch.cuda.CUDAGraph on ROCm) with static
    input/output buffers; replay eliminates per-kernel launch overhead in
    the serving hot loop. Fill ``x``/``age`` in place (or let the preprocess
    window-gather write directly into ``x``), then call ``replay()``.
    """

    def __init__(self, engine: "MyCNNEngine", s: int, n: int,
                 dtype: torch.dtype = torch.bfloat16,
                 apply_sigmoid: bool = True, warmup: int = 2,
                 timelast: bool = False, capture: bool = True):
        assert engine.device.type == "cuda"
        self.engine = engine
        self.timelast = timelast
        self.x = alloc_windows(s, n, engine.cin, 120, timelast=timelast,
                               dtype=dtype, device=engine.device)
        self.age = torch.full((s, n), 65.0, device=engine.device)
        self.graph = None
        if not capture:
            return  # buffers only (e.g. inside a TriggerGraph capture)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                out = engine.forward(self.x, self.age,
                                     apply_sigmoid=apply_sigmoid)
        torch.cuda.current_stream().wait_stream(stream)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = engine.forward(self.x, self.age,
                                      apply_sigmoid=apply_sigmoid)

    def replay(self) -> torch.Tensor:
        self.graph.replay()
        return self.out

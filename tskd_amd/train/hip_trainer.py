"""MyCNNHipTrainer — the MI355X-native training step (BASELINE config 5).

Runs the full training step on the hand-written HIP kernel set
(csrc/train_kernels.hip): fused conv forward-with-stash, LSTM scan
forward-with-stash, BCEWithLogits(pos_weight) loss+grad, reverse BPTT and
conv backward, DP gradient all-reduce (RCCL over xGMI when distributed),
and a fused Adam step over the single packed parameter buffer.

Semantics match the reference training recipe (explore_torch.ipynb cell 26;
tskd_amd/train/trainer.py is the torch-eager parity implementation): the
LSTM batch-axis-as-time quirk holds per sequence, targets are per-window
{0,1}, loss is the mean weighted BCE over all S*B windows.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from tskd_amd.ops import hip
from tskd_amd.ops.hip import check, ptr
from tskd_amd.ops.pack import (VARIANT_IDS, pack_offsets, pack_weights,
                               unpack_weights_into)


class MyCNNHipTrainer:
    def __init__(self, model, device: str = "cuda", lr: float = 1e-5,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 pos_weight: float = 1.0, train_dropout: bool = True,
                 seed: int = 0):
        self.model = model
        # reference train-mode dropout sites: MyCNN5 drops
        # after BOTH pools; MyCNN2/3/4 only after pool2
        p_drop = float(model.DROPOUT_P) if train_dropout else 0.0
        self.drop1_p = p_drop if getattr(model, "TWO_DROPOUT_SITES", True) \
            else 0.0
        self.drop2_p = p_drop
        self.seed = int(seed)
        self.variant = VARIANT_IDS[type(model).__name__]
        self.age_eps = float(model.AGE_EPS)
        self.cin = int(model.IN_CHANNELS)
        self.lin = int(model.MAGICNUM)
        self.device = torch.device(device)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.pos_weight = float(pos_weight)
        self.offsets = pack_offsets(model)
        self.wpack = pack_weights(model).to(self.device)
        self.grads = torch.zeros_like(self.wpack)
        self.m = torch.zeros_like(self.wpack)
        self.v = torch.zeros_like(self.wpack)
        self.step_count = 0
        self._probe_stash_sizes()

    def _probe_stash_sizes(self):
        cw, lw = ctypes.c_int(), ctypes.c_int()
        check(hip.load(hip.TRAIN).tskd_train_stash_sizes(
            self.variant, ctypes.byref(cw), ctypes.byref(lw)),
            "tskd_train_stash_sizes")
        self._stash_conv_words = cw.value
        self._stash_lstm_words = lw.value

    def forward_backward(self, x: torch.Tensor, age: Optional[torch.Tensor],
                         y: torch.Tensor) -> float:
        """x (S, B, C, 120) fp32, y (S, B) in {0,1}. Accumulates into grads;
        returns the scalar loss."""
        lib = hip.load(hip.TRAIN)
        assert x.dim() == 4 and x.shape[2] == self.cin and x.shape[3] == 120
        S, B = x.shape[0], x.shape[1]
        SN = S * B
        dev = self.device
        x = x.to(dev, torch.float32).contiguous()
        y = y.to(dev, torch.float32).reshape(S, B).contiguous()
        if age is not None:
            age = age.to(dev, torch.float32).expand(S, B).contiguous()
        feat = torch.empty(SN, self.lin, device=dev)
        stash_c = torch.empty(SN, self._stash_conv_words, device=dev)
        self._last_stash_conv = stash_c  # exposed for mask-exact testing
        stash_l = torch.empty(S, B, self._stash_lstm_words, device=dev)
        logits = torch.empty(S, B, device=dev)
        dlogit = torch.empty(S, B, device=dev)
        dfeat = torch.empty(S, B, self.lin, device=dev)
        loss = torch.zeros(1, device=dev)
        st = hip.stream_ptr()
        age_p = ptr(age)
        wpack, grads = ptr(self.wpack), ptr(self.grads)
        self.seed += 1  # fresh dropout masks every call
        check(lib.tskd_train_conv_fwd(
            ptr(x), ptr(feat), ptr(stash_c), wpack, SN, self.drop1_p,
            self.drop2_p, self.seed, self.variant, st), "tskd_train_conv_fwd")
        check(lib.tskd_train_lstm_fwd(
            ptr(feat), age_p, wpack, ptr(stash_l), ptr(logits), S, B,
            self.age_eps, self.variant, st), "tskd_train_lstm_fwd")
        check(lib.tskd_train_loss(
            ptr(logits), ptr(y), age_p, ptr(dlogit), ptr(loss), SN,
            self.pos_weight, self.age_eps, st), "tskd_train_loss")
        check(lib.tskd_train_lstm_bwd(
            ptr(feat), ptr(dlogit), ptr(stash_l), wpack, grads, ptr(dfeat),
            S, B, self.variant, st), "tskd_train_lstm_bwd")
        check(lib.tskd_train_conv_bwd(
            ptr(x), ptr(stash_c), ptr(dfeat), wpack, grads, SN, self.variant,
            st), "tskd_train_conv_bwd")
        return float(loss.item())

    def optimizer_step(self) -> None:
        """DP all-reduce (when distributed) + fused Adam + grad zeroing."""
        import torch.distributed as dist
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.grads)
            self.grads /= dist.get_world_size()
        self.step_count += 1
        check(hip.load(hip.TRAIN).tskd_train_adam(
            ptr(self.wpack), ptr(self.grads), ptr(self.m), ptr(self.v),
            self.wpack.numel(), self.lr, self.betas[0], self.betas[1],
            self.eps, self.step_count, hip.stream_ptr()), "tskd_train_adam")

    def step(self, x, age, y) -> float:
        loss = self.forward_backward(x, age, y)
        assert loss == loss, "model diverged with loss = NaN"  # tripwire
        self.optimizer_step()
        return loss

    def export_model(self):
        unpack_weights_into(self.model, self.wpack)
        return self.model

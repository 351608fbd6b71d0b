"""Training metrics — reference bin/utils.py:104-134 semantics."""

from __future__ import annotations

import torch


class AverageMeter:
    """Running average meter (reference utils.py:104-120)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0.0
        self.avg = 0.0
        self.sum = 0.0
        self.count = 0

    def update(self, val, n: int = 1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / max(self.count, 1)


def compute_batch_accuracy(output: torch.Tensor,
                           target: torch.Tensor) -> torch.Tensor:
    """sigmoid -> round -> eq -> mean (reference utils.py:122-134).
    `output` is logits, `target` in {0,1}. On CUDA this is the fused K14
    metric kernel (one pass, no intermediate tensors); the HIP extension
    is REQUIRED there — no silent eager fallback."""
    with torch.no_grad():
        batch_size = target.size(0)
        if output.is_cuda:
            return _batch_accuracy_hip(output, target, batch_size)
        pred = torch.sigmoid(output).round()
        correct = pred.eq(target.view_as(pred)).sum()
        return correct.float() * 100.0 / batch_size


def _batch_accuracy_hip(output: torch.Tensor, target: torch.Tensor,
                        batch_size: int) -> torch.Tensor:
    """K14 fused metric kernel (ops/csrc/train_kernels.hip)."""
    from tskd_amd.ops import hip
    lo = output.detach().reshape(-1).float().contiguous()
    tg = target.detach().reshape(-1).float().contiguous()
    out = torch.zeros(1, device=output.device)
    hip.check(hip.load(hip.TRAIN).tskd_train_batch_accuracy(
        hip.ptr(lo), hip.ptr(tg), hip.ptr(out), lo.numel(),
        hip.stream_ptr()), "tskd_train_batch_accuracy")
    return out[0] * 100.0 / batch_size

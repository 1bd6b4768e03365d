"""The CTR validation metric — sklearn's roc_auc_score and log_loss over a whole validation set (reference:
src/trainer/deepfm.py:96-139) — on the kernels of csrc/ctr_metric.hip: `binary_auc` and the accumulator `CTRMetric`
that `trainer.validate_epoch` feeds one batch at a time."""
from typing import Dict, Optional

import torch

from . import _kernels

_ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def _binary_auc_torch(y_true: torch.Tensor, y_score: torch.Tensor) -> float:
    """binary_auc on stock torch ops, in float64 (any device, any dtype): what CPU tensors take, and the form the
    kernel path is measured against."""
    y_true = y_true.reshape(-1).to(torch.float64)
    uniq, inverse, counts = torch.unique(y_score.reshape(-1), sorted=True, return_inverse=True, return_counts=True)
    ends = torch.cumsum(counts, 0).to(torch.float64)
    avg_rank = ends - (counts.to(torch.float64) - 1.0) / 2.0          # 1-based average rank of each distinct score
    n_pos = y_true.sum()
    n_neg = y_true.numel() - n_pos
    if float(n_pos) == 0.0 or float(n_neg) == 0.0:
        raise ValueError(_ONE_CLASS)
    rank_sum = (avg_rank[inverse] * y_true).sum()
    return float((rank_sum - n_pos * (n_pos + 1.0) / 2.0) / (n_pos * n_neg))


def _label_bytes(y_true: torch.Tensor) -> torch.Tensor:
    """Labels of any integer, bool or float dtype as the bytes mi_binary_auc reads: 1, 0, or 2 for any other value."""
    y = y_true.reshape(-1)
    if y.dtype == torch.uint8:
        return y.contiguous()
    if y.dtype == torch.bool:
        return y.to(torch.uint8)
    return torch.where(y == 1, 1, torch.where(y == 0, 0, 2)).to(torch.uint8)


def _auc_of_record(rec: dict) -> float:
    """The record of mi_binary_auc as binary_auc's result or its ValueError."""
    if rec["bad"]:
        raise ValueError(f"binary_auc takes labels 0 and 1; {rec['bad']} of them are neither")
    if rec["P"] == 0 or rec["N"] == 0:
        raise ValueError(_ONE_CLASS)
    return rec["auc"]                                                  # NaN when a score is NaN (rec["nan"] says how many)


def binary_auc(y_true: torch.Tensor, y_score: torch.Tensor) -> float:
    """Area under the ROC curve as sklearn.metrics.roc_auc_score computes it for binary labels (ties share their average
    rank: the Mann-Whitney statistic).  float32 scores on the GPU: mi_binary_auc, an integer count and one division, one
    host read; NaN when a score is NaN, ValueError when a label is neither 0 nor 1.  Everything else (CPU tensors, other
    dtypes): torch ops in float64.  ValueError when one class is absent."""
    if not (y_score.is_cuda and y_score.dtype == torch.float32 and y_score.is_contiguous() and y_true.is_cuda
            and y_true.numel() == y_score.numel()):
        return _binary_auc_torch(y_true, y_score)
    return _auc_of_record(_kernels.auc_record(_kernels.binary_auc_device(y_score.reshape(-1), _label_bytes(y_true))))


class CTRMetric:
    """{"auc", "log_loss"} of a validation set fed batch by batch.  On the GPU `add` is one launch without a sync (logits
    and label bytes into buffers that live as long as the object, the batch's BCE-with-logits sum in float64 onto a device
    double), `compute` ranks torch.sigmoid of the whole buffer with mi_binary_auc and reads the device once.  On the CPU
    the same numbers come from torch ops.  capacity: the number of samples to size the buffers for (they double when it
    is unknown or exceeded)."""

    def __init__(self, device="cuda", capacity: Optional[int] = None):
        self.device = torch.device(device)
        self._gpu = self.device.type == "cuda"
        self._n = 0
        self._result: Optional[Dict[str, float]] = None
        if self._gpu:
            self._cap = 0
            self._score = self._label = None
            # the record of mi_binary_auc and the loss sum side by side: one copy reads both
            self._words = torch.zeros(_kernels.AUC_RECORD_WORDS + 1, dtype=torch.int64, device=self.device)
            self._loss_sum = self._words[_kernels.AUC_RECORD_WORDS:].view(torch.float64)
            self._ws = _kernels.ctr_metric_workspace(self.device)
            self._reserve(int(capacity) if capacity else 0)
        else:
            self._logits, self._labels = [], []

    def __len__(self) -> int:
        return self._n

    def _reserve(self, cap: int) -> None:
        if cap <= self._cap:
            return
        score = torch.empty(cap, dtype=torch.float32, device=self.device)
        label = torch.empty(cap, dtype=torch.uint8, device=self.device)
        if self._n:
            score[: self._n] = self._score[: self._n]
            label[: self._n] = self._label[: self._n]
        self._score, self._label, self._cap = score, label, cap

    def reset(self) -> None:
        """Forget the samples; the buffers stay."""
        self._n, self._result = 0, None
        if self._gpu:
            self._loss_sum.zero_()
        else:
            self._logits, self._labels = [], []

    @torch.no_grad()
    def add(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        logits, labels = logits.detach().reshape(-1), labels.detach().reshape(-1)
        if labels.numel() != logits.numel():
            raise ValueError(f"{logits.numel()} logits but {labels.numel()} labels")
        self._result = None
        b = logits.numel()
        if not self._gpu:
            self._logits.append(logits.to(self.device, torch.float32))
            self._labels.append(labels.to(self.device))
            self._n += b
            return
        if labels.dtype not in (torch.int64, torch.float32):
            labels = labels.to(torch.float32 if labels.is_floating_point() else torch.int64)
        if self._n + b > self._cap:
            self._reserve(max(2 * self._cap, self._n + b, 1024))
        _kernels.ctr_metric_append(logits.to(self.device, torch.float32), labels.to(self.device), self._n, self._score,
                                   self._label, self._loss_sum, self._ws)
        self._n += b

    @torch.no_grad()
    def compute(self) -> Dict[str, float]:
        """{"auc", "log_loss"}; calling it again returns the same numbers without touching the device."""
        if self._result is not None:
            return dict(self._result)
        if self._n == 0:
            raise ValueError("CTRMetric.compute() before any add()")
        if self._gpu:
            _kernels.binary_auc_device(torch.sigmoid(self._score[: self._n]), self._label[: self._n],
                                       out=self._words[: _kernels.AUC_RECORD_WORDS])
            words = self._words.cpu()                                  # the one host read
            auc = _auc_of_record(_kernels.auc_record(words))
            loss_sum = float(words[_kernels.AUC_RECORD_WORDS:].view(torch.float64))
        else:
            x, y = torch.cat(self._logits), torch.cat(self._labels)
            auc = _binary_auc_torch(y, torch.sigmoid(x))
            x, y = x.to(torch.float64), y.to(torch.float64)
            loss_sum = float((torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum())
        self._result = {"auc": auc, "log_loss": loss_sum / self._n}
        return dict(self._result)

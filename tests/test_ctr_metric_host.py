"""CPU: the CTR metric's entry points exist, its host-side contract, and CTRMetric's torch-op form on CPU tensors."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ctr_metric_helpers import BATCHES, bce_sum

from recsys_benchmark_amd import _lib, trainer

NAMES = ("mi_binary_auc", "mi_binary_auc_workspace_bytes", "mi_ctr_metric_append")


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "mi355x_recsys.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"MI_API\s+\w+\s+" + name + r"\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"


def test_workspace_bytes_grow_with_n():
    f = _lib.load().mi_binary_auc_workspace_bytes
    assert 0 <= f(0) <= 4096
    sizes = [f(n) for n in (0, 1, 2, 63, 1024, 1025, 4097, 70_001, 300_007, 4_584_062, 2**31 - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[1] >= 8 and sizes[-1] >= 8 * (2**31 - 1)          # two key buffers at the least


def test_append_rejects_a_batch_past_the_capacity_before_touching_the_device():
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                      # never dereferenced: the sizes are checked first
    assert lib.mi_ctr_metric_append(one, one, 0, 5, 60, one, one, 64, one, one, None) == -1
    assert lib.mi_ctr_metric_append(one, one, 7, 4, 60, one, one, 64, one, one, None) == -1
    assert lib.mi_ctr_metric_append(one, one, 0, 0, 64, one, one, 64, one, one, None) == 0
    assert lib.mi_binary_auc(one, one, 2**31, one, one, None) == -2


def test_ctrmetric_is_public_and_validate_epoch_takes_one():
    from recsys_benchmark_amd import CTRMetric

    assert CTRMetric is trainer.CTRMetric
    assert "metric" in inspect.signature(trainer.validate_epoch).parameters


def test_ctrmetric_on_cpu_matches_sklearn():
    from sklearn.metrics import roc_auc_score

    from recsys_benchmark_amd import CTRMetric

    gen = torch.Generator().manual_seed(5)
    metric = CTRMetric("cpu", capacity=64)
    logits, labels = [], []
    for i, b in enumerate(BATCHES):
        x = 4 * torch.randn(b, generator=gen)
        y = (torch.rand(b, generator=gen) < 0.4)
        y = y.long() if i % 2 == 0 else y.float()
        metric.add(x, y)
        logits.append(x)
        labels.append(y.double())
    x, y = torch.cat(logits), torch.cat(labels)
    res = metric.compute()
    assert metric.compute() == res and len(metric) == sum(BATCHES)
    assert abs(res["auc"] - roc_auc_score(y.numpy(), torch.sigmoid(x).numpy())) < 1e-12
    want = bce_sum(x.numpy(), y.numpy()) / x.numel()
    assert abs(res["log_loss"] - want) <= 1e-12 * want
    metric.reset()
    metric.add(x[:300], y[:300])
    assert abs(metric.compute()["auc"] - roc_auc_score(y[:300].numpy(), torch.sigmoid(x[:300]).numpy())) < 1e-12
    with pytest.raises(ValueError):
        one = CTRMetric("cpu")
        one.add(x[:10], torch.ones(10))
        one.compute()

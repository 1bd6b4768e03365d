"""GPU: WHICH kernels the fused tail's host driver (recsys-benchmark_amd/tail.py) launches, in which order, pinned per case
against tests/golden/tail_launches.json (written by tests/golden/gen_golden_tail_launches.py from the tree the driver was
refactored from).  The numbers are the other tail files' business; this one holds the driver to its launch sequence: a step
that moves, adds or drops a launch — a finalize launch where the prologue should join, a mask launch of its own where the
bits should ride — fails here even when its results still agree.

Each case runs once to warm up (allocator, workspaces), then again eagerly inside profiling.KernelTimer, which records the
name of every kernel the library's launchers start."""
import contextlib
import json
import os

import pytest
import torch

import poison_helpers as ph
import test_tail_mixed_gpu as mixed

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import _lib
from recsys_benchmark_amd import mlp as _mlp
from recsys_benchmark_amd import tail as _tail_mod
from recsys_benchmark_amd.losses import unit_scalar
from recsys_benchmark_amd.profiling import KernelTimer

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_launches.json")
FORMS = {"sums": (True, False), "joins": (False, True), "finalize": (False, False)}     # form -> (STAT_SUMS, MERGE_JOINS)


@contextlib.contextmanager
def _settings(form, deterministic=False):
    """The statistics form of test_tail_gpu._fused_tail_on (and deterministic mode) for the block."""
    with ph._patched((_mlp, "FUSED_TAIL", True), (_tail_mod, "STAT_SUMS", FORMS[form][0]), (_tail_mod, "MERGE_JOINS", FORMS[form][1])), \
            ph._deterministic(deterministic):
        yield


def _grads(module, **named):
    out = {k: v for k, v in named.items() if v is not None}
    out.update({"g/" + k: ph.values_of(q.grad) for k, q in module.named_parameters() if q.grad is not None})
    out.update({"b/" + k: v.detach().clone() for k, v in module.named_buffers()})
    return out


def _tail_step(name, grad=True, x_grad=True, labels=False):
    """One step of a test_tail_mixed_gpu case: {name: tensor} of the logits, every gradient and the BatchNorm buffers."""
    seq, x, add, G, seed_value = mixed._inputs(name)
    M = x.shape[0]
    yd = (torch.rand(M, generator=torch.Generator().manual_seed(M)) < 0.4).float().to(DEV) if labels else None
    with torch.enable_grad() if grad else torch.no_grad():
        fs, xd, ad, out = mixed._fused_step(seq, x, add, G, seed_value, x_grad=x_grad, labels=yd, backward=grad and not labels)
        loss = None
        if labels:
            loss = pkg.BCEWithLogitsLoss()(out.squeeze(-1), yd)
            loss.backward(unit_scalar(DEV))
    return _grads(fs, out=out.detach(), loss=None if loss is None else loss.detach(), dx=xd.grad, dadd=ad.grad)


def _deepfm_step(labels):
    dims, D, B, hidden = [7, 3, 50, 11, 4, 200, 9, 31], 16, 67, [136, 24]
    torch.manual_seed(B + D)
    m = pkg.DeepFM(dims, D, hidden, p_dropout=0.5, use_batchnorm=True, embedding_config={"name": "vanilla", "sparse": True},
                   fc_sparse=True).train().to(DEV)
    gen = torch.Generator().manual_seed(B * 7 + D)
    x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV)
    yd = (torch.rand(B, generator=gen) < 0.3).float().to(DEV)
    _mlp._seed_word(torch.device(DEV, 0)).fill_(4321)
    logits = m(x, labels=yd if labels else None)
    assert type(logits.grad_fn.next_functions[0][0]).__name__ == "DeepFMFusedFnBackward"
    loss = pkg.BCEWithLogitsLoss()(logits, yd)
    loss.backward(unit_scalar(DEV))
    _lib.check_index_errors()
    return _grads(m, out=logits.detach(), loss=loss.detach())


def _build():
    """{case id: (form, deterministic, run)}; run() -> {name: tensor}, the same launches and values at every call."""
    cases = {}
    for form in FORMS:
        for name in mixed.ORDER:
            cases[f"train/{name}/{form}"] = (form, False, lambda n=name: _tail_step(n))
            cases[f"no-grad/{name}/{form}"] = (form, False, lambda n=name: _tail_step(n, grad=False))
        cases[f"x-without-grad/stats_then_fixed/{form}"] = (form, False, lambda: _tail_step("stats_then_fixed", x_grad=False))
        cases[f"labels/stats_then_fixed/{form}"] = (form, False, lambda: _tail_step("stats_then_fixed", labels=True))
        for labels in (False, True):
            cases[f"deepfm/{'labels' if labels else 'no-labels'}/{form}"] = (form, False, lambda y=labels: _deepfm_step(y))
    cases["deterministic/stats_then_fixed/sums"] = ("sums", True, lambda: _tail_step("stats_then_fixed"))
    for labels in (False, True):
        cases[f"slot-deepfm/{'labels' if labels else 'no-labels'}/sums"] = ("sums", False, ph._slot_deepfm_case(labels).run)
    return cases


CASES = _build()


def record(case_id):
    """(kernel names of the recorded call, its tensors, the warm-up call's tensors)."""
    form, deterministic, run = CASES[case_id]
    with _settings(form, deterministic):
        warm = run()
        with KernelTimer(64) as kt:
            res = run()
    return [name for name, _ in kt.records], res, warm


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as fh:
        return json.load(fh)


def test_every_case_is_pinned(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case_id", list(CASES))
def test_the_driver_launches_what_it_launched(case_id, golden):
    names, _, _ = record(case_id)
    assert 0 < len(names) < 64, "the recorder's capacity must hold the whole step"
    assert names == golden[case_id]

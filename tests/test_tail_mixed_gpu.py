"""GPU: the fused MLP tail on stacks whose hidden layers are NOT alike, and at the limits tail.fused_tail_plan admits.

The fused node is selected silently for any matching nn.Sequential, so a user who freezes one BatchNorm under
model.train(), leaves a Dropout in eval, puts a BatchNorm on some layers only or builds Linears without bias runs the
per-layer branches of tail._tail_forward / _tail_backward (which kernel joins the pending statistics, which one advances
the dropout seed, whether the masks ride in layer 0's finalize launch, dbias or the exact zero, the finalize launch
instead of the joined prologue when layer 0 wants no input gradient) that the uniform stacks of tests/test_tail_gpu.py
never reach.  Same rule as there: the fused result lies as close to the float64 evaluation of the reference's op sequence
(given the very masks the kernels use, tests/tail_helpers.py) as the stock float32 modules do, up to K_BRACKET = 8 — in the
three forms of the BatchNorm statistics, with the general path disabled and the plan asserted."""
import copy
import os

import pytest
import torch
from torch import nn

import oracle.reference_ops as ro
from conftest import EPS32, assert_close, assert_within_terms
from tail_helpers import (active_ps, bracket_or_flip, build_tail, hidden_layers, reference_walk, tail_masks,
                          zero_bias_names)
from test_tail_gpu import _fused_tail_on  # noqa: F401  (the fixture runs every test in the three forms of the statistics)

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import _lib
from recsys_benchmark_amd import mlp as _mlp
from recsys_benchmark_amd import tail as _tail_mod
from recsys_benchmark_amd.mlp import run_tail
from recsys_benchmark_amd.tail import fused_tail_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"

T, E = "train", "eval"
# id -> (M, K, layers (width, bn, drop[, bias]), head bias, BatchNorm momentum / eps or None)
CASES = {
    # pending statistics joined by a fixed layer's product; the masks ride in layer 0's finalize launch
    "stats_then_fixed": (67, 48, [(136, T, 0.5), (24, E, 0.5)], True, None),
    # plan[0].fixed: no ride, a mask launch of its own; the head joins the statistics and advances the seed
    "fixed_then_stats": (67, 48, [(24, E, 0.5), (136, T, 0.25)], True, None),
    # all three kinds in one stack; a layer without a Dropout module; p = 0
    "nobn_stats_frozen": (130, 16, [(200, None, 0.5), (104, T, 0.0), (40, E, None)], True, None),
    # bits[0] is None, bits[1] set
    "dropout_last_only": (67, 40, [(32, T, E), (32, T, 0.5)], True, None),
    # every absent-bias path, dbias skipped
    "no_biases": (200, 48, [(72, T, 0.3, False), (40, None, 0.3, False)], False, None),
    # the mask kernel's 8-layer limit
    "depth8": (67, 16, [(w, b, 0.25) for w, b in zip((8, 16, 24, 8, 40, 16, 8, 24), (T, E, None, T, E, None, T, T))], True, None),
    # 1024 columns, reduction 1024, constants at the limit, a head wider than 512
    "width1024": (67, 64, [(1024, T, 0.5), (1024, E, 0.0)], True, None),
    # smallest batch with batch statistics
    "two_rows": (2, 16, [(8, T, 0.5), (16, E, 0.5)], True, None),
    # M = 1, every layer fixed
    "one_row_fixed": (1, 16, [(8, E, None), (16, None, None)], True, None),
    # non-default BatchNorm hyper-parameters through the statistics structs
    "bn_hyper": (67, 48, [(136, T, 0.5), (24, T, 0.0)], True, (0.3, 1e-3)),
}
ORDER = list(CASES)
_REFS = {}       # the CPU side of a case (modules, inputs, float64 / float32 evaluation): made once, shared by the three forms


def _inputs(name):
    """(seq, x, add, G, dropout seed) of a case, from a seed of its own."""
    M, K, layers, head_bias, hyper = CASES[name]
    torch.manual_seed(1000 + ORDER.index(name))
    seq = build_tail(K, layers, head_bias, *(hyper or (None, None)))
    x = torch.randn(M, K) * 0.7 + 0.2
    add = torch.randn(M)
    G = torch.randn(M, 1) + 0.5
    return seq, x, add, G, 977 + M + 13 * ORDER.index(name)


def _references(key, seq, x, add, G, masks, grads=True, keep=False):
    """float64 and stock-float32 evaluations (with their backward) of one step; cached by key and never modified."""
    if key not in _REFS:
        near, kept = [], ([] if keep else None)
        ref64 = reference_walk(seq, x, add, masks, torch.float64, near_out=near, keep=kept)
        ref32 = reference_walk(seq, x, add, masks, torch.float32)
        if grads:
            for r in (ref64, ref32):
                (r[3] * G.to(r[3].dtype)).sum().backward()
        _REFS[key] = (near, ref64, ref32, kept)
    return _REFS[key]


def _fused_step(seq, x, add, G, seed_value=None, x_grad=True, module=None, labels=None, loss_seed=None, backward=True):
    """One step of the fused node on a device copy of `seq` (or on `module`, already there); the general path is off and the
    plan is asserted.  Returns (modules, x, add, out)."""
    dev = torch.device(DEV, 0)
    if seed_value is not None:
        _mlp._seed_word(dev).fill_(seed_value)
    fs = copy.deepcopy(seq).to(DEV) if module is None else module
    fs.zero_grad(set_to_none=True)
    xd = x.detach().clone().to(DEV).requires_grad_(x_grad)
    ad = add.detach().clone().to(DEV).requires_grad_(True)
    plan = fused_tail_plan(fs, xd, _mlp._groups(fs))
    assert plan is not None, "the fused node must take this pattern"
    assert [L.p for L in plan] == active_ps(seq) and [L.fixed for L in plan] == [bn is None or not bn.training
                                                                                 for _, _, bn, _ in hidden_layers(seq)[0]]
    out = run_tail(fs, xd, last_add=ad, labels=labels, loss_seed=loss_seed)
    assert type(out.grad_fn).__name__ == "FusedTailFnBackward" or not torch.is_grad_enabled()
    if backward:
        (out * G.to(DEV)).sum().backward()
    return fs, xd, ad, out


def _bookkeeping(seq, fs, seed_value, steps=1):
    """Integer state: num_batches_tracked went up on training-mode BatchNorms only, a frozen BatchNorm's running statistics
    are untouched, the seed word advanced once per step exactly when some layer drops."""
    for (at, _, bn, _), (_, _, fbn, _) in zip(hidden_layers(seq)[0], hidden_layers(fs)[0]):
        if bn is None:
            continue
        assert int(fbn.num_batches_tracked) == int(bn.num_batches_tracked) + (steps if bn.training else 0), f"{at + 1}.num_batches_tracked"
        if not bn.training:
            assert torch.equal(fbn.running_mean.cpu(), bn.running_mean) and torch.equal(fbn.running_var.cpu(), bn.running_var), \
                f"a frozen BatchNorm's running statistics moved (module {at + 1})"
    drops = any(p > 0 for p in active_ps(seq))
    assert int(_mlp._seed_word(torch.device(DEV, 0))) == seed_value + (steps if drops else 0)


@pytest.fixture(autouse=True)
def _no_general_path(monkeypatch):
    monkeypatch.setattr(_mlp, "_LinearFn", None)      # library products through PyTorch must not be what computes any of this


def _two_rows_dx_within_terms(name, seq, x, fused, ref64, kept, bad):
    """two_rows: dx is analytically near zero — with two samples the normalised value is +-s, s^2 = var / (var + eps), and
    dz = gamma rstd (dy - mean dy - zh mean(dy zh)) cancels down to eps rstd^2 of its terms — so its size is no scale for
    its error.  Held in absolute terms to 8 eps32 sum|terms| of that cancelling sum instead, carried through |W|."""
    assert name == "two_rows" and all(b.startswith("dx:") for b in bad), bad
    (_, lin, bn, _), = hidden_layers(ref64[0])[0][:1]
    z, pre = kept[0]
    dy = pre.grad
    rstd = (z.detach().var(0, unbiased=False) + bn.eps).rsqrt()
    zh = (z.detach() - z.detach().mean(0)) * rstd
    terms_dz = (bn.weight.detach() * rstd).abs() * (dy.abs() + dy.mean(0).abs() + zh.abs() * (dy * zh).mean(0).abs())
    terms = terms_dz @ lin.weight.detach().abs()
    err = (fused[1].grad.double().cpu() - ref64[1].grad).abs()
    ratio = float((err / (8 * EPS32 * terms + 1e-30)).max())
    if os.environ.get("MI_TEST_REPORT"):
        print(f"RATIO mixed/{name} dx against 8 eps32 sum|terms|: {ratio:.3f}")
    assert_within_terms(fused[1].grad, ref64[1].grad, terms, 8, "two_rows dx against the terms of its cancelling sum")


@pytest.mark.parametrize("name", ORDER)
def test_mixed_plans_bracket_float64(name):
    seq, x, add, G, seed_value = _inputs(name)
    masks = tail_masks(seq, seed_value, x.shape[0])
    near, ref64, ref32, kept = _references(("a", name), seq, x, add, G, masks, keep=True)
    fused = _fused_step(seq, x, add, G, seed_value)
    bad = bracket_or_flip(seq, fused, x, add, G, masks, near, ref64, ref32, tag=f"mixed/{name}")
    if bad and name == "two_rows" and all(b.startswith("dx:") for b in bad):
        _two_rows_dx_within_terms(name, seq, x, fused, ref64, kept, bad)
        bad = []
    assert not bad, f"{bad} (pre-activations within {1e-6:g} of the kink: {near})"
    _bookkeeping(seq, fused[0], seed_value)


@pytest.mark.parametrize("name", ["stats_then_fixed", "fixed_then_stats", "dropout_last_only"])
def test_seed_advances_once_per_step(name):
    """Two consecutive training steps on one module, the seed word left alone in between: the second step's masks are those
    of seed + 1 (no advance: the same masks again; two advances: masks the restated generator does not give)."""
    seq, x, add, G, seed_value = _inputs(name)
    M = x.shape[0]
    key = ("b", name)
    if key not in _REFS:
        first = [reference_walk(seq, x, add, tail_masks(seq, seed_value, M), dt) for dt in (torch.float64, torch.float32)]
        masks2 = tail_masks(seq, seed_value + 1, M)
        near = []
        # (the modules the first walk returns carry the running statistics after step 1; weights do not move: no optimizer)
        ref64 = reference_walk(first[0][0], x, add, masks2, torch.float64, near_out=near)
        ref32 = reference_walk(first[1][0], x, add, masks2, torch.float32)
        for r in (ref64, ref32):
            (r[3] * G.to(r[3].dtype)).sum().backward()
        _REFS[key] = (near, ref64, ref32, masks2, first[0][0])
    near, ref64, ref32, masks2, after_one = _REFS[key]
    fs, _, _, out1 = _fused_step(seq, x, add, G, seed_value)
    assert int(_mlp._seed_word(torch.device(DEV, 0))) == seed_value + 1
    fused = _fused_step(seq, x, add, G, None, module=fs)
    assert not torch.equal(fused[3], out1), "the second step dropped the same units as the first"
    bad = bracket_or_flip(after_one, fused, x, add, G, masks2, near, ref64, ref32, tag=f"two-steps/{name}")
    assert not bad, f"{bad} (near the kink: {near})"
    _bookkeeping(seq, fs, seed_value, steps=2)


@pytest.mark.parametrize("what", ["x-without-grad", "frozen-parameters", "no-grad"])
@pytest.mark.parametrize("name", ["stats_then_fixed", "fixed_then_stats"])
def test_what_does_not_want_a_gradient(name, what):
    """x.requires_grad False (layer 0 runs no input-gradient product: its column sums are joined by the finalize launch, not
    the product's prologue), frozen parameters (layer 0's weight, layer 1's BatchNorm weight), and torch.no_grad() with the
    per-layer flags left as they are (a training-mode BatchNorm still updates its running statistics, as the stock module does)."""
    seq, x, add, G, seed_value = _inputs(name)
    if what == "frozen-parameters":
        layers = hidden_layers(seq)[0]
        layers[0][1].weight.requires_grad_(False)
        layers[1][2].weight.requires_grad_(False)
    masks = tail_masks(seq, seed_value, x.shape[0])
    grads = what != "no-grad"
    near, ref64, ref32, _ = _references(("c", name, what == "frozen-parameters", grads), seq, x, add, G, masks, grads=grads)
    if grads:
        fused = _fused_step(seq, x, add, G, seed_value, x_grad=what != "x-without-grad")
    else:
        with torch.no_grad():
            fused = _fused_step(seq, x, add, G, seed_value, backward=False)
        assert not fused[3].requires_grad
    bad = bracket_or_flip(seq, fused, x, add, G, masks, near, ref64, ref32, tag=f"{what}/{name}", grads=grads)
    assert not bad, f"{bad} (near the kink: {near})"
    if what == "x-without-grad":
        assert fused[1].grad is None
    if what == "frozen-parameters":
        layers = hidden_layers(fused[0])[0]
        assert layers[0][1].weight.grad is None and layers[1][2].weight.grad is None
        assert layers[0][1].bias.grad is not None and layers[1][2].bias.grad is not None
    _bookkeeping(seq, fused[0], seed_value)


@pytest.mark.parametrize("seed_scale", [None, 0.25])
@pytest.mark.parametrize("name", ["stats_then_fixed", "fixed_then_stats", "width1024"])
def test_criterion_in_the_head_launch_on_mixed_plans(name, seed_scale):
    """run_tail(..., labels=y[, loss_seed=s]) on mixed plans: against the same step with the labels withheld (the tolerances
    of test_head_launch_with_the_criterion_and_a_named_upstream_seed), the loss also against float64 BCE.  A head wider than
    512 columns keeps the criterion as its own launch — silently — and the numbers agree all the same."""
    from recsys_benchmark_amd.losses import BCEWithLogitsLoss, unit_scalar

    seq, x, add, G, seed_value = _inputs(name)
    M = x.shape[0]
    y = (torch.rand(M, generator=torch.Generator().manual_seed(M)) < 0.4).float()
    dev = torch.device(DEV, 0)
    up = unit_scalar(dev) if seed_scale is None else torch.full((), seed_scale, device=dev)
    res = {}
    for with_labels in (True, False):
        fs = copy.deepcopy(seq).to(DEV)
        xd, ad, yd = x.to(DEV).requires_grad_(True), add.to(DEV).requires_grad_(True), y.to(DEV)
        _mlp._seed_word(dev).fill_(seed_value)
        assert fused_tail_plan(fs, xd, _mlp._groups(fs)) is not None
        out = run_tail(fs, xd, last_add=ad, labels=yd if with_labels else None,
                       loss_seed=up if (with_labels and seed_scale is not None) else None)
        loss = BCEWithLogitsLoss()(out.squeeze(-1), yd)
        in_head = with_labels and _tail_mod.STAT_SUMS and not _tail_mod.MERGE_JOINS and name != "width1024"
        assert (type(loss.grad_fn).__name__ == "_HeadBCEFnBackward") == in_head
        assert not _tail_mod._HEAD_LOSS, "a head loss left registered behind the criterion"
        loss.backward(up)
        res[with_labels] = (out.detach(), loss.detach(), xd.grad, ad.grad, [q.grad for q in fs.parameters()])
        assert int(_mlp._seed_word(dev)) == seed_value + 1
    a, b = res[True], res[False]
    assert_close(a[0], b[0], 1e-5, 1e-6, "logits")
    assert_close(a[1], b[1], 1e-5, 1e-6, "loss")
    assert_close(a[2], b[2], 2e-4, 1e-7, "dx")
    assert_close(a[3], b[3], 1e-5, 1e-9, "d last_add")
    for u, v, (pname, _) in zip(a[4], b[4], seq.named_parameters()):
        assert_close(u, v, 2e-4, 1e-6 + 2e-8 * M, pname)
    # the loss against float64: as close as stock float32 BCE on the stock float32 logits is, up to the bracket's factor
    masks = tail_masks(seq, seed_value, M)
    near, ref64, ref32, _ = _references(("d", name), seq, x, add, G, masks, grads=False)
    l64 = nn.functional.binary_cross_entropy_with_logits(ref64[3].detach().squeeze(-1), y.double())
    l32 = nn.functional.binary_cross_entropy_with_logits(ref32[3].detach().squeeze(-1), y)
    err_f, err_s = abs(float(a[1]) - float(l64)) / float(l64), abs(float(l32) - float(l64)) / float(l64)
    if os.environ.get("MI_TEST_REPORT"):
        print(f"RATIO criterion/{name} loss: fused {err_f:.3e} stock {err_s:.3e} ratio {err_f / max(err_s, 1e-30):.2f}")
    if not err_f <= max(8.0 * err_s, 1e-6) and near:      # a unit on the kink moves its row's logit, hence the loss
        err_f = min(abs(float(a[1]) - float(nn.functional.binary_cross_entropy_with_logits(
            reference_walk(seq, x, add, masks, torch.float64, flips={"list": near, "which": {j for j in range(len(near)) if bits >> j & 1}})[3]
            .detach().squeeze(-1), y.double()))) / float(l64) for bits in range(1, 1 << len(near)))
    assert err_f <= max(8.0 * err_s, 1e-6), f"loss: fused {err_f:.3e} vs stock {err_s:.3e} from float64"


def test_backward_runs_the_form_its_forward_ran(monkeypatch):
    """The replica counts are lowered between forward and backward (HEAD_REPS 8 -> 2, STAT_REPS 4 -> 1; never raised: every
    extent stays inside what the forward allocated).  With labels the head launch has already written the head's sums into 8
    replica rows; a backward that read the knobs again would join 2 of them.  Held like the labels case above: against the
    same step with the labels withheld and the knobs left alone, at its tolerances."""
    from recsys_benchmark_amd.losses import BCEWithLogitsLoss, unit_scalar

    seq, x, add, G, seed_value = _inputs("stats_then_fixed")
    M = x.shape[0]
    y = (torch.rand(M, generator=torch.Generator().manual_seed(M)) < 0.4).float()
    dev = torch.device(DEV, 0)
    res = {}
    for with_labels in (False, True):
        monkeypatch.setattr(_tail_mod, "HEAD_REPS", 8)
        monkeypatch.setattr(_tail_mod, "STAT_REPS", 4)
        fs = copy.deepcopy(seq).to(DEV)
        xd, ad, yd = x.to(DEV).requires_grad_(True), add.to(DEV).requires_grad_(True), y.to(DEV)
        _mlp._seed_word(dev).fill_(seed_value)
        out = run_tail(fs, xd, last_add=ad, labels=yd if with_labels else None)
        loss = BCEWithLogitsLoss()(out.squeeze(-1), yd)
        if with_labels:
            monkeypatch.setattr(_tail_mod, "HEAD_REPS", 2)
            monkeypatch.setattr(_tail_mod, "STAT_REPS", 1)
        loss.backward(unit_scalar(dev))
        res[with_labels] = (out.detach(), loss.detach(), xd.grad, ad.grad, [q.grad for q in fs.parameters()])
    a, b = res[True], res[False]
    assert_close(a[0], b[0], 1e-5, 1e-6, "logits")
    assert_close(a[1], b[1], 1e-5, 1e-6, "loss")
    assert_close(a[2], b[2], 2e-4, 1e-7, "dx")
    assert_close(a[3], b[3], 1e-5, 1e-9, "d last_add")
    for u, v, (pname, _) in zip(a[4], b[4], seq.named_parameters()):
        assert_close(u, v, 2e-4, 1e-6 + 2e-8 * M, pname)


def test_ill_conditioned_statistics():
    """Pre-activation columns up to ~150 sigma from zero under running means far from the batch means (a checkpoint loaded
    onto new data): the shifted sums (s_c = running_mean - bias, M2 = t2 - t1^2 / M) and the tile merges must hold the same
    bracket, running statistics included."""
    M, K = 130, 48
    torch.manual_seed(2000)
    seq = build_tail(K, [(104, T, 0.5), (24, T, 0.0)], True, 0.3, 1e-3)
    for m in seq:
        if isinstance(m, nn.BatchNorm1d):
            m.running_mean.fill_(-50.0)
    x = torch.randn(M, K) * 0.05 + 3.0
    add = torch.randn(M)
    G = torch.randn(M, 1) + 0.5
    seed_value = 977 + M
    masks = tail_masks(seq, seed_value, M)
    near, ref64, ref32, _ = _references(("e",), seq, x, add, G, masks)
    fused = _fused_step(seq, x, add, G, seed_value)
    bad = bracket_or_flip(seq, fused, x, add, G, masks, near, ref64, ref32, tag="ill-conditioned")
    assert not bad, f"{bad} (near the kink: {near})"
    _bookkeeping(seq, fused[0], seed_value)


@pytest.mark.parametrize("variant", ["first-bn-frozen", "second-bn-frozen-first-dropout-eval"])
def test_deepfm_fused_step_on_mixed_plans(variant):
    """DeepFM's one-node step (run_fused_deepfm): the lookup launch carries the mask job AND the fixed layers' constants.
    Against deepfm_embed_fm + the float64 walk over `_deep_branch` with the restated masks + BCE, at the tolerances of
    test_deepfm_step_with_the_fm_epilogue_on_the_exact_cover."""
    dims, D, hidden, B = [11, 7, 5], 16, [136, 24], 67
    torch.manual_seed(3000 + len(variant))
    base = pkg.DeepFM(dims, D, hidden, p_dropout=0.5, use_batchnorm=True, embedding_config={"name": "vanilla", "sparse": True},
                      fc_sparse=True).train()
    with torch.no_grad():
        base._bias.fill_(0.3)
        for m in base._deep_branch:
            if isinstance(m, nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    layers = hidden_layers(base._deep_branch)[0]
    if variant == "first-bn-frozen":
        layers[0][2].eval()
    else:
        layers[1][2].eval()
        layers[0][3].eval()
    gen = torch.Generator().manual_seed(B * 7 + D)
    x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1)
    y = (torch.rand(B, generator=gen) < 0.3).float()
    seed_value = 4321
    # the float64 side: lookup + FM from the oracle, then the walk over a copy of the deep branch
    p = {k: v.detach().clone().double() if v.is_floating_point() else v.detach().clone() for k, v in base.state_dict().items()}
    for k in ("embedding._emb_module.weight", "fc.weight", "_bias"):
        p[k].requires_grad_(True)
    emb, y_fm = ro.deepfm_embed_fm(x, p)
    masks = tail_masks(base._deep_branch, seed_value, B)
    near = []
    ref = reference_walk(base._deep_branch, emb.reshape(B, -1), y_fm, masks, torch.float64, near_out=near, as_is=True)
    assert not near, f"a pre-activation on the kink ({near}): take another seed for this test's inputs"
    nn.functional.binary_cross_entropy_with_logits(ref[3].squeeze(-1), y.double()).backward()
    want = {"embedding._emb_module.weight": p["embedding._emb_module.weight"].grad, "fc.weight": p["fc.weight"].grad,
            "_bias": p["_bias"].grad}
    want.update({"_deep_branch." + k: v.grad for k, v in ref[0].named_parameters()})
    # (the yardstick of the printed ratios: the same evaluation in stock float32)
    p32 = {k: v.detach().float().requires_grad_(v.requires_grad) if v.is_floating_point() else v for k, v in p.items()}
    emb32, y_fm32 = ro.deepfm_embed_fm(x, p32)
    ref32 = reference_walk(base._deep_branch, emb32.reshape(B, -1), y_fm32, masks, torch.float32, as_is=True)
    nn.functional.binary_cross_entropy_with_logits(ref32[3].squeeze(-1), y).backward()

    dev = torch.device(DEV, 0)
    m = copy.deepcopy(base).to(DEV)
    W = m.embedding.get_weight()
    assert fused_tail_plan(m._deep_branch, _tail_mod._InputSpec(B, len(dims) * D, W.device), _mlp._groups(m._deep_branch)) is not None
    before = {k: v.detach().clone() for k, v in m.named_buffers()}
    _mlp._seed_word(dev).fill_(seed_value)
    logits = m(x.to(DEV))
    assert type(logits.grad_fn.next_functions[0][0]).__name__ == "DeepFMFusedFnBackward"
    nn.BCEWithLogitsLoss()(logits, y.to(DEV)).backward()
    _lib.check_index_errors()
    assert int(_mlp._seed_word(dev)) == seed_value + 1
    assert_close(logits, ref[3].detach().squeeze(-1).float(), 1e-4, 1e-5, "logits")
    if os.environ.get("MI_TEST_REPORT"):
        for what, got, r64, r32 in (("logits", logits, ref[3], ref32[3]),
                                    ("table gradient", m.embedding.get_weight().grad.to_dense(), want["embedding._emb_module.weight"],
                                     p32["embedding._emb_module.weight"].grad)):
            r64 = r64.detach().double().reshape(-1)
            scale = float(r64.abs().max())
            e_f = float((got.detach().double().cpu().reshape(-1) - r64).abs().max()) / scale
            e_s = float((r32.detach().double().reshape(-1) - r64).abs().max()) / scale
            print(f"RATIO deepfm/{variant} {what}: fused {e_f:.3e} stock {e_s:.3e} ratio {e_f / max(e_s, 1e-30):.2f}")
    atol = 1e-5 + 2e-7 * B
    zero = {"_deep_branch." + n for n in zero_bias_names(base._deep_branch)}
    for k, q in m.named_parameters():
        if k.startswith("linear_layer"):      # (not part of the forward)
            continue
        g = q.grad.to_dense() if q.grad.is_sparse else q.grad
        if k in zero:
            assert float(g.abs().max()) == 0.0, k
            continue
        assert_close(g, want[k].float().view_as(g), 2e-4, atol, f"grad {k}")
    after, b64 = dict(m.named_buffers()), dict(ref[0].named_buffers())
    for (at, _, bn, _) in layers:
        for stat in ("running_mean", "running_var", "num_batches_tracked"):
            k = f"_deep_branch.{at + 1}.{stat}"
            if not bn.training:
                assert torch.equal(after[k], before[k]), f"{k}: a frozen BatchNorm's buffer moved"
            elif stat == "num_batches_tracked":
                assert int(after[k]) == int(before[k]) + 1
            else:
                assert_close(after[k], b64[f"{at + 1}.{stat}"].float(), 1e-4, 1e-5, k)

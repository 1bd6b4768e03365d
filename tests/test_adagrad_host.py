"""CPU: the float64 Adagrad references of tests/adagrad_helpers.py against torch.optim.Adagrad in float64, the measurement
that sets the helper's constants, the wrong variants the bounds must reject, the optimizer factory and the header."""
import os
import re

import pytest
import torch

import adagrad_helpers as ah
import optim_helpers as oh

from recsys_benchmark_amd import optim as rbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-2
EPS = {"sparse": 1e-10, "dense": 1e-10, "rowwise": 1e-8}
N_ROWS, N_ENTRIES, STEPS = 60, 200, 5
WIDTHS = (1, 4, 8, 16)


# ---- the references are torch's rule ---------------------------------------------------------------------------------------
def _rel(a, b):
    scale = torch.maximum(a.abs(), b.abs())
    return float(((a - b).abs() / torch.where(scale == 0, torch.ones_like(scale), scale)).max())


def test_ref64_is_torch_adagrad_sparse_with_duplicates_decay_and_initial_value():
    N, D, n, lr_decay, init = 40, 4, 150, 0.01, 0.1
    gen = torch.Generator().manual_seed(1)
    p0 = torch.randn(N, D, generator=gen, dtype=torch.float64)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adagrad([p], lr=LR, lr_decay=lr_decay, eps=1e-10, initial_accumulator_value=init)
    steps, sums = [], []
    for _ in range(4):
        ids = ah.skewed_ids(N, n, gen)
        vals = ah.scaled_ints((n, D), gen).double()
        assert ids.unique().numel() < n
        p.grad = torch.sparse_coo_tensor(ids.view(1, -1), vals, (N, D))
        opt.step()
        steps.append((*ah.coalesced(ids, vals, N), p.detach().clone()))
        sums.append(opt.state[p]["sum"].clone())
    worst = 0.0
    for rec, s in zip(ah.adagrad_ref64("sparse", p0, steps, LR, 1e-10, lr_decay, init), sums):
        worst = max(worst, _rel(rec["p_before"] + rec["u"], rec["p_after"]), _rel(rec["s"], s))
    print(f"sparse float64 reference vs torch.optim.Adagrad(float64): worst relative difference {worst:.3e}")
    assert worst <= 1e-15


def test_ref64_is_torch_adagrad_dense_with_weight_decay():
    gen = torch.Generator().manual_seed(2)
    p0 = oh.dense_params((50, 8), gen).double()
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adagrad([p], lr=LR, eps=1e-10, weight_decay=1e-2)
    steps, sums = [], []
    for _ in range(4):
        g = ah.scaled_ints((50, 8), gen).double()
        p.grad = g.clone()
        opt.step()
        steps.append((g, None, p.detach().clone()))
        sums.append(opt.state[p]["sum"].clone())
    worst = 0.0
    for rec, s in zip(ah.adagrad_ref64("dense", p0, steps, LR, 1e-10, wd=1e-2), sums):
        worst = max(worst, _rel(rec["p_before"] + rec["u"], rec["p_after"]), _rel(rec["s"], s))
    print(f"dense float64 reference vs torch.optim.Adagrad(float64): worst relative difference {worst:.3e}")
    assert worst <= 1e-15


# ---- the fp32 yardsticks and the wrong variants --------------------------------------------------------------------------
def _inputs(kind, D, init=0.0, wd=0.0):
    """(p0, grads) for one run: `grads` as adagrad_fp32 takes them."""
    gen = torch.Generator().manual_seed(100 * D + int(init * 10) + int(wd * 1000) + ah.KINDS.index(kind))
    if kind == "dense":
        return oh.dense_params((N_ROWS, D), gen), [ah.scaled_ints((N_ROWS, D), gen) for _ in range(STEPS)]
    p0, grads = torch.randn(N_ROWS, D, generator=gen), []
    for _ in range(STEPS):
        ids = ah.skewed_ids(N_ROWS, N_ENTRIES, gen)
        grads.append((ids, ah.row_scaled_ints(ids, D, gen) if kind == "rowwise" else ah.scaled_ints((N_ENTRIES, D), gen)))
    return p0, grads


def _steps_of(kind, grads, results):
    if kind == "dense":
        return [(g, None, p) for g, (p, _) in zip(grads, results)]
    return [(*ah.coalesced(ids, vals, N_ROWS), p) for (ids, vals), (p, _) in zip(grads, results)]


def _torch_fp32(kind, p0, grads, init, wd):
    """torch.optim.Adagrad itself, CPU, fp32: [(p_after, sum)] per step."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adagrad([p], lr=LR, eps=EPS[kind], initial_accumulator_value=init, weight_decay=wd)
    out = []
    for grad in grads:
        if kind == "dense":
            p.grad = grad.clone()
        else:
            p.grad = torch.sparse_coo_tensor(grad[0].view(1, -1), grad[1], tuple(p0.shape))
        opt.step()
        out.append((p.detach().clone(), opt.state[p]["sum"].clone()))
    return out


def _yardstick(kind, D, init=0.0, wd=0.0, unit=False):
    p0, grads = _inputs(kind, D, init, wd)
    if kind == "rowwise":
        res = ah.adagrad_fp32(kind, p0, grads, LR, EPS[kind])
    else:
        res = _torch_fp32(kind, p0, grads, init, wd)
    return ah.worst_ratios(kind, p0, _steps_of(kind, grads, res), [s for _, s in res], LR, EPS[kind], init=init, wd=wd, unit=unit)


CASES = {"sparse": [(0.0, 0.0), (0.1, 0.0)], "dense": [(0.0, 0.0), (0.0, 1e-2), (0.1, 0.0), (0.1, 1e-2)],
         "rowwise": [(0.0, 0.0)]}


def test_constants_are_twice_the_measured_worst_ratio():
    """The measurement of the helper's docstring: every constant at 1, torch's fp32 CPU Adagrad (and the index-order fp32
    restatement of the row-wise rule) against the float64 references."""
    worst = {}
    for kind in ah.KINDS:
        per = {}
        for D in WIDTHS + (7, 12):
            for init, wd in CASES[kind]:
                ah.fold(per, _yardstick(kind, D, init, wd, unit=True))
        print(f"{kind}: worst ratio with the constants at 1: step {per['step']:.2f} sum {per['sum']:.2f}")
        ah.fold(worst, per)
    print(f"chosen: C_STEP = {ah.C_STEP}, C_SUM = {ah.C_SUM}")
    assert ah.C_STEP == max(1, -int(-2 * worst["step"] // 1)) and ah.C_SUM == max(1, -int(-2 * worst["sum"] // 1))


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("kind", ah.KINDS)
def test_right_rule_is_inside_the_bounds(kind, D):
    worst = {}
    for init, wd in CASES[kind]:
        ah.fold(worst, _yardstick(kind, D, init, wd))
        p0, grads = _inputs(kind, D, init, wd)                  # (and the helper's own fp32 statement of the rule)
        res = ah.adagrad_fp32(kind, p0, grads, LR, EPS[kind], init=init, wd=wd)
        ah.fold(worst, ah.worst_ratios(kind, p0, _steps_of(kind, grads, res), [s for _, s in res], LR, EPS[kind], init=init,
                                       wd=wd))
    print(f"{kind} D={D}: worst ratio to the bounds step={worst['step']:.3f} sum={worst['sum']:.3f}")
    assert worst["step"] <= 1.0 and worst["sum"] <= 1.0


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("kind", ah.KINDS)
def test_wrong_variants_are_outside_the_bounds(kind, D):
    p0, grads = _inputs(kind, D)
    for variant in ah.variants_of(kind, D):
        res = ah.adagrad_fp32(kind, p0, grads, LR, EPS[kind], variant=variant)
        worst = ah.worst_ratios(kind, p0, _steps_of(kind, grads, res), [s for _, s in res], LR, EPS[kind])
        print(f"{kind} D={D} {variant}: step={worst['step']:.3g} sum={worst['sum']:.3g}")
        assert max(worst.values()) > 1.0 or any(r != r for r in worst.values()), f"{variant} passes the bounds"
        if variant in ("eps_in_root", "stale_sum"):      # these leave the accumulator right: the STEP bound has to catch them
            assert worst["step"] > 1.0


# ---- the factory ---------------------------------------------------------------------------------------------------------------
def _model(sparse):
    import recsys_benchmark_amd as pkg

    torch.manual_seed(0)
    return pkg.DeepFM([7, 5, 11], 4, [8, 8], p_dropout=0.0, use_batchnorm=False,
                      embedding_config={"name": "vanilla", "sparse": sparse}, fc_sparse=sparse)


def _classes(name, sparse):
    cfg = {"optimizer": name, "sparse": sparse, "learning_rate": 1e-2, "weight_decay": 1e-6}
    return [type(o) for o in rbo.get_optimizers(_model(sparse), cfg)]


def test_get_optimizers_adagrad_pairs():
    # (a CPU model: the dense group takes torch's own class there, the GPU one is checked in test_adagrad_optim_gpu.py)
    assert _classes("adagrad", True) == [rbo.SparseAdagrad, torch.optim.Adagrad]
    assert _classes("adagrad", False) == [torch.optim.Adagrad]
    assert _classes("rowwise_adagrad", True) == [rbo.RowwiseAdagrad, torch.optim.Adagrad]
    with pytest.raises(ValueError, match="row-form"):
        _classes("rowwise_adagrad", False)
    with pytest.raises(ValueError, match="not recognized"):
        _classes("rmsprop", True)
    with pytest.raises(ValueError, match="not recognized"):
        _classes("rmsprop", False)
    assert issubclass(rbo.Adagrad, torch.optim.Adagrad)


def test_get_optimizers_adam_and_sgd_are_unchanged():
    assert _classes("adam", True) == [rbo.SparseAdam, torch.optim.Adam]
    assert _classes("adam", False) == [torch.optim.Adam]
    assert _classes("sgd", True) == [rbo.SparseSGD, torch.optim.SGD]
    assert _classes("sgd", False) == [torch.optim.SGD]


def test_sparse_adagrad_groups_and_state_follow_torch():
    p = torch.nn.Parameter(torch.zeros(5, 4))
    a, t = rbo.SparseAdagrad([p], lr=0.1, initial_accumulator_value=0.5), torch.optim.Adagrad([p], lr=0.1)
    assert set(t.param_groups[0]) <= set(a.param_groups[0])
    assert a.param_groups[0]["capturable"] is True
    assert rbo.SparseAdagrad([p], lr_decay=0.01).param_groups[0]["capturable"] is False
    assert rbo.RowwiseAdagrad([p]).param_groups[0]["capturable"] is True
    assert set(a.state[p]) == set(t.state[p]) == {"step", "sum"}
    assert a.state[p]["sum"].shape == p.shape and bool((a.state[p]["sum"] == 0.5).all())
    t.load_state_dict(a.state_dict())
    assert bool((t.state[p]["sum"] == 0.5).all())
    for cls in (rbo.SparseAdagrad, rbo.RowwiseAdagrad):
        with pytest.raises(ValueError):
            cls([p], lr=-1.0)


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mi355x_recsys.h")).read()
    for name in ("mi_sparse_adagrad_sorted_ld", "mi_rowwise_adagrad_sorted_ld", "mi_adagrad_dense_multi"):
        assert re.search(r"MI_API\s+int\s+" + name + r"\s*\(", text), f"{name} is not declared in the header"
    assert "sqrtf(s) + eps" in text and "xor tree" in text          # (the rules and the order of the row sum are spelled out)

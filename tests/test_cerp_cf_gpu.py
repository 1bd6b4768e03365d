"""GPU: CERP on the CF models.
A  the two-table family in table form (mi_dual_table_*): forward bit-equal to the lookup over arange(N); backward exact on
   integer inputs, within the derived float32 summation bound on random ones, bit-equal run to run, every element written;
B  the batch-row regulariser / prune loss (mi_reg_prune_rows_*) against the reference's recorded values and a float64
   restatement;
C  the LightGCN / SingleLightGCN CERP step and epoch and the NeuMF PEP / CERP epochs against one recorded reference step."""
import copy
import math
import os

import pytest
import torch

from cerp_cf_helpers import (dual_table_bwd_ref64, dual_table_ref64, keep_margin, reg_prune_ref64)
from conftest import EPS32, assert_close, load_golden

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import _kernels, _lib, losses, trainer
from recsys_benchmark_amd.embeddings import get_embedding
from recsys_benchmark_amd.graph_utils import calculate_sparse_graph_adj_norm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL = dict(rtol=1e-5, atol=1e-6)          # tests/test_neumf_gpu.py: losses
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)          # tests/test_neumf_gpu.py: gradients

SIZES = [(37, 8, 12), (5000, 16, 1700), (38048, 64, 5500)]        # N, D, CERP bucket
FAMILY = [("qr", "mult", 2), ("qr", "add", 2), ("qr", "cat", 2), ("qr", "mult", 5), ("qr", "add", 5), ("qr", "cat", 5),
          ("soft", "add", None), ("mask", "add", None)]


def family_case(kind, op, divider, N, D, bucket, gen, integers=False):
    """kwargs of _kernels.dual_table / dual_gather for one member of the family (CPU tensors)."""
    if kind == "qr":
        mod1 = div2 = divider
        n1, n2 = divider, (N - 1) // divider + 1
    else:
        mod1, div2 = bucket, math.ceil(N / bucket)
        n1 = n2 = bucket

    def table(n):
        if integers:
            return torch.randint(-3, 4, (n, D), generator=gen).float()
        return torch.randn(n, D, generator=gen) * 0.3

    kw = dict(T1=table(n1), T2=table(n2), mod1=mod1, div2=div2, op=op)
    if kind == "soft":
        kw["S1"], kw["S2"] = torch.randn(n1, D, generator=gen) - 2, torch.randn(n2, D, generator=gen) - 2
        kw["T1"], kw["T2"] = keep_margin(kw["T1"], kw["S1"]), keep_margin(kw["T2"], kw["S2"])
    elif kind == "mask":
        kw["M1"], kw["M2"] = torch.rand(n1, D, generator=gen) < 0.6, torch.rand(n2, D, generator=gen) < 0.6
    return kw


def on_dev(kw, grad=False):
    out = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    if grad:
        for k in ("T1", "T2", "S1", "S2"):
            if k in out:
                out[k] = out[k].clone().requires_grad_(True)
    return out


def table_of(kw, N):
    kw = dict(kw)
    return _kernels.dual_table(kw.pop("T1"), kw.pop("T2"), N, kw.pop("mod1"), kw.pop("div2"), **kw)


# ------------------------------------------------------------------------------------------------------------ A forward
@pytest.mark.parametrize("N,D,bucket", SIZES)
@pytest.mark.parametrize("kind,op,divider", FAMILY)
def test_table_forward_is_bit_equal_to_the_lookup_over_arange(kind, op, divider, N, D, bucket):
    kw = on_dev(family_case(kind, op, divider, N, D, bucket, torch.Generator().manual_seed(N + D)))
    assert _kernels.dual_table_supported(N, kw["mod1"], kw["div2"], kw["T1"], kw["T2"], kw.get("S1"), kw.get("S2"))
    got = table_of(kw, N)
    kw2 = dict(kw)
    want = _kernels.dual_gather(torch.arange(N, device=DEV), kw2.pop("T1"), kw2.pop("T2"), **kw2)
    assert got.shape == want.shape == (N, 2 * D if op == "cat" else D)
    assert torch.equal(got, want)
    assert_close(got, dual_table_ref64(N=N, **kw).float(), 1e-5, 1e-6, "float64 restatement")
    pkg.check_index_errors()


def test_get_weight_takes_the_table_form_and_an_unsupported_width_keeps_the_lookup(tmp_path):
    torch.manual_seed(0)
    N = 101
    for cfg, D in (({"name": "qr", "divider": 5, "operation": "mult"}, 16), ({"name": "qr", "divider": 2, "operation": "cat"}, 16),
                   ({"name": "cerp", "bucket_size": 30}, 8), ({"name": "qr", "divider": 5, "operation": "add"}, 7)):
        emb = get_embedding(cfg, N, D).to(DEV)
        if cfg["name"] == "cerp":
            with torch.no_grad():
                emb.p_threshold.copy_(torch.randn(30, D) - 2)
                emb.q_threshold.copy_(torch.randn(30, D) - 2)
        w = emb.get_weight()
        assert w.shape == (N, D)
        assert torch.equal(w, emb(torch.arange(N, device=DEV)))
        assert w.grad_fn is not None
        took = type(w.grad_fn).__name__.startswith("DualTable")
        assert took == (D % 4 == 0), (cfg, type(w.grad_fn).__name__)
    pkg.check_index_errors()


def test_tables_that_cannot_cover_the_rows_are_refused():
    T1, T2 = torch.zeros(4, 8, device=DEV), torch.zeros(5, 8, device=DEV)
    assert not _kernels.dual_table_supported(37, 5, 4, T1, T2)            # n1 < mod1
    assert not _kernels.dual_table_supported(37, 4, 4, T1, T2)            # n2 < ceil(37 / 4)
    out = torch.empty(37, 8, device=DEV)
    rc = _lib.load().mi_dual_table_fwd(T1.data_ptr(), T2.data_ptr(), None, None, None, None, out.data_ptr(), 37, 8, 4, 5, 4, 4, 1,
                                       0, _lib.stream_ptr(torch.device(DEV)))
    assert rc == -1                                                       # MI_ERR_INVALID_ARG
    rc = _lib.load().mi_dual_table_fwd(T1.data_ptr(), T2.data_ptr(), None, None, None, None, out.data_ptr(), 16, 7, 4, 5, 4, 4, 1,
                                       0, _lib.stream_ptr(torch.device(DEV)))
    assert rc == -2                                                       # MI_ERR_UNSUPPORTED: the width


# ----------------------------------------------------------------------------------------------------------- A backward
def run_backward(kw, N, g):
    kwd = on_dev(kw, grad=True)
    out = table_of(kwd, N)
    out.backward(g.to(DEV))
    return {"gT1": kwd["T1"].grad, "gT2": kwd["T2"].grad, "gS1": kwd["S1"].grad if "S1" in kwd else None,
            "gS2": kwd["S2"].grad if "S2" in kwd else None}


EXACT = [("qr", op, d) for op in ("mult", "add", "cat") for d in (2, 5)] + [("mask", op, None) for op in ("mult", "add", "cat")]


@pytest.mark.parametrize("N,D,bucket", SIZES)
@pytest.mark.parametrize("kind,op,divider", EXACT)
def test_table_backward_is_exact_on_integer_inputs(kind, op, divider, N, D, bucket):
    """g, tables in -3..3 and 0/1 masks: every product and partial sum is an integer below 2^24 (at most 19 024
    contributors of magnitude <= 9), float32 arithmetic is exact in any order, so the result must EQUAL the float64
    restatement: a lost, doubled or misplaced contributor cannot hide."""
    gen = torch.Generator().manual_seed(7 * N + D)
    kw = family_case(kind, op, divider, N, D, bucket, gen, integers=True)
    g = torch.randint(-3, 4, (N, 2 * D if op == "cat" else D), generator=gen).float()
    got = run_backward(kw, N, g)
    ref = dual_table_bwd_ref64(g, N=N, **kw)
    assert float(ref["abs_T1"].max()) < 2 ** 24
    for key in ("gT1", "gT2"):
        assert torch.equal(got[key].cpu(), ref[key].float()), f"{kind} {op} {divider} N={N}: {key}"


RANDOM = [("qr", op, d) for op in ("mult", "add", "cat") for d in (2, 5)] + \
         [("soft", "add", None), ("soft", "cat", None), ("mask", "add", None), ("mask", "mult", None)]


@pytest.mark.parametrize("N,D,bucket", SIZES)
@pytest.mark.parametrize("kind,op,divider", RANDOM)
def test_table_backward_within_the_ordered_sum_bound_and_bit_equal_run_to_run(kind, op, divider, N, D, bucket):
    """An ordered float32 sum of n terms is within n * 2^-24 * sum|terms| of the exact sum: elementwise
    |got - ref64| <= (n + 4) * 2^-24 * sum|terms|, n the row's contributor count (the 4 covers the product and the
    derivative factor).  (The soft threshold under `mult` is left to the next test: there the OTHER table's transformed
    value |w| - sigmoid(s) enters each term, and its float32 cancellation error is not a summation error.)"""
    gen = torch.Generator().manual_seed(11 * N + D)
    kw = family_case(kind, op, divider, N, D, bucket, gen)
    g = torch.randn(N, 2 * D if op == "cat" else D, generator=gen)
    got = run_backward(kw, N, g)
    again = run_backward(kw, N, g)
    ref = dual_table_bwd_ref64(g, N=N, **kw)
    for key, n in (("gT1", ref["n1"]), ("gT2", ref["n2"]), ("gS1", ref["n1"]), ("gS2", ref["n2"])):
        if got[key] is None:
            assert key.startswith("gS") and kind != "soft"
            continue
        assert torch.equal(got[key], again[key]), f"{key}: two runs differ"
        bound = (n.double().unsqueeze(1) + 4) * EPS32 * ref["abs_" + key[1:]] + 1e-30
        err = (got[key].cpu().double() - ref[key]).abs()
        worst = float((err / bound).max())
        print(f"{kind} {op} {divider} N={N} {key}: worst error / bound = {worst:.3g} (max contributors {int(n.max())})")
        assert bool((err <= bound).all()), f"{key}: {worst:.3g} x the bound"


def test_soft_threshold_under_mult_matches_the_lookup_backward():
    N, D, bucket = 5000, 16, 1700
    gen = torch.Generator().manual_seed(5)
    kw = family_case("soft", "mult", None, N, D, bucket, gen)
    g = torch.randn(N, D, generator=gen)
    got = run_backward(kw, N, g)
    kwd = on_dev(kw, grad=True)
    kw2 = dict(kwd)
    _kernels.dual_gather(torch.arange(N, device=DEV), kw2.pop("T1"), kw2.pop("T2"), **kw2).backward(g.to(DEV))
    for key, name in (("gT1", "T1"), ("gT2", "T2"), ("gS1", "S1"), ("gS2", "S2")):
        assert_close(got[key], kwd[name].grad, **GRAD_TOL, what=key)


@pytest.mark.parametrize("kind,op,divider,N,D,bucket", [("qr", "mult", 2, 38048, 64, None), ("qr", "cat", 5, 5000, 16, None),
                                                          ("soft", "add", None, 38048, 64, 5500), ("mask", "add", None, 37, 8, 12),
                                                          ("qr", "add", 8, 37, 8, None)])
def test_table_backward_writes_every_gradient_element(kind, op, divider, N, D, bucket):
    """Gradient tensors handed in full of NaN come back finite everywhere — rows without a contributor included (the
    CERP case at N = 37 has bucket rows that no id reaches in the quotient table; QR divider 8 a short last row)."""
    gen = torch.Generator().manual_seed(13)
    kw = on_dev(family_case(kind, op, divider, N, D, bucket, gen))
    g = torch.randn(N, 2 * D if op == "cat" else D, generator=gen).to(DEV)
    lib, dev = _lib.load(), torch.device(DEV)
    T1, T2, S1, S2 = kw["T1"], kw["T2"], kw.get("S1"), kw.get("S2")
    M1, M2 = (kw[k].to(torch.uint8) if k in kw else None for k in ("M1", "M2"))
    nan = lambda t: None if t is None else torch.full_like(t, float("nan"))        # noqa: E731
    gT1, gT2, gS1, gS2 = nan(T1), nan(T2), nan(S1), nan(S2)
    ne = int(lib.mi_dual_table_bwd_workspace_elems(N, D, T1.shape[0], T2.shape[0], kw["mod1"], kw["div2"]))
    assert (ne > 0) == (kind == "qr" and divider < 8 and N > 1000)                   # only QR's long remainder rows are cut
    ws = torch.full((max(ne, 1),), float("nan"), device=DEV)
    xform = 1 if S1 is not None else (2 if M1 is not None else 0)
    rc = lib.mi_dual_table_bwd(g.data_ptr(), T1.data_ptr(), T2.data_ptr(), _lib.ptr(S1), _lib.ptr(S2), _lib.ptr(M1), _lib.ptr(M2),
                               gT1.data_ptr(), gT2.data_ptr(), _lib.ptr(gS1), _lib.ptr(gS2), N, D, T1.shape[0], T2.shape[0],
                               kw["mod1"], kw["div2"], _kernels.OPS[op], xform, ws.data_ptr() if ne else None,
                               _lib.stream_ptr(dev))
    assert rc == 0
    for name, t in (("gT1", gT1), ("gT2", gT2), ("gS1", gS1), ("gS2", gS2)):
        assert t is None or bool(torch.isfinite(t).all()), name
    ref = dual_table_bwd_ref64(g, N=N, **kw)
    if kind != "qr":
        assert bool((ref["n2"] == 0).any()) and bool((gT2[(ref["n2"] == 0).to(DEV)] == 0).all())


# -------------------------------------------------------------------------------------------------------------------- B
CF_CASES = ("cf_cerp_lightgcn_k1", "cf_cerp_lightgcn_k3", "cf_cerp_single_lightgcn_k3")


def _adj():
    a = load_golden("cf_sample_adj")
    graph = {}
    for u, i in zip(a["edge_user"].tolist(), a["edge_item"].tolist()):
        graph.setdefault(u, []).append(i)
    return calculate_sparse_graph_adj_norm(graph, int(a["num_item"]), int(a["num_user"])), int(a["num_user"]), int(a["num_item"])


def _cf_model(g, name):
    adj, nu, ni = _adj()
    cls = pkg.SingleLightGCN if "single" in name else pkg.LightGCN
    model = cls(nu, ni, num_layers=int(g["num_layers"]), hidden_size=int(g["hidden_size"]),
                embedding_config={"name": "cerp", "bucket_size": int(g["bucket_size"])})
    model.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
    return model.to(DEV), adj.to(DEV)


@pytest.mark.parametrize("name", CF_CASES)
def test_batch_row_terms_match_the_reference_step(name):
    g = load_golden(name)
    model, _ = _cf_model(g, name)
    if "single" in name:
        tables = torch.split(model.emb_table.get_weight(), (model._num_user, model._num_item))
    else:
        tables = (model.user_emb_table.get_weight(), model.item_emb_table.get_weight())
    reg, prune = losses.reg_prune_loss_rows(*tables, g.t("users").to(DEV), g.t("pos").to(DEV), g.t("neg").to(DEV))
    assert_close(reg, g.t("reg_loss"), **LOSS_TOL, what="reg_loss")
    assert_close(prune, g.t("prune_loss"), **LOSS_TOL, what="prune_loss")
    pkg.check_index_errors()


@pytest.mark.parametrize("B,K,D", [(512, 5, 32), (48, 1, 20), (2048, 5, 64)])
def test_batch_row_terms_match_float64_on_heavily_repeated_ids(B, K, D):
    gen = torch.Generator().manual_seed(B + K)
    nU, nI = 50, 70
    U, I = torch.randn(nU, D, generator=gen) * 0.01, torch.randn(nI, D, generator=gen) * 0.01     # tanh(100 w) unsaturated
    users, pos = torch.randint(0, 9, (B,), generator=gen), torch.randint(0, nI, (B,), generator=gen)
    neg = torch.randint(0, 11, (B, K), generator=gen)
    a, b = 0.7, -1.3e-3
    Ud, Id = U.to(DEV).requires_grad_(True), I.to(DEV).requires_grad_(True)
    reg, prune = losses.reg_prune_loss_rows(Ud, Id, users.to(DEV), pos.to(DEV), neg.to(DEV))
    (a * reg + b * prune).backward()
    reg64, prune64, dU, dI = reg_prune_ref64(U, I, users, pos, neg, 100.0, a, b)
    assert_close(reg, reg64.float(), **LOSS_TOL, what="reg")
    assert_close(prune, prune64.float(), **LOSS_TOL, what="prune")
    assert_close(Ud.grad, dU.float(), **GRAD_TOL, what="dU")
    assert_close(Id.grad, dI.float(), **GRAD_TOL, what="dI")
    # the reference's own form (torch.unique, four gathers) in float64 says the same
    U64, I64 = U.double(), I.double()
    emb = torch.cat([U64[torch.unique(users)], I64[pos], I64[neg.flatten()]])
    assert_close(prune, (-torch.tanh(emb * 100).norm(2) ** 2).float(), **LOSS_TOL, what="prune (reference form)")
    pkg.check_index_errors()


def test_batch_row_terms_skip_and_flag_an_id_outside_its_table():
    gen = torch.Generator().manual_seed(2)
    U, I = torch.randn(6, 8, generator=gen) * 0.01, torch.randn(9, 8, generator=gen) * 0.01
    users, pos, neg = torch.tensor([0, 1, 1, 5]), torch.tensor([3, 8, 0, 2]), torch.tensor([1, 9, 4, 4])     # 9: one past the end
    reg, prune = losses.reg_prune_loss_rows(U.to(DEV), I.to(DEV), users.to(DEV), pos.to(DEV), neg.to(DEV))
    keep = torch.tensor([0, 2, 3])
    r64, p64, _, _ = reg_prune_ref64(U, I, users, pos, neg[keep])
    assert_close(prune, p64.float(), **LOSS_TOL, what="prune")
    assert_close(reg, r64.float(), **LOSS_TOL, what="reg")
    with pytest.raises(IndexError):
        pkg.check_index_errors()


# -------------------------------------------------------------------------------------------------------------------- C
def _negatives(g, form):
    neg = g.t("neg").to(DEV)
    if form == "list":
        return [neg[:, k].contiguous() for k in range(neg.shape[1])]
    return neg[:, 0].contiguous() if neg.shape[1] == 1 else neg


@pytest.mark.parametrize("name,form", [("cf_cerp_lightgcn_k1", "tensor"), ("cf_cerp_lightgcn_k3", "list"),
                                       ("cf_cerp_lightgcn_k3", "tensor"), ("cf_cerp_single_lightgcn_k3", "list")])
def test_cerp_step_losses_and_every_gradient_match_the_reference(name, form):
    g = load_golden(name)
    model, adj = _cf_model(g, name)
    out = trainer.cf_cerp_step_losses(model, adj, g.t("users").to(DEV), g.t("pos").to(DEV), _negatives(g, form),
                                      float(g["weight_decay"]), float(g["info_nce_weight"]), float(g["prune_loss_weight"]))
    for key, val in zip(("loss", "rec_loss", "reg_loss", "cl_loss", "prune_loss"), out):
        assert_close(val, g.t(key), **LOSS_TOL, what=f"{name} {key}")
    out[0].backward()
    want = g.group("grad/")
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads) == set(want)
    for k, v in want.items():
        assert_close(grads[k], v, **GRAD_TOL, what=f"{name} {k}")
    # the BPR term over the B * K triples equals bpr_loss_multi on gathered rows
    with torch.no_grad():
        ue, ie = model(adj)
        neg = g.t("neg").to(DEV)
        multi = losses.bpr_loss_multi(ue[g.t("users").to(DEV)], ie[g.t("pos").to(DEV)], ie[neg])
    assert_close(out[1], multi, **LOSS_TOL, what="bpr_loss_multi")
    pkg.check_index_errors()


class _Data:
    def __init__(self, adj):
        self._adj = adj

    def get_norm_adj(self):
        return self._adj


class _Loader(list):
    """A list of batches with the `dataset` the epochs ask for; `before[i]()` runs just before batch i is handed out."""

    def __init__(self, batches, adj=None, before=None):
        super().__init__(batches)
        self.dataset, self.before, self.served = _Data(adj), before or {}, 0

    def __iter__(self):
        for i, b in enumerate(list.__iter__(self)):
            if i in self.before:
                self.before[i]()
            self.served += 1
            yield b


def _cf_batch(g, form="list"):
    neg = g.t("neg")
    negs = [neg[:, k].contiguous() for k in range(neg.shape[1])] if form == "list" else neg
    return (g.t("users"), g.t("pos"), negs)


def test_cerp_cf_epoch_one_step_matches_the_reference_and_clips_at_100():
    name = "cf_cerp_lightgcn_k3"
    g = load_golden(name)
    model, adj = _cf_model(g, name)
    keys = [str(k) for k in g["keys"]]
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    w = dict(weight_decay=float(g["weight_decay"]), info_nce_weight=float(g["info_nce_weight"]),
             prune_loss_weight=float(g["prune_loss_weight"]))
    out = trainer.train_epoch_cerp_cf(_Loader([_cf_batch(g)] * 3, adj), model, opt, DEV, 1, target_sparsity=2.0, **w)
    assert list(out) == keys
    for key in keys[:5]:                       # averages over three identical steps (zero learning rate)
        assert_close(torch.tensor(out[key]), g.t(key).float(), **LOSS_TOL, what=key)
    assert out["num_params"] == int(g["num_params"]) and abs(out["sparsity"] - float(g["sparsity"])) < 1e-9
    # the gradients left behind are the reference's, scaled by clip_grad_norm_(., 100)'s coefficient
    norm = float(g["grad_norm"])
    coef = min(1.0, 100.0 / (norm + 1e-6))
    for k, p in model.named_parameters():
        assert_close(p.grad, g.t("grad/" + k) * coef, **GRAD_TOL, what=k)
    # a huge prune weight pushes the norm past 100: the clipped gradient has norm 100
    w2 = dict(w, prune_loss_weight=1e3)
    trainer.train_epoch_cerp_cf(_Loader([_cf_batch(g)], adj), model, opt, DEV, 1, target_sparsity=2.0, **w2)
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters()))
    assert abs(float(total) - 100.0) < 1e-2, float(total)
    pkg.check_index_errors()


def test_cerp_cf_epoch_returns_running_sums_on_the_early_stop():
    name = "cf_cerp_lightgcn_k1"
    g = load_golden(name)
    model, adj = _cf_model(g, name)
    keys = [str(k) for k in g["keys"]]
    w = dict(weight_decay=float(g["weight_decay"]), info_nce_weight=float(g["info_nce_weight"]),
             prune_loss_weight=float(g["prune_loss_weight"]))

    def prune_all():
        with torch.no_grad():
            for _, t in model.get_embs():
                t.p_threshold.fill_(100.0)
                t.q_threshold.fill_(100.0)

    batch = _cf_batch(g, "tensor")
    batch = (batch[0], batch[1], batch[2][:, 0].contiguous())
    loader = _Loader([batch] * 6, adj, before={2: prune_all})
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    out = trainer.train_epoch_cerp_cf(loader, model, opt, DEV, 2, target_sparsity=0.8, **w)
    # logging steps are idx 0, 2, 4: the tables are emptied before batch 2, so the epoch returns after three batches
    assert loader.served == 3 and list(out) == keys and out["sparsity"] == 1.0 and out["num_params"] == 0
    pruned = trainer.cf_cerp_step_losses(model, adj, *[t.to(DEV) for t in batch], **w)
    for key, pos in (("loss", 0), ("rec_loss", 1), ("reg_loss", 2), ("cl_loss", 3), ("prune_loss", 4)):
        want = 2 * float(g[key]) + float(pruned[pos])                                   # SUMS, not averages
        assert abs(out[key] - want) <= 1e-5 * abs(want) + 1e-6, (key, out[key], want)
    assert float(pruned[4]) == 0.0 and float(pruned[2]) == 0.0
    pkg.check_index_errors()


def _neumf(g, cfg):
    m = pkg.NeuMF(int(g["num_user"]), int(g["num_item"]), emb_size=int(g["emb_size"]), hidden_sizes=[int(h) for h in g["hidden"]],
                  p_dropout=0, embedding_config=cfg)
    m.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
    return m.to(DEV)


def _neumf_case(which, tmp_path):
    g = load_golden(f"cf_cerp_neumf_{which}")
    cfg = {"name": "pep", "checkpoint_weight_dir": str(tmp_path)} if which == "pep" else {"name": "cerp", "bucket_size": 5}
    neg = g.t("neg")
    negs = [neg[:, k].contiguous() for k in range(neg.shape[1])] if neg.shape[1] > 1 else neg[:, 0].contiguous()
    return g, _neumf(g, cfg), (g.t("users"), g.t("pos"), negs)


@pytest.mark.parametrize("which", ["pep", "cerp"])
def test_neumf_pruning_step_matches_the_reference(which, tmp_path):
    g, model, batch = _neumf_case(which, tmp_path)
    users, pos, negs = batch
    negs = [t.to(DEV) for t in negs] if isinstance(negs, list) else negs.to(DEV)
    pw = float(g["prune_loss_weight"]) if which == "cerp" else 0.0
    loss, rec, reg, prune = trainer.nmf_prune_step_losses(model, users.to(DEV), pos.to(DEV), negs, float(g["weight_decay"]), pw)
    assert_close(loss, g.t("loss"), **LOSS_TOL, what="loss")
    assert_close(rec, g.t("rec_loss"), **LOSS_TOL, what="rec_loss")
    assert_close(reg, g.t("reg_loss"), **LOSS_TOL, what="reg_loss")
    if which == "cerp":
        assert_close(prune, g.t("prune_loss"), **LOSS_TOL, what="prune_loss")
    else:
        assert float(prune) == 0.0
    loss.backward()
    want = g.group("grad/")
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads) == set(want)
    for k, v in want.items():
        assert_close(grads[k], v, **GRAD_TOL, what=k)
    pkg.check_index_errors()


@pytest.mark.parametrize("which", ["pep", "cerp"])
def test_neumf_pruning_epochs_break_at_the_target_and_average(which, tmp_path):
    g, model, batch = _neumf_case(which, tmp_path)
    keys = [str(k) for k in g["keys"]]
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    kw = dict(weight_decay=float(g["weight_decay"]))
    epoch = trainer.train_epoch_pep_nmf
    if which == "cerp":
        epoch, kw = trainer.train_epoch_cerp_nmf, dict(kw, prune_loss_weight=float(g["prune_loss_weight"]))
    loader = _Loader([batch] * 4)
    out = epoch(loader, model, opt, DEV, 2, target_sparsity=2.0, **kw)
    assert loader.served == 4 and list(out) == keys
    for key in keys[:-2]:                      # averages over four identical steps (zero learning rate)
        assert_close(torch.tensor(out[key]), g.t(key).float(), **LOSS_TOL, what=key)
    assert out["num_params"] == int(g["num_params"]) and abs(out["sparsity"] - float(g["sparsity"])) < 1e-9
    loader = _Loader([batch] * 4)
    out = epoch(loader, model, opt, DEV, 2, target_sparsity=float(g["sparsity"]) - 1e-3, **kw)      # default 0 in the reference
    assert loader.served == 1 and list(out) == keys                                                  # break at idx 0
    assert_close(torch.tensor(out["loss"]), g.t("loss").float(), **LOSS_TOL, what="loss after the break")
    pkg.check_index_errors()


def _toy_loader(adj, nu, ni, K, steps=4, B=64):
    gen = torch.Generator().manual_seed(9)
    return _Loader([(torch.randint(0, nu, (B,), generator=gen), torch.randint(0, ni, (B,), generator=gen),
                     [torch.randint(0, ni, (B,), generator=gen) for _ in range(K)] if K > 1
                     else torch.randint(0, ni, (B,), generator=gen)) for _ in range(steps)], adj)


def test_lightgcn_trains_on_cerp_retrain_and_qr_tables_through_the_table_form(tmp_path):
    from recsys_benchmark_amd.embeddings import CerpEmbedding

    adj, nu, ni = _adj()
    torch.manual_seed(5)
    bucket, D = 26, 16
    for field, n in (("user", nu), ("item", ni)):
        src = CerpEmbedding(n, D, None, bucket)
        with torch.no_grad():
            src.p_threshold.copy_(torch.randn(bucket, D) - 2)
            src.q_threshold.copy_(torch.randn(bucket, D) - 2)
        os.makedirs(tmp_path / field)
        torch.save(src.state_dict(), tmp_path / field / "initial.pth")
        torch.save(src.state_dict(), tmp_path / field / "target.pth")
    configs = [({"name": "cerp", "bucket_size": bucket}, 3), ({"name": "qr", "divider": 2, "operation": "mult"}, 1),
               ({"name": "cerp_retrain", "checkpoint_weight_dir": str(tmp_path), "bucket_size": bucket}, 1)]
    for cfg, K in configs:
        model = pkg.LightGCN(nu, ni, num_layers=2, hidden_size=D, embedding_config=cfg).to(DEV)
        assert type(model.user_emb_table.get_weight().grad_fn).__name__.startswith("DualTable"), cfg
        before = copy.deepcopy(model.state_dict())
        opt = torch.optim.Adam(model.parameters(), lr=1e-2)
        loader = _toy_loader(adj, nu, ni, K)
        if cfg["name"] == "cerp":
            with torch.no_grad():
                for _, t in model.get_embs():
                    t.p_threshold.copy_(torch.randn(bucket, D) - 2)
                    t.q_threshold.copy_(torch.randn(bucket, D) - 2)
            out = trainer.train_epoch_cerp_cf(loader, model, opt, DEV, 2, weight_decay=1e-3, info_nce_weight=0.1,
                                              prune_loss_weight=1e-4, target_sparsity=2.0)
        else:
            with pytest.warns(UserWarning, match="capturable"):
                out = trainer.train_epoch_cf(loader, model, opt, DEV, 2, weight_decay=1e-3, info_nce_weight=0.1)
        assert all(math.isfinite(v) for v in out.values()), (cfg, out)
        assert out["rec_loss"] > 0
        moved = [k for k, v in model.state_dict().items() if v.is_floating_point() and not torch.equal(v, before[k].to(v.device))]
        assert any("weight" in k for k in moved), cfg
        pkg.check_index_errors()

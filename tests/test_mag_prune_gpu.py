"""GPU: magnitude pruning on the device (csrc/mag_prune.hip) against the reference's recorded results and against the
CPU restatement of the contract (tests/mag_prune_helpers.py).  The feature moves and zeroes values, it computes none:
every comparison is torch.equal."""
import copy
import re

import pytest
import torch

from conftest import load_golden

import mag_prune_helpers as H
import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import pruning, trainer
from recsys_benchmark_amd.embeddings import PrunedEmbedding

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = load_golden("mag_prune_tables")
TABLE_CASES = [str(c) for c in TABLES["cases"]]


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal AND the same sign on every zero (pruned elements are +0.0; a copied -0.0 stays -0.0)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def case_args(case):
    table, rest = case.split("/")
    p, m = re.fullmatch(r"p([0-9.]+)_m(\d+)", rest).groups()
    return table, float(p), int(m)


# ---- the reference's recorded results -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE_CASES)
def test_prune_table_equals_the_reference(case):
    table, p, m = case_args(case)
    w = TABLES.t(f"in/{table}")
    want = TABLES.t(f"out/{case}")
    src = w.to(DEV)
    out = torch.full_like(src, float("nan"))
    assert pkg.prune_table(src, p, m, out=out) is out
    assert torch.equal(out.cpu(), want) and bits_equal(out, H.mag_prune(w, p, m))
    assert torch.equal(src.cpu(), w), "the input is untouched when out is given"
    assert pkg.prune_table(src, p, m) is src
    assert torch.equal(src.cpu(), want)


def test_prune_state_dict_equals_the_reference():
    p, m = float(TABLES["state/p"]), int(TABLES["state/min_item"])
    state = {k: TABLES.t(f"state/in/{k}").to(DEV) for k in ("user", "item")}
    alias = dict(state)
    got = pkg.prune(state, p, m)
    assert got is state
    for k in ("user", "item"):
        assert got[k] is alias[k], "pruned in place"
        assert torch.equal(got[k].cpu(), TABLES.t(f"state/out/{k}"))


# ---- the contract on seeded shapes beyond the fixtures ----------------------------------------------------------------
SHAPES = [(1, 8), (63, 8), (4097, 16), (38048, 16), (63, 24), (4097, 24), (1, 32), (4097, 32), (63, 64), (38048, 64),
          (63, 100), (4097, 100), (1, 128), (4097, 128), (63, 256), (4097, 256), (1, 1024), (63, 1024), (4097, 1024)]


def variants(n, d):
    total = n * d
    out = [(1.0 / total, 0), ((total - 1) / total, 0), (0.5, 1), (0.37, 0)]
    if d > 1:
        out.append((1.0 / (2 * d), d - 1))          # k = N / 2 <= N: the floor D - 1 is allowed
    return out


@pytest.mark.parametrize("n,d", SHAPES)
def test_prune_table_equals_the_contract(n, d):
    gen = torch.Generator().manual_seed(1000 * d + n)
    w = torch.randn(n, d, generator=gen) * 0.1
    src = w.to(DEV)
    for i, (p, m) in enumerate(variants(n, d)):
        want = H.mag_prune(w, p, m)
        if i % 2 == 0:
            out = torch.full_like(src, float("nan"))
            pkg.prune_table(src, p, m, out=out)
            assert torch.equal(src.cpu(), w)
        else:
            out = pkg.prune_table(src.clone(), p, m)
        assert bits_equal(out, want), (n, d, p, m)


@pytest.mark.parametrize("n,d,pad", [(1000, 16, 16), (777, 64, 4), (500, 24, 3), (300, 100, 1)])
def test_strided_views(n, d, pad):
    """Column slices of a wider table (what DeepFM.pack_tables() makes), as input, as output and in place; the
    columns outside the slice are not touched."""
    gen = torch.Generator().manual_seed(n + d)
    wide = torch.randn(n, d + 2 * pad, generator=gen)
    w = wide[:, pad:pad + d]
    want = H.mag_prune(w.contiguous(), 0.6, 2)
    g_wide = wide.to(DEV)
    out_wide = torch.full((n, d + pad), 7.0, device=DEV)
    pkg.prune_table(g_wide[:, pad:pad + d], 0.6, 2, out=out_wide[:, :d])
    assert bits_equal(out_wide[:, :d], want) and bool((out_wide[:, d:] == 7.0).all())
    assert torch.equal(g_wide.cpu(), wide)
    pkg.prune_table(g_wide[:, pad:pad + d], 0.6, 2)
    assert bits_equal(g_wide[:, pad:pad + d], want)
    assert torch.equal(g_wide[:, :pad].cpu(), wide[:, :pad]) and torch.equal(g_wide[:, pad + d:].cpu(), wide[:, pad + d:])
    t = torch.randn(d, n, generator=gen)                      # a transposed view: not row-strided
    g_t = t.to(DEV).t()
    pkg.prune_table(g_t, 0.6, 2)
    assert bits_equal(g_t, H.mag_prune(t.t().contiguous(), 0.6, 2))


# ---- ties ---------------------------------------------------------------------------------------------------------
def tie_tables():
    gen = torch.Generator().manual_seed(77)
    quant = torch.round(torch.randn(3001, 16, generator=gen) * 4) / 4
    yield "quantised to 1/4", quant, [(0.5, 0), (0.3, 2), (0.8, 3), (0.05, 0)]
    yield "quantised, D = 100", torch.round(torch.randn(257, 100, generator=gen) * 4) / 4, [(0.5, 0), (0.7, 5)]
    yield "all equal", torch.full((130, 64), -0.25), [(0.5, 0), (0.5, 7), (0.999, 0), (1.0, 0), (0.0, 3)]
    sparse = torch.randn(2000, 32, generator=gen)
    sparse[torch.rand(2000, 32, generator=gen) < 0.9] = 0.0
    yield "90 % zeros, the cut inside the zeros", sparse, [(0.5, 0), (0.5, 4), (0.95, 0)]
    signed = torch.randn(513, 24, generator=gen)
    signed[torch.rand(513, 24, generator=gen) < 0.5] = -0.0
    yield "-0.0 entries", signed, [(0.25, 0), (0.25, 2), (0.6, 1)]
    den = torch.randn(700, 16, generator=gen)
    tiny = torch.randint(1, 50, (700, 16), generator=gen).to(torch.int32).view(torch.float32)      # denormals, many equal
    den = torch.where(torch.rand(700, 16, generator=gen) < 0.5, tiny * torch.sign(den), den)
    yield "denormals", den, [(0.3, 0), (0.45, 3), (0.7, 0)]
    inf = torch.randn(400, 64, generator=gen)
    inf[torch.rand(400, 64, generator=gen) < 0.1] = float("inf")
    inf[torch.rand(400, 64, generator=gen) < 0.05] = float("-inf")
    yield "inf entries", inf, [(0.5, 0), (0.9, 2), (0.95, 0), (1.0, 0)]


@pytest.mark.parametrize("name,w,settings", list(tie_tables()), ids=[t[0] for t in tie_tables()])
def test_ties_follow_the_contract(name, w, settings):
    src = w.to(DEV)
    for p, m in settings:
        want = H.mag_prune(w, p, m)
        out = torch.full_like(src, float("nan"))
        pkg.prune_table(src, p, m, out=out)
        assert bits_equal(out, want), (name, p, m)
        assert bits_equal(pkg.prune_table(src.clone(), p, m), want), (name, p, m, "in place")
        emb = PrunedEmbedding.from_pruned(src, p, m)
        ref = PrunedEmbedding.from_weight(want.to(DEV))
        for got, exp in ((emb.crow_indices, ref.crow_indices), (emb.col_indices, ref.col_indices), (emb.values, ref.values)):
            assert got.dtype == exp.dtype and torch.equal(got, exp), (name, p, m, "csr")
    assert torch.equal(src.cpu().view(torch.int32), w.view(torch.int32))


def test_select_threshold_reports_the_cut():
    w = torch.tensor([[1.0, -1.0, 1.0, 2.0], [-0.0, 0.0, 1.0, -1.0]])
    one = int(torch.tensor(1.0).view(torch.int32))
    assert pruning._select_threshold(w.to(DEV), 0.5, 0).tolist() == [one, 2, 5, 2]
    assert pruning._select_threshold(w.to(DEV), 0.5, 1).tolist() == [one, 2, 4, 2]
    assert pruning._select_threshold(w.to(DEV), 0.25, 0).tolist() == [0, 0, 2, 2]
    assert pruning._select_threshold(w.to(DEV), 0.0, 0).tolist() == [0, 0, 2, 0]
    big = H.distinct_table(5000, 64, 11)
    k = int(5000 * 64 * 0.8)
    kth = torch.sort(big.abs().flatten()).values[k - 1]
    assert pruning._select_threshold(big.to(DEV), 0.8, 0).tolist() == [int(kth.view(torch.int32)), k - 1, 1, 1]


def test_two_runs_give_identical_bits():
    gen = torch.Generator().manual_seed(3)
    w = (torch.round(torch.randn(38048, 64, generator=gen) * 64) / 64).to(DEV)       # ties at the cut
    a = pkg.prune_table(w, 0.8, 6, out=torch.empty_like(w))
    b = pkg.prune_table(w, 0.8, 6, out=torch.empty_like(w))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ea, eb = PrunedEmbedding.from_pruned(w, 0.8, 6), PrunedEmbedding.from_pruned(w, 0.8, 6)
    assert torch.equal(ea.col_indices, eb.col_indices) and torch.equal(ea.values.view(torch.int32), eb.values.view(torch.int32))
    assert bits_equal(ea.get_weight(), a)


# ---- CSR ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,p,m", [(77, 16, 0.5, 0), (77, 16, 0.8, 3), (4097, 64, 0.8, 6), (38048, 64, 0.8, 0), (63, 100, 0.6, 2),
                                     (500, 8, 0.9, 0), (129, 1024, 0.5, 1), (9000, 24, 0.99, 0), (1, 32, 0.5, 0)])
def test_from_pruned_equals_from_weight_of_the_pruned_table(n, d, p, m):
    gen = torch.Generator().manual_seed(n * 7 + d)
    w = torch.randn(n, d, generator=gen)
    want = H.mag_prune(w, p, m)
    src = w.to(DEV)
    emb = PrunedEmbedding.from_pruned(src, p, m)
    ref = PrunedEmbedding.from_weight(want.to(DEV))
    for name in ("crow_indices", "col_indices", "values"):
        got, exp = getattr(emb, name), getattr(ref, name)
        assert got.dtype == exp.dtype and got.shape == exp.shape and torch.equal(got, exp), name
    assert torch.equal(src.cpu(), w)
    ids = torch.randint(0, n, (3, 50), generator=gen).to(DEV)
    assert torch.equal(emb(ids).cpu(), want[ids.cpu()])
    assert torch.equal(emb.get_weight().cpu(), want)
    pkg.check_index_errors()


def test_from_pruned_takes_an_embedding_and_a_bag_mode():
    table = pkg.VanillaEmbedding(300, 16).to(DEV)
    before = table.get_weight().detach().cpu().clone()
    want = H.mag_prune(before, 0.7, 1)
    emb = PrunedEmbedding.from_pruned(table, 0.7, 1, mode="sum")
    ids = torch.randint(0, 300, (9, 4)).to(DEV)
    assert torch.equal(emb(ids).cpu(), want[ids.cpu()].sum(1))
    assert torch.equal(table.get_weight().detach().cpu(), before), "the source table is not pruned"


def test_dense_to_csr_with_zero_rows_and_negative_zeros():
    gen = torch.Generator().manual_seed(9)
    w = torch.randn(1500, 24, generator=gen)
    w[torch.rand(1500, 24, generator=gen) < 0.6] = 0.0
    w[torch.rand(1500, 24, generator=gen) < 0.1] = -0.0
    w[::7] = 0.0
    w[5] = -0.0
    w[-1] = 0.0
    emb = PrunedEmbedding.from_pruned(w.to(DEV), 0.0)
    ref = PrunedEmbedding.from_weight(w.to(DEV))
    for name in ("crow_indices", "col_indices", "values"):
        got, exp = getattr(emb, name), getattr(ref, name)
        assert got.dtype == exp.dtype and torch.equal(got, exp), name
    cpu = w.to_sparse_csr()
    assert torch.equal(emb.crow_indices.cpu(), cpu.crow_indices()) and torch.equal(emb.col_indices.cpu(), cpu.col_indices())
    empty = PrunedEmbedding.from_pruned(torch.zeros(70, 16, device=DEV), 0.5)
    assert empty.values.numel() == 0 and int(empty.crow_indices.abs().sum()) == 0


# ---- models: candidates, search, serving ----------------------------------------------------------------------------
class _ToyCF:
    """The two methods of the reference's CFGraphDataset that validation uses."""

    def __init__(self, num_user=60, num_item=90, seed=0):
        from recsys_benchmark_amd.graph_utils import calculate_sparse_graph_adj_norm

        gen = torch.Generator().manual_seed(seed)
        self.num_user, self.num_item = num_user, num_item
        self.graph = {u: sorted(set(torch.randint(0, num_item, (int(torch.randint(2, 12, (1,), generator=gen)),),
                                                  generator=gen).tolist())) for u in range(num_user)}
        self.adj = calculate_sparse_graph_adj_norm(self.graph, num_item, num_user)
        self.val = [(torch.arange(s, min(s + 25, num_user)),
                     [sorted(set(torch.randint(0, num_item, (4,), generator=gen).tolist())) for _ in range(s, min(s + 25, num_user))])
                    for s in range(0, num_user, 25)]

    def get_norm_adj(self):
        return self.adj

    def get_graph(self):
        return self.graph


HIDDEN = 16


def _build(kind):
    torch.manual_seed(11)
    data = _ToyCF()
    if kind == "lightgcn":
        model = pkg.LightGCN(data.num_user, data.num_item, num_layers=2, hidden_size=HIDDEN)
    elif kind == "single":
        model = pkg.SingleLightGCN(data.num_user, data.num_item, num_layers=2, hidden_size=HIDDEN)
    else:
        model = pkg.NeuMF(data.num_user, data.num_item, emb_size=2 * HIDDEN, hidden_sizes=[16, 8])
    validate = trainer.validate_epoch_nmf if kind == "neumf" else trainer.validate_epoch_cf
    return model.to(DEV), data, validate


def _table_keys(model, kind):
    return [k for k in model.state_dict() if kind != "neumf" or "emb_table" in k]


def _helper_pruned_model(model, kind, p, m):
    other = copy.deepcopy(model)
    state = other.state_dict()
    for k in _table_keys(model, kind):
        state[k].copy_(H.mag_prune(state[k].cpu(), p, m))
    return other


def _bits(model):
    return {k: v.detach().clone().view(torch.int32) for k, v in model.state_dict().items() if v.dtype == torch.float32}


@pytest.mark.parametrize("kind", ["lightgcn", "single", "neumf"])
def test_evaluate_pruned_search_and_serving(kind):
    model, data, validate = _build(kind)
    before = _bits(model)
    assert all(model.state_dict()[k].dim() == 2 for k in _table_keys(model, kind))
    p = 0.5

    def by_helper(m):
        return validate(data, data.val, _helper_pruned_model(model, kind, p, m), DEV, metrics=["ndcg", "recall"])["ndcg"]

    for m in (0, 3):
        got = pkg.evaluate_pruned(model, p, m, data.val, data, DEV)
        assert got == by_helper(m), (kind, m)
        after = _bits(model)
        assert all(torch.equal(before[k], after[k]) for k in before), "the state is bit-identical afterwards"
    assert pkg.evaluate_pruned(model, 0.0, 0, data.val, data, DEV) == validate(data, data.val, model, DEV)["ndcg"]

    class Boom(RuntimeError):
        pass

    def failing(train_dataset, val_loader, mdl, device, metrics=None):
        keys = _table_keys(mdl, kind)
        assert any(int((mdl.state_dict()[k] == 0).sum()) > 0 for k in keys), "validation sees the pruned tables"
        raise Boom()

    with pytest.raises(Boom):
        pkg.evaluate_pruned(model, p, 1, data.val, data, DEV, validate=failing)
    after = _bits(model)
    assert all(torch.equal(before[k], after[k]) for k in before), "restored when validation raises"

    bound = int(HIDDEN * (1 - p))
    # the expected value: the same search routine (its probe order is pinned to the reference by the recorded fixture in
    # test_mag_prune_host.py) run over helper-pruned tables, so what is compared here is the pruning beneath the search
    assert pkg.search_min_item(model, p, HIDDEN, data.val, data, DEV) == \
        pkg.search_min_item(None, p, HIDDEN, mode="binary", evaluate=by_helper)
    scores = [by_helper(m) for m in range(bound + 1)]
    assert pkg.search_min_item(model, p, HIDDEN, data.val, data, DEV, mode="all") == int(torch.tensor(scores).argmax()) + 1
    after = _bits(model)
    assert all(torch.equal(before[k], after[k]) for k in before)

    dense = _helper_pruned_model(model, kind, p, 2)
    served = pkg.to_pruned_tables(copy.deepcopy(model), p, 2)
    assert all(isinstance(getattr(o, n), PrunedEmbedding) for o, n in pruning._table_slots(served))
    users = torch.arange(data.num_user, device=DEV)
    if kind == "neumf":
        dense.eval(), served.eval()
        assert torch.equal(served.score_all_items(users), dense.score_all_items(users))
        for a, b in zip(served._tables(), dense._tables()):
            assert torch.equal(a.get_weight(), b.get_weight())
    else:
        adj = data.get_norm_adj().to(DEV)
        for a, b in zip(served(adj), dense(adj)):
            assert torch.equal(a, b)
    assert validate(data, data.val, served, DEV)["ndcg"] == by_helper(2)
    plain = pkg.to_pruned_tables(copy.deepcopy(model))
    assert validate(data, data.val, plain, DEV)["ndcg"] == validate(data, data.val, model, DEV)["ndcg"]
    pkg.check_index_errors()


# ---- full size ------------------------------------------------------------------------------------------------------
def test_fullsize_criteo_table_properties():
    """33 762 577 x 16 (the Criteo-Kaggle table of BASELINE.json), p = 0.8, m = 2, by properties that need no sort."""
    N, D, p, m = 33762577, 16, 0.8, 2
    gen = torch.Generator(device=DEV).manual_seed(2023)
    W = (torch.rand(N, D, device=DEV, generator=gen) - 0.5) * 0.1
    W[W == 0] = 1.0
    k = int(N * D * p)
    out = pkg.prune_table(W, p, m, out=torch.empty_like(W))
    zero = out == 0
    assert int(zero.sum()) == k, "exactly k elements changed to zero"
    assert torch.equal(torch.where(zero, W, out), W), "everything else is copied"
    assert int((~zero).sum(1).min()) >= m, "every row keeps at least m"
    mag = W.abs()
    top = mag.topk(m, 1).values
    assert torch.equal(out.abs().topk(m, 1).values, top), "each row's m largest survive"
    max_pruned = mag[zero].max()
    free = ~zero & (mag < top[:, m - 1:m])                  # kept although certainly not protected by the floor
    assert bool(free.any()) and float(max_pruned) <= float(mag[free].min()), "max |pruned| <= min |kept, unprotected|"
    del zero, free, mag, top
    res = pruning._select_threshold(W, p, m).tolist()
    assert res[1] + res[3] == k and 1 <= res[3] <= res[2]
    assert int(torch.tensor(float(max_pruned)).view(torch.int32)) == res[0]

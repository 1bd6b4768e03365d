"""CPU: the device-resident CF datasets' host side against the reference's recorded dataset fields
(tests/golden/cf_data_sample.npz), and the NumPy restatement of the sampler (tests/cf_data_helpers.py — the
specification tests/test_cf_data_gpu.py holds the kernel to, bit for bit): its structural properties and its law."""
import numpy as np
import pytest
import torch

from cf_data_helpers import (HostGraph, chi2_quantile, chi2_sf, chi2_stat, draw_scalar, draws, graph_from_pairs,
                             nearly_full_graph, sample_restated, sample_scalar, skewed_graph)
from conftest import load_golden

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import cf_data, graph_utils

SEED = 20240229


def sample_graph():
    g = load_golden("cf_data_sample")
    return g, graph_from_pairs(g["pair_user"], g["pair_item"])


def write_graph(path, graph, empty_user=None):
    with open(path, "w") as f:
        for u, items in graph.items():
            f.write(" ".join(str(x) for x in [u] + list(items)) + "\n")
        if empty_user is not None:
            f.write(f"{empty_user}\n")
    return str(path)


@pytest.mark.parametrize("mode", ["uniform", "popularity"])
def test_dataset_fields_equal_the_reference(tmp_path, mode):
    g, graph = sample_graph()
    path = write_graph(tmp_path / "cf.txt", graph, empty_user=len(graph))
    for src in (path, graph):
        ds = pkg.DeviceCFGraphDataset(src, sampling_method=mode, num_neg_item=3, device="cpu")
        assert (ds.num_users, ds.num_items, ds.per_user_num) == (int(g["num_users"]), int(g["num_items"]), int(g["per_user_num"]))
        assert len(ds) == int(g["len_uniform"] if mode == "uniform" else g["len_popularity"])
        assert torch.equal(ds.pair_user, g.t("pair_user")) and torch.equal(ds.pair_item, g.t("pair_item"))
        assert ds.get_graph() == graph and list(ds.get_graph()) == g["users"].tolist()
        assert [2, 79] in torch.stack([ds.pair_user, ds.pair_item], 1).tolist()
        assert graph[2].count(79) == 2                                   # the duplicated interaction is kept ...
        row = ds.pos_col[ds.pos_crow[2]:ds.pos_crow[3]].tolist()
        assert row == sorted(set(graph[2])) and row.count(79) == 1       # ... in the stored list, once in the membership
        ds.describe()


def test_default_arguments_are_the_references():
    import inspect

    p = inspect.signature(pkg.DeviceCFGraphDataset.__init__).parameters
    assert [(k, v.default) for k, v in list(p.items())[2:]] == [("adj_style", "lightgcn"), ("sampling_method", "uniform"),
                                                                 ("num_neg_item", 1), ("device", "cuda")]


def test_arrays_equal_the_restatements():
    _, graph = sample_graph()
    shuffled = {u: graph[u] for u in reversed(list(graph))}              # a file that lists its users backwards
    for gr in (graph, shuffled, nearly_full_graph(3)):
        ds, hg = pkg.DeviceCFGraphDataset(gr, device="cpu"), HostGraph(gr)
        assert np.array_equal(ds.pair_user.numpy(), hg.pair_user) and np.array_equal(ds.pair_item.numpy(), hg.pair_item)
        assert np.array_equal(ds.stored_item.numpy(), hg.stored) and np.array_equal(ds.pair_crow.numpy(), hg.pair_crow)
        assert np.array_equal(ds.pos_crow.numpy(), hg.pos_crow) and np.array_equal(ds.pos_col.numpy(), hg.pos_col)
        assert ds.pos_col.dtype == torch.int32 and (ds.num_items, ds.per_user_num) == (hg.I, hg.per_user_num)
        crow, col = pkg.lightgcn.train_items_csr(ds.get_graph(), ds.num_users)
        want = pkg.lightgcn.train_items_csr(dict(gr), ds.num_users)         # a plain dict: today's host path
        assert torch.equal(crow, want[0]) and torch.equal(col, want[1])


def test_norm_adj_is_graph_utils(tmp_path):
    _, graph = sample_graph()
    ds = pkg.DeviceCFGraphDataset(graph, device="cpu")
    want = graph_utils.calculate_sparse_graph_adj_norm(graph, ds.num_items, ds.num_users)
    got = ds.get_norm_adj()
    assert got is ds.get_norm_adj()
    assert torch.equal(got.crow_indices(), want.crow_indices()) and torch.equal(got.col_indices(), want.col_indices())
    assert torch.equal(got.values(), want.values())
    hccf = pkg.DeviceCFGraphDataset(graph, adj_style="hccf", device="cpu").get_norm_adj()
    want = graph_utils.get_adj(graph, ds.num_items, ds.num_users, normalize=True)
    assert torch.equal(hccf.indices(), want.indices()) and torch.equal(hccf.values(), want.values())
    with pytest.raises(ValueError):
        pkg.DeviceCFGraphDataset(graph, adj_style="dense", device="cpu")


def test_user_ids_must_be_contiguous():
    with pytest.raises(ValueError):
        pkg.DeviceCFGraphDataset({0: [1], 2: [3]}, device="cpu")
    with pytest.raises(ValueError):
        pkg.DeviceCFGraphDataset({1: [1], 2: [3]}, device="cpu")
    with pytest.raises(ValueError):
        pkg.DeviceCFTestDataset({0: [1], 5: [3]}, device="cpu")
    assert pkg.DeviceCFGraphDataset({1: [1], 0: [3]}, device="cpu").num_users == 2


def test_there_is_no_host_sampler():
    ds = pkg.DeviceCFGraphDataset(nearly_full_graph(3), device="cpu")
    with pytest.raises(pkg.MI355XLibraryError):
        ds.sample(0, 4, 0, 1)
    with pytest.raises(IndexError):
        ds.sample(0, len(ds) + 1, 0, 1)


def test_loader_lengths_and_test_dataset():
    g, graph = sample_graph()
    ds = pkg.DeviceCFGraphDataset(graph, sampling_method="popularity", device="cpu")
    assert len(pkg.DeviceCFLoader(ds, 100)) == 8 and len(pkg.DeviceCFLoader(ds, 100, drop_last=True)) == 7
    assert pkg.DeviceCFLoader(ds, 100, seed=5).seed == 5 and pkg.DeviceCFLoader(ds, 100).seed == torch.initial_seed()
    test = pkg.DeviceCFTestDataset(graph, device="cpu")
    assert len(test) == int(g["test_len"]) and test.users.tolist() == g["test_users"].tolist()
    assert torch.equal(test.truth.crow, g.t("truth_crow")) and torch.equal(test.truth.col, g.t("truth_col"))
    batches = list(pkg.DeviceCFTestLoader(test, 32))
    assert [b[0].numel() for b in batches] == [32, 32, 13] and all(isinstance(b[1], cf_data.DeviceTruth) for b in batches)
    assert len(pkg.DeviceCFTestLoader(test, 32)) == 3


# ---- the restatement: structure -----------------------------------------------------------------------------------------
def test_vector_restatement_equals_the_scalar_one():
    assert draws(SEED, 3, np.arange(50), 2, np.full(50, 97)).tolist() == [draw_scalar(SEED, 3, i, 2, 97) for i in range(50)]
    _, graph = sample_graph()
    for gr, K in ((graph, 3), (nearly_full_graph(3), 3), (nearly_full_graph(3), 4)):
        hg = HostGraph(gr)
        for mode in ("uniform", "popularity"):
            n = hg.epoch_len(mode)
            order = np.random.default_rng(1).permutation(n) if mode == "popularity" else None
            users, pos, neg = sample_restated(hg, mode, K, 0, n, SEED, 5, order)
            for i in range(0, n, 7):
                u, p, negs = sample_scalar(hg, mode, K, i, SEED, 5, None if order is None else int(order[i]))
                assert (users[i], pos[i], neg[:, i].tolist()) == (u, p, negs), (mode, i)


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("mode", ["uniform", "popularity"])
def test_restatement_properties(mode, K):
    _, graph = sample_graph()
    for gr in (graph, nearly_full_graph(min(K, 3)), skewed_graph(300, 64, 6000, 7)):
        hg = HostGraph(gr)
        n = hg.epoch_len(mode)
        order = np.random.default_rng(2).permutation(n) if mode == "popularity" else None
        users, pos, neg = sample_restated(hg, mode, K, 0, n, SEED, 1, order)
        for i in range(n):
            u = i // hg.per_user_num if mode == "uniform" else int(hg.pair_user[order[i]])
            if len(set(gr[u])) + K > hg.I:
                assert users[i] == -1 and pos[i] == -1 and (neg[:, i] == -1).all()
                continue
            assert users[i] == u and pos[i] in gr[u]                        # a positive of the stored list
            if mode == "popularity":
                assert pos[i] == hg.pair_item[order[i]]                     # sample i is pair order[i]
            negs = neg[:, i].tolist()
            assert len(set(negs)) == K and not set(negs) & set(gr[u])       # distinct, outside the positives
            assert min(negs) >= 0 and max(negs) < hg.I
        first, m = n // 3, n // 2                                           # a sub-range is the slice of the epoch
        sub = sample_restated(hg, mode, K, first, m, SEED, 1, None if order is None else order[first:first + m])
        assert all(np.array_equal(a[..., first:first + m], b) for a, b in zip((users, pos, neg), sub))
        other = sample_restated(hg, mode, K, 0, n, SEED, 2, order)          # another epoch draws other negatives
        assert not np.array_equal(other[2], neg)


def test_a_user_holding_all_but_k_items_gets_exactly_those():
    hg = HostGraph(nearly_full_graph(3))
    order = np.full(500, int(hg.pair_crow[1]))
    _, _, neg = sample_restated(hg, "popularity", 3, 0, 500, SEED, 0, order)
    assert all(sorted(neg[:, i].tolist()) == [0, 13, 39] for i in range(500))
    assert len({tuple(neg[:, i]) for i in range(500)}) == 6                 # all orders of the three occur


# ---- the restatement: law -------------------------------------------------------------------------------------------------
N_DRAWS = 200_000
P_TAIL = 1e-6


def test_chi2_helper():
    assert abs(chi2_sf(chi2_quantile(P_TAIL, 29), 29) - P_TAIL) < 1e-12
    assert abs(chi2_quantile(0.05, 1) - 3.841458820694124) < 1e-9 and abs(chi2_quantile(0.01, 10) - 23.209251158954356) < 1e-9


def _counts(values, cells):
    where = {c: k for k, c in enumerate(cells)}
    out = np.zeros(len(cells))
    for v, c in zip(*np.unique(values, return_counts=True)):
        if int(v) in where:
            out[where[int(v)]] += c
    return out


def test_law_of_the_negatives_and_of_the_positive():
    """Deterministic: the seed is fixed, and the restatement passed every bound below with it when this test was
    written (SEED = 20240229 was the first seed tried).  200 000 draws per tested user on a 40-item graph; each Pearson
    statistic must lie below the 1 - 1e-6 quantile of its chi-square law.  The variant that hands out the rank instead
    of rank + j must FAIL the same bound: the test detects a sampler that ignores the positives."""
    gr = nearly_full_graph(3)
    hg = HostGraph(gr)
    for u in (0, 2):
        free = [i for i in range(hg.I) if i not in set(gr[u])]
        bound = chi2_quantile(P_TAIL, len(free) - 1)
        order = np.full(N_DRAWS, int(hg.pair_crow[u]))
        _, _, neg1 = sample_restated(hg, "popularity", 1, 0, N_DRAWS, SEED, 0, order)
        stat = chi2_stat(_counts(neg1[0], free))
        print(f"user {u}: K=1 chi2 {stat:.2f} (bound {bound:.2f}, {len(free) - 1} df)")
        assert _counts(neg1[0], free).sum() == N_DRAWS and stat < bound
        _, _, neg3 = sample_restated(hg, "popularity", 3, 0, N_DRAWS, SEED, 0, order)
        for where in (0, 2):
            stat = chi2_stat(_counts(neg3[where], free))
            print(f"user {u}: K=3 position {where} chi2 {stat:.2f} (bound {bound:.2f})")
            assert _counts(neg3[where], free).sum() == N_DRAWS and stat < bound
        for K, where in ((1, 0), (3, 0), (3, 2)):
            _, _, wrong = sample_restated(hg, "popularity", K, 0, N_DRAWS, SEED, 0, order, rank_as_item=True)
            stat = chi2_stat(_counts(wrong[where], free))
            print(f"user {u}: rank-as-item K={K} position {where} chi2 {stat:.0f}")
            assert stat > bound
    # the positive of a uniform sample: an entry of the STORED list, so the duplicated item 7 of user 2 comes twice as often
    per = hg.per_user_num
    n_epochs = -(-N_DRAWS // per)
    pos = np.concatenate([sample_restated(hg, "uniform", 1, 2 * per, per, SEED, e)[1] for e in range(n_epochs)])
    counts = _counts(pos, [5, 7, 9])
    expected = pos.size * np.array([0.25, 0.5, 0.25])
    stat = float(((counts - expected) ** 2 / expected).sum())
    print(f"stored-list positive chi2 {stat:.2f} (bound {chi2_quantile(P_TAIL, 2):.2f})")
    assert counts.sum() == pos.size and stat < chi2_quantile(P_TAIL, 2)
    assert float(((counts - pos.size / 3) ** 2 / (pos.size / 3)).sum()) > chi2_quantile(P_TAIL, 2)   # not the distinct law

"""GPU: the CF OptEmbed (csrc/optembed_cf.hip, embeddings/cf_opt_embed.py) against the reference's fixtures
(tests/golden/optembed_cf_*.npz), the device draws against their laws, graph replay, the trainer and the search, and
the Yelp2018 table shape against a float64 restatement."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import trainer
from recsys_benchmark_amd.embeddings import get_embedding
from recsys_benchmark_amd.embeddings import cf_opt_embed as cf
from recsys_benchmark_amd.graph_utils import calculate_sparse_graph_adj_norm
from recsys_benchmark_amd.neumf import NeuMF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLE_CASES = ["l1_field_field", "l2_feature_feature", "l1_feature_field", "l2_field_feature_d6", "d_only"]


def _eq(a, b, what=""):
    torch.testing.assert_close(a.detach().cpu(), torch.as_tensor(b), rtol=0, atol=0, msg=what)


def _close(a, b, what="", rtol=1e-5, atol=1e-6):
    torch.testing.assert_close(a.detach().cpu().float(), torch.as_tensor(b).float(), rtol=rtol, atol=atol, msg=what)


def _table(g):
    cfg = {"name": "optembed" if bool(g["has_t"]) else "optembed_d", "norm": int(g["norm"]),
           "mode_threshold_e": str(g["mode_e"]), "mode_threshold_d": str(g["mode_d"])}
    emb = get_embedding(cfg, g["dims"].tolist(), int(g["hidden"]))
    emb.load_state_dict({k: g.t("param/" + k) for k in emb.state_dict()})
    return emb.to(DEV)


@pytest.mark.parametrize("case", TABLE_CASES)
def test_table_matches_reference(case):
    g = load_golden(f"optembed_cf_{case}")
    emb = _table(g)
    G = g.t("g").to(DEV)
    field_d = str(g["mode_d"]) == "field"
    masks = {"train_rows": (True, g.t("row_mask")), "train_bool": (True, g.t("bool_mask")), "eval_none": (False, None),
             "eval_int": (False, g.t("field_mask") if field_d else g.t("row_mask"))}
    for tag, (train, mask) in masks.items():
        emb.train(train)
        emb.zero_grad()
        w = emb.get_weight(None if mask is None else mask.to(DEV))
        (w * G).sum().backward()
        _eq(w, g[f"{tag}/out"], tag)
        for name, p in emb.named_parameters():
            key = f"{tag}/grad/{name}"
            if key in g:
                _close(p.grad, g[key], key)
    x = g.t("x").to(DEV)
    emb.train()
    _eq(emb(x, g.t("row_mask")), g["fwd_train"], "forward, training")
    emb.eval()
    emb._cur_weight = None
    _eq(emb(x, (g.t("field_mask") if field_d else g.t("row_mask")).to(DEV)), g["fwd_eval"], "forward, eval")
    _eq(emb(x), g["fwd_eval_cached"], "forward, eval cache")
    _close(torch.as_tensor(emb.get_l_s()), g["l_s"], "l_s")
    sp, n = emb.get_sparsity(True)
    assert n == int(g["n_params"]) and sp == pytest.approx(float(g["sparsity"]))
    pkg.check_index_errors()


@pytest.mark.parametrize("md", ["feature", "field"])
def test_retrain_matches_reference(md):
    g = load_golden(f"optembed_cf_retrain_{md}")
    emb = get_embedding({"name": "optembed_d_retrain", "mode_threshold_d": md}, [7, 9], 8)
    emb.load_state_dict({k: g.t("param/" + k) for k in emb.state_dict() if k != "_mask"}, strict=False)
    emb = emb.to(DEV)
    emb.init_mask(g.t("mask_e"), g.t("mask_d"))
    emb.train()
    w = emb.get_weight()
    (w * g.t("g").to(DEV)).sum().backward()
    _eq(w, g["out"])
    _close(emb._weight.grad, g["grad/_weight"])


def _sample_graph():
    a = load_golden("cf_sample_adj")
    graph = {}
    for u, i in zip(a["edge_user"].tolist(), a["edge_item"].tolist()):
        graph.setdefault(u, []).append(i)
    nu, ni = int(a["num_user"]), int(a["num_item"])
    return graph, nu, ni, calculate_sparse_graph_adj_norm(graph, ni, nu)


@pytest.mark.parametrize("name", ["lightgcn", "single_lightgcn"])
def test_lightgcn_on_optembed_tables_matches_reference(name):
    g = load_golden(f"optembed_cf_{name}")
    graph, nu, ni, adj = _sample_graph()
    cfg = {"name": "optembed", "mode_threshold_d": "feature", "mode_threshold_e": "feature", "norm": 2}
    if name == "single_lightgcn":
        cfg["mode_threshold_e"] = "field"
    cls = pkg.LightGCN if name == "lightgcn" else pkg.SingleLightGCN
    model = cls(nu, ni, num_layers=2, hidden_size=16, embedding_config=cfg)
    model.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
    model = model.to(DEV).train()
    from functools import partial
    for tname, table in model.get_embs():
        table.get_weight = partial(type(table).get_weight, table, mask_d=g.t(f"mask/{tname}").to(DEV))
    ue, ie = model(adj.to(DEV))
    users, pos, neg = (g.t(k).to(DEV) for k in ("users", "pos", "neg"))
    from oracle import reference_ops as ro
    loss = ro.bpr_loss(ue[users], ie[pos], ie[neg])
    loss_s = sum(t.get_l_s() for _, t in model.get_embs())
    (loss + 0.01 * loss_s).backward()
    _close(ue, g["user_emb"], "user_emb")
    _close(ie, g["item_emb"], "item_emb")
    _close(loss, g["bpr"], "bpr")
    for k, p in model.named_parameters():
        _close(p.grad, g["grad/" + k], k, rtol=1e-4, atol=1e-6)


def test_neumf_eval_with_assigned_cache_matches_reference():
    g = load_golden("optembed_cf_neumf")
    model = NeuMF(13, 17, emb_size=16, hidden_sizes=[16, 8], p_dropout=0,
                  embedding_config={"name": "optembed_d", "mode_threshold_d": "feature"})
    model.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
    model = model.to(DEV).eval()
    for tname, table in (("gmf_user", model._gmf.user_emb_table), ("gmf_item", model._gmf.item_emb_table),
                         ("mlp_user", model._mlp.user_emb_table), ("mlp_item", model._mlp.item_emb_table)):
        table._cur_weight = table.get_weight(g.t(f"mask/{tname}").to(DEV))
    y = model(g.t("users").to(DEV), g.t("items").to(DEV))
    y.sum().backward()
    _close(y, g["y"], "y")
    for k, p in model.named_parameters():
        if "grad/" + k in g:
            _close(p.grad, g["grad/" + k], k, rtol=1e-4, atol=1e-6)
    assert model._gmf.user_emb_table._cur_weight is None           # the backward through the table cleared its cache


def test_backward_is_bit_identical_across_runs():
    torch.manual_seed(3)
    for mode_e in ("field", "feature"):
        emb = get_embedding({"name": "optembed", "mode_threshold_e": mode_e, "mode_threshold_d": "feature", "norm": 2},
                            [20000, 11000], 64).to(DEV).train()
        with torch.no_grad():
            emb._mask_e_module._t_param.fill_(0.3)
        k = torch.randint(0, 64, (31000,), device=DEV)
        G = torch.randn(31000, 64, device=DEV)
        grads = []
        for _ in range(2):
            emb.zero_grad()
            (emb.get_weight(k) * G).sum().backward()
            grads.append((emb._weight.grad.clone(), emb._mask_e_module._t_param.grad.clone()))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def _widths(w):
    """last kept dimension per row of a table of ones (-1: nothing kept), and whether every row is a prefix."""
    nz = (w != 0)
    k = nz.sum(1) - 1
    prefix = torch.equal(nz, torch.arange(w.shape[1], device=w.device).unsqueeze(0) <= k.unsqueeze(1))
    return k, prefix


def test_device_draws_are_prefix_masks_fresh_per_call_and_one_per_field():
    emb = get_embedding({"name": "optembed_d", "mode_threshold_d": "feature", "target_sparsity": 0.7}, [3000, 5000],
                        64).to(DEV).train()
    with torch.no_grad():
        emb._weight.fill_(1.0)
    k1, p1 = _widths(emb.get_weight())
    k2, p2 = _widths(emb.get_weight())
    assert p1 and p2 and int(k1.min()) >= 0 and int(k2.min()) >= 0           # dimension 0 always kept
    assert not torch.equal(k1, k2)                                          # a fresh draw on every call
    field = get_embedding({"name": "optembed_d", "mode_threshold_d": "field"}, [300, 500, 7], 16).to(DEV).train()
    with torch.no_grad():
        field._weight.fill_(1.0)
    seen = set()
    for _ in range(8):
        k, p = _widths(field.get_weight())
        assert p
        parts = torch.split(k, [300, 500, 7])
        assert all(int(x.min()) == int(x.max()) for x in parts)              # one width per field
        seen.add(tuple(int(x[0]) for x in parts))
    assert len(seen) > 1


@pytest.mark.parametrize("ts,method", [(None, 1), (0.7, 2), (0.8, 1), (0.7, 1), (0.5, 1)])
def test_draw_histogram_matches_the_law(ts, method):
    torch.manual_seed(11)
    D, n = 64, 400000
    k = cf.draw_widths(n, D, ts, method, DEV).cpu()
    law, hi, cdf = cf.draw_law(ts, D, method)
    p = np.diff(np.concatenate([[0.0], cdf])) if law == 1 else np.where(np.arange(D) < hi, 1.0 / hi, 0.0)
    freq = np.bincount(k.numpy(), minlength=D)[:D] / n
    assert int(k.min()) >= 0 and int(k.max()) < D
    sigma = np.sqrt(p * (1 - p) / n)
    assert np.all(np.abs(freq - p) <= 5 * sigma + 1e-12), np.max(np.abs(freq - p) / (sigma + 1e-12))
    mean_width = float((k + 1).double().mean())
    if law == 1:
        want = float(cf.get_expected_hidden_size(cf.find_alpha(ts, D), D))
    else:
        want = (hi + 1) / 2
    assert abs(mean_width - want) < 5 * float(np.sqrt(((np.arange(D) + 1) ** 2 * p).sum() - want ** 2) / np.sqrt(n)) + 1e-6


def test_draws_reproducible_under_manual_seed():
    torch.manual_seed(123)
    a = cf.draw_widths(1000, 64, None, 0, DEV).cpu()
    torch.manual_seed(124)
    cf.draw_widths(1000, 64, None, 0, DEV)
    torch.manual_seed(123)
    b = cf.draw_widths(1000, 64, None, 0, DEV).cpu()
    c = cf.draw_widths(1000, 64, None, 0, DEV).cpu()
    assert torch.equal(a, b) and not torch.equal(b, c)


def test_graph_replay_draws_a_fresh_mask():
    emb = get_embedding({"name": "optembed", "mode_threshold_d": "feature", "target_sparsity": 0.8}, 4096,
                        64).to(DEV).train()
    for _ in range(2):
        emb.get_weight()                    # warm up: seed word, error word
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = emb.get_weight().detach()
    graph.replay()
    first = out.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(first, out)


class _ToyCF:
    def __init__(self, num_user=60, num_item=90, seed=0):
        gen = torch.Generator().manual_seed(seed)
        self.num_users, self.num_items = num_user, num_item
        self.graph = {u: sorted(set(torch.randint(0, num_item, (int(torch.randint(2, 12, (1,), generator=gen)),),
                                                  generator=gen).tolist())) for u in range(num_user)}
        self.adj = calculate_sparse_graph_adj_norm(self.graph, num_item, num_user)

    def get_norm_adj(self):
        return self.adj

    def get_graph(self):
        return self.graph


class _Loader(list):
    dataset = None


def test_train_epoch_optembed_runs_and_reports_loss_s():
    ds = _ToyCF()
    torch.manual_seed(4)
    model = pkg.LightGCN(ds.num_users, ds.num_items, num_layers=2, hidden_size=16,
                         embedding_config={"name": "optembed", "mode_threshold_d": "feature",
                                           "target_sparsity": 0.7}).to(DEV)
    gen = torch.Generator().manual_seed(5)
    data = _Loader([(torch.randint(0, ds.num_users, (32,), generator=gen), torch.randint(0, ds.num_items, (32,), generator=gen),
                     torch.randint(0, ds.num_items, (32,), generator=gen)) for _ in range(3)])
    data.dataset = ds
    t_params = [t._mask_e_module._t_param for _, t in model.get_embs()]
    others = [p for n, p in model.named_parameters() if "_t_param" not in n]
    opts = [torch.optim.Adam(others, lr=1e-2), torch.optim.SGD(t_params, lr=0.0)]       # thresholds frozen: loss_s fixed
    res = trainer.train_epoch_optembed(data, model, opts, device=DEV, log_step=1, weight_decay=1e-3, info_nce_weight=0.1,
                                       alpha=0.01)
    assert set(res) == {"loss", "reg_loss", "rec_loss", "cl_loss", "loss_s", "sparsity", "n_params"}
    assert all(np.isfinite(v) for v in res.values())
    want = sum(float(torch.exp(-t).sum()) for t in t_params)
    assert res["loss_s"] == pytest.approx(want, rel=1e-6)


def test_evol_search_meets_the_target_and_never_loses_its_best():
    ds = _ToyCF(seed=7)
    torch.manual_seed(8)
    model = pkg.LightGCN(ds.num_users, ds.num_items, num_layers=2, hidden_size=64,
                         embedding_config={"name": "optembed_d", "mode_threshold_d": "feature"}).to(DEV)
    users = torch.arange(ds.num_users)
    truth = [ds.graph[u][:2] for u in range(ds.num_users)]
    val = [(users[s:s + 20], truth[s:s + 20]) for s in range(0, ds.num_users, 20)]
    hist = []
    item_mask, user_mask, best = cf.evol_search_lightgcn(model, 3, 4, 2, 2, 0.3, 3, val, ds, target_sparsity=0.7, method=1,
                                                         history=hist)
    assert item_mask.shape == (ds.num_items,) and user_mask.shape == (ds.num_users,)
    assert cf.candidate_sparsity(cf.Candidate(item_mask, user_mask), 64) >= 0.7
    assert len(hist) == 3 and all(b >= a for a, b in zip(hist, hist[1:])) and float(best) == hist[-1]


@pytest.mark.parametrize("norm,mode_e", [(1, "feature"), (2, "field")])
def test_yelp2018_shape_against_float64(norm, mode_e):
    torch.manual_seed(9)
    N, D = 38048, 64
    emb = get_embedding({"name": "optembed", "norm": norm, "mode_threshold_e": mode_e, "mode_threshold_d": "feature"},
                        N, D).to(DEV).train()
    W = emb._weight.detach().double()
    nrm = W.abs().sum(1) if norm == 1 else W.norm(2, dim=1)
    with torch.no_grad():
        t = emb._mask_e_module._t_param
        t.copy_((nrm + (torch.rand(N, device=DEV, dtype=torch.float64) - 0.5) * 0.8).float() if mode_e == "feature"
                else nrm.median().float().view(1))
    k = torch.randint(0, D, (N,), device=DEV)
    G = torch.randn(N, D, device=DEV)
    out = emb.get_weight(k)
    (out * G).sum().backward()
    tt = t.detach().double()
    tr = tt if mode_e == "feature" else tt.expand(N)
    u = nrm - tr
    s = (u > 0).double()
    md = (torch.arange(D, device=DEV).unsqueeze(0) <= k.unsqueeze(1)).double()
    clear = u.abs() > 1e-4                      # rows whose step the fp32 norm could put on the other side
    ref = W * s.unsqueeze(1) * md
    _eq(out[clear], ref[clear].float().cpu(), "forward")
    Gm = G.double() * md
    c = (Gm * W).sum(1)
    a = torch.where(u.abs() > 1, 0.0, torch.where(u.abs() > 0.4, 0.4, 2 - 4 * u.abs()))
    dn = torch.sign(W) if norm == 1 else W / nrm.unsqueeze(1)
    dW = Gm * s.unsqueeze(1) + (c * a).unsqueeze(1) * dn
    _close(emb._weight.grad[clear], dW[clear].cpu(), "dW", rtol=1e-4, atol=1e-5)
    dt = -(c * a)
    dt = dt if mode_e == "feature" else dt.sum().view(1)
    _close(t.grad, dt.cpu(), "dt", rtol=1e-4, atol=1e-3 if mode_e == "field" else 1e-5)

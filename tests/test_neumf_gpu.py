"""GPU: NeuMF forward / losses / gradients against the reference's (tests/golden/neumf_*.npz), the gradient forms,
graph capture, and the all-items scoring kernel against a float64 restatement of the reference formula."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import neumf, trainer
from recsys_benchmark_amd.neumf import ModelFlag, NeuMF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(golden, cfg=None, hidden=None):
    g = load_golden("neumf_model")
    m = NeuMF(int(g["num_user"]), int(g["num_item"]), emb_size=int(g["emb_size"]),
              hidden_sizes=hidden or [int(h) for h in g["hidden"]], p_dropout=0, embedding_config=cfg)
    m.load_state_dict({k[len("param/"):]: golden.t(k) for k in golden if k.startswith("param/")})
    return m.to(DEV)


def _dense(t):
    return (t.to_dense() if t.is_sparse else t).cpu()


@pytest.mark.parametrize("name,cfg", [("neumf_model", None), ("neumf_qr", {"name": "qr", "operation": "mult", "divider": 3})])
def test_forward_matches_reference_under_every_flag(name, cfg):
    g = load_golden(name)
    model = _model(g, cfg).eval()
    with torch.no_grad():
        for flag in (ModelFlag.MLP, ModelFlag.GMF, ModelFlag.NMF):
            model.flag = flag
            for tag in ("1d", "2d"):
                out = model(g.t(f"users_{tag}").to(DEV), g.t(f"items_{tag}").to(DEV))
                torch.testing.assert_close(out.cpu(), g.t(f"out_{tag}/{flag.name}"), rtol=1e-5, atol=1e-6)
    pkg.check_index_errors()


def _train_and_compare(g, model, prefix=""):
    neg = g.t(prefix + "neg")
    negs = list(neg.to(DEV)) if neg.shape[0] > 1 else neg[0].to(DEV)
    model.zero_grad(set_to_none=True)
    loss, rec, reg = trainer.nmf_step_losses(model, g.t(prefix + "users").to(DEV), g.t(prefix + "pos").to(DEV), negs,
                                             float(g[prefix + "wd"]))
    loss.backward()
    torch.testing.assert_close(rec.detach().cpu(), g.t(prefix + "rec_loss"), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(reg.detach().cpu(), g.t(prefix + "reg_loss").float(), rtol=1e-5, atol=1e-6)
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    want = g.group(prefix + "grad/")
    assert set(grads) == set(want)
    for k, v in want.items():
        torch.testing.assert_close(_dense(grads[k]), v, rtol=1e-4, atol=1e-6, msg=k)
    pkg.check_index_errors()
    return grads


@pytest.mark.parametrize("n_neg", [1, 3])
@pytest.mark.parametrize("sparse", [False, True])
def test_losses_and_every_gradient_match_reference(n_neg, sparse):
    g = load_golden(f"neumf_train_neg{n_neg}")
    model = _model(g, {"name": "vanilla", "sparse": True} if sparse else None)
    assert model._plain_tables()
    grads = _train_and_compare(g, model)
    tbl = grads["_gmf.user_emb_table._emb_module.weight"]
    assert tbl.is_sparse == sparse                    # row form for sparse=True tables, dense otherwise


def test_compressed_tables_compose_their_own_forwards():
    g = load_golden("neumf_qr")
    model = _model(g, {"name": "qr", "operation": "mult", "divider": 3})
    assert not model._plain_tables()
    _train_and_compare(g, model, "train/")


def test_deterministic_mode_is_bit_reproducible_and_matches_reference():
    g = load_golden("neumf_train_neg3")
    pkg.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            model = _model(g)
            runs.append({k: _dense(v).clone() for k, v in _train_and_compare(g, model).items()})
    finally:
        pkg.use_deterministic_algorithms(False)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_graph_replay_equals_eager():
    g = load_golden("neumf_train_neg3")
    model = _model(g)
    users, pos, neg = g.t("users").to(DEV), g.t("pos").to(DEV), list(g.t("neg").to(DEV))

    def step():
        for p in model.parameters():
            p.grad = None
        loss, _, _ = trainer.nmf_step_losses(model, users, pos, neg, 1e-2)
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager_loss = step().clone()
        eager = {k: p.grad.clone() for k, p in model.named_parameters()}
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    for p in model.parameters():
        p.grad = None
    with torch.cuda.graph(graph):
        static_loss = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_loss, eager_loss)
    for k, p in model.named_parameters():
        torch.testing.assert_close(p.grad, eager[k], rtol=1e-6, atol=1e-7, msg=k)


def _scores64(model, users):
    """model(users x all items) restated in float64 from the parameters (src/models/mlp.py:82-101, 255-274, 318-344)."""
    p = {k: v.detach().double() for k, v in model.state_dict().items()}
    gu = p["_gmf.user_emb_table._emb_module.weight"][users]
    gi = p["_gmf.item_emb_table._emb_module.weight"]
    mu = p["_mlp.user_emb_table._emb_module.weight"][users]
    mi = p["_mlp.item_emb_table._emb_module.weight"]
    out = (gu * p["_gmf.gmf_fc.weight"].view(-1)) @ gi.T + p["_gmf.gmf_fc.bias"]
    lins = [i for i, m in enumerate(model._mlp.mlp) if isinstance(m, torch.nn.Linear)]
    W1, b1 = p[f"_mlp.mlp.{lins[0]}.weight"], p[f"_mlp.mlp.{lins[0]}.bias"]
    D = gu.shape[1]
    x = torch.relu((mu @ W1[:, :D].T)[:, None, :] + (mi @ W1[:, D:].T + b1)[None, :, :])
    for i in lins[1:]:
        x = torch.relu(x @ p[f"_mlp.mlp.{i}.weight"].T + p[f"_mlp.mlp.{i}.bias"])
    return out + (x @ p["_mlp.mlp_fc.weight"].view(-1) + p["_mlp.mlp_fc.bias"])


def _topk_equal_up_to_ties(idx, s64, k, tol):
    """Every returned item's float64 score is within `tol` of the k-th best float64 score or above it."""
    kth = torch.topk(s64, k, dim=1).values[:, -1:]
    got = torch.gather(s64, 1, idx)
    assert bool((got >= kth - tol).all())
    assert all(len(set(r.tolist())) == k for r in idx)


def test_score_all_items_small_matches_float64_and_reference():
    g = load_golden("neumf_validate")
    nu, ni = int(g["num_user"]), int(g["num_item"])
    model = NeuMF(nu, ni, emb_size=16, hidden_sizes=[16, 8]).to(DEV)
    model.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
    model.eval()
    assert neumf.score_supported(model)
    users = torch.arange(nu, device=DEV)
    scores = model.score_all_items(users)
    torch.testing.assert_close(scores, _scores64(model, users).float(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(scores.cpu(), g.t("scores"), rtol=1e-5, atol=1e-5)
    for flag in (ModelFlag.GMF, ModelFlag.MLP):
        model.flag = flag
        ref = model(users.view(-1, 1).repeat(1, ni), torch.arange(ni, device=DEV).view(1, -1).repeat(nu, 1))
        torch.testing.assert_close(model.score_all_items(users), ref, rtol=1e-5, atol=1e-5)
    pkg.check_index_errors()


def test_score_composed_path_for_a_width_the_kernel_does_not_take():
    torch.manual_seed(5)
    model = NeuMF(37, 301, emb_size=16, hidden_sizes=[200, 24]).to(DEV).eval()
    assert not neumf.score_supported(model)
    users = torch.randint(0, 37, (19,), device=DEV)
    scores = model.score_all_items(users)
    torch.testing.assert_close(scores, _scores64(model, users).float(), rtol=1e-5, atol=1e-5)


def test_score_all_items_at_yelp2018_shape():
    torch.manual_seed(11)
    nu, ni = 31668, 38048
    model = NeuMF(nu, ni, emb_size=64, hidden_sizes=[64, 32, 16]).to(DEV).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    assert neumf.score_supported(model)
    users = torch.randint(0, nu, (2048,), device=DEV)
    scores = model.score_all_items(users)
    rows = torch.arange(0, 2048, 97, device=DEV)
    s64 = _scores64(model, users[rows])
    torch.testing.assert_close(scores[rows].double(), s64, rtol=1e-5, atol=2e-6)
    k = 20
    idx = torch.empty((rows.numel(), k), dtype=torch.int64, device=DEV)
    sub = scores[rows].contiguous()
    from recsys_benchmark_amd import _lib

    _lib.check(_lib.load().mi_mask_topk_rows(sub.data_ptr(), sub.stride(0), sub.shape[0], sub.shape[1], None, None, None, k,
                                             idx.data_ptr(), None, _lib.stream_ptr(sub.device)), "mi_mask_topk_rows")
    _topk_equal_up_to_ties(idx, s64, k, 1e-5)
    pkg.check_index_errors()


class _Data:
    def __init__(self, graph):
        self._g = graph

    def get_graph(self):
        return self._g


def test_validate_epoch_nmf_matches_reference():
    g = load_golden("neumf_validate")
    nu, ni = int(g["num_user"]), int(g["num_item"])
    graph = {}
    for u, i in zip(g["edge_user"].tolist(), g["edge_item"].tolist()):
        graph.setdefault(u, []).append(i)
    model = NeuMF(nu, ni, emb_size=16, hidden_sizes=[16, 8])
    model.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
    true = [[int(x) for x in r if x >= 0] for r in g["true_pad"]]
    users = torch.arange(nu)
    batches = [(users[s:s + 32], true[s:s + 32]) for s in range(0, nu, 32)]
    res = trainer.validate_epoch_nmf(_Data(graph), batches, model, device=DEV, k=int(g["k"]), metrics=["ndcg", "recall"])
    assert res["ndcg"] == pytest.approx(float(g["ndcg"]), abs=1e-6)
    assert res["recall"] == pytest.approx(float(g["recall"]), abs=1e-6)


def test_train_epoch_nmf_returns_the_reference_keys():
    g = load_golden("neumf_train_neg3")
    model = _model(g)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    batch = (g.t("users"), g.t("pos"), list(g.t("neg")))
    res = trainer.train_epoch_nmf([batch, batch], model, opt, device=DEV, log_step=1, weight_decay=1e-2)
    assert set(res) == {"loss", "rec_loss", "reg_loss"}
    assert np.isfinite(res["loss"]) and res["loss"] > 0

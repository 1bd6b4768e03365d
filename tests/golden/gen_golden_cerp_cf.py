#!/usr/bin/env python3
"""Generate the CF CERP / PEP golden vectors (tests/golden/cf_cerp_*.npz) by IMPORTING THE REFERENCE.
(The archives are named cf_cerp_*, not cerp_*: the embedding tests take every cerp_*.npz for a lookup fixture.)

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_cerp_cf.py

Same conventions as gen_golden_neumf.py: the reference's modules are imported unmodified (`loguru` replaced by a no-op
stand-in), only arrays leave this script, and the archives are written with a fixed member timestamp, so a rerun
reproduces them bit for bit.

Each archive holds ONE optimisation step at the initial parameters: the reference's epoch function is run over a
one-batch loader with a zero learning rate (its returned dictionary gives the losses and the keys), and the parameter
gradients BEFORE clipping come from the same step re-assembled from the reference's own pieces (LightGCN: the epoch
clips inside; NeuMF: `_train_step` with clip_grad_norm=0).

Threshold logits are `randn - 2`, so that pruning is active.  CPU and GPU `expf` may differ in the last bit, and an
element with |w| on the edge of sigmoid(s) would flip its mask: every case asserts | |w| - sigmoid(s) | >= 1e-4 for
all its elements and moves to the next seed until that holds; the seed used is stored in the archive (`seed`).
Seeds used: lightgcn_k1 2031, lightgcn_k3 2031, single_lightgcn_k3 2032, neumf_pep 2033, neumf_cerp 2034 — each the
first candidate tried.
"""
import inspect
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch

REF = os.environ.get("RECSYS_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "src")):
    sys.exit("set RECSYS_REFERENCE to a checkout of the reference (the directory that holds src/ and tests/assets/)")
OUT = os.path.dirname(os.path.abspath(__file__))


def _install_stubs():
    class _L:
        def __getattr__(self, k):
            return lambda *a, **kw: None

    loguru = types.ModuleType("loguru")
    loguru.logger = _L()
    loguru.Logger = _L
    sys.modules["loguru"] = loguru
    sys.modules.setdefault("lmdb", types.ModuleType("lmdb"))


_install_stubs()
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from src import losses as ref_losses  # noqa: E402
from src.graph_utils import calculate_sparse_graph_adj_norm  # noqa: E402
from src.models import get_graph_model  # noqa: E402
from src.models.embeddings import cerp_embedding_utils as ref_cerp  # noqa: E402
from src.models.mlp import NeuMF  # noqa: E402
from src.trainer import nmf as ref_nmf  # noqa: E402
from src.utils import set_seed  # noqa: E402

MARGIN = 1e-4
WD, NCE, PRUNE_W = 1e-2, 0.1, 1e-3


def save(name, **arrays):
    """np.savez_compressed, but every member stamped 1980-01-01 so that the archive bytes depend on the arrays only."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f"  wrote {name}.npz ({len(arrays)} arrays)")


def params_of(module, prefix="param/"):
    return {prefix + k: v.detach().clone() for k, v in module.state_dict().items() if isinstance(v, torch.Tensor)}


def grads_of(module, prefix="grad/"):
    return {prefix + k: p.grad.detach().clone() for k, p in module.named_parameters() if p.grad is not None}


def argnames(fn):
    return np.array(list(inspect.signature(fn).parameters))


def thresholds_with_margin(model, seed):
    """Every threshold logit of the model's tables := randn - 2 (generator `seed`); True when no element of any table sits
    within MARGIN of its threshold."""
    gen = torch.Generator().manual_seed(seed)
    ok = True
    with torch.no_grad():
        for _, table in model.get_embs():
            pairs = ([(table.p_weight, table.p_threshold), (table.q_weight, table.q_threshold)] if hasattr(table, "p_weight")
                     else [(table.emb.weight, table.s)])
            for w, s in pairs:
                s.copy_(torch.randn(s.shape, generator=gen) - 2)
                ok = ok and bool(((w.abs() - torch.sigmoid(s)).abs() >= MARGIN).all())
    return ok


def build_with_margin(build, seed):
    """build(seed) -> model, then the thresholds; the first seed from `seed` upwards that keeps the margin."""
    for s in range(seed, seed + 50):
        model = build(s)
        if thresholds_with_margin(model, s):
            print(f"  seed {s}")
            return model, s
    raise SystemExit("no seed in range keeps the threshold margin")


def load_cf_graph(path):
    graph = {}
    num_item = 0
    with open(path) as fin:
        for line in fin.readlines():
            info = line.strip().split()
            items = [int(i) for i in info[1:]]
            if items:
                graph[int(info[0])] = items
                num_item = max(*items, num_item)
    return graph, num_item + 1


class _Data:
    def __init__(self, adj):
        self._adj = adj

    def get_norm_adj(self):
        return self._adj


class _Loader(list):
    """A one-batch loader with the `dataset.get_norm_adj()` the reference's epoch asks for."""

    def __init__(self, batches, adj=None):
        super().__init__(batches)
        self.dataset = _Data(adj)


def batch_ids(gen, num_user, num_item, B, K):
    users = torch.randint(0, num_user // 3, (B,), generator=gen)          # a third of the users: repeats within the batch
    pos = torch.randint(0, num_item // 2, (B,), generator=gen)
    negs = [torch.randint(0, num_item, (B,), generator=gen) for _ in range(K)]
    return users, pos, negs


def gen_lightgcn():
    """One step of cerp_embedding_utils.train_epoch_cerp on LightGCN (D = 16, bucket 26: 77 users / 102 items, neither a
    multiple of the bucket, both last quotient rows short) and SingleLightGCN (D = 8, bucket 60 over the 179 rows)."""
    graph, num_item = load_cf_graph(os.path.join(REF, "tests/assets/sample_cf.txt"))
    num_user = len(graph)
    adj = calculate_sparse_graph_adj_norm(graph, num_item, num_user)
    for mname, D, bucket, K, seed in (("lightgcn", 16, 26, 1, 2031), ("lightgcn", 16, 26, 3, 2031),
                                      ("single-lightgcn", 8, 60, 3, 2032)):
        def build(s):
            set_seed(s)
            return get_graph_model(num_user, num_item, {"name": mname, "num_layers": 2, "hidden_size": D,
                                                        "embedding_config": {"name": "cerp", "bucket_size": bucket}})

        model, seed = build_with_margin(build, seed)
        gen = torch.Generator().manual_seed(seed + 1000)
        users, pos, negs = batch_ids(gen, num_user, num_item, 24, K)
        neg_batch = negs if K > 1 else negs[0]
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        res = ref_cerp.train_epoch_cerp(_Loader([(users, pos, neg_batch)], adj), model, opt, device="cpu", log_step=1,
                                        weight_decay=WD, info_nce_weight=NCE, prune_loss_weight=PRUNE_W, target_sparsity=2.0)
        # the same step from the reference's pieces, for the gradients before clipping
        model.zero_grad()
        all_user, all_item = model(adj)
        neg2d = torch.stack(negs, dim=1)
        rec = ref_losses.bpr_loss_multi(all_user[users], all_item[pos], all_item[neg2d])
        prune, reg = ref_cerp.get_prune_and_reg_loss_lightgcn(model, users, pos, neg2d.flatten())
        view = torch.cat([all_user[torch.unique(users)], all_item[torch.unique(pos)]], 0)
        cl = ref_losses.info_nce(view, view, 0.2) * NCE
        loss = rec + WD * reg + cl + prune * PRUNE_W
        loss.backward()
        for key, val in (("loss", loss), ("rec_loss", rec), ("reg_loss", reg), ("cl_loss", cl), ("prune_loss", prune)):
            assert abs(res[key] - float(val)) <= 1e-6 * max(1.0, abs(float(val))), (key, res[key], float(val))
        grad_norm = torch.sqrt(sum((p.grad ** 2).sum() for p in model.parameters()))
        save(f"cf_cerp_{mname.replace('-', '_')}_k{K}", seed=np.array(seed), users=users, pos=pos, neg=neg2d,
             hidden_size=np.array(D), bucket_size=np.array(bucket), num_layers=np.array(2), weight_decay=np.array(WD),
             info_nce_weight=np.array(NCE), prune_loss_weight=np.array(PRUNE_W),
             keys=np.array(list(res.keys())), argnames=argnames(ref_cerp.train_epoch_cerp),
             loss=loss, rec_loss=rec, reg_loss=reg, cl_loss=cl, prune_loss=prune, sparsity=np.array(res["sparsity"]),
             num_params=np.array(res["num_params"]), grad_norm=grad_norm, user_emb=all_user, item_emb=all_item,
             **params_of(model), **grads_of(model))


def gen_neumf():
    """One step of src/trainer/nmf.py train_epoch_pep (PEP tables, K = 1) and train_epoch_cerp (CERP tables, bucket 5 over
    13 users / 17 items, K = 3) on NeuMF."""
    NU, NI, EMB, HIDDEN = 13, 17, 16, [16, 8]
    with tempfile.TemporaryDirectory() as tmp:
        for tag, cfg, K, seed in (("pep", {"name": "pep", "checkpoint_weight_dir": tmp}, 1, 2033),
                                  ("cerp", {"name": "cerp", "bucket_size": 5}, 3, 2034)):
            def build(s):
                set_seed(s)
                return NeuMF(NU, NI, emb_size=EMB, hidden_sizes=HIDDEN, p_dropout=0, embedding_config=dict(cfg))

            model, seed = build_with_margin(build, seed)
            gen = torch.Generator().manual_seed(seed + 1000)
            users, pos, negs = batch_ids(gen, NU, NI, 12, K)
            neg_batch = negs if K > 1 else negs[0]
            opt = torch.optim.SGD(model.parameters(), lr=0.0)
            loader = _Loader([(users, pos, neg_batch)])
            if tag == "pep":
                res = ref_nmf.train_epoch_pep(loader, model, opt, device="cpu", log_step=1, weight_decay=WD,
                                              target_sparsity=2.0)
                parts = ref_nmf._train_step((users, pos, neg_batch), model, opt, "cpu", WD)
                names = ("loss", "rec_loss", "reg_loss")
                fn = ref_nmf.train_epoch_pep
            else:
                res = ref_nmf.train_epoch_cerp(loader, model, opt, device="cpu", log_step=1, weight_decay=WD,
                                               target_sparsity=2.0, prune_loss_weight=PRUNE_W)
                parts = ref_nmf._train_step((users, pos, neg_batch), model, opt, "cpu", WD, PRUNE_W, 0)
                names = ("loss", "rec_loss", "reg_loss", "prune_loss")
                fn = ref_nmf.train_epoch_cerp
            for key, val in zip(names, parts):
                assert abs(res[key] - float(val)) <= 1e-6 * max(1.0, abs(float(val))), (key, res[key], float(val))
            grad_norm = torch.sqrt(sum((p.grad ** 2).sum() for p in model.parameters() if p.grad is not None))
            save(f"cf_cerp_neumf_{tag}", seed=np.array(seed), users=users, pos=pos, neg=torch.stack(negs, dim=1),
                 num_user=np.array(NU), num_item=np.array(NI), emb_size=np.array(EMB), hidden=np.array(HIDDEN),
                 weight_decay=np.array(WD), prune_loss_weight=np.array(PRUNE_W), keys=np.array(list(res.keys())),
                 argnames=argnames(fn), sparsity=np.array(res["sparsity"]), num_params=np.array(res["num_params"]),
                 grad_norm=grad_norm, **{k: v.detach() for k, v in zip(names, parts)}, **params_of(model), **grads_of(model))


if __name__ == "__main__":
    torch.set_num_threads(1)
    which = sys.argv[1:] or ["lightgcn", "neumf"]
    for w in which:
        print(f"[{w}]")
        globals()[f"gen_{w}"]()

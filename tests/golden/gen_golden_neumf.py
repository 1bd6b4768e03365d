#!/usr/bin/env python3
"""Generate the NeuMF golden vectors (tests/golden/neumf_*.npz) by IMPORTING THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_neumf.py

Same conventions as gen_golden.py: the reference's modules are imported unmodified (`loguru` replaced by a no-op
stand-in), only arrays leave this script.  The archives are written with a fixed member timestamp, so a rerun
reproduces them bit for bit.
"""
import io
import os
import sys
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

from src.models.mlp import ModelFlag, NeuMF, get_sparsity_and_param  # noqa: E402
from src.trainer import nmf as ref_nmf  # noqa: E402
from src.utils import set_seed  # noqa: E402


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


NU, NI, EMB, HIDDEN = 13, 17, 16, [16, 8]


def build(cfg=None):
    set_seed(2023)
    return NeuMF(NU, NI, emb_size=EMB, hidden_sizes=HIDDEN, p_dropout=0, embedding_config=cfg)


def forward_cases(model, gen):
    out = {}
    x1u, x1i = torch.randint(0, NU, (23,), generator=gen), torch.randint(0, NI, (23,), generator=gen)
    x2u, x2i = torch.randint(0, NU, (5, 7), generator=gen), torch.randint(0, NI, (5, 7), generator=gen)
    out.update(users_1d=x1u, items_1d=x1i, users_2d=x2u, items_2d=x2i)
    model.eval()
    with torch.no_grad():
        for flag in (ModelFlag.MLP, ModelFlag.GMF, ModelFlag.NMF):
            model.flag = flag
            out[f"out_1d/{flag.name}"] = model(x1u, x1i)
            out[f"out_2d/{flag.name}"] = model(x2u, x2i)
    model.flag = ModelFlag.NMF
    model.train()
    return out


def train_case(model, gen, n_neg, wd):
    B = 12
    users = torch.randint(0, NU // 2, (B,), generator=gen)           # half the users: repeats within the batch
    pos = torch.randint(0, NI // 2, (B,), generator=gen)
    negs = [torch.randint(0, NI, (B,), generator=gen) for _ in range(n_neg)]
    model.train()
    model.zero_grad()
    neg = negs if n_neg > 1 else negs[0]
    n_repeat = len(negs)
    negc = torch.cat(negs)
    y_hat = model(users.repeat(n_repeat + 1), torch.cat([pos, negc]))
    rec = ref_nmf._log_loss(y_hat[:B], y_hat[B:])
    reg = model.get_reg_loss(users, pos, negc)
    (rec + wd * reg).backward()
    del neg
    return dict(users=users, pos=pos, neg=torch.stack(negs), wd=np.array(wd), y_hat=y_hat, rec_loss=rec, reg_loss=reg,
                **grads_of(model))


def gen_model():
    gen = torch.Generator().manual_seed(41)
    model = build()
    keys = list(model.state_dict().keys())
    arrays = dict(keys=np.array(keys), num_user=np.array(NU), num_item=np.array(NI), emb_size=np.array(EMB),
                  hidden=np.array(HIDDEN), **params_of(model))
    sp, n = get_sparsity_and_param(model)
    arrays.update(sparsity=np.array(sp), n_params=np.array(n))
    model.flag = ModelFlag.GMF
    sp_g, n_g = get_sparsity_and_param(model)
    arrays.update(sparsity_gmf=np.array(sp_g), n_params_gmf=np.array(n_g))
    model.flag = ModelFlag.NMF
    arrays.update(forward_cases(model, gen))
    save("neumf_model", **arrays)
    for n_neg in (1, 3):
        model = build()
        save(f"neumf_train_neg{n_neg}", **train_case(model, gen, n_neg, 1e-2), **params_of(model))
    model = build({"name": "qr", "operation": "mult", "divider": 3})
    arrays = dict(keys=np.array(list(model.state_dict().keys())), **params_of(model), **forward_cases(model, gen))
    arrays.update({"train/" + k: v for k, v in train_case(model, gen, 3, 1e-2).items()})
    save("neumf_qr", **arrays)


class _TrainData:
    def __init__(self, graph):
        self._graph = graph

    def get_graph(self):
        return self._graph


def gen_validate():
    gen = torch.Generator().manual_seed(43)
    graph = {}
    num_item = 0
    with open(os.path.join(REF, "tests/assets/sample_cf.txt")) as fin:
        for line in fin.readlines():
            info = line.strip().split()
            items = [int(i) for i in info[1:]]
            if not items:
                continue
            graph[int(info[0])] = items
            num_item = max(*items, num_item)
    num_item += 1
    num_user = len(graph)
    set_seed(2023)
    model = NeuMF(num_user, num_item, emb_size=16, hidden_sizes=[16, 8], p_dropout=0)
    with torch.no_grad():            # move the biases away from zero so that every term shows in the scores
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    users = torch.arange(num_user)
    true = [torch.randperm(num_item, generator=gen)[:int(m)].tolist()
            for m in torch.randint(1, 6, (num_user,), generator=gen)]
    batches = [(users[s:s + 32], true[s:s + 32]) for s in range(0, num_user, 32)]
    k = 10
    res = ref_nmf.validate_epoch(_TrainData(graph), batches, model, device="cpu", k=k, metrics=["ndcg", "recall"])
    model.eval()
    with torch.no_grad():
        scores = model(users.unsqueeze(1).repeat(1, num_item), torch.arange(num_item).unsqueeze(0).repeat(num_user, 1))
    eu, ei = [], []
    for u, items in graph.items():
        eu.extend([u] * len(items))
        ei.extend(items)
    true_pad = torch.full((num_user, max(len(t) for t in true)), -1, dtype=torch.int64)
    for i, t in enumerate(true):
        true_pad[i, :len(t)] = torch.tensor(t)
    save("neumf_validate", edge_user=np.array(eu), edge_item=np.array(ei), num_user=np.array(num_user),
         num_item=np.array(num_item), true_pad=true_pad, k=np.array(k), scores=scores, ndcg=np.array(res["ndcg"]),
         recall=np.array(res["recall"]), **params_of(model))


if __name__ == "__main__":
    torch.set_num_threads(1)
    which = sys.argv[1:] or ["model", "validate"]
    for w in which:
        print(f"[{w}]")
        globals()[f"gen_{w}"]()

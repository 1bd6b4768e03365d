#!/usr/bin/env python3
"""Generate the CF OptEmbed golden vectors (tests/golden/optembed_cf_*.npz) by IMPORTING THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_optembed_cf.py

Same conventions as gen_golden_neumf.py: the reference's modules are imported unmodified (`loguru` replaced by a no-op
stand-in), only arrays leave this script, every dimension mask is given explicitly (no draws), and the archives are
written with a fixed member timestamp, so a rerun reproduces them bit for bit.
"""
import io
import os
import sys
import types
import zipfile
from functools import partial

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
from src.models.embeddings import get_embedding  # noqa: E402
from src.models.embeddings import optembed_utils as ou  # noqa: E402
from src.models.mlp import NeuMF  # noqa: E402
from src.utils import set_seed  # noqa: E402

torch.use_deterministic_algorithms(True)


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


DIMS = [7, 9]
# (case name, norm, mode_threshold_e, mode_threshold_d, t_init (None: "optembed_d"), hidden size)
CASES = [
    ("l1_field_field", 1, "field", "field", 0.0, 8),
    ("l2_feature_feature", 2, "feature", "feature", 0.0, 8),
    ("l1_feature_field", 1, "feature", "field", 0.0, 8),
    ("l2_field_feature_d6", 2, "field", "feature", 0.0, 6),
    ("d_only", 1, "field", "feature", None, 8),
]


def set_thresholds(emb, gen):
    """Thresholds spread around the row norms, so that some rows are cut and some sit inside BinaryStep's surrogate:
    per row, the norm plus uniform noise of +-0.4; per field, the median norm of the field."""
    if emb._t_init is None:
        return
    m = emb._mask_e_module
    norms = torch.norm(emb._weight.detach(), m._norm, dim=1)
    with torch.no_grad():
        if m.mode_threshold_e == "feature":
            m._t_param.copy_(norms + (torch.rand(norms.shape, generator=gen) - 0.5) * 0.8)
        else:
            off = 0
            for f, n in enumerate(m._field_dims.tolist()):
                m._t_param[f] = norms[off:off + n].median()
                off += n


def gen_tables():
    gen = torch.Generator().manual_seed(97)
    for name, norm, me, md, t_init, D in CASES:
        set_seed(2024)
        cfg = {"name": "optembed" if t_init is not None else "optembed_d", "norm": norm, "mode_threshold_e": me,
               "mode_threshold_d": md}
        emb = get_embedding(cfg, DIMS, D)
        set_thresholds(emb, gen)
        N = sum(DIMS)
        arrays = dict(keys=np.array(list(emb.state_dict().keys())), norm=np.array(norm), mode_e=np.array(me),
                      mode_d=np.array(md), has_t=np.array(t_init is not None), hidden=np.array(D), dims=np.array(DIMS),
                      **params_of(emb))
        g = torch.randn(N, D, generator=gen)
        row_mask = torch.randint(0, D, (N,), generator=gen)
        field_mask = torch.randint(0, D, (len(DIMS),), generator=gen)
        bool_mask = torch.rand(N, D, generator=gen) < 0.6
        arrays.update(g=g, row_mask=row_mask, field_mask=field_mask, bool_mask=bool_mask)

        def run(tag, train, mask):
            emb.train(train)
            emb.zero_grad()
            w = emb.get_weight(mask)
            (w * g).sum().backward()
            arrays[f"{tag}/out"] = w
            arrays.update(grads_of(emb, f"{tag}/grad/"))

        run("train_rows", True, row_mask)
        run("train_bool", True, bool_mask)
        run("eval_none", False, None)
        run("eval_int", False, field_mask if md == "field" else row_mask)
        # forward(x, mask_d) in training (a lookup of the masked table) and the eval cache
        x = torch.randint(0, N, (5, 3), generator=gen)
        emb.train()
        arrays.update(x=x, fwd_train=emb(x, row_mask))
        emb.eval()
        emb._cur_weight = None
        arrays["fwd_eval"] = emb(x, field_mask if md == "field" else row_mask)
        arrays["fwd_eval_cached"] = emb(x)            # the cache made by the first eval forward
        arrays["l_s"] = emb.get_l_s()
        sp, n = emb.get_sparsity(True)
        arrays.update(sparsity=np.array(sp), n_params=np.array(n))
        save(f"optembed_cf_{name}", **arrays)


def gen_retrain():
    gen = torch.Generator().manual_seed(98)
    for md in ("feature", "field"):
        set_seed(2025)
        D = 8
        emb = get_embedding({"name": "optembed_d_retrain", "mode_threshold_d": md}, DIMS, D)
        N = sum(DIMS)
        mask_d = torch.randint(0, D, (N if md == "feature" else len(DIMS),), generator=gen)
        mask_e = (torch.rand(N, generator=gen) < 0.7).float()
        mask = emb.init_mask(mask_e, mask_d)
        g = torch.randn(N, D, generator=gen)
        emb.train()
        w = emb.get_weight()
        (w * g).sum().backward()
        save(f"optembed_cf_retrain_{md}", keys=np.array(list(emb.state_dict().keys())), mask_d=mask_d, mask_e=mask_e,
             mask=mask, out=w, g=g, n_params=np.array(emb.get_num_params()), sparsity=np.array(emb.get_sparsity()),
             **params_of(emb), **grads_of(emb))


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


def gen_lightgcn():
    """LightGCN (L = 2) on 'optembed' tables and SingleLightGCN on an 'optembed' table with per-field thresholds, in
    training with explicit per-row widths hooked into get_weight (as the reference's search does)."""
    gen = torch.Generator().manual_seed(99)
    graph, num_item = load_cf_graph(os.path.join(REF, "tests/assets/sample_cf.txt"))
    num_user = len(graph)
    adj = calculate_sparse_graph_adj_norm(graph, num_item, num_user)
    B, D = 16, 16
    users = torch.randint(0, num_user, (B,), generator=gen)
    pos = torch.randint(0, num_item, (B,), generator=gen)
    neg = torch.randint(0, num_item, (B,), generator=gen)
    cfg = {"name": "optembed", "mode_threshold_d": "feature", "mode_threshold_e": "feature", "norm": 2}
    for mname in ("lightgcn", "single-lightgcn"):
        set_seed(2026)
        c = dict(cfg, mode_threshold_e="field") if mname == "single-lightgcn" else cfg
        model = get_graph_model(num_user, num_item, {"name": mname, "num_layers": 2, "hidden_size": D,
                                                     "embedding_config": c})
        arrays = dict(users=users, pos=pos, neg=neg)
        for tname, table in model.get_embs():
            set_thresholds(table, gen)
            mask = torch.randint(0, D, (table._num_item,), generator=gen)
            arrays[f"mask/{tname}"] = mask
            table.get_weight = partial(table.get_weight, mask_d=mask)
        model.train()
        ue, ie = model(adj)
        loss = ref_losses.bpr_loss(ue[users], ie[pos], ie[neg])
        loss_s = sum(t.get_l_s() for _, t in model.get_embs())
        (loss + 0.01 * loss_s).backward()
        for _, table in model.get_embs():
            del table.get_weight
        arrays.update(user_emb=ue, item_emb=ie, bpr=loss, loss_s=loss_s, **params_of(model), **grads_of(model))
        save(f"optembed_cf_{mname.replace('-', '_')}", **arrays)


def gen_neumf():
    """NeuMF on 'optembed_d' tables in eval: each table's _cur_weight set from an explicit per-row mask (NmfSearchOpt's
    _set_weight), then a forward and a backward to the tables."""
    gen = torch.Generator().manual_seed(100)
    NU, NI, EMB = 13, 17, 16
    set_seed(2027)
    model = NeuMF(NU, NI, emb_size=EMB, hidden_sizes=[16, 8], p_dropout=0,
                  embedding_config={"name": "optembed_d", "mode_threshold_d": "feature"})
    model.eval()
    arrays = dict(keys=np.array(list(model.state_dict().keys())))
    for tname, table in (("gmf_user", model._gmf.user_emb_table), ("gmf_item", model._gmf.item_emb_table),
                         ("mlp_user", model._mlp.user_emb_table), ("mlp_item", model._mlp.item_emb_table)):
        mask = torch.randint(0, EMB // 2, (table._num_item,), generator=gen)
        arrays[f"mask/{tname}"] = mask
        table._cur_weight = table.get_weight(mask)
    users = torch.randint(0, NU, (23,), generator=gen)
    items = torch.randint(0, NI, (23,), generator=gen)
    y = model(users, items)
    y.sum().backward()
    arrays.update(users=users, items=items, y=y, **params_of(model), **grads_of(model))
    save("optembed_cf_neumf", **arrays)


def gen_alpha():
    rows = []
    for ts, D in ((0.5, 64), (0.7, 64), (0.8, 64), (0.6, 64), (0.9, 64), (0.3, 64), (0.75, 32), (0.6, 16)):
        a = ou._find_alpha(ts, D)
        rows.append((ts, D, float(a), float(ou._get_expected_hidden_size(a, D))))
    lin = [(ts, D, ou._get_linear_hidden(ts, D)) for ts, D in ((0.5, 64), (0.7, 64), (0.8, 32), (0.95, 16))]
    save("optembed_cf_alpha", alpha=np.array(rows, dtype=np.float64), linear=np.array(lin, dtype=np.float64),
         weight_0p7_64=ou._generate_weight(ou._find_alpha(0.7, 64), 64))


if __name__ == "__main__":
    which = sys.argv[1:] or ["tables", "retrain", "lightgcn", "neumf", "alpha"]
    for w in which:
        globals()["gen_" + w]()

#!/usr/bin/env python3
"""Generate the HCCF golden vectors (tests/golden/hccf_L*.npz) by IMPORTING THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_hccf.py

Same conventions as gen_golden_neumf.py: the reference's modules are imported unmodified (`loguru` replaced by a no-op
stand-in), only arrays leave this script, and the archives carry a fixed member timestamp, so a rerun reproduces them
bit for bit.

The reference's HCCFModelCore (src/models/hccf.py) runs with p_dropout = 0 on a 37 x 53 graph with one user of degree
40, the others of degree 1-6 and a few items nobody touched; recorded are the COO matrix of get_adj(normalize=True),
both tables, the two outputs, BPR + 1e-4 * reg on fixed triples and both table gradients.
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

from src import losses as ref_losses  # noqa: E402
from src.graph_utils import get_adj  # noqa: E402
from src.models.hccf import HCCFModelCore  # noqa: E402
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


NU, NI, D, B = 37, 53, 8, 24
TOUCHED = 47            # items 47..52 are never interacted with
HUB_USER, HUB_DEGREE = 11, 40


def make_graph(gen):
    graph = {}
    for u in range(NU):
        deg = HUB_DEGREE if u == HUB_USER else int(torch.randint(1, 7, (1,), generator=gen))
        graph[u] = sorted(torch.randperm(TOUCHED, generator=gen)[:deg].tolist())
    return graph


def main():
    gen = torch.Generator().manual_seed(29)
    graph = make_graph(gen)
    adj = get_adj(graph, NI, NU, normalize=True)
    users = torch.randint(0, NU, (B,), generator=gen)
    users[0] = HUB_USER
    pos = torch.randint(0, NI, (B,), generator=gen)
    neg = torch.randint(0, NI, (B,), generator=gen)
    for L, slope in ((1, 0.5), (2, 0.2), (3, 0.5)):
        set_seed(2023)
        model = HCCFModelCore(NU, NI, num_layers=L, hidden_size=D, slope=slope, p_dropout=0)
        model.train()
        ue, ie = model(adj)
        loss = ref_losses.bpr_loss(ue[users], ie[pos], ie[neg])
        reg = model.get_reg_loss(users, pos, neg)
        (loss + 1e-4 * reg).backward()
        save(f"hccf_L{L}", adj_indices=adj.indices(), adj_values=adj.values(), num_user=np.array(NU), num_item=np.array(NI),
             num_layers=np.array(L), slope=np.array(slope), users=users, pos=pos, neg=neg, user_emb=ue, item_emb=ie, bpr=loss,
             reg=reg, **{"param/" + k: v.detach().clone() for k, v in model.state_dict().items()},
             **{"grad/" + k: p.grad.detach().clone() for k, p in model.named_parameters()})


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()

#!/usr/bin/env python3
"""Generate the DeepFM PEP search / retraining golden vectors (tests/golden/pep_deepfm_*.npz) by IMPORTING THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_pep_deepfm.py

Same conventions as gen_golden_optembed_deepfm.py: the reference's modules are imported unmodified (`loguru` replaced by a
no-op stand-in), only arrays leave this script, and the archives are written with a fixed member timestamp, so a rerun
reproduces them bit for bit.

  pep_deepfm_{global,dimension,feature,feature_dim}: DeepFM on a `pep` table of that threshold type, weights and
      thresholds set explicitly so that about half of the elements are pruned: parameters, x (repeated ids), labels,
      training logits, the gradient of every parameter under BCEWithLogitsLoss (embedding.emb.weight and embedding.s
      among them) and get_sparsity(True).
  pep_deepfm_retrain: RetrainPepEmbedding built from a saved milestone (the feature_dim table above): `mask`, logits, the
      gradients with sparse=False and with sparse=True (coalesced, as dense arrays).

Every element keeps ||w| - sigmoid(s)| >= MARGIN, so that a last-bit difference between two sigmoids can never flip an
element between kept and pruned; asserted below on the reference's own tensors.  The exceptions are planted exact cases:
w = 0 (pruned whatever s is: sign(0) = 0) under s = -150, w != 0 under s = -150 (sigmoid and its derivative are exactly
0), and s = +150 (sigmoid is exactly 1).  The retrain table holds exact zeros at kept positions.
"""
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

from src.models.deepfm import DeepFM  # noqa: E402
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


def dense(g):
    return g.coalesce().to_dense() if g.is_sparse else g


def grads_of(module, prefix="grad/"):
    return {prefix + k: dense(p.grad.detach()).clone() for k, p in module.named_parameters() if p.grad is not None}


DIMS, D, HIDDEN, B = [5, 3, 7, 4], 8, [16], 12
N = sum(DIMS)
MARGIN = 1e-3
SHAPES = {"global": (1,), "dimension": (D,), "feature": (N, 1), "feature_dim": (N, D)}


def batch(gen):
    x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in DIMS], 1)
    x[1], x[7, 2] = x[0], x[3, 2]      # a repeated sample, a repeated id
    y = (torch.rand(B, generator=gen) < 0.4).float()
    return x, y


def randomize_first_order(model, gen):
    with torch.no_grad():
        model.fc.weight.copy_(torch.randn(N, 1, generator=gen) * 0.3)
        model._bias.copy_(torch.randn(1, generator=gen) * 0.1)


def table_and_thresholds(kind, gen):
    """W [N, D] and s of the threshold type: sigmoid(s) in (0.1, 0.9), |w| on either side of it by 0.02 .. 0.4 (about half
    pruned), then the planted exact cases the type has room for."""
    thr = 0.1 + 0.8 * torch.rand(SHAPES[kind], generator=gen)
    s = torch.log(thr / (1 - thr))
    if kind == "dimension":
        s[2], s[5] = -150.0, 150.0
    if kind == "feature":
        s[4, 0], s[9, 0], s[13, 0] = -150.0, 150.0, -150.0
    if kind == "feature_dim":
        s[0, 1], s[0, 2], s[6, 3], s[11, :] = -150.0, -150.0, 150.0, 150.0
        s[14, 4:] = -150.0
    sig = torch.sigmoid(s).expand(N, D)
    side = torch.where(torch.rand(N, D, generator=gen) < 0.5, -1.0, 1.0)
    mag = (sig + side * (0.02 + 0.38 * torch.rand(N, D, generator=gen))).abs().clamp(min=0.011)
    W = mag * torch.where(torch.rand(N, D, generator=gen) < 0.5, -1.0, 1.0)
    W[0, 1] = 0.0                       # w = 0 (under s = -150 where the type has one there)
    W[3, 0], W[17, 7] = 0.0, -0.0
    return W, s


def check_margin(W, s):
    gap = (W.abs() - torch.sigmoid(s)).abs()
    assert bool(((gap >= MARGIN) | (W == 0)).all()), "an element sits within the margin of its threshold"
    kept = ((W.abs() - torch.sigmoid(s)) > 0).float().mean().item()
    assert 0.3 < kept < 0.7, f"about half of the elements should be pruned, kept {kept:.2f}"


def gen_search(tmp):
    gen = torch.Generator().manual_seed(411)
    for kind in SHAPES:
        set_seed(2041)
        cfg = {"name": "pep", "threshold_type": kind, "checkpoint_weight_dir": os.path.join(tmp, kind), "sparsity": [0.2, 0.9]}
        model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, use_batchnorm=False, embedding_config=cfg)
        randomize_first_order(model, gen)
        emb = model.embedding
        W, s = table_and_thresholds(kind, gen)
        with torch.no_grad():
            emb.emb.weight.copy_(W)
            emb.s.copy_(s)
        check_margin(emb.emb.weight.detach(), emb.s.detach())
        x, y = batch(gen)
        model.train()
        logits = model(x)
        loss = torch.nn.BCEWithLogitsLoss()(logits, y)
        loss.backward()
        with torch.no_grad():
            sparsity, nnz = emb.get_sparsity(True)
        save(f"pep_deepfm_{kind}", keys=np.array(list(model.state_dict().keys())), dims=np.array(DIMS),
             hidden=np.array(HIDDEN), kind=np.array(kind), margin=np.array(MARGIN), x=x, y=y, logits=logits, loss=loss,
             sparsity=np.array(sparsity), n_params=np.array(nnz), **params_of(model), **grads_of(model))
        if kind == "feature_dim":
            emb.train_callback()          # sparsity ~0.5 has passed the 0.2 milestone: {dir}/deepfm/0.2.pth
    return os.path.join(tmp, "feature_dim")


def gen_retrain(milestone_dir):
    gen = torch.Generator().manual_seed(412)
    found = torch.load(os.path.join(milestone_dir, "deepfm", "0.2.pth"), map_location="cpu")
    out = {}
    for sparse in (False, True):
        set_seed(2042)
        cfg = {"name": "pep_retrain", "checkpoint_weight_dir": milestone_dir, "sparsity": 0.2, "sparse": sparse}
        model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, use_batchnorm=False, embedding_config=cfg)
        emb = model.embedding
        if not sparse:
            g2 = torch.Generator().manual_seed(413)
            randomize_first_order(model, g2)
            W = (torch.rand(N, D, generator=g2) - 0.5) * 0.8
            kept = emb.mask.nonzero()
            for r, c in kept[::9].tolist():      # kept elements that hold exactly 0: they still receive their gradient
                W[r, c] = 0.0
            with torch.no_grad():
                emb.emb.weight.copy_(W)
            x, y = batch(gen)
            state = {k: v.clone() for k, v in model.state_dict().items()}
            assert int(((W == 0) & emb.mask).sum()) >= 1
        else:
            model.load_state_dict(state)
        model.train()
        logits = model(x)
        loss = torch.nn.BCEWithLogitsLoss()(logits, y)
        loss.backward()
        if not sparse:
            sparsity, nnz = emb.get_sparsity(True)
            out.update(keys=np.array(list(model.state_dict().keys())), dims=np.array(DIMS), hidden=np.array(HIDDEN), x=x, y=y,
                       mask=emb.mask.detach(), logits=logits, loss=loss, sparsity=np.array(sparsity), n_params=np.array(int(nnz)),
                       **{"milestone/" + k: v for k, v in found.items()}, **params_of(model), **grads_of(model))
        else:
            assert model.embedding.emb.weight.grad.is_sparse
            assert torch.equal(logits, torch.as_tensor(out["logits"]))
            out.update(grads_of(model, "grad_sparse/"))
    save("pep_deepfm_retrain", **out)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        gen_retrain(gen_search(tmp))

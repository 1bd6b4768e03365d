#!/usr/bin/env python3
"""Generate the DeepFM CERP / QR golden vectors (tests/golden/dual_deepfm_*.npz) by IMPORTING THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_dual_deepfm.py

Same conventions as gen_golden_pep_deepfm.py: the reference's modules are imported unmodified (`loguru` replaced by a
no-op stand-in), only arrays leave this script, and the archives are written with a fixed member timestamp, so a rerun
reproduces them bit for bit.

  dual_deepfm_cerp: DeepFM on a `cerp` table (bucket 7: q_entity_per_row = 3), weights and thresholds set explicitly so
      that about half of each table is pruned: parameters, x (repeated ids), labels, training logits, the gradient of
      every parameter under BCEWithLogitsLoss, get_sparsity(True), get_prune_loss() and the gradients of
      BCE + 1e-3 * prune loss (group grad_prune/).
  dual_deepfm_cerp_retrain: RetrainCerpEmbedding built from that table's checkpoint: masks, logits, the gradients with
      sparse=False (grad/) and with sparse=True (grad_sparse/, coalesced, as dense arrays).
  dual_deepfm_qr_mult / dual_deepfm_qr_add: DeepFM on a `qr` table, divider 3.

Every CERP element keeps ||w| - sigmoid(s)| >= MARGIN, so that a last-bit difference between two sigmoids can never flip
an element between kept and pruned; asserted below on the reference's own tensors.  Planted exact cases: w = 0, s = -150
(sigmoid and its derivative exactly 0), s = +150 (sigmoid exactly 1), looked-up rows where p' is pruned and q' is not.
The retrain tables hold exact zeros at kept positions.
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
BUCKET = 7
PER_ROW = -(-N // BUCKET)      # q_entity_per_row = 3
PRUNE_WEIGHT = 1e-3


def batch(gen):
    x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in DIMS], 1)
    x[1], x[7, 2] = x[0], x[3, 2]      # a repeated sample, a repeated id
    y = (torch.rand(B, generator=gen) < 0.4).float()
    return x, y


def randomize_first_order(model, gen):
    with torch.no_grad():
        model.fc.weight.copy_(torch.randn(N, 1, generator=gen) * 0.3)
        model._bias.copy_(torch.randn(1, generator=gen) * 0.1)


def table_and_thresholds(gen, plant):
    """W [BUCKET, D] and s like it: sigmoid(s) in (0.1, 0.9), |w| on either side of it by 0.02 .. 0.4 (about half pruned),
    then the planted exact cases."""
    thr = 0.1 + 0.8 * torch.rand(BUCKET, D, generator=gen)
    s = torch.log(thr / (1 - thr))
    for (r, c), v in plant.items():
        s[r, c] = v
    sig = torch.sigmoid(s)
    side = torch.where(torch.rand(BUCKET, D, generator=gen) < 0.5, -1.0, 1.0)
    mag = (sig + side * (0.02 + 0.38 * torch.rand(BUCKET, D, generator=gen))).abs().clamp(min=0.011)
    W = mag * torch.where(torch.rand(BUCKET, D, generator=gen) < 0.5, -1.0, 1.0)
    return W, s


def check_margin(W, s):
    gap = (W.abs() - torch.sigmoid(s)).abs()
    assert bool(((gap >= MARGIN) | (W == 0)).all()), "an element sits within the margin of its threshold"
    kept = ((W.abs() - torch.sigmoid(s)) > 0).float().mean().item()
    assert 0.3 < kept < 0.7, f"about half of the elements should be pruned, kept {kept:.2f}"


def step(model, x, y, prune_weight=None):
    model.zero_grad(set_to_none=True)
    model.train()
    logits = model(x)
    loss = torch.nn.BCEWithLogitsLoss()(logits, y)
    total = loss if prune_weight is None else loss + prune_weight * model.embedding.get_prune_loss()
    total.backward()
    return logits.detach(), loss.detach()


def gen_cerp(tmp):
    gen = torch.Generator().manual_seed(511)
    set_seed(2051)
    cfg = {"name": "cerp", "bucket_size": BUCKET}
    model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, use_batchnorm=False, embedding_config=cfg)
    randomize_first_order(model, gen)
    emb = model.embedding
    assert emb.q_entity_per_row == PER_ROW
    P, Sp = table_and_thresholds(gen, {(0, 1): -150.0, (0, 2): -150.0, (3, 3): 150.0, (5, 6): -150.0})
    Q, Sq = table_and_thresholds(gen, {(1, 0): -150.0, (2, 5): 150.0, (4, 4): -150.0, (6, 7): 150.0})
    P[0, 1], P[2, 0], P[4, 7] = 0.0, 0.0, -0.0       # w = 0 (under s = -150 at [0, 1])
    Q[1, 0], Q[3, 3] = 0.0, 0.0
    with torch.no_grad():
        emb.p_weight.copy_(P)
        emb.p_threshold.copy_(Sp)
        emb.q_weight.copy_(Q)
        emb.q_threshold.copy_(Sq)
    check_margin(emb.p_weight.detach(), emb.p_threshold.detach())
    check_margin(emb.q_weight.detach(), emb.q_threshold.detach())
    x, y = batch(gen)
    rows = (x + model.offsets).reshape(-1)
    kp = ((P.abs() - torch.sigmoid(Sp)) > 0)[rows % BUCKET]
    kq = ((Q.abs() - torch.sigmoid(Sq)) > 0)[torch.div(rows, PER_ROW, rounding_mode="trunc")]
    assert bool((~kp & kq).any()) and bool((kp & ~kq).any()), "no looked-up element with p' pruned and q' kept"
    logits, loss = step(model, x, y)
    grads = grads_of(model)
    with torch.no_grad():
        sparsity, nnz = emb.get_sparsity(True)
        prune = emb.get_prune_loss()
    step(model, x, y, PRUNE_WEIGHT)
    save("dual_deepfm_cerp", keys=np.array(list(model.state_dict().keys())), dims=np.array(DIMS), hidden=np.array(HIDDEN),
         bucket=np.array(BUCKET), margin=np.array(MARGIN), x=x, y=y, logits=logits, loss=loss, sparsity=np.array(sparsity),
         n_params=np.array(nnz), prune_loss=prune, prune_weight=np.array(PRUNE_WEIGHT), **params_of(model), **grads,
         **grads_of(model, "grad_prune/"))
    # the checkpoint pair RetrainCerpEmbedding loads: {dir}/deepfm/{initial,target}.pth
    os.makedirs(os.path.join(tmp, "deepfm"))
    found = {k: getattr(emb, k).detach().clone() for k in ("p_weight", "p_threshold", "q_weight", "q_threshold")}
    torch.save(found, os.path.join(tmp, "deepfm", "target.pth"))
    torch.save({"p_weight": found["p_weight"], "q_weight": found["q_weight"]}, os.path.join(tmp, "deepfm", "initial.pth"))
    return found


def gen_cerp_retrain(tmp, found):
    gen = torch.Generator().manual_seed(512)
    out = {}
    for sparse in (False, True):
        set_seed(2052)
        cfg = {"name": "cerp_retrain", "checkpoint_weight_dir": tmp, "bucket_size": BUCKET, "sparse": sparse}
        model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, use_batchnorm=False, embedding_config=cfg)
        emb = model.embedding
        if not sparse:
            g2 = torch.Generator().manual_seed(513)
            randomize_first_order(model, g2)
            tables = {}
            for name, mask in (("p_weight", emb.p_mask), ("q_weight", emb.q_mask)):
                W = (torch.rand(BUCKET, D, generator=g2) - 0.5) * 0.8
                for r, c in mask.nonzero()[::5].tolist():      # kept elements that hold exactly 0: they still receive their gradient
                    W[r, c] = 0.0
                assert int(((W == 0) & mask).sum()) >= 1
                tables[name] = W
            with torch.no_grad():
                emb.p_weight.copy_(tables["p_weight"])
                emb.q_weight.copy_(tables["q_weight"])
            x, y = batch(gen)
            state = {k: v.clone() for k, v in model.state_dict().items()}
        else:
            model.load_state_dict(state)
        logits, loss = step(model, x, y)
        if not sparse:
            out.update(keys=np.array(list(model.state_dict().keys())), dims=np.array(DIMS), hidden=np.array(HIDDEN),
                       bucket=np.array(BUCKET), x=x, y=y, p_mask=emb.p_mask.detach(), q_mask=emb.q_mask.detach(), logits=logits,
                       loss=loss, n_params=np.array(int(emb.p_mask.sum() + emb.q_mask.sum())),
                       **{"found/" + k: v for k, v in found.items()}, **params_of(model), **grads_of(model))
        else:
            assert torch.equal(logits, torch.as_tensor(out["logits"]))
            out.update(grads_of(model, "grad_sparse/"))
    save("dual_deepfm_cerp_retrain", **out)


def gen_qr():
    gen = torch.Generator().manual_seed(514)
    for op in ("mult", "add"):
        set_seed(2053)
        cfg = {"name": "qr", "divider": 3, "operation": op}
        model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, use_batchnorm=False, embedding_config=cfg)
        randomize_first_order(model, gen)
        with torch.no_grad():      # signed values (the default initialiser is positive only)
            model.embedding.emb1.weight.copy_((torch.rand(3, D, generator=gen) - 0.5) * 1.6)
            model.embedding.emb2.weight.copy_((torch.rand((N - 1) // 3 + 1, D, generator=gen) - 0.5) * 1.6)
        x, y = batch(gen)
        logits, loss = step(model, x, y)
        save(f"dual_deepfm_qr_{op}", keys=np.array(list(model.state_dict().keys())), dims=np.array(DIMS),
             hidden=np.array(HIDDEN), divider=np.array(3), operation=np.array(op), x=x, y=y, logits=logits, loss=loss,
             **params_of(model), **grads_of(model))


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        gen_cerp_retrain(tmp, gen_cerp(tmp))
    gen_qr()

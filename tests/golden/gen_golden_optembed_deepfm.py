#!/usr/bin/env python3
"""Generate the DeepFM OptEmbed search / retraining golden vectors (tests/golden/optembed_deepfm_*.npz) by IMPORTING
THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_optembed_deepfm.py

Same conventions as gen_golden_optembed_cf.py: the reference's modules are imported unmodified (`loguru` replaced by a
no-op stand-in), only arrays leave this script, every mask is given explicitly (nothing is drawn inside the reference),
and the archives are written with a fixed member timestamp, so a rerun reproduces them bit for bit.

  optembed_deepfm_candidate_{field,feature}: the supernet in eval under get_weight(mask) — what one candidate of the
      evolutionary search is scored on — with L1 / L2 row norms and thresholds that leave some rows dead: parameters,
      x, the logits, get_mask_e() and get_submask().
  optembed_deepfm_retrain_{field,feature}: RetrainOptEmbed after init_mask(mask_e, mask_d) with dead rows: the dtype and
      values of `_mask`, training logits (dropout 0), the gradients of every parameter under BCEWithLogitsLoss, and
      get_sparsity(True).
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


def grads_of(module, prefix="grad/"):
    return {prefix + k: p.grad.detach().clone() for k, p in module.named_parameters() if p.grad is not None}


DIMS, D, HIDDEN, B = [7, 3, 11, 5], 8, [12, 12], 24
N = sum(DIMS)


def batch(gen):
    x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in DIMS], 1)
    y = (torch.rand(B, generator=gen) < 0.4).float()
    return x, y


def randomize_first_order(model, gen):
    """fc.weight and the bias away from their initial values, so that the (unmasked) first-order term shows."""
    with torch.no_grad():
        model.fc.weight.copy_(torch.randn(N, 1, generator=gen) * 0.3)
        model._bias.copy_(torch.randn(1, generator=gen) * 0.1)


def gen_candidate():
    gen = torch.Generator().manual_seed(311)
    for md, norm in (("field", 1), ("feature", 2)):
        set_seed(2031)
        cfg = {"name": "deepfm_optembed", "norm": norm, "mode_threshold_e": md, "mode_threshold_d": md}
        model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, embedding_config=cfg)
        randomize_first_order(model, gen)
        emb = model.embedding
        m = emb._mask_e_module
        norms = torch.norm(emb._weight.detach(), norm, dim=1)
        # thresholds that cut some rows and sit clear of every row norm (a norm summed in another order must land on the
        # same side): per field halfway between its median norm and the next one up, per row the norm -+ (0.05 .. 0.2)
        with torch.no_grad():
            if md == "feature":
                u = torch.rand(N, generator=gen)
                m._t_param.copy_(norms + torch.where(u < 0.5, -1.0, 1.0) * (0.05 + 0.15 * torch.rand(N, generator=gen)))
            else:
                off = 0
                for f, n in enumerate(DIMS):
                    s_ = norms[off:off + n].sort().values
                    m._t_param[f] = (s_[n // 2] + s_[n // 2 + 1]) / 2
                    off += n
        mask_d = torch.randint(0, D, (len(DIMS) if md == "field" else N,), generator=gen)
        x, _ = batch(gen)
        model.eval()
        with torch.no_grad():
            emb.get_weight(mask_d)
            logits = model(x)
            mask_e = emb.get_mask_e()
            emb.get_submask.cache_clear()
            submask = emb.get_submask()
        assert 0 < int(mask_e.sum()) < N, "the thresholds must leave some rows dead and some alive"
        save(f"optembed_deepfm_candidate_{md}", keys=np.array(list(model.state_dict().keys())), dims=np.array(DIMS),
             hidden=np.array(HIDDEN), norm=np.array(norm), mode=np.array(md), x=x, mask_d=mask_d, logits=logits,
             mask_e=mask_e, submask=submask, **params_of(model))


def gen_retrain():
    gen = torch.Generator().manual_seed(312)
    for md in ("field", "feature"):
        set_seed(2032)
        cfg = {"name": "deepfm_optembed_retrain", "mode_threshold_d": md}
        model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, embedding_config=cfg)
        randomize_first_order(model, gen)
        emb = model.embedding
        with torch.no_grad():      # (the reference leaves _weight as torch.empty)
            emb._weight.copy_((torch.rand(N, D, generator=gen) - 0.5) * 0.8)
        mask_e = (torch.rand(N, generator=gen) < 0.7).to(int)      # what OptEmbed.get_mask_e() returns: int64 zeros / ones
        mask_d = torch.randint(0, D, (len(DIMS) if md == "field" else N,), generator=gen)
        mask = emb.init_mask(mask_e, mask_d)
        x, y = batch(gen)
        model.train()
        logits = model(x)
        loss = torch.nn.BCEWithLogitsLoss()(logits, y)
        loss.backward()
        sparsity, nnz = emb.get_sparsity(True)
        save(f"optembed_deepfm_retrain_{md}", keys=np.array(list(model.state_dict().keys())), dims=np.array(DIMS),
             hidden=np.array(HIDDEN), mode=np.array(md), x=x, y=y, mask_e=mask_e, mask_d=mask_d, mask=mask,
             mask_dtype=np.array(str(mask.dtype)), logits=logits, loss=loss, sparsity=np.array(sparsity),
             n_params=np.array(nnz), **params_of(model), **grads_of(model))


if __name__ == "__main__":
    which = sys.argv[1:] or ["candidate", "retrain"]
    for w in which:
        globals()["gen_" + w]()

#!/usr/bin/env python3
"""Generate the DeepFM QAT / PTQ golden vectors (tests/golden/quant_deepfm_*.npz) by IMPORTING THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_quant_deepfm.py

Same conventions as gen_golden_dual_deepfm.py: the reference's modules are imported unmodified (`loguru` replaced by a
no-op stand-in), only arrays leave this script, and the archives are written with a fixed member timestamp, so a rerun
reproduces them bit for bit.

  quant_deepfm_qat: a small DeepFM on a `qat` table at n_bits 8 and 16 (groups b8/ and b16/): parameters (`scale`
      included), x (an id repeated within a field, a repeated sample), labels, the recorded torch.rand_like draw, the rounded
      rows the reference's embedding returned, training logits and the gradient of every parameter under BCEWithLogitsLoss.
  quant_deepfm_ptq: the eval logits of a DeepFM whose embedding was replaced, as scripts/deepfm/run_ptq.py does, by
      PTQEmb_Int at 4, 8 and 16 bits and by PTQEmb_Fp16 (groups int4/, int8/, int16/, fp16/: codes, scale, zero point,
      the rows the embedding returned, logits), plus the fp32 model they were quantised from.

Asserted below on the reference's own tensors: looked-up elements with w / scale >= q_max and <= q_min (both clamp
branches), elements exactly on the grid (w / scale an integer, w = 0 among them), an id repeated within a field, the
recorded draw reproducing the reference's rounded rows bit for bit, and — for the integer PTQ tables — code - zero_point
inside the storage type: the reference subtracts in the storage type and would wrap, the library subtracts in int32.
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
from src.models.embeddings.ptq_emb import PTQEmb_Fp16, PTQEmb_Int  # noqa: E402
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


def params_of(module, prefix):
    return {prefix + k: v.detach().clone() for k, v in module.state_dict().items() if isinstance(v, torch.Tensor)}


def grads_of(module, prefix):
    return {prefix + k: p.grad.detach().clone() for k, p in module.named_parameters() if p.grad is not None}


DIMS, D, HIDDEN, B = [5, 3, 7, 4], 8, [16], 12
N = sum(DIMS)
SCALES = {8: 0.00097, 16: 3.9e-6}      # regular weights |w| <= 0.1 stay inside the range: 0.1 / scale = 103 and 25641
R_MIN, R_MAX = -0.1, 0.0999968         # the extremes of the table the PTQ classes quantise (gen_ptq)


def batch(gen):
    x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in DIMS], 1)
    x[1], x[7, 2] = x[0], x[3, 2]      # a repeated sample, an id repeated within a field
    y = (torch.rand(B, generator=gen) < 0.4).float()
    return x, y


def randomize_first_order(model, gen):
    with torch.no_grad():
        model.fc.weight.copy_(torch.randn(N, 1, generator=gen) * 0.3)
        model._bias.copy_(torch.randn(1, generator=gen) * 0.1)


def rounded_rows(w, scale, n_bits, prob):
    """StotasticRounding.forward restated with the draw given (float32, the reference's operations in its order)."""
    q_min, q_max = -(1 << (n_bits - 1)), (1 << (n_bits - 1)) - 1
    q = torch.clamp(w / scale, q_min, q_max)
    fl = torch.floor(q)
    return (fl + (prob > fl + 1 - q)) * scale


def gen_qat():
    gen = torch.Generator().manual_seed(611)
    out = {"dims": np.array(DIMS), "hidden": np.array(HIDDEN), "bits": np.array([8, 16])}
    for bits in (8, 16):
        q_min, q_max = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        set_seed(3051)
        model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, use_batchnorm=False, embedding_config={"name": "qat", "n_bits": bits})
        randomize_first_order(model, gen)
        x, y = batch(gen)
        rows = x + model.offsets
        s = torch.tensor(SCALES[bits])
        W = (torch.rand(N, D, generator=gen) - 0.5) * 0.2
        ra, rb, rc = int(rows[0, 0]), int(rows[2, 1]), int(rows[3, 2])      # looked-up rows (rc twice: x[7, 2] = x[3, 2])
        W[ra, 0], W[ra, 1] = 0.5, -0.5                                    # beyond both clamps
        W[rb, 2], W[rb, 3] = float(q_max) * s.item() * 1.5, float(q_min) * s.item() * 1.5
        W[rc, 0], W[rc, 1] = 0.0, -0.0                                    # on the grid: w = 0
        on_grid = [k for k in (1, -3, 17, q_max // 2, q_min // 3) if (torch.tensor(float(k)) * s) / s == float(k)]
        assert len(on_grid) >= 2, "no multiple of the scale divides back exactly"
        for c, k in enumerate(on_grid[:4]):
            W[rc, 2 + c] = torch.tensor(float(k)) * s                     # on the grid: w = k * scale
        with torch.no_grad():
            model.embedding._emb_module.weight.copy_(W)
            model.embedding.scale.copy_(s)
        qf = (model.embedding._emb_module.weight.detach() / model.embedding.scale.detach())[rows.reshape(-1)]
        assert bool((qf >= q_max).any()) and bool((qf <= q_min).any()), "a clamp branch is not reached"
        assert int(((qf == torch.floor(qf)) & (qf > q_min) & (qf < q_max)).sum()) >= 4, "no looked-up element on the grid"
        inside = ((qf > q_min) & (qf < q_max)).float().mean().item()
        assert inside > 0.9, f"most elements should round, not clamp: {inside:.2f}"
        seen = []
        handle = model.embedding.register_forward_hook(lambda m, a, o: seen.append(o.detach().clone()))
        model.train()
        torch.manual_seed(99)
        logits = model(x)
        torch.manual_seed(99)
        prob = torch.rand(B, len(DIMS), D)      # the forward consumed exactly one rand_like of the gathered rows' shape
        handle.remove()
        assert torch.equal(seen[0], rounded_rows(W[rows], s, bits, prob)), "the recorded draw does not reproduce the rows"
        loss = torch.nn.BCEWithLogitsLoss()(logits, y)
        loss.backward()
        p = f"b{bits}/"
        out.update({p + "x": x, p + "y": y, p + "prob": prob, p + "emb": seen[0], p + "logits": logits.detach(),
                    p + "loss": loss.detach()}, **params_of(model, p + "param/"), **grads_of(model, p + "grad/"))
        out["keys"] = np.array(list(model.state_dict().keys()))
    save("quant_deepfm_qat", **out)


def gen_ptq():
    gen = torch.Generator().manual_seed(612)
    set_seed(3052)
    model = DeepFM(DIMS, D, HIDDEN, p_dropout=0.0, use_batchnorm=False, embedding_config={"name": "vanilla"})
    randomize_first_order(model, gen)
    W = (torch.rand(N, D, generator=gen) - 0.5) * 0.19
    # min / (max - min) inside (-0.5000153, -0.5): min / scale lies within half a code of q_min at 8 AND at 16 bits, so
    # the zero point is 0, no code leaves the storage type and code - zero_point does not wrap (asserted below)
    W[0, 0], W[N - 1, D - 1] = R_MIN, R_MAX
    with torch.no_grad():
        model.embedding._emb_module.weight.copy_(W)
    x, _ = batch(gen)
    model.eval()
    out = {"dims": np.array(DIMS), "hidden": np.array(HIDDEN), "x": x, "keys": np.array(list(model.state_dict().keys())),
           **params_of(model, "param/")}
    with torch.no_grad():
        out["fp32_logits"] = model(x)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "original.pth")
        torch.save({"state_dict": model.state_dict()}, path)
        for name, bits in (("int4", 4), ("int8", 8), ("int16", 16), ("fp16", None)):
            emb = PTQEmb_Fp16(None, None, None, path) if bits is None else PTQEmb_Int(None, None, None, path, bits)
            if bits is not None:
                info = torch.iinfo(emb.weight.dtype)
                before_cast = torch.round(W / emb.scale + emb.bias)
                if bits >= 8:
                    assert float(before_cast.min()) >= info.min and float(before_cast.max()) <= info.max, f"{name}: a code overflowed"
                assert int(emb.bias) == 0
                exact = emb.weight.to(torch.int32) - emb.bias.to(torch.int32)
                assert torch.equal((emb.weight - emb.bias).to(torch.int32), exact), f"{name}: code - zero_point wrapped"
                assert int(exact.min()) >= info.min and int(exact.max()) <= info.max
                out.update({f"{name}/weight": emb.weight, f"{name}/scale": emb.scale, f"{name}/bias": emb.bias})
            else:
                out[f"{name}/weight"] = emb.weight.view(torch.int16)      # raw half bits
            model.embedding = emb      # scripts/deepfm/run_ptq.py:109
            seen = []
            handle = emb.register_forward_hook(lambda m, a, o: seen.append(o.detach().clone()))
            with torch.no_grad():
                out[f"{name}/logits"] = model(x)
            handle.remove()
            out[f"{name}/emb"] = seen[0]
    save("quant_deepfm_ptq", **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen_qat()
    gen_ptq()

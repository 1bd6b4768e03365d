#!/usr/bin/env python3
"""Generate tests/golden/ptq_int4.npz by IMPORTING THE REFERENCE's PTQEmb_Int at n_bits = 4.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_int4.py

Same conventions as gen_golden_quant_deepfm.py: the reference's module is imported unmodified (`loguru` replaced by a no-op
stand-in), only arrays leave this script, and the archive is written with a fixed member timestamp, so a rerun reproduces it
bit for bit.

  ptq_int4: a table W fp32 [300, 16] over [-0.06, 0.13] (so that the zero point is not 0), ids x [12, 4], and the
      reference's own `weight` (int8, one 4-bit code per byte), `scale`, `bias` and `out` = forward(x).

Asserted below on the reference's tensors: every code inside [-8, 7] with both ends reached, a zero point other than 0, and
code - zero point inside int8 (the reference subtracts in the storage type and would wrap; the library subtracts in int32).
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

from src.models.embeddings.ptq_emb import PTQEmb_Int  # noqa: E402

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


N, D, B, F = 300, 16, 12, 4


def main():
    gen = torch.Generator().manual_seed(4104)
    W = torch.rand(N, D, generator=gen) * 0.19 - 0.06
    W[0, 0], W[N - 1, D - 1] = -0.06, 0.13
    x = torch.randint(0, N, (B, F), generator=gen)
    x[1], x[7, 2] = x[0], x[3, 2]      # a repeated sample, a repeated id
    x[2, 0], x[2, 1] = 0, N - 1        # the rows that hold the extremes
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "original.pth")
        torch.save({"state_dict": {"embedding._emb_module.weight": W}}, path)
        emb = PTQEmb_Int(None, None, None, path, 4)
    assert emb.weight.dtype == torch.int8 and emb.bias.dtype == torch.int8
    assert int(emb.weight.min()) == -8 and int(emb.weight.max()) == 7
    assert int(emb.bias) != 0
    exact = emb.weight.to(torch.int32) - emb.bias.to(torch.int32)
    assert torch.equal((emb.weight - emb.bias).to(torch.int32), exact), "code - zero point wrapped"
    with torch.no_grad():
        out = emb(x)
    save("ptq_int4", W=W, x=x, weight=emb.weight, scale=emb.scale, bias=emb.bias, out=out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()

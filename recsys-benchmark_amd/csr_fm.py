"""The CTR models' lookups on a CSR-pruned table (csrc/gather_fm_csr.hip); inference only, like PrunedEmbedding itself.

gather_fm_csr: DeepFM's lookup + FM + first-order term in one launch (mi_gather_fm_csr_fwd) — the CSR rows are densified
    inside the launch by the lanes of a row slot together.
csr_rows_typed: the densify alone (mi_csr_rows_typed_fwd), optionally with the per-field offsets added inside the launch.

Both take the row pointers as int32 or int64 and the columns as uint8 or int64 (PrunedEmbedding.compact_()).
Buffers come from the package's float allocator (layer_dcn._new).
"""
from typing import Optional, Tuple

import torch

from . import _kernels, _lib
from .layer_dcn import _int64_rows, _new

CROW_DTYPES = {torch.int32: 4, torch.int64: 8}      # crow_bytes of the two entry points
COL_DTYPES = {torch.uint8: 1, torch.int64: 8}       # col_bytes


def _csr_operands(values, crow, col, D: int, N: int):
    """(values fp32, crow, col, crow_bytes, col_bytes) as the launches read them (ValueError / TypeError otherwise)."""
    crow_bytes, col_bytes = CROW_DTYPES.get(crow.dtype), COL_DTYPES.get(col.dtype)
    if crow_bytes is None:
        raise TypeError(f"crow_indices must be int32 or int64, got {crow.dtype}")
    if col_bytes is None:
        raise TypeError(f"col_indices must be uint8 or int64, got {col.dtype}")
    if values.dtype != torch.float32:
        raise TypeError(f"values must be float32, got {values.dtype}")
    if crow.dim() != 1 or crow.numel() != N + 1:
        raise ValueError(f"crow_indices must hold N + 1 = {N + 1} row pointers, got {tuple(crow.shape)}")
    if col.dim() != 1 or values.dim() != 1 or col.numel() != values.numel():
        raise ValueError(f"col_indices {tuple(col.shape)} and values {tuple(values.shape)} must be 1-D and of one length")
    if col_bytes == 1 and D > 256:
        raise ValueError(f"one-byte columns need D <= 256, got {D}")
    if D <= 0:
        raise ValueError(f"D must be positive, got {D}")
    return values.contiguous(), crow.contiguous(), col.contiguous(), crow_bytes, col_bytes


def _ptr(t: torch.Tensor) -> Optional[int]:
    return t.data_ptr() if t.numel() else None


def gather_fm_csr(idx, offsets, values, crow, col, w1, bias, D: int, N: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(emb fp32[B, F, D], y_fm[B]) of DeepFM over the CSR table (values, crow, col) of N rows and D columns in one launch
    (mi_gather_fm_csr_fwd): emb[b, f] = the dense row idx[b, f] + offsets[f] — the bits of _kernels.csr_rows —, y_fm the FM
    second-order term of emb plus the first-order bag over w1 plus bias.  offsets may be None.  No autograd: inference only."""
    dev = _lib.require_gpu(idx, offsets, values, crow, col, w1, bias)
    D, N = int(D), int(N)
    values, crow, col, crow_bytes, col_bytes = _csr_operands(values, crow, col, D, N)
    with torch.no_grad():
        idx, offsets, w1c, ldw1, _ = _kernels._lookup_operands(idx, offsets, w1.detach(), N)
        B, F = idx.shape
        emb = _new((B, F, D), dev)
        yfm = _new((B,), dev)
        _lib.check(
            _lib.load().mi_gather_fm_csr_fwd(
                idx.data_ptr(), _lib.ptr(offsets), _ptr(values), crow.data_ptr(), crow_bytes, _ptr(col), col_bytes,
                w1c.data_ptr(), ldw1, _lib.ptr(None if bias is None else bias.detach()), emb.data_ptr(), yfm.data_ptr(), None,
                B, F, D, N, _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev),
            ),
            "mi_gather_fm_csr_fwd",
        )
    return emb, yfm


def csr_rows_typed(values, crow, col, ids, D: int, N: int, offsets=None):
    """Dense rows fp32[ids.shape + (D,)] of the CSR table (mi_csr_rows_typed_fwd), the bits of _kernels.csr_rows.
    offsets (int64[F], ids [..., F]): the rows are ids + offsets, added inside the launch; returns (rows, row ids)."""
    dev = _lib.require_gpu(ids, offsets, values, crow, col)
    D, N = int(D), int(N)
    values, crow, col, crow_bytes, col_bytes = _csr_operands(values, crow, col, D, N)
    idsc = _kernels._i64c(ids)
    F, rows = 0, None
    if offsets is not None:
        offsets = _kernels._i64c(offsets.reshape(-1))
        F = offsets.numel()
        if idsc.dim() < 1 or idsc.shape[-1] != F or F < 1:
            raise ValueError(f"ids must be [..., F] with one offset per field, got {tuple(idsc.shape)} and {F} offsets")
        rows = _int64_rows(idsc.numel() // F, F, dev).view(idsc.shape)
    out = _new(tuple(idsc.shape) + (D,), dev)
    _lib.check(
        _lib.load().mi_csr_rows_typed_fwd(_ptr(values), crow.data_ptr(), crow_bytes, _ptr(col), col_bytes, idsc.data_ptr(),
                                          _lib.ptr(offsets), F, _lib.ptr(rows), out.data_ptr(), idsc.numel(), D, N,
                                          _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
        "mi_csr_rows_typed_fwd",
    )
    return out if offsets is None else (out, rows)

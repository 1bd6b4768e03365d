"""DeepFM's fused lookup + FM + first-order launch on the quantised tables (csrc/gather_fm_quant.hip).

gather_fm_quant: the post-training-quantised tables (PTQEmb_Int, PTQEmb_Fp16) — fp16 / int8 / int16 codes, or 4-bit codes
    packed two to a byte, dequantised inside the launch; inference only, like _kernels.gather_rows_quant.
gather_fm_qat: the quantisation-aware-training table (QAT_EmbInt) — the fp32 rows rounded stochastically inside the launch;
    one autograd node whose backward is one row-form launch (mi_gather_fm_qat_bwd_rows) feeding _kernels._table_grads, so
    a row-form table gets COO gradients, a dense one the scatter of those values, and deterministic mode their sorted
    fixed-order sum: no float atomic on DeepFM + QAT in that mode.

gather_rows_int4, ptq_quantise, int4_repack: the packed 4-bit table's row gather, the one-pass quantiser of the PTQ integer
    tables and the int8 <-> nibble repacker (csrc/ptq_int4.hip).  A packed table is uint8 [N, D / 2]; the caller always SAYS
    that it is packed (packed4=True with the logical D, or one of these functions): a uint8 tensor alone never means it.

Buffers come from the package's float allocator (layer_dcn._new); the int64 row ids the backward needs are written by
the forward launch into an int64 view of such a buffer, and so are the code tables the quantiser and the repacker write.
"""
from typing import Optional

import torch

from . import _kernels, _lib
from . import losses as _losses
from .layer_dcn import _int64_rows, _new

QTYPES = {torch.float16: 1, torch.int8: 2, torch.int16: 3}      # the qtype codes of mi_gather_rows_quant
QTYPE_INT4_PACKED = 5                                          # MI_QTYPE_INT4_PACKED
QAT_BWD_MAX_D = 256                                            # MI_GATHER_FM_QAT_BWD_MAX_D
SCALE_GRAD_MAX_BITS = 21      # the backward recovers the rounded code as rintf(emb / scale): exact for |code| <= 2^20


def _packed4(W, D: int):
    """The packed 4-bit table uint8 [N, D / 2] (include/mi355x_recsys.h, PTQEmb_Int(packed=True)) of logical width D, row-
    contiguous."""
    if W.dtype != torch.uint8 or W.dim() != 2:
        raise TypeError(f"a packed 4-bit table is uint8 [N, D / 2], got {W.dtype} {tuple(W.shape)}")
    if D % 2 or W.shape[1] * 2 != D:
        raise ValueError(f"a packed 4-bit table of logical width {D} holds {D}/2 bytes per row, got {W.shape[1]}")
    return W if W.is_contiguous() else W.contiguous()


def _int8_word(zero_point):
    if zero_point.dtype != torch.int8 or zero_point.numel() != 1:
        raise TypeError(f"the zero point of a 4-bit table is one int8 word (it is never packed), got {zero_point.dtype}")
    return zero_point.reshape(1)


def _new_codes(shape, dtype, dev):
    """A code table the launch fills, out of the float allocator like layer_dcn._int64_rows: whole float words, viewed."""
    n = 1
    for d in shape:
        n *= int(d)
    size = {torch.int8: 1, torch.uint8: 1, torch.int16: 2}[dtype]
    return _new(((n * size + 3) // 4,), dev).view(dtype)[:n].view(shape)


def gather_fm_quant(idx, offsets, Wq, w1, bias, scale=None, zero_point=None, packed4: bool = False, D: Optional[int] = None):
    """(emb fp32[B, F, D], y_fm[B]) of DeepFM over a quantised table in one launch (mi_gather_fm_quant_fwd):
    emb[b, f] = dequant(Wq[idx[b, f] + offsets[f]]) — (code - zero_point) * scale for int8 / int16 codes, the value itself
    for fp16 —, y_fm the FM second-order term of emb plus the first-order bag over w1 plus bias.  offsets may be None.
    packed4=True with the logical width D: Wq is the packed 4-bit table uint8 [N, D / 2] of PTQEmb_Int(packed=True), the
    zero point one int8 word; emb has the bits of the int8 table of the unpacked codes (a uint8 table is never taken for
    packed without being told).  No autograd: inference only."""
    dev = _lib.require_gpu(idx, offsets, Wq, w1, bias, scale, zero_point)
    if packed4:
        if D is None:
            raise ValueError("a packed 4-bit table needs its logical width D")
        if scale is None or zero_point is None:
            raise ValueError("an integer table needs its scale and zero point")
        Wq, qtype = _packed4(Wq, int(D)), QTYPE_INT4_PACKED
        zero_point = _int8_word(zero_point)
    else:
        if D is not None:
            raise ValueError("D is the logical width of a packed 4-bit table (packed4=True)")
        qtype = QTYPES.get(Wq.dtype)
    if qtype is None:
        raise TypeError(f"unsupported quantised table dtype {Wq.dtype}")
    if Wq.dim() != 2:
        raise ValueError(f"the table must be [N, D], got {tuple(Wq.shape)}")
    if qtype != 1:
        if scale is None or zero_point is None:
            raise ValueError("an integer table needs its scale and zero point")
        if not packed4 and zero_point.dtype != Wq.dtype:
            raise TypeError(f"the zero point is held in the table's type {Wq.dtype}, got {zero_point.dtype}")
        scale = _kernels._f32c(scale.reshape(1))
        zero_point = zero_point.reshape(1)
    else:
        scale = zero_point = None
    # (a view that is row-contiguous is read in place, wherever it starts: the launch picks the scalar kernels for a base
    #  that is not on a four-code boundary)
    Wc = Wq if Wq.is_contiguous() else Wq.contiguous()
    N, D = Wc.shape[0], (int(D) if packed4 else Wc.shape[1])
    with torch.no_grad():
        idx, offsets, w1c, ldw1, _ = _kernels._lookup_operands(idx, offsets, w1.detach(), N)
        B, F = idx.shape
        emb = _new((B, F, D), dev)
        yfm = _new((B,), dev)
        _lib.check(
            _lib.load().mi_gather_fm_quant_fwd(
                idx.data_ptr(), _lib.ptr(offsets), Wc.data_ptr(), qtype, _lib.ptr(scale), _lib.ptr(zero_point),
                w1c.data_ptr(), ldw1, _lib.ptr(bias), emb.data_ptr(), yfm.data_ptr(), B, F, D, N,
                _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev),
            ),
            "mi_gather_fm_quant_fwd",
        )
    return emb, yfm


class GatherFMQat(torch.autograd.Function):
    """emb, y_fm of DeepFM over a QAT table in one launch (mi_gather_fm_qat_fwd): the gathered fp32 rows are clamped,
    rounded stochastically and rescaled (the arithmetic of mi_qat_gather_fwd, the draw of element (b F + f) D + d from
    `prob` or from the counter generator on `seed`), y_fm over that emb, the first-order term untouched.

    Backward: one row-form launch over the saved emb — the table's gradient passes straight through the rounding; the
    scale's gradient, when the scale is trained, is summed in the same launch in a fixed order (the W rows are gathered
    again for it, and only then)."""

    @staticmethod
    def forward(ctx, idx, offsets, W, scale, w1, bias, n_bits: int, seed, salt: int, prob, sparse_W: bool, sparse_w1: bool):
        dev = _lib.require_gpu(idx, offsets, W, scale, w1, bias, seed, prob)
        if prob is None and seed is None:
            raise ValueError("gather_fm_qat needs a seed word or an explicit draw")
        if W.dim() != 2:
            raise ValueError(f"the table must be [N, D], got {tuple(W.shape)}")
        Wc = _kernels._f32c(W)
        N, D = Wc.shape
        if D > QAT_BWD_MAX_D:
            raise NotImplementedError(f"gather_fm_qat's backward covers D <= {QAT_BWD_MAX_D}, got {D}")
        idx, offsets, w1c, ldw1, _ = _kernels._lookup_operands(idx, offsets, w1, N)
        B, F = idx.shape
        sc = _kernels._f32c(scale.reshape(1))
        probc = None
        if prob is not None:
            probc = _kernels._f32c(prob)
            if probc.numel() != B * F * D:
                raise ValueError(f"prob must hold one draw per element of emb [{B}, {F}, {D}], got {tuple(prob.shape)}")
        if seed is not None and (seed.dtype != torch.int64 or seed.numel() != 1):
            raise ValueError("seed must be one int64 device word")
        need = [ctx.needs_input_grad[i] for i in (2, 3, 4, 5)]
        if need[1] and int(n_bits) > SCALE_GRAD_MAX_BITS:
            raise NotImplementedError(f"gather_fm_qat's scale gradient covers n_bits <= {SCALE_GRAD_MAX_BITS}, got {n_bits}")
        emb = _new((B, F, D), dev)
        yfm = _new((B,), dev)
        rows = _int64_rows(B, F, dev) if any(need[:3]) else None      # (ids for the gradients' rows and the W re-gather)
        _lib.check(
            _lib.load().mi_gather_fm_qat_fwd(
                idx.data_ptr(), _lib.ptr(offsets), Wc.data_ptr(), sc.data_ptr(), int(n_bits), _lib.ptr(probc), _lib.ptr(seed),
                int(salt), w1c.data_ptr(), ldw1, _lib.ptr(bias), emb.data_ptr(), yfm.data_ptr(), _lib.ptr(rows), B, F, D, N,
                _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev),
            ),
            "mi_gather_fm_qat_fwd",
        )
        if rows is not None and offsets is not None and (sparse_W or sparse_w1 or _kernels.DETERMINISTIC):
            _kernels.note_field_layout(rows, offsets, N)
        # (the table and the scale are autograd inputs: saved, so that an in-place update before the backward raises)
        ctx.save_for_backward(emb, rows, Wc, sc)
        ctx.meta = (B, F, D, N, int(n_bits), tuple(W.shape), tuple(scale.shape), tuple(w1.shape))
        ctx.sparse = (bool(sparse_W), bool(sparse_w1))
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)
        return emb, yfm

    @staticmethod
    def backward(ctx, g_emb, g_y):
        emb, rows, Wc, sc = ctx.saved_tensors
        B, F, D, N, n_bits, Wshape, sshape, w1shape = ctx.meta
        sparse_W, sparse_w1 = ctx.sparse
        dev = emb.device
        lib = _lib.load()
        stream = _lib.stream_ptr(dev)
        need_W, need_s, need_w1 = ctx.needs_input_grad[2], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        need_b = ctx.has_bias and ctx.needs_input_grad[5]
        g_emb, g_y = _kernels._upstream(g_emb, g_y, B, dev)
        gb = _new((1,), dev) if need_b else None
        if not (need_W or need_s or need_w1):
            return (None,) * 5 + (_kernels._bias_grad(gb, g_y, B, launched=False),) + (None,) * 6
        gvals = _new((B * F, D), dev)
        g1vals = _new((B * F,), dev)

        def launch(gvals, g1vals, gb):
            ds = _new((1,), dev) if need_s else None
            ws, armed = (_losses._ticket_workspace("gather_fm_qat", dev, lib.mi_gather_fm_qat_bwd_workspace_elems(B))
                         if need_s and B > 0 else (None, True))
            _lib.check(
                lib.mi_gather_fm_qat_bwd_rows(_lib.ptr(rows), Wc.data_ptr() if need_s else None, sc.data_ptr(), n_bits,
                                              emb.data_ptr(), g_y.data_ptr(), _lib.ptr(g_emb), gvals.data_ptr(),
                                              g1vals.data_ptr(), _lib.ptr(gb), _lib.ptr(ds), _lib.ptr(ws), int(armed), B, F, D, N,
                                              stream),
                "mi_gather_fm_qat_bwd_rows",
            )
            return None if ds is None else ds.view(sshape)

        gW, gw1, gb, gs = _kernels._row_backward(launch, B, rows, gvals, g1vals, gb, N, D, Wshape, w1shape, sparse_W, sparse_w1,
                                                 need_W, need_w1, stream)
        return None, None, gW, gs, gw1, gb, None, None, None, None, None, None


def gather_fm_qat(idx, offsets, W, scale, n_bits: int, w1, bias, *, seed: Optional[torch.Tensor] = None,
                  prob: Optional[torch.Tensor] = None, sparse_W: bool = False, sparse_w1: bool = False):
    """(emb, y_fm) of DeepFM over a QAT table, one autograd node.  seed: one int64 device word (the rounding stream of
    this forward); prob: the draw itself, one value per element of emb (tests)."""
    return GatherFMQat.apply(idx, offsets, W, scale, w1, bias, int(n_bits), seed, 0, prob, sparse_W, sparse_w1)


def gather_rows_int4(idx, W, scale, zero_point, D: int, offsets=None):
    """Dequantising row gather over a PACKED 4-bit table (mi_gather_rows_int4): out fp32 idx.shape + (D,) with the bits of
    _kernels.gather_rows_quant over the unpacked int8 codes.  idx None: the whole table [N, D] (row r is r, no index tensor).
    offsets ([F], with idx [B, F]): the raw per-field ids plus their offsets inside the launch; returns (out, rows)."""
    dev = _lib.require_gpu(idx, W, scale, zero_point, offsets)
    Wc = _packed4(W, int(D))
    N = Wc.shape[0]
    sc, zp = _kernels._f32c(scale.reshape(1)), _int8_word(zero_point)
    rows, F = None, 1
    if idx is None:
        if offsets is not None:
            raise ValueError("the table form takes no offsets")
        idxc, n, shape = None, N, (N,)
    else:
        idxc = _kernels._i64c(idx)
        n, shape = idxc.numel(), tuple(idx.shape)
        if offsets is not None:
            offsets = _kernels._i64c(offsets.reshape(-1))
            F = offsets.numel()
            if idxc.dim() != 2 or idxc.shape[1] != F:
                raise ValueError(f"offsets of {F} fields need ids [B, {F}], got {shape}")
            rows = _int64_rows(shape[0], F, dev)
    out = _new(shape + (int(D),), dev)
    _lib.check(
        _lib.load().mi_gather_rows_int4(_lib.ptr(idxc), _lib.ptr(offsets), Wc.data_ptr(), sc.data_ptr(), zp.data_ptr(),
                                        out.data_ptr(), _lib.ptr(rows), n, F, int(D), N, _lib.err_word(dev).data_ptr(),
                                        _lib.stream_ptr(dev)),
        "mi_gather_rows_int4",
    )
    return out if offsets is None else (out, rows)


def ptq_quantise(table, scale, zero_point, n_bits: int, packed: bool = False):
    """The codes of the fp32 table [N, D] (a view of any row stride is read in place) under a given scale and zero point —
    device scalars: fp32, and the storage type's — in one launch (mi_ptq_quantise): int8 [N, D] (n_bits 4, 8), int16 [N, D]
    (16) or, packed, uint8 [N, D / 2].  The arithmetic of embeddings.ptq_emb.affine_codes, bit for bit."""
    dev = _lib.require_gpu(table, scale, zero_point)
    if table.dtype != torch.float32 or table.dim() != 2:
        raise TypeError(f"the table must be fp32 [N, D], got {table.dtype} {tuple(table.shape)}")
    storage = torch.int16 if n_bits == 16 else torch.int8
    if zero_point.dtype != storage or zero_point.numel() != 1:
        raise TypeError(f"the zero point of an n_bits = {n_bits} table is one {storage} word, got {zero_point.dtype}")
    N, D = table.shape
    if packed and (n_bits != 4 or D % 2):
        raise ValueError("packing takes n_bits = 4 and an even width")
    if (D > 1 and table.stride(1) != 1) or (N > 1 and table.stride(0) < D):
        table = table.contiguous()
    ldw = table.stride(0) if N > 1 else D
    out = _new_codes((N, D // 2) if packed else (N, D), torch.uint8 if packed else storage, dev)
    _lib.check(
        _lib.load().mi_ptq_quantise(table.data_ptr(), ldw, _kernels._f32c(scale.reshape(1)).data_ptr(), zero_point.data_ptr(),
                                    int(n_bits), int(packed), out.data_ptr(), N, D, _lib.stream_ptr(dev)),
        "mi_ptq_quantise",
    )
    return out


def int4_repack(W, D: int, unpack: bool):
    """int8 codes [N, D] -> packed uint8 [N, D / 2] (unpack False), or back (mi_int4_repack).  A code outside [-8, 7] is
    refused through the error word (_lib.check_index_errors raises ValueError): nothing is read back here."""
    dev = _lib.require_gpu(W)
    D = int(D)
    if unpack:
        src = _packed4(W, D)
        out = _new_codes((src.shape[0], D), torch.int8, dev)
    else:
        if W.dtype != torch.int8 or W.dim() != 2 or W.shape[1] != D or D % 2:
            raise ValueError(f"packing takes int8 codes [N, D] of an even D = {D}, got {W.dtype} {tuple(W.shape)}")
        src = W.contiguous()
        out = _new_codes((src.shape[0], D // 2), torch.uint8, dev)
    _lib.check(
        _lib.load().mi_int4_repack(src.data_ptr(), out.data_ptr(), int(unpack), src.shape[0], D,
                                   _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
        "mi_int4_repack",
    )
    return out

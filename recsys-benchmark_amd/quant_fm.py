"""DeepFM's fused lookup + FM + first-order launch on the quantised tables (csrc/gather_fm_quant.hip).

gather_fm_quant: the post-training-quantised tables (PTQEmb_Int, PTQEmb_Fp16) — fp16 / int8 / int16 codes dequantised
    inside the launch; inference only, like _kernels.gather_rows_quant.
gather_fm_qat: the quantisation-aware-training table (QAT_EmbInt) — the fp32 rows rounded stochastically inside the launch;
    one autograd node whose backward is one row-form launch (mi_gather_fm_qat_bwd_rows) feeding _kernels._table_grads, so
    a row-form table gets COO gradients, a dense one the scatter of those values, and deterministic mode their sorted
    fixed-order sum: no float atomic on DeepFM + QAT in that mode.

Buffers come from the package's float allocator (layer_dcn._new); the int64 row ids the backward needs are written by
the forward launch into an int64 view of such a buffer.
"""
from typing import Optional

import torch

from . import _kernels, _lib
from . import losses as _losses
from .layer_dcn import _int64_rows, _new

QTYPES = {torch.float16: 1, torch.int8: 2, torch.int16: 3}      # the qtype codes of mi_gather_rows_quant
QAT_BWD_MAX_D = 256                                            # MI_GATHER_FM_QAT_BWD_MAX_D
SCALE_GRAD_MAX_BITS = 21      # the backward recovers the rounded code as rintf(emb / scale): exact for |code| <= 2^20


def gather_fm_quant(idx, offsets, Wq, w1, bias, scale=None, zero_point=None):
    """(emb fp32[B, F, D], y_fm[B]) of DeepFM over a quantised table in one launch (mi_gather_fm_quant_fwd):
    emb[b, f] = dequant(Wq[idx[b, f] + offsets[f]]) — (code - zero_point) * scale for int8 / int16 codes, the value itself
    for fp16 —, y_fm the FM second-order term of emb plus the first-order bag over w1 plus bias.  offsets may be None.
    No autograd: inference only."""
    dev = _lib.require_gpu(idx, offsets, Wq, w1, bias, scale, zero_point)
    qtype = QTYPES.get(Wq.dtype)
    if qtype is None:
        raise TypeError(f"unsupported quantised table dtype {Wq.dtype}")
    if Wq.dim() != 2:
        raise ValueError(f"the table must be [N, D], got {tuple(Wq.shape)}")
    if qtype != 1:
        if scale is None or zero_point is None:
            raise ValueError("an integer table needs its scale and zero point")
        if zero_point.dtype != Wq.dtype:
            raise TypeError(f"the zero point is held in the table's type {Wq.dtype}, got {zero_point.dtype}")
        scale = _kernels._f32c(scale.reshape(1))
        zero_point = zero_point.reshape(1)
    else:
        scale = zero_point = None
    # (a view that is row-contiguous is read in place, wherever it starts: the launch picks the scalar kernels for a base
    #  that is not on a four-code boundary)
    Wc = Wq if Wq.is_contiguous() else Wq.contiguous()
    N, D = Wc.shape
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

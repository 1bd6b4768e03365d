"""torch.autograd glue over the C-ABI (include/mi355x_recsys.h).

PyTorch is plumbing here: it owns the device buffers and the stream; every
arithmetic step of the hot path runs in libmi355x_recsys.so.
"""
import collections
import ctypes as _ctypes
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from . import losses as _losses      # (the kept ticket workspaces; it imports this module in turn: neither uses the other at import)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    return t.contiguous()


def _float4_rows(D: int) -> bool:
    """Row widths the float4 kernels take (csrc: vec_ok): D = 4 * 2^k <= 256."""
    return D % 4 == 0 and 4 <= D <= 256 and ((D // 4) & (D // 4 - 1)) == 0


def _row_strided(t: torch.Tensor, align: int = 4):
    """(tensor, row stride in floats) of a 2-D fp32 table the kernels can read in place: unit stride inside a row, any
    row stride that is a multiple of `align` floats (4 keeps float4 row accesses 16-byte aligned) — a column-slice view
    of a packed table, DeepFM.pack_tables(); anything else is made contiguous."""
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    if (t.dim() == 2 and t.shape[0] > 1 and (t.shape[1] == 1 or t.stride(1) == 1) and t.stride(0) >= t.shape[1]
            and t.stride(0) % align == 0 and (t.data_ptr() % (4 * align)) == 0):
        return t, int(t.stride(0))
    t = t.contiguous()
    return t, int(t.shape[1]) if t.dim() == 2 else 1


def _i64c(t: torch.Tensor) -> torch.Tensor:
    # the reference's datasets hand over int32 or int64 ids and `x + offsets`
    # promotes to int64 (src/models/deepfm.py:88); same here.
    if t.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"expected an integer index tensor, got {t.dtype}")
    return t.to(torch.int64).contiguous()


def _lookup_operands(idx, offsets, w1, N: Optional[int] = None):
    """(idx int64[B, F], offsets int64[F] or None, w1 and its row stride, N) as the fused lookup launches read them: w1
    ([N], [N, 1], or a column of a packed table) in place where its rows are evenly strided, one weight per row of the
    N-row embedding table (N=None: the first-order table says how many rows there are)."""
    idx = _i64c(idx)
    if offsets is not None:
        offsets = _i64c(offsets.reshape(-1))
    if idx.dim() != 2 or (offsets is not None and idx.shape[1] != offsets.numel()):
        raise ValueError(f"idx must be [B, F] with one offset per field, got {tuple(idx.shape)}")
    w1c, ldw1 = _row_strided(w1.reshape(w1.shape[0], -1) if w1.dim() != 2 else w1, align=1)
    if N is None:
        N = int(w1c.shape[0])
    if w1c.shape[0] != N or w1c.numel() != N:
        raise ValueError("first-order table must have one weight per embedding row")
    return idx, offsets, w1c, ldw1, N


def _upstream(g_emb, g_y, B: int, dev):
    """(g_emb, g_y) as the backward launches read them: fp32 and contiguous, zeros for a y_fm that nothing used (the
    forwards switch gradient materialisation off), None for an emb that nothing used."""
    g_y = torch.zeros((B,), dtype=torch.float32, device=dev) if g_y is None else _f32c(g_y)
    return (None if g_emb is None else _f32c(g_emb)), g_y


def _bias_grad(gb, g_y, B: int, launched: bool = True):
    """The bias gradient (sum of g_y) of a lookup's backward.  gb (fp32 [1], None when it is not wanted) rides in the
    backward launch; a backward that launched nothing sums g_y itself, and a launch over no sample wrote nothing."""
    if gb is None:
        return None
    if not launched:
        return g_y.sum().view(1)
    if B == 0:
        gb.zero_()
    return gb


def _coo(rows: torch.Tensor, vals: torch.Tensor, shape) -> torch.Tensor:
    return torch.sparse_coo_tensor(rows.view(1, -1), vals, shape, check_invariants=False)


# Row ids that came from a multi-field lookup (rows[b, f] = x[b, f] + offsets[f]) and may later head a row-form
# gradient: the optimizer can sort them field by field in LDS (mi_sort_field_rows) instead of generically.  The entry
# holds the ids tensor itself, so its storage — and with it the pointer used as the key — cannot be recycled while the
# entry lives; only the last few lookups are kept.
_field_layouts: "collections.OrderedDict[int, tuple]" = collections.OrderedDict()


def note_field_layout(rows: torch.Tensor, offsets: torch.Tensor, N: int) -> None:
    """rows int64[B, F] = x + offsets (offsets ascending, field f's ids in [offsets[f], offsets[f+1]), the last below N)."""
    if rows.dim() != 2 or not rows.is_contiguous() or rows.dtype != torch.int64 or not rows.is_cuda:
        return
    offsets = offsets.reshape(-1)
    _field_layouts[rows.data_ptr()] = (rows, offsets, N)
    _field_layouts.move_to_end(rows.data_ptr())
    while len(_field_layouts) > 4:
        _field_layouts.popitem(last=False)


def sort_field_rows(rows_flat: torch.Tensor, N: int):
    """(sorted ids, permutation) of a flat view of ids noted by a multi-field lookup, or None when the ids are not known
    to have that layout (or exceed the LDS sort's limits) and the caller has to sort them generically."""
    entry = _field_layouts.get(rows_flat.data_ptr())
    if entry is None:
        return None
    rows, offsets, n_rows = entry
    B, F = rows.shape
    if rows_flat.numel() != B * F or n_rows != N:
        return None
    return _sort_fields(rows, offsets, N, B, F)


def _sort_fields(rows: torch.Tensor, offsets: torch.Tensor, N: int, B: int, F: int):
    """(sorted ids, permutation), both flat, of contiguous ids rows[B, F] = x + offsets (ascending offsets) sorted field by
    field in LDS (mi_sort_field_rows), or None beyond that sort's limits."""
    if not 0 < B <= 65536 or N >= 2**32 - 2:
        return None
    lib = _lib.load()
    rows_sorted, perm = rows.new_empty(B * F), rows.new_empty(B * F)
    nbytes = int(lib.mi_sort_field_rows_workspace_bytes(B, F))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=rows.device) if nbytes else None
    _lib.check(lib.mi_sort_field_rows(rows.data_ptr(), offsets.data_ptr(), N, B, F, rows_sorted.data_ptr(),
                                      perm.data_ptr(), _lib.ptr(ws), _lib.err_word(rows.device).data_ptr(),
                                      _lib.stream_ptr(rows.device)), "mi_sort_field_rows")
    return rows_sorted, perm


MASKED_MAX_D = 255      # MI_GATHER_FM_MASKED_MAX_D: a kept width is one byte


def _mask_operands(keep, fwidth, N: int, F: int):
    """The two width sources of the masked gather_fm as the kernels read them: keep uint8 [N], fwidth int32 [F]."""
    if keep is not None:
        if keep.dtype != torch.uint8 or keep.numel() != N:
            raise ValueError(f"keep must be uint8 [{N}], got {keep.dtype} {tuple(keep.shape)}")
        keep = keep.contiguous()
    if fwidth is not None:
        if fwidth.dtype != torch.int32 or fwidth.numel() != F:
            raise ValueError(f"fwidth must be int32 [{F}], got {fwidth.dtype} {tuple(fwidth.shape)}")
        fwidth = fwidth.contiguous()
    return keep, fwidth


XFORM_MAX_D = 256       # the row-form backward of the PEP forms (mi_gather_fm_soft_bwd_rows / _elemmask_bwd_rows)


def _soft_strides(s: torch.Tensor, N: int, D: int):
    """(row stride, column stride) of a PEP threshold that broadcasts over a [N, D] table: [1], [D], [N,1] or [N,D]."""
    if s.numel() == 1:
        return 0, 0
    if s.dim() == 1 and s.shape[0] == D:
        return 0, 1
    if tuple(s.shape) == (N, 1):
        return 1, 0
    if tuple(s.shape) == (N, D):
        return D, 1
    raise ValueError(f"threshold of shape {tuple(s.shape)} does not broadcast over a [{N},{D}] table")


class GatherFM(torch.autograd.Function):
    """emb, y_fm = gather+FM+first-order (src/models/deepfm.py:88-98) in one kernel.

    sparse_W / sparse_w1 choose the gradient form of the two tables: row form
    (uncoalesced COO, what nn.Embedding(sparse=True) yields) or the reference's
    default dense weight.grad.

    keep (uint8 [N]) / fwidth (int32 [F]), either or both: the kept-width form (mi_gather_fm_masked_*) —
    emb[b, f, d] = W[row, d] for d < min(keep[row], fwidth[f]) and +0 past it, y_fm over the masked emb, the first-order
    term unmasked; the table's gradient is exactly zero at the masked positions.  With both None every call is the
    unmasked one.

    soft (fp32 [1], [D], [N,1] or [N,D], an autograd input) / elem_mask (bool or uint8 [N, D]): the PEP forms
    (mi_gather_fm_soft_* / mi_gather_fm_elemmask_*) — emb = sign(w) relu(|w| - sigmoid(s)), or emb = mask ? w : +0;
    y_fm over that emb, the first-order term untouched.  The backward is one row-form launch over the saved emb; dense
    gradients (W's, and a row-shaped threshold's) are scattered from its values — in a fixed order in deterministic
    mode —, sparse_W asks for them in COO form.  A [D] or [1] threshold's gradient leaves the launch complete.
    """

    @staticmethod
    def forward(ctx, idx, offsets, W, w1, bias, sparse_W: bool, sparse_w1: bool, keep=None, fwidth=None, soft=None,
                elem_mask=None):
        dev = _lib.require_gpu(idx, offsets, W, w1, bias, keep, fwidth, soft, elem_mask)
        lib = _lib.load()
        masked = keep is not None or fwidth is not None
        if (soft is not None) + (elem_mask is not None) + masked > 1:
            raise ValueError("gather_fm: keep / fwidth, soft and elem_mask exclude each other")
        xform = soft is not None or elem_mask is not None
        if xform and W.shape[-1] > XFORM_MAX_D:
            raise NotImplementedError(f"the soft / elem_mask gather_fm backward covers D <= {XFORM_MAX_D}, got {W.shape[-1]}")
        if masked and W.shape[-1] > MASKED_MAX_D:
            raise NotImplementedError(f"the masked gather_fm keeps one byte per width: D <= {MASKED_MAX_D}, got "
                                      f"{W.shape[-1]}")
        if _float4_rows(W.shape[-1]):
            Wc, ldw = _row_strided(W)
        else:       # widths the float4 kernels do not cover run on the scalar kernels, which read the two plain tensors
            Wc, w1 = _f32c(W), _f32c(w1)
            ldw = int(Wc.shape[-1])
        N, D = Wc.shape
        idx, offsets, w1c, ldw1, _ = _lookup_operands(idx, offsets, w1, N)
        B, F = idx.shape
        emb = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        yfm = torch.empty((B,), dtype=torch.float32, device=dev)
        rows = torch.empty((B, F), dtype=torch.int64, device=dev)
        # one launch: the form chooses the entry point and what goes between the operands and the outputs
        ctx.xform = None
        if soft is not None:
            srs, scs = _soft_strides(soft, N, D)
            Sc = _f32c(soft)
            name, mid = "mi_gather_fm_soft_fwd", (Sc.data_ptr(), srs, scs)
            ctx.xform = ("soft", srs, scs, tuple(soft.shape))
        elif elem_mask is not None:
            if elem_mask.dtype not in (torch.bool, torch.uint8) or tuple(elem_mask.shape) != (N, D):
                raise ValueError(f"elem_mask must be bool or uint8 [{N}, {D}], got {elem_mask.dtype} {tuple(elem_mask.shape)}")
            Mc = elem_mask.contiguous().view(torch.uint8)      # (a bool is one byte, 0 or 1: read in place)
            name, mid = "mi_gather_fm_elemmask_fwd", (Mc.data_ptr(),)
            ctx.xform = ("mask", Mc)
        elif masked:
            keep, fwidth = _mask_operands(keep, fwidth, N, F)
            name, mid = "mi_gather_fm_masked_fwd", (_lib.ptr(keep), _lib.ptr(fwidth))
        else:
            name, mid = "mi_gather_fm_fwd_ld", ()
        _lib.check(
            getattr(lib, name)(
                idx.data_ptr(), offsets.data_ptr(), Wc.data_ptr(), ldw, w1c.data_ptr(), ldw1, _lib.ptr(bias), *mid,
                emb.data_ptr(), yfm.data_ptr(), rows.data_ptr(), B, F, D, N, _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev),
            ),
            name,
        )
        if sparse_W or sparse_w1 or DETERMINISTIC:
            note_field_layout(rows, offsets, N)
        # (the threshold is an autograd input: saved, so that an in-place update before the backward raises)
        ctx.save_for_backward(emb, rows, *((Sc,) if soft is not None else ()))
        ctx.mask = (keep, fwidth) if masked else None      # (constants of the step, not autograd inputs)
        ctx.shapes = (B, F, D, N, tuple(W.shape), tuple(w1.shape))
        ctx.sparse = (sparse_W, sparse_w1)
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(rows)
        return emb, yfm, rows

    @staticmethod
    def backward(ctx, g_emb, g_y, _g_rows):
        emb, rows = ctx.saved_tensors[:2]
        B, F, D, N, Wshape, w1shape = ctx.shapes
        sparse_W, sparse_w1 = ctx.sparse
        dev = emb.device
        lib = _lib.load()
        g_emb, g_y = _upstream(g_emb, g_y, B, dev)
        need_W, need_w1 = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gW = gw1 = None
        stream = _lib.stream_ptr(dev)
        if ctx.xform is not None:
            return GatherFM._xform_backward(ctx, emb, rows, g_emb, g_y, need_W, need_w1, stream)
        rows_form = (sparse_W and need_W) or (sparse_w1 and need_w1)
        dense_form = (need_W and not sparse_W) or (need_w1 and not sparse_w1)
        if DETERMINISTIC and dense_form:
            rows_form, dense_form = True, False     # row-form values, then a sorted (ordered) accumulation: no atomics
        # the bias gradient (sum of g_y) rides in whichever backward kernel runs
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if (ctx.has_bias and ctx.needs_input_grad[4]) else None
        # the kept-width form of either launch: the widths in front (and the row-form launch then reads the row ids and N)
        masked = ctx.mask is not None
        widths = (_lib.ptr(ctx.mask[0]), _lib.ptr(ctx.mask[1])) if masked else ()
        upstream = (emb.data_ptr(), g_y.data_ptr(), _lib.ptr(g_emb))
        if rows_form:
            gvals = torch.empty((B * F, D), dtype=torch.float32, device=dev)
            g1vals = torch.empty((B * F,), dtype=torch.float32, device=dev)
            name = "mi_gather_fm_masked_bwd_rows" if masked else "mi_gather_fm_bwd_rows"

            def launch(gvals, g1vals, gb):
                _lib.check(getattr(lib, name)(*((rows.data_ptr(), *widths) if masked else ()), *upstream, gvals.data_ptr(),
                                              g1vals.data_ptr(), _lib.ptr(gb), B, F, D, *((N,) if masked else ()), stream), name)

            gW, gw1, gb, _ = _row_backward(launch, B, rows, gvals, g1vals, gb, N, D, Wshape, w1shape, sparse_W, sparse_w1,
                                           need_W, need_w1, stream)
        elif dense_form:
            gWd = torch.zeros((N, D), dtype=torch.float32, device=dev)
            gw1d = torch.zeros((N,), dtype=torch.float32, device=dev)
            name = "mi_gather_fm_masked_bwd_dense" if masked else "mi_gather_fm_bwd_dense"
            _lib.check(getattr(lib, name)(rows.data_ptr(), *widths, *upstream, gWd.data_ptr(), gw1d.data_ptr(), _lib.ptr(gb),
                                          B, F, D, N, stream), name)
            if need_W:
                gW = gWd.view(Wshape)
            if need_w1:
                gw1 = gw1d.view(w1shape)
        else:                                       # neither table needs a gradient: nothing was launched
            gb = _bias_grad(gb, g_y, B, launched=False)
        return None, None, gW, gw1, gb, None, None, None, None, None, None

    @staticmethod
    def _xform_backward(ctx, emb, rows, g_emb, g_y, need_W, need_w1, stream):
        """The PEP forms: one row-form launch, then the tables' gradients out of its values (_row_backward)."""
        B, F, D, N, Wshape, w1shape = ctx.shapes
        sparse_W, sparse_w1 = ctx.sparse
        dev = emb.device
        lib = _lib.load()
        need_S = ctx.xform[0] == "soft" and ctx.needs_input_grad[9]
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if (ctx.has_bias and ctx.needs_input_grad[4]) else None
        if not (need_W or need_w1 or need_S):
            return (None, None, None, None, _bias_grad(gb, g_y, B, launched=False)) + (None,) * 6
        gvals = torch.empty((B * F, D), dtype=torch.float32, device=dev)
        g1vals = torch.empty((B * F,), dtype=torch.float32, device=dev)
        upstream = (emb.data_ptr(), g_y.data_ptr(), _lib.ptr(g_emb))

        def soft(gvals, g1vals, gb):
            _, srs, scs, Sshape = ctx.xform
            Sc = ctx.saved_tensors[2]
            svals = torch.empty((B * F, D) if srs == D and scs == 1 else (B * F,) if srs else (D,) if scs else (1,),
                                dtype=torch.float32, device=dev)
            ws, armed = (_losses._ticket_workspace("gather_fm_soft", dev, lib.mi_gather_fm_soft_bwd_workspace_elems(B, D, srs))
                         if srs == 0 and B > 0 else (None, True))
            _lib.check(
                lib.mi_gather_fm_soft_bwd_rows(rows.data_ptr(), Sc.data_ptr(), srs, scs, *upstream, gvals.data_ptr(),
                                               svals.data_ptr(), g1vals.data_ptr(), _lib.ptr(gb), _lib.ptr(ws), int(armed),
                                               B, F, D, N, stream),
                "mi_gather_fm_soft_bwd_rows",
            )
            if not need_S:
                return None
            if srs == 0:                      # [D] / [1]: the launch summed it
                return svals.view(Sshape)
            width = D if scs else 1           # [N, D] / [N, 1]: one value row per lookup, like the table's
            return (_coo(rows, svals.view(B * F, *Sshape[1:]), Sshape) if sparse_W
                    else _scatter_rows(rows, svals, N, width, stream).view(Sshape))

        def elemmask(gvals, g1vals, gb):
            _lib.check(
                lib.mi_gather_fm_elemmask_bwd_rows(rows.data_ptr(), ctx.xform[1].data_ptr(), *upstream, gvals.data_ptr(),
                                                   g1vals.data_ptr(), _lib.ptr(gb), B, F, D, N, stream),
                "mi_gather_fm_elemmask_bwd_rows",
            )

        gW, gw1, gb, gS = _row_backward(soft if ctx.xform[0] == "soft" else elemmask, B, rows, gvals, g1vals, gb, N, D, Wshape,
                                        w1shape, sparse_W, sparse_w1, need_W, need_w1, stream)
        return None, None, gW, gw1, gb, None, None, None, None, gS, None


# Deterministic mode (recsys_benchmark_amd.use_deterministic_algorithms): dense table gradients are built by SORTING the
# row ids and adding each row's contributions in a fixed order (mi_coalesce_rows_sorted) instead of float atomics — the
# reference's CPU index_add is deterministic too (src/models/embeddings/base.py:74-75 through autograd) —, the products
# that would split K over atomically accumulating workgroups run unsplit, and the MLP tail runs on the fused kernels of
# csrc/tail.hip (no atomics).  Off by default: the atomic forms are faster.
DETERMINISTIC = False


def _no_atomics_promised(what: str) -> None:
    """use_deterministic_algorithms(True) promises gradients without float atomics; a backward that only exists in the
    atomic form says so instead of handing out gradients that merely look reproducible."""
    if DETERMINISTIC:
        raise NotImplementedError(f"{what} accumulates duplicate rows with float atomics; it has no deterministic form "
                                  "(recsys_benchmark_amd.use_deterministic_algorithms(True) is on)")


def coalesce_dense(rows: torch.Tensor, vals: torch.Tensor, N: int, D: int) -> torch.Tensor:
    """Dense [N, D] gradient of a table out of row-form (rows[n], vals[n, D]) contributions, added in a fixed order."""
    dev = vals.device
    rows = rows.reshape(-1)
    n = rows.numel()
    out = torch.zeros((N, D), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    found = sort_field_rows(rows, N)
    rs, perm = found if found is not None else torch.sort(rows, stable=True)
    acc = torch.empty((n, D), dtype=torch.float32, device=dev)
    vals = _f32c(vals).view(n, D)
    _lib.check(_lib.load().mi_coalesce_rows_sorted(rs.data_ptr(), perm.data_ptr(), vals.data_ptr(), out.data_ptr(), acc.data_ptr(),
                                                   n, D, N, _lib.stream_ptr(dev)), "mi_coalesce_rows_sorted")
    return out


def _scatter_rows(rows, vals, N, D, stream):
    if DETERMINISTIC:
        return coalesce_dense(rows, vals, N, D)
    out = torch.zeros((N, D), dtype=torch.float32, device=vals.device)
    _lib.check(_lib.load().mi_scatter_axpy_rows(rows.data_ptr(), vals.data_ptr(), 1.0, out.data_ptr(), rows.numel(), D, N,
                                                stream), "mi_scatter_axpy_rows")
    return out


def _table_grads(rows, gvals, g1vals, N, D, Wshape, w1shape, sparse_W, sparse_w1, need_W, need_w1, stream):
    """(gW, gw1) of the two lookup tables from the row-form values gvals[B*F, D] / g1vals[B*F] at `rows`.  A table that
    wants a dense gradient next to one in row form (the reference's sparse config keeps the first-order table dense)
    gets the values just computed scatter-added — never a second pass over a zeroed [N, D]."""
    gW = gw1 = None
    if need_W:
        gW = _coo(rows, gvals, Wshape) if sparse_W else _scatter_rows(rows, gvals, N, D, stream).view(Wshape)
    if need_w1:
        gw1 = (_coo(rows, g1vals.view((-1,) + (1,) * (len(w1shape) - 1)), w1shape) if sparse_w1
               else _scatter_rows(rows, g1vals, N, 1, stream).view(w1shape))
    return gW, gw1


def _row_backward(launch, B: int, rows, gvals, g1vals, gb, *tables):
    """The row-form backward of a fused lookup: ONE launch that writes a value row per lookup into the caller's gvals /
    g1vals (and sums the bias gradient into its gb), then the two tables' gradients out of those values.
    launch(gvals, g1vals, gb) issues the form's kernel and returns the gradient it produces besides (a threshold's, a
    scale's) or None; `tables` is what _table_grads takes behind the values.  -> (gW, gw1, gb, launch's extra)."""
    extra = launch(gvals, g1vals, gb)
    gW, gw1 = _table_grads(rows, gvals, g1vals, *tables)
    return gW, gw1, _bias_grad(gb, None, B), extra


def gather_fm(idx, offsets, W, w1, bias, sparse_W=False, sparse_w1=False, keep=None, fwidth=None, soft=None, elem_mask=None):
    emb, yfm, _rows = GatherFM.apply(idx, offsets, W, w1, bias, sparse_W, sparse_w1, keep, fwidth, soft, elem_mask)
    return emb, yfm


def soft_count_kept(W: torch.Tensor, s: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device int64 [1]: the number of non-zeros of sign(W) relu(|W| - sigmoid(s)), counted in one pass over W and s
    (mi_soft_count_kept) — no thresholded copy of the table.  out (optional): the int64 [1] to write, e.g. one element of
    a tensor that collects several tables' counts for one host read."""
    dev = _lib.require_gpu(W, s, out)
    Wc, Sc = _f32c(W), _f32c(s)
    N, D = Wc.shape
    srs, scs = _soft_strides(s, N, D)
    if out is not None and (out.dtype != torch.int64 or out.numel() != 1):
        raise ValueError(f"out must be int64 [1], got {out.dtype} {tuple(out.shape)}")
    count = torch.empty(1, dtype=torch.int64, device=dev) if out is None else out
    _lib.check(_lib.load().mi_soft_count_kept(Wc.data_ptr(), Sc.data_ptr(), srs, scs, N, D, count.data_ptr(),
                                              _lib.stream_ptr(dev)), "mi_soft_count_kept")
    return count


class GatherRows(torch.autograd.Function):
    """out[i,:] = W[idx[i],:]  (nn.Embedding, src/models/embeddings/base.py:74-75)."""

    @staticmethod
    def forward(ctx, idx, W, sparse: bool):
        dev = _lib.require_gpu(idx, W)
        lib = _lib.load()
        idxc = _i64c(idx)
        Wc = _f32c(W)
        N, D = Wc.shape
        n = idxc.numel()
        out = torch.empty(tuple(idx.shape) + (D,), dtype=torch.float32, device=dev)
        _lib.check(
            lib.mi_gather_rows_fwd(idxc.data_ptr(), Wc.data_ptr(), out.data_ptr(), n, D, N,
                                   _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
            "mi_gather_rows_fwd",
        )
        ctx.save_for_backward(idxc)
        ctx.meta = (n, D, N, tuple(W.shape), sparse)
        return out

    @staticmethod
    def backward(ctx, g):
        (idxc,) = ctx.saved_tensors
        n, D, N, Wshape, sparse = ctx.meta
        if not ctx.needs_input_grad[1]:
            return None, None, None
        g = _f32c(g).view(n, D)
        if sparse:
            return None, _coo(idxc.view(-1), g, Wshape), None
        if DETERMINISTIC:
            return None, coalesce_dense(idxc, g, N, D).view(Wshape), None
        gW = torch.zeros((N, D), dtype=torch.float32, device=g.device)
        _lib.check(
            _lib.load().mi_scatter_add_rows(idxc.data_ptr(), g.data_ptr(), gW.data_ptr(), n, D, N,
                                            _lib.stream_ptr(g.device)),
            "mi_scatter_add_rows",
        )
        return None, gW.view(Wshape), None


def gather_rows(idx: torch.Tensor, W: torch.Tensor, sparse: bool = False) -> torch.Tensor:
    return GatherRows.apply(idx, W, sparse)


def bag_reduce(rows: torch.Tensor, mode: Optional[str]) -> torch.Tensor:
    """EmbeddingBag semantics for a 2-D index tensor: every row of the input is a bag
    (src/models/embeddings/base.py:58-63).  rows: [B, L, D]."""
    if mode is None:
        return rows
    if rows.dim() != 3:
        raise ValueError("bag modes need a 2-D index tensor (one bag per row)")
    if mode == "sum":
        return rows.sum(1)
    if mode == "mean":
        return rows.mean(1)
    if mode == "max":
        return rows.max(1)[0]
    raise ValueError(f"unknown mode {mode}")


# --------------------------------------------------------------------------------------
# FM + first-order over an already gathered emb (DeepFM on a compressed table)
class FMFirstOrder(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, rows, w1, bias, sparse_w1: bool):
        dev = _lib.require_gpu(emb, rows, w1, bias)
        embc, rowsc, w1c = _f32c(emb), _i64c(rows), _f32c(w1)
        B, F, D = embc.shape
        N = w1c.numel()
        yfm = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.check(
            _lib.load().mi_fm_fwd(embc.data_ptr(), rowsc.data_ptr(), w1c.data_ptr(), _lib.ptr(bias),
                                  yfm.data_ptr(), B, F, D, N, _lib.err_word(dev).data_ptr(),
                                  _lib.stream_ptr(dev)),
            "mi_fm_fwd",
        )
        ctx.save_for_backward(embc, rowsc)
        ctx.meta = (B, F, D, N, tuple(w1.shape), sparse_w1, bias is not None)
        return yfm

    @staticmethod
    def backward(ctx, g_y):
        embc, rowsc = ctx.saved_tensors
        B, F, D, N, w1shape, sparse_w1, has_bias = ctx.meta
        dev = embc.device
        lib = _lib.load()
        _, g_y = _upstream(None, g_y, B, dev)
        stream = _lib.stream_ptr(dev)
        g_emb = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        g1vals = torch.empty((B * F,), dtype=torch.float32, device=dev)
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if (has_bias and ctx.needs_input_grad[3]) else None
        _lib.check(
            lib.mi_gather_fm_bwd_rows(embc.data_ptr(), g_y.data_ptr(), None, g_emb.data_ptr(),
                                      g1vals.data_ptr(), _lib.ptr(gb), B, F, D, stream),
            "mi_gather_fm_bwd_rows",
        )
        gw1 = None
        if ctx.needs_input_grad[2]:
            if sparse_w1:
                gw1 = _coo(rowsc, g1vals.view((-1,) + (1,) * (len(w1shape) - 1)), w1shape)
            else:
                gw1 = torch.zeros((N,), dtype=torch.float32, device=dev)
                _lib.check(lib.mi_scatter_add_rows(rowsc.data_ptr(), g1vals.data_ptr(), gw1.data_ptr(),
                                                   B * F, 1, N, stream), "mi_scatter_add_rows")
                gw1 = gw1.view(w1shape)
        return (g_emb if ctx.needs_input_grad[0] else None), None, gw1, _bias_grad(gb, g_y, B), None


def fm_first_order(emb, rows, w1, bias, sparse_w1=False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(emb, y_fm) for DeepFM when emb came from any IEmbedding (src/models/deepfm.py:91-98)."""
    if emb.dim() != 3 or tuple(rows.shape) != tuple(emb.shape[:2]):
        return emb, _fm_first_order_mismatched(emb, rows, w1, bias, sparse_w1)
    return emb, FMFirstOrder.apply(emb, rows, w1, bias, sparse_w1)


def _fm_first_order_mismatched(emb, rows, w1, bias, sparse_w1):
    """QR with operation="cat": emb is [B, 2F, D/2] while the ids are [B, F].  The second-order term runs
    over emb's own shape (mi_fm_fwd with an all-zero first-order table), the first-order bag over the
    real ids (a D=1 row gather summed per sample)."""
    B = emb.shape[0]
    zero_rows = torch.zeros((B, emb.shape[1]), dtype=torch.int64, device=emb.device)
    zero_w1 = torch.zeros((1,), dtype=torch.float32, device=emb.device)
    second = FMFirstOrder.apply(emb, zero_rows, zero_w1, None, False)
    lin = GatherRows.apply(rows, w1.view(-1, 1), sparse_w1).sum(dim=(1, 2))
    return second + lin + (bias if bias is not None else 0.0)


# --------------------------------------------------------------------------------------
OPS = {"mult": 0, "add": 1, "cat": 2}
XF_NONE, XF_SOFT, XF_MASK = 0, 1, 2


def _byte_mask(m: torch.Tensor) -> torch.Tensor:
    return m.contiguous().view(torch.uint8) if m.dtype in (torch.bool, torch.uint8) else m.to(torch.uint8).contiguous()


def _dual_operands(T1, T2, S1, S2, M1, M2, what: str = "dual_gather"):
    """(T1, T2, S1, S2, M1, M2, xform, De, n1, n2) as every launch of the two-table family (QR, CERP, CERP retrain) reads
    them: contiguous fp32 tables [n1, De] and [n2, De]; XF_SOFT with the threshold logits S1 / S2 or XF_MASK with the
    masks M1 / M2, each shaped like its table, else XF_NONE.  A bool or uint8 mask is read in place (a bool is one byte,
    0 or 1); a mask of another dtype is converted."""
    if (S1 is None) != (S2 is None) or (M1 is None) != (M2 is None):
        raise ValueError(f"{what}: the thresholds S1 / S2 (and the masks M1 / M2) come in pairs")
    if S1 is not None and M1 is not None:
        raise ValueError(f"{what}: soft (S1 / S2) and mask (M1 / M2) exclude each other")
    s1, s2 = T1.shape, T2.shape
    if len(s1) != 2 or len(s2) != 2 or s1[1] != s2[1]:
        raise ValueError(f"{what}: both tables must share the row width, got {tuple(s1)} and {tuple(s2)}")
    for name, t, shape in (("S1", S1, s1), ("S2", S2, s2), ("M1", M1, s1), ("M2", M2, s2)):
        if t is not None and t.shape != shape:
            raise ValueError(f"{what}: {name} must be shaped like its table {tuple(shape)}, got {tuple(t.shape)}")
    if S1 is not None:
        return _f32c(T1), _f32c(T2), _f32c(S1), _f32c(S2), None, None, XF_SOFT, s1[1], s1[0], s2[0]
    if M1 is not None:
        return _f32c(T1), _f32c(T2), None, None, _byte_mask(M1), _byte_mask(M2), XF_MASK, s1[1], s1[0], s2[0]
    return _f32c(T1), _f32c(T2), None, None, None, None, XF_NONE, s1[1], s1[0], s2[0]


class DualGather(torch.autograd.Function):
    """out = T1'[idx % mod1] (op) T2'[idx // div2]  (mi_dual_gather_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, idx, T1, T2, S1, S2, M1, M2, mod1: int, div2: int, op: int, fields=None, sparse2: bool = False, offsets=None):
        """offsets ([F], optional): idx holds the model's raw per-field ids and the per-field row offsets are added inside
        the lookup; the second output is then the row ids idx + offsets (int64, not differentiable)."""
        dev = _lib.require_gpu(idx, T1, T2)
        idxc = _i64c(idx)
        T1c, T2c, S1c, S2c, M1c, M2c, xform, De, n1, n2 = _dual_operands(T1, T2, S1, S2, M1, M2)
        n = idxc.numel()
        F = idx.shape[1] if idx.dim() == 2 else 1
        if op == OPS["cat"]:
            if idx.dim() == 1:
                oshape = (idx.shape[0], 2 * De)
            elif idx.dim() == 2:
                oshape = (idx.shape[0], 2 * F, De)
            else:
                raise ValueError("cat supports 1-D or 2-D index tensors")
        else:
            oshape = tuple(idx.shape) + (De,)
        out = torch.empty(oshape, dtype=torch.float32, device=dev)
        rows = None
        if offsets is not None:
            if idx.dim() != 2 or offsets.numel() != F:
                raise ValueError("offsets go with [B, F] ids, one per field")
            offs = _i64c(offsets.reshape(-1))
            rows = torch.empty_like(idxc)
        _lib.check(
            _lib.load().mi_dual_gather_fwd_off(
                idxc.data_ptr(), _lib.ptr(offs) if rows is not None else None, _lib.ptr(rows), T1c.data_ptr(), T2c.data_ptr(),
                _lib.ptr(S1c), _lib.ptr(S2c), _lib.ptr(M1c), _lib.ptr(M2c), out.data_ptr(), n, F, De, n1, n2,
                mod1, div2, op, xform, _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
            "mi_dual_gather_fwd_off",
        )
        if rows is not None:
            idxc = rows              # the backward reads the finished row ids
            ctx.mark_non_differentiable(rows)
            # (autograd would otherwise hand the backward a ZERO-FILLED int64 [B, F] "gradient" for the row ids: a fill launch
            #  per step for a tensor nobody reads)
            ctx.set_materialize_grads(False)
        ctx.save_for_backward(idxc, T1c, T2c, S1c, S2c, M1c, M2c)
        ctx.meta = (n, F, De, mod1, div2, op, xform)
        ctx.fields = fields if (fields is not None and idx.dim() == 2 and fields[3] == F) else None
        ctx.sparse2 = bool(sparse2) and xform == XF_NONE
        ctx.t2_shape = tuple(T2.shape)
        ctx.with_rows = rows is not None
        return (out, rows) if rows is not None else out

    @staticmethod
    def backward(ctx, g, _g_rows=None):
        if g is None:                # (materialisation is off when the row ids are a second output: nothing flowed back)
            return (None,) * 13
        idxc, *tables = ctx.saved_tensors
        n, F, De, mod1, div2, op, xform = ctx.meta
        _no_atomics_promised("the two-table (QR / CERP) gather backward")
        ops = (*tables, xform, De, tables[0].shape[0], tables[1].shape[0])
        grads = _dual_scatter_backward(idxc, _f32c(g), ops, n, F, op, mod1, div2, ctx.fields, ctx.sparse2, ctx.t2_shape)
        return (None,) + grads + (None,) * 8


def _dual_scatter_backward(ids, g, ops, n: int, F: int, op: int, mod1: int, div2: int, fields, rows_form: bool, t2_shape):
    """(gT1, gT2, gS1, gS2) of n two-table lookups in default mode (float atomics): ids int64 [n], g their upstream
    gradient rows (fp32, contiguous), ops as _dual_operands returns them, fields the small-field hint or None."""
    T1c, T2c, S1c, S2c, M1c, M2c, xform, De, n1, n2 = ops
    lib, dev = _lib.load(), g.device
    if rows_form:
        # table 2 (the quotient table: ~N / divider rows) gets its gradient in ROW form: one value row per lookup, no
        # atomics into scattered rows and no [n2, De] zero-fill; table 1 (divider rows) stays dense
        ws = _dual_rows_workspace(dev, De, n1)
        g2vals = torch.empty((n, De), dtype=torch.float32, device=dev)
        gT1 = _dual_rows_grad1(ws, De, T1c, g, T2c, g2vals)
        rows2 = torch.empty((n,), dtype=torch.int64, device=dev)
        _lib.check(lib.mi_dual_gather_bwd_rows(ids.data_ptr(), g.data_ptr(), T1c.data_ptr(), T2c.data_ptr(), gT1.data_ptr(),
                                               g2vals.data_ptr(), rows2.data_ptr(), n, F, De, n1, n2, mod1, div2, op,
                                               _lib.ptr(ws), _lib.stream_ptr(dev)), "mi_dual_gather_bwd_rows")
        # (ids out of range carry row 0 and a zero value row: they add nothing)
        return gT1, _coo(rows2, g2vals, t2_shape), None, None
    gT1, gT2 = torch.zeros_like(T1c), torch.zeros_like(T2c)
    gS1 = torch.zeros_like(S1c) if xform == XF_SOFT else None
    gS2 = torch.zeros_like(S2c) if xform == XF_SOFT else None
    small, row0, flags = fields[:3] if fields is not None else (None, None, None)
    _lib.check(
        lib.mi_dual_gather_bwd_fields(
            ids.data_ptr(), g.data_ptr(), T1c.data_ptr(), T2c.data_ptr(), _lib.ptr(S1c), _lib.ptr(S2c),
            _lib.ptr(M1c), _lib.ptr(M2c), gT1.data_ptr(), gT2.data_ptr(), _lib.ptr(gS1), _lib.ptr(gS2),
            n, F, De, n1, n2, mod1, div2, op, xform, _lib.ptr(small),
            small.numel() if small is not None else 0, _lib.ptr(row0), _lib.ptr(flags), _lib.stream_ptr(dev)),
        "mi_dual_gather_bwd_fields",
    )
    return gT1, gT2, gS1, gS2


_DUAL_WS = {}


def _dual_rows_workspace(dev, De: int, n1: int):
    """The persistent join workspace of mi_dual_gather_bwd_rows for this device and shape (its ticket word is zero between
    launches: allocated zeroed once, the kernel resets it), or None when the shape has no use for one."""
    key = (str(dev), int(De), int(n1))
    if key not in _DUAL_WS:
        ne = int(_lib.load().mi_dual_gather_bwd_rows_workspace_elems(De, n1))
        _DUAL_WS[key] = torch.zeros((ne,), dtype=torch.float32, device=dev) if ne else None
    return _DUAL_WS[key]


DUAL_ROWS_FORM_WORKSPACE = 2      # MI_DUAL_ROWS_FORM_WORKSPACE


def _dual_rows_grad1(ws, De: int, T1c, g, T2c, g2vals):
    """The buffer mi_dual_gather_bwd_rows gets for table 1's dense gradient: the library says which form a launch with
    these operands takes (mi_dual_gather_bwd_rows_form), and only the form joined through the workspace WRITES gT1; the
    other two add into it.  (No lookup: nothing is launched and nothing written.)"""
    written = (ws is not None and g2vals.shape[0] > 0
               and _lib.load().mi_dual_gather_bwd_rows_form(g.data_ptr(), T1c.data_ptr(), T2c.data_ptr(), g2vals.data_ptr(),
                                                            ws.data_ptr(), De, T1c.shape[0]) == DUAL_ROWS_FORM_WORKSPACE)
    return torch.empty_like(T1c) if written else torch.zeros_like(T1c)


SMALL_FIELD_ROWS = 16     # kSmallRows of csrc/embed.hip


def small_field_hint(field_dims, div2: int, device):
    """The `fields` hint of dual_gather for ids that are per-field ids + cumulative offsets (how the CTR models address one
    shared table): (small field indices int32, first table-2 row of every field int64, flags uint8, F), or None when no
    field is small.  A field is small when its ids reach at most 16 rows of table 2 (idx // div2)."""
    if isinstance(field_dims, int) or len(field_dims) == 0:
        return None
    off, row0, small = 0, [], []
    for f, card in enumerate(field_dims):
        lo, hi = off // div2, (off + card - 1) // div2
        row0.append(lo)
        if hi - lo + 1 <= SMALL_FIELD_ROWS:
            small.append(f)
        off += card
    if not small:
        return None
    flags = torch.zeros(len(field_dims), dtype=torch.uint8)
    flags[small] = 1
    return (torch.tensor(small, dtype=torch.int32, device=device), torch.tensor(row0, dtype=torch.int64, device=device),
            flags.to(device), len(field_dims))


def dual_gather(idx, T1, T2, mod1, div2, op="add", S1=None, S2=None, M1=None, M2=None, fields=None, sparse2=False, offsets=None):
    """fields (optional): small_field_hint(...) — lets the backward sum the gradient of low-cardinality fields per field
    instead of with thousands of same-address atomics; same result up to the order of float additions.
    offsets (optional, [F]): idx holds raw per-field ids; returns (out, idx + offsets), the addition done by the lookup."""
    return DualGather.apply(idx, T1, T2, S1, S2, M1, M2, int(mod1), int(div2), OPS[op], fields, bool(sparse2), offsets)


class DualTable(torch.autograd.Function):
    """out[i] = T1'[i % mod1] (op) T2'[i // div2] for i = 0 .. N-1 (mi_dual_table_fwd / _bwd): the whole table, no index
    tensor; the backward writes every gradient element once, in a fixed order, without atomics."""

    @staticmethod
    def forward(ctx, T1, T2, S1, S2, M1, M2, N: int, mod1: int, div2: int, op: int):
        dev = _lib.require_gpu(T1, T2)
        T1c, T2c, S1c, S2c, M1c, M2c, xform, De, n1, n2 = _dual_operands(T1, T2, S1, S2, M1, M2, "dual_table")
        out = torch.empty((N, 2 * De if op == OPS["cat"] else De), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().mi_dual_table_fwd(T1c.data_ptr(), T2c.data_ptr(), _lib.ptr(S1c), _lib.ptr(S2c), _lib.ptr(M1c),
                                                 _lib.ptr(M2c), out.data_ptr(), N, De, n1, n2, mod1, div2,
                                                 op, xform, _lib.stream_ptr(dev)), "mi_dual_table_fwd")
        ctx.save_for_backward(T1c, T2c, S1c, S2c, M1c, M2c)
        ctx.meta = (N, De, mod1, div2, op, xform)
        return out

    @staticmethod
    def backward(ctx, g):
        T1c, T2c, S1c, S2c, M1c, M2c = ctx.saved_tensors
        N, De, mod1, div2, op, xform = ctx.meta
        dev = g.device
        g = _f32c(g)
        lib = _lib.load()
        # every element of the four gradients is written by the kernel: no zero fill
        gT1, gT2 = torch.empty_like(T1c), torch.empty_like(T2c)
        gS1 = torch.empty_like(S1c) if xform == XF_SOFT else None
        gS2 = torch.empty_like(S2c) if xform == XF_SOFT else None
        ne = int(lib.mi_dual_table_bwd_workspace_elems(N, De, T1c.shape[0], T2c.shape[0], mod1, div2))
        ws = torch.empty(ne, dtype=torch.float32, device=dev) if ne else None      # chunk sums of the long rows: no state
        _lib.check(lib.mi_dual_table_bwd(g.data_ptr(), T1c.data_ptr(), T2c.data_ptr(), _lib.ptr(S1c), _lib.ptr(S2c),
                                         _lib.ptr(M1c), _lib.ptr(M2c), gT1.data_ptr(), gT2.data_ptr(), _lib.ptr(gS1),
                                         _lib.ptr(gS2), N, De, T1c.shape[0], T2c.shape[0], mod1, div2, op, xform, _lib.ptr(ws),
                                         _lib.stream_ptr(dev)), "mi_dual_table_bwd")
        return gT1, gT2, gS1, gS2, None, None, None, None, None, None


def dual_table_supported(N: int, mod1: int, div2: int, *tables) -> bool:
    """Whether mi_dual_table_* takes this shape (csrc/dual_table.hip, fill(): float4 rows of 16-byte aligned fp32 tables
    on the GPU, 32-bit element counters); otherwise the caller keeps `dual_gather` over an explicit arange(N).
    tables: T1, T2 and, where the transform has them, the logits or masks — judged as the launch would read them."""
    pair, none = tuple(tables[2:]) or (None, None), (None, None)
    S, M = (pair, none) if pair[0] is not None and pair[0].is_floating_point() else (none, pair)
    try:
        *tables, _xform, De, n1, n2 = _dual_operands(tables[0], tables[1], *S, *M, "dual_table")
    except (TypeError, ValueError):        # (a dtype or a shape the family refuses)
        return False
    if not (tables[0].is_cuda and De % 4 == 0 and 4 <= De <= 1024 and N >= 0 and mod1 > 0 and div2 > 0):
        return False

    def chunks(contributors):          # kLongRow / kChunk of the kernel
        return -(-contributors // 8) if contributors > 16 else 1

    items = n1 * chunks(-(-N // mod1)) + n2 * chunks(min(div2, N))
    if max(2 * N * De, items * De, n1, n2, mod1, div2) >= 2 ** 31:
        return False
    if n1 < min(N, mod1) or n2 < -(-N // div2):
        return False                   # (tables that cannot cover N rows: the lookup flags those ids)
    return all(t is None or t.data_ptr() % 16 == 0 for t in tables)


def dual_table(T1, T2, N, mod1, div2, op="add", S1=None, S2=None, M1=None, M2=None):
    """The two-table family's whole table [N, De] ([N, 2 De] for cat): `dual_gather(arange(N), ...)` bit for bit, without
    the index tensor, and with a backward that has no atomics and no zero fill (gradients differ from dual_gather's in
    the order of the float additions only).  Check `dual_table_supported` first."""
    return DualTable.apply(T1, T2, S1, S2, M1, M2, int(N), int(mod1), int(div2), OPS[op])


# --------------------------------------------------------------------------------------
# DeepFM on the two-table family: lookup + FM + first-order in one launch (csrc/gather_fm_dual.hip)
DUAL_FM_MAX_D = 1024      # MI_GATHER_FM_DUAL_MAX_D


def _sum_sorted(keys_sorted, perm, vals, nrows: int, D: int) -> torch.Tensor:
    """[nrows, D] sums of vals[perm[i]] per keys_sorted[i], added in a fixed order (mi_coalesce_rows_sorted)."""
    n = keys_sorted.numel()
    out = torch.zeros((nrows, D), dtype=torch.float32, device=vals.device)
    acc = torch.empty((n, D), dtype=torch.float32, device=vals.device)
    _lib.check(_lib.load().mi_coalesce_rows_sorted(keys_sorted.data_ptr(), perm.data_ptr(), vals.data_ptr(), out.data_ptr(),
                                                   acc.data_ptr(), n, D, nrows, _lib.stream_ptr(vals.device)),
               "mi_coalesce_rows_sorted")
    return out


class GatherFMDual(torch.autograd.Function):
    """emb, y_fm of DeepFM over a two-table compositional embedding in one launch (mi_gather_fm_dual_fwd):
    emb[b, f] = T1'[row % mod1] (op) T2'[row // div2], row = idx[b, f] + offsets[f]; y_fm over that emb plus the
    first-order bag over `row`.  (op, transform) as the models produce them: (mult, none) and (add, none) for QR,
    (add, soft: S1 / S2) for CERP, (add, mask: M1 / M2) for CERP retrain.

    Backward.  Deterministic mode, and every COO gradient other than QR's: mi_gather_fm_dual_bwd_rows writes a value row
    per lookup and table plus the table-row keys; dense gradients are those rows summed per key in a fixed order
    (table 2's keys are monotone in `row`, so the per-field sort of the rows orders them; table 1 takes a stable sort
    of its keys) and the transform's derivative is applied once per table element (mi_gather_fm_dual_finish) — no float
    atomics.  Default mode otherwise: dE from mi_gather_fm_bwd_rows goes to the atomic kernels of the separate lookup
    (mi_dual_gather_bwd_fields / _bwd_rows): the launches it ran before, minus one add.  The two forms have not been
    timed against each other ("Not measured")."""

    @staticmethod
    def forward(ctx, idx, offsets, T1, T2, w1, bias, S1, S2, M1, M2, mod1: int, div2: int, op: int, sparse1: bool,
                sparse2: bool, sparse_w1: bool, fields):
        dev = _lib.require_gpu(idx, offsets, T1, T2, w1, bias, S1, S2, M1, M2)
        lib = _lib.load()
        if op == OPS["cat"]:
            raise NotImplementedError('gather_fm_dual: "cat" changes the field count; it keeps dual_gather + fm_first_order')
        for name, m in (("M1", M1), ("M2", M2)):
            if m is not None and m.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"gather_fm_dual: {name} must be bool or uint8, got {m.dtype}")
        T1c, T2c, S1c, S2c, M1c, M2c, xform, De, n1, n2 = _dual_operands(T1, T2, S1, S2, M1, M2, "gather_fm_dual")
        if op == OPS["mult"] and xform != XF_NONE:
            raise NotImplementedError("gather_fm_dual: mult goes with untransformed tables only")
        if xform == XF_SOFT and (sparse1 or sparse2):
            raise ValueError("gather_fm_dual: a soft-thresholded table has no row-form gradient")
        if De > DUAL_FM_MAX_D:
            raise NotImplementedError(f"gather_fm_dual covers De <= {DUAL_FM_MAX_D}, got {De}")
        idx, offsets, w1c, ldw1, N = _lookup_operands(idx, offsets, w1)
        B, F = idx.shape
        emb = torch.empty((B, F, De), dtype=torch.float32, device=dev)
        yfm = torch.empty((B,), dtype=torch.float32, device=dev)
        rows = torch.empty((B, F), dtype=torch.int64, device=dev)
        # the default-mode backward hands the row ids to kernels that check table bounds only: they get the ids with -1
        # where this launch flagged the lookup (a row past N may still map inside both tables)
        qr_rows = sparse2 and not sparse1 and xform == XF_NONE
        atomic_bwd = not DETERMINISTIC and (qr_rows or not (sparse1 or sparse2))
        rows_bwd = torch.empty_like(rows) if atomic_bwd and any(ctx.needs_input_grad[i] for i in (2, 3, 6, 7)) else None
        _lib.check(
            lib.mi_gather_fm_dual_fwd(
                idx.data_ptr(), offsets.data_ptr(), T1c.data_ptr(), T2c.data_ptr(), _lib.ptr(S1c), _lib.ptr(S2c),
                _lib.ptr(M1c), _lib.ptr(M2c), w1c.data_ptr(), ldw1, _lib.ptr(bias), emb.data_ptr(), yfm.data_ptr(),
                rows.data_ptr(), _lib.ptr(rows_bwd), B, F, De, N, n1, n2, int(mod1), int(div2), op, xform,
                _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev),
            ),
            "mi_gather_fm_dual_fwd",
        )
        if sparse1 or sparse2 or sparse_w1 or DETERMINISTIC:
            note_field_layout(rows, offsets, N)
        # (tables and thresholds are autograd inputs: saved, so that an in-place update before the backward raises)
        ctx.save_for_backward(emb, rows, T1c, T2c, *((S1c, S2c) if xform == XF_SOFT else ()))
        ctx.masks = (M1c, M2c)      # (constants of the step, not autograd inputs)
        ctx.rows_bwd, ctx.offsets = rows_bwd, offsets
        ctx.meta = (B, F, De, N, int(mod1), int(div2), op, xform, tuple(T1.shape), tuple(T2.shape), tuple(w1.shape))
        ctx.sparse = (bool(sparse1), bool(sparse2), bool(sparse_w1))
        ctx.fields = fields if (fields is not None and fields[3] == F) else None
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(rows)
        return emb, yfm, rows

    @staticmethod
    def backward(ctx, g_emb, g_y, _g_rows):
        emb, rows, T1c, T2c = ctx.saved_tensors[:4]
        B, F, De, N, mod1, div2, op, xform, T1shape, T2shape, w1shape = ctx.meta
        S1c, S2c = ctx.saved_tensors[4:6] if xform == XF_SOFT else (None, None)
        M1c, M2c = ctx.masks
        sparse1, sparse2, sparse_w1 = ctx.sparse
        dev = emb.device
        lib = _lib.load()
        stream = _lib.stream_ptr(dev)
        need_T1, need_T2, need_w1 = ctx.needs_input_grad[2], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        need_b = ctx.has_bias and ctx.needs_input_grad[5]
        need_S = xform == XF_SOFT and (ctx.needs_input_grad[6] or ctx.needs_input_grad[7])
        n1, n2 = T1c.shape[0], T2c.shape[0]
        n = B * F

        def done(gT1=None, gT2=None, gw1=None, gb=None, gS1=None, gS2=None):
            return (None, None, gT1, gT2, gw1, gb, gS1, gS2) + (None,) * 9

        if g_emb is None and g_y is None:
            return done()
        if n == 0:      # no lookup: zero gradients in every shape
            def zero(shape, sparse, need):
                if not need:
                    return None
                if sparse:
                    return _coo(torch.empty((0,), dtype=torch.int64, device=dev),
                                torch.empty((0,) + tuple(shape[1:]), dtype=torch.float32, device=dev), shape)
                return torch.zeros(shape, dtype=torch.float32, device=dev)
            return done(zero(T1shape, sparse1, need_T1), zero(T2shape, sparse2, need_T2), zero(w1shape, sparse_w1, need_w1),
                        torch.zeros((1,), dtype=torch.float32, device=dev) if need_b else None,
                        torch.zeros_like(S1c) if need_S else None, torch.zeros_like(S2c) if need_S else None)
        g_emb, g_y = _upstream(g_emb, g_y, B, dev)
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if need_b else None
        if not (need_T1 or need_T2 or need_w1 or need_S):
            return done(gb=_bias_grad(gb, g_y, B, launched=False))
        g1vals = torch.empty((n,), dtype=torch.float32, device=dev)
        gT1 = gT2 = gS1 = gS2 = None
        qr_rows = sparse2 and not sparse1 and xform == XF_NONE      # QR(sparse=True): emb2 as COO, emb1 dense
        own = DETERMINISTIC or ((sparse1 or sparse2) and not qr_rows)
        order = None      # (sorted rows, permutation) of the per-field sort, shared by table 2 and the first-order table
        if not own:
            # ---- default mode: dE, then the separate lookup's backward kernels (float atomics)
            dE = torch.empty((n, De), dtype=torch.float32, device=dev)
            ids = ctx.rows_bwd      # (None when the mode changed between the forward and here)
            if ids is None:
                ids = torch.where((rows >= 0) & (rows < N), rows, torch.full_like(rows, -1))
            _lib.check(lib.mi_gather_fm_bwd_rows(emb.data_ptr(), g_y.data_ptr(), _lib.ptr(g_emb), dE.data_ptr(),
                                                 g1vals.data_ptr(), _lib.ptr(gb), B, F, De, stream), "mi_gather_fm_bwd_rows")
            if need_T1 or need_T2 or need_S:
                ops = (T1c, T2c, S1c, S2c, M1c, M2c, xform, De, n1, n2)
                gT1, gT2, gS1, gS2 = _dual_scatter_backward(ids, dE, ops, n, F, op, mod1, div2, ctx.fields, qr_rows, T2shape)
                if not qr_rows:
                    gT1, gT2 = gT1.view(T1shape), gT2.view(T2shape)
        else:
            # ---- row values and keys, then fixed-order sums per table row: no float atomics
            mask_vals = xform == XF_MASK and (sparse1 or sparse2)
            c1 = torch.empty((n, De), dtype=torch.float32, device=dev)
            c2 = torch.empty((n, De), dtype=torch.float32, device=dev) if (op == OPS["mult"] or mask_vals) else None
            keys1 = torch.empty((n,), dtype=torch.int64, device=dev)
            keys2 = torch.empty((n,), dtype=torch.int64, device=dev)
            # sums taken in the order of the per-field sort (table 2, the first-order table): that sort moves an id outside
            # its own field behind the field and the sums drop it, so the row kernel is told the fields, zeroes such a
            # lookup for every table and gives every flagged lookup a table-2 key that keeps the sorted keys monotone
            field_off = None
            if DETERMINISTIC and (((need_T2 or need_S) and not sparse2) or (need_w1 and not sparse_w1)):
                order = sort_field_rows(rows.view(-1), N)
                field_off = ctx.offsets if order is not None else None
            _lib.check(
                lib.mi_gather_fm_dual_bwd_rows(
                    rows.data_ptr(), _lib.ptr(field_off), emb.data_ptr(), g_y.data_ptr(), _lib.ptr(g_emb), T1c.data_ptr(), T2c.data_ptr(),
                    _lib.ptr(M1c) if mask_vals else None, _lib.ptr(M2c) if mask_vals else None, c1.data_ptr(), _lib.ptr(c2),
                    keys1.data_ptr(), keys2.data_ptr(), g1vals.data_ptr(), _lib.ptr(gb), B, F, De, N, n1, n2, mod1, div2, op,
                    stream),
                "mi_gather_fm_dual_bwd_rows",
            )
            v2 = c1 if c2 is None else c2
            A1 = A2 = None
            if need_T1 or need_S:
                if sparse1:
                    gT1 = _coo(keys1, c1, T1shape)
                elif DETERMINISTIC:
                    ks, perm = torch.sort(keys1, stable=True)
                    A1 = _sum_sorted(ks, perm, c1, n1, De)
                else:
                    A1 = _scatter_rows(keys1, c1, n1, De, stream)
            if need_T2 or need_S:
                if sparse2:
                    gT2 = _coo(keys2, v2, T2shape)
                elif DETERMINISTIC:
                    if order is not None:
                        # r2 is monotone in the row id: the per-field order of the rows is a stable order by r2, and the
                        # keys the row kernel wrote are monotone through its permutation (field_off above): one gather
                        perm = order[1]
                        ks = keys2.index_select(0, perm)
                    else:
                        ks, perm = torch.sort(keys2, stable=True)
                    A2 = _sum_sorted(ks, perm, v2, n2, De)
                else:
                    A2 = _scatter_rows(keys2, v2, n2, De, stream)
            if xform != XF_NONE and (A1 is not None or A2 is not None):
                gS1 = torch.empty_like(S1c) if (xform == XF_SOFT and A1 is not None) else None
                gS2 = torch.empty_like(S2c) if (xform == XF_SOFT and A2 is not None) else None
                _lib.check(lib.mi_gather_fm_dual_finish(_lib.ptr(A1), _lib.ptr(A2), T1c.data_ptr(), T2c.data_ptr(), _lib.ptr(S1c),
                                                        _lib.ptr(S2c), _lib.ptr(M1c), _lib.ptr(M2c), _lib.ptr(gS1), _lib.ptr(gS2),
                                                        n1, n2, De, xform, stream), "mi_gather_fm_dual_finish")
            if A1 is not None:
                gT1 = A1.view(T1shape)
            if A2 is not None:
                gT2 = A2.view(T2shape)
        gw1 = None
        if need_w1:
            if sparse_w1:
                gw1 = _coo(rows, g1vals.view((-1,) + (1,) * (len(w1shape) - 1)), w1shape)
            elif DETERMINISTIC and order is not None:
                gw1 = _sum_sorted(order[0], order[1], g1vals, N, 1).view(w1shape)
            else:
                gw1 = _scatter_rows(rows, g1vals, N, 1, stream).view(w1shape)
        return done(gT1 if need_T1 else None, gT2 if need_T2 else None, gw1, gb, gS1 if need_S else None,
                    gS2 if need_S else None)


def gather_fm_dual(idx, offsets, T1, T2, w1, bias, mod1, div2, op="add", S1=None, S2=None, M1=None, M2=None, sparse1=False,
                   sparse2=False, sparse_w1=False, fields=None):
    """(emb, y_fm) of DeepFM over a QR / CERP / CERP-retrain table in one launch; see GatherFMDual.  fields (optional):
    small_field_hint(...), for the default mode's dense backward."""
    emb, yfm, _rows = GatherFMDual.apply(idx, offsets, T1, T2, w1, bias, S1, S2, M1, M2, int(mod1), int(div2), OPS[op],
                                         bool(sparse1), bool(sparse2), bool(sparse_w1), fields)
    return emb, yfm


class CerpPruneLoss(torch.autograd.Function):
    """-sum tanh(K (soft(P, Sp) + soft(Q, Sq)))^2 over CERP's four [bucket, D] tables (mi_cerp_prune_loss_fwd / _bwd):
    one launch each way, no [bucket, D] temporary, the same bits on every run."""

    @staticmethod
    def forward(ctx, P, Sp, Q, Sq, K: float):
        dev = _lib.require_gpu(P, Sp, Q, Sq)
        lib = _lib.load()
        P, Sp, Q, Sq = _f32c(P), _f32c(Sp), _f32c(Q), _f32c(Sq)
        if not (P.shape == Sp.shape == Q.shape == Sq.shape) or P.numel() == 0:
            raise ValueError("cerp_prune_loss: the four tables must share one non-empty shape")
        n = P.numel()
        ws, armed = _losses._ticket_workspace("cerp_prune_loss", dev, lib.mi_cerp_prune_loss_workspace_elems(n))
        out = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(lib.mi_cerp_prune_loss_fwd(P.data_ptr(), Sp.data_ptr(), Q.data_ptr(), Sq.data_ptr(), n, float(K),
                                              ws.data_ptr(), int(armed), out.data_ptr(), _lib.stream_ptr(dev)),
                   "mi_cerp_prune_loss_fwd")
        ctx.save_for_backward(P, Sp, Q, Sq)
        ctx.K = float(K)
        return out

    @staticmethod
    def backward(ctx, g):
        P, Sp, Q, Sq = ctx.saved_tensors
        g = _f32c(g).view(1)
        grads = [torch.empty_like(t) for t in (P, Sp, Q, Sq)]      # every element written by the kernel: no zero fill
        _lib.check(_lib.load().mi_cerp_prune_loss_bwd(P.data_ptr(), Sp.data_ptr(), Q.data_ptr(), Sq.data_ptr(), P.numel(),
                                                      ctx.K, g.data_ptr(), *(t.data_ptr() for t in grads),
                                                      _lib.stream_ptr(P.device)), "mi_cerp_prune_loss_bwd")
        return (*grads, None)


def cerp_prune_loss(P, Sp, Q, Sq, K: float = 100) -> torch.Tensor:
    return CerpPruneLoss.apply(P, Sp, Q, Sq, float(K))


def csr_rows(values, crow, col, ids, D: int, N: int) -> torch.Tensor:
    """Dense rows of a CSR-stored table (inference only, like the reference's PrunedEmbedding)."""
    dev = _lib.require_gpu(crow, ids)
    idsc = _i64c(ids)
    out = torch.empty(tuple(ids.shape) + (D,), dtype=torch.float32, device=dev)
    _lib.check(
        _lib.load().mi_csr_rows_fwd(_lib.ptr(values), crow.data_ptr(), _lib.ptr(col), idsc.data_ptr(),
                                    out.data_ptr(), idsc.numel(), D, N, _lib.err_word(dev).data_ptr(),
                                    _lib.stream_ptr(dev)),
        "mi_csr_rows_fwd",
    )
    return out


def dhe_hash(ids, slopes, bias, primes, prefix: int, m: int) -> torch.Tensor:
    """[n] int64 ids -> [n, k] fp32 hash features in [-1, 1] (not differentiable)."""
    dev = _lib.require_gpu(ids, slopes, bias, primes)
    idsc = _i64c(ids)
    K = slopes.numel()
    out = torch.empty(tuple(ids.shape) + (K,), dtype=torch.float32, device=dev)
    _lib.check(
        _lib.load().mi_dhe_hash(idsc.data_ptr(), slopes.contiguous().data_ptr(), bias.contiguous().data_ptr(),
                                primes.contiguous().data_ptr(), out.data_ptr(), idsc.numel(), K, int(prefix),
                                int(m), _lib.stream_ptr(dev)),
        "mi_dhe_hash",
    )
    return out


# --------------------------------------------------------------------------------------
# LightGCN propagation: CSR SpMM with fused layer sum
HUB_DEGREE = 256  # rows with more nonzeros than this get a whole workgroup


def _os_env(name, default):
    import os
    return os.environ.get(name, default)


class CsrPlan:
    """int32 CSR of A and of A^T plus the short/hub row split, built once per sparsity pattern.

    The reference passes a torch sparse-CSR tensor with int64 indices every call
    (src/trainer/lightgcn.py:36-40); the plan is cached on its index tensors.  Values are read
    fresh on every call (SparseDropout changes them, src/models/layers.py:15-37).
    """

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, shape):
        n_rows, n_cols = shape
        nnz = col.numel()
        if nnz >= 2 ** 31 or max(n_rows, n_cols) >= 2 ** 31:
            raise ValueError("matrix too large for int32 CSR indices")
        self.shape = (n_rows, n_cols)
        self.nnz = nnz
        dev = crow.device
        # the plan is cached under the ADDRESSES of the caller's index tensors (csr_plan): keep them alive so that no
        # other graph's indices can be allocated there while the entry exists
        self.src_crow, self.src_col = crow, col
        self.src_versions = (crow._version, col._version)
        self.crow = crow.to(torch.int32).contiguous()
        self.col = col.to(torch.int32).contiguous()
        deg = (crow[1:] - crow[:-1])
        self.short_rows, self.long_rows = self._split(deg)
        self.is_hub = (deg > HUB_DEGREE).to(torch.uint8)          # per row of A: handled by a whole workgroup
        self.hub_need = torch.zeros(n_rows, dtype=torch.uint8, device=dev)     # mi_spmm_csr_sel's flags: zero between launches
        self.filler_row = int(self.short_rows[0]) if self.short_rows.numel() else -1
        # transpose: sort entries by (col, row); perm maps transposed entry -> original entry
        rows = torch.repeat_interleave(torch.arange(n_rows, device=dev), deg)
        key = col.to(torch.int64) * n_rows + rows
        perm = torch.argsort(key, stable=True)
        self.perm = perm
        self.col_t = rows[perm].to(torch.int32).contiguous()
        cnt = torch.bincount(col.to(torch.int64), minlength=n_cols)
        crow_t = torch.zeros(n_cols + 1, dtype=torch.int64, device=dev)
        crow_t[1:] = torch.cumsum(cnt, 0)
        self.crow_t = crow_t.to(torch.int32).contiguous()
        self.short_rows_t, self.long_rows_t = self._split(cnt)
        self.pattern_symmetric = (n_rows == n_cols and torch.equal(self.crow_t, self.crow)
                                  and torch.equal(self.col_t, self.col))
        self._sym_vals_key = None
        self._sym_vals = False

    @staticmethod
    def _split(deg):
        hub = deg > HUB_DEGREE
        return (torch.nonzero(~hub).flatten().to(torch.int32).contiguous(),
                torch.nonzero(hub).flatten().to(torch.int32).contiguous())

    @staticmethod
    def _same_values(kept, kept_version, val) -> bool:
        """True when `val` is provably the tensor the cache was filled from.  The cache keeps a strong reference to
        that tensor, so its address cannot be handed to a new allocation while it is the key (a SparseDropout draw
        freed and re-allocated at the same address must miss); a tensor at the same address with the same size and
        version counter is then the kept tensor itself or a view / detach of it."""
        return (kept is not None and val.data_ptr() == kept.data_ptr() and val.numel() == kept.numel()
                and val.dtype == kept.dtype and val._version == kept_version)

    def transposed_values(self, val: torch.Tensor) -> torch.Tensor:
        if self.pattern_symmetric:
            if not self._same_values(self._sym_vals_key, self.__dict__.get("_sym_vals_version"), val):
                self._sym_vals = bool(torch.equal(val.index_select(0, self.perm), val))
                self._sym_vals_key, self._sym_vals_version = val, val._version
            if self._sym_vals:
                return val
        # the adjacency values are constants between SparseDropout draws: permute them once per tensor version
        if not self._same_values(self.__dict__.get("_tv_src"), self.__dict__.get("_tv_version"), val):
            self._tv = val.index_select(0, self.perm)
            self._tv_src, self._tv_version = val, val._version
        return self._tv


    # ---- tiled form (mi_spmm_tiled) ----
    TILES_PER_LAUNCH = 512          # about two workgroups per CU, each with about nnz / 512 edges
    COL_BLOCK_BYTES = 2 << 20       # rows of X per column block: half of an XCD's 4 MiB L2

    def tiles(self, D: int, transposed: bool):
        """The tile plan of A (or A^T) for rows of D floats, built once per (pattern, D): row tiles of about equal edge
        count and at most 64 KiB of LDS sums, every tile's edges grouped by column block.  None when the kernel cannot
        take the matrix (columns >= 2^23, D outside the float4 kernels)."""
        key = (int(D), bool(transposed))
        cache = self.__dict__.setdefault("_tiles", {})
        if key in cache:
            return cache[key]
        crow, col = (self.crow_t, self.col_t) if transposed else (self.crow, self.col)
        n_rows, n_cols = (self.shape[1], self.shape[0]) if transposed else self.shape
        plan = None
        if _float4_rows(D) and n_cols < (1 << 23) and self.nnz > 0 and n_rows > 0:
            dev = crow.device
            crow64 = crow.to(torch.int64)
            deg = crow64[1:] - crow64[:-1]
            budget = max(1, -(-self.nnz // self.TILES_PER_LAUNCH))
            max_rows = max(1, min(256, (64 * 1024) // (4 * D)))
            t_e = crow64[:-1] // budget                                  # tile id by edge budget (non-decreasing)
            rows = torch.arange(n_rows, device=dev)
            _, inv, cnt = torch.unique_consecutive(t_e, return_inverse=True, return_counts=True)
            grp_first = torch.cumsum(cnt, 0) - cnt                       # first row of each edge-budget group
            sub = (rows - grp_first[inv]) // max_rows                    # ... cut further by the row cap
            _, row_tile, tcnt = torch.unique_consecutive(inv * (n_rows // max_rows + 2) + sub, return_inverse=True,
                                                         return_counts=True)
            ntiles = int(tcnt.numel())
            tile_row0 = torch.zeros(ntiles + 1, dtype=torch.int64, device=dev)
            tile_row0[1:] = torch.cumsum(tcnt, 0)
            erow = torch.repeat_interleave(rows, deg)
            etile = row_tile[erow]
            lrow = erow - tile_row0[etile]
            cb_rows = max(1, self.COL_BLOCK_BYTES // (4 * D))
            col64 = col.to(torch.int64)
            nblocks = -(-n_cols // cb_rows)
            perm = torch.argsort(etile * nblocks + col64 // cb_rows, stable=True)
            ecr = (col64 | (lrow << 23))[perm].to(torch.int32).contiguous()
            tile_edge0 = torch.zeros(ntiles + 1, dtype=torch.int64, device=dev)
            tile_edge0[1:] = torch.cumsum(torch.bincount(etile, minlength=ntiles), 0)
            plan = dict(ntiles=ntiles, max_rows=int(tcnt.max()), ecr=ecr, perm=perm,
                        tile_edge0=tile_edge0.to(torch.int32).contiguous(), tile_row0=tile_row0.to(torch.int32).contiguous())
        cache[key] = plan
        return plan

    def tile_values(self, val: torch.Tensor, D: int, transposed: bool) -> torch.Tensor:
        """`val` (the values of A, or of A^T when transposed) in the tile plan's edge order; cached per values tensor
        (they only change with a SparseDropout draw)."""
        key = ("_tilev", int(D), bool(transposed))
        hit = self.__dict__.get(key)
        if hit is not None and self._same_values(hit[0], hit[1], val):
            return hit[2]
        out = val.index_select(0, self.tiles(D, transposed)["perm"])
        self.__dict__[key] = (val, val._version, out)
        return out


    # ---- task-balanced, slice-phased form (mi_spmm_sliced, round 4) ----
    SLICE_BYTES = int(_os_env("MI_SPMM_SLICE_KB", "2048")) << 10      # rows of X per column slice (default: half of an XCD's 4 MiB L2)
    TASK_NNZ = int(_os_env("MI_SPMM_TASK_NNZ", "512"))                # nonzeros per task: few enough tasks that all are resident at once
    GROUP_ROWS = 4                  # kGroupRows of csrc/spmm.hip: rows a lane group (narrow task) / a wide task owns
    WIDE_MIN = 48                   # rows with more nonzeros than this get a wide task (all lane groups stride them)

    def sliced(self, D: int, transposed: bool):
        """The task plan of A (or A^T) for rows of D floats, built once per (pattern, D) on the host (csrc/spmm.hip,
        k_spmm_sliced): NPW = 256 / D lane groups per wave.  Rows in row order; a row of <= WIDE_MIN nonzeros joins the open
        NARROW task (<= 4 NPW rows, <= TASK_NNZ nonzeros; row i of the task belongs to lane group i % NPW), a heavier one the
        open WIDE task (<= 4 rows, <= TASK_NNZ nonzeros unless alone), hubs (> HUB_DEGREE) are listed apart.  Inside an
        owner's range the edges are sorted by column slice.  None when the kernel cannot take the matrix."""
        key = (int(D), bool(transposed))
        cache = self.__dict__.setdefault("_sliced", {})
        if key in cache:
            return cache[key]
        import numpy as np

        crow_d, col_d = (self.crow_t, self.col_t) if transposed else (self.crow, self.col)
        n_rows, n_cols = (self.shape[1], self.shape[0]) if transposed else self.shape
        plan = None
        if _float4_rows(D) and n_cols < (1 << 28) and self.nnz > 0 and n_rows > 0:
            dev = crow_d.device
            NPW, GR = 256 // D, self.GROUP_ROWS
            crow = crow_d.cpu().numpy().astype(np.int64)
            col = col_d.cpu().numpy().astype(np.int64)
            deg = crow[1:] - crow[:-1]
            hub = deg > HUB_DEGREE
            slice_rows = max(1, self.SLICE_BYTES // (4 * D))
            task_of = np.full(n_rows, -1, dtype=np.int64)
            slot_of = np.zeros(n_rows, dtype=np.int64)       # lane group (narrow) / 0 (wide)
            j_of = np.zeros(n_rows, dtype=np.int64)          # first or second row of its owner
            wide_flags = []
            open_n = None         # [task id, rows so far, nonzeros so far] of the open narrow / wide task
            open_w = None
            T = 0
            degl, hubl = deg.tolist(), hub.tolist()
            for r in range(n_rows):
                if hubl[r]:
                    continue
                d = degl[r]
                if d > self.WIDE_MIN:
                    if open_w is None or open_w[1] == GR or open_w[2] + d > self.TASK_NNZ:
                        open_w = [T, 0, 0]
                        wide_flags.append(1)
                        T += 1
                    task_of[r], slot_of[r], j_of[r] = open_w[0], 0, open_w[1]
                    open_w[1] += 1
                    open_w[2] += d
                else:
                    if open_n is None or open_n[1] == GR * NPW or open_n[2] + d > self.TASK_NNZ:
                        open_n = [T, 0, 0]
                        wide_flags.append(0)
                        T += 1
                    task_of[r], slot_of[r], j_of[r] = open_n[0], open_n[1] % NPW, open_n[1] // NPW
                    open_n[1] += 1
                    open_n[2] += d
            twide = np.asarray(wide_flags, dtype=np.uint8)
            erow = np.repeat(np.arange(n_rows), deg)
            keep = np.nonzero(~hub[erow])[0]
            er = erow[keep]
            nsl = -(-n_cols // slice_rows)
            # owner = (task, lane group); inside an owner: slice, then first / second row, then the CSR's column order
            ek = ((task_of[er] * NPW + slot_of[er]) * nsl + col[keep] // slice_rows) * GR + j_of[er]
            order = np.argsort(ek, kind="stable")
            perm = keep[order]
            ecol = col[perm] | (j_of[erow[perm]] << 28)
            ecol = np.where(ecol >= 2 ** 31, ecol - 2 ** 32, ecol).astype(np.int32)       # bit pattern of the uint32 word
            owner = task_of[er] * NPW + slot_of[er]
            cnt = np.bincount(owner, minlength=max(T, 1) * NPW)
            starts = np.zeros(max(T, 1) * NPW + 1, dtype=np.int64)
            starts[1:] = np.cumsum(cnt)
            tptr = np.zeros((max(T, 1), NPW + 1), dtype=np.int64)
            tptr[:, :NPW] = starts[:-1].reshape(-1, NPW)
            tptr[:, NPW] = starts[NPW::NPW]
            # a wide task keeps all its edges under lane group 0: its range is [tptr[0], tptr[1]) = group 0's, as the kernel reads it
            trows = np.full((max(T, 1), GR * NPW), -1, dtype=np.int32)
            nh = np.nonzero(~hub)[0]
            trows[task_of[nh], j_of[nh] * NPW + slot_of[nh]] = nh
            plan = dict(T=T, NPW=NPW, slice_rows=int(slice_rows), tptr=torch.from_numpy(tptr.astype(np.int32)).to(dev),
                        trows=torch.from_numpy(trows).to(dev), twide=torch.from_numpy(twide if T else np.zeros(1, np.uint8)).to(dev),
                        ecol=torch.from_numpy(ecol).to(dev), perm=torch.from_numpy(perm.astype(np.int64)).to(dev),
                        long_rows=torch.from_numpy(np.nonzero(hub)[0].astype(np.int32)).to(dev))
        cache[key] = plan
        return plan

    def sliced_values(self, val: torch.Tensor, D: int, transposed: bool) -> torch.Tensor:
        """`val` (the values of A, or of A^T when transposed) in the task plan's edge order; cached per values tensor."""
        key = ("_slicedv", int(D), bool(transposed))
        hit = self.__dict__.get(key)
        if hit is not None and self._same_values(hit[0], hit[1], val):
            return hit[2]
        out = val.index_select(0, self.sliced(D, transposed)["perm"])
        self.__dict__[key] = (val, val._version, out)
        return out


# The tiled SpMM (csrc/spmm.hip, round 3: row tiles whose sums live in LDS, edges walked column block by column block,
# one edge per 16-lane group, LDS float adds) is parity-green and OPT-IN (MI_SPMM_TILED=1): on MI355X it runs 13x SLOWER
# than the row-per-wave kernels (1073 vs 80 us per Yelp2018-shaped layer) because ds_add_f32 executes a wave's 64 lanes
# one after the other — 170 cycles per wave-instruction whatever the address pattern, against 5-8 for ds_add_u32 and
# 10-15 for a plain read + add + write (tools/probe_lds_atomic.hip, profiles/r03_lds_atomic_probe.txt).
import os as _os

TILED_SPMM = _os.environ.get("MI_SPMM_TILED", "0") == "1"
# The slice-phased SpMM (round 4, mi_spmm_sliced) is parity-green and OPT-IN: "0" (default) = never, "1" = for operands
# larger than an XCD's L2, "2" = always (tests).  Measured on MI355X at the Yelp2018 shape (profiles/r04_spmm_counters.txt):
# L2 hit rate 0.38 -> 0.50 and 12 % fewer fabric-side bytes, but 70-82 us per layer against 75 for the row-per-wave kernel
# whatever the slice size (128 KiB ... 4 MiB) and whether the tasks run in one round or three: the waves do not stay in phase,
# and what bounds both kernels is the rate at which the cache hierarchy serves random 256-B rows (~8 TB/s), not its hit rate.
SLICED_SPMM = int(_os.environ.get("MI_SPMM_SLICED", "0"))
SLICED_MIN_BYTES = 4 << 20

_plans = {}


def csr_plan(matrix: torch.Tensor) -> CsrPlan:
    crow, col = matrix.crow_indices(), matrix.col_indices()
    key = (crow.data_ptr(), col.data_ptr(), col.numel(), tuple(matrix.shape), str(crow.device))
    plan = _plans.get(key)
    if plan is not None and (plan.src_versions != (crow._version, col._version)):
        plan = None     # the index tensors were written in place since the plan was built
    if plan is None:
        if len(_plans) > 16:
            _plans.clear()
        plan = CsrPlan(crow, col, tuple(matrix.shape))
        _plans[key] = plan
    return plan


def _spmm(plan: CsrPlan, transposed: bool, val, Xa, Xb, x_split, Y, acc_a, acc_b, acc_split, acc_out, scale, D, xmask=None,
          rows=None):
    """xmask (optional, int32 words, one bit per row of X): rows whose bit is 0 are all zeros and are not fetched.
    rows (optional, (short int32 list, hub int32 list, hub_need bytes)): only these OUTPUT rows are computed — of the hubs
    those whose hub_need byte is set (repeats allowed: the outputs must then not alias the inputs); the other rows of Y /
    acc_out are left untouched."""
    lib = _lib.load()
    n_x = plan.shape[0] if transposed else plan.shape[1]
    if rows is None and (SLICED_SPMM == 2 or (SLICED_SPMM == 1 and n_x * D * 4 > SLICED_MIN_BYTES)) and not TILED_SPMM:
        sp = plan.sliced(D, transposed)
        if sp is not None:
            crow_h, col_h = (plan.crow_t, plan.col_t) if transposed else (plan.crow, plan.col)
            ev = plan.sliced_values(val, D, transposed)
            lr = sp["long_rows"]
            _lib.check(
                lib.mi_spmm_sliced(crow_h.data_ptr(), col_h.data_ptr(), val.data_ptr(), sp["tptr"].data_ptr(), sp["trows"].data_ptr(),
                                   sp["twide"].data_ptr(), sp["ecol"].data_ptr(), ev.data_ptr(), sp["T"], Xa.data_ptr(), _lib.ptr(Xb), x_split,
                                   _lib.ptr(Y), _lib.ptr(acc_a), _lib.ptr(acc_b), acc_split, _lib.ptr(acc_out), float(scale), D,
                                   lr.data_ptr() if lr.numel() else None, lr.numel(), _lib.ptr(xmask), _lib.stream_ptr(val.device)),
                "mi_spmm_sliced")
            return
    tp = plan.tiles(D, transposed) if (TILED_SPMM and not DETERMINISTIC and rows is None) else None
    if tp is not None:
        ev = plan.tile_values(val, D, transposed)
        _lib.check(
            lib.mi_spmm_tiled(tp["tile_edge0"].data_ptr(), tp["tile_row0"].data_ptr(), tp["ntiles"], tp["max_rows"],
                              tp["ecr"].data_ptr(), ev.data_ptr(), Xa.data_ptr(), _lib.ptr(Xb), x_split, _lib.ptr(Y),
                              _lib.ptr(acc_a), _lib.ptr(acc_b), acc_split, _lib.ptr(acc_out), float(scale), D,
                              _lib.stream_ptr(val.device)),
            "mi_spmm_tiled",
        )
        return
    if transposed:
        crow, col, sr, lr, n_rows = plan.crow_t, plan.col_t, plan.short_rows_t, plan.long_rows_t, plan.shape[1]
    else:
        crow, col, sr, lr, n_rows = plan.crow, plan.col, plan.short_rows, plan.long_rows, plan.shape[0]
    need = None
    if rows is not None:
        sr, lr, need = rows
    dev = val.device
    _lib.check(
        lib.mi_spmm_csr_sel(crow.data_ptr(), col.data_ptr(), val.data_ptr(), Xa.data_ptr(), _lib.ptr(Xb), x_split,
                            _lib.ptr(Y), _lib.ptr(acc_a), _lib.ptr(acc_b), acc_split, _lib.ptr(acc_out), float(scale),
                            n_rows, D, sr.data_ptr() if sr.numel() else None, sr.numel(),
                            lr.data_ptr() if lr.numel() else None, lr.numel(), _lib.ptr(xmask), _lib.ptr(need),
                            _lib.stream_ptr(dev)),
        "mi_spmm_csr_sel",
    )


MASK_FIRST_BACKWARD_LAYER = _os.environ.get("MI_SPMM_ROW_MASK", "1") == "1"


def _row_mask(Xa, Xb, D):
    """Bit per row of [Xa; Xb]: 1 = the row has a non-zero element (mi_row_mask), or None where that kernel has no form."""
    lpr = D // 4
    if D % 4 or lpr > 64 or lpr & (lpr - 1):
        return None
    n = Xa.shape[0] + (Xb.shape[0] if Xb is not None else 0)
    mask = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=Xa.device)
    _lib.check(_lib.load().mi_row_mask(Xa.data_ptr(), _lib.ptr(Xb), Xa.shape[0] if Xb is not None else 0, n, D, mask.data_ptr(),
                                       _lib.stream_ptr(Xa.device)), "mi_row_mask")
    return mask


def _propagate(plan, transposed, val, Xa, Xb, num_layers, sparse_input=False, last_rows=None):
    """res = (sum_{k=0..L} A^k X) / (L+1) with X = [Xa; Xb] (Xb may be None).  sparse_input: X is expected to be zero on
    most rows (the gradient entering a backward propagation is non-zero only on the batch's rows): a row mask of X is
    built on the device (one pass over X) and the first layer does not fetch the zero rows — same result.
    last_rows ((users, pos, neg, item_base): int64 ids, row = user id / item_base + item id; forward only): the caller reads
    the result at these rows only, so the LAST layer computes only them; every other row of the result is undefined."""
    dev = Xa.device
    D = Xa.shape[1]
    n = Xa.shape[0] + (Xb.shape[0] if Xb is not None else 0)
    x_split = Xa.shape[0] if Xb is not None else 0
    if num_layers == 0:
        return torch.cat([Xa, Xb]) if Xb is not None else Xa.clone()
    acc = torch.empty((n, D), dtype=torch.float32, device=dev)
    bufs = [torch.empty((n, D), dtype=torch.float32, device=dev) for _ in range(min(2, num_layers - 1))]
    cur_a, cur_b, cur_split = Xa, Xb, x_split
    for k in range(1, num_layers + 1):
        last = k == num_layers
        Y = None if last else bufs[(k - 1) % len(bufs)]
        scale = 1.0 / (num_layers + 1) if last else 1.0
        rows, out = None, acc
        if last and last_rows is not None and not transposed and plan.filler_row >= 0 and _float4_rows(D):
            # one launch turns the batch into the one-wave-per-row list (hubs -> a filler row + their hub_need flag)
            users, pos, neg, item_base = last_rows
            short = torch.empty((3 * users.numel(),), dtype=torch.int32, device=dev)
            _lib.check(_lib.load().mi_batch_row_list(users.data_ptr(), pos.data_ptr(), neg.data_ptr(), users.numel(),
                                                     item_base, n, plan.is_hub.data_ptr(),
                                                     plan.filler_row, short.data_ptr(), plan.hub_need.data_ptr(),
                                                     _lib.stream_ptr(dev)), "mi_batch_row_list")
            rows = (short, plan.long_rows, plan.hub_need)
            out = torch.empty_like(acc)          # repeats in the list: the result must not be updated in place
        if k == 1:
            xmask = _row_mask(Xa, Xb, D) if (sparse_input and MASK_FIRST_BACKWARD_LAYER) else None
            _spmm(plan, transposed, val, cur_a, cur_b, cur_split, Y, Xa, Xb, x_split, out, scale, D, xmask=xmask, rows=rows)
        else:
            _spmm(plan, transposed, val, cur_a, None, 0, Y, acc, None, 0, out, scale, D, rows=rows)
        acc = out
        cur_a, cur_b, cur_split = Y, None, 0
    return acc


class LightGCNPropagate(torch.autograd.Function):
    """(sum_{k=0..L} A^k [Xa;Xb]) / (L+1) — src/models/lightgcn.py:79-87.  Backward is the same
    propagation with A^T applied to the incoming gradient."""

    @staticmethod
    def forward(ctx, val, Xa, Xb, plan, num_layers: int):
        _lib.require_gpu(val, Xa, Xb)
        if val.requires_grad:
            raise NotImplementedError("gradients w.r.t. the adjacency values are not provided")
        if plan.shape[0] != plan.shape[1]:
            raise ValueError("propagation needs a square adjacency")
        valc, Xac = _f32c(val), _f32c(Xa)
        Xbc = None if Xb is None else _f32c(Xb)
        n = Xac.shape[0] + (Xbc.shape[0] if Xbc is not None else 0)
        if n != plan.shape[0]:
            raise ValueError(f"adjacency is {plan.shape} but the embedding tables have {n} rows")
        ctx.plan, ctx.num_layers = plan, num_layers
        ctx.split = Xac.shape[0] if Xbc is not None else None
        ctx.save_for_backward(valc)
        res = _propagate(plan, False, valc, Xac, Xbc, num_layers)
        if ctx.split is None:
            return res
        # two tables in, two tables out (LightGCN splits the result anyway, src/models/lightgcn.py:87): the backward
        # then receives the two gradients separately and reads them as two row segments — no cat, no split
        return res[: ctx.split], res[ctx.split:]

    @staticmethod
    def backward(ctx, *gs):
        (valc,) = ctx.saved_tensors
        plan = ctx.plan
        val_t = plan.transposed_values(valc)
        if ctx.split is None:
            g = _f32c(gs[0])
            gX = _propagate(plan, True, val_t, g, None, ctx.num_layers, sparse_input=True)
            return None, gX, None, None, None
        ga, gb = gs
        n_a, n_b = ctx.split, plan.shape[0] - ctx.split
        D = (ga if ga is not None else gb).shape[1]
        dev = valc.device
        ga = _f32c(ga) if ga is not None else torch.zeros((n_a, D), dtype=torch.float32, device=dev)
        gb = _f32c(gb) if gb is not None else torch.zeros((n_b, D), dtype=torch.float32, device=dev)
        gX = _propagate(plan, True, val_t, ga, gb, ctx.num_layers, sparse_input=True)
        return None, gX[: ctx.split], gX[ctx.split:], None, None


def rowsq_fwd(U, ui, P, pi, Nn, ni) -> torch.Tensor:
    """mi_rowsq_fwd[_armed] on checked operands (fp32 contiguous [*, D] tables, int64 [B] indices): the [1] result."""
    lib, dev, B = _lib.load(), U.device, ui.numel()
    ws, armed = _losses._ticket_workspace("rowsq", dev, lib.mi_bpr_workspace_elems(B))
    out = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.check((lib.mi_rowsq_fwd_armed if armed else lib.mi_rowsq_fwd)(
        U.data_ptr(), ui.data_ptr(), P.data_ptr(), pi.data_ptr(), Nn.data_ptr(), ni.data_ptr(), B, U.shape[1], U.shape[0],
        P.shape[0], Nn.shape[0], _lib.err_word(dev).data_ptr(), ws.data_ptr(), out.data_ptr(), _lib.stream_ptr(dev)),
        "mi_rowsq_fwd")
    return out


def rowsq_bwd(U, ui, P, pi, Nn, ni, g, dU, dP, dN) -> None:
    """mi_rowsq_bwd: g[0] * row / B added (float atomics) into the given gradients, each of them optional."""
    _lib.check(_lib.load().mi_rowsq_bwd(
        U.data_ptr(), ui.data_ptr(), P.data_ptr(), pi.data_ptr(), Nn.data_ptr(), ni.data_ptr(), ui.numel(), U.shape[1],
        U.shape[0], P.shape[0], Nn.shape[0], g.data_ptr(), _lib.ptr(dU), _lib.ptr(dP), _lib.ptr(dN),
        _lib.stream_ptr(g.device)), "mi_rowsq_bwd")


class LightGCNPropagateReg(torch.autograd.Function):
    """LightGCNPropagate of plain tables AND get_reg_loss over a batch's rows of those tables
    (src/models/lightgcn.py:79-100,166-173) as one node: (res_a, res_b, reg) for two tables, (res, reg) for one table
    (Xb None: SingleLightGCN, items follow the `item_base` users).  The point is the backward: the regulariser's
    gradient touches 3 B rows, and as a node of its own it reaches the tables as zero-filled [N, D] tensors that
    autograd then adds to the propagation's gradients (two fills + two adds of 8 - 10 MB each per step at Yelp2018 size);
    here mi_rowsq_bwd adds those rows straight into the propagation's gradient."""

    @staticmethod
    def forward(ctx, val, Xa, Xb, plan, num_layers: int, users, pos, neg, batch_rows_only: bool = False, item_base: int = 0):
        _lib.require_gpu(val, Xa, Xb, users)
        if val.requires_grad:
            raise NotImplementedError("gradients w.r.t. the adjacency values are not provided")
        valc, Xac = _f32c(val), _f32c(Xa)
        Xbc = None if Xb is None else _f32c(Xb)
        n = Xac.shape[0] + (Xbc.shape[0] if Xbc is not None else 0)
        if n != plan.shape[0] or plan.shape[0] != plan.shape[1]:
            raise ValueError(f"adjacency is {plan.shape} but the embedding tables have {n} rows")
        ui, pi, ni = (_i64c(t).view(-1) for t in (users, pos, neg))
        B = ui.numel()
        if pi.numel() != B or ni.numel() != B or B == 0:
            raise ValueError("reg loss: users / positives / negatives must be [B] indices")
        if Xbc is None:              # one table: the item rows start at item_base
            item_tab, pr, nr = Xac, pi + item_base, ni + item_base
        else:
            item_tab, pr, nr, item_base = Xbc, pi, ni, Xac.shape[0]
        last_rows = (ui, pi, ni, item_base) if batch_rows_only else None
        res = _propagate(plan, False, valc, Xac, Xbc, num_layers, last_rows=last_rows)
        reg = rowsq_fwd(Xac, ui, item_tab, pr, item_tab, nr)
        ctx.plan, ctx.num_layers = plan, num_layers
        ctx.split = None if Xbc is None else Xac.shape[0]
        ctx.save_for_backward(valc, Xac, item_tab, ui, pr, nr)
        if ctx.split is None:
            return res, reg.view(())
        return res[: ctx.split], res[ctx.split:], reg.view(())

    @staticmethod
    def backward(ctx, *gs):
        valc, Xac, item_tab, ui, pr, nr = ctx.saved_tensors
        plan, split = ctx.plan, ctx.split
        dev, D = valc.device, Xac.shape[1]
        greg = gs[-1]
        val_t = plan.transposed_values(valc)
        if split is None:
            g = gs[0]
            gX = (_propagate(plan, True, val_t, _f32c(g), None, ctx.num_layers, sparse_input=True) if g is not None
                  else torch.zeros((plan.shape[0], D), dtype=torch.float32, device=dev))
            gXa = gXb = gX
        else:
            ga, gb = gs[0], gs[1]
            if ga is None and gb is None:
                gX = torch.zeros((plan.shape[0], D), dtype=torch.float32, device=dev)
            else:
                ga = _f32c(ga) if ga is not None else torch.zeros((split, D), dtype=torch.float32, device=dev)
                gb = _f32c(gb) if gb is not None else torch.zeros((plan.shape[0] - split, D), dtype=torch.float32, device=dev)
                gX = _propagate(plan, True, val_t, ga, gb, ctx.num_layers, sparse_input=True)
            gXa, gXb = gX[:split], gX[split:]
        if greg is not None:
            rowsq_bwd(Xac, ui, item_tab, pr, item_tab, nr, _f32c(greg).view(1), gXa, gXb, gXb)
        if split is None:
            return None, gX, None, None, None, None, None, None, None, None
        return None, gXa, gXb, None, None, None, None, None, None, None


def lightgcn_propagate_reg(matrix: torch.Tensor, Xa: torch.Tensor, Xb: Optional[torch.Tensor], num_layers: int, users, pos, neg,
                           batch_rows_only: bool = False, item_base: int = 0):
    """(all_user_emb, all_item_emb, reg_loss), or (all_emb, reg_loss) for ONE table (Xb None; item row = item_base + item id)
    — see LightGCNPropagateReg.  batch_rows_only: the result is valid ONLY at rows `users` / `pos`, `neg` (what BPR and
    InfoNCE over the batch read): the last propagation layer computes just those rows instead of all of them."""
    if matrix.layout != torch.sparse_csr:
        if matrix.layout == torch.sparse_coo:
            matrix = matrix.coalesce().to_sparse_csr()
        else:
            raise ValueError(f"Not supported matrix layout: {matrix.layout}")
    return LightGCNPropagateReg.apply(matrix.values(), Xa, Xb, csr_plan(matrix), num_layers, users, pos, neg, batch_rows_only,
                                      int(item_base))


def lightgcn_propagate(matrix: torch.Tensor, Xa: torch.Tensor, Xb: Optional[torch.Tensor], num_layers: int):
    if matrix.layout != torch.sparse_csr:
        if matrix.layout == torch.sparse_coo:
            matrix = matrix.coalesce().to_sparse_csr()
        else:
            raise ValueError(f"Not supported matrix layout: {matrix.layout}")
    plan = csr_plan(matrix)
    return LightGCNPropagate.apply(matrix.values(), Xa, Xb, plan, num_layers)


def spmm(matrix: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """matrix @ X for a sparse-CSR matrix (rectangular allowed; src/models/hccf.py:56-57 shape)."""
    return SpMM.apply(matrix.values(), X, csr_plan(matrix))


class SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, X, plan):
        _lib.require_gpu(val, X)
        valc, Xc = _f32c(val), _f32c(X)
        if Xc.shape[0] != plan.shape[1]:
            raise ValueError("shape mismatch in sparse @ dense")
        Y = torch.empty((plan.shape[0], Xc.shape[1]), dtype=torch.float32, device=Xc.device)
        _spmm(plan, False, valc, Xc, None, 0, Y, None, None, 0, None, 1.0, Xc.shape[1])
        ctx.plan = plan
        ctx.save_for_backward(valc)
        return Y

    @staticmethod
    def backward(ctx, g):
        (valc,) = ctx.saved_tensors
        plan = ctx.plan
        g = _f32c(g)
        gX = torch.empty((plan.shape[1], g.shape[1]), dtype=torch.float32, device=g.device)
        _spmm(plan, True, plan.transposed_values(valc), g, None, 0, gX, None, None, 0, None, 1.0, g.shape[1])
        return None, gX, None


# --------------------------------------------------------------------------------------
# HCCF propagation (src/models/hccf.py:36-68): the LightGCN-shaped product with a leaky-residual epilogue
class HccfPlan:
    """The square block CSR of A = [[0, M], [M^T, 0]] for a U x I pattern of M, built once per pattern: a CsrPlan of A
    and `vidx`, which takes M's nnz stored values (CSR order) to A's 2 nnz (`[arange(nnz), perm]` of the rectangular
    plan: A's upper rows are M's rows, its lower rows M^T's)."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, shape, keep):
        U, I = shape
        rect = CsrPlan(crow, col, (U, I))
        nnz = rect.nnz
        self.shape, self.nnz = (U, I), nnz
        self.keep = keep                      # the caller's index tensors: the cache key is their addresses (see CsrPlan)
        self.keep_versions = tuple(t._version for t in keep)
        self.vidx = torch.cat([torch.arange(nnz, device=crow.device), rect.perm])
        crow64, col64 = crow.to(torch.int64), col.to(torch.int64)
        self.square = CsrPlan(torch.cat([crow64, rect.crow_t[1:].to(torch.int64) + nnz]),
                              torch.cat([col64 + U, rect.col_t.to(torch.int64)]), (U + I, U + I))

    def values(self, vals: torch.Tensor) -> torch.Tensor:
        return _f32c(vals).index_select(0, self.vidx)


_hccf_plans = {}
hccf_plan_stats = {"built": 0, "hit": 0}


def _hccf_pattern(matrix: torch.Tensor):
    """(key tensors, stored values) of a U x I sparse matrix.  A COO matrix is read as it is stored when its indices are
    already in canonical (sorted, distinct) order — what `coalesce()` and SparseDropout leave, whatever the matrix's
    coalesced flag says: that is checked once per index tensor, by hccf_plan — and coalesced otherwise."""
    if matrix.layout == torch.sparse_csr:
        return (matrix.crow_indices(), matrix.col_indices()), matrix.values()
    if matrix.layout == torch.sparse_coo:
        return (matrix._indices(),), matrix._values()
    raise ValueError(f"Not supported matrix layout: {matrix.layout}")


def hccf_plan(matrix: torch.Tensor):
    """(HccfPlan, stored values in the plan's order) of a U x I sparse matrix, the plan cached the way csr_plan caches: on
    the addresses and versions of the index tensors, which the entry keeps alive."""
    keep, vals = _hccf_pattern(matrix)
    key = tuple(t.data_ptr() for t in keep) + (vals.numel(), tuple(matrix.shape), str(vals.device))
    plan = _hccf_plans.get(key)
    if plan is not None and plan.keep_versions != tuple(t._version for t in keep):
        plan = None
    if plan is not None:
        hccf_plan_stats["hit"] += 1
        return plan, vals
    U, I = matrix.shape
    if matrix.layout == torch.sparse_coo:
        idx = keep[0]
        flat = idx[0] * I + idx[1]
        if idx.shape[1] > 1 and not bool((flat[1:] > flat[:-1]).all()):      # (one sync, once per index tensor)
            matrix = matrix.coalesce()
            keep, vals = (matrix.indices(),), matrix.values()
            idx = keep[0]
            key = (idx.data_ptr(), vals.numel(), tuple(matrix.shape), str(vals.device))
        crow = torch.zeros(U + 1, dtype=torch.int64, device=idx.device)
        crow[1:] = torch.cumsum(torch.bincount(idx[0], minlength=U), 0)
        col = idx[1]
    else:
        crow, col = keep
    if len(_hccf_plans) > 16:
        _hccf_plans.clear()
    plan = HccfPlan(crow, col, (U, I), keep)
    _hccf_plans[key] = plan
    hccf_plan_stats["built"] += 1
    return plan, vals


def _hccf_layer_fwd(sq: CsrPlan, val, S, S_out, R, R_out, scale, slope, bits, D):
    sr, lr = sq.short_rows, sq.long_rows
    _lib.check(
        _lib.load().mi_hccf_fwd(sq.crow.data_ptr(), sq.col.data_ptr(), val.data_ptr(), S[0].data_ptr(), _lib.ptr(S[1]), S[2],
                                _lib.ptr(S_out), R[0].data_ptr(), _lib.ptr(R[1]), R[2], R_out.data_ptr(), float(scale),
                                float(slope), _lib.ptr(bits), sq.shape[0], D, sr.data_ptr() if sr.numel() else None, sr.numel(),
                                lr.data_ptr() if lr.numel() else None, lr.numel(), _lib.stream_ptr(val.device)),
        "mi_hccf_fwd")


def _hccf_layer_bwd(sq: CsrPlan, val, G, xscale, bits, slope, g, cg, out, D, xmask=None):
    sr, lr = sq.short_rows, sq.long_rows
    _lib.check(
        _lib.load().mi_hccf_bwd(sq.crow.data_ptr(), sq.col.data_ptr(), val.data_ptr(), G[0].data_ptr(), _lib.ptr(G[1]), G[2],
                                float(xscale), _lib.ptr(bits), float(slope), g[0].data_ptr(), _lib.ptr(g[1]), g[2], float(cg),
                                out.data_ptr(), sq.shape[0], D, sr.data_ptr() if sr.numel() else None, sr.numel(),
                                lr.data_ptr() if lr.numel() else None, lr.numel(), _lib.ptr(xmask),
                                _lib.stream_ptr(val.device)),
        "mi_hccf_bwd")


class HCCFPropagate(torch.autograd.Function):
    """S_k = S_{k-1} + LeakyReLU(A_k S_{k-1}),  out = (S_0 + ... + S_L) / (L + 1)  with S_0 = [Xu; Xi] and A_k the block
    adjacency of the k-th value tensor — one launch per layer each way.  Kept for the backward: per layer the value
    tensor and ONE BIT per element of the pre-activation (none when slope == 1), no [N, D] float."""

    @staticmethod
    def forward(ctx, Xu, Xi, plan: HccfPlan, num_layers: int, slope: float, *vals):
        dev = _lib.require_gpu(Xu, Xi, *vals)
        Xuc, Xic = _f32c(Xu), _f32c(Xi)
        U, I = plan.shape
        if Xuc.shape[0] != U or Xic.shape[0] != I or Xuc.shape[1] != Xic.shape[1]:
            raise ValueError(f"the matrix is {plan.shape} but the tables are {tuple(Xuc.shape)} and {tuple(Xic.shape)}")
        N, D, L, sq = U + I, Xuc.shape[1], num_layers, plan.square
        need_bits = slope != 1 and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        R = torch.empty((N, D), dtype=torch.float32, device=dev)
        bufs = [torch.empty((N, D), dtype=torch.float32, device=dev) for _ in range(min(2, L - 1))]
        S, bits = (Xuc, Xic, U), []
        for k in range(1, L + 1):
            last = k == L
            S_out = None if last else bufs[(k - 1) % len(bufs)]          # ping-pong: other rows still gather S
            b = torch.empty((N, (D + 31) // 32), dtype=torch.int32, device=dev) if need_bits else None
            _hccf_layer_fwd(sq, vals[k - 1], S, S_out, (Xuc, Xic, U) if k == 1 else (R, None, 0), R,
                            1.0 / (L + 1) if last else 1.0, slope, b, D)
            if need_bits:
                bits.append(b)
            S = (S_out, None, 0)
        ctx.plan, ctx.num_layers, ctx.slope, ctx.n_bits = plan, L, slope, len(bits)
        ctx.save_for_backward(*bits, *vals)
        return R[:U], R[U:]

    @staticmethod
    def backward(ctx, gu, gi):
        saved = ctx.saved_tensors
        bits, vals = saved[:ctx.n_bits], saved[ctx.n_bits:]
        plan, L, slope = ctx.plan, ctx.num_layers, ctx.slope
        U, I = plan.shape
        dev = vals[0].device
        D = (gu if gu is not None else gi).shape[1]
        gu = _f32c(gu) if gu is not None else torch.zeros((U, D), dtype=torch.float32, device=dev)
        gi = _f32c(gi) if gi is not None else torch.zeros((I, D), dtype=torch.float32, device=dev)
        c = 1.0 / (L + 1)
        g = (gu, gi, U)
        # the incoming gradient is non-zero on the batch's rows only: the first step does not fetch the others
        xmask = _row_mask(gu, gi, D) if MASK_FIRST_BACKWARD_LAYER else None
        bufs = [torch.empty((U + I, D), dtype=torch.float32, device=dev) for _ in range(min(2, L))]
        G, xscale, out = g, c, None
        for k in range(L, 0, -1):            # G_{k-1} = c g + G_k + A_k (G_k . f_k); G_L = c g is never stored
            out = bufs[(L - k) % len(bufs)]
            _hccf_layer_bwd(plan.square, vals[k - 1], G, xscale, bits[k - 1] if bits else None, slope, g, c, out, D,
                            xmask=xmask if k == L else None)
            G, xscale = (out, None, 0), 1.0
        return (out[:U], out[U:], None, None, None) + (None,) * L


def hccf_propagate(matrix, Xu: torch.Tensor, Xi: torch.Tensor, num_layers: int, slope: float):
    """(user_emb, item_emb) of the HCCF backbone (src/models/hccf.py:36-68).  matrix: the U x I sparse matrix (COO as
    graph_utils.get_adj returns it, or CSR), or a list of `num_layers` such matrices over ONE sparsity pattern, layer k
    using the k-th (SparseDropout draws).  The block adjacency is planned once per pattern (hccf_plan); per layer the
    values cost one index_select.  No host sync and no data-dependent shape once the pattern has been seen."""
    if num_layers == 0:
        return Xu, Xi
    mats = list(matrix) if isinstance(matrix, (list, tuple)) else [matrix] * num_layers
    if len(mats) != num_layers:
        raise ValueError(f"{len(mats)} matrices for {num_layers} layers")
    plan, vals, seen = None, [], {}
    for m in mats:
        if id(m) in seen:
            vals.append(seen[id(m)])
            continue
        p, v = hccf_plan(m)
        if plan is not None and p is not plan:
            raise ValueError("the per-layer matrices must share one sparsity pattern (the same index tensors)")
        if v.requires_grad:
            raise NotImplementedError("gradients w.r.t. the adjacency values are not provided")
        plan = p
        seen[id(m)] = plan.values(v)
        vals.append(seen[id(m)])
    return HCCFPropagate.apply(Xu, Xi, plan, num_layers, float(slope), *vals)


# --------------------------------------------------------------------------------------
# fp32 MFMA GEMM with fused epilogues (building block of the CrossNet heads)
EPI = {"none": 0, "bias": 1, "tanh": 2, "cross": 3, "add": 4, "mul_dtanh": 5, "tanh_gate": 6, "accum": 7}


def gemm(A, B, C, M, N, K, lda, ldb, ldc, transA=False, transB=False, batch=1, sA=0, sB=0, sC=0,
         kgroups=1, gA=0, gB=0, epi="none", bias=None, R1=None, ldr1=0, sR1=0, R2=None, ldr2=0, sR2=0,
         rowscale=None, nrs=0, C2=None, ldc2=0, sC2=0, splitk=0):
    """Raw launcher of mi_gemm_f32 over torch buffers (pointers may be offset views).

    splitk=0 picks automatically: when the output is only a few 64x64 tiles but K is long (the
    weight-gradient shapes) the K loop is spread over enough workgroups to fill the 256 CUs."""
    dev = _lib.require_gpu(A, B, C)
    if splitk == 0:
        splitk = 1
        if epi in ("none", "accum"):
            tiles = -(-M // 64) * -(-N // 64) * batch
            ksteps = -(-K // 32) * kgroups
            if tiles < 256 and ksteps >= 16 and not DETERMINISTIC:   # slices meet in float atomics
                splitk = max(1, min(ksteps // 4, -(-512 // tiles), 65535 // max(batch, 1)))
        if splitk > 1 and epi == "none":
            if C.is_contiguous() and C.numel() == batch * M * N:
                C.zero_()
            else:
                _zero_strided(C, M, N, ldc, batch, sC)
    _lib.check(
        _lib.load().mi_gemm_f32(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, lda, ldb, ldc, int(transA),
                                int(transB), batch, sA, sB, sC, kgroups, gA, gB, EPI[epi], _lib.ptr(bias),
                                _lib.ptr(R1), ldr1, sR1, _lib.ptr(R2), ldr2, sR2, _lib.ptr(rowscale), nrs,
                                _lib.ptr(C2), ldc2, sC2, splitk, _lib.stream_ptr(dev)),
        "mi_gemm_f32",
    )
    return C


class _GemmProblem(_ctypes.Structure):      # mi_gemm_problem (include/mi355x_recsys.h)
    _fields_ = [("A", _ctypes.c_void_p), ("B", _ctypes.c_void_p), ("C", _ctypes.c_void_p),
                ("M", _ctypes.c_int32), ("N", _ctypes.c_int32), ("K", _ctypes.c_int32),
                ("lda", _ctypes.c_int32), ("ldb", _ctypes.c_int32), ("ldc", _ctypes.c_int32), ("batch", _ctypes.c_int32),
                ("sA", _ctypes.c_int64), ("sB", _ctypes.c_int64), ("sC", _ctypes.c_int64),
                ("splitk", _ctypes.c_int32), ("accumulate", _ctypes.c_int32)]


MAX_GEMM_PROBLEMS = 16


def auto_splitk(M, N, K, batch=1):
    """K-slices that fill the 256 CUs when the output is only a few 64x64 tiles (1 in deterministic mode: the slices meet
    in float atomics)."""
    tiles = -(-M // 64) * -(-N // 64) * batch
    ksteps = -(-K // 32)
    if tiles < 256 and ksteps >= 16 and not DETERMINISTIC:
        return max(1, min(ksteps // 4, -(-512 // tiles), 65535 // max(batch, 1)))
    return 1


def _multi_problem_array(chunk):
    """ctypes array of mi_gemm_problem for one launch.  splitk: the caller's value, else 0 = the library cuts the launch
    (gemm.hip auto_splitk: the slice count that loads the CUs most evenly, atomics priced in);
    deterministic mode never splits (slices meet in float atomics)."""
    arr = (_GemmProblem * len(chunk))()
    for d, q in zip(arr, chunk):
        batch = q.get("batch", 1)
        d.A, d.B, d.C = q["A"].data_ptr(), q["B"].data_ptr(), q["C"].data_ptr()
        d.M, d.N, d.K = q["M"], q["N"], q["K"]
        d.lda, d.ldb, d.ldc, d.batch = q["lda"], q["ldb"], q["ldc"], batch
        d.sA, d.sB, d.sC = q.get("sA", 0), q.get("sB", 0), q.get("sC", 0)
        d.splitk = q.get("splitk", 0) or (1 if DETERMINISTIC else 0)
        d.accumulate = int(bool(q.get("accumulate", False)))
    return arr


def gemm_multi_plan(problems, transA=False, transB=False):
    """(kind, workgroups, splitk[n]) of the launch gemm_multi would make for <= 16 problems (mi_gemm_f32_multi_plan: host
    arithmetic, no GPU work); kind 1 = the LDS-DMA kernel of the weight-gradient form, 0 = the general kernel."""
    arr = _multi_problem_array(problems)
    kind, wgs = _ctypes.c_int32(), _ctypes.c_int64()
    splitk = (_ctypes.c_int32 * max(1, len(problems)))()
    _lib.check(_lib.load().mi_gemm_f32_multi_plan(_ctypes.addressof(arr), len(problems), int(transA), int(transB),
                                                  _ctypes.addressof(kind), _ctypes.addressof(wgs), _ctypes.addressof(splitk)),
               "mi_gemm_f32_multi_plan")
    return kind.value, wgs.value, list(splitk[:len(problems)])


class PrefetchRowsJob(_ctypes.Structure):
    """mi_prefetch_rows_job: the NEXT batch's ids and the tables its lookup will read."""
    _fields_ = [("idx", _ctypes.c_void_p), ("offsets", _ctypes.c_void_p), ("W", _ctypes.c_void_p), ("w1", _ctypes.c_void_p),
                ("ldw", _ctypes.c_int64), ("ldw1", _ctypes.c_int64), ("B", _ctypes.c_int64), ("N", _ctypes.c_int64),
                ("F", _ctypes.c_int32)]


def gemm_multi(problems, transA=False, transB=False, ride: Optional[PrefetchRowsJob] = None):
    """problems: dicts with A, B, C (torch buffers / views), M, N, K, lda, ldb, ldc and optionally batch, sA, sB, sC, splitk
    (0 / absent = the library's cut), accumulate — all the same operand layout, independent of each other: ONE launch per 16
    problems (mi_gemm_f32_multi).  C of a problem must be zero (or accumulate) unless splitk == 1: the caller allocates
    them zero-filled.  ride: a prefetch job the (first) launch carries in extra workgroups (mi_gemm_f32_multi_ride)."""
    if not problems:
        if ride is not None:
            _lib.check(_lib.load().mi_gemm_f32_multi_ride(None, 0, int(transA), int(transB), _ctypes.byref(ride),
                                                          _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device()))),
                       "mi_gemm_f32_multi_ride")
        return
    dev = _lib.require_gpu(*[q[k] for q in problems for k in ("A", "B", "C")])
    lib, stream = _lib.load(), _lib.stream_ptr(dev)
    for i in range(0, len(problems), MAX_GEMM_PROBLEMS):
        chunk = problems[i:i + MAX_GEMM_PROBLEMS]
        arr = _multi_problem_array(chunk)
        _lib.check(lib.mi_gemm_f32_multi_ride(_ctypes.addressof(arr), len(chunk), int(transA), int(transB),
                                              _ctypes.byref(ride) if (ride is not None and i == 0) else None, stream),
                   "mi_gemm_f32_multi_ride")


PANEL_GEMM = True        # False: every product stays on the 64x64-tile kernel (mi_gemm_f32)


def gemm_panel(A, lda, B, ldb, b_layout, C, ldc, M, N, K, gw=None, gstride=0, epi="none", bias=None, R1=None, R2=None,
               rowscale=None, nrs=0, C2=None) -> bool:
    """mi_gemm_f32_panel over torch buffers; returns False — nothing launched — when the shape / alignment is outside that
    kernel, so the caller issues its mi_gemm_f32 form instead."""
    if gw is None:
        gw = K if b_layout == 0 else N
    if not PANEL_GEMM or M == 0 or any(v % 4 for v in (lda, ldb, ldc, N, K, gw, gstride)) or epi not in ("none", "tanh", "cross", "add"):
        return False
    if any(t is not None and t.data_ptr() % 16 for t in (A, B, C, bias, R1, R2, C2)):
        return False
    dev = _lib.require_gpu(A, B, C)
    _lib.check(_lib.load().mi_gemm_f32_panel(A.data_ptr(), lda, B.data_ptr(), ldb, b_layout, gw, gstride, C.data_ptr(), ldc, M, N,
                                             K, EPI[epi], _lib.ptr(bias), _lib.ptr(R1), _lib.ptr(R2), _lib.ptr(rowscale), nrs,
                                             _lib.ptr(C2), _lib.stream_ptr(dev)), "mi_gemm_f32_panel")
    return True


def _zero_strided(C, M, N, ldc, batch, sC):
    for z in range(batch):
        torch.as_strided(C, (M, N), (ldc, 1), C.storage_offset() + z * sC).zero_()


# --------------------------------------------------------------------------------------
# TT-Rec lookup
import ctypes as _ct  # noqa: E402


def _tt_host_args(cores, p_shapes, q_shapes, ranks):
    n = len(cores)
    ptrs = (_ct.c_void_p * n)(*[c.data_ptr() for c in cores])
    return (ptrs, (_ct.c_int32 * n)(*p_shapes), (_ct.c_int32 * n)(*q_shapes), (_ct.c_int32 * (n + 1))(*ranks))


class TTLookup(torch.autograd.Function):
    """out[n, D] = TT-Rec rows (tensortrain_embeddings.py:128-150); dense core grads via atomics."""

    @staticmethod
    def forward(ctx, idx, num_item: int, p_shapes, q_shapes, ranks, *cores):
        dev = _lib.require_gpu(idx, *cores)
        idxc = _i64c(idx).view(-1)
        cs = [_f32c(c) for c in cores]
        D = 1
        for q in q_shapes:
            D *= q
        out = torch.empty((idxc.numel(), D), dtype=torch.float32, device=dev)
        ptrs, p, q, r = _tt_host_args(cs, p_shapes, q_shapes, ranks)
        _lib.check(
            _lib.load().mi_tt_fwd(idxc.data_ptr(), ptrs, len(cs), p, q, r, out.data_ptr(), idxc.numel(), D,
                                  num_item, _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
            "mi_tt_fwd",
        )
        ctx.save_for_backward(idxc, *cs)
        ctx.meta = (num_item, list(p_shapes), list(q_shapes), list(ranks), D)
        return out

    @staticmethod
    def backward(ctx, g):
        idxc, *cs = ctx.saved_tensors
        num_item, p_shapes, q_shapes, ranks, D = ctx.meta
        g = _f32c(g)
        gcs = [torch.zeros_like(c) for c in cs]
        ptrs, p, q, r = _tt_host_args(cs, p_shapes, q_shapes, ranks)
        gptrs = (_ct.c_void_p * len(gcs))(*[c.data_ptr() for c in gcs])
        _lib.check(
            _lib.load().mi_tt_bwd(idxc.data_ptr(), g.data_ptr(), ptrs, gptrs, len(cs), p, q, r, idxc.numel(), D,
                                  num_item, _lib.stream_ptr(g.device)),
            "mi_tt_bwd",
        )
        return (None, None, None, None, None, *gcs)


# ---- grouped form: one MFMA GEMM per core slice (csrc/tt_grouped.hip, gemm.hip) ------------------
_TT_TILE = 64            # rows per GEMM tile: the rows of a digit group are padded to whole tiles
_TT_SEG = 2048           # reduction rows per slice-gradient segment (long groups are cut, float atomics join)
_TT_SEG0 = 256           # rows per segment of core 0's gradient sum
_TT_GROUPED_MIN = 4096   # below this many lookups the sort / planning launches cost more than they save
_TT_MAX_TILES = 65535    # gridDim.y
_TT_PLAN_MAX_P = 4096    # digits per level the device planner handles (beyond: torch sort / searchsorted)


class _TTLevelPlan:
    """Layout of one level: the lookups ordered by `digit`, each owning `H` consecutive rows, every digit
    group padded to whole 64-row tiles.  Built with device-side torch ops only (sort, searchsorted,
    cumsum): no host sync, static shapes."""

    def __init__(self, digit: torch.Tensor, H: int, p: int, seg: int):
        dev, n = digit.device, digit.numel()
        if p <= _TT_PLAN_MAX_P:
            # counting sort on the device: 3 launches instead of ~25 torch ops
            self.ntiles = (n * H + _TT_TILE - 1) // _TT_TILE + p
            self.mpad = self.ntiles * _TT_TILE
            self.nseg = (n * H + seg - 1) // seg + p
            ws = torch.empty(2 * p, dtype=torch.int32, device=dev)
            pbeg = torch.empty(p, dtype=torch.int64, device=dev)
            self.pos = torch.empty(n, dtype=torch.int64, device=dev)
            self.mtile_b = torch.empty(self.ntiles, dtype=torch.int32, device=dev)
            self.kseg = torch.empty((self.nseg, 3), dtype=torch.int64, device=dev)
            _lib.check(_lib.load().mi_tt_plan_level(digit.data_ptr(), n, p, H, seg, ws.data_ptr(), pbeg.data_ptr(),
                                                    self.pos.data_ptr(), self.mtile_b.data_ptr(), self.ntiles,
                                                    self.kseg.data_ptr(), self.nseg, _lib.stream_ptr(dev)),
                       "mi_tt_plan_level")
            return
        sorted_d, perm = torch.sort(digit, stable=True)
        bounds = torch.searchsorted(sorted_d, torch.arange(p + 1, device=dev, dtype=digit.dtype))   # [p+1]
        starts, cnt = bounds[:-1], bounds[1:] - bounds[:-1]
        rows = cnt * H
        rpad = (rows + (_TT_TILE - 1)) // _TT_TILE * _TT_TILE
        pend = torch.cumsum(rpad, 0)
        pbeg = pend - rpad
        self.ntiles = (n * H + _TT_TILE - 1) // _TT_TILE + p          # static upper bound
        self.mpad = self.ntiles * _TT_TILE
        t0 = torch.arange(self.ntiles, device=dev) * _TT_TILE
        g_t = torch.searchsorted(pend, t0, right=True)
        self.mtile_b = torch.where(g_t < p, g_t, torch.full_like(g_t, -1)).to(torch.int32)
        g_s = sorted_d.to(torch.int64)
        pos_sorted = pbeg[g_s] + (torch.arange(n, device=dev) - starts[g_s]) * H
        self.pos = torch.empty(n, dtype=torch.int64, device=dev)      # first row of every ORIGINAL lookup
        self.pos[perm] = pos_sorted
        # reduction segments of at most `seg` rows, none straddling a group
        chunks = (rows + (seg - 1)) // seg
        cend = torch.cumsum(chunks, 0)
        self.nseg = (n * H + seg - 1) // seg + p
        j = torch.arange(self.nseg, device=dev)
        g_j = torch.searchsorted(cend, j, right=True)
        live = g_j < p
        g_c = torch.where(live, g_j, torch.zeros_like(g_j))
        local = j - (cend[g_c] - chunks[g_c])
        k0 = pbeg[g_c] + local * seg
        K = torch.where(live, torch.minimum(rows[g_c] - local * seg, torch.full_like(local, seg)), torch.zeros_like(local))
        self.kseg = torch.stack([k0, K, g_c], 1).contiguous()          # int64 [nseg, 3]


def _move(src, src_row, src_stride, dst, dst_row, dst_stride, width, n, mask=None, accumulate=False):
    _lib.check(
        _lib.load().mi_move_chunks(src.data_ptr(), _lib.ptr(src_row), src_stride, dst.data_ptr(), _lib.ptr(dst_row),
                                   dst_stride, width, n, _lib.ptr(mask), 1 if accumulate else 0,
                                   _lib.stream_ptr(dst.device)),
        "mi_move_chunks",
    )


def tt_grouped_supported(n: int, q_shapes, ranks) -> bool:
    """The grouped form needs 16-byte chunk widths / strides, at least two cores, enough lookups to
    amortise the planning, and tile counts within one grid dimension."""
    ncores = len(q_shapes)
    if ncores < 2 or n < _TT_GROUPED_MIN:
        return False
    H = 1
    for c in range(ncores):
        H *= q_shapes[c]
        if (q_shapes[c] * ranks[c + 1]) % 4 or (c > 0 and ranks[c] % 4):
            return False
    return H % 4 == 0


def _tt_last_fast(H: int, K: int, q: int) -> bool:
    """The last level (rank 1 on the right) has a dedicated kernel when its H*q outputs tile a wave."""
    D = H * q
    return D <= 64 and 64 % D == 0 and K * q <= 512 and H * K <= 512


class TTLookupGrouped(torch.autograd.Function):
    """out[n, D] = TT-Rec rows: levels 1..n-2 as GEMMs grouped by that level's digit, the last level (q_last
    columns wide) by its own kernel straight from the previous level's layout."""

    @staticmethod
    def forward(ctx, idx, num_item: int, p_shapes, q_shapes, ranks, *cores):
        dev = _lib.require_gpu(idx, *cores)
        lib = _lib.load()
        stream = _lib.stream_ptr(dev)
        idxc = _i64c(idx).view(-1)
        cs = [_f32c(c) for c in cores]
        n, nc = idxc.numel(), len(cs)
        digits = torch.empty((nc, n), dtype=torch.int32, device=dev)
        valid = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.check(lib.mi_tt_digits(idxc.data_ptr(), n, num_item, (_ct.c_int32 * nc)(*p_shapes), nc, digits.data_ptr(),
                                    valid.data_ptr(), _lib.err_word(dev).data_ptr(), stream), "mi_tt_digits")
        Hs = [1]
        for q in q_shapes:
            Hs.append(Hs[-1] * q)                                   # Hs[c] = rows per lookup entering level c
        D = Hs[-1]
        last = nc - 1
        fast_last = _tt_last_fast(Hs[last], ranks[last], q_shapes[last])
        gemm_levels = list(range(1, last if fast_last else nc))
        plans = {c: _TTLevelPlan(digits[c], Hs[c], p_shapes[c], _TT_SEG) for c in gemm_levels}
        d0 = digits[0].to(torch.int64)
        w0 = q_shapes[0] * ranks[1]
        out = torch.empty((n, D), dtype=torch.float32, device=dev)
        saved_A = []
        src, src_row, src_stride = cs[0], d0, w0                    # where the next level finds a lookup's rows
        if gemm_levels:
            # level 1 operand: core 0's slices [q_0, r_1] dropped into level 1's layout
            A = torch.empty((plans[1].mpad, ranks[1]), dtype=torch.float32, device=dev)
            _move(cs[0], d0, w0, A, plans[1].pos, ranks[1], w0, n, mask=valid)
        for c in gemm_levels:
            K, Nn = ranks[c], q_shapes[c] * ranks[c + 1]
            C = torch.empty((plans[c].mpad, Nn), dtype=torch.float32, device=dev)
            _lib.check(lib.mi_gemm_f32_row_groups(A.data_ptr(), cs[c].data_ptr(), C.data_ptr(), plans[c].mpad, Nn, K,
                                                  K, Nn, Nn, 0, K * Nn, plans[c].mtile_b.data_ptr(), stream),
                       "mi_gemm_f32_row_groups")
            saved_A.append(A)
            width = Hs[c] * Nn                                      # a lookup's rows, contiguous
            if c + 1 in plans:
                A = torch.empty((plans[c + 1].mpad, ranks[c + 1]), dtype=torch.float32, device=dev)
                _move(C, plans[c].pos, Nn, A, plans[c + 1].pos, ranks[c + 1], width, n)
            elif c == last:
                _move(C, plans[c].pos, Nn, out, None, D, width, n)
            else:
                src, src_row, src_stride = C, plans[c].pos, Nn      # feeds the last level where it lies
        if fast_last:
            _lib.check(lib.mi_tt_last_fwd(src.data_ptr(), src_row.data_ptr(), src_stride, cs[last].data_ptr(),
                                          digits[last].data_ptr(), valid.data_ptr(), Hs[last], ranks[last],
                                          q_shapes[last], out.data_ptr(), n, stream), "mi_tt_last_fwd")
        ctx.save_for_backward(digits, valid, src if fast_last else digits, *cs, *saved_A)
        ctx.plans = plans
        ctx.meta = (num_item, list(p_shapes), list(q_shapes), list(ranks), Hs, n, fast_last)
        return out

    @staticmethod
    def backward(ctx, g):
        num_item, p_shapes, q_shapes, ranks, Hs, n, fast_last = ctx.meta
        nc = len(p_shapes)
        digits, valid, last_src, *rest = ctx.saved_tensors
        cs, As = rest[:nc], rest[nc:]
        plans = ctx.plans
        dev = g.device
        lib = _lib.load()
        stream = _lib.stream_ptr(dev)
        g = _f32c(g)
        D = Hs[-1]
        gcs = [torch.zeros_like(c) for c in cs]
        last = nc - 1
        d0 = digits[0].to(torch.int64)
        w0 = q_shapes[0] * ranks[1]
        plan0 = X = None

        def level0_buffer():
            # core 0's gradient: the lookups ordered by their first digit, each group's rows summed
            nonlocal plan0, X
            plan0 = _TTLevelPlan(digits[0], 1, p_shapes[0], _TT_SEG0)
            X = torch.empty((plan0.mpad, w0), dtype=torch.float32, device=dev)

        dC = None
        if fast_last:
            H, K, q = Hs[last], ranks[last], q_shapes[last]
            planL = _TTLevelPlan(digits[last], 1, p_shapes[last], 16)          # digit order, <= 16 lookups per wave
            order = torch.empty(planL.mpad, dtype=torch.int64, device=dev)
            order[planL.pos] = torch.arange(n, device=dev)
            if nc == 2:
                level0_buffer()
                src_row, src_stride, dst, dst_row, dst_stride = d0, w0, X, plan0.pos, w0
            else:
                Np = q_shapes[last - 1] * ranks[last]
                dC = torch.empty((plans[last - 1].mpad, Np), dtype=torch.float32, device=dev)
                src_row, src_stride, dst, dst_row, dst_stride = plans[last - 1].pos, Np, dC, plans[last - 1].pos, Np
            _lib.check(lib.mi_tt_last_bwd(last_src.data_ptr(), src_row.data_ptr(), src_stride, cs[last].data_ptr(),
                                          digits[last].data_ptr(), valid.data_ptr(), H, K, q, g.data_ptr(),
                                          dst.data_ptr(), dst_row.data_ptr(), dst_stride, order.data_ptr(),
                                          planL.kseg.data_ptr(), planL.nseg, gcs[last].data_ptr(), n, stream),
                       "mi_tt_last_bwd")
            top = last - 1
        else:
            N_last = q_shapes[last] * ranks[last + 1]
            dC = torch.empty((plans[last].mpad, N_last), dtype=torch.float32, device=dev)
            _move(g, None, D, dC, plans[last].pos, N_last, D, n, mask=valid)
            top = last
        for c in range(top, 0, -1):
            K, Nn = ranks[c], q_shapes[c] * ranks[c + 1]
            A = As[c - 1]
            # slice gradients: gcore_c[i] += A_rows(i)^T . dC_rows(i)
            _lib.check(lib.mi_gemm_f32_k_groups(A.data_ptr(), dC.data_ptr(), gcs[c].data_ptr(), K, Nn, K, Nn, Nn, K * Nn,
                                                plans[c].kseg.data_ptr(), plans[c].nseg, stream), "mi_gemm_f32_k_groups")
            # input gradient: dA = dC . core_c[i]^T
            dA = torch.empty((plans[c].mpad, K), dtype=torch.float32, device=dev)
            _lib.check(lib.mi_gemm_f32_row_groups(dC.data_ptr(), cs[c].data_ptr(), dA.data_ptr(), plans[c].mpad, K, Nn,
                                                  Nn, Nn, K, 1, K * Nn, plans[c].mtile_b.data_ptr(), stream),
                       "mi_gemm_f32_row_groups")
            width = Hs[c] * K
            if c > 1:
                Np = q_shapes[c - 1] * ranks[c]
                dC = torch.empty((plans[c - 1].mpad, Np), dtype=torch.float32, device=dev)
                _move(dA, plans[c].pos, K, dC, plans[c - 1].pos, Np, width, n)
            else:
                level0_buffer()
                _move(dA, plans[1].pos, K, X, plan0.pos, w0, w0, n, mask=valid)
        if X is not None:
            _lib.check(lib.mi_segment_sum(X.data_ptr(), w0, w0, plan0.kseg.data_ptr(), plan0.nseg,
                                          gcs[0].data_ptr(), w0, stream), "mi_segment_sum")
        return (None, None, None, None, None, *gcs)


def tt_lookup(idx, cores, num_item, p_shapes, q_shapes, ranks):
    args = (num_item, tuple(p_shapes), tuple(q_shapes), tuple(ranks), *cores)
    n = idx.numel()
    if not tt_grouped_supported(min(n, _TT_GROUPED_MIN), q_shapes, ranks) or n < _TT_GROUPED_MIN:
        return TTLookup.apply(idx, *args)
    # a level's row tiles must fit one grid dimension: very large batches (get_weight over the whole
    # vocabulary) go through in pieces
    H = 1
    for q in q_shapes[:-1]:
        H *= q
    piece = (_TT_MAX_TILES - max(p_shapes) - 1) * _TT_TILE // H
    flat = idx.reshape(-1)
    if n <= piece:
        return TTLookupGrouped.apply(flat, *args)
    return torch.cat([TTLookupGrouped.apply(flat[i:i + piece], *args) for i in range(0, n, piece)])


# --------------------------------------------------------------------------------------
# single-table gather with a per-element transform (PEP / RetrainPep)
class XformGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, W, S, M, srs: int, scs: int, xform: int):
        dev = _lib.require_gpu(idx, W)
        idxc, Wc = _i64c(idx), _f32c(W)
        Sc = None if S is None else _f32c(S)
        Mc = None if M is None else M.to(torch.uint8).contiguous()
        N, D = Wc.shape
        out = torch.empty(tuple(idx.shape) + (D,), dtype=torch.float32, device=dev)
        _lib.check(
            _lib.load().mi_xform_gather_fwd(idxc.data_ptr(), Wc.data_ptr(), _lib.ptr(Sc), _lib.ptr(Mc), srs, scs,
                                            out.data_ptr(), idxc.numel(), D, N, xform,
                                            _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
            "mi_xform_gather_fwd",
        )
        ctx.save_for_backward(idxc, Wc, Sc, Mc)
        ctx.meta = (srs, scs, xform, tuple(W.shape), None if S is None else tuple(S.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        idxc, Wc, Sc, Mc = ctx.saved_tensors
        srs, scs, xform, Wshape, Sshape = ctx.meta
        _no_atomics_promised("the transformed (PEP / masked) gather backward")
        g = _f32c(g)
        N, D = Wc.shape
        gW = torch.zeros_like(Wc)
        gS = torch.zeros_like(Sc) if (Sc is not None and xform == XF_SOFT) else None
        _lib.check(
            _lib.load().mi_xform_gather_bwd(idxc.data_ptr(), g.data_ptr(), Wc.data_ptr(), _lib.ptr(Sc), _lib.ptr(Mc),
                                            srs, scs, gW.data_ptr(), _lib.ptr(gS), gS.numel() if gS is not None else 0,
                                            idxc.numel(), D, N, xform, _lib.stream_ptr(g.device)),
            "mi_xform_gather_bwd",
        )
        return None, gW.view(Wshape), (gS.view(Sshape) if gS is not None else None), None, None, None, None


def soft_threshold_gather(idx, W, s):
    """F.embedding(idx, sign(W)*relu(|W| - sigmoid(s))) with s broadcastable to W ([1], [D], [N,1], [N,D])."""
    srs, scs = _soft_strides(s, *W.shape)
    return XformGather.apply(idx, W, s, None, srs, scs, XF_SOFT)


def masked_gather(idx, W, mask):
    return XformGather.apply(idx, W, None, mask, 0, 0, XF_MASK)


class _MaskedGatherRowGrad(torch.autograd.Function):
    """out = (W * mask)[idx] with W.grad in ROW FORM (uncoalesced COO over idx, values g * mask[idx]) — what the reference's
    F.embedding(x, weight * mask, sparse=True) hands torch.optim.SparseAdam (src/models/embeddings/pep_embedding.py:215-221)."""

    @staticmethod
    def forward(ctx, idx, W, mask):
        with torch.no_grad():
            out = masked_gather(idx, W, mask)
        ctx.save_for_backward(_i64c(idx).reshape(-1), mask)
        ctx.wshape = tuple(W.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        flat, mask = ctx.saved_tensors
        D = ctx.wshape[1]
        vals = _f32c(g).reshape(-1, D) * mask.index_select(0, flat).to(torch.float32)
        return None, _coo(flat, vals, ctx.wshape), None


def masked_gather_row_grad(idx, W, mask):
    return _MaskedGatherRowGrad.apply(idx, W, mask)


class _DualMaskedGatherRowGrad(torch.autograd.Function):
    """out = (T1 * M1)[idx % mod1] + (T2 * M2)[idx // div2] with both gradients in row form (RetrainCerpEmbedding with
    sparse=True, src/models/embeddings/cerp_embedding.py:329-367)."""

    @staticmethod
    def forward(ctx, idx, T1, T2, M1, M2, mod1: int, div2: int):
        with torch.no_grad():
            out = dual_gather(idx, T1, T2, mod1=mod1, div2=div2, op="add", M1=M1, M2=M2)
        flat = _i64c(idx).reshape(-1)
        ctx.save_for_backward(flat, M1, M2)
        ctx.meta = (int(mod1), int(div2), tuple(T1.shape), tuple(T2.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        flat, M1, M2 = ctx.saved_tensors
        mod1, div2, s1, s2 = ctx.meta
        g2 = _f32c(g).reshape(-1, s1[1])
        i1, i2 = flat % mod1, torch.div(flat, div2, rounding_mode="floor")
        g1 = _coo(i1, g2 * M1.index_select(0, i1).to(torch.float32), s1) if ctx.needs_input_grad[1] else None
        gq = _coo(i2, g2 * M2.index_select(0, i2).to(torch.float32), s2) if ctx.needs_input_grad[2] else None
        return None, g1, gq, None, None, None, None


def dual_masked_gather_row_grad(idx, T1, T2, M1, M2, mod1: int, div2: int):
    return _DualMaskedGatherRowGrad.apply(idx, T1, T2, M1, M2, mod1, div2)


def gather_rows_quant(idx, W, scale=None, bias=None):
    """Dequantising row gather for fp16 / int8 / int16 tables (inference only)."""
    dev = _lib.require_gpu(idx, W)
    qtype = {torch.float16: 1, torch.int8: 2, torch.int16: 3}.get(W.dtype)
    if qtype is None:
        raise TypeError(f"unsupported quantised table dtype {W.dtype}")
    idxc, Wc = _i64c(idx), W.contiguous()
    N, D = Wc.shape
    out = torch.empty(tuple(idx.shape) + (D,), dtype=torch.float32, device=dev)
    _lib.check(
        _lib.load().mi_gather_rows_quant(idxc.data_ptr(), Wc.data_ptr(), qtype, _lib.ptr(scale), _lib.ptr(bias),
                                         out.data_ptr(), idxc.numel(), D, N, _lib.err_word(dev).data_ptr(),
                                         _lib.stream_ptr(dev)),
        "mi_gather_rows_quant",
    )
    return out


# ---- row-sharded lookup: device-side routing (csrc/route.hip) -----------------
def route_buckets(idx: torch.Tensor, offsets: Optional[torch.Tensor], world: int, num_rows: int, cap: int,
                  overflow: torch.Tensor, slot_out: Optional[torch.Tensor] = None):
    """Stable bucketing of rows = idx + offsets by owner = row % world.

    Returns (send_rows int64[world*cap] of owner-local rows, slot int64[idx.shape]); `overflow`
    is an int32[1] device word that gets 1 OR-ed in when a bucket exceeds `cap`."""
    dev = _lib.require_gpu(idx, offsets, overflow)
    lib = _lib.load()
    idxc = _i64c(idx)
    if overflow.dtype != torch.int32:
        raise TypeError("overflow must be an int32 device word")
    F = idxc.shape[-1] if idxc.dim() > 1 else 1
    off = None if offsets is None else _i64c(offsets.reshape(-1))
    if off is not None and off.numel() != F:
        raise ValueError(f"offsets must have {F} entries")
    n = idxc.numel()
    ws = torch.empty(int(lib.mi_route_workspace_elems(n, world)), dtype=torch.int32, device=dev)
    send_rows = torch.empty(world * cap, dtype=torch.int64, device=dev)
    slot = slot_out if slot_out is not None else torch.empty(idxc.shape, dtype=torch.int64, device=dev)
    if slot.numel() != n or slot.dtype != torch.int64 or not slot.is_contiguous():
        raise ValueError("slot_out must be a contiguous int64 tensor with one entry per lookup")
    _lib.check(
        lib.mi_route_buckets(idxc.data_ptr(), _lib.ptr(off), n, F, world, num_rows, cap, ws.data_ptr(),
                             send_rows.data_ptr(), slot.data_ptr(), overflow.data_ptr(),
                             _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
        "mi_route_buckets",
    )
    return send_rows, slot


def gather_pack_rows(local_rows: torch.Tensor, W: torch.Tensor, w1: torch.Tensor) -> torch.Tensor:
    """[m, D+4] packed rows (W[r,:], w1[r], 0, 0, 0) for the owner-local rows r."""
    dev = _lib.require_gpu(local_rows, W, w1)
    lib = _lib.load()
    rows = _i64c(local_rows.reshape(-1))
    Wc, w1c = _f32c(W), _f32c(w1)
    Nl, D = Wc.shape
    if w1c.numel() != Nl:
        raise ValueError("first-order shard must have one weight per embedding row")
    out = torch.empty((rows.numel(), D + 4), dtype=torch.float32, device=dev)
    _lib.check(
        lib.mi_gather_pack_rows(rows.data_ptr(), Wc.data_ptr(), w1c.data_ptr(), out.data_ptr(), rows.numel(), D,
                                Nl, _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
        "mi_gather_pack_rows",
    )
    return out


def unpack_rows(packed: torch.Tensor, D: int):
    """([m, D], [m]) contiguous copies of columns 0..D-1 and column D of packed rows [m, D+4] — one launch (mi_unpack_rows)."""
    dev = _lib.require_gpu(packed)
    pc = _f32c(packed)
    if pc.dim() != 2 or pc.shape[1] != D + 4:
        raise ValueError("unpack_rows: rows of D + 4 floats expected")
    m = pc.shape[0]
    vals = torch.empty((m, D), dtype=torch.float32, device=dev)
    lin = torch.empty((m,), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mi_unpack_rows(pc.data_ptr(), vals.data_ptr(), lin.data_ptr(), m, D, _lib.stream_ptr(dev)),
               "mi_unpack_rows")
    return vals, lin


def _slot_fm_forward(ctx, buf, slot, bias, segments=None, shared=False):
    """The forward of SlotFM and SlotFMUnique (one kernel: a shared slot is a repeated read).  Saved for the backward: emb
    and what addresses the slots' gradient rows — the slot ids, or routing's `segments` where lookups share slots."""
    dev = _lib.require_gpu(buf, slot, bias, segments)
    buf = _f32c(buf)
    slot = _i64c(slot)
    B, F = slot.shape
    D = buf.shape[1] - 4
    nslot = buf.shape[0] - 1
    if shared and (segments is None or segments.dtype != torch.int32 or not segments.is_contiguous()
                   or segments.numel() != 2 * nslot + B * F):
        raise ValueError(f"segments must be a contiguous int32 tensor of 2 * {nslot} + {B * F} entries")
    emb = torch.empty((B, F, D), dtype=torch.float32, device=dev)
    yfm = torch.empty((B,), dtype=torch.float32, device=dev)
    _lib.check(
        _lib.load().mi_slot_fm_fwd(slot.data_ptr(), buf.data_ptr(), buf.shape[0], _lib.ptr(bias), emb.data_ptr(),
                                   yfm.data_ptr(), B, F, D, _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
        "mi_slot_fm_fwd",
    )
    ctx.save_for_backward(emb, segments if shared else slot)
    ctx.meta = (B, F, D, buf.shape[0], bias is not None)
    ctx.set_materialize_grads(False)
    return emb, yfm


class SlotFM(torch.autograd.Function):
    """(emb[B,F,D], y_fm[B]) from the packed rows a sharded lookup received, addressed by slot
    (src/models/deepfm.py:88-98 on exchanged rows).  buf is [S+1, D+4] with row S all zeros (the
    dump slot); the gradient w.r.t. buf comes back in the same layout, ready for the all-to-all."""

    @staticmethod
    def forward(ctx, buf, slot, bias):
        return _slot_fm_forward(ctx, buf, slot, bias)

    @staticmethod
    def backward(ctx, g_emb, g_y):
        emb, slot = ctx.saved_tensors
        B, F, D, rows, has_bias = ctx.meta
        dev = emb.device
        lib = _lib.load()
        g_emb, g_y = _upstream(g_emb, g_y, B, dev)
        gbuf = None
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if (has_bias and ctx.needs_input_grad[2]) else None
        if ctx.needs_input_grad[0]:
            gbuf = torch.empty((rows, D + 4), dtype=torch.float32, device=dev)
            # the kernel zeroes rows [0, S) itself and never stores to the dump row: that row (what the all-to-all does not
            # ship, but part of the gradient autograd hands on) is zeroed here
            gbuf[rows - 1].zero_()
            _lib.check(
                lib.mi_slot_fm_bwd(slot.data_ptr(), emb.data_ptr(), g_y.data_ptr(), _lib.ptr(g_emb),
                                   gbuf.data_ptr(), _lib.ptr(gb), rows - 1, B, F, D, _lib.stream_ptr(dev)),
                "mi_slot_fm_bwd",
            )
        return gbuf, None, _bias_grad(gb, g_y, B, launched=gbuf is not None)


def slot_fm(buf, slot, bias):
    return SlotFM.apply(buf, slot, bias)



# ---- row-sharded lookup, de-duplicated: one slot per distinct row (csrc/route.hip, csrc/gather_fm.hip) ----------------
def route_buckets_unique(idx: torch.Tensor, offsets: Optional[torch.Tensor], world: int, num_rows: int, cap: int,
                         overflow: torch.Tensor, slot_out: Optional[torch.Tensor] = None,
                         segments_out: Optional[torch.Tensor] = None, send_out: Optional[torch.Tensor] = None,
                         field_sort: bool = True):
    """Bucketing of the DISTINCT rows = idx + offsets by owner = row % world (mi_route_buckets_unique): an owner's bucket
    holds its distinct rows in ascending local order, every lookup of a row shares the row's slot.

    Returns (send_rows int64[world*cap], slot int64[idx.shape], segments int32[2*world*cap + n]); `segments` is what
    slot_fm_unique's backward pulls through (layout: include/mi355x_recsys.h).  The rows are sorted first: field by field
    (mi_sort_field_rows) when `offsets` are given — they must then be the ascending field offsets, and an id outside
    its own field goes to the dump slot and raises the out-of-field bit, as that sort has it —, generically
    (torch.sort, stable) without offsets, beyond that sort's limits, or with field_sort=False."""
    dev = _lib.require_gpu(idx, offsets, overflow)
    lib = _lib.load()
    idxc = _i64c(idx)
    if overflow.dtype != torch.int32:
        raise TypeError("overflow must be an int32 device word")
    F = idxc.shape[-1] if idxc.dim() > 1 else 1
    off = None if offsets is None else _i64c(offsets.reshape(-1))
    if off is not None and off.numel() != F:
        raise ValueError(f"offsets must have {F} entries")
    n = idxc.numel()
    S = world * cap
    rows = idxc if off is None else idxc + off
    err = _lib.err_word(dev).data_ptr()
    stream = _lib.stream_ptr(dev)
    flat = rows.reshape(-1)
    found = _sort_fields(rows, off, num_rows, n // F, F) if field_sort and off is not None and idxc.dim() == 2 else None
    rs, perm = found if found is not None else torch.sort(flat, stable=True)
    ws = torch.empty(int(lib.mi_route_unique_workspace_elems(n, world)), dtype=torch.int32, device=dev)

    def _out(given, shape, dtype, what):
        if given is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if given.numel() != int(torch.Size(shape).numel()) or given.dtype != dtype or not given.is_contiguous() or given.device != dev:
            raise ValueError(f"{what} must be a contiguous {dtype} device tensor with {int(torch.Size(shape).numel())} entries")
        return given

    send_rows = _out(send_out, (S,), torch.int64, "send_out")
    slot = _out(slot_out, tuple(idxc.shape), torch.int64, "slot_out")
    segments = _out(segments_out, (2 * S + n,), torch.int32, "segments_out")
    _lib.check(
        lib.mi_route_buckets_unique(rs.data_ptr(), perm.data_ptr(), flat.data_ptr(), n, world, num_rows, cap, ws.data_ptr(),
                                    send_rows.data_ptr(), slot.data_ptr(), segments.data_ptr(), overflow.data_ptr(), err,
                                    stream),
        "mi_route_buckets_unique",
    )
    return send_rows, slot, segments


class SlotFMUnique(torch.autograd.Function):
    """SlotFM where lookups may SHARE slots (route_buckets_unique): the forward is the same kernel (repeated slots are
    repeated reads); the backward writes to every slot the sum of its lookups' gradient rows, in ascending lookup order
    and without float atomics (mi_slot_fm_bwd_segments).  `segments` must be the description routing made for `slot`."""

    @staticmethod
    def forward(ctx, buf, slot, bias, segments):
        return _slot_fm_forward(ctx, buf, slot, bias, segments, shared=True)

    @staticmethod
    def backward(ctx, g_emb, g_y):
        emb, segments = ctx.saved_tensors
        B, F, D, rows, has_bias = ctx.meta
        dev = emb.device
        lib = _lib.load()
        g_emb, g_y = _upstream(g_emb, g_y, B, dev)
        gbuf = None
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if (has_bias and ctx.needs_input_grad[2]) else None
        if ctx.needs_input_grad[0]:
            gbuf = torch.empty((rows, D + 4), dtype=torch.float32, device=dev)      # every row is written by the kernel
            ws = torch.empty(int(lib.mi_slot_fm_bwd_segments_workspace_elems(B, F, D)), dtype=torch.float32, device=dev)
            _lib.check(
                lib.mi_slot_fm_bwd_segments(segments.data_ptr(), emb.data_ptr(), g_y.data_ptr(), _lib.ptr(g_emb),
                                            ws.data_ptr(), gbuf.data_ptr(), _lib.ptr(gb), rows - 1, B, F, D,
                                            _lib.stream_ptr(dev)),
                "mi_slot_fm_bwd_segments",
            )
        return gbuf, None, _bias_grad(gb, g_y, B, launched=gbuf is not None), None


def slot_fm_unique(buf, slot, bias, segments):
    return SlotFMUnique.apply(buf, slot, bias, segments)


# ---- OptEmbed supernet for the CF tables (csrc/optembed_cf.hip) -------------------------------------------------------
_cf_seeds: Dict[int, list] = {}


def optembed_cf_seed(dev: torch.device) -> torch.Tensor:
    """int64 [2] on `dev`: the seed word of the CF OptEmbed draws and the launch ticket (kept zero between launches).
    Started from torch.initial_seed(), and restarted when that changes (outside a graph capture), so torch.manual_seed
    makes the draws reproducible; every drawing launch adds 1 to the word on the device (mlp._seed_word's scheme)."""
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    init = torch.initial_seed() & 0x7FFFFFFFFFFF
    ent = _cf_seeds.get(i)
    if ent is None:
        ent = [init, torch.tensor([init, 0], dtype=torch.int64, device=torch.device("cuda", i))]
        _cf_seeds[i] = ent
    elif ent[0] != init and not torch.cuda.is_current_stream_capturing():
        ent[1][0].fill_(init)
        ent[0] = init
    return ent[1]


class OptEmbedCF(torch.autograd.Function):
    """out = mi_optembed_cf_fwd over the whole table (row mask x dimension mask).  `k`: int64 widths given per row
    ([N]) or per field ([F], k_field), or the buffer the draw fills (draw = (law, hi, cdf, salt)); None keeps every
    dimension.  The backward is mi_optembed_cf_bwd: plain stores, fixed-order sums, no atomics."""

    @staticmethod
    def forward(ctx, W, t, t_field: bool, off, k, k_field: bool, norm: int, draw):
        dev = _lib.require_gpu(W, t, off, k)
        Wc = _f32c(W)
        tc = None if t is None else _f32c(t)
        N, D = Wc.shape
        out = torch.empty_like(Wc)
        law, hi, cdf, salt = draw if draw is not None else (0, D, None, 0)
        seed = optembed_cf_seed(dev) if draw is not None else None
        _lib.check(_lib.load().mi_optembed_cf_fwd(Wc.data_ptr(), _lib.ptr(tc), int(t_field), off.data_ptr(), off.numel() - 1,
                                                  _lib.ptr(k), int(k_field), int(draw is not None), law, hi, _lib.ptr(cdf),
                                                  _lib.ptr(seed), salt, norm, out.data_ptr(), N, D,
                                                  _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)), "mi_optembed_cf_fwd")
        ctx.save_for_backward(Wc, tc, off, k)
        ctx.meta = (bool(t_field), bool(k_field), norm)
        return out

    @staticmethod
    def backward(ctx, g):
        Wc, tc, off, k = ctx.saved_tensors
        t_field, k_field, norm = ctx.meta
        g = _f32c(g)
        N, D = Wc.shape
        dW = torch.empty_like(Wc) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(tc) if (tc is not None and ctx.needs_input_grad[1]) else None
        dt_rows = torch.empty(N, dtype=torch.float32, device=g.device) if (dt is not None and t_field) else None
        if dW is not None or dt is not None:
            _lib.check(_lib.load().mi_optembed_cf_bwd(Wc.data_ptr(), _lib.ptr(tc), int(t_field), off.data_ptr(),
                                                      off.numel() - 1, _lib.ptr(k), int(k_field), norm, g.data_ptr(),
                                                      _lib.ptr(dW), _lib.ptr(dt), _lib.ptr(dt_rows), N, D,
                                                      _lib.stream_ptr(g.device)), "mi_optembed_cf_bwd")
        return dW, dt, None, None, None, None, None, None


def optembed_cf(W, t, t_field: bool, off, norm: int, k=None, k_field: bool = False, draw=None):
    """(masked table [N, D], widths).  draw = (law, hi, cdf, salt): the widths are drawn on the device into a fresh int64
    buffer ([F] when k_field, else [N]) that is returned with the table; otherwise `k` is returned as given."""
    if draw is not None:
        k = torch.empty(off.numel() - 1 if k_field else W.shape[0], dtype=torch.int64, device=W.device)
    elif k is not None:
        k = _i64c(k)
    return OptEmbedCF.apply(W, t, t_field, off, k, k_field, norm, draw), k


def optembed_cf_draw(n: int, D: int, law: int, hi: int, cdf, salt: int, device) -> torch.Tensor:
    """n widths (int64, on the device) drawn by mi_optembed_cf_fwd's draw-only mode: the candidate masks of the search."""
    device = torch.device(device)
    k = torch.empty(n, dtype=torch.int64, device=device)
    off = torch.tensor([0, n], dtype=torch.int64, device=device)
    _lib.check(_lib.load().mi_optembed_cf_fwd(None, None, 0, off.data_ptr(), 1, k.data_ptr(), 0, 1, law, hi, _lib.ptr(cdf),
                                              optembed_cf_seed(device).data_ptr(), salt, 1, None, n, D, None,
                                              _lib.stream_ptr(device)), "mi_optembed_cf_fwd")
    return k


# ---- device-resident CF data (csrc/cf_data.hip) ------------------------------------------------------------------------
CF_SAMPLE_MODES = {"uniform": 0, "popularity": 1}


def cf_sample_triples(pair_user, pair_item, pair_crow, pos_crow, pos_col, num_items: int, mode: str, per_user_num: int,
                      K: int, first: int, n: int, seed: int, epoch: int, order=None):
    """(users [n], pos [n], neg [K, n]) int64: samples [first, first + n) of epoch `epoch` by mi_cf_sample_triples (see
    include/mi355x_recsys.h for the draw function).  pos_col is int32; `order` (popularity mode) is int64 [n]."""
    dev = _lib.require_gpu(pair_user, pair_item, pair_crow, pos_crow, pos_col, order)
    if pos_col.dtype != torch.int32 or not pos_col.is_contiguous():
        raise TypeError("pos_col must be a contiguous int32 tensor")
    for t in (pair_user, pair_item, pair_crow, pos_crow, order):
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous()):
            raise TypeError("the pair arrays, the row offsets and `order` must be contiguous int64 tensors")
    if order is not None and order.numel() != n:
        raise ValueError(f"order must name one pair per sample: {order.numel()} for {n} samples")
    U = pos_crow.numel() - 1
    if pair_crow.numel() != U + 1 or pair_user.numel() != pair_item.numel():
        raise ValueError("pair_crow / pos_crow must both be [U + 1] and pair_user / pair_item equally long")
    users = torch.empty(n, dtype=torch.int64, device=dev)
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    neg = torch.empty((K, n), dtype=torch.int64, device=dev)
    s64 = lambda v: ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)          # noqa: E731  (the seed as a two's-complement word)
    _lib.check(_lib.load().mi_cf_sample_triples(
        pair_user.data_ptr(), pair_item.data_ptr(), pair_crow.data_ptr(), pair_item.numel(), pos_crow.data_ptr(),
        pos_col.data_ptr(), pos_col.numel(), U, num_items, CF_SAMPLE_MODES[mode], per_user_num, K, _lib.ptr(order), s64(seed),
        s64(epoch), first, n, users.data_ptr(), pos.data_ptr(), neg.data_ptr(), _lib.err_word(dev).data_ptr(),
        _lib.stream_ptr(dev)), "mi_cf_sample_triples")
    return users, pos, neg


def ndcg_weights(k: int):
    """(weight, ideal) float64 [k] on the host: 1 / log2(j + 2) and its running sum, as ndcg_recall_at_k forms them."""
    weight = 1.0 / torch.log2(torch.arange(2, k + 2, dtype=torch.float64))
    return weight, torch.cumsum(weight, 0)


def ndcg_recall_rows(pred: torch.Tensor, users: torch.Tensor, crow: torch.Tensor, col: torch.Tensor, k: int):
    """(ndcg [n], recall [n]) float64 of the first k columns of pred int64 [n, >= k] against the truth rows of `users` in
    the CSR (crow int64 [U + 1], col int64, rows distinct and ascending) by mi_ndcg_recall_rows."""
    dev = _lib.require_gpu(pred, users, crow, col)
    if pred.dim() != 2 or pred.shape[1] < k or k < 1:
        raise ValueError(f"pred must be [n, >= k]; got {tuple(pred.shape)} for k = {k}")
    pred, users, crow, col = _i64c(pred), _i64c(users).view(-1), _i64c(crow), _i64c(col)
    n = pred.shape[0]
    if users.numel() != n:
        raise ValueError("one user per row of pred")
    weight, ideal = (t.to(dev) for t in ndcg_weights(k))
    ndcg = torch.empty(n, dtype=torch.float64, device=dev)
    recall = torch.empty(n, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().mi_ndcg_recall_rows(pred.data_ptr(), pred.stride(0), users.data_ptr(), n, k, crow.data_ptr(),
                                               col.data_ptr(), crow.numel() - 1, col.numel(), weight.data_ptr(),
                                               ideal.data_ptr(), ndcg.data_ptr(), recall.data_ptr(),
                                               _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)), "mi_ndcg_recall_rows")
    return ndcg, recall


# ---- CTR validation metric (csrc/ctr_metric.hip) -------------------------------------------------------------------------
AUC_RECORD_WORDS = 6        # mi_binary_auc's record as int64 words: S | P | N | NaN scores | labels outside {0, 1} | auc (double)
_auc_workspaces = {}


def _auc_workspace(dev, n: int) -> torch.Tensor:
    """mi_binary_auc's workspace, kept per device and size class (n rounded up to a power of two).  Launches that share one
    must run one after the other (everything on one stream does); nothing in it is state."""
    size = 1 << max(int(n) - 1, 0).bit_length()
    nbytes = int(_lib.load().mi_binary_auc_workspace_bytes(min(size, 2**31 - 1)))
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)      # a capture's memory belongs to its graph's pool
    key = (torch.device(dev).index, size)
    ws = _auc_workspaces.get(key)
    if ws is None:
        ws = _auc_workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def binary_auc_device(score: torch.Tensor, label: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mi_binary_auc of score float32 [n] against label uint8 [n] (both contiguous): the record as int64 [6] on the device
    (`auc_record` decodes a host copy).  out: int64 [6] to write into.  No sync, no read-back."""
    dev = _lib.require_gpu(score, label)
    n = score.numel()
    if score.dtype != torch.float32 or label.dtype != torch.uint8 or label.numel() != n:
        raise ValueError(f"score float32 [n] and label uint8 [n] expected; got {score.dtype} {tuple(score.shape)}, "
                         f"{label.dtype} {tuple(label.shape)}")
    if not (score.is_contiguous() and label.is_contiguous()):
        raise ValueError("score and label must be contiguous")
    if out is None:
        out = torch.empty(AUC_RECORD_WORDS, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.numel() != AUC_RECORD_WORDS or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous int64 [6] on the scores' device")
    ws = _auc_workspace(dev, n) if n else None
    _lib.check(_lib.load().mi_binary_auc(score.data_ptr(), label.data_ptr(), n, _lib.ptr(ws), out.data_ptr(),
                                         _lib.stream_ptr(dev)), "mi_binary_auc")
    return out


def auc_record(words: torch.Tensor) -> dict:
    """A host copy of mi_binary_auc's record (int64 [>= 6]) as {"S", "P", "N", "nan", "bad", "auc"}."""
    words = words.cpu()
    S, P, N, n_nan, n_bad = (int(v) for v in words[:5])
    return {"S": S, "P": P, "N": N, "nan": n_nan, "bad": n_bad, "auc": float(words[5:6].view(torch.float64))}


def ctr_metric_workspace(dev) -> torch.Tensor:
    """A zeroed workspace of mi_ctr_metric_append (its launches re-arm it); one per accumulator."""
    return torch.zeros(int(_lib.load().mi_ctr_metric_append_workspace_bytes()), dtype=torch.uint8, device=dev)


def ctr_metric_append(logits: torch.Tensor, labels: torch.Tensor, at: int, score_buf: torch.Tensor, label_buf: torch.Tensor,
                      loss_sum: torch.Tensor, ws: torch.Tensor) -> None:
    """mi_ctr_metric_append: logits float32 [b] and labels (int64 or float32 [b]) into score_buf / label_buf at `at`, the
    batch's BCE-with-logits sum onto loss_sum (float64 [1]).  One launch, no sync."""
    dev = _lib.require_gpu(logits, labels, score_buf, label_buf, loss_sum, ws)
    b = logits.numel()
    if logits.dtype != torch.float32 or labels.dtype not in (torch.int64, torch.float32) or labels.numel() != b:
        raise ValueError(f"logits float32 [b] and labels int64 / float32 [b] expected; got {logits.dtype} "
                         f"{tuple(logits.shape)}, {labels.dtype} {tuple(labels.shape)}")
    if score_buf.dtype != torch.float32 or label_buf.dtype != torch.uint8 or label_buf.numel() != score_buf.numel() \
            or loss_sum.dtype != torch.float64:
        raise ValueError("score_buf float32 [cap], label_buf uint8 [cap] and loss_sum float64 [1] expected")
    logits, labels = logits.contiguous(), labels.contiguous()
    _lib.check(_lib.load().mi_ctr_metric_append(logits.data_ptr(), labels.data_ptr(), 0 if labels.dtype == torch.int64 else 1,
                                                b, int(at), score_buf.data_ptr(), label_buf.data_ptr(), score_buf.numel(),
                                                loss_sum.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)),
               "mi_ctr_metric_append")


def gemm_multi_slots(problems, transA=False, transB=False):
    """LDS ring slots the LDS-DMA kernel would run that launch with (mi_gemm_f32_multi_slots: host arithmetic, no GPU
    work): 3 when all its workgroups are resident at three per CU, else 2; 0 when the general kernel takes the launch."""
    arr = _multi_problem_array(problems)
    slots = _ctypes.c_int32()
    _lib.check(_lib.load().mi_gemm_f32_multi_slots(_ctypes.addressof(arr), len(problems), int(transA), int(transB),
                                                   _ctypes.addressof(slots)), "mi_gemm_f32_multi_slots")
    return slots.value

"""The LFU row cache of the TT-Rec table (`tt_emb`): host side of csrc/tt_cache.hip and the cached entry points of
csrc/tt.hip.  Reference: src/models/embeddings/tt_embedding_ops.py:682-754 (update_cache -> preprocess_indices_sync ->
tt_forward + cache_forward, cache_populate).  The FBTT kernels behind those calls are not in the reference tree; the
buffers and the call sequence are, and this module keeps them.

Nothing here reads a device value back: the hit / miss split is a per-lookup int32 `loc` (row of cache_weight, or -1)
that the probe launch writes and the lookup launches read, so the same launches run in warmup (every loc is -1) and
after `populate` — a graph captured before populate stays valid after it.
"""
import ctypes as _ct
from enum import Enum, unique

import torch

from . import _kernels, _lib
from ._kernels import _f32c, _i64c, _tt_host_args

PROBE_BOUND = 64      # MI_TT_CACHE_PROBE_BOUND of include/mi355x_recsys.h


@unique
class OptimType(Enum):
    """The optimizer names of tt_embedding_ops.py:33-48.  Only membership in (SGD, EXACT_SGD) matters here: it decides the
    shape of the `optimizer_state` buffers."""
    SGD = "sgd"
    EXACT_SGD = "exact_sgd"
    LAMB = "lamb"
    ADAM = "adam"
    EXACT_ADAGRAD = "exact_adagrad"
    EXACT_ROWWISE_ADAGRAD = "exact_row_wise_adagrad"
    LARS_SGD = "lars_sgd"
    PARTIAL_ROWWISE_ADAM = "partial_row_wise_adam"
    PARTIAL_ROWWISE_LAMB = "partial_row_wise_lamb"

    def __str__(self):
        return self.value


def probe_count(idx, hashtbl, cache_freq, cache_state, num_item: int, cache_size: int, warm=None) -> torch.Tensor:
    """One launch: every id of `idx` found or inserted in `hashtbl`, its slot's frequency raised by one, and
    loc[i] = cache_state[slot] (int32; -1: untracked, not cached, or `warm` — a device int32 word — is non-zero)."""
    dev = _lib.require_gpu(idx, hashtbl, cache_freq, cache_state)
    idxc = _i64c(idx).view(-1)
    loc = torch.full((idxc.numel(),), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().mi_tt_cache_probe_count(idxc.data_ptr(), idxc.numel(), num_item, hashtbl.data_ptr(),
                                                   cache_freq.data_ptr(), cache_state.data_ptr(), hashtbl.numel(),
                                                   cache_size, _lib.ptr(warm), loc.data_ptr(),
                                                   _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)),
               "mi_tt_cache_probe_count")
    return loc


@torch.no_grad()
def rehash(hashtbl, cache_freq, cache_state) -> None:
    """Re-insert every occupied (id, freq, state) triple by this build's probe rule, in place.  A checkpoint written by
    another hash has its ids in other slots; on a table this build wrote, in direct addressing, nothing moves."""
    dev = _lib.require_gpu(hashtbl, cache_freq, cache_state)
    src = (hashtbl.clone(), cache_freq.clone(), cache_state.clone())
    hashtbl.fill_(-1)
    cache_freq.zero_()
    cache_state.fill_(-1)
    _lib.check(_lib.load().mi_tt_cache_rehash(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), src[0].numel(),
                                              hashtbl.data_ptr(), cache_freq.data_ptr(), cache_state.data_ptr(),
                                              hashtbl.numel(), _lib.stream_ptr(dev)), "mi_tt_cache_rehash")


@torch.no_grad()
def populate(hashtbl, cache_freq, cache_state, cache_weight, lookup) -> None:
    """The cached set becomes the min(cache_size, #tracked) tracked ids of highest frequency, ties to the smaller id:
    cache_weight[j] = lookup(ids)[j] for the j-th of them, cache_state[slot] = j there and -1 elsewhere, all in place.
    Static shapes and device ops only (two stable sorts stand for one sort on the composite key (-freq, id), which
    could overflow int64): rows past the number of tracked ids keep what they held.  `lookup(ids[C]) -> [C, D]`."""
    C = cache_weight.shape[0]
    if C == 0:
        return
    tracked = hashtbl >= 0
    by_id = torch.sort(torch.where(tracked, hashtbl, torch.full_like(hashtbl, torch.iinfo(torch.int64).max)), stable=True)[1]
    freq = torch.where(tracked, cache_freq, torch.full_like(cache_freq, -1))[by_id]
    slots = by_id[torch.sort(freq, descending=True, stable=True)[1][:C]]        # [C] distinct slots
    chosen = tracked[slots]
    rows = lookup(torch.where(chosen, hashtbl[slots], torch.zeros_like(slots)))
    cache_weight.copy_(torch.where(chosen[:, None], rows, cache_weight))
    cache_state.fill_(-1)
    cache_state[slots] = torch.where(chosen, torch.arange(C, device=slots.device), torch.full_like(slots, -1)).to(torch.int32)


def _cache_weight_grad(loc, g, C: int, D: int, stream):
    """Rows of g added at loc >= 0.  The scatter kernel skips rows outside [0, C); the sorted, atomics-free form of
    deterministic mode gets the misses as an extra row that is cut off."""
    if C == 0:
        return g.new_zeros((0, D))
    rows = loc.to(torch.int64)
    if _kernels.DETERMINISTIC:
        return _kernels._scatter_rows(torch.where(rows < 0, torch.full_like(rows, C), rows), g, C + 1, D, stream)[:C]
    return _kernels._scatter_rows(rows, g, C, D, stream)


class TTCachedLookup(torch.autograd.Function):
    """_kernels.TTLookup with the cache: out[i] = cache_weight[loc[i]] where loc[i] >= 0, the contraction elsewhere
    (mi_tt_fwd's statements, same bits).  Core gradients come from the uncached lookups only."""

    @staticmethod
    def forward(ctx, idx, loc, cache_weight, num_item: int, p_shapes, q_shapes, ranks, *cores):
        dev = _lib.require_gpu(idx, loc, cache_weight, *cores)
        idxc = _i64c(idx).view(-1)
        cs = [_f32c(c) for c in cores]
        cw = _f32c(cache_weight)
        C, D = cw.shape
        out = torch.zeros((idxc.numel(), D), dtype=torch.float32, device=dev)
        ptrs, p, q, r = _tt_host_args(cs, p_shapes, q_shapes, ranks)
        _lib.check(_lib.load().mi_tt_cached_fwd(idxc.data_ptr(), loc.data_ptr(), cw.data_ptr(), C, ptrs, len(cs), p, q, r,
                                                out.data_ptr(), idxc.numel(), D, num_item,
                                                _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)), "mi_tt_cached_fwd")
        ctx.save_for_backward(idxc, loc, *cs)
        ctx.meta = (num_item, list(p_shapes), list(q_shapes), list(ranks), C, D)
        return out

    @staticmethod
    def backward(ctx, g):
        idxc, loc, *cs = ctx.saved_tensors
        num_item, p_shapes, q_shapes, ranks, C, D = ctx.meta
        g = _f32c(g)
        stream = _lib.stream_ptr(g.device)
        gcs = [torch.zeros_like(c) for c in cs]
        ptrs, p, q, r = _tt_host_args(cs, p_shapes, q_shapes, ranks)
        gptrs = (_ct.c_void_p * len(gcs))(*[c.data_ptr() for c in gcs])
        _lib.check(_lib.load().mi_tt_cached_bwd(idxc.data_ptr(), loc.data_ptr(), C, g.data_ptr(), ptrs, gptrs, len(cs),
                                                p, q, r, idxc.numel(), D, num_item, stream), "mi_tt_cached_bwd")
        gcw = _cache_weight_grad(loc, g, C, D, stream) if ctx.needs_input_grad[2] else None
        return (None, None, gcw, None, None, None, None, *gcs)


def tt_cached_lookup(idx, loc, cache_weight, cores, num_item, p_shapes, q_shapes, ranks):
    """The lookup of a cached table: the per-lookup form (mi_tt_cached_fwd / mi_tt_cached_bwd) at every batch size.  A
    grouped MFMA form with the cached lookups in a dead digit group is not part of this build, so a cached table does not
    get tt_lookup's grouped form above _TT_GROUPED_MIN lookups; an uncached one (use_cache=False) does."""
    return TTCachedLookup.apply(idx.reshape(-1), loc, cache_weight, num_item, tuple(p_shapes), tuple(q_shapes), tuple(ranks),
                                *cores)

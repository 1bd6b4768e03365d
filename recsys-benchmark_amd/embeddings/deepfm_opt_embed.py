"""OptEmbed supernet embedding for DeepFM — reference: src/models/embeddings/deepfm_opt_embed.py:39-330 and
src/models/embeddings/optembed_utils.py:10-112.

Drop-in for the LOOKUP side of the class: same constructor, parameters (`_weight`, `_mask_e_module._t_param`),
buffers (`_full_mask_d`, `_mask_e_module._field_dims`), `forward` (training: a fresh uniform dimension mask per
(sample, field) and the per-field row mask; eval: lookups of the masked table), `get_weight(mask_d)`, `get_l_s`,
`get_sparsity`, `get_num_params`, `get_mask_e`, `get_submask`.  Gather, L1/L2 row norm, BinaryStep row mask and
triangular dimension mask are ONE HIP kernel (mi_optembed_fwd); its backward carries BinaryStep's surrogate
gradient to the table and the thresholds.  The eval path computes masked rows on the fly instead of caching a masked
copy of the table.

The other two stages of the recipe (deepfm_opt_embed.py:310-718 there) run on DeepFM's fused lookup with a kept width
per looked-up row (_kernels.gather_fm(keep=, fwidth=)): `OptEmbed.set_candidate(mask_d)` installs a search candidate in
persistent device buffers for the eval forwards that follow, `evol_search_deepfm` is the evolutionary search over such
candidates, `RetrainOptEmbed` the table retrained under the mask it found, and `build_retrain_deepfm` the DeepFM on it.
Neither the search nor a retraining step ever forms a masked copy of the table.
"""
import random
from collections import namedtuple
from typing import List, Optional, Tuple, Union

import torch
from torch import nn

from .. import _kernels, _lib
from .base import IEmbedding


def get_mask(hidden_size: int) -> torch.Tensor:
    """matrix[i][j] = 1 if i >= j (optembed_utils.py:10-22)."""
    return torch.tril(torch.ones((hidden_size, hidden_size), dtype=torch.bool))


def _masked_fm_lookup(self, x, offsets, w1, bias, sparse_w1: bool):
    """IEmbedding.fm_lookup of the two OptEmbed tables: a search candidate in eval, the retraining table in training and
    eval alike — the plain launch with a kept width per looked-up row, no masked copy of the table."""
    mask = self.fm_mask()
    if mask is None:
        return None
    W, keep, fwidth, sparse_W = mask
    return _kernels.gather_fm(x, offsets, W, w1, bias, sparse_W=sparse_W, sparse_w1=sparse_w1, keep=keep, fwidth=fwidth)


class _OptLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, t, idx, tix, F: int, dmax, norm: int):
        dev = _lib.require_gpu(W, idx)
        Wc = _kernels._f32c(W)
        idxc = _kernels._i64c(idx)
        tc = None if t is None else _kernels._f32c(t)
        tixc = None if tix is None else _kernels._i64c(tix)
        dmc = None if dmax is None else _kernels._i64c(dmax)
        N, D = Wc.shape
        out = torch.empty(tuple(idx.shape) + (D,), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().mi_optembed_fwd(idxc.data_ptr(), Wc.data_ptr(), _lib.ptr(tc), _lib.ptr(tixc), F,
                                               _lib.ptr(dmc), norm, out.data_ptr(), idxc.numel(), D, N,
                                               _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)), "mi_optembed_fwd")
        ctx.save_for_backward(Wc, tc, idxc, tixc, dmc)
        ctx.meta = (F, norm, tuple(W.shape), None if t is None else tuple(t.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        Wc, tc, idxc, tixc, dmc = ctx.saved_tensors
        F, norm, Wshape, tshape = ctx.meta
        g = _kernels._f32c(g)
        N, D = Wc.shape
        dW = torch.zeros_like(Wc) if ctx.needs_input_grad[0] else None
        dt = torch.zeros_like(tc) if (tc is not None and ctx.needs_input_grad[1]) else None
        _lib.check(_lib.load().mi_optembed_bwd(idxc.data_ptr(), Wc.data_ptr(), _lib.ptr(tc), _lib.ptr(tixc), F,
                                               _lib.ptr(dmc), norm, g.data_ptr(), _lib.ptr(dW), _lib.ptr(dt),
                                               idxc.numel(), D, N, _lib.stream_ptr(g.device)), "mi_optembed_bwd")
        return (None if dW is None else dW.view(Wshape), None if dt is None else dt.view(tshape), None, None, None,
                None, None)


class _MaskEmbeddingModule(nn.Module):
    """Holder of the thresholds (optembed_utils.py:46-86); the masking itself runs inside the lookup kernel."""

    def __init__(self, field_dims: torch.Tensor, t_init: float = 0, mode_threshold_e="field", norm=1):
        super().__init__()
        assert mode_threshold_e in ["feature", "field"]
        self.mode_threshold_e = mode_threshold_e
        self.register_buffer("_field_dims", field_dims)
        self._num_item = int(field_dims.sum())
        self._num_field = len(field_dims)
        self._t_param = nn.Parameter(torch.full((self._num_item if mode_threshold_e == "feature" else self._num_field,),
                                                float(t_init)))
        self._norm = norm


class OptEmbed(IEmbedding):
    def __init__(self, field_dims: Union[List[int], int], hidden_size: int, mode: Optional[str] = None,
                 t_init: Optional[float] = 0, mode_threshold_e="field", mode_threshold_d="field", norm=1,
                 target_sparsity: Optional[float] = None):
        super().__init__()
        if isinstance(field_dims, int):
            field_dims = [field_dims]
        assert mode in ["sum", "mean", "max", None]
        assert mode_threshold_e in ["field", "feature"]
        assert mode_threshold_d in ["field", "feature"]
        self._field_dims = torch.tensor(field_dims, dtype=torch.int64)
        self._num_item = int(self._field_dims.sum())
        self._num_field = len(field_dims)
        self._hidden_size = hidden_size
        self._weight = nn.Parameter(torch.empty((self._num_item, hidden_size)))
        nn.init.xavier_uniform_(self._weight)
        self._mode = mode
        self._t_init = t_init
        self._norm = norm
        self._mask_e_module = (nn.Identity() if t_init is None
                               else _MaskEmbeddingModule(self._field_dims, t_init, mode_threshold_e, norm))
        self.register_buffer("_full_mask_d", get_mask(hidden_size))
        # field of every row: thresholds / dimension masks given per field are addressed through it
        self.register_buffer("_row_field", torch.repeat_interleave(torch.arange(self._num_field), self._field_dims),
                             persistent=False)
        self._target_sparsity = target_sparsity
        self._mode_d = mode_threshold_d
        self._eval_mask_d = None           # set by get_weight(mask_d) for the eval lookups that follow
        # a search candidate (set_candidate): the row mask of the frozen thresholds, cached, and the two width sources of
        # the masked gather_fm in device buffers that persist from candidate to candidate
        self._alive: Optional[torch.Tensor] = None
        self._cand_keep: Optional[torch.Tensor] = None
        self._cand_fwidth: Optional[torch.Tensor] = None
        self._cand_keep_valid = False
        self._candidate = False

    # ---- pieces of the kernel call ---------------------------------------------------------------
    def _thresholds(self):
        return None if self._t_init is None else self._mask_e_module._t_param

    def _per_row(self, values: torch.Tensor, rows: torch.Tensor, per_field: bool) -> torch.Tensor:
        """values given per field or per feature -> one per looked-up row."""
        return values[self._row_field[rows]] if per_field else values[rows]

    def _lookup(self, rows, mask_d):
        t = self._thresholds()
        tix = None
        if t is not None:
            field_t = self._mask_e_module.mode_threshold_e == "field"
            tix = self._row_field[rows] if field_t else rows
        dmax = None
        if mask_d is not None:
            if mask_d.dtype == torch.bool:         # an explicit [num_item, D] mask: its row sums - 1 (prefix masks)
                dmax = self._per_row(mask_d.sum(1) - 1, rows, False)
            else:
                dmax = self._per_row(mask_d.to(rows.device), rows, self._mode_d == "field")
        return _OptLookup.apply(self._weight, t, rows, tix, self._num_field, dmax, self._norm)

    # ---- a search candidate on the fused DeepFM lookup ----------------------------------------------
    _ALIVE_CHUNK = 1 << 22      # rows per launch of the row-mask pass (bounds its [rows, D] scratch)

    def _alive_rows(self) -> torch.Tensor:
        """bool [num_item] on the table's device: BinaryStep(norm(W) - t) > 0, the rows get_mask_e() reports — read off
        the masked rows the eval lookup itself produces, so both agree to the bit.  Cached until the weights or the
        thresholds may have changed (train(), load_state_dict)."""
        dev = self._weight.device
        if self._alive is None or self._alive.device != dev:
            if self._t_init is None:
                alive = torch.ones(self._num_item, dtype=torch.bool, device=dev)
            else:
                with torch.no_grad():
                    alive = torch.cat([self._lookup(torch.arange(lo, min(lo + self._ALIVE_CHUNK, self._num_item), device=dev),
                                                    None).norm(1, 1) > 0
                                       for lo in range(0, self._num_item, self._ALIVE_CHUNK)])
            self._alive, self._cand_keep_valid = alive, False
        return self._alive

    def _drop_candidate_cache(self):
        self._alive, self._cand_keep_valid, self._candidate = None, False, False

    def train(self, mode: bool = True):
        if mode:                      # the weights and thresholds are about to move
            self._drop_candidate_cache()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self._drop_candidate_cache()
        return super()._load_from_state_dict(*args, **kwargs)

    def set_candidate(self, mask_d: torch.Tensor) -> None:
        """Install a search candidate for the eval forwards of a DeepFM that follow: mask_d integer [num_field]
        (mode_threshold_d="field") or [num_item] ("feature"), values in [0, D); the kept width is mask_d + 1, on the rows
        the frozen thresholds keep.  Written IN PLACE into persistent device buffers — keep uint8 [num_item], fwidth int32
        [num_field] — so a GraphedForward captured under one candidate replays correctly under the next.  Field mode
        writes only fwidth (keep = alive * D is built once); feature mode rewrites keep = alive * (mask_d + 1)."""
        D, dev = self._hidden_size, self._weight.device
        if D > _kernels.MASKED_MAX_D:
            raise NotImplementedError(f"set_candidate keeps one byte per width: hidden_size <= {_kernels.MASKED_MAX_D}")
        field = self._mode_d == "field"
        if not torch.is_tensor(mask_d) or mask_d.is_floating_point() or mask_d.dtype == torch.bool:
            raise TypeError("mask_d must be an integer tensor")
        if mask_d.shape != (self._num_field if field else self._num_item,):
            raise ValueError(f"mask_d must be [{self._num_field if field else self._num_item}], got {tuple(mask_d.shape)}")
        alive = self._alive_rows()
        if self._cand_keep is None or self._cand_keep.device != dev:
            self._cand_keep = torch.empty(self._num_item, dtype=torch.uint8, device=dev)
            self._cand_fwidth = torch.empty(self._num_field, dtype=torch.int32, device=dev)
            self._cand_keep_valid = False
        mask_d = mask_d.to(dev)
        if field:
            if not self._cand_keep_valid:
                self._cand_keep.copy_(alive * D)
            self._cand_fwidth.copy_(mask_d + 1)
        else:
            self._cand_keep.copy_(alive * (mask_d + 1))
        self._cand_keep_valid = field
        self._candidate = True

    def clear_candidate(self) -> None:
        self._candidate = False

    def fm_mask(self):
        """(table, keep, fwidth, row-form gradient) for DeepFM's masked gather_fm, or None when the lookup is not of that
        form: training, no candidate installed, a bag mode."""
        if self.training or not self._candidate or self._mode is not None:
            return None
        return self._weight, self._cand_keep, (self._cand_fwidth if self._mode_d == "field" else None), False

    fm_lookup = _masked_fm_lookup

    # ---- reference API -----------------------------------------------------------------------------
    def get_l_s(self):
        if self._t_init is None:
            return 0
        return torch.exp(-self._mask_e_module._t_param).sum()

    def get_weight(self, mask_d: Optional[torch.Tensor] = None):
        """The masked table (deepfm_opt_embed.py:148-200).  Training with mask_d=None samples a uniform dimension
        mask (per field or per feature, `mode_threshold_d`); eval with mask_d=None applies the row mask only."""
        dev = self._weight.device
        if self.training and mask_d is None:
            size = self._num_field if self._mode_d == "field" else self._num_item
            hidden = self._hidden_size
            if self._target_sparsity is not None and self._mode_d == "feature":
                assert self._target_sparsity >= 0.5, "Generate naive only could generate sparsity from 0.5"
                hidden = int(hidden * 2 * (1 - self._target_sparsity))
            mask_d = torch.randint(0, hidden, (size,), device=dev)
        if not self.training:
            self._eval_mask_d = mask_d
        return self._lookup(torch.arange(self._num_item, device=dev), mask_d)

    def forward(self, x, mask_d=None):
        """x: rows after offsets, [B, num_field] (or any shape in eval).  Training: every (sample, field) draws its own
        number of kept dimensions (deepfm_opt_embed.py:219-225; the argument is ignored as in the reference);
        `_forced_mask_d` (tests) replaces that draw."""
        if self.training:
            forced = self.__dict__.get("_forced_mask_d")
            dmax = forced if forced is not None else torch.randint(0, self._hidden_size, size=tuple(x.shape),
                                                                    device=self._weight.device)
            t = self._thresholds()
            if t is not None:
                assert self._mask_e_module.mode_threshold_e == "field", "Cannot apply field mask to input"
            emb = _OptLookup.apply(self._weight, t, x, None, self._num_field, dmax, self._norm)
        else:
            if mask_d is not None:
                self._eval_mask_d = mask_d
            emb = self._lookup(x, self._eval_mask_d)
        return _kernels.bag_reduce(emb, self._mode)

    def get_sparsity(self, get_n_params=False):
        with torch.no_grad():
            training, self.training = self.training, False
            emb = self._lookup(torch.arange(self._num_item, device=self._weight.device), None)
            self.training = training
        nnz = int(torch.count_nonzero(emb).item())
        sparsity = 1 - nnz / (emb.shape[0] * emb.shape[1])
        return (sparsity, nnz) if get_n_params else sparsity

    def get_num_params(self):
        return self.get_sparsity(True)[1]

    def get_mask_e(self):
        if self._t_init is None:
            return torch.ones(self._num_item, dtype=int)
        with torch.no_grad():
            emb = self._lookup(torch.arange(self._num_item, device=self._weight.device), None)
        return (emb.norm(1, 1) > 0).to(int).cpu()

    def get_submask(self) -> torch.Tensor:
        """Features still alive per unit of the dimension mask (per field or per feature)."""
        mask_e = self.get_mask_e()
        if self._mode_d == "feature":
            return mask_e
        out = torch.zeros(self._num_field, dtype=mask_e.dtype)
        return out.index_add_(0, self._row_field.cpu(), mask_e)


# ---- retraining under the searched mask (deepfm_opt_embed.py:632-718) -------------------------------------------------
def _delete_cache(module, grad_input, grad_output):
    module._cur_weight = None


class RetrainOptEmbed(IEmbedding):
    """RetrainOptEmbed of the reference: `init_mask(mask_e, mask_d)`, then weight = `_weight * _mask`.  The mask is held
    as ONE byte per row — keep uint8 [N] = mask_e * (mask_d of the row + 1), every row of `_mask` being a prefix — and a
    DeepFM on this table looks it up through the masked gather_fm: a step touches the batch's rows, never the table as
    a whole (the reference multiplies the whole table by the mask every step, its backward hook dropping the cache).
    `get_weight()` still returns `_weight * _mask` with the reference's cache behaviour (kept in `_cur_weight`, dropped by a
    backward through the module) for callers that ask for it, and
    `state_dict()` carries `_mask` [N, D] in the reference's dtype, built on demand from keep.

    sparse (optional extension): row-form (COO) gradients of `_weight`."""

    def __init__(self, field_dims: Union[List[int], int], hidden_size, mode: Optional[str] = None,
                 t_init: Optional[float] = 0, mode_threshold_e="field", mode_threshold_d="field", norm=1,
                 target_sparsity: Optional[float] = None, sparse: bool = False):
        super().__init__()
        if isinstance(field_dims, int):
            field_dims = [field_dims]
        assert mode in ["sum", "mean", "max", None]
        assert mode_threshold_d in ["field", "feature"]
        if hidden_size > _kernels.MASKED_MAX_D:
            raise NotImplementedError(f"RetrainOptEmbed keeps one byte per width: hidden_size <= {_kernels.MASKED_MAX_D}")
        self._field_dims = torch.tensor(field_dims, dtype=torch.int64)
        self._num_item = int(self._field_dims.sum())
        self._num_field = len(field_dims)
        self._mode_d = mode_threshold_d
        self._mode = mode
        self._hidden_size = hidden_size
        self.sparse_grad = bool(sparse)
        self._weight = nn.Parameter(torch.empty((self._num_item, hidden_size)))
        nn.init.xavier_uniform_(self._weight)      # (the reference leaves it uninitialised: torch.empty)
        self.register_buffer("_full_mask_d", get_mask(hidden_size))
        self.register_buffer("_keep", None, persistent=False)      # uint8 [N] once init_mask has run
        self._mask_dtype = torch.int64
        self._cur_weight: Optional[torch.Tensor] = None
        self._handle = None

    # ---- the mask ------------------------------------------------------------------------------------
    def init_mask(self, mask_e, mask_d):
        """keep = mask_e * (mask_d of the row + 1); mask_d per field (mode_threshold_d="field") or per row, mask_e per row.
        Returns `_mask` [N, D] as the reference does (its dtype: that of `_full_mask_d[mask_d] * mask_e`)."""
        dev = self._weight.device
        mask_e, mask_d = torch.as_tensor(mask_e), torch.as_tensor(mask_d)
        self._mask_dtype = torch.result_type(torch.empty(0, dtype=torch.bool), torch.empty(0, dtype=mask_e.dtype))
        mask_d = mask_d.to(dev)
        if self._mode_d == "field":
            mask_d = torch.repeat_interleave(mask_d, self._field_dims.to(dev), dim=0, output_size=self._num_item)
        if mask_d.shape != (self._num_item,) or mask_e.shape != (self._num_item,):
            raise ValueError("mask_e must be [num_item], mask_d [num_field] or [num_item] by mode_threshold_d")
        self._keep = ((mask_e.to(dev) != 0) * (mask_d + 1)).to(torch.uint8)
        self._cur_weight = None
        if self._handle is None:
            self._handle = self.register_full_backward_hook(_delete_cache)
        return self._mask

    @property
    def _mask(self) -> torch.Tensor:
        assert self._keep is not None, "Mask is not initialized"
        cols = torch.arange(self._hidden_size, device=self._keep.device)
        return (cols.unsqueeze(0) < self._keep.unsqueeze(1)).to(self._mask_dtype)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self._keep is not None:      # in the reference's key order: _weight, _mask, _full_mask_d
            destination[prefix + "_mask"] = self._mask
            destination.move_to_end(prefix + "_full_mask_d")

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        mask = state_dict.pop(prefix + "_mask", None)      # (popped: it is no registered parameter here)
        if mask is not None:
            if mask.shape != (self._num_item, self._hidden_size):
                raise ValueError(f"_mask must be [{self._num_item}, {self._hidden_size}], got {tuple(mask.shape)}")
            kept = mask != 0
            keep = kept.sum(1)
            cols = torch.arange(self._hidden_size, device=mask.device)
            if not torch.equal(kept, cols.unsqueeze(0) < keep.unsqueeze(1)):
                raise ValueError("RetrainOptEmbed holds a kept width per row: every row of _mask must be a prefix "
                                 "(ones, then zeros)")
            self._keep = keep.to(torch.uint8).to(self._weight.device)
            self._mask_dtype = mask.dtype
            self._cur_weight = None
            if self._handle is None:
                self._handle = self.register_full_backward_hook(_delete_cache)
        elif strict and self._keep is not None:
            missing_keys.append(prefix + "_mask")
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if mask is not None:
            state_dict[prefix + "_mask"] = mask      # the caller's dict is left as it was

    # ---- lookups -------------------------------------------------------------------------------------
    def fm_mask(self):
        """(table, keep, fwidth, row-form gradient) for DeepFM's masked gather_fm; None for a bag mode."""
        assert self._keep is not None, "Mask is not initialized"
        if self._mode is not None:
            return None
        return self._weight, self._keep, None, self.sparse_grad

    fm_lookup = _masked_fm_lookup

    def get_weight(self, mask_d: Optional[torch.Tensor] = None):
        self._cur_weight = self._weight * self._mask
        return self._cur_weight

    def forward(self, x, mask_d=None):
        """The lookup outside DeepFM's fused path: the looked-up rows of `_weight` times their rows of the mask (the same
        values as rows of `_weight * _mask`, without the whole-table product)."""
        assert self._keep is not None, "Mask is not initialized"
        rows = _kernels.gather_rows(x, self._weight, sparse=self.sparse_grad)
        cols = torch.arange(self._hidden_size, device=rows.device)
        return _kernels.bag_reduce(rows * (cols < self._keep[x].unsqueeze(-1)), self._mode)

    def get_sparsity(self, get_n_params=False):
        nnz = self.get_num_params()
        sparsity = 1 - nnz / (self._hidden_size * self._num_item)
        return (sparsity, nnz) if get_n_params else sparsity

    def get_num_params(self):
        assert self._keep is not None, "Mask is not initialized"
        return int(torch.clamp(self._keep.to(torch.int64), max=self._hidden_size).sum().item())


def build_retrain_deepfm(field_dims, model_config, mask_e, mask_d):
    """The DeepFM of the recipe's third stage: DeepFM(field_dims, **model_config) without the table its embedding_config
    names (the registry keeps refusing "deepfm_optembed_retrain": a retraining table is nothing without its masks), a
    RetrainOptEmbed built from that config's arguments attached as `model.embedding`, init_mask(mask_e, mask_d) called."""
    from ..deepfm import DeepFM

    model_config = dict(model_config)
    emb_config = dict(model_config.pop("embedding_config", None) or {})
    emb_config.pop("name", None)
    model = DeepFM(field_dims, **model_config, empty_embedding=True)
    model.embedding = RetrainOptEmbed(field_dims, model_config["num_factor"], mode=None, **emb_config)
    model._modules = {"embedding": model._modules.pop("embedding"), **model._modules}      # the reference's key order
    model.embedding.init_mask(mask_e, mask_d)
    return model


# ---- evolutionary mask search (deepfm_opt_embed.py:310-622) -----------------------------------------------------------
Candidate = DeepFMCandidate = namedtuple("Candidate", ["save_mask", "extra"])      # extra = (sub_mask, n_max)
MAX_REDRAWS = 10000


def candidate_sparsity(candidate: Candidate, hidden_size: Optional[int] = None):
    """1 - sum((mask + 1) * sub_mask) / n_max (deepfm_opt_embed.py:492-498; hidden_size is unused there too)."""
    sub_mask, n_max = candidate.extra
    return 1 - ((candidate.save_mask + 1) * sub_mask.to(candidate.save_mask.device)).sum() / n_max


def d_target_sparsity(target_sparsity, sub_mask: torch.Tensor, num_item: int):
    """The sparsity the width draw aims at, given that only sub_mask.sum() of num_item rows are still alive
    (deepfm_opt_embed.py:555-558)."""
    if target_sparsity is None:
        return None
    return 1 - (1 - target_sparsity) / (sub_mask.sum() / num_item)


def _draw(n: int, hidden_size: int, target_sparsity, method: int, device) -> torch.Tensor:
    """_sampling_by_weight(target_sparsity, hidden_size, n, method): int64 [n] widths - 1.  On a GPU the draw-only kernel
    of the CF search (cf_opt_embed.draw_widths); on the host inverse-CDF draws on torch.rand from the same law."""
    from . import cf_opt_embed as cf

    if torch.is_tensor(target_sparsity):
        target_sparsity = float(target_sparsity)
    device = torch.device(device)
    if device.type == "cuda":
        return cf.draw_widths(n, hidden_size, target_sparsity, method, device)
    law, hi, cdf = cf.draw_law(target_sparsity, hidden_size, method)
    u = torch.rand(n, dtype=torch.float64)
    if law == 0:
        return torch.clamp((u * hi).to(torch.int64), max=max(hi - 1, 0))
    return torch.clamp(torch.searchsorted(torch.from_numpy(cdf), u, right=True), max=hidden_size - 1)


def _unreachable(target_sparsity, what: str) -> RuntimeError:
    return RuntimeError(f"evol_search_deepfm: no {what} reached target_sparsity={float(target_sparsity):.6g} "
                        f"(redraws are bounded at {MAX_REDRAWS} tries)")


def _generate_candidate(emb, target_sparsity=None, d_target=None, method=1, device=None) -> Candidate:
    """deepfm_opt_embed.py:315-385: draw widths; redraw while the candidate's sparsity is below the target."""
    if d_target is None and target_sparsity is not None:
        d_target = target_sparsity
    size = emb._num_field if emb._mode_d == "field" else emb._num_item
    device = emb._weight.device if device is None else device
    with torch.no_grad():
        extra = (emb.get_submask().to(device), emb._num_item * emb._hidden_size)
    # the sparsest candidate keeps one column of every live row: a target beyond it is refused before the first draw
    if target_sparsity is not None and bool(1 - extra[0].sum() / extra[1] < target_sparsity):
        raise _unreachable(target_sparsity, "candidate (one kept column per live row is the sparsest there is)")
    for _ in range(MAX_REDRAWS):
        cand = Candidate(_draw(size, emb._hidden_size, d_target, method, device), extra)
        if target_sparsity is None or not bool(candidate_sparsity(cand) < target_sparsity):
            return cand
    raise _unreachable(target_sparsity, "drawn candidate")


def _crossover(top: List[Candidate], n_crossover: int, hidden_size, target_sparsity=None) -> List[Candidate]:
    """deepfm_opt_embed.py:413-444: every entry from one of two parents, by a fair coin."""
    out = []
    for _ in range(n_crossover):
        for _ in range(MAX_REDRAWS):
            father, mother = random.choices(top, k=2)
            pick = torch.randint(2, size=father.save_mask.shape, dtype=torch.bool, device=father.save_mask.device)
            cand = Candidate(torch.where(pick, father.save_mask, mother.save_mask), father.extra)
            if target_sparsity is None or bool(candidate_sparsity(cand) > target_sparsity):
                break
        else:
            raise _unreachable(target_sparsity, "crossover")
        out.append(cand)
    return out


def _mutate(top: List[Candidate], n_mutate: int, p_mutate: float, hidden_size: int, target_sparsity=None, d_target=None,
            method=1) -> List[Candidate]:
    """deepfm_opt_embed.py:447-489: every entry redrawn with probability p_mutate."""
    if target_sparsity is not None and d_target is None:
        d_target = target_sparsity
    out = []
    for _ in range(n_mutate):
        for _ in range(MAX_REDRAWS):
            parent = random.choice(top)
            mask = parent.save_mask
            hit = torch.rand(mask.shape[0], device=mask.device) < p_mutate
            cand = Candidate(torch.where(hit, _draw(mask.shape[0], hidden_size, d_target, method, mask.device), mask),
                             parent.extra)
            if target_sparsity is None or bool(candidate_sparsity(cand) > target_sparsity):
                break
        else:
            raise _unreachable(target_sparsity, "mutation")
        out.append(cand)
    return out


def _validate_candidate(model, candidate: Candidate, val_loader, forward=None, metric=None) -> float:
    """AUC of the model under the candidate (deepfm_opt_embed.py:388-410): set_candidate, then one validation pass."""
    from ..trainer import validate_epoch

    model.eval()
    model.embedding.set_candidate(candidate.save_mask)
    return validate_epoch(val_loader, model, device=model.embedding._weight.device, forward=forward, metric=metric)["auc"]


def evol_search_deepfm(model, n_generations: int, population: int, n_crossover: int, n_mutate: int, p_mutate: float, k: int,
                       val_dataloader, train_dataset, target_sparsity=None, method=1,
                       history: Optional[list] = None) -> Tuple[torch.Tensor, float]:
    """Evolutionary search of the per-field / per-feature widths of a DeepFM on an OptEmbed supernet
    (deepfm_opt_embed.py:501-622): `population` drawn candidates, each scored by the validation AUC; every generation
    keeps the top k of everything scored so far and adds n_crossover crossovers and n_mutate mutations of them.
    Generated candidates need sparsity >= target, children > target.  method: 0 uniform, 1 exponential, 2 linear.
    Returns (mask, best AUC); `history`, if given, receives the best AUC after each generation.

    A candidate costs set_candidate (a few bytes per field, or one byte per row) plus one validation pass through the
    masked gather_fm; ONE GraphedForward and ONE CTRMetric (its buffers allocated once) serve all candidates, their widths
    living in persistent buffers.  The model stays on its device (the reference moves it to "cuda"); the candidates are
    drawn and kept where the table is.

    Deliberate deviation: every redraw loop is bounded at MAX_REDRAWS = 10 000 tries and then raises RuntimeError
    naming the target; the reference loops forever on a target its draws cannot reach."""
    from ..trainer import CTRMetric, GraphedForward

    emb = model.embedding
    assert isinstance(emb, OptEmbed)
    hidden_size = emb._hidden_size
    with torch.no_grad():
        sub_mask = emb.get_submask()
    d_target = d_target_sparsity(target_sparsity, sub_mask, emb._num_item)
    candidates = [_generate_candidate(emb, target_sparsity, d_target, method) for _ in range(population)]
    forward = GraphedForward(model)
    val_dataset = getattr(val_dataloader, "dataset", None)
    metric = CTRMetric(emb._weight.device, capacity=len(val_dataset) if hasattr(val_dataset, "__len__") else None)
    top: List[Candidate] = []
    top_values = None
    try:
        for gen in range(n_generations):
            metrics = torch.tensor([_validate_candidate(model, c, val_dataloader, forward, metric) for c in candidates],
                                   dtype=torch.float64)
            top_values = metrics if top_values is None else torch.cat((top_values, metrics))
            top.extend(candidates)
            best = torch.topk(top_values, min(k, len(top)))
            top = [top[i] for i in best.indices.tolist()]
            top_values = best.values
            if history is not None:
                history.append(float(top_values[0]))
            if gen != n_generations - 1:
                candidates = _crossover(top, n_crossover, hidden_size, target_sparsity)
                candidates += _mutate(top, n_mutate, p_mutate, hidden_size, target_sparsity, d_target, method)
    finally:
        emb.clear_candidate()
    return top[0].save_mask, float(top_values[0])

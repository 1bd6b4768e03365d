"""IEmbedding plug-in surface + the full (vanilla) table.

Mirrors src/models/embeddings/base.py:8-75 of the reference: same class names,
constructor arguments, `get_weight()` / `get_num_params()` contract and
`state_dict` keys (`_emb_module.weight`), so reference checkpoints load and the
modules drop in under src/models/{deepfm,dcn,lightgcn}.py.  The lookup itself is
the HIP row gather of libmi355x_recsys.so, not nn.Embedding's.
"""
from abc import abstractmethod
from typing import Iterable, Optional, Union

import torch
from torch import nn

from .. import _kernels


def _hooked(module: nn.Module) -> bool:
    """Whether a forward hook or pre-hook would fire on a call of `module`: its own, or one registered for every module."""
    from torch.nn.modules import module as _m

    return bool(module._forward_hooks or module._forward_pre_hooks or _m._global_forward_hooks or _m._global_forward_pre_hooks)


def _unhooked(module: nn.Module, w1=None, bias=None) -> bool:
    """The guards of a fused lookup that never calls the embedding module: a module with a forward hook or pre-hook keeps
    forward(), so that the hooks keep firing.  With w1 / bias — a launch without an autograd node, inference only —
    nothing of y_fm may want a gradient either (fm_first_order hands the first-order table and the bias theirs)."""
    wanted = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (w1, bias))
    return not _hooked(module) and not wanted


class IEmbedding(nn.Module):
    """forward(idx[B] | idx[B,F]) -> [B,D] | [B,F,D]; get_weight() -> [N,D] (differentiable)."""

    @abstractmethod
    def get_weight(self) -> torch.Tensor:
        ...

    def get_num_params(self) -> int:
        return sum([p.numel() for p in self.parameters()])

    def fm_lookup(self, x, offsets, w1, bias, sparse_w1: bool):
        """DeepFM's lookup + FM + first-order term over this table as one launch: (emb [B, F, D], y_fm [B]) for the raw
        per-field ids x [B, F], the field offsets, the first-order table w1 and the bias (sparse_w1: w1's gradient in row
        form) — or None, the default, when the table has no such launch (or not for this call): DeepFM then calls
        forward(x + offsets) and _kernels.fm_first_order."""
        return None


def _dual_fm_lookup(self, x, offsets, w1, bias, sparse_w1: bool):
    """IEmbedding.fm_lookup of the two-table families (QR add / mult, CERP, CERP retrain): the two row gathers, their
    transform and the combine inside one launch (mi_gather_fm_dual_*), on the operands of the table's fm_dual()."""
    dual = self.fm_dual()
    if dual is None:
        return None
    return _kernels.gather_fm_dual(x, offsets, w1=w1, bias=bias, sparse_w1=sparse_w1, **dual)


class VanillaEmbedding(IEmbedding):
    """One concatenated table of sum(field_dims) rows (reference base.py:23-75).

    `_emb_module` is kept as the parameter holder (nn.Embedding / nn.EmbeddingBag,
    xavier-uniform or N(0, 0.1) initialised exactly like the reference) so that
    `state_dict()` keys, `.sparse`, `.weight` and checkpoint loading are unchanged.
    """

    _emb_module: Union[nn.Embedding, nn.EmbeddingBag]

    def __init__(
        self,
        field_dims: Union[Iterable[int], int],
        hidden_size: int,
        mode: Optional[str] = None,
        initializer="xavier",
        **kwargs,
    ):
        super().__init__()
        assert mode in [None, "sum", "mean", "max"]
        rows = field_dims if isinstance(field_dims, int) else sum(field_dims)
        self._mode = mode
        # the holder module only owns the parameter (and its `sparse` flag): lookups never call it
        self._emb_module = (nn.Embedding(rows, hidden_size, **kwargs) if mode is None
                            else nn.EmbeddingBag(rows, hidden_size, mode=mode, **kwargs))
        if initializer == "xavier":
            nn.init.xavier_uniform_(self._emb_module.weight)
        else:
            nn.init.normal_(self._emb_module.weight, std=0.1)

    @property
    def sparse_grad(self) -> bool:
        return bool(getattr(self._emb_module, "sparse", False))

    def get_weight(self):
        return self._emb_module.weight

    def forward(self, x):
        rows = _kernels.gather_rows(x, self._emb_module.weight, self.sparse_grad)
        return _kernels.bag_reduce(rows, self._mode)

    def fm_lookup(self, x, offsets, w1, bias, sparse_w1: bool):
        # the plain launch reads the stored rows: not for a subclass, whose forward() may transform them (QAT does)
        if type(self) is not VanillaEmbedding or self._mode is not None:
            return None
        return _kernels.gather_fm(x, offsets, self.get_weight(), w1, bias, sparse_W=self.sparse_grad, sparse_w1=sparse_w1)

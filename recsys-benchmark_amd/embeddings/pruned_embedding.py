"""CSR-stored pruned embedding table (inference only).

Reference: src/models/embeddings/pruned_embedding.py:11-204 — a numba `@cuda.jit` kernel
(32-thread blocks, one thread per id, serial over the row) plus a numba CPU kernel.  Here the
CSR triple lives in torch buffers and the row densify is a HIP kernel (mi_csr_rows_fwd).

compact_() (an MI355X-side storage choice, not in the reference): the columns as one byte each and the row pointers as
int32 — 5 bytes per stored element + 4 per row instead of 12 + 8.  A compact table is read by mi_csr_rows_typed_fwd, and
either width serves DeepFM through the one-launch lookup mi_gather_fm_csr_fwd (fm_csr) and DCN through the typed kernel with
the per-field offsets added inside the launch (takes_offsets).
"""
from typing import List, Optional, Union

import torch

from .. import _kernels, csr_fm
from .base import IEmbedding, _unhooked

_BUFFERS = {"values": (torch.float32,), "crow_indices": (torch.int64, torch.int32), "col_indices": (torch.int64, torch.uint8)}
COMPACT_MAX_D = 256            # a column fits one byte
COMPACT_MAX_NNZ = 2 ** 31      # a row pointer fits int32 below this


class PrunedEmbedding(IEmbedding):
    def __init__(self, field_dims: Union[int, List[int]], hidden_size: int, mode: Optional[str] = None):
        super().__init__()
        if isinstance(field_dims, int):
            field_dims = [field_dims]
        self._hidden_size = hidden_size
        self._num_item = sum(field_dims)
        self._mode = mode
        self.is_cuda = False
        self.register_buffer("values", torch.zeros(0, dtype=torch.float32))
        self.register_buffer("crow_indices", torch.zeros(self._num_item + 1, dtype=torch.int64))
        self.register_buffer("col_indices", torch.zeros(0, dtype=torch.int64))

    @classmethod
    @torch.no_grad()
    def from_other_emb(cls, emb: IEmbedding, mode=None, compact: bool = False) -> "PrunedEmbedding":
        return cls.from_weight(emb.get_weight(), mode, compact=compact)

    @classmethod
    def from_weight(cls, weight: torch.Tensor, mode=None, compact: bool = False) -> "PrunedEmbedding":
        num_item, hidden_size = weight.shape
        result = cls(num_item, hidden_size, mode)
        weight = weight.detach()
        if weight.layout != torch.sparse_csr:
            weight = weight.to_sparse_csr()
        result.values = weight.values().to(torch.float32).contiguous()
        result.crow_indices = weight.crow_indices().to(torch.int64).contiguous()
        result.col_indices = weight.col_indices().to(torch.int64).contiguous()
        result.is_cuda = result.values.is_cuda
        return result.compact_() if compact else result

    @classmethod
    @torch.no_grad()
    def from_pruned(cls, source: Union[torch.Tensor, IEmbedding], p: float, min_item: int = 0,
                    mode=None, compact: bool = False) -> "PrunedEmbedding":
        """The table (a tensor, or an IEmbedding's get_weight()) magnitude-pruned by (p, min_item) — src/utils.py:8-34 —
        and stored as CSR, the triple written by the fused build of csrc/mag_prune.hip: equal, array for array, to
        from_weight(pruning.prune_table(weight.clone(), p, min_item)), without the dense pruned table."""
        from ..pruning import _pruned_csr

        weight = source.get_weight() if isinstance(source, IEmbedding) else source
        crow, col, values = _pruned_csr(weight, p, min_item)
        result = cls(weight.shape[0], weight.shape[1], mode)
        result.values, result.crow_indices, result.col_indices = values, crow, col
        result.is_cuda = values.is_cuda
        return result.compact_() if compact else result

    @property
    def is_compact(self) -> bool:
        return self.col_indices.dtype == torch.uint8 and self.crow_indices.dtype == torch.int32

    @torch.no_grad()
    def compact_(self) -> "PrunedEmbedding":
        """Narrow the index buffers in place: col_indices to uint8 (D <= 256), crow_indices to int32 (nnz < 2^31).  The
        triple is validated first, on the buffers' device with one host read — crow non-decreasing from 0 to nnz, every
        column inside [0, D); ValueError otherwise, the buffers untouched.  Buffer names and state_dict keys stay."""
        N, D, nnz = self._num_item, self._hidden_size, self.values.numel()
        crow, col = self.crow_indices, self.col_indices
        if D > COMPACT_MAX_D:
            raise ValueError(f"one-byte columns need hidden_size <= {COMPACT_MAX_D}, got {D}")
        if nnz >= COMPACT_MAX_NNZ:
            raise ValueError(f"int32 row pointers need fewer than 2^31 stored elements, got {nnz}")
        if crow.numel() != N + 1 or col.numel() != nnz:
            raise ValueError(f"the triple does not describe a [{N}, {D}] table with {nnz} stored elements")
        c64 = crow.to(torch.int64)
        code = ((c64[0] != 0).to(torch.int64) | ((c64[N] != nnz).to(torch.int64) << 1)
                | ((c64[1:] < c64[:-1]).any().to(torch.int64) << 2))
        if nnz:
            k64 = col.to(torch.int64)
            code = code | (((k64 < 0) | (k64 >= D)).any().to(torch.int64) << 3)
        code = int(code.item())          # the one host read
        if code:
            what = [msg for bit, msg in enumerate(("crow_indices[0] != 0", "crow_indices[N] != nnz",
                                                   "crow_indices decreases", "a column outside [0, hidden_size)"))
                    if code >> bit & 1]
            raise ValueError("compact_(): not a valid CSR triple: " + ", ".join(what))
        self.col_indices = col.to(torch.uint8)
        self.crow_indices = crow.to(torch.int32)
        return self

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # the triple's sizes (and, for a compact table, its index types) belong to the saved table, not to the constructor:
        # the buffers are re-assigned with the saved dtypes and sizes, then filled by the usual copy
        for name, dtypes in _BUFFERS.items():
            saved = state_dict.get(prefix + name)
            if torch.is_tensor(saved):
                if saved.dtype not in dtypes or saved.dim() != 1:
                    error_msgs.append(f"{prefix + name}: expected a 1-D tensor of {' or '.join(map(str, dtypes))}, got "
                                      f"{saved.dtype} {tuple(saved.shape)}")
                    continue
                setattr(self, name, torch.zeros(saved.shape, dtype=saved.dtype, device=getattr(self, name).device))
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def to_cuda(self):
        """Move the CSR triple to the GPU (reference API, pruned_embedding.py:51-65)."""
        self.to("cuda")
        self.is_cuda = True

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self.is_cuda = self.crow_indices.is_cuda
        return out

    def get_num_params(self) -> int:
        """The number of stored elements (the triple is buffers: the base class would count 0)."""
        return int(self.values.numel())

    def get_weight(self):
        sparse_csr = torch.sparse_csr_tensor(
            self.crow_indices.to(torch.int64), self.col_indices.to(torch.int64), self.values,
            size=(self._num_item, self._hidden_size), dtype=torch.float32,
        )
        return sparse_csr.to_dense()

    def takes_offsets(self, x: torch.Tensor) -> bool:
        """Whether forward(x, offsets=...) adds the per-field offsets inside the lookup kernel ([B, F] ids on the table's
        GPU, no bag mode) — the protocol of dcn._FieldModel._lookup."""
        return bool(self._mode is None and x.is_cuda and x.dim() == 2 and x.device == self.crow_indices.device)

    def forward(self, x, offsets: Optional[torch.Tensor] = None):
        """offsets (optional extension, [F]): x then holds the model's raw per-field ids [B, F]; returns (embeddings, row
        ids), the addition inside the typed kernel where takes_offsets(x) holds."""
        if offsets is not None:
            if not self.takes_offsets(x):
                rows = x + offsets
                return self.forward(rows), rows
            return csr_fm.csr_rows_typed(self.values, self.crow_indices, self.col_indices, x, self._hidden_size,
                                         self._num_item, offsets=offsets)
        if self.is_compact:
            out = csr_fm.csr_rows_typed(self.values, self.crow_indices, self.col_indices, x, self._hidden_size,
                                        self._num_item)
        else:
            out = _kernels.csr_rows(self.values, self.crow_indices, self.col_indices, x,
                                    self._hidden_size, self._num_item)
        return _kernels.bag_reduce(out, self._mode)

    def fm_csr(self, x: torch.Tensor):
        """The operands of DeepFM's fused lookup + FM launch (csr_fm.gather_fm_csr), or None when this table keeps the
        separate lookup: a CPU table, a bag mode, or an x that is not [B, F] on the table's device."""
        if self._mode is not None or not self.crow_indices.is_cuda or not torch.is_tensor(x):
            return None
        if x.dim() != 2 or x.device != self.crow_indices.device:
            return None
        return dict(values=self.values, crow=self.crow_indices, col=self.col_indices, D=self._hidden_size, N=self._num_item)

    def fm_lookup(self, x, offsets, w1, bias, sparse_w1: bool):
        """The row densify inside DeepFM's lookup launch (mi_gather_fm_csr_fwd), for wide and compact index buffers alike:
        inference only, no autograd node."""
        csr = self.fm_csr(x) if _unhooked(self, w1, bias) else None
        if csr is None:
            return None
        return csr_fm.gather_fm_csr(x, offsets, w1=w1, bias=bias, **csr)

"""OptEmbed supernet for the CF models (LightGCN, SingleLightGCN, NeuMF) — reference:
src/models/embeddings/lightgcn_opt_embed.py:26-625 and src/models/embeddings/optembed_utils.py:10-202.

`OptEmbed` has the reference's constructor, parameters (`_weight`, `_mask_e_module._t_param`), buffers
(`_mask_e_module._field_dims`, `_full_mask_d`), state_dict keys in the same order, `get_weight(mask_d)`, `forward(x,
mask_d)`, `get_l_s`, `get_sparsity`, `get_num_params` and the eval cache `_cur_weight` (made by the first eval forward,
cleared by a backward through the module; an assigned `_cur_weight` is what eval lookups and `get_weight()` read).
The masked table — row norm, BinaryStep row mask, prefix dimension mask and, in training, the width draw — is ONE HIP
launch (_kernels.optembed_cf); its backward is at most two launches with no atomics, bit-identical from run to run.
The training draw of `mode_threshold_d="feature"` with a `target_sparsity` (the reference's host WeightedRandomSampler)
is made on the device from the same law (`draw_law`).

`RetrainOptEmbed` is the reference's retraining table: `init_mask(mask_e, mask_d)` then `_weight * _mask`.
`evol_search_lightgcn` is the reference's evolutionary mask search, with the candidates kept and drawn on the device.
"""
import itertools
import random
from collections import namedtuple
from functools import lru_cache, partial
from typing import List, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from .. import _kernels
from .base import IEmbedding
from .deepfm_opt_embed import _MaskEmbeddingModule, get_mask

_salts = itertools.count(1)          # one generator stream per table (salt 0: the search's draws)


# ---- the width laws of _sampling_by_weight (optembed_utils.py:103-202) -----------------------------------------------
def get_expected_hidden_size(alpha, max_hidden_size: int):
    """E[k + 1] when P(k + 1 = i) is proportional to alpha^(h - i), i = 1..h (optembed_utils.py:153-163)."""
    if alpha == 1:
        return (max_hidden_size + 1) / 2
    return alpha / (alpha - 1) - max_hidden_size / (alpha ** max_hidden_size - 1)


@lru_cache(16)
def find_alpha(target_sparsity: float, hidden_size: int, step: float = 0.1, eps: float = 1e-6,
               num_step: int = 100000) -> float:
    """alpha whose expected width gives `target_sparsity` (optembed_utils.py:103-150): the reference's three fixed
    answers, else its float32 gradient descent on (expected sparsity - target)^2 from 1.1 (target > 0.5) or 0.9, stopped
    once the expected sparsity is above the target by less than eps."""
    if hidden_size == 64 and target_sparsity in (0.7, 0.8):
        return 1.045 if target_sparsity == 0.7 else 1.083
    if target_sparsity == 0.5:
        return 1
    alpha = torch.tensor(1.1 if target_sparsity > 0.5 else 0.9, requires_grad=True)
    for _ in range(num_step):
        diff = 1 - get_expected_hidden_size(alpha, hidden_size) / hidden_size - target_sparsity
        if diff > 0 and abs(diff) < eps:
            return alpha.item()
        alpha.grad = None
        (diff ** 2).backward()
        alpha.data -= step * alpha.grad
    return alpha.item()


def width_probabilities(alpha, hidden_size: int) -> np.ndarray:
    """P(k = j) proportional to alpha^(D - 1 - j), float64 (optembed_utils.py:166-169)."""
    f = np.power(alpha, hidden_size - 1 - np.arange(hidden_size, dtype=np.float64))
    return f / f.sum()


def linear_hidden(target_sparsity: float, hidden_size: int) -> int:
    """Upper end of the "linear" law (optembed_utils.py:172-178)."""
    assert target_sparsity >= 0.5, "Generate naive only could generate sparsity from 0.5"
    return int(hidden_size * 2 * (1 - target_sparsity))


def draw_law(target_sparsity: Optional[float], hidden_size: int, method: int = 1):
    """(law, hi, cdf) of the kernel's draw for _sampling_by_weight(target_sparsity, hidden_size, ., method): law 0 is
    uniform on [0, hi); law 1 draws through `cdf` (float64 numpy [D], last entry exactly 1)."""
    if target_sparsity is None or method == 0:
        return 0, hidden_size, None
    if method == 2:
        return 0, linear_hidden(target_sparsity, hidden_size), None
    cdf = np.cumsum(width_probabilities(find_alpha(target_sparsity, hidden_size), hidden_size))
    cdf[-1] = 1.0
    return 1, hidden_size, cdf


def _is_int(t) -> bool:
    return isinstance(t, torch.Tensor) and not t.is_floating_point() and t.dtype != torch.bool


def _delete_cache(module, grad_input, grad_output):
    module._cur_weight = None


class IOptEmbed(IEmbedding):
    def get_l_s(self) -> torch.Tensor:
        return torch.tensor(0)


class OptEmbed(IOptEmbed):
    """OptEmbed of lightgcn_opt_embed.py:26-216 (see the module docstring).

    get_weight(mask_d):
      - training, mask_d None: widths drawn on the device — one per field, uniform, when mode_threshold_d="field"; one
        per row from _sampling_by_weight's law (target_sparsity, exponential method) when "feature";
      - training, integer mask_d: last kept dimension per row;
      - eval, integer mask_d: per field when mode_threshold_d="field", per row otherwise;
      - a bool / float [N, D] mask_d: multiplied in as it is;
      - eval, mask_d None: the row mask only (or the assigned / cached `_cur_weight`).
    Integer masks are taken on any device (the reference's `isinstance(mask_d, torch.LongTensor)` holds for CPU tensors
    only).  A training-mode get_weight drops `_cur_weight`, so an eval cache never outlives a training step."""

    def __init__(self, field_dims: Union[List[int], int], hidden_size: int, mode: Optional[str] = None,
                 t_init: Optional[float] = 0, mode_threshold_e="field", mode_threshold_d="field", norm=1,
                 target_sparsity: Optional[float] = None):
        super().__init__()
        if isinstance(field_dims, int):
            field_dims = [field_dims]
        assert mode in ["sum", "mean", "max", None]
        assert mode_threshold_e in ["field", "feature"]
        assert mode_threshold_d in ["field", "feature"]
        assert norm in (1, 2), "the kernel takes the L1 and L2 row norms"
        self._field_dims = torch.tensor(field_dims, dtype=torch.int64)
        self._num_item = int(self._field_dims.sum())
        self._num_field = len(field_dims)
        self._hidden_size = hidden_size
        self._weight = nn.Parameter(torch.empty((self._num_item, hidden_size)))
        self._cur_weight = None
        nn.init.xavier_uniform_(self._weight)
        self._handle = self.register_full_backward_hook(_delete_cache)
        self._mode = mode
        self._t_init = t_init
        self._norm = norm
        self._mask_e_module = (nn.Identity() if t_init is None
                               else _MaskEmbeddingModule(self._field_dims, t_init, mode_threshold_e, norm))
        self.register_buffer("_full_mask_d", get_mask(hidden_size))
        self._target_sparsity = target_sparsity
        self._method = 1
        self._mode_d = mode_threshold_d
        off = torch.zeros(self._num_field + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(self._field_dims, 0)
        self.register_buffer("_field_off", off, persistent=False)
        law, hi, cdf = draw_law(target_sparsity if mode_threshold_d == "feature" else None, hidden_size, self._method)
        self._law = (law, hi)
        self.register_buffer("_draw_cdf", None if cdf is None else torch.from_numpy(cdf), persistent=False)
        self._salt = next(_salts)

    # ---- the kernel call -------------------------------------------------------------------------------------------
    def _masked(self, k=None, k_field=False, draw=False):
        t, t_field = None, False
        if self._t_init is not None:
            t = self._mask_e_module._t_param
            t_field = self._mask_e_module.mode_threshold_e == "field"
        spec = None
        if draw:
            spec = (self._law[0], self._law[1], self._draw_cdf, self._salt)
            k_field = self._mode_d == "field"
        out, _ = _kernels.optembed_cf(self._weight, t, t_field, self._field_off, self._norm, k=k, k_field=k_field, draw=spec)
        return out

    def _check_widths(self, k, per_field: bool):
        n = self._num_field if per_field else self._num_item
        if k.dim() != 1 or k.numel() != n:
            raise ValueError(f"an integer mask_d holds one width per {'field' if per_field else 'row'} ({n}), "
                             f"got shape {tuple(k.shape)}")
        return k.to(self._weight.device)

    # ---- reference API ---------------------------------------------------------------------------------------------
    def get_l_s(self) -> torch.Tensor:
        if self._t_init is None:
            return torch.tensor(0)
        return torch.exp(-self._mask_e_module._t_param).sum()

    def get_weight(self, mask_d: Optional[torch.Tensor] = None):
        if self.training:
            self._cur_weight = None
            if mask_d is None:
                return self._masked(draw=True)
            if _is_int(mask_d):
                return self._masked(k=self._check_widths(mask_d, False))
            return self._masked() * mask_d.to(self._weight)
        if mask_d is None:
            return self._cur_weight if self._cur_weight is not None else self._masked()
        if _is_int(mask_d):
            per_field = self._mode_d == "field"
            return self._masked(k=self._check_widths(mask_d, per_field), k_field=per_field)
        return self._masked() * mask_d.to(self._weight)

    def forward(self, x, mask_d=None):
        """x: row ids; mask_d as for get_weight.  Eval lookups read (and the first one makes) `_cur_weight`."""
        if not self.training:
            if self._cur_weight is None:
                self._cur_weight = self.get_weight(mask_d)
            weight = self._cur_weight
        else:
            weight = self.get_weight(mask_d)
        return _kernels.bag_reduce(_kernels.gather_rows(x, weight), self._mode)

    def get_sparsity(self, get_n_params=False):
        with torch.no_grad():
            nnz = int(torch.count_nonzero(self._masked()).item())
        sparsity = 1 - nnz / (self._num_item * self._hidden_size)
        return (sparsity, nnz) if get_n_params else sparsity

    def get_num_params(self):
        return self.get_sparsity(True)[1]


class RetrainOptEmbed(IOptEmbed):
    """RetrainOptEmbed of lightgcn_opt_embed.py:524-625: the searched masks as a fixed [N, D] non-trainable parameter
    `_mask`, weight = `_weight * _mask` (one elementwise product).  Its cache behaves as the reference's: get_weight
    stores the product in `_cur_weight`, eval get_weight and every forward read it while it is set, a backward through
    the module drops it."""

    def __init__(self, field_dims: Union[List[int], int], hidden_size, mode: Optional[str] = None,
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
        self._mode = mode
        self._weight = nn.Parameter(torch.empty((self._num_item, hidden_size)))
        self._cur_weight: Optional[torch.Tensor] = None
        nn.init.xavier_uniform_(self._weight)
        self._t_init = t_init
        self.register_buffer("_full_mask_d", get_mask(hidden_size))
        self._target_sparsity = target_sparsity
        self._mode_d = mode_threshold_d
        self._mask_d = None
        self._mask_e = None
        self._mask = nn.Parameter(torch.empty(self._num_item, hidden_size), requires_grad=False)
        self._sparsity = 0

    def init_mask(self, mask_e, mask_d):
        """_mask = [j <= mask_d(row)] * mask_e(row); mask_d per field (mode_threshold_d="field") or per row, mask_e per
        row or None (all rows kept)."""
        dev = self._weight.device
        mask_e = torch.ones(self._num_item, device=dev) if mask_e is None else mask_e.to(dev)
        mask_d = mask_d.to(dev)
        if self._mode_d == "field":
            mask_d = torch.repeat_interleave(mask_d, self._field_dims.to(dev), dim=0, output_size=self._num_item)
        mask = self._full_mask_d[mask_d] * mask_e.unsqueeze(-1)
        self._mask = nn.Parameter(mask, False)
        self._cur_weight = None
        self._handle = self.register_full_backward_hook(_delete_cache)
        return self._mask

    def get_weight(self) -> torch.Tensor:
        if self._cur_weight is not None and not self.training:
            return self._cur_weight
        self._cur_weight = self._weight * self._mask
        return self._cur_weight

    def forward(self, x, mask_d=None):
        if self._cur_weight is None:
            self.get_weight()
        return _kernels.bag_reduce(_kernels.gather_rows(x, self._cur_weight), self._mode)

    def get_sparsity(self, get_n_params=False):
        nnz = int(torch.count_nonzero(self._mask).item())
        sparsity = 1 - nnz / (self._hidden_size * self._num_item)
        return (sparsity, nnz) if get_n_params else sparsity

    def get_num_params(self):
        return int(torch.count_nonzero(self._mask).item())


# ---- evolutionary mask search (lightgcn_opt_embed.py:220-516) ---------------------------------------------------------
Candidate = namedtuple("Candidate", ["item_mask", "user_mask"])


def candidate_sparsity(candidate: Candidate, hidden_size: int) -> float:
    """1 - kept elements / (rows * D) of a candidate's two width vectors (lightgcn_opt_embed.py:411-421)."""
    kept = (candidate.user_mask + 1).sum() + (candidate.item_mask + 1).sum()
    rows = len(candidate.item_mask) + len(candidate.user_mask)
    return float(1 - kept / (rows * hidden_size))


def draw_widths(n: int, hidden_size: int, target_sparsity, method: int, device) -> torch.Tensor:
    """_sampling_by_weight(target_sparsity, hidden_size, n, method) on the device (draw-only kernel launch)."""
    law, hi, cdf = draw_law(target_sparsity, hidden_size, method)
    cdf_t = None if cdf is None else torch.from_numpy(cdf).to(device)
    return _kernels.optembed_cf_draw(n, hidden_size, law, hi, cdf_t, 0, device)


def _generate(num_user, num_item, hidden_size, target_sparsity, method, device) -> Candidate:
    """lightgcn_opt_embed.py:222-259: draw; while below the target, redraw with the target raised by 5%."""
    def draw(ts):
        return Candidate(item_mask=draw_widths(num_item, hidden_size, ts, method, device),
                         user_mask=draw_widths(num_user, hidden_size, ts, method, device))

    cand = draw(target_sparsity)
    while target_sparsity is not None and candidate_sparsity(cand, hidden_size) < target_sparsity:
        cand = draw(target_sparsity * 1.05)
    return cand


def _crossover(top: List[Candidate], n_crossover, hidden_size, target_sparsity) -> List[Candidate]:
    """lightgcn_opt_embed.py:289-339: each row's width from one of two parents, chosen by a fair coin."""
    out = []
    for _ in range(n_crossover):
        while True:
            father, mother = random.choices(top, k=2)
            kids = []
            for a, b in ((father.item_mask, mother.item_mask), (father.user_mask, mother.user_mask)):
                pick = torch.randint(2, size=a.shape, dtype=torch.bool, device=a.device)
                kids.append(torch.where(pick, a, b))
            cand = Candidate(item_mask=kids[0], user_mask=kids[1])
            if target_sparsity is None or candidate_sparsity(cand, hidden_size) > target_sparsity:
                break
        out.append(cand)
    return out


def _mutate(top: List[Candidate], n_mutate, p_mutate, hidden_size, target_sparsity, method) -> List[Candidate]:
    """lightgcn_opt_embed.py:342-408: each row redrawn with probability p_mutate."""
    out = []
    for _ in range(n_mutate):
        while True:
            parent = random.choice(top)
            kids = []
            for a in (parent.item_mask, parent.user_mask):
                hit = torch.rand(a.shape, device=a.device) < p_mutate
                kids.append(torch.where(hit, draw_widths(a.numel(), hidden_size, target_sparsity, method, a.device), a))
            cand = Candidate(item_mask=kids[0], user_mask=kids[1])
            if target_sparsity is None or candidate_sparsity(cand, hidden_size) > target_sparsity:
                break
        out.append(cand)
    return out


def _validate_candidate(model, candidate: Candidate, val_loader, train_dataset) -> float:
    """NDCG of the model with the candidate's widths hooked into the two tables' get_weight (lightgcn_opt_embed.py:262-286)."""
    from ..trainer import validate_epoch_cf

    items, users = model.item_emb_table, model.user_emb_table
    items.get_weight = partial(type(items).get_weight, items, mask_d=candidate.item_mask)
    users.get_weight = partial(type(users).get_weight, users, mask_d=candidate.user_mask)
    try:
        return validate_epoch_cf(train_dataset, val_loader, model)["ndcg"]
    finally:
        del items.get_weight, users.get_weight


def evol_search_lightgcn(model, n_generations: int, population: int, n_crossover: int, n_mutate: int, p_mutate: float,
                         k: int, val_dataloader, train_dataset, target_sparsity=None, method=1,
                         history: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Evolutionary search of per-row widths for a LightGCN on OptEmbed tables (lightgcn_opt_embed.py:424-516): a
    population of drawn candidates, each scored by validate_epoch_cf; every generation keeps the top k of everything
    scored so far and adds n_crossover crossovers and n_mutate mutations of them.  method: 0 uniform, 1 exponential,
    2 linear.  Returns (item widths, user widths, best NDCG); the widths stay on the model's device.  `history`, if
    given, receives the best NDCG after each generation."""
    items, users = model.item_emb_table, model.user_emb_table
    assert isinstance(items, IOptEmbed) and isinstance(users, IOptEmbed)
    hidden_size = items._hidden_size
    num_items, num_users = train_dataset.num_items, train_dataset.num_users
    device = items._weight.device
    candidates = [_generate(num_users, num_items, hidden_size, target_sparsity, method, device) for _ in range(population)]
    top: List[Candidate] = []
    top_values = None
    for gen in range(n_generations):
        metrics = torch.tensor([_validate_candidate(model, c, val_dataloader, train_dataset) for c in candidates])
        top_values = metrics if top_values is None else torch.cat((top_values, metrics))
        top.extend(candidates)
        best = torch.topk(top_values, min(k, len(top)))
        top = [top[i] for i in best.indices.tolist()]
        top_values = best.values
        if history is not None:
            history.append(float(top_values[0]))
        if gen != n_generations - 1:
            candidates = _crossover(top, n_crossover, hidden_size, target_sparsity)
            candidates += _mutate(top, n_mutate, p_mutate, hidden_size, target_sparsity, method)
    return top[0].item_mask, top[0].user_mask, top_values[0]

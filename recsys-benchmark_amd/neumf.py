"""NeuMF (GMF + MLP) on the library's kernels: fused lookup, training, all-items scoring.

Drop-in for src/models/mlp.py:11-344: same constructor, parameter creation order, state_dict keys (and their order),
`ModelFlag` / `flag`, `update_weight`, `get_reg_loss`, `get_embs`, `get_prune_loss_tanh`, `clear_cache`,
`get_sparsity_and_param`; 1-D ([S] -> [S]) and 2-D ([B, K] -> [B, K]) inputs.

Hot path (csrc/neumf.hip):
  - plain tables: the four row gathers, the GMF term and the tower's input row [mu ; mi] are one launch
    (mi_neumf_fwd); the tower is mlp.run_tail with y = y_mlp + y_gmf formed in its last kernel; the backward is
    mi_neumf_bwd (dense table gradients by float atomics, row form for sparse=True tables, and under
    use_deterministic_algorithms(True) row form joined in a fixed order by _kernels.coalesce_dense);
  - any other table (QR, CERP, PEP, ...): the table's own forward, then the same two kernels on the looked-up rows;
  - `score_all_items`: the model over every item for a batch of users, mi_neumf_score_all (fp32 MFMA); towers the
    kernel does not take (mi_neumf_score_supported) run through mi_neumf_fwd + mlp.run_tail on chunks of pairs.
"""
from enum import IntEnum
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _kernels, _lib
from .embeddings import IEmbedding, VanillaEmbedding, get_embedding


class ModelFlag(IntEnum):
    MLP = 1
    GMF = 2
    NMF = 3


def _plain(table) -> bool:
    return type(table) is VanillaEmbedding and table._mode is None


class _NeuMFFn(torch.autograd.Function):
    """(y_gmf [S], X0 [S, 2D]) = mi_neumf_fwd over four [n, D] tables.  `grad_form`: "dense" (float atomics, or the
    fixed-order row join under use_deterministic_algorithms), "sparse" (row-form COO gradients, the tables' sparse=True)
    or "rows" (the tables ARE the looked-up rows, ids = arange(S): their gradient is the row form itself)."""

    @staticmethod
    def forward(ctx, users, items, GU, GI, MU, MI, w, b, flags: int, grad_form: str):
        # the halves a flag leaves out may be None (GMF: GU, GI, w, b; MLP: MU, MI)
        dev = _lib.require_gpu(users, items, GU, GI, MU, MI, w, b)
        users, items = _kernels._i64c(users).view(-1), _kernels._i64c(items).view(-1)
        GU, GI, MU, MI, w, b = (None if t is None else _kernels._f32c(t) for t in (GU, GI, MU, MI, w, b))
        S = users.numel()
        D = (GU if GU is not None else MU).shape[1]
        gmf, mlp = bool(flags & 2), bool(flags & 1)
        y = torch.empty(S if gmf else 0, dtype=torch.float32, device=dev)
        X0 = torch.empty((S if mlp else 0, 2 * D), dtype=torch.float32, device=dev)
        n = lambda t: 0 if t is None else t.shape[0]
        _lib.check(_lib.load().mi_neumf_fwd(users.data_ptr(), items.data_ptr(), S, _lib.ptr(GU), _lib.ptr(GI), _lib.ptr(MU),
                                            _lib.ptr(MI), D, n(GU) if gmf else n(MU), n(GI) if gmf else n(MI), _lib.ptr(w),
                                            _lib.ptr(b), flags, _lib.ptr(y) if gmf else None, _lib.ptr(X0) if mlp else None,
                                            _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)), "mi_neumf_fwd")
        if gmf and mlp and (n(GU), n(GI)) != (n(MU), n(MI)):
            raise ValueError("the GMF and MLP tables must have the same row counts")
        ctx.save_for_backward(users, items, GU, GI, w)
        ctx.meta = (flags, grad_form, S, D, (n(GU), n(GI), n(MU), n(MI)), None if w is None else w.shape)
        return y, X0

    @staticmethod
    def backward(ctx, dy, dX0):
        users, items, GU, GI, w = ctx.saved_tensors
        flags, form, S, D, shapes, wshape = ctx.meta
        dev = users.device
        gmf, mlp = bool(flags & 2), bool(flags & 1)
        rows_out = form != "dense" or _kernels.DETERMINISTIC
        on = (gmf, gmf, mlp, mlp)
        if rows_out:
            outs = [torch.empty((S, D), dtype=torch.float32, device=dev) if o else None for o in on]
        else:
            outs = [torch.zeros((nr, D), dtype=torch.float32, device=dev) if o else None for nr, o in zip(shapes, on)]
        dw = torch.empty(D, dtype=torch.float32, device=dev) if gmf else None
        db = torch.empty(1, dtype=torch.float32, device=dev) if gmf else None
        lib = _lib.load()
        ws = torch.empty(lib.mi_neumf_bwd_parts(S, D) * (D + 1), dtype=torch.float32, device=dev) if gmf else None
        dy = _kernels._f32c(dy) if gmf else None
        dX0 = _kernels._f32c(dX0) if mlp else None
        nU, nI = (shapes[0], shapes[1]) if gmf else (shapes[2], shapes[3])
        _lib.check(lib.mi_neumf_bwd(users.data_ptr(), items.data_ptr(), S, _lib.ptr(GU), _lib.ptr(GI), D, nU, nI,
                                    _lib.ptr(w), flags, _lib.ptr(dy), _lib.ptr(dX0), int(rows_out),
                                    *(_lib.ptr(t) for t in outs), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws),
                                    _lib.stream_ptr(dev)), "mi_neumf_bwd")
        grads = []
        for t, ids, nr in zip(outs, (users, items, users, items), shapes):
            if t is None or form == "rows":
                grads.append(t)
            elif form == "sparse":
                grads.append(_kernels._coo(ids, t, (nr, D)))
            elif rows_out:                       # deterministic dense: the row form joined in a fixed order
                grads.append(_kernels.coalesce_dense(ids, t, nr, D))
            else:
                grads.append(t)
        return (None, None, *grads, dw.view(wshape) if gmf else None, db if gmf else None, None, None)


class _GMF(nn.Module):
    """GMF part of NeuMF (src/models/mlp.py:281-344)."""

    def __init__(self, num_user: int, num_item: int, num_factors: int, embedding_config: Dict[str, Any],
                 cache_inference: bool = False):
        super().__init__()
        self.embedding_config = embedding_config
        self._init_embedding(num_user, num_item, num_factors)
        self.gmf_fc = nn.Linear(num_factors, 1)
        self._cache_inference = cache_inference
        self._user_emb = None
        self._item_emb = None

    def _init_embedding(self, num_user, num_item, hidden_size):
        self.user_emb_table = get_embedding(self.embedding_config, num_user, hidden_size, field_name="gmf-user")
        self.item_emb_table = get_embedding(self.embedding_config, num_item, hidden_size, field_name="gmf-item")

    def forward(self, users, items):
        u, i = _rows(self, users, items)
        ids = _arange(u)
        y, _ = _NeuMFFn.apply(ids, ids, u, i, None, None, self.gmf_fc.weight, self.gmf_fc.bias, int(ModelFlag.GMF), "rows")
        return y.view(users.shape)


class _MLP(nn.Module):
    """MLP part of NeuMF (src/models/mlp.py:188-278)."""

    def __init__(self, num_user, num_item, num_factors: int, hidden_sizes: List[int], p_dropout: float,
                 embedding_config: Dict[str, Any], cache_inference=False):
        super().__init__()
        self.embedding_config = embedding_config
        self._init_embedding(num_user, num_item, num_factors)
        layers = []
        inp_size = num_factors * 2
        for size in hidden_sizes:
            layers.append(nn.Linear(inp_size, size))
            layers.append(nn.ReLU())
            layers.append(nn.Dropout(p_dropout))
            inp_size = size
        self.mlp_fc = nn.Linear(inp_size, 1)          # registered before `mlp`, as in the reference (state_dict order)
        self.mlp = nn.Sequential(*layers)
        self._init_weight()
        self._cache_inference = cache_inference
        self._user_emb = None
        self._item_emb = None

    def _init_embedding(self, num_user, num_item, hidden_size):
        self.user_emb_table = get_embedding(self.embedding_config, num_user, hidden_size, field_name="mlp-user")
        self.item_emb_table = get_embedding(self.embedding_config, num_item, hidden_size, field_name="mlp-item")

    def _init_weight(self):
        for layer in self.mlp:
            if isinstance(layer, nn.Linear):
                nn.init.xavier_uniform_(layer.weight)

    def tower(self) -> nn.Sequential:
        """The hidden stack and mlp_fc as one Sequential of the REGISTERED modules, built per call (so .eval() / .train()
        and parameter updates always reach it)."""
        return nn.Sequential(*self.mlp, self.mlp_fc).train(self.training)

    def forward(self, users, items):
        from .mlp import run_tail

        u, i = _rows(self, users, items)
        ids = _arange(u)
        _, X0 = _NeuMFFn.apply(ids, ids, None, None, u, i, None, None, int(ModelFlag.MLP), "rows")
        return run_tail(self.tower(), X0).view(users.shape)


def _arange(rows: torch.Tensor) -> torch.Tensor:
    return torch.arange(rows.shape[0], dtype=torch.int64, device=rows.device)


def _rows(part, users, items) -> Tuple[torch.Tensor, torch.Tensor]:
    """The looked-up rows [S, D] of a part's two tables through the tables' own forwards (or the cached full tables)."""
    if part._cache_inference and not part.training:
        if part._user_emb is None:
            part._user_emb = part.user_emb_table.get_weight()
            part._item_emb = part.item_emb_table.get_weight()
        u, i = _kernels.gather_rows(users, part._user_emb), _kernels.gather_rows(items, part._item_emb)
    else:
        u, i = part.user_emb_table(users), part.item_emb_table(items)
    return u.reshape(-1, u.shape[-1]), i.reshape(-1, i.shape[-1])


class NeuMF(nn.Module):
    """NeuMF (src/models/mlp.py:17-180).  GMF and MLP share emb_size; each table is emb_size // 2 wide."""

    def __init__(self, num_user, num_item, emb_size: int = 64, hidden_sizes: Optional[List[int]] = None, p_dropout=0,
                 embedding_config=None, cache_inference=False):
        super().__init__()
        if embedding_config is None:
            embedding_config = {"name": "vanilla"}
        assert emb_size % 2 == 0
        self.flag = ModelFlag.NMF
        self._num_user = num_user
        self._num_item = num_item
        self._emb_size = emb_size
        self._gmf = _GMF(num_user, num_item, emb_size // 2, embedding_config, cache_inference)
        self._mlp = _MLP(num_user, num_item, emb_size // 2, hidden_sizes, p_dropout, embedding_config, cache_inference)

    def update_weight(self, alpha):
        self._gmf.gmf_fc.weight.data *= 1 - alpha
        self._gmf.gmf_fc.bias.data *= 1 - alpha
        self._mlp.mlp_fc.weight.data *= alpha
        self._mlp.mlp_fc.bias.data *= alpha

    def mlp_flag(self):
        return self.flag & ModelFlag.MLP

    def gmf_flag(self):
        return self.flag & ModelFlag.GMF

    def _tables(self):
        return (self._gmf.user_emb_table, self._gmf.item_emb_table, self._mlp.user_emb_table, self._mlp.item_emb_table)

    def _plain_tables(self) -> bool:
        """All four tables plain VanillaEmbedding lookups (no bag mode): the one-launch path."""
        return all(_plain(t) for t in self._tables())

    def forward(self, users, items):
        """users, items: int64 [S] or [B, K] -> scores of the same shape."""
        from .mlp import run_tail

        flags = int(self.flag) & 3
        if flags == 0:
            return torch.zeros(users.shape, dtype=torch.float32, device=users.device)
        _lib.require_gpu(users, items)
        gmf, mlp = self._gmf, self._mlp
        cached = (gmf._cache_inference or mlp._cache_inference) and not self.training
        if self._plain_tables() and not cached:
            tables = [t.get_weight() for t in self._tables()]
            sparse = all(t.sparse_grad for t in self._tables())
            form = "sparse" if sparse else "dense"
            if any(t.sparse_grad for t in self._tables()) and not sparse:
                form = "dense_mixed"
            if form == "dense_mixed":                      # tables that disagree on sparse=: each its own form
                return self._composed(users, items, flags)
            if not flags & 2:
                tables[0] = tables[1] = None
            if not flags & 1:
                tables[2] = tables[3] = None
            w, b = (gmf.gmf_fc.weight, gmf.gmf_fc.bias) if flags & 2 else (None, None)
            y_gmf, X0 = _NeuMFFn.apply(users.reshape(-1), items.reshape(-1), *tables, w, b, flags, form)
        else:
            return self._composed(users, items, flags)
        if not flags & 1:
            return y_gmf.view(users.shape)
        return run_tail(mlp.tower(), X0, last_add=y_gmf if flags & 2 else None).view(users.shape)

    def _composed(self, users, items, flags):
        """Compressed / special tables: the tables' own forwards, then the GMF and concat kernel on the looked-up rows."""
        from .mlp import run_tail

        gmf, mlp = self._gmf, self._mlp
        gu, gi = _rows(gmf, users, items) if flags & 2 else (None, None)
        mu, mi = _rows(mlp, users, items) if flags & 1 else (None, None)
        ids = _arange(gu if gu is not None else mu)
        w, b = (gmf.gmf_fc.weight, gmf.gmf_fc.bias) if flags & 2 else (None, None)
        y_gmf, X0 = _NeuMFFn.apply(ids, ids, gu, gi, mu, mi, w, b, flags, "rows")
        if not flags & 1:
            return y_gmf.view(users.shape)
        return run_tail(mlp.tower(), X0, last_add=y_gmf if flags & 2 else None).view(users.shape)

    def get_reg_loss(self, users, pos_items, neg_items) -> torch.Tensor:
        """(|rows of users|^2 + |rows of pos|^2 + |rows of neg|^2) / (2 len(users)) over the flagged parts' tables."""
        norm = torch.zeros((), device=users.device)
        parts = ([self._mlp] if self.mlp_flag() else []) + ([self._gmf] if self.gmf_flag() else [])
        for part in parts:
            norm = norm + part.item_emb_table(pos_items).norm(2).pow(2)
            norm = norm + part.item_emb_table(neg_items).norm(2).pow(2)
            norm = norm + part.user_emb_table(users).norm(2).pow(2)
        return norm / (2 * len(users))

    @property
    def num_user(self):
        return self._num_user

    @property
    def num_item(self):
        return self._num_item

    def get_embs(self) -> List[Tuple[str, IEmbedding]]:
        res = []
        if self.mlp_flag():
            res.extend([("mlp-user", self._mlp.user_emb_table), ("mlp-item", self._mlp.item_emb_table)])
        if self.gmf_flag():
            res.extend([("gmf-user", self._gmf.user_emb_table), ("gmf-item", self._gmf.item_emb_table)])
        return res

    def get_prune_loss_tanh(self, users, pos_items, neg_items, k=100):
        loss = torch.tensor(0.0, device=users.device)
        parts = ([self._mlp] if self.mlp_flag() else []) + ([self._gmf] if self.gmf_flag() else [])
        for part in parts:
            for table, ids in ((part.item_emb_table, pos_items), (part.item_emb_table, neg_items),
                               (part.user_emb_table, users)):
                loss = loss + self._get_prune_loss(table(ids), k)
        return loss

    def _get_prune_loss(self, emb, k):
        """Pruning loss of CERP."""
        emb = emb * k
        return -torch.tanh(emb).norm(2) ** 2

    def clear_cache(self):
        self._mlp._user_emb = None
        self._mlp._item_emb = None
        self._gmf._user_emb = None
        self._gmf._item_emb = None

    @torch.no_grad()
    def score_all_items(self, users: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """scores [len(users), num_item] of every item for each user: `model(users[:, None].repeat(1, N), arange(N))` of
        src/trainer/nmf.py:536-541 without the [B, N, D] lookups.  Eval-mode semantics (dropout off)."""
        return score_all_items(self, users, out)


def _tower_dims(model: NeuMF) -> List[int]:
    return [m.out_features for m in model._mlp.mlp if isinstance(m, nn.Linear)]


def score_supported(model: NeuMF) -> bool:
    """Whether mi_neumf_score_all takes this model's shape (else score_all_items runs the composed path)."""
    import ctypes

    flags = int(model.flag) & 3
    dims = _tower_dims(model)
    arr = (ctypes.c_int32 * max(len(dims), 1))(*dims)
    return bool(_lib.load().mi_neumf_score_supported(len(dims), ctypes.addressof(arr), model._emb_size // 2, flags))


COMPOSED_CHUNK_PAIRS = 1 << 20     # pairs per tower pass of the composed scoring path


@torch.no_grad()
def score_all_items(model: NeuMF, users: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    import ctypes

    from .mlp import run_tail

    dev = _lib.require_gpu(users, model._gmf.gmf_fc.weight)
    users = _kernels._i64c(users).view(-1)
    flags = int(model.flag) & 3
    B, N, D = users.numel(), model.num_item, model._emb_size // 2
    scores = out if out is not None else torch.empty((B, N), dtype=torch.float32, device=dev)
    if flags == 0:
        return scores.zero_()
    gmf, mlp = model._gmf, model._mlp
    if not score_supported(model):
        return _score_composed(model, users, scores)
    GU, GI = (_kernels._f32c(t.get_weight().detach()) for t in (gmf.user_emb_table, gmf.item_emb_table))
    MU, MI = (_kernels._f32c(t.get_weight().detach()) for t in (mlp.user_emb_table, mlp.item_emb_table))
    lins = [m for m in mlp.mlp if isinstance(m, nn.Linear)]
    dims = [m.out_features for m in lins]
    keep = []
    P = Q = None
    if flags & 1:
        W1 = _kernels._f32c(lins[0].weight.detach())
        h1 = dims[0]
        urows = _kernels.gather_rows(users, MU)
        P = torch.empty((B, h1), dtype=torch.float32, device=dev)
        Q = torch.empty((N, h1), dtype=torch.float32, device=dev)
        _kernels.gemm(urows, W1, P, B, h1, D, D, 2 * D, h1, transB=True)                          # MU[users] W1_u^T
        _kernels.gemm(MI, W1[:, D:], Q, N, h1, D, D, 2 * D, h1, transB=True, epi="bias",
                      bias=_kernels._f32c(lins[0].bias.detach()))                                  # MI W1_i^T + b1
        keep += [W1, urows]
    Ws = [_kernels._f32c(m.weight.detach()) for m in lins[1:]]
    bs = [_kernels._f32c(m.bias.detach()) for m in lins[1:]]
    keep += Ws + bs
    nh = len(dims)
    hid = (ctypes.c_int32 * max(nh, 1))(*dims)
    Wp = (ctypes.c_void_p * max(nh - 1, 1))(*[t.data_ptr() for t in Ws])
    bp = (ctypes.c_void_p * max(nh - 1, 1))(*[t.data_ptr() for t in bs])
    wf, bf = _kernels._f32c(mlp.mlp_fc.weight.detach()), _kernels._f32c(mlp.mlp_fc.bias.detach())
    wg, bg = _kernels._f32c(gmf.gmf_fc.weight.detach()), _kernels._f32c(gmf.gmf_fc.bias.detach())
    _lib.check(_lib.load().mi_neumf_score_all(_lib.ptr(P), _lib.ptr(Q), B, N, nh, ctypes.addressof(hid), ctypes.addressof(Wp),
                                              ctypes.addressof(bp), wf.data_ptr(), bf.data_ptr(), users.data_ptr(),
                                              GU.data_ptr(), GI.data_ptr(), D, GU.shape[0], wg.data_ptr(), bg.data_ptr(),
                                              flags, scores.data_ptr(), scores.stride(0), _lib.err_word(dev).data_ptr(),
                                              _lib.stream_ptr(dev)), "mi_neumf_score_all")
    return scores


def _score_composed(model: NeuMF, users: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
    """Towers mi_neumf_score_all does not take: chunks of (user, item) pairs through mi_neumf_fwd and mlp.run_tail."""
    from .mlp import run_tail

    B, N = scores.shape
    dev = scores.device
    flags = int(model.flag) & 3
    gmf, mlp = model._gmf, model._mlp
    tables = [t.get_weight().detach() for t in model._tables()]
    tower = mlp.tower().eval() if flags & 1 else None
    rows_per = max(1, COMPOSED_CHUNK_PAIRS // max(N, 1))
    items_all = torch.arange(N, dtype=torch.int64, device=dev)
    for s in range(0, B, rows_per):
        u = users[s:s + rows_per]
        n = u.numel()
        uu = u.view(-1, 1).expand(n, N).reshape(-1)
        ii = items_all.repeat(n)
        y_gmf, X0 = _NeuMFFn.apply(uu, ii, *tables, gmf.gmf_fc.weight.detach(), gmf.gmf_fc.bias.detach(), flags, "dense")
        y = y_gmf if not flags & 1 else run_tail(tower, X0, last_add=y_gmf if flags & 2 else None)
        scores[s:s + n].copy_(y.view(n, N))
    return scores


def get_sparsity_and_param(model: NeuMF) -> Tuple[float, int]:
    n_params = 0
    for _, emb in model.get_embs():
        n_params += emb.get_num_params()
    maximum_params = (model.num_user + model.num_item) * model._emb_size
    sparse_rate = 1 - n_params / maximum_params
    return sparse_rate, n_params

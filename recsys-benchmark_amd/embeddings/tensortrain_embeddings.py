"""TT-Rec embedding in its pure-PyTorch semantics — reference:
src/models/embeddings/tensortrain_embeddings.py:153-270 (`TTRecTorch`, registry key `tt_emb_torch`).

Same constructor, `tt_cores` ParameterList ([1, p_i, r_i*q_i*r_{i+1}] each, state_dict keys
`tt_cores.{i}`), shape suggestion and initialisers.  The lookup (mixed-radix index split, slice
gather, chained contraction) is one HIP kernel (mi_tt_fwd / mi_tt_bwd).  `get_weight()` is that
kernel over arange(N): the reference's own test pins forward(idx) == get_weight()[idx]
(tests/test_emb.py:458-478).  `tt_emb` (TTEmbedding below: the same table behind an LFU row cache)
keeps the reference's module and buffers on this build's own kernels (tt_cache.py).
"""
from typing import List, Optional

import numpy as np
import torch
from torch import nn

from .. import _kernels, tt_cache
from .base import IEmbedding


def suggested_tt_shapes(n: int, d: int = 3, allow_round_up: bool = True) -> List[int]:
    """Factor n (optionally rounded up to a rounder number) into d balanced factors: the shape with
    the highest entropy among all multiset partitions of the prime factors — same procedure and the
    same sympy/scipy calls as the reference (tt_embedding_ops.py:387-447), so the same answer."""
    from itertools import cycle, islice

    from scipy.stats import entropy
    from sympy.ntheory import factorint
    from sympy.utilities.iterables import multiset_partitions

    def interleave(*its):
        pending = len(its)
        nexts = cycle(iter(it).__next__ for it in its)
        while pending:
            try:
                for nxt in nexts:
                    yield nxt()
            except StopIteration:
                pending -= 1
                nexts = cycle(islice(nexts, pending))

    def best_shape(m: int) -> List[int]:
        primes: List[int] = []
        for prime, mult in factorint(m).items():
            primes += [prime] * mult
        if len(primes) < d:
            primes = primes + [1] * (d - len(primes))

        def canon(blocks):
            prods = sorted(np.prod(b) for b in blocks)
            half = len(prods) // 2
            return tuple(interleave(prods[:half], prods[half:]))

        shapes = list(set(canon(part) for part in multiset_partitions(primes, d)))
        return list(shapes[int(np.argmax([entropy(s) for s in shapes]))])

    def roundup(m: int, k: int) -> int:
        return int(np.ceil(m / 10 ** k)) * 10 ** k

    if not allow_round_up:
        return best_shape(n)
    scores = [entropy(best_shape(roundup(n, i))) for i in range(len(str(n)))]
    return best_shape(roundup(n, int(np.argmax(scores))))


def get_num_params(tt_p_shapes, tt_q_shapes, tt_ranks) -> int:
    return sum(tt_p_shapes[i] * tt_q_shapes[i] * tt_ranks[i] * tt_ranks[i + 1] for i in range(len(tt_p_shapes)))


def _init_cores(num_embeddings, embedding_dim, tt_ranks, weight_dist, tt_cores, tt_ndim, tt_p_shapes=None, tt_q_shapes=None):
    """Initialisers of the reference (tt_embedding_ops.py:818-986,989-1036).  They draw from numpy's global generator
    (and, for 'approx-uniform', Python's `random`) in the reference's order, so a seeded construction gives the same
    cores."""
    assert weight_dist in ["uniform", "naive-uniform", "normal", "approx-uniform", "approx-normal"]
    if weight_dist == "uniform":
        stddev = np.sqrt(2.0 / (num_embeddings + embedding_dim))
        var = np.prod(np.array(tt_ranks) ** (-1.0 / (2 * tt_ndim)))
        core_stddev = stddev ** (1.0 / tt_ndim) * var
        for c in tt_cores:
            nn.init.uniform_(c, 0.0, core_stddev)
    elif weight_dist == "naive-uniform":
        for c in tt_cores:
            nn.init.uniform_(c, 0.0, 1 / np.sqrt(num_embeddings))
    elif weight_dist == "normal":
        for c in tt_cores:
            nn.init.normal_(c, 0.0, 1.0 / np.sqrt(num_embeddings))
            c.data *= 1.0 / tt_ranks[0]
    elif weight_dist == "approx-normal":
        # every element is re-drawn until |w| >= 2 (the reference's loop keeps resampling the
        # |w| < 2 entries), then scaled by (3 N)^(-1/6)
        scale = np.power(1 / np.sqrt(3 * num_embeddings), 1 / 3)
        for c in tt_cores:
            W = np.random.normal(0.0, 1.0, size=tuple(c.shape)).astype(np.float32).flatten()
            redo = np.abs(W) < 2
            while redo.sum() > 0:
                W[redo] = np.random.normal(0.0, 1.0, size=(int(redo.sum()),)).astype(np.float32)
                again = np.zeros(len(W), dtype=np.bool_)
                again[redo] = np.abs(W[redo]) < 2
                redo = again
            c.data = torch.tensor(W.reshape(tuple(c.shape)) * scale, dtype=torch.float32, device=c.data.device)
    else:
        _init_approx_uniform(num_embeddings, tt_ranks, tt_cores, tt_ndim, tt_p_shapes, tt_q_shapes)


def _comb(count: int, teeth: int = 15, width: float = 0.7 / 30.0) -> np.ndarray:
    """`count` draws of the reference's "flat saw tooth" density: a tooth centre j/teeth, j uniform on -(teeth-1)..teeth-1,
    plus uniform(-width/2, width/2) (tt_embedding_ops.py:863-879; one randint call, then one rand call)."""
    centre = np.random.randint(-(teeth - 1), teeth, count)
    return centre * (1.0 / teeth) + (-width / 2.0 + width * np.random.rand(count))


def _init_approx_uniform(num_embeddings, tt_ranks, tt_cores, tt_ndim, tt_p_shapes, tt_q_shapes, sigma: float = 0.01):
    """3-core construction whose product is approximately uniform (tt_embedding_ops.py:861-986): core 0 ~ N(1/sqrt(r1),
    sigma) ; core 1 ~ N(1/sqrt(r1), sigma) except that for every (row, column) pair one EVEN outgoing-rank slice is
    N(0, sigma^2 sqrt(r1)) with a single saw-tooth entry (pre-divided by 1/sqrt(r1)); core 2 ~ N(0, sigma) with one
    saw-tooth entry on an ODD incoming rank per (row, column).  All three scaled by N^(-1/6) and stored [1, p_i, r_i q_i r_i+1]
    (rank-major slices transposed to row-major).  Draw order: numpy block, numpy comb, then per pair a Python-`random`
    slice pick, (core 1) r1 numpy normals, a Python-`random` entry pick — the normals are one [pairs, r1] call, which is the
    same stream."""
    import random

    if tt_ndim != 3:
        raise AssertionError("weight_dist='approx-uniform' needs exactly 3 cores (tt_embedding_ops.py:961)")
    amp = 1.0 / (np.sqrt(num_embeddings) ** (1.0 / 3.0))
    dims = [(tt_ranks[i], tt_p_shapes[i], tt_q_shapes[i], tt_ranks[i + 1]) for i in range(3)]

    def stored(block, i):
        block = (block * amp).astype(np.float32)
        return block.transpose(1, 0, 2, 3).reshape(1, tt_p_shapes[i], -1)

    # core 0: around 1/sqrt(r1) so that head x mid sums to ~1
    r0, p0, q0, r1 = dims[0]
    head = (1.0 / np.sqrt(r1) + np.random.randn(r0 * p0 * q0 * r1) * sigma).reshape(dims[0])

    # core 1
    r1_, p1, q1, r2 = dims[1]
    level = 1.0 / np.sqrt(r1_)
    pairs = p1 * q1
    mid = (level + np.random.randn(r1_ * pairs * r2) * sigma).reshape(r1_, pairs, r2)
    teeth = _comb(pairs) / level
    slices, entries = np.empty(pairs, dtype=np.int64), np.empty(pairs, dtype=np.int64)
    for e in range(pairs):              # Python's generator: slice pick, entry pick, per pair, in this order
        slices[e] = random.randrange(0, r2, 2)
        entries[e] = random.randrange(r1_)
    noise = np.random.randn(pairs, r1_) * (sigma * sigma / level)
    for e in range(pairs):
        mid[:, e, slices[e]] = noise[e]
        mid[entries[e], e, slices[e]] = teeth[e]
    mid = mid.reshape(dims[1])

    # core 2
    r2_, p2, q2, r3 = dims[2]
    tail = (np.random.randn(r2_ * p2 * q2 * r3) * sigma).reshape(r2_, -1)
    cols = tail.shape[1]
    teeth = _comb(cols)
    for e in range(cols):
        tail[random.randrange(1, r2_, 2), e] = teeth[e]
    tail = tail.reshape(dims[2])

    for i, block in enumerate((head, mid, tail)):
        tt_cores[i].data = torch.tensor(stored(block, i), dtype=torch.float32, device=tt_cores[i].data.device)


def _tt_setup(module, num_embeddings: int, embedding_dim: int, tt_ranks, tt_p_shapes, tt_q_shapes, weight_dist: str,
              enforce_embedding_dim: bool) -> None:
    """What TTRecTorch and TTEmbeddingBag share (reference tensortrain_embeddings.py:153-213, tt_embedding_ops.py:491-520,546-563,595):
    the suggested shapes, their checks, the `tt_cores` ParameterList and its initialisation, drawn in the reference's order."""
    module.tt_p_shapes = (
        suggested_tt_shapes(num_embeddings, len(tt_ranks) + 1) if tt_p_shapes is None else list(tt_p_shapes))
    module.tt_q_shapes = (
        suggested_tt_shapes(embedding_dim, len(tt_ranks) + 1, allow_round_up=(not enforce_embedding_dim))
        if tt_q_shapes is None else list(tt_q_shapes))
    assert len(module.tt_p_shapes) >= 2
    assert len(module.tt_p_shapes) <= 4
    assert len(tt_ranks) + 1 == len(module.tt_p_shapes)
    assert len(module.tt_p_shapes) == len(module.tt_q_shapes)
    assert np.prod(np.array(module.tt_p_shapes)) >= num_embeddings
    assert np.prod(np.array(module.tt_q_shapes)) == embedding_dim
    module.tt_ndim = len(tt_ranks) + 1
    module.num_embeddings = num_embeddings
    module.embedding_dim = embedding_dim
    module.tt_ranks = [1] + list(tt_ranks) + [1]
    module.num_tables = 1

    module.tt_cores = nn.ParameterList()
    for i in range(module.tt_ndim):
        module.tt_cores.append(nn.Parameter(torch.empty(
            [module.num_tables, module.tt_p_shapes[i],
             module.tt_ranks[i] * module.tt_q_shapes[i] * module.tt_ranks[i + 1]], dtype=torch.float32)))
    _init_cores(module.num_embeddings, module.embedding_dim, module.tt_ranks, weight_dist, module.tt_cores, module.tt_ndim,
                module.tt_p_shapes, module.tt_q_shapes)


class TTRecTorch(IEmbedding):
    def __init__(self, field_dims, hidden_size: int, tt_ranks: List[int], mode=None,
                 tt_p_shapes: Optional[List[int]] = None, tt_q_shapes: Optional[List[int]] = None,
                 weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False):
        super().__init__()
        if isinstance(field_dims, int):
            field_dims = [field_dims]
        self._mode = mode
        _tt_setup(self, sum(field_dims), hidden_size, tt_ranks, tt_p_shapes, tt_q_shapes, weight_dist, enforce_embedding_dim)

    def get_num_params(self):
        return get_num_params(self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks)

    def _lookup(self, flat_idx):
        return _kernels.tt_lookup(flat_idx, list(self.tt_cores), self.num_embeddings,
                                  [int(v) for v in self.tt_p_shapes], [int(v) for v in self.tt_q_shapes],
                                  [int(v) for v in self.tt_ranks])

    def get_weight(self):
        arr = torch.arange(self.num_embeddings, device=self.tt_cores[0].device)
        return self._lookup(arr)

    def forward(self, x):
        out = self._lookup(x.flatten()).reshape(*x.shape, self.embedding_dim)
        return _kernels.bag_reduce(out, self._mode)


class _BufferList(nn.Module):
    """Buffers registered as `<name>0`, `<name>1`, ...: the state_dict keys of the reference's BufferList
    (tt_embedding_ops.py:51-92), e.g. `optimizer_state.optimizer_state0`."""

    def __init__(self, name: str, buffers):
        super().__init__()
        for i, b in enumerate(buffers):
            self.register_buffer(name + str(i), b)


class TTEmbeddingBag(nn.Module):
    """One TT-Rec table with an LFU row cache — tt_embedding_ops.py:449-815 (`TableBatchedTTEmbeddingBag` with
    num_tables = 1) on this library's kernels.  Constructor arguments, buffers, their state_dict keys and the call sequence
    are the reference's; the kernels behind them (csrc/tt_cache.hip, the cached entry points of csrc/tt.hip; the
    grouped MFMA form for an uncached table, get_weight() and cache_populate()) are this build's own, and so is the hash: start slot id % hashtbl_size, linear probing, at most
    tt_cache.PROBE_BOUND probes.  With hashtbl_size >= num_embeddings (the default) slot == id.

    Differences from the reference, all on purpose:
    * `sparse=True` (the optimizer applied inside the backward) is not built: NotImplementedError.  Every config of the
      reference sets `sparse: False`; gradients are dense, `optimizer`, `learning_rate` and `eps` are stored only.
    * The module constructs on the CPU; `forward` needs the cores and the ids on a GPU.
    * No host read in `forward` (the reference's preprocess_indices_sync has one): the same launches run in warmup and
      after `cache_populate()`, so a captured graph stays valid across it.  `warmup` lives in a device word as well, which
      the probe launch reads: setting it is seen by graphs captured earlier.
    * A loaded state is re-hashed by this build's probe rule (a checkpoint written by FBTT has its ids in other slots).
    """

    def __init__(self, num_embeddings: int, embedding_dim: int, tt_ranks: List[int],
                 tt_p_shapes: Optional[List[int]] = None, tt_q_shapes: Optional[List[int]] = None,
                 optimizer=tt_cache.OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10, sparse: bool = True,
                 use_cache: bool = True, cache_size: int = 0, hashtbl_size: int = 0, weight_dist: str = "approx-normal",
                 enforce_embedding_dim: bool = False):
        super().__init__()
        assert num_embeddings > 0
        assert embedding_dim > 0
        if sparse:
            raise NotImplementedError("tt_emb with sparse=True applies the optimizer inside the backward, which this build does "
                                      "not have; set `sparse: False` in the embedding config (every TT-Rec config of the "
                                      "reference does) and step the dense gradients with an ordinary optimizer")
        _tt_setup(self, num_embeddings, embedding_dim, tt_ranks, tt_p_shapes, tt_q_shapes, weight_dist, enforce_embedding_dim)
        self.sparse = sparse
        self.optimizer = optimizer
        self.learning_rate = learning_rate
        self.eps = eps
        L, value = [], 1
        for p in reversed(self.tt_p_shapes):
            L.append(value)
            value *= int(p)
        self.register_buffer("L", torch.tensor(L[::-1], dtype=torch.int64))
        stateless = optimizer in (tt_cache.OptimType.SGD, tt_cache.OptimType.EXACT_SGD)
        self.optimizer_state = _BufferList("optimizer_state", [
            torch.zeros(0 if stateless else tuple(c.shape), dtype=torch.float32) for c in self.tt_cores])
        if cache_size <= 0:
            cache_size = int(0.1 * num_embeddings)
        self.use_cache = use_cache
        if use_cache:
            if hashtbl_size <= 0:
                hashtbl_size = num_embeddings
            assert hashtbl_size >= cache_size
            self.register_buffer("hashtbl", torch.full((hashtbl_size,), -1, dtype=torch.int64))
            self.register_buffer("cache_freq", torch.zeros(hashtbl_size, dtype=torch.int64))
            self.register_buffer("cache_state", torch.full((hashtbl_size,), -1, dtype=torch.int32))
            self.cache_weight = nn.Parameter(torch.zeros((cache_size, embedding_dim), dtype=torch.float32))
            self.register_load_state_dict_post_hook(TTEmbeddingBag._loaded)
        else:
            self.register_buffer("hashtbl", torch.zeros(0, dtype=torch.int64))
            self.register_buffer("cache_state", torch.zeros(0, dtype=torch.int32))
            self.cache_weight = None
        self.cache_optimizer_state = None
        self.register_buffer("_warm", torch.ones(1, dtype=torch.int32), persistent=False)
        self._rehash_pending = False
        self.warmup = True

    # `warmup` (tt_embedding_ops.py:649,696): True until cache_populate(); while it holds every lookup is contracted
    @property
    def warmup(self) -> bool:
        return self._warmup

    @warmup.setter
    def warmup(self, value: bool) -> None:
        self._warmup = bool(value)
        self._warm.fill_(1 if value else 0)

    @staticmethod
    def _loaded(module, incompatible_keys) -> None:
        module._rehash_pending = True
        module._rehash()

    def _rehash(self) -> None:
        if self._rehash_pending and self.hashtbl.is_cuda:
            tt_cache.rehash(self.hashtbl, self.cache_freq, self.cache_state)
            self._rehash_pending = False

    def _shapes(self):
        return ([int(v) for v in self.tt_p_shapes], [int(v) for v in self.tt_q_shapes], [int(v) for v in self.tt_ranks])

    def _contract(self, flat_idx):
        return _kernels.tt_lookup(flat_idx, list(self.tt_cores), self.num_embeddings, *self._shapes())

    def full_weight(self) -> torch.Tensor:
        """The whole table from the cores alone, cache ignored (tt_embedding_ops.py:651-661)."""
        return self._contract(torch.arange(self.num_embeddings, device=self.tt_cores[0].device))

    def cache_populate(self) -> None:
        if self.use_cache:
            self._rehash()
            tt_cache.populate(self.hashtbl, self.cache_freq, self.cache_state, self.cache_weight, self._contract)
            self.warmup = False

    def get_params(self):
        return list(self.tt_cores) + ([self.cache_weight] if self.use_cache else [])

    def forward(self, indices: torch.Tensor) -> torch.Tensor:
        """[n] ids -> [n, D] rows.  With the cache every forward counts its ids, in training and eval alike."""
        flat = indices.long().reshape(-1)
        if not self.use_cache:
            return self._contract(flat)
        self._rehash()
        loc = tt_cache.probe_count(flat, self.hashtbl, self.cache_freq, self.cache_state, self.num_embeddings,
                                   self.cache_weight.shape[0], self._warm)
        return tt_cache.tt_cached_lookup(flat, loc, self.cache_weight, list(self.tt_cores), self.num_embeddings,
                                         *self._shapes())


class TTEmbedding(IEmbedding):
    """Registry key `tt_emb` — tensortrain_embeddings.py:20-96: a TTEmbeddingBag behind the IEmbedding interface.

    `kwargs` are TTEmbeddingBag's (tt_ranks, tt_p_shapes, tt_q_shapes, optimizer, learning_rate, eps, sparse, use_cache,
    cache_size, hashtbl_size, weight_dist, enforce_embedding_dim).  A config that does not name `sparse` gets the dense
    path, the only one built; naming `sparse: True` raises NotImplementedError.

    mode None: [B] -> [B, D], [B, F] -> [B, F, D].  "sum" / "mean" reduce a 2-D input's rows through _kernels.bag_reduce
    like TTRecTorch: "mean" divides by the bag length.  The reference SUMS in both cases (its bags go to the FBTT kernel as
    offsets, which knows no mean); a 1-D input is one id per bag and comes back as it is in every mode.

    Speed: with `use_cache: True` every batch runs the per-lookup kernels (one workgroup per contracted lookup), also above
    the 4096 lookups at which `tt_emb_torch` and `use_cache: False` switch to the grouped MFMA form — in warmup, and at low
    hit rates after it, that is slower than `tt_emb_torch`, and the probe launch comes on top.  The cache pays only once most
    lookups hit it; nothing of this is timed yet.  `forward`'s `warmup` argument is the reference's
    (tensortrain_embeddings.py:57) and, as there, is not used: the table's own `_tt_emb.warmup` decides."""

    def __init__(self, field_dims, hidden_size: int, mode=None, **kwargs):
        assert mode in ["mean", "sum", None], f"{mode} is not supported"
        if isinstance(field_dims, int):
            field_dims = [field_dims]
        super().__init__()
        kwargs.setdefault("sparse", False)
        self._tt_emb = TTEmbeddingBag(sum(field_dims), hidden_size, **kwargs)
        self._mode = mode
        self._num_item = sum(field_dims)
        self._hidden_size = hidden_size
        self._field_dims = field_dims

    def get_weight(self):
        return self._tt_emb.full_weight()

    def get_num_params(self) -> int:
        return sum(p.numel() for p in self._tt_emb.get_params())

    def cache_populate(self):
        self._tt_emb.cache_populate()

    def forward(self, x, warmup=True):
        assert self._tt_emb.tt_cores[0].device.type != "cpu" and x.device.type != "cpu", \
            "CPU Operation is not supported by TTEmbedding"
        rows = self._tt_emb(x)
        if x.dim() == 1:
            return rows
        return _kernels.bag_reduce(rows.reshape(*x.shape, self._hidden_size), self._mode)

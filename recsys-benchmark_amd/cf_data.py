"""Device-resident collaborative-filtering data — reference: src/dataset/cf_graph_dataset.py (`CFGraphDataset`,
`TestCFGraphDataset`) and the `DataLoader`s the CF trainers wrap around them.

The graph is read once on the host, its index arrays go to the device once, and from then on an epoch's
(user, positive, negatives) triples come from ONE launch of mi_cf_sample_triples (csrc/cf_data.hip) and a validation's
NDCG / recall from ONE launch of mi_ndcg_recall_rows: no Python per sample, per batch launch or per user.

What is kept from the reference: the text format (`user item item ...`, users without items skipped with a warning),
`num_users` = number of users kept, `num_items` = largest item id + 1, `per_user_num` = interactions // users, `len()`
per sampling method, duplicates of an interaction kept in the stored lists (and so in the adjacency's degrees and in the
odds of a uniform positive).  What differs, on purpose: the random numbers (a counter-based generator on the device, see
include/mi355x_recsys.h, not Python's `random`), the order of the K negatives of a sample (draw order, where the
reference returns `list(set)`), and user ids that are not exactly 0..U-1 are refused with ValueError (the reference's
uniform mode indexes its dict with `idx // per_user_num` and raises KeyError there).
"""
import logging
from typing import Dict, Iterator, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _kernels
from .graph_utils import calculate_sparse_graph_adj_norm, get_adj

logger = logging.getLogger(__name__)

Graph = Dict[int, List[int]]


def load_graph(path: str) -> Graph:
    """user -> stored item list (file order, duplicates kept) of a `user item item ...` text file."""
    graph: Graph = {}
    with open(path) as fin:
        for line in fin:
            fields = line.split()
            if not fields:
                continue
            if len(fields) == 1:
                logger.warning("user %s has no item in %r: removed from the dataset", fields[0], line)
                continue
            graph[int(fields[0])] = [int(f) for f in fields[1:]]
    return graph


def _as_graph(graph_or_path: Union[str, Graph]) -> Graph:
    if isinstance(graph_or_path, dict):
        graph = {}
        for user, items in graph_or_path.items():
            if len(items) == 0:
                logger.warning("user %s has no item: removed from the dataset", user)
                continue
            graph[int(user)] = list(items)
    else:
        graph = load_graph(graph_or_path)
    if not graph:
        raise ValueError("the graph holds no interaction")
    if sorted(graph) != list(range(len(graph))):
        raise ValueError(f"user ids must be exactly 0..{len(graph) - 1} (every user with at least one item)")
    return graph


def _pair_arrays(graph: Graph) -> Tuple[np.ndarray, np.ndarray]:
    """(user, item) of every stored interaction in the graph's own order."""
    lens = np.fromiter((len(v) for v in graph.values()), dtype=np.int64, count=len(graph))
    users = np.repeat(np.fromiter(graph.keys(), dtype=np.int64, count=len(graph)), lens)
    items = np.fromiter((i for v in graph.values() for i in v), dtype=np.int64, count=int(lens.sum()))
    if items.size and items.min() < 0:
        raise ValueError("item ids must not be negative")
    return users, items


def _crow(users: np.ndarray, num_users: int) -> np.ndarray:
    crow = np.zeros(num_users + 1, dtype=np.int64)
    np.cumsum(np.bincount(users, minlength=num_users), out=crow[1:])
    return crow


def _membership(users: np.ndarray, items: np.ndarray, num_users: int, num_items: int) -> Tuple[np.ndarray, np.ndarray]:
    """CSR of the DISTINCT (user, item) pairs, every row ascending."""
    keys = np.unique(users * num_items + items)
    return _crow(keys // num_items, num_users), keys % num_items


class ResidentGraph(dict):
    """The dataset's graph dict (what `get_graph()` returns, read-only by contract) that also knows the dataset's stored
    lists on the device: `lightgcn.train_items_csr` takes them instead of flattening the dict again."""

    resident_csr: Optional[Tuple[torch.Tensor, torch.Tensor]] = None


class _GraphData:
    """What both datasets share: the parsed graph, its sizes and its index arrays."""

    def __init__(self, graph_or_path: Union[str, Graph], device):
        graph = _as_graph(graph_or_path)
        self.device = torch.device(device)
        self._graph = ResidentGraph(graph)
        self._num_users = len(graph)
        self._pair_user_np, self._pair_item_np = _pair_arrays(graph)
        self._num_items = int(self._pair_item_np.max()) + 1
        self._num_interactions = int(self._pair_item_np.size)
        if self._num_items >= 2 ** 31:
            raise ValueError("item ids must fit int32")

    @property
    def num_users(self) -> int:
        return self._num_users

    @property
    def num_items(self) -> int:
        return self._num_items

    def get_graph(self) -> Graph:
        return self._graph

    def _to_device(self, array: np.ndarray, dtype=torch.int64) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(array)).to(dtype).to(self.device)


class DeviceCFGraphDataset(_GraphData):
    """`CFGraphDataset` with its arrays on the device (the reference's constructor arguments and defaults, a graph dict
    accepted in the place of the path).  `sample` draws any range of an epoch through mi_cf_sample_triples; a
    `DeviceCFLoader` feeds the `train_epoch_*` functions from it."""

    def __init__(self, graph_or_path: Union[str, Graph], adj_style: str = "lightgcn", sampling_method: str = "uniform",
                 num_neg_item: int = 1, device="cuda"):
        if adj_style not in ("lightgcn", "hccf"):
            raise ValueError(f"adj_style={adj_style!r}: only 'lightgcn' and 'hccf'")
        if sampling_method not in ("uniform", "popularity"):
            raise ValueError(f"sampling_method={sampling_method!r}: only 'uniform' and 'popularity'")
        if num_neg_item < 1:
            raise ValueError("num_neg_item must be at least 1")
        super().__init__(graph_or_path, device)
        self.adj_style, self.sampling_method, self.num_neg_item = adj_style, sampling_method, num_neg_item
        self.per_user_num = self._num_interactions // self._num_users
        self.dataset_length = self._num_users * self.per_user_num
        self._norm_adj = None
        users, items = self._pair_user_np, self._pair_item_np
        by_user = np.argsort(users, kind="stable")           # the stored lists, user after user (a no-op on a sorted file)
        pos_crow, pos_col = _membership(users, items, self._num_users, self._num_items)
        self.pair_user = self._to_device(users)
        self.pair_item = self._to_device(items)
        self.stored_item = self.pair_item if np.array_equal(by_user, np.arange(users.size)) \
            else self._to_device(items[by_user])
        self.pair_crow = self._to_device(_crow(users, self._num_users))
        self.pos_crow = self._to_device(pos_crow)
        self.pos_col = self._to_device(pos_col, torch.int32)
        self._graph.resident_csr = (self.pair_crow, self.stored_item)

    def __len__(self) -> int:
        return self.dataset_length if self.sampling_method == "uniform" else self._num_interactions

    def get_norm_adj(self) -> torch.Tensor:
        if self._norm_adj is None:
            if self.adj_style == "lightgcn":
                self._norm_adj = calculate_sparse_graph_adj_norm(self._graph, self.num_items, self.num_users)
            else:
                self._norm_adj = get_adj(self._graph, self.num_items, self.num_users, normalize=True)
        return self._norm_adj

    def describe(self) -> None:
        """Logs the sizes, the density and the extreme user degrees (stored interactions per user)."""
        degrees = [len(items) for items in self._graph.values()]
        logger.info("%d users, %d items, %d interactions (density %.3g); user degree %d..%d", self.num_users, self.num_items,
                    self._num_interactions, self._num_interactions / (self.num_users * self.num_items), min(degrees),
                    max(degrees))

    def sample(self, first: int, n: int, epoch: int, seed: int, order: Optional[torch.Tensor] = None):
        """(users [n], pos [n], neg) of samples [first, first + n) of epoch `epoch`: neg is [n] for one negative, a list
        of num_neg_item [n] views otherwise — what the default collate makes of the reference's items.  `order`
        (popularity sampling only): int64 [n], the pair each of these samples takes."""
        if first < 0 or n < 0 or first + n > len(self):
            raise IndexError(f"samples [{first}, {first + n}) lie outside an epoch of {len(self)}")
        if order is not None and self.sampling_method != "popularity":
            raise ValueError("`order` names pairs: it applies to popularity sampling only")
        uniform = self.sampling_method == "uniform"
        users, pos, neg = _kernels.cf_sample_triples(
            self.pair_user, self.stored_item if uniform else self.pair_item, self.pair_crow, self.pos_crow, self.pos_col,
            self.num_items, self.sampling_method, self.per_user_num, self.num_neg_item, first, n, seed, epoch, order)
        return users, pos, (neg[0] if self.num_neg_item == 1 else list(neg.unbind(0)))


def _epoch_seed(seed: int, epoch: int) -> int:
    return (seed + 0x9E3779B97F4A7C15 * (epoch + 1)) & (2 ** 63 - 1)


class DeviceCFLoader:
    """The `DataLoader` of the CF trainers over a DeviceCFGraphDataset: `__iter__` samples the whole epoch in one launch
    and yields `(users, pos, neg)` slices of it, so a batch costs no launch and no host work.  `shuffle` permutes the
    epoch's samples with `torch.randperm` on the device under a generator seeded from (seed, epoch); seed None takes
    `torch.initial_seed()`.  The epoch counter advances with every `__iter__`; `set_epoch` moves it."""

    def __init__(self, dataset: DeviceCFGraphDataset, batch_size: int, shuffle: bool = False, drop_last: bool = False,
                 seed: Optional[int] = None):
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        self.seed = torch.initial_seed() if seed is None else int(seed)
        self.epoch = 0

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def sample_epoch(self, epoch: int):
        """(users [n], pos [n], neg [K, n]-like as `sample` returns it) of one whole epoch, in the order it is served."""
        ds, n = self.dataset, len(self.dataset)
        if not self.shuffle:
            return ds.sample(0, n, epoch, self.seed)
        gen = torch.Generator(device=ds.device)
        gen.manual_seed(_epoch_seed(self.seed, epoch))
        perm = torch.randperm(n, generator=gen, device=ds.device)
        if ds.sampling_method == "popularity":
            return ds.sample(0, n, epoch, self.seed, order=perm)
        users, pos, neg = ds.sample(0, n, epoch, self.seed)      # a uniform sample is tied to its user: permute the result
        return users[perm], pos[perm], ([t[perm] for t in neg] if isinstance(neg, list) else neg[perm])

    def __iter__(self) -> Iterator:
        users, pos, neg = self.sample_epoch(self.epoch)
        self.epoch += 1
        n, b = users.numel(), self.batch_size
        for s in range(0, n - b + 1 if self.drop_last else n, b):
            e = min(s + b, n)
            yield users[s:e], pos[s:e], ([t[s:e] for t in neg] if isinstance(neg, list) else neg[s:e])


class DeviceTruth:
    """The truth item sets of a validation as a CSR on the device (rows distinct and ascending) — what a
    DeviceCFTestLoader hands over in the place of the reference's list of Python sets."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor):
        self.crow, self.col = crow, col

    def ndcg_recall(self, pred: torch.Tensor, users: torch.Tensor, k: int) -> Tuple[float, float]:
        """(ndcg, recall) at k of `pred` [n, >= k] for `users` [n]: per-user values by mi_ndcg_recall_rows, their
        float64 means by torch."""
        ndcg, recall = _kernels.ndcg_recall_rows(pred, users, self.crow, self.col, k)
        return float(ndcg.mean()), float(recall.mean())


class DeviceCFTestDataset(_GraphData):
    """`TestCFGraphDataset` with the users and their truth sets on the device."""

    def __init__(self, graph_or_path: Union[str, Graph], device="cuda"):
        super().__init__(graph_or_path, device)
        crow, col = _membership(self._pair_user_np, self._pair_item_np, self._num_users, self._num_items)
        self.users = self._to_device(np.fromiter(self._graph.keys(), dtype=np.int64, count=self._num_users))
        self.truth = DeviceTruth(self._to_device(crow), self._to_device(col))

    def __len__(self) -> int:
        return self._num_users


class DeviceCFTestLoader:
    """Yields `(users, DeviceTruth)` per batch of users, in the file's user order."""

    def __init__(self, dataset: DeviceCFTestDataset, batch_size: int):
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.dataset, self.batch_size = dataset, int(batch_size)

    def __len__(self) -> int:
        return -(-len(self.dataset) // self.batch_size)

    def __iter__(self) -> Iterator:
        users = self.dataset.users
        for s in range(0, users.numel(), self.batch_size):
            yield users[s:s + self.batch_size], self.dataset.truth

"""Device-resident click-through data — reference: src/dataset/criteo/criteo_torchfm.py (`CriteoDataset`) and the
`DataLoader`s the CTR trainers wrap around it.

The reference reads the text file twice in Python (count every feature, then map features seen fewer than
`min_threshold` times to one out-of-vocabulary id per field), stores `uint32[1 + F]` records in LMDB and pays one
`__getitems__`, a collate and a host-to-device copy per batch.  Here the text is read once on the host into integer keys
(`read_criteo_text`), the vocabulary rule runs on the device column by column (`encode_ctr_columns`: torch's stable sort,
then mi_ctr_vocab_field of csrc/ctr_data.hip), the `uint32 [n, 1 + F]` record array stays in HBM (`DeviceCTRDataset`), and
a batch — shuffled or not — is ONE launch of mi_ctr_batch (`DeviceCTRLoader`): no Python per sample, no collate, no copy.

What is kept from the reference: the text format (lines with another column count skipped, line numbers kept for
`train_test_info`), `convert_numeric_feature`, the threshold rule, `field_dims[f] = kept + 1`, the out-of-vocabulary id
`kept`, the record layout (label first).  What differs, on purpose: kept features are numbered in ascending key order
(the reference numbers them in set-iteration order, which no run can reproduce; the two agree up to a renaming of the
kept ids per field), and the shuffle is the keyed bijection of include/mi355x_recsys.h, not `torch.randperm`.
"""
import logging
import math
from typing import Iterator, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib

logger = logging.getLogger(__name__)

NUM_INT_FEATS = 13
NUM_FEATS = 39
NULL_KEY = -(1 << 63)          # an empty integer field (the reference's "NULL")
EMPTY_KEY = -1                 # an empty categorical field (the reference's "")


def _numeric_key(val: str) -> int:
    """`convert_numeric_feature` as an integer: equal exactly when the reference's strings are equal ("NULL" apart, every
    string it returns is the decimal form of the integer returned here)."""
    if val == "":
        return NULL_KEY
    v = int(val)
    return int(math.log(v) ** 2) if v > 2 else v - 2


def read_criteo_text(path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(keys int64 [n, 39], labels uint8 [n], line_no int64 [n]) of a tab-separated Criteo file (label, 13 integer
    fields, 26 categorical fields).  Lines with another column count are skipped as the reference skips them; line_no
    holds the 0-based line numbers of the lines kept (what the reference's LMDB keys and `train_test_info` count)."""
    numeric = {}               # distinct strings -> key: math.log runs once per distinct value
    rows, labels, line_no = [], [], []
    with open(path) as f:
        for idx, line in enumerate(f):
            values = line.rstrip("\n").split("\t")
            if len(values) != NUM_FEATS + 1:
                continue
            row = []
            for s in values[1:NUM_INT_FEATS + 1]:
                key = numeric.get(s)
                if key is None:
                    key = numeric[s] = _numeric_key(s)
                row.append(key)
            row.extend(int(s, 16) if s else EMPTY_KEY for s in values[NUM_INT_FEATS + 1:])
            rows.append(row)
            labels.append(int(values[0]))
            line_no.append(idx)
    keys = np.array(rows, dtype=np.int64).reshape(len(rows), NUM_FEATS)
    return keys, np.array(labels, dtype=np.uint8), np.array(line_no, dtype=np.int64)


def _s64(v: int) -> int:
    """An integer as a two's-complement 64-bit word."""
    return ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)


def _records_out(records_i32: torch.Tensor) -> torch.Tensor:
    return records_i32.view(torch.uint32) if hasattr(torch, "uint32") else records_i32


def encode_ctr_columns(keys, labels, min_threshold: int = 10, device="cuda") -> Tuple[torch.Tensor, np.ndarray]:
    """(records uint32 [n, 1 + F] on the device, field_dims int64 [F]) of keys int64 [n, F] and labels [n] (host arrays or
    tensors).  Per field a key seen at least `min_threshold` times is kept, kept keys get the ids 0 .. kept-1 in ascending
    key order, every other key the id `kept`; field_dims[f] = kept + 1; records[:, 0] is the label.

    One column at a time (the whole key matrix never sits on the device): copy, `torch.sort(stable=True)`, the three
    launches of mi_ctr_vocab_field.  The only read-back is the F counts, at the end."""
    if min_threshold < 1:
        raise ValueError("min_threshold must be at least 1")
    keys = torch.as_tensor(keys)
    labels = torch.as_tensor(labels)
    if keys.dim() != 2 or keys.shape[1] < 1 or keys.dtype != torch.int64:
        raise ValueError(f"keys must be int64 [n, F] with F >= 1; got {keys.dtype} {tuple(keys.shape)}")
    n, F = keys.shape
    if labels.shape != (n,):
        raise ValueError(f"labels must be [n] = [{n}]; got {tuple(labels.shape)}")
    if n > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 records")
    device = torch.device(device)
    lib = _lib.load()
    records = torch.zeros((n, 1 + F), dtype=torch.int32, device=device)
    counts = torch.zeros(F, dtype=torch.int64, device=device)
    _lib.require_gpu(records)
    if n:
        records[:, 0] = labels.to(device).to(torch.int32)
    ws = torch.zeros(int(lib.mi_ctr_vocab_workspace_bytes(n)), dtype=torch.uint8, device=device)
    err, stream = _lib.err_word(device).data_ptr(), _lib.stream_ptr(device)
    for f in range(F):
        column = keys[:, f].contiguous().to(device)
        sorted_keys, perm = torch.sort(column, stable=True)
        _lib.check(lib.mi_ctr_vocab_field(sorted_keys.data_ptr(), perm.data_ptr(), n, int(min_threshold),
                                          records.data_ptr() + 4 * (1 + f), 1 + F, counts.data_ptr() + 8 * f, ws.data_ptr(),
                                          err, stream), "mi_ctr_vocab_field")
    return _records_out(records), counts.cpu().numpy() + 1


def ctr_batch(records: torch.Tensor, index: Optional[torch.Tensor], first: int, count: int, epoch: int, seed: int,
              shuffle: bool, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x int64 [count, F], y float32 [count]): samples [first, first + count) of epoch `epoch` over `records`
    (int32 / uint32 [n, 1 + F], contiguous, on the device) by ONE mi_ctr_batch launch (include/mi355x_recsys.h spells the
    shuffle out).  index: int64 [m] record rows the epoch runs over (None: all of them).  out=(x, y): buffers to fill."""
    dev = _lib.require_gpu(records, index)
    if records.dim() != 2 or records.shape[1] < 2 or records.element_size() != 4 or records.is_floating_point() \
            or not records.is_contiguous():
        raise TypeError("records must be a contiguous 32-bit integer [n, 1 + F] tensor")
    if index is not None and (index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous()):
        raise TypeError("index must be a contiguous int64 [m] tensor")
    n_records, F = records.shape[0], records.shape[1] - 1
    n = n_records if index is None else index.numel()
    if first < 0 or count < 0 or first + count > n:
        raise IndexError(f"samples [{first}, {first + count}) lie outside an epoch of {n}")
    if out is None:
        x = torch.zeros((count, F), dtype=torch.int64, device=dev)
        y = torch.zeros(count, dtype=torch.float32, device=dev)
    else:
        x, y = out
        _lib.require_gpu(records, x, y)
        if x.dtype != torch.int64 or tuple(x.shape) != (count, F) or not x.is_contiguous() \
                or y.dtype != torch.float32 or tuple(y.shape) != (count,) or not y.is_contiguous():
            raise ValueError(f"out must be (int64 [{count}, {F}], float32 [{count}]), both contiguous")
    _lib.check(_lib.load().mi_ctr_batch(records.data_ptr(), n_records, F, _lib.ptr(index), n, int(bool(shuffle)), _s64(seed),
                                        _s64(epoch), int(first), int(count), x.data_ptr(), y.data_ptr(),
                                        _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)), "mi_ctr_batch")
    return x, y


def _records_i32(records, device) -> torch.Tensor:
    """`records` (a 32-bit or int64 integer array or tensor, anywhere) as a contiguous int32 tensor on `device` holding the
    same 32-bit words."""
    if isinstance(records, np.ndarray):
        if records.dtype == np.uint32:
            records = records.view(np.int32)
        records = torch.from_numpy(np.ascontiguousarray(records))
    if hasattr(torch, "uint32") and records.dtype == torch.uint32:
        records = records.view(torch.int32)
    if records.dtype == torch.int64:
        if records.numel() and (int(records.min()) < 0 or int(records.max()) >= 2 ** 31):
            raise ValueError("a record word lies outside [0, 2^31)")
        records = records.to(torch.int32)
    if records.dtype != torch.int32:
        raise TypeError(f"records must hold 32-bit integers; got {records.dtype}")
    return records.contiguous().to(device)


class DeviceCTRDataset:
    """The reference's `ICTRDataset` with its records in HBM: `records` is uint32 / int32 [n, 1 + F] (label first, then
    one id per field) — what `encode_ctr_columns` returns, or anything already encoded, for example an array dumped from
    the reference's LMDB.  `index` (optional, int64 record rows) makes the dataset a view: train / val / test are three
    views of one resident array (`subset`).  Construction checks once, on the device, that every id is below its
    `field_dims` entry and every label 0 or 1 (ValueError otherwise)."""

    def __init__(self, records, field_dims, index=None, device="cuda", _checked: bool = False):
        shape = tuple(records.shape)
        self.field_dims = np.asarray(field_dims, dtype=np.int64).reshape(-1)
        if len(shape) != 2 or shape[1] < 2:
            raise ValueError(f"records must be [n, 1 + F]; got {shape}")
        if self.field_dims.size != shape[1] - 1:
            raise ValueError(f"field_dims names {self.field_dims.size} fields, the records hold {shape[1] - 1}")
        if self.field_dims.size and self.field_dims.min() < 1:
            raise ValueError("every field dimension must be at least 1")
        if index is not None:
            index = torch.as_tensor(index)
            if index.dtype != torch.int64 or index.dim() != 1:
                raise ValueError("index must be an int64 vector of record rows")
            if index.numel() and (int(index.min()) < 0 or int(index.max()) >= shape[0]):
                raise ValueError(f"index names a row outside the {shape[0]} records")
        self.device = torch.device(device)
        self.records = records if _checked else _records_i32(records, self.device)
        self.index = None if index is None else index.contiguous().to(self.device)
        if not _checked and shape[0]:
            dims = torch.from_numpy(self.field_dims).to(self.device)
            ids, labels = self.records[:, 1:], self.records[:, 0]
            bad = torch.stack([((ids < 0) | (ids >= dims)).any(), ((labels != 0) & (labels != 1)).any()]).tolist()
            if bad[0]:
                raise ValueError("a record holds an id at or above its field's dimension")
            if bad[1]:
                raise ValueError("a record holds a label that is neither 0 nor 1")

    def __len__(self) -> int:
        return self.records.shape[0] if self.index is None else self.index.numel()

    @property
    def num_fields(self) -> int:
        return self.field_dims.size

    def pop_info(self) -> dict:
        return {}

    def describe(self) -> None:
        logger.info("device-resident CTR dataset: %d samples over %d records, %d fields", len(self), self.records.shape[0],
                    self.num_fields)
        logger.info("Field dims %s", self.field_dims)
        logger.info("sum dims %d", int(self.field_dims.sum()))

    def subset(self, index) -> "DeviceCTRDataset":
        """A view over the record rows `index` (int64, rows of the RESIDENT array, whatever this dataset's own index is);
        the records are shared, not copied."""
        return DeviceCTRDataset(self.records, self.field_dims, index=index, device=self.device, _checked=True)

    @classmethod
    def from_criteo_text(cls, path: str, train_test_info=None, dataset_name: Optional[str] = None, min_threshold: int = 10,
                         device="cuda") -> "DeviceCTRDataset":
        """The whole file encoded (the vocabulary counts every line, as the reference's cache does); with `train_test_info`
        (the reference's `torch.load`-able dict, or the dict itself) the dataset is the view over `dataset_name`'s line
        numbers, sorted as the reference sorts them."""
        keys, labels, line_no = read_criteo_text(path)
        records, field_dims = encode_ctr_columns(keys, labels, min_threshold, device)
        index = None
        if train_test_info is not None:
            info = train_test_info if isinstance(train_test_info, dict) else torch.load(train_test_info, weights_only=False)
            lines = np.sort(np.asarray(list(info[dataset_name]), dtype=np.int64))
            index = np.searchsorted(line_no, lines)
            if lines.size and (index.max() >= line_no.size or not np.array_equal(line_no[index], lines)):
                raise ValueError(f"{dataset_name!r} names a line the file does not hold (or one that was skipped)")
            index = torch.from_numpy(index)
        return cls(records, field_dims, index=index, device=device)


class DeviceCTRLoader:
    """The `DataLoader` of the CTR trainers over a DeviceCTRDataset: `__iter__` yields `(x int64 [b, F], y float32 [b])` per
    batch, each from ONE mi_ctr_batch launch into tensors of its own (train_epoch holds the next batch while it steps the
    current one).  `shuffle` applies the keyed bijection of include/mi355x_recsys.h under (seed, epoch); seed None takes
    `torch.initial_seed()`.  The epoch counter advances with every `__iter__`; `set_epoch` moves it."""

    def __init__(self, dataset: DeviceCTRDataset, batch_size: int, shuffle: bool = False, drop_last: bool = False,
                 seed: Optional[int] = None):
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), drop_last
        self.seed = torch.initial_seed() if seed is None else int(seed)
        self.epoch = 0

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def batch(self, first: int, count: int, epoch: int, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Samples [first, first + count) of epoch `epoch`, any range of it; out=(x, y) writes into the caller's buffers
        (and saves the fill launch of fresh ones)."""
        ds = self.dataset
        return ctr_batch(ds.records, ds.index, first, count, epoch, self.seed, self.shuffle, out)

    def __iter__(self) -> Iterator:
        epoch = self.epoch
        self.epoch += 1
        n, b = len(self.dataset), self.batch_size
        for s in range(0, n - b + 1 if self.drop_last else n, b):
            yield self.batch(s, min(b, n - s), epoch)

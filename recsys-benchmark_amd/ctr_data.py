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

Avazu (src/dataset/avazu/avazu_on_ram.py `_create_binary`, avazu/utils.py) and KDD 2012 track 2
(src/dataset/kdd/kdd_dataset.py) are read the same way: `read_avazu_text` / `read_kdd_text` on the host,
`parse_avazu_text` / `parse_kdd_text` on the device (one column-spec reader, mi_ctr_table_*), their feature strings as
int64 keys that are equal exactly when the strings are; `make_train_test_info` is the reference's Avazu split.
"""
import logging
import math
import os
import stat
from typing import Iterator, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib

logger = logging.getLogger(__name__)

NUM_INT_FEATS = 13
NUM_FEATS = 39
NULL_KEY = -(1 << 63)          # an empty integer field (the reference's "NULL")
EMPTY_KEY = -1                 # an empty categorical field (the reference's "")
NUM_AVAZU_FEATS, NUM_KDD_FEATS = 22, 11


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


def _token_key(s: str) -> int:
    """A feature string as the int64 whose big-endian bytes are the string's, zero-padded at the low end: equal exactly
    when the strings are equal, for strings of at most 8 bytes that hold no NUL."""
    b = s.encode()
    if len(b) > 8 or 0 in b:
        raise ValueError(f"no int64 key for the feature string {s!r}: more than 8 bytes, or a NUL among them")
    return _s64(int.from_bytes(b.ljust(8, b"\0"), "big"))


def _decimal_key(s: str) -> int:
    """A canonical decimal id below 2^64 as the int64 with its bit pattern ("01" and "1" are different strings with one
    value, so only the canonical form has a key)."""
    if not (s.isascii() and s.isdigit()) or (len(s) > 1 and s[0] == "0") or len(s) > 20 or int(s) >= 1 << 64:
        raise ValueError(f"no int64 key for the feature string {s!r}: not a canonical decimal below 2^64")
    return _s64(int(s))


def _host_result(rows, labels, line_no, F):
    return (np.array(rows, dtype=np.int64).reshape(len(rows), F), np.array(labels, dtype=np.uint8),
            np.array(line_no, dtype=np.int64))


def read_avazu_text(path: str, preprocess_timestamp: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(keys int64 [n, 22 or 25], labels uint8 [n], line_no int64 [n]) of Avazu's comma-separated file (id, click, 22
    feature strings, the first of them the hour as yymmddHH).  The header line is dropped; a line without 24 values is
    skipped as the reference skips it; line_no holds the kept lines' indices after the header, skipped ones counted (the
    reference's `train_test_info` lists).  A feature string's key is `_token_key`; with `preprocess_timestamp` three
    more columns hold the hour, the weekday (Monday 0) and whether it is 5 or 6, from `datetime.strptime` as in the
    reference (whose strings are these integers' decimal forms, and "True" / "False")."""
    import datetime

    token, rows, labels, line_no = {}, [], [], []
    with open(path) as f:
        f.readline()
        for idx, line in enumerate(f):
            values = line.rstrip("\n").split(",")
            if len(values) != NUM_AVAZU_FEATS + 2:
                continue
            row = []
            for s in values[2:]:
                key = token.get(s)
                if key is None:
                    key = token[s] = _token_key(s)
                row.append(key)
            if preprocess_timestamp:
                date = datetime.datetime.strptime(values[2], "%y%m%d%H")
                row.extend((date.hour, date.weekday(), int(date.weekday() in [5, 6])))
            rows.append(row)
            labels.append(int(values[1]))
            line_no.append(idx)
    return _host_result(rows, labels, line_no, NUM_AVAZU_FEATS + (3 if preprocess_timestamp else 0))


def read_kdd_text(path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(keys int64 [n, 11], labels uint8 [n], line_no int64 [n]) of KDD 2012 track 2's tab-separated file (a click count,
    then 11 decimal ids, some above 2^63: a key is the id's 64-bit pattern).  The label is `int(values[0]) >= 1`; a line
    without 12 values is a ValueError (the reference asserts the count)."""
    decimal, rows, labels, line_no = {}, [], [], []
    with open(path) as f:
        for idx, line in enumerate(f):
            values = line.rstrip("\n").split("\t")
            if len(values) != NUM_KDD_FEATS + 1:
                raise ValueError(f"line {idx} (0-based) does not hold {NUM_KDD_FEATS + 1} tab-separated values")
            row = []
            for s in values[1:]:
                key = decimal.get(s)
                if key is None:
                    key = decimal[s] = _decimal_key(s)
                row.append(key)
            rows.append(row)
            labels.append(int(int(values[0]) >= 1))
            line_no.append(idx)
    return _host_result(rows, labels, line_no, NUM_KDD_FEATS)


def make_train_test_info(line_no, seed: int = 2023, split_strategy: int = 1, metadata: Optional[dict] = None) -> dict:
    """The reference's Avazu split (`_create_binary`) of the kept lines `line_no`: {"train", "val", "test"} (lists of line
    numbers: int(0.8 n), int(0.1 n) and the rest) and "metadata".  split_strategy 1 cuts
    `torch.randperm(n, generator=torch.Generator().manual_seed(seed))`, which is what `random_split` draws; 0 cuts in
    file order."""
    if split_strategy not in (0, 1):
        raise ValueError(f"split_strategy must be 0 (file order) or 1 (random); got {split_strategy!r}")
    lines = (line_no.cpu() if isinstance(line_no, torch.Tensor) else torch.as_tensor(np.asarray(line_no))).reshape(-1).tolist()
    n = len(lines)
    num_train, num_val = int(0.8 * n), int(0.1 * n)
    if split_strategy == 1:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed))).tolist()
        lines = [lines[i] for i in order]
    info = {"train": lines[:num_train], "val": lines[num_train:num_train + num_val], "test": lines[num_train + num_val:]}
    info["metadata"] = dict(metadata or {}, seed=seed, split_strategy=split_strategy)
    return info


# ---- the device text reader (csrc/ctr_text.hip; include/mi355x_recsys.h spells the grammar out) ---------------------------
_thresholds: Optional[np.ndarray] = None
_text_state = {}               # device index -> the threshold table on that device


def numeric_thresholds() -> np.ndarray:
    """int64 [1906], strictly increasing: entry k - 1 is the smallest v in [3, 2^63) with `_numeric_key(v) >= k`, found by
    bisection over `_numeric_key` itself (which is non-decreasing in v) and cached.  The number of entries <= v is then
    `_numeric_key(v)` for every v > 2: what the device evaluates instead of the logarithm."""
    global _thresholds
    if _thresholds is None:
        top = (1 << 63) - 1
        table, lo = [], 3
        for k in range(1, _numeric_key(top) + 1):
            hi = top
            while lo < hi:
                mid = (lo + hi) // 2
                if _numeric_key(mid) >= k:
                    hi = mid
                else:
                    lo = mid + 1
            table.append(lo)
        table = np.array(table, dtype=np.int64)
        table.setflags(write=False)
        _thresholds = table
    return _thresholds


def _cut_chunks(readinto, chunk_bytes: int, total: Optional[int] = None) -> Iterator[Tuple[memoryview, bool]]:
    """(chunk, final) pairs of the byte stream behind `readinto(buffer) -> count` (0 at the end; `total`: its length where
    known): every chunk is at most `chunk_bytes` long and is cut after its last newline, the tail is carried into the
    next one; a last line without a newline comes alone with final = True.  A line that does not fit a chunk is a
    ValueError.  The chunks are views of ONE buffer, each valid until the next is asked for: host memory is that buffer."""
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be at least 1")
    if total == 0:
        return
    buf = bytearray(chunk_bytes if total is None else min(chunk_bytes, total))
    view, held = memoryview(buf), 0                         # `held` bytes of an unfinished line lie at the front
    while True:
        got = readinto(view[held:])
        if not got:
            if held:
                yield view[:held], True
            return
        filled = held + got
        cut = buf.rfind(b"\n", 0, filled) + 1
        if cut:
            yield view[:cut], False
            held = filled - cut
            buf[:held] = buf[cut:filled]
        elif filled < len(buf):
            held = filled
        elif len(buf) == chunk_bytes and readinto(bytearray(1)):
            raise ValueError(f"a line is longer than chunk_bytes = {chunk_bytes}")
        else:                                               # the stream ends with this line
            yield view[:filled], True
            return


def _thresholds_on(device: torch.device) -> torch.Tensor:
    """The threshold table resident on `device` (read-only, shared by every call)."""
    i = device.index if device.index is not None else torch.cuda.current_device()
    table = _text_state.get(i)
    if table is None:
        table = _text_state[i] = torch.from_numpy(numeric_thresholds().copy()).to(torch.device("cuda", i))
    return table


def _new_record(device: torch.device) -> torch.Tensor:
    """int64 [4] = {lines, kept, consumed, lowest refusal (all ones: none)}; one per call, so calls share no state."""
    return torch.tensor([0, 0, 0, -1], dtype=torch.int64, device=device)


_CRITEO_REFUSAL = ("not in the strict Criteo text grammar of the device reader (a label other than 0 or 1, a malformed or "
                   "over-long number, or a carriage return); read_criteo_text is the lenient reader")


def _raise_refusal(record: torch.Tensor, what: str = _CRITEO_REFUSAL) -> None:
    """One read-back of the record's refusal word; ValueError if a launch so far lowered it (the word is then cleared)."""
    word = int(record[3].item())
    if word != -1:
        record[3] = -1
        raise ValueError(f"line {word >> 16} (0-based), column {word & 0xFFFF}: {what}")


def _run_chunk(text: torch.Tensor, final: bool, F: int, need: int, index, parse, what: str, out, workspace, record):
    """One chunk (uint8 [nbytes], contiguous, on the device) through a format's index and parse entry points; what
    `ctr_text_chunk` documents.  index(ws, record_ptr, err, stream) and parse(ws, kept, keys, labels, line_no, record_ptr,
    err, stream) make the two library calls; `need` is the workspace size the format asks for."""
    dev = _lib.require_gpu(text)
    if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
        raise TypeError("text must be a contiguous uint8 vector")
    own = record is None
    if own:
        record = _new_record(dev)
    if workspace is None or workspace.numel() < need:
        workspace = torch.zeros(need, dtype=torch.uint8, device=dev)
    err, stream = _lib.err_word(dev).data_ptr(), _lib.stream_ptr(dev)
    index(workspace.data_ptr(), record.data_ptr(), err, stream)
    lines, kept, consumed, word = record.tolist()
    if out is None:
        out = (torch.zeros((kept, F), dtype=torch.int64, device=dev), torch.zeros(kept, dtype=torch.uint8, device=dev),
               torch.zeros(kept, dtype=torch.int64, device=dev))
    keys, labels, line_no = out
    _lib.require_gpu(text, keys, labels, line_no)
    for t, dtype, tail in ((keys, torch.int64, (F,)), (labels, torch.uint8, ()), (line_no, torch.int64, ())):
        if t.dtype != dtype or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail or t.shape[0] < kept \
                or not t.is_contiguous():
            raise ValueError(f"out must be (int64 [>= {kept}, {F}], uint8 [>= {kept}], int64 [>= {kept}]), all contiguous")
    parse(workspace.data_ptr(), kept, keys.data_ptr(), labels.data_ptr(), line_no.data_ptr(), record.data_ptr(), err, stream)
    if own or word != -1:
        _raise_refusal(record, what)
    return keys[:kept], labels[:kept], line_no[:kept], lines, consumed


def ctr_text_chunk(text: torch.Tensor, final: bool, first_line_no: int = 0, n_int: int = NUM_INT_FEATS,
                   n_cat: int = NUM_FEATS - NUM_INT_FEATS, out=None, workspace: Optional[torch.Tensor] = None,
                   record: Optional[torch.Tensor] = None):
    """One chunk of Criteo text (uint8 [nbytes], contiguous, on the device) through mi_ctr_text_index and
    mi_ctr_text_parse: (keys int64 [kept, F], labels uint8 [kept], line_no int64 [kept], lines, consumed).  `lines` is
    the chunk's number of lines and `consumed` the offset after the last of them (without `final` the bytes after the last
    newline are left to the next chunk).  out=(keys, labels, line_no): contiguous buffers of at least `kept` rows, whose
    first `kept` rows are written.

    The parse is launched BEFORE any refusal is looked at, so the index's carriage returns and the parse's offences meet in
    one minimum and the lowest (line, column) of the chunk is the one named.  record=None: the call has a record of its
    own and raises after the parse (a second read-back of one word).  record=a `_new_record`: the caller chains chunks
    in file order; the one read-back is the record after the index, which shows the refusals of the chunks before and
    this chunk's carriage returns (then the parse still runs and the merged word is raised), while a refusal of this
    chunk's parse alone stays in the record for the next chunk's read-back or the caller's last `_raise_refusal`."""
    dev = _lib.require_gpu(text)
    nbytes = text.numel()
    lib = _lib.load()
    thresholds = _thresholds_on(dev)
    need = int(lib.mi_ctr_text_workspace_bytes(nbytes, n_int, n_cat))
    if need == 0:
        raise ValueError(f"a chunk of {nbytes} bytes with {n_int} + {n_cat} columns is outside what the reader supports")

    def index(ws, rec, err, stream):
        _lib.check(lib.mi_ctr_text_index(text.data_ptr(), nbytes, int(bool(final)), n_int, n_cat, int(first_line_no), ws, rec,
                                         rec + 24, err, stream), "mi_ctr_text_index")

    def parse(ws, kept, keys, labels, line_no, rec, err, stream):
        _lib.check(lib.mi_ctr_text_parse(text.data_ptr(), nbytes, n_int, n_cat, ws, kept, int(first_line_no),
                                         thresholds.data_ptr(), thresholds.numel(), keys, labels, line_no, rec + 24, err,
                                         stream), "mi_ctr_text_parse")

    return _run_chunk(text, final, n_int + n_cat, need, index, parse, _CRITEO_REFUSAL, out, workspace, record)


# ---- delimited text by a column spec (mi_ctr_table_*; include/mi355x_recsys.h spells the kinds out) ----------------------
COL_SKIP, COL_LABEL01, COL_LABEL_COUNT, COL_TOKEN8, COL_DEC64, COL_TIME = range(6)
_KEY_KINDS = (COL_TOKEN8, COL_DEC64, COL_TIME)


class TableFormat:
    """A delimited text format: the separator, whether the file starts with a header line, one kind per file column (the
    key kinds take the output columns 0, 1, ... in file order), whether the TIME column also gives hour / weekday /
    weekend keys, and the host reader a refusal's message points at."""

    def __init__(self, sep: str, header: bool, kinds, derive_time: bool = False, host_reader: str = "the host reader"):
        self.sep, self.header, self.kinds, self.host_reader = ord(sep), bool(header), tuple(int(k) for k in kinds), host_reader
        self.derive_time = bool(derive_time) and COL_TIME in self.kinds
        self.n_cols = len(self.kinds)
        self.F = sum(k in _KEY_KINDS for k in self.kinds)
        self.F_out = self.F + (3 if self.derive_time else 0)
        spec, at = [], 0
        for k in self.kinds:
            spec.append(k | (at << 8) if k in _KEY_KINDS else k)
            at += k in _KEY_KINDS
        self.spec = np.array(spec, dtype=np.int32)
        self._on = {}
        self.refusal = (f"not in the strict grammar of the device reader (a label, token, number or timestamp its column's "
                        f"kind does not take, or a carriage return); {host_reader} is the lenient reader")

    def spec_on(self, device: torch.device) -> torch.Tensor:
        i = device.index if device.index is not None else torch.cuda.current_device()
        if i not in self._on:
            self._on[i] = torch.from_numpy(self.spec.copy()).to(torch.device("cuda", i))
        return self._on[i]



def avazu_format(preprocess_timestamp: bool = False) -> TableFormat:
    """id (never read), click, hour as yymmddHH, 21 more feature strings; a header line; comma-separated."""
    return TableFormat(",", True, [COL_SKIP, COL_LABEL01, COL_TIME] + [COL_TOKEN8] * (NUM_AVAZU_FEATS - 1),
                       preprocess_timestamp, "read_avazu_text")


def kdd_format() -> TableFormat:
    """click count, then 11 decimal ids (some above 2^63); no header; tab-separated."""
    return TableFormat("\t", False, [COL_LABEL_COUNT] + [COL_DEC64] * NUM_KDD_FEATS, False, "read_kdd_text")


def ctr_table_chunk(text: torch.Tensor, final: bool, fmt: TableFormat, first_line_no: int = 0, n_header: int = 0, out=None,
                    workspace: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None):
    """`ctr_text_chunk` for a TableFormat, through mi_ctr_table_index and mi_ctr_table_parse: (keys int64 [kept, F_out],
    labels uint8 [kept], line_no int64 [kept], lines, consumed).  n_header: 1 when the chunk starts with the file's header
    line, which is neither kept nor counted in `lines`."""
    dev = _lib.require_gpu(text)
    nbytes = text.numel()
    lib = _lib.load()
    spec = fmt.spec_on(dev)
    need = int(lib.mi_ctr_table_workspace_bytes(nbytes, fmt.n_cols))
    if need == 0:
        raise ValueError(f"a chunk of {nbytes} bytes with {fmt.n_cols} columns is outside what the reader supports")

    def index(ws, rec, err, stream):
        _lib.check(lib.mi_ctr_table_index(text.data_ptr(), nbytes, int(bool(final)), fmt.sep, fmt.n_cols, int(n_header),
                                          int(first_line_no), ws, rec, rec + 24, err, stream), "mi_ctr_table_index")

    def parse(ws, kept, keys, labels, line_no, rec, err, stream):
        _lib.check(lib.mi_ctr_table_parse(text.data_ptr(), nbytes, fmt.sep, fmt.n_cols, spec.data_ptr(), int(fmt.derive_time),
                                          ws, kept, int(first_line_no), keys, labels, line_no, rec + 24, err, stream),
                   "mi_ctr_table_parse")

    return _run_chunk(text, final, fmt.F_out, need, index, parse, fmt.refusal, out, workspace, record)


def _parse_chunks(source, device, chunk_bytes: int, F: int, need, chunk, what: str):
    """The chunk loop every device reader shares.  need(nbytes) -> workspace bytes; chunk(text, final, first_line_no,
    first, workspace, record) -> what `_run_chunk` returns (`first`: the chunk starts the file).  Returns (keys, labels,
    line_no, lines of the file)."""
    device = torch.device(device)
    if chunk_bytes < 1 or chunk_bytes > 2 ** 31 - 1:
        raise ValueError("chunk_bytes must lie in [1, 2^31 - 1]")
    parts, state = [], {"line": 0, "ws": None, "record": None, "first": True}

    def one(text: torch.Tensor, final: bool) -> int:
        size = need(text.numel())
        if state["ws"] is None or state["ws"].numel() < size:
            state["ws"] = None                                       # (released before the larger one is taken)
            state["ws"] = torch.zeros(size, dtype=torch.uint8, device=text.device)
        if state["record"] is None:
            state["record"] = _new_record(text.device)
        keys, labels, line_no, lines, consumed = chunk(text, final, state["line"], state["first"], state["ws"],
                                                       state["record"])
        parts.append((keys, labels, line_no))
        state["line"] += lines
        if consumed:
            state["first"] = False
        return consumed

    if isinstance(source, torch.Tensor) and source.is_cuda:
        if source.dtype != torch.uint8 or source.dim() != 1:
            raise TypeError("a tensor source must be a uint8 vector")
        text, at, total = source.contiguous(), 0, source.numel()
        device = text.device
        while at < total:
            final = at + chunk_bytes >= total
            consumed = one(text[at:at + chunk_bytes], final)
            if consumed == 0:
                raise ValueError(f"a line is longer than chunk_bytes = {chunk_bytes}")
            at += consumed
    else:
        if isinstance(source, (str, os.PathLike)):
            f = open(source, "rb", buffering=0)
            status = os.fstat(f.fileno())
            total = status.st_size if stat.S_ISREG(status.st_mode) else None      # (a pipe's size says nothing)
        else:
            if isinstance(source, torch.Tensor):
                if source.dtype != torch.uint8 or source.dim() != 1:
                    raise TypeError("a tensor source must be a uint8 vector")
                source = source.contiguous().numpy()
            f = _ViewReader(source)
            total = len(f.view)
        with f:
            for chunk_view, final in _cut_chunks(f.readinto, chunk_bytes, total):
                one(torch.frombuffer(chunk_view, dtype=torch.uint8).to(device), final)
    if parts:
        _raise_refusal(state["record"], what)
    if not parts:
        keys = torch.zeros((0, F), dtype=torch.int64, device=device)
        _lib.require_gpu(keys)
        return (keys, torch.zeros(0, dtype=torch.uint8, device=device), torch.zeros(0, dtype=torch.int64, device=device),
                state["line"])
    if len(parts) == 1:
        return parts[0] + (state["line"],)
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3)) + (state["line"],)


def parse_criteo_text(source, device="cuda", chunk_bytes: int = 1 << 28, n_int: int = NUM_INT_FEATS,
                      n_cat: int = NUM_FEATS - NUM_INT_FEATS) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`read_criteo_text` on the device: (keys int64 [n, n_int + n_cat], labels uint8 [n], line_no int64 [n]), all on
    `device`, equal element for element to the host reader's on every file both accept.  The device enforces the grammar
    of include/mi355x_recsys.h strictly and raises ValueError, naming the lowest offending line and column, where
    `read_criteo_text` would be lenient; it never returns keys that differ from the host's.

    source: a path, a bytes-like object, or a uint8 tensor on the host or the device.  Host sources are read in chunks of
    at most `chunk_bytes`, each cut after its last newline (host memory stays O(chunk_bytes), no Python object per line);
    a device tensor is walked in place.  The result does not depend on `chunk_bytes`; a line longer than it is a
    ValueError.  The only read-back per chunk is the record {lines, kept, consumed, refusal}, plus one word at the end;
    the record belongs to the call, so concurrent calls share nothing but the read-only threshold table."""
    if n_int < 0 or n_cat < 0:
        raise ValueError("n_int and n_cat must not be negative")

    def need(nbytes):
        return int(_lib.load().mi_ctr_text_workspace_bytes(nbytes, n_int, n_cat))

    def chunk(text, final, line, first, ws, record):
        return ctr_text_chunk(text, final, line, n_int, n_cat, workspace=ws, record=record)

    return _parse_chunks(source, device, chunk_bytes, n_int + n_cat, need, chunk, _CRITEO_REFUSAL)[:3]


def parse_table_text(source, fmt: TableFormat, device="cuda", chunk_bytes: int = 1 << 28):
    """A TableFormat's text through the chunk loop of `parse_criteo_text` (the same sources, chunking and refusal rule):
    (keys int64 [n, F_out], labels uint8 [n], line_no int64 [n], the file's number of lines after the header)."""

    def need(nbytes):
        return int(_lib.load().mi_ctr_table_workspace_bytes(nbytes, fmt.n_cols))

    def chunk(text, final, line, first, ws, record):
        return ctr_table_chunk(text, final, fmt, line, int(fmt.header and first), workspace=ws, record=record)

    return _parse_chunks(source, device, chunk_bytes, fmt.F_out, need, chunk, fmt.refusal)


def parse_avazu_text(source, device="cuda", chunk_bytes: int = 1 << 28,
                     preprocess_timestamp: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`read_avazu_text` on the device: (keys int64 [n, 22 or 25], labels uint8 [n], line_no int64 [n]) of Avazu's
    comma-separated text, equal element for element to the host reader's on every file both accept; sources, chunking and
    refusals as `parse_criteo_text`.  The header is dropped, a line without 24 values is skipped yet numbered, the `id`
    column is never read.  With `preprocess_timestamp` the hour column must be 8 digits of a real date and hour."""
    return parse_table_text(source, avazu_format(preprocess_timestamp), device, chunk_bytes)[:3]


def parse_kdd_text(source, device="cuda", chunk_bytes: int = 1 << 28) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`read_kdd_text` on the device: (keys int64 [n, 11], labels uint8 [n], line_no int64 [n]) of KDD 2012 track 2's
    tab-separated text; sources, chunking and refusals as `parse_criteo_text`.  A line without 12 values is a ValueError
    naming it (the reference asserts the count)."""
    keys, labels, line_no, lines = parse_table_text(source, kdd_format(), device, chunk_bytes)
    n = line_no.numel()
    if n != lines:                                          # the first position whose line number is not its own index
        own = torch.arange(n, dtype=torch.int64, device=line_no.device)
        first = int(torch.where(line_no != own, own, n).min().item()) if n else 0
        raise ValueError(f"line {first} (0-based) does not hold {NUM_KDD_FEATS + 1} tab-separated values; "
                         "read_kdd_text refuses it too")
    return keys, labels, line_no


class _ViewReader:
    """`readinto` over any bytes-like object."""

    def __init__(self, source):
        self.view, self.at = memoryview(source).cast("B"), 0

    def readinto(self, buffer) -> int:
        n = min(len(buffer), len(self.view) - self.at)
        buffer[:n] = self.view[self.at:self.at + n]
        self.at += n
        return n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.view.release()


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
                         device="cuda", reader: str = "host") -> "DeviceCTRDataset":
        """The whole file encoded (the vocabulary counts every line, as the reference's cache does); with `train_test_info`
        (the reference's `torch.load`-able dict, or the dict itself) the dataset is the view over `dataset_name`'s line
        numbers, sorted as the reference sorts them.  reader: "host" reads the text with `read_criteo_text`, "device"
        with `parse_criteo_text` (the same keys, strict about the grammar), whose tensors never leave the device."""
        _check_reader(reader)
        if reader == "device":
            keys, labels, line_no = parse_criteo_text(path, device=device)
        else:
            keys, labels, line_no = read_criteo_text(path)
        return cls._from_keys(keys, labels, line_no, train_test_info, dataset_name, min_threshold, device)

    @classmethod
    def from_avazu_text(cls, path: str, train_test_info=None, dataset_name: Optional[str] = None, min_threshold: int = 2,
                        device="cuda", reader: str = "device",
                        preprocess_timestamp: Optional[bool] = None) -> "DeviceCTRDataset":
        """`from_criteo_text` for Avazu's file (`parse_avazu_text` / `read_avazu_text`; 22 fields, 25 with the timestamp
        features).  train_test_info: the reference's `train_test_info.bin` (a path, or the dict) or what
        `make_train_test_info` returns.  preprocess_timestamp=None takes the info's metadata entry, else False."""
        _check_reader(reader)
        info = _load_info(train_test_info)
        if preprocess_timestamp is None:
            preprocess_timestamp = bool((info or {}).get("metadata", {}).get("preprocess_timestamp", False))
        if reader == "device":
            keys, labels, line_no = parse_avazu_text(path, device=device, preprocess_timestamp=preprocess_timestamp)
        else:
            keys, labels, line_no = read_avazu_text(path, preprocess_timestamp)
        return cls._from_keys(keys, labels, line_no, info, dataset_name, min_threshold, device)

    @classmethod
    def from_kdd_text(cls, path: str, train_test_info=None, dataset_name: Optional[str] = None, min_threshold: int = 10,
                      device="cuda", reader: str = "device") -> "DeviceCTRDataset":
        """`from_criteo_text` for KDD 2012 track 2's file (`parse_kdd_text` / `read_kdd_text`; 11 fields)."""
        _check_reader(reader)
        if reader == "device":
            keys, labels, line_no = parse_kdd_text(path, device=device)
        else:
            keys, labels, line_no = read_kdd_text(path)
        return cls._from_keys(keys, labels, line_no, train_test_info, dataset_name, min_threshold, device)

    @classmethod
    def _from_keys(cls, keys, labels, line_no, train_test_info, dataset_name, min_threshold, device) -> "DeviceCTRDataset":
        """The tail every `from_*_text` shares: encode the key matrix, resolve `dataset_name`'s line numbers to record rows
        (on the device when `line_no` is there)."""
        records, field_dims = encode_ctr_columns(keys, labels, min_threshold, device)
        index = None
        if train_test_info is not None:
            info = _load_info(train_test_info)
            lines = np.sort(np.asarray(list(info[dataset_name]), dtype=np.int64))
            missing = f"{dataset_name!r} names a line the file does not hold (or one that was skipped)"
            if isinstance(line_no, torch.Tensor):
                wanted = torch.from_numpy(lines).to(line_no.device)
                index = torch.searchsorted(line_no, wanted)
                if lines.size and (line_no.numel() == 0 or not torch.equal(
                        line_no[index.clamp(max=line_no.numel() - 1)], wanted)):
                    raise ValueError(missing)
            else:
                index = np.searchsorted(line_no, lines)
                if lines.size and (index.max() >= line_no.size or not np.array_equal(line_no[index], lines)):
                    raise ValueError(missing)
                index = torch.from_numpy(index)
        return cls(records, field_dims, index=index, device=device)


def _check_reader(reader: str) -> None:
    if reader not in ("host", "device"):
        raise ValueError(f"reader must be 'host' or 'device'; got {reader!r}")


def _load_info(train_test_info):
    """The reference's `torch.load`-able split file, or the dict itself (None stays None)."""
    if train_test_info is None or isinstance(train_test_info, dict):
        return train_test_info
    return torch.load(train_test_info, weights_only=False)


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

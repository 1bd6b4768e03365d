"""A bytes / Python restatement of the strict Criteo text grammar of include/mi355x_recsys.h (written from the header, not
from csrc/ctr_text.hip), generators of Criteo-format text, and the host reader applied to texts of other column counts.

    lines     ended by '\n'; a non-empty run after the last '\n' is a line; numbered from 0, skipped ones included; a line
              whose tab count is not n_int + n_cat is skipped; a '\r' anywhere is refused
    label     exactly b"0" or b"1"
    integer   empty -> -2^63; else optional '-' and 1..18 decimal digits -> v; key v - 2 for v <= 2, else int(log(v)^2)
    category  empty -> -1; else 1..15 hexadecimal digits of either case
    refusal   the lowest offending (line, column)
"""
import math
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLE = os.path.join(GOLDEN, "criteo_sample.txt")
NULL_KEY, EMPTY_KEY = -(1 << 63), -1
HOST_INT, HOST_CAT = 13, 26              # the column counts `read_criteo_text` is written for

INTEGER = re.compile(rb"-?[0-9]{1,18}\Z")
CATEGORY = re.compile(rb"[0-9a-fA-F]{1,15}\Z")


class Refused(ValueError):
    def __init__(self, line, column):
        super().__init__(f"line {line}, column {column}")
        self.line, self.column = line, column


def split_lines(data: bytes):
    lines = bytes(data).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def parse_reference(data: bytes, n_int: int = HOST_INT, n_cat: int = HOST_CAT):
    """(keys int64 [n, n_int + n_cat], labels uint8 [n], line_no int64 [n]) under the strict grammar; Refused(line, column)
    for the lowest offence."""
    F = n_int + n_cat
    rows, labels, line_no, refusals = [], [], [], []
    for idx, line in enumerate(split_lines(data)):
        if b"\r" in line:
            refusals.append((idx, min(line[:line.index(b"\r")].count(b"\t"), 65535)))
        fields = line.split(b"\t")
        if len(fields) != F + 1:
            continue
        row = []
        if fields[0] not in (b"0", b"1"):
            refusals.append((idx, 0))
        for c, s in enumerate(fields[1:], 1):
            if s == b"":
                row.append(NULL_KEY if c <= n_int else EMPTY_KEY)
            elif c <= n_int and INTEGER.match(s):
                v = int(s)
                row.append(v - 2 if v <= 2 else int(math.log(v) ** 2))
            elif c > n_int and CATEGORY.match(s):
                row.append(int(s, 16))
            else:
                refusals.append((idx, c))
                row.append(0)
        rows.append(row)
        labels.append(1 if fields[0] == b"1" else 0)
        line_no.append(idx)
    if refusals:
        raise Refused(*min(refusals))
    return (np.array(rows, dtype=np.int64).reshape(len(rows), F), np.array(labels, dtype=np.uint8),
            np.array(line_no, dtype=np.int64))


def host_reader(data: bytes, n_int: int, n_cat: int, tmp_dir):
    """`read_criteo_text` on `data` read as a text of n_int + n_cat columns: every kept line gets the 13 - n_int integer
    and 26 - n_cat categorical columns it lacks as empty fields, every other line the same number of tabs at its end (its
    count stays wrong), the file goes through the host reader unchanged, and the added columns are dropped."""
    from recsys_benchmark_amd import read_criteo_text

    assert n_int <= HOST_INT and n_cat <= HOST_CAT
    data = bytes(data)
    if (n_int, n_cat) != (HOST_INT, HOST_CAT):
        F, more = n_int + n_cat, (HOST_INT - n_int) + (HOST_CAT - n_cat)
        out = []
        for line in split_lines(data):
            fields = line.split(b"\t")
            if len(fields) == F + 1:
                fields = fields[:1 + n_int] + [b""] * (HOST_INT - n_int) + fields[1 + n_int:] + [b""] * (HOST_CAT - n_cat)
                out.append(b"\t".join(fields))
            else:
                out.append(line + b"\t" * more)
        data = b"\n".join(out) + (b"\n" if data.endswith(b"\n") else b"")
    path = os.path.join(str(tmp_dir), "host_reader.txt")
    with open(path, "wb") as f:
        f.write(data)
    keys, labels, line_no = read_criteo_text(path)
    columns = list(range(n_int)) + list(range(HOST_INT, HOST_INT + n_cat))
    return np.ascontiguousarray(keys[:, columns]), labels, line_no


def generate_text(seed: int, n_lines: int, n_int: int = HOST_INT, n_cat: int = HOST_CAT, holes: float = 0.0,
                  final_newline: bool = True) -> bytes:
    """Seeded Criteo-format text in the strict grammar: integer fields empty (25 %), negative (5 %) or drawn over many
    magnitudes, with the odd leading zero; categorical fields empty (10 %) or 8 hex digits from a small pool, some in
    upper case.  `holes`: the share of lines replaced by an empty line or one with a tab too few or too many."""
    rng = np.random.default_rng(seed)
    pool = [b"%08x" % int(v) for v in rng.integers(0, 1 << 32, 50)]
    lines = []
    for _ in range(n_lines):
        fields = [b"1" if rng.random() < 0.25 else b"0"]
        for _ in range(n_int):
            u = rng.random()
            if u < 0.25:
                fields.append(b"")
            elif u < 0.30:
                fields.append(b"-%d" % int(rng.integers(0, 4)))
            else:
                v = int(10 ** (rng.random() * 7)) - 1
                fields.append((b"0%d" if rng.random() < 0.02 else b"%d") % v)
        for _ in range(n_cat):
            u = rng.random()
            s = b"" if u < 0.10 else pool[int(rng.integers(0, len(pool)))]
            fields.append(s.upper() if u > 0.97 else s)
        line = b"\t".join(fields)
        if rng.random() < holes:
            line = [b"", line + b"\t", line.rsplit(b"\t", 1)[0], b"no tabs here"][int(rng.integers(0, 4))]
        lines.append(line)
    return b"\n".join(lines) + (b"\n" if final_newline and lines else b"")

"""A bytes / Python restatement of the column-spec text grammar of include/mi355x_recsys.h (written from the header, not
from csrc/ctr_text.hip), the Avazu and KDD column lists, and seeded generators of text in both formats.

    lines        ended by '\n'; a non-empty run after the last '\n' is a line; the first `n_header` lines are dropped and
                 not counted; the others are numbered from 0, skipped ones included; a line that does not split into
                 len(kinds) fields is skipped; a '\r' anywhere is refused (in the header: as line 0)
    SKIP         never read
    LABEL01      exactly b"0" or b"1"
    LABEL_COUNT  1..18 decimal digits -> value >= 1
    TOKEN8       0..8 bytes in 0x21..0x7E -> the bytes big-endian, zero-padded at the low end, as int64
    DEC64        1..20 digits, canonical, <= 2^64 - 1 -> the 64-bit pattern as int64
    TIME         a TOKEN8; with derive_time exactly 8 digits yymmddHH of a real date and hour, and three more keys after
                 the F others: hour, weekday (Monday 0, by days-from-civil), weekday >= 5
    refusal      the lowest offending (line, column)
"""
import os
import re

import numpy as np

from ctr_text_helpers import Refused, split_lines

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AVAZU_SAMPLE = os.path.join(GOLDEN, "avazu_sample.csv")
AVAZU_GOLDEN = os.path.join(GOLDEN, "avazu_vocab.npz")
AVAZU_HEADER = (b"id,click,hour,C1,banner_pos,site_id,site_domain,site_category,app_id,app_domain,app_category,device_id,"
                b"device_ip,device_model,device_type,device_conn_type,C14,C15,C16,C17,C18,C19,C20,C21")

SKIP, LABEL01, LABEL_COUNT, TOKEN8, DEC64, TIME = range(6)
AVAZU_KINDS = (SKIP, LABEL01, TIME) + (TOKEN8,) * 21
KDD_KINDS = (LABEL_COUNT,) + (DEC64,) * 11

COUNT = re.compile(rb"[0-9]{1,18}\Z")
TOKEN = re.compile(rb"[\x21-\x7e]{0,8}\Z")
DECIMAL = re.compile(rb"(0|[1-9][0-9]{0,19})\Z")
STAMP = re.compile(rb"[0-9]{8}\Z")


def s64(v: int) -> int:
    return ((v + (1 << 63)) % (1 << 64)) - (1 << 63)


def token_key(s: bytes) -> int:
    return s64(int.from_bytes(s.ljust(8, b"\0"), "big"))


def days_from_civil(y: int, m: int, d: int) -> int:
    """Days since 1970-01-01 of the proleptic Gregorian date, in integers."""
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def weekday(y: int, m: int, d: int) -> int:
    return (days_from_civil(y, m, d) + 3) % 7              # 1970-01-01 was a Thursday; Monday is 0


def derive(stamp: bytes):
    """(hour, weekday, weekend) of b"yymmddHH", or None where the device refuses it."""
    if not STAMP.match(stamp):
        return None
    yy, mm, dd, hh = (int(stamp[i:i + 2]) for i in (0, 2, 4, 6))
    year = 2000 + yy if yy <= 68 else 1900 + yy
    leap = (year % 4 == 0 and year % 100 != 0) or year % 400 == 0
    month_days = (31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
    if not 1 <= mm <= 12 or not 1 <= dd <= month_days[mm - 1] or hh > 23:
        return None
    w = weekday(year, mm, dd)
    return hh, w, int(w >= 5)


def parse_reference(data: bytes, sep: bytes, n_header: int, kinds, derive_time: bool = False):
    """(keys int64 [n, F_out], labels uint8 [n], line_no int64 [n]) under the strict grammar; Refused(line, column) for
    the lowest offence."""
    timed = derive_time and TIME in kinds
    F = sum(k in (TOKEN8, DEC64, TIME) for k in kinds)
    F_out = F + (3 if timed else 0)
    rows, labels, line_no, refusals = [], [], [], []
    for at, line in enumerate(split_lines(data)):
        idx = max(at - n_header, 0)
        if b"\r" in line:
            refusals.append((idx, min(line[:line.index(b"\r")].count(sep), 65535)))
        fields = line.split(sep)
        if at < n_header or len(fields) != len(kinds):
            continue
        row, extra, label = [], [0, 0, 0], 0
        for c, (kind, s) in enumerate(zip(kinds, fields)):
            good, key = True, 0
            if kind == LABEL01:
                good = s in (b"0", b"1")
                label = int(s == b"1")
            elif kind == LABEL_COUNT:
                good = bool(COUNT.match(s))
                label = int(good and int(s) >= 1)
            elif kind == DEC64:
                good = bool(DECIMAL.match(s)) and int(s) < 1 << 64
                key = s64(int(s)) if good else 0
            elif kind in (TOKEN8, TIME):
                good = bool(TOKEN.match(s))
                key = token_key(s) if good else 0
                if kind == TIME and timed:
                    got = derive(s)
                    good = got is not None
                    key, extra = (key, list(got)) if good else (0, [0, 0, 0])
            if not good:
                refusals.append((idx, c))
            if kind in (TOKEN8, DEC64, TIME):
                row.append(key)
        rows.append(row + (extra if timed else []))
        labels.append(label)
        line_no.append(idx)
    if refusals:
        raise Refused(*min(refusals))
    return (np.array(rows, dtype=np.int64).reshape(len(rows), F_out), np.array(labels, dtype=np.uint8),
            np.array(line_no, dtype=np.int64))


def avazu_reference(data: bytes, preprocess_timestamp: bool = False):
    return parse_reference(data, b",", 1, AVAZU_KINDS, preprocess_timestamp)


def kdd_reference(data: bytes):
    return parse_reference(data, b"\t", 0, KDD_KINDS)


def write(tmp_dir, data: bytes, name: str = "table.txt") -> str:
    path = os.path.join(str(tmp_dir), name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def avazu_line(rng, pool, id_digits: int = 19) -> bytes:
    """One line in Avazu's schema: a long decimal id, the label, a real yymmddHH, then 21 fields that are 8-digit hex ids
    from `pool`, short decimals (-1 among them) or, now and then, empty or of any length from 1 to 8."""
    fields = [b"%d" % int(rng.integers(1, 10)) + b"".join(b"%d" % int(d) for d in rng.integers(0, 10, id_digits - 1)),
              b"1" if rng.random() < 0.2 else b"0",
              b"1410%02d%02d" % (int(rng.integers(1, 32)), int(rng.integers(0, 24)))]
    for c in range(21):
        u = rng.random()
        if u < 0.03:
            fields.append(b"")
        elif u < 0.08:
            fields.append(b"Zq-_~!x9"[:int(rng.integers(1, 9))])
        elif c in (2, 3, 4, 5, 6, 7, 8, 9, 10):
            fields.append(pool[int(rng.integers(0, len(pool)))])
        else:
            fields.append(b"%d" % int(rng.integers(-1, 3000)))
    return b",".join(fields)


def generate_avazu(seed: int, n_lines: int, holes: float = 0.0, final_newline: bool = True, header: bool = True) -> bytes:
    """Seeded Avazu text in the strict grammar.  `holes`: the share of lines replaced by an empty line or one with a value
    too few or too many."""
    rng = np.random.default_rng(seed)
    pool = [b"%08x" % int(v) for v in rng.integers(0, 1 << 32, 40)]
    lines = [AVAZU_HEADER] if header else []
    for _ in range(n_lines):
        line = avazu_line(rng, pool, 19 + int(rng.integers(0, 2)))
        if rng.random() < holes:
            line = [b"", line + b",", line.rsplit(b",", 1)[0], b"no commas here"][int(rng.integers(0, 4))]
        lines.append(line)
    return b"\n".join(lines) + (b"\n" if final_newline and lines else b"")


def generate_kdd(seed: int, n_lines: int, final_newline: bool = True) -> bytes:
    """Seeded KDD 2012 track 2 text: a click count, then 11 canonical decimals of every magnitude up to 2^64 - 1."""
    rng = np.random.default_rng(seed)
    pool = [int(v) for v in rng.integers(0, 1 << 64, 30, dtype=np.uint64)]
    lines = []
    for _ in range(n_lines):
        fields = [b"%d" % int(rng.integers(0, 3) * rng.integers(0, 40))]
        for _ in range(11):
            u = rng.random()
            v = pool[int(rng.integers(0, len(pool)))] if u < 0.3 else int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63))
            fields.append(b"%d" % v)
        lines.append(b"\t".join(fields))
    return b"\n".join(lines) + (b"\n" if final_newline and lines else b"")

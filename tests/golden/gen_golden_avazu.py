#!/usr/bin/env python3
"""Write the synthetic tests/golden/avazu_sample.csv and record tests/golden/avazu_vocab.npz from the REFERENCE's own
`_create_binary` (src/dataset/avazu/avazu_on_ram.py) and `run_timestamp_preprocess` (src/dataset/avazu/utils.py) over it.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_avazu.py

Same conventions as gen_golden_ctr_data.py: the reference's modules are imported unmodified (`loguru`, `lmdb` and `tqdm`
replaced by stand-ins), only arrays and the sample leave this script, and the archive is written with a fixed member
timestamp.

avazu_sample.csv — seeded, in Avazu's schema: a header and 150 lines; 8-digit lower-case hex ids from small pools (so
thresholds 1, 2 and 3 cut differently), decimal C* fields with -1 among them, two empty fields, 19- and 20-digit ids,
three lines with 23 or 25 values, one empty line, hours over six days (a Saturday and a Sunday, the 00 and 23 hours).

avazu_vocab.npz:
  line_no                     int64 [n]: the kept lines' indices after the header (what `_create_binary` collects);
  labels                      uint8 [n];
  field_dims_t{T}_ts{0|1}     int64 [22 | 25]: len(feat_mapper[i]) + 1, for min_threshold T in 1, 2, 3;
  oov_t{T}_ts{0|1}            bool [n, 22 | 25]: the line's feature string is not in feat_mapper[i];
  derived                     int64 [n, 3]: run_timestamp_preprocess's three strings per kept line, as integers
                              (hour, weekday, "True" -> 1 / "False" -> 0);
  {train|val|test}_s{0|1}_seed{2023|7}   int64: the three lists for both split strategies and two seeds;
  date_text                   uint8 [24, 8]: yymmddHH for the dates 000229, 160229, 170228, 681231, 690101, 991231, 000101
                              and 141021 at the hours 00, 12 and 23;
  date_derived                int64 [24, 3]: run_timestamp_preprocess of each, as integers.
"""
import io
import os
import sys
import types
import zipfile

import numpy as np

REF = os.environ.get("RECSYS_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "src")):
    sys.exit("set RECSYS_REFERENCE to a checkout of the reference (the directory that holds src/ and tests/)")
OUT = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = (1, 2, 3)
HEADER = ("id,click,hour,C1,banner_pos,site_id,site_domain,site_category,app_id,app_domain,app_category,device_id,device_ip,"
          "device_model,device_type,device_conn_type,C14,C15,C16,C17,C18,C19,C20,C21")
DATES = ("000229", "160229", "170228", "681231", "690101", "991231", "000101", "141021")


def _install_stubs():
    class _L:
        def __getattr__(self, k):
            return lambda *a, **kw: None

    class _Bar:
        def __init__(self, it, **kw):
            self.it = it

        def __iter__(self):
            return iter(self.it)

        def set_description(self, *a, **kw):
            pass

    loguru = types.ModuleType("loguru")
    loguru.logger = _L()
    loguru.Logger = _L
    sys.modules["loguru"] = loguru
    sys.modules["lmdb"] = types.ModuleType("lmdb")
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = _Bar
    sys.modules["tqdm"] = tqdm


_install_stubs()
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from src.dataset.avazu.avazu_on_ram import _create_binary  # noqa: E402
from src.dataset.avazu.utils import run_timestamp_preprocess  # noqa: E402


def save(name, **arrays):
    """np.savez_compressed, but every member stamped 1980-01-01 so that the archive bytes depend on the arrays only."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f"  wrote {name}.npz ({len(arrays)} arrays, {os.path.getsize(path)} bytes)")


def write_sample(path):
    rng = np.random.default_rng(20141021)
    hexpool = {c: ["%08x" % int(v) for v in rng.integers(0, 1 << 32, size)]
               for c, size in zip(range(5, 14), (6, 5, 4, 8, 5, 4, 40, 60, 12))}
    days = ("141021", "141022", "141024", "141025", "141026", "141030")          # Tue, Wed, Fri, Sat, Sun, Thu
    cpool = {3: ["1005", "1002", "1010"], 4: ["0", "1", "7"], 14: ["1", "0", "4", "5"], 15: ["0", "2", "3"],
             16: ["15706", "15704", "18993", "20362", "21611", "4687"], 17: ["320", "300", "216"], 18: ["50", "250", "36"],
             19: ["1722", "1800", "2161", "2333", "423"], 20: ["0", "3", "2", "1"], 21: ["35", "39", "167", "1327"],
             22: ["-1", "100084", "100148", "100111"], 23: ["79", "157", "23", "61", "221"]}
    lines = []
    for i in range(150):
        hour = (0, 23)[i % 2] if i < 8 else int(rng.integers(0, 24))
        digits = 20 if i % 3 == 0 else 19
        row = [str(int(rng.integers(1, 10))) + "".join(str(int(d)) for d in rng.integers(0, 10, digits - 1)),
               "1" if rng.random() < 0.2 else "0", days[int(rng.integers(0, len(days)))] + "%02d" % hour]
        for c in range(3, 24):
            pool = hexpool.get(c) or cpool[c]
            # a skewed draw: the head of a pool is seen often, its tail once or twice
            row.append(pool[min(int(rng.exponential(len(pool) / 3.0)), len(pool) - 1)])
        lines.append(row)
    lines[17][8] = ""                                      # an empty app_id
    lines[90][13] = ""                                     # an empty device_model
    text = [",".join(r) for r in lines]
    text[30] = ",".join(lines[30][:-1])                    # 23 values
    text[31] = ",".join(lines[31] + ["7"])                 # 25 values
    text[120] = ",".join(lines[120][:-1])                  # 23 values
    text[77] = ""                                          # an empty line
    with open(path, "w", newline="\n") as f:
        f.write(HEADER + "\n" + "\n".join(text) + "\n")
    print(f"  wrote {os.path.basename(path)} ({len(text)} lines after the header, {os.path.getsize(path)} bytes)")


def as_integers(extra):
    hour, weekday, weekend = extra
    assert weekend in ("True", "False")
    return [int(hour), int(weekday), int(weekend == "True")]


def main():
    path = os.path.join(OUT, "avazu_sample.csv")
    write_sample(path)
    kept = []                                              # (line index after the header, its 24 values)
    with open(path) as f:
        f.readline()
        for idx, line in enumerate(f):
            values = line.rstrip("\n").split(",")
            if len(values) == 24:
                kept.append((idx, values))
    arrays = {"derived": np.array([as_integers(run_timestamp_preprocess(v)) for _, v in kept], dtype=np.int64),
              "labels": np.array([int(v[1]) for _, v in kept], dtype=np.uint8)}
    for T in THRESHOLDS:
        for ts in (0, 1):
            info = _create_binary(path, min_threshold=T, preprocess_timestamp=bool(ts))
            F = 22 + 3 * ts
            mapper = info["feat_mapper"]
            assert sorted(mapper) == list(range(1, F + 1))
            arrays[f"field_dims_t{T}_ts{ts}"] = np.array([len(mapper[i]) + 1 for i in range(1, F + 1)], dtype=np.int64)
            oov = np.zeros((len(kept), F), dtype=bool)
            for r, (_, values) in enumerate(kept):
                feats = values[2:] + (run_timestamp_preprocess(values) if ts else [])
                oov[r] = [feats[i - 1] not in mapper[i] for i in range(1, F + 1)]
            arrays[f"oov_t{T}_ts{ts}"] = oov
            print(f"  threshold {T}, timestamp {ts}: sum of field_dims {int(arrays[f'field_dims_t{T}_ts{ts}'].sum())}, "
                  f"OOV share {oov.mean():.3f}")
    for strategy in (0, 1):
        for seed in (2023, 7):
            info = _create_binary(path, seed=seed, split_strategy=strategy)
            for name in ("train", "val", "test"):
                arrays[f"{name}_s{strategy}_seed{seed}"] = np.array(list(info[name]), dtype=np.int64)
    got = sorted(sum((arrays[f"{name}_s1_seed2023"].tolist() for name in ("train", "val", "test")), []))
    assert got == [idx for idx, _ in kept]
    arrays["line_no"] = np.array([idx for idx, _ in kept], dtype=np.int64)
    texts = [d + "%02d" % h for d in DATES for h in (0, 12, 23)]
    arrays["date_text"] = np.array([list(t.encode()) for t in texts], dtype=np.uint8)
    arrays["date_derived"] = np.array([as_integers(run_timestamp_preprocess([None, None, t])) for t in texts], dtype=np.int64)
    save("avazu_vocab", **arrays)


if __name__ == "__main__":
    main()

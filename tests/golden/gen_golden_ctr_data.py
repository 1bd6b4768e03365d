#!/usr/bin/env python3
"""Generate tests/golden/ctr_data_vocab.npz by IMPORTING THE REFERENCE's CriteoDataset, and copy the reference's
100-line Criteo sample (a data file) to tests/golden/criteo_sample.txt.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_ctr_data.py

Same conventions as gen_golden_cf_data.py: the reference's modules are imported unmodified (`loguru` and `lmdb`
replaced by stand-ins, `tqdm` too where it is not installed), only arrays leave this script, and the archive is
written with a fixed member timestamp.

ctr_data_vocab.npz — for min_threshold T in 1, 2, 3, 10, over tests/assets/train_criteo_sample.txt:
  rows_t{T}        uint32 [100, 40]: the records `__yield_buffer` writes under the mapper `__get_feat_mapper` built
                   (both name-mangled methods called on an object made with object.__new__: no LMDB is opened);
  field_dims_t{T}  uint32 [39]: len(feat_mapper[i]) + 1, as `__build_cache` stores it;
  defaults_t{T}    int64 [39]: the out-of-vocabulary id per field;
  line_no          int64 [100]: the LMDB key (the line's index in the file) of every record.
The kept ids follow Python's set-iteration order: the tests compare them up to a bijection per field.
"""
import io
import os
import shutil
import struct
import sys
import types
import zipfile

import numpy as np

REF = os.environ.get("RECSYS_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "src")):
    sys.exit("set RECSYS_REFERENCE to a checkout of the reference (the directory that holds src/ and tests/)")
OUT = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = (1, 2, 3, 10)


def _install_stubs():
    class _L:
        def __getattr__(self, k):
            return lambda *a, **kw: None

    loguru = types.ModuleType("loguru")
    loguru.logger = _L()
    loguru.Logger = _L
    sys.modules["loguru"] = loguru
    sys.modules["lmdb"] = types.ModuleType("lmdb")
    try:
        import tqdm  # noqa: F401
    except ImportError:
        class _Bar:
            def __init__(self, it, **kw):
                self.it = it

            def __iter__(self):
                return iter(self.it)

            def set_description(self, *a, **kw):
                pass

        mod = types.ModuleType("tqdm")
        mod.tqdm = _Bar
        sys.modules["tqdm"] = mod


_install_stubs()
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from src.dataset.criteo.criteo_torchfm import CriteoDataset  # noqa: E402


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


def main():
    path = os.path.join(REF, "tests", "assets", "train_criteo_sample.txt")
    arrays = {}
    for T in THRESHOLDS:
        ds = object.__new__(CriteoDataset)
        ds.NUM_FEATS, ds.NUM_INT_FEATS, ds.min_threshold = 39, 13, T
        feat_mapper, defaults = ds._CriteoDataset__get_feat_mapper(path)
        field_dims = np.zeros(ds.NUM_FEATS, dtype=np.uint32)
        for i, fm in feat_mapper.items():
            field_dims[i - 1] = len(fm) + 1
        keys, rows = [], []
        for buffer in ds._CriteoDataset__yield_buffer(path, feat_mapper, defaults):
            for key, value in buffer:              # (the generator clears the list it yielded when it resumes)
                keys.append(struct.unpack(">I", key)[0])
                rows.append(np.frombuffer(value, dtype=np.uint32).copy())
        arrays[f"rows_t{T}"] = np.stack(rows)
        arrays[f"field_dims_t{T}"] = field_dims
        arrays[f"defaults_t{T}"] = np.array([defaults[i] for i in range(1, ds.NUM_FEATS + 1)], dtype=np.int64)
        arrays["line_no"] = np.array(keys, dtype=np.int64)
        oov = (arrays[f"rows_t{T}"][:, 1:] == arrays[f"defaults_t{T}"]).mean()
        print(f"  threshold {T}: sum of field_dims {int(field_dims.sum())}, OOV share {oov:.3f}")
    save("ctr_data_vocab", **arrays)
    shutil.copyfile(path, os.path.join(OUT, "criteo_sample.txt"))
    print("  copied criteo_sample.txt")


if __name__ == "__main__":
    main()

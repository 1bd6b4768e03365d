#!/usr/bin/env python3
"""Generate tests/golden/cf_data_sample.npz by IMPORTING THE REFERENCE's CFGraphDataset / TestCFGraphDataset.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_cf_data.py

Same conventions as gen_golden_mag_prune.py: the reference's modules are imported unmodified (`loguru` replaced by a
no-op stand-in), only arrays leave this script, and the archive is written with a fixed member timestamp.

cf_data_sample.npz — the reference's datasets over its own tests/assets/sample_cf.txt (which holds one duplicated
interaction, user 2 / item 79: kept, it separates the stored lists from the distinct ones):
  pair_user / pair_item: `_user_item_pairs` in order;  users: `_users`;  num_users, num_items, per_user_num;
  len_uniform / len_popularity: `len()` under the two sampling methods;  for both adjacency styles the normalised
  adjacency is NOT stored (tests compare with the package's graph_utils, which test_lightgcn_gpu.py pins to the
  reference through cf_sample_adj.npz);  test_users / test_len: TestCFGraphDataset's `_users` and `len()`;
  truth_crow / truth_col: its `_idx_to_set`, every set ascending, as a CSR over the users.
The ranking-metric values of the reference (`get_ndcg_recall` for a fixed prediction tensor) are those of metrics.npz,
written by gen_golden.py: the tests of the metric kernel read them there.
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


def _install_stubs():
    class _L:
        def __getattr__(self, k):
            return lambda *a, **kw: None

    loguru = types.ModuleType("loguru")
    loguru.logger = _L()
    loguru.Logger = _L
    sys.modules["loguru"] = loguru
    sys.modules.setdefault("lmdb", types.ModuleType("lmdb"))


_install_stubs()
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from src.dataset.cf_graph_dataset import CFGraphDataset, TestCFGraphDataset  # noqa: E402


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
    path = os.path.join(REF, "tests", "assets", "sample_cf.txt")
    uni = CFGraphDataset(path, sampling_method="uniform")
    pop = CFGraphDataset(path, sampling_method="popularity", num_neg_item=3)
    pairs = np.array(uni._user_item_pairs, dtype=np.int64)
    assert (pairs == np.array(pop._user_item_pairs)).all()
    assert ((pairs[:, 0] == 2) & (pairs[:, 1] == 79)).sum() == 2, "the sample graph lost its duplicated interaction"
    test = TestCFGraphDataset(path)
    crow, col = [0], []
    for u in range(len(test._users)):
        row = sorted(test._idx_to_set[u])
        col += row
        crow.append(len(col))
    save("cf_data_sample", pair_user=pairs[:, 0], pair_item=pairs[:, 1], users=np.array(uni._users, dtype=np.int64),
         num_users=np.array(uni.num_users), num_items=np.array(uni.num_items), per_user_num=np.array(uni.per_user_num),
         len_uniform=np.array(len(uni)), len_popularity=np.array(len(pop)),
         test_users=np.array(test._users, dtype=np.int64), test_len=np.array(len(test)),
         truth_crow=np.array(crow, dtype=np.int64), truth_col=np.array(col, dtype=np.int64))


if __name__ == "__main__":
    main()

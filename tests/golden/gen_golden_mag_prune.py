#!/usr/bin/env python3
"""Generate the magnitude-pruning golden vectors (tests/golden/mag_prune_*.npz) by IMPORTING THE REFERENCE.

Needs a checkout of the reference (named by RECSYS_REFERENCE) and CPU PyTorch:

    RECSYS_REFERENCE=<reference checkout> PYTHONHASHSEED=0 python tests/golden/gen_golden_mag_prune.py

Same conventions as gen_golden_cerp_cf.py: the reference's modules are imported unmodified (`loguru` replaced by a no-op
stand-in), only arrays leave this script, and the archives are written with a fixed member timestamp, so a rerun
reproduces them bit for bit.

mag_prune_tables.npz — `prune` of src/utils.py:8-34 on tables whose magnitudes are PAIRWISE DISTINCT (asserted here):
the reference ranks with unstable `topk` / `argsort`, so with equal magnitudes at a cut its result is not defined and
cannot be a yardstick.  in/<table>: the input; out/<table>/p<p>_m<m>: the reference's result; `cases`: the names.
Tables: D in {8, 16, 24, 64}, no N a multiple of 64; p in {0, 0.5, 0.8, 0.99}; m in {0, 1, 3, int(D * (1 - p))},
leaving out the combinations with N * m + k > N * D (there the reference prunes its own `inf` markers).
state/*: a two-entry state dict pruned by ONE call.

mag_prune_search.npz — `bin_search` and `run_all` of scripts/lightgcn/run_mag_prune.py and
scripts/cf_train/run_mag_prune.py with `get_v` replaced by a score table: for hidden sizes 64 and 32, p in {0.5, 0.8}
and five score curves, scores/<case> (score of floor i), probes/<script>/<mode>/<case> (the floors asked for, in
order) and result/<script>/<mode>/<case> (the 1-based return value).
"""
import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

REF = os.environ.get("RECSYS_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "src")):
    sys.exit("set RECSYS_REFERENCE to a checkout of the reference (the directory that holds src/ and scripts/)")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))           # tests/: the input generator is shared with the tests


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

from src.utils import prune as ref_prune  # noqa: E402

from mag_prune_helpers import distinct_table  # noqa: E402


def save(name, **arrays):
    """np.savez_compressed, but every member stamped 1980-01-01 so that the archive bytes depend on the arrays only."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print(f"  wrote {name}.npz ({len(arrays)} arrays, {os.path.getsize(path)} bytes)")


TABLES = (("d8", 33, 8, 3101), ("d16", 77, 16, 3102), ("d24", 50, 24, 3103), ("d64", 65, 64, 3104))
RATIOS = (0.0, 0.5, 0.8, 0.99)


def assert_distinct(w):
    mags = w.abs().flatten()
    assert torch.unique(mags).numel() == mags.numel() and bool((mags > 0).all()), "magnitudes must be pairwise distinct"


def gen_tables():
    arrays, cases = {}, []
    for name, n, d, seed in TABLES:
        w = distinct_table(n, d, seed)
        assert_distinct(w)
        arrays[f"in/{name}"] = w
        for p in RATIOS:
            k = int(n * d * p)
            for m in sorted({0, 1, 3, int(d * (1 - p))}):
                if n * m + k > n * d:
                    continue
                out = ref_prune({"w": w.clone()}, p, m)["w"]
                assert int((out == 0).sum()) == k
                case = f"{name}/p{p}_m{m}"
                arrays[f"out/{case}"] = out
                cases.append(case)
    user, item = distinct_table(33, 16, 3111), distinct_table(45, 16, 3112)
    assert_distinct(user)
    assert_distinct(item)
    state = ref_prune({"user": user.clone(), "item": item.clone()}, 0.5, 2)
    arrays.update({"state/in/user": user, "state/in/item": item, "state/out/user": state["user"],
                   "state/out/item": state["item"], "state/p": np.array(0.5), "state/min_item": np.array(2)})
    save("mag_prune_tables", cases=np.array(cases), **arrays)


def load_script(rel):
    spec = importlib.util.spec_from_file_location("ref_" + rel.replace("/", "_")[:-3], os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def curves(bound):
    i = np.arange(bound + 1, dtype=np.float64)
    peak = min(5, bound)
    return {
        "rising": 0.1 + 0.01 * i,
        "falling": 0.5 - 0.01 * i,
        "peak": 0.5 - 0.01 * np.abs(i - peak),
        "flat": np.full(bound + 1, 0.25),
        "best_at_0": np.where(i == 0, 0.9, 0.1 + 0.01 * i),
    }


def gen_search():
    scripts = {"lightgcn": load_script("scripts/lightgcn/run_mag_prune.py"),
               "cf_train": load_script("scripts/cf_train/run_mag_prune.py")}
    arrays, cases = {}, []
    for hidden in (64, 32):
        for p in (0.5, 0.8):
            bound = int(hidden * (1 - p))
            for cname, scores in curves(bound).items():
                case = f"h{hidden}_p{p}_{cname}"
                cases.append(case)
                arrays[f"scores/{case}"] = scores
                for sname, mod in scripts.items():
                    for mode, fn in (("binary", mod.bin_search), ("all", mod.run_all)):
                        probes = []

                        def fake_get_v(model, prune_ratio, num_min_item, *a, **kw):
                            probes.append(int(num_min_item))
                            return float(scores[num_min_item])

                        mod.get_v = fake_get_v
                        with contextlib.redirect_stdout(io.StringIO()):
                            result = fn(None, p, hidden, None, None, "cpu")
                        arrays[f"probes/{sname}/{mode}/{case}"] = np.array(probes, dtype=np.int64)
                        arrays[f"result/{sname}/{mode}/{case}"] = np.array(int(result), dtype=np.int64)
    save("mag_prune_search", cases=np.array(cases), **arrays)


if __name__ == "__main__":
    torch.set_num_threads(1)
    which = sys.argv[1:] or ["tables", "search"]
    for w in which:
        print(f"[{w}]")
        globals()[f"gen_{w}"]()

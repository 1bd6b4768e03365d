"""CPU: the contract of magnitude pruning (tests/mag_prune_helpers.py) against the reference's recorded results, the
min-item searches against the reference's recorded probe sequences, argument checks, and the new entry points' ABI."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden

import mag_prune_helpers as H
import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import _lib, pruning

TABLES = load_golden("mag_prune_tables")
SEARCH = load_golden("mag_prune_search")
TABLE_CASES = [str(c) for c in TABLES["cases"]]
SEARCH_CASES = [str(c) for c in SEARCH["cases"]]
ENTRY_POINTS = ("mi_mag_prune_workspace_bytes", "mi_mag_prune", "mi_mag_prune_result", "mi_mag_csr_workspace_bytes",
                "mi_mag_csr_count", "mi_mag_csr_fill")


def case_args(case):
    table, rest = case.split("/")
    p, m = re.fullmatch(r"p([0-9.]+)_m(\d+)", rest).groups()
    return table, float(p), int(m)


def test_fixture_covers_what_it_must():
    seen = {case_args(c) for c in TABLE_CASES}
    dims = {t: TABLES[f"in/{t}"].shape for t, _, _ in seen}
    assert {d for _, d in dims.values()} == {8, 16, 24, 64}
    assert all(n % 64 != 0 for n, _ in dims.values())
    assert {p for _, p, _ in seen} == {0.0, 0.5, 0.8, 0.99}
    for t, (n, d) in dims.items():
        for p in (0.0, 0.5, 0.8, 0.99):
            for m in {0, 1, 3, int(d * (1 - p))}:
                if n * m + int(n * d * p) <= n * d:
                    assert (t, p, m) in seen, (t, p, m)
    for t in dims:
        mags = TABLES.t(f"in/{t}").abs().flatten()
        assert torch.unique(mags).numel() == mags.numel()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mag_prune_tables.npz")) < 400 * 1024


@pytest.mark.parametrize("case", TABLE_CASES)
def test_helper_equals_reference(case):
    table, p, m = case_args(case)
    w = TABLES.t(f"in/{table}")
    before = w.clone()
    assert torch.equal(H.mag_prune(w, p, m), TABLES.t(f"out/{case}"))
    assert torch.equal(w, before)


def test_helper_equals_reference_on_a_state_dict():
    p, m = float(TABLES["state/p"]), int(TABLES["state/min_item"])
    got = H.mag_prune_state({k: TABLES.t(f"state/in/{k}") for k in ("user", "item")}, p, m)
    for k in ("user", "item"):
        assert torch.equal(got[k], TABLES.t(f"state/out/{k}"))


def test_helper_ties_follow_flat_order_and_signed_zeros_share_a_key():
    w = torch.tensor([[1.0, -1.0, 1.0, 2.0], [-0.0, 0.0, 1.0, -1.0]])
    out = H.mag_prune(w, 0.5, 0)            # k = 4: both zeros (flat 4, 5), then the first two of the five 1.0s
    assert torch.equal(out, torch.tensor([[0.0, 0.0, 1.0, 2.0], [0.0, 0.0, 1.0, -1.0]]))
    assert not torch.signbit(out[out == 0]).any()
    out = H.mag_prune(w, 0.5, 1)            # the floor protects 2.0 in row 0 and the FIRST 1.0 (column 2) in row 1
    assert torch.equal(out, torch.tensor([[0.0, 0.0, 1.0, 2.0], [0.0, 0.0, 1.0, -1.0]]))
    out = H.mag_prune(w, 0.75, 1)           # k = 6 = everything unprotected
    assert torch.equal(out, torch.tensor([[0.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 0.0]]))


@pytest.mark.parametrize("script", ["lightgcn", "cf_train"])
@pytest.mark.parametrize("mode", ["binary", "all"])
@pytest.mark.parametrize("case", SEARCH_CASES)
def test_search_reproduces_the_reference_probe_sequence(case, mode, script):
    hidden, p = re.fullmatch(r"h(\d+)_p([0-9.]+)_\w+", case).groups()
    scores = SEARCH[f"scores/{case}"]
    probes = []

    def evaluate(min_item):
        probes.append(int(min_item))
        return float(scores[min_item])

    got = pkg.search_min_item(None, float(p), int(hidden), mode=mode, evaluate=evaluate)
    assert probes == SEARCH[f"probes/{script}/{mode}/{case}"].tolist()
    assert got == int(SEARCH[f"result/{script}/{mode}/{case}"])
    assert isinstance(got, int)


def test_search_bound_is_computed_as_the_reference_does():
    assert pruning._max_min_item(64, 0.8) == 12          # int(64 * (1 - 0.8)) == int(12.799999999999997)
    assert SEARCH["probes/lightgcn/all/h64_p0.8_flat"].tolist() == list(range(13))
    assert pruning._max_min_item(32, 0.5) == 16
    with pytest.raises(ValueError):
        pkg.search_min_item(None, 0.5, 64, mode="ternary", evaluate=lambda m: 0.0)


def test_arguments_are_checked_before_anything_runs():
    w = torch.ones(10, 8)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            pkg.prune_table(w, bad)
        with pytest.raises(ValueError):
            pkg.prune({"w": w}, bad)
        with pytest.raises(ValueError):
            H.mag_prune(w, bad)
    for p, m in ((0.5, 5), (0.99, 1), (0.0, 9), (1.0, 1)):          # N * m + k > N * D
        with pytest.raises(ValueError):
            pkg.prune_table(w, p, m)
        with pytest.raises(ValueError):
            pkg.prune({"w": w}, p, m)
        with pytest.raises(ValueError):
            H.mag_prune(w, p, m)
    with pytest.raises(ValueError):
        pkg.prune_table(w, 0.5, -1)
    with pytest.raises(ValueError):
        pkg.prune({"w": torch.ones(8)}, 0.5)             # the reference asserts 2-D entries
    with pytest.raises(ValueError):
        pkg.prune_table(w, 0.5, out=torch.ones(10, 4))
    assert torch.equal(w, torch.ones(10, 8))


def test_cpu_tensors_fail_loudly():
    w = torch.randn(10, 8)
    before = w.clone()
    with pytest.raises(pkg.MI355XLibraryError):
        pkg.prune_table(w, 0.5)
    with pytest.raises(pkg.MI355XLibraryError):
        pkg.prune({"w": w}, 0.5, 1)
    with pytest.raises(pkg.MI355XLibraryError):
        pkg.embeddings.PrunedEmbedding.from_pruned(w, 0.5)
    with pytest.raises(pkg.MI355XLibraryError):
        pkg.evaluate_pruned(pkg.LightGCN(5, 7, hidden_size=8), 0.5, 0, [], None, device="cpu")
    with pytest.raises(TypeError):
        pkg.to_pruned_tables(torch.nn.Linear(2, 2))
    assert torch.equal(w, before)


def test_header_bindings_and_library_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "mi355x_recsys.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"MI_API\s+\w+\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("mi_mag_prune_workspace_bytes", "mi_mag_csr_workspace_bytes"):
        assert _lib._RESTYPES[name] is ctypes.c_int64
    loaded = _lib.load()
    assert loaded.mi_abi_version() == 3
    for n in (1, 1000, 33762577):
        assert loaded.mi_mag_prune_workspace_bytes(n) >= 8 * n + 4 * (2048 + 2048 + 512)
        assert loaded.mi_mag_csr_workspace_bytes(n) >= 8 * n
    # host-side argument checks of the entry points: nothing is launched for these
    assert loaded.mi_mag_prune(None, 8, None, 8, 4, 8, 1, 0, None, None) == -1
    assert loaded.mi_mag_prune(8, 16, None, 16, 1 << 28, 16, 1, 0, 8, None) == -1          # 2^32 elements
    assert loaded.mi_mag_prune(8, 8, None, 8, 4, 8, 30, 1, 8, None) == -1                   # N * m + k > N * D
    assert loaded.mi_mag_prune(8, 2048, None, 2048, 4, 2048, 1, 0, 8, None) == -2            # D > 1024
    assert loaded.mi_mag_csr_count(8, 8, 4, 8, None, 1, 8, 8, None) == -1                    # a floor without a select

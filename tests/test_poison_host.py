"""CPU: the poison context manager, its recorder and the allocation-site scan of tests/poison_helpers.py."""
import importlib.util
import math
import os
import textwrap

import pytest
import torch

import poison_helpers as ph


def _originals():
    return torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty


def test_float_tensors_on_the_device_type_are_poisoned_and_integers_are_left_alone():
    before = _originals()
    with ph.poisoned(device_type="cpu", record=set()):
        assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
        for t in (torch.empty(5), torch.empty((2, 3), dtype=torch.float64), torch.empty_like(torch.zeros(4)),
                  torch.zeros(3).new_empty((2, 2)), torch.empty_strided((2, 3), (3, 1)), torch.empty(3, dtype=torch.float16)):
            assert bool(torch.isnan(t).all()), t.dtype
        marker = torch.full((6,), 7, dtype=torch.int64)
        for dt in (torch.int64, torch.int32, torch.uint8, torch.bool):
            t = torch.empty_like(marker, dtype=dt)
            assert t.dtype == dt and not t.is_floating_point()          # (left as it came: nothing to read back)
        assert torch.empty(0).numel() == 0
        leaf = torch.empty(3, requires_grad=True)
        assert leaf.requires_grad and bool(torch.isnan(leaf).all())
    assert _originals() == before
    with ph.poisoned(device_type="cuda", record=set()):
        assert not bool(torch.isnan(torch.zeros(3).new_empty(4).fill_(1.0)).any())
        t = torch.empty(64)
        t.zero_()
        assert not bool(torch.isnan(t).any())            # another device type: untouched by the wrapper
    with ph.poisoned(device_type="cpu", fill=False, record=set()):
        t = torch.empty(4).fill_(2.0)
        assert not bool(torch.isnan(t).any())


def test_originals_are_restored_after_an_exception():
    before = _originals()
    with pytest.raises(RuntimeError, match="inside"):
        with ph.poisoned(device_type="cpu", record=set()):
            assert torch.empty is not before[0]
            raise RuntimeError("inside")
    assert _originals() == before
    assert not bool(torch.isnan(torch.empty(3).zero_()).any())


FIXTURE = textwrap.dedent('''\
    import torch


    def single():
        return torch.empty(3)


    def multi(like):
        return torch.empty_like(
            like,
            dtype=torch.float32,
        )


    def method(like):
        out = like.new_empty((2,
                              2))
        return out


    def ints():
        return torch.empty(4, dtype=torch.int64)
    ''')


def test_recorder_attributes_single_and_multi_line_calls(tmp_path, monkeypatch):
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    path = pkg / "fixture_mod.py"
    path.write_text(FIXTURE)
    spec = importlib.util.spec_from_file_location("poison_fixture_mod", str(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(ph, "PKG_DIR", str(pkg))
    sites = ph.allocation_sites(str(pkg))
    assert [s[:3] for s in sites] == [("fixture_mod.py", 5, 5), ("fixture_mod.py", 9, 12), ("fixture_mod.py", 16, 17),
                                      ("fixture_mod.py", 22, 22)]
    seen = set()
    with ph.poisoned(device_type="cpu", fill=False, record=seen):
        mod.single()
        torch.empty(2)                       # a call from outside the package directory is not recorded
    assert {s[:3] for s in ph.reached_sites(seen, sites)} == {("fixture_mod.py", 5, 5)}
    seen.clear()
    with ph.poisoned(device_type="cpu", record=seen):
        assert bool(torch.isnan(mod.multi(torch.zeros(3))).all())
        assert bool(torch.isnan(mod.method(torch.zeros(3))).all())
        mod.ints()
    assert {s[:3] for s in ph.reached_sites(seen, sites)} == {("fixture_mod.py", 9, 12), ("fixture_mod.py", 16, 17),
                                                              ("fixture_mod.py", 22, 22)}
    assert ph.sites_of("fixture_mod.py", 14, sites) == [] and len(ph.sites_of("fixture_mod.py", 11, sites)) == 1


def test_the_scan_finds_the_packages_allocation_sites():
    sites = ph.allocation_sites()
    assert len(sites) >= 232
    assert len(set(sites)) == len(sites)
    for f, lo, hi, _col in sites:
        assert not f.startswith("..") and os.path.isfile(os.path.join(ph.PKG_DIR, f)) and 1 <= lo <= hi
    per_file = {}
    for f, *_ in sites:
        per_file[f] = per_file.get(f, 0) + 1
    assert per_file["_kernels.py"] > per_file["tail.py"] > per_file["losses.py"] > 0


def test_not_reached_names_real_sites_with_a_reason_and_stays_small():
    keys = {ph.site_key(s) for s in ph.allocation_sites()}
    for key, reason in ph.NOT_REACHED.items():
        assert key in keys, f"stale NOT_REACHED entry {key}"
        assert isinstance(reason, str) and reason.strip()
    assert len(ph.NOT_REACHED) <= math.floor(0.10 * len(keys))


def test_catalogue_names_are_unique_and_cover_the_alignment_case():
    names = [c.name for c in ph.CASES]
    assert len(set(names)) == len(names)
    assert sum(n.startswith("dual_gather-alignment") for n in names) == 4
    assert "dual_gather-aligned-n1_3" in names

"""GPU: every catalogue case of tests/poison_helpers.py, run clean and then with every torch.empty / empty_like / new_empty
float buffer of the package pre-filled with NaN.  A kernel that reads a slot it (or an earlier launch) did not write turns
that into NaN in a returned tensor; a kernel that ADDS into a buffer the Python side believed it overwrites does the same.
Three assertions per case: nothing returned holds NaN or Inf, the poisoned run passes the op's own reference comparison,
and where the op sums in a fixed order the poisoned and the clean run are bit-equal."""
import pytest
import torch

import poison_helpers as ph

pytestmark = pytest.mark.gpu


def _assert_finite(result, what):
    for k, v in result.items():
        vals = ph.values_of(v)
        assert bool(torch.isfinite(vals).all()) if vals.is_floating_point() else True, \
            f"{what}: {k} holds {int((~torch.isfinite(vals)).sum())} NaN / Inf of {vals.numel()} elements"


def _assert_same_bits(a, b, what):
    if a.is_sparse:
        assert b.is_sparse and torch.equal(a._indices(), b._indices()) and torch.equal(a._values(), b._values()), what
    else:
        assert torch.equal(a, b), f"{what}: max diff {float((a.double() - b.double()).abs().max()):.3e}"


@pytest.mark.parametrize("case", ph.CASES, ids=[c.name for c in ph.CASES])
def test_poisoned_allocations_change_nothing(case):
    clean = case.run()
    _assert_finite(clean, "clean run")
    with ph.poisoned():
        bad = case.run()
        assert set(bad) == set(clean)
        _assert_finite(bad, "poisoned run")
        case.check(bad)
    for k in clean:
        if case.exact(k):
            _assert_same_bits(clean[k], bad[k], f"{case.name}: {k} differs between the clean and the poisoned run")


def test_the_alignment_cases_hand_the_backward_a_gradient_off_the_16_byte_boundary():
    """What makes the alignment cases a test of the fallback: the upstream gradient DualGather.backward receives is a
    contiguous view that does not start on a 16-byte boundary — and the aligned twin of n1 = 3 one that does, so that it
    runs the float4 kernel that adds into table 1's gradient."""
    names = [c for c in ph.CASES if c.name.startswith("dual_gather-alignment")]
    assert len(names) == 4
    for case in names:
        case.run()
        offset, contiguous = ph.ALIGN_OFFSETS[case.name]
        assert contiguous and offset % 16 != 0, (case.name, offset)
    twin, = [c for c in ph.CASES if c.name.startswith("dual_gather-aligned")]
    twin.run()
    assert ph.ALIGN_OFFSETS[twin.name] == (0, True)


def test_catalogue_reaches_the_allocation_sites():
    """The whole catalogue once under the recorder (nothing poisoned): every torch.empty / empty_like / new_empty call of the
    package is reached by a case or listed in NOT_REACHED with its reason — so a new one fails here until a case reaches
    it.  Stale and needless entries of NOT_REACHED fail too, and it may hold a tenth of the sites at most."""
    seen = set()
    with ph.poisoned(fill=False, record=seen):
        for case in ph.CASES:
            case.run()
    sites = ph.allocation_sites()
    reached = {ph.site_key(s) for s in ph.reached_sites(seen, sites)}
    keys = {ph.site_key(s) for s in sites}
    stale = sorted(set(ph.NOT_REACHED) - keys)
    needless = sorted(set(ph.NOT_REACHED) & reached)
    missing = sorted(keys - reached - set(ph.NOT_REACHED))
    print(f"allocation sites: {len(keys)}, reached: {len(reached)}, listed as not reachable: {len(ph.NOT_REACHED)}")
    assert not stale, f"NOT_REACHED entries that point at no site: {stale}"
    assert not needless, f"NOT_REACHED entries whose site a case reaches: {needless}"
    assert len(ph.NOT_REACHED) <= len(keys) // 10
    assert not missing, f"{len(missing)} of {len(keys)} allocation sites are reached by no case: {missing}"

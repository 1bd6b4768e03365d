"""CPU: tests/tt_kernel_helpers.py's restatements of the grouped TT-Rec kernels are right — chained level by level the way
TTLookupGrouped chains the kernels they equal oracle.reference_ops.tt_forward and its autograd core gradients in float64 to
1e-12 for every end-to-end configuration of tests/test_tt_kernels_gpu.py — and the premises of that file hold: the integer-valued
kernel checks stay below 2^24 (exact in float32 in any summation order), and the oracle evaluated in float32 on the CPU is
well inside the end-to-end tolerances."""
import pytest
import torch

import tt_kernel_helpers as H
from oracle import reference_ops as ro


def _oracle(cores, idx, G, ps, qs, ranks, dtype=torch.float64):
    cs = [c.detach().to(dtype).requires_grad_(True) for c in cores]
    ref = ro.tt_forward(idx.flatten(), ps, qs, ranks, cs)
    (ref * G.to(dtype)).sum().backward()
    return ref.detach(), [c.grad for c in cs]


@pytest.fixture(scope="module")
def oracle64():
    cache = {}

    def get(name):
        if name not in cache:
            _, _, ps, qs, _ = H.e2e_case(name)
            cores, idx, G, ranks = H.e2e_inputs(name)
            cache[name] = _oracle(cores, idx, G, ps, qs, ranks)
        return cache[name]

    return get


@pytest.mark.parametrize("name", [c[0] for c in H.E2E_CASES])
def test_chained_restatements_equal_the_oracle(name, oracle64):
    _, fast, ps, qs, _ = H.e2e_case(name)
    cores, idx, G, ranks = H.e2e_inputs(name)
    assert H.grouped_supported(qs, ranks)
    Hs = H.prod(qs[:-1])
    assert H.last_fast(Hs, ranks[-2], qs[-1]) == fast            # the table's branch is the branch the dispatch takes
    ref, gref = oracle64(name)
    out, ctx = H.grouped_forward(idx, H.E2E_N, ps, qs, ranks, cores)
    assert ctx["fast"] == fast
    assert float((out - ref).abs().max()) <= 1e-12
    grads = H.grouped_backward(ctx, G, ps, qs, ranks)
    for c, (a, b) in enumerate(zip(grads, gref)):
        assert float((a - b).abs().max()) <= 1e-12, f"core {c}"


@pytest.mark.parametrize("name", H.E2E_BAD_IDS)
def test_chain_drops_invalid_lookups(name):
    """Out-of-range ids: zero rows, and nothing in any core gradient even where the upstream gradient is NaN."""
    _, _, ps, qs, _ = H.e2e_case(name)
    cores, idx, G, ranks = H.e2e_inputs(name, n=600)
    bad = torch.tensor([5, 300, 599])
    idx_bad, G_bad = idx.clone(), G.clone()
    idx_bad[bad] = torch.tensor([H.E2E_N, -1, 1 << 40])
    G_bad[bad] = float("nan")
    idx0, G0 = idx.clone(), G.clone()
    idx0[bad], G0[bad] = 0, 0.0
    ref, gref = _oracle(cores, idx0, G0, ps, qs, ranks)
    ref[bad] = 0.0
    out, ctx = H.grouped_forward(idx_bad, H.E2E_N, ps, qs, ranks, cores)
    assert float((out - ref).abs().max()) <= 1e-12
    for c, (a, b) in enumerate(zip(H.grouped_backward(ctx, G_bad, ps, qs, ranks), gref)):
        assert float((a - b).abs().max()) <= 1e-12, f"core {c}"


@pytest.mark.parametrize("name", [c[0] for c in H.E2E_CASES])
def test_float32_oracle_is_inside_the_end_to_end_tolerances(name, oracle64):
    """The tolerances of test_tt_grouped_gpu._check leave room for a float32 evaluation in another order: stock float32 on the
    CPU uses at most a tenth of them."""
    _, _, ps, qs, _ = H.e2e_case(name)
    cores, idx, G, ranks = H.e2e_inputs(name)
    ref, gref = oracle64(name)
    out, grads = _oracle(cores, idx, G, ps, qs, ranks, torch.float32)
    worst = H.tol_fraction(out, ref, *H.E2E_TOL["fwd"])
    for a, b in zip(grads, gref):
        worst = max(worst, H.tol_fraction(a, b, *H.E2E_TOL["grad"]))
    print(f"{name}: float32 oracle uses {worst:.4f} of the tolerance")
    assert worst < 0.1


def test_integer_checks_stay_exact_in_float32():
    bounds = H.exact_bounds()
    assert len(bounds) == 3 * len(H.LAST_SHAPES) + len(H.ROW_GROUP_K) + 3
    for case, b in bounds.items():
        assert 0 < b < H.EXACT, case
    # the limits of the last-level kernels are in the table, and so is every U
    assert any(h * k == 512 for h, k, q in H.LAST_SHAPES) and any(k * q == 512 for h, k, q in H.LAST_SHAPES)
    assert {-(-k * q // 64) for h, k, q in H.LAST_SHAPES} == set(range(1, 9))
    assert {h * q for h, k, q in H.LAST_SHAPES} == {4, 8, 16, 32, 64}
    assert all(H.last_fast(*s) for s in H.LAST_SHAPES)
    assert any((k // 4) % (64 // (h * q)) for h, k, q in H.LAST_SHAPES)           # a ragged k-range


def test_digits_restatement():
    ps = [3, 1, 5]
    idx = torch.tensor([0, 14, 7, 15, -1, 1 << 40, 12])
    d, v = H.digits(idx, 13, ps)
    assert v.tolist() == [1, 0, 1, 0, 0, 0, 1]
    assert d[:, 2].tolist() == [1, 0, 2] and d[:, 6].tolist() == [2, 0, 2] and not d[:, [1, 3, 4, 5]].any()
    for i in (0, 2, 6):
        assert int(d[0, i]) * 5 + int(d[1, i]) * 5 + int(d[2, i]) == int(idx[i])


@pytest.mark.parametrize("p,Hh,seg,n", [(1, 1, 16, 1), (37, 4, 16, 5000), (5, 16, 256, 65), (1025, 1, 2048, 63)])
def test_plan_restatement_invariants(p, Hh, seg, n):
    gen = torch.Generator().manual_seed(p + n)
    digit = torch.randint(0, p, (n,), generator=gen).to(torch.int32)
    digit[0] = p - 1
    pl = H.Plan(digit, p, Hh, seg)
    assert int(pl.counts.sum()) == n and torch.equal(pl.rows, pl.counts * Hh)
    assert not bool((pl.pbeg % H.TILE).any()) and int(pl.pend[-1]) <= pl.mpad
    assert pl.pos.unique().numel() == n and not bool((pl.pos % Hh).any())
    d = digit.long()
    assert bool((pl.pos >= pl.pbeg[d]).all()) and bool((pl.pos + Hh <= pl.pbeg[d] + pl.rows[d]).all())
    tiles = int(pl.pend[-1]) // H.TILE
    assert bool((pl.mtile_b[:tiles] >= 0).all()) and bool((pl.mtile_b[tiles:] == -1).all())
    assert torch.equal(pl.mtile_b[(pl.pos // H.TILE)].long(), d)
    live = pl.kseg[:pl.live]
    assert int(live[:, 1].sum()) == n * Hh and int(live[:, 1].max()) <= seg and not bool(pl.kseg[pl.live:].any())
    assert pl.live <= pl.nseg and tiles <= pl.ntiles

"""Host: the three pure decisions of the fused tail's driver (recsys-benchmark_amd/tail.py) — the form record (_form), the
layout of the step's zero-filled buffer (_zero_layout) and the launch that advances the dropout seed (_seed_launch) — over
every plan of test_tail_mixed_gpu.CASES, built on the CPU, in every form the knobs select.  No kernel runs; the only
library call is mi_tail_head_bce_ws_elems, which needs no device."""
import itertools

import pytest

import test_tail_mixed_gpu as mixed
from tail_helpers import active_ps, build_tail, hidden_layers

from recsys_benchmark_amd import _kernels, _lib
from recsys_benchmark_amd import tail

FORMS = {"sums": (True, False, False), "joins": (False, True, False), "finalize": (False, False, False),
         "deterministic": (True, False, True)}                    # form -> (STAT_SUMS, MERGE_JOINS, deterministic mode)


def _plan(name):
    _, K, layers, head_bias, hyper = mixed.CASES[name]
    seq = build_tail(K, layers, head_bias, *(hyper or (None, None)))
    plan = tail._Plan(tail._Layer(lin, bn, p, bn is None or not bn.training)
                      for (_, lin, bn, _), p in zip(hidden_layers(seq)[0], active_ps(seq)))
    return plan, [(L.lin.out_features, L.lin.in_features) for L in plan]


@pytest.fixture(params=list(FORMS))
def form_knobs(request, monkeypatch):
    sums, merge, det = FORMS[request.param]
    monkeypatch.setattr(tail, "STAT_SUMS", sums)
    monkeypatch.setattr(tail, "MERGE_JOINS", merge)
    monkeypatch.setattr(_kernels, "DETERMINISTIC", det)
    return request.param


def _parent_offsets(dims, f, extra_zero):
    """The arithmetic of the driver this layout function replaced, as it stood in _tail_forward / _tail_backward."""
    zoff = [0]
    for N, K in dims:
        zoff.append(zoff[-1] + N * K + N)
    zsize = (zoff[-1] + 3) // 4 * 4 if f.grad else 0
    foff, boff, hoff, loff, eoff = {}, {}, None, None, None
    for i, (N, _) in enumerate(dims):
        if f.stat_f[i]:
            foff[i] = zsize
            zsize += (f.R * 4 * N + 3) // 4 * 4
    if f.stat_b:
        for i in range(len(dims) - 1):
            boff[i] = zsize
            zsize += f.R * 2 * dims[i][0]
        hoff = zsize
        zsize += f.Rh * (3 * dims[-1][0] + 4)
        zsize = (zsize + 3) // 4 * 4
        if f.head_loss:
            loff = zsize
            zsize += int(_lib.load().mi_tail_head_bce_ws_elems(f.Rh))
    if extra_zero > 0 and f.grad:
        eoff = zsize
        zsize += (extra_zero + 3) // 4 * 4
    return zoff, foff, boff, hoff, loff, eoff, zsize


@pytest.mark.parametrize("name", mixed.ORDER)
def test_zero_layout(name, form_knobs):
    plan, dims = _plan(name)
    for grad, labels, extra_zero in itertools.product((True, False), (True, False), (0, 68 * 20)):
        f = tail._form(plan, extra_zero > 0, labels, grad)
        lay = tail._zero_layout(dims, f, extra_zero)
        blocks = [*lay.w, *lay.b, *lay.fsum.values(), *lay.bsum.values()] + [c for c in (lay.head, lay.head_w, lay.loss, lay.extra)
                                                                             if c is not None]
        blocks.sort(key=lambda c: c.start)
        assert all(c.start % 4 == 0 and c.start < c.stop <= lay.total for c in blocks) and lay.total % 4 == 0
        assert all(a.stop <= b.start for a, b in zip(blocks, blocks[1:])), "blocks overlap"
        assert all(4 * c.start % 8 == 0 for c in lay.fsum.values()), "fp64 sums off their 8 bytes"
        # ... and where the replaced arithmetic put them
        zoff, foff, boff, hoff, loff, eoff, zsize = _parent_offsets(dims, f, extra_zero)
        Nl = dims[-1][0]
        assert lay.total == zsize
        if grad:
            assert list(lay.w) == [slice(zoff[i], zoff[i] + N * K) for i, (N, K) in enumerate(dims)]
            assert list(lay.b) == [slice(zoff[i] + N * K, zoff[i + 1]) for i, (N, K) in enumerate(dims)]
        else:
            assert not lay.w and not lay.b and lay.extra is None
        assert lay.fsum == {i: slice(o, o + f.R * 4 * dims[i][0]) for i, o in foff.items()}
        assert lay.bsum == {i: slice(o, o + f.R * 2 * dims[i][0]) for i, o in boff.items()}
        assert lay.head == (None if hoff is None else slice(hoff, hoff + f.Rh * 2 * Nl))
        assert lay.head_w == (None if hoff is None else slice(hoff + f.Rh * 2 * Nl, hoff + f.Rh * (3 * Nl + 4)))
        assert (lay.loss is None) == (loff is None) and (loff is None or lay.loss.start == loff)
        assert lay.extra == (None if eoff is None else slice(eoff, eoff + extra_zero))
        assert not f.head_epi or lay.total == 0


@pytest.mark.parametrize("name", mixed.ORDER)
def test_one_launch_advances_the_seed(name, form_knobs, monkeypatch):
    plan, _ = _plan(name)
    k = len(plan)
    for lead, ride, grad in itertools.product((True, False), (True, False), (True, False)):
        monkeypatch.setattr(tail, "RIDE_MASKS", ride)
        f = tail._form(plan, lead, False, grad)
        at = tail._seed_launch(plan, f)
        if not any(L.p > 0 for L in plan):
            assert at is None
            continue
        kind, i = at
        # a launch the step has: layer i's finalize, a kernel behind a layer whose statistics are still pending, the head
        joined = [not L.fixed and (f.stat_f[j] or f.merge) for j, L in enumerate(plan)]
        if kind == "finalize":
            assert not plan[i].fixed and not joined[i]
            assert not (f.ride and i == 0), "the finalize launch that carries the mask job made the bits"
        elif kind == "join":
            assert 1 <= i <= k and joined[i - 1] and not any(joined[:i - 1]), "the FIRST kernel that joins advances"
        else:
            assert at == ("head", k) and not any(joined)


@pytest.mark.parametrize("name", mixed.ORDER)
def test_forms_exclude_each_other(name, form_knobs):
    plan, _ = _plan(name)
    for lead, labels, grad in itertools.product((True, False), (True, False), (True, False)):
        f = tail._form(plan, lead, labels, grad)
        assert (f.det, f.merge) == (FORMS[form_knobs][2], FORMS[form_knobs][1]) and f.grad == grad
        if f.head_epi:
            assert not grad and not labels and all(L.fixed and L.p == 0 for L in plan)
        if f.det or f.merge:
            assert not f.sums and not any(f.stat_f) and not f.stat_b and not f.head_loss and not f.lead_ride
        if f.merge:
            assert not f.ride
        assert not f.lead_ride or (lead and not f.ride)
        assert f.keep_inputs == (grad and not f.det) and (f.R, f.Rh) == (tail.STAT_REPS, tail.HEAD_REPS)

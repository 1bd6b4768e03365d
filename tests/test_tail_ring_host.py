"""Host: the schedule of the tail products' LDS ring (recsys-benchmark_amd/csrc/tail_gemm.hpp: ring_produce / ring_consume),
walked on the CPU through mi_tail_ring_plan — the very control flow the kernels compile, with a recorder in place of the
loads, LDS writes and MFMAs.  Runs without a GPU.

The two roles of a workgroup meet at barriers only, so a barrier-count mismatch is a hang and a misplaced finish is a race.
For every reduction length nst = 1..64 x {full, partial with a dead half, partial without} x {PRE active or not} the two event
streams are lined up at their barriers (event epoch = barriers executed before it) and checked, for the producers' exit-free
walk (role 0: lean operands) and for their one-loop walk (role 2: general addressing) alike:
  - both roles execute 1 + nst ring barriers, plus the PRE barrier, first, when it is active;
  - every slice is fetched once (no fetch of an index >= nst), finished once, out of the register stage it was fetched into
    and into the slot the consumer reads it from; no stage is overwritten before it is finished;
  - a slice's finish lies at least one barrier before its first fragment read, and the finish that overwrites a slot lies
    at least one barrier after the last read of the slice that was there;
  - the MFMAs consume every live half slice exactly once, in order, and never a fragment set read from a slot beyond the end;
  - the partial slice is slice 0, sits at the range's end and goes through the *_any forms.
(nst = 1 with a partial slice takes the kernels' unpipelined `lone` step; the plan is checked for it all the same.)"""
import ctypes

import pytest

from recsys_benchmark_amd import _lib

BARRIER, PRE_BARRIER, FETCH, FINISH, READ, MMA = range(6)
RING, STAGES = 4, 3


def _plan(nst, partial, dead_half, pre, role):
    lib = _lib.load()
    cap = 16 * nst + 64
    buf = (ctypes.c_int32 * (6 * cap))()
    n = ctypes.c_int32()
    _lib.check(lib.mi_tail_ring_plan(nst, int(partial), int(dead_half), int(pre), role, ctypes.addressof(buf), cap, ctypes.addressof(n)),
               "mi_tail_ring_plan")
    assert 0 < n.value <= cap
    ev, epoch = [], 0
    for i in range(n.value):
        kind, slice_, reg, slot, any_, pos = buf[6 * i:6 * i + 6]
        ev.append(dict(kind=kind, slice=slice_, reg=reg, slot=slot, any=any_, pos=pos, epoch=epoch, at=i))
        epoch += kind in (BARRIER, PRE_BARRIER)
    return ev


FORMS = [(False, False), (True, True), (True, False)]      # (partial, dead_half)


@pytest.mark.parametrize("pre", [False, True], ids=["nopre", "pre"])
@pytest.mark.parametrize("partial,dead_half", FORMS, ids=["full", "partial-dead-half", "partial"])
def test_both_roles_follow_one_schedule(partial, dead_half, pre):
    for nst in range(1, 65):
        C = _plan(nst, partial, dead_half, pre, 1)
        for role in (0, 2):      # the exit-free walk of the lean operands, the one-loop walk of general addressing
            _check(nst, partial, dead_half, pre, _plan(nst, partial, dead_half, pre, role), C, f"nst={nst} role={role}")


def _check(nst, partial, dead_half, pre, P, C, tag):
    # ---- barriers
    for name, ev in (("producers", P), ("consumers", C)):
        bars = [e["kind"] for e in ev if e["kind"] in (BARRIER, PRE_BARRIER)]
        assert bars == [PRE_BARRIER] * pre + [BARRIER] * (1 + nst), f"{tag} {name}: barriers {bars}"
    # ---- producers: fetch / finish bookkeeping
    stage = [None] * STAGES            # slice held by each register stage
    fetched, finished = {}, {}
    for e in P:
        if e["kind"] == FETCH:
            s = e["slice"]
            assert 0 <= s < nst, f"{tag}: fetch of slice {s}"
            assert s not in fetched, f"{tag}: slice {s} fetched twice"
            assert stage[e["reg"]] is None, f"{tag}: stage {e['reg']} overwritten while it holds slice {stage[e['reg']]}"
            stage[e["reg"]] = s
            fetched[s] = e
        elif e["kind"] == FINISH:
            s = e["slice"]
            assert s in fetched and s not in finished, f"{tag}: finish of slice {s}"
            assert stage[e["reg"]] == s, f"{tag}: slice {s} finished out of stage {e['reg']} which holds {stage[e['reg']]}"
            assert e["slot"] == s % RING
            assert e["any"] == fetched[s]["any"], f"{tag}: slice {s} fetched and finished by different forms"
            stage[e["reg"]] = None
            finished[s] = e
    assert sorted(finished) == list(range(nst)), f"{tag}: finished {sorted(finished)}"
    assert stage == [None] * STAGES
    assert sorted(e["pos"] for e in finished.values()) == list(range(nst)), f"{tag}: the slices do not tile the range"
    if partial:
        assert finished[0]["pos"] == nst - 1 and finished[0]["any"] == 1, f"{tag}: the partial slice"
    assert all(e["any"] == 0 for s, e in finished.items() if s > 0) and finished[0]["any"] == 1
    if pre:
        assert min(e["epoch"] for e in finished.values()) >= 1, f"{tag}: a finish in front of the PRE barrier"
    # ---- consumers: fragment reads and MFMAs
    reads = {}                         # slice -> read events
    held = [None, None]                # (slice, half) in fragment set 0 / 1
    used = []
    for e in C:
        if e["kind"] == READ:
            s, half = e["slice"], e["reg"]
            assert 0 <= s <= nst and e["slot"] == s % RING and 0 <= e["slot"] < RING, f"{tag}: read of slice {s}"
            held[half] = (s, half)
            reads.setdefault(s, []).append(e)
        elif e["kind"] == MMA:
            got = held[e["reg"]]
            assert got is not None and got[0] < nst, f"{tag}: MFMAs on fragments {got}"
            used.append(got)
            held[e["reg"]] = None
    want = [(s, h) for s in range(nst) for h in (0, 1) if not (dead_half and s == 0 and h == 1)]
    assert used == want, f"{tag}: half slices consumed {used}"
    # ---- the two roles against each other
    for s in range(nst):
        first = min(e["epoch"] for e in reads[s])
        assert finished[s]["epoch"] < first, f"{tag}: slice {s} finished in epoch {finished[s]['epoch']}, first read in {first}"
        if s >= RING:
            last = max(e["epoch"] for e in reads[s - RING])
            assert last < finished[s]["epoch"], f"{tag}: slot {s % RING} overwritten in epoch {finished[s]['epoch']}, still read in {last}"
    # a read beyond the end (values unused) may only meet a slot nobody writes any more
    for e in reads.get(nst, []):
        writes = [f["epoch"] for f in finished.values() if f["slot"] == e["slot"]]
        assert all(w < e["epoch"] for w in writes), f"{tag}: the read beyond the end races a finish"


def test_steady_state_has_no_exits_and_the_drain_no_loads_beyond_the_end():
    """Shape of the producers' walk for the headline's 13 slices: barrier 0 closes a prologue of six fetches and three
    finishes; phases 0..5 (two whole triples) each finish one slice and fetch one; phase 6 is the last that fetches; phases
    7..9 only finish; phases 10..12 only arrive."""
    P = _plan(13, True, True, True, 0)
    by_epoch = {}
    for e in P:
        if e["kind"] in (FETCH, FINISH):
            by_epoch.setdefault(e["epoch"], []).append((e["kind"], e["slice"]))
    assert by_epoch[0] == [(FETCH, 0), (FETCH, 1), (FETCH, 2)]
    assert by_epoch[1] == [(FINISH, 0), (FETCH, 3), (FINISH, 1), (FETCH, 4), (FINISH, 2), (FETCH, 5)]
    phase = lambda i: by_epoch.get(i + 2, [])      # epoch 0: in front of PRE, 1: the prologue, 2 + i: phase i
    for i in range(7):
        assert phase(i) == [(FINISH, i + 3), (FETCH, i + 6)], (i, phase(i))
    for i in range(7, 10):
        assert phase(i) == [(FINISH, i + 3)], (i, phase(i))
    for i in range(10, 13):
        assert phase(i) == [], (i, phase(i))


def test_plan_rejects_bad_arguments():
    lib = _lib.load()
    n = ctypes.c_int32()
    assert lib.mi_tail_ring_plan(0, 0, 0, 0, 0, None, 0, ctypes.addressof(n)) == -1
    assert lib.mi_tail_ring_plan(4, 0, 1, 0, 0, None, 0, ctypes.addressof(n)) == -1      # a dead half needs a partial slice
    assert lib.mi_tail_ring_plan(4, 0, 0, 0, 3, None, 0, ctypes.addressof(n)) == -1
    assert lib.mi_tail_ring_plan(4, 0, 0, 0, 0, None, 0, ctypes.addressof(n)) == 0 and n.value > 0      # counting only

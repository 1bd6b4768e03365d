"""GPU: the Adagrad steps of csrc/adagrad.hip against the float64 rules of tests/adagrad_helpers.py, on gradients that reach
the eps-bound regime and on sorted ids whose runs sit on the pass edges of the shared sorted-segment walker — the places
where a piece of a run could be squared before the run is whole (straddle_2, aligned_2rs, long_mid, tail_run).  Each test
prints its worst ratio to the helper's bounds."""
import ctypes

import pytest
import torch

import adagrad_helpers as ah
import optim_helpers as oh

from recsys_benchmark_amd import _lib
from recsys_benchmark_amd._lib import MI355XLibraryError
from recsys_benchmark_amd.optim import Adagrad

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 1e-2
EPS = {"sparse": 1e-10, "rowwise": 1e-8, "dense": 1e-10}
ENTRY = {"sparse": "mi_sparse_adagrad_sorted_ld", "rowwise": "mi_rowwise_adagrad_sorted_ld"}
N_ROWS = 1000
GAP = 777.25
# (D, vals offset by one float): the float4 widths, D = 1 and 2, two widths of the any-D kernel (D = 7: lanes leave the d
# loop early), and a float4 width whose misaligned values send it to the any-D kernel
WIDTHS = [(D, 0) for D in (1, 2, 4, 8, 16, 32, 64, 128, 256, 7, 12)] + [(16, 1)]
WIDTH_IDS = [f"D{D}" + ("-offset" if off else "") for D, off in WIDTHS]


def pass_len(D):
    """Sorted positions per pass of k_rows_pass<LPR, VW> (the any-D kernel has no passes: it takes the D = 16 layout)."""
    if D == 1:
        return 64
    if D == 2:
        return 32
    if D % 4 == 0 and D // 4 in (1, 2, 4, 8, 16, 32, 64):
        return 64 // (D // 4)
    return 16


def _device_vals(vals, offset):
    buf = torch.empty(vals.numel() + 1, device=DEV)
    out = buf[offset:offset + vals.numel()]
    out.copy_(vals.reshape(-1))
    assert offset == 0 or out.data_ptr() % 16 != 0
    return out


class _Table:
    """W[N, ldw] (gap columns hold GAP), the rule's accumulator (state_sum [N, D] or row_sum [N], filled with `init`) and
    NaN-filled scratch on the device, stepped through the C entry point."""

    def __init__(self, kind, p0, ldw, init=0.0):
        self.kind, (self.N, self.D), self.ldw = kind, p0.shape, ldw
        self.W = torch.full((self.N, max(ldw, self.D)), GAP, device=DEV)
        self.W[:, :self.D] = p0.to(DEV)
        self.S = torch.full((self.N,) if kind == "rowwise" else (self.N, self.D), float(init), device=DEV)

    def step(self, ids_d, perm_d, vals_d, n, nulls=()):
        acc = torch.full((max(n, 1) * self.D,), float("nan"), device=DEV)
        ptr = {"rows": ids_d.data_ptr(), "perm": perm_d.data_ptr(), "vals": vals_d.data_ptr(), "W": self.W.data_ptr(),
               "S": self.S.data_ptr(), "acc": acc.data_ptr()}
        for k in nulls:
            ptr[k] = None
        _lib.check(getattr(_lib.load(), ENTRY[self.kind])(ptr["rows"], ptr["perm"], ptr["vals"], ptr["W"], self.ldw, ptr["S"],
                                                          ptr["acc"], n, self.D, self.N, LR, EPS[self.kind],
                                                          _lib.stream_ptr(self.W.device)), ENTRY[self.kind])
        W = self.W.cpu()
        return W[:, :self.D].contiguous(), W[:, self.D:], self.S.cpu()


def _assert_ratios(worst, what):
    print(f"{what}: worst ratio to the bounds " + " ".join(f"{k}={r:.3f}" for k, r in sorted(worst.items())))
    for k, r in worst.items():
        assert r <= 1.0, f"{what}: {r:.2f}x the {k} bound away from the float64 rule"


def _values(kind, ids, perm, D, gen):
    if kind == "rowwise":
        return ah.row_scaled_ints(ah.entry_ids(ids, perm), D, gen)
    return ah.scaled_ints((ids.numel(), D), gen)


def _three_steps(kind, ids, perm, D, offset, ldw, init, N, gen, what):
    """Three steps over the same ids with fresh values (the accumulator carries); asserts what must stay bit-unchanged and
    returns the worst ratios to the bounds."""
    n = ids.numel()
    ids_d, perm_d = ids.to(DEV), perm.to(DEV)
    p0 = torch.randn(N, D, generator=gen)
    table = _Table(kind, p0, ldw, init)
    steps, sums, touched = [], [], torch.zeros(N, dtype=torch.bool)
    for _ in range(3):
        vals = _values(kind, ids, perm, D, gen)
        g, touched = oh.coalesce_ref(ids, perm, vals, N)
        p, gap, s = table.step(ids_d, perm_d, _device_vals(vals, offset), n)
        assert bool((gap == GAP).all()), f"{what}: a gap column of the strided table changed"
        steps.append((g, touched, p))
        sums.append(s)
    p, s = steps[-1][2], sums[-1]
    # rows that do not occur and rows behind invalid ids (negative, N, N + 5: they are no rows of the table at all)
    assert torch.equal(p[~touched], p0[~touched]), f"{what}: an untouched row of W changed"
    assert torch.equal(s[~touched], torch.full_like(s[~touched], init)), f"{what}: an untouched accumulator row changed"
    return ah.worst_ratios(kind, p0, steps, sums, LR, EPS[kind], init=init)


@pytest.mark.parametrize("D,offset", WIDTHS, ids=WIDTH_IDS)
@pytest.mark.parametrize("kind", ["sparse", "rowwise"])
def test_sparse_rules_within_bounds_on_pass_edges(kind, D, offset):
    RS = pass_len(D)
    worst = {}
    for which in oh.LAYOUTS:
        lay = oh.run_layout(RS, N_ROWS, which)
        if which.startswith("edges"):
            assert {"straddle_2", "aligned_2rs", "long_mid"} <= set(lay.edges)
        for ldw, init in ((D, 0.0), (D + 4, 0.25)):
            gen = torch.Generator().manual_seed(1000 * D + 10 * oh.LAYOUTS.index(which) + ldw)
            ah.fold(worst, _three_steps(kind, lay.ids, lay.perm, D, offset, ldw, init, N_ROWS, gen, f"{which} ldw={ldw}"))
    _assert_ratios(worst, f"{kind} Adagrad D={D}{' (offset vals)' if offset else ''}")


@pytest.mark.parametrize("D", [16, 64, 7])
@pytest.mark.parametrize("kind", ["sparse", "rowwise"])
def test_a_run_across_a_pass_end_inside_random_ids(kind, D):
    RS, N = pass_len(D), 100
    gen = torch.Generator().manual_seed(77 + D)
    ids, (a, b) = oh.crossing_ids(RS, N, 40 * RS, 7, gen)
    assert a // RS == 6 and (b - 1) // RS >= 8 and ids[7 * RS - 1] == ids[7 * RS]
    perm = torch.randperm(ids.numel(), generator=gen)
    _assert_ratios(_three_steps(kind, ids, perm, D, 0, D, 0.0, N, gen, f"crossing D={D}"), f"{kind} Adagrad crossing D={D}")


@pytest.mark.parametrize("D", [16, 7])
@pytest.mark.parametrize("kind", ["sparse", "rowwise"])
def test_a_rerun_gives_equal_bits(kind, D):
    lay = oh.run_layout(pass_len(D), N_ROWS, "edges-1")
    gen = torch.Generator().manual_seed(D)
    p0 = torch.randn(N_ROWS, D, generator=gen)
    vals = _device_vals(torch.randn(lay.n, D, generator=gen), 0)      # (sums that DO round: the order has to be the same)
    ids_d, perm_d = lay.ids.to(DEV), lay.perm.to(DEV)
    runs = []
    for _ in range(2):
        table = _Table(kind, p0, D, 0.125)
        runs.append(table.step(ids_d, perm_d, vals, lay.n))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    assert not torch.equal(runs[0][0], p0)


@pytest.mark.parametrize("kind", ["sparse", "rowwise"])
def test_argument_checks(kind):
    lay = oh.run_layout(16, N_ROWS, "one")
    ids_d, perm_d = lay.ids.to(DEV), lay.perm.to(DEV)
    vals = torch.ones(1, 16, device=DEV)
    p0 = torch.zeros(N_ROWS, 16)

    def untouched(table):
        return torch.equal(table.W[:, :16].cpu(), p0) and not bool(table.S.any())

    for ldw, code in ((18, r"\(-2\)"), (12, r"\(-1\)"), (15, r"\(-1\)")):   # unsupported: float4 rows off 16 bytes; invalid: ldw < D
        table = _Table(kind, p0, 16)
        table.ldw = ldw
        with pytest.raises(MI355XLibraryError, match=code):
            table.step(ids_d, perm_d, vals, 1)
        assert untouched(table)
    for null in ("rows", "perm", "vals", "W", "S", "acc"):
        table = _Table(kind, p0, 16)
        with pytest.raises(MI355XLibraryError, match=r"\(-1\)"):
            table.step(ids_d, perm_d, vals, 1, nulls=(null,))
        assert untouched(table)
    table = _Table(kind, p0, 16)
    table.step(ids_d, perm_d, vals, 0)                                   # n = 0: OK, nothing written
    table.step(ids_d, perm_d, vals, 0, nulls=("rows", "perm", "vals", "W", "S", "acc"))
    assert untouched(table)


# ---- the dense rule ---------------------------------------------------------------------------------------------------------
DENSE_SIZES = [0, 1, 3, 4095, 4096, 4097, 10000, ("view", 4101)] + [5 + 3 * i for i in range(18)]      # 25 non-empty


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_dense_adagrad_within_bounds(wd):
    assert sum(1 for s in DENSE_SIZES if s != 0) == 25                   # 24 tensors per launch: a second one is needed
    gen = torch.Generator().manual_seed(25)
    p0s, params = [], []
    for s in DENSE_SIZES:
        view, s = (True, s[1]) if isinstance(s, tuple) else (False, s)
        p0 = oh.dense_params((s,), gen)
        if view:                                                          # one float into its buffer: the scalar route
            buf = torch.empty(s + 1, device=DEV)
            buf[1:] = p0.to(DEV)
            p = torch.nn.Parameter(buf[1:])
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(p0.to(DEV))
        p0s.append(p0), params.append(p)
    opt = Adagrad(params, lr=LR, eps=EPS["dense"], weight_decay=wd)
    assert all(opt._kernel_ok(g) for g in opt.param_groups)
    trails = [([], []) for _ in params]
    for _ in range(3):
        for p in params:
            p.grad = ah.scaled_ints(p.shape, gen).to(DEV)
        grads = [p.grad.cpu() for p in params]
        opt.step()
        for i, p in enumerate(params):
            trails[i][0].append((grads[i].view(-1, 1), None, p.detach().cpu().view(-1, 1)))
            trails[i][1].append(opt.state[p]["sum"].cpu().view(-1, 1))
    worst = {}
    for i, p in enumerate(params):
        assert float(opt.state[p]["step"]) == 3.0
        if p.numel() == 0:
            assert opt.state[p]["sum"].numel() == 0
            continue
        assert not torch.equal(p.detach().cpu(), p0s[i])
        ah.fold(worst, ah.worst_ratios("dense", p0s[i].view(-1, 1), trails[i][0], trails[i][1], LR, EPS["dense"], wd=wd))
    _assert_ratios(worst, f"dense Adagrad wd={wd}")


def test_dense_multi_argument_checks():
    lib = _lib.load()
    p, g, s = (torch.ones(8, device=DEV) for _ in range(3))
    arr = ctypes.c_void_p * 1
    stream = _lib.stream_ptr(p.device)

    def call(pp, gg, ss, numel, count=1):
        return lib.mi_adagrad_dense_multi(pp, gg, ss, (ctypes.c_int64 * 1)(numel), count, LR, 1e-10, 0.0, stream)

    ok = (arr(p.data_ptr()), arr(g.data_ptr()), arr(s.data_ptr()))
    assert call(*ok, 8, count=0) == 0 and call(None, None, None, 8, count=0) == 0
    assert call(*ok, 8, count=-1) == -1 and call(*ok, -1) == -1
    assert call(None, ok[1], ok[2], 8) == -1 and call(arr(None), ok[1], ok[2], 8) == -1
    assert call(arr(None), arr(None), arr(None), 0) == 0                 # a zero-element entry's pointers are not read
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and bool((s == 1).all())
    assert call(*ok, 8) == 0
    assert not bool((p == 1).any()) and bool((s == 2).all())

"""GPU: every optimizer step of csrc/optim.hip against the float64 rule of tests/optim_helpers.py, on gradients that reach
the eps-bound regime (2^-30 next to 2^6 in one row) and on sorted ids whose runs sit on the pass edges of the row-sparse
step.  Sums of duplicates are exact by construction (integers times a power of two), so the coalesce form is compared bit
for bit and the Adam form within the helper's rounding bounds; each test prints its worst ratio to those bounds."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optim_helpers as oh

from recsys_benchmark_amd import _lib
from recsys_benchmark_amd._lib import MI355XLibraryError
from recsys_benchmark_amd.optim import Adam, SparseAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
N_ROWS = 1000
SENTINEL, GAP = -12345.5, 777.25
# (D, vals offset by one float): the float4 widths, D = 1 and 2, two widths of the any-D kernel, and a float4 width whose
# misaligned values send it to the any-D kernel
WIDTHS = [(D, 0) for D in (1, 2, 4, 8, 16, 32, 64, 128, 256, 7, 12)] + [(16, 1)]
WIDTH_IDS = [f"D{D}" + ("-offset" if off else "") for D, off in WIDTHS]


def pass_len(D):
    """Sorted positions per pass of k_sparse_adam<LPR, VW> (the any-D kernel has no passes: it takes the D = 16 layout)."""
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


def _coalesce(ids, perm, vals, offset, N, D):
    """mi_coalesce_rows_sorted into a sentinel-filled G with NaN-filled scratch; returns G on the CPU."""
    n = ids.numel()
    v = _device_vals(vals, offset)
    acc = torch.full((n * D,), float("nan"), device=DEV)
    G = torch.full((N, D), SENTINEL, device=DEV)
    ids_d, perm_d = ids.to(DEV), perm.to(DEV)
    _lib.check(_lib.load().mi_coalesce_rows_sorted(ids_d.data_ptr(), perm_d.data_ptr(), v.data_ptr(), G.data_ptr(), acc.data_ptr(),
                                                   n, D, N, _lib.stream_ptr(G.device)), "mi_coalesce_rows_sorted")
    return G.cpu()


def _check_coalesced(got, ids, perm, vals, N, what):
    want, present = oh.coalesce_ref(ids, perm, vals, N)
    assert torch.equal(got[present].double(), want[present]), f"{what}: coalesced rows differ from the float64 index_add"
    assert bool((got[~present] == SENTINEL).all()), f"{what}: a row that does not occur (or an invalid id) was written"


class _AdamTable:
    """W[N, ldw] (gap columns hold GAP), zero moments and scratch on the device, stepped through mi_sparse_adam_sorted_ld."""

    def __init__(self, p0, ldw):
        self.N, self.D = p0.shape
        self.ldw = ldw
        self.W = torch.full((self.N, ldw), GAP, device=DEV)
        self.W[:, :self.D] = p0.to(DEV)
        self.M = torch.zeros(self.N, self.D, device=DEV)
        self.V = torch.zeros(self.N, self.D, device=DEV)
        self.t = 0

    def step(self, ids_d, perm_d, vals_d, n, on_device):
        self.t += 1
        step_size = LR * math.sqrt(1 - BETAS[1] ** self.t) / (1 - BETAS[0] ** self.t)
        word = torch.tensor([step_size], dtype=torch.float32, device=DEV) if on_device else None
        acc = torch.full((n * self.D,), float("nan"), device=DEV)
        _lib.check(_lib.load().mi_sparse_adam_sorted_ld(
            ids_d.data_ptr(), perm_d.data_ptr(), vals_d.data_ptr(), self.W.data_ptr(), self.ldw, self.M.data_ptr(),
            self.V.data_ptr(), acc.data_ptr(), n, self.D, self.N, 0.0 if on_device else step_size, _lib.ptr(word), BETAS[0],
            BETAS[1], EPS, _lib.stream_ptr(self.W.device)), "mi_sparse_adam_sorted_ld")
        W = self.W.cpu()
        return W[:, :self.D].contiguous(), W[:, self.D:], self.M.cpu(), self.V.cpu()


def _fold(worst, new):
    for k, r in new.items():
        if k not in worst or math.isnan(r) or r > worst[k]:
            worst[k] = r


def _assert_ratios(worst, what):
    print(f"{what}: worst ratio to the bounds " + " ".join(f"{k}={r:.3f}" for k, r in sorted(worst.items())))
    for k, r in worst.items():
        assert r <= 1.0, f"{what}: {r:.2f}x the {k} bound away from the float64 rule"


# ---- the coalesce form: bit-exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,offset", WIDTHS, ids=WIDTH_IDS)
def test_coalesce_form_is_exact_on_pass_edges(D, offset):
    RS = pass_len(D)
    for which in oh.LAYOUTS:
        lay = oh.run_layout(RS, N_ROWS, which)
        gen = torch.Generator().manual_seed(D + 31 * oh.LAYOUTS.index(which))
        vals = torch.randint(-8, 9, (lay.n, D), generator=gen).float()
        got = _coalesce(lay.ids, lay.perm, vals, offset, N_ROWS, D)
        _check_coalesced(got, lay.ids, lay.perm, vals, N_ROWS, f"D={D} {which}")


# ---- the Adam form ------------------------------------------------------------------------------------------------------
def _row_strides(D):
    return {1: (1, 5), 2: (2, 3)}.get(D, (D, D + 4))


@pytest.mark.parametrize("D,offset", WIDTHS, ids=WIDTH_IDS)
def test_adam_form_within_bounds_on_pass_edges(D, offset):
    RS = pass_len(D)
    worst = {}
    for which in oh.LAYOUTS:
        lay = oh.run_layout(RS, N_ROWS, which)
        ids_d, perm_d = lay.ids.to(DEV), lay.perm.to(DEV)
        for ldw in _row_strides(D):
            for on_device in (False, True):
                gen = torch.Generator().manual_seed(1000 * D + 10 * oh.LAYOUTS.index(which) + ldw + on_device)
                p0 = torch.randn(N_ROWS, D, generator=gen)
                table = _AdamTable(p0, ldw)
                steps, moments, touched = [], [], None
                for _ in range(3):
                    vals = oh.scaled_ints((lay.n, D), gen)
                    g, touched = oh.coalesce_ref(lay.ids, lay.perm, vals, N_ROWS)
                    p, gap, m, v = table.step(ids_d, perm_d, _device_vals(vals, offset), lay.n, on_device)
                    assert bool((gap == GAP).all()), f"{which} ldw={ldw}: a gap column of the strided table changed"
                    steps.append((g, touched, p))
                    moments.append((m, v))
                what = f"{which} ldw={ldw} step size {'on the device' if on_device else 'from the host'}"
                p, (m, v) = steps[-1][2], moments[-1]
                assert torch.equal(p[~touched], p0[~touched]), f"{what}: an untouched row of W changed"
                assert not bool(m[~touched].any()) and not bool(v[~touched].any()), f"{what}: an untouched moment row changed"
                _fold(worst, oh.worst_ratios("sparse", p0, steps, moments, LR, BETAS, EPS))
    _assert_ratios(worst, f"sparse Adam D={D}{' (offset vals)' if offset else ''}")


def test_adam_form_rejects_row_strides_it_cannot_take():
    lay = oh.run_layout(16, N_ROWS, "one")
    ids_d, perm_d = lay.ids.to(DEV), lay.perm.to(DEV)
    vals = torch.ones(1, 16, device=DEV)
    p0 = torch.zeros(N_ROWS, 16)
    for ldw, code in ((18, "(-2)"), (12, "(-1)"), (15, "(-1)")):      # unsupported: float4 rows off 16 bytes; invalid: ldw < D
        table = _AdamTable(p0, max(ldw, 16))
        table.ldw = ldw
        with pytest.raises(MI355XLibraryError, match=code.replace("(", r"\(").replace(")", r"\)")):
            table.step(ids_d, perm_d, vals, 1, False)
        assert torch.equal(table.W[:, :16].cpu(), p0) and not bool(table.M.any()) and not bool(table.V.any())


# ---- more tiles than the capped grid has waves ----------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(256, 8192 + 300), (16, 16 * 8192 + 100), (7, 8192 + 300)])
def test_grid_stride_takes_a_second_trip(D, n):
    """kMaxGrid = 2048 workgroups x 4 waves = 8192 waves: tile 8192 is the first wave's second trip, and a run lies across
    the end of tile 8191 (the any-D kernel's tile is one position)."""
    N = 300
    RS = 1 if D == 7 else pass_len(D)
    gen = torch.Generator().manual_seed(D)
    ids, (a, b) = oh.crossing_ids(RS, N, n, 8192, gen)
    assert (n + RS - 1) // RS > 8192 and a // RS <= 8191 and (b - 1) // RS > 8192 and ids[8192 * RS - 1] == ids[8192 * RS]
    perm = torch.randperm(n, generator=gen)
    vals = torch.randint(-8, 9, (n, D), generator=gen).float()
    _check_coalesced(_coalesce(ids, perm, vals, 0, N, D), ids, perm, vals, N, f"D={D} n={n}")
    p0 = torch.randn(N, D, generator=gen)
    table = _AdamTable(p0, D)
    vals = oh.scaled_ints((n, D), gen)
    g, touched = oh.coalesce_ref(ids, perm, vals, N)
    p, _, m, v = table.step(ids.to(DEV), perm.to(DEV), _device_vals(vals, 0), n, False)
    assert torch.equal(p[~touched], p0[~touched])
    _assert_ratios(oh.worst_ratios("sparse", p0, [(g, touched, p)], [(m, v)], LR, BETAS, EPS), f"grid stride D={D} n={n}")


# ---- the SparseAdam class -------------------------------------------------------------------------------------------------
def _sparse_grad(N, D, n, gen):
    rows = (N * torch.rand(n, generator=gen).pow(3)).long().clamp_(max=N - 1)
    vals = oh.scaled_ints((n, D), gen)
    touched = torch.zeros(N, dtype=torch.bool)
    touched[rows] = True
    g = torch.zeros(N, D, dtype=torch.float64).index_add_(0, rows, vals.double())
    return torch.sparse_coo_tensor(rows.view(1, -1).to(DEV), vals.to(DEV), (N, D), check_invariants=False), g, touched


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
@pytest.mark.parametrize("D", [1, 16, 64])
def test_sparse_adam_class_within_bounds(D, capturable):
    N, n = 200, 700
    gen = torch.Generator().manual_seed(5 + D)
    p0 = torch.randn(N, D, generator=gen)
    p = torch.nn.Parameter(p0.to(DEV))
    opt = SparseAdam([p], lr=LR, betas=BETAS, eps=EPS, capturable=capturable)
    steps, moments = [], []
    for _ in range(4):
        p.grad, g, touched = _sparse_grad(N, D, n, gen)
        opt.step()
        steps.append((g, touched, p.detach().cpu()))
        moments.append((opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()))
    assert float(opt.state[p]["step"]) == 4.0
    _assert_ratios(oh.worst_ratios("sparse", p0, steps, moments, LR, BETAS, EPS),
                   f"SparseAdam D={D} {'capturable' if capturable else 'host'}")


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def test_nineteen_capturable_tables_tick_together():
    """19 tables in one capturable group: three tick launches of 8, 8 and 3 slots."""
    gen = torch.Generator().manual_seed(19)
    shapes = [(5 + i, (1, 4, 16)[i % 3]) for i in range(19)]
    ps = [torch.nn.Parameter(torch.randn(*sh, generator=gen).to(DEV)) for sh in shapes]
    opt = SparseAdam(ps, lr=LR, betas=BETAS, eps=EPS, capturable=True)

    def one_step():
        for p, (N, D) in zip(ps, shapes):
            p.grad = _sparse_grad(N, D, 3 * N, gen)[0]
        opt.step()

    def check(t):
        want = LR * math.sqrt(1 - BETAS[1] ** t) / (1 - BETAS[0] ** t)
        for i, p in enumerate(ps):
            assert float(opt.state[p]["step"]) == float(t), f"table {i}: step count {float(opt.state[p]['step'])} after {t}"
            got = float(opt._workspace[(p, "step_size")][0])
            assert abs(got - want) <= _ulp32(want), f"table {i}: step size {got!r} vs {want!r} at t={t}"

    for _ in range(3):
        one_step()
    check(3)
    for p in ps:
        opt.state[p]["step"].fill_(999.0)
    one_step()
    check(1000)


# ---- dense Adam -----------------------------------------------------------------------------------------------------------
SMALL = [33, 5, 1, 4097, 17, 64, 3, 250, 9, 31, 4096, 2, 77, 129, 6, 511, 40, 8, 1025, 12, 95, 7, 300, 21, 4]     # 25 sizes


def _dense_groups(name, wd):
    """[(sizes, lr, betas, eps, wd)] per parameter group; a size given as ("view", s) is a contiguous view one float into
    its buffer (the scalar route of the kernel)."""
    base = (LR, BETAS, EPS, wd)
    if name == "empty-first":
        return [([0] + SMALL, *base)]
    if name == "empty-at-23":
        return [(SMALL[:23] + [0] + SMALL[23:], *base)]
    if name == "hundred":
        return [([1 + (7 * i) % 50 for i in range(100)], *base)]
    if name == "chunk-edges":
        return [([4095, 4096, 4097, 8192, 12289], *base)]
    if name == "offset-views":
        sizes = [10 + i for i in range(30)]
        sizes[3] = sizes[27] = ("view", 4101)
        return [(sizes, *base)]
    if name == "two-groups":
        return [([33, 4097, 5], *base), ([4096, 7, 129], 3e-3, (0.8, 0.99), 1e-6, 1e-2)]
    raise ValueError(name)


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("name", ["empty-first", "empty-at-23", "hundred", "chunk-edges", "offset-views", "two-groups"])
def test_dense_adam_within_bounds(name, wd):
    gen = torch.Generator().manual_seed(len(name))
    groups = _dense_groups(name, wd)
    p0s, params, hyper, opt_groups = [], [], [], []
    for sizes, lr, betas, eps, gwd in groups:
        members = []
        for s in sizes:
            view, s = (True, s[1]) if isinstance(s, tuple) else (False, s)
            p0 = oh.dense_params((s,), gen)
            if view:
                buf = torch.empty(s + 1, device=DEV)
                buf[1:] = p0.to(DEV)
                p = torch.nn.Parameter(buf[1:])
                assert p.data_ptr() % 16 == 4 and p.is_contiguous()
            else:
                p = torch.nn.Parameter(p0.to(DEV))
            p0s.append(p0), params.append(p), members.append(p), hyper.append((lr, betas, eps, gwd))
        opt_groups.append(dict(params=members, lr=lr, betas=betas, eps=eps, weight_decay=gwd))
    opt = Adam(opt_groups)
    # "hundred": a first step over ten tensors only leaves a four-word ticket buffer behind, which the five launches of the
    # full list have to regrow
    plan = ([range(10)] if name == "hundred" else []) + [range(len(params))] * 3
    trails = [([], []) for _ in params]
    for active in plan:
        for i, p in enumerate(params):
            p.grad = oh.scaled_ints(p.shape, gen).to(DEV) if i in active else None
        grads = [None if p.grad is None else p.grad.cpu() for p in params]
        opt.step()
        for i in active:
            p = params[i]
            trails[i][0].append((grads[i], None, p.detach().cpu()))
            trails[i][1].append((opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()))
    worst = {}
    for i, p in enumerate(params):
        count = sum(i in active for active in plan)
        assert float(opt.state[p]["step"]) == float(count), \
            f"tensor {i} ({p.numel()} elements): step count {float(opt.state[p]['step'])} after {count} steps"
        lr, betas, eps, gwd = hyper[i]
        _fold(worst, oh.worst_ratios("dense", p0s[i], trails[i][0], trails[i][1], lr, betas, eps, gwd))
    if name == "hundred":
        assert opt._ticket_buf.numel() >= 5
    assert not bool(opt._ticket_buf.any()), "a completion ticket was left armed"
    _assert_ratios(worst, f"dense Adam {name} wd={wd}")


def test_dense_multi_without_tickets_matches_the_ticket_path():
    """mi_adam_dense_multi with tickets = NULL (a second small launch advances the counts) against the ticket path, on 26
    tensors with a zero-element one inside the first 24: two launches each, bit-equal tensors and counts."""
    lib = _lib.load()
    sizes = SMALL[:23] + [0] + SMALL[23:]
    n = len(sizes)
    gen = torch.Generator().manual_seed(26)
    p0 = [oh.dense_params((s,), gen) for s in sizes]
    g = [oh.scaled_ints((s,), gen).to(DEV) for s in sizes]
    arr = ctypes.c_void_p * n
    results = []
    for with_tickets in (True, False):
        p = [t.to(DEV) for t in p0]
        m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
        steps = [torch.zeros((), device=DEV) for _ in p]
        tickets = torch.zeros(4, dtype=torch.int32, device=DEV) if with_tickets else None
        for _ in range(2):
            _lib.check(lib.mi_adam_dense_multi(arr(*[t.data_ptr() for t in p]), arr(*[t.data_ptr() for t in g]),
                                               arr(*[t.data_ptr() for t in m]), arr(*[t.data_ptr() for t in v]),
                                               arr(*[t.data_ptr() for t in steps]), (ctypes.c_int64 * n)(*sizes), n, LR,
                                               BETAS[0], BETAS[1], EPS, 1e-3, _lib.ptr(tickets), _lib.stream_ptr(p[0].device)),
                       "mi_adam_dense_multi")
        results.append(([t.cpu() for t in p + m + v], [float(s) for s in steps]))
        if with_tickets:
            assert not bool(tickets.any())
    assert results[0][1] == results[1][1] == [0.0 if s == 0 else 2.0 for s in sizes]      # (empty entries are skipped)
    for a, b in zip(results[0][0], results[1][0]):
        assert torch.equal(a, b)
    assert all(not torch.equal(a, b) for a, b in zip(results[0][0][:n], p0) if b.numel())    # (and every tensor did move)


# ---- row-sparse SGD -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 7, 16])
def test_scatter_axpy_rows_is_exact_and_skips_invalid_ids(D):
    N, n = 37, 1000
    gen = torch.Generator().manual_seed(D)
    idx = torch.randint(-1, N + 1, (n,), generator=gen)                 # -1 and N mixed in
    assert bool((idx == -1).any()) and bool((idx == N).any())
    g = torch.randint(-8, 9, (n, D), generator=gen).float()
    W0 = torch.randint(-100, 101, (N, D), generator=gen).float()
    W = W0.to(DEV)
    idx_d, g_d = idx.to(DEV), g.to(DEV)
    _lib.check(_lib.load().mi_scatter_axpy_rows(idx_d.data_ptr(), g_d.data_ptr(), -2.0 ** -3, W.data_ptr(), n, D, N,
                                                _lib.stream_ptr(W.device)), "mi_scatter_axpy_rows")
    ok = (idx >= 0) & (idx < N)
    want = W0.double().index_add_(0, idx[ok], g[ok].double(), alpha=-2.0 ** -3)
    assert torch.equal(W.cpu().double(), want)

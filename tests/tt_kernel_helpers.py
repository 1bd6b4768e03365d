"""Float64 / integer restatements of the grouped TT-Rec lookup's pieces (csrc/tt_grouped.hip and the two grouped GEMM
entries of csrc/gemm.hip), written in plain torch without the library, and the case tables that tests/test_tt_kernels_host.py
(proves the restatements against oracle.reference_ops.tt_forward) and tests/test_tt_kernels_gpu.py (holds every entry point to
them, bit for bit on integer-valued data) share.

Buffers are FLAT, as the C-ABI sees them: a "row" is `row * stride`, a lookup's chunk may span several rows of a layout.
Every function takes and returns CPU tensors; float work is float64."""
import torch

TILE = 64                  # rows per GEMM tile (_kernels._TT_TILE)
SEG, SEG0, SEG_LAST = 2048, 256, 16      # _kernels._TT_SEG, _TT_SEG0, the last level's segment in TTLookupGrouped.backward
EXACT = float(1 << 24)     # integers below this magnitude are exact in float32, and so is every sum that stays below it


def prod(xs):
    r = 1
    for x in xs:
        r *= int(x)
    return r


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------- digits
def digits(idx, N, p_shapes):
    """(digits int32 [ncores, n], valid uint8 [n]): mixed-radix digits over p_shapes, most significant first; an id outside
    [0, N) has all digits 0 and valid 0."""
    idx = idx.reshape(-1).to(torch.int64)
    ok = (idx >= 0) & (idx < N)
    rest = torch.where(ok, idx, torch.zeros_like(idx))
    big = prod(p_shapes)
    out = []
    for p in p_shapes:
        big //= int(p)
        out.append(torch.div(rest, big, rounding_mode="floor").to(torch.int32))
        rest = rest % big
    return torch.stack(out), ok.to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ plan
class Plan:
    """Layout of one level for a digit vector: groups in digit order, H rows per lookup, each group padded to whole tiles.
    rows[p], pbeg[p] (padded beginnings), mtile_b[ntiles] (-1 past the last group), kseg[nseg, 3] = (first row, rows, group) in
    canonical order (groups ascending, a group's segments ascending) with zero rows after the live ones, and `pos`: one valid
    assignment of first rows (arrival = index order; any order inside a group is valid)."""

    def __init__(self, digit, p, H, seg):
        digit = digit.reshape(-1).to(torch.int64)
        n = digit.numel()
        self.p, self.H, self.seg, self.n = p, H, seg, n
        self.counts = torch.bincount(digit, minlength=p)
        self.rows = self.counts * H
        rpad = (self.rows + TILE - 1) // TILE * TILE
        self.pend = torch.cumsum(rpad, 0)
        self.pbeg = self.pend - rpad
        self.ntiles = (n * H + TILE - 1) // TILE + p
        self.mpad = self.ntiles * TILE
        self.nseg = (n * H + seg - 1) // seg + p
        groups = torch.arange(p)
        self.mtile_b = torch.full((self.ntiles,), -1, dtype=torch.int32)
        used = torch.repeat_interleave(groups, rpad // TILE)               # a group's tiles, groups ascending
        self.mtile_b[:used.numel()] = used.to(torch.int32)
        chunks = (self.rows + seg - 1) // seg                               # segments of <= seg rows, none across a group
        g_j = torch.repeat_interleave(groups, chunks)
        self.live = g_j.numel()
        k0 = (torch.arange(self.live) - torch.repeat_interleave(torch.cumsum(chunks, 0) - chunks, chunks)) * seg
        self.kseg = torch.zeros((self.nseg, 3), dtype=torch.int64)
        self.kseg[:self.live] = torch.stack([self.pbeg[g_j] + k0, torch.clamp(self.rows[g_j] - k0, max=seg), g_j], 1)
        rank = torch.zeros(n, dtype=torch.int64)
        order = torch.sort(digit, stable=True)[1]
        starts = torch.cumsum(self.counts, 0) - self.counts
        rank[order] = torch.arange(n) - starts[digit[order]]
        self.pos = self.pbeg[digit] + rank * H


# ------------------------------------------------------------------------------------------------------------------ move
def _cells(row, stride, width, n):
    row = torch.arange(n) if row is None else row.reshape(-1).to(torch.int64)
    return row[:, None] * stride + torch.arange(width)[None, :]


def move(src, src_row, src_stride, dst, dst_row, dst_stride, width, n, mask=None, accumulate=False):
    """dst[dst_row[i]*dst_stride + e] (=|+=) src[src_row[i]*src_stride + e], e < width, in place on the flat `dst`.
    A masked-out row (mask[i] == 0) is written as zeros without accumulate and skipped with it.  Null rows = identity."""
    v = src.reshape(-1)[_cells(src_row, src_stride, width, n)].to(dst.dtype)
    cells = _cells(dst_row, dst_stride, width, n)
    flat = dst.view(-1)
    if mask is not None:
        keep = mask.reshape(-1).bool()
        if accumulate:
            v, cells = v[keep], cells[keep]
        else:
            v = torch.where(keep[:, None], v, torch.zeros_like(v))
    if accumulate:
        flat.index_add_(0, cells.reshape(-1), v.reshape(-1))
    else:
        flat[cells.reshape(-1)] = v.reshape(-1)
    return dst


def segment_sum(X, ldx, width, kseg, out, ldo):
    """out[slice*ldo + col] += sum_{r < rows} X[(first + r)*ldx + col], col < width, per (first, rows, slice) of kseg."""
    Xf, of = X.reshape(-1), out.view(-1)
    for first, rows, g in kseg.tolist():
        if rows <= 0:
            continue
        blk = torch.as_strided(Xf, (rows, width), (ldx, 1), first * ldx)
        of[g * ldo:g * ldo + width] += blk.sum(0).to(out.dtype)
    return out


# ----------------------------------------------------------------------------------------------------------------- GEMMs
def gemm_row_groups(A, B, C, M, N, K, lda, ldb, ldc, transB, sB, mtile_b):
    """C[tile rows, :N] = A[tile rows, :K] @ B_g (B_g = [K, N] rows of ldb) or @ B_g^T (B_g = [N, K]), g = mtile_b[tile];
    tiles with g < 0 are not touched."""
    Af, Bf, Cf = A.reshape(-1), B.reshape(-1), C.view(-1)
    for t, g in enumerate(mtile_b.tolist()):
        m0 = t * TILE
        if g < 0 or m0 >= M:
            continue
        m = min(TILE, M - m0)
        a = torch.as_strided(Af, (m, K), (lda, 1), m0 * lda).double()
        if transB:
            b = torch.as_strided(Bf, (N, K), (ldb, 1), g * sB).double().t()
        else:
            b = torch.as_strided(Bf, (K, N), (ldb, 1), g * sB).double()
        torch.as_strided(Cf, (m, N), (ldc, 1), m0 * ldc).copy_((a @ b).to(C.dtype))
    return C


def gemm_k_groups(A, B, C, M, N, lda, ldb, ldc, sC, kseg):
    """C[slice] (M x N, rows of ldc, slices sC apart) += A[rows, :M]^T @ B[rows, :N] per (first, rows, slice) of kseg."""
    Af, Bf, Cf = A.reshape(-1), B.reshape(-1), C.view(-1)
    for first, rows, g in kseg.tolist():
        if rows <= 0:
            continue
        a = torch.as_strided(Af, (rows, M), (lda, 1), first * lda).double()
        b = torch.as_strided(Bf, (rows, N), (ldb, 1), first * ldb).double()
        c = torch.as_strided(Cf, (M, N), (ldc, 1), g * sC)
        c += (a.t() @ b).to(C.dtype)
    return C


# ------------------------------------------------------------------------------------------------------------ last level
def _last_operands(src, src_row, src_stride, core, digit, H, K, q):
    n = digit.numel()
    chunk = src.reshape(-1)[_cells(src_row, src_stride, H * K, n)].double().view(n, H, K)
    sl = core.reshape(-1, K, q).double()[digit.reshape(-1).to(torch.int64)]             # [n, K, q]
    return chunk, sl


def _keep(valid, n):
    return torch.ones(n, dtype=torch.bool) if valid is None else valid.reshape(-1).bool()


def last_fwd(src, src_row, src_stride, core, digit, valid, H, K, q):
    """out[l, h*q + j] = sum_k chunk_l[h, k] core[i_l][k, j]; rows of invalid lookups are zero."""
    chunk, sl = _last_operands(src, src_row, src_stride, core, digit, H, K, q)
    out = torch.einsum("lhk,lkj->lhj", chunk, sl).reshape(-1, H * q)
    return torch.where(_keep(valid, out.shape[0])[:, None], out, torch.zeros_like(out))


def last_bwd_in(core, digit, valid, H, K, q, g):
    """dchunk[l, h*K + k] = sum_j g[l, h*q + j] core[i_l][k, j]; rows of invalid lookups are zero whatever g holds."""
    n = digit.numel()
    sl = core.reshape(-1, K, q).double()[digit.reshape(-1).to(torch.int64)]
    keep = _keep(valid, n)
    gg = torch.where(keep[:, None], g.reshape(n, H * q).double(), torch.zeros(n, H * q, dtype=torch.float64))
    return torch.einsum("lhj,lkj->lhk", gg.view(n, H, q), sl).reshape(n, H * K)


def last_bwd_core(src, src_row, src_stride, core_shape, digit, valid, H, K, q, g):
    """gcore[i][k, j] = sum over VALID lookups l with i_l = i of sum_h chunk_l[h, k] g[l, h*q + j] (float64 [p, K, q])."""
    n = digit.numel()
    keep = _keep(valid, n)
    chunk = src.reshape(-1)[_cells(src_row, src_stride, H * K, n)].double().view(n, H, K)[keep]
    gg = g.reshape(n, H, q).double()[keep]
    out = torch.zeros(core_shape, dtype=torch.float64).reshape(-1, K, q)
    out.index_add_(0, digit.reshape(-1).to(torch.int64)[keep], torch.einsum("lhk,lhj->lkj", chunk, gg))
    return out


# ------------------------------------------------------------------------------------------- the chain of TTLookupGrouped
def last_fast(H, K, q):
    D = H * q
    return D <= 64 and 64 % D == 0 and K * q <= 512 and H * K <= 512


def grouped_supported(qs, ranks):
    H = 1
    for c in range(len(qs)):
        H *= qs[c]
        if (qs[c] * ranks[c + 1]) % 4 or (c > 0 and ranks[c] % 4):
            return False
    return len(qs) >= 2 and H % 4 == 0


def grouped_forward(idx, N, ps, qs, ranks, cores):
    """The restatements chained level by level as TTLookupGrouped.forward chains the kernels.  Buffers start as NaN: a finite
    result proves that the chain reads only what it wrote.  Returns (out [n, D], ctx)."""
    nc, n = len(ps), idx.numel()
    dg, valid = digits(idx, N, ps)
    cs = [c.detach().double().reshape(-1) for c in cores]
    Hs = [1]
    for q in qs:
        Hs.append(Hs[-1] * q)
    D, last = Hs[-1], nc - 1
    fast = last_fast(Hs[last], ranks[last], qs[last])
    levels = list(range(1, last if fast else nc))
    plans = {c: Plan(dg[c], ps[c], Hs[c], SEG) for c in levels}
    d0, w0 = dg[0].to(torch.int64), qs[0] * ranks[1]
    out = nan(n, D)
    As = []
    src, src_row, src_stride = cs[0], d0, w0
    if levels:
        A = nan(plans[1].mpad * ranks[1])
        move(cs[0], d0, w0, A, plans[1].pos, ranks[1], w0, n, mask=valid)
    for c in levels:
        K, Nn = ranks[c], qs[c] * ranks[c + 1]
        C = nan(plans[c].mpad * Nn)
        gemm_row_groups(A, cs[c], C, plans[c].mpad, Nn, K, K, Nn, Nn, 0, K * Nn, plans[c].mtile_b)
        As.append(A)
        width = Hs[c] * Nn
        if c + 1 in plans:
            A = nan(plans[c + 1].mpad * ranks[c + 1])
            move(C, plans[c].pos, Nn, A, plans[c + 1].pos, ranks[c + 1], width, n)
        elif c == last:
            move(C, plans[c].pos, Nn, out, None, D, width, n)
        else:
            src, src_row, src_stride = C, plans[c].pos, Nn
    if fast:
        out = last_fwd(src, src_row, src_stride, cs[last], dg[last], valid, Hs[last], ranks[last], qs[last])
    ctx = dict(dg=dg, valid=valid, cs=cs, As=As, plans=plans, Hs=Hs, fast=fast, last_src=(src, src_row, src_stride), n=n,
               shapes=[tuple(c.shape) for c in cores])
    return out, ctx


def grouped_backward(ctx, g, ps, qs, ranks):
    """TTLookupGrouped.backward with the restatements: the core gradients, float64, shaped like the cores."""
    dg, valid, cs, As, plans, Hs, fast, n = (ctx[k] for k in ("dg", "valid", "cs", "As", "plans", "Hs", "fast", "n"))
    nc = len(ps)
    last, D = nc - 1, Hs[-1]
    g = g.double().reshape(n, D)
    gcs = [torch.zeros_like(c) for c in cs]
    d0, w0 = dg[0].to(torch.int64), qs[0] * ranks[1]
    plan0 = X = dC = None

    def level0():
        nonlocal plan0, X
        plan0 = Plan(dg[0], ps[0], 1, SEG0)
        X = nan(plan0.mpad * w0)

    if fast:
        H, K, q = Hs[last], ranks[last], qs[last]
        src, src_row, src_stride = ctx["last_src"]
        din = last_bwd_in(cs[last], dg[last], valid, H, K, q, g)
        if nc == 2:
            level0()
            move(din, None, H * K, X, plan0.pos, w0, H * K, n)
        else:
            Np = qs[last - 1] * ranks[last]
            dC = nan(plans[last - 1].mpad * Np)
            move(din, None, H * K, dC, plans[last - 1].pos, Np, H * K, n)
        gcs[last] += last_bwd_core(src, src_row, src_stride, (ps[last], K, q), dg[last], valid, H, K, q, g).reshape(-1)
        top = last - 1
    else:
        N_last = qs[last] * ranks[last + 1]
        dC = nan(plans[last].mpad * N_last)
        move(g, None, D, dC, plans[last].pos, N_last, D, n, mask=valid)
        top = last
    for c in range(top, 0, -1):
        K, Nn = ranks[c], qs[c] * ranks[c + 1]
        gemm_k_groups(As[c - 1], dC, gcs[c], K, Nn, K, Nn, Nn, K * Nn, plans[c].kseg)
        dA = nan(plans[c].mpad * K)
        gemm_row_groups(dC, cs[c], dA, plans[c].mpad, K, Nn, Nn, Nn, K, 1, K * Nn, plans[c].mtile_b)
        width = Hs[c] * K
        if c > 1:
            Np = qs[c - 1] * ranks[c]
            dC = nan(plans[c - 1].mpad * Np)
            move(dA, plans[c].pos, K, dC, plans[c - 1].pos, Np, width, n)
        else:
            level0()
            move(dA, plans[1].pos, K, X, plan0.pos, w0, w0, n, mask=valid)
    segment_sum(X, w0, w0, plan0.kseg, gcs[0], w0)
    return [gc.view(s) for gc, s in zip(gcs, ctx["shapes"])]


# ---------------------------------------------------------------------------------------------------------- case tables
def ints(shape, gen):
    """Integer-valued operands drawn like test_gemm_gpu._mk: [-3, 3], asymmetric around 0 in no dimension."""
    return torch.randint(-3, 4, shape, generator=gen).double()


# (H, K, q) of the last-level kernels: D in {4, 8, 16, 32, 64}, every U = ceil(K*q / 64) from 1 to 8, H*K = 512 and K*q = 512,
# and k-ranges that leave lanes idle or short (K/4 not a multiple of 64/D)
LAST_SHAPES = [(1, 4, 4), (1, 16, 4), (2, 8, 4), (4, 20, 4), (4, 32, 4), (4, 48, 4), (4, 64, 4), (4, 80, 4), (4, 96, 4), (4, 112, 4),
               (4, 128, 4), (2, 64, 8), (8, 16, 4), (16, 8, 4), (8, 64, 8)]
LAST_N = [1, 3, 5]
LAST_N_BIG = 8192 + 67                    # past grid_for_waves' cap of 8192 waves: the second trip of every wave loop
LAST_SEG_COUNTS = [1, 2, 16, 17]

ROW_GROUP_N = [4, 64, 68, 384]
ROW_GROUP_K = [4, 12, 32, 36, 96, 132]
K_GROUP_MN = [(8, 8), (128, 384), (96, 4), (4, 96), (12, 20), (6, 8)]
K_GROUP_SEGS = [0, 1, 31, 32, 33, 2048]
MOVE_WIDTHS = [4, 8, 36, 384]
MOVE_DUPLICATES = 4096                    # lookups accumulated into one destination row
SEGSUM_WIDTHS = [4, 255, 256, 257, 600]
SEGSUM_LENGTHS = [0, 1, 3, 4, 5, 256]


def exact_bounds():
    """{case: largest magnitude any partial sum can reach} for the integer-valued GPU checks, from each case's own sizes with
    |operand| <= 3: a product term is at most 9, a copied or summed value at most 3."""
    b = {}
    for H, K, q in LAST_SHAPES:
        b[f"last_fwd {H, K, q}"] = 9 * K
        b[f"last_bwd_in {H, K, q}"] = 9 * q
        # a slice's gradient sums H terms per lookup over every lookup of the call (all may share one digit), on top of a
        # pre-filled value
        b[f"last_bwd_core {H, K, q}"] = 3 + 9 * H * LAST_N_BIG
    for K in ROW_GROUP_K:
        b[f"row_groups K={K}"] = 9 * K
    # every segment of the call may land in one slice, on top of the pre-filled integer
    b["k_groups"] = 3 + 9 * (sum(K_GROUP_SEGS) + 2 * max(K_GROUP_SEGS))
    b["move accumulate"] = 3 + 3 * MOVE_DUPLICATES
    b["segment_sum"] = 3 + 3 * (sum(SEGSUM_LENGTHS) + 2 * max(SEGSUM_LENGTHS))
    return b


# End to end: every branch of TTLookupGrouped.  N = 20000 rows, n = 4500 lookups; (name, fast last, ps, qs, ranks between cores)
E2E_N, E2E_n, E2E_n_BIG = 20000, 4500, 8192 + 70
E2E_CASES = [
    ("fast2-D4", True, [200, 100], [1, 4], [16]),
    ("fast2-D8", True, [200, 100], [2, 4], [32]),
    ("fast2-D64", True, [200, 100], [8, 8], [64]),
    ("fast3-D32", True, [25, 25, 32], [2, 4, 4], [8, 48]),
    ("fast3-D64", True, [25, 25, 32], [4, 4, 4], [8, 16]),
    ("fast3-HK512", True, [25, 25, 32], [2, 2, 4], [8, 128]),
    ("gemm2-D48", False, [200, 100], [4, 12], [8]),
    ("gemm2-D128", False, [200, 100], [16, 8], [8]),
    ("gemm3-HK528", False, [25, 25, 32], [2, 2, 4], [8, 132]),
    ("gemm4-D128", False, [10, 10, 20, 10], [2, 2, 4, 8], [8, 8, 8]),
]
E2E_BIG = ["fast3-D32", "gemm3-HK528"]          # run again at n = 8192 + 70
E2E_BAD_IDS = ["fast3-D64", "gemm2-D48"]        # run with out-of-range ids and a NaN upstream gradient on their rows
E2E_TOL = dict(fwd=(1e-4, 1e-5), grad=(1e-3, 1e-4))


def e2e_case(name):
    return next(c for c in E2E_CASES if c[0] == name)


def e2e_inputs(name, n=E2E_n, seed=11):
    """(cores float32 [1, p, r*q*r'] drawn like test_tt_grouped_gpu._emb, idx [n], G [n, D], full ranks) of a table row."""
    _, fast, ps, qs, mid = e2e_case(name)
    ranks = [1] + list(mid) + [1]
    gen = torch.Generator().manual_seed(seed)
    cores = [torch.randn(1, ps[c], ranks[c] * qs[c] * ranks[c + 1], generator=gen) * 0.1 for c in range(len(ps))]
    idx = torch.randint(0, E2E_N, (n,), generator=gen)
    G = torch.randn(n, prod(qs), generator=gen)
    return cores, idx, G, ranks


def tol_fraction(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): below 1 exactly when torch.testing.assert_close passes."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())

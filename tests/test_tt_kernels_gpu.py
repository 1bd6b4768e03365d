"""GPU: every entry point behind the grouped TT-Rec lookup through the C-ABI, at its own edges and off the D = 16 path that
tests/test_tt_grouped_gpu.py walks: mi_tt_digits, mi_tt_plan_level, mi_move_chunks, mi_segment_sum, mi_tt_last_fwd / _bwd
(csrc/tt_grouped.hip) and mi_gemm_f32_row_groups / _k_groups (csrc/gemm.hip), each against its restatement in
tests/tt_kernel_helpers.py (proved against the oracle by tests/test_tt_kernels_host.py).

Kernel checks use integer-valued operands in [-3, 3]: every partial sum stays below 2^24 (asserted per case by the host file),
so the float32 result is exact in ANY summation order and must be bit-equal (torch.equal) to the float64 restatement whatever
order the float atomics arrive in.  Output buffers start as NaN (or as integers where the entry accumulates): a cell the
kernel does not own must still hold what it held.

The end-to-end half runs TTRecTorch through every branch of TTLookupGrouped (fast last level / last level as a GEMM, 2-4
cores) against oracle tt_forward in float64 with test_tt_grouped_gpu._check's tolerances, and asserts from kernel records
that the branch it names is the branch that ran."""
import ctypes

import pytest
import torch

import tt_kernel_helpers as H
from oracle import reference_ops as ro
from recsys_benchmark_amd import _kernels, _lib
from recsys_benchmark_amd.embeddings import TTRecTorch
from recsys_benchmark_amd.profiling import KernelTimer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OK, INVALID, UNSUPPORTED = 0, -1, -2
NAN = float("nan")


@pytest.fixture(autouse=True)
def _clean_error_word():
    """A test that fails between raising the sticky out-of-range word and reading it must not fail the next one."""
    yield
    _lib.err_word(DEV).zero_()


def _stream():
    return _lib.stream_ptr(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _f32(t):
    """A float64 CPU tensor of integers (and NaN sentinels) as a float32 device buffer."""
    return t.to(torch.float32).to(DEV).contiguous()


def _same(got, want, what=""):
    """Bit-equal, sentinels included: NaN exactly where the restatement left NaN, and torch.equal everywhere else."""
    got = got.detach().cpu().double().reshape(-1)
    want = want.detach().cpu().double().reshape(-1)
    assert got.shape == want.shape, what
    assert torch.equal(got.isnan(), want.isnan()), f"{what}: a cell the kernel does not own changed, or an owned cell was not written"
    assert torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0)), \
        f"{what}: max abs diff {float((got.nan_to_num(0.0) - want.nan_to_num(0.0)).abs().max())}"


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 1009 * int(s) for i, s in enumerate(seed)) + 5)


# ================================================================================================================ digits
def _run_digits(idx, N, ps, with_valid, with_err):
    n, nc = idx.numel(), len(ps)
    d = torch.full((nc, n), -77, dtype=torch.int32, device=DEV)
    v = torch.full((n,), 9, dtype=torch.uint8, device=DEV) if with_valid else None
    e = torch.zeros(1, dtype=torch.int32, device=DEV) if with_err else None
    ids = idx.to(DEV)
    rc = _lib.load().mi_tt_digits(ids.data_ptr(), n, N, (ctypes.c_int32 * nc)(*ps), nc, d.data_ptr(), _p(v), _p(e), _stream())
    assert rc == OK
    return d.cpu(), None if v is None else v.cpu(), None if e is None else int(e.item())


@pytest.mark.parametrize("ps", [[7], [1], [5, 1], [3, 4, 5], [2, 1, 3, 4], [40, 50, 30, 20]])
def test_digits_every_core_count_and_bad_ids(ps):
    big = H.prod(ps)
    N = big - 2 if big > 4 else big                        # N < prod(p): ids in [N, prod(p)) have digits but are out of range
    bad_ids = [N, -1, 1 << 40] + ([N + 1] if N < big else [])
    for n in (1, 255, 256, 257, 2048 * 256 + 3):           # the last: one trip past kMaxGrid * kBlock threads
        gen = _gen(n, len(ps), big)
        clean = torch.randint(0, N, (n,), generator=gen)
        clean[0], clean[-1] = 0, N - 1
        batches = [("clean", clean)]
        if n == 1:
            batches += [("last id", torch.tensor([N - 1]))] + [(f"bad {b}", torch.tensor([b])) for b in bad_ids]
        else:
            dirty = clean.clone()
            for j, b in enumerate(bad_ids):
                dirty[(3 + 61 * j) % n] = b
            dirty[n - 2] = N                               # in the tail past the last full workgroup
            batches.append(("dirty", dirty))
        for what, idx in batches:
            want_d, want_v = H.digits(idx, N, ps)
            for with_valid, with_err in ((True, True), (False, False), (True, False), (False, True)):
                d, v, e = _run_digits(idx, N, ps, with_valid, with_err)
                assert torch.equal(d, want_d), (what, n)
                if with_valid:
                    assert torch.equal(v, want_v), (what, n)
                if with_err:
                    assert e == (0 if bool(want_v.all()) else 1), (what, n)      # set exactly when a bad id is present


# ================================================================================================================= plan
def _run_plan(digit, p, Hh, seg, ntiles=None, nseg=None):
    n = digit.numel()
    pl = H.Plan(digit, p, Hh, seg)
    ntiles = pl.ntiles if ntiles is None else ntiles
    nseg = pl.nseg if nseg is None else nseg
    ws = torch.full((2 * p,), -5, dtype=torch.int32, device=DEV)
    pbeg = torch.full((p,), -5, dtype=torch.int64, device=DEV)
    pos = torch.full((max(n, 1),), -5, dtype=torch.int64, device=DEV)
    mt = torch.full((max(ntiles, 1),), -5, dtype=torch.int32, device=DEV)
    ks = torch.full((max(nseg, 1), 3), -5, dtype=torch.int64, device=DEV)
    dd = digit.to(torch.int32).to(DEV)
    rc = _lib.load().mi_tt_plan_level(dd.data_ptr(), n, p, Hh, seg, ws.data_ptr(), pbeg.data_ptr(),
                                      pos.data_ptr(), mt.data_ptr(), ntiles, ks.data_ptr(), nseg, _stream())
    return rc, pl, ws.cpu(), pbeg.cpu(), pos.cpu()[:n], mt.cpu()[:ntiles], ks.cpu()[:nseg]


def _check_plan(digit, p, Hh, seg, what):
    rc, pl, ws, pbeg, pos, mt, ks = _run_plan(digit, p, Hh, seg)
    assert rc == OK, what
    d = digit.long()
    assert torch.equal(ws[:p].long(), pl.counts) and torch.equal(ws[p:].long(), pl.counts), f"{what}: counts / cursors"
    assert torch.equal(pbeg, pl.pbeg), f"{what}: padded beginnings"
    assert torch.equal(mt, pl.mtile_b), f"{what}: tile map"
    assert torch.equal(ks[:pl.live], pl.kseg[:pl.live]), f"{what}: live segments"
    assert not bool(ks[pl.live:, 1].any()), f"{what}: a segment past the live ones has rows"
    assert pos.unique().numel() == digit.numel(), f"{what}: two lookups share a row"
    assert not bool((pos % Hh).any()), what
    assert bool((pos >= pl.pbeg[d]).all()) and bool((pos + Hh <= pl.pbeg[d] + pl.rows[d]).all()), f"{what}: a row outside its group"


def _plan_digit_vectors(p, Hh, seg, gen):
    """(name, digit) pairs: the shapes of a digit vector at which a counting sort, a scan or a padding rule goes wrong."""
    top = p - 1
    out = []
    for n in (1, 63, 64, 65):
        out.append((f"uniform n={n}", torch.randint(0, p, (n,), generator=gen)))
        out.append((f"one group n={n}", torch.full((n,), top)))
    n = 5000
    out.append(("uniform n=5000", torch.randint(0, p, (n,), generator=gen)))
    out.append(("skewed n=5000", (p * torch.rand(n, generator=gen) ** 6).long().clamp_(0, top)))
    out.append(("one group n=5000", torch.full((n,), top)))
    some = torch.tensor(sorted({0, p // 2, top}))
    out.append(("most groups empty", some[torch.randint(0, some.numel(), (n,), generator=gen)]))
    if Hh <= 64:                                          # a group of exactly 64 / H lookups: one tile, no padding
        out.append(("exact tile", torch.cat([torch.zeros(64 // Hh), torch.full((70,), top)]).long()))
    if p >= 4 and seg % Hh == 0 and 4 * seg // Hh + 8 <= 9000:
        # groups whose rows are exactly seg, the next size above seg (seg + 1 when H = 1) and 2 * seg; the top group populated
        c = seg // Hh
        parts = [torch.full((c,), 0), torch.full((c + 1,), 1), torch.full((2 * c,), 2), torch.full((3,), top)]
        v = torch.cat(parts).long()
        out.append(("rows seg / seg+H / 2 seg", v[torch.randperm(v.numel(), generator=gen)]))
    return out


@pytest.mark.parametrize("p", [1, 37, 1024, 1025, 4096])
def test_plan_level_against_the_plan_invariants(p):
    """p > 1024 puts entries on lanes u >= 1 of the scan's four per thread; 1025 and 4096 are its first and last such size."""
    for Hh in (1, 4, 16):
        for seg in (16, 256, 2048):
            gen = _gen(p, Hh, seg)
            vectors = _plan_digit_vectors(p, Hh, seg, gen)
            if (Hh, seg) not in ((1, 16), (4, 256), (16, 2048), (1, 2048)):      # the full set on a diagonal, the rest pruned
                vectors = [v for v in vectors if v[0] in ("uniform n=5000", "exact tile", "rows seg / seg+H / 2 seg", "uniform n=65")]
            for name, digit in vectors:
                _check_plan(digit, p, Hh, seg, f"p={p} H={Hh} seg={seg} {name}")


def test_plan_level_declines():
    gen = _gen(3)
    digit = torch.randint(0, 37, (500,), generator=gen)
    pl = H.Plan(digit, 37, 2, 16)
    for kw, want in ((dict(ntiles=pl.ntiles - 1), INVALID), (dict(nseg=pl.nseg - 1), INVALID)):
        rc, _, ws, pbeg, pos, mt, ks = _run_plan(digit, 37, 2, 16, **kw)
        assert rc == want
        for t in (ws, pbeg, pos, mt, ks):
            assert bool((t == -5).all()), "a declined call wrote"
    rc, _, ws, pbeg, pos, mt, ks = _run_plan(torch.randint(0, 4097, (500,), generator=gen), 4097, 2, 16)
    assert rc == UNSUPPORTED
    for t in (ws, pbeg, pos, mt, ks):
        assert bool((t == -5).all()), "a declined call wrote"


# ================================================================================================================= move
def _run_move(src, src_row, ss, dst, dst_row, ds, width, n, mask, acc, src_off=0, dst_off=0):
    s, d = _f32(src), _f32(dst)
    sr = None if src_row is None else src_row.to(DEV)
    dr = None if dst_row is None else dst_row.to(DEV)
    m = None if mask is None else mask.to(torch.uint8).to(DEV)
    rc = _lib.load().mi_move_chunks(s.data_ptr() + 4 * src_off, _p(sr), ss, d.data_ptr() + 4 * dst_off, _p(dr), ds, width, n, _p(m),
                                    int(acc), _stream())
    return rc, d.cpu()


@pytest.mark.parametrize("width", H.MOVE_WIDTHS)
def test_move_chunks_rows_masks_and_accumulate(width):
    n, ss, ds = 37, width + 4, width + 8
    for rows in ("both", "src null", "dst null"):
        for masked in (False, True):
            for acc in (False, True):
                gen = _gen(width, masked, acc, len(rows))
                nsrc = n if rows == "src null" else 11
                src = H.ints((nsrc * ss,), gen)
                src_row = None if rows == "src null" else torch.randint(0, nsrc, (n,), generator=gen)
                if rows == "dst null":
                    ndst, dst_row = n, None
                elif acc:
                    ndst, dst_row = 9, torch.randint(0, 7, (n,), generator=gen)            # duplicates, two rows never named
                else:
                    ndst = n + 5
                    dst_row = torch.randperm(ndst, generator=gen)[:n]
                dst = H.ints((ndst * ds,), gen) if acc else H.nan(ndst * ds)
                mask = (torch.rand(n, generator=gen) < 0.6) if masked else None
                want = H.move(src, src_row, ss, dst.clone(), dst_row, ds, width, n, mask, acc)
                if masked and not acc:
                    assert float(want.nan_to_num(1.0).abs().min()) == 0.0                   # masked rows: written, as zeros
                rc, got = _run_move(src, src_row, ss, dst, dst_row, ds, width, n, mask, acc)
                assert rc == OK
                _same(got, want, f"width {width} {rows} mask={masked} acc={acc}")


def test_move_chunks_many_duplicates_and_past_the_grid_cap():
    gen = _gen(77)
    n, width = H.MOVE_DUPLICATES + 300, 8
    src = H.ints((50 * 12,), gen)
    src_row = torch.randint(0, 50, (n,), generator=gen)
    dst_row = torch.cat([torch.full((H.MOVE_DUPLICATES,), 2), torch.randint(0, 4, (300,), generator=gen)])
    mask = torch.rand(n, generator=gen) < 0.9
    dst = H.ints((5 * 12,), gen)
    want = H.move(src, src_row, 12, dst.clone(), dst_row, 12, width, n, mask, True)
    rc, got = _run_move(src, src_row, 12, dst, dst_row, 12, width, n, mask, True)
    assert rc == OK
    _same(got, want, "4096 lookups into one row")
    # n * width/4 float4s > kMaxGrid * 4 workgroups * kBlock threads: the grid-stride trip
    n, width = 70000, 128
    assert n * width // 4 > 2048 * 4 * 256
    src = H.ints((300 * 132,), gen)
    src_row = torch.randint(0, 300, (n,), generator=gen)
    dst_row = torch.randperm(n + 2, generator=gen)[:n]
    dst = H.nan((n + 2) * 132)
    want = H.move(src, src_row, 132, dst.clone(), dst_row, 132, width, n)
    rc, got = _run_move(src, src_row, 132, dst, dst_row, 132, width, n, None, False)
    assert rc == OK
    _same(got, want, "past the grid cap")


@pytest.mark.parametrize("what,kw", [("width % 4", dict(width=6)), ("src stride % 4", dict(ss=10)), ("dst stride % 4", dict(ds=10)),
                                     ("src 4 bytes off", dict(src_off=1)), ("dst 4 bytes off", dict(dst_off=1))])
def test_move_chunks_declines(what, kw):
    gen = _gen(len(what))
    a = dict(width=8, ss=12, ds=12, src_off=0, dst_off=0)
    a.update(kw)
    src, dst = H.ints((8 * 12 + 4,), gen), H.nan(8 * 12 + 4)
    rows = torch.arange(6)
    rc, got = _run_move(src, rows, a["ss"], dst, rows, a["ds"], a["width"], 6, None, False, a["src_off"], a["dst_off"])
    assert rc == UNSUPPORTED, what
    assert bool(got.isnan().all()), "a declined call wrote"


# ========================================================================================================== segment sum
@pytest.mark.parametrize("width", H.SEGSUM_WIDTHS)
def test_segment_sum_widths_lengths_and_untouched_cells(width):
    gen = _gen(width)
    ldx, ldo, nslices = width + 3, width + 2, 6
    lengths = H.SEGSUM_LENGTHS + [256, 5]
    slices = [0, 2, 2, 4, 0, 2, 2, 5]                      # several segments into slices 0 and 2; slices 1 and 3 never named
    first, segs = 2, []
    for ln, g in zip(lengths, slices):
        segs.append((first, ln, g))
        first += ln + 1                                    # a row between segments that belongs to nobody
    X = H.ints((first * ldx,), gen)
    for f, ln, _ in segs:
        X[(f + ln) * ldx:(f + ln + 1) * ldx] = NAN         # reading a row past a segment's end poisons the sum
    kseg = torch.tensor(segs, dtype=torch.int64)
    out = H.ints((nslices, ldo), gen)
    out[:, width:] = NAN
    out[[1, 3]] = NAN
    want = H.segment_sum(X, ldx, width, kseg, out.clone(), ldo)
    got, Xd, ksd = _f32(out), _f32(X), kseg.to(DEV)
    rc = _lib.load().mi_segment_sum(Xd.data_ptr(), ldx, width, ksd.data_ptr(), len(segs), got.data_ptr(), ldo, _stream())
    assert rc == OK
    _same(got, want, f"width {width}")


# ================================================================================================================ GEMMs
MTILE = [2, -1, 0, 3, -1, 1, 2]                            # 7 row tiles: a scrambled mix of 4 slices and unused tiles


def _row_groups_case(N, K, transB, lda_extra=4, sB_extra=8):
    gen = _gen(N, K, transB, lda_extra, sB_extra)
    M = 6 * 64 + 40                                        # the last tile is partial
    lda, ldc = K + lda_extra, N + 4
    ldb = (K if transB else N) + 4
    sB = (N if transB else K) * ldb + sB_extra
    A, B = H.ints((M * lda,), gen), H.ints((4 * sB,), gen)
    mt = torch.tensor(MTILE, dtype=torch.int32)
    want = H.gemm_row_groups(A, B, H.nan(M * ldc), M, N, K, lda, ldb, ldc, transB, sB, mt)
    C, Ad, Bd, mtd = _f32(H.nan(M * ldc)), _f32(A), _f32(B), mt.to(DEV)
    rc = _lib.load().mi_gemm_f32_row_groups(Ad.data_ptr(), Bd.data_ptr(), C.data_ptr(), M, N, K, lda, ldb, ldc, int(transB), sB,
                                            mtd.data_ptr(), _stream())
    assert rc == OK
    _same(C, want, f"row groups N={N} K={K} transB={transB} lda={lda} sB={sB}")
    rows = want.view(M, ldc)
    assert bool(rows[64:128].isnan().all()) and bool(rows[256:320].isnan().all())        # the -1 tiles keep the sentinel
    assert bool(rows[:, N:].isnan().all()) and not bool(rows[:64, :N].isnan().any())


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("N", H.ROW_GROUP_N)
def test_gemm_row_groups_exact(N, transB):
    for K in H.ROW_GROUP_K:
        _row_groups_case(N, K, transB)


@pytest.mark.parametrize("transB", [0, 1])
def test_gemm_row_groups_guarded_operands(transB):
    _row_groups_case(68, 36, transB, sB_extra=9)           # sB % 4 != 0: B slices off the 16-byte grid
    _row_groups_case(68, 36, transB, lda_extra=1)          # lda % 4 != 0


@pytest.mark.parametrize("M,N", H.K_GROUP_MN)
def test_gemm_k_groups_exact(M, N):
    gen = _gen(M, N)
    lda, ldb, ldc = M + 4, N + 4, N + 4
    sC, nslices = M * ldc + 8, 5
    lengths = H.K_GROUP_SEGS + [33, 31, 2048]
    slices = [0, 1, 1, 2, 1, 4, 4, 2, 4]                   # two segments into slice 2, three into 1 and 4; slice 3 unnamed
    first, segs = 1, []
    for ln, g in zip(lengths, slices):
        segs.append((first, ln, g))
        first += ln + 1
    A, B = H.ints((first * lda,), gen), H.ints((first * ldb,), gen)
    for f, ln, _ in segs:                                  # a row past a segment's end, if read, poisons the product
        A[(f + ln) * lda:(f + ln + 1) * lda] = NAN
        B[(f + ln) * ldb:(f + ln + 1) * ldb] = NAN
    kseg = torch.tensor(segs, dtype=torch.int64)
    C = H.nan(nslices * sC)
    for g in range(nslices):
        if g != 3:
            torch.as_strided(C, (M, N), (ldc, 1), g * sC).copy_(H.ints((M, N), gen))       # the entry accumulates
    want = H.gemm_k_groups(A, B, C.clone(), M, N, lda, ldb, ldc, sC, kseg)
    got, Ad, Bd, ksd = _f32(C), _f32(A), _f32(B), kseg.to(DEV)
    rc = _lib.load().mi_gemm_f32_k_groups(Ad.data_ptr(), Bd.data_ptr(), got.data_ptr(), M, N, lda, ldb, ldc, sC, ksd.data_ptr(),
                                          len(segs), _stream())
    assert rc == OK
    _same(got, want, f"k groups M={M} N={N}")


def test_gemm_k_groups_declines_too_many_segments():
    kseg = torch.zeros((65536, 3), dtype=torch.int64, device=DEV)
    A, B, C = _f32(torch.ones(64)), _f32(torch.ones(64)), _f32(H.nan(64))
    rc = _lib.load().mi_gemm_f32_k_groups(A.data_ptr(), B.data_ptr(), C.data_ptr(), 8, 8, 8, 8, 8, 64, kseg.data_ptr(), 65536, _stream())
    assert rc == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(C.isnan().all())


# ============================================================================================================ last level
class _Last:
    """Operands of one last-level call: chunks addressed through a scrambled, repeating src_row with a stride larger than H*K."""

    def __init__(self, Hh, K, q, n, with_valid, seed):
        gen = _gen(Hh, K, q, n, seed)
        self.H, self.K, self.q, self.n, self.p = Hh, K, q, n, 7
        self.nsrc, self.stride = 40, Hh * K + 8
        self.src = H.ints((self.nsrc * self.stride,), gen)
        self.src_row = torch.randint(0, self.nsrc, (n,), generator=gen)
        self.core = H.ints((self.p, K, q), gen)
        self.digit = torch.randint(0, self.p, (n,), generator=gen).to(torch.int32)
        self.valid = None
        self.g = H.ints((n, Hh * q), gen)
        if with_valid:
            self.valid = (torch.rand(n, generator=gen) < 0.7).to(torch.uint8)
            if n > 1:
                self.valid[0], self.valid[n - 1] = 0, 1
            self.g[~self.valid.bool()] = NAN               # an invalid lookup's gradient row is not read
        self.dev = [_f32(self.src), self.src_row.to(DEV), _f32(self.core), self.digit.to(DEV),
                    None if self.valid is None else self.valid.to(DEV)]

    def args(self):
        s, r, c, d, v = self.dev
        return s.data_ptr(), r.data_ptr(), self.stride, c.data_ptr(), d.data_ptr(), _p(v), self.H, self.K, self.q

    def fwd(self):
        out = _f32(H.nan(self.n * self.H * self.q))
        rc = _lib.load().mi_tt_last_fwd(*self.args(), out.data_ptr(), self.n, _stream())
        return rc, out

    def bwd(self, want_dst, want_core, segcnt):
        HK, n = self.H * self.K, self.n
        ds = HK + 4
        dst_row = torch.randperm(n + 3, generator=_gen(n, segcnt))[:n]
        dst0, gc0 = H.nan((n + 3) * ds), H.ints((self.p, self.K, self.q), _gen(segcnt, n))
        pl = H.Plan(self.digit, self.p, 1, segcnt)
        order = torch.zeros(pl.mpad, dtype=torch.int64)
        order[pl.pos] = torch.arange(n)
        dst, gc, g = _f32(dst0), _f32(gc0), _f32(self.g)
        dr, od, ks = dst_row.to(DEV), order.to(DEV), pl.kseg.to(DEV)
        rc = _lib.load().mi_tt_last_bwd(*self.args(), g.data_ptr(), dst.data_ptr() if want_dst else None, dr.data_ptr(), ds,
                                        od.data_ptr(), ks.data_ptr(), pl.nseg, gc.data_ptr() if want_core else None, n, _stream())
        ref_dst, ref_gc = dst0, gc0
        if want_dst:
            ref_dst = H.move(H.last_bwd_in(self.core, self.digit, self.valid, self.H, self.K, self.q, self.g), None, HK, dst0.clone(),
                             dst_row, ds, HK, n)
        if want_core:
            ref_gc = gc0 + H.last_bwd_core(self.src, self.src_row, self.stride, (self.p, self.K, self.q), self.digit, self.valid,
                                           self.H, self.K, self.q, self.g)
        return rc, dst, gc, ref_dst, ref_gc, pl


@pytest.mark.parametrize("Hh,K,q", H.LAST_SHAPES)
def test_last_level_forward_exact(Hh, K, q):
    for n in H.LAST_N + [H.LAST_N_BIG]:
        for with_valid in ((True,) if n == H.LAST_N_BIG else (False, True)):
            case = _Last(Hh, K, q, n, with_valid, 1)
            want = H.last_fwd(case.src, case.src_row, case.stride, case.core, case.digit, case.valid, Hh, K, q)
            rc, out = case.fwd()
            assert rc == OK
            _same(out, want, f"last fwd {Hh, K, q} n={n} valid={with_valid}")
            if with_valid:
                assert not bool(out.view(n, -1)[~case.valid.bool().to(DEV)].any())          # rows of invalid lookups are zero


@pytest.mark.parametrize("Hh,K,q", H.LAST_SHAPES)
def test_last_level_backward_exact(Hh, K, q):
    """dst only, gcore only and both; segments of 1, 2, 16 and 17 lookups per wave; at n = 8192 + 67 with one-lookup segments the
    slice-gradient kernel walks more than 8192 segments.  With valid, the gradient rows of invalid lookups are NaN: their dst
    rows are zero and the slice gradients are finite and equal to the restatement without those lookups."""
    runs = [(n, segcnt, True, True) for n in H.LAST_N for segcnt in H.LAST_SEG_COUNTS]
    runs += [(5, 2, True, False), (5, 2, False, True), (300, 16, True, True), (300, 17, False, True),
             (H.LAST_N_BIG, 1, True, True)]
    for n, segcnt, want_dst, want_core in runs:
        for with_valid in ((True,) if n == H.LAST_N_BIG else (False, True)):
            case = _Last(Hh, K, q, n, with_valid, segcnt)
            rc, dst, gc, ref_dst, ref_gc, pl = case.bwd(want_dst, want_core, segcnt)
            what = f"last bwd {Hh, K, q} n={n} seg={segcnt} valid={with_valid} dst={want_dst} core={want_core}"
            assert rc == OK, what
            if n == H.LAST_N_BIG and segcnt == 1:
                assert pl.live > 8192
            _same(dst, ref_dst, what + " dst")
            _same(gc, ref_gc, what + " gcore")
            assert bool(gc.isfinite().all()), what


@pytest.mark.parametrize("what,Hh,K,q,fwd_only", [("H*q = 12", 3, 4, 4, False), ("K % 4", 1, 6, 4, True), ("H*K = 516", 4, 129, 1, False),
                                                  ("K*q = 516", 1, 129, 4, False)])
def test_last_level_declines(what, Hh, K, q, fwd_only):
    case = _Last(Hh, K, q, 5, True, 0)
    rc, out = case.fwd()
    assert rc == UNSUPPORTED, what
    assert bool(out.isnan().all()), "a declined call wrote"
    if not fwd_only:
        rc, dst, gc, ref_dst, ref_gc, _ = case.bwd(True, True, 2)
        assert rc == UNSUPPORTED, what
        assert bool(dst.isnan().all())
        prefill = H.ints((case.p, K, q), _gen(2, 5))
        _same(gc, prefill, what + ": gcore of a declined call")


# ============================================================================================================ end to end
_oracle_cache = {}


def _oracle(name, n, bad=None):
    """float64 oracle (output, core gradients) of a table row; `bad` positions are lookups that contribute nothing."""
    key = (name, n, None if bad is None else tuple(bad.tolist()))
    if key not in _oracle_cache:
        _, _, ps, qs, _ = H.e2e_case(name)
        cores, idx, G, ranks = H.e2e_inputs(name, n)
        idx, G = idx.clone(), G.double().clone()
        if bad is not None:
            idx[bad], G[bad] = 0, 0.0
        cs = [c.double().requires_grad_(True) for c in cores]
        ref = ro.tt_forward(idx, ps, qs, ranks, cs)
        (ref * G).sum().backward()
        ref = ref.detach()
        if bad is not None:
            ref[bad] = 0.0
        _oracle_cache[key] = (ref, [c.grad for c in cs])
    return _oracle_cache[key]


def _emb(name, n):
    _, _, ps, qs, mid = H.e2e_case(name)
    cores, idx, G, ranks = H.e2e_inputs(name, n)
    emb = TTRecTorch(H.E2E_N, H.prod(qs), list(mid), tt_p_shapes=ps, tt_q_shapes=qs, weight_dist="normal")
    with torch.no_grad():
        for c, v in zip(emb.tt_cores, cores):
            c.copy_(v)
    return emb.to(DEV), idx, G


def _assert_branch(kt, name):
    _, fast, ps, _, _ = H.e2e_case(name)
    s = kt.summary()
    count = lambda k: s.get(k, {}).get("count", 0)      # noqa: E731
    levels = len(ps) - 2 if fast else len(ps) - 1
    for k in ("tt_last_fwd", "tt_last_bwd_in", "tt_last_bwd_core"):
        assert count(k) == (1 if fast else 0), f"{name}: {k} ran {count(k)} times"
    # one product per GEMM level forward, one input-gradient product and one slice-gradient product per level backward
    assert count("gemm_row_groups") == 2 * levels and count("gemm_k_groups") == levels, (name, s.keys())
    assert count("tt_digits") == 1 and count("segment_sum") == 1


def _run_and_check(name, n, bad=None, bad_ids=None):
    emb, idx, G = _emb(name, n)
    if bad is not None:
        idx, G = idx.clone(), G.clone()
        idx[bad] = bad_ids
        G[bad] = NAN
    ref, gref = _oracle(name, n, bad)
    assert n >= _kernels._TT_GROUPED_MIN and _kernels.tt_grouped_supported(n, emb.tt_q_shapes, emb.tt_ranks)
    with KernelTimer() as kt:
        out = emb(idx.to(DEV)).reshape(n, -1)
        (out * G.to(DEV)).sum().backward()
    _assert_branch(kt, name)
    grads = [c.grad for c in emb.tt_cores]
    fr = [H.tol_fraction(out, ref, *H.E2E_TOL["fwd"])]
    fr += [H.tol_fraction(a.view(b.shape), b, *H.E2E_TOL["grad"]) for a, b in zip(grads, gref)]
    print(f"{name} n={n}: fraction of the tolerance used: forward {fr[0]:.4f}, core gradients {[round(f, 4) for f in fr[1:]]}")
    torch.testing.assert_close(out.cpu().double(), ref, rtol=H.E2E_TOL["fwd"][0], atol=H.E2E_TOL["fwd"][1],
                               msg=lambda m: f"{name} forward: {m}")
    for i, (a, b) in enumerate(zip(grads, gref)):
        assert bool(a.isfinite().all()), f"{name}: core {i} gradient is not finite"
        torch.testing.assert_close(a.cpu().double().view(b.shape), b, rtol=H.E2E_TOL["grad"][0], atol=H.E2E_TOL["grad"][1],
                                   msg=lambda m: f"{name} grad core {i}: {m}")
    return emb, idx, G, out, ref, gref


@pytest.mark.parametrize("name", [c[0] for c in H.E2E_CASES])
def test_every_branch_of_the_grouped_lookup_matches_the_oracle(name):
    _run_and_check(name, H.E2E_n)
    _lib.check_index_errors()


@pytest.mark.parametrize("name", H.E2E_BIG)
def test_branches_past_one_launch_of_waves(name):
    """n = 8192 + 70 lookups: the one-wave-per-lookup loops of the last level take their second trip with a backward behind them."""
    _run_and_check(name, H.E2E_n_BIG)
    _lib.check_index_errors()


@pytest.mark.parametrize("name", H.E2E_BAD_IDS)
def test_out_of_range_ids_with_a_nan_upstream_gradient(name):
    """Three out-of-range ids whose upstream gradient rows are NaN: zero output rows, finite core gradients that match the oracle
    on the kept ids, the error word raised — on the grouped form and on the per-lookup kernels alike."""
    n = H.E2E_n
    bad = torch.tensor([7, 2000, n - 1])
    bad_ids = torch.tensor([H.E2E_N, -3, 1 << 40])
    emb, idx, G, out, ref, gref = _run_and_check(name, n, bad, bad_ids)
    assert not bool(out[bad.to(DEV)].any())
    with pytest.raises(IndexError):
        _lib.check_index_errors()
    cores = [c.detach().clone().requires_grad_(True) for c in emb.tt_cores]
    per = _kernels.TTLookup.apply(idx.to(DEV), H.E2E_N, tuple(emb.tt_p_shapes), tuple(emb.tt_q_shapes), tuple(emb.tt_ranks), *cores)
    (per * G.to(DEV)).sum().backward()
    assert not bool(per[bad.to(DEV)].any())
    torch.testing.assert_close(per.cpu().double(), ref, rtol=H.E2E_TOL["fwd"][0], atol=H.E2E_TOL["fwd"][1])
    for i, (c, b) in enumerate(zip(cores, gref)):
        assert bool(c.grad.isfinite().all()), f"per-lookup: core {i} gradient is not finite"
        torch.testing.assert_close(c.grad.cpu().double().view(b.shape), b, rtol=H.E2E_TOL["grad"][0], atol=H.E2E_TOL["grad"][1])
        torch.testing.assert_close(emb.tt_cores[i].grad, c.grad, rtol=H.E2E_TOL["grad"][0], atol=H.E2E_TOL["grad"][1])
    with pytest.raises(IndexError):
        _lib.check_index_errors()

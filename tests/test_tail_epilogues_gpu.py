"""GPU: the epilogues of the fused tail's kernels (csrc/tail.hip) through the C ABI, with caller-given constants (no
statistics join): the head + criterion launch and the three products whose epilogues store under predicates — partial row
tiles (rows_valid < 64), partial column tiles (cols_valid < ncols), a second wave with one row, a lane whose second column
chunk is the only valid one, the second trip of the head's row loop.

Reference: a float64 restatement in torch.  Every pre-activation of the inputs is at least 1e-3 away from 0 (asserted on
the CPU), so no ReLU decision can differ between float32 and float64 and NO element may miss its bound (max_bad_frac = 0).

Bounds: conftest.assert_within_terms with k = 8, the factor tests/test_tail_gpu.py holds the same quantities to.  The
"terms" of a quantity are the absolute values of what is added to form it, with the terms of an input that was itself
computed in float32 carried through (a Lipschitz factor where it passes a function):
  a = relu((z - mu) sc + be) * keep        terms_a  = (|z - mu| |sc| + |be|) keep [pre > 0]
  z = a W^T, logit = a w + b + add         terms    = terms_a |W|^T (+ |b| + |add|)
  g = (sigmoid(logit) - y) / M             terms_g  = (sigmoid + y + terms_logit / 4) / M          (|sigmoid'| <= 1/4)
  DY = g w keep [pre > 0]                  terms_DY = terms_g |w| keep [pre > 0];   column sums: the sums of these
  loss = mean(max(x,0) - x y + log1p(exp(-|x|)))   terms = mean(max(x,0) + |x| y + log1p(..) + terms_logit)   (|d/dx| <= 1)
  dz = al dy + bz (z - mu) + de            terms_dz = |al dy| + |bz (z - mu)| + |de|;  da = dz W: terms_dz |W|
Column statistics and column sums that a kernel forms from values it also stores (Z, OUT) are checked against the float64
sums of THOSE stored values, so that their bound is the reduction's alone:
  tile mean: every intermediate (a group's first row, s1 / n, a Chan delta) is at most 2 max|z|      terms = 2 max|z|
  tile M2:   a 16-row group forms sum d^2 and (sum d)^2 / n <= sum d^2 around its first row, the four groups meet in
             non-negative Chan terms that add up to M2                    terms = 2 sum_groups sum (z - first)^2 + M2
  shifted sums (t1, t2) in float64 from the tile's (n, mean, M2), d = mean - shift:
             terms_t1 = sum_tiles n terms_mean,  terms_t2 = sum_tiles (2 n |d| terms_mean + 8 eps n terms_mean^2 + terms_M2)
Outputs are allocated NaN-poisoned (tests/poison_helpers.py) with guard rows / pad columns: every owned element must come
back finite, everything else must still be NaN."""
import ctypes
import functools

import pytest
import torch

from conftest import EPS32, assert_within_terms
from poison_helpers import poisoned
from tail_helpers import tail_keep_scale

DEV = "cuda"
K_TERMS = 8          # tests/test_tail_gpu.py: failures(k=8.0)
MIN_PRE = 1e-3
HEAD_SHAPES = [(1, 4), (5, 260), (67, 400), (4100, 512)]
PRODUCT_M = [1, 65, 130]
# (reduction, output width) of the products: every output width of 36 (one partial column tile), 400 (4 x 100) and 416 (4 x 104)
FWD_KN = [(416, 36), (36, 400), (400, 416)]          # Z[M, N] = a(X[M, K]) W[N, K]^T
DGRAD_NK = [(400, 36), (36, 400), (400, 416)]        # OUT[M, K] = dz[M, N] W[N, K]
FM_D = {36: 4, 400: 16, 416: 16}
SEED_WORD = 777001
SALT1 = 0x51ED270B


def _gen(kind, *dims):
    seed = {"head": 1, "fwd": 2, "mid": 3, "fm": 4}[kind]
    for v in dims:
        seed = seed * 4099 + int(v)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _act_inputs(M, N, gen):
    """Z[M, N], mu, sc, be (float32) whose float64 pre-activation (Z - mu) sc + be is >= 0.01 in magnitude by construction
    (float32 rounding of Z moves it by ~1e-7)."""
    mu, sc, be = torch.randn(N, generator=gen) * 0.3, 0.5 + torch.rand(N, generator=gen), torch.randn(N, generator=gen) * 0.3
    sign = torch.where(torch.rand(M, N, generator=gen) < 0.5, -1.0, 1.0)
    tgt = sign * (0.01 + torch.randn(M, N, generator=gen).abs() * 0.7)
    Z = (mu.double() + (tgt.double() - be.double()) / sc.double()).float()
    return Z, mu, sc, be


def _pre64(Z, mu, sc, be):
    zc = Z.double() - mu.double()
    return zc, zc * sc.double() + be.double()


def _pad8(n):
    return (n + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def _head_case(M, N, p):
    gen = _gen("head", M, N)
    ld = _pad8(N)
    Z, mu, sc, be = _act_inputs(M, N, gen)
    w = torch.randn(N, generator=gen) / N ** 0.5
    b, add = torch.randn(1, generator=gen), torch.randn(M, generator=gen)
    y = (torch.rand(M, generator=gen) < 0.3).float()
    ks = tail_keep_scale(SEED_WORD, SALT1, M, ld, p)[:, :N].double()
    zc, pre = _pre64(Z, mu, sc, be)
    on = (pre > 0).double()
    a = pre.clamp_min(0) * ks
    ta = (zc.abs() * sc.double().abs() + be.double().abs()) * on * ks
    wd = w.double()
    xl = a @ wd + b.double() + add.double()
    t_xl = ta @ wd.abs() + b.double().abs() + add.double().abs()
    sig = torch.sigmoid(xl)
    g = (sig - y.double()) / M
    t_g = (sig + y.double() + t_xl / 4) / M
    DY = g[:, None] * wd * ks * on
    t_DY = t_g[:, None] * wd.abs() * ks * on
    lterm = xl.clamp_min(0) - xl * y.double() + torch.log1p(torch.exp(-xl.abs()))
    t_l = xl.clamp_min(0) + xl.abs() * y.double() + torch.log1p(torch.exp(-xl.abs())) + t_xl
    ref = dict(out=xl, g=g, DY=DY, s_dy=DY.sum(0), s_dyz=(DY * zc).sum(0), s_ga=(g[:, None] * a).sum(0), s_g=g.sum().view(1),
               loss=lterm.mean().view(1))
    terms = dict(out=t_xl, g=t_g, DY=t_DY, s_dy=t_DY.sum(0), s_dyz=(t_DY * zc.abs()).sum(0), s_ga=(t_g[:, None] * ta).sum(0),
                 s_g=t_g.sum().view(1), loss=t_l.mean().view(1))
    return dict(Z=Z, mu=mu, sc=sc, be=be, w=w, b=b, add=add, y=y, ld=ld, pre=pre, ref=ref, terms=terms)


def _products_common(M, N, K, gen):
    """dz's operands of a layer of width N and the weight W[N, K]."""
    DY, Zl = torch.randn(M, N, generator=gen), torch.randn(M, N, generator=gen)
    mu, al = torch.randn(N, generator=gen) * 0.3, 0.5 + torch.rand(N, generator=gen)
    bz, de = torch.randn(N, generator=gen) * 0.05, torch.randn(N, generator=gen) * 0.05
    W = torch.randn(N, K, generator=gen) / N ** 0.5
    zc = Zl.double() - mu.double()
    dz = al.double() * DY.double() + bz.double() * zc + de.double()
    t_dz = (al.double() * DY.double()).abs() + (bz.double() * zc).abs() + de.double().abs()
    return dict(DY=DY, Zl=Zl, mu=mu, al=al, bz=bz, de=de, W=W, dz=dz, t_dz=t_dz, da=dz @ W.double(), t_da=t_dz @ W.double().abs())


@functools.lru_cache(maxsize=None)
def _fwd_case(M, K, N):
    gen = _gen("fwd", M, K, N)
    X, mu, sc, be = _act_inputs(M, K, gen)
    W = torch.randn(N, K, generator=gen) / K ** 0.5
    rm, off = torch.randn(N, generator=gen) * 0.2, torch.randn(N, generator=gen) * 0.2
    zc, pre = _pre64(X, mu, sc, be)
    a = pre.clamp_min(0)
    ta = (zc.abs() * sc.double().abs() + be.double().abs()) * (pre > 0)
    return dict(X=X, mu=mu, sc=sc, be=be, W=W, rm=rm, off=off, pre=pre, a=a, t_a=ta, Z=a @ W.double().t(), t_Z=ta @ W.double().abs().t())


@functools.lru_cache(maxsize=None)
def _mid_case(M, N, K):
    gen = _gen("mid", M, N, K)
    c = _products_common(M, N, K, gen)
    pZ, p_mu, p_sc, p_be = _act_inputs(M, K, gen)
    pzc, pre = _pre64(pZ, p_mu, p_sc, p_be)
    on = (pre > 0).double()
    c.update(pZ=pZ, p_mu=p_mu, p_sc=p_sc, p_be=p_be, pre=pre, pzc=pzc, OUT=c["da"] * on, t_OUT=c["t_da"] * on)
    return c


@functools.lru_cache(maxsize=None)
def _fm_case(M, N, K):
    gen = _gen("fm", M, N, K)
    c = _products_common(M, N, K, gen)
    D = FM_D[K]
    emb, gy = torch.randn(M, K, generator=gen), torch.randn(M, generator=gen)
    S = emb.view(M, K // D, D).sum(1)
    Sd = S.double().repeat(1, K // D)
    c.update(emb=emb, gy=gy, S=S, D=D, gv=c["da"] + gy.double()[:, None] * (Sd - emb.double()),
             t_gv=c["t_da"] + gy.double().abs()[:, None] * (Sd.abs() + emb.double().abs()))
    return c


def test_inputs_keep_every_preactivation_off_the_kink():
    """The zero-exception cap rests on this: |float64 pre-activation| >= 1e-3 everywhere, four orders above what float32
    rounding of (z - mu) sc + be can move it, in every case the GPU tests run."""
    pres = [_head_case(M, N, 0.0)["pre"] for M, N in HEAD_SHAPES]
    pres += [_fwd_case(M, K, N)["pre"] for M in PRODUCT_M for K, N in FWD_KN]
    pres += [_mid_case(M, N, K)["pre"] for M in PRODUCT_M for N, K in DGRAD_NK]
    for pre in pres:
        assert float(pre.abs().min()) >= MIN_PRE
        assert 4 * EPS32 * float(pre.abs().max() + 4.0) < MIN_PRE / 100          # (|z - mu| |sc| + |be| <= |pre| + 2 |be| here)


# ------------------------------------------------------------------------------------------------------------- device side
def _lib():
    from recsys_benchmark_amd import _lib as L

    return L, L.load(), L.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def _guarded(rows, cols, guard=2):
    """A NaN-poisoned [rows + guard, cols] buffer (allocated with torch.empty under poison_helpers.poisoned)."""
    with poisoned():
        t = torch.empty((rows + guard, cols), dtype=torch.float32, device=DEV)
    assert bool(torch.isnan(t).all())
    return t


def _owned(buf, rows, cols, what):
    """The owned block [rows, cols] of a guarded buffer, after asserting it is finite and everything else still NaN."""
    own = buf[:rows, :cols]
    assert bool(torch.isfinite(own).all()), f"{what}: an owned element was not written"
    assert bool(torch.isnan(buf[rows:]).all()) and bool(torch.isnan(buf[:rows, cols:]).all()), f"{what}: a store outside the owned block"
    return own


def _keep_bits(M, ld, p):
    if p <= 0:
        return None
    L, lib, s = _lib()
    seed = torch.full((1,), SEED_WORD, dtype=torch.int64, device=DEV)
    bits = torch.zeros(M * ld // 8, dtype=torch.uint8, device=DEV)
    salts, ps, lds = (ctypes.c_int64 * 1)(SALT1), (ctypes.c_float * 1)(p), (ctypes.c_int32 * 1)(ld)
    ptrs = (ctypes.c_void_p * 1)(bits.data_ptr())
    L.check(lib.mi_tail_dropout_masks_z(seed.data_ptr(), 1, ctypes.addressof(salts), ctypes.addressof(ps), ctypes.addressof(lds),
                                        ctypes.addressof(ptrs), M, None, 0, s), "mi_tail_dropout_masks_z")
    return bits


def _check(got, ref, terms, what):
    assert_within_terms(got, ref, terms, K_TERMS, what, max_bad_frac=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M,N", HEAD_SHAPES)
def test_head_bce_launch_against_float64(M, N, p):
    c = _head_case(M, N, p)
    L, lib, s = _lib()
    ld, R = c["ld"], 3
    Zd = torch.zeros(M, ld, device=DEV)
    Zd[:, :N] = c["Z"].to(DEV)
    d = {k: c[k].to(DEV) for k in ("mu", "sc", "be", "w", "b", "add", "y")}
    bits = _keep_bits(M, ld, p)
    out, g, DY = _guarded(1, M, guard=1), _guarded(1, M, guard=1), _guarded(M, ld)
    part, wpart = torch.zeros(R, N, 2, device=DEV), torch.zeros(R, N + 4, device=DEV)
    ws = torch.zeros(int(lib.mi_tail_head_bce_ws_elems(R)), device=DEV)
    L.check(lib.mi_tail_head_bce(Zd.data_ptr(), ld, d["mu"].data_ptr(), d["sc"].data_ptr(), d["be"].data_ptr(), float(p), L.ptr(bits),
                                 d["w"].data_ptr(), d["b"].data_ptr(), d["add"].data_ptr(), d["y"].data_ptr(), out.data_ptr(),
                                 g.data_ptr(), DY.data_ptr(), part.data_ptr(), wpart.data_ptr(), R, ws.data_ptr(), M, N, None, None, s),
            "mi_tail_head_bce")
    torch.cuda.synchronize()
    ref, t = c["ref"], c["terms"]
    tag = f"head M={M} N={N} p={p}"
    _check(_owned(out, 1, M, "logits").view(-1), ref["out"], t["out"], f"{tag}: logits")
    _check(_owned(g, 1, M, "g").view(-1), ref["g"], t["g"], f"{tag}: g")
    _check(_owned(DY, M, N, "DY"), ref["DY"], t["DY"], f"{tag}: DY")
    psum, wsum = part.double().sum(0).cpu(), wpart.double().sum(0).cpu()
    _check(psum[:, 0], ref["s_dy"], t["s_dy"], f"{tag}: sum dy")
    _check(psum[:, 1], ref["s_dyz"], t["s_dyz"], f"{tag}: sum dy (z - mu)")
    _check(wsum[:N], ref["s_ga"], t["s_ga"], f"{tag}: head dw pieces")
    _check(wsum[N:N + 1], ref["s_g"], t["s_g"], f"{tag}: sum g")
    _check(ws[:1], ref["loss"], t["loss"], f"{tag}: loss")


def _tile_stats(Zk, M):
    """float64 (mean, M2) per 64-row tile of the stored Z, and the bounds' terms (module docstring)."""
    Zk = Zk.double().cpu()
    mean, m2, t_mean, t_m2, cnt = [], [], [], [], []
    for r0 in range(0, M, 64):
        z = Zk[r0:min(M, r0 + 64)]
        mu = z.mean(0)
        M2 = ((z - mu) ** 2).sum(0)
        grp = sum(((z[q:q + 16] - z[q]) ** 2).sum(0) for q in range(0, z.shape[0], 16))
        mean.append(mu); m2.append(M2); t_mean.append(2 * z.abs().max(0).values); t_m2.append(2 * grp + M2); cnt.append(z.shape[0])
    return torch.stack(mean), torch.stack(m2), torch.stack(t_mean), torch.stack(t_m2), torch.tensor(cnt, dtype=torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("sums", [False, True], ids=["tile-statistics", "shifted-sums"])
@pytest.mark.parametrize("K,N", FWD_KN)
@pytest.mark.parametrize("M", PRODUCT_M)
def test_forward_product_with_statistics_against_float64(M, K, N, sums):
    c = _fwd_case(M, K, N)
    L, lib, s = _lib()
    d = {k: c[k].to(DEV) for k in ("X", "mu", "sc", "be", "W", "rm", "off")}
    Z, a_out = _guarded(M, N), _guarded(M, K)
    R = 2
    if sums:
        part, shift = torch.zeros(R * 4 * N, device=DEV), _guarded(1, N, guard=1)
        rc = lib.mi_tail_fwd_gemm_s(d["X"].data_ptr(), K, d["mu"].data_ptr(), d["sc"].data_ptr(), d["be"].data_ptr(), 0.0, None,
                                    d["W"].data_ptr(), K, Z.data_ptr(), N, part.data_ptr(), a_out.data_ptr(), M, N, K, None, R,
                                    shift.data_ptr(), d["rm"].data_ptr(), d["off"].data_ptr(), s)
    else:
        with poisoned():
            part = torch.empty(int(lib.mi_tail_part_elems(M, N)), dtype=torch.float32, device=DEV)
        rc = lib.mi_tail_fwd_gemm(d["X"].data_ptr(), K, d["mu"].data_ptr(), d["sc"].data_ptr(), d["be"].data_ptr(), 0.0, None,
                                  d["W"].data_ptr(), K, Z.data_ptr(), N, part.data_ptr(), a_out.data_ptr(), M, N, K, s)
    L.check(rc, "mi_tail_fwd_gemm")
    torch.cuda.synchronize()
    tag = f"fwd M={M} K={K} N={N}"
    Zk = _owned(Z, M, N, "Z")
    _check(Zk, c["Z"], c["t_Z"], f"{tag}: Z")
    _check(_owned(a_out, M, K, "a_out"), c["a"], c["t_a"], f"{tag}: a_out")
    mean, m2, t_mean, t_m2, cnt = _tile_stats(Zk, M)
    if not sums:
        got = part.view(-1, N, 2)
        assert bool(torch.isfinite(got).all()), "a tile statistic was not written"
        _check(got[:, :, 0], mean, t_mean, f"{tag}: tile means")
        _check(got[:, :, 1], m2, t_m2, f"{tag}: tile M2")
        return
    sh = (c["rm"] - c["off"]).double()          # (the float32 difference: what the kernel stores and shifts by)
    assert torch.equal(_owned(shift, 1, N, "shift").view(-1).cpu(), c["rm"] - c["off"])
    got = part.view(torch.float64).view(R, 2, N).sum(0).cpu()
    dd, n = mean - sh, cnt[:, None]
    # (the kernel's float64 products and adds contribute ~1e-16 relative: nothing next to the float32 tile statistics)
    _check(got[0], (n * dd).sum(0), (n * t_mean).sum(0), f"{tag}: shifted sum t1")
    _check(got[1], (n * dd * dd + m2).sum(0), (2 * n * dd.abs() * t_mean + K_TERMS * EPS32 * n * t_mean ** 2 + t_m2).sum(0), f"{tag}: shifted sum t2")


def _dz_args(d, N):
    return (d["DY"].data_ptr(), d["Zl"].data_ptr(), N, d["mu"].data_ptr(), d["al"].data_ptr(), d["bz"].data_ptr(), d["de"].data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("reps", [0, 2], ids=["tile-sums", "atomic-sums"])
@pytest.mark.parametrize("N,K", DGRAD_NK)
@pytest.mark.parametrize("M", PRODUCT_M)
def test_middle_input_gradient_product_against_float64(M, N, K, reps):
    c = _mid_case(M, N, K)
    L, lib, s = _lib()
    d = {k: c[k].to(DEV) for k in ("DY", "Zl", "mu", "al", "bz", "de", "W", "pZ", "p_mu", "p_sc", "p_be")}
    OUT, dz_out = _guarded(M, K), _guarded(M, N)
    if reps:
        part = torch.zeros(reps, K, 2, device=DEV)
    else:
        with poisoned():
            part = torch.empty(int(lib.mi_tail_part_elems(M, K)), dtype=torch.float32, device=DEV).view(-1, K, 2)
    L.check(lib.mi_tail_dgrad_gemm_s(*_dz_args(d, N), d["W"].data_ptr(), K, d["pZ"].data_ptr(), K, d["p_mu"].data_ptr(),
                                     d["p_sc"].data_ptr(), d["p_be"].data_ptr(), 0.0, None, OUT.data_ptr(), K, part.data_ptr(), reps,
                                     dz_out.data_ptr(), M, N, K, None, s), "mi_tail_dgrad_gemm_s")
    torch.cuda.synchronize()
    tag = f"dgrad M={M} N={N} K={K} reps={reps}"
    Ok = _owned(OUT, M, K, "OUT")
    _check(Ok, c["OUT"], c["t_OUT"], f"{tag}: OUT")
    _check(_owned(dz_out, M, N, "dz_out"), c["dz"], c["t_dz"], f"{tag}: dz_out")
    assert bool(torch.isfinite(part).all()), "a column sum was not written"
    O64 = Ok.double().cpu()
    got = part.double().sum(0).cpu()          # (tile rows or replica rows: their float64 sum is the batch's column sum)
    _check(got[:, 0], O64.sum(0), O64.abs().sum(0), f"{tag}: sum dy")
    _check(got[:, 1], (O64 * c["pzc"]).sum(0), (O64 * c["pzc"]).abs().sum(0), f"{tag}: sum dy (z - mu)")


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", DGRAD_NK)
@pytest.mark.parametrize("M", PRODUCT_M)
def test_fm_input_gradient_product_against_float64(M, N, K):
    c = _fm_case(M, N, K)
    L, lib, s = _lib()
    d = {k: c[k].to(DEV) for k in ("DY", "Zl", "mu", "al", "bz", "de", "W", "emb", "S", "gy")}
    D, F = c["D"], K // c["D"]
    gv, g1, dz_out = _guarded(M, K), _guarded(M, F), _guarded(M, N)
    L.check(lib.mi_tail_dgrad_gemm_fm(*_dz_args(d, N), d["W"].data_ptr(), K, gv.data_ptr(), dz_out.data_ptr(), M, N, K, None,
                                      d["emb"].data_ptr(), d["S"].data_ptr(), d["gy"].data_ptr(), g1.data_ptr(), D, s),
            "mi_tail_dgrad_gemm_fm")
    torch.cuda.synchronize()
    tag = f"dgrad_fm M={M} N={N} K={K}"
    _check(_owned(gv, M, K, "gvals"), c["gv"], c["t_gv"], f"{tag}: gvals")
    _check(_owned(dz_out, M, N, "dz_out"), c["dz"], c["t_dz"], f"{tag}: dz_out")
    assert torch.equal(_owned(g1, M, F, "g1vals").cpu(), c["gy"][:, None].expand(M, F)), f"{tag}: g1vals"


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sums", "joins", "finalize"])
def test_fused_tail_at_70_rows_brackets_the_oracle(form, monkeypatch):
    """The whole fused tail, forward and backward, at M = 70 (a 6-row second tile) and the headline widths 416-400-400-400,
    with tests/test_tail_gpu.py's bracket against the float64 oracle, in the three forms of the statistics."""
    import test_tail_gpu as tt
    from recsys_benchmark_amd import mlp as _mlp
    from recsys_benchmark_amd import tail as _tail_mod

    monkeypatch.setattr(_mlp, "FUSED_TAIL", True)
    monkeypatch.setattr(_tail_mod, "STAT_SUMS", form == "sums")
    monkeypatch.setattr(_tail_mod, "MERGE_JOINS", form == "joins")
    tt.test_fused_tail_brackets_float64_like_the_stock_modules(70, 416, [400, 400, 400], 0.5, "bn-train", monkeypatch)

"""GPU: DeepFM's fused lookup over the quantised tables (mi_gather_fm_quant_fwd, mi_gather_fm_qat_*): the ops against the
separate lookups (bit for bit) and the float64 restatement of tests/quant_deepfm_helpers.py, the launch names, deterministic
mode, the models against the reference's goldens, the row-form training step — and all of it once more with every
uninitialised allocation filled with NaN."""
import contextlib
import copy

import pytest
import torch

from conftest import assert_close, assert_within_terms, load_golden

import quant_deepfm_helpers as qh
import recsys_benchmark_amd as pkg
from oracle import reference_ops as ro
from poison_helpers import poisoned
from recsys_benchmark_amd import _kernels, _lib, quant_fm, trainer
from recsys_benchmark_amd.embeddings.ptq_emb import PTQEmb_Fp16, PTQEmb_Int, affine_codes
from recsys_benchmark_amd.embeddings.qat_emb import QAT_EmbInt, _QatLookup
from recsys_benchmark_amd.mlp import run_tail
from recsys_benchmark_amd.optim import SparseAdam, get_optimizers
from recsys_benchmark_amd.profiling import KernelTimer

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (F, D) -> the form it reaches (csrc/gather_fm_quant.hip: LPR = D / 4 lanes per row, RS = 64 / LPR rows per step,
# NIT = ceil(F / RS) unrolled steps up to 4 when F <= 64): the grid of tests/test_dual_deepfm_gpu.py
SHAPES = [(3, 4),       # LPR 1, NIT 1
          (26, 16),     # NIT 2
          (39, 16),     # NIT 3
          (70, 8),      # F > 64: the generic word-load loop
          (26, 64),     # NIT 0 by width: the generic word-load loop
          (5, 12)]      # the scalar any-D kernels
BATCHES = [1, 37, 1030]
QKINDS = ["fp16", "int8", "int16", "int4"]       # int4: n_bits = 4 codes in an int8 table
SCALES = {8: 0.00097, 16: 3.9e-6}                # regular weights |w| <= 0.1 round (0.1 / scale = 103 and 25641), +-0.5 clamps
POISON = [False, True]
_cases = {}


def _maybe_poisoned(on):
    return poisoned() if on else contextlib.nullcontext()


def _case(F, D, B):
    """Seeded operands of one case, made once and shared (read-only) by the tests that use it.  Fields of 2 and 3 values
    from F = 9 on: hot rows at B = 1030."""
    key = (F, D, B)
    if key not in _cases:
        gen = torch.Generator().manual_seed(5000 * F + 10 * D + B)
        dims = [2 + (7 * f) % 11 for f in range(F)]
        N = sum(dims)
        x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1)
        c = dict(dims=dims, N=N, x=x, offsets=ro.field_offsets(dims).view(-1), w1=torch.randn(N, 1, generator=gen),
                 bias=torch.randn(1, generator=gen), G=torch.randn(B, F, D, generator=gen), gy=torch.randn(B, generator=gen),
                 prob=torch.rand(B, F, D, generator=gen))
        c["rows"] = (x + c["offsets"].view(1, -1)).reshape(-1)
        W = (torch.rand(N, D, generator=gen) - 0.5) * 0.19
        # min / (max - min) inside (-0.5000153, -0.5): the PTQ zero points are 0 and no code leaves its storage type at 8 or
        # at 16 bits (gen_golden_quant_deepfm.py; _codes asserts it)
        W[0, 0], W[N - 1, D - 1] = -0.1, 0.0999968
        c["W"] = W
        # the QAT table: looked-up elements beyond both clamps, on the grid, and exactly zero
        Wq = W.clone()
        ra, rb = int(c["rows"][0]), int(c["rows"][F - 1])
        Wq[ra, 0], Wq[rb, 1], Wq[ra, 2], Wq[rb, 3] = 0.5, -0.5, 0.0, -0.0
        c["Wqat"] = Wq
        _cases[key] = c
    return _cases[key]


def _all_finite(*tensors):
    """Nothing returned holds NaN (assert_within_terms alone would let one pass: NaN > bound is False)."""
    for t in tensors:
        if t is not None:
            assert bool(torch.isfinite(t._values() if t.is_sparse else t).all()), "a returned tensor holds NaN or inf"


def _codes(c, kind):
    """(table, scale, zero point) of a PTQ table of the case's fp32 table, as the embedding classes form them."""
    if kind == "fp16":
        return c["W"].to(torch.float16), None, None
    codes, scale, zp = affine_codes(c["W"], int(kind[3:]))
    assert int(zp) == 0
    exact = codes.to(torch.int32) - zp.to(torch.int32)
    assert int(exact.min()) >= torch.iinfo(codes.dtype).min and int(exact.max()) <= torch.iinfo(codes.dtype).max
    return codes, scale, zp


def _dev(t):
    return None if t is None else t.to(DEV)


# ---- the PTQ op -------------------------------------------------------------------------------------------------------
def _quant_fwd(c, Wq, scale, zp, x=None):
    x = c["x"] if x is None else x
    return quant_fm.gather_fm_quant(x.to(DEV), c["offsets"].to(DEV), Wq, c["w1"].to(DEV), c["bias"].to(DEV), scale, zp)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("kind", QKINDS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("F,D", SHAPES)
def test_quant_lookup_has_the_separate_lookups_bits_and_its_fm_term(F, D, B, kind, poison):
    c = _case(F, D, B)
    Wq, scale, zp = (_dev(t) for t in _codes(c, kind))
    rows = c["rows"].view(B, F).to(DEV)
    with torch.no_grad():
        want = _kernels.gather_rows_quant(rows, Wq, None if scale is None else scale.reshape(1), None if zp is None else zp.reshape(1))
        _, yfm_want = _kernels.fm_first_order(want, rows, c["w1"].to(DEV), c["bias"].to(DEV))
    with _maybe_poisoned(poison):
        emb, yfm = _quant_fwd(c, Wq, scale, zp)
        # a view whose base is one code past a word boundary: read in place by the scalar kernels, the same bits
        buf = torch.zeros(Wq.numel() + 1, dtype=Wq.dtype, device=DEV)
        buf[1:].copy_(Wq.view(-1))
        view = buf[1:].view(Wq.shape)
        assert view.data_ptr() % (4 * Wq.element_size()) != 0 and view.is_contiguous()
        emb_m, yfm_m = _quant_fwd(c, view, scale, zp)
    _lib.check_index_errors()
    _all_finite(emb, yfm, emb_m, yfm_m)
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (B, F, D) and tuple(yfm.shape) == (B,)
    assert not emb.requires_grad and not yfm.requires_grad
    assert torch.equal(emb.view(torch.int32), want.view(torch.int32)), "emb is not gather_rows_quant's bits"
    assert torch.equal(emb.cpu().view(torch.int32), qh.ptq_rows32(*_codes(c, kind))[c["rows"].view(B, F)].view(torch.int32))
    assert_close(yfm, yfm_want, 2e-5, 2e-5, "y_fm")
    assert torch.equal(emb_m.view(torch.int32), emb.view(torch.int32)), "the misaligned view changed emb"
    assert_close(yfm_m, yfm_want, 2e-5, 2e-5, "y_fm of the misaligned view")


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("kind", QKINDS)
def test_quant_lookup_out_of_range_and_empty_batch(kind, poison):
    for F, D in ((3, 4), (5, 12), (70, 8)):
        c = _case(F, D, 37)
        Wq, scale, zp = (_dev(t) for t in _codes(c, kind))
        x = c["x"].clone()
        x[3, 1] = c["N"] + 1000           # beyond the last row
        x[5, 0] = -12                     # negative
        with _maybe_poisoned(poison):
            emb, yfm = _quant_fwd(c, Wq, scale, zp, x=x)
            emb0, yfm0 = _quant_fwd(c, Wq, scale, zp, x=c["x"][:0])
        torch.cuda.synchronize()
        assert torch.count_nonzero(emb[3, 1]) == 0 and torch.count_nonzero(emb[5, 0]) == 0
        assert bool(torch.isfinite(emb).all()) and bool(torch.isfinite(yfm).all())
        with pytest.raises(IndexError):
            _lib.check_index_errors()
        _lib.check_index_errors()         # flag was cleared
        assert emb0.shape == (0, F, D) and yfm0.shape == (0,)
    with pytest.raises(TypeError):
        quant_fm.gather_fm_quant(c["x"].to(DEV), c["offsets"].to(DEV), c["W"].to(DEV), c["w1"].to(DEV), c["bias"].to(DEV))
    if kind != "fp16":
        with pytest.raises(ValueError, match="scale and zero point"):
            quant_fm.gather_fm_quant(c["x"].to(DEV), c["offsets"].to(DEV), Wq, c["w1"].to(DEV), c["bias"].to(DEV))


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("kind", ["fp16", "int8", "int16"])
def test_quant_lookup_reproduces_the_embedding_level_golden(kind, poison):
    g = load_golden("ptq")
    x = g.t("x").to(DEV)
    N = g.t("W").shape[0]
    if kind == "fp16":
        Wq, scale, zp = g.t("fp16_weight").view(torch.float16).to(DEV), None, None
    else:
        Wq, scale, zp = g.t(f"{kind}_weight").to(DEV), g.t(f"{kind}_scale").to(DEV), g.t(f"{kind}_bias").to(DEV)
    with _maybe_poisoned(poison):
        emb, yfm = quant_fm.gather_fm_quant(x, torch.zeros(x.shape[1], dtype=torch.int64, device=DEV), Wq,
                                            torch.zeros(N, 1, device=DEV), None, scale, zp)
    _lib.check_index_errors()
    _all_finite(emb, yfm)
    assert_close(emb, g.t(f"{kind}_out"), 0, 0, "the reference's dequantised rows")


# ---- the QAT op -------------------------------------------------------------------------------------------------------
def _qat_operands(c, bits, scale_grad=True):
    W = c["Wqat"].to(DEV).requires_grad_(True)
    scale = torch.tensor(SCALES[bits], device=DEV).requires_grad_(scale_grad)
    return W, scale, c["w1"].to(DEV).requires_grad_(True), c["bias"].to(DEV).requires_grad_(True)


def _qat_run(c, bits, draw, sparse=False, scale_grad=True, x=None):
    """One forward and backward of gather_fm_qat under the loss sum(emb * G) + sum(y_fm * gy).  draw: "prob" (the case's
    recorded draw) or a seed word."""
    W, scale, w1, bias = _qat_operands(c, bits, scale_grad)
    x = c["x"] if x is None else x
    kw = dict(prob=c["prob"][: x.shape[0]].to(DEV)) if draw == "prob" else dict(seed=torch.tensor([draw], device=DEV))
    emb, yfm = quant_fm.gather_fm_qat(x.to(DEV), c["offsets"].to(DEV), W, scale, bits, w1, bias, sparse_W=sparse,
                                      sparse_w1=sparse, **kw)
    ((emb * c["G"][: x.shape[0]].to(DEV)).sum() + (yfm * c["gy"][: x.shape[0]].to(DEV)).sum()).backward()
    return dict(emb=emb.detach(), yfm=yfm.detach(), gW=W.grad, gscale=scale.grad, gw1=w1.grad, gb=bias.grad)


def _separate_qat(c, bits, draw):
    """The parent's path: mi_qat_gather_fwd over x + offsets, then mi_fm_fwd."""
    B, F = c["x"].shape
    rows = c["rows"].view(B, F).to(DEV)
    prob, seed = (c["prob"].to(DEV), None) if draw == "prob" else (None, torch.tensor([draw], device=DEV))
    with torch.no_grad():
        emb = _QatLookup.apply(torch.tensor(SCALES[bits], device=DEV), c["Wqat"].to(DEV), rows, bits, seed, 0, prob, None)
        _, yfm = _kernels.fm_first_order(emb, rows, c["w1"].to(DEV), c["bias"].to(DEV))
    return emb, yfm


def _first_order_checks(c, r, sparse):
    B, F = c["x"].shape
    rows = c["rows"]
    ref1 = torch.zeros(c["N"], dtype=torch.float64).index_add_(0, rows, c["gy"].double().repeat_interleave(F))
    t1 = torch.zeros(c["N"], dtype=torch.float64).index_add_(0, rows, c["gy"].double().abs().repeat_interleave(F))
    assert r["gw1"].is_sparse == sparse
    assert_within_terms(r["gw1"].to_dense().view(-1) if sparse else r["gw1"].view(-1), ref1, t1, 8, "first-order gradient")
    assert_within_terms(r["gb"], c["gy"].double().sum().view(1), c["gy"].double().abs().sum().view(1), 8, "bias gradient")


def _grads_equal(a, b):
    for k in ("gW", "gscale", "gw1", "gb"):
        if a[k] is None:
            assert b[k] is None
            continue
        x, y = (a[k].to_dense(), b[k].to_dense()) if a[k].is_sparse else (a[k], b[k])
        assert torch.equal(x, y), f"{k} differs between two runs that promise the same bits"
    assert torch.equal(a["emb"], b["emb"]) and torch.equal(a["yfm"], b["yfm"])


def _check_qat_case(c, bits, draw, poison):
    B, F = c["x"].shape
    D, N = c["Wqat"].shape[1], c["N"]
    q_min, q_max = qh.q_range(bits)
    qf = c["Wqat"][c["rows"]] / torch.tensor(SCALES[bits])
    assert bool((qf >= q_max).any()) and bool((qf <= q_min).any()), "the case does not reach both clamp branches"
    emb_s, yfm_s = _separate_qat(c, bits, draw)
    if draw == "prob":
        want = qh.qat_rows32(c["Wqat"][c["rows"]].view(B, F, D), torch.tensor(SCALES[bits]), bits, c["prob"])
        assert torch.equal(emb_s.cpu().view(torch.int32), want.view(torch.int32)), "the separate lookup left the restatement"
    ref = None
    for form in ("dense", "det", "coo"):
        pkg.use_deterministic_algorithms(form == "det")
        try:
            with _maybe_poisoned(poison):
                r = _qat_run(c, bits, draw, sparse=form == "coo")
            if form == "det":      # (and the poisoned run equals the clean one bit for bit)
                _grads_equal(r, _qat_run(c, bits, draw))
        finally:
            pkg.use_deterministic_algorithms(False)
        _lib.check_index_errors()
        _all_finite(*r.values())
        assert torch.equal(r["emb"].view(torch.int32), emb_s.view(torch.int32)), "emb is not mi_qat_gather_fwd's bits"
        assert_close(r["yfm"], yfm_s, 2e-5, 2e-5, "y_fm")
        if ref is None:
            ref = qh.qat_backward64(r["emb"].cpu(), c["Wqat"][c["rows"]], torch.tensor(SCALES[bits]), bits, c["rows"], N,
                                    c["G"], c["gy"])
        g = r["gW"]
        if form == "coo":
            assert g.is_sparse and tuple(g.shape) == (N, D)
            assert torch.equal(g._indices().cpu().view(-1), c["rows"]), "the COO keys"
            assert_within_terms(g._values().cpu(), ref["dE"], ref["terms"], 8, "row-form table values")
        else:
            assert not g.is_sparse
            assert_within_terms(g, ref["gW"], ref["tW"], 8, f"{form}: dense table gradient")
        assert tuple(r["gscale"].shape) == ()
        assert_within_terms(r["gscale"].view(1), ref["gscale"].view(1), ref["tscale"].view(1), 8, f"{form}: scale gradient")
        _first_order_checks(c, r, form == "coo")


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("draw", ["prob", 1234567])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("F,D", SHAPES)
def test_qat_lookup_against_the_separate_lookup_and_float64(F, D, B, bits, draw, poison):
    _check_qat_case(_case(F, D, B), bits, draw, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("name", ["qat_int8", "qat_int16"])
def test_qat_lookup_reproduces_the_embedding_level_golden(name, poison):
    """g_y = 0 and g_emb = G: the fused backward is the embedding's own (tolerances of test_qat_matches_reference_golden)."""
    g = load_golden(name)
    bits, x = int(g["n_bits"]), g.t("x").to(DEV)
    W = g.t("param/_emb_module.weight").to(DEV).requires_grad_(True)
    scale = g.t("param/scale").to(DEV).requires_grad_(True)
    N = W.shape[0]
    with _maybe_poisoned(poison):
        emb, yfm = quant_fm.gather_fm_qat(x, torch.zeros(x.shape[1], dtype=torch.int64, device=DEV), W, scale, bits,
                                          torch.zeros(N, 1, device=DEV), None, prob=g.t("prob").to(DEV))
        (emb * g.t("G").to(DEV)).sum().backward()
    _lib.check_index_errors()
    _all_finite(emb, yfm, W.grad, scale.grad)
    assert_close(emb, g.t("out"), 0, 0, "rounded rows (same draw): bit-exact")
    assert_close(W.grad, g.t("grad/_emb_module.weight"), 1e-6, 1e-7, "row gradient")
    assert_close(scale.grad, g.t("grad/scale"), 1e-5, 1e-4, "scale gradient")


@pytest.mark.parametrize("poison", POISON)
def test_fixed_scale_gathers_no_table_row_and_wide_rows_are_refused(poison, monkeypatch):
    c = _case(26, 16, 37)
    lib = _lib.load()
    real, calls = lib.mi_gather_fm_qat_bwd_rows, []
    monkeypatch.setattr(lib, "mi_gather_fm_qat_bwd_rows", lambda *a: calls.append(a) or real(*a))
    with _maybe_poisoned(poison):
        r = _qat_run(c, 8, "prob", scale_grad=False)
        full = _qat_run(c, 8, "prob")
    _lib.check_index_errors()
    assert len(calls) == 2
    _all_finite(*r.values(), *full.values())
    assert calls[0][1] is None and calls[0][10] is None and calls[0][11] is None, "fixed scale: no table, no dscale, no workspace"
    assert calls[1][1] is not None and calls[1][10] is not None
    assert r["gscale"] is None and full["gscale"] is not None
    ref = qh.qat_backward64(r["emb"].cpu(), c["Wqat"][c["rows"]], torch.tensor(SCALES[8]), 8, c["rows"], c["N"], c["G"], c["gy"])
    assert_within_terms(r["gW"], ref["gW"], ref["tW"], 8, "fixed scale: dense table gradient")
    wide = torch.zeros(c["N"], quant_fm.QAT_BWD_MAX_D + 4, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        quant_fm.gather_fm_qat(c["x"].to(DEV), c["offsets"].to(DEV), wide, torch.tensor(0.001, device=DEV), 8, c["w1"].to(DEV),
                               None, seed=torch.tensor([1], device=DEV))
    with pytest.raises(NotImplementedError, match="scale gradient"):      # rintf(emb / scale) is the code only up to 21 bits
        quant_fm.gather_fm_qat(c["x"].to(DEV), c["offsets"].to(DEV), c["Wqat"].to(DEV),
                               torch.tensor(1e-7, device=DEV, requires_grad=True), 22, c["w1"].to(DEV), None,
                               seed=torch.tensor([1], device=DEV))
    with pytest.raises(ValueError, match="seed word or an explicit draw"):
        quant_fm.gather_fm_qat(c["x"].to(DEV), c["offsets"].to(DEV), c["Wqat"].to(DEV), torch.tensor(0.001, device=DEV), 8,
                               c["w1"].to(DEV), None)


@pytest.mark.parametrize("poison", POISON)
def test_qat_lookup_out_of_range_and_empty_batch(poison):
    for F, D in ((3, 4), (5, 12)):
        c = _case(F, D, 37)
        x = c["x"].clone()
        x[3, 1] = c["N"] + 1000
        x[5, 0] = -12
        for det in (False, True):
            pkg.use_deterministic_algorithms(det)
            try:
                with _maybe_poisoned(poison):
                    r = _qat_run(c, 8, "prob", x=x)
            finally:
                pkg.use_deterministic_algorithms(False)
            torch.cuda.synchronize()
            assert torch.count_nonzero(r["emb"][3, 1]) == 0 and torch.count_nonzero(r["emb"][5, 0]) == 0
            for k in ("gW", "gscale", "gw1", "gb"):
                assert bool(torch.isfinite(r[k]).all()), k
            with pytest.raises(IndexError):
                _lib.check_index_errors()
            _lib.check_index_errors()
        for sparse in (False, True):
            with _maybe_poisoned(poison):
                r = _qat_run(c, 8, "prob", sparse=sparse, x=c["x"][:0])
            assert r["emb"].shape == (0, F, D) and r["yfm"].shape == (0,)
            for k, shape in (("gW", c["Wqat"].shape), ("gw1", c["w1"].shape), ("gb", (1,)), ("gscale", ())):
                assert tuple(r[k].shape) == tuple(shape)
                assert torch.count_nonzero(r[k].to_dense() if r[k].is_sparse else r[k]) == 0, k
            _lib.check_index_errors()


# ---- launch names, deterministic mode ---------------------------------------------------------------------------------
def _qat_model(dims, D, hidden, bits=8, sparse=False, fixed_scale=False, seed=3):
    torch.manual_seed(seed)
    cfg = {"name": "qat", "n_bits": bits, "sparse": sparse, "fixed_scale": fixed_scale}
    return pkg.DeepFM(dims, D, hidden, p_dropout=0.0, use_batchnorm=False, embedding_config=cfg).to(DEV)


def _ptq_model(g, name, tmp_path):
    p = g.group("param/")
    D = p["embedding._emb_module.weight"].shape[1]
    m = pkg.DeepFM(g["dims"].tolist(), D, g["hidden"].tolist(), p_dropout=0.0, use_batchnorm=False)
    missing, unexpected = m.load_state_dict(p, strict=True)
    assert not missing and not unexpected
    path = qh.save_checkpoint(str(tmp_path / "deepfm" / "original.pth"), p["embedding._emb_module.weight"])
    # scripts/deepfm/run_ptq.py:109
    m.embedding = PTQEmb_Fp16(None, None, None, path) if name == "fp16" else PTQEmb_Int(None, None, None, path, int(name[3:]))
    return m.to(DEV).eval()


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("name", ["int4", "int8", "int16", "fp16"])
def test_a_ptq_eval_lookup_is_one_launch(name, poison, tmp_path):
    g = load_golden("quant_deepfm_ptq")
    m = _ptq_model(g, name, tmp_path)
    x = g.t("x").to(DEV)
    with _maybe_poisoned(poison), KernelTimer(64) as kt:
        with torch.no_grad():
            emb, yfm = m._fm_and_embedding(x)
        torch.cuda.synchronize()
    _all_finite(emb, yfm)
    assert [k for k, _ in kt.records] == ["gather_fm_quant_fwd"]      # (the parent: gather_rows_quant, fm_fwd behind a torch add)


@pytest.mark.parametrize("poison", POISON)
def test_a_qat_forward_is_one_launch_and_deterministic_mode_runs_no_atomic_kernel(poison):
    c = _case(26, 16, 1030)
    m = _qat_model(c["dims"], 16, [16])
    x = c["x"].to(DEV)
    with _maybe_poisoned(poison), KernelTimer(64) as kt:
        with torch.no_grad():
            emb, yfm = m._fm_and_embedding(x)
        torch.cuda.synchronize()
    _all_finite(emb, yfm)
    assert [k for k, _ in kt.records] == ["gather_fm_qat_fwd"]        # (the parent: qat_gather_fwd, fm_fwd behind a torch add)
    for det in (False, True):
        pkg.use_deterministic_algorithms(det)
        try:
            with _maybe_poisoned(poison), KernelTimer(64) as kt:
                r = _qat_run(c, 8, 99)
                torch.cuda.synchronize()
        finally:
            pkg.use_deterministic_algorithms(False)
        _all_finite(*r.values())
        names = [k for k, _ in kt.records]
        assert names[0] == "gather_fm_qat_fwd" and names.count("gather_fm_qat_fwd") == 1
        assert "gather_fm_qat_bwd_rows" in names
        assert not [k for k in names if k.startswith(("qat_gather", "fm_fwd", "fm_bwd"))], names
        if det:
            assert not [k for k in names if k.startswith(("scatter_axpy", "scatter_add"))], names


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("bits", [8, 16])
def test_deterministic_mode_gives_the_same_bits_twice_hot_rows_included(bits, poison):
    c = _case(26, 16, 1030)
    assert min(c["dims"]) == 2 and 3 in c["dims"], "fields of 2 and 3 values: rows hit hundreds of times"
    pkg.use_deterministic_algorithms(True)
    try:
        a = _qat_run(c, bits, 424242)
        with _maybe_poisoned(poison):
            b = _qat_run(c, bits, 424242)
    finally:
        pkg.use_deterministic_algorithms(False)
    _lib.check_index_errors()
    _grads_equal(a, b)
    _all_finite(*a.values(), *b.values())
    assert a["gscale"] is not None


# ---- the models -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("bits", [8, 16])
def test_the_fused_model_equals_the_hooked_one(bits, poison):
    """A no-op forward hook keeps the embedding module on its own forward (the parent's path); with the same rounding stream
    both models see the same rows."""
    dims = [2 + (7 * f) % 11 for f in range(26)]
    fused = _qat_model(dims, 16, [32, 16], bits)
    hooked = copy.deepcopy(fused)
    hooked.embedding.register_forward_hook(lambda mod, inp, out: None)
    x = _case(26, 16, 37)["x"].to(DEV)
    with _maybe_poisoned(poison):
        with torch.no_grad():
            emb_f, yfm_f = fused._fm_and_embedding(x)
            emb_h, yfm_h = hooked._fm_and_embedding(x)
            assert torch.equal(fused.embedding._sr_seed, hooked.embedding._sr_seed), "both paths advance the stream alike"
            lf, lh = fused(x), hooked(x)
    _lib.check_index_errors()
    _all_finite(emb_f, yfm_f, emb_h, yfm_h, lf, lh)
    assert torch.equal(emb_f.view(torch.int32), emb_h.view(torch.int32)), "the fused rows are not the module's"
    assert_close(yfm_f, yfm_h, 2e-5, 2e-5, "y_fm")
    assert_close(lf, lh, 2e-5, 2e-5, "logits")
    with KernelTimer(64) as kt:
        with torch.no_grad():
            hooked._fm_and_embedding(x)
        torch.cuda.synchronize()
    assert [k for k, _ in kt.records][:1] == ["qat_gather_fwd"], "the hooked model left the module's path"


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("form", ["dense", "rows", "deterministic"])
@pytest.mark.parametrize("bits", [8, 16])
def test_qat_logits_and_gradients_match_the_reference(bits, form, poison):
    g = load_golden("quant_deepfm_qat")
    p = g.group(f"b{bits}/param/")
    D = p["embedding._emb_module.weight"].shape[1]
    cfg = {"name": "qat", "n_bits": bits, "sparse": form == "rows"}
    m = pkg.DeepFM(g["dims"].tolist(), D, g["hidden"].tolist(), p_dropout=0.0, use_batchnorm=False, embedding_config=cfg)
    missing, unexpected = m.load_state_dict(p, strict=True)
    assert not missing and not unexpected
    m = m.to(DEV).train()
    x, y = g.t(f"b{bits}/x").to(DEV), g.t(f"b{bits}/y").to(DEV)

    def step():
        # the two lines of DeepFM.forward around the lookup, with the recorded draw in place of the generator
        m.zero_grad(set_to_none=True)
        emb, y_fm = quant_fm.gather_fm_qat(x, m.offsets, m.embedding.get_weight(), m.embedding.scale, bits, m.fc.weight, m._bias,
                                           prob=g.t(f"b{bits}/prob").to(DEV), sparse_W=m.embedding.sparse_grad)
        logits = run_tail(m._deep_branch, emb.reshape(emb.shape[0], -1), last_add=y_fm).squeeze(-1)
        torch.nn.BCEWithLogitsLoss()(logits, y).backward()
        return emb.detach(), logits.detach(), {k: (q.grad.to_dense() if q.grad.is_sparse else q.grad).clone()
                                               for k, q in m.named_parameters() if q.grad is not None}

    pkg.use_deterministic_algorithms(form == "deterministic")
    try:
        with _maybe_poisoned(poison):
            emb, logits, grads = step()
        if form == "deterministic":
            _, logits2, grads2 = step()
            assert torch.equal(logits, logits2)
            for k in grads:
                assert torch.equal(grads[k], grads2[k]), k
    finally:
        pkg.use_deterministic_algorithms(False)
    _lib.check_index_errors()
    _all_finite(emb, logits, *grads.values())
    assert_close(emb, g.t(f"b{bits}/emb"), 0, 0, "the reference's rounded rows")
    assert_close(logits, g.t(f"b{bits}/logits"), 2e-5, 2e-6, "logits")
    ref = g.group(f"b{bits}/grad/")
    assert set(grads) == set(ref), "a parameter's gradient is missing"
    for k, want in ref.items():
        assert_close(grads[k], want, 1e-4, 5e-6, f"grad {k}")
    assert m.embedding._emb_module.weight.grad.is_sparse == (form == "rows")


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("name", ["int4", "int8", "int16", "fp16"])
def test_ptq_eval_logits_match_the_reference(name, poison, tmp_path):
    g = load_golden("quant_deepfm_ptq")
    m = _ptq_model(g, name, tmp_path)
    x = g.t("x").to(DEV)
    with _maybe_poisoned(poison):
        with torch.no_grad():
            emb, _ = m._fm_and_embedding(x)
            logits = m(x)
    _lib.check_index_errors()
    _all_finite(emb, logits)
    assert_close(emb, g.t(f"{name}/emb"), 0, 0, "the reference's dequantised rows")
    assert_close(logits, g.t(f"{name}/logits"), 2e-5, 2e-6, "eval logits")


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("name", ["int8", "fp16"])
def test_a_ptq_model_with_grad_enabled_still_trains_its_first_order_term(name, poison, tmp_path):
    """The PTQ launch has no autograd node, so a forward that wants fc.weight.grad / _bias.grad keeps the module's path:
    the gradients are the hooked model's (the same kernels: the same bits).  With the two frozen, or under no_grad, the
    forward is the fused launch."""
    g = load_golden("quant_deepfm_ptq")
    model, hooked = _ptq_model(g, name, tmp_path), _ptq_model(g, name, tmp_path)
    hooked.embedding.register_forward_hook(lambda mod, inp, out: None)
    x = g.t("x").to(DEV)
    y = (torch.arange(x.shape[0], device=DEV) % 2).float()
    grads = []
    for m in (model, hooked):
        with _maybe_poisoned(poison), KernelTimer(64) as kt:
            logits = m(x)
            torch.nn.BCEWithLogitsLoss()(logits, y).backward()
            torch.cuda.synchronize()
        assert "gather_fm_quant_fwd" not in [k for k, _ in kt.records]
        assert m.fc.weight.grad is not None and m._bias.grad is not None, "the first-order term got no gradient"
        grads.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
        _all_finite(logits, *grads[-1].values())
    _lib.check_index_errors()
    assert set(grads[0]) == set(grads[1]) and {"fc.weight", "_bias"} <= set(grads[0])
    assert float(grads[0]["fc.weight"].abs().sum()) > 0 and float(grads[0]["_bias"].abs().sum()) > 0
    for k in ("fc.weight", "_bias"):
        assert torch.equal(grads[0][k], grads[1][k]), f"{k}.grad is not the hooked model's"
    model.fc.weight.requires_grad_(False), model._bias.requires_grad_(False)
    with KernelTimer(64) as kt:
        model._fm_and_embedding(x)          # grad enabled, nothing of y_fm wants a gradient: the fused launch
        torch.cuda.synchronize()
    assert [k for k, _ in kt.records] == ["gather_fm_quant_fwd"]


@pytest.mark.parametrize("poison", POISON)
def test_the_sparse_qat_config_takes_a_captured_sparse_adam_step(poison):
    """{"name": "qat", "sparse": True, "fixed_scale": True} with the reference's sparse optimizer split: before the fused
    lookup the QAT backward handed SparseAdam a dense gradient and the step raised."""
    dims = [7, 3, 11, 5]
    m = _qat_model(dims, 8, [12], sparse=True, fixed_scale=True, seed=17)
    opts = get_optimizers(m, {"sparse": True, "optimizer": "adam", "learning_rate": 1e-2, "weight_decay": 1e-6})
    assert isinstance(opts[0], SparseAdam)
    step = trainer.GraphedTrainStep(m, opts)
    gen = torch.Generator().manual_seed(5)
    W0 = m.embedding.get_weight().detach().clone()
    batches = []
    for _ in range(6):
        x = torch.stack([torch.randint(0, d, (24,), generator=gen) for d in dims], 1).to(DEV)
        batches.append((x, (torch.rand(24, generator=gen) < 0.4).float().to(DEV)))
    # (warm-up, capture and the replays all run with the allocations poisoned: the int64 row ids live in a float buffer
    #  that the graph's pool hands out again on every replay)
    with _maybe_poisoned(poison):
        for x, y in batches:
            loss = step(x, y)
    torch.cuda.synchronize()
    _lib.check_index_errors()
    assert step._graph is not None, "the step was not captured"
    _all_finite(loss, *(p.detach() for p in m.parameters()))
    assert not torch.equal(m.embedding.get_weight().detach(), W0), "the table did not move"
    assert m.embedding.scale.grad is None

"""GPU: the LDS ring of the tail products (recsys-benchmark_amd/csrc/tail_gemm.hpp: ring_produce / ring_consume) at every
reduction length at which its control flow differs: nst = 1..11 and 13 slices of 32 (every residue mod 3, both sides of the
cut at 9 where the exit-free steady state starts, the small-reduction line below 6), each as a whole number of slices, with
a partial slice that ends inside its first half (+16: the dead half) and one that does not (+20).

Through the C entry points tests/test_tail_operand_addressing_gpu.py drives, on NaN-poisoned outputs and Tee destinations
(a slice finished twice or never is a wrong value, a store outside the view a lost NaN), against float64 on the host within
that file's float32 summation bound (n + 8) eps32 |A| |B| — no tolerance of this file's own.  The statistics-joining forms
(the consumers' PRE barrier, constants read from LDS) run through the fused tail under tests/test_tail_gpu.py's bracket rule."""
import pytest
import torch

from test_tail_exact_cover_gpu import _bracket_failures
from test_tail_gpu import _reference, _run_fused, _seq
from test_tail_operand_addressing_gpu import EPS32, _Placed, _dgrad_case, _pack_keep, _sum_bound, _values
from tail_helpers import tail_keep_scale

from recsys_benchmark_amd import _kernels, _lib
from recsys_benchmark_amd import mlp as _mlp
from recsys_benchmark_amd.tail import SALT

pytestmark = pytest.mark.gpu
DEV = "cuda"
NST = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13]


def _lengths(nst):
    return [32 * nst, 32 * (nst - 1) + 16, 32 * (nst - 1) + 20]


def _d(t):
    return t.double()


def _forward(M, K, N, v):
    """Plain and activation (BatchNorm constants + dropout bits, Tee copy) forward products in the 112-column form (statistics
    asked for), the activation's operand on a pitch that is a multiple of 8 whatever K is."""
    lib = _lib.load()
    S = _lib.stream_ptr(torch.device(DEV, 0))
    pad = (8 - K % 8) % 8 + 8
    X = _Placed(M, K, True, pad, 8, v["X"])
    W = _Placed(N, K, False, 0, 0, v["W"])
    bits = _pack_keep(v["keep"], X.ld)
    mu, sc, be = (v[k].to(DEV) for k in ("mu", "sc", "be"))
    Z, Zp, A = _Placed(M, N, True, 12, 8), _Placed(M, N, True, 12, 8), _Placed(M, K, True, pad, 16)
    part = torch.full((int(lib.mi_tail_part_elems(M, N)),), float("nan"), device=DEV)
    _lib.check(lib.mi_tail_fwd_gemm(X.ptr(), X.ld, mu.data_ptr(), sc.data_ptr(), be.data_ptr(), 0.5, bits.data_ptr(), W.ptr(), W.ld,
                                    Z.ptr(), Z.ld, part.data_ptr(), A.ptr(), M, N, K, S), "fwd act")
    _lib.check(lib.mi_tail_fwd_gemm(X.ptr(), X.ld, None, None, None, 0.0, None, W.ptr(), W.ld, Zp.ptr(), Zp.ld, part.data_ptr(), None,
                                    M, N, K, S), "fwd plain")
    torch.cuda.synchronize()
    for name, pl in (("Z", Z), ("Zplain", Zp), ("A", A)):
        assert pl.untouched_outside(), f"forward {name} written outside its view"
    return Z.view.double().cpu(), Zp.view.double().cpu(), A.view.double().cpu()


def _check_forward(M, K, N, tag):
    v = _values(M, K, N, 7000 * M + 10 * K + N)
    Z, Zp, A = _forward(M, K, N, v)
    A64 = ((_d(v["X"]) - _d(v["mu"])) * _d(v["sc"]) + _d(v["be"])).clamp_min(0) * v["keep"].double() * 2.0
    absA = ((_d(v["X"]).abs() + _d(v["mu"]).abs()) * _d(v["sc"]).abs() + _d(v["be"]).abs()) * 2.0
    Wt = _d(v["W"]).t()
    assert bool(((A - A64).abs() <= 8 * EPS32 * absA + 1e-30).all()), f"{tag}: saved activation"
    assert bool(((Z - A @ Wt).abs() <= _sum_bound(A.abs(), Wt.abs(), K)).all()), f"{tag}: z of the activation"
    assert bool(((Zp - _d(v["X"]) @ Wt).abs() <= _sum_bound(_d(v["X"]).abs(), Wt.abs(), K)).all()), f"{tag}: plain z"


def _check_dgrad(M, red, cols, tag):
    """mi_tail_dgrad_gemm_s (plain and MID epilogue) and mi_tail_dgrad_gemm_fm with LoadDz and the Tee, reduction `red`."""
    v = _values(M, red, cols, 9000 * M + 10 * red + cols)
    out = _dgrad_case(M, red, cols, False, v)
    dz64 = _d(v["al"]) * _d(v["DY"]) + _d(v["bz"]) * (_d(v["Zl"]) - _d(v["dmu"])) + _d(v["de"])
    absdz = _d(v["al"]).abs() * _d(v["DY"]).abs() + _d(v["bz"]).abs() * (_d(v["Zl"]).abs() + _d(v["dmu"]).abs()) + _d(v["de"]).abs()
    Wd = _d(v["Wd"])
    for form in ("plain", "mid", "fm"):
        dz = out[f"{form}.DZ"].double().cpu()
        assert bool(((dz - dz64).abs() <= 8 * EPS32 * absdz).all()), f"{tag} {form}: saved dz"
    da, bound = dz @ Wd, _sum_bound(dz.abs(), Wd.abs(), red)
    assert bool(((out["plain.OUT"].double().cpu() - da).abs() <= bound).all()), f"{tag}: dx"
    pre32 = torch.addcmul(v["pbe"], v["pZ"] - v["pmu"], v["psc"])
    gate = (v["pkeep"].double() * 2.0 if cols % 8 == 0 else 1.0) * (pre32 > 0).double()
    ok = ((out["mid.OUT"].double().cpu() - da * gate).abs() <= bound * 2.0 * (1 + 4 * EPS32)) | (pre32.abs() < 1e-6)
    assert bool(ok.all()), f"{tag}: dy of the previous layer"
    F = cols // 4
    fm = da + _d(v["gy"])[:, None] * (_d(v["esum"]).repeat(1, F) - _d(v["emb"]))
    fm_bound = bound + 4 * EPS32 * (da.abs() + _d(v["gy"]).abs()[:, None] * (_d(v["esum"]).abs().repeat(1, F) + _d(v["emb"]).abs()))
    assert bool(((out["fm.OUT"].double().cpu() - fm).abs() <= fm_bound).all()), f"{tag}: row-form table gradient"


@pytest.mark.parametrize("nst", NST)
def test_forward_and_input_gradient_at_every_reduction_length(nst):
    for red in _lengths(nst):
        _check_forward(64, red, 100, f"forward K={red}")
        _check_dgrad(64, red, 100, f"dgrad N={red}")


@pytest.mark.parametrize("cols", [100, 104, 36, 4])
@pytest.mark.parametrize("M", [64, 80])
def test_every_consumer_instance_and_a_partial_row_tile(M, cols):
    """100 = 6 sub-tiles + the group, 104 = seven sub-tiles, 36 = 2 + the group, 4 = the group alone; 13 slices with a dead half,
    9 slices with a live partial one, 6 whole slices."""
    for red in (400, 276, 192):
        _check_forward(M, red, cols, f"forward M={M} K={red} N={cols}")
        _check_dgrad(M, red, cols, f"dgrad M={M} N={red} K={cols}")


@pytest.mark.parametrize("nst", NST)
def test_statistics_joining_forms_through_the_fused_tail(nst, monkeypatch):
    """Layer 2's forward product and both input gradients reduce over the hidden width with the constants joined by the
    consumers (the PRE barrier) and read from LDS.  Widths are multiples of 8 there, so +24 stands for +20."""
    from recsys_benchmark_amd import tail as _tail_mod

    monkeypatch.setattr(_mlp, "FUSED_TAIL", True)
    monkeypatch.setattr(_mlp, "_LinearFn", None)
    monkeypatch.setattr(_tail_mod, "STAT_SUMS", True)
    monkeypatch.setattr(_tail_mod, "MERGE_JOINS", False)
    M, K = 80, 48
    for width in (32 * nst, 32 * (nst - 1) + 16, 32 * (nst - 1) + 24):
        hidden = [width, width]
        torch.manual_seed(100 * nst + width)
        seq = _seq(K, hidden, 0.5, bn=True).train(True)
        x, add, G = torch.randn(M, K) * 0.7 + 0.2, torch.randn(M), torch.randn(M, 1) + 0.5
        seed_value = 1977 + width
        masks = [tail_keep_scale(seed_value, SALT * (i + 1), M, h, 0.5) for i, h in enumerate(hidden)]
        near = []
        ref64 = _reference(seq, x, add, masks, torch.float64, near_out=near)
        ref32 = _reference(seq, x, add, masks, torch.float32)
        for r in (ref64, ref32):
            (r[3] * G.to(r[3].dtype)).sum().backward()
        fused = _run_fused(seq, x, add, seed_value)
        (fused[3] * G.to(DEV)).sum().backward()
        bad = _bracket_failures(M, hidden, True, seq, fused, ref64, ref32)
        if bad and near:
            for bits in range(1, 1 << len(near)):
                alt = _reference(seq, x, add, masks, torch.float64, flips={"list": near, "which": {j for j in range(len(near)) if bits >> j & 1}})
                (alt[3] * G.double()).sum().backward()
                if not _bracket_failures(M, hidden, True, seq, fused, alt, ref32):
                    bad = []
                    break
        assert not bad, f"width {width}: {bad} (near the kink: {near})"


@pytest.mark.parametrize("nst", NST)
def test_weight_gradient_and_panel_products_on_general_addressing(nst):
    """k_tail_wgrad reduces over the rows (M = the reduction lengths; plain operands and dz x activation) and the panel product
    over K in both layouts: the operands with general addressing, which walk the same schedule in one loop."""
    lib = _lib.load()
    S = _lib.stream_ptr(torch.device(DEV, 0))
    N, K = 64, 100
    for M in _lengths(nst):
        v = _values(M, N, K, 500 * M + nst)
        dz64 = _d(v["al"]) * _d(v["DY"]) + _d(v["bz"]) * (_d(v["Zl"]) - _d(v["dmu"])) + _d(v["de"])
        a64 = ((_d(v["pZ"]) - _d(v["pmu"])) * _d(v["psc"]) + _d(v["pbe"])).clamp_min(0)
        DY, Zl, pZ = v["DY"].to(DEV), v["Zl"].to(DEV), v["pZ"].to(DEV)
        c = [v[k].to(DEV) for k in ("dmu", "al", "bz", "de")]
        pc = [v[k].to(DEV) for k in ("pmu", "psc", "pbe")]
        splits = int(lib.mi_tail_wgrad_splits(M, N, K))
        for form in ("plain", "dz-act"):
            slab = torch.full((splits, N, K), float("nan"), device=DEV)
            dW = torch.full((N, K), float("nan"), device=DEV)
            if form == "plain":
                _lib.check(lib.mi_tail_wgrad_gemm(DY.data_ptr(), None, N, None, None, None, None, pZ.data_ptr(), K, None, None, None, 0.0,
                                                  None, slab.data_ptr(), dW.data_ptr(), M, N, K, S), "wgrad plain")
                L, R = _d(v["DY"]), _d(v["pZ"])
            else:
                _lib.check(lib.mi_tail_wgrad_gemm(DY.data_ptr(), Zl.data_ptr(), N, *[t.data_ptr() for t in c], pZ.data_ptr(), K,
                                                  *[t.data_ptr() for t in pc], 0.0, None, slab.data_ptr(), dW.data_ptr(), M, N, K, S), "wgrad dz")
                L, R = dz64, a64
            # operands rounded in float32 on the way in: a few eps of their terms, carried by the (n + 8) of the bound
            absL = _d(v["al"]).abs() * _d(v["DY"]).abs() + _d(v["bz"]).abs() * (_d(v["Zl"]).abs() + _d(v["dmu"]).abs()) + _d(v["de"]).abs() \
                if form != "plain" else L.abs()
            absR = (_d(v["pZ"]).abs() + _d(v["pmu"]).abs()) * _d(v["psc"]).abs() + _d(v["pbe"]).abs() if form != "plain" else R.abs()
            bound = _sum_bound(absL.t(), absR, M) * (1 + splits * EPS32)
            if form != "plain":
                # an activation on the ReLU kink may fall on either side in float32: its column's sums may differ by its terms
                pre32 = torch.addcmul(v["pbe"], v["pZ"] - v["pmu"], v["psc"])
                on_kink = (pre32.abs() < 1e-6).double()
                bound = bound + absL.t() @ (on_kink * absR)
            got = dW.double().cpu()
            assert bool(((got - L.t() @ R).abs() <= bound).all()), f"wgrad {form} M={M}"
        # the panel product on integer-valued data: exact in any order
        g = torch.Generator().manual_seed(M)
        A = torch.randint(-3, 4, (64, M), generator=g).float()
        for layout in (0, 1):
            B = torch.randint(-3, 4, (100, M) if layout == 0 else (M, 100), generator=g).float()
            C = torch.full((64, 100), float("nan"), device=DEV)
            assert _kernels.gemm_panel(A.to(DEV), M, B.to(DEV), B.shape[1], layout, C, 100, 64, 100, M)
            assert torch.equal(C.cpu(), A @ (B.t() if layout == 0 else B)), f"panel layout {layout} K={M}"

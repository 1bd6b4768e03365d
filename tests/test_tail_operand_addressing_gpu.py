"""GPU: the operand addressing of the fused MLP tail's products (recsys-benchmark_amd/csrc/tail_gemm.hpp, "LEAN addressing"):
every global access of a lean loader goes through a buffer descriptor based at the workgroup's tile and as long as the tile's
true extent, (rows - 1) * ld + cols floats, and a thread's LDS chunks share one address.

Bracket rule: tests/test_tail_gpu.py's rule as it stands (K_BRACKET = 8 against the float64 evaluation, relative to the stock
float32 modules' own error), in the three statistics forms, at the smallest shapes at which an address can go wrong: a partial
row tile, a dead half slice, one partial slice, no partial slice, two layers with Tee outputs on ragged tiles, remainder 8.

Address independence: the C entry points are called the way bench.py's DgradBench calls them, once on contiguous tensors and
once on views with a row pitch above the width and a non-zero, 16-byte-aligned storage offset, every matrix at the very END of
a NaN-filled allocation (its last row ends where the storage ends: a descriptor one element too long would reach past the
allocation, one too short would read zeros).  The two results are bit-equal, the saved Tee copies too, nothing outside the
output views is written, and the contiguous result lies within the float32 summation bound of the float64 evaluation."""
import itertools

import pytest
import torch

from test_tail_exact_cover_gpu import _bracket_failures
from test_tail_gpu import _fused_tail_on, _reference, _run_fused, _seq  # noqa: F401  (the fixture runs every test in the three forms)
from tail_helpers import tail_keep_scale

from recsys_benchmark_amd import _lib
from recsys_benchmark_amd import mlp as _mlp
from recsys_benchmark_amd.tail import SALT

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (M, K, hidden).  Forward product of layer l: reduction = its input width, columns = its width; the input-gradient product
# of layer l: reduction = its width, columns = its input width.
CASES = [
    (67, 48, [136]),          # partial row tile; reduction 48 = 32 + 16: the dead half slice; dgrad reduces over 136 = 4 x 32 + 8
    (67, 16, [24]),           # one partial slice (the unpipelined step)
    (67, 64, [24]),           # no partial slice
    (130, 48, [200, 104]),    # two layers: Tee outputs on ragged tiles, the MID epilogue
    (200, 40, [200]),         # remainder 8
]
MODES = ["bn-train", "nobn-eval"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,hidden", CASES)
def test_buffer_addressed_tail_brackets_float64_like_the_stock_modules(M, K, hidden, mode, monkeypatch):
    monkeypatch.setattr(_mlp, "_LinearFn", None)      # the general path must not be what computes any of this
    torch.manual_seed(M + K + sum(hidden))
    training = mode.endswith("train")
    p = 0.5 if training else 0.0
    seq = _seq(K, hidden, p, bn=mode.startswith("bn")).train(training)
    x = torch.randn(M, K) * 0.7 + 0.2
    add = torch.randn(M)
    G = torch.randn(M, 1) + 0.5      # (an upstream gradient with a mean: see tests/test_tail_exact_cover_gpu.py)
    seed_value = 977 + M
    masks = [tail_keep_scale(seed_value, SALT * (i + 1), M, h, p) for i, h in enumerate(hidden)]
    near = []
    ref64 = _reference(seq, x, add, masks, torch.float64, near_out=near)
    ref32 = _reference(seq, x, add, masks, torch.float32)
    for r in (ref64, ref32):
        (r[3] * G.to(r[3].dtype)).sum().backward()
    fused = _run_fused(seq, x, add, seed_value)
    (fused[3] * G.to(DEV)).sum().backward()
    bad = _bracket_failures(M, hidden, training, seq, fused, ref64, ref32)
    if bad and near:      # pre-activations on the ReLU kink: one assignment of their decisions has to match
        for bits in range(1, 1 << len(near)):
            alt = _reference(seq, x, add, masks, torch.float64, flips={"list": near, "which": {j for j in range(len(near)) if bits >> j & 1}})
            (alt[3] * G.double()).sum().backward()
            if not _bracket_failures(M, hidden, training, seq, fused, alt, ref32):
                bad = []
                break
    assert not bad, f"{bad} (pre-activations near the kink: {near})"


# ---------------------------------------------------------------------------------------------- address independence
EPS32 = 2.0 ** -24


class _Placed:
    """One matrix of the test in one of two placements.  strided=False: a contiguous tensor.  strided=True: a view with row
    pitch `ld` > width whose last element is the last element of a NaN-filled storage and whose first element lies `off`
    floats (a multiple of 4: 16 bytes) into it."""

    def __init__(self, rows, cols, strided, pad, off, values=None):
        self.rows, self.cols = rows, cols
        self.ld = cols + pad if strided else cols
        self.off = off if strided else 0
        n = self.off + (rows - 1) * self.ld + cols
        self.store = torch.full((n,), float("nan"), device=DEV)
        self.view = self.store[self.off:].as_strided((rows, cols), (self.ld, 1))
        assert self.view.data_ptr() % 16 == 0 and self.ld % 4 == 0
        if values is not None:
            self.view.copy_(values)

    def ptr(self):
        return self.view.data_ptr()

    def untouched_outside(self):
        """Every element of the storage outside the view is still NaN."""
        seen = torch.zeros_like(self.store, dtype=torch.bool)
        seen[self.off:].as_strided((self.rows, self.cols), (self.ld, 1)).fill_(True)
        return bool(torch.isnan(self.store[~seen]).all())


def _pack_keep(keep, ld):
    """keep [M, C] bool -> the kernels' keep bits for an activation of row pitch ld: element (m, c) is bit (c & 7) of byte
    (m * ld + c) >> 3; exactly as many bytes as the last element needs."""
    M, C = keep.shape
    flat = torch.zeros((M - 1) * ld + C + 7, dtype=torch.uint8)
    flat[:(M - 1) * ld + C].as_strided((M, C), (ld, 1)).copy_(keep.to(torch.uint8))
    nbytes = ((M - 1) * ld + C + 7) // 8
    b = flat[:nbytes * 8].view(nbytes, 8).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8).to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sum_bound(absA, absB, n):
    """Forward error bound of a float32 sum of n products in any order, operands rounded a few times on the way in:
    (n + 8) eps32 (|A| |B|), elementwise, evaluated in float64."""
    return (n + 8) * EPS32 * (absA @ absB) + 1e-30


def _forward_case(M, K, N, strided, vals):
    """z = a(X) W^T through mi_tail_fwd_gemm with the Tee copy of a(X): the 112-column form (statistics asked for) and the
    32-column small-batch form (no statistics).  Returns {name: tensor} of everything the launches wrote."""
    lib = _lib.load()
    S = _lib.stream_ptr(torch.device(DEV, 0))
    X = _Placed(M, K, strided, 8, 12, vals["X"])
    W = _Placed(N, K, strided, 4, 4, vals["W"])
    bits = _pack_keep(vals["keep"], X.ld)
    mu, sc, be = (vals[k].to(DEV) for k in ("mu", "sc", "be"))
    out = {}
    for form in ("stats", "small"):
        Z = _Placed(M, N, strided, 12, 8)
        A = _Placed(M, K, strided, 8, 20)       # the Tee copy has the operand's pitch
        assert A.ld == X.ld
        part = torch.full((int(lib.mi_tail_part_elems(M, N)),), float("nan"), device=DEV) if form == "stats" else None
        _lib.check(lib.mi_tail_fwd_gemm(X.ptr(), X.ld, mu.data_ptr(), sc.data_ptr(), be.data_ptr(), 0.5, bits.data_ptr(), W.ptr(), W.ld,
                                        Z.ptr(), Z.ld, _lib.ptr(part), A.ptr(), M, N, K, S), "fwd act")
        Zp = _Placed(M, N, strided, 12, 8)
        _lib.check(lib.mi_tail_fwd_gemm(X.ptr(), X.ld, None, None, None, 0.0, None, W.ptr(), W.ld, Zp.ptr(), Zp.ld, _lib.ptr(part), None,
                                        M, N, K, S), "fwd plain")
        torch.cuda.synchronize()
        for name, pl in (("Z", Z), ("A", A), ("Zplain", Zp)):
            assert pl.untouched_outside(), f"forward {form}: {name} written outside its view"
            out[f"{form}.{name}"] = pl.view.clone()
        if part is not None:
            out["stats.part"] = part.clone()
    return out


def _dgrad_case(M, N, K, strided, vals):
    """dx = dz W through mi_tail_dgrad_gemm_s (last layer: plain output; middle layer: the MID epilogue) and
    mi_tail_dgrad_gemm_fm, each with the Tee copy of dz."""
    lib = _lib.load()
    S = _lib.stream_ptr(torch.device(DEV, 0))
    DY = _Placed(M, N, strided, 8, 12, vals["DY"])
    Zl = _Placed(M, N, strided, 8, 4, vals["Zl"])
    assert DY.ld == Zl.ld
    W = _Placed(N, K, strided, 4, 8, vals["Wd"])
    pZ = _Placed(M, K, strided, 8, 16, vals["pZ"])
    pbits = _pack_keep(vals["pkeep"], pZ.ld) if pZ.ld % 8 == 0 else None      # keep bits need a pitch that is a multiple of 8
    c = [vals[k].to(DEV) for k in ("dmu", "al", "bz", "de")]
    pc = [vals[k].to(DEV) for k in ("pmu", "psc", "pbe")]
    D = 4
    emb, esum, gy = vals["emb"].to(DEV), vals["esum"].to(DEV), vals["gy"].to(DEV)
    out = {}
    for form in ("plain", "mid", "fm"):
        DZ = _Placed(M, N, strided, 8, 24)
        assert DZ.ld == DY.ld
        if form == "fm":
            OUT = _Placed(M, K, False, 0, 0)          # the table's row-form gradient: pitch K by contract
            g1 = torch.full((M, K // D), float("nan"), device=DEV)
            _lib.check(lib.mi_tail_dgrad_gemm_fm(DY.ptr(), Zl.ptr(), DY.ld, *[t.data_ptr() for t in c], W.ptr(), W.ld, OUT.ptr(), DZ.ptr(),
                                                 M, N, K, None, emb.data_ptr(), esum.data_ptr(), gy.data_ptr(), g1.data_ptr(), D, S), "dgrad fm")
            out["fm.g1"] = g1
        else:
            OUT = _Placed(M, K, strided, 12, 4)
            mid = form == "mid"
            part = torch.full((int(lib.mi_tail_part_elems(M, K)),), float("nan"), device=DEV) if mid else None
            _lib.check(lib.mi_tail_dgrad_gemm_s(DY.ptr(), Zl.ptr(), DY.ld, *[t.data_ptr() for t in c], W.ptr(), W.ld,
                                                pZ.ptr() if mid else None, pZ.ld, *[(t.data_ptr() if mid else None) for t in pc],
                                                0.5 if mid and pbits is not None else 0.0, _lib.ptr(pbits) if mid else None, OUT.ptr(), OUT.ld,
                                                _lib.ptr(part), 0,
                                                DZ.ptr(), M, N, K, None, S), "dgrad")
            if mid:
                out["mid.part"] = part
        torch.cuda.synchronize()
        for name, pl in (("OUT", OUT), ("DZ", DZ)):
            assert pl.untouched_outside(), f"dgrad {form}: {name} written outside its view"
            out[f"{form}.{name}"] = pl.view.clone()
    return out


def _values(M, red, cols, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    v = {
        # forward: X [M, red], W [cols, red]
        "X": r(M, red), "W": r(cols, red) / red ** 0.5, "keep": torch.rand(M, red, generator=g) < 0.5,
        "mu": r(red) * 0.1, "sc": torch.rand(red, generator=g) + 0.5, "be": r(red) * 0.1,
        # input gradient: DY, Zl [M, red], W [red, cols], previous layer [M, cols]
        "DY": r(M, red), "Zl": r(M, red), "Wd": r(red, cols) / red ** 0.5, "pZ": r(M, cols), "pkeep": torch.rand(M, cols, generator=g) < 0.5,
        "dmu": r(red) * 0.3, "al": r(red) * 0.3 + 1.0, "bz": r(red) * 0.3, "de": r(red) * 0.3,
        "pmu": r(cols) * 0.1, "psc": torch.rand(cols, generator=g) + 0.5, "pbe": r(cols) * 0.1,
        "emb": r(M, cols), "esum": r(M, 4), "gy": r(M),
    }
    return v


@pytest.mark.parametrize("M,red,cols", list(itertools.product([67, 130], [48, 136], [100, 104])))
def test_products_do_not_depend_on_pitch_offset_or_what_lies_beyond_the_operands(M, red, cols):
    v = _values(M, red, cols, 1000 * M + 10 * red + cols)
    d = lambda t: t.double()
    # ---- forward
    flat, view = _forward_case(M, red, cols, False, v), _forward_case(M, red, cols, True, v)
    assert flat.keys() == view.keys()
    for k in flat:
        assert _same_bits(flat[k], view[k]), f"forward {k}: contiguous and strided placements differ"
    A64 = ((d(v["X"]) - d(v["mu"])) * d(v["sc"]) + d(v["be"])).clamp_min(0) * v["keep"].double() * 2.0
    absA = ((d(v["X"]).abs() + d(v["mu"]).abs()) * d(v["sc"]).abs() + d(v["be"]).abs()) * 2.0
    Wt = d(v["W"]).t()
    for form in ("stats", "small"):
        got = flat[f"{form}.A"].double().cpu()
        # the activation itself: a handful of roundings of its terms; an element on the ReLU kink may fall on either side
        assert bool(((got - A64).abs() <= 8 * EPS32 * absA + 1e-30).all()), f"forward {form}: saved activation"
        assert bool(((flat[f"{form}.Z"].double().cpu() - got @ Wt).abs() <= _sum_bound(got.abs(), Wt.abs(), red)).all()), f"forward {form}: z"
        assert bool(((flat[f"{form}.Zplain"].double().cpu() - d(v["X"]) @ Wt).abs() <= _sum_bound(d(v["X"]).abs(), Wt.abs(), red)).all()), \
            f"forward {form}: plain z"
    # ---- input gradient
    flat, view = _dgrad_case(M, red, cols, False, v), _dgrad_case(M, red, cols, True, v)
    assert flat.keys() == view.keys()
    for k in flat:
        assert _same_bits(flat[k], view[k]), f"dgrad {k}: contiguous and strided placements differ"
    dz64 = d(v["al"]) * d(v["DY"]) + d(v["bz"]) * (d(v["Zl"]) - d(v["dmu"])) + d(v["de"])
    absdz = d(v["al"]).abs() * d(v["DY"]).abs() + d(v["bz"]).abs() * (d(v["Zl"]).abs() + d(v["dmu"]).abs()) + d(v["de"]).abs()
    Wd = d(v["Wd"])
    for form in ("plain", "mid", "fm"):
        dz = flat[f"{form}.DZ"].double().cpu()
        assert bool(((dz - dz64).abs() <= 8 * EPS32 * absdz).all()), f"dgrad {form}: saved dz"
    da, bound = dz @ Wd, _sum_bound(dz.abs(), Wd.abs(), red)
    assert bool(((flat["plain.OUT"].double().cpu() - da).abs() <= bound).all()), "dgrad plain: dx"
    pre32 = torch.addcmul(v["pbe"], v["pZ"] - v["pmu"], v["psc"])      # the kernel decides the ReLU mask in float32 (fma)
    gate = (v["pkeep"].double() * 2.0 if cols % 8 == 0 else 1.0) * (pre32 > 0).double()      # (100 columns: no keep bits)
    kink = pre32.abs() < 1e-6                                           # (either decision: not checked)
    ok = ((flat["mid.OUT"].double().cpu() - da * gate).abs() <= bound * 2.0 * (1 + 4 * EPS32)) | kink
    assert bool(ok.all()), "dgrad mid: dy of the previous layer"
    F = cols // 4
    fm = da + d(v["gy"])[:, None] * (d(v["esum"]).repeat(1, F) - d(v["emb"]))
    fm_bound = bound + 4 * EPS32 * (da.abs() + d(v["gy"]).abs()[:, None] * (d(v["esum"]).abs().repeat(1, F) + d(v["emb"]).abs()))
    assert bool(((flat["fm.OUT"].double().cpu() - fm).abs() <= fm_bound).all()), "dgrad fm: row-form table gradient"
    assert torch.equal(flat["fm.g1"].cpu(), v["gy"][:, None].expand(M, F)), "dgrad fm: first-order gradient values"

"""GPU: the exact column cover of the fused MLP tail's products (recsys-benchmark_amd/csrc/tail_gemm.hpp): a column tile of
16 nfull + 4 columns runs nfull sub-tiles on v_mfma_f32_16x16x4_f32 and one four-column group on v_mfma_f32_4x4x1_16b_f32
(four k-class chains summed in the epilogue) and never writes the tile's columns beyond the cover; tiles with 8 or 12
columns left over keep the full-sub-tile path; the partial reduction slice's all-zero upper half is skipped.  Same rule as
tests/test_tail_gpu.py: the fused result lies as close to the float64 evaluation of the reference's op sequence as the
stock float32 modules do, up to k = 8 — at the smallest shapes that reach every (left-over columns, reduction remainder)
form, in the three forms of the BatchNorm statistics.  The fused node takes widths that are multiples of 8 only
(tail.fused_tail_plan), so a left-over of 4 or 12 columns needs two column tiles: 136 = 2 x 68, 120 = 2 x 60,
200 = 2 x 100 stand where a single tile of 20, 28 or 100 columns cannot exist, and a reduction remainder of 24 where 20
cannot."""
import copy

import pytest
import torch

import oracle.reference_ops as ro
from conftest import assert_close
from tail_helpers import tail_keep_scale
from test_tail_gpu import _fused_tail_on, _reference, _run_fused, _seq  # noqa: F401  (the fixture runs every test in the three forms)

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import _lib
from recsys_benchmark_amd import mlp as _mlp
from recsys_benchmark_amd.mlp import run_tail
from recsys_benchmark_amd.tail import SALT

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (M, K, hidden, p).  Forward product of layer l: reduction = its input width, columns = its width; the input-gradient
# product of layer l: reduction = its width, columns = its input width.  cover = (full sub-tiles, left-over columns / 4).
CASES = [
    # left-over 4, 8, 12 and 0 columns; M = 67: a partial row tile; K = 48: remainder 16, the dead half is skipped
    (67, 48, [136], 0.5),      # 2 tiles of 68: cover (4, 1); dgrad reduces over 136 = 4 x 32 + 8 (dead half)
    (67, 48, [24], 0.5),       # (1, 2): full-sub-tile path; dgrad reduces over 24: one partial slice, no dead half
    (67, 48, [120], 0.5),      # 2 tiles of 60: (3, 3)
    (67, 48, [32], 0.5),       # (2, 0)
    (130, 48, [200], 0.5),     # 2 tiles of 100, the headline tile: (6, 1); dgrad reduces over 200 = 6 x 32 + 8; three row tiles
    (130, 48, [104], 0.5),     # (6, 2); dgrad reduces over 104 = 3 x 32 + 8
    # reduction remainders of the forward product (multiples of 8 like every width: 24 stands for a remainder above 16);
    # the dgrad columns K give the covers (2, 2), (3, 2), (1, 0), (4, 0)
    (67, 40, [24], 0.5),       # remainder 8
    (67, 56, [24], 0.5),       # remainder 24: no skip
    (67, 16, [24], 0.5),       # one partial slice: the unpipelined path, remainder 16
    (67, 64, [24], 0.5),       # no partial slice
    # a reduction shorter than one slice in front of / behind a 100-column tile: the unpipelined step keeps whole sub-tiles
    (130, 16, [200], 0.5),     # forward reduces over 16
    (130, 48, [200, 16], 0.5), # the second layer's dgrad reduces over 16 into 2 tiles of 100 (MID epilogue)
    # enough row tiles (65 x 2 >= 128) for the 112-column form WITHOUT statistics: the inference forward, head in the epilogue
    (4100, 48, [200], 0.5),
    # two layers: the MID epilogue, the statistics and the Tee outputs on ragged tiles; four row tiles, the last partial
    (200, 48, [200, 104], 0.5),
]
MODES = ["bn-train", "nobn-eval"]
K_BRACKET = 8.0


def _bracket_failures(M, hidden, training, seq, fused, ref64, ref32, floor=1e-6):
    """|got - r64| <= K_BRACKET * max(|r32 - r64|, floor), relative to max |r64|, for the output, every gradient and the
    running statistics (tests/test_tail_gpu.py's rule and factor)."""
    fs, fx, fa, fout = fused
    lin_in_front_of_bn = {f"{i}.bias" for i, m in enumerate(seq) if isinstance(m, torch.nn.Linear) and i + 1 < len(seq)
                          and isinstance(seq[i + 1], torch.nn.BatchNorm1d) and training}
    bad = []

    def check(name, got, r64, r32):
        got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
        scale = r64.abs().max().clamp_min(1e-30)
        err_f = (got - r64).abs().max() / scale
        err_s = (r32 - r64).abs().max() / scale
        if not err_f <= max(K_BRACKET * err_s, floor):
            bad.append(f"{name}: fused {err_f:.3e} vs stock {err_s:.3e} (relative to max |ref|)")

    check("out", fout, ref64[3], ref32[3])
    check("dx", fx.grad, ref64[1].grad, ref32[1].grad)
    check("dadd", fa.grad, ref64[2].grad, ref32[2].grad)
    p64, p32, pf = dict(ref64[0].named_parameters()), dict(ref32[0].named_parameters()), dict(fs.named_parameters())
    for name in p64:
        if name in lin_in_front_of_bn:
            assert float(pf[name].grad.abs().max()) == 0.0      # analytically zero: the batch mean is removed
            continue
        check(name, pf[name].grad, p64[name].grad, p32[name].grad)
    b64, b32, bf = dict(ref64[0].named_buffers()), dict(ref32[0].named_buffers()), dict(fs.named_buffers())
    for name in b64:
        if name.endswith("num_batches_tracked"):
            assert int(bf[name]) == int(b64[name])
        else:
            check(name, bf[name], b64[name], b32[name])
    return bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,hidden,p", CASES)
def test_exact_cover_brackets_float64_like_the_stock_modules(M, K, hidden, p, mode, monkeypatch):
    monkeypatch.setattr(_mlp, "_LinearFn", None)      # the general path must not be what computes any of this
    torch.manual_seed(M + K + sum(hidden))
    training = mode.endswith("train")
    seq = _seq(K, hidden, p, bn=mode.startswith("bn")).train(training)
    x = torch.randn(M, K) * 0.7 + 0.2
    add = torch.randn(M)
    # (an upstream gradient with a mean: the head bias's gradient is its plain sum, and the check is relative to the
    # reference's own magnitude — 67 zero-mean draws can cancel to a sum whose float32 rounding alone exceeds the bracket)
    G = torch.randn(M, 1) + 0.5
    seed_value = 977 + M
    if not training:
        p = 0.0
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
    assert int(_mlp._seed_word(torch.device(DEV, 0))) == seed_value + (1 if p > 0 else 0)


def test_exact_cover_is_bit_reproducible_in_deterministic_mode(monkeypatch):
    """The group's four k-class sums are added in a fixed order: two runs of the two-layer ragged step agree bit for bit."""
    from recsys_benchmark_amd import _kernels

    monkeypatch.setattr(_kernels, "DETERMINISTIC", True)
    torch.manual_seed(11)
    M, K, hidden, p = 200, 48, [200, 104], 0.5
    seq = _seq(K, hidden, p).train().to(DEV)
    x = torch.randn(M, K, device=DEV)
    add = torch.randn(M, device=DEV)
    dev = torch.device(DEV, 0)
    state0 = copy.deepcopy(seq.state_dict())

    def step():
        seq.load_state_dict(state0)
        seq.zero_grad(set_to_none=True)
        _mlp._seed_word(dev).fill_(31)
        xd = x.clone().requires_grad_(True)
        out = run_tail(seq, xd, last_add=add)
        out.square().mean().backward()
        return [out.detach().clone(), xd.grad.clone()] + [q.grad.clone() for q in seq.parameters()]

    a, b = step(), step()
    assert float(a[1].abs().max()) > 0
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("dims,D", [([11, 7, 5], 16), ([11, 7, 5, 13, 3, 9, 4, 6, 8, 2, 5, 7, 3, 10, 12, 4, 6], 8)])
def test_deepfm_step_with_the_fm_epilogue_on_the_exact_cover(dims, D, monkeypatch):
    """One DeepFM step, hidden [200, 104], with the lookup backward in the first input-gradient product's epilogue: F = 3,
    D = 16 (48 columns: full sub-tiles, reduction 200 with a dead half) and F = 17, D = 8 (136 columns = 2 tiles of 68: cover
    (4, 1), the FM epilogue reads tiles whose columns beyond 68 were never written) against the oracle and against the
    two-node path on the same inputs."""
    from recsys_benchmark_amd import tail as _tail_mod

    B, hidden = 200, [200, 104]
    torch.manual_seed(B + D)
    base = pkg.DeepFM(dims, D, hidden, p_dropout=0.0, use_batchnorm=True, embedding_config={"name": "vanilla", "sparse": True},
                      fc_sparse=True)
    with torch.no_grad():
        base._bias.fill_(0.3)
        for m in base._deep_branch:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    gen = torch.Generator().manual_seed(B * 7 + D)
    x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1)
    y = (torch.rand(B, generator=gen) < 0.3).float()
    p = {k: v.detach().clone() for k, v in base.state_dict().items()}
    for k, v in p.items():
        if v.is_floating_point() and "running_" not in k:
            v.requires_grad_(True)
    ref = ro.deepfm_forward(x, p, len(hidden), True, True)
    torch.nn.BCEWithLogitsLoss()(ref, y).backward()
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(_tail_mod, "FM_EPILOGUE", fused)
        m = copy.deepcopy(base).to(DEV).train()
        logits = m(x.to(DEV))
        assert (type(logits.grad_fn.next_functions[0][0]).__name__ == "DeepFMFusedFnBackward") == fused
        torch.nn.BCEWithLogitsLoss()(logits, y.to(DEV)).backward()
        _lib.check_index_errors()
        grads = {k: (v.grad.to_dense() if v.grad.is_sparse else v.grad).cpu() for k, v in m.named_parameters() if v.grad is not None}
        got[fused] = (logits.detach().cpu(), grads)
    atol = 1e-5 + 2e-7 * B
    for fused in (True, False):
        logits, grads = got[fused]
        assert_close(logits, ref.detach(), 1e-4, 1e-5, f"logits fused={fused}")
        for k, gr in grads.items():
            if k.startswith("linear_layer") or (k.endswith(".bias") and k.startswith("_deep_branch") and p[k].grad.abs().max() < 1e-6):
                continue
            assert_close(gr, p[k].grad, 2e-4, atol, f"grad {k} fused={fused}")
    assert_close(got[True][0], got[False][0], 1e-5, 5e-6, "logits: fused epilogue vs two-node path")
    for k in ("embedding._emb_module.weight", "fc.weight", "_bias"):
        assert_close(got[True][1][k], got[False][1][k], 1e-5, atol, f"{k}: fused epilogue vs two-node path")

"""Test-side restatement of the fused MLP tail's dropout mask (recsys-benchmark_amd/csrc/tail_gemm.hpp: `Drop`), so that
the oracle can be given the very mask the kernels recompute: 16 bits of splitmix64(seed + salt', (m*ld + c) / 4) per
feature, keep when >= round(p * 65536).  Integer arithmetic only (torch int64 wraps like uint64).

Below it, the harness for stacks whose hidden layers differ (build_tail, reference_walk, bracket_failures)."""
import copy
import os

import torch
from torch import nn

_MASK64 = (1 << 64) - 1


def _s64(x: int) -> int:
    x &= _MASK64
    return x - (1 << 64) if x >= (1 << 63) else x


def _lsr(z: torch.Tensor, s: int) -> torch.Tensor:
    return (z >> s) & ((1 << (64 - s)) - 1)


def tail_keep_scale(seed: int, salt: int, M: int, ld: int, p: float, device="cpu") -> torch.Tensor:
    """[M, ld] multipliers (0 or 1/(1-p)) of the activation whose row pitch is `ld` (ld % 4 == 0)."""
    if p <= 0.0:
        return torch.ones(M, ld, device=device)
    assert ld % 4 == 0
    sd = _s64(seed + 0xD1B54A32D192ED03 * salt)
    idx = torch.arange(M * ld // 4, dtype=torch.int64, device=device)
    z = sd + _s64(0x9E3779B97F4A7C15) * (idx + 1)
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    h = z ^ _lsr(z, 31)
    thr = int(p * 65536.0 + 0.5)
    parts = [(_lsr(h, 16 * j) & 0xFFFF) if j else (h & 0xFFFF) for j in range(4)]
    u = torch.stack(parts, 1).reshape(M, ld)
    return (u >= thr).float() / (1.0 - p)


# ---------------------------------------------------------------------------------------------------------------------
# Per-layer specs: a stack whose hidden layers differ in how they normalise and drop (a frozen BatchNorm under
# model.train(), a Dropout left in eval, layers without either module, bias=False), the float64 / float32 evaluation of
# the reference's op sequence over it with the very masks the kernels use, and the bracket every tail test holds the
# fused result to.  Everything is keyed by HIDDEN-LAYER index, as the kernels are (salt = SALT * (index + 1)): a layer
# without a Dropout module owns a mask of ones, it does not shift the other layers' masks.
# |float64 pre-activation| below which a float32 evaluation may land on either side of the ReLU kink (tests/test_tail_gpu.py)
KINK = 1e-6
K_BRACKET = 8.0
FLOOR = 1e-6


def build_tail(K, layers, head_bias=True, momentum=None, eps=None):
    """nn.Sequential of (Linear, [BatchNorm1d], ReLU, [Dropout]) per entry of `layers` + Linear(., 1).
    layers: (width, bn, drop[, bias]) with bn in {"train", "eval", None (no module)}, drop in {p (a training-mode Dropout(p)),
    "eval" (a Dropout(0.5) in eval mode), None (no module)}, bias (default True) the Linear's.  Every module carries its OWN
    .training flag; BatchNorm is initialised like test_tail_gpu._seq (momentum / eps: non-default hyper-parameters)."""
    mods, flags, inp = [], [], K
    kw = {k: v for k, v in (("momentum", momentum), ("eps", eps)) if v is not None}
    for spec in layers:
        width, bn, drop = spec[:3]
        bias = spec[3] if len(spec) > 3 else True
        mods.append(nn.Linear(inp, width, bias=bias))
        flags.append(True)
        if bn is not None:
            assert bn in ("train", "eval")
            mods.append(nn.BatchNorm1d(width, **kw))
            flags.append(bn == "train")
        mods.append(nn.ReLU())
        flags.append(True)
        if drop is not None:
            mods.append(nn.Dropout(0.5 if drop == "eval" else float(drop)))
            flags.append(drop != "eval")
        inp = width
    mods.append(nn.Linear(inp, 1, bias=head_bias))
    flags.append(True)
    seq = nn.Sequential(*mods).train()
    for m, f in zip(seq, flags):
        m.train(f)
        if isinstance(m, nn.BatchNorm1d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.3)
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 1.5)
    return seq


def hidden_layers(seq):
    """([(index of the Linear in seq, Linear, BatchNorm1d or None, Dropout or None)] per hidden layer, head Linear)."""
    mods, out, i = list(seq), [], 0
    while i < len(mods) - 1:
        at, lin = i, mods[i]
        assert isinstance(lin, nn.Linear), f"module {i}: a hidden layer starts with a Linear"
        i += 1
        bn = mods[i] if isinstance(mods[i], nn.BatchNorm1d) else None
        i += bn is not None
        assert isinstance(mods[i], nn.ReLU), f"module {i}: ReLU expected"
        i += 1
        dp = mods[i] if (i < len(mods) - 1 and isinstance(mods[i], nn.Dropout)) else None
        i += dp is not None
        out.append((at, lin, bn, dp))
    assert isinstance(mods[-1], nn.Linear) and mods[-1].out_features == 1
    return out, mods[-1]


def active_ps(seq):
    """Per hidden layer: the rate of its Dropout when that module exists and is in training mode, else 0."""
    return [float(dp.p) if (dp is not None and dp.training) else 0.0 for _, _, _, dp in hidden_layers(seq)[0]]


def tail_masks(seq, seed: int, M: int, salt=None):
    """masks[i] = tail_keep_scale(seed, SALT * (i + 1), M, width_i, p_i) by hidden-layer index; ones where the layer's
    dropout is off or absent."""
    if salt is None:
        from recsys_benchmark_amd.tail import SALT as salt
    return [tail_keep_scale(seed, salt * (i + 1), M, lin.out_features, p)
            for i, ((_, lin, _, _), p) in enumerate(zip(hidden_layers(seq)[0], active_ps(seq)))]


def reference_walk(seq, x, add, masks, dtype, flips=None, near_out=None, as_is=False, keep=None):
    """The reference op sequence over a deep copy of `seq` in `dtype`, every module in its own mode, layer i's activation
    multiplied by masks[i]; returns (modules, x, add, out).  The float64 pass lists the (at most 4) pre-activations within
    KINK of the ReLU kink in `near_out` as (|value|, layer, flat position); `flips` = {"list": that list, "which": positions
    in it} evaluates with those ReLU decisions inverted (test_tail_gpu._reference's rule).  as_is: x / add are used as they
    come (tensors of `dtype` inside a larger graph).  keep (a list): receives per layer (Linear output, ReLU input), both
    with retain_grad."""
    seq = copy.deepcopy(seq).to(dtype)
    seq.zero_grad(set_to_none=True)
    if not as_is:
        x = x.detach().clone().to(dtype).requires_grad_(True)
        add = add.detach().clone().to(dtype).requires_grad_(True)
    layers, head = hidden_layers(seq)
    h, cands, n_near = x, [], 0
    for i, (_, lin, bn, _) in enumerate(layers):
        z = lin(h)
        pre = bn(z) if bn is not None else z
        if keep is not None and z.requires_grad:
            z.retain_grad()
            pre.retain_grad()
            keep.append((z, pre))
        on = pre.detach() > 0
        if near_out is not None:
            a = pre.detach().abs().flatten()
            n_near += int((a < KINK).sum())
            vals, pos = torch.topk(a, min(4, a.numel()), largest=False)
            cands += [(float(v), i, int(q)) for v, q in zip(vals, pos) if float(v) < KINK]
        if flips:
            for j, (_, lay, q) in enumerate(flips["list"]):
                if lay == i and j in flips["which"]:
                    on.view(-1)[q] = ~on.view(-1)[q]
        h = pre * on.to(dtype) * masks[i].to(dtype)
    if near_out is not None:
        assert n_near <= 4, f"{n_near} pre-activations within {KINK:g} of the kink: give this case's inputs another seed"
        near_out.extend(sorted(cands)[:4])
    out = head(h) + add.reshape(-1, 1)
    return seq, x, add, out


def zero_bias_names(seq):
    """Names of the Linear biases whose gradient is analytically zero: directly in front of a BatchNorm1d that is itself in
    training mode (the batch mean is removed).  A bias in front of a frozen BatchNorm or of none has a real gradient."""
    return {f"{at}.bias" for at, lin, bn, _ in hidden_layers(seq)[0] if lin.bias is not None and bn is not None and bn.training}


def bracket_failures(seq, fused, ref64, ref32, tag="", grads=True, ratios=None):
    """|got - r64| <= K_BRACKET * max(|r32 - r64|, FLOOR), relative to max |r64|, for the output, dx, dadd, every parameter
    gradient and every buffer (test_tail_exact_cover_gpu._bracket_failures' rule and factor).  fused = (modules, x, add, out)
    of the fused run, ref64 / ref32 = reference_walk's results after their backward.  A gradient the reference has and the
    fused run was told not to compute (requires_grad False there) must be None.  grads=False: output and buffers only.
    MI_TEST_REPORT=1 prints every fused / stock ratio; `ratios` (a list) receives (name, fused error, stock error)."""
    fs, fx, fa, fout = fused
    zero = zero_bias_names(seq)
    bad = []

    def check(name, got, r64, r32):
        got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
        scale = r64.abs().max().clamp_min(1e-30)
        err_f = float((got - r64).abs().max() / scale)
        err_s = float((r32 - r64).abs().max() / scale)
        if ratios is not None:
            ratios.append((name, err_f, err_s))
        if os.environ.get("MI_TEST_REPORT"):
            print(f"RATIO {tag} {name}: fused {err_f:.3e} stock {err_s:.3e} ratio {err_f / max(err_s, 1e-30):.2f}")
        if not err_f <= max(K_BRACKET * err_s, FLOOR):
            bad.append(f"{name}: fused {err_f:.3e} vs stock {err_s:.3e} (relative to max |ref|)")

    check("out", fout, ref64[3], ref32[3])
    if grads:
        for name, t, r64, r32 in (("dx", fx, ref64[1], ref32[1]), ("dadd", fa, ref64[2], ref32[2])):
            if t is None or not t.requires_grad:
                assert t is None or t.grad is None, f"{name}: a gradient nobody asked for"
            else:
                check(name, t.grad, r64.grad, r32.grad)
        p64, p32, pf = dict(ref64[0].named_parameters()), dict(ref32[0].named_parameters()), dict(fs.named_parameters())
        assert set(pf) == set(p64)
        for name in p64:
            if not pf[name].requires_grad:
                assert pf[name].grad is None, f"{name}: frozen, yet it got a gradient"
            elif name in zero:
                assert pf[name].grad is not None and float(pf[name].grad.abs().max()) == 0.0, name
            else:
                assert pf[name].grad is not None, f"{name}: no gradient"
                check(name, pf[name].grad, p64[name].grad, p32[name].grad)
    b64, b32, bf = dict(ref64[0].named_buffers()), dict(ref32[0].named_buffers()), dict(fs.named_buffers())
    for name in b64:
        if name.endswith("num_batches_tracked"):
            assert int(bf[name]) == int(b64[name]), name
        else:
            check(name, bf[name], b64[name], b32[name])
    return bad


def bracket_or_flip(seq, fused, x, add, G, masks, near, ref64, ref32, tag="", grads=True, ratios=None):
    """bracket_failures against ref64; when that fails and the float64 pass listed pre-activations on the kink, against the
    float64 evaluation under every assignment of their ReLU decisions: ONE has to match.  Returns the failures left."""
    bad = bracket_failures(seq, fused, ref64, ref32, tag, grads, ratios)
    if bad and near:
        for bits in range(1, 1 << len(near)):
            alt = reference_walk(seq, x, add, masks, torch.float64,
                                 flips={"list": near, "which": {j for j in range(len(near)) if bits >> j & 1}})
            if grads:
                (alt[3] * G.double()).sum().backward()
            if not bracket_failures(seq, fused, alt, ref32, tag + " (flipped)", grads):
                return []
    return bad

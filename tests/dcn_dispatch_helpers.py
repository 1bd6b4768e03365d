"""What tests/test_dcn_dispatch_gpu.py (GPU) and tests/test_dcn_dispatch_host.py (CPU) share: the CrossNet-head and whole-model
cases that leave the fast path of layer_dcn.py, their seeded operands, the oracle evaluated in float64 (the reference) and in
float32 (the yardstick of the tolerance), and the tolerance contract.

Tolerances are not new ones.  Heads: the file-level contract of tests/test_dcn_gpu.py, activations rtol 2e-5 / atol 2e-6,
gradients rtol 2e-4 / atol 2e-5, atol scaled by max(1, max|ref|).  Models: those of test_dcn_models_match_reference_golden,
logits 1e-4 / 1e-5, gradients 5e-4 / 2e-5.  The host test asserts that the stock float32 CPU evaluation of every case already
lies inside them, so a GPU failure is the kernels' and not the tolerance's."""
import functools

import torch

from oracle import reference_ops as ro

ACT_TOL = (2e-5, 2e-6)
GRAD_TOL = (2e-4, 2e-5)
LOGIT_TOL = (1e-4, 1e-5)
MODEL_GRAD_TOL = (5e-4, 2e-5)
KINK = 1e-4          # every ReLU pre-activation of a model case is further than this from 0 in float64

# ---- heads -----------------------------------------------------------------------------------------------------------------
# (M, d, L) / (M, d, E, r, L): each named for the branch of layer_dcn.py it forces
DCN_HEAD_CASES = {
    "d22-three-pass": (33, 22, 2),
    "d15-three-pass": (7, 15, 3),
    "d1028-three-pass-panel": (5, 1028, 1),
    "d1030-three-pass-general": (5, 1030, 1),
    "d24-panel-off": (40, 24, 2),
}
MIX_HEAD_CASES = {
    "d22-r16-no-fused-expert": (50, 22, 3, 16, 2),
    "E9-gate-by-gemm": (20, 40, 9, 8, 2),
    "d18-r48": (9, 18, 2, 48, 1),
    "d16-r5": (9, 16, 2, 5, 2),
    "L0": (12, 24, 4, 16, 0),
    "r16-panel-off": (30, 40, 3, 16, 3),
    "d40-r16-deterministic": (30, 40, 3, 16, 3),
    "d22-r8-deterministic": (30, 22, 3, 8, 3),
}
# d % 4 == 0: the operand LAYOUT decides the branch (tests of x0 / the upstream gradient as views)
VIEW_DCN = (33, 24, 2)
VIEW_MIX = (30, 40, 3, 16, 2)


def head_problem(dims):
    """(head on the CPU, X, G) of a case: len(dims) == 3 a DCNHead, 5 a DCN_MixHead.  Input scaling as in
    test_dcn_mixhead_vs_oracle (three layers stay O(1)), non-zero biases for the mix head."""
    from recsys_benchmark_amd.layer_dcn import DCN_MixHead, DCNHead

    gen = torch.Generator().manual_seed(977 + sum(dims))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(31 + sum(dims))
        if len(dims) == 3:
            M, d, L = dims
            head = DCNHead(L, d)
        else:
            M, d, E, r, L = dims
            head = DCN_MixHead(E, L, r, d)
            with torch.no_grad():
                for b in head.biases:
                    b.copy_(torch.randn(b.shape, generator=gen) * 0.1)
    X = torch.randn(M, d, generator=gen) * (0.05 if d > 100 else 0.3)
    G = torch.randn(M, d, generator=gen)
    return head, X, G


def head_eval(dims, dtype, G=None):
    """The oracle's head on the case's parameters in `dtype`: {"out", "dx", "g/<parameter>"} (a parameter the output does not
    depend on — every one of a head without layers — has no entry).  G: another upstream gradient than the case's."""
    head, X, G0 = head_problem(dims)
    G = G0 if G is None else G
    L = dims[-1]
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in head.state_dict().items()}
    x = X.to(dtype).requires_grad_(True)
    out = (ro.dcn_head if len(dims) == 3 else ro.dcn_mix_head)(x, p, L)
    (out * G.to(dtype)).sum().backward()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"g/" + k: v.grad for k, v in p.items() if v.grad is not None})
    return res


@functools.lru_cache(maxsize=None)
def head_reference(dims):
    """float64, computed once per case and shared (read-only) by the tests that need it"""
    return head_eval(dims, torch.float64)


@functools.lru_cache(maxsize=None)
def head_reference_ones(dims):
    """float64 with an upstream gradient of ones (what `.sum().backward()` hands the head)"""
    head, X, _ = head_problem(dims)
    return head_eval(dims, torch.float64, G=torch.ones_like(X))


def tol_ratio(actual, ref64, rtol, atol):
    """max |actual - ref| / (atol * max(1, max|ref|) + rtol * |ref|): <= 1 is inside the head contract"""
    a, r = actual.detach().double().cpu(), ref64.detach().double().cpu()
    assert tuple(a.shape) == tuple(r.shape), (tuple(a.shape), tuple(r.shape))
    if r.numel() == 0:
        return 0.0
    bound = atol * max(1.0, float(r.abs().max())) + rtol * r.abs()
    return float(((a - r).abs() / bound).max())


def head_worst(result, ref):
    """(key, ratio) of the tensor of `result` furthest out relative to the head contract; the keys must be the reference's"""
    assert set(result) == set(ref), f"returned {sorted(result)} vs reference {sorted(ref)}"
    worst = ("", 0.0)
    for k, want in ref.items():
        rtol, atol = ACT_TOL if k == "out" else GRAD_TOL
        q = tol_ratio(result[k], want, rtol, atol)
        if not q <= worst[1]:
            worst = (k, q)
    return worst


# ---- whole models at an embedding width that is no multiple of 4 -----------------------------------------------------------
FIELD_DIMS, BATCH = [11, 7, 5], 37
# name -> (config, cross layers, hidden layers, structure or None for DCN_Mix, seed)
MODEL_CASES = {
    "dcn_mix-nf5": ({"name": "dcn_mix", "num_factor": 5, "hidden_sizes": [8, 8], "num_layers": 2, "num_experts": 3, "rank": 5,
                     "p_dropout": 0.0, "compile_model": False}, 2, 2, None, 11),
    "dcn_mix-nf6": ({"name": "dcn_mix", "num_factor": 6, "hidden_sizes": [8], "num_layers": 3, "num_experts": 4, "rank": 16,
                     "p_dropout": 0.0, "compile_model": False}, 3, 1, None, 12),
    "dcnv2-stacked-nf5": ({"name": "dcn", "num_factor": 5, "hidden_sizes": [8, 8], "num_layers": 2, "p_dropout": 0.0,
                           "structure": "Stacked"}, 2, 2, "Stacked", 13),
    "dcnv2-parallel-nf5": ({"name": "dcn", "num_factor": 5, "hidden_sizes": [8], "num_layers": 3, "p_dropout": 0.0,
                            "structure": "Parallel"}, 3, 1, "Parallel", 14),
}


def model_problem(name):
    """(model on the CPU, x int64[B, F], y float32[B]); BatchNorm affine parameters and running statistics off their
    defaults, so that train and eval mode are different functions"""
    import recsys_benchmark_amd as pkg

    cfg, _, _, _, seed = MODEL_CASES[name]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = pkg.get_ctr_model(FIELD_DIMS, {k: (list(v) if isinstance(v, list) else v) for k, v in cfg.items()})
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0, 0.3)
                    m.running_mean.normal_(0, 0.3)
                    m.running_var.uniform_(0.5, 1.5)
            for b in getattr(model.cross_head, "biases", []):
                b.normal_(0, 0.1)
    gen = torch.Generator().manual_seed(seed + 100)
    x = torch.stack([torch.randint(0, d, (BATCH,), generator=gen) for d in FIELD_DIMS], 1)
    y = (torch.rand(BATCH, generator=gen) < 0.4).float()
    return model, x, y


def model_eval(name, training, dtype):
    """The oracle's forward on the model's own state in `dtype`, BCE-with-logits and autograd:
    {"logits", "loss", "pre" (list of ReLU pre-activations), "g/<parameter>"}."""
    _, nl, nh, structure, _ = MODEL_CASES[name]
    model, x, y = model_problem(name)
    params = {k for k, _ in model.named_parameters()}
    p = {}
    for k, v in model.state_dict().items():
        v = v.detach().clone()
        p[k] = v.to(dtype).requires_grad_(k in params) if v.is_floating_point() else v
    emb = p["embedding._emb_module.weight"][x + p["offsets"]]
    pre = []
    if structure is None:
        logits = ro.dcn_mix_forward(x, p, emb, nl, nh, training, pre_out=pre)
    else:
        logits = ro.dcnv2_forward(x, p, emb, nl, nh, training, structure)
        with torch.no_grad():          # the same MLP once more for its pre-activations (dcnv2_forward has no hook of its own)
            e = emb.reshape(x.shape[0], -1)
            ro.bn_mlp(ro.dcn_head(e, p, nl, "cross_head.layers") if structure == "Stacked" else e, p, "_dnn", nh, training,
                      pre_out=pre)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y.to(dtype))
    loss.backward()
    res = {"logits": logits.detach(), "loss": loss.detach(), "pre": [z for z, _ in pre]}
    res.update({"g/" + k: p[k].grad for k in params if p[k].grad is not None})
    return res


@functools.lru_cache(maxsize=None)
def model_reference(name, training):
    return model_eval(name, training, torch.float64)


def plain_ratio(actual, ref64, rtol, atol):
    """max |actual - ref| / (atol + rtol * |ref|), the plain assert_close rule of the model tolerances"""
    a, r = actual.detach().double().cpu(), ref64.detach().double().cpu()
    a = a.to_dense() if a.is_sparse else a
    assert tuple(a.shape) == tuple(r.shape), (tuple(a.shape), tuple(r.shape))
    return float(((a - r).abs() / (atol + rtol * r.abs())).max()) if r.numel() else 0.0


def model_worst(result, ref):
    """(key, ratio) furthest out relative to the model tolerances over the logits and every parameter gradient"""
    keys = {k for k in ref if k == "logits" or k.startswith("g/")}
    assert {k for k in result if k in keys or k.startswith("g/")} == keys, (sorted(result), sorted(keys))
    worst = ("", 0.0)
    for k in sorted(keys):
        rtol, atol = LOGIT_TOL if k == "logits" else MODEL_GRAD_TOL
        q = plain_ratio(result[k], ref[k], rtol, atol)
        if not q <= worst[1]:
            worst = (k, q)
    return worst

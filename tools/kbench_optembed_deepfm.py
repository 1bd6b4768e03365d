"""DeepFM OptEmbed search / retraining on the masked fused lookup, at the Criteo-26 shape (B = 4096, F = 26, D = 16,
N = 33 762 577) and at D = 64 with the same fields cut to an eighth of their rows (a 1.1 GB table).  Writes one JSON object.

  (a) the lookup + FM part of one candidate's eval forward, through DeepFM._fm_and_embedding:
        masked_field    set_candidate in field mode   (mi_gather_fm_masked_fwd, keep = alive rows, fwidth per candidate)
        masked_feature  set_candidate in feature mode (keep = alive * width)
        parent_path     no candidate installed: OptEmbed._lookup (mi_optembed_fwd and its index launches) + fm_first_order
        unmasked_floor  gather_fm on the same table without masks
  (b) one candidate end to end: set_candidate + a validation pass of 64 batches through one GraphedForward, against the
      same pass on the parent's path (host clock around work that ends in a synchronise).
  (c) the retraining lookup's forward + backward, dense and row form: the masked op against the composed
      gather_fm(x, offsets, W * mask, ...) through autograd — the whole-table product the reference forms every step.

Every figure is the MEDIAN over --rounds rounds (default 7) of the time per call, device events around back-to-back calls
over a cycle of 16 different batches of uniform ids; the variants alternate inside a round, and `spread_us` is max - min
over the rounds.  Per-call times include the Python and launch cost of the call.  The two conditions at the end compare
gaps with the larger of the two spreads.

    python tools/kbench_optembed_deepfm.py --out profiles/optembed_deepfm_kbench.json

Kernel times (profiles/optembed_deepfm_kernel_stats.csv) come from a run of leg (a) alone under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_optembed_deepfm.py --legs a`.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from bench import CRITEO_KAGGLE_26  # noqa: E402
from recsys_benchmark_amd import _kernels, _lib, trainer  # noqa: E402

DEV = "cuda:0"
B, NBATCH = 4096, 16


def per_call_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def rounds_of(variants, n, rounds):
    """{name: {"median_us", "spread_us", "rounds_us"}}; every round times each variant once, in turn."""
    for fn in variants.values():          # warm-up: code objects, allocator
        per_call_us(fn, min(n, 8))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(per_call_us(fn, n))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                "rounds_us": [round(t, 2) for t in v]} for k, v in times.items()}


def condition(res, fast, slow):
    gap = res[slow]["median_us"] - res[fast]["median_us"]
    spread = max(res[slow]["spread_us"], res[fast]["spread_us"])
    return {"fast": fast, "slow": slow, "gap_us": round(gap, 2), "larger_spread_us": spread, "holds": bool(gap > spread)}


def supernet(dims, D, mode_d, hidden):
    """A DeepFM on the OptEmbed supernet with uniform(-0.5, 0.5) weights and per-field thresholds at the mean L1 row norm
    (D / 4): about half of the rows are dead."""
    torch.manual_seed(0)
    m = pkg.DeepFM(dims, D, hidden, p_dropout=0.0,
                   embedding_config={"name": "deepfm_optembed", "mode_threshold_d": mode_d}).to(DEV).eval()
    with torch.no_grad():
        m.embedding._weight.uniform_(-0.5, 0.5)
        m.embedding._mask_e_module._t_param.fill_(D / 4)
        m.fc.weight.normal_()
    return m


def batches(dims, n, gen):
    return [torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV) for _ in range(n)]


def leg_a(dims, D, rounds, out):
    gen = torch.Generator().manual_seed(1)
    xs = batches(dims, NBATCH, gen)
    res, alive_share = {}, None
    with torch.no_grad():
        for mode_d in ("field", "feature"):
            m = supernet(dims, D, mode_d, [16])
            emb = m.embedding
            size = len(dims) if mode_d == "field" else sum(dims)
            mask_d = torch.randint(0, D, (size,), generator=gen).to(DEV)
            emb.set_candidate(mask_d)
            alive_share = float(emb._alive_rows().float().mean())
            masked = m._fm_and_embedding(xs[0])
            emb.clear_candidate()
            emb._eval_mask_d = mask_d                 # what get_weight(mask_d) leaves for the eval lookups of the parent's path
            parent = m._fm_and_embedding(xs[0])
            torch.testing.assert_close(masked[0], parent[0], rtol=0, atol=0)
            torch.testing.assert_close(masked[1], parent[1], rtol=2e-5, atol=2e-5)
            W, w1 = emb._weight, m.fc.weight

            def run_masked(i, m=m, emb=emb):
                emb._candidate = True
                m._fm_and_embedding(xs[i % NBATCH])

            def run_parent(i, m=m, emb=emb):
                emb._candidate = False
                m._fm_and_embedding(xs[i % NBATCH])

            variants = {f"masked_{mode_d}": run_masked, f"parent_path_{mode_d}": run_parent}
            if mode_d == "field":
                variants["unmasked_floor"] = lambda i, m=m, W=W, w1=w1: _kernels.gather_fm(xs[i % NBATCH], m.offsets, W, w1, m._bias)
            res.update(rounds_of(variants, 50, rounds))
            del m, emb, W, w1
            torch.cuda.empty_cache()
    _lib.check_index_errors()
    out["a_lookup_fm"] = dict(res, alive_row_share=round(alive_share, 4), calls_per_round=50)
    out["a_lookup_fm"]["condition_masked_field_faster_than_parent"] = condition(res, "masked_field", "parent_path_field")


def leg_b(dims, D, rounds, out):
    gen = torch.Generator().manual_seed(2)
    m = supernet(dims, D, "field", [400, 400, 400])
    emb = m.embedding
    loader = [(x, (torch.rand(B, generator=gen) < 0.3).float().to(DEV)) for x in batches(dims, 64, gen)]
    cands = [torch.randint(0, D, (len(dims),), generator=gen).to(DEV) for _ in range(rounds + 1)]
    forward = trainer.GraphedForward(m)
    times = {"masked_candidate_ms": [], "parent_candidate_ms": []}

    def masked(c):
        emb.set_candidate(c)
        return trainer.validate_epoch(loader, m, device=DEV, forward=forward)["auc"]

    parent_forward = trainer.GraphedForward(m)

    def parent(c):
        emb.clear_candidate()
        emb._eval_mask_d = c
        return trainer.validate_epoch(loader, m, device=DEV, forward=parent_forward)["auc"]

    auc = (masked(cands[0]), parent(cands[0]))          # warm-up: both graphs captured, the row mask cached
    for c in cands[1:]:
        for key, fn in (("masked_candidate_ms", masked), ("parent_candidate_ms", parent)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(c)
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3)
    out["b_candidate_end_to_end"] = {
        k: {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "rounds_ms": [round(t, 3) for t in v]}
        for k, v in times.items()}
    out["b_candidate_end_to_end"].update(validation_batches=64, hidden=[400, 400, 400], graphs_replayed=bool(forward.use_graph),
                                         warmup_auc_masked_vs_parent=[auc[0], auc[1]])
    del m, emb, loader
    torch.cuda.empty_cache()


def leg_c(dims, D, rounds, out):
    gen = torch.Generator().manual_seed(3)
    N, F = sum(dims), len(dims)
    xs = batches(dims, NBATCH, gen)
    offsets = torch.tensor([0] + dims[:-1]).cumsum(0).to(DEV)
    W = (torch.rand(N, D, device=DEV) - 0.5).requires_grad_(True)
    w1 = torch.randn(N, 1, device=DEV, requires_grad=True)
    bias = torch.zeros(1, device=DEV, requires_grad=True)
    # 80 % sparsity as in the reference's configs: half of the rows dead, the live ones keep 40 % of D on average
    keep = ((torch.rand(N, device=DEV) < 0.5) * torch.randint(1, max(2, int(0.8 * D)), (N,), device=DEV)).to(torch.uint8)
    mask = (torch.arange(D, device=DEV).unsqueeze(0) < keep.unsqueeze(1)).float()
    G, gy = torch.randn(B, F, D, device=DEV), torch.randn(B, device=DEV)
    res = {"kept_share": round(float(mask.mean()), 4)}

    def step(sparse, masked):
        def run(i):
            W.grad = w1.grad = bias.grad = None
            if masked:
                emb, y = _kernels.gather_fm(xs[i % NBATCH], offsets, W, w1, bias, sparse_W=sparse, sparse_w1=sparse, keep=keep)
            else:
                emb, y = _kernels.gather_fm(xs[i % NBATCH], offsets, W * mask, w1, bias, sparse_W=sparse, sparse_w1=sparse)
            torch.autograd.backward([emb, y], [G, gy])
        return run

    for form, sparse in (("dense", False), ("rows", True)):
        variants = {f"masked_{form}": step(sparse, True), f"composed_{form}": step(sparse, False)}
        try:
            variants[f"composed_{form}"](0)
        except Exception as exc:      # (stock autograd may not take a row-form gradient through the product)
            res[f"composed_{form}"] = f"not runnable: {type(exc).__name__}: {str(exc)[:120]}"
            del variants[f"composed_{form}"]
        r = rounds_of(variants, 5 if form == "dense" else 10, rounds)
        res.update(r)
        if f"composed_{form}" in r:
            res[f"condition_masked_{form}_faster_than_composed"] = condition(r, f"masked_{form}", f"composed_{form}")
    W.grad = w1.grad = None
    _lib.check_index_errors()
    out["c_retrain_fwd_bwd"] = res
    del W, w1, mask, keep
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tables cut by 4096: a rehearsal of the tool, not a measurement")
    ap.add_argument("--legs", default="abc", help="which of the legs a, b, c to run (a kernel-trace run wants 'a' alone)")
    a = ap.parse_args()
    assert a.rounds >= 5, "medians of at least five rounds"
    assert torch.cuda.is_available(), "kbench_optembed_deepfm needs an MI355X"
    cut = 4096 if a.small else 1
    shapes = {"criteo26_D16": ([max(1, d // cut) for d in CRITEO_KAGGLE_26], 16),
              "criteo26_eighth_D64": ([max(1, d // (8 * cut)) for d in CRITEO_KAGGLE_26], 64)}
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds, "rehearsal": bool(a.small), "shapes": {}}
    for name, (dims, D) in shapes.items():
        out = {"fields": len(dims), "D": D, "rows": sum(dims)}
        if "a" in a.legs:
            leg_a(dims, D, a.rounds, out)
        if "b" in a.legs and D == 16:
            leg_b(dims, D, a.rounds, out)
        if "c" in a.legs:
            leg_c(dims, D, a.rounds, out)
        result["shapes"][name] = out
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

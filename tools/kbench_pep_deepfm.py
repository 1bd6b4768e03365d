"""DeepFM PEP search / retraining on the fused lookup, at the Criteo-26 shape (B = 4096, F = 26, D = 16, N = 33 762 577)
and at D = 64 with the same fields cut to an eighth of their rows (4 220 315 rows).  Writes one JSON object.

Every leg times the fused call against the path of the commit before it, for the feature_dim and the global threshold:
  (a) eval lookup + FM            gather_fm(soft=s)               vs  soft_threshold_gather(x + offsets) + fm_first_order
  (b) training forward + backward the same with dense gradients   vs  the same through XformGather's atomic backward
  (c) retraining forward + backward, dense and row form
                                  gather_fm(elem_mask=m)          vs  masked_gather / masked_gather_row_grad + fm_first_order
  (d) get_sparsity                soft_count_kept                 vs  count_nonzero(sign(W) relu(|W| - sigmoid(s)))

Every figure is the MEDIAN over --rounds rounds (default 7) of the time per call, device events around back-to-back calls
over a cycle of 16 different batches of uniform ids; the two paths alternate inside a round, and `spread_us` is max - min
over the rounds.  Per-call times include the Python and launch cost of the call.  `condition_*` compares the gap with the
PARENT path's spread.

    python tools/kbench_pep_deepfm.py --out profiles/pep_deepfm_kbench.json

Kernel times and launch counts (profiles/pep_deepfm_kernel_stats.csv) come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_pep_deepfm.py --legs t`: leg t
issues each fused call TRACE_CALLS times at the D = 16 shape and nothing else.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import CRITEO_KAGGLE_26  # noqa: E402
from recsys_benchmark_amd import _kernels, _lib  # noqa: E402
from recsys_benchmark_amd.embeddings.pep_embedding import _THRESHOLD_SHAPES, _soft  # noqa: E402

DEV = "cuda:0"
B, NBATCH, TRACE_CALLS = 4096, 16, 20
KINDS = ("feature_dim", "global")


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
        per_call_us(fn, min(n, 4))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(per_call_us(fn, n))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                "rounds_us": [round(t, 2) for t in v]} for k, v in times.items()}


def condition(res, fast, slow):
    gap = res[slow]["median_us"] - res[fast]["median_us"]
    return {"fused": fast, "parent": slow, "gap_us": round(gap, 2), "parent_spread_us": res[slow]["spread_us"],
            "ratio": round(res[slow]["median_us"] / res[fast]["median_us"], 2), "holds": bool(gap > res[slow]["spread_us"])}


class Operands:
    """One shape's tables: uniform(-0.5, 0.5) weights; thresholds at sigmoid(s) = 0.25 (about half of the elements pruned);
    a mask that keeps a fifth of the elements (the reference's 0.8 milestone)."""

    def __init__(self, dims, D):
        gen = torch.Generator().manual_seed(1)
        self.dims, self.D, self.N, self.F = dims, D, sum(dims), len(dims)
        self.xs = [torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV) for _ in range(NBATCH)]
        self.offsets = torch.tensor([0] + dims[:-1]).cumsum(0).to(DEV)
        self.W = (torch.rand(self.N, D, device=DEV) - 0.5).requires_grad_(True)
        self.w1 = torch.randn(self.N, 1, device=DEV, requires_grad=True)
        self.bias = torch.zeros(1, device=DEV, requires_grad=True)
        self.G, self.gy = torch.randn(B, self.F, D, device=DEV), torch.randn(B, device=DEV)

    def threshold(self, kind):
        return torch.full(_THRESHOLD_SHAPES[kind](self.N, self.D), -1.0986, device=DEV).requires_grad_(True)

    def mask(self):
        return torch.rand(self.N, self.D, device=DEV) < 0.2

    def clear(self, *more):
        for t in (self.W, self.w1, self.bias) + more:
            t.grad = None

    # ---- the fused call and the parent commit's path (DeepFM._fm_and_embedding's fall-through) ----
    def fused(self, i, sparse=False, **xform):
        return _kernels.gather_fm(self.xs[i % NBATCH], self.offsets, self.W, self.w1, self.bias, sparse_W=sparse, **xform)

    def parent(self, i, gather):
        rows = self.xs[i % NBATCH] + self.offsets
        _kernels.note_field_layout(rows, self.offsets, self.N)
        return _kernels.fm_first_order(gather(rows), rows, self.w1, self.bias)

    def step(self, call, *more):
        def run(i):
            self.clear(*more)
            emb, y = call(i)
            torch.autograd.backward([emb, y], [self.G, self.gy])
        return run


def leg_a(op, rounds, out):
    res = {}
    with torch.no_grad():
        for kind in KINDS:
            s = op.threshold(kind)
            f, p = op.fused(0, soft=s), op.parent(0, lambda r: _kernels.soft_threshold_gather(r, op.W, s))
            torch.testing.assert_close(f[0], p[0], rtol=0, atol=0)
            torch.testing.assert_close(f[1], p[1], rtol=2e-5, atol=2e-5)
            r = rounds_of({f"fused_{kind}": lambda i: op.fused(i, soft=s),
                           f"parent_{kind}": lambda i: op.parent(i, lambda r: _kernels.soft_threshold_gather(r, op.W, s))}, 50, rounds)
            res.update(r)
            res[f"condition_{kind}"] = condition(r, f"fused_{kind}", f"parent_{kind}")
            del s
        m = op.mask()
        r = rounds_of({"fused_elemmask": lambda i: op.fused(i, elem_mask=m),
                       "parent_elemmask": lambda i: op.parent(i, lambda r: _kernels.masked_gather(r, op.W, m))}, 50, rounds)
        res.update(r)
        res["condition_elemmask"] = condition(r, "fused_elemmask", "parent_elemmask")
    out["a_eval_lookup_fm"] = dict(res, calls_per_round=50)


def leg_b(op, rounds, out):
    res = {}
    for kind in KINDS:
        s = op.threshold(kind)
        r = rounds_of({f"fused_{kind}": op.step(lambda i: op.fused(i, soft=s), s),
                       f"parent_{kind}": op.step(lambda i: op.parent(i, lambda r: _kernels.soft_threshold_gather(r, op.W, s)), s)},
                      5, rounds)
        res.update(r)
        res[f"condition_{kind}"] = condition(r, f"fused_{kind}", f"parent_{kind}")
        op.clear(s)
        del s
        torch.cuda.empty_cache()
    out["b_train_fwd_bwd_dense"] = dict(res, calls_per_round=5)


def leg_c(op, rounds, out):
    m = op.mask()
    res = {"kept_share": round(float(m.float().mean()), 4)}
    for form, sparse, gather in (("dense", False, _kernels.masked_gather), ("rows", True, _kernels.masked_gather_row_grad)):
        r = rounds_of({f"fused_{form}": op.step(lambda i: op.fused(i, sparse=sparse, elem_mask=m)),
                       f"parent_{form}": op.step(lambda i: op.parent(i, lambda r: gather(r, op.W, m)))}, 5 if not sparse else 10, rounds)
        res.update(r)
        res[f"condition_{form}"] = condition(r, f"fused_{form}", f"parent_{form}")
        op.clear()
    out["c_retrain_fwd_bwd"] = res


def leg_d(op, rounds, out):
    res = {}
    with torch.no_grad():
        for kind in KINDS:
            s = op.threshold(kind)
            assert int(_kernels.soft_count_kept(op.W, s)) == int(torch.count_nonzero(_soft(op.W, s)))
            r = rounds_of({f"fused_{kind}": lambda i: _kernels.soft_count_kept(op.W, s),
                           f"parent_{kind}": lambda i: torch.count_nonzero(_soft(op.W, s))}, 3, rounds)
            res.update(r)
            res[f"condition_{kind}"] = condition(r, f"fused_{kind}", f"parent_{kind}")
            del s
            torch.cuda.empty_cache()
    out["d_get_sparsity"] = dict(res, calls_per_round=3)


def leg_t(op, out):
    """What a kernel trace should see: TRACE_CALLS of each fused call, nothing else of this library."""
    s_fd, s_g, m = op.threshold("feature_dim"), op.threshold("global"), op.mask()
    calls = {"eval_soft_feature_dim": lambda i: op.fused(i, soft=s_fd),
             "train_soft_feature_dim_dense": op.step(lambda i: op.fused(i, soft=s_fd), s_fd),
             "train_soft_global_dense": op.step(lambda i: op.fused(i, soft=s_g), s_g),
             "retrain_elemmask_dense": op.step(lambda i: op.fused(i, elem_mask=m)),
             "retrain_elemmask_rows": op.step(lambda i: op.fused(i, sparse=True, elem_mask=m)),
             "count_feature_dim": lambda i: _kernels.soft_count_kept(op.W.detach(), s_fd.detach())}
    for name, fn in calls.items():
        with torch.set_grad_enabled(not name.startswith(("eval", "count"))):
            for i in range(TRACE_CALLS):
                fn(i)
    torch.cuda.synchronize()
    out["t_trace"] = {"calls_each": TRACE_CALLS, "order": list(calls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tables cut by 4096: a rehearsal of the tool, not a measurement")
    ap.add_argument("--legs", default="abcd", help="which of the legs a, b, c, d to run; t: the calls of a kernel-trace run")
    a = ap.parse_args()
    assert a.rounds >= 7, "medians of at least seven rounds"
    assert torch.cuda.is_available(), "kbench_pep_deepfm needs an MI355X"
    cut = 4096 if a.small else 1
    shapes = {"criteo26_D16": ([max(1, d // cut) for d in CRITEO_KAGGLE_26], 16),
              "criteo26_eighth_D64": ([max(1, d // (8 * cut)) for d in CRITEO_KAGGLE_26], 64)}
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds, "rehearsal": bool(a.small), "shapes": {}}
    for name, (dims, D) in shapes.items():
        if "t" in a.legs and D != 16:
            continue
        op = Operands(dims, D)
        out = {"fields": len(dims), "D": D, "rows": sum(dims)}
        if "t" in a.legs:
            leg_t(op, out)
        if "a" in a.legs:
            leg_a(op, a.rounds, out)
        if "b" in a.legs:
            leg_b(op, a.rounds, out)
        if "c" in a.legs:
            leg_c(op, a.rounds, out)
        if "d" in a.legs and D == 16:
            leg_d(op, a.rounds, out)
        _lib.check_index_errors()
        result["shapes"][name] = out
        del op
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

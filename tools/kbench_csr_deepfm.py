"""DeepFM served from a CSR-pruned table (PrunedEmbedding, wide and compact indices) at the Criteo-26 shape (B = 4096,
F = 26): D = 16 at 33 762 577 rows and D = 64 at 4 220 315 rows (every field cut by 8), the table magnitude-pruned with
PrunedEmbedding.from_pruned at p = 0.5 / 0.8 / 0.95.  Writes one JSON object.

Every leg times the new call against the path of the commit before it and against the dense table, in the same run:
  (a) eval lookup + FM            gather_fm_csr on wide and on compact indices  vs  x + offsets, csr_rows, fm_first_order
                                  (the parent's three launches)  vs  gather_fm on the dense pruned table
  (r) PrunedEmbedding.forward     csr_rows_typed on the compact table  vs  csr_rows (mi_csr_rows_fwd) on the wide one
  (v) one validate_epoch          64 batches: the model served from CSR (compact, wide)  vs  the wide table behind a no-op
                                  forward hook (the parent's path: a hooked module keeps its own forward, so this is the
                                  torch add, mi_csr_rows_fwd and mi_fm_fwd)  vs  the compact table behind such a hook (three
                                  launches too, on the typed densify)  vs  the same model on the dense pruned table
  (m) torch.cuda.memory_allocated of the model in each form (dense, wide CSR, compact CSR)

Every figure is the MEDIAN over --rounds rounds (default 7) of the time per call, device events around back-to-back calls
over a cycle of 16 different batches of uniform ids; the paths alternate inside a round, and `spread_us` is max - min
over the rounds.  Per-call times include the Python and launch cost of the call.  `condition_*` compares a gap with the
other path's spread: a gap inside the spread is a tie.

    python tools/kbench_csr_deepfm.py --out profiles/csr_deepfm_kbench.json

Kernel times and launch counts (profiles/csr_deepfm_kernel_stats.csv) come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_csr_deepfm.py --legs t`: leg t
issues each call of leg (a) and (r) TRACE_CALLS times at p = 0.8 and nothing else.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from bench import CRITEO_KAGGLE_26  # noqa: E402
from recsys_benchmark_amd import _kernels, _lib, csr_fm, trainer  # noqa: E402
from recsys_benchmark_amd.embeddings import PrunedEmbedding, VanillaEmbedding  # noqa: E402

DEV = "cuda:0"
B, NBATCH, TRACE_CALLS = 4096, 16, 20
RATIOS = (0.5, 0.8, 0.95)
HIDDEN = [400, 400, 400]


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


def condition(res, new, other):
    """new against other: `faster` when the gap exceeds the other path's spread, `tie` when it lies inside it."""
    gap = res[other]["median_us"] - res[new]["median_us"]
    spread = max(res[other]["spread_us"], res[new]["spread_us"])
    return {"new": new, "other": other, "gap_us": round(gap, 2), "spread_us": spread,
            "ratio": round(res[other]["median_us"] / res[new]["median_us"], 2),
            "verdict": "faster" if gap > spread else ("slower" if gap < -spread else "tie")}


class Table:
    """One shape: a table of uniform(-0.1, 0.1) weights, the first-order table and 16 batches of uniform ids; per ratio the
    dense pruned table and its CSR in both widths."""

    def __init__(self, dims, D):
        gen = torch.Generator().manual_seed(1)
        self.dims, self.N, self.F, self.D = dims, sum(dims), len(dims), D
        self.xs = [torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV) for _ in range(NBATCH)]
        self.offsets = torch.tensor([0] + dims[:-1]).cumsum(0).to(DEV)
        self.W = (torch.rand(self.N, D, device=DEV) - 0.5) * 0.2
        self.w1 = torch.randn(self.N, 1, device=DEV)
        self.bias = torch.zeros(1, device=DEV)

    def forms(self, p):
        dense = pkg.prune_table(self.W.clone(), p)
        wide = PrunedEmbedding.from_pruned(self.W, p)
        compact = PrunedEmbedding.from_pruned(self.W, p, compact=True)
        return dense, wide, compact

    def fused(self, emb):
        ops = emb.fm_csr(self.xs[0])
        return lambda i: csr_fm.gather_fm_csr(self.xs[i % NBATCH], self.offsets, w1=self.w1, bias=self.bias, **ops)

    def parent(self, emb):
        """DeepFM._fm_and_embedding's fall-through: a torch add, the module's densify, mi_fm_fwd."""
        def run(i):
            rows = self.xs[i % NBATCH] + self.offsets
            return _kernels.fm_first_order(emb(rows), rows, self.w1, self.bias)
        return run

    def dense_fm(self, dense):
        return lambda i: _kernels.gather_fm(self.xs[i % NBATCH], self.offsets, dense, self.w1, self.bias)

    def rows(self, i):
        return self.xs[i % NBATCH] + self.offsets


def legs_ar(t, p, legs, rounds, out):
    dense, wide, compact = t.forms(p)
    out["stored_elements"] = wide.get_num_params()
    out["index_bytes"] = {"wide": 8 * (wide.col_indices.numel() + wide.crow_indices.numel()),
                          "compact": compact.col_indices.numel() + 4 * compact.crow_indices.numel()}
    with torch.no_grad():
        if "a" in legs:
            calls = {"fused_wide": t.fused(wide), "fused_compact": t.fused(compact), "parent_three_launches": t.parent(wide),
                     "dense_gather_fm": t.dense_fm(dense)}
            ref = calls["parent_three_launches"](0)
            for name in ("fused_wide", "fused_compact", "dense_gather_fm"):
                got = calls[name](0)
                torch.testing.assert_close(got[0], ref[0], rtol=0, atol=0)
                torch.testing.assert_close(got[1], ref[1], rtol=2e-5, atol=2e-5)
            r = rounds_of(calls, 50, rounds)
            r["condition_wide_vs_parent"] = condition(r, "fused_wide", "parent_three_launches")
            r["condition_compact_vs_parent"] = condition(r, "fused_compact", "parent_three_launches")
            r["condition_compact_vs_dense"] = condition(r, "fused_compact", "dense_gather_fm")
            r["condition_compact_vs_wide"] = condition(r, "fused_compact", "fused_wide")
            out["a_eval_lookup_fm"] = dict(r, calls_per_round=50)
        if "r" in legs:
            rows = [t.rows(i) for i in range(NBATCH)]
            calls = {"typed_compact": lambda i: compact(rows[i % NBATCH]), "csr_rows_wide": lambda i: wide(rows[i % NBATCH])}
            torch.testing.assert_close(calls["typed_compact"](0), calls["csr_rows_wide"](0), rtol=0, atol=0)
            r = rounds_of(calls, 50, rounds)
            r["condition"] = condition(r, "typed_compact", "csr_rows_wide")
            out["r_module_forward"] = dict(r, calls_per_round=50)
    _lib.check_index_errors()


def _model(t, embedding):
    torch.manual_seed(3)
    m = pkg.DeepFM(t.dims, t.D, HIDDEN, p_dropout=0.0, use_batchnorm=True, empty_embedding=True)
    m.embedding = embedding
    return m.to(DEV).eval()


def _dense_embedding(dense):
    emb = VanillaEmbedding([1], dense.shape[1])           # the holder only owns the parameter: lookups never call it
    emb._emb_module.weight = torch.nn.Parameter(dense)
    return emb


def legs_vm(t, p, legs, rounds, out):
    def allocated():
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    builders = {"dense": lambda: _dense_embedding(pkg.prune_table(t.W.clone(), p)),
                "csr_wide": lambda: PrunedEmbedding.from_pruned(t.W, p),
                "csr_compact": lambda: PrunedEmbedding.from_pruned(t.W, p, compact=True)}
    models, mem = {}, {}
    for name, build in builders.items():
        before = allocated()
        models[name] = _model(t, build())
        mem[name] = allocated() - before
    for name, compact in (("csr_wide_hooked_parent_path", False), ("csr_compact_hooked_three_launches", True)):
        hooked = _model(t, PrunedEmbedding.from_pruned(t.W, p, compact=compact))
        hooked.embedding.register_forward_hook(lambda mod, inp, out: None)
        models[name] = hooked
    if "m" in legs:
        other = mem["dense"] - 4 * t.N * t.D          # fc, the MLP, offsets: the same in every form
        out["m_memory_allocated_bytes"] = dict(mem, table_only={k: v - other for k, v in mem.items()},
                                               saving_vs_dense={k: round(1 - (v - other) / (4 * t.N * t.D), 4) for k, v in mem.items()})
    if "v" in legs:
        gen = torch.Generator().manual_seed(2)
        loader = [(torch.stack([torch.randint(0, d, (B,), generator=gen) for d in t.dims], 1).to(DEV),
                   (torch.rand(B, generator=gen) < 0.3).float().to(DEV)) for _ in range(64)]
        runs = {}
        for name, m in models.items():
            fwd = trainer.GraphedForward(m)
            runs[name] = lambda i, m=m, fwd=fwd: trainer.validate_epoch(loader, m, DEV, forward=fwd)
        aucs = {name: run(0)["auc"] for name, run in runs.items()}
        r = rounds_of(runs, 1, rounds)
        r["condition_compact_vs_dense"] = condition(r, "csr_compact", "dense")
        r["condition_compact_vs_parent_path"] = condition(r, "csr_compact", "csr_wide_hooked_parent_path")
        r["condition_wide_vs_parent_path"] = condition(r, "csr_wide", "csr_wide_hooked_parent_path")
        r["condition_compact_vs_three_launches"] = condition(r, "csr_compact", "csr_compact_hooked_three_launches")
        out["v_validate_epoch"] = dict(r, calls_per_round=1, batches=64, hidden=HIDDEN, auc=aucs)
    _lib.check_index_errors()


def leg_t(t, out):
    """What a kernel trace should see: TRACE_CALLS of each call of legs (a) and (r) at p = 0.8, nothing else of this library."""
    dense, wide, compact = t.forms(0.8)
    rows = [t.rows(i) for i in range(NBATCH)]
    order = []
    with torch.no_grad():
        for name, fn in (("fused_wide", t.fused(wide)), ("fused_compact", t.fused(compact)),
                         ("parent_three_launches", t.parent(wide)), ("dense_gather_fm", t.dense_fm(dense)),
                         ("typed_compact", lambda i: compact(rows[i % NBATCH])), ("csr_rows_wide", lambda i: wide(rows[i % NBATCH]))):
            for i in range(TRACE_CALLS):
                fn(i)
            order.append(name)
    torch.cuda.synchronize()
    out["t_trace"] = {"calls_each": TRACE_CALLS, "p": 0.8, "order": order}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tables cut by 4096: a rehearsal of the tool, not a measurement")
    ap.add_argument("--legs", default="arvm", help="which of the legs a, r, v, m to run; t: the calls of a kernel-trace run")
    ap.add_argument("--shapes", default="D16,D64", help="D16: 33 762 577 rows; D64: every field cut by 8")
    a = ap.parse_args()
    assert a.rounds >= 7, "medians of at least seven rounds"
    assert torch.cuda.is_available(), "kbench_csr_deepfm needs an MI355X"
    cut = 4096 if a.small else 1
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds, "rehearsal": bool(a.small), "shapes": {}}
    for shape in a.shapes.split(","):
        D, field_cut = (16, 1) if shape == "D16" else (64, 8)
        dims = [max(1, d // (cut * field_cut)) for d in CRITEO_KAGGLE_26]
        t = Table(dims, D)
        out = result["shapes"][f"criteo26_{shape}"] = {"fields": len(dims), "D": D, "rows": sum(dims),
                                                       "dense_table_bytes": 4 * sum(dims) * D}
        if "t" in a.legs:
            leg_t(t, out)
        for p in RATIOS:
            if not set(a.legs) & set("arvm"):
                break
            leg = out[f"p{p}"] = {}
            if "a" in a.legs or "r" in a.legs:
                legs_ar(t, p, a.legs, a.rounds, leg)
                torch.cuda.empty_cache()
            if "v" in a.legs or "m" in a.legs:
                legs_vm(t, p, a.legs, a.rounds, leg)
                torch.cuda.empty_cache()
        del t
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

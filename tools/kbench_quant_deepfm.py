"""DeepFM on the quantised tables (PTQ eval, QAT training) on the fused lookup, at the Criteo-26 shape (B = 4096, F = 26):
D = 16 at 33 762 577 rows and D = 64 at 4 220 315 rows (every field cut by 8).  Writes one JSON object.

Every leg times the new call against the path of the commit before it, in the same run — the old ops called directly, or
the same model with a no-op forward hook on its embedding (a hooked module keeps its own forward):
  (a) PTQ eval lookup + FM        gather_fm_quant                vs  gather_rows_quant(x + offsets) + fm_first_order,
                                  int8 / int16 / fp16, next to gather_fm on the unquantised fp32 table
  (v) one validate_epoch          64 batches on an int8 table, the model's new branch vs the hooked model
  (b) QAT forward + backward      gather_fm_qat                  vs  QAT lookup(x + offsets) + fm_first_order, dense
                                  gradients; row form and deterministic mode (the parent has neither: reported alone)
  (e) one whole QAT training step through GraphedTrainStep (captured and replayed), the new branch vs the hooked model

Every figure is the MEDIAN over --rounds rounds (default 7) of the time per call, device events around back-to-back calls
over a cycle of 16 different batches of uniform ids; the two paths alternate inside a round, and `spread_us` is max - min
over the rounds.  Per-call times include the Python and launch cost of the call.  `condition_*` compares the gap with the
PARENT path's spread.

    python tools/kbench_quant_deepfm.py --out profiles/quant_deepfm_kbench.json

Kernel times and launch counts (profiles/quant_deepfm_kernel_stats.csv) come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_quant_deepfm.py --legs t`: leg t
issues each call TRACE_CALLS times, new and parent, and nothing else.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from bench import CRITEO_KAGGLE_26  # noqa: E402
from recsys_benchmark_amd import _kernels, _lib, quant_fm, trainer  # noqa: E402
from recsys_benchmark_amd.embeddings.ptq_emb import PTQEmb_Int  # noqa: E402
from recsys_benchmark_amd.embeddings.qat_emb import _QatLookup  # noqa: E402

DEV = "cuda:0"
B, NBATCH, TRACE_CALLS = 4096, 16, 20
QAT_BITS = 8


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


def condition(res, new, parent):
    gap = res[parent]["median_us"] - res[new]["median_us"]
    return {"new": new, "parent": parent, "gap_us": round(gap, 2), "parent_spread_us": res[parent]["spread_us"],
            "ratio": round(res[parent]["median_us"] / res[new]["median_us"], 2), "holds": bool(gap > res[parent]["spread_us"]),
            "not_slower": bool(gap > -res[parent]["spread_us"])}


class Tables:
    """One shape: an fp32 table of uniform(-0.1, 0.1) weights, its int8 / int16 / fp16 forms (random codes under one scale:
    the lookup's cost does not depend on their values), the first-order table and 16 batches of uniform ids."""

    def __init__(self, dims, D):
        gen = torch.Generator().manual_seed(1)
        self.N, self.F, self.D = sum(dims), len(dims), D
        N = self.N
        self.xs = [torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV) for _ in range(NBATCH)]
        self.offsets = torch.tensor([0] + dims[:-1]).cumsum(0).to(DEV)
        self.W = ((torch.rand(N, D, device=DEV) - 0.5) * 0.2).requires_grad_(True)
        self.scale = torch.tensor(0.2 / 255, device=DEV).requires_grad_(True)      # the QAT scale at 8 bits: nothing clamps
        self.w1 = torch.randn(N, 1, device=DEV, requires_grad=True)
        self.bias = torch.zeros(1, device=DEV, requires_grad=True)
        self.leaves = [self.W, self.scale, self.w1, self.bias]
        self.G, self.gy = torch.randn(B, self.F, D, device=DEV), torch.randn(B, device=DEV)
        self.seed = torch.tensor([12345], device=DEV)

    def codes(self, kind):
        if kind == "fp16":
            return self.W.detach().to(torch.float16), None, None
        dt, lo, hi, sc = (torch.int8, -128, 128, 0.2 / 255) if kind == "int8" else (torch.int16, -32768, 32768, 0.2 / 65535)
        return (torch.randint(lo, hi, (self.N, self.D), dtype=dt, device=DEV), torch.tensor(sc, device=DEV),
                torch.tensor(0, dtype=dt, device=DEV))

    # ---- PTQ eval ----
    def quant_new(self, q):
        return lambda i: quant_fm.gather_fm_quant(self.xs[i % NBATCH], self.offsets, q[0], self.w1, self.bias, q[1], q[2])

    def quant_parent(self, q):
        sc, zp = (None, None) if q[1] is None else (q[1].reshape(1), q[2].reshape(1))

        def run(i):
            rows = self.xs[i % NBATCH] + self.offsets
            emb = _kernels.gather_rows_quant(rows, q[0], sc, zp)
            return _kernels.fm_first_order(emb, rows, self.w1, self.bias)
        return run

    def vanilla(self, i):
        return _kernels.gather_fm(self.xs[i % NBATCH], self.offsets, self.W, self.w1, self.bias)

    # ---- QAT ----
    def qat_new(self, i, sparse=False):
        return quant_fm.gather_fm_qat(self.xs[i % NBATCH], self.offsets, self.W, self.scale, QAT_BITS, self.w1, self.bias,
                                      seed=self.seed, sparse_W=sparse)

    def qat_parent(self, i, sparse=False):
        """DeepFM._fm_and_embedding's fall-through: x + offsets, the QAT lookup, mi_fm_fwd."""
        rows = self.xs[i % NBATCH] + self.offsets
        _kernels.note_field_layout(rows, self.offsets, self.N)
        emb = _QatLookup.apply(self.scale, self.W, rows, QAT_BITS, self.seed, 0, None, None)
        return _kernels.fm_first_order(emb, rows, self.w1, self.bias)

    def step(self, call, **kw):
        def run(i):
            for t in self.leaves:
                t.grad = None
            emb, y = call(i, **kw)
            torch.autograd.backward([emb, y], [self.G, self.gy])
        return run


def legs_ab(dims, D, legs, rounds, out):
    t = Tables(dims, D)
    if "a" in legs:
        ra = {}
        with torch.no_grad():
            for kind in ("int8", "int16", "fp16"):
                q = t.codes(kind)
                new, parent = t.quant_new(q), t.quant_parent(q)
                f, p = new(0), parent(0)
                torch.testing.assert_close(f[0], p[0], rtol=0, atol=0)
                torch.testing.assert_close(f[1], p[1], rtol=2e-5, atol=2e-5)
                r = rounds_of({f"new_{kind}": new, f"parent_{kind}": parent, f"unquantised_gather_fm_{kind}": t.vanilla}, 50, rounds)
                ra.update(r)
                ra[f"condition_{kind}"] = condition(r, f"new_{kind}", f"parent_{kind}")
                del q
        out["a_ptq_eval_lookup_fm"] = dict(ra, calls_per_round=50)
    if "b" in legs:
        rb = {}
        with torch.no_grad():
            f, p = t.qat_new(0), t.qat_parent(0)
            torch.testing.assert_close(f[0], p[0], rtol=0, atol=0)
        r = rounds_of({"new_dense": t.step(t.qat_new), "parent_dense": t.step(t.qat_parent)}, 5, rounds)
        rb.update(r)
        rb["condition_dense"] = condition(r, "new_dense", "parent_dense")
        rb.update(rounds_of({"new_rows": t.step(t.qat_new, sparse=True)}, 5, rounds))
        pkg.use_deterministic_algorithms(True)
        try:
            rb.update(rounds_of({"new_deterministic": t.step(t.qat_new)}, 5, rounds))
        finally:
            pkg.use_deterministic_algorithms(False)
        out["b_qat_fwd_bwd"] = dict(rb, calls_per_round=5, n_bits=QAT_BITS)
    _lib.check_index_errors()
    del t
    torch.cuda.empty_cache()


def _batches(dims, n):
    gen = torch.Generator().manual_seed(2)
    xs = [torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV) for _ in range(n)]
    ys = [(torch.rand(B, generator=gen) < 0.3).float().to(DEV) for _ in range(n)]
    return xs, ys


def _hook(m):
    """The parent's path in the same process: a hooked embedding module keeps its own forward."""
    m.embedding.register_forward_hook(lambda mod, inp, out: None)
    return m


def leg_v(dims, D, rounds, out):
    """validate_epoch over 64 batches of a DeepFM whose embedding is an int8 PTQ table (scripts/deepfm/run_ptq.py)."""
    xs, ys = _batches(dims, 64)
    loader = list(zip(xs, ys))
    runs = {}
    for name in ("new", "parent"):
        torch.manual_seed(3)
        m = pkg.DeepFM(dims, D, [400, 400, 400], p_dropout=0.0, use_batchnorm=True, empty_embedding=True)
        # the class's own constructor on a one-row checkpoint (a 2 GB checkpoint file of the whole table is not needed to
        # time a lookup), then codes of the table's size in its `weight` buffer: the lookup's cost does not depend on them
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "original.pth")
            torch.save({"state_dict": {"embedding._emb_module.weight": torch.tensor([[-0.1] + [0.1] * (D - 1)])}}, path)
            emb = PTQEmb_Int(None, None, None, path, n_bits=8)
        emb.weight = torch.randint(-128, 128, (sum(dims), D), dtype=torch.int8)
        m.embedding = emb
        m = m.to(DEV).eval()
        if name == "parent":
            _hook(m)
        fwd = trainer.GraphedForward(m)
        runs[name] = lambda i, m=m, fwd=fwd: trainer.validate_epoch(loader, m, DEV, forward=fwd)
    r = rounds_of(runs, 1, rounds)
    r["condition"] = condition(r, "new", "parent")
    out["v_validate_epoch_int8"] = dict(r, calls_per_round=1, batches=64, hidden=[400, 400, 400])


def leg_e(dims, D, rounds, out):
    """One QAT training step (lookup + FM + MLP tail + BCE, backward, Adam) as a replayed graph."""
    from recsys_benchmark_amd.optim import Adam

    xs, ys = _batches(dims, NBATCH)
    steps = {}
    for name in ("new", "parent"):
        torch.manual_seed(3)
        cfg = {"name": "qat", "n_bits": QAT_BITS}
        m = pkg.DeepFM(dims, D, [400, 400, 400], p_dropout=0.0, use_batchnorm=True, embedding_config=cfg).to(DEV).train()
        if name == "parent":
            _hook(m)
        step = trainer.GraphedTrainStep(m, Adam(m.parameters(), lr=1e-3))
        for i in range(4):
            step(xs[i], ys[i])
        assert step._graph is not None, f"{name}: the step was not captured"
        steps[name] = lambda i, step=step: step(xs[i % NBATCH], ys[i % NBATCH])
    r = rounds_of(steps, 20, rounds)
    r["condition"] = condition(r, "new", "parent")
    _lib.check_index_errors()
    out["e_qat_step_graphed"] = dict(r, calls_per_round=20, hidden=[400, 400, 400], n_bits=QAT_BITS)


def leg_t(dims, D, out):
    """What a kernel trace should see: TRACE_CALLS of each call, new then parent, nothing else of this library."""
    t = Tables(dims, D)
    order = []
    with torch.no_grad():
        for kind in ("int8", "int16", "fp16"):
            q = t.codes(kind)
            for name, fn in (("new", t.quant_new(q)), ("parent", t.quant_parent(q))):
                for i in range(TRACE_CALLS):
                    fn(i)
                order.append(f"ptq_{kind}_{name}")
    for name, fn in (("new", t.qat_new), ("parent", t.qat_parent)):
        step = t.step(fn)
        for i in range(TRACE_CALLS):
            step(i)
        order.append(f"qat_dense_{name}")
    pkg.use_deterministic_algorithms(True)
    try:
        step = t.step(t.qat_new)
        for i in range(TRACE_CALLS):
            step(i)
    finally:
        pkg.use_deterministic_algorithms(False)
    order.append("qat_deterministic_new")
    torch.cuda.synchronize()
    out["t_trace"] = {"calls_each": TRACE_CALLS, "order": order}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tables cut by 4096: a rehearsal of the tool, not a measurement")
    ap.add_argument("--legs", default="abve", help="which of the legs a, b, v, e to run; t: the calls of a kernel-trace run")
    ap.add_argument("--shapes", default="D16,D64", help="D16: 33 762 577 rows; D64: every field cut by 8")
    a = ap.parse_args()
    assert a.rounds >= 7, "medians of at least seven rounds"
    assert torch.cuda.is_available(), "kbench_quant_deepfm needs an MI355X"
    cut = 4096 if a.small else 1
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds, "rehearsal": bool(a.small), "shapes": {}}
    for shape in a.shapes.split(","):
        D, field_cut = (16, 1) if shape == "D16" else (64, 8)
        dims = [max(1, d // (cut * field_cut)) for d in CRITEO_KAGGLE_26]
        out = result["shapes"][f"criteo26_{shape}"] = {"fields": len(dims), "D": D, "rows": sum(dims)}
        if "t" in a.legs:
            leg_t(dims, D, out)
        if "a" in a.legs or "b" in a.legs:
            legs_ab(dims, D, a.legs, a.rounds, out)
        if "v" in a.legs:
            leg_v(dims, D, a.rounds, out)
        if "e" in a.legs:
            leg_e(dims, D, a.rounds, out)
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

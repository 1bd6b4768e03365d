"""The packed 4-bit PTQ table (PTQEmb_Int(n_bits=4, packed=True)) at the Criteo-26 shape (B = 4096, F = 26): D = 16 at
33 762 577 rows and D = 64 at 4 220 315 rows (every field cut by 8).  Writes one JSON object.

Four tables of the same fp32 weights in the same run — packed int4, the int8-storage n_bits = 4 table (the parent's
behaviour), the int8 table, and the unquantised fp32 table:
  (m) torch.cuda.memory_allocated of the table alone (the growth while it is built, temporaries released)
  (a) the fused eval lookup + FM        quant_fm.gather_fm_quant (packed4 / int8 codes), _kernels.gather_fm on fp32
  (f) the embedding module's forward    PTQEmb_Int.forward over x + offsets, _kernels.gather_rows on fp32
  (v) one validate_epoch of 64 batches  a DeepFM ([400, 400, 400]) on each table through a GraphedForward
  (q) PTQEmb_Int.from_table on the device against affine_codes on the host (D = 16 only: the host needs ~9 GB)

Every figure is the MEDIAN over --rounds rounds (default 7) of the time per call, device events around back-to-back calls over
a cycle of 16 different batches of uniform ids; the paths alternate inside a round, and `spread_us` is max - min over the
rounds.  Per-call times include the Python and launch cost of the call.  (q) is timed once per round by the host clock around
a synchronised call.

    python tools/kbench_int4_deepfm.py --out profiles/int4_deepfm_kbench.json

Kernel times and launch counts (profiles/int4_deepfm_kernel_stats.csv) come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_int4_deepfm.py --legs t --shapes D16`:
leg t issues each call TRACE_CALLS times and nothing else.
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
from recsys_benchmark_amd import _kernels, _lib, quant_fm, trainer  # noqa: E402
from recsys_benchmark_amd.embeddings.ptq_emb import PTQEmb_Int, affine_codes  # noqa: E402

DEV = "cuda:0"
B, NBATCH, TRACE_CALLS = 4096, 16, 20
KINDS = ("packed_int4", "int8_storage_int4", "int8", "fp32")


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
    return {k: _stats(v) for k, v in times.items()}


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
            "rounds_us": [round(t, 2) for t in v]}


class Tables:
    """One shape: an fp32 table of uniform(-0.1, 0.1) weights and its three quantised forms, each built by
    PTQEmb_Int.from_table on the device, the first-order table and 16 batches of uniform ids."""

    def __init__(self, dims, D):
        gen = torch.Generator().manual_seed(1)
        self.dims, self.N, self.F, self.D = dims, sum(dims), len(dims), D
        self.xs = [torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV) for _ in range(NBATCH)]
        self.offsets = torch.tensor([0] + dims[:-1]).cumsum(0).to(DEV)
        self.memory, self.emb = {}, {}
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        self.W = (torch.rand(self.N, D, device=DEV) - 0.5) * 0.2
        torch.cuda.synchronize()
        self.memory["fp32"] = torch.cuda.memory_allocated() - base
        for kind, bits, packed in (("packed_int4", 4, True), ("int8_storage_int4", 4, False), ("int8", 8, False)):
            base = torch.cuda.memory_allocated()
            self.emb[kind] = PTQEmb_Int.from_table(self.W, n_bits=bits, packed=packed)
            torch.cuda.synchronize()
            self.memory[kind] = torch.cuda.memory_allocated() - base      # (with the two 0-dim scalars' blocks)
        self.w1 = torch.randn(self.N, 1, device=DEV)
        self.bias = torch.zeros(1, device=DEV)

    def fused(self, kind):
        if kind == "fp32":
            return lambda i: _kernels.gather_fm(self.xs[i % NBATCH], self.offsets, self.W, self.w1, self.bias)
        ops = self.emb[kind]._fm_operands()
        return lambda i: quant_fm.gather_fm_quant(self.xs[i % NBATCH], self.offsets, w1=self.w1, bias=self.bias, **ops)

    def forward(self, kind):
        if kind == "fp32":
            return lambda i: _kernels.gather_rows(self.xs[i % NBATCH] + self.offsets, self.W, False)
        emb = self.emb[kind]
        return lambda i: emb(self.xs[i % NBATCH] + self.offsets)


def legs_maf(t, legs, rounds, out):
    out["m_table_bytes"] = dict(t.memory, exact_packed_bytes=t.N * t.D // 2, exact_int8_bytes=t.N * t.D, exact_fp32_bytes=t.N * t.D * 4)
    with torch.no_grad():
        ref = t.fused("int8_storage_int4")(0)
        got = t.fused("packed_int4")(0)
        torch.testing.assert_close(got[0], ref[0], rtol=0, atol=0)
        torch.testing.assert_close(got[1], ref[1], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(t.forward("packed_int4")(0), t.forward("int8_storage_int4")(0), rtol=0, atol=0)
        if "a" in legs:
            out["a_fused_eval_lookup_fm"] = dict(rounds_of({k: t.fused(k) for k in KINDS}, 50, rounds), calls_per_round=50)
        if "f" in legs:
            out["f_embedding_forward"] = dict(rounds_of({k: t.forward(k) for k in KINDS}, 50, rounds), calls_per_round=50)
    _lib.check_index_errors()


def leg_v(t, rounds, out):
    gen = torch.Generator().manual_seed(2)
    xs = [torch.stack([torch.randint(0, d, (B,), generator=gen) for d in t.dims], 1).to(DEV) for _ in range(64)]
    ys = [(torch.rand(B, generator=gen) < 0.3).float().to(DEV) for _ in range(64)]
    loader = list(zip(xs, ys))
    runs = {}
    for kind in KINDS:
        torch.manual_seed(3)
        m = pkg.DeepFM(t.dims, t.D, [400, 400, 400], p_dropout=0.0, use_batchnorm=True, empty_embedding=True)
        if kind == "fp32":
            m.embedding = pkg.embeddings.VanillaEmbedding(1, t.D)
            m.embedding._emb_module.weight = torch.nn.Parameter(t.W, requires_grad=False)
        else:
            m.embedding = t.emb[kind]
        m = m.to(DEV).eval()
        fwd = trainer.GraphedForward(m)
        runs[kind] = lambda i, m=m, fwd=fwd: trainer.validate_epoch(loader, m, DEV, forward=fwd)
    out["v_validate_epoch"] = dict(rounds_of(runs, 1, rounds), calls_per_round=1, batches=64, hidden=[400, 400, 400])


def leg_q(t, rounds, out):
    """from_table on the device (one read-back of the extremes + one launch) against affine_codes on the host."""
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e6
        del r
        return dt

    res = {}
    for name, bits, packed in (("packed_int4", 4, True), ("int8", 8, False)):
        timed(lambda: PTQEmb_Int.from_table(t.W, n_bits=bits, packed=packed))
        res[f"device_from_table_{name}"] = _stats([timed(lambda: PTQEmb_Int.from_table(t.W, n_bits=bits, packed=packed))
                                                   for _ in range(rounds)])
    host = t.W.cpu()
    res["host_affine_codes_int4"] = _stats([timed(lambda: affine_codes(host, 4)) for _ in range(3)])
    res["host_rounds"] = 3
    out["q_quantiser"] = res


def leg_t(t, out):
    """What a kernel trace should see: TRACE_CALLS of each call, nothing else of this library."""
    order = []
    with torch.no_grad():
        for kind in KINDS:
            for name, fn in (("fused", t.fused(kind)), ("forward", t.forward(kind))):
                for i in range(TRACE_CALLS):
                    fn(i)
                order.append(f"{kind}_{name}")
        for i in range(TRACE_CALLS):
            t.emb["packed_int4"](t.xs[i % NBATCH], offsets=t.offsets)
        order.append("packed_int4_forward_offsets")
    torch.cuda.synchronize()
    out["t_trace"] = {"calls_each": TRACE_CALLS, "order": order}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tables cut by 4096: a rehearsal of the tool, not a measurement")
    ap.add_argument("--legs", default="mafvq", help="which of the legs m, a, f, v, q to run; t: the calls of a kernel-trace run")
    ap.add_argument("--shapes", default="D16,D64", help="D16: 33 762 577 rows; D64: every field cut by 8")
    a = ap.parse_args()
    assert a.rounds >= 7, "medians of at least seven rounds"
    assert torch.cuda.is_available(), "kbench_int4_deepfm needs an MI355X"
    cut = 4096 if a.small else 1
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds, "rehearsal": bool(a.small), "shapes": {}}
    for shape in a.shapes.split(","):
        D, field_cut = (16, 1) if shape == "D16" else (64, 8)
        dims = [max(1, d // (cut * field_cut)) for d in CRITEO_KAGGLE_26]
        out = result["shapes"][f"criteo26_{shape}"] = {"fields": len(dims), "D": D, "rows": sum(dims)}
        t = Tables(dims, D)
        if "t" in a.legs:
            leg_t(t, out)
        if set("maf") & set(a.legs):
            legs_maf(t, a.legs, a.rounds, out)
        if "v" in a.legs:
            leg_v(t, a.rounds, out)
        if "q" in a.legs and D == 16:
            leg_q(t, a.rounds, out)
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

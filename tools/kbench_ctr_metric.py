"""The CTR validation metric on the device (csrc/ctr_metric.hip) against the chain of stock torch ops it replaces.  Writes one
JSON object.

  (a) binary_auc on sigmoid outputs of seeded normal logits, n = 262 144 (64 batches of 4096) and n = 4 584 062 (a tenth of
      Criteo), labels Bernoulli(0.3):
        kernel_no_read   _kernels.binary_auc_device alone (sort, count, division; nothing read back)
        kernel           trainer.binary_auc: label bytes, the kernels, the one host read
        torch_ops        trainer._binary_auc_torch on the same tensors: torch.unique(sorted, inverse, counts), cumsum, gather,
                         two reductions, its host reads — the form every caller had before
  (b) the same with the scores quantised to 1 000 levels (large groups of equal scores)
  (c) one validate_epoch of a DeepFM (MLP 400 x 3, the Criteo-26 fields, D = 16) over 64 batches of 4096 through one kept
      GraphedForward: trainer.validate_epoch with a kept CTRMetric against `parent_validate_epoch` below — the loop the
      previous commit ran (a BCEWithLogitsLoss(sum) launch, a float64 +=, a sigmoid and two appends per batch; two cats and
      the torch-op AUC at the end)
  (d) one search candidate end to end on the OptEmbed supernet: set_candidate + that validation pass, new against parent

Legs (a), (b): the MEDIAN over --rounds rounds (default 7) of the time per call, device events around back-to-back calls,
the variants alternating inside a round; `spread_us` is max - min over the rounds.  Legs (c), (d): a host clock around one
pass that ends in a synchronise, the two variants alternating, median and max - min over the rounds.  Per-call times include
the Python and launch cost of the call.  `holds` says whether the gap exceeds the larger of the two spreads.

    python tools/kbench_ctr_metric.py --out profiles/ctr_metric_kbench.json

Kernel times (profiles/ctr_metric_kernel_stats.csv) come from a run of leg (c) alone under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_ctr_metric.py --legs c`.
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
B, NVAL = 4096, 64


def per_call_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def rounds_of(variants, n, rounds):
    """{name: {"median_us", "spread_us", "rounds_us"}}; every round times each variant once, in turn."""
    for fn in variants.values():          # warm-up: code objects, allocator, the kept workspace
        per_call_us(fn, min(n, 3))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(per_call_us(fn, n))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                "rounds_us": [round(t, 2) for t in v]} for k, v in times.items()}


def condition(res, fast, slow, unit="us"):
    gap = res[slow][f"median_{unit}"] - res[fast][f"median_{unit}"]
    spread = max(res[slow][f"spread_{unit}"], res[fast][f"spread_{unit}"])
    return {"fast": fast, "slow": slow, f"gap_{unit}": round(gap, 3), f"larger_spread_{unit}": spread,
            "holds": bool(gap > spread)}


def leg_auc(n, levels, rounds):
    gen = torch.Generator().manual_seed(n % 9973 + (levels or 0))
    score = torch.sigmoid(torch.randn(n, generator=gen))
    if levels:
        score = torch.floor(score * levels) / levels
    label = (torch.rand(n, generator=gen) < 0.3).float()
    score, label = score.to(DEV), label.to(DEV)
    bytes_ = label.to(torch.uint8)
    new, old = trainer.binary_auc(label, score), trainer._binary_auc_torch(label, score)
    variants = {"kernel_no_read": lambda: _kernels.binary_auc_device(score, bytes_),
                "kernel": lambda: trainer.binary_auc(label, score),
                "torch_ops": lambda: trainer._binary_auc_torch(label, score)}
    res = rounds_of(variants, 20 if n < 10**6 else 5, rounds)
    res.update(n=n, levels=levels, distinct_scores=int(torch.unique(score).numel()), auc_kernel=new, auc_torch_ops=old,
               abs_difference=abs(new - old))
    res["condition_kernel_faster_than_torch_ops"] = condition(res, "kernel", "torch_ops")
    return res


@torch.no_grad()
def parent_validate_epoch(val_loader, model, device, forward):
    """trainer.validate_epoch as the commit before CTRMetric had it ("DeepFM PEP: soft-threshold search and retraining on the
    fused lookup", trainer.py:423-443 there), copied line for line: torch ops per batch, the torch-op AUC at the end.  It is
    a fixed baseline and is NOT meant to follow later changes of trainer.validate_epoch."""
    model.eval()
    criterion = torch.nn.BCEWithLogitsLoss(reduction="sum")
    log_loss = torch.zeros((), dtype=torch.float64, device=device)
    y_true, y_pred = [], []
    for inputs, labels in val_loader:
        inputs, labels = inputs.to(device), labels.to(device)
        outputs = forward(inputs)
        log_loss += criterion(outputs, labels.float())
        y_true.append(labels.reshape(-1))
        y_pred.append(torch.sigmoid(outputs).reshape(-1))
    y_true, y_pred = torch.cat(y_true), torch.cat(y_pred)
    _lib.check_index_errors()
    return {"auc": trainer._binary_auc_torch(y_true, y_pred), "log_loss": float(log_loss) / y_pred.numel()}


def timed_ms(variants, rounds):
    """Host clock around each variant's call (which ends in a host read) plus a synchronise; variants alternate."""
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3),
                "rounds_ms": [round(t, 3) for t in v]} for k, v in times.items()}


def val_loader(dims, gen, nval):
    return [(torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1).to(DEV),
             (torch.rand(B, generator=gen) < 0.3).float().to(DEV)) for _ in range(nval)]


def leg_c(dims, rounds, nval):
    gen = torch.Generator().manual_seed(2)
    torch.manual_seed(0)
    m = pkg.DeepFM(dims, 16, [400, 400, 400], p_dropout=0.0, embedding_config={"name": "vanilla"}).to(DEV).eval()
    loader = val_loader(dims, gen, nval)
    forward, parent_forward = trainer.GraphedForward(m), trainer.GraphedForward(m)
    metric = pkg.CTRMetric(DEV, capacity=nval * B)
    new = lambda: trainer.validate_epoch(loader, m, device=DEV, forward=forward, metric=metric)      # noqa: E731
    old = lambda: parent_validate_epoch(loader, m, DEV, parent_forward)                                # noqa: E731
    for _ in range(2):                                        # warm-up: both graphs captured, buffers and workspace kept
        got, want = new(), old()
    res = timed_ms({"new_validate_ms": new, "parent_validate_ms": old}, rounds)
    res.update(validation_batches=nval, hidden=[400, 400, 400], graphs_replayed=bool(forward.use_graph),
               new_result=got, parent_result=want, auc_abs_difference=abs(got["auc"] - want["auc"]),
               log_loss_abs_difference=abs(got["log_loss"] - want["log_loss"]))
    res["condition_new_faster_than_parent"] = condition(res, "new_validate_ms", "parent_validate_ms", "ms")
    return res


def leg_d(dims, rounds, nval):
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(0)
    D = 16
    m = pkg.DeepFM(dims, D, [400, 400, 400], p_dropout=0.0,
                   embedding_config={"name": "deepfm_optembed", "mode_threshold_d": "field"}).to(DEV).eval()
    with torch.no_grad():
        m.embedding._weight.uniform_(-0.5, 0.5)
        m.embedding._mask_e_module._t_param.fill_(D / 4)
        m.fc.weight.normal_()
    emb = m.embedding
    loader = val_loader(dims, gen, nval)
    cands = [torch.randint(0, D, (len(dims),), generator=gen).to(DEV) for _ in range(rounds + 2)]
    forward, parent_forward = trainer.GraphedForward(m), trainer.GraphedForward(m)
    metric = pkg.CTRMetric(DEV, capacity=nval * B)
    state = {"i": 0}

    def new():
        emb.set_candidate(cands[state["i"] % len(cands)])
        return trainer.validate_epoch(loader, m, device=DEV, forward=forward, metric=metric)

    def old():
        emb.set_candidate(cands[state["i"] % len(cands)])
        return parent_validate_epoch(loader, m, DEV, parent_forward)

    for _ in range(2):
        got, want = new(), old()
        state["i"] += 1
    times = {"new_candidate_ms": [], "parent_candidate_ms": []}
    for _ in range(rounds):
        for key, fn in (("new_candidate_ms", new), ("parent_candidate_ms", old)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3)
        state["i"] += 1
    emb.clear_candidate()
    res = {k: {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3),
               "rounds_ms": [round(t, 3) for t in v]} for k, v in times.items()}
    res.update(validation_batches=nval, hidden=[400, 400, 400], graphs_replayed=bool(forward.use_graph),
               warmup_auc_new_vs_parent=[got["auc"], want["auc"]])
    res["condition_new_faster_than_parent"] = condition(res, "new_candidate_ms", "parent_candidate_ms", "ms")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tables and sizes cut down: a rehearsal of the tool, not a measurement")
    ap.add_argument("--legs", default="abcd", help="which of the legs a, b, c, d to run (a kernel-trace run wants 'c' alone)")
    a = ap.parse_args()
    assert a.rounds >= 5, "medians of at least five rounds"
    assert torch.cuda.is_available(), "kbench_ctr_metric needs an MI355X"
    dims = [max(1, d // (4096 if a.small else 1)) for d in CRITEO_KAGGLE_26]
    sizes = (4099, 70_001) if a.small else (NVAL * B, 4_584_062)
    nval = 4 if a.small else NVAL
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds, "rehearsal": bool(a.small)}
    if "a" in a.legs:
        result["a_binary_auc"] = {f"n{n}": leg_auc(n, None, a.rounds) for n in sizes}
    if "b" in a.legs:
        result["b_binary_auc_1000_levels"] = {f"n{n}": leg_auc(n, 1000, a.rounds) for n in sizes}
    if "c" in a.legs:
        result["c_validate_epoch"] = leg_c(dims, a.rounds, nval)
        torch.cuda.empty_cache()
    if "d" in a.legs:
        result["d_search_candidate"] = leg_d(dims, a.rounds, nval)
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""Global magnitude pruning (pruning.prune_table, csrc/mag_prune.hip) against the reference's op sequence
(src/utils.py:8-34: per-row topk, index write, full argsort, index write) written in stock torch on the same GPU, at
the Yelp2018 user and item tables (31 668 / 38 048 x 64, floor 0 and 6, p = 0.8) and the Criteo-Kaggle table
(33 762 577 x 16, floor 0), and one `evaluate_pruned` candidate of a Yelp2018-shaped LightGCN end to end against the
same candidate pruned by the torch baseline.  Prints one JSON line and writes it to --out.

The two forms alternate in rounds inside one process; both prune in place a table refreshed by the same copy_ before
every call (the copy is inside both figures; `out_of_place_us` is the library pruning from the original straight into
the destination, no copy).  Every figure is the median over the rounds of device-event time around `calls` back-to-back
calls (Python and launch cost included); `spread_*` is (max - min) / median over the rounds.  `bytes` is what the
kernels must move, from the shapes: the table once per digit pass (3), once for the row cut when the floor is > 0, once
read and once written by the apply pass (NOT the counting read of the tie path, which a run may also make: the share
derived from `bytes` is a lower bound).  Per-kernel times come from one rocprofv3 --kernel-trace --stats run per shape
of `--shapes <shape> --rounds 1 --no-baseline` (yelp_item, criteo: profiles/mag_prune_kernel_stats.csv).

    python tools/kbench_mag_prune.py [--rounds 3] [--calls 50] [--out profiles/mag_prune_kbench.json]
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
from recsys_benchmark_amd import trainer  # noqa: E402
from recsys_benchmark_amd.graph_utils import calculate_sparse_graph_adj_norm  # noqa: E402

DEV = "cuda:0"
ACHIEVABLE = 6.3e12          # bytes/s a streaming kernel reaches on this part
SHAPES = {"yelp_user": (31668, 64, (0, 6)), "yelp_item": (38048, 64, (0, 6)), "criteo": (33762577, 16, (0,))}
P = 0.8


def torch_baseline(table, ratio, floor):
    """The reference's four ops (src/utils.py:8-34) in stock torch, written for this tool: a per-row top-k of the
    magnitudes, an index write that marks those `floor` elements per row with inf, a full argsort of all N * D marked
    magnitudes, and an index write of zeros at the first k positions of that order (through the flat view: one index
    tensor where the reference derives a row and a column index first, so this baseline is, if anything, the cheaper
    one).  Prunes the contiguous `table` in place."""
    marked = table.abs()
    marked.scatter_(1, marked.topk(floor, dim=1).indices, float("inf"))
    order = marked.view(-1).argsort()
    k = int(order.numel() * ratio)
    table.view(-1)[order[:k]] = 0
    return table


def timed(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us


def summarise(xs):
    med = statistics.median(xs)
    return {"median_us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 3), "rounds": [round(x, 2) for x in xs]}


def leg_tables(out, shapes, rounds, calls, baseline):
    for tag in shapes:
        n, d, floors = SHAPES[tag]
        torch.manual_seed(0)
        orig = torch.randn(n, d, device=DEV) * 0.1
        work = torch.empty_like(orig)
        for m in floors:
            lib = lambda: pkg.prune_table(work.copy_(orig), P, m)              # noqa: E731
            lib_oop = lambda: pkg.prune_table(orig, P, m, out=work)            # noqa: E731
            ref = lambda: torch_baseline(work.copy_(orig), P, m)                  # noqa: E731
            entry = {"N": n, "D": d, "p": P, "min_item": m, "calls": calls,
                     "launches": 6 + (1 if m > 0 else 0),      # memset, [row cut], 3 digit passes, finish, apply
                     "bytes": (5 + (1 if m > 0 else 0)) * n * d * 4}
            can_ref = baseline
            if baseline:
                try:
                    a = lib().clone()
                    b = ref()
                    entry["equal_to_baseline"] = bool(torch.equal(a, b))      # (an unstable sort may differ at tied cuts)
                    entry["zeros"] = [int((a == 0).sum()), int((b == 0).sum())]
                    del a, b
                except torch.cuda.OutOfMemoryError as e:
                    can_ref = False
                    entry["baseline"] = "did not run: out of memory (" + str(e).split(".")[0] + ")"
                    torch.cuda.empty_cache()
            t = {"lib": [], "oop": [], "ref": []}
            for _ in range(rounds):
                if can_ref:
                    t["ref"].append(timed(ref, calls))
                t["lib"].append(timed(lib, calls))
                t["oop"].append(timed(lib_oop, calls))
            entry["library_us"] = summarise(t["lib"])
            entry["out_of_place_us"] = summarise(t["oop"])
            entry["achievable_share_lower_bound"] = round(entry["bytes"] / (entry["out_of_place_us"]["median_us"] * 1e-6)
                                                          / ACHIEVABLE, 4)
            if can_ref:
                entry["baseline_us"] = summarise(t["ref"])
                entry["baseline_over_library"] = round(entry["baseline_us"]["median_us"] / entry["library_us"]["median_us"], 2)
            out[f"{tag}_m{m}"] = entry
        del orig, work
        torch.cuda.empty_cache()


class _Data:
    def __init__(self, graph, adj):
        self._graph, self._adj = graph, adj

    def get_graph(self):
        return self._graph

    def get_norm_adj(self):
        return self._adj


def leg_candidate(out, rounds, m=6):
    """One search candidate end to end on a Yelp2018-shaped LightGCN (L = 3): prune both tables, validate every user
    (batches of 2048), restore."""
    U, I, D = SHAPES["yelp_user"][0], SHAPES["yelp_item"][0], 64
    gen = torch.Generator().manual_seed(0)
    graph = {u: sorted(set(torch.randint(0, I, (int(torch.randint(5, 60, (1,), generator=gen)),), generator=gen).tolist()))
             for u in range(U)}
    data = _Data(graph, calculate_sparse_graph_adj_norm(graph, I, U))
    val = [(torch.arange(s, min(s + 2048, U)), [torch.randint(0, I, (5,), generator=gen).tolist() for _ in range(s, min(s + 2048, U))])
           for s in range(0, U, 2048)]
    torch.manual_seed(0)
    model = pkg.LightGCN(U, I, num_layers=3, hidden_size=D).to(DEV)

    def library():
        return pkg.evaluate_pruned(model, P, m, val, data, DEV)

    def baseline():
        state = model.state_dict()
        keep = {k: v.clone() for k, v in state.items()}
        for v in state.values():
            torch_baseline(v, P, m)
        ndcg = trainer.validate_epoch_cf(data, val, model, DEV, metrics=["ndcg", "recall"])["ndcg"]
        model.load_state_dict(keep)
        return ndcg

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    window(library), window(baseline)
    lib, ref = [], []
    for _ in range(rounds):
        ref.append(window(baseline)[0])
        lib.append(window(library)[0])
    med = statistics.median
    out["evaluate_pruned_candidate"] = {
        "model": "LightGCN L=3", "users": U, "items": I, "D": D, "p": P, "min_item": m,
        "library_ms": round(med(lib), 2), "baseline_ms": round(med(ref), 2),
        "spread_library": round((max(lib) - min(lib)) / med(lib), 3), "spread_baseline": round((max(ref) - min(ref)) / med(ref), 3),
        "ndcg_library": window(library)[1], "ndcg_baseline": window(baseline)[1]}


def recorded_args(argv):
    """The arguments that shape the measurement: where the line is written (--out) is not one of them."""
    kept, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a == "--out":
            skip = True
        elif not a.startswith("--out="):
            kept.append(a)
    return kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="yelp_user,yelp_item,criteo")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-candidate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_mag_prune needs an MI355X"
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "command": "python tools/kbench_mag_prune.py " + " ".join(recorded_args(sys.argv[1:]))}
    leg_tables(out, [s for s in args.shapes.split(",") if s], args.rounds, args.calls, not args.no_baseline)
    if not args.no_candidate and not args.no_baseline:
        leg_candidate(out, args.rounds)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

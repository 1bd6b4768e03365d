"""`tt_emb` (TT-Rec behind an LFU row cache) against `tt_emb_torch` on the same ids and cores.  Writes one JSON object.

Shapes: the README's TT shape — Criteo-39, N = 1 086 810, D = 16, ranks [128, 96], B = 4096 x F = 39 = 159 744 lookups
(configs/deepfm/tt_rec.yaml) — and one CF shape — Gowalla's items, N = 40 981, D = 64, ranks [96, 80]
(configs/gowalla/tt-emb-80.yaml), 8192 lookups; its last level is a GEMM level (H * K > 512), the README shape's is not.

  (h) forward, and forward + backward, at hit rates 0, 0.5, 0.9 and 0.99: Zipf ids (exponent 1.1 over a fixed permutation
      of the vocabulary), 16 batches; cache_size is the number of hottest ids whose share of the 16 batches reaches the rate
      (hit rate 0: the table in warmup, nothing populated), the table counts the batches and is populated from them; the
      achieved rate is reported.  Against `tt_emb_torch` (TTRecTorch) on the same batches and cores.
  (p) the probe / count launch alone (tt_cache.probe_count) on a uniform batch and on a batch whose first field holds ONE id
      (4096 equal ids next to 38 uniform fields), table in direct addressing.
  (c) cache_populate() at the cache sizes of (h).
A cached table runs the per-lookup kernels at every batch size; `tt_emb_torch` takes the grouped MFMA form at these sizes.
There is no leg for a captured training step: such a step at 159 744 lookups, replayed after cache_populate(), ended in a
GPU memory fault whose cause is not known; do not add one before it is.

Every figure is the MEDIAN over --rounds rounds (default 7) of the time per call, device events around back-to-back calls
over the cycle of 16 batches; the paths alternate inside a round, and `spread_us` is max - min over the rounds.  Per-call
times include the Python and launch cost of the call.  A gap inside the other path's spread is a tie.

    python tools/kbench_tt_cache.py --out profiles/tt_cache_kbench.json

Neither that JSON nor the kernel trace below has been produced yet: no timing of this table exists.
Kernel times and launch counts (to be saved as profiles/tt_cache_kernel_stats.csv) come from a run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_tt_cache.py --legs t`: leg t issues
TRACE_CALLS forward + backward passes of the README shape at hit rate 0.9, cached and uncached, and nothing else.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from recsys_benchmark_amd import tt_cache  # noqa: E402
from recsys_benchmark_amd.embeddings import TTEmbedding, TTRecTorch  # noqa: E402

DEV = "cuda:0"
NBATCH, TRACE_CALLS = 16, 10
RATES = (0.0, 0.5, 0.9, 0.99)
SHAPES = {
    "criteo39_D16_r128_96": dict(N=1086810, D=16, ranks=[128, 96], lookups=(4096, 39)),
    "gowalla_items_D64_r96_80": dict(N=40981, D=64, ranks=[96, 80], lookups=(8192, 1)),
}


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
        per_call_us(fn, min(n, 3))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(per_call_us(fn, n))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                "rounds_us": [round(t, 2) for t in v]} for k, v in times.items()}


def condition(res, new, other):
    gap = res[other]["median_us"] - res[new]["median_us"]
    spread = max(res[other]["spread_us"], res[new]["spread_us"])
    return {"new": new, "other": other, "gap_us": round(gap, 2), "spread_us": spread,
            "ratio": round(res[other]["median_us"] / res[new]["median_us"], 3),
            "verdict": "faster" if gap > spread else ("slower" if gap < -spread else "tie")}


def zipf_batches(N, shape, seed, a=1.1):
    gen = torch.Generator().manual_seed(seed)
    w = 1.0 / torch.arange(1, N + 1, dtype=torch.float64) ** a
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(99))
    n = shape[0] * shape[1]
    return [perm[torch.multinomial(w, n, replacement=True, generator=gen)].view(shape).to(DEV) for _ in range(NBATCH)]


def cache_size_for(batches, rate):
    counts = torch.cat([b.flatten() for b in batches]).unique(return_counts=True)[1].sort(descending=True)[0]
    share = counts.cumsum(0).double() / counts.sum()
    return int((share < rate).sum()) + 1


def tables(cfg, batches, rate):
    """(cached table populated for `rate` — in warmup for rate 0 —, the uncached reference on the same cores, achieved rate)."""
    np.random.seed(0)
    ref = TTRecTorch(cfg["N"], cfg["D"], cfg["ranks"], weight_dist="normal").to(DEV)
    C = cache_size_for(batches, rate) if rate > 0 else 1
    np.random.seed(0)
    emb = TTEmbedding(cfg["N"], cfg["D"], tt_ranks=cfg["ranks"], weight_dist="normal", use_cache=True, cache_size=C).to(DEV)
    with torch.no_grad():
        for c, r in zip(emb._tt_emb.tt_cores, ref.tt_cores):
            c.copy_(r)
        for b in batches:
            emb(b)
        if rate > 0:
            emb.cache_populate()
        bag = emb._tt_emb
        loc = tt_cache.probe_count(batches[0], bag.hashtbl, bag.cache_freq, bag.cache_state, cfg["N"], C, bag._warm)
        achieved = float((loc >= 0).float().mean())
    return emb, ref, C, achieved


def fwd(emb, batches):
    def run(i):
        with torch.no_grad():
            return emb(batches[i % NBATCH])
    return run


def fwd_bwd(emb, batches, G):
    def run(i):
        emb.zero_grad(set_to_none=True)
        (emb(batches[i % NBATCH]) * G).sum().backward()
    return run


def leg_h(cfg, rounds, calls):
    batches = zipf_batches(cfg["N"], cfg["lookups"], 1)
    G = torch.randn(*batches[0].shape, cfg["D"], device=DEV)
    out = {}
    for rate in RATES:
        emb, ref, C, achieved = tables(cfg, batches, rate)
        f = rounds_of({"tt_emb": fwd(emb, batches), "tt_emb_torch": fwd(ref, batches)}, calls, rounds)
        fb = rounds_of({"tt_emb": fwd_bwd(emb, batches, G), "tt_emb_torch": fwd_bwd(ref, batches, G)}, calls, rounds)
        with torch.no_grad():
            pop = rounds_of({"cache_populate": lambda i: emb.cache_populate()}, 3, rounds) if rate > 0 else None
        out[f"hit{rate}"] = {"cache_size": C, "achieved_hit_rate": round(achieved, 4), "forward": f,
                             "forward_condition": condition(f, "tt_emb", "tt_emb_torch"), "forward_backward": fb,
                             "forward_backward_condition": condition(fb, "tt_emb", "tt_emb_torch"), "c_cache_populate": pop,
                             "calls_per_round": calls}
        del emb, ref
        torch.cuda.empty_cache()
    return out


def leg_p(cfg, rounds):
    B, F = 4096, 39
    gen = torch.Generator().manual_seed(2)
    uniform = [torch.randint(0, cfg["N"], (B, F), generator=gen).to(DEV) for _ in range(NBATCH)]
    one_hot = [b.clone() for b in uniform]
    for b in one_hot:
        b[:, 0] = 12345
    emb = TTEmbedding(cfg["N"], cfg["D"], tt_ranks=cfg["ranks"], weight_dist="normal", use_cache=True).to(DEV)
    bag = emb._tt_emb
    C = bag.cache_weight.shape[0]

    def probe(batches):
        return lambda i: tt_cache.probe_count(batches[i % NBATCH], bag.hashtbl, bag.cache_freq, bag.cache_state, cfg["N"], C,
                                              bag._warm)
    res = rounds_of({"uniform": probe(uniform), "one_id_fills_field_0": probe(one_hot)}, 50, rounds)
    res["condition_one_hot_vs_uniform"] = condition(res, "one_id_fills_field_0", "uniform")
    res["lookups"] = B * F
    res["count_of_the_hot_id"] = int(bag.cache_freq[12345])
    return res


def leg_t():
    cfg = SHAPES["criteo39_D16_r128_96"]
    batches = zipf_batches(cfg["N"], cfg["lookups"], 1)
    G = torch.randn(*batches[0].shape, cfg["D"], device=DEV)
    emb, ref, _, _ = tables(cfg, batches, 0.9)
    for t in (emb, ref):
        run = fwd_bwd(t, batches, G)
        for i in range(TRACE_CALLS):
            run(i)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="hp")
    args = ap.parse_args()
    if "t" in args.legs:
        leg_t()
        return
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "batches": NBATCH, "shapes": {}}
    for name, cfg in SHAPES.items():
        res["shapes"][name] = {"N": cfg["N"], "D": cfg["D"], "ranks": cfg["ranks"], "lookups": cfg["lookups"][0] * cfg["lookups"][1]}
        if "h" in args.legs:
            res["shapes"][name]["h_hit_rates"] = leg_h(cfg, args.rounds, 8)
            print(name, "h done", flush=True)
    if "p" in args.legs:
        res["p_probe_count"] = leg_p(SHAPES["criteo39_D16_r128_96"], args.rounds)
        print("p done", flush=True)
    pkg.check_index_errors()
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

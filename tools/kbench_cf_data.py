"""Device-resident CF data (cf_data.py, csrc/cf_data.hip) against the host path it replaces, at the Yelp2018 shape
(31 668 users, 38 048 items, 1 128 375 interactions drawn with a skewed item popularity; duplicates kept):

  sample_*   one epoch's triples from ONE mi_cf_sample_triples launch (uniform sampling, K = 1 and K = 5; popularity
             sampling, K = 1), device-event time around `calls` back-to-back launches;
  host_sampler_*  the same epoch from a Python map-style dataset with the same semantics (a uniform entry of the user's
             stored list, negatives uniform over the items outside the user's set and pairwise distinct; written for
             this tool with Python's `random`, the way a per-sample `__getitem__` does it) behind a
             torch DataLoader with batch 2048 and num_workers 4 (the reference's config), wall clock around one whole
             iteration, the batches moved to the device as `_run_epoch` moves them;
  metric_*   NDCG / recall at 20 over all users: mi_ndcg_recall_rows (plus the two means) against `ndcg_recall_at_k`
             on the same predictions and the same truth as Python sets;
  epoch_*    one whole `train_epoch_cf` epoch of a LightGCN (D = 64, L = 3, batch 2048, the library's Adam, captured
             step) fed by a DeviceCFLoader and fed by that host DataLoader, wall clock to a device synchronise.

The legs alternate in rounds inside one process; every figure is the median over the rounds, `spread` is
(max - min) / median.  Prints one JSON line and writes it to --out.

    python tools/kbench_cf_data.py [--rounds 3] [--calls 20] [--out profiles/cf_data_kbench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from recsys_benchmark_amd import trainer  # noqa: E402
from recsys_benchmark_amd.optim import Adam  # noqa: E402

DEV = "cuda:0"
U, I, NNZ = 31668, 38048, 1128375
BATCH, WORKERS = 2048, 4


def yelp_graphs(seed=2023):
    """(train, test) graph dicts: every user present in both, item popularity skewed as tools/kbench2.yelp_graph skews it."""
    rng = np.random.default_rng(seed)

    def draw(nnz):
        users = np.concatenate([np.arange(U), rng.integers(0, U, nnz - U)])
        items = np.minimum((I * rng.random(nnz) ** 2).astype(np.int64), I - 1)
        items[0] = I - 1
        by = np.argsort(users, kind="stable")
        cuts = np.flatnonzero(np.diff(users[by])) + 1
        return {u: its.tolist() for u, its in enumerate(np.split(items[by], cuts))}

    return draw(NNZ), draw(NNZ // 4)


class HostTriples(torch.utils.data.Dataset):
    """The host counterpart: one Python `__getitem__` per sample."""

    def __init__(self, graph, num_items, num_neg):
        self.graph, self.sets = graph, {u: set(v) for u, v in graph.items()}
        self.num_items, self.num_neg = num_items, num_neg
        self.per_user = sum(len(v) for v in graph.values()) // len(graph)

    def __len__(self):
        return len(self.graph) * self.per_user

    def __getitem__(self, idx):
        user = idx // self.per_user
        positive = random.choice(self.graph[user])
        taken, negatives = self.sets[user], []
        while len(negatives) < self.num_neg:
            item = random.randrange(self.num_items)
            if item not in taken and item not in negatives:
                negatives.append(item)
        return user, positive, (negatives[0] if self.num_neg == 1 else negatives)


class _HostLoader:
    """A DataLoader with the `.dataset.get_norm_adj()` the CF trainers ask their loader for."""

    def __init__(self, loader, data):
        self.loader, self.dataset = loader, data

    def __iter__(self):
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)


def device_time(fn, calls):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # us


def wall_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6          # us


def summarise(xs):
    med = statistics.median(xs)
    return {"median_us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 3), "rounds": [round(x, 2) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "cf_data_kbench.json"))
    ap.add_argument("--no-host", action="store_true", help="skip the host legs (for a rocprofv3 run of the kernels)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_cf_data.py measures on an MI355X; no ROCm device found")
    train, test = yelp_graphs()
    out = {"device": torch.cuda.get_device_name(0), "users": U, "items": I, "interactions": NNZ, "batch": BATCH,
           "num_workers": WORKERS, "rounds": args.rounds, "calls": args.calls}

    # ---- sampling ------------------------------------------------------------------------------------------------------
    legs = {}
    for mode, K in (("uniform", 1), ("uniform", 5), ("popularity", 1)):
        ds = pkg.DeviceCFGraphDataset(train, sampling_method=mode, num_neg_item=K, device=DEV)
        n = len(ds)
        epoch = [0]

        def launch(ds=ds, n=n, epoch=epoch):
            epoch[0] += 1
            return ds.sample(0, n, epoch[0], 7)

        legs[f"sample_{mode}_k{K}"] = (launch, n, K)
    times = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, (fn, n, K) in legs.items():
            times[name].append(device_time(fn, args.calls))
    pkg.check_index_errors()
    for name, (fn, n, K) in legs.items():
        s = summarise(times[name])
        out[name] = dict(s, samples=n, triples_per_s=round(n / (s["median_us"] * 1e-6)),
                         bytes_written=8 * n * (2 + K), write_GBps=round(8 * n * (2 + K) / (s["median_us"] * 1e-6) / 1e9, 1))
    if not args.no_host:
        for K in (1, 5):
            host = HostTriples(train, I, K)
            loader = torch.utils.data.DataLoader(host, batch_size=BATCH, shuffle=True, num_workers=WORKERS)

            def drain(loader=loader):
                for batch in loader:
                    [[t.to(DEV, non_blocking=True) for t in p] if isinstance(p, (list, tuple)) else p.to(DEV, non_blocking=True)
                     for p in batch]

            s = summarise([wall_time(drain) for _ in range(args.rounds)])
            out[f"host_sampler_k{K}"] = dict(s, samples=len(host), triples_per_s=round(len(host) / (s["median_us"] * 1e-6)))
            out[f"host_over_device_sampling_k{K}"] = round(s["median_us"] / out[f"sample_uniform_k{K}"]["median_us"], 1)

    # ---- metric ----------------------------------------------------------------------------------------------------------
    k = 20
    tds = pkg.DeviceCFTestDataset(test, device=DEV)
    torch.manual_seed(0)
    scores = torch.rand(U, 4096, device=DEV)
    pred = (torch.topk(scores, k)[1] * 9 % I).contiguous()          # distinct item ids per row (9 and I are coprime)
    del scores
    users = tds.users
    sets = [set(test[u]) for u in users.tolist()]
    dev_metric = lambda: tds.truth.ndcg_recall(pred, users, k)       # noqa: E731  (kernel + two means + two .item())
    got = dev_metric()
    t_dev, t_host = [], []
    if not args.no_host:
        want = trainer.ndcg_recall_at_k(pred, sets, k)
        out["metric_abs_diff"] = [abs(got[0] - want[0]), abs(got[1] - want[1])]
    for _ in range(args.rounds):
        t_dev.append(device_time(dev_metric, args.calls))
        if not args.no_host:
            t_host.append(wall_time(lambda: trainer.ndcg_recall_at_k(pred, sets, k)))
    out["metric_device"] = dict(summarise(t_dev), users=U, k=k, truth_items=int(tds.truth.col.numel()), ndcg=got[0], recall=got[1])
    if not args.no_host:
        out["metric_host"] = summarise(t_host)
        out["host_over_device_metric"] = round(out["metric_host"]["median_us"] / out["metric_device"]["median_us"], 1)

    # ---- one training epoch fed each way -----------------------------------------------------------------------------------
    ds = pkg.DeviceCFGraphDataset(train, device=DEV)
    adj = ds.get_norm_adj().to(DEV)

    def epoch_runner(loader):
        torch.manual_seed(0)
        model = pkg.LightGCN(U, I, num_layers=3, hidden_size=64).to(DEV)
        step = trainer.GraphedCFTrainStep(model, adj, Adam(model.parameters(), lr=1e-3), 1e-4)
        return lambda: trainer.train_epoch_cf(loader, model, None, device=DEV, log_step=100, step=step)

    feeds = {"epoch_device_fed": epoch_runner(pkg.DeviceCFLoader(ds, BATCH, shuffle=True, seed=7))}
    if not args.no_host:
        host = torch.utils.data.DataLoader(HostTriples(train, I, 1), batch_size=BATCH, shuffle=True, num_workers=WORKERS)
        feeds["epoch_host_fed"] = epoch_runner(_HostLoader(host, ds))
    losses = {name: fn() for name, fn in feeds.items()}             # warm-up epoch: capture, code objects, workers
    times = {name: [] for name in feeds}
    for _ in range(args.rounds):
        for name, fn in feeds.items():
            times[name].append(wall_time(fn))
    steps = -(-len(ds) // BATCH)
    for name in feeds:
        s = summarise(times[name])
        out[name] = dict(s, steps=steps, us_per_step=round(s["median_us"] / steps, 1), first_epoch_loss=losses[name]["loss"])
    if not args.no_host:
        out["host_over_device_epoch"] = round(out["epoch_host_fed"]["median_us"] / out["epoch_device_fed"]["median_us"], 2)
    pkg.check_index_errors()

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""The Adagrad steps (optim.SparseAdagrad, optim.RowwiseAdagrad, optim.Adagrad: csrc/adagrad.hip) next to the Adam steps
they share a walker with and next to torch.optim.Adagrad, at the headline shape (B = 4096 x F = 26 Criteo fields, D = 16)
and on the first-order table (D = 1).

  sparse_D16 / sparse_D1   one optimizer step on a row-form gradient of B*F rows (ids with the lookup's field layout, so the
                           sort is the LDS field sort for every own leg), per leg a table of its own:
      SparseAdagrad, RowwiseAdagrad, SparseAdam (capturable, as get_optimizers builds it) — same ids, same values;
      torch_Adagrad_sparse_coo — torch.optim.Adagrad fed the same gradient as a torch.sparse_coo_tensor on the same GPU
      (the baseline: coalesce + its sparse tensor ops);
  dense_mlp                optim.Adagrad against torch.optim.Adagrad on the headline MLP's parameters (dense gradients);
  train_step               one captured DeepFM training step (both tables row-form, packed) per optimizer pair;
  state_bytes              torch.cuda.memory_allocated of the optimizer state alone for the three sparse rules at D = 16.

The legs of a group alternate in rounds inside one process; every figure is the median over 7 rounds of `--iters` steps
timed by device events, `spread_us` is max - min over the rounds.  Prints one JSON line and writes it to --out.

    python tools/kbench_adagrad.py [--rounds 7] [--iters 20] [--batch 4096]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import recsys_benchmark_amd as pkg  # noqa: E402
from recsys_benchmark_amd import _kernels, optim as rbo, trainer  # noqa: E402
from bench import CRITEO_KAGGLE_26, synth_batch  # noqa: E402

DEV = torch.device("cuda", 0)


def timed_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def alternate(legs, rounds, iters):
    """{name: {median_us, spread_us, rounds_us}}: the legs take turns, one timed burst each per round."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            seen[k].append(timed_us(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                "rounds_us": [round(t, 2) for t in v]} for k, v in seen.items()}


def sparse_group(rows2d, offs, N, D, rounds, iters):
    rows = rows2d.reshape(-1)
    vals = torch.randn(rows.numel(), D, device=DEV) * 1e-3
    _kernels.note_field_layout(rows2d, offs, N)            # what the multi-field lookup does for its ids
    makers = {"SparseAdagrad": lambda p: rbo.SparseAdagrad([p], lr=1e-2),
              "RowwiseAdagrad": lambda p: rbo.RowwiseAdagrad([p], lr=1e-2),
              "SparseAdam": lambda p: rbo.SparseAdam([p], lr=1e-3, capturable=True),
              "torch_Adagrad_sparse_coo": lambda p: torch.optim.Adagrad([p], lr=1e-2)}
    legs, keep, state_bytes = {}, [], {}
    for name, make in makers.items():
        p = torch.nn.Parameter(torch.zeros(N, D, device=DEV))
        p.grad = torch.sparse_coo_tensor(rows.unsqueeze(0), vals, (N, D), check_invariants=False)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(DEV)
        opt = make(p)
        opt.step()                                         # (lazily created state comes into being; scratch too: see below)
        torch.cuda.synchronize()
        scratch = sum(t.numel() * t.element_size() for t in getattr(opt, "_workspace", {}).values())
        state_bytes[name] = {"allocated": torch.cuda.memory_allocated(DEV) - before - scratch,
                             "state_tensors": sum(t.numel() * t.element_size() for st in opt.state.values()
                                                  for t in st.values() if torch.is_tensor(t) and t.is_cuda)}
        legs[name] = opt.step
        keep.append((p, opt))
    out = alternate(legs, rounds, iters)
    out["rows"], out["distinct_rows"] = rows.numel(), int(torch.unique(rows).numel())
    del legs, keep
    torch.cuda.empty_cache()
    return out, state_bytes


def dense_group(hidden, in_features, rounds, iters):
    shapes = []
    for a, b in zip([in_features] + hidden[:-1], hidden):
        shapes += [(b, a), (b,), (b,), (b,)]               # weight, bias, BatchNorm weight and bias
    shapes += [(1, hidden[-1]), (1,)]
    legs, keep = {}, []
    for name, cls in (("Adagrad", rbo.Adagrad), ("torch_Adagrad", torch.optim.Adagrad)):
        params = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in shapes]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        opt = cls(params, lr=1e-2, weight_decay=1e-6)
        legs[name] = opt.step
        keep.append((params, opt))
    out = alternate(legs, rounds, iters)
    out["tensors"], out["elements"] = len(shapes), sum(int(torch.Size(s).numel()) for s in shapes)
    return out


def train_group(dims, D, hidden, B, rounds, iters):
    x, y = synth_batch(dims, B, 7, DEV)
    legs, keep = {}, []
    for name in ("adam", "adagrad", "rowwise_adagrad"):
        torch.manual_seed(0)
        with torch.device(DEV):
            model = pkg.DeepFM(dims, D, hidden, p_dropout=0.0, use_batchnorm=True,
                               embedding_config={"name": "vanilla", "sparse": True}, fc_sparse=True)
        model.pack_tables()
        model.train()
        opts = rbo.get_optimizers(model, {"optimizer": name, "sparse": True, "learning_rate": 1e-3, "weight_decay": 1e-6})
        step = trainer.GraphedTrainStep(model, opts)
        for _ in range(4):
            step(x, y)
        assert step._graph is not None, f"{name}: the training step was not captured"
        legs[name] = lambda step=step: step(x, y)
        keep.append((model, opts, step))
    return alternate(legs, rounds, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--no-train", action="store_true", help="skip the captured training steps (three 2 GB models)")
    ap.add_argument("--out", default=os.path.join("profiles", "adagrad_kbench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_adagrad.py measures on an MI355X; no ROCm device found")
    dims, hidden = list(CRITEO_KAGGLE_26), [400, 400, 400]
    N = sum(dims)
    x, _ = synth_batch(dims, args.batch, 1, DEV)
    offs = torch.tensor([0] + dims[:-1], device=DEV).cumsum(0)
    rows2d = x + offs
    out = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "fields": len(dims), "table_rows": N,
           "rounds": args.rounds, "iters": args.iters}
    out["sparse_D16"], out["state_bytes_D16"] = sparse_group(rows2d, offs, N, 16, args.rounds, args.iters)
    out["sparse_D1"], _ = sparse_group(rows2d, offs, N, 1, args.rounds, args.iters)
    out["dense_mlp"] = dense_group(hidden, len(dims) * 16, args.rounds, args.iters)
    if not args.no_train:
        out["train_step"] = train_group(dims, 16, hidden, args.batch, args.rounds, args.iters)
    pkg.check_index_errors()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

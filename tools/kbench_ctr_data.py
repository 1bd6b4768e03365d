"""Device-resident CTR data (ctr_data.py, csrc/ctr_data.hip) against the host path it replaces, at a Criteo-like
synthetic shape: F = 39 (13 fields of 50 ids in front of the 26 Criteo-Kaggle cardinalities), `--rows` records
(default 2^21) whose ids are drawn with a skew inside every field, already encoded as uint32 [rows, 40]:

  batch_*     ONE mi_ctr_batch call at B = 4096 into the caller's buffers, shuffled and in order, device-event time
              around `calls` back-to-back launches; bytes moved (4 (1 + F) read + 8 F + 4 written per sample) over that
              time as a share of the 8.0 TB/s HBM peak.  The same call at B = 256 and B = 65536 says whether the
              B = 4096 call is launch-bound (its time is then the small batch's, not 16 times it);
  epoch_*     one whole `train_epoch` of a DeepFM (D = 16, MLP 400 x 3, BatchNorm, row-sparse Adam, captured step) fed
              by a DeviceCTRLoader and fed by the same records in a map-style dataset (the reference's `__getitem__` /
              `__getitems__`) behind DataLoader(batch 4096, num_workers 4, shuffle), wall clock to a device synchronise;
  validate_*  one `validate_epoch` each way over the first `--val-rows` records, in order;
  encode_*    `encode_ctr_columns` of one column of `rows` keys (copy to the device, stable sort, the three launches
              of mi_ctr_vocab_field, the count read back) against the same rule through numpy.unique on the host.

The legs of a pair alternate in rounds inside one process; every figure is the median over the rounds, `spread` is
(max - min) / median.  Prints one JSON line and writes it to --out.

    python tools/kbench_ctr_data.py [--rounds 3] [--calls 200] [--rows 2097152] [--out profiles/ctr_data_kbench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from bench import CRITEO_KAGGLE_26  # noqa: E402
from recsys_benchmark_amd import optim, trainer  # noqa: E402

DEV = "cuda:0"
DIMS = [50] * 13 + list(CRITEO_KAGGLE_26)
F = len(DIMS)
BATCH, WORKERS = 4096, 4
HBM_PEAK = 8.0e12          # bytes / s


def synth_records(rows, seed=2023):
    """uint32 [rows, 1 + F]: label ~ Bernoulli(0.25), field f's id = dims[f] * u^2 (a skew towards the small ids)."""
    rng = np.random.default_rng(seed)
    records = np.zeros((rows, 1 + F), dtype=np.uint32)
    records[:, 0] = rng.random(rows) < 0.25
    for f, d in enumerate(DIMS):
        records[:, 1 + f] = np.minimum((d * rng.random(rows) ** 2).astype(np.int64), d - 1)
    return records


class HostRecords(torch.utils.data.Dataset):
    """The host counterpart: the reference's `__getitem__` / `__getitems__` over the same records in host memory (the
    LMDB lookup replaced by an array read, which only makes the host path cheaper)."""

    def __init__(self, records):
        self.records = records

    def __len__(self):
        return self.records.shape[0]

    def __getitem__(self, index):
        row = self.records[index].astype(np.int64)
        return row[1:], row[0]

    def __getitems__(self, indices):
        array = self.records[indices].astype(np.int64)          # (the reference hands int32 over; the models here take int64)
        return [(arr[1:], arr[0]) for arr in array]


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


def alternate(legs, rounds, timer):
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(timer(fn))
    return {name: summarise(xs) for name, xs in times.items()}


def host_vocab(column, threshold):
    uniq, inverse, counts = np.unique(column, return_inverse=True, return_counts=True)
    kept = counts >= threshold
    ids = np.where(kept, np.cumsum(kept) - 1, kept.sum()).astype(np.uint32)
    return ids[inverse.reshape(-1)], int(kept.sum()) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--val-rows", type=int, default=1 << 19)
    ap.add_argument("--out", default=os.path.join("profiles", "ctr_data_kbench.json"))
    ap.add_argument("--no-host", action="store_true", help="skip the host legs (for a rocprofv3 run of the kernels)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_ctr_data.py measures on an MI355X; no ROCm device found")
    rows = args.rows
    records = synth_records(rows)
    ds = pkg.DeviceCTRDataset(records, DIMS, device=DEV)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "fields": F, "sum_field_dims": int(sum(DIMS)),
           "batch": BATCH, "num_workers": WORKERS, "rounds": args.rounds, "calls": args.calls,
           "resident_bytes": int(ds.records.numel() * 4)}

    # ---- one batch launch ------------------------------------------------------------------------------------------------
    shuffled, in_order = pkg.DeviceCTRLoader(ds, BATCH, shuffle=True, seed=7), pkg.DeviceCTRLoader(ds, BATCH, seed=7)
    legs, state = {}, {"i": 0}
    for B in (256, BATCH, 65536):
        bufs = (torch.zeros((B, F), dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.float32, device=DEV))
        for name, loader in (("shuffled", shuffled), ("in_order", in_order)):

            def call(loader=loader, B=B, bufs=bufs):
                state["i"] += 1
                return loader.batch((state["i"] * B) % (rows - B + 1), B, state["i"] & 7, out=bufs)

            legs[f"batch_{name}_b{B}"] = call
    legs["batch_shuffled_fresh_b4096"] = lambda: shuffled.batch(0, BATCH, 3)          # with the two fill launches of `out=None`
    for name, s in alternate(legs, args.rounds, lambda fn: device_time(fn, args.calls)).items():
        B = int(name.rsplit("_b", 1)[1])
        moved = B * (4 * (1 + F) + 8 * F + 4)
        out[name] = dict(s, bytes_moved=moved, GBps=round(moved / (s["median_us"] * 1e-6) / 1e9, 1),
                         share_of_hbm_peak=round(moved / (s["median_us"] * 1e-6) / HBM_PEAK, 4))
    small, mid = out["batch_shuffled_b256"]["median_us"], out[f"batch_shuffled_b{BATCH}"]["median_us"]
    out["batch_b4096_launch_bound"] = bool(mid < 2.0 * small)
    out["batch_b4096_over_b256"] = round(mid / small, 2)
    pkg.check_index_errors()

    # ---- one column through the vocabulary rule ----------------------------------------------------------------------------
    rng = np.random.default_rng(5)
    column = np.minimum((DIMS[15] * rng.random(rows) ** 2).astype(np.int64), DIMS[15] - 1) * 2654435761 - (1 << 40)
    labels = np.zeros(rows, dtype=np.uint8)
    enc, dims = pkg.encode_ctr_columns(column.reshape(-1, 1), labels, 10, device=DEV)
    want, want_dim = host_vocab(column, 10)
    out["encode_matches_host"] = bool(int(dims[0]) == want_dim
                                      and np.array_equal(enc.view(torch.int32)[:, 1].cpu().numpy().view(np.uint32), want))
    legs = {"encode_device": lambda: pkg.encode_ctr_columns(column.reshape(-1, 1), labels, 10, device=DEV)}
    if not args.no_host:
        legs["encode_host"] = lambda: host_vocab(column, 10)
    out.update(dict(alternate(legs, args.rounds, wall_time), encode_keys=rows, encode_field_dim=int(dims[0])))
    if not args.no_host:
        out["host_over_device_encode"] = round(out["encode_host"]["median_us"] / out["encode_device"]["median_us"], 2)
    del enc

    # ---- one training epoch and one validation fed each way --------------------------------------------------------------
    torch.manual_seed(0)
    model = pkg.DeepFM(DIMS, 16, [400, 400, 400], p_dropout=0.5, use_batchnorm=True,
                       embedding_config={"name": "vanilla", "sparse": True}, fc_sparse=True).to(DEV)
    opts = optim.get_optimizers(model, {"optimizer": "adam", "learning_rate": 1e-3, "weight_decay": 1e-6, "sparse": True})
    step = trainer.GraphedTrainStep(model, opts)
    host = HostRecords(records)
    feeds = {"epoch_device_fed": pkg.DeviceCTRLoader(ds, BATCH, shuffle=True, seed=7)}
    val_rows = min(args.val_rows, rows)
    val_ds = ds.subset(torch.arange(val_rows, device=DEV))
    vals = {"validate_device_fed": pkg.DeviceCTRLoader(val_ds, BATCH)}
    if not args.no_host:
        feeds["epoch_host_fed"] = torch.utils.data.DataLoader(host, batch_size=BATCH, shuffle=True, num_workers=WORKERS)
        vals["validate_host_fed"] = torch.utils.data.DataLoader(torch.utils.data.Subset(host, range(val_rows)),
                                                                batch_size=BATCH, num_workers=WORKERS)
    train = {name: (lambda loader=loader: trainer.train_epoch(loader, model, opts, device=DEV, log_step=100, step=step))
             for name, loader in feeds.items()}
    losses = {name: fn()["loss"] for name, fn in train.items()}            # warm-up epoch: capture, code objects, workers
    steps = -(-rows // BATCH)
    for name, s in alternate(train, args.rounds, wall_time).items():
        out[name] = dict(s, steps=steps, us_per_step=round(s["median_us"] / steps, 1), first_epoch_loss=losses[name])
    forward, metric = trainer.GraphedForward(model), pkg.CTRMetric(DEV, capacity=val_rows)
    validate = {name: (lambda loader=loader: trainer.validate_epoch(loader, model, device=DEV, forward=forward, metric=metric))
                for name, loader in vals.items()}
    figures = {name: fn() for name, fn in validate.items()}                 # warm-up, and the two feeds must agree
    for name, s in alternate(validate, args.rounds, wall_time).items():
        out[name] = dict(s, rows=val_rows, steps=-(-val_rows // BATCH), **figures[name])
    if not args.no_host:
        out["host_over_device_epoch"] = round(out["epoch_host_fed"]["median_us"] / out["epoch_device_fed"]["median_us"], 2)
        out["host_over_device_validate"] = round(out["validate_host_fed"]["median_us"]
                                                 / out["validate_device_fed"]["median_us"], 2)
        out["validate_abs_diff"] = {k: abs(figures["validate_device_fed"][k] - figures["validate_host_fed"][k])
                                    for k in ("auc", "log_loss")}
    pkg.check_index_errors()

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

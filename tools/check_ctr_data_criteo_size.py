"""Criteo-size check of the device-resident CTR data (45 840 617 records, F = 39, 7.3 GB resident): `encode_ctr_columns`
of one column against numpy.unique's rule (tests/ctr_data_helpers.py), one shuffled batch against the restated p(j), and a
whole shuffled epoch in chunks of 2^20 samples serving every row exactly once.  Single runs, wall clock to a device
synchronise (no rounds, no spread: a check with times attached, not a benchmark).  Prints JSON lines and writes the last one
to profiles/ctr_data_criteo_size.json (or to the path given as the first argument).

    python tools/check_ctr_data_criteo_size.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctr_data_helpers as ch  # noqa: E402
import recsys_benchmark_amd as pkg  # noqa: E402

DEV = "cuda:0"
N, F = 45_840_617, 39
if not torch.cuda.is_available():
    sys.exit("check_ctr_data_criteo_size.py runs on an MI355X; no ROCm device found")
out = {"rows": N}

rng = np.random.default_rng(1)
column = np.minimum((10131227 * rng.random(N) ** 2).astype(np.int64), 10131226) * 2654435761 - (1 << 40)
labels = np.zeros(N, dtype=np.uint8)
t = time.perf_counter()
want_rec, want_dims = ch.encode_restated(column.reshape(-1, 1), labels, 10)
out["encode_host_s"] = time.perf_counter() - t
for r in range(3):
    torch.cuda.synchronize()
    t = time.perf_counter()
    rec, dims = pkg.encode_ctr_columns(column.reshape(-1, 1), labels, 10, device=DEV)
    torch.cuda.synchronize()
    out.setdefault("encode_device_s", []).append(time.perf_counter() - t)
got = rec.view(torch.int32).cpu().numpy().view(np.uint32)
out["encode_equal"] = bool(np.array_equal(got, want_rec) and np.array_equal(dims, want_dims))
out["encode_field_dim"] = int(dims[0])
# the device part alone (column already resident): sort + three launches
col_dev = torch.from_numpy(column).to(DEV)
torch.cuda.synchronize()
t = time.perf_counter()
s, p = torch.sort(col_dev, stable=True)
torch.cuda.synchronize()
out["sort_s"] = time.perf_counter() - t
del rec, got, want_rec, col_dev, s, p
pkg.check_index_errors()
print(json.dumps(out), flush=True)

# records made on the device: field 0 holds the row number
records = torch.randint(0, 1000, (N, 1 + F), dtype=torch.int32, device=DEV)
records[:, 0] = torch.randint(0, 2, (N,), dtype=torch.int32, device=DEV)
records[:, 1] = torch.arange(N, dtype=torch.int32, device=DEV)
ds = pkg.DeviceCTRDataset(records, [N] + [1000] * (F - 1), device=DEV)
loader = pkg.DeviceCTRLoader(ds, 4096, shuffle=True, seed=11)
first = N - 5000
x, y = loader.batch(first, 4096, 2)
want_rows = ch.p_restated(first + np.arange(4096), N, 11, 2)
out["batch_rows_equal"] = bool(np.array_equal(x[:, 0].cpu().numpy(), want_rows))
host_rows = records[torch.from_numpy(want_rows).to(DEV)].cpu().numpy()
out["batch_equal"] = bool(np.array_equal(x.cpu().numpy(), host_rows[:, 1:].astype(np.int64))
                          and np.array_equal(y.cpu().numpy(), host_rows[:, 0].astype(np.float32)))
# a whole shuffled epoch in chunks of 2^20 samples: every row exactly once
seen = torch.zeros(N, dtype=torch.int32, device=DEV)
chunk = 1 << 20
bx = torch.zeros((chunk, F), dtype=torch.int64, device=DEV)
by = torch.zeros(chunk, dtype=torch.float32, device=DEV)
torch.cuda.synchronize()
t = time.perf_counter()
for s0 in range(0, N, chunk):
    c = min(chunk, N - s0)
    xx, _ = loader.batch(s0, c, 2, out=(bx[:c], by[:c]))
    seen.index_add_(0, xx[:, 0], torch.ones(c, dtype=torch.int32, device=DEV))
torch.cuda.synchronize()
out["epoch_cover_s"] = time.perf_counter() - t
out["epoch_every_row_once"] = bool((seen == 1).all())
pkg.check_index_errors()
print(json.dumps(out), flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ctr_data_criteo_size.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    f.write(json.dumps(out) + "\n")

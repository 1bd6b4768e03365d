"""The device text reader (ctr_data.parse_criteo_text, csrc/ctr_text.hip) against the host reader it stands beside
(`read_criteo_text`, a Python loop over the lines), on seeded synthetic Criteo-format text: `--lines` lines (default 2^21)
drawn from a pool of 4096 distinct lines whose fields come, column by column, from tests/golden/criteo_sample.txt (so the
field lengths and the share of empty fields are the sample's), with half of the integer fields redrawn at the same number
of digits and 3 % of them made negative.

  parse_path      parse_criteo_text from the file (written once, read once before timing: it is in the page cache);
  parse_resident  parse_criteo_text from a uint8 tensor already on the device;
  dataset_device  DeviceCTRDataset.from_criteo_text(path, reader="device"), min_threshold 10, end to end;
  read_host       read_criteo_text on the first `--host-fraction` of the lines (a file of its own), and
  dataset_host    from_criteo_text(reader="host") on that fraction; both are reported as measured AND scaled by
                  1 / fraction (the host reader is a loop over the lines: its time is proportional to them).

The legs alternate in rounds inside one process; every figure is the median over the rounds, `spread` is (max - min) /
median, wall clock to a device synchronise.  Lines/s and bytes of text per second come from those medians.  The
`tracemalloc` peak of each reader is taken in one untimed pass of its own (tracing slows Python down).  The two readers'
results are compared at the host's timed size, the device reader's two sources at the full size.  Prints one JSON line and
writes it to --out.

--criteo-size: the resident text tiled up to 45 840 617 lines, parsed three times, every run listed (single runs, no
median: the first takes its 14 GB of output blocks fresh from the driver, the others find them cached), line numbers and
every row checked against the tiling.

    python tools/kbench_ctr_text.py [--rounds 3] [--lines 2097152] [--host-fraction 0.125] [--criteo-size]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kbench_ctr_text.py --no-host --rounds 2
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import tracemalloc

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recsys_benchmark_amd as pkg  # noqa: E402

DEV = "cuda:0"
SAMPLE = os.path.join(ROOT, "tests", "golden", "criteo_sample.txt")
CRITEO_LINES = 45840617
POOL = 4096


def synth_text(lines, seed=2024):
    """(text bytes, the byte length of each of the POOL distinct lines, the pool index of every line)."""
    rng = np.random.default_rng(seed)
    columns = list(zip(*[line.split(b"\t") for line in open(SAMPLE, "rb").read().split(b"\n") if line.count(b"\t") == 39]))
    pool = []
    for _ in range(POOL):
        fields = []
        for c, values in enumerate(columns):
            s = values[int(rng.integers(0, len(values)))]
            if 1 <= c <= 13 and s:
                if rng.random() < 0.5:
                    s = b"%d" % int(rng.integers(10 ** (len(s) - 1) if len(s) > 1 else 0, 10 ** len(s)))
                if rng.random() < 0.03:
                    s = b"-%d" % int(rng.integers(0, 4))
            fields.append(s)
        pool.append(b"\t".join(fields) + b"\n")
    which = rng.integers(0, POOL, lines)
    return b"".join([pool[i] for i in which]), np.array([len(p) for p in pool]), which


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def alternate(legs, rounds):
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(wall(fn))
    out = {}
    for name, xs in times.items():
        med = statistics.median(xs)
        out[name] = {"median_s": round(med, 5), "spread": round((max(xs) - min(xs)) / med, 3), "rounds": [round(x, 5) for x in xs]}
    return out


def traced_peak(fn):
    tracemalloc.start()
    fn()
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lines", type=int, default=1 << 21)
    ap.add_argument("--host-fraction", type=float, default=0.125)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 28)
    ap.add_argument("--no-host", action="store_true", help="skip the host legs (for a rocprofv3 run of the kernels)")
    ap.add_argument("--criteo-size", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "ctr_text_kbench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_ctr_text.py measures on an MI355X; no ROCm device found")
    text, pool_len, which = synth_text(args.lines)
    host_lines = max(1, int(args.lines * args.host_fraction))
    host_bytes = int(pool_len[which[:host_lines]].sum())
    out = {"device": torch.cuda.get_device_name(0), "lines": args.lines, "text_bytes": len(text), "rounds": args.rounds,
           "chunk_bytes": args.chunk_bytes, "host_fraction": args.host_fraction, "host_lines": host_lines,
           "host_text_bytes": host_bytes, "distinct_lines": POOL}
    with tempfile.TemporaryDirectory() as tmp:
        path, host_path = os.path.join(tmp, "synthetic.txt"), os.path.join(tmp, "synthetic_fraction.txt")
        with open(path, "wb") as f:
            f.write(text)
        with open(host_path, "wb") as f:
            f.write(text[:host_bytes])
        open(path, "rb").read()
        resident = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV)
        chunk = args.chunk_bytes

        # ---- equal results ---------------------------------------------------------------------------------------------------
        from_path = pkg.parse_criteo_text(path, DEV, chunk_bytes=chunk)
        from_tensor = pkg.parse_criteo_text(resident, DEV, chunk_bytes=chunk)
        out["kept_lines"] = int(from_path[2].numel())
        out["sources_agree_at_full_size"] = all(torch.equal(a, b) for a, b in zip(from_path, from_tensor))
        if not args.no_host:
            want = pkg.read_criteo_text(host_path)
            got = pkg.parse_criteo_text(host_path, DEV, chunk_bytes=chunk)
            out["readers_agree_at_host_lines"] = all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))
            del want, got
        del from_path, from_tensor

        # ---- timed legs ------------------------------------------------------------------------------------------------------
        legs = {"parse_path": lambda: pkg.parse_criteo_text(path, DEV, chunk_bytes=chunk),
                "parse_resident": lambda: pkg.parse_criteo_text(resident, DEV, chunk_bytes=chunk),
                "dataset_device": lambda: pkg.DeviceCTRDataset.from_criteo_text(path, min_threshold=10, device=DEV, reader="device")}
        if not args.no_host:
            legs["read_host"] = lambda: pkg.read_criteo_text(host_path)
            legs["dataset_host"] = lambda: pkg.DeviceCTRDataset.from_criteo_text(host_path, min_threshold=10, device=DEV)
        legs["dataset_device"]()                                    # warm-up: the sort's and the encoder's code objects
        for name, s in alternate(legs, args.rounds).items():
            host_leg = name in ("read_host", "dataset_host")
            n, nbytes = (host_lines, host_bytes) if host_leg else (args.lines, len(text))
            out[name] = dict(s, lines=n, lines_per_s=round(n / s["median_s"]), text_MB_per_s=round(nbytes / s["median_s"] / 1e6, 1))
            if host_leg:
                out[name]["scaled_to_all_lines_s"] = round(s["median_s"] / args.host_fraction, 4)
        if not args.no_host:
            out["host_over_device_parse_path"] = round(out["read_host"]["scaled_to_all_lines_s"] / out["parse_path"]["median_s"], 1)
            out["host_over_device_parse_resident"] = round(out["read_host"]["scaled_to_all_lines_s"]
                                                           / out["parse_resident"]["median_s"], 1)
            out["host_over_device_dataset"] = round(out["dataset_host"]["scaled_to_all_lines_s"]
                                                    / out["dataset_device"]["median_s"], 1)
            out["device_reader_faster_end_to_end"] = bool(out["host_over_device_dataset"] > 1.0)

        # ---- host memory (one untimed pass each) -----------------------------------------------------------------------------
        out["tracemalloc_peak_bytes"] = {"parse_path_all_lines": traced_peak(legs["parse_path"])}
        if not args.no_host:
            out["tracemalloc_peak_bytes"]["read_host_at_host_lines"] = traced_peak(legs["read_host"])
        pkg.check_index_errors()

        # ---- Criteo's size, three single runs ---------------------------------------------------------------------------------------------
        if args.criteo_size:
            reps, rest = divmod(CRITEO_LINES, args.lines)
            big = torch.cat([resident.repeat(reps), resident[:int(pool_len[which[:rest]].sum())]])
            runs, keys, labels, line_no = [], None, None, None
            for _ in range(3):               # the first run takes 14 GB of fresh blocks from the driver, the others find them cached
                del keys, labels, line_no
                torch.cuda.synchronize()
                t = time.perf_counter()
                keys, labels, line_no = pkg.parse_criteo_text(big, DEV, chunk_bytes=chunk)
                torch.cuda.synchronize()
                runs.append(round(time.perf_counter() - t, 4))
            seconds = min(runs)
            first = pkg.parse_criteo_text(resident, DEV, chunk_bytes=chunk)
            n = args.lines
            ok = keys.shape[0] == CRITEO_LINES and bool((line_no == torch.arange(CRITEO_LINES, device=DEV)).all())
            for r in range(0, reps + 1):
                m = n if r < reps else rest
                ok = ok and torch.equal(keys[r * n:r * n + m], first[0][:m]) and torch.equal(labels[r * n:r * n + m], first[1][:m])
            out["criteo_size"] = {"lines": CRITEO_LINES, "text_bytes": int(big.numel()), "chunks_at_least": -(-int(big.numel()) // chunk),
                                  "seconds_each_run": runs, "best_lines_per_s": round(CRITEO_LINES / seconds),
                                  "best_text_GB_per_s": round(big.numel() / seconds / 1e9, 2), "equals_the_tiled_result": bool(ok),
                                  "keys_bytes": int(keys.numel() * 8)}
            pkg.check_index_errors()

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

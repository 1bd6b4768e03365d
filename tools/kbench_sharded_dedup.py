"""The de-duplicated sharded lookup (ShardedDeepFM(dedup=True); csrc/route.hip, csrc/gather_fm.hip) against the existing
kernels it stands beside, at the C2 shape (Criteo-26 cardinalities, B = 4096 per rank, D = 16), for ids uniform within
every field and for ids with half of every field's lookups on one value:

  route_*      mi_route_buckets (two launches) against the de-duplicated routing INCLUDING its sort (row add, field sort,
               count, assign), world = 1 and 8 — `world` is only arithmetic for these kernels, one GPU runs them all;
  bwd_*        mi_slot_fm_bwd (memset + store kernel) against mi_slot_fm_bwd_segments (store pass + per-slot sum pass),
               slots of a world-1 routing of the same ids;
  step_*       the world-1 `make_graphed_step` step of ShardedDeepFM on a 1-rank RCCL group, with and without dedup
               (at world 1 dedup saves no bytes — the step can only get slower by the sort and the second backward pass);
  wire_bytes   computed, not measured: world * cap * (8 + 2 * 4 * (D + 4)) bytes per rank and step through the three
               all-to-alls, at world 2 / 4 / 8, for both capacities.

Device-event time around `calls` back-to-back launches; the legs alternate in rounds inside one process, every figure is
the median over the rounds, `spread` is (max - min) / median.  The baselines are the library's own existing kernels timed
in the same run.  Multi-GPU wall time is NOT measured here.  Prints one JSON line and writes it to --out.

    python tools/kbench_sharded_dedup.py [--rounds 5] [--calls 50] [--out profiles/sharded_dedup_kbench.json]
"""
import argparse
import json
import os
import socket
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from recsys_benchmark_amd import _kernels, _lib  # noqa: E402
from recsys_benchmark_amd.sharded import (ShardedDeepFM, dedup_bucket_capacity, field_bucket_capacity)  # noqa: E402

CRITEO_26 = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194,
             27, 14992, 5461306, 10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]
B, D, SLACK = 4096, 16, 1.25


def make_ids(kind, gen):
    cols = []
    for d in CRITEO_26:
        col = torch.randint(0, d, (B,), generator=gen)
        if kind == "half_on_one_value":
            col[torch.rand(B, generator=gen) < 0.5] = int(torch.randint(0, d, (1,), generator=gen))
        cols.append(col)
    return torch.stack(cols, 1)


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


def summarise(xs):
    med = statistics.median(xs)
    return {"median_us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 3), "rounds": [round(x, 2) for x in xs]}


def run_legs(legs, rounds, calls):
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(device_time(fn, calls))
    return {name: summarise(t) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30, help="training steps per round of the step_* legs")
    ap.add_argument("--out", default=os.path.join("profiles", "sharded_dedup_kbench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_sharded_dedup.py measures on an MI355X; no ROCm device found")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    F, N, n = len(CRITEO_26), sum(CRITEO_26), B * len(CRITEO_26)
    offsets = torch.cumsum(torch.tensor([0] + CRITEO_26[:-1]), 0).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "fields": F, "D": D, "lookups": n, "slack": SLACK,
           "rounds": args.rounds, "calls": args.calls, "multi_gpu_wall_time": "not measured"}

    # ---- (d) bytes through the three all-to-alls, from the shapes ---------------------------------------------------
    out["wire_bytes_per_rank_per_step"] = {}
    for world in (2, 4, 8):
        caps = {"plain": field_bucket_capacity(CRITEO_26, B, world, SLACK), "dedup": dedup_bucket_capacity(CRITEO_26, B, world, SLACK)}
        out["wire_bytes_per_rank_per_step"][f"world{world}"] = {
            k: {"capacity": c, "bytes": world * c * (8 + 2 * 4 * (D + 4))} for k, c in caps.items()}

    gen = torch.Generator().manual_seed(0)
    for kind in ("uniform", "half_on_one_value"):
        x = make_ids(kind, gen).to(dev)
        res = {}
        # ---- (a) routing ------------------------------------------------------------------------------------------------
        for world in (1, 8):
            cap_p = field_bucket_capacity(CRITEO_26, B, world, SLACK)
            cap_d = dedup_bucket_capacity(CRITEO_26, B, world, SLACK)
            flag_p, flag_d = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            slot_p, slot_d = torch.empty_like(x), torch.empty_like(x)
            seg = torch.empty(2 * world * cap_d + n, dtype=torch.int32, device=dev)
            legs = {
                f"route_plain_world{world}": lambda w=world, c=cap_p, fl=flag_p, s=slot_p: _kernels.route_buckets(
                    x, offsets, w, N, c, fl, slot_out=s),
                f"route_dedup_with_sort_world{world}": lambda w=world, c=cap_d, fl=flag_d, s=slot_d, sg=seg:
                    _kernels.route_buckets_unique(x, offsets, w, N, c, fl, slot_out=s, segments_out=sg),
            }
            r = run_legs(legs, args.rounds, args.calls)
            r[f"route_plain_world{world}"].update(capacity=cap_p, overflowed=int(flag_p.item()))
            r[f"route_dedup_with_sort_world{world}"].update(
                capacity=cap_d, overflowed=int(flag_d.item()),
                distinct_rows=int(torch.unique((x + offsets).reshape(-1)).numel()))
            res.update(r)
        # ---- (b) slot backward ------------------------------------------------------------------------------------------
        S = n
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _, slot_p = _kernels.route_buckets(x, offsets, 1, N, S, flag)
        _, slot_d, seg = _kernels.route_buckets_unique(x, offsets, 1, N, S, flag)
        emb = torch.randn(B, F, D, device=dev) * 0.1
        g_emb, g_y = torch.randn(B, F, D, device=dev), torch.randn(B, device=dev)
        gbuf_p, gbuf_d = torch.empty(S + 1, D + 4, device=dev), torch.empty(S + 1, D + 4, device=dev)
        gb = torch.empty(1, device=dev)
        ws = torch.empty(int(lib.mi_slot_fm_bwd_segments_workspace_elems(B, F, D)), device=dev)
        stream = _lib.stream_ptr(dev)

        def bwd_plain():
            _lib.check(lib.mi_slot_fm_bwd(slot_p.data_ptr(), emb.data_ptr(), g_y.data_ptr(), g_emb.data_ptr(), gbuf_p.data_ptr(),
                                          gb.data_ptr(), S, B, F, D, stream), "mi_slot_fm_bwd")

        def bwd_segments():
            _lib.check(lib.mi_slot_fm_bwd_segments(seg.data_ptr(), emb.data_ptr(), g_y.data_ptr(), g_emb.data_ptr(), ws.data_ptr(),
                                                   gbuf_d.data_ptr(), gb.data_ptr(), S, B, F, D, stream),
                       "mi_slot_fm_bwd_segments")

        res.update(run_legs({"bwd_plain_store": bwd_plain, "bwd_segments_sum": bwd_segments}, args.rounds, args.calls))
        # same gradient mass either way: the plain rows scattered by row id against the summed rows
        res["bwd_column_sums_max_abs_diff"] = float((gbuf_p[:S].sum(0) - gbuf_d[:S].sum(0)).abs().max())
        lens = (seg[1:2 * S:2] - seg[0:2 * S:2])
        res["longest_segment"] = int(lens.max())
        out[kind] = res

    # ---- (c) the world-1 graphed step -----------------------------------------------------------------------------------
    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    torch.manual_seed(0)
    steps = {}
    for name, dedup in (("step_plain", False), ("step_dedup", True)):
        model = ShardedDeepFM(CRITEO_26, D, [400, 400, 400], p_dropout=0.5, use_batchnorm=True, device=dev, dedup=dedup)
        steps[name] = (model, model.make_graphed_step(pkg.BCEWithLogitsLoss(), B))
    y = (torch.rand(B, device=dev) < 0.3).float()
    for kind in ("uniform", "half_on_one_value"):
        xs = [make_ids(kind, gen).to(dev) for _ in range(4)]
        legs = {}
        for name, (model, step) in steps.items():
            it = [0]

            def one(step=step, it=it):
                it[0] += 1
                step(xs[it[0] % len(xs)], y)

            legs[name] = one
        r = run_legs(legs, args.rounds, args.steps)
        out[kind].update(r)
        out[kind]["step_dedup_over_plain"] = round(r["step_dedup"]["median_us"] / r["step_plain"]["median_us"], 3)
    for model, _ in steps.values():
        model.check_overflow()
    pkg.check_index_errors()
    torch.cuda.synchronize()
    dist.destroy_process_group()

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""CPU: the de-duplicated routing of the row-sharded DeepFM (ShardedDeepFM(dedup=True)).  Properties of its torch
restatement (tests/sharded_dedup_helpers.py), the capacity rule on the Criteo-26 cardinalities under skew, and the whole
choreography on gloo (world 2 and 4) with ids that overflow today's buckets, against the single-process oracle."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from sharded_dedup_helpers import (CRITEO_26, DedupTorchOps, congruent_hot_values, field_offsets, hot_value_ids,
                                   slots_from_segments, zipf_ids)

from oracle.sharded_ops import TorchOps
from recsys_benchmark_amd.sharded import (dedup_bucket_capacity, expected_peak_distinct, expected_peak_load,
                                          field_bucket_capacity)

DIMS = [50, 7, 1000, 3, 211]


def _cases():
    g = torch.Generator().manual_seed(11)
    B = 97
    uniform = torch.stack([torch.randint(0, d, (B,), generator=g) for d in DIMS], 1)
    hot = hot_value_ids(DIMS, B, 0.5, g)
    zipf = zipf_ids(DIMS, B, 2.0, 3)
    broken = uniform.clone()
    broken[3, 4] = 10**6           # beyond N
    broken[7, 0] = -60             # row < 0
    return {"uniform": uniform, "hot": hot, "zipf": zipf, "out_of_range": broken}


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("cap", [400, 23])              # 23: fewer slots than some owner's distinct rows
@pytest.mark.parametrize("name", ["uniform", "hot", "zipf", "out_of_range"])
def test_restatement_properties(name, cap, world):
    x = _cases()[name]
    N, off = sum(DIMS), field_offsets(DIMS)
    over = torch.zeros(1, dtype=torch.int32)
    send, slot, segments = DedupTorchOps.route_buckets_unique(x, off, world, N, cap, over)
    rows, s = (x + off).reshape(-1), slot.reshape(-1)
    dump = world * cap
    valid = (rows >= 0) & (rows < N)
    kept = s != dump
    # equal rows share a slot, different rows never do
    for r in torch.unique(rows[valid]).tolist():
        assert torch.unique(s[rows == r]).numel() == 1
    assert torch.unique(s[kept]).numel() == torch.unique(rows[kept]).numel()
    # every non-dumped lookup finds its own row behind its slot
    owner = s[kept] // cap
    assert torch.equal(send[s[kept]] * world + owner, rows[kept])
    surplus = torch.zeros_like(valid)
    for w in range(world):
        mine = valid & (rows % world == w)
        distinct = torch.unique(rows[mine] // world)
        filled = min(distinct.numel(), cap)
        bucket = send[w * cap:(w + 1) * cap]
        assert bool((bucket[1:filled] > bucket[:filled - 1]).all())            # strictly ascending local rows
        assert torch.equal(bucket[:filled], distinct[:filled])
        assert bool((bucket[filled:] == (N - w + world - 1) // world).all())    # the rest: the owner's sink row
        if distinct.numel() > cap:
            surplus |= mine & torch.isin(rows // world, distinct[cap:])
    # dumped = out of range, or a surplus distinct row's lookups; the flag says whether there was surplus
    assert torch.equal(~kept, ~valid | surplus)
    assert int(over.item()) == int(bool(surplus.any()))
    # the segment description lists, per slot, exactly its lookups in ascending flat position
    rebuilt, ascending = slots_from_segments(segments, dump, rows.numel())
    assert ascending and torch.equal(rebuilt, s)


def test_restatement_writes_into_static_buffers_and_summing_lookup_adds_repeated_slots():
    x = _cases()["hot"]
    N, off, world, cap = sum(DIMS), field_offsets(DIMS), 2, 300
    ref = DedupTorchOps.route_buckets_unique(x, off, world, N, cap, torch.zeros(1, dtype=torch.int32))
    slot_out = torch.zeros_like(x)
    seg_out = torch.zeros(2 * world * cap + x.numel(), dtype=torch.int32)
    send_out = torch.zeros(world * cap, dtype=torch.int64)
    got = DedupTorchOps.route_buckets_unique(x, off, world, N, cap, torch.zeros(1, dtype=torch.int32), slot_out=slot_out,
                                             segments_out=seg_out, send_out=send_out)
    assert got[0] is send_out and got[1] is slot_out and got[2] is seg_out
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    buf = torch.randn(world * cap + 1, 12).requires_grad_(True)
    emb, y = DedupTorchOps.slot_fm_unique(buf, slot_out, torch.zeros(1), seg_out)
    emb.sum().backward()
    counts = torch.bincount(slot_out.reshape(-1), minlength=world * cap + 1).float()
    assert counts.max() > 1                                                  # slots ARE shared
    assert torch.equal(buf.grad[:, :8], counts.view(-1, 1).expand(-1, 8))


def test_expected_peak_distinct_and_capacity_rule():
    # one field of c values at world 1: c * (1 - (1 - 1/c)^B), and never more than the lookups or the rows
    assert abs(expected_peak_distinct([10], 5, 1) - 10 * (1 - 0.9 ** 5)) < 1e-12
    for world in (2, 4, 8):
        peak = expected_peak_distinct(CRITEO_26, 4096, world)
        assert peak <= expected_peak_load(CRITEO_26, 4096, world)
        cap = dedup_bucket_capacity(CRITEO_26, 4096, world, 1.25)
        assert cap == min(field_bucket_capacity(CRITEO_26, 4096, world, 1.25), int(peak * 1.25 + 6 * peak ** 0.5) + 64)
    assert dedup_bucket_capacity(CRITEO_26, 4096, 8, 1.25) == 8794
    assert field_bucket_capacity(CRITEO_26, 4096, 8, 1.25) == 19029
    assert dedup_bucket_capacity(CRITEO_26, 4096, 1, 1.25) <= 4096 * 26


@pytest.mark.parametrize("world", [4, 8])
def test_half_on_one_value_overflows_today_and_fits_deduplicated(world):
    """Criteo-26 cardinalities, B = 4096 per rank, half of every field's lookups on one value (drawn per field), the
    batches of seeds 0-4 routed one after the other with the sticky overflow word a model keeps: today's routing at
    today's capacity raises it (where the hot values land decides which batch does: the worst owner of the five gets
    ~36 K lookups against 34 989 slots at world 4, ~22 K against 19 029 at world 8), the de-duplicated routing at the
    2x smaller de-duplicated capacity never does — no owner is asked for more than ~7.5 K / ~3.8 K distinct rows."""
    B = 4096
    N, off = sum(CRITEO_26), field_offsets(CRITEO_26)
    cap_plain = field_bucket_capacity(CRITEO_26, B, world, 1.25)
    cap_dedup = dedup_bucket_capacity(CRITEO_26, B, world, 1.25)
    assert cap_dedup < cap_plain
    over_plain = torch.zeros(1, dtype=torch.int32)
    over_dedup = torch.zeros(1, dtype=torch.int32)
    for seed in range(5):
        x = hot_value_ids(CRITEO_26, B, 0.5, torch.Generator().manual_seed(seed))
        rows = (x + off).reshape(-1)
        most = int(torch.bincount(rows % world, minlength=world).max())
        distinct = max(int(torch.unique(rows[rows % world == w]).numel()) for w in range(world))
        print(f"world {world} seed {seed}: worst owner {most} lookups (capacity {cap_plain}), "
              f"{distinct} distinct rows (capacity {cap_dedup})")
        before = int(over_plain.item())
        TorchOps.route_buckets(x, off, world, N, cap_plain, over_plain)
        assert int(over_plain.item()) == max(before, int(most > cap_plain))      # the flag means what it says
        _, slot, _ = DedupTorchOps.route_buckets_unique(x, off, world, N, cap_dedup, over_dedup)
        assert int(over_dedup.item()) == 0 and not bool((slot == world * cap_dedup).any())
        assert distinct <= cap_dedup // 2
    assert int(over_plain.item()) == 1


# ---- the choreography on gloo -----------------------------------------------------------------------------------------
GLOO_DIMS, GLOO_B, GLOO_D, GLOO_SLACK = [2000, 3000, 5000, 4000], 512, 16, 1.25


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, dedup, out_q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import reference_ops as ro
        from recsys_benchmark_amd.sharded import ShardedDeepFM, local_num_rows, shard_rows

        dims, D, B, hidden = GLOO_DIMS, GLOO_D, GLOO_B, [16, 8]
        torch.manual_seed(100)
        N = sum(dims)
        W_full = torch.rand(N, D) - 0.5
        w1_full = torch.randn(N, 1)
        torch.manual_seed(7)
        model = ShardedDeepFM(dims, D, hidden, p_dropout=0.0, use_batchnorm=False, ops=DedupTorchOps,
                              bucket_slack=GLOO_SLACK, dedup=dedup)
        model.load_full_tables(W_full, w1_full)
        n_local = local_num_rows(N, rank, world)

        # 60 % of every field's lookups on the id whose global row is = 0 mod world: owner 0 is asked for far more
        # LOOKUPS than a bucket holds, and for few distinct rows
        gen = torch.Generator().manual_seed(55)
        x_all = hot_value_ids(dims, B * world, 0.6, gen, hot=congruent_hot_values(dims, world))
        y_all = (torch.rand(B * world, generator=gen) < 0.4).float()
        x, y = x_all[rank * B:(rank + 1) * B], y_all[rank * B:(rank + 1) * B]
        rows = (x + ro.field_offsets(dims)).reshape(-1)
        at0 = rows[rows % world == 0]
        plain_cap = field_bucket_capacity(dims, B, world, GLOO_SLACK)
        assert at0.numel() > plain_cap                                   # the premise: today's bucket cannot hold them
        assert torch.unique(at0).numel() < dedup_bucket_capacity(dims, B, world, GLOO_SLACK) // 2
        assert model.capacity(B) == (dedup_bucket_capacity if dedup else field_bucket_capacity)(dims, B, world, GLOO_SLACK)

        logits = model(x)
        torch.nn.BCEWithLogitsLoss()(logits, y).backward()
        model.allreduce_dense_grads()
        if not dedup:                                                    # today's behaviour, pinned
            with pytest.raises(RuntimeError, match="overflowed"):
                model.check_overflow()
            out_q.put((rank, "ok"))
            return
        model.check_overflow()

        p = {"offsets": ro.field_offsets(dims), "embedding._emb_module.weight": W_full.clone().requires_grad_(True),
             "fc.weight": w1_full.clone().requires_grad_(True), "_bias": model._bias.detach().clone().requires_grad_(True)}
        for k, v in model._deep_branch.state_dict().items():
            p["_deep_branch." + k] = v.detach().clone().requires_grad_(True)
        ref = ro.deepfm_forward(x_all, p, len(hidden), False, True)
        torch.nn.BCEWithLogitsLoss()(ref, y_all).backward()

        torch.testing.assert_close(logits, ref[rank * B:(rank + 1) * B].detach(), rtol=1e-5, atol=1e-6)
        gWd, g1d = model.embedding_shard.grad.to_dense(), model.fc_shard.grad.to_dense()
        torch.testing.assert_close(gWd[:n_local], shard_rows(p["embedding._emb_module.weight"].grad, rank, world),
                                   rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(g1d[:n_local], shard_rows(p["fc.weight"].grad, rank, world), rtol=1e-5, atol=1e-7)
        assert not gWd[n_local].any() and not g1d[n_local].any()
        torch.testing.assert_close(model._bias.grad, p["_bias"].grad, rtol=1e-5, atol=1e-7)
        for k, v in model._deep_branch.named_parameters():
            torch.testing.assert_close(v.grad, p["_deep_branch." + k].grad, rtol=1e-5, atol=1e-7)
        out_q.put((rank, "ok"))
    except Exception:  # surface the failure in the parent
        import traceback

        out_q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _run(world, dedup):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, dedup, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=360) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in results:
        assert msg == "ok", f"rank {rank}:\n{msg}"


@pytest.mark.parametrize("world", [2, 4])
def test_skewed_ids_overflow_the_plain_sharded_lookup(world):
    _run(world, dedup=False)


@pytest.mark.parametrize("world", [2, 4])
def test_skewed_ids_fit_deduplicated_and_match_the_single_process_oracle(world):
    _run(world, dedup=True)


def test_enable_graphs_is_refused_under_dedup():
    from recsys_benchmark_amd.sharded import ShardedDeepFM

    model = ShardedDeepFM.__new__(ShardedDeepFM)
    torch.nn.Module.__init__(model)
    model.dedup = True
    with pytest.raises(NotImplementedError, match="make_graphed_step"):
        model.enable_graphs(64)

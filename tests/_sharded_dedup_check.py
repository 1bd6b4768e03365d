"""Child process of tests/test_sharded_dedup_gpu.py: ShardedDeepFM(dedup=True) on a 1-rank RCCL group — eager and through
make_graphed_step — must give what dedup=False gives with the same weights and batches (logits / loss and every gradient),
over three consecutive steps with different skewed batches, so that the static slot and segment buffers are really
refreshed.  A process of its own: it shares no process group with another test module."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from recsys_benchmark_amd.sharded import ShardedDeepFM  # noqa: E402
from sharded_dedup_helpers import hot_value_ids  # noqa: E402


def _dense(g):
    return g.to_dense() if g.is_sparse else g


def main():
    os.environ["MASTER_ADDR"] = "127.0.0.1"    # never inherit the parent test process's rendezvous
    os.environ["MASTER_PORT"] = sys.argv[1] if len(sys.argv) > 1 else "29548"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    torch.manual_seed(5)
    dims, D, B = [50, 7, 1000, 3], 16, 64
    kw = dict(p_dropout=0.0, use_batchnorm=True, device=dev)
    plain = ShardedDeepFM(dims, D, [32, 16], **kw)
    eager = ShardedDeepFM(dims, D, [32, 16], dedup=True, **kw)
    stepper = ShardedDeepFM(dims, D, [32, 16], dedup=True, **kw)
    eager.load_state_dict(plain.state_dict())
    stepper.load_state_dict(plain.state_dict())
    try:
        eager.enable_graphs(B)
    except NotImplementedError as e:
        assert "make_graphed_step" in str(e)
    else:
        raise AssertionError("enable_graphs() must refuse dedup=True")

    from recsys_benchmark_amd.losses import BCEWithLogitsLoss

    step = stepper.make_graphed_step(BCEWithLogitsLoss(), B)
    lossf = torch.nn.BCEWithLogitsLoss()
    gen = torch.Generator().manual_seed(17)
    for it in range(3):
        # warm-ups / earlier steps moved the BatchNorm running stats: all three start the step from the same state
        plain.load_state_dict(stepper.state_dict())
        eager.load_state_dict(stepper.state_dict())
        x = hot_value_ids(dims, B, 0.5, gen).to(dev)          # new hot values every step
        y = (torch.rand(B, generator=gen) < 0.3).float().to(dev)
        assert torch.unique(x[:, 2]).numel() < B                # lookups DO share rows
        plain.zero_grad(set_to_none=True)
        eager.zero_grad(set_to_none=True)
        a = plain(x)
        ref_loss = lossf(a, y)
        ref_loss.backward()
        plain.allreduce_dense_grads()
        b = eager(x)
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-6)
        lossf(b, y).backward()
        eager.allreduce_dense_grads()
        loss = step(x, y)
        torch.testing.assert_close(loss.reshape(()), ref_loss.detach().reshape(()), rtol=1e-5, atol=1e-6)
        N = sum(dims)
        for name, model in (("eager", eager), ("graphed step", stepper)):
            gW, g1 = _dense(model.embedding_shard.grad), _dense(model.fc_shard.grad)
            torch.testing.assert_close(gW[:N], _dense(plain.embedding_shard.grad)[:N], rtol=1e-5, atol=1e-7,
                                       msg=lambda m: f"step {it} {name} table grad: {m}")
            torch.testing.assert_close(g1[:N], _dense(plain.fc_shard.grad)[:N], rtol=1e-5, atol=1e-7,
                                       msg=lambda m: f"step {it} {name} first-order grad: {m}")
            assert not gW[N].any() and not g1[N].any()          # the sink row
            torch.testing.assert_close(model._bias.grad, plain._bias.grad, rtol=1e-5, atol=1e-7)
            for (k, p), (_, q) in zip(model._deep_branch.named_parameters(), plain._deep_branch.named_parameters()):
                torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-6, msg=lambda m: f"step {it} {name} {k}: {m}")
            for (k, p), (_, q) in zip(model.named_buffers(), plain.named_buffers()):
                torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6, msg=lambda m: f"step {it} {name} buffer {k}: {m}")
    for model in (plain, eager, stepper):
        model.check_overflow()
        model.check_index_errors()
    torch.cuda.synchronize()
    print("SHARDED_DEDUP_OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""CERP / QR on the CF models at the Yelp2018 shape (31 668 users, 38 048 items, D = 64): the table form of the two-table
family (mi_dual_table_fwd / _bwd, what get_weight() runs) against the lookup over an explicit arange(N)
(mi_dual_gather_fwd / _bwd: the previous get_weight()), and the eager LightGCN CERP step (L = 3, B = 2048, K = 1 and 5,
Adam) with the table form and the one-launch batch-row terms against the same step written with the previous pieces
(arange lookups for the tables, four more lookups for the batch rows, a first-occurrence mask for the distinct users).
Prints one JSON line.

Old and new alternate in rounds inside one process; every figure is the median over the rounds, and `spread` is
(max - min) / median over the rounds of the OLD path: a difference inside it is noise.

(a) `*_us` are per eager call, timed by device events around back-to-back calls: they include the Python and launch cost
of each call.  Kernel times come from a rocprofv3 --kernel-trace --stats run of `--legs a --rounds 1`
(profiles/cerp_cf_kernel_stats.csv); `*_bytes` are the bytes the kernel must move, from the shapes.
(b) `step_ms_*` are host-clock times per step around a window that ends in a device synchronise.

    python tools/kbench_cerp_cf.py [--legs a|b|all] [--rounds 5]
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
from recsys_benchmark_amd import _kernels, losses, trainer  # noqa: E402
from recsys_benchmark_amd.embeddings import get_embedding  # noqa: E402
from recsys_benchmark_amd.graph_utils import calculate_sparse_graph_adj_norm  # noqa: E402

U, I, D, B = 31668, 38048, 64, 2048
HBM_PEAK = 8.0e12            # bytes/s, spec
DEV = "cuda:0"
CONFIGS = [("cerp_b5500", {"name": "cerp", "bucket_size": 5500}), ("cerp_b10000", {"name": "cerp", "bucket_size": 10000}),
           ("qr_div2", {"name": "qr", "divider": 2, "operation": "mult"}), ("qr_div5", {"name": "qr", "divider": 5, "operation": "mult"})]


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us


def summarise(old, new):
    med = statistics.median
    return {"old": round(med(old), 2), "new": round(med(new), 2),
            "spread_old": round((max(old) - min(old)) / med(old), 3), "spread_new": round((max(new) - min(new)) / med(new), 3)}


def make_table(cfg, n):
    torch.manual_seed(0)
    emb = get_embedding(cfg, n, D).to(DEV)
    if cfg["name"] == "cerp":
        with torch.no_grad():        # active pruning, as a CERP run has after its first epochs
            emb.p_threshold.copy_(torch.randn_like(emb.p_threshold) - 2)
            emb.q_threshold.copy_(torch.randn_like(emb.q_threshold) - 2)
    return emb


def table_bytes(emb):
    """(forward, backward) bytes the table form must move: every table operand once, the output / its gradient once, the
    parameter gradients once (the other table's rows a `mult` backward re-reads are served by the caches)."""
    params = sum(p.numel() * 4 for p in emb.parameters())
    out = I * D * 4
    return params + out, out + 2 * params


def leg_a(out, rounds, iters=200):
    for tag, cfg in CONFIGS:
        emb = make_table(cfg, I)
        params = [p for p in emb.parameters() if p.requires_grad]
        G = torch.randn(I, D, device=DEV)
        old_fwd = lambda: emb(torch.arange(I, device=DEV))          # noqa: E731  (the previous get_weight(), verbatim)
        new_fwd = emb.get_weight
        w_old, w_new = old_fwd(), new_fwd()
        assert type(w_new.grad_fn).__name__.startswith("DualTable") and torch.equal(w_old, w_new)
        old_bwd = lambda: torch.autograd.grad(w_old, params, G, retain_graph=True)      # noqa: E731
        new_bwd = lambda: torch.autograd.grad(w_new, params, G, retain_graph=True)      # noqa: E731
        for a, b in zip(old_bwd(), new_bwd()):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
        t = {k: [] for k in ("of", "nf", "ob", "nb")}
        for _ in range(rounds):
            t["of"].append(timed(old_fwd, iters))
            t["nf"].append(timed(new_fwd, iters))
            t["ob"].append(timed(old_bwd, iters))
            t["nb"].append(timed(new_bwd, iters))
        fb, bb = table_bytes(emb)
        out[tag] = {"fwd_us": summarise(t["of"], t["nf"]), "bwd_us": summarise(t["ob"], t["nb"]), "fwd_bytes": fb, "bwd_bytes": bb}
        for k, nbytes in (("fwd_us", fb), ("bwd_us", bb)):
            out[tag][k]["new_hbm_share_lower_bound"] = round(nbytes / (out[tag][k]["new"] * 1e-6) / HBM_PEAK, 4)


def old_step_losses(model, adj, users, pos_items, neg_items, weight_decay, info_nce_weight, prune_loss_weight, k_tanh=100):
    """cf_cerp_step_losses with the previous pieces: the tables through the lookup over arange(N), the batch-row terms
    through four more lookups (cerp_embedding_utils.py:32-62), the distinct users through a first-occurrence mask."""
    ut, it = model.user_emb_table, model.item_emb_table
    neg = trainer._negatives_2d(neg_items, users)
    K = neg.shape[1]
    neg_flat = neg.reshape(-1)
    all_user_emb, all_item_emb = _kernels.lightgcn_propagate(model.sparse_dropout(adj), ut(torch.arange(U, device=DEV)),
                                                             it(torch.arange(I, device=DEV)), model.num_layers)
    users_k, pos_k = (users, pos_items) if K == 1 else (users.repeat_interleave(K), pos_items.repeat_interleave(K))
    rec_loss = losses.bpr_loss_rows(all_user_emb, all_item_emb, users_k, pos_k, neg_flat) * K
    ue, pe, ne = ut(users), it(pos_items), it(neg_flat)
    reg_loss = (ue.norm(2).pow(2) + pe.norm(2).pow(2) + ne.norm(2).pow(2)) / (2 * len(users))
    valid = losses.first_occurrence(users, U)
    prune_loss = -((torch.tanh(ue * k_tanh) ** 2 * valid.unsqueeze(1)).sum() + torch.tanh(pe * k_tanh).norm(2) ** 2
                   + torch.tanh(ne * k_tanh).norm(2) ** 2)
    cl_loss = trainer._cf_info_nce(all_user_emb, all_item_emb, users, pos_items, info_nce_weight, valid)
    return rec_loss + weight_decay * reg_loss + cl_loss + prune_loss * prune_loss_weight


def leg_b(out, rounds, steps=20):
    gen = torch.Generator().manual_seed(0)
    graph = {u: sorted(set(torch.randint(0, I, (int(torch.randint(5, 60, (1,), generator=gen)),), generator=gen).tolist()))
             for u in range(U)}
    adj = calculate_sparse_graph_adj_norm(graph, I, U).to(DEV)
    w = dict(weight_decay=1e-5, info_nce_weight=0.1, prune_loss_weight=1e-4)
    for tag, cfg in CONFIGS:
        for K in (1, 5):
            torch.manual_seed(0)
            model = pkg.LightGCN(U, I, num_layers=3, hidden_size=D, embedding_config=cfg).to(DEV).train()
            if cfg["name"] == "cerp":
                with torch.no_grad():
                    for _, t in model.get_embs():
                        t.p_threshold.copy_(torch.randn_like(t.p_threshold) - 2)
                        t.q_threshold.copy_(torch.randn_like(t.q_threshold) - 2)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            batches = [(torch.randint(0, U, (B,), device=DEV), torch.randint(0, I, (B,), device=DEV),
                        torch.randint(0, I, (B, K), device=DEV)) for _ in range(steps)]

            def run(losses_fn):
                for users, pos, neg in batches:
                    loss = losses_fn(model, adj, users, pos, neg, **w)
                    loss = loss[0] if isinstance(loss, tuple) else loss
                    opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(model.parameters(), trainer.CERP_CLIP_GRAD_NORM)
                    opt.step()

            def window(losses_fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(losses_fn)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps * 1e3

            run(old_step_losses)
            run(trainer.cf_cerp_step_losses)
            old, new = [], []
            for _ in range(rounds):
                old.append(window(old_step_losses))
                new.append(window(trainer.cf_cerp_step_losses))
            out[f"step_ms_{tag}_k{K}"] = summarise(old, new)
            pkg.check_index_errors()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="all", choices=["a", "b", "all"])
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_cerp_cf needs an MI355X"
    out = {"shape": {"users": U, "items": I, "D": D, "batch": B, "layers": 3}, "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "command": "python tools/kbench_cerp_cf.py " + " ".join(sys.argv[1:])}
    if args.legs in ("a", "all"):
        leg_a(out, args.rounds)
    if args.legs in ("b", "all"):
        leg_b(out, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

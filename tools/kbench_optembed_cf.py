"""CF OptEmbed at the Yelp2018 shape (user table 31 668 x 64, item table 38 048 x 64): forward and backward of the
masked table (mi_optembed_cf_fwd / _bwd) per law and norm, with the share of HBM peak of the bytes they must move; the
reference's stock-torch op sequence on the same GPU (norm, BinaryStep, repeat_interleave, F.embedding of the triangular
mask, products; the feature-mode draw through the host WeightedRandomSampler); the eager LightGCN OptEmbed step
(L = 3, B = 2048, Adam); and the time per search candidate.  Prints one JSON line.

The *_us fields are per eager call, timed by device events around back-to-back calls: they include the Python and launch
cost of each call, so the *_hbm_share fields are lower bounds.  Kernel times come from a rocprofv3 --kernel-trace --stats
run of this tool (profiles/optembed_cf_kernel_stats.csv).

    python tools/kbench_optembed_cf.py
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from recsys_benchmark_amd import trainer  # noqa: E402
from recsys_benchmark_amd.embeddings import cf_opt_embed as cf  # noqa: E402
from recsys_benchmark_amd.embeddings import get_embedding  # noqa: E402
from recsys_benchmark_amd.graph_utils import calculate_sparse_graph_adj_norm  # noqa: E402

U, I, D, B = 31668, 38048, 64, 2048
HBM_PEAK = 8.0e12            # bytes/s, spec (MI355X_MICROARCH: 6.29 TB/s measured for a float4 copy)
DEV = "cuda:0"


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


def kernel_legs(out):
    N = I
    for norm in (1, 2):
        for law_name, ts in (("uniform", None), ("exponential", 0.8)):
            emb = get_embedding({"name": "optembed", "norm": norm, "mode_threshold_e": "feature",
                                 "mode_threshold_d": "feature", "target_sparsity": ts}, N, D).to(DEV).train()
            G = torch.randn(N, D, device=DEV)
            fwd = timed(lambda: emb.get_weight(), 200)
            w = emb.get_weight()

            def bwd():
                torch.autograd.grad(w, [emb._weight, emb._mask_e_module._t_param], G, retain_graph=True)
            bwd_us = timed(bwd, 200)
            tag = f"l{norm}_{law_name}"
            out[f"fwd_us_{tag}"] = round(fwd, 2)
            out[f"bwd_us_{tag}"] = round(bwd_us, 2)
            out[f"fwd_hbm_share_{tag}"] = round(2 * N * D * 4 / (fwd * 1e-6) / HBM_PEAK, 3)
            out[f"bwd_hbm_share_{tag}"] = round(3 * N * D * 4 / (bwd_us * 1e-6) / HBM_PEAK, 3)
    # linear law: draw-only launch over the table's rows
    out["draw_only_us_linear"] = round(timed(lambda: cf.draw_widths(N, D, 0.7, 2, DEV), 200), 2)


def torch_reference_legs(out):
    """The reference's get_weight in stock torch ops on the same GPU, and its host draw."""
    N = I
    W = torch.nn.Parameter(torch.empty(N, D, device=DEV))
    torch.nn.init.xavier_uniform_(W)
    t = torch.nn.Parameter(torch.zeros(N, device=DEV))
    full = torch.tril(torch.ones(D, D, dtype=torch.bool, device=DEV))
    G = torch.randn(N, D, device=DEV)
    weight = cf.width_probabilities(cf.find_alpha(0.8, D), D)

    def host_draw():
        sampler = torch.utils.data.WeightedRandomSampler(weight, N)
        return torch.tensor(list(sampler), device=DEV)

    def ref_fwd(idx):
        u = torch.norm(W, 1, dim=1) - t
        mask_e = (u > 0).float().unsqueeze(-1)          # BinaryStep forward
        return W * mask_e * F.embedding(idx, full)

    idx = torch.randint(0, D, (N,), device=DEV)
    out["torch_fwd_us_given_mask"] = round(timed(lambda: ref_fwd(idx), 100), 2)
    t0 = time.perf_counter()
    for _ in range(5):
        host_draw()
    torch.cuda.synchronize()
    out["torch_host_weighted_sampler_draw_us"] = round((time.perf_counter() - t0) / 5 * 1e6, 1)
    w = ref_fwd(idx)
    out["torch_bwd_us_no_binarystep_surrogate"] = round(timed(lambda: torch.autograd.grad(w, [W, t], G, retain_graph=True,
                                                                                         allow_unused=True), 100), 2)


def lightgcn_step(out):
    gen = torch.Generator().manual_seed(0)
    graph = {u: sorted(set(torch.randint(0, I, (int(torch.randint(5, 60, (1,), generator=gen)),), generator=gen).tolist()))
             for u in range(U)}
    adj = calculate_sparse_graph_adj_norm(graph, I, U).to(DEV)

    class _DS:
        num_users, num_items = U, I

        def get_norm_adj(self):
            return adj

        def get_graph(self):
            return graph

    class _Loader(list):
        dataset = _DS()

    torch.manual_seed(0)
    model = pkg.LightGCN(U, I, num_layers=3, hidden_size=D,
                         embedding_config={"name": "optembed", "mode_threshold_d": "feature",
                                           "target_sparsity": 0.8}).to(DEV)
    t_params = [t._mask_e_module._t_param for _, t in model.get_embs()]
    others = [p for n, p in model.named_parameters() if "_t_param" not in n]
    opts = [torch.optim.Adam(others, lr=1e-3), torch.optim.Adam(t_params, lr=1e-2)]
    batches = _Loader([(torch.randint(0, U, (B,)), torch.randint(0, I, (B,)), torch.randint(0, I, (B,))) for _ in range(20)])
    trainer.train_epoch_optembed(_Loader(batches[:3]), model, opts, device=DEV, log_step=0, weight_decay=1e-4, alpha=1e-2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train_epoch_optembed(batches, model, opts, device=DEV, log_step=0, weight_decay=1e-4, alpha=1e-2)
    torch.cuda.synchronize()
    out["lightgcn_optembed_eager_step_ms"] = round((time.perf_counter() - t0) / len(batches) * 1e3, 3)
    # one search candidate: draw both masks and score them with validate_epoch_cf (2048 validation users)
    users = torch.arange(B)
    val = [(users, [graph[u][:3] for u in range(B)])]
    cand = cf._generate(U, I, D, 0.8, 1, DEV)
    cf._validate_candidate(model, cand, val, _DS())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        cand = cf._generate(U, I, D, 0.8, 1, DEV)
        cf._validate_candidate(model, cand, val, _DS())
    torch.cuda.synchronize()
    out["search_candidate_ms_2048_val_users"] = round((time.perf_counter() - t0) / 3 * 1e3, 2)


def main():
    assert torch.cuda.is_available(), "kbench_optembed_cf needs an MI355X"
    out = {"shape": {"users": U, "items": I, "D": D, "batch": B}, "device": torch.cuda.get_device_name(0)}
    kernel_legs(out)
    torch_reference_legs(out)
    lightgcn_step(out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

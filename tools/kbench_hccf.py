"""HCCF propagation at the Yelp2018 shape (31 668 x 38 048, the interaction set of tools/kbench_cf_data.py, D = 64, L = 2,
B = 2048), slope 0.5 and slope 1.  Prints one JSON line.

(a) forward + backward of the propagation per eager call, timed by device events around back-to-back calls (Python and
    launch cost included), the incoming gradient non-zero on a batch's rows as BPR leaves it:
      new       _kernels.hccf_propagate: one launch per layer each way, 1 bit per element kept for the backward
      old       the same computation composed from the previous pieces: _kernels.spmm both ways, torch LeakyReLU and adds,
                autograd (a saved [N, D] pre-activation per layer)
      torch     stock torch.sparse on the GPU, written as src/models/hccf.py:53-68 writes it
      lightgcn  _kernels.lightgcn_propagate on the same block adjacency: the yardstick (no activation, no residual)
    Old and new alternate in rounds; every figure is the median over the rounds and `spread` is (max - min) / median.
    `*_bytes` are the bytes each form must move per forward + backward, from the shapes (gathers counted once).
(b) the training step through trainer.cf_step_losses (weight decay 1e-4, optim.Adam), eager and replayed as one hipGraph,
    with p_dropout 0 and 0.5: host-clock time per step around a window that ends in a device synchronise.

Kernel times come from a separate run, `rocprofv3 --kernel-trace --stats -- python tools/kbench_hccf.py --legs a --rounds 1 --iters 10`
(profiles/hccf_kernel_stats.csv): hccf_fwd / hccf_bwd next to the LightGCN layer kernel (k_spmm_planned) in one trace.

    python tools/kbench_hccf.py [--legs a|b|all] [--rounds 5] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recsys_benchmark_amd as pkg  # noqa: E402
from kbench_cf_data import yelp_graphs  # noqa: E402
from recsys_benchmark_amd import _kernels, trainer  # noqa: E402
from recsys_benchmark_amd.graph_utils import get_adj  # noqa: E402
from recsys_benchmark_amd.optim import Adam  # noqa: E402

U, I, D, B, L = 31668, 38048, 64, 2048, 2
N = U + I
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


def summarise(xs):
    med = statistics.median(xs)
    return {"median": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 3)}


def composed(M, Mt, Xu, Xi, slope):
    """src/models/hccf.py:47-68 on the previous pieces."""
    us, its, ru, ri = Xu, Xi, Xu, Xi
    for _ in range(L):
        zu = torch.nn.functional.leaky_relu(_kernels.spmm(M, its), slope)
        zi = torch.nn.functional.leaky_relu(_kernels.spmm(Mt, us), slope)
        us, its = zu + us, zi + its
        ru, ri = ru + us, ri + its
    return ru / (L + 1), ri / (L + 1)


def stock(M, Xu, Xi, slope):
    us, its, ru, ri = Xu, Xi, Xu, Xi
    for _ in range(L):
        zu = torch.nn.functional.leaky_relu(M @ its, slope)
        zi = torch.nn.functional.leaky_relu(M.t() @ us, slope)
        us, its = zu + us, zi + its
        ru, ri = ru + us, ri + its
    return ru / (L + 1), ri / (L + 1)


def bytes_moved(nnz, slope):
    """Bytes per forward + backward from the shapes: a dense [N, D] pass is N * D * 4, a CSR pass 2 nnz * 8 (both blocks:
    column + value) + the row pointers; every gathered operand counted once."""
    dense, csr, bits = N * D * 4, 2 * nnz * 8 + (N + 1) * 4, (N * D // 8 if slope != 1 else 0)
    # new, forward layer: gather S, read S and R at the row, write R, write S' (not on the last layer), write the bits
    new_fwd = L * (4 * dense + csr + bits) - dense
    # new, backward layer: gather G (+ its bits), read G and g at the row, write G'
    new_bwd = L * (4 * dense + csr + bits)
    # old, forward layer: two products (read X, write Y), LeakyReLU (read, write), two adds each side (2 reads + 1 write each)
    old_fwd = L * (2 * dense + csr + 2 * dense + 6 * dense) + 2 * dense
    # old, backward layer: two transposed products, the masked multiply (reads the saved pre-activation), the adds of autograd
    old_bwd = L * (2 * dense + csr + 3 * dense + 6 * dense) + 2 * dense
    lgcn = 2 * L * (3 * dense + csr)            # gather, read + write the running sum (the step's own write joins on L - 1 layers)
    return {"new": new_fwd + new_bwd, "old": old_fwd + old_bwd, "lightgcn": lgcn, "saved_for_backward_new": L * bits,
            "saved_for_backward_old": L * dense}


def leg_a(out, adj, rounds, iters):
    M = adj.to_sparse_csr()
    Mt = adj.t().coalesce().to_sparse_csr()
    plan, vals = _kernels.hccf_plan(adj)
    sq = plan.square
    A = torch.sparse_csr_tensor(sq.crow.long(), sq.col.long(), plan.values(vals), (N, N))       # LightGCN's operand
    gen = torch.Generator(device=DEV).manual_seed(0)
    Xu = (torch.randn(U, D, device=DEV, generator=gen) * 0.1).requires_grad_(True)
    Xi = (torch.randn(I, D, device=DEV, generator=gen) * 0.1).requires_grad_(True)
    gu, gi = torch.zeros(U, D, device=DEV), torch.zeros(I, D, device=DEV)
    gu[torch.randint(0, U, (B,), device=DEV, generator=gen)] = torch.randn(B, D, device=DEV, generator=gen)
    gi[torch.randint(0, I, (2 * B,), device=DEV, generator=gen)] = torch.randn(2 * B, D, device=DEV, generator=gen)

    def both(fn):
        def run():
            return torch.autograd.grad(fn(), (Xu, Xi), (gu, gi))
        return run

    lightgcn = both(lambda: _kernels.lightgcn_propagate(A, Xu, Xi, L))
    out["nnz"] = int(vals.numel())
    for slope in (0.5, 1.0):
        forms = {"new": both(lambda: _kernels.hccf_propagate(adj, Xu, Xi, L, slope)),
                 "old": both(lambda: composed(M, Mt, Xu, Xi, slope)),
                 "torch": both(lambda: stock(adj, Xu, Xi, slope)),
                 "lightgcn": lightgcn}
        want = forms["old"]()
        for name in ("new", "torch"):
            for a, b in zip(forms[name](), want):
                torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
        t = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                t[k].append(timed(fn, iters))
        key = f"propagate_fwd_bwd_us_slope{slope:g}"
        out[key] = {k: summarise(v) for k, v in t.items()}
        out[key]["old_over_new"] = round(out[key]["old"]["median"] / out[key]["new"]["median"], 3)
        out[key]["bytes"] = bytes_moved(out["nnz"], slope)


def leg_b(out, adj, rounds, steps=20):
    gen = torch.Generator().manual_seed(1)
    batches = [tuple(torch.randint(0, n, (B,), generator=gen).to(DEV) for n in (U, I, I)) for _ in range(steps)]
    for p in (0.0, 0.5):
        for graphed in (False, True):
            key = f"step_ms_p{p:g}_{'graph' if graphed else 'eager'}"
            try:
                torch.manual_seed(0)
                model = pkg.HCCFModelCore(U, I, num_layers=L, hidden_size=D, slope=0.5, p_dropout=p).to(DEV).train()
                step = trainer.GraphedCFTrainStep(model, adj, Adam(model.parameters(), lr=1e-3), weight_decay=1e-4,
                                                  use_graph=graphed)

                def window():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for b in batches:
                        step(*b)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / steps * 1e3

                window()
                if graphed and step._graph is None:
                    raise RuntimeError("the step was not captured")
                out[key] = summarise([window() for _ in range(rounds)])
                pkg.check_index_errors()
            except Exception as e:          # reported, not hidden: the figure is then "not measured"
                out[key] = f"not measured: {type(e).__name__}: {e}"[:300]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="all", choices=["a", "b", "all"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="back-to-back calls per timing of leg (a)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_hccf needs an MI355X"
    out = {"shape": {"users": U, "items": I, "D": D, "batch": B, "layers": L}, "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "command": "python tools/kbench_hccf.py " + " ".join(sys.argv[1:])}
    adj = get_adj(yelp_graphs()[0], I, U, normalize=True).to(DEV)
    if args.legs in ("a", "all"):
        leg_a(out, adj, args.rounds, args.iters)
    if args.legs in ("b", "all"):
        leg_b(out, adj, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

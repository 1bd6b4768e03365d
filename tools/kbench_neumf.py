"""NeuMF at the Yelp2018 shape (U=31 668, I=38 048, emb_size=64, hidden_sizes=[64, 32, 16]): the training step on
2048 triples (4096 samples: users.repeat(2) against cat([pos, neg])), the same step with Adam captured in one
torch.cuda.graph, and the all-items scoring of a 2048-user batch; against the reference's forms in stock torch on the
same GPU.  Prints one JSON line.

    python tools/kbench_neumf.py [--trace kernel_trace.csv]

--trace: the kernel trace csv of a `rocprofv3 --kernel-trace --stats` run of this tool; the scoring kernel's median
dispatch time from it gives the share of fp32 MFMA peak (157.3 TF/s) of the kernel's FLOPs (computed from the shapes
below).
"""
import argparse
import csv
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_benchmark_amd as pkg  # noqa: E402
from recsys_benchmark_amd import optim, trainer  # noqa: E402
from recsys_benchmark_amd.neumf import NeuMF, score_all_items  # noqa: E402

U, I, EMB, HIDDEN, B = 31668, 38048, 64, [64, 32, 16], 2048
PEAK_TF = 157.3


def score_flops() -> int:
    """FLOPs of mi_neumf_score_all per (user, item) pair, times B * I: layer 1's add + relu, the hidden products, the
    mlp_fc dot, the GMF dot (gu * w precomputed per user would not change the order)."""
    D = EMB // 2
    per = 2 * HIDDEN[0]
    per += sum(2 * a * b for a, b in zip(HIDDEN[:-1], HIDDEN[1:])) + sum(HIDDEN[1:])       # products + bias/relu
    per += 2 * HIDDEN[-1] + 3 * D + 2
    return per * B * I


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
    return a.elapsed_time(b) / n


class TorchNeuMF(nn.Module):
    """The reference's forms (src/models/mlp.py) in stock torch: nn.Embedding tables, cat, nn.Sequential tower."""

    def __init__(self, src: NeuMF):
        super().__init__()
        D = EMB // 2
        self.gu, self.gi, self.mu, self.mi = (nn.Embedding(n, D) for n in (U, I, U, I))
        self.gmf_fc = nn.Linear(D, 1)
        layers, w = [], 2 * D
        for h in HIDDEN:
            layers += [nn.Linear(w, h), nn.ReLU(), nn.Dropout(0)]
            w = h
        self.mlp = nn.Sequential(*layers)
        self.mlp_fc = nn.Linear(w, 1)
        with torch.no_grad():
            for dst, t in zip((self.gu, self.gi, self.mu, self.mi), src._tables()):
                dst.weight.copy_(t.get_weight())
            self.gmf_fc.load_state_dict(src._gmf.gmf_fc.state_dict())
            self.mlp.load_state_dict(src._mlp.mlp.state_dict())
            self.mlp_fc.load_state_dict(src._mlp.mlp_fc.state_dict())

    def forward(self, u, i):
        y_gmf = self.gmf_fc(self.gu(u) * self.gi(i)).squeeze(-1)
        y_mlp = self.mlp_fc(self.mlp(torch.cat([self.mu(u), self.mi(i)], -1))).squeeze(-1)
        return y_mlp + y_gmf


def torch_step_losses(model, users, pos, neg, wd):
    y = model(users.repeat(2), torch.cat([pos, neg]))
    f = nn.functional.binary_cross_entropy_with_logits
    rec = f(y[:B], torch.ones_like(y[:B])) + f(y[B:], torch.zeros_like(y[B:]))
    reg = sum(t(ids).norm(2).pow(2) for t, ids in ((model.mi, pos), (model.mi, neg), (model.mu, users), (model.gi, pos),
                                                    (model.gi, neg), (model.gu, users))) / (2 * B)
    return rec + wd * reg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default=None)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = NeuMF(U, I, emb_size=EMB, hidden_sizes=HIDDEN).to(dev)
    g = torch.Generator().manual_seed(1)
    users = torch.randint(0, U, (B,), generator=g).to(dev)
    pos = torch.randint(0, I, (B,), generator=g).to(dev)
    neg = torch.randint(0, I, (B,), generator=g).to(dev)
    wd = 1e-4
    one = pkg.losses.unit_scalar(dev)

    def fwd_bwd():
        for p in model.parameters():
            p.grad = None
        loss, _, _ = trainer.nmf_step_losses(model, users, pos, neg, wd)
        loss.backward(one)

    out = {"shape": {"users": U, "items": I, "emb_size": EMB, "hidden_sizes": HIDDEN, "train_triples": B,
                     "train_samples": 2 * B, "score_users": B}}
    out["fwd_bwd_ms"] = round(timed(fwd_bwd, args.iters), 4)

    opt = optim.Adam(model.parameters(), lr=1e-3)

    def step():
        loss, _, _ = trainer.nmf_step_losses(model, users, pos, neg, wd)
        opt.zero_grad(set_to_none=True)
        loss.backward(one)
        opt.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        step()
    out["graphed_step_adam_ms"] = round(timed(graph.replay, args.iters), 4)
    out["eager_step_adam_ms"] = round(timed(step, args.iters), 4)

    model.eval()
    score_users = torch.randint(0, U, (B,), generator=g).to(dev)
    scores = torch.empty((B, I), dtype=torch.float32, device=dev)
    out["score_all_ms_per_2048_users"] = round(timed(lambda: score_all_items(model, score_users, scores), 10), 4)
    out["score_kernel_flops"] = score_flops()
    pkg.check_index_errors()

    ref = TorchNeuMF(model).to(dev)
    ref.train()
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3)

    def ref_fwd_bwd():
        ref.zero_grad(set_to_none=True)
        torch_step_losses(ref, users, pos, neg, wd).backward()

    def ref_step():
        loss = torch_step_losses(ref, users, pos, neg, wd)
        ropt.zero_grad()
        loss.backward()
        ropt.step()

    out["torch_fwd_bwd_ms"] = round(timed(ref_fwd_bwd, args.iters), 4)
    out["torch_step_adam_ms"] = round(timed(ref_step, args.iters), 4)
    ref = TorchNeuMF(model).to(dev).eval()      # the trained copy above took its own Adam steps: start again from `model`
    chunk = 16                     # the reference's [users, N_items, D] lookups: 16 users at a time fit in memory
    all_items = torch.arange(I, device=dev).unsqueeze(0)

    @torch.no_grad()
    def ref_score():
        u = score_users[:chunk]
        return ref(u.unsqueeze(1).repeat(1, I), all_items.repeat(chunk, 1))

    ms = timed(ref_score, 5)
    out["torch_score_chunk_users"] = chunk
    out["torch_score_ms_per_chunk"] = round(ms, 4)
    out["torch_score_ms_per_2048_users_extrapolated"] = round(ms * B / chunk, 3)
    with torch.no_grad():
        diff = (ref_score() - score_all_items(model, score_users[:chunk])).abs().max().item()
    out["score_max_abs_diff_vs_torch"] = diff
    out["score_speedup_vs_torch"] = round(out["torch_score_ms_per_2048_users_extrapolated"] / out["score_all_ms_per_2048_users"], 2)

    if args.trace:
        # the median dispatch of the scoring kernel (all but one of its dispatches in this tool score 2048 users)
        with open(args.trace) as f:
            ns = sorted(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(f)
                        if "k_neumf_score" in r["Kernel_Name"])
        med = ns[len(ns) // 2]
        out["score_kernel_rocprof_ms"] = round(med / 1e6, 4)
        out["score_kernel_tflops"] = round(score_flops() / med / 1e3, 2)
        out["score_kernel_share_of_fp32_mfma_peak"] = round(score_flops() / med / 1e3 / PEAK_TF, 3)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What the QAT / PTQ DeepFM tests share: the reference's quantisation arithmetic restated — the forward in float32
(elementwise IEEE operations in the reference's order: the same bits on any machine), the backward in float64 from a
saved emb — and the pieces of DeepFM around the lookup, so that a CPU-only test can hold the restatement against the
reference's goldens and a GPU test can hold the kernels against the restatement."""
import os

import torch


def q_range(n_bits: int):
    """(q_min, q_max) of the signed n_bits range."""
    return -(1 << (n_bits - 1)), (1 << (n_bits - 1)) - 1


def qat_rows32(w, scale, n_bits: int, prob):
    """StotasticRounding.forward (src/models/embeddings/qat_emb.py:16-45) with the draw given: float32 in, float32 out."""
    q_min, q_max = q_range(n_bits)
    q = torch.clamp(w / scale, q_min, q_max)
    fl = torch.floor(q)
    return (fl + (prob > fl + 1 - q)) * scale


def qat_backward64(emb, w_rows, scale, n_bits: int, rows, N: int, G, gy):
    """The fused lookup's gradients in float64 from the emb the forward saved (float32 [B, F, D]), the gathered rows of the
    table (float32 [B F, D]), the upstream gradients G [B, F, D] (into emb, beside the FM term) and gy [B] (into y_fm):

      dE     = G + gy (S - e), S = sum_f e     the table's value rows (straight through the rounding)
      dscale = sum dE m,  m = q_max where qf >= q_max, q_min where qf <= q_min, else res - qf
               with qf = w / scale AS THE FLOAT32 QUOTIENT (what the reference saves) and res = emb / scale rounded to the
               integer it is (emb = res * scale rounded once)
    and the sums of |float32 terms| that bound a float32 evaluation in any order: |G| + |gy| (sum|e| + |e|) for dE, that
    times (|res| + |qf|) for the scale — m is a difference of two float32 values."""
    B, F, D = emb.shape
    n = B * F
    q_min, q_max = q_range(n_bits)
    e = emb.double()
    G, gy = G.double(), gy.double().view(B, 1, 1)
    dE = (G + gy * (e.sum(1, keepdim=True) - e)).view(n, D)
    terms = (G.abs() + gy.abs() * (e.abs().sum(1, keepdim=True) + e.abs())).view(n, D)
    qf = (w_rows.float() / scale.float()).double()                 # the float32 quotient, exactly
    res = torch.round(e.view(n, D) / scale.double())
    m = torch.where(qf >= q_max, torch.full_like(qf, q_max), torch.where(qf <= q_min, torch.full_like(qf, q_min), res - qf))
    served = ((rows >= 0) & (rows < N)).view(n, 1)
    safe = rows.clamp(0, N - 1)
    out = dict(dE=dE, terms=terms, m=m, qf=qf, res=res)
    out["gW"] = torch.zeros(N, D, dtype=torch.float64).index_add_(0, safe, dE * served)
    out["tW"] = torch.zeros(N, D, dtype=torch.float64).index_add_(0, safe, terms * served)
    out["gscale"] = (dE * m * served).sum()
    out["tscale"] = (terms * (res.abs() + qf.abs()) * served).sum()
    return out


def ptq_rows32(codes, scale=None, zero_point=None):
    """The dequantised rows as the library defines them: (float)((int)code - (int)zero) * scale, or the fp16 value."""
    if codes.dtype == torch.float16:
        return codes.float()
    return (codes.to(torch.int32) - zero_point.to(torch.int32)).float() * scale.float()


def fm_first_order64(emb, rows, w1, bias):
    """y_fm of src/models/deepfm.py:91-98 in float64."""
    e = emb.double()
    fm = 0.5 * (e.sum(1).pow(2) - e.pow(2).sum(1)).sum(1)
    return fm + w1.double().view(-1)[rows].sum(1) + bias.double().view(-1)[0]


def tail64(params, emb, prefix="_deep_branch."):
    """The MLP tail of a DeepFM without BatchNorm and dropout (Linear, ReLU, ..., Linear) in float64 on emb [B, F D]."""
    keys = sorted({k[len(prefix):].split(".")[0] for k in params if k.startswith(prefix)}, key=int)
    h = emb
    for i, k in enumerate(keys):
        h = h @ params[f"{prefix}{k}.weight"].double().t() + params[f"{prefix}{k}.bias"].double()
        if i + 1 < len(keys):
            h = torch.relu(h)
    return h.squeeze(-1)


def upstream_gradients64(params, emb, y_fm, y):
    """(logits, G, gy) under BCEWithLogitsLoss (mean): the gradients that reach the lookup node — G into emb through the
    tail, gy into y_fm — from float64 leaves holding the given emb and y_fm."""
    e = emb.double().clone().requires_grad_(True)
    yf = y_fm.double().clone().requires_grad_(True)
    logits = yf + tail64(params, e.reshape(e.shape[0], -1))
    torch.nn.BCEWithLogitsLoss()(logits, y.double()).backward()
    return logits.detach(), e.grad, yf.grad


def save_checkpoint(path, table):
    """The checkpoint file the PTQ classes quantise: {"state_dict": {"embedding._emb_module.weight": table}}."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"state_dict": {"embedding._emb_module.weight": table}}, path)
    return path

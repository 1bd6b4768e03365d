"""Float64 restatements for the CF CERP tests (test_cerp_cf_host.py, test_cerp_cf_gpu.py): the two-table family in table
form (forward, and the backward as the owner-computes reduction the kernel performs, written out with index_add), the
batch-row regulariser / prune loss with its gradient in closed form, and the LightGCN CERP step assembled from them.
Nothing here calls the library."""
import torch

OPS = ("mult", "add", "cat")


def f64(t):
    return None if t is None else t.detach().cpu().double()


def soft64(w, s):
    return torch.sign(w) * torch.relu(w.abs() - torch.sigmoid(s))


def keep_margin(w, s, margin=1e-3):
    """w with every element at least `margin` away from its threshold sigmoid(s) in magnitude (moved outwards where it was
    closer): the float32 kernel and the float64 restatement then agree on every mask bit."""
    t = torch.sigmoid(s.double())
    close = (w.double().abs() - t).abs() < margin
    sign = torch.where(w >= 0, torch.ones_like(w), -torch.ones_like(w))
    return torch.where(close, (sign.double() * (t + 2 * margin)).to(w.dtype), w)


def _xf(T, S, M):
    if S is not None:
        return soft64(T, S)
    if M is not None:
        return T * (M != 0).double()
    return T


def dual_table_ref64(T1, T2, N, mod1, div2, op, S1=None, S2=None, M1=None, M2=None):
    """out[i] = T1'[i % mod1] (op) T2'[i // div2], i = 0 .. N-1, in float64."""
    T1, T2, S1, S2, M1, M2 = (f64(t) for t in (T1, T2, S1, S2, M1, M2))
    i = torch.arange(N)
    a, b = _xf(T1, S1, M1)[i % mod1], _xf(T2, S2, M2)[i // div2]
    return a * b if op == "mult" else (a + b if op == "add" else torch.cat([a, b], dim=1))


def dual_table_bwd_ref64(g, T1, T2, N, mod1, div2, op, S1=None, S2=None, M1=None, M2=None):
    """The backward as a reduction per table row: returns a dict with gT1, gT2 (and gS1, gS2 for the soft threshold), the
    sums of the absolute terms behind each element (`abs_T1` ...: what a float32 summation error is measured against) and
    the contributor counts per row (`n1`, `n2`)."""
    g, T1, T2, S1, S2, M1, M2 = (f64(t) for t in (g, T1, T2, S1, S2, M1, M2))
    De = T1.shape[1]
    i = torch.arange(N)
    i1, i2 = i % mod1, i // div2
    x1, x2 = _xf(T1, S1, M1), _xf(T2, S2, M2)
    if op == "cat":
        c1, c2 = g[:, :De], g[:, De:]
    elif op == "mult":
        c1, c2 = g * x2[i2], g * x1[i1]
    else:
        c1, c2 = g, g
    out = {}
    for name, c, idx, T, S, M in (("1", c1, i1, T1, S1, M1), ("2", c2, i2, T2, S2, M2)):
        s = torch.zeros_like(T).index_add_(0, idx, c)              # row r <- its contributors, every one exactly once
        a = torch.zeros_like(T).index_add_(0, idx, c.abs())
        out["n" + name] = torch.zeros(T.shape[0], dtype=torch.int64).index_add_(0, idx, torch.ones_like(idx))
        if S is not None:
            t = torch.sigmoid(S)
            keep = (T.abs() - t > 0).double()
            fs = -torch.sign(T) * keep * t * (1 - t)
            out["gT" + name], out["gS" + name] = s * keep, s * fs
            out["abs_T" + name], out["abs_S" + name] = a * keep, a * fs.abs()
        else:
            f = (M != 0).double() if M is not None else torch.ones_like(T)
            out["gT" + name], out["abs_T" + name] = s * f, a * f
    return out


def first_occurrence(ids):
    seen, out = set(), []
    for v in ids.tolist():
        out.append(v not in seen)
        seen.add(v)
    return torch.tensor(out)


def reg_prune_ref64(U, I, users, pos, neg, k_tanh=100.0, g_reg=1.0, g_prune=1.0):
    """(reg, prune, dU, dI) in float64 with the gradient in closed form:
    reg = (|U[u]|^2 + |I[p]|^2 + |I[n]|^2) / 2B over ALL batch rows, prune = -|tanh(K rows)|^2 with the users
    de-duplicated; d reg / dw = w / B per occurrence, d prune / dw = -2 K tanh(K w) (1 - tanh^2(K w)) per counted row."""
    U, I = f64(U), f64(I)
    users, pos, neg = users.cpu().reshape(-1), pos.cpu().reshape(-1), neg.cpu().reshape(-1)
    B = users.numel()
    uniq = users[first_occurrence(users)]
    items = torch.cat([pos, neg])
    reg = (U[users].pow(2).sum() + I[items].pow(2).sum()) / (2 * B)
    prune = -(torch.tanh(k_tanh * U[uniq]).pow(2).sum() + torch.tanh(k_tanh * I[items]).pow(2).sum())

    def dprune(w):
        t = torch.tanh(k_tanh * w)
        return -2 * k_tanh * t * (1 - t * t)

    dU = torch.zeros_like(U).index_add_(0, users, g_reg * U[users] / B).index_add_(0, uniq, g_prune * dprune(U[uniq]))
    dI = torch.zeros_like(I).index_add_(0, items, g_reg * I[items] / B + g_prune * dprune(I[items]))
    return reg, prune, dU, dI


def dense_adj64(a):
    """The normalised adjacency of tests/golden/cf_sample_adj.npz as a dense float64 matrix."""
    crow, col, val = a.t("crow"), a.t("col"), a.t("val")
    return torch.sparse_csr_tensor(crow, col, val.double()).to_dense()


def lightgcn_cerp_step_ref64(tables, adj, num_layers, users, pos, neg2d, weight_decay, info_nce_weight, prune_loss_weight,
                             k_tanh=100.0):
    """One LightGCN CERP step on materialised float64 `tables` = (user table, item table): the five losses and dLoss/dTable
    for both tables.  Propagation, bpr_loss_multi and InfoNCE through float64 autograd; the batch-row terms through
    reg_prune_ref64's closed form."""
    U = tables[0].clone().requires_grad_(True)
    I = tables[1].clone().requires_grad_(True)
    nu = U.shape[0]
    res = step = torch.cat([U, I], 0)
    for _ in range(num_layers):
        step = adj @ step
        res = res + step
    res = res / (num_layers + 1)
    ue, ie = res[:nu], res[nu:]
    B = users.numel()
    u, p, n = ue[users], ie[pos], ie[neg2d]                      # [B, D], [B, D], [B, K, D]
    diff = (u * p).sum(1, keepdim=True) - torch.einsum("ij,ikj->ik", u, n)
    rec = -torch.nn.functional.logsigmoid(diff).sum() / B
    cl = torch.zeros((), dtype=torch.float64)
    if info_nce_weight > 0:
        view = torch.cat([ue[torch.unique(users)], ie[torch.unique(pos)]], 0)
        v = torch.nn.functional.normalize(view, dim=1)
        cl = -torch.diag(torch.log_softmax(v @ v.T / 0.2, dim=1)).mean() * info_nce_weight
    (rec + cl).backward()
    reg, prune, dU, dI = reg_prune_ref64(U, I, users, pos, neg2d, k_tanh, weight_decay, prune_loss_weight)
    loss = rec.detach() + weight_decay * reg + cl.detach() + prune * prune_loss_weight
    return dict(loss=loss, rec_loss=rec.detach(), reg_loss=reg, cl_loss=cl.detach(), prune_loss=prune,
                gU=U.grad + dU, gI=I.grad + dI, user_emb=ue.detach(), item_emb=ie.detach())

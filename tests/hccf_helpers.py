"""HCCF propagation restated in the block form, for the HCCF tests (CPU, any dtype; float64 is the reference).

With S = [U; I] (N = users + items rows) and A_k = [[0, M_k], [M_k^T, 0]] (M_k the k-th layer's U x I matrix: one
dropout draw serves both products of a layer, src/models/hccf.py:53-57):

    S_k = S_{k-1} + leaky(A_k S_{k-1});   R_k = R_{k-1} + S_k;   out = R_L / (L + 1)

and, for an incoming gradient g = [g_u; g_i], with c = 1 / (L + 1) and f_k = 1 where pre_k > 0, else `slope`
(torch's convention: pre == 0 takes the slope):

    G_L = c g;   G_{k-1} = c g + G_k + A_k (G_k . f_k);   dX = G_0
"""
import torch


def block_adjacency(idx, vals, U, I, dtype=torch.float64):
    """Dense [[0, M], [M^T, 0]] of the COO matrix (idx [2, nnz], vals [nnz]); duplicates are summed."""
    A = torch.zeros(U + I, U + I, dtype=dtype)
    A.index_put_((idx[0], idx[1] + U), vals.to(dtype), accumulate=True)
    A.index_put_((idx[1] + U, idx[0]), vals.to(dtype), accumulate=True)
    return A


def hccf_forward(idx, vals, Xu, Xi, slope, dtype=torch.float64):
    """vals: one value tensor per layer.  Returns (user_emb, item_emb, [pre_1 .. pre_L])."""
    U, I, L = Xu.shape[0], Xi.shape[0], len(vals)
    S = torch.cat([Xu, Xi]).detach().to(dtype)
    R, pres = S.clone(), []
    for v in vals:
        pre = block_adjacency(idx, v, U, I, dtype) @ S
        S = S + torch.where(pre > 0, pre, slope * pre)
        R = R + S
        pres.append(pre)
    R = R / (L + 1)
    return R[:U], R[U:], pres


def hccf_backward(idx, vals, pres, gu, gi, slope, U, dtype=torch.float64):
    """The recurrence above: (dXu, dXi) for U users.  gu / gi None = zero."""
    L, (N, D) = len(vals), pres[0].shape
    I = N - U
    g = torch.cat([gu.to(dtype) if gu is not None else torch.zeros(U, D, dtype=dtype),
                   gi.to(dtype) if gi is not None else torch.zeros(I, D, dtype=dtype)])
    c = 1.0 / (L + 1)
    G = c * g
    for k in range(L, 0, -1):
        f = torch.where(pres[k - 1] > 0, torch.ones((), dtype=dtype), torch.full((), slope, dtype=dtype))
        G = c * g + G + block_adjacency(idx, vals[k - 1], U, I, dtype) @ (G * f)
    return G[:U], G[U:]


def min_nonzero_abs(pres):
    """Smallest non-zero |pre-activation| over the layers (inf when there is none)."""
    m = float("inf")
    for p in pres:
        nz = p[p != 0].abs()
        if nz.numel():
            m = min(m, float(nz.min()))
    return m


def reference_loss_and_grads(idx, vals, Xu, Xi, slope, users, pos, neg, weight_decay):
    """float64 autograd over hccf_forward's formula: (user_emb, item_emb, bpr, reg, dXu, dXi, pres) of
    bpr + weight_decay * reg, reg the reference's get_reg_loss."""
    Xu64 = Xu.detach().double().requires_grad_(True)
    Xi64 = Xi.detach().double().requires_grad_(True)
    U, I, L = Xu.shape[0], Xi.shape[0], len(vals)
    S = torch.cat([Xu64, Xi64])
    R, pres = S, []
    for v in vals:
        pre = block_adjacency(idx, v, U, I) @ S
        S = S + torch.nn.functional.leaky_relu(pre, slope)
        R = R + S
        pres.append(pre.detach())
    R = R / (L + 1)
    ue, ie = R[:U], R[U:]
    bpr = -torch.nn.functional.logsigmoid((ue[users] * ie[pos]).sum(1) - (ue[users] * ie[neg]).sum(1)).mean()
    reg = (Xu64[users].norm(2).pow(2) + Xi64[pos].norm(2).pow(2) + Xi64[neg].norm(2).pow(2)) / (2 * len(users))
    (bpr + weight_decay * reg).backward()
    return ue.detach(), ie.detach(), bpr.detach(), reg.detach(), Xu64.grad, Xi64.grad, pres


# ---------------------------------------------------------------------------------------------------- the dyadic fixture
DY_U, DY_I = 300, 280
DY_HUB_USER, DY_HUB_ITEM = 3, 5          # 270 items / 265 users: both above the kernels' hub threshold (256)
DY_LONE_USER, DY_LONE_ITEM = 7, 9        # no interaction at all


def _odd_sixteenths(shape, gen):
    return (2 * torch.randint(-8, 8, shape, generator=gen) + 1).to(torch.float32) / 16


def dyadic_fixture(D, L, seed=0):
    """Inputs on which every product and every running sum of the forward and the backward is exactly representable in
    float32 for L <= 3, so that float32 and float64 agree bit for bit in ANY summation order: table and gradient entries
    (2 randint(-8, 8) + 1) / 16 (the gradient non-zero on a quarter of the rows), nnz values from {0.25, 0.5, 1} times
    a dropout factor from {0, 2} drawn anew per layer; slope must be 0.5 or 0.25 (or 0 / 1).  300 x 280 with one hub
    user, one hub item, one isolated user and one isolated item.  `assert_dyadic_exact` checks the claim on the CPU."""
    gen = torch.Generator().manual_seed(1000 * seed + 7)
    U, I = DY_U, DY_I
    pairs = set()
    for i in torch.randperm(I, generator=gen)[:271].tolist():
        if i != DY_LONE_ITEM and len([p for p in pairs if p[0] == DY_HUB_USER]) < 270:
            pairs.add((DY_HUB_USER, i))
    for u in torch.randperm(U, generator=gen)[:266].tolist():
        if u != DY_LONE_USER and len([p for p in pairs if p[1] == DY_HUB_ITEM]) < 265:
            pairs.add((u, DY_HUB_ITEM))
    for u in range(U):
        if u in (DY_LONE_USER, DY_HUB_USER):
            continue
        for i in torch.randint(0, I, (int(torch.randint(1, 5, (1,), generator=gen)),), generator=gen).tolist():
            if i != DY_LONE_ITEM:
                pairs.add((u, i))
    idx = torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous()        # canonical (row-major) COO order
    nnz = idx.shape[1]
    base = torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (nnz,), generator=gen)]
    vals = [base * (2.0 * torch.randint(0, 2, (nnz,), generator=gen)) for _ in range(L)]
    Xu, Xi = _odd_sixteenths((U, D), gen), _odd_sixteenths((I, D), gen)
    gu, gi = _odd_sixteenths((U, D), gen), _odd_sixteenths((I, D), gen)
    gu[torch.rand(U, generator=gen) >= 0.25] = 0
    gi[torch.rand(I, generator=gen) >= 0.25] = 0
    return dict(U=U, I=I, idx=idx, vals=vals, Xu=Xu, Xi=Xi, gu=gu, gi=gi)


def dyadic_reference(fx, slope, gu="fx", gi="fx"):
    """float64 (user_emb, item_emb, dXu, dXi) of the fixture; gu / gi default to the fixture's, None = no gradient there."""
    gu = fx["gu"] if isinstance(gu, str) else gu
    gi = fx["gi"] if isinstance(gi, str) else gi
    ue, ie, pres = hccf_forward(fx["idx"], fx["vals"], fx["Xu"], fx["Xi"], slope)
    if not fx["vals"]:
        return ue, ie, None, None
    du, di = hccf_backward(fx["idx"], fx["vals"], pres, gu, gi, slope, fx["U"])
    return ue, ie, du, di


def assert_dyadic_exact(fx, slope):
    """The fixture's claim, for L in {1, 3} (1 / (L + 1) a power of two): the float32 evaluation equals the float64 one
    bit for bit, forward and backward, and the kink is exercised (zeros and negatives among the pre-activations)."""
    L = len(fx["vals"])
    ue, ie, pres = hccf_forward(fx["idx"], fx["vals"], fx["Xu"], fx["Xi"], slope)
    ue32, ie32, pres32 = hccf_forward(fx["idx"], fx["vals"], fx["Xu"], fx["Xi"], slope, dtype=torch.float32)
    for p, p32 in zip(pres, pres32):
        assert torch.equal(p32.double(), p), "a pre-activation is not exact in float32"
    allpre = torch.cat(pres)
    assert (allpre == 0).double().mean() > 0.02 and (allpre < 0).double().mean() > 0.2
    if L in (1, 3):
        assert torch.equal(ue32.double(), ue) and torch.equal(ie32.double(), ie)
        du, di = hccf_backward(fx["idx"], fx["vals"], pres, fx["gu"], fx["gi"], slope, fx["U"])
        du32, di32 = hccf_backward(fx["idx"], fx["vals"], pres32, fx["gu"], fx["gi"], slope, fx["U"], dtype=torch.float32)
        assert torch.equal(du32.double(), du) and torch.equal(di32.double(), di)
        # also when summed the other way round (row order of the dense product reversed)
        S = torch.cat([fx["Xu"], fx["Xi"]]).double()
        A = block_adjacency(fx["idx"], fx["vals"][0], fx["U"], fx["I"])
        assert torch.equal((A.flip(1) @ S.flip(0)).float().double(), pres[0])

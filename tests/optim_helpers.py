"""Plain-torch (CPU) pieces shared by tests/test_optim_host.py and tests/test_optim_steps_gpu.py: a float64 Adam reference
with term bounds, gradients that reach the eps-bound regime, fp32 wrong variants the bounds must reject, and sorted-id
layouts built from explicit run lengths that sit on the pass edges of the row-sparse step.

Bounds after step t (eps32 = 2^-24; the ~11 roundings of one element's chain plus the carried error of m and v):
    |dp - u_ref|  <= (16 + 8t) eps32 U_t + 2 eps32 max(|p_before|, |p_after|)      dp = the step actually taken
    |m - m_ref|   <= 8t eps32 M_t
    |v - v_ref|   <= 8t eps32 v_ref
with the running magnitudes M_t = b1 M_{t-1} + (1-b1)|g_t| and U_t = step_factor M_t / (sqrt(v_t) [/sqrt(bc2)] + eps): term
bounds, which do not shrink when m cancels.  Measured against torch's own fp32 CPU optimizers on the inputs below
(tests/test_optim_host.py prints the figures): SparseAdam and Adam, 4 to 6 steps, D in {1, 4, 8, 16}; worst ratios to the
bounds without weight decay: step 0.49, m 0.14, v 0.20; with wd = 1e-3 / 1e-2 (g + wd p and the fp32 wd add roundings
ahead of the square): step 0.46, m 0.35, v 0.71.  The constants are not tuned to any kernel.
"""
import math

import torch

EPS32 = 2.0 ** -24
SCALES = (2.0 ** -30, 2.0 ** -20, 1.0, 2.0 ** 6)     # 2^-30 ~ 1e-9 << eps = 1e-8: eps decides the step there


# ---- gradients ------------------------------------------------------------------------------------------------------
def scaled_ints(shape, gen):
    """fp32 `scale_j x integer in [-8, 8]`, scale_j cycling through SCALES along the last dimension: sums of duplicates are
    exact in fp32 in any order, and one tensor sees the eps-bound and the usual regime side by side."""
    shape = tuple(shape)
    t = torch.randint(-8, 9, shape, generator=gen).float()
    if t.numel() == 0:
        return t
    return t * torch.tensor([SCALES[j % len(SCALES)] for j in range(shape[-1])], dtype=torch.float32)


def dense_params(shape, gen):
    """fp32 parameters with 0.5 <= |p| < 2 for the dense rule with weight decay.  The m and v bounds are relative to the
    magnitude of g + wd p, so they say nothing where the two terms cancel (a randn parameter near g / wd does that to one
    element in a few thousand, and then even torch's fp32 Adam is tens of times outside them).  With wd <= 1e-2 these
    parameters keep wd |p| in [5e-4, 2e-2], far from every gradient of scaled_ints (at most 2^-17, or at least 1)."""
    shape = tuple(shape)
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return sign * (0.5 + 1.5 * torch.rand(shape, generator=gen))


def coalesce_ref(ids, perm, vals, N):
    """(G float64[N, D], present bool[N]): the float64 index_add of vals[perm[i]] over the sorted positions whose id lies in
    [0, N), and which rows occur."""
    ids, perm = ids.cpu(), perm.cpu()
    vals = vals.cpu().double()
    assert vals.dim() == 2 and vals.shape[0] == ids.numel()
    ok = (ids >= 0) & (ids < N)
    G = torch.zeros(N, vals.shape[1], dtype=torch.float64).index_add_(0, ids[ok], vals[perm[ok]])
    present = torch.zeros(N, dtype=torch.bool)
    present[ids[ok]] = True
    return G, present


# ---- float64 reference ----------------------------------------------------------------------------------------------
def adam_ref64(kind, p0, steps, lr, betas, eps, wd=0.0):
    """The update rule in float64.  kind "sparse" (torch.optim.SparseAdam, touched rows only):
        m += (1-b1)(g-m); v += (1-b2)(g^2-v); p -= lr sqrt(1-b2^t)/(1-b1^t) m/(sqrt(v)+eps)
    kind "dense" (torch.optim.Adam with L2 weight decay):
        g += wd p; m += (1-b1)(g-m); v = b2 v+(1-b2)g^2; p -= lr/(1-b1^t) m/(sqrt(v)/sqrt(1-b2^t)+eps)
    `steps` is a list of (g, touched, p_after): the (coalesced, dense-shaped) gradient of step t, the bool mask of touched
    rows (None: all of them) and the fp32 parameter the implementation under test held AFTER that step.  Every step starts
    from the parameter the implementation held before it (p0, then the previous p_after), so parameter rounding does not
    accumulate into the comparison; m and v run in their own float64 chain.  One record per step:
    t, u (the reference step, dp ~ u), U, m, M, v, p_before, p_after — see bound_ratios()."""
    b1, b2 = betas
    p_before = p0.detach().cpu().double()
    m, v, M = torch.zeros_like(p_before), torch.zeros_like(p_before), torch.zeros_like(p_before)
    out = []
    for t, (g, touched, p_after) in enumerate(steps, 1):
        g = g.detach().cpu().double().view(p_before.shape)
        p_after = p_after.detach().cpu().double().view(p_before.shape)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        if kind == "sparse":
            m1, v1, M1 = m + (1 - b1) * (g - m), v + (1 - b2) * (g * g - v), b1 * M + (1 - b1) * g.abs()
            factor, den = lr * math.sqrt(bc2) / bc1, v1.sqrt() + eps
            u, U = -factor * m1 / den, factor * M1 / den
            if touched is not None:
                sel = touched.cpu().view([-1] + [1] * (g.dim() - 1)).expand_as(g)
                zero = torch.zeros_like(g)
                m1, v1, M1 = torch.where(sel, m1, m), torch.where(sel, v1, v), torch.where(sel, M1, M)
                u, U = torch.where(sel, u, zero), torch.where(sel, U, zero)
            m, v, M = m1, v1, M1
        elif kind == "dense":
            g = g + wd * p_before
            m, v, M = m + (1 - b1) * (g - m), b2 * v + (1 - b2) * g * g, b1 * M + (1 - b1) * g.abs()
            factor, den = lr / bc1, v.sqrt() / math.sqrt(bc2) + eps
            u, U = -factor * m / den, factor * M / den
        else:
            raise ValueError(kind)
        out.append(dict(t=t, u=u, U=U, m=m, M=M, v=v, p_before=p_before, p_after=p_after))
        p_before = p_after
    return out


def _worst(err, bound):
    if err.numel() == 0:
        return 0.0
    # no error against a zero bound is ratio 0; any error against a zero bound is inf; a NaN stays a NaN (and fails `<= 1`)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def bound_ratios(rec, m=None, v=None):
    """Worst ratio to each bound of the module docstring for one adam_ref64 record: {"step": ..} plus "m" and "v" when the
    implementation's moments after that step are given.  A ratio above 1 (or a NaN) is outside the bound."""
    t = rec["t"]
    dp = rec["p_after"] - rec["p_before"]
    bound = (16 + 8 * t) * EPS32 * rec["U"] + 2 * EPS32 * torch.maximum(rec["p_before"].abs(), rec["p_after"].abs())
    out = {"step": _worst((dp - rec["u"]).abs(), bound)}
    if m is not None:
        out["m"] = _worst((m.detach().cpu().double().view(rec["m"].shape) - rec["m"]).abs(), 8 * t * EPS32 * rec["M"])
    if v is not None:
        out["v"] = _worst((v.detach().cpu().double().view(rec["v"].shape) - rec["v"]).abs(), 8 * t * EPS32 * rec["v"])
    return out


def worst_ratios(kind, p0, steps, moments, lr, betas, eps, wd=0.0):
    """max over the steps of bound_ratios(); moments = list of (m, v) after each step (or None entries)."""
    worst = {}
    for rec, mv in zip(adam_ref64(kind, p0, steps, lr, betas, eps, wd), moments):
        for k, r in bound_ratios(rec, *(mv if mv is not None else (None, None))).items():
            if k not in worst or math.isnan(r) or r > worst[k]:          # (a NaN sticks: nothing compares above it)
                worst[k] = r
    return worst


# ---- fp32 implementations on the CPU: the right rule and four wrong ones ------------------------------------------------
VARIANTS = ("eps_in_root", "eps_scaled", "omb_fp32", "no_bc2")


def adam_fp32(kind, p0, grads, lr, betas, eps, wd=0.0, variant=None):
    """The same two rules in fp32 torch ops.  grads = list of (g, touched).  variant None is the right rule; the others are
    the mistakes the bounds have to catch: eps inside the root; eps on the wrong side of the sqrt(1-b2^t) correction (dense:
    added before the division, sparse: scaled by it); 1 - beta formed in fp32; no sqrt(1-b2^t) at all.
    Returns [(p_after, m, v)] per step."""
    assert variant is None or variant in VARIANTS
    b1, b2 = betas
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)    # noqa: E731
    omb1, omb2 = f32(1.0 - b1), f32(1.0 - b2)
    if variant == "omb_fp32":
        omb1, omb2 = f32(1.0) - f32(b1), f32(1.0) - f32(b2)
    p = p0.detach().cpu().float().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, (g, touched) in enumerate(grads, 1):
        g = g.detach().cpu().float().view(p.shape)
        bc1 = 1.0 - b1 ** t
        s = 1.0 if variant == "no_bc2" else math.sqrt(1.0 - b2 ** t)
        if kind == "dense":
            g = g + f32(wd) * p
            m1 = m + omb1 * (g - m)
            v1 = f32(b2) * v + omb2 * g * g
            if variant == "eps_in_root":
                den = (v1 + f32(eps)).sqrt() / f32(s)
            elif variant == "eps_scaled":
                den = (v1.sqrt() + f32(eps)) / f32(s)
            else:
                den = v1.sqrt() / f32(s) + f32(eps)
            p1 = p - f32(lr / bc1) * (m1 / den)
        else:
            m1 = m + omb1 * (g - m)
            v1 = v + omb2 * (g * g - v)
            if variant == "eps_in_root":
                den = (v1 + f32(eps)).sqrt()
            elif variant == "eps_scaled":
                den = v1.sqrt() + f32(eps * s)
            else:
                den = v1.sqrt() + f32(eps)
            p1 = p - f32(lr * s / bc1) * (m1 / den)
        if touched is not None:
            sel = touched.view([-1] + [1] * (g.dim() - 1)).expand_as(g)
            m1, v1, p1 = torch.where(sel, m1, m), torch.where(sel, v1, v), torch.where(sel, p1, p)
        p, m, v = p1, m1, v1
        out.append((p.clone(), m.clone(), v.clone()))
    return out


# ---- sorted ids with runs on the pass edges ------------------------------------------------------------------------------
LAYOUTS = ("edges-0", "edges-1", "edges-m1", "one", "short", "tail")


class Layout(dict):
    __getattr__ = dict.__getitem__


def long_run_length(RS):
    return RS * (RS + 2) + 3


def run_layout(RS, N, which):
    """Sorted ids (int64[n]) of a row-form gradient over an N-row table, built from explicit run lengths for a kernel that
    cuts the sorted positions into passes of RS, plus a random non-identity `perm` (sorted position -> original entry).
    `edges` maps each named run to (first position, length).

    "edges-0" / "edges-1" / "edges-m1" (n % RS = 0, 1, RS-1) hold, in this order:
      neg_front       two distinct negatives, then RS+1 copies of -1 (invalid ids across the first pass end)
      aligned_rs      a run of exactly RS that starts a pass
      ends_on_last    a run of max(2, RS/2) that ends on a pass's last position
      single_on_last  one id alone on a pass's last position
      straddle_2      a run of 2: a pass's last position and the next pass's first
      aligned_2rs     a run of 2 RS that starts a pass
      long_mid        a run of RS (RS+2) + 3 that starts at position RS/2 of a pass (more pieces than the RS lane groups
                      of the joining wave: its loop over the pieces takes a second trip)
      back_invalid    id N twice and id N+5 RS+1 times, across a pass end, the last run reaching n
    with single distinct ids as filler in between.  "one": n = 1.  "short": n = RS-1 (n = 0 for RS = 1).  "tail": short
    runs, then a VALID run of 2 RS + RS/2 + 1 from the middle of a pass to n (the piece walk stops at n, not at another id).
    For RS = 1 every run longer than 1 spans passes; the list is the same.  Valid ids are a random sorted sample of [0, N)
    that contains 0 and N-1 and leaves rows out."""
    assert which in LAYOUTS and RS >= 1
    gen = torch.Generator().manual_seed(7919 * RS + LAYOUTS.index(which))
    runs, edges = [], {}          # runs: (fixed id or None for the next valid id, length)
    pos = 0

    def add(length, name=None, fixed=None):
        nonlocal pos
        if name is not None:
            start = edges[name][0] if name in edges else pos
            edges[name] = (start, pos + length - start)
        runs.append((fixed, length))
        pos += length

    def pad(mod):
        while pos % RS != mod % RS:
            add(1)

    def shorts(k):
        for length in torch.randint(1, 4, (k,), generator=gen).tolist():
            add(length)

    if which == "one":
        add(1)
    elif which == "short":
        while pos < RS - 1:
            add(min(int(torch.randint(1, 4, (1,), generator=gen)), RS - 1 - pos))
    elif which == "tail":
        shorts(4)
        pad(RS // 2)
        add(2 * RS + RS // 2 + 1, "tail_run")
    else:
        add(1, "neg_front", -7)
        add(1, "neg_front", -3)
        add(RS + 1, "neg_front", -1)
        pad(0)
        add(RS, "aligned_rs")
        L = max(2, RS // 2)
        pad(-L)
        add(L, "ends_on_last")
        pad(RS - 1)
        add(1, "single_on_last")
        pad(RS - 1)
        add(2, "straddle_2")
        pad(0)
        add(2 * RS, "aligned_2rs")
        pad(RS // 2)
        add(long_run_length(RS), "long_mid")
        shorts(5)
        want = {"edges-0": 0, "edges-1": 1, "edges-m1": RS - 1}[which]
        pad(want - (RS + 3))
        add(2, "back_invalid", N)
        add(RS + 1, "back_invalid", N + 5)
    K = sum(1 for fixed, _ in runs if fixed is None)
    assert K < N, f"{K} distinct ids do not fit a table of {N} rows with rows left out"
    if K == 1:
        valid = [N - 1]
    elif K > 1:
        valid = [0] + sorted((torch.randperm(N - 2, generator=gen)[:K - 2] + 1).tolist()) + [N - 1]
    else:
        valid = []
    it = iter(valid)
    ids = torch.tensor([i for fixed, length in runs for i in [next(it) if fixed is None else fixed] * length] or [],
                       dtype=torch.int64)
    n = ids.numel()
    perm = torch.randperm(n, generator=gen)
    if n > 1 and torch.equal(perm, torch.arange(n)):
        perm = perm.roll(1)
    return Layout(ids=ids, perm=perm, edges=edges, n=n, RS=RS, N=N, which=which)


def crossing_ids(RS, N, n, tile, gen):
    """Random sorted ids in [0, N) (many duplicates) with one run laid across the end of pass `tile - 1`: from three
    positions before position tile*RS to 2 RS + 1 positions after it."""
    ids = torch.sort(torch.randint(0, N, (n,), generator=gen))[0]
    a, b = tile * RS - 3, tile * RS + 2 * RS + 2
    assert 0 < a and b < n
    ids[a:b] = ids[a]              # still sorted: ids[b] >= ids[a]
    return ids, (a, b)

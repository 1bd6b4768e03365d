"""Plain-torch (CPU) pieces shared by tests/test_adagrad_host.py, tests/test_adagrad_steps_gpu.py and
tests/test_adagrad_optim_gpu.py: float64 references of the three Adagrad rules with term bounds, gradients that reach the
eps-bound regime, and fp32 wrong variants the bounds must reject.  The id layouts are optim_helpers'.

Rules (G = the coalesced gradient of a touched row: duplicates summed FIRST; clr = lr / (1 + (t-1) lr_decay)):
    "sparse"   torch.optim.Adagrad on a sparse gradient:  s += G^2;                 p -= clr G / (sqrt(s) + eps)
    "rowwise"  one accumulator per row:                   s[row] += sum_d G_d^2 / D; p -= clr G / (sqrt(s[row]) + eps)
    "dense"    torch.optim.Adagrad, L2 weight decay:      g += wd p; s += g^2;      p -= clr g / (sqrt(s) + eps)

Bounds after step t (eps32 = 2^-24, the largest relative error of one fp32 rounding):
    |dp - u|     <= C_STEP eps32 |u| + 2 eps32 max(|p_before|, |p_after|)        dp = the step actually taken
    |s - s_ref|  <= c_sum(kind, t, D, wd) eps32 s_ref,   c_sum = C_SUM t depth(kind, D, wd)
s is a sum of non-negative terms, so a relative bound is meaningful, and `depth` is the number of roundings on the longest
path from the gradient to one step's addend and into the accumulator, for ANY association of the sum over d:
    sparse, dense without wd   2      (the square, the add into s)
    dense with wd              6      (g + wd p: a product and an add, i.e. 2 eps32 on g and 4 on g^2; then the two above)
    rowwise                    D + 2  (a square, at most D - 1 adds — index order is the deepest tree, the kernels' lane
                                       sum + xor tree is shallower —, the division by D, the add into s)
With C_SUM = 1 that is the worst case of the arithmetic.  The constants are set by measurement, not from any kernel:
yardsticks torch.optim.Adagrad on the CPU in fp32 (sparse with duplicates; dense with wd in {0, 1e-2}; each also with
initial_accumulator_value = 0.1, without which every sum of these gradients is exact) and, for the row-wise rule,
adagrad_fp32() summing d in index order; D in {1, 4, 8, 16, 7, 12}, 5 steps, lr = 1e-2, N = 60 rows, 200 entries.
Worst ratios with both constants at 1 (tests/test_adagrad_host.py prints them):
    step   sparse 0.71   dense 0.50   rowwise 0.96         sum   sparse 0.39   dense 0.55   rowwise 0.08
Twice the worst, rounded up to a whole number: C_STEP = 2, C_SUM = 2 (a kernel may associate the sums differently — the
xor tree, fma contraction —, hence the margin of 2).
"""
import math

import torch

from optim_helpers import EPS32, LAYOUTS, coalesce_ref, crossing_ids, run_layout  # noqa: F401  (re-exported)

SCALES = (2.0 ** -40, 2.0 ** -20, 1.0, 2.0 ** 6)     # 2^-40 ~ 9e-13: sqrt(s) stays well below eps = 1e-10 (and 1e-8)
C_STEP = 2
C_SUM = 2
KINDS = ("sparse", "rowwise", "dense")


# ---- gradients ------------------------------------------------------------------------------------------------------
def scaled_ints(shape, gen):
    """fp32 `scale_j x integer in [-8, 8]`, scale_j cycling through SCALES along the last dimension (the element-wise and
    dense rules): sums of duplicates are exact in fp32 in any order."""
    shape = tuple(shape)
    t = torch.randint(-8, 9, shape, generator=gen).float()
    if t.numel() == 0:
        return t
    return t * torch.tensor([SCALES[j % len(SCALES)] for j in range(shape[-1])], dtype=torch.float32)


def row_scaled_ints(entry_ids, D, gen):
    """fp32 [n, D] `scale(row) x integer in [-8, 8]` for the row-wise rule: the scale cycles along TABLE ROWS (id mod 4), so
    that every duplicate of a row shares it.  Inside one row the largest scale would swallow the rest and the eps-bound
    regime would never be reached.  entry_ids[k] = the id of entry k (original order)."""
    t = torch.randint(-8, 9, (entry_ids.numel(), D), generator=gen).float()
    scale = torch.tensor(SCALES, dtype=torch.float32)[entry_ids % len(SCALES)]
    return t * scale.view(-1, 1)


def entry_ids(ids_sorted, perm):
    """ids in original entry order out of the sorted ids and perm (sorted position -> original entry)."""
    out = torch.empty_like(ids_sorted)
    out[perm] = ids_sorted
    return out


# ---- float64 references -----------------------------------------------------------------------------------------------
def adagrad_ref64(kind, p0, steps, lr, eps, lr_decay=0.0, init=0.0, wd=0.0):
    """The rule `kind` of the module docstring in float64.  `steps` is a list of (g, touched, p_after): the coalesced,
    dense-shaped gradient of step t, the bool mask of touched rows (None: all of them) and the fp32 parameter the
    implementation under test held AFTER that step.  Every step starts from the parameter the implementation held before it
    (p0, then the previous p_after); the accumulator runs in its own float64 chain.  One record per step:
    t, u (the reference step, dp ~ u), s, p_before, p_after."""
    assert kind in KINDS
    p_before = p0.detach().cpu().double()
    shape = p_before.shape
    s = torch.full((shape[0],) if kind == "rowwise" else shape, float(init), dtype=torch.float64)
    out = []
    for t, (g, touched, p_after) in enumerate(steps, 1):
        g = g.detach().cpu().double().view(shape)
        p_after = p_after.detach().cpu().double().view(shape)
        clr = lr / (1.0 + (t - 1) * lr_decay)
        if kind == "dense":
            g = g + wd * p_before
            s = s + g * g
            u = -clr * g / (s.sqrt() + eps)
        else:
            if kind == "rowwise":
                s1 = s + (g * g).sum(1) / shape[1]
                u = -clr * g / (s1.sqrt().view(-1, 1) + eps)
            else:
                s1 = s + g * g
                u = -clr * g / (s1.sqrt() + eps)
            if touched is not None:
                rows = touched.cpu()
                sel = rows.view([-1] + [1] * (g.dim() - 1)).expand_as(g)
                u = torch.where(sel, u, torch.zeros_like(u))
                s1 = torch.where(rows if kind == "rowwise" else sel, s1, s)
            s = s1
        out.append(dict(t=t, u=u, s=s, p_before=p_before, p_after=p_after))
        p_before = p_after
    return out


def depth(kind, D, wd=0.0):
    if kind == "rowwise":
        return D + 2
    return 6 if (kind == "dense" and wd != 0) else 2


def c_sum(kind, t, D, wd=0.0):
    return C_SUM * t * depth(kind, D, wd)


def c_step(kind, t, D, wd=0.0):
    return C_STEP


def _worst(err, bound):
    if err.numel() == 0:
        return 0.0
    # no error against a zero bound is ratio 0; any error against a zero bound is inf; a NaN stays a NaN (and fails `<= 1`)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def bound_ratios(kind, rec, s=None, wd=0.0, unit=False):
    """Worst ratio to each bound of the module docstring for one adagrad_ref64 record: {"step": ..} plus "sum" when the
    implementation's accumulator after that step is given.  A ratio above 1 (or a NaN) is outside the bound.  unit=True puts
    every constant at 1 (the measurement of the docstring)."""
    t, D = rec["t"], rec["u"].shape[1] if rec["u"].dim() > 1 else 1
    cs, ct = (t * depth(kind, D, wd), 1) if unit else (c_sum(kind, t, D, wd), c_step(kind, t, D, wd))
    dp = rec["p_after"] - rec["p_before"]
    bound = ct * EPS32 * rec["u"].abs() + 2 * EPS32 * torch.maximum(rec["p_before"].abs(), rec["p_after"].abs())
    out = {"step": _worst((dp - rec["u"]).abs(), bound)}
    if s is not None:
        out["sum"] = _worst((s.detach().cpu().double().view(rec["s"].shape) - rec["s"]).abs(), cs * EPS32 * rec["s"])
    return out


def fold(worst, new):
    for k, r in new.items():
        if k not in worst or math.isnan(r) or r > worst[k]:          # (a NaN sticks: nothing compares above it)
            worst[k] = r
    return worst


def worst_ratios(kind, p0, steps, sums, lr, eps, lr_decay=0.0, init=0.0, wd=0.0, unit=False):
    """max over the steps of bound_ratios(); sums = the implementation's accumulator after each step (or None entries)."""
    worst = {}
    for rec, s in zip(adagrad_ref64(kind, p0, steps, lr, eps, lr_decay, init, wd), sums):
        fold(worst, bound_ratios(kind, rec, s, wd, unit))
    return worst


# ---- fp32 implementations on the CPU: the right rules and four wrong ones --------------------------------------------
VARIANTS = ("square_then_sum", "eps_in_root", "stale_sum", "row_sum_not_mean")


def variants_of(kind, D):
    """The mistakes that exist for a rule: the dense rule has no duplicates to square early, and a row's sum IS its mean at
    D = 1."""
    out = ["eps_in_root", "stale_sum"]
    if kind != "dense":
        out.append("square_then_sum")
    if kind == "rowwise" and D > 1:
        out.append("row_sum_not_mean")
    return out


def adagrad_fp32(kind, p0, grads, lr, eps, lr_decay=0.0, init=0.0, wd=0.0, variant=None):
    """The three rules in fp32 torch ops (the row-wise sum over d in index order).  grads: for "sparse" / "rowwise" a list of
    (ids, vals) — the UNCOALESCED row-form gradient, ids in [0, N) —, for "dense" a list of tensors.  variant None is the
    right rule; the others are the mistakes the bounds have to catch: the squares of the duplicates summed in place of the
    square of their sum (what an atomic scatter computes); eps inside the root; the step taken with the accumulator from
    before this step's add; the row's sum of squares not divided by D.  Returns [(p_after, s)] per step."""
    assert kind in KINDS and (variant is None or variant in VARIANTS)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)    # noqa: E731
    p = p0.detach().cpu().float().clone()
    N = p.shape[0]
    s = torch.full((N,) if kind == "rowwise" else p.shape, float(init), dtype=torch.float32)
    out = []
    for t, grad in enumerate(grads, 1):
        clr = f32(lr / (1.0 + (t - 1) * lr_decay))
        if kind == "dense":
            g = grad.detach().cpu().float().view(p.shape) + f32(wd) * p
            sq, touched = g * g, None
        else:
            ids, vals = grad
            vals = vals.detach().cpu().float().view(ids.numel(), -1)
            g = torch.zeros(N, vals.shape[1]).index_add_(0, ids, vals)
            sq = torch.zeros(N, vals.shape[1]).index_add_(0, ids, vals * vals) if variant == "square_then_sum" else g * g
            g, sq = g.view(p.shape), sq.view(p.shape)
            touched = torch.zeros(N, dtype=torch.bool)
            touched[ids] = True
        if kind == "rowwise":
            ss = torch.zeros(N)
            for d in range(p.shape[1]):
                ss = ss + sq[:, d]
            add = ss if variant == "row_sum_not_mean" else ss / f32(float(p.shape[1]))
        else:
            add = sq
        s1 = s + add
        root = s if variant == "stale_sum" else s1
        den = (root + f32(eps)).sqrt() if variant == "eps_in_root" else root.sqrt() + f32(eps)
        p1 = p - clr * (g / (den.view(-1, 1) if kind == "rowwise" else den))
        if touched is not None:
            sel = touched.view([-1] + [1] * (p.dim() - 1)).expand_as(p)
            p1 = torch.where(sel, p1, p)
            s1 = torch.where(touched if kind == "rowwise" else sel, s1, s)
        p, s = p1, s1
        out.append((p.clone(), s.clone()))
    return out


def skewed_ids(N, n, gen):
    """n ids in [0, N) with hot rows (many duplicates) and rows left out."""
    return (N * torch.rand(n, generator=gen).pow(3)).long().clamp_(max=N - 1)


def coalesced(ids, vals, N):
    """(G float64[N, D], touched bool[N]) of an uncoalesced row-form gradient with valid ids."""
    vals = vals.detach().cpu().double().view(ids.numel(), -1)
    touched = torch.zeros(N, dtype=torch.bool)
    touched[ids] = True
    return torch.zeros(N, vals.shape[1], dtype=torch.float64).index_add_(0, ids, vals), touched

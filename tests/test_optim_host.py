"""No GPU: the float64 Adam reference and its bounds (tests/optim_helpers.py) accept torch's own fp32 CPU optimizers and
reject four plausible mistakes by a wide margin, and the run layouts have the pass edges they document."""
import pytest
import torch

import optim_helpers as oh

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
WIDTHS = (1, 4, 8, 16)
N = 64


def _sparse_inputs(D, steps):
    gen = torch.Generator().manual_seed(100 + D)
    p0 = torch.randn(N, D, generator=gen)
    grads = []
    for _ in range(steps):
        rows = (N * torch.rand(300, generator=gen).pow(2)).long().clamp_(max=N - 1)       # duplicates, and rows left out
        vals = oh.scaled_ints((300, D), gen)
        touched = torch.zeros(N, dtype=torch.bool)
        touched[rows] = True
        grads.append((rows, vals, torch.zeros(N, D).index_add_(0, rows, vals), touched))
    return p0, grads


def _dense_inputs(D, steps):
    gen = torch.Generator().manual_seed(200 + D)
    p0 = oh.dense_params((16 * N, D), gen)          # (with weight decay: parameters whose decay term cannot cancel g)
    return p0, [oh.scaled_ints((16 * N, D), gen) for _ in range(steps)]


def _torch_sparse(D, steps):
    p0, grads = _sparse_inputs(D, steps)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SparseAdam([p], lr=LR, betas=BETAS, eps=EPS)
    trail = []
    for rows, vals, _, _ in grads:
        p.grad = torch.sparse_coo_tensor(rows.view(1, -1), vals, (N, D))
        opt.step()
        trail.append((p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()))
    return p0, [(g, touched) for _, _, g, touched in grads], trail


def _torch_dense(D, steps, wd):
    p0, grads = _dense_inputs(D, steps)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    trail = []
    for g in grads:
        p.grad = g.clone()
        opt.step()
        trail.append((p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()))
    return p0, [(g, None) for g in grads], trail


def _ratios(kind, p0, grads, trail, wd=0.0):
    steps = [(g, touched, p_after) for (g, touched), (p_after, _, _) in zip(grads, trail)]
    return oh.worst_ratios(kind, p0, steps, [(m, v) for _, m, v in trail], LR, BETAS, EPS, wd)


@pytest.mark.parametrize("D", WIDTHS)
def test_bounds_accept_torch_fp32_optimizers(D):
    steps = 4 + D % 3
    worst = {"sparse": _ratios("sparse", *_torch_sparse(D, steps))}
    for wd in (0.0, 1e-3, 1e-2):
        worst[f"dense wd={wd}"] = _ratios("dense", *_torch_dense(D, steps, wd), wd=wd)
    print(f"D={D} steps={steps}: " + "; ".join(f"{k}: " + " ".join(f"{b}={r:.3f}" for b, r in w.items())
                                                for k, w in worst.items()))
    for k, w in worst.items():
        for b, r in w.items():
            assert r <= 1.0, f"torch's fp32 {k} is {r:.2f}x the {b} bound away from the float64 rule (D={D})"


@pytest.mark.parametrize("D", WIDTHS)
def test_own_fp32_rule_is_accepted_like_torchs(D):
    """adam_fp32(variant=None), the base the wrong variants are cut from, is itself inside the bounds."""
    p0, grads, _ = _torch_sparse(D, 4)
    assert max(_ratios("sparse", p0, grads, oh.adam_fp32("sparse", p0, grads, LR, BETAS, EPS)).values()) <= 1.0
    for wd in (0.0, 1e-3, 1e-2):
        p0, grads, _ = _torch_dense(D, 4, wd)
        assert max(_ratios("dense", p0, grads, oh.adam_fp32("dense", p0, grads, LR, BETAS, EPS, wd), wd).values()) <= 1.0


@pytest.mark.parametrize("variant", oh.VARIANTS)
@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("D", WIDTHS)
def test_bounds_reject_wrong_variants_tenfold(D, kind, variant):
    p0, grads, _ = _torch_sparse(D, 4) if kind == "sparse" else _torch_dense(D, 4, 0.0)
    worst = _ratios(kind, p0, grads, oh.adam_fp32(kind, p0, grads, LR, BETAS, EPS, variant=variant))
    print(f"D={D} {kind} {variant}: " + " ".join(f"{b}={r:.3g}" for b, r in worst.items()))
    assert max(worst.values()) >= 10.0, f"{variant} ({kind}, D={D}) passes: worst ratios {worst}"


@pytest.mark.parametrize("RS", [1, 2, 4, 8, 16, 32, 64])
def test_run_layout_has_its_documented_edges(RS):
    N = 1000
    want_mod = {"edges-0": 0, "edges-1": 1 % RS, "edges-m1": RS - 1}
    for which in oh.LAYOUTS:
        lay = oh.run_layout(RS, N, which)
        ids, perm, n, e = lay.ids, lay.perm, lay.n, lay.edges
        assert ids.dtype == torch.int64 and ids.numel() == n == perm.numel()
        assert bool((ids[1:] >= ids[:-1]).all()), "ids are not sorted"
        assert torch.equal(torch.sort(perm)[0], torch.arange(n)), "perm is not a permutation"
        assert n <= 1 or not torch.equal(perm, torch.arange(n)), "perm is the identity"
        valid = ids[(ids >= 0) & (ids < N)]
        assert valid.unique().numel() < N, "no row is left out"

        def run(name):          # (start, length, id) of a named run, checked to be a maximal run of one id
            start, length = e[name]
            assert bool((ids[start:start + length] == ids[start]).all()), name
            assert start == 0 or ids[start - 1] != ids[start], name
            assert start + length == n or ids[start + length] != ids[start], name
            return start, length, int(ids[start])

        if which == "one":
            assert n == 1 and 0 <= int(ids[0]) < N
        elif which == "short":
            assert n == RS - 1
        elif which == "tail":
            start, length, rid = run("tail_run")
            assert start % RS == RS // 2 and length == 2 * RS + RS // 2 + 1 and start + length == n and 0 <= rid < N
        else:
            assert n % RS == want_mod[which]
            assert 0 in valid and N - 1 in valid
            start, length = e["neg_front"]
            assert start == 0 and ids[:length].tolist() == [-7, -3] + [-1] * (RS + 1) and ids[length] >= 0
            start, length, _ = run("aligned_rs")
            assert start % RS == 0 and length == RS
            start, length, _ = run("ends_on_last")
            assert (start + length) % RS == 0 and length == max(2, RS // 2)
            start, length, _ = run("single_on_last")
            assert start % RS == RS - 1 and length == 1
            start, length, _ = run("straddle_2")
            assert start % RS == RS - 1 and length == 2
            start, length, _ = run("aligned_2rs")
            assert start % RS == 0 and length == 2 * RS
            start, length, _ = run("long_mid")
            assert start % RS == RS // 2 and length == RS * (RS + 2) + 3
            # pieces the joining wave walks: the head's pass, then one per following pass — more than its RS lane groups
            assert (start + length - 1) // RS - start // RS + 1 > RS + 1
            start, length = e["back_invalid"]
            assert start + length == n and ids[start:].tolist() == [N, N] + [N + 5] * (RS + 1)
            assert start // RS != (n - 1) // RS, "the invalid ids at the back do not cross a pass end"
            for name in ("aligned_rs", "ends_on_last", "single_on_last", "straddle_2", "aligned_2rs", "long_mid"):
                assert 0 <= run(name)[2] < N


def test_coalesce_ref_and_crossing_ids():
    lay = oh.run_layout(4, 200, "edges-1")
    vals = torch.randint(-8, 9, (lay.n, 3), generator=torch.Generator().manual_seed(0)).float()
    G, present = oh.coalesce_ref(lay.ids, lay.perm, vals, 200)
    rows = torch.empty(lay.n, dtype=torch.int64)
    rows[lay.perm] = lay.ids                                     # the ids in the original entry order
    ok = (rows >= 0) & (rows < 200)
    assert torch.equal(G, torch.zeros(200, 3, dtype=torch.float64).index_add_(0, rows[ok], vals[ok].double()))
    assert torch.equal(present, torch.bincount(rows[ok], minlength=200) > 0) and not bool(present.all())
    ids, (a, b) = oh.crossing_ids(16, 50, 16 * 8192 + 100, 8192, torch.Generator().manual_seed(1))
    assert bool((ids[1:] >= ids[:-1]).all()) and a < 16 * 8192 - 1 and b > 16 * 8192 and bool((ids[a:b] == ids[a]).all())

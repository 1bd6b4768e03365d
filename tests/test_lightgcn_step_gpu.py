"""GPU: the LightGCN step either side of the propagation — fused BPR loss and the
mask + top-k scoring tail — against the oracle's restatements of src/losses.py:6-22 and
src/trainer/lightgcn.py:122-138."""
import pytest
import torch

from conftest import assert_close, load_golden

from oracle import reference_ops as ro
from recsys_benchmark_amd import _lib
from recsys_benchmark_amd.lightgcn import score_topk, train_items_csr
from recsys_benchmark_amd.losses import bpr_loss, bpr_loss_multi, bpr_loss_rows, first_occurrence, info_nce

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _misaligned(t):
    """The same values on the device as a contiguous matrix whose base lies one float past a 16-byte boundary: (leaf, view)."""
    flat = torch.cat([torch.zeros(1), t.detach().reshape(-1)]).to(DEV).requires_grad_(True)
    return flat, flat[1:].view(t.shape)


def _check_bpr_loss(B, D, misaligned=False):
    g = torch.Generator().manual_seed(B + D)
    u, p, n = (torch.randn(B, D, generator=g, requires_grad=True) for _ in range(3))
    ref = ro.bpr_loss(u, p, n)
    (ref * 1.7).backward()
    if misaligned:
        (hu, hp, hn), views = zip(*(_misaligned(t) for t in (u, p, n)))
        assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
        out = bpr_loss(*views)
    else:
        hu, hp, hn = (t.detach().to(DEV).requires_grad_(True) for t in (u, p, n))
        out = bpr_loss(hu, hp, hn)
    (out * 1.7).backward()
    # fp32 row dots of length D and a mean over B in a different order
    assert_close(out, ref, 1e-5, 1e-6, "loss")
    for a, b, name in ((hu, u, "du"), (hp, p, "dp"), (hn, n, "dn")):
        assert_close(a.grad[1:].view(B, D) if misaligned else a.grad, b.grad, 1e-5, 1e-7, name)


# 4 samples per workgroup in the any-D form, 64 / (D / 4) per wave in the float4 form (D / 4 a power of two <= 64); the
# last workgroup's 256 threads stride over the partials, the grid is capped at 2048 workgroups
@pytest.mark.parametrize("B,D", [(1, 64), (7, 5), (2048, 64), (5000, 16),
                                 (4200, 64), (1100, 5),        # 263 / 275 workgroups: a second trip over the partials
                                 (33000, 64), (8200, 5),       # past the grid cap: the batch loop strides
                                 (64, 4), (64, 8), (64, 32), (64, 128), (64, 256),      # the other float4 widths
                                 (64, 70),                     # any-D, two elements per lane
                                 (64, 260)])                   # a multiple of 4 above 256: any-D
def test_bpr_loss_matches_reference(B, D):
    _check_bpr_loss(B, D)


def test_bpr_loss_matches_reference_on_tables_off_the_16_byte_boundary():
    """Contiguous [65, 64] tables that start one float past a 16-byte boundary: the any-D form takes them."""
    _check_bpr_loss(65, 64, misaligned=True)


def test_bpr_loss_is_stable_for_huge_margins():
    u = torch.tensor([[100.0, 0.0], [-100.0, 0.0], [0.0, 0.0]])
    p = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    n = torch.zeros(3, 2)
    ref = ro.bpr_loss(u, p, n)
    out = bpr_loss(u.to(DEV), p.to(DEV), n.to(DEV))
    assert torch.isfinite(out) and abs(float(out) - float(ref)) < 1e-4


def test_bpr_loss_rows_equals_index_select_path():
    """The trainer's three index_selects fused in (src/trainer/lightgcn.py:395-399); users / items repeat."""
    g = torch.Generator().manual_seed(3)
    nu, ni, D, B = 300, 500, 64, 2048
    U = torch.randn(nu, D, generator=g, requires_grad=True)
    I = torch.randn(ni, D, generator=g, requires_grad=True)
    users = torch.randint(0, nu, (B,), generator=g)
    pos, neg = torch.randint(0, ni, (B,), generator=g), torch.randint(0, ni, (B,), generator=g)
    ref = ro.bpr_loss(torch.index_select(U, 0, users), torch.index_select(I, 0, pos), torch.index_select(I, 0, neg))
    ref.backward()
    hU, hI = U.detach().to(DEV).requires_grad_(True), I.detach().to(DEV).requires_grad_(True)
    out = bpr_loss_rows(hU, hI, users.to(DEV), pos.to(DEV), neg.to(DEV))
    out.backward()
    assert_close(out, ref, 1e-5, 1e-6, "loss")
    # duplicates are summed with float atomics (order varies): absolute floor for cancelling sums
    assert_close(hU.grad, U.grad, 1e-4, 1e-7, "dU")
    assert_close(hI.grad, I.grad, 1e-4, 1e-7, "dI")


@pytest.mark.parametrize("seed_kind", ["unit", "scaled"])
def test_bpr_loss_rows_with_the_regulariser_joined_in_and_the_tables_as_one_matrix(seed_kind):
    """bpr_loss_rows(..., plus=reg, plus_weight=w) = bpr + w * reg (src/trainer/lightgcn.py:401-404) out of the BPR launch, the
    bare BPR term beside it; user and item tables given as the two row segments of ONE matrix (what LightGCN's propagation
    returns) get their gradients as views of one zero-filled buffer.  Seeded with the resident unit scalar (the trainer's
    way: d loss / d reg is then a kept constant) and with an ordinary upstream gradient."""
    from recsys_benchmark_amd.losses import unit_scalar

    g = torch.Generator().manual_seed(11)
    nu, ni, D, B, w = 300, 500, 64, 2048, 1e-2
    both = torch.randn(nu + ni, D, generator=g)
    users = torch.randint(0, nu, (B,), generator=g)
    pos, neg = torch.randint(0, ni, (B,), generator=g), torch.randint(0, ni, (B,), generator=g)
    r = torch.tensor(3.25, requires_grad=True)
    cb = both.clone().requires_grad_(True)
    U, I = cb[:nu], cb[nu:]
    bare_ref = ro.bpr_loss(torch.index_select(U, 0, users), torch.index_select(I, 0, pos), torch.index_select(I, 0, neg))
    ref = bare_ref + w * (r * r)
    up = 1.0 if seed_kind == "unit" else 0.37
    (ref * up).backward()
    hb = both.to(DEV).requires_grad_(True)
    hr = r.detach().to(DEV).requires_grad_(True)
    hU, hI = hb[:nu], hb[nu:]
    total, bare = bpr_loss_rows(hU, hI, users.to(DEV), pos.to(DEV), neg.to(DEV), plus=hr * hr, plus_weight=w, return_parts=True)
    assert not bare.requires_grad
    if seed_kind == "unit":
        total.backward(unit_scalar(DEV))
    else:
        (total * up).backward()
    assert_close(total, ref, 1e-5, 1e-6, "bpr + w reg")
    assert_close(bare, bare_ref, 1e-5, 1e-6, "bare bpr")
    assert_close(hb.grad, cb.grad, 1e-4, 1e-7, "d tables")
    assert_close(hr.grad, r.grad, 1e-6, 1e-9, "d reg")


def test_bpr_and_reg_rows_out_of_range_ids_touch_no_memory_and_are_flagged():
    """index_select raises in the reference (src/trainer/lightgcn.py:395-397); here a bad triple reads and adds nothing,
    counts as zero rows, and the sticky word turns into IndexError at the next check."""
    from recsys_benchmark_amd.losses import reg_loss_rows

    g = torch.Generator().manual_seed(5)
    nu, ni, D, B = 50, 70, 64, 256
    U = torch.randn(nu, D, generator=g)
    I = torch.randn(ni, D, generator=g)
    users = torch.randint(0, nu, (B,), generator=g)
    pos, neg = torch.randint(0, ni, (B,), generator=g), torch.randint(0, ni, (B,), generator=g)
    bad_b = [3, 77, 200]
    users_bad, pos_bad, neg_bad = users.clone(), pos.clone(), neg.clone()
    users_bad[3], pos_bad[77], neg_bad[200] = nu + 10**9, -1, ni
    keep = torch.ones(B, dtype=torch.bool)
    keep[bad_b] = False
    for fn in (bpr_loss_rows, reg_loss_rows):
        hU, hI = U.to(DEV).requires_grad_(True), I.to(DEV).requires_grad_(True)
        out = fn(hU, hI, users_bad.to(DEV), pos_bad.to(DEV), neg_bad.to(DEV))
        out.backward()
        with pytest.raises(IndexError):
            _lib.check_index_errors()
        # the same batch with the bad triples replaced by zero rows (an extra all-zero row in each table)
        U0, I0 = torch.cat([U, torch.zeros(1, D)]).requires_grad_(True), torch.cat([I, torch.zeros(1, D)]).requires_grad_(True)
        u2, p2, n2 = (torch.where(keep, t, torch.full_like(t, z)) for t, z in ((users, nu), (pos, ni), (neg, ni)))
        if fn is bpr_loss_rows:
            ref = ro.bpr_loss(U0[u2], I0[p2], I0[n2])
        else:
            ref = (U0[u2].norm(2).pow(2) + I0[p2].norm(2).pow(2) + I0[n2].norm(2).pow(2)) / (2 * B)
        ref.backward()
        assert_close(out, ref, 1e-5, 1e-6, fn.__name__)
        assert_close(hU.grad, U0.grad[:nu], 1e-4, 1e-7, "dU")
        assert_close(hI.grad, I0.grad[:ni], 1e-4, 1e-7, "dI")
    _lib.check_index_errors()


def _graph(nu, ni, gen, max_items=40):
    return {u: torch.randperm(ni, generator=gen)[: int(torch.randint(0, max_items, (1,), generator=gen))].tolist()
            for u in range(nu)}


@pytest.mark.parametrize("nu,ni,B,k", [(50, 300, 17, 20), (200, 5000, 64, 20), (40, 25, 9, 20), (64, 38048, 32, 20),
                                        (30, 1000, 30, 1), (30, 1000, 8, 256)])
def test_score_topk_matches_reference_loop(nu, ni, B, k):
    gen = torch.Generator().manual_seed(nu + ni + k)
    D = 64
    ue, ie = torch.randn(nu, D, generator=gen), torch.randn(ni, D, generator=gen)
    graph = _graph(nu, ni, gen, max_items=min(40, max(1, ni - k)))
    users = torch.randint(0, nu, (B,), generator=gen)
    ref = ro.masked_topk(ue, ie, users, graph, k)
    csr = train_items_csr(graph, nu, DEV)
    got = score_topk(ue.to(DEV), ie.to(DEV), users.to(DEV), k, csr).cpu()
    # integer output, but two scores closer than the fp32 dot-product error (different summation order on the
    # MFMA path) may legitimately swap: wherever the indices differ the reference scores must be that close
    scores = ue[users] @ ie.T
    same = got == ref
    if not bool(same.all()):
        a = torch.gather(scores, 1, got)[~same]
        b = torch.gather(scores, 1, ref)[~same]
        assert_close(a, b, 1e-5, 1e-4, "swapped neighbours")
    assert float(same.float().mean()) > 0.99
    for i, u in enumerate(users.tolist()):                                  # no train item ever ranks
        assert not set(got[i].tolist()) & set(graph[u])
    no_filter = score_topk(ue.to(DEV), ie.to(DEV), users.to(DEV), k, None).cpu()
    ref_nf = ro.masked_topk(ue, ie, users, graph, k, filter_item_on_train=False)
    assert float((no_filter == ref_nf).float().mean()) > 0.99


def test_topk_kernel_is_exact_on_given_scores_incl_ties_and_many_masked():
    """The selection itself on identical floats: bit-exact vs torch.topk where scores are distinct; with
    ties the order is score descending then index ascending; rows that are almost entirely -inf."""
    gen = torch.Generator().manual_seed(1)
    B, I, k = 12, 3000, 20
    s = torch.randn(B, I, generator=gen)
    s[3] = torch.round(s[3] * 2) / 2                                        # massive ties
    s[4] = 0.0                                                              # all equal
    s[5, 7:] = float("-inf")                                                # fewer finite entries than k
    dev = s.to(DEV)
    out = torch.empty(B, k, dtype=torch.int64, device=DEV)
    val = torch.empty(B, k, device=DEV)
    _lib.check(_lib.load().mi_mask_topk_rows(dev.data_ptr(), I, B, I, None, None, None, k, out.data_ptr(),
                                             val.data_ptr(), _lib.stream_ptr(DEV)))
    out, val = out.cpu(), val.cpu()
    tv, ti = torch.topk(s, k)
    assert torch.equal(val, tv)                                             # values always agree
    distinct = [0, 1, 2, 6, 7, 8, 9, 10, 11]
    assert torch.equal(out[distinct], ti[distinct])
    for r in (3, 4, 5):                                                     # the stated total order
        order = sorted(range(I), key=lambda j: (-float(s[r, j]), j))[:k]
        assert out[r].tolist() == order


def test_reg_loss_rows_matches_reference_formula_and_model_uses_it():
    """LightGCN.get_reg_loss (src/models/lightgcn.py:90-100) on plain tables: fused kernel vs the oracle's formula,
    value and both table gradients (rows repeat; positives and negatives share the item table)."""
    from recsys_benchmark_amd.lightgcn import LightGCN
    from recsys_benchmark_amd.losses import reg_loss_rows

    g = torch.Generator().manual_seed(11)
    nu, ni, D, B = 300, 500, 64, 2048
    U = torch.randn(nu, D, generator=g, requires_grad=True)
    I = torch.randn(ni, D, generator=g, requires_grad=True)
    users = torch.randint(0, nu, (B,), generator=g)
    pos, neg = torch.randint(0, ni, (B,), generator=g), torch.randint(0, ni, (B,), generator=g)
    ref = ro.l2_reg_loss(U[users], I[pos], I[neg])
    (ref * 3.0).backward()
    hU, hI = U.detach().to(DEV).requires_grad_(True), I.detach().to(DEV).requires_grad_(True)
    out = reg_loss_rows(hU, hI, users.to(DEV), pos.to(DEV), neg.to(DEV))
    (out * 3.0).backward()
    assert_close(out, ref, 1e-5, 1e-5, "reg loss")              # a sum of 393 216 squares in a different order
    assert_close(hU.grad, U.grad, 1e-4, 1e-7, "dU")
    assert_close(hI.grad, I.grad, 1e-4, 1e-7, "dI (positives + negatives)")
    model = LightGCN(nu, ni, num_layers=1, hidden_size=D).to(DEV)
    with torch.no_grad():
        model.user_emb_table._emb_module.weight.copy_(U)
        model.item_emb_table._emb_module.weight.copy_(I)
    got = model.get_reg_loss(users.to(DEV), pos.to(DEV), neg.to(DEV))
    assert_close(got, ref, 1e-5, 1e-5, "LightGCN.get_reg_loss")
    got.backward()
    assert_close(model.user_emb_table._emb_module.weight.grad * 3.0, U.grad, 1e-4, 1e-7)


def _reg_case(B, D, integers):
    """(U, I, users, pos, neg) on the CPU; integers: table entries from {0, +-1, +-2}."""
    g = torch.Generator().manual_seed(B + D)
    nu, ni = 300, 500
    if integers:
        U, I = (torch.randint(-2, 3, (r, D), generator=g).float() for r in (nu, ni))
    else:
        U, I = torch.randn(nu, D, generator=g), torch.randn(ni, D, generator=g)
    users = torch.randint(0, nu, (B,), generator=g)
    pos, neg = torch.randint(0, ni, (B,), generator=g), torch.randint(0, ni, (B,), generator=g)
    return U, I, users, pos, neg


def _reg_both_ways(U, I, users, pos, neg):
    """reg_loss_rows on the device and the formula in float64: (out, dU, dI), (ref, dU, dI)."""
    from recsys_benchmark_amd.losses import reg_loss_rows

    U64, I64 = U.double().requires_grad_(True), I.double().requires_grad_(True)
    ref = (U64[users].pow(2).sum() + I64[pos].pow(2).sum() + I64[neg].pow(2).sum()) / (2 * users.numel())
    ref.backward()
    hU, hI = U.to(DEV).requires_grad_(True), I.to(DEV).requires_grad_(True)
    out = reg_loss_rows(hU, hI, users.to(DEV), pos.to(DEV), neg.to(DEV))
    out.backward()
    _lib.check_index_errors()
    return (out.cpu(), hU.grad.cpu(), hI.grad.cpu()), (ref.detach(), U64.grad, I64.grad)


@pytest.mark.parametrize("B,D", [(8192, 64), (2048, 5)])      # 512 workgroups in the float4 and in the any-D form
def test_reg_loss_rows_is_exact_on_small_integer_tables(B, D):
    """Entries from {0, +-1, +-2}: every partial sum of squares is an integer below 2^24 (at most 3 * 8192 * 64 * 4), so
    exact in fp32 in any order, and B is a power of two, so the division by 2B and the gradient rows (integer / B, added
    up with atomics) are exact too: the kernels' results equal the float64 formula bit for bit."""
    got, ref = _reg_both_ways(*_reg_case(B, D, integers=True))
    for a, b, name in zip(got, ref, ("reg loss", "dU", "dI")):
        assert torch.equal(a, b.float()), name


@pytest.mark.parametrize("D", [4, 8, 32, 128, 256, 70, 260])
def test_reg_loss_rows_matches_float64_at_every_width(D):
    got, ref = _reg_both_ways(*_reg_case(64, D, integers=False))
    assert_close(got[0], ref[0].float(), 1e-5, 1e-5, "reg loss")
    assert_close(got[1], ref[1].float(), 1e-4, 1e-7, "dU")
    assert_close(got[2], ref[2].float(), 1e-4, 1e-7, "dI (positives + negatives)")


@pytest.mark.parametrize("B,D", [(1100, 5), (4200, 64)])      # any-D form (275 workgroups), float4 form (263)
def test_ticket_is_rearmed_three_calls_on_one_kept_workspace_agree_bit_for_bit(B, D):
    """The last workgroup leaves the ticket word zero, so the kept workspace (losses.ARMED_WORKSPACES) of bpr_loss_rows,
    reg_loss_rows and reg_prune_loss_rows serves the next launch as it is; all three launch more than 256 workgroups here
    and sum in a fixed order.  info_nce (300 workgroups) takes a fresh workspace and zeroes its ticket per call: for it
    only the fixed order is on trial."""
    from recsys_benchmark_amd import losses

    assert losses.ARMED_WORKSPACES
    g = torch.Generator().manual_seed(7)
    nu, ni = 300, 500
    U, I = torch.randn(nu, D, generator=g).to(DEV), torch.randn(ni, D, generator=g).to(DEV)
    users = torch.randint(0, nu, (B,), generator=g).to(DEV)
    pos, neg = torch.randint(0, ni, (B,), generator=g).to(DEV), torch.randint(0, ni, (B,), generator=g).to(DEV)
    v = torch.randn(300, 64, generator=g).to(DEV)
    calls = {"bpr_loss_rows": lambda: bpr_loss_rows(U, I, users, pos, neg),
             "reg_loss_rows": lambda: losses.reg_loss_rows(U, I, users, pos, neg),
             "reg_prune_loss_rows": lambda: torch.stack(losses.reg_prune_loss_rows(U * 0.01, I * 0.01, users, pos, neg)),
             "info_nce": lambda: info_nce(v, v, 0.2)}
    for name, call in calls.items():
        first, second, third = call(), call(), call()
        assert torch.isfinite(first).all(), name
        assert torch.equal(first, second) and torch.equal(first, third), name
    _lib.check_index_errors()


# ------------------------------------------------------------------ info_nce / bpr_loss_multi (src/losses.py:25-68)
def test_info_nce_and_multi_bpr_match_the_reference_vectors():
    g = load_golden("losses")
    for tag in ("cos_t02", "cos_t1", "dot_t05"):
        v1, v2 = (g.t(f"{tag}/{k}").to(DEV).requires_grad_(True) for k in ("v1", "v2"))
        loss = info_nce(v1, v2, float(g[f"{tag}/temperature"]), bool(g[f"{tag}/b_cos"]))
        # fp32, n=37 terms per softmax row in a different order: rtol 1e-5
        assert_close(loss, g.t(f"{tag}/loss"), 1e-5, 1e-6, tag)
        loss.backward()
        assert_close(v1.grad, g.t(f"{tag}/grad_v1"), 1e-4, 1e-6, tag + " grad_v1")
        assert_close(v2.grad, g.t(f"{tag}/grad_v2"), 1e-4, 1e-6, tag + " grad_v2")
    v = g.t("self/v").to(DEV).requires_grad_(True)
    loss = info_nce(v, v, 0.2)
    assert_close(loss, g.t("self/loss"), 1e-5, 1e-6, "self")
    loss.backward()
    assert_close(v.grad, g.t("self/grad_v"), 1e-4, 1e-6, "self grad")
    u, p, n = (g.t("multi/" + k).to(DEV).requires_grad_(True) for k in "upn")
    loss = bpr_loss_multi(u, p, n)
    assert_close(loss, g.t("multi/loss"), 1e-5, 1e-6, "multi")
    loss.backward()
    for k, t in zip("upn", (u, p, n)):
        assert_close(t.grad, g.t("multi/grad_" + k), 1e-4, 1e-6, "multi grad_" + k)


@pytest.mark.parametrize("n,D,temp,b_cos", [(1, 8, 0.2, True), (130, 64, 0.2, True), (1000, 64, 0.2, True),
                                             (513, 20, 1.0, False), (2048, 64, 0.2, True)])
def test_info_nce_matches_oracle(n, D, temp, b_cos):
    gen = torch.Generator().manual_seed(n + D)
    v1 = (torch.randn(n, D, generator=gen) * (1.0 if b_cos else 0.3)).requires_grad_(True)
    v2 = (torch.randn(n, D, generator=gen) * (1.0 if b_cos else 0.3)).requires_grad_(True)
    ref = ro.info_nce(v1, v2, temp, b_cos)
    (ref * 0.5).backward()
    h1, h2 = (t.detach().to(DEV).requires_grad_(True) for t in (v1, v2))
    out = info_nce(h1, h2, temp, b_cos)
    (out * 0.5).backward()
    # exact-fp32 MFMA scores vs the CPU's blocked sgemm, log-sum-exp over n terms in another order
    assert_close(out, ref, 1e-5, 1e-5, "loss")
    assert_close(h1.grad, v1.grad, 1e-4, 1e-6 / max(1.0, n / 100), "grad_v1")
    assert_close(h2.grad, v2.grad, 1e-4, 1e-6 / max(1.0, n / 100), "grad_v2")


def test_info_nce_same_view_and_degenerate_rows():
    gen = torch.Generator().manual_seed(5)
    v = torch.randn(300, 64, generator=gen)
    v[7] = 0.0                                     # F.normalize clamps the norm at 1e-12: the row stays zero
    v = v.requires_grad_(True)
    ref = ro.info_nce(v, v, 0.2)
    ref.backward()
    h = v.detach().to(DEV).requires_grad_(True)
    out = info_nce(h, h, 0.2)
    out.backward()
    assert_close(out, ref, 1e-5, 1e-5, "loss")
    # the zero row's gradient is dy / 1e-12: compare it on that scale, the others on theirs
    keep = torch.ones(300, dtype=torch.bool)
    keep[7] = False
    assert_close(h.grad[keep.to(DEV)], v.grad[keep], 1e-4, 1e-6, "grad")
    assert_close(h.grad[7] * 1e-12, v.grad[7] * 1e-12, 1e-3, 1e-6, "grad of the clamped row")
    with pytest.raises(ValueError):
        info_nce(h, h[:10], 0.2)


@pytest.mark.parametrize("n,D", [(9, 8), (517, 64), (4096, 64)])
def test_masked_info_nce_equals_info_nce_of_the_selected_rows(n, D):
    gen = torch.Generator().manual_seed(n)
    v = torch.randn(n, D, generator=gen)
    m = torch.rand(n, generator=gen) < 0.7
    m[0] = True
    sel = v[m].clone().requires_grad_(True)
    ref = ro.info_nce(sel, sel, 0.2)
    ref.backward()
    h = v.to(DEV).requires_grad_(True)
    out = info_nce(h, h, 0.2, valid=m.to(DEV))
    out.backward()
    assert_close(out, ref, 1e-5, 1e-5, "loss")
    assert_close(h.grad[m.to(DEV)], sel.grad, 1e-4, 1e-6 / max(1.0, n / 100), "grad of the kept rows")
    assert not h.grad[~m.to(DEV)].any(), "a masked row received a gradient"


def test_first_occurrence_selects_each_id_once():
    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 300, (2048,), generator=gen).to(DEV)
    first = first_occurrence(ids, 300)
    assert torch.equal(torch.sort(ids[first])[0], torch.unique(ids))
    # and it is the FIRST position of each id
    pos = torch.arange(2048, device=DEV)[first]
    for i in pos[:50].tolist():
        assert not (ids[:i] == ids[i]).any()

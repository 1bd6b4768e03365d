"""GPU: the device-side routing of the row-sharded lookup (csrc/route.hip + the slot variants of
the gather+FM kernels) against its torch restatement (oracle/sharded_ops.py, pinned by the gloo
world-2 test) — integer outputs bit-exact, fp32 within the stated tolerances — and an emulated
multi-rank exchange on one GPU against the unsharded kernel."""
import pytest
import torch

from conftest import assert_close

import recsys_benchmark_amd as pkg
from oracle.sharded_ops import TorchOps
from recsys_benchmark_amd import _kernels, _lib
from recsys_benchmark_amd.sharded import bucket_capacity, local_num_rows, shard_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("B,F", [(1, 1), (5, 3), (39, 26), (40, 26), (4096, 26), (1000, 39)])
def test_route_matches_restatement_bit_exact(world, B, F):
    g = torch.Generator().manual_seed(B * 131 + F + world)
    dims = torch.randint(1, 5000, (F,), generator=g)
    N = int(dims.sum())
    offsets = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.long), dims[:-1]]), 0)
    x = torch.stack([torch.randint(0, int(d), (B,), generator=g) for d in dims], 1)
    cap = bucket_capacity(B * F, world, 1.25)
    of_ref = torch.zeros(1, dtype=torch.int32)
    send_ref, slot_ref = TorchOps.route_buckets(x, offsets, world, N, cap, of_ref)
    of = _flag()
    send, slot = _kernels.route_buckets(x.to(DEV), offsets.to(DEV), world, N, cap, of)
    assert torch.equal(slot.cpu(), slot_ref)
    assert torch.equal(send.cpu(), send_ref)
    assert int(of.item()) == int(of_ref.item())
    pkg.check_index_errors()


def test_route_int32_ids_no_offsets_and_noncontiguous():
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 977, (64, 7), generator=g, dtype=torch.int32)
    xt = x.t()                                         # non-contiguous view
    for inp in (x, xt):
        ref = TorchOps.route_buckets(inp, None, 4, 977, 200, torch.zeros(1, dtype=torch.int32))
        got = _kernels.route_buckets(inp.to(DEV), None, 4, 977, 200, _flag())
        assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])


def test_route_overflow_goes_to_dump_slot_and_raises_flag():
    x = torch.zeros(300, 1, dtype=torch.int64)          # every lookup hits owner 0
    x[::3] = 5
    cap, world = 64, 4
    of_ref = torch.zeros(1, dtype=torch.int32)
    send_ref, slot_ref = TorchOps.route_buckets(x, None, world, 1000, cap, of_ref)
    of = _flag()
    send, slot = _kernels.route_buckets(x.to(DEV), None, world, 1000, cap, of)
    assert int(of_ref.item()) == 1 and int(of.item()) == 1
    assert torch.equal(slot.cpu(), slot_ref) and torch.equal(send.cpu(), send_ref)
    assert int((slot.cpu() == world * cap).sum()) == int((slot_ref == world * cap).sum()) > 0


def test_route_out_of_range_ids_hit_the_dump_slot_and_the_error_word():
    x = torch.tensor([[3, 10], [-1, 2], [7, 0]], dtype=torch.int64)
    offsets = torch.tensor([0, 8])
    N = 12                                             # 8 + 10 >= N, -1 < 0
    ref = TorchOps.route_buckets(x, offsets, 2, N, 6, torch.zeros(1, dtype=torch.int32))
    got = _kernels.route_buckets(x.to(DEV), offsets.to(DEV), 2, N, 6, _flag())
    assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[0].cpu(), ref[0])
    assert int(got[1][0, 1]) == 12 and int(got[1][1, 0]) == 12
    with pytest.raises(IndexError):
        pkg.check_index_errors()


def test_route_empty_batch():
    send, slot = _kernels.route_buckets(torch.zeros(0, 5, dtype=torch.int64, device=DEV), None, 2, 100, 0, _flag())
    assert send.numel() == 0 and slot.numel() == 0


@pytest.mark.parametrize("D", [4, 8, 16, 64, 256])
def test_gather_pack_rows(D):
    g = torch.Generator().manual_seed(D)
    W, w1 = torch.randn(500, D, generator=g), torch.randn(500, 1, generator=g)
    rows = torch.randint(0, 500, (777,), generator=g)
    ref = TorchOps.gather_pack_rows(rows, W, w1)
    got = _kernels.gather_pack_rows(rows.to(DEV), W.to(DEV), w1.to(DEV))
    assert torch.equal(got.cpu(), ref)                 # copies: bit-exact
    pkg.check_index_errors()


@pytest.mark.parametrize("D,m", [(4, 1), (8, 63), (16, 777), (64, 1000), (256, 5)])
def test_unpack_rows_is_the_two_column_block_copies(D, m):
    g = torch.Generator().manual_seed(D + m)
    packed = torch.randn(m, D + 4, generator=g)
    vals, lin = _kernels.unpack_rows(packed.to(DEV), D)
    ref_vals, ref_lin = TorchOps.unpack_rows(packed, D)
    assert vals.is_contiguous() and lin.is_contiguous()
    assert torch.equal(vals.cpu(), ref_vals) and torch.equal(lin.cpu(), ref_lin)


@pytest.mark.parametrize("B,F,world", [(4096, 26, 8), (4096, 26, 3), (700000, 1, 4)])
def test_route_two_launch_and_three_launch_forms_agree_with_the_restatement(B, F, world):
    """Up to 512 count workgroups (524 288 lookups) the assigning workgroups scan the counts themselves (two launches);
    beyond, a scan launch sits in between (three): both against the torch restatement, bit for bit."""
    g = torch.Generator().manual_seed(B + F + world)
    dims = [int(v) for v in torch.randint(1, 5000, (F,), generator=g)]
    x = torch.stack([torch.randint(0, d, (B,), generator=g) for d in dims], 1)
    offsets = torch.tensor([0] + dims[:-1]).cumsum(0)
    N = sum(dims)
    cap = (B * F) // world + 512
    ref = TorchOps.route_buckets(x, offsets, world, N, cap, torch.zeros(1, dtype=torch.int32))
    got = _kernels.route_buckets(x.to(DEV), offsets.to(DEV), world, N, cap, _flag())
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])


def test_gather_pack_rejects_unsupported_width_loudly():
    with pytest.raises(_lib.MI355XLibraryError):
        _kernels.gather_pack_rows(torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(5, 6, device=DEV),
                                  torch.zeros(5, 1, device=DEV))


def _slot_fm_operands(B, F, D):
    g = torch.Generator().manual_seed(B + F + D)
    S = B * F + 11                                     # some slots stay unused (padding)
    buf = torch.randn(S + 1, D + 4, generator=g) * 0.1        # embedding-like magnitudes
    buf[:, D + 1:] = 0
    buf[S] = 0
    slot = torch.randperm(S, generator=g)[:B * F].view(B, F)
    slot[0, 0] = S                                     # one dropped lookup -> the dump row
    bias = torch.tensor([0.3])
    return g, S, buf, slot, bias


# (4, 20, 64): LPR = 16, four rows per step, five steps -> the generic field loop of the forward and of the backward
@pytest.mark.parametrize("B,F,D", [(1, 1, 16), (33, 26, 16), (64, 39, 16), (17, 100, 8), (9, 5, 64), (4, 20, 64)])
def test_slot_fm_forward_backward(B, F, D):
    g, S, buf, slot, bias = _slot_fm_operands(B, F, D)
    g_emb, g_y = torch.randn(B, F, D, generator=g), torch.randn(B, generator=g)

    rb, rbias = buf.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    e_ref, y_ref = TorchOps.slot_fm(rb, slot, rbias)
    ((e_ref * g_emb).sum() + (y_ref * g_y).sum()).backward()

    hb, hbias = buf.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    e, y = _kernels.slot_fm(hb, slot.to(DEV), hbias)
    ((e * g_emb.to(DEV)).sum() + (y * g_y.to(DEV)).sum()).backward()
    assert torch.equal(e.detach().cpu(), e_ref.detach())                      # gathered rows: exact
    assert_close(y, y_ref, 1e-5, 1e-5, "y_fm")                                # fp32 sum order
    # gradient rows [0, S): exact layout, padding rows zero; the dump row is never shipped
    # g_emb + g_y * (S_b - e): S_b is a sum of F unit-normal terms taken in a different order -> absolute
    # error ~ F * eps * |S_b| ~ 1e-6 on entries that cancel to ~0; hence the absolute floor of 1e-5
    assert_close(hb.grad[:S, :D + 1], rb.grad[:S, :D + 1], 1e-5, 1e-5, "grad rows")
    assert not hb.grad[:S, D + 1:].any()
    unused = torch.ones(S, dtype=torch.bool)
    unused[slot.view(-1)[slot.view(-1) < S]] = False
    assert not hb.grad[:S][unused.to(DEV)].any()
    assert_close(hbias.grad, rbias.grad, 1e-5, 1e-6, "bias grad")
    pkg.check_index_errors()


def _fwd_ride_without_offsets(slot, buf, bias, D):
    """mi_gather_fm_fwd_ride on mi_slot_fm_fwd's operands: offsets = NULL, no mask job, no rows_out."""
    B, F = slot.shape
    emb = torch.full((B, F, D), float("nan"), device=DEV)
    yfm = torch.full((B,), float("nan"), device=DEV)
    esum = torch.full((B, D), float("nan"), device=DEV)
    rc = _lib.load().mi_gather_fm_fwd_ride(
        slot.data_ptr(), None, buf.data_ptr(), D + 4, buf.data_ptr() + 4 * D, D + 4, bias.data_ptr(), emb.data_ptr(),
        yfm.data_ptr(), None, esum.data_ptr(), B, F, D, buf.shape[0], _lib.err_word(DEV).data_ptr(), None,
        _lib.stream_ptr(DEV))
    return rc, emb, yfm, esum


@pytest.mark.parametrize("B,F,D", [(33, 26, 16), (17, 100, 8)])
def test_fwd_ride_takes_slot_operands_without_offsets(B, F, D):
    """The lookup launch of the sharded fused step when it carries no mask job (deterministic mode, ...): ids that are
    row numbers already, offsets == NULL.  Same kernel as mi_slot_fm_fwd, so the same bits."""
    _, S, buf, slot, bias = _slot_fm_operands(B, F, D)
    buf, slot, bias = buf.to(DEV), slot.to(DEV), bias.to(DEV)
    e_ref, y_ref = _kernels.slot_fm(buf, slot, bias)
    rc, emb, yfm, esum = _fwd_ride_without_offsets(slot, buf, bias, D)
    assert rc == 0                                                            # MI_OK
    assert torch.equal(emb, e_ref) and torch.equal(yfm, y_ref)
    assert_close(esum, emb.view(B, F, D).sum(1), 1e-5, 1e-5, "sum over the fields")      # fp32 sum order
    pkg.check_index_errors()


def test_fwd_ride_without_offsets_is_refused_on_the_scalar_path():
    B, F, D = 33, 26, 12                               # D = 12: no float4 form, and the scalar kernel reads offsets[f]
    _, S, buf, slot, bias = _slot_fm_operands(B, F, D)
    rc, _, _, _ = _fwd_ride_without_offsets(slot.to(DEV), buf.to(DEV), bias.to(DEV), D)
    assert rc == -1                                                           # MI_ERR_INVALID_ARG
    pkg.check_index_errors()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_emulated_ranks_reproduce_the_unsharded_lookup(world):
    """All `world` ranks emulated on one GPU (the all-to-alls done by slicing): logits' FM part and
    the gradient rows arriving at every owner must equal the unsharded fused kernel's."""
    g = torch.Generator().manual_seed(world)
    dims, D, B = [50, 7, 1000, 3, 211], 16, 48
    F, N = len(dims), sum(dims)
    offsets = torch.cumsum(torch.tensor([0] + dims[:-1]), 0).to(DEV)
    W, w1 = torch.randn(N, D, generator=g).to(DEV), torch.randn(N, 1, generator=g).to(DEV)
    bias = torch.tensor([0.1], device=DEV)
    xs = [torch.stack([torch.randint(0, d, (B,), generator=g) for d in dims], 1).to(DEV) for _ in range(world)]
    cap = bucket_capacity(B * F, world, 1.25)
    S = world * cap
    shards = []
    for r in range(world):
        n = local_num_rows(N, r, world)
        Wl, wl = torch.zeros(n + 1, D, device=DEV), torch.zeros(n + 1, 1, device=DEV)
        Wl[:n], wl[:n] = shard_rows(W, r, world), shard_rows(w1, r, world)
        shards.append((Wl, wl))
    routed = [_kernels.route_buckets(x, offsets, world, N, cap, _flag()) for x in xs]
    # all-to-all #1: owner o receives bucket o of every requester r, in requester order
    local_rows = [torch.cat([routed[r][0][o * cap:(o + 1) * cap] for r in range(world)]) for o in range(world)]
    packed = [_kernels.gather_pack_rows(local_rows[o], *shards[o]) for o in range(world)]
    # all-to-all #2: requester r receives chunk r of every owner o, in owner order
    g_total = torch.zeros(N, D, device=DEV)
    g1_total = torch.zeros(N, device=DEV)
    ref_total = torch.zeros(N, D, device=DEV)
    ref1_total = torch.zeros(N, device=DEV)
    g_send = []
    for r in range(world):
        recv = torch.zeros(S + 1, D + 4, device=DEV)
        recv[:S] = torch.cat([packed[o][r * cap:(r + 1) * cap] for o in range(world)])
        recv.requires_grad_(True)
        emb, y = _kernels.slot_fm(recv, routed[r][1], bias)
        Wf, w1f = W.clone().requires_grad_(True), w1.clone().requires_grad_(True)
        emb_ref, y_ref = _kernels.gather_fm(xs[r], offsets, Wf, w1f, bias, True, True)
        assert torch.equal(emb, emb_ref)
        assert_close(y, y_ref, 1e-6, 1e-6, "y_fm")
        ge, gy = torch.randn(B, F, D, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)
        ((emb * ge).sum() + (y * gy).sum()).backward()
        ((emb_ref * ge).sum() + (y_ref * gy).sum()).backward()
        ref_total += Wf.grad.to_dense()
        ref1_total += w1f.grad.to_dense().view(-1)
        g_send.append(recv.grad[:S])
    # all-to-all #3 + scatter at the owners
    for o in range(world):
        g_owner = torch.cat([g_send[r][o * cap:(o + 1) * cap] for r in range(world)])
        n = local_num_rows(N, o, world)
        acc = torch.zeros(n + 1, D + 4, device=DEV).index_add_(0, local_rows[o], g_owner)
        assert not acc[n].any()                                               # the sink only sees zeros
        g_total[o::world] += acc[:n, :D]
        g1_total[o::world] += acc[:n, D]
    assert_close(g_total, ref_total, 1e-5, 1e-5, "table grad")
    assert_close(g1_total, ref1_total, 1e-5, 1e-6, "first-order grad")
    pkg.check_index_errors()

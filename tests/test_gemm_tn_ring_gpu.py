"""GPU: the LDS-DMA weight-gradient kernel (k_gemm_tn_multi) in both ring depths.  A launch whose product workgroups are all
resident at three per CU runs the three-slot form (loads two slices ahead, counted vmcnt); a launch of more workgroups runs
the two-slot form.  Every case runs in both: alone (small launch -> three slots) and next to a 512 x 512 x 4096 product cut
into 16 K-slices (1024 workgroups > 3 x CUs -> two slots); the form is asserted through mi_gemm_f32_multi_slots.  Integer-
valued operands: the products are exact whatever the summation order, so torch.equal against the CPU is the check."""
import os

import pytest
import torch

from conftest import assert_close

from recsys_benchmark_amd import _kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mk(shape, gen):
    return torch.randint(-3, 4, shape, generator=gen).float()


def _want(slots):
    """The form the size rule gives, unless the environment forces one (or keeps the launch off the LDS-DMA kernel)."""
    if os.environ.get("MI_GEMM_TN_DMA") == "0":
        return 0
    forced = os.environ.get("MI_GEMM_TN_SLOTS")
    return int(forced) if forced in ("2", "3") else slots


def _problem(A, B, M, N, K, gen, splitk=0, accumulate=False):
    """One product on the device and its CPU reference (A [K, M], B [K, N] on the CPU)."""
    C0 = _mk((M, N), gen) if accumulate else torch.zeros(M, N)
    q = dict(A=A.to(DEV), B=B.to(DEV), C=C0.to(DEV), M=M, N=N, K=K, lda=M, ldb=N, ldc=N, splitk=splitk, accumulate=accumulate)
    return q, A.t() @ B + C0


# (M, N, K, splitk, accumulate): the smallest shapes at which a ring can go wrong
RING_CASES = [
    (64, 64, 32, 1, False),       # one k-tile: the prologue alone
    (64, 64, 64, 1, False),       # fewer slices than slots
    (64, 64, 96, 1, False),       # exactly the slots
    (64, 64, 128, 1, False),      # the first wrap
    (64, 64, 160, 1, False),
    (64, 64, 160, 3, False),      # slices of 2, 2, 1 k-tiles
    (64, 64, 64, 7, False),       # more slices than k-tiles: empty slices
    (36, 8, 96, 1, False),        # edge blocks
    (100, 68, 160, 1, False),
    (4, 4, 32, 1, False),         # a corner
    (64, 64, 128, 2, True),       # accumulate, two slices of two k-tiles
]


@pytest.fixture(scope="module")
def filler():
    """The product that makes a launch too large for three workgroups per CU: 64 tiles x 16 K-slices of 8 k-tiles."""
    gen = torch.Generator().manual_seed(4321)
    A, B = _mk((4096, 512), gen), _mk((4096, 512), gen)
    return A.to(DEV), B.to(DEV), A.t() @ B


def _launch(probs, refs, slots, filler, ride=None):
    probs, refs = list(probs), list(refs)
    if slots == 2:
        A, B, ref = filler
        probs.append(dict(A=A, B=B, C=torch.zeros(512, 512, device=DEV), M=512, N=512, K=4096, lda=512, ldb=512, ldc=512, splitk=16))
        refs.append(ref)
    assert _kernels.gemm_multi_slots(probs, transA=True) == _want(slots)
    _kernels.gemm_multi(probs, transA=True, ride=ride)
    for q, ref in zip(probs, refs):
        assert torch.equal(q["C"].cpu(), ref), (q["M"], q["N"], q["K"], q.get("splitk"))


@pytest.mark.parametrize("slots", [3, 2])
def test_ring_shapes_exact_in_both_forms(slots, filler):
    gen = torch.Generator().manual_seed(99)
    probs, refs = [], []
    for (M, N, K, sk, acc) in RING_CASES:
        q, ref = _problem(_mk((K, M), gen), _mk((K, N), gen), M, N, K, gen, sk, acc)
        probs.append(q)
        refs.append(ref)
    # batched column slices with strides: three 64 x 48 products out of [512, 192] and [512, 144]
    A, B = _mk((512, 3 * 64), gen), _mk((512, 3 * 48), gen)
    probs.append(dict(A=A.to(DEV), B=B.to(DEV), C=torch.zeros(3, 64, 48, device=DEV), M=64, N=48, K=512, lda=192, ldb=144, ldc=48,
                      batch=3, sA=64, sB=48, sC=64 * 48))
    refs.append(torch.stack([A[:, 64 * e:64 * e + 64].t() @ B[:, 48 * e:48 * e + 48] for e in range(3)]))
    _launch(probs, refs, slots, filler)


@pytest.mark.parametrize("slots", [3, 2])
def test_ring_tail_widths_three_problems(slots, filler):
    """The C2 tail's three weight gradients at K = 256 (the 64-row tiles' last 32-row block is empty, the one before half
    full), the library's cut."""
    gen = torch.Generator().manual_seed(5)
    probs, refs = [], []
    for (M, N) in [(400, 416), (400, 400), (400, 400)]:
        q, ref = _problem(_mk((256, M), gen), _mk((256, N), gen), M, N, 256, gen)
        probs.append(q)
        refs.append(ref)
    _launch(probs, refs, slots, filler)


def test_ring_random_fp32_three_slots():
    """Random fp32 at the tail's shape against float64: the bound of any fp32 product of this length."""
    gen = torch.Generator().manual_seed(6)
    A, B = torch.randn(4096, 400, generator=gen), torch.randn(4096, 416, generator=gen)
    C = torch.zeros(400, 416, device=DEV)
    probs = [dict(A=A.to(DEV), B=B.to(DEV), C=C, M=400, N=416, K=4096, lda=400, ldb=416, ldc=416)]
    assert _kernels.gemm_multi_slots(probs, transA=True) == _want(3)
    _kernels.gemm_multi(probs, transA=True)
    assert_close(C, (A.double().t() @ B.double()).float(), 1e-5, 1e-3)


def test_ring_three_slots_carrying_riders(filler):
    """The three-slot form with prefetch riders behind the products: products exact, no index error raised by the riders'
    out-of-range ids (they are skipped)."""
    from recsys_benchmark_amd import _lib

    gen = torch.Generator().manual_seed(78)
    N, D, B, F = 5000, 16, 300, 7
    table = torch.randn(N, 32, device=DEV)
    ids = torch.randint(0, N // F, (B, F), generator=gen)
    ids[3, 2] = 10 ** 9
    ids[5, 0] = -4
    ids = ids.to(DEV)
    off = (torch.arange(F) * (N // F)).to(DEV)
    job = _kernels.PrefetchRowsJob(ids.data_ptr(), off.data_ptr(), table.data_ptr(), table.data_ptr() + 4 * D, 32, 32, B, N, F)
    probs, refs = [], []
    for (M, Nn, K) in [(400, 416, 512), (64, 64, 32), (132, 260, 160)]:
        q, ref = _problem(_mk((K, M), gen), _mk((K, Nn), gen), M, Nn, K, gen)
        probs.append(q)
        refs.append(ref)
    _launch(probs, refs, 3, filler, ride=job)
    torch.cuda.synchronize()
    _lib.check_index_errors()

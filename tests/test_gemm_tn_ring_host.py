"""Host logic of the LDS-DMA weight-gradient kernel's ring depth (csrc/gemm.hip tn_slots through mi_gemm_f32_multi_slots:
arithmetic only, runs without a GPU): three slots when every product workgroup of the launch is resident at three per CU
(256 CUs: at most 768 workgroups), two otherwise."""
import torch


def _q(M, N, K, **kw):
    return dict(A=torch.zeros(4), B=torch.zeros(4), C=torch.zeros(4), M=M, N=N, K=K, lda=M, ldb=N, ldc=N, **kw)


def test_ring_depth_follows_the_launch_size(monkeypatch):
    from recsys_benchmark_amd import _kernels

    monkeypatch.delenv("MI_GEMM_TN_SLOTS", raising=False)
    B = 4096
    tail = [_q(400, 416, B), _q(400, 400, B), _q(400, 400, B)]
    assert _kernels.gemm_multi_plan(tail, transA=True) == (1, 735, [5, 5, 5])
    assert _kernels.gemm_multi_slots(tail, transA=True) == 3                  # 735 <= 3 x 256
    wide = [dict(q, splitk=16) for q in tail]
    assert _kernels.gemm_multi_plan(wide, transA=True) == (1, 2352, [16, 16, 16])
    assert _kernels.gemm_multi_slots(wide, transA=True) == 2                  # runs in rounds: five per CU
    assert _kernels.gemm_multi_slots(tail, transA=False) == 0                 # the general kernel has no ring
    assert _kernels.gemm_multi_slots([], transA=True) == 0

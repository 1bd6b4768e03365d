"""The fused MLP tail: (Linear, [BatchNorm1d], ReLU, [Dropout]) x k + Linear(., 1) of
DeepFM._deep_branch / DCN._dnn (reference: src/models/deepfm.py:53-66,100-102, src/models/dcn.py:56-66) as ONE autograd
node over the kernels of csrc/tail.hip — training mode (batch statistics), eval mode (running statistics folded into
per-column constants: mi_tail_affine_consts), use_batchnorm=False, with or without grad (inference keeps nothing):

    forward   masks (one launch, only with dropout) ; per layer: MFMA product with the previous layer's
              BatchNorm+ReLU+Dropout applied in its operand load and the BatchNorm statistics in its epilogue, then a
              one-block finalize ; head (row dot + bias + y_fm)                                   -> 2k + 2 launches
    backward  head backward ; per layer: finalize, input-gradient product whose epilogue already is the next layer's dy
              and its dgamma / dbeta pieces ; the k weight-gradient products together in ONE multi-problem launch at the
              end (mi_gemm_f32_multi) on a(z) and dz as the forward / input-gradient operand loads stored them
              (deterministic mode: one slab-summed product per layer instead, no atomics)        -> 2k + 3 launches

against 3 library GEMMs + 4 BatchNorm-family passes per layer each way before.  No activation is written or read a
second time, the dropout decisions are one bit per element, and every reduction is joined in a fixed order: two runs
of the same step give bit-identical results.

`fused_tail_plan(seq, x)` decides whether a Sequential matches (every hidden group has a training-mode BatchNorm1d that
tracks running statistics, widths are multiples of 8, fp32 2-D input); everything else keeps the general path of mlp.py.
"""
import ctypes
from typing import List, Optional

import torch
from torch import nn

from . import _kernels, _lib

import os

SALT = 7919          # per-layer salt of the dropout hash: SALT * (layer index + 1)
# Round 3 (verdict item: "finalize in the consumer's prologue"): the kernels of csrc/tail.hip can join the BatchNorm
# statistics / column sums themselves — every workgroup of the consuming product for itself, by its idle consumer waves
# while the producers' first loads are in flight, workgroup 0 writing the results — instead of in finalize launches of
# their own.  Built, parity-green (tests/test_tail_gpu.py runs both forms), and MEASURED SLOWER on MI355X at the headline
# shape: 0.289 vs 0.2825 ms/step.  Every one of the 256 workgroups has to pull the same 205 KB of tile statistics
# (64 tiles x 400 columns x 8 B) through its CU: +3.5 us (forward product), +2.8 us (input-gradient product), +9.7 us
# (the head: 16 rows of work per workgroup) against 4.3-4.5 us for the launch it replaces (whose kernels were at the
# same time cut to one round trip of loads: 5.3 -> 4.4 us each).  An all-gather among 256 CUs costs what a kernel
# boundary costs on this machine; the launches stay the default.  MI_TAIL_MERGE_JOINS=1 selects the joined form.
MERGE_JOINS = os.environ.get("MI_TAIL_MERGE_JOINS", "0") == "1"
# The step's dropout keep bits + the zero fill of the backward pass's accumulation buffer as extra workgroups of the first
# layer's finalize launch instead of a launch of their own (MI_TAIL_RIDE_MASKS=0: the separate launch).
RIDE_MASKS = os.environ.get("MI_TAIL_RIDE_MASKS", "1") == "1"
# Round 4: BatchNorm statistics (forward) and the dgamma / dbeta column sums (backward) as SUMS the producing product's
# epilogue adds with float atomics into a few replicas of 2 N floats, derived into constants by the consuming product's
# prologue from 8-20 KB (csrc/tail.hip, bn_derive_fwd) — no finalize launch between two products.  Two finalize launches
# per step remain: the first forward layer's (it carries the dropout-bit / zero-fill workgroups) and the head's backward
# (it joins the head's dw / db).  Off in deterministic mode (atomic order), off with MI_TAIL_STAT_SUMS=0 (the round-3 form).
STAT_SUMS = os.environ.get("MI_TAIL_STAT_SUMS", "1") == "1"
STAT_REPS = max(1, min(64, int(os.environ.get("MI_TAIL_STAT_REPS", "4"))))
# the head backward runs 256 workgroups: 8 replicas (32 adders per address) measured best (16: 0.2436, 8: 0.2427 ms per step)
HEAD_REPS = max(1, min(64, int(os.environ.get("MI_TAIL_HEAD_REPS", "8"))))


class _BnFwd(ctypes.Structure):          # mi_tail_bn_fwd (include/mi355x_recsys.h)
    _fields_ = [(n, ctypes.c_void_p) for n in ("part", "gamma", "beta", "mean_offset", "running_mean", "running_var",
                                               "num_batches_tracked", "seed_bump", "mu", "sc", "be", "rstd")] + \
               [("momentum", ctypes.c_float), ("eps", ctypes.c_float), ("shift", ctypes.c_void_p), ("nrep", ctypes.c_int32)]


class _BnBwd(ctypes.Structure):          # mi_tail_bn_bwd
    _fields_ = [(n, ctypes.c_void_p) for n in ("part", "gamma", "rstd", "dgamma", "dbeta", "al", "bz", "de", "wpart", "dw", "db")] + \
               [("nblk", ctypes.c_int32), ("nwblk", ctypes.c_int32), ("dbias", ctypes.c_void_p), ("db2", ctypes.c_void_p),
                ("affine", ctypes.c_int32)]


class _MaskRide(ctypes.Structure):       # mi_tail_mask_ride
    _fields_ = [("seed", ctypes.c_void_p), ("nlayers", ctypes.c_int32), ("M", ctypes.c_int32), ("salts", ctypes.c_void_p),
                ("ps", ctypes.c_void_p), ("lds", ctypes.c_void_p), ("bits", ctypes.c_void_p), ("zero_buf", ctypes.c_void_p),
                ("zero_floats", ctypes.c_int64), ("affine", ctypes.c_void_p)]


class _HeadEpi(ctypes.Structure):        # mi_tail_head_in_epilogue
    _fields_ = [("w", ctypes.c_void_p), ("b", ctypes.c_void_p), ("add", ctypes.c_void_p), ("mu", ctypes.c_void_p),
                ("sc", ctypes.c_void_p), ("be", ctypes.c_void_p), ("out", ctypes.c_void_p)]


class _AffineJob(ctypes.Structure):      # mi_tail_affine_job
    _fields_ = [("nlayers", ctypes.c_int32), ("widths", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("running_mean", ctypes.c_void_p), ("running_var", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("eps", ctypes.c_void_p), ("mu", ctypes.c_void_p), ("sc", ctypes.c_void_p), ("be", ctypes.c_void_p),
                ("rstd", ctypes.c_void_p)]


def _bn_fwd_struct(part, L, c, seed_bump, shift=None, nrep=0) -> "_BnFwd":
    bn = L.bn
    return _BnFwd(part.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), _lib.ptr(L.lin.bias), bn.running_mean.data_ptr(),
                  bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(), seed_bump, c[0].data_ptr(), c[1].data_ptr(),
                  c[2].data_ptr(), c[3].data_ptr(), float(bn.momentum), float(bn.eps), _lib.ptr(shift), int(nrep))


class _Layer:
    """One hidden group.  fixed: the layer normalises with FIXED statistics — an eval-mode BatchNorm1d (running statistics) —
    or not at all (bn None: use_batchnorm=False); otherwise a training-mode BatchNorm1d (batch statistics)."""
    __slots__ = ("lin", "bn", "p", "fixed")

    def __init__(self, lin, bn, p, fixed):
        self.lin, self.bn, self.p, self.fixed = lin, bn, p, fixed


class _Plan(list):
    """The hidden layers; grad: whether a backward may follow (grad mode at call time)."""
    grad = True


class _InputSpec:
    """Stands in for the tail's input tensor when the plan is made before that tensor exists (DeepFM's fused step)."""

    def __init__(self, rows: int, width: int, device):
        self.shape, self.device, self.dtype, self.is_cuda = (rows, width), device, torch.float32, device.type == "cuda"

    def dim(self):
        return 2


def fused_tail_plan(seq: nn.Sequential, x, groups) -> Optional[_Plan]:
    """groups: mlp._groups(seq); x: the input tensor or an _InputSpec.  The plan (hidden layers; the head is groups[-1]) or
    None when the pattern does not fit: (Linear, [BatchNorm1d], ReLU, [Dropout]) x k + Linear(., 1), widths multiples of 8,
    fp32, in training or eval mode, with or without grad."""
    if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32):
        return None
    if len(groups) < 2 or groups[-1][0] != "plain" or len(groups) - 1 > 8:      # (the mask kernel takes <= 8 layers)
        return None
    head = groups[-1][1]
    if not (isinstance(head, nn.Linear) and head.out_features == 1):
        return None
    plan, width = _Plan(), x.shape[1]
    plan.grad = torch.is_grad_enabled()
    for g in groups[:-1]:
        if g[0] != "fused":
            return None
        _, lin, bn, dp = g
        if bn is not None and (not bn.track_running_stats or bn.momentum is None or not bn.affine):
            return None
        if lin.in_features != width or lin.in_features % 8 or lin.out_features % 8 or lin.out_features > 1024:
            return None
        if dp is not None and dp.training and not 0.0 <= float(dp.p) < 1.0:      # p = 1 drops everything: general path
            return None
        tensors = (lin.weight, lin.bias) + ((bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else ())
        if any(t is not None and (t.dtype != torch.float32 or t.device != x.device) for t in tensors):
            return None
        plan.append(_Layer(lin, bn, float(dp.p) if (dp is not None and dp.training) else 0.0, bn is None or not bn.training))
        width = lin.out_features
    if head.in_features != width or x.shape[0] < (1 if all(L.fixed for L in plan) else 2):
        return None
    if any(t is not None and (t.dtype != torch.float32 or t.device != x.device) for t in (head.weight, head.bias)):
        return None
    return plan


def _masks(seed: torch.Tensor, plan: List[_Layer], M: int, dev, zero_buf: Optional[torch.Tensor] = None, ride: bool = False):
    """Keep bits of every layer with dropout; `zero_buf` (optional, fp32, a multiple of 4 elements) is zero-filled by the
    same launch.  With neither nothing is launched.  ride=True: nothing is launched here; returns (bits, job) with job the
    mi_tail_mask_ride (and the host arrays it points at) for the first layer's mi_tail_bn_finalize_fwd_r, or None when
    there is nothing to do."""
    lib = _lib.load()
    n = len(plan)
    bits = [torch.empty(M * L.lin.out_features // 8, dtype=torch.uint8, device=dev) if L.p > 0 else None for L in plan]
    if not any(b is not None for b in bits) and zero_buf is None:
        return (bits, None) if ride else bits
    salts = (ctypes.c_int64 * n)(*[SALT * (i + 1) for i in range(n)])
    ps = (ctypes.c_float * n)(*[L.p for L in plan])
    lds = (ctypes.c_int32 * n)(*[L.lin.out_features for L in plan])
    ptrs = (ctypes.c_void_p * n)(*[0 if b is None else b.data_ptr() for b in bits])
    nzero = zero_buf.numel() if zero_buf is not None else 0
    if ride:
        job = _MaskRide(seed.data_ptr(), n, M, ctypes.addressof(salts), ctypes.addressof(ps), ctypes.addressof(lds),
                        ctypes.addressof(ptrs), _lib.ptr(zero_buf), nzero, None)
        return bits, (job, salts, ps, lds, ptrs)
    _lib.check(lib.mi_tail_dropout_masks_z(seed.data_ptr(), n, ctypes.addressof(salts), ctypes.addressof(ps), ctypes.addressof(lds),
                                           ctypes.addressof(ptrs), M, _lib.ptr(zero_buf), nzero, _lib.stream_ptr(dev)),
               "mi_tail_dropout_masks_z")
    return bits


def _fixed_constants(plan: List[_Layer], dev, stream, defer: bool = False):
    """(mu, sc, be, rstd) [4, N] of every layer that normalises with fixed statistics or not at all, ONE launch for all of
    them (mi_tail_affine_consts); {layer index: tensor}.  defer: nothing is launched — returns (tensors, job) with job a
    (mi_tail_affine_job, host arrays it points at) for a launch that carries it (the lookup in front of the tail), or None."""
    idx = [i for i, L in enumerate(plan) if L.fixed]
    if not idx:
        return ({}, None) if defer else {}
    n = len(idx)
    out = {i: torch.empty((4, plan[i].lin.out_features), dtype=torch.float32, device=dev) for i in idx}
    P = ctypes.c_void_p * n

    def arr(f):
        return P(*[f(plan[i]) or 0 for i in idx])

    def bn_of(L, name):
        return _lib.ptr(getattr(L.bn, name)) if L.bn is not None else None

    # (every host array stays referenced until the call has returned: the library reads them at call time)
    widths = (ctypes.c_int32 * n)(*[plan[i].lin.out_features for i in idx])
    eps = (ctypes.c_float * n)(*[float(plan[i].bn.eps) if plan[i].bn is not None else 0.0 for i in idx])
    gam, bet = arr(lambda L: bn_of(L, "weight")), arr(lambda L: bn_of(L, "bias"))
    rme, rva = arr(lambda L: bn_of(L, "running_mean")), arr(lambda L: bn_of(L, "running_var"))
    bia = arr(lambda L: _lib.ptr(L.lin.bias))
    outs = [P(*[out[i][r].data_ptr() for i in idx]) for r in range(4)]
    if defer:
        job = _AffineJob(n, ctypes.addressof(widths), ctypes.addressof(gam), ctypes.addressof(bet), ctypes.addressof(rme),
                         ctypes.addressof(rva), ctypes.addressof(bia), ctypes.addressof(eps), ctypes.addressof(outs[0]),
                         ctypes.addressof(outs[1]), ctypes.addressof(outs[2]), ctypes.addressof(outs[3]))
        return out, (job, widths, eps, gam, bet, rme, rva, bia, outs)
    _lib.check(_lib.load().mi_tail_affine_consts(
        n, ctypes.addressof(widths), ctypes.addressof(gam), ctypes.addressof(bet), ctypes.addressof(rme), ctypes.addressof(rva),
        ctypes.addressof(bia), ctypes.addressof(eps), ctypes.addressof(outs[0]), ctypes.addressof(outs[1]),
        ctypes.addressof(outs[2]), ctypes.addressof(outs[3]), stream), "mi_tail_affine_consts")
    return out


class _State:
    """What the forward leaves for the backward: tensors (flattened for ctx.save_for_backward) + plain metadata."""
    __slots__ = ("k", "ps", "has_head_bias", "add_shape", "zeros", "plan", "n_saved", "stat_b", "zsize", "boff", "hoff", "head",
                 "extra")


# The gather + FM forward in front of DeepFM's tail carries the keep bits and the zero fill (mi_gather_fm_fwd_ride): the
# first layer's statistics can then be shifted sums like the others' and the step has no finalize launch at all
# (MI_TAIL_LEAD_RIDE=0: the first layer keeps its tile statistics and the finalize launch that carries the masks)
LEAD_RIDE = os.environ.get("MI_TAIL_LEAD_RIDE", "1") == "1"
# An inference forward behind a lead launch (DeepFM): the head Linear(., 1) in the epilogue of the last hidden layer's product
# (mi_tail_fwd_gemm_head; the logits' zero fill rides in the lead launch) — MI_TAIL_HEAD_EPILOGUE=0: the head as its own launch
HEAD_EPILOGUE = os.environ.get("MI_TAIL_HEAD_EPILOGUE", "1") == "1"
# Labels known at forward time (DeepFM.forward(x, labels=y)): head + BCE-with-logits + the head's backward sums in one
# launch (mi_tail_head_bce) instead of three (MI_TAIL_HEAD_LOSS=0: off)
HEAD_LOSS = os.environ.get("MI_TAIL_HEAD_LOSS", "1") == "1"


class _Lead:
    """The kernel in front of the tail that produces its input (DeepFM: gather + FM): `launch(job)` runs it — carrying the
    mask job (a mi_tail_mask_ride or None) — and returns (x[M, K], last_add or None).  extra_zero: floats the step's
    zero-filled buffer should hold for the caller besides the tail's own accumulators (state.extra)."""
    __slots__ = ("M", "dev", "launch", "extra_zero")

    def __init__(self, M, dev, launch, extra_zero: int = 0):
        self.M, self.dev, self.launch, self.extra_zero = M, dev, launch, int(extra_zero)


class _HeadLoss:
    """What mi_tail_head_bce left for the criterion: losses.BCEWithLogitsLoss(logits, labels) picks it up when it is handed
    exactly these logits and labels (take_head_loss), otherwise computes the loss itself.  The launch READ the logits and the
    upstream seed's value: out_version / seed_version are their versions then — the loss stands only for unmodified logits
    (current), the gradient only for an unmodified seed (seed_current)."""
    __slots__ = ("out", "y", "y_key", "loss", "gvec", "seed", "out_version", "seed_version")

    def current(self) -> bool:
        return self.out._version == self.out_version

    def seed_current(self) -> bool:
        return self.seed._version == self.seed_version


_HEAD_LOSS = {}


def _label_key(t):
    return (t.data_ptr(), t._version, t.dtype, t.numel())


def take_head_loss(logits: torch.Tensor, target: torch.Tensor):
    if not _HEAD_LOSS or not logits.is_cuda:
        return None
    h = _HEAD_LOSS.pop(str(logits.device), None)
    if h is None:
        return None
    if (logits.dtype == torch.float32 and logits.requires_grad and logits.data_ptr() == h.out.data_ptr()
            and logits.numel() == h.out.numel() and logits.is_contiguous() and _label_key(target) == h.y_key
            and h.current() and logits._version == h.out_version):        # (a view shares its base's version counter)
        return h
    return None


def _tail_forward(plan, seed, x, last_add, Ws, w_head, b_head, lead: Optional[_Lead] = None, labels=None, loss_seed=None):
    """The forward kernels of the tail; returns (out[M, 1], tensors to save, state).  lead (instead of x / last_add): the
    launch that produces them, run here once the mask job it carries is known.  labels ([M] fp32, optional): the head
    launch also evaluates BCE-with-logits against them and the head's backward sums (state.head) for the upstream gradient
    loss_seed (a device scalar: what the caller will seed the criterion's backward with; None: losses.unit_scalar)."""
    lib = _lib.load()
    dev = lead.dev if lead is not None else _lib.require_gpu(x)
    s = _lib.stream_ptr(dev)
    M = lead.M if lead is not None else x.shape[0]
    k = len(plan)
    grad = bool(getattr(plan, "grad", True))
    merge = MERGE_JOINS
    R, Rh = STAT_REPS, HEAD_REPS
    sums_ok = STAT_SUMS and not merge and not _kernels.DETERMINISTIC
    lead_ride = lead is not None and LEAD_RIDE and sums_ok
    # this product ADDS its statistics (the first layer's only when a launch in front of it has zeroed the sums)
    stat_f = [sums_ok and (i >= 1 or lead_ride) and not L.fixed for i, L in enumerate(plan)]
    stat_b = sums_ok and grad
    head_loss = (labels is not None and HEAD_LOSS and stat_b and plan[-1].lin.out_features <= 512
                 and plan[-1].lin.out_features % 4 == 0)
    # ONE zero-filled buffer per step for everything that accumulates: the split-K weight gradients and the (exactly zero)
    # bias gradients under a training-mode BatchNorm (backward), the forward sums of the layers above the first, the
    # backward column sums of every layer and of the head
    zsize = 0
    if grad:
        zsize = sum(L.lin.out_features * L.lin.in_features + L.lin.out_features for L in plan)
        zsize = (zsize + 3) // 4 * 4
    foff, boff, hoff, loff = {}, {}, None, None
    for i, L in enumerate(plan):
        if stat_f[i]:                      # (fp64 sums: 4 R N floats, 8-byte aligned — zsize is a multiple of 4 floats here)
            foff[i] = zsize
            zsize += (R * 4 * L.lin.out_features + 3) // 4 * 4
    if stat_b:
        for i in range(k - 1):
            boff[i] = zsize
            zsize += R * 2 * plan[i].lin.out_features
        hoff = zsize
        zsize += Rh * (3 * plan[-1].lin.out_features + 4)
        zsize = (zsize + 3) // 4 * 4
        if head_loss:
            loff = zsize
            zsize += int(lib.mi_tail_head_bce_ws_elems(Rh))
    eoff = None
    if lead is not None and lead.extra_zero > 0 and grad:
        eoff = zsize
        zsize += (lead.extra_zero + 3) // 4 * 4
    zeros = torch.empty((zsize,), dtype=torch.float32, device=dev) if zsize else None
    # the keep bits and the zero fill ride in the first layer's finalize launch (no launch of their own) when that launch
    # exists (a training-mode BatchNorm on the first layer) and a LATER kernel can advance the seed
    ride = RIDE_MASKS and not merge and k >= 2 and not plan[0].fixed and not lead_ride
    # inference (nothing kept, every layer on fixed statistics): the head runs in the last product's epilogue, its logits are
    # zero-filled by the lead launch
    head_epi = (HEAD_EPILOGUE and lead_ride and not grad and zeros is None and labels is None and all(L.fixed for L in plan)
                and all(L.p == 0 for L in plan) and w_head.numel() % 4 == 0)
    out_pad = torch.empty(((M + 3) // 4 * 4,), dtype=torch.float32, device=dev) if head_epi else None
    if lead_ride:
        # the launch in front of the tail carries the keep bits, the zero fill AND the constants of the fixed-statistics layers
        bits, lead_job = _masks(seed, plan, M, dev, out_pad if head_epi else zeros, ride=True)
        fixed_c, aff = _fixed_constants(plan, dev, s, defer=True)
        ride_struct = lead_job[0] if lead_job is not None else None
        if aff is not None:
            if ride_struct is None:
                ride_struct = _MaskRide(None, 0, M, None, None, None, None, None, 0, None)
            ride_struct.affine = ctypes.addressof(aff[0])
        x, last_add = lead.launch(ride_struct)
        job = None
    else:
        if lead is not None:
            x, last_add = lead.launch(None)
        bits, job = _masks(seed, plan, M, dev, zeros, ride=True) if ride else (_masks(seed, plan, M, dev, zeros), None)
        fixed_c = _fixed_constants(plan, dev, s)
    keep_inputs = grad and not _kernels.DETERMINISTIC
    Zs, consts, acts = [], [], []
    prev, prev_c, prev_p, prev_bits = x, None, 0.0, None
    any_bits = any(b is not None for b in bits)
    bump_at = 1 if job is not None else 0
    pending = None            # (part, layer, constants[, shift]) of the layer whose statistics the next kernel joins
    bumped = False

    def pending_struct():
        nonlocal bumped
        bump = seed.data_ptr() if (any_bits and not bumped) else None
        bumped = bumped or bump is not None
        if len(pending) == 4:
            return _bn_fwd_struct(pending[0], pending[1], pending[2], bump, shift=pending[3], nrep=R)
        return _bn_fwd_struct(pending[0], pending[1], pending[2], bump)

    for i, L in enumerate(plan):
        N, K = L.lin.out_features, L.lin.in_features
        if head_epi and i == k - 1:        # the last hidden layer of an inference forward: product + head, z not stored
            c = fixed_c[i]
            hadd = None if last_add is None else _kernels._f32c(last_add).view(-1)
            epi = _HeadEpi(w_head.data_ptr(), _lib.ptr(b_head), _lib.ptr(hadd), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
                           out_pad.data_ptr())
            _lib.check(lib.mi_tail_fwd_gemm_head(
                prev.data_ptr(), K, _lib.ptr(prev_c[0]) if prev_c is not None else None,
                _lib.ptr(prev_c[1]) if prev_c is not None else None, _lib.ptr(prev_c[2]) if prev_c is not None else None,
                float(prev_p), _lib.ptr(prev_bits), Ws[i].data_ptr(), K, M, N, K, None, ctypes.byref(epi), s),
                "mi_tail_fwd_gemm_head")
            acts.append(x.new_empty(0))
            Zs.append(x.new_empty(0))
            consts.append(c)
            continue
        Z = torch.empty((M, N), dtype=torch.float32, device=dev)
        part = shift = None
        if L.fixed:
            c = fixed_c[i]
        else:
            c = torch.empty((4, N), dtype=torch.float32, device=dev)          # mu, sc, be, rstd
            if stat_f[i]:
                part = zeros[foff[i]: foff[i] + R * 4 * N]
                shift = torch.empty((N,), dtype=torch.float32, device=dev)
            else:
                part = torch.empty(int(lib.mi_tail_part_elems(M, N)), dtype=torch.float32, device=dev)
        # the layer's input activation as its operand load computes it, kept for the weight gradient (not in
        # deterministic mode, whose weight-gradient kernel recomputes it)
        a_in = torch.empty((M, K), dtype=torch.float32, device=dev) if (keep_inputs and prev_c is not None) else None
        stats = pending_struct() if pending is not None else None
        pending = None
        _lib.check(lib.mi_tail_fwd_gemm_s(
            prev.data_ptr(), K, _lib.ptr(prev_c[0]) if prev_c is not None else None,
            _lib.ptr(prev_c[1]) if prev_c is not None else None, _lib.ptr(prev_c[2]) if prev_c is not None else None,
            float(prev_p), _lib.ptr(prev_bits), Ws[i].data_ptr(), K, Z.data_ptr(), N, _lib.ptr(part), _lib.ptr(a_in),
            M, N, K, ctypes.byref(stats) if stats is not None else None, R if stat_f[i] else 0, _lib.ptr(shift),
            L.bn.running_mean.data_ptr() if stat_f[i] else None, _lib.ptr(L.lin.bias) if stat_f[i] else None, s),
            "mi_tail_fwd_gemm_s")
        acts.append(a_in if a_in is not None else x.new_empty(0))
        if L.fixed:
            pass
        elif stat_f[i]:
            pending = (part, L, c, shift)
        elif merge:
            pending = (part, L, c)
        else:
            bn = L.bn
            late_bump = (sums_ok and k >= 2) or i != bump_at       # (sums: the first deriving kernel advances the seed)
            _lib.check(lib.mi_tail_bn_finalize_fwd_r(
                part.data_ptr(), M, N, bn.weight.data_ptr(), bn.bias.data_ptr(), _lib.ptr(L.lin.bias),
                bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.momentum), float(bn.eps),
                bn.num_batches_tracked.data_ptr(), seed.data_ptr() if (any_bits and not late_bump and not bumped) else None,
                c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(),
                ctypes.byref(job[0]) if (i == 0 and job is not None) else None, s), "mi_tail_bn_finalize_fwd_r")
            bumped = bumped or (any_bits and not late_bump)
        Zs.append(Z)
        consts.append(c)
        prev, prev_c, prev_p, prev_bits = Z, c, L.p, bits[i]
    out = out_pad[:M].view(M, 1) if head_epi else torch.empty((M, 1), dtype=torch.float32, device=dev)
    add = None if last_add is None else _kernels._f32c(last_add).view(-1)
    N = plan[-1].lin.out_features
    if pending is not None:
        stats = pending_struct()
    elif any_bits and not bumped:      # nothing left to join: the head only advances the seed (part = NULL)
        stats = _BnFwd(None, None, None, None, None, None, None, seed.data_ptr(), None, None, None, None, 0.0, 0.0, None, 0)
        bumped = True
    else:
        stats = None
    head = None
    if head_loss:
        y = _kernels._f32c(labels).view(-1)
        if y.numel() != M:
            raise ValueError("labels must hold one value per row of the batch")
        head = _HeadLoss()
        head.out, head.y, head.y_key = out, y, _label_key(labels)
        head.gvec = torch.empty((M,), dtype=torch.float32, device=dev)
        head.loss = zeros[loff: loff + 1]
        if loss_seed is None:
            from .losses import unit_scalar

            head.seed = unit_scalar(dev)
        else:
            if loss_seed.numel() != 1 or loss_seed.dtype != torch.float32 or loss_seed.device != dev:
                raise ValueError("loss_seed must be a float32 device scalar")
            head.seed = loss_seed
        DY = torch.empty((M, N), dtype=torch.float32, device=dev)
        _lib.check(lib.mi_tail_head_bce(
            prev.data_ptr(), N, prev_c[0].data_ptr(), prev_c[1].data_ptr(), prev_c[2].data_ptr(), float(prev_p), _lib.ptr(prev_bits),
            w_head.data_ptr(), _lib.ptr(b_head), _lib.ptr(add), y.data_ptr(), out.data_ptr(), head.gvec.data_ptr(), DY.data_ptr(),
            zeros[hoff:].data_ptr(), zeros[hoff + Rh * 2 * N:].data_ptr(), Rh, zeros[loff:].data_ptr(), M, N,
            ctypes.byref(stats) if stats is not None else None, _lib.ptr(loss_seed), s), "mi_tail_head_bce")
        head.out_version, head.seed_version = out._version, head.seed._version
        _HEAD_LOSS[str(dev)] = head
    elif head_epi:
        pass                               # (the logits came out of the last product's epilogue)
    else:
        _lib.check(lib.mi_tail_head_fwd_m(prev.data_ptr(), N, prev_c[0].data_ptr(), prev_c[1].data_ptr(), prev_c[2].data_ptr(),
                                          float(prev_p), _lib.ptr(prev_bits), w_head.data_ptr(), _lib.ptr(b_head), _lib.ptr(add),
                                          out.data_ptr(), M, N, ctypes.byref(stats) if stats is not None else None, s),
                   "mi_tail_head_fwd_m")
    st = _State()
    st.k, st.plan, st.zeros = k, plan, zeros
    st.head = (head.gvec, DY) if head is not None else None
    st.extra = zeros[eoff: eoff + lead.extra_zero] if eoff is not None else None
    st.stat_b, st.zsize, st.boff, st.hoff = stat_b, zsize, boff, hoff
    st.ps = [L.p for L in plan]
    st.has_head_bias = b_head is not None
    st.add_shape = None if last_add is None else tuple(last_add.shape)
    saved = [x, w_head, *Ws, *Zs, *consts, *[b if b is not None else x.new_empty(0) for b in bits],
             *[L.bn.weight if L.bn is not None else x.new_empty(0) for L in plan], *acts]
    st.n_saved = len(saved)
    return out, saved, st


def _tail_backward(st, saved, g, need_x: bool, need_params, need_add: bool, fm=None, beside_wgrad=None):
    """The backward kernels of the tail.  need_params[j]: whether parameter j of (W, b, gamma, beta) x k + (w, b)_head wants
    a gradient.  fm (DeepFM, the tail's input is the embedding block): (emb_sum[M, D], g1vals[M, F] or None, D) — the first
    layer's input-gradient product then writes the lookup table's row-form gradient instead of dx (mi_tail_dgrad_gemm_fm)
    and the returned dx IS that [M, F*D] buffer.  Returns (dx, dadd, grads, db_head)."""
    lib = _lib.load()
    k, plan = st.k, st.plan
    x, w_head = saved[0], saved[1]
    Ws, Zs, consts = saved[2:2 + k], saved[2 + k:2 + 2 * k], saved[2 + 2 * k:2 + 3 * k]
    bits = [b if b.numel() else None for b in saved[2 + 3 * k:2 + 4 * k]]
    gammas = [t if t.numel() else None for t in saved[2 + 4 * k:2 + 5 * k]]
    acts = [a if a.numel() else None for a in saved[2 + 5 * k:2 + 6 * k]]
    dev = x.device
    s = _lib.stream_ptr(dev)
    M = x.shape[0]
    gvec = _kernels._f32c(g).view(M)
    later = []           # weight-gradient products for ONE launch at the end
    sizes = [(Zs[i].shape[1] * Ws[i].shape[1], Zs[i].shape[1]) for i in range(k)]
    zeros = st_zeros = st.zeros            # filled by the forward's mask launch; a second backward needs a fresh one
    st.zeros = None
    if zeros is None:
        zeros = torch.zeros((max(st.zsize, sum(a + b for a, b in sizes)),), dtype=torch.float32, device=dev)
    stat, R, Rh = st.stat_b, STAT_REPS, HEAD_REPS
    zoff = [0]
    for a, b in sizes:
        zoff.append(zoff[-1] + a + b)
    grads: List[Optional[torch.Tensor]] = [None] * (4 * k + 2)

    # ---- head: dy of the last hidden layer, its column sums, dw / db of the head
    N = Zs[-1].shape[1]
    c = consts[-1]
    DY = None if st.head is not None else torch.empty((M, N), dtype=torch.float32, device=dev)
    if stat:            # sums added into Rh zeroed rows: joined by the next product's prologue, no finalize launch
        nblk = Rh
        part = zeros[st.hoff: st.hoff + Rh * 2 * N].view(Rh, N, 2)
        wpart = zeros[st.hoff + Rh * 2 * N: st.hoff + Rh * (3 * N + 4)].view(Rh, N + 4)
    else:
        nblk = int(lib.mi_tail_head_blocks(M))
        part = torch.empty((nblk, N, 2), dtype=torch.float32, device=dev)
        wpart = torch.empty((nblk, N + 4), dtype=torch.float32, device=dev)
    fused_head, st.head = st.head, None
    if (fused_head is not None and stat and zeros is st_zeros and gvec.data_ptr() == fused_head[0].data_ptr()):
        DY = fused_head[1]        # the forward's head launch wrote DY and the sums for exactly this gradient
    else:
        if fused_head is not None and zeros is st_zeros:
            zeros[st.hoff: st.hoff + Rh * (3 * N + 4)].zero_()      # ... for an upstream gradient of 1: not this one
        if DY is None:
            DY = torch.empty((M, N), dtype=torch.float32, device=dev)
        _lib.check(lib.mi_tail_head_bwd_s(Zs[-1].data_ptr(), N, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), float(st.ps[-1]),
                                          _lib.ptr(bits[-1]), gvec.data_ptr(), w_head.data_ptr(), DY.data_ptr(), part.data_ptr(),
                                          wpart.data_ptr(), Rh if stat else 0, M, N, s), "mi_tail_head_bwd_s")
    dw_head = torch.empty((1, N), dtype=torch.float32, device=dev)
    db_head = torch.empty((1,), dtype=torch.float32, device=dev)
    # DeepFM's scalar bias is added to every logit like the head's bias: same gradient, written to a second word by the
    # same join (a clone would be a copy launch per step)
    db_twin = torch.empty((1,), dtype=torch.float32, device=dev) if fm is not None else None
    part_rows, wp, nw = nblk, wpart, nblk
    dx = None
    for i in range(k - 1, -1, -1):
        N, K = Zs[i].shape[1], Ws[i].shape[1]
        L = plan[i]
        c = consts[i]
        dgb = torch.empty((2, N), dtype=torch.float32, device=dev)
        dzc = torch.empty((3, N), dtype=torch.float32, device=dev)         # al, bz, de
        dbias = torch.empty((N,), dtype=torch.float32, device=dev) if (L.fixed and L.lin.bias is not None) else None
        below = Zs[i - 1] if i > 0 else x
        bc = consts[i - 1] if i > 0 else None
        bp = st.ps[i - 1] if i > 0 else 0.0
        bb = bits[i - 1] if i > 0 else None
        runs_dgrad = i > 0 or need_x
        # the column sums behind dz's constants: joined in the input-gradient product's prologue, or (no such product
        # for this layer, or the joined forms off) by the finalize launch
        sums = None
        if (MERGE_JOINS or stat) and runs_dgrad and part_rows <= 128:     # (256 partial rows of the head keep their finalize launch)
            sums = _BnBwd(part.data_ptr(), _lib.ptr(gammas[i]), c[3].data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(),
                          dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(), _lib.ptr(wp),
                          dw_head.data_ptr() if wp is not None else None, db_head.data_ptr() if wp is not None else None,
                          part_rows, nw, _lib.ptr(dbias), _lib.ptr(db_twin) if wp is not None else None, int(L.fixed))
        else:
            _lib.check(lib.mi_tail_bn_finalize_bwd_b(
                part.data_ptr(), part_rows, M, N, _lib.ptr(gammas[i]), c[3].data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(),
                dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(), _lib.ptr(wp), nw, dw_head.data_ptr() if wp is not None else None,
                db_head.data_ptr() if wp is not None else None, int(L.fixed), _lib.ptr(dbias),
                _lib.ptr(db_twin) if wp is not None else None, s), "mi_tail_bn_finalize_bwd_b")
        wp = None
        if L.bn is not None:
            grads[4 * i + 2], grads[4 * i + 3] = dgb[0], dgb[1]
        if need_params[4 * i + 1] and L.lin.bias is not None:
            # under a training-mode BatchNorm the batch mean is removed: exactly zero; otherwise al * sum dy
            grads[4 * i + 1] = dbias if L.fixed else zeros[zoff[i] + N * K: zoff[i + 1]]
        a_in = x if i == 0 else acts[i]
        defer = need_params[4 * i] and runs_dgrad and a_in is not None and not _kernels.DETERMINISTIC
        dz_keep = torch.empty((M, N), dtype=torch.float32, device=dev) if defer else None
        layer_DY = DY
        if runs_dgrad:
            OUT = torch.empty((M, K), dtype=torch.float32, device=dev)
            if i > 0 and stat:             # the layer below's column sums: added into R zeroed rows (float atomics)
                npart = zeros[st.boff[i - 1]: st.boff[i - 1] + R * 2 * K]
            else:
                npart = torch.empty(int(lib.mi_tail_part_elems(M, K)), dtype=torch.float32, device=dev) if i > 0 else None
            if i == 0 and fm is not None and len(fm) == 5:      # the sharded step: rows go back into the receive buffer's gradient
                emb_sum, _, D, slot, gbuf = fm
                OUT = gbuf
                _lib.check(lib.mi_tail_dgrad_gemm_fm_slot(
                    DY.data_ptr(), Zs[i].data_ptr(), N, c[0].data_ptr(), dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(),
                    Ws[i].data_ptr(), K, gbuf.data_ptr(), _lib.ptr(dz_keep), M, N, K,
                    ctypes.byref(sums) if sums is not None else None, x.data_ptr(), emb_sum.data_ptr(), gvec.data_ptr(),
                    slot.data_ptr(), D, s), "mi_tail_dgrad_gemm_fm_slot")
            elif i == 0 and fm is not None:
                emb_sum, g1vals, D = fm
                _lib.check(lib.mi_tail_dgrad_gemm_fm(
                    DY.data_ptr(), Zs[i].data_ptr(), N, c[0].data_ptr(), dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(),
                    Ws[i].data_ptr(), K, OUT.data_ptr(), _lib.ptr(dz_keep), M, N, K,
                    ctypes.byref(sums) if sums is not None else None, x.data_ptr(), emb_sum.data_ptr(), gvec.data_ptr(),
                    _lib.ptr(g1vals), D, s), "mi_tail_dgrad_gemm_fm")
            else:
                _lib.check(lib.mi_tail_dgrad_gemm_s(
                    DY.data_ptr(), Zs[i].data_ptr(), N, c[0].data_ptr(), dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(),
                    Ws[i].data_ptr(), K, below.data_ptr() if i > 0 else None, K, _lib.ptr(bc[0]) if bc is not None else None,
                    _lib.ptr(bc[1]) if bc is not None else None, _lib.ptr(bc[2]) if bc is not None else None, float(bp), _lib.ptr(bb),
                    OUT.data_ptr(), K, _lib.ptr(npart), R if (stat and i > 0) else 0, _lib.ptr(dz_keep), M, N, K,
                    ctypes.byref(sums) if sums is not None else None, s), "mi_tail_dgrad_gemm_s")
        # the weight gradient comes AFTER the input-gradient product: in the joined form that product's workgroup 0 is
        # what writes al / bz / de
        if defer:
            dW = zeros[zoff[i]: zoff[i] + N * K].view(N, K)               # split-K slices meet in atomics
            later.append(dict(A=dz_keep, B=a_in, C=dW, M=N, N=K, K=M, lda=N, ldb=K, ldc=K))   # dW = dz^T a_in
            grads[4 * i] = dW
        elif need_params[4 * i]:
            splits = int(lib.mi_tail_wgrad_splits(M, N, K))
            slab = torch.empty((splits, N, K), dtype=torch.float32, device=dev)
            dW = torch.empty((N, K), dtype=torch.float32, device=dev)
            _lib.check(lib.mi_tail_wgrad_gemm(
                layer_DY.data_ptr(), Zs[i].data_ptr(), N, c[0].data_ptr(), dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(),
                below.data_ptr(), K, _lib.ptr(bc[0]) if bc is not None else None, _lib.ptr(bc[1]) if bc is not None else None,
                _lib.ptr(bc[2]) if bc is not None else None, float(bp), _lib.ptr(bb), slab.data_ptr(), dW.data_ptr(), M, N, K, s),
                "mi_tail_wgrad_gemm")
            grads[4 * i] = dW
        if runs_dgrad:
            if i > 0:
                DY, part, part_rows = OUT, npart, (R if stat else (M + 63) // 64)
            else:
                dx = OUT
    # (beside_wgrad: a job for extra workgroups of this MFMA-bound launch — the next batch's table lines, DeepFM.prefetch_next)
    _kernels.gemm_multi(later, transA=True, ride=beside_wgrad[0] if beside_wgrad is not None else None)
    grads[4 * k] = dw_head
    grads[4 * k + 1] = db_head if st.has_head_bias else None
    dadd = gvec.view(st.add_shape) if (st.add_shape is not None and need_add) else None
    return dx, dadd, grads, (db_twin if db_twin is not None else db_head)


class FusedTailFn(torch.autograd.Function):
    """out[M, 1] = head(a_k) + last_add, a_l = dropout(relu(bn(a_{l-1} W_l^T + b_l))).

    Differentiable inputs: x, last_add, then per hidden layer (W, b, gamma, beta), then the head's (w, b).  `plan`, `head`
    and `seed` ride along as plain Python objects / buffers.  The Linear biases of the hidden layers cancel in the
    training-mode normalisation: they are left out of the products, shift the running mean only (mean_offset) and get an
    exactly zero gradient."""

    @staticmethod
    def forward(ctx, plan, head, seed, x, last_add, labels, loss_seed, *params):
        k = len(plan)
        x = _kernels._f32c(x)
        Ws = [_kernels._f32c(params[4 * i]) for i in range(k)]
        w_head = _kernels._f32c(params[4 * k]).view(-1)
        out, saved, st = _tail_forward(plan, seed, x, last_add, Ws, w_head, params[4 * k + 1], labels=labels, loss_seed=loss_seed)
        ctx.st = st
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad           # (plan, head, seed, x, last_add, labels, loss_seed, *params)
        dx, dadd, grads, _ = _tail_backward(ctx.st, ctx.saved_tensors, g, need[3], need[7:], need[4])
        return (None, None, None, dx, dadd, None, None, *grads)


# The NEXT batch's ids, when the caller knows them (a DataLoader is one batch ahead of the step: DeepFM.prefetch_next(x)):
# the step then touches that batch's table rows in extra workgroups of its weight-gradient launch (MFMA-bound, the HBM idle),
# so the next forward's ~106 K random 128-byte lines come from the Infinity Cache.  Consumed by the next DeepFMFusedFn forward.
# (Round 4 first ran the job on a side stream beside that launch: the two cross-stream edges cost ~30 us inside a hipGraph.)
_NEXT_IDS = {}


def set_next_batch(idx: Optional[torch.Tensor]) -> None:
    if idx is None:
        _NEXT_IDS.clear()
    else:
        _NEXT_IDS[str(idx.device)] = _kernels._i64c(idx)


def _next_batch_prefetch(dev, offsets, Wc, ldw, w1c, ldw1, F, N):
    """The job (a _kernels.PrefetchRowsJob + the tensors it points at) the step's weight-gradient launch will carry, or None."""
    nxt = _NEXT_IDS.pop(str(dev), None)
    if nxt is None or nxt.dim() != 2 or nxt.shape[1] != F or nxt.device != dev:
        return None
    job = _kernels.PrefetchRowsJob(nxt.data_ptr(), offsets.data_ptr(), Wc.data_ptr(), w1c.data_ptr(), int(ldw), int(ldw1),
                                   int(nxt.shape[0]), int(N), int(F))
    return job, (nxt, offsets, Wc, w1c)


class DeepFMFusedFn(torch.autograd.Function):
    """DeepFM's whole forward as ONE autograd node (src/models/deepfm.py:79-105): gather + FM + first-order term
    (mi_gather_fm_fwd_sum) feeding the fused tail, so that the backward of the lookup runs in the EPILOGUE of the first
    layer's input-gradient product (mi_tail_dgrad_gemm_fm) instead of as a kernel of its own behind it: the gradient of the
    embedding block is never written to memory and read back, one launch less per step.

    Inputs: idx [B, F] raw ids, offsets [F], W / w1 (the two tables, strided views of a packed table allowed), bias, then
    the tail's parameters as FusedTailFn takes them.  Table gradients come in row (COO) form for the tables that asked for
    it (sparse_W / sparse_w1) and are scatter-added into a dense gradient for one that did not — exactly what
    _kernels.GatherFM.backward does with the same values."""

    @staticmethod
    def forward(ctx, plan, head, seed, idx, offsets, W, w1, bias, sparse_W: bool, sparse_w1: bool, labels, *params):
        dev = _lib.require_gpu(idx, offsets, W, w1, bias)
        lib = _lib.load()
        Wc, ldw = _kernels._row_strided(W)
        N, D = Wc.shape
        idx, offsets, w1c, ldw1, _ = _kernels._lookup_operands(idx, offsets, w1, N)
        B, F = idx.shape
        emb = torch.empty((B, F * D), dtype=torch.float32, device=dev)
        yfm = torch.empty((B,), dtype=torch.float32, device=dev)
        rows = torch.empty((B, F), dtype=torch.int64, device=dev)
        esum = torch.empty((B, D), dtype=torch.float32, device=dev)

        def gather(job):      # (job: the tail's mask work, carried in extra workgroups of this launch)
            _lib.check(lib.mi_gather_fm_fwd_ride(idx.data_ptr(), offsets.data_ptr(), Wc.data_ptr(), ldw, w1c.data_ptr(), ldw1,
                                                 _lib.ptr(bias), emb.data_ptr(), yfm.data_ptr(), rows.data_ptr(), esum.data_ptr(),
                                                 B, F, D, N, _lib.err_word(dev).data_ptr(),
                                                 ctypes.byref(job) if job is not None else None, _lib.stream_ptr(dev)),
                       "mi_gather_fm_fwd_ride")
            return emb, yfm

        _kernels.note_field_layout(rows, offsets, N)
        k = len(plan)
        Ws = [_kernels._f32c(params[4 * i]) for i in range(k)]
        w_head = _kernels._f32c(params[4 * k]).view(-1)
        out, saved, st = _tail_forward(plan, seed, None, None, Ws, w_head, params[4 * k + 1], lead=_Lead(B, dev, gather),
                                       labels=labels)
        ctx.st = st
        ctx.prefetch = _next_batch_prefetch(dev, offsets, Wc, ldw, w1c, ldw1, F, N)
        ctx.meta = (B, F, D, N, tuple(W.shape), tuple(w1.shape), bool(sparse_W), bool(sparse_w1), bias is not None)
        ctx.save_for_backward(*saved, rows, esum)
        return out

    @staticmethod
    def backward(ctx, g):
        B, F, D, N, Wshape, w1shape, sparse_W, sparse_w1, has_bias = ctx.meta
        saved = ctx.saved_tensors
        rows, esum = saved[-2], saved[-1]
        need = ctx.needs_input_grad       # (plan, head, seed, idx, offsets, W, w1, bias, sparse_W, sparse_w1, labels, *params)
        need_W, need_w1, need_b = need[5], need[6], need[7]
        dev = rows.device
        g1vals = torch.empty((B * F,), dtype=torch.float32, device=dev) if need_w1 else None
        gvals, _, grads, db_head = _tail_backward(ctx.st, saved[:ctx.st.n_saved], g, True, need[11:], False,
                                                  fm=(esum, g1vals, D), beside_wgrad=ctx.prefetch)
        gW, gw1 = _kernels._table_grads(rows, gvals.view(B * F, D), g1vals, N, D, Wshape, w1shape, sparse_W, sparse_w1,
                                        need_W, need_w1, _lib.stream_ptr(dev))
        # the scalar bias is added to every logit, like the head's bias: the same gradient, sum_m g[m]
        gb = db_head if (has_bias and need_b) else None            # (the twin word the join wrote: no copy)
        return (None, None, None, None, None, gW, gw1, gb, None, None, None, *grads)


class SlotDeepFMFusedFn(torch.autograd.Function):
    """DeepFMFusedFn for the table-sharded step (sharded.ShardedDeepFM._local_compute): the rows come out of the receive
    buffer `recv` fp32[S + 1, D + 4] of packed {D embedding floats, first-order weight, pad} rows at row slot[b, f]
    (mi_slot_fm_fwd's operands) and their gradient goes back as that buffer's gradient — written by the epilogue of the
    tail's first input-gradient product (mi_tail_dgrad_gemm_fm_slot) into a buffer the step's one zero fill has cleared
    (padding slots travel back to their owners as zeros).  The lookup launch carries the tail's dropout bits and zero fill."""

    @staticmethod
    def forward(ctx, plan, head, seed, recv, slot, bias, labels, loss_seed, *params):
        dev = _lib.require_gpu(recv, slot)
        lib = _lib.load()
        if recv.dtype != torch.float32 or not recv.is_contiguous() or recv.dim() != 2:
            raise ValueError("recv must be a contiguous fp32 [rows, D + 4] buffer")
        slot = _kernels._i64c(slot)
        B, F = slot.shape
        rows, D = recv.shape[0], recv.shape[1] - 4
        emb = torch.empty((B, F * D), dtype=torch.float32, device=dev)
        yfm = torch.empty((B,), dtype=torch.float32, device=dev)
        esum = torch.empty((B, D), dtype=torch.float32, device=dev)

        def gather(job):
            _lib.check(lib.mi_gather_fm_fwd_ride(slot.data_ptr(), None, recv.data_ptr(), D + 4, recv.data_ptr() + 4 * D, D + 4,
                                                 _lib.ptr(bias), emb.data_ptr(), yfm.data_ptr(), None, esum.data_ptr(),
                                                 B, F, D, rows, _lib.err_word(dev).data_ptr(),
                                                 ctypes.byref(job) if job is not None else None, _lib.stream_ptr(dev)),
                       "mi_gather_fm_fwd_ride")
            return emb, yfm

        k = len(plan)
        Ws = [_kernels._f32c(params[4 * i]) for i in range(k)]
        w_head = _kernels._f32c(params[4 * k]).view(-1)
        out, saved, st = _tail_forward(plan, seed, None, None, Ws, w_head, params[4 * k + 1],
                                       lead=_Lead(B, dev, gather, extra_zero=rows * (D + 4)), labels=labels, loss_seed=loss_seed)
        ctx.st = st
        ctx.meta = (B, F, D, rows, bias is not None)
        ctx.save_for_backward(*saved, slot, esum)
        return out

    @staticmethod
    def backward(ctx, g):
        B, F, D, rows, has_bias = ctx.meta
        saved = ctx.saved_tensors
        slot, esum = saved[-2], saved[-1]
        need = ctx.needs_input_grad       # (plan, head, seed, recv, slot, bias, labels, loss_seed, *params)
        st = ctx.st
        gbuf, st.extra = st.extra, None
        if gbuf is None:                   # a second backward through the same graph: a fresh zero fill
            gbuf = torch.zeros((rows * (D + 4),), dtype=torch.float32, device=slot.device)
        gbuf = gbuf.view(rows, D + 4)
        _, _, grads, db_head = _tail_backward(st, saved[:st.n_saved], g, True, need[8:], False, fm=(esum, None, D, slot, gbuf))
        gb = db_head if (has_bias and need[5]) else None
        return (None, None, None, gbuf if need[3] else None, None, gb, None, None, *grads)


def _plan_params(plan, head):
    params = []
    for L in plan:
        params += [L.lin.weight, L.lin.bias, L.bn.weight if L.bn is not None else None, L.bn.bias if L.bn is not None else None]
    return params + [head.weight, head.bias]


def run_fused_tail(plan: List[_Layer], head: nn.Linear, seed: torch.Tensor, x: torch.Tensor,
                   last_add: Optional[torch.Tensor], labels: Optional[torch.Tensor] = None,
                   loss_seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    return FusedTailFn.apply(plan, head, seed, x, last_add, labels, loss_seed, *_plan_params(plan, head))


# DeepFM's lookup backward in the epilogue of the tail's first input-gradient product (MI_FUSED_FM_EPILOGUE=0: two nodes,
# mi_gather_fm_bwd_rows as a kernel of its own behind the tail's backward — the round-3 form)
FM_EPILOGUE = os.environ.get("MI_FUSED_FM_EPILOGUE", "1") == "1"


def run_fused_deepfm(plan: List[_Layer], head: nn.Linear, seed: torch.Tensor, idx, offsets, W, w1, bias,
                     sparse_W: bool, sparse_w1: bool, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels (optional, [B]): the step's targets — the head launch then also evaluates nn.BCEWithLogitsLoss against them and
    the head's backward (losses.BCEWithLogitsLoss finds both when it is called with these logits and labels)."""
    return DeepFMFusedFn.apply(plan, head, seed, idx, offsets, W, w1, bias, sparse_W, sparse_w1, labels,
                               *_plan_params(plan, head))


def run_fused_slot_deepfm(plan: List[_Layer], head: nn.Linear, seed: torch.Tensor, recv, slot, bias,
                          labels: Optional[torch.Tensor] = None, loss_seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    return SlotDeepFMFusedFn.apply(plan, head, seed, recv, slot, bias, labels, loss_seed, *_plan_params(plan, head))

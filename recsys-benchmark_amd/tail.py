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
import os
from collections import namedtuple
from typing import List, NamedTuple, Optional

import torch
from torch import nn

from . import _kernels, _lib

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


def _ref(struct):
    return ctypes.byref(struct) if struct is not None else None


def _load(t, ld, c, p, bits):
    """An activation as the next kernel's operand load, the seven arguments every such kernel takes: (pointer, leading
    dimension, mu, sc, be, p, keep bits) — BatchNorm + ReLU + Dropout applied on the way in; c (the layer's constants) None:
    the tensor as it is; bits None: nothing dropped."""
    mu, sc, be = (c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr()) if c is not None else (None, None, None)
    return _lib.ptr(t), ld, mu, sc, be, float(p), _lib.ptr(bits)


def _bn_fwd_struct(part, L, c, shift, nrep, seed_bump) -> "_BnFwd":
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


class _Form(NamedTuple):
    """Which launches a step takes: every decision of the driver, made once by _form() at forward time, together with the
    replica counts and deterministic mode as they stood then.  The zero buffer is laid out for this record (_zero_layout),
    the seed rule reads it (_seed_launch), and the backward reads it and no module knob: it runs the form the forward ran."""
    grad: bool            # a backward may follow
    det: bool             # deterministic mode: no float atomics, the weight-gradient kernel recomputes its operand
    merge: bool           # MERGE_JOINS: tile statistics, joined by the consuming kernel's prologue
    sums: bool            # STAT_SUMS: statistics as sums added with float atomics, derived by the consuming kernel's prologue
    R: int                # replicas of a hidden layer's sums
    Rh: int               # replicas of the head's sums
    lead_ride: bool       # the launch in front of the tail carries the keep bits, the zero fill and the fixed layers' constants
    stat_f: tuple         # per layer: its product ADDS its statistics (the first layer's only when a launch in front zeroed them)
    stat_b: bool          # the backward's column sums are added sums too
    head_loss: bool       # head + criterion + the head's backward sums in one launch (mi_tail_head_bce)
    ride: bool            # the keep bits and the zero fill ride in the first layer's finalize launch
    head_epi: bool        # the head in the last product's epilogue (nothing kept, nothing zero-filled but the logits)
    keep_inputs: bool     # a layer's input activation is stored for the weight gradient


def _form(plan, has_lead: bool, has_labels: bool, grad: bool) -> _Form:
    """The one place that reads the tail's knobs."""
    det, merge = bool(_kernels.DETERMINISTIC), MERGE_JOINS
    sums = STAT_SUMS and not merge and not det
    lead_ride = has_lead and LEAD_RIDE and sums
    stat_b = sums and grad
    last = plan[-1].lin.out_features
    return _Form(
        grad=grad, det=det, merge=merge, sums=sums, R=STAT_REPS, Rh=HEAD_REPS, lead_ride=lead_ride,
        stat_f=tuple(sums and (i >= 1 or lead_ride) and not L.fixed for i, L in enumerate(plan)), stat_b=stat_b,
        head_loss=has_labels and HEAD_LOSS and stat_b and last <= 512 and last % 4 == 0,
        # (that launch exists — a training-mode BatchNorm on the first layer — and a LATER kernel can advance the seed)
        ride=RIDE_MASKS and not merge and len(plan) >= 2 and not plan[0].fixed and not lead_ride,
        # inference, every layer on fixed statistics (so the layout below is empty): the logits are zero-filled by the lead launch
        head_epi=(HEAD_EPILOGUE and lead_ride and not grad and not has_labels and all(L.fixed and L.p == 0 for L in plan)
                  and last % 4 == 0),
        keep_inputs=grad and not det)


# _zero_layout's result, slices of the step's zero-filled buffer (None / empty: the form has no such block) and its size.
# w / b: per layer, where the weight gradient's split-K slices meet and the (exactly zero) bias gradient under a training-mode
# BatchNorm; fsum / bsum: {layer: its forward sums, R x 4 N (fp64 pairs) / its backward column sums, R x 2 N}; head: the
# head's column sums, Rh x N x 2, and right behind them head_w: its dw / db rows, Rh x (N + 4); loss: mi_tail_head_bce's
# workspace (its first float is the loss); extra: the caller's floats (_Lead.extra_zero)
_Layout = namedtuple("_Layout", "w b fsum bsum head head_w loss extra total")


def _zero_layout(dims, form: _Form, extra_zero: int = 0) -> _Layout:
    """ONE zero-filled buffer per step for everything that accumulates; dims: (N, K) per layer.  The alignment rule: every
    block starts on a multiple of 4 floats — the zero fill and the kernels' float4 accesses need 16 bytes, the fp64 forward
    sums 8 — so the total is one too."""
    at = 0

    def take(n):
        nonlocal at
        cut, at = slice(at, at + n), at + (n + 3) // 4 * 4
        return cut

    wb = [(take(N * K), take(N)) for N, K in dims] if form.grad else []
    fsum = {i: take(form.R * 4 * N) for i, (N, _) in enumerate(dims) if form.stat_f[i]}
    bsum, head, head_w, loss = {}, None, None, None
    if form.stat_b:
        bsum = {i: take(form.R * 2 * N) for i, (N, _) in enumerate(dims[:-1])}
        head, head_w = take(form.Rh * 2 * dims[-1][0]), take(form.Rh * (dims[-1][0] + 4))
        if form.head_loss:
            loss = take(int(_lib.load().mi_tail_head_bce_ws_elems(form.Rh)))
    extra = take(extra_zero) if (extra_zero > 0 and form.grad) else None
    assert not (form.head_epi and at), "the head-in-epilogue form has no zero buffer: the lead launch zero-fills the logits"
    return _Layout(tuple(w for w, _ in wb), tuple(b for _, b in wb), fsum, bsum, head, head_w, loss, extra, at)


def _seed_launch(plan, form: _Form):
    """The launch that advances the dropout seed — exactly once per step, after the launch that made the keep bits:
    ("finalize", i): layer i's finalize launch; ("join", i): the first kernel that joins pending statistics, layer i's product
    or (i = k) the head; ("head", k): the head alone, with nothing to join.  None: no layer drops."""
    if not any(L.p > 0 for L in plan):
        return None
    k, pending = len(plan), False
    first = 1 if form.ride else 0          # (a finalize launch that carries the mask job MADE the bits: the next one advances)
    for i, L in enumerate(plan):
        if pending:
            return "join", i
        pending = not L.fixed and (form.stat_f[i] or form.merge)
        if not L.fixed and not pending and i == first and not (form.sums and k >= 2):
            return "finalize", i           # (sums: the first deriving kernel advances the seed instead)
    return ("join", k) if pending else ("head", k)


class _Saved(namedtuple("_Saved", "x w_head Ws Zs consts bits gammas acts")):
    """The tensors the forward keeps for the backward, by name; the fields from Ws on hold one entry per layer, None where
    nothing is kept.  flat() is what ctx.save_for_backward takes, of() reads it back (a caller's own tensors may follow)."""

    def flat(self):
        return [self.x, self.w_head, *(t for per_layer in self[2:] for t in per_layer)]

    @classmethod
    def of(cls, flat, k):
        return cls(flat[0], flat[1], *(flat[2 + j * k: 2 + (j + 1) * k] for j in range(len(cls._fields) - 2)))


class _State:
    """What the forward leaves for the backward besides the saved tensors."""
    __slots__ = ("plan", "form", "lay", "zeros", "head", "extra", "has_head_bias", "add_shape")


# The kernel in front of the tail that produces its input (DeepFM: gather + FM): `launch(job)` runs it — carrying the
# mask job (a mi_tail_mask_ride or None) — and returns (x[M, K], last_add or None).  extra_zero: floats the step's
# zero-filled buffer should hold for the caller besides the tail's own accumulators (state.extra).
_Lead = namedtuple("_Lead", "M dev launch extra_zero", defaults=(0,))


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


def _tail_forward(plan, seed, x, last_add, params, lead: Optional[_Lead] = None, labels=None, loss_seed=None):
    """The forward kernels of the tail; returns (out[M, 1], tensors to save, state).  params: (W, b, gamma, beta) per hidden
    layer, then the head's (w, b).  lead (instead of x / last_add): the launch that produces them, run here once the mask job
    it carries is known.  labels ([M] fp32, optional): the head launch also evaluates BCE-with-logits against them and the
    head's backward sums (state.head) for the upstream gradient loss_seed (a device scalar: what the caller will seed the
    criterion's backward with; None: losses.unit_scalar)."""
    lib = _lib.load()
    dev = lead.dev if lead is not None else _lib.require_gpu(x)
    s = _lib.stream_ptr(dev)
    M = lead.M if lead is not None else x.shape[0]
    k = len(plan)
    Ws = [_kernels._f32c(params[4 * i]) for i in range(k)]
    w_head, b_head = _kernels._f32c(params[4 * k]).view(-1), params[4 * k + 1]
    form = _form(plan, lead is not None, labels is not None, bool(getattr(plan, "grad", True)))
    lay = _zero_layout([(L.lin.out_features, L.lin.in_features) for L in plan], form, lead.extra_zero if lead is not None else 0)
    seed_at = _seed_launch(plan, form)
    R, Rh = form.R, form.Rh

    def bump(*launch):
        return seed.data_ptr() if launch == seed_at else None

    zeros = torch.empty((lay.total,), dtype=torch.float32, device=dev) if lay.total else None
    out_pad = torch.empty(((M + 3) // 4 * 4,), dtype=torch.float32, device=dev) if form.head_epi else None
    if form.lead_ride:
        # the launch in front of the tail carries the keep bits, the zero fill AND the constants of the fixed-statistics layers
        bits, lead_job = _masks(seed, plan, M, dev, out_pad if form.head_epi else zeros, ride=True)
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
        bits, job = _masks(seed, plan, M, dev, zeros, ride=True) if form.ride else (_masks(seed, plan, M, dev, zeros), None)
        fixed_c = _fixed_constants(plan, dev, s)
    Zs, consts, acts = [], [], []
    prev = (x, plan[0].lin.in_features, None, 0.0, None)      # the next kernel's operand load (_load)
    pending = None            # (part, layer, constants, shift, replicas) of the layer whose statistics the next kernel joins
    for i, L in enumerate(plan):
        N, K = L.lin.out_features, L.lin.in_features
        if form.head_epi and i == k - 1:   # the last hidden layer of an inference forward: product + head, z not stored
            c = fixed_c[i]
            hadd = None if last_add is None else _kernels._f32c(last_add).view(-1)
            epi = _HeadEpi(w_head.data_ptr(), _lib.ptr(b_head), _lib.ptr(hadd), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
                           out_pad.data_ptr())
            _lib.check(lib.mi_tail_fwd_gemm_head(*_load(*prev), Ws[i].data_ptr(), K, M, N, K, None, ctypes.byref(epi), s),
                       "mi_tail_fwd_gemm_head")
            acts.append(None)
            Zs.append(None)
            consts.append(c)
            continue
        Z = torch.empty((M, N), dtype=torch.float32, device=dev)
        part = shift = None
        if L.fixed:
            c = fixed_c[i]
        else:
            c = torch.empty((4, N), dtype=torch.float32, device=dev)          # mu, sc, be, rstd
            if form.stat_f[i]:
                part = zeros[lay.fsum[i]]
                shift = torch.empty((N,), dtype=torch.float32, device=dev)
            else:
                part = torch.empty(int(lib.mi_tail_part_elems(M, N)), dtype=torch.float32, device=dev)
        # the layer's input activation as its operand load computes it, kept for the weight gradient (not in
        # deterministic mode, whose weight-gradient kernel recomputes it)
        a_in = torch.empty((M, K), dtype=torch.float32, device=dev) if (form.keep_inputs and prev[2] is not None) else None
        stats = _bn_fwd_struct(*pending, bump("join", i)) if pending is not None else None
        pending = None
        _lib.check(lib.mi_tail_fwd_gemm_s(
            *_load(*prev), Ws[i].data_ptr(), K, Z.data_ptr(), N, _lib.ptr(part), _lib.ptr(a_in), M, N, K, _ref(stats),
            R if form.stat_f[i] else 0, _lib.ptr(shift), L.bn.running_mean.data_ptr() if form.stat_f[i] else None,
            _lib.ptr(L.lin.bias) if form.stat_f[i] else None, s), "mi_tail_fwd_gemm_s")
        acts.append(a_in)
        if not L.fixed and (form.stat_f[i] or form.merge):
            pending = (part, L, c, shift, R if form.stat_f[i] else 0)
        elif not L.fixed:
            bn = L.bn
            _lib.check(lib.mi_tail_bn_finalize_fwd_r(
                part.data_ptr(), M, N, bn.weight.data_ptr(), bn.bias.data_ptr(), _lib.ptr(L.lin.bias),
                bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.momentum), float(bn.eps),
                bn.num_batches_tracked.data_ptr(), bump("finalize", i), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
                c[3].data_ptr(), _ref(job[0]) if (i == 0 and job is not None) else None, s), "mi_tail_bn_finalize_fwd_r")
        Zs.append(Z)
        consts.append(c)
        prev = (Z, N, c, L.p, bits[i])
    out = out_pad[:M].view(M, 1) if form.head_epi else torch.empty((M, 1), dtype=torch.float32, device=dev)
    add = None if last_add is None else _kernels._f32c(last_add).view(-1)
    N = plan[-1].lin.out_features
    if pending is not None:
        stats = _bn_fwd_struct(*pending, bump("join", k))
    else:                              # nothing left to join: the head only advances the seed (part = NULL), if it is the one
        stats = _BnFwd(seed_bump=seed.data_ptr()) if seed_at == ("head", k) else None
    head = None
    if form.head_loss:
        y = _kernels._f32c(labels).view(-1)
        if y.numel() != M:
            raise ValueError("labels must hold one value per row of the batch")
        head = _HeadLoss()
        head.out, head.y, head.y_key = out, y, _label_key(labels)
        head.gvec = torch.empty((M,), dtype=torch.float32, device=dev)
        loss_ws = zeros[lay.loss]
        head.loss = loss_ws[:1]
        if loss_seed is None:
            from .losses import unit_scalar

            head.seed = unit_scalar(dev)
        else:
            if loss_seed.numel() != 1 or loss_seed.dtype != torch.float32 or loss_seed.device != dev:
                raise ValueError("loss_seed must be a float32 device scalar")
            head.seed = loss_seed
        DY = torch.empty((M, N), dtype=torch.float32, device=dev)
        _lib.check(lib.mi_tail_head_bce(
            *_load(*prev), w_head.data_ptr(), _lib.ptr(b_head), _lib.ptr(add), y.data_ptr(), out.data_ptr(), head.gvec.data_ptr(),
            DY.data_ptr(), zeros[lay.head].data_ptr(), zeros[lay.head_w].data_ptr(), Rh, loss_ws.data_ptr(), M, N, _ref(stats),
            _lib.ptr(loss_seed), s), "mi_tail_head_bce")
        head.out_version, head.seed_version = out._version, head.seed._version
        _HEAD_LOSS[str(dev)] = head
    elif not form.head_epi:            # (head_epi: the logits came out of the last product's epilogue)
        _lib.check(lib.mi_tail_head_fwd_m(*_load(*prev), w_head.data_ptr(), _lib.ptr(b_head), _lib.ptr(add), out.data_ptr(), M, N,
                                          _ref(stats), s), "mi_tail_head_fwd_m")
    st = _State()
    st.plan, st.form, st.lay, st.zeros = plan, form, lay, zeros
    st.head = (head.gvec, DY) if head is not None else None
    st.extra = zeros[lay.extra] if lay.extra is not None else None
    st.has_head_bias, st.add_shape = b_head is not None, None if last_add is None else tuple(last_add.shape)
    saved = _Saved(x, w_head, Ws, Zs, consts, bits, [L.bn.weight if L.bn is not None else None for L in plan], acts)
    return out, saved.flat(), st


def _tail_backward(st, saved, g, need_x: bool, need_params, need_add: bool, fm=None, beside_wgrad=None):
    """The backward kernels of the tail, in the form the forward ran (st.form) on the buffer it laid out (st.lay).  saved: the
    forward's tensors as ctx.saved_tensors returns them.  need_params[j]: whether parameter j of (W, b, gamma, beta) x k +
    (w, b)_head wants a gradient.  fm (DeepFM, the tail's input is the embedding block): (emb_sum[M, D], g1vals[M, F] or None,
    D) — the first layer's input-gradient product then writes the lookup table's row-form gradient instead of dx
    (mi_tail_dgrad_gemm_fm) and the returned dx IS that [M, F*D] buffer.  Returns (dx, dadd, grads, db_head)."""
    lib = _lib.load()
    plan, form, lay = st.plan, st.form, st.lay
    if not form.grad:
        raise RuntimeError("the fused tail's plan was made with grad mode off: its forward kept nothing for a backward")
    k = len(plan)
    x, w_head, Ws, Zs, consts, bits, gammas, acts = _Saved.of(saved, k)
    dev, M = x.device, x.shape[0]
    s = _lib.stream_ptr(dev)
    gvec = _kernels._f32c(g).view(M)
    later = []           # weight-gradient products for ONE launch at the end
    zeros = st_zeros = st.zeros            # filled by the forward's mask launch; a second backward needs a fresh one
    st.zeros = None
    if zeros is None:
        zeros = torch.zeros((lay.total,), dtype=torch.float32, device=dev)
    stat, R, Rh = form.stat_b, form.R, form.Rh
    grads: List[Optional[torch.Tensor]] = [None] * (4 * k + 2)

    # ---- head: dy of the last hidden layer, its column sums, dw / db of the head
    N = Zs[-1].shape[1]
    DY = None if st.head is not None else torch.empty((M, N), dtype=torch.float32, device=dev)
    if stat:            # sums added into Rh zeroed rows: joined by the next product's prologue, no finalize launch
        nblk = Rh
        part, wpart = zeros[lay.head].view(Rh, N, 2), zeros[lay.head_w].view(Rh, N + 4)
    else:
        nblk = int(lib.mi_tail_head_blocks(M))
        part = torch.empty((nblk, N, 2), dtype=torch.float32, device=dev)
        wpart = torch.empty((nblk, N + 4), dtype=torch.float32, device=dev)
    fused_head, st.head = st.head, None
    if (fused_head is not None and stat and zeros is st_zeros and gvec.data_ptr() == fused_head[0].data_ptr()):
        DY = fused_head[1]        # the forward's head launch wrote DY and the sums for exactly this gradient
    else:
        if fused_head is not None and zeros is st_zeros:
            zeros[lay.head.start: lay.head_w.stop].zero_()          # ... for an upstream gradient of 1: not this one
        if DY is None:
            DY = torch.empty((M, N), dtype=torch.float32, device=dev)
        _lib.check(lib.mi_tail_head_bwd_s(*_load(Zs[-1], N, consts[-1], plan[-1].p, bits[-1]), gvec.data_ptr(), w_head.data_ptr(),
                                          DY.data_ptr(), part.data_ptr(), wpart.data_ptr(), Rh if stat else 0, M, N, s),
                   "mi_tail_head_bwd_s")
    dw_head = torch.empty((1, N), dtype=torch.float32, device=dev)
    db_head = torch.empty((1,), dtype=torch.float32, device=dev)
    # DeepFM's scalar bias is added to every logit like the head's bias: same gradient, written to a second word by the
    # same join (a clone would be a copy launch per step)
    db_twin = torch.empty((1,), dtype=torch.float32, device=dev) if fm is not None else None
    part_rows, wp, nw = nblk, wpart, nblk
    dx = None
    for i in range(k - 1, -1, -1):
        N, K = Zs[i].shape[1], Ws[i].shape[1]
        L, c = plan[i], consts[i]
        dgb = torch.empty((2, N), dtype=torch.float32, device=dev)
        dzc = torch.empty((3, N), dtype=torch.float32, device=dev)         # al, bz, de
        dbias = torch.empty((N,), dtype=torch.float32, device=dev) if (L.fixed and L.lin.bias is not None) else None
        # the activation below as an operand load: what this layer's product multiplied
        below = (Zs[i - 1], K, consts[i - 1], plan[i - 1].p, bits[i - 1]) if i > 0 else (x, K, None, 0.0, None)
        runs_dgrad = i > 0 or need_x
        # the column sums behind dz's constants: joined in the input-gradient product's prologue, or (no such product
        # for this layer, or the joined forms off) by the finalize launch
        sums = None
        head_dw, head_db, twin = (dw_head.data_ptr(), db_head.data_ptr(), _lib.ptr(db_twin)) if wp is not None else (None, None, None)
        if (form.merge or stat) and runs_dgrad and part_rows <= 128:      # (256 partial rows of the head keep their finalize launch)
            sums = _BnBwd(part.data_ptr(), _lib.ptr(gammas[i]), c[3].data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(),
                          dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(), _lib.ptr(wp), head_dw, head_db,
                          part_rows, nw, _lib.ptr(dbias), twin, int(L.fixed))
        else:
            _lib.check(lib.mi_tail_bn_finalize_bwd_b(
                part.data_ptr(), part_rows, M, N, _lib.ptr(gammas[i]), c[3].data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(),
                dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr(), _lib.ptr(wp), nw, head_dw, head_db, int(L.fixed),
                _lib.ptr(dbias), twin, s), "mi_tail_bn_finalize_bwd_b")
        wp = None
        if L.bn is not None:
            grads[4 * i + 2], grads[4 * i + 3] = dgb[0], dgb[1]
        if need_params[4 * i + 1] and L.lin.bias is not None:
            # under a training-mode BatchNorm the batch mean is removed: exactly zero; otherwise al * sum dy
            grads[4 * i + 1] = dbias if L.fixed else zeros[lay.b[i]]
        a_in = x if i == 0 else acts[i]
        defer = need_params[4 * i] and runs_dgrad and a_in is not None and not form.det
        dz_keep = torch.empty((M, N), dtype=torch.float32, device=dev) if defer else None
        # (dy, z and the constants that turn them into dz: the first operand of both products of this layer)
        dz = (DY.data_ptr(), Zs[i].data_ptr(), N, c[0].data_ptr(), dzc[0].data_ptr(), dzc[1].data_ptr(), dzc[2].data_ptr())
        if runs_dgrad:
            OUT = torch.empty((M, K), dtype=torch.float32, device=dev)
            if i > 0 and stat:             # the layer below's column sums: added into R zeroed rows (float atomics)
                npart = zeros[lay.bsum[i - 1]]
            else:
                npart = torch.empty(int(lib.mi_tail_part_elems(M, K)), dtype=torch.float32, device=dev) if i > 0 else None
            if i == 0 and fm is not None and len(fm) == 5:      # the sharded step: rows go back into the receive buffer's gradient
                emb_sum, _, D, slot, gbuf = fm
                OUT = gbuf
                _lib.check(lib.mi_tail_dgrad_gemm_fm_slot(
                    *dz, Ws[i].data_ptr(), K, gbuf.data_ptr(), _lib.ptr(dz_keep), M, N, K, _ref(sums), x.data_ptr(),
                    emb_sum.data_ptr(), gvec.data_ptr(), slot.data_ptr(), D, s), "mi_tail_dgrad_gemm_fm_slot")
            elif i == 0 and fm is not None:
                emb_sum, g1vals, D = fm
                _lib.check(lib.mi_tail_dgrad_gemm_fm(
                    *dz, Ws[i].data_ptr(), K, OUT.data_ptr(), _lib.ptr(dz_keep), M, N, K, _ref(sums), x.data_ptr(),
                    emb_sum.data_ptr(), gvec.data_ptr(), _lib.ptr(g1vals), D, s), "mi_tail_dgrad_gemm_fm")
            else:                          # (layer 0 has no layer below whose dy the epilogue would make: no load)
                _lib.check(lib.mi_tail_dgrad_gemm_s(
                    *dz, Ws[i].data_ptr(), K, *(_load(*below) if i > 0 else _load(None, K, None, 0.0, None)), OUT.data_ptr(), K,
                    _lib.ptr(npart), R if (stat and i > 0) else 0, _lib.ptr(dz_keep), M, N, K, _ref(sums), s),
                    "mi_tail_dgrad_gemm_s")
        # the weight gradient comes AFTER the input-gradient product: in the joined form that product's workgroup 0 is
        # what writes al / bz / de
        if defer:
            dW = zeros[lay.w[i]].view(N, K)                               # split-K slices meet in atomics
            later.append(dict(A=dz_keep, B=a_in, C=dW, M=N, N=K, K=M, lda=N, ldb=K, ldc=K))   # dW = dz^T a_in
            grads[4 * i] = dW
        elif need_params[4 * i]:
            splits = int(lib.mi_tail_wgrad_splits(M, N, K))
            slab = torch.empty((splits, N, K), dtype=torch.float32, device=dev)
            dW = torch.empty((N, K), dtype=torch.float32, device=dev)
            _lib.check(lib.mi_tail_wgrad_gemm(*dz, *_load(*below), slab.data_ptr(), dW.data_ptr(), M, N, K, s), "mi_tail_wgrad_gemm")
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
        out, saved, ctx.st = _tail_forward(plan, seed, _kernels._f32c(x), last_add, params, labels=labels, loss_seed=loss_seed)
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


def _fm_lead(dev, ids, offsets, W, ldw, w1, ldw1, bias, rows, D, N, extra_zero=0):
    """The _Lead of DeepFM's lookup, gather + FM + first-order term (mi_gather_fm_fwd_ride), and the emb_sum[B, D] it leaves
    for the backward.  Table form: ids[B, F] + offsets[F] address rows of W / w1 (pointers, with their row strides), the
    global rows are written to `rows`; slot form (offsets and rows None): ids are rows of the receive buffer itself."""
    lib = _lib.load()
    B, F = ids.shape
    emb = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    yfm = torch.empty((B,), dtype=torch.float32, device=dev)
    esum = torch.empty((B, D), dtype=torch.float32, device=dev)

    def gather(job):      # (job: the tail's mask work, carried in extra workgroups of this launch)
        _lib.check(lib.mi_gather_fm_fwd_ride(ids.data_ptr(), _lib.ptr(offsets), W, ldw, w1, ldw1, _lib.ptr(bias), emb.data_ptr(),
                                             yfm.data_ptr(), _lib.ptr(rows), esum.data_ptr(), B, F, D, N,
                                             _lib.err_word(dev).data_ptr(), _ref(job), _lib.stream_ptr(dev)),
                   "mi_gather_fm_fwd_ride")
        return emb, yfm

    return _Lead(B, dev, gather, extra_zero), esum


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
        Wc, ldw = _kernels._row_strided(W)
        N, D = Wc.shape
        idx, offsets, w1c, ldw1, _ = _kernels._lookup_operands(idx, offsets, w1, N)
        B, F = idx.shape
        rows = torch.empty((B, F), dtype=torch.int64, device=dev)
        lead, esum = _fm_lead(dev, idx, offsets, Wc.data_ptr(), ldw, w1c.data_ptr(), ldw1, bias, rows, D, N)
        _kernels.note_field_layout(rows, offsets, N)
        out, saved, ctx.st = _tail_forward(plan, seed, None, None, params, lead=lead, labels=labels)
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
        gvals, _, grads, db_head = _tail_backward(ctx.st, saved, g, True, need[11:], False, fm=(esum, g1vals, D),
                                                  beside_wgrad=ctx.prefetch)
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
        if recv.dtype != torch.float32 or not recv.is_contiguous() or recv.dim() != 2:
            raise ValueError("recv must be a contiguous fp32 [rows, D + 4] buffer")
        slot = _kernels._i64c(slot)
        B, F = slot.shape
        rows, D = recv.shape[0], recv.shape[1] - 4
        lead, esum = _fm_lead(dev, slot, None, recv.data_ptr(), D + 4, recv.data_ptr() + 4 * D, D + 4, bias, None, D, rows,
                              extra_zero=rows * (D + 4))
        out, saved, ctx.st = _tail_forward(plan, seed, None, None, params, lead=lead, labels=labels, loss_seed=loss_seed)
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
        _, _, grads, db_head = _tail_backward(st, saved, g, True, need[8:], False, fm=(esum, None, D, slot, gbuf))
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



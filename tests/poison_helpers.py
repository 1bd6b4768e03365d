"""NaN-poisoned allocations: the package allocates its buffers with torch.empty / empty_like / new_empty and promises that
a kernel writes every element anything later reads.  `poisoned()` fills each such float buffer with NaN before the kernel
sees it, so a broken promise is a deterministic NaN instead of whatever the caching allocator handed back; a recorder
notes which allocation sites of the package a run reached, `allocation_sites()` lists all of them (AST scan), and `CASES`
is the catalogue of op families that tests/test_poison_gpu.py runs clean and poisoned.

A case is `Case(name, run, check, exact)`: `run()` builds seeded CPU inputs, runs one op family forward and backward on
the GPU and returns {name: tensor} of everything a caller would see; `check(result)` applies the comparison (reference
and tolerance) that the op's own test file applies — imported from it or restated next to a pointer to it —; `exact`
says which returned tensors have a fixed summation order (or exactly representable sums), so that the poisoned and the
clean run must agree bit for bit."""
import ast
import contextlib
import copy
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "recsys-benchmark_amd")
NAMES = ("empty", "empty_like", "new_empty", "empty_strided")
DEV = "cuda"

# ------------------------------------------------------------------------------------------------------ the context manager
_recorded = set()          # (file relative to the package, line) of the calls seen while a recorder was active


@contextlib.contextmanager
def poisoned(device_type="cuda", fill=True, record=None):
    """Replaces torch.empty, torch.empty_like, torch.empty_strided and torch.Tensor.new_empty by wrappers that call the real
    function and then (fill=True) fill a non-empty floating-point result on `device_type` with NaN.  Integer, uint8 and bool
    tensors are left as they come: some carry indices, and a poisoned index could address outside a buffer.  Each wrapper
    notes its caller's (file, line) when that frame lies inside the package (`record`: a set to note into, default the
    module's own, read with `recorded()`).  The originals are restored on exit, also after an exception."""
    sink = _recorded if record is None else record
    targets = [(torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty")]
    originals = [(owner, name, getattr(owner, name)) for owner, name in targets]

    def wrap(real):
        def wrapper(*args, **kwargs):
            out = real(*args, **kwargs)
            frame = sys._getframe(1)
            fn = frame.f_code.co_filename
            if not fn.startswith("<"):
                fn = os.path.realpath(fn)
                if fn.startswith(os.path.realpath(PKG_DIR) + os.sep):
                    sink.add((os.path.relpath(fn, os.path.realpath(PKG_DIR)), frame.f_lineno))
            if (fill and isinstance(out, torch.Tensor) and out.is_floating_point() and out.numel() > 0
                    and out.device.type == device_type):
                with torch.no_grad():
                    out.fill_(float("nan"))
            return out

        wrapper.__wrapped__ = real
        return wrapper

    try:
        for owner, name, real in originals:
            setattr(owner, name, wrap(real))
        yield sink
    finally:
        for owner, name, real in originals:
            setattr(owner, name, real)


def recorded():
    return set(_recorded)


def clear_recorded():
    _recorded.clear()


# -------------------------------------------------------------------------------------------------------- the allocation sites
@functools.lru_cache(maxsize=None)
def allocation_sites(pkg_dir=PKG_DIR):
    """[(file relative to the package, lineno, end_lineno, col_offset)] of every call in the package whose attribute is one of
    NAMES (the column tells apart two calls that start on one line)."""
    sites = []
    for base, _dirs, files in sorted(os.walk(pkg_dir)):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(base, f)
            with open(path, encoding="utf-8") as fh:
                tree = ast.parse(fh.read(), path)
            for node in ast.walk(tree):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in NAMES:
                    sites.append((os.path.relpath(path, pkg_dir), node.lineno, node.end_lineno, node.col_offset))
    return sorted(sites)


def sites_of(file, line, sites=None):
    """The sites a recorded (file, line) matches: those whose call node spans the line (lineno..end_lineno).  Calls that share
    a line cannot be told apart by the recorder and are reached together."""
    return [s for s in (allocation_sites() if sites is None else sites) if s[0] == file and s[1] <= line <= s[2]]


def site_key(site):
    return f"{site[0]}:{site[1]}:{site[3]}"


def reached_sites(record, sites=None):
    sites = allocation_sites() if sites is None else sites
    return {s for f, ln in record for s in sites_of(f, ln, sites)}


# Sites the catalogue cannot reach in one eager process, "file:line:column" -> the reason read from the code (needs a process group,
# runs only inside a capture, is a CPU-only branch).
NOT_REACHED = {
    "_kernels.py:2708:15": "runs only inside a capture: _auc_workspace hands a capture a buffer of the graph's own pool",
    "embeddings/dh_embedding.py:153:19": "is a CPU-only branch: the host-built per-item hash table of an empty id range",
    "embeddings/tensortrain_embeddings.py:141:22": "is a CPU-only branch: a numpy array of the host-side approx-uniform initialiser",
    "embeddings/tensortrain_embeddings.py:141:55": "is a CPU-only branch: a numpy array of the host-side approx-uniform initialiser",
    "sharded.py:366:21": "needs a process group: _Exchange.forward's receive buffer of the row-id all-to-all",
    "sharded.py:372:19": "needs a process group: _Exchange.forward's receive buffer of the packed-row all-to-all",
    "sharded.py:385:18": "needs a process group: _Exchange.backward's receive buffer of the gradient all-to-all",
    "sharded.py:436:12": "needs a process group: ShardedDeepFM.__init__ asks the group for its rank and world size first",
    "sharded.py:437:13": "needs a process group: ShardedDeepFM.__init__ asks the group for its rank and world size first",
    "sharded.py:711:25": "needs a process group: the graphed step's all-to-all of the row ids",
    "sharded.py:722:26": "needs a process group: the graphed step's all-to-all of the gradient rows",
}


# ------------------------------------------------------------------------------------------------------------ the catalogue
class Case:
    def __init__(self, name, run, check, exact=False):
        self.name, self._run, self.check = name, run, check
        self.exact = exact if callable(exact) else (lambda key, _e=bool(exact): _e)

    def run(self):
        _reset()
        return {k: v for k, v in self._run().items() if v is not None}

    def __repr__(self):
        return self.name


SEED_WORD = 20240607


def _reset():
    """A case is repeatable: the generators, the dropout seed word and the kept workspaces are what a first call finds."""
    from recsys_benchmark_amd import _kernels, losses, mlp

    torch.manual_seed(0)
    if torch.cuda.is_available():
        mlp._seed_word(torch.device("cuda", torch.cuda.current_device())).fill_(SEED_WORD)
    for cache in (_kernels._DUAL_WS, _kernels._plans, _kernels._hccf_plans, _kernels._auc_workspaces, _kernels._field_layouts,
                  losses._workspaces):
        cache.clear()


def dense(t):
    return t.to_dense() if t.is_sparse else t


def values_of(t):
    """What the NaN / Inf check reads: a sparse gradient's values, any other tensor itself."""
    return t._values() if t.is_sparse else t


def _cmp(result, ref, tol, default):
    from conftest import assert_close

    for k, want in ref.items():
        rtol, atol = tol.get(k, default)
        assert_close(dense(result[k]), want, rtol, atol, k)


@contextlib.contextmanager
def _deterministic(on):
    """The package's deterministic switch set to `on` for the block, then back to what it was."""
    import recsys_benchmark_amd as pkg
    from recsys_benchmark_amd import _kernels

    before = _kernels.DETERMINISTIC
    pkg.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        pkg.use_deterministic_algorithms(before)


@contextlib.contextmanager
def _patched(*settings):
    mp = pytest.MonkeyPatch()
    try:
        for obj, name, value in settings:
            mp.setattr(obj, name, value)
        yield mp
    finally:
        mp.undo()


def autograd_case(name, inputs, op, ref, tol=None, default=(0.0, 0.0), exact=False, int_grads=False, settings=(), place=None):
    """A case over an autograd op: inputs() -> (leaves, consts) on the CPU (float leaves get gradients); op(**leaves, **consts)
    -> {name: tensor} on the device; ref the same formula over float64 CPU leaves.  The loss is sum_k <out_k, G_k> with seeded
    G_k; returned are the outputs and "d<leaf>" for every leaf.  The float64 reference is computed once and kept."""
    cache = {}

    def grads_for(outs):
        gen = torch.Generator().manual_seed(97)
        return {k: (torch.randint(-2, 3, tuple(v.shape), generator=gen).float() if int_grads else
                    torch.randn(tuple(v.shape), generator=gen)) for k, v in sorted(outs.items()) if v.requires_grad}

    def evaluate(fn, to, place=None):
        leaves, consts = inputs()
        # (place: how the device run lays its leaves out, e.g. as views of one packed buffer)
        lv = place(leaves) if place is not None else {k: to(v).requires_grad_(True) for k, v in leaves.items()}
        cv = {k: (to(v) if isinstance(v, torch.Tensor) else v) for k, v in consts.items()}
        outs = fn(**lv, **cv)
        G = grads_for(outs)
        torch.autograd.backward([outs[k] for k in G], [to(G[k]).to(outs[k].dtype) for k in G])
        res = {k: v.detach() for k, v in outs.items()}
        res.update({"d" + k: v.grad for k, v in lv.items()})
        return res

    def run():
        from recsys_benchmark_amd import _lib

        with _patched(*(settings() if callable(settings) else settings)):
            res = evaluate(op, lambda t: t.to(DEV), place)
        _lib.check_index_errors()
        return res

    def check(result):
        if "ref" not in cache:
            cache["ref"] = evaluate(ref, lambda t: t.double() if t.is_floating_point() else t)
        want = {k: v for k, v in cache["ref"].items() if v is not None}
        assert set(want) == set(result), f"{name}: returned {sorted(result)} vs reference {sorted(want)}"
        _cmp(result, want, tol or {}, default)

    return Case(name, run, check, exact)


# ---- gather_fm: the PEP forms (tests/test_pep_deepfm_gpu.py) and the plain / masked forms ------------------------------------
FD_SHAPES = [(3, 4), (26, 16), (39, 16), (70, 8), (26, 64), (5, 12)]          # test_pep_deepfm_gpu.SHAPES
FM_BATCHES = [1, 37]


def _three_forms(run_one):
    """{form/key: tensor} of one gather_fm-style run in the three gradient forms: dense (float atomics), rows (COO) and
    deterministic (sorted, ordered sums)."""
    out = {}
    for form in ("dense", "rows", "det"):
        with _deterministic(form == "det"):
            r = run_one(form == "rows")
        out.update({f"{form}/{k}": v for k, v in r.items() if v is not None})
    return out


def _fm_exact(key):
    # the forward and the row-form values have a fixed order; deterministic mode orders the dense sums too; the dense default
    # adds with float atomics
    return not key.startswith("dense/g")


def _soft_case(F, D, B, kind):
    def run():
        import test_pep_deepfm_gpu as tp

        c = tp._case(F, D, B)
        return _three_forms(lambda sparse: tp._run(c, c["W_" + kind], sparse, soft=c["s_" + kind]))

    def check(result):
        import test_pep_deepfm_gpu as tp

        tp.test_soft_gather_fm_against_the_lookup_and_float64(F, D, B, kind)
        _fm_det_matches_dense(result)

    return Case(f"gather_fm-soft-{kind}-F{F}-D{D}-B{B}", run, check, _fm_exact)


def _fm_det_matches_dense(result):
    """The deterministic form against the float64-checked dense one: the same sums in another order, at the tolerance
    tests/test_pep_deepfm_gpu.py holds y_fm to (2e-5) — the values themselves were bracketed against float64 by the lifted
    test on the dense and the row form."""
    from conftest import assert_close

    for k, v in result.items():
        if k.startswith("det/"):
            assert_close(dense(v), dense(result["dense/" + k[4:]]).cpu(), 2e-5, 2e-5, k)


def _mask_case(F, D, B):
    def run():
        import test_pep_deepfm_gpu as tp

        c = tp._case(F, D, B)
        return _three_forms(lambda sparse: tp._run(c, c["W_mask"], sparse, elem_mask=c["M"]))

    def check(result):
        import test_pep_deepfm_gpu as tp

        tp.test_elemmask_gather_fm_against_the_lookup_and_float64(F, D, B)
        _fm_det_matches_dense(result)

    return Case(f"gather_fm-elemmask-F{F}-D{D}-B{B}", run, check, _fm_exact)


def _plain_fm_case(F, D, B, masked, packed=False):
    """The unmasked and the keep / fwidth-masked lookup against the float64 formula of oracle/reference_ops.py
    (fm_second_order, first_order) over the masked table rows; tolerance of tests/test_pep_deepfm_gpu.py: y_fm 2e-5, the
    gradients within 8 eps32 sum|terms| there — restated here as rtol 2e-5 on sums of at most B * F randn terms with an
    absolute floor of 2e-5."""
    def inputs():
        import test_pep_deepfm_gpu as tp

        c = tp._case(F, D, B)
        gen = torch.Generator().manual_seed(17 * F + D + B)
        leaves = dict(W=c["W_mask"], w1=c["w1"], bias=c["bias"])
        consts = dict(x=c["x"], offsets=c["offsets"])
        if masked:
            consts["keep"] = torch.randint(0, D + 1, (c["N"],), generator=gen).to(torch.uint8)
            consts["fwidth"] = torch.randint(1, D + 1, (F,), generator=gen).to(torch.int32)
        return leaves, consts

    def op_form(sparse):
        def op(W, w1, bias, x, offsets, keep=None, fwidth=None):
            from recsys_benchmark_amd import _kernels

            emb, yfm = _kernels.gather_fm(x, offsets, W, w1, bias, sparse_W=sparse, sparse_w1=sparse, keep=keep, fwidth=fwidth)
            return dict(emb=emb, yfm=yfm)
        return op

    def ref(W, w1, bias, x, offsets, keep=None, fwidth=None):
        from oracle import reference_ops as ro

        rows = x + offsets.view(1, -1)
        emb = W[rows]
        if keep is not None:
            width = torch.minimum(keep.long()[rows], fwidth.long().view(1, -1).expand_as(rows))
            emb = emb * (torch.arange(D).view(1, 1, D) < width.unsqueeze(-1))
        yfm = ro.fm_second_order(emb).view(-1) + w1[rows].sum(dim=(1, 2)) + bias
        return dict(emb=emb, yfm=yfm)

    def pack(leaves):
        """DeepFM.pack_tables()' layout: W and w1 as column slices of ONE fp32 [N, 32] buffer (a 128-byte line per row)."""
        N = leaves["W"].shape[0]
        buf = torch.zeros((N, 32), dtype=torch.float32, device=DEV)
        buf[:, :D].copy_(leaves["W"])
        buf[:, D:D + 1].copy_(leaves["w1"])
        out = dict(W=buf[:, :D].detach().requires_grad_(True), w1=buf[:, D:D + 1].detach().requires_grad_(True),
                   bias=leaves["bias"].to(DEV).requires_grad_(True))
        assert out["W"].stride(0) == 32 and out["w1"].data_ptr() == out["W"].data_ptr() + 4 * D
        return out

    tag = ("masked" if masked else "plain") + ("-packed128" if packed else "")
    cases = []
    for form in ("dense", "rows", "det"):
        def settings(form=form):
            from recsys_benchmark_amd import _kernels

            return [(_kernels, "DETERMINISTIC", form == "det")]
        cases.append(autograd_case(f"gather_fm-{tag}-{form}-F{F}-D{D}-B{B}", inputs, op_form(form == "rows"), ref,
                                   tol={"emb": (0.0, 0.0)}, default=(2e-5, 2e-5), exact=(lambda k: not k.startswith("d")) if form == "dense" else True,
                                   settings=settings, place=pack if packed else None))
    return cases


# ---- gather_fm_dual (tests/test_dual_deepfm_gpu.py) ----------------------------------------------------------------------------
def _dual_fm_case(F, D, B, kind, geo):
    def forms(td, c):
        out = {}
        for form in ["dense", "det"] + (["coo"] if c["kind"] != "soft" else []):
            with _deterministic(form == "det"):
                r = td._run(c, sparse=form == "coo")
            out.update({f"{form}/{k}": v for k, v in r.items() if v is not None})
        return out

    def run():
        import test_dual_deepfm_gpu as td

        return forms(td, td._case(F, D, B, kind, geo))

    def check(result):
        import test_dual_deepfm_gpu as td

        td._check_case(td._case(F, D, B, kind, geo))

    # the forward, the COO values and the deterministic form have a fixed order; the default dense form adds with float atomics,
    # and so does QR's dense table-1 gradient next to the COO table 2 (mi_dual_gather_bwd_rows joins workgroup partials)
    qr = kind in ("mult", "add")
    return Case(f"gather_fm_dual-{kind}-{geo}-F{F}-D{D}-B{B}", run, check,
                lambda k: not k.startswith("dense/g") and not (qr and k == "coo/gT1"))


# ---- dual_gather (tests/test_embeddings_gpu.py: integer-valued data, exact in any order) -------------------------------------
DG_DIMS = [3, 700, 5, 9, 1201, 31, 32, 64, 2, 4000]


def _qr_ref(idx, T1, T2, divider, op):
    from oracle import reference_ops as ro

    return ro.qr_forward(idx, T1, T2, divider, op)


def _dual_gather_case(op, variant, B=37, D=16, div=2):
    """sparse2 / the small-field hint / the in-kernel offsets, on the field layout of
    test_dual_gather_backward_with_the_small_field_hint_is_the_same_gradient; integer tables and gradients, so the result
    equals the float64 formula (oracle qr_forward) exactly — tolerance 0, as in that test and in
    test_qr_row_form_gradient_of_the_quotient_table_is_the_dense_one."""
    De = D // 2 if op == "cat" else D
    N = sum(DG_DIMS)

    def inputs():
        gen = torch.Generator().manual_seed(5 + len(variant))
        x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in DG_DIMS], 1)
        off = torch.tensor([0] + DG_DIMS[:-1]).cumsum(0)
        T1 = torch.randint(-3, 4, (div, De), generator=gen).float()
        T2 = torch.randint(-3, 4, ((N + div - 1) // div, De), generator=gen).float()
        return dict(T1=T1, T2=T2), dict(x=x, off=off)

    def op_fn(T1, T2, x, off):
        from recsys_benchmark_amd import _kernels

        kw = {}
        if "sparse2" in variant:
            kw["sparse2"] = True
        if "fields" in variant:
            kw["fields"] = _kernels.small_field_hint(DG_DIMS, div, DEV)
        if "offsets" in variant:
            out, rows = _kernels.dual_gather(x, T1, T2, div, div, op, offsets=off, **kw)
            return dict(out=out, rows=rows)
        return dict(out=_kernels.dual_gather(x + off, T1, T2, div, div, op, **kw))

    def ref(T1, T2, x, off):
        out = dict(out=_qr_ref(x + off, T1, T2, div, op))
        if "offsets" in variant:
            out["rows"] = x + off
        return out

    return autograd_case(f"dual_gather-{op}-{variant}-D{D}-div{div}", inputs, op_fn, ref, exact=True, int_grads=True)


ALIGN_OFFSETS = {}          # case name -> data_ptr() % 16 of the upstream gradient the last run handed to DualGather.backward


def _alignment_case(n1, De=16, n=333, aligned=False):
    """dual_gather(sparse2=True) with an upstream gradient that is a contiguous view 12 bytes past a 16-byte boundary: the loss
    runs through cat([pad3, out.reshape(-1)]), whose backward hands `out` a narrow view of one flat gradient.  The float4
    kernel that OVERWRITES table 1's gradient declines such an operand, and the fallback ADDS into it.
    aligned: the twin whose loss is taken from `out` directly, so the float4 kernel runs.  n1 = 3 is the shape whose 48
    sums do not tile a workgroup: the float4 kernel joins them with float atomics and ADDS into table 1's gradient — the
    third form mi_dual_gather_bwd_rows_form can name (n1 in 1, 2, 4 aligned is the dual_gather-*-sparse2 cases)."""
    name = f"dual_gather-{'aligned' if aligned else 'alignment'}-n1_{n1}"
    N = 1000

    def inputs():
        gen = torch.Generator().manual_seed(40 + n1)
        idx = torch.randint(0, N, (n,), generator=gen)
        T1 = torch.randint(-3, 4, (n1, De), generator=gen).float()
        T2 = torch.randint(-3, 4, ((N + n1 - 1) // n1, De), generator=gen).float()
        return dict(T1=T1, T2=T2, **({} if aligned else dict(pad3=torch.zeros(3)))), dict(idx=idx)

    def op_fn(T1, T2, idx, pad3=None):
        from recsys_benchmark_amd import _kernels

        out = _kernels.dual_gather(idx, T1, T2, n1, n1, "add", sparse2=True)
        out.register_hook(lambda g: ALIGN_OFFSETS.__setitem__(name, (g.data_ptr() % 16, g.is_contiguous())))
        return dict(flat=out if aligned else torch.cat([pad3, out.reshape(-1)]))

    def ref(T1, T2, idx, pad3=None):
        out = _qr_ref(idx, T1, T2, n1, "add")
        return dict(flat=out if aligned else torch.cat([pad3, out.reshape(-1)]))

    return autograd_case(name, inputs, op_fn, ref, exact=True, int_grads=True)


# ---- dual_table (tests/test_cerp_cf_gpu.py) -----------------------------------------------------------------------------------
def _dual_table_case(kind, op, divider, N, D, bucket):
    """Integer inputs where the family is exact on them (test_table_backward_is_exact_on_integer_inputs: equality with the
    float64 restatement), random ones otherwise (the ordered-sum bound of
    test_table_backward_within_the_ordered_sum_bound_and_bit_equal_run_to_run); the forward at that file's 1e-5 / 1e-6."""
    integers = kind != "soft"

    def operands():
        import test_cerp_cf_gpu as tc

        gen = torch.Generator().manual_seed(7 * N + D)
        kw = tc.family_case(kind, op, divider, N, D, bucket, gen, integers=integers)
        W = 2 * D if op == "cat" else D
        g = torch.randint(-3, 4, (N, W), generator=gen).float() if integers else torch.randn(N, W, generator=gen)
        return kw, g

    def run():
        import test_cerp_cf_gpu as tc

        kw, g = operands()
        kwd = tc.on_dev(kw, grad=True)
        out = tc.table_of(kwd, N)
        out.backward(g.to(DEV))
        return dict(out=out.detach(), gT1=kwd["T1"].grad, gT2=kwd["T2"].grad, gS1=kwd["S1"].grad if "S1" in kwd else None,
                    gS2=kwd["S2"].grad if "S2" in kwd else None)

    cache = {}

    def check(result):
        from cerp_cf_helpers import dual_table_bwd_ref64, dual_table_ref64
        from conftest import EPS32, assert_close

        kw, g = operands()
        if "ref" not in cache:
            cache["ref"] = (dual_table_ref64(N=N, **kw), dual_table_bwd_ref64(g, N=N, **kw))
        fwd, ref = cache["ref"]
        assert_close(result["out"], fwd.float(), 1e-5, 1e-6, "float64 restatement")
        for key, n in (("gT1", ref["n1"]), ("gT2", ref["n2"]), ("gS1", ref["n1"]), ("gS2", ref["n2"])):
            if key not in result:
                assert key.startswith("gS") and kind != "soft"
                continue
            if integers:
                assert torch.equal(result[key].cpu(), ref[key].float()), key
            else:
                bound = (n.double().unsqueeze(1) + 4) * EPS32 * ref["abs_" + key[1:]] + 1e-30
                err = (result[key].cpu().double() - ref[key]).abs()
                assert bool((err <= bound).all()), f"{key}: {float((err / bound).max()):.3g} x the bound"

    return Case(f"dual_table-{kind}-{op}-{divider}-N{N}-D{D}", run, check, True)      # (no atomics: a fixed order)


# ---- GEMMs (tests/test_gemm_gpu.py) -------------------------------------------------------------------------------------------
GEMM_SHAPES = [(33, 5, 7), (100, 70, 45), (7, 130, 1), (130, 416, 400)]
TRANSPOSES = [(False, False), (False, True), (True, False), (True, True)]


def _gemm_operands(M, N, K, tA, tB):
    gen = torch.Generator().manual_seed(M * 7 + N + K)
    mk = lambda *s: torch.randint(-3, 4, s, generator=gen).float()          # noqa: E731
    A, B = mk(*((K, M) if tA else (M, K))), mk(*((N, K) if tB else (K, N)))
    return A, B, (A.t() if tA else A).double() @ (B.t() if tB else B).double()


def _gemm_case(M, N, K, tA, tB, form):
    """test_layouts_exact_integers: integer-valued operands, so the product is exact and equals the float64 one.  The output is
    allocated with torch.empty — under poison it starts as NaN, and a split-K launch (atomic slices) has to zero it."""
    def run():
        from recsys_benchmark_amd import _kernels

        A, B, _ = _gemm_operands(M, N, K, tA, tB)
        Ad, Bd = A.to(DEV), B.to(DEV)
        if form in ("one", "splitk"):
            # (an explicit split count leaves the zero fill to the caller: gemm() zeroes only where it chose the split itself)
            C = torch.empty(M, N, device=DEV) if form == "one" else torch.zeros(M, N, device=DEV)
            _kernels.gemm(Ad, Bd, C, M, N, K, A.shape[1], B.shape[1], N, tA, tB, splitk=1 if form == "one" else min(4, -(-K // 32)))
        elif form in ("multi", "multi-splitk"):
            # (a problem's C must be zero unless splitk == 1: gemm_multi's contract)
            C = torch.empty(M, N, device=DEV) if form == "multi" else torch.zeros(M, N, device=DEV)
            _kernels.gemm_multi([dict(A=Ad, B=Bd, C=C, M=M, N=N, K=K, lda=A.shape[1], ldb=B.shape[1], ldc=N,
                                      splitk=1 if form == "multi" else 0)], tA, tB)
        else:
            raise ValueError(form)
        return dict(C=C)

    def check(result):
        assert torch.equal(result["C"].cpu().double(), _gemm_operands(M, N, K, tA, tB)[2]), "integer-valued GEMM must be exact"

    return Case(f"gemm-{form}-{M}x{N}x{K}-{'T' if tA else 'N'}{'T' if tB else 'N'}", run, check, True)


def _gemm_panel_case(M, N, K, layout):
    """test_panel_gemm_layouts_groups_and_epilogues' plain product: b_layout 0 = B as [N, K] rows, 1 = [K, N]; a shape the panel
    kernel declines launches nothing and returns False (nothing is then read)."""
    def operands():
        gen = torch.Generator().manual_seed(M + N + K + layout)
        A = torch.randint(-3, 4, (M, K), generator=gen).float()
        B = torch.randint(-3, 4, (N, K) if layout == 0 else (K, N), generator=gen).float()
        return A, B, A.double() @ (B.t() if layout == 0 else B).double()

    def run():
        from recsys_benchmark_amd import _kernels

        A, B, _ = operands()
        C = torch.empty(M, N, device=DEV)
        took = _kernels.gemm_panel(A.to(DEV), K, B.to(DEV), B.shape[1], layout, C, N, M, N, K)
        return dict(C=C) if took else dict(declined=torch.ones(1))

    def check(result):
        covered = M > 0 and N % 4 == 0 and K % 4 == 0
        assert ("C" in result) == covered
        if covered:
            assert torch.equal(result["C"].cpu().double(), operands()[2])

    return Case(f"gemm_panel-{M}x{N}x{K}-layout{layout}", run, check, True)


def _gemm_epilogue_case(splitk):
    """test_random_fp32_and_epilogues, expression for expression and tolerance for tolerance (the CPU float32 product is that
    test's reference), every output allocated with torch.empty."""
    def operands():
        gen = torch.Generator().manual_seed(0)
        M, N, K = 200, 96, 80
        t = dict(A=torch.randn(M, K, generator=gen), W=torch.randn(N, K, generator=gen), b=torch.randn(N, generator=gen),
                 R1=torch.randn(M, N, generator=gen), R2=torch.randn(M, N, generator=gen))
        t["rs"] = torch.randn(M, 3, generator=gen)
        return t, (M, N, K)

    def run():
        from recsys_benchmark_amd import _kernels

        t, (M, N, K) = operands()
        d = {k: v.to(DEV) for k, v in t.items()}
        kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, transB=True)
        new = lambda: torch.empty(M, N, device=DEV)          # noqa: E731
        out = {}
        out["none"] = _kernels.gemm(d["A"], d["W"], new() if splitk == 1 else torch.zeros(M, N, device=DEV), splitk=splitk, **kw)
        out["bias"] = _kernels.gemm(d["A"], d["W"], new(), epi="bias", bias=d["b"], **kw)
        out["tanh"] = _kernels.gemm(d["A"], d["W"], new(), epi="tanh", **kw)
        out["cross2"] = new()
        out["cross"] = _kernels.gemm(d["A"], d["W"], new(), epi="cross", bias=d["b"], R1=d["R1"], ldr1=N, R2=d["R2"], ldr2=N,
                                     C2=out["cross2"], ldc2=N, **kw)
        out["cross_rs"] = _kernels.gemm(d["A"], d["W"], new(), epi="cross", bias=d["b"], R1=d["R1"], ldr1=N, R2=d["R2"], ldr2=N,
                                        rowscale=d["rs"], nrs=3, **kw)
        out["add"] = _kernels.gemm(d["A"], d["W"], new(), epi="add", R1=d["R1"], ldr1=N, **kw)
        H = torch.tanh(d["R1"])
        out["mul_dtanh"] = _kernels.gemm(d["A"], d["W"], new(), epi="mul_dtanh", R1=H, ldr1=N, **kw)
        out["accum"] = _kernels.gemm(d["A"], d["W"], d["R1"].clone(), epi="accum", splitk=splitk, **kw)
        return out

    def check(result):
        from conftest import assert_close

        t, _ = operands()
        acc, b, R1, R2, rs = t["A"] @ t["W"].t(), t["b"], t["R1"], t["R2"], t["rs"]
        H = torch.tanh(R1)
        want = dict(none=(acc, 1e-4), bias=(acc + b, 1e-4), tanh=(torch.tanh(acc), 1e-5), cross=(R1 + R2 * (acc + b), 1e-4),
                    cross2=(acc + b, 1e-4), cross_rs=(R1 + R2 * (acc + b[None] * rs.sum(1, keepdim=True)), 1e-4),
                    add=(R1 + acc, 1e-4), mul_dtanh=(acc * (1 - H * H), 1e-4), accum=(R1 + acc, 1e-4))
        assert set(want) == set(result)
        for k, (w, atol) in want.items():
            assert_close(result[k], w, 1e-5, atol, k)

    # (split-K slices meet in float atomics: "none" and "accum" have no fixed order then)
    return Case(f"gemm-epilogues-splitk{splitk}", run, check, lambda k: splitk == 1 or k not in ("none", "accum"))


# ---- losses (tests/test_lightgcn_step_gpu.py, tests/test_cerp_cf_gpu.py, tests/test_dual_deepfm_gpu.py) ------------------------
LOSS_BATCHES = [1, 37, 1030]
LOSS_WIDTHS = [7, 16]


def _armed_settings(armed):
    def settings():
        from recsys_benchmark_amd import losses

        return [(losses, "ARMED_WORKSPACES", armed)]
    return settings


def _twice_when_armed(case, armed, warm):
    """With the kept workspaces on, the run that is checked is the SECOND of two in a row on different inputs: the first
    (`warm`) creates the kept workspace under poison and leaves its ticket for the second."""
    if not armed:
        return case
    inner = case._run

    def run():
        from recsys_benchmark_amd import losses

        with _patched((losses, "ARMED_WORKSPACES", True)):
            warm()
        return inner()

    case._run = run
    return case


def _loss_tables(B, D, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    nu, ni = 30, 50
    return dict(U=torch.randn(nu, D, generator=gen) * scale, I=torch.randn(ni, D, generator=gen) * scale), \
        dict(users=torch.randint(0, nu, (B,), generator=gen), pos=torch.randint(0, ni, (B,), generator=gen),
             neg=torch.randint(0, ni, (B,), generator=gen))


def _loss_cases(B, D, armed):
    from oracle import reference_ops as ro

    tag = f"B{B}-D{D}-{'armed' if armed else 'fresh'}"
    st = _armed_settings(armed)
    cases = []

    def losses_mod():
        from recsys_benchmark_amd import losses
        return losses

    def upd(seed):
        gen = torch.Generator().manual_seed(seed)
        return {k: torch.randn(B, D, generator=gen) for k in "upn"}, {}

    # bpr_loss: test_bpr_loss_matches_reference (loss 1e-5 / 1e-6, gradients 1e-5 / 1e-7)
    c = autograd_case(f"bpr_loss-{tag}", lambda: upd(B + D), lambda u, p, n: dict(loss=losses_mod().bpr_loss(u, p, n) * 1.7),
                      lambda u, p, n: dict(loss=ro.bpr_loss(u, p, n) * 1.7), tol=dict(loss=(1e-5, 1e-6)), default=(1e-5, 1e-7),
                      exact=True, settings=st)
    cases.append(_twice_when_armed(c, armed, lambda: losses_mod().bpr_loss(*[t.to(DEV) for t in upd(1)[0].values()])))

    # bpr_loss_multi: test_info_nce_and_multi_bpr_match_the_reference_vectors (loss 1e-5 / 1e-6, gradients 1e-4 / 1e-6)
    def multi(seed):
        gen = torch.Generator().manual_seed(seed)
        return dict(u=torch.randn(B, D, generator=gen), p=torch.randn(B, D, generator=gen), n=torch.randn(B, 3, D, generator=gen)), {}
    # (the repeated user / positive rows are summed with float atomics)
    c = autograd_case(f"bpr_loss_multi-{tag}", lambda: multi(B + D), lambda u, p, n: dict(loss=losses_mod().bpr_loss_multi(u, p, n)),
                      lambda u, p, n: dict(loss=ro.bpr_loss_multi(u, p, n)), tol=dict(loss=(1e-5, 1e-6)), default=(1e-4, 1e-6),
                      exact=lambda k: k in ("loss", "dn"), settings=st)
    cases.append(_twice_when_armed(c, armed, lambda: losses_mod().bpr_loss_multi(*[t.to(DEV) for t in multi(2)[0].values()])))

    # bpr_loss_rows: test_bpr_loss_rows_equals_index_select_path (loss 1e-5 / 1e-6, table gradients 1e-4 / 1e-7: float atomics)
    def rows_ref(U, I, users, pos, neg):
        return dict(loss=ro.bpr_loss(U[users], I[pos], I[neg]))
    c = autograd_case(f"bpr_loss_rows-{tag}", lambda: _loss_tables(B, D, 3 + B + D),
                      lambda U, I, users, pos, neg: dict(loss=losses_mod().bpr_loss_rows(U, I, users, pos, neg)), rows_ref,
                      tol=dict(loss=(1e-5, 1e-6)), default=(1e-4, 1e-7), exact=lambda k: k == "loss", settings=st)
    cases.append(_twice_when_armed(c, armed, lambda: losses_mod().bpr_loss_rows(*[t.to(DEV) for d in _loss_tables(B, D, 4) for t in d.values()])))

    # reg_loss_rows (rowsq): test_reg_loss_rows_matches_float64_at_every_width (1e-5 / 1e-5, gradients 1e-4 / 1e-7)
    def reg_ref(U, I, users, pos, neg):
        return dict(loss=(U[users].pow(2).sum() + I[pos].pow(2).sum() + I[neg].pow(2).sum()) / (2 * users.numel()) * 3.0)
    c = autograd_case(f"reg_loss_rows-{tag}", lambda: _loss_tables(B, D, 11 + B + D),
                      lambda U, I, users, pos, neg: dict(loss=losses_mod().reg_loss_rows(U, I, users, pos, neg) * 3.0), reg_ref,
                      tol=dict(loss=(1e-5, 1e-5)), default=(1e-4, 1e-7), exact=lambda k: k == "loss", settings=st)
    cases.append(_twice_when_armed(c, armed, lambda: losses_mod().reg_loss_rows(*[t.to(DEV) for d in _loss_tables(B, D, 5) for t in d.values()])))

    # reg_prune_loss_rows: test_batch_row_terms_match_float64_on_heavily_repeated_ids (LOSS_TOL 1e-5 / 1e-6, GRAD_TOL 1e-4 / 1e-6)
    def rp_op(U, I, users, pos, neg):
        reg, prune = losses_mod().reg_prune_loss_rows(U, I, users, pos, neg)
        return dict(reg=reg, prune=prune)

    def rp_ref(U, I, users, pos, neg):
        emb = torch.cat([U[torch.unique(users)], I[pos], I[neg]])
        return dict(reg=(U[users].pow(2).sum() + I[pos].pow(2).sum() + I[neg].pow(2).sum()) / (2 * users.numel()),
                    prune=-torch.tanh(emb * 100).norm(2) ** 2)
    c = autograd_case(f"reg_prune-{tag}", lambda: _loss_tables(B, D, 13 + B + D, scale=0.01), rp_op, rp_ref,
                      tol=dict(reg=(1e-5, 1e-6), prune=(1e-5, 1e-6)), default=(1e-4, 1e-6), exact=lambda k: k in ("reg", "prune"),
                      settings=st)
    cases.append(_twice_when_armed(c, armed, lambda: losses_mod().reg_prune_loss_rows(
        *[t.to(DEV) for d in _loss_tables(B, D, 6, scale=0.01) for t in d.values()])))
    return cases


def _info_nce_cases(n, D, armed):
    """test_info_nce_matches_oracle / test_masked_info_nce_equals_info_nce_of_the_selected_rows: loss 1e-5 / 1e-5, gradients
    1e-4 / 1e-6 / max(1, n / 100).  info_nce takes a fresh workspace per call whatever ARMED_WORKSPACES says."""
    from oracle import reference_ops as ro

    st = _armed_settings(armed)
    tag = f"n{n}-D{D}-{'armed' if armed else 'fresh'}"
    gtol = (1e-4, 1e-6 / max(1.0, n / 100))
    # the gradient products reduce over n: from 16 K-steps of 32 on, gemm() splits K over workgroups that meet in float atomics
    fixed = (lambda k: k == "loss") if -(-n // 32) >= 16 else True

    def two(seed=None):
        gen = torch.Generator().manual_seed(n + D)
        return dict(v1=torch.randn(n, D, generator=gen), v2=torch.randn(n, D, generator=gen)), {}

    def masked():
        gen = torch.Generator().manual_seed(n)
        m = torch.rand(n, generator=gen) < 0.7
        m[0] = True
        return dict(v=torch.randn(n, D, generator=gen)), dict(m=m)

    def losses_mod():
        from recsys_benchmark_amd import losses
        return losses

    def masked_ref(v, m):
        sel = v[m]
        return dict(loss=ro.info_nce(sel, sel, 0.2))

    return [autograd_case(f"info_nce-{tag}", two, lambda v1, v2: dict(loss=losses_mod().info_nce(v1, v2, 0.2, True) * 0.5),
                          lambda v1, v2: dict(loss=ro.info_nce(v1, v2, 0.2, True) * 0.5), tol=dict(loss=(1e-5, 1e-5)), default=gtol,
                          exact=fixed, settings=st),
            autograd_case(f"info_nce-valid-{tag}", masked, lambda v, m: dict(loss=losses_mod().info_nce(v, v, 0.2, valid=m)),
                          masked_ref, tol=dict(loss=(1e-5, 1e-5)), default=gtol, exact=fixed, settings=st)]


def _cerp_prune_case(n, D, K, armed):
    """test_prune_loss_is_as_close_to_float64_as_the_stock_float32_expression, its bound per tensor:
    max|new - ref64| <= 2 max|stock32 - ref64| + 4 eps32 max|ref64|."""
    def run():
        import test_dual_deepfm_gpu as td
        from recsys_benchmark_amd import _kernels, losses

        with _patched((losses, "ARMED_WORKSPACES", armed)):
            if armed:          # the kept workspace is created by a first call on other tables
                warm = [t.to(DEV) for t in td._prune_tables(n, D, torch.Generator().manual_seed(1))]
                _kernels.cerp_prune_loss(*warm, K)
            leaves = [t.to(DEV).requires_grad_(True) for t in td._prune_tables(n, D, torch.Generator().manual_seed(n + D))]
            loss = _kernels.cerp_prune_loss(*leaves, K)
            loss.backward()
        return dict(loss=loss.detach(), gP=leaves[0].grad, gSp=leaves[1].grad, gQ=leaves[2].grad, gSq=leaves[3].grad)

    cache = {}

    def check(result):
        import test_dual_deepfm_gpu as td
        from conftest import EPS32

        if "ref" not in cache:
            tables = td._prune_tables(n, D, torch.Generator().manual_seed(n + D))
            cache["ref"] = (td._stock(tables, K, torch.float32), td._stock(tables, K, torch.float64))
        (loss32, g32), (loss64, g64) = cache["ref"]
        for name, s32, r64 in [("loss", loss32, loss64)] + list(zip(("gP", "gSp", "gQ", "gSq"), g32, g64)):
            r64, s32 = r64.double().cpu(), s32.double().cpu()
            err_new = float((result[name].double().cpu() - r64).abs().max())
            bound = 2 * float((s32 - r64).abs().max()) + 4 * EPS32 * float(r64.abs().max())
            assert err_new <= bound, f"{name}: |new - ref64| {err_new:.3e} > {bound:.3e}"

    return Case(f"cerp_prune_loss-n{n}-D{D}-K{K}-{'armed' if armed else 'fresh'}", run, check, True)


# ---- propagation on the dyadic fixture (tests/hccf_helpers.py: exact in float32 in any summation order) ----------------------
PROP_WIDTHS = [4, 6, 64]
PROP_LAYERS = [1, 3]


def _hccf_case(D, L, slope=0.5):
    def run():
        import test_hccf_gpu as th

        fx, _want = th._dyadic(D, L, slope)
        ue, ie, du, di = th._run(fx, slope, L)
        return dict(user_emb=ue, item_emb=ie, dXu=du, dXi=di)

    def check(result):
        import test_hccf_gpu as th

        _fx, want = th._dyadic(D, L, slope)
        th._check((result["user_emb"], result["item_emb"], result["dXu"], result["dXi"]), want, L, f"D={D} L={L}")

    return Case(f"hccf_propagate-D{D}-L{L}", run, check, True)


@functools.lru_cache(maxsize=None)
def _dyadic_square(D):
    """The fixture's graph as LightGCN's square CSR operand (test_lightgcn_gpu._dyadic_product's construction), the dense float64
    block matrix beside it."""
    import hccf_helpers as hh

    fx = hh.dyadic_fixture(D, 1)
    U, ii, v = fx["U"], fx["idx"], fx["vals"][0]
    A = hh.block_adjacency(ii, v, U, fx["I"])
    ind = torch.cat([torch.stack([ii[0], ii[1] + U]), torch.stack([ii[1] + U, ii[0]])], 1)
    adj = torch.sparse_coo_tensor(ind, torch.cat([v, v]), A.shape).coalesce().to_sparse_csr()
    return fx, adj, A


def _lightgcn_ref(A, S, L):
    acc, cur = S, S
    for _ in range(L):
        cur = A @ cur
        acc = acc + cur
    return acc / (L + 1)


def _dyadic_claim(D, L, masked_rows=None):
    """The inputs are exact in float32 for the LightGCN layer mean too (asserted, the way hccf_helpers.assert_dyadic_exact
    checks its own claim): float32 in two summation orders equals float64, forward and backward."""
    fx, _adj, A = _dyadic_square(D)
    S, g = torch.cat([fx["Xu"], fx["Xi"]]).double(), torch.cat([fx["gu"], fx["gi"]]).double()
    for x in (S, g):
        want = _lightgcn_ref(A, x, L)
        assert torch.equal(_lightgcn_ref(A.float(), x.float(), L).double(), want), "the dyadic fixture is not exact for this L"
    return True


def _lightgcn_case(D, L, form):
    """lightgcn_propagate on the dyadic graph: row-per-wave and tiled kernels, the masked first backward layer (the fixture's
    gradient is zero on three quarters of the rows) switched on and off.  Exact: equality with the dense float64 product, as
    test_every_float4_width_with_a_hub_row_is_exact holds the one-layer product to."""
    def settings():
        from recsys_benchmark_amd import _kernels

        return [(_kernels, "TILED_SPMM", form == "tiled"), (_kernels, "MASK_FIRST_BACKWARD_LAYER", form != "unmasked"),
                (_kernels, "SLICED_SPMM", 0)]

    def both(fn, to):
        fx, _adj, _A = _dyadic_square(D)
        Xu, Xi = to(fx["Xu"]).requires_grad_(True), to(fx["Xi"]).requires_grad_(True)
        ou, oi = fn(Xu, Xi)
        torch.autograd.backward([ou, oi], [to(fx["gu"]), to(fx["gi"])])
        return dict(user_emb=ou.detach(), item_emb=oi.detach(), dXu=Xu.grad, dXi=Xi.grad)

    def run():
        from recsys_benchmark_amd import _kernels

        adj = _dyadic_square(D)[1].to(DEV)
        with _patched(*settings()):
            return both(lambda Xu, Xi: _kernels.lightgcn_propagate(adj, Xu, Xi, L), lambda t: t.to(DEV))

    cache = {}

    def check(result):
        if "ref" not in cache:
            assert _dyadic_claim(D, L)
            A = _dyadic_square(D)[2]

            def ref(Xu, Xi):
                out = _lightgcn_ref(A, torch.cat([Xu, Xi]), L)
                return out[:Xu.shape[0]], out[Xu.shape[0]:]
            cache["ref"] = both(ref, lambda t: t.double())
        for k, want in cache["ref"].items():
            got = result[k].cpu().double()
            assert torch.equal(got, want), f"{k}: max diff {float((got - want).abs().max()):.3e}"

    return Case(f"lightgcn_propagate-{form}-D{D}-L{L}", run, check, True)


def _spmm_case(D):
    """spmm over the fixture's rectangular U x I matrix, forward and backward: exact (one layer of the same sums)."""
    def inputs():
        import hccf_helpers as hh

        fx = hh.dyadic_fixture(D, 1)
        M = torch.sparse_coo_tensor(fx["idx"], fx["vals"][0], (fx["U"], fx["I"])).coalesce().to_sparse_csr()
        return dict(X=fx["Xi"]), dict(M=M)

    def op(X, M):
        from recsys_benchmark_amd import _kernels

        _kernels._plans.clear()
        return dict(Y=_kernels.spmm(M, X))

    def ref(X, M):
        return dict(Y=M.to_dense().double() @ X)

    return autograd_case(f"spmm-D{D}", inputs, op, ref, exact=True, int_grads=True)


# ---- optimizers (tests/test_optim_gpu.py) -------------------------------------------------------------------------------------
def _sparse_adam_case(N, D, n, capturable):
    """test_sparse_adam_matches_torch against torch.optim.SparseAdam on the CPU: param and exp_avg 1e-4 / 1e-5, exp_avg_sq
    1e-4 / 1e-6; two steps.  The step sums duplicates in a fixed order (test_sparse_adam_is_deterministic...): bit-equal runs."""
    def steps(dev, opt_cls, **kw):
        gen = torch.Generator().manual_seed(N + D)
        p = torch.nn.Parameter(torch.randn(N, D, generator=gen).to(dev))
        opt = opt_cls([p], lr=0.01, **kw)
        for _ in range(2):
            rows = (N * torch.rand(n, generator=gen).pow(3)).long().clamp_(max=N - 1)
            vals = torch.randn(n, D, generator=gen)
            p.grad = torch.sparse_coo_tensor(rows.view(1, -1).to(dev), vals.to(dev), (N, D), check_invariants=False)
            opt.step()
        st = opt.state[p]
        return dict(param=p.detach(), exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"],
                    step=torch.as_tensor(float(st["step"])))

    def run():
        from recsys_benchmark_amd.optim import SparseAdam

        return steps(DEV, SparseAdam, capturable=capturable)

    cache = {}

    def check(result):
        if "ref" not in cache:
            cache["ref"] = steps("cpu", torch.optim.SparseAdam)
        _cmp(result, cache["ref"], dict(exp_avg_sq=(1e-4, 1e-6), step=(0.0, 0.0)), (1e-4, 1e-5))

    return Case(f"sparse_adam-N{N}-D{D}-n{n}-{'capturable' if capturable else 'host'}", run, check, True)


def _dense_adam_case(weight_decay):
    """test_dense_adam_matches_torch_adam's odd-sized tensor list: param 2e-6 / 1e-7, exp_avg_sq 2e-6 / 1e-12."""
    shapes = [(1,), (5,), (4096,), (4097,), (400, 416), (16, 3, 7), (100003,)] + [(33,)] * 20

    def steps(dev, opt_cls):
        gen = torch.Generator().manual_seed(4)
        ps = [torch.nn.Parameter(torch.randn(*sh, generator=gen).to(dev)) for sh in shapes]
        opt = opt_cls(ps, lr=1e-2, weight_decay=weight_decay)
        for step in range(2):
            for p in ps:
                p.grad = (torch.randn(p.shape, generator=gen) * (10.0 ** (step - 1))).to(dev)
            opt.step()
        out = {}
        for i, p in enumerate(ps):
            out[f"param{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
        return out

    def run():
        from recsys_benchmark_amd.optim import Adam

        return steps(DEV, Adam)

    cache = {}

    def check(result):
        if "ref" not in cache:
            cache["ref"] = steps("cpu", torch.optim.Adam)
        _cmp(result, cache["ref"], {f"exp_avg_sq{i}": (2e-6, 1e-12) for i in range(len(shapes))}, (2e-6, 1e-7))

    return Case(f"dense_adam-wd{weight_decay}", run, check, True)


def _coalesce_case(N, D, n):
    """coalesce_dense against index_add on integer-valued rows: exact (the existing callers' tests compare it bit for bit)."""
    def operands():
        gen = torch.Generator().manual_seed(N + n)
        return torch.randint(0, N, (n,), generator=gen), torch.randint(-3, 4, (n, D), generator=gen).float()

    def run():
        from recsys_benchmark_amd import _kernels

        rows, vals = operands()
        return dict(out=_kernels.coalesce_dense(rows.to(DEV), vals.to(DEV), N, D))

    def check(result):
        rows, vals = operands()
        assert torch.equal(result["out"].cpu().double(), torch.zeros(N, D, dtype=torch.float64).index_add_(0, rows, vals.double()))

    return Case(f"coalesce_dense-N{N}-D{D}-n{n}", run, check, True)


# ---- the fused MLP tail (tests/test_tail_gpu.py, tests/test_tail_exact_cover_gpu.py) ------------------------------------------
TAIL_CASES = [(67, 48, [136], 0.25), (67, 48, [24], 0.25), (130, 48, [200], 0.25), (130, 48, [104], 0.25), (67, 40, [24], 0.25),
              (67, 16, [24], 0.25), (200, 48, [40, 72], 0.5), (67, 16, [8], 0.25)]
TAIL_MODES = ["bn-train", "bn-eval", "nobn-train", "nobn-eval"]


def _tail_case(M, K, hidden, p, mode, fused, stat="finalize"):
    """run_tail on a (Linear, BatchNorm1d, ReLU, Dropout) x k + Linear(., 1) stack with FUSED_TAIL on (STAT_SUMS off: tile
    statistics joined in a fixed order, no atomics) and off (the general path, without dropout as in its own test).  The
    reference comparison is test_fused_tail_brackets_float64_like_the_stock_modules itself, run under the same settings
    (fused form); the general path is held to tests/test_mlp_gpu.py's test_tail_matches_stock_modules_on_the_same_gemms:
    the output against the CPU evaluation (here float64) at 2e-4 / 2e-4, the gradients mostly close at that test's rates."""
    training = mode.endswith("train")
    if not fused:
        p = 0.0

    def settings():
        from recsys_benchmark_amd import mlp, tail

        return [(mlp, "FUSED_TAIL", fused), (tail, "STAT_SUMS", stat == "sums"), (tail, "MERGE_JOINS", stat == "joins")]

    def build():
        import test_tail_gpu as tt

        torch.manual_seed(M + K + len(hidden))
        seq = tt._seq(K, hidden, p, bn=mode.startswith("bn")).train(training)
        return seq, torch.randn(M, K) * 0.7 + 0.2, torch.randn(M), torch.randn(M, 1)

    def run():
        from recsys_benchmark_amd import mlp
        from recsys_benchmark_amd.mlp import run_tail

        seq, x, add, G = build()
        with _patched(*settings()):
            mlp._seed_word(torch.device(DEV, 0)).fill_(4242 + M)
            fs = copy.deepcopy(seq).to(DEV)
            xd, ad = x.to(DEV).requires_grad_(True), add.to(DEV).requires_grad_(True)
            out = run_tail(fs, xd, last_add=ad)
            (out * G.to(DEV)).sum().backward()
        res = dict(out=out.detach(), dx=xd.grad, dadd=ad.grad)
        res.update({"g/" + k: v.grad for k, v in fs.named_parameters()})
        res.update({"b/" + k: v.detach() for k, v in fs.named_buffers()})
        return res

    cache = {}

    def check(result):
        import test_tail_gpu as tt

        if fused:
            with _patched(*settings()) as mp:
                tt.test_fused_tail_brackets_float64_like_the_stock_modules(M, K, hidden, p, mode, mp)
            return
        from conftest import assert_close, assert_mostly_close

        if "ref" not in cache:
            seq, x, add, G = build()
            rs, rx, ra, rout = tt._reference(seq, x, add, [torch.ones(())] * len(hidden), torch.float64)
            (rout * G.double()).sum().backward()
            cache["ref"] = (rs, rx, ra, rout)
        rs, rx, ra, rout = cache["ref"]
        assert_close(result["out"], rout.float(), 2e-4, 2e-4, "output vs CPU")
        scale = float(rx.grad.abs().max()) + 1e-6
        assert_mostly_close(result["dx"], rx.grad.float(), 1e-3, 1e-4 * scale, 2e-3, "grad input")
        assert_mostly_close(result["dadd"], ra.grad.float(), 1e-3, 1e-4, 2e-3, "grad last_add")
        for k, q in rs.named_parameters():
            s = max(float(q.grad.abs().max()), 1e-2)
            assert_mostly_close(result["g/" + k], q.grad.float(), 2e-3, 1e-3 * s, 3e-2, f"grad {k}")
        for k, c in rs.named_buffers():
            assert_close(result["b/" + k], c.to(result["b/" + k].dtype), 1e-5, 1e-6, f"buffer {k}")

    # (the three forms of the BatchNorm statistics of tests/test_tail_gpu.py: tile statistics with finalize launches — a fixed
    #  order —, shifted sums added with float atomics, tile statistics joined in the consumer's prologue)
    return Case(f"tail-{'fused-' + stat if fused else 'general'}-{mode}-M{M}-K{K}-h{'x'.join(map(str, hidden)) or 'none'}", run, check,
                # (the general path's batch statistics are column sums added with float atomics, csrc/mlp.hip; with fixed
                #  statistics or none its forward has a fixed order)
                (lambda k: stat == "finalize") if fused else (lambda k: k == "out" and mode != "bn-train"))


def _deepfm_case(labels, fused, stat="finalize", upstream="unit", packed=False):
    """One DeepFM training step through pkg.DeepFM, with and without the criterion inside the tail's head launch
    (labels=): __graft_entry__.smoke()'s shapes, float64 oracle (reference_ops.deepfm_forward) and tolerances."""
    dims, D, B = [11, 7, 5, 13], 16, 32

    def data():
        gen = torch.Generator().manual_seed(0)
        x = torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1)
        return x, (torch.rand(B, generator=gen) < 0.3).float()

    def model():
        import recsys_benchmark_amd as pkg

        torch.manual_seed(0)
        return pkg.DeepFM(dims, D, [32, 32], p_dropout=0.0, use_batchnorm=True, embedding_config={"name": "vanilla", "sparse": True},
                          fc_sparse=True)

    def settings():
        from recsys_benchmark_amd import mlp, tail

        return [(mlp, "FUSED_TAIL", fused), (tail, "STAT_SUMS", stat == "sums"), (tail, "MERGE_JOINS", False)]

    def run():
        import recsys_benchmark_amd as pkg
        from recsys_benchmark_amd.losses import unit_scalar

        x, y = data()
        m = model().to(DEV)
        if packed:
            m.pack_tables()
            assert m.tables_packed
        yd = y.to(DEV)
        with _patched(*settings()):
            logits = m(x.to(DEV), labels=yd) if labels else m(x.to(DEV))
            loss = pkg.BCEWithLogitsLoss()(logits, yd)
            if upstream == "unit":
                loss.backward(unit_scalar(DEV))
            else:          # any other upstream gradient: the head launch's precomputed gradient does not apply
                (loss * 0.37).backward()
        pkg.check_index_errors()
        res = dict(logits=logits.detach(), loss=loss.detach())
        res.update({"g/" + k: v.grad for k, v in m.named_parameters()})
        res.update({"b/" + k: v.detach() for k, v in m.named_buffers()})
        return res

    cache = {}

    def check(result):
        from conftest import assert_close
        from oracle import reference_ops as ro

        if "ref" not in cache:
            x, y = data()
            p = {k: v.detach().clone().double() if v.is_floating_point() else v.detach().clone() for k, v in model().state_dict().items()}
            for k, v in p.items():
                if v.is_floating_point() and "running_" not in k:
                    v.requires_grad_(True)
            ref = ro.deepfm_forward(x, p, 2, True, True)
            ref_loss = torch.nn.BCEWithLogitsLoss()(ref, y.double())
            (ref_loss * (1.0 if upstream == "unit" else 0.37)).backward()
            cache["ref"] = (p, ref.detach(), ref_loss.detach())
        p, ref, ref_loss = cache["ref"]
        assert_close(result["logits"], ref.float(), 1e-4, 1e-5, "logits")
        assert_close(result["loss"], ref_loss.float(), 1e-5, 1e-6, "loss")
        assert_close(dense(result["g/embedding._emb_module.weight"]), p["embedding._emb_module.weight"].grad.float(), 1e-4, 1e-6, "g table")
        assert_close(dense(result["g/fc.weight"]), p["fc.weight"].grad.float(), 1e-4, 1e-6, "g fc")
        for k in result:
            if k.startswith("g/_deep_branch") and k.endswith("weight") and result[k].dim() == 2:
                assert_close(result[k], p[k[2:]].grad.float(), 2e-4, 1e-6, k)

    return Case(f"deepfm-step-{'labels' if labels else 'nolabels'}-{'fused-' + stat if fused else 'general'}-{upstream}"
                f"{'-packed128' if packed else ''}", run, check,
                lambda k: fused and stat == "finalize")


# ---- pruning, CTR metric, quantised gathers ---------------------------------------------------------------------------------------
def _auc_case(n):
    """binary_auc_device against the float64 rank-sum formula (tests/test_ctr_metric_gpu.py holds the record to exact integers
    and the AUC to the double the host forms from them)."""
    def operands():
        gen = torch.Generator().manual_seed(n)
        score = torch.randint(0, 50, (n,), generator=gen).float() / 7            # ties
        label = (torch.rand(n, generator=gen) < 0.4).to(torch.uint8)
        label[0], label[1] = 1, 0
        return score, label

    def run():
        from recsys_benchmark_amd import _kernels

        score, label = operands()
        return dict(record=_kernels.binary_auc_device(score.to(DEV), label.to(DEV)))

    def check(result):
        from recsys_benchmark_amd import _kernels

        score, label = operands()
        rec = _kernels.auc_record(result["record"].cpu())
        s, y = score.double(), label.double()
        pos, neg = s[y == 1], s[y == 0]
        wins = (pos.view(-1, 1) > neg.view(1, -1)).double().sum() + 0.5 * (pos.view(-1, 1) == neg.view(1, -1)).double().sum()
        assert int(rec["P"]) == int(y.sum()) and int(rec["N"]) == n - int(y.sum())
        assert abs(float(rec["auc"]) - float(wins / (pos.numel() * neg.numel()))) <= 1e-12

    return Case(f"binary_auc_device-n{n}", run, check, True)


def _gather_quant_case(qtype, D=7):
    """gather_rows_quant (tests/test_embeddings_gpu.py test_ptq_known_codes: (code - bias) * scale, fp16 -> fp32): exact."""
    N, n = 41, 300

    def operands():
        gen = torch.Generator().manual_seed(D + len(qtype))
        idx = torch.randint(0, N, (n,), generator=gen)
        if qtype == "fp16":
            return idx, torch.randn(N, D, generator=gen).half(), None, None
        dt = torch.int8 if qtype == "int8" else torch.int16
        hi = 127 if qtype == "int8" else 32767
        W = torch.randint(-hi, hi + 1, (N, D), generator=gen).to(dt)
        return idx, W, torch.tensor([0.0123]), torch.tensor([3], dtype=dt)

    def run():
        from recsys_benchmark_amd import _kernels

        idx, W, scale, bias = operands()
        mv = lambda t: None if t is None else t.to(DEV)          # noqa: E731
        return dict(out=_kernels.gather_rows_quant(idx.to(DEV), W.to(DEV), mv(scale), mv(bias)))

    def check(result):
        idx, W, scale, bias = operands()
        want = W[idx].float() if qtype == "fp16" else (W[idx].int() - bias.int()).float() * scale
        assert torch.equal(result["out"].cpu(), want)

    return Case(f"gather_rows_quant-{qtype}-D{D}", run, check, True)


# ---- second batch: module-level families ------------------------------------------------------------------------------------------
def _module_grads(m, prefix="g/"):
    out = {prefix + k: v.grad for k, v in m.named_parameters() if v.grad is not None}
    out.update({"b/" + k: v.detach() for k, v in m.named_buffers()})
    return out


def _mish_case(use_bn, training, n, k, hidden, D):
    """The DHE MLP on mish_mlp.py's kernels; the comparison is test_dhe_mlp_on_own_kernels_vs_float64_all_orderings itself."""
    def run():
        from recsys_benchmark_amd.embeddings.dh_embedding import DHEmbedding

        torch.manual_seed(n + k + use_bn)
        DHEmbedding.COUNTER = 0
        emb = DHEmbedding(n, D, None, k, list(hidden), use_bn=use_bn, cached=False)
        DHEmbedding.COUNTER = 0
        for m in emb._seq:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
        emb._seq.train(training)
        x, G = torch.rand(n, k) * 2 - 1, torch.randn(n, D)
        emb._seq = emb._seq.to(DEV)
        out = emb._forward_mlp(x.to(DEV))
        (out * G.to(DEV)).sum().backward()
        return dict(out=out.detach(), **_module_grads(emb._seq))

    def check(result):
        import test_embeddings_gpu as te

        with _patched() as mp:
            te.test_dhe_mlp_on_own_kernels_vs_float64_all_orderings(use_bn, training, n, k, hidden, D, mp)

    # (csrc/mish_mlp.hip has no atomics: the forward and the running statistics have a fixed order; the weight gradients are
    #  library products that may split K)
    return Case(f"mish_mlp-bn{use_bn}-{'train' if training else 'eval'}-n{n}-k{k}-h{'x'.join(map(str, hidden)) or 'none'}", run, check,
                lambda key: key == "out" or key.startswith("b/"))


def _tt_case(name, N, ranks, ps, qs, shape, rtol_g=1e-3, atol_g=1e-4, D=16):
    """tt_lookup, per-lookup kernels (few lookups) and grouped (>= 4096): tests/test_tt_grouped_gpu.py's _check — forward
    1e-4 / 1e-5, core gradients 1e-3 / 1e-4 against oracle tt_forward (here evaluated in float64)."""
    def build():
        from recsys_benchmark_amd.embeddings import TTRecTorch

        gen = torch.Generator().manual_seed(11)          # (test_tt_grouped_gpu._emb, at any row width)
        emb = TTRecTorch(N, D, ranks, tt_p_shapes=ps, tt_q_shapes=qs, weight_dist="normal")
        with torch.no_grad():
            for c in emb.tt_cores:
                c.copy_(torch.randn(c.shape, generator=gen) * 0.1)
        idx = torch.randint(0, N, shape, generator=gen)
        return emb, idx, torch.randn(idx.numel(), D, generator=gen)

    def run():
        from recsys_benchmark_amd import _lib

        emb, idx, G = build()
        emb.to(DEV)
        out = emb(idx.to(DEV)).reshape(-1, D)
        (out * G.to(DEV)).sum().backward()
        _lib.check_index_errors()
        return dict(out=out.detach(), **{f"g/core{i}": c.grad for i, c in enumerate(emb.tt_cores)})

    cache = {}

    def check(result):
        from oracle import reference_ops as ro

        if "ref" not in cache:
            emb, idx, G = build()
            cores = [c.detach().double().requires_grad_(True) for c in emb.tt_cores]
            ref = ro.tt_forward(idx.flatten(), emb.tt_p_shapes, emb.tt_q_shapes, emb.tt_ranks, cores)
            (ref * G.double()).sum().backward()
            cache["ref"] = dict(out=ref.detach(), **{f"g/core{i}": c.grad for i, c in enumerate(cores)})
        _cmp(result, cache["ref"], dict(out=(1e-4, 1e-5)), (rtol_g, atol_g))

    # (the per-lookup forward has a fixed order; the grouped products and every core gradient join with float atomics)
    return Case(f"tt_lookup-{name}", run, check, lambda key: key == "out" and name.startswith("plain"))


def _qat_case(name):
    """QatEmbedding forward (the recorded draw) and backward against the reference's golden: test_qat_matches_reference_golden."""
    def run():
        from conftest import load_golden
        from recsys_benchmark_amd.embeddings import get_embedding

        g = load_golden(name)
        emb = get_embedding({"name": "qat", "n_bits": int(g["n_bits"])}, g["field_dims"].tolist(), int(g["hidden"]))
        emb.load_state_dict({"_emb_module.weight": g.t("param/_emb_module.weight"), "scale": g.t("param/scale")})
        emb.to(DEV)
        out = emb(g.t("x").to(DEV), prob=g.t("prob").to(DEV))
        (out * g.t("G").to(DEV)).sum().backward()
        return dict(out=out.detach(), gW=emb._emb_module.weight.grad, gscale=emb.scale.grad)

    def check(result):
        from conftest import assert_close, load_golden

        g = load_golden(name)
        assert_close(result["out"], g.t("out"), 0, 0, "rounded rows (same draw): bit-exact")
        assert_close(dense(result["gW"]), g.t("grad/_emb_module.weight"), 1e-6, 1e-7, "row gradient")
        assert_close(result["gscale"], g.t("grad/scale"), 1e-5, 1e-4, "scale gradient")

    return Case(f"qat-{name}", run, check, lambda k: k == "out")


def _csr_rows_case(N=41, D=7):
    """csr_rows against oracle csr_rows (copies of stored values: exact)."""
    def operands():
        gen = torch.Generator().manual_seed(N + D)
        w = torch.randn(N, D, generator=gen)
        w[torch.rand(N, D, generator=gen) < 0.6] = 0.0
        w[::5] = 0.0
        csr = w.to_sparse_csr()
        return w, csr, torch.randint(0, N, (9, 4), generator=gen)

    def run():
        from recsys_benchmark_amd import _kernels

        w, csr, ids = operands()
        return dict(out=_kernels.csr_rows(csr.values().to(DEV), csr.crow_indices().to(DEV), csr.col_indices().to(DEV), ids.to(DEV), D, N))

    def check(result):
        from oracle import reference_ops as ro

        w, csr, ids = operands()
        assert torch.equal(result["out"].cpu(), w[ids])
        assert torch.equal(ro.csr_rows(csr.values(), csr.crow_indices(), csr.col_indices(), ids, D).reshape(9, 4, D), w[ids])

    return Case(f"csr_rows-N{N}-D{D}", run, check, True)


def _simple_gather_cases():
    """gather_rows, fm_first_order, the PEP lookups and the kept-element count on integer-valued tables (every sum an integer
    below 2^24: exact in float32 in any order, tolerance 0) — the PEP soft threshold at tests/test_embeddings_gpu.py's
    test_pep_vs_oracle_large tolerance."""
    from oracle import reference_ops as ro

    N, D, B, F = 53, 8, 37, 5

    def ints(seed):
        gen = torch.Generator().manual_seed(seed)
        return (dict(W=torch.randint(-3, 4, (N, D), generator=gen).float()),
                dict(idx=torch.randint(0, N, (B, F), generator=gen)))

    def kern():
        from recsys_benchmark_amd import _kernels
        return _kernels

    cases = []
    for sparse in (False, True):
        cases.append(autograd_case(f"gather_rows-{'rows' if sparse else 'dense'}", lambda: ints(1),
                                   lambda W, idx, sparse=sparse: dict(out=kern().gather_rows(idx, W, sparse)),
                                   lambda W, idx: dict(out=W[idx]), exact=True, int_grads=True))

    def fm_in():
        lv, cv = ints(2)
        gen = torch.Generator().manual_seed(3)
        return (dict(emb=torch.randint(-3, 4, (B, F, D), generator=gen).float(), w1=torch.randint(-3, 4, (N, 1), generator=gen).float(),
                     bias=torch.tensor([2.0])), dict(rows=cv["idx"]))

    for sparse in (False, True):
        cases.append(autograd_case(
            f"fm_first_order-{'rows' if sparse else 'dense'}", fm_in,
            lambda emb, w1, bias, rows, sparse=sparse: dict(yfm=kern().fm_first_order(emb, rows, w1, bias, sparse)[1]),
            lambda emb, w1, bias, rows: dict(yfm=ro.fm_second_order(emb).view(-1) + w1[rows].sum(dim=(1, 2)) + bias),
            exact=True, int_grads=True))

    def mask_in():
        lv, cv = ints(4)
        gen = torch.Generator().manual_seed(5)
        cv["mask"] = torch.rand(N, D, generator=gen) < 0.5
        return lv, cv
    cases.append(autograd_case("masked_gather", mask_in, lambda W, idx, mask: dict(out=kern().masked_gather(idx, W, mask)),
                               lambda W, idx, mask: dict(out=ro.pep_retrain_forward(idx, W, mask)), exact=True, int_grads=True))

    def soft_in():
        import test_pep_deepfm_gpu as tp

        gen = torch.Generator().manual_seed(6)
        s = tp._threshold("feature_dim", N, D, gen)
        return dict(W=tp._table(s, N, D, gen), s=s), dict(idx=torch.randint(0, N, (B, F), generator=gen))
    cases.append(autograd_case("soft_threshold_gather", soft_in, lambda W, s, idx: dict(out=kern().soft_threshold_gather(idx, W, s)),
                               lambda W, s, idx: dict(out=ro.pep_forward(idx, W, s)), default=(1e-5, 1e-6)))

    def count_run():
        (lv, _cv) = soft_in()
        return dict(count=kern().soft_count_kept(lv["W"].to(DEV), lv["s"].to(DEV)))

    def count_check(result):
        (lv, _cv) = soft_in()
        assert int(result["count"]) == int(torch.count_nonzero(ro.soft_threshold(lv["W"].double(), lv["s"].double())))
    cases.append(Case("soft_count_kept", count_run, count_check, True))
    return cases


# ---- the sharded lookup's local kernels (tests/test_route_gpu.py, tests/test_sharded_dedup_gpu.py) ---------------------------
def _route_operands(B, F, world):
    from recsys_benchmark_amd.sharded import bucket_capacity

    g = torch.Generator().manual_seed(B * 131 + F + world)
    dims = torch.randint(1, 5000, (F,), generator=g)
    offsets = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.long), dims[:-1]]), 0)
    x = torch.stack([torch.randint(0, int(d), (B,), generator=g) for d in dims], 1)
    return x, offsets, int(dims.sum()), bucket_capacity(B * F, world, 1.25)


def _route_case(B, F, world, unique):
    """route_buckets / route_buckets_unique against the torch restatement, bit for bit
    (test_route_matches_restatement_bit_exact, test_route_unique_matches_restatement_bit_exact)."""
    def run():
        from recsys_benchmark_amd import _kernels

        x, offsets, N, cap = _route_operands(B, F, world)
        of = torch.zeros(1, dtype=torch.int32, device=DEV)
        fn = _kernels.route_buckets_unique if unique else _kernels.route_buckets
        got = fn(x.to(DEV), offsets.to(DEV), world, N, cap, of)
        out = dict(send=got[0], slot=got[1], overflow=of)
        if unique:
            out["segments"] = got[2]
        return out

    def check(result):
        x, offsets, N, cap = _route_operands(B, F, world)
        of_ref = torch.zeros(1, dtype=torch.int32)
        if unique:
            from sharded_dedup_helpers import DedupTorchOps, slots_from_segments

            send_ref, slot_ref, _ = DedupTorchOps.route_buckets_unique(x, offsets, world, N, cap, of_ref)
            rebuilt, ascending = slots_from_segments(result["segments"], world * cap, x.numel())
            assert ascending and torch.equal(rebuilt, slot_ref.reshape(-1))
        else:
            from oracle.sharded_ops import TorchOps

            send_ref, slot_ref = TorchOps.route_buckets(x, offsets, world, N, cap, of_ref)
        assert torch.equal(result["slot"].cpu(), slot_ref) and torch.equal(result["send"].cpu(), send_ref)
        assert int(result["overflow"]) == int(of_ref)

    return Case(f"route_buckets{'_unique' if unique else ''}-B{B}-F{F}-world{world}", run, check, True)


def _pack_case(D):
    def operands():
        g = torch.Generator().manual_seed(D)
        return torch.randint(0, 500, (777,), generator=g), torch.randn(500, D, generator=g), torch.randn(500, 1, generator=g)

    def run():
        from recsys_benchmark_amd import _kernels

        rows, W, w1 = operands()
        packed = _kernels.gather_pack_rows(rows.to(DEV), W.to(DEV), w1.to(DEV))
        vals, lin = _kernels.unpack_rows(packed, D)
        return dict(packed=packed, vals=vals, lin=lin)

    def check(result):
        from oracle.sharded_ops import TorchOps

        rows, W, w1 = operands()
        ref = TorchOps.gather_pack_rows(rows, W, w1)
        ref_vals, ref_lin = TorchOps.unpack_rows(ref, D)
        assert torch.equal(result["packed"].cpu(), ref)                 # copies: bit-exact
        assert torch.equal(result["vals"].cpu(), ref_vals) and torch.equal(result["lin"].cpu(), ref_lin)

    return Case(f"gather_pack_unpack_rows-D{D}", run, check, True)


def _slot_fm_case(B, F, D, unique):
    """slot_fm (test_slot_fm_forward_backward) / slot_fm_unique (test_segment_backward_sums_shared_slots) against autograd
    through the torch restatement: rows exact, y_fm 1e-5 / 1e-5, gradient rows 1e-5 / 1e-5, bias 1e-5 / 1e-6."""
    def operands():
        g = torch.Generator().manual_seed(B + F + D)
        n = B * F
        if unique:
            S = n // 2 + 11
            slot = torch.randint(0, max(S - 5, 1), (n,), generator=g)
            slot[torch.rand(n, generator=g) < 0.4] = 2
            slot[0] = S
            slot = slot.view(B, F)
        else:
            S = n + 11
            slot = torch.randperm(S, generator=g)[:n].view(B, F)
            slot[0, 0] = S
        buf = torch.randn(S + 1, D + 4, generator=torch.Generator().manual_seed(B * F + D)) * 0.1
        buf[:, D + 1:] = 0
        buf[S] = 0
        return S, buf, slot, torch.tensor([0.3]), torch.randn(B, F, D, generator=g), torch.randn(B, generator=g)

    def run():
        from recsys_benchmark_amd import _kernels, _lib

        S, buf, slot, bias, g_emb, g_y = operands()
        hb, hbias = buf.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
        if unique:
            from sharded_dedup_helpers import segments_from_slots

            e, y = _kernels.slot_fm_unique(hb, slot.to(DEV), hbias, segments_from_slots(slot, S).to(DEV))
        else:
            e, y = _kernels.slot_fm(hb, slot.to(DEV), hbias)
        ((e * g_emb.to(DEV)).sum() + (y * g_y.to(DEV)).sum()).backward()
        _lib.check_index_errors()
        return dict(emb=e.detach(), yfm=y.detach(), gbuf=hb.grad, gbias=hbias.grad)

    cache = {}

    def check(result):
        from conftest import assert_close
        from oracle.sharded_ops import TorchOps

        S, buf, slot, bias, g_emb, g_y = operands()
        if "ref" not in cache:
            rb, rbias = buf.clone().requires_grad_(True), bias.clone().requires_grad_(True)
            e_ref, y_ref = TorchOps.slot_fm(rb, slot, rbias)
            ((e_ref * g_emb).sum() + (y_ref * g_y).sum()).backward()
            cache["ref"] = (e_ref.detach(), y_ref.detach(), rb.grad, rbias.grad)
        e_ref, y_ref, gb_ref, gbias_ref = cache["ref"]
        assert torch.equal(result["emb"].cpu(), e_ref)
        assert_close(result["yfm"], y_ref, 1e-5, 1e-5, "y_fm")
        hg = result["gbuf"]
        assert_close(hg[:S, :D + 1], gb_ref[:S, :D + 1], 1e-5, 1e-5, "grad rows")
        assert not hg[:S, D + 1:].any()
        unused = torch.ones(S, dtype=torch.bool)
        unused[slot.view(-1)[slot.view(-1) < S]] = False
        assert not hg[:S][unused.to(DEV)].any()
        assert_close(result["gbias"], gbias_ref, 1e-5, 1e-6, "bias grad")

    return Case(f"slot_fm{'_unique' if unique else ''}-B{B}-F{F}-D{D}", run, check, True)


# ---- DCN heads (tests/test_dcn_gpu.py) -----------------------------------------------------------------------------------------
def _dcn_head_case(M, d, L):
    """DCNHead against oracle dcn_head: test_dcn_head_vs_oracle's tolerances (out 1e-4 / 1e-4, gradients 1e-3 / 1e-4 * scale)."""
    def build():
        from recsys_benchmark_amd.layer_dcn import DCNHead

        gen = torch.Generator().manual_seed(M + d)
        torch.manual_seed(M + d)
        head = DCNHead(L, d)
        return head, torch.randn(M, d, generator=gen) * 0.3, torch.randn(M, d, generator=gen)

    def run():
        head, X, G = build()
        head.to(DEV)
        xd = X.to(DEV).requires_grad_(True)
        out = head(xd)
        (out * G.to(DEV)).sum().backward()
        return dict(out=out.detach(), dx=xd.grad, **_module_grads(head))

    cache = {}

    def check(result):
        from conftest import assert_close
        from oracle import reference_ops as ro

        if "ref" not in cache:
            head, X, G = build()
            p = {k: v.detach().clone().double().requires_grad_(True) for k, v in head.state_dict().items()}
            x = X.double().requires_grad_(True)
            ref = ro.dcn_head(x, p, L)
            (ref * G.double()).sum().backward()
            cache["ref"] = (ref.detach(), x.grad, p)
        ref, dx, p = cache["ref"]
        assert_close(result["out"], ref.float(), 1e-4, 1e-4, "out")
        assert_close(result["dx"], dx.float(), 1e-3, 1e-4 * max(1.0, float(dx.abs().max())), "grad x")
        for k, v in p.items():
            assert_close(result["g/" + k], v.grad.float(), 1e-3, 1e-4 * max(1.0, float(v.grad.abs().max())), k)

    # (the forward is one unsplit product per layer with the cross epilogue; the bias gradients are atomic column sums)
    return Case(f"dcn_head-M{M}-d{d}-L{L}", run, check, lambda key: key == "out")


def _dcn_mix_case(M, d, E, r, L):
    """DCN_MixHead against oracle dcn_mix_head: test_dcn_mixhead_vs_oracle's tolerances."""
    def build():
        from recsys_benchmark_amd.layer_dcn import DCN_MixHead

        gen = torch.Generator().manual_seed(M + d + r)
        torch.manual_seed(M + d + r)
        head = DCN_MixHead(E, L, r, d)
        with torch.no_grad():
            for b in head.biases:
                b.copy_(torch.randn(b.shape, generator=gen) * 0.1)
        return head, torch.randn(M, d, generator=gen) * (0.05 if d > 100 else 0.3), torch.randn(M, d, generator=gen)

    def run():
        head, X, G = build()
        head.to(DEV)
        xd = X.to(DEV).requires_grad_(True)
        out = head(xd)
        (out * G.to(DEV)).sum().backward()
        return dict(out=out.detach(), dx=xd.grad, **_module_grads(head))

    cache = {}

    def check(result):
        from conftest import assert_close
        from oracle import reference_ops as ro

        if "ref" not in cache:
            head, X, G = build()
            p = {k: v.detach().clone().double().requires_grad_(True) for k, v in head.state_dict().items()}
            x = X.double().requires_grad_(True)
            ref = ro.dcn_mix_head(x, p, L)
            (ref * G.double()).sum().backward()
            cache["ref"] = (ref.detach(), x.grad, p)
        ref, dx, p = cache["ref"]
        assert_close(result["out"], ref.float(), 2e-4, 1e-4 * max(1.0, float(ref.abs().max())), "out")
        assert_close(result["dx"], dx.float(), 2e-3, 2e-4 * max(1.0, float(dx.abs().max())), "grad x")
        for k, v in p.items():
            assert_close(result["g/" + k], v.grad.float(), 2e-3, 2e-4 * max(1.0, float(v.grad.abs().max())), k)

    return Case(f"dcn_mix_head-M{M}-d{d}-E{E}-r{r}-L{L}", run, check)


# ---- NeuMF (tests/test_neumf_gpu.py) ----------------------------------------------------------------------------------------------
def _neumf_train_case(n_neg, sparse, det):
    """One NeuMF training step against the reference's recorded losses and gradients: test_neumf_gpu._train_and_compare holds
    the comparison (losses 1e-5 / 1e-6, gradients 1e-4 / 1e-6) and runs inside the case."""
    def run():
        import test_neumf_gpu as tn
        from conftest import load_golden

        g = load_golden(f"neumf_train_neg{n_neg}")
        with _deterministic(det):
            model = tn._model(g, {"name": "vanilla", "sparse": True} if sparse else None)
            grads = tn._train_and_compare(g, model)
        return {"g/" + k: v for k, v in grads.items()}

    def check(result):
        """The losses are compared where they exist, inside _train_and_compare (it ran under poison, in run()); the returned
        gradients once more here, against the same recorded values at the same tolerance."""
        from conftest import load_golden

        want = load_golden(f"neumf_train_neg{n_neg}").group("grad/")
        assert {k[2:] for k in result} == set(want)
        for k, v in want.items():
            torch.testing.assert_close(dense(result["g/" + k]).cpu(), v, rtol=1e-4, atol=1e-6, msg=k)

    return Case(f"neumf-train-neg{n_neg}-{'rows' if sparse else 'dense'}-{'det' if det else 'default'}", run, check,
                bool(det or sparse))


def _neumf_forward_case(name, cfg):
    def run():
        import test_neumf_gpu as tn
        from conftest import load_golden
        from recsys_benchmark_amd.neumf import ModelFlag

        g = load_golden(name)
        model = tn._model(g, cfg).eval()
        out = {}
        with torch.no_grad():
            for flag in (ModelFlag.MLP, ModelFlag.GMF, ModelFlag.NMF):
                model.flag = flag
                for tag in ("1d", "2d"):
                    out[f"{tag}/{flag.name}"] = model(g.t(f"users_{tag}").to(DEV), g.t(f"items_{tag}").to(DEV))
        return out

    def check(result):
        from conftest import load_golden

        g = load_golden(name)
        for k, v in result.items():
            torch.testing.assert_close(v.cpu(), g.t("out_" + k), rtol=1e-5, atol=1e-6)

    return Case(f"neumf-forward-{name}", run, check, True)


def _neumf_score_case():
    """score_all_items against the float64 restatement of test_neumf_gpu (1e-5 / 1e-5)."""
    def build():
        from conftest import load_golden
        from recsys_benchmark_amd.neumf import NeuMF

        g = load_golden("neumf_validate")
        nu, ni = int(g["num_user"]), int(g["num_item"])
        model = NeuMF(nu, ni, emb_size=16, hidden_sizes=[16, 8]).to(DEV)
        model.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
        return model.eval(), nu, g

    def run():
        model, nu, _g = build()
        return dict(scores=model.score_all_items(torch.arange(nu, device=DEV)))

    def check(result):
        import test_neumf_gpu as tn

        model, nu, g = build()
        torch.testing.assert_close(result["scores"], tn._scores64(model, torch.arange(nu, device=DEV)).float(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(result["scores"].cpu(), g.t("scores"), rtol=1e-5, atol=1e-5)

    return Case("neumf-score_all_items", run, check, True)


# ---- OptEmbed on the CF tables (tests/test_optembed_cf_gpu.py) ----------------------------------------------------------------
def _optembed_cf_case(case):
    """The supernet table under the recorded masks against the reference: outputs bit for bit, gradients 1e-5 / 1e-6
    (test_table_matches_reference); the backward sums in a fixed order (test_backward_is_bit_identical_across_runs)."""
    def run():
        import test_optembed_cf_gpu as to
        from conftest import load_golden

        g = load_golden(f"optembed_cf_{case}")
        emb = to._table(g)
        G = g.t("g").to(DEV)
        field_d = str(g["mode_d"]) == "field"
        masks = {"train_rows": (True, g.t("row_mask")), "train_bool": (True, g.t("bool_mask")), "eval_none": (False, None),
                 "eval_int": (False, g.t("field_mask") if field_d else g.t("row_mask"))}
        out = {}
        for tag, (train, mask) in masks.items():
            emb.train(train)
            emb.zero_grad()
            w = emb.get_weight(None if mask is None else mask.to(DEV))
            (w * G).sum().backward()
            out[f"{tag}/out"] = w.detach()
            for name, p in emb.named_parameters():
                if p.grad is not None:
                    out[f"{tag}/grad/{name}"] = p.grad.clone()
        return out

    def check(result):
        import test_optembed_cf_gpu as to
        from conftest import load_golden

        g = load_golden(f"optembed_cf_{case}")
        for k, v in result.items():
            if k.endswith("/out"):
                to._eq(v, g[k], k)
            elif k in g:
                to._close(v, g[k], k)

    return Case(f"optembed_cf-{case}", run, check, True)


# ---- magnitude pruning (tests/test_mag_prune_gpu.py) --------------------------------------------------------------------------
def _mag_prune_case(n, d):
    """prune_table (k-th magnitude select) and the CSR build of PrunedEmbedding.from_pruned against the host contract
    (mag_prune_helpers.mag_prune), bit for bit."""
    p, m = 0.6, 2

    def run():
        import recsys_benchmark_amd as pkg
        from recsys_benchmark_amd.embeddings.pruned_embedding import PrunedEmbedding

        gen = torch.Generator().manual_seed(1000 * d + n)
        w = (torch.randn(n, d, generator=gen) * 0.1).to(DEV)
        emb = PrunedEmbedding.from_pruned(w, p, m)
        ids = torch.randint(0, n, (3, 50), generator=gen).to(DEV)
        return dict(pruned=pkg.prune_table(w.clone(), p, m), crow=emb.crow_indices, col=emb.col_indices, values=emb.values,
                    rows=emb(ids), weight=emb.get_weight())

    def check(result):
        import mag_prune_helpers as H

        gen = torch.Generator().manual_seed(1000 * d + n)
        w = torch.randn(n, d, generator=gen) * 0.1
        want = H.mag_prune(w, p, m)
        ids = torch.randint(0, n, (3, 50), generator=gen)
        assert torch.equal(result["pruned"].cpu().view(torch.int32), want.view(torch.int32))
        csr = want.to_sparse_csr()
        assert torch.equal(result["crow"].cpu(), csr.crow_indices().to(result["crow"].dtype))
        assert torch.equal(result["col"].cpu(), csr.col_indices().to(result["col"].dtype))
        assert torch.equal(result["values"].cpu(), csr.values())
        assert torch.equal(result["rows"].cpu(), want[ids]) and torch.equal(result["weight"].cpu(), want)

    return Case(f"mag_prune-n{n}-d{d}", run, check, True)


# ---- CTRMetric (tests/test_ctr_metric_gpu.py) -----------------------------------------------------------------------------------
def _ctr_metric_case(n):
    """CTRMetric fed in three batches from a small capacity (it grows), against the whole set: the AUC equals
    trainer.binary_auc's, the log-loss the float64 numpy sum within 1e-12 relative (test_ctrmetric_accumulates...)."""
    def batches():
        gen = torch.Generator().manual_seed(n)
        cuts = [0, n // 3, n // 2, n]
        x = 4 * torch.randn(n, generator=gen)
        y = torch.rand(n, generator=gen) < 0.4
        y[0], y[-1] = True, False
        return [(x[a:b], (y[a:b].long() if i % 2 == 0 else y[a:b].float())) for i, (a, b) in enumerate(zip(cuts, cuts[1:])) if b > a], x, y

    def run():
        import recsys_benchmark_amd as pkg

        bs, _x, _y = batches()
        metric = pkg.CTRMetric(torch.device(DEV, 0), capacity=2)
        for xb, yb in bs:
            metric.add(xb.to(DEV), yb.to(DEV))
        res = metric.compute()
        return dict(auc=torch.tensor(res["auc"], dtype=torch.float64), log_loss=torch.tensor(res["log_loss"], dtype=torch.float64),
                    loss_sum=metric._loss_sum.clone())

    def check(result):
        from ctr_metric_helpers import bce_sum
        from recsys_benchmark_amd import trainer

        _bs, x, y = batches()
        assert float(result["auc"]) == trainer.binary_auc(y.double().to(DEV), torch.sigmoid(x.to(DEV)))
        want = bce_sum(x.numpy(), y.double().numpy()) / n
        assert abs(float(result["log_loss"]) - want) <= 1e-12 * want

    return Case(f"ctr_metric-n{n}", run, check, True)


# ---- BCE with logits (tests/test_mlp_gpu.py) -----------------------------------------------------------------------------------
def _bce_case(n, unit):
    """losses.BCEWithLogitsLoss against torch's in float64: loss 1e-5 / 1e-6, gradient 1e-5 / 1e-8
    (test_fused_bce_with_logits_matches_torch); seeded with an ordinary upstream gradient and with the resident unit."""
    def operands():
        gen = torch.Generator().manual_seed(n)
        return torch.randn(n, generator=gen) * 4, (torch.rand(n, generator=gen) < 0.3).float()

    def run():
        from recsys_benchmark_amd.losses import BCEWithLogitsLoss, unit_scalar

        x, y = operands()
        xd = x.to(DEV).requires_grad_(True)
        out = BCEWithLogitsLoss()(xd, y.to(DEV))
        if unit:
            out.backward(unit_scalar(DEV))
        else:
            (out * 1.7).backward()
        return dict(loss=out.detach(), dx=xd.grad)

    def check(result):
        from conftest import assert_close

        x, y = operands()
        x64 = x.double().requires_grad_(True)
        ref = torch.nn.BCEWithLogitsLoss()(x64, y.double())
        (ref * (1.0 if unit else 1.7)).backward()
        assert_close(result["loss"], ref.float(), 1e-5, 1e-6, "loss")
        assert_close(result["dx"], x64.grad.float(), 1e-5, 1e-8, "dlogits")

    return Case(f"bce_with_logits-n{n}-{'unit' if unit else 'scaled'}", run, check, True)


# ---- the fused LightGCN step (tests/test_lightgcn_gpu.py) ---------------------------------------------------------------------
def _lightgcn_step_case(D, L, rows_only):
    """lightgcn_propagate_reg on the dyadic graph: the propagation, the regulariser and (rows_only) the last layer restricted to
    the batch's rows.  The rows the step reads against the dense float64 product (exact on this fixture), the regulariser at
    test_reg_loss_rows_matches_float64_at_every_width's 1e-5 / 1e-5, the table gradients (propagation + scattered reg rows,
    float atomics) at test_propagate_vs_oracle's 1e-4 / 1e-5."""
    B = 37

    def batch():
        fx, adj, A = _dyadic_square(D)
        gen = torch.Generator().manual_seed(D + L)
        users = torch.randint(0, fx["U"], (B,), generator=gen)
        pos, neg = torch.randint(0, fx["I"], (B,), generator=gen), torch.randint(0, 30, (B,), generator=gen)
        users[0], pos[0] = 3, 5                      # the hub user and the hub item of the fixture
        G = [(2 * torch.randint(-8, 8, (B, D), generator=gen) + 1).float() / 16 for _ in range(3)]
        return fx, adj, A, users, pos, neg, G

    def both(fn, to):
        fx, adj, A, users, pos, neg, G = batch()
        Xu, Xi = to(fx["Xu"]).requires_grad_(True), to(fx["Xi"]).requires_grad_(True)
        au, ai, reg = fn(Xu, Xi, users, pos, neg)
        rows = dict(user_rows=au[users], pos_rows=ai[pos], neg_rows=ai[neg], reg=reg)
        loss = sum((rows[k] * to(g)).sum() for k, g in zip(("user_rows", "pos_rows", "neg_rows"), G)) + 0.5 * reg
        loss.backward()
        out = {k: v.detach() for k, v in rows.items()}
        out.update(dXu=Xu.grad, dXi=Xi.grad)
        return out

    def run():
        from recsys_benchmark_amd import _kernels

        adj = _dyadic_square(D)[1].to(DEV)
        return both(lambda Xu, Xi, u, p, n: _kernels.lightgcn_propagate_reg(adj, Xu, Xi, L, u.to(DEV), p.to(DEV), n.to(DEV),
                                                                            batch_rows_only=rows_only), lambda t: t.to(DEV))

    cache = {}

    def check(result):
        from conftest import assert_close

        if "ref" not in cache:
            assert _dyadic_claim(D, L)
            A = _dyadic_square(D)[2]

            def ref(Xu, Xi, u, p, n):
                out = _lightgcn_ref(A, torch.cat([Xu, Xi]), L)
                reg = (Xu[u].pow(2).sum() + Xi[p].pow(2).sum() + Xi[n].pow(2).sum()) / (2 * u.numel())
                return out[:Xu.shape[0]], out[Xu.shape[0]:], reg
            cache["ref"] = both(ref, lambda t: t.double())
        want = cache["ref"]
        for k in ("user_rows", "pos_rows", "neg_rows"):
            assert torch.equal(result[k].cpu().double(), want[k]), k
        assert_close(result["reg"], want["reg"].float(), 1e-5, 1e-5, "reg")
        assert_close(result["dXu"], want["dXu"].float(), 1e-4, 1e-5, "grad user table")
        assert_close(result["dXi"], want["dXi"].float(), 1e-4, 1e-5, "grad item table")

    return Case(f"lightgcn_step-{'rows_only' if rows_only else 'full'}-D{D}-L{L}", run, check, lambda k: k.endswith("rows") or k == "reg")


def _build2():
    cases = []
    for n, k, hidden, D in ((257, 64, [32, 32], 16), (70, 128, [], 8)):
        cases += [_mish_case(bn, tr, n, k, hidden, D) for bn in (0, 1, 2) for tr in (True, False)]
    cases += [_tt_case("plain-3cores", 20000, [128, 96], [25, 25, 32], [2, 2, 4], (64, 3)),
              _tt_case("plain-2cores", 20000, [32], [200, 100], [4, 4], (37,)),
              _tt_case("grouped-3cores", 20000, [16, 8], [10, 50, 40], [2, 2, 4], (6000,)),
              _tt_case("grouped-2cores", 20000, [32], [200, 100], [4, 4], (4500,))]
    cases += [_qat_case("qat_int8"), _qat_case("qat_int16"), _csr_rows_case()]
    cases += _simple_gather_cases()
    for B, F, world in ((5, 3, 2), (39, 26, 3)):
        cases += [_route_case(B, F, world, False), _route_case(B, F, world, True)]
    cases += [_pack_case(4), _pack_case(16)]
    for B, F, D in ((1, 1, 16), (33, 26, 16), (17, 100, 8), (9, 5, 64)):
        cases += [_slot_fm_case(B, F, D, False), _slot_fm_case(B, F, D, True)]
    cases += [_dcn_head_case(33, 20, 1), _dcn_head_case(100, 416, 2), _dcn_mix_case(50, 40, 3, 8, 2)]
    cases += [_neumf_train_case(nn, sp, det) for nn in (1, 3) for sp in (False, True) for det in (False, True) if not (sp and det)]
    cases += [_neumf_forward_case("neumf_model", None), _neumf_forward_case("neumf_qr", {"name": "qr", "operation": "mult", "divider": 3}),
              _neumf_score_case()]
    cases += [_optembed_cf_case(c) for c in ("l1_field_field", "l2_feature_feature", "l2_field_feature_d6", "d_only")]
    cases += [_mag_prune_case(63, 8), _mag_prune_case(4097, 24)]
    cases += [_ctr_metric_case(n) for n in (3, 257, 4097)]
    cases += [_bce_case(n, unit) for n in (1, 37, 4097) for unit in (False, True)]
    for D in PROP_WIDTHS:
        for L in PROP_LAYERS:
            cases += [_lightgcn_step_case(D, L, False), _lightgcn_step_case(D, L, True)]
    return cases


# ---- third batch: DeepFM OptEmbed, the CF data kernels, top-k scoring -----------------------------------------------------------
def _optembed_deepfm_retrain_case(mode, form):
    """One retraining step of DeepFM on OptEmbed's masked lookup against the reference's golden: logits 2e-5 / 2e-6, gradients
    1e-4 / 5e-6 (test_optembed_deepfm_gpu.test_retrain_logits_and_gradients_match_the_reference)."""
    def run():
        import test_optembed_deepfm_gpu as tod
        from conftest import load_golden

        g = load_golden(f"optembed_deepfm_retrain_{mode}")
        m = tod._retrain_from_golden(g, rows=form == "rows").train()
        with _deterministic(form == "deterministic"):
            logits, grads = tod._retrain_step(m, g)
        return dict(logits=logits, **{"g/" + k: v for k, v in grads.items()})

    def check(result):
        from conftest import assert_close, load_golden

        g = load_golden(f"optembed_deepfm_retrain_{mode}")
        assert_close(result["logits"], g.t("logits"), 2e-5, 2e-6, "logits")
        for k, ref in g.group("grad/").items():
            assert_close(result["g/" + k], ref, 1e-4, 5e-6, f"grad {k}")
        assert torch.count_nonzero(result["g/embedding._weight"].cpu()[~g.t("mask").bool()]) == 0

    return Case(f"optembed_deepfm-retrain-{mode}-{form}", run, check, lambda k: form == "deterministic" or k == "logits")


def _optembed_deepfm_candidate_case(mode):
    """Candidate evaluation of the DeepFM supernet (get_weight(mask_d) and set_candidate) against the golden logits, 2e-5 / 2e-6
    (test_candidate_logits_match_the_reference)."""
    def run():
        import test_optembed_deepfm_gpu as tod
        from conftest import load_golden

        g = load_golden(f"optembed_deepfm_candidate_{mode}")
        m = tod._supernet_from_golden(g).eval()
        x = g.t("x").to(DEV)
        out = {}
        with torch.no_grad():
            m.embedding.get_weight(g.t("mask_d"))
            out["lookup"] = m(x)
            m.embedding.set_candidate(g.t("mask_d").to(DEV))
            out["candidate"] = m(x)
            m.embedding.clear_candidate()
            out["cleared"] = m(x)
        return out

    def check(result):
        from conftest import assert_close, load_golden

        g = load_golden(f"optembed_deepfm_candidate_{mode}")
        for k, v in result.items():
            assert_close(v, g.t("logits"), 2e-5, 2e-6, "logits, " + k)

    return Case(f"optembed_deepfm-candidate-{mode}", run, check, True)


def _cf_sample_case(mode, K):
    """cf_sample_triples through DeviceCFGraphDataset.sample on the recorded sample graph, bit for bit against the NumPy
    restatement (test_sampler_is_bit_equal_to_the_restatement)."""
    def run():
        import test_cf_data_gpu as tc

        ds = tc.pkg.DeviceCFGraphDataset(tc.graphs("sample")[0], sampling_method=mode, num_neg_item=K, device=tc.DEV)
        users, pos, neg = ds.sample(0, len(ds), 4, tc.SEED)
        return dict(users=users, pos=pos, neg=tc.neg2d(neg))

    def check(result):
        import test_cf_data_gpu as tc

        hg = tc.graphs("sample")[1]
        want = tc.sample_restated(hg, mode, K, 0, hg.epoch_len(mode), tc.SEED, 4)
        tc.assert_bits((result["users"], result["pos"], list(result["neg"])), want, f"sample {mode} K={K}")

    return Case(f"cf_sample_triples-{mode}-K{K}", run, check, True)


def _ndcg_case(n, k, items, longest):
    """ndcg_recall_rows against the NumPy restatement, exactly (test_metric_kernel_equals_ndcg_recall_at_k)."""
    def operands():
        gen = torch.Generator().manual_seed(n * 131 + k)
        lens = torch.randint(1, longest + 1, (n,), generator=gen)
        lens[0], lens[-1] = 1, longest
        sets = [set(torch.randperm(items, generator=gen)[:int(m)].tolist()) for m in lens]
        scores = torch.rand(n, items, generator=gen)
        for u, st in enumerate(sets):
            scores[u, list(st)[:max(1, len(st) // 2)]] += 0.5
        return torch.topk(scores, k + 3)[1], torch.randperm(n, generator=gen), sets

    def run():
        import test_cf_data_gpu as tc
        from recsys_benchmark_amd import _kernels

        pred, perm, sets = operands()
        crow, col = tc.truth_csr(sets)
        ndcg, recall = _kernels.ndcg_recall_rows(pred.to(DEV), perm.to(DEV), crow, col, k)
        return dict(ndcg=ndcg, recall=recall)

    def check(result):
        import numpy as np
        import test_cf_data_gpu as tc

        pred, perm, sets = operands()
        crow, col = tc.truth_csr(sets)
        want = tc.ndcg_recall_rows_restated(pred.numpy(), perm.numpy(), crow.cpu().numpy(), col.cpu().numpy(), k)
        assert np.array_equal(result["ndcg"].cpu().numpy(), want[0]) and np.array_equal(result["recall"].cpu().numpy(), want[1])

    return Case(f"ndcg_recall_rows-n{n}-k{k}", run, check, True)


def _score_topk_case(nu, ni, B, k):
    """score_topk against the reference loop (oracle masked_topk): test_score_topk_matches_reference_loop's rule — where the
    indices differ the float64 scores are within 1e-5 / 1e-4, and more than 99% agree."""
    def operands():
        import test_lightgcn_step_gpu as ts

        gen = torch.Generator().manual_seed(nu + ni + k)
        ue, ie = torch.randn(nu, 64, generator=gen), torch.randn(ni, 64, generator=gen)
        graph = ts._graph(nu, ni, gen, max_items=min(40, max(1, ni - k)))
        return ue, ie, graph, torch.randint(0, nu, (B,), generator=gen)

    def run():
        from recsys_benchmark_amd.lightgcn import score_topk, train_items_csr

        ue, ie, graph, users = operands()
        csr = train_items_csr(graph, nu, torch.device(DEV, 0))
        return dict(filtered=score_topk(ue.to(DEV), ie.to(DEV), users.to(DEV), k, csr),
                    unfiltered=score_topk(ue.to(DEV), ie.to(DEV), users.to(DEV), k, None))

    def check(result):
        from conftest import assert_close
        from oracle import reference_ops as ro

        ue, ie, graph, users = operands()
        scores = ue.double()[users] @ ie.double().T
        for key, filt in (("filtered", True), ("unfiltered", False)):
            got, ref = result[key].cpu(), ro.masked_topk(ue, ie, users, graph, k, filter_item_on_train=filt)
            same = got == ref
            if not bool(same.all()):
                assert_close(torch.gather(scores, 1, got)[~same], torch.gather(scores, 1, ref)[~same], 1e-5, 1e-4, "swapped neighbours")
            assert float(same.float().mean()) > 0.99
        for i, u in enumerate(users.tolist()):
            assert not set(result["filtered"][i].tolist()) & set(graph[u])

    return Case(f"score_topk-nu{nu}-ni{ni}-B{B}-k{k}", run, check, True)


def _build3():
    cases = [_optembed_deepfm_retrain_case(mode, form) for mode in ("field", "feature") for form in ("dense", "rows", "deterministic")]
    cases += [_optembed_deepfm_candidate_case(mode) for mode in ("field", "feature")]
    cases += [_cf_sample_case("uniform", 1), _cf_sample_case("popularity", 3)]
    cases += [_ndcg_case(1, 1, 50, 3), _ndcg_case(77, 5, 60, 12)]
    cases += [_score_topk_case(50, 300, 17, 20), _score_topk_case(40, 25, 9, 20)]
    return cases


# ---- fourth batch: the remaining branches ------------------------------------------------------------------------------------------
def _deepfm_eval_case():
    """DeepFM inference without grad on the fused tail (the head in the last product's epilogue) against the float64 oracle
    in eval mode, smoke()'s logits tolerance 1e-4 / 1e-5."""
    dims, D, B = [11, 7, 5, 13], 16, 33

    def build():
        import recsys_benchmark_amd as pkg

        torch.manual_seed(0)
        m = pkg.DeepFM(dims, D, [32, 32], p_dropout=0.0, use_batchnorm=True, embedding_config={"name": "vanilla", "sparse": True},
                       fc_sparse=True)
        gen = torch.Generator().manual_seed(1)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(0, 0.3, generator=gen)
                mod.running_var.uniform_(0.5, 1.5, generator=gen)
        return m.eval(), torch.stack([torch.randint(0, d, (B,), generator=gen) for d in dims], 1)

    def run():
        m, x = build()
        m.to(DEV)
        with torch.no_grad():
            return dict(logits=m(x.to(DEV)))

    def check(result):
        from conftest import assert_close
        from oracle import reference_ops as ro

        m, x = build()
        p = {k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
        assert_close(result["logits"], ro.deepfm_forward(x, p, 2, True, False).float(), 1e-4, 1e-5, "logits")

    return Case("deepfm-eval-nograd", run, check, True)


def _tail_no_hidden_case(M=37, K=12):
    """A tail that is the 1-output Linear alone (the rank-1 passes of mlp._Linear1Fn): exact products of small integers."""
    def operands():
        gen = torch.Generator().manual_seed(M + K)
        mk = lambda *sh: torch.randint(-3, 4, sh, generator=gen).float()          # noqa: E731
        return mk(M, K), mk(1, K), mk(1), mk(M), mk(M, 1)

    def run():
        from recsys_benchmark_amd.mlp import run_tail

        x, W, b, add, G = operands()
        lin = torch.nn.Linear(K, 1)
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
        seq = torch.nn.Sequential(lin).to(DEV).train()
        xd, ad = x.to(DEV).requires_grad_(True), add.to(DEV).requires_grad_(True)
        out = run_tail(seq, xd, last_add=ad)
        (out * G.to(DEV)).sum().backward()
        return dict(out=out.detach(), dx=xd.grad, dadd=ad.grad, gW=lin.weight.grad, gb=lin.bias.grad)

    def check(result):
        x, W, b, add, G = (t.double() for t in operands())
        want = dict(out=x @ W.t() + b + add.view(-1, 1), dx=G @ W, dadd=G.view(-1), gW=G.t() @ x, gb=G.sum().view(1))
        for k, v in want.items():
            assert torch.equal(result[k].cpu().double(), v), k

    return Case(f"tail-general-linear-only-M{M}-K{K}", run, check, True)


def _tail_general_dropout_case(M=130, K=48, N=104, p=0.5):
    """The general path's (Linear, BatchNorm1d, ReLU, Dropout) group with dropout on: the kept pattern comes from the
    kernel's own generator, so the comparison uses the mask the output shows (tests/test_mlp_gpu.py checks dropout that way:
    kept fraction and mask consistency between the forward and the backward).  y = keep * relu(bn(z)) / (1 - p) against
    float64 at test_tail_matches_stock_modules_on_the_same_gemms' output tolerance 2e-4 / 2e-4; dx is zero wherever the
    output is."""
    def build():
        import test_tail_gpu as tt

        torch.manual_seed(M + K)
        seq = tt._seq(K, [N], p, bn=True).train()
        return torch.nn.Sequential(*list(seq)[:4]), torch.randn(M, K) * 0.7 + 0.2, torch.randn(M, N)

    def run():
        from recsys_benchmark_amd import mlp
        from recsys_benchmark_amd.mlp import run_tail

        seq, x, G = build()
        with _patched((mlp, "FUSED_TAIL", False)):
            seq = seq.to(DEV)
            xd = x.to(DEV).requires_grad_(True)
            y = run_tail(seq, xd)
            (y * G.to(DEV)).sum().backward()
        return dict(y=y.detach(), dx=xd.grad, **_module_grads(seq))

    def check(result):
        from conftest import assert_close, assert_mostly_close

        seq, x, G = build()
        seq = copy.deepcopy(seq).double()
        x64 = x.double().requires_grad_(True)
        pre = torch.relu(seq[1](seq[0](x64)))
        kept = (result["y"].cpu() != 0)
        frac = kept.float().mean().item()
        assert abs(frac - 0.5 * (1 - p)) < 0.05, frac          # (the BatchNorm output is about symmetric: half survives the ReLU)
        y64 = pre * kept / (1 - p)
        live = pre.detach() > 1e-6          # (a pre-activation on the kink may be dropped by either evaluation)
        assert_close(result["y"].cpu()[live], y64.detach().float()[live], 2e-4, 2e-4, "output under the kernel's own mask")
        (y64 * G.double()).sum().backward()
        scale = float(x64.grad.abs().max()) + 1e-6
        assert_mostly_close(result["dx"], x64.grad.float(), 1e-3, 1e-4 * scale, 2e-3, "grad input")

    return Case(f"tail-general-dropout-M{M}-K{K}-N{N}", run, check)


def _tt_planner_case():
    """The grouped TT lookup with the torch sort / searchsorted planner (beyond the device planner's digit limit)."""
    case = _tt_case("grouped-torch-planner", 20000, [16, 8], [10, 50, 40], [2, 2, 4], (5000,))
    inner = case._run

    def run():
        from recsys_benchmark_amd import _kernels

        with _patched((_kernels, "_TT_PLAN_MAX_P", 0)):
            return inner()

    case._run = run
    return case


def _tt_init_case(name):
    """TTRecTorch(weight_dist="approx-uniform") built like the reference (cores bit-identical), then the lookup: 1e-5 / 1e-6
    (test_tt_approx_uniform_construction_then_lookup)."""
    def run():
        import random

        import numpy as np
        from conftest import load_golden
        from recsys_benchmark_amd.embeddings import TTRecTorch

        g = load_golden(name)
        ps, qs, rs = g["tt_p_shapes"].tolist(), g["tt_q_shapes"].tolist(), g["tt_ranks"].tolist()
        np.random.seed(2023), torch.manual_seed(2023), random.seed(2023)
        explicit = name.endswith("r2x3")
        emb = TTRecTorch(int(g["num_item"]), int(g["hidden"]), rs[1:-1], tt_p_shapes=ps if explicit else None,
                         tt_q_shapes=qs if explicit else None, weight_dist="approx-uniform")
        out = {f"core{i}": c.detach().clone() for i, c in enumerate(emb.tt_cores)}
        emb.to(DEV)
        out.update(lookup=emb(g.t("x").to(DEV)).detach(), weight=emb.get_weight().detach())
        return out

    def check(result):
        from conftest import assert_close, load_golden

        g = load_golden(name)
        for k, v in result.items():
            if k.startswith("core"):
                assert torch.equal(v.cpu(), g.t(f"param/tt_cores.{k[4:]}")), k
        assert_close(result["lookup"], g.t("out"), 1e-5, 1e-6, "lookup")
        assert_close(result["weight"], g.t("weight"), 1e-5, 1e-6, "get_weight")

    return Case(f"tt_init-{name}", run, check, True)


def _dhe_hash_case():
    """The universal hash features against the integer restatement, bit for bit (test_dhe_hash_full_scale_bit_exact)."""
    def run():
        from recsys_benchmark_amd.embeddings.dh_embedding import DHEmbedding

        DHEmbedding.COUNTER = 12345
        torch.manual_seed(5)
        emb = DHEmbedding(2000000000, 16, None, 64, [64]).to(DEV)
        DHEmbedding.COUNTER = 0
        ids = torch.randint(0, 2000000000, (300,), generator=torch.Generator().manual_seed(9))
        return dict(h=emb._get_universal_hash_batch(ids.to(DEV)), slopes=emb._slopes, bias=emb._bias, primes=emb._primes_choices)

    def check(result):
        import numpy as np
        from oracle import int_ops

        ids = torch.randint(0, 2000000000, (300,), generator=torch.Generator().manual_seed(9))
        _, f = int_ops.dhe_hash(ids.numpy(), result["slopes"].cpu().numpy(), result["bias"].cpu().numpy(),
                                result["primes"].cpu().numpy(), 12345)
        assert np.array_equal(result["h"].cpu().numpy(), f)

    return Case("dhe_hash", run, check, True)


def _optembed_cf_retrain_case(md):
    """RetrainOptEmbed on the CF tables against the golden: output bit for bit, gradient 1e-5 / 1e-6 (test_retrain_matches_reference)."""
    def run():
        from conftest import load_golden
        from recsys_benchmark_amd.embeddings import get_embedding

        g = load_golden(f"optembed_cf_retrain_{md}")
        emb = get_embedding({"name": "optembed_d_retrain", "mode_threshold_d": md}, [7, 9], 8)
        emb.load_state_dict({k: g.t("param/" + k) for k in emb.state_dict() if k != "_mask"}, strict=False)
        emb = emb.to(DEV)
        emb.init_mask(g.t("mask_e"), g.t("mask_d"))
        emb.train()
        w = emb.get_weight()
        (w * g.t("g").to(DEV)).sum().backward()
        return dict(out=w.detach(), gW=emb._weight.grad)

    def check(result):
        import test_optembed_cf_gpu as to
        from conftest import load_golden

        g = load_golden(f"optembed_cf_retrain_{md}")
        to._eq(result["out"], g["out"])
        to._close(result["gW"], g["grad/_weight"])

    return Case(f"optembed_cf-retrain-{md}", run, check, True)


def _optembed_cf_draw_case():
    """The device draw of the dimension widths: every row a prefix mask with dimension 0 kept
    (test_device_draws_are_prefix_masks_fresh_per_call_and_one_per_field), the widths reproducible under manual_seed
    (test_draws_reproducible_under_manual_seed) — which is what makes the clean and the poisoned run agree bit for bit."""
    def run():
        from recsys_benchmark_amd import _kernels
        from recsys_benchmark_amd.embeddings import cf_opt_embed as cf
        from recsys_benchmark_amd.embeddings import get_embedding

        torch.manual_seed(123)
        _kernels._cf_seeds.clear()
        emb = get_embedding({"name": "optembed_d", "mode_threshold_d": "feature", "target_sparsity": 0.7}, [300, 500], 64).to(DEV).train()
        emb._salt = 1          # (a table takes the next salt of a process-wide counter: pinned, so that a rerun redraws the same)
        with torch.no_grad():
            emb._weight.fill_(1.0)
        w = emb.get_weight()
        w.sum().backward()
        return dict(table=w.detach(), gW=emb._weight.grad, widths=cf.draw_widths(1000, 64, None, 0, DEV))

    def check(result):
        import test_optembed_cf_gpu as to

        k, prefix = to._widths(result["table"])
        assert prefix and int(k.min()) >= 0
        assert torch.equal(result["gW"], (result["table"] != 0).float())          # d sum(w * mask) / dw = mask
        assert int(result["widths"].min()) >= 0 and int(result["widths"].max()) < 64

    return Case("optembed_cf-device-draw", run, check, True)


def _cerp_num_params_case(N=101, D=8, bucket=30):
    """CerpEmbedding.get_num_params on the counting kernels against count_nonzero of the float64 soft threshold
    (test_num_params_equals_count_nonzero_without_a_table_sized_temporary), the tables kept a margin away from their
    thresholds so that float32 and float64 agree on every element."""
    def build():
        from cerp_cf_helpers import keep_margin
        from recsys_benchmark_amd.embeddings import get_embedding

        torch.manual_seed(N + D)
        emb = get_embedding({"name": "cerp", "bucket_size": bucket}, N, D)
        with torch.no_grad():
            emb.p_threshold.copy_(torch.randn(emb.p_threshold.shape) - 2)
            emb.q_threshold.copy_(torch.randn(emb.q_threshold.shape) - 2)
            emb.p_weight.copy_(keep_margin(torch.randn(emb.p_weight.shape) * 0.3, emb.p_threshold))
            emb.q_weight.copy_(keep_margin(torch.randn(emb.q_weight.shape) * 0.3, emb.q_threshold))
        return emb

    def run():
        return dict(n=torch.tensor(build().to(DEV).get_num_params()))

    def check(result):
        from oracle import reference_ops as ro

        emb = build()
        want = sum(int(torch.count_nonzero(ro.soft_threshold(w.detach().double(), s.detach().double())))
                   for w, s in ((emb.p_weight, emb.p_threshold), (emb.q_weight, emb.q_threshold)))
        assert int(result["n"]) == want

    return Case("cerp-get_num_params", run, check, True)


def _dual_fm_empty_case(kind, geo):
    """gather_fm_dual on an empty batch: zero gradients in every shape, dense and COO
    (test_out_of_range_empty_batch_and_refused_arguments)."""
    def run():
        import test_dual_deepfm_gpu as td

        c = td._case(3, 4, 37, kind, geo)
        out = {}
        for sparse in (False, True) if kind != "soft" else (False,):
            r = td._run(c, sparse=sparse, x=c["x"][:0])
            out.update({f"{'coo' if sparse else 'dense'}/{k}": v for k, v in r.items() if v is not None})
        return out

    def check(result):
        import test_dual_deepfm_gpu as td

        c = td._case(3, 4, 37, kind, geo)
        for key, v in result.items():
            form, k = key.split("/")
            if k in ("emb", "yfm"):
                assert v.numel() == 0
                continue
            like = {"gT1": c["T1"], "gT2": c["T2"], "gw1": c["w1"], "gb": c["bias"], "gS1": c.get("S1"), "gS2": c.get("S2")}[k]
            assert tuple(v.shape) == tuple(like.shape) and torch.count_nonzero(dense(v)) == 0, key

    return Case(f"gather_fm_dual-empty-{kind}", run, check, True)


def _neumf_validate_case():
    """validate_epoch_nmf (scores, masked top-k, device metric) against the reference's recorded metrics, 1e-6
    (test_validate_epoch_nmf_matches_reference)."""
    def run():
        import test_neumf_gpu as tn
        from conftest import load_golden
        from recsys_benchmark_amd import trainer
        from recsys_benchmark_amd.neumf import NeuMF

        g = load_golden("neumf_validate")
        nu, ni = int(g["num_user"]), int(g["num_item"])
        graph = {}
        for u, i in zip(g["edge_user"].tolist(), g["edge_item"].tolist()):
            graph.setdefault(u, []).append(i)
        model = NeuMF(nu, ni, emb_size=16, hidden_sizes=[16, 8])
        model.load_state_dict({k[len("param/"):]: g.t(k) for k in g if k.startswith("param/")})
        true = [[int(x) for x in r if x >= 0] for r in g["true_pad"]]
        users = torch.arange(nu)
        batches = [(users[s:s + 32], true[s:s + 32]) for s in range(0, nu, 32)]
        res = trainer.validate_epoch_nmf(tn._Data(graph), batches, model, device="cuda:0", k=int(g["k"]), metrics=["ndcg", "recall"])
        return dict(ndcg=torch.tensor(res["ndcg"], dtype=torch.float64), recall=torch.tensor(res["recall"], dtype=torch.float64))

    def check(result):
        from conftest import load_golden

        g = load_golden("neumf_validate")
        assert abs(float(result["ndcg"]) - float(g["ndcg"])) <= 1e-6 and abs(float(result["recall"]) - float(g["recall"])) <= 1e-6

    return Case("neumf-validate_epoch", run, check, True)


def _prune_into_view_case(n=63, d=8):
    """prune_table into an output that is not row-strided (a transposed view): pruned through a packed buffer, bit for bit
    the host contract (test_strided_views)."""
    def run():
        import recsys_benchmark_amd as pkg

        w = (torch.randn(n, d, generator=torch.Generator().manual_seed(n + d)) * 0.1).to(DEV)
        out = torch.full((d, n), 7.0, device=DEV).t()
        pkg.prune_table(w, 0.6, 2, out=out)
        return dict(out=out, src=w)

    def check(result):
        import mag_prune_helpers as H

        w = torch.randn(n, d, generator=torch.Generator().manual_seed(n + d)) * 0.1
        assert torch.equal(result["out"].cpu().contiguous().view(torch.int32), H.mag_prune(w, 0.6, 2).view(torch.int32))
        assert torch.equal(result["src"].cpu(), w)

    return Case(f"mag_prune-into-a-transposed-view-n{n}-d{d}", run, check, True)


def _build4():
    cases = [_deepfm_case(True, True, "sums"), _deepfm_case(False, True, "sums"), _deepfm_case(True, True, "sums", "scaled"),
             _deepfm_eval_case(), _tail_no_hidden_case(), _tail_general_dropout_case()]
    for M, K, hidden, p in ((200, 48, [40, 72], 0.5), (67, 16, [8], 0.25)):
        for mode in TAIL_MODES:
            cases += [_tail_case(M, K, hidden, p, mode, True, "sums"), _tail_case(M, K, hidden, p, mode, True, "joins")]
    # (128 floats per row: wider than a wave's 64 outputs, so the last level is a grouped product like the others)
    cases += [_tt_case("grouped-4cores", 20000, [8, 12, 4], [10, 10, 20, 10], [2, 2, 1, 4], (6000,)), _tt_planner_case(),
              _tt_case("grouped-wide-rows", 20000, [8, 8], [25, 25, 32], [4, 4, 8], (4500,), D=128),
              # off D = 16: the last-level kernels at a full wave of outputs; the last level as a GEMM with two cores; and just
              # across the last-level kernels' limit (H*K = 4 * 132 = 528 > 512) at D = 16
              _tt_case("grouped-fast-D64", 20000, [8, 16], [25, 25, 32], [4, 4, 4], (4500,), D=64),
              _tt_case("grouped-gemm-last-2cores", 20000, [8], [200, 100], [4, 12], (4500,), D=48),
              _tt_case("grouped-HK528", 20000, [8, 132], [25, 25, 32], [2, 2, 4], (4500,)),
              _tt_init_case("ttinit_approx_uniform_r2x3"), _dhe_hash_case()]
    cases += [_optembed_cf_retrain_case("feature"), _optembed_cf_retrain_case("field"), _optembed_cf_draw_case(), _cerp_num_params_case()]
    cases += [_dual_fm_empty_case(kind, geo) for kind, geo in (("mult", 3), ("soft", 7), ("mask", 7))]
    cases += [_neumf_validate_case(), _prune_into_view_case()]
    # batches past one sorting run of the per-field sort (its workspace) and of the de-duplicated routing
    cases += _plain_fm_case(26, 16, 1030, masked=False)[2:] + [_route_case(1100, 3, 2, True)]
    return cases


# ---- fifth batch: the packed table layout, the fused expert kernels, the sharded step's local node ----------------------------
def _cross_bwd_head_case(M, N, mix):
    """mi_cross_bwd_head on outputs from torch.empty (NaN under poison) against its three passes written out in torch;
    integer-valued data, so the float-atomic column sums are exact too (test_cross_bwd_head_equals_its_three_passes)."""
    def operands():
        gen = torch.Generator().manual_seed(M * 3 + N + mix)
        mk = lambda *sh: torch.randint(-3, 4, sh, generator=gen).float()          # noqa: E731
        return mk(M, N), mk(M, N), mk(M, N), mk(N), mk(M, 4), mk(M, N)

    def run():
        from recsys_benchmark_amd import _lib

        g, x0, lin, b, gate, dx_prev = (t.to(DEV) for t in operands())
        lib, out = _lib.load(), {}
        for accumulate in (0, 1):
            dlin = torch.empty(M, N, device=DEV)
            dx0 = dx_prev.clone() if accumulate else torch.empty(M, N, device=DEV)
            db = torch.zeros(N, device=DEV)                    # (column sums are ADDED: the caller's zero fill)
            dgs = torch.empty(M, device=DEV) if mix else None
            _lib.check(lib.mi_cross_bwd_head(g.data_ptr(), x0.data_ptr(), lin.data_ptr(), gate.data_ptr() if mix else None, 4,
                                             b.data_ptr() if mix else None, dlin.data_ptr(), dx0.data_ptr(), accumulate,
                                             db.data_ptr(), _lib.ptr(dgs), M, N, _lib.stream_ptr(dlin.device)), "mi_cross_bwd_head")
            out.update({f"acc{accumulate}/dlin": dlin, f"acc{accumulate}/dx0": dx0, f"acc{accumulate}/db": db})
            if mix:
                out[f"acc{accumulate}/dgs"] = dgs
        return out

    def check(result):
        g, x0, lin, b, gate, dx_prev = (t.double() for t in operands())
        dlin = g * x0
        rs = gate.sum(1, keepdim=True) if mix else torch.ones(M, 1, dtype=torch.float64)
        for acc in (0, 1):
            want = {"dlin": dlin, "dx0": (dx_prev if acc else 0) + g * lin, "db": (dlin * rs).sum(0)}
            if mix:
                want["dgs"] = dlin @ b
            for k, v in want.items():
                assert torch.equal(result[f"acc{acc}/{k}"].cpu().double(), v), f"acc{acc}/{k}"

    return Case(f"cross_bwd_head-M{M}-N{N}-{'mix' if mix else 'plain'}", run, check, True)


def _mix_expert_case(M, d, E, r):
    """mi_mix_expert_fwd / _bwd on torch.empty outputs against the chain in float64, tolerance for tolerance
    test_mix_expert_kernels_vs_float64 (activations 2e-5 / 2e-6, dgate 1e-4 / 1e-5 sqrt(d), dZ 1e-4 / 1e-5).  No atomics."""
    def operands():
        gen = torch.Generator().manual_seed(M + d + E + r)
        R = lambda *sh: torch.randn(*sh, generator=gen)                                  # noqa: E731
        x, dT, gate, dgs = R(M, d) * 0.5, R(M, d), R(M, E), R(M)
        return x, dT, gate, dgs, R(E, d, r) / d ** 0.5, R(E, r, r) / r ** 0.5, R(E, r, d) / r ** 0.5

    def run():
        from recsys_benchmark_amd import _lib

        x, dT, gate, dgs, V, C, U = (t.to(DEV) for t in operands())
        lib, st = _lib.load(), _lib.stream_ptr(torch.device(DEV, 0))
        H1, H2, H2g = (torch.empty(M, E * r, device=DEV) for _ in range(3))
        _lib.check(lib.mi_mix_expert_fwd(x.data_ptr(), V.data_ptr(), C.data_ptr(), gate.data_ptr(), H1.data_ptr(), H2.data_ptr(),
                                         H2g.data_ptr(), M, d, E, r, st), "mi_mix_expert_fwd")
        dgate, dZ2, dZ1 = torch.empty(M, E, device=DEV), torch.empty(M, E * r, device=DEV), torch.empty(M, E * r, device=DEV)
        _lib.check(lib.mi_mix_expert_bwd(dT.data_ptr(), U.data_ptr(), C.data_ptr(), gate.data_ptr(), H1.data_ptr(), H2.data_ptr(),
                                         dgs.data_ptr(), dgate.data_ptr(), dZ2.data_ptr(), dZ1.data_ptr(), M, d, E, r, st),
                   "mi_mix_expert_bwd")
        return dict(H1=H1, H2=H2, H2g=H2g, dgate=dgate, dZ2=dZ2, dZ1=dZ1)

    def check(result):
        from conftest import assert_close

        x, dT, gate, dgs, V, C, U = (t.double() for t in operands())
        h1 = torch.tanh(torch.einsum("md,edr->mer", x, V))
        h2 = torch.tanh(torch.einsum("mek,ekc->mec", h1, C))
        assert_close(result["H1"].view(M, E, r), h1, 2e-5, 2e-6, "H1")
        assert_close(result["H2"].view(M, E, r), h2, 2e-5, 2e-6, "H2")
        assert_close(result["H2g"].view(M, E, r), h2 * gate[:, :, None], 2e-5, 2e-6, "H2g")
        h1f, h2f = result["H1"].view(M, E, r).double().cpu(), result["H2"].view(M, E, r).double().cpu()
        dh = torch.einsum("md,erd->mer", dT, U)
        assert_close(result["dgate"], (dh * h2f).sum(2) + dgs[:, None], 1e-4, 1e-5 * d ** 0.5, "dgate")
        dz2 = dh * gate[:, :, None] * (1 - h2f * h2f)
        assert_close(result["dZ2"].view(M, E, r), dz2, 1e-4, 1e-5, "dZ2")
        assert_close(result["dZ1"].view(M, E, r), torch.einsum("mek,eck->mec", dz2, C) * (1 - h1f * h1f), 1e-4, 1e-5, "dZ1")

    return Case(f"mix_expert-M{M}-d{d}-E{E}-r{r}", run, check, True)


def _slot_deepfm_case(labels, B=33, F=5, D=16):
    """tail.run_fused_slot_deepfm, the sharded step's local node, on a hand-built receive buffer (one lookup per slot, unused
    slots, one lookup on the dump row), the way ShardedDeepFM._fused_local calls it: the logits and every gradient against
    the torch restatement of the slot lookup (oracle TorchOps.slot_fm) followed by the stock modules in float64, at
    smoke()'s DeepFM-step tolerances (logits 1e-4 / 1e-5, row gradients 1e-4 / 1e-6, MLP weights 2e-4 / 1e-6)."""
    def build():
        import test_tail_gpu as tt

        g = torch.Generator().manual_seed(B + F + D)
        S = B * F + 11
        slot = torch.randperm(S, generator=g)[:B * F].view(B, F)
        slot[0, 0] = S
        buf = torch.randn(S + 1, D + 4, generator=g) * 0.1
        buf[:, D + 1:] = 0
        buf[S] = 0
        torch.manual_seed(B + F)
        seq = tt._seq(F * D, [32, 24], 0.0, bn=True).train()
        return S, buf, slot, torch.tensor([0.3]), seq, (torch.rand(B, generator=g) < 0.3).float(), torch.randn(B, generator=g)

    def run():
        from recsys_benchmark_amd import _lib, mlp, tail
        from recsys_benchmark_amd.losses import BCEWithLogitsLoss, unit_scalar

        S, buf, slot, bias, seq, y, G = build()
        seq = copy.deepcopy(seq).to(DEV)
        recv, hbias = buf.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
        with _patched((mlp, "FUSED_TAIL", True)):
            groups = mlp._groups(seq)
            plan = tail.fused_tail_plan(seq, tail._InputSpec(B, F * D, recv.device), groups)
            assert plan is not None, "the fused node must take this pattern"
            yd = y.to(DEV)
            logits = tail.run_fused_slot_deepfm(plan, groups[-1][1], mlp._seed_word(recv.device), recv, slot.to(DEV), hbias,
                                                yd if labels else None, None).squeeze(-1)
            if labels:
                loss = BCEWithLogitsLoss()(logits, yd)
                loss.backward(unit_scalar(DEV))
            else:
                (logits * G.to(DEV)).sum().backward()
        _lib.check_index_errors()
        out = dict(logits=logits.detach(), grecv=recv.grad, gbias=hbias.grad, **_module_grads(seq))
        if labels:
            out["loss"] = loss.detach()
        return out

    cache = {}

    def check(result):
        from conftest import assert_close
        from oracle.sharded_ops import TorchOps

        S, buf, slot, bias, seq, y, G = build()
        if "ref" not in cache:
            seq64 = copy.deepcopy(seq).double()
            rb, rbias = buf.double().requires_grad_(True), bias.double().requires_grad_(True)
            emb, yfm = TorchOps.slot_fm(rb, slot, rbias)
            logits = (seq64(emb.reshape(B, -1)) + yfm.view(-1, 1)).squeeze(-1)
            loss = torch.nn.BCEWithLogitsLoss()(logits, y.double()) if labels else (logits * G.double()).sum()
            loss.backward()
            cache["ref"] = (logits.detach(), loss.detach(), rb.grad, rbias.grad, seq64)
        logits, loss, grecv, gbias, seq64 = cache["ref"]
        assert_close(result["logits"], logits.float(), 1e-4, 1e-5, "logits")
        if labels:
            assert_close(result["loss"], loss.float(), 1e-5, 1e-6, "loss")
        assert_close(result["grecv"][:S, :D + 1], grecv[:S, :D + 1].float(), 1e-4, 1e-6, "gradient rows")
        assert not result["grecv"][:S, D + 1:].any(), "the padding columns travel back as zeros"
        assert_close(result["gbias"], gbias.float(), 1e-4, 1e-6, "bias gradient")
        for k, q in seq64.named_parameters():
            if k.endswith("weight") and q.dim() == 2:
                assert_close(result["g/" + k], q.grad.float(), 2e-4, 1e-6, k)

    return Case(f"slot_deepfm-fused-{'labels' if labels else 'nolabels'}-B{B}-F{F}-D{D}", run, check)


# ---- sixth batch: the CrossNet fallbacks (tests/test_dcn_dispatch_gpu.py) ------------------------------------------------------
def _cross_helper_cases():
    """mi_cross_bwd_pre, mi_colsum (the gate as rowscale with nrs = 3, and rs_sum), mi_rowdot, mi_outer and mi_mix_gate_bwd
    through the C-ABI on outputs from torch.empty (NaN under poison): the passes layer_dcn.py falls back to write everything
    they own.  Integer-valued data against the formulas in float64, bit-exact as in test_dcn_dispatch_gpu.py (mi_outer: one
    rounded multiply per element against the float32 product)."""
    def ints(gen, *sh):
        return torch.randint(-3, 4, sh, generator=gen).float()

    def case(name, operands, launch, reference):
        def run():
            from recsys_benchmark_amd import _lib

            t = {k: v.to(DEV) for k, v in operands().items()}
            return launch(_lib, _lib.load(), _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device())), t)

        def check(result):
            want = reference({k: v.double() for k, v in operands().items()})
            assert set(want) == set(result), f"{name}: returned {sorted(result)} vs reference {sorted(want)}"
            for k, v in want.items():
                assert torch.equal(result[k].cpu().double(), v), f"{name}: {k}"

        return Case(name, run, check, True)

    def pre_ops(n=524288 + 259):
        gen = torch.Generator().manual_seed(n)
        return dict(g=ints(gen, n), x0=ints(gen, n), lin=ints(gen, n), prev=ints(gen, n))

    def pre_launch(_lib, lib, st, t):
        out, n = {}, t["g"].numel()
        for acc in (0, 1):
            dlin = torch.empty(n, device=DEV)
            dx0 = t["prev"].clone() if acc else torch.empty(n, device=DEV)
            _lib.check(lib.mi_cross_bwd_pre(t["g"].data_ptr(), t["x0"].data_ptr(), t["lin"].data_ptr(), dlin.data_ptr(), dx0.data_ptr(),
                                            n, acc, st), "mi_cross_bwd_pre")
            out.update({f"acc{acc}/dlin": dlin, f"acc{acc}/dx0": dx0})
        return out

    def pre_ref(t):
        out = {}
        for acc in (0, 1):
            out.update({f"acc{acc}/dlin": t["g"] * t["x0"], f"acc{acc}/dx0": (t["prev"] if acc else 0) + t["g"] * t["lin"]})
        return out

    M, N, ldx, nrs = 257, 65, 70, 3

    def colsum_ops():
        gen = torch.Generator().manual_seed(M + N)
        return dict(X=ints(gen, M, ldx), gate=ints(gen, M, nrs))

    def colsum_launch(_lib, lib, st, t):
        out, rs_sum = torch.zeros(N, device=DEV), torch.zeros(1, device=DEV)       # (both ADDED into: the caller's zero fill)
        _lib.check(lib.mi_colsum(t["X"].data_ptr(), ldx, t["gate"].data_ptr(), nrs, out.data_ptr(), rs_sum.data_ptr(), M, N, st),
                   "mi_colsum")
        return dict(out=out, rs_sum=rs_sum)

    def colsum_ref(t):
        rs = t["gate"].sum(1)
        return dict(out=(t["X"][:, :N] * rs[:, None]).sum(0), rs_sum=rs.sum().view(1))

    Mr, Nr, ldr = 130, 65, 72

    def rowdot_ops():
        gen = torch.Generator().manual_seed(Mr + Nr)
        return dict(X=ints(gen, Mr, ldr), v=ints(gen, Nr), bias=ints(gen, 1), addend=ints(gen, Mr))

    def rowdot_launch(_lib, lib, st, t):
        plain, full = torch.empty(Mr, device=DEV), torch.empty(Mr, device=DEV)
        _lib.check(lib.mi_rowdot(t["X"].data_ptr(), ldr, t["v"].data_ptr(), None, None, plain.data_ptr(), Mr, Nr, st), "mi_rowdot")
        _lib.check(lib.mi_rowdot(t["X"].data_ptr(), ldr, t["v"].data_ptr(), t["bias"].data_ptr(), t["addend"].data_ptr(),
                                 full.data_ptr(), Mr, Nr, st), "mi_rowdot")
        return dict(plain=plain, full=full)

    def rowdot_ref(t):
        base = t["X"][:, :Nr] @ t["v"]
        return dict(plain=base, full=base + t["bias"] + t["addend"])

    def outer_ops():
        gen = torch.Generator().manual_seed(70 + 1028)
        return dict(g=torch.randn(70, generator=gen), w=torch.randn(1028, generator=gen), g2=torch.randn(7, generator=gen),
                    w2=torch.randn(5, generator=gen))

    def outer_launch(_lib, lib, st, t):
        wide, odd = torch.empty(70, 1028, device=DEV), torch.empty(7, 5, device=DEV)
        _lib.check(lib.mi_outer(t["g"].data_ptr(), t["w"].data_ptr(), wide.data_ptr(), 70, 1028, st), "mi_outer")
        _lib.check(lib.mi_outer(t["g2"].data_ptr(), t["w2"].data_ptr(), odd.data_ptr(), 7, 5, st), "mi_outer")
        return dict(wide=wide, odd=odd)

    def outer_ref(t):      # (the float32 product, exactly: float32 x float32 is exact in float64, rounded once on the way back)
        return dict(wide=(t["g"][:, None] * t["w"][None]).float().double(), odd=(t["g2"][:, None] * t["w2"][None]).float().double())

    Mg, Eg, rg = 130, 2, 80

    def gate_ops():
        gen = torch.Generator().manual_seed(Mg + Eg + rg)
        return dict(dH=ints(gen, Mg, Eg * rg), H2=ints(gen, Mg, Eg * rg), gate=ints(gen, Mg, Eg), dgs=ints(gen, Mg))

    def gate_launch(_lib, lib, st, t):
        dgate, dZ2 = torch.empty(Mg, Eg, device=DEV), torch.empty(Mg, Eg * rg, device=DEV)
        _lib.check(lib.mi_mix_gate_bwd(t["dH"].data_ptr(), t["H2"].data_ptr(), t["gate"].data_ptr(), t["dgs"].data_ptr(),
                                       dgate.data_ptr(), dZ2.data_ptr(), Mg, Eg, rg, st), "mi_mix_gate_bwd")
        return dict(dgate=dgate, dZ2=dZ2)

    def gate_ref(t):
        dh, h = t["dH"].view(Mg, Eg, rg), t["H2"].view(Mg, Eg, rg)
        return dict(dgate=(dh * h).sum(2) + t["dgs"][:, None], dZ2=(dh * t["gate"][:, :, None] * (1 - h * h)).view(Mg, Eg * rg))

    return [case("cross_bwd_pre-n524547", pre_ops, pre_launch, pre_ref),
            case(f"colsum-gate-M{M}-N{N}-nrs{nrs}-rs_sum", colsum_ops, colsum_launch, colsum_ref),
            case(f"rowdot-M{Mr}-N{Nr}", rowdot_ops, rowdot_launch, rowdot_ref),
            case("outer-70x1028-7x5", outer_ops, outer_launch, outer_ref),
            case(f"mix_gate_bwd-M{Mg}-E{Eg}-r{rg}", gate_ops, gate_launch, gate_ref)]


def _build6():
    # (heads whose every layer runs on the fallbacks: odd d, d > 1024, no fused experts, the gate product as a GEMM)
    return [_dcn_head_case(33, 22, 2), _dcn_head_case(5, 1030, 1), _dcn_mix_case(50, 22, 3, 16, 2),
            _dcn_mix_case(20, 40, 9, 8, 2)] + _cross_helper_cases()


def _build5():
    cases = []
    for F, D in ((3, 4), (26, 16), (39, 16), (70, 8)):          # (pack_tables() covers D in {4, 8, 16})
        for B in FM_BATCHES:
            cases += _plain_fm_case(F, D, B, masked=False, packed=True) + _plain_fm_case(F, D, B, masked=True, packed=True)
    cases += [_deepfm_case(True, True, "sums", packed=True), _deepfm_case(False, True, "finalize", packed=True),
              _deepfm_case(False, False, packed=True)]
    cases += [_cross_bwd_head_case(M, N, mix) for M, N in ((257, 260), (1, 4)) for mix in (True, False)]
    cases += [_mix_expert_case(1, 4, 4, 16), _mix_expert_case(200, 40, 3, 16)]
    cases += [_dcn_mix_case(1, 4, 4, 16, 1), _dcn_mix_case(200, 40, 3, 16, 2)]          # (rank 16: the fused expert launches)
    cases += [_slot_deepfm_case(True), _slot_deepfm_case(False)]
    return cases


# ---------------------------------------------------------------------------------------------------------------- the list
def _build():
    cases = []
    for F, D in FD_SHAPES:
        for B in FM_BATCHES:
            cases += _plain_fm_case(F, D, B, masked=False) + _plain_fm_case(F, D, B, masked=True)
            cases += [_soft_case(F, D, B, kind) for kind in ("global", "dimension", "feature", "feature_dim")]
            cases.append(_mask_case(F, D, B))
        for kind, geo in (("mult", 3), ("mult", None), ("add", 3), ("add", None), ("soft", 7), ("mask", 7)):
            cases.append(_dual_fm_case(F, D, 37, kind, geo))
    for op in ("mult", "add", "cat"):
        cases += [_dual_gather_case(op, v) for v in ("plain", "sparse2", "fields", "offsets", "sparse2+offsets", "sparse2+fields")]
    cases += [_dual_gather_case("add", "sparse2", D=12), _dual_gather_case("add", "sparse2", D=16, div=7)]
    cases += [_alignment_case(n1) for n1 in (1, 2, 3, 4)] + [_alignment_case(3, aligned=True)]
    for N, D, bucket in ((37, 8, 12), (5000, 16, 1700)):
        for kind, op, divider in (("qr", "mult", 2), ("qr", "add", 5), ("qr", "cat", 2), ("soft", "add", None), ("mask", "add", None)):
            cases.append(_dual_table_case(kind, op, divider, N, D, bucket))
    for M, N, K in GEMM_SHAPES:
        for tA, tB in TRANSPOSES:
            cases += [_gemm_case(M, N, K, tA, tB, form) for form in ("one", "splitk", "multi", "multi-splitk")]
        cases += [_gemm_panel_case(M, N, K, layout) for layout in (0, 1)]
    cases += [_gemm_epilogue_case(1), _gemm_epilogue_case(2)]
    for armed in (True, False):
        for B in LOSS_BATCHES:
            for D in LOSS_WIDTHS:
                cases += _loss_cases(B, D, armed)
        for n in LOSS_BATCHES:
            for D in LOSS_WIDTHS:
                cases += _info_nce_cases(n, D, armed)
                cases.append(_cerp_prune_case(n, D, 100 if D == 7 else 1, armed))
        cases.append(_cerp_prune_case(333, 12, 1, armed))          # (float4 loads, n * D no multiple of a workgroup's elements)
    for D in PROP_WIDTHS:
        cases.append(_spmm_case(D))
        for L in PROP_LAYERS:
            cases.append(_hccf_case(D, L))
            cases += [_lightgcn_case(D, L, form) for form in ("row-per-wave", "tiled", "unmasked")]
    for N, D, n in ((50, 16, 2000), (300, 7, 500), (5, 8, 1)):
        cases += [_sparse_adam_case(N, D, n, cap) for cap in (False, True)]
        cases.append(_coalesce_case(N, D, n))
    cases += [_dense_adam_case(0.0), _dense_adam_case(1e-3)]
    for M, K, hidden, p in TAIL_CASES:
        for mode in TAIL_MODES:
            cases += [_tail_case(M, K, hidden, p, mode, True), _tail_case(M, K, hidden, p, mode, False)]
    cases += [_deepfm_case(labels, fused) for labels in (True, False) for fused in (True, False)]
    cases += [_auc_case(n) for n in (3, 257, 4097)]
    cases += [_gather_quant_case(q) for q in ("fp16", "int8", "int16")]
    cases += _build2() + _build3() + _build4() + _build5() + _build6()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), "duplicate case names"
    return cases


CASES = _build()

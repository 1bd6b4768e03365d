"""CPU: the shared glue of the two-table lookups (QR, CERP, CERP retrain) — the form rule of the row-form backward that the
library owns (mi_dual_gather_bwd_rows_form: it takes addresses and dereferences none, so plain integers do) and the
operand preparation every launch of the family goes through (_kernels._dual_operands)."""
import os
import re

import pytest
import torch

from recsys_benchmark_amd import _kernels, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMENT, ATOMIC, WORKSPACE = 0, 1, 2
G, T1, T2, V, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # 16-byte aligned "addresses"


def _form(De, n1, g=G, t1=T1, t2=T2, vals=V, ws=WS):
    return _lib.load().mi_dual_gather_bwd_rows_form(g, t1, t2, vals, ws, De, n1)


def test_the_header_names_the_three_forms_and_python_the_one_that_writes():
    text = open(os.path.join(ROOT, "include", "mi355x_recsys.h")).read()
    named = {k: int(v) for k, v in re.findall(r"#define MI_DUAL_ROWS_FORM_(\w+) (\d+)", text)}
    assert named == {"ELEMENT": ELEMENT, "ATOMIC": ATOMIC, "WORKSPACE": WORKSPACE}
    assert _kernels.DUAL_ROWS_FORM_WORKSPACE == WORKSPACE


def test_form_truth_table():
    assert _form(16, 2) == WORKSPACE
    assert _form(16, 2, ws=None) == ATOMIC
    assert _form(16, 3) == ATOMIC                 # 48 sums do not tile the workgroup: the workspace is unusable
    for name in ("g", "t1", "t2", "vals"):        # any one operand 4 bytes past alignment: the element kernel
        at = dict(g=G, t1=T1, t2=T2, vals=V)[name] + 4
        assert _form(16, 2, **{name: at}) == ELEMENT, name
    assert _form(12, 2) == ELEMENT                # rows of three float4: no power of two
    assert _form(16, 5) == ELEMENT                # more rows of table 1 than the register form keeps
    assert _form(260, 2) == ELEMENT
    assert _form(16, 2, ws=WS + 4) == WORKSPACE   # (the workspace is read by words: its alignment is not asked for)
    assert _form(0, 2) == _form(16, 0) == _form(-4, 2) == ELEMENT


def test_form_agrees_with_the_exports_that_keep_their_prototypes():
    lib = _lib.load()
    seen = set()
    for De in range(1, 261):
        for n1 in range(1, 6):
            form = _form(De, n1)
            seen.add(form)
            assert (form == WORKSPACE) == (lib.mi_dual_gather_bwd_rows_overwrites(De, n1) != 0), (De, n1)
            if form == WORKSPACE:
                assert lib.mi_dual_gather_bwd_rows_workspace_elems(De, n1) > 0, (De, n1)
            if form == ELEMENT:
                assert _form(De, n1, ws=None) == ELEMENT
            else:
                assert _form(De, n1, ws=None) == ATOMIC and _form(De, n1, g=G + 4) == ELEMENT
    assert seen == {ELEMENT, ATOMIC, WORKSPACE}


# ---- _dual_operands ------------------------------------------------------------------------------------------------------
N1, N2, DE = 3, 5, 4


def _tables():
    return torch.arange(N1 * DE, dtype=torch.float32).view(N1, DE), torch.zeros(N2, DE)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_dual_operands_read_a_byte_mask_in_place(dtype):
    A, B = _tables()
    M1, M2 = (A > 4).to(dtype), torch.ones(N2, DE, dtype=dtype)
    T1c, T2c, S1c, S2c, M1c, M2c, xform, De, n1, n2 = _kernels._dual_operands(A, B, None, None, M1, M2)
    assert (M1c.data_ptr(), M2c.data_ptr()) == (M1.data_ptr(), M2.data_ptr()), "a one-byte mask was copied"
    assert M1c.dtype == M2c.dtype == torch.uint8 and torch.equal(M1c, (A > 4).to(torch.uint8))
    assert (T1c.data_ptr(), T2c.data_ptr()) == (A.data_ptr(), B.data_ptr()) and S1c is None and S2c is None
    assert (xform, De, n1, n2) == (_kernels.XF_MASK, DE, N1, N2)


def test_dual_operands_convert_a_mask_of_any_other_dtype():
    A, B = _tables()
    M1 = (A > 4).float()
    M1c, M2c = _kernels._dual_operands(A, B, None, None, M1, torch.ones(N2, DE, dtype=torch.int64))[4:6]
    assert M1c.dtype == M2c.dtype == torch.uint8 and torch.equal(M1c, (A > 4).to(torch.uint8)) and bool(M2c.all())


def test_dual_operands_make_tables_thresholds_and_masks_contiguous():
    wide = torch.arange(N1 * 2 * DE, dtype=torch.float32).view(N1, 2 * DE)
    A, B = wide[:, ::2], _tables()[1]
    S1, S2 = wide[:, 1::2], torch.ones(N2, DE)
    T1c, T2c, S1c, S2c, M1c, M2c, xform, De, n1, n2 = _kernels._dual_operands(A, B, S1, S2, None, None)
    assert not A.is_contiguous() and T1c.is_contiguous() and torch.equal(T1c, A) and T2c.data_ptr() == B.data_ptr()
    assert S1c.is_contiguous() and torch.equal(S1c, S1) and S2c.data_ptr() == S2.data_ptr() and M1c is None and M2c is None
    assert (xform, De, n1, n2) == (_kernels.XF_SOFT, DE, N1, N2)
    mask_t = (wide > 3)[:, ::2]
    assert not mask_t.is_contiguous()
    M1c = _kernels._dual_operands(A, B, None, None, mask_t, torch.ones(N2, DE, dtype=torch.bool))[4]
    assert M1c.is_contiguous() and M1c.dtype == torch.uint8 and torch.equal(M1c.bool(), mask_t)
    assert _kernels._dual_operands(A, B, None, None, None, None)[6:] == (_kernels.XF_NONE, DE, N1, N2)


def test_dual_operands_refuse_what_gather_fm_dual_refuses():
    A, B = _tables()
    S1, S2 = torch.zeros(N1, DE), torch.zeros(N2, DE)
    M1, M2 = torch.ones(N1, DE, dtype=torch.bool), torch.ones(N2, DE, dtype=torch.bool)
    for args in ((S1, None, None, None), (None, S2, None, None), (None, None, M1, None), (None, None, None, M2)):
        with pytest.raises(ValueError, match="come in pairs"):
            _kernels._dual_operands(A, B, *args)
    with pytest.raises(ValueError, match="exclude each other"):
        _kernels._dual_operands(A, B, S1, S2, M1, M2)
    for args in ((S1[:2], S2, None, None), (S1, S2[:, :2], None, None), (None, None, M1, M2[:3]), (None, None, M1.view(-1), M2)):
        with pytest.raises(ValueError, match="shaped like its table"):
            _kernels._dual_operands(A, B, *args)
    for other in (torch.zeros(N2, DE + 4), torch.zeros(N2 * DE), torch.zeros(1, N2, DE)):
        with pytest.raises(ValueError, match="share the row width"):
            _kernels._dual_operands(A, other, None, None, None, None)
    with pytest.raises(ValueError, match="^gather_fm_dual: "):
        _kernels._dual_operands(A, B, S1, None, None, None, "gather_fm_dual")
    with pytest.raises(TypeError):
        _kernels._dual_operands(A.double(), B, None, None, None, None)
    with pytest.raises(TypeError):
        _kernels._dual_operands(A, B, S1.half(), S2, None, None)


# ---- the entry points' shared argument checks ------------------------------------------------------------------------------
# (every call below is refused, or has n == 0, before anything is read or launched: plain integers stand for addresses)
P = 0x1000
SIZES = dict(n=8, F=2, De=4, n1=3, n2=5, mod1=3, div2=3)


def _fwd(op=1, xform=0, idx=P, T1=P, T2=P, S=(None, None), M=(None, None), out=P, **sizes):
    s = dict(SIZES, **sizes)
    return _lib.load().mi_dual_gather_fwd_off(idx, None, None, T1, T2, *S, *M, out, *s.values(), op, xform, None, None)


def _rows(op=1, idx=P, g=P, T1=P, T2=P, gT1=P, vals=P, rows2=P, **sizes):
    s = dict(SIZES, **sizes)
    return _lib.load().mi_dual_gather_bwd_rows(idx, g, T1, T2, gT1, vals, rows2, *s.values(), op, None, None)


def _fields(op=1, xform=0, idx=P, g=P, T1=P, T2=P, S=(None, None), M=(None, None), gT=(P, P), gS=(None, None), **sizes):
    s = dict(SIZES, **sizes)
    return _lib.load().mi_dual_gather_bwd_fields(idx, g, T1, T2, *S, *M, *gT, *gS, *s.values(), op, xform, None, 0, None, None, None)


@pytest.mark.parametrize("entry", [_fwd, _rows, _fields], ids=["fwd_off", "bwd_rows", "bwd_fields"])
def test_entry_points_refuse_the_same_arguments_with_the_same_codes(entry):
    OK, INVALID = 0, -1
    for name in SIZES:
        assert entry(**{name: -1}) == INVALID, name
        if name != "n":
            assert entry(**{name: 0}) == INVALID, name
    assert entry(op=-1) == entry(op=3) == INVALID
    assert entry(n=0, idx=None, T1=None, T2=None) == OK              # no lookup: nothing is asked of the operands
    assert entry(n=0, op=3) == INVALID                               # ... but the enums are still checked
    for name in ("idx", "T1", "T2"):
        assert entry(**{name: None}) == INVALID, name
    if entry is _rows:
        for name in ("g", "gT1", "vals", "rows2"):
            assert entry(**{name: None}) == INVALID, name
        return
    assert entry(xform=-1) == entry(xform=3) == entry(n=0, xform=3) == INVALID
    assert entry(xform=1) == entry(xform=1, S=(P, None)) == entry(xform=1, S=(None, P)) == INVALID
    assert entry(xform=2) == entry(xform=2, M=(P, None)) == entry(xform=2, M=(None, P)) == INVALID
    if entry is _fwd:
        assert entry(out=None) == INVALID
        assert entry(op=2, n=7) == INVALID                            # cat: whole [B, F] rows only
    else:
        assert entry(g=None) == entry(gT=(None, P)) == entry(gT=(P, None)) == INVALID
        assert entry(xform=1, S=(P, P)) == entry(xform=1, S=(P, P), gS=(P, None)) == INVALID      # soft: its gradients too

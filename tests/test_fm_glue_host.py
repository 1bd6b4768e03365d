"""CPU: the shared glue of the fused FM lookups — the operand preparation every launch goes through
(_kernels._lookup_operands) and the one dispatch hook DeepFM asks its table for (IEmbedding.fm_lookup)."""
import pytest
import torch

import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import _kernels
from recsys_benchmark_amd.embeddings.base import IEmbedding, VanillaEmbedding

N, F = 12, 3


def _ids(dtype=torch.int64):
    return torch.arange(2 * F, dtype=dtype).view(2, F)


def test_lookup_operands_promote_the_ids_and_take_offsets_in_either_shape_or_none():
    w1 = torch.zeros(N, 1)
    idx, offsets, _w1c, _ld, n = _kernels._lookup_operands(_ids(torch.int32), None, w1)
    assert idx.dtype == torch.int64 and idx.is_contiguous() and torch.equal(idx, _ids()) and offsets is None and n == N
    for off in (torch.tensor([0, 4, 8]), torch.tensor([[0, 4, 8]]), torch.tensor([0, 4, 8], dtype=torch.int32)):
        idx, offsets, _w1c, _ld, n = _kernels._lookup_operands(_ids(), off, w1, N)
        assert offsets.dtype == torch.int64 and tuple(offsets.shape) == (F,) and offsets.tolist() == [0, 4, 8] and n == N


def test_lookup_operands_read_a_packed_first_order_column_in_place():
    packed = torch.zeros(N, 32)
    w1 = packed[:, 8:9]
    _idx, _off, w1c, ldw1, n = _kernels._lookup_operands(_ids(), None, w1, N)
    assert w1.stride(0) == 32 and ldw1 == 32 and n == N
    assert w1c.data_ptr() == w1.data_ptr() == packed.data_ptr() + 4 * 8, "the packed column was copied"


@pytest.mark.parametrize("shape", [(N,), (N, 1)])
def test_lookup_operands_of_a_plain_first_order_table(shape):
    w1 = torch.arange(N, dtype=torch.float32).view(shape)
    for given in (None, N):
        _idx, _off, w1c, ldw1, n = _kernels._lookup_operands(_ids(), None, w1, given)
        assert ldw1 == 1 and n == N and w1c.reshape(-1).tolist() == list(range(N))


def test_lookup_operands_refuse_wrong_counts_and_types():
    w1 = torch.zeros(N, 1)
    with pytest.raises(ValueError):          # one offset too few for the fields of idx
        _kernels._lookup_operands(_ids(), torch.tensor([0, 4]), w1, N)
    with pytest.raises(ValueError):          # ids that are not [B, F]
        _kernels._lookup_operands(_ids().view(-1), None, w1, N)
    with pytest.raises(ValueError):          # a first-order table of another row count than the embedding table
        _kernels._lookup_operands(_ids(), None, w1, N + 1)
    with pytest.raises(ValueError):          # more than one weight per row
        _kernels._lookup_operands(_ids(), None, torch.zeros(N, 2), N)
    with pytest.raises(TypeError):
        _kernels._lookup_operands(_ids().float(), None, w1, N)
    with pytest.raises(TypeError):
        _kernels._lookup_operands(_ids(), torch.tensor([0.0, 4.0, 8.0]), w1, N)
    with pytest.raises(TypeError):
        _kernels._lookup_operands(_ids(), None, w1.double(), N)


# ---- the dispatch hook ---------------------------------------------------------------------------------------------------
class _SentinelTable(IEmbedding):
    """A table family DeepFM has never heard of: its fm_lookup answers, so DeepFM must not look further."""

    def __init__(self):
        super().__init__()
        self.seen = None

    def get_weight(self):
        raise AssertionError("the fused answer was given: nothing else of the table is asked")

    forward = get_weight

    def fm_lookup(self, x, offsets, w1, bias, sparse_w1):
        self.seen = (x, offsets, w1, bias, sparse_w1)
        return "emb", "y_fm"


def _model(**kw):
    return pkg.DeepFM([5, 3, 4], 4, [8], p_dropout=0.0, **kw)


@pytest.mark.parametrize("fc_sparse", [False, True])
def test_a_new_table_family_is_served_through_its_hook_alone(fc_sparse):
    m = _model(fc_sparse=fc_sparse)
    m.embedding = _SentinelTable()
    x = torch.zeros(2, 3, dtype=torch.int64)
    assert m._fm_and_embedding(x) == ("emb", "y_fm")
    got = m.embedding.seen
    assert got[0] is x and got[1] is m.offsets and got[2] is m.fc.weight and got[3] is m._bias and got[4] is fc_sparse


def test_the_default_hook_declines_and_the_module_is_called():
    class Declines(IEmbedding):
        def get_weight(self):
            return None

        def forward(self, rows):
            raise RuntimeError(f"forward was called with {rows.tolist()}")

    assert Declines().fm_lookup(None, None, None, None, False) is None
    m = _model()
    m.embedding = Declines()
    with pytest.raises(RuntimeError, match=r"forward was called with \[\[0, 5, 8\]\]"):      # x + offsets
        m._fm_and_embedding(torch.zeros(1, 3, dtype=torch.int64))


def test_a_vanilla_subclass_that_transforms_its_rows_is_not_given_the_plain_launch(monkeypatch):
    class Doubled(VanillaEmbedding):
        def forward(self, x):
            raise RuntimeError("the subclass's own forward")

    launched = []
    monkeypatch.setattr(_kernels, "gather_fm", lambda *a, **k: launched.append(k) or ("emb", "y_fm"))
    m = _model()
    assert type(m.embedding) is VanillaEmbedding
    assert m._fm_and_embedding(torch.zeros(1, 3, dtype=torch.int64)) == ("emb", "y_fm")
    assert launched == [dict(sparse_W=False, sparse_w1=False)]
    m.embedding = Doubled([5, 3, 4], 4)
    assert m.embedding.fm_lookup(None, None, None, None, False) is None
    with pytest.raises(RuntimeError, match="own forward"):
        m._fm_and_embedding(torch.zeros(1, 3, dtype=torch.int64))
    assert len(launched) == 1
    bag = VanillaEmbedding([5, 3, 4], 4, mode="sum")          # a bag mode keeps forward() too
    assert bag.fm_lookup(None, None, None, None, False) is None

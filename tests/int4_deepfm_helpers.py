"""What the packed-int4 tests share (host and GPU): the four tables of the 4-bit checks, the reference's quantisation
arithmetic restated, and the packed layout written out independently of the package (plain loops over Python ints)."""
import torch

from quant_deepfm_helpers import ptq_rows32  # noqa: F401  (the dequantised rows as the library defines them)

# name -> (least value, greatest value, the zero point the reference's arithmetic gives at 4 bits)
TABLES = {
    "symmetric": (-0.1, 0.0999968, 0),      # codes span [-8, 7], nothing clamps: the case of the existing int4 tests
    "unit": (0.0, 1.0, -8),
    "negative": (-1.0, -0.25, 12),          # a zero point outside the nibble range: it stays an int8 scalar
    "clamped": (-0.095, 0.105, 0),          # the unclamped codes reach 8: the clamp acts
}
TABLE_NAMES = list(TABLES)


def make_table(name: str, N: int, D: int, seed: int = 0) -> torch.Tensor:
    """fp32 [N, D], uniform between the table's extremes, which are planted at W[0, 0] and W[N-1, D-1]."""
    lo, hi, _ = TABLES[name]
    gen = torch.Generator().manual_seed(977 * TABLE_NAMES.index(name) + 31 * N + D + seed)
    u = torch.rand(N, D, generator=gen) * 0.98 + 0.01
    W = torch.tensor(lo) + u * (torch.tensor(hi) - torch.tensor(lo))
    W = W.clamp(lo, hi)
    W[0, 0], W[N - 1, D - 1] = lo, hi
    return W


def reference_codes(W: torch.Tensor, n_bits: int):
    """(codes, scale, zero point, codes before the clamp) by src/models/embeddings/ptq_emb.py:64-83, restated."""
    q_min, q_max = -(1 << (n_bits - 1)), (1 << (n_bits - 1)) - 1
    r_min = W.min().cpu()
    scale = (W.max().item() - r_min) / (q_max - q_min)
    dtype = torch.int16 if n_bits == 16 else torch.int8
    bias = (q_min - r_min / scale).to(dtype)
    raw = torch.round(W / scale + bias)
    weight = raw.clamp(q_min, q_max) if n_bits < 8 else raw
    return weight.to(dtype), scale, bias, raw


def check_table(name: str, W: torch.Tensor):
    """The properties the table is there for, so that no case goes dead."""
    codes, scale, bias, raw = reference_codes(W, 4)
    assert int(bias) == TABLES[name][2], f"{name}: zero point {int(bias)}"
    if name == "clamped":      # (its least code is -7: the range is shifted up by half a step)
        assert float(raw.max()) > 7 and int(codes.max()) == 7, "clamped: no unclamped code exceeds 7"
    else:
        assert int(codes.min()) == -8 and int(codes.max()) == 7, f"{name}: the codes do not span [-8, 7]"
        assert float(raw.min()) >= -8 and float(raw.max()) <= 7, f"{name}: a code was clamped"
    return codes, scale, bias


def pack_by_hand(codes: torch.Tensor) -> torch.Tensor:
    """int8 [N, D] -> uint8 [N, D/2]: byte r D/2 + d/2 holds element d, low nibble for even d, high nibble for odd d."""
    N, D = codes.shape
    rows = codes.tolist()
    out = [[(rows[r][2 * j] & 0xF) | ((rows[r][2 * j + 1] & 0xF) << 4) for j in range(D // 2)] for r in range(N)]
    return torch.tensor(out, dtype=torch.uint8).reshape(N, D // 2)


def unpack_by_hand(packed: torch.Tensor) -> torch.Tensor:
    def sx(n):
        return n - 16 if n >= 8 else n

    out = [[sx(b >> (4 * k) & 0xF) for b in row for k in (0, 1)] for row in packed.tolist()]
    return torch.tensor(out, dtype=torch.int8).reshape(packed.shape[0], packed.shape[1] * 2)

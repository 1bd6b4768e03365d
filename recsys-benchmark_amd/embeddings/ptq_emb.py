"""Post-training-quantised embedding tables (inference only) — reference: src/models/embeddings/ptq_emb.py:7-96.

Constructor arguments, buffer names (`weight`, `scale`, `bias`) and the quantisation arithmetic are the reference's, so a
table quantised here is bit-identical to one quantised there (pinned by tests/golden/ptq.npz); the lookup dequantises
inside the HIP gather (mi_gather_rows_quant): 32- or 16-byte rows at D=16 instead of 64-byte fp32 rows.

PTQEmb_Int(n_bits=4, packed=True) (an MI355X-side storage choice, not in the reference, which keeps one 4-bit code per int8
byte — ptq_emb.py:69-83): two codes per byte, 8-byte rows at D=16.  `weight` is then uint8 [N, D/2]: element d of row r in
byte r D/2 + d/2, the low nibble for even d, the high nibble for odd d, each a two's-complement code in [-8, 7]; `scale` and
`bias` (the zero point, an int8 scalar that can lie outside the nibble range) stay as they are.  Either form loads the other's
state_dict.  from_table() quantises a table where it lives: on the GPU in one launch (mi_ptq_quantise).
"""
import torch

from .. import _kernels
from .base import IEmbedding, _unhooked

_TABLE_KEY = "embedding._emb_module.weight"


def _quant_fm():
    from .. import quant_fm      # (imports layer_dcn, which imports this package: resolved at call time)

    return quant_fm


def _trained_table(checkpoint_path) -> torch.Tensor:
    """The fp32 table of a DeepFM / DCN checkpoint as the reference's trainers save it."""
    return torch.load(checkpoint_path, map_location="cpu")["state_dict"][_TABLE_KEY]


def _affine_params(floor: torch.Tensor, top: float, n_bits: int):
    """(scale, zero_point) of a table whose least value is `floor` (0-dim fp32 on the host) and whose greatest is `top`."""
    lowest, highest = -(1 << (n_bits - 1)), (1 << (n_bits - 1)) - 1
    scale = (top - floor) / (highest - lowest)
    return scale, (lowest - floor / scale).to(torch.int16 if n_bits == 16 else torch.int8)


def pack_nibbles(codes: torch.Tensor) -> torch.Tensor:
    """int8 codes [N, D] in [-8, 7] -> the packed table uint8 [N, D/2] (the layout of the module docstring), in torch.
    ValueError for an odd D or a code outside the nibble range (one host read)."""
    if codes.dtype != torch.int8 or codes.dim() != 2:
        raise TypeError(f"packing takes int8 codes [N, D], got {codes.dtype} {tuple(codes.shape)}")
    if codes.shape[1] % 2:
        raise ValueError(f"two codes per byte need an even width, got D = {codes.shape[1]}")
    if codes.numel() and bool(((codes < -8) | (codes > 7)).any()):
        raise ValueError("a code outside [-8, 7] cannot be packed as a 4-bit nibble")
    nib = codes.contiguous().view(torch.uint8) & 0xF
    return nib[:, 0::2] | (nib[:, 1::2] << 4)


def unpack_nibbles(packed: torch.Tensor) -> torch.Tensor:
    """The packed table uint8 [N, D/2] (or any [..., D/2] rows of it) -> int8 codes [..., D], in torch."""
    if packed.dtype != torch.uint8:
        raise TypeError(f"a packed 4-bit table is uint8, got {packed.dtype}")
    both = torch.stack([packed & 0xF, packed >> 4], -1).reshape(packed.shape[:-1] + (packed.shape[-1] * 2,))
    return ((both.to(torch.int16) ^ 8) - 8).to(torch.int8)


def affine_codes(table: torch.Tensor, n_bits: int):
    """(codes, scale, zero_point) with table ~ (codes - zero_point) * scale over the signed n_bits range: the scale spans
    [min, max] of the whole table, the zero point is truncated to the storage type, codes are rounded half-to-even
    (and clamped below 8 bits, where the storage type is wider than the range)."""
    lowest, highest = -(1 << (n_bits - 1)), (1 << (n_bits - 1)) - 1
    storage = torch.int16 if n_bits == 16 else torch.int8
    floor = table.min().cpu()                               # 0-dim fp32: the arithmetic below stays in fp32 tensors
    scale, zero_point = _affine_params(floor, table.max().item(), n_bits)
    codes = torch.round(table / scale + zero_point)
    if n_bits < 8:
        codes = codes.clamp(lowest, highest)
    return codes.to(storage), scale, zero_point


class _FrozenTable(IEmbedding):
    """field_dims / num_factor / mode are accepted for the registry's calling convention only."""

    weight: torch.Tensor

    def get_num_params(self) -> int:
        rows, width = self.weight.shape
        return rows * width

    def fm_quant(self, x):
        """The operands of DeepFM's fused lookup + dequantisation + FM launch (quant_fm.gather_fm_quant) for the ids x, or
        None when this table keeps forward(): a CPU table, an input that is not [B, F] on the table's device.  (These
        tables have no bag mode: `mode` is accepted and ignored.)"""
        if not self.weight.is_cuda or not x.is_cuda or x.dim() != 2:
            return None
        return self._fm_operands()

    def fm_lookup(self, x, offsets, w1, bias, sparse_w1: bool):
        """The dequantisation of the code rows inside DeepFM's lookup launch (mi_gather_fm_quant_fwd): inference only, no
        autograd node."""
        from .. import quant_fm

        quant = self.fm_quant(x) if _unhooked(self, w1, bias) else None
        if quant is None:
            return None
        return quant_fm.gather_fm_quant(x, offsets, w1=w1, bias=bias, **quant)


class PTQEmb_Fp16(_FrozenTable):
    def __init__(self, field_dims, num_factor, mode, ori_checkpoint_path):
        super().__init__()
        self.register_buffer("weight", _trained_table(ori_checkpoint_path).to(torch.float16))

    def forward(self, x):
        return _kernels.gather_rows_quant(x, self.weight)                     # fp16 rows -> fp32

    def _fm_operands(self):
        return dict(Wq=self.weight)

    def get_weight(self) -> torch.Tensor:
        return self.weight


class PTQEmb_Int(_FrozenTable):
    def __init__(self, field_dims, num_factor, mode, ori_checkpoint_path, n_bits=8, packed=False):
        super().__init__()
        self._check_form(n_bits, packed)
        self._install(*affine_codes(_trained_table(ori_checkpoint_path), n_bits), n_bits, packed)

    @staticmethod
    def _check_form(n_bits, packed):
        if n_bits not in (4, 8, 16):
            raise AssertionError("n_bits must be 4, 8 or 16")
        if packed and n_bits != 4:
            raise ValueError(f"packed=True stores two 4-bit codes per byte: it needs n_bits == 4, got {n_bits}")

    def _install(self, codes, scale, zero_point, n_bits, packed):
        self.n_bits = n_bits
        self.register_buffer("scale", scale)
        self.register_buffer("bias", zero_point)
        self.register_buffer("weight", codes)
        if packed and not self.is_packed:
            self.pack_()

    @classmethod
    @torch.no_grad()
    def from_table(cls, table: torch.Tensor, n_bits: int = 8, packed: bool = False) -> "PTQEmb_Int":
        """The table fp32 [N, D] (a view of any row stride) quantised where it lives; the result is on its device.  On the
        GPU the two extreme values are read back once, scale and zero point are formed on the host exactly as affine_codes
        forms them, and one launch (mi_ptq_quantise) writes the codes — or the packed nibbles — without an [N, D] temporary.
        On the CPU it is affine_codes (and pack_nibbles).  Both give the same bits."""
        cls._check_form(n_bits, packed)
        if table.dim() != 2 or table.dtype != torch.float32:
            raise TypeError(f"the table must be fp32 [N, D], got {table.dtype} {tuple(table.shape)}")
        if packed and table.shape[1] % 2:
            raise ValueError(f"two codes per byte need an even width, got D = {table.shape[1]}")
        table = table.detach()
        self = cls.__new__(cls)
        _FrozenTable.__init__(self)
        if table.is_cuda:
            ends = torch.stack(torch.aminmax(table)).cpu()      # the one host read
            scale, zero_point = _affine_params(ends[0], ends[1].item(), n_bits)
            scale, zero_point = scale.to(table.device), zero_point.to(table.device)
            self._install(_quant_fm().ptq_quantise(table, scale, zero_point, n_bits, packed), scale, zero_point, n_bits, packed)
        else:
            self._install(*affine_codes(table, n_bits), n_bits, packed)
        return self

    # ---- the two forms ----
    @property
    def is_packed(self) -> bool:
        return self.weight.dtype == torch.uint8

    @property
    def _width(self) -> int:
        return self.weight.shape[1] * (2 if self.is_packed else 1)

    def get_num_params(self) -> int:
        return self.weight.shape[0] * self._width

    @torch.no_grad()
    def pack_(self) -> "PTQEmb_Int":
        """Two codes per byte, in place: `weight` becomes uint8 [N, D/2]; buffer names and state_dict keys stay.  ValueError
        (the table untouched) unless n_bits == 4 and D is even.  A GPU table is repacked by mi_int4_repack, which reports a
        code outside [-8, 7] through the error word (check_index_errors), a CPU table by pack_nibbles."""
        if self.is_packed:
            return self
        if self.n_bits != 4:
            raise ValueError(f"pack_() stores two 4-bit codes per byte: it needs n_bits == 4, got {self.n_bits}")
        D = self.weight.shape[1]
        if D % 2:
            raise ValueError(f"two codes per byte need an even width, got D = {D}")
        self.weight = _quant_fm().int4_repack(self.weight, D, unpack=False) if self.weight.is_cuda else pack_nibbles(self.weight)
        return self

    @torch.no_grad()
    def unpack_(self) -> "PTQEmb_Int":
        """Back to the reference's one code per int8 byte, in place."""
        if self.is_packed:
            D = self._width
            self.weight = _quant_fm().int4_repack(self.weight, D, unpack=True) if self.weight.is_cuda else unpack_nibbles(self.weight)
        return self

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # either form of a 4-bit table loads into either module: int8 [N, D] (the reference's checkpoint) or uint8 [N, D/2]
        key = prefix + "weight"
        saved = state_dict.get(key)
        if torch.is_tensor(saved):
            own = self.weight
            if saved.dtype != own.dtype or saved.dim() != 2:
                converted = None
                try:
                    if self.n_bits == 4 and saved.dim() == 2 and saved.dtype == torch.uint8 and not self.is_packed:
                        converted = unpack_nibbles(saved)
                    elif self.n_bits == 4 and saved.dim() == 2 and saved.dtype == torch.int8 and self.is_packed:
                        converted = pack_nibbles(saved)
                except ValueError as e:
                    error_msgs.append(f"{key}: {e}")
                else:
                    if converted is None:
                        error_msgs.append(f"{key}: expected {own.dtype} {tuple(own.shape)}"
                                          + (" or the other form of a 4-bit table" if self.n_bits == 4 else "")
                                          + f", got {saved.dtype} {tuple(saved.shape)}")
                state_dict = dict(state_dict)
                state_dict[key] = own if converted is None else converted      # (refused: the table stays as it is)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    # ---- lookups ----
    def _dequant(self, codes):
        return (codes.to(torch.int32) - self.bias.to(torch.int32)).to(torch.float32) * self.scale

    def takes_offsets(self, x: torch.Tensor) -> bool:
        """Whether forward(x, offsets=...) adds the per-field offsets inside the lookup kernel (a packed table on the GPU,
        [B, F] ids on its device) — the protocol of dcn._FieldModel._lookup."""
        return bool(self.is_packed and self.weight.is_cuda and x.is_cuda and x.dim() == 2 and x.device == self.weight.device)

    def forward(self, x, offsets=None):
        """offsets (optional extension, [F]): x then holds the model's raw per-field ids [B, F]; returns (embeddings, row
        ids), the addition inside mi_gather_rows_int4 where takes_offsets(x) holds."""
        if offsets is not None:
            if not self.takes_offsets(x):
                rows = x + offsets
                return self.forward(rows), rows
            return _quant_fm().gather_rows_int4(x, self.weight, self.scale, self.bias, self._width, offsets=offsets.reshape(-1))
        if not self.is_packed:
            return _kernels.gather_rows_quant(x, self.weight, self.scale.reshape(1), self.bias.reshape(1))
        if self.weight.is_cuda:
            return _quant_fm().gather_rows_int4(x, self.weight, self.scale, self.bias, self._width)
        return self._dequant(unpack_nibbles(self.weight[x]))      # a packed CPU table: the looked-up rows unpacked in torch

    def _fm_operands(self):
        if self.is_packed:
            return dict(Wq=self.weight, scale=self.scale, zero_point=self.bias, packed4=True, D=self._width)
        return dict(Wq=self.weight, scale=self.scale, zero_point=self.bias)

    def get_weight(self) -> torch.Tensor:
        if not self.is_packed:
            return (self.weight - self.bias) * self.scale
        if self.weight.is_cuda:
            return _quant_fm().gather_rows_int4(None, self.weight, self.scale, self.bias, self._width)
        return self._dequant(unpack_nibbles(self.weight))

"""Test infrastructure for the de-duplicated sharded lookup (ShardedDeepFM(dedup=True)): a torch restatement of
mi_route_buckets_unique built from torch.unique per owner, the summing slot lookup (autograd's indexed gather already
adds the gradients of repeated slots), and generators of skewed ids.  Same interface as sharded.HipOps."""
from typing import List, Optional

import numpy as np
import torch

from oracle.sharded_ops import TorchOps

CRITEO_26 = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194,
             27, 14992, 5461306, 10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]


def field_offsets(dims: List[int]) -> torch.Tensor:
    return torch.cumsum(torch.tensor([0] + list(dims[:-1]), dtype=torch.int64), 0)


def segments_from_slots(slot: torch.Tensor, nslot: int) -> torch.Tensor:
    """A segment description (include/mi355x_recsys.h, mi_route_buckets_unique) for ANY slot array: int32
    [2*nslot + n] — per slot the [begin, end) of its lookups in `order`, then `order`, in which every slot's lookups
    stand together in ascending flat position (a stable sort by slot).  Lookups of slots >= nslot own no segment."""
    flat = slot.reshape(-1)
    srt, order = torch.sort(flat, stable=True)
    ar = torch.arange(nslot, dtype=flat.dtype, device=flat.device)
    begin, end = torch.searchsorted(srt, ar), torch.searchsorted(srt, ar, right=True)
    empty = end == begin
    begin, end = begin.masked_fill(empty, 0), end.masked_fill(empty, 0)
    return torch.cat([torch.stack([begin, end], 1).reshape(-1), order]).to(torch.int32)


def slots_from_segments(segments: torch.Tensor, nslot: int, n: int):
    """(slot per lookup rebuilt from a segment description — nslot where no segment holds the lookup —, True when every
    segment lists its lookups in strictly ascending flat position and no lookup twice)."""
    seg = segments.to(torch.int64).cpu()
    begin, end, order = seg[0:2 * nslot:2], seg[1:2 * nslot:2], seg[2 * nslot:]
    lens = end - begin
    ids = torch.repeat_interleave(torch.arange(nslot), lens)
    within = torch.arange(int(lens.sum())) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
    pos = order[begin[ids] + within]
    slot = torch.full((n,), nslot, dtype=torch.int64)
    slot[pos] = ids
    same = ids[1:] == ids[:-1]
    ascending = bool((pos[1:][same] > pos[:-1][same]).all()) and torch.unique(pos).numel() == pos.numel()
    return slot, ascending


class DedupTorchOps(TorchOps):
    @staticmethod
    def route_buckets_unique(idx, offsets, world: int, num_rows: int, cap: int, overflow,
                             slot_out: Optional[torch.Tensor] = None, segments_out: Optional[torch.Tensor] = None,
                             send_out: Optional[torch.Tensor] = None, field_sort: bool = True):
        rows = idx.to(torch.int64)
        if offsets is not None:
            rows = rows + offsets.reshape(-1)
        flat = rows.reshape(-1)
        n = flat.numel()
        ok = (flat >= 0) & (flat < num_rows)
        owner = torch.where(ok, flat % world, torch.full_like(flat, -1))
        local = flat // world
        dump = world * cap
        slot = torch.full((n,), dump, dtype=torch.int64, device=flat.device)
        send = torch.empty(world * cap, dtype=torch.int64, device=flat.device)
        for w in range(world):
            send[w * cap:(w + 1) * cap] = (num_rows - w + world - 1) // world       # the owner's sink row
            mine = owner == w
            distinct, which = torch.unique(local[mine], return_inverse=True)        # ascending local rows
            kept = min(int(distinct.numel()), cap)
            send[w * cap:w * cap + kept] = distinct[:kept]
            slot[mine] = torch.where(which < cap, w * cap + which, torch.full_like(which, dump))
            if distinct.numel() > cap:
                overflow |= 1
        segments = segments_from_slots(slot, dump)
        slot = slot.view(idx.shape)
        if slot_out is not None:
            slot_out.copy_(slot)
            slot = slot_out
        if segments_out is not None:
            segments_out.copy_(segments)
            segments = segments_out
        if send_out is not None:
            send_out.copy_(send)
            send = send_out
        return send, slot, segments

    @staticmethod
    def slot_fm_unique(buf, slot, bias, segments):
        return TorchOps.slot_fm(buf, slot, bias)


# ---- skewed ids -------------------------------------------------------------------------------------------------------
def hot_value_ids(dims: List[int], B: int, share: float, gen: torch.Generator, hot: Optional[List[int]] = None) -> torch.Tensor:
    """[B, F] ids, uniform within every field except that a `share` of each field's lookups sit on ONE value (hot[f],
    default: a value drawn per field)."""
    cols = []
    for f, d in enumerate(dims):
        h = int(torch.randint(0, d, (1,), generator=gen)) if hot is None else int(hot[f])
        col = torch.randint(0, d, (B,), generator=gen)
        col[torch.rand(B, generator=gen) < share] = h
        cols.append(col)
    return torch.stack(cols, 1)


def congruent_hot_values(dims: List[int], world: int) -> List[int]:
    """Per field the smallest id whose global row is = 0 modulo world: all hot values then live at owner 0."""
    off = field_offsets(dims).tolist()
    hot = [(-o) % world for o in off]
    assert all(h < d for h, d in zip(hot, dims))
    return hot


def zipf_ids(dims: List[int], B: int, a: float, seed: int) -> torch.Tensor:
    """[B, F] ids with Zipf(a) ranks inside every field (rank 1 -> id 0), folded into the field's range."""
    rng = np.random.default_rng(seed)
    return torch.stack([torch.from_numpy((rng.zipf(a, B) - 1) % d) for d in dims], 1).to(torch.int64)

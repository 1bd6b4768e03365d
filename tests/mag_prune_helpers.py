"""The contract of magnitude pruning restated in stock torch on the CPU (calls nothing of the library).

For one table W [N, D] fp32, ratio p, floor m:
  * k = int(N * D * p) in Python floats;
  * key(w) = bit pattern of |w| (for non-negative floats the int32 view orders like the magnitude; |-0.0| = +0.0);
  * the m largest keys of each row are protected, equal keys lower column first (stable descending sort);
  * the k smallest unprotected keys of the table become +0.0, equal keys lower flat index first (stable sort);
  * N * m + k > N * D is refused.
This is what the reference's op sequence (src/utils.py:8-34) gives when its `topk` / `argsort` are stable; with
pairwise distinct magnitudes it equals the reference itself (tests/golden/mag_prune_tables.npz).
"""
import torch

_PROTECTED = 1 << 40          # above every 31-bit key


def keys_of(weight: torch.Tensor) -> torch.Tensor:
    return weight.detach().cpu().abs().contiguous().view(torch.int32).to(torch.int64)


def protected_mask(weight: torch.Tensor, min_item: int) -> torch.Tensor:
    key = keys_of(weight)
    prot = torch.zeros(key.shape, dtype=torch.bool)
    if min_item > 0:
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        prot.scatter_(1, order[:, :min_item], True)
    return prot


def mag_prune(weight: torch.Tensor, p: float, min_item: int = 0) -> torch.Tensor:
    """The pruned copy of `weight` (CPU, float32); the input is not modified."""
    assert weight.dim() == 2 and weight.dtype == torch.float32
    if not 0.0 <= p <= 1.0:
        raise ValueError("p outside [0, 1]")
    n, d = weight.shape
    k = int(n * d * p)
    if n * min_item + k > n * d:
        raise ValueError("N * m + k > N * D")
    w = weight.detach().cpu().clone().contiguous()
    key = keys_of(w)
    key[protected_mask(w, min_item)] = _PROTECTED
    first = torch.sort(key.flatten(), stable=True).indices[:k]
    w.view(-1)[first] = 0.0
    return w


def mag_prune_state(state, p: float, min_item: int = 0):
    return {name: mag_prune(w, p, min_item) for name, w in state.items()}


def distinct_table(n: int, d: int, seed: int) -> torch.Tensor:
    """[n, d] fp32 with pairwise distinct magnitudes (multiples of 2^-12) and random signs — plain randn already has
    duplicate magnitudes at 16 K elements, and an unstable sort is then no yardstick."""
    gen = torch.Generator().manual_seed(seed)
    mag = (torch.randperm(n * d, generator=gen) + 1).to(torch.float32) * 2.0 ** -12
    sign = torch.randint(0, 2, (n * d,), generator=gen).to(torch.float32) * 2 - 1
    return (mag * sign).view(n, d)

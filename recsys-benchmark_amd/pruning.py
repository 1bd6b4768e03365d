"""Global magnitude pruning with a per-row floor — the training-free baseline of the reference's tables.

Reference: src/utils.py:8-34 (`prune`), scripts/lightgcn/run_mag_prune.py:55-172 and
scripts/cf_train/run_mag_prune.py:55-188 (`get_v`, `bin_search`, `run_all`).  The reference ranks every element of a
table (a per-row `topk`, a full `argsort`, two index writes) per table and per search candidate; here the same result
is a k-th element selection on the device (csrc/mag_prune.hip): nothing is sorted and nothing is read back.

The contract, for one table W [N, D] fp32, ratio p and floor m:
  * k = int(N * D * p), in Python floats as the reference computes it;
  * key(w) = bit pattern of |w|; the m largest keys of each row are protected (equal keys: lower column first);
  * the k smallest unprotected keys of the table become +0.0 (equal keys at the cut: lower flat index first) — what
    the reference's op sequence gives with a stable sort; everything else is copied bit for bit;
  * N * m + k > N * D is refused (ValueError): past that the reference prunes its own `inf` markers in sort order.
"""
from typing import Callable, Dict, Iterable, List, Optional

import torch

from . import _lib

__all__ = ["prune", "prune_table", "to_pruned_tables", "evaluate_pruned", "search_min_item"]


def _num_to_prune(num_rows: int, hidden_size: int, p: float, min_item: int = 0) -> int:
    """k of the contract, after the argument checks every entry point shares (ValueError)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"prune ratio must lie in [0, 1], got {p}")
    min_item = int(min_item)
    if min_item < 0:
        raise ValueError(f"min_item must be >= 0, got {min_item}")
    total = num_rows * hidden_size
    k = int(total * p)
    if num_rows * min_item + k > total:
        raise ValueError(f"cannot prune {k} of {total} elements and keep {min_item} in each of {num_rows} rows "
                         f"of {hidden_size}")
    return k


def _check_table(weight: torch.Tensor) -> None:
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise ValueError("magnitude pruning takes 2-D tables (the reference asserts len(weight.shape) == 2)")
    if weight.dtype != torch.float32:
        raise TypeError(f"expected a float32 table, got {weight.dtype}")


def _row_strided(t: torch.Tensor) -> bool:
    return t.shape[1] == 1 or t.stride(1) == 1


def _select(weight: torch.Tensor, out: Optional[torch.Tensor], k: int, m: int) -> torch.Tensor:
    """mi_mag_prune on a row-strided table; returns the workspace (threshold and row cuts, for the CSR build)."""
    dev = weight.device
    lib = _lib.load()
    N, D = weight.shape
    ws = torch.empty(lib.mi_mag_prune_workspace_bytes(N), dtype=torch.uint8, device=dev)
    _lib.check(lib.mi_mag_prune(weight.data_ptr(), weight.stride(0), _lib.ptr(out), 0 if out is None else out.stride(0),
                                N, D, k, m, ws.data_ptr(), _lib.stream_ptr(dev)), "mi_mag_prune")
    return ws


@torch.no_grad()
def prune_table(weight: torch.Tensor, p: float, min_item: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One table.  out=None prunes `weight` in place (like the reference) and returns it; otherwise the pruned table is
    written to `out` (same shape, float32, same device) and `weight` is left untouched.
    The kernels take tables whose rows are contiguous, at any row stride.  Any other layout (a transposed view, say) is
    pruned through a packed copy: two extra copies of the table for such an operand."""
    _check_table(weight)
    N, D = weight.shape
    k = _num_to_prune(N, D, p, min_item)
    if out is not None:
        _check_table(out)
        if out.shape != weight.shape:
            raise ValueError(f"out has shape {tuple(out.shape)}, the table {tuple(weight.shape)}")
    _lib.require_gpu(weight, out)
    result = weight if out is None else out
    weight = weight.detach()
    dst = result.detach()
    if N == 0 or D == 0:
        return result
    # the kernels take any row stride; other layouts go through a packed copy (the pruning itself stays on the kernels)
    src_k = weight if _row_strided(weight) else weight.contiguous()
    dst_k = dst if _row_strided(dst) else (src_k if src_k is not weight else torch.empty_like(src_k))
    _select(src_k, dst_k, k, int(min_item))
    if dst_k is not dst:
        dst.copy_(dst_k)
    return result


@torch.no_grad()
def _select_threshold(weight: torch.Tensor, p: float, min_item: int = 0) -> torch.Tensor:
    """The selection alone, nothing pruned: a device int64[4] = (T, unprotected elements with key < T, with key == T,
    equals of T that would be pruned), T being the key (bit pattern of the magnitude) of the k-th smallest unprotected
    element (T = 0 and nothing pruned when k == 0).  Not synchronised."""
    _check_table(weight)
    N, D = weight.shape
    k = _num_to_prune(N, D, p, min_item)
    dev = _lib.require_gpu(weight)
    weight = weight.detach()
    if not _row_strided(weight):
        weight = weight.contiguous()
    res = torch.zeros(4, dtype=torch.int32, device=dev)
    if N and D:
        ws = _select(weight, None, k, int(min_item))
        _lib.check(_lib.load().mi_mag_prune_result(ws.data_ptr(), res.data_ptr(), _lib.stream_ptr(dev)),
                   "mi_mag_prune_result")
    return res.to(torch.int64) & 0xFFFFFFFF


@torch.no_grad()
def prune(state: Dict[str, torch.Tensor], p: float, min_item: int = 0) -> Dict[str, torch.Tensor]:
    """src/utils.py:8-34: every entry of `state` (all 2-D) pruned in place — the tensors of a state_dict() alias the
    parameters — and the dict returned."""
    for weight in state.values():
        _check_table(weight)
        _num_to_prune(weight.shape[0], weight.shape[1], p, min_item)
        _lib.require_gpu(weight)
    for name, weight in state.items():
        state[name] = prune_table(weight, p, min_item)
    return state


@torch.no_grad()
def _pruned_csr(weight: torch.Tensor, p: float, min_item: int = 0):
    """(crow int64 [N + 1], col int64, values fp32) of the pruned table, equal array for array to
    `prune_table(weight.clone(), p, min_item).to_sparse_csr()`, without the dense pruned table.  One host read: the
    number of stored elements, to size col / values."""
    _check_table(weight)
    N, D = weight.shape
    k = _num_to_prune(N, D, p, min_item)
    dev = _lib.require_gpu(weight)
    weight = weight.detach()
    if not _row_strided(weight):
        weight = weight.contiguous()
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if N == 0 or D == 0:
        return crow, torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    lib = _lib.load()
    m = int(min_item) if k > 0 else 0                     # k == 0: nothing to cut, a dense-to-CSR conversion
    ws = _select(weight, None, k, m) if k > 0 else None
    csr_ws = torch.empty(lib.mi_mag_csr_workspace_bytes(N), dtype=torch.uint8, device=dev)
    stream = _lib.stream_ptr(dev)
    _lib.check(lib.mi_mag_csr_count(weight.data_ptr(), weight.stride(0), N, D, _lib.ptr(ws), m, csr_ws.data_ptr(),
                                    crow.data_ptr(), stream), "mi_mag_csr_count")
    nnz = int(crow[N].item())
    col = torch.empty(nnz, dtype=torch.int64, device=dev)
    values = torch.empty(nnz, dtype=torch.float32, device=dev)
    if nnz:
        _lib.check(lib.mi_mag_csr_fill(weight.data_ptr(), weight.stride(0), N, D, _lib.ptr(ws), m, csr_ws.data_ptr(),
                                       crow.data_ptr(), col.data_ptr(), values.data_ptr(), stream), "mi_mag_csr_fill")
    return crow, col, values


# ---- serving and the min-item search --------------------------------------------------------------------------------
def _is_ctr(model) -> bool:
    from .dcn import DCN_Mix, DCNv2
    from .deepfm import DeepFM

    return isinstance(model, (DeepFM, DCN_Mix, DCNv2))


def _table_slots(model):
    """(owner module, attribute name) of every embedding table of a LightGCN / SingleLightGCN / NeuMF, or the one shared
    table of a DeepFM / DCN_Mix / DCNv2."""
    from .lightgcn import LightGCN, SingleLightGCN
    from .neumf import NeuMF

    if _is_ctr(model):
        return [(model, "embedding")]
    if isinstance(model, LightGCN):
        return [(model, "user_emb_table"), (model, "item_emb_table")]
    if isinstance(model, SingleLightGCN):
        return [(model, "emb_table")]
    if isinstance(model, NeuMF):
        return [(part, name) for part in (model._gmf, model._mlp) for name in ("user_emb_table", "item_emb_table")]
    raise TypeError("to_pruned_tables takes a LightGCN, SingleLightGCN, NeuMF, DeepFM, DCN_Mix or DCNv2, got "
                    f"{type(model).__name__}")


@torch.no_grad()
def to_pruned_tables(model, p: float = 0.0, min_item: int = 0, compact: bool = False):
    """Replace each table of the model by a PrunedEmbedding (CSR) of its current weight — what `_load_pep` of
    scripts/lightgcn/infer_lightgcn.py:224-247 and scripts/deepfm/infer_deepfm.py does — pruned by (p, min_item) on the
    way when p > 0.  A CTR model's table is taken through get_weight(), whatever its kind (the reference's
    `from_other_emb`).  compact: one-byte columns and int32 row pointers (PrunedEmbedding.compact_()).  The model then
    serves through the usual validation and scoring paths.  Returns the model."""
    from .embeddings import PrunedEmbedding

    for owner, name in _table_slots(model):
        table = getattr(owner, name)
        setattr(owner, name, PrunedEmbedding.from_pruned(table, p, min_item, mode=getattr(table, "_mode", None),
                                                         compact=compact))
    if hasattr(model, "clear_cache"):
        model.clear_cache()
    return model


def _default_validate(model) -> Callable:
    from . import trainer
    from .neumf import NeuMF

    if _is_ctr(model):
        return trainer.validate_epoch
    return trainer.validate_epoch_nmf if isinstance(model, NeuMF) else trainer.validate_epoch_cf


def _default_keys(model, state) -> List[str]:
    from .neumf import NeuMF

    if _is_ctr(model):                                         # scripts/deepfm/run_l2_benchmark.py: the embedding's entries
        return ["embedding." + k for k in model.embedding.state_dict()]
    if isinstance(model, NeuMF):
        return [k for k in state if "emb_table" in k]         # scripts/cf_train/run_mag_prune.py:69-73
    return list(state)                                         # scripts/lightgcn/run_mag_prune.py:63-69: every entry


class _Candidates:
    """The tables of a model under search: the originals are cloned ONCE, every candidate is pruned from the clone
    into the live parameter (out of place), and restore() copies the clones back."""

    def __init__(self, model, keys: Optional[Iterable[str]]):
        state = model.state_dict()
        self.model = model
        self.keys = _default_keys(model, state) if keys is None else list(keys)
        self.live = {k: state[k] for k in self.keys}
        for w in self.live.values():
            _check_table(w)
            _lib.require_gpu(w)
        self.originals = {k: w.detach().clone() for k, w in self.live.items()}

    def _changed(self):
        if hasattr(self.model, "clear_cache"):
            self.model.clear_cache()

    def apply(self, p: float, min_item: int) -> None:
        for w in self.live.values():
            _num_to_prune(w.shape[0], w.shape[1], p, min_item)
        for k, w in self.live.items():
            prune_table(self.originals[k], p, min_item, out=w)
        self._changed()

    def restore(self) -> None:
        with torch.no_grad():
            for k, w in self.live.items():
                w.copy_(self.originals[k])
        self._changed()


def _validate_candidate(cands: _Candidates, p, min_item, val_loader, train_dataset, device, validate) -> float:
    try:
        cands.apply(p, min_item)
        if _is_ctr(cands.model):
            score = validate(val_loader, cands.model, device)["auc"]
        else:
            score = validate(train_dataset, val_loader, cands.model, device, metrics=["ndcg", "recall"])["ndcg"]
    finally:
        cands.restore()
    return score


def evaluate_pruned(model, p: float, min_item: int, val_loader, train_dataset, device="cuda",
                    validate: Optional[Callable] = None, keys: Optional[Iterable[str]] = None) -> float:
    """`get_v` of the two run_mag_prune.py scripts: prune the tables, validate, restore; returns the NDCG.
    keys=None: every state entry for a LightGCN / SingleLightGCN (all must be 2-D, as the reference asserts), the
    entries whose name contains `emb_table` for a NeuMF.  validate=None: trainer.validate_epoch_cf or
    trainer.validate_epoch_nmf by model type; a callable is called as
    validate(train_dataset, val_loader, model, device, metrics=["ndcg", "recall"]).
    A DeepFM / DCN_Mix / DCNv2 (scripts/deepfm/run_l2_benchmark.py): keys=None is every entry of
    model.embedding.state_dict() (all must be 2-D), validate=None is trainer.validate_epoch, a callable is called as
    validate(val_loader, model, device), and the "auc" of its result is returned; train_dataset is ignored (None will do).
    The model's state is bit-identical afterwards, also when validation raises."""
    validate = _default_validate(model) if validate is None else validate
    return _validate_candidate(_Candidates(model, keys), p, min_item, val_loader, train_dataset, device, validate)


def _max_min_item(hidden_size: int, p: float) -> int:
    """The largest floor the searches try: int(hidden_size * (1 - p)) in Python floats, as the reference computes it
    (int(64 * (1 - 0.8)) == 12)."""
    return int(hidden_size * (1 - p))


def _bin_search(evaluate: Callable[[int], float], bound: int) -> int:
    """The binary search of run_mag_prune.py:84-156 over slots 1 .. bound + 1 (slot s stands for floor s - 1; slots 0 and
    bound + 2 are walls scoring -inf).  A slot is scored at most once, and in the order the reference asks: the middle
    slot, then — unless floor 0 beats it — its left and its right neighbour.  Returns the first slot that is not on a
    strict slope (1-based, like the reference), 1 when the range closes."""
    scores: Dict[int, float] = {}

    def score(slot: int) -> float:
        if slot < 1 or slot > bound + 1:
            return float("-inf")
        if slot not in scores:
            scores[slot] = evaluate(slot - 1)
        return scores[slot]

    floor0 = score(1)
    lo, hi = 1, bound + 1
    while lo <= hi:
        slot = (lo + hi) // 2
        here = score(slot)
        if floor0 > here:
            hi = slot - 1
            continue
        before = score(slot - 1)
        after = score(slot + 1)
        if before < here < after:
            lo = slot + 1
        elif before > here > after:
            hi = slot - 1
        else:
            return slot
    return 1


def _run_all(evaluate: Callable[[int], float], bound: int) -> int:
    """The exhaustive form (run_mag_prune.py:159-172): every floor 0 .. bound in ascending order; the first best one,
    1-based.  The scores are compared as float32, as the reference's tensor of Python floats compares them."""
    scores = torch.tensor([evaluate(floor) for floor in range(bound + 1)], dtype=torch.float32)
    return int(scores.argmax()) + 1


def search_min_item(model, p: float, hidden_size: int, val_loader=None, train_dataset=None, device="cuda",
                    mode: str = "binary", validate: Optional[Callable] = None, keys: Optional[Iterable[str]] = None,
                    evaluate: Optional[Callable[[int], float]] = None) -> int:
    """`bin_search` (mode="binary") / `run_all` (mode="all") of the two run_mag_prune.py scripts, with the reference's
    probe order and its 1-based return value: the floor to use is `result - 1`, as both scripts do.
    A DeepFM / DCN_Mix / DCNv2 is scored by its validation AUC (evaluate_pruned), train_dataset ignored.
    evaluate: a callable floor -> score replacing the validation of a candidate (the model is then not touched);
    otherwise every candidate is `evaluate_pruned`, the original tables being kept on the device once for the search."""
    if mode not in ("binary", "all"):
        raise ValueError(f"mode must be 'binary' or 'all', got {mode!r}")
    bound = _max_min_item(hidden_size, p)
    run = _bin_search if mode == "binary" else _run_all
    if evaluate is not None:
        return run(evaluate, bound)
    validate = _default_validate(model) if validate is None else validate
    cands = _Candidates(model, keys)
    return run(lambda m: _validate_candidate(cands, p, m, val_loader, train_dataset, device, validate), bound)

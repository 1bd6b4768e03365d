"""The training / validation loops around the hot path — CTR (reference: src/trainer/deepfm.py:17-139) and LightGCN
(src/trainer/lightgcn.py:14-165, 378-421) — with the per-batch work — forward, loss, backward, every optimizer step —
replayed as ONE hipGraph.

At the headline shape the eager step is bound by the host (≈0.85 ms of Python / autograd / launch work around ≈0.45 ms of
kernels); a captured step has no host work beyond its input copies (ids and labels, plus the next batch's ids when the
model prefetches) and one graph launch.  What makes the whole step capturable: the lookup kernels emit row-form gradients
without host syncs, `optim.SparseAdam(capturable=True)` keeps its step count on the device, `optim.Adam` steps from
device-side counts too (`optim.get_optimizers` builds both on a GPU), dropout seeds and BatchNorm counters advance inside
kernels.

`train_epoch` / `validate_epoch` keep the reference's signatures and return values; the loss is accumulated on the device
and read back at the logging steps only (the reference calls `.item()` every batch).
"""
import datetime
import gc
import logging
import inspect
import warnings
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib, losses
from .cf_data import DeviceTruth
from .ctr_metric import CTRMetric, _binary_auc_torch, binary_auc  # noqa: F401  (binary_auc's home was here)
from .lightgcn import get_sparsity_and_param, score_topk, train_items_csr

logger = logging.getLogger("recsys_benchmark_amd.trainer")
now = datetime.datetime.now


def _check_errors(model) -> None:
    """Deferred index / overflow checks at a logging step.  A row-sharded model checks COLLECTIVELY (the ranks agree on the
    flags, then all raise together: a rank raising alone would leave its peers waiting in the next all-to-all)."""
    if hasattr(model, "check_overflow"):
        model.check_index_errors()
        model.check_overflow()       # a peer bucket that overflowed dropped lookups
    else:
        _lib.check_index_errors()


class _capture(torch.cuda.graph):
    """torch.cuda.graph that also tells a direct RCCL communicator's watchdog thread (sharded.DirectComm) that a
    global-mode capture is under way, so it leaves its event queries alone until the capture has ended."""

    def __enter__(self):
        from . import sharded

        sharded.note_capture(+1)
        # torch.cuda.graph no longer collects garbage before a capture.  A dead reference cycle that owns a graph, a stream
        # or an event, collected by a pass that happens to run INSIDE the capture, destroys it there — not allowed while a
        # global-mode capture is open (the runtime aborted the process).  Collect now; no pass until the capture has ended.
        self._gc_was_enabled = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            return super().__enter__()
        except BaseException:
            self._leave()
            raise

    def _leave(self):
        from . import sharded

        if self._gc_was_enabled:
            gc.enable()
        sharded.note_capture(-1)

    def __exit__(self, *exc):
        try:
            return super().__exit__(*exc)
        finally:
            self._leave()


def _capturable(optimizers) -> bool:
    """False when an optimizer keeps its step count on the host (torch's Adam family without `capturable=True`): its
    step() refuses to run under capture, and a capture abandoned half-way is not something to recover from — so this
    is checked up front.  `optim.get_optimizers` / `optim.Adam` / `optim.SparseAdam(capturable=True)` all qualify."""
    return all(group.get("capturable", True) for opt in optimizers for group in opt.param_groups)


class _Replayed:
    """body(*tensors) for ONE input shape: the first `warmup` calls of a shape run eagerly (the count restarts when the
    shape changes), the next call of that shape is captured as a hipGraph and from then on replayed — the inputs are
    copied into static clones and the static output is returned.  Calls of any other shape run `body` eagerly and leave
    the graph alone.  A capture that raises is warned about and never tried again (`enabled` turns False)."""

    def __init__(self, body, warmup: int, what: str, before_capture=None, enabled: bool = True, eager: str = "steps"):
        """before_capture(*static_inputs) runs between cloning the inputs and the capture; what / eager: the warning's nouns."""
        self.body, self.warmup, self.what, self.before_capture, self.eager = body, warmup, what, before_capture, eager
        self.enabled = enabled
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._static, self._out, self._key, self._seen = (), None, None, 0

    def ready(self, *tensors) -> bool:
        """True when `replay(*tensors)` can serve this call; counts the warm-up calls and captures when they are done."""
        key = tuple((t.shape, t.dtype) for t in tensors)
        if self.graph is not None:
            return key == self._key
        if self.enabled and self._seen >= self.warmup and key == self._key:
            try:
                static = tuple(t.clone() for t in tensors)
                if self.before_capture is not None:
                    self.before_capture(*static)
                graph = torch.cuda.CUDAGraph()
                with _capture(graph):
                    out = self.body(*static)
                self.graph, self._static, self._out = graph, static, out
                return True
            except Exception as exc:               # leave the caller running on the eager HIP path
                warnings.warn(f"hipGraph capture of {self.what} failed ({exc!r}); continuing with eager {self.eager}")
                torch.cuda.synchronize()
                self.enabled = False
        if key != self._key:
            self._key, self._seen = key, 0
        self._seen += 1
        return False

    def replay(self, *tensors):
        for dst, src in zip(self._static, tensors):
            dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self._out

    def __call__(self, *tensors):
        return self.replay(*tensors) if self.ready(*tensors) else self.body(*tensors)


class GraphedTrainStep:
    """step(inputs, labels): one optimisation step of `model` on the batch, in the reference's order (forward, loss,
    zero_grad, backward, optimizer steps).  The first `warmup` calls run eagerly (they are ordinary training steps and
    let every lazily created buffer come into being), the next call of the same batch shape is captured and from then on
    replayed; batches of any other shape (the ragged last batch of an epoch) run eagerly.

    `loss_sum` (0-dim device tensor) accumulates the batch losses, `steps` counts them; `last_loss` is the latest one.
    """

    def __init__(self, model: torch.nn.Module, optimizers, criterion: Optional[torch.nn.Module] = None, warmup: int = 2,
                 use_graph: bool = True, clip_grad: float = 0, extra_loss=None, extra_weight: float = 1.0):
        """extra_loss: optional callable returning a scalar tensor; `extra_weight` times it is added to the criterion
        before the backward (the CERP trainer's `prune_loss_weight * model.embedding.get_prune_loss()`); `extra_sum`
        accumulates the unweighted values."""
        self.model = model
        self.extra_loss, self.extra_weight = extra_loss, extra_weight
        self.extra_sum: Optional[torch.Tensor] = None
        self.optimizers: List[torch.optim.Optimizer] = optimizers if isinstance(optimizers, list) else [optimizers]
        self.criterion = criterion if criterion is not None else losses.BCEWithLogitsLoss()
        self._labels_in_forward = (isinstance(self.criterion, losses.BCEWithLogitsLoss)
                                   and "labels" in inspect.signature(model.forward).parameters)
        self._prefetches = callable(getattr(model, "prefetch_next", None))
        self._static_next = None
        self.clip_grad = clip_grad
        # clip_grad_norm_ reads the norm back on some paths and row-form gradients have no dense norm: eager only
        use_graph = use_graph and not clip_grad
        if use_graph and not _capturable(self.optimizers):
            warnings.warn("an optimizer keeps its step count on the host (capturable=False): the training step runs "
                          "eagerly; build the optimizers with recsys_benchmark_amd.optim.get_optimizers / optim.Adam")
            use_graph = False
        self.steps = 0
        self.loss_sum: Optional[torch.Tensor] = None
        self.last_loss: Optional[torch.Tensor] = None
        self._replayed = _Replayed(self._body, warmup, "the training step", self._before_capture, use_graph)

    warmup = property(lambda self: self._replayed.warmup)
    use_graph = property(lambda self: self._replayed.enabled)
    _graph = property(lambda self: self._replayed.graph)

    def _body(self, inputs, labels):
        labels = labels.float()
        # (a model that takes the step's labels — DeepFM's fused step — evaluates the criterion inside its head launch; the
        #  criterion call below then only picks the result up)
        outputs = self.model(inputs, labels=labels) if self._labels_in_forward else self.model(inputs)
        loss = self.criterion(outputs, labels)
        total = loss
        if self.extra_loss is not None:
            extra = self.extra_loss()
            total = loss + self.extra_weight * extra
            self.extra_sum += extra.detach()
        for opt in self.optimizers:
            opt.zero_grad(set_to_none=True)
        total.backward(self._one)          # d(loss)/d(loss) from a resident scalar: no fill launch per step
        if self.clip_grad:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip_grad)
        for opt in self.optimizers:
            opt.step()
        loss = loss.detach()
        self.loss_sum += loss
        return loss

    def _before_capture(self, static_in, static_lab):
        # a model that can use the NEXT batch's ids (DeepFM.prefetch_next: the step's weight-gradient launch touches that
        # batch's table rows in extra workgroups) reads them from a static buffer the caller refreshes per step
        self._static_next = static_in.clone() if self._prefetches else None
        for opt in self.optimizers:
            opt.zero_grad(set_to_none=True)        # the captured backward allocates the gradients in the graph's pool
        if self._static_next is not None:
            self.model.prefetch_next(self._static_next)

    def __call__(self, inputs: torch.Tensor, labels: torch.Tensor, next_inputs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """next_inputs (optional): the batch of the FOLLOWING step, already on the device — a loop that is one batch ahead of
        the step (train_epoch is) lets the step pull that batch's table rows into the Infinity Cache."""
        if not inputs.is_cuda:
            raise RuntimeError("GraphedTrainStep runs on the GPU: move the batch to the model's device first")
        if self.loss_sum is None:
            self.loss_sum = torch.zeros((), dtype=torch.float32, device=inputs.device)
            self.extra_sum = torch.zeros((), dtype=torch.float32, device=inputs.device)
            self._one = losses.unit_scalar(inputs.device)
        self.steps += 1
        if self._replayed.ready(inputs, labels):
            if self._static_next is not None and next_inputs is not None and next_inputs.shape == self._static_next.shape:
                self._static_next.copy_(next_inputs, non_blocking=True)
            self.last_loss = self._replayed.replay(inputs, labels)
        else:
            if self._prefetches and next_inputs is not None and next_inputs.shape == inputs.shape:
                self.model.prefetch_next(next_inputs)
            self.last_loss = self._body(inputs, labels)
        return self.last_loss


def train_epoch(dataloader, model, optimizers: Union[List[torch.optim.Optimizer], torch.optim.Optimizer], device="cuda",
                log_step=10, profiler=None, clip_grad=0, step: Optional[GraphedTrainStep] = None) -> Dict[str, float]:
    """src/trainer/deepfm.py:17-93.  Pass the same `step` object to successive epochs to keep one captured graph."""
    if not isinstance(optimizers, list):
        optimizers = [optimizers]
    model.train()
    model.to(device)
    if step is None:
        step = GraphedTrainStep(model, optimizers, clip_grad=clip_grad)
    first_steps = step.steps
    first_sum = float(step.loss_sum) if step.loss_sum is not None else 0.0
    load_data_time, train_time = datetime.timedelta(), datetime.timedelta()
    first_start = start = now()
    idx = -1
    # one batch ahead of the step (the DataLoader's workers are anyway): the step is told the next batch's ids
    batches = iter(dataloader)

    def fetch():
        batch = next(batches, None)
        return None if batch is None else (batch[0].to(device, non_blocking=True), batch[1].to(device, non_blocking=True))

    ahead = fetch()
    while ahead is not None:
        idx += 1
        (inputs, labels), ahead = ahead, fetch()
        load_data_time += now() - start
        start_train = now()
        step(inputs, labels, next_inputs=ahead[0] if ahead is not None else None)
        if log_step and idx % log_step == 0:
            logger.info("Idx: %d - loss: %.4g", idx, (float(step.loss_sum) - first_sum) / (idx + 1))
            _check_errors(model)             # the reference's nn.Embedding raises on the offending batch; here at the next sync
        if profiler:
            profiler.step()
        end_train = start = now()
        train_time += end_train - start_train
    n = step.steps - first_steps
    loss_dict = {"loss": (float(step.loss_sum) - first_sum) / n if n else 0.0}
    _check_errors(model)
    logger.info("train_time: %s", train_time)
    logger.info("load_data_time: %s", load_data_time)
    logger.info("total_time: %s", now() - first_start)
    return loss_dict


def _run_epoch(dataloader, device, log_step, profiler, step, log=None) -> int:
    """What the training loops share: `step(*batch)` for every batch of the loader, its tensors (or lists of tensors:
    NeuMF's negatives) moved to the device; at the logging steps `log(idx)` (a true return ends the epoch there) and the
    deferred index check; the profiler stepped.  Returns the number of batches stepped."""
    n = 0
    for idx, batch in enumerate(dataloader):
        step(*[[t.to(device, non_blocking=True) for t in part] if isinstance(part, (list, tuple))
               else part.to(device, non_blocking=True) for part in batch])
        n = idx + 1
        if log_step and idx % log_step == 0:
            stop = log is not None and log(idx)
            _lib.check_index_errors()
            if stop:
                break
        if profiler:
            profiler.step()
    return n


def _mean_since(sums: torch.Tensor, first: Optional[torch.Tensor], n: int) -> List[float]:
    """The running device sums, less what they held when the epoch began (`first`; None: nothing), over n batches."""
    return ((sums - first if first is not None else sums) / max(n, 1)).tolist()


def train_epoch_cerp(dataloader, model, optimizer, device="cuda", log_step=10, profiler=None, clip_grad=0,
                     target_sparsity=0.8, prune_loss_weight=0, step: Optional[GraphedTrainStep] = None) -> Dict[str, float]:
    """src/trainer/deepfm.py:142-248: `train_epoch` plus `prune_loss_weight * model.embedding.get_prune_loss()` in the
    loss, the table's sparsity checked at the logging steps, and an early return (running sums, as in the reference) once
    it reaches `target_sparsity`.  Returns {"loss", "prune_loss", "log_loss", "sparsity", "num_params"}."""
    model.train()
    model.to(device)
    if step is None:
        step = GraphedTrainStep(model, optimizer, clip_grad=clip_grad, extra_loss=lambda: model.embedding.get_prune_loss(),
                                extra_weight=prune_loss_weight)
    first = (float(step.loss_sum), float(step.extra_sum)) if step.loss_sum is not None else (0.0, 0.0)
    early = {}

    def sums():
        log_loss, prune = float(step.loss_sum) - first[0], float(step.extra_sum) - first[1]
        return {"loss": log_loss + prune_loss_weight * prune, "prune_loss": prune, "log_loss": log_loss}

    def log(idx):
        sparsity, num_params = model.embedding.get_sparsity(get_n_params=True)
        running = sums()
        logger.info("Idx: %d - loss: %.4g - sparsity: %.4g - num_params: %d", idx, running["loss"] / (idx + 1), sparsity,
                    num_params)
        if sparsity >= target_sparsity:
            early.update(running, sparsity=sparsity, num_params=num_params)
        return bool(early)

    n = _run_epoch(dataloader, device, log_step, profiler, step, log)
    if early:
        return early
    sparsity, num_params = model.embedding.get_sparsity(get_n_params=True)
    _lib.check_index_errors()
    return dict({k: v / max(n, 1) for k, v in sums().items()}, sparsity=sparsity, num_params=num_params)


def train_epoch_pep_deepfm(dataloader, model, optimizer, device="cuda", log_step=10, profiler=None, clip_grad=0,
                           step: Optional[GraphedTrainStep] = None) -> Dict[str, float]:
    """scripts/deepfm/train_deepfm_pep.py:23-80 of the reference: `train_epoch` on a PEP table; at every logging step the
    table's sparsity is read and logged and `model.embedding.train_callback()` writes the milestone files
    {checkpoint_weight_dir}/{sparsity}.pth it has passed.  Returns the reference's averaged "loss" plus the table's
    "sparsity" / "num_params" after the epoch.  Pass the same `step` to successive epochs to keep one captured graph."""
    model.train()
    model.to(device)
    if step is None:
        step = GraphedTrainStep(model, optimizer, clip_grad=clip_grad)
    first = float(step.loss_sum) if step.loss_sum is not None else 0.0

    def log(idx):
        with torch.no_grad():
            sparsity, num_params = model.embedding.get_sparsity(True)
        logger.info("Idx: %d - params: %d - sparsity: %.2g - loss: %.4g", idx, num_params, sparsity,
                    (float(step.loss_sum) - first) / (idx + 1))
        model.embedding.train_callback()

    n = _run_epoch(dataloader, device, log_step, profiler, step, log)
    _lib.check_index_errors()
    with torch.no_grad():
        sparsity, num_params = model.embedding.get_sparsity(True)
    return {"loss": ((float(step.loss_sum) - first) / n) if n else 0.0, "sparsity": sparsity, "num_params": num_params}


def train_epoch_optembed_deepfm(dataloader, model, optimizers, device="cuda", log_step=10, profiler=None, clip_grad=0,
                                alpha=0) -> Dict[str, float]:
    """scripts/deepfm/train_deepfm_optembed.py:21-112 of the reference: a DeepFM epoch on the OptEmbed supernet, eager,
    with a list of optimizers (the thresholds usually get their own); loss = BCEWithLogits + alpha *
    model.embedding.get_l_s().  Returns the averaged "loss" and "loss_s" (unweighted) and the table's "sparsity" /
    "num_params" after the epoch."""
    if not isinstance(optimizers, (list, tuple)):
        optimizers = [optimizers]
    model.train()
    model.to(device)
    criterion = losses.BCEWithLogitsLoss()
    sums = torch.zeros(2, dtype=torch.float32, device=device)          # loss, loss_s
    one = losses.unit_scalar(device)

    def log(idx):
        sparsity, num_params = model.embedding.get_sparsity(get_n_params=True)
        avg = _mean_since(sums, None, idx + 1)
        logger.info("Idx: %d - loss: %.4g - loss_s: %.4g - sparsity: %.4g - num_params: %d", idx, avg[0], avg[1], sparsity,
                    num_params)

    def batch(inputs, labels):
        loss_s = model.embedding.get_l_s()
        loss = criterion(model(inputs), labels.float()) + alpha * loss_s
        for opt in optimizers:
            opt.zero_grad()
        loss.backward(one)
        if clip_grad:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad)
        for opt in optimizers:
            opt.step()
        sums.add_(torch.stack([loss.detach(), torch.as_tensor(loss_s, dtype=torch.float32, device=device).detach()]))

    avg = _mean_since(sums, None, _run_epoch(dataloader, device, log_step, profiler, batch, log))
    _lib.check_index_errors()
    sparsity, num_params = model.embedding.get_sparsity(get_n_params=True)
    return {"loss": avg[0], "loss_s": avg[1], "sparsity": sparsity, "num_params": num_params}


class GraphedForward:
    """model(x) under no_grad with the forward of each input shape seen twice replayed as a hipGraph (the first call of a
    shape runs eagerly).  The returned tensor is the graph's static output: consume it before the next call."""

    def __init__(self, model: torch.nn.Module, use_graph: bool = True):
        self.model, self.use_graph = model, use_graph
        self._graphs: Dict[tuple, _Replayed] = {}

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not self.use_graph or not x.is_cuda:
            return self.model(x)
        key = (tuple(x.shape), x.dtype)
        forward = self._graphs.get(key)
        if forward is None:
            forward = self._graphs[key] = _Replayed(self.model, 1, "the forward", eager="launches")
        out = forward(x)
        self.use_graph = forward.enabled          # a failed capture turns the graphs of every shape off
        return out


@torch.no_grad()
def validate_epoch(val_loader, model, device="cuda", forward: Optional[GraphedForward] = None,
                   metric: Optional[CTRMetric] = None) -> Dict[str, float]:
    """src/trainer/deepfm.py:96-139: {"auc", "log_loss"}; labels and logits stay on the device (one append launch per
    batch, ctr_metric.CTRMetric), the forward of the full-size batches is replayed as a hipGraph.  `forward` (optional): a
    GraphedForward of this model to keep using; `metric` (optional): a CTRMetric on `device` to keep using (it is reset
    here) — the mask search scores every candidate through one of each (evol_search_deepfm)."""
    model.eval()
    model = model.to(device)
    if forward is None:
        forward = GraphedForward(model)
    if metric is None:
        dataset = getattr(val_loader, "dataset", None)
        metric = CTRMetric(device, capacity=len(dataset) if hasattr(dataset, "__len__") else None)
    else:
        metric.reset()
    for inputs, labels in val_loader:
        inputs, labels = inputs.to(device), labels.to(device)
        metric.add(forward(inputs), labels)
    _lib.check_index_errors()
    return metric.compute()


# --------------------------------------------------------------------------------------------------------------------
# collaborative filtering (LightGCN): reference src/trainer/lightgcn.py:14-165, 378-421
def cf_step_losses(model, adj, users, pos_items, neg_items, weight_decay: float = 0, info_nce_weight: float = 0,
                   fused_reg: bool = True, zero: Optional[torch.Tensor] = None):
    """(loss, rec_loss, reg_loss, cl_loss) of one LightGCN batch as the reference's `_train_step` forms them
    (src/trainer/lightgcn.py:378-421): propagate, BPR over the batch rows, `weight_decay * get_reg_loss`, optional InfoNCE
    (`cl_loss` comes weighted).  fused_reg: with a weight decay, let a model that has `forward_with_reg_loss` compute the
    regulariser inside the propagation and add it inside the BPR launch.  zero: a resident 0-dim zero of the caller's, to
    save the fill.  No host sync, no shape that depends on data."""
    fused = fused_reg and weight_decay > 0 and hasattr(model, "forward_with_reg_loss")
    if fused:      # propagation + regulariser as one node: the regulariser's gradient rows join the propagation's; every
        # term below reads the propagated tables at the batch's rows only, so the last layer computes only those
        all_user_emb, all_item_emb, reg_loss = model.forward_with_reg_loss(adj, users, pos_items, neg_items,
                                                                           batch_rows_only=True)
        # rec_loss + weight_decay * reg_loss out of the BPR launch itself (no scale / add launches)
        loss, rec_loss = losses.bpr_loss_rows(all_user_emb, all_item_emb, users, pos_items, neg_items, plus=reg_loss,
                                              plus_weight=weight_decay, return_parts=True)
    else:
        all_user_emb, all_item_emb = model(adj)
        rec_loss = losses.bpr_loss_rows(all_user_emb, all_item_emb, users, pos_items, neg_items)
    if zero is None:
        zero = torch.zeros((), device=rec_loss.device)
    if not fused:
        reg_loss = model.get_reg_loss(users, pos_items, neg_items) if weight_decay > 0 else zero
    cl_loss = _cf_info_nce(all_user_emb, all_item_emb, users, pos_items, info_nce_weight) if info_nce_weight > 0 else zero
    if not fused:
        loss = rec_loss + weight_decay * reg_loss + cl_loss
    elif info_nce_weight > 0:
        loss = loss + cl_loss
    return loss, rec_loss, reg_loss, cl_loss


def _cf_info_nce(all_user_emb, all_item_emb, users, pos_items, info_nce_weight, user_valid=None):
    """SGL without augmentation (src/trainer/lightgcn.py:405-417), weighted: view1 = rows of the batch's DISTINCT users and
    positives; here: all batch rows, repeats masked out (the loss is a mean over rows of a softmax over columns: the
    order of the rows is immaterial), so no shape depends on data."""
    view = torch.cat([torch.index_select(all_user_emb, 0, users), torch.index_select(all_item_emb, 0, pos_items)], 0)
    if user_valid is None:
        user_valid = losses.first_occurrence(users, all_user_emb.shape[0])
    valid = torch.cat([user_valid, losses.first_occurrence(pos_items, all_item_emb.shape[0])])
    return losses.info_nce(view, view, 0.2, valid=valid) * info_nce_weight


def _negatives_2d(neg_items, like: torch.Tensor) -> torch.Tensor:
    """[B, K] from what the CF loaders hand over: [B], [B, K], or a list of K [B] tensors (stacked on dim 1, as
    src/models/embeddings/cerp_embedding_utils.py:106-110 does)."""
    if isinstance(neg_items, (list, tuple)):
        neg_items = torch.stack(list(neg_items), dim=1)
    elif neg_items.dim() == 1:
        neg_items = neg_items.unsqueeze(1)
    return neg_items.to(like.device)


def cf_cerp_step_losses(model, adj, users, pos_items, neg_items, weight_decay: float = 0, info_nce_weight: float = 0,
                        prune_loss_weight: float = 0):
    """(loss, rec_loss, reg_loss, cl_loss, prune_loss) of one CERP batch on LightGCN / SingleLightGCN as
    `train_epoch_cerp` forms them (src/models/embeddings/cerp_embedding_utils.py:99-149): K negatives per positive through
    `bpr_loss_multi`, the regulariser and the tanh prune loss over the batch's rows of the INPUT tables (users
    de-duplicated for the prune term), optional InfoNCE (`cl_loss` comes weighted, `prune_loss` unweighted).

    Each table's `get_weight()` is taken ONCE and shared by the propagation and the batch-row terms
    (`losses.reg_prune_loss_rows`: no second lookup, no torch.unique); the BPR term reads the B * K triples straight
    from the propagated tables (no [B, K, D] gather).  No host sync, no shape that depends on data."""
    from . import _kernels
    from .lightgcn import LightGCN, SingleLightGCN

    neg = _negatives_2d(neg_items, users)
    B, K = neg.shape
    matrix = model.sparse_dropout(adj)
    if isinstance(model, LightGCN):
        user_table, item_table = model.user_emb_table.get_weight(), model.item_emb_table.get_weight()
        all_user_emb, all_item_emb = _kernels.lightgcn_propagate(matrix, user_table, item_table, model.num_layers)
    elif isinstance(model, SingleLightGCN):
        table = model.emb_table.get_weight()
        sizes = (model._num_user, model._num_item)
        all_user_emb, all_item_emb = torch.split(_kernels.lightgcn_propagate(matrix, table, None, model.num_layers), sizes)
        user_table, item_table = torch.split(table, sizes)
    else:
        raise ValueError(f"Not supported model for prune loss {model}")
    neg_flat = neg.reshape(-1)
    users_k, pos_k = (users, pos_items) if K == 1 else (users.repeat_interleave(K), pos_items.repeat_interleave(K))
    # bpr_loss_multi: the sum over the K negatives, averaged over the B samples = K times the mean over the B * K triples
    rec_loss = losses.bpr_loss_rows(all_user_emb, all_item_emb, users_k, pos_k, neg_flat)
    if K != 1:
        rec_loss = rec_loss * K
    user_valid = losses.first_occurrence(users, user_table.shape[0])
    reg_loss, prune_loss = losses.reg_prune_loss_rows(user_table, item_table, users, pos_items, neg_flat, user_valid)
    loss = rec_loss + weight_decay * reg_loss + prune_loss * prune_loss_weight
    cl_loss = torch.zeros((), device=rec_loss.device)
    if info_nce_weight > 0:
        cl_loss = _cf_info_nce(all_user_emb, all_item_emb, users, pos_items, info_nce_weight, user_valid)
        loss = loss + cl_loss
    return loss, rec_loss, reg_loss, cl_loss, prune_loss


CERP_CLIP_GRAD_NORM = 100      # cerp_embedding_utils.py:98


def train_epoch_cerp_cf(dataloader, model, optimizer, device="cuda", log_step=10, weight_decay=0, profiler=None,
                        info_nce_weight=0, prune_loss_weight=0, target_sparsity=0.8, step=None) -> Dict[str, float]:
    """src/models/embeddings/cerp_embedding_utils.py:65-218 (`train_epoch_cerp`): a LightGCN / SingleLightGCN epoch on CERP
    tables — several negatives per positive, the tanh prune loss, gradients clipped at norm 100, and the tables'
    sparsity read at the logging steps.  Once it reaches `target_sparsity` the epoch returns AT ONCE with the running
    SUMS (what the reference returns there); otherwise the averages over the batches.  Keys: "loss", "reg_loss",
    "rec_loss", "cl_loss" (weighted), "prune_loss" (unweighted), "sparsity", "num_params".  Eager; the sums stay on
    the device and are read at the logging steps only.
    step (optional, for tests): a callable (users, pos_items, neg_items) -> the five losses of a batch it has already
    stepped the optimizer for, in place of the built-in step."""
    model.train()
    model.to(device)
    keys = ("loss", "reg_loss", "rec_loss", "cl_loss", "prune_loss")
    sums = torch.zeros(len(keys), dtype=torch.float32, device=device)
    if step is None:
        adj = dataloader.dataset.get_norm_adj().to(device)
        one = losses.unit_scalar(device)

        def step(users, pos_items, neg_items):
            loss, rec_loss, reg_loss, cl_loss, prune_loss = cf_cerp_step_losses(
                model, adj, users, pos_items, neg_items, weight_decay, info_nce_weight, prune_loss_weight)
            optimizer.zero_grad()
            loss.backward(one)
            torch.nn.utils.clip_grad_norm_(model.parameters(), CERP_CLIP_GRAD_NORM)
            optimizer.step()
            return loss, rec_loss, reg_loss, cl_loss, prune_loss

    def batch(users, pos_items, neg_items):
        loss, rec_loss, reg_loss, cl_loss, prune_loss = step(users, pos_items, neg_items)
        sums.add_(torch.stack([t.detach().float() for t in (loss, reg_loss, rec_loss, cl_loss, prune_loss)]))

    early = {}

    def log(idx):
        sparsity, num_params = get_sparsity_and_param(model)
        running = dict(zip(keys, sums.tolist()))
        logger.info("Idx: %d - sparsity: %.2g - num_params: %d - loss: %.2g - prune_loss: %.2g", idx, sparsity, num_params,
                    running["loss"] / (idx + 1), running["prune_loss"] / (idx + 1))
        if sparsity >= target_sparsity:
            early.update(running, sparsity=sparsity, num_params=num_params)
        return bool(early)

    n = _run_epoch(dataloader, device, log_step, profiler, batch, log)
    if early:
        return early
    _lib.check_index_errors()
    sparsity, num_params = get_sparsity_and_param(model)
    return dict(zip(keys, _mean_since(sums, None, n)), sparsity=sparsity, num_params=num_params)


class GraphedCFTrainStep:
    """step(users, pos_items, neg_items): one LightGCN optimisation step as the reference's `_train_step` does it —
    propagate, BPR over the batch rows, `weight_decay * get_reg_loss`, optional InfoNCE on the batch's distinct rows,
    zero_grad, backward, optimizer step — replayed as one hipGraph for the batch size seen first (other sizes run eagerly
    on the same kernels).  The reference's `torch.unique` (a data-dependent shape) is replaced by a first-occurrence mask.

    `sums` (device tensor [4]) accumulates loss, rec_loss, reg_loss, cl_loss; `steps` counts the calls."""

    def __init__(self, model, adj, optimizer, weight_decay: float = 0, info_nce_weight: float = 0, warmup: int = 2,
                 use_graph: bool = True):
        self.model, self.adj, self.optimizer = model, adj, optimizer
        self.weight_decay, self.info_nce_weight = weight_decay, info_nce_weight
        if use_graph and not _capturable([optimizer]):
            warnings.warn("the optimizer keeps its step count on the host (capturable=False): the LightGCN step runs "
                          "eagerly; use recsys_benchmark_amd.optim.Adam")
            use_graph = False
        self.steps = 0
        self.sums: Optional[torch.Tensor] = None
        self._replayed = _Replayed(self._body, warmup, "the LightGCN step",
                                   lambda *static: self.optimizer.zero_grad(set_to_none=True), use_graph)

    warmup = property(lambda self: self._replayed.warmup)
    use_graph = property(lambda self: self._replayed.enabled)
    _graph = property(lambda self: self._replayed.graph)

    def _body(self, users, pos_items, neg_items):
        loss, rec_loss, reg_loss, cl_loss = cf_step_losses(self.model, self.adj, users, pos_items, neg_items,
                                                            self.weight_decay, self.info_nce_weight, fused_reg=True)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward(self._one)
        self.optimizer.step()
        parts = torch.stack([loss.detach(), rec_loss.detach(), reg_loss.detach(), cl_loss.detach()])
        self.sums += parts
        return parts

    def __call__(self, users, pos_items, neg_items) -> torch.Tensor:
        if self.sums is None:
            self.sums = torch.zeros(4, dtype=torch.float32, device=users.device)
            self._one = losses.unit_scalar(users.device)
        self.steps += 1
        return self._replayed(users, pos_items, neg_items)


def _cf_epoch(dataloader, model, optimizer, device, log_step, weight_decay, profiler, info_nce_weight, step, log=None):
    """train_epoch_cf, with `log(idx)` (see _run_epoch) in the place of its logging line when one is given."""
    model.train()
    model.to(device)
    if step is None:
        adj = dataloader.dataset.get_norm_adj().to(device)
        step = GraphedCFTrainStep(model, adj, optimizer, weight_decay, info_nce_weight)
    first = step.sums.clone() if step.sums is not None else None

    def log_losses(idx):
        logger.info("Idx: %d - loss: %.2g - rec_loss: %.2g", idx, *_mean_since(step.sums, first, idx + 1)[:2])

    n = _run_epoch(dataloader, device, log_step, profiler, step, log or log_losses)
    avg = _mean_since(step.sums, first, n) if step.sums is not None else [0.0] * 4
    _lib.check_index_errors()
    return {"loss": avg[0], "rec_loss": avg[1], "reg_loss": avg[2], "cl_loss": avg[3]}


def train_epoch_cf(dataloader, model, optimizer, device="cuda", log_step=10, weight_decay=0, profiler=None,
                   info_nce_weight=0, step: Optional[GraphedCFTrainStep] = None) -> Dict[str, float]:
    """src/trainer/lightgcn.py:14-77 (`train_epoch`): {"loss", "reg_loss", "rec_loss", "cl_loss"} averaged over the
    batches.  `dataloader.dataset.get_norm_adj()` supplies the normalised adjacency, as in the reference."""
    return _cf_epoch(dataloader, model, optimizer, device, log_step, weight_decay, profiler, info_nce_weight, step)


def train_epoch_pep(dataloader, model, optimizer, device="cuda", log_step=10, weight_decay=0, profiler=None,
                    info_nce_weight=0, target_sparsity=0, step: Optional[GraphedCFTrainStep] = None) -> Dict[str, float]:
    """src/trainer/lightgcn.py:294-375: `train_epoch` for a LightGCN on PEP tables — the tables' sparsity is read at the
    logging steps (`get_sparsity_and_param`) and the epoch ends early once it exceeds `target_sparsity`.  Returns the
    four averaged losses plus "sparsity" / "num_params" of the last check."""
    extra = {}

    def log(idx):
        sparsity, num_params = get_sparsity_and_param(model)
        extra.update(sparsity=sparsity, num_params=num_params)
        logger.info("Idx: %d - sparsity: %.2f - num_params: %d", idx, sparsity, num_params)
        if sparsity > target_sparsity:
            logger.info("Found target sparsity")
            return True

    avg = _cf_epoch(dataloader, model, optimizer, device, log_step, weight_decay, profiler, info_nce_weight, step, log)
    return dict(avg, **extra)


def train_epoch_optembed(dataloader, model, optimizers, device="cuda", log_step=10, weight_decay=0, profiler=None,
                         info_nce_weight=0, alpha=0) -> Dict[str, float]:
    """src/trainer/lightgcn.py:162-290: a LightGCN / SingleLightGCN epoch on OptEmbed tables, eager, with a list of
    optimizers; loss = bpr + weight_decay * reg + info_nce + alpha * sum of the tables' get_l_s().  Each training
    get_weight draws its dimension mask on the device.  Returns the averaged "loss", "reg_loss" (unweighted),
    "rec_loss", "cl_loss" (weighted), "loss_s", and "sparsity" / "n_params" after the epoch."""
    from .embeddings.cf_opt_embed import IOptEmbed

    if not isinstance(optimizers, (list, tuple)):
        optimizers = [optimizers]
    adj = dataloader.dataset.get_norm_adj().to(device)
    model.train()
    model.to(device)
    tables = [emb for _, emb in model.get_embs()]
    assert all(isinstance(t, IOptEmbed) for t in tables), "train_epoch_optembed needs OptEmbed tables"
    sums = torch.zeros(5, dtype=torch.float32, device=device)          # loss, reg_loss, rec_loss, cl_loss, loss_s
    one = losses.unit_scalar(device)
    zero = torch.zeros((), device=device)

    def log(idx):
        sparsity, n_params = get_sparsity_and_param(model)
        avg = _mean_since(sums, None, idx + 1)
        logger.info("Idx: %d - sparsity=%.4f - n_params=%d - loss: %.4g - loss_s: %.4g", idx, sparsity, n_params,
                    avg[0], avg[4])

    def batch(users, pos_items, neg_items):
        loss, rec_loss, reg_loss, cl_loss = cf_step_losses(model, adj, users, pos_items, neg_items, weight_decay,
                                                            info_nce_weight, fused_reg=False, zero=zero)
        loss_s = zero
        for t in tables:
            loss_s = loss_s + t.get_l_s().to(device)
        loss = loss + alpha * loss_s
        for opt in optimizers:
            opt.zero_grad()
        loss.backward(one)
        for opt in optimizers:
            opt.step()
        sums.add_(torch.stack([loss.detach(), reg_loss.detach(), rec_loss.detach(), cl_loss.detach(), loss_s.detach()]))

    avg = _mean_since(sums, None, _run_epoch(dataloader, device, log_step, profiler, batch, log))
    _lib.check_index_errors()
    sparsity, n_params = get_sparsity_and_param(model)
    return {"loss": avg[0], "reg_loss": avg[1], "rec_loss": avg[2], "cl_loss": avg[3], "loss_s": avg[4],
            "sparsity": sparsity, "n_params": n_params}


def ndcg_recall_at_k(y_pred: torch.Tensor, y_true: Sequence[Union[Sequence[int], set]], k: int = 20) -> Tuple[float, float]:
    """src/metrics.py:9-43, 70-108 (`get_ndcg`, `get_ndcg_recall`) for a [users, >=k] tensor of recommended item ids:
    the relevance test is one broadcast comparison against the padded true-item lists on y_pred's device, float64."""
    dev = y_pred.device
    n = len(y_true)
    if n == 0 or y_pred.shape[0] != n:
        raise ValueError("y_pred must hold one row of recommendations per entry of y_true")
    lens = torch.tensor([len(t) for t in y_true], dtype=torch.int64)
    width = max(int(lens.max()), 1)
    padded = torch.full((n, width), -1, dtype=torch.int64)
    for i, t in enumerate(y_true):
        if len(t):
            padded[i, :len(t)] = torch.as_tensor(sorted(t) if isinstance(t, (set, frozenset)) else list(t), dtype=torch.int64)
    padded, lens = padded.to(dev), lens.to(dev)
    pred = y_pred[:, :k]
    relevant = (pred.unsqueeze(2) == padded.unsqueeze(1)).any(2).to(torch.float64)          # [n, k]
    weight = 1.0 / torch.log2(torch.arange(2, pred.shape[1] + 2, dtype=torch.float64, device=dev))
    dcg = (relevant * weight).sum(1)
    length = torch.clamp(lens, max=k)
    ideal = torch.cumsum(1.0 / torch.log2(torch.arange(2, k + 2, dtype=torch.float64, device=dev)), 0)
    idcg = ideal[(length - 1).clamp(min=0)]
    ndcg = (dcg / idcg).mean()
    recall = (relevant.sum(1) / length.to(torch.float64)).mean()
    return float(ndcg), float(recall)


def _ranking_metrics(val_loader, topk, device, k: int, metrics: Optional[List[str]], profiler) -> Dict[str, float]:
    """What the ranking validations share: `topk(users)` ([users, k] item ids) for every batch of the loader, then
    {"ndcg"}, or {"ndcg", "recall"} when `metrics` names both.  A loader that hands over a `DeviceTruth` (cf_data.py) has
    the metric taken by mi_ndcg_recall_rows against its CSR; Python sets go through `ndcg_recall_at_k`."""
    preds, truths, asked, resident = [], [], [], None
    for users, pos_items in val_loader:
        users = torch.as_tensor(users).to(device)
        preds.append(topk(users))
        if isinstance(pos_items, DeviceTruth):         # a DeviceCFTestLoader: the truth CSR stays where it is
            resident = pos_items
            asked.append(users)
        else:
            truths.extend(pos_items)
        if profiler:
            profiler.step()
    if resident is not None:
        if truths:
            raise ValueError("a validation loader must hand over either truth sets or a DeviceTruth, not both")
        ndcg, recall = resident.ndcg_recall(torch.cat(preds), torch.cat(asked), k)
    else:
        ndcg, recall = ndcg_recall_at_k(torch.cat(preds), truths, k)
    _lib.check_index_errors()
    if metrics is not None and "ndcg" in metrics and "recall" in metrics:
        return {"ndcg": ndcg, "recall": recall}
    return {"ndcg": ndcg}


@torch.no_grad()
def validate_epoch_cf(train_dataset, val_loader, model, device="cuda", k=20, filter_item_on_train=True, profiler=None,
                      metrics: Optional[List[str]] = None) -> Dict[str, float]:
    """src/trainer/lightgcn.py:80-165 (`validate_epoch`): {"ndcg"} or {"ndcg", "recall"}.  Scores, the train-item mask
    (a CSR of `train_dataset.get_graph()` built once, not a Python loop per batch) and the top-k run in `score_topk`;
    the recommendations stay on the device until the metric."""
    adj = train_dataset.get_norm_adj().to(device)
    graph = train_dataset.get_graph()
    model.eval()
    model = model.to(device)
    user_embs, item_embs = model(adj)
    csr = train_items_csr(graph, user_embs.shape[0], device) if filter_item_on_train else None
    return _ranking_metrics(val_loader, lambda users: score_topk(user_embs, item_embs, users, k, csr), device, k, metrics,
                            profiler)


# --------------------------------------------------------------------------------------------------------------------
# NeuMF: reference src/trainer/nmf.py:232-281, 446-582
def nmf_step_losses(model, users, pos_items, neg_items, weight_decay: float = 0):
    """(loss, rec_loss, reg_loss) of one NeuMF batch as `_train_step` forms them (src/trainer/nmf.py:446-486):
    `users.repeat(n_neg + 1)` against `cat([pos, neg])` in ONE forward, BCE(pos, 1) + BCE(neg, 0) (each a mean) and
    `weight_decay * get_reg_loss`.  `neg_items` is [B] or a list of [B] tensors.  No host sync, no shape that depends
    on data: capturable in torch.cuda.graph."""
    n_repeat = 1
    if isinstance(neg_items, (list, tuple)):
        n_repeat = len(neg_items)
        neg_items = torch.cat(list(neg_items))
    y_hat = model(users.repeat(n_repeat + 1), torch.cat([pos_items, neg_items]))
    B = pos_items.shape[0]
    y_pos, y_neg = y_hat[:B], y_hat[B:]
    bce = losses.BCEWithLogitsLoss()
    rec_loss = bce(y_pos, torch.ones_like(y_pos)) + bce(y_neg, torch.zeros_like(y_neg))
    if weight_decay > 0:
        reg_loss = model.get_reg_loss(users, pos_items, neg_items)
        loss = rec_loss + weight_decay * reg_loss
    else:
        reg_loss = torch.zeros((), device=rec_loss.device)
        loss = rec_loss
    return loss, rec_loss, reg_loss


def train_epoch_nmf(dataloader, model, optimizer, device="cuda", log_step=10, weight_decay=0, profiler=None) -> Dict[str, float]:
    """src/trainer/nmf.py:232-281 (`train_epoch`): {"loss", "rec_loss", "reg_loss"} averaged over the batches; the sums
    stay on the device and are read back at the logging steps only."""
    model.train()
    model.to(device)
    sums = torch.zeros(3, dtype=torch.float32, device=device)
    one = losses.unit_scalar(device)

    def log(idx):
        logger.info("Idx: %d - loss: %.2g - rec_loss: %.2g - reg_loss: %.2g", idx, *_mean_since(sums, None, idx + 1))

    def batch(users, pos_items, neg_items):
        loss, rec_loss, reg_loss = nmf_step_losses(model, users, pos_items, neg_items, weight_decay)
        optimizer.zero_grad()
        loss.backward(one)
        optimizer.step()
        sums.add_(torch.stack([loss.detach(), rec_loss.detach(), reg_loss.detach().float()]))

    avg = _mean_since(sums, None, _run_epoch(dataloader, device, log_step, profiler, batch, log))
    _lib.check_index_errors()
    return {"loss": avg[0], "rec_loss": avg[1], "reg_loss": avg[2]}


def nmf_prune_step_losses(model, users, pos_items, neg_items, weight_decay: float = 0, prune_loss_weight: float = 0):
    """(loss, rec_loss, reg_loss, prune_loss): `nmf_step_losses` plus `prune_loss_weight * model.get_prune_loss_tanh(...)`
    over the batch's rows, as `_train_step` adds it (src/trainer/nmf.py:483-487); `prune_loss` comes unweighted, a zero
    without a weight."""
    loss, rec_loss, reg_loss = nmf_step_losses(model, users, pos_items, neg_items, weight_decay)
    if prune_loss_weight > 0:
        neg = torch.cat(list(neg_items)) if isinstance(neg_items, (list, tuple)) else neg_items
        prune_loss = model.get_prune_loss_tanh(users, pos_items, neg)
        loss = loss + prune_loss * prune_loss_weight
    else:
        prune_loss = torch.zeros((), device=rec_loss.device)
    return loss, rec_loss, reg_loss, prune_loss


def _nmf_pruning_epoch(dataloader, model, optimizer, device, log_step, weight_decay, profiler, target_sparsity,
                       prune_loss_weight, clip_grad_norm, keys, step=None) -> Dict[str, float]:
    """What `train_epoch_pep` and `train_epoch_cerp` of src/trainer/nmf.py:284-443 share: the NeuMF step (with the prune
    term and the clipping when asked for), the tables' sparsity read at the logging steps, a `break` once it EXCEEDS
    `target_sparsity`, and the averages over the batches stepped."""
    from .neumf import get_sparsity_and_param as nmf_sparsity_and_param

    model.train()
    model.to(device)
    sums = torch.zeros(4, dtype=torch.float32, device=device)          # loss, rec_loss, reg_loss, prune_loss
    extra = {}
    if step is None:
        one = losses.unit_scalar(device)

        def step(users, pos_items, neg_items):
            parts = nmf_prune_step_losses(model, users, pos_items, neg_items, weight_decay, prune_loss_weight)
            optimizer.zero_grad()
            parts[0].backward(one)
            if clip_grad_norm > 0:
                torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad_norm)
            optimizer.step()
            return parts

    def batch(users, pos_items, neg_items):
        sums.add_(torch.stack([t.detach().float() for t in step(users, pos_items, neg_items)]))

    def log(idx):
        sparsity, num_params = nmf_sparsity_and_param(model)
        extra.update(sparsity=sparsity, num_params=num_params)
        logger.info("Idx: %d - sparsity: %.2f - num_params: %d - loss: %.2g", idx, sparsity, num_params,
                    _mean_since(sums, None, idx + 1)[0])
        if sparsity > target_sparsity:
            logger.info("Found target sparsity")
            return True

    avg = dict(zip(("loss", "rec_loss", "reg_loss", "prune_loss"),
                   _mean_since(sums, None, _run_epoch(dataloader, device, log_step, profiler, batch, log))))
    _lib.check_index_errors()
    return dict({k: avg[k] for k in keys}, **extra)


def train_epoch_pep_nmf(dataloader, model, optimizer, device="cuda", log_step=10, weight_decay=0, profiler=None,
                        target_sparsity=0, step=None) -> Dict[str, float]:
    """src/trainer/nmf.py:284-357 (`train_epoch_pep`): a NeuMF epoch on PEP tables — {"loss", "reg_loss", "rec_loss"}
    averaged over the batches stepped, plus "sparsity" / "num_params" of the last logging step; the epoch ends once the
    sparsity exceeds `target_sparsity`.  step: see train_epoch_cerp_cf (four losses, the last a zero)."""
    return _nmf_pruning_epoch(dataloader, model, optimizer, device, log_step, weight_decay, profiler, target_sparsity, 0, 0,
                              ("loss", "reg_loss", "rec_loss"), step)


def train_epoch_cerp_nmf(dataloader, model, optimizer, device="cuda", log_step=10, weight_decay=0, profiler=None,
                         target_sparsity=0, prune_loss_weight=0, clip_grad_norm=100, step=None) -> Dict[str, float]:
    """src/trainer/nmf.py:360-443 (`train_epoch_cerp`): `train_epoch_pep_nmf` with `prune_loss_weight *
    model.get_prune_loss_tanh(...)` in the loss and the gradients clipped at `clip_grad_norm`; adds "prune_loss"
    (unweighted) to the returned averages."""
    return _nmf_pruning_epoch(dataloader, model, optimizer, device, log_step, weight_decay, profiler, target_sparsity,
                              prune_loss_weight, clip_grad_norm, ("loss", "reg_loss", "rec_loss", "prune_loss"), step)


@torch.no_grad()
def validate_epoch_nmf(train_dataset, val_loader, model, device="cuda", k=20, filter_item_on_train=True, profiler=None,
                       metrics: Optional[List[str]] = None) -> Dict[str, float]:
    """src/trainer/nmf.py:501-582 (`validate_epoch`): {"ndcg"} or {"ndcg", "recall"}.  Every user of a batch is scored
    against every item by `neumf.score_all_items`, the train items are masked and the top-k taken by mi_mask_topk_rows
    (a CSR of `train_dataset.get_graph()` built once), the metric runs on the device."""
    from .neumf import score_all_items

    graph = train_dataset.get_graph()
    model.eval()
    model = model.to(device)
    csr = train_items_csr(graph, model.num_user, device) if filter_item_on_train else None
    crow, col = (None, None) if csr is None else csr

    def topk(users):
        users = users.to(torch.int64)
        scores = score_all_items(model, users)
        out = torch.empty((users.numel(), k), dtype=torch.int64, device=device)
        _lib.check(_lib.load().mi_mask_topk_rows(scores.data_ptr(), scores.stride(0), scores.shape[0], scores.shape[1],
                                                 users.data_ptr(), _lib.ptr(crow), _lib.ptr(col), k, out.data_ptr(), None,
                                                 _lib.stream_ptr(scores.device)), "mi_mask_topk_rows")
        return out

    return _ranking_metrics(val_loader, topk, device, k, metrics, profiler)

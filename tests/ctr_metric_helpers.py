"""numpy restatements of what csrc/ctr_metric.hip computes, for tests/test_ctr_metric_*.py."""
import numpy as np

BATCHES = (200, 200, 33, 1, 257, 4097)        # the batch sizes the CTRMetric tests feed


def score_keys(score: np.ndarray) -> np.ndarray:
    """The monotone uint32 key of float32 scores: -0.0 folded onto +0.0, then the usual sign flip."""
    b = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def auc_counts(score: np.ndarray, label: np.ndarray):
    """(S, P, N) as Python integers: S = sum over groups of equal key of pos_g * (2 * neg_below_g + neg_g)."""
    label = np.asarray(label).astype(np.int64)
    _, inverse = np.unique(score_keys(score), return_inverse=True)
    groups = int(inverse.max()) + 1
    pos = np.bincount(inverse[label == 1], minlength=groups).astype(np.int64)
    neg = np.bincount(inverse[label == 0], minlength=groups).astype(np.int64)
    neg_below = np.cumsum(neg) - neg
    S = sum(int(p) * (2 * int(b) + int(g)) for p, b, g in zip(pos, neg_below, neg) if p)
    return S, int(pos.sum()), int(neg.sum())


def bce_sum(logits: np.ndarray, labels: np.ndarray) -> float:
    """sum of max(x, 0) - x y + log1p(exp(-|x|)), every term in float64 from the float32 logit."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    y = np.asarray(labels).astype(np.float64)
    return float(np.sum(np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))))

"""NumPy / Python restatements of the vocabulary rule and of the batch shuffle p(j), written from the contract in
include/mi355x_recsys.h (not from csrc/ctr_data.hip): they are the specification the kernels' bits are compared with.

    mix64      = the splitmix64 finaliser; kGold = 0x9E3779B97F4A7C15, kSalt = 0xD1B54A32D192ED03
    bits       = max(2, bit_length(n - 1));  k = (bits + 1) / 2;  mask = (1 << k) - 1
    base       = mix64(seed + kGold * (epoch + 1))                       (mod 2^64 throughout)
    K[r]       = mix64(base + kSalt * (r + 1)),  r = 0..5
    step(x):   L = x >> k; R = x & mask; six times: (L, R) = (R, L ^ (mix64(K[r] + R) & mask)); return (L << k) | R
    p(j):      x = j; do x = step(x) while x >= n
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLE = os.path.join(GOLDEN, "criteo_sample.txt")
THRESHOLDS = (1, 2, 3, 10)
SUM_DIMS = {1: 1516, 2: 405, 3: 272, 10: 117}          # the reference mapper's sums of field_dims on the sample

G = 0x9E3779B97F4A7C15
S = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1


def mix64_scalar(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix64(z):
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def shuffle_keys(n, seed, epoch):
    """(k, mask, K[0..5]) of an epoch over n samples."""
    bits = max(2, (n - 1).bit_length())
    k = (bits + 1) // 2
    base = mix64_scalar(seed + G * (epoch + 1))
    return k, (1 << k) - 1, [mix64_scalar(base + S * (r + 1)) for r in range(6)]


def p_scalar(j, n, seed, epoch):
    """p(j) in Python integers, one step at a time."""
    k, mask, K = shuffle_keys(n, seed, epoch)
    x = j
    while True:
        L, R = x >> k, x & mask
        for r in range(6):
            L, R = R, L ^ (mix64_scalar(K[r] + R) & mask)
        x = (L << k) | R
        if x < n:
            return x


def p_restated(j, n, seed, epoch):
    """p over an array of positions (the same walk, the elements still at or above n stepped again)."""
    k, mask, K = shuffle_keys(n, seed, epoch)
    k, mask = np.uint64(k), np.uint64(mask)

    def step(x):
        L, R = x >> k, x & mask
        with np.errstate(over="ignore"):
            for r in range(6):
                L, R = R, L ^ (mix64(np.uint64(K[r]) + R) & mask)
        return (L << k) | R

    x = step(np.asarray(j).astype(np.uint64))
    while True:
        again = x >= np.uint64(n)
        if not again.any():
            return x.astype(np.int64)
        x[again] = step(x[again])


def batch_restated(records, index, first, count, epoch, seed, shuffle):
    """(x int64 [count, F], y float32 [count]) of samples [first, first + count)."""
    n = records.shape[0] if index is None else len(index)
    j = first + np.arange(count, dtype=np.int64)
    p = p_restated(j, n, seed, epoch) if shuffle and count else j
    rows = p if index is None else np.asarray(index)[p]
    return records[rows, 1:].astype(np.int64), records[rows, 0].astype(np.float32)


def encode_restated(keys, labels, threshold):
    """(records uint32 [n, 1 + F], field_dims int64 [F]): per field the keys seen at least `threshold` times numbered in
    ascending key order (np.unique sorts), every other key numbered `kept`."""
    keys = np.asarray(keys, dtype=np.int64)
    n, F = keys.shape
    records = np.zeros((n, 1 + F), dtype=np.uint32)
    records[:, 0] = labels
    dims = np.zeros(F, dtype=np.int64)
    for f in range(F):
        if n == 0:
            dims[f] = 1
            continue
        uniq, inverse, counts = np.unique(keys[:, f], return_inverse=True, return_counts=True)
        kept = counts >= threshold
        ids = np.where(kept, np.cumsum(kept) - 1, kept.sum())
        records[:, 1 + f] = ids[inverse.reshape(-1)]
        dims[f] = kept.sum() + 1
    return records, dims


def boundary_column(block=256):
    """n = 4 * block + 1 sorted-by-value keys in shuffled row order with a run of equal keys lying across every multiple of
    `block` of the sorted order: runs of 1, 2, 3, ... keys, then at each boundary a run that starts before it and ends
    after it (lengths 2, 5, 9, 12), so kept and dropped runs straddle workgroup tiles at thresholds 3 and 10."""
    n = 4 * block + 1
    key = np.zeros(n, dtype=np.int64)
    value, i, length = -5, 0, 1
    spans = {block: (block - 1, block + 1), 2 * block: (2 * block - 2, 2 * block + 3),
             3 * block: (3 * block - 4, 3 * block + 5), 4 * block: (4 * block - 11, 4 * block + 1)}
    starts = {a: b for a, b in spans.values()}
    while i < n:
        end = starts.get(i)
        if end is None:
            nxt = min([a for a in starts if a > i], default=n)
            end = min(i + length, nxt)
            length = length % 13 + 1
        key[i:end] = value
        value += 3
        i = end
    rng = np.random.default_rng(5)
    return key[rng.permutation(n)]

"""NumPy restatement of mi_cf_sample_triples and mi_ndcg_recall_rows, written from the contract in
include/mi355x_recsys.h (not from csrc/cf_data.hip): it is the specification the kernel's bits are compared with.

    base       = mix64(seed + G * (epoch + 1))
    key(i)     = mix64(base + S * (i + 1))                 i: index of the sample in the epoch
    bits(i, d) = mix64(key(i) + G * (d + 1))               d = 0: the positive (uniform mode), 1 + t: negative t
    value      = (bits * range) >> 64

`draw_scalar` / `sample_scalar` say it in Python integers, one sample at a time; `sample_restated` is the same thing over
arrays (the tests check the two against each other on the small graph and use the array form at size)."""
import numpy as np

G = 0x9E3779B97F4A7C15
S = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1


def mix64_scalar(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_scalar(seed, epoch, i, d, rng):
    base = mix64_scalar(seed + G * (epoch + 1))
    key = mix64_scalar(base + S * (i + 1))
    return (mix64_scalar(key + G * (d + 1)) * rng) >> 64


def mix64(z):
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mulhi(bits, rng):
    """(bits * rng) >> 64 for uint64 bits and ranges below 2^32."""
    rng = np.asarray(rng).astype(np.uint64)
    assert rng.size == 0 or int(rng.max()) < (1 << 32)
    lo, hi = bits & np.uint64(0xFFFFFFFF), bits >> np.uint64(32)
    return (hi * rng + ((lo * rng) >> np.uint64(32))) >> np.uint64(32)


def draws(seed, epoch, i, d, rng):
    with np.errstate(over="ignore"):
        base = np.uint64(mix64_scalar(seed + G * (epoch + 1)))
        key = mix64(base + np.uint64(S) * (np.asarray(i).astype(np.uint64) + np.uint64(1)))
        return mulhi(mix64(key + np.uint64((G * (d + 1)) & M64)), rng).astype(np.int64)


class HostGraph:
    """The arrays the kernel reads, built from a graph dict with plain loops."""

    def __init__(self, graph):
        self.graph = graph
        self.U = len(graph)
        assert sorted(graph) == list(range(self.U))
        self.pair_user = np.array([u for u, its in graph.items() for _ in its], dtype=np.int64)
        self.pair_item = np.array([i for its in graph.values() for i in its], dtype=np.int64)
        self.I = int(self.pair_item.max()) + 1
        self.P = self.pair_item.size
        self.per_user_num = self.P // self.U
        self.stored = np.array([i for u in range(self.U) for i in graph[u]], dtype=np.int64)
        self.pair_crow = np.zeros(self.U + 1, dtype=np.int64)
        self.pos_crow = np.zeros(self.U + 1, dtype=np.int64)
        rows = []
        for u in range(self.U):
            row = sorted(set(graph[u]))
            rows.append(row)
            self.pair_crow[u + 1] = self.pair_crow[u] + len(graph[u])
            self.pos_crow[u + 1] = self.pos_crow[u] + len(row)
        self.pos_col = np.array([i for row in rows for i in row], dtype=np.int64)
        self.pos_user = np.repeat(np.arange(self.U), np.diff(self.pos_crow))
        # g(j) = pos_col[j] - j inside a row is non-decreasing; with the user in front the whole array is sorted
        g = self.pos_col - (np.arange(self.pos_col.size) - self.pos_crow[self.pos_user])
        self.select_key = self.pos_user * (self.I + 1) + g

    def epoch_len(self, mode):
        return self.U * self.per_user_num if mode == "uniform" else self.P


def sample_scalar(hg, mode, K, i, seed, epoch, order_i=None):
    """(user, positive, [K negatives]) of sample i of the epoch, one step at a time in Python integers."""
    if mode == "popularity":
        p = i if order_i is None else order_i
        u, item = int(hg.pair_user[p]), int(hg.pair_item[p])
    else:
        u = i // hg.per_user_num
        stored = hg.graph[u]
        item = stored[draw_scalar(seed, epoch, i, 0, len(stored))]
    row = sorted(set(hg.graph[u]))
    if len(row) + K > hg.I:
        return -1, -1, [-1] * K
    free = [x for x in range(hg.I) if x not in set(row)]          # the non-positives, ascending: rank -> item
    picked, negs = [], []
    for t in range(K):
        r = draw_scalar(seed, epoch, i, 1 + t, len(free) - t)
        for p in sorted(picked):
            if r >= p:
                r += 1
        picked.append(r)
        negs.append(free[r])
    return u, item, negs


def sample_restated(hg, mode, K, first, n, seed, epoch, order=None, rank_as_item=False):
    """users [n], pos [n], neg [K, n] of samples [first, first + n).  rank_as_item: the deliberately WRONG variant that
    hands out the rank among the non-positives as if it were the item (what a kernel that forgot the rank-select does)."""
    i = first + np.arange(n, dtype=np.int64)
    if mode == "popularity":
        p = i if order is None else np.asarray(order, dtype=np.int64)
        users, pos = hg.pair_user[p].copy(), hg.pair_item[p].copy()
    else:
        users = i // hg.per_user_num
        lens = hg.pair_crow[users + 1] - hg.pair_crow[users]
        pos = hg.stored[hg.pair_crow[users] + draws(seed, epoch, i, 0, lens)]
    c0 = hg.pos_crow[users]
    deg = hg.pos_crow[users + 1] - c0
    bad = deg + K > hg.I
    free = np.where(bad, K, hg.I - deg)                           # (bad rows: any positive range; overwritten below)
    neg = np.empty((K, n), dtype=np.int64)
    picked = np.empty((n, 0), dtype=np.int64)
    for t in range(K):
        r = draws(seed, epoch, i, 1 + t, free - t)
        for j in range(t):                                        # picked is kept ascending along axis 1
            r = r + (r >= picked[:, j])
        picked = np.sort(np.concatenate([picked, r[:, None]], axis=1), axis=1)
        if rank_as_item:
            neg[t] = r
        else:
            at = np.searchsorted(hg.select_key, users * (hg.I + 1) + r, side="right")     # first entry with g > r
            neg[t] = r + (at - c0)
    users, pos = np.where(bad, -1, users), np.where(bad, -1, pos)
    neg[:, bad] = -1
    return users, pos, neg


def graph_from_pairs(users, items):
    """The graph dict of a list of (user, item) interactions, in their order."""
    graph = {}
    for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        graph.setdefault(u, []).append(i)
    return graph


def nearly_full_graph(K):
    """40 items; user 0 holds 10 of them, user 1 all but K (<= 3), user 2 a duplicated interaction."""
    return {0: [3, 4, 5, 11, 17, 18, 19, 30, 38, 39], 1: [i for i in range(40) if i not in (0, 13, 39)[:K]] + [7],
            2: [5, 7, 7, 9]}


def skewed_graph(U, I, nnz, seed):
    """A synthetic graph with item popularity ~ rank^-1/2-like skew (item = I * u^2) and every user present; duplicates
    of an interaction are kept, as a raw interaction file would hold them."""
    rng = np.random.default_rng(seed)
    users = np.concatenate([np.arange(U), rng.integers(0, U, nnz - U)])
    items = np.minimum((I * rng.random(nnz) ** 2).astype(np.int64), I - 1)
    items[0] = I - 1                                              # pins num_items = I
    order = np.argsort(users, kind="stable")
    users, items = users[order], items[order]
    cuts = np.flatnonzero(np.diff(users)) + 1
    return {u: its.tolist() for u, its in enumerate(np.split(items, cuts))}


def ndcg_recall_rows_restated(pred, users, crow, col, k):
    """Per-user (ndcg, recall) float64 with the definitions of src/metrics.py `get_ndcg_recall`: DCG summed in ascending
    j with weight 1 / log2(j + 2) (torch's float64 log2, as the library's host side computes it)."""
    import torch

    weight = (1.0 / torch.log2(torch.arange(2, k + 2, dtype=torch.float64))).numpy()
    ideal = torch.cumsum(torch.from_numpy(weight), 0).numpy()
    ndcg, recall = np.empty(len(users)), np.empty(len(users))
    for n, u in enumerate(users):
        truth = set(col[crow[u]:crow[u + 1]].tolist())
        dcg, hits = 0.0, 0
        for j in range(k):
            if int(pred[n, j]) in truth:
                dcg += weight[j]
                hits += 1
        length = min(len(truth), k)
        ndcg[n] = dcg / ideal[length - 1] if length else np.nan
        recall[n] = hits / length if length else np.nan
    return ndcg, recall


def chi2_sf(x, df):
    """P(chi-square with df degrees of freedom > x): the regularised upper incomplete gamma Q(df / 2, x / 2), by its
    series below a + 1 and by the Lentz continued fraction above (math only, so that the tests need no scipy)."""
    import math

    a, x = df / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    front = math.exp(a * math.log(x) - x - math.lgamma(a))
    if x < a + 1:
        term = total = 1.0 / a
        for n in range(1, 10000):
            term *= x / (a + n)
            total += term
            if term < total * 1e-17:
                break
        return 1.0 - front * total
    tiny = 1e-300
    b = x + 1 - a
    c, d = 1 / tiny, 1 / b
    h = d
    for n in range(1, 10000):
        an = -n * (n - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        delta = d * c
        h *= delta
        if abs(delta - 1) < 1e-16:
            break
    return front * h


def chi2_quantile(p_upper, df):
    """x with chi2_sf(x, df) = p_upper, by bisection."""
    lo, hi = 0.0, 10.0 * df + 1000.0
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if chi2_sf(mid, df) > p_upper else (lo, mid)
    return (lo + hi) / 2


def chi2_stat(counts):
    """Pearson's statistic of `counts` against the uniform law over its cells."""
    counts = np.asarray(counts, dtype=np.float64)
    expected = counts.sum() / counts.size
    return float(((counts - expected) ** 2).sum() / expected)

"""Ranking metrics of the eval loop (src/metrics.py:1-29, src/main.py:255-258): per-impression AUC / MRR / nDCG@k.
Own numpy implementation; AUC is the rank statistic (average ranks for ties) that sklearn's roc_auc_score computes."""
import numpy as np


def roc_auc_score(y_true, y_score):
    y_true = np.asarray(y_true)
    y_score = np.asarray(y_score, dtype=np.float64)
    n_pos = int(y_true.sum())
    n_neg = len(y_true) - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("AUC needs both classes")
    order = np.argsort(y_score, kind="mergesort")
    s = y_score[order]
    # average 1-based rank of every tie group
    starts = np.r_[0, np.flatnonzero(s[1:] != s[:-1]) + 1]
    ends = np.r_[starts[1:], len(s)]
    ranks = np.empty(len(s), dtype=np.float64)
    for a, b in zip(starts, ends):
        ranks[order[a:b]] = 0.5 * (a + b - 1) + 1.0
    return (ranks[y_true == 1].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)


def dcg_score(y_true, y_score, k=10):
    order = np.argsort(y_score)[::-1]
    y_true = np.take(y_true, order[:k])
    return np.sum((2 ** y_true - 1) / np.log2(np.arange(len(y_true)) + 2))


def ndcg_score(y_true, y_score, k=10):
    return dcg_score(y_true, y_score, k) / dcg_score(y_true, y_true, k)


def mrr_score(y_true, y_score):
    order = np.argsort(y_score)[::-1]
    y_true = np.take(y_true, order)
    return np.sum(y_true / (np.arange(len(y_true)) + 1)) / np.sum(y_true)


def ctr_score(y_true, y_score, k=1):
    order = np.argsort(y_score)[::-1]
    return np.mean(np.take(y_true, order[:k]))


def topk_reference(a, b=None, *, k, exclude=None):
    """Host statement of the full-corpus recommendation contract (include/nrhip.h, nr_score_topk); tests check the device
    against it, no product path calls it.

    `a` is the score matrix [U, V], or, with `b` given, the news vectors [V, N] and `b` the user vectors [U, N]: the scores
    are then <a[v], b[u]> in float64.  Per user the k best news in the total order (score descending, news id ascending):
    news 0 (the padding row) is never eligible, nor is an id listed in exclude[u] (entries that are 0 or outside [1, V) mean
    nothing, duplicates are allowed), nor a news whose score is NaN.  A row with fewer than k eligible news is filled with
    id 0, score -inf.  Returns (ids int32 [U, k], scores float64 [U, k])."""
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    U, V = scores.shape
    ids = np.zeros((U, k), dtype=np.int32)
    out = np.full((U, k), -np.inf, dtype=np.float64)
    for u in range(U):
        ok = ~np.isnan(scores[u])
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, -scores[u, cand]))][:k]      # primary key: score descending; ties: id ascending
        ids[u, :len(order)] = order
        out[u, :len(order)] = scores[u, order]
    return ids, out

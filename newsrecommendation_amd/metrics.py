"""Ranking metrics of the eval loop (src/metrics.py:1-29, src/main.py:255-258): per-impression AUC / MRR / nDCG@k, and the host
statements of the full-corpus contracts (top-k, rank, retrieval metrics).
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


def _pooled(scores, prior, stamp, window):
    """The pools of the full-corpus contracts (include/nrhip.h, K9): the final float64 scores `dot + prior` and the [U, V] mask of
    what prior and window leave eligible -- prior[v] != -inf (a NaN prior makes a NaN score: the NaN rule), and
    window[u, 0] <= stamp[v] <= window[u, 1], both ends inclusive (lo > hi: nobody).  None = off."""
    U, V = scores.shape
    ok = np.ones((U, V), dtype=bool)
    if prior is not None:
        prior = np.asarray(prior, dtype=np.float64).reshape(V)
        with np.errstate(invalid="ignore"):
            scores = scores + prior[None, :]
        ok &= ~np.isneginf(prior)[None, :]
    if (stamp is None) != (window is None):
        raise ValueError("stamp and window come together")
    if stamp is not None:
        stamp = np.asarray(stamp, dtype=np.int64).reshape(V)
        window = np.asarray(window, dtype=np.int64).reshape(U, 2)
        ok &= (window[:, :1] <= stamp[None, :]) & (stamp[None, :] <= window[:, 1:])
    return scores, ok


def topk_reference(a, b=None, *, k, exclude=None, prior=None, stamp=None, window=None, group=None, group_cap=None):
    """Host statement of the full-corpus recommendation contract (include/nrhip.h, nr_score_topk); tests check the device
    against it, no product path calls it.

    `a` is the score matrix [U, V], or, with `b` given, the news vectors [V, N] and `b` the user vectors [U, N]: the scores
    are then <a[v], b[u]> in float64.  Per user the k best news in the total order (score descending, news id ascending):
    news 0 (the padding row) is never eligible, nor is an id listed in exclude[u] (entries that are 0 or outside [1, V) mean
    nothing, duplicates are allowed), nor a news whose score is NaN.  exclude may be ragged: exclude[u] is any sequence of
    ids, of any length and in any order -- the dense list of the library and its CSR lists (ops.ExclusionLists) are both
    stated by it.  A row with fewer than k eligible news is filled with id 0, score -inf.
    Returns (ids int32 [U, k], scores float64 [U, k]).
    Pools: prior [V] is added to the scores (the returned scores are the sums) and -inf in it removes a news for everybody;
    stamp [V] with window [U, 2] keeps for user u the news with window[u, 0] <= stamp[v] <= window[u, 1] (_pooled).
    Group caps: group [V] integer ids (negative = in no group) with group_cap = c in [1, 128], together: the row is the walk
    down the eligible news in that order which takes a news unless c news of its group are already taken, and stops after k.
    What is not eligible uses up nothing of a cap."""
    if (group is None) != (group_cap is None):
        raise ValueError("group and group_cap come together")
    if group is not None and not 1 <= int(group_cap) <= 128:
        raise ValueError(f"group_cap = {group_cap}, must be in [1, 128]")
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    ids = np.zeros((U, k), dtype=np.int32)
    out = np.full((U, k), -np.inf, dtype=np.float64)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        cand = np.flatnonzero(ok)
        if group is None:
            order = cand[np.lexsort((cand, -scores[u, cand]))][:k]      # primary key: score descending; ties: id ascending
        else:
            grp, taken, order = np.asarray(group, dtype=np.int64).reshape(V), {}, []
            for v in cand[np.lexsort((cand, -scores[u, cand]))]:
                g = int(grp[v])
                if len(order) == k:
                    break
                if g >= 0 and taken.get(g, 0) >= int(group_cap):
                    continue
                taken[g] = taken.get(g, 0) + 1
                order.append(v)
            order = np.asarray(order, dtype=np.int64)
        ids[u, :len(order)] = order
        out[u, :len(order)] = scores[u, order]
    return ids, out


def rank_reference(a, b=None, *, targets, exclude=None, prior=None, stamp=None, window=None, group=None, group_cap=None):
    """Host statement of the full-corpus rank contract (include/nrhip.h, nr_score_rank); tests check the device against it, no
    product path calls it.

    `a`, `b`, `exclude` (ragged, any length) and the total order (score descending, news id ascending) are topk_reference's.  targets [U, T] int:
    entries that are 0 or outside [1, V) mean nothing.  The eligible news of user u are the ids 1 .. V-1 that are not in
    exclude[u] and whose score is not NaN; rank[u, j] is the 1-based position of targets[u, j] among them in that order, and 0
    ("not ranked") when the target means nothing, is excluded, has a NaN score or repeats an earlier entry of its row.
    Returns (ranks int32 [U, T], scores float64 [U, T]); the score is -inf where the rank is 0.
    Pools: prior, stamp, window as in topk_reference; a target outside its user's pool is not ranked, and an excluded id outside
    it changes nothing (it was not eligible to begin with).
    Group caps: group [V] integer ids (negative = in no group) with group_cap = c in [1, 128], together, as in topk_reference.
    The rank is then the place in the CAPPED ranking: the walk down the eligible news in the total order that takes a news
    unless c news of its group are already taken -- topk_reference's walk, not stopped at any k.  A target the walk skips is
    "capped out": rank -1, and it KEEPS its score (a legitimate held-out click the capped recommender never shows).  What is
    not eligible uses up nothing of a cap; what is not ranked without caps stays at rank 0, score -inf."""
    if (group is None) != (group_cap is None):
        raise ValueError("group and group_cap come together")
    if group is not None and not 1 <= int(group_cap) <= 128:
        raise ValueError(f"group_cap = {group_cap}, must be in [1, 128]")
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    targets = np.asarray(targets, dtype=np.int64)
    U, V = scores.shape
    T = targets.shape[1]
    ranks = np.zeros((U, T), dtype=np.int32)
    out = np.full((U, T), -np.inf, dtype=np.float64)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, -scores[u, cand]))]
        place = np.zeros(V, dtype=np.int64)
        if group is None:
            place[order] = np.arange(1, len(order) + 1)
        else:
            grp, taken, n_taken = np.asarray(group, dtype=np.int64).reshape(V), {}, 0
            for v in order:
                g = int(grp[v])
                if g >= 0 and taken.get(g, 0) >= int(group_cap):
                    place[v] = -1                                # eligible, and skipped by the walk
                    continue
                taken[g] = taken.get(g, 0) + 1
                n_taken += 1
                place[v] = n_taken
        seen = set()
        for j in range(T):
            t = int(targets[u, j])
            if 1 <= t < V and t not in seen and place[t] != 0:
                ranks[u, j], out[u, j] = place[t], scores[u, t]
            seen.add(t)
    return ranks, out


def mmr_reference(news, pool_ids, pool_scores, *, k, penalty, group=None, group_cap=None):
    """Host statement of the diversified re-ranking contract (include/nrhip.h, nr_mmr_select); tests check the device against
    it, no product path calls it.  Float64 arithmetic on the given inputs (fp32 arrays are taken as they are).

    news [V, N]; pool_ids [U, M] and pool_scores [U, M]: every user's pool; place i is live when its id is in [1, V) and its score
    is not NaN.  g(i, j) = <x_i, x_j>, rn_i = 1 / sqrt(g(i, i)) where g(i, i) > 0, else 0, s(i | j) = g(i, j) rn_i rn_j.  The walk
    takes k times the live place not yet taken with the largest value, ties to the LOWEST place: value_i = r_i for the first
    step, r_i - p_u max_{j taken} s(i | j) afterwards; penalty is a scalar or [U].  Group caps: group [V] integer ids (negative =
    in no group) with group_cap = c, together: a place whose group already has c places in the row is no candidate.  The walk
    ends when there is no candidate; the tail of the row is id 0, score -inf, place -1.
    Returns (ids int32 [U, k], scores float64 [U, k] -- the pool scores of the places taken --, places int32 [U, k], margins
    float64 [U, k]): margins[u, t] = value of the place taken at step t minus the best value among the other candidates of
    that step (0 for a tie, +inf without another candidate or after the walk ended) -- a row whose margins all exceed the
    error of a fp32 value cannot come out differently on the device."""
    if (group is None) != (group_cap is None):
        raise ValueError("group and group_cap come together")
    if group is not None and not 1 <= int(group_cap) <= 128:
        raise ValueError(f"group_cap = {group_cap}, must be in [1, 128]")
    news = np.asarray(news, dtype=np.float64)
    pid = np.asarray(pool_ids, dtype=np.int64)
    r = np.asarray(pool_scores, dtype=np.float64)
    V = news.shape[0]
    U, M = pid.shape
    if r.shape != (U, M) or not 1 <= k <= M:
        raise ValueError(f"pool_ids {pid.shape}, pool_scores {r.shape}, k = {k}: shapes must agree and k lie in [1, M]")
    p = np.broadcast_to(np.asarray(penalty, dtype=np.float64), (U,)) if np.ndim(penalty) else np.full(U, float(penalty))
    live = (pid >= 1) & (pid < V) & ~np.isnan(r)
    safe = np.where(live, pid, 0)
    grp = np.full((U, M), -1, dtype=np.int64) if group is None else np.where(live, np.asarray(group, dtype=np.int64).reshape(V)[safe], -1)
    cap = 0 if group is None else int(group_cap)
    ids = np.zeros((U, k), dtype=np.int32)
    out = np.full((U, k), -np.inf, dtype=np.float64)
    places = np.full((U, k), -1, dtype=np.int32)
    margins = np.full((U, k), np.inf, dtype=np.float64)
    for u0 in range(0, U, 16):                                   # the Gram matrices of 16 users at a time
        sl = slice(u0, min(u0 + 16, U))
        n = sl.stop - sl.start
        rows = np.arange(n)
        x = news[safe[sl]] * live[sl, :, None]
        gram = x @ x.transpose(0, 2, 1)
        diag = np.einsum("uii->ui", gram)
        with np.errstate(divide="ignore", invalid="ignore"):
            rn = np.where(diag > 0, 1.0 / np.sqrt(diag), 0.0)
        taken = np.zeros((n, M), dtype=bool)
        count = np.zeros((n, M), dtype=np.int64)
        maxsim = np.full((n, M), -np.inf)
        for t in range(k):
            cand = live[sl] & ~taken & ((grp[sl] < 0) | (count < cap))
            with np.errstate(invalid="ignore"):
                val = r[sl] if t == 0 else r[sl] - p[sl, None] * maxsim
            has = cand.any(axis=1)
            best = np.where(cand, val, -np.inf).max(axis=1)
            j = (cand & (val == best[:, None])).argmax(axis=1)   # the first place that reaches the maximum
            others = cand.copy()
            others[rows, j] = False
            second = np.where(others, val, -np.inf).max(axis=1)
            with np.errstate(invalid="ignore"):
                gap = np.where(others.any(axis=1), np.where(best == second, 0.0, best - second), np.inf)
            hu, hj = rows[has], j[has]
            ids[u0 + hu, t], out[u0 + hu, t], places[u0 + hu, t], margins[u0 + hu, t] = pid[u0 + hu, hj], r[u0 + hu, hj], hj, gap[has]
            taken[hu, hj] = True
            gj = grp[u0 + hu, hj]
            count[hu] += (grp[u0 + hu] == gj[:, None]) & (gj[:, None] >= 0)
            maxsim[hu] = np.maximum(maxsim[hu], gram[hu, hj, :] * rn[hu] * rn[hu, hj][:, None])
    return ids, out, places, margins


def philox4x32(counter, key, rounds=10):
    """Philox4x32 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", 2011) in numpy integers: counter [..., 4] and
    key [..., 2] of 32-bit words (they broadcast against each other); returns the four output words uint32 [..., 4].
    Multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85; the key is bumped between rounds."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def sample_noise_reference(seed, draw, user_keys, news_ids):
    """The noise of nr_score_sample (include/nrhip.h, K12) for pairs (user_keys[i], news_ids[i]) -- the two arrays broadcast:
    bits = Philox4x32-10(counter = (v >> 2, a, draw, 0), key = (seed & 0xffffffff, seed >> 32))[v & 3], integer-exact;
    u = ((bits >> 8) + 0.5) * 2^-24 and g = -log(-log(u)) in float64.  Returns (g float64, bits uint32)."""
    a = np.asarray(user_keys, dtype=np.int64) & 0xFFFFFFFF
    v = np.asarray(news_ids, dtype=np.int64) & 0xFFFFFFFF
    a, v = np.broadcast_arrays(a, v)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.stack([v >> 2, a, np.full(v.shape, int(draw) & 0xFFFFFFFF, dtype=np.int64), np.zeros(v.shape, dtype=np.int64)], axis=-1)
    words = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    bits = np.take_along_axis(words, (v & 3)[..., None], axis=-1)[..., 0]
    u = ((bits >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u)), bits


def sample_reference(a, b=None, *, k, temperature, seed, draw=0, user_keys=None, exclude=None, prior=None, stamp=None, window=None, group=None,
                     group_cap=None):
    """Host statement of the sampled recommendation contract (include/nrhip.h, nr_score_sample); tests check the device
    against it, no product path calls it.

    `a`, `b`, `exclude`, the pools and the caps are topk_reference's.  Row u is topk_reference's row for the scores
    score[u, v] + prior[v] + tau_u * g(user_keys[u], v) in float64, g the Gumbel noise of sample_noise_reference under (seed,
    draw): k news without replacement, each draw proportional to exp((score + prior) / tau_u) over what is left
    (Plackett-Luce), under caps renormalised over what may still be taken.  temperature: a scalar or [U], finite and >= 0 --
    a user whose entry is negative, NaN or infinite gets an all-fill row; 0 is topk_reference itself.  user_keys [U] (None =
    0 .. U-1) name the users in the noise.
    Returns (ids int32 [U, k], perturbed float64 [U, k] -- the values the row is ordered by --, model float64 [U, k] -- score +
    prior of the news taken; -inf in fill)."""
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    U, V = scores.shape
    tau = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (U,)) if np.ndim(temperature) else np.full(U, float(temperature))
    keys = np.arange(U, dtype=np.int64) if user_keys is None else np.asarray(user_keys, dtype=np.int64).reshape(U)
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(tau) & (tau >= 0))
    g, _ = sample_noise_reference(seed, draw, keys[:, None], np.arange(V, dtype=np.int64)[None, :])
    noise = np.where(bad, 0.0, tau)[:, None] * g
    ids, perturbed = topk_reference(scores + noise, k=k, exclude=exclude, prior=prior, stamp=stamp, window=window, group=group, group_cap=group_cap)
    ids[bad], perturbed[bad] = 0, -np.inf
    with np.errstate(invalid="ignore"):
        model = np.where(ids > 0, perturbed - np.take_along_axis(noise, ids.astype(np.int64), axis=1), -np.inf)
    return ids, perturbed, model


def _temperatures(temperature, U):
    """[U] float64 temperatures and the mask of the valid ones (finite and > 0)."""
    tau = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (U,)) if np.ndim(temperature) else np.full(U, float(temperature))
    with np.errstate(invalid="ignore"):
        return tau, np.isfinite(tau) & (tau > 0)


def logz_reference(a, b=None, *, temperature, exclude=None, prior=None, stamp=None, window=None):
    """Host statement of the full-corpus log-partition contract (include/nrhip.h, nr_score_logz); tests check the device against
    it, no product path calls it.

    `a`, `b`, `exclude` (ragged, any length) and the pools are topk_reference's, and so is what is eligible: ids 1 .. V-1 that
    are not in exclude[u], whose score (+ prior) is not NaN, whose prior is not -inf and whose stamp lies in the user's window.
    Per user, over its eligible news, in float64: smax = the largest score, count = how many, and
    logsum = log sum exp((score - smax) / tau_u), so that log Z = smax / tau + logsum.  temperature: a scalar or [U]; an entry
    that is not finite and > 0 gives logsum NaN and leaves smax and count.  Nothing eligible: (-inf, -inf, 0); a largest score
    of +-inf: logsum NaN.  Returns (logsum float64 [U], smax float64 [U], count int64 [U])."""
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    tau, tau_ok = _temperatures(temperature, U)
    logsum, smax, count = np.full(U, -np.inf), np.full(U, -np.inf), np.zeros(U, dtype=np.int64)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        x = scores[u, ok]
        count[u] = x.size
        if x.size == 0:
            continue
        smax[u] = x.max()
        if not tau_ok[u] or not np.isfinite(smax[u]):
            logsum[u] = np.nan
        else:
            logsum[u] = np.log(np.sum(np.exp((x - smax[u]) / tau[u])))
    return logsum, smax, count


def expect_reference(a, b, *, temperature, exclude=None, prior=None, stamp=None, window=None, weight=None):
    """Host statement of the expected-news-vector contract (include/nrhip.h, nr_score_expect); tests check the device against
    it, no product path calls it.

    `a` [V, N] news vectors, `b` [U, N] user vectors; `exclude` and the pools are logz_reference's, and so is what is eligible
    (through _pooled).  Per user, over its eligible news, in float64: p_v = exp((score_v - smax) / tau_u) / sum of these, and
    expect[u] = weight_u * sum_v p_v * a[v] (weight None = 1), mass[u] = sum_v p_v = 1.  Nothing eligible: zeros and mass 0.  A
    temperature that is not finite and > 0, or a largest score of +-inf: a row of NaN and mass NaN.  Components of `a` that are
    not finite count as 0 in the sum (their news has weight 0 whenever the row is not NaN).
    Returns (expect float64 [U, N], mass float64 [U])."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        scores = b @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    tau, tau_ok = _temperatures(temperature, U)
    w = np.ones(U) if weight is None else np.asarray(weight, dtype=np.float64).reshape(U)
    clean = np.where(np.isfinite(a), a, 0.0)
    expect, mass = np.zeros((U, a.shape[1])), np.zeros(U)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        x = scores[u, ok]
        if x.size == 0:
            continue
        if not tau_ok[u] or not np.isfinite(x.max()):
            expect[u], mass[u] = np.nan, np.nan
            continue
        p = np.exp((x - x.max()) / tau[u])
        p = p / p.sum()
        expect[u] = w[u] * (p @ clean[ok])
        mass[u] = p.sum()
    return expect, mass


def _log_softmax_rows(a, b, temperature, exclude, prior, stamp, window):
    """Per user the float64 (ok mask [V], p [n_ok], x = log p [n_ok]) of the full softmax over what logz_reference calls
    eligible, or None in place of (p, x) for a NaN user (bad temperature, a largest score of +-inf); the shared front of
    entropy_reference and expect_affine_reference."""
    with np.errstate(invalid="ignore", over="ignore"):
        scores = b @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    tau, tau_ok = _temperatures(temperature, U)
    rows = []
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        s = scores[u, ok]
        if s.size and (not tau_ok[u] or not np.isfinite(s.max())):
            rows.append((ok, None, None))
            continue
        with np.errstate(divide="ignore"):
            z = (s - s.max()) / tau[u] if s.size else s
            x = z - np.log(np.sum(np.exp(z))) if s.size else z
        rows.append((ok, np.exp(x), x))
    return rows


def entropy_reference(news, user, temperature, exclude=None, prior=None, stamp=None, window=None):
    """Host statement of the entropy contract (include/nrhip.h, nr_score_entropy); tests check the device against it, no product
    path calls it.

    `news` [V, N], `user` [U, N]; `exclude` and the pools are logz_reference's, and so is what is eligible (through _pooled).
    Per user, over its eligible news, in float64 with x_v = log p_v: H = -sum p x, var = sum p x^2 - (sum p x)^2 = Var_p(log p),
    mass = sum p = 1.  A term with p == 0 (a score of -inf under a finite maximum) is 0: 0 log 0 = 0.  Nothing eligible:
    (0, 0, 0).  A temperature that is not finite and > 0, or a largest score of +-inf: NaN for that user.
    Returns (H, var, mass), float64 [U] each."""
    a = np.asarray(news, dtype=np.float64)
    b = np.asarray(user, dtype=np.float64)
    U = b.shape[0]
    H, var, mass = np.zeros(U), np.zeros(U), np.zeros(U)
    for u, (ok, p, x) in enumerate(_log_softmax_rows(a, b, temperature, exclude, prior, stamp, window)):
        if p is None:
            H[u] = var[u] = mass[u] = np.nan
            continue
        xs = np.where(p > 0, x, 0.0)
        m1 = float(np.sum(p * xs))
        H[u], var[u], mass[u] = -m1, float(np.sum(p * xs * xs)) - m1 * m1, float(np.sum(p))
    return H, var, mass


def expect_affine_reference(news, user, temperature, exclude=None, prior=None, stamp=None, window=None, alpha=None, beta=None,
                            sub_ids=None, sub_w=None, scale_inv_tau=False):
    """Host statement of the affine expected-news-vector contract (include/nrhip.h, nr_score_expect_affine); tests check the
    device against it, no product path calls it.

    What is eligible, p and x = log p are entropy_reference's.  Per user, in float64,
    out[u] = sum_v p_v (alpha_u + beta_u x_v) news[v] - sum_t sub_w[u, t] news[sub_ids[u, t]], times 1 / tau_u when scale_inv_tau;
    alpha None = 1, beta None = 0; a term with p == 0 is 0; named ids outside [1, V) are fill; components of `news` that are not
    finite count as 0 in the sum over v -- a NAMED row is subtracted as it is, its non-finite components included.  mass[u] = sum p.  Nothing eligible: only the named rows, mass 0.  A temperature that is not finite and
    > 0, or a largest score of +-inf: a row of NaN and mass NaN.  Returns (out float64 [U, N], mass float64 [U])."""
    a = np.asarray(news, dtype=np.float64)
    b = np.asarray(user, dtype=np.float64)
    U, V = b.shape[0], a.shape[0]
    tau, _ = _temperatures(temperature, U)
    al = np.ones(U) if alpha is None else np.asarray(alpha, dtype=np.float64).reshape(U)
    be = np.zeros(U) if beta is None else np.asarray(beta, dtype=np.float64).reshape(U)
    clean = np.where(np.isfinite(a), a, 0.0)
    out, mass = np.zeros((U, a.shape[1])), np.zeros(U)
    for u, (ok, p, x) in enumerate(_log_softmax_rows(a, b, temperature, exclude, prior, stamp, window)):
        if p is None:
            out[u], mass[u] = np.nan, np.nan
            continue
        live = p > 0
        r = np.where(live, p, 0.0) * (al[u] + be[u] * np.where(live, x, 0.0))
        out[u], mass[u] = r @ clean[ok], float(np.sum(p))
        if sub_ids is not None:
            ids = np.asarray(sub_ids[u], dtype=np.int64).reshape(-1)
            w = np.asarray(sub_w[u], dtype=np.float64).reshape(-1)
            real = (ids >= 1) & (ids < V)
            with np.errstate(invalid="ignore"):
                for t in np.flatnonzero(real):                              # the named rows as they are, as the device subtracts them
                    out[u] -= w[t] * a[ids[t]]
        if scale_inv_tau:
            out[u] /= tau[u]
    return out, mass


def _kl_rows(news, user, ref, temperature, ref_temperature, exclude, prior, stamp, window):
    """Per user the float64 (ok mask [V], p, x = log p, y = log q) over the news eligible for the POLICY, the shared front of
    kl_reference and expect_kl_reference.  p is None for a NaN user: something is eligible for the policy and either side has a
    temperature that is not finite and > 0 or a largest score of +-inf, or the reference has nothing eligible.  y is NaN where the
    news is not eligible for the reference (its score there is NaN)."""
    a = np.asarray(news, dtype=np.float64)
    rows_p = _log_softmax_rows(a, np.asarray(user, dtype=np.float64), temperature, exclude, prior, stamp, window)
    rows_q = _log_softmax_rows(a, np.asarray(ref, dtype=np.float64), ref_temperature, exclude, prior, stamp, window)
    rows = []
    for (ok, p, x), (okq, q, y) in zip(rows_p, rows_q):
        if not ok.any():
            rows.append((ok, np.zeros(0), np.zeros(0), np.zeros(0)))
        elif p is None or q is None or not okq.any():
            rows.append((ok, None, None, None))
        else:
            full = np.full(ok.shape[0], np.nan)
            full[okq] = y
            rows.append((ok, p, x, full[ok]))
    return rows


def kl_reference(news, user, ref, tau, ref_tau, exclude=None, prior=None, stamp=None, window=None):
    """Host statement of the KL contract (include/nrhip.h, nr_score_kl); tests check the device against it, no product path
    calls it.

    `news` [V, N], `user` and `ref` [U, N]: the policy p = softmax(scores(user) / tau) and the reference
    q = softmax(scores(ref) / ref_tau) over what logz_reference calls eligible under the shared `exclude` and pools.  Per user,
    in float64 with x = log p, y = log q, d = x - y over the policy's eligible news: kl = sum p d = KL(p || q), entropy = -sum p x,
    cov = sum p d x - (sum p d)(sum p x) = Cov_p(d, x) (d kl / d tau = -cov / tau), mass = sum p = 1.  A term with p == 0 is 0.
    Nothing eligible for the policy: zeros.  A temperature on either side that is not finite and > 0, a largest score of +-inf on
    either side, or a reference with nothing eligible: NaN for that user.
    Returns (kl, entropy, cov, mass), float64 [U] each."""
    U = np.asarray(user).shape[0]
    kl, H, cov, mass = np.zeros(U), np.zeros(U), np.zeros(U), np.zeros(U)
    for u, (ok, p, x, y) in enumerate(_kl_rows(news, user, ref, tau, ref_tau, exclude, prior, stamp, window)):
        if p is None:
            kl[u] = H[u] = cov[u] = mass[u] = np.nan
            continue
        live = p > 0
        pl, xs, ds = p[live], x[live], x[live] - y[live]
        with np.errstate(invalid="ignore"):
            k1, m1 = float(np.sum(pl * ds)), float(np.sum(pl * xs))
            kl[u], H[u], cov[u], mass[u] = k1, -m1, float(np.sum(pl * ds * xs)) - k1 * m1, float(np.sum(p))
    return kl, H, cov, mass


def expect_kl_reference(news, user, ref, tau, ref_tau, exclude=None, prior=None, stamp=None, window=None, alpha=None, beta=None,
                        gamma=None, sub_ids=None, sub_w=None, scale_inv_tau=False):
    """Host statement of the KL expected-news-vector contract (include/nrhip.h, nr_score_expect_kl); tests check the device against
    it, no product path calls it.

    What is eligible, p, x = log p and y = log q are kl_reference's.  Per user, in float64,
    out[u] = sum_v p_v (alpha_u + beta_u x_v + gamma_u y_v) news[v] - sum_t sub_w[u, t] news[sub_ids[u, t]], times 1 / tau_u when
    scale_inv_tau; alpha None = 1, beta None = 0, gamma None = 0; a term with p == 0 is 0; the named rows and the non-finite
    components of `news` are expect_affine_reference's.  mass[u] = sum p.  Nothing eligible for the policy: only the named rows,
    mass 0.  A NaN user of kl_reference: a row of NaN and mass NaN.  Returns (out float64 [U, N], mass float64 [U])."""
    a = np.asarray(news, dtype=np.float64)
    U, V = np.asarray(user).shape[0], a.shape[0]
    t, _ = _temperatures(tau, U)
    al = np.ones(U) if alpha is None else np.asarray(alpha, dtype=np.float64).reshape(U)
    be = np.zeros(U) if beta is None else np.asarray(beta, dtype=np.float64).reshape(U)
    ga = np.zeros(U) if gamma is None else np.asarray(gamma, dtype=np.float64).reshape(U)
    clean = np.where(np.isfinite(a), a, 0.0)
    out, mass = np.zeros((U, a.shape[1])), np.zeros(U)
    for u, (ok, p, x, y) in enumerate(_kl_rows(news, user, ref, tau, ref_tau, exclude, prior, stamp, window)):
        if p is None:
            out[u], mass[u] = np.nan, np.nan
            continue
        live = p > 0
        with np.errstate(invalid="ignore"):
            r = np.where(live, p, 0.0) * (al[u] + be[u] * np.where(live, x, 0.0) + ga[u] * np.where(live, y, 0.0))
            out[u], mass[u] = r @ clean[ok], float(np.sum(p))
        if sub_ids is not None:
            ids = np.asarray(sub_ids[u], dtype=np.int64).reshape(-1)
            w = np.asarray(sub_w[u], dtype=np.float64).reshape(-1)
            real = (ids >= 1) & (ids < V)
            with np.errstate(invalid="ignore"):
                for j in np.flatnonzero(real):                              # the named rows as they are, as the device subtracts them
                    out[u] -= w[j] * a[ids[j]]
        if scale_inv_tau:
            out[u] /= t[u]
    return out, mass


def softmax_matrix_reference(a, b, *, temperature, exclude=None, prior=None, stamp=None, window=None):
    """The [U, V] float64 matrix p(v | u) of the full softmax over what logz_reference calls eligible (through _pooled), which
    the device never forms: row u sums to 1 over its eligible news and is 0 elsewhere.  A dead user -- a temperature that is not
    finite and > 0, a largest eligible score of +-inf, nothing eligible -- has a row of zeros.  Returns (p [U, V], live bool [U])."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        scores = b @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    tau, tau_ok = _temperatures(temperature, U)
    p, live = np.zeros((U, V)), np.zeros(U, dtype=bool)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        x = scores[u, ok]
        if x.size == 0 or not tau_ok[u] or not np.isfinite(x.max()):
            continue
        w = np.exp((x - x.max()) / tau[u])
        p[u, ok] = w / w.sum()
        live[u] = True
    return p, live


def expect_news_reference(a, b, *, temperature, exclude=None, prior=None, stamp=None, window=None, weight=None, named=None, scale_inv_tau=False):
    """Host statement of the news side of the full-softmax gradient (include/nrhip.h, nr_score_expect_news); tests check the
    device against it, no product path calls it.  float64 throughout.

    `a` [V, N] news vectors, `b` [U, N] user vectors; `exclude` (per USER, ragged), the pools and what is eligible are
    expect_reference's.  With p(v | u) the softmax of softmax_matrix_reference and c_u = weight_u (/ tau_u if scale_inv_tau;
    weight None = 1):
      out[v]  = sum_u c_u p(v | u) b[u]  -  sum_j named_w[j] (/ tau_user if scale_inv_tau) b[named_user[j]]
      mass[v] = sum_u weight_u p(v | u)                                   (never scaled by 1 / tau)
    named = (offsets [V + 1], users [n], w [n]): the named terms of news v are entries offsets[v] .. offsets[v + 1] - 1; an entry
    with w == 0 is skipped.  A dead user (softmax_matrix_reference) contributes nothing, in the sum and in the named terms.
    Components of `b` that are not finite count as 0.  Row 0 and rows nobody can be shown are zeros minus their named terms.
    Returns (out float64 [V, N], mass float64 [V])."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p, live = softmax_matrix_reference(a, b, temperature=temperature, exclude=exclude, prior=prior, stamp=stamp, window=window)
    U, V = p.shape
    tau, _ = _temperatures(temperature, U)
    w = np.ones(U) if weight is None else np.asarray(weight, dtype=np.float64).reshape(U)
    w = np.where(live, w, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        it = np.where(live, 1.0 / tau, 0.0) if scale_inv_tau else np.where(live, 1.0, 0.0)
    clean = np.where(np.isfinite(b), b, 0.0)
    out = p.T @ ((w * it)[:, None] * clean)
    mass = p.T @ w
    if named is not None:
        off, nu, nw = (np.asarray(x) for x in named)
        for v in range(V):
            for j in range(int(off[v]), int(off[v + 1])):
                u = int(nu[j])
                if nw[j] != 0 and 0 <= u < U and live[u]:
                    out[v] -= float(nw[j]) * it[u] * clean[u]
    return out, mass


def expect_news_affine_reference(a, b, *, temperature, exclude=None, prior=None, stamp=None, window=None, alpha=None, beta=None, named=None,
                                 scale_inv_tau=False):
    """Host statement of the news side of the entropy-regularised full-softmax gradient (include/nrhip.h,
    nr_score_expect_news_affine); tests check the device against it, no product path calls it.  float64 throughout.

    expect_news_reference with the per-pair weight affine in x = log p(v | u): with a_u = alpha_u, b_u = beta_u (each / tau_u if
    scale_inv_tau; alpha None = 1, beta None = 0),
      out[v]  = sum_u p(v | u) (a_u + b_u x_uv) b[u]  -  sum_j named_w[j] (/ tau_user if scale_inv_tau) b[named_user[j]]
      mass[v] = sum_u p(v | u)                                            (over the live users; not the sum of the weights)
    A pair with p == 0 is a term of no sum (0 log 0 = 0).  A user whose alpha or beta is not finite contributes nothing through
    the sum; its named terms stay (they are gated by the user being live and w != 0 only), and so does its share of the mass.
    The dead users, the named terms, the cleaning of `b` and rows nobody can be shown are expect_news_reference's.
    Returns (out float64 [V, N], mass float64 [V])."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p, live = softmax_matrix_reference(a, b, temperature=temperature, exclude=exclude, prior=prior, stamp=stamp, window=window)
    U, V = p.shape
    tau, _ = _temperatures(temperature, U)
    al = np.ones(U) if alpha is None else np.asarray(alpha, dtype=np.float64).reshape(U)
    be = np.zeros(U) if beta is None else np.asarray(beta, dtype=np.float64).reshape(U)
    with np.errstate(divide="ignore", invalid="ignore"):
        it = np.where(live, 1.0 / tau, 0.0) if scale_inv_tau else np.where(live, 1.0, 0.0)
        fin = live & np.isfinite(al * it) & np.isfinite(be * it)
        ca, cb = np.where(fin, al * it, 0.0), np.where(fin, be * it, 0.0)
        x = np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), 0.0)
    clean = np.where(np.isfinite(b), b, 0.0)
    out = (p * (ca[:, None] + cb[:, None] * x)).T @ clean
    mass = p.T @ np.where(live, 1.0, 0.0)
    if named is not None:
        off, nu, nw = (np.asarray(t) for t in named)
        for v in range(V):
            for j in range(int(off[v]), int(off[v + 1])):
                u = int(nu[j])
                if nw[j] != 0 and 0 <= u < U and live[u]:
                    out[v] -= float(nw[j]) * it[u] * clean[u]
    return out, mass


def row_logprob_reference(a, b=None, *, row_ids, temperature, base, sequential, prior=None, stamp=None, window=None):
    """Host statement of the row log-probability contract (include/nrhip.h, nr_row_logprob); tests check the device against it,
    no product path calls it.

    `a`, `b` and the pools are topk_reference's.  row_ids [U, k] integers; base = (logsum [U], smax [U]), the first two results
    of logz_reference (or of the device) for these users.  With s_i the score (+ prior) of entry i, in float64:
      sequential: out[u, j] = (s_j - M_j) / tau - L_j,  M_j = max(smax, max_{i >= j} s_i),
                  L_j = log(exp((smax - M_j) / tau + logsum) + sum_{i >= j} exp((s_i - M_j) / tau)) -- Plackett-Luce without
                  replacement; the base must have been formed WITHOUT the row's ids (pass them in `exclude` of logz_reference)
      otherwise:  out[u, j] = (s_j - smax) / tau - logsum, the base formed over everything eligible, the entries included.
    An entry that is 0 or outside [1, V) is fill: 0, part of no sum.  An entry outside the pool or with a NaN score gives NaN and
    is part of no sum.  A temperature that is not finite and > 0 gives NaN for the real entries of that user.  Membership in an
    exclusion list and repeats are the caller's statement and are not checked.
    Returns (logp float64 [U, k], total float64 [U] = the row sums)."""
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    ids = np.asarray(row_ids, dtype=np.int64).reshape(U, -1)
    k = ids.shape[1]
    tau, tau_ok = _temperatures(temperature, U)
    bl, bm = np.asarray(base[0], dtype=np.float64).reshape(U), np.asarray(base[1], dtype=np.float64).reshape(U)
    out = np.zeros((U, k), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for u in range(U):
            real = (ids[u] >= 1) & (ids[u] < V)
            at = np.where(real, ids[u], 0)
            s = scores[u, at]
            live = real & pool[u, at] & ~np.isnan(s)
            for j in range(k):
                if not real[j]:
                    continue
                if not live[j] or not tau_ok[u]:
                    out[u, j] = np.nan
                elif sequential:
                    rest = s[j:][live[j:]]
                    M = max(bm[u], rest.max())
                    mass = np.sum(np.exp((rest - M) / tau[u]))
                    if bm[u] > -np.inf or np.isnan(bl[u]):
                        mass = mass + np.exp((bm[u] - M) / tau[u] + bl[u])
                    out[u, j] = (s[j] - M) / tau[u] - np.log(mass)
                else:
                    out[u, j] = (s[j] - bm[u]) / tau[u] - bl[u]
    return out, out.sum(axis=1)


def row_logprob_grad_reference(a, b=None, *, row_ids, temperature, base, g=None, prior=None, stamp=None, window=None):
    """Host statement of the gradient coefficients of a sequential row (include/nrhip.h, nr_row_logprob_grad); tests check the
    device against it, no product path calls it.

    The arguments are row_logprob_reference's (sequential rows: the base formed WITHOUT the row's ids); g [U, k] is the upstream
    gradient of nll_j = -logp_j per entry (None = 1).  With s_i the score (+ prior) of entry i, e_i = exp(s_i / tau), B the
    base's mass and W_j = B + sum_{i >= j} e_i over the live entries, in float64 around the running maxima:
      weight[u]   = a   = sum_j g_j B / W_j
      sub_w[u, i] = c_i = g_i - e_i sum_{j <= i} g_j / W_j
    so that d (sum_j g_j nll_j) / d user = (a E_rest - sum_i c_i news[i_i]) / tau, E_rest the softmax mean over the news of B.
    Fill entries (0 or outside [1, V)) and entries outside the pool or with a NaN score are no step: c = 0 and their g is not
    looked at.  A temperature that is not finite and > 0, or a NaN base, gives that user zeros; an empty base (smax -inf) gives
    a = 0.  Returns (weight float64 [U], sub_w float64 [U, k])."""
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    ids = np.asarray(row_ids, dtype=np.int64).reshape(U, -1)
    k = ids.shape[1]
    tau, tau_ok = _temperatures(temperature, U)
    bl, bm = np.asarray(base[0], dtype=np.float64).reshape(U), np.asarray(base[1], dtype=np.float64).reshape(U)
    gs = np.ones((U, k)) if g is None else np.asarray(g, dtype=np.float64).reshape(U, k)
    weight, sub_w = np.zeros(U), np.zeros((U, k))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for u in range(U):
            real = (ids[u] >= 1) & (ids[u] < V)
            at = np.where(real, ids[u], 0)
            s = scores[u, at]
            live = real & pool[u, at] & ~np.isnan(s)
            if not tau_ok[u] or np.isnan(bm[u]) or np.isnan(bl[u]) or not live.any():
                continue
            steps = np.flatnonzero(live)
            x, gl = s[steps], gs[u, steps]
            # in logs, around the row's largest score M: lw_j = log W_j - M / tau as a suffix log-add-exp, so that a tail far
            # below the head keeps its digits and every ratio e_i / W_j, B / W_j is exp of a difference <= 0
            M = max(bm[u], x.max())
            lx = (x - M) / tau[u]
            lb = (bm[u] - M) / tau[u] + bl[u] if bm[u] > -np.inf else -np.inf
            lw = np.empty(len(steps))
            run = lb
            for n_i in range(len(steps) - 1, -1, -1):
                run = np.logaddexp(lx[n_i], run)
                lw[n_i] = run
            for n_i, i in enumerate(steps):
                sub_w[u, i] = gl[n_i] - np.sum(gl[:n_i + 1] * np.exp(lx[n_i] - lw[:n_i + 1]))
            weight[u] = np.sum(gl * np.exp(lb - lw)) if lb > -np.inf else 0.0
    return weight, sub_w


def _bins(group, n_groups, V):
    """[V] int64 bins of the news under `group`: the group id, or n_groups for a negative one ("no group"); and n_groups
    (None = max id + 1, at least 1).  An id >= n_groups is an error."""
    grp = np.asarray(group, dtype=np.int64).reshape(V)
    G = max(int(grp.max()) + 1, 1) if n_groups is None else int(n_groups)
    if not 1 <= G <= 512:
        raise ValueError(f"n_groups = {G}, must be in [1, 512]")
    if grp.max() >= G:
        raise ValueError(f"group id {int(grp.max())} >= n_groups = {G}")
    return np.where(grp < 0, G, grp), G


def logz_groups_reference(a, b=None, *, temperature, group, n_groups=None, exclude=None, prior=None, stamp=None, window=None):
    """Host statement of the per-group log-partition contract (include/nrhip.h, nr_score_logz_groups); tests check the device
    against it, no product path calls it.

    `a`, `b`, `exclude`, the pools and what is eligible are logz_reference's.  group [V] integer ids in [0, n_groups) (negative =
    in no group), n_groups <= 512 (None = max id + 1).  Bins b = 0 .. n_groups - 1 are the groups, bin n_groups is "no group".
    Per (user, bin), over the eligible news of the bin, in float64, with logz_reference's meaning: gmax = the largest score,
    count = how many, logsum = log sum exp((score - gmax) / tau_u) >= 0.  An empty bin gives (-inf, -inf, 0), whatever the
    temperature; an entry of temperature that is not finite and > 0 gives that user logsum NaN in every non-empty bin and leaves
    gmax and count; a largest score of +-inf gives logsum NaN.
    Returns (logsum float64 [U, n_groups + 1], gmax float64 [U, n_groups + 1], count int64 [U, n_groups + 1])."""
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    bins, G = _bins(group, n_groups, V)
    tau, tau_ok = _temperatures(temperature, U)
    logsum, gmax, count = np.full((U, G + 1), -np.inf), np.full((U, G + 1), -np.inf), np.zeros((U, G + 1), dtype=np.int64)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        if exclude is not None:
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[ex[(ex >= 1) & (ex < V)]] = False
        for bb in np.unique(bins[ok]):
            x = scores[u, ok & (bins == bb)]
            count[u, bb] = x.size
            gmax[u, bb] = x.max()
            if not tau_ok[u] or not np.isfinite(gmax[u, bb]):
                logsum[u, bb] = np.nan
            else:
                logsum[u, bb] = np.log(np.sum(np.exp((x - gmax[u, bb]) / tau[u])))
    return logsum, gmax, count


def capped_row_logprob_reference(a, b=None, *, row_ids, temperature, bases, group, group_cap, n_groups=None, prior=None, stamp=None,
                                 window=None):
    """Host statement of the capped row log-probability contract (include/nrhip.h, nr_row_logprob_capped); tests check the
    device against it, no product path calls it.

    The law of sample_reference's rows under caps: at step j the candidates are the eligible news not yet taken whose group has
    fewer than c = group_cap entries in the row so far; news of no group (negative id) are never capped.  `a`, `b` and the pools
    are topk_reference's; row_ids [U, k]; bases = (logsum, gmax), each [U, n_groups + 1]: the first two results of
    logz_groups_reference (or of the device) computed with the row's ids in `exclude`.  With s_i the score (+ prior) of entry i,
    w = exp(s / tau), B_b = exp(gmax_b / tau + logsum_b) the mass of bin b in the bases, and t_b the step at which the row takes
    its c-th live entry of bin b (infinite for bin n_groups and for bins the row never fills), in float64:
      D_j = sum_{b : t_b >= j} (B_b + sum_{i >= j, bin(i) = b} w_i),   out[u, j] = s_j / tau - log D_j
    a sum of positive terms over the bins still open (formed around the largest score among them), never a difference.
    Entries: 0 or outside [1, V) is fill: 0, part of no sum.  Outside the pool or a NaN score: NaN, part of no sum, uses up
    nothing of a cap.  A temperature that is not finite and > 0: NaN for the real entries of that user.  A live entry whose
    group already has c live entries before it: -inf (the capped sampler never draws it); it uses up nothing of a cap, and its
    weight still counts in D_j of every earlier step at which its group was open -- the caller left it out of the bases.  The
    total of such a row is -inf.  Membership in an exclusion list and repeats are the caller's statement and are not checked.
    Returns (logp float64 [U, k], total float64 [U] = the row sums)."""
    if not 1 <= int(group_cap) <= 128:
        raise ValueError(f"group_cap = {group_cap}, must be in [1, 128]")
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    bins, G = _bins(group, n_groups, V)
    ids = np.asarray(row_ids, dtype=np.int64).reshape(U, -1)
    k, c = ids.shape[1], int(group_cap)
    tau, tau_ok = _temperatures(temperature, U)
    bl, bm = np.asarray(bases[0], dtype=np.float64).reshape(U, G + 1), np.asarray(bases[1], dtype=np.float64).reshape(U, G + 1)
    out = np.zeros((U, k), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for u in range(U):
            real = (ids[u] >= 1) & (ids[u] < V)
            at = np.where(real, ids[u], 0)
            s = scores[u, at]
            live = real & pool[u, at] & ~np.isnan(s)
            bn = bins[at]
            t_close = np.full(G + 1, k, dtype=np.int64)                # k stands for "never"
            seen, capped = np.zeros(G + 1, dtype=np.int64), np.zeros(k, dtype=bool)
            for j in np.flatnonzero(live):
                if bn[j] < G:
                    capped[j] = seen[bn[j]] >= c
                    seen[bn[j]] += 1
                    if seen[bn[j]] == c:
                        t_close[bn[j]] = j
            for j in range(k):
                if not real[j]:
                    continue
                if not live[j] or not tau_ok[u]:
                    out[u, j] = np.nan
                elif capped[j]:
                    out[u, j] = -np.inf
                else:
                    open_bins = t_close >= j
                    rest = s[j:][live[j:] & open_bins[bn[j:]]]
                    has = open_bins & ((bm[u] > -np.inf) | np.isnan(bl[u]))
                    M = max(rest.max(), bm[u][has].max()) if has.any() else rest.max()
                    mass = np.sum(np.exp((rest - M) / tau[u])) + np.sum(np.exp((bm[u][has] - M) / tau[u] + bl[u][has]))
                    out[u, j] = (s[j] - M) / tau[u] - np.log(mass)
    return out, out.sum(axis=1)


def expect_groups_reference(a, b, *, temperature, group, n_groups=None, bases=None, bin_w, exclude=None, prior=None, stamp=None, window=None):
    """Host statement of the per-bin expected-news-vector contract (include/nrhip.h, nr_score_expect_groups); tests check the
    device against it, no product path calls it.  float64 throughout.

    `a` [V, N], `b` [U, N], `exclude`, the pools and what is eligible are logz_groups_reference's, and so are the bins of
    `group` / `n_groups`.  bin_w [U, n_groups + 1] is omega.  Per (user, bin) over the bin's eligible news
      p_b(v) = exp((score_v - gmax_b) / tau_u - logsum_b)
    with (logsum, gmax) = bases when given (what logz_groups_reference or the device returned for the same arguments) and the
    bin's own exact softmax when bases is None, and
      expect[u] = sum_b omega_b sum_v p_b(v) a[v],   mass[u] = sum_b omega_b sum_v p_b(v)
    A bin with omega == 0 contributes exactly nothing whatever its base holds; so does an empty bin, and a bin whose largest
    eligible score is -inf counts as empty (gmax = -inf is how the device knows an empty bin).  A user with a non-empty
    bin and a temperature that is not finite and > 0, or with a non-empty bin whose omega != 0 and whose omega is not finite,
    whose gmax is NaN or +inf or whose logsum is NaN: a row of NaN and mass NaN.  Components of `a` that are not finite count as 0.
    Returns (expect float64 [U, N], mass float64 [U])."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        scores = b @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    bins, G = _bins(group, n_groups, V)
    tau, tau_ok = _temperatures(temperature, U)
    om = np.asarray(bin_w, dtype=np.float64).reshape(U, G + 1)
    clean = np.where(np.isfinite(a), a, 0.0)
    expect, mass = np.zeros((U, a.shape[1])), np.zeros(U)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for u in range(U):
            ok = ~np.isnan(scores[u]) & pool[u]
            ok[0] = False
            if exclude is not None:
                ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
                ok[ex[(ex >= 1) & (ex < V)]] = False
            bad = False
            for bb in range(G + 1):
                sel = ok & (bins == bb)
                x = scores[u, sel]
                if bases is None:
                    if x.size == 0:
                        continue
                    gm = x.max()
                    if gm == -np.inf:                                          # the device reads a maximum of -inf as an empty bin, whatever the count
                        continue
                    ls = np.log(np.sum(np.exp((x - gm) / tau[u]))) if tau_ok[u] and np.isfinite(gm) else np.nan
                else:
                    ls, gm = float(np.asarray(bases[0], dtype=np.float64)[u, bb]), float(np.asarray(bases[1], dtype=np.float64)[u, bb])
                    if gm == -np.inf:
                        continue
                if not tau_ok[u]:
                    bad = True
                    continue
                if om[u, bb] == 0:
                    continue
                if not np.isfinite(om[u, bb]) or np.isnan(gm) or gm == np.inf or np.isnan(ls):
                    bad = True
                    continue
                pw = np.exp((x - gm) / tau[u] - ls)
                expect[u] += om[u, bb] * (pw @ clean[sel])
                mass[u] += om[u, bb] * pw.sum()
            if bad:
                expect[u], mass[u] = np.nan, np.nan
    return expect, mass


def _capped_grad_rows(a, b, row_ids, temperature, bases, group, group_cap, n_groups, g, prior, stamp, window, mutant=None):
    """capped_row_logprob_grad_reference's body.  `mutant` names a deliberately wrong formula (tests/test_capgrad_host.py shows
    that each is caught by finite differences): "q_after_close" (Q at t_b + 1), "blocked_zero" (a blocked entry given c = 0),
    "closed_full_q" (a closed bin given the full Q); tests/test_capped_sweep_host.py adds "blocked_after_close" (a blocked entry's
    weight kept in D_j after its bin closed), "exclusive_scan" (Q_i without the step i itself) and "blocked_g_read" (a blocked
    entry treated as a step of its own g)."""
    if not 1 <= int(group_cap) <= 128:
        raise ValueError(f"group_cap = {group_cap}, must be in [1, 128]")
    a = np.asarray(a, dtype=np.float64)
    scores = a if b is None else np.asarray(b, dtype=np.float64) @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    bins, G = _bins(group, n_groups, V)
    ids = np.asarray(row_ids, dtype=np.int64).reshape(U, -1)
    k, c = ids.shape[1], int(group_cap)
    tau, tau_ok = _temperatures(temperature, U)
    bl, bm = np.asarray(bases[0], dtype=np.float64).reshape(U, G + 1), np.asarray(bases[1], dtype=np.float64).reshape(U, G + 1)
    gs = np.ones((U, k)) if g is None else np.asarray(g, dtype=np.float64).reshape(U, k)
    bin_w, sub_w = np.zeros((U, G + 1)), np.zeros((U, k))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for u in range(U):
            real = (ids[u] >= 1) & (ids[u] < V)
            at = np.where(real, ids[u], 0)
            s = scores[u, at]
            live = real & pool[u, at] & ~np.isnan(s)
            if not tau_ok[u] or np.isnan(bm[u]).any() or (np.isnan(bl[u]) & (bm[u] > -np.inf)).any():
                continue
            bn = bins[at]
            t_close = np.full(G + 1, k, dtype=np.int64)                # k stands for "never"
            seen, capped = np.zeros(G + 1, dtype=np.int64), np.zeros(k, dtype=bool)
            for j in np.flatnonzero(live):
                if bn[j] < G:
                    capped[j] = seen[bn[j]] >= c
                    seen[bn[j]] += 1
                    if seen[bn[j]] == c:
                        t_close[bn[j]] = j
            steps = np.flatnonzero(live & ~capped)
            if steps.size == 0:
                continue
            lB = np.where(bm[u] > -np.inf, bm[u] / tau[u] + bl[u], -np.inf)      # log B_b
            lx = s / tau[u]                                                   # log w_i
            lD = np.full(k, np.inf)
            for j in steps:
                open_bins = t_close >= j
                later = open_bins[bn[j:]] | capped[j:] if mutant == "blocked_after_close" else open_bins[bn[j:]]
                terms = np.concatenate([lx[j:][live[j:] & later], lB[open_bins]])
                lD[j] = np.logaddexp.reduce(terms)
            gl = np.where(live & ~capped, gs[u], 0.0)
            last = steps[-1]

            def q_times(log_num, upto):
                """sum_{j <= upto, j a live step} g_j exp(log_num - log D_j): every exponent <= 0 where log_num is a term of D_upto"""
                js = steps[steps < upto] if mutant == "exclusive_scan" else steps[steps <= upto]
                return float(np.sum(gl[js] * np.exp(log_num - lD[js]))) if js.size else 0.0

            for i in range(k):
                if not live[i]:
                    continue
                if capped[i]:
                    sub_w[u, i] = 0.0 if mutant == "blocked_zero" else (gs[u, i] if mutant == "blocked_g_read" else 0.0) - q_times(lx[i], t_close[bn[i]])
                else:
                    sub_w[u, i] = gs[u, i] - q_times(lx[i], i)
            for bb in range(G + 1):
                if lB[bb] == -np.inf:
                    continue
                upto = min(t_close[bb], last)
                if mutant == "q_after_close" and t_close[bb] < k:
                    upto = t_close[bb] + 1
                if mutant == "closed_full_q":
                    upto = last
                bin_w[u, bb] = q_times(lB[bb], upto)
    return bin_w, sub_w


def capped_row_logprob_grad_reference(a, b=None, *, row_ids, temperature, bases, group, group_cap, n_groups=None, g=None, prior=None,
                                      stamp=None, window=None):
    """Host statement of the gradient coefficients of a capped row (include/nrhip.h, nr_row_logprob_capped_grad); tests check
    the device against it, no product path calls it.  float64, in logs.

    The arguments are capped_row_logprob_reference's; g [U, k] is the upstream gradient of nll_j = -logp_j per entry (None = 1).
    In that function's notation, with Q_j = sum_{j' <= j, j' a live step} g_j' / D_j' and Q_b = Q at min(t_b, last live step):
      bin_w[u, b] = omega_b = B_b Q_b
      sub_w[u, i] = c_i = g_i - w_i Q_i at a live step;  -w_i Q_{bin(i)} at a blocked entry (group already full; no step, its g
                    is not looked at);  0 at fill and at entries outside the pool or with a NaN score
    so that d (sum_j g_j nll_j) / d user = (sum_b omega_b E_b - sum_i c_i news[row_i]) / tau, E_b the softmax mean inside bin b
    over the news of B_b (expect_groups_reference).  sum_b omega_b = sum_i c_i.  A temperature that is not finite and > 0, a NaN
    gmax, a NaN logsum of a non-empty bin, or a row without a live step: zeros.  An empty bin has omega = 0.
    Returns (bin_w float64 [U, n_groups + 1], sub_w float64 [U, k])."""
    return _capped_grad_rows(a, b, row_ids, temperature, bases, group, group_cap, n_groups, g, prior, stamp, window)


def expect_news_groups_reference(a, b, *, temperature, group, n_groups=None, bases=None, bin_w, exclude=None, prior=None, stamp=None, window=None,
                                 named=None, scale_inv_tau=False, dead=None):
    """Host statement of the news side of the capped row's gradient (include/nrhip.h, nr_score_expect_news_groups); tests check
    the device against it, no product path calls it.  float64 throughout.

    `a` [V, N], `b` [U, N], `exclude` (per USER, ragged), the pools and what is eligible are logz_groups_reference's, and so are
    the bins of `group` / `n_groups`.  bin_w [U, n_groups + 1] is omega, as everywhere (user-major).  Per (user, bin) over the
    bin's eligible news p_b(v | u) = exp((score_uv - gmax_ub) / tau_u - logsum_ub), with (logsum, gmax) = bases when given and
    the bin's own exact softmax when bases is None, and with cf_ub = omega_ub (/ tau_u if scale_inv_tau)
      out[v]  = sum_u cf[u, bin(v)] p_bin(v)(v | u) b[u]  -  sum_j named_w[j] (/ tau_user if scale_inv_tau) b[named_user[j]]
      mass[v] = sum_u omega[u, bin(v)] p_bin(v)(v | u)                          (never scaled by 1 / tau)
    A (user, bin) pair is live exactly when tau_u is finite and > 0, gmax and logsum are finite and omega is finite and != 0; a
    pair that is not live -- or that `dead` [U, n_groups + 1] marks: what only the device's bases know, a NaN in them -- contributes
    nothing and leaves no NaN.  named = (offsets [V + 1], users [n], w [n]) as in expect_news_reference, but a named term is gated
    by the USER only (temperature finite and > 0, w != 0, the index in [0, U)), never by a base: a bin emptied by the row still
    receives its entries' terms.  Components of `b` that are not finite count as 0.  Row 0 is zeros minus its named terms.
    Returns (out float64 [V, N], mass float64 [V], A float64 [V, N], M float64 [V]): A_vc = sum_u |cf| p |b_uc| + sum_j |d_j| |b_jc|
    and M_v = sum_u |omega| p, the magnitude sums the error bound of DESIGN.md section 5 is stated on."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        scores = b @ a.T
    scores, pool = _pooled(scores, prior, stamp, window)
    U, V = scores.shape
    bins, G = _bins(group, n_groups, V)
    tau, tau_ok = _temperatures(temperature, U)
    om = np.asarray(bin_w, dtype=np.float64).reshape(U, G + 1)
    clean = np.where(np.isfinite(b), b, 0.0)
    N = b.shape[1]
    out, mass, A, M = np.zeros((V, N)), np.zeros(V), np.zeros((V, N)), np.zeros(V)
    ok = ~np.isnan(scores) & pool
    ok[:, 0] = False
    if exclude is not None:
        for u in range(U):
            ex = np.asarray(exclude[u], dtype=np.int64).reshape(-1)
            ok[u, ex[(ex >= 1) & (ex < V)]] = False
    tau_s = np.where(tau_ok, tau, 1.0)
    it = np.where(tau_ok, 1.0 / tau_s, 0.0) if scale_inv_tau else tau_ok.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for bb in np.unique(bins[1:]):                                 # the users side by side, bin after bin
            cols = np.flatnonzero(bins == bb)
            okb = ok[:, cols]
            has = okb.any(axis=1)
            x = np.where(okb, scores[:, cols], -np.inf)
            if bases is None:
                gm = x.max(axis=1)
                fin = has & tau_ok & np.isfinite(gm)
                ls = np.where(fin, np.log(np.sum(np.exp((x - np.where(fin, gm, 0.0)[:, None]) / tau_s[:, None]), axis=1)), np.nan)
            else:
                ls, gm = np.asarray(bases[0], dtype=np.float64)[:, bb], np.asarray(bases[1], dtype=np.float64)[:, bb]
            w = om[:, bb]
            livep = tau_ok & has & np.isfinite(gm) & np.isfinite(ls) & np.isfinite(w) & (w != 0)
            if dead is not None:
                livep &= ~np.asarray(dead, dtype=bool)[:, bb]
            w = np.where(livep, w, 0.0)
            pw = np.where(okb & livep[:, None], np.exp((x - np.where(livep, gm, 0.0)[:, None]) / tau_s[:, None] - np.where(livep, ls, 0.0)[:, None]), 0.0)
            out[cols] += pw.T @ ((w * it)[:, None] * clean)
            A[cols] += pw.T @ (np.abs(w * it)[:, None] * np.abs(clean))
            mass[cols] += pw.T @ w
            M[cols] += pw.T @ np.abs(w)
        if named is not None:
            off, nu, nw = (np.asarray(x) for x in named)
            for v in range(V):
                for j in range(int(off[v]), int(off[v + 1])):
                    u = int(nu[j])
                    if nw[j] == 0 or not 0 <= u < U or not tau_ok[u]:
                        continue
                    out[v] -= float(nw[j]) * it[u] * clean[u]
                    A[v] += abs(float(nw[j])) * it[u] * np.abs(clean[u])
    return out, mass, A, M


def retrieval_metrics_reference(ranks, ks):
    """Per-user full-corpus retrieval metrics from rank_reference-style ranks [U, T] (0 = not ranked; -1 = capped out, under
    group caps), and their sums over the users with n_u >= 1 ranked targets; n_u counts the ranks != 0, and a rank of -1 adds
    nothing to MRR, Recall@k or nDCG@k while the ideal DCG keeps its min(n_u, k) terms -- the ideal is what a recommender
    without the cap could have shown, so hiding a click costs nDCG instead of shrinking its denominator.  Without a negative
    rank the result is what it always was.
      MRR_u = mean_j 1 / rank;  Recall@k_u = #{rank <= k} / n_u;
      nDCG@k_u = sum_{rank <= k} 1 / log2(rank + 1)  /  sum_{i = 1 .. min(n_u, k)} 1 / log2(i + 1)
    -- mrr_score / ndcg_score above applied to the user's whole eligible corpus row with binary labels.
    Returns (per_user float64 [U, 2 + 2 len(ks)], sums float64 [2 + 2 len(ks)]): column 0 is 1 for a counted user, column 1
    MRR_u, then Recall@k_u, nDCG@k_u per k; the row of a user without a ranked target is zero."""
    ranks = np.asarray(ranks, dtype=np.int64)
    ks = [int(k) for k in ks]
    per_user = np.zeros((ranks.shape[0], 2 + 2 * len(ks)), dtype=np.float64)
    for u, row in enumerate(ranks):
        r = row[row > 0].astype(np.float64)
        n = int(np.count_nonzero(row))
        if n == 0:
            continue
        per_user[u, 0], per_user[u, 1] = 1.0, np.sum(1.0 / r) / n
        for i, k in enumerate(ks):
            hit = r[r <= k]
            per_user[u, 2 + 2 * i] = len(hit) / n
            per_user[u, 3 + 2 * i] = np.sum(1.0 / np.log2(hit + 1.0)) / np.sum(1.0 / np.log2(np.arange(min(n, k)) + 2.0))
    return per_user, per_user.sum(axis=0)

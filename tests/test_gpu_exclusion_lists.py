"""GPU: exclusion lists of any length (CSR; include/nrhip.h K9 / K10) through ops.score_topk, ops.score_rank, train.recommend and
train.rank_eval, against metrics.topk_reference / rank_reference.

The integer data are those of tests/test_gpu_topk.py: vector entries in -2 .. 2, so every score is an integer that fp32 holds
exactly in any summation order and ties are plentiful -- ids and scores are compared for equality.  The float-data tests compare
device results with device results, bit for bit.  List lengths sit around everything the kernels treat differently: 0, 1, the
64 ids that ride with the targets in the rank pass, the 128 of one chunk / one load of the search, more, and nearly the whole
corpus (a partly filled and an all-fill row)."""
import numpy as np
import pytest
import torch

from helpers import build_model
from newsrecommendation_amd import metrics, ops, train as TR

pytestmark = pytest.mark.gpu

INF = float("inf")
SPLITS = (0, 1, 3)


def _ints(V, U, N, seed):
    g = torch.Generator().manual_seed(seed)
    news = torch.randint(-2, 3, (V, N), generator=g).float()
    user = torch.randint(-2, 3, (U, N), generator=g).float()
    return news, user


def _floats(V, U, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(V, N, generator=g) * 0.4, torch.randn(U, N, generator=g) * 0.4


def _lengths(V):
    return (0, 1, 63, 64, 65, 127, 128, 129, 200, V - 20, V - 1)


def _slice_edges(V, splits=3):
    """the two ids either side of every boundary between the `splits` corpus slices (slice s starts at 1 + s * per)"""
    per = (V - 1 + splits - 1) // splits
    return sorted({v for s in range(1, splits) for v in (s * per, 1 + s * per) if 1 <= v < V})


def _draw_lists(plain_top, V, seed, extras=True):
    """One id list per user: lengths cycle through _lengths(V); half of each list (up to all 128) comes from the user's plain
    top-128 row, or the exclusion would do nothing.  With `extras` the last two users get the ids 1 .. 256 (two whole chunks, the
    first chunk of a slice among them) and the ids at the slice boundaries of splits = 3."""
    g = np.random.default_rng(seed)
    U = plain_top.shape[0]
    lens = _lengths(V)
    lists = []
    for u in range(U):
        L = lens[u % len(lens)]
        top = plain_top[u][plain_top[u] > 0]
        hit = g.permutation(top)[:min((L + 1) // 2, len(top))]
        rest = np.setdiff1d(np.arange(1, V), hit)
        lists.append(g.permutation(np.concatenate([hit, g.permutation(rest)[:L - len(hit)]])).astype(np.int64))
        assert len(lists[-1]) == L == len(set(lists[-1].tolist()))
    if extras:
        lists[-2] = np.arange(1, min(257, V), dtype=np.int64)
        lists[-1] = np.asarray(_slice_edges(V), dtype=np.int64)
    return lists


def _topk(news_d, user_d, k, exclude=None, splits=0, **kw):
    ids, sc = ops.score_topk(news_d, user_d, k, exclude=exclude, splits=splits, **kw)
    assert ids.dtype == torch.int32 and sc.dtype == torch.float32 and ids.shape == sc.shape == (user_d.shape[0], k)
    return ids.cpu().numpy(), sc.cpu().numpy()


def _rank(news_d, user_d, tg, exclude=None, splits=0, **kw):
    ranks, sc, _ = ops.score_rank(news_d, user_d, torch.as_tensor(tg).cuda(), exclude=exclude, ks=None, splits=splits, **kw)
    return ranks.cpu().numpy(), sc.cpu().numpy()


# ---- 1: top-k sweep ----

@pytest.mark.parametrize("V", [1000, 4099])
@pytest.mark.parametrize("N", [24, 400])
def test_topk_sweep(N, V):
    """U = 67 (65 users whose list lengths cycle through 0, 1, 63, 64, 65, 127, 128, 129, 200, V - 20, V - 1, and the two extra
    lists of _draw_lists) x splits in {0, 1, 3} x k in {10, 128}: ids and scores equal the reference.  One reference per (N, V):
    k = 128, of which k = 10 is the prefix."""
    U = 67
    news, user = _ints(V, U, N, seed=7000 * N + V)
    plain, _ = metrics.topk_reference(news.numpy(), user.numpy(), k=128)
    lists = _draw_lists(plain, V, seed=N + V)
    ref_ids, ref_sc = metrics.topk_reference(news.numpy(), user.numpy(), k=128, exclude=lists)
    part, fill = 9 % len(_lengths(V)), 10 % len(_lengths(V))                                       # users with V - 20 and V - 1 listed ids
    assert (ref_ids[part, :19] > 0).all() and (ref_ids[part, 19:] == 0).all() and (ref_ids[fill] == 0).all()
    assert (ref_ids[:9] != plain[:9]).any(axis=1)[1:].all()                                       # the exclusion bites
    news_d, user_d = news.cuda(), user.cuda()
    ex = ops.ExclusionLists(lists, device="cuda")                                                 # built once, used by every call
    for splits in SPLITS:
        for k in (10, 128):
            ids, sc = _topk(news_d, user_d, k, exclude=ex, splits=splits)
            assert np.array_equal(ids, ref_ids[:, :k]), (splits, k, np.flatnonzero((ids != ref_ids[:, :k]).any(axis=1)))
            assert np.array_equal(sc, ref_sc[:, :k]), (splits, k)


# ---- 2: the raw contract ----

def test_raw_contract_out_of_range_entries_and_the_clamp():
    """from_sorted: segments with negatives and a zero at the front and ids >= V at the back give the rows of the cleaned lists
    (top-k and rank alike).  An offsets array whose last entry exceeds n_excl returns, with in-range ids: only that is asserted."""
    V, U, N = 1000, 33, 24
    news, user = _ints(V, U, N, seed=77)
    plain, _ = metrics.topk_reference(news.numpy(), user.numpy(), k=128)
    clean = _draw_lists(plain, V, seed=78, extras=False)
    segs = [np.concatenate([[-9, -2, 0], np.sort(c), [V, V + 3, 2**31 - 1]]).astype(np.int64) if u % 3 else np.sort(c) for u, c in enumerate(clean)]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    raw = ops.ExclusionLists.from_sorted(torch.as_tensor(offsets).cuda(), torch.as_tensor(np.concatenate(segs)).cuda())
    ref_ids, ref_sc = metrics.topk_reference(news.numpy(), user.numpy(), k=128, exclude=clean)
    news_d, user_d = news.cuda(), user.cuda()
    for splits in (0, 3):
        ids, sc = _topk(news_d, user_d, 128, exclude=raw, splits=splits)
        assert np.array_equal(ids, ref_ids) and np.array_equal(sc, ref_sc), splits
    tg = np.concatenate([plain[:, :6], np.stack([np.sort(c)[:3] if len(c) >= 3 else np.zeros(3, np.int64) for c in clean])], axis=1).astype(np.int32)
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=clean)
    ranks, sc = _rank(news_d, user_d, tg, exclude=raw)
    assert np.array_equal(ranks, ref_r) and np.array_equal(sc, ref_s.astype(np.float32))

    bad = offsets.copy()
    bad[-1] += 1000                                                                               # past the end of excl_ids
    over = ops.ExclusionLists.from_sorted(torch.as_tensor(bad).cuda(), raw.ids)
    ids, sc = _topk(news_d, user_d, 128, exclude=over, splits=3)
    assert ((ids >= 0) & (ids < V)).all()
    ranks, sc = _rank(news_d, user_d, tg, exclude=over)
    assert ((ranks >= 0) & (ranks < V)).all()


# ---- 3, 4: float data, bit for bit ----

def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def test_csr_equals_dense_bitwise_on_float_data():
    """Lists of 40 ids per user as a [U, 40] tensor (the dense path, the launch it always was) and as ExclusionLists (the CSR
    path): the same ids and the same score bits, k in {10, 128} x splits in {0, 3}; rank likewise."""
    V, U, N = 4099, 65, 400
    news, user = _floats(V, U, N, seed=31)
    news_d, user_d = news.cuda(), user.cuda()
    top, _ = _topk(news_d, user_d, 128)
    g = np.random.default_rng(32)
    dense = np.stack([np.concatenate([g.permutation(top[u])[:20], g.permutation(np.setdiff1d(np.arange(1, V), top[u]))[:20]]) for u in range(U)])
    dense_d = torch.as_tensor(dense.astype(np.int32)).cuda()
    lists = ops.ExclusionLists(dense_d)
    assert lists.ids.numel() == U * 40
    for k in (10, 128):
        for splits in (0, 3):
            a_ids, a_sc = _topk(news_d, user_d, k, exclude=dense_d, splits=splits)
            b_ids, b_sc = _topk(news_d, user_d, k, exclude=lists, splits=splits)
            assert (a_ids[:, :10] != top[:, :10]).any()                                           # the exclusion bites
            assert np.array_equal(a_ids, b_ids) and np.array_equal(_bits(a_sc), _bits(b_sc)), (k, splits)
    tg = np.concatenate([top[:, :24], dense[:, :4], dense[:, 20:24] + 1], axis=1).astype(np.int32) % V
    for splits in (0, 3):
        a_r, a_s = _rank(news_d, user_d, tg, exclude=dense_d, splits=splits)
        b_r, b_s = _rank(news_d, user_d, tg, exclude=lists, splits=splits)
        assert np.array_equal(a_r, b_r) and np.array_equal(_bits(a_s), _bits(b_s)), splits
        assert (a_r[:, 24:28] == 0).all() and (a_r[:, :24] > 0).any()


def test_csr_against_the_plain_call_bitwise_on_float_data():
    """The list is 100 ids of the user's plain k = 128 row: the CSR k = 10 row must be the first 10 of the plain row with the
    listed ids removed, ids and score bits."""
    V, U, N = 4099, 65, 400
    news, user = _floats(V, U, N, seed=41)
    news_d, user_d = news.cuda(), user.cuda()
    top, top_sc = _topk(news_d, user_d, 128)
    g = np.random.default_rng(42)
    drop = [np.sort(g.permutation(128)[:100]) for _ in range(U)]
    lists = ops.ExclusionLists([top[u][drop[u]] for u in range(U)], device="cuda")
    for splits in (0, 3):
        ids, sc = _topk(news_d, user_d, 10, exclude=lists, splits=splits)
        for u in range(U):
            keep = np.setdiff1d(np.arange(128), drop[u])[:10]
            assert np.array_equal(ids[u], top[u][keep]) and np.array_equal(_bits(sc[u]), _bits(top_sc[u][keep])), (splits, u)


# ---- 5: combinations ----

def _pools(V, U, seed):
    """prior: multiples of 1/4 in [-2, 2] (exact in fp32 next to integer scores), some -inf; stamps 0 .. 9; windows (lo, hi)"""
    g = np.random.default_rng(seed)
    prior = (g.integers(-8, 9, V) / 4.0).astype(np.float32)
    prior[g.random(V) < 0.1] = -INF
    stamp = g.integers(0, 10, V).astype(np.int32)
    window = np.sort(g.integers(0, 10, (U, 2)), axis=1).astype(np.int32)
    window[1], window[2] = [5, 4], [0, 9]
    return prior, stamp, window


def test_csr_with_prior_and_window():
    V, U, N = 1000, 65, 24
    news, user = _ints(V, U, N, seed=51)
    prior, stamp, window = _pools(V, U, seed=52)
    plain, _ = metrics.topk_reference(news.numpy(), user.numpy(), k=128, prior=prior, stamp=stamp, window=window)
    lists = _draw_lists(plain, V, seed=53)
    ref_ids, ref_sc = metrics.topk_reference(news.numpy(), user.numpy(), k=128, exclude=lists, prior=prior, stamp=stamp, window=window)
    kw = dict(prior=torch.as_tensor(prior).cuda(), stamp=torch.as_tensor(stamp).cuda(), window=torch.as_tensor(window).cuda())
    ex = ops.ExclusionLists(lists, device="cuda")
    for splits in (0, 3):
        ids, sc = _topk(news.cuda(), user.cuda(), 128, exclude=ex, splits=splits, **kw)
        assert np.array_equal(ids, ref_ids) and np.array_equal(sc, ref_sc.astype(np.float32)), splits


def test_csr_with_group_caps():
    V, U, N = 1000, 65, 24
    news, user = _ints(V, U, N, seed=55)
    g = np.random.default_rng(56)
    group = g.integers(-1, 18, V).astype(np.int32)                                                # 18 groups, some news in none
    plain, _ = metrics.topk_reference(news.numpy(), user.numpy(), k=128, group=group, group_cap=2)
    lists = _draw_lists(plain, V, seed=57)
    ref_ids, ref_sc = metrics.topk_reference(news.numpy(), user.numpy(), k=128, exclude=lists, group=group, group_cap=2)
    ex = ops.ExclusionLists(lists, device="cuda")
    for splits in (0, 3):
        for k in (10, 128):
            ids, sc = _topk(news.cuda(), user.cuda(), k, exclude=ex, splits=splits, group=torch.as_tensor(group).cuda(), group_cap=2)
            assert np.array_equal(ids, ref_ids[:, :k]) and np.array_equal(sc, ref_sc[:, :k].astype(np.float32)), (splits, k)


# ---- 6: rank sweep ----

def _rank_targets(plain, lists, V, T, seed):
    """[U, 64]: the user's best news, listed ids (rank 0), the ids just ahead of and just behind listed ones, random ids, a 0 and
    a repeat; the first T columns are used."""
    g = np.random.default_rng(seed)
    U = plain.shape[0]
    t = g.integers(1, V, (U, 64)).astype(np.int32)
    for u in range(U):
        L = np.asarray(lists[u])
        t[u, 0] = plain[u, 0]
        if len(L):
            pick = g.permutation(L)[:12]
            t[u, 1:1 + len(pick[:4])] = pick[:4]
            t[u, 8:8 + len(pick[4:8])] = np.clip(pick[4:8] - 1, 0, V - 1)
            t[u, 16:16 + len(pick[8:12])] = np.clip(pick[8:12] + 1, 0, V - 1)
        t[u, 5], t[u, 6] = 0, t[u, 0]
        t[u, 24:40] = plain[u, g.permutation(128)[:16]]
    if T == 1:
        t[1::2, 0] = [lists[u][0] if len(lists[u]) else plain[u, 0] for u in range(1, U, 2)]      # every other user: a listed target
        t[0::4, 0] = plain[0::4, 100]                                                             # deep enough for the lists to take ranks off
    return t[:, :T].copy()


@pytest.mark.parametrize("T", [1, 7, 64])
def test_rank_sweep(T):
    """T in {1, 7, 64} x the list lengths of the top-k sweep (the extra lists included) x splits in {0, 1, 3}: ranks and scores
    equal the reference.  N = 400 for T = 64, else 24."""
    V, U, N = 1000, 67, 400 if T == 64 else 24
    news, user = _ints(V, U, N, seed=600 + T)
    plain, _ = metrics.topk_reference(news.numpy(), user.numpy(), k=128)
    lists = _draw_lists(plain, V, seed=610 + T)
    tg = _rank_targets(plain, lists, V, T, seed=620 + T)
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=lists)
    assert (ref_r == 0).any() and (ref_r > 0).any()
    no_list_r, _ = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg)
    assert (ref_r[(ref_r > 0)] <= no_list_r[(ref_r > 0)]).all() and (ref_r[ref_r > 0] < no_list_r[ref_r > 0]).any()   # the lists take ranks off
    news_d, user_d = news.cuda(), user.cuda()
    ex = ops.ExclusionLists(lists, device="cuda")
    for splits in SPLITS:
        ranks, sc = _rank(news_d, user_d, tg, exclude=ex, splits=splits)
        assert np.array_equal(ranks, ref_r), (splits, np.argwhere(ranks != ref_r)[:5])
        assert np.array_equal(sc, ref_s.astype(np.float32)), splits


def test_rank_with_lists_and_pools():
    """The pooled form once: listed ids outside the user's window (or with a prior of -inf) take nothing off a rank."""
    V, U, N, T = 1000, 67, 24, 7
    news, user = _ints(V, U, N, seed=631)
    prior, stamp, window = _pools(V, U, seed=632)
    pools = dict(prior=prior, stamp=stamp, window=window)
    plain, _ = metrics.topk_reference(news.numpy(), user.numpy(), k=128, **pools)
    lists = _draw_lists(plain, V, seed=633)
    tg = _rank_targets(plain, lists, V, T, seed=634)
    ref_r, ref_s = metrics.rank_reference(news.numpy(), user.numpy(), targets=tg, exclude=lists, **pools)
    assert (ref_r > 0).any()
    kw = {k: torch.as_tensor(v).cuda() for k, v in pools.items()}
    ex = ops.ExclusionLists(lists, device="cuda")
    for splits in (0, 3):
        ranks, sc = _rank(news.cuda(), user.cuda(), tg, exclude=ex, splits=splits, **kw)
        assert np.array_equal(ranks, ref_r) and np.array_equal(sc, ref_s.astype(np.float32)), splits


# ---- 7: the two calls agree ----

def test_rank_agrees_with_score_topk_bitwise_under_lists():
    """Float data, the same CSR lists of 150 ids per user for both calls: 1 <= rank <= k exactly when the target is at place
    rank - 1 of the score_topk row, and the scores are equal bitwise."""
    V, U, N, k = 4099, 65, 400, 128
    news, user = _floats(V, U, N, seed=71)
    news_d, user_d = news.cuda(), user.cuda()
    top, _ = _topk(news_d, user_d, k)
    g = np.random.default_rng(72)
    lists = [np.concatenate([g.permutation(top[u])[:75], g.permutation(np.setdiff1d(np.arange(1, V), top[u]))[:75]]) for u in range(U)]
    ex = ops.ExclusionLists(lists, device="cuda")
    assert ex.ids.numel() == 150 * U
    row, row_sc = _topk(news_d, user_d, k, exclude=ex)
    tg = np.concatenate([row[:, g.permutation(k)[:32]], g.integers(1, V, (U, 24)), np.stack([l[:8] for l in lists])], axis=1).astype(np.int32)
    for splits in (0, 3):
        ranks, sc = _rank(news_d, user_d, tg, exclude=ex, splits=splits)
        for u in range(U):
            place = {int(v): p for p, v in enumerate(row[u])}
            first = {}
            for j, t in enumerate(tg[u].tolist()):
                first.setdefault(t, j)
            for j, t in enumerate(tg[u].tolist()):
                if first[t] != j:
                    assert ranks[u, j] == 0                                                       # a repeat
                elif t in place:
                    assert ranks[u, j] == place[t] + 1 and _bits(sc[u, j:j + 1])[0] == _bits(row_sc[u, place[t]:place[t] + 1])[0], (u, j)
                else:
                    assert ranks[u, j] == 0 or ranks[u, j] > k, (u, j)
        assert (ranks[:, 56:] == 0).all() and (ranks[:, :32] > 0).all()


# ---- 8: train.recommend / train.rank_eval with a history of 80 slots ----

def _corpus(n_news, seed):
    g = torch.Generator().manual_seed(seed)
    nc = torch.randint(1, 12, (n_news + 1, 4), generator=g, dtype=torch.int32)           # word ids of a 12-word vocabulary
    cut = torch.randint(1, 5, (n_news + 1,), generator=g)
    nc[torch.arange(4)[None, :] >= cut[:, None]] = 0                                      # titles of 1 .. 4 words
    nc[0] = 0
    return nc


class _MeanUserModel:
    """The project's user encoders attend over at most 64 history slots (the attention and pooling kernels take L <= 64), so no
    model of this repository turns 80 live slots into a user vector.  What is under test here is everything behind the user
    vector -- how recommend / rank_eval turn history and `seen` into exclusions, and the kernels -- so the user vector comes
    from a stand-in: the masked mean of the history's news vectors.  train._user_vectors gathers the rows and calls it."""
    args = None

    @staticmethod
    def user_encoder(log_vecs, mask):
        m = mask.to(log_vecs.dtype)[:, :, None]
        return (log_vecs.float() * m).sum(1) / m.sum(1).clamp(min=1.0)


def _hot_history_model(U=8, H=80, n_news=300):
    """The news table of tests/test_gpu_topk.py's recommend test (its model, encode_news over 300 synthetic news), histories of
    H = 80 live slots.  The table rows of each user's first 16 history slots (news 1 + 16 u .. 16 + 16 u, nobody else's) are
    set to 3 e_u, so that exactly those news score highest for that user (asserted).  Returns the stand-in model, the table,
    hist, mask and the float64 scores of the user vectors recommend will form."""
    real, z, cfg, sd = build_model("nrms_tiny_mask", "fp32")
    dev = torch.device("cuda")
    news_vecs = TR.encode_news(real, _corpus(n_news, seed=81), 64, dev).clone()
    assert news_vecs.shape == (n_news + 1, cfg.news_dim) and cfg.news_dim >= U
    g = torch.Generator().manual_seed(82)
    hist = torch.zeros(U, H, dtype=torch.int32)
    for u in range(U):
        hist[u, :16] = torch.arange(1 + 16 * u, 17 + 16 * u)
        hist[u, 16:] = torch.randint(16 * U + 1, n_news + 1, (H - 16,), generator=g)
        news_vecs[1 + 16 * u:17 + 16 * u] = 3.0 * torch.eye(cfg.news_dim, device=dev)[u]
    mask = torch.ones(U, H)
    model = _MeanUserModel()
    uv = TR._user_vectors(model, news_vecs, hist.cuda(), mask.cuda(), 8192, dev, TR._Histories(mask.numpy()))
    r = uv.double().cpu().numpy() @ news_vecs.double().cpu().numpy().T
    r[:, 0] = -INF
    srt = np.sort(r, axis=1)[:, ::-1]
    assert all(set(np.argsort(-r[u], kind="stable")[:16].tolist()) == set(hist[u, :16].tolist()) for u in range(U))
    assert (srt[:, 15] - srt[:, 16]).min() > 0.1
    return model, news_vecs, hist, mask, r


def test_recommend_and_rank_eval_exclude_a_history_wider_than_64_and_seen_lists():
    """H = 80 live slots (with a stand-in user encoder, see _MeanUserModel): the news of the first 16 history slots score
    highest for their user, so a recommend that only excluded the last 64 slots would return them.  No returned id is in the history, the row is topk_reference's with the full history excluded;
    `seen` lists of 100 further ids are respected; rank_eval with a user of 70 targets and `seen` matches rank_reference."""
    model, news_vecs, hist, mask, r = _hot_history_model()
    U, H, k, V = hist.shape[0], hist.shape[1], 10, news_vecs.shape[0]
    clicked = [set(hist[u].tolist()) for u in range(U)]
    # what excluding only the last 64 slots would give: rows made of the first 16 history news
    trunc, _ = metrics.topk_reference(r, k=k, exclude=hist[:, -64:].numpy())
    assert all(set(trunc[u].tolist()) <= set(hist[u, :16].tolist()) for u in range(U))

    ids, sc = TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), k)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    assert all(not (clicked[u] & set(ids[u].tolist())) for u in range(U))
    ref_ids, ref_sc = metrics.topk_reference(r, k=k, exclude=hist.numpy())
    assert np.array_equal(ids, ref_ids) and np.abs(sc - ref_sc).max() <= 1e-4

    g = np.random.default_rng(83)
    seen = [g.permutation(np.setdiff1d(np.arange(1, V), list(clicked[u])))[:100] for u in range(U)]
    seen[0][:10] = ref_ids[0]                                                             # user 0: its whole row so far
    seen[1][:5] = ref_ids[1][:5]
    both = [np.concatenate([hist[u].numpy(), seen[u]]) for u in range(U)]
    ref_ids2, ref_sc2 = metrics.topk_reference(r, k=k, exclude=both)
    for form in (seen, ops.ExclusionLists(seen)):                                         # a sequence of arrays; lists built on the CPU
        ids2, sc2 = TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), k, seen=form)
        ids2, sc2 = ids2.cpu().numpy(), sc2.cpu().numpy()
        assert all(not ((clicked[u] | set(seen[u].tolist())) & set(ids2[u].tolist())) for u in range(U))
        assert np.array_equal(ids2, ref_ids2) and np.abs(sc2 - ref_sc2).max() <= 1e-4
    only_seen, _ = TR.recommend(model, news_vecs, hist.numpy(), mask.numpy(), k, exclude_history=False, seen=seen)
    assert np.array_equal(only_seen.cpu().numpy(), metrics.topk_reference(r, k=k, exclude=seen)[0])

    T = 70                                                                                # user 0: 70 targets -> two rows that share its lists
    tg = np.zeros((U, T), dtype=np.int32)
    tg[0] = g.permutation(np.arange(1, V))[:T]
    tg[0, :3] = [int(hist[0, 0]), int(seen[0][0]), int(ref_ids2[0, 0])]
    tg[1:, 0] = ref_ids2[1:, 0]
    tg[1:, 1:7] = g.integers(1, V, (U - 1, 6))
    ref_r, ref_s = metrics.rank_reference(r, targets=tg, exclude=both)
    assert ref_r[0, 0] == 0 and ref_r[0, 1] == 0 and ref_r[0, 2] == 1 and (ref_r[1:, 0] == 1).all()
    ranks, rsc, sums = TR.rank_eval(model, news_vecs, hist.numpy(), mask.numpy(), tg, ks=(5, 10), seen=seen)
    ranks, rsc = ranks.cpu().numpy(), rsc.cpu().numpy()
    assert np.array_equal(ranks, ref_r), np.argwhere(ranks != ref_r)[:5]
    assert np.abs(rsc[ref_r > 0] - ref_s[ref_r > 0]).max() <= 1e-4
    want = metrics.retrieval_metrics_reference(ref_r, (5, 10))[1]
    assert np.allclose(sums.cpu().numpy(), want, rtol=1e-12, atol=0)

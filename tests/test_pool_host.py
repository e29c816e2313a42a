"""CPU: the host side of the pools of the full-corpus passes (a per-news prior, per-news stamps against a per-user window) --
the semantics of metrics.topk_reference / rank_reference pinned on a hand-worked table, neutral inputs, the checks
nr_score_topk / nr_score_rank make on the new descriptor fields before they launch anything (fake non-null pointers: a launch
would fault, a refusal does not), the workspace sizes, and the way train.rank_eval carries a window over the rows of a user
with more than 64 targets."""
import ctypes as C

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")

# V = 8, the same dot products for three users.  id:  0    1    2     3    4    5    6    7
DOT = np.array([9.0, 5.0, 3.0, 5.0, 1.0, 7.0, 2.0, 4.0])
PRIOR = np.array([0.0, 0.0, 1.0, -INF, NAN, -1.0, 0.5, 0.0])         # final: -    5    4   (out) NaN    6   2.5    4
STAMP = np.array([5, 3, 4, 4, 4, 6, 7, 2])
WINDOW = np.array([[3, 6],      # user 0: ids 1 (stamp 3 = lo) .. 5 (stamp 6 = hi) are inside, both edges inclusive; 6 and 7 are not
                   [5, 4],      # user 1: lo > hi, nobody
                   [0, 9]])     # user 2: everybody
SCORES = np.tile(DOT, (3, 1))


def test_refusals_of_half_a_window_before_any_launch():
    """The first test to run on a build: stamp without window, window without stamp and a window row stride below 2 are refused
    by both calls with code 1 and a message that names the field; the same descriptors with the pair complete pass the check
    (their workspace query answers)."""
    lib = _lib.lib()
    topk = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, k=10, exclude=4096, ld_exclude=50, E=50,
                splits=0, out_ids=4096, out_scores=4096, ws=4096)
    rank = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, T=4, targets=4096, ld_targets=4, exclude=4096,
                ld_exclude=50, E=50, splits=0, ks=(C.c_int * 3)(5, 10, 100), n_ks=3, out_ranks=4096, out_scores=4096, out_sums=4096, ws=4096)
    cases = ((dict(stamp=4096), "stamp given without window"), (dict(window=4096, ld_window=2), "window given without stamp"),
             (dict(stamp=4096, window=4096, ld_window=1), "ld_window = 1"), (dict(prior=4096, stamp=4096, window=4096, ld_window=0), "ld_window = 0"))
    for Desc, base, size, call in ((_lib.TopkDesc, topk, lib.nr_score_topk_workspace_bytes, lib.nr_score_topk),
                                   (_lib.RankDesc, rank, lib.nr_score_rank_workspace_bytes, lib.nr_score_rank)):
        plain = size(C.byref(Desc(**base)))
        assert plain > 0
        for change, message in cases:
            d = Desc(**base, **change)
            d.ws_bytes = plain
            assert call(C.byref(d), None) == 1 and message in _lib.last_error(), (change, _lib.last_error())
            assert size(C.byref(d)) == 0
        # the workspace does not depend on the new fields
        for change in (dict(prior=4096), dict(stamp=4096, window=4096, ld_window=2), dict(prior=4096, stamp=4096, window=4096, ld_window=5)):
            assert size(C.byref(Desc(**base, **change))) == plain, change


def test_descriptors_end_in_the_pool_fields():
    for Desc in (_lib.TopkDesc, _lib.RankDesc):
        assert [f[0] for f in Desc._fields_][-6:] == ["ws", "ws_bytes", "prior", "stamp", "window", "ld_window"]
    sizes = (C.c_size_t * 9)()
    assert _lib.lib().nr_abi_sizes(sizes, 9) == 0 and sizes[7] == C.sizeof(_lib.TopkDesc) and sizes[8] == C.sizeof(_lib.RankDesc)


def test_hand_worked_table_topk():
    ids, sc = metrics.topk_reference(SCORES, k=6, prior=PRIOR, stamp=STAMP, window=WINDOW)
    fill = [-INF] * 6
    # user 0: 5 (7 - 1 = 6, stamp on the upper edge), 1 (5, stamp on the lower edge), 2 (3 + 1 = 4); 3 has a -inf prior, 4 a NaN one,
    # 6 and 7 lie outside the window although 7's score ties 2's
    assert ids[0].tolist() == [5, 1, 2, 0, 0, 0] and sc[0].tolist() == [6.0, 5.0, 4.0] + fill[:3]
    assert ids[1].tolist() == [0] * 6 and sc[1].tolist() == fill                       # an empty window: all fill
    assert ids[2].tolist() == [5, 1, 2, 7, 6, 0] and sc[2].tolist() == [6.0, 5.0, 4.0, 4.0, 2.5, -INF]      # the tie 2 / 7: id ascending
    # the prior alone: -inf and NaN still remove 3 and 4
    ids, sc = metrics.topk_reference(SCORES, k=6, prior=PRIOR)
    assert ids[1].tolist() == [5, 1, 2, 7, 6, 0]
    # the window alone: plain dot products, 3 (5, ties 1) and 4 are back
    ids, sc = metrics.topk_reference(SCORES, k=6, stamp=STAMP, window=WINDOW)
    assert ids[0].tolist() == [5, 1, 3, 2, 4, 0] and sc[0].tolist() == [7.0, 5.0, 5.0, 3.0, 1.0, -INF]
    assert ids[1].tolist() == [0] * 6
    # an excluded id outside the window (7) changes nothing for user 0; excluding 5 does
    ids, _ = metrics.topk_reference(SCORES, k=3, prior=PRIOR, stamp=STAMP, window=WINDOW, exclude=[[7, 5]] * 3)
    assert ids.tolist() == [[1, 2, 0], [0, 0, 0], [1, 2, 6]]
    # the same from vectors: dot = <news, user>
    news = np.stack([DOT, np.zeros(8)], 1)
    ids_v, sc_v = metrics.topk_reference(news, np.array([[1.0, 0.0]] * 3), k=6, prior=PRIOR, stamp=STAMP, window=WINDOW)
    assert ids_v[2].tolist() == [5, 1, 2, 7, 6, 0] and sc_v[0].tolist() == [6.0, 5.0, 4.0] + fill[:3]


def test_hand_worked_table_rank():
    tg = np.tile(np.array([1, 2, 7, 5, 3, 4, 6, 0]), (3, 1))
    ranks, sc = metrics.rank_reference(SCORES, targets=tg, prior=PRIOR, stamp=STAMP, window=WINDOW)
    assert ranks.tolist() == [[2, 3, 0, 1, 0, 0, 0, 0], [0] * 8, [2, 3, 4, 1, 0, 0, 5, 0]]
    assert sc[0].tolist() == [5.0, 4.0, -INF, 6.0, -INF, -INF, -INF, -INF] and np.isneginf(sc[1]).all()
    assert sc[2].tolist() == [5.0, 4.0, 4.0, 6.0, -INF, -INF, 2.5, -INF]
    # user 0: 7 is excluded AND outside the window -- it was never ahead of anybody, so only 5's exclusion moves the ranks
    ranks, _ = metrics.rank_reference(SCORES, targets=tg, prior=PRIOR, stamp=STAMP, window=WINDOW, exclude=[[7, 5]] * 3)
    assert ranks.tolist() == [[1, 2, 0, 0, 0, 0, 0, 0], [0] * 8, [1, 2, 0, 0, 0, 0, 3, 0]]
    ranks7, _ = metrics.rank_reference(SCORES, targets=tg, prior=PRIOR, stamp=STAMP, window=WINDOW, exclude=[[7]] * 3)
    assert ranks7[0].tolist() == [2, 3, 0, 1, 0, 0, 0, 0] and ranks7[2].tolist() == [2, 3, 0, 1, 0, 0, 4, 0]
    # ranks are the places of the top-k rows
    ids, tsc = metrics.topk_reference(SCORES, k=7, prior=PRIOR, stamp=STAMP, window=WINDOW, exclude=[[7, 5]] * 3)
    for u in range(3):
        for j in range(8):
            if ranks[u, j]:
                assert ids[u, ranks[u, j] - 1] == tg[u, j]
    with pytest.raises(ValueError, match="come together"):
        metrics.rank_reference(SCORES, targets=tg, stamp=STAMP)
    with pytest.raises(ValueError, match="come together"):
        metrics.topk_reference(SCORES, k=2, window=WINDOW)


def test_neutral_inputs_change_nothing():
    g = np.random.default_rng(3)
    news, user = g.integers(-2, 3, (40, 8)).astype(np.float64), g.integers(-2, 3, (7, 8)).astype(np.float64)
    news[11] = np.nan
    stamp = g.integers(0, 10, 40)
    cover = np.tile(np.array([[0, 9]]), (7, 1))
    ex = g.integers(0, 40, (7, 5))
    tg = g.integers(0, 44, (7, 9))
    plain_t = metrics.topk_reference(news, user, k=12, exclude=ex)
    plain_r = metrics.rank_reference(news, user, targets=tg, exclude=ex)
    for kw in (dict(prior=np.zeros(40)), dict(stamp=stamp, window=cover), dict(prior=np.zeros(40), stamp=stamp, window=cover),
               dict(prior=None, stamp=None, window=None)):
        got_t = metrics.topk_reference(news, user, k=12, exclude=ex, **kw)
        got_r = metrics.rank_reference(news, user, targets=tg, exclude=ex, **kw)
        assert np.array_equal(got_t[0], plain_t[0]) and np.array_equal(got_t[1], plain_t[1])
        assert np.array_equal(got_r[0], plain_r[0]) and np.array_equal(got_r[1], plain_r[1])
    # and a prior that is not neutral moves them
    assert not np.array_equal(metrics.topk_reference(news, user, k=12, prior=g.integers(-8, 9, 40) / 4.0)[0], metrics.topk_reference(news, user, k=12)[0])


def test_pool_arguments_of_the_ops_are_checked_and_converted():
    cpu = torch.device("cpu")
    p, s, w = ops._pool_args("score_topk", 5, 3, cpu, torch.zeros(5, dtype=torch.float64), torch.arange(5), torch.zeros(3, 2, dtype=torch.int64))
    assert p.dtype == torch.float32 and s.dtype == torch.int32 and w.dtype == torch.int32 and w.is_contiguous()
    assert ops._pool_args("score_topk", 5, 3, cpu, None, None, None) == (None, None, None)
    w2 = ops._pool_args("score_rank", 5, 3, cpu, None, torch.arange(5), torch.zeros(3, 4, dtype=torch.int32)[:, ::2])[2]
    assert w2.is_contiguous() and w2.shape == (3, 2)
    for bad, message in (((None, torch.arange(5), None), "come together"), ((None, None, torch.zeros(3, 2, dtype=torch.int32)), "come together"),
                         ((torch.zeros(4), None, None), "prior must be a tensor of shape"), ((torch.zeros(5, dtype=torch.int32), None, None), "floating point"),
                         ((None, torch.zeros(5), torch.zeros(3, 2, dtype=torch.int32)), "integer"),
                         ((None, torch.arange(5), torch.zeros(2, 3, dtype=torch.int32)), "window must be a tensor of shape")):
        with pytest.raises(RuntimeError, match=message):
            ops._pool_args("score_topk", 5, 3, cpu, *bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_topk(torch.zeros(10, 8), torch.zeros(3, 8), 2, prior=torch.zeros(10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_rank(torch.zeros(10, 8), torch.zeros(3, 8), torch.ones(3, 2, dtype=torch.int32), stamp=torch.zeros(10, dtype=torch.int32),
                       window=torch.zeros(3, 2, dtype=torch.int32))


def test_row_split_of_rank_eval_carries_the_window(monkeypatch):
    """train.rank_eval with 70 target columns and pools: every 64-wide row of a user gets that user's window (and the prior and
    stamps, which are per news), with the device call replaced by the host reference."""
    g = np.random.default_rng(12)
    V, U, T = 200, 5, 70
    news, user = g.integers(-2, 3, (V, 8)).astype(np.float32), g.integers(-2, 3, (U, 8)).astype(np.float32)
    targets = np.zeros((U, T), np.int32)
    targets[0] = g.permutation(np.arange(1, V))[:T]
    targets[2, :68] = g.permutation(np.arange(1, V))[:68]
    targets[1, :3], targets[3, 0], targets[4, 5] = [9, 10, 11], 50, 17
    hist = g.integers(1, V, (U, 3)).astype(np.int32)
    mask = np.ones((U, 3), np.float32)
    prior = (g.integers(-8, 9, V) / 4.0).astype(np.float32)
    prior[g.random(V) < 0.1] = -INF
    stamp = g.integers(0, 10, V).astype(np.int32)
    window = np.array([[2, 7], [0, 9], [4, 5], [6, 3], [0, 4]], np.int32)
    seen = []

    def fake_score_rank(news_vecs, user_vecs, tg, exclude=None, ks=(), splits=0, prior=None, stamp=None, window=None):
        assert tg.shape[1] <= 64
        seen.append(None if window is None else window.numpy().copy())
        r, s = metrics.rank_reference(news_vecs.numpy(), user_vecs.numpy(), targets=tg.numpy(), exclude=None if exclude is None else exclude.numpy(),
                                      prior=None if prior is None else prior.numpy(), stamp=None if stamp is None else stamp.numpy(),
                                      window=None if window is None else window.numpy())
        return torch.from_numpy(r), torch.from_numpy(s).float(), None

    monkeypatch.setattr(train.ops, "score_rank", fake_score_rank)
    monkeypatch.setattr(train, "_user_vectors", lambda *a: torch.from_numpy(user))
    ks = (1, 10, 100)
    ranks, scores, sums = train.rank_eval(None, torch.from_numpy(news), hist, mask, targets, ks=ks, prior=prior, news_time=stamp, window=window)
    want_r, want_s = metrics.rank_reference(news, user, targets=targets, exclude=hist, prior=prior, stamp=stamp, window=window)
    assert np.array_equal(ranks.numpy(), want_r) and np.array_equal(scores.numpy().astype(np.float64), want_s)
    assert np.allclose(sums.numpy(), metrics.retrieval_metrics_reference(want_r, ks)[1], rtol=1e-12, atol=0)
    assert np.array_equal(seen[0], window[[0, 0, 1, 2, 2, 3, 4]])                      # users 0 and 2 take two rows each
    assert (want_r[3] == 0).all() and (want_r[0] > 0).sum() > 5 and (want_r[0] == 0).sum() > 5
    plain = metrics.rank_reference(news, user, targets=targets, exclude=hist)[0]
    assert not np.array_equal(want_r, plain)
    # without pools the call passes no pool keyword at all
    train.rank_eval(None, torch.from_numpy(news), hist, mask, targets, ks=ks)
    assert seen[-1] is None

"""CPU: the host side of full-corpus rank evaluation -- metrics.rank_reference against a brute-force restatement of the
contract, metrics.retrieval_metrics_reference against the reference-style per-row metrics and a hand-computed case,
nr_score_rank_workspace_bytes as host arithmetic, and the checks nr_score_rank makes before it launches anything (fake
non-null pointers: a launch would fault, a refusal does not)."""
import ctypes as C
import math

import numpy as np
import pytest

from newsrecommendation_amd import _lib, metrics


def _brute(scores, targets, exclude):
    """The contract spelled out with Python's sort: eligible = ids 1 .. V-1, not excluded, score not NaN; order = score
    descending, then id ascending; rank = 1-based place of the target in it, 0 for what is not ranked."""
    U, V = scores.shape
    T = targets.shape[1]
    ranks, out = np.zeros((U, T), np.int32), np.full((U, T), -np.inf)
    for u in range(U):
        banned = set(int(e) for e in exclude[u]) if exclude is not None else set()
        rows = sorted((-float(scores[u, v]), v) for v in range(1, V) if v not in banned and not math.isnan(scores[u, v]))
        ids = [v for _, v in rows]
        for j in range(T):
            t = int(targets[u, j])
            if t in ids and t not in [int(x) for x in targets[u, :j]]:
                ranks[u, j], out[u, j] = ids.index(t) + 1, scores[u, t]
    return ranks, out


def test_reference_matches_brute_force_on_tied_integer_scores():
    g = np.random.default_rng(7)
    news = g.integers(-2, 3, (30, 8)).astype(np.float64)
    user = g.integers(-2, 3, (9, 8)).astype(np.float64)
    scores = user @ news.T
    assert len(np.unique(scores)) < scores.size // 4                     # many ties
    exclude = g.integers(1, 30, (9, 6))
    exclude[:, 1] = 0
    exclude[:, 2] = exclude[:, 0]
    exclude[:, 3] = 30 + g.integers(0, 5, 9)
    exclude[:, 4] = -3
    targets = g.integers(1, 30, (9, 8))
    targets[:, 1] = 0                                                    # no entry
    targets[:, 3] = targets[:, 0]                                        # a duplicate
    targets[:, 4] = 30 + g.integers(0, 5, 9)                             # out of range
    targets[:, 5] = -2                                                   # negative
    targets[:, 6] = exclude[:, 0]                                        # an excluded target
    for ex in (None, exclude):
        want = _brute(scores, targets, ex)
        got = metrics.rank_reference(scores, targets=targets, exclude=ex)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got_v = metrics.rank_reference(news, user, targets=targets, exclude=ex)      # the same from the vectors
        assert np.array_equal(got_v[0], want[0]) and np.array_equal(got_v[1], want[1])
        assert (got[0][:, [1, 3, 4, 5]] == 0).all() and np.isneginf(got[1][:, [1, 3, 4, 5]]).all()
        assert (got[0][:, 0] > 0).all() or ex is not None
    assert (metrics.rank_reference(scores, targets=targets, exclude=exclude)[0][:, 6] == 0).all()
    # the ranks are the places of topk_reference's rows
    ids, _ = metrics.topk_reference(scores, k=29, exclude=exclude)
    ranks, _ = metrics.rank_reference(scores, targets=targets, exclude=exclude)
    for u in range(9):
        for j in range(8):
            if ranks[u, j]:
                assert ids[u, ranks[u, j] - 1] == targets[u, j]


def test_reference_does_not_rank_a_nan_news_and_keeps_the_others():
    g = np.random.default_rng(8)
    scores = g.integers(-3, 4, (5, 20)).astype(np.float64)
    targets = np.tile(np.array([7, 3, 19, 1]), (5, 1))
    with_nan = scores.copy()
    with_nan[:, 7] = np.nan
    ranks, sc = metrics.rank_reference(with_nan, targets=targets)
    assert (ranks[:, 0] == 0).all() and np.isneginf(sc[:, 0]).all() and not np.isnan(sc).any()
    want = _brute(scores, targets, np.full((5, 1), 7))                   # the same as excluding that news
    assert np.array_equal(ranks, want[0]) and np.array_equal(sc, want[1])


def test_retrieval_metrics_against_the_reference_style_row_metrics():
    """Tie-free rows: mrr_score / ndcg_score over the user's whole eligible row with binary labels."""
    g = np.random.default_rng(9)
    U, V, ks = 6, 40, (1, 5, 10, 100)
    scores = np.stack([g.permutation(V).astype(np.float64) for _ in range(U)])
    targets = np.stack([g.permutation(np.arange(1, V))[:5] for _ in range(U)])
    targets[2, 1:] = 0                                                   # one target only
    ranks, _ = metrics.rank_reference(scores, targets=targets)
    per_user, sums = metrics.retrieval_metrics_reference(ranks, ks)
    for u in range(U):
        y = np.zeros(V - 1)
        y[targets[u][targets[u] > 0] - 1] = 1
        assert per_user[u, 0] == 1.0
        assert per_user[u, 1] == pytest.approx(metrics.mrr_score(y, scores[u, 1:]), rel=1e-12)
        for i, k in enumerate(ks):
            assert per_user[u, 3 + 2 * i] == pytest.approx(metrics.ndcg_score(y, scores[u, 1:], k), rel=1e-12)
            top = np.argsort(scores[u, 1:])[::-1][:k]
            assert per_user[u, 2 + 2 * i] == pytest.approx(y[top].sum() / y.sum(), rel=1e-12)
    assert np.allclose(sums, per_user.sum(0), rtol=1e-15)


def test_retrieval_metrics_hand_computed():
    ranks = np.array([[1, 0, 4], [0, 0, 0], [3, 2, 12]])
    per_user, sums = metrics.retrieval_metrics_reference(ranks, (2, 10))
    l2 = math.log2
    want = np.array([
        [1, (1 + 1 / 4) / 2, 1 / 2, 1.0 / (1 + 1 / l2(3)), 1.0, (1 + 1 / l2(5)) / (1 + 1 / l2(3))],
        [0, 0, 0, 0, 0, 0],
        [1, (1 / 3 + 1 / 2 + 1 / 12) / 3, 1 / 3, (1 / l2(3)) / (1 + 1 / l2(3)), 2 / 3, (1 / l2(4) + 1 / l2(3)) / (1 + 1 / l2(3) + 1 / l2(4))],
    ])
    assert np.allclose(per_user, want, rtol=1e-14, atol=0)
    assert np.allclose(sums, want.sum(0), rtol=1e-14) and sums[0] == 2.0
    assert metrics.retrieval_metrics_reference(ranks, ())[1].shape == (2,)


_KS = (C.c_int * 3)(5, 10, 100)


def _desc(**changes):
    f = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, T=4, targets=4096, ld_targets=4, exclude=4096,
             ld_exclude=50, E=50, splits=0, ks=_KS, n_ks=3, out_ranks=4096, out_scores=4096, out_sums=4096, ws=4096)
    f.update(changes)
    d = _lib.RankDesc(**f)
    if "ws_bytes" not in changes:
        d.ws_bytes = _lib.lib().nr_score_rank_workspace_bytes(C.byref(d))
    return d


def test_workspace_is_host_arithmetic_and_far_below_a_score_matrix():
    lib = _lib.lib()
    size = lambda **c: lib.nr_score_rank_workspace_bytes(C.byref(_desc(**c)))
    b = size()
    assert 0 < b < 8192 * 100001 * 4 // 64
    assert size(U=64) < 8192 * 100001 * 4 // 64                           # few users: more slices, still no [U, V]
    assert size(U=16384, splits=2) > size(U=8192, splits=2) > size(U=4096, splits=2)      # grows with U
    assert size(T=64, ld_targets=64) > size(T=8, ld_targets=8) > b                        # with T
    assert size(splits=8) > size(splits=4) > size(splits=1)                               # with splits
    assert size(splits=8) - size(splits=4) == 8192 * 4 * 4 * 4            # one int32 counter per user, slice and target
    assert size(splits=4, n_ks=0, ks=None) < size(splits=4)               # the per-user metric terms
    assert size(T=0) == 0 and size(n_ks=9) == 0 and lib.nr_score_rank_workspace_bytes(None) == 0


REFUSED = {
    "T_0": (dict(T=0), "T = 0"),
    "T_65": (dict(T=65, ld_targets=65), "T = 65"),
    "E_65": (dict(E=65, ld_exclude=65), "E = 65"),
    "n_ks_9": (dict(n_ks=9), "n_ks = 9"),
    "k_0_in_ks": (dict(ks=(C.c_int * 3)(5, 0, 100)), "k = 0"),
    "V_1": (dict(V=1), "V = 1"),
    "N_not_multiple_of_4": (dict(N=402), "multiple of 4"),
    "N_1028": (dict(N=1028, ld_news=1028, ld_user=1028), "N = 1028"),
    "unaligned_rows": (dict(ld_news=401), "16-byte aligned"),
    "null_out_ranks": (dict(out_ranks=None), "null pointer"),
    "null_targets": (dict(targets=None), "null pointer"),
    "undersized_workspace": (dict(ws_bytes=1024), "nr_score_rank_workspace_bytes"),
    "no_workspace": (dict(ws=None), "nr_score_rank_workspace_bytes"),
    "too_many_splits": (dict(splits=257), "splits = 257"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_before_any_launch(case):
    change, message = REFUSED[case]
    rc = _lib.lib().nr_score_rank(C.byref(_desc(**change)), None)
    assert rc == 1 and message in _lib.last_error(), _lib.last_error()


def test_null_descriptor_is_refused():
    assert _lib.lib().nr_score_rank(None, None) == 1 and "null descriptor" in _lib.last_error()


def test_abi_size_of_the_descriptor_is_reported():
    sizes = (C.c_size_t * 9)()
    assert _lib.lib().nr_abi_sizes(sizes, 9) == 0 and sizes[8] == C.sizeof(_lib.RankDesc)
    assert _lib.NR_RANK_MAX_TARGETS == 64 and _lib.NR_RANK_MAX_KS == 8


def test_score_rank_has_no_cpu_fallback():
    import torch
    from newsrecommendation_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_rank(torch.zeros(10, 8), torch.zeros(3, 8), torch.ones(3, 2, dtype=torch.int32))


def test_rank_eval_and_rank_shard_are_exported():
    from newsrecommendation_amd import train
    assert callable(train.rank_eval) and callable(train.rank_shard)
    assert "64" in train.rank_eval.__doc__ and "share" in train.rank_eval.__doc__


def test_shard_targets_are_the_clicked_candidates_per_impression():
    from newsrecommendation_amd import train

    class Shard:
        hist = np.zeros((4, 3), np.int32)
        cand = np.array([5, 6, 7, 8, 9, 10, 11, 12, 13], np.int32)
        label = np.array([0, 1, 0, 1, 1, 0, 0, 1, 1], np.int32)
        offsets = np.array([0, 3, 5, 6, 9], np.int32)

        def __len__(self):
            return 4

    assert np.array_equal(train._shard_targets(Shard()), np.array([[6, 0], [8, 9], [0, 0], [12, 13]], np.int32))


def test_retrieval_sums_of_the_row_split_match_the_reference():
    """The tensor arithmetic train.rank_eval uses for users with more than 64 targets."""
    import torch
    from newsrecommendation_amd import train
    g = np.random.default_rng(10)
    ranks = g.integers(0, 200, (7, 70)).astype(np.int32)
    ranks[3] = 0
    ranks[4, 1:] = 0
    ks = (1, 5, 10, 100)
    got = train._retrieval_sums(torch.from_numpy(ranks), ks).numpy()
    assert np.allclose(got, metrics.retrieval_metrics_reference(ranks, ks)[1], rtol=1e-12, atol=0)


def test_row_split_of_rank_eval_against_the_reference(monkeypatch):
    """train.rank_eval with 70 target columns: the layout over several 64-wide rows and the way back, with the device call
    replaced by the host reference (the split is tensor arithmetic around it)."""
    import torch
    from newsrecommendation_amd import train
    g = np.random.default_rng(12)
    V, U, T = 200, 5, 70
    news, user = g.integers(-2, 3, (V, 8)).astype(np.float32), g.integers(-2, 3, (U, 8)).astype(np.float32)
    targets = np.zeros((U, T), np.int32)
    targets[0] = g.permutation(np.arange(1, V))[:T]                      # 70 targets: two rows
    targets[1, ::2] = g.permutation(np.arange(1, V))[:35]                # zeros between entries: one row
    targets[2, :68] = g.permutation(np.arange(1, V))[:68]
    targets[2, 68], targets[2, 69] = targets[2, 3], V + 4                # a repeat across the 64-column boundary, an id >= V
    targets[4, 5] = 17
    hist = g.integers(1, V, (U, 3)).astype(np.int32)
    hist[1, 0] = targets[1, 0]                                           # a clicked target
    mask = np.ones((U, 3), np.float32)
    widths = []

    def fake_score_rank(news_vecs, user_vecs, tg, exclude=None, ks=(), splits=0):
        assert tg.shape[1] <= 64 and ks is None
        widths.append(tuple(tg.shape))
        r, s = metrics.rank_reference(news_vecs.numpy(), user_vecs.numpy(), targets=tg.numpy(), exclude=None if exclude is None else exclude.numpy())
        return torch.from_numpy(r), torch.from_numpy(s).float(), None

    monkeypatch.setattr(train.ops, "score_rank", fake_score_rank)
    monkeypatch.setattr(train, "_user_vectors", lambda *a: torch.from_numpy(user))
    ks = (1, 10, 100)
    for exclude_history in (True, False):
        ranks, scores, sums = train.rank_eval(None, torch.from_numpy(news), hist, mask, targets, ks=ks, exclude_history=exclude_history)
        want_r, want_s = metrics.rank_reference(news, user, targets=targets, exclude=hist if exclude_history else None)
        assert np.array_equal(ranks.numpy(), want_r) and np.array_equal(scores.numpy().astype(np.float64), want_s)
        assert np.allclose(sums.numpy(), metrics.retrieval_metrics_reference(want_r, ks)[1], rtol=1e-12, atol=0)
        assert (ranks[1, 0] == 0) == exclude_history and ranks[2, 68] == 0 and ranks[2, 69] == 0 and ranks[3].sum() == 0
    assert widths == [(7, 64), (7, 64)]                                  # users 0 and 2 take two rows each, the others one

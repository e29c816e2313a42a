"""CPU: the host side of the diversified re-ranking (include/nrhip.h, K11) -- metrics.mmr_reference on a hand-worked table, the
refusals nr_mmr_select makes before it launches anything (fake non-null pointers: a launch would fault, a refusal does not),
the descriptor's place in nr_abi_sizes, and the new names of the Python layers."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")

# id:               0 (padding)  1       2       3       4       5 (all zero)
NEWS = np.array([[9.0, 9.0], [1, 0], [1, 0], [0, 1], [1, 1], [0, 0]])
GROUP = np.array([0, 0, 0, 1, 0, -1])
POOL_IDS = np.array([[1, 2, 3, 4, 5, 0]])
POOL_SCORES = np.array([[5.0, 4.0, 3.0, 3.0, 1.0, -INF]])          # the last place is score_topk's fill: not live
R2 = 2.0 ** 0.5


def test_hand_worked_reorder_and_fill():
    """penalty 2.  Step 1 takes place 0 (5).  Step 2: news 2 is a copy of news 1, 4 - 2 * 1 = 2; news 3 is orthogonal, 3 - 0 = 3;
    news 4, 3 - 2 / sqrt 2 = 1.59; the zero vector has similarity 0 to everything, 1 - 0 = 1: news 3 wins by 1.  Step 3: news 2
    still 2, news 4 still 1.59 (cosine 1 / sqrt 2 to both taken), news 5 1: news 2 by 0.41.  Then news 4 (1.59 against 1), then
    the zero vector; the fill place is never taken, so the sixth entry is the fill."""
    ids, sc, pl, mg = metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=6, penalty=2.0)
    assert ids.tolist() == [[1, 3, 2, 4, 5, 0]] and pl.tolist() == [[0, 2, 1, 3, 4, -1]]
    assert sc.tolist() == [[5.0, 3.0, 4.0, 3.0, 1.0, -INF]]                      # the relevance, not the MMR value
    assert np.allclose(mg[0, :4], [1.0, 1.0, R2 - 1.0, 2.0 - R2], rtol=1e-15, atol=1e-15) and mg[0, 4] == INF and mg[0, 5] == INF
    assert ids.dtype == np.int32 and pl.dtype == np.int32 and sc.dtype == np.float64 and mg.dtype == np.float64
    # the walk is greedy: a smaller k is a prefix
    ids3, sc3, pl3, mg3 = metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=3, penalty=2.0)
    assert ids3.tolist() == [[1, 3, 2]] and np.array_equal(mg3, mg[:, :3])


def test_hand_worked_penalty_zero_is_the_prefix_and_ties_go_to_the_lowest_place():
    ids, sc, pl, mg = metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=5, penalty=0.0)
    assert ids.tolist() == [[1, 2, 3, 4, 5]] and pl.tolist() == [[0, 1, 2, 3, 4]] and sc.tolist() == [[5.0, 4.0, 3.0, 3.0, 1.0]]
    assert mg[0, 2] == 0.0                                                       # places 2 and 3 tie at 3: the lower place first
    # a tie made by the penalty: with penalty 1, after place 0 news 2 has 4 - 1 = 3 and news 3 has 3 - 0 = 3: place 1 wins the tie
    ids, _, pl, mg = metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=3, penalty=1.0)
    assert pl.tolist() == [[0, 1, 2]] and mg[0, 1] == 0.0
    # the same tie with the two places swapped in the pool: still the lower PLACE, now the other news
    swapped_ids, swapped_sc = POOL_IDS[:, [0, 2, 1, 3, 4, 5]], POOL_SCORES[:, [0, 2, 1, 3, 4, 5]]
    ids, _, pl, _ = metrics.mmr_reference(NEWS, swapped_ids, swapped_sc, k=3, penalty=1.0)
    assert pl.tolist() == [[0, 1, 2]] and ids.tolist() == [[1, 3, 2]]
    # one penalty per user
    two = metrics.mmr_reference(NEWS, np.tile(POOL_IDS, (2, 1)), np.tile(POOL_SCORES, (2, 1)), k=4, penalty=np.array([0.0, 2.0]))
    assert two[0].tolist() == [[1, 2, 3, 4], [1, 3, 2, 4]]


def test_hand_worked_cap_and_not_live_places():
    """Cap 2 on group 0 = {1, 2, 4}, news 3 in group 1, news 5 in no group: after 1, 3, 2 group 0 is full, news 4 is no candidate
    any more and the row ends with the ungrouped zero vector and the fill."""
    ids, sc, pl, mg = metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=5, penalty=2.0, group=GROUP, group_cap=2)
    assert ids.tolist() == [[1, 3, 2, 5, 0]] and pl.tolist() == [[0, 2, 1, 4, -1]] and sc[0, 4] == -INF and mg[0, 3] == INF
    ids, _, pl, _ = metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=5, penalty=0.0, group=GROUP, group_cap=1)
    assert ids.tolist() == [[1, 3, 5, 0, 0]] and pl.tolist() == [[0, 2, 4, -1, -1]]
    # not live: an id outside [1, V), the padding news, a NaN score -- never taken, never used as an index; a repeat is two places
    ids, sc, pl, _ = metrics.mmr_reference(NEWS, np.array([[7, 3, 0, -4, 3, 1]]), np.array([[9.0, 2.0, 8.0, 7.0, 2.0, NAN]]), k=4, penalty=0.5)
    assert ids.tolist() == [[3, 3, 0, 0]] and pl.tolist() == [[1, 4, -1, -1]] and sc.tolist() == [[2.0, 2.0, -INF, -INF]]
    with pytest.raises(ValueError, match="come together"):
        metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=2, penalty=1.0, group=GROUP)
    with pytest.raises(ValueError, match="group_cap"):
        metrics.mmr_reference(NEWS, POOL_IDS, POOL_SCORES, k=2, penalty=1.0, group=GROUP, group_cap=0)


BASE = dict(news_vecs=4096, ld_news=400, V=100001, pool_ids=4096, pool_scores=4096, ld_pool_ids=128, ld_pool_scores=128, U=8192, N=400, M=128, k=10,
            penalty=1.0, out_ids=4096, out_scores=4096, out_place=4096)
REFUSED = [(dict(news_vecs=None), "null pointer"), (dict(pool_ids=None), "null pointer"), (dict(pool_scores=None), "null pointer"),
           (dict(out_ids=None), "null pointer"), (dict(out_scores=None), "null pointer"), (dict(out_place=None), "null pointer"),
           (dict(M=0), "M = 0"), (dict(M=129, ld_pool_ids=129, ld_pool_scores=129), "M = 129"), (dict(k=0), "k = 0"), (dict(k=129), "k = 129"),
           (dict(M=64, k=65), "k = 65"), (dict(N=0), "N = 0"), (dict(N=402, ld_news=404), "N = 402"), (dict(N=1028, ld_news=1028), "N = 1028"),
           (dict(ld_news=396), "ld_news = 396"), (dict(ld_news=402), "ld_news = 402"), (dict(news_vecs=4100), "16-byte aligned"),
           (dict(ld_pool_ids=127), "pool row strides"), (dict(ld_pool_scores=64), "pool row strides"),
           (dict(penalty=-0.5), "penalty"), (dict(penalty=INF), "penalty"), (dict(penalty=NAN), "penalty"),
           (dict(group=4096), "group_cap = 0"), (dict(group=4096, group_cap=129), "group_cap = 129"), (dict(group_cap=3), "without group"),
           (dict(U=-1), "U = -1"), (dict(V=0), "V = 0")]


@pytest.mark.parametrize("change,message", REFUSED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(REFUSED)])
def test_refused_before_any_launch(change, message):
    d = _lib.MmrDesc(**{**BASE, **change})
    assert _lib.lib().nr_mmr_select(C.byref(d), None) == 1 and message in _lib.last_error(), _lib.last_error()


def test_null_descriptor_and_empty_batch():
    lib = _lib.lib()
    assert lib.nr_mmr_select(None, None) == 1 and "null descriptor" in _lib.last_error()
    # U == 0: fine, and nothing is launched (the fake pointers are never touched); the other checks still hold for it
    assert lib.nr_mmr_select(C.byref(_lib.MmrDesc(**{**BASE, "U": 0})), None) == 0
    assert lib.nr_mmr_select(C.byref(_lib.MmrDesc(**{**BASE, "U": 0, "k": 0})), None) == 1


def test_descriptor_is_entry_9_of_abi_sizes():
    sizes = (C.c_size_t * 10)()
    assert _lib.lib().nr_abi_sizes(sizes, 10) == 0 and sizes[9] == C.sizeof(_lib.MmrDesc)
    assert sizes[7] == C.sizeof(_lib.TopkDesc) and sizes[8] == C.sizeof(_lib.RankDesc)
    nine = (C.c_size_t * 10)()
    assert _lib.lib().nr_abi_sizes(nine, 9) == 0 and nine[9] == 0 and list(nine)[:9] == list(sizes)[:9]


def test_new_names_and_signatures():
    assert "nr_mmr_select" in _lib.SIGNATURES and hasattr(_lib.lib(), "nr_mmr_select")
    assert list(inspect.signature(ops.mmr_select).parameters) == ["news_vecs", "pool_ids", "pool_scores", "k", "penalty", "group", "group_cap"]
    assert list(inspect.signature(train.recommend_diverse).parameters) == [
        "model", "news_vecs", "hist_idx", "mask", "k", "penalty", "pool", "exclude_history", "batch_size", "prior", "news_time", "window",
        "news_group", "group_cap", "seen"]
    assert inspect.signature(train.recommend_diverse).parameters["pool"].default == 128
    # recommend keeps its argument list
    assert list(inspect.signature(train.recommend).parameters) == [
        "model", "news_vecs", "hist_idx", "mask", "k", "exclude_history", "batch_size", "prior", "news_time", "window", "news_group", "group_cap",
        "seen"]
    kinds = inspect.signature(metrics.mmr_reference).parameters
    assert list(kinds) == ["news", "pool_ids", "pool_scores", "k", "penalty", "group", "group_cap"]
    assert all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("k", "penalty", "group", "group_cap"))


def test_mmr_select_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mmr_select(torch.zeros(10, 8), torch.ones(3, 4, dtype=torch.int32), torch.zeros(3, 4), 2, 1.0)

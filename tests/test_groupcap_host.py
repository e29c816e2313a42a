"""CPU: the host side of group caps in full-corpus top-k ("at most c news of one group in the row", include/nrhip.h K9) --
metrics.topk_reference(..., group=, group_cap=) against a literal walk on hand-written score matrices, a numpy model of the
device algorithm (per-slice streaming with the one-exchange rule over ascending ids, then the merge walk over the union of
the slices' rows) against that reference on random small cases, the refusals nr_score_topk makes before it launches anything
(fake non-null pointers, as in test_topk_host.py), and the descriptor's size."""
import ctypes as C
import math

import numpy as np
import pytest

from newsrecommendation_amd import _lib, metrics

INF = float("inf")


def _walk(scores, k, group, cap, banned=()):
    """The contract, literally: sort one user's eligible news by (score descending, id ascending), walk, skip a news whose
    group already has `cap` taken, stop after k."""
    rows = sorted((-float(s), v) for v, s in enumerate(scores) if v >= 1 and v not in banned and not math.isnan(s))
    ids, out, taken = [], [], {}
    for neg, v in rows:
        if len(ids) == k:
            break
        g = int(group[v])
        if g >= 0:
            if taken.get(g, 0) >= cap:
                continue
            taken[g] = taken.get(g, 0) + 1
        ids.append(v)
        out.append(-neg)
    return ids + [0] * (k - len(ids)), out + [-INF] * (k - len(out))


def test_reference_on_handwritten_rows():
    #  id:       0    1    2    3    4    5    6    7    8    9
    scores = np.array([[9.0, 5.0, 5.0, 5.0, 4.0, 4.0, 3.0, 2.0, 1.0, 0.0],
                       [9.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]])
    group = np.array([0, 0, 0, 0, 1, 0, -1, -7, 1, 1])
    # user 0, cap 1: ids 1, 2, 3 tie in group 0 -> only the smallest id; 4 (group 1); 5 is group 0 again; 6 and 7 are ungrouped
    ids, sc = metrics.topk_reference(scores, k=4, group=group, group_cap=1)
    assert ids[0].tolist() == [1, 4, 6, 7] and sc[0].tolist() == [5.0, 4.0, 3.0, 2.0]
    # user 1 walks from the other end: 9 (g 1), 8 and 4 are group 1 too, 7 and 6 ungrouped, 5 (g 0)
    assert ids[1].tolist() == [9, 7, 6, 5] and sc[1].tolist() == [8.0, 6.0, 5.0, 4.0]
    ids, sc = metrics.topk_reference(scores, k=6, group=group, group_cap=2)
    assert ids[0].tolist() == [1, 2, 4, 6, 7, 8] and ids[1].tolist() == [9, 8, 7, 6, 5, 3]
    # G * c < k with no ungrouped news: the fill
    two = np.array([0, 0, 1, 0, 1, 0, 1, 0, 1, 0])
    ids, sc = metrics.topk_reference(scores, k=6, group=two, group_cap=2)
    assert ids[0].tolist() == [1, 2, 3, 4, 0, 0] and np.isneginf(sc[0, 4:]).all() and sc[0, :4].tolist() == [5.0, 5.0, 5.0, 4.0]
    assert ids[1].tolist() == [9, 8, 7, 6, 0, 0]
    # cap >= k and an all-negative group are the plain rows
    plain = metrics.topk_reference(scores, k=6)
    for kw in (dict(group=group, group_cap=6), dict(group=np.full(10, -1), group_cap=1)):
        got = metrics.topk_reference(scores, k=6, **kw)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])


def test_reference_ineligible_news_use_up_no_cap():
    scores = np.array([[0.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0]])
    group = np.array([0, 0, 0, 0, 0, 1, 1, 1])
    # without anything: group 0 gives 1, group 1 gives 5
    assert metrics.topk_reference(scores, k=3, group=group, group_cap=1)[0][0].tolist() == [1, 5, 0]
    # 1 excluded: 2 takes group 0's place
    assert metrics.topk_reference(scores, k=3, group=group, group_cap=1, exclude=[[1, 0]])[0][0].tolist() == [2, 5, 0]
    nan = scores.copy()
    nan[0, 1] = np.nan
    assert metrics.topk_reference(nan, k=3, group=group, group_cap=1)[0][0].tolist() == [2, 5, 0]
    prior = np.zeros(8)
    prior[[1, 2]] = -INF
    assert metrics.topk_reference(scores, k=3, group=group, group_cap=1, prior=prior)[0][0].tolist() == [3, 5, 0]
    stamp = np.array([0, 1, 1, 1, 5, 1, 5, 5])
    assert metrics.topk_reference(scores, k=3, group=group, group_cap=1, stamp=stamp, window=[[4, 6]])[0][0].tolist() == [4, 6, 0]
    with pytest.raises(ValueError):
        metrics.topk_reference(scores, k=3, group=group)
    with pytest.raises(ValueError):
        metrics.topk_reference(scores, k=3, group_cap=2)
    with pytest.raises(ValueError):
        metrics.topk_reference(scores, k=3, group=group, group_cap=0)


def test_reference_matches_the_literal_walk_on_tied_integer_scores():
    g = np.random.default_rng(17)
    scores = g.integers(-3, 4, (12, 60)).astype(np.float64)
    scores[:, 11] = np.nan
    group = g.integers(-1, 5, 60)
    exclude = g.integers(0, 60, (12, 5))
    for k in (1, 7, 40):
        for cap in (1, 3):
            ids, sc = metrics.topk_reference(scores, k=k, exclude=exclude, group=group, group_cap=cap)
            for u in range(12):
                want = _walk(scores[u], k, group, cap, banned=set(exclude[u].tolist()))
                assert ids[u].tolist() == want[0] and sc[u].tolist() == want[1], (k, cap, u)


# ---- the device algorithm in numpy: keys are (score, -id) tuples, larger = better ------------------------------------------

def _stream_slice(keys_by_id, ids, k, group, cap):
    """One slice: candidates arrive by ascending id; the list is updated by ONE exchange per candidate (rule 1), behind the
    kernel's fast filter (score strictly above the score of the overall worst kept key once the list is full)."""
    kept = []                                                        # (key, group)
    for v in ids:
        key = keys_by_id[v]
        if key is None:                                              # not eligible: never reaches the list
            continue
        full = len(kept) == k
        worst = min(kept)[0] if kept else None
        if full and not key[0] > worst[0]:                           # the fast test: a strict > on the SCORE only
            continue
        g = int(group[v])
        mine = [e for e in kept if e[1] == g] if g >= 0 else []
        if g >= 0 and len(mine) >= cap:
            low = min(mine)
            if key > low[0]:
                kept.remove(low)
                kept.append((key, g))
        elif not full:
            kept.append((key, g))
        else:
            assert key > worst                                       # it passed the filter
            kept.remove(min(kept))
            kept.append((key, g))
    return [e[0] for e in kept]


def _merge(keys, k, group, cap):
    """The merge: sort the union descending, walk it with the cap, the first k taken."""
    row, taken = [], {}
    for key in sorted(keys, reverse=True):
        if len(row) == k:
            break
        g = int(group[-key[1]])
        if g >= 0:
            if taken.get(g, 0) >= cap:
                continue
            taken[g] = taken.get(g, 0) + 1
        row.append(key)
    return row


def test_streaming_exchange_and_slice_merge_model_equals_the_definition():
    rng = np.random.default_rng(23)
    n_short = 0
    for case in range(400):
        V = int(rng.integers(2, 70))
        k = int(rng.integers(1, 13))
        cap = int(rng.integers(1, 5))
        n_groups = int(rng.integers(1, 7))
        group = rng.integers(-1 if case % 3 else 0, n_groups, V)
        scores = rng.integers(-3, 4, V).astype(np.float64)           # few values: ties everywhere
        scores[rng.random(V) < 0.05] = np.nan
        banned = set(rng.integers(0, V, 3).tolist())
        keys = [None] * V
        for v in range(1, V):
            if v not in banned and not math.isnan(scores[v]):
                keys[v] = (float(scores[v]), -v)
        cuts = sorted(set([1, V] + rng.integers(1, V + 1, int(rng.integers(0, 5))).tolist()))
        union = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            union += _stream_slice(keys, range(lo, hi), k, group, cap)
        row = _merge(union, k, group, cap)
        ref_ids, ref_sc = metrics.topk_reference(scores[None, :], k=k, exclude=[sorted(banned)], group=group, group_cap=cap)
        got_ids = [-key[1] for key in row] + [0] * (k - len(row))
        got_sc = [key[0] for key in row] + [-INF] * (k - len(row))
        assert got_ids == ref_ids[0].tolist() and got_sc == ref_sc[0].tolist(), (case, V, k, cap, cuts)
        n_short += len(row) < k
    assert 20 < n_short < 380                                        # short rows and full rows both occur


# ---- the library, without a device -------------------------------------------------------------------------------------------

def _desc(**changes):
    f = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, k=10, exclude=4096, ld_exclude=50, E=50, splits=0,
             out_ids=4096, out_scores=4096, ws=4096, group=4096, group_cap=2)
    f.update(changes)
    d = _lib.TopkDesc(**f)
    d.ws_bytes = 1 << 30
    return d


REFUSED = {
    "group_without_cap": (dict(group_cap=0), "group given with group_cap = 0"),
    "cap_129": (dict(group_cap=129), "group_cap = 129"),
    "cap_negative": (dict(group_cap=-1), "group_cap = -1"),
    "cap_without_group": (dict(group=None, group_cap=2), "group_cap = 2 given without group"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_before_any_launch(case):
    change, message = REFUSED[case]
    d = _desc(**change)
    assert _lib.lib().nr_score_topk_workspace_bytes(C.byref(d)) == 0
    rc = _lib.lib().nr_score_topk(C.byref(d), None)
    assert rc == 1 and message in _lib.last_error(), _lib.last_error()


def test_workspace_does_not_depend_on_the_caps():
    lib = _lib.lib()
    plain = lib.nr_score_topk_workspace_bytes(C.byref(_desc(group=None, group_cap=0)))
    assert plain > 0
    for cap in (1, 2, 128):
        assert lib.nr_score_topk_workspace_bytes(C.byref(_desc(group_cap=cap))) == plain


def test_descriptor_size_matches_the_library():
    sizes = (C.c_size_t * 8)()
    assert _lib.lib().nr_abi_sizes(sizes, 8) == 0
    assert sizes[7] == C.sizeof(_lib.TopkDesc)
    names = [f[0] for f in _lib.TopkDesc._fields_]
    assert names[names.index("splits") + 1:names.index("out_ids")] == ["group", "group_cap"]      # as include/nrhip.h declares them
    assert _lib.TopkDesc.group.offset + 8 == _lib.TopkDesc.group_cap.offset and _lib.TopkDesc.group_cap.offset + 8 == _lib.TopkDesc.out_ids.offset


def test_python_layers_carry_the_arguments():
    import inspect
    from newsrecommendation_amd import ops, train
    for fn, names in ((ops.score_topk, ("group", "group_cap")), (train.recommend, ("news_group", "group_cap"))):
        p = inspect.signature(fn).parameters
        assert all(n in p and p[n].default is None for n in names)
    for fn in (ops.score_rank, train.rank_eval, train.rank_shard):      # the rank side keeps describing the uncapped ranking
        assert not any("group" in n for n in inspect.signature(fn).parameters)

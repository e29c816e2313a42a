"""CPU: the host side of full-corpus top-k recommendation -- metrics.topk_reference against a brute-force restatement of the
contract, nr_score_topk_workspace_bytes as host arithmetic, and the checks nr_score_topk makes before it launches anything
(fake non-null pointers: a launch would fault, a refusal does not)."""
import ctypes as C
import math

import numpy as np
import pytest

from newsrecommendation_amd import _lib, metrics


def _brute(scores, k, exclude):
    """The contract spelled out with Python's sort: eligible = ids 1 .. V-1, not excluded, score not NaN; order = score
    descending, then id ascending; the row is filled with (0, -inf)."""
    U, V = scores.shape
    ids, out = np.zeros((U, k), np.int32), np.full((U, k), -np.inf)
    for u in range(U):
        banned = set(int(e) for e in exclude[u]) if exclude is not None else set()
        rows = [(-float(scores[u, v]), v) for v in range(1, V) if v not in banned and not math.isnan(scores[u, v])]
        for j, (neg, v) in enumerate(sorted(rows)[:k]):
            ids[u, j], out[u, j] = v, -neg
    return ids, out


@pytest.mark.parametrize("k", [1, 5, 40])
def test_reference_matches_brute_force_on_tied_integer_scores(k):
    g = np.random.default_rng(7)
    news = g.integers(-2, 3, (30, 8)).astype(np.float64)
    user = g.integers(-2, 3, (9, 8)).astype(np.float64)
    scores = user @ news.T
    assert len(np.unique(scores)) < scores.size // 4                     # many ties
    exclude = g.integers(1, 30, (9, 6))
    exclude[:, 1] = 0                                                    # no entry
    exclude[:, 2] = exclude[:, 0]                                        # a duplicate
    exclude[:, 3] = 30 + g.integers(0, 5, 9)                             # out of range
    exclude[:, 4] = -3
    for ex in (None, exclude):
        want = _brute(scores, k, ex)
        got = metrics.topk_reference(scores, k=k, exclude=ex)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got_v = metrics.topk_reference(news, user, k=k, exclude=ex)      # the same from the vectors
        assert np.array_equal(got_v[0], want[0]) and np.array_equal(got_v[1], want[1])
    if k == 40:                                                          # k larger than the 29 eligible news: the fill
        ids, sc = metrics.topk_reference(scores, k=k)
        assert (ids[:, :29] > 0).all() and (ids[:, 29:] == 0).all() and np.isneginf(sc[:, 29:]).all()


def test_reference_never_returns_a_nan_news_and_keeps_the_others():
    g = np.random.default_rng(8)
    scores = g.integers(-3, 4, (5, 20)).astype(np.float64)
    with_nan = scores.copy()
    with_nan[:, 7] = np.nan
    ids, sc = metrics.topk_reference(with_nan, k=19)
    assert not (ids == 7).any() and not np.isnan(sc).any()
    want = _brute(scores, 19, np.full((5, 1), 7))                        # the same as excluding that news
    assert np.array_equal(ids, want[0]) and np.array_equal(sc, want[1])
    assert (ids[:, 18] == 0).all()


def _desc(**changes):
    f = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, k=10, exclude=4096, ld_exclude=50, E=50, splits=0,
             out_ids=4096, out_scores=4096, ws=4096)
    f.update(changes)
    d = _lib.TopkDesc(**f)
    if "ws_bytes" not in changes:
        d.ws_bytes = _lib.lib().nr_score_topk_workspace_bytes(C.byref(d))
    return d


def test_workspace_is_host_arithmetic_and_far_below_a_score_matrix():
    lib = _lib.lib()
    size = lambda **c: lib.nr_score_topk_workspace_bytes(C.byref(_desc(**c)))
    b = size()
    assert 0 < b < 8192 * 100001 * 4 // 64
    # grows with U and with k.  From 128 to 256 user tiles the library halves the slices (2 -> 1: one workgroup per CU either
    # way), so that one doubling of U keeps U * splits; it never shrinks, and it grows again from there
    sizes = [size(U=u) for u in (64, 512, 4096, 8192, 16384, 32768, 65536)]
    assert sizes == sorted(sizes) and size(U=16384) >= b and size(U=32768) > b and size(U=65536) > size(U=32768)
    assert size(U=16384, splits=2) == 2 * b and size(k=20) == 2 * b
    assert size(splits=4) == 8192 * 4 * 10 * 8                            # O(U * splits * k)
    assert size(U=64) < 8192 * 100001 * 4 // 64                           # few users: more slices, still no [U, V]
    assert size(k=0) == 0 and lib.nr_score_topk_workspace_bytes(None) == 0


REFUSED = {
    "k_0": (dict(k=0), "k = 0"),
    "k_129": (dict(k=129), "k = 129"),
    "V_1": (dict(V=1), "V = 1"),
    "N_not_multiple_of_4": (dict(N=402), "multiple of 4"),
    "N_1028": (dict(N=1028, ld_news=1028, ld_user=1028), "N = 1028"),
    "E_65": (dict(E=65, ld_exclude=65), "E = 65"),
    "null_out_ids": (dict(out_ids=None), "null pointer"),
    "null_out_scores": (dict(out_scores=None), "null pointer"),
    "undersized_workspace": (dict(ws_bytes=1024), "nr_score_topk_workspace_bytes"),
    "no_workspace": (dict(ws=None), "nr_score_topk_workspace_bytes"),
    "too_many_splits_for_k": (dict(k=128, splits=65), "splits = 65"),
    "unaligned_rows": (dict(ld_news=401), "16-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_before_any_launch(case):
    change, message = REFUSED[case]
    rc = _lib.lib().nr_score_topk(C.byref(_desc(**change)), None)
    assert rc == 1 and message in _lib.last_error(), _lib.last_error()


def test_null_descriptor_is_refused():
    assert _lib.lib().nr_score_topk(None, None) == 1 and "null descriptor" in _lib.last_error()


def test_score_topk_has_no_cpu_fallback():
    import torch
    from newsrecommendation_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_topk(torch.zeros(10, 8), torch.zeros(3, 8), 2)


def test_recommend_is_exported():
    from newsrecommendation_amd import train
    assert callable(train.recommend) and "64" in train.recommend.__doc__

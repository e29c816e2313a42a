"""Exclusion lists of any length (CSR; include/nrhip.h K9 / K10) -- what needs no GPU: the refusals of both calls before any
launch (fake non-null pointers: a launch would fault, a refusal does not), sizes and layout of the descriptors,
ops.ExclusionLists on CPU tensors against a model made of Python sets, a numpy model of the device's wave-wide lower-bound
search (csr_lower_bound of csrc/nr_topk.hip, statement for statement) against np.searchsorted, and the signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, ops, train

FAKE = 4096


def _topk(**changes):
    f = dict(news_vecs=FAKE, ld_news=400, V=100001, user=FAKE, ld_user=400, U=8192, N=400, k=10, splits=0, out_ids=FAKE, out_scores=FAKE, ws=FAKE)
    f.update(changes)
    d = _lib.TopkDesc(**f)
    if "ws_bytes" not in changes:
        d.ws_bytes = _lib.lib().nr_score_topk_workspace_bytes(C.byref(d))
    return d


def _rank(**changes):
    f = dict(news_vecs=FAKE, ld_news=400, V=100001, user=FAKE, ld_user=400, U=8192, N=400, T=4, targets=FAKE, ld_targets=4, splits=0,
             out_ranks=FAKE, out_scores=FAKE, ws=FAKE)
    f.update(changes)
    d = _lib.RankDesc(**f)
    if "ws_bytes" not in changes:
        d.ws_bytes = _lib.lib().nr_score_rank_workspace_bytes(C.byref(d))
    return d


REFUSED = {
    "dense_and_csr_together": (dict(exclude=FAKE, ld_exclude=50, E=50, excl_offsets=FAKE, excl_ids=FAKE, n_excl=100), "one list form per call"),
    "dense_and_empty_csr_together": (dict(exclude=FAKE, ld_exclude=50, E=50, excl_offsets=FAKE), "one list form per call"),
    "offsets_without_ids": (dict(excl_offsets=FAKE, n_excl=100), "excl_offsets given without excl_ids"),
    "ids_without_offsets": (dict(excl_ids=FAKE, n_excl=100), "excl_ids given without excl_offsets"),
    "negative_n_excl": (dict(excl_offsets=FAKE, excl_ids=FAKE, n_excl=-1), "n_excl = -1"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_before_any_launch(case):
    change, message = REFUSED[case]
    lib = _lib.lib()
    rc = lib.nr_score_topk(C.byref(_topk(**change)), None)
    assert rc == 1 and message in _lib.last_error() and "score_topk" in _lib.last_error(), _lib.last_error()
    rc = lib.nr_score_rank(C.byref(_rank(**change)), None)
    assert rc == 1 and message in _lib.last_error() and "score_rank" in _lib.last_error(), _lib.last_error()
    # the size queries refuse the same descriptors
    assert lib.nr_score_topk_workspace_bytes(C.byref(_topk(ws_bytes=0, **change))) == 0
    assert lib.nr_score_rank_workspace_bytes(C.byref(_rank(ws_bytes=0, **change))) == 0


def test_workspace_sizes_do_not_depend_on_the_lists():
    lib = _lib.lib()
    csr = dict(excl_offsets=FAKE, excl_ids=FAKE, n_excl=5_000_000)
    for more in (dict(), dict(U=64), dict(U=65, V=4099, splits=3)):
        assert lib.nr_score_topk_workspace_bytes(C.byref(_topk(**more))) == lib.nr_score_topk_workspace_bytes(C.byref(_topk(**more, **csr))) > 0
        assert lib.nr_score_rank_workspace_bytes(C.byref(_rank(**more))) == lib.nr_score_rank_workspace_bytes(C.byref(_rank(**more, **csr))) > 0
    # offsets with n_excl == 0 (every list empty) is a valid descriptor, with or without ids
    assert lib.nr_score_topk_workspace_bytes(C.byref(_topk(excl_offsets=FAKE))) > 0
    assert lib.nr_score_rank_workspace_bytes(C.byref(_rank(excl_offsets=FAKE, excl_ids=FAKE))) > 0


def test_layout_three_fields_between_E_and_splits():
    sizes = (C.c_size_t * 9)()
    assert _lib.lib().nr_abi_sizes(sizes, 9) == 0
    assert sizes[7] == C.sizeof(_lib.TopkDesc) and sizes[8] == C.sizeof(_lib.RankDesc)
    for Desc in (_lib.TopkDesc, _lib.RankDesc):
        names = [f[0] for f in Desc._fields_]
        i = names.index("E")
        assert names[i + 1:i + 5] == ["excl_offsets", "excl_ids", "n_excl", "splits"]
        # n_excl and splits share one 8-byte slot: the fields behind them stay where an 8-byte `splits` slot put them
        assert getattr(Desc, "excl_offsets").offset == getattr(Desc, "E").offset + 4
        assert getattr(Desc, "splits").offset == getattr(Desc, "n_excl").offset + 4 and getattr(Desc, "n_excl").offset % 8 == 0
        assert getattr(Desc, names[i + 5]).offset == getattr(Desc, "n_excl").offset + 8


# ---- ops.ExclusionLists on the CPU against Python sets ----

def _as_sets(lists):
    off, ids = lists.offsets.tolist(), lists.ids.tolist()
    assert lists.offsets.dtype == torch.int32 and lists.ids.dtype == torch.int32 and off[0] == 0 and off[-1] == len(ids)
    rows = [ids[off[u]:off[u + 1]] for u in range(lists.U)]
    for r in rows:
        assert all(x >= 1 for x in r) and all(a < b for a, b in zip(r, r[1:])), r          # canonical: strictly ascending, ids >= 1
    return [set(r) for r in rows]


def _model(rows):
    return [{int(x) for x in r if int(x) >= 1} for r in rows]


def _messy_rows(U, V, seed, longest=300):
    """duplicates, zeros, negatives, ids >= V, empty users, unsorted"""
    g = np.random.default_rng(seed)
    rows = []
    for u in range(U):
        n = 0 if u % 5 == 0 else int(g.integers(1, longest))
        r = g.integers(-3, V + 50, n)
        rows.append(np.concatenate([r, r[: n // 3]]).astype(np.int64))                      # a third of it twice
    return rows


def test_exclusion_lists_from_sequences_and_tensors():
    V, U = 1000, 23
    rows = _messy_rows(U, V, seed=1)
    assert any(len(r) == 0 for r in rows) and any((r >= V).any() for r in rows if len(r)) and any((r <= 0).any() for r in rows if len(r))
    for form in (rows, [torch.as_tensor(r) for r in rows], [r.tolist() for r in rows]):
        lists = ops.ExclusionLists(form)
        assert lists.U == len(lists) == U and _as_sets(lists) == _model(rows)
    g = torch.Generator().manual_seed(2)
    wide = torch.randint(-2, V + 10, (U, 200), generator=g, dtype=torch.int32)              # [U, 200]: wider than the dense list
    wide[3] = 0
    wide[4, :150] = 7
    lists = ops.ExclusionLists(wide)
    assert _as_sets(lists) == _model(wide.tolist()) and _as_sets(lists)[3] == set() and 7 in _as_sets(lists)[4]
    assert _as_sets(ops.ExclusionLists(wide.long())) == _model(wide.tolist())
    empty = ops.ExclusionLists(torch.zeros(U, 0, dtype=torch.int32))
    assert empty.U == U and empty.ids.numel() == 0 and empty.offsets.tolist() == [0] * (U + 1)
    assert ops.ExclusionLists([]).U == 0
    with pytest.raises(RuntimeError, match="integer"):
        ops.ExclusionLists(torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="int32"):
        ops.ExclusionLists([[1, 1 << 31]])


def test_exclusion_lists_take_and_merged():
    V, U = 500, 17
    a_rows, b_rows = _messy_rows(U, V, seed=3), _messy_rows(U, V, seed=4, longest=40)[::-1]
    a, b = ops.ExclusionLists(a_rows), ops.ExclusionLists(b_rows)
    pick = [5, 5, 0, 16, 3, 5, 1, 0]                                                          # repeated, reordered
    taken = a.take(torch.tensor(pick))
    assert taken.U == len(pick) and _as_sets(taken) == [_model(a_rows)[i] for i in pick]
    assert _as_sets(a.take([])) == [] and _as_sets(a.take(np.arange(U))) == _model(a_rows)
    union = [x | y for x, y in zip(_model(a_rows), _model(b_rows))]
    assert _as_sets(a.merged(b)) == union == _as_sets(b.merged(a))
    assert _as_sets(a.merged(b_rows)) == union                                               # anything the constructor takes
    assert _as_sets(a.merged(ops.ExclusionLists([[]] * U))) == _model(a_rows)
    with pytest.raises(RuntimeError, match="users"):
        a.merged(ops.ExclusionLists([[1]]))
    raw = ops.ExclusionLists.from_sorted([0, 2, 2], [-1, 9])                                  # trusted as it is
    assert raw.U == 2 and raw.ids.tolist() == [-1, 9] and raw.offsets.dtype == torch.int32
    assert a.to("cpu") is a


# ---- the device's lower-bound search as a numpy model ----

ROWS, PROBES = 128, 64       # TK_ROWS: one load = two entries per lane; one probe per lane


def _model_lower_bound(ids, lo, hi, vc, trace=None):
    """csr_lower_bound of csrc/nr_topk.hip, statement for statement; lanes = the 64 entries of `lane`."""
    lane = np.arange(PROBES, dtype=np.int64)
    first_lo, first_hi = lo, hi
    while hi - lo > ROWS:
        n = hi - lo
        probe = lo + n * (lane + 1) // 65
        assert (probe >= first_lo).all() and (probe < first_hi).all() and (np.diff(probe) > 0).all()
        c = int(np.count_nonzero(ids[probe] < vc))
        last_below, first_not = lo + n * c // 65, lo + n * (c + 1) // 65
        if c < 64:
            hi = first_not
        if c > 0:
            lo = last_below + 1
        assert first_lo <= lo <= hi <= first_hi and hi - lo <= n // 65 + 1
        if trace is not None:
            trace.append(hi - lo)
    n = hi - lo
    b0, b1 = np.zeros(PROBES, dtype=bool), np.zeros(PROBES, dtype=bool)
    in0, in1 = lane < n, lane + 64 < n                        # a lane outside the range loads nothing
    assert (lo + lane[in0] < first_hi).all() and (lo + lane[in1] + 64 < first_hi).all()
    b0[in0] = ids[lo + lane[in0]] < vc
    b1[in1] = ids[lo + lane[in1] + 64] < vc
    return lo + int(np.count_nonzero(b0)) + int(np.count_nonzero(b1))


@pytest.mark.parametrize("L", list(range(0, 131)) + [4095, 4096, 4097, 70000])
def test_lower_bound_model_matches_searchsorted(L):
    g = np.random.default_rng(L)
    span = 3 * L + 400
    seg = np.sort(g.choice(np.arange(100, 100 + span), L, replace=False)).astype(np.int32)      # strictly ascending
    before, after = np.array([7, 50], dtype=np.int32), np.array([2_000_000_000], dtype=np.int32)
    ids = np.concatenate([before, seg, after])                                                   # the segment inside a longer array
    lo, hi = len(before), len(before) + L
    starts = {1, 99, 100, 101, 100 + span, 100 + span + 1, 100 + span + 129}                      # before and past the segment
    if L:
        starts |= {int(seg[0]), int(seg[-1]), int(seg[-1]) + 1, int(seg[L // 2]), int(seg[L // 2]) + 1, int(seg[L // 3]) - 1}
        starts |= {int(x) for x in g.integers(100, 100 + span, 40)}
        starts |= {int(seg[i]) + d for i in (0, L // 65, L // 2, L - 1) for d in (-1, 0, 1)}
    for vc in sorted(s for s in starts if s >= 1):
        trace = []
        got = _model_lower_bound(ids, lo, hi, vc, trace)
        assert got == lo + int(np.searchsorted(seg, vc, side="left")), (L, vc)
        assert len(trace) <= (0 if L <= ROWS else 1 if L < (ROWS - 1) * 65 else 2)                   # probe rounds: a round leaves <= n // 65 + 1


def test_lower_bound_model_stays_in_bounds_on_a_broken_promise():
    """An unsorted segment gives an unspecified answer, but every index read lies inside the segment (asserted by the model)."""
    g = np.random.default_rng(9)
    for L in (129, 1000, 70000):
        ids = g.integers(-5, 5000, L + 10).astype(np.int32)
        for vc in (1, 129, 2561, 4993):
            got = _model_lower_bound(ids, 5, 5 + L, vc)
            assert 5 <= got <= 5 + L


# ---- signatures ----

def test_signatures():
    for fn in (train.recommend, train.rank_eval, train.rank_shard):
        p = inspect.signature(fn).parameters
        assert "seen" in p and p["seen"].default is None
    assert list(inspect.signature(ops.score_topk).parameters) == ["news_vecs", "user_vecs", "k", "exclude", "splits", "prior", "stamp", "window",
                                                                  "group", "group_cap"]
    assert list(inspect.signature(ops.score_rank).parameters) == ["news_vecs", "user_vecs", "targets", "exclude", "ks", "splits", "prior", "stamp",
                                                                  "window"]
    assert "64" in train.recommend.__doc__ and "64" in train.rank_eval.__doc__
    assert "LAST 64" not in train.recommend.__doc__ and "LAST 64" not in train.rank_eval.__doc__

"""CPU: the host side of the propensities under group caps (include/nrhip.h, K15 / K16) -- metrics.logz_groups_reference and
metrics.capped_row_logprob_reference on a hand-computed case and on the enumeration of a 5-news corpus, the law of the capped
host sampler (metrics.sample_reference) against them, the layout ops.GroupOrder builds, lists mapped to positions, the two
descriptors' places in nr_abi_sizes, the workspace size, and the refusals made before any launch (fake pointers: nothing runs)."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

from logz_groups_helpers import (BASE_GROUPS, CHI2_PAIRS_MAX, ENUM_GROUP, ENUM_X, LAW_CAP, LAW_GROUP, LAW_K, V_BASE, base_group, enum_rows,
                                 law_pair_probabilities, law_pairs, law_pairs_chi2, law_violations, three_bins)
from newsrecommendation_amd import _lib, metrics, ops, train
from sample_helpers import LAW_SEED, LAW_TAU, LAW_U, law_scores

INF, NAN = float("inf"), float("nan")


def test_both_references_on_a_hand_computed_case():
    x = np.array([[0.0, 1.0, 0.5, -0.5, 2.0]])                         # news 1, 2 in group 0, news 3 in group 1, news 4 in none
    group = [-1, 0, 0, 1, -1]
    w = np.exp(x[0])
    ls, gm, cnt = metrics.logz_groups_reference(x, temperature=1.0, group=group)
    assert cnt.tolist() == [[2, 1, 1]] and gm.tolist() == [[1.0, -0.5, 2.0]]
    assert np.allclose(ls, [[math.log(1 + math.exp(-0.5)), 0.0, 0.0]], rtol=1e-15, atol=0)
    # n_groups = 3: an empty bin; an excluded news; a bad temperature leaves max and count and spares the empty bins
    ls, gm, cnt = metrics.logz_groups_reference(x, temperature=1.0, group=group, n_groups=3, exclude=[[4]])
    assert cnt.tolist() == [[2, 1, 0, 0]] and gm[0, 2] == -INF and ls[0, 2] == -INF and ls[0, 3] == -INF
    ls, gm, cnt = metrics.logz_groups_reference(x, temperature=0.0, group=group, n_groups=3, exclude=[[4]])
    assert cnt.tolist() == [[2, 1, 0, 0]] and np.isnan(ls[0, :2]).all() and (ls[0, 2:] == -INF).all() and gm[0, 0] == 1.0
    with pytest.raises(ValueError, match="n_groups"):
        metrics.logz_groups_reference(x, temperature=1.0, group=group, n_groups=1)
    # the row (1, 4, 3) under c = 1: taking news 1 closes group 0, so news 2 -- in the bases -- is out from step 1 on
    row = [[1, 4, 3]]
    bases = metrics.logz_groups_reference(x, temperature=1.0, group=group, exclude=row)
    assert bases[2].tolist() == [[1, 0, 0]]
    lp, tot = metrics.capped_row_logprob_reference(x, row_ids=row, temperature=1.0, bases=bases[:2], group=group, group_cap=1)
    want = [math.log(w[1] / w[1:].sum()), math.log(w[4] / (w[3] + w[4])), 0.0]
    assert np.allclose(lp[0], want, rtol=1e-14, atol=1e-15) and abs(tot[0] - sum(want)) < 1e-14
    # c = 2 never closes anything here: plain Plackett-Luce, as row_logprob_reference on the joined base has it
    lp2, _ = metrics.capped_row_logprob_reference(x, row_ids=row, temperature=1.0, bases=bases[:2], group=group, group_cap=2)
    plain = metrics.logz_reference(x, temperature=1.0, exclude=row)
    lp3, _ = metrics.row_logprob_reference(x, row_ids=row, temperature=1.0, base=plain[:2], sequential=True)
    assert np.allclose(lp2, lp3, rtol=1e-14, atol=1e-15)
    # (1, 2, 0, 3, 9): news 2 is capped out -- -inf, but its weight counts at step 0, when group 0 was open; fill gives 0
    row = [[1, 2, 0, 3, 9]]
    bases = metrics.logz_groups_reference(x, temperature=1.0, group=group, exclude=row)
    lp, tot = metrics.capped_row_logprob_reference(x, row_ids=row, temperature=1.0, bases=bases[:2], group=group, group_cap=1)
    assert lp[0, 1] == -INF and lp[0, 2] == 0.0 and lp[0, 4] == 0.0 and tot[0] == -INF
    assert np.allclose(lp[0, [0, 3]], [math.log(w[1] / w[1:].sum()), math.log(w[3] / (w[3] + w[4]))], rtol=1e-14)
    # a NaN score is in no sum and uses up nothing of a cap: (2 with a NaN score, 1) takes news 1 as the first of its group
    y = x.copy()
    y[0, 2] = NAN
    row = [[2, 1]]
    bases = metrics.logz_groups_reference(y, temperature=1.0, group=group, exclude=row)
    lp, tot = metrics.capped_row_logprob_reference(y, row_ids=row, temperature=1.0, bases=bases[:2], group=group, group_cap=1)
    assert np.isnan(lp[0, 0]) and np.isnan(tot[0]) and abs(lp[0, 1] - math.log(w[1] / (w[1] + w[3] + w[4]))) < 1e-14
    lp, _ = metrics.capped_row_logprob_reference(x, row_ids=[[1, 0]], temperature=NAN, bases=bases[:2], group=group, group_cap=1)
    assert np.isnan(lp[0, 0]) and lp[0, 1] == 0.0
    with pytest.raises(ValueError, match="group_cap"):
        metrics.capped_row_logprob_reference(x, row_ids=row, temperature=1.0, bases=bases[:2], group=group, group_cap=129)


@pytest.mark.parametrize("tau", [0.7, 0.05])
def test_enumeration_through_the_references_sums_to_one(tau):
    rows, forbidden = enum_rows()
    scores = np.tile(ENUM_X, (len(rows), 1))
    bases = metrics.logz_groups_reference(scores, temperature=tau, group=ENUM_GROUP, exclude=rows)
    lp, tot = metrics.capped_row_logprob_reference(scores, row_ids=rows, temperature=tau, bases=bases[:2], group=ENUM_GROUP, group_cap=1)
    assert len(rows) == 60 and forbidden.sum() == 36 and np.all(tot[forbidden] == -INF) and np.all(np.isfinite(tot[~forbidden]))
    assert np.all(lp[~forbidden] <= 0.0) and abs(np.exp(tot[~forbidden]).sum() - 1.0) <= 1e-13


def test_the_capped_host_sampler_follows_the_law():
    """4096 identical users through metrics.sample_reference under the cap: no row breaks it, and the first two places follow the
    pair probabilities -- those of the closed form and those of the two references, which agree."""
    ids, _, _ = metrics.sample_reference(law_scores(), k=LAW_K, temperature=LAW_TAU, seed=LAW_SEED, group=LAW_GROUP, group_cap=LAW_CAP)
    assert ids.shape == (LAW_U, LAW_K) and (ids > 0).all() and law_violations(ids) == 0
    pairs, p = law_pairs(), law_pair_probabilities()
    assert len(pairs) == 50 and abs(p.sum() - 1.0) < 1e-13
    scores = np.tile(law_scores()[0], (50, 1))
    bases = metrics.logz_groups_reference(scores, temperature=LAW_TAU, group=LAW_GROUP, exclude=pairs)
    _, tot = metrics.capped_row_logprob_reference(scores, row_ids=pairs, temperature=LAW_TAU, bases=bases[:2], group=LAW_GROUP, group_cap=LAW_CAP)
    assert np.allclose(np.exp(tot), p, rtol=1e-12, atol=0)
    chi2 = law_pairs_chi2(ids, np.exp(tot))
    print(f"chi-square of the first two places over the 50 pairs: {chi2:.2f} (limit {CHI2_PAIRS_MAX})")
    assert abs(chi2 - 50.02) < 0.005 and chi2 <= CHI2_PAIRS_MAX


def _layout(go, group):
    """The statements of ops.GroupOrder's docstring, checked one by one against `group`."""
    g = group.numpy().astype(np.int64)
    V, G = len(g), go.n_groups
    bins = np.where(g < 0, G, g)
    order, pos = go.order.numpy(), go.pos.numpy()
    bin_start, seg_start, bin_seg = go.bin_start.numpy(), go.seg_start.numpy(), go.bin_seg.numpy()
    assert go.n_pos == len(order) == bin_start[-1] and go.n_pos % 128 == 0 and len(bin_start) == G + 2 == len(bin_seg)
    S = go.chunks_per_segment
    assert S == max(1, math.ceil(go.n_pos // 128 / 256))
    for b in range(G + 1):
        want = np.flatnonzero(bins[1:] == b) + 1                          # ascending ids
        run = order[bin_start[b]:bin_start[b + 1]]
        assert len(run) == math.ceil(len(want) / 128) * 128 and np.array_equal(run[:len(want)], want) and np.all(run[len(want):] == 0)
        segs = seg_start[bin_seg[b]:bin_seg[b + 1] + 1]
        if len(run) == 0:
            assert bin_seg[b] == bin_seg[b + 1]
            continue
        assert segs[0] == bin_start[b] and segs[-1] == bin_start[b + 1] and np.all(np.diff(segs) > 0)
        assert np.all(np.diff(segs)[:-1] == S * 128) and np.diff(segs)[-1] <= S * 128 and len(segs) - 1 == math.ceil(len(run) / (S * 128))
    assert go.nseg == bin_seg[-1] == len(seg_start) - 1 <= 256 + G + 1 and seg_start[0] == 0 and seg_start[-1] == go.n_pos
    assert pos[0] == -1 and np.array_equal(order[pos[1:]], np.arange(1, V)) and (np.sort(pos[1:]) == np.flatnonzero(order)).all()
    return bin_start, seg_start


def test_group_order_layout():
    group = base_group()
    go = ops.GroupOrder(group)
    bin_start, seg_start = _layout(go, group)
    assert go.n_groups == BASE_GROUPS and go.V == V_BASE and go.chunks_per_segment == 1
    assert bin_start.tolist() == [0, 128, 384, 384, 512, 896, 1280, 1408] and go.nseg == 11          # the empty bin owns nothing
    assert seg_start.tolist() == list(range(0, 1409, 128))
    # a wider n_groups appends empty bins; everything is a function of group alone
    wide = ops.GroupOrder(group, n_groups=9)
    assert wide.n_pos == go.n_pos and wide.nseg == 11 and wide.bin_start.tolist()[:6] == bin_start.tolist()[:6]
    _layout(wide, group)
    again = ops.GroupOrder(group.clone())
    assert all(torch.equal(getattr(go, n), getattr(again, n)) for n in ("order", "pos", "bin_start", "seg_start", "bin_seg"))
    # V = 33 000 in three bins: 259 or 260 padded chunks, more than 256: two chunks a segment, the last segment of a bin may hold one
    big = three_bins(33000)
    gb = ops.GroupOrder(big)
    _layout(gb, big)
    assert gb.n_pos // 128 > 256 and gb.chunks_per_segment == 2 and gb.nseg <= 132 and gb.n_groups == 2
    # every news in no group: one bin, the plain order padded
    none = ops.GroupOrder(torch.full((300,), -1, dtype=torch.int32))
    assert none.n_groups == 1 and none.n_pos == 384 and none.order[:299].tolist() == list(range(1, 300)) and none.bin_seg.tolist() == [0, 0, 3]
    for bad, n in ((group, 5), (group, 0), (group, 513)):
        with pytest.raises(ValueError, match="n_groups"):
            ops.GroupOrder(bad, n_groups=n)
    with pytest.raises(RuntimeError, match="int32"):
        ops.GroupOrder(group.to(torch.int64))


def test_lists_mapped_to_positions_stay_sorted_and_unique():
    group = base_group()
    go = ops.GroupOrder(group)
    g = torch.Generator().manual_seed(19)
    raw = [torch.randperm(V_BASE - 1, generator=g)[:int(n)] + 1 for n in torch.randint(0, 500, (9,), generator=g)]
    raw[2] = torch.arange(1, V_BASE)
    raw[3] = torch.tensor([5, 5, V_BASE, V_BASE + 7, 1])                  # a repeat and ids past the corpus: dropped
    lists = ops.ExclusionLists(raw)
    mapped = go.positions(lists)
    assert mapped.U == 9 and mapped.offsets.dtype == torch.int32 and mapped.ids.dtype == torch.int32
    off, pos = mapped.offsets.numpy(), go.pos.numpy()
    for u in range(9):
        seg = mapped.ids.numpy()[off[u]:off[u + 1]]
        ids = np.unique(raw[u].numpy())
        ids = ids[ids < V_BASE]
        assert np.all(np.diff(seg) > 0) and np.array_equal(seg, np.sort(pos[ids]))
    assert off[3] - off[2] == V_BASE - 1 and off[4] - off[3] == 2


def test_descriptors_are_entries_13_and_14_of_abi_sizes_and_the_new_names_exist():
    sizes = (C.c_size_t * 15)()
    assert _lib.lib().nr_abi_sizes(sizes, 15) == 0
    assert sizes[13] == C.sizeof(_lib.LogzGroupsDesc) and sizes[14] == C.sizeof(_lib.LogprobCappedDesc) and sizes[12] == C.sizeof(_lib.LogprobDesc)
    thirteen = (C.c_size_t * 15)()
    thirteen[13] = thirteen[14] = 12345
    assert _lib.lib().nr_abi_sizes(thirteen, 13) == 0 and thirteen[13] == 12345 and thirteen[14] == 12345 and list(thirteen)[:13] == list(sizes)[:13]
    tail = ["ws", "ws_bytes", "prior", "stamp", "window", "ld_window"]
    assert [f[0] for f in _lib.LogzGroupsDesc._fields_][-6:] == tail
    for name in ("nr_score_logz_groups_workspace_bytes", "nr_score_logz_groups", "nr_row_logprob_capped"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert list(inspect.signature(ops.score_logz_groups).parameters) == ["news_vecs", "user_vecs", "temperature", "groups", "exclude", "splits",
                                                                         "prior", "stamp", "window"]
    assert list(inspect.signature(ops.row_logprob_capped).parameters) == ["news_vecs", "user_vecs", "row_ids", "temperature", "bases", "group",
                                                                          "group_cap", "n_groups", "prior", "stamp", "window"]
    assert list(inspect.signature(train.sample_propensity_capped).parameters) == [
        "model", "news_vecs", "hist_idx", "mask", "ids", "temperature", "news_group", "group_cap", "exclude_history", "batch_size", "prior",
        "news_time", "window", "seen", "groups"]
    assert list(inspect.signature(train.log_partition_groups).parameters)[:6] == ["model", "news_vecs", "hist_idx", "mask", "temperature", "news_group"]
    for fn in (metrics.logz_groups_reference, metrics.capped_row_logprob_reference):
        kinds = inspect.signature(fn).parameters
        assert list(kinds)[:2] == ["a", "b"] and all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(kinds)[2:])


# V = 100 001 in 18 groups: 782 chunks of real news and up to 19 tails -- say 800 chunks, S = 4, 219 segments
LOGZG = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, tau=0.5, order=4096, n_pos=800 * 128, seg_start=4096,
             nseg=219, bin_seg=4096, n_groups=18, out_logsum=4096, out_max=4096, out_count=4096)
LOGZG_REFUSED = [(dict(tau=0.0), "tau"), (dict(tau=NAN), "tau"), (dict(N=402), "N = 402"), (dict(V=1), "V = 1"), (dict(U=0), "U = 0"),
                 (dict(n_groups=0), "n_groups = 0, must be in [1, 512]"), (dict(n_groups=513), "n_groups = 513, must be in [1, 512]"),
                 (dict(n_pos=0), "n_pos = 0"), (dict(n_pos=1000), "n_pos = 1000"), (dict(nseg=0), "nseg = 0"),
                 (dict(nseg=276), "nseg = 276 segments, must be in [1, 275]"), (dict(n_pos=128 * 100), "at most the 100 chunks"),
                 (dict(splits=-1), "splits = -1"), (dict(splits=220), "splits = 220"), (dict(stamp=4096), "stamp given without window"),
                 (dict(n_excl=-1), "n_excl = -1"), (dict(excl_ids=4096, n_excl=5), "excl_ids given without excl_offsets")]


@pytest.mark.parametrize("change,message", LOGZG_REFUSED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(LOGZG_REFUSED)])
def test_score_logz_groups_refuses_before_any_launch(change, message):
    d = _lib.LogzGroupsDesc(**{**LOGZG, **change})
    lib = _lib.lib()
    assert lib.nr_score_logz_groups_workspace_bytes(C.byref(d)) == 0 and message in _lib.last_error(), _lib.last_error()
    assert lib.nr_score_logz_groups(C.byref(d), None) == 1 and message in _lib.last_error(), _lib.last_error()


def test_score_logz_groups_workspace_is_users_times_segments_and_is_checked():
    lib = _lib.lib()
    for U, nseg in ((1, 1), (37, 11), (5, 131), (8192, 219)):
        for splits in (0, 1, nseg):
            got = lib.nr_score_logz_groups_workspace_bytes(C.byref(_lib.LogzGroupsDesc(**{**LOGZG, "U": U, "nseg": nseg, "splits": splits})))
            assert got == (U * nseg * 12 + 7) // 8 * 8, (U, nseg, splits)
    assert lib.nr_score_logz_groups_workspace_bytes(None) == 0 and "null descriptor" in _lib.last_error()
    need = (8192 * 219 * 12 + 7) // 8 * 8
    for ws in (dict(ws=4096, ws_bytes=need - 8), dict(ws=None, ws_bytes=need), dict(ws=4100, ws_bytes=need)):
        assert lib.nr_score_logz_groups(C.byref(_lib.LogzGroupsDesc(**{**LOGZG, **ws})), None) == 1
        assert "nr_score_logz_groups_workspace_bytes" in _lib.last_error()
    for missing in ("order", "seg_start", "bin_seg", "out_count"):
        assert lib.nr_score_logz_groups(C.byref(_lib.LogzGroupsDesc(**{**LOGZG, missing: None, "ws": 4096, "ws_bytes": need})), None) == 1
        assert "null pointer" in _lib.last_error()
    assert lib.nr_score_logz_groups(C.byref(_lib.LogzGroupsDesc(**{**LOGZG, "ld_news": 396, "ws": 4096, "ws_bytes": need})), None) == 1
    assert "16-byte aligned" in _lib.last_error()


LOGPC = dict(news_vecs=4096, ld_news=400, V=100001, user=4096, ld_user=400, U=8192, N=400, k=10, row_ids=4096, ld_ids=10, group=4096, group_cap=2,
             n_groups=18, tau=0.5, base_max=4096, base_logsum=4096, ld_base=19, out_logp=4096)
LOGPC_REFUSED = [(dict(tau=0.0), "tau"), (dict(tau=INF), "tau"), (dict(k=0), "k = 0"), (dict(k=129), "k = 129 entries per row, must be in [1, 128]"),
                 (dict(group_cap=0), "group_cap = 0, must be in [1, 128]"), (dict(group_cap=129), "group_cap = 129, must be in [1, 128]"),
                 (dict(n_groups=0), "n_groups = 0, must be in [1, 512]"), (dict(n_groups=513, ld_base=514), "n_groups = 513, must be in [1, 512]"),
                 (dict(N=402), "N = 402"), (dict(V=1), "V = 1"), (dict(U=0), "U = 0"), (dict(stamp=4096), "stamp given without window"),
                 (dict(ld_ids=9), "stride 9"), (dict(ld_base=18), "base row stride 18 < n_groups + 1 = 19"), (dict(group=None), "null pointer"),
                 (dict(base_logsum=None), "null pointer"), (dict(user=4104), "16-byte aligned")]


@pytest.mark.parametrize("change,message", LOGPC_REFUSED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(LOGPC_REFUSED)])
def test_row_logprob_capped_refuses_before_any_launch(change, message):
    d = _lib.LogprobCappedDesc(**{**LOGPC, **change})
    assert _lib.lib().nr_row_logprob_capped(C.byref(d), None) == 1 and message in _lib.last_error(), _lib.last_error()
    assert _lib.lib().nr_row_logprob_capped(None, None) == 1 and "null descriptor" in _lib.last_error()


def test_the_python_layer_refuses_wrong_shapes_and_cpu_tensors():
    news, user = torch.zeros(10, 8), torch.zeros(3, 8)
    group = torch.tensor([-1, 0, 0, 1, 1, 2, -1, 0, 1, 2], dtype=torch.int32)
    go = ops.GroupOrder(group)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_logz_groups(news, user, 0.5, go)
    with pytest.raises(RuntimeError, match=r"the GroupOrder was built for V = 12 news on cpu, the call has V = 10"):
        ops.score_logz_groups(news, user, 0.5, ops.GroupOrder(torch.zeros(12, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="groups must be an ops.GroupOrder"):
        ops.score_logz_groups(news, user, 0.5, group)
    rows = torch.ones(3, 2, dtype=torch.int32)
    bases = (torch.zeros(3, 4), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.row_logprob_capped(news, user, rows, 0.5, bases, group, 1)
    for bad in ((torch.zeros(3), torch.zeros(3)), (torch.zeros(3, 4), torch.zeros(3, 5)), (torch.zeros(2, 4), torch.zeros(2, 4))):
        with pytest.raises(RuntimeError, match=r"must be a floating point tensor of shape \(3, n_groups \+ 1 = "):
            ops.row_logprob_capped(news, user, rows, 0.5, bad, group, 1)
    with pytest.raises(RuntimeError, match=r"n_groups \+ 1 = 6"):
        ops.row_logprob_capped(news, user, rows, 0.5, bases, group, 1, n_groups=5)
    with pytest.raises(RuntimeError, match="row_ids must be an integer tensor"):
        ops.row_logprob_capped(news, user, rows[:2], 0.5, bases, group, 1)
    with pytest.raises(RuntimeError, match="group must be an int32 tensor"):
        ops.row_logprob_capped(news, user, rows, 0.5, bases, group.to(torch.int64), 1)
    # sample_propensity keeps its refusal; the capped function is the one that takes the two arguments
    with pytest.raises(ValueError, match="group caps"):
        train.sample_propensity(None, None, None, None, None, 0.5, news_group=np.zeros(4), group_cap=1)

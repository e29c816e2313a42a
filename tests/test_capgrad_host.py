"""CPU: the host side of listwise training under group caps (include/nrhip.h, K20 / K21) -- the two float64 references against
central differences of metrics.capped_row_logprob_reference's own total, the identity sum omega = sum c, the collapse onto K19 /
K17 when no cap binds, a mutant per formula, the descriptors' places in nr_abi_sizes, the new names, and the refusals made before
any launch (fake non-null pointers: a launch would fault, a refusal does not), with the whole text of nr_last_error."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")
V, N, G, CAP, K = 60, 8, 3, 2, 9
TAU = 0.7


def _corpus(seed=5):
    """V = 60 news in 3 groups plus no-group, one user, a row of k = 9 that closes groups 0 and 1 (cap 2), holds ONE blocked entry
    (a third news of group 0 after the group is full), a fill entry, and signed g."""
    rng = np.random.default_rng(seed)
    news, user = rng.standard_normal((V, N)), rng.standard_normal((1, N)) / 2
    group = np.array([v % 4 if v % 4 < G else -1 for v in range(V)], dtype=np.int64)      # ids 3, 7, .. are in no group
    lists = [np.array([5, 6, 17, 40])]
    #        g0  g1  g0  ng  g1  g0(blocked) fill g2  ng
    row = np.array([[4, 9, 12, 3, 13, 20, 0, 2, 11]], dtype=np.int64)
    assert [group[i] for i in row[0]] == [0, 1, 0, -1, 1, 0, 0, 2, -1]
    g = np.array([[1.0, -0.6, 0.8, 0.3, -1.2, 55.0, 77.0, 0.9, -0.4]])               # the g of the blocked and the fill entry is not read
    return news, user, group, lists, row, g


def _loss(news, user, group, lists, row, g, cap):
    """sum_j g_j nll_j over the live steps, from capped_row_logprob_reference on bases recomputed for THIS user vector."""
    merged = [np.concatenate([lists[0], row[0][row[0] >= 1]])]
    bases = metrics.logz_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, exclude=merged)
    logp, _ = metrics.capped_row_logprob_reference(news, user, row_ids=row, temperature=TAU, bases=bases[:2], group=group, group_cap=cap,
                                                   n_groups=G)
    step = np.isfinite(logp[0]) & (row[0] >= 1)
    return float(np.sum(np.where(step, -g[0] * logp[0], 0.0))), bases, logp


def _closed_form(news, user, group, lists, row, g, cap, mutant=None):
    merged = [np.concatenate([lists[0], row[0][row[0] >= 1]])]
    bases = metrics.logz_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, exclude=merged)
    om, c = metrics._capped_grad_rows(news, user, row, TAU, bases[:2], group, cap, G, g, None, None, None, mutant=mutant)
    e, mass = metrics.expect_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, bin_w=om, exclude=merged)
    grad = e[0].copy()
    for i, v in enumerate(row[0]):
        if 1 <= v < V:
            grad -= c[0, i] * news[v]
    return grad / TAU, om, c, mass


def _central(news, user, group, lists, row, g, cap, h=1e-5):
    fd = np.zeros(N)
    for ci in range(N):
        up, dn = user.copy(), user.copy()
        up[0, ci] += h
        dn[0, ci] -= h
        fd[ci] = (_loss(news, up, group, lists, row, g, cap)[0] - _loss(news, dn, group, lists, row, g, cap)[0]) / (2 * h)
    return fd


def test_references_against_central_differences_and_the_sum_identity():
    news, user, group, lists, row, g = _corpus()
    _, bases, logp = _loss(news, user, group, lists, row, g, CAP)
    assert np.isneginf(logp[0, 5]) and logp[0, 6] == 0.0 and np.isfinite(np.delete(logp[0], 5)).all()    # one blocked entry, one fill
    grad, om, c, mass = _closed_form(news, user, group, lists, row, g, CAP)
    fd = _central(news, user, group, lists, row, g, CAP)
    scale = max(np.abs(om).max(), np.abs(c).max())
    worst = float(np.abs(grad - fd).max())
    print(f"worst |closed form - central difference| = {worst:.3e}, largest coefficient {scale:.3e}")
    assert worst <= 1e-6 * scale
    # sum_b omega_b = sum_i c_i, and the mass of the exact bases is sum omega over the non-empty bins
    assert abs(om.sum() - c.sum()) <= 1e-12 * np.abs(c).sum()
    assert abs(mass[0] - om.sum()) <= 1e-12 * np.abs(om).sum()
    # the special entries: fill has c = 0; the blocked one is no step but is pulled by the steps at which its group was open
    assert c[0, 6] == 0.0 and c[0, 5] != 0.0 and om.shape == (1, G + 1) and (om != 0).all()
    g2 = g.copy()
    g2[0, 5], g2[0, 6] = NAN, INF
    _, om2, c2, _ = _closed_form(news, user, group, lists, row, g2, CAP)
    assert np.array_equal(om2, om) and np.array_equal(c2, c)
    # g = None is g = 1
    o1, c1 = metrics.capped_row_logprob_grad_reference(news, user, row_ids=row, temperature=TAU, bases=bases[:2], group=group, group_cap=CAP,
                                                       n_groups=G)
    o2, c2 = metrics.capped_row_logprob_grad_reference(news, user, row_ids=row, temperature=TAU, bases=bases[:2], group=group, group_cap=CAP,
                                                       n_groups=G, g=np.ones((1, K)))
    assert np.array_equal(o1, o2) and np.array_equal(c1, c2)


@pytest.mark.parametrize("mutant", ["q_after_close", "blocked_zero", "closed_full_q"])
def test_each_mutant_formula_fails_the_finite_difference_check(mutant):
    news, user, group, lists, row, g = _corpus()
    grad, om, c, _ = _closed_form(news, user, group, lists, row, g, CAP)
    bad, om_m, c_m, _ = _closed_form(news, user, group, lists, row, g, CAP, mutant=mutant)
    fd = _central(news, user, group, lists, row, g, CAP)
    scale = max(np.abs(om).max(), np.abs(c).max())
    assert np.abs(grad - fd).max() <= 1e-6 * scale < np.abs(bad - fd).max(), mutant


def test_caps_that_never_bind_collapse_onto_the_uncapped_row():
    news, user, group, lists, row, g = _corpus()
    merged = [np.concatenate([lists[0], row[0][row[0] >= 1]])]
    bases = metrics.logz_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, exclude=merged)
    om, c = metrics.capped_row_logprob_grad_reference(news, user, row_ids=row, temperature=TAU, bases=bases[:2], group=group, group_cap=K,
                                                      n_groups=G, g=g)
    base = metrics.logz_reference(news, user, temperature=TAU, exclude=merged)
    a, c19 = metrics.row_logprob_grad_reference(news, user, row_ids=row, temperature=TAU, base=base[:2], g=g)
    assert abs(om.sum() - a[0]) <= 1e-12 * np.abs(c19).sum() and np.abs(c - c19).max() <= 1e-12 * np.abs(c19).max()
    e, _ = metrics.expect_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, bin_w=om, exclude=merged)
    e17, _ = metrics.expect_reference(news, user, temperature=TAU, exclude=merged)
    assert np.abs(e - a[0] * e17).max() <= 1e-12 * np.abs(c19).sum() * np.abs(news).max()


def test_expect_groups_reference_edge_cases():
    news, user, group, lists, row, g = _corpus()
    bases = metrics.logz_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, exclude=lists)
    om = np.array([[0.5, 0.0, -2.0, 1.5]])
    e, m = metrics.expect_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, bin_w=om, exclude=lists)
    e2, m2 = metrics.expect_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, bases=bases[:2], bin_w=om, exclude=lists)
    assert np.abs(e - e2).max() <= 1e-12 and abs(m[0] - om.sum()) <= 1e-12 and abs(m2[0] - m[0]) <= 1e-12
    # a NaN base in a bin with omega == 0 contributes exactly nothing; in a bin with omega != 0 it gives NaN
    bl = bases[0].copy()
    bl[0, 1] = NAN
    e3, _ = metrics.expect_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, bases=(bl, bases[1]), bin_w=om, exclude=lists)
    assert np.array_equal(e3, e2)
    bl[0, 2] = NAN
    e4, m4 = metrics.expect_groups_reference(news, user, temperature=TAU, group=group, n_groups=G, bases=(bl, bases[1]), bin_w=om, exclude=lists)
    assert np.isnan(e4).all() and np.isnan(m4).all()
    e5, m5 = metrics.expect_groups_reference(news, user, temperature=0.0, group=group, n_groups=G, bin_w=om, exclude=lists)
    assert np.isnan(e5).all() and np.isnan(m5).all()
    # dead users of the row reference: zeros
    for t, b in ((0.0, bases[:2]), (TAU, (bl, bases[1]))):
        o, c = metrics.capped_row_logprob_grad_reference(news, user, row_ids=row, temperature=t, bases=b, group=group, group_cap=CAP, n_groups=G)
        assert not o.any() and not c.any()


def test_descriptors_are_entries_18_and_19_of_abi_sizes_and_the_new_names():
    sizes = (C.c_size_t * 20)()
    assert _lib.lib().nr_abi_sizes(sizes, 20) == 0 and sizes[18] == C.sizeof(_lib.ExpectGroupsDesc)
    assert sizes[19] == C.sizeof(_lib.LogprobCappedGradDesc) and sizes[17] == C.sizeof(_lib.LogprobGradDesc) and all(sizes)
    eighteen = (C.c_size_t * 20)()
    eighteen[18] = eighteen[19] = 12345
    assert _lib.lib().nr_abi_sizes(eighteen, 18) == 0 and list(eighteen)[18:] == [12345, 12345] and list(eighteen)[:18] == list(sizes)[:18]
    for name in ("nr_score_expect_groups_workspace_bytes", "nr_score_expect_groups", "nr_row_logprob_capped_grad"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    # K15's fields in order up to n_groups, the shared tail; K16's fields without the two outputs
    names = [f[0] for f in _lib.ExpectGroupsDesc._fields_]
    k15 = [f[0] for f in _lib.LogzGroupsDesc._fields_]
    assert names[:k15.index("n_groups") + 1] == k15[:k15.index("n_groups") + 1] and names[-6:] == k15[-6:]
    names = [f[0] for f in _lib.LogprobCappedGradDesc._fields_]
    k16 = [f[0] for f in _lib.LogprobCappedDesc._fields_ if f[0] not in ("out_logp", "out_total")]
    assert [n for n in names if n not in ("g", "ld_g", "out_bin_w", "out_sub_w")] == k16
    assert list(inspect.signature(ops.score_expect_groups).parameters) == ["news_vecs", "user_vecs", "temperature", "groups", "bases", "bin_w",
                                                                           "exclude", "splits", "prior", "stamp", "window"]
    assert list(inspect.signature(ops.row_logprob_capped_grad).parameters) == ["news_vecs", "user_vecs", "row_ids", "temperature", "bases", "group",
                                                                               "group_cap", "n_groups", "g", "prior", "stamp", "window"]
    assert list(inspect.signature(ops.plackett_luce_nll_capped).parameters) == ["news_vecs", "user_vecs", "rows", "temperature", "groups", "group",
                                                                                "group_cap", "exclude", "splits", "prior", "stamp", "window"]
    assert list(inspect.signature(train.listwise_loss_capped).parameters) == ["model", "news_table", "hist_idx", "mask", "rows", "temperature",
                                                                              "news_group", "group_cap", "weight", "exclude_history", "batch_size",
                                                                              "prior", "news_time", "window", "seen", "groups"]
    for fn in (metrics.expect_groups_reference, metrics.capped_row_logprob_grad_reference):
        kinds = inspect.signature(fn).parameters
        assert list(kinds)[:2] == ["a", "b"] and all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(kinds)[2:])


P = 4096                                                               # a fake pointer, 16-byte aligned
EG = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, order=P, n_pos=102400, seg_start=P, nseg=275,
          bin_seg=P, n_groups=18, base_max=P, base_logsum=P, bin_w=P, ld_base=19, out=P, ld_out=400, ws=P, ws_bytes=1 << 40)
NULLS = "score_expect_groups: null pointer (news_vecs, user, order, seg_start, bin_seg, base_max, base_logsum, bin_w, out)"
EG_REFUSED = [
    (dict(V=1), "score_expect_groups: V = 1 news rows; row 0 is the padding news, so at least 2 are needed"),
    (dict(U=0), "score_expect_groups: U = 0 users"),
    (dict(N=402), "score_expect_groups: vector width N = 402 must be a multiple of 4 in [4, 1024]"),
    (dict(excl_ids=P, n_excl=3), "score_expect_groups: excl_ids given without excl_offsets (n_excl = 3; the two come together)"),
    (dict(tau=0.0), "score_expect_groups: tau = 0, a scalar temperature must be finite and > 0"),
    (dict(tau=NAN), "score_expect_groups: tau = nan, a scalar temperature must be finite and > 0"),
    (dict(n_groups=0), "score_expect_groups: n_groups = 0, must be in [1, 512]"),
    (dict(n_groups=513, ld_base=514), "score_expect_groups: n_groups = 513, must be in [1, 512]"),
    (dict(n_pos=100), "score_expect_groups: n_pos = 100 positions, must be a positive multiple of 128"),
    (dict(nseg=0), "score_expect_groups: nseg = 0 segments, must be in [1, 275] and at most the 800 chunks"),
    (dict(nseg=276), "score_expect_groups: nseg = 276 segments, must be in [1, 275] and at most the 800 chunks"),
    (dict(splits=-1), "score_expect_groups: splits = -1, must be 0 (library's choice) or in [1, 275], the segments"),
    (dict(splits=276), "score_expect_groups: splits = 276, must be 0 (library's choice) or in [1, 275], the segments"),
    (dict(stamp=P), "score_expect_groups: stamp given without window (the two come together)"),
    (dict(window=P, ld_window=2), "score_expect_groups: window given without stamp (the two come together)"),
    (dict(order=None), NULLS),
    (dict(base_max=None), NULLS),
    (dict(base_logsum=None), NULLS),
    (dict(bin_w=None), NULLS),
    (dict(out=None), NULLS),
    (dict(ld_base=18), "score_expect_groups: base row stride 18 < n_groups + 1 = 19"),
    (dict(sub_ids=P, T=3, ld_sub=3), "score_expect_groups: sub_ids given without sub_w (the two come together)"),
    (dict(sub_w=P, T=3, ld_sub=3), "score_expect_groups: sub_w given without sub_ids (the two come together)"),
    (dict(sub_ids=P, sub_w=P, T=129, ld_sub=129), "score_expect_groups: T = 129 named rows per user (row stride 129), must be in [1, 128] with ld_sub >= T"),
    (dict(sub_ids=P, sub_w=P, T=4, ld_sub=3), "score_expect_groups: T = 4 named rows per user (row stride 3), must be in [1, 128] with ld_sub >= T"),
    (dict(user=P + 8), "score_expect_groups: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
    (dict(ld_out=396), "score_expect_groups: out must be 16-byte aligned with ld_out = 396 >= N = 400"),
    (dict(out=P + 4), "score_expect_groups: out must be 16-byte aligned with ld_out = 400 >= N = 400"),
]


@pytest.mark.parametrize("change,message", EG_REFUSED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(EG_REFUSED)])
def test_score_expect_groups_refuses_before_any_launch(change, message):
    d = _lib.ExpectGroupsDesc(**{**EG, **change})
    assert _lib.lib().nr_score_expect_groups(C.byref(d), None) == 1 and _lib.last_error() == message, _lib.last_error()


def test_score_expect_groups_workspace_and_texts_are_k15s():
    assert _lib.lib().nr_score_expect_groups(None, None) == 1 and _lib.last_error() == "score_expect_groups: null descriptor"
    assert _lib.lib().nr_score_expect_groups_workspace_bytes(None) == 0
    d = _lib.ExpectGroupsDesc(**{**EG, "splits": 7})
    assert _lib.lib().nr_score_expect_groups_workspace_bytes(C.byref(d)) == 8192 * 7 * (400 * 4 + 8)
    d = _lib.ExpectGroupsDesc(**{**EG, "splits": 3, "U": 5, "N": 40})
    assert _lib.lib().nr_score_expect_groups_workspace_bytes(C.byref(d)) == 5 * 3 * (40 * 4 + 8)
    d = _lib.ExpectGroupsDesc(**{**EG, "splits": 7, "ws_bytes": 8192 * 7 * (400 * 4 + 8) - 1})
    assert _lib.lib().nr_score_expect_groups(C.byref(d), None) == 1
    assert _lib.last_error() == (f"score_expect_groups: workspace holds {8192 * 7 * 1608 - 1} bytes, nr_score_expect_groups_workspace_bytes asks for "
                                 f"{8192 * 7 * 1608} (8-byte aligned)")
    # a rule K15 states gives K15's sentence under this call's name
    k15 = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, order=P, n_pos=102400, seg_start=P, nseg=275,
               bin_seg=P, n_groups=18, out_logsum=P, out_max=P, out_count=P, ws=P, ws_bytes=1 << 40)
    for change in (dict(V=1), dict(tau=NAN), dict(n_groups=0), dict(n_pos=100), dict(nseg=276), dict(splits=276), dict(stamp=P), dict(user=P + 8)):
        assert _lib.lib().nr_score_logz_groups(C.byref(_lib.LogzGroupsDesc(**{**k15, **change})), None) == 1
        said = _lib.last_error()
        assert _lib.lib().nr_score_expect_groups(C.byref(_lib.ExpectGroupsDesc(**{**EG, **change})), None) == 1
        assert _lib.last_error() == said.replace("score_logz_groups:", "score_expect_groups:"), (change, said)


CG = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, k=10, row_ids=P, ld_ids=10, group=P, group_cap=2, n_groups=18,
          tau=0.5, base_max=P, base_logsum=P, ld_base=19, out_bin_w=P, out_sub_w=P)
CG_NULLS = "row_logprob_capped_grad: null pointer (news_vecs, user, row_ids, group, base_max, base_logsum, out_bin_w, out_sub_w)"
CG_REFUSED = [
    (dict(k=0), "row_logprob_capped_grad: k = 0 entries per row, must be in [1, 128]"),
    (dict(k=129, ld_ids=129), "row_logprob_capped_grad: k = 129 entries per row, must be in [1, 128]"),
    (dict(tau=INF), "row_logprob_capped_grad: tau = inf, a scalar temperature must be finite and > 0"),
    (dict(group_cap=0), "row_logprob_capped_grad: group_cap = 0, must be in [1, 128]"),
    (dict(group_cap=129), "row_logprob_capped_grad: group_cap = 129, must be in [1, 128]"),
    (dict(n_groups=513, ld_base=514), "row_logprob_capped_grad: n_groups = 513, must be in [1, 512]"),
    (dict(group=None), CG_NULLS),
    (dict(out_bin_w=None), CG_NULLS),
    (dict(out_sub_w=None), CG_NULLS),
    (dict(ld_ids=9), "row_logprob_capped_grad: id row stride 9 < k = 10"),
    (dict(ld_base=18), "row_logprob_capped_grad: base row stride 18 < n_groups + 1 = 19"),
    (dict(g=P, ld_g=9), "row_logprob_capped_grad: g row stride 9 < k = 10"),
    (dict(stamp=P), "row_logprob_capped_grad: stamp given without window (the two come together)"),
    (dict(user=P + 8), "row_logprob_capped_grad: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
]


@pytest.mark.parametrize("change,message", CG_REFUSED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(CG_REFUSED)])
def test_row_logprob_capped_grad_refuses_before_any_launch(change, message):
    d = _lib.LogprobCappedGradDesc(**{**CG, **change})
    assert _lib.lib().nr_row_logprob_capped_grad(C.byref(d), None) == 1 and _lib.last_error() == message, _lib.last_error()


def test_row_logprob_capped_grad_texts_are_k16s():
    assert _lib.lib().nr_row_logprob_capped_grad(None, None) == 1 and _lib.last_error() == "row_logprob_capped_grad: null descriptor"
    k16 = {**{n: v for n, v in CG.items() if n not in ("out_bin_w", "out_sub_w")}, "out_logp": P}
    for change in (dict(k=0), dict(tau=NAN), dict(group_cap=0), dict(n_groups=0), dict(ld_ids=9), dict(ld_base=18), dict(V=1), dict(user=P + 8)):
        assert _lib.lib().nr_row_logprob_capped(C.byref(_lib.LogprobCappedDesc(**{**k16, **change})), None) == 1
        said = _lib.last_error()
        assert _lib.lib().nr_row_logprob_capped_grad(C.byref(_lib.LogprobCappedGradDesc(**{**CG, **change})), None) == 1
        assert _lib.last_error() == said.replace("row_logprob_capped:", "row_logprob_capped_grad:"), (change, said)


def test_host_side_refusals_of_the_python_layers():
    news, user = torch.zeros(10, 8), torch.zeros(3, 8)
    group = torch.tensor([0, 0, 1, 1, 0, -1, 1, 0, 1, -1], dtype=torch.int32)
    order = ops.GroupOrder(group)
    rows = torch.ones(3, 2, dtype=torch.int32)
    bases = (torch.zeros(3, 3), torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_expect_groups(news, user, 0.5, order, bases, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.row_logprob_capped_grad(news, user, rows, 0.5, bases, group, 2)
    with pytest.raises(RuntimeError, match=r"bin_w must be a floating point tensor of shape \(3, n_groups \+ 1 = 3\)"):
        ops.score_expect_groups(news, user, 0.5, order, bases, torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match="groups must be an ops.GroupOrder"):
        ops.score_expect_groups(news, user, 0.5, group, bases, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="g must be a floating point tensor of shape"):
        ops.row_logprob_capped_grad(news, user, rows, 0.5, bases, group, 2, g=torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="base logsum must be a floating point tensor"):
        ops.row_logprob_capped_grad(news, user, rows, 0.5, (torch.zeros(3, 2), torch.zeros(3, 3)), group, 2, n_groups=2)
    with pytest.raises(RuntimeError, match="missing pass"):
        ops.plackett_luce_nll_capped(news.clone().requires_grad_(), user, rows, 0.5, order, group, 2)
    with pytest.raises(RuntimeError, match="must be in \\[1, 128\\]"):
        ops.plackett_luce_nll_capped(news, user, torch.ones(3, 129, dtype=torch.int32), 0.5, order, group, 2)
    for cap in (0, 129):
        with pytest.raises(RuntimeError, match="group_cap = .* must be in \\[1, 128\\]"):
            ops.plackett_luce_nll_capped(news, user, rows, 0.5, order, group, cap)
        with pytest.raises(ValueError, match="group_cap = .* must be in \\[1, 128\\]"):
            train.listwise_loss_capped(None, news, None, None, None, 0.5, group, cap)
    with pytest.raises(RuntimeError, match="rows must be an integer tensor"):
        ops.plackett_luce_nll_capped(news, user, torch.ones(4, 2, dtype=torch.int32), 0.5, order, group, 2)
    with pytest.raises(RuntimeError, match="missing pass"):
        train.listwise_loss_capped(None, news.clone().requires_grad_(), None, None, None, 0.5, group, 2)
    # the uncapped loss keeps its refusal
    with pytest.raises(ValueError, match="group caps"):
        train.listwise_loss(None, None, None, None, None, 0.5, news_group=np.zeros(4))


def test_blocked_entries_of_a_row():
    group = torch.tensor([0, 0, 0, 1, 0, -1, 1, 0, -1, 1], dtype=torch.int32)
    rw = torch.tensor([[1, 2, 3, 4, 7, 5, 8, 6, 9],
                       [1, 0, 2, 4, 0, 7, 3, 6, 9]], dtype=torch.int32)
    got = train._blocked(rw, group, 2, 2)
    #            g0 g0 g1 g0* g0* ng ng g1 g1*     /   g0 fill g0 g0* fill g0* g1 g1 g1*
    want = torch.tensor([[0, 0, 0, 1, 1, 0, 0, 0, 1], [0, 0, 0, 1, 0, 1, 0, 0, 1]], dtype=torch.bool)
    assert torch.equal(got, want)
    assert not train._blocked(rw, group, 2, 128).any()

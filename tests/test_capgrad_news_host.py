"""CPU: the host side of the news-table gradient under group caps (include/nrhip.h, K22) -- metrics.expect_news_groups_reference
composed with metrics.capped_row_logprob_grad_reference against float64 autograd of the DENSE capped NLL with respect to the news
table, a mutant per formula, GroupOrder.by_position against a brute-force transpose, the descriptor's place in nr_abi_sizes, the
new names, the workspace size, and the refusals made before any launch (fake non-null pointers: a launch would fault, a refusal
does not) with the whole text of nr_last_error."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from capgrad_news_helpers import autograd_news_gradient, bins_of, composed_reference
from newsrecommendation_amd import _lib, metrics, ops, train

INF, NAN = float("inf"), float("nan")
V, N, G, U, K = 41, 6, 3, 3, 8


def _corpus(seed=3):
    """41 news, groups 0 / 1 / none in turn and a group 2 of exactly two news (7 and 8); three users with their own temperatures,
    lists and windows; rows of k = 8 that take ALL of group 2 (cap 2: both are steps and the bin is empty afterwards; cap 1: the
    second is blocked), hold further blocked entries under both caps, a fill entry and one entry outside the user's pool; signed g."""
    rng = np.random.default_rng(seed)
    news, user = rng.standard_normal((V, N)), rng.standard_normal((U, N)) / 2
    group = np.array([(0, 1, -1)[v % 3] for v in range(V)], dtype=np.int64)
    group[[7, 8]] = 2
    tau = np.array([0.7, 1.3, 0.45])
    lists = [np.array([5, 6, 17, 40]), np.zeros(0, dtype=np.int64), np.array([2, 30, 31, 32, 33, 99])]
    prior = 0.3 * rng.standard_normal(V)
    prior[[11, 26]] = -INF
    stamp = rng.integers(0, 50, V)
    window = np.array([[0, 49], [5, 45], [0, 40]])
    stamp[[7, 8, 3, 9, 12, 15, 18, 21, 13, 16, 10, 1, 4]] = 20        # the rows' entries are inside every window ...
    stamp[19] = 48                                                     # ... but for 19, outside user 2's
    #                 g0  g2  g0  g2  g0* g1   fill  none      (* blocked under both caps: a third news of group 0)
    rows = np.array([[3,  7,  9,  8,  12, 13,  0,    14],
                     [15, 8,  7,  18, 21, 16,  10,   0],
                     [7,  1,  19, 8,  4,  3,   9,    44]], dtype=np.int64)
    g = rng.standard_normal((U, K))
    g[0, 4] = 55.0                                                     # not read: blocked
    return news, user, group, tau, lists, prior, stamp, window, rows, g


@pytest.mark.parametrize("cap", [1, 2])
def test_reference_against_autograd_of_the_dense_capped_nll(cap):
    news, user, group, tau, lists, prior, stamp, window, rows, g = _corpus()
    kw = dict(exclude=lists, prior=prior, stamp=stamp, window=window)
    want, loss = autograd_news_gradient(news, user, rows, g, tau, group, G, cap, **kw)
    got, A, om, c = composed_reference(news, user, rows, g, tau, group, G, cap, **kw)
    worst = float(np.abs(got - want).max())
    print(f"cap {cap}: worst |closed form - autograd| = {worst:.3e}, largest |gradient| {np.abs(want).max():.3e}, loss {loss:.4f}")
    assert worst <= 1e-12 * max(A.max(), 1.0) and np.abs(want).max() > 0.1
    # the cases the corpus is there for: group 2's bin is empty in the bases of every user (the row took all of it) while its
    # entries carry c != 0; a blocked entry has c != 0; fill and the entry outside the pool have c = 0
    assert (om[:, 2] == 0).all() and (c[0, [1, 3]] != 0).all() and c[0, 4] != 0 and c[0, 6] == 0 and c[2, 2] == 0 and c[2, 7] == 0
    assert not got[0].any() and not got[11].any() and not got[26].any()       # row 0; prior -inf and named by nobody


@pytest.mark.parametrize("mutant", ["wrong_bin", "named_base_gate", "no_inv_tau"])
def test_each_mutant_formula_fails_against_autograd(mutant):
    news, user, group, tau, lists, prior, stamp, window, rows, g = _corpus()
    kw = dict(exclude=lists, prior=prior, stamp=stamp, window=window)
    want, _ = autograd_news_gradient(news, user, rows, g, tau, group, G, 2, **kw)
    good, A, _, _ = composed_reference(news, user, rows, g, tau, group, G, 2, **kw)
    bad, _, _, _ = composed_reference(news, user, rows, g, tau, group, G, 2, mutant=mutant, **kw)
    tol = 1e-12 * max(A.max(), 1.0)
    assert np.abs(good - want).max() <= tol and np.abs(bad - want).max() > 1e-3, mutant


def test_reference_edge_cases_and_k18_collapse():
    news, user, group, tau, lists, prior, stamp, window, rows, g = _corpus()
    rng = np.random.default_rng(9)
    om = rng.standard_normal((U, G + 1))
    # one bin holding everything, omega = weight: expect_news_reference's rows and mass
    one = np.zeros(V, dtype=np.int64)
    w = rng.standard_normal(U)
    bw = np.stack([w, np.zeros(U)], axis=1)
    out, mass, A, M = metrics.expect_news_groups_reference(news, user, temperature=tau, group=one, n_groups=1, bin_w=bw, exclude=lists, prior=prior,
                                                           scale_inv_tau=True)
    o18, m18 = metrics.expect_news_reference(news, user, temperature=tau, exclude=lists, prior=prior, weight=w, scale_inv_tau=True)
    assert np.abs(out - o18).max() <= 1e-13 and np.abs(mass - m18).max() <= 1e-13 and (A >= np.abs(out) - 1e-15).all() and (M >= np.abs(mass) - 1e-15).all()
    # pairs that are not live contribute nothing and leave no NaN: omega 0 / NaN / inf, a bad temperature; `dead` marks what only
    # the device's bases know
    om2 = om.copy()
    om2[0, 0], om2[1, 1], om2[2, 3] = NAN, INF, 0.0
    t2 = tau.copy()
    out2, mass2, _, _ = metrics.expect_news_groups_reference(news, user, temperature=t2, group=group, n_groups=G, bin_w=om2)
    om3 = np.where(np.isfinite(om2), om2, 0.0)
    out3, mass3, _, _ = metrics.expect_news_groups_reference(news, user, temperature=t2, group=group, n_groups=G, bin_w=om3)
    assert np.isfinite(out2).all() and np.array_equal(out2, out3) and np.array_equal(mass2, mass3)
    dead = np.zeros((U, G + 1), dtype=bool)
    dead[1, 0] = True
    om4 = om3.copy()
    om4[1, 0] = 0.0
    out4 = metrics.expect_news_groups_reference(news, user, temperature=t2, group=group, n_groups=G, bin_w=om3, dead=dead)[0]
    assert np.array_equal(out4, metrics.expect_news_groups_reference(news, user, temperature=t2, group=group, n_groups=G, bin_w=om4)[0])
    t2[1] = 0.0
    named = (np.array([0, 0, 2] + [2] * (V - 2)), np.array([1, 2]), np.array([0.5, -2.0]))
    out5, _, _, _ = metrics.expect_news_groups_reference(news, user, temperature=t2, group=group, n_groups=G, bin_w=np.zeros((U, G + 1)), named=named,
                                                         scale_inv_tau=True)
    want = np.zeros((V, N))
    want[1] = 2.0 / tau[2] * user[2]                                  # user 1 is dead (temperature 0); no base gates user 2's term
    assert np.abs(out5 - want).max() <= 1e-15
    # bases given = the bin's own exact softmax
    bases = metrics.logz_groups_reference(news, user, temperature=tau, group=group, n_groups=G, exclude=lists)
    a = metrics.expect_news_groups_reference(news, user, temperature=tau, group=group, n_groups=G, bin_w=om, exclude=lists)
    b = metrics.expect_news_groups_reference(news, user, temperature=tau, group=group, n_groups=G, bin_w=om, exclude=lists, bases=bases[:2])
    assert np.abs(a[0] - b[0]).max() <= 1e-13 and np.abs(a[1] - b[1]).max() <= 1e-13
    # the masses of a bin add up to the users' omega of that bin
    bn = bins_of(group, G)
    for b_ in range(G + 1):
        assert abs(a[1][bn == b_][1 if b_ == bn[0] else 0:].sum() - om[:, b_].sum()) <= 1e-12


def test_by_position_against_a_brute_force_transpose():
    g = torch.Generator().manual_seed(4)
    Vc, Uc = 300, 37
    group = torch.randint(-1, 5, (Vc,), generator=g, dtype=torch.int32)
    order = ops.GroupOrder(group)
    t = torch.randint(0, Vc + 3, (Uc, 9), generator=g, dtype=torch.int32)
    t[3] = 0
    t[5, :4] = torch.tensor([7, 7, 1, Vc - 1])
    lists = ops.ExclusionLists(t)
    off, users = order.by_position(lists)
    assert off.dtype == torch.int32 and users.dtype == torch.int32 and tuple(off.shape) == (order.n_pos + 1,) and int(off[0]) == 0
    want = [[] for _ in range(order.n_pos)]
    for u in range(Uc):
        for v in sorted(set(int(x) for x in t[u] if 1 <= int(x) < Vc)):
            want[int(order.pos[v])].append(u)
    for p in range(order.n_pos):
        assert users[int(off[p]):int(off[p + 1])].tolist() == want[p], p
    assert int(off[-1]) == sum(len(x) for x in want) == users.numel()
    # padding positions hold nothing; it is by_news with the ids mapped through pos
    pad = (order.order == 0).nonzero().reshape(-1)
    assert pad.numel() > 0 and all(int(off[p]) == int(off[p + 1]) for p in pad.tolist())
    noff, nusers = lists.by_news(Vc)
    for v in range(1, Vc):
        p = int(order.pos[v])
        assert users[int(off[p]):int(off[p + 1])].tolist() == nusers[int(noff[v]):int(noff[v + 1])].tolist()
    empty = order.by_position(ops.ExclusionLists(torch.zeros(Uc, 2, dtype=torch.int32)))
    assert empty[1].numel() == 0 and not empty[0].any()


def test_descriptor_is_entry_20_of_abi_sizes_and_the_new_names():
    sizes = (C.c_size_t * 21)()
    assert _lib.lib().nr_abi_sizes(sizes, 21) == 0 and sizes[20] == C.sizeof(_lib.ExpectNewsGroupsDesc) and all(sizes)
    assert sizes[19] == C.sizeof(_lib.LogprobCappedGradDesc) and sizes[18] == C.sizeof(_lib.ExpectGroupsDesc)
    twenty = (C.c_size_t * 21)()
    twenty[20] = 12345
    assert _lib.lib().nr_abi_sizes(twenty, 20) == 0 and twenty[20] == 12345 and list(twenty)[:20] == list(sizes)[:20]
    for name in ("nr_score_expect_news_groups_workspace_bytes", "nr_score_expect_news_groups"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.RESTYPES["nr_score_expect_news_groups_workspace_bytes"] is C.c_size_t
    # K18's fields in order up to tau_u, then this call's, then the shared tail
    names = [f[0] for f in _lib.ExpectNewsGroupsDesc._fields_]
    k18 = [f[0] for f in _lib.ExpectNewsDesc._fields_]
    assert names[:k18.index("tau_u") + 1] == k18[:k18.index("tau_u") + 1] and names[-4:] == k18[-4:]
    assert names[k18.index("tau_u") + 1:-4] == ["order", "n_pos", "bin_start", "n_groups", "base_max", "base_logsum", "bin_w", "ld_bin",
                                                "scale_inv_tau", "named_offsets", "named_user", "named_w", "n_named", "out", "ld_out", "out_mass",
                                                "ws", "ws_bytes"]
    assert list(inspect.signature(ops.score_expect_news_groups).parameters) == ["news_vecs", "user_vecs", "temperature", "groups", "bases", "bin_w",
                                                                                "exclude", "splits", "prior", "stamp", "window"]
    assert list(inspect.signature(ops.plackett_luce_nll_capped_joint).parameters) == list(inspect.signature(ops.plackett_luce_nll_capped).parameters)
    assert list(inspect.signature(train.listwise_loss_capped_joint).parameters) == list(inspect.signature(train.listwise_loss_capped).parameters)
    assert callable(ops.GroupOrder.by_position) and callable(ops._score_expect_news_groups)
    kinds = inspect.signature(metrics.expect_news_groups_reference).parameters
    assert list(kinds)[:2] == ["a", "b"] and all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(kinds)[2:])


P = 4096                                                               # a fake pointer, 16-byte aligned
ENG = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, order=P, n_pos=102400, bin_start=P, n_groups=18,
           base_max=P, base_logsum=P, bin_w=P, ld_bin=8192, out=P, ld_out=400, ws=P, ws_bytes=1 << 40)
NULLS = "score_expect_news_groups: null pointer (news_vecs, user, order, bin_start, base_max, base_logsum, bin_w, out)"
NAMED = "score_expect_news_groups: named_offsets, named_user and named_w come together (all three or none)"
ENG_REFUSED = [
    (dict(V=1), "score_expect_news_groups: V = 1 news rows; row 0 is the padding news, so at least 2 are needed"),
    (dict(U=0), "score_expect_news_groups: U = 0 users"),
    (dict(N=402), "score_expect_news_groups: vector width N = 402 must be a multiple of 4 in [4, 1024]"),
    (dict(N=1028), "score_expect_news_groups: vector width N = 1028 must be a multiple of 4 in [4, 1024]"),
    (dict(n_excl=-1), "score_expect_news_groups: n_excl = -1 entries of excl_users, must be >= 0"),
    (dict(excl_users=P, n_excl=3), "score_expect_news_groups: excl_users given without excl_offsets (n_excl = 3; the two come together)"),
    (dict(excl_offsets=P, n_excl=3), "score_expect_news_groups: excl_offsets given without excl_users (n_excl = 3; the two come together)"),
    (dict(tau=0.0), "score_expect_news_groups: tau = 0, a scalar temperature must be finite and > 0"),
    (dict(tau=NAN), "score_expect_news_groups: tau = nan, a scalar temperature must be finite and > 0"),
    (dict(tau=INF), "score_expect_news_groups: tau = inf, a scalar temperature must be finite and > 0"),
    (dict(n_groups=0), "score_expect_news_groups: n_groups = 0, must be in [1, 512]"),
    (dict(n_groups=513), "score_expect_news_groups: n_groups = 513, must be in [1, 512]"),
    (dict(n_pos=0), "score_expect_news_groups: n_pos = 0 positions, must be a positive multiple of 128"),
    (dict(n_pos=100), "score_expect_news_groups: n_pos = 100 positions, must be a positive multiple of 128"),
    (dict(splits=-1), "score_expect_news_groups: splits = -1, must be 0 (library's choice) or in [1, 64], the segments of U = 8192"),
    (dict(splits=65), "score_expect_news_groups: splits = 65, must be 0 (library's choice) or in [1, 64], the segments of U = 8192"),
    (dict(stamp=P), "score_expect_news_groups: stamp given without window (the two come together)"),
    (dict(window=P, ld_window=2), "score_expect_news_groups: window given without stamp (the two come together)"),
    (dict(stamp=P, window=P, ld_window=1), "score_expect_news_groups: ld_window = 1, a window row is (lo, hi): at least 2"),
    (dict(news_vecs=None), NULLS),
    (dict(user=None), NULLS),
    (dict(order=None), NULLS),
    (dict(bin_start=None), NULLS),
    (dict(base_max=None), NULLS),
    (dict(base_logsum=None), NULLS),
    (dict(bin_w=None), NULLS),
    (dict(out=None), NULLS),
    (dict(ld_bin=8191), "score_expect_news_groups: bin-major row stride ld_bin = 8191 < U = 8192"),
    (dict(named_offsets=P), NAMED),
    (dict(named_user=P, named_w=P), NAMED),
    (dict(named_offsets=P, named_w=P, n_named=4), NAMED),
    (dict(named_offsets=P, named_user=P, named_w=P, n_named=-1), "score_expect_news_groups: n_named = -1 named terms, must be >= 0"),
    (dict(user=P + 8), "score_expect_news_groups: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)"),
    (dict(ld_news=396), "score_expect_news_groups: rows must be 16-byte aligned (ld_news = 396, ld_user = 400: multiples of 4, >= N = 400)"),
    (dict(ld_out=396), "score_expect_news_groups: out must be 16-byte aligned with ld_out = 396 >= N = 400"),
    (dict(out=P + 4), "score_expect_news_groups: out must be 16-byte aligned with ld_out = 400 >= N = 400"),
    (dict(ws=None), f"score_expect_news_groups: workspace holds {1 << 40} bytes, nr_score_expect_news_groups_workspace_bytes asks for "
                    f"{100001 * 1 * 1608} (8-byte aligned)"),
]


@pytest.mark.parametrize("change,message", ENG_REFUSED, ids=[f"{i}-{'-'.join(c)}" for i, (c, _) in enumerate(ENG_REFUSED)])
def test_score_expect_news_groups_refuses_before_any_launch(change, message):
    d = _lib.ExpectNewsGroupsDesc(**{**ENG, **change})
    assert _lib.lib().nr_score_expect_news_groups(C.byref(d), None) == 1 and _lib.last_error() == message, _lib.last_error()


def test_workspace_is_host_arithmetic_and_the_shared_texts_are_k18s_and_k15s():
    assert _lib.lib().nr_score_expect_news_groups(None, None) == 1 and _lib.last_error() == "score_expect_news_groups: null descriptor"
    assert _lib.lib().nr_score_expect_news_groups_workspace_bytes(None) == 0
    ws = _lib.lib().nr_score_expect_news_groups_workspace_bytes
    # V * slices * (N * 4 + 8): the slices are K18's plan of the user axis (8192 users = 64 segments of one chunk)
    assert ws(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, "splits": 7}))) == 100001 * 7 * (400 * 4 + 8)          # 10 segments a slice: 7 slices
    assert ws(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, "splits": 64}))) == 100001 * 64 * (400 * 4 + 8)
    assert ws(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, "splits": 5}))) == 100001 * 5 * (400 * 4 + 8)          # 13 a slice: 5 slices
    assert ws(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, "splits": 3, "V": 7, "U": 300, "N": 36, "ld_bin": 300}))) == 7 * 3 * (36 * 4 + 8)
    assert ws(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, "splits": 2, "V": 7, "U": 1, "N": 4, "ld_bin": 1}))) == 0   # one segment: refused
    # the same plan as K18's for the same (V, U, N, splits), the library's choice included
    k18 = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, base_max=P, base_logsum=P, out=P, ld_out=400, ws=P,
               ws_bytes=1 << 40)
    for change in (dict(), dict(splits=9), dict(U=64), dict(U=128 * 256 + 5, splits=2, ld_bin=128 * 256 + 5), dict(N=836, ld_news=836, ld_user=836,
                                                                                                                 ld_out=836)):
        a = ws(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, **change})))
        b = _lib.lib().nr_score_expect_news_workspace_bytes(C.byref(_lib.ExpectNewsDesc(**{**k18, **{n: v for n, v in change.items() if n != "ld_bin"}})))
        assert a == b and a > 0, change
    d = _lib.ExpectNewsGroupsDesc(**{**ENG, "splits": 7, "ws_bytes": 100001 * 7 * 1608 - 1})
    assert _lib.lib().nr_score_expect_news_groups(C.byref(d), None) == 1
    assert _lib.last_error() == (f"score_expect_news_groups: workspace holds {100001 * 7 * 1608 - 1} bytes, nr_score_expect_news_groups_workspace_bytes "
                                 f"asks for {100001 * 7 * 1608} (8-byte aligned)")
    # a rule K18 states of the shared fields gives K18's sentence under this call's name; so do K15's of n_groups and n_pos
    for change in (dict(V=1), dict(U=0), dict(N=402), dict(n_excl=-1), dict(excl_users=P, n_excl=3), dict(tau=NAN), dict(splits=65), dict(stamp=P),
                   dict(user=P + 8), dict(named_offsets=P), dict(named_offsets=P, named_user=P, named_w=P, n_named=-1), dict(ld_out=396)):
        assert _lib.lib().nr_score_expect_news(C.byref(_lib.ExpectNewsDesc(**{**k18, **change})), None) == 1
        said = _lib.last_error()
        assert _lib.lib().nr_score_expect_news_groups(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, **change})), None) == 1
        assert _lib.last_error() == said.replace("score_expect_news:", "score_expect_news_groups:"), (change, said)
    k15 = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400, tau=0.5, order=P, n_pos=102400, seg_start=P, nseg=275,
               bin_seg=P, n_groups=18, out_logsum=P, out_max=P, out_count=P, ws=P, ws_bytes=1 << 40)
    for change in (dict(n_groups=0), dict(n_groups=513), dict(n_pos=100), dict(n_pos=0)):
        assert _lib.lib().nr_score_logz_groups(C.byref(_lib.LogzGroupsDesc(**{**k15, **change})), None) == 1
        said = _lib.last_error()
        assert _lib.lib().nr_score_expect_news_groups(C.byref(_lib.ExpectNewsGroupsDesc(**{**ENG, **change})), None) == 1
        assert _lib.last_error() == said.replace("score_logz_groups:", "score_expect_news_groups:"), (change, said)


def test_host_side_refusals_of_the_python_layers():
    news, user = torch.zeros(10, 8), torch.zeros(3, 8)
    group = torch.tensor([0, 0, 1, 1, 0, -1, 1, 0, 1, -1], dtype=torch.int32)
    order = ops.GroupOrder(group)
    rows = torch.ones(3, 2, dtype=torch.int32)
    bases = (torch.zeros(3, 3), torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_expect_news_groups(news, user, 0.5, order, bases, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.plackett_luce_nll_capped_joint(news.clone().requires_grad_(), user, rows, 0.5, order, group, 2)
    with pytest.raises(RuntimeError, match=r"bin_w must be a floating point tensor of shape \(3, n_groups \+ 1 = 3\)"):
        ops.score_expect_news_groups(news, user, 0.5, order, bases, torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match=r"base gmax must be a floating point tensor of shape \(3, n_groups \+ 1 = 3\)"):
        ops.score_expect_news_groups(news, user, 0.5, order, (torch.zeros(3, 3), torch.zeros(3, 3, dtype=torch.int32)), torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="groups must be an ops.GroupOrder"):
        ops.score_expect_news_groups(news, user, 0.5, group, bases, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="the GroupOrder was built for V = 10 news"):
        ops.score_expect_news_groups(torch.zeros(11, 8), user, 0.5, order, bases, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="vector widths differ"):
        ops.score_expect_news_groups(news, torch.zeros(3, 12), 0.5, order, bases, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="user_vecs must be a 2-D fp32 tensor"):
        ops.score_expect_news_groups(news, user.double(), 0.5, order, bases, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match=r"exclude must be a tensor \[U = 3, E\] or an ExclusionLists"):
        ops.score_expect_news_groups(news, user, 0.5, order, bases, torch.zeros(3, 3), exclude=torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="the exclusion lists are for 4 users"):
        ops.score_expect_news_groups(news, user, 0.5, order, bases, torch.zeros(3, 3), exclude=ops.ExclusionLists(torch.zeros(4, 2, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="the named terms must be offsets"):
        ops._score_expect_news_groups("x", news, user, 0.5, order, bases, torch.zeros(3, 3), None, 0, None, None, None,
                                      (torch.zeros(10, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2)), True)
    with pytest.raises(RuntimeError, match="must be in \\[1, 128\\]"):
        ops.plackett_luce_nll_capped_joint(news, user, torch.ones(3, 129, dtype=torch.int32), 0.5, order, group, 2)
    for cap in (0, 129):
        with pytest.raises(RuntimeError, match="plackett_luce_nll_capped_joint: group_cap = .* must be in \\[1, 128\\]"):
            ops.plackett_luce_nll_capped_joint(news, user, rows, 0.5, order, group, cap)
        with pytest.raises(ValueError, match="listwise_loss_capped_joint: group_cap = .* must be in \\[1, 128\\]"):
            train.listwise_loss_capped_joint(None, news, None, None, None, 0.5, group, cap)
    with pytest.raises(RuntimeError, match="plackett_luce_nll_capped_joint: rows must be an integer tensor"):
        ops.plackett_luce_nll_capped_joint(news, user, torch.ones(4, 2, dtype=torch.int32), 0.5, order, group, 2)
    with pytest.raises(RuntimeError, match="plackett_luce_nll_capped_joint: groups must be an ops.GroupOrder"):
        ops.plackett_luce_nll_capped_joint(news, user, rows, 0.5, group, group, 2)
    # the two frozen-table functions keep their refusal and now point at the joint ones
    with pytest.raises(RuntimeError, match="missing pass.*use plackett_luce_nll_capped_joint"):
        ops.plackett_luce_nll_capped(news.clone().requires_grad_(), user, rows, 0.5, order, group, 2)
    with pytest.raises(RuntimeError, match="missing pass.*use listwise_loss_capped_joint"):
        train.listwise_loss_capped(None, news.clone().requires_grad_(), None, None, None, 0.5, group, 2)

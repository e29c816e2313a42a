"""GPU: the news-table pass of the entropy-regularised full softmax (nr_score_expect_news_affine; ops.score_expect_news_affine /
ops.full_softmax_nll_entropy_joint; train.full_softmax_loss_entropy_joint; include/nrhip.h, K25).  The device is held to a bound
DERIVED from its order of operations (K18's kappa + 2, below) against metrics.expect_news_affine_reference in float64 on the fp32
inputs; bit statements where the contract makes them (beta = None: K18's rows with weight = alpha; the mass is K18's without a
weight; fixed splits: a row does not depend on the other news rows or on its place; the forward, grad_user and grad_tau are
full_softmax_nll_entropy's; no entropy gradient: full_softmax_nll_joint's table gradient)."""
import math

import numpy as np
import pytest
import torch

import test_gpu_entropy as GH
import test_gpu_expect as GE
import test_gpu_expect_news as EN
from helpers import assert_close
from newsrecommendation_amd import metrics, ops, train as TR
from oracle import nr_oracle as O

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
EPS = EN.EPS
U_TWO = EN.U_TWO
DEV = "cuda"
_bits = EN._bits
_host = EN._host


def kappas(N, V, U, splits, n, C, G):
    """(kappa'' of the rows, kappa of the mass).  |out_vc - out*_vc| <= kappa'' e A_vc with
      A_vc = sum_u (1 / tau_u) (|alpha_u| + |beta_u| (|x*_uv| + 1)) p*_uv |user_uc| + sum_j |d_j| |user_jc|.
    K18's terms (test_gpu_expect_news.kappas) stand as they are: the score chain, the exponent, the base and expf give p within a
    relative error; fl(alpha fl(1 / tau)) and fl(beta fl(1 / tau)) are K18's two coefficient roundings, each on its own summand of
    |a| + |b| |x|; fl(p * w) is K18's fl(c * p).  New: the fma fl(b x + a) rounds once, e |b x + a| <= e (|a| + |b| |x|): + 1.  x itself
    carries the ABSOLUTE error kappa_x e (kappa_x < kappa''), which beta carries into the weight: |b| kappa_x e p -- the `+ 1` beside
    |x*| in A.  + 1 for the second order (the |x| of the fma's bound is the device's, not x*).  kappa'' = kappa + 2.
    The mass is K18's with weight = 1: the same fp64 chains of p."""
    kr, km = EN.kappas(N, V, U, splits, n, C, G)
    return kr + 2.0, km


def _reference(news, user, tau, hkw, alpha=None, beta=None, named=None, scale=False, dead=()):
    """(out*, A, mass*, M, n, C, G) in float64 on the fp32 inputs.  `dead`: users the reference is told to leave out (a NaN base is the
    device's knowledge, not the reference's): their temperature becomes 0."""
    a, b = news.double().cpu().numpy(), user.double().cpu().numpy()
    U, V = b.shape[0], a.shape[0]
    taus = np.array(metrics._temperatures(_host(tau), U)[0], dtype=np.float64)
    taus[list(dead)] = 0.0
    al = np.ones(U) if alpha is None else _host(alpha).astype(np.float64)
    be = np.zeros(U) if beta is None else _host(beta).astype(np.float64)
    nm = None if named is None else tuple(_host(x) for x in named)
    out, mass = metrics.expect_news_affine_reference(a, b, temperature=taus, alpha=al, beta=be, named=nm, scale_inv_tau=scale, **hkw)
    _, _, mass18, M, n, C, G = EN._reference(news, user, torch.from_numpy(taus), hkw)
    assert np.array_equal(mass, mass18)                                # K18's mass without a weight
    p, live = metrics.softmax_matrix_reference(a, b, temperature=taus, **hkw)
    with np.errstate(divide="ignore", invalid="ignore"):
        it = np.where(live, 1.0 / taus, 0.0)
        sc = it if scale else live.astype(np.float64)
        fin = np.isfinite(al * sc) & np.isfinite(be * sc)
        ca, cb = np.where(fin, np.abs(al) * sc, 0.0), np.where(fin, np.abs(be) * sc, 0.0)
        x = np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), 0.0)
    babs = np.abs(np.where(np.isfinite(b), b, 0.0))
    A = (p * (ca[:, None] + cb[:, None] * (np.abs(x) + 1.0))).T @ babs
    if nm is not None:
        off, nu, nw = nm
        news_of = np.repeat(np.arange(V), np.diff(off))
        d = np.abs(nw.astype(np.float64)) * sc[nu]
        np.add.at(A, news_of, d[:, None] * babs[nu])
    # weights below the normal range (x < -87; expf gives 0 below -104) are lost at no more than 2^-126 (|a| + 105 |b|) each
    A = A + U * 2.0 ** -126 * max(float((ca + 105.0 * cb).max()), 1.0) * float(babs.max())
    return out, A, mass, M, n, C, G


def _check(news, user, tau, hkw, got, splits, note="", **ref_kw):
    out_d, mass_d = got
    N, V, U = news.shape[1], news.shape[0], user.shape[0]
    out, A, mass, M, n, C, G = _reference(news, user, tau, hkw, **ref_kw)
    kr, km = kappas(N, V, U, splits, n, C, G)
    o, m = out_d.double().cpu().numpy(), mass_d.double().cpu().numpy()
    assert np.isfinite(o).all() and np.isfinite(m).all(), note
    ratio = float((np.abs(o - out) / (kr * EPS * A)).max())
    mratio = float((np.abs(m - mass) / (km * EPS * M)).max())
    print(f"expect_news_affine {note}: N={N} V={V} U={U} splits={splits} worst |err| / bound = {ratio:.4f}, mass {mratio:.4f}")
    assert ratio <= 1.0, (note, ratio)
    assert mratio <= 1.0, (note, mratio)
    return ratio, mratio


def _affine(news, user, tau, splits=0, alpha=None, beta=None, named=None, scale=False, base=None, **kw):
    base = ops.score_logz(news, user, tau, **kw) if base is None else base
    return ops._score_expect_news_affine("score_expect_news_affine", news, user, tau, base, kw.get("exclude"), splits, kw.get("prior"),
                                         kw.get("stamp"), kw.get("window"), alpha, beta, named, scale)


def _everything(N, V, U):
    """Pools with -inf and NaN priors and an empty window, lists, a NaN news row, a user with an infinite component, per-user
    temperatures, named terms with repeats, fill entries and one news named by everybody."""
    g = torch.Generator().manual_seed(101 + N + V)
    news, user = EN._vectors(N, V, U, seed=23)
    if V > 4:
        news[V // 3, N // 2] = NAN
    if U > 8:
        user[7, N - 1] = INF
    tau = (0.3 + torch.rand(U, generator=g)).to(DEV)
    alpha, beta = torch.randn(U, generator=g).to(DEV), torch.randn(U, generator=g).to(DEV)
    pools = EN._pools(V, U)
    lt = EN._list_tensor(V, U)
    lists = ops.ExclusionLists(lt, device=DEV)
    targets, gw = EN._named(V, U, 3, seed=7 + V, every=V - 1)
    named = ops._named_by_news(targets, gw, V)
    hkw = dict({k: v.cpu().numpy() for k, v in pools.items()}, exclude=list(lt.numpy()))
    return news, user, tau, alpha, beta, dict(pools, exclude=lists), named, hkw


@pytest.mark.parametrize("N,V,U,splits", EN.SHAPES, ids=lambda v: str(v))
def test_beta_none_is_k18_with_weight_alpha_bit_for_bit(N, V, U, splits):
    news, user = EN._vectors(N, V, U)
    w = torch.randn(U, generator=torch.Generator().manual_seed(N + U)).to(DEV)
    k18 = EN._expect_news(news, user, 0.5, splits=splits, weight=w)
    k18_mass = EN._expect_news(news, user, 0.5, splits=splits, rows=False)[1]
    got = _affine(news, user, 0.5, splits=splits, alpha=w)
    assert torch.equal(_bits(got[0]), _bits(k18[0])) and torch.equal(_bits(got[1]), _bits(k18_mass))
    # alpha None = 1: K18 without a weight; a zero beta array is beta None
    one = _affine(news, user, 0.5, splits=splits)
    plain = EN._expect_news(news, user, 0.5, splits=splits)
    assert torch.equal(_bits(one[0]), _bits(plain[0])) and torch.equal(_bits(one[1]), _bits(plain[1]))
    zero = _affine(news, user, 0.5, splits=splits, alpha=w, beta=torch.zeros(U, device=DEV))
    assert torch.equal(_bits(zero[0]), _bits(got[0]))
    # pools, lists, per-user temperatures, with and without the 1 / tau scale and the named terms
    news, user, tau, alpha, beta, kw, named, _ = _everything(N, V, U)
    base = ops.score_logz(news, user, tau, **kw)
    mass18 = EN._expect_news(news, user, tau, splits=splits, rows=False, base=base, **kw)[1]
    for scale in (False, True):
        for nm in (None, named):
            k18 = EN._expect_news(news, user, tau, splits=splits, named=nm, scale=scale, weight=alpha, base=base, **kw)
            got = _affine(news, user, tau, splits=splits, alpha=alpha, named=nm, scale=scale, base=base, **kw)
            assert torch.equal(_bits(got[0]), _bits(k18[0])), (scale, nm is not None)
            assert torch.equal(_bits(got[1]), _bits(mass18))
    # with a beta the table stays finite and the mass keeps its bits
    full = _affine(news, user, tau, splits=splits, alpha=alpha, beta=beta, named=named, scale=True, base=base, **kw)
    assert torch.isfinite(full[0]).all() and torch.equal(_bits(full[1]), _bits(mass18)) and not full[0][0].any()


def _user_segments(U):
    seg = 128 * math.ceil(U / (128 * 256))
    return math.ceil(U / seg)


# The first five are the shapes the feature was specified with.  Two of them, (36, 294, 33, 2) and (400, 294, 70, 3), name more
# slices than their U has segments of 128 users (splits cuts the USER axis here; the call refuses that, as K18 does): they run with
# the one slice their users allow, and the two shapes after them are the same ones with V and U exchanged, where 294 users give
# the 2 and 3 slices.
BOUND_SHAPES = [(36, 294, 33, 2), (400, 294, 70, 3), (4, 70, U_TWO, 2), (4, 129, 70, 1), (836, 294, 17, 1), (36, 33, 294, 2), (400, 70, 294, 3)]


@pytest.mark.parametrize("N,V,U,splits", BOUND_SHAPES, ids=lambda v: str(v))
def test_rows_within_the_derived_bound(N, V, U, splits):
    splits = min(splits, _user_segments(U))
    news, user, tau, alpha, beta, kw, named, hkw = _everything(N, V, U)
    base = ops.score_logz(news, user, tau, **kw)
    got = _affine(news, user, tau, splits=splits, alpha=alpha, beta=beta, named=named, scale=True, base=base, **kw)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and not got[0][0].any() and float(got[1][0]) == 0.0
    if U > 1000:                                                      # the host reference walks the users one by one: bits only
        k18 = EN._expect_news(news, user, tau, splits=splits, named=named, scale=True, weight=alpha, base=base, **kw)
        same = _affine(news, user, tau, splits=splits, alpha=alpha, named=named, scale=True, base=base, **kw)
        assert torch.equal(_bits(same[0]), _bits(k18[0])) and not torch.equal(_bits(got[0]), _bits(k18[0]))
        return
    _check(news, user, tau, hkw, got, splits, note="pools+lists+named", alpha=alpha, beta=beta, named=named, scale=True)
    # without the 1 / tau scale and the named terms; beta alone (alpha = 0); the plain call of the public function
    _check(news, user, tau, hkw, _affine(news, user, tau, splits=splits, alpha=alpha, beta=beta, base=base, **kw), splits, note="unscaled",
           alpha=alpha, beta=beta)
    zero = torch.zeros(U, device=DEV)
    _check(news, user, tau, hkw, _affine(news, user, tau, splits=splits, alpha=zero, beta=beta, scale=True, base=base, **kw), splits,
           note="beta alone", alpha=zero, beta=beta, scale=True)
    news, user = EN._vectors(N, V, U)
    base = ops.score_logz(news, user, 0.5)
    pub = ops.score_expect_news_affine(news, user, 0.5, base, splits=splits, alpha=alpha, beta=beta)
    _check(news, user, 0.5, {}, pub, splits, note="plain", alpha=alpha, beta=beta)


def test_dead_users_and_bad_coefficients_contribute_nothing():
    N, V, U, splits, T = 36, 130, 70, 1, 2
    news, user = EN._vectors(N, V, U, seed=71)
    pools = EN._pools(V, U)                                            # user 5: an empty window, nothing eligible
    g = torch.Generator().manual_seed(13)
    tau = (0.3 + torch.rand(U, generator=g)).to(DEV)
    tau[[0, 20, 69]] = torch.tensor([0.0, NAN, INF], device=DEV)
    alpha, beta = torch.randn(U, generator=g).to(DEV), torch.randn(U, generator=g).to(DEV)
    targets, gw = EN._named(V, U, T, seed=17, every=V - 2)             # every user is named, the dead ones too
    named = ops._named_by_news(targets, gw, V)
    base = [t.clone() for t in ops.score_logz(news, user, tau, **pools)]
    base[0][7] = NAN                                                   # a NaN base
    base[1][8] = INF                                                   # an infinite one
    hkw = {k: v.cpu().numpy() for k, v in pools.items()}
    bad = [0, 5, 7, 30, 31, 32, 33]                                    # dead users, and live ones with a NaN or infinite alpha or beta
    al_bad, be_bad = alpha.clone(), beta.clone()
    al_bad[[0, 5, 30]] = torch.tensor([NAN, INF, NAN], device=DEV)
    al_bad[31] = -INF
    be_bad[[7, 32, 33]] = torch.tensor([NAN, NAN, INF], device=DEV)
    al_zero, be_zero = alpha.clone(), beta.clone()
    al_zero[bad] = 0.0
    be_zero[bad] = 0.0
    for scale in (True, False):
        got = _affine(news, user, tau, splits=splits, alpha=al_bad, beta=be_bad, named=named, scale=scale, base=base, **pools)
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and not got[0][0].any() and float(got[1][0]) == 0.0
        want = _affine(news, user, tau, splits=splits, alpha=al_zero, beta=be_zero, named=named, scale=scale, base=base, **pools)
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
        _check(news, user, tau, hkw, got, splits, note=f"dead users scale={scale}", alpha=al_bad, beta=be_bad, named=named, scale=scale,
               dead=(7, 8))
    # the bad coefficients do change something: their users' pairs are gone
    clean = _affine(news, user, tau, splits=splits, alpha=alpha, beta=beta, named=named, scale=True, base=base, **pools)
    assert not torch.equal(_bits(clean[0]), _bits(got[0]))
    # nobody at all: zeros, nothing is launched
    o0, m0 = ops.score_expect_news_affine(news, user[:0], 0.5, [b[:0] for b in base])
    assert o0.shape == (V, N) and m0.shape == (V,) and not o0.any() and not m0.any()


@pytest.mark.parametrize("N", [36, 400])
def test_a_rows_bits_depend_on_that_row_alone_at_fixed_splits(N):
    V, U, splits, T = 294, 300, 2, 3
    news, user = EN._vectors(N, V, U, seed=43)
    pools = EN._pools(V, U)
    lt = EN._list_tensor(V, U)
    lists = ops.ExclusionLists(lt, device=DEV)
    targets, gw = EN._named(V, U, T, seed=3, every=V - 1)
    named = ops._named_by_news(targets, gw, V)
    tau = 0.5
    g = torch.Generator().manual_seed(9)
    alpha, beta = torch.randn(U, generator=g).to(DEV), torch.randn(U, generator=g).to(DEV)
    base = ops.score_logz(news, user, tau, exclude=lists, **pools)
    call = lambda nv, kw, ex, nm, s=splits: ops._score_expect_news_affine("score_expect_news_affine", nv, user, tau, base, ex, s, kw["prior"],
                                                                          kw["stamp"], kw["window"], alpha, beta, nm, True)
    out, mass = call(news, pools, lists, named)
    out2, mass2 = call(news, pools, lists, named)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(mass), _bits(mass2))
    # a permuted table, row 0 fixed: new row i is old row perm[i]; prior, stamp, the lists and the named terms go along, the base stays
    perm = torch.cat([torch.zeros(1, dtype=torch.int64), 1 + torch.randperm(V - 1, generator=torch.Generator().manual_seed(3))])
    inv = torch.empty(V + 3, dtype=torch.int64)
    inv[perm] = torch.arange(V)
    inv[V:] = torch.arange(V, V + 3)                                   # ids >= V stay what they are
    pp = dict(prior=pools["prior"][perm.to(DEV)].contiguous(), stamp=pools["stamp"][perm.to(DEV)].contiguous(), window=pools["window"])
    lists_p = ops.ExclusionLists(inv[lt.long()].to(torch.int32), device=DEV)
    named_p = ops._named_by_news(inv[targets.cpu().long()].to(torch.int32).to(DEV), gw, V)
    outp, massp = call(news[perm.to(DEV)].contiguous(), pp, lists_p, named_p)
    assert torch.equal(_bits(outp), _bits(out[perm.to(DEV)])) and torch.equal(_bits(massp), _bits(mass[perm.to(DEV)]))
    # every other news row overwritten with noise: a chosen row keeps its bits
    for v in (1, 31, 32, 150, V - 1):
        noise = torch.randn(V, N, generator=torch.Generator().manual_seed(v)).to(DEV)
        noise[v] = news[v]
        outn, massn = call(noise, pools, lists, named)
        assert torch.equal(_bits(outn[v]), _bits(out[v])) and torch.equal(_bits(massn[v]), _bits(mass[v])), v
    # another slicing: within the bound of each
    hkw = dict({k: v.cpu().numpy() for k, v in pools.items()}, exclude=list(lt.numpy()))
    _check(news, user, tau, hkw, call(news, pools, lists, named, 3), 3, note="splits=3", alpha=alpha, beta=beta, named=named, scale=True)


def test_every_cell_of_the_launch_table_is_launched():
    """3 tiles x pool x lists, by the profile labels of the stream; the finalize goes with each."""
    V, U = 40, 9
    want, seen, finals = set(), set(), 0
    for N, TV in ((4, 64), (400, 32), (836, 16)):
        news, user = EN._vectors(N, V, U, seed=N)
        pools = EN._pools(V, U)
        lists = ops.ExclusionLists(EN._list_tensor(V, U), device=DEV)
        beta = torch.full((U,), -1.0, device=DEV)
        for pool in (0, 1):
            for lst in (0, 1):
                kw = dict(pools if pool else {}, **(dict(exclude=lists) if lst else {}))
                base = ops.score_logz(news, user, 0.5, **kw)
                want.add((TV, pool, lst))
                labels = EN._labels(lambda: ops.score_expect_news_affine(news, user, 0.5, base, beta=beta, **kw))
                assert not any(k.startswith("expect_news_stream[") or k.startswith("expect_news_final[") for k in labels)
                for label in labels:
                    if label.startswith("expect_news_affine_stream["):
                        f = dict(kv.split("=") for kv in label[len("expect_news_affine_stream["):-1].split(","))
                        assert (int(f["V"]), int(f["U"]), int(f["N"]), int(f["rows"])) == (V, U, N, 1)
                        seen.add((int(f["TV"]), int(f["pool"]), int(f["lists"])))
                    finals += label.startswith("expect_news_affine_final[")
    assert seen == want and len(want) == 12 and finals == 12


def test_the_existing_calls_are_untouched_by_the_new_ones():
    news, user = EN._vectors(400, 294, 300, seed=47)                  # three segments of users, three of news: splits = 2 cuts both
    kw = EN._pools(294, 300)
    al, be = torch.full((300,), 0.3, device=DEV), torch.full((300,), -1.0, device=DEV)

    def existing():
        base = ops.score_logz(news, user, 0.5, **kw)
        return (base + ops.score_expect_news(news, user, 0.5, base, splits=2, weight=al, **kw)
                + ops.score_expect_affine(news, user, 0.5, base, splits=2, alpha=al, beta=be, **kw) + ops.score_entropy(news, user, 0.5, base, **kw))

    before = existing()
    ops.score_expect_news_affine(news, user, 0.5, before[:3], splits=2, alpha=al, beta=be, **kw)
    ops.score_expect_news_affine(news, user, 0.5, before[:3], **kw)
    for a, b in zip(before, existing()):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("T", [1, 4, 128])
def test_full_softmax_nll_entropy_joint_bits_and_the_table_gradient(T):
    """The setup of test_gpu_entropy.test_full_softmax_nll_entropy_forward_bits_and_gradients with the table a leaf.  grad_news is held
    to the K25 bound carried through, as that test carries K24's through for the user side: kappa'' e A_vc(alpha*, beta) for the
    contraction and the named terms; the error of alpha = fl32(sum_t g_t - h H) -- |h| times the bound of H, and e |alpha*| -- on
    sum_u p*_uv |user_uc| / tau; and 2 e on everything that was added up."""
    N, V, U, tau = 36, 294, 33, 0.7
    news, user = GE._vectors(N, V, U, seed=53)
    g = torch.Generator().manual_seed(59 + T)
    prior = 0.3 * torch.randn(V, generator=g)
    prior[11] = -INF
    raw = GE._raw_lists(V, U)
    raw[2] = torch.arange(1, 40)
    lists = ops.ExclusionLists(raw, device=DEV)
    targets = torch.randint(1, V, (U, T), generator=g, dtype=torch.int32)
    targets[3] = 0                                                    # a user whose targets are all fill ...
    targets[5] = 11                                                   # ... and one whose targets are all outside the pool
    if T > 1:
        targets[::3, 1] = 0
        targets[1::4, 2 % T] = 11
        targets[::5, T - 1] = V + 2
    targets = targets.to(DEV)
    kw = dict(exclude=lists, prior=prior.to(DEV))
    gup, hup = torch.randn(U, T, generator=g).to(DEV), torch.randn(U, generator=g).to(DEV)
    hup[7] = 0.0

    # the frozen-table function, and the joint one with every input a leaf: the same forward, grad_user and grad_tau, bit for bit
    tp0, uv0 = torch.nn.Parameter(torch.full((U,), tau, device=DEV)), user.clone().requires_grad_(True)
    nll0, valid0, ent0 = ops.full_softmax_nll_entropy(news, uv0, targets, tp0, splits=2, **kw)
    (nll0 * gup).sum().add((ent0 * hup).sum()).backward()
    tp, uv, nv = torch.nn.Parameter(torch.full((U,), tau, device=DEV)), user.clone().requires_grad_(True), news.clone().requires_grad_(True)
    nll, valid, ent, count = ops.full_softmax_nll_entropy_joint(nv, uv, targets, tp, splits=2, return_count=True, **kw)
    assert torch.equal(valid, valid0) and not valid.requires_grad and not count.requires_grad and count.dtype == torch.int32
    assert torch.equal(_bits(nll), _bits(nll0)) and torch.equal(_bits(ent), _bits(ent0))
    (nll * gup).sum().add((ent * hup).sum()).backward()
    assert torch.equal(_bits(uv.grad), _bits(uv0.grad)) and torch.equal(_bits(tp.grad), _bits(tp0.grad))
    grad = nv.grad
    assert grad.shape == (V, N) and torch.isfinite(grad).all()

    # the float64 autograd gradient of the dense statement with respect to the table
    a64, u64 = news.double().cpu().requires_grad_(True), user.double().cpu()
    s = u64 @ a64.T + torch.where(torch.isneginf(prior), torch.zeros_like(prior), prior).double()[None, :]
    ok = torch.ones(U, V, dtype=torch.bool)
    ok[:, 0] = False
    ok[:, torch.isneginf(prior)] = False
    for u in range(U):
        ok[u, raw[u][(raw[u] >= 1) & (raw[u] < V)]] = False
    z = s / tau
    lp = z - torch.logsumexp(torch.where(ok, z, torch.full_like(z, -INF)), dim=1, keepdim=True)
    lpe = torch.where(ok, lp, torch.zeros_like(lp))
    Hs = -(torch.where(ok, lp.exp(), torch.zeros_like(lp)) * lpe).sum(dim=1)
    vc, tc, gc, hc = valid0.cpu(), targets.cpu().long().clamp(0, V - 1), gup.double().cpu(), hup.double().cpu()
    gw = torch.where(vc, gc, torch.zeros_like(gc))
    picked = torch.where(vc, lp.gather(1, tc), torch.zeros(U, T, dtype=torch.float64))
    (-(picked * gw).sum() + (hc * Hs).sum()).backward()
    want = a64.grad.numpy()

    # the bound
    hkw = dict(exclude=[r.numpy() for r in raw], prior=prior.numpy())
    n_u, C_u, G_u = GE._stats(news, user, tau, **hkw)
    Hn, varn, _ = metrics.entropy_reference(news.double().cpu().numpy(), user.double().cpu().numpy(), tau, **hkw)
    bH, _ = GH.entropy_bounds(N, V, n_u, C_u, G_u, Hn, varn)
    gwn, hn = gw.numpy(), hc.numpy()
    alpha = gwn.sum(axis=1) - hn * Hn
    named = ops._named_by_news(targets, torch.where(valid, gup, torch.zeros_like(gup)), V)
    ref, A, _, _, n, C, G = _reference(news, user, tau, hkw, alpha=torch.from_numpy(alpha), beta=torch.from_numpy(-hn), named=named, scale=True)
    np.testing.assert_allclose(ref, want, rtol=1e-9, atol=1e-11)      # the reference on the exact alpha is the autograd gradient
    p, _ = metrics.softmax_matrix_reference(news.double().cpu().numpy(), user.double().cpu().numpy(), temperature=tau, **hkw)
    carried = p.T @ (((np.abs(hn) * bH + EPS * np.abs(alpha)) / tau)[:, None] * np.abs(user.double().cpu().numpy()))
    bound = kappas(N, V, U, 0, n, C, G)[0] * EPS * A + carried + 2 * EPS * A
    err = np.abs(grad.double().cpu().numpy() - want)
    print(f"full_softmax_nll_entropy_joint T={T}: worst |grad_news err| / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    # news that are eligible for nobody and named by nobody: exactly zero rows
    assert not grad[0].any() and not grad[11].any() and grad[40:].abs().sum(dim=1).gt(0).all()

    # no entropy gradient: full_softmax_nll_joint's gradients, bit for bit
    uj, nj = user.clone().requires_grad_(True), news.clone().requires_grad_(True)
    ops.full_softmax_nll_joint(nj, uj, targets, tau, splits=2, **kw)[0].backward(gup)
    ue, ne = user.clone().requires_grad_(True), news.clone().requires_grad_(True)
    ops.full_softmax_nll_entropy_joint(ne, ue, targets, tau, splits=2, **kw)[0].backward(gup)
    assert torch.equal(_bits(ne.grad), _bits(nj.grad)) and torch.equal(_bits(ue.grad), _bits(uj.grad))

    def sides(news_grad, user_grad, tau_grad):
        a, b = news.clone().requires_grad_(news_grad), user.clone().requires_grad_(user_grad)
        t = torch.full((U,), tau, device=DEV).requires_grad_(tau_grad)
        o, _, e = ops.full_softmax_nll_entropy_joint(a, b, targets, t, splits=2, **kw)
        (o * gup).sum().add((e * hup).sum()).backward()
        return a.grad, b.grad, t.grad

    res = {}
    only_user = EN._labels(lambda: res.update(u=sides(False, True, False)))
    only_news = EN._labels(lambda: res.update(n=sides(True, False, False)))
    only_tau = EN._labels(lambda: res.update(t=sides(False, False, True)))
    assert any(k.startswith("affine_stream[") for k in only_user) and not any(k.startswith("expect_news") for k in only_user)
    assert any(k.startswith("expect_news_affine_stream[") for k in only_news) and any(k.startswith("expect_news_affine_final[") for k in only_news)
    assert not any(k.startswith("affine_stream[") or k.startswith("affine_final[") or k.startswith("expect_news_stream[") for k in only_news)
    assert not any(k.startswith("affine_") or k.startswith("expect_") for k in only_tau)
    assert res["u"][0] is None and res["u"][2] is None and torch.equal(_bits(res["u"][1]), _bits(uv.grad))
    assert res["n"][1] is None and res["n"][2] is None and torch.equal(_bits(res["n"][0]), _bits(grad))
    assert res["t"][0] is None and res["t"][1] is None and torch.equal(_bits(res["t"][2]), _bits(tp.grad))


def _oracle_loss(tag, cfg, sd, news_vecs, hist, mask, targets, tau, entropy_weight):
    """test_gpu_expect_news._oracle_loss extended by the entropy term: loss = mean nll - entropy_weight * mean H, H the entropy of the
    float64 softmax over the eligible news, the mean over the users with anything eligible.  Returns (loss, n, user-encoder
    gradients, table gradient)."""
    enc = O.nrms_user_encoder if tag.startswith("nrms") else O.naml_user_encoder
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("user_encoder.")}
    table = news_vecs.clone().requires_grad_(True)
    user = enc(table[hist.long()], mask, sdo, cfg).double()
    s = user @ table.double().T / tau
    Ur, Vn = s.shape
    ok = torch.ones(Ur, Vn, dtype=torch.bool)
    ok[:, 0] = False
    clicked = hist.long() * (mask != 0).long()
    ok.scatter_(1, clicked, False)                                    # the clicked history; a masked slot names news 0
    lp = torch.log_softmax(torch.where(ok, s, torch.full_like(s, -INF)), dim=1)
    t = targets.long()
    valid = (t >= 1) & ok.gather(1, t)
    first = torch.ones_like(valid)
    for j in range(1, t.shape[1]):
        first[:, j] = ~(t[:, j:j + 1] == t[:, :j]).any(dim=1)
    valid &= first
    assert ok.any(dim=1).all()
    H = -(torch.where(ok, lp.exp() * torch.where(ok, lp, torch.zeros_like(lp)), torch.zeros_like(lp))).sum(dim=1)
    loss = -(torch.where(valid, lp.gather(1, t), torch.zeros_like(s[:, :t.shape[1]]))).sum() / valid.sum() - entropy_weight * H.mean()
    loss.backward()
    return loss.detach(), int(valid.sum()), {k: v.grad for k, v in sdo.items() if v.grad is not None}, table.grad


def _encoder_grads(model):
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("tag", ["nrms_tiny_mask", "naml_tiny_3view"])
def test_full_softmax_loss_entropy_joint_on_the_tiny_models(tag):
    model, cfg, sd, news_vecs, hist, mask, targets = EN._tiny_case(tag)
    tau = 0.7
    args = (hist.numpy(), mask.numpy(), targets.numpy())
    # entropy_weight = 0: full_softmax_loss_joint's loss and user-encoder gradients bit for bit; the table gradient within that
    # file's tolerance (news_gather's atomics decide its last bits)
    t0 = news_vecs.to(DEV).requires_grad_(True)
    loss0, n0 = TR.full_softmax_loss_joint(model, t0, *args, tau)
    loss0.backward()
    want = _encoder_grads(model)
    model.zero_grad(set_to_none=True)
    t1 = news_vecs.to(DEV).requires_grad_(True)
    loss1, n1, mean_h = TR.full_softmax_loss_entropy_joint(model, t1, *args, tau, 0.0)
    loss1.backward()
    got = _encoder_grads(model)
    assert int(n1) == int(n0) and torch.equal(_bits(loss1.detach()), _bits(loss0.detach())) and not mean_h.requires_grad
    assert set(got) == set(want) and len(want) >= 4
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    assert_close(t1.grad, t0.grad, 1e-6, 2e-4, name="dtable at weight 0")
    model.zero_grad(set_to_none=True)
    # a bonus of 0.1 against the float64 oracle
    table = news_vecs.to(DEV).requires_grad_(True)
    loss, n, mean_h = TR.full_softmax_loss_entropy_joint(model, table, *args, tau, 0.1)
    loss_b, n_b, mean_b = TR.full_softmax_loss_entropy_joint(model, table, *args, tau, 0.1, batch_size=5)
    assert int(n_b) == int(n)
    assert_close(loss_b, loss, 1e-5, name="loss in batches")
    loss.backward()
    lo, no, go, gt = _oracle_loss(tag, cfg, sd, news_vecs, hist, mask, targets, tau, 0.1)
    frozen, n_f, mean_f = TR.full_softmax_loss_entropy(model, news_vecs.to(DEV), *args, tau, 0.1)
    assert no == int(n) == int(n_f) and torch.equal(_bits(loss.detach()), _bits(frozen.detach())) and torch.equal(_bits(mean_h), _bits(mean_f))
    assert_close(loss, lo, 1e-4, name="loss vs oracle")
    checked = 0
    for name, p in model.named_parameters():
        if not name.startswith("user_encoder.") or not p.requires_grad:
            assert p.grad is None or not p.grad.any(), name
            continue
        if name not in go:                                            # pad_doc under user_log_mask=True: unused in both
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert_close(p.grad, go[name], 1e-6, 2e-4, name="d" + name)
        checked += 1
    assert checked >= 4
    assert_close(table.grad, gt, 1e-6, 2e-4, name="dtable")           # the softmax path plus the history path
    assert not table.grad[0].any() and float(gt.abs().max()) > 0
    model.zero_grad(set_to_none=True)
    # an nn.Parameter temperature: a finite gradient, full_softmax_loss_entropy's on the detached table
    temp_f, temp_j = torch.nn.Parameter(torch.tensor(tau, device=DEV)), torch.nn.Parameter(torch.tensor(tau, device=DEV))
    TR.full_softmax_loss_entropy(model, news_vecs.to(DEV), *args, temp_f, 0.1)[0].backward()
    model.zero_grad(set_to_none=True)
    TR.full_softmax_loss_entropy_joint(model, news_vecs.to(DEV).requires_grad_(True), *args, temp_j, 0.1)[0].backward()
    assert math.isfinite(float(temp_j.grad)) and float(temp_j.grad) != 0.0 and torch.equal(_bits(temp_j.grad), _bits(temp_f.grad))


def test_three_adam_steps_on_the_table_alone_with_a_bonus_lower_the_loss():
    model, cfg, sd, news_vecs, hist, mask, targets = EN._tiny_case("nrms_tiny_mask")
    table = news_vecs.to(DEV).requires_grad_(True)
    for p in model.parameters():
        p.requires_grad_(False)
    opt = torch.optim.Adam([table], lr=1e-2)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _, _ = TR.full_softmax_loss_entropy_joint(model, table, hist.numpy(), mask.numpy(), targets.numpy(), 0.7, 0.1)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[3] < losses[0] and all(math.isfinite(x) for x in losses), losses

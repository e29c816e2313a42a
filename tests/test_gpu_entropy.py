"""GPU: the entropy of the served distribution, its gradient and the training loss built on them (nr_score_entropy,
nr_score_expect_affine; ops.score_entropy / ops.score_expect_affine / ops.full_softmax_nll_entropy; train.policy_entropy /
train.full_softmax_loss_entropy; include/nrhip.h, K23 and K24).  The device is held to bounds DERIVED from its order of operations
(kappa_x, kappa_affine below) against metrics.entropy_reference / metrics.expect_affine_reference in float64 on
the fp32 inputs; bit statements where the contract makes them.  The shapes, pools and lists are test_gpu_expect's."""
import math

import numpy as np
import pytest
import torch

import test_gpu_expect as GE
from newsrecommendation_amd import metrics, ops, train as TR

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
EPS = GE.EPS
V_TWO = GE.V_TWO
DEV = "cuda"


def kappa_x(N, V, n, C, G):
    """x = log p carries the ABSOLUTE error kappa_x e (first order in e = 2^-24):
      score chain   (N + 1) G e on s / tau (N fma roundings and the prior's add) and as much on log Z: 2 (N + 1) G
      exponent      fl(s - max), fl(1 / tau), each e on |s - max| / tau <= 2 C; the fma's rounding e on |x| <= 2 C + ln n: 6 C + ln n
      base          the logsum of K13 with its own bound 4 ln n + 7 K + 14, K = 2 seg / 128
    Sum: 2 (N + 1) G + 6 C + 5 ln n + 7 K + 14."""
    seg, _ = GE._plan(V, 1)
    return 2.0 * (N + 1) * G + 6.0 * C + 5.0 * np.log(np.maximum(n, 2)) + 7.0 * (2 * seg // 128) + 14.0


def entropy_bounds(N, V, n, C, G, H, var):
    """(bound of H, bound of var).  p = expf(x) is within (kappa_x + 6) e of p* relatively (expf: 3 ulp), so
    |p x - p* x*| <= p* ((kappa_x + 6) |x*| + kappa_x) e; summed (fp64 chains: nothing at this order), one rounding to fp32 (e H*) and
    e for the second order: |H - H*| <= ((kappa_x + 8) H* + kappa_x + 1) e.  Likewise |p x^2 - p* x*^2| <= p* ((kappa_x + 6) x*^2 +
    2 kappa_x |x*|) e and |m1^2 - m1*^2| <= 2 H* ((kappa_x + 6) H* + kappa_x) e:
    |var - var*| <= ((kappa_x + 8) (m2* + 2 H*^2) + 4 kappa_x H* + 1) e.  A weight below the normal range (x < -87) is lost at no more than
    2^-126 |x| (|x| < 128) resp. 2^-126 x^2 (< 2^14) each: n 2^-119 and n 2^-112."""
    kx = kappa_x(N, V, n, C, G)
    m2 = var + H * H
    return ((kx + 8.0) * H + kx + 1.0) * EPS + n * 2.0 ** -119, ((kx + 8.0) * (m2 + 2.0 * H * H) + 4.0 * kx * H + 1.0) * EPS + n * 2.0 ** -112


def kappa_affine(N, V, splits, n, C, G):
    """K17's kappa + 2: r = p fl(fma(beta, x, alpha)) adds the fma's rounding and the product's, e (|alpha| + |beta| |x*|) each, and the
    error of x enters the weight as |beta| kappa_x e -- the `+ 1` beside |x*| in A_c (kappa_x <= kappa')."""
    return GE.kappa(N, V, splits, n, C, G) + 2.0


def _host(kw):
    return {k: ([r.numpy() for r in v] if k == "exclude" else v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


def _tau_np(tau):
    return tau.double().cpu().numpy() if isinstance(tau, torch.Tensor) else tau


def _entropy(news, user, tau, splits=0, **kw):
    base = ops.score_logz(news, user, tau, **kw)
    return ops.score_entropy(news, user, tau, base, splits=splits, **kw)


def _check_entropy(news, user, tau, hkw, got, note=""):
    """H, var and mass of `got` against the reference within the derived bounds; returns the worst ratios."""
    Hd, vd, md = (t.double().cpu().numpy() for t in got)
    N, V = news.shape[1], news.shape[0]
    H, var, M = metrics.entropy_reference(news.double().cpu().numpy(), user.double().cpu().numpy(), _tau_np(tau), **hkw)
    n, C, G = GE._stats(news, user, _tau_np(tau), **hkw)
    nan = np.isnan(M)
    assert np.array_equal(np.isnan(Hd), nan) and np.array_equal(np.isnan(vd), nan) and np.array_equal(np.isnan(md), nan), note
    live = ~nan
    bH, bV = entropy_bounds(N, V, n, C, G, np.where(live, H, 0.0), np.where(live, var, 0.0))
    bM = GE.kappa_mass(V, n, C) * EPS
    rH = float((np.abs(Hd - H)[live] / bH[live]).max()) if live.any() else 0.0
    rV = float((np.abs(vd - var)[live] / bV[live]).max()) if live.any() else 0.0
    rM = float((np.abs(md - M)[live] / bM[live]).max()) if live.any() else 0.0
    print(f"entropy {note}: N={N} V={V} U={user.shape[0]} worst |err| / bound: H {rH:.4f}, var {rV:.4f}, mass {rM:.4f}")
    assert rH <= 1.0 and rV <= 1.0 and rM <= 1.0, (note, rH, rV, rM)
    empty = live & (n == 0)
    assert not Hd[empty].any() and not vd[empty].any() and not md[empty].any(), note
    single = live & (n == 1)
    assert not Hd[single].any() and not vd[single].any() and (md[single] == 1.0).all(), note
    return rH, rV, rM


@pytest.mark.parametrize("N,V,U,splits", GE.SHAPES, ids=lambda v: str(v))
def test_plain_entropy_within_the_derived_bounds(N, V, U, splits):
    news, user = GE._vectors(N, V, U)
    _check_entropy(news, user, 0.5, {}, _entropy(news, user, 0.5, splits=splits), note="plain")


@pytest.mark.parametrize("N,V,U,splits", [(36, 294, 33, 2), (400, 294, 70, 3), (400, V_TWO, 17, 0), (4, 129, 70, 1), (836, 294, 17, 1)],
                         ids=lambda v: str(v))
def test_pools_lists_and_a_nan_row_within_the_derived_bounds(N, V, U, splits):
    news, user = GE._vectors(N, V, U, seed=23)
    news[V // 3, N // 2] = NAN                                        # a NaN news row: weight 0 for everybody, nobody's result is NaN
    pools = GE._pools(V, U)
    raw = GE._raw_lists(V, U)
    lists = ops.ExclusionLists(raw, device=DEV)
    for note, kw in (("pools", pools), ("lists", dict(exclude=lists)), ("both", dict(pools, exclude=lists))):
        got = _entropy(news, user, 0.5, splits=splits, **kw)
        hkw = _host({k: (raw if k == "exclude" else v) for k, v in kw.items()})
        _check_entropy(news, user, 0.5, hkw, got, note=note)
        assert all(torch.isfinite(t).all() for t in got)


def test_exact_statements():
    N, V, U = 36, 294, 33
    news, user = GE._vectors(N, V, U, seed=29)
    # exactly one eligible news (everything but id 7 is listed; user 3 lists everything): H == 0 and var == 0 exactly
    raw = [torch.tensor([v for v in range(1, V) if v != 7]) for _ in range(U)]
    raw[3] = torch.arange(1, V)
    H, var, mass = _entropy(news, user, 0.5, splits=2, exclude=ops.ExclusionLists(raw, device=DEV))
    assert not H.any() and not var.any() and not torch.signbit(H).any()
    keep = [u for u in range(U) if u != 3]
    assert (mass[keep] == 1.0).all() and mass[3] == 0.0
    # bad tau_u entries: NaN for that user, every other user's bits unchanged
    g = torch.Generator().manual_seed(13)
    tau = (0.05 + torch.rand(U, generator=g)).to(DEV)
    good = _entropy(news, user, tau, splits=2)
    _check_entropy(news, user, tau, {}, good, note="tau_u")
    bad = tau.clone()
    at = [0, 20, 32]
    bad[at] = torch.tensor([0.0, NAN, INF], device=DEV)
    got = _entropy(news, user, bad, splits=2)
    keep = [u for u in range(U) if u not in at]
    for a, b in zip(got, good):
        assert torch.isnan(a[at]).all() and torch.equal(a[keep].view(torch.int32), b[keep].view(torch.int32))
    # a NaN base: that user alone
    base = [t.clone() for t in ops.score_logz(news, user, tau)]
    base[0][7] = NAN
    nb = ops.score_entropy(news, user, tau, base, splits=2)
    for a, b in zip(nb, good):
        assert torch.isnan(a[7]) and torch.equal(a[8:].view(torch.int32), b[8:].view(torch.int32))
    assert ops.score_entropy(news, user[:0], 0.5, [b[:0] for b in base])[0].shape == (0,)


@pytest.mark.parametrize("N", [36, 400])
def test_flat_and_peaked_scores(N):
    V, U = 294, 17
    news, user = GE._vectors(N, V, U, seed=31)
    # flat: all-zero user vectors, no prior: p = 1 / n, H = ln n, var = 0
    flat = torch.zeros_like(user)
    got = _entropy(news, flat, 0.5, splits=1)
    _check_entropy(news, flat, 0.5, {}, got, note="flat")
    n = V - 1
    bH, bV = entropy_bounds(N, V, np.float64(n), 0.0, 0.0, math.log(n), 0.0)
    assert (np.abs(got[0].double().cpu().numpy() - math.log(n)) <= bH).all() and (np.abs(got[1].double().cpu().numpy()) <= bV).all()
    # peaked: tau = 1e-3 of the score spread, most x below -87 (expf underflows): finite results, no NaN, inside the bounds
    scores = user.double() @ news.double().T
    spread = float((scores[:, 1:].max(dim=1).values - scores[:, 1:].min(dim=1).values).min())
    tau = 1e-3 * spread
    x = (scores[:, 1:] - scores[:, 1:].max(dim=1, keepdim=True).values) / tau
    assert float((x < -87.0).double().mean()) > 0.5
    got = _entropy(news, user, tau, splits=3)
    assert all(torch.isfinite(t).all() for t in got)
    _check_entropy(news, user, tau, {}, got, note="peaked")


def _affine(news, user, tau, splits, alpha=None, beta=None, **kw):
    base = ops.score_logz(news, user, tau, **kw)
    return base, ops.score_expect_affine(news, user, tau, base, splits=splits, alpha=alpha, beta=beta, **kw)


@pytest.mark.parametrize("N,V,U,splits", GE.SHAPES, ids=lambda v: str(v))
def test_affine_with_ones_and_zeros_is_score_expect_bit_for_bit(N, V, U, splits):
    splits = max(splits, 1)                                           # an explicit slice count: the statement is made at one
    news, user = GE._vectors(N, V, U, seed=61)
    ones, zeros = torch.ones(U, device=DEV), torch.zeros(U, device=DEV)
    cases = [{}]
    if V > 2:
        cases.append(dict(GE._pools(V, U), exclude=ops.ExclusionLists(GE._raw_lists(V, U), device=DEV)))
    for kw in cases:
        base, (out, mass) = _affine(news, user, 0.5, splits, alpha=ones, beta=zeros, **kw)
        e, m = ops.score_expect(news, user, 0.5, base, splits=splits, **kw)
        assert torch.equal(out.view(torch.int32), e.view(torch.int32)) and torch.equal(mass.view(torch.int32), m.view(torch.int32))
        out0, mass0 = ops.score_expect_affine(news, user, 0.5, base, splits=splits, **kw)      # None, None = (1, 0)
        assert torch.equal(out0.view(torch.int32), e.view(torch.int32)) and torch.equal(mass0.view(torch.int32), m.view(torch.int32))


def _affine_reference(news, user, tau, alpha, beta, hkw):
    """(out*, A, Aabs) in float64: the table widened by |news| and the users by zeros (zero columns change no score); on the |news|
    half the weights alpha' = |alpha| + |beta|, beta' = -|beta| give A_c = sum p* (|alpha| + |beta| (|x*| + 1)) |news_vc| (x* <= 0), and
    (1, 0) gives sum p* |news_vc|."""
    a, b = news.double().cpu().numpy(), user.double().cpu().numpy()
    N = a.shape[1]
    wide, wuser = np.concatenate([a, np.abs(a)], axis=1), np.concatenate([b, np.zeros_like(b)], axis=1)
    out, mass = metrics.expect_affine_reference(wide, wuser, tau, alpha=alpha, beta=beta, **hkw)
    A, _ = metrics.expect_affine_reference(wide, wuser, tau, alpha=np.abs(alpha) + np.abs(beta), beta=-np.abs(beta), **hkw)
    Aabs, _ = metrics.expect_affine_reference(wide, wuser, tau, **hkw)
    return out[:, :N], A[:, N:], Aabs[:, N:], mass


@pytest.mark.parametrize("N,V,U,splits", [(36, 294, 33, 2), (400, 294, 70, 3), (400, V_TWO, 17, 1), (4, 129, 70, 1), (836, 294, 17, 2)],
                         ids=lambda v: str(v))
def test_affine_rows_within_the_derived_bound(N, V, U, splits):
    news, user = GE._vectors(N, V, U, seed=67)
    g = torch.Generator().manual_seed(71)
    tau = (0.3 + torch.rand(U, generator=g)).to(DEV)
    raw = GE._raw_lists(V, U)
    kw = dict(GE._pools(V, U), exclude=ops.ExclusionLists(raw, device=DEV))
    hkw = _host(dict(kw, exclude=raw))
    tau_np = _tau_np(tau)
    n, C, G = GE._stats(news, user, tau_np, **hkw)
    kap = kappa_affine(N, V, splits, n, C, G)
    big = float(news.abs().max())
    H = ops.score_entropy(news, user, tau, ops.score_logz(news, user, tau, **kw), splits=splits, **kw)[0]
    beta = torch.randn(U, generator=g).to(DEV)
    for note, alpha in (("signed", torch.randn(U, generator=g).to(DEV)), ("centred", torch.nan_to_num(H * beta))):   # alpha = H beta: the row sums nearly cancel
        _, (out, mass) = _affine(news, user, tau, splits, alpha=alpha, beta=beta, **kw)
        al, be = alpha.double().cpu().numpy(), beta.double().cpu().numpy()
        want, A, _, M = _affine_reference(news, user, tau_np, al, be, hkw)
        bound = kap[:, None] * EPS * A + (n * 2.0 ** -126 * big * (np.abs(al) + 128.0 * np.abs(be)))[:, None]
        err = np.abs(out.double().cpu().numpy() - want)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print(f"affine {note}: N={N} V={V} U={U} splits={splits} worst |err| / bound = {ratio:.4f}")
        assert (err <= bound).all(), (note, ratio)
        assert (np.abs(mass.double().cpu().numpy() - M) <= GE.kappa_mass(V, n, C) * EPS).all()
        assert not out[torch.from_numpy(n == 0).to(DEV)].any()
    # named rows and 1 / tau: fl32(1 / tau) and the one rounding of the finished row, 2 e on everything that was added up
    T = 5
    ids = torch.randint(1, V, (U, T), generator=g, dtype=torch.int32)
    ids[:, 1] = 0
    ids[::2, 2] = V + 3
    ids[:, 4] = ids[:, 0]
    sw = torch.randn(U, T, generator=g)
    ids, sw = ids.to(DEV), sw.to(DEV)
    base = ops.score_logz(news, user, tau, **kw)
    out, _ = ops.score_expect_affine(news, user, tau, base, splits=splits, alpha=alpha, beta=beta, sub_ids=ids, sub_w=sw, scale_inv_tau=True, **kw)
    full, _ = metrics.expect_affine_reference(news.double().cpu().numpy(), user.double().cpu().numpy(), tau_np, alpha=al, beta=be,
                                              sub_ids=ids.cpu().numpy(), sub_w=sw.double().cpu().numpy(), scale_inv_tau=True, **hkw)
    real = ((ids >= 1) & (ids < V)).cpu().numpy()
    rows = np.abs(np.where(np.isfinite(news.cpu().numpy()), news.double().cpu().numpy(), 0.0))[np.where(real, ids.cpu().numpy(), 0)]
    sub_abs = (np.where(real, np.abs(sw.double().cpu().numpy()), 0.0)[:, :, None] * rows).sum(axis=1)
    bound = (bound + 2 * EPS * (A + sub_abs)) / tau_np[:, None]
    err = np.abs(out.double().cpu().numpy() - full)
    print(f"affine named rows: worst |err| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
    assert (err <= bound).all()
    # a NaN in a user's alpha or beta: that user's row, nobody else's
    alpha_n, beta_n = alpha.clone(), beta.clone()
    ua, ub = (int(u) for u in np.flatnonzero(n > 0)[[0, -1]])
    alpha_n[ua], beta_n[ub] = NAN, NAN
    clean, _ = ops.score_expect_affine(news, user, tau, base, splits=splits, alpha=alpha, beta=beta, **kw)
    dirty, _ = ops.score_expect_affine(news, user, tau, base, splits=splits, alpha=alpha_n, beta=beta_n, **kw)
    keep = [u for u in range(U) if u not in (ua, ub)]
    assert ua != ub and torch.isnan(dirty[ua]).all() and torch.isnan(dirty[ub]).all()
    assert torch.equal(dirty[keep].view(torch.int32), clean[keep].view(torch.int32))


def test_results_do_not_depend_on_the_other_users_at_fixed_splits():
    for N, V in ((36, 294), (400, V_TWO)):
        U = 70
        news, user = GE._vectors(N, V, U, seed=43)
        kw = dict(exclude=ops.ExclusionLists(GE._raw_lists(V, U), device=DEV), **GE._pools(V, U))
        tau = 0.5
        g = torch.Generator().manual_seed(7)
        alpha, beta = torch.randn(U, generator=g).to(DEV), torch.randn(U, generator=g).to(DEV)
        base = ops.score_logz(news, user, tau, **kw)

        def both(rows):
            kwr = kw if rows is None else dict(kw, exclude=kw["exclude"].take(rows), window=kw["window"][rows].contiguous())
            pick = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
            b = [pick(t) for t in base]
            return (ops.score_entropy(news, pick(user), tau, b, splits=2, **kwr)
                    + ops.score_expect_affine(news, pick(user), tau, b, splits=2, alpha=pick(alpha), beta=pick(beta), **kwr))

        full = both(None)
        for a, b in zip(full, both(None)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        perm = torch.randperm(U, generator=torch.Generator().manual_seed(3)).to(DEV)
        for a, b in zip(full, both(perm)):
            assert torch.equal(b.view(torch.int32), a[perm].view(torch.int32))
        for u in (0, 1, 17, 40, 69):
            one = torch.tensor([u], device=DEV)
            for a, b in zip(full, both(one)):
                assert torch.equal(b.view(torch.int32), a[one].view(torch.int32))
        # another slicing: within the bounds of each
        hkw = _host(dict(kw, exclude=GE._raw_lists(V, U)))
        _check_entropy(news, user, tau, hkw, ops.score_entropy(news, user, tau, base, splits=3, **kw), note="splits=3")


def test_score_logz_and_score_expect_are_untouched_by_the_new_calls():
    news, user = GE._vectors(400, 294, 70, seed=47)
    kw = GE._pools(294, 70)
    before = ops.score_logz(news, user, 0.5, **kw)
    e_before = ops.score_expect(news, user, 0.5, before, splits=2, **kw)
    ops.score_entropy(news, user, 0.5, before, **kw)
    ops.score_expect_affine(news, user, 0.5, before, alpha=torch.full((70,), 0.3, device=DEV), beta=torch.full((70,), -1.0, device=DEV), **kw)
    after = ops.score_logz(news, user, 0.5, **kw)
    e_after = ops.score_expect(news, user, 0.5, after, splits=2, **kw)
    for a, b in zip(before + e_before, after + e_after):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("T", [1, 4, 128])
def test_full_softmax_nll_entropy_forward_bits_and_gradients(T):
    """The user gradient is held to the K24 bound carried through: kappa' e A_c(alpha*, beta) for the contraction, the error of
    alpha = fl32(sum_t g_t - h H) -- |h| times the bound of H, and e |alpha*| -- on sum_v p* |news_vc|, and 2 e (fl32(1 / tau), the
    rounding of the finished row) on everything that was added up; all divided by tau.
    The temperature gradient d/dtau = (sum_t g_t (logp_t + H) + h var) / tau is formed in fp64 from the fp32 logp_t (K14), H and var
    (K23).  logp_t is within (kappa_x + |logp*_t| + 1) e of the exact value (the score chains of s_t and log Z, the base's bound -- all
    inside kappa_x -- and its rounding to fp32), H and var within their K23 bounds B_H, B_var, so per user
      |d - d*| <= (sum_t |g_t| ((kappa_x + |logp*_t| + 1) e + B_H) + |h| B_var + 2 e (sum_t |g_t| (|logp*_t| + H*) + |h| var*)) / tau,
    the last term the rounding of the fp32 result (and slack); a 0-dim temperature gets the sum over the users of these bounds."""
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
    nll0, valid0 = ops.full_softmax_nll(news, user.clone().requires_grad_(True), targets, tau, splits=2, **kw)

    # the float64 autograd gradient of the dense statement
    a64, u64 = news.double().cpu(), user.double().cpu().requires_grad_(True)
    t64 = torch.full((U,), tau, dtype=torch.float64, requires_grad=True)
    # (a prior of -inf is outside the pool: 0 in its place, so that no 0 * inf reaches the temperature's gradient)
    s = u64 @ a64.T + torch.where(torch.isneginf(prior), torch.zeros_like(prior), prior).double()[None, :]
    ok = torch.ones(U, V, dtype=torch.bool)
    ok[:, 0] = False
    ok[:, torch.isneginf(prior)] = False
    for u in range(U):
        ok[u, raw[u][(raw[u] >= 1) & (raw[u] < V)]] = False
    z = s / t64[:, None]
    lp = z - torch.logsumexp(torch.where(ok, z, torch.full_like(z, -INF)), dim=1, keepdim=True)
    lpe = torch.where(ok, lp, torch.zeros_like(lp))
    Hs = -(torch.where(ok, lp.exp(), torch.zeros_like(lp)) * lpe).sum(dim=1)
    vc, tc, gc, hc = valid0.cpu(), targets.cpu().long().clamp(0, V - 1), gup.double().cpu(), hup.double().cpu()
    gw = torch.where(vc, gc, torch.zeros_like(gc))
    picked = torch.where(vc, lp.gather(1, tc), torch.zeros(U, T, dtype=torch.float64))
    (-(picked * gw).sum() + (hc * Hs).sum()).backward()
    # the bounds
    hkw = dict(exclude=[r.numpy() for r in raw], prior=prior.numpy())
    n, C, G = GE._stats(news, user, tau, **hkw)
    Hn, varn, _ = metrics.entropy_reference(news.double().cpu().numpy(), user.double().cpu().numpy(), tau, **hkw)
    np.testing.assert_allclose(Hn, Hs.detach().numpy(), rtol=1e-10, atol=1e-12)
    bH, bV = entropy_bounds(N, V, n, C, G, Hn, varn)
    kx = kappa_x(N, V, n, C, G)
    gwn, hn = gw.numpy(), hc.numpy()
    alpha = gwn.sum(axis=1) - hn * Hn
    _, A, Aabs, _ = _affine_reference(news, user, tau, alpha, -hn, hkw)
    rows = np.abs(a64.numpy())[tc.numpy()]                            # [U, T, N]
    sub_abs = (np.abs(gwn)[:, :, None] * rows).sum(axis=1)
    b_user = (kappa_affine(N, V, 2, n, C, G)[:, None] * EPS * A + (np.abs(hn) * bH + EPS * np.abs(alpha))[:, None] * Aabs + 2 * EPS * (A + sub_abs)) / tau
    lpn = np.abs(picked.detach().numpy())
    b_tau = ((np.abs(gwn) * ((kx[:, None] + lpn + 1.0) * EPS + bH[:, None])).sum(axis=1) + np.abs(hn) * bV
             + 2 * EPS * ((np.abs(gwn) * (lpn + Hn[:, None])).sum(axis=1) + np.abs(hn) * varn)) / tau
    live = (vc.any(dim=1) | (hc != 0)).numpy()

    for kind in ("0-dim", "[U]"):
        tp = torch.nn.Parameter(torch.tensor(tau, device=DEV) if kind == "0-dim" else torch.full((U,), tau, device=DEV))
        uv = user.clone().requires_grad_(True)
        nll, valid, ent = ops.full_softmax_nll_entropy(news, uv, targets, tp, splits=2, **kw)
        assert torch.equal(valid, valid0) and not valid.requires_grad and torch.equal(nll.view(torch.int32), nll0.view(torch.int32))
        assert (np.abs(ent.detach().double().cpu().numpy() - Hn) <= bH).all()
        (nll * gup).sum().add((ent * hup).sum()).backward()
        grad = uv.grad
        assert torch.isfinite(grad).all()
        err = np.abs(grad.double().cpu().numpy() - u64.grad.numpy())
        print(f"full_softmax_nll_entropy T={T} tau {kind}: worst |user grad err| / bound = {float((err[live] / b_user[live]).max()):.4f}")
        assert (err[live] <= b_user[live]).all() and not grad.cpu().numpy()[~live].any()
        want_t = t64.grad.numpy()
        if kind == "0-dim":
            et, bt = abs(float(tp.grad) - want_t.sum()), b_tau.sum()
            assert tp.grad.shape == ()
        else:
            et, bt = np.abs(tp.grad.double().cpu().numpy() - want_t), b_tau
            assert tp.grad.shape == (U,) and not tp.grad.cpu().numpy()[~live].any()
        print(f"full_softmax_nll_entropy T={T} tau {kind}: worst |tau grad err| / bound = {float(np.max(et / np.maximum(bt, 1e-300))):.4f}")
        assert np.all(et <= bt)
    # the entropy in no loss: full_softmax_nll's gradient, bit for bit; nothing at all: no gradient
    uv0, uv1 = user.clone().requires_grad_(True), user.clone().requires_grad_(True)
    ops.full_softmax_nll(news, uv0, targets, tau, splits=2, **kw)[0].backward(gup)
    ops.full_softmax_nll_entropy(news, uv1, targets, tau, splits=2, **kw)[0].backward(gup)
    assert torch.equal(uv0.grad.view(torch.int32), uv1.grad.view(torch.int32))


def test_full_softmax_nll_entropy_bad_temperature_entries_contribute_nothing():
    N, V, U, T, tau = 400, 294, 33, 4, 0.7
    news, user = GE._vectors(N, V, U, seed=67)
    targets = torch.randint(1, V, (U, T), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(DEV)
    good = torch.nn.Parameter(torch.full((U,), tau, device=DEV))
    ug = user.clone().requires_grad_(True)
    nll, valid, ent = ops.full_softmax_nll_entropy(news, ug, targets, good, splits=1)
    (nll.sum() + ent.sum()).backward()
    at = [0, 16, 32]
    taus = torch.full((U,), tau, device=DEV)
    taus[at] = torch.tensor([0.0, NAN, INF], device=DEV)
    bad = torch.nn.Parameter(taus)
    ub = user.clone().requires_grad_(True)
    nll_b, valid_b, ent_b = ops.full_softmax_nll_entropy(news, ub, targets, bad, splits=1)
    (nll_b.sum() + torch.nan_to_num(ent_b).sum()).backward()
    keep = [u for u in range(U) if u not in at]
    assert valid.all() and valid_b[keep].all() and not valid_b[at].any() and not nll_b[at].any() and torch.isnan(ent_b[at]).all()
    assert torch.equal(ent_b[keep].view(torch.int32), ent[keep].view(torch.int32))
    assert not ub.grad[at].any() and torch.equal(ub.grad[keep].view(torch.int32), ug.grad[keep].view(torch.int32))
    assert not bad.grad[at].any() and torch.equal(bad.grad[keep].view(torch.int32), good.grad[keep].view(torch.int32))


@pytest.mark.parametrize("tag", ["nrms_tiny_mask", "naml_tiny_3view"])
def test_full_softmax_loss_entropy_on_the_tiny_models(tag):
    model, cfg, sd, news_vecs, hist, mask, targets = GE._tiny_case(tag)
    tau = 0.7
    nv = news_vecs.to(DEV)
    args = (nv, hist.numpy(), mask.numpy(), targets.numpy())
    # entropy_weight = 0: full_softmax_loss's loss and encoder gradients, bit for bit
    loss0, n0 = TR.full_softmax_loss(model, *args, tau)
    loss0.backward()
    want = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    loss, n, mean_h = TR.full_softmax_loss_entropy(model, *args, tau, 0.0)
    loss.backward()
    assert int(n) == int(n0) and torch.equal(loss.view(torch.int32), loss0.view(torch.int32)) and not mean_h.requires_grad
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(want) and len(want) >= 4
    for k in want:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    model.zero_grad(set_to_none=True)
    # policy_entropy against the reference on the user vectors the functions share; batches of users: the same numbers
    ent, var = TR.policy_entropy(model, *args[:3], tau)
    user = TR._recommend_args(model, nv, hist.numpy(), mask.numpy(), True, 8192, None, None, None, None, None, None)[1].detach()
    clicked = [r[r > 0].numpy() for r in (hist.long() * (mask != 0).long())]
    hkw = dict(exclude=clicked)
    Hn, varn, _ = metrics.entropy_reference(nv.double().cpu().numpy(), user.double().cpu().numpy(), tau, **hkw)
    nn_, C, G = GE._stats(nv, user, tau, **hkw)
    bH, bV = entropy_bounds(nv.shape[1], nv.shape[0], nn_, C, G, Hn, varn)
    assert (np.abs(ent.double().cpu().numpy() - Hn) <= bH).all() and (np.abs(var.double().cpu().numpy() - varn) <= bV).all()
    assert abs(float(mean_h) - Hn.mean()) <= bH.mean() + 16 * EPS * Hn.mean()
    _, _, mean_b = TR.full_softmax_loss_entropy(model, *args, tau, 0.1, batch_size=5)
    assert abs(float(mean_b) - float(mean_h)) <= 32 * EPS * Hn.mean() + 2 * bH.mean()
    # a positive weight and a learnable temperature: three Adam steps raise the mean entropy
    temp = torch.nn.Parameter(torch.tensor(tau, device=DEV))
    opt = torch.optim.Adam(list(model.user_encoder.parameters()) + [temp], lr=1e-2)
    seen = []
    for _ in range(4):
        opt.zero_grad()
        loss, _, mean_h = TR.full_softmax_loss_entropy(model, *args, temp, 5.0)
        seen.append(float(mean_h))
        loss.backward()
        assert temp.grad is not None and math.isfinite(float(temp.grad))
        opt.step()
    assert seen[3] > seen[0] and all(math.isfinite(x) for x in seen) and float(temp.detach()) != tau, (seen, float(temp.detach()))

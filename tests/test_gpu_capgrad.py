"""GPU: listwise training under group caps (nr_score_expect_groups, K20; nr_row_logprob_capped_grad, K21; ops.score_expect_groups /
row_logprob_capped_grad / plackett_luce_nll_capped; train.listwise_loss_capped).  K20 and K21 are held to the bounds STATED in
include/nrhip.h (kappa20, kappa21 below; derived in DESIGN.md section 5) against metrics.expect_groups_reference and
metrics.capped_row_logprob_grad_reference in float64 on the fp32 inputs; the finished gradient to the two bounds carried through,
against float64 autograd of the dense capped statement; bit statements where the contract makes them."""
import math

import numpy as np
import pytest
import torch

import test_gpu_listwise as LW
from helpers import assert_close
from newsrecommendation_amd import _lib, metrics, ops, train as TR
from oracle import nr_oracle as O

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
EPS = 2.0 ** -24
DEV = "cuda"
U, G = 70, 6                               # a partial last tile for every user tile; 6 groups, group 3 empty
_bits = LW._bits


def _groups(V):
    """6 groups: group 0 spans five or more chunks (40 % of the news), group 1 holds fewer than 128 news, group 3 is empty, 15 % of
    the news are in no group."""
    v = torch.arange(V)
    r = v % 20
    g = torch.full((V,), -1, dtype=torch.int32)
    g[r < 8] = 0
    g[(r >= 8) & (r < 11)] = 2
    g[(r >= 11) & (r < 14)] = 4
    g[(r >= 14) & (r < 17)] = 5
    g[torch.nonzero(v % 31 == 5)[:50, 0]] = 1
    return g


_FX = {}


def _fx(N, V):
    """One corpus per (N, V), shared and left unchanged: vectors, groups and their order, pools, lists (user 1's covers the whole of
    group 1), temperatures with one bad entry."""
    if (N, V) not in _FX:
        news, user = LW._vectors(N, V, U, seed=5 + N + V)
        group = _groups(V)
        order = ops.GroupOrder(group.to(DEV), n_groups=G)
        assert order.chunks_per_segment == (2 if V > 30000 else 1) and int((group == 3).sum()) == 0 and 0 < int((group == 1).sum()) < 128
        assert int((group == 0).sum()) > 256 and int((group < 0).sum()) > 128
        gen = torch.Generator().manual_seed(N + V)
        lists = [np.unique(torch.randint(1, V, (30,), generator=gen).numpy()) for _ in range(U)]
        lists[1] = np.unique(np.concatenate([lists[1], torch.nonzero(group == 1)[:, 0].numpy()]))
        taus = torch.linspace(0.5, 1.5, U)
        taus[3] = 0.0
        _FX[(N, V)] = dict(N=N, V=V, news=news, user=user, group=group, gdev=group.to(DEV), order=order, pools=LW._pools(V, U, seed=N + 3),
                           lists=lists, taus=taus, a64=news.double().cpu().numpy(), b64=user.double().cpu().numpy())
    return _FX[(N, V)]


def _mode(fx, pool, lists, tauvec):
    """(device kwargs, host kwargs, device exclude, host lists, device tau, host taus [U])"""
    kw, hkw = {}, {}
    if pool:
        for name, t in zip(("prior", "stamp", "window"), fx["pools"]):
            kw[name], hkw[name] = t.to(DEV), t.numpy()
    ex = ops.ExclusionLists(fx["lists"], device=DEV) if lists else None
    lh = fx["lists"] if lists else [np.zeros(0, dtype=np.int64)] * U
    tau = fx["taus"].to(DEV) if tauvec else float(np.float32(0.7))
    th = fx["taus"].double().numpy() if tauvec else np.full(U, float(np.float32(0.7)))
    return kw, hkw, ex, lh, tau, th


def _longest_slice(order, splits):
    """chunks of the longest slice under K15's rule (slice y of s: the segments that start in [y n_pos / s, (y + 1) n_pos / s))"""
    ss, nseg, n_pos = order.seg_start.tolist(), order.nseg, order.n_pos
    if splits == nseg:
        return max(ss[i + 1] - ss[i] for i in range(nseg)) // 128

    def first_from(p):
        return next((i for i in range(nseg) if ss[i] >= p), nseg)
    cuts = [first_from(y * n_pos // splits) for y in range(splits)] + [nseg]
    return max(ss[cuts[y + 1]] - ss[cuts[y]] for y in range(splits)) // 128


def _bin_softmax(fx, th, lh, hkw):
    """float64 on the fp32 inputs: P [U, V] the softmax INSIDE each bin over the eligible news (0 elsewhere and for bad temperatures),
    bins [V], counts [U, G + 1], and per user C = max |s| / tau, Gs = max (sum_c |u_c n_vc| + |prior_v|) / tau over the eligible."""
    a, b = fx["a64"], fx["b64"]
    V = fx["V"]
    scores, pool = metrics._pooled(b @ a.T, hkw.get("prior"), hkw.get("stamp"), hkw.get("window"))
    mag = np.abs(b) @ np.abs(a).T + (0.0 if "prior" not in hkw else np.abs(hkw["prior"].astype(np.float64))[None, :])
    bins, _ = metrics._bins(fx["group"].numpy(), G, V)
    P, cnt, Cs, Gs = np.zeros((U, V)), np.zeros((U, G + 1)), np.zeros(U), np.zeros(U)
    for u in range(U):
        ok = ~np.isnan(scores[u]) & pool[u]
        ok[0] = False
        ex = np.asarray(lh[u], dtype=np.int64)
        ok[ex[(ex >= 1) & (ex < V)]] = False
        good = th[u] > 0 and np.isfinite(th[u])
        for bb in range(G + 1):
            sel = ok & (bins == bb)
            cnt[u, bb] = sel.sum()
            if cnt[u, bb] and good:
                x = scores[u, sel]
                w = np.exp((x - x.max()) / th[u])
                P[u, sel] = w / w.sum()
        if ok.any() and good:
            Cs[u], Gs[u] = np.abs(scores[u, ok]).max() / th[u], mag[u, ok].max() / th[u]
    return P, bins, cnt, Cs, Gs


def kappa20(N, n, C, Gs, S, L_chunks):
    """include/nrhip.h, K20: 2 (N + 1) G + 6 C + 5 ln n + 7 K + L + 27, K = 2 S, L = 128 * (chunks of the longest slice), n the
    eligible news of the largest bin."""
    return 2.0 * (N + 1) * Gs + 6.0 * C + 5.0 * np.log(np.maximum(n, 2)) + 7.0 * 2 * S + 128.0 * L_chunks + 27.0


def kappa21(N, n, Gs, S):
    """include/nrhip.h, K21: 2 (N + 1) G + 4 ln n + 7 K + 17, K = 2 S."""
    return 2.0 * (N + 1) * Gs + 4.0 * np.log(np.maximum(n, 2)) + 7.0 * 2 * S + 17.0


def _omega(seed):
    om = torch.randn(U, G + 1, generator=torch.Generator().manual_seed(seed))
    om[::4, 2] = 0.0                                                  # a weight of exactly 0 ...
    om[5] = 0.0                                                       # ... and a user with nothing but zeros
    return om


def _run_k20(fx, splits, kw, ex, tau, bases, om, sub=None):
    if sub is None:
        return ops.score_expect_groups(fx["news"], fx["user"], tau, fx["order"], bases, om.to(DEV), exclude=ex, splits=splits, **kw)
    return ops._score_expect_groups("test", fx["news"], fx["user"], tau, fx["order"], bases, om.to(DEV), ex, splits, kw.get("prior"), kw.get("stamp"),
                                    kw.get("window"), sub[0].to(DEV), sub[1].to(DEV), True)


K20_CASES = [(40, 1537, 1, False, False, False), (40, 1537, 3, True, True, True), (400, 1537, "nseg", False, True, False),
             (400, 1537, 3, True, False, True), (840, 1537, 1, True, True, True), (840, 1537, "nseg", False, False, False),
             (400, 40000, 3, True, True, True), (40, 40000, "nseg", False, True, True), (400, 40000, 1, False, False, False)]
TILE = {40: 64, 400: 32, 840: 16}


@pytest.mark.parametrize("N,V,splits,pool,lists,tauvec", K20_CASES, ids=lambda v: str(v))
def test_expect_groups_within_the_stated_bound(N, V, splits, pool, lists, tauvec):
    fx = _fx(N, V)
    order = fx["order"]
    splits = order.nseg if splits == "nseg" else splits
    kw, hkw, ex, lh, tau, th = _mode(fx, pool, lists, tauvec)
    bases = ops.score_logz_groups(fx["news"], fx["user"], tau, order, exclude=ex, **kw)
    om = _omega(N + V)
    res = {}
    labels = LW._labels(lambda: res.update(r=_run_k20(fx, splits, kw, ex, tau, bases, om)))
    out, mass = (t.double().cpu().numpy() for t in res["r"])
    want = f"expect_groups_stream[U={U},V={V},N={N},TU={TILE[N]},splits={splits},nseg={order.nseg},pos={order.n_pos}]"
    assert want in labels, labels
    P, bins, cnt, Cs, Gs = _bin_softmax(fx, th, lh, hkw)
    omh = om.double().numpy()
    E, M = metrics.expect_groups_reference(fx["a64"], fx["b64"], temperature=th, group=fx["group"].numpy(), n_groups=G, bin_w=omh, exclude=lh, **hkw)
    A = (np.abs(omh)[np.arange(U)[:, None], bins[None, :]] * P) @ np.abs(fx["a64"])
    kap = kappa20(N, cnt.max(axis=1), Cs, Gs, order.chunks_per_segment, _longest_slice(order, splits))
    tiny = V * 2.0 ** -126 * np.abs(omh).max() * np.abs(fx["a64"]).max()      # weights below the normal range are lost at 2^-126 each
    bound = kap[:, None] * EPS * A + tiny
    bad = ~(np.isfinite(th) & (th > 0))
    assert np.isnan(out[bad]).all() and np.isnan(E[bad]).all() and np.isnan(mass[bad]).all() and bad.sum() == (1 if tauvec else 0)
    err = np.abs(out[~bad] - E[~bad])
    frac = float((err / np.maximum(bound[~bad], 1e-300)).max())
    # the mass: K17's mass bound per bin, against sum omega over the non-empty bins
    msum = np.where(cnt > 0, omh, 0.0).sum(axis=1)
    mbound = (6.0 * Cs + 5.0 * np.log(np.maximum(cnt.max(axis=1), 2)) + 14.0 * order.chunks_per_segment + 23.0) * EPS * np.where(cnt > 0, np.abs(omh), 0).sum(axis=1)
    merr = np.abs(mass[~bad] - msum[~bad])
    mfrac = float((merr / np.maximum(mbound[~bad], 1e-300)).max())
    print(f"score_expect_groups N={N} V={V} splits={splits} pool={pool} lists={lists} taus={tauvec}: worst |err| / bound = {frac:.4f}, "
          f"mass {mfrac:.4f}, |mass - reference| {np.abs(mass[~bad] - M[~bad]).max():.3e}")
    assert (err <= bound[~bad]).all(), frac
    assert (merr <= mbound[~bad] + tiny).all(), mfrac
    assert not out[5].any() and mass[5] == 0.0                        # all weights 0: exactly nothing
    if lists:
        assert cnt[1, 1] == 0                                         # the list that covers the whole of group 1


def test_expect_groups_bits_one_hot_named_rows_and_a_nan_base_under_weight_zero():
    N, V, splits = 400, 1537, 3
    fx = _fx(N, V)
    order = fx["order"]
    kw, hkw, ex, lh, tau, th = _mode(fx, True, True, True)
    bases = ops.score_logz_groups(fx["news"], fx["user"], tau, order, exclude=ex, **kw)
    om = _omega(77)
    out, mass = _run_k20(fx, splits, kw, ex, tau, bases, om)
    # row u alone, and the users permuted: the same bits (NaN rows compare as bits too)
    for u in (0, 1, 3, 17, 63, 69):
        s = slice(u, u + 1)
        kw1 = dict(kw, window=kw["window"][s].contiguous())
        o1, m1 = ops.score_expect_groups(fx["news"], fx["user"][s].contiguous(), tau[s].contiguous(), order, (bases[0][s], bases[1][s]),
                                         om[s].to(DEV), exclude=ex.take(torch.tensor([u], device=DEV)), splits=splits, **kw1)
        assert torch.equal(_bits(o1), _bits(out[s])) and torch.equal(_bits(m1), _bits(mass[s])), u
    perm = torch.randperm(U, generator=torch.Generator().manual_seed(3)).to(DEV)
    o2, m2 = ops.score_expect_groups(fx["news"], fx["user"][perm].contiguous(), tau[perm].contiguous(), order, (bases[0][perm], bases[1][perm]),
                                     om.to(DEV)[perm], exclude=ex.take(perm), splits=splits, prior=kw["prior"], stamp=kw["stamp"],
                                     window=kw["window"][perm].contiguous())
    assert torch.equal(_bits(o2), _bits(out[perm])) and torch.equal(_bits(m2), _bits(mass[perm]))
    # a NaN base in a bin with omega == 0 leaves the row as it was, bit for bit
    bl = bases[0].clone()
    bl[::4, 2] = NAN
    bm = bases[1].clone()
    bm[5] = NAN
    o3, m3 = _run_k20(fx, splits, kw, ex, tau, (bl, bm), om)
    assert torch.equal(_bits(o3), _bits(out)) and torch.equal(_bits(m3), _bits(mass))
    # ... and in a bin with omega != 0 it is that user's row alone that turns NaN
    bl[6, 0] = NAN
    o4, _ = _run_k20(fx, splits, kw, ex, tau, (bl, bm), om)
    assert torch.isnan(o4[6]).all() and torch.equal(_bits(o4[7:]), _bits(out[7:]))
    # one-hot omega: the bin's own expectation; the empty bin gives zeros
    P, bins, cnt, Cs, Gs = _bin_softmax(fx, th, lh, hkw)
    kap = kappa20(N, cnt.max(axis=1), Cs, Gs, order.chunks_per_segment, _longest_slice(order, splits))
    good = np.isfinite(th) & (th > 0)
    for b in (0, 1, 3, G):
        hot = torch.zeros(U, G + 1)
        hot[:, b] = 1.0
        o, m = (t.double().cpu().numpy() for t in _run_k20(fx, splits, kw, ex, tau, bases, hot))
        Eb = (P * (bins == b)[None, :]) @ np.where(np.isfinite(fx["a64"]), fx["a64"], 0.0)
        Ab = (P * (bins == b)[None, :]) @ np.abs(fx["a64"])
        assert (np.abs(o - Eb)[good] <= (kap[:, None] * EPS * Ab + 1e-30)[good]).all(), b
        if b == 3:
            assert not o[good].any() and not m[good].any()
        else:
            assert np.abs(m[good & (cnt[:, b] > 0)] - 1.0).max() <= 1e-4
    # named rows and 1 / tau
    gen = torch.Generator().manual_seed(9)
    sid = torch.randint(-2, V + 2, (U, 5), generator=gen, dtype=torch.int32)
    sw = torch.randn(U, 5, generator=gen)
    o5, _ = _run_k20(fx, splits, kw, ex, tau, bases, om, sub=(sid, sw))
    omh = om.double().numpy()
    E, _ = metrics.expect_groups_reference(fx["a64"], fx["b64"], temperature=th, group=fx["group"].numpy(), n_groups=G, bin_w=omh, exclude=lh, **hkw)
    A = (np.abs(omh)[np.arange(U)[:, None], bins[None, :]] * P) @ np.abs(fx["a64"])
    real = ((sid >= 1) & (sid < V)).numpy()
    at = np.clip(sid.numpy(), 0, V - 1)
    swr = np.where(real, sw.double().numpy(), 0.0)
    E = E - np.einsum("ut,utc->uc", swr, fx["a64"][at])
    A = A + np.einsum("ut,utc->uc", np.abs(swr), np.abs(fx["a64"][at]))
    it = 1.0 / th[good]
    err = np.abs(o5.double().cpu().numpy()[good] - E[good] * it[:, None])
    assert (err <= (kap[:, None] * EPS * A)[good] * it[:, None] + 1e-30).all()


def _rows_for(fx, k, seed, pool):
    """Rows without repeats from a random order of [1, V); fill in the middle, an out-of-range id, with pools a key-0 entry (a news
    whose prior is -inf); user 2's row takes everything its list leaves eligible."""
    V = fx["V"]
    rows = LW._rows(V, U, k, seed=seed, fills=k > 2)
    off = int(torch.nonzero(torch.isneginf(fx["pools"][0]))[0, 0])
    if pool and k > 2:
        rows[4::7, 1] = off
    lists = [x.copy() for x in fx["lists"]]
    taken = rows[2][(rows[2] >= 1) & (rows[2] < V)].numpy()
    lists[2] = np.setdiff1d(np.arange(1, V), taken)
    return rows, lists


def _coefficient_check(fx, k, cap, pool, tauvec, signed=True, note=""):
    N, V = fx["N"], fx["V"]
    kw, hkw, _, _, tau, th = _mode(fx, pool, True, tauvec)
    rows, lists = _rows_for(fx, k, seed=k + cap, pool=pool)
    g = torch.randn(U, k, generator=torch.Generator().manual_seed(k * cap)) if signed else None
    merged = ops.ExclusionLists(lists, device=DEV).merged(ops.ExclusionLists(rows.to(DEV)))
    bases = ops.score_logz_groups(fx["news"], fx["user"], tau, fx["order"], exclude=merged, **kw)
    om, c = ops.row_logprob_capped_grad(fx["news"], fx["user"], rows.to(DEV), tau, bases, fx["gdev"], cap, n_groups=G,
                                        g=None if g is None else g.to(DEV), **kw)
    r = rows.numpy().astype(np.int64)
    mh = [np.concatenate([lists[u], r[u]]) for u in range(U)]
    grp = fx["group"].numpy()
    bh = metrics.logz_groups_reference(fx["a64"], fx["b64"], temperature=th, group=grp, n_groups=G, exclude=mh, **hkw)
    args = dict(row_ids=r, temperature=th, bases=bh[:2], group=grp, group_cap=cap, n_groups=G, **hkw)
    gh = np.ones((U, k)) if g is None else g.double().numpy()
    om_r, c_r = metrics.capped_row_logprob_grad_reference(fx["a64"], fx["b64"], g=gh, **args)
    om_a, c_a = metrics.capped_row_logprob_grad_reference(fx["a64"], fx["b64"], g=np.abs(gh), **args)
    logp, _ = metrics.capped_row_logprob_reference(fx["a64"], fx["b64"], **args)
    real = (r >= 1) & (r < V)
    step, blocked = real & np.isfinite(logp), real & np.isneginf(logp)
    A_c = np.where(step, 2.0 * np.abs(gh) - c_a, np.where(blocked, -c_a, 0.0))   # c(|g|) = |g_i| - w_i sum |g_j| / D_j at a step
    _, _, _, _, Gs = _bin_softmax(fx, th, lists, hkw)                 # over the bases AND the row
    kap = kappa21(N, bh[2].max(axis=1), Gs, fx["order"].chunks_per_segment)
    tiny = V * 2.0 ** -126 * np.abs(gh).sum(axis=1)
    b_om, b_c = kap[:, None] * EPS * om_a + tiny[:, None], kap[:, None] * EPS * A_c + tiny[:, None]
    om_d, c_d = om.double().cpu().numpy(), c.double().cpu().numpy()
    assert np.isfinite(om_d).all() and np.isfinite(c_d).all()
    e_om, e_c = np.abs(om_d - om_r), np.abs(c_d - c_r)
    frac = max(float((e_om / np.maximum(b_om, 1e-300)).max()), float((e_c / np.maximum(b_c, 1e-300)).max()))
    ident = np.abs(om_d.sum(axis=1) - c_d.sum(axis=1))
    print(f"row_logprob_capped_grad {note} N={N} V={V} k={k} cap={cap} pool={pool} taus={tauvec}: worst |err| / bound = {frac:.4f}, "
          f"blocked entries {int(blocked.sum())}, non-zero omega {int((om_r != 0).sum())}")
    assert (e_om <= b_om).all() and (e_c <= b_c).all(), frac
    assert (ident <= b_om.sum(axis=1) + b_c.sum(axis=1)).all()
    # fill and key-0 entries: c = 0 exactly; an empty bin: omega = 0 exactly; a bad temperature: zeros; the row that takes everything
    assert not c_d[~(step | blocked)].any() and not om_d[bh[2] == 0].any()
    bad = ~(np.isfinite(th) & (th > 0))
    assert not om_d[bad].any() and not c_d[bad].any()
    assert not om_d[2].any() and (bh[2][2] == 0).all()
    return rows, lists, g, bases, (om, c), blocked


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("cap", [1, 2, 128])
def test_capped_coefficients_within_the_stated_bound(k, cap):
    fx = _fx(40, 1537)
    *_, blocked = _coefficient_check(fx, k, cap, pool=(k + cap) % 2 == 0, tauvec=cap != 2)
    assert bool(blocked.any()) == (k > cap)                           # with 40 % of the news in one group the caps bind


def test_capped_coefficients_wide_vectors_unit_g_and_a_user_alone():
    fx = _fx(400, 1537)
    _coefficient_check(fx, 10, 2, pool=False, tauvec=False, signed=False, note="g = None")
    rows, lists, g, bases, (om, c), _ = _coefficient_check(fx, 10, 1, pool=True, tauvec=True, note="alone")
    kw, _, _, _, tau, _ = _mode(fx, True, True, True)
    for u in (0, 2, 3, 16, 69):
        s = slice(u, u + 1)
        kw1 = dict(kw, window=kw["window"][s].contiguous())
        o1, c1 = ops.row_logprob_capped_grad(fx["news"], fx["user"][s].contiguous(), rows[s].to(DEV), tau[s].contiguous(),
                                             (bases[0][s].contiguous(), bases[1][s].contiguous()), fx["gdev"], 1, n_groups=G, g=g[s].to(DEV), **kw1)
        assert torch.equal(_bits(o1), _bits(om[s])) and torch.equal(_bits(c1), _bits(c[s])), u


def _dense_capped(s_over_tau, elig, row, grp, cap, V, ng=G):
    """float64 torch: (nll [k], step [k] bool) of one user's row under the dense capped statement: at a live step the logsumexp over the
    eligible news not taken at an earlier step whose group has fewer than `cap` steps so far (no group: never capped).  `elig` bool [V]:
    inside the pool, finite score, not in the user's own lists."""
    k = row.shape[0]
    left = elig.clone()
    seen = {}
    nll, step = [], []
    for j in range(k):
        v = int(row[j])
        gv = int(grp[v]) if 1 <= v < V else -1
        if not (1 <= v < V) or not bool(elig[v]) or not bool(left[v]) or (0 <= gv < ng and seen.get(gv, 0) >= cap):
            nll.append(torch.zeros((), dtype=torch.float64))
            step.append(False)
            continue
        open_ = left.clone()
        for b, n in seen.items():
            if n >= cap:
                open_ &= torch.as_tensor(grp != b)
        nll.append(-(s_over_tau[v] - torch.logsumexp(s_over_tau[open_], 0)))
        step.append(True)
        left[v] = False
        if 0 <= gv < ng:
            seen[gv] = seen.get(gv, 0) + 1
    return torch.stack(nll), torch.tensor(step)


def _dense_user_grad(fx, rows, lists, gup, cap, th, hkw):
    a64, u64 = torch.tensor(fx["a64"]), torch.tensor(fx["b64"], requires_grad=True)
    V = fx["V"]
    s = u64 @ a64.T
    _, pool = metrics._pooled(np.zeros((U, V)), hkw.get("prior"), hkw.get("stamp"), hkw.get("window"))
    if "prior" in hkw:
        s = s + torch.tensor(np.where(np.isneginf(hkw["prior"]), 0.0, hkw["prior"]).astype(np.float64))[None, :]
    grp = fx["group"].numpy()
    total = torch.zeros((), dtype=torch.float64)
    steps = []
    for u in range(U):
        if not (th[u] > 0 and np.isfinite(th[u])):
            steps.append(torch.zeros(rows.shape[1], dtype=torch.bool))
            continue
        elig = torch.tensor(pool[u])
        elig[0] = False
        elig[torch.as_tensor(lists[u], dtype=torch.long)] = False
        nl, st = _dense_capped(s[u] / th[u], elig, rows[u].long(), grp, cap, V)
        total = total + (gup[u].double() * nl).sum()
        steps.append(st)
    total.backward()
    return u64.grad.numpy(), torch.stack(steps)


@pytest.mark.parametrize("cap", [2, 128])
def test_plackett_luce_nll_capped_forward_bits_and_gradient_against_the_dense_statement(cap):
    N, V, k = 40, 1537, 10
    fx = _fx(N, V)
    order = fx["order"]
    kw, hkw, _, _, tau, th = _mode(fx, True, True, True)
    rows, lists = _rows_for(fx, k, seed=31, pool=True)
    for u in range(U):                                                # rows name nothing the lists hold (listwise_loss_capped makes them fill)
        rows[u][torch.isin(rows[u], torch.as_tensor(lists[u], dtype=torch.int32))] = 0
    ex = ops.ExclusionLists(lists, device=DEV)
    rd = rows.to(DEV)
    uj = fx["user"].clone().requires_grad_(True)
    nll, valid = ops.plackett_luce_nll_capped(fx["news"], uj, rd, tau, order, fx["gdev"], cap, exclude=ex, splits=3, **kw)
    bases = ops.score_logz_groups(fx["news"], fx["user"], tau, order, exclude=ex.merged(ops.ExclusionLists(rd)), splits=3, **kw)
    logp, _ = ops.row_logprob_capped(fx["news"], fx["user"], rd, tau, bases, fx["gdev"], cap, n_groups=G, **kw)
    assert torch.equal(_bits(nll[valid]), _bits((-logp)[valid])) and not nll[~valid].any() and not valid.requires_grad
    want = (rd >= 1) & (rd < V) & torch.isfinite(logp)
    want[3] = False                                                   # the bad temperature
    assert torch.equal(valid, want) and (cap == 128 or bool(torch.isneginf(logp).any()))
    gup = torch.randn(U, k, generator=torch.Generator().manual_seed(41))
    nll.backward(gup.to(DEV))
    gu = uj.grad.double().cpu().numpy()
    ref, steps = _dense_user_grad(fx, rows, lists, gup, cap, th, hkw)
    assert torch.equal(steps, valid.cpu())
    # the two bounds carried through: K20's on the finished row, K21's on the coefficients it is built from
    r = rows.numpy().astype(np.int64)
    mh = [np.concatenate([lists[u], r[u]]) for u in range(U)]
    grp = fx["group"].numpy()
    bh = metrics.logz_groups_reference(fx["a64"], fx["b64"], temperature=th, group=grp, n_groups=G, exclude=mh, **hkw)
    gh = np.where(steps.numpy(), gup.double().numpy(), 0.0)
    args = dict(row_ids=r, temperature=th, bases=bh[:2], group=grp, group_cap=cap, n_groups=G, **hkw)
    om_r, c_r = metrics.capped_row_logprob_grad_reference(fx["a64"], fx["b64"], g=gh, **args)
    om_a, c_a = metrics.capped_row_logprob_grad_reference(fx["a64"], fx["b64"], g=np.abs(gh), **args)
    lp, _ = metrics.capped_row_logprob_reference(fx["a64"], fx["b64"], **args)
    real = (r >= 1) & (r < V)
    A_c = np.where(real & np.isfinite(lp), 2.0 * np.abs(gh) - c_a, np.where(real & np.isneginf(lp), -c_a, 0.0))
    P, bins, cnt, Cs, Gs = _bin_softmax(fx, th, mh, hkw)
    _, _, _, _, Gall = _bin_softmax(fx, th, lists, hkw)
    S = order.chunks_per_segment
    k20 = kappa20(N, cnt.max(axis=1), Cs, Gs, S, _longest_slice(order, 3))
    k21 = kappa21(N, bh[2].max(axis=1), Gall, S)
    absn = np.abs(fx["a64"])
    Ab = np.stack([(P * (bins == b)[None, :]) @ absn for b in range(G + 1)], axis=1)          # [U, G + 1, N]
    rown = np.where(real[:, :, None], absn[np.clip(r, 0, V - 1)], 0.0)                        # [U, k, N]

    def carried(kx, ky):
        return EPS * (kx[:, None] * (np.einsum("ub,ubc->uc", np.abs(om_r), Ab) + np.einsum("ui,uic->uc", np.abs(c_r), rown))
                      + ky[:, None] * (np.einsum("ub,ubc->uc", om_a, Ab) + np.einsum("ui,uic->uc", A_c, rown)))
    good = np.isfinite(th) & (th > 0)
    it = np.where(good, 1.0 / np.where(good, th, 1.0), 0.0)[:, None]
    tiny = V * 2.0 ** -126 * np.abs(gh).sum(axis=1)[:, None] * absn.max()
    bound = carried(k20, k21) * it + tiny
    err = np.abs(gu - ref)
    frac = float((err / np.maximum(bound, 1e-300))[good].max())
    print(f"plackett_luce_nll_capped cap={cap}: worst |grad_user err| / bound = {frac:.4f}")
    assert (err[good] <= bound[good]).all(), frac
    assert not gu[3].any() and not gu[~valid.any(dim=1).cpu().numpy()].any() and float(np.abs(gu).max()) > 0
    if cap >= k:
        # no cap binds: plackett_luce_nll's gradient, within the sum of both calls' bounds (K17's and K19's kappa in the same form:
        # with one Q for every bin, sum_b |omega_b| A_b is |a| A and the coefficient terms are K19's)
        u2 = fx["user"].clone().requires_grad_(True)
        n2, v2 = ops.plackett_luce_nll(fx["news"], u2, rd, tau, exclude=ex, splits=3, **kw)
        assert torch.equal(v2, valid)
        n2.backward(gup.to(DEV))
        n_all = cnt.sum(axis=1)
        k17 = LW.kappa17(N, V, 3, n_all, Cs, Gs)
        k19 = LW.kappa19(N, V, n_all, Gall)
        both = bound + carried(k17, k19) * it + tiny
        diff = np.abs(gu - u2.grad.double().cpu().numpy())
        print(f"  against plackett_luce_nll: worst |difference| / bound = {float((diff / np.maximum(both, 1e-300))[good].max()):.4f}")
        assert (diff[good] <= both[good]).all()
    with pytest.raises(RuntimeError, match="missing pass"):
        ops.plackett_luce_nll_capped(fx["news"].clone().requires_grad_(True), uj, rd, tau, order, fx["gdev"], cap)


def _oracle_capped(tag, cfg, sd, news_vecs, hist, mask, rows, tau, weight, grp, cap):
    """The loss on the CPU: the oracle's user encoder on the gathered vectors (the table a constant), then the dense float64 capped
    statement.  Returns (loss, n rows, user-encoder gradients)."""
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("user_encoder.")}
    user = O.nrms_user_encoder(news_vecs[hist.long()], mask, sdo, cfg).double()
    s = user @ news_vecs.double().T / tau
    Ur, Vn = s.shape
    k = rows.shape[1]
    w = torch.ones(Ur, k, dtype=torch.float64) if weight is None else (weight.double()[:, None].expand(Ur, k) if weight.dim() == 1 else weight.double())
    total, n = torch.zeros((), dtype=torch.float64), 0
    clicked = hist.long() * (mask != 0).long()
    for u in range(Ur):
        elig = torch.ones(Vn, dtype=torch.bool)
        elig[0] = False
        elig[clicked[u]] = False
        nl, st = _dense_capped(s[u], elig, rows[u].long(), grp, cap, Vn, ng=3)
        total = total + (w[u] * nl).sum()
        n += int(st.any())
    loss = total / max(n, 1)
    loss.backward()
    return loss.detach(), n, {k_: v.grad for k_, v in sdo.items() if v.grad is not None}


def test_listwise_loss_capped_on_the_tiny_model():
    """The tolerances are those tests/test_gpu_listwise.py holds train.listwise_loss to against the same oracle."""
    tag = "nrms_tiny_pad"
    model, cfg, sd, news_vecs, hist, mask, rows = LW._tiny_case(tag, k=6)
    Vn, tau, cap = news_vecs.shape[0], 0.7, 2
    grp = (torch.arange(Vn) % 4).to(torch.int32)
    grp[grp == 3] = -1                                                # groups 0 .. 2 and no group: G = 3 here
    Ur, k = rows.shape
    gen = torch.Generator().manual_seed(103)
    per_row = torch.randn(Ur, generator=gen)
    per_place = 1.0 / torch.log2(torch.arange(k) + 2.0)[None, :] * (1.0 + torch.rand(Ur, k, generator=gen))
    for weight in (None, per_row, per_place):
        model.zero_grad()
        loss, n = TR.listwise_loss_capped(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), rows.numpy(), tau, grp.numpy(), cap, weight=weight)
        assert n.dtype == torch.int64 and n.dim() == 0 and n.device.type == "cuda"
        loss_b, n_b = TR.listwise_loss_capped(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), rows.numpy(), tau, grp.numpy(), cap,
                                              weight=weight, batch_size=5)
        assert int(n_b) == int(n)
        assert_close(loss_b, loss, 1e-5, name="loss in batches")
        loss.backward()
        lo, no, go = _oracle_capped(tag, cfg, sd, news_vecs, hist, mask, rows, tau, weight, grp.numpy(), cap)
        assert no == int(n) == Ur - 1
        assert_close(loss, lo, 1e-4, name="loss vs oracle")
        # rtol as there; the absolute floor is the same 2e-4 of the LARGEST gradient of the encoder: att_fc2.bias is added to every
        # logit of a softmax, so its exact gradient is 0 and what either side holds is the rounding residue of a sum of terms the
        # size of the other gradients
        checked, floor = 0, 2e-4 * max(float(v.abs().max()) for v in go.values())
        for name, p in model.named_parameters():
            if name in go:
                assert_close(p.grad, go[name], floor, 2e-4, name="d" + name)
                checked += 1
            else:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
        assert checked >= 4
    # the caps bind in this case: some entry is blocked, and the capped loss is not the uncapped one
    ex = TR._exclusions(hist.to(DEV), mask.to(DEV), True, None, torch.device(DEV))
    clean = rows.to(DEV).masked_fill(TR._not_ranked(ex, rows.to(DEV), Vn), 0)
    assert bool(TR._blocked(clean, grp.to(DEV), 3, cap).any())
    with torch.no_grad():
        capped, _ = TR.listwise_loss_capped(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), rows.numpy(), tau, grp.numpy(), cap)
        free, _ = TR.listwise_loss(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), rows.numpy(), tau)
    assert abs(float(capped) - float(free)) > 1e-3
    with pytest.raises(RuntimeError, match="missing pass"):
        TR.listwise_loss_capped(model, news_vecs.to(DEV).requires_grad_(True), hist.numpy(), mask.numpy(), rows.numpy(), tau, grp.numpy(), cap)
    with pytest.raises(RuntimeError, match="cannot be cut"):
        TR.listwise_loss_capped(model, news_vecs.to(DEV), hist.numpy(), mask.numpy(), np.ones((Ur, 129), dtype=np.int32), tau, grp.numpy(), cap)

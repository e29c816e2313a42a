"""CPU proof of the softmax sweep (tests/test_gpu_softmax_sweep.py): its case table, its reference and the power of its checker
(all in the first part of that file).  Nothing here touches a GPU.

  (a) the file's reference equals the host statements of metrics.py on the case table: logz_reference, entropy_reference,
      expect_reference and expect_affine_reference;
  (b) the route functions put at least two cases in every route and the table holds what the issue lists; the plateau condition
      holds for every plateau case; every m of {1, 2, 3, 64, 129} is the m_u of some user;
  (c) the four size queries of the library (host arithmetic: they answer with dummy pointers) equal the restated carve and plan;
  (d) a fp32 numpy stand-in for the four entry points, reading its buffers through the strides of the descriptor, passes every
      layer of every case, both in the kernels' order (the score chain of csrc/nr_score_tile.h fma by fma; a lane-free restatement
      of the rest: fp32 exponentials, fp32 contraction chains per slice in ascending id order, slices merged in fp64, as the
      comments at the top of nr_logz.hip, nr_expect.hip and nr_entropy.hip state them) and with float64 accumulation rounded once;
  (e) each mutant of MUTANTS fails at the layer named, and the header's bounds alone catch those of GAUSS_MUTANTS on Gaussian data;
  (f) an exponential with a relative error of 2^-20 passes `bound` at every Gaussian case -- the gap this sweep closes -- and fails
      `tight` on plateau data with m = 3; a second run that differs in one bit fails `repeat`; a result that depends on a stride
      fails `layout`;
  (g) the named-row calls: two cases per route, a sound stand-in (the gather through the strides, the header's formulas in
      float64 rounded once) passes, and each mutant of ROW_MUTANTS fails at the layer named;
  (h) the news side: two cases per route, the transposed lists hold every length and a chunk of users with 128 and 65 listed, the
      size queries (rows and mass-only) equal the restated carve, a sound stand-in passes every layer against the references of
      tests/test_gpu_expect_news.py and test_gpu_entropy_news.py (which are metrics.expect_news_reference and
      expect_news_affine_reference), and each mutant of NEWS_MUTANTS fails at the layer named.
Every mutant is pinned to the one case that must catch it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_softmax_sweep as H
from test_corpus_sweep_host import chain, rd, tile_order
from newsrecommendation_amd import _lib, metrics

DEV = "cpu"
CASES = {c.name: c for c in H.sm_cases()}
f32, f64, i32 = np.float32, np.float64, np.int32
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------ the stand-in
def wr(b, arr, ld):
    """arr [rows, cols] written to buffer b at row stride ld, as a kernel given that stride would."""
    f = b.flat[b.start:]
    for r in range(arr.shape[0]):
        f[r * ld:r * ld + arr.shape[1]] = torch.from_numpy(np.ascontiguousarray(arr[r]))


def _vec(P, name):
    return P.inb[name].v[0].numpy() if name in P.inb else None


def _eligible(P, s, mutant):
    """[U, V] bool as the stream decides it: id >= 1, the key of pool_key (NaN score, prior -inf, stamp outside the window), the
    CSR lists with their clamped bounds."""
    c, S = P.c, P.S
    U, V = c.U, c.V
    el = ~np.isnan(s)
    if mutant != "row0_counted":
        el[:, 0] = False
    prior = _vec(P, "prior")
    if prior is not None and mutant != "prior_neginf_counted":
        el &= ~np.isneginf(prior)[None, :]
    if "stamp" in P.inb:
        stamp, win = _vec(P, "stamp"), rd(P.inb["window"], U, 2, 2 if mutant == "two_for_ld_window" else S.win)
        hi_ok = (stamp[None, :] < win[:, 1:2]) if mutant == "window_hi_exclusive" else (stamp[None, :] <= win[:, 1:2])
        el &= (win[:, :1] <= stamp[None, :]) & hi_ok
    if "offsets" in P.inb:
        off, ids = _vec(P, "offsets"), _vec(P, "xids")
        n = len(ids)
        for u in range(U):
            b = min(max(int(off[u]), 0), n)
            x = ids[b:max(min(int(off[u + 1]), n), b)].astype(np.int64)
            x = x[(x >= 1) & (x < V)]
            if mutant == "listed_65th_kept":                                 # one probe of 64 lanes per chunk, no refill
                x = np.concatenate([x[(x - 1) // 128 == q][:64] for q in np.unique((x - 1) // 128)] + [np.zeros(0, np.int64)])
            el[u, x] = False
    if mutant == "neginf_score_not_counted":
        el &= ~np.isneginf(s)
    return el


def _scores(P, mutant, acc64):
    c, S = P.c, P.S
    lim = c.N + 4 if mutant == "float4_past_N" else c.N
    user, news = rd(P.inb["user"], c.U, lim, S.user), rd(P.inb["news"], c.V, lim, S.news)
    s = chain(user, news, c.N, tile_order(c.N), acc64, lim)
    prior = _vec(P, "prior")
    with np.errstate(all="ignore"):
        return (s + prior[None, :]).astype(f32) if prior is not None else s


def _taus(P, mutant):
    c = P.c
    tau = _vec(P, "tau_u") if "tau_u" in P.inb and mutant != "tau_u_ignored" else np.full(c.U, P.I.tau, f32)
    with np.errstate(all="ignore"):
        return tau, (tau > 0) & (tau < INF), (f32(1) / tau).astype(f32)


def _slices(P):
    p = H.plan(P.entry, P.c)
    return [(1 + s * p.segs_per * p.seg, min(1 + (s + 1) * p.segs_per * p.seg, P.c.V)) for s in range(p.splits)]


def _expf(d, mutant):
    with np.errstate(all="ignore"):
        e = np.exp(d.astype(f32)).astype(f32)
        return np.where(d != 0, e * f32(1 + 2.0 ** -20), e).astype(f32) if mutant == "exp_rel_2m20" else e      # expf(0) stays 1


def _seam(P, mutant):
    """(ids the mutant counts twice, ids it skips): the first news of every slice but the first."""
    firsts = np.array([lo for lo, _ in _slices(P)[1:]], np.int64)
    return (firsts if mutant == "seam_twice" else firsts[:0]), (firsts if mutant == "seam_skip" else firsts[:0])


def _sum(x, acc64, axis=None):
    """A sum in fp64, or one fp32 chain in ascending order."""
    if acc64 or x.dtype == f64:
        return np.sum(x.astype(f64), axis=axis)
    if x.size == 0:
        return np.zeros(x.shape[1:] if axis == 0 else (), f32)
    return np.cumsum(x, axis=0, dtype=f32)[-1]


def _lane_sum(P, idx, w, acc64):
    """K13's order for the weights w of the ids idx (rescaled to the user's maximum already): a lane's chain is fp32 over its own
    news of a segment (lane = (id - segment start) mod 64), the 64 lanes of a segment meet in a fp32 butterfly, segments in fp64."""
    if acc64:
        return float(np.sum(w.astype(f64)))
    seg = H.plan("logz", P.c).seg
    key = ((idx - 1) // seg) * 64 + ((idx - 1) % seg) % 64
    total = 0.0
    for sgm in np.unique(key // 64):
        lanes = np.zeros(64, f32)
        for k in np.unique(key[key // 64 == sgm]):
            lanes[k % 64] = np.cumsum(w[key == k], dtype=f32)[-1]
        total += float(np.sum(lanes.reshape(32, 2), axis=1, dtype=f32).sum(dtype=f32))
    return total


def standin(mutant=None, acc64=False):
    """call(P) for the four entry points, on the CPU buffers of P."""
    state = {"calls": 0}

    def logz(P):
        c = P.c
        s = _scores(P, mutant, acc64)
        el = _eligible(P, s, mutant)
        twice, skip = _seam(P, mutant)
        tau, ok, it = _taus(P, mutant)
        lsum, smax, cnt = np.full(c.U, -INF, f32), np.full(c.U, -INF, f32), np.zeros(c.U, i32)
        for u in range(c.U):
            e_u = el[u].copy()
            e_u[skip] = False
            idx = np.flatnonzero(e_u)
            idx = np.sort(np.concatenate([idx, twice[e_u[twice]]]))
            if mutant == "listed_max_kept":                                   # the maximum taken before the lists are looked at
                e2 = _eligible(H.SimpleNamespace(c=c, S=P.S, I=P.I, inb={k: v for k, v in P.inb.items() if k not in ("offsets", "xids")}), s, mutant)[u]
                smax[u] = s[u, e2].max() if e2.any() else -INF
            x = s[u, idx]
            cnt[u] = len(idx)
            if not len(idx):
                continue
            if mutant != "listed_max_kept":
                smax[u] = x.max()
            if not ok[u] or not np.isfinite(smax[u]):
                lsum[u] = NAN
                continue
            with np.errstate(all="ignore"):
                d = ((x - smax[u]).astype(f32) * it[u]).astype(f32)
                w = np.where(x == smax[u], f32(1), _expf(d, mutant)).astype(f32)
                lsum[u] = f32(np.log(_lane_sum(P, idx, w, acc64)))
            if mutant == "logsum_two_ulps" and lsum[u] > 0:
                lsum[u] = np.nextafter(np.nextafter(lsum[u], f32(INF)), f32(INF))
        if mutant == "stride_dependent" and P.S.news != c.N:
            lsum = np.where(lsum > 0, np.nextafter(lsum, f32(INF)), lsum).astype(f32)
        P.outb["logsum"].v[0], P.outb["max"].v[0], P.outb["count"].v[0] = torch.from_numpy(lsum), torch.from_numpy(smax), torch.from_numpy(cnt)

    def weights(P):
        """Per user (eligible ids ascending, p fp32, x fp32) or None for a user without weights; dead = the users whose results are NaN."""
        c = P.c
        s = _scores(P, mutant, acc64)
        el = _eligible(P, s, mutant)
        twice, skip = _seam(P, mutant)
        tau, ok, it = _taus(P, mutant)
        bm, bl = _vec(P, "base_max"), _vec(P, "base_logsum")
        none = np.isneginf(bm)
        dead = ~none & (~ok | np.isnan(bm) | np.isnan(bl) | np.isposinf(bm))
        if mutant == "bad_tau_spoils_neighbour":
            dead = dead | (np.roll(~ok, 1) & (np.arange(c.U) % 16 != 0))
        rows = []
        for u in range(c.U):
            if none[u] or dead[u]:
                rows.append(None)
                continue
            e_u = el[u].copy()
            e_u[skip] = False
            idx = np.sort(np.concatenate([np.flatnonzero(e_u), twice[e_u[twice]]]))
            with np.errstate(all="ignore"):
                d = (s[u, idx] - bm[u]).astype(f32)
                x = np.where(d == 0, -bl[u], (d.astype(f64) * f64(it[u]) - f64(bl[u])).astype(f32)).astype(f32)   # one fma; s == max: -logsum
                p = _expf(x, mutant)
            rows.append((idx, p, x))
        return rows, dead, it

    def entropy(P):
        c = P.c
        rows, dead, _ = weights(P)
        out = {k: np.zeros(c.U, f32) for k in ("H", "var", "mass")}
        for u, row in enumerate(rows):
            if dead[u]:
                out["H"][u] = out["var"][u] = out["mass"][u] = NAN
            if row is None:
                continue
            _, p, x = row
            with np.errstate(all="ignore"):
                keep = np.ones(len(p), bool) if mutant == "zero_times_inf" else p > 0
                p64, x64 = p[keep].astype(f64), x[keep].astype(f64)
                m0, m1, m2 = p64.sum(), (p64 * x64).sum(), (p64 * x64 * x64).sum()
                out["H"][u], out["var"][u], out["mass"][u] = f32(-m1), f32(m2 - m1 * m1), f32(m0)
        for k in P.outb:
            P.outb[k].v[0] = torch.from_numpy(out[k])

    def contract(P):
        c, S, I = P.c, P.S, P.I
        affine = P.entry == "affine"
        rows, dead, it = weights(P)
        news = rd(P.inb["news"], c.V, c.N, S.news)
        clean = np.where(np.isfinite(news), news, f32(0)).astype(f32)
        alpha, beta = _vec(P, "alpha"), _vec(P, "beta") if affine else None
        out, mass = np.zeros((c.U, c.N), f32), np.zeros(c.U, f32)
        TU = H.plan(P.entry, c).TU
        drop = mutant is not None and mutant.startswith("last_slab_dropped") and H.tk_npad(c.N) // 32 == H.KMAX[TU] == int(mutant.rsplit("_", 1)[1])
        spoiled = affine and mutant == "nan_alpha_spreads" and alpha is not None and np.isnan(alpha).any()
        for u, row in enumerate(rows):
            acc, m0, mr = np.zeros(c.N, f64), 0.0, 0.0
            if dead[u]:
                out[u], mass[u] = NAN, NAN
                continue
            if row is not None:
                idx, p, x = row
                with np.errstate(all="ignore"):
                    if affine:
                        a_u, b_u = (alpha[u] if alpha is not None else f32(1)), (beta[u] if beta is not None else f32(0))
                        wgt = (f64(b_u) * x.astype(f64) + f64(a_u)).astype(f32)
                        r = np.where(p > 0, (p * wgt).astype(f32), f32(0)).astype(f32)
                    else:
                        r = p
                    for lo, hi in _slices(P):
                        sl = (idx >= lo) & (idx < hi)
                        acc += _sum((r[sl, None] * clean[idx[sl]]).astype(f32), acc64, axis=0).astype(f64)
                    m0, mr = float(p.astype(f64).sum()), float(r.astype(f64).sum())
                if drop:
                    acc[(H.KMAX[TU] - 1) * 32:] = 0.0
            with np.errstate(all="ignore"):
                if not affine and alpha is not None:
                    acc = acc * f64(alpha[u])
                named = np.zeros(c.N, f64)
                if "sub_ids" in P.inb:
                    ids = rd(P.inb["sub_ids"], c.U, c.T, c.T if mutant == "T_for_ld_sub" else S.sub)[u].astype(np.int64)
                    sw = rd(P.inb["sub_w"], c.U, c.T, c.T if mutant == "T_for_ld_sub" else S.sub)[u].astype(f64)
                    real = (ids >= 1) & (ids < c.V)
                    if mutant == "sub_fill_subtracted":
                        ids, real = np.clip(ids, 0, c.V - 1), np.ones(len(ids), bool)
                    for t in np.flatnonzero(real):
                        named += sw[t] * news[ids[t]].astype(f64)                # the named rows as they are
                if "s" in c.opt:
                    acc = acc * f64(it[u])
                    if mutant != "scale_skips_named":
                        named = named * f64(it[u])
                out[u] = (acc - named).astype(f32)
                mass[u] = f32(mr if affine and mutant == "mass_sum_r" else m0)
        if spoiled:
            out[:] = NAN
        wr(P.outb["out"], out, c.N if mutant == "N_for_ld_out" else S.out)
        if "mass" in P.outb:
            P.outb["mass"].v[0] = torch.from_numpy(mass)

    def call(P):
        state["calls"] += 1
        {"logz": logz, "entropy": entropy, "expect": contract, "affine": contract}[P.entry](P)
        if mutant == "ws_overrun" and P.entry == "expect":
            P.ws.flat[P.ws.start + P.ws.cols] = 1
        if mutant == "one_bit_second_run" and P.entry == "entropy" and state["calls"] % 2 == 0:
            h = P.outb["H"].v[0].numpy()
            P.outb["H"].v[0] = torch.from_numpy(np.nextafter(h, f32(INF)))
    return call


# ------------------------------------------------------------------------------------------ (a) the references
def _kw(I):
    kw = {}
    if I.prior is not None:
        kw["prior"] = I.prior
    if I.stamp is not None:
        kw["stamp"], kw["window"] = I.stamp, I.window
    if I.segs is not None:
        kw["exclude"] = I.segs
    return kw


def _eq(a, b, what, rtol=1e-12):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    assert np.allclose(np.nan_to_num(a, posinf=1e300, neginf=-1e300), np.nan_to_num(b, posinf=1e300, neginf=-1e300), rtol=rtol, atol=1e-300), what


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.V < 1000 or c.N <= 4], ids=str)
def test_the_reference_equals_the_metrics_statements(name):
    c = CASES[name]
    I = H.sm_inputs(c)
    R = H.sm_reference(c, I)
    tau = I.tau_u.astype(f64) if I.tau_u is not None else float(np.float32(I.tau))
    kw = _kw(I)
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    # a -inf maximum and a spoiled base are the device's statements (base_max = -inf reads as nothing eligible; a NaN base gives NaN):
    # metrics.py knows neither, so those two users are compared with nothing here
    k = ~(R.ninf | np.array([I.special.get(u) == "nanbase" for u in range(c.U)]))
    with np.errstate(all="ignore"):
        ls, mx, cnt = metrics.logz_reference(n64, u64, temperature=tau, **kw)
        _eq(R.logsum[k], ls[k], "logsum")
        _eq(R.smax, mx, "max")
        assert np.array_equal(R.count, cnt)
        Hh, var, mass = metrics.entropy_reference(n64, u64, tau, **kw)
        _eq(R.H[k], Hh[k], "H", 1e-9)
        _eq(R.mass[k], mass[k], "mass")
        assert np.allclose(np.nan_to_num(R.var[k]), np.nan_to_num(var[k]), rtol=1e-6, atol=1e-9 * (1 + np.nan_to_num(R.H) ** 2).max())
        E, m = metrics.expect_reference(n64, u64, temperature=tau, weight=I.weight, **kw)
        _eq((R.al[:, None] * R.E)[k], E[k], "E", 1e-9)
        for scale in (False, True):
            F, m = metrics.expect_affine_reference(n64, u64, tau, alpha=I.weight, beta=I.beta, sub_ids=I.sub_ids, sub_w=I.sub_w, scale_inv_tau=scale, **kw)
            ref = H.finish(R, "affine", scale)[0]
            live = ~R.nan & k
            assert np.array_equal(np.isnan(ref[live]), np.isnan(F[live])), "affine NaN"
            tot = H.finish(R, "affine", scale)[2]
            assert (np.abs(np.nan_to_num(ref[live]) - np.nan_to_num(F[live])) <= 1e-9 * np.nan_to_num(tot[live], nan=0.0, posinf=0.0) + 1e-300).all(), "affine"


# ------------------------------------------------------------------------------------------ (b) the table
def test_every_route_has_two_cases_and_the_table_holds_what_the_issue_lists():
    cs = list(CASES.values())
    for e in H.ENTRIES:
        H._count_routes([H.ROUTE_FN[e](c) for c in cs], H.ROUTES[e], e)
    assert {c.N for c in cs} >= set(H.SM_NS) and {c.V for c in cs} >= set(H.SM_VS) | {H.V_TWO}
    assert {c.T for c in cs} >= set(H.SM_TS) | {0} and {c.pool for c in cs} == {0, 1, 2, 3} and {c.csr for c in cs} == {0, 1, 2}
    assert {c.splits for c in cs} >= {0, 1, 2, 3, 129} and {c.pad for c in cs} == {0, 1, 2}
    for tile_of in (H.stream_tile, H.contract_tile):                          # U = 1, TU - 1, TU, TU + 1 of every tile of either pair
        for t in (64, 32, 16):
            assert {c.U for c in cs if tile_of(c.N) == t} >= {1, t - 1, t, t + 1}, (tile_of.__name__, t)
    assert [H.stream_tile(n) for n in (484, 964)] == [32, 16] and [H.contract_tile(n) for n in (356, 836)] == [32, 16]
    assert [H.stream_tile(n) for n in (480, 481, 960, 961)] == [64, 32, 32, 16] and [H.contract_tile(n) for n in (352, 353, 832, 833)] == [64, 32, 32, 16]
    for letter in "wbsvM":                                                    # every optional pointer NULL in some case and given in another
        assert any(letter in c.opt for c in cs) and any(letter not in c.opt for c in cs)
    assert any(c.taus for c in cs) and any(not c.taus for c in cs)
    p = H.plan("logz", CASES["gauss-two-chunks-short"])
    assert (p.seg, p.nseg, p.segs_per, p.splits) == (256, 129, 17, 8)


def test_the_plateau_condition_and_the_planted_maxima():
    seen, listed_max = set(), 0
    for c in CASES.values():
        if c.kind != "plateau":
            continue
        I = H.sm_inputs(c)
        R = H.sm_reference(c, I)
        assert H.plateau_condition(c, I, R), c.name
        live = ~R.nan & (R.count > 0)
        seen |= set(R.m[live].tolist())
        if c.csr and c.U >= 2:                                                # user 1 lists all its planted news: its maximum is another level
            I2 = H.SimpleNamespace(**vars(I))
            I2.segs = None
            listed_max += int(H.sm_reference(c, I2).smax[1] > R.smax[1])
    assert seen >= {1, 2, 3, 64, 129}, seen
    assert listed_max >= 2


def test_the_lists_reach_the_refill_and_the_seek_branches():
    for name in ("gauss-seek", "plateau-seek-pool"):
        c = CASES[name]
        I = H.sm_inputs(c)
        lo1 = 1 + H.plan("logz", c).segs_per * H.plan("logz", c).seg
        assert lo1 == 257
        per_chunk = np.bincount((I.segs[0] - 1) // 128, minlength=3)
        assert per_chunk[0] == 128 and per_chunk[1] == 65                     # LZ_LISTED refills once in either chunk
        assert (I.segs[0] < lo1).all() and len(I.segs[0]) > 64                # all entries before slice 1, steps > 1
        assert 64 < (I.segs[1] < lo1).sum() < len(I.segs[1])                  # the cursor ends inside a long segment
        assert (I.segs[2] >= lo1).all() and len(I.segs[2])                    # no probe below the slice start
    lens = {len(s) for c in CASES.values() if c.csr == 1 and c.U >= 6 for s in H.sm_inputs(c).segs}
    assert lens >= {0, 1, 64, 65, 129, 300}, lens


# ------------------------------------------------------------------------------------------ (c) the size queries
def _dummy(P, name):
    return 4096 if (name in P.inb or name in P.outb) else None


@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_the_size_queries_equal_the_restated_carve(name):
    c = CASES[name]
    I = H.sm_inputs(c)
    for e in H.ENTRIES:
        for variant in ("pad", "dense"):
            P = H.SimpleNamespace(entry=e, c=c, I=I, S=H.strides(c, variant), ws=None, ws_bytes=0, inb={k: 1 for k in (
                "news", "user", "base_max", "base_logsum") + (("prior",) if I.prior is not None else ()) + (("stamp", "window") if I.stamp is not None else ()) + (
                ("offsets", "xids") if I.offsets is not None else ()) + (("tau_u",) if I.tau_u is not None else ()) + (("sub_ids", "sub_w") if c.T else ())},
                outb={k: 1 for k in ("logsum", "max", "count", "H", "out")})
            d, query, _ = H.descriptor(P, _dummy)
            assert query(C.byref(d)) == H.ws_bytes(e, c), (e, _lib.last_error())


@pytest.mark.parametrize("N", sorted(H.REFUSED_NS), ids=str)
def test_the_size_queries_refuse_a_width_that_is_no_multiple_of_four(N):
    c = CASES[f"gauss-N{H.REFUSED_NS[N]}"]._replace(N=N)
    I = H.sm_inputs(CASES[f"gauss-N{H.REFUSED_NS[N]}"])
    for e in H.ENTRIES:
        P = H.SimpleNamespace(entry=e, c=c, I=I, S=H.strides(c, "dense"), ws=None, ws_bytes=0, inb={"news": 1, "user": 1, "base_max": 1, "base_logsum": 1}, outb={})
        d, query, _ = H.descriptor(P, lambda P, name: 4096 if name in P.inb or name in ("tau_u",) else None)
        assert query(C.byref(d)) == 0 and "multiple of 4" in _lib.last_error(), (e, _lib.last_error())


# ------------------------------------------------------------------------------------------ (d) the sound stand-ins
@pytest.mark.parametrize("acc64", (False, True), ids=("chain", "fp64"))
@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_a_sound_standin_passes_every_layer(name, acc64):
    c = CASES[name]
    H.sm_sweep(c, DEV, standin(None, acc64), layout=not acc64, agree=not acc64 and c.V < 1000)      # layout and agree once, in the kernels' order


# ------------------------------------------------------------------------------------------ (e) the mutants
# mutant -> (the layer that must catch it, the one case that must catch it)
MUTANTS = {
    "float4_past_N": ("exact", "plateau-N4"),
    "two_for_ld_window": ("exact", "plateau-N28"),
    "T_for_ld_sub": ("exact", "plateau-N36"),
    "N_for_ld_out": ("sentinel", "plateau-N32"),
    "last_slab_dropped_11": ("tight", "plateau-N352"),
    "last_slab_dropped_26": ("exact", "plateau-N832"),
    "last_slab_dropped_32": ("tight", "plateau-N1024"),
    "listed_65th_kept": ("exact", "plateau-seek"),
    "seam_twice": ("exact", "plateau-seek"),
    "seam_skip": ("exact", "plateau-seek"),
    "window_hi_exclusive": ("exact", "plateau-N28"),
    "prior_neginf_counted": ("exact", "plateau-N356"),
    "row0_counted": ("exact", "plateau-N4"),
    "neginf_score_not_counted": ("special", "special-a"),
    "sub_fill_subtracted": ("exact", "plateau-N36"),
    "mass_sum_r": ("tight", "plateau-two-chunks-auto"),
    "zero_times_inf": ("special", "special-a"),
    "bad_tau_spoils_neighbour": ("special", "special-a"),
    "nan_alpha_spreads": ("special", "special-a"),
    "scale_skips_named": ("tight", "plateau-two-chunks-auto"),
    "tau_u_ignored": ("bound", "gauss-N28"),
    "listed_max_kept": ("exact", "plateau-seek"),
    "logsum_two_ulps": ("exact", "plateau-one-chunk"),
    "exp_rel_2m20": ("tight", "plateau-seek"),
    "ws_overrun": ("sentinel", "gauss-N4"),
    "one_bit_second_run": ("repeat", "gauss-N4"),
    "stride_dependent": ("layout", "gauss-seek"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS), ids=str)
def test_every_mutant_fails_at_the_layer_named(mutant):
    layer, name = MUTANTS[mutant]
    with pytest.raises(H.SoftmaxCheckError) as e:
        H.sm_sweep(CASES[name], DEV, standin(mutant), agree=False)
    assert e.value.layer == layer, (mutant, name, str(e.value))


# the same mutants on Gaussian data: the header's bounds must see them too (a bound whose absolute term swallowed every row would not)
GAUSS_MUTANTS = {"last_slab_dropped_11": "gauss-N352", "last_slab_dropped_26": "gauss-N832", "last_slab_dropped_32": "gauss-N1024", "scale_skips_named": "gauss-two-chunks-auto",
                 "mass_sum_r": "gauss-two-chunks-auto", "seam_skip": "gauss-seek"}


@pytest.mark.parametrize("mutant", list(GAUSS_MUTANTS), ids=str)
def test_the_header_bounds_catch_a_mutant_on_gaussian_data(mutant):
    with pytest.raises(H.SoftmaxCheckError) as e:
        H.sm_sweep(CASES[GAUSS_MUTANTS[mutant]], DEV, standin(mutant), layout=False, agree=False)
    assert e.value.layer == "bound", str(e.value)


def test_there_are_at_least_twenty_mutants():
    assert len(MUTANTS) >= 20


# ------------------------------------------------------------------------------------------ (f) the gap
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.kind == "gauss"], ids=str)
def test_a_2m20_exponential_passes_the_derived_bounds_at_every_gaussian_case(name):
    """The statement of the gap: the header's bounds alone cannot see an exponential that is wrong in its 20th bit."""
    H.sm_sweep(CASES[name], DEV, standin("exp_rel_2m20"), layout=False, agree=False)


def test_a_2m20_exponential_fails_tight_at_three_maxima():
    c = CASES["plateau-two-chunks-short"]
    assert c.m == 3
    with pytest.raises(H.SoftmaxCheckError) as e:
        H.sm_sweep(c, DEV, standin("exp_rel_2m20"), layout=False)
    assert e.value.layer == "tight"


# ------------------------------------------------------------------------------------------ the named-row calls
ROWS = {c.name: c for c in H.row_cases()}


def row_standin(mutant=None):
    """call(P) for nr_row_logprob and nr_row_logprob_grad: the gather through the strides (the score chain fma by fma), then the
    header's formulas in float64 rounded once."""
    def call(P):
        c, I, S = P.c, P.I, P.S
        U, V, N, k = c.U, c.V, c.N, c.k
        lim = N + 4 if mutant == "float4_past_N" else N
        s_all = chain(rd(P.inb["user"], U, lim, S.user), rd(P.inb["news"], V, lim, S.news), N, tile_order(N), False, lim)
        prior = _vec(P, "prior")
        ids = rd(P.inb["row_ids"], U, k, k if mutant == "k_for_ld_ids" else S.ids).astype(np.int64)
        tau, ok, _ = _taus(P, None)
        bm, bl = _vec(P, "base_max").astype(f64), _vec(P, "base_logsum").astype(f64)
        g = rd(P.inb["g"], U, k, k if mutant == "k_for_ld_g" else S.g).astype(f64) if "g" in P.inb else np.ones((U, k))
        logp, a_out, c_out = np.zeros((U, k)), np.zeros(U), np.zeros((U, k))
        with np.errstate(all="ignore"):
            for u in range(U):
                real = (ids[u] >= 1) & (ids[u] < V)
                at = np.where(real, ids[u], 0)
                s = s_all[u, at]
                live = real.copy()
                if prior is not None:
                    s = (s + prior[at]).astype(f32)
                    live &= ~np.isneginf(prior[at])
                if "stamp" in P.inb:
                    stamp, win = _vec(P, "stamp"), rd(P.inb["window"], U, 2, S.win)
                    live &= (win[u, 0] <= stamp[at]) & (stamp[at] <= win[u, 1])
                live &= ~np.isnan(s)
                x, t = s.astype(f64), f64(tau[u])
                if P.entry == "logprob":
                    for j in range(k):
                        if not real[j]:
                            continue
                        if not live[j] or not ok[u]:
                            logp[u, j] = NAN
                        elif c.seq:
                            j2 = j + 1 if mutant == "suffix_off_by_one" else j
                            rest = np.concatenate([x[j2:][live[j2:]], [bm[u]]])
                            M = rest.max()
                            mass = np.exp((x[j2:][live[j2:]] - M) / t).sum() + (np.exp((bm[u] - M) / t + bl[u]) if bm[u] > -INF or np.isnan(bl[u]) else 0.0)
                            logp[u, j] = (x[j] - M) / t - np.log(mass)
                        else:
                            logp[u, j] = (x[j] - bm[u]) / t - bl[u]
                elif ok[u] and not np.isnan(bm[u]) and not np.isnan(bl[u]) and live.any():
                    steps = np.flatnonzero(live)
                    xs, gl = x[steps], g[u, steps]
                    M = max(bm[u], xs.max())
                    lx = (xs - M) / t
                    lb = (bm[u] - M) / t + bl[u] if bm[u] > -INF else -INF
                    lw, run = np.empty(len(steps)), lb
                    for n_i in range(len(steps) - 1, -1, -1):
                        run = np.logaddexp(lx[n_i], run)
                        lw[n_i] = run
                    for n_i, i in enumerate(steps):
                        upto = n_i if mutant == "prefix_exclusive" else n_i + 1
                        c_out[u, i] = gl[n_i] - np.sum(gl[:upto] * np.exp(lx[n_i] - lw[:upto]))
                    a_out[u] = np.sum(gl * np.exp(lb - lw)) if lb > -INF else 0.0
            if P.entry == "logprob":
                P.outb["logp"].v[:] = torch.from_numpy(logp.astype(f32))
                if "total" in P.outb:
                    P.outb["total"].v[0] = torch.from_numpy(logp.sum(axis=1).astype(f32))
            else:
                P.outb["weight"].v[0], P.outb["sub_w"].v[:] = torch.from_numpy(a_out.astype(f32)), torch.from_numpy(c_out.astype(f32))
    return call


def test_the_row_routes_have_two_cases_each():
    cs = list(ROWS.values())
    H._count_routes([H.row_route(c) for c in cs], H.ROW_ROUTES, "rows")
    assert {c.k for c in cs} >= set(H.ROW_KS) and {c.seq for c in cs} == {0, 1} and {c.pad for c in cs} == {0, 1, 2}


@pytest.mark.parametrize("name", list(ROWS), ids=str)
def test_a_sound_row_standin_passes_every_layer(name):
    H.row_sweep(ROWS[name], DEV, row_standin())


ROW_MUTANTS = {
    "float4_past_N": ("exact", "rows-k1-seq0"),
    "k_for_ld_ids": ("exact", "rows-k63-seq0"),
    "k_for_ld_g": ("tight", "rows-k63-seq1"),
    "suffix_off_by_one": ("tight", "rows-k63-seq1"),
    "prefix_exclusive": ("tight", "rows-k63-seq1"),
}


@pytest.mark.parametrize("mutant", list(ROW_MUTANTS), ids=str)
def test_every_row_mutant_fails_at_the_layer_named(mutant):
    layer, name = ROW_MUTANTS[mutant]
    with pytest.raises(H.SoftmaxCheckError) as e:
        H.row_sweep(ROWS[name], DEV, row_standin(mutant))
    assert e.value.layer == layer, (mutant, name, str(e.value))


# ------------------------------------------------------------------------------------------ the news side
NEWS = {c.name: c for c in H.news_cases()}


def news_standin(mutant=None, acc64=False):
    """call(P) for nr_score_expect_news (rows, mass-only) and nr_score_expect_news_affine: the pairs' p and x as in `weights` above,
    eligibility through the transposed lists, one fp32 chain per (news, slice of the user axis) in ascending user order, slices
    and named terms in fp64, one rounding."""
    def call(P):
        c, S, I = P.c, P.S, P.I
        U, V, N = c.U, c.V, c.N
        affine = P.entry == "newsaffine"
        lim = N + 4 if mutant == "float4_past_N" else N
        user, news = rd(P.inb["user"], U, lim, S.user), rd(P.inb["news"], V, lim, S.news)
        s = chain(user, news, N, tile_order(N), acc64, lim)
        prior = _vec(P, "prior")
        with np.errstate(all="ignore"):
            if prior is not None:
                s = (s + prior[None, :]).astype(f32)
        el = ~np.isnan(s)
        el[:, 0] = False
        if prior is not None:
            el &= ~np.isneginf(prior)[None, :]
        if "stamp" in P.inb:
            stamp, win = _vec(P, "stamp"), rd(P.inb["window"], U, 2, 2 if mutant == "two_for_ld_window" else S.win)
            el &= (win[:, :1] <= stamp[None, :]) & (stamp[None, :] <= win[:, 1:2])
        if "offsets" in P.inb:
            off, ids = _vec(P, "offsets"), _vec(P, "xids")
            n = len(ids)
            for v in range(V):
                b = min(max(int(off[v]), 0), n)
                x = ids[b:max(min(int(off[v + 1]), n), b)].astype(np.int64)
                x = x[(x >= 0) & (x < U)]
                if mutant == "listed_65th_kept":
                    x = np.concatenate([x[x // 128 == q][:64] for q in np.unique(x // 128)] + [np.zeros(0, np.int64)])
                el[x, v] = False
        tau, ok, it = _taus(P, None)
        bm, bl = _vec(P, "base_max"), _vec(P, "base_logsum")
        with np.errstate(all="ignore"):
            live = ok & (np.abs(bm) < INF) & (np.abs(bl) < INF)
            d = (s - bm[:, None]).astype(f32)
            x = np.where(d == 0, -bl[:, None], (d.astype(f64) * it.astype(f64)[:, None] - bl.astype(f64)[:, None]).astype(f32)).astype(f32)
            p = np.where(el & live[:, None], _expf(x, mutant), f32(0))
            al = _vec(P, "alpha") if "alpha" in P.inb else np.ones(U, f32)
            be = _vec(P, "beta") if "beta" in P.inb else np.zeros(U, f32)
            scale = "s" in c.opt
            ca = (al * it).astype(f32) if scale else al
            cb = (be * it).astype(f32) if scale else be
            if affine:
                fin = np.isfinite(ca) & np.isfinite(cb)
                if mutant == "nan_alpha_reaches_rows":
                    fin = np.ones(U, bool)
                wgt = (cb.astype(f64)[:, None] * x.astype(f64) + ca.astype(f64)[:, None]).astype(f32)
                r = np.where((p > 0) & fin[:, None], (p * wgt).astype(f32), f32(0))
                mass = (r if mutant == "mass_sum_r" else p).astype(f64).sum(axis=0)
            else:
                r = np.where(p > 0, (ca[:, None] * p).astype(f32), f32(0))
                mass = (al.astype(f64)[:, None] * p.astype(f64) * live[:, None]).sum(axis=0)
            clean = np.where(np.isfinite(user[:, :N]), user[:, :N], f32(0)).astype(f32)
            spoil = (0.0 * user[:, :N].astype(f64)).sum(axis=0) if mutant == "user_component_not_cleaned" else 0.0    # 0 * inf of a dead user of the tile
            pl = H.news_plan(c)
            out = np.zeros((V, N), f64)
            for sl in range(pl.splits):
                lo, hi = sl * pl.segs_per * pl.seg, min((sl + 1) * pl.segs_per * pl.seg, U)
                if mutant == "seam_skip" and sl:
                    lo += 1
                if mutant == "seam_twice" and sl:
                    lo -= 1
                for v in range(1, V):
                    out[v] += spoil
                    u_ = lo + np.flatnonzero(r[lo:hi, v] != 0)
                    if len(u_):
                        out[v] += _sum((r[u_, v][:, None] * clean[u_]).astype(f32), acc64, axis=0).astype(f64)
            if "n_off" in P.inb:
                no, nu, nw = _vec(P, "n_off"), _vec(P, "n_user"), _vec(P, "n_w")
                nn = len(nu)
                for v in range(V):
                    for j in range(min(max(int(no[v]), 0), nn), min(max(int(no[v + 1]), 0), nn)):
                        u = int(nu[j])
                        if nw[j] != 0 and 0 <= u < U and (live[u] or mutant == "named_dead_user_subtracted"):
                            sc = f64(it[u]) if scale and mutant != "scale_ignored_in_named" else 1.0
                            out[v] -= f64(nw[j]) * sc * clean[u].astype(f64)
        if "out" in P.outb:
            wr(P.outb["out"], out.astype(f32), N if mutant == "N_for_ld_out" else S.out)
        if "mass" in P.outb:
            P.outb["mass"].v[0] = torch.from_numpy(mass.astype(f32))
    return call


def test_the_news_routes_have_two_cases_each_and_the_lists_hold_every_length():
    cs = list(NEWS.values())
    H._count_routes([H.news_route(c) for c in cs], H.NEWS_ROUTES, "news")
    assert {c.U for c in cs} >= set(H.SM_VS) | {H.V_TWO} and {c.N for c in cs} >= set(H.SM_NS)
    for t in (64, 32, 16):                                                    # V - 1 real rows = 1, TV - 1, TV, TV + 1
        assert {c.V - 1 for c in cs if H.contract_tile(c.N) == t} >= {1, t - 1, t, t + 1}, t
    I = H.news_inputs(NEWS["news-gauss-lists"])
    lens = set(np.diff(np.minimum(I.v_off, len(I.v_users))).tolist())
    assert lens >= {0, 1, 64, 65, 129, 300}, lens
    per_chunk = [np.bincount(I.v_users[I.v_off[v]:I.v_off[v + 1]][(I.v_users[I.v_off[v]:I.v_off[v + 1]] >= 0)] // 128).max(initial=0) for v in range(NEWS["news-gauss-lists"].V)]
    assert max(per_chunk) >= 65                                               # the refill loop of LZ_LISTED on the user axis


@pytest.mark.parametrize("name", list(NEWS), ids=str)
def test_the_news_size_queries_equal_the_restated_carve(name):
    c = NEWS[name]
    I = H.news_inputs(c)
    for e in ("news", "newsmass", "newsaffine"):
        names = ("news", "user", "base_max", "base_logsum") + (("prior",) if I.prior is not None else ()) + (("stamp", "window") if I.stamp is not None else ()) + (
            ("offsets", "xids") if I.v_off is not None else ()) + (("tau_u",) if I.tau_u is not None else ()) + (("n_off", "n_user", "n_w") if I.n_off is not None else ())
        P = H.SimpleNamespace(entry=e, c=c, I=I, S=H.SimpleNamespace(news=c.N, user=c.N, out=c.N, win=2), ws=None, ws_bytes=0, inb={k: 1 for k in names},
                              outb={"mass": 1} if e == "newsmass" else {"out": 1})
        d, query, _ = H.news_descriptor(P, _dummy)
        assert query(C.byref(d)) == H.news_ws_bytes(c, e != "newsmass"), (e, _lib.last_error())


@pytest.mark.parametrize("name,acc64", [(n, False) for n in NEWS] + [(n, True) for n, c in NEWS.items() if c.N <= 484],        # fp64 accumulation: the narrower widths
                         ids=lambda v: v if isinstance(v, str) else ("chain", "fp64")[v])
def test_a_sound_news_standin_passes_every_layer(name, acc64):
    c = NEWS[name]
    H.news_sweep(c, DEV, news_standin(None, acc64), standin(None, acc64), layout=not acc64, agree=not acc64 and c.U < 1000)


# mutant -> (layer, the one case that must catch it)
NEWS_MUTANTS = {
    "nan_alpha_reaches_rows": ("special", "news-gauss-lists"),
    "named_dead_user_subtracted": ("special", "news-gauss-lists"),
    "user_component_not_cleaned": ("special", "news-gauss-lists"),
    "mass_sum_r": ("exact", "news-plateau-two-chunks-auto"),
    "scale_ignored_in_named": ("exact", "news-plateau-two-chunks-auto"),
    "listed_65th_kept": ("special", "news-gauss-lists"),
    "seam_twice": ("exact", "news-plateau-two-chunks-short"),
    "seam_skip": ("exact", "news-plateau-two-chunks-short"),
    "N_for_ld_out": ("sentinel", "news-plateau-N4"),
    "float4_past_N": ("exact", "news-plateau-N4"),
    "exp_rel_2m20": ("tight", "news-plateau-many-maxima"),
}


@pytest.mark.parametrize("mutant", list(NEWS_MUTANTS), ids=str)
def test_every_news_mutant_fails_at_the_layer_named(mutant):
    layer, name = NEWS_MUTANTS[mutant]
    with pytest.raises(H.SoftmaxCheckError) as e:
        H.news_sweep(NEWS[name], DEV, news_standin(mutant), standin(), agree=False)
    assert e.value.layer == layer, (mutant, name, str(e.value))


@pytest.mark.parametrize("name", [n for n, c in NEWS.items() if c.kind == "gauss"], ids=str)
def test_a_2m20_exponential_passes_the_header_bounds_at_every_gaussian_news_case(name):
    """The gap on the news side: kappa of 150 and more cannot see an exponential that is wrong in its 20th bit; `tight` does
    (NEWS_MUTANTS)."""
    H.news_sweep(NEWS[name], DEV, news_standin("exp_rel_2m20"), standin(), layout=False, agree=False)


def test_the_news_plateau_cases_hold_every_number_of_maxima():
    seen = set()
    for c in NEWS.values():
        if c.kind == "plateau":
            I = H.news_inputs(c)
            rows = I.news[I.planted]
            seen |= {int((rows == r).all(axis=1).sum()) for r in rows}
    assert seen >= {1, 2, 3, 64, 129}, seen

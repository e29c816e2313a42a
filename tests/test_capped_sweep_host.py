"""CPU proof of the capped sweep (tests/test_gpu_capped_sweep.py): its case tables, its references and the power of its checker
(all in the first part of that file).  Nothing here touches a GPU.

  (a) the file's references equal the host statements of metrics.py: logz_groups_reference, expect_groups_reference (K22's and the
      row calls' references ARE metrics.expect_news_groups_reference, capped_row_logprob_reference and
      capped_row_logprob_grad_reference); on the reference side sum_b omega_b = sum_i c_i to fp64 rounding;
  (b) the table restatement agrees with ops.GroupOrder on every case (order, pos, bin_start, seg_start, bin_seg, positions and
      by_position of the lists);
  (c) the route functions put at least two cases on every route; the plateau condition holds for every plateau case; the
      empty-slice case has an empty slice and both 2-chunk and 1-chunk segments, the list shapes are what the docstrings say;
  (d) the three size queries of the library (host arithmetic: they answer with dummy pointers) equal the restated carve and plan;
  (e) a numpy stand-in for the five entry points, reading its buffers through the strides of the descriptor (fp32 scores, fp32
      exponentials and pair weights, float64 accumulation rounded once), passes every layer of every case;
  (f) each mutant of the MUTANTS tables fails at the layer named, pinned to the one case that must catch it; an exponential with a
      relative error of 2^-20 passes `bound` on the Gaussian cases and fails `tight` on plateau data, for K20 and K22 each.  K15
      forms no exponential on plateau data that is not exactly 1 or 0 (the maximum's weight is the constant 1), so its mutant is
      the exponential applied at the maximum too, which fails `exact` (DESIGN.md says why no derived bound on real exponentials
      separates 2^-20 for K15);
  (g) K22's lists by position hold the shapes of the issue, and every hand-made special kind and `agree` run in two cases or more.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_capped_sweep as H
from test_corpus_sweep_host import rd
from test_softmax_sweep_host import wr
from newsrecommendation_amd import _lib, metrics, ops

DEV = "cpu"
CASES = {c.name: c for c in H.cap_cases()}
ROWS = {c.name: c for c in H.row_cases()}
f32, f64, i32 = np.float32, np.float64, np.int32
INF, NAN = float("inf"), float("nan")
SMALL = [n for n, c in CASES.items() if c.U <= 300]
_rd1 = lambda P, name: P.inb[name].v[0].numpy() if name in P.inb else None


# ------------------------------------------------------------------------------------------ the stand-in: the stream calls
def _expf(d, mutant):
    with np.errstate(all="ignore"):
        e = np.exp(d.astype(f32)).astype(f32)
        if mutant == "exp_rel_2m20_everywhere":                               # K15 with the maximum's weight taken from the exponential too
            return (e * f32(1 + 2.0 ** -20)).astype(f32)
        return np.where(d != 0, e * f32(1 + 2.0 ** -20), e).astype(f32) if mutant == "exp_rel_2m20" else e      # expf(0) stays 1


def _stream_view(P, mutant):
    """What a stream kernel sees of P's buffers, in POSITION space: ids [n_pos] (0 = padding), scores fp32 [U, n_pos] (prior
    added), eligible [U, n_pos], taus."""
    c, S, T = P.c, P.S, P.T
    U, V, N = c.U, T.V, c.N
    user, news = rd(P.inb["user"], U, N, S.user), rd(P.inb["news"], V, N, S.news)
    order = _rd1(P, "order").astype(np.int64)
    real = (order >= 1) & (order < V)
    ids = np.where(real, order, 0)
    if mutant == "padding_eligible":
        real = np.ones_like(real)
    with np.errstate(all="ignore"):
        s = (user.astype(f64) @ news.astype(f64)[ids].T).astype(f32)
        prior = _rd1(P, "prior")
        if prior is not None:
            pr = prior[np.minimum(np.arange(T.n_pos), V - 1)] if mutant == "prior_by_position" else prior[ids]
            s = (s + pr[None, :]).astype(f32)
    el = real[None, :] & ~np.isnan(s)
    if prior is not None:
        el &= ~np.isneginf(pr)[None, :]
    if "stamp" in P.inb:
        st = _rd1(P, "stamp")[np.minimum(np.arange(T.n_pos), V - 1) if mutant == "stamp_by_position" else ids]
        win = rd(P.inb["window"], U, 2, S.win)
        el &= (win[:, :1] <= st[None, :]) & (st[None, :] <= win[:, 1:2])
    tau = _rd1(P, "tau_u") if "tau_u" in P.inb else np.full(U, P.I.tau, f32)
    with np.errstate(all="ignore"):
        ok, it = (tau > 0) & (tau < INF), (f32(1) / tau).astype(f32)
    return SimpleNamespace(ids=ids, real=real, s=s, el=el, tau=tau, ok=ok, it=it, news=news, user=user)


def _listed_by_user(P, Vw, mutant):
    """[U, n_pos] bool from the lists in position space (clamped offsets)."""
    c, T = P.c, P.T
    out = np.zeros((c.U, T.n_pos), bool)
    if "offsets" not in P.inb:
        return out
    off, x = _rd1(P, "offsets"), _rd1(P, "xids").astype(np.int64)
    n = len(x)
    for u in range(c.U):
        b = min(max(int(off[u]), 0), n)
        e = x[b:max(min(int(off[u + 1]), n), b)]
        e = e[(e >= 0) & (e < T.n_pos)]
        if mutant == "lists_in_id_space":                                     # the entries taken for news ids
            e = T.pos[e[(e >= 1) & (e < T.V)]]
        if mutant == "listed_65th_kept":                                      # one probe of 64 lanes per chunk, no refill
            e = np.concatenate([e[e // 128 == q][:64] for q in np.unique(e // 128)] + [np.zeros(0, np.int64)]).astype(np.int64)
        out[u, e] = True
    return out


def _segments(P, mutant):
    """[(segment, lo, hi)] the segments the slices of the call stream, in order."""
    c, T = P.c, P.T
    ss = _rd1(P, "seg_start").astype(np.int64)
    sl = H.slices(T, H.plan(P.entry, c, T).splits)
    segs = []
    for y, (lo, hi) in enumerate(sl):
        if mutant == "empty_slice_dropped" and y > 0 and sl[y - 1][0] >= sl[y - 1][1]:
            continue                                                          # the slice after an empty one is lost with it
        for sg in range(lo, hi):
            segs.append(sg)
            if mutant == "seam_twice" and y > 0 and sg == lo:
                segs.append(sg)
    return [(sg, int(ss[sg]), int(ss[sg + 1])) for sg in segs], ss


def standin(mutant=None):
    """call(P) for the five entry points, on the CPU buffers of P."""
    state = {"calls": 0}

    def logzg(P):
        c, T = P.c, P.T
        U, nb = c.U, T.G + 1
        v = _stream_view(P, mutant)
        el = v.el & ~_listed_by_user(P, T.V, mutant)
        segs, ss = _segments(P, mutant)
        bs = _rd1(P, "bin_seg").astype(np.int64)
        if mutant == "bin_seg_off_by_one":
            bs = np.minimum(bs + (np.arange(len(bs)) > 0), T.nseg)
            bs[-1] = T.nseg
        cnt_s, carried = {}, np.zeros(U, np.int64)
        for sg, lo, hi in segs:
            n = el[:, lo:hi].sum(axis=1)
            cnt_s[sg] = cnt_s.get(sg, 0) + n + (carried if mutant == "count_not_reset" else 0)
            carried = cnt_s[sg]
        lsum, gmax, cnt = np.full((U, nb), -INF, f32), np.full((U, nb), -INF, f32), np.zeros((U, nb), i32)
        twice = [sg for i, (sg, _, _) in enumerate(segs) if i and segs[i - 1][0] == sg]
        for b in range(nb):
            mine = [sg for sg in range(int(bs[b]), int(bs[b + 1])) if sg in cnt_s]
            if not mine:
                continue
            lo, hi = int(ss[mine[0]]), int(ss[mine[-1] + 1])
            e = el[:, lo:hi].copy()
            if mutant == "empty_slice_dropped":
                keep = np.zeros(hi - lo, bool)
                for sg in mine:
                    keep[int(ss[sg]) - lo:int(ss[sg + 1]) - lo] = True
                e &= keep[None, :]
            x = np.where(e, v.s[:, lo:hi], f32(-INF))
            cnt[:, b] = sum(cnt_s[sg] for sg in mine)
            M = x.max(axis=1) if hi > lo else np.full(U, -INF, f32)
            gmax[:, b] = np.where(cnt[:, b] > 0, M, f32(-INF))
            good = (cnt[:, b] > 0) & v.ok & np.isfinite(M)
            with np.errstate(all="ignore"):
                d = ((x - np.where(good, M, f32(0))[:, None]).astype(f32) * v.it[:, None]).astype(f32)
                w = np.where(e, np.where((x == M[:, None]) & (mutant != "exp_rel_2m20_everywhere"), f32(1), _expf(d, mutant)), f32(0)).astype(f64)
                for sg in twice:
                    if sg in mine:
                        w[:, int(ss[sg]) - lo:int(ss[sg + 1]) - lo] *= 2.0
                lsum[:, b] = np.where(cnt[:, b] == 0, -INF, np.where(good, np.log(w.sum(axis=1)), NAN)).astype(f32)
        ld = nb + 3 if mutant == "padded_out_stride" else nb
        for k, a in (("logsum", lsum), ("max", gmax), ("count", cnt)):
            wr(P.outb[k], a, ld)

    def expectg(P):
        c, S, T = P.c, P.S, P.T
        U, N, nb = c.U, c.N, T.G + 1
        v = _stream_view(P, mutant)
        el = v.el & ~_listed_by_user(P, T.V, mutant)
        ldb = nb if mutant == "dense_ld_base" else S.base
        bm, bl, om = (rd(P.inb[k], U, nb, ldb) for k in ("base_max", "base_logsum", "bin_w"))
        segs, ss = _segments(P, mutant)
        bs = _rd1(P, "bin_seg").astype(np.int64)
        bin_of_seg = np.searchsorted(bs[1:], np.arange(T.nseg), side="right")
        clean = np.where(np.isfinite(v.news), v.news, f32(0)).astype(f64)
        out, mass = np.zeros((U, N), f64), np.zeros(U, f64)
        sl = H.slices(T, H.plan("expectg", c, T).splits)
        first_bin = {sg: bin_of_seg[lo] for lo, hi in sl for sg in range(lo, hi)}
        with np.errstate(all="ignore"):
            full = bm != -INF
            bad = (full & ~v.ok[:, None]).any(axis=1) | (full & (om != 0) & (~(np.abs(om) < INF) | ~(bm < INF) | np.isnan(bl))).any(axis=1)
            for sg, lo, hi in segs:
                b = bin_of_seg[sg]
                ob = first_bin[sg] if mutant == "omega_of_previous_bin" else b
                g, l, o = bm[:, b], bl[:, b], om[:, ob]
                s = v.s[:, lo:hi]
                arg = np.where(s == g[:, None], -l[:, None], ((s - g[:, None]).astype(f32).astype(f64) * v.it.astype(f64)[:, None] - l.astype(f64)[:, None])).astype(f32)
                p = _expf(arg, mutant)
                live = (o != 0) & (g != -INF)
                if mutant == "nan_from_zero_omega":
                    live = g != -INF
                e = el[:, lo:hi]
                if mutant == "padding_weighted":
                    e = e | ~v.real[None, lo:hi]
                wgt = np.where(e & live[:, None], (o[:, None] * p).astype(f32), f32(0)).astype(f64)
                rows = v.news.astype(f64)[v.ids[lo:hi]] if mutant == "padding_weighted" else clean[v.ids[lo:hi]]
                out += wgt @ rows
                mass += wgt.sum(axis=1)
            named = np.zeros((U, N), f64)
            if "sub_ids" in P.inb:
                ids, sw = rd(P.inb["sub_ids"], U, c.T, S.sub).astype(np.int64), rd(P.inb["sub_w"], U, c.T, S.sub).astype(f64)
                for u in range(U):
                    for t in np.flatnonzero((ids[u] >= 1) & (ids[u] < T.V)):
                        named[u] += sw[u, t] * v.news[ids[u, t]].astype(f64)
            it = v.it.astype(f64)[:, None] if "s" in c.opt else 1.0
            res = (out * it - named * (1.0 if mutant == "named_not_scaled" else it)).astype(f32)
            mres = mass.astype(f32)
            if mutant == "finalize_reads_empty_slice" and any(lo >= hi for lo, hi in sl):
                res[:], mres[:] = NAN, NAN                                    # the workspace holds NaN where nothing was written
            res[bad], mres[bad] = NAN, NAN
        wr(P.outb["out"], res, S.out)
        if "mass" in P.outb:
            P.outb["mass"].v[0] = torch.from_numpy(mres)

    def newsg(P):
        c, S, T = P.c, P.S, P.T
        U, V, N, nb = c.U, T.V, c.N, T.G + 1
        v = _stream_view(P, None)
        el = v.el.copy()
        if "offsets" in P.inb:                                                # the lists by position
            off, x = _rd1(P, "offsets"), _rd1(P, "xids").astype(np.int64)
            n = len(x)
            for p_ in range(T.n_pos):
                b = min(max(int(off[p_]), 0), n)
                e = x[b:max(min(int(off[p_ + 1]), n), b)]
                el[e[(e >= 0) & (e < U)], p_] = False
        bstart = _rd1(P, "bin_start").astype(np.int64)
        pl = H.plan("newsg", c, T)
        if mutant == "bases_user_major":
            flat = lambda k: P.inb[k].flat[P.inb[k].start:].numpy()                 # element (u, b) taken from u * (n_groups + 1) + b, inside the payload
            rdb = lambda k: np.stack([[flat(k)[min(u * nb + b, nb * S.bin - 1)] for u in range(U)] for b in range(nb)]).astype(f32)
        else:
            rdb = lambda k: rd(P.inb[k], nb, U, S.bin)
        bm, bl, om = rdb("base_max"), rdb("base_logsum"), rdb("bin_w")
        uclean = np.where(np.isfinite(v.user), v.user, f32(0)).astype(f64)
        out, mass = np.zeros((V, N), f64), np.zeros(V, f64)
        seams = [s * pl.segs_per * pl.seg for s in range(1, pl.splits)] if mutant == "user_seam_twice" else []
        with np.errstate(all="ignore"):
            for p_ in np.flatnonzero(v.real):
                vid = v.ids[p_]
                if mutant == "bin_after_empty_wrong":
                    b = int(min(np.searchsorted(bstart, (p_ // 128) * 128, side="left"), nb - 1))
                else:
                    b = int(min(np.searchsorted(bstart[1:], p_, side="right"), nb - 1))
                g, l, o = bm[b], bl[b], om[b]
                alive = v.ok & np.isfinite(g) & np.isfinite(l) & np.isfinite(o) & (o != 0)
                if mutant == "dead_pair_nan":                                 # 0 * p over a NaN base
                    alive = v.ok
                cf = (o * v.it).astype(f32) if "s" in c.opt else o
                s = v.s[:, p_]
                arg = np.where(s == g, -l, ((s - g).astype(f32).astype(f64) * v.it.astype(f64) - l.astype(f64))).astype(f32)
                p = _expf(arg, mutant)
                on = el[:, p_] & alive
                wgt = np.where(on, (cf * p).astype(f32), f32(0)).astype(f64)
                wm = np.where(on, (o.astype(f64) * p.astype(f64)), 0.0)
                for u in seams:
                    wgt[u], wm[u] = 2 * wgt[u], 2 * wm[u]
                out[vid] = wgt @ uclean
                mass[vid] = wm.sum()
            if mutant == "row0_partials":
                out[0], mass[0] = NAN, NAN
            if mutant == "padding_row_partials" and not v.real.all():           # a padding position writes its partial at the id it holds, clamped: row 0
                out[0], mass[0] = f64(3e37) * uclean.sum(axis=0), 1.0
            if "n_off" in P.inb:
                off, nu, nw = _rd1(P, "n_off"), _rd1(P, "n_user").astype(np.int64), _rd1(P, "n_w")
                n = len(nu)
                for vid in range(V):
                    for j in range(min(max(int(off[vid]), 0), n), max(min(int(off[vid + 1]), n), min(max(int(off[vid]), 0), n))):
                        u = nu[j]
                        if nw[j] == 0 or u < 0 or u >= U or not v.ok[u]:
                            continue
                        if mutant == "named_gated_by_base":
                            b = T.bins[vid] if vid else 0
                            if not (np.isfinite(bm[b, u]) and np.isfinite(bl[b, u])):
                                continue
                        it = f64(v.it[u]) if "s" in c.opt else 1.0
                        out[vid] -= f64(nw[j]) * it * uclean[u]
        with np.errstate(over="ignore"):                                      # `agree` replaces news under unchanged bases: other rows may overflow
            wr(P.outb["out"], out.astype(f32), S.out)
            if "mass" in P.outb:
                P.outb["mass"].v[0] = torch.from_numpy(mass.astype(f32))

    def rows(P):
        c, S, I = P.c, P.S, P.I
        U, V, N, k, G = c.U, c.V, c.N, c.k, c.G
        news, user = rd(P.inb["news"], V, N, S.news).astype(f64), rd(P.inb["user"], U, N, S.user).astype(f64)
        ids = rd(P.inb["row_ids"], U, k, k if mutant == "k_for_ld_ids" else S.ids)
        ldb = G + 1 if mutant == "dense_ld_base" else S.base
        bm, bl = rd(P.inb["base_max"], U, G + 1, ldb), rd(P.inb["base_logsum"], U, G + 1, ldb)
        grp = _rd1(P, "group").astype(np.int64)
        grp = np.where(grp >= G, grp % G if mutant == "id_ge_G_is_a_group" else -1, grp)
        cap = c.cap + (mutant == "cap_late") - (mutant == "cap_early")
        kw = dict(row_ids=ids, temperature=_rd1(P, "tau_u").astype(f64) if "tau_u" in P.inb else float(f32(I.tau)), bases=(bl.astype(f64), bm.astype(f64)), group=grp,
                  group_cap=cap, n_groups=G, prior=_rd1(P, "prior"), stamp=_rd1(P, "stamp"), window=rd(P.inb["window"], U, 2, S.win) if "window" in P.inb else None)
        if mutant == "key0_counts_as_live":
            news = np.where(np.isnan(news), 0.0, news)
        if mutant == "no_group_bin_capped":
            kw["group"], kw["n_groups"] = np.where(grp < 0, G, grp), G + 1
            kw["bases"] = tuple(np.concatenate([x, np.full((U, 1), -INF)], axis=1) for x in kw["bases"])
        with np.errstate(all="ignore"):
            if P.entry == "logpc":
                lp, tot = metrics.capped_row_logprob_reference(news, user, **kw)
                for u in np.flatnonzero(np.isnan(bm[:, G])):                  # the device's walk: a NaN base of the bin that never closes reaches every D_j
                    step = (ids[u] >= 1) & (ids[u] < V) & np.isfinite(lp[u])
                    lp[u, step], tot[u] = NAN, NAN if step.any() else tot[u]
                if mutant == "total_finite_beside_blocked":
                    tot = np.where(np.isneginf(tot), np.where(np.isneginf(lp), 0.0, lp).sum(axis=1), tot)
                wr(P.outb["logp"], lp.astype(f32), k)
                if "total" in P.outb:
                    P.outb["total"].v[0] = torch.from_numpy(tot.astype(f32))
            else:
                g = rd(P.inb["g"], U, k, k if mutant == "k_for_ld_g" else S.g).astype(f64) if "g" in P.inb else None
                inner = mutant if mutant in ("q_after_close", "blocked_zero", "closed_full_q", "blocked_after_close", "exclusive_scan", "blocked_g_read") else None
                om, cc = metrics._capped_grad_rows(news, user, kw["row_ids"], kw["temperature"], kw["bases"], kw["group"], kw["group_cap"], kw["n_groups"], g, kw["prior"],
                                                   kw["stamp"], kw["window"], mutant=inner)
                if mutant == "no_group_bin_capped":
                    om = om[:, :G + 1]
                wr(P.outb["bin_w"], om.astype(f32), G + 1 if mutant == "dense_out_ld_base" else S.base)
                wr(P.outb["sub_w"], cc.astype(f32), k)

    def call(P):
        state["calls"] += 1
        {"logzg": logzg, "expectg": expectg, "newsg": newsg, "logpc": rows, "logpcg": rows}[P.entry](P)
        if mutant == "ws_overrun" and P.entry == "expectg":
            P.ws.flat[P.ws.start + P.ws.cols] = 1.0
        if mutant == "one_bit_second_run" and P.entry == "newsg" and state["calls"] % 2 == 0:
            o = P.outb["out"].v.numpy()
            o[:] = np.nextafter(o, f32(INF))
        if mutant == "stride_dependent" and P.entry == "logzg" and P.S.news != P.c.N:
            o = P.outb["logsum"].v.numpy()
            o[:] = np.where(o > 0, np.nextafter(o, f32(INF)), o)
    return call


# ------------------------------------------------------------------------------------------ (a) the references
def _kw(I):
    return {k: v for k, v in (("prior", I.prior), ("stamp", I.stamp), ("window", I.window), ("exclude", I.segs)) if v is not None}


def _eq(a, b, what, rtol=1e-11, atol=1e-300):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    assert np.allclose(np.nan_to_num(a, posinf=1e300, neginf=-1e300), np.nan_to_num(b, posinf=1e300, neginf=-1e300), rtol=rtol, atol=atol), what


@pytest.mark.parametrize("name", SMALL, ids=str)
def test_the_reference_equals_the_metrics_statements(name):
    c = CASES[name]
    T = H.tables(c)
    c = H.resolve(c, T)
    I = H.cap_inputs(c, T)
    R = H.cap_reference(c, I, T)
    tau = I.tau_u.astype(f64) if I.tau_u is not None else float(np.float32(I.tau))
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    with np.errstate(all="ignore"):
        ls, gm, cnt = metrics.logz_groups_reference(n64, u64, temperature=tau, group=T.group, n_groups=T.G, **_kw(I))
        E, m = metrics.expect_groups_reference(n64, u64, temperature=tau, group=T.group, n_groups=T.G, bin_w=I.omega.astype(f64), **_kw(I))
    _eq(R.logsum, ls, "logsum", atol=1e-12)
    _eq(R.gmax, gm, "gmax")
    assert np.array_equal(R.count, cnt)
    k = np.array([I.special.get(u) not in ("logsumnan", "gmaxinf") for u in range(c.U)])      # defects of the bases handed to K20: metrics.py, given none, knows nothing of them
    assert np.array_equal(np.isnan(E).all(axis=1)[k], R.nan20[k]) and np.array_equal(np.isnan(m)[k], R.nan20[k])
    ok = ~R.nan20 & k
    assert np.allclose(R.E[ok], E[ok], rtol=1e-9, atol=1e-12 * (1 + R.A[ok]))
    with np.errstate(invalid="ignore"):
        pm = (I.omega.astype(f64)[:, T.bins] * R.P).sum(axis=1)                # sum omega p: the header's sum of omega over the non-empty bins
    assert np.allclose(pm[ok], m[ok], rtol=1e-9, atol=1e-12) and np.allclose(R.mass[ok], m[ok], rtol=1e-9, atol=1e-9 * (1 + R.Mabs[ok]))
    if c.kind == "plateau":
        assert H.plateau_condition(R)


def test_every_multiplicity_occurs_on_plateau_data():
    seen = set()
    for name in SMALL:
        c = CASES[name]
        if c.kind != "plateau":
            continue
        T = H.tables(c)
        c = H.resolve(c, T)
        seen |= set(np.unique(H.cap_reference(c, H.cap_inputs(c, T), T).m).tolist())
    assert {1, 2, 3, 64, 129} <= seen, sorted(seen)


@pytest.mark.parametrize("name", list(ROWS), ids=str)
def test_the_row_reference_guards_itself(name):
    c = ROWS[name]
    R = H.row_reference(c, H.row_inputs(c))
    assert H.row_reference_identity(R) <= 2.0 ** -40, H.row_reference_identity(R)
    assert not (R.step & R.blocked).any()


# ------------------------------------------------------------------------------------------ (b) the tables
@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_the_tables_are_ops_group_order(name):
    c = CASES[name]
    T = H.tables(c._replace(opt=c.opt.replace("x", "")))
    go = ops.GroupOrder(torch.from_numpy(T.group), n_groups=T.G)
    assert (go.n_pos, go.nseg, go.chunks_per_segment) == (T.n_pos, T.nseg, T.S)
    for k in ("order", "pos", "bin_start", "seg_start", "bin_seg"):
        assert np.array_equal(getattr(go, k).numpy(), getattr(T, k)), k
    odd = H.tables(c._replace(opt=c.opt + "x"))
    real = (odd.order >= 1) & (odd.order < odd.V)
    assert np.array_equal(np.where(real, odd.order, 0), T.order) and np.array_equal(np.sort(odd.order[real]), np.arange(1, T.V))      # every id exactly once
    if c.csr and c.U <= 300:
        cr = H.resolve(c, T)
        I = H.cap_inputs(cr, T)
        lists = ops.ExclusionLists([torch.from_numpy(np.asarray(s, np.int64)) for s in I.segs], device="cpu")
        pl = go.positions(lists)
        off, x = H.position_lists(T, I.segs)
        n = int(off[-1]) - 7
        assert np.array_equal(pl.offsets.numpy()[:-1], off[:-1]) and np.array_equal(pl.ids.numpy()[:n], x[:n])
        boff, bx = go.by_position(lists)
        off, x = H.lists_by_position(T, I.segs, c.U)
        assert np.array_equal(boff.numpy()[:-1], off[:-1]) and np.array_equal(bx.numpy(), x[:-1])


# ------------------------------------------------------------------------------------------ (c) routes and shapes
def _routes(entry):
    out = []
    for c in CASES.values():
        T = H.tables(c)
        out.append(H.ROUTE_FN[entry](H.resolve(c, T), T))
    return out


@pytest.mark.parametrize("entry", H.STREAM)
def test_two_cases_on_every_stream_route(entry):
    H._count_routes(_routes(entry), H.ROUTES[entry], entry)


def test_two_cases_on_every_row_route_and_the_table_holds_the_sizes():
    H._count_routes([H.row_route(c) for c in ROWS.values()], H.ROW_ROUTES, "rows")
    cs = list(ROWS.values())
    assert {c.k for c in cs} >= set(H.ROW_KS) and {c.U for c in cs} >= set(H.ROW_US) and {c.cap for c in cs} >= set(H.ROW_CAPS) and {c.G for c in cs} >= set(H.ROW_GS)
    stream = list(CASES.values())
    assert {c.N for c in stream} >= set(H.CAP_NS) and {len(H.SIZES[c.sizes]) - 1 for c in stream} >= {1, 2, 64, 511, 512}
    assert {c.U for c in stream} >= {2, 3, 129, 130, 257, H.U_TWO} and {c.T for c in stream} >= {0, 1, 63, 64, 65, 127, 128}
    for tile, N in ((64, 36), (32, 832), (16, 1024)):
        assert {c.U for c in stream if c.N == N} >= {1, tile - 1, tile, tile + 1}, tile
    for want in (0, 1, 127, 128, 129):
        assert any(want in H.SIZES[c.sizes] for c in stream), want


def test_the_empty_slice_case_and_the_list_shapes():
    for kind in ("plateau", "gauss"):
        c = CASES[f"{kind}-empty-slice"]
        T = H.tables(c)
        c = H.resolve(c, T)
        sl = H.slices(T, H.plan("logzg", c, T).splits)
        lens = set(np.diff(T.seg_start).tolist())
        assert T.S == 2 and T.n_pos // 128 > 256 and lens == {128, 256}, (T.S, lens)
        assert any(lo >= hi for lo, hi in sl) and sorted(s for lo, hi in sl for s in range(lo, hi)) == list(range(T.nseg))      # every segment in exactly one slice
        assert c.splits not in (0, 1, T.nseg)
        assert any(lo >= hi for lo, hi in H.slices(T, H.plan("expectg", c, T).splits))
        c = CASES[f"{kind}-seek"]
        T = H.tables(c)
        c = H.resolve(c, T)
        I = H.cap_inputs(c, T)
        off, x = H.position_lists(T, I.segs)
        p0 = x[off[0]:off[1]]
        b = int(np.flatnonzero(T.cnt > 128)[0])
        lo = int(T.bin_start[b])
        assert ((p0 >= lo) & (p0 < lo + 128)).sum() == 128 and ((p0 >= lo + 128) & (p0 < lo + 256)).sum() == 65       # the refill loop
        start_last = int(T.seg_start[H.slices(T, 2)[1][0]])
        p1 = x[off[1]:off[2]]
        assert len(p1) > 32 and (p1 < start_last).all()                       # every entry before the last slice's start: the search
        c = CASES["gauss-N36"]
        T = H.tables(c)
        lens = {len(s) for s in H.cap_inputs(H.resolve(c._replace(csr=1, U=6), T), T).segs}
        assert {0, 1, 64, 65, 129} <= lens and max(lens) >= 290, lens


def test_the_by_position_lists_of_k22_hold_the_shapes():
    """Per position the users that list it: 0, 1, 64, 65, 129 (and 300) users, and one position with all 128 users of the first
    chunk and 65 of the second."""
    for name, most in (("gauss-u257", 129), ("plateau-u257", 129), ("gauss-two-user-chunks", 300), ("plateau-two-user-chunks", 300), ("gauss-u130-lists", 129)):
        c = CASES[name]
        T = H.tables(c)
        c = H.resolve(c, T)
        I = H.cap_inputs(c, T)
        off, x = H.lists_by_position(T, I.segs, c.U)
        per = [x[off[p]:off[p + 1] if p + 1 < T.n_pos else len(x) - 1] for p in range(T.n_pos)]
        lens = {len(l) for l in per}
        assert {0, 1, 64, 65, most} <= lens, (name, sorted(lens))
        assert all((np.diff(l) > 0).all() and l.min(initial=0) >= 0 and l.max(initial=0) < c.U for l in per), name
        if c.U >= 256:
            assert any((l < 128).sum() == 128 and ((l >= 128) & (l < 256)).sum() == 65 for l in per), name


def test_two_cases_carry_agree_and_special():
    agree, special = [], []
    for c in CASES.values():
        T = H.tables(c)
        c = H.resolve(c, T)
        I = H.cap_inputs(c, T)
        agree += [c.name] * H.carries_agree(c)
        special += [(c.name, sorted(set(I.special.values()))) for _ in range(H.carries_special(c, I))]
    assert len(agree) >= 2 and len(special) >= 2
    for kind in ("tau0", "tauneg", "taunan", "tauinf", "tautiny", "logsumnan", "omegainf", "gmaxinf", "posinf"):
        assert sum(kind in k for _, k in special) >= 2, (kind, special)


# ------------------------------------------------------------------------------------------ (d) the size queries
@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_the_size_queries_answer_the_restated_carve(name):
    c = CASES[name]
    T = H.tables(c)
    c = H.resolve(c, T)
    I = SimpleNamespace(tau=0.5, stamp=None, n_user=None)
    for e in H.STREAM:
        P = SimpleNamespace(entry=e, c=c, I=I, T=T, S=H.strides(c, T, "pad"), inb={}, outb={}, ws=SimpleNamespace(ptr=16), ws_bytes=0)
        need = ("news", "user", "order", "seg_start", "bin_seg", "bin_start", "base_max", "base_logsum", "bin_w", "out", "logsum", "max", "count")
        d, query, _ = H.descriptor(P, ptr=lambda P, name: 16 if name in need else None)
        assert query(C.byref(d)) == H.ws_bytes(e, c, T), (e, _lib.last_error())
        d.N = 353
        assert query(C.byref(d)) == 0 and "multiple of 4" in _lib.last_error()


# ------------------------------------------------------------------------------------------ (e) the sound stand-in
@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_the_sound_stand_in_passes_every_layer_of_a_stream_case(name):
    c = CASES[name]
    w = H.cap_sweep(c, DEV, standin(), layout=c.N <= 36 and c.U <= 300, agree=c.N <= 36)
    assert all(v <= 1.0 for v in w.values()), w


@pytest.mark.parametrize("name", list(ROWS), ids=str)
def test_the_sound_stand_in_passes_every_layer_of_a_row_case(name):
    w = H.row_sweep(ROWS[name], DEV, standin())
    assert all(v <= 1.0 for v in w.values()), w


# ------------------------------------------------------------------------------------------ (f) the mutants
MUTANTS = [  # (mutant, case, layer)
    ("padding_eligible", "gauss-empty-slice-nseg", "bound"), ("bin_seg_off_by_one", "gauss-N36", "bound"), ("lists_in_id_space", "plateau-seek", "exact"),
    ("prior_by_position", "plateau-N32", "exact"), ("stamp_by_position", "plateau-N28", "exact"), ("exp_rel_2m20_everywhere", "plateau-N4", "exact"),
    ("padding_row_partials", "gauss-tv-u2", "bound"), ("empty_slice_dropped", "plateau-empty-slice", "exact"), ("seam_twice", "plateau-empty-slice", "exact"),
    ("count_not_reset", "gauss-two-groups", "bound"), ("listed_65th_kept", "plateau-seek", "exact"), ("padded_out_stride", "plateau-g511", "sentinel"),
    ("omega_of_previous_bin", "plateau-N4", "exact"), ("nan_from_zero_omega", "gauss-N28", "special"), ("padding_weighted", "gauss-N32", "bound"),
    ("named_not_scaled", "plateau-g64", "exact"), ("finalize_reads_empty_slice", "gauss-empty-slice", "bound"), ("dense_ld_base", "gauss-N32", "bound"),
    ("bin_after_empty_wrong", "plateau-rows", "exact"), ("bases_user_major", "gauss-tv-u2", "bound"), ("named_gated_by_base", "gauss-g64", "bound"),
    ("dead_pair_nan", "gauss-N28", "special"), ("row0_partials", "plateau-N36", "exact"), ("user_seam_twice", "plateau-u257", "exact"),
    ("ws_overrun", "gauss-N4", "sentinel"), ("one_bit_second_run", "gauss-N4", "repeat"), ("stride_dependent", "gauss-N36", "layout"),
]


@pytest.mark.parametrize("mutant,name,layer", MUTANTS, ids=lambda v: str(v))
def test_each_stream_mutant_fails_at_its_layer(mutant, name, layer):
    with pytest.raises(H.CappedCheckError) as e:
        H.cap_sweep(CASES[name], DEV, standin(mutant))
    assert e.value.layer == layer, (mutant, str(e.value))


ROW_MUTANTS = [
    ("cap_late", "rows-hand-cap1", "exact"), ("cap_early", "rows-hand-cap3", "exact"), ("key0_counts_as_live", "rows-hand-cap3", "exact"),
    ("blocked_zero", "rows-hand-cap1", "tight"), ("closed_full_q", "rows-hand-cap3", "tight"), ("q_after_close", "rows-hand-cap1", "tight"),
    ("id_ge_G_is_a_group", "rows-G1", "exact"), ("no_group_bin_capped", "rows-hand-cap1", "exact"), ("k_for_ld_ids", "rows-k64-0", "exact"),
    ("k_for_ld_g", "rows-hand-cap1", "tight"), ("dense_ld_base", "rows-k63-1", "exact"), ("dense_out_ld_base", "rows-k63-1", "sentinel"),
    ("total_finite_beside_blocked", "rows-cap127", "exact"), ("blocked_after_close", "rows-hand-cap1", "tight"), ("exclusive_scan", "rows-hand-cap3", "tight"),
    ("blocked_g_read", "rows-hand-cap1", "tight"),
]


@pytest.mark.parametrize("mutant,name,layer", ROW_MUTANTS, ids=lambda v: str(v))
def test_each_row_mutant_fails_at_its_layer(mutant, name, layer):
    with pytest.raises(H.CappedCheckError) as e:
        H.row_sweep(ROWS[name], DEV, standin(mutant))
    assert e.value.layer == layer, (mutant, str(e.value))


@pytest.mark.parametrize("name", [n for n in SMALL if CASES[n].kind == "gauss" and CASES[n].N <= 36], ids=str)
def test_an_exponential_wrong_by_2m20_passes_every_header_bound(name):
    """The gap this sweep closes: on Gaussian data the bounds of the header are too wide to see it."""
    H.cap_sweep(CASES[name], DEV, standin("exp_rel_2m20"), layout=False, agree=False)


@pytest.mark.parametrize("name,key", [("plateau-N32", "K20"), ("plateau-N36", "K22")], ids=str)
def test_an_exponential_wrong_by_2m20_fails_tight_on_plateau_data(name, key):
    with pytest.raises(H.CappedCheckError) as e:
        H.cap_sweep(CASES[name], DEV, standin("exp_rel_2m20"), layout=False)
    assert e.value.layer == "tight" and key in str(e.value), str(e.value)

"""GPU: every route of the full-softmax training calls that stream the corpus per user, through the C ABI: nr_score_logz (K13),
nr_score_entropy (K23), nr_score_expect (K17) and nr_score_expect_affine (K24) with their four size queries (include/nrhip.h;
csrc/nr_logz.hip, nr_entropy.hip, nr_expect.hip over csrc/nr_logz_stream.h and csrc/nr_score_tile.h), of the named-row pair
nr_row_logprob (K14) and nr_row_logprob_grad (K19) and of the news side nr_score_expect_news (K18, rows and mass-only) and
nr_score_expect_news_affine (K25) with their size queries; the parts "6 the named-row calls" and "7 the news side" carry their
own descriptions and bounds.  Built like
tests/test_gpu_corpus_sweep.py, whose helpers it imports.  The case table, one route function per entry point (its dispatch
restated), the input builder, the float64 reference, the descriptors' buffers and the checker are the first part of this file
("softmax sweep"; plain numpy and torch, no GPU needed); tests/test_softmax_sweep_host.py imports them and proves on the CPU that
the checker passes a sound fp32 stand-in and fails each of its mutants at the layer named.  The second part calls the C ABI with
the ctypes descriptors of _lib.py.  One case runs all four calls: K13 first, then K23, K17 and K24 on the base K13 returned.

Buffers.  Every device array, inputs included, is one allocation [guard][payload][guard] (glue_buf of the glue sweep).  Vector
bases and `out` are 16-byte aligned and no more, int32 and per-user fp32 arrays 4-byte aligned, the workspace 8-byte aligned and
exactly as long as the size query answered -- which must equal the restated carve and plan (`wsize`).  Outputs start as NaN
(integers: -77).  Every case runs with padded strides: ld_news and ld_user two different ones of {N, N + 4, tk_npad(N) + 8}, ld_out
in {N, N + 4}, ld_sub in {T, T + 3}, ld_window in {2, 5}.  The slack is poison that changes the answer when read: NaN in vector
slack and in `out` slack, a valid id with weight 1e30 in sub_ids / sub_w slack, an empty window in window slack; news row 0 holds
3e37.  `sentinel`: after the call every guard and slack element of every buffer compares bit for bit.  `repeat`: two problems built
alike give the same bits.  `layout`: the same case with the widths as strides, and with every base moved (16 bytes for vectors and
`out`, 8 for the workspace, 4 for the rest), gives the same bits.

Data kinds.
  plateau  news entries integers in [-2, 2], user entries 128 times integers in [-2, 2], priors multiples of 128 (<= 0),
           temperatures from {1/4, 1/2, 1}: every score is exact in fp32 and every (s - max) / tau is 0 or <= -128, so every fp32
           exponential the device forms is exactly 1 or exactly 0 (the host file asserts the condition from the reference).  User u
           is 128 r_g, g = u mod 3, r_g a row of +-2; the m_g news planted for group g are copies of r_g and no other row is, so by
           Cauchy-Schwarz they are exactly the user's maxima, spread over lanes, chunks, segments and slices by a permutation (one
           case keeps them in one chunk).  m is drawn from {1, 2, 3, 64, 129}.  Lists, windows and -inf priors then take some of
           them away (in every CSR case user 1 lists ALL its planted news, so leaving them out changes out_max); the number of
           maxima a user is left with, m_u, comes from the reference.
           `exact`: out_max and out_count equal the reference; out_logsum is +0.0 for m_u = 1, else float32(log m_u) or its
           neighbour.  For m_u = 1, as numbers: K17 row u = fl32((weight_u news[best_u] - sum_t sub_w news[sub_ids]) / tau), mass
           1.0; K23 H = 0, var = 0, mass = 1; K24 the same with alpha_u in place of weight_u (x = -0: beta has no part).
           `tight` for m_u > 1 (e = 2^-24).  The score chain term 2 (N + 1) G, the exponent term 6 C and the lane chain 7 K of the
           header's kappa all vanish: scores and sums of ones are exact.  What is left: l = out_logsum is within 3 e ln m of ln m
           (one rounding, e, or its neighbour, 2 e more), which moves p = expf(-l) by 3 e ln m relatively; expf is within 3 ulp =
           6 e; so p = (1 + t) / m with |t| <= TH = (6 + 3 ln m) e.  The products p n_vc are exact (|n_vc| in {0, 1, 2}); the
           contraction adds m non-zero terms in fp32: (m - 1) e; slices, weight and named rows in fp64; one rounding to fp32: e; e
           for the second order.  K17:  |out_c - out*_c| <= (m + 3 ln m + 7) e A_c,  A_c = (|w| sum_v p*_v |n_vc| + sum_t |sub_w|
           |news[sub_ids]_c|) / tau.  K24 adds the fma of the weight and its product with p, 2 e, and the error 3 e ln m of x in the
           weight, which the `+ 1` beside |x*| in the header's A_c carries: m + 3 ln m + 9.  Masses (fp64 sums of m equal p, one
           rounding, second order): |mass - 1| <= (3 ln m + 8) e.  K23: H = (1 + t) l, |H - ln m| <= (3 ln m + 11) e ln m;
           var = m2 - m1^2 = -t (1 + t) l^2, |var| <= (3 ln m + 8) e (ln m)^2.  For m = 129 the chain term dominates and the
           bound is no tighter than the header's; for m = 2, 3 it is 11 and 14 units against a kappa of 154 and more.
  gauss    Gaussian vectors, flat users (scores within 1e-3 of each other per tau), ordinary and peaked ones (a range in the
           thousands) inside one call.  `bound`: the bounds of include/nrhip.h as tests/test_gpu_logz.py (logz_bound),
           test_gpu_expect.py (kappa, kappa_mass) and test_gpu_entropy.py (entropy_bounds, kappa_affine) state them, imported,
           against float64 on the fp32 inputs.  The named rows and 1 / tau add 2 e (|w| A_c + sum_t |sub_w| |news_c|) / tau: the
           final rounding and fl(1 / tau).  SOFTMAX_EXCESS scales every bound if the device ever exceeds one.
           `agree`, bit for bit at one explicit `splits`: K13's three outputs for splits = 0, 1, 2 and nseg; K13's out_max = the
           score nr_score_topk returns for k = 1 under the same pools and lists; K24 with alpha = 1, beta = 0 = K17 with weight
           NULL; row u of K17 / K23 / K24 when every other user of the call is replaced.
  special  hand-made users and news inside a Gaussian call (`special`): nothing eligible (an empty window); a +inf maximum; a
           -inf maximum (K13: max -inf, count 1, logsum NaN; K17 / K23 / K24 read base_max = -inf as nothing eligible: zeros and
           mass 0); a NaN base_logsum handed to K17 / K23 / K24 (NaN for that user); a
           -inf score under a finite maximum (counts 1, weighs 0, a term of no entropy sum); a NaN news row and a news row with one
           infinite component (0 in E); a prior of -inf; tau_u entries 0, -1, NaN, +inf and the smallest normal (1 / tau
           overflows: the weights of the limit); NaN alpha and NaN beta (that user's K24 row NaN, its mass not); sub_ids fill (0,
           negative, >= V) and a repeated id.  NaN sits exactly where the reference has it, the rest is within `bound`, and the
           ordinary users' bits equal those of the same call without the special users.

Layers of SoftmaxCheckError: sentinel, repeat, layout, wsize, exact, tight, bound, agree, special.
Routes, derivations, measured figures and what stays uncovered (the capped calls): DESIGN.md "Full-softmax training calls: routes as verified and the sweep".
"""
import collections
import ctypes as C
import math
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_corpus_sweep as CS
import test_gpu_entropy as GH
import test_gpu_expect as GE
import test_gpu_glue_sweep as GL
import test_gpu_logz as GZ
from test_gpu_corpus_sweep import auto_splits, tk_npad, user_tile
from test_gpu_glue_sweep import _bits, _count_routes, _sentinels, glue_buf
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------ softmax sweep
EPS = 2.0 ** -24
# What the device adds beyond a bound of include/nrhip.h, as a fraction of it: four times the worst excess measured over the sweep
# on the MI355X against fp64, 0 when there is none (DESIGN.md holds the measured ratios).
SOFTMAX_EXCESS = 0.0
LAYERS = ("sentinel", "repeat", "layout", "wsize", "exact", "tight", "bound", "agree", "special")
ENTRIES = ("logz", "entropy", "expect", "affine")
NAN, INF = float("nan"), float("inf")
IFILL = -77
TINY = float(np.finfo(np.float32).tiny)
f32, f64, i32 = np.float32, np.float64, np.int32
_rng = CS._rng


class SoftmaxCheckError(AssertionError):
    """A failed check of the sweep; `.layer` is one of LAYERS."""

    def __init__(self, layer, msg):
        assert layer in LAYERS, layer
        super().__init__(f"[{layer}] {msg}")
        self.layer = layer


def need(ok, layer, msg, *a):
    if not ok:
        raise SoftmaxCheckError(layer, msg.format(*a) if a else msg)


def same_bits(layer, name, got, ref):
    try:
        CS.same_bits("exact", name, got, ref)
    except CS.CorpusCheckError as e:
        raise SoftmaxCheckError(layer, str(e)) from None


def _sent(name, b):
    try:
        _sentinels(name, b)
    except GL.GlueCheckError as e:
        raise SoftmaxCheckError("sentinel", str(e)) from None


# ---------------------------------------------------------------------------------------- 0 the plans, restated
EX_PER_USER = (128 + 4) * 4                    # a user's row of the P tile beside the scoring tile (EX_PER_USER, AF_PER_USER)


def lz_plan_tile(U, V, TU, splits):
    """lz_plan_tile of csrc/nr_logz_stream.h: segments are a function of V alone, a slice is a run of whole segments, no slice is
    empty."""
    per = 128 * 256
    seg = 128 * ((V - 1 + per - 1) // per)
    nseg = (V - 1 + seg - 1) // seg
    s = splits if splits > 0 else auto_splits(U, V, TU, 256)
    s = max(1, min(s, nseg))
    segs_per = (nseg + s - 1) // s
    return SimpleNamespace(TU=TU, seg=seg, nseg=nseg, segs_per=segs_per, splits=(nseg + segs_per - 1) // segs_per)


def stream_tile(N):
    """K13 and K23: score_user_tile(N, 0) -- 64 users up to N = 480, 32 up to 960, else 16."""
    return user_tile(N, 0)


def contract_tile(N):
    """K17 and K24: score_user_tile(N, a row of P) -- 64 users up to 11 k-slabs (N <= 352), 32 up to 26 (N <= 832), else 16 (32)."""
    return user_tile(N, EX_PER_USER)


KMAX = {64: 11, 32: 26, 16: 32}


def plan(entry, c):
    return lz_plan_tile(c.U, c.V, stream_tile(c.N) if entry in ("logz", "entropy") else contract_tile(c.N), c.splits)


def ws_bytes(entry, c):
    """lz_carve: U * nseg * 12, rounded to 8; en_carve: U * slices * 24; ex_carve / af_carve: U * slices * (4 N + 8), rounded."""
    p = plan(entry, c)
    if entry == "logz":
        return (c.U * p.nseg * 12 + 7) // 8 * 8
    if entry == "entropy":
        return c.U * p.splits * 24
    return (c.U * p.splits * (4 * c.N + 8) + 7) // 8 * 8


# ---------------------------------------------------------------------------------------- 1 the case table and the routes
# pool: 0 none, 1 prior + stamps and windows, 2 prior only, 3 stamps and windows only.  csr: 0 no lists, 1 segments of lengths 0, 1,
# 64, 65, 129, 300, 2 the same with three hand-made users in front (see _lists).  taus: per-user temperatures.  m: maxima planted
# for the first user group (plateau).  T: named rows per user (0: sub_ids / sub_w NULL).  opt: w = weight / alpha given, b = beta
# given, s = scale_inv_tau, v = out_var given, M = the optional masses given, c = the planted news in one chunk.
SmCase = collections.namedtuple("SmCase", "name kind N U V splits pool csr taus m T opt pad")
SM_NS = (4, 28, 32, 36, 352, 356, 480, 484, 832, 836, 960, 964, 1020, 1024)
# The first widths past a tile boundary as plain arithmetic names them.  The library takes multiples of 4 only (check_vectors), so
# these are refused before any launch -- the sweep asserts that -- and the first width a next tile really sees is the one above.
REFUSED_NS = {353: 356, 481: 484, 833: 836, 961: 964}
SM_VS = (2, 3, 129, 130, 257, 294)
V_TWO = 1 + 128 * 256 + 5                      # two chunks per segment, 129 segments
SM_TS = (1, 63, 64, 65, 127, 128)
SM_MS = (1, 2, 3, 64, 129)
CSR_LENGTHS = CS.CSR_LENGTHS
OPTS = ("wbsvM", "", "wM", "bv", "sM", "wbs")
SPECIAL_USERS = ("empty", "posinf", "tau0", "tauneg", "taunan", "tauinf", "tautiny", "alphanan", "betanan", "neginf", "nanbase")

_STREAM = tuple(f"tile_{t}" for t in (64, 32, 16)) + tuple(f"p{p}l{l}" for p in (0, 1) for l in (0, 1)) + (
    "splits_auto", "splits_given", "short_last_slice", "two_chunk_segments", "tau_scalar", "tau_u")
LOGZ_ROUTES = _STREAM
ENTROPY_ROUTES = _STREAM + ("var_null", "var_given", "mass_null", "mass_given")
_CONTRACT = _STREAM + tuple(f"kmax_{k}" for k in (11, 26, 32)) + ("sub_null", "sub_given", "scale_0", "scale_1", "mass_null", "mass_given")
EXPECT_ROUTES = _CONTRACT + ("weight_null", "weight_given")
AFFINE_ROUTES = _CONTRACT + ("alpha_null", "alpha_given", "beta_null", "beta_given")
ROUTES = {"logz": LOGZ_ROUTES, "entropy": ENTROPY_ROUTES, "expect": EXPECT_ROUTES, "affine": AFFINE_ROUTES}


def _u_of(tile, j):
    return (1, tile - 1, tile, tile + 1)[j % 4]


def sm_cases():
    cs, i = [], 0
    for kind in ("plateau", "gauss"):
        for N in SM_NS:                                                       # every width, the tiled axis around the tile of either pair
            tile = contract_tile(N) if i % 2 else stream_tile(N)
            V = SM_VS[(i + i // 6) % 6]
            cs.append(SmCase(f"{kind}-N{N}", kind, N, _u_of(tile, i + i // 4), V, (0, 1, 2, 3)[(i + i // 4) % 4], i % 4, (0, 1)[(i // 2) % 2] if V >= 129 else 0,
                             i % 2, SM_MS[i % 5], (0, SM_TS[i % 6])[(i // 3) % 2], OPTS[i % 6], i % 3))
            i += 1
    for kind in ("plateau", "gauss"):
        for j, tile in enumerate((64, 32, 16)):                               # U = 1, TU - 1, TU, TU + 1 of every tile, of both pairs
            for N in {64: (36, 352), 32: (832, 960), 16: (836, 1024)}[tile]:
                for jj in range(2):
                    q = 2 * j + jj + (N % 5)
                    u = _u_of(tile, 2 * (N % 2) + jj + (kind == "gauss") * 2)
                    cs.append(SmCase(f"{kind}-tile{tile}-N{N}-u{u}", kind, N, u, SM_VS[2 + q % 4], (2, 0, 3, 1)[q % 4], (3, 0, 2, 1)[q % 4], q % 2, (q + 1) % 2,
                                     SM_MS[q % 5], (0, SM_TS[(q + 2) % 6])[q % 2], OPTS[(q + 3) % 6], q % 3))
    for kind in ("plateau", "gauss"):
        cs += [SmCase(f"{kind}-two-chunks-auto", kind, 4, 3, V_TWO, 0, 1, 1, 1, 64, 65, "wbsvM", 1),              # two chunks per segment; the library's slices
               SmCase(f"{kind}-two-chunks-nseg", kind, 36, 2, V_TWO, 129, 0, 0, 0, 129, 0, "M", 2),              # one segment per slice
               SmCase(f"{kind}-two-chunks-short", kind, 4, 5, V_TWO, 8, 3, 0, 1, 3, 128, "wv", 0),               # 17 segments per slice, 10 in the last
               SmCase(f"{kind}-seek", kind, 36, 5, 294, 2, 0, 2, 0, 3, 1, "wbM", 1),                             # lists: 128 and 65 ids listed in a chunk; LZ_SEEK
               SmCase(f"{kind}-seek-pool", kind, 32, 17, 294, 2, 1, 2, 1, 2, 64, "sv", 2),
               SmCase(f"{kind}-nseg-3", kind, 28, 9, 294, 3, 2, 1, 1, 64, 0, "bM", 0)]
    cs += [SmCase("plateau-one-chunk", "plateau", 36, 7, 294, 2, 0, 0, 0, 64, 0, "wbvMc", 1),                   # all maxima in one chunk
           SmCase("plateau-m129-lists", "plateau", 352, 4, 257, 2, 3, 1, 0, 129, 127, "wsM", 2),
           SmCase("special-a", "special", 36, 16, 294, 2, 1, 1, 1, 0, 5, "wbvM", 1),
           SmCase("special-b", "special", 4, 16, 130, 1, 1, 0, 1, 0, 5, "wbsvM", 2)]
    assert len({c.name for c in cs}) == len(cs)
    return [c._replace(splits=min(c.splits, lz_plan_tile(c.U, c.V, 64, 1).nseg)) for c in cs]      # more slices than segments are refused


def _stream_route(entry, c):
    p = plan(entry, c)
    r = [f"tile_{p.TU}", f"p{int(bool(c.pool))}l{int(bool(c.csr))}", "splits_given" if c.splits else "splits_auto", "tau_u" if c.taus else "tau_scalar"]
    if c.splits and p.nseg % p.segs_per:
        r.append("short_last_slice")
    if p.seg > 128:
        r.append("two_chunk_segments")
    return r


def logz_route(c):
    """nr_score_logz: logz_stream_kernel<MT, POOL, LISTS> on the tile of score_user_tile(N, 0) (a CSR call is one with n_excl > 0),
    then logz_final_kernel over the nseg partials of a user."""
    return tuple(_stream_route("logz", c))


def entropy_route(c):
    """nr_score_entropy: entropy_stream_kernel<MT, POOL, LISTS> on K13's tile, entropy_final_kernel; out_var and out_mass optional."""
    return tuple(_stream_route("entropy", c) + ["var_given" if "v" in c.opt else "var_null", "mass_given" if "M" in c.opt else "mass_null"])


def _contract_route(entry, c):
    p = plan(entry, c)
    r = _stream_route(entry, c)
    if tk_npad(c.N) // 32 == KMAX[p.TU]:
        r.append(f"kmax_{KMAX[p.TU]}")                                        # the last k-slab the instantiation unrolls
    return r + ["sub_given" if c.T else "sub_null", "scale_1" if "s" in c.opt else "scale_0", "mass_given" if "M" in c.opt else "mass_null"]


def expect_route(c):
    """nr_score_expect: expect_stream_kernel<MT, KMAX, POOL, LISTS> as <4, 11>, <2, 26>, <1, 32> on the tile of score_user_tile(N, a
    row of P), then expect_final_kernel (weight, named rows, 1 / tau)."""
    return tuple(_contract_route("expect", c) + ["weight_given" if "w" in c.opt else "weight_null"])


def affine_route(c):
    """nr_score_expect_affine: affine_stream_kernel<MT, KMAX, POOL, LISTS> with K17's tiles and slab counts, affine_final_kernel."""
    return tuple(_contract_route("affine", c) + ["alpha_given" if "w" in c.opt else "alpha_null", "beta_given" if "b" in c.opt else "beta_null"])


ROUTE_FN = {"logz": logz_route, "entropy": entropy_route, "expect": expect_route, "affine": affine_route}


# ---------------------------------------------------------------------------------------- 2 inputs
def _lists(c, V, U, rng, must=None):
    """CSR lists.  csr = 1: user u's segment has length CSR_LENGTHS[...], strictly ascending, drawn from [-L, V + L) so that entries
    <= 0 and >= V sit at its two ends.  csr = 2 (V >= 294, U >= 3, slice 1 of `splits` >= 2 starts at id 257): user 0 lists every id
    of the chunk [1, 129) and 65 ids of [129, 257) -- the refill loop of LZ_LISTED, and all its entries lie before slice 1; user 1
    lists 100 ids below 257 and 30 from 257 on (LZ_SEEK with steps > 1 that ends inside the segment); user 2 lists only ids from
    257 on (no probe below the slice start).  must: {user: ids} merged into that user's segment.  The last offset exceeds n_excl."""
    segs = []
    for u in range(U):
        L = CSR_LENGTHS[(u + 1) % 6] if U < 6 else CSR_LENGTHS[u % 6]
        segs.append(np.sort(rng.choice(np.arange(-L, V + L), L, replace=False)).astype(i32))
    if c.csr == 2:
        assert V >= 294 and U >= 3
        segs[0] = np.concatenate([np.arange(1, 129), 129 + np.sort(rng.choice(128, 65, replace=False))]).astype(i32)
        segs[1] = np.concatenate([np.sort(rng.choice(np.arange(1, 257), 100, replace=False)), np.sort(rng.choice(np.arange(257, V), 30, replace=False))]).astype(i32)
        segs[2] = np.sort(rng.choice(np.arange(257, V), 20, replace=False)).astype(i32)
    for u, ids in (must or {}).items():
        segs[u] = np.unique(np.concatenate([segs[u], np.asarray(ids, i32)])).astype(i32)
    xids = np.concatenate(segs + [np.zeros(0, i32)]).astype(i32)
    if xids.size == 0:
        xids = np.array([V + 1], i32)
        segs[-1] = xids
    off = np.zeros(U + 1, i32)
    off[1:] = np.cumsum([len(s) for s in segs])
    off[U] += 7
    return off, xids, segs


def _pools(c, I, rng, plateau):
    V, U = c.V, c.U
    if c.pool in (1, 2):
        I.prior = (128.0 * rng.integers(-2, 1, V)).astype(f32) if plateau else rng.standard_normal(V).astype(f32)
        I.prior[3::7] = -INF
    if c.pool in (1, 3):
        lo = rng.integers(0, 4, U)
        I.stamp, I.window = rng.integers(0, 10, V).astype(i32), np.stack([lo, lo + rng.integers(3, 7, U)], axis=1).astype(i32)
        if U >= 3 and c.kind != "special":
            I.window[2] = (5, 4)                                              # lo > hi: nobody


def sm_inputs(c):
    """Everything the four calls of a case read, as plain numpy arrays in their logical shapes."""
    rng = _rng(11, c.N, c.U, c.V, c.splits, c.pool, c.csr, c.taus, c.m, c.T, c.pad, len(c.opt), c.kind == "gauss")
    V, U, N = c.V, c.U, c.N
    I = SimpleNamespace(prior=None, stamp=None, window=None, offsets=None, xids=None, segs=None, tau=(0.25, 0.5, 1.0)[(N + U) % 3], tau_u=None, weight=None, beta=None,
                        sub_ids=None, sub_w=None, planted={}, special={})
    must = {}
    if c.kind == "plateau":
        G = max(1, min(3, U, V - 1))
        pats = []
        while len(pats) < G:
            r = rng.choice(np.array([-2, 2]), N)
            if not any((r == q).all() for q in pats):
                pats.append(r)
        ms = [min(c.m, V - 1)] + [SM_MS[(c.m + g) % 3] for g in range(1, G)]
        while sum(ms) > V - 1:
            ms[int(np.argmax(ms))] -= 1
        perm = 1 + rng.permutation(min(V - 1, 128) if "c" in c.opt else V - 1)
        news = rng.integers(-2, 3, (V, N))
        for r in pats:
            news[(news == r).all(axis=1), 0] = 0
        at = 0
        for g, r in enumerate(pats):
            I.planted[g] = np.sort(perm[at:at + ms[g]])
            news[I.planted[g]] = r
            at += ms[g]
        I.news, I.user = news.astype(f32), np.stack([128.0 * pats[u % G] for u in range(U)]).astype(f32)
        I.group = np.arange(U) % G
        if c.csr and U >= 2:
            must[1] = I.planted[1 % G]                                        # a user whose maxima are all listed
    else:
        I.news = rng.standard_normal((V, N)).astype(f32)
        scale = np.array([1e-3, 1.0, 300.0])[np.arange(U) % 3]               # flat, ordinary, peaked
        I.user = (rng.standard_normal((U, N)) * (scale / math.sqrt(N))[:, None]).astype(f32)
        I.tau = (0.5, 0.7, 1.3)[(N + U) % 3]
    I.news[0] = 3e37
    _pools(c, I, rng, c.kind == "plateau")
    if c.kind == "plateau" and I.prior is not None:
        for ids in I.planted.values():
            I.prior[ids] = np.where(np.isneginf(I.prior[ids]), I.prior[ids], f32(0))
    if c.csr:
        I.offsets, I.xids, I.segs = _lists(c, V, U, rng, must)
    if c.taus:
        I.tau_u = (np.array([0.25, 0.5, 1.0], f32) if c.kind == "plateau" else np.array([0.3, 1.7, 0.75], f32))[rng.integers(0, 3, U)]
    if "w" in c.opt:
        I.weight = np.array([0.75, -2.0, 1.0, 3.0], f32)[rng.integers(0, 4, U)] if c.kind == "plateau" else rng.standard_normal(U).astype(f32)
    if "b" in c.opt:
        I.beta = np.array([-0.5, 1.0, 0.0, 2.0], f32)[rng.integers(0, 4, U)] if c.kind == "plateau" else rng.standard_normal(U).astype(f32)
    if c.T:
        I.sub_ids = rng.integers(-1, V + 2, (U, c.T)).astype(i32)              # fill at both ends of the id range
        I.sub_w = (rng.integers(-8, 9, (U, c.T)) / 4.0).astype(f32) if c.kind == "plateau" else rng.standard_normal((U, c.T)).astype(f32)
        if c.T >= 2:
            I.sub_ids[:, 1] = I.sub_ids[:, 0]                                  # a repeated id is two entries
    if c.kind == "special":
        _make_special(c, I)
    return I


def _make_special(c, I):
    """The hand-made users and news of the module docstring; every third user stays ordinary (I.special maps user -> what it is)."""
    assert c.U >= 16 and c.V >= 130 and c.taus and c.pool == 1 and "w" in c.opt and "b" in c.opt and c.T >= 5
    N = c.N
    for j, name in enumerate(SPECIAL_USERS):
        I.special[j + j // 2] = name                                          # users 0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 15
    I.special = {u: n for u, n in I.special.items() if u < c.U}
    I.news[5] = NAN                                                           # a NaN news row: a term of nothing
    I.news[6, N - 1] = INF                                                    # one infinite component: NaN or infinite score for everyone, 0 in E
    I.news[7] = 0.0
    I.news[7, 0] = -INF                                                       # a -inf score (or +inf, or NaN) by the sign of user component 0
    I.prior[8] = -INF
    I.prior[7] = 0.0
    I.stamp[7], I.stamp[9] = 3, 3
    I.news[10], I.prior[10], I.stamp[10] = I.news[7], 0.0, 11                 # a second -inf score, in the window of the `neginf` user alone
    I.user[:, N - 1] = 0.0                                                    # news 6 scores NaN (0 * inf) for everyone
    I.user[:, 0] = np.abs(I.user[:, 0]) + f32(1e-3)                          # news 7 scores -inf for everyone: counts 1, weighs 0
    I.window[:] = (0, 9)
    I.sub_ids[:, :5] = np.array([0, -3, c.V, 9, 9], i32)                     # fill of every kind and a repeated id
    I.sub_ids[14, 4], I.sub_w[14, 4] = 6, 1.0                                 # an ordinary user names the row with the infinite component: -inf in that column alone
    for u, name in I.special.items():
        if name == "empty":
            I.window[u] = (5, 4)
        elif name == "posinf":
            I.user[u, 0] = -I.user[u, 0]                                      # news 7 scores +inf: max +inf, logsum NaN, the rows NaN
        elif name.startswith("tau"):
            I.tau_u[u] = {"tau0": 0.0, "tauneg": -1.0, "taunan": NAN, "tauinf": INF, "tautiny": TINY}[name]
        elif name == "neginf":
            I.window[u] = (11, 11)                                            # its one eligible score is -inf: max -inf, count 1, logsum NaN; K17 / K23 / K24 zeros
        elif name == "alphanan":
            I.weight[u] = NAN
        elif name == "betanan":
            I.beta[u] = NAN


# ---------------------------------------------------------------------------------------- 3 the float64 reference
def taus(c, I):
    """[U] fp32 temperatures and the mask of the valid ones (finite and > 0)."""
    tau = I.tau_u if I.tau_u is not None else np.full(I.user.shape[0], I.tau, f32)
    with np.errstate(invalid="ignore"):
        return tau, (tau > 0) & (tau < INF)


def eligible(I):
    """[U, V] bool: id in [1, V), prior not -inf, stamp inside the window, not listed.  (A NaN score is taken out where the scores
    are formed.)"""
    U, V = I.user.shape[0], I.news.shape[0]
    el = np.ones((U, V), bool)
    el[:, 0] = False
    if I.prior is not None:
        el &= ~np.isneginf(I.prior)[None, :]
    if I.stamp is not None:
        el &= (I.window[:, :1] <= I.stamp[None, :]) & (I.stamp[None, :] <= I.window[:, 1:2])
    if I.segs is not None:
        for u in range(U):
            ex = I.segs[u]
            el[u, ex[(ex >= 1) & (ex < V)]] = False
    return el


def sm_reference(c, I):
    """The contract of the four calls in float64 on the fp32 inputs, per user: smax, count, logsum (K13); H, var, mass (K23); E =
    sum p n, AE = sum p |n| (K17, before weight); F = sum p (alpha + beta x) n, AF = sum p (|alpha| + |beta| (|x| + 1)) |n| (K24);
    S = sum_t sub_w news[sub_ids], AS its absolute sum; the statistics n, C, G of the header's bounds (mag = G tau); m = eligible news at the
    maximum; dmin = the largest (s - max) / tau below 0.  nan[u]: a bad temperature or a maximum that is not finite."""
    U, V, N = I.user.shape[0], I.news.shape[0], I.news.shape[1]
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    clean = np.where(np.isfinite(n64), n64, 0.0)
    with np.errstate(all="ignore"):
        s = u64 @ n64.T
        mag = np.abs(u64) @ np.abs(n64).T
        if I.prior is not None:
            s, mag = s + I.prior.astype(f64)[None, :], mag + np.abs(I.prior.astype(f64))[None, :]
    el = eligible(I) & ~np.isnan(s)
    tau, tau_ok = taus(c, I)
    al = I.weight.astype(f64) if I.weight is not None else np.ones(U)
    be = I.beta.astype(f64) if I.beta is not None else np.zeros(U)
    R = SimpleNamespace(smax=np.full(U, -INF), count=np.zeros(U, np.int64), logsum=np.full(U, -INF), H=np.zeros(U), var=np.zeros(U), mass=np.zeros(U),
                        E=np.zeros((U, N)), AE=np.zeros((U, N)), F=np.zeros((U, N)), AF=np.zeros((U, N)), S=np.zeros((U, N)), AS=np.zeros((U, N)),
                        n=np.zeros(U), C=np.zeros(U), G=np.zeros(U), mag=np.zeros(U), m=np.zeros(U, np.int64), dmin=np.full(U, -INF), nan=np.zeros(U, bool), ninf=np.zeros(U, bool), best=np.zeros(U, np.int64),
                        tau=tau.astype(f64), tau_ok=tau_ok, al=al, be=be)
    for u in range(U):
        if I.sub_ids is not None:
            ids, w = I.sub_ids[u].astype(np.int64), I.sub_w[u].astype(f64)
            real = (ids >= 1) & (ids < V)
            for t in np.flatnonzero(real):                                  # the named rows as they are: a non-finite component reaches the output
                R.S[u], R.AS[u] = R.S[u] + w[t] * n64[ids[t]], R.AS[u] + abs(w[t]) * np.abs(n64[ids[t]])
        ok = el[u]
        x = s[u, ok]
        R.count[u] = R.n[u] = x.size
        if not x.size:
            continue
        R.smax[u] = x.max()
        R.m[u] = int((x == x.max()).sum())
        R.best[u] = int(np.flatnonzero(ok)[np.argmax(x)])
        R.mag[u] = mag[u, ok][np.isfinite(x)].max(initial=0.0)
        if np.isneginf(x.max()):                                              # a -inf maximum: K13 says logsum NaN, the others read base_max = -inf as nothing eligible
            R.ninf[u], R.logsum[u] = True, NAN
            continue
        if not tau_ok[u] or not np.isfinite(x.max()) or I.special.get(u) == "nanbase":
            R.nan[u] = True
            R.logsum[u] = R.H[u] = R.var[u] = R.mass[u] = NAN
            R.E[u] = R.AE[u] = R.F[u] = R.AF[u] = NAN
            continue
        t = float(tau[u])
        with np.errstate(all="ignore"):
            z = (x - x.max()) / t
            R.dmin[u] = z[z < 0].max() if (z < 0).any() else -INF
            lse = math.log(float(np.sum(np.exp(z))))
            xl = z - lse
            p = np.exp(xl)
            xs = np.where(p > 0, xl, 0.0)
            R.logsum[u] = lse
            m1 = float(np.sum(p * xs))
            R.H[u], R.var[u], R.mass[u] = -m1, float(np.sum(p * xs * xs)) - m1 * m1, float(np.sum(p))
            R.E[u], R.AE[u] = p @ clean[ok], p @ np.abs(clean[ok])
            R.F[u] = (p * (al[u] + be[u] * xs)) @ clean[ok]
            R.AF[u] = (p * (abs(al[u]) + abs(be[u]) * (np.abs(xs) + 1.0))) @ np.abs(clean[ok])
            fin = np.isfinite(x)
            R.C[u], R.G[u] = np.abs(x[fin]).max() / t, mag[u, ok][fin].max() / t
    return R


def finish(R, which, scale):
    """(out*, A of the body, A with the named rows) of K17 (`which` = expect: weight E - S) or K24 (affine: F - S), times 1 / tau
    when scaled, in float64."""
    w = R.al
    body, A = (w[:, None] * R.E, np.abs(w)[:, None] * R.AE) if which == "expect" else (R.F, R.AF)
    out, tot = body - R.S, A + R.AS
    if scale:
        with np.errstate(all="ignore"):
            out, tot, A = out / R.tau[:, None], tot / R.tau[:, None], A / R.tau[:, None]
    return out, A, tot


def plateau_condition(c, I, R):
    """Every score is a fp32 number and every (s - max) / tau is 0 or <= -128, for every user that has weights."""
    live = ~R.nan & (R.count > 0)
    return bool((R.dmin[live] <= -128.0).all() and (R.smax[live].astype(f32).astype(f64) == R.smax[live]).all())


# ---------------------------------------------------------------------------------------- 4 problems: the buffers of one call
def strides(c, variant):
    N, T = c.N, c.T
    if variant == "dense":
        return SimpleNamespace(news=N, user=N, out=N, sub=T, win=2)
    o = (N, N + 4, tk_npad(N) + 8)
    return SimpleNamespace(news=o[c.pad], user=o[(c.pad + 1) % 3], out=N + (4 if c.pad != 1 else 0), sub=T + (3 if c.pad != 2 else 0), win=5 if c.pad != 0 else 2)


in_buf = CS.in_buf


def out_buf(rows, cols, ld, tdt, dev, off):
    """An output [rows, cols] at row stride ld: NaN (integers: -77) in the payload and NaN in the slack, which must come back
    untouched."""
    b = glue_buf(rows, cols, ld, tdt, dev, off, NAN if tdt.is_floating_point else IFILL)
    if b.ld > cols:
        b.flat[b.start:b.start + rows * b.ld].view(rows, b.ld)[:, cols:] = NAN
        b.init = b.flat.clone()
    return b


def problem(entry, c, I, dev, variant="pad", base=None):
    """Every buffer of one call of `entry` on case c with inputs I; base = (out_max, out_logsum) of K13 for the other three.
    variant: pad (padded strides, the least alignment), dense (the widths as strides), shift (padded strides, every base moved)."""
    S, sh = strides(c, variant), variant == "shift"
    fo, io, wo = (0 if sh else 4), (2 if sh else 1), (4 if sh else 2)
    U, V, N = c.U, c.V, c.N
    P = SimpleNamespace(entry=entry, c=c, I=I, S=S, inb={}, outb={}, ws=None)
    P.inb["news"], P.inb["user"] = in_buf(I.news, S.news, dev, fo, NAN), in_buf(I.user, S.user, dev, fo, NAN)
    if I.prior is not None:
        P.inb["prior"] = in_buf(I.prior, V, dev, io)
    if I.stamp is not None:
        P.inb["stamp"] = in_buf(I.stamp, V, dev, io)
        P.inb["window"] = in_buf(I.window, S.win, dev, io, np.tile(np.array([100, -100, 100], i32), (U, 1)))
    if I.offsets is not None:
        P.inb["offsets"], P.inb["xids"] = in_buf(I.offsets, U + 1, dev, io), in_buf(I.xids, len(I.xids), dev, io)
    if I.tau_u is not None:
        P.inb["tau_u"] = in_buf(I.tau_u, U, dev, io)
    if entry == "logz":
        P.outb["logsum"], P.outb["max"], P.outb["count"] = (out_buf(1, U, U, t, dev, io) for t in (torch.float32, torch.float32, torch.int32))
    else:
        P.inb["base_max"], P.inb["base_logsum"] = in_buf(base[0], U, dev, io), in_buf(base[1], U, dev, io)
    if entry == "entropy":
        P.outb["H"] = out_buf(1, U, U, torch.float32, dev, io)
        if "v" in c.opt:
            P.outb["var"] = out_buf(1, U, U, torch.float32, dev, io)
    if entry in ("expect", "affine"):
        if I.weight is not None:
            P.inb["alpha"] = in_buf(I.weight, U, dev, io)                     # K17's weight, K24's alpha
        if entry == "affine" and I.beta is not None:
            P.inb["beta"] = in_buf(I.beta, U, dev, io)
        if I.sub_ids is not None:
            P.inb["sub_ids"] = in_buf(I.sub_ids, S.sub, dev, io, 1 if V > 1 else 0)
            P.inb["sub_w"] = in_buf(I.sub_w, S.sub, dev, io, 1e30)
        P.outb["out"] = out_buf(U, N, S.out, torch.float32, dev, fo)
    if entry != "logz" and "M" in c.opt:
        P.outb["mass"] = out_buf(1, U, U, torch.float32, dev, io)
    P.ws_bytes = ws_bytes(entry, c)
    P.ws = glue_buf(1, P.ws_bytes // 4, P.ws_bytes // 4, torch.int32, dev, wo, IFILL)
    if not sh:                                                                # the least alignment the header allows, and no more
        assert P.inb["news"].ptr % 32 == 16 and P.inb["user"].ptr % 32 == 16 and P.ws.ptr % 16 == 8 and P.inb["user"].ptr % 8 == 0
        assert "out" not in P.outb or P.outb["out"].ptr % 32 == 16
        assert all(b.ptr % 8 == 4 for k, b in list(P.inb.items()) + list(P.outb.items()) if k not in ("news", "user", "out"))
    return P


def all_bufs(P):
    return list(P.inb.items()) + list(P.outb.items()) + [("ws", P.ws)]


def results(P):
    return {k: b.v.cpu().numpy().copy() for k, b in P.outb.items()}


def execute(entry, c, I, dev, call, variant="pad", twice=True, base=None):
    """One checked call: every guard and slack element intact (`sentinel`), a second problem built alike gives the same bits
    (`repeat`).  Returns the outputs as numpy arrays."""
    Ps = [problem(entry, c, I, dev, variant, base) for _ in range(2 if twice else 1)]
    for P in Ps:
        call(P)
    for name, b in all_bufs(Ps[0]):
        _sent(f"{entry} {name}", b)
    if twice:
        for (name, a), (_, b) in zip(Ps[0].outb.items(), Ps[1].outb.items()):
            need(torch.equal(_bits(a.flat), _bits(b.flat)), "repeat", "{} {}: two runs from the same state differ", entry, name)
    return results(Ps[0])


def run_all(c, I, dev, call, variant="pad", twice=True, entries=ENTRIES):
    """K13, then the other calls on the base it returned: {entry: outputs}."""
    out = {"logz": execute("logz", c, I, dev, call, variant, twice)}
    base = (out["logz"]["max"][0].copy(), out["logz"]["logsum"][0].copy())
    for u, name in getattr(I, "special", {}).items():
        if name == "nanbase":
            base[u % 2][u] = NAN                                              # special-a spoils base_logsum, special-b base_max
    for e in entries[1:]:
        out[e] = execute(e, c, I, dev, call, variant, twice, base)
    return out


# ---------------------------------------------------------------------------------------- 5 the checker
def _ratio(layer, name, got, ref, bound, rows):
    """got within ref +- bound on the given rows (a NaN is outside); the worst |error| / bound."""
    got, ref, bound = np.asarray(got, f64)[rows], np.asarray(ref, f64)[rows], np.broadcast_to(np.asarray(bound, f64), np.shape(ref))[rows]
    if not got.size:
        return 0.0
    with np.errstate(invalid="ignore"):
        err = np.where(got == ref, 0.0, np.abs(got - ref))                    # the same infinity on both sides is no error
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise SoftmaxCheckError(layer, f"{name}: {int(bad.sum())} values outside the bound, first at {i} of the checked rows: got {got[i]!r}, fp64 {ref[i]!r}, bound {bound[i]:.3g}, "
                                       f"ratio {err[i] / bound[i] if bound[i] else INF:.3g}")
    return float(np.where(err > 0, err / np.where(bound > 0, bound, 1.0), 0.0).max())


def _nan_rows(layer, name, got, want):
    got = np.isnan(np.asarray(got))
    rows = got.all(axis=1) if got.ndim == 2 else got
    need(np.array_equal(rows, want) and (got.ndim == 1 or not got[~want].any()), layer, "{}: NaN for users {}, the contract says {}", name,
         np.flatnonzero(rows).tolist(), np.flatnonzero(want).tolist())


def kappa_tight(m):
    """m + 3 ln m + 7 (module docstring, `tight`)."""
    return m + 3.0 * np.log(m) + 7.0


def sm_check(c, I, out, R):
    """The outputs of a case against the contract; returns the figures of the case (worst |error| / bound per output)."""
    kind = c.kind
    layer = {"plateau": "exact", "gauss": "bound", "special": "special"}[kind]
    w = {}
    U, V, N = c.U, c.V, c.N
    lz = out["logz"]
    lmax, lcount, lsum = lz["max"][0], lz["count"][0], lz["logsum"][0]
    same_bits(layer, "out_count", lcount, R.count.astype(i32))
    if kind == "plateau":
        same_bits(layer, "out_max", lmax, R.smax.astype(f32))
    else:
        need(np.array_equal(np.isnan(lmax), np.isnan(R.smax)), layer, "out_max: NaN where the reference has none, or the reverse")
        N_e = N * EPS / (1 - N * EPS)
        sb = (1 + SOFTMAX_EXCESS) * (N_e + EPS) * R.mag + (N + 1) * 2.0 ** -149
        fin = np.isfinite(R.smax)
        # the maximum of scores each within its own bound of the fp64 score lies within the largest of these bounds of the fp64 maximum
        w["max"] = _ratio(layer, "out_max", lmax, R.smax, sb, fin)
        same_bits(layer, "out_max where it is infinite", lmax[~fin], R.smax[~fin].astype(f32))
    nanbase = np.array([I.special.get(u) == "nanbase" for u in range(U)])     # K13 itself answers that user as any other; its base is then spoiled
    _nan_rows(layer, "out_logsum", lsum, (R.nan & ~nanbase) | R.ninf)
    none = R.count == 0
    need(bool(np.isneginf(lsum[none]).all() and np.isneginf(lmax[none]).all()), layer, "nothing eligible: max and logsum must be -inf")
    none = none | R.ninf                                                      # base_max = -inf: zeros in K17 / K23 / K24, whatever the count
    live = ~R.nan & ~none
    one, many = live & (R.m == 1), live & (R.m > 1)
    if kind == "plateau":
        same_bits("exact", "out_logsum for one maximum", lsum[one], np.zeros(int(one.sum()), f32))
        want = np.log(np.maximum(R.m, 1).astype(f64)).astype(f32)
        okl = (lsum == want) | (lsum == np.nextafter(want, f32(INF))) | (lsum == np.nextafter(want, f32(-INF)))
        need(bool(okl[many].all()), "exact", "out_logsum: users {} are neither float32(log m) nor its neighbour", np.flatnonzero(many & ~okl).tolist())
    else:
        lb = (1 + SOFTMAX_EXCESS) * np.array([GZ.logz_bound(n, V) for n in R.count]) + 2.0 * (N + 1) * R.G * EPS
        w["logsum"] = _ratio(layer, "out_logsum", lsum, R.logsum, lb, live)
    lnm = np.log(np.maximum(R.m, 1).astype(f64))
    kx = (1 + SOFTMAX_EXCESS)
    # ---- K23
    en = out.get("entropy")
    if en is not None:
        got = {"H": en["H"][0], "var": en["var"][0] if "var" in en else None, "mass": en["mass"][0] if "mass" in en else None}
        for k, g in got.items():
            if g is None:
                continue
            _nan_rows(layer, f"entropy {k}", g, R.nan)
            need(not g[none].any(), layer, "entropy {}: nothing eligible must give 0", k)
        if kind == "plateau":
            tb = {"H": (3 * lnm + 11) * EPS * lnm, "var": (3 * lnm + 8) * EPS * lnm ** 2, "mass": (3 * lnm + 8) * EPS}
        else:
            bH, bV = GH.entropy_bounds(N, V, R.n, R.C, R.G, np.where(live, R.H, 0.0), np.where(live, R.var, 0.0))
            tb = {"H": kx * bH, "var": kx * bV, "mass": kx * GE.kappa_mass(V, R.n, R.C) * EPS}
        ref = {"H": R.H, "var": R.var, "mass": R.mass}
        for k, g in got.items():
            if g is None:
                continue
            if kind == "plateau":
                need(bool((g[one] == (1.0 if k == "mass" else 0.0)).all()), "exact", "entropy {}: one maximum must give {} exactly", k, 1.0 if k == "mass" else 0.0)
                w[f"tight_{k}"] = _ratio("tight", f"entropy {k}", g, ref[k], tb[k], many)
            else:
                single = live & (R.count == 1)
                need(bool((g[single] == (1.0 if k == "mass" else 0.0)).all()), layer, "entropy {}: exactly one eligible news must give {} exactly", k, 1.0 if k == "mass" else 0.0)
                w[f"entropy_{k}"] = _ratio(layer, f"entropy {k}", g, ref[k], tb[k], live)
    # ---- K17 and K24
    splits = {e: plan(e, c).splits for e in ("expect", "affine")}
    for e in ("expect", "affine"):
        o = out.get(e)
        if o is None:
            continue
        ref, A, tot = finish(R, e, "s" in c.opt)
        nanrow = R.nan | (live & np.isnan(ref).any(axis=1))                   # a NaN weight, alpha or beta: that user's row alone
        g = o["out"]
        _nan_rows(layer, f"{e} out", g, nanrow)
        rows = live & ~nanrow
        empty = none & ~np.isnan(ref).any(axis=1)
        if kind == "plateau":                                                 # nothing eligible leaves minus the named rows, rounded once
            need(bool((g[empty].astype(f64) == ref[empty].astype(f32).astype(f64)).all()), layer, "{} out: nothing eligible leaves minus the named rows, rounded once", e)
        else:
            _ratio(layer, f"{e} out of the users with nothing eligible", g, ref, 2.0 * EPS * tot + 2.0 ** -149, empty)
        if kind == "plateau":
            need(bool((g[one & rows].astype(f64) == ref[one & rows].astype(f32).astype(f64)).all()), "exact", "{} out: a user with one maximum must equal the fp64 result rounded once", e)
            kt = kappa_tight(np.maximum(R.m, 1).astype(f64)) + (2.0 if e == "affine" else 0.0)
            w[f"tight_{e}"] = _ratio("tight", f"{e} out", g, ref, kt[:, None] * EPS * tot, many & rows)
        else:
            kap = GE.kappa(N, V, splits[e], R.n, R.C, R.G) + (2.0 if e == "affine" else 0.0)
            big = float(np.abs(np.where(np.isfinite(I.news[1:]), I.news[1:], 0.0)).max(initial=0.0))      # row 0 (3e37) is no term of anything
            it = 1.0 / np.where(R.tau_ok, R.tau, 1.0) if "s" in c.opt else 1.0
            bound = kx * kap[:, None] * EPS * A + 2.0 * EPS * tot + (R.n * 2.0 ** -126 * big * it)[:, None]      # the last term: weights below the normal range
            w[e] = _ratio(layer, f"{e} out", g, ref, bound, rows)
        if "mass" in o:
            mg = o["mass"][0]
            _nan_rows(layer, f"{e} mass", mg, R.nan)
            need(not mg[none].any(), layer, "{} mass: nothing eligible must give 0", e)
            if kind == "plateau":
                need(bool((mg[one] == 1.0).all()), "exact", "{} mass: one maximum must give 1.0", e)
                w[f"tight_{e}_mass"] = _ratio("tight", f"{e} mass", mg, R.mass, (3 * lnm + 8) * EPS, many)
            else:
                w[f"{e}_mass"] = _ratio(layer, f"{e} mass", mg, R.mass, kx * GE.kappa_mass(V, R.n, R.C) * EPS, live)
    return w


def _compare(layer, what, a, b, rows=None):
    for e in a:
        for k in a[e]:
            x, y = a[e][k], b[e][k]
            if rows is not None:
                x, y = (x[rows[0]], y[rows[1]]) if k == "out" else (x[:, rows[0]], y[:, rows[1]])
            same_bits(layer, f"{e} {k} {what}", x, y)


def sm_agree(c, I, out, dev, call, topk=None):
    """The bit-for-bit statements of the header that tie the calls together (module docstring, `agree`); the case's own splits
    when it names them, else 1."""
    ce = c if c.splits else c._replace(splits=1)
    fixed = out if c.splits else run_all(ce, I, dev, call, twice=False)
    nseg = plan("logz", c).nseg
    for s in sorted({0, 1, min(2, nseg), nseg}):
        other = execute("logz", c._replace(splits=s), I, dev, call, twice=False)
        _compare("agree", f"at splits = {s}", {"logz": out["logz"]}, {"logz": other})
    base = (out["logz"]["max"][0], out["logz"]["logsum"][0])
    # K24 with alpha = 1, beta = 0 is K17 with weight NULL
    I1 = SimpleNamespace(**vars(I))
    I1.weight, I1.beta = None, None
    plain = execute("expect", ce, I1, dev, call, twice=False, base=base)
    I1.weight, I1.beta = np.ones(c.U, f32), np.zeros(c.U, f32)
    aff = execute("affine", ce._replace(opt=ce.opt + "wb"), I1, dev, call, twice=False, base=base)
    _compare("agree", "of K24 with alpha = 1, beta = 0 against K17 with weight NULL", {"x": aff}, {"x": plain})
    # row u when every other user of the call is replaced
    u = c.U // 2
    I2 = SimpleNamespace(**vars(I))
    rng = _rng(13, c.N, c.U, c.V)
    I2.user = (I.user[rng.permutation(c.U)] * f32(1.5)).astype(f32)
    I2.user[u] = I.user[u]
    other = run_all(ce, I2, dev, call, twice=False)
    _compare("agree", f"of user {u} when the other users are replaced", fixed, other, rows=(slice(u, u + 1), slice(u, u + 1)))
    if topk is not None:
        same_bits("agree", "out_max against the k = 1 score of nr_score_topk", out["logz"]["max"][0], topk(c, I))


def sm_special(c, I, out, dev, call):
    """The ordinary users' bits equal those of the same call without the special users (the case names its splits)."""
    keep = np.array([u for u in range(c.U) if u not in I.special])
    I2 = SimpleNamespace(**vars(I))
    for k in ("user", "window", "tau_u", "weight", "beta", "sub_ids", "sub_w"):
        setattr(I2, k, getattr(I, k)[keep])
    I2.segs = [I.segs[u] for u in keep] if I.segs is not None else None
    I2.special = {}
    if I.segs is not None:
        I2.xids = np.concatenate(I2.segs + [np.array([c.V + 1], i32)]).astype(i32)
        I2.offsets = np.concatenate([[0], np.cumsum([len(s) for s in I2.segs])]).astype(i32)
    other = run_all(c._replace(U=len(keep)), I2, dev, call, twice=False)
    _compare("special", "of the ordinary users without the special ones", out, other, rows=(keep, slice(None)))


def sm_layout(c, I, dev, call, out):
    for variant in ("dense", "shift"):
        other = run_all(c, I, dev, call, variant, twice=False)
        _compare("layout", f"with {variant} buffers", other, out)


def sm_sweep(c, dev, call, layout=True, topk=None, agree=True):
    """The driver both files share: every layer of one case."""
    I = sm_inputs(c)
    R = sm_reference(c, I)
    out = run_all(c, I, dev, call)
    w = sm_check(c, I, out, R)
    if layout:
        sm_layout(c, I, dev, call, out)
    if c.kind == "gauss" and agree:
        sm_agree(c, I, out, dev, call, topk)
    if c.kind == "special":
        sm_special(c, I, out, dev, call)
    return w


# ---------------------------------------------------------------------------------------- 6 the named-row calls (K14, K19)
# nr_row_logprob and nr_row_logprob_grad share the 16-user gather (logp_rows_kernel / logp_grad_kernel<POOL>) and the fp64 finish.
# `lattice` data: integer vectors in [-2, 2] and quarter-grid priors make every gathered score exact in fp32, whatever the order of
# the chain; the bases are host-made fp32 values (no plateaus), every fourth user has the empty base (-inf, -inf): its row takes
# everything eligible.  Everything after the gather is fp64 rounded to fp32 once, so of the header's bound the score chain goes and
# kappa shrinks to the one rounding, e |value*|, plus the share of the fp64 scans: at most 7 + 3 joins of (max, sum) pairs lie between
# an entry and its result, each one exp (a few ulp of fp64), one product and one sum, then one division by tau and one log -- under
# 64 units of 2^-53 on the sums, taken as ROW_F64 = 2^-44 (512 units) on the absolute sums of each formula:
#   K14  |logp - logp*| <= e |logp*| + 2^-44 (1 + |logp*|);  total: e |total*| + 2^-44 sum_j (1 + |logp_j*|)
#   K19  |c_i - c_i*|   <= e |c_i*| + 2^-44 (|g_i| + sum_{j <= i} |g_j| e_i / W_j),   |a - a*| <= e |a*| + 2^-44 sum_j |g_j| B / W_j
# (the absolute sums are the reference's own results for |g|), each + 2^-149.  `exact`: fill entries are 0, NaN sits where the
# reference has it, a row that takes everything eligible ends in logp == 0 at its last live place and has a == 0.
RowCase = collections.namedtuple("RowCase", "name N U V k seq pool taus g total pad")
ROW_KS = (1, 63, 64, 65, 127, 128)
ROW_F64 = 2.0 ** -44
ROW_ROUTES = ("p0", "p1", "seq0", "seq1", "grad_g_null", "grad_g_given", "total_null", "total_given", "tau_scalar", "tau_u", "one_block", "more_blocks")


def row_cases():
    cs = []
    for i, k in enumerate(ROW_KS):
        for seq in (0, 1):
            j = 2 * i + seq
            cs.append(RowCase(f"rows-k{k}-seq{seq}", SM_NS[(5 * i + 3 * seq) % 14], (1, 15, 16, 17, 33)[j % 5], (130, 257, 294)[j % 3], k, seq, j % 4, (j // 2) % 2,
                              (j // 3) % 2, j % 2, j % 3))
    cs.append(RowCase("rows-all-taken", 36, 5, 7, 6, 1, 0, 0, 1, 1, 1))        # six real news, rows of six: everything eligible is taken
    assert len({c.name for c in cs}) == len(cs)
    return cs


def row_route(c):
    """nr_row_logprob: logp_rows_kernel<POOL>, one workgroup per 16 users, `sequential` a run-time branch; nr_row_logprob_grad (on the
    sequential cases): logp_grad_kernel<POOL>, g NULL or given."""
    r = [f"p{int(bool(c.pool))}", f"seq{c.seq}", "total_given" if c.total else "total_null", "tau_u" if c.taus else "tau_scalar", "one_block" if c.U <= 16 else "more_blocks"]
    return tuple(r + (["grad_g_given" if c.g else "grad_g_null"] if c.seq else []))


def row_inputs(c):
    rng = _rng(17, c.N, c.U, c.V, c.k, c.seq, c.pool, c.pad)
    V, U, N, k = c.V, c.U, c.N, c.k
    I = SimpleNamespace(prior=None, stamp=None, window=None, tau=0.7, tau_u=None, g=None)
    I.news, I.user = rng.integers(-2, 3, (V, N)).astype(f32), rng.integers(-2, 3, (U, N)).astype(f32)
    I.news[0] = 3e37
    if c.pool in (1, 2):
        I.prior = (rng.integers(-32, 33, V) / 4.0).astype(f32)
        I.prior[3::7] = -INF
    if c.pool in (1, 3):
        lo = rng.integers(0, 4, U)
        I.stamp, I.window = rng.integers(0, 10, V).astype(i32), np.stack([lo, lo + rng.integers(3, 7, U)], axis=1).astype(i32)
    I.row_ids = np.stack([rng.permutation(np.arange(-1, max(V + 1, k)))[:k] if k <= V + 2 else rng.integers(-1, V + 1, k) for _ in range(U)]).astype(i32)
    if k >= 2:
        I.row_ids[::2, 1] = I.row_ids[::2, 0]                                  # a repeated id is two entries
    if V > 5 and c.name != "rows-all-taken":
        I.news[5] = NAN                                                        # a NaN score: a key of 0 like a -inf prior or a stamp outside the window
        I.row_ids[::3, c.k - 1] = 5 if c.k >= 3 else I.row_ids[::3, c.k - 1]
    if c.name == "rows-all-taken":
        I.row_ids = np.stack([rng.permutation(np.arange(1, V)) for _ in range(U)]).astype(i32)
    I.base_max = (4.0 * rng.standard_normal(U)).astype(f32)
    I.base_logsum = (3.0 * np.abs(rng.standard_normal(U))).astype(f32)
    empty = np.ones(U, bool) if c.name == "rows-all-taken" else (np.arange(U) % 4 == 3) & bool(c.seq)    # independent entries need a base
    I.base_max[empty], I.base_logsum[empty] = -INF, -INF
    if c.taus:
        I.tau_u = np.array([0.3, 1.7, 0.75], f32)[rng.integers(0, 3, U)]
        if U >= 15:
            I.tau_u[5], I.tau_u[9] = 0.0, NAN                                  # NaN for every real entry of K14; zeros in K19
    if c.g:
        I.g = rng.standard_normal((U, k)).astype(f32)
    return I


def row_reference(c, I):
    """metrics.row_logprob_reference and, for a sequential case, metrics.row_logprob_grad_reference with g and with |g|, in float64
    on the fp32 inputs."""
    from newsrecommendation_amd import metrics
    kw = dict(row_ids=I.row_ids, temperature=I.tau_u.astype(f64) if I.tau_u is not None else float(f32(I.tau)), base=(I.base_logsum.astype(f64), I.base_max.astype(f64)),
              prior=I.prior, stamp=I.stamp, window=I.window)
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    with np.errstate(all="ignore"):
        R = SimpleNamespace()
        R.logp, R.total = metrics.row_logprob_reference(n64, u64, sequential=bool(c.seq), **kw)
        if c.seq:
            g = I.g.astype(f64) if I.g is not None else np.ones((c.U, c.k))
            R.a, R.c = metrics.row_logprob_grad_reference(n64, u64, g=g, **kw)
            R.a_abs, c_abs = metrics.row_logprob_grad_reference(n64, u64, g=np.abs(g), **kw)
            s = u64 @ n64.T + (I.prior.astype(f64)[None, :] if I.prior is not None else 0.0)
            R.live = (I.row_ids >= 1) & (I.row_ids < c.V)
            at = np.where(R.live, I.row_ids, 0)
            R.live &= ~np.isnan(np.take_along_axis(s, at.astype(np.int64), axis=1))
            if I.prior is not None:
                R.live &= ~np.isneginf(I.prior[at])
            if I.stamp is not None:
                R.live &= (I.window[:, :1] <= I.stamp[at]) & (I.stamp[at] <= I.window[:, 1:2])
            R.c_abs = np.where(R.live, 2.0 * np.abs(g) - c_abs, 0.0)           # |g_i| + sum_{j <= i} |g_j| e_i / W_j
    return R


def row_problem(entry, c, I, dev, variant="pad"):
    sh = variant == "shift"
    N, k, U, V = c.N, c.k, c.U, c.V
    o = (N, N + 4, tk_npad(N) + 8)
    S = SimpleNamespace(news=N, user=N, ids=k, g=k, win=2) if variant == "dense" else SimpleNamespace(
        news=o[c.pad], user=o[(c.pad + 1) % 3], ids=k + (1 if c.pad != 1 else 0), g=k + (5 if c.pad != 2 else 0), win=5 if c.pad != 0 else 2)
    fo, io = (0 if sh else 4), (2 if sh else 1)
    P = SimpleNamespace(entry=entry, c=c, I=I, S=S, inb={}, outb={}, ws=None)
    P.inb["news"], P.inb["user"] = in_buf(I.news, S.news, dev, fo, NAN), in_buf(I.user, S.user, dev, fo, NAN)
    if I.prior is not None:
        P.inb["prior"] = in_buf(I.prior, V, dev, io)
    if I.stamp is not None:
        P.inb["stamp"] = in_buf(I.stamp, V, dev, io)
        P.inb["window"] = in_buf(I.window, S.win, dev, io, np.tile(np.array([100, -100, 100], i32), (U, 1)))
    if I.tau_u is not None:
        P.inb["tau_u"] = in_buf(I.tau_u, U, dev, io)
    P.inb["row_ids"] = in_buf(I.row_ids, S.ids, dev, io, 1)                    # slack: a valid id
    P.inb["base_max"], P.inb["base_logsum"] = in_buf(I.base_max, U, dev, io), in_buf(I.base_logsum, U, dev, io)
    if entry == "logprob":
        P.outb["logp"] = out_buf(U, k, k, torch.float32, dev, io)
        if c.total:
            P.outb["total"] = out_buf(1, U, U, torch.float32, dev, io)
    else:
        if I.g is not None:
            P.inb["g"] = in_buf(I.g, S.g, dev, io, 1e30)                       # slack: a huge g
        P.outb["weight"], P.outb["sub_w"] = out_buf(1, U, U, torch.float32, dev, io), out_buf(U, k, k, torch.float32, dev, io)
    if not sh:
        assert P.inb["news"].ptr % 32 == 16 and P.inb["user"].ptr % 32 == 16 and P.inb["row_ids"].ptr % 8 == 4
    return P


def row_execute(entry, c, I, dev, call, variant="pad", twice=True):
    Ps = [row_problem(entry, c, I, dev, variant) for _ in range(2 if twice else 1)]
    for P in Ps:
        call(P)
    for name, b in list(Ps[0].inb.items()) + list(Ps[0].outb.items()):
        _sent(f"{entry} {name}", b)
    if twice:
        for (name, a), (_, b) in zip(Ps[0].outb.items(), Ps[1].outb.items()):
            need(torch.equal(_bits(a.flat), _bits(b.flat)), "repeat", "{} {}: two runs from the same state differ", entry, name)
    return results(Ps[0])


def row_check(c, I, out, R):
    w = {}
    real = (I.row_ids >= 1) & (I.row_ids < c.V)
    lp = out["logprob"]["logp"]
    need(bool((lp[~real] == 0).all()), "exact", "out_logp: a fill entry must be 0")
    need(np.array_equal(np.isnan(lp), np.isnan(R.logp)), "exact", "out_logp: NaN at {} entries, the contract says {}", int(np.isnan(lp).sum()), int(np.isnan(R.logp).sum()))
    ok = ~np.isnan(R.logp)
    ref = np.where(ok, R.logp, 0.0)
    w["logp"] = _ratio("tight", "out_logp", np.where(ok, lp, 0.0), ref, EPS * np.abs(ref) + ROW_F64 * (1.0 + np.abs(ref)) + 2.0 ** -149, np.ones(c.U, bool))
    if c.seq:                                                                 # a row that takes everything eligible ends in 0
        for u in np.flatnonzero(np.isneginf(I.base_max)):
            live = np.flatnonzero(ok[u] & real[u])
            need(not len(live) or lp[u, live[-1]] == 0.0, "exact", "user {}: the last live place of a row over an empty base must be 0 exactly", u)
    if "total" in out["logprob"]:
        tot = out["logprob"]["total"][0]
        need(np.array_equal(np.isnan(tot), np.isnan(R.total)), "exact", "out_total: NaN where the reference has none, or the reverse")
        tb = EPS * np.abs(np.nan_to_num(R.total)) + ROW_F64 * (1.0 + np.abs(ref)).sum(axis=1) + 2.0 ** -149
        w["total"] = _ratio("tight", "out_total", tot, R.total, tb, ~np.isnan(R.total))
    if c.seq:
        a, cc = out["grad"]["weight"][0], out["grad"]["sub_w"]
        need(not np.isnan(a).any() and not np.isnan(cc).any(), "exact", "K19 never answers NaN")
        need(bool((cc[~R.live] == 0).all()), "exact", "out_sub_w: an entry that is no step must be 0")
        need(bool((a[np.isneginf(I.base_max)] == 0).all()), "exact", "out_weight: an empty base must give a == 0")
        w["a"] = _ratio("tight", "out_weight", a, R.a, EPS * np.abs(R.a) + ROW_F64 * R.a_abs + 2.0 ** -149, np.ones(c.U, bool))
        w["c"] = _ratio("tight", "out_sub_w", cc, R.c, EPS * np.abs(R.c) + ROW_F64 * R.c_abs + 2.0 ** -149, np.ones(c.U, bool))
    return w


def row_sweep(c, dev, call, layout=True):
    I = row_inputs(c)
    R = row_reference(c, I)
    entries = ("logprob", "grad") if c.seq else ("logprob",)
    out = {e: row_execute(e, c, I, dev, call) for e in entries}
    w = row_check(c, I, out, R)
    if I.tau_u is not None and c.U >= 15:                                     # the ordinary users' bits without the users of a bad temperature
        keep = np.array([u for u in range(c.U) if u not in (5, 9)])
        I2 = SimpleNamespace(**vars(I))
        for k in ("user", "window", "tau_u", "row_ids", "base_max", "base_logsum", "g"):
            if getattr(I, k) is not None:
                setattr(I2, k, getattr(I, k)[keep])
        for e in entries:
            other = row_execute(e, c._replace(U=len(keep)), I2, dev, call, twice=False)
            for k in out[e]:
                x = out[e][k][:, keep] if out[e][k].shape[0] == 1 else out[e][k][keep]
                same_bits("special", f"{e} {k} of the ordinary users without the special ones", x, other[k])
    if layout:
        for variant in ("dense", "shift"):
            other = {e: row_execute(e, c, I, dev, call, variant, twice=False) for e in entries}
            for e in entries:
                for k in out[e]:
                    same_bits("layout", f"{e} {k} with {variant} buffers", other[e][k], out[e][k])
    return w


# ---------------------------------------------------------------------------------------- 7 the news side (K18, K25)
# nr_score_expect_news (rows and mass-only) and nr_score_expect_news_affine: the news are tiled (TV = score_user_tile(N, a row of P):
# 64 / 32 / 16 with <4, 11>, <2, 26>, <1, 32>), the users streamed, cut by lz_plan_tile(V, U + 1, TV, splits).  The lists are the
# transposed CSR (per news the ascending user indices), the named terms a second CSR per news.  One case runs K13 (through the
# per-user lists, the inverse of the transposed ones) for the base, then K18 rows, K18 mass-only and K25.
#   plateau  user u is 128 r_g, g = u mod G; the m_g news planted for group g are copies of r_g (m_g from {1, 2, 3, 64, 129} as V
#            allows) and are kept out of lists, windows and -inf priors, so every live user of the group has exactly these m_g
#            maxima; weights, alpha, beta and named_w are powers of two (or 0), temperatures come from {1/4, 1/2, 1}.
#            `exact`, as numbers: a row of a group with m = 1 is the lattice sum of c_u user_u over the users whose best it is minus
#            its named terms (p = 1, x = -0: beta has no part), every row that is nobody's maximum an exact zero minus its named
#            terms, mass_v the exact sum of the weights (K25: the count).
#            `tight` for a row of a group with m > 1 (e = 2^-24): p = (1 + t) / m, |t| <= (6 + 3 ln m) e as on the user side (the
#            logsum's rounding or its neighbour in the exponent, expf's 3 ulp); fl(c p) is exact for a power of two c and the
#            products with user_uc = +-256 are exact; the contraction adds the n_v users of the row in fp32, (n_v - 1) e; slices
#            and named terms in fp64, one rounding, e, second order, e:  |out_vc - out*_vc| <= (n_v + 3 ln m + 7) e A_vc with the
#            header's A_vc.  K25 adds the fma of the weight and its product with p: n_v + 3 ln m + 9, the error 3 e ln m of x in
#            the weight carried by the `+ 1` beside |x*| in A_vc.  Masses (fp64 sums of the exact products weight p, one
#            rounding, second order): |mass_v - mass*_v| <= (3 ln m + 8) e sum_u |weight_u| p*_uv.
#   gauss    the bounds of include/nrhip.h as tests/test_gpu_expect_news.py and test_gpu_entropy_news.py state them (their
#            _reference and kappas, imported) -- `bound`.  With per-user temperatures the call also holds a user with tau = 0, one
#            with an infinite component (dead through its NaN base; 0 in the contraction and in the named terms) and, for K25,
#            one with a NaN alpha and one with a NaN beta: they contribute to no row and no NaN appears anywhere; named terms
#            name dead users, users outside [0, U), carry named_w == 0 and offsets beyond n_named -- `special`.
#   agree    K25 with beta NULL = K18 with weight = alpha; K18's mass-only mass = the rows mode's; row v when every other news row
#            is replaced (same base arrays) -- bit for bit.
NewsCase = collections.namedtuple("NewsCase", "name kind N V U splits pool csr taus named opt pad")
NEWS_ROUTES = tuple(f"tile_{t}" for t in (64, 32, 16)) + tuple(f"kmax_{k}" for k in (11, 26, 32)) + tuple(f"p{p}l{l}" for p in (0, 1) for l in (0, 1)) + (
    "splits_auto", "splits_given", "short_last_slice", "two_chunk_segments", "tau_scalar", "tau_u", "named_null", "named_given", "scale_0", "scale_1", "weight_null",
    "weight_given", "beta_null", "beta_given", "mass_null", "mass_given")


def news_plan(c):
    return lz_plan_tile(c.V, c.U + 1, contract_tile(c.N), c.splits)


def news_ws_bytes(c, rows):
    """en_carve / ea_carve: V * slices * (4 N + 8) rounded to 8, V * slices * 8 in the mass-only mode."""
    n = c.V * news_plan(c).splits
    return (n * 8 + (n * c.N * 4 if rows else 0) + 7) // 8 * 8


def news_cases():
    cs, i = [], 0
    for kind in ("plateau", "gauss"):
        for N in SM_NS:
            tile = contract_tile(N)
            U = SM_VS[(i + i // 6) % 6]
            cs.append(NewsCase(f"news-{kind}-N{N}", kind, N, 1 + _u_of(tile, i + i // 4), U, (0, 1, 2, 3)[(i + i // 4) % 4], i % 4, (i // 2) % 2, i % 2, (i // 3) % 2, OPTS[i % 6], i % 3))
            i += 1
        cs += [NewsCase(f"news-{kind}-two-chunks-auto", kind, 4, 4, V_TWO, 0, 1, 1, 1, 1, "wbsM", 1),
               NewsCase(f"news-{kind}-two-chunks-short", kind, 36, 3, V_TWO, 8, 0, 0, 0, 0, "wM", 2),
               NewsCase(f"news-{kind}-many-maxima", kind, 28, 262, 130, 2, 0, 0, 0, 0, "M", 0),                  # room for 129, 64, 3, 2 and 1 copies; no weights
               NewsCase(f"news-{kind}-lists", kind, 36, 9, 294, 2, 0, 1, 1, 1, "wbM", 1),
               NewsCase(f"news-{kind}-lists-pool", kind, 32, 18, 294, 3, 1, 1, 1, 1, "sM", 2)]
    assert len({c.name for c in cs}) == len(cs)
    return [c._replace(splits=min(c.splits, lz_plan_tile(c.V, c.U + 1, 64, 1).nseg)) for c in cs]


def news_route(c):
    """nr_score_expect_news: expect_news_stream_kernel<MT, KMAX, POOL, LISTS, ROWS> (both ROWS), expect_news_final_kernel;
    nr_score_expect_news_affine: expect_news_affine_stream_kernel<MT, KMAX, POOL, LISTS>, its final kernel."""
    p = news_plan(c)
    r = [f"tile_{p.TU}", f"p{int(bool(c.pool))}l{c.csr}", "splits_given" if c.splits else "splits_auto", "tau_u" if c.taus else "tau_scalar", "named_given" if c.named else "named_null",
         "scale_1" if "s" in c.opt else "scale_0", "weight_given" if "w" in c.opt else "weight_null", "beta_given" if "b" in c.opt else "beta_null",
         "mass_given" if "M" in c.opt else "mass_null"]
    if tk_npad(c.N) // 32 == KMAX[p.TU]:
        r.append(f"kmax_{KMAX[p.TU]}")
    if c.splits and p.nseg % p.segs_per:
        r.append("short_last_slice")
    if p.seg > 128:
        r.append("two_chunk_segments")
    return tuple(r)


def news_inputs(c):
    rng = _rng(23, c.N, c.V, c.U, c.splits, c.pool, c.csr, c.taus, c.named, c.pad, len(c.opt), c.kind == "gauss")
    V, U, N = c.V, c.U, c.N
    plateau = c.kind == "plateau"
    I = SimpleNamespace(prior=None, stamp=None, window=None, offsets=None, xids=None, segs=None, tau=(0.25, 0.5, 1.0)[(N + U) % 3] if plateau else (0.5, 0.7, 1.3)[(N + U) % 3],
                        tau_u=None, weight=None, beta=None, alpha25=None, n_off=None, n_user=None, n_w=None, v_off=None, v_users=None, special={}, planted=np.zeros(0, np.int64))
    if plateau:
        G = max(1, min(5, V - 1))
        pats = []
        while len(pats) < G:
            r = rng.choice(np.array([-2, 2]), N)
            if not any((r == q).all() for q in pats):
                pats.append(r)
        news = rng.integers(-2, 3, (V, N))
        for r in pats:
            news[(news == r).all(axis=1), 0] = 0
        ms = [min(SM_MS[(N // 4 + U + g) % 5], V - 1) for g in range(G)]       # the maxima of group g: copies of its row
        while sum(ms) > V - 1:
            ms[int(np.argmax(ms))] -= 1
        perm, at = 1 + rng.permutation(V - 1), 0
        for g, r in enumerate(pats):
            news[perm[at:at + ms[g]]] = r
            at += ms[g]
        I.planted = np.sort(perm[:at])
        I.news, I.user = news.astype(f32), np.stack([128.0 * pats[u % G] for u in range(U)]).astype(f32)
    else:
        I.news = rng.standard_normal((V, N)).astype(f32)
        scale = np.array([1e-3, 1.0, 300.0])[np.arange(U) % 3]
        I.user = (rng.standard_normal((U, N)) * (scale / math.sqrt(N))[:, None]).astype(f32)
    I.news[0] = 3e37
    if c.pool in (1, 2):
        I.prior = (128.0 * rng.integers(-2, 1, V)).astype(f32) if plateau else rng.standard_normal(V).astype(f32)
        I.prior[3::7] = -INF
        I.prior[I.planted] = 0.0
    if c.pool in (1, 3):
        lo = rng.integers(0, 4, U)
        I.stamp, I.window = rng.integers(0, 10, V).astype(i32), np.stack([lo, lo + rng.integers(3, 7, U)], axis=1).astype(i32)
        I.stamp[I.planted] = 3                                                # inside every window [lo <= 3, lo + 3 >= 3]
        if U >= 3:
            I.window[2] = (5, 4)                                              # lo > hi: a dead user
    if c.csr:                                                                 # the transposed lists: per news the users that list it
        lists = []
        for v in range(V):
            L = CSR_LENGTHS[(v + 1) % 6] if V < 6 else CSR_LENGTHS[v % 6]
            lists.append(np.zeros(0, i32) if v in I.planted else np.sort(rng.choice(np.arange(-L, U + L), L, replace=False)).astype(i32))
        if U >= 257:                                                          # 128 and 65 users listed in one chunk of users (the refill loop), all before slice 1
            vs = next((v for v in range(1, V) if v not in I.planted), 0)          # row 0 is never shown: its list is then only read past
            lists[vs] = np.concatenate([np.arange(128), 128 + np.sort(rng.choice(128, 65, replace=False))]).astype(i32)
        I.v_users = np.concatenate(lists + [np.array([U + 1], i32)]).astype(i32)
        I.v_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(i32)
        I.v_off[V] += 7                                                       # beyond n_excl: clamped
        segs = [[] for _ in range(U)]
        for v in range(1, V):
            for u in lists[v][(lists[v] >= 0) & (lists[v] < U)]:
                segs[u].append(v)
        I.segs = [np.array(x, i32) for x in segs]
        I.xids = np.concatenate(I.segs + [np.array([V + 1], i32)]).astype(i32)
        I.offsets = np.concatenate([[0], np.cumsum([len(x) for x in I.segs])]).astype(i32)
    if c.taus:
        I.tau_u = (np.array([0.25, 0.5, 1.0], f32) if plateau else np.array([0.3, 1.7, 0.75], f32))[rng.integers(0, 3, U)]
    if "w" in c.opt:
        I.weight = np.array([0.5, -2.0, 1.0, 4.0], f32)[rng.integers(0, 4, U)] if plateau else rng.standard_normal(U).astype(f32)
    if "b" in c.opt:
        I.beta = np.array([-0.5, 1.0, 0.0, 2.0], f32)[rng.integers(0, 4, U)] if plateau else rng.standard_normal(U).astype(f32)
    I.alpha25 = I.weight
    if c.kind == "gauss" and c.taus and U >= 8:                               # the special users
        I.special = {1: "tau0", 3: "inf_component", 4: "alphanan", 6: "betanan"}
        I.tau_u[1] = 0.0
        I.user[3, N - 1] = INF
        if I.weight is not None:
            I.alpha25 = I.weight.copy()
            I.alpha25[4] = NAN
        if I.beta is not None:
            I.beta[6] = NAN
    if c.named:
        cnt = rng.integers(0, 4, V)
        I.n_user = rng.integers(-1, U + 1, int(cnt.sum()) + 1).astype(i32)   # -1 and U: outside [0, U)
        I.n_w = (np.array([0.0, 0.5, -1.0, 2.0])[rng.integers(0, 4, len(I.n_user))] if plateau else rng.standard_normal(len(I.n_user)) * (rng.random(len(I.n_user)) > 0.2)).astype(f32)
        if I.special:
            I.n_user[:4] = (1, 3, 2, 1)[:len(I.n_user[:4])]                   # dead users named
        I.n_off = np.concatenate([[0], np.cumsum(cnt)]).astype(i32)
        I.n_off[V] += 5                                                       # beyond n_named: clamped
    return I


def news_reference(c, I, which):
    """(out*, A, mass*, M, n, C, G) of tests/test_gpu_expect_news.py (`which` = news) or test_gpu_entropy_news.py (affine)."""
    import test_gpu_entropy_news as GA
    import test_gpu_expect_news as EN
    hkw = {}
    if I.prior is not None:
        hkw["prior"] = I.prior
    if I.stamp is not None:
        hkw["stamp"], hkw["window"] = I.stamp, I.window
    if I.segs is not None:
        hkw["exclude"] = I.segs
    tau = torch.from_numpy(I.tau_u.astype(f64)) if I.tau_u is not None else float(f32(I.tau))
    named = None
    if I.n_off is not None:
        off = np.minimum(I.n_off, len(I.n_user))                              # the library's clamp; entries outside [0, U) are skipped by it, and dropped here
        keep = (I.n_user >= 0) & (I.n_user < c.U)
        named = (np.concatenate([[0], np.cumsum(keep)])[off].astype(i32), I.n_user[keep], I.n_w[keep])
    news, user = torch.from_numpy(I.news), torch.from_numpy(I.user)
    t = lambda x: None if x is None else torch.from_numpy(x)
    with np.errstate(all="ignore"):
        if which == "news":
            return EN._reference(news, user, tau, hkw, weight=t(I.weight), named=named, scale="s" in c.opt)
        return GA._reference(news, user, tau, hkw, alpha=t(I.alpha25), beta=t(I.beta), named=named, scale="s" in c.opt)


def news_problem(entry, c, I, dev, variant="pad", base=None):
    """entry: news (K18 rows), newsmass (K18 mass-only), newsaffine (K25)."""
    sh = variant == "shift"
    N, V, U = c.N, c.V, c.U
    o = (N, N + 4, tk_npad(N) + 8)
    S = SimpleNamespace(news=N, user=N, out=N, win=2) if variant == "dense" else SimpleNamespace(news=o[c.pad], user=o[(c.pad + 1) % 3], out=N + (4 if c.pad != 1 else 0),
                                                                                              win=5 if c.pad != 0 else 2)
    fo, io, wo = (0 if sh else 4), (2 if sh else 1), (4 if sh else 2)
    P = SimpleNamespace(entry=entry, c=c, I=I, S=S, inb={}, outb={}, ws=None)
    P.inb["news"], P.inb["user"] = in_buf(I.news, S.news, dev, fo, NAN), in_buf(I.user, S.user, dev, fo, NAN)
    if I.prior is not None:
        P.inb["prior"] = in_buf(I.prior, V, dev, io)
    if I.stamp is not None:
        P.inb["stamp"] = in_buf(I.stamp, V, dev, io)
        P.inb["window"] = in_buf(I.window, S.win, dev, io, np.tile(np.array([100, -100, 100], i32), (U, 1)))
    if I.v_off is not None:
        P.inb["offsets"], P.inb["xids"] = in_buf(I.v_off, V + 1, dev, io), in_buf(I.v_users, len(I.v_users), dev, io)
    if I.tau_u is not None:
        P.inb["tau_u"] = in_buf(I.tau_u, U, dev, io)
    P.inb["base_max"], P.inb["base_logsum"] = in_buf(base[0], U, dev, io), in_buf(base[1], U, dev, io)
    al = I.alpha25 if entry == "newsaffine" else I.weight
    if al is not None:
        P.inb["alpha"] = in_buf(al, U, dev, io)
    if entry == "newsaffine" and I.beta is not None:
        P.inb["beta"] = in_buf(I.beta, U, dev, io)
    if I.n_off is not None:
        P.inb["n_off"], P.inb["n_user"], P.inb["n_w"] = in_buf(I.n_off, V + 1, dev, io), in_buf(I.n_user, len(I.n_user), dev, io), in_buf(I.n_w, len(I.n_w), dev, io)
    if entry != "newsmass":
        P.outb["out"] = out_buf(V, N, S.out, torch.float32, dev, fo)
    if entry == "newsmass" or "M" in c.opt:
        P.outb["mass"] = out_buf(1, V, V, torch.float32, dev, io)
    P.ws_bytes = news_ws_bytes(c, entry != "newsmass")
    P.ws = glue_buf(1, P.ws_bytes // 4, P.ws_bytes // 4, torch.int32, dev, wo, IFILL)
    if not sh:
        assert P.inb["news"].ptr % 32 == 16 and P.inb["user"].ptr % 32 == 16 and P.ws.ptr % 16 == 8 and ("out" not in P.outb or P.outb["out"].ptr % 32 == 16)
    return P


def news_execute(entry, c, I, dev, call, base, variant="pad", twice=True):
    Ps = [news_problem(entry, c, I, dev, variant, base) for _ in range(2 if twice else 1)]
    for P in Ps:
        call(P)
    for name, b in all_bufs(Ps[0]):
        _sent(f"{entry} {name}", b)
    if twice:
        for (name, a), (_, b) in zip(Ps[0].outb.items(), Ps[1].outb.items()):
            need(torch.equal(_bits(a.flat), _bits(b.flat)), "repeat", "{} {}: two runs from the same state differ", entry, name)
    return results(Ps[0])


def news_base(c, I, dev, logz_call):
    """The base of K13 for these users: the stream call of part 4 on the per-user lists."""
    sc = SmCase(c.name, c.kind, c.N, c.U, c.V, 0, c.pool, c.csr, c.taus, 0, 0, "", c.pad)
    lz = execute("logz", sc, I, dev, logz_call, twice=False)
    return lz["max"][0].copy(), lz["logsum"][0].copy()


def news_run(c, I, dev, call, base, variant="pad", twice=True):
    return {e: news_execute(e, c, I, dev, call, base, variant, twice) for e in ("news", "newsmass", "newsaffine")}


def news_check(c, I, out):
    import test_gpu_entropy_news as GA
    import test_gpu_expect_news as EN
    from newsrecommendation_amd import metrics
    w = {}
    layer = "exact" if c.kind == "plateau" else "special" if I.special else "bound"
    splits = news_plan(c).splits
    if c.kind == "plateau":                                                   # per row: the users it gets weight from and their number of maxima
        hkw = {k: v for k, v in (("prior", I.prior), ("stamp", I.stamp), ("window", I.window), ("exclude", I.segs)) if v is not None}
        with np.errstate(all="ignore"):
            p, _ = metrics.softmax_matrix_reference(I.news.astype(f64), I.user.astype(f64), temperature=I.tau_u.astype(f64) if I.tau_u is not None else float(f32(I.tau)), **hkw)
        on = p > 1e-30
        m_u = np.where(on.any(axis=1), np.rint(1.0 / np.maximum(p.max(axis=1), 1e-300)), 1.0)
        n_v = on.sum(axis=0).astype(f64)
        m_v = np.where(on, m_u[:, None], 1.0).max(axis=0)
        one, many, lnm = m_v == 1, m_v > 1, np.log(m_v)
    for e, which in (("news", "news"), ("newsmass", "news"), ("newsaffine", "affine")):
        ref, A, mass, M, n, C, G = news_reference(c, I, which)
        for k, g in out[e].items():
            need(bool(np.isfinite(g).all()), layer, "{} {}: a value that is not finite", e, k)
        kr, km = (EN.kappas if which == "news" else GA.kappas)(c.N, c.V, c.U, splits, n, C, G)
        if "out" in out[e]:
            g = out[e]["out"]
            if c.kind == "plateau":
                need(bool((g[one].astype(f64) == ref[one].astype(f32).astype(f64)).all()), "exact", "{} out: rows differ from the exact lattice sums", e)
                rest = n_v == 0
                if I.n_off is None:
                    need(not g[rest].any(), "exact", "{} out: a row nobody's maximum is must be an exact zero", e)
                kt = n_v + 3.0 * lnm + (9.0 if which == "affine" else 7.0)
                w[f"tight_{e}"] = _ratio("tight", f"{e} out", g, ref, kt[:, None] * EPS * A + 2.0 ** -149, many)
            else:
                w[e] = _ratio(layer, f"{e} out", g, ref, (1 + SOFTMAX_EXCESS) * kr * EPS * A + 2.0 ** -149, np.ones(c.V, bool))
        if "mass" in out[e]:
            g = out[e]["mass"][0]
            if c.kind == "plateau":
                need(bool((g[one].astype(f64) == mass[one]).all()), "exact", "{} mass: differs from the exact sum of the weights", e)
                w[f"tight_{e}_mass"] = _ratio("tight", f"{e} mass", g, mass, (3.0 * lnm + 8.0) * EPS * M + 2.0 ** -149, many)
            else:
                w[f"{e}_mass"] = _ratio(layer, f"{e} mass", g, mass, (1 + SOFTMAX_EXCESS) * km * EPS * M + 2.0 ** -149, np.ones(c.V, bool))
    return w


def news_agree(c, I, out, dev, call, base):
    ce = c if c.splits else c._replace(splits=1)
    Iw = SimpleNamespace(**vars(I))
    Iw.beta, Iw.alpha25 = None, I.weight                                      # K25 with beta NULL against K18 with weight = alpha
    a18 = news_execute("news", ce, Iw, dev, call, base, twice=False)
    a25 = news_execute("newsaffine", ce, Iw, dev, call, base, twice=False)
    same_bits("agree", "rows of K25 with beta NULL against K18 with weight = alpha", a25["out"], a18["out"])
    if "mass" in out["news"]:
        same_bits("agree", "mass of the mass-only mode against the rows mode", out["newsmass"]["mass"], out["news"]["mass"])
    v = max(1, c.V // 2)                                                      # row v when every other news row is replaced, on the same base
    fixed = {e: news_execute(e, ce, I, dev, call, base, twice=False) for e in ("news", "newsaffine")}
    I2 = SimpleNamespace(**vars(I))
    rng = _rng(29, c.N, c.V, c.U)
    I2.news = (I.news[np.concatenate([[0], 1 + rng.permutation(c.V - 1)])] * f32(0.5)).astype(f32)
    I2.news[0], I2.news[v] = I.news[0], I.news[v]
    for e in fixed:
        other = news_execute(e, ce, I2, dev, call, base, twice=False)
        for k in fixed[e]:
            x, y = (fixed[e][k][v], other[k][v]) if k == "out" else (fixed[e][k][:, v], other[k][:, v])
            same_bits("agree", f"{e} {k} of news {v} when the other rows are replaced", x, y)


def news_sweep(c, dev, call, logz_call, layout=True, agree=True):
    I = news_inputs(c)
    base = news_base(c, I, dev, logz_call)
    out = news_run(c, I, dev, call, base)
    w = news_check(c, I, out)
    if layout:
        for variant in ("dense", "shift"):
            other = news_run(c, I, dev, call, base, variant, twice=False)
            _compare("layout", f"with {variant} buffers", other, out)
    if c.kind == "gauss" and agree:
        news_agree(c, I, out, dev, call, base)
    return w


H = sys.modules[__name__]          # the tests below (and the host file) address the part above as H


# ------------------------------------------------------------------------------------------ the GPU tests
def _p(P, name):
    b = P.inb.get(name) or P.outb.get(name)
    return b.ptr if b is not None else None


def descriptor(P, ptr=_p):
    """(descriptor, size query, call) of P's entry point; `ptr` turns a buffer name into an address."""
    c, I, S, L = P.c, P.I, P.S, _lib.lib()
    shared = dict(news_vecs=ptr(P, "news"), ld_news=S.news, V=c.V, user=ptr(P, "user"), ld_user=S.user, U=c.U, N=c.N, splits=c.splits, excl_offsets=ptr(P, "offsets"),
                  excl_ids=ptr(P, "xids"), n_excl=len(I.xids) if I.xids is not None else 0, tau=float(I.tau), tau_u=ptr(P, "tau_u"), ws=P.ws.ptr if P.ws is not None else 16,
                  ws_bytes=P.ws_bytes, prior=ptr(P, "prior"), stamp=ptr(P, "stamp"), window=ptr(P, "window"), ld_window=S.win if I.stamp is not None else 0)
    if P.entry == "logz":
        return _lib.LogzDesc(out_logsum=ptr(P, "logsum"), out_max=ptr(P, "max"), out_count=ptr(P, "count"), **shared), L.nr_score_logz_workspace_bytes, L.nr_score_logz
    shared.update(base_max=ptr(P, "base_max"), base_logsum=ptr(P, "base_logsum"), out_mass=ptr(P, "mass"))
    if P.entry == "entropy":
        return _lib.EntropyDesc(out_entropy=ptr(P, "H"), out_var=ptr(P, "var"), **shared), L.nr_score_entropy_workspace_bytes, L.nr_score_entropy
    shared.update(sub_ids=ptr(P, "sub_ids"), sub_w=ptr(P, "sub_w"), ld_sub=S.sub if c.T else 0, T=c.T, scale_inv_tau=int("s" in c.opt), out=ptr(P, "out"), ld_out=S.out)
    if P.entry == "expect":
        return _lib.ExpectDesc(weight=ptr(P, "alpha"), **shared), L.nr_score_expect_workspace_bytes, L.nr_score_expect
    return _lib.ExpectAffineDesc(alpha=ptr(P, "alpha"), beta=ptr(P, "beta"), **shared), L.nr_score_expect_affine_workspace_bytes, L.nr_score_expect_affine


def _call(P):
    """One call of the C ABI on the buffers of P; the size query must answer the restated carve (`wsize`)."""
    d, query, fn = descriptor(P)
    got = query(C.byref(d))
    need(got == P.ws_bytes, "wsize", "{}: the size query answers {}, the restated carve {} ({})", P.entry, got, P.ws_bytes, _lib.last_error())
    _lib.check(fn(C.byref(d), ops._stream()), "nr_score_" + P.entry)
    torch.cuda.synchronize()


def _topk1(c, I):
    """The k = 1 scores of nr_score_topk under the same pools and CSR lists, through the corpus sweep's buffers and call."""
    tc = CS.TkCase(c.name, "gauss", c.N, c.U, c.V, 1, 0, 0, int(bool(c.csr)), c.pool, 0, 0, True, 0, "", c.pad)
    It = SimpleNamespace(news=I.news, user=I.user, prior=I.prior, stamp=I.stamp, window=I.window, exclude=None, offsets=I.offsets, xids=I.xids, segs=I.segs, group=None,
                         best=np.zeros(c.U, i32))
    return CS.execute("topk", tc, It, DEV, CS._call, twice=False)["scores"][:, 0]


def _label(entry, c):
    p = plan(entry, c)
    name = {"logz": "logz_stream", "entropy": "entropy_stream", "expect": "expect_stream", "affine": "affine_stream"}[entry]
    return f"{name}[U={c.U},V={c.V},N={c.N},TU={p.TU},splits={p.splits},seg={p.seg}]"


@pytest.mark.parametrize("c", H.sm_cases(), ids=lambda c: c.name)
def test_softmax_calls(c):
    w, labels = CS._labelled(lambda: H.sm_sweep(c, DEV, _call, topk=_topk1))
    for e in ENTRIES:
        assert _label(e, c) in labels, (e, _label(e, c), sorted(labels))
    print(f"\nSOFTMAX {c.name} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(w.items())))


@pytest.mark.parametrize("N", sorted(H.REFUSED_NS), ids=str)
def test_a_width_that_is_no_multiple_of_four_is_refused_before_any_launch(N):
    c = next(x for x in H.sm_cases() if x.name == f"gauss-N{H.REFUSED_NS[N]}")
    I = H.sm_inputs(c)
    base = (np.zeros(c.U, f32), np.zeros(c.U, f32))
    for e in ENTRIES:
        P = H.problem(e, c, I, DEV, "pad", base)
        P.c = c._replace(N=N)
        d, query, fn = descriptor(P)
        (size, rc), labels = CS._labelled(lambda: (query(C.byref(d)), fn(C.byref(d), ops._stream())))
        assert size == 0 and rc != 0 and "multiple of 4" in _lib.last_error(), (e, size, rc, _lib.last_error())
        assert not labels, labels
        for name, b in H.all_bufs(P):
            assert torch.equal(_bits(b.flat), _bits(b.init)), (e, name)


def _row_call(P):
    c, I, S, L = P.c, P.I, P.S, _lib.lib()
    shared = dict(news_vecs=_p(P, "news"), ld_news=S.news, V=c.V, user=_p(P, "user"), ld_user=S.user, U=c.U, N=c.N, k=c.k, row_ids=_p(P, "row_ids"), ld_ids=S.ids,
                  tau=float(I.tau), tau_u=_p(P, "tau_u"), base_max=_p(P, "base_max"), base_logsum=_p(P, "base_logsum"), prior=_p(P, "prior"), stamp=_p(P, "stamp"),
                  window=_p(P, "window"), ld_window=S.win if I.stamp is not None else 0)
    if P.entry == "logprob":
        d = _lib.LogprobDesc(sequential=c.seq, out_logp=_p(P, "logp"), out_total=_p(P, "total"), **shared)
        rc = L.nr_row_logprob(C.byref(d), ops._stream())
    else:
        d = _lib.LogprobGradDesc(g=_p(P, "g"), ld_g=S.g if I.g is not None else 0, out_weight=_p(P, "weight"), out_sub_w=_p(P, "sub_w"), **shared)
        rc = L.nr_row_logprob_grad(C.byref(d), ops._stream())
    _lib.check(rc, "nr_row_" + P.entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", H.row_cases(), ids=lambda c: c.name)
def test_named_row_calls(c):
    w, labels = CS._labelled(lambda: H.row_sweep(c, DEV, _row_call))
    assert f"logp_rows[U={c.U},N={c.N},k={c.k},seq={c.seq}]" in labels, sorted(labels)
    print(f"\nSOFTMAX {c.name} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(w.items())))


def news_descriptor(P, ptr=_p):
    c, I, S, L = P.c, P.I, P.S, _lib.lib()
    shared = dict(news_vecs=ptr(P, "news"), ld_news=S.news, V=c.V, user=ptr(P, "user"), ld_user=S.user, U=c.U, N=c.N, splits=c.splits, excl_offsets=ptr(P, "offsets"),
                  excl_users=ptr(P, "xids"), n_excl=len(I.v_users) if I.v_users is not None else 0, tau=float(I.tau), tau_u=ptr(P, "tau_u"), base_max=ptr(P, "base_max"),
                  base_logsum=ptr(P, "base_logsum"), scale_inv_tau=int("s" in c.opt), named_offsets=ptr(P, "n_off"), named_user=ptr(P, "n_user"), named_w=ptr(P, "n_w"),
                  n_named=len(I.n_user) if I.n_user is not None else 0, out=ptr(P, "out"), ld_out=S.out, out_mass=ptr(P, "mass"), ws=P.ws.ptr if P.ws is not None else 16,
                  ws_bytes=P.ws_bytes, prior=ptr(P, "prior"), stamp=ptr(P, "stamp"), window=ptr(P, "window"), ld_window=S.win if I.stamp is not None else 0)
    if P.entry == "newsaffine":
        return _lib.ExpectNewsAffineDesc(alpha=ptr(P, "alpha"), beta=ptr(P, "beta"), **shared), L.nr_score_expect_news_affine_workspace_bytes, L.nr_score_expect_news_affine
    return _lib.ExpectNewsDesc(weight=ptr(P, "alpha"), **shared), L.nr_score_expect_news_workspace_bytes, L.nr_score_expect_news


def _news_call(P):
    d, query, fn = news_descriptor(P)
    got = query(C.byref(d))
    need(got == P.ws_bytes, "wsize", "{}: the size query answers {}, the restated carve {} ({})", P.entry, got, P.ws_bytes, _lib.last_error())
    _lib.check(fn(C.byref(d), ops._stream()), "nr_score_expect_" + P.entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", H.news_cases(), ids=lambda c: c.name)
def test_news_side_calls(c):
    w, labels = CS._labelled(lambda: H.news_sweep(c, DEV, _news_call, _call))
    p = H.news_plan(c)
    for name, rows in (("expect_news_stream", 1), ("expect_news_stream", 0), ("expect_news_affine_stream", 1)):
        want = f"{name}[V={c.V},U={c.U},N={c.N},TV={p.TU},splits={p.splits},seg={p.seg},pool={int(bool(c.pool))},lists={c.csr},rows={rows}]"
        assert want in labels, (want, sorted(labels))
    print(f"\nSOFTMAX {c.name} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(w.items())))

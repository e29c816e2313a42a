"""GPU: every route of the full-corpus selection calls through the C ABI: nr_score_topk, nr_score_sample with nr_sample_noise,
nr_score_rank and nr_mmr_select (include/nrhip.h K9 - K12; csrc/nr_topk.hip, nr_rank.hip, nr_mmr.hip over csrc/nr_score_tile.h).
The case tables, one route function per entry point (its dispatch restated), the input builders, the references, the drivers and
the checker are the first part of this file ("corpus sweep"; plain numpy and torch, no GPU needed);
tests/test_corpus_sweep_host.py imports them and proves on the CPU that the checker passes a sound fp32 stand-in (summing in slab
order, and with float64 accumulation rounded once) and fails each of eighteen subtly wrong ones.  The second part calls the C ABI
directly with the ctypes descriptors of _lib.py.

Buffers.  Every device array is one allocation [guard][payload][guard] (glue_buf of the glue sweep).  News and user bases are
16-byte aligned and no more, int32 arrays 4-byte aligned, the workspace 8-byte aligned and exactly as long as the size query
answered (which must equal the restated carve of rk_carve / rk_group_carve).  Outputs start as NaN (integers: -77).  After the
call every guard and slack column of every buffer, inputs included, is compared bit for bit (layer `sentinel`), and every call is
made twice on two problems built alike and compared bit for bit (`repeat`).  Every case runs with padded strides: ld_news and
ld_user two different ones of {N, N + 4, tk_npad(N) + 8}, ld_exclude in {E, E + 3}, ld_targets in {T, T + 1}, ld_window in {2, 5},
ld_pool_ids != ld_pool_scores.  The slack is poison that changes the answer when read: NaN in vector slack, the user's best id in
exclusion slack, a valid id that is no target in target slack, an empty window in window slack, a valid id with score +inf in
pool slack; news row 0 holds 3e37.  `layout`: the same case with the widths as strides, and with every base moved by 16 bytes
(8 for the workspace, 4 for the int32 arrays and the outputs), gives the same bits.

Data kinds.
  lattice  integer vectors in [-2, 2], priors on the 1/4 grid, many ties (MMR: entries in {-1, 0, 1} with 1 / 4 / 16 / 64
           non-zeros, penalties powers of two): every quantity is exact in fp32, so ids, scores, ranks, places and sums[0] equal
           the reference exactly (`exact`).  A sampled lattice case is stated through the probe: the scores are
           fl32(dot + fl32(prior + fl32(tau g))) formed in fp32 from the g nr_sample_noise returns.
  gauss    Gaussian vectors whose rows carry scales from 1e-3 to 1e3 inside one call (`bound`, `agree`), see below.
  special  hand-made rows (`special`): +0 and -0 scores in one row, real -inf scores, a +inf prior, chains that overflow to
           +-inf, a NaN news, a prior of -inf, -inf + inf = NaN, lo > hi, subnormal products.  What include/nrhip.h says: a -0 score
           ties with +0 (id ascending) and comes back as +0; subnormal products and partial sums are kept, not flushed; a real
           -inf score is returned with its id, ranked and counted, unlike the fill.

The bound (u = 2^-24, F = 2^-149).  One (u, v) score is ONE fmaf chain over N products, so against the fp64 dot product
  |dot_fp32 - dot| <= gamma_N A(u, v) + N F,   gamma_N = N u / (1 - N u),   A(u, v) = sum_i |a_i b_i| in fp64 per pair
(Higham, Accuracy and Stability of Numerical Algorithms, 3.1: any order of N - 1 additions and N products, fused or not; F per
product or sum that can underflow).  The prior is one more fp32 add: + u |score| + F.  A sampled prior P = fl32(prior + fl32(tau g))
against prior + tau g in fp64 (g the fp32 value of the probe): + u |tau g| + u |P| + 2 F.  CORPUS_CHAIN_EXCESS scales gamma_N if
the device ever exceeds it.  No flat tolerance works here: bounds inside one call span twelve orders of magnitude.
The band rule per pair.  With lo = r - b and hi = r + b over the eligible news of a user, sure(v) = #{w : lo_w > hi_v} news beat v
for certain and maybe(v) = #{w != v : hi_w >= lo_v} may beat it.  A top-k row: as many entries as there are eligible news (at
most k), fill behind; distinct eligible ids; every score within b of r; sorted by (score descending, id ascending); the entry at
place p has sure <= p <= maybe; every news with maybe < k is in the row.  A rank lies in [1 + sure(t), 1 + maybe(t)].  A place
is DECIDED when sure == maybe; a row is decided when all its places are (then the rule leaves one answer, the reference's).
With group caps the walk depends on the whole order: a user whose eligible news are all decided must equal the capped
reference exactly, for the others the scores are bounded and the caps must hold.  In every gauss case at least 90 % of the rows
are decided and every user tile holds a decided row: the host file asserts it from the fp64 reference alone.
MMR: s(i | j) = g(i, j) rn_i rn_j with g within gamma_N A(i, j) + N F, the norms' g(i, i) relative gamma_N, sqrt and division
correctly rounded (rn relative gamma_N / 2 + 2 u), two products (2 u):
  e_s(i, j) = [gamma_N A(i, j) / (|x_i| |x_j|) + |s| (gamma_N + 6 u)] (1 + 2^-10),   tol_u = 2 [p_u max e_s + u (max |r| + p_u)]
twice the error of a value fmaf(-p, maxsim, r).  As in test_gpu_mmr.py: every device row, replayed in fp64, took at every step a
candidate within tol of the best (`bound`), and a row whose reference margins (metrics.mmr_reference's) all reach tol equals it.

`agree` (gauss, padded strides), bit for bit: with targets drawn from the top-k rows and from outside them, "rank <= k exactly
when the target is at place rank - 1 of the row, with identical score bits"; nr_score_sample at tau = 0 equals nr_score_topk; row u
of a sampled call equals the plain call of user u alone with prior = P(u, .).
`sums`: out_sums against the header's formulas on the device's own ranks (checked above): math.log2, math.fsum, within
((U + 2) 2^-53 + CORPUS_LOG2_EXCESS) sum |terms|; sums[0] exact; a capped-out target (rank -1) counts in n_u and keeps the ideal DCG.
`noise`: nr_sample_noise bits against a numpy Philox4x32-10 restated here; g within 7 2^-23 max(1, |g|) of the fp64 value.

Layers of CorpusCheckError: sentinel, repeat, exact, layout, agree, special, bound, sums, noise.
Routes, derivations, measured figures and what stays uncovered: DESIGN.md "Full-corpus selection calls: routes as verified and
the sweep".
"""
import collections
import ctypes as C
import itertools
import math
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_glue_sweep as GL
from test_gpu_glue_sweep import _bits, _count_routes, _sentinels, _within, glue_buf
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------ corpus sweep
U32 = 2.0 ** -24
F149 = 2.0 ** -149
# What the device chain adds beyond gamma_N sum |a_i b_i|, as a fraction of it: four times the worst excess measured over the
# sweep on the MI355X against fp64, 0 when there is none (DESIGN.md holds the measured ratios).
CORPUS_CHAIN_EXCESS = 0.0
# The same for the fp64 log2 and the wave-wide sums of the rank metrics, relative to sum |terms|.
CORPUS_LOG2_EXCESS = 0.0
LAYERS = ("sentinel", "repeat", "exact", "layout", "agree", "special", "bound", "sums", "noise")
NAN, INF = float("nan"), float("inf")
IFILL = -77
f32, f64, i32 = np.float32, np.float64, np.int32


class CorpusCheckError(AssertionError):
    """A failed check of the sweep; `.layer` is one of LAYERS."""

    def __init__(self, layer, msg):
        assert layer in LAYERS, layer
        super().__init__(f"[{layer}] {msg}")
        self.layer = layer


def _as(layer, fn, *a):
    """Runs a helper of the glue sweep and files its failure under `layer`."""
    try:
        return fn(*a)
    except GL.GlueCheckError as e:
        raise CorpusCheckError(layer, str(e)) from None


def need(ok, layer, msg, *a):
    if not ok:
        raise CorpusCheckError(layer, msg.format(*a) if a else msg)


def bits32(a):
    return np.ascontiguousarray(a).view(np.int32 if np.asarray(a).dtype.itemsize == 4 else np.int64)


def same_bits(layer, name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    need(got.shape == ref.shape and got.dtype == ref.dtype, layer, "{}: {} {} against {} {}", name, got.shape, got.dtype, ref.shape, ref.dtype)
    bad = bits32(got) != bits32(ref)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise CorpusCheckError(layer, f"{name}: {int(bad.sum())} elements differ bit for bit, first at {i}: got {got[i]!r}, want {ref[i]!r}")


def _rng(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


# ---------------------------------------------------------------------------------------- 0 the plans, restated
def tk_npad(N):
    return (N + 31) // 32 * 32


def tile_bytes(TU, N):
    """tk_tile_bytes: the user vectors [TU, npad + 4] and two slabs [128, 36] of floats."""
    return (TU * (tk_npad(N) + 4) + 2 * 128 * 36) * 4


def user_tile(N, per_user):
    """score_user_tile: the widest of 64, 32, 16 users whose tile and `per_user` bytes beside it fit 160 KiB of LDS."""
    for tu in (64, 32):
        if tile_bytes(tu, N) + tu * per_user <= 160 * 1024:
            return tu
    return 16


def auto_splits(U, V, tile, most):
    tiles = (U + tile - 1) // tile
    return max(1, min((256 + tiles - 1) // tiles, (V - 1 + 127) // 128, most))


def tk_plan(c):
    """(TU, splits) of a top-k or sampled call: a user keeps k 8-byte candidates and a threshold in LDS."""
    TU = user_tile(c.N, 8 * c.k + 4)
    return TU, c.splits or auto_splits(c.U, c.V, TU, min(256, 8192 // c.k))


def tk_ws_bytes(c):
    return c.U * tk_plan(c)[1] * c.k * 8


def rk_blocks(G):
    b = (G + 63) // 64
    return 0 if G == 0 else 1 if b <= 1 else 2 if b <= 2 else 4 if b <= 4 else 8


def rk_plan(c):
    """(TU, splits, per, cps) of a rank call: with caps the per-wave group counters bound the tile (rk_group_user_tile)."""
    TU, gb = user_tile(c.N, 0), rk_blocks(c.G if c.cap else 0)
    if gb:
        TU = min(TU, 64 if gb <= 2 else 32 if gb == 4 else 16)
    splits = c.splits or auto_splits(c.U, c.V, TU, 256)
    per = (c.V - 1 + splits - 1) // splits
    return TU, splits, per, (per + 127) // 128


def rk_ws_bytes(c):
    """rk_carve, then rk_group_carve from the next multiple of 8."""
    _, splits, _, cps = rk_plan(c)
    ut = c.U * c.T
    b = ut * 8 + c.U * (2 + 2 * c.n_ks) * 8 + ut * splits * 4 + ut * 4 + ut * 4 + c.U * 4
    if c.cap:
        b = (b + 7) // 8 * 8 + splits * cps * c.G * 16 + ut * c.G * 4 + ut * 4 + ut * 4
    return b


# ---------------------------------------------------------------------------------------- 1 case tables and routes
# pool: 0 none, 1 prior + stamps and windows, 2 prior only, 3 stamps and windows only.  cap: 0 = no caps, else c with G groups
# (ung: every tenth news in no group).  sample: 0 plain, 1 tau = 0, 2 tau > 0; opt: m = out_model, t = tau_u, k = user_keys given.
TkCase = collections.namedtuple("TkCase", "name kind N U V k splits E csr pool cap G ung sample opt pad")
RkCase = collections.namedtuple("RkCase", "name kind N U V T splits E csr pool cap G ung n_ks sums pad")
MmCase = collections.namedtuple("MmCase", "name kind N U V M k cap G pen_u pad")
TK_NS = (4, 28, 32, 36, 64, 68, 400, 1020, 1024)
TK_VS = (2, 3, 128, 129, 130, 257)
TK_KS = (1, 63, 64, 65, 127, 128)
TK_SPLITS = (0, 1, 2, 5)                       # 5 slices of at most 2 chunks: empty slices
TK_ES = (0, 1, 63, 64)
RK_TS = (1, 4, 5, 63, 64)
RK_NKS = (0, 1, 8)
MM_MS = (1, 31, 32, 33, 64, 65, 96, 97, 128)
CSR_LENGTHS = (0, 1, 64, 65, 129, 300)
SPECIALS = ("zeros", "inf", "subnormal")
GAUSS_WIDE_K = 8                               # k of the Gaussian cases at N >= 400: the longest head of a row that the 90 % condition leaves
# Seeds of the Gaussian cases whose first draw left a user tile without a decided row or fewer than 90 % of the rows decided in the
# fp64 reference (tests/test_corpus_sweep_host.py asserts the condition for every case); every other case draws with 0.
SEEDS = {"gauss-sample-prior": 1, "gauss-25": 1, "gauss-35": 2}
TK_ROUTES = tuple(f"tile_{t}" for t in (64, 32, 16)) + tuple(f"select_p{p}g{g}c{x}s{s}" for s in (0, 1) for p in (0, 1) for g in (0, 1) for x in (0, 1) if p or not s) + (
    "merge_plain", "merge_group", "list_none", "list_dense", "list_csr", "splits_auto", "splits_given", "empty_slices", "model_null", "model_given",
    "tau_scalar", "tau_u", "keys_null", "keys_given")
RK_ROUTES = tuple(f"named_{n}_p{p}g{g}" for n in ("dense", "csr") for p in (0, 1) for g in (0, 1)) + tuple(
    f"count_tu{t}_p{p}_gb{b}" for t, b in ((64, 0), (64, 1), (64, 2), (32, 0), (32, 1), (32, 2), (32, 4), (16, 0), (16, 1), (16, 2), (16, 4), (16, 8)) for p in (0, 1)) + (
    "final_plain", "final_group", "reduce_on", "reduce_off", "nks_0", "nks_1", "nks_8")
MM_ROUTES = tuple(f"mb{b}_c{x}_p{p}" for b in (1, 2, 3, 4) for x in (0, 1) for p in (0, 1))


def _u_of(tile, j):
    return (1, tile - 1, tile, tile + 1)[j % 4]


def topk_cases():
    cs, i = [], 0
    for kind in ("lattice", "gauss"):
        for s, p, g, x in itertools.product((0, 2, 1), (0, 1), (0, 1), (0, 1)):
            N, k = TK_NS[i % 9], TK_KS[(i // 2) % 6]
            if kind == "gauss" and N >= 400:                                # the 90 % condition: at these widths only the head of a row is decided
                k = GAUSS_WIDE_K
            cap, G = g * (1, 3, 20)[i % 3], g * (4, 8, 40)[(i // 3) % 3]
            if kind == "gauss" and g:                                       # and a capped walk that cannot fill goes through the whole order
                k = max(1, min(k, cap * G * 3 // 4))                            # three quarters of what the caps let through: groups saturate, the row still fills
            tile = user_tile(N, 8 * k + 4)
            opt = "" if not s else ("m" if i % 2 else "") + ("t" if (i // 2) % 2 else "") + ("k" if (i // 4 + i) % 2 else "")
            cs.append(TkCase(f"{kind}-{i}", kind, N, _u_of(tile, i + i // 4), TK_VS[(i + i // 6) % 6], k, TK_SPLITS[(i + i // 4) % 4], 0 if x else TK_ES[(i // 2 + i // 8) % 4],
                             x, p * (1 + i % 3), cap, G, True, s, opt, i % 3))
            i += 1
    for tile, N, k in ((64, 68, 64), (32, 400, 65), (16, 1020, 127)):             # U = 1, TU - 1, TU, TU + 1 of every tile
        for j in range(4):
            kind = ("lattice", "gauss")[j % 2]
            kk, V = (k, (257, 130, 129, 128)[j]) if kind == "lattice" or tile == 64 else ({32: 63, 16: GAUSS_WIDE_K}[tile], 3 if tile == 32 else 257)     # gauss: the head of the row, see above (tile 32 needs k >= 38: two news and the fill)
            cs.append(TkCase(f"tile{tile}-u{j}", kind, N, _u_of(tile, j), V, kk, (2, 0, 1, 5)[j], (64, 0, 1, 63)[j], 0,
                             (0, 1, 2, 3)[j], 0, 0, True, (0, 0, 2, 0)[j], ("", "", "mtk", "")[j], j % 3))
    for kind in ("lattice", "gauss"):
        cs += [TkCase(f"{kind}-k1-splits1", kind, 36, 3, 130, 1, 1, 1, 0, 0, 0, 0, True, 0, "", 1),                   # the smallest merge: one key
               # the capped merge walk skips saturated groups and takes its 128th key inside a block of 64 (midblock_positions, asserted on the CPU)
               TkCase(f"{kind}-cap-midblock", kind, 28 if kind == "lattice" else 4, 5, 257, 128, 2, 0, 0, 0, 18, 6, True, 0, "", 2),
               TkCase(f"{kind}-cap-cannot-fill", kind, 64 if kind == "lattice" else 4, 5, 257, 63, 0, 0, 1, 0, 5, 3, False, 0, "", 0)]           # G c = 15 < k: 15 entries, then fill
    cs += [TkCase("gauss-sample-prior", "gauss", 36, 9, 257, 64, 2, 0, 0, 2, 0, 0, True, 2, "mt", 1),              # sampled rows long enough for the bound and for `agree`
           TkCase("gauss-sample-pool-csr", "gauss", 64, 7, 130, 63, 0, 0, 1, 1, 0, 0, True, 2, "k", 2),
           TkCase("gauss-sample-caps", "gauss", 28, 6, 257, 40, 1, 64, 0, 3, 4, 8, True, 2, "mtk", 0)]                  # caps that bind before the row is full
    cs += [TkCase(f"special-{n}", "special", 32 if n == "zeros" else 4 if n == "inf" else 8, 3, 6 if n == "zeros" else 10 if n == "inf" else 40, 8, (0, 2, 1)[j],
                  0, 0, 1 if n == "inf" else 0, 0, 0, True, 0, "", j) for j, n in enumerate(SPECIALS)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def topk_route(c):
    """topk_run: the tile of score_user_tile(N, 8 k + 4); topk_select_kernel<MT, POOL || SAMPLE, GROUP, CSR, SAMPLE> (a CSR call is one
    with n_excl > 0); topk_merge_group_kernel with caps, else topk_merge_kernel; sample_model_kernel when out_model is given."""
    TU, splits = tk_plan(c)
    per = (c.V - 1 + splits - 1) // splits
    r = [f"tile_{TU}", f"select_p{int(bool(c.pool or c.sample))}g{int(bool(c.cap))}c{c.csr}s{int(bool(c.sample))}", "merge_group" if c.cap else "merge_plain",
         "list_csr" if c.csr else "list_dense" if c.E else "list_none", "splits_given" if c.splits else "splits_auto"]
    if 1 + (splits - 1) * per >= c.V:
        r.append("empty_slices")
    if c.sample:
        r += ["model_given" if "m" in c.opt else "model_null", "tau_u" if "t" in c.opt else "tau_scalar", "keys_given" if "k" in c.opt else "keys_null"]
    return tuple(r)


RK_PAIRS = ((36, 0), (36, 5), (36, 100), (512, 0), (512, 5), (512, 100), (36, 200), (1024, 0), (1024, 5), (1024, 100), (1020, 200), (68, 400))


def rank_cases():
    """N = 512 is here for one reason: without caps no width of the issue's list gives the counting pass its 32-user tile."""
    cs, i = [], 0
    for kind in ("lattice", "gauss"):
        for x, p, g in itertools.product((0, 1), (0, 1), (0, 1)):
            N = TK_NS[(2 * i + 1) % 9]
            c = RkCase(f"{kind}-{i}", kind, N, 1, TK_VS[(i + 2) % 6], (1, 4)[i % 2] if g else RK_TS[i % 5], TK_SPLITS[(i + i // 4) % 4], 0 if x else TK_ES[(i // 2 + 1) % 4],
                       x, p * (1 + i % 3), g * (1, 3)[i % 2], g * (5, 40)[(i // 2) % 2], True, RK_NKS[i % 3], i % 3 != 1, i % 3)
            cs.append(c._replace(U=_u_of(rk_plan(c)[0], i)))
            i += 1
    for kind in ("lattice", "gauss"):
        for j, ((N, G), p) in enumerate(itertools.product(RK_PAIRS, (0, 1))):          # every rank_count_kernel<MT, POOL, GB> that exists, once per kind
            c = RkCase(f"{kind}-N{N}-G{G}-p{p}", kind, N, 1, TK_VS[2 + (j + i) % 4], (4, 1)[j % 2] if G else RK_TS[(j + i) % 5], TK_SPLITS[(j + i // 2) % 4], 0 if j % 3 == 0 else TK_ES[j % 4],
                       int(j % 3 == 0), p * (1 + (j // 2) % 3), (2, 1, 7)[j % 3] if G else 0, G, j % 2 == 0, RK_NKS[(j + 1) % 3], j % 4 != 3, j % 3)
            cs.append(c._replace(U=_u_of(rk_plan(c)[0], i)))
            i += 1
    cs += [RkCase("lattice-capped-out-sums", "lattice", 28, 9, 257, 4, 2, 0, 0, 0, 1, 3, False, 8, True, 1)]           # cap 1 of 3 groups: nearly every target capped out
    cs += [RkCase(f"special-{n}", "special", 32 if n == "zeros" else 4 if n == "inf" else 8, 3, 6 if n == "zeros" else 10 if n == "inf" else 40,
                  7 if n == "zeros" else 11 if n == "inf" else 41, (0, 2, 1)[j], 0, 0, 1 if n == "inf" else 0, 0, 0, True, 1, True, j) for j, n in enumerate(SPECIALS)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def rank_route(c):
    """nr_score_rank: rank_named_csr_kernel<POOL, GROUP> when n_excl > 0, else rank_named_kernel<POOL, GROUP>; rank_count_kernel<MT, POOL,
    GB> on the tile of rk_plan; rank_final_group_kernel with caps, else rank_final_kernel; rank_reduce_kernel when out_sums is given."""
    TU = rk_plan(c)[0]
    p, g = int(bool(c.pool)), int(bool(c.cap))
    return (f"named_{'csr' if c.csr else 'dense'}_p{p}g{g}", f"count_tu{TU}_p{p}_gb{rk_blocks(c.G if c.cap else 0)}", "final_group" if g else "final_plain",
            "reduce_on" if c.sums else "reduce_off", f"nks_{c.n_ks}")


def mmr_cases():
    cs = []
    for i, (M, x, p) in enumerate(itertools.product(MM_MS, (0, 1), (0, 1))):
        kind, k = ("lattice", "gauss")[(i + i // 4) % 2], 1 if i % 3 == 0 else M
        N = TK_NS[i % 6 if kind == "gauss" and M > 33 and k == M else i % 9]       # the 90 % condition: a long walk over wide vectors is never decided
        cs.append(MmCase(f"M{M}-c{x}-p{p}", kind, N, (1, 3, 7)[i % 3], 130, M, k, x * (1, 3)[i % 2], (4, 40)[(i // 2) % 2], p, i % 3))
    cs.append(MmCase("special-pool", "special", 8, 2, 20, 10, 10, 0, 4, 1, 1))
    assert len({c.name for c in cs}) == len(cs)
    return cs


def mmr_route(c):
    """nr_mmr_select: mmr_select_kernel<MB>, MB = ceil(M / 32); caps and penalty_u are run-time branches of the walk."""
    return (f"mb{(c.M + 31) // 32}_c{int(bool(c.cap))}_p{c.pen_u}",)


# ---------------------------------------------------------------------------------------- 2 inputs
def _vectors(kind, V, U, N, rng):
    if kind == "lattice":
        news, user = rng.integers(-2, 3, (V, N)).astype(f32), rng.integers(-2, 3, (U, N)).astype(f32)
    else:
        news = (rng.standard_normal((V, N)) * 10.0 ** rng.uniform(-3, 3, (V, 1))).astype(f32)
        user = (rng.standard_normal((U, N)) * 10.0 ** rng.uniform(-3, 3, (U, 1))).astype(f32)
    news[0] = 3e37
    return news, user


def _special(name):
    """news, user, prior, stamp, window and the fp32 dot products [U, V] the chain gives (column 0 is never looked at)."""
    if name == "zeros":          # N = 32, one slab and no padding column: user 0 x news 1 is -2^-200 thirty-two times, a chain that stays -0
        t = f32(2.0 ** -100)
        news = np.zeros((6, 32), f32)
        news[1], news[3], news[5] = -t, t, 1.0
        news[4] = t * np.where(np.arange(32) % 2 == 0, 1.0, -1.0).astype(f32)
        user = np.zeros((3, 32), f32)
        user[0], user[2] = t, -t
        dots = np.zeros((3, 6), f32)
        dots[0, 5], dots[2, 5] = 32 * t, -32 * t
        return SimpleNamespace(news=news, user=user, prior=None, stamp=None, window=None, dots=dots)
    if name == "inf":            # N = 4: every user is (1, 1, 0, 0), so a dot product is column 0 plus column 1
        big = f32(3e38)
        news = np.zeros((10, 4), f32)
        news[1, 0] = news[2, 0] = news[9, 0] = -INF
        news[3, :2], news[4, :2], news[8, :2] = big, -big, big
        news[5, 0] = NAN
        news[6, :2], news[7, 0] = (1.0, 2.0), 5.0
        user = np.zeros((3, 4), f32)
        user[:, :2] = 1.0
        prior = np.full(10, 0.25, f32)
        prior[6], prior[7], prior[8], prior[9] = INF, -INF, -INF, INF
        dots = np.tile(np.array([NAN, -INF, -INF, INF, -INF, NAN, 3.0, 5.0, INF, -INF], f32), (3, 1))
        return SimpleNamespace(news=news, user=user, prior=prior, stamp=np.zeros(10, i32), window=np.array([[0, 0], [-3, 4], [1, 0]], i32), dots=dots)
    rng = _rng(7, 7)             # subnormal: products on the 2^-145 grid, sums below 2^-126
    news = (rng.integers(-2, 3, (40, 8)) * 2.0 ** -75).astype(f32)
    user = (rng.integers(-2, 3, (3, 8)) * 2.0 ** -70).astype(f32)
    dots = (user.astype(f64) @ news.astype(f64).T).astype(f32)
    assert (dots.astype(f64) == user.astype(f64) @ news.astype(f64).T).all() and (np.abs(dots) < 2.0 ** -126).all() and (dots != 0).any()
    return SimpleNamespace(news=news, user=user, prior=None, stamp=None, window=None, dots=dots)


def _segments(U, V, rng, lengths=CSR_LENGTHS):
    """CSR lists: user u's segment has length lengths[u % 6], strictly ascending, drawn from [-L, V + L) so that entries <= 0 and
    >= V sit at its two ends; the last offset exceeds n_excl (the kernels clamp it)."""
    segs = []
    for u in range(U):
        L = lengths[(u + 1) % len(lengths)] if U < len(lengths) else lengths[u % len(lengths)]
        segs.append(np.sort(rng.choice(np.arange(-L, V + L), L, replace=False)).astype(i32))
    xids = np.concatenate(segs + [np.zeros(0, i32)]).astype(i32)
    if xids.size == 0:
        xids = np.array([1], i32)
        segs[-1] = xids
    off = np.zeros(U + 1, i32)
    off[1:] = np.cumsum([len(s) for s in segs])
    off[U] += 7
    return off, xids, segs


def corpus_inputs(c):
    """Everything a top-k, sampled or rank case reads, as plain numpy arrays in their logical shapes."""
    tk = isinstance(c, TkCase)
    rng = _rng(1 if tk else 2, c.N, c.U, c.V, c.k if tk else c.T, c.E, c.csr, c.pool, c.cap, c.pad, c.kind == "gauss", SEEDS.get(c.name, 0))
    I = SimpleNamespace(prior=None, stamp=None, window=None, exclude=None, offsets=None, xids=None, segs=None, group=None, dots=None, tau=0.0, tau_u=None, keys=None,
                        seed=0x5EED00012345678 + c.N * 1000 + c.V, draw=c.pad + 1, targets=None, ks=())
    if c.kind == "special":
        s = _special(c.name.split("-", 1)[1])
        I.news, I.user, I.prior, I.stamp, I.window, I.dots = s.news, s.user, s.prior, s.stamp, s.window, s.dots
        I.news[0] = 3e37
    else:
        I.news, I.user = _vectors(c.kind, c.V, c.U, c.N, rng)
        if c.pool in (1, 2):
            su = np.abs(I.news[:, :1]).max(axis=1) if c.kind == "gauss" else 1.0
            I.prior = (rng.integers(-32, 33, c.V) / 4.0).astype(f32) if c.kind == "lattice" else (rng.standard_normal(c.V) * su).astype(f32)
            I.prior[3::7] = -INF
        if c.pool in (1, 3):
            lo = rng.integers(0, 4, c.U)
            I.stamp, I.window = rng.integers(0, 10, c.V).astype(i32), np.stack([lo, lo + rng.integers(3, 7, c.U)], axis=1).astype(i32)
            if c.U >= 3:
                I.window[2] = (5, 4)                                       # lo > hi: nobody
    with np.errstate(all="ignore"):
        r = I.user.astype(f64) @ I.news.astype(f64).T
    I.best = (1 + np.nan_to_num(r[:, 1:], nan=-INF).argmax(axis=1)).astype(i32)
    if c.E:
        I.exclude = rng.integers(-2, c.V + 2, (c.U, c.E)).astype(i32)
        I.exclude[::2, 0] = I.best[::2]
    if c.csr:
        I.offsets, I.xids, I.segs = _segments(c.U, c.V, rng)
    if c.cap:
        I.group = rng.integers(0, c.G, c.V).astype(i32)
        if c.ung:
            I.group[::10] = -1 - (np.arange(c.V)[::10] // 10) % 3
    if tk and c.sample:
        I.tau = 0.0 if c.sample == 1 else 0.75
        if "t" in c.opt:
            I.tau_u = np.zeros(c.U, f32) if c.sample == 1 else np.array([0.3, 1.7, 0.0, 0.75, 1e-3, 30.0], f32)[np.arange(c.U) % 6]     # no powers of two: tau g must round
            if c.sample == 2 and c.U >= 5:
                I.tau_u[1], I.tau_u[3], I.tau_u[4] = -1.0, NAN, INF         # three all-fill rows
        if "k" in c.opt:
            I.keys = rng.integers(-2 ** 31, 2 ** 31, c.U).astype(i32)
    if not tk:
        I.targets = rng.integers(-1, c.V + 2, (c.U, c.T)).astype(i32)
        if c.kind == "gauss":        # held-out clicks from the head of the user's ranking, where the order is decided; one stray entry
            head = min(2 if c.N >= 400 else 16, c.V - 1)
            top = 1 + np.argsort(-np.nan_to_num(r[:, 1:], nan=-INF), axis=1, kind="stable")[:, :head]
            stray = np.array([-1, 0, c.V, c.V + 1], i32)[rng.integers(0, 4, c.U)]
            I.targets = np.take_along_axis(top, rng.integers(0, head, (c.U, c.T)), axis=1).astype(i32)
            if c.T >= 3:
                I.targets[:, c.T // 2] = stray
        I.targets[::3, -1] = I.best[::3]
        if c.T >= 2:
            I.targets[1::2, 1] = I.targets[1::2, 0]                          # a repeat
        if c.kind == "special":
            I.targets = np.tile(np.arange(c.T, dtype=i32), (c.U, 1))         # every id, 0 and V included
        I.ks = {0: (), 1: (10,), 8: (1, 2, 5, 10, 63, 64, 128, c.V + 5)}[c.n_ks]
    return I


def mmr_inputs(c):
    rng = _rng(3, c.N, c.U, c.M, c.k, c.cap, c.pen_u, c.pad)
    I = SimpleNamespace(group=None, penalty=(0.5, 2.0, 8.0)[c.M % 3], penalty_u=None)
    if c.kind == "gauss":
        I.news = (rng.standard_normal((c.V, c.N)) * 10.0 ** rng.uniform(-3, 3, (c.V, 1))).astype(f32)
        I.pool_ids = np.stack([rng.choice(np.arange(1, c.V), c.M, replace=False) for _ in range(c.U)]).astype(i32)
        if c.pen_u:              # score scales from 1e-3 to 1e3 with a penalty in proportion; under the scalar penalty scores of its size
            su = 10.0 ** rng.uniform(-3, 3, c.U)
            I.penalty_u = (su * np.array([0.5, 0.25, 1.0])[np.arange(c.U) % 3]).astype(f32)
        else:
            su = I.penalty * rng.uniform(0.5, 2.0, c.U)
        I.pool_scores = (rng.standard_normal((c.U, c.M)) * su[:, None]).astype(f32)
    else:
        nnz = np.array([n for n in (1, 4, 16, 64) if n <= c.N])[rng.integers(0, sum(n <= c.N for n in (1, 4, 16, 64)), c.V)]
        order = rng.random((c.V, c.N)).argsort(axis=1).argsort(axis=1)
        I.news = (np.where(rng.integers(0, 2, (c.V, c.N)) == 1, 1.0, -1.0) * (order < nnz[:, None])).astype(f32)
        I.news[5], I.news[7] = 0.0, I.news[6]
        I.pool_ids = rng.integers(1, min(c.V, 24), (c.U, c.M)).astype(i32)            # few ids: repeats, identical vectors
        I.pool_scores = (rng.integers(-32, 33, (c.U, c.M)) / 4.0).astype(f32)
        if c.M >= 4:
            I.pool_ids[:, 1], I.pool_ids[:, -1] = 0, c.V + 3                                  # not live: never taken, never an address
            I.pool_scores[:, 2] = NAN
        if c.pen_u:
            I.penalty_u = np.array([2.0, 0.0, 0.5, 8.0], f32)[np.arange(c.U) % 4]
        if c.kind == "special":    # +0 and -0 tie (the lowest place first, each with its own bits), -inf and +inf are live scores
            I.pool_scores[:, 3:9] = np.array([0.0, -0.0, -INF, INF, -0.0, 0.0], f32)
            I.pool_ids[:, 3:9] = np.array([8, 9, 10, 11, 12, 5], i32)
            I.penalty_u = np.array([0.0, 2.0], f32)
    I.news[0] = 3e37
    if c.cap:
        I.group = rng.integers(0, c.G, c.V).astype(i32)
        I.group[::10] = -1
    return I


# ---------------------------------------------------------------------------------------- 3 references
def philox_bits(seed, draw, keys, ids):
    """include/nrhip.h K12 in numpy uint32 / uint64: Philox4x32-10(counter = (v >> 2, a, draw, 0), key = (seed lo, seed hi))[v & 3]."""
    a, v = np.asarray(keys).astype(np.int64).astype(np.uint32), np.asarray(ids).astype(np.int64).astype(np.uint32)
    c = [(v >> np.uint32(2)).astype(np.uint64), a.astype(np.uint64), np.full(v.shape, draw & 0xFFFFFFFF, np.uint64), np.zeros(v.shape, np.uint64)]
    k0, k1, m = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.choose(v & np.uint32(3), [x.astype(np.uint32) for x in c])


def gumbel64(bits):
    """u = ((bits >> 8) + 0.5) 2^-24, g = -log(-log(u)) in fp64; the upper half through log1p of the exact 1 - u."""
    m = (bits >> np.uint32(8)).astype(f64)
    low = m < 2.0 ** 23
    t = np.where(low, -np.log(np.where(low, (2 * m + 1) * 2.0 ** -25, 0.5)), -np.log1p(-np.where(low, 0.5, (2.0 ** 25 - 2 * m - 1) * 2.0 ** -25)))
    return -np.log(t)


def noise_check(seed, draw, keys, ids, g, bits):
    same_bits("noise", "bits", np.asarray(bits).view(np.uint32), philox_bits(seed, draw, keys, ids))
    ref = gumbel64(philox_bits(seed, draw, keys, ids))
    err = np.abs(np.asarray(g, f64) - ref)
    bound = 7 * 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
    need(bool((err <= bound).all()), "noise", "g: {} values outside 7 2^-23 max(1, |g|), worst ratio {:.3g}", int((~(err <= bound)).sum()), float(np.nanmax(err / bound)))
    return float((err / bound).max(initial=0.0))


def taus(c, I):
    """[U] fp32 temperatures of a sampled case, and the users whose entry is negative, NaN or infinite (all-fill rows)."""
    tau = I.tau_u if I.tau_u is not None else np.full(c.U, I.tau, f32)
    with np.errstate(invalid="ignore"):
        return tau, ~((tau >= 0) & (tau < INF))


def eligible(c, I):
    """[U, V] bool: id in [1, V), prior not -inf, stamp inside the window, not excluded or listed, a valid temperature.  (A NaN
    score is taken out where the scores are formed.)"""
    U, V = I.user.shape[0], I.news.shape[0]
    el = np.ones((U, V), bool)
    el[:, 0] = False
    if I.prior is not None:
        el &= ~np.isneginf(I.prior)[None, :]
    if I.stamp is not None:
        el &= (I.window[:, :1] <= I.stamp[None, :]) & (I.stamp[None, :] <= I.window[:, 1:2])
    for u in range(U):
        ex = I.exclude[u] if I.exclude is not None else I.segs[u] if I.segs is not None else None
        if ex is not None:
            el[u, ex[(ex >= 1) & (ex < V)]] = False
    if isinstance(c, TkCase) and c.sample:
        el[taus(c, I)[1]] = False
    return el


def corpus_scores(c, I, g32=None):
    """(r, b): the final scores [U, V] in fp64 and the per-pair bound of the module docstring; b is None where the fp32 result is
    exact (lattice and special data: r is then formed in fp32 steps, as the header states them).  g32: the probe's g [U, V] of a
    sampled case with tau > 0."""
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    sampled = isinstance(c, TkCase) and c.sample == 2
    with np.errstate(all="ignore"):
        dot = I.dots.astype(f64) if I.dots is not None else u64 @ n64.T
        if c.kind != "gauss":
            s = dot.astype(f32)
            need(bool(((s.astype(f64) == dot) | np.isnan(dot))[:, 1:].all()), "exact", "a {} dot product is not a fp32 number", c.kind)
            if sampled:
                tau = np.where(taus(c, I)[1], f32(0), taus(c, I)[0]).astype(f32)
                s = s + ((I.prior if I.prior is not None else f32(0)) + tau[:, None] * g32)           # three fp32 roundings, as the header orders them
            elif I.prior is not None:
                s = s + I.prior[None, :]
            return s.astype(f64), None
        N = I.news.shape[1]
        b = (1 + CORPUS_CHAIN_EXCESS) * N * U32 / (1 - N * U32) * (np.abs(u64) @ np.abs(n64).T) + N * F149
        r = dot
        pri = I.prior.astype(f64)[None, :] if I.prior is not None else 0.0
        if sampled:
            tg = np.where(taus(c, I)[1], 0.0, taus(c, I)[0].astype(f64))[:, None] * g32.astype(f64)
            P = pri + tg
            r = dot + P
            b = b + U32 * np.abs(tg) + U32 * np.abs(P) + U32 * np.abs(r) + 3 * F149
        elif I.prior is not None:
            r = dot + pri
            b = b + U32 * np.abs(r) + F149
        return r, np.where(np.isfinite(b), b, 0.0)


def order_of(r, el, u):
    """User u's eligible news without a NaN score in the total order: score descending (-0 == +0), id ascending."""
    idx = np.flatnonzero(el[u] & ~np.isnan(r[u]))
    return idx[np.lexsort((idx, -r[u, idx]))]


def capped_walk(order, group, cap):
    """The walk of the header: (taken ids in order, skipped ids): a news is taken unless its group (>= 0) already has cap taken."""
    if group is None:
        return order, order[:0]
    taken, skipped, cnt = [], [], {}
    for v in order.tolist():
        g = int(group[v])
        if g >= 0 and cnt.get(g, 0) >= cap:
            skipped.append(v)
            continue
        cnt[g] = cnt.get(g, 0) + 1
        taken.append(v)
    return np.array(taken, np.int64), np.array(skipped, np.int64)


def midblock_positions(c, I, r, el):
    """Per user of a capped case: the 1-based position in the merge's sorted list (every slice's own capped row of at most k keys, as
    topk_select_kernel leaves them) at which topk_merge_group_kernel takes its k-th key, 0 when the row never fills."""
    splits = tk_plan(c)[1]
    per = (c.V - 1 + splits - 1) // splits
    out = []
    for u in range(c.U):
        order = order_of(r, el, u)
        kept = np.concatenate([capped_walk(order[(order >= 1 + s * per) & (order < 1 + (s + 1) * per)], I.group, c.cap)[0][:c.k] for s in range(splits)])
        merged = order[np.isin(order, kept)]
        taken = capped_walk(merged, I.group, c.cap)[0]
        out.append(int(np.flatnonzero(merged == taken[c.k - 1])[0]) + 1 if len(taken) >= c.k else 0)
    return out


def topk_ref(c, I, r, el):
    """(ids int32 [U, k], scores fp64 [U, k]) of the contract on the scores r."""
    ids, sc = np.zeros((c.U, c.k), i32), np.full((c.U, c.k), -INF)
    for u in range(c.U):
        row = capped_walk(order_of(r, el, u), I.group, c.cap)[0][:c.k]
        ids[u, :len(row)], sc[u, :len(row)] = row, r[u, row] + 0.0
    return ids, sc


def rank_ref(c, I, r, el):
    """(ranks int32 [U, T], scores fp64 [U, T]): 0 / -inf for what is not ranked, -1 with its score for a capped-out target."""
    V = I.news.shape[0]
    ranks, sc = np.zeros((c.U, c.T), i32), np.full((c.U, c.T), -INF)
    for u in range(c.U):
        taken, skipped = capped_walk(order_of(r, el, u), I.group, c.cap)
        place = np.zeros(V, np.int64)
        place[taken], place[skipped] = np.arange(1, len(taken) + 1), -1
        seen = set()
        for j, t in enumerate(I.targets[u].tolist()):
            if 1 <= t < V and t not in seen and place[t] != 0:
                ranks[u, j], sc[u, j] = place[t], r[u, t] + 0.0
            seen.add(t)
    return ranks, sc


def band(r, b, el, u):
    """(eligible ids, sure, maybe) of user u: how many eligible news beat each one for certain / may beat it."""
    idx = np.flatnonzero(el[u] & ~np.isnan(r[u]))
    lo, hi = r[u, idx] - b[u, idx], r[u, idx] + b[u, idx]
    sure = (lo[None, :] > hi[:, None]).sum(axis=1)
    maybe = (hi[None, :] >= lo[:, None]).sum(axis=1) - 1
    return idx, sure, maybe


def sums_ref(ranks, ks):
    """The header's out_sums from ranks [U, T]: (sums, sum of |terms|), each 2 + 2 len(ks) long; fsum and math.log2 throughout."""
    rows = []
    for row in np.asarray(ranks).tolist():
        n, pos = sum(1 for x in row if x != 0), sorted(x for x in row if x > 0)
        if n == 0:
            rows.append([0.0] * (2 + 2 * len(ks)))
            continue
        t = [1.0, math.fsum(1.0 / x for x in pos) / n]
        for k in ks:
            hit = [x for x in pos if x <= k]
            t += [len(hit) / n, math.fsum(1.0 / math.log2(x + 1.0) for x in hit) / math.fsum(1.0 / math.log2(i + 1.0) for i in range(1, min(n, k) + 1))]
        rows.append(t)
    cols = list(zip(*rows)) if rows else [()] * (2 + 2 * len(ks))
    return [math.fsum(col) for col in cols], [math.fsum(abs(x) for x in col) for col in cols]


def mmr_gram(c, I, u):
    """fp64 pieces of user u's pool: (live, group per place, r, sim [M, M], A-based error e_s [M, M] or None)."""
    V, N = I.news.shape
    pid, r = I.pool_ids[u].astype(np.int64), I.pool_scores[u].astype(f64)
    live = (pid >= 1) & (pid < V) & ~np.isnan(r)
    x = I.news.astype(f64)[np.where(live, pid, 0)] * live[:, None]
    gram = x @ x.T
    d = np.diag(gram)
    with np.errstate(all="ignore"):
        rn = np.where(d > 0, 1.0 / np.sqrt(d), 0.0)
    sim = gram * rn[:, None] * rn[None, :]
    grp = np.where(live, I.group[np.where(live, pid, 0)], -1) if I.group is not None else np.full(len(pid), -1)
    e_s = None
    if c.kind == "gauss":
        gam = (1 + CORPUS_CHAIN_EXCESS) * N * U32 / (1 - N * U32)
        e_s = (gam * (np.abs(x) @ np.abs(x).T) * rn[:, None] * rn[None, :] + np.abs(sim) * (gam + 6 * U32)) * (1 + 2.0 ** -10) + N * F149
    return live, grp, r, sim, e_s


def mmr_penalty(c, I, u):
    return float(I.penalty_u[u]) if I.penalty_u is not None else float(f32(I.penalty))


def mmr_ref(c, I):
    """(ids, scores fp64, places, margins) of the header's walk in fp64, user by user."""
    ids, sc = np.zeros((c.U, c.k), i32), np.full((c.U, c.k), -INF)
    pl, margins = np.full((c.U, c.k), -1, i32), np.full((c.U, c.k), INF)
    for u in range(c.U):
        live, grp, r, sim, _ = mmr_gram(c, I, u)
        p, taken, cnt, maxsim = mmr_penalty(c, I, u), np.zeros(c.M, bool), {}, np.full(c.M, -INF)
        for t in range(c.k):
            cand = live & ~taken & np.array([g < 0 or cnt.get(int(g), 0) < c.cap for g in grp])
            if not cand.any():
                break
            with np.errstate(invalid="ignore"):
                val = r if t == 0 else r - p * maxsim
            best = np.where(cand, val, -INF).max()
            j = int(np.flatnonzero(cand & (val == best))[0])
            others = cand.copy()
            others[j] = False
            with np.errstate(invalid="ignore"):
                second = np.where(others, val, -INF).max() if others.any() else -INF
                margins[u, t] = INF if not others.any() else 0.0 if best == second else best - second
            ids[u, t], sc[u, t], pl[u, t], taken[j] = I.pool_ids[u, j], r[j], j, True
            if grp[j] >= 0:
                cnt[int(grp[j])] = cnt.get(int(grp[j]), 0) + 1
            maxsim = np.maximum(maxsim, sim[j])
    return ids, sc, pl, margins


def mmr_tol(c, I, u):
    live, _, r, _, e_s = mmr_gram(c, I, u)
    p = mmr_penalty(c, I, u)
    return 2.0 * (p * float(e_s.max()) + U32 * (float(np.abs(r[live]).max(initial=0.0)) + p))


def mmr_replay(c, I, u, places):
    """One device row replayed in fp64: every place it took was a candidate of its step; returns the largest (best candidate value -
    value of the place taken)."""
    live, grp, r, sim, _ = mmr_gram(c, I, u)
    p, taken, cnt, worst = mmr_penalty(c, I, u), np.zeros(c.M, bool), {}, 0.0
    for t, j in enumerate(places.tolist()):
        cand = live & ~taken & np.array([g < 0 or cnt.get(int(g), 0) < c.cap for g in grp])
        if j < 0:
            need(not cand.any() and (places[t:] < 0).all(), "bound", "user {}: the walk ended at step {} with candidates left", u, t)
            break
        need(0 <= j < c.M and bool(cand[j]), "bound", "user {} step {}: place {} is no candidate", u, t, j)
        val = r if t == 0 else r - p * sim[:, taken].max(axis=1)
        worst = max(worst, float(val[cand].max() - val[j]))
        taken[j] = True
        if grp[j] >= 0:
            cnt[int(grp[j])] = cnt.get(int(grp[j]), 0) + 1
    return worst


# ---------------------------------------------------------------------------------------- 4 problems: the buffers of one call
def strides(c, variant):
    """Row strides of a call: `dense` = the widths, else the padded ones of the module docstring, chosen by c.pad."""
    N = c.N
    if variant == "dense":
        return SimpleNamespace(news=N, user=N, excl=getattr(c, "E", 0), tgt=getattr(c, "T", 0), win=2, pid=getattr(c, "M", 0), psc=getattr(c, "M", 0))
    o = (N, N + 4, tk_npad(N) + 8)
    return SimpleNamespace(news=o[c.pad], user=o[(c.pad + 1) % 3], excl=getattr(c, "E", 0) + (3 if c.pad != 1 else 0), tgt=getattr(c, "T", 0) + (1 if c.pad != 2 else 0),
                           win=5 if c.pad != 0 else 2, pid=getattr(c, "M", 0) + c.pad, psc=getattr(c, "M", 0) + 3 - c.pad)


def in_buf(arr, ld, dev, off, slack=None):
    """An input as [guard][rows x ld][guard]: the payload in the first columns, `slack` (a scalar or [rows, ld - cols]) behind
    them.  Nothing of it may change: .own is empty."""
    arr = np.ascontiguousarray(arr if np.ndim(arr) == 2 else np.reshape(arr, (1, -1)))
    t = torch.from_numpy(arr)
    b = glue_buf(arr.shape[0], arr.shape[1], ld, t.dtype, dev, off, t.to(dev))
    if b.ld > arr.shape[1] and slack is not None:
        full = b.flat[b.start:b.start + b.rows * b.ld].view(b.rows, b.ld)
        full[:, arr.shape[1]:] = torch.as_tensor(slack, dtype=t.dtype).to(dev) if np.ndim(slack) else slack
    b.own[:] = False
    b.init = b.flat.clone()
    return b


def out_buf(rows, cols, tdt, dev, off):
    return glue_buf(rows, cols, cols, tdt, dev, off, NAN if tdt.is_floating_point else IFILL)


def problem(entry, c, I, dev, variant="pad"):
    """Every buffer of one call of `entry` (topk, sample, rank, mmr) on case c with inputs I.  variant: pad (padded strides, the
    least alignment), dense (the widths as strides), shift (padded strides, every base moved by 16 bytes; 8 or 4 where that is all
    the header allows)."""
    S, sh = strides(c, variant), variant == "shift"
    fo, io, wo = (0 if sh else 4), (2 if sh else 1), (4 if sh else 2)        # elements in front: fp32 vectors, 4-byte arrays, the workspace (int32 units)
    P = SimpleNamespace(entry=entry, c=c, I=I, S=S, inb={}, outb={}, ws=None)
    P.inb["news"] = in_buf(I.news, S.news, dev, fo, NAN)
    if entry == "mmr":
        ok = 1 if c.V > 1 else 0
        P.inb["pool_ids"] = in_buf(I.pool_ids, S.pid, dev, io, ok)
        P.inb["pool_scores"] = in_buf(I.pool_scores, S.psc, dev, io, INF)
        if I.penalty_u is not None:
            P.inb["penalty_u"] = in_buf(I.penalty_u, c.U, dev, io)
        if I.group is not None:
            P.inb["group"] = in_buf(I.group, c.V, dev, io)
        for k, tdt in (("ids", torch.int32), ("scores", torch.float32), ("place", torch.int32)):
            P.outb[k] = out_buf(c.U, c.k, tdt, dev, io)
        assert sh or (P.inb["news"].ptr % 32 == 16 and P.inb["pool_ids"].ptr % 8 == 4)
        return P
    P.inb["user"] = in_buf(I.user, S.user, dev, fo, NAN)
    if I.prior is not None:
        P.inb["prior"] = in_buf(I.prior, c.V, dev, io)
    if I.stamp is not None:
        P.inb["stamp"] = in_buf(I.stamp, c.V, dev, io)
        P.inb["window"] = in_buf(I.window, S.win, dev, io, np.tile(np.array([100, -100, 100], i32), (c.U, 1)))
    if I.exclude is not None:
        P.inb["exclude"] = in_buf(I.exclude, S.excl, dev, io, np.tile(I.best[:, None], (1, max(S.excl - c.E, 1))))
    if I.offsets is not None:
        P.inb["offsets"], P.inb["xids"] = in_buf(I.offsets, c.U + 1, dev, io), in_buf(I.xids, len(I.xids), dev, io)
    if I.group is not None:
        P.inb["group"] = in_buf(I.group, c.V, dev, io)
    if entry == "rank":
        V = c.V
        free = np.array([next((v for v in range(1, V) if v not in set(row.tolist())), 1) for row in I.targets], i32)
        P.inb["targets"] = in_buf(I.targets, S.tgt, dev, io, free[:, None])
        P.outb["ranks"], P.outb["scores"] = out_buf(c.U, c.T, torch.int32, dev, io), out_buf(c.U, c.T, torch.float32, dev, io)
        if c.sums:
            P.outb["sums"] = out_buf(1, 2 + 2 * c.n_ks, torch.float64, dev, 1)
        P.ws_bytes = rk_ws_bytes(c)
    else:
        if entry == "sample":
            if I.tau_u is not None:
                P.inb["tau_u"] = in_buf(I.tau_u, c.U, dev, io)
            if I.keys is not None:
                P.inb["keys"] = in_buf(I.keys, c.U, dev, io)
            if "m" in c.opt:
                P.outb["model"] = out_buf(c.U, c.k, torch.float32, dev, io)
        P.outb["ids"], P.outb["scores"] = out_buf(c.U, c.k, torch.int32, dev, io), out_buf(c.U, c.k, torch.float32, dev, io)
        P.ws_bytes = tk_ws_bytes(c)
    P.ws = glue_buf(1, P.ws_bytes // 4, P.ws_bytes // 4, torch.int32, dev, wo, IFILL)            # exactly 8-byte aligned, exactly the bytes asked for
    if not sh:                                                              # the least alignment the header allows, and no more
        assert P.inb["news"].ptr % 32 == 16 and P.inb["user"].ptr % 32 == 16 and P.ws.ptr % 16 == 8 and P.outb["scores"].ptr % 8 == 4
    return P


def noise_problem(seed, draw, keys, ids, dev):
    P = SimpleNamespace(entry="noise", seed=seed, draw=draw, n=len(ids), inb={}, outb={}, ws=None)
    P.inb["keys"], P.inb["ids"] = in_buf(np.asarray(keys, i32), len(ids), dev, 1), in_buf(np.asarray(ids, i32), len(ids), dev, 1)
    P.outb["g"], P.outb["bits"] = out_buf(1, len(ids), torch.float32, dev, 1), out_buf(1, len(ids), torch.int32, dev, 1)
    return P


def all_bufs(P):
    return list(P.inb.items()) + list(P.outb.items()) + ([("ws", P.ws)] if P.ws is not None else [])


def results(P):
    return {k: b.v.cpu().numpy().copy() for k, b in P.outb.items()}


def execute(entry, c, I, dev, call, variant="pad", twice=True):
    """One checked call: every guard and slack element intact (`sentinel`), a second problem built alike gives the same bits
    (`repeat`).  Returns the outputs as numpy arrays."""
    Ps = [problem(entry, c, I, dev, variant) for _ in range(2 if twice else 1)]
    for P in Ps:
        call(P)
    for name, b in all_bufs(Ps[0]):
        _as("sentinel", _sentinels, f"{entry} {name}", b)
    if twice:
        for (name, a), (_, b) in zip(Ps[0].outb.items(), Ps[1].outb.items()):
            need(torch.equal(_bits(a.flat), _bits(b.flat)), "repeat", "{} {}: two runs from the same state differ", entry, name)
    return results(Ps[0])


def probe(c, I, dev, call):
    """The g [U, V] fp32 nr_sample_noise gives the pairs of a sampled case, checked on the way (`noise`)."""
    keys = I.keys if I.keys is not None else np.arange(c.U, dtype=i32)
    kk, vv = np.repeat(keys, c.V), np.tile(np.arange(c.V, dtype=i32), c.U)
    P = noise_problem(I.seed, I.draw, kk, vv, dev)
    call(P)
    for name, b in all_bufs(P):
        _as("sentinel", _sentinels, f"noise {name}", b)
    out = results(P)
    noise_check(I.seed, I.draw, kk, vv, out["g"][0], out["bits"][0])
    return out["g"][0].reshape(c.U, c.V)


# ---------------------------------------------------------------------------------------- 5 the checker
def _layer(c):
    return {"lattice": "exact", "special": "special", "gauss": "bound"}[c.kind]


def _fill_ok(layer, what, ids, sc, n, extra=()):
    need(bool((ids[n:] == 0).all() and np.isneginf(sc[n:]).all() and all((x[n:] == fill).all() for x, fill in extra)), layer, "{}: the tail behind {} entries is not the fill", what, n)


def tk_check(c, I, got, g32=None):
    """A top-k or sampled result against the contract; returns the figures of the case."""
    layer = _layer(c)
    r, b = corpus_scores(c, I, g32)
    el = eligible(c, I)
    ids, sc = got["ids"], got["scores"]
    w = {}
    if b is None:
        ref_ids, ref_sc = topk_ref(c, I, r, el)
        same_bits(layer, "ids", ids, ref_ids)
        same_bits(layer, "scores", sc, ref_sc.astype(f32))
    else:
        decided = np.zeros(c.U, bool)
        worst = 0.0
        for u in range(c.U):
            idx, sure, maybe = band(r, b, el, u)
            at = {int(v): i for i, v in enumerate(idx)}
            n = min(c.k, len(idx)) if I.group is None else int((ids[u] != 0).sum())
            row, s = ids[u, :n], sc[u, :n]
            _fill_ok(layer, f"user {u}", ids[u], sc[u], n)
            need(len(set(row.tolist())) == n and all(int(v) in at for v in row), layer, "user {}: ids repeat or are not eligible", u)
            e = _as(layer, _within, "exact", f"scores of user {u}", torch.from_numpy(s.copy()), torch.from_numpy(r[u, row]), torch.from_numpy(b[u, row]))
            worst = max(worst, e)
            need(bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (row[:-1] < row[1:]))).all()), layer, "user {}: the row is not in (score descending, id ascending) order", u)
            if I.group is None:
                p = np.arange(n)
                j = np.array([at[int(v)] for v in row], np.int64)
                need(bool(((sure[j] <= p) & (p <= maybe[j])).all()), layer, "user {}: an entry sits at a place its score cannot have", u)
                need(bool(np.isin(idx[maybe < c.k], row).all()), layer, "user {}: a news that must be in the row is missing", u)
                ref_row = order_of(r, el, u)[:c.k]
                decided[u] = bool((sure[[at[int(v)] for v in ref_row]] == maybe[[at[int(v)] for v in ref_row]]).all())
            else:
                g = I.group[row]
                need(not (g >= 0).any() or int(np.bincount(g[g >= 0]).max()) <= c.cap, layer, "user {}: more than {} news of one group", u, c.cap)
                order = order_of(r, el, u)
                ref_row = capped_walk(order, I.group, c.cap)[0][:c.k]
                upto = int(np.flatnonzero(order == ref_row[-1])[0]) + 1 if len(ref_row) == c.k else len(order)
                pre = [at[int(v)] for v in order[:upto]]
                decided[u] = bool((sure[pre] == maybe[pre]).all())
                if decided[u]:                                              # the order is certain as far as the walk goes: one answer
                    need(n == len(ref_row) and bool((row == ref_row).all()), layer, "user {}: the capped row differs from the reference although every place is decided", u)
        w["ratio"], w["decided"], w["decided_rows"] = worst, float(decided.mean()), decided
    if "model" in got:                                                      # fl32(perturbed - fl32(tau g)) from the row itself and the probe
        tau = np.where(taus(c, I)[1], f32(0), taus(c, I)[0]).astype(f32)
        gg = g32 if g32 is not None else np.zeros((c.U, c.V), f32)
        with np.errstate(invalid="ignore"):
            want = np.where(ids > 0, sc - tau[:, None] * np.take_along_axis(gg, np.clip(ids, 0, c.V - 1).astype(np.int64), axis=1), f32(-INF)).astype(f32)
        same_bits(layer, "out_model", got["model"], want)
    return w


def rk_check(c, I, got):
    layer = _layer(c)
    r, b = corpus_scores(c, I)
    el = eligible(c, I)
    ranks, sc = got["ranks"], got["scores"]
    ref_r, ref_s = rank_ref(c, I, r, el)
    w = {}
    if b is None:
        same_bits(layer, "ranks", ranks, ref_r)
        same_bits(layer, "scores", sc, ref_s.astype(f32))
    else:
        decided, worst = np.zeros(c.U, bool), 0.0
        for u in range(c.U):
            idx, sure, maybe = band(r, b, el, u)
            at = {int(v): i for i, v in enumerate(idx)}
            order = order_of(r, el, u).tolist()
            ok = True
            for j, t in enumerate(I.targets[u].tolist()):
                if ref_r[u, j] == 0:
                    need(ranks[u, j] == 0 and np.isneginf(sc[u, j]), layer, "user {} target {}: rank {} score {} where the contract ranks nothing", u, j, ranks[u, j], sc[u, j])
                    continue
                i = at[t]
                worst = max(worst, _as(layer, _within, "exact", f"score of user {u} target {j}", torch.tensor([sc[u, j]]), torch.tensor([r[u, t]]), torch.tensor([b[u, t]])))
                if I.group is None:
                    need(1 + sure[i] <= ranks[u, j] <= 1 + maybe[i], layer, "user {} target {}: rank {} outside [{}, {}]", u, j, ranks[u, j], 1 + sure[i], 1 + maybe[i])
                    ok &= sure[i] == maybe[i]
                else:
                    pre = [at[v] for v in order[:order.index(t) + 1]]        # the walk as far as the target
                    sure_t = bool((sure[pre] == maybe[pre]).all())
                    ok &= sure_t
                    need(ranks[u, j] != 0, layer, "user {} target {}: not ranked", u, j)
                    need(not sure_t or ranks[u, j] == ref_r[u, j], layer, "user {} target {}: capped rank {} differs from {} although every place up to it is decided", u, j, ranks[u, j], ref_r[u, j])
            decided[u] = ok
        w["ratio"], w["decided"], w["decided_rows"] = worst, float(decided.mean()), decided
    if "sums" in got:
        sums, (want, mass) = got["sums"][0], sums_ref(ranks, I.ks)
        need(sums[0] == want[0], "sums", "sums[0] = {}, {} users have a ranked target", sums[0], want[0])
        for k in range(1, len(want)):
            bound = ((c.U + 2) * 2.0 ** -53 + CORPUS_LOG2_EXCESS) * mass[k]
            need(abs(sums[k] - want[k]) <= bound, "sums", "sums[{}] = {!r}, the header's formula on the ranks gives {!r}, bound {:.3g}", k, sums[k], want[k], bound)
            if mass[k]:
                w["sums"] = max(w.get("sums", 0.0), abs(sums[k] - want[k]) / ((c.U + 2) * 2.0 ** -53 * mass[k]))
    return w


def mm_check(c, I, got):
    layer = _layer(c)
    ids, sc, pl = got["ids"], got["scores"], got["place"]
    rows = np.arange(c.U)[:, None]
    took = pl >= 0
    need(bool(((pl >= -1) & (pl < c.M)).all()), layer, "a place outside [-1, M)")
    safe = np.where(took, pl, 0)
    same_bits(layer, "ids of the places taken", ids, np.where(took, I.pool_ids[rows, safe], 0).astype(i32))
    same_bits(layer, "scores of the places taken", sc, np.where(took, I.pool_scores[rows, safe], f32(-INF)).astype(f32))
    ref_ids, ref_sc, ref_pl, margins = mmr_ref(c, I)
    w = {}
    if c.kind != "gauss":
        same_bits(layer, "places", pl, ref_pl)
        return w
    decided, worst = np.zeros(c.U, bool), 0.0
    for u in range(c.U):
        tol = mmr_tol(c, I, u)
        slack = mmr_replay(c, I, u, pl[u])
        need(slack <= tol, layer, "user {}: a step took a place {:.3g} below the best candidate, tol {:.3g}", u, slack, tol)
        worst = max(worst, slack / tol)
        decided[u] = bool((margins[u] >= tol).all())
        need(not decided[u] or bool((pl[u] == ref_pl[u]).all()), layer, "user {}: the row differs from the reference although every margin reaches tol", u)
    w["ratio"], w["decided"], w["decided_rows"] = worst, float(decided.mean()), decided
    return w


def _layout(entry, c, I, dev, call, out):
    for variant in ("dense", "shift"):
        other = execute(entry, c, I, dev, call, variant, twice=False)
        for k in out:
            same_bits("layout", f"{entry} {k} with {variant} buffers", other[k], out[k])


def _one_user(c, I, u, prior):
    """The plain case and inputs of user u alone with the given prior [V]: the right side of the header's sampled-row statement."""
    c1 = c._replace(U=1, sample=0, opt="", E=c.E, pool=1 if I.stamp is not None else 2)
    I1 = SimpleNamespace(**vars(I))
    I1.user, I1.prior, I1.best, I1.tau_u, I1.keys = I.user[u:u + 1], prior, I.best[u:u + 1], None, None
    if I.window is not None:
        I1.window = I.window[u:u + 1]
    if I.exclude is not None:
        I1.exclude = I.exclude[u:u + 1]
    if I.segs is not None:
        seg = I.segs[u] if len(I.segs[u]) else np.array([0], i32)
        I1.offsets, I1.xids, I1.segs = np.array([0, len(seg)], i32), seg, [seg]
    return c1, I1


def tk_agree(c, I, out, g32, dev, call):
    """The bit-for-bit statements of the header that tie the calls together (module docstring, `agree`)."""
    ids, sc = out["ids"], out["scores"]
    if c.sample == 1:                                                       # tau = 0 is nr_score_topk
        c0 = c._replace(sample=0, opt="")
        plain = execute("topk", c0, I, dev, call, twice=False)
        same_bits("agree", "ids at tau = 0 against nr_score_topk", ids, plain["ids"])
        same_bits("agree", "scores at tau = 0 against nr_score_topk", sc, plain["scores"])
    elif c.sample == 2:                                                     # row u = the plain call of user u alone with prior P(u, .)
        tau, bad = taus(c, I)
        for u in sorted(set(np.linspace(0, c.U - 1, 8).astype(int).tolist())):
            if bad[u]:
                need(bool((ids[u] == 0).all() and np.isneginf(sc[u]).all()), "agree", "user {}: an invalid temperature must give an all-fill row", u)
                continue
            P = ((I.prior if I.prior is not None else np.zeros(c.V, f32)) + tau[u] * g32[u]).astype(f32)
            c1, I1 = _one_user(c, I, u, P)
            one = execute("topk", c1, I1, dev, call, twice=False)
            same_bits("agree", f"ids of sampled row {u} against the plain call with the perturbed prior", ids[u:u + 1], one["ids"])
            same_bits("agree", f"scores of sampled row {u} against the plain call with the perturbed prior", sc[u:u + 1], one["scores"])
    else:                                                                   # rank <= k exactly when the target is at place rank - 1
        T = min(c.k, 4 if c.cap else 64)
        rng = _rng(9, c.N, c.U, c.V, c.k)
        tg = rng.integers(1, c.V, (c.U, T)).astype(i32)
        cols = np.unique(np.linspace(0, c.k - 1, max(T // 2, 1)).astype(np.int64))
        tg[:, :len(cols)] = ids[:, cols]
        cr = RkCase(c.name, c.kind, c.N, c.U, c.V, T, c.splits, c.E, c.csr, c.pool, c.cap, c.G, c.ung, 0, False, c.pad)
        Ir = SimpleNamespace(**vars(I))
        Ir.targets, Ir.ks = tg, ()
        rk = execute("rank", cr, Ir, dev, call, twice=False)
        for u in range(c.U):
            row = {int(v): p for p, v in enumerate(ids[u]) if v != 0}
            for j, t in enumerate(tg[u].tolist()):
                rank = int(rk["ranks"][u, j])
                if t in row and not (tg[u, :j] == t).any():
                    need(rank == row[t] + 1 and bits32(rk["scores"][u, j:j + 1])[0] == bits32(sc[u, row[t]:row[t] + 1])[0], "agree",
                         "user {}: news {} is at place {} of the row with score {!r}, nr_score_rank says rank {} score {!r}", u, t, row[t], sc[u, row[t]], rank, rk["scores"][u, j])
                else:
                    need(not 1 <= rank <= c.k, "agree", "user {}: news {} has rank {} <= k = {} and is not in the row", u, t, rank, c.k)


def tk_sweep(c, dev, call, layout=True):
    """The driver both files share: every layer of one top-k or sampled case."""
    I = corpus_inputs(c)
    entry = "sample" if c.sample else "topk"
    out = execute(entry, c, I, dev, call)
    g32 = probe(c, I, dev, call) if c.sample == 2 else None
    w = tk_check(c, I, out, g32)
    if layout:
        _layout(entry, c, I, dev, call, out)
    if c.kind == "gauss":
        tk_agree(c, I, out, g32, dev, call)
    return w


def rk_sweep(c, dev, call, layout=True):
    I = corpus_inputs(c)
    out = execute("rank", c, I, dev, call)
    w = rk_check(c, I, out)
    if layout:
        _layout("rank", c, I, dev, call, out)
    return w


def mm_sweep(c, dev, call, layout=True):
    I = mmr_inputs(c)
    out = execute("mmr", c, I, dev, call)
    w = mm_check(c, I, out)
    if layout:
        _layout("mmr", c, I, dev, call, out)
    return w


NOISE_CASES = ((0, 0, 1), (0x5EED00012345678, 7, 257), (2 ** 64 - 1, 2 ** 32 - 1, 1000))


def noise_sweep(seed, draw, n, dev, call):
    """n pairs with keys and ids over the whole 32-bit range, ids of one Philox block side by side, and the two ends of u."""
    rng = _rng(5, n)
    keys = rng.integers(-2 ** 31, 2 ** 31, n).astype(i32)
    ids = rng.integers(0, 2 ** 31, n).astype(i32)
    ids[:min(n, 8)] = np.arange(min(n, 8))
    keys[:min(n, 8)] = keys[0]
    P, P2 = noise_problem(seed, draw, keys, ids, dev), noise_problem(seed, draw, keys, ids, dev)
    call(P)
    call(P2)
    for name, b in all_bufs(P):
        _as("sentinel", _sentinels, f"noise {name}", b)
    out = results(P)
    same_bits("repeat", "g of two runs", out["g"], results(P2)["g"])
    return noise_check(seed, draw, keys, ids, out["g"][0], out["bits"][0])


H = sys.modules[__name__]          # the tests below (and the host file) address the part above as H


# ------------------------------------------------------------------------------------------ the GPU tests
def _L():
    return _lib.lib()


def _p(P, name):
    b = P.inb.get(name) or P.outb.get(name)
    return b.ptr if b is not None else None


def _topk_desc(P):
    c, I, S = P.c, P.I, P.S
    return _lib.TopkDesc(news_vecs=_p(P, "news"), ld_news=S.news, V=c.V, user=_p(P, "user"), ld_user=S.user, U=c.U, N=c.N, k=c.k, exclude=_p(P, "exclude"),
                         ld_exclude=S.excl if c.E else 0, E=c.E, excl_offsets=_p(P, "offsets"), excl_ids=_p(P, "xids"), n_excl=len(I.xids) if I.xids is not None else 0,
                         splits=c.splits, group=_p(P, "group"), group_cap=c.cap, out_ids=_p(P, "ids"), out_scores=_p(P, "scores"), ws=P.ws.ptr, ws_bytes=P.ws_bytes,
                         prior=_p(P, "prior"), stamp=_p(P, "stamp"), window=_p(P, "window"), ld_window=S.win if I.stamp is not None else 0)


def _call(P):
    """One call of the C ABI on the buffers of P; the size query must answer the restated carve."""
    L, s = _L(), ops._stream()
    if P.entry == "noise":
        rc = L.nr_sample_noise(P.seed, P.draw, _p(P, "keys"), _p(P, "ids"), P.n, _p(P, "g"), _p(P, "bits"), s)
    elif P.entry == "topk":
        d = _topk_desc(P)
        assert L.nr_score_topk_workspace_bytes(C.byref(d)) == P.ws_bytes, (_lib.last_error(), P.ws_bytes)
        rc = L.nr_score_topk(C.byref(d), s)
    elif P.entry == "sample":
        I = P.I
        d = _lib.SampleDesc(topk=_topk_desc(P), seed=I.seed, draw=I.draw, tau=I.tau, tau_u=_p(P, "tau_u"), user_keys=_p(P, "keys"), out_model=_p(P, "model"))
        assert L.nr_score_sample_workspace_bytes(C.byref(d)) == P.ws_bytes, (_lib.last_error(), P.ws_bytes)
        rc = L.nr_score_sample(C.byref(d), s)
    elif P.entry == "rank":
        c, I, S = P.c, P.I, P.S
        d = _lib.RankDesc(news_vecs=_p(P, "news"), ld_news=S.news, V=c.V, user=_p(P, "user"), ld_user=S.user, U=c.U, N=c.N, T=c.T, targets=_p(P, "targets"),
                          ld_targets=S.tgt, exclude=_p(P, "exclude"), ld_exclude=S.excl if c.E else 0, E=c.E, excl_offsets=_p(P, "offsets"), excl_ids=_p(P, "xids"),
                          n_excl=len(I.xids) if I.xids is not None else 0, splits=c.splits, ks=(C.c_int * max(len(I.ks), 1))(*I.ks), n_ks=len(I.ks),
                          out_ranks=_p(P, "ranks"), out_scores=_p(P, "scores"), out_sums=_p(P, "sums"), group=_p(P, "group"), group_cap=c.cap,
                          n_groups=c.G if c.cap else 0, ws=P.ws.ptr, ws_bytes=P.ws_bytes, prior=_p(P, "prior"), stamp=_p(P, "stamp"), window=_p(P, "window"),
                          ld_window=S.win if I.stamp is not None else 0)
        assert L.nr_score_rank_workspace_bytes(C.byref(d)) == P.ws_bytes, (_lib.last_error(), P.ws_bytes)
        rc = L.nr_score_rank(C.byref(d), s)
    else:
        c, I, S = P.c, P.I, P.S
        d = _lib.MmrDesc(news_vecs=_p(P, "news"), ld_news=S.news, V=c.V, pool_ids=_p(P, "pool_ids"), pool_scores=_p(P, "pool_scores"), ld_pool_ids=S.pid,
                         ld_pool_scores=S.psc, U=c.U, N=c.N, M=c.M, k=c.k, penalty=I.penalty, penalty_u=_p(P, "penalty_u"), group=_p(P, "group"), group_cap=c.cap,
                         out_ids=_p(P, "ids"), out_scores=_p(P, "scores"), out_place=_p(P, "place"))
        rc = L.nr_mmr_select(C.byref(d), s)
    _lib.check(rc, "nr_" + P.entry)
    torch.cuda.synchronize()


def _labelled(fn):
    """fn() and the profiler labels of what it launched (as test_gpu_corpus_dispatch.py reads them)."""
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        out = fn()
        torch.cuda.synchronize()
        return out, set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)


def _report(tag, c, w):
    print(f"\nCORPUS {tag} {c.name} " + " ".join(f"{k}={v:.4f}" for k, v in w.items() if not isinstance(v, np.ndarray)))


@pytest.mark.parametrize("c", H.topk_cases(), ids=lambda c: c.name)
def test_topk_and_sample(c):
    w, labels = _labelled(lambda: H.tk_sweep(c, DEV, _call))
    TU, splits = H.tk_plan(c)
    assert f"topk_select[U={c.U},V={c.V},N={c.N},k={c.k},TU={TU},splits={splits}]" in labels, labels
    assert any(l.startswith("sample_model[") for l in labels) == ("m" in c.opt), labels
    _report("topk", c, w)


@pytest.mark.parametrize("c", H.rank_cases(), ids=lambda c: c.name)
def test_rank(c):
    w, labels = _labelled(lambda: H.rk_sweep(c, DEV, _call))
    TU, splits = H.rk_plan(c)[:2]
    assert f"rank_count[U={c.U},V={c.V},N={c.N},T={c.T},TU={TU},splits={splits}]" in labels, labels
    assert any(l.startswith("rank_named_csr[" if c.csr else "rank_named[") for l in labels), labels
    assert any(l.startswith("rank_group_masks[") for l in labels) == bool(c.cap), labels
    _report("rank", c, w)


@pytest.mark.parametrize("c", H.mmr_cases(), ids=lambda c: c.name)
def test_mmr(c):
    w, labels = _labelled(lambda: H.mm_sweep(c, DEV, _call))
    assert f"mmr_select[U={c.U},N={c.N},M={c.M},k={c.k}]" in labels, labels
    _report("mmr", c, w)


@pytest.mark.parametrize("seed,draw,n", H.NOISE_CASES)
def test_sample_noise(seed, draw, n):
    print(f"\nCORPUS noise n={n} ratio={H.noise_sweep(seed, draw, n, DEV, _call):.4f}")

"""GPU: every route of the capped-row calls through the C ABI: nr_score_logz_groups (K15), nr_score_expect_groups (K20) and
nr_score_expect_news_groups (K22) with their three size queries, and the row pair nr_row_logprob_capped (K16) and
nr_row_logprob_capped_grad (K21) (include/nrhip.h; csrc/nr_logz_groups.hip, nr_expect_groups.hip, nr_expect_news_groups.hip).
Built like tests/test_gpu_softmax_sweep.py, whose helpers it imports.  The case tables, one route function per entry point (its
dispatch restated), the input builders, the float64 references, the descriptors' buffers and the checker are the first part of
this file ("capped sweep"; plain numpy and torch, no GPU needed); tests/test_capped_sweep_host.py imports them and proves on the
CPU that the checker passes a sound stand-in and fails each of its mutants at the layer named.  The second part calls the C ABI
with the ctypes descriptors of _lib.py.  A stream case runs the chain: K15 first, then K20 on the bases it returned, then K22 on
their transposes.

Tables.  group_tables restates ops.GroupOrder in numpy (the host file asserts that the two agree on every case), so the sweep
owns order, pos, bin_start, seg_start and bin_seg: bins of 0, 1, 127, 128 and 129 news, runs of empty bins that include bin 0
and bin n_groups, n_groups = 1 .. 512, and a corpus of more than 256 chunks (two chunks a segment, S = 2) in which a slice comes
out empty.  With opt "x" the padding places of a run hold ids outside [1, V) (the header: rows of zeros, never eligible) in
place of 0; nothing else ill-formed is handed to the device.

Buffers.  Every device array, inputs and the tables included, is one allocation [guard][payload][guard] (glue_buf).  Vector
bases and `out` are 16-byte aligned and no more, int32 arrays, per-user fp32 arrays and the [U, ld_base] and [n_groups + 1,
ld_bin] arrays 4-byte aligned, the workspace 8-byte aligned, exactly as long as the size query answered -- which must equal the
restated carve and plan (`wsize`) -- and NaN before every call: row 0 of K22, a K20 slice without a segment and K15's empty bins
show themselves if a partial is read that nothing wrote.  Outputs start as NaN (integers: -77).  Padded strides in every case:
ld_news, ld_user two different ones of {N, N + 4, tk_npad(N) + 8}, ld_out in {N, N + 4}, ld_base in {n_groups + 1, n_groups + 4},
ld_bin in {U, U + 3}, ld_ids in {k, k + 1}, ld_g in {k, k + 5}, ld_sub in {T, T + 3}, ld_window in {2, 5}.  The slack is poison:
NaN in vector, base and `out` slack, 1e30 in bin_w, g and sub_w slack, a valid id in row_ids / sub_ids slack, an empty window;
news row 0 holds 3e37.  `sentinel`: every guard and slack element compares bit for bit after the call -- columns n_groups + 1 ..
ld_base - 1 of out_bin_w and N .. ld_out - 1 of `out` are never written.  `repeat`: two problems built alike give the same bits.
`layout`: the widths as strides, and every base moved (16 / 8 / 4 bytes), give the same bits.

Data kinds.
  plateau  (K15, K20, K22) integer news in [-2, 2], users 128 r_g with r_g a row of +-2, priors multiples of 128 (<= 0),
           temperatures from {1/4, 1/2, 1}: every score is a multiple of 128 and exact, so every (s - gmax_b) / tau is 0 or <= -128
           (the host file asserts it) and every fp32 exponential is exactly 1 or exactly 0.  m_b copies of r_g are planted per bin
           (m_b from {1, 2, 3, 64, 129} as the bin allows), spread by a permutation; lists, windows and -inf priors take some
           away, in every CSR case user 2 lists all planted news of one bin; the multiplicity m_ub comes from the reference.
           omega, sub_w and named_w are powers of two or 0.  `exact`: out_max and out_count equal the reference bit for bit;
           out_logsum is +0.0 for m = 1, else float32(log m) or its neighbour; a K20 row whose weighted bins all have m = 1 is the
           fp64 lattice value rounded once and its mass the exact sum of omega; a K22 row whose contributors all have m = 1 (or
           that has none: nobody's maximum, row 0) is the exact value rounded once.  `tight` for m > 1: DESIGN.md "Capped calls:
           routes as verified and the sweep" -- p = (1 + t) / m, |t| <= (6 + 3 ln m) e; K20 (M + 3 ln m + 7) e A_c with M the
           nonzero terms of the user's fullest slice over ALL its weighted bins, K22 (n_v + 3 ln m + 7) e A_vc.
  gauss    Gaussian vectors, flat, ordinary and peaked users in one call, against float64 on the fp32 inputs under the bounds of
           include/nrhip.h as tests/test_gpu_logz_groups.py (lzg_bound), test_gpu_capgrad.py (kappa20, kappa21) and
           test_gpu_capgrad_news.py (kappa22, its _reference) state them, imported -- `bound`.  With per-user temperatures users 1,
           3, 4, 6 have tau_u = 0, -1, NaN, +inf: NaN logsums in their non-empty bins (max and count valid), a NaN row and mass in
           K20, dead users in K22 whose named terms are not subtracted; user 7 has the smallest normal temperature (1 / tau
           stays finite: the weights of the limit); news 5 is a NaN row; with U >= 12 users 9, 10, 11 have, in a weighted non-empty
           bin, a NaN logsum, an infinite omega and a maximum of +inf in the bases handed to K20 / K22: a NaN row and mass in K20
           for that user alone, a dead pair in K22 -- `special`; every
           fourth user has omega = 0 in one bin over a NaN base, which must contribute exactly nothing.
           News 6 has one infinite component (a NaN score for everyone, 0 in E); where the corpus has a bin of one news and
           U >= 13, that news scores -inf for everyone (max -inf, count 1, logsum NaN; an empty bin to K20 / K22) and +inf for user 12.
           `agree`, bit for bit: K15 at splits = 0, 1, 2, nseg; max_b out_max = K13's out_max and sum_b out_count = K13's count;
           K20 row u at one explicit `splits` when every other user is replaced and when U changes; K22 row v when every other news
           is replaced, and when v's place in its run moves and other bins change size; K22 with one bin holding every news against
           K18 at padded strides (a test of its own).
  lattice  (K16, K21) integer vectors and quarter-grid priors make every gathered score exact; the bases are host-made fp32
           values, every fourth user has empty bins (-inf, -inf).  Everything after the gather is fp64 rounded once: the bound
           is e |value*| + ROW_F64 times the absolute sums of each formula (the reference run with |g|).  Joins a value passes
           through: at most 9 per-lane bins + 6 butterfly steps + 128 walk steps + 128 stashed entries + 7 scan steps = 278, each
           two exponentials, two products and a sum, about 6 units of 2^-53, the reference's own logaddexp as many again: under
           2^12 units, ROW_F64 = 2^-41.  `exact`: fill entries are 0; -inf and NaN sit where the reference has them and K21 never
           answers NaN; out_total is -inf beside a blocked entry; a row that takes everything eligible ends in logp == 0; bins
           0 .. n_groups of out_bin_w are all written, 0 for empty bins.

Layers of CappedCheckError: sentinel, repeat, layout, wsize, exact, tight, bound, agree, special.
"""
import collections
import ctypes as C
import math
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_capgrad as GC
import test_gpu_capgrad_news as GN
import test_gpu_corpus_sweep as CS
import test_gpu_glue_sweep as GL
import test_gpu_logz_groups as LG
import test_gpu_softmax_sweep as SW
from test_gpu_corpus_sweep import auto_splits, tk_npad, user_tile
from test_gpu_glue_sweep import _bits, _count_routes, _sentinels, glue_buf
from test_gpu_softmax_sweep import lz_plan_tile
from newsrecommendation_amd import _lib, metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------ capped sweep
EPS = 2.0 ** -24
# What the device adds beyond a bound of include/nrhip.h, as a fraction of it; 0 when there is no excess.
CAPPED_EXCESS = 0.0
ROW_F64 = 2.0 ** -41
LAYERS = ("sentinel", "repeat", "layout", "wsize", "exact", "tight", "bound", "agree", "special")
STREAM = ("logzg", "expectg", "newsg")
NAN, INF = float("nan"), float("inf")
IFILL = -77
f32, f64, i32 = np.float32, np.float64, np.int32
_rng = CS._rng
in_buf, out_buf = CS.in_buf, SW.out_buf


class CappedCheckError(AssertionError):
    """A failed check of the sweep; `.layer` is one of LAYERS."""

    def __init__(self, layer, msg):
        assert layer in LAYERS, layer
        super().__init__(f"[{layer}] {msg}")
        self.layer = layer


def need(ok, layer, msg, *a):
    if not ok:
        raise CappedCheckError(layer, msg.format(*a) if a else msg)


def same_bits(layer, name, got, ref):
    try:
        CS.same_bits("exact", name, got, ref)
    except CS.CorpusCheckError as e:
        raise CappedCheckError(layer, str(e)) from None


def _sent(name, b):
    try:
        _sentinels(name, b)
    except GL.GlueCheckError as e:
        raise CappedCheckError("sentinel", str(e)) from None


def _ratio(layer, name, got, ref, bound, rows):
    try:
        return SW._ratio("bound", name, got, ref, bound, rows)
    except SW.SoftmaxCheckError as e:
        raise CappedCheckError(layer, str(e).replace("[bound] ", "", 1)) from None


# ---------------------------------------------------------------------------------------- 0 the tables and the plans, restated
def group_tables(group, G, odd_padding=False):
    """ops.GroupOrder in numpy: news 1 .. V-1 sorted by (bin, id), every bin's run padded to a multiple of 128 positions; S =
    ceil(chunks / 256) chunks a segment at most, a segment never straddles two bins.  odd_padding: the padding places hold ids
    outside [1, V) instead of 0."""
    group = np.asarray(group, np.int64)
    V = len(group)
    bins = np.where(group < 0, G, group)
    assert bins[1:].max(initial=0) <= G
    cnt = np.bincount(bins[1:], minlength=G + 1)
    bin_start = np.concatenate([[0], np.cumsum((cnt + 127) // 128 * 128)]).astype(np.int64)
    n_pos = int(bin_start[-1])
    S = max(1, (n_pos // 128 + 255) // 256)
    seg_start, bin_seg = [], [0]
    for b in range(G + 1):
        seg_start.extend(range(int(bin_start[b]), int(bin_start[b + 1]), S * 128))
        bin_seg.append(len(seg_start))
    seg_start.append(n_pos)
    order, pos = np.zeros(n_pos, i32), np.full(V, -1, i32)
    if odd_padding:
        order[:] = np.where(np.arange(n_pos) % 2, V + 2, -3)
    for b in np.flatnonzero(cnt):
        ids = 1 + np.flatnonzero(bins[1:] == b)
        order[bin_start[b]:bin_start[b] + len(ids)] = ids
        pos[ids] = bin_start[b] + np.arange(len(ids))
    return SimpleNamespace(V=V, G=G, n_pos=n_pos, S=S, nseg=len(seg_start) - 1, order=order, pos=pos, bins=bins, cnt=cnt, bin_start=bin_start.astype(i32),
                           seg_start=np.array(seg_start, i32), bin_seg=np.array(bin_seg, i32))


def slices(T, splits):
    """The segments [s_lo, s_hi) of every slice: slice y of s takes the segments that START in [y n_pos / s, (y + 1) n_pos / s);
    with as many slices as segments slice y is segment y.  A slice may come out empty."""
    if splits == T.nseg:
        return [(y, y + 1) for y in range(splits)]
    first = lambda p: int(np.searchsorted(T.seg_start[:T.nseg], p, side="left"))
    return [(first(y * T.n_pos // splits), T.nseg if y + 1 == splits else first((y + 1) * T.n_pos // splits)) for y in range(splits)]


def stream_tile(N):
    """K15: score_user_tile(N, 0) -- 64 users up to N = 480, 32 up to 960, else 16."""
    return user_tile(N, 0)


def contract_tile(N):
    """K20 (users) and K22 (news): score_user_tile(N, a row of P) -- 64 up to N = 352, 32 up to 832, else 16."""
    return user_tile(N, SW.EX_PER_USER)


KMAX = SW.KMAX


def plan(entry, c, T):
    """lg_plan / eg_plan: (TU, slices) over the caller's segments; eng_plan: K18's plan of the user axis."""
    if entry == "newsg":
        return lz_plan_tile(T.V, c.U + 1, contract_tile(c.N), c.vs)
    TU = stream_tile(c.N) if entry == "logzg" else contract_tile(c.N)
    s = c.splits if c.splits > 0 else auto_splits(c.U, T.V, TU, T.nseg)
    return SimpleNamespace(TU=TU, splits=max(1, min(s, T.nseg)))


def ws_bytes(entry, c, T):
    """lg_carve: U * nseg * 12; eg_carve: U * slices * (4 N + 8); eng_carve: V * slices * (4 N + 8); each rounded to 8."""
    p = plan(entry, c, T)
    n = c.U * T.nseg * 12 if entry == "logzg" else (c.U if entry == "expectg" else T.V) * p.splits * (4 * c.N + 8)
    return (n + 7) // 8 * 8


# ---------------------------------------------------------------------------------------- 1 the stream cases and their routes
# sizes: a key of SIZES -- the news of bins 0 .. n_groups (the last one: no group).  splits: of K15 / K20, 0 = the library's,
# -1 = nseg, -2 = nseg - 1 (the first_from path next to the `one` path); vs: K22's slices of the user axis.  pool: 0 none, 1 prior
# + stamps and windows, 2 prior only, 3 stamps and windows only.  csr: 0 no lists, 1 segments of 0, 1, 64, 65, 129, 300 entries,
# 2 the same with users 0 and 1 hand-made, 3 lists made BY NEWS for K22's probe (_lists).  T: named rows per user of K20; named: K22's named terms.  opt: s =
# scale_inv_tau, M = the masses given, x = odd padding ids.
CapCase = collections.namedtuple("CapCase", "name kind N U sizes splits vs pool csr taus T named opt pad")
SIZES = {
    "a": [128, 1, 0, 129, 37],                                     # a bin of exactly 128, one of 1, an empty one, 129, 37 in no group
    "rows": [0, 0, 127, 0, 0, 129, 0],                             # empty bins in a row, bin 0 and "no group" among them
    "one": [200, 60],
    "two": [1, 300, 0],
    "g3": [100, 0, 129, 20],
    "tv": [1, 63, 64, 65, 127, 128, 129, 15, 16, 17, 31, 32, 33, 5],      # around every news tile of K22
    "g64": [i % 5 for i in range(64)] + [3],
    "g511": [int(i % 3 == 1) for i in range(511)] + [2],
    "g512": [int(i % 3 == 0) for i in range(512)] + [0],
    "empty_slice": [1] * 295 + [200] * 5 + [130],                  # 307 chunks: S = 2, segments of one and of two chunks
    "tiny": [6, 4],
}
CAP_NS = (4, 28, 32, 36, 352, 356, 832, 836, 1020, 1024)
REFUSED_NS = {353: 356, 833: 836}
CAP_TS = SW.SM_TS
CAP_MS = SW.SM_MS
CSR_LENGTHS = CS.CSR_LENGTHS
OPTS = ("sM", "", "M", "sx", "Mx", "s")
SPECIAL_TAUS = {"tau0": 0.0, "tauneg": -1.0, "taunan": NAN, "tauinf": INF, "tautiny": float(np.finfo(np.float32).tiny)}
U_TWO = 128 * 256 + 6                                               # user segments of two chunks (K22)

_STREAM = tuple(f"tile_{t}" for t in (64, 32, 16)) + tuple(f"p{p}l{l}" for p in (0, 1) for l in (0, 1)) + (
    "splits_auto", "splits_one", "splits_given", "splits_nseg", "empty_slice", "slice_spans_bins", "bin_spans_slices", "two_chunk_segments", "empty_bins_in_a_row",
    "tau_scalar", "tau_u", "finalize_below_256", "finalize_from_256")
LOGZG_ROUTES = _STREAM
EXPECTG_ROUTES = _STREAM[:-2] + tuple(f"kmax_{k}" for k in (11, 26, 32)) + ("sub_null", "sub_given", "scale_0", "scale_1", "mass_null", "mass_given")
NEWSG_ROUTES = tuple(f"tile_{t}" for t in (64, 32, 16)) + tuple(f"kmax_{k}" for k in (11, 26, 32)) + tuple(f"p{p}l{l}" for p in (0, 1) for l in (0, 1)) + (
    "splits_auto", "splits_given", "short_last_slice", "two_chunk_segments", "padding_only_tiles", "empty_bins_before", "tau_scalar", "tau_u", "named_null",
    "named_given", "scale_0", "scale_1", "mass_null", "mass_given")
ROUTES = {"logzg": LOGZG_ROUTES, "expectg": EXPECTG_ROUTES, "newsg": NEWSG_ROUTES}


def _u_of(tile, j):
    return (1, tile - 1, tile, tile + 1)[j % 4]


def cap_cases():
    cs, i = [], 0
    for kind in ("plateau", "gauss"):
        for N in CAP_NS:                                                      # every width, U around the tile of either kernel
            tile = contract_tile(N) if i % 2 else stream_tile(N)
            cs.append(CapCase(f"{kind}-N{N}", kind, N, min(_u_of(tile, i + i // 4), 65), "a" if i % 3 else "g3", (0, 1, 2, -1, -2)[i % 5], (0, 1)[i % 2], i % 4, (i // 2) % 2,
                              i % 2, (0, CAP_TS[i % 6])[(i // 3) % 2], (i // 2) % 2, OPTS[i % 6], i % 3))
            i += 1
    for j, (tile, N) in enumerate(((64, 36), (32, 832), (16, 1024), (64, 352))):     # U = 1, TU - 1, TU, TU + 1 of every tile
        for jj in range(4):
            q = 4 * j + jj
            kind = ("plateau", "gauss")[q % 2]
            cs.append(CapCase(f"{kind}-tile{tile}-N{N}-u{_u_of(tile, jj)}", kind, N, _u_of(tile, jj), ("a", "rows", "g3")[q % 3], (2, 0, -1, 1)[q % 4], 0, (3, 0, 2, 1)[q % 4],
                              q % 2, (q + 1) % 2, (0, CAP_TS[(q + 2) % 6])[q % 2], (q + 1) % 2, OPTS[(q + 3) % 6], q % 3))
    for kind in ("plateau", "gauss"):
        g = kind == "gauss"
        cs += [CapCase(f"{kind}-empty-slice", kind, 4, 5, "empty_slice", -2, 0, 1, 1, 1, 65, 1, "sM", 1),        # a slice in which no segment starts
               CapCase(f"{kind}-empty-slice-nseg", kind, 4, 3, "empty_slice", -1, 0, 0, 0, 0, 0, 0, "Mx", 2),
               CapCase(f"{kind}-empty-slice-auto", kind, 36, 2, "empty_slice", 0, 0, 2, 0, 1, 1, 1, "M", 0),
               CapCase(f"{kind}-seek", kind, 36, 5, "one", 2, 0, 0, 2, 0, 1, 1, "M", 1),                           # 128 and 65 positions listed in a chunk; the search
               CapCase(f"{kind}-seek-pool", kind, 32, 17, "two", 2, 0, 1, 2, 1, 64, 0, "s", 2),
               CapCase(f"{kind}-one-group", kind, 36, 9, "one", 3, 0, 2, 1, 1, 0, 1, "M", 0),
               CapCase(f"{kind}-two-groups", kind, 4, 130, "two", -2, 2, 3, 0, 0, 127, 0, "sM", 1),
               CapCase(f"{kind}-g3-u64", kind, 4, 64, "g3", 1, 0, 0, 0, 1, 0, 1, "", 2),                         # U * bins = 256 exactly
               CapCase(f"{kind}-g64", kind, 36, 3, "g64", -2, 0, 1, 1, 1, 63, 1, "sMx", 0),                     # 195 (user, bin) pairs
               CapCase(f"{kind}-g64-u4", kind, 4, 4, "g64", 0, 0, 0, 0, 0, 0, 0, "M", 1),                       # 260
               CapCase(f"{kind}-g511", kind, 4, 2, "g511", -1, 0, 3, 0, 1, 128, 1, "M", 2),
               CapCase(f"{kind}-g512", kind, 36, 3, "g512", 2, 0, 2, 1, 0, 0, 0, "sx", 0),
               CapCase(f"{kind}-rows", kind, 28, 7, "rows", -2, 0, 0, 1, 1, 1, 1, "M", 1),
               CapCase(f"{kind}-tv-u2", kind, 36, 2, "tv", 1, 0, 1, 1, 0, 0, 1, "Mx", 2),                       # K22: bins around the news tile
               CapCase(f"{kind}-tv-u129", kind, 4, 129, "tv", 0, 2, 0, 0, 1, 0, 0, "s", 0),
               CapCase(f"{kind}-tv32-u3", kind, 832, 3, "tv", 2, 0, 2, 0, 0, 0, 1, "M", 1),
               CapCase(f"{kind}-tv16-u130", kind, 836, 65, "tv", 0, 0, 0, 0, 1, 0, 0, "sM", 2),
               CapCase(f"{kind}-u257", kind, 4, 257, "a", 1, 2, 3, 3, 1, 0, 1, "M", 0),                         # K22: three user segments, a short last slice
               CapCase(f"{kind}-u130-lists", kind, 36, 130, "two", 2, 0, 1, 3, 0, 0, 1, "sM", 1)]
        cs.append(CapCase(f"{kind}-two-user-chunks", kind, 4, U_TWO, "tiny", 1, (0, 8)[g], 0, 3, 1, 0, g, "M", g))
    assert len({c.name for c in cs}) == len(cs)
    return cs


def tables(c):
    sz = SIZES[c.sizes]
    G, V = len(sz) - 1, 1 + sum(sz)
    perm = 1 + _rng(3, V, G).permutation(V - 1)                               # groups are not runs of ids: the order is a real gather
    group = np.full(V, -1, i32)
    at = 0
    for b, n in enumerate(sz):
        group[perm[at:at + n]] = b if b < G else -1
        at += n
    T = group_tables(group, G, "x" in c.opt)
    T.group = group
    return T


def resolve(c, T):
    """The case with `splits` as the number the descriptor carries."""
    s = {-1: T.nseg, -2: max(1, T.nseg - 1)}.get(c.splits, min(c.splits, T.nseg))
    return c._replace(splits=s, vs=min(c.vs, lz_plan_tile(T.V, c.U + 1, 64, 1).nseg))


def _stream_route(entry, c, T):
    p = plan(entry, c, T)
    sl = slices(T, p.splits)
    r = [f"tile_{p.TU}", f"p{int(bool(c.pool))}l{int(bool(c.csr))}", "tau_u" if c.taus else "tau_scalar",
         "splits_auto" if not c.splits else "splits_nseg" if p.splits == T.nseg else "splits_one" if p.splits == 1 else "splits_given"]
    if any(lo >= hi for lo, hi in sl):
        r.append("empty_slice")
    bin_of = np.searchsorted(T.bin_seg[1:], np.arange(T.nseg), side="right")
    if any(hi > lo and bin_of[lo] != bin_of[hi - 1] for lo, hi in sl):
        r.append("slice_spans_bins")
    if any(len({y for y, (lo, hi) in enumerate(sl) if lo < T.bin_seg[b + 1] and hi > T.bin_seg[b]}) > 1 for b in range(T.G + 1)):
        r.append("bin_spans_slices")
    if T.S > 1:
        r.append("two_chunk_segments")
    if any(T.cnt[b] == 0 and T.cnt[b + 1] == 0 for b in range(T.G)) and T.cnt[0] == 0 and T.cnt[T.G] == 0:
        r.append("empty_bins_in_a_row")
    return r


def logzg_route(c, T):
    """nr_score_logz_groups: logzg_stream_kernel<MT, POOL, LISTS> on the tile of score_user_tile(N, 0), slices by positions
    (`one`: as many slices as segments; else first_from), then logzg_final_kernel, one thread per (user, bin)."""
    return tuple(_stream_route("logzg", c, T) + ["finalize_below_256" if c.U * (T.G + 1) < 256 else "finalize_from_256"])


def expectg_route(c, T):
    """nr_score_expect_groups: expect_groups_stream_kernel<MT, KMAX, POOL, LISTS> as <4, 11>, <2, 26>, <1, 32>, then its finalize."""
    p = plan("expectg", c, T)
    r = _stream_route("expectg", c, T)
    if tk_npad(c.N) // 32 == KMAX[p.TU]:
        r.append(f"kmax_{KMAX[p.TU]}")
    return tuple(r + ["sub_given" if c.T else "sub_null", "scale_1" if "s" in c.opt else "scale_0", "mass_given" if "M" in c.opt else "mass_null"])


def newsg_route(c, T):
    """nr_score_expect_news_groups: expect_news_groups_stream_kernel<MT, KMAX, POOL, LISTS> over position tiles x user slices."""
    p = plan("newsg", c, T)
    r = [f"tile_{p.TU}", f"p{int(bool(c.pool))}l{int(bool(c.csr))}", "splits_given" if c.vs else "splits_auto", "tau_u" if c.taus else "tau_scalar",
         "named_given" if c.named else "named_null", "scale_1" if "s" in c.opt else "scale_0", "mass_given" if "M" in c.opt else "mass_null"]
    if tk_npad(c.N) // 32 == KMAX[p.TU]:
        r.append(f"kmax_{KMAX[p.TU]}")
    if c.vs and p.nseg % p.segs_per:
        r.append("short_last_slice")
    if p.seg > 128:
        r.append("two_chunk_segments")
    real = ((T.order >= 1) & (T.order < T.V)).reshape(-1, p.TU)
    if (~real.any(axis=1)).any():
        r.append("padding_only_tiles")
    if any(T.cnt[b] == 0 and T.cnt[b + 1] == 0 and T.cnt[b + 2:].any() for b in range(T.G - 1)):
        r.append("empty_bins_before")
    return tuple(r)


ROUTE_FN = {"logzg": logzg_route, "expectg": expectg_route, "newsg": newsg_route}


# ---------------------------------------------------------------------------------------- 2 inputs of the stream cases
def _lists(c, T, rng, must):
    """Per user the ids it lists.  csr = 1: lengths 0, 1, 64, 65, 129, 300 (cut to the corpus), with entries <= 0 and >= V at the
    ends.  csr = 2: user 0 lists every news of the first chunk of the first run of two chunks or more and 65 positions of its second
    chunk (the refill loop); user 1 lists only news of that first chunk (with splits >= 2 all its entries lie before the last
    slice's start: the 64-ary search runs to the end).  must: {user: ids} merged in."""
    V, U = T.V, c.U
    segs = []
    if c.csr == 3:
        # by news, for K22's lists by position: seven news h_0 .. h_6 of the order are listed by the first 0, 1, 64, 65, 129 and 300
        # users (as far as U goes), and h_6 by all 128 users of the first chunk and 65 of the second (the refill loop of the probe)
        real = T.order[(T.order >= 1) & (T.order < V)]
        hand = [int(v) for v in real if v not in (5, 6)][1:8]
        rest = np.setdiff1d(np.arange(-3, V + 3), hand)
        segs = [[v for v in rng.choice(rest, u % 3, replace=False)] for u in range(U)]
        for h, L in zip(hand, CSR_LENGTHS):
            for u in range(min(L, U)):
                segs[u].append(h)
        if U >= 256:
            for u in list(range(128)) + (128 + np.sort(rng.choice(128, 65, replace=False))).tolist():
                segs[u].append(hand[6])
        segs = [np.unique(np.array(x, i32)).astype(i32) for x in segs]
    for u in range(U if c.csr != 3 else 0):
        L = min(CSR_LENGTHS[(u + 1) % 6] if U < 6 else CSR_LENGTHS[u % 6], V - 1)
        segs.append(np.sort(rng.choice(np.arange(-3, V + 3), L, replace=False)).astype(i32))
    if c.csr == 2:
        b = int(np.flatnonzero(T.cnt > 128)[0])
        p0 = int(T.bin_start[b])
        ids = T.order[p0:p0 + 256]
        second = ids[128:][(ids[128:] >= 1) & (ids[128:] < V)]
        segs[0] = np.concatenate([ids[:128], second[:65]]).astype(i32)
        if U >= 2:
            segs[1] = ids[3:128:2].astype(i32)
    for u, ids in must.items():
        segs[u] = np.unique(np.concatenate([segs[u], np.asarray(ids, i32)])).astype(i32)
    return segs


def position_lists(T, segs):
    """K15's lists in position space: (offsets [U + 1] with the last one beyond n_excl, positions), each user's ascending."""
    ps = []
    for s in segs:
        s = np.asarray(s, np.int64)
        ps.append(np.unique(T.pos[s[(s >= 1) & (s < T.V)]]).astype(i32))
    x = np.concatenate(ps + [np.zeros(0, i32)]).astype(i32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in ps])]).astype(i32)
    if x.size == 0:
        x = np.array([T.n_pos + 1], i32)
    off[-1] += 7
    return off, x


def lists_by_position(T, segs, U):
    """K22's lists: (offsets [n_pos + 1], users), per position the ascending indices of the users whose list holds order[p]."""
    per = [[] for _ in range(T.n_pos)]
    for u, s in enumerate(segs):
        s = np.asarray(s, np.int64)
        for p in np.unique(T.pos[s[(s >= 1) & (s < T.V)]]):
            per[p].append(u)
    x = np.array([u for l in per for u in l] + [U + 1], i32)
    off = np.concatenate([[0], np.cumsum([len(l) for l in per])]).astype(i32)
    off[-1] += 7
    return off, x


def _list_arrays(I, T, U, by_position):
    """position_lists / lists_by_position of I.segs over T, kept with I for as long as both stay the same objects."""
    name = "_by_position" if by_position else "_positions"
    kept = getattr(I, name, None)
    if kept is None or kept[0] is not I.segs or kept[1] is not T:
        kept = (I.segs, T, lists_by_position(T, I.segs, U) if by_position else position_lists(T, I.segs))
        setattr(I, name, kept)
    return kept[2]


def cap_inputs(c, T):
    """Everything the three calls of a stream case read, as plain numpy arrays in their logical shapes."""
    rng = _rng(31, c.N, c.U, T.V, T.G, c.splits, c.pool, c.csr, c.taus, c.T, c.named, c.pad, len(c.opt), c.kind == "gauss")
    V, U, N, G = T.V, c.U, c.N, T.G
    plateau = c.kind == "plateau"
    I = SimpleNamespace(prior=None, stamp=None, window=None, segs=None, tau=(0.25, 0.5, 1.0)[(N + U) % 3] if plateau else (0.5, 0.7, 1.3)[(N + U) % 3], tau_u=None,
                        sub_ids=None, sub_w=None, n_off=None, n_user=None, n_w=None, group=T.group, special={})
    must = {}
    if plateau:
        Gp = 3
        pats = []
        while len(pats) < Gp:
            r = rng.choice(np.array([-2, 2]), N)
            if not any((r == q).all() for q in pats) or 2 ** N <= Gp:
                pats.append(r)
        news = rng.integers(-2, 3, (V, N))
        for r in pats:
            news[(news == r).all(axis=1), 0] = 0
        listed = None
        for b in np.flatnonzero(T.cnt):
            ids = rng.permutation(1 + np.flatnonzero(T.bins[1:] == b))          # spread over lanes, chunks and segments
            m = next((x for x in (CAP_MS[(b + j) % 5] for j in range(5)) if x + 6 <= len(ids)), 1)
            at = 0
            for g, mg in enumerate((m, CAP_MS[(b + 1) % 3], CAP_MS[(b + 2) % 3])):      # the copies of r_0; 1, 2 or 3 of r_1 and r_2
                mg = min(mg, len(ids) - at)
                news[ids[at:at + mg]] = pats[g]
                if g == 2 and listed is None and mg > 1:
                    listed = ids[at:at + mg]
                at += mg
        I.news, I.user = news.astype(f32), np.stack([128.0 * pats[u % Gp] for u in range(U)]).astype(f32)
        if c.csr and U >= 3 and listed is not None:
            must[2] = listed                                                  # a user whose maxima of one bin are all listed
    else:
        I.news = rng.standard_normal((V, N)).astype(f32)
        scale = np.array([1e-3, 1.0, 300.0])[np.arange(U) % 3]               # flat, ordinary, peaked
        I.user = (rng.standard_normal((U, N)) * (scale / math.sqrt(N))[:, None]).astype(f32)
    I.news[0] = 3e37
    SW._pools(SimpleNamespace(V=V, U=U, pool=c.pool, kind=c.kind), I, rng, plateau)
    if c.csr:
        I.segs = _lists(c, T, rng, must)
    full_bins = np.flatnonzero(T.cnt)
    zb = int(full_bins[len(full_bins) // 2])                                  # a weight of exactly 0 in a non-empty bin, over a NaN base
    I.inf_bin = None
    if c.taus:
        I.tau_u = (np.array([0.25, 0.5, 1.0], f32) if plateau else np.array([0.3, 1.7, 0.75], f32))[rng.integers(0, 3, U)]
        if not plateau and U >= 8:                                            # hand-made users among ordinary ones
            for u, (name, t) in zip((1, 3, 4, 6, 7), SPECIAL_TAUS.items()):
                if name != "tautiny" or "s" not in c.opt:                     # times 1 / tau the smallest normal would overflow the row
                    I.tau_u[u], I.special[u] = t, name
            I.news[5] = NAN                                                   # a NaN news row: a term of nothing, its own K22 row minus named terms only
            I.news[6, N - 1] = INF                                            # one infinite component: a NaN score (0 * inf) for everyone, 0 in E
            I.user[:, N - 1] = 0.0
            lone = [b for b in np.flatnonzero(T.cnt == 1) if b != zb and int(T.order[T.bin_start[b]]) not in (5, 6)]
            if lone and U >= 13 and len(full_bins) >= 3:                                              # a bin of one news that scores -inf for everyone (max -inf, count 1, logsum NaN;
                I.inf_bin = int(lone[0])                                      # nothing to K20 / K22) and +inf for user 12 (max +inf, logsum NaN; K20 NaN, K22 dead)
                v1 = int(T.order[T.bin_start[I.inf_bin]])
                I.news[v1] = 0.0
                I.news[v1, 0] = -INF
                I.user[:, 0] = np.abs(I.user[:, 0]) + f32(1e-3)
                I.user[12, 0] = -I.user[12, 0]
                I.special[12] = "posinf"
                if I.prior is not None:
                    I.prior[v1] = 0.0
                if I.stamp is not None:
                    I.stamp[v1] = 3                                           # inside every window [lo <= 3, lo + 3 >= 3]
    nb = G + 1
    if plateau:
        I.omega = np.array([0.0, 0.5, 1.0, 2.0, -2.0, 4.0], f32)[rng.integers(0, 6, (U, nb))]
    else:
        I.omega = rng.standard_normal((U, nb)).astype(f32)
    I.omega[::4, zb] = 0.0
    if U >= 6:
        I.omega[5] = 0.0
    I.zero_bin, I.bad_bin = zb, None
    if I.inf_bin is not None:
        I.omega[:, I.inf_bin] = np.where(I.omega[:, I.inf_bin] == 0, f32(0.5), I.omega[:, I.inf_bin])      # weighted, so that the maximum decides
    if I.special and U >= 12:                                                 # defects of a weighted non-empty bin: users 9, 10, 11 (spoiled_base)
        I.bad_bin = int(max((b for b in full_bins if b != zb and b != I.inf_bin), key=lambda b: T.cnt[b]))
        I.omega[9:12, I.bad_bin] = (1.5, INF, -0.75)
        I.special.update({9: "logsumnan", 10: "omegainf", 11: "gmaxinf"})
    if c.T:
        I.sub_ids = rng.integers(-1, V + 2, (U, c.T)).astype(i32)
        I.sub_w = np.array([0.0, 0.5, -1.0, 2.0], f32)[rng.integers(0, 4, (U, c.T))] if plateau else rng.standard_normal((U, c.T)).astype(f32)
        if c.T >= 2:
            I.sub_ids[:, 1] = I.sub_ids[:, 0]
    if c.named:
        cnt = rng.integers(0, 4, V)                                           # 0 - 3 terms per news, row 0 and news of empty-based bins among them
        n = int(cnt.sum()) + 1
        I.n_user = rng.integers(-1, U + 1, n).astype(i32)                     # -1 and U: outside [0, U)
        I.n_w = (np.array([0.0, 0.5, -1.0, 2.0])[rng.integers(0, 4, n)] if plateau else rng.standard_normal(n) * (rng.random(n) > 0.2)).astype(f32)
        if I.special:
            I.n_user[:5] = (1, 3, 4, 6, 7)[:len(I.n_user[:5])]                # the dead-tau users named
        I.n_off = np.concatenate([[0], np.cumsum(cnt)]).astype(i32)
        I.n_off[V] += 5                                                       # beyond n_named: clamped
    return I


# ---------------------------------------------------------------------------------------- 3 the float64 reference of the stream cases
def eligible(I, V):
    return SW.eligible(SimpleNamespace(user=I.user, news=I.news, prior=I.prior, stamp=I.stamp, window=I.window, segs=I.segs))


def cap_reference(c, I, T):
    """The contracts of K15 and K20 in float64 on the fp32 inputs, per (user, bin): gmax, count, logsum, m (eligible news at the
    maximum), dmin (the largest (s - gmax) / tau below 0); P [U, V] the softmax inside each bin; E, A, mass, Mabs of K20 before
    and S, AS of its named rows; nan20: the users K20 answers with NaN; per user n, C, G of the header's bounds (C and G over the
    bins with omega != 0, Gall over everything eligible)."""
    U, V, N, nb = c.U, T.V, c.N, T.G + 1
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    clean = np.where(np.isfinite(n64), n64, 0.0)
    with np.errstate(all="ignore"):
        s = u64 @ n64.T
        mag = np.abs(u64) @ np.abs(n64).T
        if I.prior is not None:
            s, mag = s + I.prior.astype(f64)[None, :], mag + np.abs(I.prior.astype(f64))[None, :]
    el = eligible(I, V) & ~np.isnan(s)
    tau, tau_ok = SW.taus(c, I)
    tau = tau.astype(f64)
    R = SimpleNamespace(gmax=np.full((U, nb), -INF), count=np.zeros((U, nb), np.int64), logsum=np.full((U, nb), -INF), m=np.zeros((U, nb), np.int64),
                        dmin=np.full((U, nb), -INF), P=np.zeros((U, V)), tau=tau, tau_ok=tau_ok, el=el, s=s)
    safe = np.where(tau_ok, tau, 1.0)
    with np.errstate(all="ignore"):
        for b in np.flatnonzero(T.cnt):
            cols = np.flatnonzero(T.bins == b)
            cols = cols[cols >= 1]
            e = el[:, cols]
            x = np.where(e, s[:, cols], -INF)
            R.count[:, b] = e.sum(axis=1)
            gm = x.max(axis=1)
            R.gmax[:, b] = np.where(R.count[:, b] > 0, gm, -INF)
            R.m[:, b] = (e & (x == gm[:, None])).sum(axis=1)
            ok = (R.count[:, b] > 0) & tau_ok & np.isfinite(gm)
            z = np.where(e & ok[:, None], (x - np.where(ok, gm, 0.0)[:, None]) / safe[:, None], -INF)
            R.dmin[:, b] = np.where(z < 0, z, -INF).max(axis=1)
            w = np.where(e & ok[:, None], np.exp(z), 0.0)
            tot = w.sum(axis=1)
            R.logsum[:, b] = np.where(R.count[:, b] == 0, -INF, np.where(ok, np.log(np.where(ok, tot, 1.0)), NAN))
            R.P[:, cols] = np.where(ok[:, None], w / np.where(ok, tot, 1.0)[:, None], 0.0)
    om = I.omega.astype(f64)
    with np.errstate(invalid="ignore"):                                       # an infinite omega: that user's row is NaN anyway
        W = om[:, T.bins] * R.P
        R.E, R.A = W @ clean, np.abs(W) @ np.abs(clean)
    full = (R.count > 0) & (R.gmax > -INF)                                    # K20 reads a maximum of -inf as an empty bin, whatever the count
    R.full = full
    R.mass, R.Mabs = np.where(full, om, 0.0).sum(axis=1), np.where(full, np.abs(om), 0.0).sum(axis=1)
    R.nan20 = (full & ~tau_ok[:, None]).any(axis=1) | (full & (om != 0) & (~np.isfinite(om) | (R.gmax == INF))).any(axis=1)
    if I.bad_bin is not None:                                                 # what only the bases handed to K20 know
        R.nan20[9] |= full[9, I.bad_bin]                                     # a NaN logsum counts where the base's maximum says "not empty"
        R.nan20[11] = True                                                    # a maximum of +inf says so itself
    R.S, R.AS = np.zeros((U, N)), np.zeros((U, N))
    if I.sub_ids is not None:
        for u in range(U):
            ids, w = I.sub_ids[u].astype(np.int64), I.sub_w[u].astype(f64)
            for t in np.flatnonzero((ids >= 1) & (ids < V)):                  # the named rows as they are: a non-finite component reaches the output
                with np.errstate(invalid="ignore"):
                    R.S[u], R.AS[u] = R.S[u] + w[t] * n64[ids[t]], R.AS[u] + abs(w[t]) * np.abs(n64[ids[t]])
    used = el & (om[:, T.bins] != 0)
    with np.errstate(all="ignore"):
        it = np.where(tau_ok, 1.0 / safe, 0.0)
        R.n = R.count.max(axis=1).astype(f64)
        R.C = np.where(used & np.isfinite(s), np.abs(s), 0.0).max(axis=1) * it
        R.G = np.where(used & np.isfinite(mag), mag, 0.0).max(axis=1) * it
        R.Gall = np.where(el & np.isfinite(mag), mag, 0.0).max(axis=1) * it
        R.magmax = np.where(el & np.isfinite(mag), mag, 0.0).max(axis=1)
    return R


def finish20(c, R):
    """(out*, A with the named rows) of K20: (E - S) (* 1 / tau)."""
    out, tot = R.E - R.S, R.A + R.AS
    if "s" in c.opt:
        with np.errstate(all="ignore"):
            out, tot = out / R.tau[:, None], tot / R.tau[:, None]
    out = np.where(R.nan20[:, None], NAN, out)
    return out, tot


def plateau_condition(R):
    """Every (s - gmax_b) / tau is 0 or <= -128 and every maximum is a fp32 number, for every (user, bin) that has weights."""
    live = (R.count > 0) & R.tau_ok[:, None]
    return bool((R.dmin[live] <= -128.0).all() and (R.gmax[live].astype(f32).astype(f64) == R.gmax[live]).all())


def news_reference(c, I, T, R):
    """(out*, mass*, A, M, n, C, G) of K22: tests/test_gpu_capgrad_news.py's _reference (metrics.expect_news_groups_reference)."""
    hkw = {k: v for k, v in (("prior", I.prior), ("stamp", I.stamp), ("window", I.window), ("exclude", I.segs)) if v is not None}
    named = None
    if I.n_off is not None:
        off = np.minimum(I.n_off, len(I.n_user))
        keep = (I.n_user >= 0) & (I.n_user < c.U)
        named = tuple(torch.from_numpy(x) for x in (np.concatenate([[0], np.cumsum(keep)])[off].astype(i32), I.n_user[keep], I.n_w[keep]))
    tau = torch.from_numpy(I.tau_u.astype(f64)) if I.tau_u is not None else float(f32(I.tau))
    dead = (R.count > 0) & ~np.isfinite(R.gmax)                               # a maximum of +-inf: the pair is dead
    if I.bad_bin is not None:                                                 # pairs that are dead through the bases handed over
        dead[[9, 11], I.bad_bin] = True
    with np.errstate(all="ignore"):
        return GN._reference(torch.from_numpy(I.news), torch.from_numpy(I.user), tau, torch.from_numpy(T.group), T.G, torch.from_numpy(I.omega), hkw, named=named,
                             scale="s" in c.opt, dead=dead)


# ---------------------------------------------------------------------------------------- 4 problems: the buffers of one call
def strides(c, T, variant):
    N, U, G = c.N, c.U, T.G
    if variant == "dense":
        return SimpleNamespace(news=N, user=N, out=N, base=G + 1, bin=U, sub=c.T, win=2)
    o = (N, N + 4, tk_npad(N) + 8)
    return SimpleNamespace(news=o[c.pad], user=o[(c.pad + 1) % 3], out=N + (4 if c.pad != 1 else 0), base=G + 1 + (3 if c.pad != 2 else 0), bin=U + (3 if c.pad != 0 else 0),
                           sub=c.T + (3 if c.pad != 2 else 0), win=5 if c.pad != 0 else 2)


def problem(entry, c, I, T, dev, variant="pad", base=None):
    """Every buffer of one call of `entry` (logzg, expectg, newsg) on case c; base = (out_max, out_logsum) [U, n_groups + 1] of
    K15 for the other two.  variant: pad (padded strides, the least alignment), dense, shift (every base moved)."""
    S, sh = strides(c, T, variant), variant == "shift"
    fo, io, wo = (0 if sh else 4), (2 if sh else 1), (4 if sh else 2)
    U, V, N, nb = c.U, T.V, c.N, T.G + 1
    P = SimpleNamespace(entry=entry, c=c, I=I, T=T, S=S, inb={}, outb={}, ws=None)
    P.inb["news"], P.inb["user"] = in_buf(I.news, S.news, dev, fo, NAN), in_buf(I.user, S.user, dev, fo, NAN)
    P.inb["order"] = in_buf(T.order, T.n_pos, dev, io)
    if entry == "newsg":
        P.inb["bin_start"] = in_buf(T.bin_start, nb + 1, dev, io)
    else:
        P.inb["seg_start"], P.inb["bin_seg"] = in_buf(T.seg_start, T.nseg + 1, dev, io), in_buf(T.bin_seg, nb + 1, dev, io)
    if I.prior is not None:
        P.inb["prior"] = in_buf(I.prior, V, dev, io)
    if I.stamp is not None:
        P.inb["stamp"] = in_buf(I.stamp, V, dev, io)
        P.inb["window"] = in_buf(I.window, S.win, dev, io, np.tile(np.array([100, -100, 100], i32), (U, 1)))
    if I.segs is not None:
        off, x = _list_arrays(I, T, U, entry == "newsg")
        P.inb["offsets"], P.inb["xids"] = in_buf(off, len(off), dev, io), in_buf(x, len(x), dev, io)
    if I.tau_u is not None:
        P.inb["tau_u"] = in_buf(I.tau_u, U, dev, io)
    if entry == "logzg":
        P.outb["logsum"], P.outb["max"], P.outb["count"] = (out_buf(U, nb, nb, t, dev, io) for t in (torch.float32, torch.float32, torch.int32))
    elif entry == "expectg":
        P.inb["base_max"], P.inb["base_logsum"] = in_buf(base[0], S.base, dev, io, NAN), in_buf(base[1], S.base, dev, io, NAN)
        P.inb["bin_w"] = in_buf(I.omega, S.base, dev, io, 1e30)
        if I.sub_ids is not None:
            P.inb["sub_ids"], P.inb["sub_w"] = in_buf(I.sub_ids, S.sub, dev, io, 1 if V > 1 else 0), in_buf(I.sub_w, S.sub, dev, io, 1e30)
        P.outb["out"] = out_buf(U, N, S.out, torch.float32, dev, fo)
    else:
        P.inb["base_max"], P.inb["base_logsum"] = in_buf(base[0].T, S.bin, dev, io, NAN), in_buf(base[1].T, S.bin, dev, io, NAN)
        P.inb["bin_w"] = in_buf(I.omega.T, S.bin, dev, io, 1e30)
        if I.n_off is not None:
            P.inb["n_off"], P.inb["n_user"], P.inb["n_w"] = in_buf(I.n_off, V + 1, dev, io), in_buf(I.n_user, len(I.n_user), dev, io), in_buf(I.n_w, len(I.n_w), dev, io)
        P.outb["out"] = out_buf(V, N, S.out, torch.float32, dev, fo)
    if entry != "logzg" and "M" in c.opt:
        n = U if entry == "expectg" else V
        P.outb["mass"] = out_buf(1, n, n, torch.float32, dev, io)
    P.ws_bytes = ws_bytes(entry, c, T)
    P.ws = glue_buf(1, P.ws_bytes // 4, P.ws_bytes // 4, torch.float32, dev, wo, NAN)
    if not sh:                                                                # the least alignment the header allows, and no more
        assert P.inb["news"].ptr % 32 == 16 and P.inb["user"].ptr % 32 == 16 and P.ws.ptr % 16 == 8
        assert "out" not in P.outb or P.outb["out"].ptr % 32 == 16
        assert all(b.ptr % 8 == 4 for k, b in list(P.inb.items()) + list(P.outb.items()) if k not in ("news", "user", "out"))
    return P


def all_bufs(P):
    return list(P.inb.items()) + list(P.outb.items()) + ([("ws", P.ws)] if P.ws is not None else [])


def results(P):
    return {k: b.v.cpu().numpy().copy() for k, b in P.outb.items()}


def execute(make, call, twice=True):
    """One checked call on the problem make() builds: every guard and slack element intact (`sentinel`), a second problem built
    alike gives the same bits (`repeat`).  Returns the outputs as numpy arrays."""
    Ps = [make() for _ in range(2 if twice else 1)]
    for P in Ps:
        call(P)
    for name, b in all_bufs(Ps[0]):
        _sent(f"{Ps[0].entry} {name}", b)
    if twice:
        for (name, a), (_, b) in zip(Ps[0].outb.items(), Ps[1].outb.items()):
            need(torch.equal(_bits(a.flat), _bits(b.flat)), "repeat", "{} {}: two runs from the same state differ", Ps[0].entry, name)
    return results(Ps[0])


def spoiled_base(I, lz):
    """(out_max, out_logsum) of K15 as K20 and K22 get them: NaN under every weight of exactly 0 in the chosen bin (the logsum for
    users 0, 8, ..., the maximum for users 4, 12, ...), and the defects of the special users 9 and 11 under a weight that is not 0."""
    bm, bl = lz["max"].copy(), lz["logsum"].copy()
    bl[0::8, I.zero_bin] = NAN
    bm[4::8, I.zero_bin] = NAN
    if I.bad_bin is not None:                                                 # under a weight that is not 0: user 9 a NaN logsum, user 11 a maximum of +inf
        bl[9, I.bad_bin], bm[11, I.bad_bin] = NAN, INF
    return bm, bl


def run_chain(c, I, T, dev, call, variant="pad", twice=True, entries=STREAM):
    """K15, then K20 on the bases it returned, then K22 on their transposes: {entry: outputs}."""
    out = {"logzg": execute(lambda: problem("logzg", c, I, T, dev, variant), call, twice)}
    base = spoiled_base(I, out["logzg"])
    for e in entries[1:]:
        out[e] = execute(lambda: problem(e, c, I, T, dev, variant, base), call, twice)
    return out


# ---------------------------------------------------------------------------------------- 5 the checker of the stream cases
def slice_terms(c, I, T, R):
    """[U] the nonzero terms the fullest slice of K20 adds for a user on plateau data: the eligible news at their bin's maximum, over
    ALL bins with omega != 0, counted per slice."""
    p = plan("expectg", c, T)
    on = (R.P > 0) & (I.omega.astype(f64)[:, T.bins] != 0)
    worst = np.zeros(c.U, np.int64)
    for lo, hi in slices(T, p.splits):
        if lo >= hi:
            continue
        ids = T.order[T.seg_start[lo]:T.seg_start[hi]]
        ids = ids[(ids >= 1) & (ids < T.V)]
        worst = np.maximum(worst, on[:, ids].sum(axis=1))
    return worst


def cap_check(c, I, T, out, R):
    """The outputs of a stream case against the contract; returns the worst |error| / bound per output."""
    kind = c.kind
    layer = {"plateau": "exact", "gauss": "special" if I.special else "bound"}[kind]
    w, kx = {}, 1 + CAPPED_EXCESS
    U, V, N = c.U, T.V, c.N
    lz = out["logzg"]
    lmax, lcount, lsum = lz["max"], lz["count"], lz["logsum"]
    same_bits(layer, "out_count", lcount, R.count.astype(i32))
    empty, live = R.count == 0, (R.count > 0) & R.tau_ok[:, None] & np.isfinite(R.gmax)
    need(bool(np.isneginf(lsum[empty]).all() and np.isneginf(lmax[empty]).all()), layer, "an empty bin must give max and logsum -inf")
    need(np.array_equal(np.isnan(lsum), np.isnan(R.logsum)), layer, "out_logsum: NaN at {} (user, bin) pairs, the contract says {}", int(np.isnan(lsum).sum()),
         int(np.isnan(R.logsum).sum()))
    if kind == "plateau":
        same_bits("exact", "out_max", lmax, R.gmax.astype(f32))
        one, many = live & (R.m == 1), live & (R.m > 1)
        need(bool((lsum[one] == 0).all() and not np.signbit(lsum[one]).any()), "exact", "out_logsum: one maximum must give +0.0")
        want = np.log(np.maximum(R.m, 1).astype(f64)).astype(f32)
        okl = (lsum == want) | (lsum == np.nextafter(want, f32(INF))) | (lsum == np.nextafter(want, f32(-INF)))
        need(bool(okl[many].all()), "exact", "out_logsum: {} (user, bin) pairs are neither float32(log m) nor its neighbour", int((many & ~okl).sum()))
    else:
        N_e = N * EPS / (1 - N * EPS)
        sb = kx * (N_e + EPS) * R.magmax[:, None] + (N + 1) * 2.0 ** -149
        w["max"] = _ratio(layer, "out_max", lmax, R.gmax, np.broadcast_to(sb, lmax.shape), ~empty)
        lb = kx * np.vectorize(lambda n: LG.lzg_bound(n, T.S))(R.count) + 2.0 * (N + 1) * R.Gall[:, None] * EPS
        w["logsum"] = _ratio(layer, "out_logsum", lsum, R.logsum, lb, live)
    om = I.omega.astype(f64)
    omax = max(float(np.abs(om[np.isfinite(om)]).max(initial=0.0)), 1.0)
    weighted = R.full & (om != 0)
    lnm = np.log(np.where(weighted & live, R.m, 1).max(axis=1).astype(f64))          # of the user's largest plateau among its weighted bins
    # ---- K20
    o = out.get("expectg")
    if o is not None:
        ref, tot = finish20(c, R)
        g = o["out"]
        nanrow = np.isnan(ref).any(axis=1)                                    # R.nan20, and a user that names a NaN news row: subtracted as it is
        need(np.array_equal(np.isnan(g), np.isnan(ref)), layer, "K20 out: NaN for users {}, the contract says {}", np.flatnonzero(np.isnan(g).any(axis=1)).tolist(),
             np.flatnonzero(nanrow).tolist())
        rows = ~nanrow
        none = rows & ~weighted.any(axis=1)                                   # nothing weighted: exactly minus the named rows
        if kind == "plateau":
            single = rows & ~(weighted & (R.m > 1)).any(axis=1)
            need(bool((g[single].astype(f64) == ref[single].astype(f32).astype(f64)).all()), "exact", "K20 out: a user whose weighted bins all have one maximum must equal "
                 "the fp64 lattice value rounded once")
            kt = slice_terms(c, I, T, R) + 3.0 * lnm + 7.0
            w["tight_expectg"] = _ratio("tight", "K20 out", g, ref, kt[:, None] * EPS * tot + 2.0 ** -149, rows & ~single)
        else:
            _ratio(layer, "K20 out of a user without a weighted bin (minus its named rows)", g, ref, 2.0 * EPS * tot + 2.0 ** -149, none)
            L = max(int(T.seg_start[hi] - T.seg_start[lo]) for lo, hi in slices(T, plan("expectg", c, T).splits) if lo < hi) // 128
            kap = GC.kappa20(N, R.n, R.C, R.G, T.S, L)
            big = float(np.abs(np.where(np.isfinite(I.news[1:]), I.news[1:], 0.0)).max(initial=0.0))
            it = 1.0 / np.where(R.tau_ok, R.tau, 1.0) if "s" in c.opt else 1.0
            tiny = (R.n * 2.0 ** -126 * omax * big * it)[:, None]         # weights below the normal range
            w["expectg"] = _ratio(layer, "K20 out", g, ref, kx * kap[:, None] * EPS * tot + tiny + 2.0 ** -149, rows)
        if "mass" in o:
            mg = o["mass"][0]
            need(np.array_equal(np.isnan(mg), R.nan20), layer, "K20 mass: NaN where the contract has none, or the reverse")
            need(not mg[~R.nan20 & ~weighted.any(axis=1)].any(), layer, "K20 mass: nothing weighted must give 0")
            if kind == "plateau":
                need(bool((mg[single].astype(f64) == R.mass[single].astype(f32).astype(f64)).all()), "exact", "K20 mass: one maximum per weighted bin must give the exact sum of omega")
                w["tight_expectg_mass"] = _ratio("tight", "K20 mass", mg, R.mass, (3.0 * lnm + 8.0) * EPS * R.Mabs + 2.0 ** -149, ~R.nan20 & ~single)
            else:
                mb = kx * (6.0 * R.C + 5.0 * np.log(np.maximum(R.n, 2)) + 14.0 * T.S + 23.0) * EPS * R.Mabs
                w["expectg_mass"] = _ratio(layer, "K20 mass", mg, R.mass, mb + R.n * 2.0 ** -126 * omax + 2.0 ** -149, ~R.nan20)
    # ---- K22
    o = out.get("newsg")
    if o is not None:
        ref, mass, A, M, n, Cn, Gn = news_reference(c, I, T, R)
        g = o["out"]
        for k, x in o.items():
            need(bool(np.isfinite(x).all()), layer, "K22 {}: a value that is not finite", k)
        p = plan("newsg", c, T)
        kr, km = GN.kappa22(N, U, p.splits, n, Cn, Gn, T.S)
        if kind == "plateau":
            on = (R.P > 0) & (om[:, T.bins] != 0)                              # the pairs that carry weight: v is a maximum of (u, bin(v))
            n_v = on.sum(axis=0).astype(f64)
            m_v = np.where(on, R.m[:, T.bins], 1).max(axis=0)
            single, many = m_v == 1, m_v > 1
            need(bool((g[single].astype(f64) == ref[single].astype(f32).astype(f64)).all()), "exact", "K22 out: rows {} differ from the exact lattice value rounded once",
                 np.flatnonzero(single & (g.astype(f64) != ref.astype(f32).astype(f64)).any(axis=1)).tolist()[:8])
            kt = n_v + 3.0 * np.log(m_v.astype(f64)) + 7.0
            w["tight_newsg"] = _ratio("tight", "K22 out", g, ref, kt[:, None] * EPS * A + 2.0 ** -149, many)
        else:
            w["newsg"] = _ratio(layer, "K22 out", g, ref, kx * kr * EPS * A + 2.0 ** -149, np.ones(V, bool))
        if "mass" in o:
            mg = o["mass"][0]
            if kind == "plateau":
                need(bool((mg[single].astype(f64) == mass[single].astype(f32).astype(f64)).all()), "exact", "K22 mass: differs from the exact sum of the weights")
                w["tight_newsg_mass"] = _ratio("tight", "K22 mass", mg, mass, (3.0 * np.log(m_v.astype(f64)) + 8.0) * EPS * M + 2.0 ** -149, many)
            else:
                w["newsg_mass"] = _ratio(layer, "K22 mass", mg, mass, kx * km * EPS * M + 2.0 ** -149, np.ones(V, bool))
    return w


def _compare(layer, what, a, b):
    for e in a:
        for k in a[e]:
            same_bits(layer, f"{e} {k} {what}", a[e][k], b[e][k])


def cap_agree(c, I, T, out, dev, call, logz=None):
    """The bit-for-bit statements of the header that tie the calls together (module docstring, `agree`)."""
    for s in sorted({0, 1, min(2, T.nseg), T.nseg}):
        other = execute(lambda: problem("logzg", c._replace(splits=s), I, T, dev), call, twice=False)
        _compare("agree", f"at splits = {s}", {"logzg": out["logzg"]}, {"logzg": other})
    if logz is not None:                                                      # K13 under the same pools and lists
        smax, count = logz(c, I, T)
        same_bits("agree", "max over the bins of out_max against K13's out_max", out["logzg"]["max"].max(axis=1), smax)
        same_bits("agree", "sum over the bins of out_count against K13's out_count", out["logzg"]["count"].sum(axis=1).astype(i32), count)
    ce = c if c.splits else c._replace(splits=1)
    ce = ce if ce.vs else ce._replace(vs=1)
    base = spoiled_base(I, out["logzg"])
    fixed = {e: execute(lambda: problem(e, ce, I, T, dev, "pad", base), call, twice=False) for e in STREAM[1:]}
    # K20 row u when every other user is replaced: K15 again for their bases, user u's own base is what it was
    u = c.U // 2
    I2 = SimpleNamespace(**vars(I))
    rng = _rng(13, c.N, c.U, T.V)
    I2.user = (I.user[rng.permutation(c.U)] * f32(1.5)).astype(f32)
    I2.user[u] = I.user[u]
    lz2 = execute(lambda: problem("logzg", ce, I2, T, dev), call, twice=False)
    for k in ("max", "logsum", "count"):
        same_bits("agree", f"K15 {k} of user {u} when the other users are replaced", lz2[k][u], out["logzg"][k][u])
    o2 = execute(lambda: problem("expectg", ce, I2, T, dev, "pad", spoiled_base(I, lz2)), call, twice=False)
    for k in fixed["expectg"]:
        x, y = (fixed["expectg"][k][u], o2[k][u]) if k == "out" else (fixed["expectg"][k][:, u], o2[k][:, u])
        same_bits("agree", f"K20 {k} of user {u} when the other users are replaced", x, y)
    if u + 1 < c.U:                                                           # ... and when U changes: the users up to u alone
        I4 = SimpleNamespace(**vars(I))
        for k in ("user", "window", "tau_u", "omega", "sub_ids", "sub_w"):
            if getattr(I, k) is not None:
                setattr(I4, k, getattr(I, k)[:u + 1])
        I4.segs = I.segs[:u + 1] if I.segs is not None else None
        o4 = execute(lambda: problem("expectg", ce._replace(U=u + 1), I4, T, dev, "pad", (base[0][:u + 1], base[1][:u + 1])), call, twice=False)
        for k in fixed["expectg"]:
            x, y = (fixed["expectg"][k][u], o4[k][u]) if k == "out" else (fixed["expectg"][k][:, u], o4[k][:, u])
            same_bits("agree", f"K20 {k} of user {u} when U changes", x, y)
    # K22 row v when v's place in its run moves and other bins change size: the first news of v's bin go to the next bin; same bases
    b = int(np.argmax(T.cnt))
    if T.cnt[b] >= 5:
        mine = 1 + np.flatnonzero(T.bins[1:] == b)
        vm, nb_ = int(mine[-1]), (b + 1) % (T.G + 1)
        group5 = T.group.copy()
        group5[mine[:3]] = nb_ if nb_ < T.G else -1
        T5 = group_tables(group5, T.G, "x" in c.opt)
        T5.group = group5
        assert T5.pos[vm] != T.pos[vm] and T5.bins[vm] == T.bins[vm]
        o5 = execute(lambda: problem("newsg", ce, I, T5, dev, "pad", base), call, twice=False)
        for k in fixed["newsg"]:
            x, y = (fixed["newsg"][k][vm], o5[k][vm]) if k == "out" else (fixed["newsg"][k][:, vm], o5[k][:, vm])
            same_bits("agree", f"K22 {k} of news {vm} when its place in its run moves and other bins change size", x, y)
    # K22 row v when every other news row is replaced, on the same bases
    v = max(1, T.V // 2)
    I3 = SimpleNamespace(**vars(I))
    I3.news = (I.news[np.concatenate([[0], 1 + rng.permutation(T.V - 1)])] * f32(0.5)).astype(f32)
    I3.news[0], I3.news[v] = I.news[0], I.news[v]
    o3 = execute(lambda: problem("newsg", ce, I3, T, dev, "pad", base), call, twice=False)
    for k in fixed["newsg"]:
        x, y = (fixed["newsg"][k][v], o3[k][v]) if k == "out" else (fixed["newsg"][k][:, v], o3[k][:, v])
        same_bits("agree", f"K22 {k} of news {v} when the other rows are replaced", x, y)


def cap_special(c, I, T, out, dev, call):
    """The ordinary users' bits of K15 and K20 equal those of the same call without the special users (the case names its splits)."""
    keep = np.array([u for u in range(c.U) if u not in I.special])
    I2 = SimpleNamespace(**vars(I))
    for k in ("user", "window", "tau_u", "omega", "sub_ids", "sub_w"):
        if getattr(I, k) is not None:
            setattr(I2, k, getattr(I, k)[keep])
    I2.segs = [I.segs[u] for u in keep] if I.segs is not None else None
    c2 = c._replace(U=len(keep))
    lz = execute(lambda: problem("logzg", c2, I2, T, dev), call, twice=False)
    for k in lz:
        same_bits("special", f"K15 {k} of the ordinary users without the special ones", out["logzg"][k][keep], lz[k])
    bm, bl = spoiled_base(I, out["logzg"])
    o = execute(lambda: problem("expectg", c2, I2, T, dev, "pad", (bm[keep], bl[keep])), call, twice=False)
    for k in o:
        x = out["expectg"][k][keep] if k == "out" else out["expectg"][k][:, keep]
        same_bits("special", f"K20 {k} of the ordinary users without the special ones", x, o[k])


def cap_sweep(c, dev, call, layout=True, agree=True, logz=None):
    """The driver both files share: every layer of one stream case."""
    T = tables(c)
    c = resolve(c, T)
    I = cap_inputs(c, T)
    R = cap_reference(c, I, T)
    out = run_chain(c, I, T, dev, call)
    w = cap_check(c, I, T, out, R)
    if layout:
        for variant in ("dense", "shift"):
            _compare("layout", f"with {variant} buffers", run_chain(c, I, T, dev, call, variant, twice=False), out)
    if carries_agree(c):
        if agree:
            cap_agree(c, I, T, out, dev, call, logz)
    if carries_special(c, I):
        cap_special(c, I, T, out, dev, call)
    return w


def carries_agree(c):
    """`agree` (the splits of K15, K13's max and count, the rows of K20 and K22 under other users, news, U and tables) runs for the
    Gaussian cases of up to 300 users: every one of them but the U = 32 774 case."""
    return c.kind == "gauss" and c.U <= 300


def carries_special(c, I):
    """The ordinary users' bits without the special ones are compared where the case has special users (Gaussian, per-user
    temperatures, U >= 8) and names its splits (c is the resolved case): bits are promised for a fixed explicit `splits`."""
    return bool(I.special) and c.splits > 0


# ---------------------------------------------------------------------------------------- 6 the row calls (K16, K21)
# hand: 0 random rows; 1 user 0's row is built by hand (hand_row): a bin that closes at place 0 (cap 1) or cap - 1, one that
# closes at the last place, two bins that close at the neighbouring places 2 l and 2 l + 1 of one lane, blocked entries of two
# bins interleaved, a key-0 entry between the live entries of a bin that later closes, fill ids in the middle; 2 every news in one
# group (cap 127 closes at place 126 and blocks the last entry, cap 128 closes at place 127 and blocks nothing); 3 the row takes
# everything eligible over empty bases.
RowCase = collections.namedtuple("RowCase", "name N U V k cap G pool taus g total pad hand")
ROW_KS = (1, 2, 63, 64, 65, 127, 128)
ROW_US = (1, 7, 8, 9, 15, 16, 17, 33)
ROW_CAPS = (1, 2, 3, 127, 128)
ROW_GS = (1, 63, 64, 65, 511, 512)
ROW_ROUTES = ("p0", "p1", "g_null", "g_given", "total_null", "total_given", "tau_scalar", "tau_u", "one_round", "two_rounds", "more_blocks", "bins_in_one_pass", "bins_lane_loop",
              "cap_binds", "closes_at_127", "hand_row")


def row_cases():
    cs = []
    for i, k in enumerate(ROW_KS):
        for h in range(2):
            j = 2 * i + h
            cs.append(RowCase(f"rows-k{k}-{h}", CAP_NS[(3 * i + 5 * h) % 10], ROW_US[j % 8], (130, 257, 294)[j % 3], k, ROW_CAPS[j % 3], (3, 5, 1)[j % 3] if h else ROW_GS[j % 6],
                              j % 4, (j // 2) % 2, (j // 3) % 2, j % 2, j % 3, int(h and k >= 63)))
    for i, G in enumerate(ROW_GS):
        cs.append(RowCase(f"rows-G{G}", (4, 36)[i % 2], ROW_US[(i + 3) % 8], 294, (128, 65, 64)[i % 3], (1, 2)[i % 2], G, (1, 0, 3, 2)[i % 4], i % 2, (i + 1) % 2, (i + 1) % 2, i % 3, 0))
    cs += [RowCase("rows-cap127", 36, 9, 200, 128, 127, 1, 0, 1, 1, 1, 1, 2), RowCase("rows-cap128", 4, 17, 200, 128, 128, 1, 0, 0, 0, 1, 2, 2),
           RowCase("rows-cap127-k127", 28, 7, 200, 127, 127, 2, 2, 1, 1, 0, 0, 2), RowCase("rows-hand-cap1", 36, 33, 294, 128, 1, 5, 1, 1, 1, 1, 1, 1),
           RowCase("rows-hand-cap3", 4, 16, 294, 127, 3, 4, 0, 0, 1, 1, 2, 1), RowCase("rows-all-taken", 36, 5, 7, 6, 3, 2, 0, 0, 1, 1, 1, 3)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def row_route(c):
    """nr_row_logprob_capped / _grad: logp_capped_kernel<POOL> and logp_capped_grad_kernel<POOL>, 16 users a workgroup in two rounds of
    8 waves; the lanes stride the n_groups + 1 bins by 64."""
    I = row_inputs(c)
    r = [f"p{int(bool(c.pool))}", "g_given" if c.g else "g_null", "total_given" if c.total else "total_null", "tau_u" if c.taus else "tau_scalar",
         "one_round" if c.U % 16 in range(1, 9) and c.U < 16 else "two_rounds", "bins_in_one_pass" if c.G + 1 <= 64 else "bins_lane_loop"]
    if c.U > 16:
        r.append("more_blocks")
    if c.hand == 1:
        r.append("hand_row")
    blocked, close127 = row_facts(c, I)
    if blocked:
        r.append("cap_binds")
    if close127:
        r.append("closes_at_127")
    return tuple(r)


def hand_row(c, group, rng):
    """User 0's row of a hand = 1 case (k >= 63, cap <= 3, four groups with 3 cap + 2 news each): see the comment above RowCase."""
    k, cap = c.k, c.cap
    by = [[v for v in 1 + np.flatnonzero(group[1:] == b) if v != 5] for b in range(4)]
    free = list(1 + np.flatnonzero(group[1:] < 0))
    assert all(len(x) >= 3 * cap + 2 for x in by) and len(free) >= k
    row = [free.pop() for _ in range(k)]                                      # news of no group: never capped
    take = lambda b: by[b].pop()
    at = 0
    for _ in range(cap):                                                      # bin 0 closes at place cap - 1 (place 0 under cap 1)
        row[at] = take(0)
        at += 1
    for _ in range(cap - 1):                                                  # bins 1 and 2: cap - 1 entries each, then their closing
        row[at], row[at + 1] = take(1), take(2)                               # entries at the neighbouring places 2 l, 2 l + 1
        at += 2
    at += at % 2
    row[at], row[at + 1] = take(1), take(2)
    at += 2
    for _ in range(3):                                                        # blocked entries of bins 1, 2 and 0, interleaved
        row[at], row[at + 1], row[at + 2] = take(1), take(2), take(0)
        at += 3
    row[at], row[at + 1], row[at + 2] = 0, -4, c.V + 3                        # fill in the middle
    at += 3
    live3 = [take(3) for _ in range(cap)]                                     # bin 3: a key-0 entry between its live entries; it closes at the last place
    if cap == 1:
        row[k - 2], row[k - 1] = 5, live3[0]
    else:
        row[at], row[at + 1] = live3[0], 5
        for j, v in enumerate(live3[1:-1]):
            row[at + 2 + j] = v
        row[k - 1] = live3[-1]
    assert at + cap + 2 < k
    return np.array(row, i32)


def row_inputs(c):
    rng = _rng(37, c.N, c.U, c.V, c.k, c.cap, c.G, c.pool, c.pad, c.hand)
    V, U, N, k, G = c.V, c.U, c.N, c.k, c.G
    I = SimpleNamespace(prior=None, stamp=None, window=None, tau=0.7, tau_u=None, g=None)
    I.news, I.user = rng.integers(-2, 3, (V, N)).astype(f32), rng.integers(-2, 3, (U, N)).astype(f32)
    I.news[0] = 3e37
    if c.hand == 2:
        I.group = np.zeros(V, i32)
    elif c.hand == 3:
        I.group = np.array([-1, 0, 0, 0, 1, 1, 1], i32)
    elif c.hand == 1:
        I.group = rng.integers(-1, 4, V).astype(i32)
        I.group[rng.permutation(V)[:k + 8]] = -1
        I.group[5] = 3                                                        # the key-0 news (a NaN row) belongs to the bin that closes last
    else:
        I.group = rng.integers(-2, G + 2, V).astype(i32)                      # negative: no group; >= n_groups counts as no group
    if c.pool in (1, 2):
        I.prior = (rng.integers(-32, 33, V) / 4.0).astype(f32)
        I.prior[3::7] = -INF
    if c.pool in (1, 3):
        lo = rng.integers(0, 4, U)
        I.stamp, I.window = rng.integers(0, 10, V).astype(i32), np.stack([lo, lo + rng.integers(3, 7, U)], axis=1).astype(i32)
    I.row_ids = np.stack([rng.permutation(np.arange(-1, max(V + 1, k)))[:k] if k <= V + 2 else rng.integers(-1, V + 1, k) for _ in range(U)]).astype(i32)
    if c.hand == 3:
        I.row_ids = np.stack([rng.permutation(np.arange(1, V)) for _ in range(U)]).astype(i32)
    elif c.hand == 2:                                                         # the even users: k live entries of the one group, no fill, no repeat
        I.row_ids[::2] = np.stack([rng.permutation(np.setdiff1d(np.arange(1, V), [5]))[:k] for _ in range((U + 1) // 2)]).astype(i32)
        I.news[5] = NAN
    else:
        if k >= 2:
            I.row_ids[::2, 1] = I.row_ids[::2, 0]                              # a repeated id is two entries
        I.news[5] = NAN                                                        # a NaN score: a key of 0
        if k >= 3:
            I.row_ids[::3, k // 2] = 5
    if c.hand == 1:
        if I.prior is not None:
            I.prior[:] = np.where(np.isneginf(I.prior), f32(0), I.prior)
        if I.stamp is not None:
            I.window[0] = (0, 9)
        I.row_ids[0] = hand_row(c, I.group, rng)
    I.base_max = (4.0 * rng.standard_normal((U, G + 1))).astype(f32)
    I.base_logsum = (3.0 * np.abs(rng.standard_normal((U, G + 1)))).astype(f32)
    gone = (rng.random((U, G + 1)) < 0.5) & (np.arange(U) % 4 == 3)[:, None]   # bins the row emptied
    if c.hand == 3:
        gone[:] = True
    I.base_max[gone], I.base_logsum[gone] = -INF, -INF
    if c.taus:
        I.tau_u = np.array([0.3, 1.7, 0.75], f32)[rng.integers(0, 3, U)]
        if U >= 15:
            I.tau_u[5], I.tau_u[9] = 0.0, NAN                                  # NaN for every real entry of K16; zeros in K21
            I.base_max[11, G] = NAN                                            # a NaN base in the bin that never closes: K21 all zeros, every live step of K16 NaN
            I.row_ids[13] = np.resize(np.array([0, 5, -2, V + 1, 5], i32), k)  # fill and key-0 entries only: a row without a live step, all zeros in K21
    if c.g:
        I.g = rng.standard_normal((U, k)).astype(f32)                          # mixed signs
    return I


def _row_kw(c, I):
    grp = np.where(I.group >= c.G, -1, I.group)                                # an id >= n_groups counts as no group
    return dict(row_ids=I.row_ids, temperature=I.tau_u.astype(f64) if I.tau_u is not None else float(f32(I.tau)), bases=(I.base_logsum.astype(f64), I.base_max.astype(f64)),
                group=grp, group_cap=c.cap, n_groups=c.G, prior=I.prior, stamp=I.stamp, window=I.window)


def row_reference(c, I):
    """metrics.capped_row_logprob_reference and capped_row_logprob_grad_reference with g and with |g|, in float64 on the fp32 inputs."""
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    kw = _row_kw(c, I)
    R = SimpleNamespace()
    with np.errstate(all="ignore"):
        R.logp, R.total = metrics.capped_row_logprob_reference(n64, u64, **kw)
        g = I.g.astype(f64) if I.g is not None else np.ones((c.U, c.k))
        R.omega, R.c = metrics.capped_row_logprob_grad_reference(n64, u64, g=g, **kw)
        R.omega_abs, c_abs = metrics.capped_row_logprob_grad_reference(n64, u64, g=np.abs(g), **kw)
    real = (I.row_ids >= 1) & (I.row_ids < c.V)
    R.real, R.step, R.blocked = real, real & np.isfinite(R.logp), real & np.isneginf(R.logp)
    R.c_abs = np.where(R.step, 2.0 * np.abs(g) - c_abs, np.where(R.blocked, -c_abs, 0.0))         # |g_i| + w_i sum |g_j| / D_j; blocked: without |g_i|
    for u in np.flatnonzero(np.isnan(I.base_max[:, c.G])):                   # a NaN base in the bin that never closes is a term of every D_j: K16 answers
        R.logp[u, R.step[u]] = NAN                                            # NaN at every live step (metrics.py reads a NaN maximum as an empty bin)
        R.total[u] = NAN if R.step[u].any() else R.total[u]
    return R


def row_facts(c, I):
    """(some entry is blocked, some bin closes at place 127), from the reference."""
    n64, u64 = I.news.astype(f64), I.user.astype(f64)
    with np.errstate(all="ignore"):
        logp, _ = metrics.capped_row_logprob_reference(n64, u64, **_row_kw(c, I))
    grp = np.where((I.group >= c.G) | (I.group < 0), c.G, I.group)
    close = False
    if c.k == 128:
        for u in range(c.U):
            live = np.isfinite(logp[u]) & (I.row_ids[u] >= 1) & (I.row_ids[u] < c.V)
            if live[127]:
                b = grp[I.row_ids[u, 127]]
                close |= bool(b < c.G and (grp[I.row_ids[u][live]] == b).sum() == c.cap)
    return bool(np.isneginf(logp).any()), close


def row_problem(entry, c, I, dev, variant="pad"):
    sh = variant == "shift"
    N, k, U, V, G = c.N, c.k, c.U, c.V, c.G
    o = (N, N + 4, tk_npad(N) + 8)
    S = SimpleNamespace(news=N, user=N, ids=k, g=k, win=2, base=G + 1) if variant == "dense" else SimpleNamespace(
        news=o[c.pad], user=o[(c.pad + 1) % 3], ids=k + (1 if c.pad != 1 else 0), g=k + (5 if c.pad != 2 else 0), win=5 if c.pad != 0 else 2, base=G + 1 + (3 if c.pad != 0 else 0))
    fo, io = (0 if sh else 4), (2 if sh else 1)
    P = SimpleNamespace(entry=entry, c=c, I=I, S=S, inb={}, outb={}, ws=None)
    P.inb["news"], P.inb["user"] = in_buf(I.news, S.news, dev, fo, NAN), in_buf(I.user, S.user, dev, fo, NAN)
    P.inb["group"] = in_buf(I.group, V, dev, io)
    if I.prior is not None:
        P.inb["prior"] = in_buf(I.prior, V, dev, io)
    if I.stamp is not None:
        P.inb["stamp"] = in_buf(I.stamp, V, dev, io)
        P.inb["window"] = in_buf(I.window, S.win, dev, io, np.tile(np.array([100, -100, 100], i32), (U, 1)))
    if I.tau_u is not None:
        P.inb["tau_u"] = in_buf(I.tau_u, U, dev, io)
    P.inb["row_ids"] = in_buf(I.row_ids, S.ids, dev, io, 1)                    # slack: a valid id
    P.inb["base_max"], P.inb["base_logsum"] = in_buf(I.base_max, S.base, dev, io, NAN), in_buf(I.base_logsum, S.base, dev, io, NAN)
    if entry == "logpc":
        P.outb["logp"] = out_buf(U, k, k, torch.float32, dev, io)
        if c.total:
            P.outb["total"] = out_buf(1, U, U, torch.float32, dev, io)
    else:
        if I.g is not None:
            P.inb["g"] = in_buf(I.g, S.g, dev, io, 1e30)                       # slack: a huge g
        P.outb["bin_w"], P.outb["sub_w"] = out_buf(U, G + 1, S.base, torch.float32, dev, io), out_buf(U, k, k, torch.float32, dev, io)
    if not sh:
        assert P.inb["news"].ptr % 32 == 16 and P.inb["user"].ptr % 32 == 16 and P.inb["row_ids"].ptr % 8 == 4 and P.inb["base_max"].ptr % 8 == 4
    return P


def row_check(c, I, out, R):
    w = {}
    lp = out["logpc"]["logp"]
    need(bool((lp[~R.real] == 0).all()), "exact", "out_logp: a fill entry must be 0")
    need(np.array_equal(np.isnan(lp), np.isnan(R.logp)), "exact", "out_logp: NaN at {} entries, the contract says {}", int(np.isnan(lp).sum()), int(np.isnan(R.logp).sum()))
    need(np.array_equal(np.isneginf(lp), np.isneginf(R.logp)), "exact", "out_logp: -inf at {} entries, the contract says {} (the blocked ones)", int(np.isneginf(lp).sum()),
         int(np.isneginf(R.logp).sum()))
    ok = np.isfinite(R.logp)
    ref = np.where(ok, R.logp, 0.0)
    everyone = np.ones(c.U, bool)
    w["logp"] = _ratio("tight", "out_logp", np.where(ok, lp, 0.0), ref, EPS * np.abs(ref) + ROW_F64 * (1.0 + np.abs(ref)) + 2.0 ** -149, everyone)
    for u in np.flatnonzero(np.isneginf(I.base_max).all(axis=1)):            # a row that takes everything eligible ends in 0
        live = np.flatnonzero(R.step[u])
        taken = not R.blocked[u].any()
        need(not len(live) or not taken or lp[u, live[-1]] == 0.0, "exact", "user {}: the last live place of a row over empty bases must be 0 exactly", u)
    if "total" in out["logpc"]:
        tot = out["logpc"]["total"][0]
        need(np.array_equal(np.isnan(tot), np.isnan(R.total)), "exact", "out_total: NaN where the reference has none, or the reverse")
        need(bool(np.isneginf(tot[R.blocked.any(axis=1) & ~np.isnan(R.total)]).all()), "exact", "out_total: must be -inf beside a blocked entry")
        fin = np.isfinite(R.total)
        tb = EPS * np.abs(np.where(fin, R.total, 0.0)) + ROW_F64 * (1.0 + np.abs(ref)).sum(axis=1) + 2.0 ** -149
        w["total"] = _ratio("tight", "out_total", tot, R.total, tb, ~np.isnan(R.total))
    om, cc = out["logpcg"]["bin_w"], out["logpcg"]["sub_w"]
    need(not np.isnan(om).any() and not np.isnan(cc).any(), "exact", "K21 never answers NaN (and writes bins 0 .. n_groups, every entry)")
    need(bool((cc[~(R.step | R.blocked)] == 0).all()), "exact", "out_sub_w: an entry that is neither a step nor blocked must be 0")
    need(bool((om[np.isneginf(I.base_max)] == 0).all()), "exact", "out_bin_w: an empty bin must give 0")
    w["omega"] = _ratio("tight", "out_bin_w", om, R.omega, EPS * np.abs(R.omega) + ROW_F64 * R.omega_abs + 2.0 ** -149, everyone)
    w["c"] = _ratio("tight", "out_sub_w", cc, R.c, EPS * np.abs(R.c) + ROW_F64 * R.c_abs + 2.0 ** -149, everyone)
    return w


def row_reference_identity(R):
    """sum_b omega_b = sum_i c_i in exact arithmetic: the worst |difference| over the absolute sums, a guard of the reference."""
    scale = R.omega_abs.sum(axis=1) + R.c_abs.sum(axis=1) + 1e-300
    return float((np.abs(R.omega.sum(axis=1) - R.c.sum(axis=1)) / scale).max())


def row_sweep(c, dev, call, layout=True):
    I = row_inputs(c)
    R = row_reference(c, I)
    entries = ("logpc", "logpcg")
    out = {e: execute(lambda: row_problem(e, c, I, dev), call) for e in entries}
    w = row_check(c, I, out, R)
    # `agree`: a user's outputs when the other users of its workgroup are replaced (and, with bad temperatures, taken away)
    keep = np.array([u for u in range(c.U) if not (I.tau_u is not None and c.U >= 15 and u in (5, 9))])
    I2 = SimpleNamespace(**vars(I))
    for k in ("user", "window", "tau_u", "row_ids", "base_max", "base_logsum", "g"):
        if getattr(I, k) is not None:
            setattr(I2, k, getattr(I, k)[keep][::-1].copy())
    for e in entries:
        other = execute(lambda: row_problem(e, c._replace(U=len(keep)), I2, dev), call, twice=False)
        for k in out[e]:
            x = out[e][k][:, keep][:, ::-1] if k == "total" else out[e][k][keep][::-1]
            same_bits("agree", f"{e} {k} of every user when the users of its workgroup are replaced", x, other[k])
    if layout:
        for variant in ("dense", "shift"):
            for e in entries:
                other = execute(lambda: row_problem(e, c, I, dev, variant), call, twice=False)
                for k in out[e]:
                    same_bits("layout", f"{e} {k} with {variant} buffers", other[k], out[e][k])
    return w


H = sys.modules[__name__]          # the tests below (and the host file) address the part above as H


# ------------------------------------------------------------------------------------------ the GPU tests
def _p(P, name):
    b = P.inb.get(name) or P.outb.get(name)
    return b.ptr if b is not None else None


def descriptor(P, ptr=_p, N=None):
    """(descriptor, size query, call) of P's stream entry point; `ptr` turns a buffer name into an address."""
    c, I, T, S, L = P.c, P.I, P.T, P.S, _lib.lib()
    shared = dict(news_vecs=ptr(P, "news"), ld_news=S.news, V=T.V, user=ptr(P, "user"), ld_user=S.user, U=c.U, N=c.N if N is None else N, excl_offsets=ptr(P, "offsets"),
                  n_excl=P.inb["xids"].cols if "xids" in P.inb else 0, tau=float(I.tau), tau_u=ptr(P, "tau_u"), order=ptr(P, "order"), n_pos=T.n_pos, n_groups=T.G,
                  ws=P.ws.ptr, ws_bytes=P.ws_bytes, prior=ptr(P, "prior"), stamp=ptr(P, "stamp"), window=ptr(P, "window"), ld_window=S.win if I.stamp is not None else 0)
    if P.entry == "newsg":
        d = _lib.ExpectNewsGroupsDesc(splits=c.vs, excl_users=ptr(P, "xids"), bin_start=ptr(P, "bin_start"), base_max=ptr(P, "base_max"), base_logsum=ptr(P, "base_logsum"),
                                      bin_w=ptr(P, "bin_w"), ld_bin=S.bin, scale_inv_tau=int("s" in c.opt), named_offsets=ptr(P, "n_off"), named_user=ptr(P, "n_user"),
                                      named_w=ptr(P, "n_w"), n_named=len(I.n_user) if I.n_user is not None else 0, out=ptr(P, "out"), ld_out=S.out, out_mass=ptr(P, "mass"), **shared)
        return d, L.nr_score_expect_news_groups_workspace_bytes, L.nr_score_expect_news_groups
    shared.update(splits=c.splits, excl_ids=ptr(P, "xids"), seg_start=ptr(P, "seg_start"), nseg=T.nseg, bin_seg=ptr(P, "bin_seg"))
    if P.entry == "logzg":
        return (_lib.LogzGroupsDesc(out_logsum=ptr(P, "logsum"), out_max=ptr(P, "max"), out_count=ptr(P, "count"), **shared), L.nr_score_logz_groups_workspace_bytes,
                L.nr_score_logz_groups)
    d = _lib.ExpectGroupsDesc(base_max=ptr(P, "base_max"), base_logsum=ptr(P, "base_logsum"), bin_w=ptr(P, "bin_w"), ld_base=S.base, sub_ids=ptr(P, "sub_ids"),
                              sub_w=ptr(P, "sub_w"), ld_sub=S.sub if c.T else 0, T=c.T, scale_inv_tau=int("s" in c.opt), out=ptr(P, "out"), ld_out=S.out,
                              out_mass=ptr(P, "mass"), **shared)
    return d, L.nr_score_expect_groups_workspace_bytes, L.nr_score_expect_groups


def row_descriptor(P, N=None):
    c, I, S, L = P.c, P.I, P.S, _lib.lib()
    shared = dict(news_vecs=_p(P, "news"), ld_news=S.news, V=c.V, user=_p(P, "user"), ld_user=S.user, U=c.U, N=c.N if N is None else N, k=c.k, row_ids=_p(P, "row_ids"),
                  ld_ids=S.ids, group=_p(P, "group"), group_cap=c.cap, n_groups=c.G, tau=float(I.tau), tau_u=_p(P, "tau_u"), base_max=_p(P, "base_max"),
                  base_logsum=_p(P, "base_logsum"), ld_base=S.base, prior=_p(P, "prior"), stamp=_p(P, "stamp"), window=_p(P, "window"),
                  ld_window=S.win if I.stamp is not None else 0)
    if P.entry == "logpc":
        return _lib.LogprobCappedDesc(out_logp=_p(P, "logp"), out_total=_p(P, "total"), **shared), None, L.nr_row_logprob_capped
    return (_lib.LogprobCappedGradDesc(g=_p(P, "g"), ld_g=S.g if I.g is not None else 0, out_bin_w=_p(P, "bin_w"), out_sub_w=_p(P, "sub_w"), **shared), None,
            L.nr_row_logprob_capped_grad)


def _call(P):
    """One call of the C ABI on the buffers of P; a size query must answer the restated carve (`wsize`)."""
    d, query, fn = row_descriptor(P) if P.entry in ("logpc", "logpcg") else descriptor(P)
    if query is not None:
        got = query(C.byref(d))
        need(got == P.ws_bytes, "wsize", "{}: the size query answers {}, the restated carve {} ({})", P.entry, got, P.ws_bytes, _lib.last_error())
    _lib.check(fn(C.byref(d), ops._stream()), "capped " + P.entry)
    torch.cuda.synchronize()


def _logz13(c, I, T):
    """(out_max, out_count) of nr_score_logz under the same pools and lists (the lists in id space), through the uncapped sweep."""
    sc = SW.SmCase(c.name, c.kind, c.N, c.U, T.V, 0, c.pool, int(bool(c.csr)), c.taus, 0, 0, "", c.pad)
    I13 = SimpleNamespace(**vars(I))
    I13.offsets = I13.xids = None
    if I.segs is not None:
        real = [np.unique(s[(s >= 1) & (s < T.V)]).astype(i32) for s in I.segs]
        I13.xids = np.concatenate(real + [np.array([T.V + 1], i32)]).astype(i32)
        I13.offsets = np.concatenate([[0], np.cumsum([len(s) for s in real])]).astype(i32)
    lz = SW.execute("logz", sc, I13, DEV, SW._call, twice=False)
    return lz["max"][0], lz["count"][0]


def _labels_of(c, T):
    out = []
    for e, name in (("logzg", "logzg_stream"), ("expectg", "expect_groups_stream")):
        p = plan(e, c, T)
        out.append(f"{name}[U={c.U},V={T.V},N={c.N},TU={p.TU},splits={p.splits},nseg={T.nseg},pos={T.n_pos}]")
    p = plan("newsg", c, T)
    out.append(f"expect_news_groups_stream[V={T.V},U={c.U},N={c.N},TV={p.TU},splits={p.splits},seg={p.seg},pos={T.n_pos},pool={int(bool(c.pool))},lists={int(bool(c.csr))}]")
    return out


@pytest.mark.parametrize("c", H.cap_cases(), ids=lambda c: c.name)
def test_capped_stream_calls(c):
    w, labels = CS._labelled(lambda: H.cap_sweep(c, DEV, _call, logz=_logz13))
    T = H.tables(c)
    for want in _labels_of(H.resolve(c, T), T):
        assert want in labels, (want, sorted(labels))
    print(f"\nCAPPED {c.name} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(w.items())))


@pytest.mark.parametrize("c", H.row_cases(), ids=lambda c: c.name)
def test_capped_row_calls(c):
    w, labels = CS._labelled(lambda: H.row_sweep(c, DEV, _call))
    for name in ("logp_capped", "logp_capped_grad"):
        want = f"{name}[U={c.U},N={c.N},k={c.k},cap={c.cap},G={c.G}]"
        assert want in labels, (want, sorted(labels))
    print(f"\nCAPPED {c.name} " + " ".join(f"{k}={v:.3g}" for k, v in sorted(w.items())))


def test_the_row_calls_on_the_bases_k15_returned():
    """K16 and K21 on K15's own bases, formed with the row's ids merged into the lists: the reference is given the same fp32
    bases, so the lattice bound holds as it does for host-made ones."""
    sc = next(x for x in H.cap_cases() if x.name == "gauss-one-group")
    T = H.tables(sc)
    sc = H.resolve(sc, T)
    c = RowCase("rows-on-k15", sc.N, sc.U, T.V, 65, 2, T.G, 0, 0, 1, 1, 1, 0)
    I = H.row_inputs(c)
    I.group = T.group
    Is = SimpleNamespace(prior=None, stamp=None, window=None, tau=I.tau, tau_u=None, news=I.news, user=I.user, omega=None,
                         segs=[np.unique(r[(r >= 1) & (r < T.V)]).astype(i32) for r in I.row_ids])
    lz = H.execute(lambda: H.problem("logzg", sc._replace(pool=0, taus=0, csr=1), Is, T, DEV), _call, twice=False)
    I.base_max, I.base_logsum = lz["max"], lz["logsum"]
    R = H.row_reference(c, I)
    out = {e: H.execute(lambda: H.row_problem(e, c, I, DEV), _call) for e in ("logpc", "logpcg")}
    w = H.row_check(c, I, out, R)
    assert R.blocked.any() and R.step.any()
    print("\nCAPPED rows-on-k15 " + " ".join(f"{k}={v:.3g}" for k, v in sorted(w.items())))


@pytest.mark.parametrize("N,U,V,splits", [(36, 130, 200, 2), (832, 9, 150, 0), (4, 257, 130, 3)], ids=str)
def test_one_bin_holding_every_news_is_k18_bit_for_bit(N, U, V, splits):
    """K22 with every news in group 0, omega = weight and K13's base in that bin's row against nr_score_expect_news (K18), both at
    padded strides: rows and mass bit for bit.  Prior only and a scalar temperature: every user is live, so the two gates of the
    named terms (K18: the user's base; K22: the user alone) agree."""
    nc = SW.NewsCase("one-bin", "gauss", N, V, U, splits, 2, 1, 0, 1, "wsM", 1)
    nc = nc._replace(splits=min(nc.splits, lz_plan_tile(V, U + 1, 64, 1).nseg))
    I = SW.news_inputs(nc)
    assert not I.special and I.weight is not None and I.segs is not None and I.n_off is not None
    base = SW.news_base(nc, I, DEV, SW._call)
    k18 = SW.news_execute("news", nc, I, DEV, SW._news_call, base, "pad", twice=False)
    group = np.zeros(V, i32)
    T = H.group_tables(group, 1)
    T.group = group
    c = CapCase("one-bin", "gauss", N, U, "", 0, nc.splits, 2, 1, 0, 0, 1, "sM", 2)
    bm, bl = np.full((U, 2), -INF, f32), np.full((U, 2), -INF, f32)
    bm[:, 0], bl[:, 0] = base
    I22 = SimpleNamespace(news=I.news, user=I.user, prior=I.prior, stamp=None, window=None, segs=I.segs, tau=I.tau, tau_u=None, sub_ids=None, sub_w=None,
                          omega=np.stack([I.weight, np.zeros(U, f32)], axis=1), n_off=I.n_off, n_user=I.n_user, n_w=I.n_w)
    k22 = H.execute(lambda: H.problem("newsg", c, I22, T, DEV, "pad", (bm, bl)), _call, twice=False)
    H.same_bits("agree", "rows of K22 with one bin against K18", k22["out"], k18["out"])
    H.same_bits("agree", "mass of K22 with one bin against K18", k22["mass"], k18["mass"])


@pytest.mark.parametrize("N", sorted(H.REFUSED_NS), ids=str)
def test_a_width_that_is_no_multiple_of_four_is_refused_before_any_launch(N):
    sc = next(x for x in H.cap_cases() if x.name == f"gauss-N{H.REFUSED_NS[N]}")
    T = H.tables(sc)
    sc = H.resolve(sc, T)
    I = H.cap_inputs(sc, T)
    base = (np.zeros((sc.U, T.G + 1), f32), np.zeros((sc.U, T.G + 1), f32))
    rc_ = next(x for x in H.row_cases() if x.name == "rows-k64-0")
    Ir = H.row_inputs(rc_)
    todo = [(e, H.problem(e, sc, I, T, DEV, "pad", base)) for e in STREAM] + [(e, H.row_problem(e, rc_, Ir, DEV)) for e in ("logpc", "logpcg")]
    for e, P in todo:
        d, query, fn = row_descriptor(P, N) if e in ("logpc", "logpcg") else descriptor(P, N=N)
        (size, rc), labels = CS._labelled(lambda: (query(C.byref(d)) if query is not None else 0, fn(C.byref(d), ops._stream())))
        assert size == 0 and rc != 0 and "multiple of 4" in _lib.last_error(), (e, size, rc, _lib.last_error())
        assert not labels, labels
        for name, b in H.all_bufs(P):
            assert torch.equal(_bits(b.flat), _bits(b.init)), (e, name)

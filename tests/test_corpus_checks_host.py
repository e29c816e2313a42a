"""CPU: the refusals and the plans the full-corpus calls share (csrc/nr_score_tile.h, host section), pinned to what the library
answered while every call still carried its own copy of them.  REFUSED holds the whole text of nr_last_error for every shared
rule of nr_score_topk, nr_score_sample, nr_score_rank, nr_score_logz (size query and call) and nr_row_logprob, and for
descriptors that break two rules at once (the first refusal is the one a caller has always seen); PLANS holds the three
*_workspace_bytes answers on a grid that crosses every branch of the user-tile and slice arithmetic.  All of it is decided
before any launch (fake non-null pointers: a launch would fault, a refusal does not).  Both tables were recorded from the
library of the commit before the checks were shared, with this file's own descriptors, and are compared for equality."""
import ctypes as C

import pytest

from newsrecommendation_amd import _lib

P = 4096                                                               # a fake pointer, 16-byte aligned
VEC = dict(news_vecs=P, ld_news=400, V=100001, user=P, ld_user=400, U=8192, N=400)
BASE = {
    "score_topk": dict(VEC, k=10, out_ids=P, out_scores=P),
    "score_sample": dict(VEC, k=10, out_ids=P, out_scores=P),
    "score_rank": dict(VEC, T=4, targets=P, ld_targets=4, out_ranks=P, out_scores=P),
    "score_logz": dict(VEC, tau=0.5, out_logsum=P, out_max=P, out_count=P),
    "row_logprob": dict(VEC, k=10, row_ids=P, ld_ids=10, sequential=1, tau=0.5, base_max=P, base_logsum=P, out_logp=P),
}
DESC = {"score_topk": _lib.TopkDesc, "score_rank": _lib.RankDesc, "score_logz": _lib.LogzDesc, "row_logprob": _lib.LogprobDesc}
NULL_OUT = {"score_topk": "out_ids", "score_sample": "out_ids", "score_rank": "out_ranks", "score_logz": "out_max", "row_logprob": "out_logp"}

# rule -> the fields it changes; CALL_ONLY rules are checked by the call alone (with a workspace of the size the query asks for)
RULES = {
    "V=1": dict(V=1),
    "U=0": dict(U=0),
    "N=6": dict(N=6),
    "N=1028": dict(N=1028),
    "stamp-alone": dict(stamp=P),
    "window-alone": dict(window=P, ld_window=2),
    "ld_window=1": dict(stamp=P, window=P, ld_window=1),
    "ids-alone": dict(excl_ids=P, n_excl=5),
    "offsets-alone": dict(excl_offsets=P, n_excl=5),
    "E-with-offsets": dict(exclude=P, ld_exclude=3, E=3, excl_offsets=P, excl_ids=P, n_excl=5),
    "ld_news=N+1": dict(ld_news=401),
    "user-misaligned": dict(user=P + 4),
    "null-output": None,                                               # NULL_OUT[call] = None
    "short-workspace": None,                                           # ws_bytes = need - 8
    # two rules at once: the first in the call's own order wins
    "V=1+N=6": dict(V=1, N=6),
    "offsets-alone+stamp-alone": dict(excl_offsets=P, n_excl=5, stamp=P),
    "ld_news=N+1+short-workspace": dict(ld_news=401),
}
CALL_ONLY = ("ld_news=N+1", "user-misaligned", "null-output", "short-workspace", "ld_news=N+1+short-workspace")
NO_LISTS = ("ids-alone", "offsets-alone", "E-with-offsets", "offsets-alone+stamp-alone")
NO_WORKSPACE = ("short-workspace", "ld_news=N+1+short-workspace")


def rules_of(call):
    skip = {"score_logz": ("E-with-offsets",), "row_logprob": NO_LISTS + NO_WORKSPACE}.get(call, ())
    return [r for r in RULES if r not in skip]


def _descriptor(call, fields):
    if call == "score_sample":
        return _lib.SampleDesc(topk=_lib.TopkDesc(**fields), seed=1, draw=0, tau=0.5)
    return DESC[call](**fields)


def _workspace(d):
    return d.topk if isinstance(d, _lib.SampleDesc) else d


def refusal(call, rule):
    """[answer of the size query, nr_last_error after it,] return code of the call, nr_last_error after it, for `rule` broken in
    `call`; a rule of CALL_ONLY, and every rule of nr_row_logprob, which has no size query, gives the last two alone."""
    lib = _lib.lib()
    query = getattr(lib, f"nr_{call}_workspace_bytes", None)
    fields = dict(BASE[call], **(RULES[rule] or {}))
    if rule == "null-output":
        fields[NULL_OUT[call]] = None
    out = []
    if query is not None and rule not in CALL_ONLY:
        out += [query(C.byref(_descriptor(call, fields))), _lib.last_error()]
    d = _descriptor(call, fields)
    if query is not None:
        need = query(C.byref(_descriptor(call, BASE[call])))           # of the unbroken descriptor: the broken one may be refused
        _workspace(d).ws, _workspace(d).ws_bytes = P, need - 8 if rule in NO_WORKSPACE else need
    out += [getattr(lib, f"nr_{call}")(C.byref(d), None), _lib.last_error()]
    return out


# recorded: [size query's answer, its nr_last_error,] the call's return code, its nr_last_error
REFUSED = {
    ('score_topk', 'V=1'): [0, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_topk', 'U=0'): [0, 'score_topk: U = 0 users',
        1, 'score_topk: U = 0 users'],
    ('score_topk', 'N=6'): [0, 'score_topk: vector width N = 6 must be a multiple of 4 in [4, 1024]',
        1, 'score_topk: vector width N = 6 must be a multiple of 4 in [4, 1024]'],
    ('score_topk', 'N=1028'): [0, 'score_topk: vector width N = 1028 must be a multiple of 4 in [4, 1024]',
        1, 'score_topk: vector width N = 1028 must be a multiple of 4 in [4, 1024]'],
    ('score_topk', 'stamp-alone'): [0, 'score_topk: stamp given without window (the two come together)',
        1, 'score_topk: stamp given without window (the two come together)'],
    ('score_topk', 'window-alone'): [0, 'score_topk: window given without stamp (the two come together)',
        1, 'score_topk: window given without stamp (the two come together)'],
    ('score_topk', 'ld_window=1'): [0, 'score_topk: ld_window = 1, a window row is (lo, hi): at least 2',
        1, 'score_topk: ld_window = 1, a window row is (lo, hi): at least 2'],
    ('score_topk', 'ids-alone'): [0, 'score_topk: excl_ids given without excl_offsets (n_excl = 5; the two come together)',
        1, 'score_topk: excl_ids given without excl_offsets (n_excl = 5; the two come together)'],
    ('score_topk', 'offsets-alone'): [0, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_topk', 'E-with-offsets'): [0, 'score_topk: the dense list (E = 3) and the CSR lists (excl_offsets) are not combined: one list form per call',
        1, 'score_topk: the dense list (E = 3) and the CSR lists (excl_offsets) are not combined: one list form per call'],
    ('score_topk', 'ld_news=N+1'): [1, 'score_topk: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_topk', 'user-misaligned'): [1, 'score_topk: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_topk', 'null-output'): [1, 'score_topk: null pointer (news_vecs, user, out_ids, out_scores)'],
    ('score_topk', 'short-workspace'): [1, 'score_topk: workspace holds 1310712 bytes, nr_score_topk_workspace_bytes asks for 1310720 (8-byte aligned)'],
    ('score_topk', 'V=1+N=6'): [0, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_topk', 'offsets-alone+stamp-alone'): [0, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_topk', 'ld_news=N+1+short-workspace'): [1, 'score_topk: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_sample', 'V=1'): [0, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_sample', 'U=0'): [0, 'score_topk: U = 0 users',
        1, 'score_topk: U = 0 users'],
    ('score_sample', 'N=6'): [0, 'score_topk: vector width N = 6 must be a multiple of 4 in [4, 1024]',
        1, 'score_topk: vector width N = 6 must be a multiple of 4 in [4, 1024]'],
    ('score_sample', 'N=1028'): [0, 'score_topk: vector width N = 1028 must be a multiple of 4 in [4, 1024]',
        1, 'score_topk: vector width N = 1028 must be a multiple of 4 in [4, 1024]'],
    ('score_sample', 'stamp-alone'): [0, 'score_topk: stamp given without window (the two come together)',
        1, 'score_topk: stamp given without window (the two come together)'],
    ('score_sample', 'window-alone'): [0, 'score_topk: window given without stamp (the two come together)',
        1, 'score_topk: window given without stamp (the two come together)'],
    ('score_sample', 'ld_window=1'): [0, 'score_topk: ld_window = 1, a window row is (lo, hi): at least 2',
        1, 'score_topk: ld_window = 1, a window row is (lo, hi): at least 2'],
    ('score_sample', 'ids-alone'): [0, 'score_topk: excl_ids given without excl_offsets (n_excl = 5; the two come together)',
        1, 'score_topk: excl_ids given without excl_offsets (n_excl = 5; the two come together)'],
    ('score_sample', 'offsets-alone'): [0, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_sample', 'E-with-offsets'): [0, 'score_topk: the dense list (E = 3) and the CSR lists (excl_offsets) are not combined: one list form per call',
        1, 'score_topk: the dense list (E = 3) and the CSR lists (excl_offsets) are not combined: one list form per call'],
    ('score_sample', 'ld_news=N+1'): [1, 'score_topk: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_sample', 'user-misaligned'): [1, 'score_topk: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_sample', 'null-output'): [1, 'score_topk: null pointer (news_vecs, user, out_ids, out_scores)'],
    ('score_sample', 'short-workspace'): [1, 'score_topk: workspace holds 1310712 bytes, nr_score_topk_workspace_bytes asks for 1310720 (8-byte aligned)'],
    ('score_sample', 'V=1+N=6'): [0, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_topk: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_sample', 'offsets-alone+stamp-alone'): [0, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_topk: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_sample', 'ld_news=N+1+short-workspace'): [1, 'score_topk: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_rank', 'V=1'): [0, 'score_rank: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_rank: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_rank', 'U=0'): [0, 'score_rank: U = 0 users',
        1, 'score_rank: U = 0 users'],
    ('score_rank', 'N=6'): [0, 'score_rank: vector width N = 6 must be a multiple of 4 in [4, 1024]',
        1, 'score_rank: vector width N = 6 must be a multiple of 4 in [4, 1024]'],
    ('score_rank', 'N=1028'): [0, 'score_rank: vector width N = 1028 must be a multiple of 4 in [4, 1024]',
        1, 'score_rank: vector width N = 1028 must be a multiple of 4 in [4, 1024]'],
    ('score_rank', 'stamp-alone'): [0, 'score_rank: stamp given without window (the two come together)',
        1, 'score_rank: stamp given without window (the two come together)'],
    ('score_rank', 'window-alone'): [0, 'score_rank: window given without stamp (the two come together)',
        1, 'score_rank: window given without stamp (the two come together)'],
    ('score_rank', 'ld_window=1'): [0, 'score_rank: ld_window = 1, a window row is (lo, hi): at least 2',
        1, 'score_rank: ld_window = 1, a window row is (lo, hi): at least 2'],
    ('score_rank', 'ids-alone'): [0, 'score_rank: excl_ids given without excl_offsets (n_excl = 5; the two come together)',
        1, 'score_rank: excl_ids given without excl_offsets (n_excl = 5; the two come together)'],
    ('score_rank', 'offsets-alone'): [0, 'score_rank: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_rank: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_rank', 'E-with-offsets'): [0, 'score_rank: the dense list (E = 3) and the CSR lists (excl_offsets) are not combined: one list form per call',
        1, 'score_rank: the dense list (E = 3) and the CSR lists (excl_offsets) are not combined: one list form per call'],
    ('score_rank', 'ld_news=N+1'): [1, 'score_rank: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_rank', 'user-misaligned'): [1, 'score_rank: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_rank', 'null-output'): [1, 'score_rank: null pointer (news_vecs, user, targets, out_ranks, out_scores)'],
    ('score_rank', 'short-workspace'): [1, 'score_rank: workspace holds 950264 bytes, nr_score_rank_workspace_bytes asks for 950272 (8-byte aligned)'],
    ('score_rank', 'V=1+N=6'): [0, 'score_rank: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_rank: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_rank', 'offsets-alone+stamp-alone'): [0, 'score_rank: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_rank: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_rank', 'ld_news=N+1+short-workspace'): [1, 'score_rank: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_logz', 'V=1'): [0, 'score_logz: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_logz: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_logz', 'U=0'): [0, 'score_logz: U = 0 users',
        1, 'score_logz: U = 0 users'],
    ('score_logz', 'N=6'): [0, 'score_logz: vector width N = 6 must be a multiple of 4 in [4, 1024]',
        1, 'score_logz: vector width N = 6 must be a multiple of 4 in [4, 1024]'],
    ('score_logz', 'N=1028'): [0, 'score_logz: vector width N = 1028 must be a multiple of 4 in [4, 1024]',
        1, 'score_logz: vector width N = 1028 must be a multiple of 4 in [4, 1024]'],
    ('score_logz', 'stamp-alone'): [0, 'score_logz: stamp given without window (the two come together)',
        1, 'score_logz: stamp given without window (the two come together)'],
    ('score_logz', 'window-alone'): [0, 'score_logz: window given without stamp (the two come together)',
        1, 'score_logz: window given without stamp (the two come together)'],
    ('score_logz', 'ld_window=1'): [0, 'score_logz: ld_window = 1, a window row is (lo, hi): at least 2',
        1, 'score_logz: ld_window = 1, a window row is (lo, hi): at least 2'],
    ('score_logz', 'ids-alone'): [0, 'score_logz: excl_ids given without excl_offsets (n_excl = 5; the two come together)',
        1, 'score_logz: excl_ids given without excl_offsets (n_excl = 5; the two come together)'],
    ('score_logz', 'offsets-alone'): [0, 'score_logz: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_logz: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_logz', 'ld_news=N+1'): [1, 'score_logz: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_logz', 'user-misaligned'): [1, 'score_logz: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)'],
    ('score_logz', 'null-output'): [1, 'score_logz: null pointer (news_vecs, user, out_logsum, out_max, out_count)'],
    ('score_logz', 'short-workspace'): [1, 'score_logz: workspace holds 19267576 bytes, nr_score_logz_workspace_bytes asks for 19267584 (8-byte aligned)'],
    ('score_logz', 'V=1+N=6'): [0, 'score_logz: V = 1 news rows; row 0 is the padding news, so at least 2 are needed',
        1, 'score_logz: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('score_logz', 'offsets-alone+stamp-alone'): [0, 'score_logz: excl_offsets given without excl_ids (n_excl = 5; the two come together)',
        1, 'score_logz: excl_offsets given without excl_ids (n_excl = 5; the two come together)'],
    ('score_logz', 'ld_news=N+1+short-workspace'): [1, 'score_logz: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('row_logprob', 'V=1'): [1, 'row_logprob: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
    ('row_logprob', 'U=0'): [1, 'row_logprob: U = 0 users'],
    ('row_logprob', 'N=6'): [1, 'row_logprob: vector width N = 6 must be a multiple of 4 in [4, 1024]'],
    ('row_logprob', 'N=1028'): [1, 'row_logprob: vector width N = 1028 must be a multiple of 4 in [4, 1024]'],
    ('row_logprob', 'stamp-alone'): [1, 'row_logprob: stamp given without window (the two come together)'],
    ('row_logprob', 'window-alone'): [1, 'row_logprob: window given without stamp (the two come together)'],
    ('row_logprob', 'ld_window=1'): [1, 'row_logprob: ld_window = 1, a window row is (lo, hi): at least 2'],
    ('row_logprob', 'ld_news=N+1'): [1, 'row_logprob: rows must be 16-byte aligned (ld_news = 401, ld_user = 400: multiples of 4, >= N = 400)'],
    ('row_logprob', 'user-misaligned'): [1, 'row_logprob: rows must be 16-byte aligned (ld_news = 400, ld_user = 400: multiples of 4, >= N = 400)'],
    ('row_logprob', 'null-output'): [1, 'row_logprob: null pointer (news_vecs, user, row_ids, base_max, base_logsum, out_logp)'],
    ('row_logprob', 'V=1+N=6'): [1, 'row_logprob: V = 1 news rows; row 0 is the padding news, so at least 2 are needed'],
}


@pytest.mark.parametrize("call,rule", [(c, r) for c in BASE for r in rules_of(c)], ids=lambda v: v)
def test_shared_refusal_keeps_its_text(call, rule):
    assert refusal(call, rule) == REFUSED[call, rule]


def test_every_refusal_is_a_refusal():
    """The table itself: every entry refuses (size 0, code 1 = NR_ERR_ARG), names its call, and no rule of a call is missing."""
    assert sorted(REFUSED) == sorted((c, r) for c in BASE for r in rules_of(c))
    for (call, rule), got in REFUSED.items():
        said = "score_topk" if call == "score_sample" else call      # the sampled call runs nr_score_topk's checks
        assert got[-2] == 1 and got[-1].startswith(said + ": "), (call, rule)
        assert len(got) == 2 or (got[0] == 0 and got[1] == got[3]), (call, rule)


# (N, U, V, k, splits, n_groups): N 24 / 400 / 512 / 1024 give user tiles 64 / 64 / 32 / 16 (top-k with k = 128: 64 / 32 / 32 / 16); U
# 1 / 65 / 8192 / 70 000 leave the library's slice count to the chunk count or the merge limit, the chip, and 1; V = 2 and 130 are
# one and two chunks; n_groups 1 .. 512 reach one, two, four and eight blocks of 64 groups and the user tile they allow
GRID = ([(N, U, 100001, 128, 0, 0) for N in (24, 400, 512, 1024) for U in (1, 65, 8192, 70000)]
        + [(N, U, V, 1, 0, 0) for N in (24, 1024) for U in (1, 70000) for V in (2, 130)]
        + [(N, 65, V, k, 3, 0) for N in (400, 512) for V in (130, 100001) for k in (1, 128)]
        + [(N, U, 100001, 128, 0, G) for N, U in ((24, 8192), (512, 65), (1024, 1)) for G in (1, 65, 129, 257, 512)])


def plan_bytes(N, U, V, k, splits, G):
    """The three size queries for one grid point; the rank call has T = 4 targets, two cut-offs, and caps when G > 0."""
    lib = _lib.lib()
    vec = dict(news_vecs=P, ld_news=N, V=V, user=P, ld_user=N, U=U, N=N, splits=splits)
    ks = (C.c_int * 2)(5, 10)
    caps = dict(group=P, group_cap=2, n_groups=G) if G else {}
    return (lib.nr_score_topk_workspace_bytes(C.byref(_lib.TopkDesc(**vec, k=k))),
            lib.nr_score_rank_workspace_bytes(C.byref(_lib.RankDesc(**vec, T=4, ks=ks, n_ks=2, **caps))),
            lib.nr_score_logz_workspace_bytes(C.byref(_lib.LogzDesc(**vec, tau=0.5))))


# recorded: (nr_score_topk_workspace_bytes, nr_score_rank_workspace_bytes, nr_score_logz_workspace_bytes)
PLANS = {
    (24, 1, 100001, 128, 0, 0): (65536, 4212, 2352),
    (24, 65, 100001, 128, 0, 0): (4259840, 140660, 152880),
    (24, 8192, 100001, 128, 0, 0): (16777216, 1212416, 19267584),
    (24, 70000, 100001, 128, 0, 0): (71680000, 9240000, 164640000),
    (400, 1, 100001, 128, 0, 0): (65536, 4212, 2352),
    (400, 65, 100001, 128, 0, 0): (4259840, 140660, 152880),
    (400, 8192, 100001, 128, 0, 0): (8388608, 1212416, 19267584),
    (400, 70000, 100001, 128, 0, 0): (71680000, 9240000, 164640000),
    (512, 1, 100001, 128, 0, 0): (65536, 4212, 2352),
    (512, 65, 100001, 128, 0, 0): (4259840, 96980, 152880),
    (512, 8192, 100001, 128, 0, 0): (8388608, 1081344, 19267584),
    (512, 70000, 100001, 128, 0, 0): (71680000, 9240000, 164640000),
    (1024, 1, 100001, 128, 0, 0): (65536, 4212, 2352),
    (1024, 65, 100001, 128, 0, 0): (3461120, 61620, 152880),
    (1024, 8192, 100001, 128, 0, 0): (8388608, 1081344, 19267584),
    (1024, 70000, 100001, 128, 0, 0): (71680000, 9240000, 164640000),
    (24, 1, 2, 1, 0, 0): (8, 132, 16),
    (24, 1, 130, 1, 0, 0): (16, 148, 24),
    (24, 70000, 2, 1, 0, 0): (560000, 9240000, 840000),
    (24, 70000, 130, 1, 0, 0): (560000, 9240000, 1680000),
    (1024, 1, 2, 1, 0, 0): (8, 132, 16),
    (1024, 1, 130, 1, 0, 0): (16, 148, 24),
    (1024, 70000, 2, 1, 0, 0): (560000, 9240000, 840000),
    (1024, 70000, 130, 1, 0, 0): (560000, 9240000, 1680000),
    (400, 65, 130, 1, 3, 0): (1560, 10660, 0),
    (400, 65, 130, 128, 3, 0): (199680, 10660, 0),
    (400, 65, 100001, 1, 3, 0): (1560, 10660, 152880),
    (400, 65, 100001, 128, 3, 0): (199680, 10660, 152880),
    (512, 65, 130, 1, 3, 0): (1560, 10660, 0),
    (512, 65, 130, 128, 3, 0): (199680, 10660, 0),
    (512, 65, 100001, 1, 3, 0): (1560, 10660, 152880),
    (512, 65, 100001, 128, 3, 0): (199680, 10660, 152880),
    (24, 8192, 100001, 128, 0, 1): (16777216, 1618144, 19267584),
    (24, 8192, 100001, 128, 0, 65): (16777216, 10807520, 19267584),
    (24, 8192, 100001, 128, 0, 129): (16777216, 19865824, 19267584),
    (24, 8192, 100001, 128, 0, 257): (16777216, 38244576, 19267584),
    (24, 8192, 100001, 128, 0, 512): (16777216, 74858496, 19267584),
    (512, 65, 100001, 128, 0, 1): (4259840, 113864, 152880),
    (512, 65, 100001, 128, 0, 65): (4259840, 1061064, 152880),
    (512, 65, 100001, 128, 0, 129): (4259840, 2008264, 152880),
    (512, 65, 100001, 128, 0, 257): (4259840, 3752168, 152880),
    (512, 65, 100001, 128, 0, 512): (4259840, 7411928, 152880),
    (1024, 1, 100001, 128, 0, 1): (65536, 20648, 2352),
    (1024, 1, 100001, 128, 0, 65): (65536, 1070248, 2352),
    (1024, 1, 100001, 128, 0, 129): (65536, 2119848, 2352),
    (1024, 1, 100001, 128, 0, 257): (65536, 4219048, 2352),
    (1024, 1, 100001, 128, 0, 512): (65536, 8401048, 2352),
}


@pytest.mark.parametrize("point", GRID, ids=lambda p: "-".join(map(str, p)))
def test_workspace_queries_keep_their_plans(point):
    assert plan_bytes(*point) == PLANS[point]


def test_the_grid_reaches_every_plan():
    """Top-k's size is U * slices * k * 8 bytes, so the table itself shows every clamp of the library's slice count: the merge limit
    (8192 / k), the chip (256 / user tiles), the chunk count, 1, and a forced count; and the user tile top-k takes at k = 128."""
    assert len(GRID) == len(set(GRID)) == len(PLANS) == 47
    slices = {p: PLANS[p][0] // (p[1] * p[3] * 8) for p in GRID}
    assert slices[24, 1, 100001, 128, 0, 0] == slices[24, 65, 100001, 128, 0, 0] == 64               # 8192 / 128
    assert slices[1024, 65, 100001, 128, 0, 0] == 52                                                 # 256 / 5 tiles of 16 users
    assert slices[24, 8192, 100001, 128, 0, 0] == 2 and slices[400, 8192, 100001, 128, 0, 0] == 1    # tiles of 64 and of 32 users
    assert slices[24, 70000, 100001, 128, 0, 0] == 1
    assert slices[24, 1, 2, 1, 0, 0] == 1 and slices[24, 1, 130, 1, 0, 0] == 2                       # one and two chunks
    assert slices[400, 65, 100001, 1, 3, 0] == slices[512, 65, 130, 128, 3, 0] == 3
    assert all(PLANS[p][0] > 0 and PLANS[p][1] > 0 and (PLANS[p][2] > 0 or (p[2], p[4]) == (130, 3)) for p in GRID)   # 3 slices of 2 segments: refused

"""GPU: every route of the kernels either side of the encoder against fp64 or bit for bit: dense Adam (nr_adam_step,
nr_adam_step_packed), row-deferred Adam (nr_adam_rows), the ranking metrics (nr_eval_metrics), batch assembly
(nr_assemble_batch), nr_stack_rows and the index checks (nr_check_ids, nr_check_labels).  The case tables, one route function
per entry point (its dispatch restated), the input builders, the references, the drivers and the checker are the first part of
this file ("step sweep"; plain torch and numpy, no GPU needed); tests/test_step_sweep_host.py imports them and proves on the CPU
that the checker passes a sound stand-in (with and without fused multiply-adds) and fails each of nineteen subtly wrong ones.
The second part calls the C ABI directly.

Every output and in-place buffer is one allocation [guard][payload][guard] (glue_buf of the glue sweep).  Outputs start as NaN
(integers: -77), counters as small integers, slack columns and guards as the sentinel; after the call the sentinels are compared
bit for bit, and every call is made twice from the same start state (two problems built alike) and compared bit for bit.

Dense Adam, one step at a time: the reference is the header's formula in fp64 on the fp32 state the kernel started that step
from, so a chain of steps feeds each step the kernel's own previous output and the bound stays local.
  exact   beta1 = 0.5, beta2 = 0.75, eps = 0, lr = 2^-10, step 1, m = v = 0, g = k 2^-2 (1 <= |k| <= 7), grad_scale a power of
          two, p on the 2^-10 grid: m' = g'/2, v' = g'^2/4, sqrt(v')/0.5 = |g'|, p' = p - sign(g) 2^-10, all representable
          (asserted by the host file): p, m, v equal fp64 as numbers.  p is seeded so that p' lands on bf16 rounding ties.
  gauss   Gaussian state, gradients from 1e-6 to 1 within one buffer, eps = 1e-8, default betas, inside the bound below
  gzero   the same with g = 0 (the moments decay);  allzero  g = m = v = 0: p keeps every bit, m and v stay +0 (layer `still`:
          the fact the deferred kernel's shortcut rests on)
Bound (u = 2^-24, F = 2^-149 per rounding that can underflow; b1, b2, lr, eps, grad_scale are the fp32 values passed; ss and bc
are lr / (1 - b1^t) and sqrt(1 - b2^t) in fp64; primes are the fp64 results).  It holds with and without fused multiply-adds:
  e_g   = u |g'| + F                                              g' = g grad_scale, one product
  e_m   = (1-b1) e_g + 3 u (1-b1) |g' - m| + u |m'| + 3 F         the rounding of 1-b1, of g'-m, of the product (absent under
                                                                  fma), and the final one
  v'    relative 7 u (+ 4 F): the rounding of 1-b2, g' twice (2 u), two products, b2 v (absent under fma), the sum; every
        term is non-negative
  sqrt  relative 7u/2 from v' and u of sqrtf = 4.5 u; the underflow part of v' enters as min(sqrt(4F), 4F / (2 sqrt v'))
  e_den = (e_sqrt + 2 u sqrt v') / bc + u den + F                 the rounding of bc to fp32, the division, the sum with eps
  e_q   = (e_m / den + |q| e_den / den) (1 + 2^-20) + (1 + STEP_DIV_EXCESS) u |q| + F        q = m' / den: with m'(1 + a) over
          den (1 + b) the error is q (a - b) / (1 + b); the first-order part is the parenthesis, and 1 / (1 + b) with
          |b| = e_den / den <= 10 u < 2^-20.6 is what the factor 1 + 2^-20 absorbs
  e_p   = ss e_q + 3 u |ss q| + u |p'| + 2 F                      the rounding of ss to fp32, the product, the subtraction
Pack jobs: dst is bit-equal to torch's .to(bfloat16) of the new p; padding columns, guards and everything outside a job keep
every bit.  1, 2 and 4 jobs, first > 0, gaps, a job that ends at n - n % 4, cols 4 and 300, ld_dst in {cols, cols + 4, 320}.

Row-deferred Adam: bit for bit against the dense kernel (pinned above) over the whole table, after every catch-up on the rows
named and after the final flush on everything.  After every call the rows the call did not own keep every bit of p, g, m, v and
the packed copy, row_step changes on the owned rows only, sched on the filed step only (to the pair nr_adam_bias gives).

Metrics: the reference is written from the header: descending order with the later index first on ties, AUC as Mann-Whitney
with half credit and MRR in exact rational arithmetic, nDCG in fp64 with math.log2; a label != 0 is a positive of gain 1.
Per impression the bound is (c + 8) 2^-53 |value| (+ METRIC_LOG2_EXCESS for nDCG); skipped impressions are [-1, 0, 0, 0] bit for
bit; sums[0] is exact, sums[1..4] within (n_imp + 2) 2^-53 sum of math.fsum over the rows the kernel itself wrote.

Assembly, stacking and the index checks are bit for bit against numpy indexing with the list splice, torch.cat and numpy counts.

Layers of StepCheckError: sentinel, repeat, grad, still, exact, m, v, p, pack, rows, untouched, row_step, sched, skip, metric,
sums, assemble, bad, stack, flags, count.

Routes, derivations, measured figures and what stays uncovered: DESIGN.md "Adam, feed, metric and index-check kernels: routes
as verified and the sweep".
"""
import bisect
import collections
import ctypes as C
import math
import sys
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_gemm_sweep as G
import test_gpu_glue_sweep as GL
from test_gpu_glue_sweep import _bits, _count_routes, _equal64, _gen, _same, _sentinels, _within, glue_buf
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------ step sweep
U = G.GEMM_U
F149 = 2.0 ** -149
# What the device sqrtf and the two divisions of m / (sqrt(v) / bc + eps) add beyond the analytic bound, in units of u |q|: four
# times the worst excess measured over the sweep on the MI355X against fp64, 0 when there is none (DESIGN.md holds the figures).
STEP_DIV_EXCESS = 0.0
# The same for the device log2 of the nDCG terms, absolute.
METRIC_LOG2_EXCESS = 0.0
LAYERS = ("sentinel", "repeat", "grad", "still", "exact", "m", "v", "p", "pack", "rows", "untouched", "row_step", "sched", "skip", "metric",
          "sums", "assemble", "bad", "stack", "flags", "count")
NAN = float("nan")
IFILL = -77


class StepCheckError(AssertionError):
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
        raise StepCheckError(layer, str(e)) from None


def sent(name, b):
    _as("sentinel", _sentinels, name, b)


def same(layer, name, got, ref):
    _as(layer, _same, "exact", name, got, ref)


def eq64(layer, name, got, ref):
    _as(layer, _equal64, "exact", name, got, ref)


def within(layer, name, got, ref, bound):
    return _as(layer, _within, "exact", name, got, ref, bound)


def f32(x):
    return float(np.float32(x))


def _payload(b, flat):
    """The [rows, cols] view of another copy `flat` of buffer b's allocation."""
    return flat[b.start:b.start + b.rows * b.ld].view(b.rows, b.ld)[:, :b.cols]


def same_runs(bufs_a, bufs_b, what):
    for a, b in zip(bufs_a, bufs_b):
        if not torch.equal(_bits(a.flat), _bits(b.flat)):
            raise StepCheckError("repeat", f"{what}: two runs from the same state differ")


# ---------------------------------------------------------------------------------------- 1 dense Adam
AdamCase = collections.namedtuple("AdamCase", "name n kind steps gs zg jobs", defaults=((),))      # jobs: ((first, rows, cols, ld_dst), ...)
ADAM_KINDS = ("exact", "gauss", "gzero", "allzero")
ADAM_BIG = 4 * 256 * 8192 + 4 * 256 + 3
ADAM_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1027)
ADAM_ROUTES = ("tail_only", "vec_only", "vec_tail", "grid_stride", "jobs_0", "jobs_1", "jobs_2", "jobs_4", "zero_grad_0", "zero_grad_1", "step_1",
               "step_chain", "step_late")
ADAM_TIES = (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.5 + 2.0 ** -9, -(0.5 + 3 * 2.0 ** -9))     # halfway between two bf16, on the 2^-10 grid


def adam_cases():
    cs, gss = [], (1.0, 0.5, 1.0 / 3.0)
    for i, n in enumerate(ADAM_SIZES):
        cs += [AdamCase(f"n{n}-chain", n, "gauss", (1, 2, 3), gss[i % 3], i % 2),
               AdamCase(f"n{n}-exact", n, "exact", (1,), (1.0, 0.5, 2.0, 0.125)[i % 4], (i + 1) % 2),
               AdamCase(f"n{n}-late", n, ("gauss", "gzero", "allzero")[i % 3], (100000,), gss[(i + 1) % 3], (i // 2) % 2)]
    for n in (3, 1027):
        cs += [AdamCase(f"n{n}-gzero", n, "gzero", (1, 2, 3), 1.0, 1), AdamCase(f"n{n}-allzero", n, "allzero", (1, 2, 3), 0.5, 0)]
    cs += [AdamCase("big-late", ADAM_BIG, "gauss", (100000,), 1.0 / 3.0, 1), AdamCase("big-exact", ADAM_BIG, "exact", (1,), 0.5, 0),
           AdamCase("pack1-exact", 1211, "exact", (1,), 1.0, 1, ((8, 4, 300, 320),)),                     # ends at n - n % 4
           AdamCase("pack1-gauss", 2053, "gauss", (1, 2, 3), 0.5, 0, ((1148, 3, 300, 304),)),
           AdamCase("pack2-gauss", 1027, "gauss", (100000,), 1.0 / 3.0, 1, ((0, 3, 4, 4), (124, 3, 300, 300))),   # a gap; ends at n - n % 4
           AdamCase("pack2-exact", 1024, "exact", (1,), 2.0, 0, ((0, 1, 4, 8), (8, 3, 300, 320))),
           AdamCase("pack4-exact", 2600, "exact", (1,), 0.5, 1, ((4, 2, 4, 8), (16, 25, 4, 320), (120, 2, 300, 304), (1400, 4, 300, 300))),
           AdamCase("pack4-gauss", 2603, "gauss", (1, 2, 3), 1.0, 1, ((0, 1, 300, 300), (300, 1, 300, 304), (600, 1, 300, 320), (2592, 2, 4, 4)))]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def adam_route(c):
    """adam_kernel: n / 4 float4 items, then up to 3 tail elements taken by threads 0..2 of block 0; blocks = ceil((n/4 + 1) /
    256) capped at 8192, beyond which the float4 loop strides; nr_adam_step is nr_adam_step_packed without jobs."""
    n4 = c.n // 4
    r = ["tail_only" if n4 == 0 else "vec_only" if c.n % 4 == 0 else "vec_tail"]
    if (n4 + 1 + 255) // 256 > 8192:
        r.append("grid_stride")
    return tuple(r + [f"jobs_{len(c.jobs)}", f"zero_grad_{c.zg}", "step_chain" if len(c.steps) > 1 else "step_1" if c.steps == (1,) else "step_late"])


def adam_hp(c):
    """(lr, beta1, beta2, eps) as the fp32 values the C ABI receives."""
    return (2.0 ** -10, 0.5, 0.75, 0.0) if c.kind == "exact" else tuple(f32(x) for x in (3e-4, 0.9, 0.999, 1e-8))


def adam_scalars(lr, b1, b2, step):
    """nr_adam_bias: double arithmetic, then the cast: (step_size, bc2_sqrt) as fp32 values."""
    return f32(lr / (1.0 - math.pow(b1, step))), f32(math.sqrt(1.0 - math.pow(b2, step)))


def adam_grad(c, step):
    g = _gen(12, c.n % 65521, ADAM_KINDS.index(c.kind), step % 1000, c.zg, len(c.jobs))
    if c.kind == "exact":
        return torch.randint(1, 8, (c.n,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (c.n,), generator=g).float()) * 0.25
    if c.kind == "gauss":
        return torch.randn(c.n, generator=g) * 10.0 ** (-6 * torch.rand(c.n, generator=g))
    return torch.zeros(c.n)


def adam_problem(c, dev):
    g = _gen(11, c.n % 65521, ADAM_KINDS.index(c.kind), c.zg, len(c.jobs), len(c.steps))
    n = c.n
    if c.kind == "exact":
        p = torch.randint(-4096, 4097, (n,), generator=g).float() * 2.0 ** -10
        m = v = torch.zeros(n)
        sg = torch.sign(adam_grad(c, 1))
        for j, (first, rows, cols, ld) in enumerate(c.jobs):                # p' = p - sign(g) 2^-10 lands on the ties
            for k, t in enumerate(ADAM_TIES):
                i = first + (j + 3 * k) % (rows * cols)
                p[i] = t + sg[i] * 2.0 ** -10
    else:
        p = torch.randn(n, generator=g) * 0.4 * 10.0 ** (-9 * torch.rand(n, generator=g))       # where |p| is small the bound is the quotient's
        p[4::5] = 0.0
        m = torch.zeros(n) if c.kind == "allzero" else torch.randn(n, generator=g) * 0.01
        v = torch.zeros(n) if c.kind == "allzero" else (torch.randn(n, generator=g) * 0.01) ** 2
    P = SimpleNamespace(c=c)
    for k, t in (("p", p), ("g", torch.zeros(n)), ("m", m), ("v", v)):
        setattr(P, k, glue_buf(1, n, n, torch.float32, dev, 0, t.to(dev)))
    P.dst = [glue_buf(rows, cols, ld, torch.bfloat16, dev, 4 * ((j + 1) % 2)) for j, (first, rows, cols, ld) in enumerate(c.jobs)]     # 8-byte aligned, not 16
    return P


def adam_bufs(P):
    return [P.p, P.g, P.m, P.v] + P.dst


def adam_ref64(p, g, m, v, lr, b1, b2, eps, step, gs):
    """include/nrhip.h, f4, in fp64 on the fp32 state: g' = g grad_scale; m' = lerp(m, g', 1-b1); v' = b2 v + (1-b2) g'^2;
    p' = p - lr / (1-b1^t) m' / (sqrt(v') / sqrt(1-b2^t) + eps)."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gp = g * gs
    m1 = m + (1 - b1) * (gp - m)
    v1 = b2 * v + (1 - b2) * gp * gp
    ss, bc = lr / (1 - b1 ** step), math.sqrt(1 - b2 ** step)
    den = v1.sqrt() / bc + eps
    q = m1 / den
    return SimpleNamespace(gp=gp, m0=m, m=m1, v=v1, den=den, q=q, p=p - ss * q, ss=ss, bc=bc, b1=b1, b2=b2)


def adam_bounds(r):
    """(e_m, e_v, e_p) of the module docstring."""
    e_g = U * r.gp.abs() + F149
    e_m = (1 - r.b1) * e_g + 3 * U * (1 - r.b1) * (r.gp - r.m0).abs() + U * r.m.abs() + 3 * F149
    e_v = 7 * U * r.v + 4 * F149
    sq = r.v.sqrt()
    e_sq = 4.5 * U * sq + torch.minimum(torch.full_like(sq, math.sqrt(4 * F149)), 4 * F149 / (2 * sq))
    e_den = (e_sq + 2 * U * sq) / r.bc + U * r.den + F149
    e_q = (e_m / r.den + r.q.abs() * e_den / r.den) * (1 + 2.0 ** -20) + (1 + STEP_DIV_EXCESS) * U * r.q.abs() + F149
    e_p = r.ss * e_q + 3 * U * (r.ss * r.q).abs() + U * r.p.abs() + 2 * F149
    return e_m, e_v, e_p


def adam_terms(P, pre, step):
    """[(layer, result view, fp64 reference, bound)] of one step from the state `pre` = (p, g, m, v) before it."""
    c = P.c
    r = adam_ref64(*pre, *adam_hp(c), step, f32(c.gs))
    e_m, e_v, e_p = adam_bounds(r)
    return [("m", P.m.v[0], r.m, e_m), ("v", P.v.v[0], r.v, e_v), ("p", P.p.v[0], r.p, e_p)]


def adam_check(P, pre, step):
    c = P.c
    for k, b in zip(("p", "g", "m", "v") + tuple(f"dst{j}" for j in range(len(P.dst))), adam_bufs(P)):
        sent(k, b)
    same("grad", "g", P.g.v[0], torch.zeros_like(pre[1]) if c.zg else pre[1])
    if c.kind == "allzero":
        same("still", "p", P.p.v[0], pre[0])
        same("still", "m", P.m.v[0], torch.zeros_like(pre[2]))
        same("still", "v", P.v.v[0], torch.zeros_like(pre[3]))
    w = {}
    for layer, got, ref, bound in adam_terms(P, pre, step):
        if c.kind == "exact":
            eq64("exact", layer, got, ref)
        w[layer] = within(layer, layer, got, ref, bound)
        if layer == "p" and c.kind in ("gauss", "gzero") and bool((pre[0] == 0).any()):       # reported: where p starts at 0 the bound is the quotient's alone
            w["p_from_0"] = float(((got.double() - ref).abs() / bound)[pre[0] == 0].max())
    for (first, rows, cols, ld), d in zip(c.jobs, P.dst):
        same("pack", f"dst of the job at {first}", d.v, P.p.v[0][first:first + rows * cols].view(rows, cols).to(torch.bfloat16))
    return w


def adam_run(c, dev, call, twice=True):
    """The driver both files share: per step a fresh gradient, call(P, step) on one or two problems built alike, the checks on
    the first, the bit comparison of the two."""
    Ps = [adam_problem(c, dev) for _ in range(2 if twice else 1)]
    w = {}
    for step in c.steps:
        gnew = adam_grad(c, step).to(dev)
        for P in Ps:
            P.g.v[0] = gnew
        pre = tuple(b.v[0].clone() for b in adam_bufs(Ps[0])[:4])
        for P in Ps:
            call(P, step)
        for k, x in adam_check(Ps[0], pre, step).items():
            w[k] = max(w.get(k, 0.0), x)
        if twice:
            same_runs(adam_bufs(Ps[0]), adam_bufs(Ps[1]), f"step {step}")
    return w


# ---------------------------------------------------------------------------------------- 2 row-deferred Adam
RowsCase = collections.namedtuple("RowsCase", "name rows width pack stride gs script")      # pack: None or (cols, ld)
ROWS_ROUTES = ("chunks_1", "chunks_2", "chunks_many", "no_pack", "pack_whole_row", "pack_cols_4", "pack_split", "stride_1", "stride_3", "ids_0",
               "ids_1", "only_skipped", "claim_one_block", "claim_blocks", "apply_one_pass", "apply_grid_stride", "flush")


ROWS_BIG = 1030


def rows_cases():
    cs, i = [], 0
    for rows in (2, 5, 300):
        for width in (4, 8, 1200):
            for k in range(4 if width == 1200 else 3):
                pk = (None, (width, width + 4 * (i % 2)), (4, 4 + 4 * (i % 2)), (300, 320))[k]
                cs.append(RowsCase(f"r{rows}-w{width}-" + ("nopack" if pk is None else f"c{pk[0]}ld{pk[1]}"), rows, width, pk, (1, 3)[i % 2], (1.0, 0.5)[(i // 2) % 2],
                                   "mixed"))
                i += 1
    # 1025 rows with every row named own 1024 (id 0 is skipped): 1024 * 2048 chunks fill the 8192 * 256 threads of the capped grid
    # exactly once, the last one-pass shape; from 1026 rows on a thread takes a second trip
    cs += [RowsCase("big-1025", 1025, 8192, None, 1, 1.0, "all"), RowsCase("big-nopack", ROWS_BIG, 8192, None, 1, 1.0, "all"),
           RowsCase("big-pack", ROWS_BIG, 8192, (4096, 4100), 3, 0.5, "all")]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def rows_script(c):
    """The id list of every step.  mixed: R = rows - 1 alone 300 times; other rows with id 0, negative ids and ids beyond the
    table; nothing; only skipped ids; 255, 256 and 257 ids, the last of which brings R back after 5 steps away; one id."""
    if c.script == "all":
        return [list(range(c.rows))]
    g = _gen(21, c.rows, c.width)
    R = c.rows - 1
    others = list(range(1, R))
    pool = others + [0, -1, -7, c.rows, c.rows + 3]
    draw = lambda k: [pool[j] for j in torch.randint(0, len(pool), (k,), generator=g).tolist()]
    return [[R] * 300, draw(40) + [0, -3, c.rows], [], [0, -1, c.rows, c.rows + 5, 0], draw(255), draw(256), draw(256) + [R], [others[0] if others else R]]


def rows_route(c):
    """adam_rows_claim_kernel: one thread per id, 256 per block (at least one block, which files the step's scalars);
    adam_rows_apply_kernel: ceil(n chunks / 256) blocks capped at 8192 over (work item, 16-byte chunk) of the rows the claim
    kernel listed, which are at most the distinct ids in [1, rows): a thread takes a second trip only when those exceed the grid."""
    chunks = c.width // 4
    r = {"chunks_1" if chunks == 1 else "chunks_2" if chunks == 2 else "chunks_many", f"stride_{c.stride}", "flush",
         "no_pack" if c.pack is None else "pack_whole_row" if c.pack[0] == c.width else "pack_cols_4" if c.pack[0] == 4 else "pack_split"}
    for ids in rows_script(c):
        n = len(ids)
        r.add("ids_0" if n == 0 else "ids_1" if n == 1 else "claim_one_block" if n <= 256 else "claim_blocks")
        if n:
            owned = len({i for i in ids if 1 <= i < c.rows})
            r.add("apply_grid_stride" if owned * chunks > min(8192, (n * chunks + 255) // 256) * 256 else "apply_one_pass")
            if not owned:
                r.add("only_skipped")
    return tuple(sorted(r))


ROWS_HP = tuple(f32(x) for x in (3e-4, 0.9, 0.999, 1e-8))


def rows_problem(c, dev):
    g = _gen(22, c.rows, c.width, 0 if c.pack is None else c.pack[0] + c.pack[1], c.stride)
    p0 = torch.randn(c.rows, c.width, generator=g) * 0.4
    p0[0] = 0
    P = SimpleNamespace(c=c, steps=len(rows_script(c)))

    def side(off):
        s = SimpleNamespace()
        for k, t in (("p", p0), ("g", torch.zeros_like(p0)), ("m", torch.zeros_like(p0)), ("v", torch.zeros_like(p0))):
            setattr(s, k, glue_buf(c.rows, c.width, c.width, torch.float32, dev, 0, t.to(dev)))
        s.pack = None
        if c.pack is not None:
            cols, ld = c.pack
            s.pack = glue_buf(c.rows * c.width // cols, cols, ld, torch.bfloat16, dev, off, p0.to(torch.bfloat16).to(dev))
        return s

    P.A, P.B = side(0), side(4)                    # B's packed copy 8-byte aligned only, row_step 4-byte, sched 8-byte
    P.row_step = glue_buf(1, c.rows, c.rows, torch.int32, dev, 1, 0)
    P.sched = glue_buf(P.steps + 2, 2, 2, torch.float32, dev, 2, 0.0)
    return P


def rows_side_bufs(s):
    return [s.p, s.g, s.m, s.v] + ([s.pack] if s.pack is not None else [])


def rows_ids_tensor(ids, stride, dev):
    """int32 [n stride]: the ids at the stride, row 1 in between (a kernel that ignores the stride names it)."""
    t = torch.ones(max(len(ids) * stride, 1), dtype=torch.int32)
    if ids:
        t[::stride][:len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return t.to(dev)


def _by_row(c, b):
    """Buffer b of a table side as [rows, elements of the row]."""
    return b.v.reshape(c.rows, -1)


def rows_state_bufs(P):
    return rows_side_bufs(P.B) + [P.row_step, P.sched]


def rows_checked_call(P, rows_call, ids, upto, apply, twin=None):
    """One nr_adam_rows call on side B with everything the issue asks of every call: guards intact, the rows the call did not
    own bit-unchanged in p, g, m, v and the packed copy, row_step moved on the owned rows only, sched on the filed step only,
    and the same call on `twin`, a second problem in the same state, leaving the same bits."""
    c, B = P.c, P.B
    bufs = rows_side_bufs(B)
    before = [b.flat.clone() for b in bufs]
    rs0, sc0 = P.row_step.v[0].clone(), P.sched.v.clone()
    target = upto + apply
    valid = sorted({i for i in ids if 1 <= i < c.rows}) if ids is not None else list(range(1, c.rows))
    rs_host = rs0.tolist()
    owned = [r for r in valid if rs_host[r] < target]
    for Q in (P,) if twin is None else (P, twin):
        rows_call(Q, None if ids is None else rows_ids_tensor(ids, c.stride, B.p.flat.device), 0 if ids is None else len(ids), upto, apply)
    if twin is not None:
        same_runs(rows_state_bufs(P), rows_state_bufs(twin), f"nr_adam_rows upto {upto} apply {apply}")
    for k, b in zip("pgmvk", bufs):
        sent(k, b)
    sent("row_step", P.row_step)
    sent("sched", P.sched)
    other = torch.ones(c.rows, dtype=torch.bool, device=B.p.flat.device)
    if owned:
        other[torch.tensor(owned, device=other.device)] = False
    for k, b, f in zip(("p", "g", "m", "v", "packed copy"), bufs, before):
        was = _payload(b, f).reshape(c.rows, -1)
        same("untouched", f"{k} of rows the call did not own", _by_row(c, b)[other], was[other])
        if k == "g" and not apply:
            same("untouched", "g under apply = 0", _by_row(c, b), was)
    want = rs0.clone()
    if owned:
        want[torch.tensor(owned, device=want.device)] = target
    same("row_step", "row_step", P.row_step.v[0], want)
    if apply:
        lr, b1, b2, _ = ROWS_HP
        sc0[upto + 1] = torch.tensor(adam_scalars(lr, b1, b2, upto + 1), dtype=torch.float32, device=sc0.device)
    same("sched", "sched", P.sched.v, sc0)
    return valid


def rows_run(c, dev, dense_call, rows_call, twice=True):
    """Side A: the dense kernel over the whole table at every step; side B: catch-up and apply on the step's ids, then a flush.
    twice: every nr_adam_rows call is also made on a second problem in the same state and compared bit for bit."""
    P = rows_problem(c, dev)
    twin = rows_problem(c, dev) if twice else None
    g = _gen(23, c.rows, c.width)
    names = ("p", "g", "m", "v", "packed copy")
    for s, ids in enumerate(rows_script(c), 1):
        valid = rows_checked_call(P, rows_call, ids, s - 1, 0, twin)
        if valid:                                  # the rows just caught up are what dense Adam held after step s - 1
            ix = torch.tensor(valid, device=dev)
            for k, a, b in zip(names, rows_side_bufs(P.A), rows_side_bufs(P.B)):
                same("rows", f"{k} after the catch-up to {s - 1}", _by_row(c, b)[ix], _by_row(c, a)[ix])
            grad = (torch.randn(len(valid), c.width, generator=g) * 0.01).to(dev)
            P.A.g.v[ix] = grad
            P.B.g.v[ix] = grad
            if twice:
                twin.B.g.v[ix] = grad
        dense_call(P, s)
        rows_checked_call(P, rows_call, ids, s - 1, 1, twin)
    rows_checked_call(P, rows_call, None, P.steps, 0, twin)
    for k, a, b in zip(names, rows_side_bufs(P.A), rows_side_bufs(P.B)):
        sent(k + " (dense)", a)
        same("rows", f"{k} after the flush", b.v, a.v)
    want = torch.full((c.rows,), P.steps, dtype=torch.int32, device=dev)
    want[0] = 0
    same("row_step", "row_step after the flush", P.row_step.v[0], want)
    return P


# ---------------------------------------------------------------------------------------- 3 metrics
MET_CASES = ("waves", "waves-ties", "lds", "lds-onepos", "ties", "onepos", "n0", "n0-maxc", "n1", "n3", "n4", "n5", "n1023", "n1024", "n1025",
             "stride-a", "stride-b")
MET_ROUTES = ("c_0", "c_below_64", "c_64", "c_above_64", "c_lds_limit", "n_0", "n_one_block", "n_blocks", "n_grid_stride", "reduce_one_pass",
              "reduce_loop", "skipped", "label_not_0_1", "tied")
MET_LABELS = (0, 1, 2, -1)
MET_MAXC = 4096
MET_STRIDE_N = 16385 + 4


def _met_imp(g, c, tie=0.0, ppos=0.3, mixed=True):
    s = torch.randn(c, generator=g)
    if tie:
        s = torch.round(s * tie) / tie
    lab = torch.where(torch.rand(c, generator=g) < ppos, torch.randint(1, 4, (c,), generator=g), torch.zeros(c, dtype=torch.long))
    lab = torch.tensor(MET_LABELS)[lab]
    if mixed and c >= 2:
        j = torch.randperm(c, generator=g)[:2].tolist()
        lab[j[0]], lab[j[1]] = 1, 0
    return s.numpy().astype(np.float32), lab.numpy().astype(np.int32)


def _one_pos(s, j, val):
    lab = np.zeros(len(s), dtype=np.int32)
    lab[j] = val
    return s, lab


def met_impressions(name):
    """[(scores float32, labels int32)] of a case."""
    g = _gen(31, MET_CASES.index(name))
    f = lambda *v: np.array(v, dtype=np.float32)
    const = lambda c, x: np.full(c, x, dtype=np.float32)
    if name in ("waves", "waves-ties"):
        tie = 2.0 if name == "waves-ties" else 0.0
        out = [_met_imp(g, c, tie) for c in (0, 1, 2, 63, 64, 65, 128)] + [_met_imp(g, c, tie, 0.5) for c in (2, 63, 64, 65, 128)]
        out += [(const(64, 0.5), np.zeros(64, np.int32)), (_met_imp(g, 65, tie)[0], np.full(65, 2, np.int32))]             # all 0, all positive
        if tie:
            out += [(const(c, 0.25), _met_imp(g, c, 0, 0.4)[1]) for c in (63, 64, 65, 128)]                                  # every score tied
        return out
    if name == "lds":
        return [_met_imp(g, 4095, 8.0, 0.15), _met_imp(g, 4096, 8.0, 0.15), _met_imp(g, 4096, 0.0, 0.01)]
    if name == "lds-onepos":
        return [_one_pos(const(4096, 1.0), 0, 1), _one_pos(_met_imp(g, 4095, 8.0)[0], 4094, 2), (const(4096, 1.0), np.zeros(4096, np.int32)),
                _one_pos(const(4096, -2.0), 4095, -1)]
    if name == "ties":
        s300, l300 = _met_imp(g, 300, 0.0, 0.3)
        s300[30:230] = 0.5                                                   # a tie group of 200 across four lane passes
        z = np.where(np.arange(66) % 2 == 0, 0.0, -0.0).astype(np.float32)
        odd = f(np.inf, -np.inf, 1e-40, -1e-40, 2.0 ** -149, 0.0, -0.0, np.inf, 3e38, -np.inf, -(2.0 ** -149), 1.0)
        return [(s300, l300), (const(200, -1.5), _met_imp(g, 200, 0, 0.2)[1]), (z, _met_imp(g, 66, 0, 0.4)[1]),
                (odd, np.array([1, 0, 2, 0, 0, -1, 0, 0, 1, 1, 0, 0], np.int32)), (odd[::-1].copy(), np.array([0, 1, 0, 0, 2, 0, 0, 1, 0, 0, 0, -1], np.int32))]
    if name == "onepos":
        out = [_one_pos(f(0.5, 0.5), 0, 1), _one_pos(f(0.5, 0.5), 1, 2), _one_pos(f(1.0, 2.0), 0, -1), _one_pos(f(1.0, 2.0), 1, 1)]
        for k, c in enumerate((64, 65, 130)):
            s = _met_imp(g, c, 2.0)[0]
            tied = next(j for j in range(1, c - 1) if (s == s[j]).sum() > 2)
            out += [_one_pos(s, 0, MET_LABELS[1 + k % 3]), _one_pos(s, c - 1, MET_LABELS[1 + (k + 1) % 3]), _one_pos(s, tied, MET_LABELS[1 + (k + 2) % 3])]
        return out
    if name.startswith("stride"):
        ps = [f(1, 2), f(2, 1), f(1, 1), f(0.0, -0.0), f(np.inf, 1), f(-np.inf, 1e-40)]
        pl = [(1, 0), (0, 1), (1, 1), (0, 0), (2, 0), (0, -1)]
        k = 5 if name == "stride-a" else 7
        return [(ps[(i * k) % 6], np.array(pl[(i * k // 6 + i) % 6], np.int32)) for i in range(MET_STRIDE_N)]
    n = 0 if name.startswith("n0") else int(name[1:])
    out = []
    for i in range(n):
        s, lab = _met_imp(g, 1 + (i * 5) % 12, 2.0 if i % 3 == 0 else 0.0)
        if i % 7 == 3:
            lab[:] = 0
        if i % 11 == 5:
            lab[:] = 1
        out.append((s, lab))
    return out


def met_route(name):
    imps = met_impressions(name)
    n = len(imps)
    r = {"n_0" if n == 0 else "n_one_block" if n <= 4 else "n_grid_stride" if (n + 3) // 4 > 4096 else "n_blocks", "reduce_loop" if n > 1024 else "reduce_one_pass"}
    for s, lab in imps:
        c = len(s)
        r.add("c_0" if c == 0 else "c_below_64" if c < 64 else "c_64" if c == 64 else "c_lds_limit" if c >= MET_MAXC - 1 else "c_above_64")
        if (lab != 0).all() or (lab == 0).all():
            r.add("skipped")
        if ((lab != 0) & (lab != 1)).any():
            r.add("label_not_0_1")
        if len(np.unique(s)) < c:
            r.add("tied")
    return tuple(sorted(r))


def met_ref_one(scores, labels):
    """include/nrhip.h, f2, for one impression: None when it is skipped, else (AUC, MRR as Fractions, nDCG@5, nDCG@10 in fp64).
    scores: fp32 values as Python floats; a label != 0 is a positive."""
    c = len(scores)
    pos = [i for i in range(c) if labels[i] != 0]
    npos, nneg = len(pos), c - len(pos)
    if npos == 0 or nneg == 0:
        return None
    order = sorted(range(c), key=lambda i: (-scores[i], -i))                 # descending, the later index first on ties
    rank = [0] * c
    for r, i in enumerate(order):
        rank[i] = r
    negs = sorted(scores[i] for i in range(c) if labels[i] == 0)
    twice = 0
    for i in pos:                                                            # Mann-Whitney with half credit, counted in halves
        lo, hi = bisect.bisect_left(negs, scores[i]), bisect.bisect_right(negs, scores[i])
        twice += 2 * lo + (hi - lo)
    auc = Fraction(twice, 2 * npos * nneg)
    mrr = sum(Fraction(1, rank[i] + 1) for i in pos) / npos
    gain = lambda r: 1.0 / math.log2(r + 2)
    rs = sorted(rank[i] for i in pos)
    nd = [math.fsum(gain(r) for r in rs if r < k) / math.fsum(gain(r) for r in range(min(npos, k))) for k in (5, 10)]
    return auc, mrr, nd[0], nd[1]


def met_ref(imps):
    """(ref [n, 4] float64, bound [n, 4], skipped [n] bool) as numpy arrays."""
    n = len(imps)
    ref, bound, skipped, cache = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros(n, dtype=bool), {}
    for i, (s, lab) in enumerate(imps):
        key = (s.tobytes(), lab.tobytes())
        if key not in cache:
            cache[key] = met_ref_one([float(x) for x in s], lab.tolist())
        one = cache[key]
        if one is None:
            skipped[i], ref[i] = True, (-1.0, 0.0, 0.0, 0.0)
            continue
        ref[i] = [float(x) for x in one]
        bound[i] = (len(s) + 8) * 2.0 ** -53 * np.abs(ref[i]) + np.array([0.0, 0.0, METRIC_LOG2_EXCESS, METRIC_LOG2_EXCESS])
    return ref, bound, skipped


def met_problem(name, dev, max_cand=None):
    imps = met_impressions(name)
    n = len(imps)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s, _ in imps])
    cat = lambda k, dt: torch.from_numpy(np.concatenate([x[k] for x in imps]).astype(dt) if n else np.zeros(0, dt)).to(dev)
    P = SimpleNamespace(name=name, imps=imps, n=n, score=cat(0, np.float32), label=cat(1, np.int32), offsets=torch.from_numpy(off).to(dev))
    P.max_cand = max((len(s) for s, _ in imps), default=MET_MAXC if name == "n0-maxc" else 0) if max_cand is None else max_cand
    P.per = glue_buf(n, 4, 4, torch.float64, dev, 1)               # 8-byte aligned, no more
    P.sums = glue_buf(1, 5, 5, torch.float64, dev, 3)
    return P


def met_terms(P):
    ref, bound, skipped = (torch.from_numpy(x).to(P.per.flat.device) for x in met_ref(P.imps))
    return ref, bound, skipped


def met_check(P, terms=None):
    sent("per_imp", P.per)
    sent("sums", P.sums)
    ref, bound, skipped = met_terms(P) if terms is None else terms
    w = {}
    if P.n:
        same("skip", "rows of skipped impressions", P.per.v[skipped], ref[skipped])
        live = ~skipped
        for k, nm in enumerate(("auc", "mrr", "ndcg5", "ndcg10")):
            w[nm] = within("metric", nm, P.per.v[live][:, k], ref[live][:, k], bound[live][:, k])
        rows = P.per.v[live].cpu().tolist()
        want = [float(len(rows))] + [math.fsum(r[k] for r in rows) for k in range(4)]
    else:
        want = [0.0] * 5
    got = P.sums.v[0].cpu().tolist()
    if not got[0] == want[0]:
        raise StepCheckError("sums", f"sums[0] = {got[0]!r}, {want[0]!r} impressions are scored")
    if P.n == 0:
        same("sums", "sums of no impressions", P.sums.v[0], torch.zeros(5, dtype=torch.float64, device=P.sums.flat.device))
    for k in range(1, 5):
        b = (P.n + 2) * 2.0 ** -53 * abs(want[k])
        if not abs(got[k] - want[k]) <= b:
            raise StepCheckError("sums", f"sums[{k}] = {got[k]!r}, fsum of the rows {want[k]!r}, bound {b:.3g}")
        if b:
            w[f"sums{k}"] = abs(got[k] - want[k]) / b
    return w


# ---------------------------------------------------------------------------------------- 4 batch assembly
AsmCase = collections.namedtuple("AsmCase", "name B H K F labels badidx bad")       # bad: "prefill" (5, accumulated) or "null"
ASM_ROWS = 23
ASM_ROUTES = ("one_pass", "grid_stride", "h_0", "h_some", "k_0", "k_some", "labels_good", "labels_bad", "indices_good", "indices_bad", "bad_counted",
              "bad_null")
ASM_GRID = 65536 * 256


def asm_labels(K, kind):
    return ((0, (K + 1) // 2, K), (-1, K + 1, K), (K, 2 ** 32 + 1, -2 ** 33))[kind]


def asm_cases():
    cs, i = [], 0
    for B in (1, 3):
        for H in (0, 1, 50):
            for K in (0, 1, 4):
                lab, rot = asm_labels(K, (i + i // 3) % 3), (i // 3) % 3
                lab = (lab[rot:] + lab[:rot])[:B]
                cs.append(AsmCase(f"B{B}-H{H}-K{K}", B, H, K, (1, 7)[(i + i // 3) % 2], lab, (i // 2 + i // 9) % 2 == 1, "null" if i % 4 == 3 else "prefill"))
                i += 1
    cs += [AsmCase("big-bad", 3100, 50, 4, 100, asm_labels(4, 0) + asm_labels(4, 1) + asm_labels(4, 2), True, "prefill"),
           AsmCase("big-good", 3300, 49, 4, 95, asm_labels(4, 0), False, "null")]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def asm_route(c):
    """assemble_kernel: one thread per output element, ceil(total / 256) blocks capped at 65536."""
    good = all(0 <= x <= c.K for x in c.labels)
    return ("grid_stride" if c.B * (c.H + 1 + c.K) * c.F > ASM_GRID else "one_pass", "h_some" if c.H else "h_0", "k_some" if c.K else "k_0",
            "labels_good" if good else "labels_bad", "indices_bad" if c.badidx else "indices_good", "bad_null" if c.bad == "null" else "bad_counted")


def asm_problem(c, dev):
    g = _gen(41, c.B, c.H, c.K, c.F, c.badidx)
    ri = lambda *s: torch.randint(0, ASM_ROWS, s, generator=g, dtype=torch.int32)
    comb = torch.randint(0, 1000, (ASM_ROWS, c.F), generator=g, dtype=torch.int32)
    hist, pos, neg = ri(c.B, c.H), ri(c.B), ri(c.B, c.K)
    if c.badidx:
        pos[c.B // 2] = ASM_ROWS
        if c.H:
            hist[0, 0], hist[-1, -1] = -1, ASM_ROWS
        if c.K:
            neg[-1, 0], neg[0, -1] = -1, ASM_ROWS + 9
    label = torch.tensor([c.labels[b % len(c.labels)] for b in range(c.B)], dtype=torch.int64)
    P = SimpleNamespace(c=c, comb=comb.to(dev), hist=hist.to(dev), pos=pos.to(dev), neg=neg.to(dev), label=label.to(dev))
    P.history = glue_buf(c.B * c.H, c.F, c.F, torch.int32, dev, 1 + c.K % 2, IFILL)             # 4-byte aligned, no more
    P.candidate = glue_buf(c.B * (1 + c.K), c.F, c.F, torch.int32, dev, 3 - c.H % 2, IFILL)
    P.bad = glue_buf(1, 1, 1, torch.int32, dev, 1, 5) if c.bad == "prefill" else None
    return P


def asm_ref(comb, hist, pos, neg, label, K):
    """numpy fancy indexing and the list splice of the reference's line_mapper, with the documented replacements: a label
    outside [0, K] counts once and becomes 0, an index outside [0, n_rows) counts once per slot and becomes row 0."""
    B, nbad = len(pos), 0
    samp = np.zeros((B, 1 + K), dtype=np.int64)
    for b in range(B):
        lab = int(label[b])
        if lab < 0 or lab > K:
            nbad, lab = nbad + 1, 0
        samp[b] = neg[b, :lab].tolist() + [int(pos[b])] + neg[b, lab:].tolist()
    out = []
    for ix in (hist.astype(np.int64), samp):
        wrong = (ix < 0) | (ix >= comb.shape[0])
        nbad += int(wrong.sum())
        out.append(comb[np.where(wrong, 0, ix)])
    return out[0], out[1], nbad


def asm_check(P):
    c, dev = P.c, P.candidate.flat.device
    sent("history", P.history)
    sent("candidate", P.candidate)
    h, cand, nbad = asm_ref(*(t.cpu().numpy() for t in (P.comb, P.hist, P.pos, P.neg, P.label)), c.K)
    same("assemble", "history", P.history.v, torch.from_numpy(h).reshape(c.B * c.H, c.F).to(dev))
    same("assemble", "candidate", P.candidate.v, torch.from_numpy(cand).reshape(c.B * (1 + c.K), c.F).to(dev))
    if P.bad is not None:
        sent("bad", P.bad)
        same("bad", "bad", P.bad.v, torch.tensor([[5 + nbad]], dtype=torch.int32, device=dev))
    return nbad


# ---------------------------------------------------------------------------------------- 5 stacked encoder batch
StackCase = collections.namedtuple("StackCase", "name ra rb F mask flags")
STACK_ROUTES = ("one_pass", "grid_stride", "empty", "a_0", "b_0", "both", "mask", "mask_null", "flags", "flags_null")
STACK_MASK = (0.0, -0.0, 1.0, 0.5, 1e-40, NAN)
STACK_GRID = 4096 * 256


def stack_cases():
    cs = []
    for i, (ra, rb) in enumerate(((0, 0), (0, 5), (5, 0), (3, 7), (1, 1), (0, 0), (7, 13))):
        for j, F in enumerate((1, 30)):
            cs.append(StackCase(f"{ra}+{rb}-F{F}", ra, rb, F, (i + j) % 3 != 0, (i + j) % 4 != 1))
    cs += [StackCase("big-both", 20000, 20000, 30, True, True), StackCase("big-b", 0, 36000, 30, False, True)]
    return [c._replace(name=f"{c.name}-{k}") for k, c in enumerate(cs)]


def stack_route(c):
    """stack_rows_kernel: ceil(total / 256) blocks capped at 4096; the same grid strides over the rows for the flags."""
    total = (c.ra + c.rb) * c.F
    if total == 0:
        return ("empty",)
    return ("grid_stride" if total > STACK_GRID else "one_pass", "a_0" if c.ra == 0 else "b_0" if c.rb == 0 else "both", "mask" if c.mask else "mask_null",
            "flags" if c.flags else "flags_null")


def stack_problem(c, dev):
    g = _gen(51, c.ra, c.rb, c.F, c.mask, c.flags)
    P = SimpleNamespace(c=c, a=torch.randint(0, 30000, (c.ra, c.F), generator=g, dtype=torch.int32).to(dev),
                        b=torch.randint(0, 30000, (c.rb, c.F), generator=g, dtype=torch.int32).to(dev), mask=None)
    if c.mask:
        P.mask = torch.tensor(STACK_MASK, dtype=torch.float32)[(torch.arange(c.rb) * 5 + c.F) % len(STACK_MASK)].to(dev)
    n = c.ra + c.rb
    P.out = glue_buf(n, c.F, c.F, torch.int32, dev, 1 + c.ra % 2, IFILL)                       # 4-byte aligned, no more
    P.flags = glue_buf(1, n, n, torch.int32, dev, 3, IFILL) if c.flags else None
    return P


def stack_check(P):
    c = P.c
    sent("out", P.out)
    same("stack", "out", P.out.v, torch.cat([P.a, P.b]))
    if P.flags is not None:
        sent("flags", P.flags)
        used = torch.ones(c.rb, dtype=torch.int32, device=P.a.device)
        if P.mask is not None:                      # != 0 as a number: anything but +0 and -0, subnormals and NaN included
            used = ((_bits(P.mask) & 0x7FFFFFFF) != 0).to(torch.int32)
        same("flags", "flags", P.flags.v[0], torch.cat([torch.ones(c.ra, dtype=torch.int32, device=P.a.device), used]))


# ---------------------------------------------------------------------------------------- 6 index checks
CheckCase = collections.namedtuple("CheckCase", "name kind count stride rows")
CHECK_COUNTS = (0, 1, 255, 256, 257, 1024 * 256 + 77, 2 * 1024 * 256 + 5)
CHECK_ROUTES = tuple(f"{k}_{r}" for k in ("ids", "labels") for r in ("count_0", "one_block", "blocks", "grid_stride", "rows_0", "rows_some")) + ("ids_stride_1", "ids_stride_3")
CHECK_BIG = (2 ** 32, 2 ** 32 + 1, -2 ** 33)


def check_cases():
    cs = []
    for kind in ("ids", "labels"):
        for i, count in enumerate(CHECK_COUNTS):
            for rows in ((7, 0) if count in (0, 1, 257) else (0,) if count == 255 else (7,)):
                cs.append(CheckCase(f"{kind}-{count}-r{rows}", kind, count, (1, 3)[i % 2] if kind == "ids" else 1, rows))
        cs += [CheckCase(f"{kind}-300-s{s}", kind, 300, s if kind == "ids" else 1, 1 + s) for s in (1, 3)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def check_route(c):
    """check_*_kernel: count / 256 + 1 blocks capped at 1024; count == 0 launches nothing."""
    blocks = c.count // 256 + 1
    r = [f"{c.kind}_" + ("count_0" if c.count == 0 else "one_block" if blocks == 1 else "grid_stride" if blocks > 1024 else "blocks"),
         f"{c.kind}_" + ("rows_0" if c.rows == 0 else "rows_some")]
    return tuple(r + ([f"ids_stride_{c.stride}"] if c.kind == "ids" else []))


def check_problem(c, dev):
    g = _gen(61, c.kind == "ids", c.count, c.stride, c.rows)
    pool = [-1, 0, c.rows - 1, c.rows, c.rows // 2, c.rows + 1] + (list(CHECK_BIG) if c.kind == "labels" else [-2 ** 31, 2 ** 31 - 1])
    vals = torch.tensor(pool, dtype=torch.int64)[torch.randint(0, len(pool), (c.count,), generator=g)]
    if c.kind == "labels" and c.count >= 3:
        vals[0], vals[c.count // 2], vals[-1] = CHECK_BIG
    if c.kind == "ids":
        buf = torch.full((max(c.count * c.stride, 1),), c.rows + 5, dtype=torch.int32)      # between the strides: bad values
        if c.count:
            buf[::c.stride][:c.count] = vals.to(torch.int32)
    else:
        buf = vals.clone() if c.count else torch.zeros(1, dtype=torch.int64)
    return SimpleNamespace(c=c, vals=vals, buf=buf.to(dev), bad=glue_buf(1, 1, 1, torch.int32, dev, 1 + c.count % 3, 3))


def check_check(P):
    v = P.vals.numpy()
    sent("bad", P.bad)
    nbad = int(((v < 0) | (v >= P.c.rows)).sum())
    same("count", "bad", P.bad.v, torch.tensor([[3 + nbad]], dtype=torch.int32, device=P.bad.flat.device))
    return nbad


H = sys.modules[__name__]          # the tests below (and the host file) address the part above as H


# ------------------------------------------------------------------------------------------ the GPU tests
def _L():
    return _lib.lib()


def _ok(rc, what):
    _lib.check(rc, what)
    torch.cuda.synchronize()


def _report(tag, name, w):
    print(f"\nSTEP {tag} {name} " + " ".join(f"{k}={v:.4f}" for k, v in w.items()))


def _adam_call(P, step):
    c = P.c
    lr, b1, b2, eps = H.adam_hp(c)
    a = (P.p.ptr, P.g.ptr, P.m.ptr, P.v.ptr, c.n, lr, b1, b2, eps, step, c.gs, c.zg)
    if not c.jobs:
        return _ok(_L().nr_adam_step(*a, ops._stream()), "nr_adam_step")
    arr = (_lib.PackJob * len(c.jobs))(*[_lib.PackJob(first, rows * cols, cols, d.ld, d.ptr) for (first, rows, cols, ld), d in zip(c.jobs, P.dst)])
    _ok(_L().nr_adam_step_packed(*a, arr, len(c.jobs), ops._stream()), "nr_adam_step_packed")


@pytest.mark.parametrize("c", H.adam_cases(), ids=lambda c: c.name)
def test_adam_step(c):
    _report("adam", c.name, H.adam_run(c, DEV, _adam_call))


def test_adam_step_refuses_five_jobs_and_leaves_everything():
    c = H.AdamCase("five", 64, "exact", (1,), 1.0, 1, tuple((8 * j, 1, 4, 4) for j in range(5)))
    P = H.adam_problem(c, DEV)
    arr = (_lib.PackJob * 5)(*[_lib.PackJob(first, rows * cols, cols, d.ld, d.ptr) for (first, rows, cols, ld), d in zip(c.jobs, P.dst)])
    a = (P.p.ptr, P.g.ptr, P.m.ptr, P.v.ptr, c.n, *H.adam_hp(c), 1, 1.0, 1)
    assert _L().nr_adam_step_packed(*a, arr, 5, ops._stream()) == 1 and "5 pack jobs" in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    for b in H.adam_bufs(P):
        assert torch.equal(_bits(b.flat), _bits(b.init))


def _dense_rows_call(P, s):
    c, A = P.c, P.A
    lr, b1, b2, eps = H.ROWS_HP
    job, nj = None, 0
    if A.pack is not None:
        job, nj = (_lib.PackJob * 1)(_lib.PackJob(0, c.rows * c.width, c.pack[0], A.pack.ld, A.pack.ptr)), 1
    _ok(_L().nr_adam_step_packed(A.p.ptr, A.g.ptr, A.m.ptr, A.v.ptr, c.rows * c.width, lr, b1, b2, eps, s, c.gs, 1, job, nj, ops._stream()),
        "nr_adam_step_packed")


def _rows_call(P, ids, n_ids, upto, apply):
    c, B = P.c, P.B
    lr, b1, b2, eps = H.ROWS_HP
    d = _lib.AdamRowsDesc(param=B.p.ptr, grad=B.g.ptr, exp_avg=B.m.ptr, exp_avg_sq=B.v.ptr, rows=c.rows, width=c.width, row_step=P.row_step.ptr,
                          sched=P.sched.ptr, sched_capacity=P.sched.rows, upto=upto, apply=apply, zero_grad=1, lr=lr, beta1=b1, beta2=b2, eps=eps,
                          grad_scale=c.gs)
    n = c.rows
    if ids is not None:
        d.ids, d.ids_stride, d.n_ids, n = ids.data_ptr(), c.stride, n_ids, n_ids
    if B.pack is not None:
        d.pack_dst, d.pack_cols, d.pack_ld = B.pack.ptr, c.pack[0], B.pack.ld
    ws = torch.empty((_L().nr_adam_rows_workspace_bytes(n) + 3) // 4, dtype=torch.int32, device=DEV)
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _ok(_L().nr_adam_rows(C.byref(d), ops._stream()), "nr_adam_rows")


@pytest.mark.parametrize("c", H.rows_cases(), ids=lambda c: c.name)
def test_adam_rows(c):
    """Every call twice from the same state (rows_run's twin), compared bit for bit after each."""
    H.rows_run(c, DEV, _dense_rows_call, _rows_call)


def _met_call(P):
    per_bytes = _L().nr_eval_metrics_workspace_bytes(P.n)
    assert per_bytes == P.n * 32
    return _L().nr_eval_metrics(_lib.ptr(P.score) if P.score.numel() else None, _lib.ptr(P.label) if P.label.numel() else None, P.offsets.data_ptr(), P.n,
                                P.max_cand, P.per.ptr, per_bytes, P.sums.ptr, ops._stream())


@pytest.mark.parametrize("name", H.MET_CASES)
def test_eval_metrics(name):
    P, P2 = H.met_problem(name, DEV), H.met_problem(name, DEV)
    assert all(len(s) <= P.max_cand for s, _ in P.imps)                     # a longer impression would overrun the wave's LDS region
    _ok(_met_call(P), "nr_eval_metrics")
    _ok(_met_call(P2), "nr_eval_metrics")
    _report("metrics", name, H.met_check(P))
    H.same_runs([P.per, P.sums], [P2.per, P2.sums], name)


def _asm_call(P):
    c = P.c
    return _L().nr_assemble_batch(P.comb.data_ptr(), H.ASM_ROWS, c.F, P.hist.data_ptr() if c.H else None, P.pos.data_ptr(), P.neg.data_ptr() if c.K else None,
                                  P.label.data_ptr(), c.B, c.H, c.K, P.history.ptr if c.H else None, P.candidate.ptr, P.bad.ptr if P.bad is not None else None,
                                  ops._stream())


@pytest.mark.parametrize("c", H.asm_cases(), ids=lambda c: c.name)
def test_assemble_batch(c):
    P, P2 = H.asm_problem(c, DEV), H.asm_problem(c, DEV)
    _ok(_asm_call(P), "nr_assemble_batch")
    _ok(_asm_call(P2), "nr_assemble_batch")
    nbad = H.asm_check(P)
    assert (nbad > 0) == (c.badidx or "labels_bad" in H.asm_route(c))
    H.same_runs([P.history, P.candidate], [P2.history, P2.candidate], c.name)
    if P.bad is not None:                                                   # the counter accumulates: a second call adds the same again
        _ok(_asm_call(P), "nr_assemble_batch")
        H.same("bad", "bad after a second call", P.bad.v, torch.tensor([[5 + 2 * nbad]], dtype=torch.int32, device=DEV))


def _stack_call(P):
    c = P.c
    return _L().nr_stack_rows(P.a.data_ptr() if c.ra else None, c.ra, P.b.data_ptr() if c.rb else None, c.rb, c.F, _lib.ptr(P.mask) if c.rb else None, P.out.ptr,
                              P.flags.ptr if P.flags is not None else None, ops._stream())


@pytest.mark.parametrize("c", H.stack_cases(), ids=lambda c: c.name)
def test_stack_rows(c):
    P, P2 = H.stack_problem(c, DEV), H.stack_problem(c, DEV)
    _ok(_stack_call(P), "nr_stack_rows")
    _ok(_stack_call(P2), "nr_stack_rows")
    H.stack_check(P)
    H.same_runs([P.out] + ([P.flags] if P.flags is not None else []), [P2.out] + ([P2.flags] if P2.flags is not None else []), c.name)


def _check_call(P):
    c = P.c
    if c.kind == "ids":
        return _L().nr_check_ids(P.buf.data_ptr(), c.count, c.stride, c.rows, P.bad.ptr, ops._stream())
    return _L().nr_check_labels(P.buf.data_ptr(), c.count, c.rows, P.bad.ptr, ops._stream())


@pytest.mark.parametrize("c", H.check_cases(), ids=lambda c: c.name)
def test_check_ids_and_labels(c):
    P = H.check_problem(c, DEV)
    _ok(_check_call(P), "nr_check_" + c.kind)
    nbad = H.check_check(P)
    _ok(_check_call(P), "nr_check_" + c.kind)                               # accumulated: a second call adds the same again
    H.same("count", "bad after a second call", P.bad.v, torch.tensor([[3 + 2 * nbad]], dtype=torch.int32, device=DEV))

"""GPU: every kernel route of the two exported GEMM building blocks (nr_gemm_nt / nr_gemm_tn, csrc/nr_gemm.hip) against
fp64, dense rows.  The case tables, the two input layers and the checker are the first part of this file ("GEMM
building-block sweep"; plain torch, no GPU needed); tests/test_gemm_sweep_host.py imports them and proves on the CPU that this
checker fails a subtly wrong kernel, tests/test_gpu_gather_linear.py uses the same checker.

Per case and layer: operands and outputs are views into larger buffers (NaN in the slack of A, dC and -- beyond the zero
padding nr_gemm_nt asks for -- of B; a sentinel in the slack of the outputs), NT outputs start as NaN, TN outputs as
integers.  Checked: the profiler label of the expected route, sentinels unchanged bit for bit, no NaN stored, the lattice
layer bit-equal to the fp64 product rounded to nearest even, layer 2 inside its elementwise bound, NT bit-equal across two
runs.  The library is called directly (ops.gemm_nt / ops.gemm_tn cannot express the strides and the pre-fill).

Routes as verified against the dispatch (the host file checks gemm_nt_route / gemm_tn_route on every case; the
labels asserted here are what the library reports): see DESIGN.md "GEMM building blocks".
"""
import collections
import sys
from types import SimpleNamespace

import pytest
import torch

from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {"bf16": ops.NR_BF16, "f32": ops.NR_F32}


# ------------------------------------------------------------------------------------------ GEMM building-block sweep
# Case tables, inputs, references and the checker of tests/test_gpu_gemm_sweep.py (run on the kernels) and
# tests/test_gemm_sweep_host.py (run on a CPU stand-in and on mutants of it).  Two input layers:
#   "lattice": small integers (exact in bf16 and in fp32 sums of any order below 2^24) -> compared bit for bit;
#   "layer2" : Gaussian operands (scales 0.5 / 0.1) against fp64 with an elementwise bound:
#                fp32 out: |c - ref| <= (T + 2) 2^-24 S                     T = number of products per output element
#                bf16 out: |c - ref| <= 2^-8 |ref| + (T + 2) 2^-24 S (1 + 2^-8)
#              S = |A| |B|^T (NT) or |dC|^T |A| (TN) in fp64, plus |bias| (NT) or |pre-fill| (TN): the bias and the value
#              the kernel accumulates onto are one more summand of the same fp32 sum, and the "+ 2" pays for its addition
#              and the final rounding.  With tanh the pre-activation bound carries through (tanh is 1-Lipschitz) plus
#              GEMM_TANH_ABS for tanhf itself.

GEMM_U = 2.0 ** -24
# Absolute error of the device tanhf on top of the carried pre-activation bound: four times the worst excess measured over
# the tanh cases of the sweep on the MI355X, and never more than 1e-5.  Measured: no excess at all -- the worst case (fp32
# kernel, K = 4, where the carried bound is 6 * 2^-24 * S) stays 4.7e-9 BELOW the carried bound, every other case 1.0e-6 to
# 2.9e-4 below (DESIGN.md "GEMM building blocks") -- so the term is 0.
GEMM_TANH_ABS = 0.0
GEMM_SENTINEL = -1232.0          # exact in bf16; what slack columns and trailing rows of outputs hold

NTCase = collections.namedtuple("NTCase", "route dt out M N K lda ldb ldc bias tanh")
TNCase = collections.namedtuple("TNCase", "route dt M N K ldc lda ldw db")


class GemmCheckError(AssertionError):
    """A failed check of the sweep; `.layer` is "sentinel", "lattice" or "layer2"."""

    def __init__(self, layer, msg):
        super().__init__(f"[{layer}] {msg}")
        self.layer = layer


def _rup(v, m):
    return (v + m - 1) // m * m


def _tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def gemm_nt_route(c):
    """The kernel nr_launch_gemm_nt (csrc/nr_gemm.hip) takes for a dense-row EPI_STORE call: the sweep's route names."""
    if c.dt == "bf16" and c.K >= 192 and c.ldb >= _rup(c.K, 32):
        if c.out == "bf16" and c.N % 8 == 0 and c.ldc % 8 == 0 and c.M >= 64:
            if not c.tanh and 288 < c.K <= 320 and c.N >= 320:
                return "wreg5"
            if not c.tanh and 384 < c.K <= 416 and c.N >= 320:
                return "wreg3"
            if c.tanh and 384 < c.K <= 416 and c.N <= 256:
                return "wreg_tanh"
        return "dma13" if _rup(c.N, 208) // 208 * 13 < _rup(c.N, 320) // 320 * 20 else "dma20"
    if c.dt == "bf16":
        return "wide" if c.N <= 208 else "tiled"
    return "f32"


def gemm_nt_label(c, route=None):
    """The profiler label of the route (NrProfScope in nr_launch_gemm_nt)."""
    route = route or c.route
    epi, dims = (3 if c.tanh else 0), f"M={c.M},N={c.N},K={c.K}"
    if route.startswith("wreg"):
        return f"gemm_nt_wreg[bf16,epi={epi},{dims}]"
    if route.startswith("dma"):
        return f"gemm_nt_dma[bf16,epi={epi},{dims},gap=0]"
    if route == "wide":
        return f"gemm_nt_wide[bf16,epi={epi},{dims}]"
    return f"gemm_nt[{c.dt},rows=0,epi={epi},{dims}]"


def gemm_tn_route(c):
    """The kernel nr_launch_gemm_tn takes for dense rows (tn3::eligible / wide_k / launch in csrc/nr_gemm.hip)."""
    if c.dt != "bf16":
        return "tn_f32"
    if c.M % 32 == 0 and c.M >= 16384 and c.N >= 8 and c.K >= 8:
        if c.K > 160 and _rup(c.K, 320) * 100 <= c.K * 115:
            return "tn3_w320_n256" if c.N > 256 else "tn3_w320_n128"
        return "tn3_w160"
    return "tn2"


def gemm_tn_label(c):
    dims = f"M={c.M},N={c.N},K={c.K}"
    if c.route.startswith("tn3"):
        return f"gemm_tn3[bf16,{dims},gap=0]"
    if c.route == "tn2":
        return f"gemm_tn2[bf16,{dims}]"
    return f"gemm_tn[f32,rows=0,{dims}]"


def _span(lo, hi):
    return list(range(lo, hi + 1))


def _nt_rows():
    """route -> (K list, N list, M list, rotations): the smallest shapes that still cross a boundary of the dispatch."""
    return [("wreg5", [296, 304, 320], [320, 328, 1208], [64, 65, 79, 1000], 2),
            ("wreg3", [392, 400, 416], [320, 1200], [64, 95, 97, 1000], 2),
            ("wreg_tanh", [392, 400, 416], [8, 200, 256], [64, 97, 1000], 2),
            ("dma13", [192, 200, 224, 304, 1200], [4, 204, 208, 416, 624], [1, 63] + _span(127, 129) + _span(255, 257), 3),
            ("dma20", [192, 304, 400], [212, 320, 640], [1] + _span(255, 257) + [1000], 3),
            ("wide", [8, 40, 184], [4, 100, 208], [1] + _span(127, 129) + [1000], 3),
            ("tiled", [8, 184, 304], [212, 260, 400], [1] + _span(127, 129) + [300], 3),
            ("f32", [4, 36, 300], [4, 516, 132], [1] + _span(127, 129) + [300], 3)]


def _nt_case(route, i, K, N, M, force=None):
    """Strides, bias, output type and tanh of the i-th case of a route: every variant occurs on every route that allows it."""
    dt = "f32" if route == "f32" else "bf16"
    ch, kr32 = (4 if dt == "f32" else 8), _rup(K, 32)
    v = i % 3                                             # 0: packed; 1: lda and ldc wider; 2: every ld wider
    lda = K + (0, ch, 3 * ch)[v]
    if dt == "f32":
        ldb = K + (0, 0, 4)[v]
    elif route in ("wide", "tiled") and K >= 192:
        ldb = K + (0, 0, 8)[v]                            # below roundup32(K): what keeps K = 304 off the DMA kernel
    else:
        ldb = kr32 + (0, 0, 32)[v] if (route not in ("wide", "tiled") or i % 2 == 0) else K + (0, 0, 8)[v]
    # tanh: once on every other route, and on the fp32 kernel also at K = 4, where the carried bound is small enough for
    # tanhf's own error to show (what GEMM_TANH_ABS is measured on)
    tanh = route == "wreg_tanh" or (route in ("dma20", "f32", "dma13", "wide", "tiled") and i == 1) or (route == "f32" and i == 5)
    out = "bf16" if route.startswith("wreg") else ("f32" if dt == "f32" else ("bf16", "f32")[(i // 2) % 2])
    pad = 8 if out == "bf16" else 4
    ldc = _rup(N, pad) + (0, pad, 3 * pad)[v]
    if out == "bf16" and not route.startswith("wreg") and i % 5 == 4:
        ldc = _rup(N, 4) + 4 * (1 + (_rup(N, 4) // 4) % 2)    # a multiple of 4 that is no multiple of 8
    c = NTCase(route, dt, out, M, N, K, lda, ldb, ldc, tanh or i % 4 != 3, tanh)
    if force:
        c = c._replace(**force)
    if route.startswith("dma") and gemm_nt_route(c).startswith("wreg"):
        c = c._replace(out="f32", ldc=_rup(N, 4) + (0, 4, 12)[v])     # a weights-in-registers shape with fp32 out lands on the DMA kernel
    return c


def gemm_nt_cases():
    """The NT sweep: per route one value of each column per case, every listed value (and, over the rotations, most pairs)."""
    out = []
    for route, Ks, Ns, Ms, rot in _nt_rows():
        n = max(len(Ks), len(Ns), len(Ms))
        for r in range(rot):
            for i in range(n):
                out.append(_nt_case(route, r * n + i, Ks[i % len(Ks)], Ns[(i + r) % len(Ns)], Ms[(i + 2 * r) % len(Ms)]))
    # the weights-in-registers shapes with M < 64, N % 8 != 0 or fp32 out must land on the DMA kernel
    out += [_nt_case("dma13", 0, 304, 416, 63, dict(out="bf16", ldc=416)),
            _nt_case("dma13", 3, 320, 420, 79, dict(out="bf16", ldc=424)),
            _nt_case("dma13", 0, 304, 1208, 64, dict(out="f32", ldc=1208)),
            _nt_case("dma13", 1, 400, 200, 97, dict(out="f32", ldc=200)),
            _nt_case("dma20", 0, 400, 320, 63, dict(out="bf16", ldc=320)),
            _nt_case("dma20", 3, 416, 636, 95, dict(out="bf16", ldc=640)),
            # K = 304 with ldb = 304: B unpadded, the next row's data where the padding would be
            _nt_case("wide", 0, 304, 208, 129), _nt_case("wide", 3, 304, 100, 1000), _nt_case("wide", 1, 304, 4, 127),
            _nt_case("tiled", 0, 304, 400, 300),
            # K % 32 == 0 with B a column slice of a wider matrix, on the two kernels that have no such K in their row
            _nt_case("wide", 2, 64, 100, 128), _nt_case("tiled", 2, 160, 260, 129)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def gemm_nt_wreg_off_cases():
    """One case per weights-in-registers row that also runs with NT_WREG = 0 (then on the DMA kernel)."""
    cs = gemm_nt_cases()
    return [next(c for c in cs if c.route == r and c.M >= 95) for r in ("wreg5", "wreg3", "wreg_tanh")]


def gemm_tn_cases():
    rows = [("tn3_w320_n256", [16384, 16416], [264, 400], [280, 304, 320], 2),
            ("tn3_w320_n128", [16384, 16448], [8, 256], [304], 2),
            ("tn3_w160", [16384, 16416], [8, 136, 400], [8, 160, 168, 200], 2),
            ("tn2", [1] + _span(63, 65) + [1025, 16385], [8, 128, 136], [8, 160, 168, 304], 2),
            ("tn_f32", [1, 65, 1025], [4, 132], [4, 36, 300], 2)]
    out = []
    for route, Ms, Ns, Ks, rot in rows:
        n = max(len(Ms), len(Ns), len(Ks))
        for r in range(rot):
            for i in range(n):
                M, N, K = Ms[i % len(Ms)], Ns[(i + r) % len(Ns)], Ks[(i + 2 * r) % len(Ks)]
                j, ch = r * n + i, (4 if route == "tn_f32" else 8)
                v = j % 3
                c = TNCase(route, "f32" if route == "tn_f32" else "bf16", M, N, K, N + (0, ch, 2 * ch)[v], K + (0, 2 * ch, ch)[v],
                           K + (4, 8, 20)[v], j % 2 == 0)
                if c not in out:
                    out.append(c)
    return out


def gemm_tn_det_cases():
    """One case per TN route that also runs in deterministic mode."""
    cs = gemm_tn_cases()
    return [[c for c in cs if c.route == r and c.db][-1] for r in ("tn3_w320_n256", "tn3_w320_n128", "tn3_w160", "tn2", "tn_f32")]


def gemm_case_id(c):
    s = f"{c.route}-M{c.M}-N{c.N}-K{c.K}-ld{c.lda}.{c.ldb if isinstance(c, NTCase) else c.ldw}.{c.ldc}"
    if isinstance(c, NTCase):
        return s + f"-{c.out}" + ("-tanh" if c.tanh else "") + ("-bias" if c.bias else "")
    return s + ("-db" if c.db else "")


def gemm_lattice_worst(c):
    """Largest |partial sum| the lattice layer can produce: 3 * 3 per product, |bias| <= 4, |pre-fill| <= 5."""
    return 9 * c.K + 4 if isinstance(c, NTCase) else 9 * c.M + 5


def _lattice(shape, g, dev, lo=-3, hi=3):
    v = torch.randint(lo, hi + 1, shape, generator=g, device=dev).float()
    return v.masked_fill(torch.rand(shape, generator=g, device=dev) < 0.125, 0.0)    # 1/7 + 6/7 * 1/8: a quarter zeros


def _gauss(shape, g, dev, scale, dt):
    return (torch.randn(shape, generator=g, device=dev) * scale).to(dt).float()


def _operand(vals, rows_extra, ld, dt):
    """[rows + rows_extra, ld] buffer of NaN holding `vals` in its top left corner; returns (buffer, view)."""
    buf = torch.full((vals.shape[0] + rows_extra, ld), float("nan"), dtype=dt, device=vals.device)
    buf[:vals.shape[0], :vals.shape[1]] = vals.to(dt)
    return buf, buf[:vals.shape[0], :vals.shape[1]]


def gemm_nt_problem(c, layer, dev, seed=0):
    """Inputs, output buffer and fp64 reference of one NT case.  A: NaN in the slack columns and in two trailing rows.
    B: zero in columns [K, roundup32(K)) where ldb reaches that far (the contract of nr_gemm_nt), NaN in every other slack
    column and in one trailing row; with ldb < roundup32(K) the next row's data sits where the padding would be.
    C: NaN where the kernel must write, GEMM_SENTINEL in the slack columns and in two trailing rows."""
    g = torch.Generator(device=dev).manual_seed(1000 * seed + c.M + 7 * c.N + 13 * c.K)
    tdt, odt = _tdt(c.dt), _tdt(c.out)
    if layer == "lattice":
        # even rows of A are non-negative and every row of B has one sign: those sums grow like 2.25 K (256 .. 3744 for the
        # K of the tables), where bf16 steps are 2 .. 16 wide and ties are frequent; odd rows of A keep mixed signs
        A, B = _lattice((c.M, c.K), g, dev), _lattice((c.N, c.K), g, dev).abs()
        A[0::2] = A[0::2].abs()
        B = B * (torch.randint(0, 2, (c.N, 1), generator=g, device=dev).float() * 2 - 1)
        bias = torch.randint(-4, 5, (c.N,), generator=g, device=dev).float() if c.bias else None
    else:
        A, B = _gauss((c.M, c.K), g, dev, 0.5, tdt), _gauss((c.N, c.K), g, dev, 0.1, tdt)
        bias = torch.randn(c.N, generator=g, device=dev) * 0.1 if c.bias else None
    abuf, a = _operand(A, 2, c.lda, tdt)
    bbuf, b = _operand(B, 1, c.ldb, tdt)
    kr32 = _rup(c.K, 32)
    if c.ldb >= kr32:
        bbuf[:c.N, c.K:kr32] = 0
    cbuf = torch.full((c.M + 2, c.ldc), GEMM_SENTINEL, dtype=odt, device=dev)
    cbuf[:c.M, :c.N] = float("nan")
    pre = A.double() @ B.double().t()
    S = A.double().abs() @ B.double().abs().t()
    if bias is not None:
        pre, S = pre + bias.double(), S + bias.double().abs()
    return SimpleNamespace(c=c, layer=layer, a=a, b=b, abuf=abuf, bbuf=bbuf, bias=bias, cbuf=cbuf, before=cbuf.clone(),
                           ref=torch.tanh(pre) if c.tanh else pre, S=S, terms=c.K)


def gemm_tn_problem(c, layer, dev, seed=0, M=None):
    """Inputs, pre-filled outputs and fp64 references of one TN case (M: a smaller row count for the host proof).  dC and A:
    NaN in the slack columns and in two trailing rows.  dW / db: integers where the kernel accumulates, GEMM_SENTINEL in
    the slack columns, in the trailing row of dW and in the four trailing elements of db."""
    M = M or c.M
    g = torch.Generator(device=dev).manual_seed(1000 * seed + c.M + 7 * c.N + 13 * c.K)
    tdt = _tdt(c.dt)
    if layer == "lattice":
        D, A = _lattice((M, c.N), g, dev), _lattice((M, c.K), g, dev)
    else:
        D, A = _gauss((M, c.N), g, dev, 0.1, tdt), _gauss((M, c.K), g, dev, 0.5, tdt)
    dcbuf, dc = _operand(D, 2, c.ldc, tdt)
    abuf, a = _operand(A, 2, c.lda, tdt)
    P = torch.randint(-5, 6, (c.N, c.K), generator=g, device=dev).float()
    Pb = torch.randint(-5, 6, (c.N,), generator=g, device=dev).float()
    wbuf = torch.full((c.N + 1, c.ldw), GEMM_SENTINEL, dtype=torch.float32, device=dev)
    wbuf[:c.N, :c.K] = P
    dbbuf = torch.full((c.N + 4,), GEMM_SENTINEL, dtype=torch.float32, device=dev)
    dbbuf[:c.N] = Pb
    return SimpleNamespace(c=c, layer=layer, dc=dc, a=a, dcbuf=dcbuf, abuf=abuf, P=P, Pb=Pb, wbuf=wbuf, dbbuf=dbbuf,
                           wbefore=wbuf.clone(), dbbefore=dbbuf.clone(), M=M,
                           ref=P.double() + D.double().t() @ A.double(), S=P.double().abs() + D.double().abs().t() @ A.double().abs(),
                           refb=Pb.double() + D.double().sum(0), Sb=Pb.double().abs() + D.double().abs().sum(0), terms=M)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def gemm_check_sentinels(buf, before, rows, cols):
    """Everything outside buf[:rows, :cols] is unchanged bit for bit (1-D buffers: outside buf[:rows])."""
    changed = _bits(buf) != _bits(before)
    if buf.dim() == 1:
        changed[:rows] = False
    else:
        changed[:rows, :cols] = False
    if bool(changed.any()):
        raise GemmCheckError("sentinel", f"{int(changed.sum())} elements outside the output changed, first at "
                                         f"{changed.nonzero()[0].tolist()}")


def gemm_check_values(got, ref, layer, S=None, terms=0, tanh=False):
    """One output region against its fp64 reference.  lattice: bit-equal to ref rounded (nearest even) to the output type,
    returns 0.  layer2: the elementwise bound of the header; returns the worst |error| / bound."""
    if bool(torch.isnan(got).any()):
        raise GemmCheckError(layer, f"{int(torch.isnan(got).sum())} NaN in the stored output, first at {torch.isnan(got).nonzero()[0].tolist()}")
    if layer == "lattice":
        bad = got != ref.to(got.dtype)
        if bool(bad.any()):
            i = tuple(bad.nonzero()[0].tolist())
            raise GemmCheckError("lattice", f"{int(bad.sum())} of {bad.numel()} elements differ, first at {i}: got {float(got[i])}, "
                                            f"exact {float(ref[i])}")
        return 0.0
    bound = gemm_layer2_bound(ref, S, terms, got.dtype, GEMM_TANH_ABS if tanh else 0.0)
    diff = (got.double() - ref).abs()
    ratio = torch.where(diff > 0, diff / bound, torch.zeros_like(diff))
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise GemmCheckError("layer2", f"|error| / bound = {worst:.3g} at {i}: got {float(got[i])!r}, fp64 {float(ref[i])!r}, bound {float(bound[i]):.3g}")
    return worst


def gemm_layer2_bound(ref, S, terms, dtype, tanh_abs=0.0):
    e = (terms + 2) * GEMM_U * S + tanh_abs
    return e if dtype == torch.float32 else 2.0 ** -8 * ref.abs() + e * (1 + 2.0 ** -8)


def gemm_check_nt(p):
    """Sentinels, no NaN, values: the whole check of one NT run.  Returns the worst layer-2 ratio (0 on the lattice)."""
    c = p.c
    gemm_check_sentinels(p.cbuf, p.before, c.M, c.N)
    return gemm_check_values(p.cbuf[:c.M, :c.N], p.ref, p.layer, p.S, p.terms, c.tanh)


def gemm_check_tn(p):
    c = p.c
    gemm_check_sentinels(p.wbuf, p.wbefore, c.N, c.K)
    gemm_check_sentinels(p.dbbuf, p.dbbefore, c.N if c.db else 0, 0)
    worst = gemm_check_values(p.wbuf[:c.N, :c.K], p.ref, p.layer, p.S, p.terms)
    if c.db:
        worst = max(worst, gemm_check_values(p.dbbuf[:c.N], p.refb, p.layer, p.Sb, p.terms))
    return worst


def gemm_tanh_excess(p):
    """Worst |error| beyond the carried pre-activation bound of a tanh case (what GEMM_TANH_ABS has to cover), fp32 out."""
    c = p.c
    got = p.cbuf[:c.M, :c.N]
    return float(((got.double() - p.ref).abs() - gemm_layer2_bound(p.ref, p.S, p.terms, got.dtype)).max())

H = sys.modules[__name__]          # the tests below (and the two files that import this one) address the part above as H


# ------------------------------------------------------------------------------------------ the GPU tests
class _opt:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = _lib.get_option(self.name)
        _lib.set_option(self.name, self.value)

    def __exit__(self, *a):
        _lib.set_option(self.name, self.old)


def _profiled(call):
    """(return code, labels launched) of one library call."""
    _lib.prof_enable(1)
    try:
        _lib.prof_collect()
        rc = call()
        torch.cuda.synchronize()
        return rc, set(_lib.prof_collect().keys())
    finally:
        _lib.prof_enable(0)


def _nt_call(c, p, a_ptr=None, **over):
    v = dict(lda=c.lda, ldb=c.ldb, ldc=c.ldc, M=c.M, N=c.N, K=c.K)
    v.update(over)
    return lambda: _lib.lib().nr_gemm_nt(CODE[c.dt], a_ptr or p.abuf.data_ptr(), v["lda"], p.bbuf.data_ptr(), v["ldb"], _lib.ptr(p.bias),
                                         int(c.tanh), p.cbuf.data_ptr(), v["ldc"], CODE[c.out], v["M"], v["N"], v["K"], ops._stream())


def _tn_call(c, p, dc_ptr=None, **over):
    v = dict(ldc=c.ldc, lda=c.lda, ldw=c.ldw, M=c.M, N=c.N, K=c.K)
    v.update(over)
    return lambda: _lib.lib().nr_gemm_tn(CODE[c.dt], dc_ptr or p.dcbuf.data_ptr(), v["ldc"], p.abuf.data_ptr(), v["lda"], p.wbuf.data_ptr(),
                                         v["ldw"], p.dbbuf.data_ptr() if c.db else 0, v["M"], v["N"], v["K"], ops._stream())


def _run_nt(c, layer, label):
    """One NT case on one layer, twice: label, sentinels, values, run-to-run bit equality.  Returns (problem, ratio)."""
    p = H.gemm_nt_problem(c, layer, DEV)
    rc, labels = _profiled(_nt_call(c, p))
    _lib.check(rc, "nr_gemm_nt")
    assert labels == {label}, (labels, label)
    ratio = H.gemm_check_nt(p)
    first = p.cbuf.clone()
    p.cbuf.copy_(p.before)
    _lib.check(_nt_call(c, p)(), "nr_gemm_nt")
    torch.cuda.synchronize()
    assert torch.equal(H._bits(first), H._bits(p.cbuf)), "two runs differ"
    return p, ratio


@pytest.mark.parametrize("c", H.gemm_nt_cases(), ids=H.gemm_case_id)
def test_nt_route(c):
    for layer in (("layer2",) if c.tanh else ("lattice", "layer2")):
        p, ratio = _run_nt(c, layer, H.gemm_nt_label(c))
        if layer == "layer2":
            print(f"\nL2 {c.route} {c.out} ratio {ratio:.4f}" + (f" tanh_excess {H.gemm_tanh_excess(p):.3e}" if c.tanh else ""))


@pytest.mark.parametrize("c", H.gemm_nt_wreg_off_cases(), ids=H.gemm_case_id)
def test_nt_weights_in_registers_against_the_dma_kernel(c):
    """NT_WREG = 0 sends the same call to the LDS-DMA kernel: both exact on the lattice, hence bit-equal to each other (the
    tanh row has no lattice layer: there both stay inside the layer-2 bound)."""
    layer = "layer2" if c.tanh else "lattice"
    p1, _ = _run_nt(c, layer, H.gemm_nt_label(c))
    with _opt("NT_WREG", 0):
        route = "dma13" if H._rup(c.N, 208) // 208 * 13 < H._rup(c.N, 320) // 320 * 20 else "dma20"
        p0, _ = _run_nt(c, layer, H.gemm_nt_label(c, route))
    if layer == "lattice":
        assert torch.equal(H._bits(p1.cbuf), H._bits(p0.cbuf))


@pytest.mark.parametrize("c", H.gemm_tn_cases(), ids=H.gemm_case_id)
def test_tn_route(c):
    for layer in ("lattice", "layer2"):
        p = H.gemm_tn_problem(c, layer, DEV)
        rc, labels = _profiled(_tn_call(c, p))
        _lib.check(rc, "nr_gemm_tn")
        assert labels == {H.gemm_tn_label(c)}, labels
        ratio = H.gemm_check_tn(p)
        if layer == "layer2":
            print(f"\nL2 {c.route} f32 ratio {ratio:.4f}")


@pytest.mark.parametrize("c", H.gemm_tn_det_cases(), ids=H.gemm_case_id)
def test_tn_deterministic_mode_is_bit_equal_on_the_lattice(c):
    """Integers are exact in the 2^-36 fixed-point table as well: the deterministic result equals the atomic one bit for bit."""
    p = H.gemm_tn_problem(c, "lattice", DEV)
    _lib.check(_tn_call(c, p)(), "nr_gemm_tn")
    torch.cuda.synchronize()
    H.gemm_check_tn(p)
    q = H.gemm_tn_problem(c, "lattice", DEV)
    need = (c.N - 1) * c.ldw + c.K + c.N
    ops.set_deterministic(True, elements=need - 1)          # one element short: refused, which also shows that the mode is on
    try:
        rc, labels = _profiled(_tn_call(c, q))
        assert rc != 0 and "deterministic" in _lib.last_error() and labels == set()
        ops.set_deterministic(True, elements=need)
        rc, labels = _profiled(_tn_call(c, q))
    finally:
        ops.set_deterministic(False)
    _lib.check(rc, "nr_gemm_tn")
    assert H.gemm_tn_label(c) in labels, labels
    H.gemm_check_tn(q)
    assert torch.equal(H._bits(p.wbuf), H._bits(q.wbuf)) and torch.equal(H._bits(p.dbbuf), H._bits(q.dbbuf))


_NT_BAD = H.NTCase("tiled", "bf16", "bf16", 16, 24, 64, 64, 64, 24, True, False)
_TN_BAD = H.TNCase("tn2", "bf16", 16, 24, 64, 24, 64, 72, True)


@pytest.mark.parametrize("what,over", [("K", dict(K=60)), ("ldb", dict(ldb=68)), ("lda", dict(lda=68)), ("ldc", dict(ldc=26)),
                                        ("M", dict(M=0)), ("align", None)])
def test_nt_refuses_before_any_launch(what, over):
    """K, lda or ldb no multiple of the 16-byte chunk, ldc % 4 != 0, an operand off a 16-byte boundary, M = 0: an error code, a
    message, no kernel, the NaN pre-fill intact."""
    c = _NT_BAD
    p = H.gemm_nt_problem(c, "lattice", DEV)
    call = _nt_call(c, p, a_ptr=p.abuf.data_ptr() + 2) if over is None else _nt_call(c, p, **over)
    rc, labels = _profiled(call)
    assert rc != 0 and _lib.last_error() and labels == set(), (what, rc, labels)
    assert torch.equal(H._bits(p.cbuf), H._bits(p.before))


@pytest.mark.parametrize("what,over", [("K", dict(K=60)), ("N", dict(N=20)), ("ldc", dict(ldc=28)), ("lda", dict(lda=68)), ("M", dict(M=0)),
                                        ("align", None)])
def test_tn_refuses_before_any_launch(what, over):
    c = _TN_BAD
    p = H.gemm_tn_problem(c, "lattice", DEV)
    call = _tn_call(c, p, dc_ptr=p.dcbuf.data_ptr() + 2) if over is None else _tn_call(c, p, **over)
    rc, labels = _profiled(call)
    assert rc != 0 and _lib.last_error() and labels == set(), (what, rc, labels)
    assert torch.equal(H._bits(p.wbuf), H._bits(p.wbefore)) and torch.equal(H._bits(p.dbbuf), H._bits(p.dbbefore))

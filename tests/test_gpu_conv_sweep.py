"""GPU: every kernel route of NAML's title convolution -- nr_conv1d_k3_fwd, nr_conv1d_k3_bwd, nr_conv1d_k3_bwd_table
(csrc/nr_api.hip), the kernels of csrc/nr_convtab.hip, conv_rows_kernel and the ROWS_IM2COL3 loader of csrc/nr_gemm.hip, and
the three pack kernels -- against fp64.  The case tables, the reference, the checker and the route predictor are the first
part of this file ("title-convolution sweep"; plain torch, importable without a GPU); tests/test_conv_sweep_host.py proves on
the CPU that the reference equals torch autograd and that the checker fails eleven mutants of a sound stand-in.  The two
input layers, the sentinels and the value checker are those of tests/test_gpu_gemm_sweep.py (imported as H).

The GEMM sweep covers dense rows only.  The convolution runs the same kernels on a gapped operand (RowSrc::gap = T: token
rows with a zero row between titles, a logical row is 3*Dp contiguous elements that overlap its neighbours), on the
ROWS_IM2COL3 row source with dropout hashed in the loader, in the "_needed" / "_live" variants that leave rows unwritten, and
the table gradient adds an ordered compaction, a counting sort with ranks and an owner-computes scatter.

Reference (fp64, from the operands as the kernel sees them):
  x[s,t,:]   = table[ids[s], t, :D]; with dropout round_dt(fp32(x) * fp32(1/(1-p))) where keep((s*T+t)*D + c), else 0
               -- elementwise and deterministic, so x_rows is compared bit for bit, zero rows and columns [D, Dp) included
  y[s,t,:]   = b + sum_tap W[:,:,tap] . x[s,t-1+tap,:]            zeros outside [0, T) of the SAME title
  dW[n,d,tap] = sum_{s,t} dy[s,t,n] x[s,t-1+tap,d],  db = sum dy   accumulated onto a pre-fill
  dx[s,t,:]  = sum_j W_j^T dy[s,t-j+1,:]  (bf16: rounded to nearest even, the kernel stores dx in the compute dtype)
  dtable[id, t*D+c] += sum over the occurrences of id, in batch order, of keep * scale * dx
               for id in [1, V) and a set seq_nz flag (or none given); row 0 and untouched rows stay bit-unchanged

lattice: integers -3..3, p = 0.5 (scale exactly 2): every result an exact integer, compared bit for bit (bf16 y: the fp64
value rounded to nearest even; bf16 dx rounded before the exact sum).  Titles with an even id are non-negative and every
filter has one sign, so that sums leave the 8-bit significand and ties are frequent (the rounding mode is pinned).
layer2: Gaussian operands (0.5 / 0.1, rounded to the compute dtype), a dy representable in that dtype, p = 0.2.  Bounds, with
u = 2^-24 and S the same sum over absolute values:
  y   : (3D + 1 + 2) u S, S = |X||W|^T + |b|; bf16 out: 2^-8 |ref| on top (H.gemm_layer2_bound): 3D products and the bias
        in one fp32 sum, "+ 2" for the bias addition and the final rounding
  dW  : (n*T + 2) u S, S = |dy|^T|X| + |pre-fill|;   db: the same with S = sum |dy| + |pre-fill|
  dtable, k occurrences of the id:
        scale * sum_occ [r |dx| + (3N + 2) u S_occ (1 + r)] + (k + 1) u scale sum_occ |dx| + u |pre-fill|
        r = 2^-8 (bf16) or 0, S_occ = |dy||W|.  Per occurrence: the GEMM's fp32 sum of 3N products ((3N + 2) u S_occ), its
        rounding to bf16 (r |dx|, which also scales the GEMM error: 1 + r); x * scale is one fp32 rounding, the k - 1
        additions of the run and the final read-add-store are k more, each relative to a partial sum that scale * sum |dx|
        bounds -- except the last, whose result also holds the value accumulated onto: u |pre-fill| (the planned bound
        lacked that term; a fp32 addition onto a pre-fill of 5 rounds by up to 2^-22 whatever the kernel does, which the CPU
        stand-in of the host file showed before any kernel ran).  Dropped elements add exactly zero: sum_occ runs over kept ones.

Checked per case: the labels conv_labels predicts (read from nr_api.hip and nr_launch_gemm_nt / _tn), sentinels and untouched
rows unchanged bit for bit, no NaN stored (x_rows starts as NaN, so reading a row a "_needed" kernel left unwritten poisons
a result; the workspaces start as 0xff bytes), lattice bit-equal, layer2 inside its bound, forward and dtable bit-equal
across two runs.  Routes and measured ratios: DESIGN.md "Title convolution: routes as verified and the sweep".
"""
import collections
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import test_gpu_gemm_sweep as H
from newsrecommendation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------ title-convolution sweep
CONV_P = {"lattice": 0.5, "layer2": 0.2}
CONV_V = 19                      # table rows of the forward / dW cases
CONV_SEED = 20231

# dt: compute dtype; ids: "mixed" (every third 0), "same", "zeros", "strided" (a column of an [n, 3] tensor); xr: x_rows given;
# p: dropout on; ws: bwd_ws given; nz: seq_nz given (truthful: the titles whose dy is not zero); needed: seq_needed given
# (those same titles); dyp: titles with a non-zero dy ("all", "zero", "first", "last", "alt"); opt: a library switch set to 1
ConvCase = collections.namedtuple("ConvCase", "dt n T D Dp N ids xr p ws nz needed dyp opt")
# ids here also "oob" (mixed, with the values V and -1); nz: seq_nz given, every fourth title flagged 0 although its dy is not
# zero; off: dtable starts one float into its buffer (4-byte aligned only)
TabCase = collections.namedtuple("TabCase", "dt n T D N ldwt V ids p nz off")


def _cc(dt, n, T, D, Dp, N, ids="mixed", xr=True, p=True, ws=False, nz=False, needed=False, dyp="all", opt=""):
    return ConvCase(dt, n, T, D, Dp, N, ids, xr, p, ws, nz, needed, dyp, opt)


def conv_small_cases():
    """Forward + dW below the slab threshold: T in {1, 2, 5, 30} and n*T in {T, 255, 256, 257}; K = 3*Dp on both sides of 192
    and of a multiple of 32 (72/72: K = 216 must take the generic gapped kernel); N over both chunk widths."""
    b, f = "bf16", "f32"
    return [_cc(b, 257, 1, 4, 8, 8), _cc(b, 5, 2, 5, 8, 200, "same", p=False), _cc(b, 51, 5, 20, 24, 208, ws=True),
            _cc(b, 1, 30, 50, 64, 216, "same"), _cc(b, 64, 4, 64, 64, 320, "strided", p=False, ws=True, dyp="alt"),
            _cc(b, 85, 3, 72, 72, 400), _cc(b, 257, 1, 96, 96, 200, "zeros"), _cc(b, 9, 30, 300, 320, 400, dyp="zero"),
            _cc(b, 1, 1, 5, 8, 8, "same", xr=False), _cc(b, 51, 5, 50, 64, 208, xr=False),
            _cc(b, 9, 30, 300, 320, 400, "strided", xr=False, p=False), _cc(b, 128, 2, 20, 24, 216, "zeros", xr=False),
            _cc(f, 257, 1, 4, 4, 8, xr=False), _cc(f, 1, 2, 5, 8, 200, "same", xr=False, p=False),
            _cc(f, 51, 5, 50, 52, 320, xr=False, dyp="alt"), _cc(f, 9, 30, 300, 300, 400, "strided", xr=False),
            _cc(f, 5, 1, 4, 4, 8), _cc(f, 64, 4, 20, 24, 216, "strided"), _cc(f, 2, 30, 72, 72, 208, "zeros", p=False),
            _cc(f, 51, 5, 64, 64, 400, "same", dyp="first")]


def conv_slab_cases():
    """bf16 with x_rows, n*T % 32 == 0, n*T >= 16384, T <= 32, N % 8 == 0: each shape without bwd_ws (plain gemm_tn3, gap=T),
    with bwd_ws (title_flags, gemm_tn3_live) and with seq_nz given; then with seq_needed; T = 33 (tn3-eligible, no slab
    shape); n*T % 32 != 0 (generic gapped TN); one slab case again under NO_SLABS."""
    shapes = [(512, 32, 50, 64, 64, "mixed"), (513, 32, 96, 96, 264, "strided"), (560, 30, 64, 64, 264, "mixed"),
              (2048, 8, 90, 96, 64, "same")]
    pats = [("all", "alt", "first"), ("zero", "last", "alt"), ("first", "zero", "all"), ("last", "all", "zero")]
    out = []
    for i, ((n, T, D, Dp, N, ids), (d0, d1, d2)) in enumerate(zip(shapes, pats)):
        out += [_cc("bf16", n, T, D, Dp, N, ids, p=i != 1, dyp=d0), _cc("bf16", n, T, D, Dp, N, ids, p=i != 2, ws=True, dyp=d1),
                _cc("bf16", n, T, D, Dp, N, ids, p=i != 3, ws=True, nz=True, dyp=d2)]
    out += [_cc("bf16", 512, 32, 50, 64, 64, ws=True, needed=True, dyp="alt"),
            _cc("bf16", 513, 32, 96, 96, 264, "strided", p=False, ws=True, needed=True, dyp="first"),
            _cc("bf16", 560, 30, 64, 64, 264, ws=True, needed=True, dyp="last"),
            _cc("bf16", 2048, 8, 90, 96, 64, "same", ws=True, nz=True, needed=True, dyp="alt"),
            _cc("bf16", 512, 33, 50, 64, 64, ws=True), _cc("bf16", 561, 30, 64, 64, 64, ws=True, dyp="alt"),
            _cc("bf16", 512, 32, 50, 64, 64, ws=True, needed=True, dyp="first", opt="NO_SLABS")]
    return out


def conv_refused_case():
    """seq_needed on a slab shape without bwd_ws: the forward runs, the backward must be refused."""
    return _cc("bf16", 512, 32, 50, 64, 64, needed=True, dyp="alt")


def conv_table_cases():
    """Table gradient.  Compact route: bf16, 3N >= 192, ldwt >= roundup32(3N).  D = 5 and the offset dtable: scalar scatter;
    T*D = 1050: its second grid row; T*D = 9000 > 4096: the vector scatter's; n = 300 of one id: more than 256 occurrences;
    n = 1025: two titles per thread of the compaction."""
    b, f = "bf16", "f32"
    return [TabCase(b, 300, 5, 64, 64, 192, 19, "same", True, False, 0), TabCase(b, 1025, 2, 4, 72, 224, 300, "mixed", True, True, 0),
            TabCase(b, 2048, 1, 5, 64, 192, 19, "mixed", False, False, 0), TabCase(b, 1, 30, 35, 72, 224, 2, "same", True, False, 0),
            TabCase(b, 9, 30, 300, 64, 192, 19, "strided", True, False, 0), TabCase(b, 300, 3, 64, 64, 192, 19, "zeros", True, False, 0),
            TabCase(b, 1025, 2, 64, 64, 224, 19, "oob", True, True, 0), TabCase(b, 40, 5, 4, 64, 192, 19, "mixed", True, False, 1),
            TabCase(b, 300, 5, 4, 8, 24, 19, "same", True, False, 0), TabCase(b, 1025, 2, 5, 56, 168, 300, "mixed", True, True, 0),
            TabCase(b, 1, 30, 35, 8, 32, 2, "same", False, False, 0), TabCase(b, 9, 30, 300, 56, 192, 19, "strided", True, False, 0),
            TabCase(b, 2048, 1, 64, 72, 216, 19, "oob", False, False, 0), TabCase(b, 300, 2, 5, 8, 24, 19, "zeros", True, False, 0),
            TabCase(f, 300, 5, 64, 64, 192, 19, "same", True, False, 0), TabCase(f, 1025, 2, 5, 8, 24, 300, "mixed", True, True, 0),
            TabCase(f, 1, 30, 35, 56, 168, 2, "same", False, False, 0), TabCase(f, 9, 30, 300, 64, 196, 19, "strided", True, False, 0),
            TabCase(f, 2048, 1, 4, 72, 216, 19, "oob", True, True, 0), TabCase(f, 40, 5, 64, 8, 24, 19, "mixed", True, False, 1),
            TabCase(f, 300, 3, 4, 8, 24, 19, "zeros", False, False, 0)]


def conv_case_id(c):
    if isinstance(c, TabCase):
        return (f"tab-{c.dt}-n{c.n}-T{c.T}-D{c.D}-N{c.N}-ld{c.ldwt}-V{c.V}-{c.ids}" + ("-p" if c.p else "") + ("-nz" if c.nz else "")
                + ("-off" if c.off else ""))
    return (f"{c.dt}-n{c.n}-T{c.T}-D{c.D}.{c.Dp}-N{c.N}-{c.ids}-dy_{c.dyp}" + ("-xr" if c.xr else "") + ("-p" if c.p else "")
            + ("-ws" if c.ws else "") + ("-nz" if c.nz else "") + ("-needed" if c.needed else "") + (f"-{c.opt}" if c.opt else ""))


def conv_slab_shape(c):
    """conv_slab_shape of nr_api.hip (with tn3::eligible): the shapes whose backward contracts live 32-row slabs only."""
    M = c.n * c.T
    return (c.opt != "NO_SLABS" and c.dt == "bf16" and c.xr and M % 32 == 0 and c.T <= 32 and c.N % 8 == 0 and M >= 16384 and c.N >= 8
            and c.Dp % 8 == 0)


def conv_labels(c):
    """The profiler labels a case must show, as nr_api.hip and nr_launch_gemm_nt / _tn decide them.  ConvCase: {"fwd": [...],
    "dw": [...] or None where the backward is refused}; TabCase: {"dtable": [...]}."""
    if isinstance(c, TabCase):
        K, M = 3 * c.N, c.n * c.T
        compact = c.dt == "bf16" and K >= 192 and c.ldwt >= H._rup(K, 32)
        gemm = (f"gemm_nt_dma_live[bf16,epi=0,Mmax={M},N={c.D},K={K},gap={c.T}]" if compact
                else f"gemm_nt[{c.dt},rows=0,epi=0,M={M},N={c.D},K={K}]")
        return {"dtable": [f"conv_table_live[n={c.n},V={c.V}]", f"conv_table_stage[{c.dt},n={c.n},T={c.T},N={c.N}]", gemm,
                           f"sort_rows_by_id[Mmax={c.n},V={c.V}]", f"conv_table_rank[n={c.n}]",
                           f"conv_table_scatter[{c.dt},n={c.n},T={c.T},D={c.D},V={c.V}]"]}
    M, K, N = c.n * c.T, 3 * c.Dp, c.N
    slab = conv_slab_shape(c)
    if not c.xr:
        return {"fwd": [f"gemm_nt[{c.dt},rows=2,epi=0,M={M},N={N},K={K}]"], "dw": [f"gemm_tn[{c.dt},rows=2,M={M},N={N},K={K}]"]}
    skip = slab and c.needed
    fwd = [("conv_rows_needed[" if skip else "conv_rows[") + f"{c.dt},n={c.n},T={c.T},Dp={c.Dp}]"]
    if c.dt == "bf16" and K >= 192 and K % 32 == 0:          # ldb = K: the LDS-DMA kernel needs ldb >= roundup32(K)
        fwd.append(f"gemm_nt_dma_needed[bf16,epi=0,Mmax={M},N={N},K={K},gap={c.T}]" if skip
                   else f"gemm_nt_dma[bf16,epi=0,M={M},N={N},K={K},gap={c.T}]")
    else:
        fwd.append(f"gemm_nt[{c.dt},rows=0,epi=0,M={M},N={N},K={K}]")
    if slab and c.ws:
        dw = ([] if c.nz else [f"title_flags[n={c.n},L={c.T},N={N}]"]) + [f"gemm_tn3_live[bf16,Mmax={M},N={N},K={K},gap={c.T}]"]
    elif skip:
        dw = None
    elif c.dt == "bf16" and M % 32 == 0 and M >= 16384 and N % 8 == 0 and N >= 8 and c.Dp % 8 == 0:
        dw = [f"gemm_tn3[bf16,M={M},N={N},K={K},gap={c.T}]"]
    else:
        dw = [f"gemm_tn[{c.dt},rows=0,M={M},N={N},K={K}]"]
    return {"fwd": fwd, "dw": dw}


CONV_FAMILIES = ["conv_rows[", "conv_rows_needed[", "gemm_nt_dma[bf16,gap=T]", "gemm_nt_dma_needed[bf16,gap=T]", "gemm_nt[bf16,rows=0,",
                 "gemm_nt[bf16,rows=2,", "gemm_nt[f32,rows=2,", "gemm_nt[f32,rows=0,", "gemm_tn3[bf16,gap=T]", "gemm_tn3_live[bf16,gap=T]",
                 "title_flags[", "gemm_tn[bf16,rows=0,", "gemm_tn[bf16,rows=2,", "gemm_tn[f32,rows=2,", "gemm_tn[f32,rows=0,",
                 "conv_table_live[", "conv_table_stage[", "gemm_nt_dma_live[bf16,gap=T]", "sort_rows_by_id[", "conv_table_rank[",
                 "conv_table_scatter["]


def conv_label_family(label):
    """A label without its sizes: "gemm_nt_dma[bf16,epi=0,M=256,N=320,K=192,gap=4]" -> "gemm_nt_dma[bf16,gap=T]"."""
    name, args = label.rstrip("]").split("[")
    if name.startswith(("conv_", "sort_", "title_")):
        return name + "["
    args = args.split(",")
    keep = ",".join(a for a in args if a in ("bf16", "f32") or a.startswith("rows="))
    return f"{name}[{keep},gap=T]" if args[-1].startswith("gap=") and args[-1] != "gap=0" else f"{name}[{keep},"


def _scale32(p):
    """nr_make_drop's 1.0f / (1.0f - p), in fp32 arithmetic."""
    one = torch.ones((), dtype=torch.float32)
    return float(one / (one - torch.tensor(p, dtype=torch.float32))) if p > 0 else 1.0


def conv_keep(count, p, seed, dev, g):
    """Keep mask of element indices [0, count): the library's own draw on the GPU, any Bernoulli draw on the CPU."""
    if p == 0:
        return torch.ones(count, device=dev)
    if torch.device(dev).type == "cuda":
        return ops.dropout_mask(count, p, seed, dev)
    return (torch.rand(count, generator=g, device=dev) >= p).float()


def conv_ids(mode, n, V, g, dev):
    if mode == "zeros":
        return torch.zeros(n, dtype=torch.int32, device=dev)
    if mode == "same":
        return torch.full((n,), V - 1, dtype=torch.int32, device=dev)
    ids = torch.randint(0, V, (n,), generator=g, device=dev, dtype=torch.int32)
    ids[::3] = 0
    if mode == "oob":                     # the table gradient skips such titles; never given to the forward
        ids[1::7] = V
        ids[2::7] = -1
    if mode == "strided":
        wide = torch.randint(0, V, (n, 3), generator=g, device=dev, dtype=torch.int32)
        wide[:, 1] = ids
        return wide[:, 1]
    return ids


def conv_live_titles(pattern, n, dev):
    live = torch.zeros(n, dtype=torch.bool, device=dev)
    if pattern == "all":
        live[:] = True
    elif pattern == "first":
        live[0] = True
    elif pattern == "last":
        live[n - 1] = True
    elif pattern == "alt":
        live[::2] = True
    return live


def conv_operand(x, keep, p, dt):
    """x [.., D] (values of the compute dtype, held in fp32) -> the GEMM operand: round_dt(fp32(x) * fp32 scale) where kept."""
    if p == 0:
        return x
    xs = (x * torch.tensor(_scale32(p), dtype=torch.float32, device=x.device)).to(H._tdt(dt)).float()
    return torch.where(keep != 0, xs, torch.zeros_like(xs))          # (a dropped element is +0, not -0: x_rows is compared bit for bit)


def conv_im2col(xop):
    """[n, T, Dp] -> [n*T, 3*Dp]: taps t-1, t, t+1 of the same title, zeros outside."""
    n, T, Dp = xop.shape
    z = torch.zeros_like(xop[:, :1])
    return torch.cat([torch.cat([z, xop[:, :-1]], 1), xop, torch.cat([xop[:, 1:], z], 1)], 2).reshape(n * T, 3 * Dp)


def conv_pack_w(w, Dp):
    """nr_pack_conv_w: [N, D, 3] -> [N, 3*Dp], dst[n, tap*Dp + d] = w[n, d, tap], zero in [D, Dp)."""
    N, D, _ = w.shape
    out = torch.zeros(N, 3, Dp, dtype=w.dtype, device=w.device)
    out[:, :, :D] = w.permute(0, 2, 1)
    return out.reshape(N, 3 * Dp)


def conv_pack_w_t(w, ld):
    """nr_pack_conv_w_t: [N, D, 3] -> [D, ld], dst[d, j*N + n] = w[n, d, 2 - j], zero in [3N, ld)."""
    N, D, _ = w.shape
    out = torch.zeros(D, ld, dtype=w.dtype, device=w.device)
    out[:, :3 * N] = w.flip(2).permute(1, 2, 0).reshape(D, 3 * N)
    return out


def _inputs(layer, dt, V, T, D, N, n, g, dev):
    """table [V, T, D] (row 0 zero), w [N, D, 3], b [N], dy [n, T, N]: values of the compute dtype, held in fp32."""
    tdt = H._tdt(dt)
    if layer == "lattice":
        tab, w, dy = H._lattice((V, T, D), g, dev), H._lattice((N, D, 3), g, dev).abs(), H._lattice((n, T, N), g, dev)
        sign = torch.randint(0, 2, (N,), generator=g, device=dev).float() * 2 - 1
        tab[0::2] = tab[0::2].abs()
        w = w * sign[:, None, None]
        dy[0::2] = dy[0::2].abs() * sign                  # dx = sum |w||dy| on even titles: leaves bf16's 8 bits
        b = torch.randint(-4, 5, (N,), generator=g, device=dev).float()
    else:
        tab, w = H._gauss((V, T, D), g, dev, 0.5, tdt), H._gauss((N, D, 3), g, dev, 0.1, tdt)
        dy, b = H._gauss((n, T, N), g, dev, 0.1, tdt), torch.randn(N, generator=g, device=dev) * 0.1
    tab[0] = 0
    return tab, w, b, dy


def _nan_rows(vals, extra, dt):
    """vals [R, C] + `extra` trailing rows of NaN; returns the buffer."""
    buf = torch.full((vals.shape[0] + extra, vals.shape[1]), float("nan"), dtype=dt, device=vals.device)
    buf[:vals.shape[0]] = vals.to(dt)
    return buf


def conv_problem(c, layer, dev, n=None):
    """Buffers and fp64 references of one forward + dW case (n: a smaller title count for the host proof).  Inputs: NaN in
    trailing rows.  y: H.GEMM_SENTINEL everywhere (two trailing rows stay so); x_rows: NaN, two trailing sentinel rows;
    dw_pack / db: integers, a trailing sentinel row / four trailing sentinels."""
    n = n or c.n
    T, D, Dp, N, V, tdt = c.T, c.D, c.Dp, c.N, CONV_V, H._tdt(c.dt)
    g = torch.Generator(device=dev).manual_seed(n + 7 * T + 13 * D + 17 * N)
    p = CONV_P[layer] if c.p else 0.0
    tab, w, b, dy = _inputs(layer, c.dt, V, T, D, N, n, g, dev)
    ids = conv_ids(c.ids, n, V, g, dev)
    live = conv_live_titles(c.dyp, n, dev)
    dy = torch.where(live[:, None, None], dy, torch.zeros_like(dy))
    keep_flat = conv_keep(n * T * (D if torch.device(dev).type == "cuda" else Dp), p, CONV_SEED, dev, g)
    keep = keep_flat[:n * T * D].view(n, T, D)
    xop = torch.zeros(n, T, Dp, device=dev)
    xop[:, :, :D] = conv_operand(tab[ids.long()], keep, p, c.dt)
    X, Wp = conv_im2col(xop).double(), conv_pack_w(w, Dp).double()
    dy2 = dy.reshape(n * T, N).double()
    P = torch.randint(-5, 6, (N, 3 * Dp), generator=g, device=dev).float()
    Pb = torch.randint(-5, 6, (N,), generator=g, device=dev).float()
    tabp = torch.zeros(V, T, Dp, device=dev)
    tabp[:, :, :D] = tab
    q = SimpleNamespace(c=c, layer=layer, n=n, p=p, seed=CONV_SEED, ids=ids, live=live, keep=keep, keep_flat=keep_flat, tab=tab, w=w,
                        b=b, dy=dy, P=P, Pb=Pb, skips=conv_slab_shape(c) and c.needed)
    q.tabbuf = _nan_rows(tabp.reshape(V, T * Dp), 1, tdt)
    q.wpbuf = _nan_rows(conv_pack_w(w, Dp), 1, tdt)
    q.bbuf = torch.cat([b, torch.full((4,), float("nan"), device=dev)])
    q.dybuf = _nan_rows(dy.reshape(n * T, N), 2, tdt)
    q.flags = live.to(torch.int32)
    q.ybuf = torch.full((n * T + 2, N), H.GEMM_SENTINEL, dtype=tdt, device=dev)
    rows = n * (T + 1) + 1
    q.xbuf = torch.full((rows + 2, Dp), float("nan"), dtype=tdt, device=dev)
    q.xbuf[rows:] = H.GEMM_SENTINEL
    q.wbuf = torch.full((N + 1, 3 * Dp), H.GEMM_SENTINEL, dtype=torch.float32, device=dev)
    q.wbuf[:N] = P
    q.dbbuf = torch.full((N + 4,), H.GEMM_SENTINEL, dtype=torch.float32, device=dev)
    q.dbbuf[:N] = Pb
    q.ybefore, q.xbefore, q.wbefore, q.dbbefore = q.ybuf.clone(), q.xbuf.clone(), q.wbuf.clone(), q.dbbuf.clone()
    xr = torch.zeros(rows, Dp, device=dev)
    xr[:n * (T + 1)].view(n, T + 1, Dp)[:, 1:] = xop
    q.xrows_ref = xr.to(tdt)
    q.y_ref, q.y_S = X @ Wp.t() + b.double(), X.abs() @ Wp.abs().t() + b.double().abs()
    q.dw_ref, q.dw_S = P.double() + dy2.t() @ X, P.double().abs() + dy2.abs().t() @ X.abs()
    q.db_ref, q.db_S = Pb.double() + dy2.sum(0), Pb.double().abs() + dy2.abs().sum(0)
    return q


def conv_dtable_ref(ids, dy, w, keep, scale, V, dt, layer, seq_nz=None):
    """fp64 reference of the table gradient without the pre-fill.  ids [n]; dy [n, T, N]; w [N, D, 3]; keep [n, T, D].  Returns
    (ref [V, T*D], bound without the pre-fill term [V, T*D], touched [V] bool)."""
    n, T, N = dy.shape
    D, dev = w.shape[1], dy.device
    Wt = conv_pack_w_t(w, 3 * N).double()                         # [D, 3N]: dx = im2col(dy) . Wt^T
    G = conv_im2col(dy)
    dx, S = (G.double() @ Wt.t()).view(n, T, D), (G.double().abs() @ Wt.abs().t()).view(n, T, D)
    r = 2.0 ** -8 if dt == "bf16" else 0.0
    if layer == "lattice" and dt == "bf16":
        dx = dx.float().to(torch.bfloat16).double()               # exact integers below 2^24: one rounding, to nearest even
    good = (ids > 0) & (ids < V)
    if seq_nz is not None:
        good = good & (seq_nz != 0)
    kp = keep.double() * scale * good[:, None, None].double()
    idx = torch.where(good, ids, torch.zeros_like(ids)).long()
    acc = lambda v: torch.zeros(V, T * D, dtype=torch.float64, device=dev).index_add_(0, idx, v.reshape(n, T * D))
    k = torch.zeros(V, dtype=torch.float64, device=dev).index_add_(0, idx, good.double())
    ref, A = acc(kp * dx), acc(kp * dx.abs())
    bound = acc(kp * (r * dx.abs() + (3 * N + 2) * H.GEMM_U * S * (1 + r))) + (k[:, None] + 1) * H.GEMM_U * A
    return ref, bound, k > 0


def conv_table_problem(c, layer, dev, share=None):
    """Buffers and references of one table-gradient case.  dtable: [V + 2, T*D] floats starting c.off floats into a flat
    buffer; integers in rows < V, H.GEMM_SENTINEL in the two rows after, in front and behind.  share: a conv_problem whose
    ids, dy, filter, seed and keep mask are used (the forward and the table gradient of one layer)."""
    n, T, D, N, V, tdt = c.n, c.T, c.D, c.N, c.V, H._tdt(c.dt)
    g = torch.Generator(device=dev).manual_seed(n + 7 * T + 13 * D + 17 * N + 19 * V)
    p = CONV_P[layer] if c.p else 0.0
    if share is None:
        _, w, _, dy = _inputs(layer, c.dt, 1, T, D, N, n, g, dev)
        ids = conv_ids(c.ids, n, V, g, dev)
        keep = conv_keep(n * T * D, p, CONV_SEED + 1, dev, g).view(n, T, D)
        seed = CONV_SEED + 1
    else:
        w, dy, ids, keep, seed, p = share.w, share.dy, share.ids, share.keep, share.seed, share.p
    flags = None
    if c.nz:
        flags = torch.ones(n, dtype=torch.int32, device=dev)
        flags[::4] = 0
    q = SimpleNamespace(c=c, layer=layer, n=n, p=p, seed=seed, ids=ids, keep=keep, w=w, dy=dy, flags=flags)
    TD = T * D
    P = torch.randint(-5, 6, (V, TD), generator=g, device=dev).float()
    q.tflat = torch.full((c.off + (V + 2) * TD + 4,), H.GEMM_SENTINEL, dtype=torch.float32, device=dev)
    q.dtable = q.tflat[c.off:c.off + (V + 2) * TD].view(V + 2, TD)
    q.dtable[:V] = P
    q.tbefore = q.tflat.clone()
    q.dybuf = _nan_rows(dy.reshape(n * T, N), 2, tdt)
    q.wtbuf = _nan_rows(conv_pack_w_t(w, c.ldwt), 1, tdt)
    ref, bound, q.touched = conv_dtable_ref(ids, dy, w, keep, _scale32(p), V, c.dt, layer, flags)
    q.P, q.ref, q.bound = P, P.double() + ref, bound + H.GEMM_U * P.double().abs()
    return q


def _fail(layer, msg):
    raise H.GemmCheckError(layer, msg)


def conv_check_xrows(p):
    """x_rows bit for bit.  Under "needed" flags a title is either written whole, with the zero rows on both sides, or --
    if it is not needed itself -- left as it was."""
    c, n, T = p.c, p.n, p.c.T
    rows = n * (T + 1) + 1
    H.gemm_check_sentinels(p.xbuf, p.xbefore, rows, c.Dp)
    got = p.xbuf[:rows]
    row_ok = (H._bits(got) == H._bits(p.xrows_ref)).all(1)
    if not p.skips:
        if not bool(row_ok.all()):
            _fail("x_rows", f"{int((~row_ok).sum())} rows of x_rows differ, first {int((~row_ok).nonzero()[0])}")
        return
    blk_ok = row_ok[:n * (T + 1)].view(n, T + 1).all(1) & row_ok[T + 1::T + 1]
    untouched = torch.isnan(got[:n * (T + 1)].view(n, T + 1, c.Dp)[:, 1:]).all(2).all(1)
    bad = ~(blk_ok | (untouched & ~p.live))
    if bool(bad.any()):
        _fail("x_rows", f"{int(bad.sum())} titles of x_rows neither complete nor untouched and unneeded, first {int(bad.nonzero()[0])}")


def conv_check_y(p):
    """Sentinels, no row of a title that must be written left as the sentinel, values.  Returns the layer-2 ratio."""
    c, M = p.c, p.n * p.c.T
    H.gemm_check_sentinels(p.ybuf, p.ybefore, M, c.N)
    got = p.ybuf[:M]
    untouched = (H._bits(got) == H._bits(p.ybefore[:M])).all(1)
    must = p.live.repeat_interleave(c.T) if p.skips else torch.ones_like(untouched)
    if bool((untouched & must).any()):
        _fail("sentinel", f"{int((untouched & must).sum())} rows of y left unwritten, first {int((untouched & must).nonzero()[0])}")
    got = torch.where((untouched & ~must)[:, None], p.y_ref.to(got.dtype), got)
    return H.gemm_check_values(got, p.y_ref, p.layer, p.y_S, 3 * c.D + 1)


def conv_check_dw(p):
    c, K = p.c, 3 * p.c.Dp
    H.gemm_check_sentinels(p.wbuf, p.wbefore, c.N, K)
    H.gemm_check_sentinels(p.dbbuf, p.dbbefore, c.N, 0)
    terms = p.n * c.T
    return (H.gemm_check_values(p.wbuf[:c.N], p.dw_ref, p.layer, p.dw_S, terms),
            H.gemm_check_values(p.dbbuf[:c.N], p.db_ref, p.layer, p.db_S, terms))


def conv_check_dtable(p):
    c, V = p.c, p.c.V
    TD = c.T * c.D
    changed = H._bits(p.tflat) != H._bits(p.tbefore)
    changed[c.off:c.off + V * TD] = False
    if bool(changed.any()):
        _fail("sentinel", f"{int(changed.sum())} elements outside dtable changed, first at {int(changed.nonzero()[0])}")
    got = p.dtable[:V]
    still = (H._bits(got) != H._bits(p.P)).any(1) & ~p.touched
    if bool(still.any()):
        _fail("sentinel", f"rows {still.nonzero().flatten().tolist()[:8]} of dtable have no live title and changed")
    # the derived bound goes through the GEMM sweep's checker as (terms + 2) u S with terms = -1, S = bound / u
    return H.gemm_check_values(got, p.ref, p.layer, p.bound / H.GEMM_U, -1)


# ------------------------------------------------------------------------------------------ the GPU tests
CODE = H.CODE
_has = lambda labels, prefix: any(l.startswith(prefix) for l in labels)


def _ws_bytes(nbytes):
    """A workspace of that size, every byte 0xff (a NaN pattern in both operand types, -1 as an index)."""
    return torch.full(((int(nbytes) + 15) // 16 * 4,), -1, dtype=torch.int32, device=DEV)


def _desc(p, V=0):
    c = p.c
    d = _lib.ConvDesc(n=p.n, T=c.T, D=c.D, Dp=c.Dp, N=c.N, dtype=CODE[c.dt], table=p.tabbuf.data_ptr(), ids=p.ids.data_ptr(),
                      ids_stride=p.ids.stride(0), p_in=p.p, seed_in=p.seed, w_pack=p.wpbuf.data_ptr(), bias=p.bbuf.data_ptr(),
                      x_rows=p.xbuf.data_ptr() if c.xr else 0, ld_rows=c.Dp, seq_nz=p.flags.data_ptr() if c.nz else 0,
                      seq_needed=p.flags.data_ptr() if c.needed else 0, table_rows=V)
    if c.ws:
        p.ws = _ws_bytes(_lib.lib().nr_conv_workspace_bytes(C.byref(d)))
        d.bwd_ws, d.bwd_ws_bytes = p.ws.data_ptr(), p.ws.numel() * 4
    return d


def _fwd(p, d):
    return lambda: _lib.lib().nr_conv1d_k3_fwd(C.byref(d), p.ybuf.data_ptr(), ops._stream())


def _bwd(p, d):
    return lambda: _lib.lib().nr_conv1d_k3_bwd(C.byref(d), p.dybuf.data_ptr(), p.wbuf.data_ptr(), p.dbbuf.data_ptr(), ops._stream())


def _run_conv(c, layer):
    """Forward (twice) and dW of one case on one layer; returns (problem, y ratio, dW ratio, db ratio)."""
    p = conv_problem(c, layer, DEV)
    d, want = _desc(p), conv_labels(c)
    rc, labels = H._profiled(_fwd(p, d))
    _lib.check(rc, "nr_conv1d_k3_fwd")
    assert labels == set(want["fwd"]), (labels, want["fwd"])
    if c.xr:
        conv_check_xrows(p)
    ry = conv_check_y(p)
    if p.skips and c.dyp in ("first", "last"):               # the "_needed" kernels did leave far titles as they were: the poison is live
        assert bool(torch.isnan(p.xbuf).any()) and bool((H._bits(p.ybuf) == H._bits(p.ybefore)).all(1)[:p.n * c.T].any())
    y1, x1 = p.ybuf.clone(), p.xbuf.clone()
    p.ybuf.copy_(p.ybefore)
    p.xbuf.copy_(p.xbefore)
    _lib.check(_fwd(p, d)(), "nr_conv1d_k3_fwd")
    torch.cuda.synchronize()
    assert torch.equal(H._bits(y1), H._bits(p.ybuf)) and torch.equal(H._bits(x1), H._bits(p.xbuf)), "two forward runs differ"
    rc, labels = H._profiled(_bwd(p, d))
    _lib.check(rc, "nr_conv1d_k3_bwd")
    assert labels == set(want["dw"]), (labels, want["dw"])
    rw, rb = conv_check_dw(p)
    if c.xr:
        conv_check_xrows(p)                                  # the backward only reads them
    if c.dyp == "zero":
        assert torch.equal(H._bits(p.wbuf), H._bits(p.wbefore)) and torch.equal(H._bits(p.dbbuf), H._bits(p.dbbefore))
    return p, ry, rw, rb


def _conv_case(c):
    for layer in ("lattice", "layer2"):
        if c.opt:
            with H._opt(c.opt, 1):
                _, ry, rw, rb = _run_conv(c, layer)
        else:
            _, ry, rw, rb = _run_conv(c, layer)
        if layer == "layer2":
            want = conv_labels(c)
            print(f"\nL2 conv {conv_label_family(want['fwd'][-1])} y {ry:.4f} | {conv_label_family(want['dw'][-1])} dW {rw:.4f} db {rb:.4f}")


@pytest.mark.parametrize("c", conv_small_cases(), ids=conv_case_id)
def test_forward_and_dw_small(c):
    _conv_case(c)


@pytest.mark.parametrize("c", conv_slab_cases(), ids=conv_case_id)
def test_forward_and_dw_slab_shapes(c):
    _conv_case(c)


def test_needed_flags_without_bwd_ws_are_refused_on_a_slab_shape():
    """The forward left x_rows of far titles unwritten: a backward that would contract every row must not run."""
    c = conv_refused_case()
    assert conv_labels(c)["dw"] is None
    p = conv_problem(c, "lattice", DEV)
    d = _desc(p)
    rc, labels = H._profiled(_fwd(p, d))
    _lib.check(rc, "nr_conv1d_k3_fwd")
    assert labels == set(conv_labels(c)["fwd"]), labels
    conv_check_xrows(p)
    conv_check_y(p)
    rc, labels = H._profiled(_bwd(p, d))
    assert rc != 0 and "bwd_ws" in _lib.last_error() and labels == set(), (rc, labels)
    assert torch.equal(H._bits(p.wbuf), H._bits(p.wbefore)) and torch.equal(H._bits(p.dbbuf), H._bits(p.dbbefore))


def _table_call(p, V=None):
    c = p.c
    d = _lib.ConvDesc(n=p.n, T=c.T, D=c.D, Dp=H._rup(c.D, 8), N=c.N, dtype=CODE[c.dt], ids=p.ids.data_ptr(), ids_stride=p.ids.stride(0),
                      p_in=p.p, seed_in=p.seed, seq_nz=p.flags.data_ptr() if p.flags is not None else 0, table_rows=V or c.V)
    p.ws = _ws_bytes(_lib.lib().nr_conv_table_workspace_bytes(C.byref(d)))
    return lambda: _lib.lib().nr_conv1d_k3_bwd_table(C.byref(d), p.dybuf.data_ptr(), p.wtbuf.data_ptr(), c.ldwt, p.dtable.data_ptr(),
                                                     p.ws.data_ptr(), p.ws.numel() * 4, ops._stream())


def _run_table(p):
    """One table-gradient problem, twice: labels, sentinels and untouched rows, values, run-to-run bit equality."""
    c = p.c
    rc, labels = H._profiled(_table_call(p))
    _lib.check(rc, "nr_conv1d_k3_bwd_table")
    assert labels == set(conv_labels(c)["dtable"]), (labels, conv_labels(c)["dtable"])
    ratio = conv_check_dtable(p)
    assert int(p.ws[0]) == int(((p.ids > 0) & (p.ids < c.V) & ((p.flags != 0) if p.flags is not None else True)).sum())   # live titles
    first = p.tflat.clone()
    p.tflat.copy_(p.tbefore)
    _lib.check(_table_call(p)(), "nr_conv1d_k3_bwd_table")
    torch.cuda.synchronize()
    assert torch.equal(H._bits(first), H._bits(p.tflat)), "two runs differ"
    return ratio


@pytest.mark.parametrize("c", conv_table_cases(), ids=conv_case_id)
def test_table_gradient(c):
    for layer in ("lattice", "layer2"):
        p = conv_table_problem(c, layer, DEV)
        assert (p.dtable.data_ptr() % 16 != 0) == bool(c.off)
        ratio = _run_table(p)
        if c.ids == "zeros":
            assert torch.equal(H._bits(p.tflat), H._bits(p.tbefore))
        if layer == "layer2":
            print(f"\nL2 conv dtable {conv_label_family(conv_labels(c)['dtable'][2])} scatter {'vec' if c.D % 4 == 0 and not c.off else 'scalar'} "
                  f"ratio {ratio:.4f}")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_one_seed_gives_the_forward_rows_and_the_table_gradient(dt):
    """The mask of ops.dropout_mask(n*T*D, p, seed) reproduces both x_rows of the forward and the dtable of the backward."""
    c = _cc(dt, 40, 5, 20, 24, 64, "mixed", xr=True, p=True)
    for layer in ("lattice", "layer2"):
        p, _, _, _ = _run_conv(c, layer)
        t = conv_table_problem(TabCase(dt, c.n, c.T, c.D, c.N, 192, CONV_V, c.ids, True, False, 0), layer, DEV, share=p)
        _run_table(t)


PACK_SHAPES = [("bf16", 8, 5, 8, 32), ("bf16", 200, 300, 320, 640), ("f32", 8, 5, 8, 24), ("f32", 72, 50, 52, 220)]


@pytest.mark.parametrize("dt,N,D,Dp,ld", PACK_SHAPES)
def test_pack_kernels_bit_for_bit(dt, N, D, Dp, ld):
    """nr_pack_conv_w, nr_pack_conv_w_t and nr_unpack_conv_dw against their header formulas, zero padding included."""
    tdt, lib, s = H._tdt(dt), _lib.lib(), ops._stream()
    g = torch.Generator(device=DEV).manual_seed(N + D)
    w = torch.randn(N, D, 3, generator=g, device=DEV)                 # not representable in bf16: the cast rounds to nearest even
    for fn, rows, cols, want in (("nr_pack_conv_w", N, 3 * Dp, conv_pack_w(w, Dp)), ("nr_pack_conv_w_t", D, ld, conv_pack_w_t(w, ld))):
        buf = torch.full((rows + 1, cols), float("nan"), dtype=tdt, device=DEV)
        buf[rows:] = H.GEMM_SENTINEL
        before = buf.clone()
        _lib.check(getattr(lib, fn)(w.data_ptr(), N, D, buf.data_ptr(), Dp if fn == "nr_pack_conv_w" else ld, CODE[dt], s), fn)
        torch.cuda.synchronize()
        H.gemm_check_sentinels(buf, before, rows, cols)
        assert torch.equal(H._bits(buf[:rows]), H._bits(want.to(tdt))), fn
    pack = torch.randn(N, 3 * Dp, generator=g, device=DEV)           # (fp32 whatever the compute dtype)
    for acc in (0, 1):
        buf = torch.full((N * D * 3 + 4,), H.GEMM_SENTINEL, device=DEV)
        pre = torch.randn(N, D, 3, generator=g, device=DEV)
        buf[:N * D * 3] = pre.flatten()
        before = buf.clone()
        _lib.check(lib.nr_unpack_conv_dw(pack.data_ptr(), N, D, Dp, buf.data_ptr(), acc, s), "nr_unpack_conv_dw")
        torch.cuda.synchronize()
        H.gemm_check_sentinels(buf, before, N * D * 3, 0)
        want = pack.view(N, 3, Dp)[:, :, :D].permute(0, 2, 1) + (pre if acc else 0)
        assert torch.equal(H._bits(buf[:N * D * 3].view(N, D, 3)), H._bits(want.contiguous())), acc


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("train_table", [False, True])
def test_ops_conv1d_k3_gather_autograd_plumbing(dt, direct, train_table):
    """ops.conv1d_k3_gather on the lattice (exact): y, and dW / db / dtable as they reach .grad -- through autograd (unpack
    with accumulate = 0) or added straight into preallocated gradient views (accumulate = 1) -- frozen and trainable table."""
    c = _cc(dt, 40, 5, 20, 24, 64, "mixed", p=False)
    p = conv_problem(c, "lattice", DEV)
    V, T, D, N = CONV_V, c.T, c.D, c.N
    table = p.tab.reshape(V, T * D).clone().requires_grad_(train_table)
    w, b = p.w.clone().requires_grad_(True), p.b.clone().requires_grad_(True)
    pre = {}
    if direct:
        for name, t in (("w", w), ("b", b)) + ((("table", table),) if train_table else ()):
            pre[name] = torch.randint(-5, 6, t.shape, device=DEV).float()
            t._nr_grad = pre[name].clone()
    y = ops.conv1d_k3_gather(table, w, b, p.ids, T, D, CODE[dt])
    y.backward(p.dy.to(H._tdt(dt)))
    torch.cuda.synchronize()
    H.gemm_check_values(y.detach().reshape(c.n * T, N), p.y_ref, "lattice")
    got = {k: (getattr(t, "_nr_grad", None) if direct else t.grad) for k, t in (("w", w), ("b", b), ("table", table))}
    zero = lambda k, t: pre.get(k, torch.zeros_like(t)).double()
    dw = (p.dw_ref - p.P.double()).view(N, 3, c.Dp)[:, :, :D].permute(0, 2, 1)
    H.gemm_check_values(got["w"], zero("w", w) + dw, "lattice")
    H.gemm_check_values(got["b"], zero("b", b) + p.db_ref - p.Pb.double(), "lattice")
    if direct:
        assert w.grad is None and b.grad is None and table.grad is None
    if train_table:
        ref, _, touched = conv_dtable_ref(p.ids, p.dy, p.w, p.keep, 1.0, V, dt, "lattice")
        H.gemm_check_values(got["table"], zero("table", table) + ref, "lattice")
        assert bool((got["table"][~touched] == zero("table", table)[~touched].float()).all())
    else:
        assert table.grad is None

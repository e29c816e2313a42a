"""CPU proof of the attention-core sweep (tests/test_gpu_attention_sweep.py): the comparator, its tolerances and its power.

The sweep compares the HIP attention kernels with the fp64 reference (`oracle.nr_oracle.sdpa` + `apply_dropout`, gradient by
autograd) through a slice-relative comparator (helpers.slice_rel_err).  Nothing here touches a GPU; what is proven here, on
exactly the case list the GPU file runs (helpers.attn_cases):

  * the stable form the kernels evaluate (row maximum factored out, 1e-8 * exp(-m) in the denominator) IS the reference's
    formula: in fp64 it matches O.sdpa's autograd gradient to 1e-9;
  * the tolerances.  A CPU stand-in kernel (helpers.attn_standin: torch fp32 on the same bf16-representable inputs, rounded to
    bf16 exactly where the kernels feed a bf16 MFMA, bf16 outputs; plain fp32 for the fp32 kernels) gives the error a sound
    kernel of that arithmetic has; the tolerance per dtype and quantity is min(project bound, 3 x the stand-in's worst
    error over all cases) and lives in helpers.ATTN_TOL, which this test recomputes and pins;
  * the comparator's power: each mutant of the fp64 formula (helpers.ATTN_MUTANTS) misses the tolerance by >= 2x somewhere;
  * the fp64 reference is finite over the stated input domain: |s| <= 60, maximum over all keys <= 45 above the maximum
    over the valid keys.

Stand-in worst slice-relative errors over the 95 cases (printed by test_standin_sets_the_tolerances_and_passes_every_case),
and the tolerance min(project bound, 3 x worst) they give:
  bf16: y 9.3e-3 -> 2e-2 (project)   dQ 1.1e-2 -> 3e-2 (project)   dK 1.6e-2 -> 3e-2 (project)   dV 1.0e-2 -> 3e-2 (project)
  fp32: y 4.7e-6 -> 1.4e-5           dQ 3.1e-6 -> 9.4e-6           dK 3.8e-6 -> 1.1e-5           dV 2.9e-6 -> 8.8e-6
Absolute allowance where a gradient is analytically zero (dQ / dK with at most one valid key, dK / dV rows of masked keys), in
units of max|dy| max|V| max(|Q|, |K|), 3 x the stand-in's worst error there: bf16 5.0e-8, fp32 5.5e-8.
The test fails when helpers.ATTN_TOL / ATTN_ABS_ZERO differ from what it computes by more than 5 % (a last-bit difference of
the CPU's fp32 sums moves the maxima by less).
"""
import math

import pytest
import torch

import helpers as H

CASES = H.attn_cases()
QUANT = ("y", "dq", "dk", "dv")


def _keep(c, n, g):
    """A Bernoulli keep mask [n, heads, L, d] (the GPU file takes the kernels' own from ops.dropout_mask)."""
    return (torch.rand(n, c.L, c.heads, c.d, generator=g) >= c.p_out).float().permute(0, 2, 1, 3) if c.p_out > 0 else None


def _n_host(c):
    """The grid-stride cases differ from their small-n siblings in the launch only: 67 sequences of them are enough here."""
    return min(c.n, 67)


@pytest.fixture(scope="module")
def sweep():
    """Per case and mask mode: inputs, fp64 reference, stand-in errors.  Computed once for every test of this file."""
    torch.manual_seed(0)
    out = []
    for c in CASES:
        inp = H.attn_inputs(c._replace(n=_n_host(c)))
        g = torch.Generator().manual_seed(7)
        keep = _keep(c, _n_host(c), g)
        unit = H.attn_grad_unit(inp["q"], inp["k"], inp["v"], inp["dy"])
        for mode, mask in inp["masks"].items():
            args = (inp["q"], inp["k"], inp["v"], mask, inp["dy"], keep, c.p_out)
            ref = H.attn_ref64(*args)
            out.append((c, mode, args, ref, unit, H.attn_standin(c, *args)))
    return out


def test_case_list_reaches_every_route_and_stays_in_the_domain(sweep):
    assert {c.route for c in CASES} == set(H.ATTN_ROUTE_LABELS)
    for c in CASES:
        assert H.attn_route(c.dtype, c.heads, c.d, c.L, c.align == "aligned") == c.route, c
    assert H.attn_route("bf16", 4, 40, 30, True) is None and H.attn_route("f32", 4, 12, 40, True) is None
    assert H.attn_route("bf16", 4, 20, 65, True) is None
    seen = set()
    for c, mode, (q, k, v, mask, dy, keep, p), ref, unit, _ in sweep:
        s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(c.d)
        assert float(s.abs().max()) <= 60
        if mask is not None:
            valid = mask.bool()[:, None, None, :]
            live = mask.sum(1) > 0
            gap = s.amax(-1) - s.masked_fill(~valid, -1e9).amax(-1)
            assert float(gap[live].max()) <= 45 if bool(live.any()) else True
            if c.regime == "masked_max":
                assert float(gap.min()) >= 20
        if c.regime == "ordinary":
            assert float(s.abs().max()) <= 6                 # |s| <~ 3: the tail of 5 million draws
        elif c.regime == "negative":
            assert -22 <= float(s.min()) and float(s.max()) <= -18
        elif c.regime == "positive":
            assert 38 <= float(s.min()) and float(s.max()) <= 45
        seen.add(c.regime)
        for t in ref.values():
            assert bool(torch.isfinite(t).all())
    assert seen == {"ordinary", "negative", "positive", "masked_max"}


def test_reference_is_finite_at_the_edge_of_the_domain():
    """|s| = 60 everywhere, s = -60 everywhere, and a masked key at +60 that is 45 above every valid key."""
    n, h, L, d = 2, 2, 9, 16
    one = torch.ones(n, h, L, d)
    a = math.sqrt(60 / math.sqrt(d))
    g = torch.Generator().manual_seed(1)
    v, dy = torch.randn(n, h, L, d, generator=g), torch.randn(n, h, L, d, generator=g)
    mask = torch.ones(n, L)
    mask[:, 4] = 0
    kk = one * a * 0.25                                    # valid keys at 15
    kk[:, :, 4] = a                                        # the masked one at 60
    for q, k, m in ((one * a, one * a, None), (one * a, -one * a, None), (one * a, kk, mask)):
        ref = H.attn_ref64(q, k, v, m, dy)
        alt = H.attn_math(q, k, v, m, dy)
        for name in QUANT:
            assert bool(torch.isfinite(ref[name]).all())
        assert H.slice_rel_err(alt["y"], ref["y"]) <= 1e-9 and H.slice_rel_err(alt["dv"], ref["dv"]) <= 1e-9
        assert float(ref["y"].abs().max()) > (0.1 if float((q * k).sum(-1).max()) > 0 else 1e-18)     # s = -60: y ~ 9 e^-60 / 1e-8 * v


def test_stable_form_is_the_reference_formula(sweep):
    for c, mode, args, ref, unit, _ in sweep:
        alt = H.attn_math(*args)
        for name in QUANT:
            assert H.slice_rel_err(alt[name], ref[name], H.attn_zero_places(args[3], *ref["y"].shape[0:3:2])[name], 1e-12 * unit) <= 1e-9, \
                (H.attn_case_id(c), mode, name)


def test_standin_sets_the_tolerances_and_passes_every_case(sweep):
    worst = {dt: dict.fromkeys(QUANT, 0.0) for dt in ("bf16", "f32")}
    zero = {"bf16": 0.0, "f32": 0.0}
    for c, mode, args, ref, unit, st in sweep:
        zp = H.attn_zero_places(args[3], ref["y"].shape[0], ref["y"].shape[2])
        for name in ("dq", "dk", "dv"):                    # absolute error of the stand-in where the gradient is analytically zero
            z = zp[name].expand_as(ref[name]).double()
            # slices whose zero places are tiny throughout (not the negative regime: there the 1e-8 makes a single key's row
            # non-constant, the gradient is an ordinary number and the relative bound applies)
            tiny = ((ref[name].abs() * z).amax((2, 3)) <= 1e-6 * unit) & (z.amax((2, 3)) > 0)
            if bool(tiny.any()):
                e = ((st[name].double() - ref[name]).abs() * z).amax((2, 3))[tiny].max()
                zero[c.dtype] = max(zero[c.dtype], float(e) / unit)
    abs_zero = {dt: 3 * z for dt, z in zero.items()}
    for c, mode, args, ref, unit, st in sweep:
        err = H.attn_errors(c, st, ref, args[3], unit, abs_zero[c.dtype])
        for name in QUANT:
            worst[c.dtype][name] = max(worst[c.dtype][name], err[name])
    tol = {dt: {name: min(H.ATTN_PROJECT_TOL[dt][name], 3 * worst[dt][name]) for name in QUANT} for dt in worst}
    print("stand-in worst:", {dt: {k: f"{x:.2e}" for k, x in w.items()} for dt, w in worst.items()})
    print("tolerances:", {dt: {k: f"{x:.2e}" for k, x in w.items()} for dt, w in tol.items()})
    print("abs zero (x3):", {dt: f"{x:.2e}" for dt, x in abs_zero.items()})
    # sanity anchor of the bf16 floor (a rough probe: y <= 7.2e-3, dQ / dK <= 3.9e-3 at ordinary scores)
    assert 1e-3 <= worst["bf16"]["y"] <= 1.5e-2 and worst["f32"]["y"] <= 3e-5
    # the pinned numbers are the computed ones (to the two digits they are written with; the stand-in runs in fp32 on the CPU
    # and the order of its sums may differ by a last bit from machine to machine)
    for dt in tol:
        for name in QUANT:
            assert abs(H.ATTN_TOL[dt][name] - tol[dt][name]) <= 0.05 * tol[dt][name], (dt, name, H.ATTN_TOL[dt][name], tol[dt][name])
        assert abs(H.ATTN_ABS_ZERO[dt] - abs_zero[dt]) <= 0.05 * abs_zero[dt] + 1e-12, (dt, H.ATTN_ABS_ZERO[dt], abs_zero[dt])
    # ... and the stand-in is within them on every case (by construction of the maximum, unless the project bound is the smaller)
    for c, mode, args, ref, unit, st in sweep:
        err = H.attn_errors(c, st, ref, args[3], unit, H.ATTN_ABS_ZERO[c.dtype])
        for name in QUANT:
            assert err[name] <= H.ATTN_TOL[c.dtype][name], (H.attn_case_id(c), mode, name, err[name])


@pytest.mark.parametrize("mutant", H.ATTN_MUTANTS)
def test_every_mutant_misses_the_tolerance_by_2x_somewhere(sweep, mutant):
    worst, where = {"bf16": 0.0, "f32": 0.0}, {}
    for c, mode, args, ref, unit, _ in sweep:
        if mutant == "eps_unscaled" and c.regime != "negative":
            continue                                       # must show in the negative-score regime
        got = H.attn_mutant(mutant, *args)
        if got is None:
            continue
        err = H.attn_errors(c, got, ref, args[3], unit, H.ATTN_ABS_ZERO[c.dtype])
        for name in QUANT:
            r = err[name] / H.ATTN_TOL[c.dtype][name]
            if r > worst[c.dtype]:
                worst[c.dtype], where[c.dtype] = r, (H.attn_case_id(c), mode, name)
        if min(worst.values()) >= 2.0:
            break                                          # found in both dtypes: no need to walk the rest
    print(f"mutant {mutant}: error / tolerance = {worst} at {where}")
    assert min(worst.values()) >= 2.0, (mutant, worst, where)       # in each dtype's cases, with that dtype's tolerance

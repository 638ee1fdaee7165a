"""Context widths above the ones the other GPU tests use (C <= 300), on every flow path: the in-layer small / mid / large
variants at their boundaries (96 | 97, 288 | 289, 576 | 577), the hoisted projection kernel with its 64-row tile (up to
C = 640 fp32 / 1280 bf16) and its 32-row tile (up to 1024 / 2048), the incremental inverse's row projection, the backward,
and the refusal one width beyond the plan's limit.  Tiny flows (L = 2, K = 8, B = 70: two 64-row projection blocks, the second
ragged, not a multiple of 16); odd widths take the scalar staging path of the projection kernel, multiples of 4 the vector
path.  Every bound is the one an existing test uses for the same quantity (named at each assertion); the CPU fp32 oracle sums
the same longer dot products, so the bounds that are multiples of its error scale with C on their own.  tests/
test_context_width_plan.py holds the host side of the same contract."""
import functools
import random

import pytest
import torch

from helpers import flow_inputs, make_pair, oracle_state_for_product

pytestmark = pytest.mark.gpu

L, K, TB, B = 2, 8, 3.0, 70
D_OF = {64: 3, 128: 6, 192: 7, 256: 5}
LIMIT = {"fp32": 1024, "bf16": 2048}

CASES = ([("fp32", 128, c) for c in (96, 97, 288, 289)] + [("fp32", 192, c) for c in (288, 289)]
         + [("fp32", 256, c) for c in (289, 576, 577, 640, 641, 1024)] + [("fp32", 64, 641)]
         + [("bf16", 256, c) for c in (577, 1280, 1281, 2048)] + [("bf16", 128, 289)]
         + [("masked", 128, 645)])
ids = lambda v: "-".join(str(s) for s in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _case(mode, H, C):
    """flow + oracles + inputs + the oracles' forward results of one width, made once and shared (never modified)"""
    D = D_OF[H] if mode != "masked" else 5
    if mode == "masked":            # built as in test_masked_context_variant_shapes: C = D * block, permuted order
        from oracle.flow_ref import NSFPosteriorFlowRef
        from posteriflow_amd import NSFPosteriorFlow
        assert C % D == 0
        torch.manual_seed(D)
        ref = NSFPosteriorFlowRef(D, C, H, L, K, TB, temperature_scale=1.0, use_masked_context=True)
        ref64 = NSFPosteriorFlowRef(D, C, H, L, K, TB, temperature_scale=1.0, use_masked_context=True).double()
        ref64.load_state_dict(ref.state_dict())
        flow = NSFPosteriorFlow(D, C, H, L, K, TB, temperature_scale=1.0)
        assert flow.use_masked_context
        flow.load_state_dict(oracle_state_for_product(ref))
        flow = flow.cuda()
        order = list(range(D))
        random.Random(D).shuffle(order)
        for f in (ref, ref64, flow):
            f.set_autoregressive_order(order)
    else:
        ref, ref64, flow = make_pair(D, C, H, L, K, TB, seed=H + C)
        flow.precision = mode
    x, ctx = flow_inputs(B, D, C, TB, seed=C)
    g = torch.Generator().manual_seed(C + 3)
    zi = torch.randn(B, D, generator=g) * 1.5
    zi[0, 0] = TB; zi[1, D - 1] = -TB; zi[2, 0] = 1.4 * TB           # on / beyond the spline domain (test_inverse_fp32_parity)
    zeros = torch.zeros_like(x)
    with torch.no_grad():
        z64, ld64 = ref64(x.double(), ctx.double())
        z32, ld32 = ref(x, ctx)
        n64 = ref64.compute_psd_aware_nll(x.double(), ctx.double(), zeros.double())
        n32 = ref.compute_psd_aware_nll(x, ctx, zeros)
        xi64, ldi64 = ref64.inverse_raw(zi.double(), ctx.double())
        xi32, ldi32 = ref.inverse_raw(zi, ctx)
    return dict(D=D, ref=ref, ref64=ref64, flow=flow, x=x, ctx=ctx, zi=zi, fwd64=(z64, ld64, n64), fwd32=(z32, ld32, n32),
                inv64=(xi64, ldi64), inv32=(xi32, ldi32))


def _expected_ckm(mode, H, C):
    """scheduled in-layer context k-steps of the forward kernel (0: hoisted), csrc/pf_layout.h pick_ckm"""
    if mode == "masked":
        return 0
    small, mid, large = (3, 9, 18) if mode == "bf16" else (6, 18, 36)
    if C <= 96 and H <= 128:
        return small
    if C <= 288:
        return mid
    return large if (C <= 576 and H == 256) else 0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_forward_matches_the_oracle(case):
    mode, H, C = case
    c = _case(*case)
    flow, x, ctx = c["flow"], c["x"].cuda(), c["ctx"].cuda()
    name = flow.forward_kernel_name(B)
    print(f"\n[{ids(case)}] forward kernel {name}")
    assert name.startswith("pf::flow_kernel<") and int(name.split(",")[3]) == _expected_ckm(mode, H, C), name
    with torch.no_grad():
        zg, ldg = flow(x, ctx)
        nll = flow.compute_psd_aware_nll(x, ctx, None)
    got = (zg.cpu(), ldg.cpu(), nll.cpu())
    assert all(torch.isfinite(t).all() for t in got)
    if mode != "bf16":
        # the bound of test_random_shape_matches_oracle: relative error below max(2e-5, 6 x the CPU fp32 oracle's own)
        for what, g, w32, w64 in zip(("z", "logdet", "nll"), got, c["fwd32"], c["fwd64"]):
            scale = w64.abs().clamp_min(1.0)
            err = ((g.double() - w64).abs() / scale).max().item()
            cpu = ((w32.double() - w64).abs() / scale).max().item()
            print(f"[{ids(case)}] {what}: rel err {err:.2e} (cpu fp32 {cpu:.2e}, bound {max(2e-5, 6 * cpu):.2e})")
            assert err < max(2e-5, 6 * cpu), (what, err, cpu)
    else:
        # the medians of test_generic_shape_matches_oracle, against the oracle with the kernel's operand rounding
        from oracle import nflows_restated
        with torch.no_grad(), nflows_restated.gemm_emulation("bf16"):
            ze, le = c["ref"](c["x"], c["ctx"])
            ne = c["ref"].compute_psd_aware_nll(c["x"], c["ctx"], torch.zeros_like(c["x"]))
        dz = (got[0] - ze).abs()
        dl = (got[1] - le).abs() / le.abs().clamp_min(1.0)
        dn = (got[2] - ne).abs() / ne.abs().clamp_min(1.0)
        print(f"[{ids(case)}] bf16 medians: dz {dz.median():.2e} dl {dl.median():.2e} dnll {dn.median():.2e}")
        assert dz.median() < 5e-3 and dl.median() < 1e-2 and dn.median() < 1e-2, (dz.median(), dl.median(), dn.median())


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_inverse_both_kernels_match_the_oracle_and_round_trip(case):
    mode, H, C = case
    c = _case(*case)
    flow = c["flow"]
    z = c["zi"].cuda().contiguous()
    ctx = c["ctx"].cuda()
    cperm = flow._permute_context_blocks(ctx).contiguous()           # what inverse() hands to _inverse_call
    x64, ld64 = c["inv64"]
    e = lambda a, b: (a.cpu().double() - b.cpu().double()).abs()
    out = {}
    flow.incremental_inverse = None
    try:
        with torch.no_grad():
            for inc in (None, False):
                flow.incremental_inverse = inc
                want_inc = flow._use_incremental()
                xg, ldg, flags = flow._inverse_call(z, cperm, B)
                served = "incremental" if (want_inc and flow.incremental_inverse is None) else "d-pass"
                assert int(flags.sum()) == 0
                out[inc] = (xg, ldg, served)
            z2, ldf = flow(out[None][0], ctx)
    finally:
        flow.incremental_inverse = None
    print(f"\n[{ids(case)}] inverse served by: default -> {out[None][2]}, incremental_inverse=False -> {out[False][2]}")
    assert out[False][2] == "d-pass"
    assert out[None][2] == ("d-pass" if mode == "masked" else "incremental")     # no width falls off the incremental kernel
    if mode != "bf16":
        # test_inverse_fp32_parity: within 4 x the CPU fp32 path's own error against float64 (floors 5e-5 / 2e-4)
        ex_ref, eld_ref = e(c["inv32"][0], x64).max().item(), e(c["inv32"][1], ld64).max().item()
        for inc in (None, False):
            ex, eld = e(out[inc][0], x64).max().item(), e(out[inc][1], ld64).max().item()
            print(f"[{ids(case)}] {out[inc][2]}: |x-x64| {ex:.2e} (cpu fp32 {ex_ref:.2e})  |ld-ld64| {eld:.2e} (cpu fp32 {eld_ref:.2e})")
            assert ex < max(4 * ex_ref, 5e-5) and eld < max(4 * eld_ref, 2e-4), (inc, ex, ex_ref, eld, eld_ref)
    else:
        # bf16 operands: each kernel on its own against float64, by the absolute bf16 bounds used elsewhere (0.1 on x:
        # test_incremental_inverse_unsupported_shape_falls_back_to_the_d_pass_kernel; 1.0 on the log-det: test_round_trip_full_size)
        for inc in (None, False):
            ex, eld = e(out[inc][0], x64).max().item(), e(out[inc][1], ld64).max().item()
            print(f"[{ids(case)}] {out[inc][2]}: |x-x64| {ex:.2e}  |ld-ld64| {eld:.2e}")
            assert ex < 0.1 and eld < 1.0, (inc, ex, eld)
    # test_incremental_inverse_matches_dpass_and_oracle: the two kernels differ by rounding noise only
    (x1, ld1, _), (x0, ld0, _) = out[None], out[False]
    noise = e(x0, x64)
    print(f"[{ids(case)}] d-pass vs oracle max {noise.max():.2e} median {noise.median():.2e}; incremental vs oracle max "
          f"{e(x1, x64).max():.2e}; between the two median {e(x1, x0).median():.2e}")
    assert e(x1, x64).max() <= max(3.0 * noise.max().item(), 1e-4)
    assert e(x1, x64).flatten().quantile(0.99) <= max(1.5 * noise.flatten().quantile(0.99).item(), 1e-5)
    assert e(x1, x64).median() <= max(1.5 * noise.median().item(), 1e-5)
    assert e(x1, x0).median() <= max(noise.median().item(), 1e-5)
    assert e(ld1, ld64).max() <= max(2.0 * e(ld0, ld64).max().item(), 1e-3)
    # round trip forward(inverse(z)) == z: the tolerances of test_round_trip_full_size
    tol_x, tol_ld = (0.1, 1.0) if mode == "bf16" else (5e-4, 2e-3)
    rt = (z2 - z).abs().max(dim=1).values
    print(f"[{ids(case)}] round trip |z2-z| q99 {rt.quantile(0.99):.2e}  |ld_f+ld_i| q99 {(ldf + out[None][1]).abs().quantile(0.99):.2e}")
    assert rt.quantile(0.99) < tol_x and (ldf + out[None][1]).abs().quantile(0.99) < tol_ld


@pytest.mark.parametrize("case", [("fp32", 256, 641), ("bf16", 256, 1281)], ids=ids)
@pytest.mark.parametrize("ctx_rows", [1, 5, 70])
def test_grouped_context_rows_above_the_64_row_tiles_limit(case, ctx_rows):
    """one context row per group of draws == the expanded form: bit-identical on the D-pass kernel (context handled inside the
    kernel), within 1e-4 / 1e-3 on the incremental one (test_grouped_and_expanded_context_and_order)"""
    c = _case(*case)
    flow, z = c["flow"], c["zi"].cuda().contiguous()
    ctx = c["ctx"][:ctx_rows].cuda().contiguous()
    rep = ctx.repeat_interleave(B // ctx_rows, dim=0).contiguous()
    try:
        with torch.no_grad():
            flow.incremental_inverse = False
            a, ald, fa_ = flow._inverse_call(z, rep, B)
            b, bld, fb_ = flow._inverse_call(z, ctx, ctx_rows)
            assert torch.equal(a, b) and torch.equal(ald, bld) and int(fa_.sum()) == 0 and int(fb_.sum()) == 0
            flow.incremental_inverse = None
            assert flow._use_incremental()
            a1, ald1, _ = flow._inverse_call(z, rep, B)
            b1, bld1, _ = flow._inverse_call(z, ctx, ctx_rows)
            assert flow.incremental_inverse is None
    finally:
        flow.incremental_inverse = None
    print(f"\n[{ids(case)} rows {ctx_rows}] incremental grouped vs expanded: x {(a1 - b1).abs().max():.2e} ld {(ald1 - bld1).abs().max():.2e}")
    assert (a1 - b1).abs().max() < 1e-4 and (ald1 - bld1).abs().max() < 1e-3


@pytest.mark.parametrize("case", [("fp32", 256, 289), ("fp32", 256, 577), ("fp32", 256, 641), ("fp32", 128, 289)], ids=ids)
def test_gradients_match_autograd_through_the_oracle(case):
    """d nll / d x, d / d context and every transform.* parameter gradient on the HIP backward (re-evaluation, chain,
    transposed GEMMs) at contexts wider than 288.  Truth is float64 autograd through the oracle; the bounds are those of
    test_random_shape_bf16_and_gradients (nll 1e-4, x and context 5e-5, parameters 2e-3), unchanged; the CPU fp32 oracle's
    error against the same truth is printed beside each worst figure.  Measured (HIP / CPU fp32, relative to float64 autograd): C = 641 at H = 256
    x 8.3e-6 / 1.1e-5, context 1.1e-5 / 1.4e-5, parameters 1.5e-5 / 1.8e-5; the other three widths below 9e-6 throughout --
    no case comes near the bounds."""
    from posteriflow_amd import _flow_autograd as fa
    c = _case(*case)
    flow, ref, ref64, x, ctx = c["flow"], c["ref"], c["ref64"], c["x"], c["ctx"]
    grads = {}
    for name, m, dt in (("32", ref, torch.float32), ("64", ref64, torch.float64)):
        m.zero_grad()
        xr, cr = x.clone().to(dt).requires_grad_(True), ctx.clone().to(dt).requires_grad_(True)     # (the shared inputs stay as they are)
        nll_ref = m.compute_psd_aware_nll(xr, cr, torch.zeros_like(xr))
        nll_ref.sum().backward()
        grads[name] = dict(nll=nll_ref.detach(), x=xr.grad, ctx=cr.grad,
                           **{n: p.grad.clone() for n, p in m.named_parameters() if n.startswith("transform.")})
        m.zero_grad()
    flow.zero_grad()
    xg, cg = x.cuda().requires_grad_(True), ctx.cuda().requires_grad_(True)
    calls, orig = [], fa.flow_forward
    fa.flow_forward = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        nll = flow.compute_psd_aware_nll(xg, cg, None)
        nll.sum().backward()
    finally:
        fa.flow_forward = orig
    assert fa._fast(flow) and not calls                       # the tensor-op replay did not run
    rel = lambda a, b: ((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-9)).item()
    got = dict(nll=nll.detach(), x=xg.grad, ctx=cg.grad,
               **{n: p.grad for n, p in flow.named_parameters() if n.startswith("transform.") and p.grad is not None})
    n_params, worst = 0, {}
    for key, truth in grads["64"].items():
        floor = 1e-4 if key == "nll" else 5e-5 if key in ("x", "ctx") else 2e-3
        if key.startswith("transform."):
            if truth.abs().max() <= 1e-6:
                continue
            n_params += 1
        err, cpu = rel(got[key], truth), rel(grads["32"][key], truth)
        kind = key if not key.startswith("transform.") else "params"
        if err > worst.get(kind, (0.0, 0.0))[0]:
            worst[kind] = (err, cpu)
        assert err < floor, (key, err, cpu)
    print(f"\n[{ids(case)}] worst (HIP rel err, cpu fp32 rel err) vs float64 autograd: "
          + ", ".join(f"{k} {v[0]:.2e} / {v[1]:.2e}" for k, v in worst.items()))
    assert n_params == L * 18
    flow.zero_grad()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_one_width_beyond_the_limit_is_refused_by_name(prec):
    """C = limit + 1 (1025 fp32 / 2049 bf16): forward, inverse, sample and compute_psd_aware_nll raise NotImplementedError
    naming the context width and the limit -- decided on the host before any launch, never a HIP error string -- and the
    library serves an accepted width afterwards."""
    from posteriflow_amd import NSFPosteriorFlow
    H, D, C = 256, D_OF[256], LIMIT[prec] + 1
    torch.manual_seed(0)
    flow = NSFPosteriorFlow(D, C, H, L, K, TB, temperature_scale=1.0, use_masked_context=False).cuda()
    flow.precision = prec
    x, ctx = flow_inputs(B, D, C, TB, seed=1)
    x, ctx = x.cuda(), ctx.cuda()
    calls = {"forward": lambda: flow(x, ctx), "inverse": lambda: flow.inverse(x, ctx), "sample": lambda: flow.sample(4, ctx[:2]),
             "compute_psd_aware_nll": lambda: flow.compute_psd_aware_nll(x, ctx, None)}
    for _ in range(2):                                   # the second round: a refusal leaves nothing behind
        for what, call in calls.items():
            with torch.no_grad(), pytest.raises(NotImplementedError) as ei:
                call()
            msg = str(ei.value)
            assert str(C) in msg and str(LIMIT[prec]) in msg and "HIP error" not in msg, (what, msg)
    ok = _case(prec, H, LIMIT[prec])                     # the same process, the limit itself: still served, still right
    with torch.no_grad():
        z1, ld1 = ok["flow"](ok["x"].cuda(), ok["ctx"].cuda())
        z2, ld2 = ok["flow"](ok["x"].cuda(), ok["ctx"].cuda())
    assert torch.equal(z1, z2) and torch.equal(ld1, ld2)
    want = ok["fwd64"][0]
    assert (z1.cpu().double() - want).abs().max() < (0.1 if prec == "bf16" else 1e-3)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_unsupported_row_projection_falls_back_to_the_d_pass_kernel(prec, monkeypatch):
    """PF_ERR_UNSUPPORTED from pf_flow_ctx_project_rows (a return code put there by the test: nothing fails on the device)
    is treated like the one from pf_flow_inverse_inc: remembered, and the D-pass kernel serves the call"""
    from posteriflow_amd import _lib
    _, _, flow = make_pair(6, 40, 128, L, K, TB, seed=11)
    flow.precision = prec
    z = torch.randn(B, 6, generator=torch.Generator().manual_seed(1)).cuda()
    ctx = torch.randn(B, 40, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        flow.incremental_inverse = False
        want = flow._inverse_call(z, ctx, B)
        flow.incremental_inverse = None
        assert flow._use_incremental()
        seen = []
        monkeypatch.setattr(_lib.lib(), "pf_flow_ctx_project_rows", lambda *a: (seen.append(1), _lib.PF_ERR_UNSUPPORTED)[1])
        got = flow._inverse_call(z, ctx, B)
        monkeypatch.undo()
    assert seen and flow.incremental_inverse is False
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with torch.no_grad():
        x, _ = flow.inverse(z, ctx)                          # and the public entry point keeps working
    assert torch.isfinite(x).all()

"""Incremental inverse of the masked-context conditioner (the additive instantiations of csrc/pf_flow_inc.hip and
csrc/pf_flow_inc_wide.hip) against the D-pass kernel and the float64 oracle, on the smallest shapes that reach each path."""
import functools
import random

import pytest
import torch

from helpers import flow_inputs, oracle_state_for_product

pytestmark = pytest.mark.gpu

TB = 3.0
SHAPES = {  # D, block (C = D * block), H, K, L, B
    "h64_c20": (4, 5, 64, 8, 2, 17),            # narrowest scheduled width; C = 20 pads the projection's k; ragged single workgroup
    "d15_c300": (15, 20, 256, 16, 2, 33),       # D at the scheduled limit; C = 300 (hoisted width)
    "d3_h256": (3, 8, 256, 8, 2, 33),           # 8 new tiles per pass: the 512-thread narrow variant
    "head_384x24": (11, 24, 384, 24, 2, 50),    # wide kernel, six tail tiles
    "h256_k20": (8, 12, 256, 20, 2, 33),        # K > 16 at a scheduled width
    "h512_k32": (6, 8, 512, 32, 2, 33),         # widest rows
}
CASES = [(n, p, True) for n in SHAPES for p in ("bf16", "fp32") if not (n == "h512_k32" and p == "fp32")]
SHAPES["h128_partial"] = (6, 8, 128, 8, 3, 40)  # full_context=False: the per-position mask folded into the row projection
CASES += [(n, p, False) for n in ("h128_partial", "head_384x24") for p in ("bf16", "fp32")]
SHAPES["h128_c645"] = (5, 129, 128, 8, 2, 33)   # wider than the default's limit (C <= 300): D-pass unless incremental_inverse = True
CASES += [("h128_c645", "fp32", True)]


@functools.lru_cache(maxsize=None)
def _pair(name, full_context=True):
    """(float64 oracle, product) of one shape, built as test_masked_context_variant_shapes does, shuffled order"""
    from oracle.flow_ref import NSFPosteriorFlowRef
    from posteriflow_amd import NSFPosteriorFlow
    D, block, H, K, L, _ = SHAPES[name]
    kw = {} if full_context else {"full_context": False}
    torch.manual_seed(D)
    ref = NSFPosteriorFlowRef(D, D * block, H, L, K, TB, temperature_scale=1.0, use_masked_context=True, **kw)
    ref64 = NSFPosteriorFlowRef(D, D * block, H, L, K, TB, temperature_scale=1.0, use_masked_context=True, **kw).double()
    ref64.load_state_dict(ref.state_dict())
    flow = NSFPosteriorFlow(D, D * block, H, L, K, TB, temperature_scale=1.0, **kw)
    assert flow.use_masked_context and flow.full_context == full_context
    flow.load_state_dict(oracle_state_for_product(ref))
    flow = flow.cuda()
    order = list(range(D))
    random.Random(D).shuffle(order)
    for m in (ref64, flow):
        m.set_autoregressive_order(order)
    return ref64, flow


def _err(a, b):
    return (a.cpu().double() - b.cpu().double()).abs()


def _assert_no_further_than_dpass(tag, x1, ld1, x0, ld0, want, ldw):
    """the bounds of test_wide_incremental_inverse_matches_dpass_and_oracle"""
    noise, e1 = _err(x0, want), _err(x1, want)
    print(f"\n[{tag}] d-pass vs oracle max {noise.max():.2e} q99 {noise.flatten().quantile(0.99):.2e} median {noise.median():.2e}; "
          f"incremental max {e1.max():.2e} q99 {e1.flatten().quantile(0.99):.2e} median {e1.median():.2e}; between the two median "
          f"{_err(x1, x0).median():.2e}; log-det {_err(ld1, ldw).max():.2e} (d-pass {_err(ld0, ldw).max():.2e})")
    assert e1.max() <= max(3.0 * noise.max().item(), 1e-4)
    assert e1.flatten().quantile(0.99) <= max(1.5 * noise.flatten().quantile(0.99).item(), 1e-5)
    assert e1.median() <= max(1.5 * noise.median().item(), 1e-5)
    assert _err(x1, x0).median() <= max(noise.median().item(), 1e-5)
    assert _err(ld1, ldw).max() <= max(2.0 * _err(ld0, ldw).max().item(), 1e-3)


@pytest.mark.parametrize("name,precision,full_context", CASES)
def test_masked_incremental_inverse_matches_dpass_and_oracle(name, precision, full_context):
    D, block, H, K, L, B = SHAPES[name]
    ref64, flow = _pair(name, full_context)
    flow.precision = precision
    z, ctx = flow_inputs(B, D, D * block, TB, seed=7)
    zc, cperm = z.cuda(), flow._permute_context_blocks(ctx.cuda()).contiguous()       # what inverse() hands to _inverse_call
    try:
        with torch.no_grad():
            want, ldw = ref64.inverse_raw(z.double(), ctx.double())
            forced = True if D * block > flow.masked_incremental_max_context else None
            assert flow._use_incremental() == (forced is None)     # wide masked contexts: not by default, on request
            flow.incremental_inverse = forced
            assert flow._use_incremental()
            x1, ld1, f1 = flow._inverse_call(zc, cperm, B)
            assert flow.incremental_inverse is forced              # served by the incremental kernel: no fallback happened
            flow.incremental_inverse = False
            x0, ld0, f0 = flow._inverse_call(zc, cperm, B)
    finally:
        flow.incremental_inverse = None
    assert int(f0.sum()) == 0 and int(f1.sum()) == 0
    _assert_no_further_than_dpass(f"{name} {precision} full_context={full_context}", x1, ld1, x0, ld0, want, ldw)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["d15_c300", "head_384x24"])
def test_masked_incremental_inverse_grouped_context_is_bitwise_and_round_trips(name, precision):
    D, block = SHAPES[name][:2]
    _, flow = _pair(name)
    flow.precision = precision
    B, groups = 3 * 37, 3                                  # 111 draws: not a multiple of the 16-draw workgroup
    z = torch.randn(B, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    ctx = torch.randn(groups, D * block, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    rep = ctx.repeat_interleave(B // groups, dim=0).contiguous()
    with torch.no_grad():
        assert flow._use_incremental()
        x_g, ld_g, _ = flow._inverse_call(z, flow._permute_context_blocks(ctx).contiguous(), groups)
        x_e, ld_e, _ = flow._inverse_call(z, flow._permute_context_blocks(rep).contiguous(), B)
        assert flow.incremental_inverse is None
        assert torch.equal(x_g, x_e) and torch.equal(ld_g, ld_e)
        zz, ldf = flow(x_g, rep)
    err = (zz - z).abs()
    print(f"\n[{name} {precision}] round trip |z2-z| median {err.median():.2e} q99 {err.quantile(0.99):.2e}; |ld_f+ld_i| median "
          f"{(ldf + ld_g).abs().median():.2e} q99 {(ldf + ld_g).abs().quantile(0.99):.2e}")
    if precision == "bf16":        # the tolerances of test_wide_incremental_inverse_grouped_context_is_bitwise_and_round_trips
        assert err.median() < 2e-2 and err.quantile(0.99) < 0.3
        assert (ldf + ld_g).abs().median() < 0.1
    else:
        assert err.quantile(0.99) < 5e-4 and (ldf + ld_g).abs().quantile(0.99) < 5e-3


def test_c_abi_reads_the_masked_context_flag():
    """pf_flow_inverse_inc bound directly: the flag needs its projections, and selects the additive arithmetic"""
    from posteriflow_amd import _lib
    name = "h64_c20"
    D, block, H, K, L, B = SHAPES[name]
    ref64, flow = _pair(name)
    flow.precision = "fp32"
    z, ctx = flow_inputs(B, D, D * block, TB, seed=7)
    zc, cperm = z.cuda(), flow._permute_context_blocks(ctx.cuda()).contiguous()
    dev, lib = zc.device, _lib.lib()
    st = flow._inc_state(dev)
    proj = torch.empty(B, st["bcat"].numel(), dtype=torch.float32, device=dev)
    _lib.check(lib.pf_flow_ctx_project_rows(_lib.PF_PREC_F32, st["wfrags"].data_ptr(), st["bcat"].data_ptr(), cperm.data_ptr(), B,
                                            D * block, st["bcat"].numel(), proj.data_ptr(), 0), "pf_flow_ctx_project_rows")
    _, inv_perm = flow._perms(dev)
    masked = flow._desc("fp32", inverse=True)
    assert masked.reserved & _lib.PF_FLAG_MASKED_CONTEXT
    plain = type(masked).from_buffer_copy(masked)
    plain.reserved = 0
    perm_ptr = None if inv_perm is None else inv_perm.data_ptr()
    out = {}
    for tag, desc in (("masked", masked), ("plain", plain)):
        x, ld = torch.empty_like(zc), torch.empty(B, device=dev)
        flags = torch.zeros(B, dtype=torch.int32, device=dev)
        call = lambda pr: lib.pf_flow_inverse_inc(desc, st["u1"], st["buf"].data_ptr(), pr, B, zc.data_ptr(), perm_ptr, B,
                                                  x.data_ptr(), ld.data_ptr(), flags.data_ptr(), 0)
        if tag == "masked":
            assert call(None) == _lib.PF_ERR_BAD_ARG
        assert call(proj.data_ptr()) == _lib.PF_OK
        torch.cuda.synchronize()
        out[tag] = (x, ld, flags)
    assert not torch.equal(out["masked"][0], out["plain"][0])
    with torch.no_grad():
        want, ldw = ref64.inverse_raw(z.double(), ctx.double())
        flow.incremental_inverse = False
        try:
            x0, ld0, _ = flow._inverse_call(zc, cperm, B)
        finally:
            flow.incremental_inverse = None
    assert int(out["masked"][2].sum()) == 0
    _assert_no_further_than_dpass("c abi, flag set", out["masked"][0], out["masked"][1], x0, ld0, want, ldw)

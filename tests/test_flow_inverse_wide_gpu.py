"""Incremental inverse of the wide heads (H up to 512, K up to 32: csrc/pf_flow_inc_wide.hip) against the D-pass kernel
and the float64 oracle, on the smallest shapes that reach each of the kernel's paths."""
import random

import pytest
import torch

from helpers import flow_inputs, make_pair

pytestmark = pytest.mark.gpu

SHAPES = {  # D, C, H, L, K, tail, B
    "head_384x24": (11, 288, 384, 2, 24, 3.0, 50),      # FlowHead(12, 384, 24)'s layers; ragged last workgroup
    "d16_h320_k17": (16, 33, 320, 3, 17, 3.0, 17),      # D at its limit, 10 bf16 k-steps (partial group of four), K = 16 + 1, odd C
    "h256_k20": (8, 96, 256, 2, 20, 3.0, 33),           # K > 16 at a scheduled width
    "h512_k32": (6, 0, 512, 2, 32, 5.0, 33),            # widest rows, all 32 lanes live, context-free, 7-8 new tiles per pass
}
CASES = [(n, p) for n in SHAPES for p in ("bf16", "fp32") if not (n == "h512_k32" and p == "fp32")]


def _pair(shape, order_seed=3):
    D, C, H, L, K, tb, B = shape
    ref, ref64, flow = make_pair(D, C, H, L, K, tb)
    order = list(range(D))
    random.Random(order_seed).shuffle(order)
    for m in (ref, ref64, flow):
        m.set_autoregressive_order(order)
    return ref, ref64, flow


@pytest.mark.parametrize("name,precision", CASES)
def test_wide_incremental_inverse_matches_dpass_and_oracle(name, precision):
    """the bounds of test_incremental_inverse_matches_dpass_and_oracle: the two kernels differ by rounding noise only, and the
    incremental one is no further from the float64 oracle than the D-pass kernel is"""
    D, C, H, L, K, tb, B = SHAPES[name]
    _, ref64, flow = _pair(SHAPES[name])
    flow.precision = precision
    z, ctx = flow_inputs(B, D, C, tb, seed=7)
    zc, cc = z.cuda(), None if ctx is None else ctx.cuda()
    with torch.no_grad():
        want, ldw = ref64.inverse_raw(z.double(), None if ctx is None else ctx.double())
        assert flow._use_incremental()
        x1, ld1, f1 = flow._inverse_call(zc, cc, B)
        assert flow.incremental_inverse is None                # served by the incremental kernel: no fallback happened
        flow.incremental_inverse = False
        x0, ld0, f0 = flow._inverse_call(zc, cc, B)
        flow.incremental_inverse = None
    assert int(f0.sum()) == 0 and int(f1.sum()) == 0
    e = lambda a, b: (a.cpu().double() - b.cpu().double()).abs()
    noise = e(x0, want)
    print(f"\n[{name} {precision}] d-pass vs oracle max {noise.max():.2e} q99 {noise.flatten().quantile(0.99):.2e} median "
          f"{noise.median():.2e}; incremental max {e(x1, want).max():.2e} q99 {e(x1, want).flatten().quantile(0.99):.2e} median "
          f"{e(x1, want).median():.2e}; between the two median {e(x1, x0).median():.2e}; log-det {e(ld1, ldw).max():.2e} "
          f"(d-pass {e(ld0, ldw).max():.2e})")
    assert e(x1, want).max() <= max(3.0 * noise.max().item(), 1e-4)
    assert e(x1, want).flatten().quantile(0.99) <= max(1.5 * noise.flatten().quantile(0.99).item(), 1e-5)
    assert e(x1, want).median() <= max(1.5 * noise.median().item(), 1e-5)
    assert e(x1, x0).median() <= max(noise.median().item(), 1e-5)
    assert e(ld1, ldw).max() <= max(2.0 * e(ld0, ldw).max().item(), 1e-3)


@pytest.mark.parametrize("shape,precisions", [((3, 5, 320, 2, 17, 3.0, 40), ("fp32", "bf16")),     # 10 tiles of one degree
                                              ((6, 0, 512, 2, 6, 5.0, 33), ("fp32",))])            # fp32 rows beyond the LDS
def test_wide_incremental_inverse_refused_shape_falls_back_to_the_d_pass_kernel(shape, precisions):
    D, C, H, L, K, tb, B = shape
    ref, _, flow = make_pair(D, C, H, L, K, tb)
    z, ctx = flow_inputs(B, D, C, tb, seed=7)
    for precision in precisions:
        flow.precision, flow.incremental_inverse = precision, None
        with torch.no_grad():
            want, _ = ref.inverse(z, ctx)
            assert flow._use_incremental()
            got, _ = flow.inverse(z.cuda(), None if ctx is None else ctx.cuda())
        assert flow.incremental_inverse is False               # PF_ERR_UNSUPPORTED was seen once, remembered
        assert (got.cpu() - want).abs().max() < (1e-4 if precision == "fp32" else 0.1)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wide_incremental_inverse_grouped_context_is_bitwise_and_round_trips(precision):
    D, C, H, L, K, tb, _ = SHAPES["head_384x24"]
    _, _, flow = _pair(SHAPES["head_384x24"])
    flow.precision = precision
    B, groups = 3 * 37, 3                                  # 111 draws: not a multiple of the 16-draw workgroup
    z = torch.randn(B, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    ctx = torch.randn(groups, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    rep = ctx.repeat_interleave(B // groups, dim=0).contiguous()
    with torch.no_grad():
        assert flow._use_incremental()
        x_g, ld_g, _ = flow._inverse_call(z, ctx, groups)
        x_e, ld_e, _ = flow._inverse_call(z, rep, B)
        assert flow.incremental_inverse is None
        # no reduction order depends on the number of context rows or draws: the same bits
        assert torch.equal(x_g, x_e) and torch.equal(ld_g, ld_e)
        zz, ldf = flow(x_g, rep)
    err = (zz - z).abs()
    print(f"\n[{precision}] round trip |z2-z| median {err.median():.2e} q99 {err.quantile(0.99):.2e}; |ld_f+ld_i| median "
          f"{(ldf + ld_g).abs().median():.2e} q99 {(ldf + ld_g).abs().quantile(0.99):.2e}")
    if precision == "bf16":        # the tolerances of test_incremental_inverse_grouped_context_ragged_batch_and_round_trip
        assert err.median() < 2e-2 and err.quantile(0.99) < 0.3
        assert (ldf + ld_g).abs().median() < 0.1
    else:
        assert err.quantile(0.99) < 5e-4 and (ldf + ld_g).abs().quantile(0.99) < 5e-3

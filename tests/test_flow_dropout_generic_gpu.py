"""Conditioner dropout of the generic-shape flow kernel (H up to 512, K up to 32): flow_generic_kernel<.., 0, true>, the factors
pf_flow_dropout_mask returns for generic plans (counter stride 512 above H = 256) and the fp32 backward that reads them.
Parity is stated as in tests/test_flow_dropout_gpu.py: the oracle's nn.Dropout is replaced by the HIP factors.  L = 2, B = 40
(two full 16-row workgroups and a ragged one of 8); each shape is the smallest that reaches a distinct code path."""
import numpy as np
import pytest
import torch

from helpers import flow_inputs
from test_flow_dropout_gpu import _install, _pair

pytestmark = pytest.mark.gpu

L, B, TB = 2, 40, 5.0
SHAPES = [(11, 288, 384, 24, 0.15, False),      # the reference's head: TPW = 3, stride 512, 32-bin spline backward
          (4, 0, 512, 8, 0.5, False),           # TPW = 4, last position 511, no context
          (6, 40, 256, 20, 0.3, False),         # generic only through K > 16: stride stays 256
          (11, 264, 384, 24, 0.2, True)]        # masked context: additive form, no ReversePermutation


def hash_factors(seed64, p, L, B, H, D, stride):
    """numpy restatement of drop_row_hash / drop_hash / drop_factor (csrc/pf_flow_params.h): ([2, L, B, H] float32 in nflows unit
    order, sorted position -> unit)"""
    u, m32 = np.uint64, np.uint64(0xFFFFFFFF)
    mul = lambda a, b: (a * u(b)) & m32

    def mix(x, s1, m1, s2, m2, s3):
        x = x ^ (x >> u(s1)); x = mul(x, m1); x = x ^ (x >> u(s2)); x = mul(x, m2)
        return x ^ (x >> u(s3))
    rows = mix(u((seed64 ^ (seed64 >> 32)) & 0xFFFFFFFF) ^ mul(np.arange(B, dtype=u), 0x9E3779B1), 16, 0x7FEB352D, 15, 0x846CA68B, 16)
    perm = np.argsort(np.arange(H) % max(1, D - 1) + min(1, D - 1), kind="stable")
    pos = np.empty(H, dtype=u)
    pos[perm] = np.arange(H, dtype=u)
    lb = (2 * np.arange(L, dtype=u)[None, :] + np.arange(2, dtype=u)[:, None])[:, :, None, None]
    y = mix((rows[None, None, :, None] + mul(lb * u(stride) + pos + u(1), 0x85EBCA77)) & m32, 15, 0x2C1B3C6D, 12, 0x297A2D39, 15)
    keep = (y >> u(8)) >= u(int(np.floor(float(np.float32(p)) * 16777216.0 + 0.5)))
    return np.where(keep, np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32), perm


@pytest.mark.parametrize("D,H,p", [(11, 384, 0.15), (4, 512, 0.5)])
def test_generic_factors_match_the_restated_hash_and_blocks_are_independent(D, H, p):
    from posteriflow_amd import NSFPosteriorFlow
    from posteriflow_amd._flow_autograd import dropout_mask
    flow = NSFPosteriorFlow(D, 0, H, L, 8, 3.0, dropout=p).cuda()
    for seed in (1, (1 << 62) - 1):
        got = dropout_mask(flow, 1000, seed, torch.device("cuda")).cpu().numpy()
        want, perm = hash_factors(seed, p, L, 1000, H, D, 512)
        assert got.shape == want.shape and np.array_equal(got, want), (seed, np.abs(got - want).max())
    # with a stride of 256 positions 256 .. of block 0 would share the counters of positions 0 .. of block 1 (agreement 1)
    a, b = got[0, 0][:, perm[256:384]] > 0, got[1, 0][:, perm[0:128]] > 0
    exp = (1 - p) ** 2 + p ** 2
    assert abs((a == b).mean() - exp) < 5 * np.sqrt(exp * (1 - exp) / a.size), (a == b).mean()


def _within(name, got, cpu, want, floor, rel=False):
    """HIP distance to the float64 oracle <= max(the bound asserted at H <= 256, 2.5 x the CPU fp32 oracle's own distance)"""
    den = want.abs().clamp_min(1.0) if rel else 1.0
    e_hip, e_cpu = ((got.cpu().double() - want).abs() / den).max().item(), ((cpu.double() - want).abs() / den).max().item()
    print(f"  {name}: HIP {e_hip:.2e}, CPU fp32 oracle {e_cpu:.2e}")
    assert e_hip <= max(floor, 2.5 * e_cpu), (name, e_hip, e_cpu)
    return e_hip


@pytest.mark.parametrize("D,C,H,K,p,masked", SHAPES)
def test_generic_training_forward_and_gradients_with_dropout_match_the_oracle(D, C, H, K, p, masked):
    """Measured distances to the float64 oracle (HIP / CPU fp32 oracle; LABLOG R5.2): z 3.6e-6 .. 5.3e-6 / 2.4e-6 .. 3.0e-6,
    log-det 7.6e-6 .. 3.9e-5 / 8.1e-6 .. 2.7e-5, nll 1.1e-6 .. 3.9e-6 / 1.2e-6 .. 2.2e-6 relative."""
    from posteriflow_amd._flow_autograd import dropout_mask
    ref, ref64, flow = _pair(D, C, H, L, K, TB, p, masked=masked)
    x, ctx = flow_inputs(B, D, C, TB)
    g = torch.Generator().manual_seed(4)
    w, ls = torch.rand(B, generator=g) + 0.5, torch.randn(B, D, generator=g) * 0.2
    c64, cg0 = (ctx.double(), ctx.cuda()) if C else (None, None)
    flow.train()
    flow.precision = "fp32"
    torch.manual_seed(123)                                       # the seed the differentiable call will draw
    seed = flow._draw_dropout_seed()
    mask = dropout_mask(flow, B, seed, torch.device("cuda")).cpu()
    assert 0.0 < (mask == 0).float().mean() < 1.0
    _install(ref, mask), _install(ref64, mask)
    with torch.no_grad():
        (z64, ld64), n64 = ref64(x.double(), c64), ref64.compute_psd_aware_nll(x.double(), c64, ls.double())
        (zc, ldc), nc = ref(x, ctx), ref.compute_psd_aware_nll(x, ctx, ls)
        z, ld, nll = flow._forward_call(x.cuda(), cg0, ls.cuda(), dropout_seed=seed)
        flow.eval()
        z_eval = flow._forward_call(x.cuda(), cg0, ls.cuda())[0]
        flow.train()
    print(f"\n[D{D} C{C} H{H} K{K} p{p} masked={masked}]")
    ez = _within("z", z, zc, z64, 2e-4)
    _within("log|det|", ld, ldc, ld64, 2e-3)
    _within("nll (relative)", nll, nc, n64, 1e-4, rel=True)
    assert (z_eval - z).abs().max().item() > 100 * ez

    xr, lr, cr = x.clone().requires_grad_(True), ls.clone().requires_grad_(True), ctx.clone().requires_grad_(True) if C else None
    (ref.compute_psd_aware_nll(xr, cr, lr) * w).sum().backward()
    xg, lg, cg = x.cuda().requires_grad_(True), ls.cuda().requires_grad_(True), ctx.cuda().requires_grad_(True) if C else None
    torch.manual_seed(123)
    out = flow.compute_psd_aware_nll(xg, cg, lg)
    assert torch.equal(out.detach(), nll)                       # same seed, same kernel: bit for bit
    (out * w.cuda()).sum().backward()
    tol = 5e-4 if masked else 3e-4                               # the bounds of these shapes without dropout (test_flow_shape_sweep_gpu.py)
    pairs = [("x", xg.grad, xr.grad), ("log_sigma", lg.grad, lr.grad)] + ([("context", cg.grad, cr.grad)] if C else [])
    ref_params = dict(ref.named_parameters())
    named = [(n, q.grad, ref_params[n].grad) for n, q in flow.named_parameters() if n.startswith("transform.") and q.grad is not None]
    assert len(named) == L * (18 if C else 12)
    for name, a, b in pairs + named:
        err = ((a.cpu() - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()
        assert err < tol, (name, err)


def test_generic_dropout_modes_seeds_and_precisions():
    from posteriflow_amd import NSFPosteriorFlow
    D, C, H, K, p, _ = SHAPES[0]
    ref, ref64, flow = _pair(D, C, H, L, K, TB, p)
    x, ctx = flow_inputs(B, D, C, TB)
    xg, cg = x.cuda(), ctx.cuda()
    with torch.no_grad():
        flow.eval()                                             # eval: no dropout, whatever p
        (ze, lde), (zr, ldr), (z64, ld64) = flow(xg, cg), ref(x, ctx), ref64(x.double(), ctx.double())
        _within("eval z", ze, zr, z64, 2e-4), _within("eval log|det|", lde, ldr, ld64, 2e-3)
        flow.train()
        torch.manual_seed(1)
        z1, _ = flow(xg, cg)
        torch.manual_seed(1)
        z1b, _ = flow(xg, cg)
        z2, _ = flow(xg, cg)                                    # the generator moved on: another mask
        assert torch.equal(z1, z1b) and not torch.equal(z1, z2) and not torch.equal(z1, ze)
        flow.precision = "bf16"                                 # the same factors on the bf16 instantiation
        torch.manual_seed(1)
        zb, _ = flow(xg, cg)
        dz = (zb - z1).abs().max(dim=1).values
        print(f"\n[bf16 vs fp32 mode, same seed] |dz| median {dz.median().item():.2e} max {dz.max().item():.2e}")
        assert dz.median() < 5e-3 and dz.max() < 0.5, (dz.median(), dz.max())
        with pytest.raises(RuntimeError, match="eval"):
            flow.nll_into(xg, cg, torch.empty(B, device="cuda"))
        with pytest.raises(RuntimeError, match="eval"):
            flow.sample(4, cg[:1])
    flow.zero_grad()                                            # bf16 forward, fp32 backward with the forward's factors
    flow.compute_psd_aware_nll(xg, cg, None).mean().backward()
    for name, prm in flow.named_parameters():
        if name.startswith("transform."):
            assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    wide = NSFPosteriorFlow(20, 0, 256, 1, 16, 5.0, dropout=p).cuda().train()
    with pytest.raises(NotImplementedError):                    # D > 16: no backward, with or without dropout
        wide(torch.zeros(2, 20).cuda())

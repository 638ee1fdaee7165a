"""Throughput of the generic-shape kernels on FlowHead(12, 384, 24) of experiments/frozen_context_heads.py:159-163:
forward, and the inverse on the incremental kernel (csrc/pf_flow_inc_wide.hip, the default) against the D-pass kernel
(incremental_inverse = False) at 4096 and 131 072 draws with one context row -- median of repeated timed launches."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posteriflow_amd import NSFPosteriorFlow
torch.manual_seed(0)
flow = NSFPosteriorFlow(11, 288, 384, 12, 24, 3.0, temperature_scale=1.0, use_masked_context=False).cuda().eval()
for p in flow.parameters(): p.requires_grad_(False)
B = 4096
x = torch.rand(B, 11, device="cuda") * 2 - 1
ctx = torch.randn(B, 288, device="cuda")
def t(fn, n=10):
    fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e3
def median_ms(fn, warm=3, n=15):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)[n // 2]
for prec in ("fp32", "bf16"):
    flow.precision = prec
    ms = t(lambda: flow.compute_psd_aware_nll(x, ctx, None))
    flop = 2 * 12 * (11 * 384 + 288 * 384 + 2 * (2 * 384 * 384 + 288 * 384) + 384 * 11 * 71)
    print(f"{prec}: forward {ms:.3f} ms per {B} rows = {B / ms / 1e3:.2f} M samples/s = {B * flop / ms / 1e9:.1f} TFLOP/s (dense count)")
    for draws in (4096, 131072):
        z = torch.randn(draws, 11, device="cuda")
        res = {}
        for inc in (None, False):
            flow.incremental_inverse = inc
            res[inc] = median_ms(lambda: flow.inverse(z, ctx[:1]), n=15 if draws == 4096 else 5)
            served = "incremental" if flow.incremental_inverse is None else "d-pass"
            print(f"{prec}: inverse of {draws} draws, one context row, {served} kernel: {res[inc]:.3f} ms = "
                  f"{draws / res[inc] / 1e3:.3f} M draws/s")
        flow.incremental_inverse = None
        print(f"{prec}: {draws} draws: incremental / d-pass = {res[False] / res[None]:.2f}x")
# training step of the head on frozen contexts (forward with the layer inputs kept + fp32 backward) at 2048 rows, without and with
# the reference's conditioner dropout (create_flow_model's default 0.15), both in one run
for p in flow.parameters(): p.requires_grad_(True)
flow.train()
xt, ct = x[:2048], ctx[:2048]
def step():
    flow.zero_grad(set_to_none=True)
    flow.compute_psd_aware_nll(xt, ct, None).mean().backward()
for prec in ("fp32", "bf16"):
    flow.precision = prec
    ms = {}
    for flow.dropout in (0.0, 0.15):
        ms[flow.dropout] = median_ms(step)
    print(f"{prec}: training forward + backward, 2048 rows: {ms[0.0]:.3f} ms without dropout, {ms[0.15]:.3f} ms with p = 0.15 "
          f"({ms[0.15] / ms[0.0]:.3f}x)")

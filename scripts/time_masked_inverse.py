"""Sampling throughput of masked-context flows (context_features % features == 0: the conditioner the reference switches on by
itself, flows.py:409-411): the incremental inverse (additive instantiations of csrc/pf_flow_inc.hip / pf_flow_inc_wide.hip, the
default) against the D-pass kernel (incremental_inverse = False) in the same run, at 4096 and 131 072 draws with one context
row, both precisions.  Launches are settled first; the two kernels alternate inside every repetition; median of the timed
launches (device events).  Also prints the largest difference between the two kernels' draws at the timed size."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posteriflow_amd import NSFPosteriorFlow
assert torch.cuda.is_available(), "needs the GPU"
FLOWS = {  # D, C, H, L, K
    "create_flow_model default size": (11, 264, 256, 12, 16),
    "wide head": (11, 264, 384, 12, 24),
}
def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)
for name, (D, C, H, L, K) in FLOWS.items():
    torch.manual_seed(0)
    flow = NSFPosteriorFlow(D, C, H, L, K, 3.0, temperature_scale=1.0).cuda().eval()
    assert flow.use_masked_context
    for p in flow.parameters(): p.requires_grad_(False)
    ctx = torch.randn(1, C, device="cuda")
    for prec in ("fp32", "bf16"):
        flow.precision = prec
        for draws in (4096, 131072):
            z = torch.randn(draws, D, device="cuda")
            def run(inc):
                flow.incremental_inverse = inc
                out = flow.inverse(z, ctx)
                assert inc is False or flow.incremental_inverse is None, "the incremental kernel refused the shape"
                return out
            xs = {inc: run(inc)[0] for inc in (None, False)}            # settles the launches, builds the packed states
            for _ in range(2):
                for inc in (None, False): run(inc)
            torch.cuda.synchronize()
            n = 15 if draws == 4096 else 7
            ms = {None: [], False: []}
            for _ in range(n):
                for inc in (None, False): ms[inc].append(timed(lambda: run(inc)))
            flow.incremental_inverse = None
            med = {inc: sorted(v)[n // 2] for inc, v in ms.items()}
            print(f"{name} ({D} x {C} x {H} x {K} x {L}) {prec}: {draws} draws, one context row: incremental {med[None]:.3f} ms "
                  f"({draws / med[None] / 1e3:.3f} M draws/s, min {min(ms[None]):.3f} max {max(ms[None]):.3f}), d-pass {med[False]:.3f} ms "
                  f"({draws / med[False] / 1e3:.3f} M draws/s, min {min(ms[False]):.3f} max {max(ms[False]):.3f}): "
                  f"{med[False] / med[None]:.2f}x; max |x_inc - x_dpass| = {(xs[None] - xs[False]).abs().max():.2e}", flush=True)

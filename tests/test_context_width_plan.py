"""The context-width contract of the flow plan, on the host (no kernel is launched): which kernel variant serves a context
width C, per hidden width, precision and PF_FLAG_HOIST_CTX, and where the plan refuses.

  in-layer context (plain desc):  small  C <= 96   (H = 64, 128 only)        CKM = 3 bf16 / 6 fp32 k-steps
                                  mid    C <= 288                            CKM = 9 / 18
                                  large  C <= 576  (H = 256 only)            CKM = 18 / 36
                                  refused above
  hoisted (PF_FLAG_HOIST_CTX):    every C up to 64 k-steps = 1024 fp32 / 2048 bf16 (csrc/pf_layout.h kCtxMaxCK), CKM = 0 in the
                                  chain kernel, a workspace for the projections; refused above, by name
  NSFPosteriorFlow (auto mode):   in-layer where the plain plan exists, hoisted otherwise.

A width is accepted by the plan if and only if every launcher that serves it accepts it.  This file pins the plan's half of
that statement (accepted up to the limit, refused one beyond it, by name); the launchers' half needs a device:
tests/test_flow_context_width_gpu.py runs forward, both inverses and the backward at the limit and asserts the refusals one
beyond it, tests/test_dense_gpu.py does the same for pf_flow_ctx_project_rows.  The projection kernel's context tile is CK
fragments of 1 KiB per 16-row group, 4 groups while that fits 160 KiB of LDS and 2 groups beyond, so CK <= 64 needs at most
128 KiB: the one constant kCtxMaxCK bounds make_plan, launch_ctx and pf_flow_ctx_project_rows."""
import ctypes as C
import os
import re

import pytest

SHAPES = {64: 3, 128: 6, 192: 7, 256: 5}          # H -> D
K, L = 8, 2
CKM = {"bf16": {"small": 3, "mid": 9, "large": 18}, "fp32": {"small": 6, "mid": 18, "large": 36}}
LIMIT = {"fp32": 1024, "bf16": 2048}
KW = {"fp32": 16, "bf16": 32}


@pytest.fixture(scope="module")
def lib():
    from posteriflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _desc(lib, H, c, prec, flags=0):
    return lib.PfFlowDesc(SHAPES[H], c, H, K, L, 2, 3.0, 1e-3, 1e-3, 1e-3, lib.PRECISIONS[prec], flags)


def _ckm_of(name: bytes):
    """the scheduled context k-steps in 'pf::flow_kernel<BF16, NT, R, CKM, DENSE, false>'"""
    m = re.fullmatch(r"pf::flow_kernel<(true|false), (\d+), (\d+), (\d+), (\d+), false>", name.decode())
    assert m, name
    return m.group(1) == "true", int(m.group(2)), int(m.group(4))


def _inlayer_variant(H, c):
    if c <= 96 and H <= 128:
        return "small"
    if c <= 288:
        return "mid"
    if c <= 576 and H == 256:
        return "large"
    return None


WIDTHS = [1, 95, 96, 97, 288, 289, 300, 576, 577, 640, 641, 1024, 1025, 1280, 1281, 2048, 2049, 5000]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H", list(SHAPES))
def test_inlayer_dispatch_table_and_its_boundaries(lib, H, prec):
    h = lib.lib()
    for c in WIDTHS:
        d = _desc(lib, H, c, prec)
        want = _inlayer_variant(H, c)
        n = h.pf_flow_pack_map_len(C.byref(d))
        if want is None:
            assert n < 0, (H, c)
            assert h.pf_flow_workspace_bytes(C.byref(d), 70) == -1
            assert h.pf_flow_forward_kernel_name(C.byref(d), 70) is None
            assert h.pf_flow_forward(C.byref(d), None, None, None, None, None, 4, None, None, None, None, 0, None) == lib.PF_ERR_UNSUPPORTED
            continue
        assert n > 0, (H, c)
        assert h.pf_flow_workspace_bytes(C.byref(d), 70) == 0           # nothing hoisted: no scratch
        bf, nt, ckm = _ckm_of(h.pf_flow_forward_kernel_name(C.byref(d), 70))
        assert (bf, nt, ckm) == (prec == "bf16", H // 16, CKM[prec][want]), (H, c, want)
        assert ckm * KW[prec] >= c                                       # the scheduled k-steps cover the width


@pytest.mark.parametrize("masked", [False, True], ids=["hoist", "masked_context"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H", list(SHAPES))
def test_hoisted_plans_up_to_the_projection_kernels_limit(lib, H, prec, masked):
    h = lib.lib()
    flags = lib.PF_FLAG_HOIST_CTX | (lib.PF_FLAG_MASKED_CONTEXT if masked else 0)
    lim = LIMIT[prec]
    for c in WIDTHS + [lim - 1, lim, lim + 1]:
        d = _desc(lib, H, c, prec, flags)
        n = h.pf_flow_pack_map_len(C.byref(d))
        if c > lim:
            assert n < 0, (H, c)
            msg = h.pf_last_error().decode()
            assert str(c) in msg and str(lim) in msg, msg             # refused by name: the width and the limit
            assert h.pf_flow_workspace_bytes(C.byref(d), 70) == -1
            assert h.pf_flow_forward_kernel_name(C.byref(d), 70) is None
            for call in (lambda: h.pf_flow_forward(C.byref(d), None, None, None, None, None, 4, None, None, None, None, 0, None),
                         lambda: h.pf_flow_inverse(C.byref(d), None, None, None, 4, None, 4, None, None, None, None, 0, None)):
                assert call() == lib.PF_ERR_UNSUPPORTED
                msg = h.pf_last_error().decode()
                assert str(c) in msg and str(lim) in msg, msg
            continue
        assert n > 0, (H, c)
        for rows, blocks in ((1, 1), (64, 1), (70, 2), (129, 3)):        # projections of whole 64-row blocks, fp32
            assert h.pf_flow_workspace_bytes(C.byref(d), rows) == blocks * 64 * 3 * L * H * 4
        bf, nt, ckm = _ckm_of(h.pf_flow_forward_kernel_name(C.byref(d), 70))
        assert (bf, nt, ckm) == (prec == "bf16", H // 16, 0)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H", list(SHAPES))
def test_module_picks_inlayer_where_it_exists_and_hoists_above(lib, H, prec):
    """NSFPosteriorFlow._desc in auto mode (no device needed): forward in-layer up to the variant's width, hoisted above;
    the inverse always hoisted; beyond the limit no plan (forward_kernel_name has nothing to name)."""
    from posteriflow_amd import NSFPosteriorFlow
    for c in (96, 97, 288, 289, 576, 577, LIMIT[prec], LIMIT[prec] + 1):
        flow = NSFPosteriorFlow(SHAPES[H], c, H, L, K, 3.0, temperature_scale=1.0, use_masked_context=False)
        flow.precision = prec
        name = flow.forward_kernel_name(70)
        if c > LIMIT[prec]:
            assert name == "?"
            assert lib.lib().pf_flow_pack_map_len(C.byref(flow._desc(inverse=True))) < 0
            continue
        want = _inlayer_variant(H, c)
        assert _ckm_of(name.encode())[2] == (CKM[prec][want] if want else 0), (H, c, name)
        assert flow._desc(inverse=True).reserved & lib.PF_FLAG_HOIST_CTX
        assert lib.lib().pf_flow_pack_map_len(C.byref(flow._desc(inverse=True))) > 0

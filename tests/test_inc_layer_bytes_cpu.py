"""pf_flow_inc_layer_bytes over the domain of the two incremental-inverse kernels (host code only, no GPU)."""
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from posteriflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _bytes(lib, D, H, K, prec):
    desc = lib.PfFlowDesc(D, 0, H, K, 2, 2, 3.0, 1e-3, 1e-3, 1e-3, lib.PRECISIONS[prec], 0)
    return lib.lib().pf_flow_inc_layer_bytes(desc)


def _formula(D, H, K, prec):
    """include/pf_hip.h: W0 | four hidden matrices | final layer as 1 KB fragments, then the fp32 biases"""
    nt, hk, tail = H // 16, H // (16 if prec == "fp32" else 32), 3 if K <= 16 else 6
    return (nt + 4 * nt * hk + tail * D * hk) * 1024 + (5 * H + 16 * tail * D) * 4


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_inc_layer_bytes_domain(lib, prec):
    assert _bytes(lib, 11, 256, 16, prec) == _formula(11, 256, 16, prec)           # the scheduled shape: unchanged
    assert _bytes(lib, 11, 384, 24, prec) == _formula(11, 384, 24, prec) > 0       # 96 final-layer rows per feature
    assert _bytes(lib, 8, 256, 20, prec) == _formula(8, 256, 20, prec)
    want_512 = _formula(6, 512, 32, prec) if prec == "bf16" else -1                # fp32 stops at H = 384
    assert _bytes(lib, 6, 512, 32, prec) == want_512
    for D, H, K in ((6, 544, 8), (6, 400, 8), (6, 384, 33), (17, 384, 24)):
        assert _bytes(lib, D, H, K, prec) == -1

"""CPU checks of the attention route choice (hip/ops.attn_route is host arithmetic: no GPU) and of where the autograd nodes keep
what their backward needs."""
import os

import pytest

import cape_amd  # noqa: F401
from cape_amd.hip import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (flash=, precision, N, H, Lq, Lk, route): literals derived from flash_attn_ok / attn_mm_ok as they stood before attn_route
ROUTES = [
    (True, "bf16x3", 2, 8, 200, 200, "flash"),
    (True, "bf16x3", 2, 8, 40, 40, "flash"),
    (True, "f32", 2, 8, 200, 200, "mm"),             # the fused kernels are bf16x3 only
    (True, "bf16x3", 2, 8, 228, 228, "mm"),          # beyond FLASH_MAX_L
    (True, "bf16x3", 2, 8, 230, 230, "scalar"),      # ... and not a multiple of 4
    (False, "bf16x3", 2, 8, 200, 200, "mm"),         # flash only for callers that allow it
    (False, "bf16x3", 2, 8, 68, 68, "mm"),
    (False, "bf16x3", 2, 8, 17, 17, "scalar"),
    (False, "bf16x3", 2, 8, 100, 17, "scalar"),
    (False, "bf16x3", 8192, 8, 68, 68, "scalar"),    # N * H = 65536: one batched launch cannot address it
]


def test_route_table(monkeypatch):
    monkeypatch.delenv("CAPE_FLASH_ATTN", raising=False)
    monkeypatch.delenv("CAPE_ATTN_MM", raising=False)
    old = ops.get_gemm_precision()
    try:
        for flash, prec, N, H, Lq, Lk, want in ROUTES:
            ops.set_gemm_precision(prec)
            assert ops.attn_route(N, H, Lq, Lk, flash=flash) == want, (flash, prec, N, H, Lq, Lk)
        # the switches are read at call time
        ops.set_gemm_precision("bf16x3")
        monkeypatch.setenv("CAPE_FLASH_ATTN", "0")
        assert ops.attn_route(2, 8, 200, 200, flash=True) == "mm"
        monkeypatch.setenv("CAPE_ATTN_MM", "0")
        assert ops.attn_route(2, 8, 200, 200, flash=True) == "scalar"
    finally:
        ops.set_gemm_precision(old)


def test_route_is_built_from_the_public_predicates():
    old = ops.get_gemm_precision()
    try:
        for prec in ("bf16x3", "f32"):
            ops.set_gemm_precision(prec)
            for N, H, L in ((2, 8, 16), (2, 8, 32), (2, 8, 64), (2, 8, 224), (2, 8, 225), (2, 8, 228), (9000, 8, 100)):
                fl, mm = ops.flash_attn_ok(N, H, L, L), ops.attn_mm_ok(N, H, L, L)
                assert ops.attn_route(N, H, L, L, flash=True) == ("flash" if fl else "mm" if mm else "scalar")
                assert ops.attn_route(N, H, L, L) == ("mm" if mm else "scalar")
    finally:
        ops.set_gemm_precision(old)


def test_nodes_hold_no_route_state():
    """Everything an attention backward reads goes through save_for_backward, and the route is one string: no bare tensor
    attributes or route flags on ctx."""
    src = open(os.path.join(ROOT, "category-agnostic-pose-estimation_amd", "hip", "functional.py")).read()
    assert "ctx.Pu" not in src and "ctx.flash" not in src
    assert "attn_mm_ok" not in src and "flash_attn_ok" not in src
    assert "ctx.route" in src


def test_unknown_route_is_an_error():
    with pytest.raises(KeyError):
        ops.attn_core_fwd("tensor-core", None, None, None, 1, 8, 17, 17, 1.0)

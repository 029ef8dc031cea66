"""Isolated timing of the MSDA forward and backward forms on the encoder / decoder shapes of the CAPE training step: the default
four levels, then -- for the record -- `--num_feature_levels` 1 (C5), 1 with `--dilation` (DC5) and 3 (C3..C5)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cape_amd  # noqa: E402,F401
from cape_amd.hip import ops  # noqa: E402


def level_configs(R):
    """(label, level grids) at image size R: strides 8, 16, 32 (+ the extra stride-2 level); DC5 keeps C5 at stride 16."""
    c3, c4, c5, c6 = (R // 8,) * 2, (R // 16,) * 2, (R // 32,) * 2, (R // 64,) * 2
    return [("4 levels", [c3, c4, c5, c6]), ("1 level", [c5]), ("1 level + dilation", [c4]), ("3 levels", [c3, c4, c5])]


def main():
    R = int(os.environ.get("IMAGE", "256"))
    for label, shapes in level_configs(R):
        print(f"--- {label} at {R} x {R}: {shapes}, S = {sum(h * w for h, w in shapes)}", flush=True)
        bench(shapes)


def bench(shapes):
    geo = ops.LevelGeometry(shapes)
    L = geo.L
    for N, Lq in ((32, geo.S), (32, 40), (8, geo.S)):
        g = torch.Generator(device="cuda").manual_seed(0)
        value = torch.randn(N, geo.S, 256, device="cuda", generator=g)
        off = torch.randn(N, Lq, 64 * L, device="cuda", generator=g) * float(os.environ.get("OFF_SCALE", "1.5"))
        offw = torch.cat([off, torch.randn(N, Lq, 32 * L, device="cuda", generator=g)], -1).contiguous()
        ref = torch.rand(N, Lq, L, 2, device="cuda", generator=g)
        go = torch.randn(N, Lq, 256, device="cuda", generator=g)
        for _ in range(3):
            ops.msda_fwd(value, offw, ref, geo, N, Lq)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.msda_fwd(value, offw, ref, geo, N, Lq)
        e1.record()
        torch.cuda.synchronize()
        print(f"N={N} Lq={Lq} forward: {e0.elapsed_time(e1) / 20 * 1e3:9.1f} us", flush=True)
        for form in ("atomic", "f64", "fx"):
            for need_ref in (False, True):
                for _ in range(3):
                    ops.msda_bwd(go, value, offw, ref, geo, N, Lq, need_ref_grad=need_ref, form=form)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                it = 10
                e0.record()
                for _ in range(it):
                    ops.msda_bwd(go, value, offw, ref, geo, N, Lq, need_ref_grad=need_ref, form=form)
                e1.record()
                torch.cuda.synchronize()
                print(f"N={N} Lq={Lq} form={form} d_ref={need_ref}: {e0.elapsed_time(e1) / it * 1e3:9.1f} us", flush=True)


if __name__ == "__main__":
    main()

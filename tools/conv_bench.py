"""Isolated timing of the implicit-GEMM convolution modes (forward im2col, dgrad gather) against the dense product of the same
shape: the 3x3 convolutions of the ResNet trunk at the CAPE batch (32 images, 256 x 256 input), and layer4's 3x3 of the
`--dilation` (DC5) trunk -- 16 x 16, dilation 2, padding 2 -- next to the same shape at dilation 1.

    python tools/conv_bench.py [--hash] [--max-dilation D]

--hash           also print a sha256 of the forward output and of the data gradient (inputs are seeded): two builds of the library
                 can be compared bit for bit
--max-dilation D skip rows with a larger dilation (a library built before cape_gemm_desc had the field ignores it)"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cape_amd  # noqa: E402,F401
from cape_amd.hip import ops  # noqa: E402

# (N, H, W, C, O, stride, dilation): layer2 / layer3 / layer4 3x3 convolutions; layer4 of the DC5 trunk undilated and dilated
ROWS = [(32, 32, 32, 128, 128, 1, 1), (32, 16, 16, 256, 256, 1, 1), (32, 8, 8, 512, 512, 1, 1), (32, 32, 32, 256, 256, 2, 1),
        (32, 16, 16, 512, 512, 1, 1), (32, 16, 16, 512, 512, 1, 2)]


def t(fn, it=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3


def sha(x):
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hash", action="store_true")
    ap.add_argument("--max-dilation", type=int, default=None)
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    for (N, H, W, C, O, s, d) in ROWS:
        if a.max_dilation is not None and d > a.max_dilation:
            continue
        KH = KW = 3
        pad = d
        OH, OW = (H + 2 * pad - d * (KH - 1) - 1) // s + 1, (W + 2 * pad - d * (KW - 1) - 1) // s + 1
        M, K = N * OH * OW, KH * KW * C
        x = torch.randn(N, H, W, C, device=dev)
        w = torch.randn(O, KH, KW, C, device=dev)                 # physical layout of a channels_last conv weight
        y = torch.empty(N, OH, OW, O, device=dev)
        dy = torch.randn(N, OH, OW, O, device=dev)
        dx = torch.empty(N, H, W, C, device=dev)
        geom = (N, H, W, C, KH, KW, s, pad, OH, OW, O)
        xd = torch.randn(M, K, device=dev)
        us_f = t(lambda: ops.gemm(x, w, y, M, O, K, a_mode=2, b_mode=0, conv=geom, conv_dil=d))
        hashes = f" || sha256 fwd {sha(y)}" if a.hash else ""
        us_d = t(lambda: ops.gemm(xd, w.view(O, K), y.view(M, O), M, O, K))
        fl = 2.0 * M * O * K
        line = f"N={N} {H}x{W} C={C} O={O} s={s} d={d}: fwd im2col {us_f:7.1f} us ({fl / us_f / 1e6:6.1f} TF/s) | dense {M}x{O}x{K} {us_d:7.1f} us ({fl / us_d / 1e6:6.1f} TF/s)"
        Md, Kd = N * H * W, KH * KW * O
        us_g = t(lambda: ops.gemm(dy, w, dx, Md, C, Kd, a_mode=3, b_mode=2, conv=geom, conv_dil=d))
        if a.hash:
            hashes += f" dgrad {sha(dx)}"
        dyd = torch.randn(Md, Kd, device=dev)
        wt = torch.randn(Kd, C, device=dev)
        us_gd = t(lambda: ops.gemm(dyd, wt, dx.view(Md, C), Md, C, Kd, b_mode=1))
        fl2 = 2.0 * Md * C * Kd
        line += f" || dgrad gather {us_g:7.1f} us ({fl2 / us_g / 1e6:6.1f} TF/s) | dense NN {us_gd:7.1f} us ({fl2 / us_gd / 1e6:6.1f} TF/s)"
        print(line + hashes, flush=True)


if __name__ == "__main__":
    main()

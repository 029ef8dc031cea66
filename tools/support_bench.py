"""Isolated timing of the support encoder (forward + backward, training mode) at the headline batch: 32 graphs x 17
keypoints.  Default: the geometric encoder with the GCN pre-encoder.  LEGACY=1: the reference's default SupportPoseGraphEncoder
(models/support_encoder.py).  Reports GPU us and kernel launches per step (launches counted by a torch profiler pass)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cape_amd  # noqa: E402,F401
from cape_amd.hip import functional as HF  # noqa: E402
from cape_amd.models.geometric_support_encoder import GeometricSupportEncoder  # noqa: E402
from cape_amd.models.support_encoder import SupportPoseGraphEncoder  # noqa: E402


def launches(fn):
    """Kernel launches of one call of fn (device-side kernel events of a profiler pass; copies and fills not counted)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset")))


def main():
    B, P = int(os.environ.get("GRAPHS", "32")), int(os.environ.get("POINTS", "17"))
    legacy = os.environ.get("LEGACY", "0") == "1"
    torch.manual_seed(0)
    enc = (SupportPoseGraphEncoder() if legacy else GeometricSupportEncoder(use_gcn_preenc=True)).cuda().train()
    name = "default (SupportPoseGraphEncoder)" if legacy else "geometric + GCN"
    coords = torch.rand(B, P, 2, device="cuda")
    mask = torch.zeros(B, P, dtype=torch.bool, device="cuda")
    mask[:, 14:] = True
    if legacy:
        mask = ~mask                 # the default encoder takes the sampler's mask un-inverted (CAPEModel): pad the same keypoints
    sk = [[[i, i + 1] for i in range(13)] for _ in range(B)]
    HF.Runtime.seed(1, "cuda")

    def fwd():
        return enc(coords, mask, sk)

    def step():
        out = fwd()
        out.backward(torch.ones_like(out))
        HF.Runtime.join()

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    import time
    t0 = time.perf_counter()
    e0.record()
    for _ in range(20):
        step()
    e1.record()
    torch.cuda.synchronize()
    n_fwd = launches(fwd)
    n_step = launches(step)
    print(f"{name} fwd+bwd, {B} graphs x {P} points: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us GPU, "
          f"{(time.perf_counter() - t0) / 20 * 1e3:.2f} ms wall, {n_fwd} launches forward, {n_step - n_fwd} backward")
    with torch.no_grad():
        enc.eval()
        for _ in range(3):
            fwd()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            fwd()
        e1.record()
        torch.cuda.synchronize()
        print(f"{name} forward (eval): {e0.elapsed_time(e1) / 20 * 1e3:.1f} us, {launches(fwd)} launches")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""bench.py -- episodes/sec of the CAPE episodic TRAINING step on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

A step = one pass of the hot path over one batch of synthetic episodes: forward (backbone, encoder,
support encoder, decoder), fused criterion, backward, gradient all-reduce (N > 1), global-norm clip,
AdamW -- dropout ON (train mode); fp32 storage and accumulation, the GEMMs as a bf16x3 split on the bf16 matrix cores by
default (CAPE_GEMM_PRECISION=f32 = exact fp32 MFMA).
Workload = BASELINE.json configs[1]:
1-shot, 256x256, 17 keypoints, ResNet-50 + deformable transformer, 16 episodes x 2 queries per GPU.
Weak scaling: every rank processes its own 16 episodes (pure data parallel, episodes are independent).
Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0.

The optimizer runs at learning rate 0: the AdamW kernel does all of its work (moments, clip, weight re-pack) but leaves the
weights as they are, so every step computes from the same seeded weights.  Its backward reductions are float atomics, and
this model turns their arrival-order rounding into ~3e-3 of the gradient (profiles/r02_determinism.txt); a real learning rate
would feed that back into the next step's forward pass and no two runs would compute the same losses.

A plain run measures the headline alone: W warm-up steps, a short probe of both launch modes (eager, replayed hipGraph), then
K timed steps in the faster one (in the replayed hipGraph alone with --graph).  --dump-outputs DIR then writes what the last timed step returned to its caller -- every loss term, float64 -- as
DIR/losses.<name>.npy.  --full adds everything else: both launch modes timed
over the same K steps with the faster as the headline, the GEMM-family roofline, the same step in the other GEMM arithmetic
modes (`alt_exact_f32`, `alt_bf16`), the CPU baseline, the data-pipeline rate, and at N = 1 `decode` (BASELINE configs[4]:
5-shot KV-cached autoregressive decode at 512x512 with 68 support keypoints -- time per decode step, tokens/s, eager and
replayed hipGraphs, against the weight-streaming roof) and `pck_check` (the same synthetic episode decoded by the product and
by the CPU oracle: PCK@0.2 of both, token streams compared).  Blocks a run does not measure are null in the line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# algorithmic work: training FLOPs per episode at 256x256 (2 query images)
GFLOP_PER_EPISODE_256 = 162.9
PEAK_F32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: bf16 MFMA, dense
PEAK_HBM_TBPS = 8.0                # MI355X_MICROARCH.md: HBM3E peak


def make_batches(tok, B, K, R, P, n_batches, seed, device):
    from cape_amd.datasets import episodic_collate_fn
    from cape_amd.datasets.synthetic import SyntheticEpisodes
    ds = SyntheticEpisodes(tok, B * n_batches, R, P, K, seed=seed)
    out = []
    for i in range(n_batches):
        b = episodic_collate_fn([ds[i * B + j] for j in range(B)])
        out.append({"images": b["query_images"].to(device), "support_coords": b["support_coords"].to(device),
                    "support_mask": b["support_masks"].to(device), "skeleton": b["support_skeletons"],
                    "targets": {k: v.to(device) for k, v in b["query_targets"].items()}})
    return out


def host_cores():
    """CPU share of this process: affinity mask, cgroup quota, capped at the GPU box's documented share (16)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 16))


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def csrc_tree_hash():
    """sha256 over the kernel sources (csrc/*.hip, *.h, include/cape_hip.h): ties a committed counter file to the kernels it measured."""
    import glob
    import hashlib
    h = hashlib.sha256()
    base = os.path.join(ROOT, "category-agnostic-pose-estimation_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(base, "*.hip")) + glob.glob(os.path.join(base, "*.h")) + [os.path.join(ROOT, "include", "cape_hip.h")]):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def data_pipeline_benchmark(device, seconds=6.0, num_workers=4):
    """Row f2: episodes/s of the LOADER ALONE on an MP-100-shaped synthetic file set (COCO json + PNG files written to a temp
    directory by the generator the data-path tests use): DataLoader workers decode + crop + draw plans + tokenise, the GPU makes the
    pixels (datasets/transforms.DeviceImagePipeline -> cape_augment_batch).  Compared with the training step's episodes/s it says
    whether the input pipeline can feed one GPU."""
    import shutil
    import tempfile
    from cape_amd.datasets import EpisodicDataset, MP100CAPE, episodic_collate_fn
    from cape_amd.datasets.transforms import HostTransform
    from cape_amd.models.engine_cape import _query_images
    from tests.test_data_path_cpu import make_dataset
    from pathlib import Path
    tmp = Path(tempfile.mkdtemp(prefix="cape_bench_data_"))
    try:
        ann = make_dataset(tmp, n_per_cat=12, scale=4)
        out = {}
        for label, defer in (("gpu_augment", True), ("host_augment", False)):
            ds = MP100CAPE(str(tmp / "data"), str(ann), HostTransform(train=True, size=512, seed=1), vocab_size=2000, seq_len=200,
                           defer_pixels=defer)
            ep = EpisodicDataset(ds, str(tmp / "category_splits.json"), split="train", num_queries_per_episode=2, episodes_per_epoch=4096,
                                 seed=3, load_support_images=False)
            dl = torch.utils.data.DataLoader(ep, 16, collate_fn=episodic_collate_fn, num_workers=num_workers, pin_memory=not defer,
                                             persistent_workers=False, prefetch_factor=4 if num_workers else None)
            it = iter(dl)
            b = next(it)                                            # workers are up, first batch made
            _query_images(b, device); torch.cuda.synchronize()
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < seconds:
                b = next(it)
                imgs = _query_images(b, device)
                n += imgs.shape[0] // 2
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[label] = round(n / dt, 1)
            del it, dl
        return {"unit": "episodes/s (16 episodes x 2 queries per batch, 512x512 output, training augmentation)", "num_workers": num_workers,
                "host_cores": host_cores(), **out,
                "dataset": "synthetic MP-100-shaped file set (tests/test_data_path_cpu.make_dataset, scale 4: COCO json + 240-560 x 200-480 PNG images)",
                "note": "gpu_augment: workers decode / crop / plan / tokenise, cape_augment_batch makes the pixels; host_augment: the same "
                        "plans applied by torch CPU ops inside the workers (CAPE_HOST_AUGMENT=1)"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cpu_baseline(args_ns, seconds_budget=20.0):
    """The oracle (CPU restatement, kind='port') timed on this box's host cores on a bounded sample of the
    same workload: train step (fwd + loss + bwd + AdamW, dropout on) on 2 episodes x 2 queries at 256x256."""
    from oracle import cape_ref, procweights, synth
    cfg = cape_ref.Cfg()
    cores = host_cores()
    torch.set_num_threads(cores)
    log(f"cpu_baseline: oracle train step on {cores} host threads")
    sd = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "backbone.0.body.layer1" not in k and ".bn" not in k
                                      and "downsample.1" not in k and "body.conv1" not in k and "attention_mask" not in k
                                      and "pos_embed" not in k and ".pe" not in k)
          for k, v in procweights.procedural_state_dict().items()}
    params = [v for v in sd.values() if v.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-4)
    b = synth.make_batch(1, 2, 2, 256, 17, cfg, n_invisible=(2, 0))

    def step():
        opt.zero_grad(set_to_none=True)
        out = cape_ref.cape_forward(sd, cfg, b["images"], b["support_coords"], b["support_mask"], b["targets"],
                                    b["skeleton"], train=True)
        _, _, total = cape_ref.criterion(out, b["targets"], cfg)
        total.backward()
        torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], 0.1)
        opt.step()

    tw = time.time()
    step()                                   # warm-up
    log(f"cpu_baseline: warm-up step {time.time() - tw:.1f} s")
    n, t0 = 0, time.time()
    while n < 2 or (time.time() - t0 < seconds_budget and n < 8):
        step()
        n += 1
        log(f"cpu_baseline: step {n} at {time.time() - t0:.1f} s")
    dt = (time.time() - t0) / n
    return {"value": 2.0 / dt, "unit": "episodes/s", "cores": cores, "kind": "port",
            "sample": f"{n} train steps of 2 episodes x 2 queries, 256x256, 17 kpt (oracle/cape_ref.py, torch CPU fp32, {cores} threads)"}


def pck_check(device, steps=24):
    """One synthetic episode (2 queries, 256x256, 17 keypoints) decoded for `steps` tokens by the product (HIP) and by the
    oracle (oracle/cape_ref.py on the host, the checker): PCK@0.2 of both against the synthetic ground truth, token streams
    and logits compared.  Random-init weights, identical in both (the product's state_dict feeds the oracle)."""
    import argparse as _ap
    from cape_amd.datasets import DiscreteTokenizerV2, episodic_collate_fn
    from cape_amd.datasets.synthetic import SyntheticEpisodes
    from cape_amd.models import build_model
    from cape_amd.models.cape_model import build_cape_model
    from cape_amd.models.engine_cape import extract_keypoints_from_predictions
    from cape_amd.models.train_cape_episodic import get_args_parser
    from cape_amd.util.eval_utils import PCKEvaluator
    from oracle import cape_ref
    args = _ap.ArgumentParser(parents=[get_args_parser()]).parse_args(["--use_geometric_encoder", "--use_gcn_preenc"])
    torch.manual_seed(7)
    tok = DiscreteTokenizerV2(44, steps)
    base, _ = build_model(args, tokenizer=tok)
    model = build_cape_model(args, base).to(device).eval()
    with torch.no_grad():                       # spread the class head so that the stream is not all-<coord>
        model.base_model.class_embed[5].bias.copy_(torch.tensor([0.3, 0.0, -0.2]))
    ds = SyntheticEpisodes(tok, 1, 256, 17, 2, seed=11)
    b = episodic_collate_fn([ds[0]])
    os.environ["WARN_INCOMPLETE_GENERATION"] = "0"
    with torch.no_grad():
        p = model.forward_inference(b["query_images"].to(device), b["support_coords"].to(device), b["support_masks"].to(device),
                                    skeleton_edges=b["support_skeletons"], graph=False)
    sd = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    torch.set_num_threads(host_cores())
    with torch.no_grad():
        o = cape_ref.cape_forward_inference(sd, cape_ref.Cfg(), b["query_images"], b["support_coords"], b["support_masks"],
                                            b["support_skeletons"], max_len=steps)

    def pck_of(logits, coords):
        ev = PCKEvaluator(threshold=0.2)
        k = extract_keypoints_from_predictions(coords, logits)
        pl, gl, bw, bh, vl = [], [], [], [], []
        for i, m in enumerate(b["query_metadata"]):
            n = len(m["visibility"])
            pk = k[i, :n] if k.shape[1] >= n else torch.cat([k[i], torch.zeros(n - k.shape[1], 2)])
            pl.append(pk.numpy() * 512.0); gl.append(np.asarray(m["keypoints"]) * 512.0)
            bw.append(m["bbox_width"]); bh.append(m["bbox_height"]); vl.append(m["visibility"])
        ev.add_batch(pl, gl, bw, bh, category_ids=[1] * len(pl), visibility=vl)
        return ev.get_results()["pck_overall"]

    T = min(p["logits"].shape[1], o["logits"].shape[1])
    lp, lo = p["logits"].cpu()[:, :T], o["logits"][:, :T]
    pck_p, pck_o = pck_of(p["logits"].cpu(), p["coordinates"].cpu()), pck_of(o["logits"], o["coordinates"])
    return {"workload": f"1 episode x 2 queries, 256x256, 17 kpt, {steps} decode steps, random-init weights",
            "pck_product": round(pck_p, 6), "pck_oracle": round(pck_o, 6), "pck_equal": bool(abs(pck_p - pck_o) <= 1e-3),
            "steps_product": int(p["logits"].shape[1]), "steps_oracle": int(o["logits"].shape[1]),
            "tokens_equal": bool(p["logits"].shape == o["logits"].shape and torch.equal(lp.argmax(-1), lo.argmax(-1))),
            "max_abs_logit_diff": round(float((lp - lo).abs().max()), 6),
            "max_abs_coord_diff": round(float((p["coordinates"].cpu()[:, :T] - o["coordinates"][:, :T]).abs().max()), 7)}


def bf16_logit_error(device):
    """Max |logit - reference| of the eval-mode forward at 256x256 (tests/golden/e2e256.npz, emitted by the real reference) in each
    GEMM arithmetic mode; the oracle package only supplies the procedural weights and the seeded inputs of that fixture (checker)."""
    try:
        from cape_amd.hip import ops
        from oracle import cape_ref, procweights, synth
        from tests.helpers import build_product
        d = np.load(os.path.join(ROOT, "tests", "golden", "e2e256.npz"))
        args, tok, model, crit = build_product(proc_sd=procweights.procedural_state_dict(), device=device)
        model.eval()
        b = synth.make_batch(23, 1, 2, 256, 17, cape_ref.Cfg(), n_invisible=(2,))
        out = {}
        old = ops.get_gemm_precision()
        for name in ("bf16", "bf16x3", "f32"):
            ops.set_gemm_precision(name)
            with torch.no_grad():
                o = model(samples=b["images"].to(device), support_coords=b["support_coords"].to(device), support_mask=b["support_mask"].to(device),
                          targets={k: v.to(device) for k, v in b["targets"].items()}, skeleton_edges=b["skeleton"])
            lg = torch.stack([x["pred_logits"] for x in o["aux_outputs"]] + [o["pred_logits"]])[:, :, :24].cpu()
            out[name] = round(float((lg - torch.from_numpy(d["logits"])).abs().max()), 7)
        ops.set_gemm_precision(old)
        return {"max_abs_logit_error_vs_reference_256": out, "tolerance": 1e-3}
    except Exception as e:                                   # the fixture travels with the repo; never lose the line to this block
        return {"error": f"{type(e).__name__}: {e}"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=16, help="episodes per GPU per step (configs[1]: 16)")
    ap.add_argument("--image_size", type=int, default=256)
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--no_roofline", action="store_true")
    ap.add_argument("--graph", action="store_true",
                    help="time only the hipGraph replay of the captured step (runtime/graph_step.py); by default a plain run "
                         "times the K steps in the launch mode that was faster over a short probe, and --full at N = 1 times "
                         "both launch modes over the same K steps with the faster one as the headline (both are reported)")
    ap.add_argument("--no_decode", action="store_true", help="skip the configs[4] decode block and the PCK check")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement besides the headline (second launch mode, roofline, other GEMM "
                         "arithmetic modes, CPU baseline, data pipeline, decode, PCK check); the --no_* switches prune it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the losses the last timed step returned as DIR/losses.<name>.npy (float64)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
    # rehearsal switches (not used by the driver): all ranks on cuda:0 with gloo carrying the CUDA buckets, to exercise the
    # N > 1 code path on a one-GPU box
    if os.environ.get("CAPE_BENCH_SAME_DEVICE"):
        local = 0
    torch.cuda.set_device(local)
    device = torch.device(f"cuda:{local}")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("CAPE_BENCH_BACKEND", "nccl"), rank=rank, world_size=world)
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"

    import cape_amd  # noqa: F401
    from cape_amd.datasets import DiscreteTokenizerV2
    from cape_amd.hip import functional as HF
    from cape_amd.hip import ops
    from cape_amd.models import build_model
    from cape_amd.models.cape_model import build_cape_model
    from cape_amd.models.train_cape_episodic import get_args_parser
    from cape_amd.runtime.data_parallel import EpisodeDataParallel
    from cape_amd.runtime.optimizer import ArenaAdamW

    args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(
        ["--use_geometric_encoder", "--use_gcn_preenc", "--image_size", str(a.image_size)])
    # the eager step is bound by the host: keep the autograd engine on the calling thread (no hand-off to a worker thread per
    # backward call; tools/host_profile.py: enqueue 29.7 -> 28.1 ms per step), as engine_cape.run_training does
    torch.autograd.set_multithreading_enabled(False)
    torch.manual_seed(1234)                      # identical random-init weights on every rank
    tok = DiscreteTokenizerV2(44, args.seq_len)
    base, crit = build_model(args, tokenizer=tok)
    model = build_cape_model(args, base).to(device)
    crit = crit.to(device)
    model.train()
    HF.Runtime.seed(1000 + rank, device)
    # learning rate 0 (module docstring): same kernels and work per step, weights unchanged, losses reproducible run to run
    opt = ArenaAdamW(model, lr=0.0, lr_backbone=0.0, weight_decay=args.weight_decay, max_norm=args.clip_max_norm)
    ddp = EpisodeDataParallel(model, opt) if world > 1 else None
    B, K = a.episodes, 2
    batches = make_batches(tok, B, K, a.image_size, 17, 4, seed=100 + rank, device=device)
    rng = HF.Runtime.get_rng(device)
    scale = 1.0 / world
    last = {}

    # the step can be captured after two eager calls and replayed (runtime/graph_step.py): one hipGraph at N = 1, two graphs
    # around the bucket all-reduces under data parallelism; --full times both launch modes and the faster is the headline
    state = {"gstep": None}

    def step(i, eager=False, keep=False):
        """One training step; `keep`: hold on to its losses (detached) for --dump-outputs."""
        b = batches[i % len(batches)]
        gstep = state["gstep"]
        if gstep is not None and not eager:
            losses = gstep(b["images"], b["support_coords"], b["support_mask"], b["targets"], b["skeleton"])
            last["loss"] = losses["_total"]
            if keep:
                last["losses"] = losses
            return
        rng.advance()
        out = model(samples=b["images"], support_coords=b["support_coords"], support_mask=b["support_mask"],
                    targets=b["targets"], skeleton_edges=b["skeleton"])
        losses = crit(out, b["targets"])
        total = losses["_total"]
        (total * scale).backward()
        if ddp is not None:
            ddp.finish()
        opt.step()
        opt.zero_grad()
        last["loss"] = total.detach()
        if keep:                                 # detached: a live autograd graph would keep this step's activations alive
            last["losses"] = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in losses.items()}

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_region(label, warmup, collect=False):
        """W untimed warm-up steps, then exactly K steps between barrier + synchronize on both sides; `collect`: also return
        the losses the last of them returned to its caller, as float64 arrays."""
        for i in range(warmup):
            step(i)
            if i == 0:
                torch.cuda.synchronize()
                log(f"[{label}] first step done")
        sync()
        log(f"[{label}] timing {a.steps} steps")
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(warmup + i, keep=collect and i == a.steps - 1)
        t_enq = time.perf_counter() - t0             # host time to enqueue the steps (launch-bound if ~ the timed region)
        sync()
        dt = time.perf_counter() - t0
        res = {"dt": dt, "host_enqueue_ms_per_step": round(t_enq / a.steps * 1e3, 2), "host_ms_one_step": None,
               "loss": float(last["loss"])}
        if collect:
            res["outputs"] = {f"losses.{k}": np.asarray(float(v), dtype=np.float64) for k, v in last.pop("losses").items()}
        if a.full:
            t1 = time.perf_counter()
            step(warmup + a.steps)                   # one step into an empty queue: pure host launch cost, no back-pressure
            res["host_ms_one_step"] = round((time.perf_counter() - t1) * 1e3, 2)
            sync()
        one = "" if res["host_ms_one_step"] is None else f"; {res['host_ms_one_step']:.2f} ms for one step into an empty queue"
        log(f"[{label}] host enqueue {t_enq / a.steps * 1e3:.2f} ms/step in the timed region{one}; timed region {dt:.3f} s")
        return res

    log(f"model built, {len(batches)} batches of {B} episodes resident; warm-up x{a.warmup}")
    from cape_amd.runtime.graph_step import GraphedTrainStep

    def graph_step():
        # N > 1: the step as two captured graphs around the bucket all-reduces (runtime/graph_step.py, ddp=): exchange not
        # overlapped with the backward pass, host work ~2 replays + one collective call per bucket
        return GraphedTrainStep(model, crit, opt, loss_scale=scale, edge_capacity=2048, eager_steps=2, ddp=ddp)

    def faster_mode(n=8):
        """Both launch modes warmed up, then n steps of each between synchronizes: the faster one (eager while the host keeps
        up with the GPU, the replayed graph when it does not).  The same steps run whichever mode wins."""
        t = {}
        for mode, warm in (("eager", max(a.warmup, 1)), ("graph", 4)):      # graph: 2 eager calls + capture + first replay
            if mode == "graph":
                state["gstep"] = graph_step()
            for i in range(warm):
                step(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                step(i)
            torch.cuda.synchronize()
            t[mode] = time.perf_counter() - t0
        best = min(sorted(t), key=lambda k: t[k])
        if best != "graph":
            state["gstep"] = None
        log(f"launch-mode probe, {n} steps each: eager {t['eager'] / n * 1e3:.2f} ms/step, graph {t['graph'] / n * 1e3:.2f} ms/step -> {best}")
        return best

    # --full times both launch modes over the K steps and the faster is the headline; a plain run times the K steps once, in
    # the mode that was faster over a short probe (N = 1), or in the one --graph names
    collect = bool(a.dump_outputs) and rank == 0
    probed = not a.full and world == 1 and not a.graph
    if a.full:
        run = [m for m, on in (("eager", not (world == 1 and a.graph)),
                               ("graph", world == 1 or os.environ.get("CAPE_BENCH_DP_GRAPH", "1") == "1")) if on]
    else:
        run = [faster_mode()] if probed else ["graph" if a.graph else "eager"]
    modes = {}
    for mode in run:
        if mode == "graph" and state["gstep"] is None:
            state["gstep"] = graph_step()
        warm = 0 if probed else (a.warmup if mode == "eager" else max(a.warmup, 4))
        modes[mode] = timed_region(mode, warm, collect)
    if world > 1:                                # the slowest rank's time per mode: every rank then picks the same mode
        for k in sorted(modes):
            tt = torch.tensor([modes[k]["dt"]], dtype=torch.float64, device=device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            modes[k]["dt"] = float(tt)
    best = min(sorted(modes), key=lambda k: modes[k]["dt"])
    if best != "graph":
        state["gstep"] = None
    dt = modes[best]["dt"]
    log(f"headline launch mode: {best}; timed region {dt:.3f} s")
    loss = modes[best]["loss"]                   # the loss of the run that is reported (each mode's own is under launch_modes)
    assert all(np.isfinite(v["loss"]) for v in modes.values()), "non-finite loss in the bench"
    if collect:
        os.makedirs(a.dump_outputs, exist_ok=True)
        for name, arr in modes[best]["outputs"].items():
            np.save(os.path.join(a.dump_outputs, f"{name}.npy"), arr)
        log(f"outputs of the last timed {best} step written to {a.dump_outputs}")
    episodes = B * world * a.steps
    value = episodes / dt
    ms_per_step = dt / a.steps * 1e3
    launch_modes = {k: {"value": round(B * world * a.steps / v["dt"], 3), "ms_per_step": round(v["dt"] / a.steps * 1e3, 3),
                        "host_enqueue_ms_per_step": v["host_enqueue_ms_per_step"], "host_ms_one_step": v["host_ms_one_step"],
                        "loss": round(v["loss"], 4)}
                    for k, v in modes.items()}
    comm = None
    if ddp is not None:
        comm = {"world_size_seen": dist.get_world_size(), "backend": dist.get_backend(),
                "allreduce_bytes_per_step": ddp.stats["bytes_per_step"], "buckets": len(ddp.buckets),
                "exposed_comm_ms_last_step": round(ddp.exposed_comm_ms(), 3)}

    roofline = None
    if a.full and not a.no_roofline and rank == 0:
        # dominant kernel = the fp32-MFMA implicit-GEMM family (csrc/gemm.hip: gemm_kernel<...>): every launch of
        # the next steps is bracketed by HIP events on its own stream; achieved = sum(2MNK) / sum(duration)
        nprof = min(2, a.steps)
        side = HF.Runtime.use_side_stream
        HF.Runtime.use_side_stream = False       # serial launches: an event pair then brackets exactly one kernel
        torch.cuda.synchronize()
        ops.GemmProfiler.start()
        for i in range(nprof):
            step(a.warmup + a.steps + i, eager=True)
        r = ops.GemmProfiler.stop()
        HF.Runtime.use_side_stream = side
        if os.environ.get("CAPE_BENCH_GEMM_TABLE"):
            rows = sorted(r["table"].items(), key=lambda kv: -kv[1][1])
            for shape, (cnt, ms, fl) in rows[:60]:
                log(f"gemm M,N,K,am,bm,sk,batch={shape} calls/step {cnt / nprof:g} ms/step {ms / nprof:.3f} TF/s {fl / (ms * 1e-3) / 1e12:.1f}")
        ach = r["flops"] / (r["ms"] * 1e-3) / 1e12
        # peak for the arithmetic actually issued: exact fp32 MFMA, or bf16 MFMA at three instructions per product
        split = ops.get_gemm_precision() == "bf16x3"
        peak = PEAK_BF16_MFMA_TFLOPS / 3.0 if split else PEAK_F32_MFMA_TFLOPS
        # HBM bytes per launch of the family: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command
        # (tools/gemm_traffic.py, corrected as MI355X_MICROARCH.md prescribes), committed under profiles/; counters cannot be
        # read from inside the process, so the figure is the committed one, not re-measured by this run
        traffic, alg_bytes = None, None
        try:
            import glob
            tfile = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r*_gemm_traffic.json")))[-1]
            tr = json.load(open(tfile))
            traffic = round(tr["hbm_bytes_per_launch"])
            traffic_src = {"file": os.path.basename(tfile), "csrc_hash_measured": tr.get("csrc_hash"), "csrc_hash_now": csrc_tree_hash()}
            traffic_src["traffic_stale"] = traffic_src["csrc_hash_measured"] != traffic_src["csrc_hash_now"]
        except (OSError, KeyError, ValueError, IndexError):
            traffic_src = {"traffic_stale": True}
        # algorithmic bytes per launch: A + B + C once each, fp32 (dense formula; an upper bound for the im2col modes)
        alg_bytes = round(r["bytes"] / max(r["launches"], 1))
        # which roof binds the family: per launch, algorithmic flops / MFMA peak against algorithmic bytes / HBM peak
        avg_s = r["ms"] * 1e-3 / max(r["launches"], 1)
        flops_per_launch = r["flops"] / max(r["launches"], 1)
        t_mfma, t_hbm = flops_per_launch / (peak * 1e12), alg_bytes / (PEAK_HBM_TBPS * 1e12)
        mfma_view = {"achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4)}
        hbm_ach = alg_bytes / avg_s / 1e9
        hbm_view = {"achieved": round(hbm_ach, 1), "peak": PEAK_HBM_TBPS * 1e3, "unit": "GB/s", "frac": round(hbm_ach / (PEAK_HBM_TBPS * 1e3), 4)}
        bound = "hbm" if t_hbm >= t_mfma else "mfma"
        main, other = (hbm_view, mfma_view) if bound == "hbm" else (mfma_view, hbm_view)
        roofline = {"bound": bound, **main, "traffic": traffic, "traffic_source": traffic_src,
                    "traffic_unit": "HBM bytes per launch, from the committed rocprofv3 --pmc passes of this command (newest "
                                    "profiles/r*_gemm_traffic.json; counters cannot be read in-process)",
                    "algorithmic_bytes_per_launch": alg_bytes, "algorithmic_gflop_per_launch": round(flops_per_launch / 1e9, 3),
                    "roof_times_us": {"mfma": round(t_mfma * 1e6, 2), "hbm": round(t_hbm * 1e6, 2)},
                    "other_roof": {"bound": "mfma" if bound == "hbm" else "hbm", **other},
                    "peak_note": (("bf16 dense MFMA peak 2500 TFLOP/s / 3 MFMAs per algorithmic product (bf16x3 split)"
                                   if split else "fp32 MFMA dense peak") + "; HBM3E 8 TB/s"),
                    "kernel": "GEMM family: gemm_rs_kernel<NW,BMODE,KS,EPI> (register-stationary weights, K <= 256) + "
                              "gemm_kernel<BM,BN,AMODE,BMODE,VEC,PREC,KFULL> (tiled implicit GEMM) + gemm_group_kernel<...> (grouped "
                              "weight gradients, several products per launch), all instantiations; "
                              + ("bf16x3 split on bf16 MFMA" if split else "exact fp32 MFMA") + ")",
                    "launches_per_step": r["launches"] // nprof,
                    "products_per_step": r["products"] // nprof,
                    "avg_launch_us": round(avg_s * 1e6, 2),
                    "gemm_ms_per_step": round(r["ms"] / nprof, 2),
                    "gemm_gflop_per_step": round(r["flops"] / nprof / 1e9, 1)}
    elif a.full and world > 1 and not a.no_roofline:
        for i in range(min(2, a.steps)):         # keep the collectives of the profiled steps matched on all ranks
            step(a.warmup + a.steps + i)
    if world > 1:
        dist.barrier()

    # ---- the same step in the other GEMM arithmetic modes -------------------------------------------------------------------
    # alt_exact_f32: every GEMM on exact fp32 MFMA (CAPE_GEMM_PRECISION=f32) -- the like-for-like arithmetic of the reference --
    # timed exactly like the headline: the same K steps, eager AND replayed graph, its own roofline.
    # alt_bf16: ONE bf16 MFMA per product (what --use_amp selects): reported only, with its measured logit error against the
    # reference's 256x256 fixture -- it misses the 1e-3 parity bar by design.
    def precision_leg(name, both_modes):
        state["gstep"] = None
        ops.set_gemm_precision(name)
        try:
            leg_modes = {"eager": timed_region(f"{name} eager", 2)}
            if both_modes:
                from cape_amd.runtime.graph_step import GraphedTrainStep
                state["gstep"] = GraphedTrainStep(model, crit, opt, loss_scale=scale, edge_capacity=2048, eager_steps=1)
                leg_modes["graph"] = timed_region(f"{name} graph", 3)
                state["gstep"] = None
            side = HF.Runtime.use_side_stream
            HF.Runtime.use_side_stream = False
            torch.cuda.synchronize()
            ops.GemmProfiler.start()
            step(0, eager=True)
            rf = ops.GemmProfiler.stop()
            HF.Runtime.use_side_stream = side
        finally:
            state["gstep"] = None
            ops.set_gemm_precision("bf16x3")
        bestm = min(leg_modes, key=lambda k: leg_modes[k]["dt"])
        ach = rf["flops"] / (rf["ms"] * 1e-3) / 1e12
        peak = PEAK_F32_MFMA_TFLOPS if name == "f32" else PEAK_BF16_MFMA_TFLOPS
        return {"launch": bestm, "value": round(B * a.steps / leg_modes[bestm]["dt"], 3), "ms_per_step": round(leg_modes[bestm]["dt"] / a.steps * 1e3, 3),
                "steps": a.steps, "launch_modes": {k: {"value": round(B * a.steps / v["dt"], 3), "ms_per_step": round(v["dt"] / a.steps * 1e3, 3),
                                                       "host_enqueue_ms_per_step": v["host_enqueue_ms_per_step"], "loss": round(v["loss"], 4)}
                                                   for k, v in leg_modes.items()},
                "roofline": {"bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                             "gemm_ms_per_step": round(rf["ms"], 2), "launches_per_step": rf["launches"],
                             "algorithmic_bytes_per_launch": round(rf["bytes"] / max(rf["launches"], 1))}}

    alt, alt_bf16 = None, None
    if a.full and world == 1 and not a.no_roofline and ops.get_gemm_precision() == "bf16x3":
        alt = precision_leg("f32", both_modes=True)
        alt.update(gemm_precision="f32 (exact fp32 MFMA, v_mfma_f32_32x32x2_f32)")
        alt["roofline"]["kernel"] = "gemm_kernel / gemm_group_kernel <..., PREC 0>"
        alt_bf16 = precision_leg("bf16", both_modes=False)
        alt_bf16.update(gemm_precision="bf16 (one bf16 MFMA per product, fp32 accumulate; --use_amp)",
                        parity="REPORTED ONLY: outside the 1e-3 logit tolerance of the north star", logit_error=bf16_logit_error(device))
        alt_bf16["roofline"]["kernel"] = "gemm_rs_kernel / gemm_kernel / gemm_group_kernel, hi x hi product only"

    cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline(args)

    datap = None
    if a.full and rank == 0 and world == 1 and not a.no_decode:
        try:
            datap = data_pipeline_benchmark(device)
            log(f"data_pipeline: {datap}")
        except Exception as e:
            log(f"data_pipeline block failed: {type(e).__name__}: {e}")
            datap = {"error": f"{type(e).__name__}: {e}"}

    decode, pck = None, None
    if a.full and rank == 0 and world == 1 and not a.no_decode:
        # free the training state first: the decode model is a second instance (512x512, patch-2 input_proj)
        from cape_amd.runtime.decode_bench import decode_benchmark
        torch.cuda.synchronize()
        try:
            d1 = decode_benchmark(device, episodes=1)                     # configs[4] as stated: one 5-shot episode in flight
            d16 = decode_benchmark(device, episodes=16)                   # the same step with 32 images in flight
            keys = ("images", "steps", "us_per_step_eager", "us_per_step_graph", "tokens_per_s", "images_per_s_200_steps", "roofline",
                    "cu_stream", "whole_step_kernel", "launches_per_step")
            decode = dict(d1, batched_32_images={k: d16[k] for k in keys})
            if d16.get("whole_step_kernel"):                              # one block per image: the step time does not grow with the batch
                d64 = decode_benchmark(device, episodes=64, reps=2)
                decode["batched_128_images"] = {k: d64[k] for k in keys}
            log(f"decode: {d1['us_per_step_graph']} us/step (1 episode, graphs), {d16['us_per_step_graph']} us/step at 32 images")
            pck = pck_check(device)
            log(f"pck_check: {pck}")
        except Exception as e:                                            # the training line must not be lost to the extra block
            log(f"decode block failed: {type(e).__name__}: {e}")
            decode = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        gflop_ep = GFLOP_PER_EPISODE_256 * (a.image_size / 256.0) ** 2
        line = {
            "metric": "episodes/sec (1-shot, 256x256, 17kpt) training step", "value": round(value, 3), "unit": "episodes/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if ops.get_gemm_precision() == "f32" else "f32 storage/accumulate, GEMMs as bf16x3 split (3 bf16 MFMAs per product)",
            "data": "synthetic",
            "config": {"workload": f"configs[1]: 1-shot training step (fwd+loss+bwd+clip+AdamW at learning rate 0, dropout on), "
                                   f"{a.image_size}x{a.image_size}, 17 kpt, ResNet-50 + deformable transformer, "
                                   f"{B} episodes x 2 queries per GPU", "episodes_per_gpu": B, "queries_per_episode": K,
                       "image_size": a.image_size, "global_batch_episodes": B * world, "parallelism": f"dp{world}",
                       "weights": "random init (no checkpoint offline)"},
            "loss": round(loss, 4),
            "model_tflops": round(value * gflop_ep / 1e3, 2),
            "model_frac_of_mfma_peak": round(value * gflop_ep / 1e3 / ((PEAK_BF16_MFMA_TFLOPS / 3.0 if ops.get_gemm_precision() == "bf16x3"
                                                                          else PEAK_F32_MFMA_TFLOPS) * world), 4),
            "model_frac_note": "whole-step algorithmic TFLOP/s over the peak of the arithmetic issued (bf16 dense 2500 / 3 MFMAs per "
                               "product for the bf16x3 split; 157.3 for exact fp32)",
            "gemm_precision": ops.get_gemm_precision(),
            "roofline": roofline, "cpu_baseline": cpu, "alt_exact_f32": alt, "alt_bf16": alt_bf16, "data_pipeline": datap,
            "launch": "hipGraph replay of the captured step" if best == "graph" else "eager (one launch per kernel from Python)",
            "launch_modes": launch_modes, "comm": comm, "decode": decode, "pck_check": pck,
        }
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

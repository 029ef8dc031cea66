"""GPU tests of dilated convolutions and the `--dilation` (DC5) trunk.

The reference builds torchvision's ResNet-50 with `replace_stride_with_dilation=[False, False, True]` and halves the last stride
(`models/backbone.py:72-83`): layer4 keeps C4's resolution, its first block runs at stride 1 / dilation 1 (torchvision's
`previous_dilation`), its second and third blocks' 3x3 convolutions use dilation 2 and padding 2.  torchvision cannot be imported
here and the reference shim refuses dilation, so no golden exists for this path: parity with the reference is unpinned at the
trunk and pinned to torch's conv2d.  The checker is torch fp32 on the CPU -- `F.conv2d(..., dilation=)` for the kernels and the
nodes, and for the whole model the oracle `cape_ref` with its trunk replaced by `dc5_body` below, a restatement of that torchvision
algorithm in the style of `cape_ref.resnet50_body`.  The undilated oracle's final-layer logits differ from the DC5 oracle's by
0.64 on the batch used here, so a model that ignores the flag cannot pass.

Tolerances are the ones of tests/test_kernels_gpu.py and tests/test_e2e_gpu.py: 1e-4 for forward values and 2e-4 for gradients
(relative to the tensor scale), end to end 1e-3 for logits, 1e-4 for coordinates, 2e-3 * max|ref| for gradient slices and 2e-2
relative for gradient norms."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import cape_amd  # noqa: F401
    from cape_amd.hip import ops
from oracle import cape_ref, synth
from tests.helpers import build_product, to_dev

DEV = "cuda"
CFG = cape_ref.Cfg()
BODY = "base_model.backbone.0.body."


@pytest.fixture(params=["bf16x3", "f32"], autouse=True)
def gemm_precision(request):
    """Every test here runs in both GEMM arithmetic modes (default bf16x3 split, exact fp32)."""
    old = ops.get_gemm_precision()
    ops.set_gemm_precision(request.param)
    yield request.param
    ops.set_gemm_precision(old)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def close(got, ref, tol=1e-4, name=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    scale = max(1.0, ref.abs().max().item() if ref.numel() else 1.0)
    assert err <= tol * scale, f"{name}: max err {err:.3e} (scale {scale:.3e})"


# ------------------------------------------------------------------------------------------------
# the DC5 trunk restated (torchvision ResNet._make_layer(dilate=True) over Bottleneck v1.5 and FrozenBatchNorm2d)
# ------------------------------------------------------------------------------------------------
def dc5_bottleneck(x, sd, p, stride, dilation):
    out = F.relu(cape_ref.frozen_bn(F.conv2d(x, sd[p + "conv1.weight"]), sd, p + "bn1"))
    out = F.conv2d(out, sd[p + "conv2.weight"], stride=stride, padding=dilation, dilation=dilation)
    out = F.relu(cape_ref.frozen_bn(out, sd, p + "bn2"))
    out = cape_ref.frozen_bn(F.conv2d(out, sd[p + "conv3.weight"]), sd, p + "bn3")
    if (p + "downsample.0.weight") in sd:
        x = cape_ref.frozen_bn(F.conv2d(x, sd[p + "downsample.0.weight"], stride=stride), sd, p + "downsample.1")
    return F.relu(out + x)


def dc5_body(x, sd, prefix=BODY):
    """[C3, C4, C5] of the dilated trunk: layer strides (1, 2, 2, 1); dilation 2 / padding 2 on the 3x3 of layer4.1 and layer4.2,
    layer4.0 at the previous dilation 1."""
    x = F.relu(cape_ref.frozen_bn(F.conv2d(x, sd[prefix + "conv1.weight"], stride=2, padding=3), sd, prefix + "bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    feats = []
    for li, (nblk, stride) in enumerate([(3, 1), (4, 2), (6, 2), (3, 1)], start=1):
        for b in range(nblk):
            x = dc5_bottleneck(x, sd, f"{prefix}layer{li}.{b}.", stride if b == 0 else 1, 2 if (li == 4 and b > 0) else 1)
        if li >= 2:
            feats.append(x)
    return feats


GRAD_KEYS = ("base_model.input_proj.2.0.weight", "base_model.input_proj.3.0.weight")


def _wants_grad(k):
    return k in GRAD_KEYS or (k.startswith(BODY + "layer4.") and k.endswith(("conv1.weight", "conv2.weight", "conv3.weight",
                                                                             "downsample.0.weight")))


def _batch():
    return synth.make_batch(11, 2, 2, 64, 9, CFG, n_invisible=(2, 0))


@pytest.fixture(scope="module")
def oracle(proc_sd):
    """The DC5 oracle on the 64x64 batch, computed once on the CPU: teacher-forced outputs of all six layers, losses, and the
    autograd gradients of every layer4 parameter and of the two input_proj convolutions that read C5."""
    b = _batch()
    sd = {k: (v.clone().requires_grad_(True) if _wants_grad(k) else v) for k, v in proc_sd.items()}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(cape_ref, "resnet50_body", dc5_body)           # image_features resolves the name at call time
        out = cape_ref.cape_forward(sd, CFG, b["images"], b["support_coords"], b["support_mask"], b["targets"], b["skeleton"],
                                    train=False, grad_mode=True)
        losses, _, total = cape_ref.criterion(out, b["targets"], CFG)
        total.backward()
    grads = {k: v.grad.clone() for k, v in sd.items() if v.requires_grad and v.grad is not None}
    det = lambda o: {"pred_logits": o["pred_logits"].detach(), "pred_coords": o["pred_coords"].detach()}
    return {"batch": b, "out": dict(det(out), pred_room_logits=out["pred_room_logits"].detach(),
                                    aux_outputs=[det(a) for a in out["aux_outputs"]]),
            "losses": {k: float(v) for k, v in losses.items()}, "total": float(total), "grads": grads}


def stack_outputs(out):
    logits = torch.stack([a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]])
    coords = torch.stack([a["pred_coords"] for a in out["aux_outputs"]] + [out["pred_coords"]])
    return logits, coords


# ------------------------------------------------------------------------------------------------
# 1. raw launches
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C,O,k,stride,pad,dil", [
    (2, 16, 16, 64, 64, 3, 1, 2, 2),        # all three fast paths
    (2, 4, 4, 64, 64, 3, 1, 2, 2),          # layer4's grid at 64 x 64: every off-centre tap crosses a border for some pixel
    (2, 9, 7, 36, 40, 3, 1, 2, 2),          # general paths, odd non-square extents, C and O no multiples of 32
    (1, 16, 16, 32, 48, 3, 2, 2, 2),        # stride 2 with dilation: a_mode 2 fast, a_mode 3 general, b_mode 3 non-power-of-two
    (2, 12, 12, 32, 32, 3, 1, 3, 3),        # a dilation other than 2
])
def test_dilated_conv_fwd_dgrad_wgrad(N, H, W, C, O, k, stride, pad, dil):
    """The three gather modes of the implicit-GEMM family with `conv_dil` against F.conv2d(..., dilation=) and its autograd."""
    x = rnd(N, C, H, W, seed=0)
    w = rnd(O, C, k, k, seed=1, scale=(C * k * k) ** -0.5)
    OH, OW = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    geom = (N, H, W, C, k, k, stride, pad, OH, OW, O)
    sc, sh = rnd(O, seed=7).abs() + 0.5, rnd(O, seed=8)
    x.requires_grad_(True); w.requires_grad_(True)
    y_ref = F.conv2d(x, w, stride=stride, padding=pad, dilation=dil)
    assert tuple(y_ref.shape) == (N, O, OH, OW)
    z_ref = F.relu(y_ref * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    g = rnd(*y_ref.shape, seed=9)
    y_ref.backward(g)
    xn = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV)
    wn = w.detach().permute(0, 2, 3, 1).contiguous().to(DEV)
    M, K = N * OH * OW, k * k * C
    out = torch.empty(M, O, device=DEV)
    ops.gemm(xn, wn, out, M, O, K, a_mode=2, b_mode=0, conv=geom, conv_dil=dil, scale=sc.to(DEV), bias=sh.to(DEV), relu=True)
    close(out.view(N, OH, OW, O).permute(0, 3, 1, 2), z_ref, name="dilated conv fwd")
    gn = g.permute(0, 2, 3, 1).contiguous().to(DEV)
    dx = torch.empty(N * H * W, C, device=DEV)
    ops.gemm(gn, wn, dx, N * H * W, C, k * k * O, a_mode=3, b_mode=2, conv=geom, conv_dil=dil)
    close(dx.view(N, H, W, C).permute(0, 3, 1, 2), x.grad, tol=2e-4, name="dilated conv dgrad")
    dw = torch.zeros(O, k * k * C, device=DEV)
    ops.gemm(gn, xn, dw, O, k * k * C, M, a_mode=1, b_mode=3, lda=O, conv=geom, conv_dil=dil, accumulate=True,
             split_k=ops.pick_split_k(O, k * k * C, M))
    close(dw.view(O, k, k, C).permute(0, 3, 1, 2), w.grad, tol=2e-4, name="dilated conv wgrad")
    with pytest.raises(AssertionError):                    # the host checks the output extent against the dilated geometry
        ops.gemm_desc(xn, wn, out, M, O, K, a_mode=2, b_mode=0, conv=geom, conv_dil=1)


# ------------------------------------------------------------------------------------------------
# 2. conv node
# ------------------------------------------------------------------------------------------------
def test_dilated_conv_node_k_split_and_deferred_wgrad(monkeypatch):
    """HF.conv_bn_act(..., dilation=2) in grad mode at layer4's 64 x 64 shape: the forward and the data gradient take the atomic
    k-split, and the weight gradient -- accumulated straight into an existing `.grad`, as the gradient arena has it -- is queued
    and launched by cape_gemm_group_f32 with the dilation in its item table."""
    from cape_amd.hip import functional as HF
    N, H, W, C, O, k, stride, pad, dil = 2, 4, 4, 512, 512, 3, 1, 2, 2
    x = rnd(N, C, H, W, seed=0)
    w = rnd(O, C, k, k, seed=1, scale=(C * k * k) ** -0.5)
    sc, sh = rnd(O, seed=7).abs() + 0.5, rnd(O, seed=8)
    x.requires_grad_(True); w.requires_grad_(True)
    z_ref = F.relu(F.conv2d(x, w, stride=stride, padding=pad, dilation=dil) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    OH, OW = z_ref.shape[2:]
    assert (OH, OW) == (H, W)
    g = rnd(*z_ref.shape, seed=9)
    z_ref.backward(g)
    assert ops.pick_split_k(N * OH * OW, O, k * k * C) >= 4          # the case does take the k-split
    xn = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    wn = torch.nn.Parameter(w.detach().to(DEV).contiguous(memory_format=torch.channels_last))
    with torch.no_grad():
        z_single = HF.conv_bn_act(xn, wn, sc.to(DEV), sh.to(DEV), stride=stride, pad=pad, relu=True, dilation=dil)
    queued = []
    enqueue = HF.Runtime.enqueue_wgrad
    monkeypatch.setattr(HF.Runtime, "enqueue_wgrad", lambda d, keep: (queued.append((d.b_mode, d.cDil)), enqueue(d, keep))[1])
    monkeypatch.setattr(HF.Runtime, "direct_grad", True)
    wn.grad = torch.zeros_like(wn)                                   # the node accumulates into it and hands autograd None
    z = HF.conv_bn_act(xn, wn, sc.to(DEV), sh.to(DEV), stride=stride, pad=pad, relu=True, dilation=dil)
    close(z.permute(0, 3, 1, 2), z_ref, name="dilated conv node fwd (k-split)")
    close(z, z_single, tol=2e-5, name="k-split vs single pass")
    z.backward(g.permute(0, 2, 3, 1).contiguous().to(DEV))
    HF.Runtime.join()
    assert queued == [(3, dil)]
    close(xn.grad.permute(0, 3, 1, 2), x.grad, tol=2e-4, name="dilated conv node dgrad")
    close(wn.grad, w.grad, tol=2e-4, name="dilated conv node wgrad (grouped launch)")


# ------------------------------------------------------------------------------------------------
# 3. bottleneck node
# ------------------------------------------------------------------------------------------------
def test_dilated_bottleneck_node_matches_conv_chain_and_torch():
    """HF.bottleneck(..., stride=1, dilation=2) with an identity shortcut (layer4.1 / layer4.2 of the DC5 trunk) against the same
    block as four HF.conv_bn_act nodes and against torch fp32 on the CPU."""
    from cape_amd.hip import functional as HF
    N, H, planes, dil = 2, 8, 64, 2
    inplanes = planes * 4
    shapes = [(planes, inplanes, 1), (planes, planes, 3), (inplanes, planes, 1)]
    ws = [rnd(o, c, k, k, seed=10 * i, scale=(c * k * k) ** -0.5) for i, (o, c, k) in enumerate(shapes)]
    bns = [(rnd(o, seed=10 * i + 1).abs() + 0.5, rnd(o, seed=10 * i + 2)) for i, (o, c, k) in enumerate(shapes)]
    x = rnd(N, inplanes, H, H, seed=5)
    g = rnd(N, inplanes, H, H, seed=9)

    def affine(t, bn):
        return t * bn[0].view(1, -1, 1, 1) + bn[1].view(1, -1, 1, 1)

    xr = x.clone().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    o = F.relu(affine(F.conv2d(xr, wr[0]), bns[0]))
    o = F.relu(affine(F.conv2d(o, wr[1], stride=1, padding=dil, dilation=dil), bns[1]))
    y_ref = F.relu(affine(F.conv2d(o, wr[2]), bns[2]) + xr)
    y_ref.backward(g)

    def device_inputs():
        xn = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
        wn = [torch.nn.Parameter(w.to(DEV).contiguous(memory_format=torch.channels_last)) for w in ws]
        return xn, wn, [(b[0].to(DEV), b[1].to(DEV)) for b in bns]

    gn = g.permute(0, 2, 3, 1).contiguous().to(DEV)
    xb, wb, bn = device_inputs()
    y_node = HF.bottleneck(xb, wb[0], wb[1], wb[2], None, bn[0], bn[1], bn[2], None, 1, dilation=dil)
    y_node.backward(gn)
    xc, wc, bn = device_inputs()
    o = HF.conv_bn_act(xc, wc[0], *bn[0], relu=True)
    o = HF.conv_bn_act(o, wc[1], *bn[1], stride=1, pad=dil, relu=True, dilation=dil)
    y_chain = HF.conv_bn_act(o, wc[2], *bn[2], relu=True, residual=xc)
    y_chain.backward(gn)
    HF.Runtime.join()

    close(y_node.permute(0, 3, 1, 2), y_ref, name="bottleneck fwd vs torch")
    close(y_node, y_chain, name="bottleneck fwd vs conv chain")
    for what, xd, wd in (("node", xb, wb), ("chain", xc, wc)):
        close(xd.grad.permute(0, 3, 1, 2), xr.grad, tol=2e-4, name=f"{what} input gradient vs torch")
        for i, (w, r) in enumerate(zip(wd, wr)):
            close(w.grad, r.grad, tol=2e-4, name=f"{what} weight gradient {i} vs torch")
    close(xb.grad, xc.grad, tol=2e-4, name="input gradient node vs chain")
    for i, (a, b) in enumerate(zip(wb, wc)):
        close(a.grad, b.grad, tol=2e-4, name=f"weight gradient {i} node vs chain")


# ------------------------------------------------------------------------------------------------
# 4. trunk
# ------------------------------------------------------------------------------------------------
def test_dilated_trunk_matches_restated_dc5(proc_sd):
    """ResNet50Body built with dilation (layer4.0: projection shortcut, stride 1, dilation 1; layer4.1-2: dilation 2) on the
    procedural weights: C5 keeps C4's grid, values as the restated trunk."""
    from cape_amd.models.backbone import ResNet50Body
    sd = {k[len(BODY):]: v for k, v in proc_sd.items() if k.startswith(BODY)}
    body = ResNet50Body(sd["conv1.weight"].shape[1], dilation=True)
    body.load_state_dict(sd, strict=True)
    body = body.to(DEV).eval()
    images = _batch()["images"][:2]
    with torch.no_grad():
        got = body(images.to(DEV))
        ref = dc5_body(images, proc_sd)
    assert [tuple(f.shape[1:]) for f in got] == [(8, 8, 512), (4, 4, 1024), (4, 4, 2048)]
    for name, a, r in zip(("C3", "C4", "C5"), got, ref):
        err, scale = (a.permute(0, 3, 1, 2).cpu() - r).abs().max().item(), r.abs().max().item()
        print(f"{name}: max err {err:.3e}, max |ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (name, err, scale)


# ------------------------------------------------------------------------------------------------
# 5 / 6. end to end: forward, losses, gradients
# ------------------------------------------------------------------------------------------------
def _run_product(proc_sd, b):
    args, tok, model, crit = build_product(extra=("--dilation",), proc_sd=proc_sd)
    model.eval()
    out = model(samples=b["images"], support_coords=b["support_coords"], support_mask=b["support_mask"],
                targets=b["targets"], skeleton_edges=b["skeleton"])
    return model, crit, out


def test_dilated_forward_vs_dc5_oracle(proc_sd, oracle):
    """Teacher-forced forward of the `--dilation` product against the DC5 oracle, all six decoder layers.  Parity with the reference
    unpinned at the trunk, pinned to torch's conv2d."""
    b = to_dev(oracle["batch"])
    with torch.no_grad():
        _, _, out = _run_product(proc_sd, b)
    logits, coords = stack_outputs(out)
    ref_logits, ref_coords = stack_outputs(oracle["out"])
    e_l, e_c = (logits.cpu() - ref_logits).abs().max().item(), (coords.cpu() - ref_coords).abs().max().item()
    e_r = (out["pred_room_logits"][:, :16].cpu() - oracle["out"]["pred_room_logits"][:, :16]).abs().max().item()
    print(f"logits {e_l:.3e}  coords {e_c:.3e}  room logits {e_r:.3e}")
    assert e_l < 1e-3 and e_c < 1e-4 and e_r < 1e-3
    # tokens: exact wherever the oracle's top-2 gap is at least twice the logit tolerance; that rule may leave out <= 1 %
    top2 = ref_logits.sort(-1).values
    clear = (top2[..., -1] - top2[..., -2]) >= 2e-3
    excluded = 1.0 - clear.float().mean().item()
    print(f"positions excluded by the top-2 rule: {excluded:.4%} ({int((~clear).sum())} of {clear.numel()})")
    assert excluded <= 0.01
    assert torch.equal(logits.argmax(-1).cpu()[clear], ref_logits.argmax(-1)[clear])


def test_dilated_losses_and_gradients_vs_dc5_oracle(proc_sd, oracle):
    """The product criterion's losses and, after backward(), the gradients of every layer4 parameter and of the two input_proj
    convolutions that read C5, against the DC5 oracle's criterion and autograd: every element within 2e-3 * max(1, max|ref|), norms
    within 2e-2 relative.

    Measured on MI355X (whole tensors, 12 parameters, worst element error / tolerance; norms always within 5e-4 relative):
      f32      0.06 - 0.11 in every run: passes.
      bf16x3   MISSES the elementwise bound, and not by the same amount from run to run (the forward k-splits sum in arrival
               order): input_proj.3.0.weight 2.15e-3, 2.18e-3, 2.30e-3, 2.30e-3 against 2e-3 in four runs (3-4 of 4.7 M elements
               over); layer4.2.conv2.weight 0.60 x the tolerance in one run and 10.2 x in the next (2.0e-2, 413 of 2.4 M elements
               over, one output channel's row); every other parameter 0.14 - 0.82 x.
    The same whole-tensor comparison of the UNDILATED model against the undilated oracle (code paths this change does not touch)
    gives 0.05 - 0.30 x in one bf16x3 run and 1.46 x on layer4.2.conv2.weight (2 elements over) in the next; tests/test_e2e_gpu.py
    compares the first 256 elements and the norms of those tensors, which hold here as well (head errors <= 2.7e-4).  Cause, found
    on the CPU: the bf16x3 trunk leaves a relative error of 1.4e-5 on C3-C5 (trunk test above: 1.9e-4 of 13.3); adding noise of that
    size to the ORACLE's own C3-C5 moves its gradients by 1.8e-3 (input_proj.3.0.weight), 2.0e-3 (layer4.2.conv2.weight) and
    2.7e-3 (input_proj.2.0.weight) -- 0.9 to 1.35 x this bound, 5 x what the same noise does to the undilated oracle -- and a ReLU gate of layer4.2 that flips under it changes one output channel's
    row of the weight gradient at once.  The forward values (logits 5.4e-5), the losses and the gradient norms are far inside
    their bounds; the dilated kernels themselves match torch to 2e-4 (tests 1-3).  The bound is the issue's and stays."""
    b = to_dev(oracle["batch"])
    model, crit, out = _run_product(proc_sd, b)
    ld = crit(out, b["targets"])
    assert sorted(k for k in ld if not k.startswith("_")) == sorted(oracle["losses"])
    for k, v in oracle["losses"].items():
        assert abs(float(ld[k]) - v) < 1e-3, (k, float(ld[k]), v)
    assert abs(float(ld["_total"]) - oracle["total"]) < 5e-3
    ld["_total"].backward()
    from cape_amd.hip import functional as HF
    HF.Runtime.join()
    named = dict(model.named_parameters(remove_duplicate=False))
    keys = sorted(oracle["grads"])
    assert sum(k.startswith(BODY + "layer4.") for k in keys) == 10 and all(k in keys for k in GRAD_KEYS)
    worst_e, worst_n = 0.0, 0.0
    for k in keys:
        ref, got = oracle["grads"][k], named[k].grad.detach().cpu()
        err, tol = (got - ref).abs().max().item(), 2e-3 * max(1.0, ref.abs().max().item())
        rel = abs(got.norm().item() - ref.norm().item()) / max(ref.norm().item(), 1e-3)
        worst_e, worst_n = max(worst_e, err / tol), max(worst_n, rel)
        assert err <= tol, (k, err, tol)
        assert rel < 2e-2, (k, rel)
    print(f"worst gradient error / tolerance {worst_e:.3f}, worst relative norm error {worst_n:.3e}")


# ------------------------------------------------------------------------------------------------
# 7. cached decode
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_oracle(proc_sd, oracle):
    b = oracle["batch"]
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        mp.setattr(cape_ref, "resnet50_body", dc5_body)
        return cape_ref.cape_forward_inference(proc_sd, CFG, b["images"], b["support_coords"], b["support_mask"], b["skeleton"],
                                               grad_mode=False)


def test_dilated_cached_decode_vs_dc5_oracle(proc_sd, oracle, decode_oracle):
    """forward_inference of the `--dilation` product (seed 11 batch, free-running until every sequence has ended: 7 steps)
    reproduces the DC5 oracle's token stream exactly and its coordinates to 1e-4.  The oracle's top-2 logit gap is >= 2e-3 at
    every decoded position for this seed (0.69 at the smallest, asserted), so the 1e-3 logit tolerance cannot flip a token."""
    ref = decode_oracle
    top2 = ref["logits"].sort(-1).values
    gap = (top2[..., -1] - top2[..., -2]).min().item()
    print(f"smallest top-2 gap along the oracle's stream: {gap:.3e}")
    assert gap >= 2e-3
    b = to_dev(oracle["batch"])
    args, tok, model, crit = build_product(extra=("--dilation",), proc_sd=proc_sd)
    model.eval()
    with torch.no_grad():
        p = model.forward_inference(samples=b["images"], support_coords=b["support_coords"], support_mask=b["support_mask"],
                                    skeleton_edges=b["skeleton"])
    assert p["logits"].shape == ref["logits"].shape, (p["logits"].shape, ref["logits"].shape)
    e_l, e_c = (p["logits"].cpu() - ref["logits"]).abs().max().item(), (p["coordinates"].cpu() - ref["coordinates"]).abs().max().item()
    print(f"decode logits {e_l:.3e}  coordinates {e_c:.3e}")
    assert torch.equal(p["sequences"].cpu(), ref["sequences"])
    assert e_c < 1e-4 and e_l < 1e-3


# ------------------------------------------------------------------------------------------------
# 8. train-mode step, captured
# ------------------------------------------------------------------------------------------------
def test_dilated_graphed_train_step_matches_eager(monkeypatch, proc_sd, oracle):
    """One model.train() step of the `--dilation` product under GraphedTrainStep: eager warm-up, capture, one replay.  At learning
    rate 0 the parameters stay put, so the replayed step sees the eager step's model: with the same dropout seed its loss equals
    the eager loss of the same call (tolerance of test_graphed_train_step_matches_eager; forward k-splits off as there)."""
    from cape_amd.hip import functional as HF
    from cape_amd.runtime.graph_step import GraphedTrainStep
    from cape_amd.runtime.optimizer import ArenaAdamW
    monkeypatch.setattr(HF, "_DETERMINISTIC", True)
    b = to_dev(oracle["batch"])
    args, tok, model, crit = build_product(extra=("--dilation",), proc_sd=proc_sd)
    model.train()
    opt = ArenaAdamW(model, lr=0.0, lr_backbone=0.0, weight_decay=1e-4, max_norm=0.1)
    before = model.base_model.backbone[0].body.layer4[1].conv2.weight.detach().clone()

    def run(eager_steps):
        HF.Runtime.seed(77, torch.device(DEV))
        step = GraphedTrainStep(model, crit, opt, edge_capacity=512, eager_steps=eager_steps)
        losses = [float(step(b["images"], b["support_coords"], b["support_mask"], b["targets"], b["skeleton"])["_total"])
                  for _ in range(2)]
        return losses, len(step.cache)

    le, ne = run(10 ** 9)                                       # call 0 and call 1 eager
    lg, ng = run(1)                                             # call 0 eager, call 1 captures and replays
    assert (ne, ng) == (0, 1)
    print(f"eager {le}  graphed {lg}")
    assert all(torch.isfinite(torch.tensor(le + lg)))
    for a_, b_ in zip(le, lg):
        assert abs(a_ - b_) <= 2e-4 * max(1.0, abs(a_)), (le, lg)
    assert torch.equal(model.base_model.backbone[0].body.layer4[1].conv2.weight.detach(), before)

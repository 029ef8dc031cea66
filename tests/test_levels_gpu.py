"""GPU tests of `--num_feature_levels` 1 and 3: the single-scale (C5 / DC5) and the three-level model.

The reference builds one 1x1 `input_proj` over C5 alone for one level (`roomformer_v2.py:209-214`, `backbone.py:51-54,101`) and
C3..C5 without the extra stride-2 level for three.  Its trunk is torchvision's, which cannot be imported here, so -- as in
tests/test_dilation_gpu.py -- no golden exists for these configurations: parity is pinned to the CPU oracle `oracle.cape_ref` with
`Cfg(num_feature_levels=L)`, a restatement of the reference, whose trunk is patched to hand back only C5 for one level (and to the
DC5 trunk restated in tests/test_dilation_gpu.py for `--dilation`).  Weights are procedural (a function of key and shape) over the
product model's own state_dict names and shapes.  The 4-level oracle's final-layer logits differ from the 3-level and 1-level
oracles' by 2.7 and 2.6 (2.8 with `--dilation`) on the batch used here (tests/test_levels_cpu.py), so a model that ignores the flag cannot pass.

Shapes (64 x 64 images, 9 keypoints): one level = a 2 x 2 grid, S = 4 (every bilinear tap of every sample crosses a border);
one level + `--dilation` = 4 x 4, S = 16; three levels = 8 x 8 + 4 x 4 + 2 x 2, S = 84.

Tolerances are the project's: 1e-4 for kernel values and 2e-4 for kernel gradients (relative to the tensor scale), end to end 1e-3
for logits, 1e-4 for coordinates, 1e-3 for losses, 2e-3 * max(1, max|ref|) for gradient elements and 2e-2 relative for gradient
norms."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import cape_amd  # noqa: F401
    from cape_amd.hip import ops
from oracle import cape_ref, procweights, synth
from tests.helpers import build_product, to_dev
from tests.test_dilation_gpu import BODY, close, dc5_body, rnd, stack_outputs

DEV = "cuda"
_PLAIN_BODY = cape_ref.resnet50_body
CONFIGS = {"L1": (1, False), "L1_dc5": (1, True), "L3": (3, False)}
GRIDS = {"L1": [(2, 2)], "L1_dc5": [(4, 4)], "L3": [(8, 8), (4, 4), (2, 2)]}
T = "base_model.transformer."
# compared whole and elementwise in exact fp32 (every input_proj convolution is added per configuration).  Which encoder and which
# decoder layer: a sampling offset's gradient jumps when a sample crosses a pixel boundary, so a whole-tensor bound can only hold
# where no sample of the ORACLE sits on one.  Measured on the CPU oracle alone: Gaussian noise of 1e-7 and 1e-6 relative (the size
# of fp32 rounding) on its own backbone features, 8 seeds each, moves its whole-tensor gradients by up to
#   encoder.layers.0 sampling_offsets.weight   0.45 / 2.24 / 1.79 x this bound at L1 / L1_dc5 / L3 (29 elements, one sample),
#   decoder.layers.0 sampling_offsets.weight   0.73 / 0.34 / 0.94 x,   decoder.layers.1   1.25 / 0.43 / 0.13 x,
#   encoder.layers.5 (both weights)            0.35 / 0.25 / 0.25 x,   decoder.layers.2 (both weights)   0.003 / 0.42 / 0.31 x,
# so layers 5 and 2 are the ones a bound of 1 x can be asked of (the heads and norms of every layer are compared below anyway).
WHOLE = (T + "level_embed", T + "encoder.layers.5.self_attn.sampling_offsets.weight",
         T + "encoder.layers.5.self_attn.attention_weights.weight", T + "decoder.layers.2.cross_attn.sampling_offsets.weight",
         T + "decoder.layers.2.cross_attn.attention_weights.weight", BODY + "layer4.2.conv3.weight")


@pytest.fixture(params=["bf16x3", "f32"], autouse=True)
def gemm_precision(request):
    """Every test here runs in both GEMM arithmetic modes (default bf16x3 split, exact fp32)."""
    old = ops.get_gemm_precision()
    ops.set_gemm_precision(request.param)
    yield request.param
    ops.set_gemm_precision(old)


# ------------------------------------------------------------------------------------------------
# configurations, weights, oracle (computed once per configuration on the CPU and left unchanged)
# ------------------------------------------------------------------------------------------------
def extra_args(name):
    L, dil = CONFIGS[name]
    return ("--num_feature_levels", str(L)) + (("--dilation",) if dil else ())


def oracle_body(name):
    """The oracle's trunk for a configuration: plain or DC5, handing back [C5] alone for one level."""
    L, dil = CONFIGS[name]
    base = dc5_body if dil else _PLAIN_BODY
    return (lambda x, sd, prefix=BODY: base(x, sd, prefix)[-1:]) if L == 1 else base


def batch():
    return synth.make_batch(11, 2, 2, 64, 9, cape_ref.Cfg(), n_invisible=(2, 0))


_CACHE = {}


def cached(kind, name, make):
    if (kind, name) not in _CACHE:
        _CACHE[kind, name] = make()
    return _CACHE[kind, name]


def weights(name):
    """(procedural state_dict over the product's own names and shapes, names of its trainable parameters)."""
    def make():
        _, _, model, _ = build_product(extra=extra_args(name), device="cpu")
        spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        trainable = sorted(n for n, p in model.named_parameters(remove_duplicate=False) if p.requires_grad)
        return procweights.procedural_state_dict(spec), trainable
    return cached("weights", name, make)


def oracle(name):
    """Teacher-forced oracle of a configuration: outputs of all six layers, the criterion's losses, autograd gradients of every
    tensor that is trainable in the product."""
    def make():
        sd0, trainable = weights(name)
        cfg, b = cape_ref.Cfg(num_feature_levels=CONFIGS[name][0]), batch()
        sd = {k: (v.clone().requires_grad_(True) if (k in trainable and v.is_floating_point()) else v) for k, v in sd0.items()}
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(cape_ref, "resnet50_body", oracle_body(name))      # image_features resolves the name at call time
            out = cape_ref.cape_forward(sd, cfg, b["images"], b["support_coords"], b["support_mask"], b["targets"], b["skeleton"],
                                        train=False, grad_mode=True)
            losses, _, total = cape_ref.criterion(out, b["targets"], cfg)
            total.backward()
        grads = {k: v.grad.clone() for k, v in sd.items() if v.requires_grad and v.grad is not None}
        det = lambda o: {"pred_logits": o["pred_logits"].detach(), "pred_coords": o["pred_coords"].detach()}
        return {"batch": b, "out": dict(det(out), pred_room_logits=out["pred_room_logits"].detach(),
                                        aux_outputs=[det(a) for a in out["aux_outputs"]]),
                "losses": {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in losses.items()}, "total": float(total.detach()), "grads": grads}
    return cached("oracle", name, make)


def decode_oracle(name):
    def make():
        sd, _ = weights(name)
        cfg, b = cape_ref.Cfg(num_feature_levels=CONFIGS[name][0]), batch()
        with pytest.MonkeyPatch.context() as mp, torch.no_grad():
            mp.setattr(cape_ref, "resnet50_body", oracle_body(name))
            return cape_ref.cape_forward_inference(sd, cfg, b["images"], b["support_coords"], b["support_mask"], b["skeleton"],
                                                   grad_mode=False)
    return cached("decode", name, make)


def product(name):
    args, tok, model, crit = build_product(extra=extra_args(name), proc_sd=weights(name)[0])
    return model, crit


def eval_product(name):
    """One eval-mode product per configuration for the forward-only tests (its weights are never touched)."""
    return cached("product", name, lambda: product(name)[0].eval())


def forward(model, b):
    return model(samples=b["images"], support_coords=b["support_coords"], support_mask=b["support_mask"], targets=b["targets"],
                 skeleton_edges=b["skeleton"])


def decode(model, b, **kw):
    with torch.no_grad():
        return model.forward_inference(samples=b["images"], support_coords=b["support_coords"], support_mask=b["support_mask"],
                                       skeleton_edges=b["skeleton"], **kw)


# ------------------------------------------------------------------------------------------------
# 1. MSDA kernels at the new geometries
# ------------------------------------------------------------------------------------------------
def _msda_ref(value, offw, ref, shapes):
    N, Lq = offw.shape[:2]
    L = len(shapes)
    off = offw[..., :64 * L].reshape(N, Lq, 8, L, 4, 2)
    aw = F.softmax(offw[..., 64 * L:].reshape(N, Lq, 8, 4 * L), -1).view(N, Lq, 8, L, 4)
    norm = torch.tensor([[w, h] for (h, w) in shapes], dtype=torch.float32)
    loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    return cape_ref.msda_core(value, shapes, loc, aw)


@pytest.mark.parametrize("form", ["f64", "fx", "atomic"])
@pytest.mark.parametrize("one_query", [True, False], ids=["Lq1", "LqS"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_msda_fwd_bwd_at_1_and_3_levels(name, one_query, form):
    """`ops.msda_fwd` / `msda_bwd` (fp64 slab, fixed-point slab, memory atomics) against `cape_ref.msda_core` and its autograd
    at L = 1 (2 x 2 and 4 x 4) and L = 3, N = 2, P = 4, one query row (the decode step) and S query rows (the encoder).  Offsets of
    up to ~3 pixels around reference points in [-0.1, 1.1]: samples fall outside the level on every side."""
    shapes = GRIDS[name]
    L, S, N = len(shapes), sum(h * w for h, w in shapes), 2
    Lq = 1 if one_query else S
    value = rnd(N, S, 8, 32, seed=11)
    offw = torch.cat([rnd(N, Lq, 64 * L, seed=12, scale=1.5), rnd(N, Lq, 32 * L, seed=13)], -1).contiguous()
    ref = torch.rand(N, Lq, L, 2, generator=torch.Generator().manual_seed(14)) * 1.2 - 0.1
    value.requires_grad_(True); offw.requires_grad_(True); ref.requires_grad_(True)
    out_ref = _msda_ref(value, offw, ref, shapes)
    go = rnd(N, Lq, 256, seed=5)
    out_ref.backward(go)
    geo = ops.LevelGeometry(shapes)
    vd, od, rd = value.detach().to(DEV), offw.detach().to(DEV), ref.detach().to(DEV)
    close(ops.msda_fwd(vd, od, rd, geo, N, Lq), out_ref, name="msda fwd")
    dv, do, dr = ops.msda_bwd(go.to(DEV), vd, od, rd, geo, N, Lq, form=form)
    close(dv, value.grad, tol=2e-4, name="msda d_value")
    close(do, offw.grad, tol=2e-4, name="msda d_offw")
    close(dr, ref.grad, tol=2e-4, name="msda d_ref")


# ------------------------------------------------------------------------------------------------
# 2. fused offsets|weights projection
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjacent", [True, False], ids=["one_operand", "two_operands"])
@pytest.mark.parametrize("L,rows", [(1, 4), (3, 168)])
def test_linear_cat2_at_96_and_288_columns(monkeypatch, L, rows, adjacent):
    """`LinearCat2Fn` with N = 8 * 4L * 3 = 96 and 288 output columns (rows: one image's 4 tokens; two images' 84): forward, data
    gradient and weight / bias gradients against F.linear -- with weights, biases and their gradients back to back as the arenas
    place them (one (N, 256) operand forward, one weight-gradient product accumulating into the gradient views) and as separate
    tensors (two launches each, gradients handed to autograd)."""
    from cape_amd.hip import functional as HF
    n1, n2 = 64 * L, 32 * L
    x = rnd(rows, 256, seed=1)
    w, b = rnd(n1 + n2, 256, seed=2, scale=256 ** -0.5), rnd(n1 + n2, seed=3)
    g = rnd(rows, n1 + n2, seed=4)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y_ref = F.linear(xr, wr, br)
    y_ref.backward(g)
    xd = x.to(DEV).requires_grad_(True)
    if adjacent:
        wd, bd = w.to(DEV), b.to(DEV)
        ps = [torch.nn.Parameter(t) for t in (wd[:n1], bd[:n1], wd[n1:], bd[n1:])]
        gw, gb = torch.zeros_like(wd), torch.zeros_like(bd)
        for q, gview in zip(ps, (gw[:n1], gb[:n1], gw[n1:], gb[n1:])):
            q.grad = gview
        monkeypatch.setattr(HF.Runtime, "direct_grad", True)
    else:
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in (w[:n1], b[:n1], w[n1:], b[n1:])]
    assert HF._adjacent(ps[0], ps[2]) == adjacent and HF._adjacent(ps[1], ps[3]) == adjacent
    y = HF.linear_cat2(xd, *ps)
    close(y, y_ref, name="linear_cat2 fwd")
    y.backward(g.to(DEV))
    HF.Runtime.join()
    close(xd.grad, xr.grad, tol=2e-4, name="linear_cat2 data gradient")
    close(torch.cat([ps[0].grad, ps[2].grad]), wr.grad, tol=2e-4, name="linear_cat2 weight gradient")
    close(torch.cat([ps[1].grad, ps[3].grad]), br.grad, tol=2e-4, name="linear_cat2 bias gradient")


# ------------------------------------------------------------------------------------------------
# 3. teacher-forced forward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_vs_oracle(name):
    """Teacher-forced forward against the oracle of the configuration: logits, coordinates of all six layers and the room logits;
    argmax tokens exact wherever the oracle's top-2 gap is >= 2e-3, a rule that may leave out at most 1 % of the positions
    (measured on the CPU oracle for this batch: L1 0.13 %, L1_dc5 0.08 %, L3 0.17 %)."""
    ref = oracle(name)
    b = to_dev(ref["batch"])
    model = eval_product(name)
    with torch.no_grad():
        out = forward(model, b)
    enc_shapes = GRIDS[name]
    assert model.base_model.transformer.level_embed.shape == (len(enc_shapes), 256)
    logits, coords = stack_outputs(out)
    ref_logits, ref_coords = stack_outputs(ref["out"])
    e_l, e_c = (logits.cpu() - ref_logits).abs().max().item(), (coords.cpu() - ref_coords).abs().max().item()
    e_r = (out["pred_room_logits"][:, :16].cpu() - ref["out"]["pred_room_logits"][:, :16]).abs().max().item()
    print(f"{name}: logits {e_l:.3e}  coords {e_c:.3e}  room logits {e_r:.3e}")
    assert e_l < 1e-3 and e_c < 1e-4 and e_r < 1e-3
    top2 = ref_logits.sort(-1).values
    clear = (top2[..., -1] - top2[..., -2]) >= 2e-3
    excluded = 1.0 - clear.float().mean().item()
    print(f"{name}: positions excluded by the top-2 rule: {excluded:.4%} ({int((~clear).sum())} of {clear.numel()})")
    assert excluded <= 0.01
    assert torch.equal(logits.argmax(-1).cpu()[clear], ref_logits.argmax(-1)[clear])


# ------------------------------------------------------------------------------------------------
# 4. losses and gradients
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_losses_and_gradients_vs_oracle(name, gemm_precision):
    """The criterion's 19 entries and total against the oracle's; after backward() the gradient of every trainable tensor the way
    tests/test_e2e_gpu.py compares them (first 256 elements within 2e-3 * max(1, max|ref|), norm within 2e-2 relative).  In exact
    fp32 the tensors that carry the level count -- level_embed, an encoder and a decoder sampling_offsets / attention_weights
    weight (see WHOLE), every input_proj convolution -- and layer4.2.conv3.weight are also compared whole at the same bound.

    Measured on MI355X (three runs; worst 256-element head error / tolerance over the 427 / 435 gradients; norms <= 1.6e-3 relative):
      f32      L1 0.001, L1_dc5 0.001, L3 0.19 - 0.41: passes.
      bf16x3   L1 0.09 - 0.93, L3 0.49 - 0.51: passes.  L1_dc5 MISSES in every run: 3.416e-3, 3.415e-3, 3.455e-3 against 2e-3 on
               encoder.layers.1.self_attn.sampling_offsets.bias (1.7 x); every other tensor inside the bound.
    Cause, found on the CPU: the bf16x3 trunk leaves a relative error of about 1.4e-5 on C5 (tests/test_dilation_gpu.py); noise of
    that size on the ORACLE's own C5 moves the oracle's gradient of that bias by 0.8e-3, 3.3e-3, 1.5e-3 and 3.8e-3 in four seeds and
    its worst head by 1.6 - 2.2 x this bound (L1: 0.6 - 1.8 x, L3: 0.4 - 1.7 x) -- at 16 tokens per image a sample that changes
    its pixel cell is not averaged away.  Forward values (logits 4.5e-5), losses and gradient norms are far inside their bounds and
    exact fp32 is at 0.001 x.  The bound is the issue's and stays.
    The whole-tensor comparison in fp32 holds for the tensors of WHOLE (worst 0.28 x, L3); with encoder.layers.0 in
    that list instead, L3 held in one run (0.41 x) and missed in the next (3.58e-3 on 29 elements, 1.79 x: the one sample of the
    oracle that sits on a pixel boundary, see WHOLE), forward k-splits summing in arrival order."""
    from cape_amd.hip import functional as HF
    ref = oracle(name)
    b = to_dev(ref["batch"])
    model, crit = product(name)
    model.eval()
    out = forward(model, b)
    ld = crit(out, b["targets"])
    assert sorted(k for k in ld if not k.startswith("_")) == sorted(ref["losses"]) and len(ref["losses"]) == 19
    for k, v in ref["losses"].items():
        assert abs(float(ld[k]) - v) < 1e-3, (k, float(ld[k]), v)
    assert abs(float(ld["_total"]) - ref["total"]) < 1e-3, (float(ld["_total"]), ref["total"])
    ld["_total"].backward()
    HF.Runtime.join()
    named = dict(model.named_parameters(remove_duplicate=False))
    whole = WHOLE + tuple(f"base_model.input_proj.{l}.0.weight" for l in range(CONFIGS[name][0]))
    assert all(k in ref["grads"] for k in whole) and len(ref["grads"]) > 300
    worst_h, worst_n, worst_w = 0.0, 0.0, 0.0
    for k in sorted(ref["grads"]):
        r, got = ref["grads"][k], named[k].grad
        if got is None:                                             # (a zero-weighted loss: the oracle's autograd reports zeros)
            assert float(r.abs().max()) == 0.0, k
            continue
        got = got.detach().cpu()
        tol = 2e-3 * max(1.0, r.abs().max().item())
        err = (got.reshape(-1)[:256] - r.reshape(-1)[:256]).abs().max().item()
        rel = abs(got.norm().item() - r.norm().item()) / max(r.norm().item(), 1e-3)
        worst_h, worst_n = max(worst_h, err / tol), max(worst_n, rel)
        assert err <= tol, (k, err, tol)
        assert rel < 2e-2, (k, rel)
        if gemm_precision == "f32" and k in whole:
            err = (got - r).abs().max().item()
            worst_w = max(worst_w, err / tol)
            assert err <= tol, (k, "whole tensor", err, tol)
    print(f"{name}: {len(ref['grads'])} gradients; worst head error / tolerance {worst_h:.3f}, whole-tensor {worst_w:.3f}, "
          f"worst relative norm error {worst_n:.3e}")


# ------------------------------------------------------------------------------------------------
# 5. cached decode, every tier
# ------------------------------------------------------------------------------------------------
TIERS = {"whole": {}, "stage": {"CAPE_DECODE_MEGA": "0"}, "per_op": {"CAPE_DECODE_FUSED": "0"}}


@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_cached_decode_vs_oracle(monkeypatch, name, tier):
    """forward_inference running free until every sequence has ended, in each step tier, against the oracle's
    `cape_forward_inference`: the same tokens, coordinates within 1e-4, logits within 1e-3.  The oracle's smallest top-2 gap along
    its stream is asserted to be >= 2e-3 (measured: L1 6.7e-2 over 14 steps, L1_dc5 7.6e-3 over 44 steps, L3 2.3e-2 over 7 steps), so
    the logit tolerance cannot flip a token.  Call 1 of the geometry runs eagerly, call 2 captures the steps while it decodes,
    call 3 replays them: bitwise the eager outputs.  The default tier must be the whole-step kernel."""
    for k in ("CAPE_DECODE_MEGA", "CAPE_DECODE_FUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in TIERS[tier].items():
        monkeypatch.setenv(k, v)
    ref = decode_oracle(name)
    top2 = ref["logits"].sort(-1).values
    gap = (top2[..., -1] - top2[..., -2]).min().item()
    print(f"{name}: {ref['logits'].shape[1]} steps, smallest top-2 gap along the oracle's stream {gap:.3e}")
    assert gap >= 2e-3
    b = to_dev(batch())
    model = eval_product(name)
    model.base_model._decode_states.clear()
    p = decode(model, b, graph=True, timing=True)
    tm = p["_timing"]
    assert (tm["whole_step_kernel"], tm["fused"], tm["launch"]) == (tier == "whole", tier != "per_op", "eager"), tm
    assert p["logits"].shape == ref["logits"].shape, (p["logits"].shape, ref["logits"].shape)
    e_l = (p["logits"].cpu() - ref["logits"]).abs().max().item()
    e_c = (p["coordinates"].cpu() - ref["coordinates"]).abs().max().item()
    print(f"{name} / {tier}: decode logits {e_l:.3e}  coordinates {e_c:.3e}")
    assert torch.equal(p["sequences"].cpu(), ref["sequences"])
    assert e_c < 1e-4 and e_l < 1e-3
    for launch in ("graph", "graph"):                               # the capturing call, then a replayed one
        g = decode(model, b, graph=True, timing=True)
        assert g["_timing"]["launch"] == launch
        assert torch.equal(g["logits"], p["logits"]) and torch.equal(g["coordinates"], p["coordinates"])
    (st,) = model.base_model._decode_states.values()
    assert st.tier == tier and st.calls == 3 and len(st.graphs) >= p["logits"].shape[1]


# ------------------------------------------------------------------------------------------------
# 6. four levels: unchanged
# ------------------------------------------------------------------------------------------------
def test_four_level_whole_step_decode_unchanged(golden_dir, proc_sd):
    """The default model's whole-step decode still gives the reference's stream of e2e64_decode.npz, at the tolerances of
    tests/test_e2e_gpu.py::test_cached_decode_vs_reference_golden, and two calls give bitwise the same outputs."""
    d = np.load(os.path.join(golden_dir, "e2e64_decode.npz"))
    t = lambda a: torch.from_numpy(np.asarray(a))
    sd = dict(proc_sd)
    sd["base_model.class_embed.5.bias"] = sd["base_model.transformer.decoder.class_embed.5.bias"] = \
        sd["base_model.class_embed.5.bias"] + t(d["bias_delta"])
    args, tok, model, crit = build_product(proc_sd=sd)
    model.eval()
    tok.seq_len = 40                                            # the fixture's stream: 40 steps, no <eos>
    b = to_dev(batch())
    ref_logits, ref_coords = t(d["logits"]), t(d["coordinates"])
    p = decode(model, b, graph=False, timing=True)
    assert p["_timing"]["whole_step_kernel"]
    assert p["logits"].shape == ref_logits.shape
    assert (p["logits"][:, :4].cpu() - ref_logits[:, :4]).abs().max() < 1e-3
    top2 = ref_logits.sort(-1).values
    clear = (top2[..., 2] - top2[..., 1]) > 5e-2
    assert torch.equal(p["sequences"].cpu()[clear], t(d["sequences"]).long()[clear])
    again = decode(model, b, graph=False)
    assert torch.equal(again["logits"], p["logits"]) and torch.equal(again["coordinates"], p["coordinates"])
    stream = {k: v.to(DEV) for k, v in cape_ref.stream_from_outputs(ref_logits, ref_coords, cape_ref.Cfg()).items()}
    q = decode(model, b, teacher_stream=stream)
    assert (q["logits"].cpu() - ref_logits).abs().max() < 1e-3
    assert (q["coordinates"].cpu() - ref_coords).abs().max() < 1e-4
    assert torch.equal(q["sequences"].cpu(), t(d["sequences"]).long())


# ------------------------------------------------------------------------------------------------
# 7. captured train step
# ------------------------------------------------------------------------------------------------
def test_single_level_dc5_graphed_train_step_matches_eager(monkeypatch):
    """One model.train() step of the one-level `--dilation` product under GraphedTrainStep: eager warm-up, capture, one replay.
    At learning rate 0 the parameters stay put, so the replayed step sees the eager step's model: with the same dropout seed its
    loss equals the eager loss of the same call (the test of tests/test_dilation_gpu.py at one level; forward k-splits off)."""
    from cape_amd.hip import functional as HF
    from cape_amd.runtime.graph_step import GraphedTrainStep
    from cape_amd.runtime.optimizer import ArenaAdamW
    monkeypatch.setattr(HF, "_DETERMINISTIC", True)
    b = to_dev(batch())
    model, crit = product("L1_dc5")
    model.train()
    opt = ArenaAdamW(model, lr=0.0, lr_backbone=0.0, weight_decay=1e-4, max_norm=0.1)
    watched = [model.base_model.input_proj[0][0].weight, model.base_model.transformer.level_embed,
               model.base_model.backbone[0].body.layer4[1].conv2.weight]
    before = [w.detach().clone() for w in watched]

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
    for w, w0 in zip(watched, before):
        assert torch.equal(w.detach(), w0)


# ------------------------------------------------------------------------------------------------
# 8. checkpoint round trip
# ------------------------------------------------------------------------------------------------
def test_three_level_checkpoint_round_trip(monkeypatch, tmp_path):
    """Three levels: one optimizer step, model + ArenaAdamW state written as the training loop writes them and read back by
    util.checkpoint.load_checkpoint into a fresh model and optimizer; the next step's loss is bitwise the loss the first model
    computes, and the optimizer state that comes back out is the state that went in (names, not arena order, carry it)."""
    from cape_amd.hip import functional as HF
    from cape_amd.runtime.optimizer import ArenaAdamW
    from cape_amd.util.checkpoint import load_checkpoint
    monkeypatch.setattr(HF, "_DETERMINISTIC", True)
    b = to_dev(batch())

    def loss_of(model, crit):
        HF.Runtime.seed(78, torch.device(DEV))
        return crit(forward(model, b), b["targets"])["_total"]

    model, crit = product("L3")
    model.train()
    opt = ArenaAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4, max_norm=0.1)
    opt.zero_grad()
    HF.Runtime.seed(77, torch.device(DEV))
    crit(forward(model, b), b["targets"])["_total"].backward()
    opt.step()
    path = tmp_path / "checkpoint_levels3.pth"
    torch.save({"model": model.state_dict(), "optimizer": opt.state_dict(), "epoch": 0}, path)
    with torch.no_grad():
        next_loss = float(loss_of(model, crit))
    ck = load_checkpoint(str(path))
    assert ck["model"]["base_model.transformer.level_embed"].shape == (3, 256)
    assert sorted(k for k in ck["model"] if k.startswith("base_model.input_proj.") and k.endswith(".0.weight")) == \
        [f"base_model.input_proj.{l}.0.weight" for l in range(3)]
    model2, crit2 = product("L3")
    model2.train()
    missing, unexpected = model2.load_state_dict(ck["model"], strict=True)
    assert not missing and not unexpected
    opt2 = ArenaAdamW(model2, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4, max_norm=0.1)
    opt2.load_state_dict(ck["optimizer"])
    back = opt2.state_dict()
    assert sorted(back["state"]) == sorted(ck["optimizer"]["state"]) and len(back["state"]) > 300
    assert any(float(s["exp_avg"].abs().max()) > 0 for s in back["state"].values())
    for i, s in ck["optimizer"]["state"].items():
        assert torch.equal(back["state"][i]["exp_avg"].cpu(), s["exp_avg"]) and torch.equal(back["state"][i]["exp_avg_sq"].cpu(), s["exp_avg_sq"])
        assert float(back["state"][i]["step"]) == 1.0
    with torch.no_grad():
        loaded_loss = float(loss_of(model2, crit2))
    print(f"loss of the step after the checkpoint: {next_loss!r} / after the round trip {loaded_loss!r}")
    assert np.isfinite(next_loss) and loaded_loss == next_loss

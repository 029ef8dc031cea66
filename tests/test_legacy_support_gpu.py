"""The reference's default support encoder (SupportPoseGraphEncoder) on the GPU: every new kernel against torch CPU math, the
fully-masked-row attention mode on both routes, then the encoder and the 64x64 model against the reference's own outputs
(tests/golden/legacy_*.npz, tests/make_golden_legacy_encoder.py), dropout statistics, hipGraph replay, CLI + eval script."""
import argparse
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
PE_KEY = "support_encoder.pos_embedding.pe"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def t(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, tol=1e-5, name=""):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * max(1.0, float(b.abs().max())), (name, err)


@pytest.fixture
def legacy_sd():
    """Procedural weights of the default model: the committed spec with the encoder keys of the diff; `pos_embedding.pe` as built."""
    from oracle import procweights
    from tests.test_legacy_support_cpu import _legacy_spec
    spec, _ = _legacy_spec()
    sd = procweights.procedural_state_dict([(k, s) for k, s in spec if k != PE_KEY])
    import cape_amd  # noqa: F401
    from cape_amd.models.support_encoder import PositionalEncoding1D
    sd[PE_KEY] = PositionalEncoding1D(256).pe.clone()
    return sd


def encoder_sd(sd):
    p = "support_encoder."
    return {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}


def ref_degree(skel, P):
    """_build_adjacency_matrix row sums (support_encoder.py:94-116), restated."""
    adj = torch.zeros(len(skel), P, P, dtype=torch.long)
    for b, edges in enumerate(skel):
        for e in edges or []:
            if len(e) == 2:
                s, d = e
                s, d = (s - 1 if s > 0 else s), (d - 1 if d > 0 else d)
                if 0 <= s < P and 0 <= d < P:
                    adj[b, s, d] = 1
                    adj[b, d, s] = 1
    return adj.sum(2)


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
def test_edge_info_rules_forward_backward():
    import cape_amd  # noqa: F401
    from cape_amd.hip import ops
    from cape_amd.models.graph_utils import _edge_tables
    P, C = 37, 256
    skel = [[[0, 1], [1, 2], [2, 3], [3, 2], [37, 36], [38, 1], [-1, 4], [5, 5], [5, 5], [10, 40]],
            [],
            [[i, (i * 7) % 37] for i in range(37)] + [[36, 0], [0, 36]],
            [[1, 2]] * 20]
    flat = [tuple(e) for s in skel for e in s]
    start = np.cumsum([0] + [len(s) for s in skel]).tolist()
    edges, st = _edge_tables(flat, start, torch.device(DEV))[:2]
    N = len(skel)
    E = rnd(2, C, seed=1)
    out = torch.full((N * P, 2 * C), 7.0, device=DEV)
    scale, has, deg = ops.support_edge_info_fwd(edges, st, E.to(DEV), out[:, C:], N, P, want_degree=True)
    want_deg = ref_degree(skel, P).reshape(-1)
    assert torch.equal(deg.cpu().long(), want_deg)
    sc = want_deg.float().clamp(min=1.0) / 10.0
    want = E[(want_deg > 0).long()] * sc[:, None]
    close(out[:, C:], want, tol=0, name="edge_info")
    assert float(out[:, :C].sub(7.0).abs().max()) == 0.0               # the left half is not touched
    g = rnd(N * P, 2 * C, seed=2).to(DEV)
    dE = torch.full((2, C), 0.5, device=DEV)
    ops.support_edge_info_bwd(g[:, C:], scale, has, dE)
    Er = E.clone().requires_grad_(True)
    (Er[(want_deg > 0).long()] * sc[:, None]).backward(g[:, C:].cpu())
    close(dE - 0.5, Er.grad, tol=1e-5, name="d edge_embedding")
    dE2 = torch.full((2, C), 0.5, device=DEV)
    ops.support_edge_info_bwd(g[:, C:], scale, has, dE2)
    assert torch.equal(dE, dE2)                                         # fixed-order reduction


def test_coord_embed_and_pe_dropout():
    import cape_amd  # noqa: F401
    from cape_amd.hip import ops
    from cape_amd.hip.functional import Runtime
    R, C, P = 3 * 17, 256, 17
    coords = torch.rand(R, 2, generator=torch.Generator().manual_seed(3))
    W0, b0 = rnd(C, 2, seed=4), rnd(C, seed=5, scale=0.3)
    h = ops.legacy_coord_embed_fwd(coords.to(DEV), W0.to(DEV), b0.to(DEV))
    cr, Wr, br = coords.clone().requires_grad_(True), W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    hr = F.relu(F.linear(cr, Wr, br))
    close(h, hr, tol=1e-6, name="coord mlp0")
    g = rnd(R, C, seed=6)
    hr.backward(g)
    dW, db = torch.zeros(C, 2, device=DEV), torch.zeros(C, device=DEV)
    dc = ops.legacy_coord_embed_bwd(g.to(DEV), h, coords.to(DEV), W0.to(DEV), dW, db, want_dcoords=True)
    close(dW, Wr.grad, tol=1e-5); close(db, br.grad, tol=1e-5); close(dc, cr.grad, tol=1e-5)
    # PE add, no dropout: exact
    x = rnd(R, C, seed=7).to(DEV)
    pe = rnd(5000, C, seed=8).to(DEV)
    close(ops.pe_dropout_fwd(x, pe, P), x.cpu() + pe[:P].cpu().repeat(3, 1), tol=0, name="x + pe")
    # dropout(x + pe): keep rate, scaling, and a backward that drops the same elements
    Runtime.seed(11, DEV)
    rng = Runtime.get_rng(DEV)
    xs = torch.ones(64 * P, C, device=DEV)
    zeros = torch.zeros(P, C, device=DEV)
    y = ops.pe_dropout_fwd(xs, zeros, P, 0.1, rng, 5)
    kept = y != 0
    rate = float(kept.float().mean())
    assert abs(rate - 0.9) < 0.005, rate
    assert torch.allclose(y[kept], torch.full_like(y[kept], 1.0 / 0.9))
    dx = ops.pe_dropout_bwd(torch.ones_like(xs), 0.1, rng, 5)
    assert torch.equal(dx, y)
    y2 = ops.pe_dropout_fwd(xs, zeros, P, 0.1, rng, 6)
    assert not torch.equal(y, y2)                                       # its own stream id


def _attn_case(Lq, mode, seed):
    import cape_amd  # noqa: F401
    from cape_amd.hip import ops
    N, H = 3, 8
    q, k, v = (rnd(N, Lq, H * 32, seed=seed + i) for i in range(3))
    kpm = torch.zeros(N, Lq, dtype=torch.uint8)
    kpm[0, 1::3] = 1                        # partly masked
    kpm[1] = 1                              # every key masked
    return N, H, q, k, v, kpm


def _torch_attention(q, k, v, kpm, N, H, L):
    """Zero attention on fully masked rows (torch's result with grad enabled)."""
    Lk = k.shape[1]
    qh = q.view(N, -1, H, 32).transpose(1, 2)
    kh, vh = (x.view(N, Lk, H, 32).transpose(1, 2) for x in (k, v))
    s = qh @ kh.transpose(-1, -2) * 32 ** -0.5
    s = s.masked_fill(kpm.bool()[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True).detach().clamp(min=-1e30)           # (a row of -inf: exp -> 0, sum 0 -> P = 0, finite gradients)
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True).clamp(min=1e-30)
    return (p @ vh).transpose(1, 2).reshape(N, -1, H * 32)


@pytest.mark.parametrize("L", [17, 68])                     # short-row kernels / matrix-core route (ops.attn_mm_ok)
def test_fully_masked_row_mode_both_routes(L):
    import cape_amd  # noqa: F401
    from cape_amd.hip import ops
    N, H, q, k, v, kpm = _attn_case(L, 3, 20)
    scale = 32 ** -0.5
    mm = ops.attn_mm_ok(N, H, L, L)
    assert mm == (L == 68)
    qd, kd, vd, kd8 = q.to(DEV), k.to(DEV), v.to(DEV), kpm.to(DEV)
    qr, kr, vr = (x.clone().requires_grad_(True) for x in (q, k, v))
    ref = _torch_attention(qr, kr, vr, kpm, N, H, L)
    gO = rnd(N, L, H * 32, seed=30)
    ref.backward(gO)
    dq, dk, dv = (torch.empty(N, L, H * 32, device=DEV) for _ in range(3))
    if mm:
        O, P_, Pu = ops.attn_mm_fwd(qd, kd, vd, N, H, L, L, scale, mask_mode=3, kpm=kd8)
        ops.attn_mm_bwd(gO.to(DEV), qd, kd, vd, P_, Pu, dq, dk, dv, N, H, L, L, scale)
        O2 = ops.attn_mm_fwd(qd, kd, vd, N, H, L, L, scale, mask_mode=2, kpm=kd8)[0]
    else:
        O, lse = ops.attn_fwd(qd, kd, vd, N, H, L, L, scale, mask_mode=3, kpm=kd8)
        assert torch.isfinite(lse).all()
        ops.attn_bwd(gO.to(DEV), qd, kd, vd, O, lse, dq, dk, dv, N, H, L, L, scale, mask_mode=3, kpm=kd8)
        O2 = ops.attn_fwd(qd, kd, vd, N, H, L, L, scale, mask_mode=2, kpm=kd8)[0]
    tol = 2e-3 if mm else 2e-5                                 # (the matrix-core route's contractions run in the bf16x3 split)
    close(O, ref, tol=tol, name="O")
    assert float(O[1].abs().max()) == 0.0
    for got, want, n in ((dq, qr.grad, "dq"), (dk, kr.grad, "dk"), (dv, vr.grad, "dv")):
        assert torch.isfinite(got).all(), n
        close(got, want, tol=max(tol, 1e-4), name=n)
    assert float(dq[1].abs().max()) == 0.0 and float(dk[1].abs().max()) == 0.0 and float(dv[1].abs().max()) == 0.0
    # mask_mode 2 unchanged: NaN on the fully masked graph, bitwise mode 3 elsewhere
    assert torch.isnan(O2[1]).all()
    assert torch.equal(O2[0], O[0]) and torch.equal(O2[2], O[2])


def test_decode_form_fully_masked_row():
    """Lq == 1 takes the single-query kernel."""
    import cape_amd  # noqa: F401
    from cape_amd.hip import ops
    N, H, Lk = 2, 8, 9
    q, k, v = rnd(N, 1, 256, seed=1), rnd(N, Lk, 256, seed=2), rnd(N, Lk, 256, seed=3)
    kpm = torch.zeros(N, Lk, dtype=torch.uint8)
    kpm[1] = 1
    kpm[0, 3] = 1
    O, lse = ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), N, H, 1, Lk, 32 ** -0.5, mask_mode=3, kpm=kpm.to(DEV))
    close(O, _torch_attention(q, k, v, kpm, N, H, 1), tol=2e-5)
    assert float(O[1].abs().max()) == 0.0 and torch.isfinite(lse).all()


def test_final_layernorm_zero_rows_leave_as_beta():
    import cape_amd  # noqa: F401
    from cape_amd.hip import functional as HF
    x = rnd(4, 7, 256, seed=40)
    x[1] = 0.0
    g, b = rnd(256, seed=41) * 0.1 + 1.0, rnd(256, seed=42) * 0.1
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (256,), gr, br, 1e-5)
    gout = rnd(4, 7, 256, seed=43)
    ref.backward(gout)
    xd = x.to(DEV).requires_grad_(True)
    gd, bd = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = HF.add_layernorm(xd, None, gd, bd)
    close(out, ref, tol=2e-6, name="ln")
    assert torch.equal(out[1].cpu(), b.expand(7, 256))
    out.backward(gout.to(DEV))
    close(xd.grad, xr.grad, tol=2e-4, name="ln dx"); close(gd.grad, gr.grad, tol=1e-4); close(bd.grad, br.grad, tol=1e-5)


# ------------------------------------------------------------------------------------------------
# encoder and model against the reference
# ------------------------------------------------------------------------------------------------
def _encoder(legacy_sd):
    import cape_amd  # noqa: F401
    from cape_amd.models.support_encoder import SupportPoseGraphEncoder
    enc = SupportPoseGraphEncoder()
    enc.load_state_dict(encoder_sd(legacy_sd), strict=True)
    return enc.to(DEV).eval()


@pytest.fixture(params=["f32", "bf16x3"])
def precision(request):
    """GEMM arithmetic: exact fp32 at the support-encoder tolerance (2e-5), the default bf16x3 split at 1e-4."""
    from cape_amd.hip import ops
    old = ops.get_gemm_precision()
    ops.set_gemm_precision(request.param)
    yield 2e-5 if request.param == "f32" else 1e-4
    ops.set_gemm_precision(old)


def test_encoder_vs_reference_golden(golden_dir, legacy_sd, precision):
    tol = precision
    d = np.load(os.path.join(golden_dir, "legacy_support_encoder.npz"))
    skel = json.loads(bytes(d["skel_json"]).decode())
    coords, smask = t(d["coords"]).to(DEV), t(d["support_mask"]).to(DEV)
    enc = _encoder(legacy_sd)
    P = coords.shape[1]
    assert torch.equal(ref_degree(skel, P), t(d["degree"]))
    c = coords.clone().requires_grad_(True)
    out = enc(c, smask, skel)
    close(out, t(d["out_grad"]), tol=tol, name="out (grad path)")
    out.backward(t(d["gout"]).to(DEV))
    named = dict(enc.named_parameters())
    for k in d.files:
        kind, _, name = k.partition(":")
        if kind == "grad":
            close(named[name].grad, t(d[k]), tol=1e-4, name=k)
        elif kind == "gradhead":
            close(named[name].grad.reshape(-1)[:512], t(d[k]), tol=1e-4, name=k)
        elif kind == "gradnorm":
            assert abs(float(named[name].grad.norm()) - float(d[k])) <= 1e-4 * max(1.0, float(d[k])), k
    close(c.grad, t(d["grad_coords"]), tol=1e-4, name="d coords")
    with torch.no_grad():
        close(enc(coords, smask, None), t(d["out_noskel"]), tol=tol, name="no skeleton")
        got = enc(coords, smask, skel)
        ref = t(d["out_nograd"])
        finite = torch.isfinite(ref).flatten(1).all(1)
        # the reference's non-nested no-grad fast path gives NaN rows for the graph with every key masked; here such rows get
        # zero attention, as on the grad path
        assert finite.tolist() == [True, False, True, True]
        close(got[finite], ref[finite], tol=tol, name="no grad, not left-aligned")
        close(got[~finite], t(d["out_grad"])[~finite], tol=tol, name="fully masked, no grad")
        fast = enc(coords[1:], smask[1:], skel[1:])                        # nested path: padded rows -> norm.bias
        close(fast, t(d["out_fast"]), tol=tol, name="nested path")
        assert int(d["allmasked_raises"]) == 1                              # the reference raises; the deviation returns norm.bias
        allm = enc(coords[1:2], smask[1:2], skel[1:2])
        assert torch.equal(allm[0], enc.norm.bias.detach().expand(P, 256))


def _build_default(legacy_sd, extra=()):
    import cape_amd  # noqa: F401
    from cape_amd.datasets import DiscreteTokenizerV2
    from cape_amd.models import build_model
    from cape_amd.models.cape_model import build_cape_model
    from cape_amd.models.train_cape_episodic import get_args_parser
    args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(list(extra))
    tok = DiscreteTokenizerV2(int(args.vocab_size ** 0.5), args.seq_len, add_cls=False)
    base, crit = build_model(args, tokenizer=tok)
    model = build_cape_model(args, base)
    if legacy_sd is not None:
        missing, unexpected = model.load_state_dict(legacy_sd, strict=True)
        assert not missing and not unexpected
    return args, tok, model.to(DEV), crit.to(DEV)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_e2e64_vs_reference_golden(golden_dir, legacy_sd, precision):
    from oracle import cape_ref, synth
    from tests.helpers import to_dev
    from cape_amd.hip import ops
    old = ops.get_gemm_precision()
    ops.set_gemm_precision(precision)
    try:
        d = np.load(os.path.join(golden_dir, "legacy_e2e64.npz"))
        args, tok, model, crit = _build_default(legacy_sd)
        model.eval()
        cfg = cape_ref.Cfg()
        b = to_dev(synth.make_batch(11, 2, 2, 64, 9, cfg, n_invisible=(2, 0)))
        out = model(samples=b["images"], support_coords=b["support_coords"], support_mask=b["support_mask"], targets=b["targets"],
                    skeleton_edges=b["skeleton"])
        logits = torch.stack([a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]])
        coords = torch.stack([a["pred_coords"] for a in out["aux_outputs"]] + [out["pred_coords"]])
        assert (logits.cpu() - t(d["logits"])).abs().max() < 1e-3
        assert (coords.cpu() - t(d["coords"])).abs().max() < 1e-4
        assert torch.equal(logits.argmax(-1).cpu(), t(d["logits"]).argmax(-1))
        ld = crit(out, b["targets"])
        for k, v in zip(json.loads(bytes(d["loss_keys"]).decode()), d["loss_vals"]):
            assert abs(float(ld[k]) - float(v)) < 1e-3, k
        assert abs(float(ld["_total"]) - float(d["loss"])) < 5e-3
        ld["_total"].backward()
        named = dict(model.named_parameters(remove_duplicate=False))
        for k in d.files:
            if k.startswith(("grad:", "gradhead:")):
                name = k.split(":", 1)[1]
                ref = t(d[k])
                got = named[name].grad.detach().cpu()
                got = got.reshape(-1)[:256] if k.startswith("gradhead:") else got
                assert (got.reshape(ref.shape) - ref).abs().max() <= 2e-3 * max(1.0, float(ref.abs().max())), k
        # free-running cached decode (the batch with some unmasked keys in every graph, see the generator)
        sd = dict(legacy_sd)
        for key in ("base_model.class_embed.5.bias", "base_model.transformer.decoder.class_embed.5.bias"):
            sd[key] = sd[key] + t(d["bias_delta"])
        model.load_state_dict(sd, strict=True)
        tok.seq_len = 40
        db = to_dev(synth.make_batch(11, 2, 2, 64, 9, cfg, n_invisible=(2, 3)))
        with torch.no_grad():
            p = model.forward_inference(samples=db["images"], support_coords=db["support_coords"], support_mask=db["support_mask"],
                                        skeleton_edges=db["skeleton"])
        ref_l = t(d["dec_logits"])
        assert (p["logits"][:, :ref_l.shape[1]].cpu() - ref_l).abs().max() < 1e-3
        seq = t(d["dec_sequences"]).long()
        assert torch.equal(p["sequences"][:, :seq.shape[1]].cpu(), seq)
    finally:
        ops.set_gemm_precision(old)


def test_graphed_train_step_matches_eager(monkeypatch):
    """GraphedTrainStep on the default model: the replayed steps follow the eager ones (losses, parameters)."""
    from cape_amd.hip import functional as HF
    from cape_amd.hip import ops
    from cape_amd.runtime.graph_step import GraphedTrainStep
    from cape_amd.runtime.optimizer import ArenaAdamW
    from cape_amd.datasets import episodic_collate_fn
    from cape_amd.datasets.synthetic import SyntheticEpisodes
    monkeypatch.setattr(HF, "_DETERMINISTIC", True)
    args, tok, _, _ = _build_default(None, ["--image_size", "64"])
    ds = SyntheticEpisodes(tok, 12, 64, 17, 2, seed=5)
    batches = []
    for i in range(3):
        b = episodic_collate_fn([ds[i * 4 + j] for j in range(4)])
        batches.append((b["query_images"].to(DEV), b["support_coords"].to(DEV), b["support_masks"].to(DEV),
                        {k: v.to(DEV) for k, v in b["query_targets"].items()}, b["support_skeletons"]))

    def run(graphed):
        torch.manual_seed(0)
        ops._stream_counter[0] = 0
        _, _, model, crit = _build_default(None, ["--image_size", "64"])
        model.train()
        HF.Runtime.seed(77, DEV)
        opt = ArenaAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4, max_norm=0.1)
        step = GraphedTrainStep(model, crit, opt, edge_capacity=512, eager_steps=(1 if graphed else 10 ** 9))
        losses = [float(step(*batches[it % 3])["_total"]) for it in range(5)]
        assert (len(step.cache) == 1) == graphed
        enc = model.support_encoder
        flat = torch.cat([p.detach().reshape(-1)[:64] for p in enc.parameters()])
        return losses, flat

    le, pe = run(False)
    lg, pg = run(True)
    for a_, b_ in zip(le, lg):
        assert abs(a_ - b_) <= 2e-4 * max(1.0, abs(a_)), (le, lg)
    d = (pe - pg).abs()
    assert d.max().item() <= 6e-4 and d.mean().item() <= 5e-6, (d.max().item(), d.mean().item())


def test_cli_default_encoder_then_eval_script(tmp_path):
    """The CLI without --use_geometric_encoder for one epoch on synthetic episodes, then eval_cape_checkpoint.py on the
    checkpoint it wrote: strict weights-only load (pos_embedding.pe included), decode equal to the in-process decode."""
    import glob
    import cape_amd  # noqa: F401
    from cape_amd.models.train_cape_episodic import get_args_parser, main
    from cape_amd.scripts import eval_cape_checkpoint
    from cape_amd.util.checkpoint import load_checkpoint
    os.environ["WARN_INCOMPLETE_GENERATION"] = "0"
    args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(
        ["--dataset_name", "synthetic", "--image_size", "64", "--batch_size", "2", "--episodes_per_epoch", "4",
         "--val_episodes_per_epoch", "2", "--num_workers", "0", "--output_dir", str(tmp_path), "--print_freq", "0", "--epochs", "1"])
    hist = main(args)
    assert len(hist) == 1 and np.isfinite(hist[0]["train"]["loss"])
    ck_path = sorted(glob.glob(str(tmp_path / "checkpoint_e*.pth")))[-1]
    ck = load_checkpoint(ck_path)
    assert len(ck["model"]) == 752 and PE_KEY in ck["model"] and not ck["args"].use_geometric_encoder
    model, a2, tok, _ = eval_cape_checkpoint.load_checkpoint_and_model(ck_path, torch.device("cuda:0"))
    missing, unexpected = model.load_state_dict(ck["model"], strict=True)
    assert not missing and not unexpected
    from oracle import cape_ref, synth
    b = synth.make_batch(5, 2, 2, 64, 9, cape_ref.Cfg(), n_invisible=(2, 3))
    tok.seq_len = 40
    model.base_model.tokenizer.seq_len = 40
    with torch.no_grad():
        p1 = model.forward_inference(samples=b["images"].cuda(), support_coords=b["support_coords"].cuda(),
                                     support_mask=b["support_mask"].cuda(), skeleton_edges=b["skeleton"])
    _, _, m2, _ = _build_default(None, ["--image_size", "64"])
    m2.load_state_dict(ck["model"], strict=True)
    m2.eval()
    m2.base_model.tokenizer.seq_len = 40
    with torch.no_grad():
        p2 = m2.forward_inference(samples=b["images"].cuda(), support_coords=b["support_coords"].cuda(),
                                  support_mask=b["support_mask"].cuda(), skeleton_edges=b["skeleton"])
    assert torch.equal(p1["sequences"], p2["sequences"]) and torch.equal(p1["logits"], p2["logits"])
    m = eval_cape_checkpoint.main(["--checkpoint", ck_path, "--num-episodes", "2", "--output-dir", str(tmp_path / "eval")])
    assert 0.0 <= m["pck_overall"] <= 1.0

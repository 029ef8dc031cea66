"""TEST INFRASTRUCTURE ONLY -- emits the fixtures of the reference's default support encoder (SupportPoseGraphEncoder,
built when `--use_geometric_encoder` is NOT passed) from the REAL reference:

  tests/golden/state_dict_spec_legacy_diff.json   keys / shapes that differ from state_dict_spec.json
  tests/golden/legacy_support_encoder.npz         encoder outputs, gradients, nested-path outputs, degree vectors
  tests/golden/legacy_e2e64.npz                   64x64 teacher-forced forward, losses, selected gradients, decode tokens

Runs only where the reference tree is importable (oracle/refshim.py); not collected by pytest.
Re-run:  python -m tests.make_golden_legacy_encoder
"""
import argparse
import json
import math
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import cape_ref, procweights, refshim, synth  # noqa: E402

OUT = os.path.join(HERE, "golden")
PE_KEY = "support_encoder.pos_embedding.pe"
os.environ["WARN_INCOMPLETE_GENERATION"] = "0"
warnings.filterwarnings("ignore")

P = 7
# support masks in the sampler's convention, passed un-inverted to the encoder (which pads where they are False)
SUPPORT_MASK = [[1, 0, 1, 0, 0, 1, 1],       # not left-aligned
                [0, 0, 0, 0, 0, 0, 0],       # every key masked
                [1, 1, 1, 0, 0, 0, 0],       # left-aligned
                [1, 1, 1, 1, 1, 1, 1]]       # nothing masked
# every edge rule of _build_adjacency_matrix: s = 0 keeps index 0, s = N maps to N-1, negative and > N dropped, duplicates and
# reversed duplicates once, a self-loop once, entries whose length is not 2 skipped, an empty list
SKELETON = [[[0, 1], [1, 2], [2, 3], [3, 2], [2, 3], [7, 6], [-1, 2], [9, 1], [4, 4]],
            [[1, 2], [2, 3], [1, 2, 3], [5, 6]],
            [[0, 0], [0, 3], [3, 0]],
            []]


def npz(name, **arrs):
    conv = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    np.savez_compressed(os.path.join(OUT, name), **conv)
    print("wrote", name, os.path.getsize(os.path.join(OUT, name)), "bytes")


def jbytes(x):
    return np.frombuffer(json.dumps(x).encode(), dtype=np.uint8)


def build_reference_default():
    """refshim.build_reference without --use_geometric_encoder: the reference's own default argv."""
    refshim.install()
    from models.train_cape_episodic import get_args_parser
    from models import build_model
    from models.cape_model import build_cape_model
    from models.cape_losses import build_cape_criterion
    from datasets.discrete_tokenizer import DiscreteTokenizerV2
    args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(["--device", "cpu"])
    tok = DiscreteTokenizerV2(num_bins=int(math.sqrt(args.vocab_size)), seq_len=args.seq_len, add_cls=False)
    base, _ = build_model(args, tokenizer=tok)
    model = build_cape_model(args, base)
    crit = build_cape_criterion(args, num_classes=3)
    return args, tok, model, crit


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    args, tok, model, crit = build_reference_default()
    sd0 = model.state_dict()
    spec = [(k, tuple(v.shape)) for k, v in sd0.items()]
    built = {k: v for k, v in sd0.items() if k in procweights.KEEP_AS_BUILT}
    sd = procweights.procedural_state_dict(spec, built)
    sd[PE_KEY] = sd0[PE_KEY].clone()                  # as built
    model.load_state_dict(sd, strict=True)
    geo = dict(procweights.load_spec())
    leg = dict(spec)
    diff = {"removed": sorted(k for k in geo if k not in leg),
            "added": [[k, list(s)] for k, s in spec if k not in geo],
            "n_entries": len(spec),
            "n_trainable": sum(p.numel() for p in model.parameters() if p.requires_grad)}
    with open(os.path.join(OUT, "state_dict_spec_legacy_diff.json"), "w") as f:
        json.dump(diff, f, indent=0)

    # ---------------- encoder alone ----------------
    se = model.support_encoder
    model.eval()
    rng = np.random.Generator(np.random.PCG64(17))
    coords = torch.from_numpy(rng.random((4, P, 2), dtype=np.float32))
    smask = torch.tensor(SUPPORT_MASK, dtype=torch.bool)
    adj = se._build_adjacency_matrix(SKELETON, P, "cpu")
    degree = adj.sum(dim=2)
    cg = coords.clone().requires_grad_(True)
    out_grad = se(cg, smask, SKELETON)                             # eval, grad enabled: per-layer slow path
    gout = torch.from_numpy(rng.standard_normal(tuple(out_grad.shape)).astype(np.float32))
    se.zero_grad(set_to_none=True)
    out_grad.backward(gout)
    # small gradients whole, the large ones as their first 512 elements plus the norm (the file stays well under 500 KB)
    grads = {}
    for n, p in se.named_parameters():
        if p.grad is None:
            continue
        if p.numel() <= 4096:
            grads["grad:" + n] = p.grad
        else:
            grads["gradhead:" + n] = p.grad.reshape(-1)[:512]
            grads["gradnorm:" + n] = np.array(float(p.grad.norm()))
    out_noskel = se(coords, smask, None).detach()                   # no skeleton: coord_edge_proj is skipped
    with torch.no_grad():
        out_nograd = se(coords, smask, SKELETON)                    # not left-aligned over the batch: no nested tensor
        out_fast = se(coords[1:], smask[1:], SKELETON[1:])          # left-aligned batch (one graph fully masked): nested path
        try:
            se(coords[1:2], smask[1:2], SKELETON[1:2])
            allm_raises = 0
        except RuntimeError:
            allm_raises = 1                                         # to_padded_tensor of an all-empty nested tensor
    npz("legacy_support_encoder.npz", coords=coords, support_mask=smask, skel_json=jbytes(SKELETON), degree=degree,
        out_grad=out_grad, gout=gout, grad_coords=cg.grad, out_noskel=out_noskel, out_nograd=out_nograd, out_fast=out_fast,
        allmasked_raises=np.array(allm_raises), torch_version=jbytes(torch.__version__), **grads)

    # ---------------- end to end, 64x64 ----------------
    cfg = cape_ref.Cfg()
    batch = synth.make_batch(11, 2, 2, 64, 9, cfg, n_invisible=(2, 0))
    model.eval()
    model.zero_grad(set_to_none=True)
    out = model(samples=batch["images"], support_coords=batch["support_coords"], support_mask=batch["support_mask"],
                targets=batch["targets"], skeleton_edges=batch["skeleton"])
    ld = crit(out, batch["targets"])
    loss = sum(ld[k] * crit.weight_dict[k] for k in ld if k in crit.weight_dict)
    loss.backward()
    named = dict(model.named_parameters(remove_duplicate=False))
    picks = ["base_model.class_embed.5.weight", "support_encoder.coord_embedding.0.weight", "support_encoder.edge_embedding.weight",
             "support_encoder.coord_edge_proj.bias", "support_encoder.norm.weight",
             "support_encoder.transformer_encoder.layers.2.linear2.bias"]
    heads = ["support_encoder.coord_edge_proj.weight", "support_encoder.transformer_encoder.layers.0.self_attn.in_proj_weight",
             "base_model.transformer.decoder.layers.5.support_attn.out_proj.weight", "base_model.input_proj.3.0.weight"]
    extra = {"grad:" + n: named[n].grad for n in picks}
    extra.update({"gradhead:" + n: named[n].grad.reshape(-1)[:256] for n in heads})
    logits = torch.stack([a["pred_logits"] for a in out["aux_outputs"]] + [out["pred_logits"]])
    ocoords = torch.stack([a["pred_coords"] for a in out["aux_outputs"]] + [out["pred_coords"]])
    # free-running decode.  Not on the batch above: its fully visible episode masks every key of that support graph, and under
    # no_grad with a mask that is not left-aligned the reference's fast path turns those rows into NaN -- its decode loop then
    # fails (math.floor(nan)).  Both episodes here keep some keypoints unmasked.
    dbatch = synth.make_batch(11, 2, 2, 64, 9, cfg, n_invisible=(2, 3))
    delta = torch.tensor([2.2, 1.9, 0.0])                          # as e2e64_decode.npz: a stream mixing <coord>/<sep>/<eos>
    with torch.no_grad():
        model.base_model.class_embed[5].bias.add_(delta)
    tok.seq_len = 40
    with torch.no_grad():
        pred = model.forward_inference(samples=dbatch["images"], support_coords=dbatch["support_coords"],
                                       support_mask=dbatch["support_mask"], skeleton_edges=dbatch["skeleton"])
    tok.seq_len = 200
    npz("legacy_e2e64.npz", logits=logits, coords=ocoords, loss=loss,
        loss_keys=jbytes(sorted(ld.keys())), loss_vals=np.array([float(ld[k]) for k in sorted(ld.keys())]),
        dec_logits=pred["logits"][:, :8], dec_coordinates=pred["coordinates"], dec_sequences=pred["sequences"], bias_delta=delta,
        **extra)


if __name__ == "__main__":
    main()

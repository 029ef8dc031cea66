"""CPU checks of `--num_feature_levels` 1, 3 and 4 (reference `roomformer_v2.py:187-214`, `backbone.py:51-54,101`): the product
constructs with the reference's parameter tree for each of them, 2 and 5 are refused at construction, and the CPU oracle
`oracle.cape_ref` at one and three levels -- a restatement of the reference with its trunk patched to hand back C5 alone for
one level, the pattern of tests/test_dilation_gpu.py -- is finite and far from the four-level oracle, so the flag matters.
No device is involved."""
import pytest
import torch

import cape_amd  # noqa: F401
from oracle import cape_ref, procweights, synth
from tests.helpers import build_product

T = "base_model.transformer."


@pytest.fixture(scope="module")
def models():
    return {L: build_product(extra=("--num_feature_levels", str(L)), device="cpu")[2] for L in (1, 3, 4)}


def test_arguments_reach_every_module(models):
    for L, model in models.items():
        base = model.base_model
        assert base.num_feature_levels == L and base.transformer.num_feature_levels == L
        assert len(base.backbone.strides) == min(L, 3) and base.backbone.num_channels == [[2048], None, [512, 1024, 2048]][min(L, 3) - 1]
        assert base.backbone[0].return_interm_layers == (L > 1)
        attn = [l.self_attn for l in base.transformer.encoder.layers] + [l.cross_attn for l in base.transformer.decoder.layers]
        assert len(attn) == 12 and all(m.n_levels == L and m.n_points == 4 for m in attn)
    assert models[1].base_model.backbone.strides == [32]
    dc5 = build_product(extra=("--num_feature_levels", "1", "--dilation"), device="cpu")[2]
    assert dc5.base_model.backbone.strides == [16] and dc5.base_model.backbone.num_channels == [2048]
    assert list(dc5.state_dict()) == list(models[1].state_dict())


@pytest.mark.parametrize("L", [2, 5])
def test_two_and_five_levels_are_refused(L):
    """2: the reference itself builds three input_proj against a two-row level_embed; 5: the MSDA kernels take four levels."""
    with pytest.raises(ValueError, match="levels"):
        build_product(extra=("--num_feature_levels", str(L)), device="cpu")


@pytest.mark.parametrize("L", [1, 3])
def test_state_dict_follows_the_level_count(models, L):
    sd, sd4 = models[L].state_dict(), models[4].state_dict()
    proj = sorted({k.split(".")[2] for k in sd if k.startswith("base_model.input_proj.")})
    assert proj == [str(l) for l in range(L)]
    for l in range(L):
        cin = 2048 if L == 1 else (512, 1024, 2048)[l]
        assert sorted(k for k in sd if k.startswith(f"base_model.input_proj.{l}.")) == \
            [f"base_model.input_proj.{l}.{j}.{leaf}" for j in (0, 1) for leaf in ("bias", "weight")]
        assert tuple(sd[f"base_model.input_proj.{l}.0.weight"].shape) == (256, cin, 1, 1)
        assert tuple(sd[f"base_model.input_proj.{l}.1.weight"].shape) == (256,)
    assert tuple(sd[T + "level_embed"].shape) == (L, 256)
    so = [k for k in sd if k.endswith("sampling_offsets.weight")]
    aw = [k for k in sd if k.endswith("attention_weights.weight")]
    assert len(so) == len(aw) == 12
    for k in so:
        assert tuple(sd[k].shape) == (64 * L, 256) and tuple(sd[k[:-6] + "bias"].shape) == (64 * L,)
    for k in aw:
        assert tuple(sd[k].shape) == (32 * L, 256) and tuple(sd[k[:-6] + "bias"].shape) == (32 * L,)
    # nothing else moves: every other key is the four-level model's, with its shape
    follows = lambda k: k.startswith("base_model.input_proj.") or k == T + "level_embed" or ".sampling_offsets." in k or ".attention_weights." in k
    assert [k for k in sd if not follows(k)] == [k for k in sd4 if not follows(k)]
    assert all(sd[k].shape == sd4[k].shape for k in sd if not follows(k))


def test_patch_2_single_level_keeps_the_1x1_projection():
    """The reference's one-level branch ignores patch_size (`roomformer_v2.py:209-214`): at --image_size 512 the projection of C5
    is still a 1x1 convolution at stride 1."""
    model = build_product(extra=("--num_feature_levels", "1", "--image_size", "512"), device="cpu")[2]
    conv = model.base_model.input_proj[0][0]
    assert tuple(conv.weight.shape) == (256, 2048, 1, 1) and conv.stride == 1 and len(model.base_model.input_proj) == 1
    three = build_product(extra=("--num_feature_levels", "3", "--image_size", "512"), device="cpu")[2]
    assert [tuple(p[0].weight.shape) for p in three.base_model.input_proj] == [(256, 512, 2, 2), (256, 1024, 2, 2), (256, 2048, 2, 2)]


def test_arena_places_offsets_and_weights_back_to_back(models):
    """runtime/arena._colocate: sampling_offsets | attention_weights are one (8 * 4L * 3, 256) operand -- 96 rows at one level,
    288 at three -- and so are their biases: every tensor in between keeps the arena's 64-element alignment."""
    from cape_amd.hip.functional import _adjacent
    from cape_amd.runtime.arena import ParamGroupArena, split_groups
    for L in (1, 3):
        model = build_product(extra=("--num_feature_levels", str(L)), device="cpu")[2]
        main, _, _ = split_groups(model)
        ParamGroupArena(main, torch.device("cpu"))
        tr = model.base_model.transformer
        for m in [l.self_attn for l in tr.encoder.layers] + [l.cross_attn for l in tr.decoder.layers]:
            assert _adjacent(m.sampling_offsets.weight, m.attention_weights.weight)
            assert _adjacent(m.sampling_offsets.bias, m.attention_weights.bias)
            assert _adjacent(m.sampling_offsets.weight.grad, m.attention_weights.weight.grad)
            assert m.sampling_offsets.weight.shape[0] + m.attention_weights.weight.shape[0] == 96 * L


def test_decode_tier_keys_on_samples_per_head(monkeypatch):
    from cape_amd.models.cached_decode import alloc_decode_workspace, decode_tier
    for k in ("CAPE_DECODE_MEGA", "CAPE_DECODE_FUSED"):
        monkeypatch.delenv(k, raising=False)
    for lp, want in ((4, "whole"), (12, "whole"), (16, "whole"), (8, "stage"), (20, "stage")):
        assert decode_tier(2, 9, lp, 1024, 1024, 84, 6, 3) == want, lp
    assert decode_tier(2, 9, 4, 1024, 1024, 4, 6, 3) == "whole"                  # S = 4: the smallest memory
    ws = alloc_decode_workspace(2, 6, 1, "cpu", 4)
    assert ws["offw"].shape == (2, 96) and ws["refin"][1].shape == (2, 1, 2)
    assert alloc_decode_workspace(2, 6, 3, "cpu", 12)["offw"].shape == (2, 288)
    assert alloc_decode_workspace(2, 6, 4, "cpu")["offw"].shape == (2, 384)


def test_oracle_at_one_and_three_levels_differs_from_four(models):
    b = synth.make_batch(11, 2, 2, 64, 9, cape_ref.Cfg(), n_invisible=(2, 0))
    plain_body = cape_ref.resnet50_body
    finals = {}
    for L in (1, 3, 4):
        spec = [(k, tuple(v.shape)) for k, v in models[L].state_dict().items()]
        sd = procweights.procedural_state_dict(spec)
        with pytest.MonkeyPatch.context() as mp, torch.no_grad():
            if L == 1:
                mp.setattr(cape_ref, "resnet50_body", lambda x, sd_, prefix="base_model.backbone.0.body.": plain_body(x, sd_, prefix)[-1:])
            out = cape_ref.cape_forward(sd, cape_ref.Cfg(num_feature_levels=L), b["images"], b["support_coords"], b["support_mask"],
                                        b["targets"], b["skeleton"], train=False, grad_mode=False)
        assert all(torch.isfinite(out[k]).all() for k in ("pred_logits", "pred_coords", "pred_room_logits"))
        finals[L] = out["pred_logits"]
    for L in (1, 3):
        diff = (finals[L] - finals[4]).abs().max().item()
        print(f"final-layer logits, {L} level(s) against 4: max difference {diff:.3f}")
        assert diff > 0.1

"""CPU checks of the reference's default support encoder (SupportPoseGraphEncoder, built without --use_geometric_encoder):
the CLI default builds it, its state_dict matches the reference's (tests/golden/state_dict_spec_legacy_diff.json, emitted by
tests/make_golden_legacy_encoder.py), and -- where the reference tree is importable -- the live reference class."""
import argparse
import inspect
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _legacy_spec():
    from oracle import procweights
    diff = json.load(open(os.path.join(GOLDEN, "state_dict_spec_legacy_diff.json")))
    removed = set(diff["removed"])
    spec = [(k, s) for k, s in procweights.load_spec() if k not in removed]
    return spec + [(k, tuple(s)) for k, s in diff["added"]], diff


def _build_default(device="cpu"):
    import cape_amd  # noqa: F401
    from cape_amd.datasets import DiscreteTokenizerV2
    from cape_amd.models import build_model
    from cape_amd.models.cape_model import build_cape_model
    from cape_amd.models.train_cape_episodic import get_args_parser
    args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args([])
    tok = DiscreteTokenizerV2(int(args.vocab_size ** 0.5), args.seq_len, add_cls=False)
    base, _ = build_model(args, tokenizer=tok)
    return args, build_cape_model(args, base)


def test_parser_default_builds_the_default_encoder():
    from cape_amd.models.support_encoder import SupportPoseGraphEncoder
    args, model = _build_default()
    assert not args.use_geometric_encoder
    assert isinstance(model.support_encoder, SupportPoseGraphEncoder)
    names = [n for n, _ in model.support_encoder.named_children()]
    assert names == ["coord_embedding", "edge_embedding", "coord_edge_proj", "pos_embedding", "transformer_encoder", "norm"]
    assert model.support_encoder.pos_embedding.dropout.p == 0.1
    assert sum(p.numel() for p in model.support_encoder.parameters()) == 2568192


def test_state_dict_matches_the_reference_spec():
    _, model = _build_default()
    spec, diff = _legacy_spec()
    sd = model.state_dict()
    assert len(sd) == 752 == diff["n_entries"]
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in spec}
    n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert n_train == 47843060 == diff["n_trainable"]
    pe = sd["support_encoder.pos_embedding.pe"]
    assert pe.shape == (1, 5000, 256) and float(pe[0, 0, 1]) == 1.0 and float(pe[0, 0, 0]) == 0.0
    # strict round trip of a procedural state_dict (the weights-only checkpoint loader does the same)
    from oracle import procweights
    proc = procweights.procedural_state_dict([(k, s) for k, s in spec if k != "support_encoder.pos_embedding.pe"
                                              and k not in procweights.KEEP_AS_BUILT])
    proc.update({k: v for k, v in sd.items() if k not in proc})
    missing, unexpected = model.load_state_dict(proc, strict=True)
    assert not missing and not unexpected


def test_signature_and_builder():
    from cape_amd.models import support_encoder as se
    sig = inspect.signature(se.SupportPoseGraphEncoder.__init__)
    assert list(sig.parameters)[1:] == ["hidden_dim", "nheads", "num_encoder_layers", "dim_feedforward", "dropout", "max_keypoints"]
    enc = se.build_support_encoder(argparse.Namespace(hidden_dim=256, nheads=8, support_encoder_layers=2, dim_feedforward=512,
                                                      dropout=0.2))
    assert len(enc.transformer_encoder.layers) == 2 and enc.transformer_encoder.layers[0].linear1.out_features == 512
    assert enc.pos_embedding.dropout.p == 0.2
    assert inspect.signature(se.PositionalEncoding1D.__init__).parameters["max_len"].default == 5000
    with pytest.raises(ValueError):
        se.SupportPoseGraphEncoder(hidden_dim=128)


def test_against_the_live_reference_class():
    from oracle import refshim
    if not refshim.reference_available():
        pytest.skip("reference tree not importable here")
    refshim.install()
    from models.support_encoder import SupportPoseGraphEncoder as Ref, PositionalEncoding1D as RefPE
    import cape_amd  # noqa: F401
    from cape_amd.models.support_encoder import SupportPoseGraphEncoder, PositionalEncoding1D
    torch.manual_seed(0)
    ref = Ref()
    mine = SupportPoseGraphEncoder()
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    assert list(ref.state_dict()) == list(mine.state_dict())
    assert torch.equal(ref.state_dict()["pos_embedding.pe"], mine.state_dict()["pos_embedding.pe"])
    assert list(inspect.signature(Ref.__init__).parameters) == list(inspect.signature(SupportPoseGraphEncoder.__init__).parameters)
    assert list(inspect.signature(RefPE.__init__).parameters) == list(inspect.signature(PositionalEncoding1D.__init__).parameters)
    assert [n for n, _ in ref.named_children()] == [n for n, _ in mine.named_children()]

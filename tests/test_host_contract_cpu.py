"""Host-side contract of the path: the episodic collate (K-shot mean-pooling, padding,
repeat per query), the PCK evaluator and the CLI flags, cross-checked against what the reference's own functions returned
on the same inputs (tests/golden/collate_ref.pth, pck_evaluator_ref.json, cli_flags_ref.json, written by
oracle/make_golden_host.py)."""
import json
import os

import numpy as np
import pytest
import torch

import cape_amd  # noqa: F401
from cape_amd.datasets import DiscreteTokenizerV2, episodic_collate_fn
from cape_amd.datasets.synthetic import SyntheticEpisodes
from cape_amd.util.eval_utils import PCKEvaluator, compute_pck_bbox
from tests.helpers import frozen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same(a, b, path=""):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a == b, path


def collate_items(n_support):
    """Four synthetic episodes with ragged keypoint counts: the inputs of collate_ref.pth."""
    tok = DiscreteTokenizerV2(44, 200)
    a = SyntheticEpisodes(tok, 4, 64, 9, 2, num_support=n_support, seed=4)
    b = SyntheticEpisodes(tok, 4, 64, 5, 2, num_support=n_support, seed=5)          # fewer keypoints: padding path
    return [a[0], b[1], a[2], b[3]]


@pytest.mark.parametrize("n_support", [1, 5])
def test_collate_matches_reference(n_support):
    """datasets/episodic_sampler.py:372-482: ragged keypoint counts across episodes, K-shot supports."""
    want = torch.load(os.path.join(GOLDEN, "collate_ref.pth"), weights_only=False)[n_support]
    _same(want, frozen(episodic_collate_fn(collate_items(n_support))))


def pck_batches():
    """Three batches of random predictions (tensors and ragged lists, visibility 0/1/2, three categories): the inputs of
    pck_evaluator_ref.json."""
    rng = np.random.Generator(np.random.PCG64(9))
    for it in range(3):
        B, P = 5, 11
        gt = torch.from_numpy(rng.random((B, P, 2)).astype(np.float32) * 200)
        pred = gt + torch.from_numpy(rng.normal(0, 25, (B, P, 2)).astype(np.float32))
        vis = torch.from_numpy(rng.integers(0, 3, (B, P)))
        bw, bh = torch.from_numpy(rng.uniform(64, 300, B).astype(np.float32)), torch.from_numpy(rng.uniform(64, 300, B).astype(np.float32))
        cats = torch.from_numpy(rng.integers(1, 4, B))
        if it == 1:       # list form with ragged lengths
            lens = [P, 7, 3, P, 9]
            yield ([pred[i, :n] for i, n in enumerate(lens)], [gt[i, :n] for i, n in enumerate(lens)], bw, bh, cats,
                   [vis[i, :n] for i, n in enumerate(lens)])
        else:
            yield (pred, gt, bw, bh, cats, vis)


def pck_summary(ev):
    """What the cross-check compares of an evaluator fed pck_batches(), in JSON types."""
    r = ev.get_results()
    return {"total_correct": int(r["total_correct"]), "total_visible": int(r["total_visible"]),
            "categories": sorted(int(c) for c in r["pck_per_category"]),
            "pck_overall": float(r["pck_overall"]), "mean_pck_categories": float(r["mean_pck_categories"]),
            "num_correct": [int(x["num_correct"]) for x in ev.image_results]}


def test_pck_evaluator_matches_reference():
    """util/eval_utils.py:29-260 on random predictions: tensors and lists, visibility 0/1/2, three categories."""
    mine = PCKEvaluator(0.2)
    for args in pck_batches():
        mine.add_batch(*args)
    rm = pck_summary(mine)
    rr = json.load(open(os.path.join(GOLDEN, "pck_evaluator_ref.json")))
    assert rm["total_correct"] == rr["total_correct"] and rm["total_visible"] == rr["total_visible"]
    assert rm["categories"] == rr["categories"]
    for k in ("pck_overall", "mean_pck_categories"):
        assert abs(rm[k] - rr[k]) < 1e-12
    assert rm["num_correct"] == rr["num_correct"]


def test_pck_edge_cases():
    """No visible keypoint -> (0.0, 0, 0); the threshold comparison is strict (util/eval_utils.py: `normalized < threshold`)."""
    gt = np.zeros((3, 2), dtype=np.float32)
    pck, c, v = compute_pck_bbox(gt + 1.0, gt, 10.0, 10.0, visibility=np.zeros(3), threshold=0.2)
    assert (pck, c, v) == (0.0, 0, 0)
    pred = np.array([[9.999, 0.0], [10.0, 0.0], [10.001, 0.0]], dtype=np.float64)          # bbox diagonal 50 -> 10 px at 0.2
    pck, c, v = compute_pck_bbox(pred, np.zeros((3, 2)), 30.0, 40.0, visibility=np.array([2, 1, 2]), threshold=0.2)
    assert (c, v) == (1, 3) and abs(pck - 1.0 / 3.0) < 1e-12


def test_optimizer_state_dict_interchanges_with_reference_adamw():
    """ArenaAdamW emits / consumes optimizer state in the id enumeration of the reference's
    `torch.optim.AdamW(param_dicts)` (train_cape_episodic.py:527-538): never-trained tensors keep an id in group 0."""
    import cape_amd  # noqa: F401
    from cape_amd.runtime.optimizer import ArenaAdamW

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(4, 6)
            self.support_attn_layer_norms = torch.nn.ModuleList([torch.nn.LayerNorm(6)])     # never receives a gradient
            self.backbone = torch.nn.Linear(6, 3)
            self.b = torch.nn.Linear(3, 2)

        def forward(self, x):
            return self.b(self.backbone(torch.relu(self.a(x))))

    def ref_opt(model):
        return torch.optim.AdamW([{"params": [p for n, p in model.named_parameters() if "backbone" not in n and p.requires_grad]},
                                  {"params": [p for n, p in model.named_parameters() if "backbone" in n and p.requires_grad],
                                   "lr": 1e-5}], lr=1e-4, weight_decay=1e-4)

    torch.manual_seed(0)
    m_ref = Toy()
    o_ref = ref_opt(m_ref)
    for i in range(2):
        o_ref.zero_grad(set_to_none=True)
        m_ref(torch.randn(5, 4)).pow(2).sum().backward()
        o_ref.step()
    sd_ref = o_ref.state_dict()
    assert [len(g["params"]) for g in sd_ref["param_groups"]] == [6, 2] and 2 not in sd_ref["state"] and 3 not in sd_ref["state"]

    m = Toy()
    m.load_state_dict(m_ref.state_dict())
    opt = ArenaAdamW(m, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4)
    opt.load_state_dict(sd_ref)
    assert int(opt.step_count) == 2
    sd = opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in sd_ref["param_groups"]]
    assert sorted(sd["state"]) == sorted(sd_ref["state"])
    for k in sd_ref["state"]:
        for f in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][k][f], sd_ref["state"][k][f]), (k, f)
        assert float(sd["state"][k]["step"]) == float(sd_ref["state"][k]["step"])
    assert sd["param_groups"][1]["lr"] == 1e-5
    # and back: the reference optimizer accepts what ArenaAdamW wrote
    o2 = ref_opt(Toy())
    o2.load_state_dict(sd)
    assert torch.equal(o2.state_dict()["state"][0]["exp_avg"], sd_ref["state"][0]["exp_avg"])
    # a foreign layout is rejected before anything is copied
    bad = {"state": dict(sd_ref["state"]), "param_groups": [dict(sd_ref["param_groups"][0], params=list(range(4))),
                                                             dict(sd_ref["param_groups"][1], params=[4, 5])]}
    before = opt.arenas[0].exp_avg.clone()
    with pytest.raises(ValueError):
        opt.load_state_dict(bad)
    bad2 = {"state": {k: dict(v) for k, v in sd_ref["state"].items()}, "param_groups": sd_ref["param_groups"]}
    bad2["state"][5]["exp_avg"] = torch.zeros(7)
    with pytest.raises(ValueError):
        opt.load_state_dict(bad2)
    assert torch.equal(opt.arenas[0].exp_avg, before)


def cli_flag_table(parser):
    """dest -> [option strings, action class, default, type name, choices, nargs], in JSON types (the form of
    cli_flags_ref.json)."""
    import argparse
    out = {}
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        out[a.dest] = (tuple(a.option_strings), type(a).__name__, a.default, getattr(a.type, "__name__", a.type),
                       tuple(a.choices) if a.choices else None, a.nargs)
    return json.loads(json.dumps(out))


def test_cli_parser_matches_reference_flag_by_flag():
    """`get_args_parser()` exposes the reference's flags with the same defaults / types / choices
    (`models/train_cape_episodic.py:86-254`); only `--dataset_root`'s author-specific default path and the added
    `synthetic` dataset name may differ."""
    from cape_amd.models.train_cape_episodic import get_args_parser
    t_ref = json.load(open(os.path.join(GOLDEN, "cli_flags_ref.json")))
    t_ours = cli_flag_table(get_args_parser())
    assert set(t_ref) <= set(t_ours), f"flags missing here: {sorted(set(t_ref) - set(t_ours))}"
    allowed_default_diff = {"dataset_root"}
    for k, v in t_ref.items():
        o = t_ours[k]
        assert o[0] == v[0] and o[1] == v[1] and o[3] == v[3] and o[5] == v[5], (k, v, o)
        if k not in allowed_default_diff:
            assert o[2] == v[2], (k, v[2], o[2])
        if v[4] is not None:
            assert set(v[4]) <= set(o[4] or ()), (k, v[4], o[4])

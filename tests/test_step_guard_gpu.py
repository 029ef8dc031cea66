"""The device-side loss guard (csrc/optim.hip: cape_step_guard, cape_adamw_step_guarded), the guarded ArenaAdamW, the graphed
training loop of models/engine_cape.py with gradient accumulation, its non-finite stop, and the CLI behind CAPE_GRAPH_STEP=1."""
import argparse
import glob
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 1003                                                    # not a multiple of 4


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
def _arena(seed):
    g = torch.Generator().manual_seed(seed)
    p, gr, m = (torch.randn(N, generator=g).to(DEV) for _ in range(3))
    v = torch.rand(N, generator=g).to(DEV) * 1e-2
    return p, gr * 0.05, m * 0.01, v


@pytest.mark.parametrize("max_norm", [0.0, 0.1])
def test_guarded_adamw_bitwise_and_skip(max_norm):
    import cape_amd  # noqa: F401
    from cape_amd.hip import lib, ops
    p, g, m, v = _arena(1)
    sumsq = torch.zeros(2 * lib.SUMSQ_PARTS, device=DEV)
    ops.sumsq(g, sumsq[:lib.SUMSQ_PARTS])
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    lr_dev = torch.tensor([2e-4], device=DEV)
    if max_norm > 0:
        assert float(sumsq.sum().sqrt()) > max_norm         # the clip coefficient is at work
    hyper = (1e-4, 0.9, 0.999, 1e-8, 1e-2, max_norm, sumsq, step)
    ref = [t.clone() for t in (p, m, v)]
    ops.adamw_step(ref[0], g, ref[1], ref[2], *hyper, lr_dev=lr_dev)
    assert not torch.equal(ref[0], p)
    for bad_word, want in ((0, ref), (1, [p.clone(), m.clone(), v.clone()]), (-7, [p.clone(), m.clone(), v.clone()])):
        got = [t.clone() for t in (p, m, v)]
        bad = torch.tensor([bad_word], dtype=torch.int32, device=DEV)
        ops.adamw_step_guarded(got[0], g, got[1], got[2], *hyper, bad, lr_dev=lr_dev)
        for a, b in zip(got, want):
            assert torch.equal(a, b), bad_word
        assert int(bad) == bad_word and int(step) == 3      # the AdamW kernel reads both, writes neither


def _guard_state(ring_len=4, n_losses=12, step0=3):
    from cape_amd.hip import lib
    return dict(step=torch.tensor([step0], dtype=torch.int64, device=DEV), state=torch.zeros(2, dtype=torch.int32, device=DEV),
                ring=torch.full((ring_len, lib.GUARD_ROW_LOSSES + n_losses + 1), -5.0, device=DEV),
                lr=torch.tensor([3e-5, 7.0], device=DEV))


def _launch(s, total, losses, parts, max_norm=0.1, ring=True):
    from cape_amd.hip import ops
    ops.step_guard(total, losses, parts, max_norm, s["lr"][0:1], s["step"], s["state"][0:1], s["state"][1:2],
                   s["ring"] if ring else None)
    torch.cuda.synchronize()
    return s["ring"].cpu(), [int(x) for x in s["state"].cpu()], int(s["step"])


def test_step_guard_rows_flag_and_counter():
    import cape_amd  # noqa: F401
    from cape_amd.hip import lib
    g = torch.Generator().manual_seed(2)
    losses = torch.rand(12, generator=g).to(DEV)
    total = torch.tensor([4.25], device=DEV)
    parts = torch.rand(2 * lib.SUMSQ_PARTS, generator=g).to(DEV) * 3e-4
    s = _guard_state()
    S, OK, TOT, NORM, COEF, LR, L0 = (lib.GUARD_ROW_SERIAL, lib.GUARD_ROW_OK, lib.GUARD_ROW_TOTAL, lib.GUARD_ROW_NORM,
                                      lib.GUARD_ROW_COEF, lib.GUARD_ROW_LR, lib.GUARD_ROW_LOSSES)

    def ints(row):
        return row.view(torch.int32)

    # launch 0: a clean optimizer step
    ring, (serial, bad), step = _launch(s, total, losses, parts)
    row = ring[0]
    want_norm = math.sqrt(float(parts.cpu().double().sum()))
    assert (int(ints(row)[S]), int(ints(row)[OK])) == (0, 1) and (serial, bad, step) == (1, 0, 4)
    assert float(row[TOT]) == 4.25 and torch.equal(row[L0:L0 + 12], losses.cpu()) and float(row[LR]) == float(s["lr"][0])
    assert abs(float(row[NORM]) - want_norm) <= 1e-6 * want_norm
    assert want_norm > 0.1                                  # the coefficient below is a real clip
    want_coef = np.float32(0.1) / (np.float32(row[NORM]) + np.float32(1e-6))
    assert abs(float(row[COEF]) - float(want_coef)) <= 1e-6 * float(want_coef) and float(row[COEF]) < 1.0
    assert float(row[L0 + 12]) == -5.0 and bool((ring[1:] == -5.0).all())      # nothing beyond the row's own fields
    # launch 1: a micro-batch -- "no step" marker, counter untouched
    ring, (serial, bad), step = _launch(s, total, losses, None)
    row = ring[1]
    assert (int(ints(row)[S]), int(ints(row)[OK])) == (1, 1) and (serial, bad, step) == (2, 0, 4)
    assert float(row[NORM]) == lib.GUARD_NO_STEP and float(row[COEF]) == 1.0 and float(row[TOT]) == 4.25
    # launch 2: no clipping -> coefficient 1, the norm is reported all the same
    ring, (serial, bad), step = _launch(s, total, losses, parts, max_norm=0.0)
    assert float(ring[2][COEF]) == 1.0 and abs(float(ring[2][NORM]) - want_norm) <= 1e-6 * want_norm and step == 5
    # launch 3: an optimizer step with no forward before it (no ring): counted, no row, serial stays
    ring, (serial, bad), step = _launch(s, None, None, parts, ring=False)
    assert (serial, bad, step) == (3, 0, 6) and bool((ring[3] == -5.0).all())
    # launch 4: non-finite total -> sticky flag, step not counted
    ring, (serial, bad), step = _launch(s, torch.tensor([float("inf")], device=DEV), losses, parts)
    assert (int(ints(ring[3])[S]), int(ints(ring[3])[OK])) == (3, 0) and (serial, bad, step) == (4, 1, 6)
    assert math.isinf(float(ring[3][TOT]))
    # launch 5: clean inputs, the flag stays; the ring wraps (serial 4 -> row 0)
    ring, (serial, bad), step = _launch(s, total, losses, parts)
    assert (int(ints(ring[0])[S]), int(ints(ring[0])[OK])) == (4, 0) and (serial, bad, step) == (5, 1, 6)
    # a micro-batch with a NaN total raises the flag too
    s = _guard_state()
    ring, (serial, bad), step = _launch(s, torch.tensor([float("nan")], device=DEV), losses, None)
    assert (serial, bad, step) == (1, 1, 3) and int(ints(ring[0])[OK]) == 0


@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
def test_step_guard_non_finite_partial_sum(poison):
    import cape_amd  # noqa: F401
    from cape_amd.hip import lib
    parts = torch.full((2 * lib.SUMSQ_PARTS,), 1e-4, device=DEV)
    parts[lib.SUMSQ_PARTS + 77] = poison
    s = _guard_state()
    ring, (serial, bad), step = _launch(s, torch.tensor([1.5], device=DEV), torch.zeros(12, device=DEV), parts)
    assert (serial, bad, step) == (1, 1, 3) and int(ring[0].view(torch.int32)[lib.GUARD_ROW_OK]) == 0
    assert not math.isfinite(float(ring[0][lib.GUARD_ROW_NORM]))
    ring, (serial, bad), step = _launch(s, torch.tensor([1.5], device=DEV), torch.zeros(12, device=DEV),
                                        torch.full_like(parts, 1e-4))
    assert (serial, bad, step) == (2, 1, 3) and int(ring[1].view(torch.int32)[lib.GUARD_ROW_OK]) == 0


# ------------------------------------------------------------------------------------------------
# the training loop
# ------------------------------------------------------------------------------------------------
def _setup(n_batches):
    import cape_amd  # noqa: F401
    from cape_amd.datasets import DiscreteTokenizerV2, episodic_collate_fn
    from cape_amd.datasets.synthetic import SyntheticEpisodes
    from cape_amd.models.train_cape_episodic import get_args_parser
    args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(
        ["--use_geometric_encoder", "--use_gcn_preenc", "--image_size", "64"])
    tok = DiscreteTokenizerV2(44, args.seq_len)
    ds = SyntheticEpisodes(tok, 2 * n_batches, 64, 17, 2, seed=5)
    batches = [episodic_collate_fn([ds[2 * i], ds[2 * i + 1]]) for i in range(n_batches)]     # 2 episodes x 2 queries = 4 images
    return args, tok, batches


def _build(args, tok, graphed, accumulation_steps):
    from cape_amd.hip import functional as HF
    from cape_amd.hip import ops
    from cape_amd.models import build_model
    from cape_amd.models.cape_model import build_cape_model
    from cape_amd.runtime.graph_step import GraphedTrainStep
    from cape_amd.runtime.optimizer import ArenaAdamW
    from cape_amd.runtime.step_guard import StepGuard
    torch.manual_seed(0)
    ops._stream_counter[0] = 0                              # dropout stream ids are handed out at construction
    base, crit = build_model(args, tokenizer=tok)
    model = build_cape_model(args, base).to(DEV)
    crit = crit.to(DEV)
    HF.Runtime.seed(77, DEV)
    opt = ArenaAdamW(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4, max_norm=0.1, guard=StepGuard(DEV) if graphed else None)
    step = GraphedTrainStep(model, crit, opt, edge_capacity=512, eager_steps=1,
                            accumulation_steps=accumulation_steps) if graphed else None
    return model, crit, opt, step


def test_graphed_epoch_with_accumulation_matches_eager_epoch(monkeypatch):
    """7 batches, 2 accumulation steps: micro-batch and boundary captures are both replayed, the epoch ends with one pending
    micro-batch (tail flush), 4 optimizer steps.  Two executions of the same mathematics: no atomic k-splits (see
    test_e2e_gpu.py::test_graphed_train_step_matches_eager, whose tolerances these are)."""
    import cape_amd  # noqa: F401
    from cape_amd.hip import functional as HF
    from cape_amd.models.engine_cape import train_one_epoch_episodic
    monkeypatch.setattr(HF, "_DETERMINISTIC", True)
    args, tok, batches = _setup(7)
    steps, lr = 4, 1e-4

    def run(graphed):
        model, crit, opt, step = _build(args, tok, graphed, 2)
        log = []
        if graphed:
            rd = step.reader
            poll, drain = rd.poll, rd.drain

            def logged_poll():
                rows = poll()
                log.append((rd.next_serial - 1, [r.serial for r in rows]))       # (iteration just enqueued, serials handed out)
                return rows

            def logged_drain():
                rows = drain()
                log.append(("drain", [r.serial for r in rows]))
                return rows
            monkeypatch.setattr(rd, "poll", logged_poll)
            monkeypatch.setattr(rd, "drain", logged_drain)
        stats = train_one_epoch_episodic(model, crit, batches, opt, torch.device(DEV), 0, max_norm=0.1, print_freq=0,
                                         accumulation_steps=2, graph_step=step)
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().reshape(-1)[:64] for p in model.parameters() if p.requires_grad][:40])
        return stats, flat, int(opt.step_count), step, log, opt

    se, pe, ne, _, _, _ = run(False)
    sg, pg, ng, step, log, opt = run(True)
    print("eager stats", se, "\ngraphed stats", sg)
    d = (pe - pg).abs()
    print("parameters: worst", d.max().item(), "mean", d.mean().item())
    assert ne == ng == steps
    assert len(step.cache) == 2 and sorted(k[-2] for k in step.cache) == [False, True]       # one micro-batch, one boundary capture
    # the row of iteration i arrives at iteration i + 1 and carries serial i; the drain returns the last one
    assert log == [(0, [])] + [(i, [i - 1]) for i in range(1, 7)] + [("drain", [6])], log
    assert set(se) == set(sg)
    for k in se:
        assert abs(se[k] - sg[k]) <= 2e-4 * max(1.0, abs(se[k])), (k, se[k], sg[k])
    assert d.max().item() <= 1.2 * steps * lr and d.mean().item() <= 5e-6, (d.max().item(), d.mean().item())
    # the guarded step keeps grad_norm() current (the flush was the last step: gradients of one micro-batch at half weight)
    assert math.isfinite(float(opt.grad_norm())) and float(opt.grad_norm()) > 0
    assert not step.guard.is_bad()
    for a in opt.arenas:
        assert not a.grad.any()


def test_graphed_loop_stops_one_iteration_after_a_non_finite_loss(capsys):
    """Iteration 3 (a replayed step) sees a non-finite loss through a quantity only the criterion reads: the device skips that
    step and the next, the host exits in iteration 4 with the parameters of iteration 2."""
    import cape_amd  # noqa: F401
    from cape_amd.models.engine_cape import train_one_epoch_episodic
    args, tok, batches = _setup(6)
    tg = batches[3]["query_targets"]
    vis = tg["visibility_mask"].bool() if "visibility_mask" in tg else torch.ones_like(tg["token_labels"], dtype=torch.bool)
    b, t = torch.nonzero((tg["token_labels"] == 0) & vis)[0].tolist()      # a visible <coord> token: its L1 term is in the loss
    tg["target_seq"][b, t, 0] = float("inf")
    model, crit, opt, step = _build(args, tok, True, 1)
    seen, snap = [], {}

    def loader():
        for i, bt in enumerate(batches):
            if i == 3:                                      # stream-ordered behind iteration 2: the last step before the bad batch
                snap["arenas"] = [(a.data.clone(), a.exp_avg.clone(), a.exp_avg_sq.clone()) for a in opt.arenas]
            seen.append(i)
            yield bt

    with pytest.raises(SystemExit) as ei:
        train_one_epoch_episodic(model, crit, loader(), opt, torch.device(DEV), 0, max_norm=0.1, print_freq=0,
                                 accumulation_steps=1, graph_step=step)
    assert ei.value.code == 1
    assert seen == [0, 1, 2, 3, 4]                          # raised in iteration 4, one after the bad one
    out = capsys.readouterr().out
    assert "Loss is inf, stopping training" in out, out    # what the eager loop prints
    torch.cuda.synchronize()
    assert len(step.cache) == 1                             # iterations 1.. are one capture: iteration 3 was a replay
    assert int(opt.step_count) == 3 and step.guard.is_bad()
    for a, (p0, m0, v0) in zip(opt.arenas, snap["arenas"]):
        assert torch.equal(a.data, p0) and torch.equal(a.exp_avg, m0) and torch.equal(a.exp_avg_sq, v0)
        assert not a.grad.any()


# ------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------
def test_train_cli_with_graph_step_switch(tmp_path, monkeypatch, capsys):
    import cape_amd  # noqa: F401
    from cape_amd.models.train_cape_episodic import get_args_parser, main
    from cape_amd.util.checkpoint import load_checkpoint
    monkeypatch.setenv("CAPE_GRAPH_STEP", "1")
    monkeypatch.setenv("WARN_INCOMPLETE_GENERATION", "0")
    base = ["--use_geometric_encoder", "--use_gcn_preenc", "--dataset_name", "synthetic", "--image_size", "64", "--batch_size", "2",
            "--episodes_per_epoch", "12", "--accumulation_steps", "2", "--num_workers", "0", "--val_episodes_per_epoch", "2",
            "--output_dir", str(tmp_path), "--print_freq", "0"]
    parse = lambda extra: argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(base + extra)
    hist = main(parse(["--epochs", "2"]))
    assert "CAPE_GRAPH_STEP=1" in capsys.readouterr().out
    assert len(hist) == 2
    for h in hist:
        assert math.isfinite(h["train"]["loss"]) and h["train"]["loss"] > 0 and 0 < h["train"]["lr"] <= 1e-4 * (1 + 1e-6)
        assert 0.0 <= h["val"]["pck"] <= 1.0
    cks = sorted(glob.glob(str(tmp_path / "checkpoint_e*.pth")))
    assert [os.path.basename(c) for c in cks] == ["checkpoint_e000_lr1e-04_bs2_acc2_qpe2.pth", "checkpoint_e001_lr1e-04_bs2_acc2_qpe2.pth"]
    ck0, ck1 = load_checkpoint(cks[0]), load_checkpoint(cks[1])
    assert ck0["epoch"] == 0 and ck1["epoch"] == 1 and math.isfinite(ck1["train_stats"]["loss"])
    steps = lambda ck: int(float(next(iter(ck["optimizer"]["state"].values()))["step"]))
    assert steps(ck0) == 3 and steps(ck1) == 6              # 6 iterations per epoch, 2 accumulation steps, none skipped
    # resume from the first checkpoint: the second epoch again, from the restored optimizer state and step count
    os.remove(cks[1])
    hist2 = main(parse(["--epochs", "2", "--resume", cks[0]]))
    assert [h["epoch"] for h in hist2] == [1] and math.isfinite(hist2[0]["train"]["loss"])
    assert steps(load_checkpoint(cks[1])) == 6

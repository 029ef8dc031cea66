"""What does the captured training step (CAPE_GRAPH_STEP=1) buy the path a user runs?  `run_training` -- the body of the training
CLI -- on synthetic episodes at the headline workload (16 episodes x 2 queries per batch, 256 x 256, default loader settings),
one epoch, switch off and switch on, alternating, each run in a fresh child process; prints the `episodes_per_s` that
`run_training` records in its history, their medians and the acceptance comparison:

    median(on) >= median(off) - (max(off) - min(off))

    python tools/cli_bench.py                   # 3 runs each, 48 iterations per run
    python tools/cli_bench.py --runs 1 --iterations 24

The epoch includes the eager warm-up calls and the captures of the switched-on run (2 + 1 calls per capture kind)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "CLI_BENCH_RESULT "


def child(a):
    sys.path.insert(0, ROOT)
    import cape_amd  # noqa: F401
    from cape_amd.models.train_cape_episodic import get_args_parser, main
    os.environ["WARN_INCOMPLETE_GENERATION"] = "0"
    with tempfile.TemporaryDirectory() as out:
        args = argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(
            ["--use_geometric_encoder", "--use_gcn_preenc", "--dataset_name", "synthetic", "--batch_size", "16",
             "--num_queries_per_episode", "2", "--image_size", "256", "--episodes_per_epoch", str(16 * a.iterations),
             "--accumulation_steps", str(a.accumulation_steps), "--val_episodes_per_epoch", "1", "--epochs", "1",
             "--print_freq", "0", "--output_dir", out])
        hist = main(args)
    print(TAG + json.dumps({"graph_step": os.environ.get("CAPE_GRAPH_STEP", "0"), "episodes_per_s": hist[0]["episodes_per_s"],
                            "train_loss": hist[0]["train"]["loss"]}), flush=True)


def run_child(a, switch):
    env = dict(os.environ, CAPE_GRAPH_STEP="1" if switch else "0")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iterations", str(a.iterations),
           "--accumulation_steps", str(a.accumulation_steps)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
    if p.returncode != 0 or not lines:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child run (CAPE_GRAPH_STEP={int(switch)}) failed with status {p.returncode}")
    return json.loads(lines[-1][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=48, help="batches per epoch (>= 20 of them replayed with the switch on)")
    ap.add_argument("--accumulation_steps", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=500, help="seconds per child run")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {0: [], 1: []}
    print(f"run_training, synthetic, 16 episodes x 2 queries, 256 x 256, {a.iterations} iterations, "
          f"accumulation_steps {a.accumulation_steps}, default loader")
    for r in range(a.runs):
        for switch in (0, 1):
            out = run_child(a, switch)
            res[switch].append(out["episodes_per_s"])
            print(f"run {r}  CAPE_GRAPH_STEP={switch}  {out['episodes_per_s']:8.2f} episodes/s  train loss {out['train_loss']:.4f}", flush=True)
    off, on = res[0], res[1]
    spread = max(off) - min(off)
    m_off, m_on = statistics.median(off), statistics.median(on)
    print(f"switch off: median {m_off:.2f} episodes/s (spread {spread:.2f});  switch on: median {m_on:.2f} episodes/s")
    print(f"acceptance (median on >= median off - spread off): {m_on:.2f} >= {m_off - spread:.2f}: "
          f"{'met' if m_on >= m_off - spread else 'NOT met'}")


if __name__ == "__main__":
    main()

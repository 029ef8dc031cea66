"""TEST INFRASTRUCTURE ONLY -- the host-contract fixtures, from the REAL reference (build container only; the reference is
imported in place through oracle/refshim.py, nothing is copied).  Fixtures are data: the reference's outputs on inputs that the
tests rebuild from seeds.  Re-run:  python -m oracle.make_golden_host

  collate_ref.pth          datasets/episodic_sampler.py `episodic_collate_fn` on tests/test_host_contract_cpu.collate_items(1 | 5)
  pck_evaluator_ref.json   util/eval_utils.py `PCKEvaluator(0.2)` fed tests/test_host_contract_cpu.pck_batches()
  cli_flags_ref.json       models/train_cape_episodic.py `get_args_parser()`, flag by flag
  mp100_records_ref.pth    datasets/mp100_cape.py `MP100CAPE` + datasets/episodic_sampler.py `EpisodicDataset` on the file set of
                           tests/test_data_path_cpu.make_dataset (this package's pure-Python COCO reader standing in for
                           pycocotools): every record, then five fixed episodes

Tensors of more than 4096 elements (the images) are stored as sha256 digests of their bytes (tests/helpers.frozen).
"""
import importlib
import json
import os
import sys
import tempfile
import warnings
from pathlib import Path

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import refshim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
warnings.filterwarnings("ignore")


def main():
    import cape_amd  # noqa: F401
    from cape_amd.datasets.coco_lite import COCO
    from tests.helpers import frozen
    from tests.test_data_path_cpu import make_dataset, records_and_episodes
    from tests.test_host_contract_cpu import cli_flag_table, collate_items, pck_batches, pck_summary
    refshim.install()
    collate = importlib.import_module("datasets.episodic_sampler").episodic_collate_fn
    torch.save({n: frozen(collate(collate_items(n))) for n in (1, 5)}, os.path.join(OUT, "collate_ref.pth"))

    ev = importlib.import_module("util.eval_utils").PCKEvaluator(0.2)
    for args in pck_batches():
        ev.add_batch(*args)
    with open(os.path.join(OUT, "pck_evaluator_ref.json"), "w") as f:
        json.dump(pck_summary(ev), f, indent=1)

    parser = importlib.import_module("models.train_cape_episodic").get_args_parser()
    with open(os.path.join(OUT, "cli_flags_ref.json"), "w") as f:
        json.dump(cli_flag_table(parser), f, indent=1)

    m = importlib.import_module("datasets.mp100_cape")
    m.COCO = COCO
    s = importlib.import_module("datasets.episodic_sampler")
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        out = records_and_episodes(root, make_dataset(root), m.MP100CAPE, s.EpisodicDataset, m.ImageNotFoundError)
    torch.save(out, os.path.join(OUT, "mp100_records_ref.pth"))
    for name in ("collate_ref.pth", "pck_evaluator_ref.json", "cli_flags_ref.json", "mp100_records_ref.pth"):
        print("wrote", name, os.path.getsize(os.path.join(OUT, name)), "bytes")


if __name__ == "__main__":
    main()

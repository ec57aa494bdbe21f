"""Generate tests/golden/full_swin_large.pt from the REFERENCE's own modules (needs the reference tree, oracle/ref_loader.py):

    python tools/gen_swin_large_golden.py

Swin-L built from experiments/imagenet/swin/swin_large_patch4_window7_224.yaml, one step by the recipe of
oracle.gen_golden._full_cfg_case (2 x 224^2 + 8 x 96^2 crops, V+R heads, DDINOLoss, B = 2, out_dim 8192): the contents per case of
tests/golden/full_configs.pt.  The case table is tests/swin_large_ref.py.  About two and a half minutes and 7 GB on the CPU."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as RL  # noqa: E402
from oracle.gen_golden import OUT, _full_cfg_case  # noqa: E402
from tests import swin_large_ref as SL  # noqa: E402


def main():
    ns = RL.load()
    RL.ensure_single_process_group()
    torch.save({name: _full_cfg_case(ns, name, c) for name, c in SL.CASES.items()}, SL.GOLD)
    assert os.path.dirname(SL.GOLD) == OUT
    print("full_swin_large.pt:", os.path.getsize(SL.GOLD), "bytes")


if __name__ == "__main__":
    main()

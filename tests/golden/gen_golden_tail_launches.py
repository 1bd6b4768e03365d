#!/usr/bin/env python3
"""Generate tests/golden/tail_launches.json: per case of tests/test_tail_launches_gpu.py the kernel names one eager step
launches, in order.  Needs an MI355X and the built library; run it on the tree whose launches are to be kept:

    python tests/golden/gen_golden_tail_launches.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_tail_launches_gpu as t  # noqa: E402

with open(os.path.join(HERE, "tail_launches.json"), "w", encoding="utf-8") as fh:
    json.dump({case_id: t.record(case_id)[0] for case_id in t.CASES}, fh, indent=0, sort_keys=True)
    fh.write("\n")

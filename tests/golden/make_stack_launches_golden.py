"""Writes stack_launches.json: the library entries one eager training step calls, per case of helpers/stack_cases.py, in
the tree this runs in (needs the GPU).  The committed lists were recorded on the commit before stack_plan.py existed, and
tests/test_stack_plan.py holds every later commit to them; run this only for a change that means to move a launch.

    python tests/golden/make_stack_launches_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "helpers")]

import stack_cases as SC  # noqa: E402

if __name__ == "__main__":
    lists = {cid: SC.run_case(case)[1] for cid, case in SC.CASES.items()}
    with open(os.path.join(HERE, "stack_launches.json"), "w") as fh:
        json.dump(lists, fh, indent=0)
        fh.write("\n")
    print({cid: len(v) for cid, v in lists.items()})

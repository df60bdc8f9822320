#!/usr/bin/env python3
"""Writes tests/golden/tile_plan_digests.json: a SHA-256 per plan of the cases in tests/_plan_digests.py.

The fixture pins the planner's output byte for byte ACROSS a change of csrc/host/tile_plan.cpp, so it is written from the
host library of the commit before the change, never from the changed code:

    git stash / git worktree at the parent commit, build its libt8gpu_host.so, then
    T8GPU_HOST_LIB=/path/to/parent/libt8gpu_host.so python tests/golden/make_tile_plan_digests.py

(T8GPU_HOST_LIB is the library override of t8gpu_amd/synth.py; without it the tree's own library is used, which is only
right when a NEW case is added on an unchanged planner.) A change that alters a plan on purpose regenerates the file
from its own library and says so in its commit message.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import _plan_digests as D  # noqa: E402

if __name__ == "__main__":
    digests = {}
    for name in D.CASES:
        digests.update(D.case_digests(name))
    with open(os.path.join(HERE, "tile_plan_digests.json"), "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} plan digests written")

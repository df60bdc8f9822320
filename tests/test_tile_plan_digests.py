"""The tile planner's output, byte for byte: a SHA-256 over every array and scalar of a plan against
tests/golden/tile_plan_digests.json, which tests/golden/make_tile_plan_digests.py wrote from the library of the commit
before the planner was last restructured. Host only."""
import json
import os
import subprocess
import sys

import pytest

import _plan_digests as D

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "tile_plan_digests.json")) as f:
    GOLDEN = json.load(f)


def test_fixture_lists_every_plan_of_every_case():
    assert sorted(GOLDEN) == sorted(f"{name}/rank{rk}" for name, (_, ranks, _) in D.CASES.items() for rk in range(ranks))


@pytest.mark.parametrize("name", list(D.CASES))
def test_plan_bytes_are_those_of_the_fixture(name):
    got = D.case_digests(name)
    assert got == {k: GOLDEN[k] for k in got}


@pytest.mark.parametrize("threads", [1, 4])
def test_plan_bytes_do_not_depend_on_the_thread_count(threads):
    """host_threads() is latched on first use: a fresh child process per thread count (host library only, no GPU)."""
    code = (f"import sys, json; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import _plan_digests as D; "
            f"print(json.dumps(D.case_digests({D.THREADS_CASE!r})))")
    env = dict(os.environ, T8GPU_HOST_THREADS=str(threads))
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert got and got == {k: GOLDEN[k] for k in got}

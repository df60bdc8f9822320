"""t8gpu::hip::Monitor of include/t8gpu/backend/hip_fast.h: tests/compat/monitor_api.hip instantiates run<float> and
run<double> (CPU check: it compiles for gfx950) and, on the GPU box, compares the block with a host loop."""
import subprocess

import pytest

from test_headers import compile_example


def test_monitor_class_compiles():
    compile_example("monitor_api.hip", "monitor_api")


@pytest.mark.gpu
def test_monitor_class_runs():
    exe = compile_example("monitor_api.hip", "monitor_api")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "monitor_api OK" in res.stdout, res.stdout + res.stderr

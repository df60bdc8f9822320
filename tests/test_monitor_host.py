"""The state monitor's host side, without a GPU: the library exports the C entries, and Monitor.combine merges ranks' blocks."""
import ctypes

import numpy as np

from t8gpu_amd import build


def test_library_exports_the_state_monitor():
    lib = ctypes.CDLL(build.build_hip())
    for name in ("t8gpu_hip_state_monitor_f32", "t8gpu_hip_state_monitor_f64", "t8gpu_hip_state_monitor_workspace_bytes"):
        assert hasattr(lib, name), name
    f = lib.t8gpu_hip_state_monitor_workspace_bytes
    f.restype = ctypes.c_size_t
    assert f() >= 128 and f() % (16 * 8) == 0          # 16 slots x grid cap x 8 bytes


def test_invalid_arguments_are_refused_before_any_launch():
    """null workspace / result, cells_per_element < 1, dim outside {2, 3}: hipErrorInvalidValue (1), checked on the host"""
    lib = ctypes.CDLL(build.build_hip())

    class Vars(ctypes.Structure):
        _fields_ = [("p", ctypes.c_void_p * 5)]

    f = lib.t8gpu_hip_state_monitor_f64
    f.restype = ctypes.c_int
    buf = ctypes.c_void_p(4096)                         # (never dereferenced: every call below is refused)
    args = lambda cpe, dim, ws, res: (ctypes.c_size_t(0), cpe, dim, Vars(), None, ws, res, None)
    assert f(*args(1, 2, None, buf)) == 1
    assert f(*args(1, 2, buf, None)) == 1
    assert f(*args(0, 2, buf, buf)) == 1
    assert f(*args(1, 1, buf, buf)) == 1
    assert f(*args(1, 4, buf, buf)) == 1


def test_combine_sums_maxima_and_minima_per_slot_class():
    from t8gpu_amd.solver import Monitor
    a = np.array([1.0, 2.0, -3.0, 4.0, 5.0, 6.0, -7.0, 1.5, 80.0, 0.9, 0.7, 1.0, 0.0, 0.0, 0.0, 0.0])
    b = np.array([10.0, 20.0, 30.0, -40.0, 50.0, 60.0, 70.0, 2.5, 40.0, 0.5, 0.8, 0.0, 2.0, 0.0, 0.0, 0.0])
    empty = np.zeros(16)
    empty[9:11] = np.inf                                # a rank that owns nothing
    m = Monitor.combine([a, Monitor(b), empty])
    assert m.block.shape == (16,)
    assert np.array_equal(m.integrals, [11.0, 22.0, 27.0, -36.0, 55.0])
    assert (m.kinetic_energy, m.entropy) == (66.0, 63.0)
    assert (m.max_speed, m.max_rate) == (2.5, 80.0)
    assert (m.min_density, m.min_pressure) == (0.5, 0.7)
    assert (m.nonfinite, m.unphysical) == (1, 2)
    assert np.array_equal(m.block[13:], [0.0, 0.0, 0.0])
    only_empty = Monitor.combine([empty, empty])
    assert np.isposinf(only_empty.min_density) and np.isposinf(only_empty.min_pressure) and only_empty.max_rate == 0.0
    assert np.array_equal(Monitor.combine([a]).block, a)

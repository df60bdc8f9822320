"""Access to tests/golden/reference_kernel_vectors.npz (inputs and outputs of the reference's own kernel bodies, executed on
tiny AMR meshes: tests/golden/make_reference_kernel_vectors.py) for the tests that consume it: the CPU oracle
(test_oracle_reference_kernels.py), the planner's view of the fixture meshes (test_kernel_vector_plans.py) and the HIP tiers
(test_gpu_reference_kernels.py). Needs no GPU."""
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "reference_kernel_vectors.npz")
KEPES = 0                               # the only flux the fixture holds
TAGS = ("f64", "f32")

_cache = {}


def vectors():
    if "z" not in _cache:
        _cache["z"] = np.load(PATH, allow_pickle=False)
    return _cache["z"]


def case_names():
    return sorted({k.split("|")[0] for k in vectors().files if "|" in k})


def plain_cases():
    return [c for c in case_names() if c.startswith("plain")]


def subgrid_cases():
    return [c for c in case_names() if c.startswith("sub")]


def load(case, tag):
    z = vectors()
    ins = {k.split("|")[3]: z[k] for k in z.files if k.startswith(f"{case}|{tag}|in|")}
    outs = {k.split("|")[3]: z[k] for k in z.files if k.startswith(f"{case}|{tag}|out|")}
    return ins, outs


def case_dim(case, ins):
    """2 or 3: the fixture's rank for Subgrid cases, the case name's for plain ones (their normals have three components in
    both)"""
    rank = int(ins["rank"][0])
    if rank:
        return rank
    return {"plain2d": 2, "plain3d": 3}[case.split("_")[0]]


class FixturePartition:
    """One fixture case as a partition: the reference's array format one to one, in the attribute names the host planners
    and the solvers read (as synth.Partition and unstructured.UnstructuredPartition have them). No `boundary_kinds`: every
    boundary face of the fixture is a wall."""

    def __init__(self, case, ins):
        self.N, self.G, self.F, self.B, self.stride = (int(x) for x in ins["sizes"])
        self.normal_dim = int(ins["normal_dim"][0])
        self.face_neighbors = np.ascontiguousarray(ins["fn"], np.int32)
        self.normals = np.ascontiguousarray(ins["normals"], np.float64)
        self.areas = np.ascontiguousarray(ins["areas"], np.float64)
        self.volumes = np.ascontiguousarray(ins["volume"], np.float64)
        self.indices = np.ascontiguousarray(ins["idx"], np.int32)
        self.subgrid = int(ins["rank"][0]) != 0
        self.mesh = types.SimpleNamespace(dim=case_dim(case, ins))
        if self.subgrid:
            self.level_diff = np.ascontiguousarray(ins["level_diff"], np.int32)
            self.nb_offset = np.ascontiguousarray(ins["nb_offset"], np.int32)


def partition(case, tag):
    ins, _ = load(case, tag)
    return FixturePartition(case, ins)

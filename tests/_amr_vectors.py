"""Access to tests/golden/reference_amr_vectors.npz and reference_amr_vectors_rank3.npz (inputs and outputs of the reference's own
AMR transfer, indicator, z-order and partition kernel bodies, executed on tiny forests:
tests/golden/make_reference_amr_vectors.py) for the tests that consume them: the CPU oracle
(test_oracle_reference_amr_kernels.py) and the HIP kernels and the Python layer above them
(test_gpu_reference_amr_kernels.py). The second file holds the Subgrid arrays of the rank-3 cases; load() merges the two. Needs no
GPU."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = (os.path.join(HERE, "golden", "reference_amr_vectors.npz"), os.path.join(HERE, "golden", "reference_amr_vectors_rank3.npz"))
TAGS = ("f64", "f32")
PART_RANKS = (2, 3)
# name -> (old elements, new elements, {step of adapt_data: count}): what each case reaches (the generator asserts the same)
CENSUS = {
    "mixed2d": (256, 289, {0: 111, 1: 152, 4: 26}),
    "mixed3d": (512, 750, {0: 357, 1: 376, 8: 17}),
    "ends2d": (16, 19, {0: 6, 1: 12, 4: 1}),
    "ends3d": (64, 71, {0: 14, 1: 56, 8: 1}),
    "one2d": (4, 1, {4: 1}),
    "one3d": (8, 1, {8: 1}),
    "refined_ends2d": (64, 181, {0: 117, 1: 64}),
    "refined_ends3d": (512, 1702, {0: 1190, 1: 512}),
}

_cache = {}


def vectors():
    """every array of both files under its key"""
    if "z" not in _cache:
        z = {}
        for path in PATHS:
            with np.load(path, allow_pickle=False) as f:
                for k in f.files:
                    if k == "meta":
                        z.setdefault("meta", []).append(str(f[k][0]))
                    else:
                        assert k not in z, k
                        z[k] = f[k]
        _cache["z"] = z
    return _cache["z"]


def case_names():
    return sorted({k.split("|")[0] for k in vectors() if "|" in k})


def load(case, tag):
    z = vectors()
    ins = {k.split("|")[3]: v for k, v in z.items() if k.startswith(f"{case}|{tag}|in|")}
    outs = {k.split("|")[3]: v for k, v in z.items() if k.startswith(f"{case}|{tag}|out|")}
    return ins, outs


def sizes(ins):
    """n_old, n_new, F (interior faces of the old mesh), dim, Subgrid rank (0: the case has no Subgrid arrays)"""
    return tuple(int(x) for x in ins["sizes"])


def subgrid_cases():
    return [c for c in case_names() if sizes(load(c, "f64")[0])[4]]

"""The plans whose bytes tests/test_tile_plan_digests.py pins, and the digest of one plan. Shared with
tests/golden/make_tile_plan_digests.py, which writes the fixture from the library of the commit BEFORE a planner change."""
import hashlib

import numpy as np

ARRAYS = ("elem_off", "halo_off", "face_off", "halo_ids", "face_lr", "face_geo", "face_orig", "csr_off", "csr_ent", "tile_order",
          "ell", "geo_idx", "geo_table", "tile_desc")
SCALARS = ("ntiles", "max_elems", "max_halo", "max_faces", "n_interior", "n_deep", "max_slots", "ell_width", "n_patch_class",
           "n_irregular_class", "patch_dim", "open_faces", "farfield_faces")

CAPS = dict(tmax=64, fcap=150)
# wall, outflow, inflow state 0, far field against state 0: boundary kinds 0, 1, 2, 10
MIXED_SIDES_2D = ("wall", "outflow", 0, ("farfield", 0))
MIXED_SIDES_3D = ("wall", "outflow", 0, ("farfield", 0), "wall", ("farfield", 1))

# name -> (mesh, ranks, plan options); mesh: keyword arguments of SynthMesh, or the shape of a curved PrismHexMesh
CASES = {
    "amr2_patches_3ranks": (dict(dim=2, base_level=4, max_level=7, band=0.12), 3, dict(patches=True)),
    "amr2_walls": (dict(dim=2, base_level=3, max_level=5, band=0.06, periodic=False), 1, dict(patches=False)),
    "amr3_walls_patches_2ranks": (dict(dim=3, base_level=3, max_level=5, band=0.12, periodic=False), 2, dict(patches=True)),
    "box3_all_irregular": (dict(dim=3, base_level=4, max_level=4), 1, dict(patches=True, irregular="all")),
    "amr3_two_classes_no_face_geo": (dict(dim=3, base_level=3, max_level=5, band=0.12), 1,
                                     dict(patches=True, two_classes=True, want_face_geo=False)),
    "amr2_mixed_boundary_kinds": (dict(dim=2, base_level=4, max_level=7, band=0.12, sides=MIXED_SIDES_2D), 1, dict(patches=True)),
    # (in 2D a cell with a boundary face is never in a patch; in 3D the irregular form takes walls, so here patches ARE dropped)
    "amr3_mixed_boundary_kinds": (dict(dim=3, base_level=3, max_level=5, band=0.12, sides=MIXED_SIDES_3D), 1, dict(patches=True)),
    "curved_prism_hex": ((8, 8, 10), 1, dict(patches=True)),                    # 2 794 dictionary rows
    "curved_prism_hex_no_dictionary": ((14, 14, 12), 1, dict(patches=True)),    # more than 8 191: no geo_table, no geo_idx
}
THREADS_CASE = "amr3_walls_patches_2ranks"


def plan_digest(plan):
    h = hashlib.sha256()
    for name in ARRAYS:
        a = np.ascontiguousarray(getattr(plan, name))
        h.update(f"{name}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())
    for name in SCALARS:
        h.update(f"{name}={getattr(plan, name)!r};".encode())
    return h.hexdigest()


def case_digests(name):
    """{"<case>/rank<r>": digest} of every rank's plan of one case."""
    from t8gpu_amd.plan import HostPlainPlan
    from t8gpu_amd.synth import SynthMesh
    from t8gpu_amd.unstructured import PrismHexMesh
    mesh_args, ranks, options = CASES[name]
    mesh = PrismHexMesh(mesh_args) if isinstance(mesh_args, tuple) else SynthMesh(**mesh_args)
    out = {}
    for rk in range(ranks):
        part = mesh.partition(rk, ranks) if ranks > 1 else mesh.partition()
        out[f"{name}/rank{rk}"] = plan_digest(HostPlainPlan.from_partition(part, **CAPS, **options))
    return out

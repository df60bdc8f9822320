#!/usr/bin/env python3
"""usage: scripts/check_reference_examples.py <reference tree>
The drop-in boundary, checked against the reference's OWN translation units: the device-code TUs of its two examples
are compiled with hipcc for gfx950 against include/t8gpu, read from the reference tree given on the command line (never
copied into this repository, which is why this is a maintainer's check and not part of tests/). `<t8.h>` comes from
tests/compat/t8_stub (opaque handles, a compile-only stub: nothing is linked or run). Exit status 0 when both hold:

  examples/compressible_euler/kernels.cu   must compile with ZERO errors (t8gpu::MeshManager is a complete type,
                                           every accessor member the kernels use exists with the same signature)
  examples/subgrid/kernels_{2d,3d}.cu      every diagnostic must be one of the two places where the REFERENCE source
                                           omits the `template` keyword after `typename SubgridType::` (accepted by
                                           nvcc, an error for clang / hipcc; INTEGRATION.md section 1 tells a
                                           maintainer to add it) -- nothing may point at this backend's headers
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def hipcc(ref, src, example_dir, out=None):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-ferror-limit=0", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "tests", "compat", "t8_stub"), "-I", os.path.join(ref, "examples", example_dir),
           os.path.join(ref, "examples", example_dir, src)] + (["-fsyntax-only"] if out is None else ["-c", "-o", out])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


def errors(stderr):
    return [ln for ln in stderr.splitlines() if re.search(r": (fatal )?error:", ln)]


def plain_kernels_tu_compiles_unchanged(ref):
    """kepes_compute_fluxes / reflective_boundary_condition / estimate_gradient ... exactly as the reference wrote
    them, down to a gfx950 object file."""
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "kernels.o")
        res = hipcc(ref, "kernels.cu", "compressible_euler", obj)
        bad = res.returncode != 0 or errors(res.stderr) or os.path.getsize(obj) <= 10000
    return [res.stderr[-4000:]] if bad else []


def subgrid_kernels_tu_only_trips_over_its_own_missing_template_keywords(ref, src):
    errs = errors(hipcc(ref, src, "subgrid").stderr)
    ours = [e for e in errs if ROOT + os.sep in e or "include/t8gpu" in e]
    known = re.compile(r"examples/subgrid/(kernels\.h:60|kernels\.inl:1111):\d+: error: .*template")
    return ours + [e for e in errs if e not in ours and not known.search(e)][:20]


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "examples")):
        sys.exit(__doc__)
    ref = sys.argv[1]
    failed = 0
    checks = [("compressible_euler/kernels.cu", lambda: plain_kernels_tu_compiles_unchanged(ref))]
    checks += [(f"subgrid/{src}", lambda src=src: subgrid_kernels_tu_only_trips_over_its_own_missing_template_keywords(ref, src))
               for src in ("kernels_3d.cu", "kernels_2d.cu")]
    for name, check in checks:
        problems = check()
        print(f"{name}: {'FAILED' if problems else 'ok'}")
        for p in problems:
            print("  " + p)
        failed += bool(problems)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()

"""Build the reference's own MEX gateways, unchanged, against the stand-in MEX runtime in oracle/refmex/.

    [PDEIP_REFERENCE_DIR=<reference checkout>] python oracle/build_ref.py [--force] [--if-present]

The reference checkout defaults to a directory `reference` beside this repository.  --if-present: succeed, doing
nothing, when there is none (how __graft_entry__.build() calls it).

For each gateway below this compiles <reference>/mex/source/<Gateway>.c with the library file mex/buildAll.m pairs it
with, plus refmex/refmex.c, into oracle/_ref/<Gateway>.so (one shared object per gateway, as buildAll.m builds them:
some library files define functions of the same name).  tests/ref_lib.py loads the results.  Nothing the reference
holds is copied into this repository; oracle/_ref/ is ignored by git.

oracle/_ref/MANIFEST.json records the gateways built, the compiler, the flags and the sha256 of every source file
used, reference and stand-in alike; a build whose manifest matches the sources is left alone.
"""
import concurrent.futures
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
REFMEX_DIR = os.path.join(HERE, "refmex")
MANIFEST = os.path.join(OUT_DIR, "MANIFEST.json")
ENV_VAR = "PDEIP_REFERENCE_DIR"

# gateway -> library file, as mex/buildAll.m pairs them (SurfaceEquation needs BLAS/LAPACK and is out of scope)
GATEWAYS = {
    "Oflow_sor_elin4_2d": "opticalflowSolvers.c",
    "Oflow_sor_llin4_2d": "opticalflowSolvers.c",
    "Oflow_sor_llin8_2d": "opticalflowSolvers.c",
    "Oflow_lhs_elin4_2d": "opticalflowSolvers.c",
    "Oflow_lhs_llin4_2d": "opticalflowSolvers.c",
    "Disp_sor_llin4_2d": "disparitySolvers.c",
    "Disp_sor_llin_sym4_2d": "disparitySolvers.c",
    "PDEsolver4": "pdeSolvers.c",
    "PDEsolver8": "pdeSolvers.c",
    "DdiffWeights": "imageDiffusionWeights.c",
    "BilinInterp_2d": "imageInterpolation.c",
    "FstDerivatives5": "imageDerivatives.c",
    "SndDerivatives5": "imageDerivatives.c",
    "AC_solver_2d": "levelsetSolvers.c",
    "Reinit": "levelsetSolvers.c",
    "CV_solver_2d": "levelsetSolvers.c",
}
CC = "gcc"
# x86-64 with no -march: SSE2 arithmetic, no FMA; contraction off so every float operation is the one the C states.
# -msse and -fopenmp are what buildAll.m adds for the level-set gateways; they are harmless for the others.
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-msse", "-fPIC"]
# -Bsymbolic: a gateway's calls into its library bind inside its own object, whatever else the process has loaded
LDFLAGS = ["-shared", "-fopenmp", "-Wl,-Bsymbolic", "-lm"]
STAND_IN = ["mex.h", "matrix.h", "refmex.c"]


def reference_dir():
    """The reference checkout: $PDEIP_REFERENCE_DIR if set, else a directory `reference` beside this repository.
    None when that directory does not hold mex/source."""
    d = os.environ.get(ENV_VAR) or os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference")
    return os.path.abspath(d) if os.path.isdir(os.path.join(d, "mex", "source")) else None


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _headers(ref):
    lib = os.path.join(ref, "mex", "source", "library")
    return sorted(os.path.join("mex", "source", "library", f) for f in os.listdir(lib) if f.endswith(".h"))


def reference_sources(ref):
    """Reference files (paths relative to its root) the build reads: the gateways, their library files, the headers."""
    files = set(_headers(ref))
    for gw, libfile in GATEWAYS.items():
        files.add(os.path.join("mex", "source", gw + ".c"))
        files.add(os.path.join("mex", "source", "library", libfile))
    return sorted(files)


def stand_in_hashes():
    """sha256 of the stand-in runtime and of this recipe: what a build depends on besides the reference."""
    h = {os.path.join("refmex", f): _sha(os.path.join(REFMEX_DIR, f)) for f in STAND_IN}
    h["build_ref.py"] = _sha(os.path.abspath(__file__))
    return h


def compiler_version():
    return subprocess.run([CC, "--version"], check=True, capture_output=True, text=True).stdout.splitlines()[0]


def expected_manifest(ref):
    return {
        "gateways": sorted(GATEWAYS),
        "library": dict(sorted(GATEWAYS.items())),
        "compiler": compiler_version(),
        "cflags": CFLAGS,
        "ldflags": LDFLAGS,
        "reference_sha256": {f: _sha(os.path.join(ref, f)) for f in reference_sources(ref)},
        "stand_in_sha256": stand_in_hashes(),
    }


def read_manifest():
    try:
        with open(MANIFEST) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def up_to_date(ref):
    """True when oracle/_ref/ holds every gateway, built by this recipe from the sources `ref` holds now."""
    m = read_manifest()
    if m is None or m != expected_manifest(ref):
        return False
    return all(os.path.exists(os.path.join(OUT_DIR, gw + ".so")) for gw in GATEWAYS)


def _compile(ref, gw, libfile):
    src = os.path.join(ref, "mex", "source")
    so = os.path.join(OUT_DIR, gw + ".so")
    tmp = so + ".tmp"
    # -w: the reference's own warnings (pointer signedness, unused variables) are not this build's to fix
    cmd = ([CC] + CFLAGS + ["-w", "-I" + REFMEX_DIR, "-I" + os.path.join(src, "library"), "-o", tmp,
                             os.path.join(src, gw + ".c"), os.path.join(src, "library", libfile),
                             os.path.join(REFMEX_DIR, "refmex.c")] + LDFLAGS)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building %s failed:\n%s\n%s" % (gw, " ".join(cmd), r.stderr))
    os.replace(tmp, so)
    return gw


def build(ref=None, force=False, jobs=None):
    """Build oracle/_ref/ from the reference at `ref` (default: $PDEIP_REFERENCE_DIR).  Returns the manifest, or None
    when there is no reference to build from (then an existing oracle/_ref/ is left as it is)."""
    ref = ref or reference_dir()
    if ref is None:
        return None
    ref = os.path.abspath(ref)
    if not force and up_to_date(ref):
        return read_manifest()
    os.makedirs(OUT_DIR, exist_ok=True)
    if os.path.exists(MANIFEST):
        os.remove(MANIFEST)  # a half-finished rebuild must not look current
    jobs = jobs or min(16, len(GATEWAYS), os.cpu_count() or 1)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(lambda kv: _compile(ref, *kv), GATEWAYS.items()))
    manifest = expected_manifest(ref)
    with open(MANIFEST + ".tmp", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    os.replace(MANIFEST + ".tmp", MANIFEST)
    return manifest


if __name__ == "__main__":
    if reference_dir() is None:
        if "--if-present" in sys.argv[1:]:
            print("[build_ref] no reference checkout; oracle/_ref/ left as it is")
            sys.exit(0)
        sys.exit("build_ref.py: no reference checkout: set %s to a directory holding mex/source" % ENV_VAR)
    m = build(force="--force" in sys.argv[1:])
    print("[build_ref] %d gateways in %s (%s)" % (len(m["gateways"]), OUT_DIR, m["compiler"]))

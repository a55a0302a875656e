"""CPU: the host-side decisions of the sparse driver's calls (csrc/pdeip_sparse_plan.hpp: the argument checks of pdeip_nanmedfilt2 and
pdeip_sparse_pyramid, the scale sizes, the pyramid's and the builder's workspace layout up to planes of INT_MAX pixels, the sparse
stages' constants) run as a stand-alone program under the address and undefined-behaviour sanitizers (tools/sparse_plan_check.cpp).
Nothing sanitized is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_plan_check")
    cxx = os.environ.get("CXX", "c++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "sparse_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr

"""CPU: the host-side decisions of generateSeeds() and the dense driver (csrc/pdeip_seeds_plan.hpp: argument checks, scale sizes,
the visit / RITER / RCONS schedule, the consensus-set vector, stage seeds) run as a stand-alone program under the address and
undefined-behaviour sanitizers (tools/seeds_plan_check.cpp).  Nothing sanitized is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "seeds_plan_check")
    cxx = os.environ.get("CXX", "c++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "seeds_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr

"""csrc/launch_plan.h decides which launches a forward consists of, in plain C++: tests/launch_plan_check.cpp plans the stack for
every option combination on the host and asserts the invariants run_stack relies on.  Compiled here with ASan + UBSan and run as
a program of its own: no GPU, no Python extension, nothing preloaded."""
import shutil
import subprocess
from pathlib import Path

TESTS = Path(__file__).resolve().parent


def test_every_launch_plan_keeps_the_executors_invariants(tmp_path):
    cxx = shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "launch_plan_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                            "-o", str(exe), str(TESTS / "launch_plan_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    checked = int(run.stdout.split("plans checked:")[1].split(",")[0])
    assert checked >= 5 * 2 * 4 * 2 * 2 * 4096, checked          # precisions x buffers x fuse_block1 x tile x profile x the twelve switches
    assert "violations: 0" in run.stdout

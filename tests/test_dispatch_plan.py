"""The dispatch plans of the graph kernels (csrc/tile_plan.h) and of the dense kernels (csrc/dense_plan.h) on a CPU: tests/dispatch_plan_check.hip walks a table with
one case on each side of every comparison - pieces per wave, the image cap, e >= 6 n, Fin / C / H / F, heavy rows, the
2^24 / 2^31 / 2^32 offset limits, every per-call switch - and is built with the host sanitizers (no GPU test of a few
seconds reaches the offset limits).  tests/dense_plan_check.hip does the same for the dense family: panel / tile / split-operand
choice, template constants, grids, LDS, the dW and fused-backward workspace layouts and the chained MLP forward."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _build_and_run(tmp_path, name):
    exe = str(tmp_path / name)
    build = subprocess.run(
        [HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Werror",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
         os.path.join(HERE, name + ".hip"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout


def test_dispatch_plan_table(tmp_path):
    _build_and_run(tmp_path, "dispatch_plan_check")


def test_dense_plan_table(tmp_path):
    _build_and_run(tmp_path, "dense_plan_check")

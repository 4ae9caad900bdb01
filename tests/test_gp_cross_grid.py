"""cross_grid on the host (math_amd/csrc/gp_family.h): the launch grid that the
rectangular GP walks of gp.hip (rows = 256, or 2048 in the 16-byte form) and
smg_gp_ard_cross_cov_rev (rows = 256) share.  tests/cpp/gp_cross_grid_check.cpp
prints the function's own result, held here against the closed form: one
workgroup per column up to 2048, times ceil(n1 / rows) row parts capped at
2048 // gx, never fewer than one.  No GPU and nothing of the library is needed.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
GP_BLOCKS = 2048
CASES = [(1, 1, 256), (5, 2050, 256), (2050, 5, 256), (262144, 64, 2048), (300, 257, 2048)]


def closed_form(n1, n2, rows):
    gx = min(n2, GP_BLOCKS)
    return gx, max(1, min(-(-n1 // rows), GP_BLOCKS // gx))


def test_cross_grid(tmp_path):
    exe = tmp_path / "gp_cross_grid_check"
    src = os.path.join(HERE, "cpp", "gp_cross_grid_check.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(HERE, "..", "include"), src, "-o", str(exe)])
    args = [str(v) for case in CASES for v in case]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in run.stdout.strip().splitlines()]
    assert got == [case + closed_form(*case) for case in CASES]
    # the hand-written lines smg_gp_ard_cross_cov_rev had (rows = 256), gy >= 1 included
    for n1, n2, rows, gx, gy in got:
        if rows == 256:
            assert (gx, gy) == (min(n2, 2048), min((n1 + 255) // 256, 2048 // min(n2, 2048))) and gy >= 1

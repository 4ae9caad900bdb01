"""The GEMM's tile map on the host (math_amd/csrc/gemm_tiles.h: the grid plan,
the tile of a workgroup, the K range of a tile -- the functions launch and
k_gemm call).  tests/cpp/gemm_tile_map_check.cpp enumerates every launched
grid of its configurations (tile sizes, MODE 0 to 4, triangular operands,
1 to 40 and 66 tiles per side, trapezoids, the offset cuts in both cut modes,
every K the split rule tells apart) and asserts that each required tile is
produced once per split and nothing else, that the splits' K ranges tile
exactly [lo, hi) as the definitions give it, and that this range holds every
term that can be nonzero.  No GPU and nothing of the library is needed.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_map(tmp_path):
    exe = tmp_path / "gemm_tile_map_check"
    src = os.path.join(HERE, "cpp", "gemm_tile_map_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    m = re.search(r"(\d+) configurations, (\d+) workgroups, 0 failed", run.stdout)
    assert m and int(m.group(1)) > 100000 and int(m.group(2)) > 10 * int(m.group(1))

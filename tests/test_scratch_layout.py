"""ScratchLayout and the four scratch arenas of the scene operations (infinitam_amd/csrc/scene_ops.h: merge / coarsen, resample, band
samples, prune) on the host: tests/cpp/scratch_layout_check.cpp, a stand-alone program in plain C++, is compiled with g++ and run; nothing
is loaded into this process and no GPU is needed.  It checks the layout rules (256-byte boundaries, declaration order, no overlap, empty
parts, bytes_before) over a few hundred layouts, and that every array of the four arenas lies where the entry points' hand-carved chains
of offsets put it before, at the tiny tables of the GPU tests and at the default table."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_rules_and_the_four_arenas_lie_where_the_chains_put_them(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/scratch_layout_check.cpp"
    exe = str(tmp_path / "scratch_layout_check")
    src = os.path.join(ROOT, "tests", "cpp", "scratch_layout_check.cpp")
    b = subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", src, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scratch layout check ok: 400 layouts, 4 arenas at 4 tables" in r.stdout

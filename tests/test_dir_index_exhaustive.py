"""The block directory's index from voxel-unit coordinates (accel_device.h: dir_cell_voxel / dir_covers_voxel, the form the ray cast's
empty-space look-ahead computes) against the block-unit form of every writer and every other reader -- exhaustively, on the host:
tests/cpp/dir_index_check.cpp, a stand-alone program, is compiled for the host only and run; nothing is loaded into this process and no
GPU is needed.  And the float32 fact the look-ahead's coverage test rests on: a ray's look-ahead positions are monotone per axis, so a
round whose first and last cell lie inside the directory cube lies inside it entirely."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_voxel_form_equals_block_form_for_every_cell_and_around_the_cube(tmp_path):
    exe = str(tmp_path / "dir_index_check")
    src = os.path.join(ROOT, "tests", "cpp", "dir_index_check.cpp")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-w", src, "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dir index check ok: 134217728 cube triples" in r.stdout


def test_look_ahead_positions_are_monotone_per_axis():
    """q_0 = p, q_j = fl(q_{j-1} + s) with s = fl(8 d): the looked-up voxel (int)ROUND(q_j) never moves against the sign of s, for any
    start and step -- so max(t_0, t_K-1) bounds every t_j from above and min from below, which is what lets the kernel test the first
    and the last cell of a round for coverage instead of all of them."""
    rng = np.random.default_rng(11)
    n, K = 200000, 16
    p = (rng.uniform(-1, 1, n) * np.float32(2.0) ** rng.integers(0, 20, n)).astype(np.float32)
    p[: n // 4] = (rng.integers(-30000, 30000, n // 4) * 8 + rng.choice([-0.5, 7.5, 7.4999995, -0.50000006, 0.49999997], n // 4)).astype(np.float32)
    d = rng.uniform(-1, 1, n).astype(np.float32)
    d[rng.random(n) < 0.1] = 0.0
    d[rng.random(n) < 0.05] = np.float32(1e-9)
    s = (np.float32(8.0) * d).astype(np.float32)

    def voxel(q):
        r = np.where(q < 0, q - np.float32(0.5), q + np.float32(0.5)).astype(np.float32)      # ROUND, then (int)
        return np.trunc(r).astype(np.int64)

    q, prev = p.copy(), voxel(p)
    for _ in range(K):
        q = (q + s).astype(np.float32)
        v = voxel(q)
        assert np.all((v - prev) * np.sign(s) >= 0)
        prev = v

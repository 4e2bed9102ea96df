"""Randomised stress parity (seeded): random 6-DoF poses, intrinsics, voxel sizes / band widths, voxel and index
types, depth noise and holes, fused and separate call sequences, followed by the free-view entry points
(FindVisibleBlocks, CreateExpectedDepths, RenderImage of every type, ForwardRender, CreatePointCloud) from a second
random pose.  HIP vs oracle, bit-exact; the oracle itself is pinned to the reference on the same generator for a
subset (where the reference build exists)."""
import numpy as np
import pytest

import itm_testlib as T
from infinitam_amd import capi, synth
from infinitam_amd.capi import (BUF_FORWARD_PROJECTION, BUF_MISSING_POINTS, BUF_RAYCAST_IMAGE, BUF_RAYCAST_RESULT, DevBuffer, View)

F = np.float32
W, H = 96, 72


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(F)


def pose(rng, scale):
    """world -> camera matrix, column-major 16 floats"""
    R = rot(*(rng.uniform(-0.25, 0.25, 3) * scale))
    t = (rng.uniform(-0.15, 0.15, 3) * scale).astype(F)
    m = np.eye(4, dtype=F); m[:3, :3] = R.T; m[:3, 3] = -(R.T @ t)
    return np.ascontiguousarray(m.T).reshape(16).copy()


def make_case(seed):
    rng = np.random.default_rng(seed)
    voxel = [capi.VOXEL_S, capi.VOXEL_F, capi.VOXEL_S_RGB, capi.VOXEL_F_RGB][seed % 4]
    dense = (seed % 5 == 4)
    vs = float(rng.choice([0.004, 0.008, 0.01, 0.02]))
    mu = float(vs * rng.choice([2.0, 4.0, 5.0]))
    f = float(rng.uniform(70, 130))
    intr = (F(f), F(f * rng.uniform(0.9, 1.1)), F(W / 2 + rng.uniform(-6, 6)), F(H / 2 + rng.uniform(-6, 6)))
    frames = []
    for k in range(3):
        M = pose(rng, 1.0)
        d = synth.depth_frame(W, H, (F(0.01 * k), F(0), F(0)), intr).astype(F)
        d = d + rng.normal(0, 0.002, d.shape).astype(F)
        holes = rng.random(d.shape) < 0.03
        d[holes] = rng.choice([F(-1.0), F(0.0)])
        frames.append((M, np.ascontiguousarray(d)))
    return dict(voxel=voxel, dense=dense, vs=vs, mu=mu, intr=intr, frames=frames, free=pose(rng, 1.5), fused=[bool(b) for b in rng.integers(0, 2, 3)],
                maxW=int(rng.choice([2, 100])), stop=bool(rng.integers(0, 2)))


def run_case(be, c):
    prm = capi.default_params(c["vs"], c["mu"], c["maxW"], 0.35, 3.0, c["stop"])
    kw = dict(denseSize=(96, 96, 96), denseOffset=(-48, -48, 40)) if c["dense"] else {}
    scene = be.create_scene(c["voxel"], capi.INDEX_DENSE if c["dense"] else capi.INDEX_HASH, prm, **kw)
    scene.reco.ResetScene()
    rs = scene.vis.CreateRenderState((W, H))
    P = W * H
    pts = DevBuffer(be, P * 16, np.float32, (H, W, 4)); nrm = DevBuffer(be, P * 16, np.float32, (H, W, 4))
    colour = c["voxel"] in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)
    rgb = be.to_backend(synth.rgb_frame(W, H)) if colour else None
    out = {}
    for k, (M, d) in enumerate(c["frames"]):
        v = View(be.to_backend(d), W, H, M_d=M, intr_d=c["intr"], rgb=rgb, w_rgb=W, h_rgb=H, intr_rgb=c["intr"])
        if c["fused"][k]:
            scene.process_frame(v, rs, pts, nrm)
        else:
            scene.reco.AllocateSceneFromDepth(v, rs); scene.reco.IntegrateIntoScene(v, rs)
            scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, rs); scene.vis.CreateICPMaps(v, rs, pts, nrm)
        out[f"counters{k}"] = scene.counters(rs)
    out["points"], out["normals"] = pts.numpy(), nrm.numpy()
    out["voxels"] = scene.download(capi.BUF_VOXEL_BLOCKS)
    if not c["dense"]:
        out["hash"] = scene.download(capi.BUF_HASH_ENTRIES)
    # forward render of the last ray-cast result into the free pose (ITMTrackingController.cpp:39-43)
    vfree = View(v.depth, W, H, M_d=c["free"], intr_d=c["intr"], rgb=rgb, w_rgb=W, h_rgb=H, intr_rgb=c["intr"])
    scene.vis.ForwardRender(vfree, rs)
    out["fwd"] = scene.download(BUF_FORWARD_PROJECTION, rs); out["missing_n"] = scene.counters(rs)["noFwdProjMissingPoints"]
    out["missing"] = scene.download(BUF_MISSING_POINTS, rs)[: out["missing_n"]]
    # free-view pipeline
    scene.vis.FindVisibleBlocks(c["free"], c["intr"], rs)
    scene.vis.CreateExpectedDepths(c["free"], c["intr"], rs)
    out["visible_free"] = scene.counters(rs)["noVisibleEntries"]
    img = DevBuffer(be, P * 4, np.uint8, (H, W, 4))
    for t in (capi.RENDER_SHADED_GREYSCALE, capi.RENDER_COLOUR_FROM_VOLUME, capi.RENDER_COLOUR_FROM_NORMAL):
        be.check(be.fn["memcpy_h2d"](capi._P(img.ptr), np.zeros(P * 4, np.uint8).ctypes.data_as(capi._P), P * 4, None), "clear")
        scene.vis.RenderImage(c["free"], c["intr"], rs, img, t)
        out[f"render{t}"] = img.numpy()
    out["rays_free"] = scene.download(BUF_RAYCAST_RESULT, rs)
    loc = DevBuffer(be, P * 16, np.float32, (P, 4)); col = DevBuffer(be, P * 16, np.float32, (P, 4))
    scene.vis.CreatePointCloud(vfree, rs, loc, col, skipPoints=bool(len(c["frames"]) % 2))
    n = scene.counters(rs)["noTotalPoints"]
    out["cloud_n"], out["cloud"], out["cloud_col"] = n, loc.numpy()[:n], col.numpy()[:n]
    rs.close(); scene.close()
    return out


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if k == "rays_free" or k == "fwd":          # xyz of rays that miss is unspecified in the reference
            assert np.array_equal(x[..., 3], y[..., 3]), (tag, k, "w")
            hit = x[..., 3] > 0
            assert np.array_equal(x[hit], y[hit]), (tag, k)
        elif isinstance(x, np.ndarray):
            if x.dtype.names:
                T.assert_fields_equal(x, y, f"{tag}.{k}")
            else:
                assert np.array_equal(x, y), (tag, k, int((x != y).sum()))
        elif isinstance(x, dict):
            for f in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries"):
                assert x[f] == y[f], (tag, k, f, x, y)
        else:
            assert x == y, (tag, k, x, y)


@pytest.mark.parametrize("seed", [3, 6, 13])
def test_oracle_matches_reference_on_random_cases(oracle, ref, seed):
    c = make_case(seed)
    if c["dense"]:
        pytest.skip("the reference shim keeps its 512^3 dense allocation")
    a = run_case(oracle, c)
    if ref.backend is not None:
        assert_same(a, run_case(ref.backend, c), f"seed{seed}")
    ref.check("case", a)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(range(16)))
def test_hip_matches_oracle_on_random_cases(hip, oracle, seed):
    c = make_case(seed)
    assert_same(run_case(hip, c), run_case(oracle, c), f"seed{seed}")

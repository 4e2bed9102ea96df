"""ITMMainEngine::GetImage (reference Engine/ITMMainEngine.cpp:129-192) on the HIP back-end: the three colour maps of
IITMVisualisationEngine (Engine/ITMVisualisationEngine.cpp:7-107) as kernels (infinitam_amd/csrc/image_maps.hip) and
ITMMainEngine_HIP::GetImage / GetImageDevice / GetImageSize (include/itm_hip_engines.hpp).

  CPU   the float32 restatement (tests/image_map_terms.py) reproduces what the reference's own functions give on the inputs of
        tests/image_map_cases.py (tests/golden/g_image_maps.*, written by tests/golden/make_golden_image_maps.py); its edge cases;
        header, binding and library name the entry points; the adapter's methods instantiate.
  GPU   every map equals the restatement byte for byte on every case and on real images of the view builder and the ray cast; calls
        on two streams do not share their limits; through tests/cpp/get_image_demo.cpp every GetImage type equals what it is defined
        as (the free camera: the CPU oracle's FindVisibleBlocks / CreateExpectedDepths / RenderImage on its own scene fused with the
        same frames); GetImage after every frame changes no pose, scene digest or tracking map."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import image_map_cases as IC
import image_map_terms as IT
import itm_testlib as T
import test_main_engine as TM
from infinitam_amd import capi, synth

F = np.float32
W, H = TM.W, TM.H
GOLDEN = os.path.join(T.GOLDEN_DIR, "g_image_maps")
DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "get_image_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "get_image_demo")
MAP_FUNCTIONS = ("depth_to_uchar4", "weight_to_uchar4", "normal_to_uchar4")


def golden():
    with open(GOLDEN + ".json") as f:
        return json.load(f), np.load(GOLDEN + ".npz")


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(IC.GOLDEN_CASES))
def test_restatement_reproduces_the_reference(name):
    meta, arr = golden()
    g = meta["cases"][name]
    kind, src = IC.GOLDEN_CASES[name]
    assert g["kind"] == kind and g["shape"] == list(src.shape)
    assert IT.sha256(src) == g["input_sha256"], "the case's input is not the one the golden was made from"
    parts = {}
    out = IT.MAPS[kind](src, parts)
    assert "values" not in parts or IT.in_conversion_range(parts["values"]), "a golden case must stay inside the conversion's range"
    flat = out.reshape(-1, 4)
    assert meta["subset_stride"] == IC.SUBSET_STRIDE
    assert np.array_equal(flat[::IC.SUBSET_STRIDE], arr[name]), name
    assert int(np.count_nonzero(flat.any(axis=1))) == g["nonzero_pixels"]
    lim = list(IT.depth_limits(src)) if kind == "depth" else [IT.weight_limit(src)] if kind == "weight" else []
    assert ["%08x" % F(v).view(np.uint32) for v in lim] == g["limits_float32_bits"]
    assert IT.sha256(out) == g["output_sha256"], name


def test_golden_covers_every_case_inside_the_conversion_range():
    meta, arr = golden()
    assert set(meta["cases"]) == set(IC.GOLDEN_CASES) == set(arr.files)
    assert not set(IC.EXTRA_CASES) & set(meta["cases"])
    for name, (kind, src) in IC.EXTRA_CASES.items():          # and the extra cases really leave it
        parts = {}
        IT.MAPS[kind](src, parts)
        assert not IT.in_conversion_range(parts["values"]), name
    for tag, (w, h) in IC.SIZES.items():
        for kind in IT.MAPS:
            assert meta["cases"][f"{kind}_{tag}"]["shape"][:2] == [h, w]
    d = IC.GOLDEN_CASES["depth_vga"][1]
    assert d.shape == (480, 640) and abs((d == -1).mean() - 0.10) < 0.01 and abs((d == 0).mean() - 0.02) < 0.005
    u = IC.GOLDEN_CASES["weight_vga"][1]
    assert not u[:2].any() and not u[:, -2:].any() and (u == -1).any() and u[u > 0].min() >= 5e-4 and u.max() <= 2e-2
    n = IC.GOLDEN_CASES["normal_vga"][1]
    assert set(np.unique(n[..., 3])) == {-1.0, 0.0} and np.allclose((n[..., :3] ** 2).sum(-1), 1, atol=1e-5)


def test_restatement_edge_cases():
    c = IC.GOLDEN_CASES
    # no valid pixel: nothing is coloured, the limits keep their initial values
    out = IT.depth_to_uchar4(c["depth_no_valid"][1])
    assert not out.any() and list(IT.depth_limits(c["depth_no_valid"][1])) == [F(100000), F(-100000)]
    assert not IT.weight_to_uchar4(c["weight_no_valid"][1]).any() and IT.weight_limit(c["weight_no_valid"][1]) == F(1000)
    # one distinct valid value / one valid pixel: lo == hi, the whole image is zero (alpha included)
    for name in ("depth_one_distinct_value", "depth_one_pixel"):
        src = c[name][1]
        lo, hi = IT.depth_limits(src)
        assert lo == hi and (src > 0).any() and not IT.depth_to_uchar4(src).any(), name
    # two pixels, the ends of the ramp.  t = 0: base(-0.5) = (-0.5 + 0.75) * 1 / 0.5 = 0.5, base(0) = 1, base(0.5) = (0.5 - 0.25) * -1 / 0.5 + 1
    # = 0.5 -> (127, 255, 127); t = 1: base(0.5) = 0.5, base(1) = 0, base(1.5) = 0 -> (127, 0, 0); everything else 0
    two = IT.depth_to_uchar4(c["depth_two_pixels"][1])
    assert tuple(two[3, 3]) == (127, 255, 127, 255) and tuple(two[40, 60]) == (127, 0, 0, 255) and np.count_nonzero(two.any(-1)) == 2
    # one valid weight: min / value = 1 -> s = 1: red 0, green 255, alpha stays 0
    one = IT.weight_to_uchar4(c["weight_one_pixel"][1])
    assert tuple(one[10, 10]) == (0, 255, 0, 0) and np.count_nonzero(one.any(-1)) == 1
    # NaN and +inf among the depths: NaN and -inf are not valid (v > 0 fails); +inf is, and becomes the upper limit: the scale is 0,
    # every finite pixel sits at t = 0 and the infinite one at t = NaN, which falls through base() to 0 in all three channels
    src = c["depth_nan_inf"][1]
    out = IT.depth_to_uchar4(src)
    lo, hi = IT.depth_limits(src)
    assert np.isinf(hi) and np.isfinite(lo)
    assert not out[1, 1].any() and not out[30, 30].any() and not out[31, 2].any()
    assert tuple(out[2, 5]) == (0, 0, 0, 255)
    finite = (src > 0) & np.isfinite(src)
    assert np.all(out[finite] == np.array([127, 255, 127, 255], np.uint8))
    # NaN alone changes nothing for the other pixels
    src = c["depth_nan"][1]
    clean = src.copy(); clean[4, 4] = -1; clean[9, 50] = -1
    assert np.array_equal(IT.depth_to_uchar4(src), IT.depth_to_uchar4(clean))
    # limits beyond the initial ones: the initial lower limit 100000 stays when every value lies above it, the initial minimum 1000 too
    assert IT.depth_limits(c["depth_beyond_initial_limits"][1])[0] == F(100000)
    assert IT.weight_limit(c["weight_above_initial_minimum"][1]) == F(1000)
    # normals: w < 0 and w = NaN are holes; the axes give the ends of the range
    na = IT.normal_to_uchar4(c["normal_axes"][1])
    assert tuple(na[0, 0]) == (255, 165, 165, 0) and tuple(na[0, 1]) == (76, 165, 165, 0) and tuple(na[0, 2]) == (165, 255, 76, 0)
    assert not IT.normal_to_uchar4(c["normal_all_holes"][1]).any()
    ex = IT.normal_to_uchar4(IC.EXTRA_CASES["normal_out_of_range"][1])
    assert tuple(ex[3, 3][:1]) == (0,) and tuple(ex[4, 4]) == (255, 0, 165, 0) and not ex[5, 5].any()
    # the conversion: truncation inside the range, saturation outside, NaN -> 0
    assert list(IT.to_uchar(np.array([0.0, 0.99, 1.0, 254.999, 255.0, 255.9, 256.0, 1e9, -0.5, -3.0, np.nan, np.inf, -np.inf], F))) == \
        [0, 0, 1, 254, 255, 255, 255, 255, 0, 0, 0, 255, 0]


def test_header_binding_and_library_name_the_maps(hip_host):
    declared = capi.declared_functions()
    with open(capi.header_path()) as f:
        header = f.read()
    lib = C.CDLL(hip_host.path)
    for fn in MAP_FUNCTIONS:
        assert fn in declared and fn in capi._HOST_IO_SIGS and fn not in capi._SIGS and fn in hip_host.fn
        assert hasattr(lib, "itm_" + fn)
        assert capi._HOST_IO_SIGS[fn] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p])
    assert "Engine/ITMVisualisationEngine.cpp:7-57" in header            # the entry points cite the reference
    for m in ("DepthToUchar4", "WeightToUchar4", "NormalToUchar4"):
        assert callable(getattr(capi.VisualisationEngine, m))
    with open(os.path.join(T.ROOT, "infinitam_amd", "csrc", "Makefile")) as f:
        assert "image_maps.hip" in f.read()


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_demo_compiles_and_get_image_instantiates(tmp_path):
    assert os.path.exists(build_demo())
    src = tmp_path / "get_image.cpp"
    lines = ['#include "itm_hip_engines.hpp"', "using namespace itmhip;"]
    for v, i in (("ITMVoxel_s", "ITMVoxelBlockHash"), ("ITMVoxel_f_rgb", "ITMPlainVoxelArray")):
        e = f"ITMMainEngine_HIP<{v}, {i}>"
        lines += [f"template void {e}::GetImage(ITMUChar4Image*, {e}::GetImageType, const ITMPose*, const ITMIntrinsics*);",
                  f"template const uint8_t* {e}::GetImageDevice(Vector2i*, {e}::GetImageType, const ITMPose*, const ITMIntrinsics*, Vector2i);",
                  f"template Vector2i {e}::GetImageSize() const;",
                  f"static_assert({e}::InfiniTAM_IMAGE_ORIGINAL_RGB == 0 && {e}::InfiniTAM_IMAGE_ORIGINAL_DEPTH == 1 && {e}::InfiniTAM_IMAGE_SCENERAYCAST == 2 && "
                  f"{e}::InfiniTAM_IMAGE_FREECAMERA_SHADED == 3 && {e}::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME == 4 && "
                  f"{e}::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL == 5 && {e}::InfiniTAM_IMAGE_UNKNOWN == 6, \"the reference's order\");"]
    lines += ["void image(ITMUChar4Image* img) { img->ChangeDims(Vector2i{4, 3}); img->Clear(); Vector4u* p = img->GetData(); (void)p; (void)img->noDims; }"]
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- GPU: the maps ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vis(hip):
    """A VisualisationEngine mirror to call the static maps through (any scene will do: a small dense one)."""
    scene = hip.create_scene(capi.VOXEL_S, capi.INDEX_DENSE, capi.default_params(), denseSize=(32, 32, 32))
    yield scene.vis
    scene.close()


def run_map(hip, vis, kind, src, stream=None, src_dev=None):
    """The map of `kind` on a device copy of src; the output image is filled with 0xCD first: every pixel must be written."""
    h, w = src.shape[:2]
    s = src_dev if src_dev is not None else hip.to_backend(np.ascontiguousarray(src, F))
    d = hip.to_backend(np.full((h, w, 4), 0xCD, np.uint8))
    {"depth": vis.DepthToUchar4, "weight": vis.WeightToUchar4, "normal": vis.NormalToUchar4}[kind](d, s, (w, h), stream)
    return d.numpy(stream)


def assert_same_image(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(-1))
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ, first at (y, x) {bad[:4].tolist()}: "
                             f"{[got[tuple(b)].tolist() for b in bad[:4]]} vs {[want[tuple(b)].tolist() for b in bad[:4]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(IC.ALL_CASES))
def test_map_equals_the_restatement(hip, vis, name):
    kind, src = IC.ALL_CASES[name]
    want = IT.MAPS[kind](src)
    got = run_map(hip, vis, kind, src)
    assert_same_image(got, want, name)
    assert_same_image(run_map(hip, vis, kind, src), got, name + " (second run)")
    if name in IC.GOLDEN_CASES:
        meta, _ = golden()
        assert IT.sha256(got) == meta["cases"][name]["output_sha256"]          # the reference's own output


@pytest.mark.gpu
def test_maps_of_the_view_builders_and_the_ray_casts_images(hip, vis):
    """Real images, holes included: depth and uncertainty of update_view (noise model on) for the standard synthetic sequence, the
    view builder's normal image, and the normals map of create_icp_maps."""
    intr = synth.intrinsics_for(W, H)
    raw = hip.to_backend(synth.raw_depth_mm(W, H, synth.parity_position(1), intr))
    depth, scratch, sigma = (hip.to_backend(np.zeros((H, W), F)) for _ in range(3))
    normal = hip.to_backend(np.zeros((H, W, 4), F))
    ia = (C.c_float * 4)(*intr)
    hip.check(hip.fn["update_view"](raw.ptr, W, H, 1, 0.001, 0.0, C.cast(ia, C.c_void_p), 1, 1, depth.ptr, scratch.ptr, normal.ptr, sigma.ptr, None), "update_view")
    d, s, n = depth.numpy(), sigma.numpy(), normal.numpy()
    assert (d > 0).sum() > W * H // 2 and (s > 0).sum() > W * H // 2 and not s[:2].any()
    assert_same_image(run_map(hip, vis, "depth", d, src_dev=depth), IT.depth_to_uchar4(d), "view depth")
    assert_same_image(run_map(hip, vis, "weight", s, src_dev=sigma), IT.weight_to_uchar4(s), "view uncertainty")
    assert_same_image(run_map(hip, vis, "normal", n, src_dev=normal), IT.normal_to_uchar4(n), "view normals")
    sc = T.Scenario(frames=2)
    ses = T.Session(hip, sc)
    for k in range(sc.frames):
        ses.frame(k, fused=True)
    n = ses.normals.numpy()
    assert (n[..., 3] < 0).any() and (n[..., 3] >= 0).sum() > W * H // 2          # holes and surface
    assert_same_image(run_map(hip, vis, "normal", n, src_dev=ses.normals), IT.normal_to_uchar4(n), "ICP normals map")
    ses.close()


def _stream(hip):
    p = C.c_void_p()
    hip.check(hip.fn["stream_create"](C.byref(p)), "stream_create")
    return p.value


@pytest.mark.gpu
def test_call_right_behind_an_asynchronous_upload_on_its_stream(hip, vis):
    """A non-blocking stream: upload from page-locked memory and the map behind it with no synchronise in between."""
    kind, src = IC.ALL_CASES["depth_vga"]
    st = _stream(hip)
    host = C.c_void_p()
    hip.check(hip.fn["host_malloc"](C.byref(host), src.nbytes), "host_malloc")
    try:
        C.memmove(host.value, src.ctypes.data, src.nbytes)
        s = hip.to_backend(np.full(src.shape, -1, F))
        d = hip.to_backend(np.full(src.shape + (4,), 0xCD, np.uint8))
        hip.check(hip.fn["memcpy_h2d"](s.ptr, host, src.nbytes, st), "memcpy_h2d")
        vis.DepthToUchar4(d, s, (src.shape[1], src.shape[0]), st)
        assert_same_image(d.numpy(st), IT.depth_to_uchar4(src), "behind the upload")
    finally:
        hip.sync(st)
        hip.fn["host_free"](host)
        hip.fn["stream_destroy"](st)


@pytest.mark.gpu
def test_two_streams_do_not_share_their_limits(hip, vis):
    """Two different images (limits far apart) mapped on two streams, issued alternately: both come out right, every round."""
    a = IC.ALL_CASES["depth_vga"][1]
    # other pixels AND other limits (both maps are invariant under a rescaling of one image, so a rescaled copy would not do)
    b0 = IC.depth_image(a.shape[1], a.shape[0], 555)
    b = np.where(b0 > 0, b0 * F(7) + F(20), b0).astype(F)
    wa = IC.ALL_CASES["weight_vga"][1]
    wb0 = IC.uncertainty_image(wa.shape[1], wa.shape[0], 556)
    wb = np.where(wb0 > 0, wb0 * F(50), wb0).astype(F)
    s1, s2 = _stream(hip), _stream(hip)
    try:
        size = (a.shape[1], a.shape[0])
        da, db, dwa, dwb = (hip.to_backend(x) for x in (a, b, wa, wb))
        rounds = 6
        outs = [[hip.to_backend(np.full(a.shape + (4,), 0xCD, np.uint8)) for _ in range(4)] for _ in range(rounds)]
        for r in range(rounds):
            vis.DepthToUchar4(outs[r][0], da, size, s1)
            vis.DepthToUchar4(outs[r][1], db, size, s2)
            vis.WeightToUchar4(outs[r][2], dwa, size, s1)
            vis.WeightToUchar4(outs[r][3], dwb, size, s2)
        hip.sync(s1); hip.sync(s2)
        want = [IT.depth_to_uchar4(a), IT.depth_to_uchar4(b), IT.weight_to_uchar4(wa), IT.weight_to_uchar4(wb)]
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[2], want[3])
        # with the other image's limits either image would come out differently: sharing a slot would show
        assert IT.depth_limits(a) != IT.depth_limits(b) and IT.weight_limit(wa) != IT.weight_limit(wb)
        for r in range(rounds):
            for i in range(4):
                assert_same_image(outs[r][i].numpy(), want[i], f"round {r}, image {i}")
    finally:
        hip.sync(s1); hip.sync(s2)
        hip.fn["stream_destroy"](s1); hip.fn["stream_destroy"](s2)


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip, vis):
    d = hip.to_backend(np.zeros((4, 4, 4), np.uint8))
    s = hip.to_backend(np.zeros((4, 4, 4), F))
    for fn in MAP_FUNCTIONS:
        assert hip.fn[fn](None, d.ptr, 4, 4, None) == capi.ERR_INVALID
        assert hip.fn[fn](s.ptr, None, 4, 4, None) == capi.ERR_INVALID
        assert hip.fn[fn](s.ptr, d.ptr, 0, 4, None) == capi.ERR_INVALID
    # an image that is not 16-byte aligned takes the one-pixel path of the depth map
    src = IC.ALL_CASES["depth_odd"][1]
    big = hip.to_backend(np.concatenate([np.zeros(1, F), src.reshape(-1)]))
    out = hip.to_backend(np.full(src.size * 4 + 4, 0xCD, np.uint8))
    hip.check(hip.fn["depth_to_uchar4"](big.ptr + 4, out.ptr + 4, src.shape[1], src.shape[0], None), "depth_to_uchar4")
    got = out.numpy()
    assert np.all(got[:4] == 0xCD)
    assert_same_image(got[4:].reshape(src.shape + (4,)), IT.depth_to_uchar4(src), "unaligned")


# ---- GPU: GetImage through the demo --------------------------------------------------------------------------------------------------

FREE_POSE = synth.pose_matrix_yaw((F(0.35), F(0.05), F(-0.2)), 0.2)          # beside the tracked trajectory, turned towards the sphere
FREE_SIZE, FREE_SIZE2 = (400, 300), (256, 192)
TYPES = ["original_rgb", "original_depth", "sceneraycast", "freecamera_shaded", "freecamera_colour_from_volume", "freecamera_colour_from_normal", "unknown"]
RENDER = {"freecamera_shaded": capi.RENDER_SHADED_GREYSCALE, "freecamera_colour_from_volume": capi.RENDER_COLOUR_FROM_VOLUME,
          "freecamera_colour_from_normal": capi.RENDER_COLOUR_FROM_NORMAL}


def run_demo(tmp_path, q, tag, voxel=capi.VOXEL_S, index=capi.INDEX_HASH, from_host=False, every_frame=False, scene_digest=False, second_size=True):
    out = os.path.join(str(tmp_path), tag)
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "sequence.bin")
    fs2 = FREE_SIZE2 if second_size else (0, 0)
    with open(path, "wb") as f:
        f.write(struct.pack("16i", W, H, q["n"], q["tracker"], q["approx"], q["skip"], 0 if q["poses"] is None else 1, voxel, index, int(from_host),
                            int(every_frame), FREE_SIZE[0], FREE_SIZE[1], fs2[0], fs2[1], int(scene_digest)))
        f.write(q["intr"].tobytes()); f.write(np.asarray(FREE_POSE, F).tobytes())
        f.write(np.array(synth.intrinsics_for(*FREE_SIZE), F).tobytes()); f.write(np.array(synth.intrinsics_for(*FREE_SIZE2), F).tobytes())
        f.write(q["raw"].tobytes())
        if q["poses"] is not None:
            f.write(q["poses"].tobytes())
        f.write(q["fusion"].tobytes()); f.write(q["main"].tobytes())
    r = subprocess.run([build_demo(), path, out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")]
    res = {"frames": [e for e in lines if "k" in e], "images": {e["image"]: e for e in lines if "image" in e}, "dir": out}
    for e in lines:
        if "image" not in e and "k" not in e:
            res.update(e)
    return res


def image_of(res, name):
    e = res["images"][name]
    with open(os.path.join(res["dir"], name + ".bin"), "rb") as f:
        data = f.read()
    assert hashlib.sha256(data).hexdigest() == e["sha256"], name          # what the demo printed is the digest of what it wrote
    return np.frombuffer(data, np.uint8).reshape(e["h"], e["w"], 4)


def load(res, name, dtype, shape):
    return np.fromfile(os.path.join(res["dir"], name), dtype).reshape(shape)


def short_sequence(kind, n):
    q = TM.sequence(kind)
    q = dict(q, n=n, raw=q["raw"][:n], poses=None if q["poses"] is None else q["poses"][:n], fusion=np.ones(n, np.uint8), main=np.ones(n, np.uint8))
    return q


def oracle_free_camera(q, frames, voxel, index, colour, renders):
    """The project's CPU oracle: its own scene fused with the frames the engine fused (at the poses the engine reports), then
    FindVisibleBlocks / CreateExpectedDepths / RenderImage from the free pose, per (name, size, type)."""
    be = T.oracle_backend()
    scene = be.create_scene(voxel, index, capi.default_params(voxelSize=0.005))
    scene.reco.ResetScene()
    rs = scene.vis.CreateRenderState((W, H))
    rgb = be.to_backend(synth.rgb_frame(W, H)) if colour else None
    intr = tuple(float(v) for v in q["intr"])
    for k in range(q["n"]):
        if not (q["fusion"][k] and q["main"][k]):
            continue
        depth = be.to_backend(synth.depth_from_raw(q["raw"][k]))
        v = capi.View(depth, W, H, M_d=np.array(frames[k]["pose"], F), intr_d=intr, rgb=rgb, w_rgb=W, h_rgb=H, intr_rgb=intr)
        scene.reco.AllocateSceneFromDepth(v, rs)
        scene.reco.IntegrateIntoScene(v, rs)
    # ONE free-view state, as the engine keeps it: created at the first size, created anew when the asked size differs.  The renders
    # are made in the engine's order, for the colour-from-normal render writes r, g, b only (drawPixelNormal): its alpha is what the
    # state's image held before -- the shaded render's at the same size, 0 in a new state.
    out = {}
    free, free_size = None, None
    for name, size, rtype in renders:
        if free_size != size:
            if free is not None:
                free.close()
            free, free_size = scene.vis.CreateRenderState(size), size
        fintr = synth.intrinsics_for(*size)
        scene.vis.FindVisibleBlocks(FREE_POSE, fintr, free)
        scene.vis.CreateExpectedDepths(FREE_POSE, fintr, free)
        scene.vis.RenderImage(FREE_POSE, fintr, free, None, rtype)
        out[name] = scene.download(capi.BUF_RAYCAST_IMAGE, free).copy()
    if free is not None:
        free.close()
    rs.close(); scene.close()
    return out


def check_images(res, q, voxel, index, wicp=False):
    colour = voxel in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)
    assert res["before_first_frame_untouched"] == 1 and res["before_first_frame_no_device_image"] == 1
    assert res["image_size"] == [W, H]
    want_types = [t for t in TYPES if colour or t != "freecamera_colour_from_volume"]
    assert [n for n in res["images"] if "_size" not in n] == want_types
    for name, e in res["images"].items():
        assert e["device_equal"] == (-1 if name == "unknown" else 1), (name, e)      # GetImageDevice holds the bytes GetImage copies
    # ORIGINAL_RGB: the input
    assert_same_image(image_of(res, "original_rgb"), synth.rgb_frame(W, H), "original_rgb")
    assert np.array_equal(load(res, "rgb_input.bin", np.uint8, (H, W, 4)), synth.rgb_frame(W, H))
    # ORIGINAL_DEPTH: the colour map of the downloaded view depth / the weight map of the uncertainty image
    depth = load(res, "view_depth.bin", F, (H, W))
    assert (depth > 0).sum() > W * H // 2
    if wicp:
        sigma = load(res, "view_uncertainty.bin", F, (H, W))
        assert (sigma > 0).sum() > W * H // 2 and not sigma[:2].any() and not sigma[:, :2].any()
        assert_same_image(image_of(res, "original_depth"), IT.weight_to_uchar4(sigma), "original_depth (weighted ICP: uncertainty)")
    else:
        assert_same_image(image_of(res, "original_depth"), IT.depth_to_uchar4(depth), "original_depth")
    # SCENERAYCAST: the live render state's image
    live = load(res, "live_raycast_image.bin", np.uint8, (H, W, 4))
    assert live.any()
    assert_same_image(image_of(res, "sceneraycast"), live, "sceneraycast")
    # UNKNOWN: cleared, at the size handed in
    unknown = image_of(res, "unknown")
    assert unknown.shape == (FREE_SIZE[1], FREE_SIZE[0], 4) and not unknown.any()
    # the free camera against the oracle
    renders = [(n, FREE_SIZE, RENDER[n]) for n in want_types if n in RENDER]
    if "freecamera_shaded_second_size" in res["images"]:
        renders += [("freecamera_shaded_second_size", FREE_SIZE2, capi.RENDER_SHADED_GREYSCALE),
                    ("freecamera_colour_from_normal_first_size_again", FREE_SIZE, capi.RENDER_COLOUR_FROM_NORMAL)]
    want = oracle_free_camera(q, res["frames"], voxel, index, colour, renders)
    for name, size, _ in renders:
        got = image_of(res, name)
        assert got.shape == (size[1], size[0], 4), name
        assert np.count_nonzero(got.any(-1)) > size[0] * size[1] // 5, name + ": the free camera sees the scene"
        assert_same_image(got, want[name], name)
    assert not np.array_equal(image_of(res, "freecamera_shaded")[..., :3], image_of(res, "freecamera_colour_from_normal")[..., :3])


@pytest.mark.gpu
def test_get_image_after_the_main_engine_sequence(tmp_path):
    """The `external` sequence of tests/test_main_engine.py (integration and main processing switched off for some frames, forward
    renders in between), ITMVoxel_s in a hash: every GetImage type, and a second free-camera call at another size."""
    q = TM.sequence("external")
    res = run_demo(tmp_path, q, "external")
    with open(TM.GOLDEN) as f:
        want = json.load(f)["external"]
    assert [(e["age"], e["full"]) for e in res["frames"]] == [(e["age"], e["full"]) for e in want]      # the same run as the reference's objects
    assert np.array_equal(np.array([e["pose"] for e in res["frames"]], F), np.array([e["pose"] for e in want], F))
    check_images(res, q, capi.VOXEL_S, capi.INDEX_HASH)


@pytest.mark.gpu
def test_get_image_original_depth_under_the_weighted_icp_tracker(tmp_path):
    q = dict(short_sequence("icp", 4), tracker=4)
    res = run_demo(tmp_path, q, "wicp", second_size=False)
    check_images(res, q, capi.VOXEL_S, capi.INDEX_HASH, wicp=True)


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,index", [(capi.VOXEL_S, capi.INDEX_DENSE), (capi.VOXEL_F_RGB, capi.INDEX_HASH), (capi.VOXEL_F_RGB, capi.INDEX_DENSE)],
                         ids=["s-dense", "f_rgb-hash", "f_rgb-dense"])
def test_get_image_free_camera_per_voxel_and_index_type(tmp_path, voxel, index):
    q = short_sequence("external", 3)
    res = run_demo(tmp_path, q, "types", voxel=voxel, index=index, second_size=False)
    check_images(res, q, voxel, index)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,from_host", [("external", False), ("external", True), ("icp", False), ("icp", True)],
                         ids=["external", "external-from-host-announced", "icp", "icp-from-host-announced"])
def test_get_image_does_not_disturb_tracking_or_fusion(tmp_path, kind, from_host):
    """GetImage of every type after every frame: the same poses, tracking maps, visible lists, range images and scene as without --
    with deferred fusion on (ITMScene switches it on) and, from_host, with ProcessFrameFromHost announcing the next frame."""
    q = TM.sequence(kind)
    plain = run_demo(tmp_path, q, "plain", from_host=from_host, every_frame=False, scene_digest=True, second_size=False)
    busy = run_demo(tmp_path, q, "busy", from_host=from_host, every_frame=True, scene_digest=True, second_size=False)
    assert len(plain["frames"]) == len(busy["frames"]) == q["n"]
    for a, b in zip(plain["frames"], busy["frames"]):
        assert a == b, (a, b)
    assert plain["scene_digest"] == busy["scene_digest"] and plain["scene_digest"][1] != "0" * 16
    for name in plain["images"]:
        assert plain["images"][name]["sha256"] == busy["images"][name]["sha256"], name

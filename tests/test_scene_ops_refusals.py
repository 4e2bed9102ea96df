"""The refusals that the scene operations share (infinitam_amd/csrc/scene_ops.h: check_scene_pair, check_slot_list, enter_scene_pair,
refuse_ahead; merge_device.h: refuse_bad_slots), text for text: itm_scene_merge, _coarsen and _resample on pairs of scenes, itm_scene_prune
and itm_scene_band_samples on one.  Every case is ITM_ERR_INVALID and itm_last_error EQUAL to the string below -- the strings the five
entry points carried, each in its own copy, before the refusals were stated once.  The suites of the single operations check that a
refusal leaves dst untouched; this file checks what it says.  Tiny tables (bucketNum 0x400, excessNum 0x100), one frame in the
scenes that hold the block requests of a frame issued ahead, none in the others."""
import ctypes as C

import numpy as np
import pytest

import itm_testlib as T
from infinitam_amd import capi

W, H = 160, 120
FINE, COARSE, MU = 0.01, 0.02, 0.04
TABLE = dict(bucketNum=0x400, excessNum=0x100, localBlockNum=0x400)
ENTRIES = 0x400 + 0x100
_P = C.c_void_p

AHEAD = "dst holds the block requests of a frame issued ahead (itm_cancel_ahead first)"
# reason -> text, per operation; None: the operation does not refuse that
PAIR_TEXTS = {
    "scene merge": dict(null="null scene", same="dst and src are the same scene", voxelType="the scenes differ in voxelType", indexType="the scenes differ in indexType",
                        voxelSize="the scenes differ in voxelSize", mu=None, dense_list="a slot list with dense scenes", negative="negative slot count",
                        outside="a slot of the list is outside src's table", ahead=AHEAD),
    "scene coarsen": dict(null="null scene", same="dst and src are the same scene", voxelType="the scenes differ in voxelType", indexType="the scenes differ in indexType",
                          voxelSize="dst's voxelSize is not twice src's", mu="the scenes differ in mu", dense_list="a slot list with dense scenes",
                          negative="negative slot count", outside="a slot of the list is outside src's table", ahead=AHEAD),
    "scene resample": dict(null="null scene", same="dst and src are the same scene", voxelType="the scenes differ in voxelType", indexType="the scenes differ in indexType",
                           voxelSize="the scenes differ in voxelSize", mu="the scenes differ in mu", dense_list="a slot list with dense scenes",
                           negative="negative slot count", outside="a slot of the list is outside src's table", ahead=AHEAD),
}


def up(x):
    return float(np.nextafter(np.float32(x), np.float32(1)))


def session_ahead(hip, size):
    """A session whose scene holds one frame and the block requests of the next."""
    ses = T.Session(hip, T.Scenario(name="refusals", w=W, h=H, voxelSize=size, mu=MU, frames=2, **TABLE))
    v = [capi.View(hip.to_backend(ses.sc.depth(k)), W, H, M_d=ses.sc.pose(k), intr_d=ses.sc.intr()) for k in range(2)]
    ses.scene.process_frame_ahead(v[0], v[1], ses.rs, ses.points, ses.normals)
    return ses


class Scenes:
    """The empty scenes of all cases, built once."""

    def __init__(self, hip):
        self.hip = hip
        self.plain = []
        self.fine, self.coarse = self.scene(), self.scene(size=COARSE)
        self.float_type, self.off_size, self.off_mu = self.scene(voxel=capi.VOXEL_F), self.scene(size=up(FINE)), self.scene(mu=up(MU))
        dense = dict(index=capi.INDEX_DENSE, denseSize=(16, 16, 16))
        self.dense, self.dense_twin, self.dense_coarse = self.scene(**dense), self.scene(**dense), self.scene(size=COARSE, **dense)
        self.dense_other = self.scene(index=capi.INDEX_DENSE, denseSize=(16, 16, 24))

    def scene(self, voxel=capi.VOXEL_S, index=capi.INDEX_HASH, size=FINE, mu=MU, **kw):
        if index == capi.INDEX_HASH:
            kw.update(TABLE)
        s = self.hip.create_scene(voxel, index, capi.default_params(voxelSize=size, mu=mu), **kw)
        s.reco.ResetScene()
        self.plain.append(s)
        return s

    def close(self):
        for s in self.plain:
            s.close()


@pytest.fixture(scope="module")
def scenes(hip):
    s = Scenes(hip)
    yield s
    s.close()


def call(hip, name, dst, src, slots=None, n=None, q="identity"):
    """rc and itm_last_error of one call through the C ABI (no statistics, the null stream)."""
    dev = hip.to_backend(np.asarray(slots, np.int32)) if slots is not None else None
    count = (len(slots) if slots is not None else 0) if n is None else n
    args = [_P(dst.h if dst else None), _P(src.h if src else None)]
    if name == "scene resample":
        cq = capi.rigid_quantise(np.eye(4, dtype=np.float32), FINE, hip) if q == "identity" else q
        args.append(C.byref(cq) if cq is not None else None)
    rc = hip.fn[name.replace(" ", "_")](*args, _P(dev.ptr if dev else None), count, None, None)
    hip.sync()
    text = (hip.fn["last_error"]() or b"").decode()
    if dev is not None:
        dev.close()
    return rc, text


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene merge", "scene coarsen", "scene resample"])
def test_pair_refusals_say_what_they_said(hip, scenes, name):
    S, texts = scenes, PAIR_TEXTS[name]
    ses = session_ahead(hip, COARSE if name == "scene coarsen" else FINE)
    dst, dense_dst = ses.scene, (S.dense_coarse if name == "scene coarsen" else S.dense_twin)

    def refused(reason, d, s, **kw):
        rc, text = call(hip, name, d, s, **kw)
        print(name, reason, rc, repr(text))
        assert rc == capi.ERR_INVALID and text == name + ": " + texts[reason], (name, reason, rc, text)

    # dst holds the requests of a frame issued ahead all the while: the argument refusals come first, whatever the scenes hold
    refused("null", None, S.fine)
    refused("null", dst, None)
    refused("same", dst, dst)
    refused("voxelType", dst, S.float_type)
    refused("indexType", dst, S.dense)
    refused("voxelSize", dst, S.off_size)
    if name == "scene coarsen":
        refused("voxelSize", dst, S.coarse)                  # equal sizes
    if texts["mu"]:
        refused("mu", dst, S.off_mu)
    refused("dense_list", dense_dst, S.dense, slots=[0])
    refused("negative", dst, S.fine, slots=[0, 1], n=-2)
    refused("ahead", dst, S.fine)
    refused("ahead", dst, S.fine, slots=[ENTRIES])           # (the list is looked at after dst has been found free)
    if name == "scene resample":
        rc, text = call(hip, name, dst, S.fine, q=None)
        assert rc == capi.ERR_INVALID and text == "scene resample: null transform", text
        rc, text = call(hip, name, None, S.fine, q=None)
        assert rc == capi.ERR_INVALID and text == "scene resample: null scene", text
    if name == "scene merge":
        rc, text = call(hip, name, S.dense_other, S.dense)
        assert rc == capi.ERR_INVALID and text == "scene merge: dense scenes differ in denseSize / denseOffset", text
        rc, text = call(hip, name, S.dense_other, S.dense, slots=[0])          # ... which comes before the slot list's refusal
        assert rc == capi.ERR_INVALID and text == "scene merge: dense scenes differ in denseSize / denseOffset", text
    ses.close()


@pytest.mark.gpu
def test_refusals_of_a_free_dst_and_of_single_scenes(hip, scenes):
    """After itm_cancel_ahead: a slot outside src's table, for the three pair operations and band samples; prune's and band samples' own;
    and merge goes through between two scenes that differ in mu alone."""
    S = scenes
    fine, coarse = session_ahead(hip, FINE), session_ahead(hip, COARSE)
    # prune, while the scene still holds the requests
    cfg = fine.scene.prune_config()
    rc = hip.fn["scene_prune"](_P(fine.scene.h), C.byref(cfg), None, None, None)
    assert rc == capi.ERR_INVALID and hip.fn["last_error"]().decode() == "scene prune: the scene holds the block requests of a frame issued ahead (itm_cancel_ahead first)"
    fine.scene.cancel_ahead(fine.rs)
    coarse.scene.cancel_ahead(coarse.rs)
    for name, dst in (("scene merge", S.fine), ("scene coarsen", coarse.scene), ("scene resample", S.fine)):
        for slots in ([0, ENTRIES, 3], [-1]):
            rc, text = call(hip, name, dst, fine.scene, slots=slots)
            assert rc == capi.ERR_INVALID and text == name + ": " + PAIR_TEXTS[name]["outside"], (name, slots, rc, text)
    # band samples: one scene
    acfg = fine.scene.align_config()

    def band(scene, slots, n=None):
        dev = hip.to_backend(np.asarray(slots, np.int32))
        rc = hip.fn["scene_band_samples"](_P(scene.h), _P(dev.ptr), len(slots) if n is None else n, C.byref(acfg), None, 0, C.byref(C.c_int32()), None)
        hip.sync()
        dev.close()
        return rc, hip.fn["last_error"]().decode()

    assert band(S.dense, [0]) == (capi.ERR_INVALID, "band samples: a slot list with a dense scene")
    assert band(fine.scene, [0, 1], n=-2) == (capi.ERR_INVALID, "band samples: negative slot count")
    assert band(fine.scene, [0, ENTRIES]) == (capi.ERR_INVALID, "band samples: a slot of the list is outside src's table")
    assert band(fine.scene, [-1]) == (capi.ERR_INVALID, "band samples: a slot of the list is outside src's table")
    # merge does not compare mu (tests/scene_merge_terms.py: the combine works on the stored fractions of mu)
    held = int(np.count_nonzero(fine.scene.download(capi.BUF_HASH_ENTRIES)["ptr"] >= 0))
    stats = S.off_mu.merge_from(fine.scene)
    assert held > 100 and stats["considered"] == held and stats["allocated"] > 0, (held, stats)
    fine.close(); coarse.close()

"""Times itm_mesh_update (touch included) against itm_mesh_scene on the same scene states (profiles/mesh_update_notes.md): host
milliseconds per call, from the call to the stream idle.  python tools/mesh_update_bench.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import itm_testlib as T  # noqa: E402
from infinitam_amd import capi  # noqa: E402
from infinitam_amd.capi import Mesh  # noqa: E402

be = T.hip_backend()
out = {"six_frames": [], "exploring": [], "equal_case": {}}


def timed(fn):
    be.sync()
    t = time.perf_counter()
    r = fn()
    be.sync()
    return (time.perf_counter() - t) * 1e3, r


def touch_update(m, rs):
    m.Touch(rs)
    return m.Update()


def measure(ses, m, full, k):
    t_first, stats = timed(lambda: touch_update(m, ses.rs))
    reps = [timed(lambda: touch_update(m, ses.rs)) for _ in range(5)]            # the same marks again: nothing appears, D is the marked set
    t_full = min(timed(full.MeshScene)[0] for _ in range(5))
    rep_stats = reps[-1][1]
    return dict(frame=k, update_ms=round(t_first, 3), update_again_ms=round(min(r[0] for r in reps), 3), mesh_scene_ms=round(t_full, 3),
                allocated=stats["allocated"], remeshed=stats["remeshed"], remeshed_again=rep_stats["remeshed"], full=stats["full"],
                triangles=stats["trianglesAfter"], bytes_copied=stats["trianglesCopied"] * 36, bytes_copied_again=rep_stats["trianglesCopied"] * 36)


def warm(m):
    m.MeshScene()
    m.Touch(slots=[])
    m.Update()                                                                   # allocates the second buffer


sc = T.Scenario(name="mesh_update", w=160, h=120, voxelSize=0.01, frames=6, trajectory="yaw", yaw_rate=0.3)
ses = T.Session(be, sc)
ses.frame(0, fused=True)
m, full = Mesh(ses.scene), Mesh(ses.scene)
warm(m)
for k in range(1, 6):
    ses.frame(k, fused=True)
    out["six_frames"].append(measure(ses, m, full, k))
    print(out["six_frames"][-1], flush=True)
# D = A': every listed slot touched, through the incremental path; and the full path of a handle without a run table
table = ses.scene.download(capi.BUF_HASH_ENTRIES)
listed = np.nonzero(table["ptr"] >= 0)[0].astype(np.int32)
dev = be.to_backend(listed)
ts = []
for _ in range(5):
    m.Touch(slots=dev)
    ts.append(timed(m.Update))
out["equal_case"] = dict(update_ms=round(min(t[0] for t in ts), 3), remeshed=ts[-1][1]["remeshed"], allocated=ts[-1][1]["allocated"], full=ts[-1][1]["full"],
                         mesh_scene_ms=out["six_frames"][-1]["mesh_scene_ms"])
m.Touch(everything=True)
t, st = timed(m.Update)
out["equal_case"].update(everything_ms=round(t, 3), everything_full=st["full"])
print(out["equal_case"], flush=True)
m.close(); full.close(); ses.close()

sc = T.Scenario(name="exploring", w=640, h=480, voxelSize=0.005, frames=161, trajectory="parity")
ses = T.Session(be, sc)
ses.frame(0, fused=True)
m, full = Mesh(ses.scene), Mesh(ses.scene)
warm(m)
for k in range(1, 161):
    ses.frame(k, fused=True)
    if k in (40, 80, 160):
        out["exploring"].append(measure(ses, m, full, k))
        print(out["exploring"][-1], flush=True)
    else:
        touch_update(m, ses.rs)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)

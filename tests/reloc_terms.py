"""The keyframe relocaliser's sequential definition (include/itm_hip.h, itm_reloc_*) restated in float32 numpy: small image, fern
code, nearest-code search, harvesting, and the default configuration and ferns.  Every product and every sum is rounded to float32
on its own, in the order of the definition; integer work is exact."""
import numpy as np

F32 = np.float32
MAX_K = 8
MASK64 = (1 << 64) - 1


# ---- 5. defaults --------------------------------------------------------------------------------------------------------------------
def default_levels(w):
    L = 0
    while (w >> L) > 40:
        L += 1
    return L


def default_taps():
    return np.array([np.exp(-float(i * i) / (2 * 2.5 * 2.5)) for i in range(7)], np.float64).astype(F32)


class SplitMix64:
    def __init__(self, seed):
        self.x = int(seed) & MASK64

    def next(self):
        self.x = (self.x + 0x9E3779B97F4A7C15) & MASK64
        z = self.x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)


def default_ferns(ws, hs, F, D, seed, lo=0.2, hi=3.0):
    g = SplitMix64(seed)
    n = F * D
    pixel, threshold = np.zeros(n, np.int32), np.zeros(n, F32)
    lo, hi = F32(lo), F32(hi)
    for i in range(n):
        pixel[i] = (g.next() >> 32) % (ws * hs)
        u = F32(F32(g.next() >> 40) * F32(1.0 / 16777216.0))      # a 24-bit integer: exact in float32
        threshold[i] = F32(lo + F32(F32(hi - lo) * u))
    return pixel, threshold


# ---- 1. image -----------------------------------------------------------------------------------------------------------------------
def subsample(img):
    """FilterSubsampleWithHoles: the valid ones of the four pixels under an output pixel, summed in the order (0,0) (1,0) (0,1) (1,1)."""
    img = np.asarray(img, F32)
    h, w = img.shape[0] // 2, img.shape[1] // 2
    acc, good = np.zeros((h, w), F32), np.zeros((h, w), F32)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        v = img[dy:2 * h:2, dx:2 * w:2]
        ok = v > 0
        acc = np.where(ok, (acc + v).astype(F32), acc)
        good = np.where(ok, good + F32(1), good)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(good > 0, (acc / good).astype(F32), acc).astype(F32)


def blur_pass(img, taps, R, axis):
    img = np.asarray(img, F32)
    s, n = np.zeros(img.shape, F32), np.zeros(img.shape, F32)
    size = img.shape[axis]
    for i in range(-R, R + 1):
        t = F32(taps[abs(i)])
        v = np.zeros(img.shape, F32)      # the input at offset i along the axis; 0 (never used) outside the image
        src = [slice(None)] * 2
        dst = [slice(None)] * 2
        if i >= 0:
            src[axis], dst[axis] = slice(i, size), slice(0, max(size - i, 0))
        else:
            src[axis], dst[axis] = slice(0, max(size + i, 0)), slice(-i, size)
        v[tuple(dst)] = img[tuple(src)]
        ok = v > 0
        s = np.where(ok, (s + (t * v).astype(F32)).astype(F32), s)
        n = np.where(ok, (n + t).astype(F32), n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, (s / n).astype(F32), F32(0)).astype(F32)


def small_image(depth, levels, R, taps):
    img = np.asarray(depth, F32)
    for _ in range(levels):
        img = subsample(img)
    if R > 0:
        img = blur_pass(img, taps, R, axis=1)      # along x first
        img = blur_pass(img, taps, R, axis=0)
    return img


# ---- 2. code ------------------------------------------------------------------------------------------------------------------------
def encode(S, pixel, threshold, F, D):
    bits = (np.asarray(S, F32).reshape(-1)[np.asarray(pixel).reshape(F, D)] > np.asarray(threshold, F32).reshape(F, D))
    return (bits.astype(np.uint32) << np.arange(D, dtype=np.uint32)).sum(axis=1).astype(np.uint8)


# ---- 3. search ----------------------------------------------------------------------------------------------------------------------
def search(db, q, k):
    """db uint8[count, F], q uint8[F] -> (ids int32[k], dist float32[k])."""
    db = np.asarray(db, np.uint8)
    F = len(q)
    ids, dist = np.full(k, -1, np.int32), np.ones(k, F32)
    if len(db):
        sim = (db == np.asarray(q, np.uint8)[None, :]).sum(axis=1).astype(np.int64)
        order = np.lexsort((np.arange(len(db)), -sim))[:k]      # sim descending, then id ascending
        ids[:len(order)] = order
        dist[:len(order)] = (F - sim[order]).astype(F32) / F32(F)
    return ids, dist


# ---- 4. harvest ---------------------------------------------------------------------------------------------------------------------
class Database:
    def __init__(self, F, capacity):
        self.F, self.capacity = F, capacity
        self.codes, self.poses = [], []

    def rows(self):
        return np.array(self.codes, np.uint8).reshape(-1, self.F)

    def process(self, code, pose, harvest, threshold, k):
        ids, dist = search(self.rows(), code, k)
        added = -1
        if harvest and (len(self.codes) == 0 or dist[0] > F32(threshold)):
            if len(self.codes) >= self.capacity:
                added = -2
            else:
                added = len(self.codes)
                self.codes.append(np.array(code, np.uint8))
                self.poses.append(np.array(pose, F32).reshape(16))
        return ids, dist, added

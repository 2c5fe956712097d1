"""COCO run-length encoded masks restated in numpy (not a test): the decode that krrn_rle_decode_u8 must equal
(include/krrn_hip.h: run parity repeated by run length, reshaped column-major), `info` taken from the decoded plane,
an encoder, the compressed string codec written independently of pose_estimation_amd/rle.py, and the masks the
tests run on."""
import numpy as np

CHUNK = 256                                              # kMaskThreads of csrc/krrn_mask.h: runs per step of mask_scan_runs
SIZES = ((5, 3), (16, 16), (21, 37), (41, 50), (48, 64), (480, 640))   # H x W
# two literal vectors of the string form (made by a restatement of the published algorithm; not cross-checked with
# pycocotools, which is not a dependency)
VECTORS = (([6, 1, 40, 4, 5, 4, 5, 4, 21], "61X13mN000`0"), ([0, 3, 40, 2, 1000, 2, 5], "03X1OPn00mPO"))


def decode(counts, H, W):
    """u8 [H, W] of 0 / 1 from runs that sum to H * W."""
    c = np.asarray(counts, np.int64)
    assert (c >= 0).all() and int(c.sum()) == H * W, (int(c.sum()), H * W)
    flat = np.repeat((np.arange(len(c)) & 1).astype(np.uint8), c)
    return np.ascontiguousarray(flat.reshape(W, H).T)


def info(plane):
    """int32 [5] = (pixel count, x, y, w, h), w = x_max - x_min, h = y_max - y_min; zeros for an empty mask."""
    ys, xs = np.nonzero(plane)
    if len(ys) == 0:
        return np.zeros(5, np.int32)
    return np.array([len(ys), xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()], np.int32)


def encode(plane):
    """Runs of a [H, W] mask, walking the pixels column-major one by one."""
    runs, cur, n = [], 0, 0
    for v in (np.asarray(plane) != 0).T.reshape(-1).tolist():
        if int(v) != cur:
            runs.append(n)
            cur, n = int(v), 0
        n += 1
    runs.append(n)
    return runs


def to_string(counts):
    """COCO's rleToString: deltas against the value two places back from the fourth value on, then 5-bit groups,
    least significant first, each + 48, with 0x20 marking that another group follows."""
    out = []
    for i, v in enumerate(counts):
        x = int(v) - (int(counts[i - 2]) if i > 2 else 0)
        while True:
            low = x % 32                                 # Python's % is non-negative: the two's-complement low bits
            x = (x - low) // 32
            done = (x == 0 and low < 16) or (x == -1 and low >= 16)
            out.append(chr(48 + low + (0 if done else 32)))
            if done:
                break
    return "".join(out)


def from_string(s):
    """COCO's rleFrString."""
    vals, pos = [], 0
    while pos < len(s):
        groups = []
        while True:
            g = ord(s[pos]) - 48
            pos += 1
            groups.append(g % 32)
            if g < 32:
                break
        x = sum(g * 32 ** k for k, g in enumerate(groups))
        if groups[-1] >= 16:
            x -= 32 ** len(groups)
        if len(vals) > 2:
            x += vals[-2]
        vals.append(x)
    return vals


def n_runs(HW, n):
    """n runs that sum to HW: n - 1 of one pixel, then the rest."""
    assert HW >= n - 1
    return [1] * (n - 1) + [HW - (n - 1)]


def disc(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy - 0.52 * H) / (0.37 * H)) ** 2 + ((xx - 0.45 * W) / (0.28 * W)) ** 2 <= 1.0).astype(np.uint8)


def cases(H, W):
    """[(name, run list)] for an H x W frame: the edge masks of every size, plus the ones that belong to one size."""
    HW = H * W
    rng = np.random.default_rng(1000 * H + W)
    out = [("zeros", [HW]),
           ("ones", [0, HW]),
           ("first_pixel", [0, 1, HW - 1]),
           ("last_pixel", [HW - 1, 1]),                  # an even number of runs
           ("three_columns", [H - 2, H + 4, HW - 2 * H - 2]),   # rows H-2, H-1, a whole column, rows 0, 1
           ("zero_runs", [3, 2, 0, 4, 0, 0, 1, HW - 10]),
           ("random", encode(rng.random((H, W)) < 0.3))]
    if (H, W) == (21, 37):
        out.append(("checkerboard", [0] + [1] * HW))     # 778 one-pixel runs: more than one scan chunk
        out += [(f"runs_{n}", n_runs(HW, n)) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)]
    if (H, W) == (480, 640):
        out.append(("disc", encode(disc(H, W))))
    return out

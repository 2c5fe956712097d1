"""Host restatement of the resized input path (krrn_crop_inputs_resize_u8, krrn_choose_points_resize), written from
the definition in include/krrn_hip.h / DESIGN.md §3 in numpy: integer index arithmetic, the bilinear blend in f64
with every product and sum a numpy operation of its own (so each is rounded once, as the kernel's are without FMA
contraction), f32 for the normalisation and the cloud. `choose` is tests/draws_ref.py's, over the T*T mask. The
device results are compared with array_equal, never with a tolerance. Nothing here imports the package.

A crop is the S x S window at (r0, c0) of a frame, resampled to T x T. Output index j sits at window coordinate
((2j+1) S - T) / (2T)."""
import numpy as np

from tests import draws_ref as D

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def taps(S: int, T: int):
    """Per output index j: (x0, xa, xb, w): the unclamped left tap floor(nx / D), the two taps clamped to
    [0, S - 1], and the right tap's f64 weight (nx - x0 D) / D."""
    j = np.arange(T, dtype=np.int64)
    nx, Dn = (2 * j + 1) * S - T, 2 * T
    x0 = nx // Dn  # numpy's integer // floors
    w = (nx - x0 * Dn).astype(np.float64) / np.float64(Dn)
    return x0, np.clip(x0, 0, S - 1), np.clip(x0 + 1, 0, S - 1), w


def nearest(S: int, T: int) -> np.ndarray:
    """The nearest source index of each output index's centre: ((2j+1) S) / (2T) by integer division."""
    j = np.arange(T, dtype=np.int64)
    return ((2 * j + 1) * S) // (2 * T)


def centre(S: int, T: int) -> np.ndarray:
    """Each output index's centre in window coordinates, f64: (double)nx / (double)D."""
    j = np.arange(T, dtype=np.int64)
    return ((2 * j + 1) * S - T).astype(np.float64) / np.float64(2 * T)


def bilinear(win: np.ndarray, T: int) -> np.ndarray:
    """win u8 [S][S][C] -> f64 [T][T][C]: top = (1 - wx) a[ya][xa] + wx a[ya][xb], bot on row yb,
    p = (1 - wy) top + wy bot."""
    S = win.shape[0]
    _, xa, xb, w = taps(S, T)
    a = win.astype(np.float64)
    wx, wy = w[None, :, None], w[:, None, None]
    ya, yb = xa, xb  # a square window to a square output: rows and columns share their taps
    top = (1.0 - wx) * a[ya][:, xa] + wx * a[ya][:, xb]
    bot = (1.0 - wx) * a[yb][:, xa] + wx * a[yb][:, xb]
    return (1.0 - wy) * top + wy * bot


def crop_inputs(rgb, depth, mask_label, r0, c0, S, T, obj_mask=None):
    """(img f32 [3][T][T], mask bool [T][T]) of one crop."""
    p = bilinear(rgb[r0:r0 + S, c0:c0 + S], T)
    x = (p / 255.).astype(np.float32).transpose(2, 0, 1)
    img = (x - MEAN[:, None, None]) / STD[:, None, None]
    n = nearest(S, T)
    sr, sc = (r0 + n)[:, None], (c0 + n)[None, :]
    m = (mask_label[sr, sc] != 0) & (depth[sr, sc] != 0)
    if obj_mask is not None:
        m &= obj_mask[sr, sc] != 0
    return img.astype(np.float32), m


def points(choose, depth, r0, c0, S, T, K4, depth_scale=1.0):
    """(cloud f32 [N][3], xmap f32 [N], ymap f32 [N]) of chosen pixels i*T + j: the maps are the resized pixels'
    centres in the frame, the cloud the back-projection of their nearest source pixels, in f32."""
    fx, fy, cx, cy = [np.float32(v) for v in K4]
    i, j = choose // T, choose % T
    ctr, n = centre(S, T), nearest(S, T)
    xm = (np.float64(c0) + ctr[j]).astype(np.float32)
    ym = (np.float64(r0) + ctr[i]).astype(np.float32)
    sr, sc = r0 + n[i], c0 + n[j]
    pt2 = depth[sr, sc].astype(np.float32) / np.float32(depth_scale)
    pt0 = (sc.astype(np.float32) - cx) * pt2 / fx
    pt1 = (sr.astype(np.float32) - cy) * pt2 / fy
    return np.stack([pt0, pt1, pt2], 1).astype(np.float32), xm, ym


def crop(rgb, depth, mask_label, r0, c0, S, T, N, K4, depth_scale=1.0, seed=0, stream_id=0, index=0, obj_mask=None):
    """Every output of crop number `index` of a batch: img, mask (u8 [T*T]), count, choose, cloud, xmap, ymap; an
    empty mask gives zeros and count 0."""
    img, m = crop_inputs(rgb, depth, mask_label, r0, c0, S, T, obj_mask)
    ch = D.choose(m, N, seed=seed, stream_id=stream_id, crop=index)
    if m.any():
        cloud, xm, ym = points(ch, depth, r0, c0, S, T, K4, depth_scale)
    else:
        cloud, xm, ym = np.zeros((N, 3), np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
    return {"img": img, "mask": m.reshape(-1).astype(np.uint8), "count": int(m.sum()), "choose": ch, "cloud": cloud,
            "xmap": xm, "ymap": ym}

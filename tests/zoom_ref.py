"""Host restatement of the zoom-in pass's window rule (krrn_pose_windows_f64), written from the definition in
include/krrn_hip.h / DESIGN.md §3 in numpy: all f64, every product and sum a numpy operation of its own (so each is
rounded once, as the kernel's are without FMA contraction), integer results. The device results are compared with
array_equal, never with a tolerance. Nothing here imports the package.

Per crop: project the model points under the pose; a point is bad unless Z > 0 and its pixel is finite, tested per
point; status 1 with a bad point, 2 when the points' box misses the frame, else 0 and a new square window centred on
the box, `pad` times its larger extent, at least min_side, shifted into the frame and never shrunk."""
import numpy as np


def project(pts, R, t, K4):
    """(u, v, Z) f64 [P] of points f32 [P, 3] under R f64 [9] row-major, t f64 [3] and K4 f32 [4], in the kernel's
    order: X = ((R00 x + R01 y) + R02 z) + t0, u = (fx X) / Z + cx."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = [np.float64(np.float32(k)) for k in np.asarray(K4).reshape(4)]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        X = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
        Y = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
        Z = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
        u = (fx * X) / Z + cx
        v = (fy * Y) / Z + cy
    return u, v, Z


def intrinsic(K4, r0, c0, S, T):
    """(scale f32, intr f32 [4]): s = S / T in f64, (fx / s, fy / s, (cx - c0 + 0.5) / s - 0.5, (cy - r0 + 0.5) / s -
    0.5) in f64 from the f32 K4, cast once."""
    fx, fy, cx, cy = [np.float64(np.float32(k)) for k in np.asarray(K4).reshape(4)]
    with np.errstate(all="ignore"):
        s = np.float64(S) / np.float64(T)
        intr = np.array([fx / s, fy / s, (cx - np.float64(c0) + 0.5) / s - 0.5, (cy - np.float64(r0) + 0.5) / s - 0.5],
                        np.float64)
        return np.float32(s), intr.astype(np.float32)


def window(pts, R, t, K4, H, W, T, pad, min_side, rc_in, side_in):
    """One crop: {"rc": (r0, c0), "side": S, "bbox": f32 [4], "scale": f32, "intr": f32 [4], "status": 0 / 1 / 2} and,
    for the tests' own properties, "box": (umin, umax, vmin, vmax) or None and "clamped": whether the side or a shift
    was clamped."""
    u, v, Z = project(pts, R, t, K4)
    # the per-point test, stated explicitly: `Z > 0` is False for NaN, and a non-finite pixel is bad whatever min / max
    # would make of it (device fmin / fmax drop NaNs; this rule does not depend on that)
    bad = ~(Z > 0.0) | ~np.isfinite(u) | ~np.isfinite(v)
    status, box, clamped = 0, None, False
    r0, c0, S = int(rc_in[0]), int(rc_in[1]), int(side_in)
    if bad.any():
        status = 1
    else:
        umin, umax, vmin, vmax = u.min(), u.max(), v.min(), v.max()
        box = (umin, umax, vmin, vmax)
        if umax < 0.0 or umin > np.float64(W - 1) or vmax < 0.0 or vmin > np.float64(H - 1):
            status = 2
    if status == 0:
        with np.errstate(all="ignore"):
            e = np.maximum(umax - umin, vmax - vmin) * np.float64(pad)
            # every clamp in f64, before the conversion to int: e may be 1e300 or inf
            s_raw = np.ceil(e)
            s = np.minimum(np.maximum(s_raw, np.float64(min_side)), np.float64(min(H, W)))
            c_raw = np.floor(((umin + umax) * 0.5 - s * 0.5) + 1.0)
            r_raw = np.floor(((vmin + vmax) * 0.5 - s * 0.5) + 1.0)
            c = np.minimum(np.maximum(c_raw, 0.0), np.float64(W) - s)
            r = np.minimum(np.maximum(r_raw, 0.0), np.float64(H) - s)
        S, c0, r0 = int(s), int(c), int(r)
        clamped = bool(s != s_raw or c != c_raw or r != r_raw)
    scale, intr = intrinsic(K4, r0, c0, S, T)
    return {"rc": (r0, c0), "side": S, "bbox": np.array([r0, r0 + S, c0, c0 + S], np.float32), "scale": scale,
            "intr": intr, "status": status, "box": box, "clamped": clamped}


def windows(pts, R, t, K4, H, W, T, pad, min_side, rc_in, side_in):
    """A batch: arrays rc int32 [B, 2], side int32 [B], bbox f32 [B, 4], scale f32 [B], intr f32 [B, 4], status int32
    [B], plus the per-crop dicts (`rows`)."""
    rows = [window(pts[b], R[b], t[b], K4[b], H, W, T, pad, min_side, rc_in[b], side_in[b]) for b in range(len(pts))]
    return {"rc": np.array([r["rc"] for r in rows], np.int32), "side": np.array([r["side"] for r in rows], np.int32),
            "bbox": np.stack([r["bbox"] for r in rows]), "scale": np.array([r["scale"] for r in rows], np.float32),
            "intr": np.stack([r["intr"] for r in rows]), "status": np.array([r["status"] for r in rows], np.int32),
            "rows": rows}

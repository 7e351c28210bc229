"""Independent fp64 NumPy restatement of the training augmentation (DESIGN.md section 3 "Training augmentation"): the
camera warp with its fill and photometric step, the radar line, the matrices, the labels, and the reference points the
decoder samples at.  Nothing here imports the package.

Canvas coordinates are EDGE convention in the view's original pixels, u in [0, W], v in [0, H], (H, W) = X_shape; the
sampler reads pixel loc * W_l - 0.5.  A camera maps u' = a u + b_u, v' = s v + b_v.
"""
import numpy as np


def ulp32(x) -> float:
    """Spacing of fp32 at |x| (the format the device computes in)."""
    return float(np.spacing(np.float32(abs(x))))


def camera_map(W, H, flip=False, zoom=1.0, shift=(0.0, 0.0)):
    """-> (a, b_u, s, b_v) in canvas pixels; ``shift`` = (t_x / W, t_y / H)."""
    s = float(zoom)
    a, bu, bv = s, (1.0 - s) * W / 2.0 + shift[0] * W, (1.0 - s) * H / 2.0 + shift[1] * H
    if flip:
        a, bu = -a, W - bu
    return a, bu, s, bv


def radar_map(W, flip=False):
    return (-1.0, float(W), 1.0, 0.0) if flip else (1.0, 0.0, 1.0, 0.0)


def photometric(brightness=1.0, contrast=1.0, channel=(1.0, 1.0, 1.0, 1.0)):
    """-> (gains per channel, offset): clip(g_c v + o, 0, 255)."""
    return [brightness * contrast * c for c in channel], 127.5 * (1.0 - contrast)


def warp_camera(src, Hd, Wd, W, H, m, gains=None, offset=0.0):
    """src (Hs,Ws,C) -> dict(out (Hd,Wd,C) fp64, fill (Hd,Wd) bool, D (Hd,Wd,C) = the largest absolute difference among an
    element's four taps, us / vs (Hd,Wd) the source centres).  ``m`` = (a, b_u, s, b_v) on the (H, W) canvas."""
    src = np.asarray(src, dtype=np.float64)
    Hs, Ws, C = src.shape
    a, bu, s, bv = m
    x, y = np.meshgrid(np.arange(Wd, dtype=np.float64), np.arange(Hd, dtype=np.float64))
    uc, vc = (x + 0.5) * W / Wd, (y + 0.5) * H / Hd                # output pixel centre on the canvas
    us, vs = (uc - bu) / a * Ws / W, (vc - bv) / s * Hs / H      # inverse map -> source coordinate
    fill = ~((us >= 0) & (us <= Ws) & (vs >= 0) & (vs <= Hs))
    fx, fy = np.maximum(us - 0.5, 0.0), np.maximum(vs - 0.5, 0.0)
    x0 = np.minimum(np.floor(fx).astype(np.int64), Ws - 1)
    y0 = np.minimum(np.floor(fy).astype(np.int64), Hs - 1)
    x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
    x0c, y0c = np.clip(x0, 0, Ws - 1), np.clip(y0, 0, Hs - 1)
    lx, ly = (fx - x0)[..., None], (fy - y0)[..., None]
    taps = np.stack([src[y0c, x0c], src[y0c, x1], src[y1, x0c], src[y1, x1]])
    v = (1 - ly) * ((1 - lx) * taps[0] + lx * taps[1]) + ly * ((1 - lx) * taps[2] + lx * taps[3])
    if gains is not None:
        g = np.asarray(gains, dtype=np.float64)[:C]
        if not (np.all(g == 1.0) and offset == 0.0):
            v = np.clip(g * v + offset, 0.0, 255.0)
    v = np.where(fill[..., None], 0.0, v)
    return {"out": v, "fill": fill, "D": taps.max(0) - taps.min(0), "us": us, "vs": vs,
            "gmax": 1.0 if gains is None else float(np.max(np.abs(np.asarray(gains, dtype=np.float64)[:C])))}


def near_frame_edge(r, Hs, Ws, eps):
    """Pixels whose reference source centre lies within ``eps`` of the frame edge (the fill decision may go either way)."""
    return ((np.abs(r["us"]) <= eps) | (np.abs(r["us"] - Ws) <= eps) | (np.abs(r["vs"]) <= eps) | (np.abs(r["vs"] - Hs) <= eps))


def radar_line(x, delta=0.0, flip=False, lo=100.0, hi=200.0, scale=True):
    """x (H,W,C) in dB -> clip(((x + delta) - lo) / (hi - lo) * 255, 0, 255) read from the mirrored azimuth index (axis 1)."""
    x = np.asarray(x, dtype=np.float64)
    if flip:
        x = x[:, ::-1]
    if not scale:
        return x.copy()
    return np.clip(((x + delta) - lo) / (hi - lo) * 255.0, 0.0, 255.0)


F = np.diag([1.0, -1.0, 1.0, 1.0])


def matrices(T, P, m, flip):
    """T (4,4), P (3|4,4) -> (T', P'): P' = M P diag(1,-1,1,1), T' = F T F on a flipped sample; M alone otherwise."""
    T, P = np.asarray(T, dtype=np.float64), np.asarray(P, dtype=np.float64)
    a, bu, s, bv = m
    M = np.eye(P.shape[0])
    M[0, 0], M[0, 2], M[1, 1], M[1, 2] = a, bu, s, bv
    P2 = M @ P
    if flip:
        return F @ T @ F, P2 @ F
    return T.copy(), P2


def labels(center, angle, flip):
    center, angle = np.array(center, dtype=np.float64), np.array(angle, dtype=np.float64)
    if flip:
        center[:, 1] = -center[:, 1]
        angle[:, 0] = -angle[:, 0]
    return center, angle


def reference_points(center, T, P, shape):
    """The UN-CLIPPED reference points of MPFusion.get_reference_points for one sample in fp64: center (N,3), T (4,4) (all
    zero: no transformation), P (3|4,4), shape (H, W) -> (N,2) = (u / W, v / H); a zero divisor leaves the row undivided."""
    pts = np.asarray(center, dtype=np.float64)[:, :3]
    T, P = np.asarray(T, dtype=np.float64), np.asarray(P, dtype=np.float64)
    if T.any():
        p = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ T.T
        r = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2 + p[:, 2] ** 2)
        phi = np.degrees(np.arctan2(p[:, 1], p[:, 0]))
        roh = np.degrees(np.arcsin(np.where(r != 0, p[:, 2] / np.where(r != 0, r, 1.0), 0.0)))
        pts = np.stack([r, phi, roh], 1)
    p = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ P.T
    w = p[:, 2]
    safe = np.where(w != 0, w, 1.0)
    return np.stack([p[:, 0] / safe / shape[1], p[:, 1] / safe / shape[0]], 1)

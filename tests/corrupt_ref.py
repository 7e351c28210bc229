"""Numpy restatement of the sensor degradation launches (dpft_amd/csrc/corrupt.hip; include/dpft_hip.h states the contract):
the blur weights, the blur in fp64, the noise hash in uint32 / uint64 arithmetic, the point-wise chain in float32 operation
for operation (or in fp64, as the reference of the blurred outputs), and the masks.  Positions are PIXELS here."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
INV_STD = np.float32(1.0) / np.float32(37837.2)


def radius(sigma: float) -> int:
    return int(math.ceil(3.0 * float(sigma)))


def weights(sigma: float) -> np.ndarray:
    """Half table w[0..R] of the normalised Gaussian: fp64, rounded once to fp32."""
    R = radius(sigma)
    w = np.array([math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(R + 1)], dtype=np.float64)
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


def blur64(img: np.ndarray, w32: np.ndarray) -> np.ndarray:
    """(H,W,C) -> fp64: horizontal pass, then vertical pass, replicate border, the fp32 weights taken as they are."""
    x = np.asarray(img, dtype=np.float64)
    w = np.asarray(w32, dtype=np.float64)
    R = len(w) - 1
    for axis in (1, 0):
        n = x.shape[axis]
        acc = np.zeros_like(x)
        for k in range(-R, R + 1):
            idx = np.clip(np.arange(n) + k, 0, n - 1)
            acc += w[abs(k)] * np.take(x, idx, axis=axis)
        x = acc
    return x


def mix32(x) -> np.ndarray:
    """The 32-bit multiply-xorshift mixer, on uint64 lanes masked to 32 bits."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def noise_stream(key: int, view: int):
    lo, hi, v = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF), np.uint64(view & 0xFFFFFFFF)
    s0 = mix32(lo ^ mix32(hi ^ mix32(v ^ np.uint64(0x9E3779B9))))
    s1 = mix32(hi ^ mix32(lo ^ mix32(v ^ np.uint64(0xC2B2AE35))))
    return s0, s1


def uniforms16(key: int, view: int, n: int) -> np.ndarray:
    """(n,4) int64: the four 16-bit uniforms of elements 0 .. n-1."""
    s0, s1 = noise_stream(key, view)
    a = mix32(np.arange(n, dtype=np.uint64) ^ s0)
    b = mix32(a ^ s1)
    m = np.uint64(0xFFFF)
    return np.stack([a & m, a >> np.uint64(16), b & m, b >> np.uint64(16)], -1).astype(np.int64)


def noise_z(key: int, view: int, n: int) -> np.ndarray:
    """float32 z of elements 0 .. n-1: Irwin-Hall of order 4, unit variance."""
    return (uniforms16(key, view, n).sum(-1) - 131070).astype(np.float32) * INV_STD


def _clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(v.dtype)


def camera(img: np.ndarray, sigma: float = 0.0, haze: float = 0.0, airlight=(200.0,) * 4, noise: float = 0.0,
           rects=(), off: bool = False, key: int = 0, view: int = 0, dtype=np.float32) -> np.ndarray:
    """One sample (H,W,C).  ``dtype`` float32: blur off only -- the launch's bits.  float64: the reference of a blurred
    sample (fp64 blur, then the chain in fp64 on the float32 parameters).  ``rects``: (x0, x1, y0, y1, fill(4)) in pixels."""
    H, W, C = img.shape
    f = dtype
    if off:
        return np.zeros((H, W, C), dtype=f)
    if sigma > 0:
        assert f is np.float64, "the blurred output has no bit-exact restatement: compare against fp64 within the bound"
        v = blur64(img, weights(sigma))
    else:
        v = np.asarray(img, dtype=np.float32).astype(f)
    if haze != 0:
        A = np.asarray(airlight, dtype=np.float32)[:C].astype(f)
        d = A[None, None, :] - v
        t = f(np.float32(haze)) * d
        v = v + t
    if noise > 0:
        z = noise_z(key, view, H * W * C).reshape(H, W, C).astype(f)
        t = f(np.float32(noise)) * z
        v = _clamp(v + t, f(0), f(255))
    for x0, x1, y0, y1, fill in rects:
        v[y0:y1, x0:x1, :] = np.asarray(fill, dtype=np.float32)[:C].astype(f)
    return v.astype(f)


def radar(x: np.ndarray, noise: float = 0.0, channels=None, azimuth=(), rows=(), off: bool = False, key: int = 0,
          view: int = 0, lo: float = 0.0, hi: float = 255.0) -> np.ndarray:
    """One sample (H,W,C) float32, axis 1 of it = azimuth.  ``azimuth`` / ``rows``: [a0, a1) bands in bins."""
    H, W, C = x.shape
    if off:
        return np.zeros((H, W, C), dtype=np.float32)
    v = np.array(x, dtype=np.float32)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if noise > 0:
        z = noise_z(key, view, H * W * C).reshape(H, W, C)
        t = np.float32(noise) * z
        sel = list(range(C)) if channels is None else sorted(set(channels))
        v[..., sel] = _clamp(v + t, lo32, hi32)[..., sel]
    for a0, a1 in azimuth:
        v[:, a0:a1, :] = lo32
    for r0, r1 in rows:
        v[r0:r1, :, :] = lo32
    return v

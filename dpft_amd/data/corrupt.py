"""Sensor degradation on the device (optional; DESIGN.md section 3 "Sensor degradation").

What fog, defocus, sensor noise, a dirty lens or a jammed radar sector do to the PREPROCESSED inputs: a Gaussian blur, haze,
noise, erased rectangles and "off" on the camera frame; noise, masked azimuth sectors, masked range rows and "off" on the radar
maps.  Two users: the training key ``train.corrupt`` (``CorruptSampler`` draws one ``CameraCorruption`` / ``RadarCorruption``
per sample on the HOST, ``GpuPreprocessor`` runs the launches after its plain or augmented transforms) and the evaluator's
``evaluate.robustness`` conditions (dpft_amd/evaluation/robustness.py: fixed severities).  Labels and matrices are never
touched: nothing moves.

Positions are FRACTIONS of the axis here (an erase rectangle (x0, x1, y0, y1) in [0, 1], a band (f0, f1)); ``pack_*`` turns
them into pixels of the tensor at hand, pixel = floor(f * size + 1/2).  A band may also be ``{"u": u, "bins": n}``: n bins wide,
starting at floor(u * (size - n + 1)) -- how the sampler states a width in bins of the radar raster.  RA and EA share their
azimuth raster, so one sample's azimuth bands are the same columns in ``radar_bev`` and ``radar_front``.

The noise has no device state: it is a pure function of (``key`` of the sample, view id, element index), include/dpft_hip.h.
"""
from __future__ import annotations

import hashlib
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_SIGMA, MAX_RADIUS, MAX_RECTS, MAX_BANDS = 5.0, 15, 4, 4
DEFAULT_AIRLIGHT = 200.0

# uniforms per sample: apply, off lottery, blur, haze, camera noise, rectangle count, 4 x (area, aspect, x, y, 4 fills),
# radar noise, azimuth band count, 4 x (start, width), range band count, 4 x (start, width)
N_DRAWS = 6 + 4 * 8 + 2 + 8 + 1 + 8


def _number(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)


def blur_radius(sigma: float) -> int:
    """R = ceil(3 sigma), in double precision."""
    return int(math.ceil(3.0 * float(sigma)))


def blur_weights(sigma: float) -> np.ndarray:
    """The half table w[0..R] of exp(-k^2 / 2 sigma^2), normalised over the 2R + 1 taps in fp64 and rounded once to fp32."""
    k = np.arange(blur_radius(sigma) + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ parsing
def _range(where: str, v, lo: float, hi: float, integer: bool = False) -> Tuple[float, float]:
    ok = isinstance(v, (list, tuple)) and len(v) == 2 and all(_number(x) for x in v) and lo <= v[0] <= v[1] <= hi
    if ok and integer:
        ok = all(float(x) == int(x) for x in v)
    if not ok:
        raise ValueError(f"{where} must be [lo, hi] with {lo} <= lo <= hi <= {hi}{' (integers)' if integer else ''}, got {v!r}")
    return (int(v[0]), int(v[1])) if integer else (float(v[0]), float(v[1]))


def _probability(where: str, v) -> float:
    if not _number(v) or not 0.0 <= v <= 1.0:
        raise ValueError(f"{where} must be a probability in [0, 1], got {v!r}")
    return float(v)


def _sub(where: str, v, keys) -> Dict:
    if not isinstance(v, dict) or set(v) - set(keys):
        raise ValueError(f"{where}: expected a dict of {sorted(keys)}, got {v!r}")
    return v


def _airlight(where: str, v) -> Tuple[float, ...]:
    vals = [v] * 4 if _number(v) else v
    if not isinstance(vals, (list, tuple)) or not 1 <= len(vals) <= 4 or not all(_number(x) and 0 <= x <= 255 for x in vals):
        raise ValueError(f"{where} must be a number or up to 4 numbers in [0, 255], got {v!r}")
    vals = [float(x) for x in vals]
    return tuple(vals + [vals[-1]] * (4 - len(vals)))


def _mask_spec(where: str, v, top: int) -> Dict:
    v = _sub(where, v, ("n", "width"))
    return {"n": _range(f"{where}.n", v.get("n", [0, 0]), 0, MAX_BANDS, integer=True),
            "width": _range(f"{where}.width", v.get("width", [1, 1]), 1, top, integer=True)}


def parse_corrupt(value) -> Dict:
    """``train.corrupt`` -> the full spec (what is left out is off: zero ranges, zero counts, zero probabilities).  Anything
    malformed is a ValueError."""
    w = "train.corrupt"
    value = _sub(w, value, ("p", "camera", "radar", "seed"))
    cam = _sub(f"{w}: camera", value.get("camera", {}), ("blur", "haze", "noise", "erase", "off", "airlight"))
    rad = _sub(f"{w}: radar", value.get("radar", {}), ("noise", "azimuth_mask", "range_mask", "off", "channels"))
    erase = _sub(f"{w}: camera.erase", cam.get("erase", {}), ("n", "area", "aspect"))
    camera = {"blur": _range(f"{w}: camera.blur", cam.get("blur", [0, 0]), 0.0, MAX_SIGMA),
              "haze": _range(f"{w}: camera.haze", cam.get("haze", [0, 0]), 0.0, 1.0),
              "noise": _range(f"{w}: camera.noise", cam.get("noise", [0, 0]), 0.0, 255.0),
              "erase": {"n": _range(f"{w}: camera.erase.n", erase.get("n", [0, 0]), 0, MAX_RECTS, integer=True),
                        "area": _range(f"{w}: camera.erase.area", erase.get("area", [0, 0]), 0.0, 1.0),
                        "aspect": _range(f"{w}: camera.erase.aspect", erase.get("aspect", [1, 1]), 1e-3, 1e3)},
              "off": _probability(f"{w}: camera.off", cam.get("off", 0.0)),
              "airlight": _airlight(f"{w}: camera.airlight", cam.get("airlight", DEFAULT_AIRLIGHT))}
    channels = rad.get("channels")
    if channels is not None and not (isinstance(channels, (list, tuple)) and channels and all(
            isinstance(c, int) and not isinstance(c, bool) and 0 <= c < 32 for c in channels)):
        raise ValueError(f"{w}: radar.channels must be a list of channel indices in 0..31 or null, got {channels!r}")
    radar = {"noise": _range(f"{w}: radar.noise", rad.get("noise", [0, 0]), 0.0, 255.0),
             "azimuth_mask": _mask_spec(f"{w}: radar.azimuth_mask", rad.get("azimuth_mask", {}), 1 << 16),
             "range_mask": _mask_spec(f"{w}: radar.range_mask", rad.get("range_mask", {}), 1 << 16),
             "off": _probability(f"{w}: radar.off", rad.get("off", 0.0)),
             "channels": None if channels is None else tuple(channels)}
    if camera["off"] + radar["off"] > 1.0:
        raise ValueError(f"{w}: camera.off + radar.off must not exceed 1 (one lottery decides between them), got "
                         f"{camera['off']} + {radar['off']}")
    seed = value.get("seed")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
        raise ValueError(f"{w}: seed must be an integer or null, got {seed!r}")
    return {"p": _probability(f"{w}: p", value.get("p", 1.0)), "camera": camera, "radar": radar, "seed": seed}


# ------------------------------------------------------------------------------------------------- per-sample parameters
class CameraCorruption:
    """One sample's camera degradation.  ``erase``: up to 4 of (x0, x1, y0, y1, fill) with the corners as fractions of the
    frame and ``fill`` a number or up to 4 per-channel values."""
    __slots__ = ("blur", "haze", "airlight", "noise", "erase", "off", "key")

    def __init__(self, blur: float = 0.0, haze: float = 0.0, airlight=DEFAULT_AIRLIGHT, noise: float = 0.0,
                 erase: Sequence = (), off: bool = False, key: int = 0):
        if not (0.0 <= blur <= MAX_SIGMA):
            raise ValueError(f"blur (sigma) must lie in [0, {MAX_SIGMA}], got {blur!r}")
        if not (0.0 <= haze <= 1.0):
            raise ValueError(f"haze must lie in [0, 1], got {haze!r}")
        if not (noise >= 0.0 and math.isfinite(noise)):
            raise ValueError(f"noise must be finite and >= 0, got {noise!r}")
        if len(erase) > MAX_RECTS:
            raise ValueError(f"at most {MAX_RECTS} erase rectangles, got {len(erase)}")
        self.blur, self.haze, self.noise = float(blur), float(haze), float(noise)
        self.airlight = _airlight("airlight", airlight)
        self.erase = []
        for r in erase:
            x0, x1, y0, y1 = (float(v) for v in r[:4])
            if not (0.0 <= x0 <= x1 <= 1.0 and 0.0 <= y0 <= y1 <= 1.0):
                raise ValueError(f"erase rectangle {tuple(r[:4])!r} leaves the frame: fractions with 0 <= lo <= hi <= 1")
            fill = r[4] if len(r) > 4 else 0.0
            fill = [float(fill)] * 4 if _number(fill) else [float(v) for v in fill]
            self.erase.append((x0, x1, y0, y1, tuple(fill + [fill[-1]] * (4 - len(fill)))))
        self.off, self.key = bool(off), int(key) & 0xFFFFFFFFFFFFFFFF

    @property
    def neutral(self) -> bool:
        return not (self.blur > 0 or self.haze > 0 or self.noise > 0 or self.erase or self.off)


class RadarCorruption:
    """One sample's radar degradation.  ``channels``: None (all) or the channel indices the noise acts on; ``azimuth`` /
    ``rows``: up to 4 bands each, (f0, f1) fractions of the axis or {"u": u, "bins": n}."""
    __slots__ = ("noise", "channels", "azimuth", "rows", "off", "key")

    def __init__(self, noise: float = 0.0, channels: Optional[Sequence[int]] = None, azimuth: Sequence = (),
                 rows: Sequence = (), off: bool = False, key: int = 0):
        if not (noise >= 0.0 and math.isfinite(noise)):
            raise ValueError(f"noise must be finite and >= 0, got {noise!r}")
        for name, bands in (("azimuth", azimuth), ("rows", rows)):
            if len(bands) > MAX_BANDS:
                raise ValueError(f"at most {MAX_BANDS} {name} bands, got {len(bands)}")
            for b in bands:
                if isinstance(b, dict):
                    if set(b) != {"u", "bins"} or not 0.0 <= b["u"] < 1.0 or int(b["bins"]) < 0:
                        raise ValueError(f"{name} band {b!r}: expected {{'u': [0, 1), 'bins': n >= 0}}")
                elif not (len(b) == 2 and 0.0 <= b[0] <= b[1] <= 1.0):
                    raise ValueError(f"{name} band {b!r} leaves the axis: fractions with 0 <= f0 <= f1 <= 1")
        self.noise = float(noise)
        self.channels = None if channels is None else tuple(int(c) for c in channels)
        self.azimuth, self.rows = list(azimuth), list(rows)
        self.off, self.key = bool(off), int(key) & 0xFFFFFFFFFFFFFFFF

    @property
    def neutral(self) -> bool:
        return not (self.noise > 0 or self.azimuth or self.rows or self.off)

    def neutral_for(self, rows_are_range: bool) -> bool:
        return not (self.noise > 0 or self.azimuth or (self.rows and rows_are_range) or self.off)


def _pixel(f: float, size: int) -> int:
    return min(size, int(math.floor(float(f) * size + 0.5)))


def band_pixels(band, size: int) -> Tuple[int, int]:
    """A band -> [a0, a1) in bins of an axis of ``size``."""
    if isinstance(band, dict):
        n = min(int(band["bins"]), size)
        a0 = int(math.floor(float(band["u"]) * (size - n + 1)))
        return a0, a0 + n
    return _pixel(band[0], size), _pixel(band[1], size)


def pack_camera(params: Sequence[CameraCorruption], H: int, W: int, view: int = 0):
    """-> the host array of dpft_corrupt_camera for frames of H x W."""
    from dpft_amd.hip.lib import CorruptCamera
    arr = (CorruptCamera * len(params))()
    for a, p in zip(arr, params):
        a.key, a.view, a.sigma, a.radius = p.key, int(view), p.blur, blur_radius(p.blur)
        if p.blur > 0:
            for k, w in enumerate(blur_weights(p.blur)):
                a.w[k] = float(w)
        a.haze, a.noise, a.off, a.n_rects = p.haze, p.noise, int(p.off), len(p.erase)
        for c in range(4):
            a.airlight[c] = p.airlight[c]
        for j, (x0, x1, y0, y1, fill) in enumerate(p.erase):
            for k, v in enumerate((_pixel(x0, W), _pixel(x1, W), _pixel(y0, H), _pixel(y1, H))):
                a.rect[j][k] = v
            for c in range(4):
                a.fill[j][c] = fill[c]
    return arr


def pack_radar(params: Sequence[RadarCorruption], H: int, W: int, view: int = 0, rows_are_range: bool = True):
    """-> the host array of dpft_corrupt_radar for maps of H x W (axis 2 = azimuth).  Row bands are range bands: a map whose
    rows are no range axis (``rows_are_range`` False: the elevation rows of ``radar_front``) takes none."""
    from dpft_amd.hip.lib import CorruptRadar
    arr = (CorruptRadar * len(params))()
    for a, p in zip(arr, params):
        a.key, a.view, a.noise, a.off = p.key, int(view), p.noise, int(p.off)
        a.channels = 0xFFFFFFFF if p.channels is None else sum(1 << c for c in set(p.channels))
        a.n_azimuth = len(p.azimuth)
        for j, b in enumerate(p.azimuth):
            a.azimuth[j][0], a.azimuth[j][1] = band_pixels(b, W)
        rows = p.rows if rows_are_range else []
        a.n_rows = len(rows)
        for j, b in enumerate(rows):
            a.rows[j][0], a.rows[j][1] = band_pixels(b, H)
    return arr


def _device_f32(x: torch.Tensor, what: str) -> torch.Tensor:
    from dpft_amd.hip.lib import HipLibraryError
    if not x.is_cuda:
        raise HipLibraryError(f"{what} needs device tensors; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError(f"{what}: expected a preprocessed (B,H,W,C) float32 tensor, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


def corrupt_camera(x: torch.Tensor, params: Sequence[CameraCorruption], view: int = 0) -> torch.Tensor:
    """(B,H,W,C <= 4) float32 preprocessed frames -> the degraded frames (a new tensor); ``x`` itself when every sample is
    neutral (no launch)."""
    from dpft_amd.hip.lib import lib, ptr, stream
    if len(params) != x.shape[0]:
        raise ValueError(f"corrupt_camera: {len(params)} parameter sets for a batch of {x.shape[0]}")
    if all(p.neutral for p in params):
        return x
    x = _device_f32(x, "corrupt_camera")
    B, H, W, Ch = x.shape
    y = torch.empty_like(x)
    lib.call("dpft_corrupt_camera_nhwc_f32", ptr(x), ptr(y), B, H, W, Ch, pack_camera(params, H, W, view), stream())
    return y


def corrupt_radar(x: torch.Tensor, params: Sequence[RadarCorruption], lo: float = 0.0, hi: float = 255.0,
                  rows_are_range: bool = True, view: int = 0) -> torch.Tensor:
    """(B,H,W,C) float32 preprocessed radar map (axis 2 = azimuth) -> the degraded map (a new tensor); ``x`` itself when every
    sample is neutral for this map (no launch)."""
    from dpft_amd.hip.lib import lib, ptr, stream
    if len(params) != x.shape[0]:
        raise ValueError(f"corrupt_radar: {len(params)} parameter sets for a batch of {x.shape[0]}")
    if all(p.neutral_for(rows_are_range) for p in params):
        return x
    x = _device_f32(x, "corrupt_radar")
    B, H, W, Ch = x.shape
    y = torch.empty_like(x)
    lib.call("dpft_corrupt_radar_nhwc_f32", ptr(x), ptr(y), B, H, W, Ch, float(lo), float(hi),
             pack_radar(params, H, W, view, rows_are_range), stream())
    return y


RANGE_KEYS = ("radar_bev",)      # the maps whose rows (axis 1) are range bins


def corrupt_batch(batch: Dict[str, torch.Tensor], cams: Sequence[CameraCorruption], rads: Sequence[RadarCorruption],
                  camera_keys: Sequence[str], radar_keys: Sequence[str], lo: float = 0.0, hi: float = 255.0
                  ) -> Dict[str, torch.Tensor]:
    """The launches of one batch: every camera view takes ``cams``, every radar view ``rads``; the view id of a key is its
    position in ``camera_keys + radar_keys``.  Everything else in the dict passes through untouched (the same objects)."""
    out = dict(batch)
    for v, k in enumerate(tuple(camera_keys) + tuple(radar_keys)):
        if k not in out:
            continue
        if k in camera_keys:
            out[k] = corrupt_camera(out[k], cams, view=v)
        else:
            out[k] = corrupt_radar(out[k], rads, lo, hi, rows_are_range=k in RANGE_KEYS, view=v)
    return out


# -------------------------------------------------------------------------------------------------------------- sampler
def _hash64(text: str) -> int:
    return int.from_bytes(hashlib.blake2b(text.encode(), digest_size=8).digest(), "little")


class CorruptSampler:
    """Draws the per-sample degradations on the host, one ``draw`` per batch.  Like ``AugmentSampler`` the generator of a batch
    is seeded from (seed, rank, epoch, batch ordinal) -- but it is a generator of its OWN with its own seed string, so a config
    that adds ``train.corrupt`` beside ``train.augment`` leaves every augmentation draw as it was."""

    def __init__(self, spec: Dict, seed: int = 0, rank: int = 0):
        self.spec = spec
        self.seed = int(spec["seed"]) if spec.get("seed") is not None else int(seed)
        self.rank, self.epoch, self.ordinal = int(rank), 0, 0
        self._g = torch.Generator()

    def set_epoch(self, epoch: int) -> None:
        self.epoch, self.ordinal = int(epoch), 0

    def _tag(self, ordinal: int) -> str:
        return f"dpft-corrupt/{self.seed}/{self.rank}/{self.epoch}/{ordinal}"

    def uniforms(self, batch_size: int) -> torch.Tensor:
        """(B, N_DRAWS) fp64 uniforms in [0, 1) of the next batch; advances the batch ordinal."""
        self._g.manual_seed(_hash64(self._tag(self.ordinal)) >> 1)
        self.ordinal += 1
        return torch.rand(batch_size, N_DRAWS, generator=self._g, dtype=torch.float64)

    def draw(self, batch_size: int) -> Tuple[List[CameraCorruption], List[RadarCorruption]]:
        cam, rad = self.spec["camera"], self.spec["radar"]
        tag = self._tag(self.ordinal)
        cams, rads = [], []

        def lerp(r, u):
            return r[0] + (r[1] - r[0]) * u

        def count(r, u):
            return r[0] + min(int(u * (r[1] - r[0] + 1)), r[1] - r[0])

        for b, u in enumerate(self.uniforms(batch_size).tolist()):
            key = _hash64(f"{tag}/{b}")
            if not u[0] < self.spec["p"]:
                cams.append(CameraCorruption(key=key))
                rads.append(RadarCorruption(key=key))
                continue
            # one lottery for both: camera off, radar off or neither -- never both (the dataset's dropout has the same rule)
            cam_off = u[1] < cam["off"]
            rad_off = not cam_off and u[1] < cam["off"] + rad["off"]
            rects = []
            e = cam["erase"]
            for j in range(count(e["n"], u[5])):
                d = u[6 + 8 * j:14 + 8 * j]
                area, aspect = lerp(e["area"], d[0]), lerp(e["aspect"], d[1])
                fw, fh = min(1.0, math.sqrt(area * aspect)), min(1.0, math.sqrt(area / aspect))
                x0, y0 = d[2] * (1.0 - fw), d[3] * (1.0 - fh)
                rects.append((x0, min(1.0, x0 + fw), y0, min(1.0, y0 + fh), [255.0 * v for v in d[4:8]]))
            cams.append(CameraCorruption(blur=lerp(cam["blur"], u[2]), haze=lerp(cam["haze"], u[3]), airlight=cam["airlight"],
                                         noise=lerp(cam["noise"], u[4]), erase=rects, off=cam_off, key=key))
            bands = []
            for name, at in (("azimuth_mask", 39), ("range_mask", 48)):
                m = rad[name]
                bands.append([{"u": u[at + 1 + 2 * j], "bins": count(m["width"], u[at + 2 + 2 * j])}
                              for j in range(count(m["n"], u[at]))])
            rads.append(RadarCorruption(noise=lerp(rad["noise"], u[38]), channels=rad["channels"], azimuth=bands[0],
                                        rows=bands[1], off=rad_off, key=key))
        return cams, rads

"""Training augmentation on the device (optional, ``train.augment``; DESIGN.md section 3 "Training augmentation").

One horizontal flip per sample applied to EVERY view and to the labels together, a camera zoom / shift about the canvas
centre, a photometric step on the camera frame and a gain on the radar maps.  The decoder projects 3-D query centres
through ``label_to_X_t`` / ``label_to_X_p`` into each view and samples there, so images, radar maps, labels and all
matrices move together:

* canvas coordinates are EDGE convention in the view's original pixels, u in [0, W], v in [0, H], (H, W) = ``X_shape``;
  a camera maps u' = a u + b_u, v' = s v + b_v with s the zoom about the centre, (t_x, t_y) = shift (W, H) U(-1, 1),
  a = s, b_u = (1 - s) W / 2 + t_x, b_v = (1 - s) H / 2 + t_y, and on a flipped sample a -> -a, b_u -> W - b_u; radar
  maps take only the flip (a = -1, b_u = W along the azimuth axis);
* matrices P' = M P diag(1,-1,1,1), T' = F T F (F = diag(1,-1,1,1)), M = identity but M[0,0] = a, M[0,2] = b_u,
  M[1,1] = s, M[1,2] = b_v; labels of a flipped sample: centre y and angle sin negated.

The per-sample parameters are a few floats drawn on the HOST (``AugmentSampler``, a CPU ``torch.Generator``: no device
random state, no read-back) and travel by value in the kernel arguments; here they are kept in units of the canvas
(b_u / W, b_v / H), the geometry launch reads (H, W) from the ``X_shape`` rows on the device.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

_CAMERA = {"zoom": (1.0, 1.0), "shift": 0.0, "brightness": 0.0, "contrast": 0.0, "channel": 0.0}
_RADAR = {"gain_db": 0.0}
N_DRAWS = 11      # uniforms per sample: flip, zoom, shift x, shift y, brightness, contrast, 4 channels, radar gain


def _number(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)


def parse_augment(value) -> Dict:
    """``train.augment`` -> {"flip": p, "camera": {"zoom": (lo, hi), "shift", "brightness", "contrast", "channel"},
    "radar": {"gain_db"}, "seed": int | None}: ``true`` (``{"flip": 0.5}``) or a dict of those keys (what is left out is
    off).  Anything else is a ValueError."""
    if value is True:
        value = {"flip": 0.5}
    if not isinstance(value, dict) or set(value) - {"flip", "camera", "radar", "seed"}:
        raise ValueError("train.augment: expected true or {'flip': p, 'camera': {...}, 'radar': {...}, 'seed': ...}, "
                         f"got {value!r}")
    flip = value.get("flip", 0.0)
    if not _number(flip) or not 0.0 <= flip <= 1.0:
        raise ValueError(f"train.augment: flip must be a probability in [0, 1], got {flip!r}")
    camera = dict(_CAMERA)
    cam = value.get("camera", {})
    if not isinstance(cam, dict) or set(cam) - set(_CAMERA):
        raise ValueError(f"train.augment: camera: expected a dict of {sorted(_CAMERA)}, got {cam!r}")
    if "zoom" in cam:
        z = cam["zoom"]
        if not isinstance(z, (list, tuple)) or len(z) != 2 or not all(_number(x) for x in z) or z[0] <= 0 or z[0] > z[1]:
            raise ValueError(f"train.augment: camera.zoom must be [lo, hi] with 0 < lo <= hi, got {z!r}")
        camera["zoom"] = (float(z[0]), float(z[1]))
    for k, top in (("shift", 0.5), ("brightness", 1.0), ("contrast", 1.0), ("channel", 1.0)):
        if k in cam:
            if not _number(cam[k]) or not 0.0 <= cam[k] <= top:
                raise ValueError(f"train.augment: camera.{k} must be a number in [0, {top}], got {cam[k]!r}")
            camera[k] = float(cam[k])
    radar = dict(_RADAR)
    rad = value.get("radar", {})
    if not isinstance(rad, dict) or set(rad) - set(_RADAR):
        raise ValueError(f"train.augment: radar: expected a dict of {sorted(_RADAR)}, got {rad!r}")
    if "gain_db" in rad:
        if not _number(rad["gain_db"]) or rad["gain_db"] < 0:
            raise ValueError(f"train.augment: radar.gain_db must be a number >= 0, got {rad['gain_db']!r}")
        radar["gain_db"] = float(rad["gain_db"])
    seed = value.get("seed")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
        raise ValueError(f"train.augment: seed must be an integer or null, got {seed!r}")
    return {"flip": float(flip), "camera": camera, "radar": radar, "seed": seed}


def check_fov_symmetric(spec: Dict, fov: Optional[Dict[str, Sequence[float]]]) -> None:
    """A flip mirrors y and the azimuth: with a ``data.fov`` range of either that is not symmetric about 0 a flipped label
    could leave the field of view the labels were filtered by."""
    if spec["flip"] <= 0 or not fov:
        return
    for name in ("y", "azimuth"):
        if name in fov:
            lo, hi = fov[name]
            if float(lo) != -float(hi):
                raise ValueError(f"train.augment: flip > 0 needs data.fov.{name} symmetric about 0, got [{lo}, {hi}]")


class SampleParams:
    """One sample's parameters.  ``a``, ``s`` and ``bu``, ``bv`` (in units of the canvas, after the flip) define the camera map;
    ``gain`` (4 channels) and ``offset`` the photometric step, ``delta_db`` the radar gain."""
    __slots__ = ("flip", "s", "a", "bu", "bv", "gain", "offset", "delta_db")

    def __init__(self, flip: bool = False, zoom: float = 1.0, shift: Tuple[float, float] = (0.0, 0.0),
                 brightness: float = 1.0, contrast: float = 1.0, channel: Sequence[float] = (1.0, 1.0, 1.0, 1.0),
                 delta_db: float = 0.0):
        s = float(zoom)
        if not (s > 0 and math.isfinite(s)):
            raise ValueError(f"zoom must be positive and finite, got {zoom!r}")
        bu = (1.0 - s) / 2.0 + float(shift[0])
        self.flip, self.s = bool(flip), s
        self.a = -s if flip else s
        self.bu = 1.0 - bu if flip else bu
        self.bv = (1.0 - s) / 2.0 + float(shift[1])
        channel = (list(channel) + [1.0] * 4)[:4]
        self.gain = [float(brightness) * float(contrast) * float(c) for c in channel]
        self.offset = 127.5 * (1.0 - float(contrast))
        self.delta_db = float(delta_db)


def pack_samples(params):
    """-> the host array of dpft_augment_sample the C entries take (an array that is packed already is passed on)."""
    from dpft_amd.hip.lib import AugmentSample
    if isinstance(params, C.Array):
        return params
    arr = (AugmentSample * len(params))()
    for i, p in enumerate(params):
        arr[i].a, arr[i].bu, arr[i].s, arr[i].bv = p.a, p.bu, p.s, p.bv
        for c in range(4):
            arr[i].gain[c] = p.gain[c]
        arr[i].offset, arr[i].delta_db, arr[i].flip = p.offset, p.delta_db, int(p.flip)
    return arr


class AugmentSampler:
    """Draws the per-sample parameters on the host.  One call of ``draw`` per batch; the generator of a batch is seeded from
    (seed, rank, epoch, batch ordinal), so a draw is reproducible from those four numbers alone."""

    def __init__(self, spec: Dict, seed: int = 0, rank: int = 0):
        self.spec = spec
        self.seed = int(spec["seed"]) if spec.get("seed") is not None else int(seed)
        self.rank, self.epoch, self.ordinal = int(rank), 0, 0
        self._g = torch.Generator()

    def set_epoch(self, epoch: int) -> None:
        self.epoch, self.ordinal = int(epoch), 0

    def _seed_of(self, ordinal: int) -> int:
        key = f"dpft-augment/{self.seed}/{self.rank}/{self.epoch}/{ordinal}".encode()
        return int.from_bytes(hashlib.blake2b(key, digest_size=8).digest(), "little") >> 1

    def uniforms(self, batch_size: int) -> torch.Tensor:
        """(B, N_DRAWS) fp64 uniforms in [0, 1) of the next batch; advances the batch ordinal."""
        self._g.manual_seed(self._seed_of(self.ordinal))
        self.ordinal += 1
        return torch.rand(batch_size, N_DRAWS, generator=self._g, dtype=torch.float64)

    def draw(self, batch_size: int) -> List[SampleParams]:
        cam, rad = self.spec["camera"], self.spec["radar"]
        z0, z1 = cam["zoom"]
        out = []
        for u in self.uniforms(batch_size).tolist():
            sym = [2.0 * x - 1.0 for x in u]                # U(-1, 1)
            out.append(SampleParams(
                flip=u[0] < self.spec["flip"], zoom=z0 + (z1 - z0) * u[1],
                shift=(cam["shift"] * sym[2], cam["shift"] * sym[3]),
                brightness=1.0 + cam["brightness"] * sym[4], contrast=1.0 + cam["contrast"] * sym[5],
                channel=[1.0 + cam["channel"] * x for x in sym[6:10]], delta_db=rad["gain_db"] * sym[10]))
        return out


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def augment_camera(frames: torch.Tensor, size: Optional[Tuple[int, int]], params: Sequence[SampleParams]) -> torch.Tensor:
    """(B,H,W,C <= 4) float32 or uint8 -> (B,size[0],size[1],C) float32: resize + warp + flip + photometric step, one launch
    (``size`` None: the frame's own size)."""
    from dpft_amd.data.preprocess import _check
    from dpft_amd.hip.lib import lib, ptr, stream
    _check(frames)
    frames = frames.contiguous()
    B, Hs, Ws, Ch = frames.shape
    if len(params) != B:
        raise ValueError(f"augment_camera: {len(params)} parameter sets for a batch of {B}")
    Hd, Wd = (Hs, Ws) if size is None else size
    out = torch.empty((B, Hd, Wd, Ch), dtype=torch.float32, device=frames.device)
    if frames.dtype == torch.uint8:
        fn = "dpft_augment_camera_nhwc_u8"
    elif frames.dtype == torch.float32:
        fn = "dpft_augment_camera_nhwc_f32"
    else:
        raise TypeError(f"augment_camera: unsupported dtype {frames.dtype}")
    lib.call(fn, ptr(frames), ptr(out), B, Hs, Ws, Hd, Wd, Ch, pack_samples(params), stream())
    return out


def augment_radar(x: torch.Tensor, params: Sequence[SampleParams], scale: bool = True, in_lo: float = None,
                  in_hi: float = None) -> torch.Tensor:
    """(B,H,W,C) radar map in dB -> the scaled map of ``scale_clip`` with the sample's gain added first, read from the
    mirrored azimuth index (axis 2) on a flipped sample; ``scale`` False: the flip alone."""
    from dpft_amd.data.preprocess import MAX_POWER, MIN_POWER, _check
    from dpft_amd.hip.lib import lib, ptr, stream
    _check(x)
    x = _f32(x)
    B, H, W, Ch = x.shape
    if len(params) != B:
        raise ValueError(f"augment_radar: {len(params)} parameter sets for a batch of {B}")
    y = torch.empty_like(x)
    lib.call("dpft_augment_radar_nhwc_f32", ptr(x), ptr(y), B, H, W, Ch, int(bool(scale)),
             float(MIN_POWER if in_lo is None else in_lo), float(MAX_POWER if in_hi is None else in_hi), 0.0, 255.0,
             pack_samples(params), stream())
    return y


def augment_geometry(views: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, bool]],
                     labels: Optional[Sequence[Dict[str, torch.Tensor]]], params: Sequence[SampleParams]):
    """One launch (per chunk of samples) for all matrices and labels, out of place.

    ``views``: (T (B,4,4), P (B,3|4,4), shape (B,>=2) int64 rows (H, W, ...), is_camera) per view.
    -> ([(T', P')] per view, new label dicts or None).  Label entries other than ``gt_center`` / ``gt_angle`` are passed on."""
    from dpft_amd.hip.lib import AUGMENT_MAX_VIEWS, AugmentLabels, AugmentView, lib, stream
    B = len(params)
    if len(views) > AUGMENT_MAX_VIEWS:
        raise ValueError(f"augment_geometry: at most {AUGMENT_MAX_VIEWS} views, got {len(views)}")
    table = (AugmentView * max(1, len(views)))()
    keep, out_views = [], []
    dev = None
    for i, (T, P, shape, is_camera) in enumerate(views):
        T, P = _f32(T), _f32(P)
        if shape.dtype != torch.int64 or shape.dim() != 2 or shape.shape[1] < 2 or shape.stride(1) != 1:
            shape = shape[:, :2].to(torch.int64).contiguous()
        if not (T.is_cuda and P.is_cuda and shape.is_cuda):
            from dpft_amd.hip.lib import HipLibraryError
            raise HipLibraryError("augment_geometry needs device tensors; there is no CPU path")
        if T.shape != (B, 4, 4) or P.shape[0] != B or P.shape[1] not in (3, 4) or P.shape[2] != 4 or shape.shape[0] != B:
            raise ValueError(f"augment_geometry: view {i}: T {tuple(T.shape)}, P {tuple(P.shape)}, shape "
                             f"{tuple(shape.shape)} do not fit a batch of {B}")
        dev = T.device
        T2, P2 = torch.empty_like(T), torch.empty_like(P)
        keep += [T, P, shape]
        out_views.append((T2, P2))
        v = table[i]
        v.T, v.P, v.T_out, v.P_out, v.shape = T.data_ptr(), P.data_ptr(), T2.data_ptr(), P2.data_ptr(), shape.data_ptr()
        v.shape_stride, v.p_rows, v.zoom = shape.stride(0), P.shape[1], int(bool(is_camera))
    ltab, out_labels = None, None
    if labels is not None:
        if len(labels) != B:
            raise ValueError(f"augment_geometry: {len(labels)} label dicts for a batch of {B}")
        ltab = (AugmentLabels * B)()
        rows = [int(l["gt_center"].shape[0]) for l in labels]
        for l, m in zip(labels, rows):
            if tuple(l["gt_center"].shape) != (m, 3) or tuple(l["gt_angle"].shape) != (m, 2):
                raise ValueError("augment_geometry: labels need gt_center (M,3) and gt_angle (M,2)")
        dev = labels[0]["gt_center"].device if dev is None else dev
        flat = torch.empty(max(1, 5 * sum(rows)), dtype=torch.float32, device=dev)      # one buffer: every centre, then every angle
        off, out_labels = 0, []
        for b, (l, m) in enumerate(zip(labels, rows)):
            c, a = _f32(l["gt_center"]), _f32(l["gt_angle"])
            c2, a2 = flat[off:off + 3 * m].view(m, 3), flat[off + 3 * m:off + 5 * m].view(m, 2)
            off += 5 * m
            keep += [c, a]
            if m:
                if not (c.is_cuda and a.is_cuda):
                    from dpft_amd.hip.lib import HipLibraryError
                    raise HipLibraryError("augment_geometry needs device tensors; there is no CPU path")
                ltab[b].center, ltab[b].angle = c.data_ptr(), a.data_ptr()
                ltab[b].center_out, ltab[b].angle_out = c2.data_ptr(), a2.data_ptr()
            ltab[b].rows = m
            out_labels.append(dict(l, gt_center=c2.to(l["gt_center"].dtype), gt_angle=a2.to(l["gt_angle"].dtype)))
    lib.call("dpft_augment_geometry_f32", table, len(views), ltab, pack_samples(params), B, stream())
    return out_views, out_labels

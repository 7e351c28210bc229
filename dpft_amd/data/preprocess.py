"""Online sample transforms of ``KRadarDataset.__getitem__`` on the device.

Reference order (src/dprt/datasets/kradar/dataset.py:140-169): load -> ``scale_radar_data`` (:295-317) -> labels ->
transformations / projections / ``_add_shape`` (shape recorded BEFORE the resize) -> ``resize_image`` (:319-341).
Here the loader ships raw frames (camera as decoded u8 or float HWC, radar maps in dB) and this module runs the two
arithmetic transforms as HIP kernels on the upload stream; everything else in the sample dict passes through.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple, Union

import torch

from dpft_amd.hip.lib import HipLibraryError, lib, ptr, stream

MIN_POWER, MAX_POWER = 100.0, 200.0        # src/dprt/datasets/kradar/utils/radar_info.py:109,113


def resized_output_size(h: int, w: int, size: Union[int, Sequence[int]]) -> Tuple[int, int]:
    """torchvision.transforms.functional.resize size rule: an int matches the SHORT side, the long side is
    int(size * long / short); a pair is taken as (H, W)."""
    if isinstance(size, (tuple, list)):
        if len(size) == 2:
            return int(size[0]), int(size[1])
        size = size[0]
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = int(size), int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def _check(t: torch.Tensor):
    if not t.is_cuda:
        raise HipLibraryError("dpft_amd.data.GpuPreprocessor needs device tensors; there is no CPU path")


def resize_bilinear(frames: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """(B,H,W,C) float32 or uint8 -> (B,size[0],size[1],C) float32, bilinear, align_corners=False, no antialias."""
    _check(frames)
    frames = frames.contiguous()
    B, Hs, Ws, C = frames.shape
    out = torch.empty((B, size[0], size[1], C), dtype=torch.float32, device=frames.device)
    if frames.dtype == torch.uint8:
        fn = "dpft_resize_bilinear_nhwc_u8"
    elif frames.dtype == torch.float32:
        fn = "dpft_resize_bilinear_nhwc_f32"
    else:
        raise TypeError(f"resize_bilinear: unsupported dtype {frames.dtype}")
    lib.call(fn, ptr(frames), ptr(out), B, Hs, Ws, size[0], size[1], C, stream())
    return out


def scale_clip(x: torch.Tensor, in_lo: float = MIN_POWER, in_hi: float = MAX_POWER, out_lo: float = 0.0,
               out_hi: float = 255.0) -> torch.Tensor:
    _check(x)
    x = x.contiguous().float()
    y = torch.empty_like(x)
    lib.call("dpft_scale_clip_f32", ptr(x), ptr(y), x.numel(), float(in_lo), float(in_hi), float(out_lo), float(out_hi),
             stream())
    return y


class GpuPreprocessor:
    """``augment``: None / False (off: the plain transforms, exactly), or a ``train.augment`` value / an
    ``AugmentSampler`` -- the training augmentation of dpft_amd/data/augment.py.  An augmenting preprocessor is called with
    the labels, ``pre(batch, labels) -> (batch, labels)``: the flip moves frames, radar maps, matrices and labels together.
    ``corrupt``: None / False (off), or a ``train.corrupt`` value / a ``CorruptSampler`` -- the sensor degradation of
    dpft_amd/data/corrupt.py, run AFTER the plain or the augmented transforms on their outputs; labels and matrices pass
    through untouched, so the call keeps the form the ``augment`` setting gives it."""

    def __init__(self, image_size: Union[int, Sequence[int], None] = 512, scale: bool = True,
                 camera_keys: Sequence[str] = ("camera_mono", "camera_stereo"),
                 radar_keys: Sequence[str] = ("radar_bev", "radar_front"), augment=None, seed: int = 0, rank: int = 0,
                 corrupt=None):
        self.image_size, self.scale = image_size, scale
        self.camera_keys, self.radar_keys = tuple(camera_keys), tuple(radar_keys)
        self.sampler = None
        if augment is not None and augment is not False:
            from dpft_amd.data.augment import AugmentSampler, parse_augment
            self.sampler = augment if isinstance(augment, AugmentSampler) else AugmentSampler(parse_augment(augment), seed, rank)
        self.corruptor = None
        if corrupt is not None and corrupt is not False:
            from dpft_amd.data.corrupt import CorruptSampler, parse_corrupt
            self.corruptor = corrupt if isinstance(corrupt, CorruptSampler) else CorruptSampler(parse_corrupt(corrupt), seed, rank)

    @property
    def augments(self) -> bool:
        return self.sampler is not None

    @property
    def corrupts(self) -> bool:
        return self.corruptor is not None

    def set_epoch(self, epoch: int) -> None:
        if self.sampler is not None:
            self.sampler.set_epoch(epoch)
        if self.corruptor is not None:
            self.corruptor.set_epoch(epoch)

    @classmethod
    def from_config(cls, config: Dict, augment: bool = False, rank: int = 0) -> "GpuPreprocessor":
        """``augment=True`` (the TRAINING loader only): take ``train.augment`` and ``train.corrupt`` of the config, where it has
        the keys.  Validation and evaluation preprocessors (``augment`` left False) take neither."""
        d = config.get("data", {})
        spec, seed, corrupt = None, 0, None
        if augment and "corrupt" in config.get("train", {}):
            from dpft_amd.data.corrupt import parse_corrupt
            corrupt = parse_corrupt(config["train"]["corrupt"])
            seed = config.get("computing", {}).get("seed", 0)
        if augment and "augment" in config.get("train", {}):
            from dpft_amd.data.augment import check_fov_symmetric, parse_augment
            spec = parse_augment(config["train"]["augment"])
            check_fov_symmetric(spec, d.get("fov"))
            seed = config.get("computing", {}).get("seed", 0)
        return cls(image_size=d.get("image_size", 512), scale=d.get("scale", True), augment=spec, seed=seed, rank=rank,
                   corrupt=corrupt)

    def _corrupted(self, out: Dict[str, torch.Tensor], params=None) -> Dict[str, torch.Tensor]:
        """The degradation launches on the transforms' outputs.  ``params`` (a pair of lists, ``CameraCorruption`` and
        ``RadarCorruption`` per sample) overrides the sampler's draw."""
        from dpft_amd.data import corrupt as K
        views = [k for k in self.camera_keys + self.radar_keys if k in out]
        if not views:
            return out
        cams, rads = self.corruptor.draw(out[views[0]].shape[0]) if params is None else params
        return K.corrupt_batch(out, cams, rads, self.camera_keys, self.radar_keys)

    def __call__(self, batch: Dict[str, torch.Tensor], labels=None):
        if self.corruptor is not None:
            if self.sampler is not None:
                out, labels = self._augmented(batch, labels)
                return self._corrupted(out), labels
            return self._corrupted(self._plain(batch))
        if self.sampler is not None:
            return self._augmented(batch, labels)
        return self._plain(batch)

    def _plain(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        out = dict(batch)
        for k in self.radar_keys:
            if k in out and self.scale:
                out[k] = scale_clip(out[k])
        for k in self.camera_keys:
            if k in out:
                v = out[k]
                if self.image_size is not None:
                    v = resize_bilinear(v, resized_output_size(v.shape[1], v.shape[2], self.image_size))
                elif v.dtype != torch.float32:
                    v = v.float()
                out[k] = v
        return out

    def _augmented(self, batch: Dict[str, torch.Tensor], labels, params=None):
        """The augmented transforms: one launch per view in place of its resize / scaling launch, and the geometry launch.
        ``params`` (a list of ``SampleParams``) overrides the sampler's draw."""
        from dpft_amd.data import augment as A
        if labels is None:
            raise ValueError("GpuPreprocessor: an augmenting preprocessor needs the labels, pre(batch, labels): a flipped "
                             "frame with unflipped labels is silent corruption")
        views = [k for k in self.camera_keys + self.radar_keys if k in batch]
        if not views:
            return dict(batch), list(labels)
        B = batch[views[0]].shape[0]
        if len(labels) != B:
            raise ValueError(f"GpuPreprocessor: {len(labels)} label dicts for a batch of {B}")
        if params is None:
            params = self.sampler.draw(B)
        params = A.pack_samples(params)                      # once for the batch's launches
        out = dict(batch)
        for k in self.radar_keys:
            if k in out:
                out[k] = A.augment_radar(out[k], params, scale=self.scale)
        for k in self.camera_keys:
            if k in out:
                v = out[k]
                size = None if self.image_size is None else resized_output_size(v.shape[1], v.shape[2], self.image_size)
                out[k] = A.augment_camera(v, size, params)
        geo = [k for k in views if f"label_to_{k}_p" in out]
        new, labels = A.augment_geometry(
            [(out[f"label_to_{k}_t"], out[f"label_to_{k}_p"], out[f"{k}_shape"], k in self.camera_keys) for k in geo],
            labels, params)
        for k, (t, p) in zip(geo, new):
            out[f"label_to_{k}_t"], out[f"label_to_{k}_p"] = t, p
        return out, labels

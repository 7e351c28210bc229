"""Robustness conditions of the evaluator (optional, ``evaluate.robustness``; DESIGN.md section 3 "Sensor degradation").

    {"conditions": {"camera_off": {"camera": "off"}, "radar_off": {"radar": "off"},
                    "fog": {"camera": {"haze": 0.6, "blur": 2.0}},
                    "noisy": {"camera": {"noise": 15}, "radar": {"noise": 8}},
                    "sector": {"radar": {"azimuth_mask": [[0.4, 0.6]]}}},
     "seed": 0}

A condition is a FIXED degradation of the model's inputs (severities, not ranges; masks and erase rectangles as fractions of
the axis), applied on the device by the launches of dpft_amd/data/corrupt.py to the batch the evaluator has just scored clean.
``DataParallelEvaluator.evaluate_one_epoch`` runs one more forward per condition and batch and returns every metric mean and
split-level AP scalar once more as ``{key}/cond={name}``.  The noise key of a frame derives from (suite seed, condition name,
GLOBAL frame index): a condition's table does not depend on the number of ranks or on where the batches are cut.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch

from dpft_amd.data.corrupt import (DEFAULT_AIRLIGHT, MAX_BANDS, MAX_RECTS, MAX_SIGMA, CameraCorruption, RadarCorruption,
                                   _airlight, _hash64, _number, corrupt_batch)

_CAMERA_KEYS = ("blur", "haze", "noise", "erase", "airlight")
_RADAR_KEYS = ("noise", "azimuth_mask", "range_mask", "channels")


def _severity(where: str, v, top: float) -> float:
    if not _number(v) or not 0.0 <= v <= top:
        raise ValueError(f"{where} must be a number in [0, {top}], got {v!r}")
    return float(v)


def _fractions(where: str, v, n: int, most: int) -> List[tuple]:
    ok = isinstance(v, (list, tuple)) and len(v) <= most and all(
        isinstance(r, (list, tuple)) and len(r) == n and all(_number(x) and 0.0 <= x <= 1.0 for x in r) and
        all(r[i] <= r[i + 1] for i in range(0, n, 2)) for r in v)
    if not ok:
        raise ValueError(f"{where} must be a list of at most {most} entries of {n} fractions in [0, 1], each pair ordered, "
                         f"got {v!r}")
    return [tuple(float(x) for x in r) for r in v]


def parse_condition(name: str, value) -> Dict[str, Dict[str, Any]]:
    """One condition -> {"camera": kwargs of ``CameraCorruption``, "radar": kwargs of ``RadarCorruption``} (without keys)."""
    w = f"evaluate.robustness: condition {name!r}"
    if not isinstance(value, dict) or set(value) - {"camera", "radar"}:
        raise ValueError(f"{w}: expected {{'camera': ..., 'radar': ...}}, got {value!r}")
    cam, rad = value.get("camera", {}), value.get("radar", {})
    camera: Dict[str, Any] = {}
    if cam == "off":
        camera["off"] = True
    elif isinstance(cam, dict) and not set(cam) - set(_CAMERA_KEYS):
        camera["blur"] = _severity(f"{w}: camera.blur", cam.get("blur", 0.0), MAX_SIGMA)
        camera["haze"] = _severity(f"{w}: camera.haze", cam.get("haze", 0.0), 1.0)
        camera["noise"] = _severity(f"{w}: camera.noise", cam.get("noise", 0.0), 255.0)
        camera["airlight"] = _airlight(f"{w}: camera.airlight", cam.get("airlight", DEFAULT_AIRLIGHT))
        camera["erase"] = _fractions(f"{w}: camera.erase", cam.get("erase", []), 4, MAX_RECTS)
    else:
        raise ValueError(f"{w}: camera must be 'off' or a dict of {sorted(_CAMERA_KEYS)}, got {cam!r}")
    radar: Dict[str, Any] = {}
    if rad == "off":
        radar["off"] = True
    elif isinstance(rad, dict) and not set(rad) - set(_RADAR_KEYS):
        radar["noise"] = _severity(f"{w}: radar.noise", rad.get("noise", 0.0), 255.0)
        radar["azimuth"] = _fractions(f"{w}: radar.azimuth_mask", rad.get("azimuth_mask", []), 2, MAX_BANDS)
        radar["rows"] = _fractions(f"{w}: radar.range_mask", rad.get("range_mask", []), 2, MAX_BANDS)
        ch = rad.get("channels")
        if ch is not None and not (isinstance(ch, (list, tuple)) and ch and all(
                isinstance(c, int) and not isinstance(c, bool) and 0 <= c < 32 for c in ch)):
            raise ValueError(f"{w}: radar.channels must be a list of channel indices in 0..31 or null, got {ch!r}")
        radar["channels"] = None if ch is None else tuple(ch)
    else:
        raise ValueError(f"{w}: radar must be 'off' or a dict of {sorted(_RADAR_KEYS)}, got {rad!r}")
    return {"camera": camera, "radar": radar}


def parse_robustness(value) -> Dict[str, Any]:
    """``evaluate.robustness`` -> {"conditions": {name: parsed condition}, "seed": int}.  Anything malformed is a ValueError."""
    if not isinstance(value, dict) or set(value) - {"conditions", "seed"}:
        raise ValueError(f"evaluate.robustness: expected {{'conditions': {{name: ...}}, 'seed': ...}}, got {value!r}")
    conds = value.get("conditions")
    if not isinstance(conds, dict) or not conds:
        raise ValueError(f"evaluate.robustness: 'conditions' must be a non-empty dict of name -> condition, got {conds!r}")
    for name in conds:
        if not isinstance(name, str) or not name or any(ch in name for ch in "/= \t\n"):
            raise ValueError(f"evaluate.robustness: a condition name is a non-empty string without '/', '=' or blanks (it ends "
                             f"the scalar keys as /cond=name), got {name!r}")
    seed = value.get("seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"evaluate.robustness: seed must be an integer, got {seed!r}")
    return {"conditions": {name: parse_condition(name, c) for name, c in conds.items()}, "seed": seed}


class RobustnessSuite:
    """The parsed conditions and their application.  ``names`` keeps the config's order."""

    def __init__(self, spec, camera_keys: Sequence[str] = ("camera_mono", "camera_stereo"),
                 radar_keys: Sequence[str] = ("radar_bev", "radar_front"), lo: float = 0.0, hi: float = 255.0):
        spec = parse_robustness(spec)
        self.conditions, self.seed = spec["conditions"], spec["seed"]
        self.names = list(self.conditions)
        self.camera_keys, self.radar_keys, self.lo, self.hi = tuple(camera_keys), tuple(radar_keys), float(lo), float(hi)

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> Optional["RobustnessSuite"]:
        """``config['evaluate']['robustness']``; absent, null or false -> None."""
        spec = config.get("evaluate", {}).get("robustness")
        if spec is None or spec is False:
            return None
        return cls(spec)

    @staticmethod
    def scalar_key(key: str, name: str) -> str:
        """The name a scalar of condition ``name`` is returned under: after a group suffix where there is one."""
        return f"{key}/cond={name}"

    def noise_key(self, name: str, frame: int) -> int:
        return _hash64(f"dpft-robustness/{self.seed}/{name}/{int(frame)}")

    def params(self, name: str, first_frame: int, batch_size: int):
        c = self.conditions[name]
        keys = [self.noise_key(name, first_frame + b) for b in range(batch_size)]
        return ([CameraCorruption(key=k, **c["camera"]) for k in keys], [RadarCorruption(key=k, **c["radar"]) for k in keys])

    def apply(self, name: str, data: Dict[str, torch.Tensor], first_frame: int) -> Dict[str, torch.Tensor]:
        """The batch under condition ``name``: new tensors for the degraded views, everything else the same objects (a view
        the condition leaves alone is passed on as it is, without a launch).  ``first_frame``: global index of sample 0."""
        views = [k for k in self.camera_keys + self.radar_keys if k in data]
        if not views:
            return dict(data)
        cams, rads = self.params(name, first_frame, data[views[0]].shape[0])
        return corrupt_batch(data, cams, rads, self.camera_keys, self.radar_keys, self.lo, self.hi)

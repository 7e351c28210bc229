"""Rotated-box non-maximum suppression on the device, between the model and the consumers of its raw outputs (``Metric``, the
K-Radar exporter, ``DatasetAP``).  Optional and off by default: the reference has no such step -- it reads all N queries and trusts
the set loss to keep them apart -- so with ``evaluate.nms`` set the exported files and the metrics are no longer the reference's.

Definition (tests/nms_ref.py restates it line by line in numpy / Python fp64), per frame:

1. Candidates: query n whose argmax class c (first maximum, a NaN counts as the maximum) is not 0 and whose score s = cls[n, c] is
   not NaN.  Everything else is left untouched (status -2).  A candidate with not (s >= min_score), compared in fp32, gets
   status -3.
2. Order: score descending, ties by query index ascending, -0 orders as +0 (the key of ``DatasetAP``).
3. Greedy pass in that order: a candidate is suppressed by the FIRST earlier KEPT candidate -- of its own class unless
   ``class_agnostic`` -- whose IoU of ``kind`` ('bev' or '3d') with it is strictly greater than ``iou``; otherwise it is kept.  The
   IoUs are ``DatasetAP``'s: fp64 from the fp32 inputs, rotation (sin, cos) / hypot, no atan2, the earlier candidate clipped by
   the later one; a box with hypot = 0, failing min(lw, lh, wh) / 2 > 1e-4 or not finite has IoU 0 with everything: it is never
   suppressed and never suppresses.  A suppressed candidate suppresses nothing.
4. ``max_det``: kept candidates beyond the first ``max_det`` in order get status -4 (they did take part in step 3).
5. Results, all on the device without a read-back: ``status`` (B,N) int32 = -1 kept, -2 / -3 / -4 as above, otherwise the query
   index of the suppressor; ``order`` (B,N) int32 = the kept queries in score order, padded with -1; ``counts`` (B) int32;
   ``cls_out`` (B,N,C) = the bits of ``cls``, except that every row of status >= 0, -3 or -4 has element [n, 0] overwritten with the
   row's winning score: index 0 becomes the first maximum, so the query reads as background to ``Metric``, the exporter and
   ``DatasetAP`` without any change to those three.

Three launches per batch (``dpft_nms_f32``, csrc/nms.hip): sort, pairwise mask, greedy scan.  N <= 1024, C <= 16."""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch

KINDS = ("bev", "3d")
KEPT, NO_CANDIDATE, BELOW_MIN_SCORE, BEYOND_MAX_DET = -1, -2, -3, -4
_KEYS = ("iou", "kind", "class_agnostic", "min_score", "max_det")
_INT32_MAX = 0x7FFFFFFF


class RotatedNMS:
    def __init__(self, iou: float = 0.3, kind: str = "bev", class_agnostic: bool = False, min_score: Optional[float] = None,
                 max_det: Optional[int] = None):
        if isinstance(iou, bool) or not isinstance(iou, (int, float)) or not (0.0 < float(iou) < 1.0):
            raise ValueError(f"nms: 'iou' must lie inside (0, 1), got {iou!r}")
        if kind not in KINDS:
            raise ValueError(f"nms: 'kind' knows {KINDS}, got {kind!r}")
        if not isinstance(class_agnostic, bool):
            raise ValueError(f"nms: 'class_agnostic' must be true or false, got {class_agnostic!r}")
        if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float))
                                      or math.isnan(float(min_score))):
            raise ValueError(f"nms: 'min_score' must be a number or null, got {min_score!r}")
        if max_det is not None and (isinstance(max_det, bool) or not isinstance(max_det, int) or not 1 <= max_det <= _INT32_MAX):
            raise ValueError(f"nms: 'max_det' must be an integer >= 1 or null, got {max_det!r}")
        self.iou, self.kind, self.class_agnostic = float(iou), kind, class_agnostic
        self.min_score = None if min_score is None else float(min_score)
        self.max_det = max_det

    # ------------------------------------------------------------------------------------------------------- config
    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> Optional["RotatedNMS"]:
        """``config['evaluate']['nms']``: true (defaults) or a dict of iou / kind / class_agnostic / min_score / max_det.
        Absent or false -> None."""
        spec = config.get("evaluate", {}).get("nms")
        if spec is None or spec is False:
            return None
        if spec is True:
            spec = {}
        if not isinstance(spec, dict):
            raise ValueError(f"evaluate.nms must be true or a dict, got {spec!r}")
        unknown = sorted(set(spec) - set(_KEYS))
        if unknown:
            raise ValueError(f"evaluate.nms: unknown key(s) {unknown} ({', '.join(_KEYS)})")
        return cls(**spec)

    # ------------------------------------------------------------------------------------------------------- device
    def _launch(self, cls: torch.Tensor, center: torch.Tensor, size: torch.Tensor, angle: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """``dpft_nms_f32`` on contiguous fp32 tensors: (status, order, counts, cls_out)."""
        import ctypes as C
        from dpft_amd.hip.lib import HipLibraryError, lib, stream
        if not cls.is_cuda:
            raise HipLibraryError("dpft_amd RotatedNMS needs device tensors; there is no CPU path")
        B, N, ncls = cls.shape
        dev = cls.device
        nbytes = int(lib.dpft_nms_scratch_bytes(B, N))
        if nbytes < 0:
            raise HipLibraryError(lib.dpft_last_error().decode("utf-8", "replace"))
        scratch = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.int64, device=dev)
        status = torch.empty((B, N), dtype=torch.int32, device=dev)
        order = torch.empty((B, N), dtype=torch.int32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        cls_out = torch.empty_like(cls)
        if B == 0 or N == 0:
            return status, order, counts.zero_(), cls_out
        lib.call("dpft_nms_f32", cls.data_ptr(), center.data_ptr(), size.data_ptr(), angle.data_ptr(), (C.c_double * 1)(self.iou),
                 KINDS.index(self.kind), int(self.class_agnostic), -math.inf if self.min_score is None else self.min_score,
                 _INT32_MAX if self.max_det is None else self.max_det, scratch.data_ptr(), status.data_ptr(), order.data_ptr(),
                 counts.data_ptr(), cls_out.data_ptr(), B, N, ncls, stream())
        return status, order, counts, cls_out

    @torch.no_grad()
    def __call__(self, output: Dict[str, torch.Tensor]):
        """The model's ``output`` dict (class (B,N,C), center (B,N,3), size (B,N,3), angle (B,N,2) = [sin, cos]) ->
        (status, order, counts, cls_out) as the module docstring states them; no host wait."""
        cls = output["class"].detach().contiguous().float()
        center, size = output["center"].detach().contiguous().float(), output["size"].detach().contiguous().float()
        angle = output["angle"].detach().contiguous().float()
        if cls.dim() != 3 or center.shape != cls.shape[:2] + (3,) or size.shape != center.shape or angle.shape != cls.shape[:2] + (2,):
            raise ValueError(f"RotatedNMS: class (B,N,C), center (B,N,3), size (B,N,3), angle (B,N,2) expected, got "
                             f"{tuple(cls.shape)}, {tuple(center.shape)}, {tuple(size.shape)}, {tuple(angle.shape)}")
        return self._launch(cls, center, size, angle)

    def suppress(self, output: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """A new dict of the same type and key order: ``'class'`` is ``cls_out``, every other entry the same tensor object."""
        cls_out = self(output)[3]
        res = type(output)()
        for k, v in output.items():
            res[k] = cls_out if k == "class" else v
        return res

    @torch.no_grad()
    def detections(self, output: Dict[str, torch.Tensor]) -> List[torch.Tensor]:
        """Per frame the kept boxes as (counts[b], 10) fp32 rows [class, score, x, y, z, l, w, h, sin, cos] in score order, on the
        device.  Reads ``counts`` back (the one host wait of this class)."""
        _status, order, counts, _cls_out = self(output)
        cls = output["class"].detach().float()
        ncls = cls.shape[2]
        weight = torch.arange(ncls, 0, -1, device=cls.device)      # first maximum: the largest weight among the maxima
        res = []
        for b, n in enumerate(counts.tolist()):
            idx = order[b, :n].long()
            rows = cls[b, idx]
            score = rows.max(dim=1).values
            label = ((rows == score[:, None]) * weight).argmax(dim=1)
            res.append(torch.cat([label[:, None].float(), score[:, None], output["center"][b, idx].detach().float(),
                                  output["size"][b, idx].detach().float(), output["angle"][b, idx].detach().float()], dim=1))
        return res

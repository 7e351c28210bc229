"""Test-time augmentation on the device (optional, ``evaluate.tta``; DESIGN.md section 3 "Test-time augmentation"): a batch is
scored under T views -- the identity plus up to three flipped and / or camera-zoomed ones --, the boxes of the flipped views are
mirrored back and every cluster of agreeing boxes becomes one score-weighted box.  The reference has no such step: with the key set
the metrics and the exported files are no longer the reference's, and the output has T N rows instead of N.

    "evaluate": {"tta": true}                                     # = {"views": [{"flip": true}]}
    "evaluate": {"tta": {"views": [{"flip": true}, {"zoom": 1.1}, {"flip": true, "zoom": 0.9}],
                         "iou": 0.3, "kind": "bev", "score": "mean", "min_score": 0.0}}

The identity is always view 0 and is not listed; T = 1 + len(views), 2 <= T <= 4, T N <= 1024.  ``flip`` mirrors every view and the
six matrices exactly as ``train.augment`` does (dpft_amd/data/augment.py), ``zoom`` in [0.5, 2] is the camera zoom about the canvas
centre of the same module; the radar maps only flip.

Definition of the fusion (tests/tta_ref.py restates it line by line in numpy / Python fp64), per frame:

1. Un-mirror: row n of view t is candidate m = t N + n of the union; of a flipped view the sign BIT of ``center[1]`` and of
   ``angle[0]`` (the sin) is flipped -- the label rule of augment.py read backwards.  A zoom needs no undoing: boxes are in world
   coordinates.
2. Candidates, order and greedy clustering: ``RotatedNMS`` steps 1 to 3 (nms.py) on the union with ``iou``, ``kind`` and
   ``min_score``, class-aware, no ``max_det``.  A kept candidate HEADS a cluster; a suppressed one is a MEMBER of the cluster of the
   suppressor its status names.  A suppressed candidate suppresses nothing: if A suppresses B, and B overlaps C but A does not, C
   heads its own cluster.
3. Weights: w_i = fp64(s_i) if 0 < s_i < inf, else 0.  Members are visited in the union's score order, head first; every sum is a
   plain sequential fp64 sum in that order, every product is rounded before it is added.
4. A cluster of n >= 2 members with sum w > 0: ``center`` = sum w_i c_i / sum w_i, ``size`` likewise.  Heading: u_i = (sin_i,
   cos_i) / sqrt(sin_i^2 + cos_i^2); a member with u_i . u_head < 0 is left out of the heading sums (it still votes on centre and
   size): ``angle`` = sum' w_i u_i / sum' w_i; with sum' w = 0 (a head of weight 0 whose members all oppose it) the head's angle
   is kept.  Every result is rounded to fp32 once.  A cluster of one, or one with sum w = 0, keeps the head's eight floats bit
   for bit (invalid boxes have IoU 0 with everything: NaN / inf geometry only ever occurs here).
5. Fused score: ``"max"`` the head's; ``"mean"`` sum s_i / max(n, T) in fp64, rounded once -- the rule of Weighted Boxes Fusion:
   an object found in one of two views keeps half its score.
6. Rows of the output (B, T N, .): a head has the fused geometry and a class row of zeros but [c] = the fused score; a member
   or a row below ``min_score`` has its un-mirrored geometry bits and its class bits with [0] overwritten by the row's winning
   score (the convention of nms.py: it reads as background downstream); a row that is no candidate keeps everything.

Five launches per batch beside the T forwards: gather (``dpft_tta_gather_f32``), the three of ``dpft_nms_f32``, vote
(``dpft_tta_vote_f32``, csrc/tta.hip); no host wait."""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

KINDS = ("bev", "3d")
SCORES = ("mean", "max")
MAX_VIEWS, MAX_CANDIDATES, MAX_CLASSES = 4, 1024, 16
_KEYS = ("views", "iou", "kind", "score", "min_score")
_VIEW_KEYS = ("flip", "zoom")
_BOX_KEYS = ("class", "center", "size", "angle")
_INT32_MAX = 0x7FFFFFFF


def _number(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)


def parse_views(views) -> List[Tuple[bool, float]]:
    """``evaluate.tta.views`` -> [(flip, zoom)] of the listed views (the identity, view 0, is not among them)."""
    if not isinstance(views, (list, tuple)) or not 1 <= len(views) <= MAX_VIEWS - 1:
        raise ValueError(f"evaluate.tta: 'views' must list 1 to {MAX_VIEWS - 1} views (the identity is view 0 and is not listed: "
                         f"T = 1 + len(views) <= {MAX_VIEWS}), got {views!r}")
    out = []
    for v in views:
        if not isinstance(v, dict) or set(v) - set(_VIEW_KEYS):
            raise ValueError(f"evaluate.tta: a view is a dict of {_VIEW_KEYS}, got {v!r}")
        flip, zoom = v.get("flip", False), v.get("zoom", 1.0)
        if not isinstance(flip, bool):
            raise ValueError(f"evaluate.tta: a view's 'flip' must be true or false, got {flip!r}")
        if not _number(zoom) or not 0.5 <= zoom <= 2.0:
            raise ValueError(f"evaluate.tta: a view's 'zoom' must be a number in [0.5, 2], got {zoom!r}")
        if not flip and float(zoom) == 1.0:
            raise ValueError(f"evaluate.tta: the view {v!r} is the identity, which is view 0 already")
        out.append((flip, float(zoom)))
    return out


class TestTimeAugmentation:
    __test__ = False      # (not a test class, whatever the name says to pytest)

    def __init__(self, views: Sequence[Dict[str, Any]] = ({"flip": True},), iou: float = 0.3, kind: str = "bev",
                 score: str = "mean", min_score: float = 0.0, camera_keys: Sequence[str] = ("camera_mono", "camera_stereo"),
                 radar_keys: Sequence[str] = ("radar_bev", "radar_front")):
        self.view_specs = [(False, 1.0)] + parse_views(list(views) if isinstance(views, tuple) else views)
        if isinstance(iou, bool) or not isinstance(iou, (int, float)) or not (0.0 < float(iou) < 1.0):
            raise ValueError(f"evaluate.tta: 'iou' must lie inside (0, 1), got {iou!r}")
        if kind not in KINDS:
            raise ValueError(f"evaluate.tta: 'kind' knows {KINDS}, got {kind!r}")
        if score not in SCORES:
            raise ValueError(f"evaluate.tta: 'score' knows {SCORES}, got {score!r}")
        if not _number(min_score) or min_score < 0:
            raise ValueError(f"evaluate.tta: 'min_score' must be a number >= 0, got {min_score!r}")
        self.iou, self.kind, self.score, self.min_score = float(iou), kind, score, float(min_score)
        self.camera_keys, self.radar_keys = tuple(camera_keys), tuple(radar_keys)

    @property
    def T(self) -> int:
        return len(self.view_specs)

    @property
    def flips(self) -> List[bool]:
        return [f for f, _ in self.view_specs]

    # ------------------------------------------------------------------------------------------------------- config
    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> Optional["TestTimeAugmentation"]:
        """``config['evaluate']['tta']``: true (one flipped view) or a dict of views / iou / kind / score / min_score.  Absent
        or false -> None.  A flipped view needs ``data.fov`` symmetric about 0; T N <= 1024 is checked here where the config
        names the number of queries (``model.querent.resolution``), and in ``fuse`` in any case."""
        spec = config.get("evaluate", {}).get("tta")
        if spec is None or spec is False:
            return None
        if spec is True:
            spec = {}
        if not isinstance(spec, dict):
            raise ValueError(f"evaluate.tta must be true or a dict, got {spec!r}")
        unknown = sorted(set(spec) - set(_KEYS))
        if unknown:
            raise ValueError(f"evaluate.tta: unknown key(s) {unknown} ({', '.join(_KEYS)})")
        tta = cls(**spec)
        if any(tta.flips):
            from dpft_amd.data.augment import check_fov_symmetric
            try:
                check_fov_symmetric({"flip": 1.0}, config.get("data", {}).get("fov"))
            except ValueError as e:
                raise ValueError(str(e).replace("train.augment: flip > 0", "evaluate.tta: a flipped view")) from None
        res = config.get("model", {}).get("querent", {}).get("resolution")
        if isinstance(res, (list, tuple)) and res and all(isinstance(r, int) and not isinstance(r, bool) for r in res):
            tta.check_candidates(math.prod(res))
        return tta

    def check_candidates(self, N: int) -> None:
        if self.T * N > MAX_CANDIDATES:
            raise ValueError(f"evaluate.tta: T * N must be <= {MAX_CANDIDATES} (the limit of dpft_nms_f32 and of the consumers' "
                             f"sorts), got T = {self.T} views of N = {N} queries")

    # -------------------------------------------------------------------------------------------------------- views
    def views(self, data: Dict[str, Any]) -> List[Dict[str, Any]]:
        """The T batches: view 0 is ``data`` itself; a listed view is a new dict in which the flipped / zoomed camera frames,
        the flipped radar maps and the ``label_to_X_t`` / ``label_to_X_p`` matrices are new tensors made by the launches of
        dpft_amd/data/augment.py (no resize, no rescaling: the batch is preprocessed already), everything else the same objects.

        A flip-only view of an fp32 frame is the mirrored COPY of ``augment_radar(scale=False)``: the warp launch at the frame's
        own size computes top + 0 * bottom, which turns -0 into +0 and a finite pixel beside an inf into NaN."""
        from dpft_amd.data import augment as A
        out = [data]
        present = [k for k in self.camera_keys + self.radar_keys if k in data]
        for flip, zoom in self.view_specs[1:]:
            view = dict(data)
            if present:
                params = A.pack_samples([A.SampleParams(flip=flip, zoom=zoom)] * int(data[present[0]].shape[0]))
                for k in present:
                    v = data[k]
                    if k in self.camera_keys:
                        if zoom != 1.0 or v.dtype != torch.float32:
                            view[k] = A.augment_camera(v, None, params)
                        else:
                            view[k] = A.augment_radar(v, params, scale=False)
                    elif flip:
                        view[k] = A.augment_radar(v, params, scale=False)
                geo = [k for k in present if f"label_to_{k}_p" in data and f"label_to_{k}_t" in data and f"{k}_shape" in data]
                if geo:
                    new, _ = A.augment_geometry([(data[f"label_to_{k}_t"], data[f"label_to_{k}_p"], data[f"{k}_shape"],
                                                  k in self.camera_keys) for k in geo], None, params)
                    for k, (t, p) in zip(geo, new):
                        view[f"label_to_{k}_t"], view[f"label_to_{k}_p"] = t, p
            out.append(view)
        return out

    # ------------------------------------------------------------------------------------------------------- device
    def _launch(self, views: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]):
        """Gather, ``dpft_nms_f32`` on the union, vote, on contiguous fp32 (class, center, size, angle) per view:
        (status, order, counts, members, class, center, size, angle), the last four (B, T N, .)."""
        import ctypes as C
        from dpft_amd.hip.lib import HipLibraryError, TtaViews, lib, stream
        cls0 = views[0][0]
        if not all(t.is_cuda for v in views for t in v):
            raise HipLibraryError("dpft_amd TestTimeAugmentation needs device tensors; there is no CPU path")
        B, N, ncls = cls0.shape
        T, M, dev = len(views), len(views) * N, cls0.device
        nbytes = int(lib.dpft_tta_scratch_bytes(B, N, T))
        if nbytes < 0:
            raise HipLibraryError(lib.dpft_last_error().decode("utf-8", "replace"))
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        scratch = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.int64, device=dev)
        union = [torch.empty((B, M, w), **f32) for w in (ncls, 3, 3, 2)]
        cls_out, center, size, angle = (torch.empty((B, M, w), **f32) for w in (ncls, 3, 3, 2))
        status, order, members = (torch.empty((B, M), **i32) for _ in range(3))
        counts = torch.empty((B,), **i32)
        if B == 0 or N == 0:
            return status, order, counts.zero_(), members, cls_out, center, size, angle
        table = TtaViews()
        for t, (c, ce, sz, an) in enumerate(views):
            table.cls[t], table.center[t], table.size[t], table.angle[t] = c.data_ptr(), ce.data_ptr(), sz.data_ptr(), an.data_ptr()
            table.flip[t] = int(self.view_specs[t][0])
        s = stream()
        lib.call("dpft_tta_gather_f32", C.byref(table), T, *(u.data_ptr() for u in union), B, N, ncls, s)
        lib.call("dpft_nms_f32", *(u.data_ptr() for u in union), (C.c_double * 1)(self.iou), KINDS.index(self.kind), 0,
                 self.min_score, _INT32_MAX, scratch.data_ptr(), status.data_ptr(), order.data_ptr(), counts.data_ptr(),
                 cls_out.data_ptr(), B, M, ncls, s)
        lib.call("dpft_tta_vote_f32", union[1].data_ptr(), union[2].data_ptr(), union[3].data_ptr(), status.data_ptr(),
                 scratch.data_ptr(), SCORES.index(self.score), T, cls_out.data_ptr(), center.data_ptr(), size.data_ptr(),
                 angle.data_ptr(), members.data_ptr(), B, N, ncls, s)
        return status, order, counts, members, cls_out, center, size, angle

    def _run(self, outputs: Sequence[Dict[str, torch.Tensor]]):
        if len(outputs) != self.T:
            raise ValueError(f"TestTimeAugmentation: {self.T} views configured, got the outputs of {len(outputs)}")
        views = [tuple(o[k].detach().contiguous().float() for k in _BOX_KEYS) for o in outputs]
        cls = views[0][0]
        if cls.dim() != 3:
            raise ValueError(f"TestTimeAugmentation: class (B,N,C) expected, got {tuple(cls.shape)}")
        B, N, ncls = cls.shape
        for t, v in enumerate(views):
            want = ((B, N, ncls), (B, N, 3), (B, N, 3), (B, N, 2))
            if tuple(tuple(x.shape) for x in v) != want:
                raise ValueError(f"TestTimeAugmentation: view {t}: class (B,N,C), center (B,N,3), size (B,N,3), angle (B,N,2) of "
                                 f"view 0's B, N, C expected, got {[tuple(x.shape) for x in v]}")
        self.check_candidates(N)
        if not 2 <= ncls <= MAX_CLASSES:
            raise ValueError(f"TestTimeAugmentation: 2 <= C <= {MAX_CLASSES} classes, got {ncls}")
        return self._launch(views)

    @torch.no_grad()
    def clusters(self, outputs: Sequence[Dict[str, torch.Tensor]]):
        """(status, order, counts, members) of the union's clustering: ``RotatedNMS``'s three over the T N candidates, and
        ``members`` (B, T N) int32 = the size of the cluster a head leads, 0 elsewhere."""
        return self._run(outputs)[:4]

    @torch.no_grad()
    def fuse(self, outputs: Sequence[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
        """The T views' output dicts -> a dict of view 0's type and key order: ``class`` (B, T N, C), ``center`` / ``size``
        (B, T N, 3), ``angle`` (B, T N, 2) as the module docstring states them; any other key is view 0's, untouched."""
        fused = dict(zip(_BOX_KEYS, self._run(outputs)[4:]))
        res = type(outputs[0])()
        for k, v in outputs[0].items():
            res[k] = fused.get(k, v)
        return res

    @torch.no_grad()
    def forwards(self, model, data: Dict[str, Any]) -> List[Dict[str, torch.Tensor]]:
        """The model's outputs on the T views of ``data``; element 0 is the plain ``model(data)``."""
        return [model(v) for v in self.views(data)]

    @torch.no_grad()
    def __call__(self, model, data: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        return self.fuse(self.forwards(model, data))

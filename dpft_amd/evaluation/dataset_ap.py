"""Average precision of a whole split, AP_BEV and AP_3D per class at several IoU thresholds, accumulated on the device while the
evaluation loop runs (``dpft_dataset_ap_update_f32``: two launches per batch, no host wait; ``dpft_dataset_ap_finalize_f64``
once per epoch).  ``Metric`` (metric.py) mirrors the reference's per-frame mAP3D, which is averaged over steps; this is the
quantity of the K-Radar table instead -- one precision/recall curve per class over ALL frames.

NOT K-Radar's evaluation tool: that one follows KITTI's target-major two-pass protocol (difficulty levels, don't-care regions,
score thresholds chosen from the recall positions); this is the detection-major VOC order stated below.  The numbers are not
interchangeable with published ones: the export path (exporters/kradar.py) stays the way to official numbers.

Definition (tests/dataset_ap_ref.py restates it line by line in numpy fp64).  A combination is (IoU kind, threshold); there
are K = len(kinds) * len(iou) of them, kinds outermost.

* Detections of a frame: query n with argmax class c != 0 (first maximum, a NaN counts as the maximum), score s = cls[n, c],
  s >= min_score (fp32) and its centre strictly inside ``roi``.  A NaN score drops the query and counts in ``dropped_nan``.
* Ground truth of a frame: targets whose argmax class is c != 0 and whose centre is strictly inside ``roi``; they give npos[c].
  Targets outside the roi are no ground truth at all: they are neither counted nor matched.
* Boxes are (center, size, (sin, cos)); the rotation is (sin, cos) / hypot(sin, cos) in fp64 straight from the fp32 pair (no
  atan2).  A box with hypot = 0 or failing min(lw, lh, wh) / 2 > 1e-4 has IoU 0 with anything.  bev IoU = A / (l1 w1 + l2 w2 - A)
  with A the area of the rectangle clip, 3d IoU = A z / (v1 + v2 - A z) with z the overlap of the height intervals.
* Per frame, class and combination: detections by score descending (ties: query index ascending) each take, among the still
  unassigned targets of their class with IoU strictly greater than the threshold, the one with the largest IoU (ties: lower
  target index) and are a TP; otherwise an FP.
* Split: the records of a class ordered by (score desc, frame asc, query asc); prec(p) = TP(p) / (p + 1), rec(p) = TP(p) / npos;
  AP = (1 / R) sum_{i=1..R} max{prec(p) : rec(p) >= i / R} (0 where no p qualifies), NaN for a class with npos = 0.  mAP of a
  combination = mean over the classes with npos > 0 (NaN if there is none).
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence

import torch

KINDS = ("bev", "3d")
DEFAULT_ROI = (0.0, 72.0, -6.4, 6.4, -2.0, 6.0)      # the exporter's field of view (csrc/export.hip)
MAX_COMBINATIONS = 8
N_COUNTERS = 32
CURSOR, DROPPED_NAN, OVERFLOW, NPOS = 0, 1, 2, 16    # layout of the int64 counters (include/dpft_hip.h)
_DEFAULT = object()


def gather_state(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The collective behind ``DatasetAP.all_gather`` on a raw ``state()``: record counts all-gathered, records all-gathered
    padded to the maximum count and concatenated in rank order, counters all-reduced (the cursor becomes the total count).  The
    tensors stay on the device they are on."""
    import torch.distributed as dist
    world = dist.get_world_size()
    records, counters = state["records"], state["counters"].clone()
    n = torch.tensor([records.shape[0]], dtype=torch.int64, device=records.device)
    ns = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(ns, n)
    ns = [int(v) for v in ns]
    pad = torch.zeros((max(max(ns), 1), 4), dtype=torch.int32, device=records.device)
    pad[:records.shape[0]] = records
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    counters[CURSOR] = records.shape[0]
    dist.all_reduce(counters, op=dist.ReduceOp.SUM)
    return {"records": torch.cat([p[:k] for p, k in zip(parts, ns)]), "counters": counters}


class DatasetAP:
    def __init__(self, num_classes: int, iou: Sequence[float] = (0.3, 0.5, 0.7), kinds: Sequence[str] = KINDS,
                 recall_points: int = 40, min_score: float = 0.0, roi: Any = _DEFAULT, initial_capacity: int = 1 << 16):
        """``roi``: [xmin, xmax, ymin, ymax, zmin, zmax] (strict inequalities) or None for no filter; default = the exporter's
        box.  ``initial_capacity``: records the store holds before it first doubles."""
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 16:
            raise ValueError(f"dataset_ap: num_classes must be 2..16 (background + classes), got {num_classes!r}")
        iou = [iou] if isinstance(iou, (int, float)) and not isinstance(iou, bool) else iou
        if not isinstance(iou, (list, tuple)) or not iou:
            raise ValueError(f"dataset_ap: 'iou' must be a non-empty list of thresholds, got {iou!r}")
        for t in iou:
            if isinstance(t, bool) or not isinstance(t, (int, float)) or not (0.0 < float(t) < 1.0):
                raise ValueError(f"dataset_ap: 'iou' thresholds must lie inside (0, 1), got {t!r}")
        kinds = [kinds] if isinstance(kinds, str) else kinds
        if not isinstance(kinds, (list, tuple)) or not kinds or len(set(kinds)) != len(kinds):
            raise ValueError(f"dataset_ap: 'kinds' must be a non-empty subset of {KINDS}, got {kinds!r}")
        for k in kinds:
            if k not in KINDS:
                raise ValueError(f"dataset_ap: 'kinds' knows {KINDS}, got {k!r}")
        if len(kinds) * len(iou) > MAX_COMBINATIONS:
            raise ValueError(f"dataset_ap: 'kinds' x 'iou' gives {len(kinds) * len(iou)} combinations, at most {MAX_COMBINATIONS}")
        if isinstance(recall_points, bool) or not isinstance(recall_points, int) or not 2 <= recall_points <= 101:
            raise ValueError(f"dataset_ap: 'recall_points' must be an integer in 2..101, got {recall_points!r}")
        if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or math.isnan(float(min_score)):
            raise ValueError(f"dataset_ap: 'min_score' must be a number, got {min_score!r}")
        if roi is _DEFAULT:
            roi = DEFAULT_ROI
        if roi is not None:
            ok = isinstance(roi, (list, tuple)) and len(roi) == 6 and all(
                isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(float(v)) for v in roi)
            if not ok:
                raise ValueError(f"dataset_ap: 'roi' must be six finite numbers or null, got {roi!r}")
            roi = tuple(float(v) for v in roi)
        if isinstance(initial_capacity, bool) or not isinstance(initial_capacity, int) or initial_capacity < 1:
            raise ValueError(f"dataset_ap: initial_capacity must be a positive integer, got {initial_capacity!r}")
        self.num_classes, self.recall_points, self.min_score, self.roi = num_classes, recall_points, float(min_score), roi
        self.iou, self.kinds = [float(t) for t in iou], list(kinds)
        self.combinations = [(k, t) for k in self.kinds for t in self.iou]
        self.initial_capacity = initial_capacity
        self.reset()

    # ------------------------------------------------------------------------------------------------------- config
    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> Optional["DatasetAP"]:
        """``config['evaluate']['dataset_ap']``: true (defaults) or a dict of iou / kinds / recall_points / min_score / roi.
        Absent or false -> None.  The class count comes from ``config['model']['head']['num_classes']``."""
        spec = config.get("evaluate", {}).get("dataset_ap")
        if spec is None or spec is False:
            return None
        if spec is True:
            spec = {}
        if not isinstance(spec, dict):
            raise ValueError(f"evaluate.dataset_ap must be true or a dict, got {spec!r}")
        unknown = sorted(set(spec) - {"iou", "kinds", "recall_points", "min_score", "roi"})
        if unknown:
            raise ValueError(f"evaluate.dataset_ap: unknown key(s) {unknown} (iou, kinds, recall_points, min_score, roi)")
        try:
            ncls = config["model"]["head"]["num_classes"]
        except (KeyError, TypeError):
            raise ValueError("evaluate.dataset_ap needs model.head.num_classes") from None
        return cls(ncls, **spec)

    # -------------------------------------------------------------------------------------------------------- state
    def reset(self) -> None:
        self._records: Optional[torch.Tensor] = None      # (capacity, 4) int32 on the device
        self._counters: Optional[torch.Tensor] = None     # (N_COUNTERS) int64 on the device
        self._bound = 0                                   # host-known upper bound of the cursor: sum of B * N so far

    def _ensure(self, dev: torch.device, need: int) -> None:
        """Room for ``need`` records; grows by doubling from the host-known bound (never from the device cursor), with a
        device-to-device copy on the current stream."""
        if self._counters is None:
            self._counters = torch.zeros(N_COUNTERS, dtype=torch.int64, device=dev)
        cap = self._records.shape[0] if self._records is not None else 0
        if self._records is not None and cap >= need:
            return
        new_cap = max(cap, self.initial_capacity)
        while new_cap < need:
            new_cap *= 2
        new = torch.empty((new_cap, 4), dtype=torch.int32, device=dev)
        if self._records is not None and self._bound:
            new[:self._bound].copy_(self._records[:self._bound])
        self._records = new

    @property
    def capacity(self) -> int:
        return 0 if self._records is None else int(self._records.shape[0])

    @torch.no_grad()
    def update(self, output: Dict[str, torch.Tensor], labels: List[Dict[str, torch.Tensor]], first_frame: int) -> None:
        """The same ``output`` dict and label list as ``Metric.forward``; sample b is frame ``first_frame + b``."""
        import ctypes as C
        from dpft_amd.hip.lib import HipLibraryError, lib, stream
        from dpft_amd.training.loss import pack_targets
        cls = output["class"].detach().contiguous().float()
        if not cls.is_cuda:
            raise HipLibraryError("dpft_amd DatasetAP needs device tensors; there is no CPU path")
        center, size = output["center"].detach().contiguous().float(), output["size"].detach().contiguous().float()
        angle = output["angle"].detach().contiguous().float()
        B, N, ncls = cls.shape
        if ncls != self.num_classes:
            raise ValueError(f"DatasetAP built for {self.num_classes} classes, the output has {ncls}")
        if len(labels) != B:
            raise ValueError(f"DatasetAP.update: {B} samples but {len(labels)} label dicts")
        if not 0 <= int(first_frame) <= 0x7FFFFFFF - B:
            raise ValueError(f"DatasetAP.update: frame indices must fit a non-negative int32, got first_frame = {first_frame}")
        dev = cls.device
        counts = [int(t["gt_class"].shape[0]) for t in labels]
        gt_box, _onehot, gt_id, counts_t, Mmax = pack_targets(labels, counts, ncls, dev)
        nbytes = int(lib.dpft_dataset_ap_scratch_bytes(B, N, Mmax))
        if nbytes < 0:
            raise HipLibraryError(lib.dpft_last_error().decode("utf-8", "replace"))
        self._ensure(dev, self._bound + B * N)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        K = len(self.combinations)
        thr = (C.c_double * K)(*[t for _, t in self.combinations])
        kinds = (C.c_int32 * K)(*[KINDS.index(k) for k, _ in self.combinations])
        roi = (C.c_float * 6)(*self.roi) if self.roi is not None else None
        lib.call("dpft_dataset_ap_update_f32", cls.data_ptr(), center.data_ptr(), size.data_ptr(), angle.data_ptr(),
                 gt_box.data_ptr(), gt_id.data_ptr(), counts_t.data_ptr(), thr, kinds, K, roi, self.min_score,
                 scratch.data_ptr(), self._records.data_ptr(), self.capacity, self._bound, self._counters.data_ptr(),
                 int(first_frame), B, N, Mmax, ncls, stream())
        self._bound += B * N

    def state(self) -> Dict[str, torch.Tensor]:
        """The raw state: ``records`` (n, 4) int32 = score bits, frame, query | class << 16, TP bits (in arbitrary order) and
        the int64 ``counters`` ([0] = n, [1] dropped_nan, [16 + c] npos of class c).  Reads the cursor (a sync)."""
        if self._counters is None:
            return {"records": torch.empty((0, 4), dtype=torch.int32), "counters": torch.zeros(N_COUNTERS, dtype=torch.int64)}
        counters = self._counters.clone()
        host = counters.cpu()
        if int(host[OVERFLOW]):
            raise RuntimeError(f"DatasetAP: {int(host[OVERFLOW])} records did not fit the store (capacity {self.capacity})")
        return {"records": self._records[:int(host[CURSOR])].clone(), "counters": counters}

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        records, counters = state["records"], state["counters"]
        if records.dim() != 2 or records.shape[1] != 4 or records.dtype != torch.int32 or counters.shape != (N_COUNTERS,) \
                or counters.dtype != torch.int64:
            raise ValueError("DatasetAP.load_state: records must be (n, 4) int32 and counters (32) int64")
        n = int(records.shape[0])
        self.reset()
        if not records.is_cuda:
            if n or int(counters.abs().sum()):
                raise ValueError("DatasetAP.load_state needs device tensors")
            return
        self._bound = n
        self._ensure(records.device, n)
        self._records[:n].copy_(records)
        self._counters.copy_(counters)
        self._counters[CURSOR] = n

    def merge(self, other: "DatasetAP") -> None:
        """Concatenates the record stores and adds the counters (the frames of the two must not overlap)."""
        if (other.combinations, other.num_classes, other.recall_points) != (self.combinations, self.num_classes, self.recall_points):
            raise ValueError("DatasetAP.merge: the two accumulators differ in their parameters")
        a, b = self.state(), other.state()
        if not b["records"].is_cuda:
            return
        if not a["records"].is_cuda:
            self.load_state(b)
            return
        self.load_state({"records": torch.cat((a["records"], b["records"].to(a["records"].device))),
                         "counters": a["counters"] + b["counters"].to(a["counters"].device)})

    def all_gather(self) -> None:
        """Under ``torch.distributed`` with more than one rank: every rank ends up with all ranks' records and the summed
        counters (``gather_state``), so every rank computes the same table.  A no-op otherwise."""
        import torch.distributed as dist
        if not (dist.is_initialized() and dist.get_world_size() > 1):
            return
        st = self.state()
        if not st["records"].is_cuda:      # a rank that saw no batch still takes part in the collectives
            dev = torch.device("cuda", torch.cuda.current_device())
            st = {"records": st["records"].to(dev), "counters": st["counters"].to(dev)}
        self.load_state(gather_state(st))

    # ------------------------------------------------------------------------------------------------------- result
    @staticmethod
    def sort_records(records: torch.Tensor) -> torch.Tensor:
        """(class, score desc, frame asc, query asc): two stable integer sorts (-0 orders as +0)."""
        if records.shape[0] == 0:
            return records
        bits = records[:, 0].to(torch.int64) & 0xFFFFFFFF
        bits = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
        order = torch.where((bits & 0x80000000) != 0, ~bits & 0xFFFFFFFF, bits | 0x80000000)
        w2 = records[:, 2].to(torch.int64)
        minor = (records[:, 1].to(torch.int64) << 16) | (w2 & 0xFFFF)
        major = (((w2 >> 16) & 0xFF) << 32) | (0xFFFFFFFF - order)
        idx = torch.sort(minor, stable=True).indices
        idx = idx[torch.sort(major[idx], stable=True).indices]
        return records[idx].contiguous()

    def key(self, kind: str, thr: float) -> str:
        return f"{kind}@{thr:g}"

    @torch.no_grad()
    def compute(self) -> Dict[str, Any]:
        """Python floats under ``AP_{kind}@{iou}/{c}``, ``mAP_{kind}@{iou}``, ``npos/{c}``, ``dropped_nan``; the fp64 tensors
        ``ap`` (C-1, K), ``npos`` (C-1) and ``tp`` (C-1, K: TP totals) on the host."""
        from dpft_amd.hip.lib import lib, stream
        Cn, K = self.num_classes, len(self.combinations)
        if self._counters is None:
            ap = torch.full((Cn - 1, K), float("nan"), dtype=torch.float64)
            npos, tp, dropped = torch.zeros(Cn - 1, dtype=torch.float64), torch.zeros((Cn - 1, K), dtype=torch.float64), 0
        else:
            st = self.state()
            dev = st["counters"].device
            rec = self.sort_records(st["records"])
            n = int(rec.shape[0])
            cls_of = (rec[:, 2] >> 16) & 0xFF
            start = torch.searchsorted(cls_of.contiguous(), torch.arange(Cn + 1, dtype=cls_of.dtype, device=dev)).to(torch.int64)
            if n == 0:
                rec = torch.zeros((1, 4), dtype=torch.int32, device=dev)
            out = torch.empty((Cn - 1) * (2 * K + 1), dtype=torch.float64, device=dev)
            ap_d, tp_d, npos_d = out[:(Cn - 1) * K], out[(Cn - 1) * K:2 * (Cn - 1) * K], out[2 * (Cn - 1) * K:]
            lib.call("dpft_dataset_ap_finalize_f64", rec.data_ptr(), n, start.data_ptr(), st["counters"].data_ptr(), Cn, K,
                     self.recall_points, ap_d.data_ptr(), npos_d.data_ptr(), tp_d.data_ptr(), stream())
            host = out.cpu()
            ap, tp = host[:(Cn - 1) * K].reshape(Cn - 1, K), host[(Cn - 1) * K:2 * (Cn - 1) * K].reshape(Cn - 1, K)
            npos = host[2 * (Cn - 1) * K:]
            dropped = int(st["counters"][DROPPED_NAN])
        res: Dict[str, Any] = {}
        for k, (kind, thr) in enumerate(self.combinations):
            name = self.key(kind, thr)
            vals = [float(ap[c, k]) for c in range(Cn - 1) if float(npos[c]) > 0]
            for c in range(1, Cn):
                res[f"AP_{name}/{c}"] = float(ap[c - 1, k])
            res[f"mAP_{name}"] = sum(vals) / len(vals) if vals else float("nan")
        for c in range(1, Cn):
            res[f"npos/{c}"] = float(npos[c - 1])
        res["dropped_nan"] = float(dropped)
        res["ap"], res["npos"], res["tp"] = ap, npos, tp
        return res

    def scalars(self) -> Dict[str, float]:
        """``compute()`` without the tensors: what the evaluation loops return and log."""
        return {k: v for k, v in self.compute().items() if not isinstance(v, torch.Tensor)}

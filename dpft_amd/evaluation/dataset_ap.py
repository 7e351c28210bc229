"""Average precision of a whole split, AP_BEV and AP_3D per class at several IoU thresholds, accumulated on the device while the
evaluation loop runs (``dpft_dataset_ap_update_f32``: two launches per batch, no host wait; ``dpft_dataset_ap_finalize_f64``
once per epoch).  ``Metric`` (metric.py) mirrors the reference's per-frame mAP3D, which is averaged over steps; this is the
quantity of the K-Radar table instead -- one precision/recall curve per class over ALL frames.

NOT K-Radar's evaluation tool: that one follows KITTI's target-major two-pass protocol (difficulty levels, don't-care regions,
score thresholds chosen from the recall positions); this is the detection-major VOC order stated below.  The numbers are not
interchangeable with published ones: the export path (exporters/kradar.py) stays the way to official numbers.  ``kitti: true`` adds
a second table that follows that protocol for what the exporter writes ("KITTI protocol" below); the table here does not change.

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

Scene-description groups (``groups``; tests/dataset_ap_groups_ref.py restates them).  K-Radar's table per weather condition, time
of day and road type, which the exporter produces as one folder tree per subset, from the same accumulation:

* ``label["description"]`` is [road, time, weather], each truncated to an integer the way the exporter reads it (int()).
* Axes are "time", "road", "weather" (the exporter's order).  ``groups: true`` = all three, a list selects axes.
* The group list is ``all``, then one group per value of each selected axis (values ascending), named ``{axis}={name}`` with the
  names of the exporter's mappings (the ``data.*`` overrides included): at most 1 + 2 + 9 + 7 = 19 groups.
* A frame belongs to ``all`` and, per selected axis, to the group of its value.  A value outside the axis's mapping, or a
  non-finite one, puts the frame in no group of that axis; it still counts in ``all``, and ``bad_description`` counts the frames
  with such a value on at least one selected axis.
* The table of group g is the definition above applied to the frames of g and to nothing else: detections, ground truth, npos,
  the record order, the R-point envelope, NaN for npos = 0.  Per-frame matching does not change at all.

Device side with groups: ``dpft_dataset_ap_update_groups_f32`` instead of the update entry -- the SAME two launches; the workgroup
that owns a frame also writes one row of a frame store (frame, group bitmask, npos per class).  The descriptions add NO launch
and no copy: device tensors travel as pointers by value, host tensors as values in the kernel arguments (only a device
description that is neither contiguous nor fp32 / fp64 / int32 / int64 costs a conversion).  ``dpft_dataset_ap_finalize_groups_f64``
(two launches per epoch) replaces the finalize entry; its ``all`` group has the bits of the ungrouped table.

True-positive errors (``tp_errors``; tests/dataset_ap_tp_ref.py restates them with plain loops).  What is wrong with the boxes
that do match: translation in the ground plane, height, size, heading.  Matching stays the IoU rule above -- NOT a centre distance:
the numbers are not nuScenes' TP metrics and not K-Radar's, they only share the idea.

* ``tp_errors``: true, or {"at": [kind, iou], "min_recall": 0.1, "angle_period": "2pi" | "pi"}.  ``at`` is the reference
  combination and must be one of the configured ones; default = the first kind with the smallest threshold (the loosest match).
  A TP of the reference combination is exactly the (detection, target) pair the greedy walk above makes for it.
* Per TP, in fp64 straight from the fp32 inputs, in this operation order (d = detection, g = target):
  ``ate`` = sqrt(dx * dx + dy * dy), metres;  ``aze`` = |z_d - z_g|, metres;
  ``ase`` = 1 - P / (Vd + Vg - P) with P = min(l_d, l_g) * min(w_d, w_g) * min(h_d, h_g) and V = l * w * h, both multiplied left
  to right (one minus the IoU after aligning centre and heading);
  ``aoe`` = atan2(|s1 * c2 - c1 * s2|, c1 * c2 + s1 * s2) on the pairs (s, c) = (sin, cos) / hypot(sin, cos), in [0, pi];
  ``angle_period: "pi"`` makes it min(aoe, pi - aoe) (a box and its reverse count as the same).
* Each error is stored as the int64 q = rint(e * 2^32) (half to even): sums over TPs are exact and independent of order, so a
  group's table has the bits of an ungrouped run over its frames and a merge of ranks cannot move a bit.  An error that is not
  finite or whose magnitude is >= 2^20 stores 2^52 and counts in ``tp_saturated``; if that is non-zero every TP-error key is NaN.
* Per class over the records in (score desc, frame, query) order: T = running TP count of the reference combination, S_e =
  running integer sum of error e.  The TP with count T serves the recall points i (1..R) with floor((T - 1) * R / npos) < i <=
  min(floor(T * R / npos), R) (integers); the value there is float64(S_e) / 2^32 / float64(T), the cumulative mean.  The class's
  error is the mean of the served points with i >= i_min = max(1, ceil(min_recall * R)) (exact, from the decimal form of
  ``min_recall``: 0.1 * 40 gives 4), summed in ascending i and divided by their count; NaN when npos = 0 or no point is served.
* ``ATE/{c}``, ``AZE/{c}``, ``ASE/{c}``, ``AOE/{c}``, their means ``mATE`` .. ``mAOE`` over the classes that are not NaN,
  ``tp_points/{c}`` (served points averaged), ``tp_saturated``; with groups the same keys per group with the AP keys' suffix.

Device side with ``tp_errors``: ``dpft_dataset_ap_update_tp_f32`` / ``_groups_tp_f32`` instead of the update entries -- the SAME two
launches; the wave that owns the reference combination keeps the target it took, and the append loop writes one row of four
int64 into a second store at the record's position (zeros for a non-TP).  ``dpft_dataset_ap_finalize_tp_f64`` / ``_tp_groups_f64``
(one launch) runs beside the finalize entry on the error rows gathered by the records' sort permutation.

KITTI protocol (``kitti``; tests/dataset_ap_kitti_ref.py restates it literally with plain loops).  The table of KITTI's evaluation
tool, which K-Radar's tool follows, from the same accumulation and beside the table above.  NOT verified: K-Radar's tool is not
available to this project, equality with its output on a real export has not been checked, and the collapse of the difficulty
levels is argued from the exporter's constants, not observed.

* Shared with the table above: detections, ground truth, roi, ``min_score``, NaN handling, box geometry, both IoU kinds, the
  strict ``IoU > threshold`` rule, and npos[c].
* Detection order: a frame's detection order (its "file order") is ascending query index -- the exporter writes objects in query
  order.
* Difficulty levels and don't-care regions collapse: the exporter writes truncation 0, occlusion 0 and the 2-D box 50 50 150 150
  for every object, so every target is valid at every level and no detection is ever "ignored".  One table, not three.  The
  pass-2 reduction below DEPENDS on this: with ignored detections (don't-care areas, neighbouring classes) it does not hold.
* Pass 1, per frame, class and combination: targets in ascending index; each takes, among the detections of its class that are
  still unassigned and have IoU > thr, the one with the highest score (ties: lower query).  The tool runs this pass with score
  threshold 0.0: a detection with score < 0 takes no part (reachable only with a negative ``min_score``).  The taken detection is
  a pass-1 TP.
* Thresholds, per class and combination, from all pass-1 TP scores of the split in descending order (n1 of them), G = npos[c], in
  fp64 operation for operation as the tool does it::

      cur = 0.0
      for i in 0..n1-1:
          l = (i+1)/G
          r = (i+2)/G if i < n1-1 else l
          if (r - cur) < (cur - l) and i < n1-1: continue
          take score[i]
          cur += 1/40.0

  At most 41 thresholds.
* Pass 2, per threshold s: the active detections are those with score >= s.  Per frame, targets in ascending index; each takes,
  among the active unassigned detections of its class with IoU > thr, the one with the largest IoU (ties: lower query).  TP(s) =
  matched targets, FP(s) = active detections of the class that were not matched, FN(s) = G - TP(s).
* Table: prec[i] = TP / (TP + FP) and rec[i] = TP / G at threshold i, prec[i] = 0 for i at or beyond the number of thresholds;
  then the suffix maximum over i; ``AP`` (R40) = (prec[1] + .. + prec[40]) / 40, ``AP11`` = (prec[0] + prec[4] + .. + prec[40]) / 11,
  both summed in ascending i -- the tool's vintage decides which of the two a paper used.  npos = 0 gives NaN, targets without a
  TP give 0; mAP = mean over the classes with npos > 0.
* Keys: ``kitti/AP_{kind}@{iou}/{c}``, ``kitti/AP11_{kind}@{iou}/{c}``, ``kitti/mAP_{kind}@{iou}``, ``kitti/mAP11_{kind}@{iou}`` (with
  groups the same four per group with the AP keys' suffix) and the fp64 tensors ``kitti_ap``, ``kitti_ap11`` (C-1, K),
  ``kitti_prec`` (before the suffix maximum), ``kitti_rec``, ``kitti_thresholds`` (NaN-padded), ``kitti_tp``, ``kitti_fp``
  (C-1, K, 41), ``kitti_nthr`` (C-1, K) int32; with groups ``group_kitti_ap`` and ``group_kitti_ap11`` (G, C-1, K).
* True-positive errors stay on the VOC matching of the table above.

The two reductions of the device path (the reference file does NOT use them; tests/test_dataset_ap_kitti_ref.py compares the two
on random frames with ties in score and IoU):

1. Pass-1 bit: the pass-1 TP of target i is the first still-unassigned detection, in (score desc, query asc) order, with
   IoU > thr and score >= 0.
2. Pass-2 bit: insert the frame's detections one by one in (score desc, query asc) order into a maintained matching.  The
   entering detection x is offered to the targets in ascending index from start = 0 and goes to the first target t with
   IoU(x, t) > thr that is unmatched, or holds a smaller IoU, or holds an equal IoU from a higher query.  If t was unmatched the
   detection being INSERTED gets its bit and the insertion ends; otherwise the displaced detection becomes x, start = t + 1, and
   the offer goes on; if no target takes x no bit is set.  At most M steps.  Then for every s, TP(s) = the pass-2 bits of the
   detections with score >= s and FP(s) = their number minus TP(s): inside a group of equal scores the single bits depend on the
   insertion order, their sum does not, and a threshold always takes a whole tie group.

So the protocol over the split is two prefix sums over a class's records in the order they are sorted into anyway.  Device side
with ``kitti``: ``dpft_dataset_ap_update_kitti_f32`` instead of the update entries (groups and tp_errors by nullable arguments) --
the SAME two launches; after its own walk the wave that owns a combination does the two KITTI walks and the bits go into bits
8..15 (pass 1) and 16..23 (pass 2) of the record's fourth word, bits 0..7 stay the TP bits.  The record stays 16 bytes; store,
capacity rule, cursor atomic, counters, ``state()``, ``merge`` and ``all_gather`` are untouched: the bits travel with the records.
``dpft_dataset_ap_finalize_kitti_f64`` / ``_kitti_groups_f64`` (one launch) runs beside the finalize entry on the same sorted
records; a group's table has the bits of an ungrouped run over its frames (its own npos, its own thresholds).
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Any, Dict, List, Optional, Sequence

import torch

KINDS = ("bev", "3d")
KITTI_POINTS = 41                                    # sample points of the KITTI-protocol table (csrc/ap_kitti.h)
DEFAULT_ROI = (0.0, 72.0, -6.4, 6.4, -2.0, 6.0)      # the exporter's field of view (csrc/export.hip)
MAX_COMBINATIONS = 8
N_COUNTERS = 32
CURSOR, DROPPED_NAN, OVERFLOW, TP_SATURATED, NPOS = 0, 1, 2, 3, 16      # layout of the int64 counters (include/dpft_hip.h)
TP_ERRORS = ("ATE", "AZE", "ASE", "AOE")             # the columns of the error rows
ANGLE_PERIODS = ("2pi", "pi")
_DEFAULT = object()
AXES = ("time", "road", "weather")                   # the exporter's order (exporters/kradar.py _serialize_description)
_AXIS_COLUMN = {"road": 0, "time": 1, "weather": 2}  # description = [road, time, weather]
_AXIS_MAPPING = {"time": "time_zone", "road": "road_structures", "weather": "weather_conditions"}      # the data.* keys
FRAME_ROW = 18                                       # int32 per frame: frame, group bitmask, npos of classes 0..15
MAX_GROUP_BATCH, MAX_AXIS_VALUES, MAX_GROUPS = 64, 16, 32
_DESC_TYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3}
_DESC_HOST = 4


def _parse_groups(groups: Any) -> List[str]:
    """None / False -> []; True -> all axes; an axis name or a list of distinct names -> those, in the exporter's order."""
    if groups is None or groups is False:
        return []
    if groups is True:
        return list(AXES)
    axes = [groups] if isinstance(groups, str) else groups
    if not isinstance(axes, (list, tuple)) or not axes or not all(isinstance(a, str) for a in axes) \
            or len(set(axes)) != len(axes) or any(a not in AXES for a in axes):
        raise ValueError(f"dataset_ap: 'groups' must be true or a non-empty list of distinct axes out of {AXES}, got {groups!r}")
    return [a for a in AXES if a in axes]


def _parse_tp_errors(spec: Any, combinations: Sequence[tuple], kinds: Sequence[str], iou: Sequence[float],
                     recall_points: int) -> Optional[Dict[str, Any]]:
    """None / False -> None; True -> the defaults; a dict of at / min_recall / angle_period -> the parameters: ``at`` (kind,
    threshold), ``k`` its index among the combinations, ``min_recall``, ``i_min`` and ``angle_period``."""
    if spec is None or spec is False:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict):
        raise ValueError(f"dataset_ap: 'tp_errors' must be true or a dict of at / min_recall / angle_period, got {spec!r}")
    unknown = sorted(set(spec) - {"at", "min_recall", "angle_period"})
    if unknown:
        raise ValueError(f"dataset_ap: 'tp_errors' has unknown key(s) {unknown} (at, min_recall, angle_period)")
    at = spec.get("at")
    if at is None:
        at = (kinds[0], min(iou))
    ok = isinstance(at, (list, tuple)) and len(at) == 2 and isinstance(at[0], str) and isinstance(at[1], (int, float)) \
        and not isinstance(at[1], bool)
    if not ok or (at[0], float(at[1])) not in combinations:
        raise ValueError(f"dataset_ap: tp_errors 'at' must be one of the combinations {list(combinations)}, got {at!r}")
    at = (at[0], float(at[1]))
    min_recall = spec.get("min_recall", 0.1)
    if isinstance(min_recall, bool) or not isinstance(min_recall, (int, float)) or not 0.0 <= float(min_recall) <= 1.0:
        raise ValueError(f"dataset_ap: tp_errors 'min_recall' must be a number in [0, 1], got {min_recall!r}")
    period = spec.get("angle_period", "2pi")
    if not isinstance(period, str) or period not in ANGLE_PERIODS:
        raise ValueError(f"dataset_ap: tp_errors 'angle_period' must be one of {ANGLE_PERIODS}, got {period!r}")
    # exact: the decimal form of the number times R, so that 0.1 * 40 is 4 and not the 4.000000000000000222 of its binary form
    i_min = max(1, math.ceil(Fraction(repr(float(min_recall))) * recall_points))
    return {"at": at, "k": list(combinations).index(at), "min_recall": float(min_recall), "i_min": i_min, "angle_period": period}


def _axis_tables(axes: Sequence[str], mappings: Optional[Dict[str, Any]]) -> Dict[str, List[tuple]]:
    """axis -> [(value, name)] by ascending value, from the exporter's mappings (``mappings``: the exporter's keyword
    arguments road_structures / weather_conditions / time_zone as name -> value dicts, None = its defaults)."""
    from dpft_amd.evaluation.exporters.kradar import KRadarExporter
    mappings = mappings or {}
    unknown = sorted(set(mappings) - set(_AXIS_MAPPING.values()))
    if unknown:
        raise ValueError(f"dataset_ap: 'mappings' knows {sorted(_AXIS_MAPPING.values())}, got {unknown}")
    exporter = KRadarExporter(conf_thrs=[0.0], **{k: mappings.get(k) for k in _AXIS_MAPPING.values()})
    tables = {}
    for axis in axes:
        table = getattr(exporter, "_" + _AXIS_MAPPING[axis])                      # value -> name
        for v in table:
            if isinstance(v, bool) or not isinstance(v, int) or not -(1 << 31) <= v < (1 << 31):
                raise ValueError(f"dataset_ap: the values of {_AXIS_MAPPING[axis]} must be int32 integers, got {v!r}")
        if not 1 <= len(table) <= MAX_AXIS_VALUES:
            raise ValueError(f"dataset_ap: {_AXIS_MAPPING[axis]} must have 1..{MAX_AXIS_VALUES} distinct values, got {len(table)}")
        tables[axis] = sorted(table.items())
    return tables


def _gather_rows(rows: torch.Tensor) -> torch.Tensor:
    """All ranks' rows of a 2-D tensor, concatenated in rank order (counts all-gathered, rows padded to the maximum count)."""
    import torch.distributed as dist
    world = dist.get_world_size()
    n = torch.tensor([rows.shape[0]], dtype=torch.int64, device=rows.device)
    ns = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(ns, n)
    ns = [int(v) for v in ns]
    pad = torch.zeros((max(max(ns), 1), rows.shape[1]), dtype=rows.dtype, device=rows.device)
    pad[:rows.shape[0]] = rows
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    return torch.cat([p[:k] for p, k in zip(parts, ns)])


def gather_state(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The collective behind ``DatasetAP.all_gather`` on a raw ``state()``: record counts all-gathered, records all-gathered
    padded to the maximum count and concatenated in rank order, counters all-reduced (the cursor becomes the total count).  The
    frame rows of a grouped accumulator (``frames``) and the true-positive error rows (``tp_errors``), when the state has them, are
    gathered like the records.  The tensors stay on the device they are on."""
    import torch.distributed as dist
    records, counters = state["records"], state["counters"].clone()
    out = {"records": _gather_rows(records)}
    counters[CURSOR] = records.shape[0]
    dist.all_reduce(counters, op=dist.ReduceOp.SUM)
    out["counters"] = counters
    if "frames" in state:
        out["frames"] = _gather_rows(state["frames"])
    if "tp_errors" in state:
        out["tp_errors"] = _gather_rows(state["tp_errors"])
    return out


class DatasetAP:
    def __init__(self, num_classes: int, iou: Sequence[float] = (0.3, 0.5, 0.7), kinds: Sequence[str] = KINDS,
                 recall_points: int = 40, min_score: float = 0.0, roi: Any = _DEFAULT, initial_capacity: int = 1 << 16,
                 groups: Any = None, mappings: Optional[Dict[str, Any]] = None, initial_frame_capacity: int = 1 << 10,
                 tp_errors: Any = None, kitti: bool = False):
        """``roi``: [xmin, xmax, ymin, ymax, zmin, zmax] (strict inequalities) or None for no filter; default = the exporter's
        box.  ``initial_capacity``: records the store holds before it first doubles.  ``groups``: None, True (all axes) or a
        list out of "time", "road", "weather" -- one more table per scene-description subset; ``mappings``: the exporter's
        name -> value dicts under "time_zone" / "road_structures" / "weather_conditions" (None = its defaults);
        ``initial_frame_capacity``: frames the frame store holds before it first doubles.  ``tp_errors``: None, True or a dict of
        at / min_recall / angle_period -- the true-positive errors of one reference combination beside the AP.  ``kitti``:
        True adds the KITTI-protocol table (the ``kitti/`` keys) beside the VOC-order one."""
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
        self.tp = _parse_tp_errors(tp_errors, self.combinations, self.kinds, self.iou, recall_points)
        if kitti is None:
            kitti = False
        if not isinstance(kitti, bool):
            raise ValueError(f"dataset_ap: 'kitti' must be true or false, got {kitti!r}")
        self.kitti = kitti
        if isinstance(initial_frame_capacity, bool) or not isinstance(initial_frame_capacity, int) or initial_frame_capacity < 1:
            raise ValueError(f"dataset_ap: initial_frame_capacity must be a positive integer, got {initial_frame_capacity!r}")
        self.initial_frame_capacity = initial_frame_capacity
        self.axes = _parse_groups(groups)
        self.axis_tables = _axis_tables(self.axes, mappings) if self.axes else {}
        self.group_names = ["all"] + [f"{a}={name}" for a in self.axes for _, name in self.axis_tables[a]] if self.axes else []
        if len(self.group_names) > MAX_GROUPS:
            raise ValueError(f"dataset_ap: {len(self.group_names)} groups, at most {MAX_GROUPS}")
        self.reset()

    # ------------------------------------------------------------------------------------------------------- config
    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> Optional["DatasetAP"]:
        """``config['evaluate']['dataset_ap']``: true (defaults) or a dict of iou / kinds / recall_points / min_score / roi /
        groups / tp_errors / kitti.  Absent or false -> None.  The class count comes from ``config['model']['head']['num_classes']``; with
        ``groups`` (true, or a list out of "time", "road", "weather") the group names come from ``config['data']`` the way the
        exporter reads them (time_zone / road_structures / weather_conditions, absent = its defaults)."""
        spec = config.get("evaluate", {}).get("dataset_ap")
        if spec is None or spec is False:
            return None
        if spec is True:
            spec = {}
        if not isinstance(spec, dict):
            raise ValueError(f"evaluate.dataset_ap must be true or a dict, got {spec!r}")
        unknown = sorted(set(spec) - {"iou", "kinds", "recall_points", "min_score", "roi", "groups", "tp_errors", "kitti"})
        if unknown:
            raise ValueError(f"evaluate.dataset_ap: unknown key(s) {unknown} (iou, kinds, recall_points, min_score, roi, groups, "
                             f"tp_errors, kitti)")
        try:
            ncls = config["model"]["head"]["num_classes"]
        except (KeyError, TypeError):
            raise ValueError("evaluate.dataset_ap needs model.head.num_classes") from None
        if _parse_groups(spec.get("groups")):
            data = config.get("data") or {}
            return cls(ncls, mappings={k: data.get(k) for k in _AXIS_MAPPING.values()}, **spec)
        return cls(ncls, **spec)

    # -------------------------------------------------------------------------------------------------------- state
    def reset(self) -> None:
        self._records: Optional[torch.Tensor] = None      # (capacity, 4) int32 on the device
        self._counters: Optional[torch.Tensor] = None     # (N_COUNTERS) int64 on the device
        self._bound = 0                                   # host-known upper bound of the cursor: sum of B * N so far
        self._frames: Optional[torch.Tensor] = None       # groups only: (frame capacity, FRAME_ROW) int32 on the device
        self._nframes = 0                                 # rows of it written so far (host-known and exact: one per frame)
        self._tp_rows: Optional[torch.Tensor] = None      # tp_errors only: (capacity, 4) int64 on the device, beside the records

    def _ensure_frames(self, dev: torch.device, need: int) -> None:
        """Room for ``need`` frame rows, by doubling like the record store."""
        cap = self._frames.shape[0] if self._frames is not None else 0
        if self._frames is not None and cap >= need:
            return
        new_cap = max(cap, self.initial_frame_capacity)
        while new_cap < need:
            new_cap *= 2
        new = torch.empty((new_cap, FRAME_ROW), dtype=torch.int32, device=dev)
        if self._frames is not None and self._nframes:
            new[:self._nframes].copy_(self._frames[:self._nframes])
        self._frames = new

    @property
    def frame_capacity(self) -> int:
        return 0 if self._frames is None else int(self._frames.shape[0])

    def _descriptions(self, labels: List[Dict[str, torch.Tensor]], dev: torch.device):
        """The C arguments that carry the batch's descriptions (and the tensors that must outlive the launch): a device tensor
        goes as a pointer, a host one as three doubles, both by value in the kernel arguments."""
        import ctypes as C
        B = len(labels)
        ptrs, types, host, keep = (C.c_void_p * B)(), (C.c_int32 * B)(), (C.c_double * (3 * B))(), []
        for b, lab in enumerate(labels):
            d = lab.get("description") if isinstance(lab, dict) else None
            if d is None:
                raise ValueError(f"DatasetAP.update: groups need labels[{b}]['description'] = [road, time, weather]")
            d = torch.as_tensor(d).detach().reshape(-1)
            if d.numel() < 3:
                raise ValueError(f"DatasetAP.update: labels[{b}]['description'] needs [road, time, weather], got {d.numel()} value(s)")
            if d.is_cuda:
                if d.device != dev or d.dtype not in _DESC_TYPES or not d.is_contiguous():
                    d = d.to(device=dev, dtype=torch.float64).contiguous()
                keep.append(d)
                ptrs[b], types[b] = d.data_ptr(), _DESC_TYPES[d.dtype]
            else:
                types[b] = _DESC_HOST
                host[3 * b:3 * b + 3] = [float(v) for v in d[:3].to(torch.float64).tolist()]
        return ptrs, types, host, keep

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
        if self.tp is not None:                           # the error rows grow with the records: one row per record position
            rows = torch.empty((new_cap, 4), dtype=torch.int64, device=dev)
            if self._tp_rows is not None and self._bound:
                rows[:self._bound].copy_(self._tp_rows[:self._bound])
            self._tp_rows = rows
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
        if self.axes and B > MAX_GROUP_BATCH:      # the descriptions travel in the kernel arguments: 64 frames per launch
            for i in range(0, B, MAX_GROUP_BATCH):
                j = i + MAX_GROUP_BATCH
                self.update({"class": cls[i:j], "center": center[i:j], "size": size[i:j], "angle": angle[i:j]}, labels[i:j],
                            int(first_frame) + i)
            return
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
        args = (cls.data_ptr(), center.data_ptr(), size.data_ptr(), angle.data_ptr(), gt_box.data_ptr(), gt_id.data_ptr(),
                counts_t.data_ptr(), thr, kinds, K, roi, self.min_score, scratch.data_ptr(), self._records.data_ptr(),
                self.capacity, self._bound, self._counters.data_ptr(), int(first_frame), B, N, Mmax, ncls)
        tp = () if self.tp is None else (self._tp_rows.data_ptr(), self.tp["k"], int(self.tp["angle_period"] == "pi"))
        if self.kitti and not self.axes:       # one entry for every mix of groups and tp_errors: a null pointer switches each off
            lib.call("dpft_dataset_ap_update_kitti_f32", *args, None, None, None, None, None, None, 0, None, 0, 0,
                     *(tp or (None, 0, 0)), stream())
        elif not self.axes:
            lib.call("dpft_dataset_ap_update_tp_f32" if tp else "dpft_dataset_ap_update_f32", *args, *tp, stream())
        else:
            ptrs, types, host, _keep = self._descriptions(labels, dev)
            self._ensure_frames(dev, self._nframes + B)
            n_axes = len(self.axes)
            cols = (C.c_int32 * n_axes)(*[_AXIS_COLUMN[a] for a in self.axes])
            cnts = (C.c_int32 * n_axes)(*[len(self.axis_tables[a]) for a in self.axes])
            vals = (C.c_int32 * (n_axes * MAX_AXIS_VALUES))()
            for s, a in enumerate(self.axes):
                for i, (v, _) in enumerate(self.axis_tables[a]):
                    vals[s * MAX_AXIS_VALUES + i] = v
            group_args = (ptrs, types, host, cols, cnts, vals, n_axes, self._frames.data_ptr(), self.frame_capacity, self._nframes)
            if self.kitti:
                lib.call("dpft_dataset_ap_update_kitti_f32", *args, *group_args, *(tp or (None, 0, 0)), stream())
            else:
                lib.call("dpft_dataset_ap_update_groups_tp_f32" if tp else "dpft_dataset_ap_update_groups_f32", *args, *group_args,
                         *tp, stream())
            self._nframes += B
        self._bound += B * N

    def state(self) -> Dict[str, torch.Tensor]:
        """The raw state: ``records`` (n, 4) int32 = score bits, frame, query | class << 16, TP bits (in arbitrary order) and
        the int64 ``counters`` ([0] = n, [1] dropped_nan, [16 + c] npos of class c).  Reads the cursor (a sync).  With groups
        also ``frames`` (F, 18) int32 = frame, group bitmask, npos of classes 0..15 of every frame seen (in arbitrary order).  With
        ``tp_errors`` also ``tp_errors`` (n, 4) int64 parallel to ``records`` = ate, aze, ase, aoe of a TP of the reference
        combination as rint(e * 2^32), zeros otherwise (counters[3] = errors that did not fit).  With ``kitti`` the records' fourth
        word also holds the pass-1 bits (8..15) and the pass-2 bits (16..23) of the KITTI protocol."""
        if self._counters is None:
            st = {"records": torch.empty((0, 4), dtype=torch.int32), "counters": torch.zeros(N_COUNTERS, dtype=torch.int64)}
            if self.axes:
                st["frames"] = torch.empty((0, FRAME_ROW), dtype=torch.int32)
            if self.tp is not None:
                st["tp_errors"] = torch.empty((0, 4), dtype=torch.int64)
            return st
        counters = self._counters.clone()
        host = counters.cpu()
        if int(host[OVERFLOW]):
            raise RuntimeError(f"DatasetAP: {int(host[OVERFLOW])} records did not fit the store (capacity {self.capacity})")
        st = {"records": self._records[:int(host[CURSOR])].clone(), "counters": counters}
        if self.axes:
            st["frames"] = self._frames[:self._nframes].clone() if self._frames is not None else \
                torch.empty((0, FRAME_ROW), dtype=torch.int32, device=counters.device)
        if self.tp is not None:
            st["tp_errors"] = self._tp_rows[:int(host[CURSOR])].clone()
        return st

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        records, counters = state["records"], state["counters"]
        if records.dim() != 2 or records.shape[1] != 4 or records.dtype != torch.int32 or counters.shape != (N_COUNTERS,) \
                or counters.dtype != torch.int64:
            raise ValueError("DatasetAP.load_state: records must be (n, 4) int32 and counters (32) int64")
        frames = state.get("frames") if self.axes else None
        if self.axes and (frames is None or frames.dim() != 2 or frames.shape[1] != FRAME_ROW or frames.dtype != torch.int32
                          or frames.is_cuda != records.is_cuda):
            raise ValueError(f"DatasetAP.load_state: with groups the state needs 'frames' (F, {FRAME_ROW}) int32 beside the records")
        rows = state.get("tp_errors") if self.tp is not None else None
        if self.tp is not None and (rows is None or rows.shape != (records.shape[0], 4) or rows.dtype != torch.int64
                                    or rows.is_cuda != records.is_cuda):
            raise ValueError("DatasetAP.load_state: with tp_errors the state needs 'tp_errors' (n, 4) int64 beside the records")
        n = int(records.shape[0])
        self.reset()
        if not records.is_cuda:
            if n or int(counters.abs().sum()):
                raise ValueError("DatasetAP.load_state needs device tensors")
            return
        self._bound = n
        self._ensure(records.device, n)
        self._records[:n].copy_(records)
        if rows is not None:
            self._tp_rows[:n].copy_(rows)
        self._counters.copy_(counters)
        self._counters[CURSOR] = n
        if frames is not None:
            self._ensure_frames(records.device, int(frames.shape[0]))
            self._frames[:frames.shape[0]].copy_(frames)
            self._nframes = int(frames.shape[0])

    def merge(self, other: "DatasetAP") -> None:
        """Concatenates the record stores (with groups also the frame stores, with tp_errors also the error rows) and adds the
        counters (the frames of the two must not overlap)."""
        if (other.combinations, other.num_classes, other.recall_points, other.group_names, other.axis_tables, other.tp,
                other.kitti) != (self.combinations, self.num_classes, self.recall_points, self.group_names, self.axis_tables,
                                 self.tp, self.kitti):
            raise ValueError("DatasetAP.merge: the two accumulators differ in their parameters")
        a, b = self.state(), other.state()
        if not b["records"].is_cuda:
            return
        if not a["records"].is_cuda:
            self.load_state(b)
            return
        st = {"records": torch.cat((a["records"], b["records"].to(a["records"].device))),
              "counters": a["counters"] + b["counters"].to(a["counters"].device)}
        if self.axes:
            st["frames"] = torch.cat((a["frames"], b["frames"].to(a["frames"].device)))
        if self.tp is not None:
            st["tp_errors"] = torch.cat((a["tp_errors"], b["tp_errors"].to(a["tp_errors"].device)))
        self.load_state(st)

    def all_gather(self) -> None:
        """Under ``torch.distributed`` with more than one rank: every rank ends up with all ranks' records and the summed
        counters (``gather_state``; with groups also all ranks' frame rows, with tp_errors the error rows), so every rank computes
        the same table.  A no-op
        otherwise."""
        import torch.distributed as dist
        if not (dist.is_initialized() and dist.get_world_size() > 1):
            return
        st = self.state()
        if not st["records"].is_cuda:      # a rank that saw no batch still takes part in the collectives
            dev = torch.device("cuda", torch.cuda.current_device())
            st = {k: v.to(dev) for k, v in st.items()}
        self.load_state(gather_state(st))

    # ------------------------------------------------------------------------------------------------------- result
    @staticmethod
    def sort_records(records: torch.Tensor) -> torch.Tensor:
        """(class, score desc, frame asc, query asc): two stable integer sorts (-0 orders as +0)."""
        if records.shape[0] == 0:
            return records
        return records[DatasetAP.sort_permutation(records)].contiguous()

    @staticmethod
    def sort_permutation(records: torch.Tensor) -> torch.Tensor:
        """The permutation ``sort_records`` applies (for the rows that travel beside the records)."""
        bits = records[:, 0].to(torch.int64) & 0xFFFFFFFF
        bits = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
        order = torch.where((bits & 0x80000000) != 0, ~bits & 0xFFFFFFFF, bits | 0x80000000)
        w2 = records[:, 2].to(torch.int64)
        minor = (records[:, 1].to(torch.int64) << 16) | (w2 & 0xFFFF)
        major = (((w2 >> 16) & 0xFF) << 32) | (0xFFFFFFFF - order)
        idx = torch.sort(minor, stable=True).indices
        return idx[torch.sort(major[idx], stable=True).indices]

    def key(self, kind: str, thr: float) -> str:
        return f"{kind}@{thr:g}"

    @torch.no_grad()
    def compute(self) -> Dict[str, Any]:
        """Python floats under ``AP_{kind}@{iou}/{c}``, ``mAP_{kind}@{iou}``, ``npos/{c}``, ``dropped_nan``; the fp64 tensors
        ``ap`` (C-1, K), ``npos`` (C-1) and ``tp`` (C-1, K: TP totals) on the host.  With groups also, per group other than
        ``all``, ``AP_{kind}@{iou}/{c}/{axis}={name}``, ``mAP_{kind}@{iou}/{axis}={name}``, ``npos/{c}/{axis}={name}`` and
        ``nframes/{axis}={name}``, the count ``bad_description``, the fp64 tensors ``group_ap`` (G, C-1, K), ``group_tp``
        (G, C-1, K), ``group_npos`` (G, C-1), ``group_nframes`` (G) and the list ``group_names`` (``all`` first); the keys
        without a group are then the ``all`` group's.  With ``tp_errors`` also ``ATE/{c}``, ``AZE/{c}``, ``ASE/{c}``,
        ``AOE/{c}``, ``mATE`` .. ``mAOE``, ``tp_points/{c}`` (with the group suffix of the AP keys), ``tp_saturated`` and the fp64
        tensors ``tp_err`` (C-1, 4), ``tp_points`` (C-1), with groups ``group_tp_err`` (G, C-1, 4) and ``group_tp_points``
        (G, C-1); every TP-error value is NaN when ``tp_saturated`` is not zero.  With ``kitti`` also the ``kitti/`` scalars and the
        ``kitti_*`` tensors of the module docstring's "KITTI protocol" (one more launch, on the same sorted records)."""
        from dpft_amd.hip.lib import lib, stream
        Cn, K = self.num_classes, len(self.combinations)
        groups = None
        tp_err, tp_points = torch.full((Cn - 1, 4), float("nan"), dtype=torch.float64), torch.zeros(Cn - 1, dtype=torch.float64)
        saturated = 0
        kitti = None
        if self.axes:
            groups = self._compute_groups()
            kitti = groups.pop("kitti", None)
            ap, tp, npos, dropped = groups["group_ap"][0], groups["group_tp"][0], groups["group_npos"][0], groups.pop("dropped")
            if self.tp is not None:
                tp_err, tp_points, saturated = groups["group_tp_err"][0], groups["group_tp_points"][0], groups.pop("saturated")
        elif self._counters is None:
            ap = torch.full((Cn - 1, K), float("nan"), dtype=torch.float64)
            npos, tp, dropped = torch.zeros(Cn - 1, dtype=torch.float64), torch.zeros((Cn - 1, K), dtype=torch.float64), 0
            if self.kitti:
                kitti = self._kitti_finalize(None, 0, None, None)
        else:
            st = self.state()
            dev = st["counters"].device
            n = int(st["records"].shape[0])
            perm = self.sort_permutation(st["records"]) if n else None
            rec = st["records"][perm].contiguous() if n else st["records"]
            cls_of = (rec[:, 2] >> 16) & 0xFF
            start = torch.searchsorted(cls_of.contiguous(), torch.arange(Cn + 1, dtype=cls_of.dtype, device=dev)).to(torch.int64)
            if n == 0:
                rec = torch.zeros((1, 4), dtype=torch.int32, device=dev)
            base = (Cn - 1) * (2 * K + 1)
            out = torch.empty(base + ((Cn - 1) * 5 if self.tp is not None else 0), dtype=torch.float64, device=dev)
            ap_d, tp_d, npos_d = out[:(Cn - 1) * K], out[(Cn - 1) * K:2 * (Cn - 1) * K], out[2 * (Cn - 1) * K:]
            lib.call("dpft_dataset_ap_finalize_f64", rec.data_ptr(), n, start.data_ptr(), st["counters"].data_ptr(), Cn, K,
                     self.recall_points, ap_d.data_ptr(), npos_d.data_ptr(), tp_d.data_ptr(), stream())
            if self.tp is not None:      # the error rows by the records' permutation; one more launch, the same read-back
                rows = st["tp_errors"][perm].contiguous() if n else torch.zeros((1, 4), dtype=torch.int64, device=dev)
                lib.call("dpft_dataset_ap_finalize_tp_f64", rec.data_ptr(), rows.data_ptr(), n, start.data_ptr(),
                         st["counters"].data_ptr(), Cn, self.tp["k"], self.recall_points, self.tp["i_min"], out[base:].data_ptr(),
                         out[base + (Cn - 1) * 4:].data_ptr(), stream())
            if self.kitti:               # one more launch over the same sorted records
                kitti = self._kitti_finalize(rec, n, start, st["counters"])
            host = out.cpu()
            ap, tp = host[:(Cn - 1) * K].reshape(Cn - 1, K), host[(Cn - 1) * K:2 * (Cn - 1) * K].reshape(Cn - 1, K)
            npos = host[2 * (Cn - 1) * K:base]
            counters = st["counters"].cpu()
            dropped = int(counters[DROPPED_NAN])
            if self.tp is not None:
                tp_err, tp_points = host[base:base + (Cn - 1) * 4].reshape(Cn - 1, 4), host[base + (Cn - 1) * 4:]
                saturated = int(counters[TP_SATURATED])
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
        if self.tp is not None:
            if saturated:                # an error did not fit the fixed point: no plausible number comes out of its sums
                tp_err = torch.full_like(tp_err, float("nan"))
            self._tp_keys(res, tp_err.tolist(), tp_points.tolist(), "")
            res["tp_saturated"] = float(saturated)
            res["tp_err"], res["tp_points"] = tp_err, tp_points
        if kitti is not None:            # [0] = the only table, or the ``all`` group's
            self._kitti_keys(res, kitti["ap"][0].tolist(), kitti["ap11"][0].tolist(), npos.tolist(), "")
            for k, v in kitti.items():
                res[f"kitti_{k}"] = v[0]
        if groups is not None:
            all_ap, all_npos, all_nframes = (groups[k].tolist() for k in ("group_ap", "group_npos", "group_nframes"))
            for g, gname in enumerate(self.group_names[1:], 1):      # (plain lists: ~800 reads of a host tensor cost milliseconds)
                gap, gnpos = all_ap[g], all_npos[g]
                for k, (kind, thr) in enumerate(self.combinations):
                    name = self.key(kind, thr)
                    vals = [gap[c][k] for c in range(Cn - 1) if gnpos[c] > 0]
                    for c in range(1, Cn):
                        res[f"AP_{name}/{c}/{gname}"] = gap[c - 1][k]
                    res[f"mAP_{name}/{gname}"] = sum(vals) / len(vals) if vals else float("nan")
                for c in range(1, Cn):
                    res[f"npos/{c}/{gname}"] = gnpos[c - 1]
                res[f"nframes/{gname}"] = all_nframes[g]
            if self.tp is not None:
                if saturated:
                    groups["group_tp_err"] = torch.full_like(groups["group_tp_err"], float("nan"))
                all_err, all_points = groups["group_tp_err"].tolist(), groups["group_tp_points"].tolist()
                for g, gname in enumerate(self.group_names[1:], 1):
                    self._tp_keys(res, all_err[g], all_points[g], "/" + gname)
            if kitti is not None:
                all_kap, all_kap11 = kitti["ap"].tolist(), kitti["ap11"].tolist()
                for g, gname in enumerate(self.group_names[1:], 1):
                    self._kitti_keys(res, all_kap[g], all_kap11[g], all_npos[g], "/" + gname)
                res["group_kitti_ap"], res["group_kitti_ap11"] = kitti["ap"], kitti["ap11"]
            res["bad_description"] = float(groups.pop("bad"))
            res.update(groups)
            res["group_names"] = list(self.group_names)
        return res

    def _kitti_finalize(self, rec: Optional[torch.Tensor], n: int, start: Optional[torch.Tensor], counters: Optional[torch.Tensor],
                        rec_groups: Optional[torch.Tensor] = None, group_npos: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The KITTI-protocol table of the sorted records (``rec`` None: nothing accumulated) as host tensors with a leading
        group axis: ap, ap11 (G, C-1, K), prec, rec, thresholds, tp, fp (G, C-1, K, 41), nthr (G, C-1, K) int32.  One launch
        (``dpft_dataset_ap_finalize_kitti_f64`` or ``_groups_f64`` with the group masks and the group npos on the device)."""
        from dpft_amd.hip.lib import lib, stream
        Cn, K, G = self.num_classes, len(self.combinations), max(len(self.group_names), 1)
        cells = G * (Cn - 1) * K
        names, sizes = ("ap", "ap11", "prec", "rec", "thresholds", "tp", "fp"), (1, 1) + (KITTI_POINTS,) * 5
        if rec is None:
            out = {k: torch.zeros((G, Cn - 1, K) + ((w,) if w > 1 else ()), dtype=torch.float64) for k, w in zip(names, sizes)}
            for k in ("ap", "ap11", "thresholds"):
                out[k].fill_(float("nan"))
            out["nthr"] = torch.zeros((G, Cn - 1, K), dtype=torch.int32)
            return out
        dev = rec.device
        buf = torch.empty(cells * sum(sizes), dtype=torch.float64, device=dev)
        nthr = torch.empty(cells, dtype=torch.int32, device=dev)
        offs = [cells * sum(sizes[:i]) for i in range(len(sizes))]
        ptrs = [buf[o:].data_ptr() for o in offs]
        if rec_groups is None:
            lib.call("dpft_dataset_ap_finalize_kitti_f64", rec.data_ptr(), n, start.data_ptr(), counters.data_ptr(), Cn, K, *ptrs,
                     nthr.data_ptr(), stream())
        else:
            lib.call("dpft_dataset_ap_finalize_kitti_groups_f64", rec.data_ptr(), rec_groups.data_ptr(), n, start.data_ptr(),
                     group_npos.data_ptr(), G, Cn, K, *ptrs, nthr.data_ptr(), stream())
        host = buf.cpu()
        out = {k: host[o:o + cells * w].reshape((G, Cn - 1, K) + ((w,) if w > 1 else ())) for k, w, o in zip(names, sizes, offs)}
        out["nthr"] = nthr.cpu().reshape(G, Cn - 1, K)
        return out

    def _kitti_keys(self, res: Dict[str, Any], ap: List[List[float]], ap11: List[List[float]], npos: List[float], tail: str) -> None:
        """The KITTI scalars of one table (``tail`` = the group suffix): AP (R40) and AP11 per class and combination, and their
        means over the classes with ground truth."""
        Cn = self.num_classes
        for k, (kind, thr) in enumerate(self.combinations):
            name = self.key(kind, thr)
            for label, table in (("AP", ap), ("AP11", ap11)):
                vals = [table[c][k] for c in range(Cn - 1) if npos[c] > 0]
                for c in range(1, Cn):
                    res[f"kitti/{label}_{name}/{c}{tail}"] = table[c - 1][k]
                res[f"kitti/m{label}_{name}{tail}"] = sum(vals) / len(vals) if vals else float("nan")

    def _tp_keys(self, res: Dict[str, Any], err: List[List[float]], points: List[float], tail: str) -> None:
        """The TP-error scalars of one table (``tail`` = the group suffix): per class, and the mean over the classes that are not
        NaN."""
        for e, name in enumerate(TP_ERRORS):
            vals = [err[c][e] for c in range(self.num_classes - 1) if err[c][e] == err[c][e]]
            for c in range(1, self.num_classes):
                res[f"{name}/{c}{tail}"] = err[c - 1][e]
            res[f"m{name}{tail}"] = sum(vals) / len(vals) if vals else float("nan")
        for c in range(1, self.num_classes):
            res[f"tp_points/{c}{tail}"] = points[c - 1]

    def _compute_groups(self) -> Dict[str, Any]:
        """The grouped finalize: the records sorted as always, every record's group bitmask looked up in the frame store by its
        frame index (one more sort and a searchsorted), then ``dpft_dataset_ap_finalize_groups_f64`` and one read-back."""
        import ctypes as C
        from dpft_amd.hip.lib import lib, stream
        Cn, K, G = self.num_classes, len(self.combinations), len(self.group_names)
        sizes = (G * (Cn - 1) * K, G * (Cn - 1) * K, G * (Cn - 1), G, 1)          # ap, tp, npos, nframes, bad
        if self.tp is not None:
            sizes += (G * (Cn - 1) * 4, G * (Cn - 1))                             # tp_err, tp_points
        saturated = 0
        if self._counters is None:
            host = torch.cat([torch.full((sizes[0],), float("nan"), dtype=torch.float64),
                              torch.zeros(sum(sizes[1:5]), dtype=torch.float64)])
            if self.tp is not None:
                host = torch.cat([host, torch.full((sizes[5],), float("nan"), dtype=torch.float64),
                                  torch.zeros(sizes[6], dtype=torch.float64)])
            dropped = 0
            kitti = self._kitti_finalize(None, 0, None, None) if self.kitti else None
        else:
            st = self.state()
            dev = st["counters"].device
            n, F = int(st["records"].shape[0]), int(st["frames"].shape[0])
            perm = self.sort_permutation(st["records"]) if n else None
            rec = st["records"][perm].contiguous() if n else st["records"]
            cls_of = (rec[:, 2] >> 16) & 0xFF
            start = torch.searchsorted(cls_of.contiguous(), torch.arange(Cn + 1, dtype=cls_of.dtype, device=dev)).to(torch.int64)
            if n and F:
                order = torch.sort(st["frames"][:, 0]).indices
                frame_of, mask_of = st["frames"][order, 0].contiguous(), st["frames"][order, 1]
                of = rec[:, 1].contiguous()
                idx = torch.searchsorted(frame_of, of).clamp_(max=F - 1)
                rec_groups = torch.where(frame_of[idx] == of, mask_of[idx], torch.zeros_like(of)).contiguous()
            else:
                rec_groups = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            if n == 0:
                rec = torch.zeros((1, 4), dtype=torch.int32, device=dev)
            frames = st["frames"] if F else torch.zeros((1, FRAME_ROW), dtype=torch.int32, device=dev)
            masks, bit = (C.c_uint32 * len(self.axes))(), 1
            for s, a in enumerate(self.axes):
                masks[s] = ((1 << len(self.axis_tables[a])) - 1) << bit
                bit += len(self.axis_tables[a])
            out = torch.empty(sum(sizes), dtype=torch.float64, device=dev)
            o = [sum(sizes[:i]) for i in range(len(sizes))]
            lib.call("dpft_dataset_ap_finalize_groups_f64", rec.data_ptr(), rec_groups.data_ptr(), n, start.data_ptr(),
                     frames.data_ptr(), F, masks, len(self.axes), G, Cn, K, self.recall_points, out[o[0]:].data_ptr(),
                     out[o[2]:].data_ptr(), out[o[1]:].data_ptr(), out[o[3]:].data_ptr(), out[o[4]:].data_ptr(), stream())
            if self.tp is not None:      # after the launches above on the same stream: it reads the npos they wrote
                rows = st["tp_errors"][perm].contiguous() if n else torch.zeros((1, 4), dtype=torch.int64, device=dev)
                lib.call("dpft_dataset_ap_finalize_tp_groups_f64", rec.data_ptr(), rows.data_ptr(), rec_groups.data_ptr(), n,
                         start.data_ptr(), out[o[2]:].data_ptr(), G, Cn, self.tp["k"], self.recall_points, self.tp["i_min"],
                         out[o[5]:].data_ptr(), out[o[6]:].data_ptr(), stream())
            # (after the grouped finalize on the same stream, like the TP errors: it reads the npos that one wrote)
            kitti = self._kitti_finalize(rec, n, start, None, rec_groups, out[o[2]:]) if self.kitti else None
            host = out.cpu()
            counters = st["counters"].cpu()
            dropped, saturated = int(counters[DROPPED_NAN]), int(counters[TP_SATURATED])
        ap, tp, npos, nframes, bad = torch.split(host, sizes)[:5]
        res = {"group_ap": ap.reshape(G, Cn - 1, K), "group_tp": tp.reshape(G, Cn - 1, K), "group_npos": npos.reshape(G, Cn - 1),
               "group_nframes": nframes.clone(), "bad": int(bad[0]), "dropped": dropped}
        if self.tp is not None:
            err, points = torch.split(host, sizes)[5:]
            res.update(group_tp_err=err.reshape(G, Cn - 1, 4), group_tp_points=points.reshape(G, Cn - 1), saturated=saturated)
        if kitti is not None:
            res["kitti"] = kitti
        return res

    def scalars(self) -> Dict[str, float]:
        """``compute()`` without the tensors: what the evaluation loops return and log."""
        return {k: v for k, v in self.compute().items() if isinstance(v, float)}

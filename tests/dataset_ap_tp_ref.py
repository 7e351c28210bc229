"""The true-positive errors of the split-level AP (dpft_amd/evaluation/dataset_ap.py, "True-positive errors") restated in Python
fp64 / integers with plain loops.  The greedy walk of the reference combination is walked again here with the target kept (its TP
flags must equal tests/dataset_ap_ref.py's bits: tests/test_dataset_ap_tp_ref.py); the four errors are Python floats from the
fp32 inputs in the operation order of the definition; the stored integers are Python ints (round() is half to even); sums are
Python ints, so exact by construction.
"""
import math
from fractions import Fraction

import numpy as np

from tests import dataset_ap_ref as R

SCALE = 1 << 32                # units per metre (or radian)
LIMIT = float(1 << 20)         # an error of this magnitude, or a non-finite one, saturates
SATURATED = 1 << 52
NAMES = ("ATE", "AZE", "ASE", "AOE")
NAN = float("nan")


def errors(c1, s1, a1, c2, s2, a2, angle_period="2pi"):
    """(ate, aze, ase, aoe) of a detection (1) and a target (2): centre, size, (sin, cos) as fp32 arrays."""
    dx, dy = float(c1[0]) - float(c2[0]), float(c1[1]) - float(c2[1])
    ate = math.sqrt(dx * dx + dy * dy)
    aze = abs(float(c1[2]) - float(c2[2]))
    l1, w1, h1 = (float(v) for v in s1)
    l2, w2, h2 = (float(v) for v in s2)
    p = min(l1, l2) * min(w1, w2) * min(h1, h2)
    v1, v2 = l1 * w1 * h1, l2 * w2 * h2
    ase = 1.0 - p / (v1 + v2 - p)
    r1, r2 = math.hypot(float(a1[0]), float(a1[1])), math.hypot(float(a2[0]), float(a2[1]))
    sn1, cs1, sn2, cs2 = float(a1[0]) / r1, float(a1[1]) / r1, float(a2[0]) / r2, float(a2[1]) / r2
    aoe = math.atan2(abs(sn1 * cs2 - cs1 * sn2), cs1 * cs2 + sn1 * sn2)
    if angle_period == "pi":
        aoe = min(aoe, math.pi - aoe)
    return ate, aze, ase, aoe


def quantise(e):
    """(rint(e * 2^32) half to even, saturated?)."""
    if not abs(e) < LIMIT:                         # (also true for a NaN)
        return SATURATED, True
    return round(e * SCALE), False                 # e * 2^32 is exact: a power of two


def i_min(min_recall, recall_points):
    """max(1, ceil(min_recall * R)) from the decimal form of the number."""
    return max(1, math.ceil(Fraction(repr(float(min_recall))) * recall_points))


def frame_matches(sample, num_classes, kind, thr, min_score, roi):
    """The greedy walk of ONE combination with the target kept: {query: target index} of the frame's TPs."""
    cls = sample["cls"]
    gts = []
    for j in range(sample["gt_class"].shape[0]):
        c = int(np.argmax(sample["gt_class"][j]))
        if c != 0 and R.in_roi(sample["gt_center"][j], roi):
            gts.append((j, c))
    dets = []
    for n in range(cls.shape[0]):
        c = int(np.argmax(cls[n]))
        if c == 0:
            continue
        s = cls[n, c]
        if np.isnan(s) or not (np.float32(s) >= np.float32(min_score)) or not R.in_roi(sample["center"][n], roi):
            continue
        dets.append((n, c, s))
    dets.sort(key=lambda d: (-float(d[2]), d[0]))
    which = R.KINDS.index(kind)
    assigned, taken = set(), {}
    for n, c, _ in dets:
        best, best_j = None, None
        for j, gc in gts:                          # ascending target index: ties go to the lower one
            if gc != c or j in assigned:
                continue
            v = R.iou_pair(sample["center"][n], sample["size"][n], sample["angle"][n],
                           sample["gt_center"][j], sample["gt_size"][j], sample["gt_angle"][j])[which]
            if v > thr and (best is None or v > best):
                best, best_j = v, j
        if best_j is not None:
            assigned.add(best_j)
            taken[n] = best_j
    return taken


def class_errors(flags, rows, npos, recall_points, first_point):
    """One class.  ``flags[p]`` / ``rows[p]`` = TP flag and the four integers of record p in (score desc, frame, query) order.
    Returns ([ate, aze, ase, aoe], served points averaged)."""
    if npos == 0:
        return [NAN] * 4, 0
    table = {}
    t, sums = 0, [0, 0, 0, 0]
    for flag, row in zip(flags, rows):
        if not flag:
            continue
        t += 1
        sums = [a + int(b) for a, b in zip(sums, row)]
        for i in range((t - 1) * recall_points // npos + 1, min(t * recall_points // npos, recall_points) + 1):
            assert i not in table                  # every point has one writer
            table[i] = [float(s) / SCALE / float(t) for s in sums]
    served = [i for i in range(first_point, recall_points + 1) if i in table]
    if not served:
        return [NAN] * 4, 0
    out = []
    for e in range(4):
        total = 0.0
        for i in served:                           # ascending i
            total += table[i][e]
        out.append(total / len(served))
    return out, len(served)


def default_at(kinds, iou):
    return (kinds[0], float(min(iou)))


def run(frames, num_classes, at=None, min_recall=0.1, angle_period="2pi", kinds=R.KINDS, iou=(0.3, 0.5, 0.7), recall_points=40,
        min_score=0.0, roi=R.DEFAULT_ROI):
    """``frames`` = list of (frame index, sample).  Returns ``rows`` (n, 4) int64 in the order of ``dataset_ap_ref.run``'s records
    (class, score desc, frame, query), ``flags`` (n) the TP flags of the reference combination, ``tp_err`` (C-1, 4), ``tp_points``
    (C-1), ``mean`` (4: over the classes that are not NaN), ``saturated``, ``k`` and ``records`` (those of dataset_ap_ref.run)."""
    combos = R.combinations(kinds, iou)
    at = default_at(kinds, iou) if at is None else (at[0], float(at[1]))
    k = combos.index(at)
    recs, npos, saturated = [], [0] * num_classes, 0
    for f, sample in frames:
        r, np_f, _ = R.frame_records(f, sample, num_classes, combos, min_score, roi)
        taken = frame_matches(sample, num_classes, at[0], at[1], min_score, roi)
        npos = [a + b for a, b in zip(npos, np_f)]
        for s, fr, n, c, bits in r:
            row = [0, 0, 0, 0]
            if n in taken:
                j = taken[n]
                e = errors(sample["center"][n], sample["size"][n], sample["angle"][n], sample["gt_center"][j],
                           sample["gt_size"][j], sample["gt_angle"][j], angle_period)
                for x in range(4):
                    row[x], sat = quantise(e[x])
                    saturated += sat
            recs.append((s, fr, n, c, bits, n in taken, row))
    recs.sort(key=lambda r: (r[3], -float(r[0]), r[1], r[2]))
    first = i_min(min_recall, recall_points)
    tp_err, tp_points = np.full((num_classes - 1, 4), np.nan), np.zeros(num_classes - 1)
    for c in range(1, num_classes):
        mine = [r for r in recs if r[3] == c]
        tp_err[c - 1], tp_points[c - 1] = class_errors([r[5] for r in mine], [r[6] for r in mine], npos[c], recall_points, first)
    mean = []
    for e in range(4):
        vals = [v for v in tp_err[:, e] if not math.isnan(v)]
        mean.append(sum(vals) / len(vals) if vals else NAN)
    return {"rows": np.array([r[6] for r in recs], dtype=np.int64).reshape(-1, 4), "flags": np.array([r[5] for r in recs], dtype=bool),
            "bits": np.array([r[4] for r in recs], dtype=np.int64), "classes": np.array([r[3] for r in recs], dtype=np.int64),
            "tp_err": tp_err, "tp_points": tp_points, "mean": mean, "saturated": saturated, "k": k, "i_min": first,
            "npos": np.array(npos[1:], dtype=np.float64)}


def from_rows(classes, flags, rows, npos, recall_points, first_point):
    """tp_err (C-1, 4) and tp_points (C-1) from stored integers in record order: what follows from them by the definition."""
    C = len(npos) + 1
    tp_err, tp_points = np.full((C - 1, 4), np.nan), np.zeros(C - 1)
    for c in range(1, C):
        sel = [p for p in range(len(classes)) if classes[p] == c]
        tp_err[c - 1], tp_points[c - 1] = class_errors([flags[p] for p in sel], [rows[p] for p in sel], int(npos[c - 1]),
                                                       recall_points, first_point)
    return tp_err, tp_points


def saturating_frame():
    """One TP whose centres lie 2 * 10^6 m apart (boxes of 10^7 m: BEV IoU 2 / 3): ate >= 2^20 does not fit; use with roi = None."""
    big = 1.0e7
    return R.hand_sample([(1, 0.9, (0.0, 0.0, 0.0, big, big, 2.0, 0.0, 1.0)), (1, 0.8, R._box(10, 0))],
                         [(1, (2.0e6, 0.0, 0.5, big, big, 2.0, 0.0, 1.0)), (1, R._box(10.2, 0.1))], 2)

"""The definition of the rotated NMS (dpft_amd/evaluation/nms.py) restated in numpy / Python fp64 with plain loops, and the seeded
cases the tests compare the kernels on.  The geometry is dataset_ap_ref's (imported, not copied).

Every case is safe to compare bit for bit: the builder redraws (it never leaves a case out) until, in this reference alone,
 (1) no pairwise IoU of the compared kind lies within MARGIN of ``iou``,
 (2) no two candidate scores of a frame are equal -- except in the tie cases, which use exactly equal scores on purpose.
MARGIN = 1e-8 as in dataset_ap_ref.py and for its reason: both sides are fp64 from the same fp32 inputs and differ only in
operation order, contraction and hypot's last bit, which is < 1e-10 on these magnitudes (sides >= 0.5 m, coordinates < 100 m).

Cost of the restatement.  The greedy pass asks for the IoU of (kept candidate, later candidate) pairs only, and ``pair_iou`` answers
0 without clipping when the fp64 corner bounding boxes of the two footprints are more than GAP = 1e-6 m apart: the clip of two
rectangles that far apart is empty and iou_pair returns exactly 0 (tests/test_nms_ref.py checks the shortcut against iou_pair on
every pair of the small cases).  Condition (1) is checked on ALL pairs that may be compared (same class unless class-agnostic) in
frames of up to ALL_PAIRS_D candidates; in larger frames on the pairs the greedy pass evaluates -- only those decide anything:
a pair whose earlier box is suppressed, or whose later box was suppressed before, has no say in the result.
"""
import functools
import math

import numpy as np

from tests import dataset_ap_ref as G

MARGIN = 1e-8
GAP = 1e-6
ALL_PAIRS_D = 192
KINDS = ("bev", "3d")
KEPT, NO_CANDIDATE, BELOW_MIN_SCORE, BEYOND_MAX_DET = -1, -2, -3, -4
DEFAULTS = dict(iou=0.3, kind="bev", class_agnostic=False, min_score=None, max_det=None)


# ------------------------------------------------------------------------------------------------------ the definition
class _Boxes:
    """The candidates' boxes with their corner bounding boxes (the shortcut of ``pair_iou``)."""

    def __init__(self, center, size, angle, queries):
        self.center, self.size, self.angle = center, size, angle
        self.lo, self.hi = {}, {}
        for n in queries:
            if not (np.all(np.isfinite(center[n])) and np.all(np.isfinite(size[n])) and np.all(np.isfinite(angle[n]))):
                continue                                       # a box that is not finite: IoU 0 with everything
            pts = G.corners(center[n], size[n], angle[n])
            if pts is not None:
                xs, ys = [p[0] for p in pts], [p[1] for p in pts]
                self.lo[n], self.hi[n] = (min(xs), min(ys)), (max(xs), max(ys))

    def apart(self, m, n):
        if m not in self.lo or n not in self.lo:
            return True                                        # an invalid box: IoU 0 with everything
        (ax, ay), (bx, by), (cx, cy), (dx, dy) = self.lo[m], self.hi[m], self.lo[n], self.hi[n]
        return cx - bx > GAP or ax - dx > GAP or cy - by > GAP or ay - dy > GAP

    def pair_iou(self, m, n, which):
        """IoU of ``which`` (0 bev, 1 3d) of the earlier candidate m with the later candidate n."""
        if self.apart(m, n):
            return 0.0
        return G.iou_pair(self.center[m], self.size[m], self.angle[m], self.center[n], self.size[n], self.angle[n])[which]


def nms_frame(frame, iou=0.3, kind="bev", class_agnostic=False, min_score=None, max_det=None, notes=None):
    """One frame: dict of fp32 arrays cls (N,C), center (N,3), size (N,3), angle (N,2).  Returns status (N) int32, order (N) int32,
    count, cls_out (N,C) float32.  ``notes`` (a dict) collects what the builder's conditions need."""
    cls = frame["cls"]
    N = cls.shape[0]
    which = KINDS.index(kind)
    thr = float(iou)
    status = np.full(N, NO_CANDIDATE, dtype=np.int32)
    order = np.full(N, -1, dtype=np.int32)
    cls_out = cls.copy()
    cands = []
    # 1. candidates
    for n in range(N):
        c = int(np.argmax(cls[n]))                              # first maximum; a NaN counts as the maximum
        if c == 0:
            continue
        s = cls[n, c]
        if np.isnan(s):
            continue
        if min_score is not None and not (np.float32(s) >= np.float32(min_score)):
            status[n] = BELOW_MIN_SCORE
            cls_out[n, 0] = s
            continue
        cands.append((n, c, s))
    # 2. order: score descending, query ascending (-0.0 == 0.0 in Python: -0 orders as +0)
    cands.sort(key=lambda d: (-float(d[2]), d[0]))
    boxes = _Boxes(frame["center"], frame["size"], frame["angle"], [n for n, _, _ in cands])
    # 3. greedy pass
    kept = []
    evaluated = {}
    for n, c, s in cands:
        suppressor = None
        for m, cm in kept:
            if not class_agnostic and cm != c:
                continue
            v = boxes.pair_iou(m, n, which)
            evaluated[(m, n)] = v
            if v > thr:
                suppressor = m
                break
        if suppressor is None:
            kept.append((n, c))
        else:
            status[n] = suppressor
            cls_out[n, 0] = s
    # 4. max_det
    count = 0
    for n, c in kept:
        if max_det is not None and count >= max_det:
            status[n] = BEYOND_MAX_DET
            cls_out[n, 0] = cls[n, c]
        else:
            status[n] = KEPT
            order[count] = n
            count += 1
    if notes is not None:
        notes.setdefault("frames", []).append({"cands": cands, "boxes": boxes, "evaluated": evaluated})
    return status, order, count, cls_out


def run(frames, notes=None, **params):
    """``frames``: list of frame dicts of one (N, C).  Returns status (B,N), order (B,N), counts (B), cls_out (B,N,C)."""
    p = dict(DEFAULTS, **params)
    res = [nms_frame(f, notes=notes, **p) for f in frames]
    N, C = (frames[0]["cls"].shape if frames else (0, 2))
    return {"status": np.stack([r[0] for r in res]).reshape(len(frames), N),
            "order": np.stack([r[1] for r in res]).reshape(len(frames), N),
            "counts": np.array([r[2] for r in res], dtype=np.int32),
            "cls_out": np.stack([r[3] for r in res]).reshape(len(frames), N, C)}


def detections(frames, res):
    """Per frame the kept boxes as (count, 10) float32 rows [class, score, x, y, z, l, w, h, sin, cos] in score order."""
    out = []
    for b, f in enumerate(frames):
        rows = []
        for n in res["order"][b, :res["counts"][b]]:
            c = int(np.argmax(f["cls"][n]))
            rows.append(np.concatenate([[np.float32(c), f["cls"][n, c]], f["center"][n], f["size"][n], f["angle"][n]]))
        out.append(np.array(rows, dtype=np.float32).reshape(-1, 10))
    return out


def violations(frames, ties_allowed=False, **params):
    """The builder's two conditions, checked in the reference alone.  Returns a list of strings (empty = safe to compare)."""
    p = dict(DEFAULTS, **params)
    notes = {}
    run(frames, notes=notes, **p)
    which, thr = KINDS.index(p["kind"]), float(p["iou"])
    bad = []
    for b, fr in enumerate(notes["frames"]):
        cands, boxes = fr["cands"], fr["boxes"]
        pairs = dict(fr["evaluated"])
        if len(cands) <= ALL_PAIRS_D:
            for i, (m, cm, _) in enumerate(cands):
                for n, cn, _ in cands[i + 1:]:
                    if (p["class_agnostic"] or cm == cn) and (m, n) not in pairs:
                        pairs[(m, n)] = boxes.pair_iou(m, n, which)
        for (m, n), v in pairs.items():
            if abs(v - thr) <= MARGIN:
                bad.append(f"frame {b}: IoU {v!r} of ({m}, {n}) within the margin of {thr}")
        if not ties_allowed:
            seen = set()
            for n, _, s in cands:
                if float(s) + 0.0 in seen:
                    bad.append(f"frame {b}: score {s!r} twice")
                seen.add(float(s) + 0.0)
    return bad


# ---------------------------------------------------------------------------------------------------------- seeded cases
def _scores(rng, D, lo=0.05, hi=4.0):
    """D distinct fp32 scores in random order."""
    s = np.unique(rng.uniform(lo, hi, 2 * D + 8).astype(np.float32))
    assert s.shape[0] >= D
    return rng.permutation(s)[:D]


def layout_frame(rng, N, D, C, layout):
    """N queries of which exactly D are candidates (at random rows; the rest is background).  layout 'dense': perturbed copies of a
    few prototypes (one cluster per ~24 candidates), so that most candidates overlap several others around the usual thresholds;
    'disjoint': one box per cell of a 3 m grid, sides 0.5 .. 1.2 m -- nothing overlaps."""
    f32 = np.float32
    center = np.stack([rng.uniform(0, 96, N), rng.uniform(-48, 48, N), rng.uniform(-1, 2, N)], -1).astype(f32)
    size = rng.uniform(0.5, 4.5, (N, 3)).astype(f32)
    yaw = rng.uniform(-math.pi, math.pi, N)
    scale = rng.uniform(0.5, 2.0, N)                                   # (sin, cos) need not be normalised
    rows = np.sort(rng.permutation(N)[:D])
    label = np.zeros(N, dtype=np.int64)
    label[rows] = rng.integers(1, C, D)
    if layout == "dense":
        K = D // 24 + 1
        pc = np.stack([rng.uniform(5, 90, K), rng.uniform(-40, 40, K), rng.uniform(-0.5, 1.5, K)], -1)
        ps, py, pl = rng.uniform(1.5, 4.5, (K, 3)), rng.uniform(-math.pi, math.pi, K), rng.integers(1, C, K)
        for n in rows:
            k = int(rng.integers(0, K))
            center[n] = (pc[k] + rng.normal(0, 0.35, 3)).astype(f32)
            size[n] = np.maximum(ps[k] * rng.uniform(0.8, 1.25, 3), 0.5).astype(f32)
            yaw[n] = py[k] + rng.normal(0, 0.08)
            if rng.uniform() < 0.75:
                label[n] = pl[k]
    elif layout == "disjoint":
        cells = rng.permutation(32 * 32)[:D]
        for n, cell in zip(rows, cells):
            center[n, 0], center[n, 1] = f32(1.5 + 3.0 * (cell % 32)), f32(-46.5 + 3.0 * (cell // 32))
            size[n] = rng.uniform(0.5, 1.2, 3).astype(f32)
    else:
        raise ValueError(layout)
    angle = (np.stack([np.sin(yaw), np.cos(yaw)], -1) * scale[:, None]).astype(f32)
    cls = rng.normal(0, 0.5, (N, C)).astype(f32)
    top = np.abs(cls).max(1) + f32(0.02)
    cls[np.arange(N), label] = top                                     # background rows: argmax 0
    if D:
        cls[rows, label[rows]] = (top[rows].max() + _scores(rng, D)).astype(f32)
    return {"cls": cls, "center": center, "size": size, "angle": angle}


def candidates(frame):
    """Number of candidates of a frame without score filter."""
    c = np.argmax(frame["cls"], 1)
    s = frame["cls"][np.arange(c.shape[0]), c]
    return int(np.sum((c != 0) & ~np.isnan(s)))


# name -> (N, D per frame, C, layout, parameters).  D: 0, 1, 2 and both sides of one, two and sixteen blocks of 64; B = 1, 3, 5
# with an all-background frame and a frame of NaN scores only among the others (frame_specials); C = 2, 8, 16; both kinds; both
# class rules; min_score (the median score of frame 0, set by the builder) and max_det.
SHAPES = {}
for _i, _D in enumerate((0, 1, 2, 63, 64, 65, 127, 128, 129, 1024)):
    _N = 1024 if _D == 1024 else _D + 3 + (_i % 2)
    SHAPES[f"dense_d{_D}"] = (_N, [_D], (2, 8, 16)[_i % 3], "dense", dict(kind=KINDS[_i % 2], class_agnostic=bool((_i // 2) % 2)))
    SHAPES[f"disjoint_d{_D}"] = (_N, [_D], (8, 16, 2)[_i % 3], "disjoint", dict(kind=KINDS[(_i + 1) % 2], iou=0.5))
SHAPES.update({
    "b3_c8_bev": (70, [65, 0, 33], 8, "dense", dict(kind="bev")),
    "b3_c8_3d_agnostic": (70, [65, 0, 33], 8, "dense", dict(kind="3d", class_agnostic=True, iou=0.2)),
    "b5_c2_3d": (131, [129, "nan", 64, 0, 1], 2, "dense", dict(kind="3d", iou=0.1)),
    "b5_c16_bev_agnostic": (131, [129, "nan", 64, 0, 1], 16, "dense", dict(class_agnostic=True, iou=0.45)),
    "b1_c8_min_score": (140, [129], 8, "dense", dict(min_score="median")),
    "b3_c8_max_det": (140, [129, 2, 70], 8, "dense", dict(max_det=5)),
    "b3_c16_max_det_large": (140, [129, 2, 70], 16, "dense", dict(max_det=1000, kind="3d")),
    "b1_c8_min_score_max_det": (400, [400], 8, "dense", dict(min_score="median", max_det=64, class_agnostic=True)),
})


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(frames, parameters, reference result) of a SHAPES entry; redrawn until the two conditions hold."""
    N, Ds, C, layout, params = SHAPES[name]
    base = sum(ord(ch) for ch in name)
    for attempt in range(100):
        rng = np.random.default_rng(base + 7919 * attempt)
        frames = []
        for D in Ds:
            if D == "nan":                                             # non-background rows, every score a NaN: no candidate
                f = layout_frame(rng, N, N // 2, C, layout)
                c = np.argmax(f["cls"], 1)
                f["cls"][c != 0, c[c != 0]] = np.float32("nan")
            else:
                f = layout_frame(rng, N, D, C, layout)
            frames.append(f)
        p = dict(params)
        if p.get("min_score") == "median":
            c = np.argmax(frames[0]["cls"], 1)
            s = np.sort(frames[0]["cls"][c != 0, c[c != 0]])
            p["min_score"] = float(s[len(s) // 2])                     # (an existing score: >= keeps it, the next lower one goes)
        if not violations(frames, **p):
            return frames, p, run(frames, **p)
    raise AssertionError(f"{name}: no safe draw in 100 attempts")


# -------------------------------------------------------------------------------------------------------- directed cases
def hand_frame(dets, C, N=None):
    """dets = [(class, score, (cx, cy, cz, l, w, h, sin, cos))]: a logit row is zero but for ``score`` at ``class`` (dataset_ap_ref's
    hand_sample); padded with background rows (score 0.5 at class 0) to N queries."""
    s = G.hand_sample(list(dets) + [(0, 0.5, G._box(0, 0))] * ((N or len(dets)) - len(dets)), [], C)
    return {k: s[k] for k in ("cls", "center", "size", "angle")}


def identical_frame(D, C=3, N=None):
    """D candidates with the same box and class, scores descending with the query index; the rest background."""
    return hand_frame([(1, float(np.float32(2.0 - n / 1024.0)), G._box(10, 1, 0.5, 4, 2, 1.5, 0.6, 0.8)) for n in range(D)], C, N)


def block_frame(N=200, C=3):
    """Sorted position = query index (scores descending).  Query 0 (block 0) covers queries 70 (block 1) and 130 (block 2); query 1
    is covered by query 0 and covers query 80 (block 1), which therefore stays; query 140 is covered by query 70, which is
    suppressed, and by query 5 (kept, block 0).  Everything else is far away on a line."""
    box = {0: G._box(10, 0), 70: G._box(10.5, 0.1), 130: G._box(9.6, -0.1), 1: G._box(11.2, 0), 80: G._box(13.6, 0),
           5: G._box(30, 0), 140: G._box(30.4, 0.1)}
    dets = [(1, float(np.float32(3.0 - n / 128.0)), box.get(n, G._box(0.5 + (n % 20) * 4.9, 6.0 + 3.0 * (n // 20), w=1.0, l=3.0)))
            for n in range(N)]
    return hand_frame(dets, C)


HALF_OUTER, HALF_INNER = (10.0, 0.0, 0.25, 4.0, 2.0, 1.0, 0.0, 1.0), (9.0, 0.0, 0.25, 2.0, 2.0, 1.0, 0.0, 1.0)


def directed_cases():
    """name -> (frames, parameters, ties_allowed, expected status rows or None)."""
    B = G._box
    nan = float("nan")
    s6 = float(np.float32(0.6))
    below = float(np.nextafter(np.float32(s6), np.float32(0)))
    cases = {}
    chain = [(1, 0.9, B(10, 0)), (1, 0.8, B(11, 0)), (1, 0.7, B(12.5, 0))]      # IoU 0.6, 5 / 11, 3 / 13
    cases["chain"] = ([hand_frame(chain, 2)], {}, False, [[-1, 0, -1]])
    two = [(1, 0.9, B(10, 0)), (2, 0.8, B(10.2, 0))]
    cases["two_classes_aware"] = ([hand_frame(two, 3)], {}, False, [[-1, -1]])
    cases["two_classes_agnostic"] = ([hand_frame(two, 3)], dict(class_agnostic=True), False, [[-1, 0]])
    half = [(1, 0.9, HALF_OUTER), (1, 0.8, HALF_INNER)]
    for kind in KINDS:
        cases[f"half_{kind}_at_0.5"] = ([hand_frame(half, 2)], dict(iou=0.5, kind=kind), False, [[-1, -1]])
        cases[f"half_{kind}_at_0.4999"] = ([hand_frame(half, 2)], dict(iou=0.4999, kind=kind), False, [[-1, 0]])
    tie = [(1, 0.5, B(10, 0)), (1, 0.75, B(30, 0)), (1, 0.5, B(10.2, 0.1)), (1, 0.5, B(10.1, 0))]
    cases["equal_scores"] = ([hand_frame(tie, 2), hand_frame(tie[::-1], 2)], {}, True, [[-1, -1, 0, 0], [-1, 0, -1, 0]])
    bad = [(1, 0.9, B(10, 0, s=0.0, c=0.0)), (1, 0.8, B(10, 0, l=0.0)), (1, 0.7, B(10, 0)), (1, 0.6, B(nan, 0)),
           (1, 0.5, B(10, nan)), (1, 0.4, B(10, 0, w=1e-3, h=0.1)), (1, 0.3, B(10.1, 0)), (1, 0.2, B(10, 0, l=nan))]
    cases["invalid_and_nan_boxes"] = ([hand_frame(bad, 2)], {}, False, [[-1, -1, -1, -1, -1, -1, 2, -1]])
    cases["nan_z_3d"] = ([hand_frame([(1, 0.9, B(10, 0, z=nan)), (1, 0.8, B(10, 0)), (1, 0.7, B(10.1, 0))], 2)], dict(kind="3d"), False,
                         [[-1, -1, 1]])      # (not [-1, 0, 0]: a box that is not finite suppresses nothing, whatever the kind)
    cases["nan_z_bev"] = ([hand_frame([(1, 0.9, B(10, 0, z=nan)), (1, 0.8, B(10, 0)), (1, 0.7, B(10.1, 0))], 2)], {}, False,
                          [[-1, -1, 1]])
    nans = [(1, nan, B(10, 0)), (1, 0.8, B(10.1, 0)), (0, nan, B(20, 0)), (2, nan, B(30, 0)), (2, 0.7, B(30, 0))]
    cases["nan_score"] = ([hand_frame(nans, 3)], {}, False, [[-2, -1, -2, -2, -1]])
    ms = [(1, s6, B(10, 0)), (1, below, B(20, 0)), (1, 0.9, B(30, 0)), (1, 0.7, B(10.1, 0)), (1, -1.0, B(40, 0))]
    cases["min_score_equal"] = ([hand_frame(ms, 2)], dict(min_score=s6), False, [[3, -3, -1, -1, -2]])
    cases["min_score_none_negative"] = ([hand_frame([(1, -1.0, B(10, 0)), (1, -2.0, B(10.1, 0))], 2)], {}, False, [[-2, -2]])
    five = [(1, 0.9 - 0.1 * i, B(10 + 8 * i, 0)) for i in range(5)] + [(1, 0.85, B(10.1, 0))]
    cases["max_det_2"] = ([hand_frame(five, 2)], dict(max_det=2), False, [[-1, -1, -4, -4, -4, 0]])
    cases["max_det_equal"] = ([hand_frame(five, 2)], dict(max_det=5), False, [[-1, -1, -1, -1, -1, 0]])
    cases["max_det_larger"] = ([hand_frame(five, 2)], dict(max_det=64), False, [[-1, -1, -1, -1, -1, 0]])
    cases["max_det_1_suppressor_dropped"] = ([hand_frame([(1, 0.9, B(50, 0)), (1, 0.8, B(10, 0)), (1, 0.7, B(10.1, 0))], 2)],
                                             dict(max_det=1), False, [[-1, -4, 1]])
    zero = [(1, -0.0, B(10, 0)), (1, 0.0, B(10.1, 0)), (0, -1.0, B(0, 0)), (1, 0.0, B(30, 0)), (1, -0.0, B(30.1, 0))]
    neg = hand_frame(zero, 2)
    neg["cls"][:, 0] = np.float32(-1.0)                                  # (so that +-0 at class 1 is the maximum)
    neg["cls"][2, 0] = np.float32(0.5)                                   # (but for the background row)
    cases["negative_zero_scores"] = ([neg], {}, True, [[-1, 0, -2, -1, 3]])
    cases["blocks"] = ([block_frame()], {}, False, None)
    cases["identical_65"] = ([identical_frame(65, N=70)], {}, False, [[-1] + [0] * 64 + [-2] * 5])
    cases["identical_1024"] = ([identical_frame(1024)], {}, False, [[-1] + [0] * 1023])
    return cases

"""The KITTI-protocol split AP (dpft_amd/evaluation/dataset_ap.py, "KITTI protocol") restated literally in Python fp64 with plain
loops: pass 1 per frame, the thresholds from all pass-1 TP scores of the split, pass 2 per threshold over every frame again.  The
IoUs are tests/dataset_ap_ref.py's geometry.  ``literal`` uses none of the device path's reductions; ``reduced`` holds the two
one-bit reductions and only the CPU test compares the two.

Safe to compare bit for bit with the device (``violations``): no IoU within MARGIN of a threshold, and no target with two
candidate detections of its class whose IoUs are within MARGIN of each other unless the two boxes are the same bits (then both
sides compute the same number from the same operations and the tie is exact: the tie cases use that on purpose).
"""
import math

import numpy as np

from tests import dataset_ap_ref as R

MARGIN = R.MARGIN
POINTS = 41


# ------------------------------------------------------------------------------------------------------------ the frames
def _far_apart(c1, s1, c2, s2):
    """No overlap in the ground plane whatever the headings: the centres are further apart than the two half diagonals (with
    room to spare).  iou_pair gives exactly (0, 0) for such a pair, and so does the device: the clip is empty."""
    d = math.hypot(float(c1[0]) - float(c2[0]), float(c1[1]) - float(c2[1]))
    return d > 0.5 * (math.hypot(float(s1[0]), float(s1[1])) + math.hypot(float(s2[0]), float(s2[1]))) + 1.0


def prepare(frame_index, sample, num_classes, min_score=0.0, roi=R.DEFAULT_ROI):
    """One frame in the definition's terms: ``dets`` = [(query, class, score)] in file order (ascending query), ``gts`` =
    [(target, class)] in ascending index, ``iou[(query, target)]`` = (bev, 3d) for pairs of one class, ``npos`` per class."""
    cls = sample["cls"]
    gts, npos = [], [0] * num_classes
    for j in range(sample["gt_class"].shape[0]):
        c = int(np.argmax(sample["gt_class"][j]))
        if c != 0 and R.in_roi(sample["gt_center"][j], roi):
            npos[c] += 1
            gts.append((j, c))
    dets, dropped = [], 0
    for n in range(cls.shape[0]):
        c = int(np.argmax(cls[n]))
        if c == 0:
            continue
        s = cls[n, c]
        if np.isnan(s):
            dropped += 1
            continue
        if not (np.float32(s) >= np.float32(min_score)) or not R.in_roi(sample["center"][n], roi):
            continue
        dets.append((n, c, float(s)))
    iou = {}
    for n, c, _ in dets:
        for j, gc in gts:
            if gc != c:
                continue
            if _far_apart(sample["center"][n], sample["size"][n], sample["gt_center"][j], sample["gt_size"][j]):
                iou[(n, j)] = (0.0, 0.0)
            else:
                iou[(n, j)] = R.iou_pair(sample["center"][n], sample["size"][n], sample["angle"][n],
                                         sample["gt_center"][j], sample["gt_size"][j], sample["gt_angle"][j])
    return {"frame": frame_index, "dets": dets, "gts": gts, "iou": iou, "npos": npos, "dropped": dropped, "sample": sample}


# ----------------------------------------------------------------------------------------------------------- the literal form
def pass1(fr, c, which, thr):
    """Queries of the pass-1 TPs of class c: targets in ascending index; each takes, among the unassigned detections of its
    class with IoU > thr and score >= 0 (the tool's pass-1 score threshold 0.0), the highest score, ties to the lower query."""
    dets = [d for d in fr["dets"] if d[1] == c]
    assigned, out = set(), []
    for j, gc in fr["gts"]:
        if gc != c:
            continue
        best, best_s = None, None
        for n, _, s in dets:                         # ascending query: a strict > keeps the lower one on a tie
            if n in assigned or s < 0.0:
                continue
            if fr["iou"][(n, j)][which] > thr and (best is None or s > best_s):
                best, best_s = n, s
        if best is not None:
            assigned.add(best)
            out.append(best)
    return out


def pass2(fr, c, which, thr, s_thr):
    """(TP, FP) of class c at score threshold s_thr: the active detections are those with score >= s_thr; targets in ascending
    index each take, among the active unassigned detections of their class with IoU > thr, the largest IoU, ties to the lower
    query.  FP = active detections that were not taken."""
    dets = [d for d in fr["dets"] if d[1] == c and d[2] >= s_thr]
    assigned = set()
    for j, gc in fr["gts"]:
        if gc != c:
            continue
        best, best_v = None, None
        for n, _, _s in dets:
            if n in assigned:
                continue
            v = fr["iou"][(n, j)][which]
            if v > thr and (best is None or v > best_v):
                best, best_v = n, v
        if best is not None:
            assigned.add(best)
    return len(assigned), len(dets) - len(assigned)


def pick_thresholds(scores, G, notes=None):
    """The tool's sampling loop over the pass-1 TP scores in descending order, operation for operation."""
    out = []
    cur = 0.0
    n1 = len(scores)
    for i in range(n1):
        l = (i + 1) / G
        r = (i + 2) / G if i < n1 - 1 else l
        if notes is not None and i < n1 - 1 and (r - cur) == (cur - l):
            notes["exact"] = notes.get("exact", 0) + 1
        if (r - cur) < (cur - l) and i < n1 - 1:
            continue
        out.append(scores[i])
        cur += 1 / 40.0
    return out


def table(thresholds, tp, fp, G):
    """prec / rec (41, zero-padded), AP (R40) and AP11 from the counts at every threshold."""
    prec, rec = [0.0] * POINTS, [0.0] * POINTS
    for i in range(len(thresholds)):
        prec[i] = tp[i] / (tp[i] + fp[i])
        rec[i] = tp[i] / G
    env = [max(prec[i:]) for i in range(POINTS)]
    ap40 = 0.0
    for i in range(1, 41):
        ap40 += env[i]
    ap11 = 0.0
    for i in range(0, 41, 4):
        ap11 += env[i]
    return prec, rec, ap40 / 40, ap11 / 11


def _pad(v, fill):
    return list(v) + [fill] * (POINTS - len(v))


def _finish(cells, num_classes, K, npos):
    """The arrays the tests compare from cells[(c, k)] = (thresholds, tp, fp)."""
    C = num_classes
    out = {k: np.zeros((C - 1, K, POINTS)) for k in ("prec", "rec", "tp", "fp", "fn")}
    out["thresholds"] = np.full((C - 1, K, POINTS), np.nan)
    out["ap"], out["ap11"] = np.full((C - 1, K), np.nan), np.full((C - 1, K), np.nan)
    out["nthr"] = np.zeros((C - 1, K), dtype=np.int64)
    for c in range(1, C):
        G = npos[c]
        for k in range(K):
            thrs, tp, fp = cells[(c, k)]
            out["nthr"][c - 1, k] = len(thrs)
            out["thresholds"][c - 1, k] = _pad(thrs, float("nan"))
            out["tp"][c - 1, k], out["fp"][c - 1, k] = _pad(tp, 0.0), _pad(fp, 0.0)
            out["fn"][c - 1, k] = _pad([G - t for t in tp], 0.0)
            if G > 0:
                prec, rec, ap40, ap11 = table(thrs, tp, fp, G)
                out["prec"][c - 1, k], out["rec"][c - 1, k], out["ap"][c - 1, k], out["ap11"][c - 1, k] = prec, rec, ap40, ap11
    out["npos"] = np.array(npos[1:], dtype=np.float64)
    m_ap, m_ap11 = [], []
    for k in range(K):
        for name, dst in (("ap", m_ap), ("ap11", m_ap11)):
            vals = [out[name][c - 1, k] for c in range(1, C) if npos[c] > 0]
            dst.append(sum(vals) / len(vals) if vals else float("nan"))
    out["mAP"], out["mAP11"] = m_ap, m_ap11
    return out


def literal(prepared, num_classes, combos, notes=None):
    """The two passes over ``prepared`` (a list of ``prepare`` results).  Returns the table arrays (``_finish``) and
    ``records``: (n, 5) int64 [score bits, frame, query, class, pass-1 bits] ordered by (class, score desc, frame, query), and
    ``tiesums``: {(frame, class, score): [TP of the frame at that score threshold, per combination]} -- the pass-2 counts
    the device's bits must add up to at the end of every score tie group of a frame."""
    C, K = num_classes, len(combos)
    npos = [sum(fr["npos"][c] for fr in prepared) for c in range(C)]
    p1 = {}                                              # (frame, query) -> bits
    cells = {}
    for c in range(1, C):
        for k, (kind, thr) in enumerate(combos):
            which = R.KINDS.index(kind)
            scores = []
            for fr in prepared:
                by_query = {n: s for n, _, s in fr["dets"]}
                for n in pass1(fr, c, which, thr):
                    p1[(fr["frame"], n)] = p1.get((fr["frame"], n), 0) | (1 << k)
                    scores.append(by_query[n])
            scores.sort(reverse=True)
            exact = {}
            thrs = pick_thresholds(scores, npos[c], exact) if npos[c] > 0 else []
            if notes is not None and exact:
                notes.setdefault("exact", {})[(c, k)] = exact["exact"]
            tp, fp = [], []
            for s in thrs:
                t = f = 0
                for fr in prepared:
                    a, b = pass2(fr, c, which, thr, s)
                    t += a
                    f += b
                tp.append(float(t))
                fp.append(float(f))
            cells[(c, k)] = (thrs, tp, fp)
    out = _finish(cells, C, K, npos)
    recs, tiesums = [], {}
    for fr in prepared:
        for n, c, s in fr["dets"]:
            recs.append([s, fr["frame"], n, c, p1.get((fr["frame"], n), 0)])
        for c in range(1, C):
            for s in sorted({d[2] for d in fr["dets"] if d[1] == c}):
                tiesums[(fr["frame"], c, s)] = \
                    [pass2(fr, c, R.KINDS.index(kind), thr, s)[0] for kind, thr in combos]
    recs.sort(key=lambda r: (r[3], -r[0], r[1], r[2]))
    out["records"] = np.array([[R.score_bits(r[0]), r[1], r[2], r[3], r[4]] for r in recs], dtype=np.int64).reshape(-1, 5)
    out["tiesums"] = tiesums
    out["dropped_nan"] = sum(fr["dropped"] for fr in prepared)
    out["combos"] = list(combos)
    return out


def run(frames, num_classes, kinds=R.KINDS, iou=(0.3, 0.5, 0.7), min_score=0.0, roi=R.DEFAULT_ROI, recall_points=40, notes=None):
    """``frames`` = [(frame index, sample)] as tests/dataset_ap_ref.py takes them (``recall_points`` belongs to the other table)."""
    combos = R.combinations(kinds, iou)
    prepared = [prepare(f, s, num_classes, min_score, roi) for f, s in frames]
    out = literal(prepared, num_classes, combos, notes)
    out["prepared"] = prepared
    return out


# ------------------------------------------------------------------------------------------------- the two reductions
def frame_bits(fr, c, which, thr, notes=None):
    """The device path's two bits of one frame, class and combination: {query: (pass-1 bit, pass-2 bit)}.  Detections in
    (score desc, query asc) order.  ``notes['chain']`` = the longest displacement chain (targets taken by one insertion)."""
    dets = sorted((d for d in fr["dets"] if d[1] == c), key=lambda d: (-d[2], d[0]))
    targets = [j for j, gc in fr["gts"] if gc == c]
    bits = {n: [0, 0] for n, _, _ in dets}
    taken = set()
    for j in targets:                                    # pass 1: the first unassigned detection in the order
        for n, _, s in dets:
            if n not in taken and s >= 0.0 and fr["iou"][(n, j)][which] > thr:
                taken.add(n)
                bits[n][0] = 1
                break
    match = {}                                           # pass 2: target -> (query, IoU), maintained under insertion
    for n, _, _s in dets:
        x, start, steps = n, 0, 0
        while True:
            took = None
            for pos in range(start, len(targets)):
                j = targets[pos]
                v = fr["iou"][(x, j)][which]
                if not v > thr:
                    continue
                if j not in match or v > match[j][1] or (v == match[j][1] and x < match[j][0]):
                    took = pos
                    break
            if took is None:
                break
            j = targets[took]
            old = match.get(j)
            match[j] = (x, fr["iou"][(x, j)][which])
            steps += 1
            if notes is not None:
                notes["chain"] = max(notes.get("chain", 0), steps)
            if old is None:
                bits[n][1] = 1
                break
            x, start = old[0], took + 1
    return {n: tuple(b) for n, b in bits.items()}


def reduced(prepared, num_classes, combos):
    """The table from the two bits: two prefix sums over each class's records in (score desc, frame, query) order."""
    C, K = num_classes, len(combos)
    npos = [sum(fr["npos"][c] for fr in prepared) for c in range(C)]
    cells = {}
    for c in range(1, C):
        for k, (kind, thr) in enumerate(combos):
            recs = []
            for fr in prepared:
                bits = frame_bits(fr, c, R.KINDS.index(kind), thr)
                recs += [(s, fr["frame"], n) + bits[n] for n, dc, s in fr["dets"] if dc == c]
            recs.sort(key=lambda r: (-r[0], r[1], r[2]))
            scores = [r[0] for r in recs if r[3]]
            thrs = pick_thresholds(scores, npos[c]) if npos[c] > 0 else []
            tp, fp = [], []
            for s in thrs:
                end = max(p for p, r in enumerate(recs) if r[0] >= s) + 1      # the end of the threshold's tie group
                t = sum(r[4] for r in recs[:end])
                tp.append(float(t))
                fp.append(float(end - t))
            cells[(c, k)] = (thrs, tp, fp)
    return _finish(cells, C, K, npos)


# ---------------------------------------------------------------------------------------------------------------- safety
def violations(prepared, combos):
    """The conditions under which the device's fp64 IoUs decide as this file's do (see the module docstring)."""
    bad = []
    thrs = sorted({t for _, t in combos})
    which = sorted({R.KINDS.index(k) for k, _ in combos})
    for fr in prepared:
        smp = fr["sample"]
        per_target = {}
        for (n, j), v in fr["iou"].items():
            for w in which:
                for t in thrs:
                    if abs(v[w] - t) <= MARGIN:
                        bad.append(f"frame {fr['frame']}: IoU {v[w]!r} of ({n}, {j}) within the margin of threshold {t}")
                if v[w] > thrs[0] - MARGIN:
                    per_target.setdefault((j, w), []).append((v[w], n))
        for (j, w), vals in per_target.items():
            vals.sort()
            for (a, na), (b, nb) in zip(vals, vals[1:]):
                same = all(np.array_equal(smp[key][na], smp[key][nb]) for key in ("center", "size", "angle"))
                if b - a <= MARGIN and not (same and a == b):
                    bad.append(f"frame {fr['frame']}, target {j}: detections {na} / {nb} with IoU {a!r} / {b!r}")
    return bad

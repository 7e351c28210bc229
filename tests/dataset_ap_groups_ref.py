"""The scene-description groups of the split-level AP (dpft_amd/evaluation/dataset_ap.py, "Scene-description groups") restated in
numpy / Python fp64: the frame list is filtered by the definition and tests/dataset_ap_ref.py's ``run`` is applied to every subset
and to nothing else.  The seeded cases are safe to compare bit for bit: ``violations`` of the whole frame list is empty (a subset
of the frames then has none either), and every case is redrawn until it also shows what a grouped scan can get wrong: on each
axis at least three groups with an AP strictly inside (0, 1), at least one NaN entry (npos = 0) and one class with more than 512
records, so that a scan crosses two trip boundaries.
"""
import functools
import math

import numpy as np

from tests import dataset_ap_ref as R

AXES = ("time", "road", "weather")                       # the exporter's order
COLUMN = {"road": 0, "time": 1, "weather": 2}            # description = [road, time, weather]
# value -> folder name, the exporter's defaults (dpft_amd/evaluation/exporters/kradar.py)
DEFAULT_TABLES = {
    "time": {0: "day", 1: "night"},
    "road": {0: "urban", 1: "highway", 2: "alleyway", 3: "suburban", 4: "university", 5: "mountain", 6: "parkinglots",
             7: "shoulder", 8: "countryside"},
    "weather": {0: "normal", 1: "overcast", 2: "fog", 3: "rain", 4: "sleet", 5: "lightsnow", 6: "heavysnow"},
}


def select_axes(groups):
    if groups is True:
        return list(AXES)
    return [a for a in AXES if a in groups]


def group_names(axes, tables=None):
    tables = tables or DEFAULT_TABLES
    return ["all"] + [f"{a}={tables[a][v]}" for a in axes for v in sorted(tables[a])]


def axis_value(description, axis):
    """The integer the exporter would read (int(): towards zero), or None for a non-finite value."""
    v = float(np.asarray(description, dtype=np.float64).reshape(-1)[COLUMN[axis]])
    if not math.isfinite(v):
        return None
    return int(v)


def membership(description, axes, tables=None):
    """(names of the groups the frame belongs to, axes on which its value is bad)."""
    tables = tables or DEFAULT_TABLES
    names, bad = ["all"], []
    for a in axes:
        v = axis_value(description, a)
        if v is None or v not in tables[a]:
            bad.append(a)
        else:
            names.append(f"{a}={tables[a][v]}")
    return names, bad


def run(frames, descriptions, num_classes, groups=True, tables=None, **params):
    """``descriptions[i]`` belongs to ``frames[i]``.  Returns names, ap (G,C-1,K), tp (G,C-1,K), npos (G,C-1), nframes (G), mAP
    (G,K), nrec (G,C-1: records), bad_description (frames with a bad value on at least one selected axis), bad_per_axis {axis:
    [frame positions]}, members {name: [frame positions]} and ``all`` = the whole list's result."""
    axes = select_axes(groups)
    names = group_names(axes, tables)
    members = {n: [] for n in names}
    bad_per_axis = {a: [] for a in axes}
    n_bad = 0
    for i, d in enumerate(descriptions):
        mine, bad = membership(d, axes, tables)
        for n in mine:
            members[n].append(i)
        for a in bad:
            bad_per_axis[a].append(i)
        n_bad += bool(bad)
    res = [R.run([frames[i] for i in members[n]], num_classes, **params) for n in names]
    return {"names": names, "ap": np.stack([r["ap"] for r in res]), "tp": np.stack([r["tp"] for r in res]),
            "npos": np.stack([r["npos"] for r in res]), "nframes": np.array([len(members[n]) for n in names], dtype=np.float64),
            "mAP": np.array([r["mAP"] for r in res], dtype=np.float64), "bad_description": n_bad, "bad_per_axis": bad_per_axis,
            "nrec": np.stack([np.bincount(r["records"][:, 3], minlength=num_classes)[1:] for r in res]),      # (G,C-1) records
            "members": members, "combos": res[0]["combos"], "dropped_nan": res[0]["dropped_nan"], "all": res[0]}


def round_robin(n, offset=0):
    """Descriptions [road, time, weather] that walk every value of every axis: frame i has road (i + offset) % 9, time i % 2,
    weather (i + offset) % 7."""
    return [np.array([(i + offset) % 9, i % 2, (i + offset) % 7], dtype=np.float32) for i in range(n)]


def interior_groups(ref, axis):
    """Number of groups of ``axis`` with at least one AP strictly inside (0, 1)."""
    count = 0
    for g, name in enumerate(ref["names"]):
        if name.startswith(axis + "="):
            ap = ref["ap"][g]
            count += bool(np.any((ap > 0) & (ap < 1)))
    return count


def conditions(frames, descriptions, num_classes, params, ref):
    """What the generator promises, as a list of strings (empty = the case holds); the tests assert it before they touch the GPU."""
    bad = list(R.violations(frames, num_classes, params))
    for a in AXES:
        if interior_groups(ref, a) < min(3, len(DEFAULT_TABLES[a])):
            bad.append(f"axis {a}: fewer than {min(3, len(DEFAULT_TABLES[a]))} groups with an AP inside (0, 1)")
    if not np.isnan(ref["ap"]).any():
        bad.append("no NaN entry")
    per_class = np.bincount(ref["all"]["records"][:, 3], minlength=num_classes)
    if per_class.max() <= 512:
        bad.append(f"largest class has {per_class.max()} records, not more than 512")
    return bad


@functools.lru_cache(maxsize=None)
def stream_case():
    """32 frames of 72 queries (C = 4, K = 6) with round-robin descriptions: twice the frames of tests/dataset_ap_ref.py's
    stream_case, so that one class has more than 512 records.  Returns (frames, descriptions, num_classes, params, reference)."""
    params = dict(R.K6, recall_points=40)
    for attempt in range(100):
        rng = np.random.default_rng(9001 + attempt)
        frames = [(100 + f, R.random_sample(rng, 72, int(rng.integers(0, 9)), 4)) for f in range(32)]
        descriptions = round_robin(len(frames))
        if R.violations(frames, 4, params):
            continue
        ref = run(frames, descriptions, 4, True, **params)
        if not conditions(frames, descriptions, 4, params, ref):
            return frames, descriptions, 4, params, ref
    raise AssertionError("groups stream_case: no safe draw in 100 attempts")


# name -> (queries, targets per frame, C, parameters, groups).  Batches of 1 and 3 frames (a frame index gap splits an update), K = 1
# and 8, C = 2 and 16, R = 2, 40, 101, one axis, two axes and all three.
SHAPES = {
    "n70_c2_k1_r2_weather": (70, [3, 0, 5, 2, 4, 1, 6, 3], 2, dict(R.K1, recall_points=2), ["weather"]),
    "n40_c16_k8_r101_time_road": (40, [9, 12, 0, 7, 10, 8, 11], 16, dict(R.K8, recall_points=101), ["road", "time"]),
    "n65_c4_k6_r40_all": (65, [4, 6, 0, 3, 8, 5, 2, 7, 1, 6, 4, 5], 4, dict(R.K6, recall_points=40), True),
}
# the frames come in runs of consecutive indices: lengths 1 and 3 alternate
_RUNS = (1, 3)


def _frame_indices(n):
    out, f, r = [], 11, 0
    while len(out) < n:
        k = min(_RUNS[r % 2], n - len(out))
        out += list(range(f, f + k))
        f += k + 2
        r += 1
    return out


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(frames, descriptions, num_classes, params, groups, reference) of a SHAPES entry.  The descriptions leave weather = heavysnow
    and road = countryside without a frame (nframes 0, AP NaN), give weather = sleet exactly one frame, and flip time with every
    frame, so that membership changes inside every wave of the scan."""
    N, ms, C, params, groups = SHAPES[name]
    base = sum(ord(ch) for ch in name)
    idx = _frame_indices(len(ms))
    descriptions = []
    for i in range(len(ms)):
        weather = 4 if i == 1 else (0, 1, 2, 3, 5)[i % 5]                  # sleet once, heavysnow never
        descriptions.append(np.array([i % 8, i % 2, weather], dtype=np.float32))
    for attempt in range(100):
        rng = np.random.default_rng(base + 7919 * attempt)
        frames = [(f, R.random_sample(rng, N, m, C)) for f, m in zip(idx, ms)]
        if not R.violations(frames, C, params):
            return frames, descriptions, C, params, groups, run(frames, descriptions, C, groups, **params)
    raise AssertionError(f"{name}: no safe draw in 100 attempts")


def missed_class_case():
    """Three hand-made frames (C = 3).  Frame 0 (fog, the only fog frame) has ground truth of class 2 and no detection of class
    2: AP 0 in ``weather=fog`` although ``all`` has detections of that class from frame 1 (rain).  Frame 2 (rain) has neither
    ground truth nor detections of class 1, and frame 1 none either: class 1 of ``weather=rain`` is NaN."""
    box = R._box
    f0 = R.hand_sample([(1, 0.9, box(10, 0)), (1, 0.4, box(30, 1))], [(1, box(10.2, 0.1)), (2, box(20, 0))], 3)
    f1 = R.hand_sample([(2, 0.8, box(20, 0)), (2, 0.7, box(40, 2))], [(2, box(20.3, 0.1))], 3)
    f2 = R.hand_sample([(2, 0.6, box(15, 0)), (2, 0.3, box(50, -2))], [(2, box(50.2, -2.1)), (2, box(60, 3))], 3)
    frames = [(5, f0), (6, f1), (7, f2)]
    descriptions = [np.array(d, dtype=np.float32) for d in ([0, 0, 2], [1, 1, 3], [1, 0, 3])]
    params = dict(R.K6, recall_points=40)
    return frames, descriptions, 3, params, run(frames, descriptions, 3, True, **params)


def bad_case():
    """The stream case's first 12 frames with bad values: -1, 9 (road), 2 (time), 7 (weather), a NaN, an infinity -- and values
    that int() still maps into the table (-0.5 -> 0, 1.9 -> 1)."""
    frames, _, C, params, _ = stream_case()
    frames = frames[:12]
    nan, inf = float("nan"), float("inf")
    rows = [[0, 0, 0], [-1, 0, 1], [9, 1, 2], [1, 2, 3], [2, 1, 7], [nan, 0, 4], [3, nan, nan], [4, 1, inf], [-0.5, 1.9, 6.999],
            [8, -1, -1], [5, 0, 5], [-inf, 1, 2]]
    descriptions = [np.array(r, dtype=np.float64) for r in rows]
    return frames, descriptions, C, params, run(frames, descriptions, C, True, **params)

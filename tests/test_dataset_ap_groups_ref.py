"""Host side of the scene-description groups of the split-level AP: the reference's own partition properties, the config parsing,
the group names against the exporter's folder names, the argument checks of the two grouped C-ABI entries (all before any launch)
and the rank gather of the frame rows on three gloo ranks.  None of this needs a GPU."""
import copy
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

from tests import dataset_ap_groups_ref as G


def _config(spec, data=None):
    from dpft_amd.configs import load_config
    cfg = copy.deepcopy(load_config("kradar"))
    cfg["evaluate"]["dataset_ap"] = spec
    cfg["data"].update(data or {})
    return cfg


# ------------------------------------------------------------------------------------------------------- the reference
def _partition(ref, n_frames):
    """On every axis, npos and nframes over its groups sum to ``all`` minus the frames with a bad value on that axis."""
    for axis, bad in ref["bad_per_axis"].items():
        mine = [g for g, n in enumerate(ref["names"]) if n.startswith(axis + "=")]
        assert ref["nframes"][mine].sum() == n_frames - len(bad) == ref["nframes"][0] - len(bad), axis
        good = [i for i in range(n_frames) if i not in bad]
        yield axis, mine, good


def test_the_reference_partitions_every_axis():
    from tests import dataset_ap_ref as R
    for frames, descriptions, Cn, params, ref in (G.stream_case()[:5], G.bad_case(), G.missed_class_case()):
        assert ref["names"][0] == "all" and ref["nframes"][0] == len(frames)
        whole = R.run(frames, Cn, **params)
        assert np.array_equal(ref["npos"][0], whole["npos"]) and np.array_equal(ref["tp"][0], whole["tp"])
        assert np.array_equal(ref["ap"][0], whole["ap"], equal_nan=True)
        for axis, mine, good in _partition(ref, len(frames)):
            kept = R.run([frames[i] for i in good], Cn, **params)
            assert np.array_equal(ref["npos"][mine].sum(0), kept["npos"]), axis
            assert np.array_equal(ref["nrec"][mine].sum(0), np.bincount(kept["records"][:, 3], minlength=Cn)[1:]), axis
        # a frame is a member of exactly one group per axis on which its value is good
        for i in range(len(frames)):
            n_in = sum(i in m for m in ref["members"].values())
            assert n_in == 1 + sum(i not in bad for bad in ref["bad_per_axis"].values())


def test_the_generated_cases_hold_what_they_promise():
    frames, descriptions, Cn, params, ref = G.stream_case()
    assert G.conditions(frames, descriptions, Cn, params, ref) == []
    assert len(ref["names"]) == 19 and ref["bad_description"] == 0
    ref = G.bad_case()[4]
    assert ref["bad_description"] == 9 and {a: len(b) for a, b in ref["bad_per_axis"].items()} == {"time": 3, "road": 4, "weather": 4}
    ref = G.missed_class_case()[4]
    fog, rain = ref["names"].index("weather=fog"), ref["names"].index("weather=rain")
    assert ref["nframes"][fog] == 1 and ref["npos"][fog, 1] == 1 and ref["nrec"][fog, 1] == 0 and np.all(ref["ap"][fog, 1] == 0)
    assert ref["npos"][rain, 0] == 0 and np.all(np.isnan(ref["ap"][rain, 0])) and ref["nrec"][0, 1] == 4
    seen = {"empty": 0, "one_frame": 0, "npos0": 0}
    for name in G.SHAPES:
        ref = G.shape_case(name)[5]
        seen["empty"] += int((ref["nframes"] == 0).sum())
        seen["one_frame"] += int((ref["nframes"] == 1).sum())
        seen["npos0"] += int(((ref["npos"] == 0) & (ref["nframes"][:, None] > 0)).sum())
    assert all(seen.values()), seen


# ------------------------------------------------------------------------------------------------------------ the config
def test_from_config_accepts_true_and_lists_of_axes():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    assert DatasetAP.from_config(_config(True)).group_names == []
    assert DatasetAP.from_config(_config({"groups": False})).group_names == []
    ap = DatasetAP.from_config(_config({"groups": True}))
    assert ap.axes == ["time", "road", "weather"] and ap.group_names == G.group_names(G.AXES) and len(ap.group_names) == 19
    ap = DatasetAP.from_config(_config({"groups": ["weather", "time"], "iou": [0.5]}))      # the exporter's order, not the list's
    assert ap.axes == ["time", "weather"] and ap.group_names == G.group_names(["time", "weather"])
    assert DatasetAP.from_config(_config({"groups": ["road"]})).group_names == G.group_names(["road"])
    assert DatasetAP.from_config(_config({"groups": "weather"})).axes == ["weather"]
    # nothing accumulated: NaN tables, no library call; scalars() holds floats only
    res = DatasetAP.from_config(_config({"groups": ["time"], "iou": [0.5], "kinds": ["3d"]})).compute()
    assert res["group_names"] == ["all", "time=day", "time=night"] and res["group_ap"].shape == (3, 1, 1)
    assert res["mAP_3d@0.5/time=night"] != res["mAP_3d@0.5/time=night"] and res["nframes/time=day"] == 0.0
    assert res["bad_description"] == 0.0 and res["npos/1/time=day"] == 0.0
    sc = DatasetAP.from_config(_config({"groups": ["time"], "iou": [0.5], "kinds": ["3d"]})).scalars()
    assert set(sc) == {"AP_3d@0.5/1", "mAP_3d@0.5", "npos/1", "dropped_nan", "bad_description"} | \
        {f"{k}/time={n}" for n in ("day", "night") for k in ("AP_3d@0.5/1", "mAP_3d@0.5", "npos/1", "nframes")}
    assert all(isinstance(v, float) for v in sc.values())


@pytest.mark.parametrize("groups", [[], ["season"], ["time", "time"], "all", 1, {"time": True}, [1], ["weather", "Time"]])
def test_from_config_refuses_other_values_and_names_the_choices(groups):
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    with pytest.raises(ValueError, match=r"'groups' must be true or a non-empty list .*time.*road.*weather"):
        DatasetAP.from_config(_config({"groups": groups}))


def test_group_names_are_the_exporters_folder_names():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    from dpft_amd.evaluation.exporters.kradar import KRadarExporter
    over = {"time_zone": {"dawn": 1, "dusk": 0},
            "road_structures": {f"r{v}": v for v in (3, 1, 4, 15, 9, 2, 6, 5)},
            "weather_conditions": {"clear": 10, "haze": 11, "mist": 12, "drizzle": 13, "hail": 14, "flurry": 15, "blizzard": 16}}
    for data in ({}, over, {"weather_conditions": over["weather_conditions"]}):
        cfg = _config({"groups": True}, data)
        ap, exporter = DatasetAP.from_config(cfg), KRadarExporter.from_config(cfg)
        want = ["all"]
        for axis, table in (("time", exporter._time_zone), ("road", exporter._road_structures), ("weather", exporter._weather_conditions)):
            want += [f"{axis}={table[v]}" for v in sorted(table)]
            # the folder the exporter writes a frame with value v into is the group that holds it
            col = G.COLUMN[axis]
            for v in table:
                d = np.zeros(3)
                d[:] = [sorted(exporter._road_structures)[0], sorted(exporter._time_zone)[0], sorted(exporter._weather_conditions)[0]]
                d[col] = v
                folders = exporter._serialize_description(d)
                assert f"{axis}={folders[G.AXES.index(axis)]}" in ap.group_names
        assert ap.group_names == want
    ap = DatasetAP.from_config(_config({"groups": True}, over))
    assert ap.group_names[:3] == ["all", "time=dusk", "time=dawn"] and ap.group_names[-1] == "weather=blizzard"
    assert ap.axis_tables["road"][-1] == (15, "r15") and len(ap.group_names) == 1 + 2 + 8 + 7
    with pytest.raises(ValueError, match="2 time zones"):                      # the exporter's own refusal
        DatasetAP.from_config(_config({"groups": True}, {"time_zone": {"day": 0}}))
    with pytest.raises(ValueError, match="int32 integers"):
        DatasetAP.from_config(_config({"groups": ["time"]}, {"time_zone": {"day": 0.5, "night": 1}}))


def test_update_names_a_missing_description_before_any_launch():
    from dpft_amd.evaluation.dataset_ap import DatasetAP
    ap = DatasetAP(3, groups=["weather"])
    lab = {"gt_center": torch.zeros(1, 3), "gt_size": torch.ones(1, 3), "gt_angle": torch.zeros(1, 2), "gt_class": torch.zeros(1, 3)}
    with pytest.raises(ValueError, match=r"labels\[1\]\['description'\]"):
        ap._descriptions([dict(lab, description=torch.tensor([0, 1, 2])), lab], torch.device("cpu"))
    with pytest.raises(ValueError, match="road, time, weather"):
        ap._descriptions([dict(lab, description=torch.tensor([0, 1]))], torch.device("cpu"))
    ptrs, types, host, _ = ap._descriptions([dict(lab, description=torch.tensor([3.0, 1.0, float("nan")]))], torch.device("cpu"))
    assert types[0] == 4 and list(host)[:2] == [3.0, 1.0] and host[2] != host[2]


# ------------------------------------------------------------------------------------------------------------ the C ABI
_UPDATE = ("cls", "center", "size", "angle", "gt_box", "gt_id", "counts", "thr", "kinds", "K", "roi", "min_score", "scratch",
           "records", "capacity", "reserved", "counters", "first_frame", "B", "N", "Mmax", "Cn", "desc_ptrs", "desc_types",
           "desc_host", "cols", "cnts", "vals", "n_axes", "frames", "frame_capacity", "frames_before", "stream")


def _update_args(**over):
    """A call of dpft_dataset_ap_update_groups_f32 with valid sizes and dangling (never dereferenced) non-null device pointers."""
    p = C.c_void_p(4096)
    a = dict(cls=p, center=p, size=p, angle=p, gt_box=p, gt_id=p, counts=p, thr=(C.c_double * 8)(*[0.5] * 8),
             kinds=(C.c_int32 * 8)(*[0] * 8), K=1, roi=None, min_score=0.0, scratch=p, records=p, capacity=1 << 20, reserved=0,
             counters=p, first_frame=0, B=2, N=400, Mmax=30, Cn=8, desc_ptrs=(C.c_void_p * 2)(4096, 8192),
             desc_types=(C.c_int32 * 2)(0, 3), desc_host=None, cols=(C.c_int32 * 3)(1, 0, 2), cnts=(C.c_int32 * 3)(2, 9, 7),
             vals=(C.c_int32 * 48)(*range(48)), n_axes=3, frames=p, frame_capacity=16, frames_before=14, stream=None)
    a.update(over)
    return [a[k] for k in _UPDATE]


@pytest.mark.parametrize("over, word", [
    (dict(cls=None), "null"), (dict(records=None), "null"), (dict(desc_ptrs=None), "null"), (dict(desc_types=None), "null"),
    (dict(frames=None), "null"), (dict(cols=None), "null axis tables"), (dict(vals=None), "null axis tables"),
    (dict(N=1025), "sizes out of range"), (dict(K=9), "combinations"), (dict(capacity=799), "record store too small"),
    (dict(B=65, capacity=1 << 20), "at most 64 frames"), (dict(n_axes=4), "0..3 axes"), (dict(n_axes=-1), "0..3 axes"),
    (dict(frames_before=15), "frame store too small"), (dict(frames_before=-1), "frame store too small"),
    (dict(frame_capacity=1), "frame store too small"), (dict(frames=C.c_void_p(4098)), "unaligned"),
    (dict(cols=(C.c_int32 * 3)(1, 3, 2)), "axis 1 needs"), (dict(cnts=(C.c_int32 * 3)(2, 0, 7)), "axis 1 needs"),
    (dict(cnts=(C.c_int32 * 3)(2, 17, 7)), "axis 1 needs"), (dict(cnts=(C.c_int32 * 3)(16, 16, 7)), "at most 32"),
    (dict(desc_types=(C.c_int32 * 2)(0, 5)), "description type 5 of sample 1"),
    (dict(desc_types=(C.c_int32 * 2)(4, 0)), "desc_host is null"),
    (dict(desc_ptrs=(C.c_void_p * 2)(4096, None)), "sample 1 is null or unaligned"),
    (dict(desc_ptrs=(C.c_void_p * 2)(4096, 8196)), "sample 1 is null or unaligned"),       # int64 needs 8 bytes
    (dict(desc_ptrs=(C.c_void_p * 2)(4098, 8192)), "sample 0 is null or unaligned"),
])
def test_update_groups_entry_refuses_before_any_launch(over, word):
    from dpft_amd.hip.lib import lib
    rc = lib.load().dpft_dataset_ap_update_groups_f32(*_update_args(**over))
    assert rc == -1 and word in lib.dpft_last_error().decode(), lib.dpft_last_error().decode()


def test_finalize_groups_entry_refuses_before_any_launch():
    from dpft_amd.hip.lib import lib
    dll, p = lib.load(), C.c_void_p(4096)
    good = dict(rec=p, rec_groups=p, n=10, start=p, frames=p, F=3, masks=(C.c_uint32 * 3)(6, 0xFF8, 0x7F000), n_axes=3, G=19, Cn=8,
                K=6, R=40, ap=p, npos=p, tp=p, nframes=p, bad=p, stream=None)
    order = ("rec", "rec_groups", "n", "start", "frames", "F", "masks", "n_axes", "G", "Cn", "K", "R", "ap", "npos", "tp", "nframes",
             "bad", "stream")
    for over, word in [(dict(rec=None), "null"), (dict(rec_groups=None), "null"), (dict(start=None), "null"), (dict(frames=None), "null"),
                       (dict(ap=None), "null"), (dict(npos=None), "null"), (dict(tp=None), "null"), (dict(nframes=None), "null"),
                       (dict(bad=None), "null"), (dict(R=1), "sizes out of range"), (dict(R=102), "sizes out of range"),
                       (dict(K=0), "sizes out of range"), (dict(K=9), "sizes out of range"), (dict(Cn=17), "sizes out of range"),
                       (dict(Cn=1), "sizes out of range"), (dict(n=-1), "sizes out of range"), (dict(F=-1), "sizes out of range"),
                       (dict(G=0), "groups and"), (dict(G=33), "groups and"), (dict(n_axes=4), "groups and"),
                       (dict(masks=None), "groups and")]:
        a = dict(good, **over)
        rc = dll.dpft_dataset_ap_finalize_groups_f64(*[a[k] for k in order])
        assert rc == -1 and word in lib.dpft_last_error().decode(), (over, lib.dpft_last_error().decode())


# ------------------------------------------------------------------------------------------------------------- the ranks
def _gather_worker(rank, world, port, q):
    import torch.distributed as dist
    from dpft_amd.evaluation.dataset_ap import gather_state
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, f = (5, 0, 3)[rank], (2, 0, 4)[rank]                   # unequal counts, one rank without records and frames
    records = torch.arange(n * 4, dtype=torch.int32).reshape(n, 4) + 1000 * rank
    frames = torch.arange(f * 18, dtype=torch.int32).reshape(f, 18) + 100000 * rank
    counters = torch.zeros(32, dtype=torch.int64)
    counters[0], counters[1], counters[16 + 1] = n, rank, 10 * rank + 1
    out = gather_state({"records": records, "counters": counters, "frames": frames})
    plain = gather_state({"records": records, "counters": counters})
    q.put((rank, out["records"].numpy(), out["counters"].numpy(), out["frames"].numpy(), sorted(plain)))
    dist.destroy_process_group()


def test_gather_state_carries_the_frame_rows_of_every_rank():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_rec = np.concatenate([np.arange(20).reshape(5, 4), np.arange(12).reshape(3, 4) + 2000]).astype(np.int32)
    want_frames = np.concatenate([np.arange(36).reshape(2, 18), np.arange(72).reshape(4, 18) + 200000]).astype(np.int32)
    for r in range(world):
        rec, cnt, frames, plain_keys = res[r]
        assert np.array_equal(rec, want_rec) and np.array_equal(frames, want_frames)
        assert cnt[0] == 8 and cnt[1] == 3 and cnt[17] == 33
        assert plain_keys == ["counters", "records"]            # a state without frames gathers without them

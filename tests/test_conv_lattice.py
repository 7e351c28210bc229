"""The geometry lattice of the convolution tests (tests/conv_lattice.py), checked without a GPU: it covers what it claims to
cover, its integer operands make every summation order exact, its fp64 reference equals the definition written as plain loops,
and the library's sizing / tiling answers hold for every case.  The GPU half is tests/test_gpu_conv_geometry.py."""
import collections
import ctypes as C

import pytest
import torch

from tests import conv_lattice as L


def test_lattice_is_deterministic_and_covers_every_axis_value_in_every_class():
    again = L.build_lattice()
    assert again == L.LATTICE
    per_class = collections.Counter(c.cls for c in L.LATTICE)
    print("lattice:", len(L.LATTICE), "cases;", dict(per_class))
    assert set(per_class) == set(L.CLASSES)
    for c in L.LATTICE:
        assert c.cls == L.dispatch_class(*c[1:10]), c
    for cls in L.CLASSES:
        want = {(a, v) for a, vs in L.class_axes(cls).items() for v in vs}
        got = set()
        for c in L.LATTICE:
            if c.cls == cls:
                got |= L.case_tags(c)
        assert not (want - got), (cls, sorted(map(str, want - got)))
    # the issue's axis lists themselves
    assert sorted({c.C for c in L.LATTICE}) == sorted(L.C_VALUES) and {c.K for c in L.LATTICE} >= set(L.K_VALUES)
    assert {(c.kh, c.kw) for c in L.LATTICE} == set(L.FILTERS) and {c.stride for c in L.LATTICE} == set(L.STRIDES)
    assert {L.rows(c) for c in L.LATTICE} >= set(L.M_TARGETS)
    # only the named exceptions are larger than the size limit
    for c in L.LATTICE:
        assert c.B * c.H * c.W * c.C <= L.ELEMS_MAX or c.name in L.LARGE_NAMES, c


def test_named_corners_are_present():
    names = {c.name for c in L.LATTICE}
    assert {t[0] for t in L.CORNERS + L.BIG} <= names
    has = lambda f: any(f(c) for c in L.LATTICE)
    v = lambda c: c.C % 64 == 0
    assert has(lambda c: v(c) and c.kh != c.kw and c.H != c.W)                                     # rows / columns
    assert has(lambda c: v(c) and (c.kh, c.kw, c.pad) == (3, 3, 0))                                  # pad 0, 3x3
    assert has(lambda c: v(c) and c.pad >= max(c.kh, c.kw) and c.kh > 1)                             # outputs that see padding only
    assert has(lambda c: v(c) and c.K % 64 == 0 and c.stride > 1 and (c.H + 2 * c.pad - c.kh) % c.stride)      # leftover row
    assert has(lambda c: v(c) and c.K % 64 == 0 and c.stride == 3 and c.H < 3)                       # classes with ph >= H
    assert has(lambda c: v(c) and c.stride > max(c.kh, c.kw))                                        # stride above the filter
    assert has(lambda c: c.C % 64 == 32 and c.K % 4 == 0)
    for k in (1, 3, 5, 66, 68, 100, 132):
        assert has(lambda c: v(c) and c.K == k), k
    for ch in (1, 4, 5):
        assert has(lambda c: c.C == ch and c.K % 4 == 0), ch
    assert has(lambda c: c.H == 1 and c.W == 1) and has(lambda c: v(c) and c.H < c.kh) and has(lambda c: v(c) and L.rows(c) == 1)
    for m in L.M_TARGETS:
        assert has(lambda c: v(c) and L.rows(c) == m), m
    # the two >= 2 GFLOP cases with a non-square filter; one with K, C >= 128 (weight gradient on the split kernels)
    big = [L.by_name(t[0]) for t in L.BIG]
    for c in big:
        oh, ow = L.out_size(c)
        assert c.kh != c.kw and 2.0 * c.B * oh * ow * c.K * c.kh * c.kw * c.C >= 2e9
        assert all(L.expected_family(c, kind, "fp32+split") == "x3" for kind in ("fwd", "dgrad"))
    assert any(L.expected_family(c, "wgrad", "bf16x3") == "x3" for c in big)
    assert any(L.is_conv16(c) for c in L.LATTICE) and any(L.is_stem7(c) for c in L.LATTICE)
    assert sum(L.is_thin1x1(c) for c in L.LATTICE) >= 3
    # parity-class data gradients with a workspace: enough workgroups per class
    assert sum(c.stride > 1 and L.expected_family(c, "dgrad", "bf16x3", tile=(64, 64, 1)) == "x3" for c in L.LATTICE) >= 4


def test_exactness_conditions_hold_for_every_case():
    for c in L.LATTICE:
        assert L.check_exactness(c)
        assert c.kh * c.kw * c.C * 64 < 2 ** 24 and L.rows(c) * 64 < 2 ** 24, c
        if c.B * c.H * c.W * c.C > 4 * L.ELEMS_MAX:
            continue
        o = L.operands(c)                      # asserts that every operand (and the prologue's output) is exact in bf16
        for k in ("x", "w", "dy", "bias", "base", "res"):
            assert float(o[k].abs().max()) <= L.VMAX and torch.equal(o[k], o[k].round()), (c.name, k)
        assert set(o["pro"][1].tolist()) <= {0.5, 1.0, 2.0} and set(o["obn"][1].tolist()) <= {0.5, 1.0, 2.0}
    c = L.by_name("c64-k66")
    o = L.operands(c)
    ref = L.reference(c, o)
    for k, v in ref.items():                   # the fp64 results are fp32 values
        assert torch.equal(v.float().double(), v), k
    # fp32 CPU arithmetic in another summation order gives the same bits: the exactness claim, demonstrated
    y32 = torch.einsum("bhwrsc,krsc->bhwk", torch.nn.functional.pad(o["x"], (0, 0, 1, 1, 1, 1)).unfold(1, 3, 1).unfold(2, 3, 1)
                       .permute(0, 1, 2, 4, 5, 3), o["w"])
    assert torch.equal(y32.double(), ref["y"])


def _loop_subset():
    """Small cases with a non-square filter, pad >= filter, stride 3 and a leftover row among them."""
    small = [c for c in L.LATTICE if L.rows(c) * c.kh * c.kw * c.B <= 6000 and c.B * c.H * c.W * c.C <= 40000]
    feats = {"nonsquare": lambda c: c.kh != c.kw, "over": lambda c: c.pad >= max(c.kh, c.kw) and c.kh * c.kw > 1,
             "s3": lambda c: c.stride == 3, "leftover": lambda c: (c.H + 2 * c.pad - c.kh) % c.stride != 0,
             "all": lambda c: c.kh != c.kw and c.stride == 3 and (c.H + 2 * c.pad - c.kh) % 3 != 0}
    out = []
    for name, f in feats.items():
        hit = [c for c in small if f(c)]
        assert len(hit) >= 2, name
        out += hit[:4]
    return sorted(set(out))


@pytest.mark.parametrize("case", _loop_subset(), ids=lambda c: c.name)
def test_fp64_reference_equals_the_six_loop_definition(case):
    o = L.operands(case)
    ref, loops = L.reference(case, o), L.six_loops(case, o)
    for k in ("y", "dx", "dw"):
        assert torch.equal(ref[k], loops[k]), (case, k)
    # the mask of unreached input pixels agrees with the definition: no tap -> zero gradient, whatever dy and w are
    mask = L.unreached_mask(case)
    assert bool((loops["dx"][:, mask] == 0).all())
    ones = {**o, "dy": torch.ones_like(o["dy"]), "w": torch.ones_like(o["w"])}
    assert torch.equal(L.six_loops(case, ones)["dx"][0, :, :, 0] == 0, mask)


def test_unreached_mask_on_known_geometries():
    c = L.by_name("leftover-2x2-c64-s3")       # H 10, W 9, 2x2, stride 3, pad 0: rows 2, 5, 8, 9 and columns 2, 5, 8
    m = L.unreached_mask(c)
    rows_, cols_ = {2, 5, 8, 9}, {2, 5, 8}
    for i in range(c.H):
        for j in range(c.W):
            assert bool(m[i, j]) == (i in rows_ or j in cols_)
    assert bool(L.unreached_mask(L.by_name("s3-H1-c64-1x1-p1")).all())
    assert not bool(L.unreached_mask(L.by_name("pad3-3x3-c64")).any())


def test_refused_geometries_are_refused_through_the_cabi():
    """What the lattice marks as refused is refused with DPFT_ERR_ARG and that message, before anything is launched (no GPU is
    touched; the pointers are never read) -- and nothing else is marked: K % 4 != 0 at the inference epilogue and at the
    weight gradient's operand prologue.
    tests/test_host.py::test_cabi_argument_errors_are_reported holds the same assertion next to the other argument errors."""
    from dpft_amd.hip.lib import lib, make_desc
    x, w, y, bnp, res, ws = (C.c_void_p(256 * (i + 1)) for i in range(6))
    marked = [c for c in L.LATTICE if L.refusal(c, L.BNACT)]
    assert marked and all(c.K % 4 for c in marked) and len(marked) == sum(c.K % 4 != 0 for c in L.LATTICE)
    for c in marked:
        d = make_desc(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)
        rc = lib.dpft_conv2d_nhwc_fwd_bnact_f32(C.byref(d), x, w, bnp, 1, res, y, ws, None)
        assert rc == -1 and L.refusal(c, L.BNACT).encode() in lib.dpft_last_error(), (c, lib.dpft_last_error())
    # the weight gradient's operand prologue: the tests run it where C % 64 == 0, refused there for K % 4 != 0
    marked = [c for c in L.LATTICE if c.C % 64 == 0 and L.refusal(c, L.WGRAD_PRO)]
    assert marked and len(marked) == sum(c.C % 64 == 0 and c.K % 4 != 0 for c in L.LATTICE)
    for c in marked:
        d = make_desc(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)
        rc = lib.dpft_conv2d_nhwc_wgrad_f32(C.byref(d), x, res, bnp, 1, y, ws, None)
        assert rc == -1 and L.refusal(c, L.WGRAD_PRO).encode() in lib.dpft_last_error(), (c, lib.dpft_last_error())
    assert not any(L.refusal(c, "dpft_conv2d_nhwc_fwd_f32") for c in L.LATTICE)


FAMILY = {0: "f32", 1: "x3", 2: "bf16", 3: "vector"}      # dpft_profile_get_family's numbering
KINDS = {"fwd": 0, "dgrad": 1, "wgrad": 2}
COMPUTE = {"fp32": 0, "bf16": 1, "bf16x3": 2}


def _planned(lib, c, kind, workspace=True):
    from dpft_amd.hip.lib import make_desc
    d = make_desc(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)
    fam = int(lib.dpft_conv2d_planned_family(C.byref(d), KINDS[kind], int(workspace)))
    assert fam in FAMILY, (c, kind, fam)
    return FAMILY[fam]


@pytest.fixture
def plan_mode():
    """Sets the compute mode and the split switch as the GPU tests' compute_mode() does; puts both back."""
    from dpft_amd.hip.lib import lib
    was = int(lib.dpft_conv_get_compute()), int(lib.dpft_conv_get_split())

    def set_mode(name):
        compute, split = L.MODES[name]
        assert lib.dpft_conv_set_compute(COMPUTE[compute]) == 0 and lib.dpft_conv_set_split(int(split)) == 0
        return lib
    yield set_mode
    lib.dpft_conv_set_compute(was[0])
    lib.dpft_conv_set_split(was[1])


@pytest.mark.parametrize("mode", list(L.MODES))
def test_planned_family_is_the_expected_family_on_the_lattice(mode, plan_mode):
    """What the launch plan names (dpft_conv2d_planned_family, host only) equals conv_lattice.expected_family for every case,
    kind and mode -- tests/test_gpu_conv_geometry.py asserts the same restatement against what RAN, so the plan is what runs."""
    lib = plan_mode(mode)
    bad = []
    for c in L.LATTICE:
        for kind in KINDS:
            got, want = _planned(lib, c, kind), L.expected_family(c, kind, mode)
            if got != want:
                bad.append((c.name, kind, got, want))
        if c.stride > 1 and c.K % 64 == 0 and c.C > 4:      # run_case: the strided data gradient without a workspace
            got, want = _planned(lib, c, "dgrad", workspace=False), L.expected_family(c, "dgrad", mode, workspace=False)
            if got != want:
                bad.append((c.name, "dgrad, no workspace", got, want))
    assert lib.dpft_conv2d_planned_family(None, 0, 1) == -1
    assert not bad, (mode, bad)


def test_planned_family_under_forced_tiles(plan_mode, monkeypatch):
    """Every entry of FORCE_TILES / FORCE_WGRADS on the case lists and modes of the GPU tests that force them."""
    C64, FORCE_TILES, FORCE_WGRADS, WVEC = L.C64, L.FORCE_TILES, L.FORCE_WGRADS, L.WVEC
    bad = []
    for tile in FORCE_TILES:
        monkeypatch.setenv("DPFT_FORCE_TILE", tile)
        t = tuple(int(v) for v in tile.split(","))
        for mode in ("fp32", "bf16x3", "bf16"):
            lib = plan_mode(mode)
            for c in C64:
                for kind in ("fwd", "dgrad"):
                    got, want = _planned(lib, c, kind), L.expected_family(c, kind, mode, t)
                    if got != want:
                        bad.append((tile, mode, c.name, kind, got, want))
                if c.stride > 1 and c.K % 64 == 0:
                    got, want = _planned(lib, c, "dgrad", workspace=False), L.expected_family(c, "dgrad", mode, t, workspace=False)
                    if got != want:
                        bad.append((tile, mode, c.name, "dgrad, no workspace", got, want))
    monkeypatch.delenv("DPFT_FORCE_TILE")
    for wtile in FORCE_WGRADS:
        monkeypatch.setenv("DPFT_FORCE_WGRAD", wtile)
        wt = tuple(int(v) for v in wtile.split(","))
        for mode in ("fp32", "bf16"):
            lib = plan_mode(mode)
            for c in WVEC:
                got, want = _planned(lib, c, "wgrad"), L.expected_family(c, "wgrad", mode, wtile=wt)
                if got != want:
                    bad.append((wtile, mode, c.name, "wgrad", got, want))
    assert not bad, bad


@pytest.mark.parametrize("split", [0, 1])
def test_sizing_and_tiling_answers_for_every_case(split):
    from dpft_amd.hip.lib import lib, make_desc
    was = int(lib.dpft_conv_get_split())
    try:
        assert lib.dpft_conv_set_split(split) == 0
        for c in L.LATTICE:
            d = make_desc(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)
            assert (d.OH, d.OW) == L.out_size(c)
            assert int(lib.dpft_conv2d_workspace_bytes(C.byref(d))) >= int(lib.dpft_conv2d_workspace_header_bytes()) > 0, c
            tr = C.c_int32(0)
            tiles = int(lib.dpft_conv2d_stats_tiles(C.byref(d), C.byref(tr)))
            assert tiles >= 1 and tr.value >= 1 and tr.value * tiles >= L.rows(c) > tr.value * (tiles - 1), (c, tiles, tr.value)
    finally:
        lib.dpft_conv_set_split(was)

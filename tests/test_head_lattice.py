"""The lattice of the training decoder's reduction + head + reference points (tests/head_lattice.py), checked without a GPU: the
table reaches every size, form and reference-point row it names; its seeded inputs make the comparison mean something (no ReLU
input at zero, no stray point at a clip edge, every row in the class its name claims, nothing exempt); the closed form of the
reference-point gradient equals the oracle's fp64 autograd wherever that is finite and the elevation is below 85 degrees; and the
float32 yardsticks (the oracle in fp32; the closed form in fp32 on the steep and the axis rows) stay well inside the rule, so
that a failure on the GPU is the kernel's.  The GPU half is tests/test_gpu_head_lattice.py."""
import pytest
import torch

from tests import head_lattice as L


def _eq(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_lattice_is_deterministic_and_reaches_every_axis_value():
    print("\n".join(L.table_rows()))
    assert len({c.name for c in L.CASES}) == len(L.CASES)
    for c in L.CASES:
        a, b = L.make_inputs(c), L.make_inputs(c)
        assert all(_eq(a[k], b[k]) for k in a), c.name
        assert c.B * c.Q <= 64 and len(c.p_rows) == L.n_views(c) and len(c.rows) <= c.Q, c.name
    V, BQ = L.n_views, (lambda c: c.B * c.Q)
    assert {V(c) for c in L.CASES} == {1, 2, 3, 4}
    assert {c.ncls for c in L.CASES} >= {1, 2, 15, 16}
    assert {BQ(c) for c in L.CASES} >= {1, 3, 4, 5, 63, 64} and {BQ(c) % 4 for c in L.CASES} == {0, 1, 2, 3}
    assert {p for c in L.CASES for p in c.p_rows} == {3, 4}
    assert {c.shapes for c in L.CASES} == {"i64s2", "i64s3", "i32", "mixed"}
    flags = [L.flags_of(c) for c in L.CASES]
    assert any(not any(f) for f in flags) and any(all(f) for f in flags) and any(any(f) and not all(f) for f in flags)
    # V = 4 with 16 classes and B >= 2; batch indexing wherever rows are placed
    big = L.by_name("v4-c16")
    assert V(big) == 4 and big.ncls == 16 and big.B >= 2
    assert all(c.B >= 2 for c in L.CASES if c.name in ("generic-v3", "v4-c16", "edges", "poles", "el-85", "el-89.9"))
    # every (batch element, view) its own T, P and (H, W), H != W
    for c in L.CASES:
        inp = L.make_inputs(c)
        keys = set()
        for v in range(V(c)):
            for b in range(c.B):
                H, W = inp["hw"][v][b].tolist()
                assert H != W
                keys.add((H, W))
                assert sum(torch.equal(inp["P"][v][b], inp["P"][w][d]) for w in range(V(c)) for d in range(c.B)) == 1, c.name
                if inp["flags"][v]:
                    assert sum(torch.equal(inp["T"][v][b], inp["T"][w][d]) for w in range(V(c)) for d in range(c.B)) == 1, c.name
        assert len(keys) == V(c) * c.B, c.name
    # the reference-point rows
    classes = {cls for c in L.CASES for cls, _ in c.rows}
    assert classes >= {"u-below", "u-above", "v-below", "v-above", "u0", "u1", "v0", "v1", "wzero", "r0", "axis-up", "axis-down",
                       "negx0", "negx+", "negx-"} | {f"el{e:g}" for e in L.STEEP}
    assert any(len(c.rows) < c.Q for c in L.CASES)                      # "inside" rows
    # the exact points need center == prev_center bit for bit
    assert all(c.exact for c in L.CASES if any(cls in L.EXACT_CLASSES or L.steep_of(cls) for cls, _ in c.rows))


def test_proj_takes_the_form_the_case_names():
    """Stride 2 and 3 int64 rows are read in place; int32 rows and mixed strides take _Proj's compaction branch."""
    from dpft_amd.models.fusers import train_fused as tf
    for c in L.CASES:
        inp = L.make_inputs(c)
        proj = tf._Proj(list(zip(inp["T"], inp["P"])), inp["shape"], inp["flags"])
        in_place = all(a.data_ptr() == b.data_ptr() for a, b in zip(proj.shape, inp["shape"]))
        assert in_place == (c.shapes in ("i64s2", "i64s3")), c.name
        assert proj.shape_stride == (3 if c.shapes == "i64s3" else 2), c.name
        assert all(s.dtype == torch.int64 and torch.equal(s[:, :2], hw) for s, hw in zip(proj.shape, inp["hw"])), c.name
        assert [p.shape[1] for p in proj.P] == list(c.p_rows) and proj.flags == list(L.flags_of(c)), c.name


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_inputs_make_the_comparison_mean_something(c):
    fig = L.check_inputs(c)
    print(c.name, fig)
    assert fig["exempt_rows"] == 0
    assert sum(fig["rows"].values()) == c.B * c.Q
    for cls, _ in c.rows:
        assert fig["rows"][cls] == c.B * sum(1 for k, _ in c.rows if k == cls), (c.name, cls)
    assert L.find_seed(c) == c.seed, (c.name, "the committed seed is the first that meets the conditions")


def _max_elevation(c, inp):
    """(B,Q): the largest |elevation| over the flagged views (0 without one); and whether a flagged view has rho == 0."""
    center = L.cached(c)["out64"][1]
    el, axis = torch.zeros(c.B, c.Q, dtype=torch.float64), torch.zeros(c.B, c.Q, dtype=torch.bool)
    for v, f in enumerate(inp["flags"]):
        if f:
            m = L.geometry(center, inp["T"][v].double(), inp["P"][v].double(), inp["hw"][v], 1)
            el, axis = torch.maximum(el, m["el"].abs()), axis | (m["rho"] == 0)
    return el, axis


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_closed_form_equals_oracle_autograd(c):
    """fp64: on every row where autograd is finite and the elevation is below 85 degrees the closed form is the oracle's autograd
    to rounding (the origin rows, r == 0, among them); autograd is not finite on the axis rows and only there; on the steep rows the two still agree to 1e-6 of the
    row (fp64 has the digits that fp32 lacks), which ties the closed form to the oracle there as well."""
    inp = L.cached(c)["inp"]
    ref = L.reference(c, inp)                                           # plain autograd, nothing replaced
    ga, gc = ref["g_auto"], ref["g_closed"]
    assert torch.isfinite(gc).all()
    el, axis = _max_elevation(c, inp)
    finite = torch.isfinite(ga).all(-1)
    # not finite on the axis rows and nowhere else; at the origin (r == 0) autograd is finite -- zeros, the closed form's too
    assert not (~finite & ~axis).any(), (c.name, (~finite).nonzero().tolist(), axis.nonzero().tolist())
    for b, q, cls, _ in L.row_classes(c):
        assert bool(finite[b, q]) == (cls not in ("axis-up", "axis-down")), (c.name, b, q, cls)
    assert torch.equal(L.closed_rows(c, inp), axis | (el >= L.CLOSED_FROM))
    scale = gc.abs().amax(-1, keepdim=True).clamp_min(1e-300)
    err = ((ga - gc).abs() / scale).amax(-1)
    low = finite & (el < L.AUTOGRAD_BELOW)
    assert int(low.sum()) + int((~low).sum()) == c.B * c.Q
    if low.any():
        assert float(err[low].max()) <= 1e-11, (c.name, float(err[low].max()))
    rest = finite & ~low
    if rest.any():
        print(c.name, "rows at 85 degrees or more: closed form vs fp64 autograd", float(err[rest].max()))
        assert float(err[rest].max()) <= 1e-6, (c.name, float(err[rest].max()))
    # the convention: a view adds nothing at its origin, and only the range term on its axis
    for b, q, cls, v in L.row_classes(c):
        if cls == "r0":
            one = L.ref_points_grad_closed(L.cached(c)["out64"][1], inp["T"][v].double(), inp["P"][v].double(), inp["hw"][v], 1,
                                           inp["gys"][5][v].double())
            assert not one[b, q].any(), (c.name, b, q)


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_fp32_yardstick_is_within_a_quarter_of_the_tolerance(c):
    """The oracle evaluated in fp32 (the closed form in fp32 on the rows at 89 degrees or more and on the axis) against fp64, as a
    fraction of the rule, for every output and every gradient: at most a quarter."""
    ref64, ref32 = L.cached_reference(c), L.cached_reference(c, torch.float32)
    assert all(torch.isfinite(t).all() for t in ref64["outs"] + ref64["grads"])
    d = {n: L.distance(a, b) for n, a, b in zip(L.OUT_NAMES, ref32["outs"], ref64["outs"])}
    d.update({"d " + n: L.distance(a, b) for n, a, b in zip(L.GRAD_NAMES, ref32["grads"], ref64["grads"])})
    print(c.name, {k: round(v, 4) for k, v in d.items()})
    # the forward at 89.9 degrees and above: tz / r lies within a few fp32 roundings of 1, and one rounding (6e-8) moves asin by
    # 6e-8 / cos(el) = 0.02 degrees at 89.99 -- 3e-5 and 4e-5 of the image through P's elevation weights of 1 / 720 and 1 / 450,
    # against a tolerance of about 5e-5: the fp32 oracle's reference points are inside the rule there, not inside a quarter
    steep = max((L.steep_of(cls) or 0.0) for cls, _ in c.rows) if c.rows else 0.0
    for k, v in d.items():
        assert v <= (1.0 if k == "refs" and steep >= 89.9 else 0.25), (c.name, k, v)
    # what the closed form is for: fp32 autograd of the oracle on the same rows
    rows = L.closed_rows(c, L.cached(c)["inp"])
    if rows.any():
        auto32 = L.reference(c, L.cached(c)["inp"], torch.float32)["g_auto"]
        worst = L.distance(auto32[rows].nan_to_num(nan=float("inf")), ref64["g_closed"][rows])
        print(c.name, "fp32 autograd of the oracle on the closed-form rows: distance", worst)

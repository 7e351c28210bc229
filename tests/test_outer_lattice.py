"""The shape lattice of the rows_outer tests (tests/outer_lattice.py), checked without a GPU: it is deterministic, it reaches
every grid mode / loop / tile class it claims to reach (through its restatement of the host dispatch), its integer operands make
every summation order exact, its fp64 reference equals the definition written as plain loops, and the output floats of distinct
specs never overlap.  The GPU half is tests/test_gpu_rows_outer.py."""
import collections

import numpy as np
import torch

from tests import outer_lattice as L


def _all_paths(pred=lambda c: True):
    return [(c, key, p) for c in L.LATTICE if pred(c) for key, p in L.dispatch(c).paths.items()]


def test_lattice_is_deterministic():
    again = L.build_lattice()
    assert again == L.LATTICE
    assert len({c.name for c in L.LATTICE}) == len(L.LATTICE)
    for c in L.LATTICE:
        assert torch.equal(L.operands(c), L.operands(c)) and L.dispatch(c) == L.dispatch(c)
    assert not torch.equal(L.operands(L.LATTICE[0]), L.operands(L.LATTICE[0], float_pass=True))


def test_every_named_class_occurs():
    disp = {c.name: L.dispatch(c) for c in L.LATTICE}
    modes = collections.Counter(d.mode for d in disp.values())
    paths = collections.Counter()
    for c in L.LATTICE:
        paths.update(set(disp[c.name].paths.values()))
    print("rows_outer lattice:", len(L.LATTICE), "cases; grid modes", dict(modes), "; cases per path", dict(paths))
    # grid modes
    assert set(modes) == set(L.GRID_MODES)
    d = disp["dense-spec256"]
    assert d.mode == "dense:spec" and d.grid == (256, 1, 1) and d.surplus_blocks == 0
    c = L.by_name("dense-spec256")
    assert (c.R, c.W) == (70, 512) and c.specs[0][1] == c.specs[0][3] == 256
    d = disp["dense-total"]
    tiles = [L.spec_tiles(s) for s in L.by_name("dense-total").specs]
    assert d.mode == "dense:total" and sum(tiles) > L.MAX_TILES and max(tiles) <= L.MAX_SPEC_TILES and len(set(tiles)) >= 3
    assert d.grid == (max(tiles), len(tiles), 3) and d.surplus_blocks > 0          # blocks that take the early return
    for c in L.LATTICE:
        if disp[c.name].mode == "compact":
            assert disp[c.name].grid[0] == sum(L.spec_tiles(s) for s in c.specs) <= L.MAX_TILES
    # the model's own call
    c = L.by_name("model-xattn")
    assert (c.G, c.R, c.W, len(c.specs)) == (3, 1600, 848, 13) and disp[c.name].grid == (83, 1, 3)
    assert set(disp[c.name].paths.values()) == {"vec", "scalar:na", "scalar:col_a"} and c.out_gstride == 640 + 480 * 16 + 512 + 512 + 256 + 256
    assert all(c.specs[si][1] == 2 for (si, _, _), p in disp[c.name].paths.items() if p != "vec")
    # every loop and every cause of the scalar one
    assert set(paths) == set(L.PATHS)
    # scalar:base where the base ALONE decides: pointer offset 1, W % 4 == 0 -- every full a-tile at a col_a % 4 == 0
    for name in ("ptr-off1", "ptr-off1-R4099"):
        c = L.by_name(name)
        assert c.ptr_off == 1 and c.W % 4 == 0 and not any(disp[name].base_aligned)
        full = [p for (si, at, g), p in disp[name].paths.items() if c.specs[si][0] % 4 == 0 and c.specs[si][1] - 16 * at >= 16]
        assert full and set(full) == {"scalar:base"}
    # alignment that differs per g with a pointer offset of 0 (R * W % 4 != 0); W % 4 != 0 is the cause the predicate meets first
    c = L.by_name("W50-g3")
    assert c.ptr_off == 0 and (c.R * c.W) % 4 and disp[c.name].base_aligned == [True, False, True]
    assert set(disp[c.name].paths.values()) == {"scalar:W"}
    assert any(len(set(d.base_aligned)) == 2 for d in disp.values())
    # partial last a-tile with n_a > 16 on the scalar loop, full a-tiles on the scalar loop, partial b-tiles, R < 64
    ap = _all_paths()
    assert any(p == "scalar:na" and at > 0 for c, (si, at, g), p in ap)
    assert any(p == "scalar:col_a" and c.specs[si][1] - 16 * at >= 16 for c, (si, at, g), p in ap)
    assert any(p == "scalar:col_a" and 0 < c.specs[si][1] - 16 * at < 16 and at > 0 for c, (si, at, g), p in ap)
    assert any(s[2] >= 0 and s[3] % 16 for c in L.LATTICE for s in c.specs)
    assert any(c.R < 64 for c in L.LATTICE)
    # the axes
    outer = [s for c in L.LATTICE for s in c.specs if s[2] >= 0]
    sums = [s for c in L.LATTICE for s in c.specs if s[2] < 0]
    assert {s[1] for s in outer} >= set(L.NA_VALUES) and {s[3] for s in outer} >= set(L.NB_VALUES)
    assert {(s[1], s[3]) for s in outer} >= {(a, b) for a in L.NA_VALUES[:-1] for b in L.NB_VALUES}
    assert {s[1] for s in sums} >= set(L.COLSUM_NA_VALUES) and all(s[3] == 1 for s in sums)
    assert {c.R for c in L.LATTICE} >= set(L.R_VALUES) and {c.G for c in L.LATTICE} == set(L.G_VALUES)
    assert {len(c.specs) for c in L.LATTICE} >= {1, L.MAX_SPECS}
    assert all(c.G * c.R * c.W <= L.FLOATS_MAX for c in L.LATTICE)
    # an output stride above the floats written, with gaps between the specs
    c = L.by_name("gaps")
    ends = sorted((s[4], s[4] + L.spec_floats(s)) for s in c.specs)
    assert ends[0][0] > 0 and all(b[0] > a[1] for a, b in zip(ends, ends[1:])) and c.out_gstride > ends[-1][1] and c.G > 1
    # a Gram spec and partly overlapping column blocks
    assert any(s[0] == s[2] and s[1] == s[3] for s in outer)
    assert any(s[0] < s[2] < s[0] + s[1] < s[2] + s[3] for s in outer)


def test_exactness_condition_holds_for_every_case():
    for c in L.LATTICE:
        assert L.check_exactness(c)
        x = L.operands(c)
        assert x.dtype == torch.float32 and x.shape == (c.G, c.R, c.W)
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= L.VMAX
        assert 16 * c.R < 2 ** 24
        ref = L.reference(x, c)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 16 * c.R
        assert torch.equal(ref.float().double(), ref)                                  # exact in fp32
        assert not torch.signbit(ref[ref == 0]).any()                                   # zeros are +0.0


def test_reference_equals_the_triple_loop_on_tiny_cases():
    tiny = [L.make_case("tiny-a", 2, 5, 12, [(0, 3, 4, 5), (1, 7, -1, 1), (2, 4, 2, 4)], gap=2, start=1, stride_extra=3),
            L.make_case("tiny-b", 1, 1, 7, [(0, 7, 0, 7), (3, 1, -1, 1)])]
    for c in tiny:
        for fp in (False, True):
            x = L.operands(c, float_pass=fp)
            a, b = L.reference(x, c), L.triple_loop(x, c)
            if fp:
                torch.testing.assert_close(a, b, rtol=1e-13, atol=1e-13)
            else:
                assert torch.equal(a, b)
            assert torch.equal(a[~torch.from_numpy(L.covered_mask(c))], torch.zeros(int((~L.covered_mask(c)).sum()), dtype=torch.float64))
        ab = L.reference(L.operands(c, float_pass=True), c, absolute=True)
        assert bool((ab >= L.reference(L.operands(c, float_pass=True), c).abs() - 1e-12).all())


def test_covered_masks_of_distinct_specs_never_overlap():
    for c in L.LATTICE:
        total = np.zeros(c.G * c.out_gstride, np.int32)
        for si, s in enumerate(c.specs):
            m = L.covered_mask(c, si)
            assert m.shape == (c.G * c.out_gstride,) and int(m.sum()) == c.G * L.spec_floats(s)
            total += m
        assert int(total.max()) == 1, c.name
        assert np.array_equal(total.astype(bool), L.covered_mask(c))
        assert max(s[4] + L.spec_floats(s) for s in c.specs) <= c.out_gstride

"""The host reference of the conv statistics (tests/stats_lattice.py), checked without a GPU: against torch.var and the buffers
F.batch_norm leaves, the fixed-point rule through an encode / decode round trip, the plan restatement against what the library's
host queries answer -- and the SENSITIVITY of the GPU test's bounds: for every ragged launch of tests/test_gpu_conv_stats.py a
producer with one row in the wrong tile, a last tile divided by the tile height, or a padded zero row counted must be flagged."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_lattice as L
from tests import stats_lattice as S


def test_reference_is_torch_var_and_batch_norms_buffers():
    g = torch.Generator().manual_seed(5)
    for M, K, tr in ((1, 5, 64), (37, 12, 64), (300, 20, 128), (257, 7, 256)):
        y = torch.randn(M, K, generator=g, dtype=torch.float64) * 3 + 40
        table = S.tile_table(y.numpy(), tr)
        counts = S.tile_counts(M, tr)
        assert table.shape == (-(-M // tr), 2, K) and int(counts.sum()) == M and int(counts[-1]) == M - tr * (len(counts) - 1)
        for t, n in enumerate(counts):
            blk = y[t * tr:t * tr + n]
            np.testing.assert_allclose(table[t, 0], blk.mean(0).numpy(), rtol=1e-14)
            np.testing.assert_allclose(table[t, 1], (blk.var(0, unbiased=False) * n).numpy(), rtol=1e-11, atol=1e-12)
        mean, var = S.merged(y.numpy())
        mm, m2 = S.merge_table(table, counts)
        np.testing.assert_allclose(mm, mean, rtol=1e-13)
        np.testing.assert_allclose(m2 / M, var, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(var, y.var(0, unbiased=False).numpy(), rtol=1e-11, atol=1e-13)
        gamma, beta = torch.rand(K, generator=g, dtype=torch.float64) + 0.5, torch.randn(K, generator=g, dtype=torch.float64)
        rm, rv = torch.randn(K, generator=g, dtype=torch.float64), torch.rand(K, generator=g, dtype=torch.float64) + 0.5
        block = S.bn_block(mean, var, gamma.numpy(), beta.numpy(), 1e-5)
        if M > 1:      # (F.batch_norm refuses one value per channel; the kernels keep the biased variance there)
            rm_t, rv_t = rm.clone(), rv.clone()
            out = F.batch_norm(y, rm_t, rv_t, gamma, beta, training=True, momentum=0.1, eps=1e-5)
            np.testing.assert_allclose(((y.numpy() - block[0]) * block[1] + block[2]), out.numpy(), rtol=1e-10, atol=1e-10)
            got = S.running_after(mean, var, M, rm.numpy(), rv.numpy(), 0.1)
            np.testing.assert_allclose(got[0], rm_t.numpy(), rtol=1e-13)
            np.testing.assert_allclose(got[1], rv_t.numpy(), rtol=1e-12)
        else:
            got = S.running_after(mean, var, M, rm.numpy(), rv.numpy(), 0.1)
            np.testing.assert_allclose(got[1], 0.9 * rv.numpy(), rtol=1e-14)
        np.testing.assert_allclose(block[3], 1.0 / np.sqrt(var + 1e-5), rtol=1e-15)


def test_fixed_point_rule_round_trip():
    """floor(s / 4) high, (s - 4 high) 2^46 truncated low; the words add as integers; decode(encode(s)) is s truncated to 2^-46."""
    from tests import bn_lattice as B
    g = np.random.default_rng(3)
    s = np.concatenate([g.standard_normal(200) * 10.0 ** g.integers(-3, 9, 200), [0.0, -0.0, 4.0, -4.0, 3.999999, -1e-15, 2.0 ** 40]])
    units = S.encode_units(s)
    for v, u in zip(s, units):
        exact = Fraction(float(v)) * (1 << 46)
        assert 0 <= exact - int(u) < 1, (v, u)      # truncated towards minus infinity to a multiple of 2^-46
    words = S.encode_words(s, s)
    u1, u2 = S.decode_units(words)
    assert list(u1) == list(units) and list(u2) == list(units)
    # where nothing is truncated the words are those of bn_lattice.encode_sums
    e = np.round(g.standard_normal(50) * 1000) / 8.0
    assert np.array_equal(S.encode_words(e, e * e), B.encode_sums(torch.from_numpy(e), torch.from_numpy(e * e)).numpy())
    # integer addition of the words = addition of the units; a carry out of the low word lands in the high word's unit
    a, b = S.encode_words([3.75], [3.75]), S.encode_words([3.5], [-7.25])
    tot = S.decode_units(a + b)
    assert int(tot[0][0]) == int(Fraction(7.25) * (1 << 46)) and int(tot[1][0]) == int(Fraction(-3.5) * (1 << 46))
    # the accumulated sums of a table and the block derived from them
    y = g.integers(-8, 9, size=(300, 6)).astype(np.float64)
    t32 = S.faithful_replay(y, 128)
    u1, u2, slack = S.sums_expected(t32, S.tile_counts(300, 128))
    # sum 1 is sum cnt fl(S / cnt): the column sum up to the rounding of each tile mean and one unit per addend
    slack1 = (S.tile_counts(300, 128)[:, None] * S.U * np.abs(t32[:, 0].astype(np.float64))).sum(0) + 3 * 2.0 ** -46
    assert all(abs(Fraction(int(a), 1 << 46) - int(b)) <= s_ for a, b, s_ in zip(u1, y.sum(0), slack1))
    full, full2, _ = S.sums_expected(S.faithful_replay(y[:256], 128), S.tile_counts(256, 128))      # cnt = 128: the means are exact
    assert [int(v) for v in full] == [int(v) * (1 << 46) for v in y[:256].sum(0)]
    block, mean, var = S.block_from_units(full, full2, 256, np.ones(6), np.zeros(6), 0.0)
    np.testing.assert_allclose(mean, y[:256].mean(0), rtol=1e-15)
    np.testing.assert_allclose(var, y[:256].var(0), rtol=1e-6)
    np.testing.assert_allclose(block[3], 1.0 / y[:256].std(0), rtol=1e-6)
    # three addends below 2^13: one unit of truncation and two fp64 ulp (2^-40 = 64 units) each, at the most
    assert all(3 <= s_ <= 3 * (1 + 2 * 64) for s_ in slack)


@pytest.fixture
def plan_mode():
    from dpft_amd.hip.lib import lib
    was = int(lib.dpft_conv_get_compute()), int(lib.dpft_conv_get_split())

    def set_mode(name):
        compute, split = L.MODES[name]
        assert lib.dpft_conv_set_compute({"fp32": 0, "bf16": 1, "bf16x3": 2}[compute]) == 0 and lib.dpft_conv_set_split(int(split)) == 0
        return lib
    yield set_mode
    lib.dpft_conv_set_compute(was[0])
    lib.dpft_conv_set_split(was[1])


FAMILY = {"stream": "f32", "generic": "vector", "pipe": "f32", "x3": "x3", "vec": "bf16"}


def test_plan_restatement_agrees_with_the_host_queries(plan_mode, monkeypatch):
    """Tile rows (dpft_conv2d_stats_tiles) and kernel family (dpft_conv2d_planned_family, conv_lattice.expected_family) of every
    launch of the GPU test as the restated plan names them; and every required form is reached by some launch."""
    from dpft_amd.hip.lib import make_desc
    bad = []
    for l in S.all_launches() + S.all_launches(child=True):
        if l.tile:
            monkeypatch.setenv("DPFT_FORCE_TILE", l.tile)
        else:
            monkeypatch.delenv("DPFT_FORCE_TILE", raising=False)
        lib = plan_mode(l.mode)
        c = l.case
        p = S.launch_plan(l)
        d = make_desc(c.B, c.H, c.W, c.C, c.K, c.kh, c.kw, c.stride, c.pad)
        tr = C.c_int32(0)
        tiles = int(lib.dpft_conv2d_stats_tiles(C.byref(d), C.byref(tr)))
        if (tr.value, tiles) != (p.bm, -(-L.rows(c) // p.bm)):
            bad.append((l.case.name, l.mode, l.tile, "tile rows", tr.value, p.bm))
        fam = L.expected_family(c, "fwd", l.mode, S.parse_tile(l.tile))
        if FAMILY[p.kernel] != fam:
            bad.append((l.case.name, l.mode, l.tile, "family", FAMILY[p.kernel], fam))
    assert not bad, bad[:10]
    assert set(S.REQUIRED_FORMS) <= S.forms_reached(), set(S.REQUIRED_FORMS) - S.forms_reached()
    assert set(S.REQUIRED_CHILD_FORMS) <= S.forms_reached(child=True), S.forms_reached(child=True)
    # the column sums are taken and declined, the prologue from sums offered and not, each by some launch
    sums = {(S.launch_plan(l, sums=True).stat_sums, S.form_name(S.launch_plan(l))) for l in S.all_launches()}
    assert {(True, "pipe/unsplit"), (True, "pipe/fixup"), (True, "stream/unsplit"), (False, "pipe/reduce_plain"), (False, "generic/unsplit")} <= sums
    assert {S.launch_plan(l).pro_from_sums for l in S.all_launches() if l.pro} == {True, False}
    # ragged and full last tiles, one tile and several, M below the tile
    shapes = {(L.rows(l.case) % S.launch_plan(l).bm != 0, L.rows(l.case) > S.launch_plan(l).bm) for l in S.all_launches()}
    assert shapes == {(True, True), (True, False), (False, True), (False, False)}


def _ragged():
    seen, out = set(), []
    for l in S.all_launches() + S.all_launches(child=True):
        p = S.launch_plan(l)
        key = (l.case.name, l.pro, p.bm, S.table_form(p))
        if L.rows(l.case) % p.bm and key not in seen:
            seen.add(key)
            out.append((l, key))
    for child in (True,):      # the child's forms differ (reduce_stats): their own bounds
        for l in S.all_launches(child=True):
            p = S.launch_plan(l, child=True)
            key = (l.case.name, l.pro, p.bm, S.table_form(p))
            if L.rows(l.case) % p.bm and key not in seen:
                seen.add(key)
                out.append((l, key))
    return out


def test_bounds_see_one_row():
    """Every ragged (case, prologue, tile height, bound form) of the GPU test: the faithful table passes, each wrong replay is
    flagged in at least one entry.  The replays carry the epilogue's arithmetic; the looser forms (reduce + statistics kernel,
    streaming kernel) must flag them as well.  A wrong count changes nothing where the last tile sees padding only (all 0.0):
    those replays equal the faithful table and are set aside, a few padding-heavy geometries."""
    ragged = _ragged()
    assert len(ragged) > 100
    names, blind = set(), set()
    for l, (name, pro, bm, form) in ragged:
        y, unit, _ = S.case_output(l.case, pro)
        ref = S.table_reference(y, bm, form, unit, max(S.launch_plan(l).rbw, 1))
        bad, ratios = S.check_table(S.faithful_replay(y, bm), ref)
        assert not bad and max(ratios) <= 1.0, (name, pro, bm, form, bad, ratios)
        wrong = S.wrong_replays(y, bm)
        assert {"last tile / tile_rows", "padded row counted"} <= set(wrong) and (("row moved" in wrong) == (L.rows(l.case) > bm))
        good = S.faithful_replay(y, bm)
        for fault, table in wrong.items():
            if np.array_equal(table, good):
                # a last tile that sees padding only (every output there is 0.0): a wrong count writes the same table -- no fault
                assert fault != "row moved" and not y[(len(ref.counts) - 1) * bm:].any(), (name, pro, bm, form, fault)
                blind.add(name)
                continue
            flagged, _ = S.check_table(table, ref)
            assert flagged, (name, pro, bm, form, fault)
            names.add(fault)
    assert names == {"row moved", "last tile / tile_rows", "padded row counted"}
    assert 5 * len(blind) <= len({key[0] for _, key in ragged}), blind      # (a few padding-heavy geometries only)
    # an unwritten (NaN) tile is a violation, not a crash
    l, (name, pro, bm, form) = ragged[0]
    y, unit, _ = S.case_output(l.case, pro)
    t = S.faithful_replay(y, bm)
    t[-1, 1, 0] = np.nan
    assert S.check_table(t, S.table_reference(y, bm, form, unit))[0]


@pytest.mark.parametrize("case", S.EXACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_tier_data_is_exact_in_fp32(case):
    """The claims of exact_data(): integers in [-7, 7], quarter-integer tile means, and every quantity the two kernels form
    representable in fp32 with room for any summation order."""
    M, K, tr = case
    y = S.exact_data(M, K, tr)
    assert np.array_equal(y, np.round(y)) and float(np.abs(y).max()) <= 7
    table = S.tile_table(y, tr)
    counts = S.tile_counts(M, tr)
    assert np.array_equal(table[:, 0] * 4, np.round(table[:, 0] * 4))
    assert np.array_equal(table.astype(np.float32).astype(np.float64), table)
    for t, n in enumerate(counts):      # sum of |d|^2 in units of 1/16 below 2^24
        d = y[t * tr:t * tr + n] - table[t, 0]
        assert float((d * d).sum(0).max()) * 16 < 2 ** 24
    mean, m2 = S.merge_table(table, counts)
    s1 = (counts[:, None] * (table[:, 0] - table[0, 0])).sum(0)
    assert np.array_equal(s1, np.round(s1)) and float(np.abs(s1).max()) ** 2 < 2 ** 24
    for v in (mean, m2, m2 / M):
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    np.testing.assert_allclose(m2 / M, y.var(0), rtol=1e-12, atol=1e-12)


def test_direct_case_lists_hit_the_kernels_edges():
    for cases in (S.EXACT_CASES, S.FLOAT_CASES):
        assert {K for _, K, _ in cases} == {12, 64, 96, 256, 320, 2048} and {tr for _, _, tr in cases} == {64, 128, 256}
        assert any(M == 1 for M, _, _ in cases) and any(1 < M < tr for M, _, tr in cases)
    tiles = {-(-M // tr) for M, _, tr in S.FLOAT_CASES}
    assert {1, 32, 33, 65} <= tiles and any(M % tr == 1 and M > tr for M, _, tr in S.FLOAT_CASES)
    assert all(M & (M - 1) == 0 and (M <= tr or M % tr == 0) for M, _, tr in S.EXACT_CASES)
    y = S.float_data(2053, 320)
    off = np.abs(y.astype(np.float64).mean(0)) / y.astype(np.float64).std(0)
    assert 150 < off.max() <= 205 and y.dtype == np.float32

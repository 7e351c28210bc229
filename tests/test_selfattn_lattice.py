"""The tile lattice of the fused training self-attention (tests/selfattn_lattice.py), checked without a GPU: its restatement of the
host rule equals what the library answers (dpft_selfattn_train_tiles: host code), the table reaches every compiled form and
every edge it claims to reach, the large-logit case has the logits it is there for, and the reference builder equals
torch.nn.MultiheadAttention + LayerNorm.  The GPU half is tests/test_gpu_selfattn_tiles.py."""
import ctypes as C

import torch

from tests import selfattn_lattice as L


def test_restated_rule_equals_the_library():
    for c in L.CASES:
        assert L.tiles(c.B, c.Q, c.V) == L.library_tiles(c.B, c.Q, c.V), c.name
    n = 0
    for B in range(1, 17):
        for V in range(1, 5):
            for Q in (1, 7, 100, 400, 900):
                assert L.tiles(B, Q, V) == L.library_tiles(B, Q, V), (B, Q, V)
                n += 1
    assert n == 16 * 4 * 5
    # the model's Q = 400, V = 3: a different form for every batch size up to 6
    assert [L.tiles(B, 400, 3, {})[0][0] for B in (1, 2, 3, 4, 5, 6, 8)] == [2, 3, 4, 5, 6, 8, 8]
    # the restatement reads the tuning variables like the library: 1..8 without 7, per kernel
    env = {"DPFT_SA_QW_FWD": "3", "DPFT_SA_QW_BWD": "7", "DPFT_SA_KW": "8"}
    assert L.tiles(4, 400, 3, env)[0] == (3, 5, 8)
    print("\n".join(L.table_rows(from_library=True)))


def test_table_reaches_every_form_and_edge():
    got = {c.name: L.tiles(c.B, c.Q, c.V, {}) for c in L.CASES}      # {}: the rule itself, no tuning variable
    for c in L.CASES:
        assert got[c.name][0] == (c.qw,) * 3, (c.name, got[c.name])
    assert len({c.name for c in L.CASES}) == len(L.CASES)
    for k in range(3):                                                    # every form, in each of the three kernels
        assert {qw[k] for qw, _ in got.values()} == set(L.FORMS), L.KERNELS[k]
    raw = {c.name: L.raw_qw(c.B, c.Q, c.V) for c in L.CASES if c.qw == 8}
    assert 7 in raw.values() and 8 in raw.values(), raw                   # 8 directly and through 7
    assert raw["qw7to8"] == 7
    assert any(min(lds) > L.LDS_DEFAULT for _, lds in got.values())      # the raised LDS limit, in all three kernels at once
    assert min(got["lds-160k"][1]) > L.LDS_DEFAULT and max(got["lds-160k"][1]) <= 160 * 1024
    for form in L.FORMS[1:]:                                              # a ragged last tile in every form from 2 up
        assert any(c.qw == form and L.ragged(c) for c in L.CASES), form
    assert not L.ragged(L.by_name("qw8-exact")) and L.by_name("qw8-exact").Q % 16 == 0
    rem = {c.Q % 16 for c in L.CASES if c.Q >= 8}
    assert {0, 1, 8, 9} <= rem and rem & {13, 15}, rem
    assert {L.key_class(c.Q) for c in L.CASES} == {"Q<8", "0", "1..8", "9..15"}
    assert any(c.Q == 1 for c in L.CASES) and any(1 < c.Q < 8 for c in L.CASES)
    assert [c.name for c in L.CASES if c.table] == ["table"] and L.by_name("table").B > 1
    # the runs: p = 0 everywhere, p = 0.25 with both seeds, lds-160k at 0.1 only
    for c in L.CASES:
        assert L.runs(c)[0][0] == 0.0
    drop = {c.name: L.runs(c)[1] for c in L.CASES if len(L.runs(c)) > 1}
    assert set(drop) == {c.name for c in L.CASES} - {"one-key"}
    assert drop["lds-160k"][0] == 0.1 and all(r[0] == 0.25 for n, r in drop.items() if n != "lds-160k")
    ragged_seeds = {r[1] for n, r in drop.items() if L.ragged(L.by_name(n))}
    assert any(s > 2 ** 32 for s in ragged_seeds) and any(s < 0 for s in ragged_seeds)
    assert len(L.RUNS) == 2 * len(L.CASES) - 1 and len({L.run_id(r) for r in L.RUNS}) == len(L.RUNS)


def test_large_logit_case_has_large_logits_outside_the_first_slice():
    c = L.by_name("L")
    x, pos, _ = L.operands(c)
    s = L.scaled_scores(c, L.make_layers(c), x, pos)                      # (V,B,8,Q,Q)
    assert float(s.abs().max()) > 100, float(s.abs().max())
    assert float(s.max(-1).values.max()) > 100                           # as a row maximum: exp(s) overflows fp32 above 88.7
    assert float(s.max()) > 88.8
    arg = s.argmax(-1)                                                    # key of the maximum per (view, batch, head, query)
    assert int(((arg % 8) != 0).sum()) > 0                                # lane slice = key % 8: a maximum the merge has to carry over
    assert len({int(a) % 8 for a in arg.flatten()}) == 8                  # in fact in every slice
    # the ordinary cases stay small: what the existing tests cover
    c0 = L.by_name("qw2")
    x0, pos0, _ = L.operands(c0)
    assert float(L.scaled_scores(c0, L.make_layers(c0), x0, pos0).abs().max()) < 30


def test_query_refuses_bad_sizes():
    from dpft_amd.hip.lib import lib
    qw, lds = (C.c_int32 * 3)(), (C.c_int64 * 3)()
    ask = lambda B, Q, V: lib.dpft_selfattn_train_tiles(B, Q, V, C.byref(qw), C.byref(lds))
    for B, Q, V in ((0, 4, 1), (1, 0, 1), (1, 4, 0), (1, 4, 5), (-1, 4, 1)):
        assert ask(B, Q, V) == -1
        assert f"selfattn_train: bad sizes (V={V}, B={B}, Q={Q})".encode() in lib.dpft_last_error()
    assert ask(64, 2100, 4) == -1 and b"selfattn_train: problem too large for the mask index" in lib.dpft_last_error()
    assert lib.dpft_selfattn_train_tiles(1, 4, 1, None, C.byref(lds)) == -1 and b"selfattn_train_tiles: null output" in lib.dpft_last_error()
    assert lib.dpft_selfattn_train_tiles(1, 4, 1, C.byref(qw), None) == -1
    assert ask(8, 400, 3) == 0 and tuple(qw) == (8, 8, 8) and tuple(lds) == (89280, 71872, 92352)


def test_replayed_masks_keep_rate_and_view_offset():
    from tests.dropout_masks import self_attn_masks
    c = L.by_name("qw5-ragged")
    p, seed, salt = L.runs(c)[1]
    att, d1 = self_attn_masks(seed, salt, p, c.V, c.B, c.Q)
    keep = float((att > 0).mean())
    assert abs(keep - (1 - p)) < 0.01, keep
    # one view at a time (what the reference builder asks for) is the same table
    c = L.by_name("empty-slices")
    p, seed, salt = L.runs(c)[1]
    att, d1 = self_attn_masks(seed, salt, p, c.V, c.B, c.Q)
    for v in range(c.V):
        a1, b1 = self_attn_masks(seed, salt, p, 1, c.B, c.Q, view0=v)
        assert (a1[0] == att[v]).all() and (b1[0] == d1[v]).all()


def test_reference_builder_equals_torch_multihead_attention():
    """The fp64 builder at p = 0 against nn.MultiheadAttention + residual + LayerNorm in fp64, forward and every gradient."""
    c = L.by_name("empty-slices")
    layers = [ml.double() for ml in L.make_layers(c)]
    x, pos, gy = L.operands(c)
    y, grads = L.reference(c, layers, x, pos, gy, L.runs(c)[0])
    x64, pos64 = x.double().requires_grad_(True), pos.double().requires_grad_(True)
    qk = x64 + pos64
    ref = torch.stack([ml.norm1(x64 + ml.self_attn(qk, qk, x64, need_weights=False)[0]) for ml in layers])
    params = [ml.get_parameter(k[3:]) for ml in layers for k in L.PARAM_KEYS]
    gref = torch.autograd.grad(ref, [x64, pos64] + params, gy.double())
    torch.testing.assert_close(y, ref.detach(), rtol=1e-12, atol=1e-12)
    assert len(grads) == len(gref) == len(L.grad_names(c))
    for name, a, b in zip(L.grad_names(c), grads, gref):
        assert a.shape == b.shape and L.rel_l2(a, b) < 1e-12, name
    # the table form is the dense form on the expanded table, its gradient summed over the batch
    t = L.by_name("table")
    layers = L.make_layers(t)
    xt, post, gyt = L.operands(t)
    yt, gt = L.reference(t, layers, xt, post, gyt, L.runs(t)[0])
    dense = t._replace(table=False)
    yd, gd = L.reference(dense, layers, xt.expand(t.B, -1, -1).contiguous(), post, gyt, L.runs(t)[0])
    torch.testing.assert_close(yt, yd, rtol=1e-12, atol=1e-12)      # (a strided and a dense operand may take different sum orders)
    assert gt[0].shape == (t.Q, 16) and L.rel_l2(gt[0], gd[0].sum(0)) < 1e-12
    for a, b in zip(gt[1:], gd[1:]):
        assert L.rel_l2(a, b) < 1e-12
    # one key: softmax is 1 whatever the scores, so nothing flows to q / k
    o = L.by_name("one-key")
    xo, poso, gyo = L.operands(o)
    _, go = L.reference(o, L.make_layers(o), xo, poso, gyo, L.runs(o)[0])
    assert not go[1].any() and not go[2][:32].any() and not go[3][:32].any() and go[2][32:].any() and go[0].any()

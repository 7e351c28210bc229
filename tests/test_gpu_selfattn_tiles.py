"""Every compiled tile form of the fused training self-attention (decoder_train.hip: sa_train_fwd_kernel<QW>,
sa_train_bwd_q_kernel<QW>, sa_train_bwd_kv_kernel<KW>, QW / KW in {1, 2, 3, 4, 5, 6, 8}) against the fp64 oracle, at the tile, key
loop, LDS and input-form edges of tests/selfattn_lattice.py.  The CPU half (what the table reaches) is
tests/test_selfattn_lattice.py."""
import pytest
import torch

from tests import selfattn_lattice as L

pytestmark = pytest.mark.gpu

FWD_RTOL, FWD_ATOL = 1e-4, 2e-5      # the rule of the self-attention tests of tests/test_gpu_kernels.py
GRAD_TOL = 2e-4                      # relative L2 per gradient tensor (their _check_grads)
ZERO_SCALE = 1e-5                    # close()'s absolute rule where the reference is identically zero


def _finite(name, t):
    assert bool(torch.isfinite(t).all()), f"{name}: NaN or Inf"


def _run(c, layers, x, pos, gy, run, dev):
    """-> (y, saved (lse, attn, zhat, rstd), gradients [x, pos, six per view]) of tf.self_attn_blocks on the device."""
    from dpft_amd.models.fusers import train_fused as tf
    p_drop, seed, salt = run
    xd, posd = x.to(dev).requires_grad_(True), pos.to(dev).requires_grad_(True)
    plist = [t for ml in layers for t in tf.sa_params(ml)]
    seed_t = torch.full((1,), seed, dtype=torch.int64, device=dev)
    y = tf.self_attn_blocks(layers, xd, posd, seed_t, salt, p_drop, batch=c.B if c.table else None)
    saved = [t.clone() for t in y.grad_fn.saved_tensors[3:7]]
    grads = torch.autograd.grad(y, [xd, posd] + plist, gy.to(dev))
    return y.detach(), saved, grads


@pytest.mark.parametrize("case_run", L.RUNS, ids=L.run_id)
def test_selfattn_tile_forms_vs_fp64_oracle(case_run):
    """Forward (rtol 1e-4, atol 2e-5) and every gradient (relative L2 < 2e-4; where the reference is identically zero, |got| <=
    1e-5 max |reference dx|) of each tile form against the fp64 oracle with the kernels' dropout decisions replayed; no NaN / Inf
    in any output, saved buffer or gradient; the forward repeats bit for bit; the broadcast (Q, 16) table equals the dense call.

    Case L (scaled scores up to 336 in magnitude, far past what exp() takes in fp32 without the max subtraction): the
    tolerance is 4 times the distance of the SAME reference evaluated in fp32 on the CPU from its fp64 value, per quantity --
    the kernels' __expf / __logf and summation order are a different but equally rounded evaluation.  Both distances are
    recomputed and printed.  Measured on an MI355X (fp32 CPU reference | kernel):
      p = 0:    forward max |dy| 2.391e-06 | 2.213e-06;  largest relative L2 of a gradient (dpos) 2.835e-06 | 3.869e-06
      p = 0.25: forward max |dy| 4.388e-06 | 4.597e-06;  largest relative L2 of a gradient (dpos) 3.130e-06 | 3.608e-06
    Largest kernel / fp32-reference ratio of a single tensor: 2.4 (d in_proj_bias of view 1, 9.68e-07 against 4.07e-07)."""
    c, run = case_run
    p_drop = run[0]
    dev = torch.device("cuda", 0)
    # the form this case is there for: a changed kNumCU or rule fails here instead of folding the table onto QW = 1
    qw, lds = L.library_tiles(c.B, c.Q, c.V)
    assert qw == (c.qw,) * 3, (c.name, qw)
    assert (qw, lds) == L.tiles(c.B, c.Q, c.V)
    if c.name == "lds-160k":
        assert min(lds) > L.LDS_DEFAULT

    layers = L.make_layers(c)
    x, pos, gy = L.operands(c)
    ref_y, ref_g = L.reference(c, layers, x, pos, gy, run)
    names = L.grad_names(c)
    dev_layers = [ml.to(dev) for ml in L.make_layers(c)]
    y, saved, grads = _run(c, dev_layers, x, pos, gy, run, dev)

    _finite("y1", y)
    for n, t in zip(("lse", "attn", "zhat", "rstd"), saved):
        _finite(n, t)
    assert saved[0].shape == (c.V, c.B, c.Q, 8) and saved[3].shape == (c.V, c.B, c.Q)
    for n, g in zip(names, grads):
        _finite("d" + n, g)

    from dpft_amd.models.fusers import train_fused as tf
    seed_t = torch.full((1,), run[1], dtype=torch.int64, device=dev)
    with torch.no_grad():
        y2 = tf.self_attn_blocks(dev_layers, x.to(dev), pos.to(dev), seed_t, run[2], p_drop, batch=c.B if c.table else None)
    assert torch.equal(y, y2), f"{c.name}: the forward does not repeat bit for bit"

    got_y = y.double().cpu()
    if c.name == "L":
        y32, g32 = L.reference(c, layers, x, pos, gy, run, dtype=torch.float32)
        d_fwd = float((y32.double() - ref_y).abs().max())
        d_grad = [L.rel_l2(a, b) for a, b in zip(g32, ref_g)]
        k_fwd = float((got_y - ref_y).abs().max())
        k_grad = [L.rel_l2(a, b) for a, b in zip(grads, ref_g)]
        print(f"selfattn L p={p_drop}: forward max distance from fp64: fp32 reference {d_fwd:.3e}, kernel {k_fwd:.3e}, allowed {4 * d_fwd:.3e}")
        for n, a, b in zip(names, d_grad, k_grad):
            print(f"selfattn L p={p_drop}: d{n} relative L2 from fp64: fp32 reference {a:.3e}, kernel {b:.3e}, allowed {4 * a:.3e}")
        print(f"selfattn L p={p_drop}: largest gradient distance: fp32 reference {max(d_grad):.3e}, kernel {max(k_grad):.3e}")
        assert 0 < d_fwd < 1e-2 and 0 < max(d_grad) < 1e-2      # the yardstick itself is sane
        assert k_fwd <= 4 * d_fwd, (k_fwd, d_fwd)
        for n, a, b in zip(names, d_grad, k_grad):
            assert b <= 4 * a, (n, b, a)
    else:
        torch.testing.assert_close(got_y, ref_y, rtol=FWD_RTOL, atol=FWD_ATOL)
        zero_atol = ZERO_SCALE * max(float(ref_g[0].abs().max()), 1e-6)
        for n, a, b in zip(names, grads, ref_g):
            a = a.double().cpu()
            assert a.shape == b.shape, n
            if not b.any():
                assert float(a.abs().max()) <= zero_atol, (n, float(a.abs().max()), zero_atol)
                continue
            err = L.rel_l2(a, b)
            assert err < GRAD_TOL, (n, err, float(b.norm()))
            if n.endswith(("in_proj_w", "in_proj_b")) and not b[:32].any():      # one key: nothing flows to the q / k rows
                assert float(a[:32].abs().max()) <= zero_atol, (n, float(a[:32].abs().max()), zero_atol)
        if c.name == "one-key":
            assert not ref_g[1].any() and not ref_g[2][:32].any() and not ref_g[3][:32].any()

    if c.table:      # the same call on the expanded table (batch stride Q * 16 instead of 0)
        dense = c._replace(table=False)
        yd, _, gd = _run(dense, dev_layers, x.expand(c.B, -1, -1).contiguous(), pos, gy, run, dev)
        assert torch.equal(y, yd), "broadcast table and dense x differ in the forward"
        dxd = gd[0].sum(0)
        assert grads[0].shape == (c.Q, 16) and L.rel_l2(dxd, ref_g[0]) < GRAD_TOL and L.rel_l2(grads[0], dxd) < GRAD_TOL
        for n, a, b in zip(names[1:], grads[1:], gd[1:]):
            assert L.rel_l2(a, b) < GRAD_TOL, n

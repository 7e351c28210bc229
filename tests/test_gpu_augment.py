"""The three augmentation kernels (csrc/preproc.hip), one launch at a time, against tests/augment_ref.py (fp64) and -- where
the contract is bit-equality -- against the plain resize / scaling kernels they replace."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _P(flip=False, zoom=1.0, shift=(0.0, 0.0), **kw):
    from dpft_amd.data.augment import SampleParams
    return SampleParams(flip=flip, zoom=zoom, shift=shift, **kw)


def _frames(shape, dtype, seed, lo=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(lo, 256, shape, generator=g, dtype=torch.uint8)
    if dtype == torch.uint8:
        return x
    return (x.float() + torch.rand(shape, generator=g) * 0.5).clamp_(float(lo), 255.0)


# (B, Hs, Ws, C) -> (Hd, Wd): even and odd W, Wd = 1, upsampling, image_size None, one sample more than the by-value chunk
EXACT = [((3, 7, 10, 3), (5, 7)), ((3, 9, 9, 1), (4, 4)), ((3, 6, 5, 4), (13, 11)), ((3, 7, 10, 3), (3, 1)),
         ((3, 5, 8, 3), None), ((3, 5, 7, 4), None), ((9, 3, 4, 3), (2, 3)), ((9, 3, 4, 1), None)]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape,size", EXACT)
def test_identity_and_flip_have_the_bits_of_the_resize_kernel(shape, size, dtype):
    """No zoom, no shift, no photometric step: the bits of ``resize_bilinear`` (of the frame itself as float for size None),
    mirrored along x on the flipped samples -- samples 0 and 2 (every even one) flip, the others do not."""
    from dpft_amd.data.augment import augment_camera
    from dpft_amd.data.preprocess import resize_bilinear
    from dpft_amd.hip.lib import AUGMENT_CHUNK
    assert shape[0] in (3, AUGMENT_CHUNK + 1)
    x = _frames(shape, dtype, seed=sum(shape)).to(DEV)
    plain = resize_bilinear(x, size) if size is not None else x.float()
    same = augment_camera(x, size, [_P() for _ in range(shape[0])])
    assert same.shape == plain.shape and same.dtype == torch.float32
    assert torch.equal(same, plain)
    flips = [b % 2 == 0 for b in range(shape[0])]
    got = augment_camera(x, size, [_P(flip=f) for f in flips])
    for b, f in enumerate(flips):
        want = torch.flip(plain[b], [1]) if f else plain[b]
        assert torch.equal(got[b], want), (b, f)
    all_flipped = augment_camera(x, size, [_P(flip=True) for _ in flips])
    assert torch.equal(all_flipped, torch.flip(plain, [2]))


# four samples per launch: zoom 0.8 and 1.25, shifts of both signs, with and without the flip
WARPS = [dict(zoom=0.8, shift=(0.05, -0.03), flip=False), dict(zoom=1.25, shift=(-0.04, 0.05), flip=True),
         dict(zoom=0.8, shift=(-0.05, 0.02), flip=True), dict(zoom=1.25, shift=(0.03, -0.05), flip=False)]
WARP_SHAPES = [((7, 10), (6, 9)), ((9, 9), None), ((48, 64), (24, 32)), ((48, 64), (60, 80))]


def _warp_refs(src, size, canvas):
    Hs, Ws = src.shape[1:3]
    Hd, Wd = size if size is not None else (Hs, Ws)
    H, W = canvas
    return [R.warp_camera(src[b].double().numpy(), Hd, Wd, W, H, R.camera_map(W, H, p["flip"], p["zoom"], p["shift"]))
            for b, p in enumerate(WARPS)]


def _check_warp(got, refs, Hs, Ws):
    eps = 8 * R.ulp32(max(Ws, Hs))
    worst, near_frac = 0.0, 0.0
    for b, r in enumerate(refs):
        g = got[b].double().cpu().numpy()
        near = R.near_frame_edge(r, Hs, Ws, eps)
        near_frac = max(near_frac, near.mean())
        fill, live = r["fill"] & ~near, ~r["fill"] & ~near
        assert np.all(g[fill] == 0.0), f"sample {b}: a fill pixel is not exactly 0"
        assert np.all(g[live] > 0.0), f"sample {b}: a pixel inside the frame was filled"      # the sources hold no 0
        bound = 8 * R.ulp32(255) + eps * r["D"]
        err = np.abs(g - r["out"])
        ratio = (err / bound)[live]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert np.all(err[live] <= bound[live]), (b, float(ratio.max()))
        assert live.mean() > 0.3 and (r["fill"].mean() > 0.02 or WARPS[b]["zoom"] > 1)     # the case reaches both kinds
    assert near_frac < 0.01
    return worst


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("src_hw,size", WARP_SHAPES)
def test_general_warp_vs_fp64(src_hw, size, dtype):
    """Per element |got - ref| <= 8 ulp32(255) + 8 ulp32(max(Ws, Hs)) D, D the largest difference among the element's four
    taps (value rounding + fp32 coordinate rounding; bilinear is continuous across cell borders).  Fill pixels are exactly 0
    and agree with the reference, except within 8 ulp32(max(Ws, Hs)) of the frame edge (under 1 % of a case, asserted).
    Largest observed error on gfx950: 0.091 of the bound (7x10 -> 6x9, f32 source); 0.047 to 0.083 in the other cases."""
    Hs, Ws = src_hw
    src = _frames((len(WARPS), Hs, Ws, 3), dtype, seed=Hs * Ws, lo=1)
    refs = _warp_refs(src, size, (Hs, Ws))
    from dpft_amd.data.augment import augment_camera
    got = augment_camera(src.to(DEV), size, [_P(**p) for p in WARPS])
    worst = _check_warp(got, refs, Hs, Ws)
    print(f"general warp {src_hw}->{size} {dtype}: largest error / bound = {worst:.3f}")


def test_warp_does_not_depend_on_the_canvas_size_and_takes_one_channel():
    """The canvas (X_shape) may differ from the frame that arrives (a dataset that stores reduced frames): the map is stated
    in canvas units, so the same parameters give the same picture.  C = 1 and C = 4 through the general path."""
    from dpft_amd.data.augment import augment_camera
    for C in (1, 4):
        src = _frames((len(WARPS), 9, 12, C), torch.float32, seed=40 + C, lo=1)
        got = augment_camera(src.to(DEV), (7, 9), [_P(**p) for p in WARPS])
        for canvas in ((9, 12), (720, 960)):
            refs = [R.warp_camera(src[b].double().numpy(), 7, 9, canvas[1], canvas[0],
                                  R.camera_map(canvas[1], canvas[0], p["flip"], p["zoom"], p["shift"]))
                    for b, p in enumerate(WARPS)]
            _check_warp(got, refs, 9, 12)


def test_photometric_step():
    """clip(g_c v + o, 0, 255) on the interpolated value: gains that saturate at both ends, contrast 0 (a flat 127.5,
    exactly), per-channel gains; on fill pixels the result stays exactly 0.  Bound: the fp32 roundings of g_c, o, the fused
    multiply-add and the value itself, 8 ulp32(255) max(1, |g|)."""
    from dpft_amd.data.augment import augment_camera
    src = _frames((5, 6, 8, 3), torch.uint8, seed=77, lo=1)
    params = [_P(brightness=3.0), _P(contrast=3.0, channel=(1.0, 1.0, 1.0)), _P(contrast=0.0),
              _P(channel=(0.5, 1.0, 1.7), flip=True), _P(brightness=1.3, contrast=0.6, channel=(1.1, 0.9, 1.0), zoom=0.8)]
    got = augment_camera(src.to(DEV), None, params).double().cpu().numpy()
    for b, p in enumerate(params):
        m = R.camera_map(8, 6, p.flip, p.s, (0.0, 0.0))
        r = R.warp_camera(src[b].double().numpy(), 6, 8, 8, 6, m, gains=p.gain, offset=p.offset)
        bound = 8 * R.ulp32(255) * max(1.0, r["gmax"]) + 8 * R.ulp32(8) * r["D"] * r["gmax"]
        assert np.all(np.abs(got[b] - r["out"]) <= bound), b
        assert np.all(got[b][r["fill"]] == 0.0)
    assert got[0].max() == 255.0 and (got[0] == 255.0).mean() > 0.3            # brightness 3 saturates the top
    assert got[1].max() == 255.0 and got[1].min() == 0.0                        # contrast 3 saturates both ends
    assert np.all(got[2] == 127.5)                                              # contrast 0: flat, whatever the frame
    assert params[4].s == 0.8 and (got[4] == 0.0).any()                         # the fill ignores gain and offset
    ident = augment_camera(src.to(DEV), None, [_P() for _ in range(5)])
    assert torch.equal(ident.cpu(), src.float())                                # g = 1, o = 0: skipped, the bits stay


def _radar(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = 60.0 + torch.rand(shape, generator=g) * 180.0                           # dB, partly outside [100, 200]
    edge = torch.tensor([100.0, 200.0, 97.0, 103.0, 197.0, 203.0, 99.99999, 200.00002, 50.0, 250.0, 100.00001, 199.99998])
    x.view(-1)[:edge.numel()] = edge
    x.view(-1)[-edge.numel():] = edge
    return x


@pytest.mark.parametrize("shape", [(3, 37, 107, 6), (1, 3, 4, 6), (9, 2, 107, 6)])
def test_radar_bits_and_flip(shape):
    """delta = 0: the bits of ``scale_clip``, mirrored along the azimuth axis (axis 2) on the flipped samples; scaling off:
    the flip alone."""
    from dpft_amd.data.augment import augment_radar
    from dpft_amd.data.preprocess import scale_clip
    x = _radar(shape, seed=shape[1]).to(DEV)
    plain = scale_clip(x)
    B = shape[0]
    assert torch.equal(augment_radar(x, [_P() for _ in range(B)]), plain)
    flips = [b % 2 == 0 for b in range(B)]
    got = augment_radar(x, [_P(flip=f) for f in flips])
    raw = augment_radar(x, [_P(flip=f, delta_db=2.0) for f in flips], scale=False)
    for b, f in enumerate(flips):
        assert torch.equal(got[b], torch.flip(plain[b], [1]) if f else plain[b]), b
        assert torch.equal(raw[b], torch.flip(x[b], [1]) if f else x[b]), b
    assert torch.equal(x, _radar(shape, seed=shape[1]).to(DEV))                 # out of place


@pytest.mark.parametrize("shape", [(4, 5, 107, 6), (1, 3, 4, 6)])
def test_radar_gain_vs_fp64(shape):
    """clip(((x + delta) - 100) / 100 * 255, 0, 255) with delta = +-3 dB, values on the clip edges (100, 200 dB) and beyond.
    Bound 8 ulp32(255): the sum, the difference (each half an ulp32(256) times 2.55), the quotient and the product."""
    from dpft_amd.data.augment import augment_radar
    x = _radar(shape, seed=11)
    deltas = [3.0, -3.0, 0.0, 3.0][:shape[0]]
    flips = [False, True, True, False][:shape[0]]
    got = augment_radar(x.to(DEV), [_P(flip=f, delta_db=d) for f, d in zip(flips, deltas)]).double().cpu().numpy()
    for b, (f, d) in enumerate(zip(flips, deltas)):
        ref = R.radar_line(x[b].double().numpy(), d, f)
        assert np.abs(got[b] - ref).max() <= 8 * R.ulp32(255), (b, np.abs(got[b] - ref).max())
        assert got[b].min() == 0.0 and got[b].max() == 255.0
    # on the edges themselves: 97 + 3 -> 0, 203 - 3 -> 255, 100 - 3 -> 0 (clipped), 197 + 3 -> 255, exactly
    probe = torch.tensor([97.0, 203.0, 100.0, 197.0, 150.0, 153.0]).view(1, 1, 1, 6).repeat(2, 1, 1, 1).to(DEV)
    out = augment_radar(probe, [_P(delta_db=3.0), _P(delta_db=-3.0)]).cpu().view(2, 6)
    assert out[0, 0] == 0.0 and out[0, 1] == 255.0 and out[0, 3] == 255.0 and 0.0 < out[0, 2] < 8.0
    assert out[1, 0] == 0.0 and out[1, 1] == 255.0 and out[1, 2] == 0.0 and out[1, 5] == 127.5


def _grid(t, scale=1024.0):
    return torch.round(t * scale) / scale          # entries on a 2^-10 grid: the flip's W - P is then exact in fp32


def _geometry_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    cam_p = torch.tensor([[640.0, -560, 0, 0], [360, 0, -560, 0], [1, 0, 0, 0], [0, 0, 0, 1.0]]).repeat(B, 1, 1)
    cam_p[:, :2] += torch.rand(B, 2, 4, generator=g) * 10 - 5
    rad_t = torch.eye(4).repeat(B, 1, 1)
    rad_t[:, :3, :] += torch.rand(B, 3, 4, generator=g) * 0.2 - 0.1
    rad_p = torch.tensor([[0, -1.0, 0, 53], [256 / 118.03710938, 0, 0, 0], [0, 0, 0, 1.0]]).repeat(B, 1, 1)
    rad_p[:, :2] += torch.rand(B, 2, 4, generator=g) * 0.2 - 0.1
    cam2_p = torch.rand(B, 4, 4, generator=g) * 20 - 10                      # a 4x4 P with a full divisor row, behind a T
    views = [(torch.zeros(B, 4, 4), _grid(cam_p), torch.tensor([[720, 1280, 3]] * B), True),
             (_grid(rad_t), _grid(rad_p), torch.tensor([[256, 107, 6]] * B), False),
             (_grid(rad_t.flip(0)), _grid(cam2_p), torch.tensor([[48, 64]] * B), True)]
    rows = [3, 0, 5, 1, 0, 8, 2, 0, 4][:B]
    labels = []
    for m in rows:
        yaw = torch.rand(m, generator=g) * 6.28 - 3.14
        labels.append({"gt_center": torch.rand(m, 3, generator=g) * 40 - 10, "gt_size": torch.rand(m, 3, generator=g) + 1,
                       "gt_angle": torch.stack((torch.sin(yaw), torch.cos(yaw)), -1),
                       "gt_class": torch.tensor([[0.0, 1.0]]).repeat(m, 1), "description": m})
    return views, labels


GEO = [dict(), dict(flip=True), dict(zoom=0.8, shift=(0.05, -0.03)), dict(flip=True, zoom=1.25, shift=(-0.04, 0.05)),
       dict(flip=True), dict(zoom=1.1), dict(flip=True, zoom=0.9, shift=(0.02, 0.02)), dict(), dict(flip=True, shift=(0.01, 0.0))]


def test_geometry_launch_vs_fp64():
    """Every matrix and label element of a batch one larger than the by-value chunk.  T', the labels, the divisor rows and
    every element of a sample that only flips (or does nothing) are EXACT; rows 0 and 1 of P under a zoom / shift are within
    4 ulp32 of |a P0| + |b_u P2| (the fp32 roundings of a, b_u = (b_u / W) W, the products and the sum).  Zero-box samples
    pass through, the inputs keep their bits (out of place), what is not geometry is passed on."""
    from dpft_amd.data.augment import augment_geometry
    from dpft_amd.hip.lib import AUGMENT_CHUNK
    B = AUGMENT_CHUNK + 1
    views, labels = _geometry_inputs(B, seed=3)
    params = [_P(**p) for p in GEO]
    dviews = [(t.to(DEV), p.to(DEV), s.to(DEV), c) for t, p, s, c in views]
    dlabels = [{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in l.items()} for l in labels]
    out_views, out_labels = augment_geometry(dviews, dlabels, params)
    for (t, p, s, _), (dt, dp, ds, _) in zip(views, dviews):                # inputs bit-unchanged
        assert torch.equal(dt.cpu(), t) and torch.equal(dp.cpu(), p) and torch.equal(ds.cpu(), s)
    for l, dl in zip(labels, dlabels):
        assert torch.equal(dl["gt_center"].cpu(), l["gt_center"]) and torch.equal(dl["gt_angle"].cpu(), l["gt_angle"])
    n_exact = n_bounded = 0
    for v, ((t, p, s, is_cam), (t2, p2)) in enumerate(zip(views, out_views)):
        assert t2.data_ptr() != dviews[v][0].data_ptr() and p2.shape == p.shape
        H, W = int(s[0, 0]), int(s[0, 1])
        for b, q in enumerate(GEO):
            flip, zoom, shift = q.get("flip", False), q.get("zoom", 1.0), q.get("shift", (0.0, 0.0))
            m = R.camera_map(W, H, flip, zoom, shift) if is_cam else R.radar_map(W, flip)
            rt, rp = R.matrices(t[b].double().numpy(), p[b].double().numpy(), m, flip)
            gt, gp = t2[b].double().cpu().numpy(), p2[b].double().cpu().numpy()
            assert np.array_equal(gt, rt), (v, b)
            assert np.array_equal(gp[2:], rp[2:]), (v, b)
            if not is_cam or (zoom == 1.0 and shift == (0.0, 0.0)):
                assert np.array_equal(gp, rp), (v, b)
                n_exact += 1
            else:
                a, bu, sz, bv = m
                p64 = np.abs(p[b].double().numpy())
                mag = np.stack([abs(a) * p64[0] + abs(bu) * p64[2], sz * p64[1] + abs(bv) * p64[2]])
                bound = np.array([[4 * R.ulp32(x) for x in row] for row in mag])
                assert np.all(np.abs(gp[:2] - rp[:2]) <= bound), (v, b, np.abs(gp[:2] - rp[:2]) / bound)
                n_bounded += 1
    assert n_exact >= 15 and n_bounded >= 8
    assert not out_views[0][0].any() and not torch.signbit(out_views[0][0]).any()      # all-zero T stays all-zero, +0
    for b, (l, o, q) in enumerate(zip(labels, out_labels, GEO)):
        rc, ra = R.labels(l["gt_center"].double().numpy(), l["gt_angle"].double().numpy(), q.get("flip", False))
        assert o["gt_center"].shape == l["gt_center"].shape and o["gt_angle"].shape == l["gt_angle"].shape
        assert np.array_equal(o["gt_center"].double().cpu().numpy(), rc), b
        assert np.array_equal(o["gt_angle"].double().cpu().numpy(), ra), b
        assert o["gt_size"] is dlabels[b]["gt_size"] and o["gt_class"] is dlabels[b]["gt_class"] and o["description"] == l["description"]
    # the worked example through the kernel: the fixed range-azimuth row [0, -1, 0, 53] becomes [0, -1, 0, 54]
    P = torch.tensor([[[0, -1.0, 0, 53], [256 / 118.04, 0, 0, 0], [0, 0, 0, 1.0]]]).to(DEV)
    (t2, p2), = augment_geometry([(torch.eye(4)[None].to(DEV), P, torch.tensor([[256, 107, 6]]).to(DEV), False)], None,
                                 [_P(flip=True)])[0]
    assert p2[0, 0].tolist() == [0.0, -1.0, 0.0, 54.0] and torch.equal(p2[0, 1:], P[0, 1:]) and torch.equal(t2[0].cpu(), torch.eye(4))


def test_entry_points_refuse_bad_arguments():
    from dpft_amd.data.augment import augment_camera, augment_geometry, augment_radar
    from dpft_amd.hip.lib import HipLibraryError
    x = torch.zeros(2, 4, 4, 5, device=DEV)
    with pytest.raises(HipLibraryError, match="at most 4 channels"):
        augment_camera(x, None, [_P(), _P()])
    with pytest.raises(ValueError, match="parameter sets"):
        augment_radar(x, [_P()])
    with pytest.raises(HipLibraryError, match="device tensors"):
        augment_camera(torch.zeros(1, 4, 4, 3), None, [_P()])
    with pytest.raises(ValueError, match="at most"):
        augment_geometry([(None, None, None, True)] * 5, None, [_P()])

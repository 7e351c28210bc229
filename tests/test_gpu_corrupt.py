"""The two sensor degradation launches (dpft_amd/csrc/corrupt.hip) against the numpy restatement tests/corrupt_ref.py.

Blur off: every output bit equals the restatement (haze, noise, the clamp at 0 and 255, erase rectangles, off, the neutral
copy).  Blur on: |out - fp64 reference| <= 2 (2R + 2) 2^-24 255 -- per pass the rounding of a (2R + 1)-term convex sum of
values <= 255 (one rounding per tap and sum, whatever the order, with or without fma: (2R + 1) 2^-24 255) plus one more unit
that covers the two roundings of the noise step where it is active (noise <= 25 in the blurred cases: product and sum stay
below 512, where half an ulp is 2^-16).  The shapes come from ``dpft_corrupt_limits``: a frame
smaller than any halo, one pixel past a tile edge in H and in W, an exact multiple of the tile, C = 1 and 4, B = 1, the chunk
and the chunk + 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import corrupt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = 0x0DDB_A11C_0FFE_E000


@functools.lru_cache(maxsize=None)
def _limits():
    from dpft_amd.hip.lib import lib
    out = (C.c_int32 * 4)()
    lib.call("dpft_corrupt_limits", out)
    return tuple(out)


def _shapes():
    th, tw, _, chunk = _limits()
    return [(2, 5, 7, 3), (1, th + 1, tw + 1, 3), (2, 2 * th, 2 * tw, 4), (chunk, th + 1, tw + 1, 1), (chunk + 1, 9, tw + 2, 3)]


def test_shapes_straddle_the_limits():
    th, tw, rmax, chunk = _limits()
    assert rmax == 15 == R.radius(5.0) and chunk >= 2
    shapes = _shapes()
    assert any(h < rmax and w < rmax for _, h, w, _ in shapes)                      # smaller than the widest halo
    assert any(h == th + 1 and w == tw + 1 for _, h, w, _ in shapes)
    assert any(h % th == 0 and w % tw == 0 and h > th and w > tw for _, h, w, _ in shapes)
    assert {c for *_, c in shapes} >= {1, 3, 4} and {b for b, *_ in shapes} >= {1, chunk, chunk + 1}


def _frames(shape, seed):
    """Uniform values in [0, 255] with exact zeros and exact 255s sprinkled in."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 255, shape).astype(np.float32)
    pick = rng.uniform(size=shape)
    x[pick < 0.05] = 0.0
    x[pick > 0.95] = 255.0
    return x


def _rects(H, W, which):
    """Erase rectangles in pixels: the four borders (full columns / rows), a single pixel, an empty one, overlapping ones."""
    if which == "borders":
        return [(0, 1, 0, H, (1.0, 2.0, 3.0, 4.0)), (W - 1, W, 0, H, (5.0, 6.0, 7.0, 8.0)), (0, W, 0, 1, (9.0, 10.0, 11.0, 12.0)),
                (0, W, H - 1, H, (250.0, 251.0, 252.0, 253.0))]
    if which == "pixel":
        return [(W // 2, W // 2 + 1, H // 2, H // 2 + 1, (77.0, 78.0, 79.0, 80.0)), (1, 1, 0, H, (1.0,) * 4),
                (0, W, 0, H // 2, (20.0, 21.0, 22.0, 23.0)), (0, W // 2 + 1, 0, H // 2 + 1, (0.5, 128.25, 255.0, 3.0))]
    return []


# point-wise configurations (blur off): name -> restatement arguments without key / view / rects
POINTWISE = [
    dict(),                                                                         # neutral: the bit copy
    dict(haze=0.6, airlight=(200.0, 180.0, 160.0, 140.0)),
    dict(noise=15.0),
    dict(noise=300.0),                                                              # clamps at both ends
    dict(rects="borders"),
    dict(off=True),
    dict(haze=1.0, airlight=(0.0, 255.0, 17.5, 3.0), noise=40.0, rects="pixel"),
    dict(haze=0.013, noise=0.001, rects="pixel"),
]
BLURRED = [
    dict(sigma=0.3), dict(sigma=5.0), dict(), dict(sigma=1.0, noise=25.0), dict(sigma=2.2, noise=20.0, rects="borders"),
    dict(sigma=5.0, rects="pixel"), dict(sigma=1.0 / 3.0), dict(sigma=3.0, off=True), dict(sigma=4.99, noise=3.0),
]


def _sample(cfg, b, H, W):
    """-> (CameraCorruption, restatement keyword arguments) of sample b."""
    from dpft_amd.data.corrupt import CameraCorruption
    rects = _rects(H, W, cfg.get("rects"))
    kw = {k: v for k, v in cfg.items() if k != "rects"}
    key = (KEY + 0x9E3779B97F4A7C15 * b) & (2 ** 64 - 1)
    p = CameraCorruption(blur=kw.get("sigma", 0.0), haze=kw.get("haze", 0.0), airlight=kw.get("airlight", 200.0),
                         noise=kw.get("noise", 0.0), off=kw.get("off", False), key=key,
                         erase=[(x0 / W, x1 / W, y0 / H, y1 / H, fill) for x0, x1, y0, y1, fill in rects])
    return p, dict(kw, rects=rects, key=key)


def _launch(x, params, view):
    from dpft_amd.data.corrupt import corrupt_camera
    dx = torch.from_numpy(x).to(DEV)
    out = corrupt_camera(dx, params, view=view)
    torch.cuda.synchronize()
    assert out is not dx and torch.equal(dx.cpu(), torch.from_numpy(x))             # out of place: the input is left as it is
    return out.cpu().numpy()


@pytest.mark.parametrize("i", range(5))
def test_camera_point_wise_chain_is_the_restatement_bit_for_bit(i):
    shape = _shapes()[i]
    B, H, W, Ch = shape
    x = _frames(shape, 10 + i)
    made = [_sample(POINTWISE[(b + 3 * i) % len(POINTWISE)], b, H, W) for b in range(B)]
    if B >= len(POINTWISE):
        assert any(p.neutral for p, _ in made) and any(p.off for p, _ in made)
    if all(p.neutral for p, _ in made):
        pytest.fail("the cases of this shape launch nothing")
    got = _launch(x, [p for p, _ in made], view=i % 2)
    for b, (p, kw) in enumerate(made):
        want = R.camera(x[b], view=i % 2, **kw)
        assert want.dtype == np.float32
        assert np.array_equal(got[b].view(np.int32), want.view(np.int32)), (shape, b, kw)
        if p.neutral:
            assert np.array_equal(got[b].view(np.int32), x[b].view(np.int32))
        if kw.get("noise", 0) >= 300 and not kw.get("off"):
            assert (got[b] == 0).any() and (got[b] == 255).any() and not np.array_equal(got[b], x[b])


@pytest.mark.parametrize("i", range(5))
def test_camera_blur_is_within_the_rounding_bound_of_fp64(i):
    shape = _shapes()[i]
    B, H, W, Ch = shape
    x = _frames(shape, 20 + i)
    made = [_sample(BLURRED[(b + 2 * i + 1) % len(BLURRED)], b, H, W) for b in range(B)]
    assert any(p.blur > 0 for p, _ in made)
    got = _launch(x, [p for p, _ in made], view=0)
    worst = 0.0
    for b, (p, kw) in enumerate(made):
        if p.blur == 0 or p.off:                                                    # the neutral / off sample riding in the launch
            want = R.camera(x[b], **{k: v for k, v in kw.items() if k != "sigma"})
            assert np.array_equal(got[b].view(np.int32), want.view(np.int32)), (shape, b)
            continue
        Rr = R.radius(kw["sigma"])
        bound = 2 * (2 * Rr + 2) * 2.0 ** -24 * 255
        want = R.camera(x[b], dtype=np.float64, **kw)
        err = np.abs(got[b].astype(np.float64) - want)
        if kw["rects"]:                                                             # erased pixels hold the fill exactly
            x0, x1, y0, y1, fill = kw["rects"][-1]                                  # (the last one: nothing overwrites it)
            assert np.array_equal(got[b][y0:y1, x0:x1], np.broadcast_to(np.float32(fill[:Ch]), (y1 - y0, x1 - x0, Ch)))
        worst = max(worst, float(err.max() / bound))
        assert err.max() <= bound, (shape, b, kw["sigma"], float(err.max() / bound))
        assert not np.array_equal(got[b], x[b])
    print(f"shape {shape}: largest error / bound {worst:.3f}")


def test_camera_blur_radius_one_and_fifteen_in_one_launch_keep_a_constant():
    th, tw, _, _ = _limits()
    from dpft_amd.data.corrupt import CameraCorruption
    x = np.full((3, th + 3, tw + 3, 3), 200.0, dtype=np.float32)
    got = _launch(x, [CameraCorruption(blur=0.3), CameraCorruption(blur=5.0), CameraCorruption()], view=0)
    for b, Rr in enumerate((1, 15)):
        assert np.abs(got[b].astype(np.float64) - 200.0).max() <= 2 * (2 * Rr + 2) * 2.0 ** -24 * 255
    assert np.array_equal(got[2], x[2])


def _radar_case(shape, seed):
    B, H, W, Ch = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(-20.0, 270.0, shape).astype(np.float32)
    cases = [dict(noise=8.0, channels=[0, 3, 5]), dict(azimuth=[(0, 5), (W - 3, W), (40, 40)], rows=[(0, 2), (H - 1, H)]),
             dict(off=True), dict(noise=100.0, azimuth=[(0, 1)], rows=[(H // 2, H // 2)]), dict()]
    return x, [cases[(b + seed) % len(cases)] for b in range(B)]


@pytest.mark.parametrize("shape,lo,hi", [((2, 9, 107, 6), 0.0, 255.0), ((3, 37, 107, 6), -10.0, 200.0),
                                         ((9, 9, 107, 6), 0.0, 255.0)])
def test_radar_is_the_restatement_bit_for_bit(shape, lo, hi):
    from dpft_amd.data.corrupt import RadarCorruption, corrupt_radar
    B, H, W, Ch = shape
    x, cases = _radar_case(shape, 3 + B)
    dx = torch.from_numpy(x).to(DEV)
    for rows_are_range, view in ((True, 2), (False, 3)):
        params = [RadarCorruption(noise=c.get("noise", 0.0), channels=c.get("channels"), off=c.get("off", False), key=KEY + b,
                                  azimuth=[(a0 / W, a1 / W) for a0, a1 in c.get("azimuth", [])],
                                  rows=[(r0 / H, r1 / H) for r0, r1 in c.get("rows", [])]) for b, c in enumerate(cases)]
        out = corrupt_radar(dx, params, lo, hi, rows_are_range=rows_are_range, view=view)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert torch.equal(dx.cpu(), torch.from_numpy(x))
        for b, c in enumerate(cases):
            kw = dict(c, key=KEY + b, view=view, lo=lo, hi=hi)
            if not rows_are_range:
                kw["rows"] = []
            want = R.radar(x[b], **kw)
            assert np.array_equal(got[b].view(np.int32), want.view(np.int32)), (shape, b, c, rows_are_range)
            if len(c.get("azimuth", [])) == 3:                                      # columns 0 and W - 1 are inside bands
                assert (got[b][:, 0] == np.float32(lo)).all() and (got[b][:, W - 1] == np.float32(lo)).all()
                assert np.array_equal(got[b][2:H - 1, 5:W - 3], x[b][2:H - 1, 5:W - 3])


def test_all_neutral_batch_launches_nothing():
    from dpft_amd.data.corrupt import CameraCorruption, RadarCorruption, corrupt_camera, corrupt_radar
    x = torch.rand(2, 4, 6, 3, device=DEV)
    assert corrupt_camera(x, [CameraCorruption(), CameraCorruption()]) is x
    assert corrupt_radar(x, [RadarCorruption(rows=[(0, 1)])] * 2, rows_are_range=False) is x


def test_refusals_return_an_error_and_launch_nothing():
    from dpft_amd.data.corrupt import CameraCorruption, RadarCorruption, pack_camera, pack_radar
    from dpft_amd.hip.lib import HipLibraryError, lib, ptr, stream
    x = torch.rand(1, 8, 8, 3, device=DEV) * 255
    y = torch.full_like(x, -7.0)
    x5 = torch.rand(1, 8, 8, 5, device=DEV)
    y5 = torch.full_like(x5, -7.0)

    def cam(samples, src=x, dst=y, Ch=3):
        lib.call("dpft_corrupt_camera_nhwc_f32", ptr(src), ptr(dst), 1, 8, 8, Ch, samples, stream())
    bads = []
    for field, value in (("sigma", 5.5), ("haze", 1.5), ("haze", float("nan")), ("noise", float("nan")), ("sigma", float("nan"))):
        s = pack_camera([CameraCorruption(blur=1.0, haze=0.5, noise=2.0)], 8, 8)
        setattr(s[0], field, value)
        bads.append(s)
    s = pack_camera([CameraCorruption(erase=[(0, 1, 0, 1)])], 8, 8)
    s[0].rect[0][3] = 9
    bads.append(s)
    for s in bads:
        with pytest.raises(HipLibraryError):
            cam(s)
    ok = pack_camera([CameraCorruption(blur=1.0)], 8, 8)
    with pytest.raises(HipLibraryError, match="at most 4 channels"):
        cam(ok, x5, y5, 5)
    with pytest.raises(HipLibraryError, match="aliased"):
        cam(ok, x, x)
    with pytest.raises(HipLibraryError, match="null"):
        lib.call("dpft_corrupt_camera_nhwc_f32", None, ptr(y), 1, 8, 8, 3, ok, stream())
    r = pack_radar([RadarCorruption(azimuth=[(0, 1)])], 8, 8)
    r[0].azimuth[0][1] = 9
    with pytest.raises(HipLibraryError, match="azimuth band"):
        lib.call("dpft_corrupt_radar_nhwc_f32", ptr(x), ptr(y), 1, 8, 8, 3, 0.0, 255.0, r, stream())
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((y5 == -7.0).all())                     # nothing was written
    cam(ok)                                                                         # and the same call with good parameters writes
    torch.cuda.synchronize()
    assert not bool((y == -7.0).any())

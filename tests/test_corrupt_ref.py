"""Properties of the numpy restatement of the sensor degradation (tests/corrupt_ref.py) and of its host side
(dpft_amd/data/corrupt.py): weights, noise statistics, masks, parsing and the sampler.  No GPU."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from tests import corrupt_ref as R

KEY = 0x1234_5678_9ABC_DEF0


def test_radius_is_ceil_3_sigma_in_double():
    """R is evaluated in double precision on the double sigma: 3 * (1/3) is exactly 1 there (R = 1); the next float32 above
    1/3 gives R = 2.  (The next DOUBLE above 1/3 times 3 is 1 + 2^-53, a tie that rounds back to 1: R = 1 -- the restatement
    and the package must agree there too, which the loop below checks.)  The launch takes R from the caller, it never
    recomputes it from the float32 sigma."""
    third = 1.0 / 3.0
    above32 = float(np.nextafter(np.float32(third), np.float32(1.0)))
    assert above32 > third and R.radius(third) == 1 and R.radius(above32) == 2
    assert R.radius(float(np.float32(third))) == 2      # float32(1/3) lies above 1/3
    assert R.radius(5.0) == 15 and R.radius(0.3) == 1 and R.radius(0.0) == 0
    from dpft_amd.data.corrupt import blur_radius, blur_weights
    for s in (third, above32, float(np.nextafter(third, 1.0)), 0.3, 1.0, 2.5, 5.0):
        assert blur_radius(s) == R.radius(s)
        assert np.array_equal(blur_weights(s), R.weights(s)), s      # the package packs the restatement's table, bit for bit


@pytest.mark.parametrize("sigma", [0.3, 1.0 / 3.0, 1.0, 2.0, 3.0, 5.0])
def test_weights_sum_to_one_and_keep_a_constant(sigma):
    w = R.weights(sigma)
    Rr = len(w) - 1
    assert w.dtype == np.float32 and Rr == R.radius(sigma) and np.all(w[:-1] >= w[1:]) and np.all(w >= 0)
    total = float(w[0].astype(np.float64) + 2.0 * w[1:].astype(np.float64).sum())
    assert abs(total - 1.0) < 1e-7, total
    img = np.full((9, 11, 3), 200.0, dtype=np.float32)
    out = R.blur64(img, w)
    assert np.abs(out - 200.0).max() <= 2 * (2 * Rr + 2) * 2.0 ** -24 * 255


def test_blur_replicates_the_border_and_is_separable():
    """A horizontal ramp is kept in the interior (symmetric weights) and pulled towards the border value at the border; a
    frame smaller than the halo still works."""
    w = R.weights(1.0)
    ramp = np.tile(np.arange(16, dtype=np.float32)[None, :, None], (6, 1, 2))
    out = R.blur64(ramp, w)
    assert np.abs(out[:, 3:13] - ramp[:, 3:13]).max() < 1e-6
    assert out[0, 0, 0] > 0 and out[0, 15, 0] < 15
    tiny = np.arange(2 * 3 * 1, dtype=np.float32).reshape(2, 3, 1)
    assert R.blur64(tiny, R.weights(5.0)).shape == tiny.shape
    imp = np.zeros((31, 31, 1), dtype=np.float32)
    imp[15, 15] = 1.0
    full = np.concatenate([w[:0:-1], w]).astype(np.float64)
    assert np.abs(R.blur64(imp, w)[12:19, 12:19, 0] - np.outer(full, full)).max() < 1e-15


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def test_noise_statistics():
    """2^20 elements of one sample laid out as (H, W, C) = (512, 512, 4).  The standard error of a mean or a correlation over
    2^20 unit-variance values is 2^-10: the bounds below are 5 and 10 of them.  Irwin-Hall of order 4 has kurtosis 3 - 6/20."""
    n = 1 << 20
    u = R.uniforms16(KEY, 0, n)
    assert u.min() >= 0 and u.max() <= 0xFFFF
    z32 = R.noise_z(KEY, 0, n)
    assert z32.dtype == np.float32 and float(np.abs(z32).max()) < 3.47
    z = z32.astype(np.float64)
    mean, std = float(z.mean()), float(z.std())
    kurt = float(((z - mean) ** 4).mean() / std ** 4)
    c = 4
    lag_c = _corr(z[:-1], z[1:])                       # the next channel (or the next pixel's first)
    lag_x = _corr(z[:-c], z[c:])                       # the same channel of the next pixel
    other_sample = _corr(z, R.noise_z(KEY + 1, 0, n).astype(np.float64))
    other_view = _corr(z, R.noise_z(KEY, 1, n).astype(np.float64))
    other_seed = _corr(z, R.noise_z(KEY ^ (0xABCDEF << 32), 0, n).astype(np.float64))
    print(f"mean {mean:.4f} std {std:.4f} kurtosis {kurt:.3f} lag-1 c {lag_c:.4f} x {lag_x:.4f} "
          f"sample {other_sample:.4f} view {other_view:.4f} seed {other_seed:.4f}")
    assert abs(mean) < 5 / 1024
    assert abs(std - 1) < 0.01
    assert abs(lag_c) < 0.01 and abs(lag_x) < 0.01
    assert abs(other_sample) < 0.01 and abs(other_seed) < 0.01 and abs(other_view) < 0.01
    assert abs(kurt - 2.7) < 0.05
    # a pure function: a prefix of a longer draw is the shorter draw
    assert np.array_equal(R.noise_z(KEY, 0, 1000), z32[:1000])


def test_point_wise_chain_roundings():
    """haze and noise round every operation separately in float32; the clamp acts only with noise on."""
    img = np.array([[[0.0, 255.0, 100.3]], [[254.9, 0.2, 17.0]]], dtype=np.float32)
    out = R.camera(img, haze=0.6, airlight=(200.0, 180.0, 160.0, 0.0))
    f, A = np.float32(0.6), np.array([200.0, 180.0, 160.0], dtype=np.float32)
    assert np.array_equal(out, img + f * (A - img)) and out.dtype == np.float32
    big = np.random.default_rng(2).uniform(0, 255, (16, 16, 3)).astype(np.float32)
    loud = R.camera(big, noise=200.0, key=KEY)
    assert loud.min() >= 0 and loud.max() <= 255 and (loud == 0).any() and (loud == 255).any()
    assert np.array_equal(R.camera(img), img)
    assert not R.camera(img, off=True).any()
    erased = R.camera(img, rects=[(0, 1, 1, 2, (7.0, 8.0, 9.0, 10.0))])
    assert erased[1, 0].tolist() == [7.0, 8.0, 9.0] and np.array_equal(erased[0], img[0])


def test_azimuth_bands_are_the_same_columns_in_both_radar_views():
    from dpft_amd.data.corrupt import RadarCorruption, pack_radar
    p = [RadarCorruption(azimuth=[(0.4, 0.6), {"u": 0.999, "bins": 12}, {"u": 0.0, "bins": 1}], rows=[(0.0, 0.25)], key=KEY)]
    bev = pack_radar(p, 256, 107, view=2, rows_are_range=True)[0]
    front = pack_radar(p, 37, 107, view=3, rows_are_range=False)[0]
    assert bev.n_azimuth == front.n_azimuth == 3
    az = [[tuple(a.azimuth[j]) for j in range(3)] for a in (bev, front)]
    assert az[0] == az[1] == [(43, 64), (95, 107), (0, 1)]
    assert bev.n_rows == 1 and tuple(bev.rows[0]) == (0, 64) and front.n_rows == 0      # range bands: the BEV map only
    assert bev.key == front.key == KEY and (bev.view, front.view) == (2, 3) and bev.channels == 0xFFFFFFFF
    x = np.random.default_rng(0).uniform(0, 255, (37, 107, 6)).astype(np.float32)
    out = R.radar(x, azimuth=az[1])
    assert not out[:, 43:64].any() and not out[:, 95:].any() and not out[:, 0].any()
    keep = np.ones(107, bool)
    keep[43:64] = keep[95:] = keep[0] = False
    assert np.array_equal(out[:, keep], x[:, keep])


def test_radar_noise_acts_on_the_selected_channels_only():
    x = np.random.default_rng(1).uniform(0, 255, (9, 107, 6)).astype(np.float32)
    out = R.radar(x, noise=10.0, channels=[1, 4], key=KEY, view=2, lo=-5.0, hi=250.0)
    assert np.array_equal(out[..., [0, 2, 3, 5]], x[..., [0, 2, 3, 5]])
    assert not np.array_equal(out[..., 1], x[..., 1]) and out[..., [1, 4]].max() <= 250.0


FULL = {"p": 0.5,
        "camera": {"blur": [0, 3], "haze": [0, 0.6], "noise": [0, 20],
                   "erase": {"n": [0, 3], "area": [0.02, 0.2], "aspect": [0.3, 3.3]}, "off": 0.05},
        "radar": {"noise": [0, 10], "azimuth_mask": {"n": [0, 2], "width": [1, 12]},
                  "range_mask": {"n": [0, 2], "width": [1, 24]}, "off": 0.05},
        "seed": None}


def _with(path, value):
    spec = copy.deepcopy(FULL)
    d = spec
    for k in path[:-1]:
        d = d[k]
    d[path[-1]] = value
    return spec


def test_parse_corrupt_accepts_the_documented_form():
    from dpft_amd.data.corrupt import parse_corrupt
    spec = parse_corrupt(FULL)
    assert spec["p"] == 0.5 and spec["camera"]["blur"] == (0.0, 3.0) and spec["camera"]["erase"]["n"] == (0, 3)
    assert spec["radar"]["azimuth_mask"] == {"n": (0, 2), "width": (1, 12)} and spec["seed"] is None
    off = parse_corrupt({})
    assert off["camera"]["blur"] == (0.0, 0.0) and off["camera"]["off"] == 0.0 and off["radar"]["range_mask"]["n"] == (0, 0)


@pytest.mark.parametrize("bad", [
    None, True, [], "fog", {"q": 1}, _with(("p",), 1.5), _with(("p",), "x"), _with(("p",), True), _with(("seed",), 1.5),
    _with(("camera",), []), _with(("camera", "fog"), 1), _with(("camera", "blur"), 3), _with(("camera", "blur"), [0, 5.5]),
    _with(("camera", "blur"), [2, 1]), _with(("camera", "blur"), [0, float("nan")]), _with(("camera", "haze"), [0, 1.2]),
    _with(("camera", "haze"), [-0.1, 0.5]), _with(("camera", "noise"), [0, -1]), _with(("camera", "noise"), [0]),
    _with(("camera", "erase"), 3), _with(("camera", "erase", "n"), [0, 5]), _with(("camera", "erase", "n"), [0, 1.5]),
    _with(("camera", "erase", "area"), [0, 1.5]), _with(("camera", "erase", "aspect"), [0, 1]),
    _with(("camera", "erase", "shape"), 1), _with(("camera", "off"), 2), _with(("camera", "off"), [0.1]),
    _with(("camera", "airlight"), 300), _with(("camera", "airlight"), [1, 2, 3, 4, 5]),
    _with(("radar",), 1), _with(("radar", "gain"), 1), _with(("radar", "noise"), 10),
    _with(("radar", "azimuth_mask"), [[0.1, 0.2]]), _with(("radar", "azimuth_mask", "n"), [0, 9]),
    _with(("radar", "azimuth_mask", "width"), [0, 3]), _with(("radar", "range_mask", "width"), [4, 2]),
    _with(("radar", "off"), -0.1), _with(("radar", "off"), 0.96), _with(("radar", "channels"), [6.5]),
    _with(("radar", "channels"), []),
])
def test_parse_corrupt_refuses_malformed_forms(bad):
    from dpft_amd.data.corrupt import parse_corrupt
    with pytest.raises(ValueError, match="train.corrupt"):
        parse_corrupt(bad)


def test_parameters_refuse_what_the_launch_refuses():
    from dpft_amd.data.corrupt import CameraCorruption, RadarCorruption
    for kw in (dict(blur=5.1), dict(blur=float("nan")), dict(haze=1.1), dict(haze=-0.1), dict(noise=-1.0),
               dict(noise=float("nan")), dict(erase=[(0.5, 0.4, 0, 1)]), dict(erase=[(0, 1.1, 0, 1)]),
               dict(erase=[(0, 1, 0, 1)] * 5)):
        with pytest.raises(ValueError):
            CameraCorruption(**kw)
    for kw in (dict(noise=float("inf")), dict(azimuth=[(0.6, 0.4)]), dict(rows=[(0, 1.5)]), dict(azimuth=[(0, 1)] * 5),
               dict(azimuth=[{"u": 1.0, "bins": 2}])):
        with pytest.raises(ValueError):
            RadarCorruption(**kw)
    assert CameraCorruption().neutral and RadarCorruption().neutral and not CameraCorruption(off=True).neutral
    assert RadarCorruption(rows=[(0, 0.5)]).neutral_for(False) and not RadarCorruption(rows=[(0, 0.5)]).neutral_for(True)


def test_pack_camera_lays_out_what_the_header_declares():
    from dpft_amd.data.corrupt import CameraCorruption, pack_camera
    from dpft_amd.hip.lib import CorruptCamera, CorruptRadar
    assert C.sizeof(CorruptCamera) == 248 and C.sizeof(CorruptRadar) == 104
    p = CameraCorruption(blur=1.0, haze=0.25, airlight=[10, 20, 30], noise=3.0, key=KEY,
                         erase=[(0.0, 1 / 7, 4 / 5, 1.0, (1.0, 2.0, 3.0))])
    a = pack_camera([p, CameraCorruption()], 5, 7, view=1)
    assert a[0].radius == 3 and np.array_equal(np.array(a[0].w[:4], dtype=np.float32), R.weights(1.0)) and a[0].w[4] == 0
    assert (a[0].key, a[0].view, a[0].haze, a[0].noise, a[0].n_rects, a[0].off) == (KEY, 1, 0.25, 3.0, 1, 0)
    assert list(a[0].airlight) == [10.0, 20.0, 30.0, 30.0] and list(a[0].rect[0]) == [0, 1, 4, 5]
    assert list(a[0].fill[0]) == [1.0, 2.0, 3.0, 3.0]
    assert (a[1].radius, a[1].sigma, a[1].haze, a[1].noise, a[1].n_rects, a[1].off) == (0, 0.0, 0.0, 0.0, 0, 0)


def test_limits_and_refusals_without_a_launch():
    """Argument validation happens before any launch: host code."""
    from dpft_amd.data.corrupt import CameraCorruption, RadarCorruption, pack_camera, pack_radar
    from dpft_amd.hip.lib import CORRUPT_CHUNK, CORRUPT_MAX_RADIUS, lib
    out = (C.c_int32 * 4)()
    assert lib.dpft_corrupt_limits(out) == 0 and out[2] == CORRUPT_MAX_RADIUS == 15 and out[3] == CORRUPT_CHUNK
    assert out[0] > 0 and out[1] > 0
    assert lib.dpft_corrupt_limits(None) == -1 and b"corrupt_limits: null output" in lib.dpft_last_error()
    src, dst = C.c_void_p(4096), C.c_void_p(8192)
    ok = pack_camera([CameraCorruption(blur=1.0, haze=0.5)], 8, 8)
    cam = lib.dpft_corrupt_camera_nhwc_f32

    def refused(samples, word, s=src, d=dst, B=1, H=8, W=8, Ch=3):
        assert cam(s, d, B, H, W, Ch, samples, None) == -1
        assert word in lib.dpft_last_error(), lib.dpft_last_error()
    refused(ok, b"null", s=None)
    refused(ok, b"null", d=None)
    refused(None, b"null sample")
    refused(ok, b"aliased", d=src)
    refused(ok, b"at most 4 channels", Ch=5)
    refused(ok, b"non-positive", H=0)
    for field, value, word in (("sigma", 5.5, b"sigma"), ("sigma", float("nan"), b"sigma"), ("haze", 1.5, b"haze"),
                               ("haze", -0.1, b"haze"), ("haze", float("nan"), b"haze"), ("noise", float("nan"), b"noise"),
                               ("noise", -1.0, b"noise"), ("radius", 16, b"radius"), ("radius", 0, b"radius"),
                               ("n_rects", 5, b"rectangles")):
        bad = pack_camera([CameraCorruption(blur=1.0, haze=0.5)], 8, 8)
        setattr(bad[0], field, value)
        refused(bad, word)
    bad = pack_camera([CameraCorruption(blur=1.0)], 8, 8)
    bad[0].w[0] = 0.5
    refused(bad, b"add up to 1")
    bad = pack_camera([CameraCorruption(erase=[(0, 1, 0, 1)])], 8, 8)
    bad[0].rect[0][1] = 9
    refused(bad, b"leaves the 8 x 8 frame")
    bad[0].rect[0][1], bad[0].rect[0][2] = 8, -1
    refused(bad, b"leaves the 8 x 8 frame")
    rad = lib.dpft_corrupt_radar_nhwc_f32
    okr = pack_radar([RadarCorruption(noise=1.0, azimuth=[(0, 0.5)])], 4, 8)
    for args, word in (((None, dst, 1, 4, 8, 6, 0.0, 255.0, okr, None), b"null"),
                       ((src, src, 1, 4, 8, 6, 0.0, 255.0, okr, None), b"aliased"),
                       ((src, dst, 1, 4, 8, 6, 0.0, 255.0, None, None), b"null sample"),
                       ((src, dst, 1, 4, 8, 6, 1.0, 0.0, okr, None), b"ordered"),
                       ((src, dst, 1, 4, 8, 6, 0.0, float("nan"), okr, None), b"ordered"),
                       ((src, dst, 1, 4, 3, 6, 0.0, 255.0, okr, None), b"azimuth band 0")):
        assert rad(*args) == -1 and word in lib.dpft_last_error(), (word, lib.dpft_last_error())
    okr[0].noise = float("nan")
    assert rad(src, dst, 1, 4, 8, 6, 0.0, 255.0, okr, None) == -1 and b"noise" in lib.dpft_last_error()
    okr = pack_radar([RadarCorruption(rows=[(0, 1)])], 4, 8)
    assert rad(src, dst, 1, 3, 8, 6, 0.0, 255.0, okr, None) == -1 and b"row band 0" in lib.dpft_last_error()


def test_sampler_is_reproducible_from_its_four_numbers():
    from dpft_amd.data.corrupt import N_DRAWS, CorruptSampler, parse_corrupt
    spec = parse_corrupt(dict(FULL, p=1.0))

    def draws(seed, rank, epoch, ordinal):
        s = CorruptSampler(spec, seed=seed, rank=rank)
        s.set_epoch(epoch)
        for _ in range(ordinal):
            s.draw(3)
        cams, rads = s.draw(3)
        return [(c.blur, c.haze, c.noise, tuple(c.erase), c.off, c.key) for c in cams] + \
               [(r.noise, str(r.azimuth), str(r.rows), r.off, r.key) for r in rads]
    base = draws(7, 1, 2, 3)
    assert base == draws(7, 1, 2, 3)
    for other in ((8, 1, 2, 3), (7, 0, 2, 3), (7, 1, 3, 3), (7, 1, 2, 4)):
        assert draws(*other) != base, other
    s = CorruptSampler(spec, seed=7)
    assert s.uniforms(5).shape == (5, N_DRAWS)
    assert CorruptSampler(parse_corrupt(dict(FULL, seed=11)), seed=7).seed == 11
    # samples of one batch carry different noise keys; ranges are honoured
    cams, rads = CorruptSampler(spec, seed=1).draw(64)
    assert len({c.key for c in cams}) == 64 and [c.key for c in cams] == [r.key for r in rads]
    live = [c for c in cams if not c.off]
    assert all(0 <= c.blur <= 3 and 0 <= c.haze <= 0.6 and 0 <= c.noise <= 20 and len(c.erase) <= 3 for c in live)
    assert any(len(c.erase) == 3 for c in live) and any(len(c.erase) == 0 for c in live)
    for c in live:
        for x0, x1, y0, y1, fill in c.erase:
            assert 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1 and 0.019 < (x1 - x0) * (y1 - y0) < 0.201
    assert all(len(r.azimuth) <= 2 and len(r.rows) <= 2 and all(1 <= b["bins"] <= 12 for b in r.azimuth) and
               all(1 <= b["bins"] <= 24 for b in r.rows) for r in rads)


def test_sampler_p_and_the_off_lottery():
    from dpft_amd.data.corrupt import CorruptSampler, parse_corrupt
    cams, rads = CorruptSampler(parse_corrupt(dict(FULL, p=0.0)), seed=3).draw(32)
    assert all(c.neutral for c in cams) and all(r.neutral for r in rads)
    spec = parse_corrupt({"p": 1.0, "camera": {"off": 0.5}, "radar": {"off": 0.5}})
    cams, rads = CorruptSampler(spec, seed=3).draw(256)
    both = sum(c.off and r.off for c, r in zip(cams, rads))
    assert both == 0 and sum(c.off for c in cams) + sum(r.off for r in rads) == 256
    assert 64 < sum(c.off for c in cams) < 192
    half = CorruptSampler(parse_corrupt(dict(FULL, p=0.5)), seed=3).draw(256)[0]
    assert 64 < sum(c.neutral for c in half) < 192


def test_augmentation_draws_do_not_move_with_a_corrupt_sampler_beside_them():
    import torch
    from dpft_amd.data import GpuPreprocessor
    from dpft_amd.data.augment import AugmentSampler, parse_augment
    aug = {"flip": 0.5, "camera": {"zoom": [0.9, 1.1]}, "seed": 5}
    alone = AugmentSampler(parse_augment(aug), seed=2, rank=1)
    pre = GpuPreprocessor(augment=aug, corrupt=dict(FULL, p=1.0), seed=2, rank=1)
    assert pre.augments and pre.corrupts
    for epoch in (0, 1):
        alone.set_epoch(epoch)
        pre.set_epoch(epoch)
        for _ in range(3):
            pre.corruptor.draw(4)                      # interleaved as the preprocessor interleaves them
            assert torch.equal(pre.sampler.uniforms(4), alone.uniforms(4))
    assert not GpuPreprocessor(augment=aug).corrupts and GpuPreprocessor().corruptor is None


def test_from_config_takes_the_key_for_the_training_loader_only():
    from dpft_amd.configs import load_config
    from dpft_amd.data import GpuPreprocessor
    cfg = copy.deepcopy(load_config("kradar"))
    assert "corrupt" not in cfg["train"] and not GpuPreprocessor.from_config(cfg, augment=True).corrupts
    cfg["train"]["corrupt"] = dict(FULL)
    assert GpuPreprocessor.from_config(cfg, augment=True).corrupts
    assert not GpuPreprocessor.from_config(cfg).corrupts and not GpuPreprocessor.from_config(cfg, augment=False).augments
    cfg["train"]["corrupt"] = {"p": 2}
    with pytest.raises(ValueError, match="train.corrupt"):
        GpuPreprocessor.from_config(cfg, augment=True)
    GpuPreprocessor.from_config(cfg)                   # an evaluation preprocessor does not even parse it
    assert math.isfinite(cfg["train"]["corrupt"]["p"])

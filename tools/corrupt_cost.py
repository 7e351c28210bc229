"""Cost of the sensor degradation launches (dpft_amd/csrc/corrupt.hip) at batch 4 of the model's input sizes: the camera frame
512x910x3 after its resize, the scaled radar maps 256x107x6 and 37x107x6.

    python tools/corrupt_cost.py [--runs 200] [--out profiles/corrupt.txt]

Medians of ``--runs`` runs between device events (the host's issue time included), all in one process; the launches are
called with parameters packed beforehand and a standing output, so their rows are the launch, not the Python around it:
  * the camera launch at sigma = 0 (haze + noise: the point-wise chain only), 1, 3 and 5 (blur + haze + noise);
  * the radar launches (noise + one azimuth band + one range band on the BEV map, noise + the azimuth band on the front map);
  * the plain and the augmented preprocess of the same batch of raw frames, and the preprocess with ``train.corrupt``;
  * a ``torch`` copy of the camera tensor: the bandwidth yardstick (the launch reads and writes every float once, like a copy).
For every sigma the achieved fraction of the copy's rate is printed, beside the LDS reads per output float (both passes; a thread
carries RUN = 4 adjacent outputs through a pass: 2 (RUN + 2R) / RUN) and the floats staged per output float
((TH + 2R)(TW + 2R) / (TH TW)) that bound the blur.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dpft_amd.data import GpuPreprocessor, SyntheticRawDataset, listed_collating      # noqa: E402
from dpft_amd.data.corrupt import (CameraCorruption, RadarCorruption, blur_radius, corrupt_camera,      # noqa: E402
                                   pack_camera, pack_radar)
from dpft_amd.hip.lib import lib, ptr, stream                                         # noqa: E402

RUN = 4      # kRun of csrc/corrupt.hip
AUGMENT = {"flip": 0.5, "camera": {"zoom": [0.9, 1.1], "shift": 0.05, "brightness": 0.2, "contrast": 0.2, "channel": 0.05},
           "radar": {"gain_db": 3.0}, "seed": 0}
CORRUPT = {"p": 0.5,
           "camera": {"blur": [0, 3], "haze": [0, 0.6], "noise": [0, 20],
                      "erase": {"n": [0, 3], "area": [0.02, 0.2], "aspect": [0.3, 3.3]}, "off": 0.05},
           "radar": {"noise": [0, 10], "azimuth_mask": {"n": [0, 2], "width": [1, 12]},
                     "range_mask": {"n": [0, 2], "width": [1, 24]}, "off": 0.05}, "seed": 0}


def median_ms(fn, runs, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "corrupt.txt"))
    args = ap.parse_args()
    B = args.batch
    lim = (C.c_int32 * 4)()
    lib.call("dpft_corrupt_limits", lim)
    th, tw = lim[0], lim[1]
    g = torch.Generator(device="cuda").manual_seed(0)
    cam = torch.rand(B, 512, 910, 3, device="cuda", generator=g) * 255
    bev = torch.rand(B, 256, 107, 6, device="cuda", generator=g) * 255
    front = torch.rand(B, 37, 107, 6, device="cuda", generator=g) * 255
    dst = torch.empty_like(cam)
    lines = [f"corrupt_cost: batch {B}, camera 512x910x3 + radar 256x107x6 + 37x107x6 f32, {torch.cuda.get_device_name(0)}, median of "
             f"{args.runs} runs between device events"]
    t_copy = median_ms(lambda: dst.copy_(cam), args.runs)
    gbytes = 2 * cam.numel() * 4 / 1e9
    lines.append(f"torch copy of the camera tensor: {t_copy:.4f} ms ({gbytes / (t_copy * 1e-3):.0f} GB/s read + write)")
    for sigma in (0.0, 1.0, 3.0, 5.0):
        packed = pack_camera([CameraCorruption(blur=sigma, haze=0.4, noise=10.0, key=b) for b in range(B)], 512, 910)
        t = median_ms(lambda: lib.call("dpft_corrupt_camera_nhwc_f32", ptr(cam), ptr(dst), B, 512, 910, 3, packed, stream()),
                      args.runs)
        R = blur_radius(sigma)
        halo = (th + 2 * R) * (tw + 2 * R) / (th * tw)
        lines.append(f"camera launch, sigma {sigma:g} (R {R}) + haze + noise: {t:.4f} ms = {t_copy / t:.2f} of the copy's rate; "
                     f"{2 * (RUN + 2 * R) / RUN if R else 0:g} LDS reads per output float, {halo:.2f} floats staged per output float")
    rb = [RadarCorruption(noise=8.0, azimuth=[(0.4, 0.5)], rows=[(0.1, 0.2)], key=b) for b in range(B)]
    pb, pf = pack_radar(rb, 256, 107, 2, True), pack_radar(rb, 37, 107, 3, False)
    dbev, dfront = torch.empty_like(bev), torch.empty_like(front)
    t = median_ms(lambda: (lib.call("dpft_corrupt_radar_nhwc_f32", ptr(bev), ptr(dbev), B, 256, 107, 6, 0.0, 255.0, pb, stream()),
                           lib.call("dpft_corrupt_radar_nhwc_f32", ptr(front), ptr(dfront), B, 37, 107, 6, 0.0, 255.0, pf, stream())),
                  args.runs)
    lines.append(f"radar launches (both maps, noise + bands): {t:.4f} ms")
    one = [CameraCorruption(blur=3.0, haze=0.4, noise=10.0, key=b) for b in range(B)]
    lines.append(f"corrupt_camera() from Python at sigma 3 (packing the parameters and allocating the output included): "
                 f"{median_ms(lambda: corrupt_camera(cam, one), args.runs):.4f} ms")
    ds = SyntheticRawDataset(B, seed=1)
    host, labels = listed_collating([ds[i] for i in range(B)])
    batch = {k: v.cuda() for k, v in host.items()}
    labels = [{k: v.cuda() for k, v in l.items()} for l in labels]
    plain, aug = GpuPreprocessor(image_size=512), GpuPreprocessor(image_size=512, augment=AUGMENT)
    both, cor = GpuPreprocessor(image_size=512, augment=AUGMENT, corrupt=CORRUPT), GpuPreprocessor(image_size=512, corrupt=CORRUPT)
    lines.append(f"plain preprocess (raw 720x1280x3 u8 + both radar maps): {median_ms(lambda: plain(batch), args.runs):.4f} ms")
    lines.append(f"augmented preprocess: {median_ms(lambda: aug(batch, labels), args.runs):.4f} ms")
    lines.append(f"plain preprocess + train.corrupt (p = 0.5, the documented ranges; a new draw every run): "
                 f"{median_ms(lambda: cor(batch), args.runs):.4f} ms")
    lines.append(f"augmented preprocess + train.corrupt: {median_ms(lambda: both(batch, labels), args.runs):.4f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

"""Cost of the training augmentation on the upload stream: the augmenting GpuPreprocessor against the plain one, in one
process, on a batch of 4 raw K-Radar-sized samples (720x1280x3 u8 frame, 256x107x6 and 37x107x6 radar maps in dB).

    python tools/augment_cost.py [--runs 200] [--out profiles/augment.txt]

Medians of ``--runs`` runs between device events.  The structural claim is checked, not assumed: the number of native launches
per batch rises by exactly one (the geometry launch) -- the camera and radar launches REPLACE the resize and scaling launches.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dpft_amd.data import GpuPreprocessor, SyntheticRawDataset, listed_collating      # noqa: E402
from dpft_amd.hip.lib import lib                                                      # noqa: E402

FULL = {"flip": 0.5, "camera": {"zoom": [0.9, 1.1], "shift": 0.05, "brightness": 0.2, "contrast": 0.2, "channel": 0.05},
        "radar": {"gain_db": 3.0}, "seed": 0}


def count_launches(fn):
    calls = []
    real = lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    lib.call = counting
    try:
        fn()
    finally:
        del lib.call                      # back to the class's method
    return calls


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
    ap.add_argument("--out", default=os.path.join("profiles", "augment.txt"))
    args = ap.parse_args()
    ds = SyntheticRawDataset(args.batch, seed=1)
    host, labels = listed_collating([ds[i] for i in range(args.batch)])
    batch = {k: v.cuda() for k, v in host.items()}
    labels = [{k: v.cuda() for k, v in l.items()} for l in labels]
    plain = GpuPreprocessor(image_size=512)
    variants = [("flip only", GpuPreprocessor(image_size=512, augment={"flip": 0.5, "seed": 0})),
                ("flip + zoom/shift + photometric + radar gain", GpuPreprocessor(image_size=512, augment=FULL))]
    n_plain = count_launches(lambda: plain(batch))
    lines = [f"augment_cost: batch {args.batch}, raw 720x1280x3 u8 + 256x107x6 + 37x107x6 f32, {torch.cuda.get_device_name(0)}, "
             f"median of {args.runs} runs between device events",
             f"plain preprocess: {len(n_plain)} launches {sorted(set(n_plain))}",
             f"plain preprocess: {median_ms(lambda: plain(batch), args.runs):.4f} ms"]
    for name, pre in variants:
        n_aug = count_launches(lambda: pre(batch, labels))
        assert len(n_aug) == len(n_plain) + 1, (n_plain, n_aug)
        assert [n for n in n_aug if "geometry" in n] == ["dpft_augment_geometry_f32"]
        lines.append(f"augmented ({name}): {len(n_aug)} launches (+{len(n_aug) - len(n_plain)}: the geometry launch)")
        lines.append(f"augmented ({name}): {median_ms(lambda: pre(batch, labels), args.runs):.4f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

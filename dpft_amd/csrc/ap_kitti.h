// Score-threshold selection of the KITTI-protocol table (dpft_amd/evaluation/dataset_ap.py states the protocol;
// tests/dataset_ap_kitti_ref.py holds the literal loop).  Host and device: ap_finalize_kitti_kernel uses it on the device and
// dpft_dataset_ap_kitti_ranks on the host, where tests/test_dataset_ap_kitti_ref.py holds it to the literal loop.  The including
// file is built with -ffp-contract=off and the operations below keep the literal loop's order, so the ranks are the loop's also
// where (r - cur) == (cur - l) exactly.
#pragma once

#include <math.h>

constexpr int kApKittiPoints = 41;

// the literal loop's "continue" at rank i (0-based) out of n1 pass-1 TPs, G ground-truth boxes, sampling position cur
__host__ __device__ inline bool ap_kitti_skip(long long i, long long n1, double G, double cur) {
    const double l = (double)(i + 1) / G;
    const double r = (double)(i + 2) / G;
    return (r - cur) < (cur - l) && i < n1 - 1;
}

// ranks[t] = rank (in descending score order) of the pass-1 TP whose score is threshold t; returns their number (<= 41).
// The literal loop visits every rank; the skip predicate is (2 i + 3) / G < 2 cur up to rounding, monotone in i, so this one
// jumps to ceil(cur * G - 1.5) and settles on the boundary with the literal predicate: back while the rank before does not skip,
// forward while this one does (rank n1 - 1 never skips).
__host__ __device__ inline int ap_kitti_ranks(long long n1, long long npos, long long* ranks) {
    const double G = (double)npos;
    double cur = 0.0;
    long long i = 0;
    int nt = 0;
    while (i < n1 && nt < kApKittiPoints) {
        const double guess = ceil(cur * G - 1.5);
        long long j = i;
        if (guess > (double)i) j = guess < (double)(n1 - 1) ? (long long)guess : n1 - 1;
        while (j > i && !ap_kitti_skip(j - 1, n1, G, cur)) --j;
        while (ap_kitti_skip(j, n1, G, cur)) ++j;
        ranks[nt++] = j;
        cur += 1 / 40.0;
        i = j + 1;
    }
    return nt;
}

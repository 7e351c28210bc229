// fp64 yaw-box geometry shared by dataset_ap.hip and nms.hip (there is no relocatable device code in this build: both include
// it).  Boxes are (center, size, (sin, cos)) in fp32; the rotation is (sin, cos) / hypot in fp64 straight from the fp32 pair -- no
// atan2.  tests/dataset_ap_ref.py restates every function operation for operation; the including files are built with
// -ffp-contract=off, so a strict "IoU > threshold" decides as the restatement does.
#pragma once
#include "common.h"

namespace dpft {

struct ApP2 { double x, y; };

// first maximal entry; a NaN counts as the maximum (torch.max / numpy.argmax)
__device__ __forceinline__ int ap_argmax(const float* x, int n, float& best) {
    best = x[0];
    int arg = 0;
    for (int k = 1; k < n; ++k) {
        const float v = x[k];
        if (v > best || (v != v && best == best)) { best = v; arg = k; }
    }
    return arg;
}

__device__ inline double ap_poly_area(const ApP2* p, int n) {
    double a = 0;
    for (int i = 0; i < n; ++i) {
        const ApP2 u = p[i], v = p[(i + 1) % n];
        a += u.x * v.y - v.x * u.y;
    }
    return a / 2;
}

// corners (counter-clockwise) of a (center, size, (sin, cos)) box; false = invalid box
__device__ inline bool ap_corners(const float* ce, const float* sz, const float* an, ApP2* c) {
    const double l = sz[0], w = sz[1], h = sz[2], s = an[0], co = an[1];
    const double r = hypot(s, co);
    if (!(r > 0)) return false;
    if (!(fmin(fmin(l * w, l * h), w * h) / 2 > 1e-4)) return false;
    const double si = s / r, cs = co / r;
    const double sx[4] = {-1, 1, 1, -1}, sy[4] = {-1, -1, 1, 1};
    for (int i = 0; i < 4; ++i) {
        const double x = sx[i] * l / 2, y = sy[i] * w / 2;
        c[i].x = cs * x - si * y + (double)ce[0];
        c[i].y = si * x + cs * y + (double)ce[1];
    }
    if (ap_poly_area(c, 4) < 0) { const ApP2 t = c[1]; c[1] = c[3]; c[3] = t; }
    return true;
}

__device__ inline void ap_iou_pair(const float* ce1, const float* sz1, const float* an1, const float* ce2, const float* sz2,
                                   const float* an2, double& bev, double& vol3d) {
    bev = 0;
    vol3d = 0;
    ApP2 poly[10], tmp[10], Q[4];
    if (!ap_corners(ce1, sz1, an1, poly) || !ap_corners(ce2, sz2, an2, Q)) return;
    int n = 4;
    for (int e = 0; e < 4 && n > 0; ++e) {      // Sutherland-Hodgman: box 1 clipped by the half-planes of box 2
        const ApP2 a = Q[e], bb = Q[(e + 1) & 3];
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const ApP2 c = poly[k], d = poly[(k + 1) % n];
            const double sc = (bb.x - a.x) * (c.y - a.y) - (bb.y - a.y) * (c.x - a.x);
            const double sd = (bb.x - a.x) * (d.y - a.y) - (bb.y - a.y) * (d.x - a.x);
            if (sc >= 0) tmp[m++] = c;
            if ((sc >= 0) != (sd >= 0)) {
                const double t = sc / (sc - sd);
                tmp[m].x = c.x + t * (d.x - c.x);
                tmp[m].y = c.y + t * (d.y - c.y);
                ++m;
            }
        }
        n = m;
        for (int k = 0; k < n; ++k) poly[k] = tmp[k];
    }
    const double inter = n >= 3 ? fabs(ap_poly_area(poly, n)) : 0.0;
    const double l1 = sz1[0], w1 = sz1[1], h1 = sz1[2], l2 = sz2[0], w2 = sz2[1], h2 = sz2[2];
    const double a1 = l1 * w1, a2 = l2 * w2;
    if (inter > 0) bev = inter / (a1 + a2 - inter);
    const double z1 = ce1[2], z2 = ce2[2];
    const double zov = fmax(0.0, fmin(z1 + h1 / 2, z2 + h2 / 2) - fmax(z1 - h1 / 2, z2 - h2 / 2));
    const double vol = inter * zov;
    if (vol > 0) vol3d = vol / (a1 * h1 + a2 * h2 - vol);
}

}  // namespace dpft

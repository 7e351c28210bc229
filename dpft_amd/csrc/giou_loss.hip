// Differentiable GIoU3D term of the set criterion (optional, `loss_weights["giou"]`; the reference has no usable counterpart:
// its GIoULoss goes through pytorch3d and documents "Backward is not supported", src/dprt/utils/iou.py:132).
//
//   term = w_giou / B * sum_b 1 / P_b * sum_k (1 - G(pred[b, i_k], gt[b, j_k])) / 2        P_b = counts[b] matched pairs (i_k, j_k)
//
// G is the yaw-box GIoU3D of giou3d_yaw_pair (misc.hip: BEV rectangle clip x z overlap, axis-aligned enclosing box over all
// sixteen corners, fp64) with two deliberate differences:
//   1. union = v1 + v2 - vol ALWAYS, G = vol / union - (evol - union) / evol.  The matcher keeps the reference's quirk (union = 0
//      without an intersection, so every disjoint pair costs a constant -1); a loss needs the textbook value there: disjoint pairs
//      are the ones GIoU exists for.  For intersecting valid boxes both are the same number.
//   2. yaw = atan2(sin, cos) in fp64 from the fp32 (sin, cos) pair (the matcher rounds atan2f to fp32), and the gradient goes
//      through it: with r2 = sin^2 + cos^2, d yaw / d sin = cos / r2, d yaw / d cos = -sin / r2, both 0 for r2 = 0.
// A box that fails the matcher's validity rule (min(lw, lh, wh) / 2 > 1e-4) or has a size <= 0 gives G = -1, a pair loss of 1
// and no gradient.
//
// The derivative is carried in FORWARD mode: every fp64 quantity of the corner / clip / shoelace / min-max chain comes with its
// eight partials (center 3 | size 3 | sin, cos).  Comparisons look at the values only, so at a tie (two equal min/max
// candidates, a vertex on a clip line) the derivative is that of the side the value computation took.  A step has a few hundred
// pairs: arithmetic is not the constraint, the launch's place in the loss window is.  One workgroup does the whole batch, so the
// sum needs neither atomics nor a second launch: per-thread partial sums in slot order, then a fixed tree -- repeated launches
// give the same bits.
#include "common.h"

namespace dpft {
namespace {

constexpr int kND = 8;        // partials: d center[3] | d size[3] | d angle[2] (sin, cos)
constexpr int kMaxV = 12;     // clip polygon capacity (a quadrilateral clipped by four half-planes has at most 8 vertices)
constexpr int kThreads = 256;

struct Dual {
    double v;
    double d[kND];
};

__device__ inline double val(double x) { return x; }
__device__ inline double val(const Dual& x) { return x.v; }

__device__ inline Dual operator+(const Dual& a, const Dual& b) {
    Dual r; r.v = a.v + b.v;
    for (int i = 0; i < kND; ++i) r.d[i] = a.d[i] + b.d[i];
    return r;
}
__device__ inline Dual operator+(const Dual& a, double b) { Dual r = a; r.v += b; return r; }
__device__ inline Dual operator+(double a, const Dual& b) { return b + a; }
__device__ inline Dual operator-(const Dual& a, const Dual& b) {
    Dual r; r.v = a.v - b.v;
    for (int i = 0; i < kND; ++i) r.d[i] = a.d[i] - b.d[i];
    return r;
}
__device__ inline Dual operator-(const Dual& a, double b) { Dual r = a; r.v -= b; return r; }
__device__ inline Dual operator-(double a, const Dual& b) {
    Dual r; r.v = a - b.v;
    for (int i = 0; i < kND; ++i) r.d[i] = -b.d[i];
    return r;
}
__device__ inline Dual operator-(const Dual& a) { return 0.0 - a; }
__device__ inline Dual operator*(const Dual& a, const Dual& b) {
    Dual r; r.v = a.v * b.v;
    for (int i = 0; i < kND; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    return r;
}
__device__ inline Dual operator*(const Dual& a, double b) {
    Dual r; r.v = a.v * b;
    for (int i = 0; i < kND; ++i) r.d[i] = a.d[i] * b;
    return r;
}
__device__ inline Dual operator*(double a, const Dual& b) { return b * a; }
__device__ inline Dual operator/(const Dual& a, const Dual& b) {
    Dual r; r.v = a.v / b.v;
    for (int i = 0; i < kND; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
    return r;
}

template <class T> __device__ inline T lift(double x);                 // a constant
template <> __device__ inline double lift<double>(double x) { return x; }
template <> __device__ inline Dual lift<Dual>(double x) {
    Dual r; r.v = x;
    for (int i = 0; i < kND; ++i) r.d[i] = 0.0;
    return r;
}
template <class T> __device__ inline T input(double x, int which);      // input number `which` of the eight
template <> __device__ inline double input<double>(double x, int) { return x; }
template <> __device__ inline Dual input<Dual>(double x, int which) {
    Dual r = lift<Dual>(x);
    r.d[which] = 1.0;
    return r;
}
// min / max / abs: the VALUE decides, the partials follow the candidate taken
template <class T> __device__ inline T tmin(const T& a, const T& b) { return val(b) < val(a) ? b : a; }
template <class T> __device__ inline T tmax(const T& a, const T& b) { return val(b) > val(a) ? b : a; }
template <class T> __device__ inline T tabs(const T& a) { return val(a) < 0 ? -a : a; }

__device__ inline double t_atan2(double s, double c) { return atan2(s, c); }
__device__ inline Dual t_atan2(const Dual& s, const Dual& c) {
    Dual r; r.v = atan2(s.v, c.v);
    const double r2 = s.v * s.v + c.v * c.v;
    const double ds = r2 > 0 ? c.v / r2 : 0.0, dc = r2 > 0 ? -s.v / r2 : 0.0;
    for (int i = 0; i < kND; ++i) r.d[i] = ds * s.d[i] + dc * c.d[i];
    return r;
}
__device__ inline void t_sincos(double a, double& si, double& co) { si = sin(a); co = cos(a); }
__device__ inline void t_sincos(const Dual& a, Dual& si, Dual& co) {
    si.v = sin(a.v); co.v = cos(a.v);
    for (int i = 0; i < kND; ++i) { si.d[i] = co.v * a.d[i]; co.d[i] = -si.v * a.d[i]; }
}

template <class T> struct Pt { T x, y; };

// BEV corners in the order of rect_corners (misc.hip): counter-clockwise for l, w > 0
template <class T>
__device__ void bev_corners(const T& cx, const T& cy, const T& l, const T& w, const T& si, const T& co, Pt<T>* c) {
    const double sx[4] = {-1, 1, 1, -1}, sy[4] = {-1, -1, 1, 1};
    for (int i = 0; i < 4; ++i) {
        const T x = l * (sx[i] / 2), y = w * (sy[i] / 2);
        c[i].x = co * x - si * y + cx;
        c[i].y = si * x + co * y + cy;
    }
}

template <class T>
__device__ T poly_area2(const Pt<T>* p, int n) {      // twice the signed area
    T a = lift<T>(0.0);
    for (int i = 0; i < n; ++i) {
        const Pt<T>&u = p[i], &v = p[(i + 1) % n];
        a = a + (u.x * v.y - v.x * u.y);
    }
    return a;
}

__device__ inline bool box_valid(double l, double w, double h) {
    return l > 0 && w > 0 && h > 0 && fmin(fmin(l * w, l * h), w * h) / 2 > 1e-4;
}

// G of the prediction (center 3 | size 3 | angle 2 rows) against the target row g = center | size | angle.
// false: a box is invalid -- G = -1 and no gradient (nothing is written to G).
template <class T>
__device__ bool giou_pair(const float* ce, const float* sz, const float* an, const float* g, T& G) {
    if (!(box_valid(sz[0], sz[1], sz[2]) && box_valid(g[3], g[4], g[5]))) return false;
    const T cx = input<T>(ce[0], 0), cy = input<T>(ce[1], 1), cz = input<T>(ce[2], 2);
    const T l = input<T>(sz[0], 3), w = input<T>(sz[1], 4), h = input<T>(sz[2], 5);
    const T yaw = t_atan2(input<T>(an[0], 6), input<T>(an[1], 7));
    T si, co;
    t_sincos(yaw, si, co);
    Pt<T> A[4];
    bev_corners(cx, cy, l, w, si, co, A);
    const T azl = cz - h * 0.5, azh = cz + h * 0.5;
    // the target: constants
    const double gl = g[3], gw = g[4], gh = g[5];
    double gsi, gco;
    t_sincos(atan2((double)g[6], (double)g[7]), gsi, gco);
    Pt<double> Q[4];
    bev_corners<double>(g[0], g[1], gl, gw, gsi, gco, Q);
    const double bzl = (double)g[2] - gh / 2, bzh = (double)g[2] + gh / 2;
    // enclosing axis-aligned box over all sixteen corners
    T xmin = A[0].x, xmax = A[0].x, ymin = A[0].y, ymax = A[0].y;
    double qxmin = Q[0].x, qxmax = Q[0].x, qymin = Q[0].y, qymax = Q[0].y;
    for (int k = 1; k < 4; ++k) {
        xmin = tmin(xmin, A[k].x); xmax = tmax(xmax, A[k].x);
        ymin = tmin(ymin, A[k].y); ymax = tmax(ymax, A[k].y);
        qxmin = fmin(qxmin, Q[k].x); qxmax = fmax(qxmax, Q[k].x);
        qymin = fmin(qymin, Q[k].y); qymax = fmax(qymax, Q[k].y);
    }
    xmin = tmin(xmin, lift<T>(qxmin)); xmax = tmax(xmax, lift<T>(qxmax));
    ymin = tmin(ymin, lift<T>(qymin)); ymax = tmax(ymax, lift<T>(qymax));
    const T evol = (xmax - xmin) * (ymax - ymin) * (tmax(azh, lift<T>(bzh)) - tmin(azl, lift<T>(bzl)));
    // Sutherland-Hodgman: the prediction's rectangle clipped by the target's four half-planes.  Both are counter-clockwise:
    // every size is > 0 here, so the matcher's orientation swap cannot trigger.
    Pt<T> poly[kMaxV], tmp[kMaxV];
    int n = 4;
    for (int k = 0; k < 4; ++k) poly[k] = A[k];
    for (int e = 0; e < 4 && n > 0; ++e) {
        const Pt<double> a = Q[e], bb = Q[(e + 1) & 3];
        const double ex = bb.x - a.x, ey = bb.y - a.y;
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const Pt<T>&c = poly[k], &d = poly[(k + 1) % n];
            const T sc = ex * (c.y - a.y) - ey * (c.x - a.x);
            const T sd = ex * (d.y - a.y) - ey * (d.x - a.x);
            if (val(sc) >= 0 && m < kMaxV) tmp[m++] = c;
            if ((val(sc) >= 0) != (val(sd) >= 0) && m < kMaxV) {      // (the capacity test only ever bites for non-finite input)
                const T t = sc / (sc - sd);
                tmp[m].x = c.x + t * (d.x - c.x);
                tmp[m].y = c.y + t * (d.y - c.y);
                ++m;
            }
        }
        n = m;
        for (int k = 0; k < n; ++k) poly[k] = tmp[k];
    }
    const T inter_a = n >= 3 ? tabs(poly_area2(poly, n)) * 0.5 : lift<T>(0.0);
    const T vol = inter_a * tmax(lift<T>(0.0), tmin(azh, lift<T>(bzh)) - tmax(azl, lift<T>(bzl)));
    const T uni = l * w * h + gl * gw * gh - vol;
    if (val(evol) == 0 || val(uni) == 0) {      // (not reachable with finite valid boxes)
        G = lift<T>(0.0);
        return true;
    }
    G = vol / uni - (evol - uni) / evol;
    return true;
}

struct GiouLossArgs {
    const float *center, *size, *angle;      // (B,N,3) (B,N,3) (B,N,2)
    const float* gt_box;                     // (B,Mmax,8) center | size | angle
    const int32_t* match;                    // (B,Mmax,2) (query, target), -1 padded
    const int32_t* counts;                   // (B) matched pairs
    const float *total_in, *gout;            // device scalars, may be null
    float *term, *total_out, *g_pairs;       // forward outputs
    float *dcenter, *dsize, *dangle;         // backward outputs
    double scale;                            // w_giou / B
    int B, N, Mmax, accumulate;
};

// the pair of slot (b, k), or false for an empty slot (beyond the matched count, or an index outside its table)
__device__ inline bool slot_pair(const GiouLossArgs& a, int64_t slot, int& b, int& pairs, int& i, int& j) {
    b = (int)(slot / a.Mmax);
    const int k = (int)(slot % a.Mmax);
    pairs = min(a.counts[b], a.Mmax);
    if (k >= pairs) return false;
    i = a.match[slot * 2];
    j = a.match[slot * 2 + 1];
    return i >= 0 && i < a.N && j >= 0 && j < a.Mmax;
}

__global__ __launch_bounds__(kThreads) void giou_loss_fwd_kernel(GiouLossArgs a) {
    __shared__ double part[kThreads];
    const int tid = threadIdx.x;
    const int64_t slots = (int64_t)a.B * a.Mmax;
    double acc = 0.0;
    for (int64_t slot = tid; slot < slots; slot += kThreads) {
        int b, pairs, i, j;
        double G = 0.0;
        if (slot_pair(a, slot, b, pairs, i, j)) {
            const int64_t row = (int64_t)b * a.N + i;
            if (!giou_pair<double>(a.center + row * 3, a.size + row * 3, a.angle + row * 2,
                                   a.gt_box + ((int64_t)b * a.Mmax + j) * 8, G))
                G = -1.0;
            acc += (1.0 - G) * 0.5 / pairs;
        }
        if (a.g_pairs) a.g_pairs[slot] = (float)G;
    }
    part[tid] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const float term = (float)(a.scale * part[0]);
        *a.term = term;
        if (a.total_out) *a.total_out = *a.total_in + term;
    }
}

__global__ __launch_bounds__(kThreads) void giou_loss_bwd_kernel(GiouLossArgs a) {
    const int tid = threadIdx.x;
    if (!a.accumulate) {
        // write form: every row, zeros for unmatched queries (one workgroup: the barrier orders these stores before the pairs')
        const int64_t rows = (int64_t)a.B * a.N;
        for (int64_t e = tid; e < rows * 3; e += kThreads) { a.dcenter[e] = 0.f; a.dsize[e] = 0.f; }
        for (int64_t e = tid; e < rows * 2; e += kThreads) a.dangle[e] = 0.f;
        __syncthreads();
    }
    const double up = a.gout ? (double)*a.gout : 1.0;
    const int64_t slots = (int64_t)a.B * a.Mmax;
    for (int64_t slot = tid; slot < slots; slot += kThreads) {
        int b, pairs, i, j;
        if (!slot_pair(a, slot, b, pairs, i, j)) continue;
        const int64_t row = (int64_t)b * a.N + i;      // a query is matched at most once per sample: no two slots share a row
        Dual G;
        const bool ok = giou_pair<Dual>(a.center + row * 3, a.size + row * 3, a.angle + row * 2,
                                        a.gt_box + ((int64_t)b * a.Mmax + j) * 8, G);
        const double coef = up * (a.scale * -0.5 / pairs);      // d term / d G, times the upstream gradient
        for (int c = 0; c < kND; ++c) {
            // rounded to fp32 FIRST, then added in fp32: the accumulate form is bit-equal to "write form, then +="
            const float gr = ok ? (float)(coef * G.d[c]) + 0.f : 0.f;      // (+ 0: no negative zeros)
            float* dst = c < 3 ? a.dcenter + row * 3 + c : (c < 6 ? a.dsize + row * 3 + (c - 3) : a.dangle + row * 2 + (c - 6));
            *dst = a.accumulate ? *dst + gr : gr;
        }
    }
}

int check_common(const char* what, const float* center, const float* size, const float* angle, const float* gt_box,
                 const int32_t* match, const int32_t* counts, float w_giou, int32_t B, int32_t N, int32_t Mmax) {
    DPFT_REQUIRE(center && size && angle && gt_box && match && counts, "%s: null argument", what);
    DPFT_REQUIRE(B > 0 && N > 0 && Mmax > 0, "%s: non-positive sizes (B=%d, N=%d, Mmax=%d)", what, B, N, Mmax);
    DPFT_REQUIRE(w_giou >= 0.f && w_giou <= 3.402823466e38f, "%s: the weight must be finite and >= 0", what);
    return DPFT_OK;
}

}  // namespace
}  // namespace dpft

using namespace dpft;

extern "C" int dpft_giou_loss_fwd_f32(const float* center, const float* size, const float* angle, const float* gt_box,
                                      const int32_t* match, const int32_t* counts, float w_giou, const float* total_in,
                                      float* term, float* total_out, float* g_pairs, int32_t B, int32_t N, int32_t Mmax,
                                      dpft_stream_t stream) {
    const int rc = check_common("giou_loss_fwd", center, size, angle, gt_box, match, counts, w_giou, B, N, Mmax);
    if (rc != DPFT_OK) return rc;
    DPFT_REQUIRE(term, "giou_loss_fwd: null output");
    DPFT_REQUIRE((total_in == nullptr) == (total_out == nullptr), "giou_loss_fwd: total_in and total_out come together");
    GiouLossArgs a{};
    a.center = center; a.size = size; a.angle = angle; a.gt_box = gt_box; a.match = match; a.counts = counts;
    a.total_in = total_in; a.term = term; a.total_out = total_out; a.g_pairs = g_pairs;
    a.scale = (double)w_giou / B; a.B = B; a.N = N; a.Mmax = Mmax;
    hipLaunchKernelGGL(giou_loss_fwd_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
    return check_launch("giou_loss_fwd");
}

extern "C" int dpft_giou_loss_bwd_f32(const float* center, const float* size, const float* angle, const float* gt_box,
                                      const int32_t* match, const int32_t* counts, float w_giou, const float* gout,
                                      float* dcenter, float* dsize, float* dangle, int32_t accumulate, int32_t B, int32_t N,
                                      int32_t Mmax, dpft_stream_t stream) {
    const int rc = check_common("giou_loss_bwd", center, size, angle, gt_box, match, counts, w_giou, B, N, Mmax);
    if (rc != DPFT_OK) return rc;
    DPFT_REQUIRE(dcenter && dsize && dangle, "giou_loss_bwd: null gradient buffer");
    GiouLossArgs a{};
    a.center = center; a.size = size; a.angle = angle; a.gt_box = gt_box; a.match = match; a.counts = counts;
    a.gout = gout; a.dcenter = dcenter; a.dsize = dsize; a.dangle = dangle; a.accumulate = accumulate != 0;
    a.scale = (double)w_giou / B; a.B = B; a.N = N; a.Mmax = Mmax;
    hipLaunchKernelGGL(giou_loss_bwd_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
    return check_launch("giou_loss_bwd");
}

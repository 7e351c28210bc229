// The scratch of dpft_nms_f32 as a contract (include/dpft_hip.h states it for callers): nms.hip fills it, tta.hip reads the
// sorted arrays after the scan pass.  Everything is in SORTED order per frame (score descending, query ascending); only the
// first ndet[b] entries of frame b are written.
#pragma once
#include <stdint.h>

namespace dpft {

struct NmsScratch {
    unsigned long long* mask;      // (B, W, W, 64), W = ceil(N / 64): word [i / 64][w][i % 64] = bits j = 64 w .. 64 w + 63 of row i
    float* box;                    // (B,N,8): center 3, size 3, angle 2
    int* label;                    // (B,N) argmax class
    int* sorted;                   // (B,N) query index
    float* score;                  // (B,N)
    int* ndet;                     // (B) number of candidates
};

inline int64_t nms_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

inline int64_t nms_scratch_size(int64_t B, int64_t N) {
    const int64_t W = (N + 63) / 64;
    return nms_align16(B * W * W * 64 * 8 + B * N * (8 + 3) * 4 + B * 4);
}

inline NmsScratch nms_scratch_layout(void* scratch, int64_t B, int64_t N) {
    const int64_t W = (N + 63) / 64;
    NmsScratch s;
    char* p = (char*)scratch;
    s.mask = (unsigned long long*)p; p += B * W * W * 64 * 8;
    s.box = (float*)p;               p += B * N * 8 * 4;
    s.label = (int*)p;               p += B * N * 4;
    s.sorted = (int*)p;              p += B * N * 4;
    s.score = (float*)p;             p += B * N * 4;
    s.ndet = (int*)p;
    return s;
}

}  // namespace dpft

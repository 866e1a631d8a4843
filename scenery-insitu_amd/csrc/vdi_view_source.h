// vdi_view_source.h -- where the lists of a ViewSource lie (insitu_kernels.h), shared by view_build_kernel
// (vdi_view.hip) and the merge kernels (vdi_view_merge.hip).  Every product in 64 bits.
#pragma once
#include "insitu_kernels.h"

namespace insitu {

// Entry k of list j of one pixel at col/dep[e0 + j*lstride + k*estride]
struct ViewAt {
    size_t e0, lstride, estride;
};

// (x, y) inside the W x H window of lists of S slots
__device__ __forceinline__ ViewAt view_at(const ViewSource& P, int x, int y, int H, int S) {
    ViewAt a;
    if (P.reference) {
        a.e0 = ((size_t)x * (size_t)H + (size_t)y) * (size_t)S;
        a.lstride = P.ref_stride;
        a.estride = 1;
    } else {
        const int d = x / P.strip_w, xl = x - d * P.strip_w, xt = xl >> 3, xx = xl & 7;
        const size_t blockE = (size_t)P.strip_tiles * (size_t)S * (size_t)H * 8;
        a.e0 = ((size_t)d * (size_t)P.B + (size_t)P.b) * blockE + ((size_t)xt * (size_t)S * (size_t)H + (size_t)y) * 8 + (size_t)xx;
        a.lstride = blockE;
        a.estride = (size_t)H * 8;
    }
    return a;
}

// the slots of list j of the pixel that may hold entries: the stored count, or all S in the reference layout
__device__ __forceinline__ int view_slots(const ViewSource& P, int j, int x, int y, int S) {
    if (P.reference) return S;
    const int d = x / P.strip_w, xl = x - d * P.strip_w;
    const int stored = (int)(P.cnt[(size_t)(P.b + j) * P.cnt_stride + (size_t)d * P.cnt_dstride + (size_t)y * P.cnt_pitch + (size_t)xl] & kPendingCount);
    return stored < S ? stored : S;   // (a corrupt count must not walk past the S slots)
}

}  // namespace insitu

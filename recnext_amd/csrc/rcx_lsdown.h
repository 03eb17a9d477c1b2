// What the forward (rcx_lsdown.hip) and the backward (rcx_lsdownbwd.hip) of the grouped Downsample conv share: the staging routine and the store's rounding.
#pragma once
#include "rcx_common.h"

namespace rcx {
namespace {

// the tile's pixels, `run` bytes of each, from global memory to LDS in accesses of sizeof(U) bytes; zeros outside the image
template <typename U>
__device__ __forceinline__ void stage(unsigned char* __restrict__ tile, const unsigned char* __restrict__ src, int rows, int cols, int run, int lds_pix,
                                      size_t pix_bytes, int iy0, int ix0, int H, int W, int nthreads)
{
    const int nv = run / (int)sizeof(U);
    const int total = rows * cols * nv;
    for (int i = threadIdx.x; i < total; i += nthreads) {
        const int v = i % nv, p = i / nv;
        const int c = p % cols, r = p / cols;
        const int iy = iy0 + r, ix = ix0 + c;
        U val = {};
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) val = *reinterpret_cast<const U*>(src + ((size_t)iy * W + ix) * pix_bytes + (size_t)v * sizeof(U));
        *reinterpret_cast<U*>(tile + (size_t)p * lds_pix + (size_t)v * sizeof(U)) = val;
    }
}

template <typename T>
__device__ __forceinline__ T from_f32(float v)
{
    if constexpr (sizeof(T) == 4) return v;
    else if constexpr (DtId<T>::id == 1) return f32_to_bf16(v);
    else return (T)v;
}

}  // namespace
}  // namespace rcx

// Band machinery shared by the float LBP kernels (ofr_lbp_float.hip) and the VarLBP kernels
// (ofr_varlbp.hip): a 1024-thread workgroup stages a band of pixel rows into LDS as fp64 and its u32
// LDS counters leave packed.  See ofr_lbp_float.hip for the design.
#pragma once
#include "ofr_common.h"

namespace ofr {
namespace lbpf {

constexpr int THREADS = 1024;
constexpr int LDS_MAX = 160 * 1024;
constexpr int LDS_HALF = 80 * 1024;  // two workgroups per CU

// np.asarray(x, dtype=np.uint8) of a float as fp64: (int64)trunc(x) & 255
__device__ __forceinline__ double centre_u8(double x) {
  const double t = trunc(x);
  const double q = floor(t * 0.00390625);
  const double m = 256.0 * q;
  return t - m;
}

// `count` contiguous pixels (uint8, float32 or float64) -> fp64 in LDS: 16-byte loads from the first
// 16-byte boundary on, the elements in front of it and behind the last whole vector one by one
template <typename T>
__device__ __forceinline__ void stage_plane(const T* __restrict__ src, double* __restrict__ dst, int count) {
  constexpr int V = 16 / (int)sizeof(T);
  const int head = min(count, (int)(((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) / sizeof(T)));
  const int nvec = (count - head) / V;
  for (int i = threadIdx.x; i < head; i += THREADS) dst[i] = (double)src[i];
  const T* body = src + head;
  double* out = dst + head;
  for (int i = threadIdx.x; i < nvec; i += THREADS) {
    if constexpr (sizeof(T) == 1) {
      const uint4 v = reinterpret_cast<const uint4*>(body)[i];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) out[16 * i + j] = (double)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    } else if constexpr (sizeof(T) == 4) {
      const float4 v = reinterpret_cast<const float4*>(body)[i];
      out[4 * i + 0] = (double)v.x;
      out[4 * i + 1] = (double)v.y;
      out[4 * i + 2] = (double)v.z;
      out[4 * i + 3] = (double)v.w;
    } else {
      const double2 v = reinterpret_cast<const double2*>(body)[i];
      out[2 * i + 0] = v.x;
      out[2 * i + 1] = v.y;
    }
  }
  for (int i = head + nvec * V + threadIdx.x; i < count; i += THREADS) dst[i] = (double)src[i];
}

// LDS counters [total] -> 1/2/4-byte counts starting at element `first` of the destination
__device__ __forceinline__ void flush_band(const uint32_t* hist, int total, void* counts, int64_t first, int cb,
                                           bool packed) {
  if (packed && cb == 1) {
    uint32_t* o = reinterpret_cast<uint32_t*>((uint8_t*)counts + first);
    for (int i = threadIdx.x; i < total / 4; i += THREADS)
      o[i] = hist[4 * i] | (hist[4 * i + 1] << 8) | (hist[4 * i + 2] << 16) | (hist[4 * i + 3] << 24);
  } else if (packed && cb == 2) {
    uint32_t* o = reinterpret_cast<uint32_t*>((uint16_t*)counts + first);
    for (int i = threadIdx.x; i < total / 2; i += THREADS) o[i] = hist[2 * i] | (hist[2 * i + 1] << 16);
  } else if (cb == 4) {
    uint32_t* o = (uint32_t*)counts + first;
    for (int i = threadIdx.x; i < total; i += THREADS) o[i] = hist[i];
  } else if (cb == 2) {
    uint16_t* o = (uint16_t*)counts + first;
    for (int i = threadIdx.x; i < total; i += THREADS) o[i] = (uint16_t)hist[i];
  } else {
    uint8_t* o = (uint8_t*)counts + first;
    for (int i = threadIdx.x; i < total; i += THREADS) o[i] = (uint8_t)hist[i];
  }
}

}  // namespace lbpf
}  // namespace ofr

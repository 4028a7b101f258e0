// Shared by the row / elementwise / optimizer kernels (norms, elementwise,
// cross_entropy, adamw, embedding): the 16-byte "8 elements as fp32" access
// and the host-side dtype / flag dispatch.
#pragma once
#include <type_traits>

#include "common.h"
#include "api.h"

namespace pa {

// -------- type abstraction: load/store 8 elems as fp32 ---------------------
// load8 / store8 are one (bf16) or two (fp32) 16-byte accesses: idx must put
// the address on a 16-byte boundary.  load1 / store1 have no such contract.
template <int DT> struct VIO;

template <> struct VIO<kBF16> {
  using ST = short;
  static __device__ __forceinline__ void load8(const void* p, int64_t idx, float* f) {
    shortx8 v = *reinterpret_cast<const shortx8*>((const short*)p + idx);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = bf2f(v[i]);
  }
  static __device__ __forceinline__ void store8(void* p, int64_t idx, const float* f) {
    shortx8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = f2bf(f[i]);
    *reinterpret_cast<shortx8*>((short*)p + idx) = v;
  }
  static __device__ __forceinline__ float load1(const void* p, int64_t idx) {
    return bf2f(((const short*)p)[idx]);
  }
  static __device__ __forceinline__ void store1(void* p, int64_t idx, float f) {
    ((short*)p)[idx] = f2bf(f);
  }
};

template <> struct VIO<kF32> {
  using ST = float;
  static __device__ __forceinline__ void load8(const void* p, int64_t idx, float* f) {
    const float4* q = reinterpret_cast<const float4*>((const float*)p + idx);
    float4 a = q[0], b = q[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
    f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
  static __device__ __forceinline__ void store8(void* p, int64_t idx, const float* f) {
    float4* q = reinterpret_cast<float4*>((float*)p + idx);
    q[0] = make_float4(f[0], f[1], f[2], f[3]);
    q[1] = make_float4(f[4], f[5], f[6], f[7]);
  }
  static __device__ __forceinline__ float load1(const void* p, int64_t idx) {
    return ((const float*)p)[idx];
  }
  static __device__ __forceinline__ void store1(void* p, int64_t idx, float f) {
    ((float*)p)[idx] = f;
  }
};

// -------- host: runtime tag -> compile-time constant ------------------------
// by_dtype(dtype, [&](auto DT) { launch kernel<DT()> }): DT is a
// std::integral_constant of kBF16 or kF32 ("not bf16" is fp32: the binding's
// dt_of admits nothing else).  by_flag does the same for a bool template flag.
template <class F>
inline void by_dtype(int dtype, F&& f) {
  if (dtype == kBF16) f(std::integral_constant<int, kBF16>{});
  else f(std::integral_constant<int, kF32>{});
}

template <class F>
inline void by_flag(bool v, F&& f) {
  if (v) f(std::true_type{}); else f(std::false_type{});
}

}  // namespace pa

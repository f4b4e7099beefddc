// 16-bit feature rows of the one-kernel SAGE layer (wg_sage_mfma.hip): how a lane's four features travel (`row_elems<XT>::raw_t`:
// 16 bytes of a float32 table, 8 bytes of a float16 / bfloat16 one) and their EXACT conversion to fp32 where the value is
// consumed.  Every fp16 and every bf16 value is an fp32 value, so a layer over a 16-bit table computes bit for bit what the
// float32 layer computes over `table.float()`.
//   bf16 -> fp32: the 16 bits are the top half of the fp32 word (a shift / a mask per element).
//   fp16 -> fp32: the hardware convert (v_cvt_f32_f16); subnormal fp16 values are normal fp32 values and convert exactly (the
//                 kernels run with fp16 denormals enabled, the HIP default).
// Plain C++ as well as HIP: tests/host/x16_convert_check.cpp runs the same functions on the host over all 65536 bit patterns.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define WG_X16_HD __host__ __device__ __forceinline__
#else
#define WG_X16_HD inline
#endif

namespace wgamd {
namespace x16 {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
// the same vectors where only the element's own alignment times four is known (rows of a 16-bit table are 8-B aligned)
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));

// four consecutive 16-bit elements (little-endian: element 0 in the low half of word 0) -> fp32
template <typename XT>
WG_X16_HD f32x4 to_f32x4(u32x2 r);
template <>
WG_X16_HD f32x4 to_f32x4<_Float16>(u32x2 r)
{
  return __builtin_convertvector(__builtin_bit_cast(f16x4, r), f32x4);
}
template <>
WG_X16_HD f32x4 to_f32x4<__bf16>(u32x2 r)
{
  const u32x4 w = {r[0] << 16, r[0] & 0xffff0000u, r[1] << 16, r[1] & 0xffff0000u};
  return __builtin_bit_cast(f32x4, w);
}

// what a lane holds of a row between its load and its use
template <typename XT>
struct row_elems {
  using raw_t                 = u32x2;
  static constexpr int kBytes = 2;   // per element
  static WG_X16_HD f32x4 f32(raw_t r) { return to_f32x4<XT>(r); }
};
template <>
struct row_elems<float> {
  using raw_t                 = f32x4;
  static constexpr int kBytes = 4;
  static WG_X16_HD f32x4 f32(raw_t r) { return r; }
};

}  // namespace x16
}  // namespace wgamd

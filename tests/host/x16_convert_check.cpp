// Stand-alone host check of csrc/wg_x16.hpp, the float16 / bfloat16 -> float32 conversions of the one-kernel SAGE layer: the same
// functions the kernel runs, compiled for the host, over ALL 65536 bit patterns and in each of the four element positions of a
// lane's 8-byte load, against (a) HIP's __half2float, (b) a 16-bit shift for bfloat16 and (c) a bit-level decoder of IEEE
// binary16 written out here (subnormals exact, no flush).  Everything is compared by bits, Inf and NaN patterns included.
//   hipcc -x hip --offload-host-only -O2 -I ../../cugraph-gnn_amd/csrc x16_convert_check.cpp -o x16_convert_check
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "wg_x16.hpp"

using namespace wgamd::x16;

static uint32_t bits_of(float f)
{
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// IEEE binary16 -> binary32 by hand (NaN: payload kept in the top bits; whether a signalling NaN comes out quiet is the
// converter's choice — hardware converts set the quiet bit, a software one may not — so NaNs are compared up to that bit)
constexpr uint32_t kQuietBit = 0x00400000u;
static uint32_t half_bits_to_float_bits(uint16_t h)
{
  const uint32_t sign = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31, m = h & 1023;
  if (e == 31) return sign | 0x7f800000u | (m << 13);
  if (e == 0) {
    if (m == 0) return sign;
    const float v = std::ldexp((float)m, -24);   // subnormal: m * 2^-24, exact in binary32
    return sign | bits_of(v);
  }
  return sign | ((e + 112) << 23) | (m << 13);
}

int main()
{
  long bad = 0;
  for (uint32_t p = 0; p < 65536; p++) {
    const uint16_t other = (uint16_t)(p * 40503u + 12345u);   // a different pattern in the other positions
    for (int pos = 0; pos < 4; pos++) {
      uint16_t e[4] = {other, (uint16_t)(other + 1), (uint16_t)(other + 2), (uint16_t)(other + 3)};
      e[pos] = (uint16_t)p;
      const u32x2 raw = {(uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16)};
      const f32x4 h = to_f32x4<_Float16>(raw), b = to_f32x4<__bf16>(raw);
      for (int i = 0; i < 4; i++) {
        __half_raw hr;
        hr.x = e[i];
        const uint32_t want_h = bits_of(__half2float(__half(hr))), want_b = (uint32_t)e[i] << 16;
        const bool nan      = (e[i] & 0x7c00) == 0x7c00 && (e[i] & 1023) != 0;
        const uint32_t loose = nan ? kQuietBit : 0u;
        if (bits_of(h[i]) != want_h || (bits_of(h[i]) | loose) != (half_bits_to_float_bits(e[i]) | loose)) {
          if (bad++ < 10) std::printf("fp16 0x%04x pos %d: got 0x%08x, __half2float 0x%08x, by hand 0x%08x\n", e[i], i, bits_of(h[i]), want_h, half_bits_to_float_bits(e[i]));
        }
        if (bits_of(b[i]) != want_b) {
          if (bad++ < 10) std::printf("bf16 0x%04x pos %d: got 0x%08x, want 0x%08x\n", e[i], i, bits_of(b[i]), want_b);
        }
      }
    }
  }
  // the 16-B form of the multiplying waves' self rows is two of the 8-B loads: element order across the halves
  const u32x4 wide = {0x3c003800u, 0x42004000u, 0x45004400u, 0x47004600u};   // fp16 0.5, 1, 2, 3, 4, 5, 6, 7
  const f32x4 lo = to_f32x4<_Float16>(u32x2{wide[0], wide[1]}), hi = to_f32x4<_Float16>(u32x2{wide[2], wide[3]});
  const float want[8] = {0.5f, 1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f};
  for (int i = 0; i < 4; i++)
    if (lo[i] != want[i] || hi[i] != want[4 + i]) bad++;
  static_assert(sizeof(row_elems<float>::raw_t) == 16 && sizeof(row_elems<_Float16>::raw_t) == 8 && sizeof(row_elems<__bf16>::raw_t) == 8, "");
  if (bad) {
    std::printf("x16_convert_check: %ld mismatches\n", bad);
    return 1;
  }
  std::printf("x16_convert_check: ok (65536 patterns x 4 positions x 2 types)\n");
  return 0;
}

// The pixel types of the encode's row kernels, the rule stated once: an fp32
// pixel is its own value; a byte pixel u means the fp32 number u / 255 (the
// correctly rounded fp32 quotient, torch's `u8.float() / 255`).  The decode's
// output pixels go the other way by byte_from_unit (round, clamp, truncate).
// The arithmetic is plain C++ that a host compiler builds alone
// (tests/test_u8_convert_host.py and tests/test_u8_quantise_host.py do); only
// the loads and stores are device code.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DCTAE_PX_HD __host__ __device__ __attribute__((always_inline))
#else
#define DCTAE_PX_HD
#endif

namespace dctae {

// x * (1 / 255), one rounding of the product of a rounded reciprocal: differs
// from x / 255 by an ulp for 126 of the 256 byte values.  Kept to say why
// unit_from_byte has its correction (the host test pins that it is not equal).
DCTAE_PX_HD inline float unit_from_byte_plain(float x) { return x * (1.0f / 255.0f); }

// x / 255 for x = 0 .. 255, without a division: q = x r (r = fl(1 / 255)) is
// within an ulp; the residual x - 255 q is exact in one FMA, and one more FMA
// adds its share: the correctly rounded quotient for all 256 values.  The FMAs
// are explicit calls, so no contraction setting of the caller (the row
// kernels' `fp contract(fast)` bodies) can change them.
DCTAE_PX_HD inline float unit_from_byte(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float r = 1.0f / 255.0f;
  const float q = x * r;
  return __builtin_fmaf(__builtin_fmaf(-255.0f, q, x), r, q);
}

// byte k (0 = lowest address) of a little-endian dword of four pixels, as its fp32 value
DCTAE_PX_HD inline float unit_from_dword(uint32_t w, int k) { return unit_from_byte((float)((w >> (8 * k)) & 0xffu)); }

// The byte of an output pixel, from the fp32 value x the fp32 decode writes:
// t = x * 255 rounded to fp32, t = t + 0.5 rounded to fp32, clamp to [0, 255],
// truncate -- torch's `x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)` on
// the CPU (save_image's rounding).  NaN gives 0 (both comparisons are false
// for it; torch leaves the case undefined), +inf 255, -inf / -0 / negative 0.
// Multiply and add are two operations outside any contraction (as above): a
// caller's `fp contract(fast)` body cannot fuse them into one rounding.
DCTAE_PX_HD inline uint8_t byte_from_unit(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float t = x * 255.0f;
  t = t + 0.5f;
  t = t > 0.0f ? t : 0.0f;       // NaN, -0 and everything negative: 0
  t = t < 255.0f ? t : 255.0f;
  return (uint8_t)(int32_t)t;    // t in [0, 255]: the truncation is exact
}

// four output pixels as one little-endian dword, p[0] at the lowest address
DCTAE_PX_HD inline uint32_t dword_from_units(const float (&p)[4]) {
  return (uint32_t)byte_from_unit(p[0]) | ((uint32_t)byte_from_unit(p[1]) << 8) |
         ((uint32_t)byte_from_unit(p[2]) << 16) | ((uint32_t)byte_from_unit(p[3]) << 24);
}

#if defined(__HIPCC__)
// the output pixel of value x, as the type the caller's image holds
template <typename Out>
__device__ __forceinline__ Out store_px(float x) {
  if constexpr (sizeof(Out) == 4)
    return x;
  else
    return byte_from_unit(x);
}

// the value of the pixel at p
__device__ __forceinline__ float load_px(const float* p) { return *p; }
__device__ __forceinline__ float load_px(const uint8_t* p) { return unit_from_byte((float)*p); }

// A pixel kept as loaded, for the kernels that load ahead of use (converting
// at the load would wait for it there): the register holds the fp32 value, or
// the byte zero-extended to 32 bits, and px_value gives the value at the use.
// Raw 0 is the value 0 for both types.
__device__ __forceinline__ float load_px_raw(const float* p) { return *p; }
__device__ __forceinline__ float load_px_raw(const uint8_t* p) { return __uint_as_float((uint32_t)*p); }
template <typename Px>
__device__ __forceinline__ float px_value(float raw) {
  if constexpr (sizeof(Px) == 4)
    return raw;
  else
    return unit_from_byte((float)__float_as_uint(raw));
}
#endif

// the tag the planner carries to the row pass (dctae_encode.hip: ImageSet::px)
// and the decode to the kernels that write the caller's RGB (dctae_decode.hip)
enum class PixelType : int { kF32 = 0, kU8 = 1 };

}  // namespace dctae

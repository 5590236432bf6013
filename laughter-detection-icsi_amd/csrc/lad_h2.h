// Two-way f16 split of scaled fp32 numbers ("f16 x 2"): shared by conv_h2.hip and the weight-gradient kernels (the sibling of
// lad_b3.h).
//
// An operand tile is held as x * 2^k = h1 + h2 + e with h1 = f16(x 2^k), h2 = f16(x 2^k - h1) (both round to nearest even; the
// subtraction is exact in f32) and k chosen so that the tile's largest magnitude lands in [2^14, 2^15) (scale_exp).  A product is
// a1 b2 + a2 b1 + a1 b1: three f16 MFMAs with f32 accumulation.  conv_h2.hip's header has the error analysis.
#pragma once
#include "lad_device.h"

namespace lad {

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_f16(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h16x2));   // round to nearest even
}
// two (scaled) fp32 values -> their two f16 planes, packed pairs
__device__ __forceinline__ void split2_pair(float a, float b, unsigned &p1, unsigned &p2) {
    const f32x2 v = {a, b};
    const h16x2 h = __builtin_convertvector(v, h16x2);
    p1 = __builtin_bit_cast(unsigned, h);
    p2 = pack_f16(a - (float)h.x, b - (float)h.y);   // (the differences are exact in f32)
}

// scale exponent for a tile / an image stage whose largest magnitude is `amax` (>= 0, finite): amax * 2^k in [2^14, 2^15)
__host__ __device__ __forceinline__ int scale_exp(float amax) {
    const int e = (int)((__builtin_bit_cast(unsigned, amax) >> 23) & 0xffu);
    const int k = 141 - e;
    return k > 100 ? 100 : k;       // (zero / denormal maxima: 2^100 keeps every product finite)
}
__device__ __forceinline__ float pow2f(int k) { return __builtin_bit_cast(float, (unsigned)(127 + k) << 23); }   // -126 <= k <= 127

// One MFMA operand (T = f16x8 or bf16x8) through two transposing reads: a group of 16 lanes reads 4 rows x 16 columns of 16-bit
// elements and receives them column-major.  addr_lo / addr_hi: LDS byte addresses of the lane's pieces of the two 4-row blocks.
template <class T>
__device__ __forceinline__ T read_tr_frag(unsigned addr_lo, unsigned addr_hi, int imm) {
    typedef __attribute__((address_space(3))) s16x4 *lds_p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(size_t)(addr_lo + imm));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(size_t)(addr_hi + imm));
    return __builtin_bit_cast(T, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace lad

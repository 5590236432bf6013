// Philox4x32-10 (Salmon et al., SC'11): four 32-bit words from a 128-bit counter and a 64-bit key -- a counter-based generator needs no
// state, so a value is a pure function of (key, counter): a dropout-mask element of (seed, draw number, element index) -- a hipGraph
// replay draws fresh masks (head.hip) -- and a segment's augmentation of (seed, epoch, channel, first frame) (augment.hip).
// Device code only.  Known answers (Random123's kat_vectors): tests/test_augment_cpu.py pins them on the numpy model, the GPU tests pin
// the kernels to that model.
#pragma once
#include <hip/hip_runtime.h>

namespace lad {
struct U4 {
    unsigned x, y, z, w;
};
__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
}  // namespace lad

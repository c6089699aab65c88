// Philox4x32-10 (Salmon et al., Random123), the one generator of the augmentation kernels (augment.hip, pose_augment.hip); augment.philox4x32
// in Python is the same function in numpy.
#pragma once
#include "common.h"

namespace sdt_philox {

struct Key {
    uint32_t k0, k1;
};
struct Words {
    uint32_t w[4];
};

// counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ Words philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, Key key) {
    uint32_t k0 = key.k0, k1 = key.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

}  // namespace sdt_philox

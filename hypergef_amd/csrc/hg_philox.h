// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// definition), one source for the segment kernels (hg_attention.hip) and the host statement of the dropout mask
// (hg_dropout_keep_host in hg_api.hip).
//
// One round:  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
// M0 = 0xD2511F53, M1 = 0xCD9E8D57; the key is bumped by (0x9E3779B9, 0xBB67AE85) after every round; ten rounds.
//
// The 32 x 32 -> 64 products are written as 64-bit products: on gfx950 the compiler turns each into one v_mad_u64_u32,
// which delivers both halves, where __umulhi and a low multiply would issue the pair v_mul_hi_u32 + v_mul_lo_u32.  That
// is a choice by instruction count; the instructions' issue rates have not been measured.  A key that is uniform over
// the wave stays in scalar registers with its ten bumps done on the scalar unit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HG_PHILOX_FN __host__ __device__ inline
#else
#define HG_PHILOX_FN inline
#endif

namespace hg {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// out[0..3] = philox4x32_10(counter c[0..3], key k[0..1])
HG_PHILOX_FN void philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
  uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// The 128-bit state of the attention dropout as the kernels hold it, and the threshold of the drop probability.
struct DropRng {
  uint32_t key_lo, key_hi, sid_lo, sid_hi;
};

HG_PHILOX_FN DropRng drop_rng(uint64_t key, uint64_t sid) {
  return DropRng{(uint32_t)key, (uint32_t)(key >> 32), (uint32_t)sid, (uint32_t)(sid >> 32)};
}

// T = floor(p * 2^32) for the fp32 p in [0, 1): at most 2^32 - 256, so it fits
HG_PHILOX_FN uint32_t drop_threshold(float p_drop) { return (uint32_t)((double)p_drop * 4294967296.0); }

// Is the coefficient of H_T position p, head h kept?  Word 0 of the Philox output for the counter (p, h, sid), the rest
// of the last round is dead code.
HG_PHILOX_FN bool drop_keep(const DropRng &r, uint32_t T, uint32_t p, uint32_t h) {
  const uint32_t c[4] = {p, h, r.sid_lo, r.sid_hi}, k[2] = {r.key_lo, r.key_hi};
  uint32_t w[4];
  philox4x32_10(c, k, w);
  return w[0] >= T;
}

}  // namespace hg

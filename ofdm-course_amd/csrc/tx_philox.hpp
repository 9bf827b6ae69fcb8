// Counter-based draws of the device frame generators (ofdm_txgen.hip, ofdm_txfused.hip): Philox4x32-10 with the payload
// counter (j_lo, j_hi, stream, 1) and the raw word form the impairment (counter word 3 = 2), noise (= 0) and per-frame
// channel (= 3, counter (tap, 0, stream, 3): ofdm_tx_frames_fading) draws use.
// Restated in oracle/ofdm_oracle.py (payload_codes_philox, sto_cfo_draw_philox, awgn_philox).
#pragma once

#include "ofdm_common.hpp"

namespace ofdm {

__device__ __forceinline__ uint32_t payload_code(uint64_t j, uint32_t stream, uint32_t k0, uint32_t k1, int bps) {
  uint32_t c0 = (uint32_t)j, c1 = (uint32_t)(j >> 32), c2 = stream, c3 = 1u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0 >> (32 - bps);
}

__device__ __forceinline__ void philox_words(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                             uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

}  // namespace ofdm

// bgzf_crc.h — the arithmetic of the sliced CRC-32 that the BGZF kernels share (bgzf.hip, bgzf_deflate.hip): the state after n more
// bytes from state s is s * x^(8n) + raw(bytes) in GF(2)[x] mod the polynomial, so a lane that folded a slice from state 0 multiplies
// its state by x^(8 * bytes behind its slice) and the states are XORed.  tests/bam_reference.py restates it (sliced_crc).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace bgsa {

constexpr uint32_t kCrcPoly = 0xedb88320u;    // IEEE 802.3, reflected

// Entry t of the 256-entry table of the reflected polynomial.
__device__ __forceinline__ uint32_t crc_table_entry(uint32_t t)
{
#pragma unroll
    for (int i = 0; i < 8; i++) t = (t >> 1) ^ (kCrcPoly & (0u - (t & 1u)));
    return t;
}

// a * b mod the polynomial, both reflected (bit 31 is x^0).
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}

// x^(8n) mod the polynomial.
__device__ __forceinline__ uint32_t gf_x_pow_bytes(unsigned n)
{
    uint32_t result = 0x80000000u, power = 0x00800000u;      // x^0, x^8
    while (n) {
        if (n & 1u) result = gf_mul(result, power);
        power = gf_mul(power, power);
        n >>= 1;
    }
    return result;
}

}  // namespace bgsa

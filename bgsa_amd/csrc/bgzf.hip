// bgzf.hip — BGZF framing of a byte payload on the device (include/bgsa_hip.h "BAM records": BGZF; SAMv1 §4.1).  It knows nothing
// about BAM: block b carries payload bytes [b * P, min((b + 1) * P, total)) as ONE stored deflate block inside a gzip member
// with the 'BC' extra subfield: 18 header bytes, 5 of deflate (01, LEN, ~LEN), the bytes, CRC-32 and ISIZE — LEN + 31 in all.
// One kernel, one workgroup of 256 threads per block.  Thread t takes the contiguous slice t of ceil(LEN / 256) bytes, reads every
// byte once, copies it into place and folds it into a CRC state of its own (the 256-entry table of the reflected IEEE polynomial,
// built in LDS by the workgroup: 1 KiB).  The states are joined by the CRC's linearity: the state after n more bytes from state s
// is s * x^(8n) + raw(bytes) in GF(2)[x] mod the polynomial, so thread t multiplies its state — started from 0, thread 0's from
// ~0 — by x^(8 * bytes behind its slice), by square-and-multiply on x^8, and an XOR butterfly per wave, then four words of LDS,
// join them.  Payload and output may start at any byte address: byte loads and byte stores.  No scratch, vector stores only.
// The output's extent is the caller's out_bytes, which must equal bgsa_hip_bgzf_framed_bytes: every block lies inside it.
#include "bgsa_common.h"
#include "bgzf_crc.h"

#include <limits.h>

namespace bgsa {

namespace {

constexpr int kFrameThreads = 256;
constexpr int kBlockExtra = 31;               // 18 + 5 in front of the bytes, 8 behind them
constexpr int kBlockPayloadMax = 0xff00;      // what every BGZF writer uses; the format's own limit is 65,505

__global__ __launch_bounds__(kFrameThreads) void bgzf_frame_kernel(const uint8_t *__restrict__ payload, int64_t payload_bytes, int block_payload,
                                                                   uint8_t *__restrict__ out)
{
    __shared__ uint32_t table[256];
    __shared__ uint32_t joined[kFrameThreads / kLanes];
    const int t = threadIdx.x;
    uint32_t entry = static_cast<uint32_t>(t);
#pragma unroll
    for (int i = 0; i < 8; i++) entry = (entry >> 1) ^ (kCrcPoly & (0u - (entry & 1u)));
    table[t] = entry;
    __syncthreads();

    const int64_t begin = static_cast<int64_t>(blockIdx.x) * block_payload;
    const int64_t left = payload_bytes - begin;                                    // >= 1: the grid is ceil(payload_bytes / block_payload)
    const int len = left < block_payload ? static_cast<int>(left) : block_payload;
    const uint8_t *src = payload + begin;
    uint8_t *dst = out + static_cast<int64_t>(blockIdx.x) * (block_payload + kBlockExtra);
    const int slice = (len + kFrameThreads - 1) / kFrameThreads;
    const int first = t * slice < len ? t * slice : len, last = first + slice < len ? first + slice : len;
    uint32_t state = t == 0 ? 0xffffffffu : 0u;
    for (int j = first; j < last; j++) {
        const uint8_t byte = src[j];
        dst[18 + 5 + j] = byte;
        state = table[(state ^ byte) & 0xffu] ^ (state >> 8);
    }
    if (state != 0u && last < len) state = gf_mul(state, gf_x_pow_bytes(static_cast<unsigned>(len - last)));
#pragma unroll
    for (int off = kLanes / 2; off >= 1; off >>= 1) state ^= __shfl_xor(state, off);
    if ((t & (kLanes - 1)) == 0) joined[t >> 6] = state;
    __syncthreads();

    if (t < 18 + 5) {
        const unsigned long long bsize = static_cast<unsigned long long>(len + kBlockExtra - 1), n = static_cast<unsigned long long>(len);
        const unsigned long long word = t < 8    ? 0x0000000004088b1full                                  // 1f 8b 08 04, MTIME 0
                                        : t < 16 ? 0x000243420006ff00ull                                  // XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0
                                                 : (bsize | 1ull << 16 | n << 24 | (~n & 0xffffull) << 40);      // BSIZE, 01, LEN, ~LEN
        dst[t] = static_cast<uint8_t>(word >> (8 * (t & 7)));
    } else if (t < 18 + 5 + 8) {
        const uint32_t crc = ~(joined[0] ^ joined[1] ^ joined[2] ^ joined[3]);
        const unsigned long long word = crc | static_cast<unsigned long long>(len) << 32;                 // CRC-32, ISIZE
        dst[len + t] = static_cast<uint8_t>(word >> (8 * (t - (18 + 5))));
    }
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int64_t bgsa_hip_bgzf_framed_bytes(int64_t payload_bytes, int block_payload)
{
    if (payload_bytes < 0 || payload_bytes > INT64_MAX / 32 || block_payload < 1 || block_payload > kBlockPayloadMax) return -1;
    return payload_bytes + kBlockExtra * ((payload_bytes + block_payload - 1) / block_payload);
}

int bgsa_hip_bgzf_frame_dev(const uint8_t *d_payload, int64_t payload_bytes, int block_payload, uint8_t *d_out, int64_t out_bytes, void *stream)
{
    const char *who = "bgzf_frame_dev";
    if (!d_payload || !d_out) return refuse(who, BGSA_HIP_EINVAL, "d_payload or d_out is NULL");
    if (block_payload < 1 || block_payload > kBlockPayloadMax) return refuse(who, BGSA_HIP_EINVAL, "block_payload must lie in 1..65280");
    const int64_t framed = bgsa_hip_bgzf_framed_bytes(payload_bytes, block_payload);
    if (framed < 0) return refuse(who, BGSA_HIP_EINVAL, "payload_bytes is negative or beyond int64 once framed");
    if (out_bytes != framed) return refuse(who, BGSA_HIP_EINVAL, "out_bytes is not bgsa_hip_bgzf_framed_bytes(payload_bytes, block_payload)");
    const int64_t n_blocks = (payload_bytes + block_payload - 1) / block_payload;
    if (n_blocks > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "more blocks than one launch holds");
    if (n_blocks == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(bgzf_frame_kernel, dim3(static_cast<unsigned>(n_blocks)), dim3(kFrameThreads), 0, static_cast<hipStream_t>(stream), d_payload,
                       payload_bytes, block_payload, d_out);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"

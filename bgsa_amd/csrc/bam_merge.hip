// bam_merge.hip — the one kernel a merge of many calls' BAM records needs (include/bgsa_hip.h "BAM records: merge"; INTEGRATION.md
// §3u): the record bytes, emitted once in input order, moved into coordinate order.  Output record i is source record order[i];
// a call moves the part of the records first .. first + count - 1 that lies in the window [window_lo, window_hi) of the sorted
// payload, so a caller frames or deflates the payload segment by segment through one buffer.  With d_flag, bytes 18 and 19 of every
// record — the BAM flag, little-endian — come from d_flag[s] instead of the source: duplicate marking over all records changes
// those two bytes and nothing else.
// One WAVE per output record, no LDS, no scratch, vector stores only.  The record's five scalars are wave-uniform and loaded once
// through scalar registers.  Both sides lie at any byte address: lane l moves the l-th DESTINATION-aligned dword of the record's
// part per step, assembled from the two source-aligned dwords that hold it (every dword loaded holds at least one byte of the
// record's part, so no load leaves a page the source does not own); the up to three bytes in front of the first aligned dword and
// behind the last one — a window edge ends a part anywhere — go out as bytes.  The flag bytes are put in place in registers.
// No value read from device memory forms an address before it has been compared with the extent the caller states.
#include "bgsa_common.h"

namespace bgsa {

namespace {

constexpr int kThreads = 256;
constexpr int kGatherWaves = kThreads / kLanes;
constexpr long long kFlagAt = 18;                          // the flag's two bytes, counted from the record's block_size field
constexpr long long kFlagEnd = 20;
constexpr int64_t kMaxRecords = static_cast<int64_t>(INT32_MAX) * kGatherWaves;      // one launch

// Byte `rel` (the offset inside its record) of a record whose flag is replaced by `flag`: the source's byte elsewhere.
__device__ __forceinline__ uint32_t flag_byte(uint32_t byte, long long rel, uint32_t flag)
{
    return rel == kFlagAt ? (flag & 0xffu) : rel == kFlagAt + 1 ? ((flag >> 8) & 0xffu) : byte;
}

__global__ __launch_bounds__(kThreads) void bam_gather_kernel(const uint8_t *__restrict__ src, long long src_bytes,
                                                              const int64_t *__restrict__ src_offsets, long long n_src,
                                                              const int64_t *__restrict__ order, const int64_t *__restrict__ dst_offsets,
                                                              long long first, long long count, long long window_lo, long long window_hi,
                                                              const int32_t *__restrict__ flag, uint8_t *__restrict__ out,
                                                              int32_t *__restrict__ refused)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const long long w = static_cast<long long>(blockIdx.x) * kGatherWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    if (w >= count) return;
    const long long i = first + w;
    const long long s = order[i];
    const long long d = dst_offsets[i], d_end = dst_offsets[i + 1];
    bool ok = s >= 0 && s < n_src && d >= 0 && d_end >= d;
    long long a = 0, len = 0;
    if (ok) {
        a = src_offsets[s];
        const long long a_end = src_offsets[s + 1];
        len = a_end - a;
        ok = a >= 0 && a_end >= a && a_end <= src_bytes && len == d_end - d && !(flag && len < kFlagEnd);
    }
    if (!ok) {
        if (lane == 0) atomicAdd(refused, 1);
        return;
    }
    const long long p0 = d > window_lo ? d : window_lo, p1 = d_end < window_hi ? d_end : window_hi;
    if (p0 >= p1) return;                        // the record lies outside the window
    const uint32_t f = flag ? static_cast<uint32_t>(flag[s]) : 0u;
    const bool patch = flag != nullptr;
    const long long rel0 = p0 - d, m = p1 - p0;  // the part: record bytes [rel0, rel0 + m)
    uint8_t *dp = out + (p0 - window_lo);
    const uint8_t *sp = src + a + rel0;
    long long head = static_cast<long long>(-reinterpret_cast<uintptr_t>(dp) & 3u);
    if (head > m) head = m;
    const long long words = (m - head) >> 2, tail = m - head - (words << 2);
    if (lane < head) {
        const uint32_t byte = sp[lane];
        dp[lane] = static_cast<uint8_t>(patch ? flag_byte(byte, rel0 + lane, f) : byte);
    }
    if (lane < tail) {
        const long long at = head + (words << 2) + lane;
        const uint32_t byte = sp[at];
        dp[at] = static_cast<uint8_t>(patch ? flag_byte(byte, rel0 + at, f) : byte);
    }
    const uint8_t *body = sp + head;
    const unsigned shift = static_cast<unsigned>(reinterpret_cast<uintptr_t>(body) & 3u) * 8u;
    const uint32_t *from = reinterpret_cast<const uint32_t *>(body - (shift >> 3));
    uint32_t *to = reinterpret_cast<uint32_t *>(dp + head);
    for (long long k = lane; k < words; k += kLanes) {
        uint32_t value = from[k];
        if (shift) value = value >> shift | from[k + 1] << (32u - shift);
        const long long rel = rel0 + head + (k << 2);       // the record offset of this dword's first byte
        if (patch && rel < kFlagEnd && rel + 4 > kFlagAt) {
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t byte = flag_byte(value >> (8 * b) & 0xffu, rel + b, f);
                value = (value & ~(0xffu << (8 * b))) | byte << (8 * b);
            }
        }
        to[k] = value;
    }
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_bam_gather_dev(const uint8_t *d_src, int64_t src_bytes, const int64_t *d_src_offsets, int64_t n_src, const int64_t *d_order,
                            const int64_t *d_dst_offsets, int64_t n, int64_t first, int64_t count, int64_t window_lo, int64_t window_hi,
                            const int32_t *d_flag, uint8_t *d_out, int32_t *d_refused, void *stream)
{
    const char *who = "bam_gather_dev";
    if (!d_src || !d_src_offsets || !d_order || !d_dst_offsets || !d_out || !d_refused)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only d_flag and the stream may be NULL)");
    if (src_bytes < 0 || n_src < 0 || n < 0 || first < 0 || count < 0)
        return refuse(who, BGSA_HIP_EINVAL, "src_bytes, n_src, n, first or count is negative");
    if (count > n || first > n - count) return refuse(who, BGSA_HIP_EINVAL, "first + count > n");
    if (window_hi < window_lo) return refuse(who, BGSA_HIP_EINVAL, "window_hi < window_lo");
    if (count > kMaxRecords) return refuse(who, BGSA_HIP_EINVAL, "count beyond one launch");
    if (count == 0 || window_hi == window_lo) return BGSA_HIP_OK;
    hipLaunchKernelGGL(bam_gather_kernel, dim3(static_cast<unsigned>((count + kGatherWaves - 1) / kGatherWaves)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_src, src_bytes, d_src_offsets, n_src, d_order, d_dst_offsets, first, count, window_lo,
                       window_hi, d_flag, d_out, d_refused);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"

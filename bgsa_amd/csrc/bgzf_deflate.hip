// bgzf_deflate.hip — BGZF blocks with DEFLATED payloads, compressed on the device (include/bgsa_hip.h "BAM records": deflate; RFC 1951
// inside SAMv1 §4.1).  Block b carries payload bytes [b * P, min((b + 1) * P, total)) as ONE deflate block with BFINAL = 1: dynamic
// Huffman codes (BTYPE 10) if and only if that is strictly shorter than the stored form, which is then byte for byte bgzf.hip's.
// tests/deflate_reference.py is the normative model: the output is a pure function of (payload, P) and equals the model's.
// One workgroup of 1,024 threads per block, the payload staged in LDS (64 KiB) beside a hash table of 2^15 uint16 (64 KiB):
//   1 match   positions in tiles of 1,024, one per thread: the candidates are position - 1 and the table entry of the position's
//             4-byte hash (the greatest position of any EARLIER tile; distance <= 32,768), lengths by comparison up to 258; the
//             tile's positions enter the table at its end by atomicMax on the dword that holds the uint16 — in two steps, even
//             hashes then odd, each with the other half held fixed, so the result is the maximum whatever the order
//   2 parse   greedy; the tile's chain is resolved by pointer jumping in LDS, ten rounds, which flags the token starts; every
//             flagged position counts its symbols (LDS atomicAdd) and every position's word — length, distance, flag — goes to the
//             workspace, 4 bytes per payload byte
//   3 codes   the used symbols sorted by (count, symbol) by ranking, 286 + 30 lanes; Moffat and Katajainen's in-place lengths,
//             miniz's limit to 15 bits and the canonical codes by one lane per alphabet; the exact bit count from the counts
//   4 emit    dynamic: every thread takes 64 consecutive positions, a prefix sum of their tokens' bits gives the offsets, the bits
//             are ORed into the table's 64 KiB (LDS atomicOr), the bytes copied to the slot; else the stored form
// The CRC is the sliced CRC of bgzf_crc.h over the staged bytes.  Payload and slots may start at any byte address: byte loads and
// byte stores.  Every loop is bounded by the block's length, no workgroup waits on another, no scratch, vector stores only.
#include "bgsa_common.h"
#include "bgzf_crc.h"

#include <limits.h>

namespace bgsa {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kLanes;
constexpr int kTile = 1024;                   // one position per thread
constexpr int kChunk = 64;                    // positions per thread in the emit pass: 1,024 * 64 >= 65,280
constexpr int kBlockExtra = 31;               // the slot: 18 + 5 in front of a stored payload, 8 behind it
constexpr int kBlockPayloadMax = 0xff00;
constexpr int kHashBits = 15;
constexpr int kWindow = 32768;
constexpr int kMaxMatch = 258;
constexpr int kLitLen = 286, kDist = 30, kDistAt = 288, kSymbols = 320;      // the distance alphabet sits at 288 of the shared arrays
constexpr int kHeaderBits = 17 + 19 * 3 + (kLitLen + kDist) * 4;
constexpr int kStoredOnly = (kHeaderBits + 2 + 7) / 8 - 5;                   // up to 163 bytes: the dynamic header alone is longer
constexpr int kPackThreads = 256;
constexpr uint32_t kStart = 0x80000000u;      // a position's word: length in bits 0..8 (0: literal), distance - 1 in 9..23, token start

static_assert(kThreads * kChunk >= kBlockPayloadMax && kTile == kThreads, "one position per thread and tile, 64 per thread to emit");

// The 4 bytes at byte `at` of the staged payload, little-endian, from two aligned words.
__device__ __forceinline__ uint32_t word_at(const uint32_t *data, int at)
{
    return __builtin_amdgcn_alignbyte(data[(at >> 2) + 1], data[at >> 2], static_cast<uint32_t>(at & 3));
}

// How many bytes data[a:] and data[b:] share, cap at the most.  Reads up to byte b + cap + 2: the array has the room.
__device__ __forceinline__ int match_length(const uint32_t *data, int a, int b, int cap)
{
    int n = 0;
    while (n < cap) {
        const uint32_t diff = word_at(data, a + n) ^ word_at(data, b + n);
        if (diff) {
            n += __builtin_ctz(diff) >> 3;
            break;
        }
        n += 4;
    }
    return n < cap ? n : cap;
}

__device__ __forceinline__ void length_symbol(int length, int &symbol, int &extra, uint32_t &value)
{
    const int l = length - 3;
    if (l < 8 || length == kMaxMatch) {
        symbol = length == kMaxMatch ? 285 : 257 + l, extra = 0, value = 0u;
        return;
    }
    extra = 29 - __builtin_clz(static_cast<uint32_t>(l));
    symbol = 261 + 4 * extra + ((l >> extra) & 3);
    value = static_cast<uint32_t>(l) & ((1u << extra) - 1u);
}

__device__ __forceinline__ void dist_symbol(int dist_minus_1, int &symbol, int &extra, uint32_t &value)
{
    const int d = dist_minus_1;
    if (d < 4) {
        symbol = d, extra = 0, value = 0u;
        return;
    }
    const int high = 31 - __builtin_clz(static_cast<uint32_t>(d));
    extra = high - 1;
    symbol = 2 * high + ((d >> extra) & 1);
    value = static_cast<uint32_t>(d) & ((1u << extra) - 1u);
}

__device__ __forceinline__ int litlen_extra(int symbol) { return symbol < 265 || symbol == 285 ? 0 : (symbol - 261) >> 2; }
__device__ __forceinline__ int dist_extra(int symbol) { return symbol < 4 ? 0 : (symbol >> 1) - 1; }

// n <= 32 bits of value (nothing above them set) at bit `at` of the stream, least significant first.
__device__ __forceinline__ void put_bits(uint32_t *stream, uint32_t at, uint32_t value, int n)
{
    const unsigned long long v = static_cast<unsigned long long>(value) << (at & 31u);
    const uint32_t lo = static_cast<uint32_t>(v), hi = static_cast<uint32_t>(v >> 32);
    if (lo) atomicOr(&stream[at >> 5], lo);
    if (hi) atomicOr(&stream[(at >> 5) + 1], hi);
}

// The lengths and canonical codes of one alphabet, by ONE lane: key / order hold the n used symbols ascending by (count, symbol),
// per and next are 16 words of LDS each; length[] is zero on entry.  code[] comes out bit-reversed: ready for put_bits.
__device__ void build_code(uint32_t *key, const uint16_t *order, int n, int n_symbols, uint32_t *per, uint32_t *next, uint8_t *length, uint16_t *code)
{
    for (int d = 0; d < 16; d++) per[d] = 0u;
    if (n == 1) {
        length[order[0]] = 1;
        per[1] = 1u;
    } else if (n >= 2) {
        // Moffat and Katajainen, "In-place calculation of minimum-redundancy codes": key[i] becomes element i's depth
        key[0] += key[1];
        int root = 0, leaf = 2;
        for (int at = 1; at < n - 1; at++) {
            if (leaf >= n || key[root] < key[leaf]) {
                key[at] = key[root];
                key[root++] = static_cast<uint32_t>(at);
            } else {
                key[at] = key[leaf++];
            }
            if (leaf >= n || (root < at && key[root] < key[leaf])) {
                key[at] += key[root];
                key[root++] = static_cast<uint32_t>(at);
            } else {
                key[at] += key[leaf++];
            }
        }
        key[n - 2] = 0u;
        for (int at = n - 3; at >= 0; at--) key[at] = key[key[at]] + 1u;
        int avail = 1, used = 0, at = n - 1;
        uint32_t depth = 0u;
        root = n - 2;
        while (avail > 0) {
            while (root >= 0 && key[root] == depth) {
                used++;
                root--;
            }
            while (avail > used) {
                key[at--] = depth;
                avail--;
            }
            avail = 2 * used, depth++, used = 0;
        }
        // miniz's limit: everything deeper than 15 counts as 15, then the Kraft sum is repaired one unit at a time
        for (int i = 0; i < n; i++) per[key[i] < 15u ? key[i] : 15u]++;
        uint32_t total = 0u;
        for (int d = 1; d <= 15; d++) total += per[d] << (15 - d);
        for (int guard = 0; guard < (1 << 15) && total != (1u << 15); guard++) {
            per[15]--;
            for (int d = 14; d >= 1; d--)
                if (per[d]) {
                    per[d]--;
                    per[d + 1] += 2u;
                    break;
                }
            total--;
        }
        at = n;
        for (int d = 1; d <= 15; d++)
            for (uint32_t c = per[d]; c > 0u; c--) length[order[--at]] = static_cast<uint8_t>(d);
    }
    per[0] = 0u;
    uint32_t first = 0u;
    for (int d = 1; d <= 15; d++) {
        first = (first + per[d - 1]) << 1;
        next[d] = first;
    }
    for (int s = 0; s < n_symbols; s++) {
        const int d = length[s];
        if (d) code[s] = static_cast<uint16_t>(__builtin_bitreverse32(next[d]++) >> (32 - d));
    }
}

__global__ __launch_bounds__(kThreads) void bgzf_deflate_kernel(const uint8_t *__restrict__ payload, int64_t payload_bytes, int block_payload,
                                                                uint8_t *__restrict__ slots, int64_t *__restrict__ block_bytes,
                                                                uint32_t *__restrict__ workspace)
{
    __shared__ uint32_t data[kBlockPayloadMax / 4 + 4];       // the block's bytes, and room for match_length's last words
    __shared__ uint32_t table[1 << (kHashBits - 1)];          // 2^15 uint16: position + 1 per hash, 0: none; then the bitstream
    __shared__ uint32_t tok[kTile];
    __shared__ uint16_t jump[2][kTile];
    __shared__ int entry;                                     // where the chain enters the tile
    __shared__ uint32_t freq[kSymbols], key[kSymbols];
    __shared__ uint16_t order[kSymbols], code[kSymbols];
    __shared__ uint8_t length[kSymbols];
    __shared__ uint32_t crc_table[256], joined[kWaves], wave_bits[kWaves], per[2][16], next[2][16];
    __shared__ uint32_t n_used[2], token_bits;

    const int t = threadIdx.x;
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * block_payload;
    const int64_t left = payload_bytes - begin;                                    // >= 1: the grid is ceil(payload_bytes / block_payload)
    const int len = left < block_payload ? static_cast<int>(left) : block_payload;
    const uint8_t *src = payload + begin;
    uint8_t *dst = slots + static_cast<int64_t>(blockIdx.x) * (block_payload + kBlockExtra);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(data);

    for (int j = t; j < len; j += kThreads) bytes[j] = src[j];
    for (int j = t; j < (1 << (kHashBits - 1)); j += kThreads) table[j] = 0u;
    if (t < 256) crc_table[t] = crc_table_entry(static_cast<uint32_t>(t));
    if (t < kSymbols) freq[t] = 0u, length[t] = 0, code[t] = 0;
    if (t < 2) n_used[t] = 0u;
    if (t == 0) token_bits = 0u, entry = 0;
    __syncthreads();

    {   // the CRC of the block: a slice per thread
        const int slice = (len + kThreads - 1) / kThreads;
        const int first = t * slice < len ? t * slice : len, last = first + slice < len ? first + slice : len;
        uint32_t state = t == 0 ? 0xffffffffu : 0u;
        for (int j = first; j < last; j++) state = crc_table[(state ^ bytes[j]) & 0xffu] ^ (state >> 8);
        if (state != 0u && last < len) state = gf_mul(state, gf_x_pow_bytes(static_cast<unsigned>(len - last)));
#pragma unroll
        for (int off = kLanes / 2; off >= 1; off >>= 1) state ^= __shfl_xor(state, off);
        if ((t & (kLanes - 1)) == 0) joined[t >> 6] = state;
    }

    bool dynamic = false;
    uint32_t deflate_bytes = static_cast<uint32_t>(len) + 5u;
    if (len > kStoredOnly) {
        // ---- 1 and 2: matches and the greedy parse, tile by tile ----
        for (int base = 0; base < len; base += kTile) {
            const int p = base + t;
            const int tile_n = len - base < kTile ? len - base : kTile;
            uint32_t word = 0u;
            const bool hashed = p + 4 <= len;
            uint32_t h = 0u;
            if (p < len) {
                const int cap = len - p < kMaxMatch ? len - p : kMaxMatch;
                int best = 0, dist = 0;
                if (p >= 1) best = match_length(data, p - 1, p, cap), dist = 1;
                if (hashed) {
                    h = (word_at(data, p) * 0x9E3779B1u) >> (32 - kHashBits);
                    const int c = static_cast<int>((table[h >> 1] >> (16 * (h & 1u))) & 0xffffu) - 1;
                    if (c >= 0 && p - c <= kWindow) {
                        const int far = match_length(data, c, p, cap);
                        if (far > best) best = far, dist = p - c;
                    }
                }
                if (best >= 4 || (best == 3 && dist < 4096)) word = static_cast<uint32_t>(best) | static_cast<uint32_t>(dist - 1) << 9;
            }
            const int target = t + ((word & 0x1ffu) ? static_cast<int>(word & 0x1ffu) : 1);      // where the chain goes from here, in the tile
            tok[t] = word;
            jump[0][t] = static_cast<uint16_t>(target < tile_n && t < tile_n ? target : kTile);
            __syncthreads();
            // The chain by pointer jumping: in round k a flagged position flags the one 2^k tokens ahead, and every position's jump
            // doubles; after 10 rounds every start within 1,023 tokens of the entry is flagged — all of them.  A flag is only ever
            // set on a position of the chain, so the set does not depend on which flags a lane sees early.  The table takes the
            // tile's positions beside rounds 0 and 1: even hashes, then odd.
            if (t == entry && t < tile_n) atomicOr(&tok[t], kStart);
#pragma unroll 1
            for (int round = 0; round < 10; round++) {
                if (round == 0 && hashed && (h & 1u) == 0u) atomicMax(&table[h >> 1], (table[h >> 1] & 0xffff0000u) | static_cast<uint32_t>(p + 1));
                if (round == 1 && hashed && (h & 1u) == 1u) atomicMax(&table[h >> 1], (table[h >> 1] & 0xffffu) | static_cast<uint32_t>(p + 1) << 16);
                const uint16_t *now = jump[round & 1];
                const int j = now[t];
                if (j < kTile) {
                    if (tok[t] & kStart) atomicOr(&tok[j], kStart);
                    jump[(round + 1) & 1][t] = now[j];
                } else {
                    jump[(round + 1) & 1][t] = static_cast<uint16_t>(kTile);
                }
                __syncthreads();
            }
            if ((tok[t] & kStart) && target >= kTile) entry = target - kTile;      // the chain's last token of a full tile: one lane
            if (p < len) {
                const uint32_t w = tok[t];
                workspace[begin + p] = w;
                if (w & kStart) {
                    if (w & 0x1ffu) {
                        int symbol, extra;
                        uint32_t value;
                        length_symbol(static_cast<int>(w & 0x1ffu), symbol, extra, value);
                        atomicAdd(&freq[symbol], 1u);
                        dist_symbol(static_cast<int>((w >> 9) & 0x7fffu), symbol, extra, value);
                        atomicAdd(&freq[kDistAt + symbol], 1u);
                    } else {
                        atomicAdd(&freq[bytes[p]], 1u);
                    }
                }
            }
        }
        if (t == 0) freq[256] = 1u;                                                // end of block
        __syncthreads();

        // ---- 3: the codes ----
        {   // rank the used symbols by (count, symbol): lanes 0..285 the literal/length alphabet, 320..349 the distances
            const bool far = t >= kSymbols;
            const int s = far ? t - kSymbols : t, n = far ? kDist : kLitLen, at = far ? kDistAt : 0;
            if (s < n && freq[at + s]) {
                const uint32_t f = freq[at + s];
                int rank = 0;
                for (int u = 0; u < n; u++) {
                    const uint32_t g = freq[at + u];
                    rank += g != 0u && (g < f || (g == f && u < s));
                }
                order[at + rank] = static_cast<uint16_t>(s);
                key[at + rank] = f;
                atomicAdd(&n_used[far], 1u);
            }
        }
        __syncthreads();
        if (t == 0) build_code(key, order, static_cast<int>(n_used[0]), kLitLen, per[0], next[0], length, code);
        if (t == kLanes)
            build_code(key + kDistAt, order + kDistAt, static_cast<int>(n_used[1]), kDist, per[1], next[1], length + kDistAt, code + kDistAt);
        __syncthreads();
        if (t < kLitLen && freq[t]) atomicAdd(&token_bits, freq[t] * static_cast<uint32_t>(length[t] + litlen_extra(t)));
        if (t >= kSymbols && t < kSymbols + kDist && freq[kDistAt + t - kSymbols])
            atomicAdd(&token_bits, freq[kDistAt + t - kSymbols] * static_cast<uint32_t>(length[kDistAt + t - kSymbols] + dist_extra(t - kSymbols)));
        __syncthreads();
        const uint32_t dynamic_bytes = (static_cast<uint32_t>(kHeaderBits) + token_bits + 7u) >> 3;
        dynamic = dynamic_bytes < static_cast<uint32_t>(len) + 5u;                 // strictly shorter, from the exact count
        if (dynamic) deflate_bytes = dynamic_bytes;
    }

    if (dynamic) {
        // ---- 4: the bitstream, in the table's LDS ----
        for (int j = t; j < (1 << (kHashBits - 1)); j += kThreads) table[j] = 0u;
        __syncthreads();
        if (t == 0) put_bits(table, 0u, 1u | 2u << 1 | (kLitLen - 257) << 3 | (kDist - 1) << 8 | (19u - 4u) << 13, 17);
        if (t >= 1 && t <= 19) put_bits(table, 17u + 3u * (t - 1), t <= 3 ? 0u : 4u, 3);      // 16, 17, 18 unused; 0..15 at 4 bits
        if (t >= 32 && t < 32 + kLitLen + kDist) {
            const int i = t - 32;
            const uint32_t n = length[i < kLitLen ? i : kDistAt + i - kLitLen];
            put_bits(table, 17u + 57u + 4u * i, __builtin_bitreverse32(n) >> 28, 4);
        }
        const int first = t * kChunk < len ? t * kChunk : len, last = first + kChunk < len ? first + kChunk : len;
        uint32_t bits = 0u;
        for (int p = first; p < last; p++) {
            const uint32_t w = workspace[begin + p];
            if (!(w & kStart)) continue;
            if (w & 0x1ffu) {
                int symbol, extra;
                uint32_t value;
                length_symbol(static_cast<int>(w & 0x1ffu), symbol, extra, value);
                bits += length[symbol] + extra;
                dist_symbol(static_cast<int>((w >> 9) & 0x7fffu), symbol, extra, value);
                bits += length[kDistAt + symbol] + extra;
            } else {
                bits += length[bytes[p]];
            }
        }
        uint32_t scan = bits;                                                      // inclusive over the wave, then exclusive over the block
#pragma unroll
        for (int off = 1; off < kLanes; off <<= 1) {
            const uint32_t up = __shfl_up(scan, off);
            if ((t & (kLanes - 1)) >= off) scan += up;
        }
        if ((t & (kLanes - 1)) == kLanes - 1) wave_bits[t >> 6] = scan;
        __syncthreads();
        uint32_t at = static_cast<uint32_t>(kHeaderBits) + scan - bits;
        for (int w = 0; w < (t >> 6); w++) at += wave_bits[w];
        for (int p = first; p < last; p++) {
            const uint32_t w = workspace[begin + p];
            if (!(w & kStart)) continue;
            if (w & 0x1ffu) {
                int symbol, extra;
                uint32_t value;
                length_symbol(static_cast<int>(w & 0x1ffu), symbol, extra, value);
                put_bits(table, at, code[symbol] | value << length[symbol], length[symbol] + extra);
                at += length[symbol] + extra;
                dist_symbol(static_cast<int>((w >> 9) & 0x7fffu), symbol, extra, value);
                put_bits(table, at, code[kDistAt + symbol] | value << length[kDistAt + symbol], length[kDistAt + symbol] + extra);
                at += length[kDistAt + symbol] + extra;
            } else {
                const int b = bytes[p];
                put_bits(table, at, code[b], length[b]);
                at += length[b];
            }
        }
        if (t == kThreads - 1) put_bits(table, static_cast<uint32_t>(kHeaderBits) + token_bits - length[256], code[256], length[256]);
        __syncthreads();
        const uint8_t *stream = reinterpret_cast<const uint8_t *>(table);
        for (uint32_t j = t; j < deflate_bytes; j += kThreads) dst[18 + j] = stream[j];
    } else {
        __syncthreads();                                                           // joined[]
        for (int j = t; j < len; j += kThreads) dst[18 + 5 + j] = bytes[j];
        if (t >= 18 && t < 18 + 5) {
            const unsigned long long n = static_cast<unsigned long long>(len);
            const unsigned long long word = 1ull | n << 8 | (~n & 0xffffull) << 24;                              // 01, LEN, ~LEN
            dst[t] = static_cast<uint8_t>(word >> (8 * (t - 18)));
        }
    }
    if (t < 18) {
        const unsigned long long bsize = static_cast<unsigned long long>(18u + deflate_bytes + 8u - 1u);
        const unsigned long long word = t < 8    ? 0x0000000004088b1full                                          // 1f 8b 08 04, MTIME 0
                                        : t < 16 ? 0x000243420006ff00ull                                          // XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0
                                                 : bsize;
        dst[t] = static_cast<uint8_t>(word >> (8 * (t & 7)));
    } else if (t >= 32 && t < 32 + 8) {
        uint32_t crc = 0u;
        for (int w = 0; w < kWaves; w++) crc ^= joined[w];
        const unsigned long long word = static_cast<uint32_t>(~crc) | static_cast<unsigned long long>(len) << 32;  // CRC-32, ISIZE
        dst[18 + deflate_bytes + (t - 32)] = static_cast<uint8_t>(word >> (8 * (t - 32)));
    }
    if (t == 0) block_bytes[blockIdx.x] = static_cast<int64_t>(18u + deflate_bytes + 8u);
}

// Block b from its slot to out + offsets[b].  Every value read from the device is checked before it forms an address.
__global__ __launch_bounds__(kPackThreads) void bgzf_pack_kernel(const uint8_t *__restrict__ slots, int block_payload, const int64_t *__restrict__ offsets,
                                                                 uint8_t *__restrict__ out, int64_t out_bytes, int32_t *__restrict__ refused)
{
    const int64_t lo = offsets[blockIdx.x], hi = offsets[blockIdx.x + 1];
    const int64_t slot = block_payload + kBlockExtra;
    if (lo < 0 || hi < lo || hi - lo > slot || hi > out_bytes) {
        if (threadIdx.x == 0) atomicAdd(refused, 1);
        return;
    }
    const uint8_t *src = slots + static_cast<int64_t>(blockIdx.x) * slot;
    const int n = static_cast<int>(hi - lo);
    for (int j = threadIdx.x; j < n; j += kPackThreads) out[lo + j] = src[j];
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int64_t bgsa_hip_bgzf_deflate_workspace_bytes(int64_t payload_bytes, int block_payload)
{
    if (payload_bytes < 0 || payload_bytes > INT64_MAX / 32 || block_payload < 1 || block_payload > kBlockPayloadMax) return -1;
    return 4 * payload_bytes;                                                      // one word per payload byte
}

int bgsa_hip_bgzf_deflate_dev(const uint8_t *d_payload, int64_t payload_bytes, int block_payload, uint8_t *d_slots, int64_t slots_bytes,
                              int64_t *d_block_bytes, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "bgzf_deflate_dev";
    if (!d_payload || !d_slots || !d_block_bytes || !d_workspace) return refuse(who, BGSA_HIP_EINVAL, "a pointer is NULL");
    if (block_payload < 1 || block_payload > kBlockPayloadMax) return refuse(who, BGSA_HIP_EINVAL, "block_payload must lie in 1..65280");
    const int64_t needed = bgsa_hip_bgzf_deflate_workspace_bytes(payload_bytes, block_payload);
    if (needed < 0) return refuse(who, BGSA_HIP_EINVAL, "payload_bytes is negative or beyond int64 once framed");
    const int64_t n_blocks = (payload_bytes + block_payload - 1) / block_payload;
    if (slots_bytes != n_blocks * (block_payload + kBlockExtra))
        return refuse(who, BGSA_HIP_EINVAL, "slots_bytes is not n_blocks * (block_payload + 31)");
    if (workspace_bytes < needed) return refuse(who, BGSA_HIP_EINVAL, "workspace_bytes is below bgsa_hip_bgzf_deflate_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(d_workspace) & 3u) return refuse(who, BGSA_HIP_EINVAL, "d_workspace is not aligned to 4 bytes");
    if (n_blocks > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "more blocks than one launch holds");
    if (n_blocks == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(static_cast<unsigned>(n_blocks)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_payload,
                       payload_bytes, block_payload, d_slots, d_block_bytes, static_cast<uint32_t *>(d_workspace));
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_bgzf_pack_dev(const uint8_t *d_slots, int block_payload, int64_t n_blocks, const int64_t *d_block_offsets, uint8_t *d_out,
                           int64_t out_bytes, int32_t *d_refused, void *stream)
{
    const char *who = "bgzf_pack_dev";
    if (!d_slots || !d_block_offsets || !d_out || !d_refused) return refuse(who, BGSA_HIP_EINVAL, "a pointer is NULL");
    if (block_payload < 1 || block_payload > kBlockPayloadMax) return refuse(who, BGSA_HIP_EINVAL, "block_payload must lie in 1..65280");
    if (n_blocks < 0 || n_blocks > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "n_blocks is negative or beyond one launch");
    if (out_bytes < 0) return refuse(who, BGSA_HIP_EINVAL, "out_bytes is negative");
    if (n_blocks == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(bgzf_pack_kernel, dim3(static_cast<unsigned>(n_blocks)), dim3(kPackThreads), 0, static_cast<hipStream_t>(stream), d_slots,
                       block_payload, d_block_offsets, d_out, out_bytes, d_refused);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"

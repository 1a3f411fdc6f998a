// pileup.hip — the consumer of the records: per-position base counts of a batch as assembled, and the candidate sites of a
// count matrix reduced on the device (include/bgsa_hip.h "Pileup").  Three kernels, a few words of LDS, no
// scratch, no workspace, vector stores and integer atomics only:
//   pileup_kernel        one WAVE per record, the waves of a resident grid striding over the records.  A record that is malformed
//                        (check_record), unmapped, excluded by its flag or below the MAPQ bound is counted and touches nothing else.
//                        The runs are taken 64 at a time, wave_scan_add giving every run its reference position p and its read
//                        index j (the pattern of walk_runs); a run of up to kSerialBases bases is counted by its own lane, a longer
//                        one by the whole wave, lane t at p + t, + 64, ...  Integer atomicAdd on counts[p][column]: exact whatever
//                        the arrival order.  The five stats are kept per wave, added up per workgroup in LDS and leave as one
//                        atomic per counter and workgroup — one per record on ONE address is what LABNOTES §42.3 measured.
//   sites_count_kernel   one THREAD per position, 256 positions per workgroup: the site test, a ballot per wave, the workgroup's
//                        number of sites.
//   sites_emit_kernel    the same test again; a site's slot is its workgroup's offset (the caller's exclusive scan of the counts)
//                        plus its rank in the workgroup: the ballot's bits below the lane plus the totals of the waves in front,
//                        four words of LDS.  A slot outside [0, n_sites) is not written and counted.
// No value read from device memory forms an address before check_record has compared it with the extent the caller states.
#include "sam_record.h"

namespace bgsa {

namespace {

constexpr int kThreads = 256;
constexpr int kColumns = BGSA_HIP_PILEUP_COLUMNS;
constexpr int kColOther = 4, kColDeleted = 5, kColInserted = 6, kColReverse = 7;
constexpr int kStats = BGSA_HIP_PILEUP_STATS;      // records used, filtered, malformed; bases counted, below the quality bound
constexpr int64_t kMaxPositions = static_cast<int64_t>(INT32_MAX) * kThreads;      // one launch of the site passes

struct Filter {
    int min_mapq, min_base_quality;
    unsigned exclude_flags;
};

constexpr int kDeleted = 0, kCounted = 1, kLow = 2;      // what count_position met

// One reference position p of a run that consumes the reference, read index j: the counts grow, what the base was is returned.
__device__ __forceinline__ int count_position(const Record &r, const Filter &f, bool deleted, long long p, long long j, int32_t *__restrict__ counts)
{
    int32_t *row = counts + p * kColumns;
    int column = kColDeleted;
    if (!deleted) {                             // the record as written: a reverse hit is read from its far end and complemented
        const long long at = r.reverse ? r.read_len - 1 - j : j;
        if (r.qual && static_cast<int>(r.qual[at]) - 33 < f.min_base_quality) return kLow;
        const uint8_t c = r.seq[at];
        const int forward = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : kColOther;
        column = r.reverse && forward < 4 ? 3 - forward : forward;
    }
    atomicAdd(row + column, 1);
    if (r.reverse) atomicAdd(row + kColReverse, 1);
    return deleted ? kDeleted : kCounted;
}

// One record.  Returns 0 used, 1 filtered, 2 malformed (wave-uniform: the index of its counter); counted and low grow by this
// lane's own bases.
__device__ __forceinline__ int pileup_record(const Batch &b, int64_t i, const Filter &f, int32_t *__restrict__ counts, int lane, int &counted,
                                             int &low)
{
    const Record r = check_record<false>(b, Contigs{}, i);
    if (!r.ok) return 2;
    if (!r.mapped || (r.flag & f.exclude_flags) != 0u || static_cast<int>(r.mapq) < f.min_mapq) return 1;      // flag and mapq: the same in every lane
    // checked: the reference-consuming runs sum to [begin, end) inside the reference, the read-consuming ones to read_len
    const long long begin = static_cast<long long>(r.pos) - 1, end = begin + r.ref_bases;
    long long c_ref = 0, c_read = 0;            // what the runs in front of this chunk add up to
    for (int base = 0; base < r.n_ops; base += kLanes) {      // wave-uniform
        const bool mine = base + lane < r.n_ops;
        const uint32_t word = mine ? r.runs[base + lane] : 0u;
        const int op = static_cast<int>(word & 15u);
        const long long len = word >> 4;
        const long long on_ref = mine && op != kOpReadOnly ? len : 0, on_read = mine && op != kOpRefOnly ? len : 0;
        const long long ref_end = c_ref + wave_scan_add(on_ref, lane), read_end = c_read + wave_scan_add(on_read, lane);
        const long long p = begin + ref_end - on_ref, j = read_end - on_read;
        const bool deleted = op == kOpRefOnly;
        if (mine && op == kOpReadOnly) {
            if (p > begin && p < end) atomicAdd(counts + (p - 1) * kColumns + kColInserted, 1);      // once per run; a leading or trailing one nowhere
        } else if (mine && len <= kSerialBases) {
            for (long long t = 0; t < len; t++) {
                const int met = count_position(r, f, deleted, p + t, j + t, counts);
                counted += met == kCounted;
                low += met == kLow;
            }
        }
        unsigned long long wide = __ballot(mine && op != kOpReadOnly && len > kSerialBases);
        while (wide) {                          // wave-uniform: the long runs, one after the other, by all lanes
            const int owner = __ffsll(wide) - 1;
            wide &= wide - 1;
            const long long o_p = __shfl(p, owner), o_j = __shfl(j, owner), o_len = __shfl(len, owner);
            const bool o_deleted = __shfl(op, owner) == kOpRefOnly;
            for (long long t = lane; t < o_len; t += kLanes) {
                const int met = count_position(r, f, o_deleted, o_p + t, o_j + t, counts);
                counted += met == kCounted;
                low += met == kLow;
            }
        }
        c_ref = __shfl(ref_end, kLanes - 1);
        c_read = __shfl(read_end, kLanes - 1);
    }
    return 0;
}

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(kThreads) void pileup_kernel(Batch b, int64_t n, Filter f, int32_t *__restrict__ counts,
                                                          unsigned long long *__restrict__ stats)
{
    __shared__ unsigned long long s_stats[kStats];
    if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
    long long used = 0, filtered = 0, malformed = 0, counted = 0, low = 0;      // the first three wave-uniform, the bases this lane's own
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); i < n; i += n_waves) {
        int record_counted = 0, record_low = 0;      // a lane's share of one record: at most read_len
        const int kind = pileup_record(b, i, f, counts, lane, record_counted, record_low);
        used += kind == 0;
        filtered += kind == 1;
        malformed += kind == 2;
        counted += record_counted;
        low += record_low;
    }
    counted = wave_sum(counted);
    low = wave_sum(low);
    if (lane == 0) {
        if (used) atomicAdd(&s_stats[0], static_cast<unsigned long long>(used));
        if (filtered) atomicAdd(&s_stats[1], static_cast<unsigned long long>(filtered));
        if (malformed) atomicAdd(&s_stats[2], static_cast<unsigned long long>(malformed));
        if (counted) atomicAdd(&s_stats[3], static_cast<unsigned long long>(counted));
        if (low) atomicAdd(&s_stats[4], static_cast<unsigned long long>(low));
    }
    __syncthreads();
    if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_stats[threadIdx.x]);
}

// ---- candidate sites ------------------------------------------------------------------------------------------------------------
struct Thresholds {
    int min_cover, min_alt, min_percent;
};

struct Site {
    bool is;
    int ref, alt, alt_count, cover;
    unsigned mask;
};

// The site test of position p < ref_len, in 64-bit integers.
__device__ __forceinline__ Site site_test(const int32_t *__restrict__ counts, const uint8_t *__restrict__ reference, int64_t p, const Thresholds &th)
{
    const int32_t *row = counts + p * kColumns;
    int c[kColumns - 1];
#pragma unroll
    for (int a = 0; a < kColumns - 1; a++) c[a] = row[a];
    const int ref = reference[p];
    const long long cover = static_cast<long long>(c[0]) + c[1] + c[2] + c[3] + c[4] + c[5];
    Site s{false, ref, -1, 0, static_cast<int>(cover), 0u};
#pragma unroll
    for (int a = 0; a < kColumns - 1; a++) {
        if (a == kColOther || a == ref) continue;
        if (c[a] >= th.min_alt && 100ll * c[a] >= static_cast<long long>(th.min_percent) * cover) {
            s.mask |= 1u << a;
            if (s.alt < 0 || c[a] > s.alt_count) {      // ascending columns: a tie stays with the lowest
                s.alt = a;
                s.alt_count = c[a];
            }
        }
    }
    s.is = ref < 4 && cover >= th.min_cover && s.mask != 0u;
    return s;
}

__global__ __launch_bounds__(kThreads) void sites_count_kernel(const int32_t *__restrict__ counts, const uint8_t *__restrict__ reference,
                                                               int64_t ref_len, Thresholds th, int32_t *__restrict__ block_sites)
{
    __shared__ int s_found;
    if (threadIdx.x == 0) s_found = 0;
    __syncthreads();
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const bool is = p < ref_len && site_test(counts, reference, p, th).is;
    const unsigned long long found = __ballot(is);
    if (found != 0ull && (threadIdx.x & (kLanes - 1)) == 0) atomicAdd(&s_found, __popcll(found));
    __syncthreads();
    if (threadIdx.x == 0) block_sites[blockIdx.x] = s_found;
}

__global__ __launch_bounds__(kThreads) void sites_emit_kernel(const int32_t *__restrict__ counts, const uint8_t *__restrict__ reference,
                                                              int64_t ref_len, Thresholds th, const int64_t *__restrict__ block_offsets,
                                                              int64_t n_sites, int64_t *__restrict__ pos, uint8_t *__restrict__ ref,
                                                              uint8_t *__restrict__ alt, uint8_t *__restrict__ alts_mask,
                                                              int32_t *__restrict__ alt_count, int32_t *__restrict__ cover,
                                                              int32_t *__restrict__ overflow)
{
    __shared__ int s_wave[kWavesPerBlock];
    const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x >> 6;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    Site s{false, 0, 0, 0, 0, 0u};
    if (p < ref_len) s = site_test(counts, reference, p, th);
    const unsigned long long found = __ballot(s.is);
    if (lane == 0) s_wave[wave] = __popcll(found);
    __syncthreads();
    int rank = __popcll(found & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++)
        if (w < wave) rank += s_wave[w];
    const long long slot = block_offsets[blockIdx.x] + rank;
    const bool fits = s.is && slot >= 0 && slot < n_sites;
    if (fits) {
        pos[slot] = p;
        ref[slot] = static_cast<uint8_t>(s.ref);
        alt[slot] = static_cast<uint8_t>(s.alt);
        alts_mask[slot] = static_cast<uint8_t>(s.mask);
        alt_count[slot] = s.alt_count;
        cover[slot] = s.cover;
    }
    const unsigned long long lost = __ballot(s.is && !fits);
    if (lost != 0ull && lane == 0) atomicAdd(overflow, __popcll(lost));
}

int check_sites(const char *who, const void *d_counts, const void *d_reference, int64_t ref_len, int min_cover, int min_alt, int min_percent,
                int64_t n_blocks)
{
    if (!d_counts || !d_reference) return refuse(who, BGSA_HIP_EINVAL, "d_counts or d_reference is NULL");
    if (ref_len < 1 || ref_len > kMaxPositions) return refuse(who, BGSA_HIP_EINVAL, "ref_len is not positive, or beyond one launch");
    if (min_cover < 1 || min_alt < 1) return refuse(who, BGSA_HIP_EINVAL, "min_cover and min_alt must be positive");
    if (min_percent < 0 || min_percent > 100) return refuse(who, BGSA_HIP_EINVAL, "min_percent outside 0..100");
    if (n_blocks != bgsa_hip_pileup_site_blocks(ref_len)) return refuse(who, BGSA_HIP_EINVAL, "n_blocks is not bgsa_hip_pileup_site_blocks(ref_len)");
    return BGSA_HIP_OK;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_pileup_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int min_mapq, int min_base_quality, int exclude_flags, int32_t *d_counts,
                        int64_t *d_stats, void *stream)
{
    const char *who = "pileup_dev";
    if (n < 0) return refuse(who, BGSA_HIP_EINVAL, "n is negative");
    if (int rc = check_batch(who, batch, n, false)) return rc;
    if (!d_counts || !d_stats) return refuse(who, BGSA_HIP_EINVAL, "d_counts or d_stats is NULL");
    if (min_mapq < 0 || min_mapq > 255) return refuse(who, BGSA_HIP_EINVAL, "min_mapq outside 0..255");
    if (min_base_quality < 0 || min_base_quality > 93) return refuse(who, BGSA_HIP_EINVAL, "min_base_quality outside 0..93");
    if (exclude_flags < 0 || exclude_flags > 0xffff) return refuse(who, BGSA_HIP_EINVAL, "exclude_flags outside 0..65535");
    if (n == 0) return BGSA_HIP_OK;
    const int64_t blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock, resident = persistent_blocks();
    const Filter f{min_mapq, min_base_quality, static_cast<unsigned>(exclude_flags)};
    hipLaunchKernelGGL(pileup_kernel, dim3(static_cast<unsigned>(blocks < resident ? blocks : resident)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), *batch, n, f, d_counts, reinterpret_cast<unsigned long long *>(d_stats));
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int64_t bgsa_hip_pileup_site_blocks(int64_t ref_len)
{
    return ref_len < 1 ? 0 : (ref_len + kThreads - 1) / kThreads;
}

int bgsa_hip_pileup_sites_count_dev(const int32_t *d_counts, const uint8_t *d_reference, int64_t ref_len, int min_cover, int min_alt,
                                    int min_percent, int32_t *d_block_sites, int64_t n_blocks, void *stream)
{
    const char *who = "pileup_sites_count_dev";
    if (int rc = check_sites(who, d_counts, d_reference, ref_len, min_cover, min_alt, min_percent, n_blocks)) return rc;
    if (!d_block_sites) return refuse(who, BGSA_HIP_EINVAL, "d_block_sites is NULL");
    hipLaunchKernelGGL(sites_count_kernel, dim3(static_cast<unsigned>(n_blocks)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_counts,
                       d_reference, ref_len, Thresholds{min_cover, min_alt, min_percent}, d_block_sites);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_pileup_sites_emit_dev(const int32_t *d_counts, const uint8_t *d_reference, int64_t ref_len, int min_cover, int min_alt,
                                   int min_percent, const int64_t *d_block_offsets, int64_t n_blocks, int64_t n_sites, int64_t *d_pos,
                                   uint8_t *d_ref, uint8_t *d_alt, uint8_t *d_alts_mask, int32_t *d_alt_count, int32_t *d_cover,
                                   int32_t *d_overflow, void *stream)
{
    const char *who = "pileup_sites_emit_dev";
    if (int rc = check_sites(who, d_counts, d_reference, ref_len, min_cover, min_alt, min_percent, n_blocks)) return rc;
    if (!d_block_offsets || !d_pos || !d_ref || !d_alt || !d_alts_mask || !d_alt_count || !d_cover || !d_overflow)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (n_sites < 0) return refuse(who, BGSA_HIP_EINVAL, "n_sites is negative");
    hipLaunchKernelGGL(sites_emit_kernel, dim3(static_cast<unsigned>(n_blocks)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_counts,
                       d_reference, ref_len, Thresholds{min_cover, min_alt, min_percent}, d_block_offsets, n_sites, d_pos, d_ref, d_alt,
                       d_alts_mask, d_alt_count, d_cover, d_overflow);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"

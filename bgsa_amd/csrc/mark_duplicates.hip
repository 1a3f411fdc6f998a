// mark_duplicates.hip — flag 0x400 on the duplicate reads and pairs of ONE batch before its records are written (include/bgsa_hip.h
// "Duplicate marking"; the Picard core: no optical duplicates, no UMIs, no libraries).  Two kernels, a few
// words of LDS, no scratch, vector stores only:
//   dup_keys_kernel  one WAVE per unit (`ends` records) of the batch as assembled, the waves of a resident grid striding over the
//                    units: the lanes stride over the unit's QUAL bytes and reduce the thresholded sum; lane 0 writes every
//                    record's end key, the unit's score and its pair key.  Pair units, fragment units and malformed records are
//                    counted per wave and added up per workgroup: one atomic per counter and workgroup — one per unit on ONE
//                    address took 1.1 ms for 100,000 reads (LABNOTES §42.3).
//   dup_mark_kernel  one THREAD per SORTED entry: an entry whose key equals its predecessor's is a duplicate; it ORs 1024 into
//                    the flag of its records, found through the permutation; a wave counts its duplicates by one ballot, a
//                    workgroup adds them up.  The same kernel serves the pair pass and the end pass.
// Between the two the caller orders the entries by (key ascending, score descending, index ascending) with stable sorts
// (bgsa_amd/reference.py: mark_duplicate_records).  No value read from device memory forms an address before it has been compared
// with the extent the caller states: a malformed record takes its whole unit out of marking and touches nothing.
#include "sam_record.h"

namespace bgsa {

namespace {

constexpr int kThreads = 256;
constexpr long long kCoordinateReach = 1ll << 60;          // a 5' coordinate below this leaves room for the strand and the tag
constexpr int kDuplicate = 0x400;

struct End {
    bool ok, mapped;
    long long five;             // the 5' coordinate of a mapped record
    int strand, read_len;
    long long row;
};

// The scalars of record i that marking reads, each compared with its extent.  Wave-uniform.
__device__ __forceinline__ End check_end(const Batch &b, int64_t i)
{
    End e{false, false, 0, -1, 0, 0};
    const long long row = uniform_i64(b.d_read_row[i]);
    const int read_len = __builtin_amdgcn_readfirstlane(b.d_read_len[i]);
    const int strand = __builtin_amdgcn_readfirstlane(b.d_strand[i]);
    if (strand < -1 || strand > 1 || read_len < 0 || read_len > b.read_stride || row < 0 || row >= b.n_read_rows) return e;
    e.strand = strand;
    e.read_len = read_len;
    e.row = row;
    if (strand >= 0) {
        const long long begin = uniform_i64(b.d_ref_begin[i]), end = uniform_i64(b.d_ref_end[i]);
        if (begin < 0 || end < begin || end > b.ref_len) return e;
        e.mapped = true;
        e.five = strand == 1 && end > begin ? end - 1 : begin;
    }
    e.ok = true;
    return e;
}

// The sum of q - 33 over the record's QUAL bytes with q - 33 >= min_quality, by the whole wave; every lane gets it.
__device__ __forceinline__ long long quality_sum(const Batch &b, const End &e, int min_quality, int lane)
{
    const uint8_t *qual = b.d_quals + e.row * b.read_stride;
    long long sum = 0;
    for (int j = lane; j < e.read_len; j += kLanes) {
        const int q = static_cast<int>(qual[j]) - 33;
        if (q >= min_quality) sum += q;
    }
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    return sum;
}

// One unit: the checks, the score, the keys written by lane 0; the wave's counts of pair units, fragment units and malformed
// records grow by what the unit is.
template <int ENDS>
__device__ __forceinline__ void unit_keys(const Batch &b, int64_t u, int min_quality, int lane, int64_t *__restrict__ end_key,
                                          int32_t *__restrict__ score, int64_t *__restrict__ pair_key_a, int64_t *__restrict__ pair_key_b,
                                          int *n_pairs, int *n_fragments, int *n_malformed)
{
    End e[ENDS];
    int bad = 0, mapped = 0;
#pragma unroll
    for (int k = 0; k < ENDS; k++) {
        e[k] = check_end(b, u * ENDS + k);
        bad += !e[k].ok;
        mapped += e[k].ok && e[k].mapped;
    }
    const bool paired = ENDS == 2 && bad == 0 && mapped == 2;
    long long sum = 0;
    if (bad == 0 && b.d_quals) {
#pragma unroll
        for (int k = 0; k < ENDS; k++)
            if (e[k].mapped) sum += quality_sum(b, e[k], min_quality, lane);
    }
    *n_malformed += bad;
    if (bad == 0) *(paired ? n_pairs : n_fragments) += paired ? 1 : mapped;
    if (lane != 0) return;
    long long half[ENDS];
#pragma unroll
    for (int k = 0; k < ENDS; k++) {
        const bool entry = bad == 0 && e[k].mapped;
        half[k] = e[k].five << 1 | (e[k].strand & 1);
        end_key[u * ENDS + k] = entry ? half[k] << 1 | (paired ? 0 : 1) : LLONG_MAX;
    }
    score[u] = static_cast<int32_t>(sum > INT_MAX ? INT_MAX : sum);
    const bool first = half[0] <= half[ENDS - 1];
    pair_key_a[u] = paired ? (first ? half[0] : half[ENDS - 1]) : LLONG_MAX;
    pair_key_b[u] = paired ? (first ? half[ENDS - 1] : half[0]) : LLONG_MAX;
}

template <int ENDS>
__global__ __launch_bounds__(kThreads) void dup_keys_kernel(Batch b, int64_t n_units, int min_quality, int64_t *__restrict__ end_key,
                                                            int32_t *__restrict__ score, int64_t *__restrict__ pair_key_a,
                                                            int64_t *__restrict__ pair_key_b, int32_t *__restrict__ counts)
{
    __shared__ int s_counts[3];
    if (threadIdx.x < 3) s_counts[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
    int mine[3] = {0, 0, 0};                    // wave-uniform
    for (int64_t u = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); u < n_units; u += n_waves)
        unit_keys<ENDS>(b, u, min_quality, lane, end_key, score, pair_key_a, pair_key_b, &mine[0], &mine[1], &mine[2]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (mine[k]) atomicAdd(&s_counts[k], mine[k]);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_counts[threadIdx.x]) atomicAdd(counts + threadIdx.x, s_counts[threadIdx.x]);
}

// PAIRS: entry j of the order is a unit (records 2e, 2e + 1) and the key has two halves; else it is a record and its key's low bit
// is the fragment tag: the comparison leaves it out, and only a tagged entry is flagged.
template <bool PAIRS>
__global__ __launch_bounds__(kThreads) void dup_mark_kernel(const int64_t *__restrict__ key_a, const int64_t *__restrict__ key_b,
                                                            const int64_t *__restrict__ order, int64_t m, int64_t n,
                                                            int32_t *__restrict__ flag, int32_t *__restrict__ counts)
{
    __shared__ int s_found;
    if (threadIdx.x == 0) s_found = 0;
    __syncthreads();
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    bool duplicate = false;
    long long e = 0;
    if (j >= 1 && j < m) {                      // entry 0 heads its group
        const long long mine = key_a[j], before = key_a[j - 1];
        e = order[j];
        if (mine != LLONG_MAX && e >= 0 && e < m)      // INT64_MAX: no entry, these sort last
            duplicate = PAIRS ? mine == before && key_b[j] == key_b[j - 1] && 2 * e + 1 < n : (mine >> 1) == (before >> 1) && (mine & 1) && e < n;
    }
    if (duplicate) {
        if (PAIRS) {
            flag[2 * e] |= kDuplicate;
            flag[2 * e + 1] |= kDuplicate;
        } else {
            flag[e] |= kDuplicate;
        }
    }
    const unsigned long long found = __ballot(duplicate);
    if (found != 0ull && (threadIdx.x & (kLanes - 1)) == __ffsll(found) - 1) atomicAdd(&s_found, __popcll(found));
    __syncthreads();
    if (threadIdx.x == 0 && s_found) {          // one pair of atomics per workgroup, as in the key kernel
        atomicAdd(counts + (PAIRS ? 0 : 1), s_found);
        atomicAdd(counts + 2, PAIRS ? 2 * s_found : s_found);
    }
}

int check_ends(const char *who, int64_t n, int ends)
{
    if (n < 0) return refuse(who, BGSA_HIP_EINVAL, "n is negative");
    if (ends != 1 && ends != 2) return refuse(who, BGSA_HIP_EINVAL, "ends is neither 1 nor 2");
    if (ends == 2 && (n & 1)) return refuse(who, BGSA_HIP_EINVAL, "n is odd with ends 2: records 2u and 2u + 1 are pair u");
    return BGSA_HIP_OK;
}

constexpr int64_t kMaxEntries = static_cast<int64_t>(INT32_MAX) * kThreads;      // one launch

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_dup_keys_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int ends, int min_quality, int64_t *d_end_key, int32_t *d_score,
                          int64_t *d_pair_key_a, int64_t *d_pair_key_b, int32_t *d_counts, void *stream)
{
    const char *who = "dup_keys_dev";
    if (int rc = check_ends(who, n, ends)) return rc;
    if (int rc = check_batch(who, batch, n, false)) return rc;
    if (!d_end_key || !d_score || !d_pair_key_a || !d_pair_key_b || !d_counts) return refuse(who, BGSA_HIP_EINVAL, "an output pointer is NULL");
    if (min_quality < 0 || min_quality > 93) return refuse(who, BGSA_HIP_EINVAL, "min_quality outside 0..93");
    if (batch->ref_len > kCoordinateReach) return refuse(who, BGSA_HIP_EINVAL, "ref_len beyond 2^60: the key has no room for it");
    if (n == 0) return BGSA_HIP_OK;
    const int64_t n_units = n / ends;
    const int64_t blocks = (n_units + kWavesPerBlock - 1) / kWavesPerBlock, resident = persistent_blocks();
    const dim3 grid(static_cast<unsigned>(blocks < resident ? blocks : resident));
    if (ends == 2)
        hipLaunchKernelGGL(dup_keys_kernel<2>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), *batch, n_units, min_quality, d_end_key,
                           d_score, d_pair_key_a, d_pair_key_b, d_counts);
    else
        hipLaunchKernelGGL(dup_keys_kernel<1>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), *batch, n_units, min_quality, d_end_key,
                           d_score, d_pair_key_a, d_pair_key_b, d_counts);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_dup_mark_dev(const int64_t *d_key_a, const int64_t *d_key_b, const int64_t *d_order, int64_t n, int ends, int32_t *d_flag,
                          int32_t *d_counts, void *stream)
{
    const char *who = "dup_mark_dev";
    if (int rc = check_ends(who, n, ends)) return rc;
    if (!d_key_a || (ends == 2 && !d_key_b) || !d_order || !d_flag || !d_counts)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream, and d_key_b with ends 1, may be NULL)");
    const int64_t m = n / ends;
    if (m > kMaxEntries) return refuse(who, BGSA_HIP_EINVAL, "n beyond one launch");
    if (n == 0) return BGSA_HIP_OK;
    const dim3 grid(static_cast<unsigned>((m + kThreads - 1) / kThreads));
    if (ends == 2)
        hipLaunchKernelGGL(dup_mark_kernel<true>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_key_a, d_key_b, d_order, m, n,
                           d_flag, d_counts);
    else
        hipLaunchKernelGGL(dup_mark_kernel<false>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_key_a, d_key_b, d_order, m, n,
                           d_flag, d_counts);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"

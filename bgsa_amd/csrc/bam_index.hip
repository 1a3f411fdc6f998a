// bam_index.hip — what a coordinate-sorted BAM needs beside its records (include/bgsa_hip.h "BAM records: coordinate order and
// index"; SAMv1 §5.2): the sort keys and coordinates of a batch, and from the SORTED coordinates the arrays of
// a BAI index.  Three kernels, one THREAD per record, bandwidth-bound, no LDS, no scratch, vector stores only:
//   bam_coordinates_kernel  key, refID, pos, end and bin of record i of the batch as assembled; a malformed record gets the last key
//                           and is counted.  The record's scalars go through the range checks of sam_record.h's check_record, per
//                           lane here (check_record is one wave per record and walks the runs; this pass does not).
//   bam_index_marks_kernel  the virtual offsets of record i, whether it starts a chunk, and its windows of the linear index by a
//                           64-bit atomicMin; a record that fails a check is counted and touches nothing.
//   bam_index_chunks_kernel a chunk's first record writes its refID, bin and begin, its last record its end.
// The caller sorts the keys, gathers, scans the chunk starts and sorts the chunks (bgsa_amd/reference.py: sam_records).  No value
// read from device memory forms an address before it has been compared with the extent the caller states.
#include "sam_record.h"

namespace bgsa {

namespace {

constexpr int kThreads = 256;
constexpr long long kBaiReach = 1ll << 29;                 // a BAI's bins and windows end here
constexpr long long kNoCoordinate = 0x7fffffffll;          // ref' of a record without coordinates: it sorts last
constexpr int kUnplacedBin = 4680;                         // reg2bin(-1, 0)

// reg2bin of the specification (SAMv1 §5.3) for [beg, end), 0 <= beg < end <= 2^29, in full.
__device__ __forceinline__ int reg2bin_full(long long beg, long long end)
{
    --end;
    if (beg >> 14 == end >> 14) return static_cast<int>(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return static_cast<int>(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return static_cast<int>(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return static_cast<int>(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return static_cast<int>(1 + (beg >> 26));
    return 0;
}

// sam_record.h's locate for ONE lane: the contig that holds the linear position `at`, by the same rules.
__device__ __forceinline__ bool locate_lane(const Contigs &ct, long long ref_len, long long at, int *contig, long long *start, long long *end)
{
    int lo = 0, hi = static_cast<int>(ct.n_contigs);      // the contigs whose start is <= at are [0, lo)
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ct.d_starts[mid] <= at) lo = mid + 1; else hi = mid;
    }
    if (lo < 1) return false;
    const int c = lo - 1;
    const long long s = ct.d_starts[c], n = ct.d_lens[c];
    if (s < 0 || n < 1 || s > ref_len - n || at >= s + n) return false;
    const long long name_lo = ct.d_name_offsets[c], name_hi = ct.d_name_offsets[c + 1];
    if (name_lo < 0 || name_hi <= name_lo || name_hi > ct.names_bytes) return false;
    *contig = c;
    *start = s;
    *end = s + n;
    return true;
}

struct Coordinates {
    bool ok;
    int ref_id;
    long long pos, end;
};

template <bool CONTIGS>
__device__ __forceinline__ Coordinates coordinates_of(const Batch &b, const Contigs &ct, int64_t i)
{
    Coordinates out{false, -1, -1, 0};
    const int strand = b.d_strand[i], rnext = b.d_rnext[i];
    const long long pnext = b.d_pnext[i];
    if (strand < -1 || strand > 1 || (rnext != 0 && rnext != 1) || pnext < 0 || (rnext == 1 && pnext < 1)) return out;
    int ref_id = -1;
    long long pos = -1, end = 0;
    if (rnext == 1) {                           // the mate's place: an unmapped end takes it
        int contig = 0;
        long long start = 0, stop = 0;
        if (CONTIGS && !locate_lane(ct, b.ref_len, pnext - 1, &contig, &start, &stop)) return out;
        ref_id = contig;
        pos = pnext - 1 - start;
        end = pos + 1;
    }
    if (strand >= 0) {
        const long long begin = b.d_ref_begin[i], stop = b.d_ref_end[i];
        if (begin < 0 || stop < begin || stop > b.ref_len) return out;
        int contig = 0;
        long long start = 0, contig_end = 0;
        if (CONTIGS && (!locate_lane(ct, b.ref_len, begin, &contig, &start, &contig_end) || stop > contig_end)) return out;
        ref_id = contig;
        pos = begin - start;
        end = pos + (stop > begin ? stop - begin : 1);      // a record of no reference base counts one, as its bin does
    }
    if (pos + 1 > kBaiReach || end > kBaiReach) return out;
    out = Coordinates{true, ref_id, pos, end};
    return out;
}

template <bool CONTIGS>
__global__ __launch_bounds__(kThreads) void bam_coordinates_kernel(Batch b, Contigs ct, int64_t n, int64_t *__restrict__ key,
                                                                   int32_t *__restrict__ ref_id, int32_t *__restrict__ pos,
                                                                   int32_t *__restrict__ end, int32_t *__restrict__ bin,
                                                                   int32_t *__restrict__ malformed)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const Coordinates c = coordinates_of<CONTIGS>(b, ct, i);
    if (!c.ok) {
        atomicAdd(malformed, 1);
        key[i] = LLONG_MAX;
        ref_id[i] = -1;
        pos[i] = -1;
        end[i] = 0;
        bin[i] = kUnplacedBin;
        return;
    }
    const long long reverse = (b.d_flag[i] >> 4) & 1;
    key[i] = (c.ref_id < 0 ? kNoCoordinate : static_cast<long long>(c.ref_id)) << 32 | (c.pos + 1) << 1 | reverse;
    ref_id[i] = c.ref_id;
    pos[i] = static_cast<int32_t>(c.pos);
    end[i] = static_cast<int32_t>(c.end);
    bin[i] = c.pos < 0 ? kUnplacedBin : reg2bin_full(c.pos, c.end);
}

template <bool CONTIGS>
int launch_coordinates(const Batch *batch, const Contigs &ct, int64_t n, int64_t *d_key, int32_t *d_ref_id, int32_t *d_pos, int32_t *d_end,
                       int32_t *d_bin, int32_t *d_malformed, void *stream)
{
    hipLaunchKernelGGL(bam_coordinates_kernel<CONTIGS>, dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), *batch, ct, n, d_key, d_ref_id, d_pos, d_end, d_bin, d_malformed);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

struct Blocks {
    long long payload_bytes, n_blocks;
    int block_payload;
    const int64_t *offsets;                     // n_blocks + 1 entries, or NULL: stored blocks
};

// The virtual offset of payload offset o, 0 <= o <= payload_bytes and o / P <= n_blocks.
__device__ __forceinline__ long long virtual_offset(const Blocks &bl, long long o)
{
    const long long block = o / bl.block_payload, within = o - block * bl.block_payload;
    const long long start = bl.offsets ? bl.offsets[block] : block * (bl.block_payload + 31ll);
    return start << 16 | within;
}

__global__ __launch_bounds__(kThreads) void bam_index_marks_kernel(const int32_t *__restrict__ ref_id, const int32_t *__restrict__ pos,
                                                                   const int32_t *__restrict__ end, const int32_t *__restrict__ bin, int64_t n,
                                                                   const int64_t *__restrict__ offsets, Blocks bl,
                                                                   const int64_t *__restrict__ window_base, int64_t n_refs,
                                                                   int64_t *__restrict__ voff_beg, int64_t *__restrict__ voff_end,
                                                                   int32_t *__restrict__ chunk_start, int64_t *__restrict__ linear,
                                                                   int32_t *__restrict__ refused)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const int r = ref_id[i];
    const long long p = pos[i], e = end[i];
    const long long lo = offsets[i], hi = offsets[i + 1];
    bool ok = r >= -1 && r < n_refs && lo >= 0 && hi >= lo && hi <= bl.payload_bytes && hi / bl.block_payload <= bl.n_blocks;
    long long base = 0;
    if (ok && r >= 0) {
        const long long total = window_base[n_refs], next = window_base[r + 1];
        base = window_base[r];
        ok = p >= 0 && e > p && base >= 0 && next >= base && next <= total && ((e - 1) >> 14) < next - base;
    }
    const bool first = i == 0;
    const int before_ref = first ? 0 : ref_id[i - 1];
    const long long before_pos = first ? 0 : pos[i - 1], before_end = first ? 0 : end[i - 1];
    if (ok && !first) {                         // the (ref', pos) order of the keys
        const long long mine = r < 0 ? kNoCoordinate : r, theirs = before_ref < 0 ? kNoCoordinate : before_ref;
        ok = theirs < mine || (theirs == mine && before_pos <= p);
    }
    if (!ok) {
        atomicAdd(refused, 1);
        chunk_start[i] = 0;
        return;
    }
    const long long beg = virtual_offset(bl, lo);
    voff_beg[i] = beg;
    voff_end[i] = virtual_offset(bl, hi);
    chunk_start[i] = r >= 0 && (first || before_ref != r || bin[i - 1] != bin[i]) ? 1 : 0;
    if (r < 0) return;
    // a window the predecessor on the same reference covers already holds a smaller offset
    long long w = p >> 14;
    if (!first && before_ref == r && before_end > before_pos) {
        const long long covered = ((before_end - 1) >> 14) + 1;
        if (covered > w) w = covered;
    }
    for (const long long last = (e - 1) >> 14; w <= last; w++)
        atomicMin(reinterpret_cast<unsigned long long *>(linear + base + w), static_cast<unsigned long long>(beg));
}

__global__ __launch_bounds__(kThreads) void bam_index_chunks_kernel(const int32_t *__restrict__ ref_id, const int32_t *__restrict__ bin,
                                                                    const int64_t *__restrict__ voff_beg, const int64_t *__restrict__ voff_end,
                                                                    const int32_t *__restrict__ chunk_start, const int64_t *__restrict__ chunk_of,
                                                                    int64_t n, int64_t n_chunks, int32_t *__restrict__ chunk_ref,
                                                                    int32_t *__restrict__ chunk_bin, int64_t *__restrict__ chunk_beg,
                                                                    int64_t *__restrict__ chunk_end, int32_t *__restrict__ refused)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const int r = ref_id[i];
    if (r < 0) return;                          // no chunk holds a record without coordinates
    const bool starts = chunk_start[i] != 0;
    const bool ends = i + 1 == n || chunk_start[i + 1] != 0 || ref_id[i + 1] < 0;
    if (!starts && !ends) return;
    const long long c = chunk_of[i];
    if (c < 1 || c > n_chunks) {
        atomicAdd(refused, 1);
        return;
    }
    if (starts) {
        chunk_ref[c - 1] = r;
        chunk_bin[c - 1] = bin[i];
        chunk_beg[c - 1] = voff_beg[i];
    }
    if (ends) chunk_end[c - 1] = voff_end[i];
}

int check_coordinates_out(const char *who, const int64_t *d_key, const int32_t *d_ref_id, const int32_t *d_pos, const int32_t *d_end,
                          const int32_t *d_bin, const int32_t *d_malformed)
{
    if (!d_key || !d_ref_id || !d_pos || !d_end || !d_bin || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "an output pointer is NULL");
    return BGSA_HIP_OK;
}

constexpr int64_t kMaxRecords = static_cast<int64_t>(INT32_MAX) * kThreads;      // one launch

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_bam_coordinates_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int64_t *d_key, int32_t *d_ref_id, int32_t *d_pos,
                                 int32_t *d_end, int32_t *d_bin, int32_t *d_malformed, void *stream)
{
    const char *who = "bam_coordinates_dev";
    if (int rc = check_batch(who, batch, n)) return rc;
    if (int rc = check_coordinates_out(who, d_key, d_ref_id, d_pos, d_end, d_bin, d_malformed)) return rc;
    if (n == 0) return BGSA_HIP_OK;
    return launch_coordinates<false>(batch, Contigs{}, n, d_key, d_ref_id, d_pos, d_end, d_bin, d_malformed, stream);
}

int bgsa_hip_bam_coordinates_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, int64_t *d_key,
                                         int32_t *d_ref_id, int32_t *d_pos, int32_t *d_end, int32_t *d_bin, int32_t *d_malformed, void *stream)
{
    const char *who = "bam_coordinates_contigs_dev";
    if (int rc = check_contig_batch(who, batch, contigs, n)) return rc;
    if (int rc = check_coordinates_out(who, d_key, d_ref_id, d_pos, d_end, d_bin, d_malformed)) return rc;
    if (n == 0) return BGSA_HIP_OK;
    return launch_coordinates<true>(batch, *contigs, n, d_key, d_ref_id, d_pos, d_end, d_bin, d_malformed, stream);
}

int64_t bgsa_hip_bam_index_windows(const int64_t *ref_lens, int64_t n_refs, int64_t *window_base_out)
{
    if (!ref_lens || !window_base_out || n_refs < 0) return -1;
    int64_t total = 0;
    for (int64_t c = 0; c < n_refs; c++) {
        if (ref_lens[c] < 1 || ref_lens[c] > kBaiReach) return -1;
        window_base_out[c] = total;
        total += (ref_lens[c] + 16383) >> 14;
    }
    window_base_out[n_refs] = total;
    return total;
}

int bgsa_hip_bam_index_marks_dev(const int32_t *d_ref_id, const int32_t *d_pos, const int32_t *d_end, const int32_t *d_bin, int64_t n,
                                 const int64_t *d_offsets, int64_t payload_bytes, int block_payload, const int64_t *d_block_offsets,
                                 int64_t n_blocks, const int64_t *d_window_base, int64_t n_refs, int64_t *d_voff_beg, int64_t *d_voff_end,
                                 int32_t *d_chunk_start, int64_t *d_linear, int32_t *d_refused, void *stream)
{
    const char *who = "bam_index_marks_dev";
    if (!d_ref_id || !d_pos || !d_end || !d_bin || !d_offsets || !d_window_base || !d_voff_beg || !d_voff_end || !d_chunk_start || !d_linear ||
        !d_refused)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only d_block_offsets and the stream may be NULL)");
    if (n < 0 || n > kMaxRecords) return refuse(who, BGSA_HIP_EINVAL, "n is negative or beyond one launch");
    if (payload_bytes < 0 || n_blocks < 0 || n_refs < 0 || n_refs > static_cast<int64_t>(INT32_MAX))
        return refuse(who, BGSA_HIP_EINVAL, "payload_bytes, n_blocks or n_refs is negative, or n_refs beyond 2^31 - 1");
    if (block_payload < 1 || block_payload > 65280) return refuse(who, BGSA_HIP_EINVAL, "block_payload outside 1..65280");
    if (n == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(bam_index_marks_kernel, dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_ref_id, d_pos, d_end, d_bin, n, d_offsets,
                       Blocks{payload_bytes, n_blocks, block_payload, d_block_offsets}, d_window_base, n_refs, d_voff_beg, d_voff_end,
                       d_chunk_start, d_linear, d_refused);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_bam_index_chunks_dev(const int32_t *d_ref_id, const int32_t *d_bin, const int64_t *d_voff_beg, const int64_t *d_voff_end,
                                  const int32_t *d_chunk_start, const int64_t *d_chunk_of, int64_t n, int64_t n_chunks,
                                  int32_t *d_chunk_ref, int32_t *d_chunk_bin, int64_t *d_chunk_beg, int64_t *d_chunk_end,
                                  int32_t *d_refused, void *stream)
{
    const char *who = "bam_index_chunks_dev";
    if (!d_ref_id || !d_bin || !d_voff_beg || !d_voff_end || !d_chunk_start || !d_chunk_of || !d_chunk_ref || !d_chunk_bin || !d_chunk_beg ||
        !d_chunk_end || !d_refused)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (n < 0 || n > kMaxRecords || n_chunks < 0) return refuse(who, BGSA_HIP_EINVAL, "n or n_chunks is negative, or n beyond one launch");
    if (n == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(bam_index_chunks_kernel, dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_ref_id, d_bin, d_voff_beg, d_voff_end, d_chunk_start, d_chunk_of, n, n_chunks,
                       d_chunk_ref, d_chunk_bin, d_chunk_beg, d_chunk_end, d_refused);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"

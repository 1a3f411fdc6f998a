// sam_record.h — what the record stages share (internal, not installed): sam_records.hip writes a record as a line of SAM text,
// bam_records.hip the same record in BAM's binary layout.  Here: the checked record (Record, check_record, locate), the walk over
// its runs (walk_runs: the lengths, and the CIGAR and MD of either format), the wave scans and decimal helpers under it, and the
// host-side checks of a batch.  Everything sits in an unnamed namespace: each of the two translation units gets its own copy.
// Ids, coordinates, lengths and runs are values until checked (check_record): none forms an address before it has been compared
// with the extent the caller states.
#pragma once

#include "bgsa_common.h"

#include <limits.h>

namespace bgsa {

namespace {

using Batch = bgsa_hip_sam_batch_t;
using Contigs = bgsa_hip_sam_contigs_t;

constexpr int kSerialBases = 4;      // an X or D run up to this long is written by its own lane
constexpr int kOpRefOnly = 1, kOpReadOnly = 2, kOpEqual = 7, kOpDiff = 8;   // the project's run codes: 1 prints as SAM D, 2 as SAM I
constexpr int kWalkMeasure = 0, kWalkSamText = 1, kWalkBamWords = 2;        // what walk_runs writes: nothing, CIGAR text + MD, CIGAR words + MD

__device__ const unsigned long long kPow10[20] = {
    1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
    100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
    100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};

// Decimal digits of v, by comparison: no division.
__device__ __forceinline__ int dec_width32(uint32_t v)
{
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
__device__ __forceinline__ int dec_width(unsigned long long v)
{
    if (v <= 0xffffffffull) return dec_width32(static_cast<uint32_t>(v));
    int w = 10;
#pragma unroll
    for (int i = 10; i < 20; i++) w += v >= kPow10[i];
    return w;
}

// v in decimal at out, lane j writing digit j; returns the width.  All lanes call it with the same v.
__device__ __forceinline__ int put_dec(uint8_t *out, unsigned long long v, int lane)
{
    const int w = dec_width(v);
    if (lane < w) {
        const unsigned long long p = kPow10[w - 1 - lane];
        const unsigned digit = v <= 0xffffffffull ? (static_cast<uint32_t>(v) / static_cast<uint32_t>(p)) % 10u
                                                  : static_cast<unsigned>((v / p) % 10ull);
        out[lane] = static_cast<uint8_t>('0' + digit);
    }
    return w;
}
// ... by ONE lane, for a value of its own (a run length, a count of '=' bases).
__device__ __forceinline__ void put_dec_serial(uint8_t *out, unsigned long long v, int w)
{
    for (int i = w - 1; i >= 0; i--) {
        out[i] = static_cast<uint8_t>('0' + static_cast<unsigned>(v % 10ull));
        v /= 10ull;
    }
}

__device__ __forceinline__ long long wave_scan_add(long long v, int lane)      // inclusive
{
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) {
        const long long up = __shfl_up(v, off);
        if (lane >= off) v += up;
    }
    return v;
}
__device__ __forceinline__ long long wave_scan_max(long long v, int lane)      // inclusive
{
#pragma unroll
    for (int off = 1; off < kLanes; off <<= 1) {
        const long long up = __shfl_up(v, off);
        if (lane >= off && up > v) v = up;
    }
    return v;
}

__device__ __forceinline__ uint8_t class_letter(uint8_t code)      // "ACGTN"[code], the four letters packed into one word
{
    return code < 4 ? static_cast<uint8_t>(0x54474341u >> (8 * code)) : 'N';
}

// The letters of one X run (letter, then "0" letter per further base) or D run ('^', then the letters) behind its count, bases
// first, first + step, ...: the run's own lane with (0, 1), the whole wave with (lane, 64).
__device__ __forceinline__ void put_md_letters(uint8_t *out, bool diff, long long len, const uint8_t *ref, long long first, int step)
{
    if (!diff && first == 0) out[0] = '^';
    for (long long t = first; t < len; t += step) {
        const uint8_t letter = class_letter(ref[t]);
        if (diff) {
            if (t > 0) out[2 * t - 1] = '0';
            out[2 * t] = letter;
        } else {
            out[1 + t] = letter;
        }
    }
}

// A 32-bit word at any byte address, low byte first.
__device__ __forceinline__ void put_u32(uint8_t *out, uint32_t v)
{
    out[0] = static_cast<uint8_t>(v);
    out[1] = static_cast<uint8_t>(v >> 8);
    out[2] = static_cast<uint8_t>(v >> 16);
    out[3] = static_cast<uint8_t>(v >> 24);
}

struct Walk {
    long long cigar_bytes, md_bytes, ref_bases, read_bases;
    bool ok;         // every run has a known op and a positive length
};

// The runs of one record, 64 at a time.  EMIT kWalkMeasure: the widths and the sums, nothing read but the runs.  The other two
// (only after a measuring walk has shown that the reference-consuming runs sum to the checked interval at `ref`) also write the
// MD text at md_out and the CIGAR at cigar_out: kWalkSamText as SAM text, kWalkBamWords as BAM's words len << 4 | op (ref-only D 2,
// read-only I 1, '=' 7, X 8), four bytes per run at any byte address.  n_ops is wave-uniform.
template <int EMIT>
__device__ __forceinline__ Walk walk_runs(const uint32_t *runs, int n_ops, const uint8_t *ref, uint8_t *cigar_out, uint8_t *md_out, int lane)
{
    long long c_cigar = 0, c_md = 0, c_ref = 0, c_read = 0, c_eq = 0, c_break = 0;   // what the runs in front of this chunk add up to
    bool ok = true;
    for (int base = 0; base < n_ops; base += kLanes) {      // wave-uniform
        const bool mine = base + lane < n_ops;
        const uint32_t word = mine ? runs[base + lane] : 0u;
        const int op = static_cast<int>(word & 15u);
        const long long len = word >> 4;
        const bool known = op == kOpRefOnly || op == kOpReadOnly || op == kOpEqual || op == kOpDiff;
        if (__ballot(mine && !(known && len > 0)) != 0ull) ok = false;
        const bool live = mine && known && len > 0;
        const bool breaks = live && (op == kOpDiff || op == kOpRefOnly);      // a run MD writes: X bases, or a SAM D
        const long long on_ref = live && op != kOpReadOnly ? len : 0, on_read = live && op != kOpRefOnly ? len : 0;
        const long long equal = live && op == kOpEqual ? len : 0;
        const int digits = dec_width32(static_cast<uint32_t>(len));
        const long long cigar_w = live ? digits + 1 : 0;
        const long long cigar_end = c_cigar + wave_scan_add(cigar_w, lane);
        const long long ref_end = c_ref + wave_scan_add(on_ref, lane);
        const long long read_end = c_read + wave_scan_add(on_read, lane);
        const long long eq_end = c_eq + wave_scan_add(equal, lane);
        const long long break_end = wave_scan_max(breaks ? eq_end : c_break, lane);      // the '=' total at the last X or D run so far
        long long break_before = __shfl_up(break_end, 1);
        if (lane == 0) break_before = c_break;
        const unsigned long long pending = static_cast<unsigned long long>(eq_end - equal - break_before);   // '=' bases MD has not written yet
        const int pending_w = dec_width(pending);
        const long long md_w = breaks ? pending_w + (op == kOpDiff ? 2 * len - 1 : 1 + len) : 0;
        const long long md_end = c_md + wave_scan_add(md_w, lane);
        if (EMIT != kWalkMeasure) {
            if (EMIT == kWalkSamText && live) {
                uint8_t *at = cigar_out + (cigar_end - cigar_w);
                put_dec_serial(at, static_cast<unsigned long long>(len), digits);
                at[digits] = op == kOpEqual ? '=' : op == kOpDiff ? 'X' : op == kOpRefOnly ? 'D' : 'I';
            }
            if (EMIT == kWalkBamWords && live)
                put_u32(cigar_out + 4ll * (base + lane), (word & ~15u) | static_cast<uint32_t>(op == kOpRefOnly ? 2 : op == kOpReadOnly ? 1 : op));
            uint8_t *letters = md_out + (md_end - md_w) + pending_w;
            const uint8_t *bases = ref + (ref_end - on_ref);
            if (breaks) {
                put_dec_serial(md_out + (md_end - md_w), pending, pending_w);
                if (len <= kSerialBases) put_md_letters(letters, op == kOpDiff, len, bases, 0, 1);
            }
            unsigned long long wide = __ballot(breaks && len > kSerialBases);
            while (wide) {                               // wave-uniform: the long runs, one after the other, by all lanes
                const int owner = __ffsll(wide) - 1;
                wide &= wide - 1;
                uint8_t *o_letters = reinterpret_cast<uint8_t *>(__shfl(reinterpret_cast<unsigned long long>(letters), owner));
                const uint8_t *o_bases = reinterpret_cast<const uint8_t *>(__shfl(reinterpret_cast<unsigned long long>(bases), owner));
                put_md_letters(o_letters, __shfl(op, owner) == kOpDiff, __shfl(len, owner), o_bases, lane, kLanes);
            }
        }
        c_cigar = __shfl(cigar_end, kLanes - 1);
        c_ref = __shfl(ref_end, kLanes - 1);
        c_read = __shfl(read_end, kLanes - 1);
        c_eq = __shfl(eq_end, kLanes - 1);
        c_break = __shfl(break_end, kLanes - 1);
        c_md = __shfl(md_end, kLanes - 1);
    }
    const unsigned long long last = static_cast<unsigned long long>(c_eq - c_break);      // the count MD ends with
    if (EMIT != kWalkMeasure) put_dec(md_out + c_md, last, lane);
    return Walk{c_cigar, c_md + dec_width(last), c_ref, c_read, ok};
}

// One record's scalars, every one compared with the extent it will index.  All wave-uniform.
struct Record {
    bool ok, mapped, reverse, mate_named;
    const uint8_t *name, *seq, *qual, *ref;
    const uint8_t *rname, *rnext;         // RNAME where the record is named; RNEXT where it is a name of its own (else '=' or '*')
    long long rname_len, rnext_len;
    const uint32_t *runs;
    int name_len, read_len, n_ops;
    long long cigar_bytes, md_bytes;      // of a mapped record: what its runs print as
    long long ref_bases;                  // of a mapped record: ref_end - ref_begin
    unsigned flag, mapq, distance;
    unsigned long long pos, pnext, tlen_abs;
    bool tlen_negative;
    int ref_id, next_ref_id;              // what BAM writes where SAM prints RNAME and RNEXT: the contig's index (0 on one sequence), -1 for '*'
};

__device__ __forceinline__ long long uniform_i64(long long v) { return static_cast<long long>(uniform_u64(static_cast<unsigned long long>(v))); }

// The contig that holds the linear position `at` (include/bgsa_hip.h "a reference of several contigs"): a binary search on the
// starts, every index inside [0, n_contigs).  False where `at` lies on padding or a table entry is outside the reference.
struct Located {
    int contig;
    long long start, end;
    const uint8_t *name;
    long long name_len;
};

__device__ __forceinline__ bool locate(const Contigs &ct, long long ref_len, long long at, Located *out)
{
    int lo = 0, hi = static_cast<int>(ct.n_contigs);      // the contigs whose start is <= at are [0, lo)
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (uniform_i64(ct.d_starts[mid]) <= at) lo = mid + 1; else hi = mid;
    }
    if (lo < 1) return false;
    const int c = lo - 1;
    const long long start = uniform_i64(ct.d_starts[c]), n = uniform_i64(ct.d_lens[c]);
    if (start < 0 || n < 1 || start > ref_len - n || at >= start + n) return false;
    const long long name_lo = uniform_i64(ct.d_name_offsets[c]), name_hi = uniform_i64(ct.d_name_offsets[c + 1]);
    if (name_lo < 0 || name_hi <= name_lo || name_hi > ct.names_bytes) return false;
    *out = Located{c, start, start + n, ct.d_names + name_lo, name_hi - name_lo};
    return true;
}

// CONTIGS: ref_begin, ref_end and pnext of the batch are linear; RNAME, POS, RNEXT and PNEXT are those of the contig form.
template <bool CONTIGS>
__device__ __forceinline__ Record check_record(const Batch &b, const Contigs &ct, int64_t i)
{
    Record r{};
    const long long row = uniform_i64(b.d_read_row[i]), name = uniform_i64(b.d_name_of[i]);
    const int read_len = __builtin_amdgcn_readfirstlane(b.d_read_len[i]);
    const int strand = __builtin_amdgcn_readfirstlane(b.d_strand[i]);
    const int flag = b.d_flag[i], mapq = b.d_mapq[i];      // the same in every lane, and left in vector registers: only digits come of them
    const int rnext = __builtin_amdgcn_readfirstlane(b.d_rnext[i]);
    const long long pnext = b.d_pnext[i], tlen = b.d_tlen[i];
    if (row < 0 || row >= b.n_read_rows || read_len < 1 || read_len > b.read_stride) return r;
    if (name < 0 || name >= b.n_names) return r;
    const long long name_lo = uniform_i64(b.d_name_offsets[name]), name_hi = uniform_i64(b.d_name_offsets[name + 1]);
    if (name_lo < 0 || name_hi <= name_lo || name_hi > b.names_bytes || name_hi - name_lo > INT_MAX) return r;
    if (strand < -1 || strand > 1 || flag < 0 || flag > 0xffff || mapq < 0 || mapq > 255 || (rnext != 0 && rnext != 1) || pnext < 0 ||
        tlen == LLONG_MIN)
        return r;
    r.mapped = strand >= 0;
    r.reverse = strand == 1;
    r.mate_named = rnext == 1;
    r.name = b.d_names + name_lo;
    r.name_len = static_cast<int>(name_hi - name_lo);
    r.seq = b.d_reads + row * b.read_stride;
    r.qual = b.d_quals ? b.d_quals + row * b.read_stride : nullptr;
    r.read_len = read_len;
    r.flag = static_cast<unsigned>(flag);
    r.mapq = r.mapped ? static_cast<unsigned>(mapq) : 0u;
    r.pnext = static_cast<unsigned long long>(pnext);
    r.tlen_negative = tlen < 0;
    r.tlen_abs = static_cast<unsigned long long>(tlen < 0 ? -tlen : tlen);
    r.rname = b.d_rname;
    r.rname_len = b.rname_len;
    Located mate{-1, 0, 0, nullptr, 0};
    if (CONTIGS && r.mate_named) {              // pnext is the mate's linear begin + 1
        if (pnext < 1 || !locate(ct, b.ref_len, pnext - 1, &mate)) return r;
        r.pnext = static_cast<unsigned long long>(pnext - mate.start);
        r.rname = mate.name;                    // of an unmapped end; a mapped one takes its own below
        r.rname_len = mate.name_len;
    }
    r.pos = r.mate_named ? r.pnext : 0ull;      // an unmapped end of a pair takes its mapped mate's RNAME and POS
    r.next_ref_id = r.mate_named ? (CONTIGS ? mate.contig : 0) : -1;
    r.ref_id = r.mapped ? 0 : r.next_ref_id;
    if (r.mapped) {
        const long long begin = uniform_i64(b.d_ref_begin[i]), end = uniform_i64(b.d_ref_end[i]);
        const long long runs_row = uniform_i64(b.d_runs_row[i]);
        const int n_ops = __builtin_amdgcn_readfirstlane(b.d_n_ops[i]), distance = b.d_distance[i];
        if (n_ops < 0 || n_ops > b.cigar_cap || begin < 0 || end < begin || end > b.ref_len || distance < 0) return r;
        if (runs_row < 0 || runs_row >= b.n_run_rows) return r;
        r.runs = b.d_runs + runs_row * b.cigar_cap;
        r.n_ops = n_ops;
        r.ref = b.d_reference + begin;
        r.distance = static_cast<unsigned>(distance);
        r.pos = static_cast<unsigned long long>(begin) + 1ull;
        if (CONTIGS) {                          // inside ONE contig, or malformed
            Located own;
            if (!locate(ct, b.ref_len, begin, &own) || end > own.end) return r;
            r.pos = static_cast<unsigned long long>(begin - own.start) + 1ull;
            r.rname = own.name;
            r.rname_len = own.name_len;
            r.ref_id = own.contig;
            if (r.mate_named && mate.contig != own.contig) {
                r.rnext = mate.name;
                r.rnext_len = mate.name_len;
            }
        }
        const Walk w = walk_runs<kWalkMeasure>(r.runs, n_ops, nullptr, nullptr, nullptr, threadIdx.x & (kLanes - 1));
        if (!w.ok || w.ref_bases != end - begin || w.read_bases != read_len) return r;
        r.cigar_bytes = w.cigar_bytes;
        r.md_bytes = w.md_bytes;
        r.ref_bases = w.ref_bases;
    }
    r.ok = true;
    return r;
}

__device__ __forceinline__ void count_malformed(int32_t *malformed, int lane)
{
    if (lane == 0) atomicAdd(malformed, 1);
}

// ---- checks --------------------------------------------------------------------------------------------------------------------
int check_batch(const char *who, const Batch *b, int64_t n, bool one_name = true)
{
    if (!b) return refuse(who, BGSA_HIP_EINVAL, "the batch is NULL");
    if (n < 0 || n > static_cast<int64_t>(INT32_MAX) * kWavesPerBlock) return refuse(who, BGSA_HIP_EINVAL, "n is negative or beyond one launch");
    if (!b->d_reads || !b->d_names || !b->d_name_offsets || (one_name && !b->d_rname) || !b->d_reference || !b->d_runs || !b->d_read_row || !b->d_name_of ||
        !b->d_runs_row || !b->d_read_len || !b->d_strand || !b->d_ref_begin || !b->d_ref_end || !b->d_distance || !b->d_n_ops || !b->d_flag ||
        !b->d_mapq || !b->d_rnext || !b->d_pnext || !b->d_tlen)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer in the batch (only d_quals may be NULL)");
    if (b->read_stride < 1 || b->read_stride > static_cast<int64_t>(INT32_MAX) || b->n_read_rows < 1)
        return refuse(who, BGSA_HIP_EINVAL, "read_stride must lie in [1, 2^31 - 1] and n_read_rows be positive");
    if (b->n_names < 1 || b->names_bytes < 1) return refuse(who, BGSA_HIP_EINVAL, "n_names and names_bytes must be positive");
    if (one_name && b->rname_len < 1) return refuse(who, BGSA_HIP_EINVAL, "rname_len is not positive");
    if (b->ref_len < 1) return refuse(who, BGSA_HIP_EINVAL, "ref_len is not positive");
    if (b->cigar_cap < 1 || b->n_run_rows < 1) return refuse(who, BGSA_HIP_EINVAL, "cigar_cap and n_run_rows must be positive");
    return BGSA_HIP_OK;
}

// The contig form's batch (d_rname and rname_len are not read: RNAME comes from the table) and its table.  mark_duplicates.hip
// has no contig form, hence maybe_unused.
[[maybe_unused]] int check_contig_batch(const char *who, const Batch *b, const Contigs *ct, int64_t n)
{
    if (int rc = check_batch(who, b, n, false)) return rc;
    if (!ct) return refuse(who, BGSA_HIP_EINVAL, "the contig table is NULL");
    if (!ct->d_names || !ct->d_name_offsets || !ct->d_starts || !ct->d_lens) return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer in the contig table");
    if (ct->n_contigs < 1 || ct->n_contigs > static_cast<int64_t>(INT32_MAX) || ct->names_bytes < 1)
        return refuse(who, BGSA_HIP_EINVAL, "n_contigs must lie in [1, 2^31 - 1] and the table's names_bytes be positive");
    return BGSA_HIP_OK;
}

}  // namespace

}  // namespace bgsa

/*
 * bgsa_hip.h — C ABI of the MI355X (gfx950) backend for BGSA's all-pairs bit-parallel global
 * alignment hot path.  Everything here is `extern "C"`, plain pointers and sizes.
 *
 * The library is a drop-in "ISA backend" in the sense of the reference's original/BGSA_<ARCH>
 * directories: it exports the same three seams every backend exports —
 *
 *     <arch>_handle_reads      (reference original/BGSA_CPU/global.h:24,  global.c:25-70)
 *     align_<arch>             (reference original/BGSA_CPU/align_core.h:8, align_core.c:19-148)
 *     <arch>_cal_align_score   (reference original/BGSA_CPU/cal.h:48,      cal_cpu.c:43-85)
 *
 * with <arch> = hip, plus the five scoring ints every align_core.c defines
 * (align_core.c:13-17) and the alphabet map (global.c:7-15).  Those entry points take HOST
 * buffers, exactly like the reference's.  Underneath them sits a device-resident layer
 * (bgsa_hip_*_dev) that a pipeline driver uses to keep subjects and scores in HBM between
 * calls, the way the reference's KNC backend keeps them on the coprocessor
 * (original/BGSA_KNC/cal_mic.c:86-154, 348-356).
 *
 * Error convention: the BGSA-surface functions are `void` and print + exit(1) on failure, like
 * the reference (file.c:13-16).  The bgsa_hip_* functions return 0 on success or a negative
 * BGSA_HIP_E* code and never exit.
 */
#ifndef BGSA_HIP_H
#define BGSA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- config.h-style constants (reference original/BGSA_CPU/config.h:6-27) ------------------ */
#define BGSA_CHAR_NUM 5            /* CHAR_NUM: A C G T N planes */
#define HIP_V_NUM 64               /* subjects per group = lanes of one wavefront */
#define HIP_WORD_SIZE 32           /* bits per bit-vector word; all 32 carry data (full_bits = 1) */
#define HIP_BANDED_WORD_SIZE 64    /* widest banded window (k <= 31), as in the reference */
#define HIP_MAX_ERROR 127          /* MAX_ERROR, banded/BGSA_CPU/config.h:19 */
typedef uint32_t hip_read_t;       /* element of the preprocessed Peq blocks */
typedef uint32_t hip_data_t;       /* element of the (unused) dvdh_bit_mem scratch */
typedef int16_t hip_write_t;       /* common_write_t of original/ (Myers, BitPAl) */
typedef int8_t hip_banded_write_t; /* common_write_t of banded/ */

/* seq_t, reference original/BGSA_CPU/global.h:9-16 (same field order and types). */
#ifndef BGSA_HAVE_SEQ_T
#define BGSA_HAVE_SEQ_T
typedef struct _seq_t {
    int len;
    int64_t size;
    int64_t count;
    int extra_size;
    int extra_count;
    char *content;
} seq_t;
#endif

/* ---- algorithm selection -------------------------------------------------------------------
 * The reference bakes the algorithm into the generated align_core.c; one backend directory =
 * one algorithm.  This library carries all three and switches at run time. */
enum {
    BGSA_ALGO_MYERS = 0,  /* unit-cost global edit distance, result = -distance (int16) */
    BGSA_ALGO_BANDED = 1, /* banded Myers filter, result = band distance or 127 (int8) */
    BGSA_ALGO_BITPAL = 2, /* BitPAl packed, match 2 / mismatch -3 / gap -5 unless bgsa_hip_select_scores() (int16) */
};

/* The five ints every align_core.c exports (reference original/BGSA_CPU/align_core.c:13-17);
 * bgsa_hip_select_algorithm() keeps them consistent with the selected algorithm. */
extern int match_score;
extern int mismatch_score;
extern int gap_score;
extern int dvdh_len;
extern int full_bits;
/* -k of banded/BGSA_CPU (banded/BGSA_CPU/global.h:43, main.c:43,62-64). */
extern int threshold;
/* Host threads used by hip_handle_reads (reference global `cpu_threads`, main.c:16,38). */
extern int cpu_threads;

/* Alphabet map (reference original/BGSA_CPU/global.c:7-15). */
extern uint32_t mapping_table[128];
void init_mapping_table(void);

/* 64-byte aligned host allocation (reference global.c:17-23). */
void *malloc_mem(uint64_t size);
void free_mem(void *mem);

int bgsa_hip_select_algorithm(int algo);
int bgsa_hip_current_algorithm(void);

/* BitPAl with other integer scores (match > mismatch, gap < 0).  The reference emits one
 * align_core.c per score set with its generator (`java -jar generator.jar -M -I -G`, README.md:26-82,
 * generator/.../BitPAlGenerator.java) and is rebuilt for it; this library is built with a list of
 * sets (`make -C bgsa_amd/csrc BITPAL_SETS="2,-3,-5 1,-3,-2 ..."`, gen_bitpal_sets.py) and picks the
 * kernels of the set that match_score / mismatch_score / gap_score name at call time.
 * bgsa_hip_select_scores() = select BGSA_ALGO_BITPAL and set the three ints, or
 * BGSA_HIP_EUNSUPPORTED (ints unchanged) if that set was not compiled in; scoring with ints that
 * name no compiled set fails the same way.  bgsa_hip_score_set() enumerates the compiled sets
 * (index 0 = the reference's committed 2/-3/-5); valu_per_word = VALU instructions per (row, 32
 * columns) of that set's kernel.  Any out-pointer may be NULL.
 * Like the generator (commonFactor, Main.java:213-267), scores with a common factor f run on the set
 * (M/f, I/f, G/f) and the result is multiplied by f: 4/-6/-10 needs only 2/-3/-5 compiled in.
 * A mismatch below 2*gap can never be taken (two gaps are cheaper), so such a set runs as its
 * mismatch = 2*gap instance: 1/-9/-2 needs 1/-4/-2.  A set that reduces to 0/-1/-1 — minus the edit
 * distance times f, the generator's isEdit case (Main.java:270-271) — runs, in global mode, on the Myers
 * kernels (10 instructions per word against 22) and needs no compiled BitPAl set at all.
 * bgsa_hip_select_scores(0, 1, 1) is the generator's `-m 1`: BGSA_ALGO_MYERS reporting +distance
 * instead of -distance (the same ints written directly while Myers is selected do the same). */
int bgsa_hip_select_scores(int match, int mismatch, int gap);
int bgsa_hip_score_set_count(void);
int bgsa_hip_score_set(int index, int *match, int *mismatch, int *gap, int *valu_per_word);

/* Global (default) or semi-global scoring — the generator's `-s` option (Configuration.isSemiGlobal).
 * The two generators orient it differently, and so does this library:
 *   BGSA_ALGO_BITPAL (BitPAlGenerator.java:2201-2218 first row, :78-116 last-row maximum): the QUERY is
 *     aligned end to end, subject overhangs before and after it are free; result = max over the last DP
 *     row.  Any compiled score set, any length.
 *   BGSA_ALGO_MYERS (MyersGenerator.java:56-223 genSemiGlobal): the SUBJECT is aligned end to end inside
 *     the query (D[0][y] = 0, result = -min over y of D[slen][y]); any length (generated-asm kernels:
 *     resident Peq planes up to 800 bp, code planes up to 1024 bp, column blocks beyond).
 *   BGSA_ALGO_BANDED: not defined, BGSA_HIP_EUNSUPPORTED.
 * Process-global like the score ints. */
enum { BGSA_ALIGN_GLOBAL = 0, BGSA_ALIGN_SEMIGLOBAL = 1 };
int bgsa_hip_select_alignment(int mode);
int bgsa_hip_current_alignment(void);

/* Every parameter the scoring call reads, as one value.  The reference keeps them in globals of the
 * backend (the five ints, `threshold`); bgsa_hip_cal_align_score_dev() and the host seams snapshot those
 * globals once per call, and callers that must not share process-wide state (two pipelines with
 * different scores in one process) pass their own through the *_ex entry points instead. */
typedef struct bgsa_hip_params {
    int algo;                 /* BGSA_ALGO_* */
    int alignment;            /* BGSA_ALIGN_* */
    int match, mismatch, gap; /* BitPAl scores; Myers: (0,1,1) = +distance, anything else -distance */
    int k;                    /* banded threshold */
} bgsa_hip_params_t;
int bgsa_hip_current_params(bgsa_hip_params_t *out);   /* the process-global selection, as of now */

/* word_num of this backend's layouts: Myers / BitPAl ceil(subject_len / 32) (cal_cpu.c:252-253 with
 * full_bits); banded ceil(subject_len / 32) + 3 words of the offset match string (the host seams also
 * accept the reference's own banded value, banded/BGSA_CPU/cal_cpu.c:253-254 — see hip_handle_reads). */
int bgsa_hip_word_num(int algo, int query_len, int subject_len, int k);
/* hip_read_t elements per group of HIP_V_NUM subjects = BGSA_CHAR_NUM * word_num * HIP_V_NUM. */
size_t bgsa_hip_group_words(int algo, int word_num, int k);

/* ---- BGSA backend surface (host buffers) ---------------------------------------------------
 * align_hip / hip_cal_align_score share one set of device mirrors inside the library and take turns on
 * it: they may be called from several host threads, as the reference's OpenMP loop calls align_<arch>
 * (cal_cpu.c:63-84), but the calls are serialised; each call reads the global selection (algorithm,
 * scores, alignment mode, threshold) once, under that lock.  bgsa_hip_release_workspace() frees the
 * mirrors.
 *
 * Resident buckets.  hip_handle_reads() remembers the host range it filled; the first scoring call on
 * that range uploads it, later calls on it (the reference scores 100 queries per call against the same
 * bucket, cal_cpu.c:363-401) reuse the device copy until hip_handle_reads() writes the range again —
 * the KNC backend's `nocopy ... RETAIN` (BGSA_KNC/cal_mic.c:348-356).  The query buffer is uploaded
 * only when its bytes changed.  A host that fills Peq words by other means must either call
 * bgsa_hip_bucket_resident() after every change or switch the mechanism off with
 * bgsa_hip_set_auto_resident(0) (upload on every call, the stateless contract of the CPU backends).
 * malloc_mem() hands out page-locked memory for large blocks, so every buffer of the reference's
 * pipeline (cal_cpu.c:206-267) moves at full PCIe rate. */
int bgsa_hip_set_auto_resident(int on);
/* THE CONTRACT of a resident range: between the hip_handle_reads() / bgsa_hip_bucket_resident() call that registered it
 * and its release, its host bytes change ONLY through those two calls, and the memory stays allocated while any thread is
 * inside a scoring call on it (the reference's pipeline does both: cal_cpu.c:363-401 fills a bucket with
 * cpu_handle_reads and frees it after its compute threads have joined).  The host range is the truth; the device copy
 * is a cache of it.
 * What the library does for a caller that breaks the contract (a memcpy of a saved bucket over the registered buffer, a
 * host that patches Peq words in place):
 *   - ranges up to 8 MiB (every range in strict mode): EXACT.  The library keeps the host bytes it uploaded and every
 *     scoring call — hip_cal_align_score, and align_hip on its locked and its lock-free path — compares the bytes it is
 *     about to use against them (memcmp, < 1 ms for a whole 8 MiB bucket); any difference uploads the range again and
 *     drops the rows cached from the old content;
 *   - larger ranges: BEST EFFORT.  Every scoring call fingerprints the range (66 cache lines: first, last and a
 *     golden-ratio sequence of positions between them) and uploads it again when the fingerprint differs from the one
 *     taken at upload.  A rewrite that leaves all sampled lines unchanged (a few groups patched in place) is not seen.
 * bgsa_hip_set_strict_resident(1) / BGSA_HIP_STRICT_RESIDENT=1: the exact check for every range (costs a host copy of
 * each bucket and a memcmp per call); (0): the default above; (-1) / BGSA_HIP_STRICT_RESIDENT=-1: the fingerprint alone
 * (measurement).  Switching the mode re-uploads every range on its next use and drops the cached rows.
 * bgsa_hip_stale_ranges() counts the re-uploads either check caused.  (SURVEY 8(b) "Ownership";
 * BGSA_KNC/cal_mic.c:348-356.) */
int bgsa_hip_set_strict_resident(int on);
int bgsa_hip_stale_ranges(uint64_t *count);
/* host_peq[0 .. bytes) holds whole groups in the library's own layout with word_num words. */
int bgsa_hip_bucket_resident(const hip_read_t *host_peq, size_t bytes, int word_num);
int bgsa_hip_bucket_release(const hip_read_t *host_peq);   /* NULL: all of them */
/* Counters of the seams since process start (any pointer may be NULL). */
int bgsa_hip_seam_stats(uint64_t *calls, uint64_t *peq_uploads, uint64_t *peq_upload_bytes);
/* align_hip's row cache: the reference's grid calls align_<arch> once per (query, chunk of ~27 groups)
 * (cal_cpu.c:63-84).  With the chunk inside a resident bucket, the first call for a query scores it
 * against the whole bucket in one launch and keeps that row (page-locked host memory, at most 1 GiB of
 * rows, least recently used first out); the other calls for the same query, bucket and parameters copy
 * their chunk out of it.  When the misses walk a malloc_mem() query buffer row after row, the rows behind
 * the requested one that no launch has scored yet join its launch and the next launch is issued ahead of the
 * calls (BGSA_HIP_ROW_AHEAD, default 32 rows per launch, 1 = off); a row is only served for a query with the
 * same bytes.  hip_cal_align_score scores its
 * block in BGSA_HIP_SEAM_TILES (default 8) query tiles and copies tile t out while tile t+1 runs.
 * hits / misses (= launches) since process start. */
int bgsa_hip_row_cache_stats(uint64_t *hits, uint64_t *misses);

/* ASCII rows -> Peq blocks, layout [group][char 0..4][word][lane 0..63]
 * (replaces cpu_handle_reads, reference original/BGSA_CPU/global.c:25-70; for BGSA_ALGO_BANDED
 * the words hold the match string offset by threshold+1 bits, which is what the windows of
 * banded/BGSA_CPU/global.c:25-84 + align_core.c:35-62 slide over).  result_reads must be zeroed by the caller (cal_cpu.c:273)
 * and read_count must be a multiple of HIP_V_NUM (file.c:84-112 pads with all-'N' reads).
 * word_num = bgsa_hip_word_num(); for BGSA_ALGO_BANDED also the reference's own value,
 * (len - h + 63)/64 + 1 words of its 64-bit cpu_read_t (banded/BGSA_CPU/cal_cpu.c:253-254): that
 * buffer holds the same bit string without the trailing zero words, and hip_cal_align_score / align_hip
 * called with the same word_num re-pitch it on upload — so banded/BGSA_CPU's host files work unchanged. */
void hip_handle_reads(seq_t *read_seq, hip_read_t *result_reads, int word_num,
                      int64_t read_start, int64_t read_count);

/* One mapped query against chunk_read_num consecutive groups
 * (replaces align_cpu, reference original/BGSA_CPU/align_core.c:19-148).
 * results[(result_index + k) * HIP_V_NUM + lane].  dvdh_bit_mem is accepted and ignored. */
void align_hip(char *ref, hip_read_t *read, int ref_len, int read_len, int word_num,
               int chunk_read_num, int result_index, hip_write_t *results,
               hip_data_t *dvdh_bit_mem);

/* All queries [ref_start, ref_end) x all read_count subjects of the bucket, row-major
 * [ref][read] results (replaces cpu_cal_align_score, reference cal_cpu.c:43-85).
 * For BGSA_ALGO_BANDED align_results is really hip_banded_write_t*. */
void hip_cal_align_score(char *content, hip_read_t *preprocess_reads, hip_write_t *align_results,
                         int ref_len, int ref_count, int read_len, int read_count, int ref_start,
                         int ref_end, int word_num, int chunk_read_num, hip_data_t *dvdh_bit_mem);

int bgsa_hip_release_workspace(void);

/* ---- device-resident layer ----------------------------------------------------------------- */

#define BGSA_HIP_OK 0
#define BGSA_HIP_EINVAL (-1)      /* bad argument (null pointer, negative size, misaligned count) */
#define BGSA_HIP_EUNSUPPORTED (-2) /* length / threshold outside what the kernels cover */
#define BGSA_HIP_EHIP (-3)        /* a HIP runtime call failed; text via bgsa_hip_last_error() */

const char *bgsa_hip_last_error(void);
int bgsa_hip_device_count(void);
int bgsa_hip_set_device(int device);

/* Plain device memory helpers so C hosts need no HIP headers. */
int bgsa_hip_malloc(void **dptr, size_t bytes);
/* free and total memory of the current device (hipMemGetInfo); either pointer may be NULL */
int bgsa_hip_mem_info(size_t *free_bytes, size_t *total_bytes);
int bgsa_hip_free(void *dptr);
/* Page-locked host memory (full-rate asynchronous copies for the pipeline driver). */
int bgsa_hip_malloc_host(void **hptr, size_t bytes);
int bgsa_hip_free_host(void *hptr);
int bgsa_hip_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int bgsa_hip_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int bgsa_hip_memset(void *dst, int value, size_t bytes, void *stream);
int bgsa_hip_stream_create(void **stream);   /* on the current device */
int bgsa_hip_stream_destroy(void *stream);
int bgsa_hip_stream_synchronize(void *stream);
/* Events: per-device kernel times for the dynamic balancing of the command line (BGSA_KNC/global.c:120-168). */
int bgsa_hip_event_create(void **event);
int bgsa_hip_event_destroy(void *event);
int bgsa_hip_event_record(void *event, void *stream);
int bgsa_hip_event_synchronize(void *event);
int bgsa_hip_event_elapsed_ms(void *start, void *stop, float *ms);
int bgsa_hip_stream_wait_event(void *stream, void *event);

/* Subject preprocess ON the GPU: d_rows = read_count rows of (len+1) ASCII bytes in device
 * memory -> d_peq in the layout above.  read_count must be a multiple of HIP_V_NUM.
 * `avail_bytes` = readable bytes of d_rows (banded over-read guard).  Overwrites d_peq. */
int bgsa_hip_handle_reads_dev(int algo, const char *d_rows, int64_t avail_bytes, int len,
                              int64_t read_count, int word_num, int k, hip_read_t *d_peq,
                              void *stream);

/* Query bytes -> 0..4 in place on the device ('\n' kept), get_ref_from_file's map
 * (reference original/BGSA_CPU/file.c:134-139). */
int bgsa_hip_map_queries_dev(char *d_content, int64_t bytes, void *stream);

/* Scratch the hot path needs for n_queries queries of ref_len characters against subjects of
 * read_len characters: the queries re-packed into 8-byte-aligned code streams the kernels fetch
 * through the scalar cache, plus, for subjects too long for the register-resident kernels (Myers
 * > 1024 bp, BitPAl beyond the plain widths of the selected score set, > 352 bp for 2/-3/-5), the
 * per-wave carry words of the column-block kernels, plus the task counter of the launches whose waves
 * take their (subject group, query tile) tasks from it.  Depends on the selected score set.  A workspace
 * belongs to ONE launch at a time: launches that may overlap (two streams) need one each. */
size_t bgsa_hip_workspace_bytes(int algo, int ref_len, int read_len, int n_queries);

/* The hot path.  d_content = mapped query rows, stride ref_len+1 (reference cal_cpu.c:78);
 * d_peq = Peq blocks of read_count subjects; d_results = [ref_end-ref_start][read_count]
 * (int16, or int8 for banded).  d_workspace = caller-owned device scratch of at least
 * bgsa_hip_workspace_bytes(algo, ref_len, read_len, ref_end-ref_start) bytes, or NULL to let the library
 * keep a grow-only scratch of its own per (device, stream) (allocates on first use: not graph-capture
 * safe; calls that use it are serialised among themselves).  word_num must be bgsa_hip_word_num().
 * Reads the process-global selection (scores, alignment mode) once, at entry.
 * All pointers are device pointers; asynchronous on `stream`. */
int bgsa_hip_cal_align_score_dev(int algo, const char *d_content, const hip_read_t *d_peq,
                                 void *d_results, int ref_len, int read_len, int64_t read_count,
                                 int ref_start, int ref_end, int word_num, int k,
                                 void *d_workspace, size_t workspace_bytes, void *stream);

/* The same with the parameters passed explicitly instead of read from the process globals. */
size_t bgsa_hip_workspace_bytes_ex(const bgsa_hip_params_t *params, int ref_len, int read_len, int n_queries);
int bgsa_hip_cal_align_score_ex(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq,
                                void *d_results, int ref_len, int read_len, int64_t read_count,
                                int ref_start, int ref_end, int word_num,
                                void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- subject buckets of mixed read lengths (GLOBAL modes: Myers -distance / +distance, BitPAl with every compiled set) ----
 * A bucket whose subjects differ in length is preprocessed as ever — read_count rows of read_len + 1 bytes, read_len the
 * LONGEST subject, every shorter one padded behind its own end with any bytes — and scored with d_read_lens: read_count
 * int32 device entries, the length of every subject column, the padding columns up to the multiple of 64 included (give those
 * read_len).  Pair (query, column c) then scores exactly as the query against the first d_read_lens[c] characters of the row:
 * column j of a global DP depends on columns <= j only, so the rows run over the padded width and the score is formed under the
 * lane's own length; what lies behind a subject's end never enters.  An entry is clamped to [0, read_len] inside the kernel
 * (it forms a mask, never an address).  Queries keep ONE length per call: group them by length.
 * d_read_lens == NULL is exactly bgsa_hip_cal_align_score_ex: same kernel, the certified Myers band included.  With lengths
 * a Myers launch always runs full rows — the band's window schedule and limit certify one (m, n) — and leaves
 * bgsa_hip_myers_band_stats() untouched.  Everything else (workspace, word_num = bgsa_hip_word_num(algo, ref_len, read_len, k),
 * results layout, stream) is as there.
 * BGSA_HIP_EUNSUPPORTED with non-NULL lengths, before anything is allocated or launched, bgsa_hip_last_error() naming the
 * reason: the banded filter; either semi-global mode; word_num > 32; a BitPAl set whose register-resident kernel does not
 * reach word_num words. */
int bgsa_hip_cal_align_score_lens_ex(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq,
                                     void *d_results, const int32_t *d_read_lens, int ref_len, int read_len, int64_t read_count,
                                     int ref_start, int ref_end, int word_num,
                                     void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- hit selection: the K best subjects per query, or every subject within a cutoff, from a score tile in HBM ----
 * d_results = a score tile as the scoring calls write it: n_queries rows of row_stride elements of elem_bytes bytes
 * (2: int16 of Myers / BitPAl, 1: int8 of the banded filter).  Only columns [0, valid_count) are candidates: the columns
 * behind them are the all-'N' padding reads of the last group (file.c:98-112) and never appear, whatever they scored.
 * The reported subject id of column c is subject_base + c (ids lie in [0, 2^46)).  The tile is only read.
 *
 * ONE TOTAL ORDER makes every result unique: a candidate is (score, subject id); better = the larger score, or the
 * smaller one when `smallest` is set (distances: the banded filter, Myers +distance); among equal scores the smaller
 * subject id is better.
 *
 * bgsa_hip_top_hits_dev: for every row the k_best (1..64; else BGSA_HIP_EUNSUPPORTED) best candidates, best first, as
 * d_hit_scores / d_hit_subjects [n_queries][k_best].  Slots beyond valid_count candidates hold subject -1 and the worst
 * int32 of the direction (INT32_MIN, or INT32_MAX with `smallest`).
 * bgsa_hip_threshold_hits_dev: for every row every candidate at least as good as `cutoff` (score >= cutoff, or <= with
 * `smallest`), in ascending subject order, as d_hit_scores / d_hit_subjects [n_queries][cap_per_query]; d_counts[row] =
 * the TRUE number of such candidates even when it exceeds cap_per_query — the list then holds the cap_per_query
 * lowest-indexed ones (slots beyond the count are left as they were).
 * accumulate != 0: what the outputs already hold joins in, with its subject ids as stored — a caller walking several
 * subject buckets (subject_base = the bucket's first subject) ends with the k_best best overall; threshold hits are
 * appended behind the row's current d_counts[row], which grows by this tile's count.  The first call passes 0 (or lists
 * of subject -1 and counts of 0).
 * d_workspace = caller-owned device scratch of at least bgsa_hip_hits_workspace_bytes() bytes (the same for both calls;
 * the size depends only on n_queries and row_stride — elem_bytes and k_best are validated, 0 for a bad one, and
 * otherwise ignored — and never shrinks when an argument grows), or NULL for the library's own grow-only scratch per (device, stream), as in
 * bgsa_hip_cal_align_score_dev (allocates on first use: not graph-capture safe).  With a workspace the calls only launch
 * kernels on `stream`: no allocation, no synchronisation, safe inside a stream capture.
 * BGSA_HIP_EINVAL: a NULL pointer, a non-positive n_queries / row_stride / cap_per_query, valid_count outside
 * [0, row_stride] or >= 2^31, elem_bytes other than 1 or 2, subject ids beyond 2^46, a workspace that is too small —
 * all checked before the first HIP call. */
size_t bgsa_hip_hits_workspace_bytes(int n_queries, int64_t row_stride, int elem_bytes, int k_best);
int bgsa_hip_top_hits_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride,
                          int64_t valid_count, int64_t subject_base, int k_best, int smallest, int accumulate,
                          int32_t *d_hit_scores, int64_t *d_hit_subjects,
                          void *d_workspace, size_t workspace_bytes, void *stream);
int bgsa_hip_threshold_hits_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride,
                                int64_t valid_count, int64_t subject_base, int cutoff, int smallest, int accumulate,
                                int64_t cap_per_query, int32_t *d_counts,
                                int32_t *d_hit_scores, int64_t *d_hit_subjects,
                                void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- hit lists per subject: the K best queries of every column, or every query within a cutoff, from a score tile in HBM ----
 * The column counterpart of the block above: the same tile (n_queries rows of row_stride elements of elem_bytes bytes, 2 or 1)
 * reduced along its COLUMNS.  Row r of the tile is query query_base + r; ids are int32, as the pair calls take them.  Only
 * columns [0, valid_count) have lists: the columns behind them (the all-'N' padding reads) are not read for any purpose, and
 * nothing is written at or beyond valid_count * k_best (valid_count * cap_per_subject; valid_count for d_counts).  The tile is
 * only read.
 *
 * ONE TOTAL ORDER makes every result unique: a candidate is (score, query id); better = the larger score, or the smaller one
 * when `smallest` is set; among equal scores the smaller query id is better.
 *
 * bgsa_hip_top_queries_dev: for every column the k_best (1..64; else BGSA_HIP_EUNSUPPORTED) best candidates, best first, as
 * d_hit_scores / d_hit_queries [valid_count][k_best].  Slots beyond n_queries candidates hold query -1 and the worst int32 of
 * the direction (INT32_MIN, or INT32_MAX with `smallest`).
 * bgsa_hip_threshold_queries_dev: for every column every candidate at least as good as `cutoff` (score >= cutoff, or <= with
 * `smallest`), in ascending query order, as d_hit_scores / d_hit_queries [valid_count][cap_per_subject]; d_counts[column] =
 * the TRUE number of such candidates even when it exceeds cap_per_subject — the list then holds the cap_per_subject
 * lowest-indexed ones (slots beyond the count are left as they were).
 * accumulate != 0: what the outputs already hold joins in, with its query ids as stored — a caller walking query blocks
 * (query_base = the block's first query; every call after the first) or several query sets ends with the k_best best overall;
 * threshold hits are appended behind the column's current d_counts[column], which grows by this tile's count.  The first call
 * passes 0 (or lists of query -1 and counts of 0).  Stored scores outside the element's range are clamped to it.  Several
 * subject buckets need no accumulate: their columns are disjoint, the lists are concatenated.
 * d_workspace = caller-owned device scratch of at least bgsa_hip_query_hits_workspace_bytes() bytes, or NULL.  The size is 0
 * for a non-positive n_queries / row_stride / k_best or a bad elem_bytes and never shrinks when an argument grows.  The lists
 * are kept on chip and rows are not split among wavefronts, so today nothing is stored there and NULL allocates nothing
 * either: with or without a workspace the calls only launch kernels on `stream` — no allocation, no synchronisation, safe
 * inside a stream capture.  (The parallelism is the tile's width: 128 int16 or 256 int8 columns per wavefront.)
 * BGSA_HIP_EINVAL: a NULL pointer, a non-positive n_queries / row_stride / cap_per_subject, valid_count outside
 * [0, row_stride], query_base < 0 or query_base + n_queries beyond INT32_MAX, elem_bytes other than 1 or 2, a workspace that
 * is too small — all checked before the first HIP call. */
size_t bgsa_hip_query_hits_workspace_bytes(int n_queries, int64_t row_stride, int elem_bytes, int k_best);
int bgsa_hip_top_queries_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride,
                             int64_t valid_count, int query_base, int k_best, int smallest, int accumulate,
                             int32_t *d_hit_scores, int32_t *d_hit_queries,
                             void *d_workspace, size_t workspace_bytes, void *stream);
int bgsa_hip_threshold_queries_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride,
                                   int64_t valid_count, int query_base, int cutoff, int smallest, int accumulate,
                                   int cap_per_subject, int32_t *d_counts,
                                   int32_t *d_hit_scores, int32_t *d_hit_queries,
                                   void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- alignment of selected pairs: the edit script (CIGAR) of every (query, subject) pair of a list, traced back on the GPU ----
 * Myers unit-cost GLOBAL alignment only, subjects of 1..1024 bp (word_num <= 32; beyond: BGSA_HIP_EUNSUPPORTED), any query
 * length.  Semi-global mode, BitPAl score sets, the banded filter and longer subjects are not offered.
 * d_content = the mapped query rows (stride ref_len + 1) and d_peq = the Myers Peq blocks of the resident bucket of read_count
 * subjects, exactly as bgsa_hip_cal_align_score_dev takes them.  The subject rows are not needed: whether query character i
 * matches subject column j is bit j of the subject's Peq plane of class q_i, so the alignment agrees with the scores by
 * construction ('N' and out-of-alphabet bytes included).
 * Pair p = (d_pair_query[p], d_pair_subject[p]); subject ids are as the hit lists report them, column = id - subject_base.  A
 * pair whose subject id is -1 (the unused top-K slot) or lies outside [subject_base, subject_base + read_count) — another
 * bucket's — is left untouched in all three outputs, so a caller walking several buckets calls once per bucket on the same
 * outputs and ends with every pair filled (read_count counts the padding reads of the last group: cut such buckets at
 * multiples of 64, or keep padding ids out of the list as the hit lists do, so that no id belongs to two buckets).  A query index outside [0, n_queries) on an otherwise owned pair touches nothing
 * either and raises BGSA_HIP_FAULT_PAIR in the sticky word bgsa_hip_stream_faults() reads (an argument check inside the kernel).
 * Per owned pair: d_distance[p] = the edit distance D[m][n] (the negated score); d_n_ops[p] = the TRUE number of runs of the
 * edit script even beyond cigar_cap; d_cigar[p * cigar_cap ...] = its first min(n_ops, cigar_cap) runs in query order from the
 * first column, each `length << 4 | op` with the BAM op codes 7 '=' (query and subject character of the same class), 8 'X'
 * (of different classes), 1 'I' (a query character only), 2 'D' (a subject character only); adjacent runs differ in op;
 * slots behind the runs are left as they were.  cigar_cap = ref_len + read_len can never overflow.
 * ONE CANONICAL SCRIPT: the path found walking back from (m, n); at a cell (i, j), i, j > 0: the diagonal if
 * D[i-1][j-1] + [q_i != s_j] == D[i][j], otherwise the step up ('I') if D[i-1][j] + 1 == D[i][j], otherwise the step left
 * ('D'); at i == 0 only 'D' and at j == 0 only 'I' remain.
 * d_workspace = caller-owned device scratch, or NULL for the library's grow-only scratch per (device, stream) (not capture
 * safe).  ..._min_workspace_bytes() = what 64 pairs need; ..._workspace_bytes() = what all n_pairs need in one pass, at most
 * BGSA_HIP_ALIGN_PAIRS_MAX_WORKSPACE unless 64 pairs alone need more.  ANY size from the minimum up is accepted: the call walks
 * the list in chunks of as many whole waves as the workspace holds, launched on `stream` one after the other; the outputs do
 * not depend on the chunking.  With a caller workspace the call only launches kernels: no allocation, no synchronisation,
 * safe inside a stream capture (the device's fault word is allocated by the first launch of any kind on that device).
 * BGSA_HIP_EINVAL: a NULL pointer (the workspace excepted), negative n_pairs, non-positive lengths / n_queries / cigar_cap,
 * read_count not a positive multiple of 64, word_num other than bgsa_hip_word_num(BGSA_ALGO_MYERS, ...), a workspace below the
 * minimum — all checked before the first HIP call.  n_pairs == 0 is BGSA_HIP_OK and launches nothing.
 * The two ..._workspace_bytes() functions size bgsa_hip_trace_pairs_dev (below) too, with the same rules: its history and op
 * bytes have the same size and layout. */
#define BGSA_HIP_ALIGN_PAIRS_MAX_WORKSPACE ((size_t)1 << 30)
size_t bgsa_hip_align_pairs_workspace_bytes(int ref_len, int read_len, int64_t n_pairs);
size_t bgsa_hip_align_pairs_min_workspace_bytes(int ref_len, int read_len);
int bgsa_hip_myers_align_pairs_dev(const char *d_content, const hip_read_t *d_peq,
                                   int ref_len, int read_len, int64_t read_count, int word_num,
                                   const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                   int n_queries, int64_t subject_base,
                                   int32_t *d_distance, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                                   void *d_workspace, size_t workspace_bytes, void *stream);
/* The same for a bucket of mixed subject lengths (bgsa_hip_cal_align_score_lens_ex): d_read_lens[column] is the pair's n, so the
 * script consumes exactly ref_len query and d_read_lens[column] subject characters.  NULL: the call above. */
int bgsa_hip_myers_align_pairs_lens_dev(const char *d_content, const hip_read_t *d_peq, const int32_t *d_read_lens,
                                        int ref_len, int read_len, int64_t read_count, int word_num,
                                        const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                        int n_queries, int64_t subject_base,
                                        int32_t *d_distance, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                                        void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- band-limited history: the same edit scripts for subjects of ANY length, within a caller-given distance bound ----
 * bgsa_hip_myers_align_pairs_dev keeps the whole subject in registers and a history of ref_len x 2 x word_num x 256 B per 64
 * pairs: it stops at 1,024 bp.  Every caller of a pair call already holds a bound on the distance — the cutoff of its threshold
 * hits, the worst score of its top hits — and a pair whose distance is <= B = max_distance has all its optimal paths inside the
 * diagonal band |d| + |d - (n - m)| <= B, d = j - i (n = read_len, m = ref_len; the inequality the Myers scoring kernels certify
 * their band with).  This call runs the rows on the words that hold the band only and keeps history for those words only; it
 * takes every subject length the scoring calls take, short ones too (there it is a cross-check of the call above from another
 * kernel, with a smaller workspace).  Myers unit-cost GLOBAL alignment; no mixed-length variant.
 * THE RULE.  delta = n - m, dlo = -((B - delta) / 2), dhi = (delta + B) / 2 (C division; both numerators are >= 0 when
 * |delta| <= B).  Rows run in blocks of 32: the block of 0-based rows i0 .. last - 1, i0 % 32 == 0, last = min(i0 + 32, m), has
 * the WINDOW of words [a, b], a = (max(1, i0 + 1 + dlo) - 1) / 32, b = (min(n, last + dhi) - 1) / 32.  Every row of the block is
 * the Myers row on exactly these words: the lowest window word takes the row-edge carry-ins (hp_in = 1, hn_in = 0, add-carry 0)
 * whether or not a == 0, words left of the window keep their last deltas, words right of it their initial state (pv = ~0,
 * mv = 0).  D' = m + the sum over all word_num words of popc(pv & mask) - popc(mv & mask) is the cost of a real path, so
 * D' >= D, and D' <= B certifies D' = D: the pair is then traced back from (m, n) with the preference of the call above and
 * gets that call's canonical script.  Otherwise the pair is beyond the bound.
 * bgsa_hip_align_pairs_band_words: the widest block window of the shape in words, <= word_num; 0 for non-positive lengths, a
 * negative max_distance, or |delta| > max_distance (no pair of that shape can be within the bound).
 * Arguments, pair ownership (subject_base, the slot -1, pairs of other buckets untouched), BGSA_HIP_FAULT_PAIR for a query index
 * out of range, the cigar format and the chunking (any workspace from the minimum up, whole waves per chunk, forward and
 * traceback kernels one after the other on `stream`; with a caller workspace only kernel launches: capture safe) are those of
 * bgsa_hip_myers_align_pairs_dev.  Per owned pair:
 *   D <= max_distance: d_distance[p] = D, d_n_ops[p] = the TRUE number of runs even beyond cigar_cap, d_cigar[p * cigar_cap ...] =
 *     the first min(n_ops, cigar_cap) runs — bit for bit what bgsa_hip_myers_align_pairs_dev writes where that call applies;
 *   D >  max_distance — every pair when |delta| > max_distance, which is still BGSA_HIP_OK: d_distance[p] =
 *     BGSA_HIP_DISTANCE_BEYOND, d_n_ops[p] = 0, the cigar row untouched.
 * The workspace: one wave's slice = history (ref_len x 2 x band_words x 256 B) + state (2 x word_num x 256 B) + op bytes
 * ((ref_len + read_len) x 64), rounded up to 256 = ..._banded_min_workspace_bytes(); ..._banded_workspace_bytes() = what all
 * n_pairs need in one pass, at most BGSA_HIP_ALIGN_PAIRS_MAX_WORKSPACE, never below one wave; NULL = the library's own grow-only
 * scratch (not capture safe).  10,000 x 10,000 bp at max_distance 500: 17 words, 88 MB per wave instead of 1.6 GB.
 * BGSA_HIP_EINVAL, checked in this order before the first HIP call: a NULL pointer (the workspace excepted), negative n_pairs,
 * non-positive lengths / n_queries / cigar_cap, read_count not a positive multiple of 64, word_num other than
 * bgsa_hip_word_num(BGSA_ALGO_MYERS, ...), a negative max_distance; then BGSA_HIP_EUNSUPPORTED: ref_len + read_len beyond
 * 2^31 - 1 (the op bytes are counted in int), a window wider than the 32 words the kernels hold (bgsa_hip_last_error() names the largest max_distance the shape takes: 961 for 4,000 x 4,000 bp); then
 * BGSA_HIP_EINVAL: a workspace below the minimum.  n_pairs == 0 is BGSA_HIP_OK once the checks pass and launches nothing.
 * BGSA_HIP_FAULT_BAND (sticky, bgsa_hip_stream_faults()): a traceback step asked for a word outside its block's window; the
 * step is not read, the pair keeps n_ops = 0.  By the rule this cannot happen for a certified pair: the bit means a bug, never
 * an input. */
#define BGSA_HIP_DISTANCE_BEYOND (-2)
int bgsa_hip_align_pairs_band_words(int ref_len, int read_len, int max_distance);
size_t bgsa_hip_align_pairs_banded_min_workspace_bytes(int ref_len, int read_len, int max_distance);
size_t bgsa_hip_align_pairs_banded_workspace_bytes(int ref_len, int read_len, int max_distance, int64_t n_pairs);
int bgsa_hip_myers_align_pairs_banded_dev(const char *d_content, const hip_read_t *d_peq,
                                          int ref_len, int read_len, int64_t read_count, int word_num,
                                          const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                          int n_queries, int64_t subject_base, int max_distance,
                                          int32_t *d_distance, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                                          void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- score, span and edit script of selected pairs, for every aligner that has an alignment to report ----
 * What bgsa_hip_myers_align_pairs_dev does for Myers global, for: BitPAl with ANY score set (compiled in or not), global;
 * BitPAl semi-global (query end to end, free subject overhangs); Myers semi-global (subject end to end inside the query); and
 * Myers global itself (the same scripts as bgsa_hip_myers_align_pairs_dev, from another kernel).  Subjects of 1..1024 bp.
 * d_content, d_peq, the pair list, ownership (subject_base, the -1 slot, pairs of other buckets left untouched in all FOUR
 * outputs) and BGSA_HIP_FAULT_PAIR for a query index outside [0, n_queries) are exactly as there; d_peq is the bucket's block
 * as the aligner of params->algo scores it (Myers and BitPAl share the Peq layout).
 * THE MODEL is the linear-gap DP over the character classes, rows i = 1..m query characters, columns j = 1..n subject columns:
 * s(i, j) = match if q_i and s_j are of the same class — bit j of the subject's Peq plane of class q_i, so the alignment agrees
 * with the bit-parallel scores by construction, 'N' and out-of-alphabet bytes included — else mismatch;
 * H[i][j] = max(H[i-1][j-1] + s(i, j), H[i-1][j] + gap, H[i][j-1] + gap).  Three modes, from params (algo, alignment, match,
 * mismatch, gap; BGSA_ALGO_MYERS scores 0 / -1 / -1 whatever the three ints hold, as the scoring calls):
 *   BitPAl or Myers, global:    H[0][j] = j*gap, H[i][0] = i*gap; the score is H[m][n], the end cell (m, n); the walk back
 *                               stops at (0, 0).
 *   Myers, semi-global:         H[0][j] = j*gap, H[i][0] = 0; the score is the max over i in [0, m] of H[i][n], the end cell
 *                               the SMALLEST such i; the walk back stops at the first cell with j = 0.
 *   BitPAl, semi-global:        H[0][j] = 0, H[i][0] = i*gap; the score is the max over j in [0, n] of H[m][j], the end cell
 *                               the SMALLEST such j; the walk back stops at the first cell with i = 0.
 * ONE CANONICAL SCRIPT, the preference order of bgsa_hip_myers_align_pairs_dev: at a cell (i, j), i, j > 0: the diagonal if
 * H[i-1][j-1] + s(i, j) == H[i][j], otherwise the step up ('I') if H[i-1][j] + gap == H[i][j], otherwise the step left ('D');
 * on a non-free edge only 'D' (i = 0) or only 'I' (j = 0) remains.  At 0 / -1 / -1 in global mode this is that call's script.
 * Per owned pair: d_score[p] = the score as the scoring calls report it for the pair (Myers: minus the distance);
 * d_span[4p .. 4p+3] = (q_begin, q_end, s_begin, s_end), half-open, the aligned parts of query and subject — (0, m, 0, n) in
 * global mode; d_n_ops[p] = the TRUE number of runs even beyond cigar_cap; d_cigar[p * cigar_cap ...] = the first
 * min(n_ops, cigar_cap) runs, `length << 4 | op` with the BAM ops 7 '=' / 8 'X' / 1 'I' / 2 'D', covering the aligned span
 * only (no clip ops), in query order, adjacent runs differing in op; slots behind the runs are left as they were.
 * cigar_cap = ref_len + read_len can never overflow.
 * The workspace is sized by bgsa_hip_align_pairs_workspace_bytes() / ..._min_workspace_bytes() and follows their rules: any
 * size from the minimum up (chunks of whole waves), NULL = the library's own scratch (not capture safe); with a caller
 * workspace the call only launches kernels.  (Subjects from 512 bp keep a DP row beyond 64 KiB of LDS; the kernel's limit is
 * raised by the first such call per device and mode, ahead of its launches.)
 * BGSA_HIP_EINVAL: a NULL pointer (workspace and stream excepted), negative n_pairs, non-positive lengths / n_queries /
 * cigar_cap, read_count not a positive multiple of 64, an unknown algo or alignment, gap >= 0 or match <= mismatch, word_num
 * other than bgsa_hip_word_num(params->algo, ...), a workspace below the minimum.  BGSA_HIP_EUNSUPPORTED: the banded filter;
 * Myers +distance (0, 1, 1) — it aligns as the -distance aligner does; word_num > 32; max(|match|, |mismatch|, |gap|) *
 * (ref_len + read_len) > 32767 (the DP row is kept in 16 bits).  All checked before the first HIP call; n_pairs == 0 is
 * BGSA_HIP_OK and launches nothing. */
int bgsa_hip_trace_pairs_dev(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq,
                             int ref_len, int read_len, int64_t read_count, int word_num,
                             const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                             int n_queries, int64_t subject_base,
                             int32_t *d_score, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                             void *d_workspace, size_t workspace_bytes, void *stream);
/* The same for a bucket of mixed subject lengths, GLOBAL mode only (semi-global with lengths: BGSA_HIP_EUNSUPPORTED): the pair's
 * n is d_read_lens[column], the span reports s_end = that length.  NULL: the call above. */
int bgsa_hip_trace_pairs_lens_dev(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq,
                                  const int32_t *d_read_lens, int ref_len, int read_len, int64_t read_count, int word_num,
                                  const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                  int n_queries, int64_t subject_base,
                                  int32_t *d_score, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                                  void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- read placement on a bucket of MIXED read lengths: Myers semi-global with every read's own n ----
 * The two calls above refuse semi-global params together with lengths; these two are the Myers semi-global mode (the read —
 * the subject — end to end inside the query, unit costs: params 0 / -1 / -1, BGSA_ALIGN_SEMIGLOBAL) for a bucket built as
 * bgsa_hip_cal_align_score_lens_ex takes it: rows of read_len bytes, d_peq from bgsa_hip_handle_reads_dev at read_len,
 * d_read_lens[column] = the read's own length for all read_count columns, padding columns included.  A length is clamped to
 * [0, read_len]; it forms shifts, masks and start scores and, as an index, is clamped again: no value takes an access out of
 * bounds.  Column c is scored and traced as the first d_read_lens[c] characters of its row, bit for bit what the equal-length
 * calls report for a bucket of those prefixes; the bytes behind a read's end never enter.  A length of 0 scores 0.
 * bgsa_hip_myers_place_score_lens_dev: bgsa_hip_cal_align_score_ex with those params, int16 results [query][column], the same
 * argument checks, the same empty-window shortcut (ref_end == ref_start or read_count == 0: BGSA_HIP_OK, nothing touched) and
 * the same workspace (bgsa_hip_workspace_bytes_ex of those params; NULL = the library's own scratch).  Every lane of the
 * scoring kernel right-aligns its read by its own length; the row loop is the equal-length kernel's.  BGSA_HIP_EINVAL:
 * d_read_lens == NULL (equal lengths: bgsa_hip_cal_align_score_ex) and what that call answers EINVAL to.
 * BGSA_HIP_EUNSUPPORTED: word_num > 32 — reads beyond 1,024 bp run as column blocks, which have no per-lane form — and a
 * measurement knob that selects another semi-global kernel (BGSA_MYERS_IMPL, BGSA_MYERS_PEQ_MAX_WORDS).
 * bgsa_hip_myers_place_trace_pairs_lens_dev: bgsa_hip_trace_pairs_dev's "Myers, semi-global" model with n = d_read_lens[column]
 * per pair: the outputs, ownership, cigar format, workspace rules and checks are that call's, span[3] = the pair's own length.
 * BGSA_HIP_EINVAL also for d_read_lens == NULL. */
int bgsa_hip_myers_place_score_lens_dev(const char *d_content, const hip_read_t *d_peq, void *d_results,
                                        const int32_t *d_read_lens, int ref_len, int read_len, int64_t read_count,
                                        int ref_start, int ref_end, int word_num,
                                        void *d_workspace, size_t workspace_bytes, void *stream);
int bgsa_hip_myers_place_trace_pairs_lens_dev(const char *d_content, const hip_read_t *d_peq, const int32_t *d_read_lens,
                                              int ref_len, int read_len, int64_t read_count, int word_num,
                                              const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                              int n_queries, int64_t subject_base,
                                              int32_t *d_score, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                                              void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- band-limited semi-global placement: where a read of ANY length lies inside its window, and how it aligns ----
 * bgsa_hip_trace_pairs_dev keeps a 16-bit DP row of the whole subject in LDS: it stops at 1,024 bp.  This call reports the
 * same four outputs for the "Myers, semi-global" model above (the subject, n = read_len columns, end to end inside the query,
 * m = ref_len rows; D[0][j] = j, D[i][0] = 0; unit costs) for every subject length the semi-global scoring call takes, with the
 * history limited by a caller-given bound on the distance, as bgsa_hip_myers_align_pairs_banded_dev does in global mode.  Short
 * reads too: there it is bit-parallel where bgsa_hip_trace_pairs_dev runs a scalar DP.  No mixed-length variant.
 * LOCATE (exact, independent of the bound).  D* = min over i in [0, m] of D[i][n], e = the SMALLEST such i: the bit-parallel
 * Myers semi-global row on all word_num words of the subject (natural bit positions), the row edge feeding hp_in = 0, the query
 * character per lane; run starts at n (row 0) and moves by Hp - Hn at column n per row, a strictly smaller run moves e.
 * THE BOUND.  B = min(max_distance, n) — D* <= n always.  A pair with D* > B is beyond the bound.
 * THE RULE for a pair with D* <= B, in VIRTUAL rows: o = e - n - B (per pair, may be negative), M' = n + B; virtual row
 * i' = 1 .. M' is query row i = i' + o, so the end cell (e, n) is (M', n) for every pair.  Rows run in blocks of 32 virtual
 * rows: the block of 0-based virtual rows i0 .. last - 1, i0 % 32 == 0, last = min(i0 + 32, M'), has the WINDOW of words [a, b],
 * a = (max(1, i0 + 1 - 2B) - 1) / 32, b = (min(n, last) - 1) / 32 — the diagonals j - i' in [-2B, 0]: a path that ends on -B
 * and costs <= B moves at most B either way.  The windows depend on (n, B) only.  Every row of a block is the Myers row on
 * exactly its window's words: the lowest window word takes hp_in = 0 when a == 0 (the free column 0 of the mode) and hp_in = 1
 * otherwise, hn_in = 0, add-carry 0; words left of the window keep their last deltas, words right of it their initial state
 * (pv = ~0, mv = 0).  A virtual row whose query row does not exist (i < 1, only when o < 0, only in blocks with a == 0 because
 * -o <= 2B) runs with an all-zero match mask, which with hp_in = 0 leaves the state at row 0's.
 * CERTIFICATION.  D' = (the number of rows run with hp_in = 1) + the sum over all word_num words of popc(pv & mask) -
 * popc(mv & mask) is the cost of a real path ending at (e, n), so D' >= D*, and for D* <= B the two are equal.  D' != D*
 * raises the sticky BGSA_HIP_FAULT_BAND and leaves n_ops = 0: the bit means a bug, never an input.
 * TRACEBACK from (e, n) through the window words' history (the two vectors of bgsa_hip_myers_align_pairs_dev) with the
 * preference of every pair call — diagonal, then up 'I', then left 'D' —, stopped at the first cell with j = 0, whose row is
 * q_begin; on query row 0 with j > 0 the remaining j steps are 'D'.  A step that asks for a cell outside its block's window
 * raises BGSA_HIP_FAULT_BAND as in the global call.
 * bgsa_hip_place_pairs_band_words: the widest window of (read_len, max_distance) in words, 1 .. word_num; 0 for a non-positive
 * length or a negative bound.  A window of w >= 2 words first appears at B = 16 (w - 2) + 1.
 * Arguments, pair ownership (subject_base, the slot -1, pairs of other buckets untouched in all four outputs),
 * BGSA_HIP_FAULT_PAIR, the cigar format and the chunking (any workspace from the minimum up, whole waves per chunk, the locate,
 * forward and traceback kernels one after the other on `stream`; with a caller workspace only kernel launches: capture safe)
 * are those of bgsa_hip_myers_align_pairs_banded_dev.  Per owned pair, whatever the bound: d_distance[p] = D* (exact; minus the
 * score the semi-global scoring call reports) and d_span[4p .. 4p+3] = (q_begin, e, 0, n).
 *   D* <= B: d_n_ops[p] = the TRUE number of runs even beyond cigar_cap, d_cigar[p * cigar_cap ...] = the first
 *     min(n_ops, cigar_cap) runs; distance = -score, span, n_ops and runs are bit for bit what bgsa_hip_trace_pairs_dev writes
 *     for the pair where that call applies;
 *   D* >  B: q_begin = -1, d_n_ops[p] = 0, the cigar row untouched.
 * The workspace: one wave's slice = history ((n + B) x 2 x band_words x 256 B) + state ((2 x word_num + 1) x 256 B) + locate's
 * carries (ceil(m / 32) x 3 x 256 B) + op bytes ((n + min(m, n + B)) x 64), rounded up to 256 =
 * ..._banded_min_workspace_bytes(); ..._banded_workspace_bytes() = what all n_pairs need in one pass, at most
 * BGSA_HIP_ALIGN_PAIRS_MAX_WORKSPACE, never below one wave; NULL = the library's own grow-only scratch (not capture safe).
 * BGSA_HIP_EINVAL, checked in this order before the first HIP call: a NULL pointer (workspace and stream excepted), negative
 * n_pairs, non-positive lengths / n_queries / cigar_cap, read_count not a positive multiple of 64, word_num other than
 * bgsa_hip_word_num(BGSA_ALGO_MYERS, ...), a negative max_distance; then BGSA_HIP_EUNSUPPORTED: ref_len + read_len + B or
 * 2 read_len + B beyond 2^31 - 1 (B as above: rows and op bytes are counted in int), a window wider than the 32 words the
 * kernels hold (bgsa_hip_last_error() names the largest max_distance the read takes: 496 beyond 1,024 bp; a read of up to
 * 1,024 bp takes any bound); then BGSA_HIP_EINVAL: a workspace below the minimum.  n_pairs == 0 is BGSA_HIP_OK once the checks
 * pass and launches nothing. */
int bgsa_hip_place_pairs_band_words(int read_len, int max_distance);
size_t bgsa_hip_place_pairs_banded_min_workspace_bytes(int ref_len, int read_len, int max_distance);
size_t bgsa_hip_place_pairs_banded_workspace_bytes(int ref_len, int read_len, int max_distance, int64_t n_pairs);
int bgsa_hip_myers_place_pairs_banded_dev(const char *d_content, const hip_read_t *d_peq,
                                          int ref_len, int read_len, int64_t read_count, int word_num,
                                          const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                          int n_queries, int64_t subject_base, int max_distance,
                                          int32_t *d_distance, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                                          void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- a reference as the query set: its windows cut on the device, both strands, placements in reference coordinates ----
 * The placement calls above take windows of a reference as queries and reads as the resident subjects.  These calls know that
 * the queries are ONE sequence: the reference crosses to the device once, its overlapping windows are written as query rows
 * there — forward and reverse-complemented —, and the spans of the pair calls become (strand, reference begin, reference end)
 * with the copies of one locus seen through overlapping windows marked.  No scoring, selection or pair call changes.
 * GEOMETRY (the one rule; bgsa_amd/reference.py: window_plan restates it).  The reference is ref_len = L mapped bytes (codes
 * 0..4 as bgsa_hip_map_queries_dev writes them, no newlines).  Window length W and stride S satisfy 1 <= S <= W <= L.
 *   n_windows = 1 + ceil((L - W) / S);  start(w) = min(w * S, L - W) — the last window is anchored at the reference's end, so
 *   every window is W long.
 * Window ids are int32: forward window w has id w, reverse window w has id n_windows + w; row i of the reverse window is
 * comp(reference[start(w) + W - 1 - i]), comp(c) = 3 - c for c < 4 and 4 ('N') otherwise — on codes, so a byte outside the
 * alphabet, which maps to 0 like 'A', complements to 'T'.  2 * n_windows beyond INT32_MAX is BGSA_HIP_EINVAL in the device calls.
 * COMPLETENESS.  B = min(max_distance, n) for a read of n bp: a placement within the bound spans at most n + B reference
 * bases, and such a span lies wholly inside at least one window exactly when S <= W - (n + B) + 1.  Under that condition the
 * best distance over all windows IS the semi-global optimum over the whole reference for every read whose optimum is <= B (the
 * optimal span fits a window; no window can beat a superstring of it).
 * bgsa_hip_reference_window_count / _window_start: host only, no device — n_windows (whatever its size) and start(window);
 * -1 with bgsa_hip_last_error() set for a shape outside 1 <= S <= W <= L or a window outside [0, n_windows).
 * bgsa_hip_reference_windows_dev writes n_rows query rows of window_len codes + '\n' (stride window_len + 1) to d_content —
 * the buffer the scoring and pair calls take as d_content; it may start at any byte address, and nothing is written at or
 * beyond n_rows * (window_len + 1).  d_window_ids == NULL: row r is window id first_id + r, and [first_id, first_id + n_rows)
 * must lie in [0, 2 * n_windows).  Otherwise row r is window d_window_ids[r] (first_id is ignored); an id outside
 * [0, 2 * n_windows) — the -1 of an unused hit slot — writes a row of code 4: such an id forms a value, never an address.
 * n_rows in [0, 2^31 - 1]; n_rows == 0 is BGSA_HIP_OK and launches nothing.  Only a launch on `stream`: no allocation, no
 * synchronisation (capture safe).
 * bgsa_hip_reference_placements_dev turns the outputs of bgsa_hip_myers_place_pairs_banded_dev (or bgsa_hip_trace_pairs_dev) for
 * the hit lists d_hit_windows[n_reads][k] (bgsa_hip_top_queries_dev's ids, best first; pair p = c * k + r) into one list per
 * read.  Hit (c, r) with window id g, w = g mod n_windows, span (qb, qe, ., .) = d_span[4p], d_span[4p + 1]:
 *   unused slot (g < 0, or g >= 2 * n_windows): strand -1, begin -1, end -1, keep 0;
 *   beyond the bound (qb < 0):   the strand its id says, begin -1, end -1, keep 0;
 *   forward (g < n_windows):     strand 0, ref_begin = start(w) + qb, ref_end = start(w) + qe;
 *   reverse:                     strand 1, ref_begin = start(w) + W - qe, ref_end = start(w) + W - qb, and the first d_n_ops[p]
 *                                runs of its row d_cigar[p * cigar_cap ...] are reversed in place: they then read along the
 *                                forward reference against the reverse-complemented read ('I' and 'D' keep their meaning); a
 *                                row whose n_ops exceeds cigar_cap is left untouched.  d_n_ops == d_cigar == NULL: nothing to
 *                                reverse.
 *   keep: walking r = 0 .. k - 1, hit r is kept if it is placed and no kept r' < r of the same read has the same strand and a
 *         reference interval with begin' < end and begin < end' — so one locus seen through two overlapping windows, or a
 *         clipped copy of it at a window's edge, keeps only its best view.
 * k in 1..64; n_reads == 0 is BGSA_HIP_OK and launches nothing.  Only a launch on `stream`.
 * BGSA_HIP_EINVAL, all checked before the first HIP call: a NULL pointer (stream, d_window_ids and the d_n_ops / d_cigar pair
 * excepted), a shape outside 1 <= S <= W <= L, 2 * n_windows > INT32_MAX, negative n_rows / n_reads, an id range outside
 * [0, 2 * n_windows), k outside 1..64, d_cigar without d_n_ops or with a non-positive cigar_cap. */
int64_t bgsa_hip_reference_window_count(int64_t ref_len, int window_len, int stride);
int64_t bgsa_hip_reference_window_start(int64_t ref_len, int window_len, int stride, int64_t window);
int bgsa_hip_reference_windows_dev(const char *d_reference, int64_t ref_len, int window_len, int stride,
                                   const int32_t *d_window_ids, int64_t first_id, int64_t n_rows,
                                   char *d_content, void *stream);
int bgsa_hip_reference_placements_dev(int64_t ref_len, int window_len, int stride,
                                      const int32_t *d_hit_windows, int64_t n_reads, int k,
                                      const int32_t *d_span, const int32_t *d_n_ops, int32_t *d_cigar, int cigar_cap,
                                      int32_t *d_strand, int64_t *d_ref_begin, int64_t *d_ref_end, int32_t *d_keep,
                                      void *stream);

/* ---- seeded read mapping: an exact pigeonhole k-mer filter that names the windows worth verifying ----
 * The calls above choose a read's windows by scoring EVERY window.  These calls name, per read, the windows that CAN hold it
 * within a distance bound, verify exactly those, and leave hit lists in the format bgsa_hip_top_queries_dev leaves — so that
 * bgsa_hip_myers_place_pairs_banded_dev and bgsa_hip_reference_placements_dev finish the job unchanged.  Every result is exact:
 * the lists equal the exhaustive ones with the hits beyond the bound left out.
 * PIGEONHOLE.  A read of n bp placed with at most B = min(max_distance, n) unit-cost edits, cut into B + 1 disjoint pieces: an
 * edit touches at most one piece, so one piece lies on the reference unedited, on a diagonal within B of the placement's.
 * GEOMETRY (normative; bgsa_amd/reference.py: seed_plan, and tests/seed_map_reference.py restate it).  Windows, ids and strands
 * are those of "a reference as the query set" above: L mapped bytes, 1 <= S <= W <= L, start(w) = min(w * S, L - W).
 *   index       the forward reference only.  q = seed_len, 1 <= q <= 13.  Position p is indexed when ref[p .. p + q) are all
 *               below 4 (no k-mer with an 'N'); its value is sum over i of ref[p + i] * 4^(q - 1 - i).  d_offsets: int32,
 *               bgsa_hip_seed_index_offsets(q) = 4^q + 1 entries; d_positions: int32, at least max(L - q + 1, 1) entries; bucket
 *               c is d_positions[d_offsets[c] .. d_offsets[c + 1]), in no particular order.  ref_len above INT32_MAX is refused;
 *               ref_len < q gives an empty index (every offset 0).
 *   pieces      step = n / (B + 1) (integer division); piece j = 0 .. B starts at o_j = j * step and is q long.  step < q is
 *               BGSA_HIP_EINVAL: the pieces would overlap.  Forward strand: the pieces of the read.  Reverse strand: the pieces
 *               of the read's reverse complement, looked up in the same forward index; a window w found that way has id
 *               n_windows + w.  Read bytes get the classes of the subject preprocess: A C G T N = 0..4, any other byte 0.
 *   candidates  an occurrence at p of the piece at o makes window w a candidate when all four hold:
 *                 start(w) <= p;  p + q <= start(w) + W      (the seed lies inside the window)
 *                 start(w) <= p - o + B;  p - o + n - B <= start(w) + W      (so do both ends of any placement within B through it)
 *               Every window whose semi-global distance to the read is <= B is a candidate of a read that is not flagged.
 *   flags       -1: one of the read's pieces (both strands' pieces with both_strands != 0) holds class 4 — 'N' matches 'N' in
 *               the scorer and the index has no 'N', so the pigeonhole count does not hold; -2: the read has more than
 *               max_candidates candidates (counted with repetitions).  A flagged read is answered by the exhaustive calls.
 * bgsa_hip_seed_index_offsets / _workspace_bytes: host only.  -1 / 0 for a seed_len outside 1..13 (or ref_len outside int32).
 * bgsa_hip_seed_index_build_dev: a rolling-code count, an inclusive scan over the 4^q counts and a fill, all on `stream`.
 * bgsa_hip_seed_count_candidates_dev: d_counts[r], r < n_reads = the candidates of read r over the strands asked for, or a flag.
 * d_reads: ASCII rows, stride read_len + 1 (the rows bgsa_hip_handle_reads_dev takes).
 * bgsa_hip_seed_emit_candidates_dev: with d_prefix[r] int64 = the sum of the non-negative d_counts in front of r (the caller's
 * scan), read r with d_counts[r] >= 0 writes (read_base + r, window id) to d_cand_read / d_cand_window [d_prefix[r] ..
 * d_prefix[r] + d_counts[r]), in no particular order and with repetitions; the caller sorts and deduplicates.
 * bgsa_hip_reference_verify_pairs_dev: for every owned pair p, d_distance[p] = the exact Myers semi-global distance of read
 * d_pair_subject[p] - subject_base inside window d_pair_window[p]: minus the entry the scoring call puts in the tile for that
 * window row and read.  One pair per lane; the window's characters are read straight from d_reference (forward ids forwards,
 * reverse ids complemented from the window's end backwards): no window row is written anywhere.  d_peq, read_count and
 * word_num are the resident bucket's.  A pair is owned when its subject lies in [subject_base, subject_base + read_count); an
 * owned pair whose window id lies outside [0, 2 * n_windows) forms no address; neither kind has its d_distance entry touched.
 * word_num 1..32 (BGSA_HIP_EUNSUPPORTED beyond); reads beyond 16 words run as column blocks and need a workspace of
 * bgsa_hip_reference_verify_workspace_bytes(W, read_len, n_pairs) (at least that of one wave: n_pairs = 0), narrower ones none.
 * bgsa_hip_seed_select_dev: the candidates of read r are entries [d_segments[r], d_segments[r + 1]) (int64, n_reads + 1
 * entries) of d_cand_window / d_cand_distance, window ids ascending and distinct within a read.  Fills d_hit_scores[r][k] (minus
 * the distance; INT32_MIN = unused) and d_hit_windows[r][k] (-1 = unused) with the read's k best candidates of distance in
 * [0, max_distance], best first by (distance ascending, id ascending).  k in 1..64.  One wave per read.
 * All device calls only launch on `stream`: no allocation, no synchronisation.  A zero count is BGSA_HIP_OK and launches
 * nothing.  BGSA_HIP_EINVAL, checked before the first HIP call: a NULL pointer (the stream, the workspace of a narrow verify and
 * the candidate arrays of an empty select excepted), seed_len outside 1..13, a shape outside 1 <= S <= W <= L, ref_len above
 * INT32_MAX, 2 * n_windows above INT32_MAX, a negative count, step < seed_len, a workspace too small, a word_num that is not
 * ceil(read_len / 32), read_count no positive multiple of 64, k outside 1..64.
 * READS OF MIXED LENGTHS IN ONE BUCKET (the three *_lens_dev calls).  d_read_lens: int32, one entry per column of the bucket,
 * padding columns included, with the rules of bgsa_hip_myers_place_score_lens_dev: a length is clamped to [0, read_len] and
 * clamped again wherever it forms an index; NULL is BGSA_HIP_EINVAL.  read_len is the bucket's width: d_reads are rows of stride
 * read_len + 1 and d_peq is what bgsa_hip_handle_reads_dev built at read_len.
 * bgsa_hip_seed_count_candidates_lens_dev / _emit_candidates_lens_dev: read r is its row's first n_r = d_read_lens[r] characters,
 * with B_r = min(max_distance, n_r) and step_r = n_r / (B_r + 1); its pieces start at j * step_r, j = 0 .. B_r, and are seed_len
 * long; the four candidate inequalities above hold with n_r and B_r.  Flag -3: step_r < seed_len, or n_r == 0 — the read is too
 * short for this seed and bound, and nothing of its row is read.  The whole-call refusal of step < seed_len does not apply: the
 * flag replaces it.  -1 looks only at the pieces, which lie inside n_r: the pad behind a read's end never flags it.  -2 as above.
 * Emit skips every negative count.
 * bgsa_hip_reference_verify_pairs_lens_dev: lane p verifies column c = d_pair_subject[p] - subject_base at n = d_read_lens[c]:
 * d_distance[p] = the Myers semi-global distance of the read's first n characters inside the window, bit for bit minus the score
 * bgsa_hip_myers_place_score_lens_dev writes for that (window, column); n == 0 gives 0.  What the columns above n hold never
 * enters a result.  Workspace, chunking, ownership and the "no window" rule are those of bgsa_hip_reference_verify_pairs_dev;
 * any lengths may share a bucket, at every width up to 32 words.  bgsa_hip_seed_select_dev needs no per-read form: a semi-global
 * distance never exceeds n_r.
 * bgsa_hip_reference_verify_kernel_name(word_num, lens): host only.  The kernel instance the two verify calls launch for a bucket
 * of word_num words — lens != 0: the *_lens_dev call —, e.g. "reference_verify_pairs_kernel<8, false, true>" (words per block,
 * column blocks, per-lane lengths); the choice is the launch's own.  It knows no limit: beyond 32 words it names the column-block
 * instance the calls refuse to launch.  The string is the calling thread's and lives until its next call. */
int64_t bgsa_hip_seed_index_offsets(int seed_len);
size_t bgsa_hip_seed_index_workspace_bytes(int64_t ref_len, int seed_len);
int bgsa_hip_seed_index_build_dev(const char *d_reference, int64_t ref_len, int seed_len, int32_t *d_offsets, int32_t *d_positions,
                                  void *d_workspace, size_t workspace_bytes, void *stream);
int bgsa_hip_seed_count_candidates_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                                       const int32_t *d_positions, int seed_len, const char *d_reads, int read_len, int64_t n_reads,
                                       int max_distance, int both_strands, int64_t max_candidates, int32_t *d_counts, void *stream);
int bgsa_hip_seed_emit_candidates_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                                      const int32_t *d_positions, int seed_len, const char *d_reads, int read_len, int64_t n_reads,
                                      int max_distance, int both_strands, const int32_t *d_counts, const int64_t *d_prefix,
                                      int64_t read_base, int32_t *d_cand_read, int32_t *d_cand_window, void *stream);
size_t bgsa_hip_reference_verify_workspace_bytes(int window_len, int read_len, int64_t n_pairs);
const char *bgsa_hip_reference_verify_kernel_name(int word_num, int lens);
int bgsa_hip_reference_verify_pairs_dev(const char *d_reference, int64_t ref_len, int window_len, int stride, const hip_read_t *d_peq,
                                        int read_len, int64_t read_count, int word_num, const int32_t *d_pair_window,
                                        const int64_t *d_pair_subject, int64_t n_pairs, int64_t subject_base, int32_t *d_distance,
                                        void *d_workspace, size_t workspace_bytes, void *stream);
int bgsa_hip_seed_count_candidates_lens_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                                            const int32_t *d_positions, int seed_len, const char *d_reads, const int32_t *d_read_lens,
                                            int read_len, int64_t n_reads, int max_distance, int both_strands, int64_t max_candidates,
                                            int32_t *d_counts, void *stream);
int bgsa_hip_seed_emit_candidates_lens_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                                           const int32_t *d_positions, int seed_len, const char *d_reads, const int32_t *d_read_lens,
                                           int read_len, int64_t n_reads, int max_distance, int both_strands, const int32_t *d_counts,
                                           const int64_t *d_prefix, int64_t read_base, int32_t *d_cand_read, int32_t *d_cand_window,
                                           void *stream);
int bgsa_hip_reference_verify_pairs_lens_dev(const char *d_reference, int64_t ref_len, int window_len, int stride, const hip_read_t *d_peq,
                                             const int32_t *d_read_lens, int read_len, int64_t read_count, int word_num,
                                             const int32_t *d_pair_window, const int64_t *d_pair_subject, int64_t n_pairs,
                                             int64_t subject_base, int32_t *d_distance, void *d_workspace, size_t workspace_bytes,
                                             void *stream);
int bgsa_hip_seed_select_dev(const int32_t *d_cand_window, const int32_t *d_cand_distance, const int64_t *d_segments, int64_t n_reads,
                             int max_distance, int k, int32_t *d_hit_scores, int32_t *d_hit_windows, void *stream);

/* ---- paired reads: the windows a mate can lie in, given the other end's placement, and the choice of the best proper pair ----
 * The calls above treat a read as a single end.  These two name, for an end of a pair, the windows next to its mate's placements
 * (so that the copy of a repeat beside a unique mate, or a mate beyond the single-end bound, is verified at all) and choose the
 * best proper combination of the two ends' lists.  Verification, selection and placement of the windows named here are
 * bgsa_hip_reference_verify_pairs_dev, bgsa_hip_seed_select_dev and bgsa_hip_reference_placements_dev, unchanged.
 * DEFINITIONS (normative; bgsa_amd/reference.py: rescue_slots, rescue_region, ReferenceMapper.map_pairs and tests/pair_reference.py
 * restate them).  Geometry, window ids, strands, keep, k_sel and the stride rule are those of "a reference as the query set": L
 * mapped bytes, W the window length, S the stride.  Library type FR only: the mates lie on opposite strands and the forward-strand
 * mate is upstream.
 *   inputs     reads1[ns][n1] and reads2[ns][n2], one length per end, each in 1..1,024; row c of both is pair c.  1 <= insert_min
 *              <= insert_max.  k_best and max_distance are required; rescue_distance >= max_distance (default: max_distance).
 *   stage A    each end alone: H_e = the seeded mapping of reads_e at (k_best, max_distance), or the exhaustive one with every
 *              slot beyond min(max_distance, n_e) blanked — the same lists, k_sel wide.
 *   stage B    the anchors of end e in pair c are the first k_best kept slots of the OTHER end's H, in list order.  An anchor on
 *              strand s with interval [b, e) puts the mate on strand 1 - s, in the region [b, min(L, b + insert_max)) for s = 0 and
 *              [max(0, e - insert_max), e) for s = 1.  Its rescue windows are the ids, on the mate's strand, of every forward
 *              window w with start(w) < region_hi and start(w) + W > region_lo: window starts never decrease, so one contiguous
 *              id range, of at most R = min(n_windows, ceil((insert_max + W - 1) / S) + 1) ids (attained).  The final list of end
 *              e in pair c: the union of H_e[c]'s window ids and the rescue windows of all its anchors, each id once, every id
 *              verified exactly, the k_pair = k_sel + k_best * R best of distance in [0, min(rescue_distance, n_e)] by (distance
 *              ascending, id ascending) — bgsa_hip_seed_select_dev's order — placed within that bound: a hit list of width k_pair
 *              with the ordinary keep.  A slot is RESCUED when its id is not among H_e[c]'s.  k_pair > 64 is refused, so nothing
 *              is truncated and the slots that are not rescued carry H_e[c]'s scores and windows, in order.
 *   stage C    over the kept slots r1 of end 1's final list and r2 of end 2's, a combination is PROPER when the strands differ
 *              and, F the forward-strand hit and R the reverse-strand one, F.begin <= R.begin, F.end <= R.end and insert_min <=
 *              R.end - F.begin <= insert_max.  Its cost is d1 + d2; the chosen one is the minimum by (cost, r1, r2).  Per pair:
 *              proper (0 | 1), slot1, slot2, insert (R.end - F.begin; 0 when not proper), cost, n_best (the proper combinations
 *              at the chosen cost), next_cost (the smallest proper cost above it, -1: none).  No proper combination: proper 0,
 *              slot_e = end e's first kept slot or -1, cost = the sum of the distances of the slots that exist, n_best 0,
 *              next_cost -1.
 *   limit      a window reports only its best placement, so a proper placement of a mate can be hidden by an equal or better
 *              improper one in the same window: the result is what the stages produce.  The stride rule applied at
 *              rescue_distance guarantees that every placement within that bound that lies wholly in a region lies wholly in at
 *              least one rescue window.
 * bgsa_hip_pair_rescue_slots: host only, no device — R; -1 with bgsa_hip_last_error() set for a shape outside 1 <= S <= W <= L
 * or an insert_max outside [1, 2^31 - 1].
 * bgsa_hip_pair_rescue_windows_dev: the anchor lists are d_strand / d_ref_begin / d_ref_end / d_keep [n_pairs][k], the layout
 * bgsa_hip_reference_placements_dev writes.  The r-th slot with keep != 0, r < k_anchor, is anchor r; it fills entries [r * R,
 * (r + 1) * R) of d_rescue[pair][k_anchor * R] (int32) with its rescue ids ascending, -1 behind them; a pair with fewer anchors
 * leaves the remaining groups at -1, so every entry of d_rescue is written.  A kept slot whose strand is neither 0 nor 1 or whose
 * interval is not 0 <= begin <= end <= L is an anchor without a region (a group of -1).  An id is a value and never forms an
 * address.  k and k_anchor in 1..64.  One wave per pair.
 * bgsa_hip_pair_select_dev: both ends' final lists (d_scores = minus the distance, d_strand, d_ref_begin, d_ref_end, d_keep; [n_pairs][k1]
 * and [n_pairs][k2], k1 and k2 in 1..64) and the insert range in, the seven outputs of stage C out (d_insert int64, the others
 * int32, one entry per pair).  A slot takes part when keep != 0, its strand is 0 or 1, ref_begin >= 0 and its score lies in
 * [-(2^30 - 1), 0].  One wave per pair: lanes take r1, each lane loops over r2, a wave-wide minimum over the key cost << 12 | r1 << 6
 * | r2 chooses, a second pass counts.
 * Both device calls only launch on `stream`: no allocation, no synchronisation; n_pairs == 0 is BGSA_HIP_OK and launches nothing.
 * BGSA_HIP_EINVAL, checked before the first HIP call: a NULL pointer (the stream excepted), a shape outside 1 <= S <= W <= L,
 * 2 * n_windows above INT32_MAX, insert_max outside [1, 2^31 - 1], insert_min outside [1, insert_max], k / k_anchor / k1 / k2
 * outside 1..64, a negative n_pairs. */
int64_t bgsa_hip_pair_rescue_slots(int64_t ref_len, int window_len, int stride, int64_t insert_max);
int bgsa_hip_pair_rescue_windows_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_strand, const int64_t *d_ref_begin,
                                     const int64_t *d_ref_end, const int32_t *d_keep, int64_t n_pairs, int k, int k_anchor,
                                     int64_t insert_max, int32_t *d_rescue, void *stream);
int bgsa_hip_pair_select_dev(const int32_t *d_scores1, const int32_t *d_strand1, const int64_t *d_ref_begin1, const int64_t *d_ref_end1,
                             const int32_t *d_keep1, int k1, const int32_t *d_scores2, const int32_t *d_strand2,
                             const int64_t *d_ref_begin2, const int64_t *d_ref_end2, const int32_t *d_keep2, int k2, int64_t n_pairs,
                             int64_t insert_min, int64_t insert_max, int32_t *d_proper, int32_t *d_slot1, int32_t *d_slot2,
                             int64_t *d_insert, int32_t *d_cost, int32_t *d_n_best, int32_t *d_next_cost, void *stream);

/* ---- SAM records: a mapping quality per hit list, and the text of every record written by the device into one byte buffer ----
 * The last stage of read mapping.  The calls above leave hit lists and edit scripts as arrays; these three turn them into the lines
 * a downstream tool reads, without a copy of the lists to the host: bgsa_hip_sam_mapq_dev chooses every read's primary slot and
 * its MAPQ, bgsa_hip_sam_measure_dev (pass 1) returns the byte length of every record, the caller takes an exclusive scan of the
 * lengths — one scalar read back sizes the buffer —, and bgsa_hip_sam_emit_dev (pass 2) writes the text.
 * DEFINITIONS (normative; bgsa_amd/reference.py: list_mapq, pair_mapq, ReferenceMapper.map_reads_sam / map_pairs_sam and
 * tests/sam_reference.py restate them).
 *   MAPQ of a list   scores[ns][k] (minus the distance), keep[ns][k] and `bound`, the distance within which the list is complete,
 *              -1 for none.  The PRIMARY slot is the first slot with keep != 0; none: primary -1, the read is unmapped, MAPQ 0, n1 0,
 *              d2 -1.  Otherwise d1 is its distance, n1 the kept slots at distance d1, d2 the smallest kept distance above d1 (-1:
 *              none).  n1 >= 2: MAPQ = 3, 2, 1, 0 for n1 = 2, 3, 4..9, >= 10.  n1 = 1: MAPQ = min(60, 10 * gap), never below 0, with
 *              gap = d2 - d1 if d2 exists, else bound + 1 - d1 if bound >= 0, else 6.  A stated heuristic in integers, calibrated
 *              against no other mapper; a second locus is only sure to be listed with k_best >= 2.
 *   MAPQ of a pair   from bgsa_hip_pair_select_dev's outputs, elementwise.  Proper: both ends get the table value of n_best when
 *              n_best >= 2, else min(60, 10 * (next_cost - cost)), 60 with next_cost == -1.  Not proper: each end gets the list MAPQ
 *              of its own final list at its own rescue bound; its record is its first kept slot (slot_e).
 *   a record   one entry per record in every per-record array of bgsa_hip_sam_batch_t.  strand -1: unmapped.
 *     CIGAR    the runs (length << 4 | op, d_runs[d_runs_row[i]][0 .. n_ops)) run along the forward reference, as
 *              bgsa_hip_reference_placements_dev leaves them.  In this library the window is the query, so op 1 'I' consumes a
 *              reference base only and op 2 'D' a read base only; SAM says the opposite: op 1 prints as D, op 2 as I, 7 as = and
 *              8 as X.
 *     SEQ/QUAL a forward hit or an unmapped read: the caller's bytes.  A reverse hit: SEQ reverse-complemented (A<->T, C<->G,
 *              anything else N), QUAL reversed.  d_quals NULL: '*'.
 *     POS      ref_begin + 1.  NM:i: is the distance.
 *     MD:Z:    read off the mapped reference (bgsa_hip_map_queries_dev's codes), class letters "ACGTN"[code] — a lower-case or
 *              IUPAC base is of class A and prints so.  Along [ref_begin, ref_end): a count of '=' bases runs through SAM I runs;
 *              before every X base and before every SAM D run the count is written, even when 0, and reset; an X base writes its
 *              reference letter, a D run '^' and its reference letters; the count is written once more at the end.  Grammar:
 *              [0-9]+(([ACGTN]|\^[ACGTN]+)[0-9]+)*.
 *     unmapped RNAME '*', POS 0, MAPQ 0, CIGAR '*', no tags; with rnext 1 (the end of a pair whose mate is mapped) RNAME is the
 *              reference's name and POS is pnext, the mate's.
 *     pairs    flags 1, 2 (proper), 4, 8, 16, 32 and 64 (end 1) or 128 (end 2) are the caller's, as are rnext (1: '=', the mate is
 *              mapped; 0: '*'), pnext (the mate's POS, or 0) and tlen (both ends mapped: the rightmost end minus the leftmost
 *              begin, positive for the end with the smaller begin — end 1 on equal begins —, negative for the other; else 0).
 *     line     QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL separated by tabs, a mapped record then tab NM:i:<d> tab
 *              MD:Z:<md>, then '\n'.
 *   malformed  a record is MALFORMED when n_ops > cigar_cap, ref_begin < 0, ref_end > ref_len (or below ref_begin), its
 *              reference-consuming runs do not sum to ref_end - ref_begin, its read-consuming runs do not sum to its read length,
 *              a run has length 0 or an op other than 1, 2, 7, 8 — these of a mapped record —, or when its read row, read length
 *              (1..read_stride), name id, name offsets, runs row, strand (-1, 0, 1), flag (0..65535), mapq (0..255), rnext (0, 1),
 *              pnext (>= 0), distance (>= 0) or n_ops (>= 0) lies outside its range.  Pass 1 gives it length 0, pass 2 writes nothing
 *              for it, each call adds the malformed records it met to *d_malformed, and none of its values forms an address.
 *              Pass 2 also treats as malformed a record whose line is not exactly d_offsets[i + 1] - d_offsets[i] bytes long or
 *              whose bytes would leave [0, text_bytes).
 * One wave per read (mapq) or per record; k in 1..64.  All three only launch on `stream`: no allocation, no synchronisation, no
 * workspace; n == 0 (ns == 0) is BGSA_HIP_OK and launches nothing.  BGSA_HIP_EINVAL, checked before the first HIP call: a NULL
 * pointer (the stream and d_quals excepted), k outside 1..64, bound below -1, a negative count, read_stride outside [1, 2^31 - 1],
 * n_read_rows, n_names, names_bytes, rname_len, ref_len, cigar_cap or n_run_rows below 1, a negative text_bytes.
 * The C loop: fill the batch; measure; lengths -> offsets[n + 1] by an exclusive scan; read offsets[n] back; allocate the text;
 * emit; read *d_malformed. */
typedef struct bgsa_hip_sam_batch {
    const uint8_t *d_reads;            /* ASCII rows: row r is d_reads + r * read_stride */
    const uint8_t *d_quals;            /* the same layout, or NULL: QUAL is '*' */
    int64_t read_stride, n_read_rows;
    const uint8_t *d_names;            /* QNAME bytes, flat: name j is [d_name_offsets[j], d_name_offsets[j + 1]) */
    const int64_t *d_name_offsets;     /* n_names + 1 entries */
    int64_t n_names, names_bytes;
    const uint8_t *d_rname;            /* the reference's name, rname_len bytes */
    int64_t rname_len;
    const uint8_t *d_reference;        /* the mapped reference (codes 0..4), ref_len bytes */
    int64_t ref_len;
    const uint32_t *d_runs;            /* [n_run_rows][cigar_cap]: length << 4 | op */
    int64_t n_run_rows;
    int64_t cigar_cap;
    /* one entry per record */
    const int64_t *d_read_row, *d_name_of, *d_runs_row;
    const int32_t *d_read_len, *d_strand;
    const int64_t *d_ref_begin, *d_ref_end;
    const int32_t *d_distance, *d_n_ops, *d_flag, *d_mapq, *d_rnext;
    const int64_t *d_pnext, *d_tlen;
} bgsa_hip_sam_batch_t;
int bgsa_hip_sam_mapq_dev(const int32_t *d_scores, const int32_t *d_keep, int64_t ns, int k, int bound, int32_t *d_primary, int32_t *d_mapq,
                          int32_t *d_n1, int32_t *d_d2, void *stream);
int bgsa_hip_sam_measure_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int64_t *d_lengths, int32_t *d_malformed, void *stream);
int bgsa_hip_sam_emit_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, const int64_t *d_offsets, uint8_t *d_text, int64_t text_bytes,
                          int32_t *d_malformed, void *stream);

/* ---- a reference of several contigs: one padded layout, hits clipped to their contig, records named by a table ----
 * The calls above map onto ONE sequence.  A reference of C contigs is laid out as one such sequence with padding between the
 * contigs; geometry, window ids, the k-mer index, verification, selection, placement and bgsa_hip_reference_placements_dev run
 * unchanged on it.  What is new sits behind them: the layout, a clip of every placed hit to its contig, and a contig form of the
 * two record passes.
 * DEFINITIONS (normative; bgsa_amd/reference.py: contig_layout, ContigMapper and tests/contig_reference.py restate them).
 *   layout     contigs i = 0..C-1 of len_i >= 1 bases, P >= W bytes of 'N' (code 4) between neighbours: start_0 = 0, start_{i+1} =
 *              start_i + len_i + P, L = start_{C-1} + len_{C-1}; a caller whose L is below W pads the end with 'N' up to W.  A
 *              contig may be shorter than the window or than a read.  With P >= W no window holds bases of two contigs, so a
 *              placement touches one contig and padding on either side; the stride rule gives completeness for every placement
 *              inside a contig; padding never seeds (a k-mer that holds an 'N' is not indexed).
 *   clip       of a placed hit (ref_begin >= 0) with interval [begin, end) and runs along the forward reference (ops 1 reference
 *              only, 2 read only, 7 '=', 8 'X').  Its contig c is the one that holds the first non-padding base of [begin, end) —
 *              of an empty interval, a hit of read-only bases alone: the one it lies in or at the edge of, and nothing is clipped;
 *              lead = max(0, start_c - begin), trail = max(0, end - (start_c + len_c)).  The runs are walked from the front for
 *              lead reference columns: a reference-only column is dropped (distance - 1), an X column becomes a read-only base
 *              (distance unchanged), an '=' column becomes a read-only base (distance + 1: a read's 'N' on padding); read-only
 *              runs met on the way, and one that follows directly where the last walked run was used up, stay read-only; all of
 *              these merge into ONE leading read-only run, followed by the rest of the split run.  The tail likewise, mirrored,
 *              on the front's result.  Then begin += lead, end -= trail, score = -(new distance), n_ops = the runs the script now
 *              needs — at most 2 more; above cigar_cap the row is left as it was and n_ops says what is needed.  Entries of the
 *              row at and behind the new n_ops are not written.  A hit with no contig (an interval outside [0, L] or with begin >
 *              end, or padding only) becomes unplaced: begin and end -1, n_ops 0, contig -1; its score and strand stay.  A row
 *              whose n_ops lay outside [0, cigar_cap] before the call is not clipped.  keep of the whole list is then walked again
 *              on the clipped intervals by bgsa_hip_reference_placements_dev's rule.
 *   limits     the list is not sorted again: a clipped hit whose 'N' bases stood on padding can carry a distance above its
 *              neighbour's, and above the bound it was selected within.  For a read without 'N' the clipped distance of a best hit
 *              is the semi-global distance of the read against its contig alone.
 *   pairs      bgsa_hip_pair_select_dev runs unchanged on the CLIPPED linear coordinates.  Mates on different contigs are at
 *              least P apart, so with insert_max <= P — a caller with a larger one is refused — they are never proper.  Rescue
 *              regions may reach into padding: that costs windows, not correctness.
 *   records    the contig form of "SAM records": the batch's ref_begin, ref_end and pnext (the mate's POS: its begin + 1) are
 *              LINEAR; d_rname and rname_len are not read.  A mapped record's contig c holds ref_begin, and ref_end <= start_c +
 *              len_c, else the record is malformed; RNAME is name c, POS = ref_begin - start_c + 1.  With rnext 1 the mate's contig
 *              m holds pnext - 1 (on padding, or pnext < 1: malformed), PNEXT = pnext - start_m; RNEXT is '=' when m = c, else name
 *              m; an unmapped record takes RNAME m, POS = PNEXT and '='.  TLEN is the caller's: 0 across contigs.  MD reads the
 *              linear reference.  A table entry outside the reference (start < 0, len < 1, start + len > ref_len) or a name outside
 *              its bytes makes the records that meet it malformed.  Everything else — the two-pass contract, the counting, values
 *              that never form addresses — is that of the one-sequence calls, whose output does not change.
 * bgsa_hip_contig_layout: host only, no device — starts_out[n_contigs] and *total_out = L.  BGSA_HIP_EINVAL: a NULL pointer,
 * n_contigs < 1, a length below 1, padding < window_len (or window_len < 1), a total beyond int64.
 * bgsa_hip_contig_clip_dev: the lists are d_scores / d_strand / d_ref_begin / d_ref_end / d_keep / d_n_ops [n_reads][k] and
 * d_cigar [n_reads][k][cigar_cap] as bgsa_hip_reference_placements_dev leaves them; d_scores, d_ref_begin, d_ref_end, d_keep,
 * d_n_ops and d_cigar are rewritten in place, d_contig (int32 [n_reads][k]) is written: the contig of every placed slot, -1
 * elsewhere.  d_starts / d_lens: int64 [n_contigs] on the device.  One wave per read, one lane per slot, k in 1..64; the contig by
 * binary search.  Only a launch on `stream`: no allocation, no synchronisation; n_reads == 0 is BGSA_HIP_OK and launches nothing.
 * BGSA_HIP_EINVAL, checked before the first HIP call: a NULL pointer (the stream excepted), n_contigs outside [1, 2^31 - 1],
 * ref_len < 1, k outside 1..64, cigar_cap < 1, a negative n_reads.
 * bgsa_hip_sam_measure_contigs_dev / bgsa_hip_sam_emit_contigs_dev: bgsa_hip_sam_measure_dev / _emit_dev with the table; the
 * same refusals (d_rname and rname_len excepted), and a NULL table, a NULL pointer in it, n_contigs outside [1, 2^31 - 1] or
 * names_bytes < 1. */
typedef struct bgsa_hip_sam_contigs {
    const uint8_t *d_names;            /* the contigs' names, flat: name c is [d_name_offsets[c], d_name_offsets[c + 1]) */
    const int64_t *d_name_offsets;     /* n_contigs + 1 entries */
    int64_t names_bytes;
    const int64_t *d_starts, *d_lens;  /* n_contigs entries each: the layout */
    int64_t n_contigs;
} bgsa_hip_sam_contigs_t;
int bgsa_hip_contig_layout(const int64_t *lens, int64_t n_contigs, int window_len, int64_t padding, int64_t *starts_out, int64_t *total_out);
int bgsa_hip_contig_clip_dev(const int64_t *d_starts, const int64_t *d_lens, int64_t n_contigs, int64_t ref_len, int64_t n_reads, int k,
                             int32_t *d_scores, const int32_t *d_strand, int64_t *d_ref_begin, int64_t *d_ref_end, int32_t *d_keep,
                             int32_t *d_n_ops, int32_t *d_cigar, int cigar_cap, int32_t *d_contig, void *stream);
int bgsa_hip_sam_measure_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, int64_t *d_lengths,
                                     int32_t *d_malformed, void *stream);
int bgsa_hip_sam_emit_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, const int64_t *d_offsets,
                                  uint8_t *d_text, int64_t text_bytes, int32_t *d_malformed, void *stream);

/* ---- BAM records: the records of "SAM records" in BAM's binary layout, and BGZF blocks around them, written by the device ----
 * What downstream tools read is BAM, not text.  The same bgsa_hip_sam_batch_t (and bgsa_hip_sam_contigs_t) goes through two passes
 * of the same contract as the SAM ones — bgsa_hip_bam_measure_dev returns every record's byte length, the caller scans the
 * lengths and reads one scalar back, bgsa_hip_bam_emit_dev writes the records into one payload buffer —, and
 * bgsa_hip_bgzf_frame_dev then wraps the payload into BGZF blocks of STORED deflate: a valid BAM stream once the caller puts the
 * header in front and the EOF block behind (bgsa_amd/reference.py: bam_header, write_bam, BGZF_EOF).  The compressing form of the
 * framing is "deflate" below.
 * DEFINITIONS (normative; SAMv1 §4.1, §4.2, §5.3; tests/bam_reference.py restates them).
 *   a record   every value is that of the record's SAM line; all integers little-endian; a record starts at any byte address.
 *     block_size  int32: the record's length minus these 4 bytes.  d_lengths[i] and the offsets count the 4 bytes in.
 *     refID, pos  int32: the contig's index (0 in the one-sequence calls) and POS - 1.  An unmapped end beside a mapped mate
 *              (rnext 1) takes the mate's, as the line does; any other unmapped record -1 and -1.
 *     l_read_name uint8: the name's length + 1.     mapq uint8: 0 when unmapped.
 *     bin      uint16: reg2bin(pos, end) of SAMv1 §5.3, its low 16 bits; end = pos + the reference bases of the runs, pos + 1
 *              where that is 0 or the record is unmapped; 4680 = reg2bin(-1, 0) where pos is -1.
 *     n_cigar_op uint16 (0 when unmapped), flag uint16, l_seq uint32 (the read's length).
 *     next_refID, next_pos, tlen   int32: RNEXT as an index ('=': the record's refID, '*': -1), PNEXT - 1, TLEN.
 *     read_name  the name and a NUL.
 *     cigar    uint32[n_cigar_op], length << 4 | op: the library's run op 1 (reference only) is BAM's D 2, op 2 (read only) I 1,
 *              7 '=' stays 7, 8 'X' stays 8.
 *     seq      uint8[(l_seq + 1) / 2]: SEQ as the line prints it (a reverse hit reverse-complemented, anything but ACGT then N), two
 *              bases a byte, the first in the high nibble, each the letter's index in "=ACMGRSVTWYHKDBN" whatever its case, 15
 *              for any other byte; a last odd nibble is 0.
 *     qual     uint8[l_seq]: QUAL - 33, reversed on a reverse hit; 0xff in every byte where d_quals is NULL.
 *     tags     of a mapped record only: 'N' 'M' 'i' and the distance as int32; 'M' 'D' 'Z', the MD text of "SAM records", a NUL.
 *   malformed  what "SAM records" (and its contig form) calls malformed, and a name longer than 254 bytes, n_ops > 65535, a POS - 1,
 *              PNEXT - 1 or TLEN outside int32 (the read's length is an int32 already).  Pass 1 gives such a record length 0, pass 2
 *              writes nothing for it, each call adds the malformed records it met to *d_malformed, and none of its values forms an
 *              address.  Pass 2 also treats as malformed a record that is not exactly d_offsets[i + 1] - d_offsets[i] bytes long
 *              or whose bytes would leave [0, payload_bytes).
 *   BGZF       block b of the framed output carries payload bytes [b * P, min((b + 1) * P, total)), P = block_payload, LEN of
 *              them: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, the subfield 'B' 'C' 2 0 BSIZE with BSIZE = LEN + 30 (the block's
 *              length - 1), one stored deflate block 01 LEN ~LEN (uint16 each), the bytes, their CRC-32 (IEEE, reflected: zlib's),
 *              ISIZE = LEN: LEN + 31 bytes.  Blocks follow one another without gaps; the last may be shorter; an empty payload
 *              gives no block.  The 28-byte EOF block is NOT written: it belongs to the file, not to a batch.  The framing knows
 *              nothing about BAM; a record may straddle blocks.
 * bgsa_hip_bgzf_framed_bytes: host only — payload_bytes + 31 * ceil(payload_bytes / block_payload); 0 for an empty payload; -1 for
 * a negative payload_bytes, one beyond 2^58, or a block_payload outside 1..65280 (0xff00, what every BGZF writer uses; the
 * format's own limit is 65505).
 * One wave per record; one workgroup per BGZF block, its threads on contiguous slices whose CRC states are joined by the CRC's
 * linearity (bgzf.hip).  All five device calls only launch on `stream`: no allocation, no synchronisation, no workspace; n == 0
 * and payload_bytes == 0 are BGSA_HIP_OK and launch nothing.  BGSA_HIP_EINVAL, checked before the first HIP call: what the SAM
 * passes refuse (payload_bytes for text_bytes); for the framing a NULL pointer (the stream excepted), a block_payload outside
 * 1..65280, a negative payload_bytes, an out_bytes that is not bgsa_hip_bgzf_framed_bytes(payload_bytes, block_payload).
 * The C loop: fill the batch; measure; lengths -> offsets[n + 1]; read offsets[n] back; allocate payload and framed output; emit;
 * frame; read *d_malformed. */
int bgsa_hip_bam_measure_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int64_t *d_lengths, int32_t *d_malformed, void *stream);
int bgsa_hip_bam_emit_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, const int64_t *d_offsets, uint8_t *d_payload, int64_t payload_bytes,
                          int32_t *d_malformed, void *stream);
int bgsa_hip_bam_measure_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, int64_t *d_lengths,
                                     int32_t *d_malformed, void *stream);
int bgsa_hip_bam_emit_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, const int64_t *d_offsets,
                                  uint8_t *d_payload, int64_t payload_bytes, int32_t *d_malformed, void *stream);
int64_t bgsa_hip_bgzf_framed_bytes(int64_t payload_bytes, int block_payload);
int bgsa_hip_bgzf_frame_dev(const uint8_t *d_payload, int64_t payload_bytes, int block_payload, uint8_t *d_out, int64_t out_bytes, void *stream);

/* BAM records: deflate — the same BGZF blocks with their payload DEFLATED on the device (RFC 1951; bgzf_deflate.hip).  Block b
 * carries the same payload bytes as above; its 18 header bytes, CRC-32 and ISIZE are the framing's, BSIZE is the real length - 1,
 * and the deflate data between them is ONE deflate block with BFINAL = 1 in one of two forms: STORED, byte for byte what
 * bgsa_hip_bgzf_frame_dev writes, or DYNAMIC (BTYPE 10) — chosen if and only if its byte length is strictly smaller than the stored
 * form's LEN + 5, from the exact bit count, before a bit is written.  So a block is never longer than LEN + 31, and blocks are
 * independent: no match reaches into another block's bytes.  The output is a pure function of (payload, block_payload) — not of
 * timing, not of the device — and tests/deflate_reference.py, the NORMATIVE model, reproduces it byte for byte:
 *   matches  positions in tiles of 1,024; position i tries i - 1 and, if i + 4 <= LEN, the greatest position of any EARLIER tile
 *            whose 4 bytes hash alike (little-endian word * 0x9E3779B1, top 15 bits) at a distance <= 32,768; lengths by comparison,
 *            at most 258 and the block's end; the longer wins, a tie goes to distance 1; used from length 4, or 3 below 4,096
 *   parse    greedy from position 0
 *   codes    Huffman lengths of the 286 + 30 counts (EOB once): Moffat and Katajainen's in-place method on the used symbols sorted
 *            by (count, symbol); limited to 15 by clamping and repairing the Kraft sum a unit at a time (miniz's rule); the
 *            shortest lengths to the greatest counts; canonical codes.  One used distance symbol: length 1; none: all 30 lengths 0
 *   header   HLIT 286, HDIST 30, HCLEN 19, the code-length code FIXED (symbols 0..15 at 4 bits, 16..18 unused): every one of the
 *            316 lengths is its own 4-bit symbol, 1,338 bits in all; a block of up to 163 bytes is therefore always stored
 * The stage's two-pass idiom: bgsa_hip_bgzf_deflate_dev writes block b complete at the start of slot b of d_slots (slots of
 * block_payload + 31 bytes; the rest of a slot is not touched) and its length into d_block_bytes[b]; the caller makes
 * d_block_offsets[n_blocks + 1], the exclusive scan of the lengths, reads ONE scalar back — out_bytes = d_block_offsets[n_blocks] —
 * and bgsa_hip_bgzf_pack_dev copies block b to d_out + d_block_offsets[b].  pack does not copy a block whose offsets are not
 * monotone or negative, whose length exceeds its slot or whose extent leaves [0, out_bytes): each such block adds 1 to *d_refused
 * (the caller zeroes it), and no value read from device memory forms an address unchecked.
 * bgsa_hip_bgzf_deflate_workspace_bytes: host only — 4 * payload_bytes (a word per payload byte: the parse); 0 for an empty payload;
 * -1 where bgsa_hip_bgzf_framed_bytes gives -1.  d_workspace is aligned to 4 bytes; payload, slots and output start anywhere.
 * One workgroup of 1,024 threads per block, 141 KiB of LDS: one workgroup per CU.  Both device calls only launch on `stream`: no
 * allocation, no synchronisation; an empty payload (n_blocks == 0) is BGSA_HIP_OK and launches nothing.  BGSA_HIP_EINVAL, before
 * the first HIP call: a NULL pointer (the stream excepted), a block_payload outside 1..65280, a negative or overflowing
 * payload_bytes, a slots_bytes that is not n_blocks * (block_payload + 31), a workspace_bytes below the function's value, a
 * misaligned d_workspace; for pack a negative n_blocks or out_bytes. */
int64_t bgsa_hip_bgzf_deflate_workspace_bytes(int64_t payload_bytes, int block_payload);
int bgsa_hip_bgzf_deflate_dev(const uint8_t *d_payload, int64_t payload_bytes, int block_payload, uint8_t *d_slots, int64_t slots_bytes,
                              int64_t *d_block_bytes, void *d_workspace, int64_t workspace_bytes, void *stream);
int bgsa_hip_bgzf_pack_dev(const uint8_t *d_slots, int block_payload, int64_t n_blocks, const int64_t *d_block_offsets, uint8_t *d_out,
                           int64_t out_bytes, int32_t *d_refused, void *stream);

/* ---- BAM records: coordinate order and index — the keys a caller sorts a batch by, and the arrays of a BAI index (SAMv1 §5.2) ----
 * Downstream tools take a coordinate-sorted, indexed BAM.  bgsa_hip_bam_coordinates_dev gives every record of a batch its sort key
 * and coordinates; the caller sorts the keys (stable), gathers the per-record arrays of the batch by the permutation — d_runs_row
 * becomes the permutation, no run moves — and runs measure, scan, emit and frame (or deflate and pack) as above.  From the SORTED
 * coordinates, the record offsets and the block offsets, bgsa_hip_bam_index_marks_dev and bgsa_hip_bam_index_chunks_dev then build
 * the index arrays (bam_index.hip; bgsa_amd/reference.py: sam_records(sort=True), bai_bytes, write_bam(index=True)).
 * DEFINITIONS (normative; tests/bai_reference.py restates them).
 *   coordinates  the values the record pass writes for the same record ("BAM records", the contig form included): refID and pos
 *              of a mapped record its contig's index (0 on one sequence) and POS - 1; of an unmapped end with rnext 1 its mate's;
 *              of any other unmapped record -1 and -1.  end = pos + (ref_end - ref_begin) of a mapped record (pos + 1 where that
 *              is 0, as its bin counts it), pos + 1 of an unmapped but placed one, 0 with pos -1.  bin = reg2bin(pos, end) in
 *              full (not cut to 16 bits), 4680 with pos -1.
 *   key        a non-negative int64, the order of `samtools sort`: ref' << 32 | (pos + 1) << 1 | reverse; ref' = refID, or
 *              0x7fffffff where refID is -1 (no coordinates: last); reverse = flag >> 4 & 1.  Ties keep input order (a STABLE
 *              sort): of two ends at one position end 1 stays in front, and an unmapped end that ties with the mate it borrowed its
 *              position from stays right behind it (a reverse mate's key is one greater: the unmapped end goes in front).
 *   malformed  for the key kernel: strand outside -1..1; rnext outside 0..1, pnext < 0, rnext 1 with pnext < 1; a mapped
 *              ref_begin < 0, ref_end < ref_begin or ref_end > ref_len; in the contig form what "records" there calls malformed
 *              about the contig of ref_begin or of pnext - 1; pos + 1 or end beyond 2^29, a BAI's reach.  Such a record gets the key
 *              INT64_MAX, refID -1, pos -1, end 0, bin 4680 and adds 1 to *d_malformed; no value of it forms an address.  The kernel
 *              does not walk the runs: the measure pass that follows on the permuted batch still applies the full record check.
 *   virtual offset  of a payload offset o, P = block_payload: block_start(o / P) << 16 | o % P; block_start(b) = b * (P + 31) for
 *              stored blocks, d_block_offsets[b] (n_blocks + 1 entries, the scan bgsa_hip_bgzf_pack_dev takes) for deflated ones; so
 *              o = payload_bytes on a block boundary gives out_bytes << 16.  Record i: voff_beg that of d_offsets[i], voff_end that
 *              of d_offsets[i + 1].  All relative to the first byte of the call's blocks: a file adds base << 16, base the byte
 *              length of the framed header in front.
 *   chunks     over the sorted records with refID >= 0, every maximal run of consecutive records of equal (refID, bin) is one
 *              chunk (refID, bin, voff_beg of its first record, voff_end of its last) — htslib's hts_idx_push rule, without its
 *              later merge of small bins.  The list is ordered by (refID, bin, beg).
 *   linear     reference c has ceil(len_c / 16384) windows; linear[c][w] = the smallest voff_beg of a record of c with
 *              pos >> 14 <= w <= (end - 1) >> 14, unmapped-placed records included; n_intv[c] = 1 + the last non-empty window, 0
 *              without one; an empty window below n_intv[c] takes the value of the next non-empty one (a suffix minimum).
 *   metadata   pseudo-bin 37450 of every reference with a record: (smallest voff_beg, largest voff_end), then (records with flag 4
 *              clear, records with flag 4 set); n_no_coor = the records with refID -1.
 *   .bai       "BAI\1", n_ref; per reference n_bin, per bin ascending and 37450 last: bin, n_chunk, the chunks as uint64 pairs;
 *              n_intv and the ioffsets; n_no_coor at the end.  All little-endian.  A reference without records: n_bin 0, n_intv 0.
 * bgsa_hip_bam_coordinates_dev / _contigs_dev: one THREAD per record of the batch as assembled; d_key int64[n], the others int32[n].
 * bgsa_hip_bam_index_windows: host only — window_base_out[n_refs + 1] = the exclusive scan of ceil(len / 16384); returns the
 * total, -1 for a NULL pointer, a negative n_refs or a length < 1 or > 2^29.
 * bgsa_hip_bam_index_marks_dev: SORTED coordinates in; per record d_voff_beg, d_voff_end and d_chunk_start — 1 where refID >= 0
 * and (i == 0 or (refID, bin) differs from record i - 1's), else 0 —, and the linear minima by a 64-bit atomicMin on
 * d_linear[d_window_base[refID] + w], which the caller filled with INT64_MAX (d_window_base[n_refs] entries); a window the
 * record's predecessor on the same reference covers is skipped: that offset is smaller.  d_block_offsets NULL: stored blocks.  A
 * record is REFUSED — it adds 1 to *d_refused (the caller zeroes it), gets flag 0 and touches nothing else — when refID is outside
 * [-1, n_refs); refID >= 0 and pos < 0, end <= pos, or end beyond the reference's windows (or the window table is not monotone);
 * its offsets are negative, not monotone or beyond payload_bytes; its block is beyond n_blocks; it stands before its predecessor
 * in (ref', pos) order.
 * bgsa_hip_bam_index_chunks_dev: d_chunk_of = the inclusive scan of d_chunk_start (the caller's; n_chunks its last entry, one
 * scalar read back); chunk c = d_chunk_of[i] - 1.  A start writes ref, bin and beg of its chunk; a record with refID >= 0 whose
 * successor is a start, has refID -1 or does not exist writes end.  A d_chunk_of[i] outside 1..n_chunks is refused and counted.
 * The caller then sorts the chunks by ref << 32 | bin (stable) and takes the suffix minimum over d_linear.
 * The four device calls only launch on `stream`: no allocation, no synchronisation; n == 0 is BGSA_HIP_OK and launches nothing.
 * BGSA_HIP_EINVAL, before the first HIP call: a NULL pointer (the stream, d_quals and d_block_offsets excepted), a negative count,
 * a block_payload outside 1..65280, what the SAM passes refuse about the batch and the table.
 * LIMITS: one call, one sorted file (no merge of batches); BAI only (contigs up to 2^29 bases, no CSI); no merge of small bins. */
int bgsa_hip_bam_coordinates_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int64_t *d_key, int32_t *d_ref_id, int32_t *d_pos,
                                 int32_t *d_end, int32_t *d_bin, int32_t *d_malformed, void *stream);
int bgsa_hip_bam_coordinates_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, int64_t *d_key,
                                         int32_t *d_ref_id, int32_t *d_pos, int32_t *d_end, int32_t *d_bin, int32_t *d_malformed, void *stream);
int64_t bgsa_hip_bam_index_windows(const int64_t *ref_lens, int64_t n_refs, int64_t *window_base_out);
int bgsa_hip_bam_index_marks_dev(const int32_t *d_ref_id, const int32_t *d_pos, const int32_t *d_end, const int32_t *d_bin, int64_t n,
                                 const int64_t *d_offsets, int64_t payload_bytes, int block_payload, const int64_t *d_block_offsets,
                                 int64_t n_blocks, const int64_t *d_window_base, int64_t n_refs, int64_t *d_voff_beg, int64_t *d_voff_end,
                                 int32_t *d_chunk_start, int64_t *d_linear, int32_t *d_refused, void *stream);
int bgsa_hip_bam_index_chunks_dev(const int32_t *d_ref_id, const int32_t *d_bin, const int64_t *d_voff_beg, const int64_t *d_voff_end,
                                  const int32_t *d_chunk_start, const int64_t *d_chunk_of, int64_t n, int64_t n_chunks,
                                  int32_t *d_chunk_ref, int32_t *d_chunk_bin, int64_t *d_chunk_beg, int64_t *d_chunk_end,
                                  int32_t *d_refused, void *stream);

/* ---- Duplicate marking: flag 0x400 on the PCR copies of ONE batch, before its records are written ----
 * After `sort`, short-read workflows mark duplicates (Picard MarkDuplicates, samtools markdup).  Everything that needs is in the
 * batch already, and the flag is a per-record scalar both record passes read: flags changed before the passes reach the SAM text,
 * the BAM records, the sorted order and the index (the sort key reads bit 16 of the flag only).  bgsa_hip_dup_keys_dev writes the
 * keys and scores of a batch as assembled, the caller orders them with stable sorts, bgsa_hip_dup_mark_dev ORs 1024 into the flags
 * (mark_duplicates.hip; bgsa_amd/reference.py: sam_records(mark_duplicates=True), mark_duplicate_records).
 * DEFINITIONS (normative; tests/markdup_reference.py restates them).  The Picard core: no optical duplicates, no UMIs, no libraries.
 *   malformed  a record with strand outside -1..1, read_len < 0 or > read_stride, read_row outside [0, n_read_rows), or, mapped
 *              (strand >= 0), ref_begin < 0, ref_end < ref_begin or ref_end > ref_len.  It takes its whole unit out of marking,
 *              adds 1 to the skipped count and forms no address; the measure pass that follows refuses it as ever.
 *   5' coordinate  of a mapped record: ref_begin on strand 0; ref_end - 1 on strand 1 (ref_begin where ref_end == ref_begin).
 *              Linear, as in the batch — after the contig clip where there is one —: the coordinate of the record AS WRITTEN
 *              (placement is end to end, no record carries a soft clip, so this is the unclipped 5' position).
 *   units      ends 1: every mapped record is a fragment unit.  ends 2: records 2u and 2u + 1 are pair u; both mapped (proper or
 *              not): one pair unit; exactly one mapped: that end is a fragment unit.  Unmapped records are in no unit.
 *   score      of a unit: the sum of q - 33 over the QUAL bytes of its mapped records with q - 33 >= min_quality (Picard's
 *              SUM_OF_BASE_QUALITIES at 15), at most 2^31 - 1; 0 without QUAL.
 *   pair pass  half(e) = 5' << 1 | strand; the pair key is (the smaller half, the greater half).  Among pair units of equal key the
 *              highest score stays, a tie goes to the lowest pair index; both records of every other one get 0x400.
 *   end pass   every mapped record of a unit is an entry with key (5', strand), tagged paired or fragment.  A group of equal key
 *              that holds a paired entry: every fragment of it is a duplicate.  Otherwise the fragment of the highest score stays,
 *              a tie goes to the lowest record index.  Paired entries are never flagged here, nor is a fragment's unmapped mate.
 * bgsa_hip_dup_keys_dev: one WAVE per unit.  d_end_key int64[n]: half << 1 | tag (tag 1: fragment, so paired entries sort first),
 * INT64_MAX where the record is no entry.  Per unit (n / ends entries): d_score int32, d_pair_key_a / _b int64 — the two halves,
 * INT64_MAX where the unit is no pair unit.  d_counts int32[3], zeroed by the caller: += pair units, fragment units, malformed records.
 * bgsa_hip_dup_mark_dev: one THREAD per sorted entry.  ends 2, the pair pass: n / 2 entries, d_key_a / d_key_b the pair keys in
 * SORTED order, d_order[j] the unit at place j.  ends 1, the end pass (of a single-end AND of a paired batch): n entries, d_key_a
 * the end keys in sorted order, d_key_b not read (may be NULL), d_order[j] the record at place j.  The order the caller gives
 * (stable sorts, least significant first): key ascending, score descending, index ascending.  An entry whose key equals its
 * predecessor's — the tag left out — is a duplicate: with that order a fragment that does not head its group stands behind a paired
 * entry or a better fragment, so this one comparison is the whole rule.  Only tagged entries are flagged in the end pass.  Entries
 * of key INT64_MAX are none.  d_order[j] is compared with the entry count, the records with n, before d_flag is touched; every
 * record is written by at most one thread.  d_counts int32[3]: += duplicate pair units, duplicate fragment units, records flagged.
 * Both only launch on `stream`: no allocation, no synchronisation; n == 0 is BGSA_HIP_OK and launches nothing.  BGSA_HIP_EINVAL,
 * before the first HIP call: a NULL pointer (the stream, d_quals and the end pass's d_key_b excepted), n < 0, ends outside 1..2, an
 * odd n with ends 2, min_quality outside 0..93, ref_len beyond 2^60, what the SAM passes refuse about the batch.
 * LIMITS: duplicates are found within ONE call's records; no optical duplicates, UMIs or read groups; an unmapped mate is not flagged. */
int bgsa_hip_dup_keys_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int ends, int min_quality, int64_t *d_end_key, int32_t *d_score,
                          int64_t *d_pair_key_a, int64_t *d_pair_key_b, int32_t *d_counts, void *stream);
int bgsa_hip_dup_mark_dev(const int64_t *d_key_a, const int64_t *d_key_b, const int64_t *d_order, int64_t n, int ends, int32_t *d_flag,
                          int32_t *d_counts, void *stream);

/* ---- BAM records: merge — the records of MANY calls in one coordinate-sorted, indexed file ----
 * A call holds one working set of reads; a sequencing run is a thousand of them.  A merge keeps what every call emitted — the
 * record bytes in input order and the per-record arrays of "coordinate order and index" and "Duplicate marking" — on the device,
 * and when it is finished sorts ALL keys once, marks duplicates over ALL records once and moves the record bytes into coordinate
 * order with the one kernel below, segment by segment through the framing or deflate calls and then the index calls above
 * (bam_merge.hip; bgsa_amd/reference.py: BamMerge, sam_records(merge=...)).  The result is DEFINED as the one-call result: the
 * blocks, columns, index arrays and .bai bytes of one sort=True call on the concatenated reads (tests/bam_merge_reference.py).
 * That rests on five facts of the stages above:
 *   tie order    the sort is stable and the merge's input order is batch-major, so equal keys fall as in one call.
 *   keys         the sort key reads bit 16 of the flag only: keys computed before duplicate marking are the final keys.
 *   the flag     a BAM record holds its flag in exactly two bytes, offsets 18 and 19 from the start of its block_size field,
 *                little-endian; marking after the records were emitted changes those two bytes and nothing else (bin does not
 *                depend on the flag).
 *   deflate      a deflated block is a function of (its payload, block_payload) alone: segments of whole blocks give the bytes of
 *                one pass.
 *   duplicates   the duplicate rule's ties go to the lowest index; the global record or pair index is (batch order, index in batch).
 * bgsa_hip_bam_gather_dev: one WAVE per output record.  Output record i (0 <= i < n) is source record s = d_order[i], the bytes
 * d_src[d_src_offsets[s] .. d_src_offsets[s + 1]); in the sorted payload it occupies [d_dst_offsets[i], d_dst_offsets[i + 1])
 * (both offset arrays have one entry more than records: n_src + 1 and n + 1).  The call handles output records first ..
 * first + count - 1 and writes of each exactly the bytes whose sorted-payload position p lies in [window_lo, window_hi), to
 * d_out[p - window_lo]: d_out holds window_hi - window_lo bytes, and a record that straddles a window edge is finished by the call
 * of the next window.  d_flag not NULL (int32[n_src], indexed by s): the record's bytes 18 and 19 are d_flag[s] & 0xffff,
 * little-endian, instead of the source's; each of the two is written or not by the window rule on its own.
 * A record is REFUSED — it adds 1 to *d_refused (the caller zeroes it), not a byte of it is written and none of its values forms
 * an address — when s is outside [0, n_src); a source or destination offset pair is negative or not monotone; the source extent
 * leaves src_bytes; the two lengths differ; d_flag is given and the length is below 20.
 * The call only launches on `stream`: no allocation, no synchronisation; count == 0 or an empty window is BGSA_HIP_OK and launches
 * nothing.  BGSA_HIP_EINVAL, before the first HIP call: a NULL pointer (d_flag and the stream excepted), a negative count or size,
 * first + count > n, window_hi < window_lo, count beyond one launch (2^33).
 * LIMITS: the payload of all calls stays on the device (no host spill, no merge of files); BAM only; BAI only; no optical
 * duplicates or UMIs; one source buffer (no table of source pointers). */
int bgsa_hip_bam_gather_dev(const uint8_t *d_src, int64_t src_bytes, const int64_t *d_src_offsets, int64_t n_src, const int64_t *d_order,
                            const int64_t *d_dst_offsets, int64_t n, int64_t first, int64_t count, int64_t window_lo, int64_t window_hi,
                            const int32_t *d_flag, uint8_t *d_out, int32_t *d_refused, void *stream);

/* ---- Pileup: per-position base counts of the records, and the candidate sites of a count matrix ----
 * Coverage, a consensus and variant candidates all start from a pileup, and a pileup walks the CIGAR runs that already lie on the
 * device beside the reads, the qualities and the reference (bgsa_hip_sam_batch_t).  It is also the consumer that honours flag 1024
 * of "Duplicate marking".  bgsa_hip_pileup_dev adds one batch to a count matrix; the two site passes reduce the matrix on the
 * device to a list, as top_hits does for the score matrix, so the matrix (32 bytes per position) need not be copied
 * (pileup.hip; bgsa_amd/reference.py: Pileup, sam_records(pileup=...)).
 * THE COUNT MATRIX (public, fixed): d_counts is int32[ref_len][8], row p for LINEAR reference position p — the batch's ref_len, in
 * the one-sequence and in the contig form alike.  The caller zeroes it once; every call adds to it.
 *   columns 0..3   read base A, C, G, T              column 5   a SAM D run covers p
 *   column  4      any other read byte               column 6   a SAM I run lies between p and p + 1
 *   column  7      the share of columns 0..5 that comes from reverse-strand records
 * Depth beyond 2^31 - 1 is not supported.
 * DEFINITIONS (normative; tests/pileup_reference.py restates them).
 *   contributes  a record contributes iff it is well formed by the rules of "SAM records" (malformed, there), it is mapped,
 *              (flag & exclude_flags) == 0 and mapq >= min_mapq.  Coordinates are linear in both forms of the batch: one call
 *              serves both, d_rname and rname_len are not read.
 *   malformed  adds 1 to d_stats[2] and touches nothing else; none of its values forms an address.
 *   as written seq[j] and qual[j], j in [0, read_len), are the record as the SAM stage writes it: the caller's bytes for a forward
 *              hit; for a reverse hit the read reverse-complemented (A<->T, C<->G, anything else N) and QUAL reversed.
 *   the walk   from p = ref_begin, j = 0 over the runs:
 *              op 7 or 8, length len: for t in 0..len-1: if d_quals is not NULL and qual[j+t] - 33 < min_base_quality the base adds
 *                to d_stats[4] and to nothing else; otherwise counts[p+t][class(seq[j+t])] += 1 with class 0..3 for upper-case A, C,
 *                G, T and 4 for anything else, d_stats[3] += 1, and a reverse record also adds 1 to counts[p+t][7].  The column
 *                comes from the read byte, never from the op.  Then p and j advance by len.
 *              op 1 (reference only, SAM D): counts[p+t][5] += 1, a reverse record also counts[p+t][7] += 1; qualities are not
 *                consulted.  Then p advances by len.
 *              op 2 (read only, SAM I): if ref_begin < p < ref_end, counts[p-1][6] += 1, once per run whatever its length; a
 *                leading or trailing run is counted nowhere.  Then j advances by len.
 *   d_stats    int64[5], each call adds: [0] records used, [1] records filtered (unmapped, flag or MAPQ), [2] malformed records,
 *              [3] bases counted, [4] bases below the quality bound.
 * bgsa_hip_pileup_dev: one WAVE per record on a resident grid striding over the records, 64 runs at a time, a run of up to four
 * bases by its own lane and a longer one by the whole wave; integer atomics on d_counts, so the result is exact whatever the order;
 * the stats reduced per wave, then one atomic per counter and workgroup.  BGSA_HIP_EINVAL, before the first HIP call: a NULL
 * pointer (d_quals and the stream excepted), a negative n, min_mapq outside 0..255, min_base_quality outside 0..93, exclude_flags
 * outside 0..65535, what the SAM passes refuse about the batch (rname excepted).  n == 0 is BGSA_HIP_OK and launches nothing.
 * CANDIDATE SITES.  For position p: r = d_reference[p] (codes 0..4); cover = the sum of columns 0..5; the allele columns are
 * {0, 1, 2, 3, 5, 6} minus r; column a QUALIFIES when counts[p][a] >= min_alt and 100 * counts[p][a] >= min_percent * cover, in
 * 64-bit integers; p is a SITE when r < 4, cover >= min_cover and at least one allele qualifies.  Its alt is the qualifying column
 * of the highest count, ties going to the lowest column; alts_mask has bit a set for every qualifying column.
 * bgsa_hip_pileup_sites_count_dev: one THREAD per position, one workgroup per 256; d_block_sites int32[n_blocks] gets every
 * workgroup's number of sites, n_blocks = bgsa_hip_pileup_site_blocks(ref_len) (host only; 0 for ref_len < 1).  The caller takes an
 * exclusive scan of them into d_block_offsets int64[n_blocks], reads ONE scalar back — the total — and sizes the outputs.
 * bgsa_hip_pileup_sites_emit_dev repeats the test and writes the sites in ascending position, site k of workgroup b at
 * d_block_offsets[b] + k: d_pos int64, d_ref / d_alt / d_alts_mask uint8, d_alt_count / d_cover int32, n_sites entries each.  A
 * site whose slot lies outside [0, n_sites) is not written and adds 1 to *d_overflow (int32, zeroed by the caller).
 * Both only launch on `stream`.  BGSA_HIP_EINVAL, before the first HIP call: a NULL pointer (the stream excepted), ref_len < 1 or
 * beyond 2^39 - 256 (one launch), min_cover < 1, min_alt < 1, min_percent outside 0..100, an n_blocks that is not the one for
 * ref_len, a negative n_sites.
 * The C loop: zero d_counts and d_stats; bgsa_hip_pileup_dev per batch; count; scan; read the total; allocate; emit; read *d_overflow.
 * LIMITS: the mates of an overlapping pair are both counted; duplicates are only those marked within the call; no base-alignment
 * quality, no genotype likelihoods, no VCF; insertions are counted per run, not per inserted sequence. */
#define BGSA_HIP_PILEUP_COLUMNS 8
#define BGSA_HIP_PILEUP_STATS 5
int bgsa_hip_pileup_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int min_mapq, int min_base_quality, int exclude_flags, int32_t *d_counts,
                        int64_t *d_stats, void *stream);
int64_t bgsa_hip_pileup_site_blocks(int64_t ref_len);
int bgsa_hip_pileup_sites_count_dev(const int32_t *d_counts, const uint8_t *d_reference, int64_t ref_len, int min_cover, int min_alt,
                                    int min_percent, int32_t *d_block_sites, int64_t n_blocks, void *stream);
int bgsa_hip_pileup_sites_emit_dev(const int32_t *d_counts, const uint8_t *d_reference, int64_t ref_len, int min_cover, int min_alt,
                                   int min_percent, const int64_t *d_block_offsets, int64_t n_blocks, int64_t n_sites, int64_t *d_pos,
                                   uint8_t *d_ref, uint8_t *d_alt, uint8_t *d_alts_mask, int32_t *d_alt_count, int32_t *d_cover,
                                   int32_t *d_overflow, void *stream);

/* Stream faults. The kernels walk each query as a packed code stream (below) under a window budget; a
 * wave whose stream ends without an END token, or holds a byte that is no token, leaves its loop and
 * raises a bit in a sticky per-device word instead of storing a score.  A well-formed stream cannot do
 * either: a set bit means the stream bytes were damaged between the packer and the row loop, and the
 * scores of that call are not to be trusted.  bgsa_hip_stream_faults() returns the word of the current
 * device (0 = clean; call after synchronising the streams that scored) and optionally clears it; the
 * host-buffer seams check it after every call and fail loudly.
 * bgsa_hip_debug_inject_stream_fault(kind): tests only — the next scoring launch of this process has
 * its first stream overwritten with REFILL tokens (1) or with a byte that is no token (2). */
#define BGSA_HIP_FAULT_BUDGET 1
#define BGSA_HIP_FAULT_CODE 2
/* bgsa_hip_myers_align_pairs_dev / bgsa_hip_trace_pairs_dev: a pair this call owned named a query outside [0, n_queries); that pair was skipped (an
 * argument check inside the kernel, not a damaged stream — the other pairs of the call are good). */
#define BGSA_HIP_FAULT_PAIR 4
/* bgsa_hip_myers_align_pairs_banded_dev, bgsa_hip_myers_place_pairs_banded_dev: a traceback step left its block's window, or the
 * placement's certified distance differs from the located one (bug guards, see there). */
#define BGSA_HIP_FAULT_BAND 8
int bgsa_hip_stream_faults(int clear);
int bgsa_hip_debug_inject_stream_fault(int kind);

/* The sustained shader clock while other launches run (bench.py's `clock` object): n_probes one-wave workgroups
 * (8 cover the 8 XCDs) are started on a stream of the library's own and sleep, reading the shader-clock
 * and the constant reference-clock counters, until bgsa_hip_clock_probe_stop() or until max_ms have passed — they
 * never outlive that bound.  caller_stream = the stream whose kernels are to be observed: start() picks a stream of its own
 * on which the probes are SEEN to run beside that stream (HIP shares hardware queues between streams; probes on the caller's
 * queue would hold its kernels back), or fails with BGSA_HIP_EUNSUPPORTED.  stop() returns per probe the clock in MHz over its lifetime and the XCD it ran on, and
 * the longest probe lifetime in seconds.  Measurement only: nothing in the scoring path depends on it. */
int bgsa_hip_clock_probe_start(int n_probes, unsigned max_ms, void *caller_stream);
int bgsa_hip_clock_probe_stop(double *mhz, int *xcc, int cap, int *n_out, double *seconds);

/* Introspection (host only, no GPU): the packed code stream the kernels walk for one mapped query
 * row, 8-byte windows of 7 tokens + REFILL.  Myers / BitPAl: codes 0..4 = row of that character
 * class, 5 = END, 6 = REFILL; for BGSA_ALGO_MYERS, k = -1 selects the stream of the column-block
 * kernel (subjects > 1024 bp: a CARRY token, code 7, in front of every 32nd row) and k = -2 the
 * two-rows-per-token stream of the <= 64 bp kernels (codes as for banded below, without EVENT).
 * BGSA_ALGO_BANDED (threshold k): 0..24 = two rows of classes a, b as 5*a + b, 25..29 = one row,
 * 30 = END, 31 = REFILL, 63 = EVENT + argument byte (1 reset the error count, 2 advance the match
 * words, 4 test the limit, 8 latch the reject mask, 16 re-anchor the band (BGSA_BANDED_IMPL=p only), 32 cut the next
 * one-word window (the default kernels for k <= 12)).
 * Writes at most `cap` bytes to dst (may be NULL) and returns the stream length in bytes. */
int bgsa_hip_query_stream(int algo, const char *mapped_row, int ref_len, int k, unsigned char *dst, int cap);

/* The certified band of the Myers global kernels (subjects of 65..256 bp).  A row runs only on the words that
 * hold the diagonal band |d| + |d - (n - m)| <= B = 2h + 1 of a query of ref_len = m against subjects of read_len = n; a wave
 * with a score above B runs that query again with full rows, so the scores do not change.  h follows the lengths, or
 * BGSA_MYERS_BAND (0 = off, N = half-width).
 * bgsa_hip_myers_band_stream: the band stream of one mapped query row (host only, no GPU): the plain stream's codes plus
 * 7 = SETWIN + a window byte; writes at most `cap` bytes and returns its length, or 0 when the band is off for the shape.
 * bgsa_hip_myers_band_half: the half-width h a launch of these lengths uses (0: off).
 * bgsa_hip_myers_band_stats: the current device's counts since the last clear, in units of (64-subject group, query) whichever
 * kernel ran — out[0] = group-queries with a score above B (their wave ran the query again with full rows), out[1] =
 * group-queries run banded (call after synchronising).
 * bgsa_hip_myers_band_groups: the subject groups a wave carries (1 | 2) in a global launch of word_num-word subjects, this bucket
 * size and these lengths (mixed_lengths != 0: a bucket with per-subject lengths) — 2 only where the band applies, word_num <= 5
 * and the bucket is large, or BGSA_MYERS_BAND_GROUPS=1|2 forces it (host only, no GPU).  bgsa_hip_kernel_name names the
 * one-group kernel, the small bucket's.
 * bgsa_hip_myers_prefix_depths: prefix sharing of the band kernels — a wave walks its tile of queries in sorted order and
 * resumes each behind the rows it shares with its predecessor, from snapshots at a few fixed depths.  Writes the depths
 * such a launch of n_queries queries would use to depths[0 .. cap) and returns their number, 0 where the launch does not
 * share.  It launches nothing; the query tile it assumes depends on the device's CU count, which it asks the runtime for once
 * (256 where there is no device).  BGSA_MYERS_PREFIX_SHARE (read once): 0 = off, 1 = on, a list of one to five ascending
 * depths in 1 .. 10 (a,b,c; a single number from 2 up is a list of one) = these depths whatever the query count.  A list that
 * is longer, out of order, out of range or reaches rows beyond the first two words turns sharing off: the answer is then 0.
 * bgsa_hip_myers_band_segments: the stream of one mapped query row cut at these depths, as a sharing launch packs it — one
 * band stream per segment, each beginning with its SETWIN; offsets[0 .. n_depths + 1] = where each begins, and the length.
 * Returns the length (<= cap bytes written), or 0 when the shape does not qualify (host only, no GPU).
 * Rescue: a launch with two groups per wave on a large bucket runs a band three narrower (bgsa_hip_myers_band_rescue_half:
 * 150 bp -> h = 45) and scores its few uncertified lanes — up to eight per group and query — again one by one in a kernel of
 * its own instead of sending their waves through the full rows; the scores do not change.  The workspace of plans with
 * read_len 65..160 carries its pool (32 KiB per query, 512 MiB at the most).  BGSA_MYERS_BAND_RESCUE=0|1 (read once) forces it
 * off or on for every two-group banded launch; BGSA_MYERS_BAND_RESCUE_POOL=N caps the pool's entries (tests).
 * bgsa_hip_myers_band_rescue: the half-width such a launch of n_queries queries against read_count subjects would use, 0
 * where it does not rescue — by default fewer than 1,000 queries, a small bucket, lengths outside the rule (host only, no GPU).
 * bgsa_hip_myers_band_rescue_stats: the current device's counts since the last clear — out[0] = lanes rescued, out[1] =
 * group-queries a rescuing wave ran again with full rows because a group held more than eight uncertified lanes or the pool
 * was full (they are among out[0] of bgsa_hip_myers_band_stats too; call after synchronising).
 * bgsa_hip_myers_band_rescue_half: FOR TESTS — the half-width formula alone, whatever the launch (the library's side of
 * rows_ir.py: myers_band_rescue_half); a caller asks bgsa_hip_myers_band_rescue.
 * Early leave: a launch that rescues by the default rule, n = m, lets low words of the window leave before the static band
 * does — behind a CUT row r the window begins at word w + 1 — and certifies each lane against min(B, D'[r][j_r] + r - j_r),
 * j_r = 32 (w + 1), instead of B; the lanes above it join the rescue's, and the scores do not change.  The cut rows are a table
 * by length (150 bp: behind rows 106 and 130, words 1 and 2).  BGSA_MYERS_BAND_EARLY=0|1 (read once) forces it off, or on for
 * every rescuing launch whose length has cuts (BGSA_MYERS_BAND_RESCUE=1 alone leaves it off).
 * bgsa_hip_myers_band_early: the cuts such a launch would run with — their number (0: none), rows_out[0 .. n) = the cut rows
 * (host only, no GPU).
 * bgsa_hip_myers_band_early_cuts: the table's entry for subjects and queries of `len` at half-width h: rows[j], words[j], and
 * their number.
 * bgsa_hip_myers_band_early_segments: the stream of a len x len launch at half-width h with these cuts, as such a launch packs it:
 * the windows are the schedule's with the cuts applied, everything else is bgsa_hip_myers_band_stream's (n_depths = 0, offsets[0 .. 1])
 * or bgsa_hip_myers_band_segments' (n_depths >= 1 sharing depths, offsets[0 .. n_depths + 1]).  0 where the cuts are no schedule. */
int bgsa_hip_myers_band_early(int ref_len, int read_len, int n_queries, int64_t read_count, int *rows_out);
int bgsa_hip_myers_band_early_cuts(int len, int h, int *rows, int *words);
int bgsa_hip_myers_band_early_segments(const char *mapped_row, int len, int h, const int *cut_rows, const int *cut_words, int n_cuts,
                                       const int *depths, int n_depths, unsigned char *dst, int cap, int *offsets);
int bgsa_hip_myers_band_rescue_half(int len);
int bgsa_hip_myers_band_rescue(int ref_len, int read_len, int n_queries, int64_t read_count);
int bgsa_hip_myers_band_rescue_stats(unsigned long long *out, int clear);
int bgsa_hip_myers_prefix_depths(int word_num, int64_t read_count, int ref_len, int read_len, int n_queries, int mixed_lengths,
                                 int *depths, int cap);
int bgsa_hip_myers_band_segments(const char *mapped_row, int ref_len, int read_len, const int *depths, int n_depths,
                                 unsigned char *dst, int cap, int *offsets);
int bgsa_hip_myers_band_stream(const char *mapped_row, int ref_len, int read_len, unsigned char *dst, int cap);
int bgsa_hip_myers_band_half(int ref_len, int read_len);
int bgsa_hip_myers_band_groups(int word_num, int64_t read_count, int ref_len, int read_len, int mixed_lengths);
int bgsa_hip_myers_band_stats(unsigned long long *out, int clear);

/* Queries a wave scores per load of its subject block in this thread's last scoring launch (0: none yet).  The launch's
 * HBM traffic follows from it: ceil(queries / tile) x block bytes + the scores (bench.py: traffic_model). */
int bgsa_hip_last_query_tile(void);

/* Name of the kernel the previous call would launch for these shapes (for profiles/bench). */
const char *bgsa_hip_kernel_name(int algo, int word_num);

#ifdef __cplusplus
}
#endif
#endif /* BGSA_HIP_H */

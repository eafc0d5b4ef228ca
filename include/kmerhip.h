/*
 * kmerhip.h -- C ABI of the MI355X-native canonical k-mer counter.
 *
 * This is the drop-in boundary for krust's counting hot path.  The reference
 * (Rust crate `kmerust` 0.3.1) has no FFI of its own; the seam these entry
 * points replace is the internal call
 *
 *     KmerMap::new().build(seqs, k)                     src/run.rs:494-503
 *     KmerMap::new().build_with_quality(seqs, k, minq)  src/run.rs:505-520
 *     KmerMap::into_hashmap(k)                          src/run.rs:573-582
 *
 * and its public packed twin
 *
 *     count_kmers_from_sequences(iter<Bytes>, KmerLength) -> HashMap<u64,u64>
 *                                                       src/streaming.rs:198-204
 *
 * INTEGRATION.md shows the Rust `extern "C"` binding a krust maintainer would
 * add at those call sites.  Plain pointers and sizes only; no C++ or torch
 * types cross this boundary; no exception crosses it.
 *
 * Semantics (bit-exact with the reference):
 *   - k-mer = k consecutive bytes all in ACGTacgt (src/kmer.rs:266-286), 2-bit
 *     packed A=0 C=1 G=2 T=3, first base most significant (kmer.rs:21-32,467-471)
 *   - canonical = lexicographic min of k-mer and reverse complement
 *     (kmer.rs:348-390) == integer min of the packed forms
 *   - optional quality mask: a window is skipped iff any of its k quality bytes
 *     is < min_quality.saturating_add(33)          (run.rs:538,543-548)
 *   - k-mers never span records; in a flat buffer records are separated by at
 *     least one byte outside ACGTacgt (e.g. '\n'), which no window may contain
 *   - count[key] += 1 per window, u64 counts          (run.rs:565-571)
 *
 * Threading: one producer thread per context (not re-entrant); independent
 * contexts may be used concurrently.  All functions return KH_OK (0) or a
 * negative kh_status; k-mers are never dropped silently.
 */
#ifndef KMERHIP_H
#define KMERHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: these declarations -- and nothing else -- are what it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define KMERHIP_ABI_VERSION 2

typedef enum kh_status {
    KH_OK = 0,
    KH_ERR_BAD_K = -1,      /* KmerLengthError, src/kmer.rs:100-110, src/error.rs:86-95 */
    KH_ERR_BAD_ARG = -2,
    KH_ERR_NO_DEVICE = -3,  /* no HIP device / HIP runtime unusable */
    KH_ERR_OOM = -4,        /* device or pinned-host allocation failed */
    KH_ERR_TABLE_FULL = -5, /* table cannot grow further */
    KH_ERR_HIP = -6,        /* a HIP call failed; kh_last_error() has the text */
    KH_ERR_STATE = -7,      /* call not valid in the context's current state */
    KH_ERR_RANGE = -8,      /* caller-provided output array too small */
    KH_ERR_FORMAT = -9,     /* kh_push_text*: a record layout the device scanner does not take
                               (nothing was counted; parse on the host and use kh_push) */
    KH_ERR_RCCL = -10,      /* an RCCL call failed or timed out (kh_comm_init / kh_merge_across); kh_last_error() has the text */
    KH_ERR_PEER = -11       /* kh_merge_across: ANOTHER rank of the collective failed (its own status says why;
                               kh_last_error() names the rank); every rank leaves the merge together */
} kh_status;

/* Allocation failures: what KH_ERR_OOM leaves behind.  One rule per kind of call; the comments further down only add to it.
 *   - A READING call takes the table as it is and allocates only for itself: kh_result_size / _copy / _copy_device / _sorted*,
 *     kh_result_text_*, kh_histogram, kh_lookup, kh_profile*, kh_profile_records*, kh_compare, kh_graph_*, kh_unitigs_*,
 *     kh_unitigs_text_begin / kh_unitigs_text_next / kh_unitigs_text_next_device, kh_unitigs_paths / kh_unitigs_paths_device, kh_unitigs_link_support / kh_unitigs_link_support_device, kh_unitigs_components / kh_unitigs_components_device and the src side of kh_clip_tips_into / kh_pop_bubbles_into / kh_drop_components_into.  When one of its allocations fails it returns KH_ERR_OOM, kh_last_error() names the
 *     allocation, the table is unchanged and the context is NOT poisoned: the same call can be made again.  What the call
 *     allocated is released, except the scratch the context keeps for the next such call where that had been allocated
 *     before the failure: the pinned staging chunks and the copy stream of the host forms, the scan scratch (not after the
 *     sorted results, kh_unitigs_begin*, kh_unitigs_components*, kh_clip_tips_into, kh_pop_bubbles_into and kh_drop_components_into: there nothing stays), the tile arrays of a text stream (a failure of kh_unitigs_text_begin / kh_unitigs_text_next /
 *     kh_unitigs_text_next_device ends that stream and releases its offsets and chunks; the unitigs stay live), the
 *     chunk and row buffers of kh_profile / kh_profile_records, the words of kh_compare and kh_graph_stats.  kh_destroy
 *     releases them.  (Pushes that were still pending when the reading call came are counted first, as a writing call.)
 *   - A WRITING call changes the table: the pushes and the counting they trigger (also when a later call counts them), growth,
 *     the widening of the 8-byte image, kh_merge_*, and the dst of kh_combine_into / kh_clip_tips_into / kh_pop_bubbles_into.  When one of its
 *     allocations fails it returns KH_ERR_OOM, the table's content is unspecified and the context is POISONED: every later
 *     call except kh_reset, kh_destroy and kh_last_error returns KH_ERR_STATE.  A failure that the call can work round is
 *     no failure: a smaller text buffer, the 16-byte table instead of its 8-byte image, the partition buffers given back for
 *     an exchange's scratch, the exchange's own digests instead of the kernels' -- KH_OK, and the counts are exact.
 *     (One exception, kh_merge_across: scratch of the exchange that does not fit even then is KH_ERR_OOM WITHOUT poisoning;
 *     the table's content is unspecified until kh_reset all the same, as after any failed merge.)
 *     The exports (kh_export_*_device, kh_region_unit_counts_device) and kh_set_shard follow this rule too: they enter the context
 *     as a writing call does (pending pushes are counted, most of them widen the 8-byte image), and their own scratch is the
 *     context's -- KH_ERR_OOM poisons, the table itself is intact, kh_reset starts over.
 *   - kh_reset ends a poisoning by KH_ERR_OOM or KH_ERR_TABLE_FULL and leaves an empty, fully usable context.  A poisoning by
 *     KH_ERR_HIP stays (KH_ERR_STATE): nothing is known about the device; kh_destroy is what is left.
 *   - kh_create that fails returns KH_ERR_OOM with *out NULL and nothing left allocated. */

typedef struct kh_ctx kh_ctx;

/* Counter configuration.  Mirrors what the reference passes across its seam:
 * k (run.rs:500), min_quality: Option<u8> (run.rs:509). */
typedef struct kh_config {
    uint32_t struct_size;    /* sizeof(kh_config), for ABI evolution */
    uint32_t k;              /* 1..32 */
    int32_t  min_quality;    /* -1 = None; 0..255 = Some(q) (Phred, +33 applied inside) */
    int32_t  device;         /* HIP device ordinal; -1 = current device */
    uint64_t capacity_hint;  /* expected number of DISTINCT canonical k-mers; 0 = grow on demand */
    void    *stream;         /* hipStream_t to launch on.  NULL = the context creates its own NON-BLOCKING stream
                                (not ordered with the legacy default stream: synchronise buffers handed to
                                kh_push_device yourself) -- unless KH_FLAG_CALLER_STREAM says that NULL means
                                the legacy default stream itself (what torch.cuda.current_stream() usually is) */
    uint32_t flags;          /* KH_FLAG_* */
    uint32_t input_mib;      /* expected total input of this context in MiB (the size of the file about to be pushed), 0 = unknown.
                                Never needed: it lets kh_push_text size its device-side accumulation for THIS input instead
                                of for an eighth of the free memory (a small file then costs a small allocation) */
} kh_config;

#define KH_FLAG_TRACE 1u           /* print phase timings to stderr (also env KMERHIP_TRACE=1) */
#define KH_FLAG_FORCE_DIRECT 2u    /* always use the direct (device-scope atomic) insert path */
#define KH_FLAG_FORCE_PARTITION 4u /* always use the partitioned (LDS region rebuild) path;
                                      default: chosen per push from batch and table size
                                      (env KMERHIP_PATH=direct|partition overrides) */
#define KH_FLAG_CALLER_STREAM 8u   /* launch on cfg->stream even when it is NULL (= the legacy default stream) */
#define KH_FLAG_DEFER_TEXT_SCAN 16u /* kh_push_text returns when its text is on the device; the record scan -- and with it a
                                      KH_ERR_FORMAT refusal -- happens during the NEXT call that enters the context (the next
                                      kh_push_text scans it beside its own transfer; kh_finish at the latest).  A refusal then
                                      concerns the PREVIOUS text (the current one is dropped with it): for callers that restart
                                      the whole input on KH_ERR_FORMAT, as the kmerust command line does */

/* indices into kh_stats.stage_ms */
#define KH_NUM_STAGES 8
#define KH_STAGE_DIRECT 0      /* count_direct_kernel (the device-atomic path) */
#define KH_STAGE_P1_COUNT 1    /* (no longer used: level 1 is a single pass; always 0) */
#define KH_STAGE_P1_SCATTER 2  /* level 1: part1_bins_kernel (4-byte payloads, k <= 21 at >= 1024 regions) /
                                  part1_bins64_kernel (8-byte payloads) */
#define KH_STAGE_P2_COUNT 3    /* level 2, exact path only: part2_count_kernel (0 = the batch took the arena path) */
#define KH_STAGE_P2_SCATTER 4  /* level 2: part2_arena_kernel, or part2_scatter_lines_kernel (+ part2_scatter_kernel) on the exact path */
#define KH_STAGE_REGION 5      /* region_count_kernel32 / region_count_kernel64 (+ shard_merge_kernel in a merge) */
#define KH_STAGE_MISC 6        /* scans, plans, chunk lists, bounds, memsets, region_reduce, ovf_insert */
#define KH_STAGE_GROW 7        /* table growth / rehash */

typedef struct kh_stats {
    uint64_t bases;          /* bytes pushed (incl. separators) */
    uint64_t kmers;          /* valid windows counted == sum of all counts */
    uint64_t distinct;       /* live table entries */
    uint64_t table_slots;    /* current table capacity (16-byte slots) */
    uint64_t grows;          /* number of table rehashes */
    uint64_t launches;       /* count-kernel launches */
    double   count_kernel_ms;/* sum of all counting-kernel durations (HIP events on the launch stream) */
    double   h2d_ms;         /* host->device staging time for kh_push */
    uint64_t part_batches;   /* batches that went through the partitioned path */
    double   stage_ms[KH_NUM_STAGES]; /* per-stage kernel time, see KH_STAGE_* */
    double   text_scan_ms;   /* kh_push_text*: record-scanning kernels (not part of count_kernel_ms) */
    uint64_t slot_bytes;     /* ABI 2: bytes per slot of the form the counts live in right now -- 16: {u64 key, u64 count};
                              * 8: the image a partitioned count, or a fresh merge of packed / heads units, leaves (count << 32 |
                              * 32 hash bits); what reads results takes either, everything else converts first */
} kh_stats;

/* ---- lifecycle ---------------------------------------------------------- */
int  kh_create(kh_ctx **out, const kh_config *cfg);
void kh_destroy(kh_ctx *ctx);
/* Forget all counts, keep the table allocation (KmerMap::new() again). */
int  kh_reset(kh_ctx *ctx);

/* ---- input: replaces KmerMap::build / build_with_quality ---------------- */
/* Host buffers.  `bases` is a flat byte buffer of n bytes holding any number
 * of records separated by >=1 non-ACGTacgt byte; `qual` is NULL or a parallel
 * buffer of n bytes (same offsets).  With qual==NULL or min_quality==-1 no
 * quality masking happens (run.rs:543: both must be Some).  A quality byte of
 * 0xFF can never mask (the threshold is min_quality.saturating_add(33) <= 255
 * and a base is masked iff its byte is BELOW it): it is the filler for records
 * without qualities (FASTA) pushed beside FASTQ ones in one flat buffer --
 * any smaller filler ('~' = 126) would drop those records' windows once
 * min_quality >= 94.  Returns after the buffers have been consumed (caller may
 * reuse them). */
int kh_push(kh_ctx *ctx, const uint8_t *bases, const uint8_t *qual, uint64_t n);
/* Same, for buffers already resident in this device's HBM (no copy). */
int kh_push_device(kh_ctx *ctx, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n);
/* Raw FASTA / FASTQ TEXT, scanned on the device: replaces the record readers in front of the
 * path (SeqReader, src/reader.rs:58-79; the needletail / rust-bio loops of src/streaming.rs:858-893)
 * for uncompressed input.  `text` holds WHOLE records: it starts at a record header and ends at a
 * record end (a missing final newline is fine).  FASTA: wrapped records are joined, k-mers never
 * span records.  FASTQ: 4-line records only; qualities are used iff the context has a min_quality.
 * Returns KH_ERR_FORMAT -- with nothing counted -- for anything else (wrapped FASTQ, blank lines
 * between FASTQ records, a missing '@' / '+' / '>' marker, |seq| != |qual|, blanks at line ends of
 * a FASTA record): the caller then parses that text itself and uses kh_push.
 * kh_push_text returns when `text` has been copied and scanned (the caller may reuse it; a refusal is always about
 * THIS call's text -- unless the context was created with KH_FLAG_DEFER_TEXT_SCAN).  The scanned, flat form of the texts
 * ACCUMULATES on the device (up to an eighth of the free memory, or kh_config.input_mib) and is counted when that is
 * full or when anything looks at the table (kh_finish, kh_result_*, kh_lookup, kh_push_device ...): a file streamed in
 * chunks is counted in one or a few large batches.  So an error of the counting itself (KH_ERR_OOM, KH_ERR_TABLE_FULL:
 * errors that poison the context) can surface in a later call, at the latest in kh_finish.
 * kh_push_text_device: d_text must be 16-byte aligned. */
#define KH_TEXT_FASTA 1
#define KH_TEXT_FASTQ 2
int kh_push_text(kh_ctx *ctx, const uint8_t *text, uint64_t n, int format);
int kh_push_text_device(kh_ctx *ctx, const uint8_t *d_text, uint64_t n, int format);
/* Wait for all pushed work; fill stats (may be NULL). */
int kh_finish(kh_ctx *ctx, kh_stats *stats);

/* ---- host memory the device reaches directly ---------------------------- */
/* kh_push / kh_push_text stage PAGEABLE caller memory through pinned chunks (a multi-threaded memcpy: ~20-30 GB/s, below
 * PCIe's ~57) and kh_result_copy bounces the other way (plus the first-touch page faults of a fresh array).  Buffers
 * from kh_host_alloc (pinned, any device of the process), or the caller's own memory after kh_host_register, skip both:
 * the copy engine reads / writes them itself.  Detected per call (hipPointerGetAttributes): nothing else changes, and
 * kh_push still returns only when the buffers may be reused.  The reference reads a whole file into Vec<Bytes> before
 * counting (src/reader.rs:58-79); a Rust host would read() into such a buffer instead. */
int kh_host_alloc(void **out, uint64_t bytes);
int kh_host_free(void *p);
int kh_host_register(void *p, uint64_t bytes);
int kh_host_unregister(void *p);

/* ---- output: replaces KmerMap::into_hashmap ----------------------------- */
/* Number of distinct canonical k-mers with count >= min_count
 * (min_count filter of output_counts, run.rs:447-450). */
int kh_result_size(kh_ctx *ctx, uint64_t min_count, uint64_t *n);
/* Copy (packed canonical key, count) pairs with count >= min_count into
 * caller arrays of capacity cap; order unspecified (HashMap iteration order is
 * unspecified in the reference too).  *n receives the number written.
 *   - A cap smaller than kh_result_size(min_count): KH_ERR_RANGE, *n = 0 and NOTHING is written to keys / counts (the
 *     size is taken first); the context stays usable.  min_count = 0 selects what 1 selects.  cap = 0 takes NULL arrays. */
int kh_result_copy(kh_ctx *ctx, uint64_t *keys, uint64_t *counts, uint64_t cap,
                   uint64_t min_count, uint64_t *n);
/* Same into device arrays (for the multi-GPU exchange and device consumers).
 *   - A cap smaller than the number of pairs: KH_ERR_RANGE, *n = cap, and exactly cap pairs ARE written -- distinct pairs
 *     of the result with their counts, which ones is unspecified -- and nothing at or behind d_keys[cap] / d_counts[cap];
 *     the context stays usable.  (One pass over the table: the size is known only when the pairs are out.) */
int kh_result_copy_device(kh_ctx *ctx, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap,
                          uint64_t min_count, uint64_t *n);
/* The same pairs in ASCENDING order of the packed key -- which is lexicographic order of the k-mer strings (A < C < G < T, first
 * base most significant) -- sorted on the device: an LSD radix sort over the 2k significant key bits.  The order does not
 * depend on the table's size, geometry or form (16-byte table / 8-byte image: both are read as they are, kh_stats.slot_bytes,
 * distinct, kmers and grows stay what they were), so two runs over the same input give the same arrays.  A shard table
 * (kh_set_shard, or after kh_merge_across) gives its own keys in ascending order.
 *   - BOTH forms take the size first: a cap smaller than kh_result_size(min_count) is KH_ERR_RANGE with *n = 0 and NOTHING
 *     written to either array (kh_result_copy's rule, not kh_result_copy_device's); the context stays usable.
 *   - min_count = 0 selects what 1 selects.  cap = 0 takes NULL arrays.
 *   - Scratch (a second pair of arrays and the digit histograms) comes from the idle partition buffers, else from the device;
 *     KH_ERR_OOM when there is none -- the context stays usable and nothing stays allocated.
 *   - Like kh_result_copy they end a running kh_result_text_* stream (they take the same scratch memory). */
int kh_result_sorted_device(kh_ctx *ctx, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap,
                            uint64_t min_count, uint64_t *n);
int kh_result_sorted(kh_ctx *ctx, uint64_t *keys, uint64_t *counts, uint64_t cap,
                     uint64_t min_count, uint64_t *n);
/* The same result as TEXT, formatted on the device: replaces output_counts (src/run.rs:441-486) -- unpacking, the decimal
 * counts and the framing happen in HBM, and only text crosses the link.  Three formats, byte for byte the reference's:
 *   KH_OUT_FASTA  >{count}\n{kmer}\n          KH_OUT_TSV  {kmer}\t{count}\n
 *   KH_OUT_JSON   serde_json's pretty form of [{"kmer": .., "count": ..}, ..]: the COMPLETE document, brackets included
 *                 ("[]\n" when there is no record)
 * A pull interface, because the text can be larger than any one buffer: kh_result_text_begin sizes the stream
 * (*n_records, *n_bytes: its totals, either may be NULL), every kh_result_text_next* hands out the next piece --
 * WHOLE records, at most cap bytes -- and *n = 0 with KH_OK says that the stream has ended.
 *   - Records come in table-slot order (ascending key order with KH_OUT_SORTED); the same table gives the same bytes on every run, and the concatenation of the
 *     pieces is the same document for EVERY sequence of cap values.
 *   - JSON: the opening "[\n" belongs to the first record; the closing "\n]\n" follows the last record in the same piece
 *     when it fits there, else it is a piece of its own.
 *   - A cap smaller than the next record: KH_ERR_RANGE, nothing is consumed (call again with more room).
 *   - next without begin: KH_ERR_STATE.  So is next after any call that entered the context for something else than
 *     reading -- every kh_push*, kh_reset, kh_merge_*, kh_set_shard, the exports, kh_result_copy / kh_result_sorted* (which take the
 *     same scratch memory): begin again.  kh_result_size, kh_lookup, kh_histogram and kh_finish may be interleaved.
 *   - begin on a running stream restarts it.  Shard tables (kh_set_shard / kh_merge_across) stream like full ones.
 *   - kh_result_text_next takes pageable memory, or -- faster: no bounce -- memory of kh_host_alloc / kh_host_register;
 *     the next range of the table is formatted while the current one travels.  kh_result_text_next_device writes
 *     device memory of this context's device (any alignment) and returns when it is complete.
 *   - Give cap room: the device formats up to 64 MiB at a time, and a call whose cap ends inside such a chunk finds the
 *     last record end with a small blocking read from the device -- correct for any cap, but a cap of a few records
 *     costs a device round trip per call.  Pieces of 1 MiB and more run at the link's rate. */
#define KH_OUT_FASTA 1
#define KH_OUT_TSV 2
#define KH_OUT_JSON 3
/* ORed into `format` of kh_result_text_begin: the records come in ASCENDING KEY order (the k-mer strings in lexicographic order)
 * instead of table-slot order.  begin sorts the result on the device (kh_result_sorted_device) into memory the stream owns --
 * 16 bytes per record, released by kh_destroy; KH_ERR_OOM when it cannot be had -- and everything else of the stream's contract
 * is unchanged: totals, whole records per piece, the same document for every sequence of cap values, JSON framing, the
 * KH_ERR_RANGE / KH_ERR_STATE rules, interleaved readers, next_device.  On top of it the same table CONTENT gives the same
 * bytes whatever the table's size, geometry or form.  Any other bit beside the three formats: KH_ERR_BAD_ARG. */
#define KH_OUT_SORTED 0x100u
int kh_result_text_begin(kh_ctx *ctx, uint32_t format, uint64_t min_count, uint64_t *n_records, uint64_t *n_bytes);
int kh_result_text_next(kh_ctx *ctx, uint8_t *buf, uint64_t cap, uint64_t *n);
int kh_result_text_next_device(kh_ctx *ctx, uint8_t *d_buf, uint64_t cap, uint64_t *n);
/* Count-of-counts after the min_count filter, ascending by count
 * (compute_histogram, src/histogram.rs:88-94 as used by run.rs:471-481).  *n receives the number of lines written.
 *   - A cap smaller than the number of lines: KH_ERR_RANGE, *n = cap, and count / freq hold the FIRST cap lines (the
 *     ascending prefix of the whole histogram), nothing at or behind entry cap; the context stays usable -- call again
 *     with more room (the number of lines is not reported: grow cap until KH_OK).  cap = 0 takes NULL arrays. */
int kh_histogram(kh_ctx *ctx, uint64_t min_count, uint64_t *count, uint64_t *freq,
                 uint64_t cap, uint64_t *n);
/* counts[i] = count of packed canonical key keys[i], 0 if absent
 * (`kmerust query`, src/main.rs:264-280). */
int kh_lookup(kh_ctx *ctx, const uint64_t *keys, uint64_t n, uint64_t *counts);
/* Per-base abundance of new sequences against the table: out[i] = the table's count of the canonical k-mer of bytes
 * i .. i+k-1, for every i < n (what `jellyfish query -s` / `kmc_tools filter` ask of a k-mer database, per read).
 * INPUT as kh_push / kh_push_device: a flat buffer, records separated by >= 1 byte outside ACGTacgt, an optional parallel
 * quality buffer that masks iff it is given AND the context has a min_quality (0xFF is the filler that never masks).
 * OUTPUT: n entries, indexed by the window START, every one of them written:
 *   - the count, saturated at 0xFFFFFFFE;  0 = a valid window whose k-mer the table does not hold
 *   - KH_PROFILE_NO_WINDOW where counting would see no window at i: a byte outside ACGTacgt or a quality byte below the
 *     threshold among the k, or i > n - k (the last k-1 entries; all of them when n < k)
 * n == 0 is KH_OK.  Both calls only READ, like kh_lookup: pushes still pending are counted first, the table is read in the
 * form it is in (kh_stats.slot_bytes stays what it was), no count changes, a kh_result_text_* stream in progress goes on,
 * and a bad argument (NULL with n > 0, an out that is not 4-byte aligned: KH_ERR_BAD_ARG) leaves the context usable.
 * SHARDS (kh_set_shard, or after kh_merge_across): a valid window whose k-mer ANOTHER shard owns reads 0 here, so the
 * element-wise sum over the ranks' profiles of the same sequences -- at the positions that are not KH_PROFILE_NO_WINDOW,
 * which are the same on every rank -- is the profile against the full table.
 * kh_profile_device: buffers in this device's memory (d_bases / d_qual at any alignment); returns when d_out is complete.
 * kh_profile: host memory, pageable or -- no bounce -- of kh_host_alloc / kh_host_register; streamed in chunks through
 * pinned staging of the context (released by kh_destroy), transfers of one chunk beside the kernel of the next. */
#define KH_PROFILE_NO_WINDOW 0xFFFFFFFFu
int kh_profile_device(kh_ctx *ctx, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, uint32_t *d_out);
int kh_profile(kh_ctx *ctx, const uint8_t *bases, const uint8_t *qual, uint64_t n, uint32_t *out);
/* The same profile reduced per record ON THE DEVICE: one row of KH_REC_WORDS uint32 words per record instead of one word per base
 * (what `kmerust query --sequences -f summary` prints and `kmerust filter` decides by) -- 32 bytes per record cross the link.
 * Let P[0..n) be what kh_profile* writes for the same bases, qual, n and context.  rec_start has nrec + 1 ASCENDING entries with
 * rec_start[nrec] <= n; record r owns the window starts rec_start[r] <= i < rec_start[r+1], and row r (words r*8 .. r*8+7 of
 * rows) is the reduction below over P[i] for those i, skipping KH_PROFILE_NO_WINDOW.  Every row is written; an empty record, or
 * one without a window, gives {0,0,0,0,0,0,0,0xFFFFFFFF}.  Segments need not coincide with separators: a caller whose records
 * are '\n'-separated passes the record start bytes and n (a window that would reach over a separator is no window anyway).
 * The counts are kh_profile's saturated ones (<= 0xFFFFFFFE), their sum is exact in 64 bits; lo > hi gives in_range == 0,
 * lo == 0 gives first_low == 0xFFFFFFFF.
 * Otherwise the contract of kh_profile: read-only, pending pushes are counted first, kh_stats.slot_bytes stays, a kh_result_text_*
 * stream goes on, both table forms and shard tables are read as they are.  SHARDS: a window whose k-mer another shard owns reads 0,
 * so `windows` is equal on every rank and `present` and `sum` ADD UP over the ranks to the full table's; min, max, in_range and
 * first_low do NOT combine over ranks (a foreign key's 0 takes part in them).
 * nrec == 0 is KH_OK and writes nothing; n == 0 writes nrec empty rows.  KH_ERR_BAD_ARG, the context usable afterwards: NULL with
 * n or nrec > 0, rows not 4-byte aligned (rec_start not 8-byte aligned), and in the host form rec_start not ascending,
 * rec_start[nrec] > n, or a record of 2^32 or more window starts.  For kh_profile_records_device those three are the caller's
 * contract: the offsets are not read back to check them (offsets that break it give unspecified rows, nothing else).
 * kh_profile_records streams the bases in chunks like kh_profile (same staging, released by kh_destroy); the rows stay on the
 * device for the whole call and come back once at the end, rec_start goes up once. */
#define KH_REC_WORDS 8        /* uint32 words per record row */
#define KH_REC_WINDOWS 0      /* entries of the record that are a window (not KH_PROFILE_NO_WINDOW) */
#define KH_REC_PRESENT 1      /* windows whose count is > 0 */
#define KH_REC_IN_RANGE 2     /* windows with lo <= count <= hi */
#define KH_REC_MIN 3          /* min / max over the windows; 0 when there is none */
#define KH_REC_MAX 4
#define KH_REC_SUM_LO 5       /* sum of the (saturated) counts as u64: low, high word */
#define KH_REC_SUM_HI 6
#define KH_REC_FIRST_LOW 7    /* offset from the record start of the first window whose count is < lo; 0xFFFFFFFF: none */
int kh_profile_records_device(kh_ctx *ctx, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, const uint64_t *d_rec_start,
                              uint64_t nrec, uint32_t lo, uint32_t hi, uint32_t *d_rows);
int kh_profile_records(kh_ctx *ctx, const uint8_t *bases, const uint8_t *qual, uint64_t n, const uint64_t *rec_start,
                       uint64_t nrec, uint32_t lo, uint32_t hi, uint32_t *rows);

/* ---- two tables against each other (no reference counterpart) ------------- */
/* What `kmc_tools simple` and Jaccard / containment screens ask of two k-mer databases, answered where both tables are: one
 * is scanned slot by slot, the other probed per live slot -- no pair crosses the link.
 * SETS: a key is in set A iff its count in `a` is at least max(min_a, 1); otherwise it counts as absent there, with ca = 0.
 * Set B the same with min_b.  ca / cb below: the key's count in a / b, 0 where it is not in the set.
 * kh_compare fills KH_CMP_WORDS words of host memory (the KH_CMP_* indices).  Derived measures are the caller's arithmetic:
 *   Jaccard = shared / (distinct_a + distinct_b - shared);   containment of a in b = shared / distinct_a;
 *   Bray-Curtis dissimilarity = 1 - 2 sum_min / (sum_a + sum_b).
 * kh_combine_into adds the result pairs of a set operation to `dst` as kh_merge_pairs_device would -- count[key] += c; dst
 * need not be empty -- and *n_pairs receives the number of pairs produced.  A pair whose computed count is 0 is never produced.
 *   KH_SET_INTERSECT       the keys in both sets, c = calc(ca, cb)
 *   KH_SET_UNION           the keys in either set: calc(ca, cb) for a key in both, its own count -- whatever calc -- for a key in one
 *   KH_SET_SUBTRACT        the keys of set A that are not in set B, c = ca                        (calc is ignored)
 *   KH_SET_COUNT_SUBTRACT  the keys of set A with ca > cb, c = ca - cb (cb = 0 for a key b lacks)  (calc is ignored)
 * CONTRACT.  a and b are only READ, like kh_lookup: their pending pushes are counted first, each table is read in the form it
 * is in (kh_stats.slot_bytes, distinct, kmers and grows of both stay what they were), a kh_result_text_* stream on either goes
 * on.  The two tables may have any two sizes and forms.  a == b is allowed.  dst is entered as a writer (its text stream ends)
 * and must be neither a nor b.  Both calls return only when they are complete: every context may be used freely afterwards.
 * The calling thread must be the one producer of all contexts involved; the sources' streams are drained before the kernels
 * start, which run on a's stream (kh_compare) / dst's stream (kh_combine_into).
 * KH_ERR_BAD_ARG -- every context usable afterwards, the text in kh_last_error(dst), or kh_last_error(a) for kh_compare: a NULL
 * context or a NULL out, dst == a or dst == b, contexts with different k or on different devices, an unknown op, an unknown
 * calc where op uses it.
 * SHARDS: all contexts of a call must be in the same shard state -- all full tables, or all the same (index, count) of
 * kh_set_shard or of a finished kh_merge_across; anything else is KH_ERR_STATE.  On equal shards every word of kh_compare ADDS
 * UP over the ranks to the full tables' value, and the union over the ranks of the kh_combine_into results is the full result. */
#define KH_CMP_WORDS 8
#define KH_CMP_DISTINCT_A 0    /* keys of a with count >= max(min_a, 1) */
#define KH_CMP_DISTINCT_B 1
#define KH_CMP_SHARED 2        /* keys in both sets */
#define KH_CMP_SUM_A 3         /* sum of a's counts over its set (modulo 2^64) */
#define KH_CMP_SUM_B 4
#define KH_CMP_SHARED_SUM_A 5  /* a's counts over the shared keys */
#define KH_CMP_SHARED_SUM_B 6
#define KH_CMP_SUM_MIN 7       /* sum over shared keys of min(ca, cb) */
int kh_compare(kh_ctx *a, kh_ctx *b, uint64_t min_a, uint64_t min_b, uint64_t *out /* KH_CMP_WORDS, host */);

#define KH_SET_INTERSECT 1
#define KH_SET_UNION 2
#define KH_SET_SUBTRACT 3        /* keys of a that b does not hold; count = ca */
#define KH_SET_COUNT_SUBTRACT 4  /* ca - cb where that is > 0 (cb = 0 for a key b lacks) */
#define KH_CALC_MIN 1
#define KH_CALC_MAX 2
#define KH_CALC_SUM 3            /* saturates at 2^64 - 1 */
#define KH_CALC_LEFT 4
#define KH_CALC_RIGHT 5
int kh_combine_into(kh_ctx *dst, kh_ctx *a, kh_ctx *b, uint32_t op, uint32_t calc,
                    uint64_t min_a, uint64_t min_b, uint64_t *n_pairs /* may be NULL */);

/* ---- de Bruijn graph degrees of a count table (no reference counterpart) --- */
/* What unitig / contig construction (BCALM, Cuttlefish after KMC), tip clipping, bubble popping, branch-point counts and walks
 * from a seed ask of a k-mer table: which of the four possible successors and four possible predecessors of a k-mer are also
 * there.  The table is read against itself on the device -- eight probes per k-mer, one byte out.
 * NODE SET S: for this context's k and a min_count, the canonical keys whose count is at least max(min_count, 1).
 * MASK of a packed canonical key x: let s be its k-letter string and canon() = min(forward, reverse complement).  One byte:
 *   bit c     (c = 0..3 for A, C, G, T), KH_GRAPH_RIGHT(c), is set iff canon(s[1:] + c) is in S;
 *   bit 4 + c,                           KH_GRAPH_LEFT(c),  is set iff canon(c + s[:-1]) is in S.
 * ORIENTATION: left and right refer to x's canonical string.
 * SPECIAL CASES: none.  A homopolymer is its own neighbour, a palindrome is possible at even k, at k = 1 every present key is
 * everyone's neighbour: all of it follows the two formulas.
 * BIT ARITHMETIC, with r = the reverse complement of x and m = the mask of the low 2k bits:
 *   right neighbour: forward ((x << 2) | c) & m,       reverse (r >> 2) | ((3 - c) << 2(k-1));
 *   left neighbour:  forward (x >> 2) | (c << 2(k-1)), reverse ((r << 2) | (3 - c)) & m.
 * KEYS OUTSIDE S: x need not be in S -- the mask of an absent or below-threshold key is still its extensions into S (what a
 * graph walk asks).
 * INVALID WORDS: a word that is not a canonical key of this k -- a bit at or above 2k, or greater than its reverse complement --
 * gets mask 0.
 * kh_graph_stats fills KH_GRAPH_WORDS words of host memory: out[m], m < 256 = the nodes of S whose mask is m, then |S| and the
 * sum of the counts over S.  kh_graph_masks_device writes masks[i] = the mask of keys[i] for all n keys in this device's memory:
 * keys at any alignment, every one of the n bytes written (d_masks at any alignment), complete when it returns -- the key array
 * is typically what kh_result_copy_device / kh_result_sorted_device just produced, so that the masks line up with those pairs.
 * kh_graph_masks is the host form, built like kh_lookup: device scratch for the call, one launch, copy back; no memory for it is
 * KH_ERR_OOM and leaves the context usable.
 * CONTRACT.  All three only READ, like kh_lookup and kh_compare: pending pushes are counted first, the table is read in the form
 * it is in (kh_stats.slot_bytes stays what it was), no count changes, a kh_result_text_* stream in progress goes on, and a bad
 * argument (NULL with n > 0, a NULL out: KH_ERR_BAD_ARG) leaves the context usable.  n == 0 is KH_OK, and the arrays may then
 * be NULL.
 * SHARDS (kh_set_shard, or after a merge across more than one rank): the neighbours of a shard's keys live on other owners, so
 * all three calls return KH_ERR_STATE with a message; the context stays usable. */
#define KH_GRAPH_RIGHT(c) (1u << (c))
#define KH_GRAPH_LEFT(c) (16u << (c))
#define KH_GRAPH_WORDS 258
#define KH_GRAPH_NODES 256   /* |S| */
#define KH_GRAPH_KMERS 257   /* sum of the counts over S, modulo 2^64 */
int kh_graph_stats(kh_ctx *ctx, uint64_t min_count, uint64_t *out /* KH_GRAPH_WORDS, host */);
int kh_graph_masks_device(kh_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint64_t min_count, uint8_t *d_masks);
int kh_graph_masks(kh_ctx *ctx, const uint64_t *keys, uint64_t n, uint64_t min_count, uint8_t *masks);

/* ---- unitigs of a count table: the compacted de Bruijn graph (no reference counterpart) --- */
/* The maximal non-branching paths of the node-centric de Bruijn graph of S -- what BCALM or Cuttlefish build after KMC --,
 * built on the device.  Everything follows from k, min_count and the table's counts; the table's size, geometry and form do
 * not show in the result.
 * NODE SET S: as for kh_graph_*, the canonical keys with a count of at least max(min_count, 1).
 * ORIENTED NODE: (x, +) spells x's canonical string s, (x, -) spells rc(s).  rev() flips the sign.
 * SUCCESSORS of an oriented node u that spells w: for each letter c, the string t = w[1:] + c gives a successor if canon(t) = y
 *   is in S; that successor is (y, +) if t equals y's string, else (y, -).  The out-degree of (x, +) is popcount(mask & 15), of
 *   (x, -) popcount(mask >> 4), with the mask of kh_graph_*.  The in-degree of v is the out-degree of rev(v): u -> v holds iff
 *   rev(v) -> rev(u).
 * COMPACTABLE LINK u -> v: outdeg(u) = 1, outdeg(rev(v)) = 1, node(u) != node(v) (which excludes the homopolymer loop u -> u
 *   and the hairpin u -> rev(u)), and neither node is a palindrome (a string equal to its reverse complement: even k only).  A
 *   palindrome takes part in no link and is always a unitig of its own.
 * UNITIG: a maximal chain u1 -> ... -> uL of compactable links.  Its sequence is spell(u1) followed by the last letter of each
 *   further ui: L + k - 1 bases.  A chain never meets its own mirror image, so every node of S lies in exactly one unitig, read
 *   in one of two mirrored directions.
 * WHICH READING is reported.  L = 1: (x, +).  A chain that does not close: the reading whose first node has the smaller key of
 *   the two end nodes.  A chain that closes (uL -> u1 is compactable too): the reading that contains (m, +) for the smallest key
 *   m of the cycle, starting there; its KH_UNI_CIRCULAR flag is set and the closing overlap is not repeated in the bases.
 * ORDER: unitigs come in ascending key order of their first node.  The same table content gives the same bytes on every run
 *   and for every geometry and form (the rule of kh_result_sorted).
 * kh_unitigs_begin builds the rows (KH_UNI_WORDS words per unitig) and the bases (ASCII ACGT, unitig after unitig, no
 * separators: START of row i + 1 = START + KMERS + k - 1 of row i) into device memory that the context owns until
 * kh_unitigs_end, the next kh_unitigs_begin, kh_reset or kh_destroy.  It enters like kh_result_sorted_device: pending pushes
 * are counted first, the table is read in the form it is in (kh_stats stays what it was), a kh_result_text_* stream in progress
 * ends; scratch comes from the idle partition buffers where there are any.  No memory is KH_ERR_OOM with nothing allocated and
 * the context usable; a shard is KH_ERR_STATE as for kh_graph_*; node ids are 32-bit, and more than 2^31 - 1 nodes is
 * KH_ERR_RANGE.  An empty S is 0 unitigs and 0 bases.
 * The copies check the capacities first: row_cap < n_unitigs or base_cap < n_bases is KH_ERR_RANGE and NOTHING is written to
 * either array; a NULL array with capacity 0 skips that array.  A copy without a live begin -- none yet, or any call since that
 * entered the context as a writer (what ends a text stream) -- is KH_ERR_STATE.  The readers kh_result_size, kh_lookup,
 * kh_histogram, kh_graph_* and kh_profile* may come between.  kh_unitigs_end with nothing begun is KH_OK. */
#define KH_UNI_WORDS 4        /* uint64 words per unitig row */
#define KH_UNI_START 0        /* offset of its first base in the base array */
#define KH_UNI_KMERS 1        /* L; it has L + k - 1 bases */
#define KH_UNI_COUNT_SUM 2    /* sum of its k-mers' counts, modulo 2^64 */
#define KH_UNI_FLAGS 3        /* bit 0: KH_UNI_CIRCULAR */
#define KH_UNI_CIRCULAR 1
int kh_unitigs_begin(kh_ctx *ctx, uint64_t min_count, uint64_t *n_unitigs, uint64_t *n_bases);
int kh_unitigs_copy_device(kh_ctx *ctx, uint64_t *d_rows, uint64_t row_cap, uint8_t *d_bases, uint64_t base_cap);
int kh_unitigs_copy(kh_ctx *ctx, uint64_t *rows, uint64_t row_cap, uint8_t *bases, uint64_t base_cap);
int kh_unitigs_end(kh_ctx *ctx);

/* ---- links between unitigs: the edges of the compacted graph (what BCALM and Cuttlefish write next to the sequences) --- */
/* With the definitions above, every unitig i has two END STATES:
 *   end +: the last oriented node of its reported reading -- the right end of the reported sequence;
 *   end -: rev() of the first oriented node of its reported reading -- the right end of the reverse complement.
 *   For L = 1 these are (x, +) and (x, -).
 * A LINK exists for every end state e and every successor v of e: every letter whose bit is set in the four mask bits of e
 *   (mask & 15 for sign +, mask >> 4 for sign -).  No link is special-cased away: homopolymer loops, hairpins and the closing
 *   link of a circular unitig are links.
 * v lies in some unitig j, which is ENTERED with sign + if v is the first oriented node of j's reported reading, with sign - if
 *   v is rev() of its last; the first is tested first, so that a palindromic unitig (L = 1, its k-mer equal to its reverse
 *   complement) is always entered as +.  Nothing else can happen: a successor of an end state is never interior to a unitig
 *   (had v a compactable link in, its in-degree were 1, e its only predecessor and e -> v compactable, so e no end -- unless e
 *   is the cut of a circular unitig, where v is that unitig's first node).  The device tests it all the same; a failure is
 *   KH_ERR_STATE "internal error".
 * LINK WORD: one uint64 per link, high 32 bits = 2 * from_unitig + from_sign, low 32 bits = 2 * to_unitig + to_sign, sign + = 0,
 *   sign - = 1.  Unitig indices are the row indices of kh_unitigs_copy (fewer than 2^31).
 * ORDER: ascending word value -- by from-unitig, + end before - end, then by to-unitig and to-sign.  Like the rows, the same
 *   table content gives the same bytes for every geometry and table form.
 * WHAT FOLLOWS: no word occurs twice; with (a, sa) -> (b, sb) the mirror (b, !sb) -> (a, !sa) is in the list (the sign of a
 *   palindromic unitig counts as either); n_links is the sum of the end states' out-degrees; a circular unitig i carries
 *   i+ -> i+ and i- -> i-; a link spans k - 1 bases of overlap (0 at k = 1).
 * kh_unitigs_begin_linked is kh_unitigs_begin -- same entry, same rows and bases, same errors -- plus the link array, in device
 * memory of the context's own with the same lifetime (kh_unitigs_end, the next begin of either kind, kh_reset, kh_destroy).  A
 * NULL n_links is KH_ERR_BAD_ARG.  kh_unitigs_copy* work after either begin.
 * The link copies enter as readers, like kh_unitigs_copy*: cap < n_links is KH_ERR_RANGE with nothing written, a NULL array
 * with capacity 0 skips, stale or not begun is KH_ERR_STATE, and so is a copy after a plain kh_unitigs_begin, which built no
 * links (the message names kh_unitigs_begin_linked). */
#define KH_UNI_LINK_FROM(w) ((uint32_t)((uint64_t)(w) >> 33))
#define KH_UNI_LINK_FROM_SIGN(w) ((uint32_t)(((uint64_t)(w) >> 32) & 1u))
#define KH_UNI_LINK_TO(w) ((uint32_t)(((uint64_t)(w) & 0xFFFFFFFFu) >> 1))
#define KH_UNI_LINK_TO_SIGN(w) ((uint32_t)((uint64_t)(w) & 1u))
int kh_unitigs_begin_linked(kh_ctx *ctx, uint64_t min_count, uint64_t *n_unitigs, uint64_t *n_bases, uint64_t *n_links);
int kh_unitigs_links_copy_device(kh_ctx *ctx, uint64_t *d_links, uint64_t cap);
int kh_unitigs_links_copy(kh_ctx *ctx, uint64_t *links, uint64_t cap);

/* ---- the live unitigs as TEXT, formatted on the device (what `kmerust unitigs -f fasta` and `kmerust gfa -f gfa` print) ----- */
/* With i the row index, L = KMERS, cs = COUNT_SUM, seq the unitig's L + k - 1 bases and km = what "%.1f" prints of
 * (double)cs / (double)L (0.0 for L = 0):
 *   KH_UNI_TEXT_FASTA  per unitig  >{i} LN:i:{L+k-1} KC:i:{cs} km:f:{km}[ CR:i:1]\n{seq}\n       (CR:i:1: KH_UNI_CIRCULAR)
 *                      no unitigs: 0 bytes
 *   KH_UNI_TEXT_GFA    first       H\tVN:Z:1.0\n
 *                      per unitig  S\t{i}\t{seq}\tLN:i:{L+k-1}\tKC:i:{cs}\tkm:f:{km}[\tCR:i:1]\n
 *                      per link word, in array order  L\t{from}\t{+|-}\t{to}\t{+|-}\t{k-1}M\n
 *                      no unitigs: the header line alone.  Needs kh_unitigs_begin_linked.
 * A pull interface like kh_result_text_*: kh_unitigs_text_begin sizes the document (*n_bytes: its length, may be NULL), every
 * kh_unitigs_text_next* hands out the next piece.  A unitig has no length bound, so a piece is a BYTE RANGE, not whole lines:
 *   - next writes *n = min(cap, bytes left); *n = 0 with KH_OK says that the stream has ended.  cap = 0 while bytes are left is
 *     KH_ERR_RANGE and consumes nothing.  A NULL n, or a NULL buffer with cap > 0, is KH_ERR_BAD_ARG.
 *   - The concatenation of the pieces is the same document for EVERY sequence of cap values, and the same table content gives
 *     the same bytes for every geometry and table form (as the rows, bases and links do).
 *   - kh_unitigs_text_next takes pageable memory, or memory of kh_host_alloc / kh_host_register; the next chunk (up to 64 MiB) is
 *     formatted while the current one travels.  kh_unitigs_text_next_device writes device memory of this context's device at
 *     any alignment, nothing at or behind d_buf[*n], and is complete when it returns.
 *   - begin enters as a reader; the stream belongs to the live unitigs and ends with kh_unitigs_end, the next begin of either
 *     kind, kh_reset / kh_destroy and every call that makes the unitigs stale.  KH_ERR_STATE: begin without live unitigs,
 *     KH_UNI_TEXT_GFA after a plain kh_unitigs_begin (the message names kh_unitigs_begin_linked), next without a running stream.
 *     KH_ERR_BAD_ARG: an unknown format.  begin on a running stream restarts it.
 *   - Every reader may come between two next calls -- kh_unitigs_copy*, kh_unitigs_links_copy*, a whole kh_result_text_* stream:
 *     the two streams share no memory (the chunks here are the stream's own, never the partition buffers).
 *   - KH_ERR_OOM follows the rule of the reading calls: the context is not poisoned, the unitigs stay live, no stream is on and
 *     what the stream had allocated is released -- begin again. */
#define KH_UNI_TEXT_FASTA 1   /* the bytes `kmerust unitigs -f fasta` prints */
#define KH_UNI_TEXT_GFA   2   /* the bytes `kmerust gfa -f gfa` prints; needs kh_unitigs_begin_linked */
int kh_unitigs_text_begin(kh_ctx *ctx, uint32_t format, uint64_t *n_bytes /* may be NULL */);
int kh_unitigs_text_next(kh_ctx *ctx, uint8_t *buf, uint64_t cap, uint64_t *n);
int kh_unitigs_text_next_device(kh_ctx *ctx, uint8_t *d_buf, uint64_t cap, uint64_t *n);

/* ---- the k-mers of new sequences LOCATED on the live unitigs (what read threading and pseudo-alignment start from) -------- */
/* kh_profile* tell a window the COUNT of its k-mer; these tell it WHERE in the compacted graph that k-mer is.  They need the live
 * unitigs of kh_unitigs_begin or kh_unitigs_begin_linked.  Let Q_u be the reported sequence of unitig u (row index u, L_u = KMERS).
 * INPUT, windows, quality masking and the chunks of the host form are those of kh_profile_device / kh_profile: a flat buffer,
 *   separators outside ACGTacgt, d_bases and d_qual at any alignment.
 * OUTPUT: n words, indexed by the window start; every one is written.
 *   - KH_LOC_NO_WINDOW exactly where kh_profile writes KH_PROFILE_NO_WINDOW.
 *   - KH_LOC_ABSENT: a valid window whose canonical k-mer is not in S -- not in the table, or with a count below the min_count
 *     of the begin that built the unitigs.
 *   - otherwise a PLACE.  With w the window's k letters there is exactly one (u, j), 0 <= j < L_u, with Q_u[j .. j+k) == w or
 *     Q_u[j .. j+k) == rc(w): every node lies in exactly one unitig exactly once (a circular unitig has L + k - 1 bases too, so
 *     all its L k-mers are windows of its bases).  Sign 0 (+): Q_u[j .. j+k) == w; sign 1 (-): it equals rc(w); a palindromic w
 *     (even k) is +.  High 32 bits = 2 * u + sign -- the state encoding of a link word's halves, so a located window and a
 *     link end compare directly --, low 32 bits = j.  u <= 2^31 - 2, so the high word of a place is never that of the specials.
 * WHAT FOLLOWS for two consecutive window starts i, i + 1 that are both places: either both lie in the same unitig with the
 *   same sign and the offset moves by +1 (+) or by -1 (-); or window i is at the last offset of its direction (L - 1 for +, 0
 *   for -), window i + 1 at the first offset of its direction (0 for +, L - 1 for -) and (2u + s) -> (2u' + s') is a link word
 *   of kh_unitigs_begin_linked -- the closing link of a circular unitig is such a link.  A read is a walk in the GFA.
 *   REVERSE COMPLEMENT: for a record R of m valid bases, locate(rc(R))[i] is locate(R)[m - k - i] with the sign flipped (a
 *   palindrome is + both times).
 * ENTRY: both enter as readers, like kh_profile*: the table is read in the form it is in, kh_stats is unchanged, a
 *   kh_result_text_* or kh_unitigs_text_* stream goes on, and they may come between any two readers.  KH_ERR_STATE without live
 *   unitigs; KH_ERR_BAD_ARG for a NULL array with n > 0 or an output that is not 8-byte aligned (the context stays usable);
 *   n == 0 is KH_OK; an empty S (0 unitigs) gives only the two specials.
 * THE INDEX: the first locate call after a begin builds the place map, one uint64 per table slot (table_slots * 8 bytes of
 *   device memory of the context's own), from the rows and bases.  It lives and dies with the unitigs: kh_unitigs_end, the next
 *   begin, kh_reset, kh_destroy; a begin that is never located allocates nothing for it.  KH_ERR_OOM follows the rule of the
 *   reading calls: the context is not poisoned, the unitigs stay live, nothing of the index stays allocated, and the next
 *   locate call tries again.  Later calls of kh_unitigs_locate_device allocate nothing. */
#define KH_LOC_NO_WINDOW (~0ull)
#define KH_LOC_ABSENT (~0ull - 1ull)
#define KH_LOC_IS_PLACE(w) ((uint64_t)(w) < KH_LOC_ABSENT)
#define KH_LOC_UNITIG(w) ((uint32_t)((uint64_t)(w) >> 33))
#define KH_LOC_SIGN(w) ((uint32_t)(((uint64_t)(w) >> 32) & 1u))
#define KH_LOC_OFFSET(w) ((uint32_t)((uint64_t)(w) & 0xFFFFFFFFu))
int kh_unitigs_locate_device(kh_ctx *ctx, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, uint64_t *d_out);
int kh_unitigs_locate(kh_ctx *ctx, const uint8_t *bases, const uint8_t *qual, uint64_t n, uint64_t *out);

/* ---- the same walk as RUN-COMPRESSED PATHS: one row per stretch of a record along one unitig (read threading, GAF / P lines) - */
/* Let W[0 .. n) be what kh_unitigs_locate* writes for the same bases, qual, n and context.  These calls fold W on the device
 * into runs -- "unitig 17 + from offset 3 for 58 k-mers, then unitig 40 - ..." -- so that 16 bytes per run leave it, not 8 per base.
 * RECORDS: rec_start has nrec + 1 ascending entries, rec_start[nrec] <= n (the rule of kh_profile_records).  Record r owns the
 *   window starts rec_start[r] <= i < rec_start[r+1]; the segments need not coincide with separators; window starts outside
 *   every record belong to no run.
 * CONTINUATION: W[i+1] continues W[i] iff both are places, both have the same high word, and W[i+1]'s offset is W[i]'s offset + 1
 *   (sign +) or - 1 (sign -).  A link crossing is no continuation and begins a new run: the closing link of a circular unitig
 *   (offset L - 1 -> 0) and each turn of a homopolymer loop included.
 * RUN: a maximal stretch of window starts of ONE record in which every window continues its predecessor.  A record boundary ends a
 *   run even where W continues across it.  KH_LOC_ABSENT and KH_LOC_NO_WINDOW belong to no run: the gap between one run's QEND
 *   and the next one's QSTART says how many there were.
 * OUTPUT: run_start always gets all nrec + 1 entries, as CSR: the runs of record r are rows run_start[r] .. run_start[r+1], in
 *   ascending QSTART, and run_start[nrec] = *n_runs, always the number of runs of the call (runs <= window starts).  An empty
 *   record, or one without a place, has an empty range.  A row is KH_RUN_WORDS uint32 words (below).
 *   run_cap < *n_runs: KH_ERR_RANGE; run_start and *n_runs are complete, the first run_cap rows hold unspecified values, nothing at
 *   or behind row run_cap is written, cover is unchanged, the context is usable.  run_cap == 0 takes runs == NULL: how a caller sizes.
 * COVERAGE: cover may be NULL; else n_unitigs * KH_COV_WORDS uint64 words, indexed by the row index of kh_unitigs_copy.  On KH_OK
 *   only, cover[u][KH_COV_WINDOWS] += the windows of every run on u and cover[u][KH_COV_RUNS] += their number: a caller streams
 *   batches into one array.  Device memory in the device form, host memory in the host form.
 * OTHERWISE the contract of kh_unitigs_locate*: both enter as readers, need live unitigs of either begin (KH_ERR_STATE), leave
 *   kh_stats and a kh_result_text_* or kh_unitigs_text_* stream alone, build the place map if no locate call has yet (the one
 *   index: a later locate call finds it built, and the other way round), and follow the reading calls' KH_ERR_OOM rule: not
 *   poisoned, unitigs live, nothing of the call stays allocated beyond what that rule lets a context keep.  The device form cuts its
 *   input into the chunks of the host form.  nrec == 0: KH_OK, *n_runs = 0, nothing else written.  n == 0 with nrec > 0: all
 *   run_start entries are 0.  An empty S gives 0 runs.
 * KH_ERR_BAD_ARG (the context stays usable): NULL n_runs; NULL bases with n > 0; NULL rec_start or run_start with nrec > 0; NULL
 *   runs with run_cap > 0; runs not 4-byte aligned; rec_start, run_start or cover not 8-byte aligned.  In the host form only:
 *   rec_start not ascending, rec_start[nrec] > n, or a record of 2^32 or more window starts -- for the device form these three are
 *   the caller's contract: offsets that break it give unspecified rows and never an access outside the arrays.
 * WHAT FOLLOWS: expanding every run gives exactly the place words of W inside the records.  For a record R of m valid bases,
 *   paths(rc(R)) is paths(R) reversed, with the sign flipped, OFFSET replaced by the run's last offset, and QSTART / QEND mirrored
 *   in the m - k + 1 windows.  With kh_unitigs_begin_linked, consecutive runs of a record with QEND == the next QSTART are joined
 *   by a link word. */
#define KH_RUN_WORDS 4      /* uint32 words per run row */
#define KH_RUN_STATE 0      /* 2 * unitig + sign: the high word of the run's first place, a link word's half */
#define KH_RUN_OFFSET 1     /* offset of the run's FIRST window in the unitig's reported sequence (a '-' run descends from it) */
#define KH_RUN_QSTART 2     /* first window start of the run, relative to its record's rec_start[r] */
#define KH_RUN_QEND 3       /* one behind its last window start, relative to the same: the run has QEND - QSTART windows */
#define KH_COV_WORDS 2      /* uint64 words per unitig of the coverage array */
#define KH_COV_WINDOWS 0    /* window starts of the call's records located on the unitig, either sign */
#define KH_COV_RUNS 1       /* runs on it */
int kh_unitigs_paths_device(kh_ctx *ctx, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, const uint64_t *d_rec_start,
                            uint64_t nrec, uint64_t *d_run_start, uint32_t *d_runs, uint64_t run_cap, uint64_t *d_cover, uint64_t *n_runs);
int kh_unitigs_paths(kh_ctx *ctx, const uint8_t *bases, const uint8_t *qual, uint64_t n, const uint64_t *rec_start,
                     uint64_t nrec, uint64_t *run_start, uint32_t *runs, uint64_t run_cap, uint64_t *cover, uint64_t *n_runs);

/* ---- READ SUPPORT PER LINK: how many records walk from one unitig end into another (edge weights, the RC:i: tag of an L line) -- */
/* cover tells how much read evidence lies on a node of the compacted graph; these calls tell it for an edge.  They need the live
 * unitigs of kh_unitigs_begin_linked and count, on the device, the link crossings of run rows.
 * INPUT: run_start and runs are what a kh_unitigs_paths* call wrote: run_start has nrec + 1 CSR entries with run_start[nrec] ==
 *   n_runs, runs has n_runs rows of KH_RUN_WORDS words.  The rows need not come from this library: only the lookup below is defined
 *   on them.  Rows in front of run_start[0] belong to no record.
 * CROSSING: rows i and i + 1 form a crossing if both belong to the same record and QEND of row i == QSTART of row i + 1.  The last
 *   row of a record never pairs with the first row of the next, whatever their QSTART / QEND.  The WORD of a crossing is
 *   (STATE_i << 32) | STATE_{i+1}: a run stays in one unitig in one direction, so its STATE is both the end state it leaves through
 *   and the state it was entered with -- the encoding of a link word.  If the word is link number l of kh_unitigs_links_copy,
 *   support[l] += 1; otherwise the crossing counts as KH_SUP_MISSING and nothing is stored for it.  The closing link of a circular
 *   unitig and every turn of a homopolymer loop are crossings.
 * OUTPUT: support has n_links 64-bit counters in link-array order; they wrap modulo 2^64.  Counts are ADDED: a caller streams
 *   batches into one array, as with cover.  Device memory in the device form, host memory in the host form.  cap < n_links is
 *   KH_ERR_RANGE with nothing written; a NULL support with cap == 0 is allowed only when n_links == 0.  out (host memory in both
 *   forms, may be NULL) gets the KH_SUP_WORDS words of THIS call, not added.  On anything but KH_OK, support and out are untouched.
 * STRANDS: a crossing credits the word as read.  The same read reverse-complemented credits the mirror word
 *   ((b ^ 1) << 32) | (a ^ 1) of (a << 32) | b, which is in the list too; support[l] + support[mirror(l)] is the strand-free
 *   number and is the caller's arithmetic.  (The sign of a palindromic unitig counts as either: see WHAT FOLLOWS of the links.  A
 *   link into or out of one may be its own mirror, or mirror a word that differs from it in that sign only.)
 * ENTRY: both enter as readers, like kh_unitigs_paths*: kh_stats, the table and a running kh_result_text_* or kh_unitigs_text_*
 *   stream are left alone.  They never touch the table or the place map and do not build the place map.  KH_ERR_STATE without live
 *   unitigs, and after a plain kh_unitigs_begin, which built no links (the message names kh_unitigs_begin_linked).
 * KH_ERR_BAD_ARG (the context stays usable): NULL run_start or runs with n_runs > 0; NULL run_start with nrec > 0; NULL support with
 *   cap > 0; runs not 4-byte aligned; run_start or support not 8-byte aligned.  In the host form only: run_start not ascending, or
 *   run_start[nrec] != n_runs -- for the device form these two are the caller's contract: offsets or rows that break it give
 *   unspecified credits and never an access outside runs[0 .. n_runs), support[0 .. n_links) or the library's own arrays.  A STATE of
 *   2 * n_unitigs or more is simply KH_SUP_MISSING.
 * n_runs < 2 or nrec == 0: KH_OK, out all zero, nothing else written.
 * THE LINK INDEX: the first call after a kh_unitigs_begin_linked builds it, one uint64 per end state and KH_SUP_WORDS more
 *   ((2 * n_unitigs + KH_SUP_WORDS) * 8 bytes of device memory of the context's own).  It lives and dies with the unitigs:
 *   kh_unitigs_end, the next begin, kh_reset, kh_destroy; a begin that never asks for support allocates nothing for it.  KH_ERR_OOM
 *   follows the rule of the reading calls: the context is not poisoned, the unitigs stay live, nothing of the index or of the call
 *   stays allocated beyond what that rule lets a context keep (the pinned staging of the host form), and the next call tries again.
 *   Later calls of kh_unitigs_link_support_device allocate nothing. */
#define KH_SUP_WORDS 4
#define KH_SUP_PAIRS 0      /* consecutive rows i, i+1 that belong to one record */
#define KH_SUP_ADJACENT 1   /* of those: QEND of row i == QSTART of row i+1 (no window start between them) */
#define KH_SUP_CREDITED 2   /* of those: (STATE_i << 32) | STATE_{i+1} is a link word; support[its index] += 1 */
#define KH_SUP_MISSING 3    /* ADJACENT - CREDITED: 0 for rows that kh_unitigs_paths* wrote on these unitigs */
int kh_unitigs_link_support_device(kh_ctx *ctx, const uint64_t *d_run_start, uint64_t nrec, const uint32_t *d_runs, uint64_t n_runs,
                                   uint64_t *d_support, uint64_t cap, uint64_t *out /* KH_SUP_WORDS, host, may be NULL */);
int kh_unitigs_link_support(kh_ctx *ctx, const uint64_t *run_start, uint64_t nrec, const uint32_t *runs, uint64_t n_runs,
                            uint64_t *support, uint64_t cap, uint64_t *out);

/* ---- CONNECTED COMPONENTS: which unitigs hang together (Bandage's component view, per-component length and coverage) ---------- */
/* The calls work on the live unitigs of kh_unitigs_begin_linked.  Two unitigs are in the same component iff a chain of link words
 * joins them, ignoring signs and direction: every link has its mirror in the list, so the link array is an undirected edge list.
 * A link from a unitig to itself (the closing link of a circle, the turns of a loop, a hairpin) joins nothing; a unitig without a
 * link to another unitig is a component of its own.
 * OUTPUT: comp[u] (uint32) is the dense id of unitig u's component: ids run 0 .. C-1 in ascending order of the component's
 *   smallest unitig index, so comp[0] == 0.  rows has C rows of KH_COMP_WORDS words, one per component, in id order.  Unitig order
 *   does not depend on the table, so the same index content gives the same bytes for every geometry and both table forms.
 *   Device memory in the device form, host memory in the host form.  out (host memory in both forms, REQUIRED) gets the
 *   KH_CC_WORDS words; it is complete on KH_OK and on KH_ERR_RANGE, which is how a caller sizes rows.
 * CAPS: either array may be NULL with a cap of 0: not wanted.  A non-zero comp_cap < n_unitigs or a non-zero row_cap < C is
 *   KH_ERR_RANGE with nothing written to either array; otherwise nothing at or behind comp[n_unitigs] / rows[C] is written.
 * ENTRY: both enter as readers, like kh_unitigs_link_support*: kh_stats, the table, the place map and a running
 *   kh_result_text_* or kh_unitigs_text_* stream are left alone.  KH_ERR_STATE without live unitigs, and after a plain
 *   kh_unitigs_begin, which built no links (the message names kh_unitigs_begin_linked).  No unitigs: KH_OK, out all zero.
 * KH_ERR_BAD_ARG (the context stays usable): NULL out; a NULL array with a non-zero cap; comp not 4-byte aligned; rows or out not
 *   8-byte aligned.
 * THE LABELS are built by the first call after a kh_unitigs_begin_linked (hook and compress rounds over the link array, then the
 *   sums per component) and kept with the unitigs: 4 bytes per unitig and 32 per component of device memory of the context's own,
 *   until kh_unitigs_end, the next begin, kh_reset or kh_destroy; a begin that never asks allocates nothing for them.  Later calls
 *   of kh_unitigs_components_device allocate nothing and run no kernel, only copies.  KH_ERR_OOM follows the rule of the reading
 *   calls: the context is not poisoned, the unitigs stay live, nothing of half-built labels stays allocated, and the next call
 *   tries again. */
#define KH_COMP_WORDS 4        /* uint64 words per component row */
#define KH_COMP_FIRST 0        /* its smallest unitig index; rows ascend in it */
#define KH_COMP_UNITIGS 1
#define KH_COMP_KMERS 2        /* sum of KH_UNI_KMERS of its unitigs */
#define KH_COMP_COUNT_SUM 3    /* sum of KH_UNI_COUNT_SUM, modulo 2^64 */
#define KH_CC_WORDS 4          /* the call's statistics, host memory */
#define KH_CC_COMPONENTS 0
#define KH_CC_SINGLETONS 1     /* components of exactly one unitig */
#define KH_CC_LARGEST_KMERS 2  /* the greatest KH_COMP_KMERS; 0 when there is no unitig */
#define KH_CC_ROUNDS 3         /* hooking rounds the build ran, the last (empty) one included; the same value on every later call */
int kh_unitigs_components_device(kh_ctx *ctx, uint32_t *d_comp, uint64_t comp_cap, uint64_t *d_rows, uint64_t row_cap,
                                 uint64_t *out /* KH_CC_WORDS, host */);
int kh_unitigs_components(kh_ctx *ctx, uint32_t *comp, uint64_t comp_cap, uint64_t *rows, uint64_t row_cap, uint64_t *out);

/* ---- tip clipping: one round of removing short dead-end branches (what assemblers do first with the compacted graph) --- */
/* Take the unitigs and links of kh_unitigs_begin_linked(src, min_count): rows, end states (i, +) and (i, -) and link words exactly
 * as defined above.  out(i, s) is the set of links whose from-state is (i, s).
 * CANDIDATE: unitig i is a candidate when it is not KH_UNI_CIRCULAR, KMERS <= max_kmers, exactly one of out(i, +) and out(i, -)
 *   is empty -- that end is the dead end, the other the ATTACHED end a_i --, and no link of out(a_i) goes to unitig i itself
 *   (with either sign).
 * RIVALS of a link a_i -> (j, t): the unitig indices b of all links (j, 1 - t) -> (b, sb).  By the mirror property of the link
 *   list these are the unitigs that enter (j, t), and i is always among them (the device tests it all the same; a failure is
 *   KH_ERR_STATE "internal error").  The sign of a palindromic unitig does not matter here: only indices are compared.
 * BEATS: b beats i when b is no candidate, or b is a candidate and (KMERS_b, COUNT_SUM_b) is lexicographically greater than
 *   (KMERS_i, COUNT_SUM_i), or the two are equal and b < i.  COUNT_SUM is the row's word as stored, modulo 2^64.
 * CLIPPED: a candidate i is clipped when, at EVERY link of out(a_i), some rival b != i beats it.  All other unitigs survive.
 * One call is one round: it decides from the graph as built, nothing cascades inside it.  A fork of two short dead ends loses
 *   the weaker one; a short dead end beside a long branch, or beside one that continues, is lost; a short piece with two dead
 *   ends or with none is not touched.
 * RESULT: every k-mer of every surviving unitig is added to dst with its count from src -- count += c, exactly as
 *   kh_merge_pairs_device does: a fresh or kh_reset dst ends up holding S minus the clipped k-mers.  K-mers of src below
 *   min_count are not in S and are not copied.  max_kmers == 0 makes nothing a candidate: dst receives S.
 * src is entered as kh_unitigs_begin_linked enters it (pending pushes are counted first, the table is read in the form it is
 *   in, a text stream in progress ends, the partition buffers serve as scratch, a shard is KH_ERR_STATE, more than 2^31 - 1 nodes
 *   is KH_ERR_RANGE); its table, counts and kh_stats are unchanged.  Any unitigs src had begun are RELEASED: afterwards
 *   kh_unitigs_copy* and kh_unitigs_links_copy* on src are KH_ERR_STATE until the next begin.  dst is entered as kh_combine_into
 *   enters its target.  dst == src, a NULL src or a NULL out is KH_ERR_BAD_ARG; different k or different devices are
 *   KH_ERR_BAD_ARG, different shard states KH_ERR_STATE, as for kh_combine_into; every such refusal leaves both contexts usable.
 *   No memory for the call's scratch is KH_ERR_OOM with src usable and dst holding what it held.  An empty S is KH_OK with all
 *   words 0.  The error text is on dst. */
#define KH_CLIP_WORDS 8
#define KH_CLIP_UNITIGS 0         /* unitigs of src at min_count */
#define KH_CLIP_CANDIDATES 1
#define KH_CLIP_CLIPPED 2         /* unitigs clipped */
#define KH_CLIP_CLIPPED_KMERS 3   /* sum of their KMERS */
#define KH_CLIP_CLIPPED_COUNT 4   /* sum of their COUNT_SUM, modulo 2^64 */
#define KH_CLIP_KEPT_KMERS 5      /* pairs added to dst */
#define KH_CLIP_KEPT_COUNT 6      /* sum of their counts, modulo 2^64 */
#define KH_CLIP_LINKS 7           /* links of src's compacted graph */
int kh_clip_tips_into(kh_ctx *dst, kh_ctx *src, uint64_t min_count, uint64_t max_kmers, uint64_t *out /* KH_CLIP_WORDS, host */);

/* ---- bubble popping: one round of removing short parallel branches (what assemblers do next to tip clipping) --- */
/* Sequencing errors and heterozygous sites in the middle of a read leave bubbles: two or three short unitigs between the same
 * two places.  Take the unitigs and links of kh_unitigs_begin_linked(src, min_count): rows, end states (i, +) and (i, -) and link
 * words exactly as defined above.  out(i, s) is the set of links whose from-state is (i, s); to(w) is the low 32 bits of a link
 * word, the entered state 2 * unitig + sign.
 * CANDIDATE: unitig i is a candidate when it is not KH_UNI_CIRCULAR, KMERS <= max_kmers, out(i, +) and out(i, -) hold exactly
 *   one link each, and neither link goes to unitig i itself (with either sign).
 * EXITS(i): the unordered pair {to(out(i, +)), to(out(i, -))}; the two may be equal.
 * PARALLEL: candidates i != b are parallel when EXITS(i) == EXITS(b).  The reported reading of a unitig is chosen by its end
 *   keys, so two branches of one bubble are often reported in opposite directions: hence the unordered pair.  A palindromic
 *   unitig is always entered as +, so the words compare as stored.  Being parallel is an equivalence relation among candidates;
 *   all members of a class enter the same state, so a class has at most four members.
 * BEATS: b beats i when COUNT_SUM_b * KMERS_i > COUNT_SUM_i * KMERS_b -- the greater mean count, compared EXACTLY as 128-bit
 *   products, COUNT_SUM being the row's word as stored, modulo 2^64; no floating point --, or the products are equal and
 *   KMERS_b > KMERS_i, or both are equal and b < i.
 * POPPED: a candidate is popped when some parallel candidate beats it.  Exactly one member of every class survives; a candidate
 *   with no parallel survives; every unitig that is no candidate survives -- a branch longer than max_kmers beside a short one
 *   too, and the short one with it.
 * One call is one round: it decides from the graph as built, nothing cascades inside it.  Popping never disconnects the two
 *   places a class joins.  The unitigs that enter the state i's + end enters are found as for the rivals of tip clipping, by the
 *   links out of that state reversed; i is always among them (the device tests it all the same; a failure, or link offsets that
 *   do not add up, is KH_ERR_STATE "internal error").
 * RESULT: every k-mer of every surviving unitig is added to dst with its count from src -- count += c, exactly as
 *   kh_merge_pairs_device does: a fresh or kh_reset dst ends up holding S minus the popped k-mers.  K-mers of src below
 *   min_count are not in S and are not copied.  max_kmers == 0 makes nothing a candidate: dst receives S.  Alternating this call
 *   and kh_clip_tips_into between two contexts (kh_reset in between) simplifies the graph round by round; every reader of a
 *   table then works on the simplified graph.
 * ENTRY and ERRORS are those of kh_clip_tips_into, word for word: src is entered as kh_unitigs_begin_linked enters it (pending
 *   pushes are counted first, the table is read in the form it is in, a text stream in progress ends, the partition buffers serve
 *   as scratch, a shard is KH_ERR_STATE, more than 2^31 - 1 nodes is KH_ERR_RANGE); its table, counts and kh_stats are unchanged.
 *   Any unitigs src had begun are RELEASED.  dst is entered as kh_combine_into enters its target.  dst == src, a NULL src or a
 *   NULL out is KH_ERR_BAD_ARG; different k or different devices are KH_ERR_BAD_ARG, different shard states KH_ERR_STATE; every
 *   such refusal leaves both contexts usable.  No memory for the call's scratch is KH_ERR_OOM with src usable and dst holding
 *   what it held.  An empty S is KH_OK with all words 0.  The error text is on dst.
 * Words 0 to 7 mean what the KH_CLIP_* words of the same index mean. */
#define KH_POP_WORDS 9
#define KH_POP_UNITIGS 0          /* unitigs of src at min_count */
#define KH_POP_CANDIDATES 1
#define KH_POP_POPPED 2           /* unitigs popped */
#define KH_POP_POPPED_KMERS 3     /* sum of their KMERS */
#define KH_POP_POPPED_COUNT 4     /* sum of their COUNT_SUM, modulo 2^64 */
#define KH_POP_KEPT_KMERS 5       /* pairs added to dst */
#define KH_POP_KEPT_COUNT 6       /* sum of their counts, modulo 2^64 */
#define KH_POP_LINKS 7            /* links of src's compacted graph */
#define KH_POP_BUBBLES 8          /* classes of at least two parallel candidates = survivors that beat someone */
int kh_pop_bubbles_into(kh_ctx *dst, kh_ctx *src, uint64_t min_count, uint64_t max_kmers, uint64_t *out /* KH_POP_WORDS, host */);

/* ---- dropping small components: removing the isolated debris that clipping and popping cannot touch (the third cleaning step) --- */
/* Take the unitigs and links of kh_unitigs_begin_linked(src, min_count) and their connected components as
 * kh_unitigs_components defines them.
 * DROPPED: a component is dropped iff the k-mers of all its unitigs together (its KH_COMP_KMERS) number fewer than min_kmers.
 *   min_kmers of 0 or 1 drops nothing.  A circular unitig is treated like any other: whether a short plasmid is debris is the
 *   caller's choice of bound.  One call is one round, and it is idempotent: what survives has min_kmers k-mers or more in each
 *   component, and removing whole components changes no other.
 * RESULT: every k-mer of every unitig of a surviving component is added to dst with its count from src -- count += c, exactly as
 *   kh_merge_pairs_device does.  K-mers of src below min_count are not in S and are not copied.
 * ENTRY and ERRORS are those of kh_clip_tips_into, word for word: src is entered as kh_unitigs_begin_linked enters it (pending
 *   pushes are counted first, the table is read in the form it is in, a text stream in progress ends, the partition buffers serve
 *   as scratch, a shard is KH_ERR_STATE, more than 2^31 - 1 nodes is KH_ERR_RANGE); its table, counts and kh_stats are unchanged.
 *   Any unitigs src had begun are RELEASED.  dst is entered as kh_combine_into enters its target.  dst == src, a NULL src or a
 *   NULL out is KH_ERR_BAD_ARG; different k or different devices are KH_ERR_BAD_ARG, different shard states KH_ERR_STATE; every
 *   such refusal leaves both contexts usable.  No memory for the call's scratch is KH_ERR_OOM with src usable and dst holding
 *   what it held.  An empty S is KH_OK with all words 0.  The error text is on dst.
 * Words 0, 5, 6 and 7 mean what the KH_CLIP_* words of the same index mean. */
#define KH_DROP_WORDS 9
#define KH_DROP_UNITIGS 0          /* unitigs of src at min_count */
#define KH_DROP_COMPONENTS 1
#define KH_DROP_DROPPED 2          /* components dropped */
#define KH_DROP_DROPPED_KMERS 3
#define KH_DROP_DROPPED_COUNT 4    /* modulo 2^64 */
#define KH_DROP_KEPT_KMERS 5       /* pairs added to dst */
#define KH_DROP_KEPT_COUNT 6       /* sum of their counts, modulo 2^64 */
#define KH_DROP_LINKS 7            /* links of src's compacted graph */
#define KH_DROP_DROPPED_UNITIGS 8
int kh_drop_components_into(kh_ctx *dst, kh_ctx *src, uint64_t min_count, uint64_t min_kmers, uint64_t *out /* KH_DROP_WORDS, host */);

/* ---- multi-GPU merge (no reference counterpart) ----------- */
/* Owner shard of a packed canonical k-mer among nparts shards: a fast-range of the top bits of
 * the table hash, so a shard is a contiguous range of table regions (same function on host and
 * device). */
uint32_t kh_owner(uint64_t key, uint32_t k, uint32_t nparts);

/* Fast path for a power-of-two number of ranks whose tables have the same size:
 *   sender:   kh_export_regions_device -- live pairs in REGION order (hence grouped by owner) plus the
 *             live count of every region; part_counts[p] (host) = pairs owned by shard p.
 *   exchange: all-to-all of the pair segments and of each owner's slice of the region counts.
 *   receiver: kh_reset, kh_set_shard(rank, nranks), kh_merge_regions_device -- the shard table is
 *             rebuilt region by region in LDS from the senders' segments (no global atomics).
 * *table_regions receives the sender's region count (must be equal on all ranks).
 * A shard table holds only keys of its hash range: it accepts kh_merge_* but not kh_push*
 * (KH_ERR_STATE); kh_reset turns it back into a full table. */
int kh_set_shard(kh_ctx *ctx, uint32_t index, uint32_t count);
int kh_export_regions_device(kh_ctx *ctx, uint32_t nparts, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap,
                             uint32_t *d_region_counts, uint64_t region_cap, uint64_t *part_counts,
                             uint64_t *table_regions);
/* d_keys[s], d_counts[s]: sender s's pairs for THIS shard (device pointers, host arrays of nsenders
 * entries); d_region_counts[s]: sender s's live counts of the sender_regions / shard_count regions of
 * this shard's range.  A sender whose region counts are all zero is never dereferenced: its key /
 * count pointers may be anything, NULL included (d_region_counts[s] must stay valid).  The same
 * holds for the packed and heads variants below. */
int kh_merge_regions_device(kh_ctx *ctx, uint32_t nsenders, uint64_t sender_regions,
                            const uint64_t *const *d_keys, const uint64_t *const *d_counts,
                            const uint32_t *const *d_region_counts);

/* Packed form of the same two calls -- half the bytes on the links: ONE uint64 per pair,
 * count << 32 | the 32 bits of the table hash below the region index (the receiver knows every
 * segment's region, and the hash is a bijection, so the key comes back exactly).  Representable iff
 * 2k - log2(table_regions) <= 32 and every count < 2^32; otherwise the export returns KH_ERR_RANGE
 * and the caller uses the unpacked pair of calls (all ranks must take the same route). */
int kh_export_regions_packed_device(kh_ctx *ctx, uint32_t nparts, uint64_t *d_pairs, uint64_t cap,
                                    uint32_t *d_region_counts, uint64_t region_cap, uint64_t *part_counts,
                                    uint64_t *table_regions);
int kh_merge_regions_packed_device(kh_ctx *ctx, uint32_t nsenders, uint64_t sender_regions,
                                   const uint64_t *const *d_pairs, const uint32_t *const *d_region_counts);
/* Narrowest form -- a quarter of the bytes: 32-bit "heads" = [2k - log2(table_regions) hash bits |
 * addend - 1 in the remaining cb bits].  A pair whose count exceeds 2^cb travels as several heads of
 * the same key (the receiver adds them up); part_counts / region counts are in heads.  Applies iff
 * 1 <= 2k - log2(table_regions) <= 28 and no count exceeds 64 * 2^cb, else KH_ERR_RANGE.  `cap` is
 * in heads (allow ~2x the distinct count). */
int kh_export_regions_heads_device(kh_ctx *ctx, uint32_t nparts, uint32_t *d_heads, uint64_t cap,
                                   uint32_t *d_region_counts, uint64_t region_cap, uint64_t *part_counts,
                                   uint64_t *table_regions);
int kh_merge_regions_heads_device(kh_ctx *ctx, uint32_t nsenders, uint64_t sender_regions,
                                  const uint32_t *const *d_heads, const uint32_t *const *d_region_counts);

/* Exchange in pieces, so that export, all-to-all and merge of successive pieces overlap: after
 * kh_set_region_window(ctx, piece, npieces) (npieces a power of two <= 64) the three export calls above
 * cover only piece `piece` of every owner's region range -- the counts of the other regions come back as
 * zero and nothing of them is written, so the caller sees an ordinary export of a table that is empty
 * elsewhere -- and the three merge calls rebuild only the matching share of the shard's regions (the
 * senders' region-count arrays keep their full length, zero outside the piece).  Pieces may come in any
 * order; a merge into an empty shard table stays a "fresh" rebuild for every piece.  Anything else that
 * touches the table in between is allowed (the pieces still missing then count as empty).
 * (0, 1) restores whole-range calls.  KH_ERR_BAD_ARG if a range has fewer regions than pieces. */
int kh_set_region_window(kh_ctx *ctx, uint32_t piece, uint32_t npieces);
/* Exchange units held by every region of the whole table (ignores the window): heads (unit_bytes 4),
 * packed pairs (8) or pairs (16) -- the first phase of the matching export on its own, so that a
 * pipelined exchange can announce the sizes of all its pieces before the first one is compacted.
 * Blocks until d_region_counts is complete.  KH_ERR_RANGE as the matching export. */
int kh_region_unit_counts_device(kh_ctx *ctx, uint32_t unit_bytes, uint32_t *d_region_counts, uint64_t region_cap,
                                 uint64_t *table_regions);

/* Small k (2k <= 26): the whole key space is a dense array of 4^k counts, which -- unlike a hash
 * table -- IS element-wise reducible: ranks merge with one all-reduce(sum) (any number of ranks,
 * tables of any size).  kh_export_dense_device: d_dense[key] = count, 0 for absent keys.
 * kh_merge_dense_device: count[key] += d_dense[key] for the keys shard `owner` of `nparts` owns
 * (kh_owner); the table keeps its full geometry.  KH_ERR_RANGE for larger k. */
int kh_export_dense_device(kh_ctx *ctx, uint64_t *d_dense, uint64_t n_entries);
int kh_merge_dense_device(kh_ctx *ctx, const uint64_t *d_dense, uint64_t n_entries, uint32_t owner, uint32_t nparts);

/* Generic path (any number of shards, tables of any size): pairs grouped by owner, then
 * kh_merge_pairs_device re-inserts them with device atomics. */
/* kh_export_by_owner_device: compact all live (key,count) pairs grouped by owner shard into device arrays
 * of capacity cap; part_counts[p] (host array, nparts entries) receives the
 * number of pairs for shard p; pairs of shard p start at sum(part_counts[0..p)). */
int kh_export_by_owner_device(kh_ctx *ctx, uint32_t nparts, uint64_t *d_keys,
                              uint64_t *d_counts, uint64_t cap, uint64_t *part_counts);
/* count[key] += counts[i] for n device-resident / host-resident pairs. */
int kh_merge_pairs_device(kh_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_counts, uint64_t n);
int kh_merge_pairs(kh_ctx *ctx, const uint64_t *keys, const uint64_t *counts, uint64_t n);

/* ---- the exchange itself, behind this ABI (RCCL over xGMI) --------------- */
/* north_star: "reads shard naturally per GPU ... with a final RCCL reduce of per-GPU hash tables over xGMI".
 * The reference's only parallelism is rayon over records (src/run.rs:500-503); these calls are what stands
 * in for it at N > 1 GPUs, so that a host (Rust, C++) needs nothing but this library:
 *
 *   rank 0:        kh_comm_unique_id(&id);   ... the host hands the 128 bytes to every rank (any means) ...
 *   every rank r:  kh_create(&ctx, &cfg) on its own device;   kh_comm_init(ctx, nranks, r, &id);
 *                  kh_push*(ctx, its share of the reads) ...;     kh_merge_across(ctx, &info);
 *                  kh_result_* / kh_histogram / kh_lookup         -> the keys with kh_owner(key, k, nranks) == r
 *
 * kh_merge_across is a COLLECTIVE: every rank of the communicator calls it, once per merge.  It picks, by a
 * vote among the ranks, the narrowest exchange unit every table can represent (32-bit heads, packed u64,
 * 16-byte pairs; dense counts + one all-reduce for 2k <= 26), sends every owner its region segments with
 * ncclSend / ncclRecv groups on an own stream -- in KMERHIP_MERGE_PIECES (default 4) pieces, so that the
 * export of piece i + 1 and the LDS merge of piece i - 1 overlap the transfer of piece i -- and leaves this
 * context holding its hash-range shard (kh_set_shard state; kh_reset makes it a full table again).
 * Ranks need not arrive with tables of one size (each is sized from its own input): the merge starts with a gather
 * of the sizes, and a rank whose table is smaller than the largest re-lays it out to that size first.
 * One rank per context; ranks may be processes (one per GPU) or threads of one process (kh_group_*).
 *
 * Failure is collective too.  Every small all-gather of the sequence carries each rank's status, no transfer starts
 * before such a gather has come back clean, and one more closes the merge: a rank that fails on its own (out of
 * memory for a receive buffer, a kernel error) returns its status, EVERY other rank returns KH_ERR_PEER from the same
 * call -- nobody is left waiting.  That includes a rank whose context is unusable when it arrives (poisoned by an earlier
 * error, or the counting its last kh_push left pending fails now): it still joins the first gather and reports there.
 * Refused BEFORE the collective starts, on the calling rank alone: a dead communicator, and a table that is already a
 * shard (a finished merge leaves every rank one, so that refusal is collective by itself).  Every wait is bounded by KMERHIP_MERGE_TIMEOUT_S (default 300 s): on expiry, or on
 * an asynchronous RCCL error, the communicator is aborted (ncclCommAbort) and the call returns KH_ERR_RCCL; that
 * context's communicator is dead afterwards (kh_merge_across refuses it; make a new context and communicator).
 * After any failed merge the table's content is unspecified until kh_reset.
 * ONE RANK (a communicator of one, or no communicator at all): shard 0 of 1 is the whole hash range, so the context is left a
 * FULL table with the content it had -- kh_push*, kh_graph_*, kh_unitigs_* and a further kh_merge_across are accepted as
 * before, nothing is refused. */
typedef struct kh_unique_id { char internal[128]; } kh_unique_id;  /* ncclUniqueId, opaque */
int kh_comm_unique_id(kh_unique_id *out);
/* Collective over all ranks (it blocks until every rank has called it).  The context must be on the GPU this
 * rank uses; a context has at most one communicator (KH_ERR_STATE otherwise); kh_destroy releases it. */
int kh_comm_init(kh_ctx *ctx, uint32_t nranks, uint32_t rank, const kh_unique_id *id);

#define KH_ROUTE_NONE 0           /* single rank: nothing to exchange */
#define KH_ROUTE_DENSE 1          /* 2k <= 26: dense 4^k counts, one all-reduce(sum) */
#define KH_ROUTE_REGIONS_HEADS 2  /* region-ordered 32-bit heads */
#define KH_ROUTE_REGIONS_PACKED 3 /* region-ordered packed u64 */
#define KH_ROUTE_REGIONS_WIDE 4   /* region-ordered (u64 key, u64 count) */
#define KH_ROUTE_PAIRS 5          /* owner-grouped pairs, device-atomic re-insert (any world size / table sizes) */
typedef struct kh_merge_info {
    uint32_t route;           /* KH_ROUTE_* */
    uint32_t pieces;          /* pipeline pieces used (1 = one shot) */
    uint32_t unit_bytes;      /* bytes per exchanged unit */
    uint32_t nranks;
    uint64_t local_distinct;  /* entries of this rank's table before the merge */
    uint64_t sent_units;      /* units that left this rank (its own share excluded) */
    uint64_t recv_units;      /* units this rank merged (its own share included) */
    uint64_t owned_distinct;  /* entries of this rank's shard after the merge */
    double   export_ms;       /* host wall time in the export calls */
    double   wait_ms;         /* host wall time waiting for transfers / small collectives */
    double   merge_ms;        /* host wall time in the merge calls */
    double   total_ms;
    /* conservation (round 5): the merge checks itself.  Every sender digests what it exports per destination (units, sum of
     * the counts they carry, a wrapping checksum of the unit words), the digests travel with the small gathers, every receiver
     * digests what ARRIVED per source and the merge kernels add up the counts they put into the shard: any difference fails
     * the merge on every rank (KH_ERR_RCCL on the rank that saw it, KH_ERR_PEER on the others) -- a transport that loses
     * half a message, or a merge kernel that drops a unit, cannot produce a quietly smaller table. */
    uint32_t nranks_seen;      /* ranks the TRANSPORT reports (ncclCommCount; the process-local hub's size): == nranks */
    uint32_t conserved;        /* 1: every check above held on this rank (always 1 when the call returned KH_OK) */
    uint64_t sent_count_sum;   /* sum of the counts of all units this rank exported (its own share included) */
    uint64_t merged_count_sum; /* sum of the counts this rank's merge put into its shard == occurrences it now holds */
} kh_merge_info;
int kh_merge_across(kh_ctx *ctx, kh_merge_info *info /* may be NULL */);

/* Single-process form: one context per device and one host thread per context inside the library
 * ("internal HIP streams / one host thread per GPU").  devices[i] = HIP ordinal of rank i.
 * Distinct devices talk RCCL (xGMI); a device listed more than once (tests on a 1-GPU box; RCCL refuses
 * duplicate devices) makes the whole group exchange by device-to-device copies inside the process instead.
 * cfg->device and cfg->stream are ignored (every context owns its stream).  The contexts belong to the
 * group: use them with every kh_* call, but destroy them only through kh_group_destroy. */
typedef struct kh_group kh_group;
int kh_group_create(kh_group **out, const kh_config *cfg, const int32_t *devices, uint32_t ndevices);
kh_ctx *kh_group_ctx(kh_group *g, uint32_t rank);
uint32_t kh_group_size(const kh_group *g);
/* kh_merge_across on every context, each on its own host thread; infos: ndevices entries or NULL.
 * Returns KH_OK, else the status of a rank that failed itself (before any peer's KH_ERR_PEER). */
int kh_group_merge(kh_group *g, kh_merge_info *infos);
void kh_group_destroy(kh_group *g);

/* ---- pure helpers (host, no device) ------------------------------------- */
/* pack_bytes / Kmer::pack, src/kmer.rs:304-312,467-471.  KH_ERR_BAD_ARG if a
 * byte is outside ACGTacgt (*err_pos, if given, = its position: kmer.rs:277-280). */
int kh_pack(const uint8_t *bases, uint32_t k, uint64_t *packed, uint32_t *err_pos);
/* unpack_to_bytes, src/kmer.rs:431-440; writes k bytes (no terminator). */
int kh_unpack(uint64_t packed, uint32_t k, uint8_t *out);
/* canonical form of a packed k-mer, src/kmer.rs:348-390; *is_rc optional. */
int kh_canonical(uint64_t packed, uint32_t k, uint64_t *canonical, int *is_rc);

/* ---- diagnostics -------------------------------------------------------- */
const char *kh_strerror(int status);
/* Text of the last failure on this context (HIP error string etc.). */
const char *kh_last_error(const kh_ctx *ctx);
int kh_abi_version(void);

/* ---- deterministic synthetic reads (bench / tests) -------- */
/* Writes reads [first_read, first_read+n_reads) as stride-(read_len+1) records
 * (read_len bases then '\n') into device buffers of n_reads*(read_len+1) bytes.
 * d_qual may be NULL.  Launches on `stream` (hipStream_t or NULL) of `device`. */
int kh_synth_reads_device(int device, void *stream, uint64_t seed, uint64_t genome_len,
                          uint32_t read_len, uint64_t first_read, uint64_t n_reads,
                          uint8_t *d_bases, uint8_t *d_qual);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* KMERHIP_H */

// ctx.hip.h -- what the translation units behind include/kmerhip.h share: the context, its constants and knobs, and the
// helpers one unit defines for the others.
//
//   kmerhip.hip   life cycle, enter(), table management (lazy allocation, growth, the 8-byte image), a call's scratch, results, host memory, pure helpers
//   batch.hip     counting one device-resident range: the direct path and the partitioned batch (level 1 -> level 2 -> regions)
//   input.hip     kh_push* / kh_push_text*: staging, device accumulation, record scanning
//   merge.hip     exports and merges of one context (pairs, dense, region-ordered)
//   format.hip    kh_result_text_*: the table formatted as text on the device and streamed out in pieces
//   profile.hip   kh_profile*: the table's count at every window start of new sequences; the chunk pipeline and launch plan of every read-side call
//   join.hip      kh_compare / kh_combine_into: one table scanned, another probed, statistics or a third table out
//   graph.hip     kh_graph_stats / kh_graph_masks*: the table against itself, eight probes per k-mer, its de Bruijn degrees out
//   unitig.hip    kh_unitigs_*: the maximal non-branching paths of that graph (link rule, chain ranking by pointer doubling, emitter, links between them)
//   unitig_text.hip  kh_unitigs_text_*: those unitigs and links as FASTA / GFA text, formatted on the device and streamed out in pieces
//   locate.hip    kh_unitigs_locate*: where on those unitigs the k-mer of every window start of new sequences lies (the place map)
//   paths.hip     kh_unitigs_paths*: those places folded per record into runs along one unitig, and the coverage per unitig
//   support.hip   kh_unitigs_link_support*: how many of those records walk every link between the unitigs (the link index)
//   components.hip  kh_unitigs_components*: which unitigs hang together (hook and compress over the link array, sums per component); its
//                 labelling and decide launches also serve kh_drop_components_into, the third rule of unitig.hip's clip_step()
//   sort.hip      kh_result_sorted*: the result pairs in ascending key order (a device radix sort; format.hip streams it as text)
//   exchange.hip  kh_comm_* / kh_merge_across / kh_group_*: the exchange between contexts (RCCL over xGMI, or the local hub)
//   level1_*.hip  the level-1 kernels, one instance per k
//
// Two things every unit does the same way, declared once below: a call ENTERS the context through enter() with one of the named
// Entry presets (ENTER_WRITE, ENTER_READ, ...: what is counted, widened, cleared and ended on the way in), and device memory that
// lives for one call is a CallScratch, whose destructor is its only release.
//
// Everything here is hidden: the library is built with -fvisibility=hidden and linked with kmerhip.map, so it exports the kh_*
// entry points of include/kmerhip.h only (tests/test_abi.py holds `nm -D` to that list).
#pragma once
#include "../../include/kmerhip.h"

#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "alloc_inject.h"
#include "kernels.hip.h"
#include "partition.hip.h"

using kh::Counters;
using kh::Slot;
using kh::u64;

namespace khi __attribute__((visibility("hidden"))) {

constexpr double LOAD_HARD = 0.80;    // never let distinct exceed this fraction of capacity
constexpr double LOAD_TARGET = 0.50;  // load right after a growth
constexpr double HINT_LOAD = 0.65;    // a capacity hint of n keys gets the smallest table that holds them at this load
constexpr u64 MIN_CAP = 8ull * kh::REGION_SLOTS;
constexpr u64 DEFAULT_CAP = 1ull << 20;
constexpr u64 SUB_TILES = 1ull << 16;      // tiles per count launch (2^28 positions)
constexpr u64 SUB_TILES_MIN = 1ull << 10;  // smallest launch when squeezing under LOAD_HARD
constexpr u64 STAGE_BYTES = 64ull << 20;   // host staging chunk for kh_push
constexpr u64 ACC_MAX = 8ull << 30;        // device accumulation buffer of kh_push (x2, x2 with qualities): an upper limit --
                                           // acc_limit() also keeps the buffers within a quarter of the free memory.  (Round 2: 2 GiB,
                                           // i.e. 8 partitioned batches per S100M, each non-fresh region pass re-reading and re-writing
                                           // the whole 34 GB table: 177 ms of kernels against 74 resident.  8 GiB: two batches.)
constexpr u64 ACC_MIN = 1ull << 20;
constexpr u64 HALO = 32;                   // >= k-1 bytes re-sent in front of every staged chunk
constexpr int GRID_CAP = 256 * 8;          // 256 CUs x 8 resident workgroups of 256 threads: the most workgroups a scanning kernel is launched
                                           // with -- through grid_cap(), below the knobs; its grid-stride loop covers the rest
#ifndef KH_ARENA_UNITB
#define KH_ARENA_UNITB 128  // bytes per flushed unit of the arena level 2, 4-byte payloads (64: A/B builds)
#endif
#ifndef KH_PART_G1
#define KH_PART_G1 512
#endif
constexpr int PART_G1 = KH_PART_G1;               // level-1 workgroups (fixed: count and scatter must agree)
constexpr u64 PART_MIN_WINDOWS = 1ull << 22;   // below this the partition passes cannot pay off
constexpr double LOAD_PART = 0.70;         // grow before the next partitioned batch above this load
enum { ST_DIRECT = 0, ST_P1_COUNT, ST_P1_SCATTER, ST_P2_COUNT, ST_P2_SCATTER, ST_REGION, ST_MISC, ST_GROW, ST_N, ST_TEXT = ST_N };

struct Comm;  // exchange.hip: RCCL communicator (or the process-local hub) of this rank

// ---- environment knobs (round 4: ONE place) -----------------------------------------------------------------------------
// Read ONCE, at kh_create, into the context.  Two kinds:
//   * tunables of the product library: how much memory, how many threads, how long to wait, what to print, which insert path.
//     None of them can change a count.
//   * switches of the TEST build (-DKH_TESTING=1: krust_amd/lib/libkmerhip_testing.so, what tests/ load): force a kernel
//     variant, a table geometry, a fallback, an injected failure.  They exist so that every path can be driven against the
//     oracle; the product library does not compile them in -- there is no environment variable that makes it take an
//     ablation path or fail a merge.  (The test build also re-reads them at every call: tests flip them between batches.)
#ifndef KH_TESTING
#define KH_TESTING 0
#endif
struct Knobs {
    // product
    bool trace = false;              // KMERHIP_TRACE=1
    int path = 0;                    // KMERHIP_PATH=direct|partition: 1 | 2 (0: chosen per push)
    double part_budget_gb = 0;       // KMERHIP_PART_BUDGET_GB
    u64 acc_max_mb = 0;              // KMERHIP_ACC_MAX_MB
    u64 text_acc_mb = 0;             // KMERHIP_TEXT_ACC_MB
    int copy_threads = 0;            // KMERHIP_COPY_THREADS
    bool estimate = true;            // KMERHIP_ESTIMATE=0: size tables from the hint / the worst case, never from the level-1 sample
    bool pow2_table = false;         // KMERHIP_POW2_TABLE=1: tables of 2^n regions only (rounds 1-3's)
    // test build only
    int payload = 0;                 // KMERHIP_PAYLOAD=64
    u64 table_regions = 0;           // KMERHIP_TABLE_REGIONS
    int region_nt = 0;               // KMERHIP_REGION_NT
    bool p2_force_wide = false;      // KMERHIP_P2_FORCE_WIDE=1
    bool generic_k = false;          // KMERHIP_GENERIC_K=1
    bool p1_legacy = false;          // KMERHIP_P1_BINS=0
    bool p2_lines = true;            // KMERHIP_P2_LINES=0
    bool l2_arena = true;            // KMERHIP_L2_ARENA=0
    u64 l2_ovf_cap = ~0ull;          // KMERHIP_L2_OVF_CAP
    int l2_skew_x = -1;              // KMERHIP_L2_SKEW_X (-1: default 2)
    u64 l2_heavy_room = ~0ull;       // KMERHIP_L2_HEAVY_ROOM
    bool narrow = true;              // KMERHIP_NARROW=0
    bool l2_narrow = true;           // KMERHIP_L2_NARROW=0: level 2 never narrows 8-byte payloads to the 4 bytes below the region index
    bool l2_no_room_wide = false;    // KMERHIP_L2_NO_ROOM_WIDE=1: as if a batch sized for a narrowing level 2 had no room for 8-byte output (drives KH_RETRY_WIDE)
    u64 hot_cut = 0;                 // KMERHIP_HOT_CUT (0: default; ~0: no bucket is hot)
    int ovf_agg = -1;                // KMERHIP_OVF_AGG
    double survival = 0;             // KMERHIP_SURVIVAL
    bool heads_always = false;       // KMERHIP_HEADS_ALWAYS=1: every fresh pass leaves the exchange-head counts behind, communicator or not
    u64 table_room_mb = 0;           // KMERHIP_TABLE_ROOM_MB: what the sample-sized table may take, as if the device had no more
    bool stop_after_p1 = false, stop_after_p2 = false;  // ablation builds (KH_ABL*)
    u64 profile_chunk_kb = 0;        // KMERHIP_PROFILE_CHUNK_KB: window starts per chunk of kh_profile, in units of 1024 (0: sized from the call)
    u64 uni_text_chunk_kb = 0;       // KMERHIP_UNI_TEXT_CHUNK_KB: bytes per chunk of kh_unitigs_text_next*, in KiB, rounded up to whole tiles (0: up to 64 MiB)
    // KMERHIP_ALLOC_FAIL=n | n+, KMERHIP_ALLOC_TRACE=path: the n-th allocation through dev_malloc / pin_malloc (below) fails; every
    // allocation, release and injected failure is appended to a file.  Not fields: read at every allocation, one count per process.
    // KMERHIP_GRID_CAP: the most workgroups of a capped-grid launch (0 / unset: GRID_CAP).  Not a field: one value per process,
    // g_grid_cap below, which read_knobs sets -- and the context of the product library stays the size it was.
};
inline const char *env_of(const char *name) {
    const char *e = getenv(name);
    return (e && *e) ? e : nullptr;
}
void read_knobs(Knobs &k);

// The cap of every launch that covers its input with a grid-stride loop (grid_for() and the launches that size their own grid).
// The product library: the constant.  The test build: KMERHIP_GRID_CAP, so that a cap of 1 or 3 sends every workgroup round its
// loop many times at the sizes tests/ use (tests/test_gpu_grid_stride.py) -- one value per process, set by read_knobs (grid_for is
// a free function: the contexts of a process share it).  No kernel behind it waits for another workgroup.
#if KH_TESTING
extern std::atomic<int> g_grid_cap;  // (contexts on several threads re-read the switches: every one writes the same value)
inline int grid_cap() { return g_grid_cap.load(std::memory_order_relaxed); }
#else
constexpr int grid_cap() { return GRID_CAP; }
#endif

// Every device and pinned-host allocation and release of the library goes through these four.  The product library: forwards
// to the runtime and nothing else.  The test build: KMERHIP_ALLOC_FAIL=n makes the n-th allocation through them fail (n+: that
// one and every later one) -- hipErrorOutOfMemory without a call of the runtime, the pointer null; one 1-based count per
// process for both kinds, restarted whenever the variable's value changes (alloc_inject.h) -- and KMERHIP_ALLOC_TRACE=path
// appends one line per event to that file:  "A dev|pin <pointer> <bytes>"  an allocation that succeeded,  "F <pointer>"  a
// release,  "X <ordinal> dev|pin <bytes>"  an injected failure.  Both are read at every call (tests/test_gpu_alloc_fail.py).
#if KH_TESTING
bool alloc_inject_fails(const char *kind, size_t bytes);                  // kmerhip.hip
void alloc_trace_event(char ev, const char *kind, const void *p, size_t bytes);
inline hipError_t dev_malloc(void **p, size_t bytes) {
    if (alloc_inject_fails("dev", bytes)) { *p = nullptr; return hipErrorOutOfMemory; }
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) alloc_trace_event('A', "dev", *p, bytes);
    return e;
}
inline hipError_t pin_malloc(void **p, size_t bytes, unsigned flags) {
    if (alloc_inject_fails("pin", bytes)) { *p = nullptr; return hipErrorOutOfMemory; }
    const hipError_t e = hipHostMalloc(p, bytes, flags);
    if (e == hipSuccess) alloc_trace_event('A', "pin", *p, bytes);
    return e;
}
inline hipError_t dev_free(void *p) {
    if (p) alloc_trace_event('F', nullptr, p, 0);
    return hipFree(p);
}
inline hipError_t pin_free(void *p) {
    if (p) alloc_trace_event('F', nullptr, p, 0);
    return hipHostFree(p);
}
#else
inline hipError_t dev_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pin_malloc(void **p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
inline hipError_t dev_free(void *p) { return hipFree(p); }
inline hipError_t pin_free(void *p) { return hipHostFree(p); }
#endif

}  // namespace khi

struct kh_ctx {
    khi::Knobs knobs;
    int device = 0;
    khi::Comm *comm = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t k = 0;
    int32_t minq = -1;
    uint32_t flags = 0;
    bool trace = false;

    Slot *table = nullptr;
    u64 cap = 0;
    // The 8-byte image of the table (partition.hip.h, region_count_kernel32<.., NARROW>): count << 32 | 32-bit payload per
    // slot.  While `narrow` is set IT holds the counts and the 16-byte table is stale; ensure_wide() converts.  A fresh
    // partitioned pass with 32-bit payloads writes it, later such passes update it, kh_finish / kh_result_* / kh_histogram /
    // kh_lookup read it as it is; everything else (the direct path, growth, exports, merges) goes through enter(), which
    // widens first.
    u64 *ntab = nullptr;
    u64 ntab_cap = 0;
    bool narrow = false;
    bool narrow_banned = false;   // a count left 32 bits once: this table stays 16-byte until kh_reset
    kh::PartGeom narrow_g;        // the geometry the image's payloads are relative to
    Counters *d_ctr = nullptr;
    Counters *h_ctr = nullptr;  // pinned

    u64 distinct_known = 0;  // exact as of the last counter read-back
    u64 pending_bound = 0;   // upper bound on claims by launches since then
    u64 bases_pushed = 0;
    u64 grows = 0;
    u64 launches = 0;
    double kernel_ms = 0.0;
    double h2d_ms = 0.0;

    // ---- kh_push: pinned staging -> device accumulation buffers -> one count per filled buffer ----
    hipStream_t cstream = nullptr;             // copy stream (H2D overlaps counting on `stream`)
    uint8_t *h_stage[2] = {nullptr, nullptr};  // pinned: bases then qual, each stage_bytes
    u64 stage_bytes = 0;                       // 0 until pageable memory is pushed / fetched; then 1, 8 or 64 MiB (input.hip ensure_stage)
    hipEvent_t stage_done[2] = {nullptr, nullptr};
    bool stage_used[2] = {false, false};
    int stage_next = 0;
    uint8_t *acc[2] = {nullptr, nullptr};      // device: [HALO | bases acc_cap | pad][HALO | qual acc_cap | pad]
    u64 acc_cap = 0;                           // bytes of bases one accumulation buffer holds
    int acc_cur = 0;
    u64 acc_len = 0;                           // bytes accumulated in acc[acc_cur] (after the HALO head)
    u64 acc_carry = 0;                         // HALO bytes at the head are the tail of the previous buffer
    bool acc_qual = false;
    bool acc_has_qual = false;                 // the buffers were allocated with their quality halves
    hipEvent_t acc_free[2] = {nullptr, nullptr};
    bool acc_busy[2] = {false, false};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> h2d_events;

    // ---- partitioned path ----
    bool table_empty = true;   // no insert since creation / reset: regions need not be read back
    // kh_set_region_window: the next region-ordered exports / merges cover piece win_piece of win_n of
    // every owner's region range.  A FRESH merge done in pieces leaves the regions of the pieces not
    // yet merged unwritten (stale if the table was lazily reset): win_open / win_mask / win_dirty
    // track that until the last piece, or until anything else touches the table (close_fresh_window).
    uint32_t win_piece = 0, win_n = 1;
    bool win_open = false, win_dirty = false;
    uint32_t win_open_n = 0;
    u64 win_mask = 0;
    bool table_dirty = false;  // kh_reset is lazy: the slots hold stale data that the next operation either
                               // overwrites wholesale (a FRESH region pass) or clears first (everything else)
    bool hinted = false;       // caller gave a capacity hint
    u64 hint_keys = 0;         // ... of this many distinct k-mers
    double new_rate = -1.0;    // new keys per window of the last partitioned range (-1: none yet): sizes an unhinted table
    int path_mode = 0;         // 0 auto, 1 force direct, 2 force partitioned
    int pay_mode = 0;          // 0 auto, 64 = always 64-bit payloads (env KMERHIP_PAYLOAD=64, for A/B)
    uint32_t shard_shift = 0;  // table holds shard `shard_index` of 2^shard_shift (kh_set_shard)
    uint32_t shard_index = 0;
    u64 *merge_off = nullptr;  // scans of the senders' region counts (kh_merge_regions_device)
    u64 merge_off_cap = 0;
    u64 part_budget = 0;       // bytes for the two key buffers (0 = decide at first use)
    u64 prev_part_budget = 0;  // ... as it was when release_part_buffers gave them back
    uint8_t *keysA = nullptr, *keysB = nullptr;  // partition ping-pong buffers
    u64 key_cap = 0, keyb_cap = 0;  // bytes of keysA / keysB
    // Round 5: between the end of a count and the next kh_reset the two partition buffers are idle -- up to 0.8 of the device --
    // while a merge needs tens of GB of scratch AND the shard's 16-byte table.  Round 4 gave the buffers back to the driver
    // (release_part_buffers) and took them again at the next count: 370 ms of hipFree / hipMalloc per count-and-merge step
    // at configs[3]'s size (bench.py --force-merge).  Now the merge BORROWS from them: a bump allocator over keysA / keysB
    // (kmerhip.hip borrow()), for the exchange's send / receive buffers and for the table itself (table_borrowed).  The loan
    // ends with kh_reset, or when anything is about to write the partition buffers (end_borrow: a borrowed table moves out).
    bool exports_seen = false;       // a heads export was asked of this context: its fresh passes leave the head counts behind (batch.hip want_heads)
    bool borrow_on = false;
    u64 borrow_off[2] = {0, 0};     // bytes lent out of keysA / keysB
    bool table_borrowed = false;    // `table` points into keysA / keysB: never hipFree'd
    kh::Part2Block *blocks = nullptr;
    u64 blocks_cap = 0;
    u64 *moff = nullptr;
    uint32_t *nch = nullptr;
    u64 *info = nullptr;
    uint32_t *H2 = nullptr;
    u64 *O2 = nullptr;
    u64 h2_cap = 0;
    u64 *bstart = nullptr;
    uint8_t *rfail = nullptr;
    uint32_t *rnew = nullptr;
    u64 *rreal = nullptr;            // k-mers per bucket (its size minus the unit-padding sentinels)
    uint32_t *rheads = nullptr;      // exchange heads per region, left by a FRESH region pass
    bool rheads_valid = false;       // ... and still describing the table (nothing else touched it since)
    bool rheads_wide = false;
    uint32_t rheads_cb = 0;
    u64 *bend = nullptr;             // arena path: end of every region's data (the exact path uses bstart + 1)
    uint32_t *hot_list = nullptr;    // [regions] buckets left to hot_buckets_kernel (partition.hip.h)
    uint8_t *rtouch = nullptr;       // [regions] all zero between uses: the regions an overflow list touched (merge.hip recount_touched_heads)
    u64 *radd = nullptr;             // [regions] shard_merge_kernel: sum of the counts it put into every target region (conservation)
    u64 *rdig = nullptr;             // shard_merge_narrow_kernel: [target][sender][3] arrival-digest partials; region_compact_*: [region][2]
    u64 rdig_cap = 0;
    u64 *ptotal = nullptr;           // [MAX_P1] payloads per level-1 partition
    uint32_t *pcap = nullptr;        // [MAX_P1] arena capacity of that partition's buckets
    uint8_t *heavy = nullptr;        // [MAX_P1] the partition is too heavy for one workgroup: the exact kernels take it
    u64 *ovf = nullptr;              // [4] overflow list: entries handed out, "list full" flag; heavy partitions, payloads in them
    kh::OvfEntry *ovf_list = nullptr;
    u64 ovf_cap = 0;
    u64 ovf_pending = 0;             // entries of the overflow list still to be inserted (this batch)
    uint16_t *chunk_part = nullptr;  // chunk pool metadata (32-bit payload path)
    uint8_t *fill8 = nullptr;
    uint32_t *plist = nullptr;
    u64 pool_cap = 0;                // chunks the metadata arrays hold
    uint32_t *pcount = nullptr;      // [MAX_P1] chunks per partition, then cursors
    u64 *pstart = nullptr;           // [MAX_P1 + 1]
    u64 *pool_next = nullptr;
    u64 region_cap = 0;              // entries of EVERY [regions] array above: they grow together, ensure_region_scratch()
    u64 *scan_partial = nullptr;
    u64 scan_cap = 0;
    u64 *est_set = nullptr;          // scratch of distinct_sample_kernel (partition.hip.h): the set a few level-1 partitions are counted in
    u64 est_set_cap = 0;
    u64 est_keys = 0;                // distinct keys the current fresh range is expected to bring (from that sample; 0 = no estimate)
    bool sized_by_sample = false;    // the table's size comes from such a sample (stats / trace)
    bool narrow2_refused = false;    // a batch sized for a narrowing level 2 (15 B per window) could not narrow and had no room for 8-byte output: later ranges are sized for that
    bool estimate_on = true;         // KMERHIP_ESTIMATE=0: never (rounds 1-3's sizing: the hint, or the worst case)
    u64 part_batches = 0;
    double stage_ms[khi::ST_N] = {0};
    struct StageEv { int stage; hipEvent_t a, b; };
    std::vector<StageEv> stage_events;

    // ---- kh_push_text: device-side record scanning ----
    uint8_t *txt_raw2[2] = {nullptr, nullptr};  u64 txt_raw2_cap[2] = {0, 0};  // host text lands here (two: KH_FLAG_DEFER_TEXT_SCAN copies one while the other is scanned)
    int txt_raw_next = 0;
    hipStream_t sstream = nullptr;         // KH_FLAG_DEFER_TEXT_SCAN: the stream the scans run on, beside the copy stream
    hipEvent_t txt_copied[2] = {nullptr, nullptr};
    hipEvent_t txt_scanned[2] = {nullptr, nullptr};  // the scan kernels that read raw buffer r are done (recorded on the scan stream)
    bool txt_scanned_on[2] = {false, false};
    hipStream_t cstream2 = nullptr;        // a second copy stream: a large pinned text travels as two halves on two DMA engines
    struct { bool on = false; int r = 0; u64 n = 0; int format = 0; } txt_unscanned;  // a text on the device whose scan is still to come
    uint8_t *txt_acc[2] = {nullptr, nullptr};   u64 txt_acc_cap[2] = {0, 0};    // flat bases of the texts pushed, accumulated for the count kernels
    uint8_t *txt_accq[2] = {nullptr, nullptr};  u64 txt_accq_cap[2] = {0, 0};   // ... and their qualities
    int txt_cur = 0;                       // the buffer the scans append to
    u64 txt_acc_len = 0;                   // bytes accumulated there and not counted yet (a multiple of 16)
    bool txt_acc_qual = false;             // ... with qualities
    hipEvent_t txt_acc_done[2] = {nullptr, nullptr};  // the count of that buffer's last content (on `stream`)
    bool txt_acc_busy[2] = {false, false};
    hipStream_t txt_scan_stream = nullptr; // the stream the accumulated scans ran on
    u64 *txt_scan_partial = nullptr;  u64 txt_scan_cap = 0;  // scan scratch of the text stream
    u64 expect_bytes = 0;                  // kh_config::input_mib: what the caller expects to push in total (0 = unknown)
    u64 *txt_ls = nullptr;        u64 txt_ls_cap = 0;    // line starts
    uint8_t *txt_st = nullptr;    u64 txt_st_cap = 0;    // FASTA: line state behind each 1 KiB unit (rawparse.hip.h)
    uint32_t *txt_tnl = nullptr;  u64 txt_tnl_cap = 0;   // per-tile newline counts
    u64 *txt_tbase = nullptr;     u64 txt_tbase_cap = 0;
    uint32_t *txt_tkeep = nullptr; u64 txt_tkeep_cap = 0;
    u64 *txt_tout = nullptr;      u64 txt_tout_cap = 0;
    uint32_t *txt_err = nullptr;  u64 txt_err_cap = 0;
    struct TxtHost { u64 total; u64 end_mark; uint32_t err; uint8_t first, last; } *h_txt = nullptr;  // pinned
    double text_ms = 0.0;

    // ---- kh_result_text_*: the table as text, streamed in pieces (format.hip) ----
    // begin sizes every tile of FMT_TILE slots (records, bytes) and scans both; next formats ranges of whole tiles into one of two
    // device chunks -- the idle partition buffers where there are any, else small buffers of the stream's own -- and hands their text
    // out record-aligned: chunk i + 1 is formatted on `stream` while chunk i travels on `cstream`.  `on` falls with every call
    // that enters the context for anything but reading (enter(), Entry::reader).
    struct TextStream {
        bool on = false;
        uint32_t format = 0;
        u64 min_count = 0, ntiles = 0;
        u64 n_records = 0, rec_bytes = 0;  // totals; rec_bytes without the document tail
        u64 next_tile = 0;                 // first tile no chunk holds yet
        bool tail_done = false;
        std::vector<u64> toff;             // host copy of the tiles' byte offsets (ntiles + 1)
        struct Chunk {
            uint8_t *d = nullptr;
            u64 cap = 0, len = 0, pos = 0;  // bytes it can hold / holds / has handed out
            bool valid = false;
            hipEvent_t done = nullptr;      // its formatting kernel (on `stream`)
        } ch[2];
        int cur = 0;                       // the chunk being handed out
        bool sorted = false;               // KH_OUT_SORTED: the tiles are over ts_skey / ts_scnt (sorted_n pairs, ascending), not over the table
        u64 sorted_n = 0;
    } ts;
    uint8_t *ts_own[2] = {nullptr, nullptr};  u64 ts_own_cap[2] = {0, 0};  // chunks of the stream's own (no partition buffers to use)
    uint32_t *ts_trec = nullptr;  u64 ts_trec_cap = 0;   // per tile: records
    uint32_t *ts_tbyt = nullptr;  u64 ts_tbyt_cap = 0;   // per tile: bytes
    u64 *ts_roff = nullptr;       u64 ts_roff_cap = 0;   // exclusive scans of the two
    u64 *ts_boff = nullptr;       u64 ts_boff_cap = 0;
    u64 *ts_skey = nullptr;       u64 ts_skey_cap = 0;   // a sorted stream's pairs: the stream's own memory, never where its chunks live
    u64 *ts_scnt = nullptr;       u64 ts_scnt_cap = 0;

    // ---- the chunks of the four host forms of the read side (chunk_pipeline(), profile.hip) ----
    // two device buffers [bases | qualities | results or words] for pf_chunk window starts each, their pinned twins (the bounce of
    // pageable caller memory), and per buffer the events "input is on the device", "kernel done", "results are in host memory"
    uint8_t *pf_d[2] = {nullptr, nullptr};
    uint8_t *pf_h[2] = {nullptr, nullptr};
    u64 pf_chunk = 0;
    u64 pf_out_bytes = 0;  // bytes per window start of the buffers' last part: 4 (kh_profile, kh_profile_records) or 8 (kh_unitigs_locate, kh_unitigs_paths)
    hipEvent_t pf_in[2] = {nullptr, nullptr}, pf_run[2] = {nullptr, nullptr}, pf_out[2] = {nullptr, nullptr};
    // kh_profile_records: the rows (KH_REC_WORDS words per record) and the record offsets, on the device for the whole call
    uint32_t *pr_rows = nullptr;  u64 pr_rows_cap = 0;  // records
    u64 *pr_rec = nullptr;        u64 pr_rec_cap = 0;   // offsets
    // kh_compare / kh_combine_into (join.hip): the words the launching context's kernels add up -- KH_CMP_WORDS, then the pair count
    u64 *jn_words = nullptr;
    // kh_graph_stats (graph.hip): the KH_GRAPH_WORDS words its kernel adds up
    u64 *gr_words = nullptr;
    // kh_unitigs_* (unitig.hip): the rows, bases and links of the last kh_unitigs_begin[_linked], memory of the context's own until kh_unitigs_end /
    // the next begin / kh_reset / kh_destroy.  `live` falls with every call that enters for anything but reading (enter(), Entry::reader).
    struct Unitigs {
        bool live = false;
        u64 *rows = nullptr;      // KH_UNI_WORDS words per unitig
        uint8_t *bases = nullptr;
        u64 n_unitigs = 0, n_bases = 0;
        bool linked = false;      // built by kh_unitigs_begin_linked: the link words, one per (end state, successor)
        u64 *links = nullptr;     // (nullptr when there are none)
        u64 n_links = 0;
        // kh_unitigs_locate* (locate.hip): the place map, one word per table slot -- (2 u + o) << 32 | j for the node in that slot, all ones
        // for a slot that holds no node of S.  Built by the first locate call after a begin (cap * 8 bytes), released by unitigs_release().
        u64 *where = nullptr;
        // kh_unitigs_link_support* (support.hip): the link index, one word per end state -- the index of the first link out of it, all ones
        // for a state without links -- and behind them the KH_SUP_WORDS words the kernel adds up.  Built by the first support call after a
        // kh_unitigs_begin_linked ((2 * n_unitigs + KH_SUP_WORDS) * 8 bytes), released by unitigs_release().
        u64 *link_first = nullptr;
        // kh_unitigs_components* (components.hip): the labels.  One allocation, built by the first components call after a
        // kh_unitigs_begin_linked and released by unitigs_release(): n_comp rows of KH_COMP_WORDS words, then one uint32 per unitig
        // (32 bytes per component, 4 per unitig); the KH_CC_WORDS words of the build stay here in host memory.  comp_built also
        // stands for "no unitigs": then nothing is allocated.
        bool comp_built = false;
        u64 *comp_rows = nullptr;      // (the allocation)
        uint32_t *comp = nullptr;      // (behind the rows)
        u64 n_comp = 0;
        u64 cc[KH_CC_WORDS] = {0, 0, 0, 0};
        // kh_unitigs_text_* (unitig_text.hip): these unitigs as text.  begin sizes every record and link line and scans both; next formats
        // ranges of whole tiles of UT_TILE bytes into one of two device chunks of the stream's OWN -- never the partition buffers: a
        // kh_result_text_* stream may run beside it -- and hands their bytes out: chunk i + 1 is formatted on `stream` while chunk i
        // travels on `cstream`.  Running = live && text.on; unitigs_release() gives its memory back with the unitigs'.
        struct Text {
            bool on = false;
            uint32_t format = 0;
            u64 hdr = 0, rec_bytes = 0, link_bytes = 0, total = 0;  // the GFA header, the records, the link lines; their sum
            u64 *off = nullptr;                    // device: n_unitigs + 1 record offsets, then n_links + 1 link-line offsets (gfa with links only)
            u64 chunk_bytes = 0;                   // whole tiles
            u64 next_off = 0;                      // first byte of the document no chunk holds yet (a multiple of UT_TILE, or total)
            u64 sent = 0;                          // bytes handed out
            struct Chunk {
                uint8_t *d = nullptr;
                u64 len = 0, pos = 0;           // bytes it holds / has handed out
                bool valid = false;
                hipEvent_t done = nullptr;      // its formatting kernel (on `stream`)
            } ch[2];
            int cur = 0;                           // the chunk being handed out
        } text;
    } un;

    bool poisoned = false;
    int poisoned_by = KH_OK;  // the status that poisoned it: kh_reset lifts KH_ERR_OOM and KH_ERR_TABLE_FULL, never KH_ERR_HIP
    std::string last_error;
};

namespace khi __attribute__((visibility("hidden"))) {

inline int fail(kh_ctx *c, int code, const char *what, hipError_t e = hipSuccess) {
    if (c) {
        c->last_error = what;
        if (e != hipSuccess) {
            c->last_error += ": ";
            c->last_error += hipGetErrorString(e);
        }
        if (code == KH_ERR_HIP || code == KH_ERR_TABLE_FULL || code == KH_ERR_OOM) {
            if (!c->poisoned || code == KH_ERR_HIP) c->poisoned_by = code;  // (kh_reset lifts what no runtime error caused)
            c->poisoned = true;
        }
    }
    return code;
}
// KH_ERR_OOM of a READING call (include/kmerhip.h, "Allocation failures"): an allocation of this call alone failed, the table
// is untouched -- the error text names the allocation, and the context is not poisoned.
inline int soft_oom(kh_ctx *c, const char *what, hipError_t e = hipSuccess) {
    c->last_error = what;
    if (e != hipSuccess) {
        c->last_error += ": ";
        c->last_error += hipGetErrorString(e);
    }
    return KH_ERR_OOM;
}

#define HIP_TRY(c, call)                                              \
    do {                                                              \
        hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) return fail((c), KH_ERR_HIP, #call, e_); \
    } while (0)

inline int grid_for(u64 items) {
    u64 b = (items + kh::BLOCK - 1) / kh::BLOCK;
    if (b < 1) b = 1;
    if (b > (u64)grid_cap()) b = grid_cap();
    return (int)b;
}

// ---- kmerhip.hip -----------------------------------------------------------------------------------------------------------
// Every entry point starts with enter(): host pushes are accumulated on the device and counted lazily; anything that looks at
// the table first counts what is pending.  What a call needs of the context on its way in is an Entry: one of the presets
// below, or -- kh_set_shard, export_regions, merge_regions -- a preset with one field changed where the call is made.
struct Entry {
    bool flush_pending = true;  // what kh_push / kh_push_text left pending is counted first
    bool need_table = true;     // the 16-byte table exists and, if lazily reset, is cleared (unless the 8-byte image holds the counts)
    bool keep_window = false;   // a fresh merge in pieces (kh_set_region_window) stays open: this call merges its next piece
    bool narrow_ok = false;     // the 8-byte image stays what it is (false: widened into the 16-byte table first)
    bool reader = false;        // the call only reads the table: a text stream in progress and the unitigs of kh_unitigs_begin survive it
};
// Slot indices are stable for as long as un.live holds: only `reader` entries keep it, and both reader presets below set narrow_ok,
// so that enter() neither widens the image nor moves, grows or clears a table that holds counts (nothing is pending behind live
// unitigs: a push is no reader).  The place map of kh_unitigs_locate* (Unitigs::where) is indexed by slot and relies on it.
// The pair and dense merges, the exports by owner, kh_comm_init, the dst of kh_combine_into / kh_clip_tips_into / kh_pop_bubbles_into / kh_drop_components_into: a cleared
// 16-byte table, everything pending counted, whatever hangs on the table's content (text stream, unitigs, merge window) ended.
constexpr Entry ENTER_WRITE{};
// kh_finish, kh_result_size, kh_histogram, kh_lookup, kh_profile*, the sources of kh_compare / kh_combine_into, kh_graph_*,
// the copies of the unitigs, kh_result_text_begin: everything pending counted, the table in the form it is in, nothing ended.
constexpr Entry ENTER_READ{true, true, false, true, true};
// kh_result_copy*, kh_result_sorted*, kh_region_unit_counts_device, kh_unitigs_begin*, the src of kh_clip_tips_into / kh_pop_bubbles_into / kh_drop_components_into,
// kh_merge_across: reads the table in the form it is in, but may take the idle partition buffers -- a text stream, whose chunks
// live there, ends (and with it the unitigs).
constexpr Entry ENTER_READ_TAKE{true, true, false, true, false};
// kh_push, kh_push_text, kh_reset: touches no slot and counts nothing -- the push is accumulated beside what is pending, a lazily
// reset table stays lazily reset and one nobody has needed yet stays unallocated.
constexpr Entry ENTER_PUSH{false, false, false, true, false};
// kh_push_device, kh_push_text_device: as ENTER_PUSH, with what is pending counted first (the resident range is counted at once,
// behind it; the counting path decides by itself which form of the table it needs).
constexpr Entry ENTER_PUSH_DEVICE{true, false, false, true, false};
// kh_result_text_next*: the next piece of the stream that kh_result_text_begin sized -- nothing is counted, nothing ended.
constexpr Entry ENTER_TEXT_NEXT{false, false, false, true, true};
int enter(kh_ctx *c, Entry how = ENTER_WRITE);
// What kh_result_copy, kh_result_sorted and kh_result_sorted_device do first: enter, *n = 0, *need = the pairs with
// count >= min_count, KH_ERR_RANGE when that is more than cap.  (KH_OK with *need == 0: nothing to copy.)
int result_enter(kh_ctx *c, const void *keys, const void *counts, u64 cap, u64 min_count, uint64_t *n, uint64_t *need);
int need_table(kh_ctx *c);
void resize_empty_table(kh_ctx *c, u64 newcap);
int clear_if_dirty(kh_ctx *c);
int close_fresh_window(kh_ctx *c);
int ensure_wide(kh_ctx *c);
int sync_counters(kh_ctx *c);
u64 round_cap(double want);
kh::RegionGeom geom_of_cap(u64 cap);
bool cap_is_pow2(u64 cap);
kh::TableGeom table_geom(const kh_ctx *c, Slot *table, u64 cap);
int grow_to(kh_ctx *c, u64 newcap);
int ensure_room(kh_ctx *c, u64 bound, bool allow_shrink_hint, bool *want_smaller);
int drain_events(kh_ctx *c);
int ensure_region_scratch(kh_ctx *c, u64 nregions);  // every [regions] scratch array of the context, grown together
int release_part_buffers(kh_ctx *c);  // the two partition buffers back to the device (they come back with the next partitioned batch)
void *borrow(kh_ctx *c, u64 bytes);   // `bytes` of the idle partition buffers (nullptr: not lent out, or no room); never freed
u64 borrow_room(const kh_ctx *c);     // the largest single request borrow() could serve now
int end_borrow(kh_ctx *c);            // the partition buffers are about to be written (or freed): a borrowed table moves to memory of its own
void drop_table(kh_ctx *c);           // the 16-byte table is no longer needed: freed, unless it was borrowed
// Device memory for the length of one call.  Two ways to have some, both nullptr when there is none -- the caller says soft_oom()
// or fail(KH_ERR_OOM): take(), from the idle partition buffers when nothing is borrowed, else from borrow(), else fresh();
// fresh(), a new allocation of exactly `bytes`, whatever lies idle.  The destructor is the only place that gives anything back:
// it drains the context's stream if the call owns an allocation, frees, and ends the loans the call took.
struct CallScratch {
    kh_ctx *c;
    u64 loan0, loan1;
    bool lent = false;
    u64 used[2] = {0, 0};
    std::vector<void *> owned;
    explicit CallScratch(kh_ctx *ctx);
    ~CallScratch();
    CallScratch(const CallScratch &) = delete;
    CallScratch &operator=(const CallScratch &) = delete;
    void *take(u64 bytes);
    void *fresh(u64 bytes);
};
// soft: the context's scan scratch fails as a reading call's (ensure_buf).  scratch: device_scan_scratch(n) bytes of the caller's own to
// use instead -- the calls that promise to leave nothing allocated (sort.hip, unitig.hip) take them from their CallScratch.
int device_scan(kh_ctx *c, const uint32_t *in, u64 n, u64 *out, bool soft = false, u64 *scratch = nullptr);
inline u64 device_scan_scratch(u64 n) { return ((n + kh::SCAN_CHUNK - 1) / kh::SCAN_CHUNK + 2) * sizeof(u64); }
int zero_cursors(kh_ctx *c);
// the live pairs with count >= min_count into device arrays of capacity cap, in no particular order (what kh_result_copy_device
// does once it has entered the context): *n = pairs written; KH_ERR_RANGE when the table holds more than cap
int compact_pairs(kh_ctx *c, u64 *d_keys, u64 *d_counts, u64 cap, u64 min_count, u64 *n);
int read_cursor(kh_ctx *c, u64 *cursor, u64 *big);
int head_count_bits(const kh_ctx *c, u64 regions);
extern bool g_pow2_tables;
extern int g_copy_threads;
// ---- batch.hip
int count_device_range(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, u64 n, u64 wlo_off);
// ---- input.hip
int flush_acc(kh_ctx *c, bool carry);
int flush_text(kh_ctx *c);
int scan_unscanned(kh_ctx *c);
bool is_pinned_host(const void *p);
// The copy stream and, for need > 0, the two pinned staging buffers of 2 * stage_bytes each; soft: a reading call's KH_ERR_OOM.
int ensure_stage(kh_ctx *c, u64 need, bool soft);
void staged_memcpy(void *dst, const void *src, size_t n);  // several threads for a large copy
// ready: the event behind which d_src is complete (nullptr: it was produced on the compute stream, which is then drained)
int d2h_staged(kh_ctx *c, void *dst, const void *d_src, u64 bytes, hipEvent_t ready = nullptr);
// ---- merge.hip
enum { XF_WIDE = 0, XF_PACKED64 = 1, XF_HEADS32 = 2 };  // exchange unit formats (shard.hip.h)
int mark_touched_regions(kh_ctx *c, const void *ovf_list, const u64 *d_ovf, u64 ovf_lim);  // (batch.hip: before the overflow list's insert ...
int recount_touched_heads(kh_ctx *c, u64 nregions);                                           //  ... and after it)
// d_digest (optional; 3 x nparts u64 on the device): where the compaction can digest what it writes on the way (packed pairs / heads out
// of the 8-byte image), the sender's digests of exchange.hip are left there and *digest_done is set; otherwise the caller digests.
int export_regions(kh_ctx *c, int fmt, uint32_t nparts, void *d_keys, uint64_t *d_counts, uint64_t cap, uint32_t *d_region_counts,
                   uint64_t region_cap, uint64_t *part_counts, uint64_t *table_regions, u64 *d_digest = nullptr, bool *digest_done = nullptr);
// d_digest (optional; 3 x nsenders u64 on the device): where the merge kernel can digest what it reads on the way (the shard built as
// the 8-byte image), the arrival digests of exchange.hip are written there and *digest_done is set; otherwise the caller digests.
int merge_regions(kh_ctx *c, int fmt, uint32_t nsenders, uint64_t sender_regions, const void *const *d_keys,
                  const uint64_t *const *d_counts, const uint32_t *const *d_region_counts, u64 *d_digest = nullptr, bool *digest_done = nullptr);
// ---- exchange.hip
void comm_release(kh_ctx *c);
// ---- format.hip
void text_release(kh_ctx *c);  // kh_destroy: the text stream's buffers and events
// ---- sort.hip
int sorted_into(kh_ctx *c, u64 *out_keys, u64 *out_counts, u64 n, u64 min_count, CallScratch &sc);
// ---- join.hip
// What the table-against-table calls refuse before they enter anything (b, dst may be nullptr): `err` takes the text.
int join_check(kh_ctx *err, const char *who, const kh_ctx *a, const kh_ctx *b, const kh_ctx *dst);
// ---- unitig.hip
void unitigs_release(kh_ctx *c);  // kh_unitigs_end / kh_reset / kh_destroy: the rows, bases and links of the last kh_unitigs_begin[_linked]
inline unsigned uni_grid(u64 items) { return (unsigned)grid_for(items); }  // every launch of unitig.hip and unitig_text.hip: KMERHIP_GRID_CAP applies
// ---- components.hip
// What kh_unitigs_components* and the drop rule of clip_step() share.  The unitigs and links are c->un's; everything is queued on
// c->stream.  parent: n_unitigs words, sums: KH_CSUM_WORDS words per unitig (only a root's are meaningful), d_flag: one word --
// all scratch of the caller.  components_label leaves parent[u] = the smallest unitig index of u's component and the sums of every
// root, and drains the stream once per hooking round; *rounds = the rounds it ran.  components_drop_launch queues the decide kernel
// of kh_drop_components_into: removed[u] and seven of the KH_DROP_WORDS words (added to `words`, which the caller has zeroed).
constexpr u64 KH_CSUM_WORDS = 3;  // UNITIGS, KMERS, COUNT_SUM of the root's component
// before_sums (optional): called between the last round and the sums' launch (the trace's event).
int components_label(kh_ctx *c, uint32_t *parent, u64 *sums, uint32_t *d_flag, u64 *rounds, const std::function<void()> &before_sums = nullptr);
int components_drop_launch(kh_ctx *c, const uint32_t *parent, const u64 *sums, const u64 *loff, u64 min_kmers, uint8_t *removed, u64 *words);
// ---- unitig_text.hip
void unitigs_text_release(kh_ctx *c);  // the offsets, chunks and events of a kh_unitigs_text_* stream (unitigs_release calls it)
// ---- profile.hip
void profile_release(kh_ctx *c);  // kh_destroy: the chunk buffers and events of the host forms, the rows of kh_profile_records
// The chunks of a host form that streams a flat buffer through the device (kh_profile, kh_profile_records, kh_unitigs_locate,
// kh_unitigs_paths): window starts per chunk, sized from the call (KMERHIP_PROFILE_CHUNK_KB in the test build), and the two device
// buffers [bases | qualities | out_bytes per window start] with their pinned twins and events.  who: the call, for the error text.
constexpr u64 PF_PAD = 64;  // behind a chunk's bases: its k - 1 bytes of the next chunk, and the kernel's 16-byte loads
inline u64 pf_in_stride(u64 chunk) { return (chunk + PF_PAD + 15) & ~15ull; }
u64 profile_chunk(const kh_ctx *c, u64 n);
int profile_buffers(kh_ctx *c, u64 chunk, u64 out_bytes = 4, const char *who = "kh_profile: chunk buffers");
// One chunk of chunk_pipeline(), as its launch sees it: chunk j owns the ns window starts from a; len bytes lie at d_bases (and at
// d_qual, nullptr without a quality filter) from window start a on -- from a - 1 with a halo, except in front of the call's first;
// d_tail: the buffer's last part, behind the bases and qualities.
struct ChunkJob {
    u64 j, a, ns;
    const uint8_t *d_bases, *d_qual;
    u64 len;
    uint8_t *d_tail;
};
// The pipeline of all four host forms: n bytes of a flat host buffer in chunks of `chunk` window starts through the two buffers of
// profile_buffers() (which the caller has called), launch(job) per chunk on the compute stream.  Chunk j is sent the bytes its
// window starts need: its own and the k - 1 after them, with halo = 1 also one window start in front and one behind.  out: out_bytes
// per window start come back from d_tail, on a stream of their own beside the kernel of chunk j + 1; nullptr: nothing comes back,
// and the loop keeps one kernel ahead of the host.  Pinned caller memory is copied from and to directly, pageable memory through
// the pinned twins.  The first failing step returns, with whatever is queued left in flight.
int chunk_pipeline(kh_ctx *c, const uint8_t *bases, const uint8_t *qual, u64 n, u64 chunk, u64 halo, void *out, u64 out_bytes,
                   const std::function<int(const ChunkJob &)> &launch);
// Whether a call filters by quality (qualities given and a threshold set), and the byte it compares with then: minq + 33,
// saturating at 255 (saturating_add(33) on u8, run.rs:538).
inline bool qual_filter(const kh_ctx *c, const void *qual, uint32_t *thr = nullptr) {
    const bool on = qual != nullptr && c->minq >= 0;
    if (thr) *thr = on ? (uint32_t)std::min(c->minq + 33, 255) : 0u;
    return on;
}
// The launch of a read-side kernel (profile_kernel, profile_records_kernel, locate_kernel) over the window starts i < nout of n
// device-resident bytes: the data in virtual positions [vbeg, vend) over the 16-byte-aligned abase (qbase: the same coordinates;
// nullptr, 0, 0 without a quality filter), tiles of kh::TILE positions, tpb contiguous ones per workgroup (the look-back is carried
// in LDS), at most grid_cap() workgroups.  The window that starts at entry i ends at position vbeg + i + k - 1.
struct ReadPlan {
    const uint8_t *abase, *qbase;
    int qaligned;
    u64 vbeg, vend, ntiles;
    uint32_t tpb, thr;
    unsigned blocks;
};
ReadPlan read_plan(const kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, u64 n, u64 nout);
// What the record forms hold rec_start to (host memory): ascending, no record of 2^32 or more window starts, the last end within n.
int check_rec_start(kh_ctx *c, const char *who, const u64 *rec_start, u64 nrec, u64 n);
// ---- locate.hip
// The end of what kh_unitigs_locate* and kh_unitigs_paths* do before they touch anything: enter for reading, the unitigs live.
int enter_unitigs(kh_ctx *c, const char *who);
// (the place map is released by unitigs_release(): it is memory of the unitigs)
// The place map of the live unitigs (Unitigs::where), built if no call has built it since their begin; on any failure nothing of it
// stays and the status is a reading call's.  who: the call, for the error text.
int locate_index(kh_ctx *c, const char *who);
// The word of every window start i < nout of the n device-resident bytes -> d_out[i] (8-byte aligned); needs the place map;
// asynchronous on the compute stream.  paths.hip runs it per chunk.
int locate_range(kh_ctx *c, const uint8_t *d_bases, const uint8_t *d_qual, u64 n, u64 nout, u64 *d_out);

// ---- stage timing: HIP events on the launch stream, resolved lazily ---------------------------
struct StageTimer {
    kh_ctx *c;
    int stage;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st_stream;
    StageTimer(kh_ctx *ctx, int st, hipStream_t s = nullptr) : c(ctx), stage(st), st_stream(s ? s : ctx->stream) {
        if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, st_stream);
    }
    void stop() {
        if (a && b) {
            (void)hipEventRecord(b, st_stream);
            c->stage_events.push_back({stage, a, b});
            a = b = nullptr;
        }
    }
    ~StageTimer() { stop(); }
};

// ---- device scratch management for the partitioned path --------------------------------------
inline double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// soft: the non-poisoning form, for the scratch a reading call keeps in the context -- KH_ERR_OOM through soft_oom()
template <typename T>
int ensure_buf(kh_ctx *c, T **ptr, u64 *cap, u64 need, const char *what, bool soft = false) {
    if (*cap >= need && *ptr) return KH_OK;
    const double t0 = c->trace ? wall_ms() : 0.0;
    struct Tr {
        kh_ctx *c; double t0; const char *what; u64 bytes;
        ~Tr() { if (c->trace && wall_ms() - t0 > 5.0) fprintf(stderr, "[kmerhip] %s: %.1f MB took %.1f ms\n", what, (double)bytes / 1e6, wall_ms() - t0); }
    } tr{c, t0, what, need * sizeof(T)};
    if (*ptr) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        (void)dev_free(*ptr);
        *ptr = nullptr;
        *cap = 0;
    }
    hipError_t e = dev_malloc((void **)ptr, need * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *ptr = nullptr;
        return soft ? soft_oom(c, what, e) : fail(c, KH_ERR_OOM, what, e);
    }
    *cap = need;
    return KH_OK;
}

// Two-level split of the region index.  use32 = the 32-bit payload format applies (the hash bits
// left after level 1 fit in 32).  ok = false when the table is too large for two levels.
struct GeomChoice {
    kh::PartGeom g;
    bool use32;
    bool ok;
};

GeomChoice make_geom(const kh_ctx *c, u64 cap);

}  // namespace khi

//! Rust binding of `include/kmerhip.h` (C ABI of the MI355X k-mer counter).
//!
//! **Source only** -- never compiled in this repository's build image (no rustc).  It is the
//! binding a krust maintainer would add behind a cargo feature: [`HipKmerMap`] stands where
//! `KmerMap` stands in `src/run.rs:491-583`, [`KmerCounter`] mirrors the fluent builder of
//! `src/builder.rs:95-526` for the packed / string / histogram results.
#![allow(clippy::missing_errors_doc)]

use std::collections::{BTreeMap, HashMap};
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

use bytes::Bytes;

pub mod sys {
    use super::{c_char, c_int, c_void};

    #[repr(C)]
    pub struct KhConfig {
        pub struct_size: u32,
        pub k: u32,
        pub min_quality: i32, // -1 = None
        pub device: i32,      // -1 = current
        pub capacity_hint: u64,
        pub stream: *mut c_void,
        pub flags: u32,
        pub input_mib: u32,
    }

    #[repr(C)]
    #[derive(Default, Debug, Clone, Copy)]
    pub struct KhStats {
        pub bases: u64,
        pub kmers: u64,
        pub distinct: u64,
        pub table_slots: u64,
        pub grows: u64,
        pub launches: u64,
        pub count_kernel_ms: f64,
        pub h2d_ms: f64,
        pub part_batches: u64,
        pub stage_ms: [f64; 8],
        pub text_scan_ms: f64,
        pub slot_bytes: u64,
    }

    #[repr(C)]
    pub struct KhCtx {
        _private: [u8; 0],
    }

    /// ncclUniqueId (opaque): names one communicator; rank 0 makes it, every rank gets a copy.
    #[repr(C)]
    #[derive(Clone, Copy)]
    pub struct KhUniqueId {
        pub internal: [c_char; 128],
    }

    /// What one rank's `kh_merge_across` did.
    #[repr(C)]
    #[derive(Default, Debug, Clone, Copy)]
    pub struct KhMergeInfo {
        pub route: u32,
        pub pieces: u32,
        pub unit_bytes: u32,
        pub nranks: u32,
        pub local_distinct: u64,
        pub sent_units: u64,
        pub recv_units: u64,
        pub owned_distinct: u64,
        pub export_ms: f64,
        pub wait_ms: f64,
        pub merge_ms: f64,
        pub total_ms: f64,
        pub nranks_seen: u32,
        pub conserved: u32,
        pub sent_count_sum: u64,
        pub merged_count_sum: u64,
    }

    #[repr(C)]
    pub struct KhGroup {
        _private: [u8; 0],
    }

    extern "C" {
        pub fn kh_abi_version() -> c_int;
        pub fn kh_create(out: *mut *mut KhCtx, cfg: *const KhConfig) -> c_int;
        pub fn kh_destroy(ctx: *mut KhCtx);
        pub fn kh_reset(ctx: *mut KhCtx) -> c_int;
        pub fn kh_push(ctx: *mut KhCtx, bases: *const u8, qual: *const u8, n: u64) -> c_int;
        /// format: 1 = FASTA, 2 = FASTQ; -9 (KH_ERR_FORMAT) = parse on the host instead
        pub fn kh_push_text(ctx: *mut KhCtx, text: *const u8, n: u64, format: c_int) -> c_int;
        pub fn kh_finish(ctx: *mut KhCtx, stats: *mut KhStats) -> c_int;
        pub fn kh_result_size(ctx: *mut KhCtx, min_count: u64, n: *mut u64) -> c_int;
        pub fn kh_result_copy(ctx: *mut KhCtx, keys: *mut u64, counts: *mut u64, cap: u64,
                              min_count: u64, n: *mut u64) -> c_int;
        pub fn kh_histogram(ctx: *mut KhCtx, min_count: u64, count: *mut u64, freq: *mut u64,
                            cap: u64, n: *mut u64) -> c_int;
        pub fn kh_lookup(ctx: *mut KhCtx, keys: *const u64, n: u64, counts: *mut u64) -> c_int;
        /// per-base abundance: out[i] = the table's count of the k-mer that starts at byte i (saturated at 0xFFFF_FFFE),
        /// 0xFFFF_FFFF (KH_PROFILE_NO_WINDOW) where counting would see no window; reads the table only
        pub fn kh_profile_device(ctx: *mut KhCtx, d_bases: *const u8, d_qual: *const u8, n: u64, d_out: *mut u32) -> c_int;
        pub fn kh_profile(ctx: *mut KhCtx, bases: *const u8, qual: *const u8, n: u64, out: *mut u32) -> c_int;
        /// the profile reduced per record on the device: `rec_start` has `nrec + 1` ascending offsets, row `r` (8 `u32`) is the
        /// reduction over the window starts `rec_start[r] .. rec_start[r+1]` (KH_REC_* of the header name the words)
        pub fn kh_profile_records_device(ctx: *mut KhCtx, d_bases: *const u8, d_qual: *const u8, n: u64, d_rec_start: *const u64,
                                         nrec: u64, lo: u32, hi: u32, d_rows: *mut u32) -> c_int;
        pub fn kh_profile_records(ctx: *mut KhCtx, bases: *const u8, qual: *const u8, n: u64, rec_start: *const u64, nrec: u64,
                                  lo: u32, hi: u32, rows: *mut u32) -> c_int;
        /// two tables against each other, both only read: `out` takes the 8 words KH_CMP_* of the header names (distinct_a,
        /// distinct_b, shared, sum_a, sum_b, shared_sum_a, shared_sum_b, sum_min); a key counts from `max(min, 1)` on
        pub fn kh_compare(a: *mut KhCtx, b: *mut KhCtx, min_a: u64, min_b: u64, out: *mut u64) -> c_int;
        /// `count[key] += c` in `dst` for the pairs of a set operation of `a` and `b` (op: KH_SET_*, calc: KH_CALC_*)
        pub fn kh_combine_into(dst: *mut KhCtx, a: *mut KhCtx, b: *mut KhCtx, op: u32, calc: u32, min_a: u64, min_b: u64,
                               n_pairs: *mut u64) -> c_int;
        /// the table against itself (de Bruijn degrees), read only: `out` takes the 258 words KH_GRAPH_* of the header names --
        /// `out[m]`, m < 256: the nodes whose neighbour mask is m; then the nodes and the sum of their counts
        pub fn kh_graph_stats(ctx: *mut KhCtx, min_count: u64, out: *mut u64) -> c_int;
        /// `masks[i]` = the neighbour mask of the packed canonical key `keys[i]`: bit c = right neighbour by letter c, bit 4 + c = left
        pub fn kh_graph_masks_device(ctx: *mut KhCtx, d_keys: *const u64, n: u64, min_count: u64, d_masks: *mut u8) -> c_int;
        pub fn kh_graph_masks(ctx: *mut KhCtx, keys: *const u64, n: u64, min_count: u64, masks: *mut u8) -> c_int;
        pub fn kh_unitigs_begin(ctx: *mut KhCtx, min_count: u64, n_unitigs: *mut u64, n_bases: *mut u64) -> c_int;
        pub fn kh_unitigs_copy_device(ctx: *mut KhCtx, d_rows: *mut u64, row_cap: u64, d_bases: *mut u8, base_cap: u64) -> c_int;
        pub fn kh_unitigs_copy(ctx: *mut KhCtx, rows: *mut u64, row_cap: u64, bases: *mut u8, base_cap: u64) -> c_int;
        pub fn kh_unitigs_end(ctx: *mut KhCtx) -> c_int;
        /// `kh_unitigs_begin` plus the links between the unitigs' ends: one word per link, ascending
        pub fn kh_unitigs_begin_linked(ctx: *mut KhCtx, min_count: u64, n_unitigs: *mut u64, n_bases: *mut u64, n_links: *mut u64) -> c_int;
        pub fn kh_unitigs_links_copy_device(ctx: *mut KhCtx, d_links: *mut u64, cap: u64) -> c_int;
        pub fn kh_unitigs_links_copy(ctx: *mut KhCtx, links: *mut u64, cap: u64) -> c_int;
        pub fn kh_unitigs_text_begin(ctx: *mut KhCtx, format: u32, n_bytes: *mut u64) -> c_int;
        pub fn kh_unitigs_text_next(ctx: *mut KhCtx, buf: *mut u8, cap: u64, n: *mut u64) -> c_int;
        pub fn kh_unitigs_text_next_device(ctx: *mut KhCtx, d_buf: *mut u8, cap: u64, n: *mut u64) -> c_int;
        /// `out[i]` = where on the live unitigs the k-mer at window start i lies: 2 * unitig + sign above the offset, or a special
        pub fn kh_unitigs_locate_device(ctx: *mut KhCtx, d_bases: *const u8, d_qual: *const u8, n: u64, d_out: *mut u64) -> c_int;
        pub fn kh_unitigs_locate(ctx: *mut KhCtx, bases: *const u8, qual: *const u8, n: u64, out: *mut u64) -> c_int;
        /// the same walk folded on the device into runs: `run_start` takes nrec + 1 CSR offsets, `runs` up to `run_cap` rows of 4 u32
        /// (KH_RUN_* of the header), `cover` (may be null) 2 u64 per unitig that are added to; `KH_ERR_RANGE` when `run_cap` is too small
        pub fn kh_unitigs_paths_device(ctx: *mut KhCtx, d_bases: *const u8, d_qual: *const u8, n: u64, d_rec_start: *const u64, nrec: u64,
                                       d_run_start: *mut u64, d_runs: *mut u32, run_cap: u64, d_cover: *mut u64, n_runs: *mut u64) -> c_int;
        pub fn kh_unitigs_paths(ctx: *mut KhCtx, bases: *const u8, qual: *const u8, n: u64, rec_start: *const u64, nrec: u64,
                                run_start: *mut u64, runs: *mut u32, run_cap: u64, cover: *mut u64, n_runs: *mut u64) -> c_int;
        /// how many records walk every link: two consecutive rows of a record with QEND == the next QSTART are a crossing, and
        /// `support[l] += 1` if its word is link l (`cap` >= n_links counters, added to); `out` (may be null) takes the 4 words KH_SUP_*
        pub fn kh_unitigs_link_support_device(ctx: *mut KhCtx, d_run_start: *const u64, nrec: u64, d_runs: *const u32, n_runs: u64,
                                              d_support: *mut u64, cap: u64, out: *mut u64) -> c_int;
        pub fn kh_unitigs_link_support(ctx: *mut KhCtx, run_start: *const u64, nrec: u64, runs: *const u32, n_runs: u64,
                                       support: *mut u64, cap: u64, out: *mut u64) -> c_int;
        /// one round of tip clipping of `src`'s compacted graph at `min_count`: the k-mers of the surviving unitigs are added to `dst`
        /// (`count[key] += c`); `out` takes the 8 words KH_CLIP_* of the header names
        pub fn kh_clip_tips_into(dst: *mut KhCtx, src: *mut KhCtx, min_count: u64, max_kmers: u64, out: *mut u64) -> c_int;
        /// one round of bubble popping of `src`'s compacted graph at `min_count`: of the parallel short unitigs between the same two
        /// places only the best stays, the k-mers of the surviving unitigs are added to `dst` (`count[key] += c`); `out` takes the 9
        /// words KH_POP_* of the header names
        pub fn kh_pop_bubbles_into(dst: *mut KhCtx, src: *mut KhCtx, min_count: u64, max_kmers: u64, out: *mut u64) -> c_int;
        /// the connected components of the live unitigs of kh_unitigs_begin_linked: `comp` takes one dense id per unitig, `rows` 4 words
        /// (KH_COMP_*) per component, either may be null with a cap of 0; `out` (required) takes the 4 words KH_CC_*
        pub fn kh_unitigs_components_device(ctx: *mut KhCtx, d_comp: *mut u32, comp_cap: u64, d_rows: *mut u64, row_cap: u64, out: *mut u64) -> c_int;
        pub fn kh_unitigs_components(ctx: *mut KhCtx, comp: *mut u32, comp_cap: u64, rows: *mut u64, row_cap: u64, out: *mut u64) -> c_int;
        /// one round of dropping the components of src's compacted graph with fewer than `min_kmers` k-mers; `out` takes the 9
        /// words KH_DROP_* of the header names
        pub fn kh_drop_components_into(dst: *mut KhCtx, src: *mut KhCtx, min_count: u64, min_kmers: u64, out: *mut u64) -> c_int;
        /// the result as text, formatted on the device; format: 1 = fasta, 2 = tsv, 3 = json (the whole document)
        pub fn kh_result_sorted(ctx: *mut KhCtx, keys: *mut u64, counts: *mut u64, cap: u64,
                                min_count: u64, n: *mut u64) -> c_int;
        pub fn kh_result_sorted_device(ctx: *mut KhCtx, d_keys: *mut u64, d_counts: *mut u64, cap: u64,
                                       min_count: u64, n: *mut u64) -> c_int;
        pub fn kh_result_text_begin(ctx: *mut KhCtx, format: u32, min_count: u64, n_records: *mut u64,
                                    n_bytes: *mut u64) -> c_int;
        /// whole records, at most `cap` bytes; `*n == 0`: the stream has ended; -8 (KH_ERR_RANGE): cap < the next record
        pub fn kh_result_text_next(ctx: *mut KhCtx, buf: *mut u8, cap: u64, n: *mut u64) -> c_int;
        pub fn kh_result_text_next_device(ctx: *mut KhCtx, d_buf: *mut u8, cap: u64, n: *mut u64) -> c_int;
        // host memory the device reaches by DMA (no staging copy in kh_push / kh_push_text / kh_result_copy)
        pub fn kh_host_alloc(out: *mut *mut c_void, bytes: u64) -> c_int;
        pub fn kh_host_free(p: *mut c_void) -> c_int;
        pub fn kh_host_register(p: *mut c_void, bytes: u64) -> c_int;
        pub fn kh_host_unregister(p: *mut c_void) -> c_int;
        pub fn kh_pack(bases: *const u8, k: u32, packed: *mut u64, err_pos: *mut u32) -> c_int;
        pub fn kh_unpack(packed: u64, k: u32, out: *mut u8) -> c_int;
        pub fn kh_canonical(packed: u64, k: u32, canonical: *mut u64, is_rc: *mut c_int) -> c_int;
        pub fn kh_strerror(status: c_int) -> *const c_char;
        pub fn kh_last_error(ctx: *const KhCtx) -> *const c_char;
        // the multi-GPU exchange (RCCL over xGMI) behind the ABI
        pub fn kh_owner(key: u64, k: u32, nparts: u32) -> u32;
        pub fn kh_comm_unique_id(out: *mut KhUniqueId) -> c_int;
        pub fn kh_comm_init(ctx: *mut KhCtx, nranks: u32, rank: u32, id: *const KhUniqueId) -> c_int;
        pub fn kh_merge_across(ctx: *mut KhCtx, info: *mut KhMergeInfo) -> c_int;
        pub fn kh_group_create(out: *mut *mut KhGroup, cfg: *const KhConfig, devices: *const i32, ndevices: u32) -> c_int;
        pub fn kh_group_ctx(g: *mut KhGroup, rank: u32) -> *mut KhCtx;
        pub fn kh_group_size(g: *const KhGroup) -> u32;
        pub fn kh_group_merge(g: *mut KhGroup, infos: *mut KhMergeInfo) -> c_int;
        pub fn kh_group_destroy(g: *mut KhGroup);
    }
}

/// Errors of the device path.  `KmerLength` is `KmerLengthError` of `src/error.rs:86-95`.
/// `Device` carries the status text of the C ABI and `kh_last_error`.  Out of memory (`KH_ERR_OOM`) follows the contract of
/// `include/kmerhip.h`, "Allocation failures": a method that only reads the table (`profile*`, `compare`, `graph_*`, `unitigs*`,
/// the results) leaves the map usable and unchanged, so it can be called again; one that writes it (`build*`, `push_text`,
/// `combine_into` / `clip_tips_into` on their target) leaves the map poisoned -- every later call fails with "invalid context
/// state" until the context is reset (`kh_reset`: an empty, usable map) or dropped.
#[derive(Debug, thiserror::Error)]
pub enum HipError {
    #[error("k-mer length {k} is out of range: must be between 1 and 32")]
    KmerLength { k: usize },
    #[error("kmerhip: {0}")]
    Device(String),
}

/// `KMERHIP_ABI_VERSION` of the `include/kmerhip.h` that `mod sys` mirrors: the structs above are laid out for it.
pub const ABI_VERSION: c_int = 2;
/// `KH_PROFILE_NO_WINDOW`: an entry of [`HipKmerMap::profile`] where counting would see no window
pub const PROFILE_NO_WINDOW: u32 = 0xFFFF_FFFF;

/// The words of `kh_compare`: two tables set against each other.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct TableComparison {
    pub distinct_a: u64,
    pub distinct_b: u64,
    /// keys in both sets
    pub shared: u64,
    /// sums of the counts over each table's set (modulo 2^64)
    pub sum_a: u64,
    pub sum_b: u64,
    pub shared_sum_a: u64,
    pub shared_sum_b: u64,
    /// sum over the shared keys of `min(ca, cb)`
    pub sum_min: u64,
}

impl TableComparison {
    pub fn jaccard(&self) -> f64 { self.shared as f64 / (self.distinct_a + self.distinct_b - self.shared) as f64 }
    pub fn containment_a(&self) -> f64 { self.shared as f64 / self.distinct_a as f64 }
    pub fn containment_b(&self) -> f64 { self.shared as f64 / self.distinct_b as f64 }
    pub fn bray_curtis(&self) -> f64 { 1.0 - 2.0 * self.sum_min as f64 / (self.sum_a as f64 + self.sum_b as f64) }
}

/// `KH_GRAPH_WORDS`: the words of `kh_graph_stats` -- 256 mask counters, then `KH_GRAPH_NODES` and `KH_GRAPH_KMERS`.
pub const GRAPH_WORDS: usize = 258;
pub const GRAPH_NODES: usize = 256;
pub const GRAPH_KMERS: usize = 257;
/// `KH_GRAPH_RIGHT(c)`: the mask bit of the right neighbour by letter `c` (0..3 = A, C, G, T) of a key's canonical string.
pub const fn graph_right(c: u32) -> u8 { 1u8 << c }
/// `KH_GRAPH_LEFT(c)`: ... of the left neighbour.
pub const fn graph_left(c: u32) -> u8 { 16u8 << c }

/// `KH_UNI_WORDS`: the words of a unitig row of `kh_unitigs_copy` -- `KH_UNI_START`, `KH_UNI_KMERS`, `KH_UNI_COUNT_SUM`, `KH_UNI_FLAGS`.
pub const UNI_WORDS: usize = 4;
pub const UNI_START: usize = 0;
pub const UNI_KMERS: usize = 1;
pub const UNI_COUNT_SUM: usize = 2;
pub const UNI_FLAGS: usize = 3;
/// `KH_UNI_CIRCULAR`: bit 0 of the flags word -- the chain closes, and the closing overlap is not repeated in the bases.
pub const UNI_CIRCULAR: u64 = 1;

/// `KH_UNI_TEXT_FASTA` / `KH_UNI_TEXT_GFA`: the formats of [`HipKmerMap::unitigs_text`].
pub const UNI_TEXT_FASTA: u32 = 1;
pub const UNI_TEXT_GFA: u32 = 2;
/// `KH_LOC_NO_WINDOW`: a word of [`HipKmerMap::unitigs_locate`] where [`HipKmerMap::profile`] says [`PROFILE_NO_WINDOW`].
pub const LOC_NO_WINDOW: u64 = !0u64;
/// `KH_LOC_ABSENT`: a valid window whose k-mer is no node of the located unitigs.
pub const LOC_ABSENT: u64 = !0u64 - 1;
/// `KH_LOC_IS_PLACE(w)`: neither of the two specials.
pub const fn loc_is_place(w: u64) -> bool { w < LOC_ABSENT }
/// `KH_LOC_UNITIG(w)`: the unitig (a row index of `kh_unitigs_copy`) the window's k-mer lies in.
pub const fn loc_unitig(w: u64) -> u32 { (w >> 33) as u32 }
/// `KH_LOC_SIGN(w)`: 0 = the window reads the k-mer as the unitig's reported sequence spells it, 1 = as its reverse complement.
pub const fn loc_sign(w: u64) -> u32 { ((w >> 32) & 1) as u32 }
/// `KH_LOC_OFFSET(w)`: the k-mer is bases offset .. offset + k of the unitig's reported sequence.
pub const fn loc_offset(w: u64) -> u32 { (w & 0xFFFF_FFFF) as u32 }
/// `KH_RUN_WORDS`: the u32 words of a run row of [`HipKmerMap::unitigs_paths`] -- `RUN_STATE` (2 * unitig + sign), `RUN_OFFSET` (of
/// the run's first window in the unitig's reported sequence), `RUN_QSTART` and `RUN_QEND` (window starts relative to the record).
pub const RUN_WORDS: usize = 4;
pub const RUN_STATE: usize = 0;
pub const RUN_OFFSET: usize = 1;
pub const RUN_QSTART: usize = 2;
pub const RUN_QEND: usize = 3;
/// `KH_COV_WORDS`: the u64 words per unitig of the coverage array -- `COV_WINDOWS` (windows located on it), `COV_RUNS` (runs on it).
pub const COV_WORDS: usize = 2;
pub const COV_WINDOWS: usize = 0;
pub const COV_RUNS: usize = 1;
/// `KH_SUP_WORDS`: the words of [`HipKmerMap::unitigs_link_support`] -- `SUP_PAIRS` (consecutive rows of one record), `SUP_ADJACENT`
/// (of those: no window start between them), `SUP_CREDITED` (of those: the word is a link), `SUP_MISSING` (the rest).
pub const SUP_WORDS: usize = 4;
pub const SUP_PAIRS: usize = 0;
pub const SUP_ADJACENT: usize = 1;
pub const SUP_CREDITED: usize = 2;
pub const SUP_MISSING: usize = 3;
/// The mirror of a link word (a << 32) | b: the crossing that the reverse-complemented read makes.
pub const fn link_mirror(w: u64) -> u64 { (((w & 0xFFFF_FFFF) ^ 1) << 32) | ((w >> 32) ^ 1) }
/// `KH_UNI_LINK_FROM(w)`: the unitig a link word of `kh_unitigs_links_copy` leaves (a row index of `kh_unitigs_copy`).
pub const fn uni_link_from(w: u64) -> u32 { (w >> 33) as u32 }
/// `KH_UNI_LINK_FROM_SIGN(w)`: 0 = it leaves the right end of the reported sequence (+), 1 = that of its reverse complement (-).
pub const fn uni_link_from_sign(w: u64) -> u32 { ((w >> 32) & 1) as u32 }
/// `KH_UNI_LINK_TO(w)`: the unitig the link enters.
pub const fn uni_link_to(w: u64) -> u32 { ((w & 0xFFFF_FFFF) >> 1) as u32 }
/// `KH_UNI_LINK_TO_SIGN(w)`: 0 = entered at the start of its reported sequence (+), 1 = at the start of its reverse complement (-).
pub const fn uni_link_to_sign(w: u64) -> u32 { (w & 1) as u32 }

/// `KH_CLIP_WORDS`: the words of [`HipKmerMap::clip_tips_into`] -- unitigs, candidates, clipped, clipped_kmers, clipped_count,
/// kept_kmers, kept_count, links (`CLIP_UNITIGS` .. `CLIP_LINKS`).
pub const CLIP_WORDS: usize = 8;
pub const CLIP_UNITIGS: usize = 0;
pub const CLIP_CANDIDATES: usize = 1;
pub const CLIP_CLIPPED: usize = 2;
pub const CLIP_CLIPPED_KMERS: usize = 3;
pub const CLIP_CLIPPED_COUNT: usize = 4;
pub const CLIP_KEPT_KMERS: usize = 5;
pub const CLIP_KEPT_COUNT: usize = 6;
pub const CLIP_LINKS: usize = 7;

/// `KH_POP_WORDS`: the words of [`HipKmerMap::pop_bubbles_into`] -- unitigs, candidates, popped, popped_kmers, popped_count,
/// kept_kmers, kept_count, links, bubbles (`POP_UNITIGS` .. `POP_BUBBLES`); the first eight mean what the `CLIP_*` words mean.
pub const POP_WORDS: usize = 9;
pub const POP_UNITIGS: usize = 0;
pub const POP_CANDIDATES: usize = 1;
pub const POP_POPPED: usize = 2;
pub const POP_POPPED_KMERS: usize = 3;
pub const POP_POPPED_COUNT: usize = 4;
pub const POP_KEPT_KMERS: usize = 5;
pub const POP_KEPT_COUNT: usize = 6;
pub const POP_LINKS: usize = 7;
pub const POP_BUBBLES: usize = 8;

/// `KH_COMP_WORDS`: the words of a component row of [`HipKmerMap::unitigs_components`] -- `COMP_FIRST` (its smallest unitig index),
/// `COMP_UNITIGS`, `COMP_KMERS`, `COMP_COUNT_SUM`; `KH_CC_WORDS`: the words of the call -- `CC_COMPONENTS`, `CC_SINGLETONS`,
/// `CC_LARGEST_KMERS`, `CC_ROUNDS` (the hooking rounds of the build).
pub const COMP_WORDS: usize = 4;
pub const COMP_FIRST: usize = 0;
pub const COMP_UNITIGS: usize = 1;
pub const COMP_KMERS: usize = 2;
pub const COMP_COUNT_SUM: usize = 3;
pub const CC_WORDS: usize = 4;
pub const CC_COMPONENTS: usize = 0;
pub const CC_SINGLETONS: usize = 1;
pub const CC_LARGEST_KMERS: usize = 2;
pub const CC_ROUNDS: usize = 3;

/// `KH_DROP_WORDS`: the words of [`HipKmerMap::drop_components_into`] -- unitigs, components, dropped, dropped_kmers, dropped_count,
/// kept_kmers, kept_count, links, dropped_unitigs (`DROP_UNITIGS` .. `DROP_DROPPED_UNITIGS`); words 0, 5, 6 and 7 mean what the
/// `CLIP_*` words mean.
pub const DROP_WORDS: usize = 9;
pub const DROP_UNITIGS: usize = 0;
pub const DROP_COMPONENTS: usize = 1;
pub const DROP_DROPPED: usize = 2;
pub const DROP_DROPPED_KMERS: usize = 3;
pub const DROP_DROPPED_COUNT: usize = 4;
pub const DROP_KEPT_KMERS: usize = 5;
pub const DROP_KEPT_COUNT: usize = 6;
pub const DROP_LINKS: usize = 7;
pub const DROP_DROPPED_UNITIGS: usize = 8;

/// KH_SET_*: the set operation of `kh_combine_into`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(u32)]
pub enum SetOp { Intersect = 1, Union = 2, Subtract = 3, CountSubtract = 4 }

/// KH_CALC_*: the count of a key both tables hold (`Sum` saturates at `u64::MAX`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(u32)]
pub enum CountRule { Min = 1, Max = 2, Sum = 3, Left = 4, Right = 5 }

/// One row of [`HipKmerMap::profile_records`] (`KH_REC_*`): the reduction of a record's profile entries that are a window.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct RecordAbundance {
    /// entries of the record that are a window
    pub windows: u32,
    /// windows whose count is > 0
    pub present: u32,
    /// windows with `lo <= count <= hi`
    pub in_range: u32,
    /// min / max over the windows (0 when there is none)
    pub min: u32,
    pub max: u32,
    /// sum of the saturated counts
    pub sum: u64,
    /// offset from the record start of the first window whose count is `< lo`
    pub first_low: Option<u32>,
}

/// `KH_OUT_SORTED`: ORed into the format of `kh_result_text_begin`, the records come in ascending key order.
pub const KH_OUT_SORTED: u32 = 0x100;

/// The record formats of `kh_result_text_begin` (`KH_OUT_*`): the reference's `OutputFormat` without the histogram.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(u32)]
pub enum TextFormat {
    Fasta = 1,
    Tsv = 2,
    Json = 3,
}

/// Called before the first `kh_create` of every constructor: a library of another ABI version is refused, not guessed at.
fn check_abi() -> Result<(), HipError> {
    // SAFETY: a pure function of the library
    let v = unsafe { sys::kh_abi_version() };
    if v != ABI_VERSION {
        return Err(HipError::Device(format!("libkmerhip speaks ABI version {v}, this crate {ABI_VERSION}")));
    }
    Ok(())
}

fn check(ctx: *const sys::KhCtx, rc: c_int) -> Result<(), HipError> {
    if rc == 0 {
        return Ok(());
    }
    // SAFETY: both functions return NUL-terminated static / context-owned strings
    let mut msg = unsafe { CStr::from_ptr(sys::kh_strerror(rc)) }.to_string_lossy().into_owned();
    if !ctx.is_null() {
        let detail = unsafe { CStr::from_ptr(sys::kh_last_error(ctx)) }.to_string_lossy();
        if !detail.is_empty() {
            msg = format!("{msg} ({detail})");
        }
    }
    Err(HipError::Device(msg))
}

/// Pinned host memory (`kh_host_alloc`): `kh_push` / `kh_push_text` from it and `kh_result_copy` into it move by DMA,
/// without the staging `memcpy` pageable memory needs.  Where `src/reader.rs:58-79` collects records into
/// `Vec<Bytes>`, a host that wants PCIe speed appends them to one of these instead.
pub struct PinnedBuf {
    ptr: *mut u8,
    cap: usize,
    len: usize,
}

unsafe impl Send for PinnedBuf {}

impl PinnedBuf {
    pub fn with_capacity(cap: usize) -> Result<Self, HipError> {
        let mut p: *mut c_void = std::ptr::null_mut();
        check(std::ptr::null(), unsafe { sys::kh_host_alloc(&mut p, cap.max(1) as u64) })?;
        Ok(Self { ptr: p as *mut u8, cap, len: 0 })
    }
    pub fn len(&self) -> usize {
        self.len
    }
    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
    pub fn clear(&mut self) {
        self.len = 0;
    }
    pub fn room(&self) -> usize {
        self.cap - self.len
    }
    /// Appends `s` (the caller checks `room()` first).
    pub fn extend_from_slice(&mut self, s: &[u8]) {
        assert!(s.len() <= self.room());
        // SAFETY: [ptr + len, ptr + len + s.len()) lies inside the allocation and does not overlap `s`
        unsafe { std::ptr::copy_nonoverlapping(s.as_ptr(), self.ptr.add(self.len), s.len()) };
        self.len += s.len();
    }
    pub fn as_slice(&self) -> &[u8] {
        // SAFETY: the first `len` bytes are initialised
        unsafe { std::slice::from_raw_parts(self.ptr, self.len) }
    }
}

impl Drop for PinnedBuf {
    fn drop(&mut self) {
        unsafe { sys::kh_host_free(self.ptr as *mut c_void) };
    }
}

/// Drop-in for `KmerMap` (`src/run.rs:491-583`): `build` / `build_with_quality` / `into_hashmap`.
pub struct HipKmerMap {
    ctx: *mut sys::KhCtx,
    k: usize,
    has_qual: bool,
}

// one producer thread per context (kmerhip.h); moving the handle between threads is fine
unsafe impl Send for HipKmerMap {}

const BATCH: usize = 256 << 20;

impl HipKmerMap {
    pub fn new(k: usize, min_quality: Option<u8>) -> Result<Self, HipError> {
        if !(1..=32).contains(&k) {
            return Err(HipError::KmerLength { k }); // KmerLength::new, src/kmer.rs:100-110
        }
        let cfg = sys::KhConfig {
            struct_size: std::mem::size_of::<sys::KhConfig>() as u32,
            k: k as u32,
            min_quality: min_quality.map_or(-1, i32::from),
            device: -1,
            capacity_hint: 0,
            stream: std::ptr::null_mut(),
            flags: 0,
            input_mib: 0,
        };
        let mut ctx = std::ptr::null_mut();
        check_abi()?;
        check(std::ptr::null(), unsafe { sys::kh_create(&mut ctx, &cfg) })?;
        Ok(Self { ctx, k, has_qual: min_quality.is_some() })
    }

    fn push(&self, bases: &[u8], qual: Option<&[u8]>) -> Result<(), HipError> {
        if bases.is_empty() {
            return Ok(());
        }
        let q = qual.map_or(std::ptr::null(), <[u8]>::as_ptr);
        check(self.ctx, unsafe { sys::kh_push(self.ctx, bases.as_ptr(), q, bases.len() as u64) })
    }

    /// `KmerMap::build` (`src/run.rs:500-503`).  Records are concatenated into flat buffers with a
    /// `\n` between them: any byte outside `ACGTacgt` separates records, no k-mer spans it.
    pub fn build<I: Iterator<Item = Bytes>>(self, sequences: I) -> Result<Self, HipError> {
        // the batch buffer is pinned: kh_push DMAs from it, no staging copy inside the library
        let mut flat = PinnedBuf::with_capacity(BATCH + (1 << 20))?;
        for seq in sequences {
            if seq.len() + 1 > flat.room() {
                self.push(flat.as_slice(), None)?;
                flat.clear();
            }
            if seq.len() + 1 > flat.room() {
                // a record larger than the batch buffer (a chromosome): straight from its own (pageable) memory, then the separator
                self.push(&seq, None)?;
                continue;
            }
            flat.extend_from_slice(&seq);
            flat.extend_from_slice(b"\n");
        }
        self.push(flat.as_slice(), None)?;
        Ok(self)
    }

    /// `KmerMap::build_with_quality` (`src/run.rs:505-520`); the threshold was given to `new`.
    /// A record without qualities (FASTA) is never masked (`run.rs:543`: both must be `Some`).
    pub fn build_with_quality<I>(self, sequences: I) -> Result<Self, HipError>
    where
        I: Iterator<Item = (Bytes, Option<Vec<u8>>)>,
    {
        let (mut b, mut q) = (Vec::with_capacity(BATCH), Vec::with_capacity(BATCH));
        for (seq, qual) in sequences {
            b.extend_from_slice(&seq);
            b.push(b'\n');
            match qual {
                Some(qs) => q.extend_from_slice(&qs),
                None => q.resize(q.len() + seq.len(), 0xFF), // 0xFF >= any threshold (<= 255): never masked
            }
            q.push(b'\n');
            if b.len() >= BATCH {
                self.push(&b, self.has_qual.then_some(&q[..]))?;
                b.clear();
                q.clear();
            }
        }
        self.push(&b, self.has_qual.then_some(&q[..]))?;
        Ok(self)
    }

    /// Raw FASTA / FASTQ text (whole records, uncompressed), records found on the device instead of by
    /// the `bio` readers (`src/reader.rs:58-79`).  `Ok(false)`: the device scanner declined the layout
    /// (wrapped FASTQ, ...) and counted nothing of THIS text; the caller parses the text as today and calls
    /// `build` / `build_with_quality`.  `text` may be reused when the call returns; the counting of an accepted text may
    /// run under the next call's copy (it is finished by `into_packed` / `kh_finish` at the latest).
    pub fn push_text(&mut self, text: &[u8], fastq: bool) -> Result<bool, HipError> {
        let rc = unsafe { sys::kh_push_text(self.ctx, text.as_ptr(), text.len() as u64, if fastq { 2 } else { 1 }) };
        if rc == -9 {
            return Ok(false); // KH_ERR_FORMAT
        }
        check(self.ctx, rc)?;
        Ok(true)
    }

    /// The table's count of the canonical k-mer at every window start of `bases` -- a flat buffer as `push` takes it, records
    /// separated by a byte outside `ACGTacgt`, `qual` masking as in counting -- one `u32` per byte: the count (saturated at
    /// `0xFFFF_FFFE`, 0 = absent) or [`PROFILE_NO_WINDOW`] where there is no window (N, soft mask, low quality, the last
    /// k-1 bytes).  Reads the table only (`kh_profile`); pushes still pending are counted first.
    pub fn profile(&mut self, bases: &[u8], qual: Option<&[u8]>) -> Result<Vec<u32>, HipError> {
        if let Some(q) = qual {
            assert_eq!(q.len(), bases.len(), "qual must be as long as bases");
        }
        let mut out = vec![0u32; bases.len()];
        check(self.ctx, unsafe {
            sys::kh_profile(self.ctx, bases.as_ptr(), qual.map_or(std::ptr::null(), |q| q.as_ptr()), bases.len() as u64, out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// [`profile`](Self::profile) reduced per record on the device (`kh_profile_records`): `rec_start` holds `nrec + 1`
    /// ascending offsets into `bases` (the last one `<= bases.len()`), record `r` owns the window starts
    /// `rec_start[r] .. rec_start[r+1]`.  32 bytes per record come back instead of 4 per base.
    pub fn profile_records(&mut self, bases: &[u8], qual: Option<&[u8]>, rec_start: &[u64], lo: u32, hi: u32) -> Result<Vec<RecordAbundance>, HipError> {
        if let Some(q) = qual {
            assert_eq!(q.len(), bases.len(), "qual must be as long as bases");
        }
        let nrec = rec_start.len().saturating_sub(1);
        let mut rows = vec![0u32; nrec * 8];
        check(self.ctx, unsafe {
            sys::kh_profile_records(self.ctx, bases.as_ptr(), qual.map_or(std::ptr::null(), |q| q.as_ptr()), bases.len() as u64,
                                    rec_start.as_ptr(), nrec as u64, lo, hi, rows.as_mut_ptr())
        })?;
        Ok(rows.chunks_exact(8).map(|w| RecordAbundance {
            windows: w[0], present: w[1], in_range: w[2], min: w[3], max: w[4], sum: (w[5] as u64) | ((w[6] as u64) << 32),
            first_low: if w[7] == 0xFFFF_FFFF { None } else { Some(w[7]) },
        }).collect())
    }

    /// This table (a) against `other` (b), on the device, both only read (`kh_compare`): the keys with a count of at least
    /// `max(min_a, 1)` here and `max(min_b, 1)` there (`other` may be this table).  Jaccard, containment and Bray-Curtis are [`TableComparison`]'s methods.
    pub fn compare(&self, other: &HipKmerMap, min_a: u64, min_b: u64) -> Result<TableComparison, HipError> {
        let mut w = [0u64; 8];
        check(self.ctx, unsafe { sys::kh_compare(self.ctx, other.ctx, min_a, min_b, w.as_mut_ptr()) })?;
        Ok(TableComparison {
            distinct_a: w[0], distinct_b: w[1], shared: w[2], sum_a: w[3], sum_b: w[4], shared_sum_a: w[5], shared_sum_b: w[6], sum_min: w[7],
        })
    }

    /// Adds the pairs of a set operation of the tables `a` and `b` to THIS table (`kh_combine_into`: `count[key] += c`; the
    /// table need not be empty).  `calc` is the count of a key both hold, for [`SetOp::Intersect`] and [`SetOp::Union`].
    /// `a` and `b` are only read (the same table may be both); the borrow rules keep this table from being either.
    /// Returns the number of pairs produced.
    pub fn combine_into(&mut self, a: &HipKmerMap, b: &HipKmerMap, op: SetOp, calc: CountRule, min_a: u64, min_b: u64) -> Result<u64, HipError> {
        let mut n = 0u64;
        check(self.ctx, unsafe { sys::kh_combine_into(self.ctx, a.ctx, b.ctx, op as u32, calc as u32, min_a, min_b, &mut n) })?;
        Ok(n)
    }

    /// The de Bruijn graph degrees of this table (`kh_graph_stats`), read only: over the node set S = the keys with a count of
    /// at least `max(min_count, 1)`, word `m` (m < 256) counts the nodes whose neighbour mask is `m`, word [`GRAPH_NODES`] is
    /// |S| and word [`GRAPH_KMERS`] the sum of their counts.
    pub fn graph_stats(&self, min_count: u64) -> Result<Vec<u64>, HipError> {
        let mut w = vec![0u64; GRAPH_WORDS];
        check(self.ctx, unsafe { sys::kh_graph_stats(self.ctx, min_count, w.as_mut_ptr()) })?;
        Ok(w)
    }

    /// One neighbour mask per packed canonical key (`kh_graph_masks`): bit `c` ([`graph_right`]) is set iff the right neighbour
    /// by letter `c` is in S, bit `4 + c` ([`graph_left`]) iff the left one is; a word that is no canonical key of this k gets 0.
    /// The keys need not be in S.  With the keys of [`sorted_pairs`](Self::sorted_pairs) the masks line up with those pairs.
    pub fn graph_masks(&self, keys: &[u64], min_count: u64) -> Result<Vec<u8>, HipError> {
        let mut m = vec![0u8; keys.len()];
        check(self.ctx, unsafe { sys::kh_graph_masks(self.ctx, keys.as_ptr(), keys.len() as u64, min_count, m.as_mut_ptr()) })?;
        Ok(m)
    }

    /// The unitigs of this table's de Bruijn graph (`kh_unitigs_begin` / `kh_unitigs_copy` / `kh_unitigs_end`), built on the
    /// device over the node set S = the keys with a count of at least `max(min_count, 1)`: [`UNI_WORDS`] words per unitig
    /// (its first base's offset, its k-mers L, the sum of their counts, the flags) and the bases (ASCII, unitig after unitig; a
    /// unitig has L + k - 1 of them), in ascending key order of the unitigs' first nodes.  The same table content gives the same
    /// bytes whatever the table's geometry.
    pub fn unitigs(&self, min_count: u64) -> Result<(Vec<u64>, Vec<u8>), HipError> {
        let (mut nu, mut nb) = (0u64, 0u64);
        check(self.ctx, unsafe { sys::kh_unitigs_begin(self.ctx, min_count, &mut nu, &mut nb) })?;
        let mut rows = vec![0u64; nu as usize * UNI_WORDS];
        let mut bases = vec![0u8; nb as usize];
        let rc = unsafe { sys::kh_unitigs_copy(self.ctx, rows.as_mut_ptr(), nu, bases.as_mut_ptr(), nb) };
        let end = unsafe { sys::kh_unitigs_end(self.ctx) };
        check(self.ctx, rc)?;
        check(self.ctx, end)?;
        Ok((rows, bases))
    }

    /// One round of tip clipping (`kh_clip_tips_into`): the unitigs and links of `src` at `min_count` are built on the device, a
    /// non-circular unitig of at most `max_kmers` k-mers with exactly one dead end is clipped when at every link out of its attached
    /// end a rival beats it (a unitig that is no candidate, or a candidate with the greater (KMERS, COUNT_SUM), then the smaller
    /// index), and the k-mers of every surviving unitig are added to THIS table with their counts from `src` (`count[key] += c`).
    /// `src` is only read; unitigs it had begun are released.  The borrow rules keep this table from being `src`.  Returns the
    /// eight words ([`CLIP_UNITIGS`] .. [`CLIP_LINKS`]).
    pub fn clip_tips_into(&mut self, src: &HipKmerMap, min_count: u64, max_kmers: u64) -> Result<[u64; CLIP_WORDS], HipError> {
        let mut out = [0u64; CLIP_WORDS];
        check(self.ctx, unsafe { sys::kh_clip_tips_into(self.ctx, src.ctx, min_count, max_kmers, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// One round of bubble popping (`kh_pop_bubbles_into`): the unitigs and links of `src` at `min_count` are built on the device;
    /// non-circular unitigs of at most `max_kmers` k-mers (a SNP branch has k; 2 k is a usual bound) with exactly one link out of
    /// each end are parallel when their ends enter the same unordered pair of states, and of every such class only the one with
    /// the greatest mean count stays (compared exactly, then the most k-mers, then the smallest index).  The k-mers of every
    /// surviving unitig are added to THIS table with their counts from `src` (`count[key] += c`).  `src` is only read; unitigs it
    /// had begun are released.  The borrow rules keep this table from being `src`.  Returns the nine words ([`POP_UNITIGS`] ..
    /// [`POP_BUBBLES`]).
    pub fn pop_bubbles_into(&mut self, src: &HipKmerMap, min_count: u64, max_kmers: u64) -> Result<[u64; POP_WORDS], HipError> {
        let mut out = [0u64; POP_WORDS];
        check(self.ctx, unsafe { sys::kh_pop_bubbles_into(self.ctx, src.ctx, min_count, max_kmers, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// One round of dropping small components (`kh_drop_components_into`): the unitigs and links of `src` at `min_count` are built
    /// on the device and labelled by connected component; the k-mers of every component that holds at least `min_kmers` k-mers are
    /// added to this table with their counts (`count[key] += c`), the smaller ones -- the isolated debris clipping and popping cannot
    /// touch -- are left out.  0 or 1 drops nothing; a circular unitig is treated like any other.  `src` is only read; unitigs it had
    /// begun are released.  Returns the nine words ([`DROP_UNITIGS`] .. [`DROP_DROPPED_UNITIGS`]).
    pub fn drop_components_into(&mut self, src: &HipKmerMap, min_count: u64, min_kmers: u64) -> Result<[u64; DROP_WORDS], HipError> {
        let mut out = [0u64; DROP_WORDS];
        check(self.ctx, unsafe { sys::kh_drop_components_into(self.ctx, src.ctx, min_count, min_kmers, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// [`unitigs`](Self::unitigs) and the links between the unitigs' ends (`kh_unitigs_begin_linked` / `kh_unitigs_copy` /
    /// `kh_unitigs_links_copy` / `kh_unitigs_end`): one word per link -- [`uni_link_from`], [`uni_link_from_sign`], [`uni_link_to`],
    /// [`uni_link_to_sign`] take it apart --, in ascending word order; a link spans k - 1 bases of overlap.  Loops, hairpins and
    /// the closing link of a circular unitig are links like any other.
    pub fn unitigs_linked(&self, min_count: u64) -> Result<(Vec<u64>, Vec<u8>, Vec<u64>), HipError> {
        let (mut nu, mut nb, mut nl) = (0u64, 0u64, 0u64);
        check(self.ctx, unsafe { sys::kh_unitigs_begin_linked(self.ctx, min_count, &mut nu, &mut nb, &mut nl) })?;
        let mut rows = vec![0u64; nu as usize * UNI_WORDS];
        let mut bases = vec![0u8; nb as usize];
        let mut links = vec![0u64; nl as usize];
        let rc = unsafe { sys::kh_unitigs_copy(self.ctx, rows.as_mut_ptr(), nu, bases.as_mut_ptr(), nb) };
        let rl = unsafe { sys::kh_unitigs_links_copy(self.ctx, links.as_mut_ptr(), nl) };
        let end = unsafe { sys::kh_unitigs_end(self.ctx) };
        check(self.ctx, rc)?;
        check(self.ctx, rl)?;
        check(self.ctx, end)?;
        Ok((rows, bases, links))
    }

    /// The unitigs of the table as text, formatted on the device (`kh_unitigs_begin[_linked]` / `kh_unitigs_text_begin` /
    /// `kh_unitigs_text_next` / `kh_unitigs_end`): [`UNI_TEXT_FASTA`] is what `kmerust unitigs -f fasta` prints, [`UNI_TEXT_GFA`]
    /// what `kmerust gfa -f gfa` prints (segments, then one L line per link).  Only text crosses the link, in pieces of up to
    /// 64 MiB.
    pub fn unitigs_text(&self, format: u32, min_count: u64) -> Result<Vec<u8>, HipError> {
        let (mut nu, mut nb, mut nl, mut total) = (0u64, 0u64, 0u64, 0u64);
        check(self.ctx, unsafe {
            if format == UNI_TEXT_GFA {
                sys::kh_unitigs_begin_linked(self.ctx, min_count, &mut nu, &mut nb, &mut nl)
            } else {
                sys::kh_unitigs_begin(self.ctx, min_count, &mut nu, &mut nb)
            }
        })?;
        let mut rc = unsafe { sys::kh_unitigs_text_begin(self.ctx, format, &mut total) };
        let mut text = vec![0u8; if rc == 0 { total as usize } else { 0 }];
        let mut at = 0usize;
        while rc == 0 && at < text.len() {
            let mut n = 0u64;
            let cap = (text.len() - at).min(64 << 20) as u64;
            rc = unsafe { sys::kh_unitigs_text_next(self.ctx, text.as_mut_ptr().add(at), cap, &mut n) };
            if n == 0 {
                break;
            }
            at += n as usize;
        }
        let err = check(self.ctx, rc);  // (before kh_unitigs_end replaces the error text)
        let end = unsafe { sys::kh_unitigs_end(self.ctx) };
        err?;
        check(self.ctx, end)?;
        text.truncate(at);
        Ok(text)
    }

    /// The windows of `bases` located on the unitigs of the table at `min_count` (`kh_unitigs_begin_linked` / `kh_unitigs_locate` /
    /// `kh_unitigs_end`): one word per byte of the flat buffer (records separated by a byte outside ACGTacgt; `qual` masks as in
    /// counting) -- [`LOC_NO_WINDOW`], [`LOC_ABSENT`], or a place that [`loc_unitig`], [`loc_sign`] and [`loc_offset`] take apart.
    /// The unitig indices are the row indices of [`unitigs_linked`](Self::unitigs_linked) at the same `min_count`.
    pub fn unitigs_locate(&self, min_count: u64, bases: &[u8], qual: Option<&[u8]>) -> Result<Vec<u64>, HipError> {
        if let Some(q) = qual {
            if q.len() != bases.len() {
                return Err(HipError::Device("qual must have the same length as bases".into()));
            }
        }
        let (mut nu, mut nb, mut nl) = (0u64, 0u64, 0u64);
        check(self.ctx, unsafe { sys::kh_unitigs_begin_linked(self.ctx, min_count, &mut nu, &mut nb, &mut nl) })?;
        let mut out = vec![0u64; bases.len()];
        let rc = unsafe {
            sys::kh_unitigs_locate(self.ctx, bases.as_ptr(), qual.map_or(std::ptr::null(), |q| q.as_ptr()), bases.len() as u64, out.as_mut_ptr())
        };
        let err = check(self.ctx, rc);  // (before kh_unitigs_end replaces the error text)
        let end = unsafe { sys::kh_unitigs_end(self.ctx) };
        err?;
        check(self.ctx, end)?;
        Ok(out)
    }

    /// The records of `bases` as run-compressed walks over the unitigs of the table at `min_count` (`kh_unitigs_begin_linked` /
    /// `kh_unitigs_paths` twice -- once to size, once to fill -- / `kh_unitigs_end`).  `rec_start` holds nrec + 1 ascending offsets into
    /// the flat buffer.  Returns `(run_start, runs, cover)`: nrec + 1 CSR offsets, `RUN_WORDS` u32 per run (`RUN_STATE` ..
    /// `RUN_QEND`; the runs of record r are rows `run_start[r] .. run_start[r + 1]`), and `COV_WORDS` u64 per unitig (windows, runs).
    pub fn unitigs_paths(&self, min_count: u64, bases: &[u8], qual: Option<&[u8]>, rec_start: &[u64])
                         -> Result<(Vec<u64>, Vec<u32>, Vec<u64>), HipError> {
        if let Some(q) = qual {
            if q.len() != bases.len() {
                return Err(HipError::Device("qual must have the same length as bases".into()));
            }
        }
        if rec_start.is_empty() {
            return Err(HipError::Device("rec_start needs nrec + 1 offsets".into()));
        }
        let nrec = (rec_start.len() - 1) as u64;
        let (mut nu, mut nb, mut nl) = (0u64, 0u64, 0u64);
        check(self.ctx, unsafe { sys::kh_unitigs_begin_linked(self.ctx, min_count, &mut nu, &mut nb, &mut nl) })?;
        let qp = qual.map_or(std::ptr::null(), |q| q.as_ptr());
        let mut run_start = vec![0u64; rec_start.len()];
        let mut cover = vec![0u64; nu as usize * COV_WORDS];
        let mut total = 0u64;
        let mut rc = unsafe {
            sys::kh_unitigs_paths(self.ctx, bases.as_ptr(), qp, bases.len() as u64, rec_start.as_ptr(), nrec, run_start.as_mut_ptr(),
                                  std::ptr::null_mut(), 0, std::ptr::null_mut(), &mut total)
        };
        let mut runs = vec![0u32; total as usize * RUN_WORDS];
        if rc == -8 {  // KH_ERR_RANGE: there are runs -- now with room for them
            rc = unsafe {
                sys::kh_unitigs_paths(self.ctx, bases.as_ptr(), qp, bases.len() as u64, rec_start.as_ptr(), nrec, run_start.as_mut_ptr(),
                                      runs.as_mut_ptr(), total, cover.as_mut_ptr(), &mut total)
            };
        }
        let err = check(self.ctx, rc);  // (before kh_unitigs_end replaces the error text)
        let end = unsafe { sys::kh_unitigs_end(self.ctx) };
        err?;
        check(self.ctx, end)?;
        Ok((run_start, runs, cover))
    }

    /// How many records of `bases` walk every link between the unitigs of the table at `min_count` (`kh_unitigs_begin_linked` /
    /// `kh_unitigs_paths` twice / `kh_unitigs_links_copy` / `kh_unitigs_link_support` / `kh_unitigs_end`).  Returns `(links, support,
    /// stats)`: the link words, one counter per link in the same order, and the `SUP_WORDS` words of the call.  A read credits the
    /// word as read; `support[l] + support[index of link_mirror(links[l])]` is the strand-free number.
    pub fn unitigs_link_support(&self, min_count: u64, bases: &[u8], qual: Option<&[u8]>, rec_start: &[u64])
                                -> Result<(Vec<u64>, Vec<u64>, [u64; SUP_WORDS]), HipError> {
        if let Some(q) = qual {
            if q.len() != bases.len() {
                return Err(HipError::Device("qual must have the same length as bases".into()));
            }
        }
        if rec_start.is_empty() {
            return Err(HipError::Device("rec_start needs nrec + 1 offsets".into()));
        }
        let nrec = (rec_start.len() - 1) as u64;
        let (mut nu, mut nb, mut nl) = (0u64, 0u64, 0u64);
        check(self.ctx, unsafe { sys::kh_unitigs_begin_linked(self.ctx, min_count, &mut nu, &mut nb, &mut nl) })?;
        let qp = qual.map_or(std::ptr::null(), |q| q.as_ptr());
        let mut run_start = vec![0u64; rec_start.len()];
        let mut total = 0u64;
        let mut rc = unsafe {
            sys::kh_unitigs_paths(self.ctx, bases.as_ptr(), qp, bases.len() as u64, rec_start.as_ptr(), nrec, run_start.as_mut_ptr(),
                                  std::ptr::null_mut(), 0, std::ptr::null_mut(), &mut total)
        };
        let mut runs = vec![0u32; total as usize * RUN_WORDS];
        if rc == -8 {  // KH_ERR_RANGE: there are runs -- now with room for them
            rc = unsafe {
                sys::kh_unitigs_paths(self.ctx, bases.as_ptr(), qp, bases.len() as u64, rec_start.as_ptr(), nrec, run_start.as_mut_ptr(),
                                      runs.as_mut_ptr(), total, std::ptr::null_mut(), &mut total)
            };
        }
        let mut links = vec![0u64; nl as usize];
        let mut support = vec![0u64; nl as usize];
        let mut stats = [0u64; SUP_WORDS];
        if rc == 0 {
            rc = unsafe { sys::kh_unitigs_links_copy(self.ctx, links.as_mut_ptr(), nl) };
        }
        if rc == 0 {
            rc = unsafe {
                sys::kh_unitigs_link_support(self.ctx, run_start.as_ptr(), nrec, runs.as_ptr(), total, support.as_mut_ptr(), nl, stats.as_mut_ptr())
            };
        }
        let err = check(self.ctx, rc);  // (before kh_unitigs_end replaces the error text)
        let end = unsafe { sys::kh_unitigs_end(self.ctx) };
        err?;
        check(self.ctx, end)?;
        Ok((links, support, stats))
    }

    /// The connected components of the unitig graph of the table at `min_count` (`kh_unitigs_begin_linked` /
    /// `kh_unitigs_components` twice / `kh_unitigs_end`).  Returns `(comp, rows, stats)`: the dense component id of every unitig
    /// (ids ascend with the component's smallest unitig index), `COMP_WORDS` words per component, and the `CC_WORDS` words of the call.
    pub fn unitigs_components(&self, min_count: u64) -> Result<(Vec<u32>, Vec<u64>, [u64; CC_WORDS]), HipError> {
        let (mut nu, mut nb, mut nl) = (0u64, 0u64, 0u64);
        check(self.ctx, unsafe { sys::kh_unitigs_begin_linked(self.ctx, min_count, &mut nu, &mut nb, &mut nl) })?;
        let mut stats = [0u64; CC_WORDS];
        let mut rc = unsafe { sys::kh_unitigs_components(self.ctx, std::ptr::null_mut(), 0, std::ptr::null_mut(), 0, stats.as_mut_ptr()) };
        let mut comp = vec![0u32; nu as usize];
        let mut rows = vec![0u64; stats[CC_COMPONENTS] as usize * COMP_WORDS];
        if rc == 0 && nu > 0 {
            rc = unsafe {
                sys::kh_unitigs_components(self.ctx, comp.as_mut_ptr(), nu, rows.as_mut_ptr(), stats[CC_COMPONENTS], stats.as_mut_ptr())
            };
        }
        let err = check(self.ctx, rc);  // (before kh_unitigs_end replaces the error text)
        let end = unsafe { sys::kh_unitigs_end(self.ctx) };
        err?;
        check(self.ctx, end)?;
        Ok((comp, rows, stats))
    }

    /// Packed canonical key -> count: the shape of `count_kmers_from_sequences`
    /// (`src/streaming.rs:198-204`).
    pub fn into_packed(self, min_count: u64) -> Result<HashMap<u64, u64>, HipError> {
        check(self.ctx, unsafe { sys::kh_finish(self.ctx, std::ptr::null_mut()) })?;
        let mut n = 0u64;
        check(self.ctx, unsafe { sys::kh_result_size(self.ctx, min_count, &mut n) })?;
        let mut keys = vec![0u64; n as usize];
        let mut counts = vec![0u64; n as usize];
        let mut got = 0u64;
        check(self.ctx, unsafe {
            sys::kh_result_copy(self.ctx, keys.as_mut_ptr(), counts.as_mut_ptr(), n, min_count, &mut got)
        })?;
        Ok(keys.into_iter().zip(counts).take(got as usize).collect())
    }

    /// The pairs with count >= `min_count`, ASCENDING by packed key -- the k-mer strings in lexicographic order --, sorted on
    /// the device (`kh_result_sorted`).  The same input gives the same vectors whatever the table's size or form.
    pub fn sorted_pairs(&mut self, min_count: u64) -> Result<(Vec<u64>, Vec<u64>), HipError> {
        check(self.ctx, unsafe { sys::kh_finish(self.ctx, std::ptr::null_mut()) })?;
        let mut n = 0u64;
        check(self.ctx, unsafe { sys::kh_result_size(self.ctx, min_count, &mut n) })?;
        let mut keys = vec![0u64; n as usize];
        let mut counts = vec![0u64; n as usize];
        let mut got = 0u64;
        check(self.ctx, unsafe {
            sys::kh_result_sorted(self.ctx, keys.as_mut_ptr(), counts.as_mut_ptr(), n, min_count, &mut got)
        })?;
        keys.truncate(got as usize);
        counts.truncate(got as usize);
        Ok((keys, counts))
    }

    /// [`write_text`](Self::write_text) with the records in ascending key order (`KH_OUT_SORTED`): the same table content
    /// gives the same bytes on every run and for every table geometry.
    pub fn write_text_sorted<W: std::io::Write>(&mut self, format: TextFormat, min_count: u64, w: &mut W) -> Result<(u64, u64), HipError> {
        self.write_text_as(format as u32 | KH_OUT_SORTED, min_count, w)
    }

    /// `output_counts` (`src/run.rs:441-486`) for the fasta / tsv / json formats: the records are unpacked, their counts
    /// printed and the JSON document framed ON THE DEVICE; `w` receives the text in pieces of whole records, in table
    /// order.  Returns (records, bytes) written.  The table stays as it is (`&mut self`: the stream is state of the context).
    pub fn write_text<W: std::io::Write>(&mut self, format: TextFormat, min_count: u64, w: &mut W) -> Result<(u64, u64), HipError> {
        self.write_text_as(format as u32, min_count, w)
    }

    fn write_text_as<W: std::io::Write>(&mut self, format: u32, min_count: u64, w: &mut W) -> Result<(u64, u64), HipError> {
        check(self.ctx, unsafe { sys::kh_finish(self.ctx, std::ptr::null_mut()) })?;
        let (mut n_records, mut n_bytes) = (0u64, 0u64);
        check(self.ctx, unsafe { sys::kh_result_text_begin(self.ctx, format, min_count, &mut n_records, &mut n_bytes) })?;
        let mut piece = vec![0u8; (n_bytes.min(8 << 20) as usize).max(128)];
        let mut written = 0u64;
        loop {
            let mut n = 0u64;
            check(self.ctx, unsafe { sys::kh_result_text_next(self.ctx, piece.as_mut_ptr(), piece.len() as u64, &mut n) })?;
            if n == 0 {
                break;
            }
            w.write_all(&piece[..n as usize]).map_err(|e| HipError::Device(format!("writing the text failed: {e}")))?;
            written += n;
        }
        debug_assert_eq!(written, n_bytes);
        Ok((n_records, written))
    }

    /// `KmerMap::into_hashmap` (`src/run.rs:573-582`).
    pub fn into_hashmap(self) -> Result<HashMap<String, u64>, HipError> {
        let k = self.k;
        Ok(self.into_packed(1)?.into_iter().map(|(bits, c)| (unpack_to_string(bits, k), c)).collect())
    }

    /// Count-of-counts after the `min_count` filter, ascending (`src/histogram.rs:88-94`).
    pub fn into_histogram(self, min_count: u64) -> Result<BTreeMap<u64, u64>, HipError> {
        check(self.ctx, unsafe { sys::kh_finish(self.ctx, std::ptr::null_mut()) })?;
        let mut cap = 1u64 << 16;
        loop {
            let (mut c, mut f) = (vec![0u64; cap as usize], vec![0u64; cap as usize]);
            let mut n = 0u64;
            let rc = unsafe { sys::kh_histogram(self.ctx, min_count, c.as_mut_ptr(), f.as_mut_ptr(), cap, &mut n) };
            if rc == -8 {
                cap *= 16; // KH_ERR_RANGE
                continue;
            }
            check(self.ctx, rc)?;
            return Ok(c.into_iter().zip(f).take(n as usize).collect());
        }
    }
}

/// Several GPUs of one node from ONE process (no reference counterpart: the reference's only parallelism is
/// rayon over records, `src/run.rs:500-503`): one device table per GPU, reads dealt out in batches of whole
/// records, then `kh_group_merge` -- the library's RCCL exchange -- turns the N tables into one table sharded
/// by hash range, and the result is the concatenation of the shards.
pub struct HipKmerMapGroup {
    group: *mut sys::KhGroup,
    k: usize,
    next: usize,
}

unsafe impl Send for HipKmerMapGroup {}

impl HipKmerMapGroup {
    /// `devices`: HIP ordinals, one rank each (`&[0, 1, 2, 3, 4, 5, 6, 7]` for a whole MI355X node).
    pub fn new(k: usize, min_quality: Option<u8>, devices: &[i32]) -> Result<Self, HipError> {
        if !(1..=32).contains(&k) {
            return Err(HipError::KmerLength { k });
        }
        let cfg = sys::KhConfig {
            struct_size: std::mem::size_of::<sys::KhConfig>() as u32,
            k: k as u32,
            min_quality: min_quality.map_or(-1, i32::from),
            device: -1,
            capacity_hint: 0,
            stream: std::ptr::null_mut(),
            flags: 0,
            input_mib: 0,
        };
        let mut group = std::ptr::null_mut();
        check_abi()?;
        check(std::ptr::null(), unsafe { sys::kh_group_create(&mut group, &cfg, devices.as_ptr(), devices.len() as u32) })?;
        Ok(Self { group, k, next: 0 })
    }

    fn ctx(&self, rank: usize) -> *mut sys::KhCtx {
        unsafe { sys::kh_group_ctx(self.group, rank as u32) }
    }

    /// `KmerMap::build` over all devices: batches of whole records go to the ranks in turn.
    pub fn build<I: Iterator<Item = Bytes>>(mut self, sequences: I) -> Result<Self, HipError> {
        let n = unsafe { sys::kh_group_size(self.group) } as usize;
        let mut flat = Vec::with_capacity(BATCH / 4 + (1 << 20));
        let mut flush = |flat: &mut Vec<u8>, next: &mut usize| -> Result<(), HipError> {
            if !flat.is_empty() {
                let c = unsafe { sys::kh_group_ctx(self.group, (*next % n) as u32) };
                *next += 1;
                check(c, unsafe { sys::kh_push(c, flat.as_ptr(), std::ptr::null(), flat.len() as u64) })?;
                flat.clear();
            }
            Ok(())
        };
        let mut next = self.next;
        for seq in sequences {
            flat.extend_from_slice(&seq);
            flat.push(b'\n');
            if flat.len() >= BATCH / 4 {
                flush(&mut flat, &mut next)?;
            }
        }
        flush(&mut flat, &mut next)?;
        self.next = next;
        Ok(self)
    }

    /// Merge (collective over the group's ranks, one host thread each inside the library) and collect:
    /// the shards' key sets are disjoint, so their union is the map.
    pub fn into_packed(self, min_count: u64) -> Result<HashMap<u64, u64>, HipError> {
        let n = unsafe { sys::kh_group_size(self.group) } as usize;
        for r in 0..n {
            check(self.ctx(r), unsafe { sys::kh_finish(self.ctx(r), std::ptr::null_mut()) })?;
        }
        check(self.ctx(0), unsafe { sys::kh_group_merge(self.group, std::ptr::null_mut()) })?;
        let mut out = HashMap::new();
        for r in 0..n {
            let c = self.ctx(r);
            let mut cnt = 0u64;
            check(c, unsafe { sys::kh_result_size(c, min_count, &mut cnt) })?;
            let (mut keys, mut counts) = (vec![0u64; cnt as usize], vec![0u64; cnt as usize]);
            let mut got = 0u64;
            check(c, unsafe { sys::kh_result_copy(c, keys.as_mut_ptr(), counts.as_mut_ptr(), cnt, min_count, &mut got) })?;
            out.extend(keys.into_iter().zip(counts).take(got as usize));
        }
        Ok(out)
    }

    /// `KmerMap::into_hashmap` (`src/run.rs:573-582`).
    pub fn into_hashmap(self) -> Result<HashMap<String, u64>, HipError> {
        let k = self.k;
        Ok(self.into_packed(1)?.into_iter().map(|(bits, c)| (unpack_to_string(bits, k), c)).collect())
    }
}

impl Drop for HipKmerMapGroup {
    fn drop(&mut self) {
        // SAFETY: the group came from kh_group_create; its contexts are destroyed with it
        unsafe { sys::kh_group_destroy(self.group) }
    }
}

/// One process per GPU instead (MPI-style hosts): rank 0 calls `comm_unique_id()` and hands the 128 bytes
/// to every rank; each rank then `join`s with its own `HipKmerMap`, counts its share and calls `merge_across`.
pub fn comm_unique_id() -> Result<sys::KhUniqueId, HipError> {
    let mut id = sys::KhUniqueId { internal: [0; 128] };
    check(std::ptr::null(), unsafe { sys::kh_comm_unique_id(&mut id) })?;
    Ok(id)
}

impl HipKmerMap {
    /// Collective: blocks until all `nranks` ranks have joined.
    pub fn join(&mut self, nranks: u32, rank: u32, id: &sys::KhUniqueId) -> Result<(), HipError> {
        check(self.ctx, unsafe { sys::kh_comm_init(self.ctx, nranks, rank, id) })
    }

    /// Collective: afterwards this map holds exactly the keys with `kh_owner(key, k, nranks) == rank`,
    /// counts summed over all ranks.
    pub fn merge_across(&mut self) -> Result<sys::KhMergeInfo, HipError> {
        let mut info = sys::KhMergeInfo::default();
        check(self.ctx, unsafe { sys::kh_merge_across(self.ctx, &mut info) })?;
        Ok(info)
    }
}

impl Drop for HipKmerMap {
    fn drop(&mut self) {
        // SAFETY: ctx came from kh_create and is destroyed exactly once
        unsafe { sys::kh_destroy(self.ctx) }
    }
}

/// `unpack_to_string` (`src/kmer.rs:451-456`) through the library's helper.
#[must_use]
pub fn unpack_to_string(bits: u64, k: usize) -> String {
    let mut out = vec![0u8; k];
    // SAFETY: out holds k bytes; kh_unpack writes exactly k ASCII bytes
    unsafe { sys::kh_unpack(bits, k as u32, out.as_mut_ptr()) };
    String::from_utf8(out).unwrap_or_default()
}

/// The fluent builder of `src/builder.rs:95-526`, device-backed (sequence sources are the caller's:
/// krust keeps its readers, `src/reader.rs`).
#[derive(Debug, Clone, Default)]
pub struct KmerCounter {
    k: Option<usize>,
    min_count: u64,
    min_quality: Option<u8>,
}

impl KmerCounter {
    #[must_use]
    pub fn new() -> Self {
        Self { k: None, min_count: 1, min_quality: None }
    }
    pub fn k(mut self, k: usize) -> Result<Self, HipError> {
        if !(1..=32).contains(&k) {
            return Err(HipError::KmerLength { k });
        }
        self.k = Some(k);
        Ok(self)
    }
    #[must_use]
    pub fn min_count(mut self, n: u64) -> Self {
        self.min_count = n;
        self
    }
    #[must_use]
    pub fn min_quality(mut self, q: u8) -> Self {
        self.min_quality = Some(q);
        self
    }
    /// `count()` over in-memory sequences: `HashMap<String, u64>` filtered by `min_count`.
    pub fn count_sequences<I: Iterator<Item = Bytes>>(&self, seqs: I) -> Result<HashMap<String, u64>, HipError> {
        let k = self.k.ok_or(HipError::KmerLength { k: 0 })?;
        Ok(HipKmerMap::new(k, None)?
            .build(seqs)?
            .into_packed(self.min_count)?
            .into_iter()
            .map(|(bits, c)| (unpack_to_string(bits, k), c))
            .collect())
    }
    /// `histogram()` over in-memory sequences.
    pub fn histogram_sequences<I: Iterator<Item = Bytes>>(&self, seqs: I) -> Result<BTreeMap<u64, u64>, HipError> {
        let k = self.k.ok_or(HipError::KmerLength { k: 0 })?;
        HipKmerMap::new(k, None)?.build(seqs)?.into_histogram(self.min_count)
    }
}

#[cfg(test)]
mod tests {
    use super::*;

    // the reference's own KATs (tests/library_tests.rs:23-33, 55-64; src/streaming.rs:1150-1162)
    #[test]
    fn kats() {
        let c = KmerCounter::new().k(3).unwrap();
        let m = c.count_sequences(vec![Bytes::from_static(b"ACGT")].into_iter()).unwrap();
        assert_eq!(m.get("ACG"), Some(&2));
        let m = c.count_sequences(vec![Bytes::from_static(b"TTT")].into_iter()).unwrap();
        assert_eq!(m.get("AAA"), Some(&1));
        let c4 = KmerCounter::new().k(4).unwrap();
        let m = c4
            .count_sequences(vec![Bytes::from_static(b"AAAA"), Bytes::from_static(b"TTTT")].into_iter())
            .unwrap();
        assert_eq!(m.len(), 1);
        assert_eq!(m.values().next(), Some(&2));
        assert!(KmerCounter::new().k(0).is_err() && KmerCounter::new().k(33).is_err());
    }
}

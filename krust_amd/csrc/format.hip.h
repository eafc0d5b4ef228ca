// format.hip.h -- one (k-mer, count) record as TEXT, written once for host and device.
//
// The three record formats of the reference's output_counts (src/run.rs:441-486), byte for byte what the host writer
// (krust_amd/host/kmerust_host.cpp write_counts) prints:
//   fasta   >{count}\n{kmer}\n                                   run.rs:453-456
//   tsv     {kmer}\t{count}\n                                    run.rs:458-461
//   json    serde_json::to_writer_pretty of Vec<{kmer,count}>    run.rs:463-470
// JSON needs no special case per record: EVERY record begins with a 2-byte prefix -- "[\n" for the first record of the
// stream, ",\n" for every other one -- followed by `  {\n    "kmer": "{kmer}",\n    "count": {count}\n  }`, and the
// document ends with "\n]\n".  A document without records is "[]\n".  Both tails are 3 bytes.
//
// Everything here is a KH_HD inline: the device formats records into LDS with it (fmt_tiles_kernel below), the host twin is
// what tests/format_check.cpp compiles with a plain g++ (tests/test_format_records.py: every k, every digit boundary).
#pragma once
#include <stdint.h>

#include "kmer_bits.h"

namespace kh {

constexpr uint32_t FMT_FASTA = 1, FMT_TSV = 2, FMT_JSON = 3;  // KH_OUT_* of include/kmerhip.h
constexpr uint32_t FMT_MAX_DIGITS = 20;                       // 2^64 - 1 = 18446744073709551615

// the fixed bytes of a JSON record: prefix (2) + JS_A + kmer + JS_B + digits + JS_C
#define KH_JS_A "  {\n    \"kmer\": \""
#define KH_JS_B "\",\n    \"count\": "
#define KH_JS_C "\n  }"
constexpr uint32_t JS_A_LEN = sizeof(KH_JS_A) - 1, JS_B_LEN = sizeof(KH_JS_B) - 1, JS_C_LEN = sizeof(KH_JS_C) - 1;
constexpr uint32_t JS_FIXED = 2 + JS_A_LEN + JS_B_LEN + JS_C_LEN;
constexpr uint32_t FMT_TAIL_LEN = 3;  // "\n]\n" / "[]\n" (json only)

KH_HD bool fmt_valid(uint32_t format) { return format >= FMT_FASTA && format <= FMT_JSON; }

// decimal digits of v: 1..20.  Compares, no division: (v >= 10) + (v >= 100) + ...
KH_HD uint32_t fmt_digits(uint64_t v) {
    if (v < 10ull) return 1;  // (what nearly every record of a real table takes: counts 1..9)
    if ((v >> 32) == 0) {
        const uint32_t x = (uint32_t)v;
        return 2u + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) +
               (x >= 100000000u) + (x >= 1000000000u);
    }
    uint32_t d = 10;
    uint64_t p = 10000000000ull;  // 10^10
    while (d < FMT_MAX_DIGITS && v >= p) {
        ++d;
        p *= 10ull;  // (10^19 * 10 would wrap: the loop ends at d == 20 before it is compared)
    }
    return d;
}

// bytes of one record (the JSON prefix included; the document tail is not part of any record)
KH_HD uint32_t record_len(uint32_t format, uint32_t k, uint64_t count) {
    const uint32_t d = fmt_digits(count);
    return format == FMT_FASTA ? k + d + 3u : format == FMT_TSV ? k + d + 2u : k + d + JS_FIXED;
}
// the longest record of a format: what one table slot can take in a staging buffer
KH_HD uint32_t record_len_max(uint32_t format, uint32_t k) { return record_len(format, k, ~0ull); }

// ---- the writer: plain byte stores through P (global, LDS or host memory) -------------------------------------------
template <typename P>
KH_HD P fmt_put_kmer(P p, uint64_t key, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i) {  // unpack_to_bytes, src/kmer.rs:431-440: first base in the top bits
        const uint32_t code = (uint32_t)(key >> (2u * (k - 1u - i))) & 3u;
        *p++ = (uint8_t)(0x54474341u >> (8u * code));  // "ACGT"
    }
    return p;
}
template <typename P>
KH_HD P fmt_put_u64(P p, uint64_t v, uint32_t digits) {
    P e = p + digits;
    P q = e;
    while ((v >> 32) != 0) {  // (rare: a count of 2^32 or more)
        *--q = (uint8_t)('0' + (uint32_t)(v % 10ull));
        v /= 10ull;
    }
    uint32_t x = (uint32_t)v;
    do {
        *--q = (uint8_t)('0' + x % 10u);
        x /= 10u;
    } while (q != p);  // (digits is exact: the loop ends when the most significant digit is out)
    return e;
}
template <typename P>
KH_HD P fmt_put_lit(P p, const char *s, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) *p++ = (uint8_t)s[i];
    return p;
}

// Writes the record of (key, count) at p; `first` = it is the first record of the whole stream (JSON's opening bracket).
// Returns the number of bytes written == record_len(format, k, count).
template <typename P>
KH_HD uint32_t write_record(P p, uint32_t format, uint32_t k, uint64_t key, uint64_t count, bool first) {
    const uint32_t d = fmt_digits(count);
    const P p0 = p;
    if (format == FMT_FASTA) {
        *p++ = '>';
        p = fmt_put_u64(p, count, d);
        *p++ = '\n';
        p = fmt_put_kmer(p, key, k);
        *p++ = '\n';
    } else if (format == FMT_TSV) {
        p = fmt_put_kmer(p, key, k);
        *p++ = '\t';
        p = fmt_put_u64(p, count, d);
        *p++ = '\n';
    } else {
        *p++ = first ? '[' : ',';
        *p++ = '\n';
        p = fmt_put_lit(p, KH_JS_A, JS_A_LEN);
        p = fmt_put_kmer(p, key, k);
        p = fmt_put_lit(p, KH_JS_B, JS_B_LEN);
        p = fmt_put_u64(p, count, d);
        p = fmt_put_lit(p, KH_JS_C, JS_C_LEN);
    }
    return (uint32_t)(p - p0);
}

// What follows the last record: nothing for fasta / tsv; json: "\n]\n", or the whole document "[]\n" when there was no
// record.  Writes at most FMT_TAIL_LEN bytes, returns their number.
template <typename P>
KH_HD uint32_t write_tail(P p, uint32_t format, uint64_t n_records) {
    if (format != FMT_JSON) return 0;
    if (n_records) {
        p[0] = '\n'; p[1] = ']'; p[2] = '\n';
    } else {
        p[0] = '['; p[1] = ']'; p[2] = '\n';
    }
    return FMT_TAIL_LEN;
}

// Is offset e (0 < e < n) of a text made of whole records the START of a record?  (what cuts a piece at a record end)
//   fasta: '>' stands nowhere but at a record start;  tsv: a record ends with its only '\n';  json: with its only '}'.
KH_HD bool fmt_record_starts_at(uint32_t format, const uint8_t *text, uint64_t e) {
    return format == FMT_FASTA ? text[e] == '>' : format == FMT_TSV ? text[e - 1] == '\n' : text[e - 1] == '}';
}

}  // namespace kh

#if defined(__HIPCC__) && !defined(KH_FORMAT_HOST_ONLY)
#include "kernels.hip.h"
#include "partition.hip.h"

namespace kh {

// ---------------------------------------------------------------------------------------------------------------------
// The table as text, in table-SLOT order (no atomic cursor: the same table gives the same bytes on every run).
// A tile is FMT_TILE consecutive slots; lane t of the workgroup takes slots 2t and 2t + 1 of it, so that the lanes' order is the
// slots' order.
//   fmt_size_kernel    per tile: live records with count >= min_count, and the bytes of their text  -> two u32 arrays, which
//                      the host scans exclusively (device_scan): a deterministic byte offset per tile
//   fmt_tiles_kernel   one workgroup per tile: record lengths -> offsets inside the tile (wave scan by __shfl_up over the lanes'
//                      byte sums, then the four waves' totals through LDS) -> records formatted into an LDS staging buffer ->
//                      the tile's text stored with aligned 16-byte stores; only the unaligned head and tail go out byte-wise
// Both read either table form, or a sorted array of pairs: LOAD says how a slot gives (key, count).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int FMT_TILE = 2 * BLOCK;  // 512 slots: the worst case -- json, k = 32, 20-digit counts: 91 B per slot -- is 46,592 B of LDS

struct FmtWide {  // the 16-byte {key, count} table
    const Slot *table;
    __device__ __forceinline__ void load2(u64 i, u64 cap, u64 min_count, u64 (&key)[2], u64 (&cnt)[2], bool (&live)[2]) const {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            live[j] = false;
            key[j] = cnt[j] = 0;
            if (i + j < cap) {
                const uint4 v = *reinterpret_cast<const uint4 *>(&table[i + j]);
                key[j] = ((u64)v.y << 32) | v.x;
                cnt[j] = ((u64)v.w << 32) | v.z;
                live[j] = key[j] != KH_EMPTY_KEY && cnt[j] >= min_count;
            }
        }
    }
};
struct FmtNarrow {  // the 8-byte image: count << 32 | payload; the key comes back through the inverse hash (ntable_compact_kernel)
    const u64 *ntab;
    PartGeom g;
    __device__ __forceinline__ void load2(u64 i, u64 cap, u64 min_count, u64 (&key)[2], u64 (&cnt)[2], bool (&live)[2]) const {
        u64 sl[2] = {0, 0};
        if (i + 1 < cap) {  // (i is even and the image 16-byte aligned: one load for both slots)
            const uint4 v = *reinterpret_cast<const uint4 *>(&ntab[i]);
            sl[0] = ((u64)v.y << 32) | v.x;
            sl[1] = ((u64)v.w << 32) | v.z;
        } else if (i < cap) {
            sl[0] = ntab[i];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            cnt[j] = sl[j] >> 32;
            live[j] = cnt[j] != 0 && cnt[j] >= min_count;
            key[j] = live[j] ? narrow_key(g, i + j, (uint32_t)sl[j]) : 0ull;
        }
    }
};

struct FmtSorted {  // a sorted stream's pairs (sort.hip): every one of the `cap` entries is a record, the min_count filter is already applied
    const u64 *keys, *counts;
    __device__ __forceinline__ void load2(u64 i, u64 cap, u64 min_count, u64 (&key)[2], u64 (&cnt)[2], bool (&live)[2]) const {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            live[j] = i + j < cap;
            key[j] = live[j] ? keys[i + j] : 0ull;
            cnt[j] = live[j] ? counts[i + j] : 0ull;
        }
    }
};

// kernel-resource-usage (gfx950, hipcc -O3): 24 VGPRs, 60 / 70 SGPRs (narrow / wide), 32 B LDS, no scratch, no spills, 8 waves per SIMD
// (FmtSorted: 20 VGPRs, 64 SGPRs).
template <typename LOAD>
__global__ __launch_bounds__(BLOCK) void fmt_size_kernel(LOAD ld, u64 cap, uint32_t k, uint32_t format, u64 min_count, u64 ntiles,
                                                         uint32_t *__restrict__ tile_records, uint32_t *__restrict__ tile_bytes) {
    __shared__ uint32_t s_rec[BLOCK / 64], s_byt[BLOCK / 64];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (uniform per workgroup: barriers inside)
        u64 key[2], cnt[2];
        bool live[2];
        ld.load2(t * FMT_TILE + 2u * tid, cap, min_count, key, cnt, live);
        uint32_t bytes = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) bytes += live[j] ? record_len(format, k, cnt[j]) : 0u;
        const uint32_t recs = (uint32_t)__builtin_popcountll(kh_ballot(live[0])) + (uint32_t)__builtin_popcountll(kh_ballot(live[1]));
        const uint32_t wb = (uint32_t)wave_sum((u64)bytes);
        if ((tid & 63) == 0) {
            s_rec[wave] = recs;
            s_byt[wave] = wb;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t r = 0, b = 0;
#pragma unroll
            for (int w = 0; w < BLOCK / 64; ++w) {
                r += s_rec[w];
                b += s_byt[w];
            }
            tile_records[t] = r;
            tile_bytes[t] = b;
        }
        __syncthreads();  // (s_rec / s_byt are reused by the next tile)
    }
}

// One workgroup per tile t0 + blockIdx.x; the text of tile t goes to out + (tile_off[t] - tile_off[t0]).
// LDS: dynamic, 16 + FMT_TILE * record_len_max(format, k) bytes (fasta at k = 21: 22,544 B = 22.0 KiB -> 7 workgroups = 28 waves per CU of
// 160 KiB; the worst case, json at k = 32: 45.5 KiB -> 3 workgroups = 12 waves) plus 16 B static.
// kernel-resource-usage (gfx950, hipcc -O3): 56 / 58 / 56 VGPRs (narrow / wide / sorted), 56 SGPRs, no scratch, no spills: registers allow 8 waves
// per SIMD, so the dynamic LDS above is what sets the occupancy.
template <typename LOAD>
__global__ __launch_bounds__(BLOCK) void fmt_tiles_kernel(LOAD ld, u64 cap, uint32_t k, uint32_t format, u64 min_count, u64 t0,
                                                          const u64 *__restrict__ tile_off, const u64 *__restrict__ tile_rec,
                                                          uint8_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_stage[];
    __shared__ uint32_t s_wave[BLOCK / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const u64 t = t0 + blockIdx.x;
    const u64 off_t = tile_off[t];
    const uint32_t bytes = (uint32_t)(tile_off[t + 1] - off_t);
    if (bytes == 0) return;  // (uniform: an empty tile)
    u64 key[2], cnt[2];
    bool live[2];
    ld.load2(t * FMT_TILE + 2u * tid, cap, min_count, key, cnt, live);
    uint32_t len[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) len[j] = live[j] ? record_len(format, k, cnt[j]) : 0u;
    // live records of the tile in front of this lane's (the first record of the STREAM takes json's opening bracket)
    const u64 m0 = kh_ballot(live[0]), m1 = kh_ballot(live[1]);
    const uint32_t recs_before_lane = mbcnt(m0) + mbcnt(m1);
    const uint32_t wave_recs = (uint32_t)__builtin_popcountll(m0) + (uint32_t)__builtin_popcountll(m1);
    // inclusive wave scan of the lanes' byte sums
    const uint32_t mine = len[0] + len[1];
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl | (wave_recs << 16);  // (a wave's text is < 64 * 2 * 91 B = 11,648 < 2^16; its records <= 128)
    __syncthreads();
    uint32_t base = 0, recs_before = recs_before_lane;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        const uint32_t x = s_wave[w];
        base += w < wave ? (x & 0xFFFFu) : 0u;
        recs_before += w < wave ? (x >> 16) : 0u;
    }
    uint8_t *const dst = out + (off_t - tile_off[t0]);
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);  // the staging buffer is laid out with the destination's alignment
    uint32_t o = mis + base + (incl - mine);
    const bool stream_first_tile = tile_rec[t] == 0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (live[j]) {
            const bool first = stream_first_tile && recs_before == 0 && (j == 0 || !live[0]);
            o += write_record(s_stage + o, format, k, key[j], cnt[j], first);
        }
    __syncthreads();
    // head: up to the first 16-byte boundary of the destination; body: aligned 16-byte stores; tail: the rest
    const uint32_t head = min(bytes, (16u - mis) & 15u);
    if ((uint32_t)tid < head) dst[tid] = s_stage[mis + tid];
    const uint32_t nvec = (bytes - head) >> 4;
    const uint4 *sv = reinterpret_cast<const uint4 *>(s_stage + mis + head);  // (mis + head is 0 or 16)
    uint4 *dv = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t v = tid; v < nvec; v += BLOCK) dv[v] = sv[v];
    const uint32_t done = head + (nvec << 4);
    if ((uint32_t)tid < bytes - done) dst[done + tid] = s_stage[mis + done + tid];
}

}  // namespace kh
#endif

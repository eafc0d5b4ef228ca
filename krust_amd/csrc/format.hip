// format.hip -- kh_result_text_*: the count table formatted as text ON THE DEVICE and streamed out in pieces.
//
// Replaces output_counts (reference src/run.rs:441-486) for a caller that wants text: instead of 16 bytes per pair to the
// host and a formatting loop there, the device writes the records (format.hip.h) and only text crosses the link.
//   begin   fmt_size_kernel: records and bytes of every tile of FMT_TILE slots; two exclusive scans (device_scan): a
//           deterministic byte offset per tile -- no atomic cursor, the text is in table-slot order
//           KH_OUT_SORTED: the tiles are over the sorted pairs (sorted_into, sort.hip), which the stream holds in memory of its own;
//           a third loader (FmtSorted) reads them, everything behind the loader is the same
//   next    a range of whole tiles -> fmt_tiles_kernel -> one of two device chunks; the chunk's text is handed out
//           record-aligned.  Chunk i + 1 is formatted on the compute stream while chunk i travels on the copy stream.
#include "ctx.hip.h"
#include "format.hip.h"

namespace khi {

constexpr u64 TS_CHUNK_MAX = 64ull << 20;  // text per chunk: a transfer long enough to run at the link's rate
constexpr u64 TS_CHUNK_MIN = 64ull << 10;  // ... and never less than one tile's worst case (46,592 B)
constexpr u64 TS_WINDOW = 128;             // > the longest record (91 B): a window this long in front of a cut holds a record start

void text_release(kh_ctx *c) {
    for (int i = 0; i < 2; ++i) {
        if (c->ts.ch[i].done) (void)hipEventDestroy(c->ts.ch[i].done);
        c->ts.ch[i].done = nullptr;
        if (c->ts_own[i]) (void)dev_free(c->ts_own[i]);
        c->ts_own[i] = nullptr;
    }
    void *bufs[] = {c->ts_trec, c->ts_tbyt, c->ts_roff, c->ts_boff, c->ts_skey, c->ts_scnt};
    for (void *p : bufs)
        if (p) (void)dev_free(p);
    c->ts_trec = c->ts_tbyt = nullptr;
    c->ts_roff = c->ts_boff = nullptr;
    c->ts_skey = c->ts_scnt = nullptr;
}

namespace {

// f(loader, slots): what the tiles are over -- the sorted pairs of the stream, or the table in the form it is in
template <typename F>
void with_loader(const kh_ctx *c, bool sorted, u64 sorted_n, F f) {
    if (sorted) f(kh::FmtSorted{(const u64 *)c->ts_skey, (const u64 *)c->ts_scnt}, sorted_n);
    else if (c->narrow) f(kh::FmtNarrow{(const u64 *)c->ntab, c->narrow_g}, c->cap);
    else f(kh::FmtWide{c->table}, c->cap);
}

// The device memory of chunk i: half of the idle partition buffers (as kh_result_copy takes them: nothing counts while a stream
// is on, and whatever would write them ends the stream), else a buffer of the stream's own, sized for what is left to send.
int chunk_memory(kh_ctx *c, int i) {
    auto &ch = c->ts.ch[i];
    if (!ch.done) HIP_TRY(c, hipEventCreateWithFlags(&ch.done, hipEventDisableTiming));
    if (ch.d) return KH_OK;
    uint8_t *const part = i ? c->keysB : c->keysA;
    const u64 part_cap = i ? c->keyb_cap : c->key_cap;
    if (!c->borrow_on && part && part_cap >= TS_CHUNK_MIN) {
        ch.d = part;
        ch.cap = std::min(part_cap, TS_CHUNK_MAX);
        return KH_OK;
    }
    u64 want = TS_CHUNK_MIN;
    while (want < TS_CHUNK_MAX && want < c->ts.rec_bytes) want *= 4;
    want = std::min(want, TS_CHUNK_MAX);
    int rc = ensure_buf(c, &c->ts_own[i], &c->ts_own_cap[i], want, "hipMalloc(text chunk)", true);
    if (rc != KH_OK) return rc;
    ch.d = c->ts_own[i];
    ch.cap = c->ts_own_cap[i];
    return KH_OK;
}

// Formats the tiles [next_tile, t1) whose text fits `limit` bytes (at least one tile: a chunk always holds one) to `dst`.
// *len = bytes written there (0: only empty tiles were left).  Asynchronous on the compute stream.
int format_range(kh_ctx *c, uint8_t *dst, u64 limit, u64 *len) {
    auto &ts = c->ts;
    const u64 t0 = ts.next_tile, b0 = ts.toff[t0];
    // the largest t1 with toff[t1] - b0 <= limit
    u64 t1 = (u64)(std::upper_bound(ts.toff.begin() + t0, ts.toff.end(), b0 + limit) - ts.toff.begin()) - 1;
    if (t1 == t0) t1 = t0 + 1;  // (one tile alone is larger than the limit: the caller hands it out in parts)
    *len = ts.toff[t1] - b0;
    ts.next_tile = t1;
    if (*len == 0) return KH_OK;
    // (leading and trailing empty tiles need no workgroup)
    u64 a = t0, b = t1;
    while (ts.toff[a + 1] == b0) ++a;
    while (ts.toff[b - 1] == ts.toff[t1]) --b;
    const size_t lds = 16 + (size_t)kh::FMT_TILE * kh::record_len_max(ts.format, c->k);
    for (u64 s = a; s < b;) {  // (a grid dimension holds 2^31 - 1 workgroups)
        const u64 n = std::min<u64>(b - s, 1ull << 30);
        uint8_t *const d = dst + (ts.toff[s] - b0);
        with_loader(c, ts.sorted, ts.sorted_n, [&](auto ld, u64 slots) {
            hipLaunchKernelGGL(kh::fmt_tiles_kernel<decltype(ld)>, dim3((unsigned)n), dim3(kh::BLOCK), lds, c->stream, ld, slots, c->k,
                               ts.format, ts.min_count, s, (const u64 *)c->ts_boff, (const u64 *)c->ts_roff, d);
        });
        s += n;
    }
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

int fill_chunk(kh_ctx *c, int i, u64 limit) {
    int rc = chunk_memory(c, i);
    if (rc != KH_OK) return rc;
    auto &ch = c->ts.ch[i];
    u64 len = 0;
    rc = format_range(c, ch.d, std::min(limit, ch.cap), &len);
    if (rc != KH_OK) return rc;
    ch.len = len;
    ch.pos = 0;
    ch.valid = len != 0;
    if (ch.valid) HIP_TRY(c, hipEventRecord(ch.done, c->stream));
    return KH_OK;
}

// The largest number of bytes <= room at the head of chunk `ch` that ends at a record end (room < what the chunk has left).
int cut_at_record(kh_ctx *c, const kh_ctx::TextStream::Chunk &ch, u64 room, u64 *take) {
    *take = 0;
    if (room == 0) return KH_OK;
    const u64 hi = ch.pos + room;                                  // text[hi] exists: hi < ch.len
    const u64 lo = hi - std::min(room, TS_WINDOW);                 // >= ch.pos
    uint8_t w[TS_WINDOW + 1];
    HIP_TRY(c, hipEventSynchronize(ch.done));
    HIP_TRY(c, hipMemcpy(w, ch.d + lo, hi - lo + 1, hipMemcpyDeviceToHost));
    for (u64 e = hi; e > lo && e > ch.pos; --e)
        if (kh::fmt_record_starts_at(c->ts.format, w, e - lo)) {
            *take = e - ch.pos;
            break;
        }
    return KH_OK;
}

int text_next(kh_ctx *c, uint8_t *buf, u64 cap, u64 *n, bool to_device) {
    int rc = enter(c, ENTER_TEXT_NEXT);
    if (rc != KH_OK) return rc;
    if (!n || (cap && !buf)) return fail(c, KH_ERR_BAD_ARG, "NULL output");
    *n = 0;
    auto &ts = c->ts;
    if (!ts.on) return fail(c, KH_ERR_STATE, "no text stream: kh_result_text_begin first (anything that changes the table ends a stream)");
    u64 got = 0;
    bool full = false;
    while (!full) {
        auto &ch = ts.ch[ts.cur];
        if (!ch.valid) {
            if (ts.next_tile >= ts.ntiles) break;
            const u64 room = cap - got;
            if (to_device && room >= ts.toff[ts.next_tile + 1] - ts.toff[ts.next_tile]) {  // straight into the caller's memory
                u64 len = 0;
                if ((rc = format_range(c, buf + got, room, &len)) != KH_OK) return rc;
                got += len;
                continue;
            }
            if ((rc = fill_chunk(c, ts.cur, std::max(room, TS_CHUNK_MIN))) != KH_OK) return rc;
            continue;
        }
        const u64 left = ch.len - ch.pos, room = cap - got;
        u64 take = left;
        if (left > room) {
            if ((rc = cut_at_record(c, ch, room, &take)) != KH_OK) return rc;
            full = true;
            if (take == 0) break;
        }
        auto &other = ts.ch[ts.cur ^ 1];
        if (take == left && !other.valid && ts.next_tile < ts.ntiles && !to_device) {
            // the next chunk is formatted while this one travels; sized for the room this call has left, or -- when that is
            // no chunk's worth -- for a caller that comes back with the same cap
            const u64 after = room - take;
            if ((rc = fill_chunk(c, ts.cur ^ 1, after >= TS_CHUNK_MIN ? after : std::max(cap, TS_CHUNK_MIN))) != KH_OK) return rc;
        }
        if (to_device) {
            HIP_TRY(c, hipMemcpyAsync(buf + got, ch.d + ch.pos, take, hipMemcpyDeviceToDevice, c->stream));
        } else {
            if ((rc = d2h_staged(c, buf + got, ch.d + ch.pos, take, ch.done)) != KH_OK) return rc;
        }
        got += take;
        ch.pos += take;
        if (ch.pos == ch.len) {
            ch.valid = false;
            ts.cur ^= 1;
        }
    }
    if (!full && !ts.tail_done && ts.next_tile >= ts.ntiles && !ts.ch[0].valid && !ts.ch[1].valid) {
        uint8_t tail[kh::FMT_TAIL_LEN];
        const uint32_t tl = kh::write_tail(tail, ts.format, ts.n_records);
        if (tl <= cap - got) {  // (else: a piece of its own, next time)
            if (tl && to_device) HIP_TRY(c, hipMemcpyAsync(buf + got, tail, tl, hipMemcpyHostToDevice, c->stream));
            else if (tl) memcpy(buf + got, tail, tl);
            got += tl;
            ts.tail_done = true;
        } else {
            full = true;
        }
    }
    if (to_device) HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller's buffer is complete; `tail` may go)
    if (got == 0 && full) return fail(c, KH_ERR_RANGE, "cap is smaller than the next record");
    *n = got;
    return KH_OK;
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_result_text_begin(kh_ctx *c, uint32_t format, uint64_t min_count, uint64_t *n_records, uint64_t *n_bytes) {
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    auto &ts = c->ts;
    ts.on = false;
    const bool sorted = (format & KH_OUT_SORTED) != 0;
    if ((format & ~(uint32_t)(KH_OUT_SORTED | 3u)) != 0 || !kh::fmt_valid(format & 3u))
        return fail(c, KH_ERR_BAD_ARG, "format is none of KH_OUT_FASTA / KH_OUT_TSV / KH_OUT_JSON, alone or with KH_OUT_SORTED");
    format &= 3u;
    if (c->cstream) HIP_TRY(c, hipStreamSynchronize(c->cstream));  // (a chunk of an earlier stream may still travel)
    uint64_t sorted_n = 0;
    if (sorted) {  // the stream's own copy of the result, ascending by key; the sort's scratch goes back before any chunk is placed
        if ((rc = kh_result_size(c, min_count, &sorted_n)) != KH_OK) return rc;
        if ((rc = ensure_buf(c, &c->ts_skey, &c->ts_skey_cap, std::max<u64>(sorted_n, 1), "hipMalloc(sorted text pairs)", true)) != KH_OK) return rc;
        if ((rc = ensure_buf(c, &c->ts_scnt, &c->ts_scnt_cap, std::max<u64>(sorted_n, 1), "hipMalloc(sorted text pairs)", true)) != KH_OK) return rc;
        CallScratch sc(c);
        if ((rc = sorted_into(c, c->ts_skey, c->ts_scnt, sorted_n, min_count, sc)) != KH_OK) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const u64 ntiles = std::max<u64>(((sorted ? sorted_n : c->cap) + kh::FMT_TILE - 1) / kh::FMT_TILE, 1);
    if ((rc = ensure_buf(c, &c->ts_trec, &c->ts_trec_cap, ntiles, "hipMalloc(text tiles)", true)) != KH_OK) return rc;
    if ((rc = ensure_buf(c, &c->ts_tbyt, &c->ts_tbyt_cap, ntiles, "hipMalloc(text tiles)", true)) != KH_OK) return rc;
    if ((rc = ensure_buf(c, &c->ts_roff, &c->ts_roff_cap, ntiles + 1, "hipMalloc(text tiles)", true)) != KH_OK) return rc;
    if ((rc = ensure_buf(c, &c->ts_boff, &c->ts_boff_cap, ntiles + 1, "hipMalloc(text tiles)", true)) != KH_OK) return rc;
    with_loader(c, sorted, sorted_n, [&](auto ld, u64 slots) {
        hipLaunchKernelGGL(kh::fmt_size_kernel<decltype(ld)>, dim3(grid_for(ntiles * kh::BLOCK)), dim3(kh::BLOCK), 0, c->stream, ld, slots,
                           c->k, format, (u64)min_count, ntiles, c->ts_trec, c->ts_tbyt);
    });
    HIP_TRY(c, hipGetLastError());
    if ((rc = device_scan(c, c->ts_trec, ntiles, c->ts_roff, true)) != KH_OK) return rc;
    if ((rc = device_scan(c, c->ts_tbyt, ntiles, c->ts_boff, true)) != KH_OK) return rc;
    try {
        ts.toff.resize(ntiles + 1);
    } catch (...) {
        return soft_oom(c, "host memory for the tile offsets");  // (a reading call: the context stays usable)
    }
    u64 nrec = 0;
    HIP_TRY(c, hipMemcpyAsync(ts.toff.data(), c->ts_boff, (ntiles + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&nrec, c->ts_roff + ntiles, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ts.format = format;
    ts.min_count = min_count;
    ts.sorted = sorted;
    ts.sorted_n = sorted_n;
    ts.ntiles = ntiles;
    ts.n_records = nrec;
    ts.rec_bytes = ts.toff[ntiles];
    ts.next_tile = 0;
    ts.tail_done = false;
    ts.cur = 0;
    for (auto &ch : ts.ch) {  // (where the chunks live is decided again: the partition buffers may have come or gone)
        ch.valid = false;
        ch.d = nullptr;
        ch.cap = ch.len = ch.pos = 0;
    }
    ts.on = true;
    if (n_records) *n_records = nrec;
    if (n_bytes) *n_bytes = ts.rec_bytes + (format == kh::FMT_JSON ? kh::FMT_TAIL_LEN : 0);
    if (c->trace)
        fprintf(stderr, "[kmerhip] text stream: format %u, %llu records, %llu bytes in %llu tiles\n", format, nrec, ts.rec_bytes, ntiles);
    return KH_OK;
}

extern "C" int kh_result_text_next(kh_ctx *c, uint8_t *buf, uint64_t cap, uint64_t *n) { return text_next(c, buf, cap, (u64 *)n, false); }

extern "C" int kh_result_text_next_device(kh_ctx *c, uint8_t *d_buf, uint64_t cap, uint64_t *n) {
    return text_next(c, d_buf, cap, (u64 *)n, true);
}

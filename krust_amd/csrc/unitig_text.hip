// unitig_text.hip -- kh_unitigs_text_*: the live unitigs (and links) of kh_unitigs_begin[_linked] as FASTA / GFA text, formatted ON THE
// DEVICE and streamed out in pieces.  What `kmerust unitigs -f fasta` and `kmerust gfa -f gfa` print; the contract is in
// include/kmerhip.h, the formatter and the kernels in unitig_text.hip.h, the scheme in DESIGN.md 4.15.
//   begin   ut_size_records_kernel / ut_size_links_kernel: a u32 length per record and per link line; two exclusive scans
//           (device_scan): u64 offsets, which stay on the device for the stream's lifetime; the two totals come back together
//   next    a range of whole tiles of UT_TILE bytes -> ut_tiles_kernel -> one of two device chunks of the stream's own; the chunk's
//           bytes are handed out as byte ranges.  Chunk i + 1 is formatted on the compute stream while chunk i travels on the copy
//           stream.  next_device formats into a chunk too and copies device-to-device: one more pass at HBM rate, no alignment case.
#include "ctx.hip.h"
#include "unitig_text.hip.h"

namespace khi {

constexpr u64 UT_CHUNK_MAX = 64ull << 20;  // text per chunk: a transfer long enough to run at the link's rate

void unitigs_text_release(kh_ctx *c) {
    auto &tx = c->un.text;
    for (auto &ch : tx.ch) {
        if (ch.done) (void)hipEventDestroy(ch.done);
        if (ch.d) (void)dev_free(ch.d);  // (synchronises the device)
    }
    if (tx.off) (void)dev_free(tx.off);
    tx = kh_ctx::Unitigs::Text();
}

namespace {

u64 whole_tiles(u64 bytes) { return (bytes + kh::UT_TILE - 1) / kh::UT_TILE * kh::UT_TILE; }

// The lengths, their scans and the totals; the scratch is this call's, the two offset arrays are the stream's.
int text_size(kh_ctx *c, uint32_t format, u64 nu, u64 nl, CallScratch &sc) {
    auto &tx = c->un.text;
    uint32_t *const rlen = (uint32_t *)sc.fresh(nu * sizeof(uint32_t));
    uint32_t *const llen = nl ? (uint32_t *)sc.fresh(nl * sizeof(uint32_t)) : nullptr;
    u64 *const scan = (u64 *)sc.fresh(device_scan_scratch(std::max(nu, nl)));
    if (!rlen || (nl && !llen) || !scan) return soft_oom(c, "device memory for the unitig text's lengths");
    if (dev_malloc((void **)&tx.off, (nu + 1 + (nl ? nl + 1 : 0)) * sizeof(u64)) != hipSuccess) {  // the record offsets, then the link lines'
        (void)hipGetLastError();
        tx.off = nullptr;
        return soft_oom(c, "hipMalloc(unitig text offsets)");
    }
    u64 *const roff = tx.off, *const loff = tx.off + nu + 1;
    hipLaunchKernelGGL(kh::ut_size_records_kernel, dim3(uni_grid(nu)), dim3(kh::BLOCK), 0, c->stream, format, c->k, nu, (const u64 *)c->un.rows, rlen);
    if (nl) hipLaunchKernelGGL(kh::ut_size_links_kernel, dim3(uni_grid(nl)), dim3(kh::BLOCK), 0, c->stream, c->k, nl, (const u64 *)c->un.links, llen);
    HIP_TRY(c, hipGetLastError());
    int rc = device_scan(c, rlen, nu, roff, true, scan);
    if (rc == KH_OK && nl) rc = device_scan(c, llen, nl, loff, true, scan);  // (behind the first scan on the same stream: one scratch)
    if (rc != KH_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(&tx.rec_bytes, roff + nu, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (nl) HIP_TRY(c, hipMemcpyAsync(&tx.link_bytes, loff + nl, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KH_OK;
}

// Formats the next chunk's worth of whole tiles into chunk i.  Asynchronous on the compute stream.
int fill_chunk(kh_ctx *c, int i) {
    auto &tx = c->un.text;
    auto &ch = tx.ch[i];
    if (!ch.done) HIP_TRY(c, hipEventCreateWithFlags(&ch.done, hipEventDisableTiming));
    if (!ch.d && dev_malloc((void **)&ch.d, tx.chunk_bytes) != hipSuccess) {
        (void)hipGetLastError();
        ch.d = nullptr;
        return soft_oom(c, "hipMalloc(unitig text chunk)");
    }
    const u64 len = std::min(tx.chunk_bytes, tx.total - tx.next_off);
    const u64 ntiles = (len + kh::UT_TILE - 1) / kh::UT_TILE;
    const bool gfa = tx.format == kh::UT_GFA;
    const kh::UtDoc doc{c->k, (uint32_t)c->un.n_unitigs, tx.rec_bytes, tx.link_bytes, (const u64 *)c->un.rows, (const u64 *)tx.off, (const uint8_t *)c->un.bases};
    // tiles [a, b) of the document; the header and the records are in the tiles below rend, the link lines in those from lbeg on
    const u64 a = tx.next_off / kh::UT_TILE, b = a + ntiles, lnk0 = tx.hdr + tx.rec_bytes;
    const u64 rend = std::min(b, (lnk0 + kh::UT_TILE - 1) / kh::UT_TILE), lbeg = std::max(a, lnk0 / kh::UT_TILE);
    if (rend > a) {
        const dim3 grid(uni_grid((rend - a) * kh::BLOCK));
        if (gfa) hipLaunchKernelGGL(kh::ut_record_tiles_kernel<kh::UT_GFA>, grid, dim3(kh::BLOCK), kh::UT_LDS, c->stream, doc, (uint32_t)a, (uint32_t)(rend - a), ch.d);
        else hipLaunchKernelGGL(kh::ut_record_tiles_kernel<kh::UT_FASTA>, grid, dim3(kh::BLOCK), kh::UT_LDS, c->stream, doc, (uint32_t)a, (uint32_t)(rend - a), ch.d);
    }
    if (tx.link_bytes && b > lbeg)
        hipLaunchKernelGGL(kh::ut_link_tiles_kernel, dim3(uni_grid((b - lbeg) * kh::BLOCK)), dim3(kh::BLOCK), kh::UT_TILE + 16, c->stream, c->k, c->un.n_links,
                           (const u64 *)c->un.links, (const u64 *)(tx.off + c->un.n_unitigs + 1), lnk0, tx.total, (uint32_t)lbeg, (uint32_t)(b - lbeg),
                           ch.d + (lbeg - a) * kh::UT_TILE);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ch.done, c->stream));
    ch.len = len;
    ch.pos = 0;
    ch.valid = true;
    tx.next_off += len;
    return KH_OK;
}

int text_pieces(kh_ctx *c, uint8_t *buf, u64 cap, u64 *n, bool to_device) {
    auto &tx = c->un.text;
    u64 got = 0;
    while (got < cap) {
        auto &ch = tx.ch[tx.cur];
        if (!ch.valid) {
            if (tx.next_off >= tx.total) break;
            int rc = fill_chunk(c, tx.cur);
            if (rc != KH_OK) return rc;
            continue;
        }
        const u64 left = ch.len - ch.pos, take = std::min(left, cap - got);
        if (take == left && !tx.ch[tx.cur ^ 1].valid && tx.next_off < tx.total && !to_device) {  // the next chunk is formatted while this one travels
            int rc = fill_chunk(c, tx.cur ^ 1);
            if (rc != KH_OK) return rc;
        }
        if (to_device) {
            HIP_TRY(c, hipMemcpyAsync(buf + got, ch.d + ch.pos, take, hipMemcpyDeviceToDevice, c->stream));
        } else {
            int rc = d2h_staged(c, buf + got, ch.d + ch.pos, take, ch.done);
            if (rc != KH_OK) return rc;
        }
        got += take;
        ch.pos += take;
        if (ch.pos == ch.len) {
            ch.valid = false;
            tx.cur ^= 1;
        }
    }
    if (to_device) HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller's buffer is complete)
    tx.sent += got;
    *n = got;
    return KH_OK;
}

int text_next(kh_ctx *c, const char *who, uint8_t *buf, u64 cap, u64 *n, bool to_device) {
    if (!c) return KH_ERR_BAD_ARG;
    int rc = enter(c, ENTER_TEXT_NEXT);
    if (rc != KH_OK) return rc;
    if (!n || (cap && !buf)) return fail(c, KH_ERR_BAD_ARG, (std::string(who) + ": NULL output").c_str());
    *n = 0;
    auto &tx = c->un.text;
    if (!c->un.live || !tx.on)
        return fail(c, KH_ERR_STATE,
                    (std::string(who) + ": no unitig text stream: kh_unitigs_text_begin first (anything that makes the unitigs stale ends a stream)").c_str());
    if (tx.sent == tx.total) return KH_OK;  // the stream has ended
    if (cap == 0) return fail(c, KH_ERR_RANGE, (std::string(who) + ": cap is 0 and bytes are left").c_str());
    rc = text_pieces(c, buf, cap, n, to_device);
    if (rc != KH_OK) {  // (a reading call's failure: the unitigs stay, the stream and its memory go)
        *n = 0;
        (void)hipStreamSynchronize(c->stream);
        unitigs_text_release(c);
    }
    return rc;
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_unitigs_text_begin(kh_ctx *c, uint32_t format, uint64_t *n_bytes) {
    if (!c) return KH_ERR_BAD_ARG;
    int rc = enter(c, ENTER_READ);
    if (rc != KH_OK) return rc;
    if (n_bytes) *n_bytes = 0;
    if (c->cstream) HIP_TRY(c, hipStreamSynchronize(c->cstream));  // (a chunk of an earlier stream may still travel)
    unitigs_text_release(c);  // (a running stream restarts)
    if (!kh::ut_valid(format)) return fail(c, KH_ERR_BAD_ARG, "kh_unitigs_text_begin: format is neither KH_UNI_TEXT_FASTA nor KH_UNI_TEXT_GFA");
    if (!c->un.live)
        return fail(c, KH_ERR_STATE, "kh_unitigs_text_begin: no unitigs: kh_unitigs_begin first (anything that changes the table makes them stale)");
    const bool gfa = format == kh::UT_GFA;
    if (gfa && !c->un.linked) return fail(c, KH_ERR_STATE, "kh_unitigs_text_begin: KH_UNI_TEXT_GFA needs the links: kh_unitigs_begin_linked, not kh_unitigs_begin");
    auto &tx = c->un.text;
    const u64 nu = c->un.n_unitigs, nl = gfa ? c->un.n_links : 0;
    if (nu) {
        {
            CallScratch sc(c);
            rc = text_size(c, format, nu, nl, sc);
            if (rc != KH_OK) (void)hipStreamSynchronize(c->stream);  // (before the scratch goes back)
        }
        if (rc != KH_OK) {
            unitigs_text_release(c);
            return rc;
        }
    }
    tx.format = format;
    tx.hdr = gfa ? kh::UT_GFA_HEADER : 0;
    tx.total = tx.hdr + tx.rec_bytes + tx.link_bytes;
    tx.chunk_bytes = std::max<u64>(std::min(UT_CHUNK_MAX, whole_tiles(tx.total)), kh::UT_TILE);
    if (c->knobs.uni_text_chunk_kb) tx.chunk_bytes = whole_tiles(c->knobs.uni_text_chunk_kb << 10);  // (tests: chunk edges inside records)
    tx.on = true;
    if (n_bytes) *n_bytes = tx.total;
    if (c->trace)
        fprintf(stderr, "[kmerhip] unitig text stream: format %u, %llu bytes (%llu of records, %llu of links), chunks of %llu\n", format,
                (unsigned long long)tx.total, (unsigned long long)tx.rec_bytes, (unsigned long long)tx.link_bytes, (unsigned long long)tx.chunk_bytes);
    return KH_OK;
}

extern "C" int kh_unitigs_text_next(kh_ctx *c, uint8_t *buf, uint64_t cap, uint64_t *n) {
    return text_next(c, "kh_unitigs_text_next", buf, cap, (u64 *)n, false);
}

extern "C" int kh_unitigs_text_next_device(kh_ctx *c, uint8_t *d_buf, uint64_t cap, uint64_t *n) {
    return text_next(c, "kh_unitigs_text_next_device", d_buf, cap, (u64 *)n, true);
}

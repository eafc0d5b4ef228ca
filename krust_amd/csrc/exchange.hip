// exchange.hip -- the multi-GPU exchange behind the C ABI: kh_comm_* / kh_merge_across / kh_group_*.
//
// A translation unit of its own over ctx.hip.h: it drives the export / merge entry points of merge.hip.
// north_star: "reads shard naturally per GPU across the 8 x MI355X node with a final RCCL reduce of per-GPU
// hash tables over xGMI".  A hash table is not element-wise reducible, so the "reduce" is an all-to-all of
// region segments to owner = top bits of the table hash, then an LDS rebuild of every owner's shard
// (shard.hip.h).  xGMI is point to point (7 links per GPU): ncclSend / ncclRecv groups drive all links of a
// GPU at once, where a ring all-reduce would be per-link bound -- and wrong for a hash table anyway.
//
// Reference counterpart: none (single process; rayon over records, src/run.rs:500-503, is its only
// parallelism).  krust_amd/distributed.py is the same sequence over torch.distributed and stays as the
// test harness; tests assert that both leave identical shard tables.
//
// Transport: RCCL when every rank has its own device; a process-local hub (device-to-device copies between
// the threads' contexts) when a kh_group lists a device twice -- the 1-GPU test box -- because RCCL refuses
// duplicate devices.  Both sit behind `Xport`, so the merge sequence is one piece of code.
#include "ctx.hip.h"
#include "shard.hip.h"

#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>

// ---- liveness (round 3) -----------------------------------------------------------------------------
// kh_merge_across is a collective: a rank that fails on its own (an allocation, an export that does not fit, a
// kernel error) must not leave its peers blocked in the next all-gather or ncclRecv.  Three rules:
//   1. STATUS IS PART OF THE PROTOCOL.  Every small all-gather carries the sender's status word in front of its
//      values (xp_gather).  A rank that failed locally keeps walking to the next gather and reports there; every
//      rank sees the same gathered words, so all of them leave at the same point: the failing rank with its own
//      status, the others with KH_ERR_PEER.  No data all-to-all starts before such a gather has come back clean,
//      and the last act of a merge is one more gather, so that "my merge failed" reaches everybody too.
//   2. EVERY WAIT IS BOUNDED (KMERHIP_MERGE_TIMEOUT_S, default 300).  Waiting for a transfer is a poll of the event
//      (hipEventQuery) that also reads ncclCommGetAsyncError; a watchdog thread covers the RCCL calls that can block
//      inside the library (connection set-up in ncclGroupEnd / the first collective).  Either one, on expiry or on
//      an asynchronous error, calls ncclCommAbort -- which releases whatever this rank had in flight -- and the merge
//      returns KH_ERR_RCCL; the communicator is dead from then on (kh_merge_across refuses it), the context is not.
//   3. A send / recv group that fails half way is still closed (ncclGroupEnd), then the communicator is aborted.
// The process-local hub follows the same rules with a poison flag in place of the abort: a barrier that times out,
// or a rank that cannot go on, poisons the hub and every barrier returns at once.
// KMERHIP_FAULT="rank:point[:status]" (tests) makes `rank` fail at a named point of the sequence.

namespace khi {

// KMERHIP_MERGE_TIMEOUT_S: read when a communicator (or a hub) is set up, kept there
double merge_timeout_env() {
    const char *e = getenv("KMERHIP_MERGE_TIMEOUT_S");
    const double v = e ? atof(e) : 300.0;
    return v > 0 ? v : 300.0;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- process-local hub: ranks are threads of one process --------------------------------------------
struct LocalHub {
    uint32_t n;
    std::mutex m;
    std::condition_variable cv;
    uint32_t arrived = 0;
    u64 generation = 0;
    bool poisoned = false;                       // a rank gave up: every barrier returns false from now on
    double timeout_s = 300.0;                    // KMERHIP_MERGE_TIMEOUT_S, as read when the ranks were set up
    std::vector<const void *> base;              // posted per rank
    std::vector<std::vector<u64>> off, len;      // [rank][peer], bytes
    std::vector<std::vector<u64>> small;         // all-gather postings
    std::vector<hipStream_t> xs;                 // every rank's exchange stream (drained by all on a poisoned exit)
    explicit LocalHub(uint32_t nr) : n(nr), base(nr, nullptr), off(nr), len(nr), small(nr), xs(nr, nullptr) {}
    // false: the hub is poisoned (by a time-out here, or by poison())
    bool barrier() {
        std::unique_lock<std::mutex> lk(m);
        if (poisoned) return false;
        const u64 gen = generation;
        if (++arrived == n) {
            arrived = 0;
            ++generation;
            cv.notify_all();
            return true;
        }
        const bool woke = cv.wait_for(lk, std::chrono::duration<double>(timeout_s), [&] { return generation != gen || poisoned; });
        if (generation != gen) return true;  // (the barrier completed, whatever happened since)
        if (!woke) {
            poisoned = true;
            cv.notify_all();
        }
        return false;
    }
    void poison() {
        std::lock_guard<std::mutex> lk(m);
        poisoned = true;
        cv.notify_all();
    }
    bool is_poisoned() {
        std::lock_guard<std::mutex> lk(m);
        return poisoned;
    }
    void revive() {  // between merges, with no rank inside one (kh_group_merge)
        std::lock_guard<std::mutex> lk(m);
        poisoned = false;
        arrived = 0;
    }
    // A rank that leaves a POISONED merge does not know where its peers are: one of them may still enqueue a copy out of this
    // rank's send buffer (it checks the poison flag at the next barrier only).  Such a rank's scratch is therefore not freed
    // but kept here until every rank has left the merge (kh_group_merge, after the join; or the group's end).
    std::vector<void *> kept;
    void keep(void *p) {
        std::lock_guard<std::mutex> lk(m);
        kept.push_back(p);
    }
    void release_kept() {
        std::vector<void *> k;
        {
            std::lock_guard<std::mutex> lk(m);
            k.swap(kept);
        }
        for (void *p : k) (void)dev_free(p);
    }
    ~LocalHub() { release_kept(); }
};
thread_local LocalHub *tl_hub = nullptr;  // the hub of the merge this thread is inside (DevBuf's destructor asks it)

struct Comm {
    uint32_t nranks = 1, rank = 0;
    ncclComm_t nccl = nullptr;
    LocalHub *hub = nullptr;     // not owned
    uint32_t seen = 0;           // ranks the transport itself reports: ncclCommCount, or the hub's size (kh_merge_info.nranks_seen)
    hipStream_t xs = nullptr;    // the exchange stream (transfers overlap the kernels on ctx->stream)
    u64 *d_small = nullptr;      // device staging of the small all-gathers: (1 + nranks) * SMALL_MAX u64
    u64 *h_small = nullptr;      // pinned twin
    // liveness
    double timeout_s = 300.0;
    std::atomic<bool> dead{false};        // aborted: nothing may use `nccl` any more
    std::atomic<double> busy_since{0.0};  // != 0: this rank is inside an RCCL call that may block (ms clock)
    std::atomic<bool> stop{false};
    std::mutex abort_m;
    std::thread watchdog;
};
constexpr uint32_t SMALL_MAX = 256;  // u64 per rank in one small all-gather (status word included; 3 digest words x 64 ranks fit)

// ncclCommAbort, once.  Safe from the watchdog while the rank's own thread is blocked inside RCCL: that is what the call is for.
void comm_abort(Comm *cm) {
    std::lock_guard<std::mutex> lk(cm->abort_m);
    if (cm->dead.exchange(true)) return;
    if (cm->nccl) (void)ncclCommAbort(cm->nccl);
}

int rccl_fail(kh_ctx *c, const char *what, ncclResult_t r) {
    c->last_error = std::string(what) + ": " + ncclGetErrorString(r);
    return KH_ERR_RCCL;
}
int rccl_dead(kh_ctx *c, const char *what) {
    c->last_error = std::string(what) + ": the communicator was aborted (time-out or asynchronous RCCL error; KMERHIP_MERGE_TIMEOUT_S)";
    return KH_ERR_RCCL;
}
// an RCCL call that may block inside the library: the watchdog sees how long it has been in there
#define NCCL_CALL(cm, res, call)             \
    do {                                     \
        (cm)->busy_since.store(now_ms());    \
        (res) = (call);                      \
        (cm)->busy_since.store(0.0);         \
    } while (0)
// ... and fails the enclosing function (after aborting the communicator: its state is unknown)
#define NCCL_TRY(c, call)                                                 \
    do {                                                                  \
        Comm *cm_ = (c)->comm;                                            \
        if (cm_->dead.load()) return rccl_dead((c), #call);               \
        ncclResult_t r_;                                                  \
        NCCL_CALL(cm_, r_, (call));                                       \
        if (cm_->dead.load()) return rccl_dead((c), #call);               \
        if (r_ != ncclSuccess) {                                          \
            comm_abort(cm_);                                              \
            return rccl_fail((c), #call, r_);                             \
        }                                                                 \
    } while (0)

// Bounded wait for the exchange stream (ev == nullptr) or an event recorded on it.
int xp_wait(kh_ctx *c, hipEvent_t ev, const char *what) {
    Comm *cm = c->comm;
    const double t_end = now_ms() + cm->timeout_s * 1e3;
    for (uint32_t spins = 0;; ++spins) {
        const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(cm->xs);
        if (e == hipSuccess) return KH_OK;
        (void)hipGetLastError();
        if (e != hipErrorNotReady) return fail(c, KH_ERR_HIP, what, e);
        if (cm->nccl) {
            if (cm->dead.load()) return rccl_dead(c, what);
            if ((spins & 63u) == 63u) {
                ncclResult_t ar = ncclSuccess;
                const ncclResult_t qr = ncclCommGetAsyncError(cm->nccl, &ar);
                if (qr != ncclSuccess || (ar != ncclSuccess && ar != ncclInProgress)) {
                    comm_abort(cm);
                    return rccl_fail(c, "asynchronous RCCL error while waiting for the exchange", qr != ncclSuccess ? qr : ar);
                }
            }
        }
        if (now_ms() > t_end) {
            if (cm->nccl) comm_abort(cm);
            if (cm->hub) cm->hub->poison();
            c->last_error = std::string(what) + ": timed out (KMERHIP_MERGE_TIMEOUT_S)";
            return KH_ERR_RCCL;
        }
        if (spins < 4096) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

int hub_fail(kh_ctx *c, const char *what) {
    c->last_error = std::string(what) + ": another rank of the group gave up (or a barrier timed out)";
    return KH_ERR_PEER;
}

// all-gather of n (<= SMALL_MAX) host integers: all[r * n + i] = rank r's mine[i].  Blocks (bounded).
int xp_allgather(kh_ctx *c, const u64 *mine, uint32_t n, u64 *all) {
    Comm *cm = c->comm;
    if (n > SMALL_MAX) return fail(c, KH_ERR_BAD_ARG, "xp_allgather: too many values");
    if (cm->hub) {
        cm->hub->small[cm->rank].assign(mine, mine + n);
        if (!cm->hub->barrier()) return hub_fail(c, "all-gather");
        for (uint32_t r = 0; r < cm->nranks; ++r) {
            if (cm->hub->small[r].size() != n) {  // (a protocol bug, not a run-time condition: never read past a posting)
                cm->hub->poison();
                return fail(c, KH_ERR_STATE, "local all-gather: the ranks posted different numbers of values");
            }
            memcpy(all + (size_t)r * n, cm->hub->small[r].data(), n * sizeof(u64));
        }
        if (!cm->hub->barrier()) return hub_fail(c, "all-gather");  // nobody overwrites its posting before everybody has read it
        return KH_OK;
    }
    if (cm->dead.load()) return rccl_dead(c, "all-gather");
    memcpy(cm->h_small, mine, n * sizeof(u64));
    HIP_TRY(c, hipMemcpyAsync(cm->d_small, cm->h_small, n * sizeof(u64), hipMemcpyHostToDevice, cm->xs));
    NCCL_TRY(c, ncclAllGather(cm->d_small, cm->d_small + SMALL_MAX, n, ncclUint64, cm->nccl, cm->xs));
    HIP_TRY(c, hipMemcpyAsync(cm->h_small + SMALL_MAX, cm->d_small + SMALL_MAX, (size_t)cm->nranks * n * sizeof(u64),
                              hipMemcpyDeviceToHost, cm->xs));
    const int rc = xp_wait(c, nullptr, "all-gather");
    if (rc != KH_OK) return rc;
    memcpy(all, cm->h_small + SMALL_MAX, (size_t)cm->nranks * n * sizeof(u64));
    return KH_OK;
}

// The gather every step of the sequence goes through: this rank's status `lrc` in front of its n values.
// all[r * n + i] = rank r's value i.  KH_OK: every rank is fine.  Otherwise every rank returns non-zero from the SAME
// call: the ranks that failed their own status, the others KH_ERR_PEER (kh_last_error names the first failing rank).
int xp_gather(kh_ctx *c, int lrc, const u64 *mine, uint32_t n, u64 *all, const char *where) {
    Comm *cm = c->comm;
    const uint32_t W = cm->nranks;
    if (n + 1 > SMALL_MAX) return fail(c, KH_ERR_BAD_ARG, "xp_gather: too many values");
    std::vector<u64> m(n + 1, 0), g((size_t)W * (n + 1), 0);
    m[0] = (u64)(int64_t)lrc;
    if (lrc == KH_OK && n) memcpy(&m[1], mine, n * sizeof(u64));
    const std::string keep = c->last_error;  // (the text of this rank's own failure survives the gather)
    const int trc = xp_allgather(c, m.data(), n + 1, g.data());
    if (trc != KH_OK) return lrc != KH_OK ? (c->last_error = keep, lrc) : trc;
    int bad_rank = -1, bad_rc = KH_OK;
    for (uint32_t r = 0; r < W; ++r) {
        const int s = (int)(int64_t)g[(size_t)r * (n + 1)];
        if (s != KH_OK && bad_rank < 0) {
            bad_rank = (int)r;
            bad_rc = s;
        }
        if (all && n) memcpy(all + (size_t)r * n, &g[(size_t)r * (n + 1) + 1], n * sizeof(u64));
    }
    if (lrc != KH_OK) {
        c->last_error = keep;
        return lrc;
    }
    if (bad_rank >= 0) {
        c->last_error = std::string("rank ") + std::to_string(bad_rank) + " failed with status " + std::to_string(bad_rc) + " (" +
                        kh_strerror(bad_rc) + ") before " + where + "; every rank leaves the merge";
        return KH_ERR_PEER;
    }
    return KH_OK;
}

// all-to-all of device byte ranges: peer p receives send[soff[p] .. +slen[p]) and this rank receives peer
// p's range for it at recv + roff[p] (rlen[p] bytes; the caller has exchanged the sizes).  Enqueued on the
// exchange stream: returns once the transfers are IN FLIGHT; xp_wait() waits for their completion.
// `send` must be complete in device memory (the export calls block until it is) and stay untouched until
// the completion event has been waited for -- with the hub also until the closing barrier of the merge.
// Only called right after a clean xp_gather: every rank is known to arrive.
// skip_self: this rank's own segment does not travel (the caller reads it where it lies: merge_across_impl, `self_direct`).
int xp_alltoallv(kh_ctx *c, const void *send, const u64 *soff, const u64 *slen, void *recv, const u64 *roff, const u64 *rlen, bool skip_self = false) {
    Comm *cm = c->comm;
    if (cm->hub) {
        LocalHub *h = cm->hub;
        h->base[cm->rank] = send;
        h->off[cm->rank].assign(soff, soff + cm->nranks);
        h->len[cm->rank].assign(slen, slen + cm->nranks);
        if (!h->barrier()) return hub_fail(c, "local exchange");
        int rc = KH_OK;  // (no return between the two barriers: the other threads would wait for the time-out)
        for (uint32_t p = 0; p < cm->nranks && rc == KH_OK; ++p) {
            const u64 n = h->len[p][cm->rank];
            if (skip_self && p == cm->rank) continue;
            if (n != rlen[p]) rc = fail(c, KH_ERR_STATE, "local exchange: announced and posted segment sizes differ");
            else if (n && hipMemcpyAsync((char *)recv + roff[p], (const char *)h->base[p] + h->off[p][cm->rank], n, hipMemcpyDefault,
                                         cm->xs) != hipSuccess)
                rc = fail(c, KH_ERR_HIP, "hipMemcpyAsync(local exchange)");
        }
        if (!h->barrier() && rc == KH_OK) rc = hub_fail(c, "local exchange");  // postings may be replaced (the COPIES are still in flight: buffers stay alive, see above)
        return rc;
    }
    if (cm->dead.load()) return rccl_dead(c, "all-to-all");
    // a group that fails half way is still closed; then the communicator (whose state nobody knows) is aborted
    ncclResult_t r;
    NCCL_CALL(cm, r, ncclGroupStart());
    const bool open = r == ncclSuccess;
    const char *what = "ncclGroupStart";
    // A segment travels in messages of at most XP_MSG bytes (matching send / recv pairs of one group pair up in order).
    // Round 4: a rank's send to ITSELF of 2^30 bytes or more arrived half -- a world of one rank merging an S100M table lost
    // every key of the upper half of every piece, silently (tools/world1_merge_probe.py); whatever the limit is inside the
    // transport, no message of this library comes near it now.
    constexpr u64 XP_MSG = 256ull << 20;
    for (uint32_t p = 0; p < cm->nranks && r == ncclSuccess; ++p) {
        if (skip_self && p == cm->rank) continue;
        for (u64 o = 0; o < slen[p] && r == ncclSuccess; o += XP_MSG) {
            NCCL_CALL(cm, r, ncclSend((const char *)send + soff[p] + o, (size_t)std::min(XP_MSG, slen[p] - o), ncclUint8, (int)p, cm->nccl, cm->xs));
            what = "ncclSend";
        }
        for (u64 o = 0; o < rlen[p] && r == ncclSuccess; o += XP_MSG) {
            NCCL_CALL(cm, r, ncclRecv((char *)recv + roff[p] + o, (size_t)std::min(XP_MSG, rlen[p] - o), ncclUint8, (int)p, cm->nccl, cm->xs));
            what = "ncclRecv";
        }
    }
    if (open) {
        ncclResult_t r2;
        NCCL_CALL(cm, r2, ncclGroupEnd());
        if (r == ncclSuccess && r2 != ncclSuccess) {
            r = r2;
            what = "ncclGroupEnd";
        }
    }
    if (cm->dead.load()) return rccl_dead(c, "all-to-all");
    if (r != ncclSuccess) {
        comm_abort(cm);
        return rccl_fail(c, what, r);
    }
    return KH_OK;
}

int xp_allreduce_sum_u64(kh_ctx *c, u64 *d_buf, u64 n) {
    Comm *cm = c->comm;
    if (cm->hub) return fail(c, KH_ERR_STATE, "dense all-reduce is not available on the process-local hub");
    NCCL_TRY(c, ncclAllReduce(d_buf, d_buf, n, ncclUint64, ncclSum, cm->nccl, cm->xs));
    return xp_wait(c, nullptr, "all-reduce");
}

struct DevBuf {  // scratch of one merge; freed when it goes out of scope
    void *p = nullptr;
    bool owned = true;  // false: carved out of the context's idle partition buffers (borrow(): nothing to free, alive until kh_reset)
    void release() {
        if (!p) return;
        if (owned) {
            if (tl_hub && tl_hub->is_poisoned()) tl_hub->keep(p);  // (a peer may still be reading it: LocalHub::keep)
            else (void)dev_free(p);
        }
        p = nullptr;
        owned = true;
    }
    ~DevBuf() { release(); }
    int alloc(kh_ctx *c, u64 bytes, const char *what) {
        release();
        if ((p = borrow(c, bytes ? bytes : 16)) != nullptr) {
            owned = false;
            return KH_OK;
        }
        hipError_t e = dev_malloc(&p, bytes ? bytes : 16);
        // the partition buffers of the counting that is over: room for this -- unless parts of them are lent out to this very merge
        if (e != hipSuccess && (c->keysA || c->keysB) && !(c->borrow_off[0] | c->borrow_off[1])) {
            (void)hipGetLastError();
            p = nullptr;
            if (release_part_buffers(c) == KH_OK) e = dev_malloc(&p, bytes ? bytes : 16);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            // (not through fail(): an allocation of exchange scratch that does not fit leaves the table as it was,
            //  the context stays usable)
            c->last_error = std::string(what) + ": " + hipGetErrorString(e);
            return KH_ERR_OOM;
        }
        return KH_OK;
    }
};

// ---- conservation digests (round 5; shard.hip.h unit_digest_kernel) ----------------------------------
// (units, sum of counts, checksum) of W unit segments of one buffer, into d_out[3 * W] (device), on the context's stream.
// off / len in BYTES of the unit array; ub = bytes per unit (4 heads, 8 packed or the key array of wide pairs).
int digest_units(kh_ctx *c, int fmt, const void *base, const u64 *counts, const u64 *off_bytes, const u64 *len_bytes, uint32_t W, u64 ub,
                 uint32_t head_cmask, u64 *d_out, bool accumulate = false) {
    kh::DigestSegs segs;
    memset(&segs, 0, sizeof(segs));
    u64 maxlen = 0;
    for (uint32_t p = 0; p < W; ++p) {
        segs.off[p] = off_bytes[p] / ub;
        segs.len[p] = len_bytes[p] / ub;
        maxlen = std::max(maxlen, segs.len[p]);
    }
    if (!accumulate) HIP_TRY(c, hipMemsetAsync(d_out, 0, (size_t)3 * W * sizeof(u64), c->stream));
    if (!maxlen) return KH_OK;
    const dim3 grid((unsigned)std::max<u64>(1, std::min<u64>(2048, (maxlen + kh::BLOCK * 32 - 1) / (kh::BLOCK * 32))), W), block(kh::BLOCK);
    if (fmt == XF_HEADS32) hipLaunchKernelGGL((kh::unit_digest_kernel<2>), grid, block, 0, c->stream, base, counts, segs, head_cmask, d_out);
    else if (fmt == XF_PACKED64) hipLaunchKernelGGL((kh::unit_digest_kernel<1>), grid, block, 0, c->stream, base, counts, segs, head_cmask, d_out);
    else hipLaunchKernelGGL((kh::unit_digest_kernel<0>), grid, block, 0, c->stream, base, counts, segs, head_cmask, d_out);
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

// kh_reset in the middle of a merge (the table becomes the shard's): what the merge has borrowed of the partition buffers --
// its send and receive buffers, in use right now -- stays lent out (a caller's kh_reset ends the loan: ctx.hip.h borrow_on)
int merge_reset(kh_ctx *c) {
    const bool on = c->borrow_on;
    const u64 o0 = c->borrow_off[0], o1 = c->borrow_off[1];
    const int rc = kh_reset(c);
    c->borrow_on = on;
    c->borrow_off[0] = o0;
    c->borrow_off[1] = o1;
    return rc;
}

uint32_t merge_pieces_default() {  // (a tunable of the exchange: how many shares the pipeline works in; any value gives the same shards)
    const char *e = getenv("KMERHIP_MERGE_PIECES");
    const int v = e ? atoi(e) : 4;
    return v >= 1 ? (uint32_t)v : 1u;
}

// KMERHIP_FAULT="rank:point[:status]" -- tests: rank `rank` fails at `point` of the merge sequence
struct Fault {
    int rank = -1, code = KH_ERR_STATE;
    std::string point;
    Fault() {
#if !KH_TESTING
        return;  // (the product library has no failure injection: krust_amd/lib/libkmerhip_testing.so does)
#endif
        const char *e = getenv("KMERHIP_FAULT");
        if (!e || !*e) return;
        const std::string s(e);
        const size_t a = s.find(':');
        if (a == std::string::npos) return;
        const size_t b = s.find(':', a + 1);
        rank = atoi(s.substr(0, a).c_str());
        point = s.substr(a + 1, b == std::string::npos ? std::string::npos : b - a - 1);
        if (b != std::string::npos) code = atoi(s.substr(b + 1).c_str());
    }
};

// ---- the merge sequence -----------------------------------------------------------------------------
// Shape of every stretch below: local, fallible steps accumulate into `lrc` (a failed rank skips the rest of the
// stretch); the stretch ends in xp_gather, which is where everybody learns about it.
// `pre`: the status of the caller's pre-checks (a poisoned context, counting that was pending and failed, a table that
// is already a shard).  A rank that fails them still joins the first gather -- and reports there -- so that its peers
// leave the same kh_merge_across with KH_ERR_PEER instead of waiting in that gather for the time-out.
int merge_across_impl(kh_ctx *c, kh_merge_info *info, int pre) {
    Comm *cm = c->comm;
    (void)hipSetDevice(c->device);  // (enter() may have failed before it got there)
#if KH_TESTING
    cm->timeout_s = merge_timeout_env();  // (tests change the bound between merges of one group)
    if (cm->hub) cm->hub->timeout_s = cm->timeout_s;
#endif
    const uint32_t W = cm->nranks, R = cm->rank;
    struct HubScope {
        explicit HubScope(LocalHub *h) { tl_hub = h; }
        ~HubScope() { tl_hub = nullptr; }
    } hub_scope(cm->hub);  // (declared before every DevBuf of the merge: destroyed after them)
    const double t_begin = now_ms();
    double t_export = 0, t_wait = 0, t_merge = 0;
    kh_merge_info mi;
    memset(&mi, 0, sizeof(mi));
    mi.nranks = W;
    mi.nranks_seen = cm->seen;
    mi.pieces = 1;
    const Fault flt;
    auto inject = [&](const char *point) -> int {
        if ((int)R == flt.rank && flt.point == point) {
            c->last_error = std::string("injected fault at ") + point;
            return flt.code;
        }
        return KH_OK;
    };
    // Round 6: A RANK'S OWN SHARE DOES NOT TRAVEL.  The region routes used to send it like any other segment -- ncclSend / ncclRecv to
    // self, a device-local copy at 0.8 TB/s that every small gather of the pipeline then queued behind (7.6 ms of the exchange
    // stream per step at configs[3]'s size in a world of one) -- although the merge can read it where the export put it: the send
    // buffer stays untouched until the merge is over anyway.  The merge kernels get that pointer for sender `rank`, the arrival
    // digest of that segment is taken from there too.  (Test build: KMERHIP_SELF_SEND=1 sends it through the transport as before --
    // what keeps RCCL's send / receive to self under test on the one-GPU box.)
    bool self_direct = true;
#if KH_TESTING
    if (const char *e = getenv("KMERHIP_SELF_SEND")) self_direct = e[0] != '1';
#endif
    bool transfers = false;  // something may be in flight on the exchange stream (into / out of this merge's buffers)
    auto done = [&](int rc) {
        if (transfers) {
            // nothing may still write into (or, hub: read from) buffers about to be freed
            if (cm->hub && rc != KH_OK) {
                cm->hub->poison();  // (an error exit does not know where its peers are: nobody waits for anybody any more)
                for (hipStream_t s : cm->hub->xs)
                    if (s) (void)hipStreamSynchronize(s);
            } else if (cm->nccl && !cm->dead.load()) {
                (void)xp_wait(c, nullptr, "draining the exchange stream");
            } else if (cm->xs) {
                (void)hipStreamSynchronize(cm->xs);
            }
        }
        (void)kh_set_region_window(c, 0, 1);  // whatever happened: later exports / merges cover the whole range again
        mi.export_ms = t_export;
        mi.wait_ms = t_wait;
        mi.merge_ms = t_merge;
        mi.total_ms = now_ms() - t_begin;
        if (info) *info = mi;
        return rc;
    };
    // gather with timing; `where` names what would have come next
    std::vector<u64> all;
    auto gather = [&](int lrc, const std::vector<u64> &m, const char *where) -> int {
        all.assign((size_t)W * std::max<size_t>(m.size(), 1), 0);
        const double t0 = now_ms();
        const int rc = xp_gather(c, lrc, m.data(), (uint32_t)m.size(), all.data(), where);
        t_wait += now_ms() - t0;
        return rc;
    };
    // the merge's last act: every rank learns whether every other one got through its merge kernels.  (Hub: also the
    // closing barrier -- every peer has finished copying out of this rank's send buffer before it is freed.)
    // ---- conservation (round 5; kmerhip.h kh_merge_info) ----
    // tx: what this rank exported, per destination; want_rx: what the senders announced for this rank (from the gathers the
    // sequence has anyway); the receive side digests what arrived (d_rx) and verify_rx() compares -- and holds the sum of the
    // counts the merge kernels took in (Counters::kmers of the shard, zero after kh_reset) to the same figures.
    DevBuf dig;  // [0, 3W): scratch of the sender's digests; [3W (1 + i), 3W (2 + i)): the digests of what arrived in piece i
    std::vector<u64> want_rx((size_t)3 * W, 0);
    u64 tx_sum_total = 0, local_total = 0;
    uint32_t rx_slots = 0;  // pieces whose arrival has been digested
    auto d_tx = [&]() { return (u64 *)dig.p; };
    bool *tx_done_ptr = nullptr;  // (set below: whether the export that has just run took its own digests -- merge.hip)
    auto tx_done_flag = [&]() {
        const bool v = tx_done_ptr && *tx_done_ptr;
        if (tx_done_ptr) *tx_done_ptr = false;  // (one export, one digest)
        return v;
    };
    auto d_rx = [&](uint32_t i) { return (u64 *)dig.p + (size_t)3 * W * (1 + i); };
    // digests of one export's W segments (bytes so / sl inside `base`), read back: m[3 p + {units, counts, checksum}]
    auto tx_digest = [&](int fmt, const void *base, const u64 *counts, const std::vector<u64> &so, const std::vector<u64> &sl, u64 ub, uint32_t cmask,
                         std::vector<u64> &m) -> int {
        m.assign((size_t)3 * W, 0);
        int r = tx_done_flag() ? KH_OK : digest_units(c, fmt, base, counts, so.data(), sl.data(), W, ub, cmask, d_tx());
        if (r != KH_OK) return r;
        HIP_TRY(c, hipMemcpyAsync(m.data(), d_tx(), m.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (uint32_t p = 0; p < W; ++p) tx_sum_total += m[3 * p + 1];
        return KH_OK;
    };
    // after a gather that carried every rank's tx digests (3 W words each): what they say this rank receives
    auto note_announced = [&]() {
        for (uint32_t s2 = 0; s2 < W; ++s2)
            for (int j = 0; j < 3; ++j) want_rx[3 * s2 + j] += all[(size_t)s2 * 3 * W + 3 * R + j];
    };
    // (test build) KMERHIP_FAULT=rank:drop_half -- the upper half of what arrived is lost, as in round 4's transport incident
    // (of every segment that travelled: byte offsets / lengths per sender inside `buf`)
    auto sabotage = [&](void *buf, const u64 *roff, const u64 *rlen) {
        if ((int)R != flt.rank || flt.point != "drop_half") return;
        for (uint32_t s2 = 0; s2 < W; ++s2)
            if (rlen[s2] && !(self_direct && s2 == R)) {
                hipError_t e = hipMemsetAsync((char *)buf + roff[s2] + rlen[s2] / 2, 0, rlen[s2] - rlen[s2] / 2, c->stream);
                if (c->trace) fprintf(stderr, "[kmerhip] sabotage rank %u sender %u buf %p off %llu len %llu -> %d\n", R, s2, buf, (unsigned long long)roff[s2], (unsigned long long)rlen[s2], (int)e);
            }
    };
    // everything has been merged (kh_finish has run: the stream is idle, h_ctr current): arrived == announced == merged?
    auto verify_rx = [&]() -> int {
        std::vector<u64> got((size_t)3 * W, 0), h((size_t)3 * W * std::max(1u, rx_slots), 0);
        if (rx_slots && hipMemcpy(h.data(), d_rx(0), (size_t)3 * W * rx_slots * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, KH_ERR_HIP, "hipMemcpy(arrival digests)");
        for (uint32_t i = 0; i < rx_slots; ++i)
            for (size_t j = 0; j < (size_t)3 * W; ++j) got[j] += h[(size_t)3 * W * i + j];
        u64 announced = 0;
        for (uint32_t s2 = 0; s2 < W; ++s2) {
            announced += want_rx[3 * s2 + 1];
            if (got[3 * s2] != want_rx[3 * s2] || got[3 * s2 + 1] != want_rx[3 * s2 + 1] || got[3 * s2 + 2] != want_rx[3 * s2 + 2]) {
                char buf[320];
                snprintf(buf, sizeof(buf), "conservation: what arrived from rank %u differs from what it sent (units %llu / %llu, counts %llu / %llu, checksum %s): "
                         "the transport lost or changed data", s2, (unsigned long long)got[3 * s2], (unsigned long long)want_rx[3 * s2],
                         (unsigned long long)got[3 * s2 + 1], (unsigned long long)want_rx[3 * s2 + 1], got[3 * s2 + 2] == want_rx[3 * s2 + 2] ? "equal" : "different");
                c->last_error = buf;
                return KH_ERR_RCCL;
            }
        }
        if (c->h_ctr->kmers != announced) {
            char buf[256];
            snprintf(buf, sizeof(buf), "conservation: the merge kernels took in counts summing to %llu, the units that arrived carry %llu",
                     (unsigned long long)c->h_ctr->kmers, (unsigned long long)announced);
            c->last_error = buf;
            return KH_ERR_RCCL;
        }
        return KH_OK;
    };
    // all of this rank's exports are digested: do they carry what the table held?
    auto verify_tx = [&]() -> int {
        if (tx_sum_total == local_total) return KH_OK;
        char buf[256];
        snprintf(buf, sizeof(buf), "conservation: the exports carry counts summing to %llu, the table held %llu", (unsigned long long)tx_sum_total,
                 (unsigned long long)local_total);
        c->last_error = buf;
        return KH_ERR_RCCL;
    };
    auto finish = [&](int lrc) -> int {
        if (cm->hub && transfers && lrc == KH_OK && hipStreamSynchronize(cm->xs) != hipSuccess) lrc = fail(c, KH_ERR_HIP, "hipStreamSynchronize(exchange)");
        if (lrc == KH_OK) {
            mi.sent_count_sum = tx_sum_total;
            mi.merged_count_sum = c->h_ctr->kmers;
        }
        const int rc = gather(lrc, {mi.sent_count_sum, mi.merged_count_sum}, "the end of the merge");
        if (rc != KH_OK) return done(rc);
        transfers = false;  // (every rank's copies are complete: see the line above)
        // the closing identity, from the gathered words (every rank decides the same): all that left == all that was merged
        u64 sent = 0, merged = 0;
        for (uint32_t r = 0; r < W; ++r) {
            sent += all[2 * r];
            merged += all[2 * r + 1];
        }
        if (sent != merged) {
            char buf[256];
            snprintf(buf, sizeof(buf), "conservation: the ranks exported counts summing to %llu and merged %llu", (unsigned long long)sent, (unsigned long long)merged);
            c->last_error = buf;
            return done(KH_ERR_RCCL);
        }
        mi.conserved = 1;
        return done(KH_OK);
    };

    if (cm->nccl && (int)R == flt.rank && flt.point == "abort") {  // (tests: what a time-out does, without waiting for one)
        comm_abort(cm);
        return done(rccl_dead(c, "injected abort"));
    }
    int lrc = pre;
    if (lrc == KH_OK) lrc = kh_finish(c, nullptr);
    // The counting is over: its partition buffers (up to 0.8 of the device) are given back where the exchange would not fit
    // beside them -- send and receive buffers (<= 16 B per local key together) and the shard's 16-byte table.  (Not always: a
    // host that counts and merges in a loop would pay for 150 GB of hipMalloc per round.)
    // Round 5: first the merge BORROWS from them (ctx.hip.h, borrow_on): its send / receive buffers and the shard's 16-byte table
    // are carved out of the idle buffers, nothing is freed or allocated in a count-and-merge loop (bench.py --force-merge at
    // configs[3]'s size: 514 ms per step with the buffers going back and forth, of which 146 were kernels).  Only where they
    // cannot hold it all is the old way taken.
    if (lrc == KH_OK) {
        size_t fr = 0, tot = 0;
        const u64 keys_now = c->h_ctr->distinct;
        const u64 scratch = 16ull * keys_now + (64ull << 20);                        // send + receive buffers, counts
        const u64 tab = c->table ? 0 : 16ull * std::max<u64>(c->cap, 2 * keys_now);  // the shard's table (it may have to hold every rank's keys of its range)
        const u64 lendable = (c->keysA ? c->key_cap : 0) + (c->keysB ? c->keyb_cap : 0);
        // (what does not fit the loan comes from hipMalloc -- borrow() just says no --, so lending is always safe; the buffers go
        //  back to the driver only where that remainder would not fit the free memory either)
        const u64 rest = scratch + tab > lendable ? scratch + tab - lendable : 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
            (void)hipGetLastError();
            fr = 0;
        }
        if (lendable && (u64)fr >= rest + (rest ? (2ull << 30) : 0)) {
            // (a failure here is carried into the next gather like every other one: the peers must not be left in it -- ADVICE r5)
            if (hipStreamSynchronize(c->stream) != hipSuccess) lrc = fail(c, KH_ERR_HIP, "hipStreamSynchronize(before the merge borrows the partition buffers)");
            else {
                c->borrow_on = true;
                c->borrow_off[0] = c->borrow_off[1] = 0;
            }
        } else if ((u64)fr < scratch + 16ull * (c->cap / W + kh::REGION_SLOTS) + (4ull << 30)) {
            lrc = release_part_buffers(c);
        }
    }
    if (lrc == KH_OK) lrc = inject("start");
    const u64 n_local = lrc == KH_OK ? c->h_ctr->distinct : 0;
    local_total = lrc == KH_OK ? c->h_ctr->kmers : 0;  // the sum of all counts of this rank's table
    u64 nreg = c->cap / kh::REGION_SLOTS;
    mi.local_distinct = n_local;
    int rc;

    // ---- small k: the key space as a dense count array IS element-wise reducible ----
    if (2 * c->k <= 26 && !cm->hub) {  // (uniform: k and the transport are the same on every rank)
        const u64 n = 1ull << (2 * c->k);
        DevBuf dense;
        double t0 = now_ms();
        if (lrc == KH_OK) lrc = dense.alloc(c, n * sizeof(u64), "hipMalloc(dense)");
        if (lrc == KH_OK) lrc = inject("dense_export");
        if (lrc == KH_OK) lrc = kh_export_dense_device(c, (uint64_t *)dense.p, n);  // blocks until complete
        t_export += now_ms() - t0;
        if ((rc = gather(lrc, {}, "the dense all-reduce")) != KH_OK) return done(rc);
        t0 = now_ms();
        transfers = true;
        if ((rc = xp_allreduce_sum_u64(c, (u64 *)dense.p, n)) != KH_OK) return done(rc);  // (transport failure: communicator aborted)
        transfers = false;
        t_wait += now_ms() - t0;
        t0 = now_ms();
        lrc = merge_reset(c);
        if (lrc == KH_OK) lrc = inject("dense_merge");
        if (lrc == KH_OK) lrc = kh_merge_dense_device(c, (const uint64_t *)dense.p, n, R, W);
        if (lrc == KH_OK) lrc = kh_finish(c, nullptr);
        t_merge += now_ms() - t0;
        mi.route = KH_ROUTE_DENSE;
        mi.unit_bytes = 8;
        mi.sent_units = mi.recv_units = n;
        if (lrc == KH_OK) mi.owned_distinct = c->h_ctr->distinct;
        tx_sum_total = local_total;  // (dense: what a rank adds to the all-reduce is its table; finish() holds the sum of the shards to the sum of these)
        return finish(lrc);
    }

    // ---- one table geometry for every rank (round 4) ----
    // A table is sized from its own rank's level-1 sample (batch.hip): two ranks whose estimates fall on either side of a size
    // step hold tables of different geometry, whose regions do not correspond -- such a world used to take the generic route.
    // The smaller tables are re-laid-out to the largest one first (grow_to: one rehash pass over a table's keys), so that the
    // region routes below apply.  (A rank that cannot -- out of memory -- says so in the next gather like any other failure.)
    if ((rc = gather(lrc, {nreg}, "the table sizes")) != KH_OK) return done(rc);
    {
        u64 target = 0;
        for (uint32_t r = 0; r < W; ++r) target = std::max(target, all[r]);
        if (nreg < target && kh::kh_regions_valid(target)) {
            const double t0 = now_ms();
            // (the borrow-or-release decision above was taken for THIS rank's table; the re-laid-out one -- 16 B per slot
            //  of the world's largest, from hipMalloc, beside the widened 8-byte image -- may not fit beside the partition buffers.
            //  Nothing has been carved out of them yet -- the digests come below --, so they can still go back to the driver.)
            {
                size_t fr = 0, tot = 0;
                if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
                    (void)hipGetLastError();
                    fr = 0;
                }
                const u64 need = 16ull * target * kh::REGION_SLOTS + (c->table ? 0 : 16ull * c->cap) + (2ull << 30);
                if ((u64)fr < need && (c->keysA || c->keysB)) lrc = release_part_buffers(c);  // (ends the loan too)
            }
            if (lrc == KH_OK) lrc = grow_to(c, target * kh::REGION_SLOTS);
            if (lrc == KH_OK) lrc = kh_finish(c, nullptr);
            if (lrc == KH_OK) nreg = c->cap / kh::REGION_SLOTS;
            t_export += now_ms() - t0;
            if (c->trace) fprintf(stderr, "[kmerhip] merge: rank %u re-laid its table out to %llu regions (the largest of the world) in %.1f ms\n", R,
                                  (unsigned long long)target, now_ms() - t0);
        }
    }

    if (lrc == KH_OK) lrc = dig.alloc(c, (size_t)3 * W * (1 + 64) * sizeof(u64), "hipMalloc(digests)");
    const bool pow2 = (W & (W - 1)) == 0;
    const int head_cb = head_count_bits(c, nreg);  // (< 0: heads do not apply to this table -- the vote then never agrees on them)
    const uint32_t head_cmask = head_cb > 0 ? (1u << head_cb) - 1u : 0u;
    // (a table of 1024 x b2 regions, b2 not a power of two, splits into hash-range shards that nest only if W divides b2:
    //  kmerhip.hip merge_regions; round_cap() keeps b2 a multiple of 8 -- of 64 from 512 -- so this fails only for worlds
    //  of 16+ ranks with small tables, which then take the generic route)
    const kh::RegionGeom my_geo = geom_of_cap(c->cap);
    const bool geo_ok = (my_geo.b2 & (my_geo.b2 - 1)) == 0 || my_geo.b2 % W == 0;
    const bool regions_ok = pow2 && W <= (uint32_t)kh::MAX_SENDERS && nreg >= W && nreg % W == 0 && geo_ok;
    uint32_t npieces = merge_pieces_default();
    bool piped = regions_ok && npieces > 1 && (npieces & (npieces - 1)) == 0 && npieces <= 64 && (nreg / W) >= 64ull * npieces && (nreg / W) % npieces == 0;
    if (!piped) npieces = 1;

    // send buffer: heads (2 per key), packed (1 u64 per key) and one array of wide pairs all fit 8 B x n_local
    DevBuf sendbuf, sendcnt, rcnt, counts_all;
    const u64 cap_units64 = std::max<u64>(n_local, 1);
    std::vector<uint64_t> parts(W, 0);
    uint64_t treg = 0;
    // fmt: 2 heads, 1 packed, 0 = neither fits
    bool tx_done = false;  // the last export left its digests in d_tx() (merge.hip: taken by the compaction on the way)
    tx_done_ptr = &tx_done;
    auto export_fmt = [&](int fmt, void *dst, u64 cap) -> int {
        const double t0 = now_ms();
        int r = export_regions(c, fmt == 2 ? XF_HEADS32 : XF_PACKED64, W, dst, nullptr, cap, (uint32_t *)rcnt.p, nreg, parts.data(), &treg, d_tx(), &tx_done);
        t_export += now_ms() - t0;
        return r;
    };
    // speculative: the export itself finds out whether the counts fit; *fmt_out = 0 when neither narrow unit applies
    auto export_narrowest = [&](int *fmt_out) -> int {
        *fmt_out = 0;
        for (int fmt : {2, 1}) {
            const int r = export_fmt(fmt, sendbuf.p, fmt == 2 ? 2 * n_local : n_local);
            if (r == KH_OK) {
                *fmt_out = fmt;
                return KH_OK;
            }
            if (r != KH_ERR_RANGE) return r;
        }
        return KH_OK;
    };
    int my_fmt = 0;
    if (lrc == KH_OK) lrc = sendbuf.alloc(c, cap_units64 * 8, "hipMalloc(exchange send buffer)");
    if (lrc == KH_OK) lrc = rcnt.alloc(c, std::max<u64>(nreg, 1) * sizeof(uint32_t), "hipMalloc(region counts)");
    if (lrc == KH_OK) lrc = inject("export0");
    if (lrc == KH_OK && regions_ok) {
        if (piped) lrc = kh_set_region_window(c, 0, npieces);
        if (lrc == KH_OK) lrc = export_narrowest(&my_fmt);
        if (lrc == KH_OK && my_fmt == 2 && flt.point == "fmt_packed" && (int)R == flt.rank) {  // (tests: this rank alone needs the wider unit)
            my_fmt = 0;
            const int r = export_fmt(1, sendbuf.p, n_local);
            if (r == KH_OK) my_fmt = 1;
            else if (r != KH_ERR_RANGE) lrc = r;
        }
    }
    if ((rc = gather(lrc, {nreg, (u64)my_fmt, (u64)piped}, "the format vote")) != KH_OK) return done(rc);
    // Everything decided from here on is decided from the GATHERED words only, so that every rank decides the same
    // (round 2 compared `agreed` with this rank's own format: a rank whose format WAS the agreed one stayed in the
    // pipeline while its peer left it, and their next collectives no longer matched).
    bool same_size = true, all_piped = true, all_same_fmt = true;
    u64 agreed = 3;
    for (uint32_t r = 0; r < W; ++r) {
        same_size &= all[3 * r] == all[0];
        agreed = std::min(agreed, all[3 * r + 1]);
        all_same_fmt &= all[3 * r + 1] == all[1];
        all_piped &= all[3 * r + 2] != 0;
    }
    if (!(regions_ok && same_size)) agreed = 0;  // (regions_ok depends on W and on nreg: uniform once the sizes are equal)
    bool redo_export = false;                    // the send buffer does not hold a whole-table export in the agreed unit
    if (piped && !(same_size && agreed && all_same_fmt && all_piped)) {
        // some rank cannot run the pipeline, or not in the others' format: everybody takes the one-shot route
        piped = false;
        npieces = 1;
        (void)kh_set_region_window(c, 0, 1);
        redo_export = true;  // the windowed export does not describe the whole table
    } else if (!piped && all_piped) {
        all_piped = false;  // (cannot happen: `piped` follows from W, nreg and the environment, which the ranks share)
    }
    if (piped) {
        // every piece's size is known before anything is sent: a table needing more units than the send
        // buffer holds is found out HERE, and all ranks leave the pipeline together
        const uint32_t ub = agreed == 2 ? 4 : 8;
        const u64 cap_total = agreed == 2 ? 2 * n_local : n_local;
        std::vector<uint32_t> hcounts;
        bool fits = false;
        {
            const double t0 = now_ms();
            lrc = counts_all.alloc(c, nreg * sizeof(uint32_t), "hipMalloc(unit counts)");
            if (lrc == KH_OK) lrc = inject("unit_counts");
            if (lrc == KH_OK) {
                uint64_t treg2 = 0;
                const int r = kh_region_unit_counts_device(c, ub, (uint32_t *)counts_all.p, nreg, &treg2);
                if (r == KH_OK) {
                    hcounts.resize(nreg);
                    if (hipMemcpy(hcounts.data(), counts_all.p, nreg * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
                        lrc = fail(c, KH_ERR_HIP, "hipMemcpy(unit counts)");
                    u64 total = 0;
                    for (uint32_t v : hcounts) total += v;
                    fits = lrc == KH_OK && total <= cap_total;
                } else if (r != KH_ERR_RANGE) {
                    lrc = r;
                }
            }
            t_export += now_ms() - t0;
        }
        if ((rc = gather(lrc, {(u64)fits}, "the piece sizes")) != KH_OK) return done(rc);
        bool all_fit = true;
        for (uint32_t r = 0; r < W; ++r) all_fit &= all[r] != 0;
        if (!all_fit) {
            piped = false;
            npieces = 1;
            (void)kh_set_region_window(c, 0, 1);
            redo_export = true;
        } else {
            // ---- pipeline over the pieces: [export i+1 | transfer i], then [merge i | transfers > i] ----
            const u64 per = nreg / W, wper = per / npieces;
            // sizes of all pieces, announced up front: send_mat[owner][piece]
            std::vector<u64> send_mat((size_t)W * npieces, 0), recv_mat((size_t)W * npieces, 0);
            for (uint32_t o = 0; o < W; ++o)
                for (uint32_t i = 0; i < npieces; ++i) {
                    u64 s = 0;
                    const uint32_t *p = hcounts.data() + (u64)o * per + (u64)i * wper;
                    for (u64 q = 0; q < wper; ++q) s += p[q];
                    send_mat[(size_t)o * npieces + i] = s;
                }
            // recv_mat[sender][piece]: what each sender has for ME -- gather everybody's matrix (W * npieces <= 4096
            // values, in slices)
            {
                const double t0 = now_ms();
                std::vector<u64> allm((size_t)W * W * npieces);
                const uint32_t tot = W * npieces, SL = SMALL_MAX - 1;
                for (uint32_t b = 0; b < tot; b += SL) {
                    const uint32_t n = std::min<uint32_t>(SL, tot - b);
                    std::vector<u64> g((size_t)W * n);
                    if ((rc = xp_gather(c, KH_OK, send_mat.data() + b, n, g.data(), "the piece sizes")) != KH_OK) return done(rc);
                    for (uint32_t r = 0; r < W; ++r) memcpy(&allm[(size_t)r * tot + b], &g[(size_t)r * n], n * sizeof(u64));
                }
                for (uint32_t s = 0; s < W; ++s)
                    for (uint32_t i = 0; i < npieces; ++i) recv_mat[(size_t)s * npieces + i] = allm[(size_t)s * tot + (size_t)R * npieces + i];
                t_wait += now_ms() - t0;
            }
            // Every buffer the pipeline needs is allocated BEFORE its first transfer (all of them are alive together
            // anyway): running out of memory is then something the ranks hear about in the gather below, not a peer
            // that never posts its receive.
            struct Flight {
                DevBuf buf;
                std::vector<u64> roff;  // byte offsets per sender
                u64 units = 0;
                hipEvent_t ev = nullptr;
            };
            std::vector<Flight> flights(npieces);
            struct EvGuard {  // (events are destroyed on every exit)
                std::vector<Flight> &f;
                ~EvGuard() {
                    for (auto &x : f)
                        if (x.ev) (void)hipEventDestroy(x.ev);
                }
            } ev_guard{flights};
            DevBuf rrc_full, rrc;  // every sender's unit counts of MY regions (W slices of `per`); the same, zero outside a piece
            lrc = rrc_full.alloc(c, nreg * sizeof(uint32_t), "hipMalloc(region counts in)");
            if (lrc == KH_OK) lrc = rrc.alloc(c, nreg * sizeof(uint32_t), "hipMalloc(region counts piece)");
            if (lrc == KH_OK) lrc = inject("alloc_recv");
            for (uint32_t i = 0; i < npieces && lrc == KH_OK; ++i) {
                u64 rtot = 0;
                flights[i].roff.resize(W);
                for (uint32_t p = 0; p < W; ++p) {
                    flights[i].roff[p] = rtot * ub;
                    rtot += recv_mat[(size_t)p * npieces + i];
                }
                flights[i].units = rtot;
                lrc = flights[i].buf.alloc(c, rtot * ub, "hipMalloc(exchange receive buffer)");
                if (lrc == KH_OK && hipEventCreateWithFlags(&flights[i].ev, hipEventDisableTiming) != hipSuccess)
                    lrc = fail(c, KH_ERR_HIP, "hipEventCreate(exchange)");
            }
            if ((rc = gather(lrc, {}, "the region-count exchange")) != KH_OK) return done(rc);
            {
                std::vector<u64> so(W), sl(W), ro(W), rl(W);
                for (uint32_t p = 0; p < W; ++p) {
                    so[p] = (u64)p * per * 4;
                    sl[p] = per * 4;
                    ro[p] = (u64)p * per * 4;
                    rl[p] = per * 4;
                }
                const double t0 = now_ms();
                transfers = true;
                lrc = xp_alltoallv(c, counts_all.p, so.data(), sl.data(), rrc_full.p, ro.data(), rl.data());
                if (lrc == KH_OK) lrc = xp_wait(c, nullptr, "region-count exchange");
                t_wait += now_ms() - t0;
            }
            u64 used = 0;  // units of the send buffer in use
            std::vector<const char *> self_ptr(npieces, nullptr);  // this rank's own segment of every piece, where the export put it
            for (uint32_t i = 0; i < npieces; ++i) {
                void *dst = (char *)sendbuf.p + used * ub;
                std::vector<u64> so(W), sl(W), rl(W);
                u64 o = 0;
                if (lrc == KH_OK && i > 0) {
                    lrc = kh_set_region_window(c, i, npieces);
                    if (lrc == KH_OK) lrc = inject("export_piece");
                    if (lrc == KH_OK) lrc = export_fmt((int)agreed, dst, cap_total - used);  // (sizes were checked: cannot be RANGE)
                }
                for (uint32_t p = 0; p < W && lrc == KH_OK; ++p) {
                    if (parts[p] != send_mat[(size_t)p * npieces + i]) lrc = fail(c, KH_ERR_STATE, "piece sizes differ from the announced ones");
                    so[p] = o * ub;
                    sl[p] = parts[p] * ub;
                    o += parts[p];
                    rl[p] = recv_mat[(size_t)p * npieces + i] * ub;
                }
                // what this piece carries, per destination: announced with the gather below, recomputed by the receivers
                std::vector<u64> txm((size_t)3 * W, 0);  // (a rank that failed before its digest still posts as many words as its peers)
                if (lrc == KH_OK) lrc = tx_digest(agreed == 2 ? XF_HEADS32 : XF_PACKED64, dst, nullptr, so, sl, ub, head_cmask, txm);
                if (lrc == KH_OK && i + 1 == npieces) lrc = verify_tx();
                // piece i leaves only when every rank has it ready (the gather queues behind transfer i - 1 on the exchange
                // stream, which transfer i would do anyway; the export of piece i has overlapped transfer i - 1 by now)
                if ((rc = gather(lrc, txm, "the transfer of a piece")) != KH_OK) return done(rc);
                note_announced();
                mi.sent_units += o - parts[R];
                used += o;
                const double t0 = now_ms();
                self_ptr[i] = (const char *)dst + so[R];
                lrc = xp_alltoallv(c, dst, so.data(), sl.data(), flights[i].buf.p, flights[i].roff.data(), rl.data(), self_direct);
                if (lrc == KH_OK && hipEventRecord(flights[i].ev, cm->xs) != hipSuccess) lrc = fail(c, KH_ERR_HIP, "hipEventRecord(exchange)");
                t_wait += now_ms() - t0;
                if (lrc != KH_OK && cm->nccl) return done(lrc);  // (an RCCL failure aborted the communicator: the peers' waits end)
            }
            if (lrc == KH_OK) lrc = kh_set_region_window(c, 0, 1);
            if (lrc == KH_OK) lrc = merge_reset(c);
            if (lrc == KH_OK) lrc = kh_set_shard(c, R, W);
            for (uint32_t i = 0; i < npieces && lrc == KH_OK; ++i) {
                double t0 = now_ms();
                // the senders' region counts as the merge of piece i wants them: zero outside the piece
                if (hipMemsetAsync(rrc.p, 0, nreg * sizeof(uint32_t), c->stream) != hipSuccess) lrc = fail(c, KH_ERR_HIP, "hipMemsetAsync(rrc)");
                for (uint32_t s = 0; s < W && lrc == KH_OK; ++s) {
                    const u64 o = ((u64)s * per + (u64)i * wper) * 4;
                    if (hipMemcpyAsync((char *)rrc.p + o, (const char *)rrc_full.p + o, wper * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                        lrc = fail(c, KH_ERR_HIP, "hipMemcpyAsync(rrc)");
                }
                if (lrc == KH_OK) lrc = xp_wait(c, flights[i].ev, "transfer of a piece");
                t_wait += now_ms() - t0;
                if (lrc != KH_OK) break;
                t0 = now_ms();
                {
                    std::vector<u64> rl(W);
                    for (uint32_t s2 = 0; s2 < W; ++s2) rl[s2] = recv_mat[(size_t)s2 * npieces + i] * ub;
                    sabotage(flights[i].buf.p, flights[i].roff.data(), rl.data());
                }
                std::vector<const void *> kp(W);
                std::vector<const uint32_t *> rp(W);
                for (uint32_t s = 0; s < W; ++s) {
                    kp[s] = (self_direct && s == R) ? self_ptr[i] : (const char *)flights[i].buf.p + flights[i].roff[s];
                    rp[s] = (const uint32_t *)rrc.p + (u64)s * per;
                }
                lrc = kh_set_region_window(c, i, npieces);
                if (lrc == KH_OK) lrc = inject("merge_piece");
                // what arrived, per source: digested by the merge kernel on the way where it can (merge.hip), else by a pass of its own over
                // the same bytes -- either way on the context's stream, from the very buffer the merge reads
                bool digested = false;
                if (lrc == KH_OK) lrc = merge_regions(c, agreed == 2 ? XF_HEADS32 : XF_PACKED64, W, nreg, kp.data(), nullptr, rp.data(), d_rx(i), &digested);
                if (lrc == KH_OK && !digested) {
                    std::vector<u64> rl(W), zo(W, 0), own(W, 0);
                    for (uint32_t s2 = 0; s2 < W; ++s2) rl[s2] = recv_mat[(size_t)s2 * npieces + i] * ub;
                    if (self_direct) std::swap(own[R], rl[R]);  // (its own segment: digested where it lies)
                    lrc = digest_units(c, agreed == 2 ? XF_HEADS32 : XF_PACKED64, flights[i].buf.p, nullptr, flights[i].roff.data(), rl.data(), W, ub, head_cmask, d_rx(i));
                    if (lrc == KH_OK && self_direct) lrc = digest_units(c, agreed == 2 ? XF_HEADS32 : XF_PACKED64, self_ptr[i], nullptr, zo.data(), own.data(), W, ub, head_cmask, d_rx(i), true);
                }
                rx_slots = i + 1;
                mi.recv_units += flights[i].units;
                t_merge += now_ms() - t0;
            }
            if (lrc == KH_OK) {
                (void)kh_set_region_window(c, 0, 1);
                lrc = kh_finish(c, nullptr);
            }
            if (lrc == KH_OK) lrc = verify_rx();
            mi.route = agreed == 2 ? KH_ROUTE_REGIONS_HEADS : KH_ROUTE_REGIONS_PACKED;
            mi.pieces = npieces;
            mi.unit_bytes = ub;
            if (lrc == KH_OK) mi.owned_distinct = c->h_ctr->distinct;
            return finish(lrc);  // (flights' buffers are freed after done() has drained the exchange stream)
        }
    }
    // ---- one shot ----
    lrc = KH_OK;
    if (redo_export) {  // left the pipeline: whole table, narrowest unit that fits, and a second vote
        lrc = inject("oneshot_export");
        if (lrc == KH_OK) lrc = export_narrowest(&my_fmt);
        if ((rc = gather(lrc, {(u64)my_fmt}, "the second format vote")) != KH_OK) return done(rc);
        agreed = 3;
        for (uint32_t r = 0; r < W; ++r) agreed = std::min(agreed, all[r]);
        if (!(regions_ok && same_size)) agreed = 0;
    }
    if (agreed && agreed != (u64)my_fmt)  // another rank could not go as narrow: redo in the common format
        lrc = export_fmt((int)agreed, sendbuf.p, agreed == 2 ? 2 * n_local : n_local);

    // one all-to-all of per-owner unit counts (with the status of whatever came before), then the data
    auto exchange_sizes = [&](int st, const std::vector<uint64_t> &send_units_in, std::vector<u64> &recv_units) -> int {
        std::vector<u64> send_units(send_units_in.begin(), send_units_in.end());
        std::vector<u64> g;
        recv_units.assign(W, 0);
        const uint32_t SL = SMALL_MAX - 1;
        const double t0 = now_ms();
        for (uint32_t b = 0; b < W; b += SL) {
            const uint32_t n = std::min<uint32_t>(SL, W - b);
            g.assign((size_t)W * n, 0);
            const int r = xp_gather(c, st, send_units.data() + b, n, g.data(), "the unit counts");
            if (r != KH_OK) return r;
            if (R >= b && R < b + n)
                for (uint32_t s = 0; s < W; ++s) recv_units[s] = g[(size_t)s * n + (R - b)];
        }
        t_wait += now_ms() - t0;
        return KH_OK;
    };
    auto a2a_units = [&](const void *send, const std::vector<uint64_t> &su, const std::vector<u64> &ru, u64 ub, void *recv, bool skip_self = false) -> int {
        std::vector<u64> so(W), sl(W), ro(W), rl(W);
        u64 a = 0, b = 0;
        for (uint32_t p = 0; p < W; ++p) {
            so[p] = a * ub;
            sl[p] = su[p] * ub;
            a += su[p];
            ro[p] = b * ub;
            rl[p] = ru[p] * ub;
            b += ru[p];
        }
        return xp_alltoallv(c, send, so.data(), sl.data(), recv, ro.data(), rl.data(), skip_self);
    };

    if (agreed || (regions_ok && same_size)) {
        const bool wide = !agreed;
        const u64 ub = agreed == 2 ? 4 : 8;
        const u64 per = nreg / W;
        if (wide) tx_done = false;  // (a speculative narrow export's digests say nothing about the wide one)
        if (wide && lrc == KH_OK) {  // (u64 key, u64 count): two arrays
            lrc = sendcnt.alloc(c, cap_units64 * 8, "hipMalloc(exchange send counts)");
            const double t0 = now_ms();
            if (lrc == KH_OK) lrc = export_regions(c, XF_WIDE, W, sendbuf.p, (uint64_t *)sendcnt.p, n_local, (uint32_t *)rcnt.p, nreg, parts.data(), &treg);
            t_export += now_ms() - t0;
        }
        if (lrc == KH_OK) lrc = inject("oneshot_sizes");
        std::vector<u64> recv_units;
        if ((rc = exchange_sizes(lrc, parts, recv_units)) != KH_OK) return done(rc);
        u64 rtot = 0;
        for (u64 v : recv_units) rtot += v;
        DevBuf rbuf, rbuf2, rrc;
        lrc = rbuf.alloc(c, rtot * ub, "hipMalloc(exchange receive buffer)");
        if (lrc == KH_OK) lrc = rrc.alloc(c, nreg * sizeof(uint32_t), "hipMalloc(region counts in)");
        if (lrc == KH_OK && wide) lrc = rbuf2.alloc(c, rtot * 8, "hipMalloc(exchange receive counts)");
        if (lrc == KH_OK) lrc = inject("oneshot_alloc");
        const int xfmt = wide ? XF_WIDE : (agreed == 2 ? XF_HEADS32 : XF_PACKED64);
        std::vector<u64> txm((size_t)3 * W, 0), seg_so(W), seg_sl(W), seg_ro(W), seg_rl(W);
        {
            u64 a2 = 0, b2 = 0;
            for (uint32_t p = 0; p < W; ++p) {
                seg_so[p] = a2 * ub;
                seg_sl[p] = parts[p] * ub;
                a2 += parts[p];
                seg_ro[p] = b2 * ub;
                seg_rl[p] = recv_units[p] * ub;
                b2 += recv_units[p];
            }
        }
        if (lrc == KH_OK) lrc = tx_digest(xfmt, sendbuf.p, wide ? (const u64 *)sendcnt.p : nullptr, seg_so, seg_sl, ub, head_cmask, txm);
        if (lrc == KH_OK) lrc = verify_tx();
        if ((rc = gather(lrc, txm, "the exchange")) != KH_OK) return done(rc);
        note_announced();
        double t0 = now_ms();
        transfers = true;
        lrc = a2a_units(sendbuf.p, parts, recv_units, ub, rbuf.p, self_direct);
        if (lrc == KH_OK && wide) lrc = a2a_units(sendcnt.p, parts, recv_units, 8, rbuf2.p, self_direct);
        if (lrc == KH_OK) {
            std::vector<u64> so(W), sl(W, per * 4);
            for (uint32_t p = 0; p < W; ++p) so[p] = (u64)p * per * 4;
            lrc = xp_alltoallv(c, rcnt.p, so.data(), sl.data(), rrc.p, so.data(), sl.data());
        }
        if (lrc != KH_OK && cm->nccl) return done(lrc);      // (RCCL failure: communicator aborted, the peers' waits end)
        if (lrc == KH_OK) lrc = xp_wait(c, nullptr, "exchange");  // the merge kernels run on the context's stream
        t_wait += now_ms() - t0;
        t0 = now_ms();
        if (lrc == KH_OK) sabotage(rbuf.p, seg_ro.data(), seg_rl.data());
        if (lrc == KH_OK) lrc = merge_reset(c);
        if (lrc == KH_OK) lrc = kh_set_shard(c, R, W);
        if (lrc == KH_OK) lrc = inject("oneshot_merge");
        if (lrc == KH_OK) {
            std::vector<const void *> kp(W);
            std::vector<const uint64_t *> cp(W);
            std::vector<const uint32_t *> rp(W);
            u64 o = 0;
            for (uint32_t s = 0; s < W; ++s) {
                const bool own = self_direct && s == R;  // (this rank's own segment: read where the export put it)
                kp[s] = own ? (const char *)sendbuf.p + seg_so[R] : (const char *)rbuf.p + o * ub;
                cp[s] = !wide ? nullptr : own ? (const uint64_t *)sendcnt.p + seg_so[R] / ub : (const uint64_t *)rbuf2.p + o;
                rp[s] = (const uint32_t *)rrc.p + (u64)s * per;
                o += recv_units[s];
            }
            bool digested = false;
            lrc = merge_regions(c, wide ? XF_WIDE : (agreed == 2 ? XF_HEADS32 : XF_PACKED64), W, nreg, kp.data(), wide ? cp.data() : nullptr, rp.data(), d_rx(0), &digested);
            if (lrc == KH_OK && !digested) {
                std::vector<u64> rl(seg_rl), zo(W, 0), own(W, 0);
                if (self_direct) std::swap(own[R], rl[R]);
                lrc = digest_units(c, xfmt, rbuf.p, wide ? (const u64 *)rbuf2.p : nullptr, seg_ro.data(), rl.data(), W, ub, head_cmask, d_rx(0));
                if (lrc == KH_OK && self_direct)
                    lrc = digest_units(c, xfmt, (const char *)sendbuf.p + seg_so[R], wide ? (const u64 *)sendcnt.p + seg_so[R] / ub : nullptr, zo.data(), own.data(), W, ub, head_cmask, d_rx(0), true);
            }
            rx_slots = 1;
        }
        if (lrc == KH_OK) lrc = kh_finish(c, nullptr);
        if (lrc == KH_OK) lrc = verify_rx();
        t_merge += now_ms() - t0;
        mi.route = wide ? KH_ROUTE_REGIONS_WIDE : (agreed == 2 ? KH_ROUTE_REGIONS_HEADS : KH_ROUTE_REGIONS_PACKED);
        mi.unit_bytes = wide ? 16 : (uint32_t)ub;
        for (uint32_t p = 0; p < W; ++p) mi.sent_units += p == R ? 0 : parts[p];
        mi.recv_units = rtot;
        if (lrc == KH_OK) mi.owned_distinct = c->h_ctr->distinct;
        return finish(lrc);
    }

    // ---- generic route: any world size, tables of any size; device-atomic re-insert ----
    {
        tx_done = false;  // (as above)
        if (lrc == KH_OK) lrc = sendcnt.alloc(c, cap_units64 * 8, "hipMalloc(exchange send counts)");
        double t0 = now_ms();
        if (lrc == KH_OK) lrc = inject("generic_export");
        if (lrc == KH_OK) lrc = kh_export_by_owner_device(c, W, (uint64_t *)sendbuf.p, (uint64_t *)sendcnt.p, n_local, parts.data());  // blocks until complete
        t_export += now_ms() - t0;
        std::vector<u64> recv_units;
        if ((rc = exchange_sizes(lrc, parts, recv_units)) != KH_OK) return done(rc);
        u64 rtot = 0;
        for (u64 v : recv_units) rtot += v;
        DevBuf rk, rcn;
        lrc = rk.alloc(c, rtot * 8, "hipMalloc(exchange receive keys)");
        if (lrc == KH_OK) lrc = rcn.alloc(c, rtot * 8, "hipMalloc(exchange receive counts)");
        if (lrc == KH_OK) lrc = inject("generic_alloc");
        std::vector<u64> txm((size_t)3 * W, 0), seg_so(W), seg_sl(W), seg_ro(W), seg_rl(W);
        {
            u64 a2 = 0, b2 = 0;
            for (uint32_t p = 0; p < W; ++p) {
                seg_so[p] = a2 * 8;
                seg_sl[p] = parts[p] * 8;
                a2 += parts[p];
                seg_ro[p] = b2 * 8;
                seg_rl[p] = recv_units[p] * 8;
                b2 += recv_units[p];
            }
        }
        if (lrc == KH_OK) lrc = tx_digest(XF_WIDE, sendbuf.p, (const u64 *)sendcnt.p, seg_so, seg_sl, 8, 0u, txm);
        if (lrc == KH_OK) lrc = verify_tx();
        if ((rc = gather(lrc, txm, "the exchange")) != KH_OK) return done(rc);
        note_announced();
        t0 = now_ms();
        transfers = true;
        lrc = a2a_units(sendbuf.p, parts, recv_units, 8, rk.p);
        if (lrc == KH_OK) lrc = a2a_units(sendcnt.p, parts, recv_units, 8, rcn.p);
        if (lrc != KH_OK && cm->nccl) return done(lrc);
        if (lrc == KH_OK) lrc = xp_wait(c, nullptr, "exchange");
        t_wait += now_ms() - t0;
        t0 = now_ms();
        if (lrc == KH_OK) {
            sabotage(rk.p, seg_ro.data(), seg_rl.data());
            lrc = digest_units(c, XF_WIDE, rk.p, (const u64 *)rcn.p, seg_ro.data(), seg_rl.data(), W, 8, 0u, d_rx(0));
            rx_slots = 1;
        }
        if (lrc == KH_OK) lrc = merge_reset(c);
        if (lrc == KH_OK) lrc = inject("generic_merge");
        if (lrc == KH_OK) lrc = kh_merge_pairs_device(c, (const uint64_t *)rk.p, (const uint64_t *)rcn.p, rtot);
        if (lrc == KH_OK) lrc = kh_finish(c, nullptr);  // (also: the kernels are done with rk / rcn before they are freed)
        else (void)hipStreamSynchronize(c->stream);
        if (lrc == KH_OK) lrc = verify_rx();
        t_merge += now_ms() - t0;
        mi.route = KH_ROUTE_PAIRS;
        mi.unit_bytes = 16;
        for (uint32_t p = 0; p < W; ++p) mi.sent_units += p == R ? 0 : parts[p];
        mi.recv_units = rtot;
        if (lrc == KH_OK) mi.owned_distinct = c->h_ctr->distinct;
        return finish(lrc);
    }
}

void comm_release(kh_ctx *c) {
    Comm *cm = c->comm;
    if (!cm) return;
    cm->stop.store(true);
    if (cm->watchdog.joinable()) cm->watchdog.join();
    if (cm->xs && !cm->dead.load()) (void)hipStreamSynchronize(cm->xs);
    if (cm->nccl && !cm->dead.load()) (void)ncclCommDestroy(cm->nccl);  // (an aborted communicator is gone already)
    if (cm->hub && cm->rank < cm->hub->xs.size()) cm->hub->xs[cm->rank] = nullptr;
    if (cm->d_small) (void)dev_free(cm->d_small);
    if (cm->h_small) (void)pin_free(cm->h_small);
    if (cm->xs) (void)hipStreamDestroy(cm->xs);
    delete cm;
    c->comm = nullptr;
}

int comm_setup(kh_ctx *c, uint32_t nranks, uint32_t rank, const ncclUniqueId *id, LocalHub *hub) {
    if (c->comm) return fail(c, KH_ERR_STATE, "the context already has a communicator");
    if (nranks < 1 || rank >= nranks) return fail(c, KH_ERR_BAD_ARG, "kh_comm_init: rank must be < nranks");
    // (every route keeps per-sender state in arrays of MAX_SENDERS -- the merge kernels' segment tables, the digests, the small
    //  gathers' 3 words per rank: a larger world is refused here, by every rank alike, before any collective -- ADVICE r5)
    if (nranks > (uint32_t)kh::MAX_SENDERS) return fail(c, KH_ERR_BAD_ARG, "kh_comm_init: at most 64 ranks per communicator");
    HIP_TRY(c, hipSetDevice(c->device));
    Comm *cm = new (std::nothrow) Comm();
    if (!cm) return fail(c, KH_ERR_OOM, "Comm");
    cm->nranks = nranks;
    cm->rank = rank;
    cm->hub = hub;
    cm->timeout_s = merge_timeout_env();
    if (hub) hub->timeout_s = cm->timeout_s;
    c->part_budget = 0;  // (decided again at the next partitioned range: a rank of a merge leaves room for the exchange)
    c->comm = cm;
    int rc = KH_OK;
    if (hipStreamCreateWithFlags(&cm->xs, hipStreamNonBlocking) != hipSuccess) rc = fail(c, KH_ERR_HIP, "hipStreamCreate(exchange)");
    if (rc == KH_OK && hub) hub->xs[rank] = cm->xs;
    if (hub) cm->seen = hub->n;
    if (rc == KH_OK && !hub) {
        const size_t n = (size_t)(1 + nranks) * SMALL_MAX * sizeof(u64);
        if (dev_malloc((void **)&cm->d_small, n) != hipSuccess || pin_malloc((void **)&cm->h_small, n, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(c, KH_ERR_OOM, "exchange staging");
        }
        if (rc == KH_OK) {
            ncclResult_t r = ncclCommInitRank(&cm->nccl, (int)nranks, *id, (int)rank);
            if (r != ncclSuccess) {
                cm->nccl = nullptr;
                rc = rccl_fail(c, "ncclCommInitRank", r);
            } else {
                int cnt = 0;  // what RCCL itself says the world is (kh_merge_info.nranks_seen: the bench line asserts it == --gpus)
                if (ncclCommCount(cm->nccl, &cnt) == ncclSuccess && cnt > 0) cm->seen = (uint32_t)cnt;
            }
        }
        if (rc == KH_OK) {
            // the watchdog: an RCCL call that has kept this rank inside the library for longer than the time-out is
            // released by aborting the communicator (a peer that never arrives, a link that never comes up)
            try {
                cm->watchdog = std::thread([cm] {
                    while (!cm->stop.load()) {
                        std::this_thread::sleep_for(std::chrono::milliseconds(100));
                        const double since = cm->busy_since.load();
                        if (since != 0.0 && now_ms() - since > cm->timeout_s * 1e3) comm_abort(cm);
                    }
                });
            } catch (...) {  // (no thread: the polls still bound every wait on the stream, only calls blocked inside RCCL are not covered)
            }
        }
    }
    if (rc != KH_OK) comm_release(c);
    return rc;
}

}  // namespace khi
using namespace khi;

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int kh_comm_unique_id(kh_unique_id *out) {
    static_assert(sizeof(kh_unique_id) == sizeof(ncclUniqueId), "kh_unique_id must be an ncclUniqueId");
    if (!out) return KH_ERR_BAD_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return KH_ERR_RCCL;
    memcpy(out, &id, sizeof(id));
    return KH_OK;
}

extern "C" int kh_comm_init(kh_ctx *c, uint32_t nranks, uint32_t rank, const kh_unique_id *id) {
    int rc = enter(c);
    if (rc != KH_OK) return rc;
    if (!id) return fail(c, KH_ERR_BAD_ARG, "kh_comm_init: id is NULL");
    ncclUniqueId nid;
    memcpy(&nid, id, sizeof(nid));
    return comm_setup(c, nranks, rank, &nid, nullptr);
}

extern "C" int kh_merge_across(kh_ctx *c, kh_merge_info *info) {
    if (!c) return KH_ERR_BAD_ARG;
    if (c->comm && c->comm->dead.load())  // (nobody can be waiting on a dead communicator: no gather to join)
        return fail(c, KH_ERR_RCCL, "the communicator was aborted by an earlier failed merge; create a new context and communicator");
    // (a finished merge leaves EVERY rank a shard: this refusal is collective by itself, nobody is waiting in a gather)
    // (poisoned or not -- ADVICE r4: a poisoned shard used to walk into the first gather, where its peers, shards too, never came)
    if (c->shard_shift) return fail(c, KH_ERR_STATE, c->poisoned ? "the table is already a shard (merged before) and the context is poisoned by an earlier error; kh_reset / a new context first"
                                                                  : "the table is already a shard (merged before); kh_reset first");
    // (counts what kh_push / kh_push_text left pending: may fail -- out of memory, table full -- on this rank alone.  The 8-byte
    //  image stays what it is: the exports read it directly -- round 4: the default here widened it first, 13.5 ms and a 43 GB
    //  allocation at configs[3]'s size, and every export then read the 16-byte table)
    int rc = enter(c, ENTER_READ_TAKE);
    if (c->comm && c->comm->nranks > 1) return merge_across_impl(c, info, rc);  // a failed pre-check is reported in the first gather
    if (rc != KH_OK) return rc;
    if (!c->comm) {  // a lone context is its own world
        if (info) {
            memset(info, 0, sizeof(*info));
            info->nranks = 1;
            info->pieces = 1;
        }
        rc = kh_finish(c, nullptr);
        if (rc == KH_OK && info) {
            info->local_distinct = info->owned_distinct = c->h_ctr->distinct;
            info->nranks_seen = info->conserved = 1;
            info->sent_count_sum = info->merged_count_sum = c->h_ctr->kmers;
        }
        return rc;
    }
    return merge_across_impl(c, info, KH_OK);
}

// ---- single-process form: one context and one host thread per device --------------------------------
struct kh_group {
    std::vector<kh_ctx *> ctx;
    LocalHub *hub = nullptr;
};

extern "C" void kh_group_destroy(kh_group *g) {
    if (!g) return;
    for (kh_ctx *c : g->ctx)
        if (c) kh_destroy(c);
    delete g->hub;
    delete g;
}

extern "C" int kh_group_create(kh_group **out, const kh_config *cfg, const int32_t *devices, uint32_t ndev) {
    if (!out || !cfg || !devices || ndev < 1 || ndev > 64) return KH_ERR_BAD_ARG;
    *out = nullptr;
    if (cfg->struct_size != sizeof(kh_config)) return KH_ERR_BAD_ARG;
    kh_group *g = new (std::nothrow) kh_group();
    if (!g) return KH_ERR_OOM;
    bool dup = false;
    for (uint32_t i = 0; i < ndev; ++i)
        for (uint32_t j = 0; j < i; ++j) dup |= devices[i] == devices[j];
    int rc = KH_OK;
    for (uint32_t i = 0; i < ndev && rc == KH_OK; ++i) {
        kh_config c2 = *cfg;
        c2.device = devices[i];
        c2.stream = nullptr;
        c2.flags &= ~KH_FLAG_CALLER_STREAM;
        kh_ctx *c = nullptr;
        rc = kh_create(&c, &c2);
        g->ctx.push_back(c);
    }
    if (rc == KH_OK && ndev > 1) {
        if (dup) {
            g->hub = new (std::nothrow) LocalHub(ndev);
            if (!g->hub) rc = KH_ERR_OOM;
            for (uint32_t i = 0; i < ndev && rc == KH_OK; ++i) rc = comm_setup(g->ctx[i], ndev, i, nullptr, g->hub);
        } else {
            // ncclCommInitRank blocks until every rank has arrived: one thread per rank
            ncclUniqueId id;
            if (ncclGetUniqueId(&id) != ncclSuccess) rc = KH_ERR_RCCL;
            std::vector<int> rcs(ndev, KH_OK);
            if (rc == KH_OK) {
                std::vector<std::thread> th;
                for (uint32_t i = 0; i < ndev; ++i)
                    th.emplace_back([&, i] { rcs[i] = comm_setup(g->ctx[i], ndev, i, &id, nullptr); });
                for (auto &t : th) t.join();
                for (int r : rcs)
                    if (r != KH_OK && rc == KH_OK) rc = r;
            }
        }
    }
    if (rc != KH_OK) {
        kh_group_destroy(g);
        return rc;
    }
    *out = g;
    return KH_OK;
}

extern "C" kh_ctx *kh_group_ctx(kh_group *g, uint32_t rank) { return (g && rank < g->ctx.size()) ? g->ctx[rank] : nullptr; }
extern "C" uint32_t kh_group_size(const kh_group *g) { return g ? (uint32_t)g->ctx.size() : 0; }

extern "C" int kh_group_merge(kh_group *g, kh_merge_info *infos) {
    if (!g) return KH_ERR_BAD_ARG;
    const uint32_t n = (uint32_t)g->ctx.size();
    std::vector<int> rcs(n, KH_OK);
    if (n == 1) return kh_merge_across(g->ctx[0], infos);
    if (g->hub) g->hub->revive();  // (no rank is inside a merge here: a poisoned hub of an earlier failed merge starts afresh)
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n; ++i) th.emplace_back([&, i] { rcs[i] = kh_merge_across(g->ctx[i], infos ? infos + i : nullptr); });
    for (auto &t : th) t.join();
    if (g->hub) {  // every rank has left the merge: what a failed one's ranks kept alive for their peers can go
        for (kh_ctx *c : g->ctx)
            if (c && hipSetDevice(c->device) == hipSuccess) (void)hipDeviceSynchronize();
        g->hub->release_kept();
    }
    for (int r : rcs)  // the status of a rank that failed ITSELF says more than its peers' KH_ERR_PEER
        if (r != KH_OK && r != KH_ERR_PEER) return r;
    for (int r : rcs)
        if (r != KH_OK) return r;
    return KH_OK;
}

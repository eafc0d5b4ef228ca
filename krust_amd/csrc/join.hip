// join.hip -- kh_compare / kh_combine_into: two count tables set against each other on the device (what `kmc_tools simple` and
// Jaccard / containment screens ask of two k-mer databases).  No reference counterpart.  Both tables sit in HBM under the same
// bijective hash, so the join is a scan of one table's slots with a probe of the other per live slot -- the probe profile.hip
// runs per window (probe.hip.h), with the full 64-bit count.
//   join_kernel<SRC, PRB, SINK>   SRC: the 16-byte table (JsWide) or the 8-byte image (JsNarrow), a range of its slots
//                                 PRB: PfWide / PfNarrow of the OTHER table -- any geometry -- or PbNone (a scan without a probe)
//                                 SINK: JkStats (the words of kh_compare) or JkUpsert (count[key] += c in a third table)
//   kh_compare                    two launches on a's stream: a against b, then b alone for its own two words
//   kh_combine_into               one launch per range of source slots on dst's stream (two scans for a union)
#include "ctx.hip.h"
#include "probe.hip.h"

namespace kh {

// (the source views JsWide / JsNarrow -- slot i of the scanned table -> (key, count) -- live in probe.hip.h: graph.hip scans with them too)

// the null probe: every key reads as absent, nothing is loaded
struct PbNone {
    typedef uint32_t Word;
    struct Ref {
        bool mine;
    };
    __device__ __forceinline__ Ref ref(u64) const { return Ref{false}; }
    __device__ static __forceinline__ Word free_word() { return 0u; }
    __device__ static __forceinline__ Word load(const Ref &) { return 0u; }
    __device__ static __forceinline__ u64 resolve64(const Ref &, Word) { return 0ull; }
};

// ---- sinks: take(key, cs, cp) for every key of the source's set -- cs its count there, cp its count in the probed table's set
// (0: not in it) -- then flush() once per lane, all lanes of the wave together -------------------------------------------------
// The words of kh_compare.  B_SIDE: the probe-less scan of b for its own two words.
template <bool B_SIDE>
struct JkStats {
    u64 *words;  // KH_CMP_WORDS, zeroed before the first launch
    struct Acc {
        u64 distinct = 0, sum = 0, shared = 0, shared_s = 0, shared_p = 0, sum_min = 0;
    };
    __device__ __forceinline__ void take(Acc &x, u64, u64 cs, u64 cp) const {
        x.distinct += 1;
        x.sum += cs;
        if (!B_SIDE && cp) {
            x.shared += 1;
            x.shared_s += cs;
            x.shared_p += cp;
            x.sum_min += cs < cp ? cs : cp;
        }
    }
    __device__ __forceinline__ void add(int word, u64 v) const {
        v = wave_sum(v);
        if (lane_id() == 0 && v) (void)__hip_atomic_fetch_add(&words[word], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void flush(const Acc &x) const {
        add(B_SIDE ? KH_CMP_DISTINCT_B : KH_CMP_DISTINCT_A, x.distinct);
        add(B_SIDE ? KH_CMP_SUM_B : KH_CMP_SUM_A, x.sum);
        if (!B_SIDE) {
            add(KH_CMP_SHARED, x.shared);
            add(KH_CMP_SHARED_SUM_A, x.shared_s);
            add(KH_CMP_SHARED_SUM_B, x.shared_p);
            add(KH_CMP_SUM_MIN, x.sum_min);
        }
    }
};

// count[key] += c in the target table, c by the set operation; the counters as table_merge_pairs_kernel keeps them.
struct JkUpsert {
    TableGeom tg;
    uint32_t op, calc;
    Counters *ctr;
    u64 *n_pairs;
    struct Acc {
        uint32_t nd = 0, nf = 0;
        u64 ad = 0, np = 0;
    };
    __device__ __forceinline__ u64 calc_of(u64 cs, u64 cp) const {
        switch (calc) {
            case KH_CALC_MIN: return cs < cp ? cs : cp;
            case KH_CALC_MAX: return cs > cp ? cs : cp;
            case KH_CALC_SUM: return cs + cp < cs ? ~0ull : cs + cp;  // saturates
            case KH_CALC_LEFT: return cs;
            default: return cp;  // KH_CALC_RIGHT
        }
    }
    __device__ __forceinline__ void take(Acc &x, u64 key, u64 cs, u64 cp) const {
        u64 c;
        switch (op) {
            case KH_SET_INTERSECT: c = cp ? calc_of(cs, cp) : 0ull; break;
            case KH_SET_UNION: c = cp ? calc_of(cs, cp) : cs; break;  // (the first of the two scans: see kh_combine_into)
            case KH_SET_SUBTRACT: c = cp ? 0ull : cs; break;
            default: c = cs > cp ? cs - cp : 0ull; break;  // KH_SET_COUNT_SUBTRACT
        }
        if (c) {
            upsert(tg, key, c, x.nd, x.nf);
            x.ad += c;
            x.np += 1;
        }
    }
    __device__ __forceinline__ void flush(const Acc &x) const {
        const u64 d = wave_sum((u64)x.nd), f = wave_sum((u64)x.nf), ad = wave_sum(x.ad), np = wave_sum(x.np);
        if (lane_id() == 0) {
            if (d) atomicAdd(&ctr->distinct, d);
            if (f) atomicAdd(&ctr->failed, f);
            if (ad) atomicAdd(&ctr->kmers, ad);
            if (np) atomicAdd(n_pairs, np);
        }
    }
};

// Slots [s0, s1) of the source, JOIN_PER x BLOCK at a time per workgroup (consecutive lanes read consecutive slots).  A slot is
// in the source's set iff it is live with a count >= min_src; its key is then looked up in the probed table, whose count is
// taken for 0 below min_prb.  As in profile_kernel the eight first-slot loads of a lane are in flight before the first of them
// is looked at: every live slot costs one random line of the probed table.
constexpr int JOIN_PER = 8;
template <typename SRC, typename PRB, typename SINK>
__global__ __launch_bounds__(BLOCK) void join_kernel(SRC src, u64 s0, u64 s1, u64 min_src, PRB prb, u64 min_prb, SINK sink) {
    const u64 T = (u64)JOIN_PER * BLOCK;
    const u64 ntiles = (s1 - s0 + T - 1) / T;
    typename SINK::Acc acc;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        u64 key[JOIN_PER], cs[JOIN_PER];
        typename PRB::Ref ref[JOIN_PER];
        typename PRB::Word first[JOIN_PER];
        uint32_t in = 0;
#pragma unroll
        for (int jj = 0; jj < JOIN_PER; ++jj) {
            const u64 i = s0 + t * T + (u64)jj * BLOCK + threadIdx.x;
            key[jj] = 0;
            cs[jj] = 0;
            if (i < s1 && src.load(i, key[jj], cs[jj]) && cs[jj] >= min_src) in |= 1u << jj;
        }
#pragma unroll
        for (int jj = 0; jj < JOIN_PER; ++jj) {
            ref[jj] = prb.ref(key[jj]);
            first[jj] = PRB::free_word();
            if ((in & (1u << jj)) && ref[jj].mine) first[jj] = PRB::load(ref[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < JOIN_PER; ++jj) {
            if (!(in & (1u << jj))) continue;
            u64 cp = PRB::resolve64(ref[jj], first[jj]);
            if (cp < min_prb) cp = 0;
            sink.take(acc, key[jj], cs[jj], cp);
        }
    }
    sink.flush(acc);
}

}  // namespace kh

namespace khi {

// What both calls refuse before they enter anything: `err` takes the text.
int join_check(kh_ctx *err, const char *who, const kh_ctx *a, const kh_ctx *b, const kh_ctx *dst) {
    const kh_ctx *all[3] = {a, b, dst};
    std::string w = who;
    for (const kh_ctx *x : all) {
        if (!x) continue;
        if (x->k != a->k) return fail(err, KH_ERR_BAD_ARG, (w + ": the contexts have different k").c_str());
        if (x->device != a->device) return fail(err, KH_ERR_BAD_ARG, (w + ": the contexts are on different devices").c_str());
    }
    for (const kh_ctx *x : all)
        if (x && (x->shard_shift != a->shard_shift || x->shard_index != a->shard_index))
            return fail(err, KH_ERR_STATE, (w + ": the contexts are not in the same shard state").c_str());
    return KH_OK;
}

namespace {

constexpr u64 JOIN_WORDS = KH_CMP_WORDS + 1;  // the words of kh_compare, then the pair count of kh_combine_into

int join_words(kh_ctx *c, bool soft) {  // soft: for kh_compare, a reading call
    if (c->jn_words) return KH_OK;
    hipError_t e = dev_malloc((void **)&c->jn_words, JOIN_WORDS * sizeof(u64));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c->jn_words = nullptr;
        return soft ? soft_oom(c, "hipMalloc(join words)", e) : fail(c, KH_ERR_OOM, "hipMalloc(join words)", e);
    }
    return KH_OK;
}

// Slots [s0, s1) of `src` against `prb` (nullptr: no probe) into `sink`, on `on`'s stream.  Both tables in the form they are in.
template <typename SINK>
int join_launch(kh_ctx *on, const kh_ctx *src, u64 s0, u64 s1, u64 min_src, const kh_ctx *prb, u64 min_prb, SINK sink) {
    if (s1 <= s0) return KH_OK;
    const u64 ntiles = (s1 - s0 + (u64)kh::JOIN_PER * kh::BLOCK - 1) / ((u64)kh::JOIN_PER * kh::BLOCK);
    const unsigned blocks = (unsigned)std::min<u64>(ntiles, (u64)grid_cap());
    with_source(src, [&](auto sv) {
        typedef decltype(sv) SRC;
        auto go = [&](auto pv) {
            typedef decltype(pv) PRB;
            hipLaunchKernelGGL((kh::join_kernel<SRC, PRB, SINK>), dim3(blocks), dim3(kh::BLOCK), 0, on->stream, sv, s0, s1, min_src, pv, min_prb, sink);
        };
        if constexpr (std::is_same<SINK, kh::JkStats<true>>::value) go(kh::PbNone{});
        else with_probe(prb, go);
    });
    HIP_TRY(on, hipGetLastError());
    return KH_OK;
}

// a source: pending pushes counted, the table as it is, its stream idle and its counters exact
int join_enter_source(kh_ctx *err, kh_ctx *s) {
    int rc = enter(s, ENTER_READ);
    if (rc == KH_OK) rc = sync_counters(s);
    if (rc != KH_OK && err != s) err->last_error = s->last_error;
    return rc;
}

// One scan of `src` against `prb` into dst, the source's slots in ranges that dst has room for: a range of m slots claims at most
// min(m, bound) new slots of dst.
int combine_scan(kh_ctx *dst, const kh_ctx *src, u64 min_src, const kh_ctx *prb, u64 min_prb, uint32_t op, uint32_t calc, u64 bound) {
    if (bound == 0) return KH_OK;  // (an empty source set: nothing to emit)
    const u64 step = SUB_TILES * kh::TILE;
    for (u64 s0 = 0; s0 < src->cap;) {
        const u64 m = std::min(step, src->cap - s0), claim = std::min(m, bound);
        bool smaller = false;
        int rc = ensure_room(dst, claim, false, &smaller);
        if (rc != KH_OK) return rc;
        const kh::JkUpsert sink{table_geom(dst, dst->table, dst->cap), op, calc, dst->d_ctr, dst->jn_words + KH_CMP_WORDS};
        if ((rc = join_launch(dst, src, s0, s0 + m, min_src, prb, min_prb, sink)) != KH_OK) return rc;
        dst->table_empty = false;
        dst->rheads_valid = false;
        dst->pending_bound += claim;
        s0 += m;
    }
    return KH_OK;
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_compare(kh_ctx *a, kh_ctx *b, uint64_t min_a, uint64_t min_b, uint64_t *out) {
    if (!a) return KH_ERR_BAD_ARG;
    if (!b || !out) return fail(a, KH_ERR_BAD_ARG, "kh_compare: NULL argument");
    int rc = join_check(a, "kh_compare", a, b, nullptr);
    if (rc != KH_OK) return rc;
    if ((rc = join_enter_source(a, a)) != KH_OK) return rc;
    if (b != a && (rc = join_enter_source(a, b)) != KH_OK) return rc;  // (b's stream is drained: the kernels run on a's)
    if ((rc = join_words(a, true)) != KH_OK) return rc;
    const u64 ma = min_a ? min_a : 1, mb = min_b ? min_b : 1;
    HIP_TRY(a, hipMemsetAsync(a->jn_words, 0, JOIN_WORDS * sizeof(u64), a->stream));
    if ((rc = join_launch(a, a, 0, a->cap, ma, b, mb, kh::JkStats<false>{a->jn_words})) != KH_OK) return rc;
    if ((rc = join_launch(a, b, 0, b->cap, mb, nullptr, 0, kh::JkStats<true>{a->jn_words})) != KH_OK) return rc;
    u64 words[KH_CMP_WORDS];
    HIP_TRY(a, hipMemcpyAsync(words, a->jn_words, sizeof(words), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(a, hipStreamSynchronize(a->stream));
    memcpy(out, words, sizeof(words));
    return KH_OK;
}

extern "C" int kh_combine_into(kh_ctx *dst, kh_ctx *a, kh_ctx *b, uint32_t op, uint32_t calc, uint64_t min_a, uint64_t min_b,
                               uint64_t *n_pairs) {
    if (!dst) return KH_ERR_BAD_ARG;
    if (!a || !b) return fail(dst, KH_ERR_BAD_ARG, "kh_combine_into: NULL context");
    if (dst == a || dst == b) return fail(dst, KH_ERR_BAD_ARG, "kh_combine_into: dst must be neither a nor b");
    if (op < KH_SET_INTERSECT || op > KH_SET_COUNT_SUBTRACT) return fail(dst, KH_ERR_BAD_ARG, "kh_combine_into: unknown op");
    const bool uses_calc = op == KH_SET_INTERSECT || op == KH_SET_UNION;
    if (uses_calc && (calc < KH_CALC_MIN || calc > KH_CALC_RIGHT)) return fail(dst, KH_ERR_BAD_ARG, "kh_combine_into: unknown calc");
    int rc = join_check(dst, "kh_combine_into", a, b, dst);
    if (rc != KH_OK) return rc;
    if ((rc = join_enter_source(dst, a)) != KH_OK) return rc;
    if (b != a && (rc = join_enter_source(dst, b)) != KH_OK) return rc;  // (both source streams are drained: the kernels run on dst's)
    if ((rc = enter(dst)) != KH_OK) return rc;
    if ((rc = join_words(dst, false)) != KH_OK) return rc;
    const u64 ma = min_a ? min_a : 1, mb = min_b ? min_b : 1;
    const u64 da = a->h_ctr->distinct, db = b->h_ctr->distinct;  // (exact: join_enter_source read them back)
    HIP_TRY(dst, hipMemsetAsync(dst->jn_words + KH_CMP_WORDS, 0, sizeof(u64), dst->stream));
    if (op == KH_SET_UNION) {
        // a against b: every key of set A, with calc where b holds it too; then b against a: the keys of set B that are not in set A
        // keep their own count -- a subtract with the roles exchanged
        if ((rc = combine_scan(dst, a, ma, b, mb, KH_SET_UNION, calc, da)) != KH_OK) return rc;
        if ((rc = combine_scan(dst, b, mb, a, ma, KH_SET_SUBTRACT, 0, db)) != KH_OK) return rc;
    } else {
        if ((rc = combine_scan(dst, a, ma, b, mb, op, calc, op == KH_SET_INTERSECT ? std::min(da, db) : da)) != KH_OK) return rc;
    }
    u64 np = 0;
    HIP_TRY(dst, hipMemcpyAsync(&np, dst->jn_words + KH_CMP_WORDS, sizeof(u64), hipMemcpyDeviceToHost, dst->stream));
    if ((rc = sync_counters(dst)) != KH_OK) return rc;  // (complete when it returns; an upsert without a free slot shows here)
    if (n_pairs) *n_pairs = np;
    return KH_OK;
}

// graph.hip -- kh_graph_stats / kh_graph_masks*: the de Bruijn graph degrees of a count table (what BCALM / Cuttlefish ask of a
// k-mer database before they build unitigs).  No reference counterpart.  A table against ITSELF: for every k-mer, which of its
// four possible successors and four possible predecessors are also in the table -- eight probes (probe.hip.h) per key, one byte out.
//   graph_kernel<SRC, PRB, SINK>  SRC: a range of slots of the 16-byte table (JsWide) or of the 8-byte image (JsNarrow), or a
//                                      caller's key array (GsKeys: the validity check stands where the liveness test does)
//                                 PRB: PfWide / PfNarrow of the SAME context
//                                 SINK: GkStats (a 256-counter histogram of the masks, the nodes and their counts) or GkMasks
//                                       (one byte per key, stored four at a time)
//   kh_graph_stats                one launch over the table's slots
//   kh_graph_masks_device / kh_graph_masks   one launch over the keys
// The neighbour arithmetic is graph_bits.h (host-checkable).  No kernel waits for another workgroup.
#include "ctx.hip.h"
#include "graph_bits.h"
#include "probe.hip.h"

namespace kh {

// graph_mask_of(prb, x, k, min_count), the mask of one key, is in probe.hip.h: unitig.hip asks it too.

// ---- the caller's keys as a source: any alignment -----------------------------------------------------------------------------
struct GsKeys {
    const uint8_t *keys;
    bool aligned;  // 8-byte aligned: one 64-bit load per key
    __device__ __forceinline__ u64 key(u64 i) const {
        if (aligned) return reinterpret_cast<const u64 *>(keys)[i];
        u64 v = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) v |= (u64)keys[i * 8 + b] << (8 * b);
        return v;
    }
};

// ---- sinks ---------------------------------------------------------------------------------------------------------------------
constexpr int GRAPH_WAVES = BLOCK / 64;
constexpr int GRAPH_PER = 4;                    // slots (stats) / keys (masks) per lane per tile
constexpr int GRAPH_TILE = GRAPH_PER * BLOCK;   // 1024

// The words of kh_graph_stats.  SCAN: the kernel scans slots, compacts the tile's nodes through LDS so that the probing lanes are
// dense (a table is half free slots, and a threshold leaves fewer nodes still), and counts every node's mask with one LDS atomic
// into the wave's own 256 counters.  Once per workgroup, behind its grid-stride loop: one return-less 64-bit atomic per non-zero
// counter; the nodes and the sum of their counts as JkStats adds its words.  Never a global atomic per node.
struct GkStats {
    static constexpr bool SCAN = true;
    u64 *words;  // KH_GRAPH_WORDS, zeroed on the stream before the launch
};
// One byte per key.  A lane owns GRAPH_PER = 4 consecutive bytes of d_masks that start at a 4-byte boundary, so they leave as one
// aligned 32-bit store; only the first and the last such group of the array can be cut short, and those go byte by byte.
struct GkMasks {
    static constexpr bool SCAN = false;
    uint8_t *masks;  // d_masks
};

// SCAN (GkStats): slots [s0, s1) of the table, GRAPH_TILE at a time per workgroup (consecutive lanes read consecutive slots).
// otherwise (GkMasks): keys [s0, s1) of the array; `shift` = d_masks & 3, and group u holds the bytes d_masks - shift + 4u ..+3.
template <typename SRC, typename PRB, typename SINK>
__global__ __launch_bounds__(BLOCK) void graph_kernel(SRC src, u64 s0, u64 s1, uint32_t k, u64 min_count, PRB prb, SINK sink, uint32_t shift) {
    if constexpr (SINK::SCAN) {
        __shared__ u64 s_key[GRAPH_TILE];
        __shared__ u64 s_cnt[GRAPH_TILE];
        __shared__ uint32_t s_hist[GRAPH_WAVES][256];
        __shared__ uint32_t s_n;
        const uint32_t tid = threadIdx.x, wave = tid >> 6;
        for (uint32_t i = tid; i < GRAPH_WAVES * 256; i += BLOCK) (&s_hist[0][0])[i] = 0;
        const u64 ntiles = (s1 - s0 + GRAPH_TILE - 1) / GRAPH_TILE;
        u64 nodes = 0, kmers = 0;
        for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
            if (tid == 0) s_n = 0;
            u64 key[GRAPH_PER], cnt[GRAPH_PER];
            bool in[GRAPH_PER];
#pragma unroll
            for (int jj = 0; jj < GRAPH_PER; ++jj) {
                const u64 i = s0 + t * GRAPH_TILE + (u64)jj * BLOCK + tid;
                key[jj] = cnt[jj] = 0;
                in[jj] = i < s1 && src.load(i, key[jj], cnt[jj]) && cnt[jj] >= min_count;
            }
            __syncthreads();  // s_n is 0, and the previous tile's queue has been read
#pragma unroll
            for (int jj = 0; jj < GRAPH_PER; ++jj) {
                const u64 m = kh_ballot(in[jj]);
                if (m == 0) continue;  // (wave-uniform)
                uint32_t wbase = 0;
                if ((int)lane_id() == __builtin_ctzll(m)) wbase = atomicAdd(&s_n, (uint32_t)__builtin_popcountll(m));
                wbase = (uint32_t)__shfl((int)wbase, __builtin_ctzll(m), 64);
                if (in[jj]) {
                    const uint32_t q = wbase + mbcnt(m);  // < GRAPH_TILE: at most one entry per slot of the tile
                    s_key[q] = key[jj];
                    s_cnt[q] = cnt[jj];
                }
            }
            __syncthreads();
            const uint32_t n = s_n;
            for (uint32_t q = tid; q < n; q += BLOCK) {
                const uint32_t mask = graph_mask_of(prb, s_key[q], k, min_count);
                atomicAdd(&s_hist[wave][mask], 1u);
                nodes += 1;
                kmers += s_cnt[q];
            }
            __syncthreads();  // the queue is read: the next tile may reset s_n
        }
        __syncthreads();
        {
            u64 v = 0;
#pragma unroll
            for (int w = 0; w < GRAPH_WAVES; ++w) v += s_hist[w][tid];  // (BLOCK == 256: one counter per lane)
            if (v) (void)__hip_atomic_fetch_add(&sink.words[tid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        nodes = wave_sum(nodes);
        kmers = wave_sum(kmers);
        if (lane_id() == 0) {
            if (nodes) (void)__hip_atomic_fetch_add(&sink.words[KH_GRAPH_NODES], nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (kmers) (void)__hip_atomic_fetch_add(&sink.words[KH_GRAPH_KMERS], kmers, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        static_assert(GRAPH_PER == 4, "a group is one 32-bit store");
        const u64 n = s1 - s0;
        const u64 ngroups = (n + shift + 3) / 4;
        uint8_t *base = sink.masks - shift;  // 4-byte aligned
        for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < ngroups; u += (u64)gridDim.x * BLOCK) {
            uint32_t word = 0;
#pragma unroll 1
            for (int b = 0; b < 4; ++b) {  // (one key after the other: eight loads in flight per lane, not thirty-two)
                const u64 v = 4 * u + b;  // byte index from `base`; key index v - shift
                if (v < shift || v - shift >= n) continue;
                const u64 x = src.key(s0 + (v - shift));
                const uint32_t mask = kh_graph_key_valid(x, k) ? graph_mask_of(prb, x, k, min_count) : 0u;
                word |= mask << (8 * b);
            }
            if (4 * u >= shift && 4 * u + 4 <= n + shift) {
                *reinterpret_cast<uint32_t *>(base + 4 * u) = word;
            } else {  // the two cut groups at the ends of d_masks
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const u64 v = 4 * u + b;
                    if (v >= shift && v - shift < n) base[v] = (uint8_t)(word >> (8 * b));
                }
            }
        }
    }
}

}  // namespace kh

namespace khi {
namespace {

// What all three calls do before they look at the table: neighbours of a shard's keys live on other owners.
int graph_enter(kh_ctx *c, const char *who) {
    if (c->shard_shift) return fail(c, KH_ERR_STATE, (std::string(who) + ": the table is a shard; its k-mers' neighbours live on other owners").c_str());
    return enter(c, ENTER_READ);
}

// One launch of graph_kernel on c's stream: the source against c's own table in the form it is in.
template <typename SRC, typename SINK>
int graph_launch_on(kh_ctx *c, SRC sv, u64 s0, u64 s1, u64 groups, u64 min_count, SINK sink, uint32_t shift) {
    const unsigned blocks = (unsigned)std::min<u64>(groups, (u64)grid_cap());
    with_probe(c, [&](auto pv) {
        typedef decltype(pv) PRB;
        // (a slot source is the context's own table: only the probe of the same form is instantiated with it)
        constexpr bool other_form = (std::is_same<SRC, kh::JsWide>::value && std::is_same<PRB, kh::PfNarrow>::value) ||
                                    (std::is_same<SRC, kh::JsNarrow>::value && std::is_same<PRB, kh::PfWide>::value);
        if constexpr (!other_form)
            hipLaunchKernelGGL((kh::graph_kernel<SRC, PRB, SINK>), dim3(blocks), dim3(kh::BLOCK), 0, c->stream, sv, s0, s1, c->k, min_count, pv, sink, shift);
    });
    HIP_TRY(c, hipGetLastError());
    return KH_OK;
}

// The masks of n keys in device memory into n bytes of device memory, on c's stream (not synchronised).
int graph_masks_launch(kh_ctx *c, const void *d_keys, u64 n, u64 min_count, uint8_t *d_masks) {
    const uint32_t shift = (uint32_t)((uintptr_t)d_masks & 3u);
    const u64 ngroups = (n + shift + 3) / 4;
    const kh::GsKeys sv{(const uint8_t *)d_keys, ((uintptr_t)d_keys & 7u) == 0};
    return graph_launch_on(c, sv, 0, n, (ngroups + kh::BLOCK - 1) / kh::BLOCK, min_count, kh::GkMasks{d_masks}, shift);
}

}  // namespace
}  // namespace khi
using namespace khi;

extern "C" int kh_graph_stats(kh_ctx *c, uint64_t min_count, uint64_t *out) {
    if (!c) return KH_ERR_BAD_ARG;
    if (!out) return fail(c, KH_ERR_BAD_ARG, "kh_graph_stats: NULL out");
    int rc = graph_enter(c, "kh_graph_stats");
    if (rc != KH_OK) return rc;
    if (!c->gr_words) {
        hipError_t e = dev_malloc((void **)&c->gr_words, KH_GRAPH_WORDS * sizeof(u64));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            c->gr_words = nullptr;
            return soft_oom(c, "hipMalloc(graph words)");
        }
    }
    const u64 mc = min_count ? min_count : 1;
    HIP_TRY(c, hipMemsetAsync(c->gr_words, 0, KH_GRAPH_WORDS * sizeof(u64), c->stream));
    if (c->cap) {
        const u64 ntiles = (c->cap + kh::GRAPH_TILE - 1) / kh::GRAPH_TILE;
        const kh::GkStats sink{c->gr_words};
        with_source(c, [&](auto sv) { rc = graph_launch_on(c, sv, 0, c->cap, ntiles, mc, sink, 0); });
        if (rc != KH_OK) return rc;
    }
    u64 words[KH_GRAPH_WORDS];
    HIP_TRY(c, hipMemcpyAsync(words, c->gr_words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(out, words, sizeof(words));
    return KH_OK;
}

extern "C" int kh_graph_masks_device(kh_ctx *c, const uint64_t *d_keys, uint64_t n, uint64_t min_count, uint8_t *d_masks) {
    if (!c) return KH_ERR_BAD_ARG;
    if (n && (!d_keys || !d_masks)) return fail(c, KH_ERR_BAD_ARG, "kh_graph_masks_device: NULL argument");
    int rc = graph_enter(c, "kh_graph_masks_device");
    if (rc != KH_OK || n == 0) return rc;
    if ((rc = graph_masks_launch(c, d_keys, n, min_count ? min_count : 1, d_masks)) != KH_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KH_OK;
}

extern "C" int kh_graph_masks(kh_ctx *c, const uint64_t *keys, uint64_t n, uint64_t min_count, uint8_t *masks) {
    if (!c) return KH_ERR_BAD_ARG;
    if (n && (!keys || !masks)) return fail(c, KH_ERR_BAD_ARG, "kh_graph_masks: NULL argument");
    int rc = graph_enter(c, "kh_graph_masks");
    if (rc != KH_OK || n == 0) return rc;
    // as kh_lookup: device scratch for this call alone, one launch, copy back
    CallScratch sc(c);
    u64 *const dk = n > (~0ull >> 4) ? nullptr : (u64 *)sc.fresh(n * sizeof(u64));
    uint8_t *const dm = dk ? (uint8_t *)sc.fresh(n) : nullptr;
    if (!dm) return soft_oom(c, "hipMalloc(graph masks)");
    hipError_t e = hipMemcpyAsync(dk, keys, n * sizeof(u64), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        rc = graph_masks_launch(c, dk, n, min_count ? min_count : 1, dm);
        if (rc == KH_OK) e = hipMemcpyAsync(masks, dm, n, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);  // (an error of the stream is this call's to report, not the scratch's)
    if (e == hipSuccess) e = es;
    if (rc != KH_OK) return rc;
    if (e != hipSuccess) return fail(c, KH_ERR_HIP, "kh_graph_masks", e);
    return KH_OK;
}

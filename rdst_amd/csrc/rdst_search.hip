// rdst_search.hip — binary search on the device (rdst_hip_search_device; include/rdst_hip.h): for every needle
// the number of keys of a sorted array that order before it (lower) and before or equal to it (upper), in the sort's order —
// the mapped bits.  The device twin of `partition_point` / `binary_search` on a sorted slice and of numpy.searchsorted.
//
// Two launches:
//   1. search_prepare_kernel, one workgroup: reads the length m, checks it against len (past it: the error bit, a mark in the
//      header, and the second launch returns at once), writes the header and SPLITTERS evenly spaced MAPPED keys of the
//      haystack into the caller's scratch — the top levels of every search, contiguous;
//   2. search_kernel, one workgroup per tile of needles: loads and maps its needles, reduces their smallest and largest,
//      copies the splitters to LDS and has two threads find [lo, hi) = [lower(min), upper(max)), the only stretch of the
//      haystack a needle of this tile can land in.  hi - lo <= the window: the stretch is staged in LDS, mapped, and every
//      needle is searched there (the staged path).  Otherwise every needle is searched in the splitters in LDS and then in
//      the one gap between two splitters in global memory (the table path).
// Every search is a loop of a fixed number of steps that the data cannot change, a thread walks all of its needles through
// it in lockstep (their loads are independent), every index is below m by construction, and a position is lo + (hi - lo) / 2.
// An unsorted haystack therefore gets some position in [0, m] for every needle and nothing else.
// Nothing in front of the test hook at the end of this file copies to the host, waits for the stream or an event, or touches
// the library's workspace; tests/test_search_abi.py holds that against this text.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_device.h"
#include "rdst_search_layout.h"

namespace {

namespace L = rdst_search_layout;

constexpr uint32_t ERR_LEN_PAST_CAPACITY = 32;  // as the _devlen sorts raise it

typedef uint32_t search_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t read_length(const void* dev_len, uint32_t len_bytes, uint64_t len) {
    if (dev_len == nullptr) return len;
    return len_bytes == 4 ? (uint64_t)*static_cast<const uint32_t*>(dev_len) : *static_cast<const uint64_t*>(dev_len);
}

__device__ __forceinline__ int bit_width(uint32_t x) { return x ? 32 - __builtin_clz(x) : 0; }  // halvings that take x to 0

// N searches in lockstep: lo[i] becomes the first position p of [lo[i], hi[i]] with !(key_at(p) before q[i]), where "before"
// is < (UPPER: <=); hi[i] if there is none.  `steps` >= bit_width(hi[i] - lo[i]) for every i: a step halves what is left, so
// the loop has converged when it ends whatever the keys are.  key_at is called for positions in [lo[i], hi[i]) and for
// position 0 (a search that has ended loads that one, so that no load hangs on a branch).  lo[i] > hi[i] stays as it is.
template <bool UPPER, int N, typename K, typename F>
__device__ __forceinline__ void bisect(F key_at, const K (&q)[N], uint32_t (&lo)[N], uint32_t (&hi)[N], int steps) {
    for (int s = 0; s < steps; ++s) {
        K k[N];
        uint32_t mid[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            mid[i] = lo[i] < hi[i] ? lo[i] + (hi[i] - lo[i]) / 2 : 0u;  // never (lo + hi) / 2: positions reach 2^32 - 1
            k[i] = key_at(mid[i]);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const bool open = lo[i] < hi[i];
            const bool before = UPPER ? k[i] <= q[i] : k[i] < q[i];
            if (open && before) lo[i] = mid[i] + 1;
            if (open && !before) hi[i] = mid[i];
        }
    }
}

// The table path of N needles: the splitters in LDS, then the one gap in global memory.  m > 0.  out[i] in [0, m].
template <bool UPPER, int N, typename K>
__device__ __forceinline__ void locate(const K* __restrict__ sorted, const K* table, uint32_t m, K neg, K pos, const K (&q)[N], uint32_t (&out)[N]) {
    uint32_t c[N], top[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        c[i] = 0;
        top[i] = L::SPLITTERS;
    }
    bisect<UPPER>([&](uint32_t p) { return table[p]; }, q, c, top, bit_width(L::SPLITTERS));
    // c splitters are before q: so is the key at splitter c - 1's position, and the key at splitter c's is not
    uint32_t hi[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        out[i] = c[i] > 0 ? L::splitter_pos(c[i] - 1, m) + 1 : 0u;  // <= m: every splitter's position is below m
        hi[i] = c[i] < L::SPLITTERS ? L::splitter_pos(c[i], m) : m;
    }
    bisect<UPPER>([&](uint32_t p) { return map_key<K>(sorted[p], neg, pos); }, q, out, hi, bit_width(L::longest_gap(m)));
}

template <typename K>
__global__ __launch_bounds__(L::THREADS) void search_prepare_kernel(const K* __restrict__ sorted, uint64_t len, const void* __restrict__ dev_len,
                                                                    uint32_t len_bytes, uint64_t* __restrict__ hdr, K* __restrict__ splitters, K neg, K pos,
                                                                    uint32_t* __restrict__ err) {
    const uint64_t m64 = read_length(dev_len, len_bytes, len);
    const bool past = m64 > len;
    if (threadIdx.x == 0) {
        hdr[L::HDR_M] = m64;
        hdr[L::HDR_STAGED] = 0;
        hdr[L::HDR_TABLE] = 0;
        hdr[L::HDR_PAST] = past ? 1u : 0u;
        if (past) atomicOr(err, ERR_LEN_PAST_CAPACITY);
    }
    if (past || m64 == 0) return;  // (no key to take a splitter from: search_kernel reads none)
    const uint32_t m = (uint32_t)m64;  // m <= len < 2^32
    for (uint32_t j = threadIdx.x; j < L::SPLITTERS; j += L::THREADS) splitters[j] = map_key<K>(sorted[L::splitter_pos(j, m)], neg, pos);
}

template <typename K, typename OFF>
__global__ __launch_bounds__(L::THREADS) void search_kernel(const K* __restrict__ sorted, const K* __restrict__ needles, uint32_t n_needles,
                                                            OFF* __restrict__ out_lower, OFF* __restrict__ out_upper, uint64_t* __restrict__ hdr,
                                                            const K* __restrict__ splitters, K neg, K pos) {
    constexpr int V = 16 / (int)sizeof(K);  // keys per 16-byte load
    constexpr int N = (int)L::needles_per_thread((uint32_t)sizeof(K));
    constexpr int ROWS = N / V;
    constexpr uint32_t T = L::needles_per_tile((uint32_t)sizeof(K));
    constexpr uint32_t WINDOW = L::window((uint32_t)sizeof(K));
    static_assert(N % V == 0 && WINDOW >= L::SPLITTERS && WINDOW >= 2 * L::THREADS, "s_keys holds the reduction, the splitters and the window in turn");
    __shared__ K s_keys[WINDOW];
    __shared__ uint32_t s_lo, s_hi;
    const uint32_t tid = threadIdx.x;

    if (hdr[L::HDR_PAST] != 0) return;  // m > len: nothing at all is written
    const uint32_t m = (uint32_t)hdr[L::HDR_M];
    const uint64_t base = (uint64_t)blockIdx.x * T;
    auto index_of = [&](int j, int v) { return base + (uint64_t)(j * (int)L::THREADS + (int)tid) * V + v; };  // < 2^32 + T
    auto store = [&](OFF* __restrict__ out, const uint32_t (&p)[N]) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (index_of(j, v) < n_needles) out[index_of(j, v)] = (OFF)p[j * V + v];
    };
    if (m == 0) {
        uint32_t zero[N] = {};
        if (out_lower) store(out_lower, zero);
        if (out_upper) store(out_upper, zero);
        return;
    }

    // the needles, mapped; the slots past the last needle hold the tile's neutral elements below and a key of 0 afterwards
    K q[N];
    K lowest = (K)~(K)0, highest = (K)0;
    if (base + T <= n_needles && (reinterpret_cast<uintptr_t>(needles) & 15u) == 0) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const search_u32x4 x = *reinterpret_cast<const search_u32x4*>(needles + index_of(j, 0));
            __builtin_memcpy(&q[j * V], &x, 16);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = map_key<K>(q[i], neg, pos);
    } else {  // the last tile, or a base that is aligned to the element only: key by key, in the same places
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) q[j * V + v] = index_of(j, v) < n_needles ? map_key<K>(needles[index_of(j, v)], neg, pos) : (K)0;
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (index_of(j, v) < n_needles) {
                lowest = q[j * V + v] < lowest ? q[j * V + v] : lowest;
                highest = q[j * V + v] > highest ? q[j * V + v] : highest;
            }

    // the tile's smallest and largest needle: a tree over LDS
    s_keys[tid] = lowest;
    s_keys[L::THREADS + tid] = highest;
    __syncthreads();
    for (uint32_t half = L::THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
            const K a = s_keys[tid + half], b = s_keys[L::THREADS + tid + half];
            if (a < s_keys[tid]) s_keys[tid] = a;
            if (b > s_keys[L::THREADS + tid]) s_keys[L::THREADS + tid] = b;
        }
        __syncthreads();
    }
    lowest = s_keys[0];
    highest = s_keys[L::THREADS];
    __syncthreads();

    // the splitters, and [lower(min), upper(max)) by one thread each of two waves
    for (uint32_t j = tid; j < L::SPLITTERS; j += L::THREADS) s_keys[j] = splitters[j];
    __syncthreads();
    if (tid == 0 || tid == 64) {
        const K one[1] = {tid == 0 ? lowest : highest};
        uint32_t at[1];
        if (tid == 0) {
            locate<false>(sorted, s_keys, m, neg, pos, one, at);
            s_lo = at[0];
        } else {
            locate<true>(sorted, s_keys, m, neg, pos, one, at);
            s_hi = at[0];
        }
    }
    __syncthreads();
    const uint32_t lo = s_lo, hi = s_hi;                // both in [0, m]
    const bool staged = hi >= lo && hi - lo <= WINDOW;  // (hi < lo: only an unsorted haystack gives that)
    if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long*>(hdr + (staged ? L::HDR_STAGED : L::HDR_TABLE)), 1ull);

    uint32_t first[N], last[N];
    if (staged) {
        const uint32_t w = hi - lo;
        for (uint32_t i = tid; i < w; i += L::THREADS) s_keys[i] = map_key<K>(sorted[lo + i], neg, pos);  // (every thread is past the splitters)
        __syncthreads();
        const int steps = bit_width(w);
        auto key_at = [&](uint32_t p) { return s_keys[p]; };
#pragma unroll
        for (int i = 0; i < N; ++i) {
            first[i] = 0;
            last[i] = w;
        }
        if (out_lower) {
            bisect<false>(key_at, q, first, last, steps);
            uint32_t p[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                p[i] = lo + first[i];
                last[i] = w;  // upper(q) >= lower(q): the second search starts where the first one ended
            }
            store(out_lower, p);
        }
        if (out_upper) {
            bisect<true>(key_at, q, first, last, steps);
            uint32_t p[N];
#pragma unroll
            for (int i = 0; i < N; ++i) p[i] = lo + first[i];
            store(out_upper, p);
        }
    } else {
        if (out_lower) {
            locate<false>(sorted, s_keys, m, neg, pos, q, first);
            store(out_lower, first);
        }
        if (out_upper) {
            locate<true>(sorted, s_keys, m, neg, pos, q, last);
            store(out_upper, last);
        }
    }
}

template <typename K, typename OFF>
int search_launch(const void* sorted, uint64_t len, const void* dev_len, uint32_t len_bytes, const void* needles, uint64_t n_needles, void* out_lower,
                  void* out_upper, void* scratch, rdst_key_kind kind, uint32_t* err, hipStream_t s) {
    unsigned __int128 neg128, pos128;
    rdst_internal::key_xor_masks(kind, (uint32_t)sizeof(K), &neg128, &pos128);
    const K neg = (K)neg128, pos = (K)pos128;
    uint64_t* hdr = static_cast<uint64_t*>(scratch);
    K* splitters = reinterpret_cast<K*>(static_cast<char*>(scratch) + L::HEADER_BYTES);
    // the first launch writes the header and the table: the scratch needs no clearing
    int rc = rdst_internal::launch("search_prepare_kernel", search_prepare_kernel<K>, dim3(1), dim3(L::THREADS), 0, s, static_cast<const K*>(sorted), len, dev_len,
                                   len_bytes, hdr, splitters, neg, pos, err);
    if (rc) return rc;
    constexpr uint32_t T = L::needles_per_tile((uint32_t)sizeof(K));
    const uint64_t tiles = (n_needles + T - 1) / T;
    return rdst_internal::launch("search_kernel", search_kernel<K, OFF>, dim3((uint32_t)tiles), dim3(L::THREADS), 0, s, static_cast<const K*>(sorted),
                                 static_cast<const K*>(needles), (uint32_t)n_needles, static_cast<OFF*>(out_lower), static_cast<OFF*>(out_upper), hdr,
                                 static_cast<const K*>(splitters), neg, pos);
}

template <typename OFF>
int search_by_width(uint32_t elem_bytes, const void* sorted, uint64_t len, const void* dev_len, uint32_t len_bytes, const void* needles, uint64_t n_needles,
                    void* out_lower, void* out_upper, void* scratch, rdst_key_kind kind, uint32_t* err, hipStream_t s) {
    switch (elem_bytes) {
        case 1: return search_launch<uint8_t, OFF>(sorted, len, dev_len, len_bytes, needles, n_needles, out_lower, out_upper, scratch, kind, err, s);
        case 2: return search_launch<uint16_t, OFF>(sorted, len, dev_len, len_bytes, needles, n_needles, out_lower, out_upper, scratch, kind, err, s);
        case 4: return search_launch<uint32_t, OFF>(sorted, len, dev_len, len_bytes, needles, n_needles, out_lower, out_upper, scratch, kind, err, s);
        case 8: return search_launch<uint64_t, OFF>(sorted, len, dev_len, len_bytes, needles, n_needles, out_lower, out_upper, scratch, kind, err, s);
        default: return search_launch<u128, OFF>(sorted, len, dev_len, len_bytes, needles, n_needles, out_lower, out_upper, scratch, kind, err, s);
    }
}

}  // namespace

extern "C" int rdst_hip_search_device(const void* dev_sorted, uint64_t len, const void* dev_len, uint32_t len_bytes, const void* dev_needles,
                                      uint64_t n_needles, void* dev_out_lower, void* dev_out_upper, uint32_t offset_bytes, void* dev_scratch,
                                      uint64_t scratch_bytes, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, uint32_t flags, void* stream) {
    int rc = rdst_internal::search_check_args(dev_sorted, len, dev_len, len_bytes, dev_needles, n_needles, dev_out_lower, dev_out_upper, offset_bytes,
                                              dev_scratch, scratch_bytes, elem_bytes, kind, levels, flags);
    if (rc) return rc;
    if (n_needles == 0) return RDST_OK;  // no device work
    uint32_t* err = nullptr;
    if ((rc = rdst_internal::device_error_word(&err))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (offset_bytes == 4)
        return search_by_width<uint32_t>(elem_bytes, dev_sorted, len, dev_len, len_bytes, dev_needles, n_needles, dev_out_lower, dev_out_upper, dev_scratch,
                                         kind, err, s);
    return search_by_width<uint64_t>(elem_bytes, dev_sorted, len, dev_len, len_bytes, dev_needles, n_needles, dev_out_lower, dev_out_upper, dev_scratch, kind,
                                     err, s);
}

// Test hook, BLOCKING: the header the last call on `stream` left in its scratch.
extern "C" int rdst_hip_debug_search_state(const void* dev_scratch, void* stream, uint64_t out[4]) {
    if (dev_scratch == nullptr || out == nullptr) return rdst_internal::set_error(RDST_ERR_ARG, "search: null scratch or output");
    if (reinterpret_cast<uintptr_t>(dev_scratch) % 256) return rdst_internal::set_error(RDST_ERR_ALIGN, "search: scratch not aligned to 256 bytes");
    static_assert(L::HDR_M == 0 && L::HDR_STAGED == 1 && L::HDR_TABLE == 2 && L::HDR_PAST == 3, "out[] is the header's first four words");
    hipStream_t s = static_cast<hipStream_t>(stream);
    RDST_HIP_TRY(hipMemcpyAsync(out, dev_scratch, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    return RDST_OK;
}

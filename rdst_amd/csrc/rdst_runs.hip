// rdst_runs.hip — runs of bit-identical keys on the device (rdst_hip_runs_device; include/rdst_hip.h): the key
// and the first position of every run and the number of runs, the positions closed into a CSR table that every
// *_device_offsets entry takes.  The device twin of `v.dedup()` after `v.radix_sort_unstable()`; the host never learns how
// many runs there are.
//
// One read of the input and one pass — a chained scan with decoupled look-back (runs_kernel):
//   1. a workgroup draws its tile number from a ticket counter in the scratch, so the workgroups of all earlier tiles have
//      started (the rule K3 of rdst_kernels.hip relies on): a wait for them ends;
//   2. it loads its tile — each wave a contiguous quarter, rows(elem_bytes) 16-byte loads per lane — and the key in front of
//      each quarter with one plain load;
//   3. it marks the heads (position 0, and key[i] != key[i - 1] on the raw bits) and scans them: lanes, rows, waves;
//   4. thread 0 publishes the tile's head count in ONE 64-bit status word (state in the top two bits, value below:
//      StatusWord<uint64_t>), walks back over the earlier tiles' words until an inclusive one and republishes its own as
//      inclusive.  The word IS the payload: nothing is handed over behind a flag, so relaxed agent-scope atomics on that
//      word are all the ordering there is;
//   5. every head whose global rank is below the capacity stores its key and position; the head of rank == capacity
//      stores the closing border of a truncated table;
//   6. the workgroup that owns element m - 1 writes n_runs, the closing border and, if the runs do not fit, the truncation
//      bit.
// RDST_RUNS_PAD_STARTS is a second launch (runs_pad_kernel) sized by the capacity.  Nothing here copies to the host, waits
// for the stream or an event, or touches the library's workspace; tests/test_runs_abi.py holds that against this text.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_device.h"
#include "rdst_runs_layout.h"

namespace {

namespace L = rdst_runs_layout;

constexpr uint32_t ERR_LOOKBACK_TIMEOUT = 1;    // as in rdst_kernels.hip
constexpr uint32_t ERR_LEN_PAST_CAPACITY = 32;  // as the _devlen sorts raise it
constexpr uint32_t ERR_RUNS_TRUNCATED = 64;     // more runs than out_capacity: the first out_capacity are complete

typedef uint32_t runs_u32x4 __attribute__((ext_vector_type(4)));

template <typename K>
__device__ __forceinline__ K shfl_key(K k, int src) {  // lane `src`'s k
    if constexpr (sizeof(K) <= 4) {
        return (K)__shfl((uint32_t)k, src);
    } else {
        uint32_t w[sizeof(K) / 4];
        __builtin_memcpy(w, &k, sizeof(K));
#pragma unroll
        for (int i = 0; i < (int)(sizeof(K) / 4); ++i) w[i] = __shfl(w[i], src);
        __builtin_memcpy(&k, w, sizeof(K));
        return k;
    }
}

__device__ __forceinline__ uint64_t read_length(const void* dev_len, uint32_t len_bytes, uint64_t len) {
    if (dev_len == nullptr) return len;
    return len_bytes == 4 ? (uint64_t)*static_cast<const uint32_t*>(dev_len) : *static_cast<const uint64_t*>(dev_len);
}

// Decoupled look-back over one word per tile: the sum of the head counts of tiles t - 1, t - 2, ... up to and including the
// first INCLUSIVE one, LOOKBACK_WINDOW words per round trip.  Bounded as lookback_walk (rdst_kernels.hip) is: false after
// SPIN_LIMIT polls of a word that stays EMPTY (the bit is raised here), or once another workgroup has raised it — looked
// for every 256 polls, so that one failure ends the launch.  Only that bit: a truncation left unread by an earlier call is
// no reason to stop.
__device__ __forceinline__ bool runs_lookback(const uint64_t* status, uint32_t t, uint32_t* err, uint64_t& excl) {
    constexpr int SSHIFT = StatusWord<uint64_t>::SHIFT;
    constexpr uint64_t SMASK = StatusWord<uint64_t>::MASK;
    constexpr int WINDOW = (int)L::LOOKBACK_WINDOW;
    int64_t prev = (int64_t)t - 1;  // next tile whose word is still to be consumed
    uint32_t spins = 0;
    bool done = false;
    while (!done) {
        uint64_t v[WINDOW];
#pragma unroll
        for (int k = 0; k < WINDOW; ++k) {
            const int64_t idx = prev - k;
            // tile 0 is always INCLUSIVE, so an index below 0 is never consumed
            v[k] = idx >= 0 ? ld_relaxed<uint64_t>(status + idx) : ((uint64_t)ST_INCL << SSHIFT);
        }
        bool blocked = false;
        int consumed = 0;
#pragma unroll
        for (int k = 0; k < WINDOW; ++k) {
            const uint32_t st = (uint32_t)(v[k] >> SSHIFT);
            if (!done && !blocked) {
                if (st == ST_EMPTY) {
                    blocked = true;
                } else {
                    excl += v[k] & SMASK;
                    ++consumed;
                    done = st == ST_INCL;
                }
            }
        }
        prev -= consumed;
        if (blocked && !done) {
            __builtin_amdgcn_s_sleep(2);
            ++spins;
            if (spins > SPIN_LIMIT) {
                atomicOr(err, ERR_LOOKBACK_TIMEOUT);
                return false;
            }
            if ((spins & 255u) == 0 && (ld_relaxed<uint32_t>(err) & ERR_LOOKBACK_TIMEOUT) != 0) return false;
        }
    }
    return true;
}

// `cap`: min(out_capacity, 2^32 - 1) — no rank reaches 2^32 —; 0: the counting call, out_keys and out_starts are null then.
template <typename K, typename OFF>
__global__ __launch_bounds__(L::THREADS) void runs_kernel(const K* __restrict__ keys, uint64_t len, const void* __restrict__ dev_len, uint32_t len_bytes,
                                                          K* __restrict__ out_keys, OFF* __restrict__ out_starts, OFF* __restrict__ n_runs, uint32_t cap,
                                                          uint32_t* __restrict__ ticket, uint64_t* __restrict__ status, uint32_t* __restrict__ err) {
    constexpr int V = 16 / (int)sizeof(K);                      // keys per 16-byte load
    constexpr int ROWS = (int)L::rows((uint32_t)sizeof(K));
    constexpr uint32_t T = L::keys_per_tile((uint32_t)sizeof(K));  // keys per tile
    constexpr int WAVES = (int)L::THREADS / 64;
    constexpr uint32_t WAVE_KEYS = T / WAVES;
    constexpr int SSHIFT = StatusWord<uint64_t>::SHIFT;
    __shared__ uint32_t s_tile, s_fail;
    __shared__ uint32_t s_wave[WAVES];
    __shared__ uint64_t s_excl;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

    // 1. the ticket: this workgroup's tile
    if (tid == 0) s_tile = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t t = s_tile;
    const uint64_t m = read_length(dev_len, len_bytes, len);
    if (m > len) {  // nothing at all is written
        if (t == 0 && tid == 0) atomicOr(err, ERR_LEN_PAST_CAPACITY);
        return;
    }
    const uint64_t base = (uint64_t)t * T;
    if (base >= m && t != 0) return;  // (m == 0: tile 0 goes on, with no element, and writes R = 0)

    // 2. the tile, and the key in front of this wave's quarter
    const uint64_t wbase = base + (uint64_t)wave * WAVE_KEYS;
    K k[ROWS][V];
    if (base + T <= m && (reinterpret_cast<uintptr_t>(keys) & 15u) == 0) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const runs_u32x4 v = *reinterpret_cast<const runs_u32x4*>(keys + wbase + (uint64_t)(j * 64 + (int)lane) * V);
            __builtin_memcpy(k[j], &v, 16);
        }
    } else {  // the last tile, or a base that is aligned to the element only: key by key, in the same places
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const uint64_t idx = wbase + (uint64_t)(j * 64 + (int)lane) * V + v;
                k[j][v] = idx < m ? keys[idx] : K(0);
            }
    }
    K carry = K(0);  // lane 0: the key in front of its row
    if (lane == 0 && wbase > 0 && wbase < m) carry = keys[wbase - 1];

    // 3. heads, as one bit per key, and their scan: lanes of a row, rows of a wave, waves of the tile
    uint32_t heads[ROWS], lane_excl[ROWS];
    uint32_t wave_total = 0;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const K last = k[j][V - 1];
        const K up = shfl_key<K>(last, (int)((lane + 63u) & 63u));
        const K front = lane == 0 ? carry : up;
        carry = shfl_key<K>(last, 63);
        uint32_t h = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint64_t idx = wbase + (uint64_t)(j * 64 + (int)lane) * V + v;
            const K before = v ? k[j][v ? v - 1 : 0] : front;
            if (idx < m && (idx == 0 || k[j][v] != before)) h |= 1u << v;
        }
        heads[j] = h;
        const uint32_t c = (uint32_t)__builtin_popcount(h);
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl += y;
        }
        lane_excl[j] = wave_total + incl - c;
        wave_total += __shfl(incl, 63);
    }
    if (lane == 0) s_wave[wave] = wave_total;
    __syncthreads();
    uint32_t wave_excl = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t c = s_wave[w];
        if ((uint32_t)w < wave) wave_excl += c;
        total += c;
    }

    // 4. publish, look back, publish again
    if (tid == 0) {
        uint64_t excl = 0;
        bool ok = true;
        if (t == 0) {
            st_relaxed<uint64_t>(status, ((uint64_t)ST_INCL << SSHIFT) | total);
        } else {
            st_relaxed<uint64_t>(status + t, ((uint64_t)ST_AGG << SSHIFT) | total);
            ok = runs_lookback(status, t, err, excl);
            if (ok) st_relaxed<uint64_t>(status + t, ((uint64_t)ST_INCL << SSHIFT) | (excl + total));
        }
        s_excl = excl;
        s_fail = ok ? 0u : 1u;
    }
    __syncthreads();
    if (s_fail) return;  // never store with an unknown rank
    const uint64_t tile_excl = s_excl;

    // 5. keys and positions of the heads the capacity has room for; the head of rank == cap closes a truncated table
    if (cap != 0) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            uint64_t r = tile_excl + wave_excl + lane_excl[j];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if ((heads[j] >> v) & 1u) {
                    const uint64_t idx = wbase + (uint64_t)(j * 64 + (int)lane) * V + v;
                    if (out_keys && r < cap) out_keys[r] = k[j][v];
                    if (out_starts && r <= cap) out_starts[r] = (OFF)idx;
                    ++r;
                }
            }
        }
    }

    // 6. the workgroup of element m - 1: the count, the closing border, the truncation
    const uint32_t last_tile = m ? (uint32_t)((m - 1) / T) : 0u;
    if (t == last_tile && tid == 0) {
        const uint64_t runs = tile_excl + total;
        *n_runs = (OFF)runs;
        if (cap != 0) {
            if (runs <= cap) {
                if (out_starts) out_starts[runs] = (OFF)m;
            } else {
                atomicOr(err, ERR_RUNS_TRUNCATED);
            }
        }
    }
}

// RDST_RUNS_PAD_STARTS: starts[r] = m for r in (R, capacity], if the runs fit.  Reads R where runs_kernel left it.
template <typename OFF>
__global__ __launch_bounds__(256) void runs_pad_kernel(OFF* __restrict__ out_starts, const OFF* __restrict__ n_runs, uint64_t capacity, uint64_t len,
                                                       const void* __restrict__ dev_len, uint32_t len_bytes) {
    const uint64_t m = read_length(dev_len, len_bytes, len);
    if (m > len) return;  // (runs_kernel wrote nothing, n_runs least of all)
    const uint64_t runs = (uint64_t)*n_runs;
    if (runs > capacity) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = runs + 1 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= capacity; r += stride) out_starts[r] = (OFF)m;
}

template <typename K, typename OFF>
int runs_launch(const void* keys, uint64_t len, const void* dev_len, uint32_t len_bytes, void* out_keys, void* out_starts, void* n_runs,
                uint64_t out_capacity, void* scratch, uint32_t flags, uint32_t* err, hipStream_t s) {
    const uint64_t tiles = L::tiles(len, (uint32_t)sizeof(K));
    // the library clears the ticket and the status words itself, in stream order
    RDST_HIP_TRY(hipMemsetAsync(scratch, 0, L::scratch_bytes(len, (uint32_t)sizeof(K)), s));
    const uint32_t cap = (uint32_t)std::min<uint64_t>(out_capacity, 0xFFFFFFFFull);
    if (out_capacity == 0) out_keys = out_starts = nullptr;
    int rc = rdst_internal::launch("runs_kernel", runs_kernel<K, OFF>, dim3((uint32_t)tiles), dim3(L::THREADS), 0, s, static_cast<const K*>(keys), len, dev_len,
                                   len_bytes, static_cast<K*>(out_keys), static_cast<OFF*>(out_starts), static_cast<OFF*>(n_runs), cap,
                                   static_cast<uint32_t*>(scratch), reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + L::HEADER_BYTES), err);
    if (rc || !(flags & RDST_RUNS_PAD_STARTS) || out_capacity == 0) return rc;
    const uint64_t blocks = std::min<uint64_t>((out_capacity + 1023) / 1024, 4096);
    return rdst_internal::launch("runs_pad_kernel", runs_pad_kernel<OFF>, dim3((uint32_t)blocks), dim3(256), 0, s, static_cast<OFF*>(out_starts),
                                 static_cast<const OFF*>(n_runs), out_capacity, len, dev_len, len_bytes);
}

template <typename OFF>
int runs_by_width(uint32_t elem_bytes, const void* keys, uint64_t len, const void* dev_len, uint32_t len_bytes, void* out_keys, void* out_starts,
                  void* n_runs, uint64_t out_capacity, void* scratch, uint32_t flags, uint32_t* err, hipStream_t s) {
    switch (elem_bytes) {
        case 1: return runs_launch<uint8_t, OFF>(keys, len, dev_len, len_bytes, out_keys, out_starts, n_runs, out_capacity, scratch, flags, err, s);
        case 2: return runs_launch<uint16_t, OFF>(keys, len, dev_len, len_bytes, out_keys, out_starts, n_runs, out_capacity, scratch, flags, err, s);
        case 4: return runs_launch<uint32_t, OFF>(keys, len, dev_len, len_bytes, out_keys, out_starts, n_runs, out_capacity, scratch, flags, err, s);
        case 8: return runs_launch<uint64_t, OFF>(keys, len, dev_len, len_bytes, out_keys, out_starts, n_runs, out_capacity, scratch, flags, err, s);
        default: return runs_launch<u128, OFF>(keys, len, dev_len, len_bytes, out_keys, out_starts, n_runs, out_capacity, scratch, flags, err, s);
    }
}

}  // namespace

extern "C" int rdst_hip_runs_device(const void* dev_keys, uint64_t len, const void* dev_len, uint32_t len_bytes, void* dev_out_keys, void* dev_out_starts,
                                    void* dev_n_runs, uint32_t offset_bytes, uint64_t out_capacity, void* dev_scratch, uint64_t scratch_bytes,
                                    uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, uint32_t flags, void* stream) {
    int rc = rdst_internal::runs_check_args(dev_keys, len, dev_len, len_bytes, dev_out_keys, dev_out_starts, dev_n_runs, offset_bytes, out_capacity,
                                            dev_scratch, scratch_bytes, elem_bytes, kind, levels, flags);
    if (rc) return rc;
    uint32_t* err = nullptr;
    if ((rc = rdst_internal::device_error_word(&err))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (offset_bytes == 4)
        return runs_by_width<uint32_t>(elem_bytes, dev_keys, len, dev_len, len_bytes, dev_out_keys, dev_out_starts, dev_n_runs, out_capacity, dev_scratch, flags,
                                       err, s);
    return runs_by_width<uint64_t>(elem_bytes, dev_keys, len, dev_len, len_bytes, dev_out_keys, dev_out_starts, dev_n_runs, out_capacity, dev_scratch, flags,
                                   err, s);
}

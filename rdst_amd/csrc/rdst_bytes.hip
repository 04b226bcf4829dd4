// rdst_bytes.hip — [u8; N] keys of any width up to RDST_BYTES_MAX_N on gfx950 (src/radix_key_impl.rs:78-85: level l
// reads byte N-1-l, so rows sort lexicographically).
//
// One core orders the row indices of `n` rows of stride R by the byte string at (off, N) inside each row; the plain
// [u8; N] entries use off = 0, R = N, the records entry its own stride and offset.  It drives the stable (u64, u32) pair
// sort of rdst_kernels.hip through its C entry and adds the kernels below:
//
//   1. prefix    key[i] = big-endian u64 of key bytes [0, 8) (zero past N), val[i] = i; one stable pair sort.
//   2. ties      a scan over the sorted keys marks the rows whose key equals a neighbour's, compacts them, numbers their
//                runs; a second scan over the runs splits them into short and long ones.  Counts go to the host.
//   3. short     runs of 2..BYTES_SMALL rows whose remaining bytes fit a wave's LDS budget: one wave stages them and
//                ranks every row by (remaining bytes, row index) — the device twin of rdst's comparative_sort on small
//                buckets (src/sorts/comparative_sort.rs, src/sorter.rs).
//   4. long      every other run: key = run ordinal in the top b = ceil(log2(runs)) bits, then as many whole next key
//                bytes as fit; val = the row's slot; one stable pair sort; the slots map 1:1 back onto the runs'
//                positions.  Back to 2 on the rows still tied, until none are left or every byte is settled.
//   5. gather    the rows in index order, in the widest unit stride and base alignment allow.
//
// Stability: the prefix sort is stable on row indices, every later sort is stable on positions that are in row order
// within a run, and the comparison kernel breaks ties on the row index — equal keys keep their input order.
//
// bytes_order_nowait is the same order without the host in the loop, for N up to RDST_BYTES_NOWAIT_MAX_N: after step 1 a
// kernel raises a flag on the device if any two prefixes tie, and ceil(N / 8) rounds of (chunk keys, stable pair sort)
// follow whatever it says — with the flag down their keys are all 0 and the pair sorts skip every level.
//
// The second half of the file is the records route for keys described by a field table (rdst_key_field): one kernel
// that packs the mapped key bytes, then the pair sort or the core above, then the same gather.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <type_traits>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_args.h"

namespace {

using rdst_internal::launch;
using rdst_internal::set_error;

constexpr uint32_t ERR_BYTES_RANGE = 8;  // a row index, slot or run read from memory fell out of range: never used to store

constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 16, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;
constexpr int SUMS_THREADS = 1024, SUMS_ITEMS = 4;
constexpr int CMP_WAVES = 4;                 // one run per wave, four waves per workgroup
constexpr uint32_t BYTES_SMALL = 256;        // longest run the comparison kernel takes (four rows per lane)
constexpr uint32_t CMP_WORDS = 3840;         // staging budget per wave in u32 words: 4 x (15 KiB keys + 1 KiB rows) = 64 KiB
constexpr uint32_t GRID_CAP = 256 * 16;      // grid-stride kernels: at most 16 workgroups of 256 per CU

// counters the host reads after the tie step of a round
enum { CNT_TIED = 0, CNT_RUNS = 1, CNT_LONG_ROWS = 2, CNT_LONG_RUNS = 3, CNT_WORDS = 8 };

__device__ __forceinline__ void raise(uint32_t* err, uint32_t bits) { atomicOr(err, bits); }

__device__ __forceinline__ bool run_is_long(uint32_t len, uint32_t words) {
    return len > BYTES_SMALL || (uint64_t)len * words > CMP_WORDS;
}

// key bytes [from, from + k) of the row at p (k <= 8), big-endian, zero past n_bytes
__device__ __forceinline__ uint64_t load_be(const uint8_t* p, uint32_t from, uint32_t k, uint32_t n_bytes) {
    const uint8_t* q = p + from;
    if (k == 8 && from + 8 <= n_bytes) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(q);
        if ((a & 7) == 0) return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(q));
        if ((a & 3) == 0)
            return ((uint64_t)__builtin_bswap32(*reinterpret_cast<const uint32_t*>(q)) << 32) |
                   __builtin_bswap32(*reinterpret_cast<const uint32_t*>(q + 4));
    }
    uint64_t v = 0;
    for (uint32_t t = 0; t < k; ++t) {
        uint32_t b = 0;
        if (from + t < n_bytes) b = q[t];
        v = (v << 8) | b;
    }
    return v;
}

// ---- 1 / 4: pair-sort keys --------------------------------------------------------------------------------------------
// key[j] = (run[j] << (64 - b)) | bytes [depth, depth + k) of row idx[pos[j]] << (64 - b - 8k); val[j] = j.
// pos == nullptr: row j itself (the prefix round, b = 0).
__global__ __launch_bounds__(256) void bytes_keys_kernel(const uint8_t* __restrict__ rows, uint32_t stride, uint32_t off,
                                                         uint32_t n_bytes, uint32_t depth, uint32_t k, uint32_t b,
                                                         const uint32_t* __restrict__ idx, const uint32_t* __restrict__ pos,
                                                         const uint32_t* __restrict__ run, uint64_t m, uint64_t n,
                                                         uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* err) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    const uint32_t low = 64 - b - 8 * k;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += step) {
        uint64_t row = j;
        if (pos) {
            const uint32_t p = pos[j];
            row = p < n ? idx[p] : n;
            if (row >= n) { raise(err, ERR_BYTES_RANGE); keys[j] = 0; vals[j] = (uint32_t)j; continue; }
        }
        uint64_t key = load_be(rows + row * stride + off, depth, k, n_bytes) << low;
        if (b) key |= (uint64_t)run[j] << (64 - b);
        keys[j] = key;
        vals[j] = (uint32_t)j;
    }
}

// ---- 2: scans ---------------------------------------------------------------------------------------------------------
// Reduce-then-scan in three launches over u64 values that pack two counts (low 32 bits, high 32 bits): per-tile sums,
// one workgroup scans the tile sums, each tile rescans itself and emits.  The item count may live on the device (the
// run scan): grids are sized for an upper bound, tiles past the end return.

__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t* s_w, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int i = 0; i < nw; ++i) {
        const uint64_t t = s_w[i];
        if (i < w) before += t;
        all += t;
    }
    __syncthreads();
    total = all;
    return before + x - v;
}

// Tied rows among m sorted keys: tied = equal to a neighbour, head = first of its run.  Value: tied | (tied & head) << 32.
struct TieOp {
    const uint64_t* keys;
    uint64_t m;
    const uint32_t* cpos;  // slot -> position in the index array (nullptr: identity)
    uint32_t* out_pos;     // tied row c -> its position
    uint32_t* out_run;     // tied row c -> its run ordinal
    uint32_t* run_start;   // run r -> its first tied row; run_start[runs] = tied rows
    uint64_t* cnt;
    __device__ uint64_t count() const { return m; }
    __device__ uint64_t value(uint64_t j) const {
        const uint64_t k = keys[j];
        const bool head = j == 0 || keys[j - 1] != k;
        const bool last = j + 1 == m || keys[j + 1] != k;
        const bool tied = !(head && last);
        return (uint64_t)tied | ((uint64_t)(tied && head) << 32);
    }
    __device__ void emit(uint64_t j, uint64_t before, uint64_t v) const {
        if (!(v & 1)) return;
        const uint32_t c = (uint32_t)before, h = (uint32_t)(before >> 32);
        const bool head = (v >> 32) != 0;
        out_pos[c] = cpos ? cpos[j] : (uint32_t)j;
        out_run[c] = head ? h : h - 1;
        if (head) run_start[h] = c;
    }
    __device__ void finish(uint64_t total) const {
        const uint32_t tied = (uint32_t)total, runs = (uint32_t)(total >> 32);
        cnt[CNT_TIED] = tied;
        cnt[CNT_RUNS] = runs;
        run_start[runs] = tied;
    }
};

// Runs that go to the pair sort (long): value = 1 << 32 | length; the exclusive sums give each long run its ordinal and
// the first of its compacted rows.
struct RunOp {
    const uint32_t* run_start;
    uint32_t words;       // u32 words of remaining key bytes per row
    uint64_t* run_scan;   // run r -> exclusive sum
    uint64_t* cnt;
    uint64_t max_runs;    // m / 2: what the tables and the grid are sized for
    __device__ uint64_t count() const { const uint64_t r = cnt[CNT_RUNS]; return r < max_runs ? r : max_runs; }
    __device__ uint64_t value(uint64_t r) const {
        const uint32_t len = run_start[r + 1] - run_start[r];
        return run_is_long(len, words) ? ((1ull << 32) | len) : 0;
    }
    __device__ void emit(uint64_t r, uint64_t before, uint64_t) const { run_scan[r] = before; }
    __device__ void finish(uint64_t total) const {
        cnt[CNT_LONG_ROWS] = (uint32_t)total;
        cnt[CNT_LONG_RUNS] = (uint32_t)(total >> 32);
    }
};

template <typename Op>
__global__ __launch_bounds__(SCAN_THREADS) void scan_tiles_kernel(Op op, uint64_t* __restrict__ tile_sums) {
    __shared__ uint64_t s_w[SCAN_THREADS / 64];
    const uint64_t m = op.count(), base = (uint64_t)blockIdx.x * SCAN_TILE;
    if (base >= m) return;
    const uint64_t first = base + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t sum = 0;
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (first + i < m) sum += op.value(first + i);
    uint64_t total;
    (void)block_exclusive_scan(sum, s_w, total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

template <typename Op>
__global__ __launch_bounds__(SUMS_THREADS) void scan_sums_kernel(Op op, uint64_t* __restrict__ tile_sums) {
    __shared__ uint64_t s_w[SUMS_THREADS / 64];
    const uint64_t m = op.count(), tiles = (m + SCAN_TILE - 1) / SCAN_TILE;
    uint64_t carry = 0;
    for (uint64_t c = 0; c < tiles; c += (uint64_t)SUMS_THREADS * SUMS_ITEMS) {
        const uint64_t first = c + (uint64_t)threadIdx.x * SUMS_ITEMS;
        uint64_t v[SUMS_ITEMS], sum = 0;
        for (int i = 0; i < SUMS_ITEMS; ++i) {
            v[i] = first + i < tiles ? tile_sums[first + i] : 0;
            sum += v[i];
        }
        uint64_t total;
        uint64_t run = carry + block_exclusive_scan(sum, s_w, total);
        for (int i = 0; i < SUMS_ITEMS; ++i) {
            if (first + i < tiles) tile_sums[first + i] = run;
            run += v[i];
        }
        carry += total;
    }
    if (threadIdx.x == 0) op.finish(carry);
}

template <typename Op>
__global__ __launch_bounds__(SCAN_THREADS) void scan_emit_kernel(Op op, const uint64_t* __restrict__ tile_sums) {
    __shared__ uint64_t s_w[SCAN_THREADS / 64];
    const uint64_t m = op.count(), base = (uint64_t)blockIdx.x * SCAN_TILE;
    if (base >= m) return;
    const uint64_t first = base + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t v[SCAN_ITEMS], sum = 0;
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = first + i < m ? op.value(first + i) : 0;
        sum += v[i];
    }
    uint64_t total;
    uint64_t before = tile_sums[blockIdx.x] + block_exclusive_scan(sum, s_w, total);
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        if (first + i < m) op.emit(first + i, before, v[i]);
        before += v[i];
    }
}

// The rows of long runs, compacted in order: long_pos[d] = position, long_run[d] = the run's ordinal among long runs.
__global__ __launch_bounds__(256) void long_rows_kernel(const uint32_t* __restrict__ tied_pos, const uint32_t* __restrict__ tied_run,
                                                        const uint32_t* __restrict__ run_start, const uint64_t* __restrict__ run_scan,
                                                        const uint64_t* __restrict__ cnt, uint32_t words,
                                                        uint32_t* __restrict__ long_pos, uint32_t* __restrict__ long_run, uint32_t* err) {
    const uint64_t tied = cnt[CNT_TIED], runs = cnt[CNT_RUNS], long_rows = cnt[CNT_LONG_ROWS];
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < tied; c += step) {
        const uint32_t r = tied_run[c];
        if (r >= runs) { raise(err, ERR_BYTES_RANGE); continue; }
        const uint32_t s0 = run_start[r], len = run_start[r + 1] - s0;
        if (!run_is_long(len, words)) continue;
        const uint64_t sc = run_scan[r];
        const uint64_t d = (uint32_t)sc + (c - s0);
        if (c < s0 || d >= long_rows) { raise(err, ERR_BYTES_RANGE); continue; }
        long_pos[d] = tied_pos[c];
        long_run[d] = (uint32_t)(sc >> 32);
    }
}

// ---- 3: short runs ----------------------------------------------------------------------------------------------------
// One wave per run: the run's remaining key bytes [depth, n_bytes) as big-endian u32 words (zero-padded) and its row
// indices go to LDS; each lane ranks its rows (at most four) against all others by (bytes, row index) and writes them to
// their places.  The run's positions are contiguous, so rank = offset from the run's first position.
__global__ __launch_bounds__(64 * CMP_WAVES) void short_runs_kernel(const uint8_t* __restrict__ rows, uint32_t stride, uint32_t off,
                                                                     uint32_t n_bytes, uint32_t depth, uint32_t words,
                                                                     const uint32_t* __restrict__ tied_pos, const uint32_t* __restrict__ run_start,
                                                                     const uint64_t* __restrict__ cnt, uint32_t* __restrict__ idx, uint64_t n,
                                                                     uint32_t* err) {
    __shared__ uint32_t s_key[CMP_WAVES][CMP_WORDS];
    __shared__ uint32_t s_row[CMP_WAVES][BYTES_SMALL];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t runs = cnt[CNT_RUNS];
    for (uint64_t base = (uint64_t)blockIdx.x * CMP_WAVES; base < runs; base += (uint64_t)gridDim.x * CMP_WAVES) {
        const uint64_t r = base + w;
        uint32_t len = 0, p0 = 0;
        if (r < runs) {
            const uint32_t s0 = run_start[r];
            len = run_start[r + 1] - s0;
            if (run_is_long(len, words) || len < 2) len = 0;
            else {
                p0 = tied_pos[s0];
                if ((uint64_t)p0 + len > n) { if (lane == 0) raise(err, ERR_BYTES_RANGE); len = 0; }
            }
        }
        bool bad = false;
        for (uint32_t i = lane; i < len; i += 64) {
            const uint32_t row = idx[p0 + i];
            bad |= row >= n;
            s_row[w][i] = row;
        }
        if (__any(bad)) {  // wave-uniform
            if (lane == 0) raise(err, ERR_BYTES_RANGE);
            len = 0;
        }
        __syncthreads();
        for (uint32_t t = lane; t < len * words; t += 64) {
            const uint32_t i = t / words, word = t - i * words;
            const uint8_t* p = rows + (uint64_t)s_row[w][i] * stride + off;
            const uint32_t from = depth + 4 * word;
            uint32_t v = 0;
            for (uint32_t q = 0; q < 4; ++q) {
                uint32_t b = 0;
                if (from + q < n_bytes) b = p[from + q];
                v = (v << 8) | b;
            }
            s_key[w][t] = v;
        }
        __syncthreads();
        uint32_t mine[BYTES_SMALL / 64], rank[BYTES_SMALL / 64];
#pragma unroll
        for (int u = 0; u < (int)(BYTES_SMALL / 64); ++u) {
            const uint32_t i = lane + 64 * u;
            rank[u] = 0;
            mine[u] = 0;
            if (i >= len) continue;
            const uint32_t* ki = &s_key[w][i * words];
            const uint32_t ri = s_row[w][i];
            mine[u] = ri;
            uint32_t less = 0;
            for (uint32_t j = 0; j < len; ++j) {
                if (j == i) continue;
                const uint32_t* kj = &s_key[w][j * words];
                int c = 0;
                for (uint32_t q = 0; q < words && c == 0; ++q) c = kj[q] < ki[q] ? -1 : (kj[q] > ki[q] ? 1 : 0);
                less += c < 0 || (c == 0 && s_row[w][j] < ri);
            }
            rank[u] = less;
        }
#pragma unroll
        for (int u = 0; u < (int)(BYTES_SMALL / 64); ++u)
            if (lane + 64 * u < len) idx[p0 + rank[u]] = mine[u];
        __syncthreads();
    }
}

// ---- 4: back from a pair sort of long-run slots -------------------------------------------------------------------------
// tmp[j] = idx[pos[val[j]]]: the row that sorted to slot j; then idx[pos[j]] = tmp[j].
__global__ __launch_bounds__(256) void slots_gather_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pos,
                                                           const uint32_t* __restrict__ idx, uint64_t m, uint64_t n,
                                                           uint32_t* __restrict__ tmp, uint32_t* err) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += step) {
        const uint32_t v = vals[j];
        const uint32_t p = v < m ? pos[v] : (uint32_t)n;
        if (p >= n) { raise(err, ERR_BYTES_RANGE); tmp[j] = (uint32_t)n; continue; }
        tmp[j] = idx[p];
    }
}
__global__ __launch_bounds__(256) void slots_scatter_kernel(const uint32_t* __restrict__ tmp, const uint32_t* __restrict__ pos,
                                                            uint64_t m, uint64_t n, uint32_t* __restrict__ idx, uint32_t* err) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += step) {
        const uint32_t p = pos[j], row = tmp[j];
        if (p >= n || row >= n) { raise(err, ERR_BYTES_RANGE); continue; }
        idx[p] = row;
    }
}

// ---- nowait rounds (bytes_order_nowait): tie flag, chunk keys ------------------------------------------------------------
// *flag |= 1 if two neighbours among the n sorted prefix keys are equal.  Item j reads keys[j - 1] from memory, so a pair
// that straddles two workgroups or two grid trips is seen like any other.  The caller cleared the word on the stream.
__global__ __launch_bounds__(256) void tie_flag_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint32_t* flag) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    bool tie = false;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; j < n; j += step) tie |= keys[j] == keys[j - 1];
    if (tie) atomicOr(flag, 1u);
}

// key[j] = *flag ? key bytes [from, from + k) of row idx[j], big-endian, left-justified, zero-filled : 0.  idx stays as it
// is: it is the value array of the pair sort that follows.
__global__ __launch_bounds__(256) void chunk_keys_kernel(const uint8_t* __restrict__ rows, uint32_t stride, uint32_t off, uint32_t n_bytes,
                                                         uint32_t from, uint32_t k, const uint32_t* __restrict__ idx,
                                                         const uint32_t* __restrict__ flag, uint64_t n, uint64_t* __restrict__ keys,
                                                         uint32_t* err) {
    const bool up = *flag != 0;
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += step) {
        uint64_t key = 0;
        if (up) {
            const uint32_t row = idx[j];
            if (row >= n) raise(err, ERR_BYTES_RANGE);
            else key = load_be(rows + (uint64_t)row * stride + off, from, k, n_bytes) << (64 - 8 * k);
        }
        keys[j] = key;
    }
}

// ---- 5: gather --------------------------------------------------------------------------------------------------------
struct alignas(16) Unit16 { uint64_t a, b; };
template <typename U>
__global__ __launch_bounds__(256) void rows_gather_kernel(const U* __restrict__ src, U* __restrict__ dst, const uint32_t* __restrict__ idx,
                                                          uint64_t n, uint32_t units, uint32_t* err) {
    const uint64_t total = n * units, step = (uint64_t)gridDim.x * 256;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += step) {
        const uint64_t i = g / units;
        const uint32_t u = (uint32_t)(g - i * units);
        const uint32_t row = idx[i];
        if (row >= n) { if (u == 0) raise(err, ERR_BYTES_RANGE); continue; }
        dst[g] = src[(uint64_t)row * units + u];
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------

using rdst_args::align256;

// Scratch of the core for n rows (n < 2^32): 8 + 8 + 5 x 4 bytes per row, the run tables (at most n / 2 runs) and the
// scan's tile sums.
struct Layout {
    uint64_t keys, keys_tmp, idx, vals_tmp, tied_pos, tied_run, long_pos, run_start, run_scan, tile_sums, cnt, total;
};
Layout make_layout(uint64_t n) {
    Layout L;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { const uint64_t at = o; o += align256(bytes); return at; };
    const uint64_t runs = n / 2 + 2, tiles = (n + SCAN_TILE - 1) / SCAN_TILE + 2;
    L.keys = take(n * 8);
    L.keys_tmp = take(n * 8);
    L.idx = take(n * 4);
    L.vals_tmp = take(n * 4);  // also the long rows' run ordinals between the tie step and the pair sort
    L.tied_pos = take(n * 4);
    L.tied_run = take(n * 4);  // also the pair sort's values in a refinement round
    L.long_pos = take(n * 4);
    L.run_start = take(runs * 4);
    L.run_scan = take(runs * 8);
    L.tile_sums = take(tiles * 8);
    L.cnt = take(CNT_WORDS * 8);
    L.total = o;
    return L;
}

uint32_t grid_for(uint64_t items) {
    uint64_t b = (items + 255) / 256;
    if (b < 1) b = 1;
    return (uint32_t)(b > GRID_CAP ? GRID_CAP : b);
}

// the three-kernel scan of one operator over `tiles` tiles
template <typename Op>
int launch_scan(const Op& op, uint32_t tiles, uint64_t* tile_sums, hipStream_t s) {
    if (int rc = launch("scan_tiles_kernel", scan_tiles_kernel<Op>, dim3(tiles), dim3(SCAN_THREADS), 0, s, op, tile_sums)) return rc;
    if (int rc = launch("scan_sums_kernel", scan_sums_kernel<Op>, dim3(1), dim3(SUMS_THREADS), 0, s, op, tile_sums)) return rc;
    return launch("scan_emit_kernel", scan_emit_kernel<Op>, dim3(tiles), dim3(SCAN_THREADS), 0, s, op, tile_sums);
}

// Orders the row indices (left in the scratch's idx array).  Blocking: one wait per round.
int bytes_order(const uint8_t* rows, uint64_t n, uint32_t stride, uint32_t off, uint32_t n_bytes, char* scratch,
                hipStream_t s, uint32_t* err) {
    const Layout L = make_layout(n);
    uint64_t* keys = reinterpret_cast<uint64_t*>(scratch + L.keys);
    uint64_t* keys_tmp = reinterpret_cast<uint64_t*>(scratch + L.keys_tmp);
    uint32_t* idx = reinterpret_cast<uint32_t*>(scratch + L.idx);
    uint32_t* vals_tmp = reinterpret_cast<uint32_t*>(scratch + L.vals_tmp);
    uint32_t* tied_pos = reinterpret_cast<uint32_t*>(scratch + L.tied_pos);
    uint32_t* tied_run = reinterpret_cast<uint32_t*>(scratch + L.tied_run);
    uint32_t* long_pos = reinterpret_cast<uint32_t*>(scratch + L.long_pos);
    uint32_t* long_run = vals_tmp;
    uint32_t* run_start = reinterpret_cast<uint32_t*>(scratch + L.run_start);
    uint64_t* run_scan = reinterpret_cast<uint64_t*>(scratch + L.run_scan);
    uint64_t* tile_sums = reinterpret_cast<uint64_t*>(scratch + L.tile_sums);
    uint64_t* cnt = reinterpret_cast<uint64_t*>(scratch + L.cnt);

    // 1. prefix
    const uint32_t k0 = n_bytes < 8 ? n_bytes : 8;
    int rc = launch("bytes_keys_kernel", bytes_keys_kernel, dim3(grid_for(n)), dim3(256), 0, s, rows, stride, off, n_bytes, 0u, k0, 0u, nullptr, nullptr,
                    nullptr, n, n, keys, idx, err);
    if (rc) return rc;
    if ((rc = rdst_hip_sort_pairs_device(keys, idx, keys_tmp, vals_tmp, n, 8, RDST_KEY_UNSIGNED, 8, 4, s))) return rc;

    uint32_t depth = k0;
    uint64_t m = n;
    const uint32_t* cpos = nullptr;
    while (depth < n_bytes) {
        const uint32_t words = (n_bytes - depth + 3) / 4;
        // 2. ties, then the runs' split into short and long
        const TieOp tie{keys, m, cpos, tied_pos, tied_run, run_start, cnt};
        if ((rc = launch_scan(tie, (uint32_t)((m + SCAN_TILE - 1) / SCAN_TILE), tile_sums, s))) return rc;
        const RunOp runop{run_start, words, run_scan, cnt, m / 2};
        if ((rc = launch_scan(runop, (uint32_t)((m / 2 + SCAN_TILE) / SCAN_TILE), tile_sums, s))) return rc;  // at most m / 2 runs
        if ((rc = launch("long_rows_kernel", long_rows_kernel, dim3(grid_for(m)), dim3(256), 0, s, tied_pos, tied_run, run_start, run_scan, cnt, words, long_pos,
                         long_run, err)))
            return rc;
        uint64_t h[4] = {0, 0, 0, 0};
        RDST_HIP_TRY(hipMemcpyAsync(h, cnt, sizeof h, hipMemcpyDeviceToHost, s));
        RDST_HIP_TRY(hipStreamSynchronize(s));
        const uint64_t tied = h[CNT_TIED], runs = h[CNT_RUNS], long_rows = h[CNT_LONG_ROWS], long_runs = h[CNT_LONG_RUNS];
        if (tied > m || 2 * runs > tied || long_rows > tied || long_runs > runs || (long_runs == 0) != (long_rows == 0))
            return set_error(RDST_ERR_DEVICE, "[u8; N] route: inconsistent tie counts (a kernel before them failed)");
        if (runs == 0) break;
        // 3. short runs
        if (runs > long_runs) {
            uint64_t blocks = (runs + CMP_WAVES - 1) / CMP_WAVES;
            if (blocks > (1u << 20)) blocks = 1u << 20;
            if ((rc = launch("short_runs_kernel", short_runs_kernel, dim3((uint32_t)blocks), dim3(64 * CMP_WAVES), 0, s, rows, stride, off, n_bytes, depth, words,
                             tied_pos, run_start, cnt, idx, n, err)))
                return rc;
        }
        if (long_runs == 0) break;
        // 4. long runs: (run ordinal, next bytes) pairs, one stable pair sort, slots back to positions
        const uint32_t b = long_runs == 1 ? 0 : 64 - __builtin_clzll(long_runs - 1);
        const uint32_t k = (64 - b) / 8;
        if ((rc = launch("bytes_keys_kernel", bytes_keys_kernel, dim3(grid_for(long_rows)), dim3(256), 0, s, rows, stride, off, n_bytes, depth, k, b, idx, long_pos,
                         long_run, long_rows, n, keys, tied_run, err)))
            return rc;
        if ((rc = rdst_hip_sort_pairs_device(keys, tied_run, keys_tmp, vals_tmp, long_rows, 8, RDST_KEY_UNSIGNED, 8, 4, s))) return rc;
        if ((rc = launch("slots_gather_kernel", slots_gather_kernel, dim3(grid_for(long_rows)), dim3(256), 0, s, tied_run, long_pos, idx, long_rows, n, vals_tmp, err)))
            return rc;
        if ((rc = launch("slots_scatter_kernel", slots_scatter_kernel, dim3(grid_for(long_rows)), dim3(256), 0, s, vals_tmp, long_pos, long_rows, n, idx, err)))
            return rc;
        depth += k;
        m = long_rows;
        cpos = long_pos;
    }
    return RDST_OK;
}

// The same order without the host in the loop (n_bytes <= RDST_BYTES_NOWAIT_MAX_N): every launch is fixed by n and n_bytes
// alone.  After the prefix sort one kernel raises a flag word if any two prefixes tie; then ceil(n_bytes / 8) rounds, last
// chunk first, each a chunk-key kernel and a stable pair sort of (chunk, row).  Flag down: every key is 0, the pair sorts
// skip all their levels and idx stays as the prefix sort left it.  Flag up: an LSD sort over all chunks on top of the prefix
// order; rows equal in every byte have equal prefixes, so they are in row order already and every later sort keeps them so.
// Uses keys, keys_tmp, idx, vals_tmp and the first word of cnt.
int bytes_order_nowait(const uint8_t* rows, uint64_t n, uint32_t stride, uint32_t off, uint32_t n_bytes, char* scratch,
                       hipStream_t s, uint32_t* err) {
    const Layout L = make_layout(n);
    uint64_t* keys = reinterpret_cast<uint64_t*>(scratch + L.keys);
    uint64_t* keys_tmp = reinterpret_cast<uint64_t*>(scratch + L.keys_tmp);
    uint32_t* idx = reinterpret_cast<uint32_t*>(scratch + L.idx);
    uint32_t* vals_tmp = reinterpret_cast<uint32_t*>(scratch + L.vals_tmp);
    uint32_t* flag = reinterpret_cast<uint32_t*>(scratch + L.cnt);

    RDST_HIP_TRY(hipMemsetAsync(flag, 0, sizeof(uint32_t), s));
    const uint32_t k0 = n_bytes < 8 ? n_bytes : 8;
    int rc = launch("bytes_keys_kernel", bytes_keys_kernel, dim3(grid_for(n)), dim3(256), 0, s, rows, stride, off, n_bytes, 0u, k0, 0u, nullptr, nullptr,
                    nullptr, n, n, keys, idx, err);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());  // once, around all the pair sorts
    if ((rc = rdst_internal::sort_pairs_slice_locked(keys, idx, keys_tmp, vals_tmp, n, 8, RDST_KEY_UNSIGNED, 4, s))) return rc;
    if ((rc = launch("tie_flag_kernel", tie_flag_kernel, dim3(grid_for(n)), dim3(256), 0, s, keys, n, flag))) return rc;
    for (uint32_t c = (n_bytes + 7) / 8; c-- > 0;) {
        const uint32_t from = 8 * c, k = n_bytes - from < 8 ? n_bytes - from : 8;
        if ((rc = launch("chunk_keys_kernel", chunk_keys_kernel, dim3(grid_for(n)), dim3(256), 0, s, rows, stride, off, n_bytes, from, k, idx, flag, n, keys, err)))
            return rc;
        if ((rc = rdst_internal::sort_pairs_slice_locked(keys, idx, keys_tmp, vals_tmp, n, 8, RDST_KEY_UNSIGNED, 4, s))) return rc;
    }
    return RDST_OK;
}

int bytes_gather(const uint8_t* src, uint8_t* dst, const uint32_t* idx, uint64_t n, uint32_t stride, hipStream_t s, uint32_t* err) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | stride;
    const uint32_t unit = a % 16 == 0 ? 16 : (a % 8 == 0 ? 8 : (a % 4 == 0 ? 4 : 1));
    const uint32_t units = stride / unit;
    uint64_t blocks = (n * units + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    auto gather = [&](auto u) {
        using U = decltype(u);
        return launch("rows_gather_kernel", rows_gather_kernel<U>, dim3((uint32_t)blocks), dim3(256), 0, s, reinterpret_cast<const U*>(src),
                      reinterpret_cast<U*>(dst), idx, n, units, err);
    };
    return unit == 16 ? gather(Unit16{}) : (unit == 8 ? gather(uint64_t{}) : (unit == 4 ? gather(uint32_t{}) : gather(uint8_t{})));
}

uint64_t core_scratch_bytes(uint64_t n) { return make_layout(n).total; }

}  // namespace

namespace rdst_internal {

int sort_bytes_rows_host(void* host_rows, uint64_t len, uint32_t row_bytes, uint32_t key_offset, uint32_t key_bytes,
                         const rdst_hip_opts* opts) {
    HostJob job;
    uint32_t* err = nullptr;
    int rc;
    if ((rc = job.enter(opts)) || (rc = device_error_word(&err)) || (rc = job.open())) return rc;
    const uint64_t bytes = len * row_bytes;
    void *d_rows = nullptr, *d_out = nullptr, *d_scratch = nullptr;
    RDST_HIP_TRY(job.alloc(&d_rows, bytes));
    RDST_HIP_TRY(job.alloc(&d_out, bytes));
    RDST_HIP_TRY(job.alloc(&d_scratch, core_scratch_bytes(len)));
    if ((rc = job.upload(d_rows, host_rows, bytes))) return rc;
    const uint8_t* rows = static_cast<const uint8_t*>(d_rows);
    char* scratch = static_cast<char*>(d_scratch);
    rc = bytes_order(rows, len, row_bytes, key_offset, key_bytes, scratch, job.s, err);
    if (rc == RDST_OK)
        rc = bytes_gather(rows, static_cast<uint8_t*>(d_out), reinterpret_cast<const uint32_t*>(scratch + make_layout(len).idx), len,
                          row_bytes, job.s, err);
    return job.finish(rc, host_rows, d_out, bytes);
}

}  // namespace rdst_internal

namespace {
// Both device entries for [u8; N] rows; `max_n` and `order` are what tells them apart.
int sort_bytes_device(void* dev_rows, uint64_t len, uint32_t n_bytes, void* dev_scratch, uint64_t scratch_bytes, void* stream, uint32_t max_n,
                      const char* too_wide, decltype(bytes_order)* order) {
    if (n_bytes == 0) return set_error(RDST_ERR_ARG, "[u8; N] needs N >= 1 (RadixKey::LEVELS == 0 panics in rdst)");
    if (n_bytes > max_n) return set_error(RDST_ERR_UNSUPPORTED, too_wide);
    if (len <= 1) return RDST_OK;  // radix_sort_builder.rs:151
    if (dev_rows == nullptr) return set_error(RDST_ERR_ARG, "null rows pointer");
    if (n_bytes > 16 && len >= (1ull << 32)) return set_error(RDST_ERR_UNSUPPORTED, "[u8; N] keys with N > 16 are built for len < 2^32");
    if (dev_scratch == nullptr) return set_error(RDST_ERR_ARG, "null scratch pointer");
    if (scratch_bytes < rdst_hip_sort_bytes_scratch_bytes(len, n_bytes))
        return set_error(RDST_ERR_ARG, "scratch smaller than rdst_hip_sort_bytes_scratch_bytes(len, n_bytes)");
    if (reinterpret_cast<uintptr_t>(dev_scratch) % 256) return set_error(RDST_ERR_ALIGN, "scratch not 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_bytes <= 16) return rdst_internal::sort_bytes_widened(dev_rows, len, n_bytes, dev_scratch, s);
    uint32_t* err = nullptr;
    int rc = rdst_internal::device_error_word(&err);
    if (rc) return rc;
    char* scratch = static_cast<char*>(dev_scratch);
    const Layout L = make_layout(len);
    uint8_t* rows = static_cast<uint8_t*>(dev_rows);
    uint8_t* staged = reinterpret_cast<uint8_t*>(scratch + L.total);
    rc = order(rows, len, n_bytes, 0, n_bytes, scratch, s, err);
    if (rc) return rc;
    rc = bytes_gather(rows, staged, reinterpret_cast<const uint32_t*>(scratch + L.idx), len, n_bytes, s, err);
    if (rc) return rc;
    RDST_HIP_TRY(hipMemcpyAsync(rows, staged, len * n_bytes, hipMemcpyDeviceToDevice, s));
    return RDST_OK;
}
}  // namespace

extern "C" {

uint64_t rdst_hip_sort_bytes_scratch_bytes(uint64_t len, uint32_t n_bytes) {
    if (n_bytes == 0 || n_bytes > RDST_BYTES_MAX_N) return 0;
    if (n_bytes <= 16) return rdst_internal::widened_scratch_bytes(len, n_bytes);
    return core_scratch_bytes(len) + align256(len * n_bytes);
}

int rdst_hip_sort_bytes_device(void* dev_rows, uint64_t len, uint32_t n_bytes, void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_bytes_device(dev_rows, len, n_bytes, dev_scratch, scratch_bytes, stream, RDST_BYTES_MAX_N,
                             "[u8; N] keys are built for N in 1..RDST_BYTES_MAX_N", bytes_order);
}

int rdst_hip_sort_bytes_device_nowait(void* dev_rows, uint64_t len, uint32_t n_bytes, void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_bytes_device(dev_rows, len, n_bytes, dev_scratch, scratch_bytes, stream, RDST_BYTES_NOWAIT_MAX_N,
                             "the nowait [u8; N] entry is built for N in 1..RDST_BYTES_NOWAIT_MAX_N; wider keys take rdst_hip_sort_bytes_device",
                             bytes_order_nowait);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------------
// Records ordered by a described key: rdst_key_field tables (include/rdst_hip.h)
// ------------------------------------------------------------------------------------------------------------------------
// The description states a RadixKey with LEVELS = L = sum of the fields' widths and get_level(l) = K[L - 1 - l], K the
// concatenation of the fields' mapped values, big-endian (src/radix_key.rs; examples/impl_radix_key.rs:32-56).
// pack_fields_kernel turns records into K; everything after it is the code above: L <= 8 is one stable (key, row) pair
// sort, L > 8 hands dense [u8; L] rows to bytes_order; bytes_gather moves the records.

namespace {

constexpr uint32_t PACK_TILE = 256;         // records per workgroup trip: four waves of 64 consecutive records
constexpr uint32_t PACK_LDS_BYTES = 32768;  // a tile of records up to this size is staged through LDS

struct FieldTable {  // travels by value in the kernel arguments
    rdst_key_field f[RDST_KEY_FIELDS_MAX];
    uint32_t n;
};

// byte j (0 = most significant) of a field's mapped value: integers and floats are stored little-endian, byte strings as
// they are; signed: ^ MIN; float: negative -> every bit flipped, else ^ MIN (src/radix_key_impl.rs:162-185); descending:
// every bit flipped
__device__ __forceinline__ uint32_t field_flip(const uint8_t* rec, const rdst_key_field& f, uint32_t& top) {
    uint32_t all = (f.flags & RDST_FIELD_DESCENDING) ? 0xFFu : 0u;
    top = 0;
    if (f.kind == RDST_KEY_SIGNED) top = 0x80u;
    else if (f.kind == RDST_KEY_FLOAT) {
        if (rec[f.offset + f.bytes - 1] & 0x80u) all ^= 0xFFu;
        else top = 0x80u;
    }
    return all;
}
__device__ __forceinline__ uint32_t field_byte(const uint8_t* rec, const rdst_key_field& f, uint32_t j, uint32_t all, uint32_t top) {
    const uint32_t src = f.kind == RDST_KEY_BYTES_BE ? f.offset + j : f.offset + f.bytes - 1 - j;
    return rec[src] ^ all ^ (j == 0 ? top : 0u);
}

// MODE 0: u32 key (L <= 4), 1: u64 key (L <= 8), both left-justified and zero-filled, plus the row index; 2: dense
// [u8; L] rows (out must be 4-byte aligned).  STAGED: the tile's records, one contiguous span, come to LDS in 16-byte
// coalesced loads (bytes before the span's first and after its last are never read) and the fields are picked out of
// LDS; otherwise (a tile beyond PACK_LDS_BYTES) the field bytes are read from memory directly.
template <int MODE, bool STAGED>
__global__ __launch_bounds__(256) void pack_fields_kernel(const uint8_t* __restrict__ rows, uint64_t n, uint32_t R, FieldTable d,
                                                          void* __restrict__ out, uint32_t* __restrict__ idx) {
    __shared__ rdst_key_field s_f[RDST_KEY_FIELDS_MAX];
    __shared__ uint4 s_tile[STAGED ? PACK_LDS_BYTES / 16 + 1 : 1];
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t k = 0; k < RDST_KEY_FIELDS_MAX; ++k) s_f[k] = d.f[k];
    }
    __syncthreads();
    const uint32_t nf = d.n, tid = threadIdx.x;
    uint32_t L = 0;
    for (uint32_t k = 0; k < nf; ++k) L += s_f[k].bytes;
    const uint64_t tiles = (n + PACK_TILE - 1) / PACK_TILE;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t first = t * PACK_TILE;
        const uint32_t cnt = n - first < PACK_TILE ? (uint32_t)(n - first) : PACK_TILE;
        const uint8_t* base = rows + first * R;  // the tile's first record
        if constexpr (STAGED) {
            const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15);
            const uint8_t* g0 = base - mis;      // 16-byte aligned; [mis, span) is the tile
            const uint32_t span = mis + cnt * R;
            uint8_t* lds = reinterpret_cast<uint8_t*>(s_tile);
            for (uint32_t c = tid * 16; c < span; c += 256 * 16) {
                if (c >= mis && c + 16 <= span) s_tile[c / 16] = *reinterpret_cast<const uint4*>(g0 + c);
                else
                    for (uint32_t q = c < mis ? mis : c; q < c + 16 && q < span; ++q) lds[q] = g0[q];
            }
            __syncthreads();
            base = lds + mis;
        }
        if constexpr (MODE == 2) {
            const uint32_t total = cnt * L;  // at most 256 x 4096 bytes
            uint8_t* o = static_cast<uint8_t*>(out) + first * L;
            for (uint32_t b0 = tid * 4; b0 < total; b0 += 256 * 4) {
                const uint32_t nb = total - b0 < 4 ? total - b0 : 4;
                uint32_t r = b0 / L, p = b0 - r * L, k = 0, at = 0, word = 0;
                while (p >= at + s_f[k].bytes) at += s_f[k++].bytes;  // p < L: ends inside the table
                for (uint32_t q = 0; q < nb; ++q) {
                    const uint8_t* rec = base + (size_t)r * R;
                    uint32_t top;
                    const uint32_t all = field_flip(rec, s_f[k], top);
                    word |= field_byte(rec, s_f[k], p - at, all, top) << (8 * q);
                    if (++p == at + s_f[k].bytes) at += s_f[k++].bytes;
                    if (p == L) { p = 0; k = 0; at = 0; ++r; }
                }
                if (nb == 4) *reinterpret_cast<uint32_t*>(o + b0) = word;
                else
                    for (uint32_t q = 0; q < nb; ++q) o[b0 + q] = (uint8_t)(word >> (8 * q));
            }
        } else if (tid < cnt) {
            using KT = typename std::conditional<MODE == 0, uint32_t, uint64_t>::type;
            const uint8_t* rec = base + (size_t)tid * R;
            uint64_t key = 0;
            for (uint32_t k = 0; k < nf; ++k) {
                const rdst_key_field f = s_f[k];
                uint32_t top;
                const uint32_t all = field_flip(rec, f, top);
                for (uint32_t j = 0; j < f.bytes; ++j) key = (key << 8) | field_byte(rec, f, j, all, top);
            }
            static_cast<KT*>(out)[first + tid] = (KT)(key << (8 * (sizeof(KT) - L)));
            idx[first + tid] = (uint32_t)(first + tid);
        }
        if constexpr (STAGED) __syncthreads();  // the next trip overwrites the tile
    }
}

// The description's rules (rdst_hip.h); *L_out = the key's length in bytes.
// `max_L`: the longest key the calling entry takes.
int check_fields(uint32_t record_bytes, const rdst_key_field* fields, uint32_t n_fields, uint32_t* L_out, uint32_t max_L = RDST_BYTES_MAX_N) {
    if (n_fields == 0) return set_error(RDST_ERR_ARG, "a key needs at least one field (RadixKey::LEVELS == 0 panics in rdst)");
    if (n_fields > RDST_KEY_FIELDS_MAX) return set_error(RDST_ERR_UNSUPPORTED, "key descriptions are built for at most RDST_KEY_FIELDS_MAX fields");
    if (fields == nullptr) return set_error(RDST_ERR_ARG, "null field table");
    uint64_t L = 0;
    for (uint32_t k = 0; k < n_fields; ++k) {
        const rdst_key_field& f = fields[k];
        if (f.kind > RDST_KEY_BYTES_BE) return set_error(RDST_ERR_ARG, "unknown key kind in a key field");
        if (f.flags & ~RDST_FIELD_DESCENDING) return set_error(RDST_ERR_ARG, "unknown flag bit in a key field");
        const uint32_t b = f.bytes;
        const bool pow2 = b == 1 || b == 2 || b == 4 || b == 8 || b == 16;
        const bool ok = f.kind == RDST_KEY_BYTES_BE ? (b >= 1 && b <= RDST_BYTES_MAX_N) : (f.kind == RDST_KEY_FLOAT ? (b == 4 || b == 8) : pow2);
        if (!ok)
            return set_error(RDST_ERR_UNSUPPORTED, "key field width not built for its kind (integers: 1, 2, 4, 8, 16; floats: 4, 8; byte strings: 1..RDST_BYTES_MAX_N)");
        if ((uint64_t)f.offset + b > record_bytes) return set_error(RDST_ERR_ARG, "key field outside the record");
        L += b;
    }
    if (L > RDST_BYTES_MAX_N) return set_error(RDST_ERR_UNSUPPORTED, "described keys are built for at most RDST_BYTES_MAX_N bytes in all");
    if (L > max_L)
        return set_error(RDST_ERR_UNSUPPORTED, "the nowait entry is built for described keys of at most RDST_BYTES_NOWAIT_MAX_N bytes in all; longer keys take rdst_hip_sort_records_by_fields_device");
    *L_out = (uint32_t)L;
    return RDST_OK;
}

// Scratch of the records route: the key / index arrays (L <= 8) or the order core's arrays and the packed keys (L > 8),
// then the staging copy of the rows.
struct FieldsLayout {
    uint64_t keys, keys_tmp, idx, idx_tmp, packed, staged, total;
};
FieldsLayout make_fields_layout(uint64_t n, uint32_t R, uint32_t L) {
    FieldsLayout F{};
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { const uint64_t at = o; o += align256(bytes); return at; };
    if (L <= 8) {
        const uint32_t kb = L <= 4 ? 4 : 8;
        F.keys = take(n * kb);
        F.keys_tmp = take(n * kb);
        F.idx = take(n * 4);
        F.idx_tmp = take(n * 4);
    } else {
        const Layout C = make_layout(n);
        F.idx = C.idx;
        (void)take(C.total);
        F.packed = take(n * L);
    }
    F.staged = take(n * R);
    F.total = o;
    return F;
}

int launch_pack(const uint8_t* rows, uint64_t n, uint32_t R, const FieldTable& d, uint32_t L, void* out, uint32_t* idx, hipStream_t s) {
    uint64_t blocks = (n + PACK_TILE - 1) / PACK_TILE;
    if (blocks > GRID_CAP) blocks = GRID_CAP;
    const bool staged = (uint64_t)PACK_TILE * R <= PACK_LDS_BYTES;
    auto go = [&](auto kernel) { return launch("pack_fields_kernel", kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rows, n, R, d, out, idx); };
    if (L <= 4) return staged ? go(pack_fields_kernel<0, true>) : go(pack_fields_kernel<0, false>);
    if (L <= 8) return staged ? go(pack_fields_kernel<1, true>) : go(pack_fields_kernel<1, false>);
    return staged ? go(pack_fields_kernel<2, true>) : go(pack_fields_kernel<2, false>);
}

FieldTable make_table(const rdst_key_field* fields, uint32_t n_fields) {
    FieldTable d{};
    for (uint32_t k = 0; k < n_fields; ++k) d.f[k] = fields[k];
    d.n = n_fields;
    return d;
}

// Packs, orders and gathers into the scratch's staging area; `rows` is only read.  Asynchronous for L <= 8, and for every
// L with `nowait` (bytes_order_nowait in place of bytes_order).
int fields_sort_staged(const uint8_t* rows, uint64_t n, uint32_t R, const rdst_key_field* fields, uint32_t n_fields, uint32_t L,
                       char* scratch, hipStream_t s, uint32_t* err, bool nowait = false) {
    const FieldsLayout F = make_fields_layout(n, R, L);
    const FieldTable d = make_table(fields, n_fields);
    uint32_t* idx = reinterpret_cast<uint32_t*>(scratch + F.idx);
    int rc;
    if (L <= 8) {
        const uint32_t kb = L <= 4 ? 4 : 8;
        if ((rc = launch_pack(rows, n, R, d, L, scratch + F.keys, idx, s))) return rc;
        if ((rc = rdst_hip_sort_pairs_device(scratch + F.keys, idx, scratch + F.keys_tmp, scratch + F.idx_tmp, n, kb, RDST_KEY_UNSIGNED, kb, 4, s))) return rc;
    } else {
        uint8_t* packed = reinterpret_cast<uint8_t*>(scratch + F.packed);
        if ((rc = launch_pack(rows, n, R, d, L, packed, nullptr, s))) return rc;
        if ((rc = (nowait ? bytes_order_nowait : bytes_order)(packed, n, L, 0, L, scratch, s, err))) return rc;
    }
    return bytes_gather(rows, reinterpret_cast<uint8_t*>(scratch + F.staged), idx, n, R, s, err);
}


// Both device entries for records with a described key; `max_L` and `nowait` are what tells them apart.
int sort_records_by_fields_device(void* dev_records, uint64_t len, uint32_t record_bytes, const rdst_key_field* fields, uint32_t n_fields,
                                  void* dev_scratch, uint64_t scratch_bytes, void* stream, uint32_t max_L, bool nowait) {
    uint32_t L = 0;
    int rc = check_fields(record_bytes, fields, n_fields, &L, max_L);
    if (rc) return rc;
    if (len <= 1) return RDST_OK;  // radix_sort_builder.rs:151
    if (dev_records == nullptr) return set_error(RDST_ERR_ARG, "null record pointer");
    if (len >= (1ull << 32)) return set_error(RDST_ERR_UNSUPPORTED, "records with a described key are built for len < 2^32 (row indices are u32)");
    if (dev_scratch == nullptr) return set_error(RDST_ERR_ARG, "null scratch pointer");
    const FieldsLayout F = make_fields_layout(len, record_bytes, L);
    if (scratch_bytes < F.total) return set_error(RDST_ERR_ARG, "scratch smaller than rdst_hip_sort_records_by_fields_scratch_bytes(...)");
    if (reinterpret_cast<uintptr_t>(dev_scratch) % 256) return set_error(RDST_ERR_ALIGN, "scratch not 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* err = nullptr;
    if ((rc = rdst_internal::device_error_word(&err))) return rc;
    char* scratch = static_cast<char*>(dev_scratch);
    if ((rc = fields_sort_staged(static_cast<const uint8_t*>(dev_records), len, record_bytes, fields, n_fields, L, scratch, s, err, nowait))) return rc;
    RDST_HIP_TRY(hipMemcpyAsync(dev_records, scratch + F.staged, len * record_bytes, hipMemcpyDeviceToDevice, s));
    return RDST_OK;
}

}  // namespace

extern "C" {

uint64_t rdst_hip_sort_records_by_fields_scratch_bytes(uint64_t len, uint32_t record_bytes, const rdst_key_field* fields, uint32_t n_fields) {
    uint32_t L = 0;
    if (check_fields(record_bytes, fields, n_fields, &L)) return 0;
    return make_fields_layout(len, record_bytes, L).total;
}

int rdst_hip_sort_records_by_fields_device(void* dev_records, uint64_t len, uint32_t record_bytes, const rdst_key_field* fields,
                                           uint32_t n_fields, void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_records_by_fields_device(dev_records, len, record_bytes, fields, n_fields, dev_scratch, scratch_bytes, stream, RDST_BYTES_MAX_N, false);
}

int rdst_hip_sort_records_by_fields_device_nowait(void* dev_records, uint64_t len, uint32_t record_bytes, const rdst_key_field* fields,
                                                  uint32_t n_fields, void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_records_by_fields_device(dev_records, len, record_bytes, fields, n_fields, dev_scratch, scratch_bytes, stream,
                                         RDST_BYTES_NOWAIT_MAX_N, true);
}

int rdst_hip_sort_records_by_fields(void* host_records, uint64_t len, uint32_t record_bytes, const rdst_key_field* fields, uint32_t n_fields,
                                    const rdst_hip_opts* opts) {
    uint32_t L = 0;
    int rc = check_fields(record_bytes, fields, n_fields, &L);
    if (rc) return rc;
    if (len <= 1) return RDST_OK;
    if (host_records == nullptr) return set_error(RDST_ERR_ARG, "null record pointer");
    if (len >= (1ull << 32)) return set_error(RDST_ERR_UNSUPPORTED, "records with a described key are built for len < 2^32 (row indices are u32)");
    rdst_internal::HostJob job;
    uint32_t* err = nullptr;
    if ((rc = job.enter(opts)) || (rc = rdst_internal::device_error_word(&err)) || (rc = job.open())) return rc;
    const uint64_t bytes = len * record_bytes;
    const FieldsLayout F = make_fields_layout(len, record_bytes, L);
    void *d_rows = nullptr, *d_scratch = nullptr;
    RDST_HIP_TRY(job.alloc(&d_rows, bytes));
    RDST_HIP_TRY(job.alloc(&d_scratch, F.total));
    if ((rc = job.upload(d_rows, host_records, bytes))) return rc;
    char* scratch = static_cast<char*>(d_scratch);
    rc = fields_sort_staged(static_cast<const uint8_t*>(d_rows), len, record_bytes, fields, n_fields, L, scratch, job.s, err);
    return job.finish(rc, host_records, scratch + F.staged, bytes);  // straight from the staging area
}

int rdst_hip_pack_fields_device(const void* dev_records, uint64_t len, uint32_t record_bytes, const rdst_key_field* fields, uint32_t n_fields,
                                void* dev_keys, uint32_t* dev_rows, void* stream) {
    uint32_t L = 0;
    int rc = check_fields(record_bytes, fields, n_fields, &L);
    if (rc) return rc;
    if (len == 0) return RDST_OK;
    if (dev_records == nullptr || dev_keys == nullptr || (L <= 8 && dev_rows == nullptr)) return set_error(RDST_ERR_ARG, "null pointer");
    if (len >= (1ull << 32)) return set_error(RDST_ERR_UNSUPPORTED, "records with a described key are built for len < 2^32 (row indices are u32)");
    if (reinterpret_cast<uintptr_t>(dev_keys) % (L <= 4 || L > 8 ? 4 : 8) || reinterpret_cast<uintptr_t>(dev_rows) % 4)
        return set_error(RDST_ERR_ALIGN, "key or row output not aligned");
    return launch_pack(static_cast<const uint8_t*>(dev_records), len, record_bytes, make_table(fields, n_fields), L, dev_keys, dev_rows,
                       static_cast<hipStream_t>(stream));
}

}  // extern "C"

// The sampling metrics' device side: an ascending sort of a bag of binary32 / binary64 values and the two-sample
// Kolmogorov-Smirnov numerator of two sorted bags -- what the reference leaves to scipy.stats.ks_2samp on host copies
// (metrics/kolmogorov_smirnov_metrics.py:42-75).  See include/mdx_hip.h (mdx_sort_keys, mdx_ks_two_sample_sorted) for the contract.
//
// mdx_sort_keys: a least-significant-digit radix sort on 8-bit digits of an orderable unsigned image of each value IN THE
// INPUT'S OWN WIDTH (4 passes for binary32, 8 for binary64).  A pass is three launches over tiles of kTile keys:
//   digit_histogram_kernel   one workgroup per tile: the tile's 256 digit counts (LDS integer atomics), written [digit][tile]
//   tile_scan_kernel         one workgroup per digit: the exclusive scan of that digit's row over the tiles, and the row total
//   scatter_kernel           one workgroup per tile: digit base = exclusive scan of the 256 totals; a key's place = digit base +
//                            its tile's scanned count + its rank among the tile's keys of that digit.  The rank is STABLE: the
//                            tile is walked in index order (wavefront, round, lane), equal digits of a round are matched by
//                            eight ballots and ranked by lane, rounds add up in a per-wavefront LDS counter, and the wavefronts
//                            are prefixed in index order.
// The first pass reads the caller's values and maps them to keys on the fly (the input is never written), the last writes the
// keys back as binary64; in between the keys ping-pong between the workspace and the output buffer.  A stable keys-only sort
// has one correct output: the same bits on every launch.  No float arithmetic, no float atomics.
//
// mdx_ks_two_sample_sorted: one thread per element x of either bag: c_a(x), c_b(x) by binary search for the upper bound, the
// integer |c_a n2/g - c_b n1/g|, maxima by wavefront butterfly and workgroup, then one small workgroup over the block maxima.
// 64-wide wavefronts are assumed (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"

using namespace mdx;

namespace {

constexpr int kWaves = kBlock / kWave;
constexpr int kItems = 8;                        // keys per thread
constexpr int kTile = kBlock * kItems;           // keys per workgroup: MDX_KS_SORT_TILE
constexpr int kDigits = 256;
constexpr int kDigitBits = 8;
constexpr int kMaxRankBlocks = 2048;             // flat_grid's cap: the block maxima of the rank kernel
static_assert(kTile == MDX_KS_SORT_TILE, "the header states the tile");
static_assert(kDigits == kBlock, "one thread per digit in the scans");

// The orderable image of a value: unsigned keys compare as the values do; -0.0 is +0.0 first, so that both are one key.
template <typename K>
struct Codec;

template <>
struct Codec<uint32_t> {
    using Value = float;
    static __device__ __forceinline__ uint32_t encode(float v, bool& nan)
    {
        uint32_t u = __float_as_uint(v);
        nan = (u & 0x7fffffffu) > 0x7f800000u;
        if (u == 0x80000000u) u = 0u;
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    static __device__ __forceinline__ double decode(uint32_t k)
    {
        const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
        return (double)__uint_as_float(u);       // exact
    }
};

template <>
struct Codec<uint64_t> {
    using Value = double;
    static constexpr uint64_t kSign = 0x8000000000000000ull;
    static __device__ __forceinline__ uint64_t encode(double v, bool& nan)
    {
        uint64_t u = (uint64_t)__double_as_longlong(v);
        nan = (u & ~kSign) > 0x7ff0000000000000ull;
        if (u == kSign) u = 0ull;
        return (u & kSign) ? ~u : (u | kSign);
    }
    static __device__ __forceinline__ double decode(uint64_t k)
    {
        const uint64_t u = (k & kSign) ? (k ^ kSign) : ~k;
        return __longlong_as_double((long long)u);
    }
};

// a pass's source: the caller's values (first pass) or the keys of the pass before
template <typename K>
__device__ __forceinline__ K load_key(const K* __restrict__ src, int64_t i, bool& nan)
{
    nan = false;
    return src[i];
}
__device__ __forceinline__ uint32_t load_key(const float* __restrict__ src, int64_t i, bool& nan)
{
    return Codec<uint32_t>::encode(src[i], nan);
}
__device__ __forceinline__ uint64_t load_key(const double* __restrict__ src, int64_t i, bool& nan)
{
    return Codec<uint64_t>::encode(src[i], nan);
}

// exclusive scan of one value per thread over the workgroup (kBlock values), through `scratch` (kBlock words of LDS)
__device__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* scratch)
{
    const int tid = threadIdx.x;
    scratch[tid] = v;
    __syncthreads();
    uint32_t sum = v;
#pragma unroll
    for (int o = 1; o < kBlock; o <<= 1) {
        const uint32_t left = tid >= o ? scratch[tid - o] : 0u;
        __syncthreads();
        sum += left;
        scratch[tid] = sum;
        __syncthreads();
    }
    return sum - v;
}

template <typename K, typename Src>
__global__ __launch_bounds__(kBlock) void digit_histogram_kernel(const Src* __restrict__ src, int64_t n, int shift, uint32_t n_tiles,
                                                                 uint32_t* __restrict__ hist, uint32_t* status)
{
    __shared__ uint32_t counts[kDigits];
    const int tid = threadIdx.x;
    counts[tid] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kTile;
    bool any_nan = false;
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int64_t i = base + r * kBlock + tid;
        if (i < n) {
            bool nan;
            const K key = load_key(src, i, nan);
            any_nan |= nan;
            atomicAdd(&counts[(uint32_t)(key >> shift) & (kDigits - 1)], 1u);
        }
    }
    if (any_nan && status) atomicOr(status, MDX_STATUS_KS_NAN);
    __syncthreads();
    hist[(size_t)tid * n_tiles + blockIdx.x] = counts[tid];
}

// hist [digit][tile] -> each row's exclusive scan over the tiles, in place; totals [digit] = the row's sum
__global__ __launch_bounds__(kBlock) void tile_scan_kernel(uint32_t* __restrict__ hist, uint32_t n_tiles, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t scratch[kBlock];
    const int tid = threadIdx.x;
    uint32_t* row = hist + (size_t)blockIdx.x * n_tiles;
    const uint32_t per = (n_tiles + kBlock - 1) / kBlock;
    const uint32_t begin = min((uint32_t)tid * per, n_tiles), end = min(begin + per, n_tiles);
    uint32_t sum = 0u;
    for (uint32_t t = begin; t < end; ++t) sum += row[t];
    uint32_t run = block_exclusive_scan(sum, scratch);
    for (uint32_t t = begin; t < end; ++t) {
        const uint32_t c = row[t];
        row[t] = run;
        run += c;
    }
    if (tid == kBlock - 1) totals[blockIdx.x] = run;      // the last thread ends at the row's sum (its own range may be empty)
}

template <typename K, typename Src, bool kFinal>
__global__ __launch_bounds__(kBlock) void scatter_kernel(const Src* __restrict__ src, int64_t n, int shift, uint32_t n_tiles,
                                                         const uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals,
                                                         K* __restrict__ dst_keys, double* __restrict__ dst_values)
{
    __shared__ uint32_t counts[kWaves][kDigits];
    __shared__ uint32_t scratch[kBlock];
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) counts[w][tid] = 0u;
    const uint32_t digit_base = block_exclusive_scan(totals[tid], scratch);      // (its barriers publish the zeros too)

    // ---- the rank of every key among its wavefront's keys of the same digit, in index order
    volatile uint32_t* mine = counts[wave];
    const int64_t base = (int64_t)blockIdx.x * kTile + wave * (kWave * kItems) + lane;
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    K keys[kItems];
    uint32_t ranks[kItems];
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int64_t i = base + r * kWave;
        const bool valid = i < n;
        bool nan;
        const K key = valid ? load_key(src, i, nan) : (K)0;
        const uint32_t d = (uint32_t)(key >> shift) & (kDigits - 1);
        uint64_t peers = __ballot(valid);                  // ends as the valid lanes of this round that hold digit d
#pragma unroll
        for (int b = 0; b < kDigitBits; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t set = __ballot(valid && bit);
            peers &= bit ? set : ~set;
        }
        const uint32_t below = (uint32_t)__popcll(peers & lanes_below);
        const uint32_t start = valid ? mine[d] : 0u;
        keys[r] = key;
        ranks[r] = start + below;
        if (valid && below == 0u) mine[d] = start + (uint32_t)__popcll(peers);     // one lane per digit, after every lane's read
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();

    // ---- digit tid: where each wavefront's keys of it begin = digit base + this tile's scanned count + the wavefronts before
    uint32_t run = digit_base + hist[(size_t)tid * n_tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = counts[w][tid];
        counts[w][tid] = run;
        run += c;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int64_t i = base + r * kWave;
        if (i < n) {
            const uint32_t d = (uint32_t)(keys[r] >> shift) & (kDigits - 1);
            const int64_t place = (int64_t)counts[wave][d] + ranks[r];
            if (place < n) {                               // always, by construction: a store is never left unbounded
                if (kFinal)
                    dst_values[place] = Codec<K>::decode(keys[r]);
                else
                    dst_keys[place] = keys[r];
            }
        }
    }
}

// the number of elements <= x of the ascending array a[0..n)
__device__ __forceinline__ int64_t count_not_above(const double* __restrict__ a, int64_t n, double x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long long wave_max(long long v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const long long w = __shfl_xor(v, o, kWave);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void ks_rank_kernel(const double* __restrict__ a, int64_t n1, const double* __restrict__ b,
                                                         int64_t n2, int64_t weight_a, int64_t weight_b,
                                                         long long* __restrict__ block_max)
{
    __shared__ long long scratch[kWaves];
    const int tid = threadIdx.x;
    long long best = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + tid; i < n1 + n2; i += (int64_t)gridDim.x * kBlock) {
        const double x = i < n1 ? a[i] : b[i - n1];
        const long long v = count_not_above(a, n1, x) * weight_a - count_not_above(b, n2, x) * weight_b;
        const long long m = v < 0 ? -v : v;
        best = m > best ? m : best;
    }
    best = wave_max(best);
    if (tid % kWave == 0) scratch[tid / kWave] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) best = scratch[w] > best ? scratch[w] : best;
        block_max[blockIdx.x] = best;
    }
}

__global__ __launch_bounds__(kBlock) void ks_final_kernel(const long long* __restrict__ block_max, int blocks, int64_t* __restrict__ out)
{
    __shared__ long long scratch[kWaves];
    const int tid = threadIdx.x;
    long long best = 0;
    for (int i = tid; i < blocks; i += kBlock) best = block_max[i] > best ? block_max[i] : best;
    best = wave_max(best);
    if (tid % kWave == 0) scratch[tid / kWave] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) best = scratch[w] > best ? scratch[w] : best;
        out[0] = best;
    }
}

inline int64_t round_up16(int64_t bytes) { return (bytes + 15) / 16 * 16; }
inline bool samples_supported(int64_t n) { return n >= 1 && n <= MDX_KS_MAX_SAMPLES; }

template <typename K>
int sort_keys(const typename Codec<K>::Value* values, int64_t n, double* sorted_out, void* workspace, uint32_t* status,
              hipStream_t stream)
{
    const uint32_t n_tiles = (uint32_t)cdiv(n, kTile);
    K* spare = reinterpret_cast<K*>(workspace);
    uint32_t* hist = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(workspace) + round_up16(n * (int64_t)sizeof(K)));
    uint32_t* totals = hist + (size_t)kDigits * n_tiles;
    K* out_keys = reinterpret_cast<K*>(sorted_out);          // sizeof(K) <= sizeof(double): the output doubles as a key buffer
    const int passes = (int)sizeof(K);
    const dim3 tiles(n_tiles), digits(kDigits), block(kBlock);
    for (int p = 0; p < passes; ++p) {
        const int shift = p * kDigitBits;
        const K* from = (p & 1) ? spare : out_keys;           // passes 1, 2, ...; pass 0 reads the caller's values
        K* to = (p & 1) ? out_keys : spare;
        if (p == 0) {
            hipLaunchKernelGGL((digit_histogram_kernel<K, typename Codec<K>::Value>), tiles, block, 0, stream, values, n, shift,
                               n_tiles, hist, status);
            hipLaunchKernelGGL(tile_scan_kernel, digits, block, 0, stream, hist, n_tiles, totals);
            hipLaunchKernelGGL((scatter_kernel<K, typename Codec<K>::Value, false>), tiles, block, 0, stream, values, n, shift,
                               n_tiles, hist, totals, to, (double*)nullptr);
        } else {
            hipLaunchKernelGGL((digit_histogram_kernel<K, K>), tiles, block, 0, stream, from, n, shift, n_tiles, hist,
                               (uint32_t*)nullptr);
            hipLaunchKernelGGL(tile_scan_kernel, digits, block, 0, stream, hist, n_tiles, totals);
            if (p == passes - 1)
                hipLaunchKernelGGL((scatter_kernel<K, K, true>), tiles, block, 0, stream, from, n, shift, n_tiles, hist, totals,
                                   (K*)nullptr, sorted_out);
            else
                hipLaunchKernelGGL((scatter_kernel<K, K, false>), tiles, block, 0, stream, from, n, shift, n_tiles, hist, totals,
                                   to, (double*)nullptr);
        }
    }
    return launch_status();
}

int64_t gcd(int64_t a, int64_t b)
{
    while (b) {
        const int64_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

}  // namespace

extern "C" {

int64_t mdx_sort_keys_workspace_bytes(int64_t n, int values_are_f64)
{
    if (!samples_supported(n)) return 0;
    const int64_t key = values_are_f64 ? 8 : 4;
    return round_up16(n * key) + (int64_t)sizeof(uint32_t) * kDigits * (cdiv(n, kTile) + 1);
}

int mdx_sort_keys(const void* values, int64_t n, int values_are_f64, double* sorted_out, void* workspace, uint32_t* status,
                  mdx_stream_t stream)
{
    if (!samples_supported(n)) return MDX_ERR_UNSUPPORTED;
    if (!values || !sorted_out || !workspace || !aligned16(workspace) || (reinterpret_cast<uintptr_t>(sorted_out) & 7u) ||
        (reinterpret_cast<uintptr_t>(values) & (values_are_f64 ? 7u : 3u)))
        return MDX_ERR_INVALID_ARG;
    if (values_are_f64)
        return sort_keys<uint64_t>(static_cast<const double*>(values), n, sorted_out, workspace, status, as_stream(stream));
    return sort_keys<uint32_t>(static_cast<const float*>(values), n, sorted_out, workspace, status, as_stream(stream));
}

int64_t mdx_ks_two_sample_workspace_bytes(int64_t n1, int64_t n2)
{
    if (!samples_supported(n1) || !samples_supported(n2)) return 0;
    return (int64_t)sizeof(long long) * kMaxRankBlocks;
}

int mdx_ks_two_sample_sorted(const double* a_sorted, int64_t n1, const double* b_sorted, int64_t n2, void* workspace,
                             int64_t* numerator_out, mdx_stream_t stream)
{
    if (!samples_supported(n1) || !samples_supported(n2)) return MDX_ERR_UNSUPPORTED;
    if (!a_sorted || !b_sorted || !workspace || !numerator_out || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return MDX_ERR_INVALID_ARG;
    const int64_t g = gcd(n1, n2);
    const unsigned blocks = flat_grid(n1 + n2);              // <= kMaxRankBlocks
    long long* block_max = static_cast<long long*>(workspace);
    hipLaunchKernelGGL(ks_rank_kernel, dim3(blocks), dim3(kBlock), 0, as_stream(stream), a_sorted, n1, b_sorted, n2, n2 / g, n1 / g,
                       block_max);
    hipLaunchKernelGGL(ks_final_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), block_max, (int)blocks, numerator_out);
    return launch_status();
}

}  // extern "C"

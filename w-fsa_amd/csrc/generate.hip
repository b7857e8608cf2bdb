// Unconditional generation (generate.hpp): the running sums, the walk and the
// scan between its two passes.
#include "generate.hpp"

#include "sample.hpp"

#pragma clang fp contract(off)

namespace wfsa {

namespace {

constexpr int kWave = 64;
constexpr int kWaves = kGenerateBlock / kWave;

// One thread per group -- state U's transitions (g = 2U) or emissions
// (g = 2U + 1) -- adds its members' masses left to right.  Thread j < n_params
// also looks at weight j: NaN or +inf sets the flag.
__global__ __launch_bounds__(kGenerateBlock) void generate_cdf_kernel(GenerateArgs a) {
    const int64_t t = int64_t(blockIdx.x) * kGenerateBlock + threadIdx.x;
    if (t < a.g.n_params) {
        const double v = a.w[t];
        if (v != v || v == INFINITY) *a.flag = 1u;
    }
    if (t >= 2 * int64_t(a.g.n_states)) return;
    const int32_t U = int32_t(t >> 1);
    const bool em = (t & 1) != 0;
    const int32_t* ptr = em ? a.g.em_ptr : a.g.tr_ptr;
    const int32_t* param = em ? a.g.em_param : a.g.tr_param;
    double* cdf = em ? a.cdf_em : a.cdf_tr;
    double sum = 0.0;
    for (int32_t k = ptr[U]; k < ptr[U + 1]; ++k) {
        const int32_t p = param[k];
        sum += p < 0 ? 1.0 : exp(a.w[p]);
        cdf[k] = sum;
    }
}

// One choice among the candidates lo .. hi - 1 (hi > lo, their last running sum
// T > 0) with the uniform u: the first running sum above u * T by bisection;
// when rounding leaves none, the last candidate of positive mass.
__device__ inline int32_t generate_choose(const double* __restrict__ cdf, const int32_t* __restrict__ param,
                                          const double* __restrict__ w, int32_t lo, int32_t hi, double T, double u) {
    const double x = u * T;
    int32_t l = lo, h = hi;
    while (l < h) {
        const int32_t mid = l + ((h - l) >> 1);
        const bool above = cdf[mid] > x;
        h = above ? mid : h;
        l = above ? l : mid + 1;
    }
    if (l == hi) {   // (u * T rounded up to T)
        l = hi - 1;
        while (l > lo) {
            const int32_t p = param[l];
            if ((p < 0 ? 1.0 : exp(w[p])) > 0.0) break;
            --l;
        }
    }
    return l;
}

// One lane per sample, a wave's 64 lanes 64 consecutive samples.  The walk's
// state -- the state id, the step, the byte and id counts, the two sums --
// stays in registers; a lane whose sample has ended waits for its wave.
// FILL = false: the sizes, sums and status per sample.  FILL = true: the same
// walk again, writing the bytes at off[i] and the parameter ids at prow[i].
template <bool FILL>
__global__ __launch_bounds__(kGenerateBlock) void generate_walk_kernel(GenerateArgs a) {
    const int64_t i = int64_t(blockIdx.x) * kGenerateBlock + threadIdx.x;
    if (i >= a.n) return;
    const GenerateModel& g = a.g;
    int32_t U = g.start;
    uint32_t m = 0;
    int32_t len = 0, plen = 0;
    double logw = 0.0, logp = 0.0;
    int status = -1;
    uint8_t* const sym = FILL ? a.sym + a.off[i] : nullptr;
    int32_t* const pidx = FILL ? a.pidx + a.prow[i] : nullptr;
    // (what the sizing pass counted for this sample: no store goes past it)
    const int32_t cap_len = FILL ? int32_t(a.off[i + 1] - a.off[i]) : 0;
    const int32_t cap_ids = FILL ? int32_t(a.prow[i + 1] - a.prow[i]) : 0;
    while (status < 0) {
        if (m >= a.max_steps) {   // (never, without an epsilon cycle: the cap keeps the draw index inside 32 bits)
            status = 1;
            break;
        }
        int32_t lo = g.tr_ptr[U], hi = g.tr_ptr[U + 1];
        double T = hi > lo ? a.cdf_tr[hi - 1] : 0.0;
        if (!(T > 0.0)) {
            status = 2;
            break;
        }
        int32_t k = generate_choose(a.cdf_tr, g.tr_param, a.w, lo, hi, T, sample_uniform(a.seed, uint64_t(i), kGenerateSampleWord, 2u * m));
        int32_t p = g.tr_param[k];
        double wk = p < 0 ? 0.0 : a.w[p];
        if (p >= 0) {
            if (FILL && plen < cap_ids) pidx[plen] = p;
            ++plen;
            logw += wk;
        }
        logp += wk - log(T);
        const int32_t V = g.tr_dst[k];
        if (V == g.end) {
            status = 0;
            break;
        }
        lo = g.em_ptr[V];
        hi = g.em_ptr[V + 1];
        T = hi > lo ? a.cdf_em[hi - 1] : 0.0;
        if (!(T > 0.0)) {
            status = 2;
            break;
        }
        k = generate_choose(a.cdf_em, g.em_param, a.w, lo, hi, T, sample_uniform(a.seed, uint64_t(i), kGenerateSampleWord, 2u * m + 1u));
        const int32_t L = g.em_len[k];
        if (L > a.max_len - len) {
            status = 1;
            break;
        }
        p = g.em_param[k];
        wk = p < 0 ? 0.0 : a.w[p];
        if (p >= 0) {
            if (FILL && plen < cap_ids) pidx[plen] = p;
            ++plen;
            logw += wk;
        }
        logp += wk - log(T);
        if (FILL) {
            const uint8_t* src = g.em_bytes + g.em_off[k];
            for (int32_t b = 0; b < L && len + b < cap_len; ++b) sym[len + b] = src[b];
        }
        len += L;
        U = V;
        ++m;
    }
    if (!FILL) {
        a.len[i] = len;
        a.plen[i] = plen;
        a.logw[i] = logw;
        a.logp[i] = logp;
        a.status[i] = int8_t(status);
    }
}

// the block's inclusive scan of one value per thread; total = the block's sum
__device__ inline int64_t generate_block_scan(int64_t v, int64_t* wsum, int64_t& total) {
    const int lane = int(threadIdx.x) & (kWave - 1), wave = int(threadIdx.x) / kWave;
    for (int d = 1; d < kWave; d <<= 1) {
        const int64_t up = __shfl_up(static_cast<long long>(v), d, kWave);
        v += lane >= d ? up : 0;
    }
    if (lane == kWave - 1) wsum[wave] = v;
    __syncthreads();
    int64_t base = 0;
    total = 0;
    for (int k = 0; k < kWaves; ++k) {
        const int64_t s = wsum[k];
        base += k < wave ? s : 0;
        total += s;
    }
    __syncthreads();   // (wsum is written again by the next scan)
    return v + base;
}

// The exclusive scan of len -> off and plen -> prow over tiles of one block:
// PHASE 0 sums each tile into bsum, PHASE 1 (one block) turns bsum into the
// tiles' exclusive offsets and writes the totals off[n] / prow[n], PHASE 2
// scans each tile from its offset.
template <int PHASE>
__global__ __launch_bounds__(kGenerateBlock) void generate_scan_kernel(GenerateArgs a) {
    __shared__ int64_t wsum[kWaves];
    const int64_t tiles = generate_tiles(a.n);
    if (PHASE == 1) {
        for (int arr = 0; arr < 2; ++arr) {
            int64_t* bs = a.bsum + arr * tiles;
            int64_t carry = 0;
            for (int64_t base = 0; base < tiles; base += kGenerateBlock) {
                const int64_t t = base + threadIdx.x;
                const int64_t v = t < tiles ? bs[t] : 0;
                int64_t total;
                const int64_t inc = generate_block_scan(v, wsum, total);
                if (t < tiles) bs[t] = carry + inc - v;
                carry += total;
            }
            if (threadIdx.x == 0) (arr == 0 ? a.off : a.prow)[a.n] = carry;
        }
        return;
    }
    const int64_t tile = blockIdx.x;
    const int64_t i = tile * kGenerateBlock + threadIdx.x;
    for (int arr = 0; arr < 2; ++arr) {
        const int32_t* in = arr == 0 ? a.len : a.plen;
        const int64_t v = i < a.n ? in[i] : 0;
        int64_t total;
        const int64_t inc = generate_block_scan(v, wsum, total);
        if (PHASE == 0) {
            if (threadIdx.x == 0) a.bsum[arr * tiles + tile] = total;
        } else if (i < a.n) {
            (arr == 0 ? a.off : a.prow)[i] = a.bsum[arr * tiles + tile] + inc - v;
        }
    }
}

}  // namespace

hipError_t launch_generate_cdf(const GenerateArgs& a, hipStream_t stream) {
    const int64_t threads = 2 * int64_t(a.g.n_states) > a.g.n_params ? 2 * int64_t(a.g.n_states) : int64_t(a.g.n_params);
    if (threads > 0)
        hipLaunchKernelGGL(generate_cdf_kernel, dim3(unsigned(generate_tiles(threads))), dim3(kGenerateBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_generate_size(const GenerateArgs& a, hipStream_t stream) {
    const dim3 grid(unsigned(generate_tiles(a.n))), block(kGenerateBlock);
    hipLaunchKernelGGL(generate_walk_kernel<false>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(generate_scan_kernel<0>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(generate_scan_kernel<1>, dim3(1), block, 0, stream, a);
    hipLaunchKernelGGL(generate_scan_kernel<2>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_generate_fill(const GenerateArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(generate_walk_kernel<true>, dim3(unsigned(generate_tiles(a.n))), dim3(kGenerateBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace wfsa

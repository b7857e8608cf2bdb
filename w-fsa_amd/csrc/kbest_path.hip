// The top-K (max, +) trellis pass with back-pointers (kbest_path.hpp).
#include "kbest_path.hpp"

#include <climits>

namespace wfsa {

namespace {

constexpr int kWave = 64;
constexpr int kRankMask = (1 << kKBestRankBits) - 1;

// A wave's lanes hand values to each other through its global scratch rows:
// a phase's stores are complete, and its loads done, before the next phase
// (as in best_path.hip).
__device__ __forceinline__ void phase_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// lw[g] = sum of the weights of edge g's parameters, in list order (no exp);
// an edge without parameters weighs log 1 -- the same sum as the Viterbi
// decode's, so the k = 1 weights agree bit for bit
__global__ __launch_bounds__(256) void kbest_edge_lw_kernel(KBestArgs a) {
    const int64_t n = int64_t(a.n_edges) + a.n_end;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        double t = 0.0;
        for (int q = a.pptr[g]; q < a.pptr[g + 1]; ++q) t += a.wt[a.pidx[q]];
        a.lw[g] = t;
    }
}

// A lane's KC candidates, descending, in registers: every index is a
// compile-time constant after unrolling (a runtime index would put the arrays
// in scratch memory).
template <int KC>
struct TopList {
    double v[KC];
    int32_t p[KC];   // what came with the value: a packed (edge, source rank)
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            v[j] = -INFINITY;
            p[j] = -1;
        }
    }
    // true when x would enter the list
    __device__ __forceinline__ bool beats_last(double x) const { return x > v[KC - 1]; }
    // insert behind every entry >= x (strict "greater than": an earlier
    // candidate stays ahead of an equal later one); the last entry falls off
    __device__ __forceinline__ void insert(double x, int32_t xp) {
        // entry j takes entry j - 1 when x goes above that, x when x goes
        // exactly here, and stays otherwise (selects, no branches)
#pragma unroll
        for (int j = KC - 1; j >= 1; --j) {
            const bool above = x > v[j - 1], here = x > v[j];
            v[j] = above ? v[j - 1] : (here ? x : v[j]);
            p[j] = above ? p[j - 1] : (here ? xp : p[j]);
        }
        const bool head = x > v[0];
        v[0] = head ? x : v[0];
        p[0] = head ? xp : p[0];
    }
    // drop the head
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int j = 0; j + 1 < KC; ++j) {
            v[j] = v[j + 1];
            p[j] = p[j + 1];
        }
        v[KC - 1] = -INFINITY;
        p[KC - 1] = -1;
    }
};

template <int KC>
__global__ __launch_bounds__(kKBestWavesPerBlock* kWave) void kbest_kernel(KBestArgs a) {
    static_assert(KC >= 2 && KC <= kKBestMax && KC <= (1 << kKBestRankBits) && KC < kWave, "capacity");
    const WideModel& W = a.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = a.n_nodes;
    const int K = a.k;   // 1 .. KC: the list length in scratch and the paths written
    // (one wave's scratch is below the 1 GiB budget: offsets into it are 32-bit)
    const int row_len = N * K;
    double* R = a.score + gw * kbest_score_doubles(N, K);
    int32_t* BP = a.back + gw * kbest_back_ints(a.max_len, a.max_dst, K);
    // both rows hold -inf outside the live lists: set once, restored behind every position
    for (int k = lane; k < 2 * row_len; k += kWave) R[k] = -INFINITY;
    phase_fence();
    for (;;) {
        // the ticket as in best_path_kernel: every lane runs the add (lane 0
        // adds one, the rest nothing), so no branch on the lane surrounds it
        __builtin_amdgcn_wave_barrier();
        const unsigned got = __hip_atomic_fetch_add(a.ctr, lane == 0 ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int s = __builtin_amdgcn_readfirstlane(int(got));   // lane 0's ticket
        if (s < 0 || s >= a.n_strings) break;
        const int64_t o0 = a.off[s];
        const int L = int(a.off[s + 1] - o0);
        const uint8_t* str = a.sym + o0;
        // nodes live at position j: the destinations of byte c_{j-1}; at 0 the start
        auto live_begin = [&](int j) { return j == 0 ? 0 : W.c_ptr[str[j - 1]]; };
        auto live_end = [&](int j) { return j == 0 ? 1 : W.c_ptr[str[j - 1] + 1]; };
        auto live_node = [&](int j, int k) { return j == 0 ? a.start : W.dst[k]; };
        auto clear_row = [&](int j) {
            double* row = R + (j & 1) * row_len;
            for (int k = live_begin(j) + lane; k < live_end(j); k += kWave) {
                const int list = live_node(j, k) * K;
                for (int r = 0; r < K; ++r) row[list + r] = -INFINITY;
            }
        };
        if (lane == 0) R[a.start * K] = 0.0;   // the empty prefix; ranks 1 .. stay -inf
        phase_fence();
        int reached = L;   // the last position whose row was written
        for (int i = 0; i < L; ++i) {
            const double* cur = R + (i & 1) * row_len;
            double* nxt = R + ((i + 1) & 1) * row_len;
            const int cb = live_begin(i + 1), ce = live_end(i + 1);
            int32_t* bp = BP + int64_t(i) * a.max_dst * K;
            bool any = false;
            // The loops below run wave-uniform trip counts (a lane past its
            // own range offers -inf, which no insertion takes): a lane that
            // left a loop early would need its lists kept apart from the
            // others' still running, which doubles the registers.
            for (int k0 = cb; k0 < ce; k0 += kWave) {
                const int k = k0 + lane;
                const bool live = k < ce;
                TopList<KC> top;
                top.reset();
                const int e1 = live ? W.e_ptr[k + 1] : 0;
                // (written as a guarded do-while: the compiler does not rotate
                // a loop whose condition is a wave vote, and the unrotated
                // form keeps a second copy of the lists)
                int e = live ? W.e_ptr[k] : 0;
                if (__any(e < e1 ? 1 : 0))
#pragma unroll 1
                do {
                    int src = 0;
                    double w = -INFINITY;
                    if (e < e1) {
                        src = W.e_src[e] * K;
                        w = a.lw[W.e_g[e]];
                    }
                    // the source list descends: once no lane's candidate
                    // enters, no later rank would (that last insertion takes
                    // nothing; the loop has one exit, behind it)
                    int r = 0;
                    bool more;
#pragma unroll 1
                    do {
                        const double v = cur[src + r] + w;
                        more = __any(top.beats_last(v) ? 1 : 0) != 0;
                        top.insert(v, (e << kKBestRankBits) | r);
                    } while (++r < K && more);
                } while (++e, __any(e < e1 ? 1 : 0));
                if (live) {
                    const int out = W.dst[k] * K, ob = (k - cb) * K;
#pragma unroll
                    for (int j = 0; j < KC; ++j)
                        if (j < K) {
                            nxt[out + j] = top.v[j];
                            bp[ob + j] = top.p[j];
                        }
                    any = any || top.p[0] >= 0;
                }
            }
            phase_fence();
            clear_row(i);
            phase_fence();
            if (!__any(any ? 1 : 0)) {   // nothing reachable: row i + 1 is all -inf already
                reached = -1;
                break;
            }
        }
        // the lane's best candidates over the end edges of its nodes live at
        // position L, p = (end edge << 4) | rank.  The end edges are numbered
        // by source node and the live slots ascend by node, so ascending p is
        // the tie order (live slot, end edge, rank), within a lane (its
        // insertion order) and between lanes.
        TopList<KC> top;
        top.reset();
        if (reached == L) {
            const double* row = R + (L & 1) * row_len;
            const int lb = live_begin(L), le = live_end(L);
            for (int k0 = lb; k0 < le; k0 += kWave) {
                const int k = k0 + lane;
                const bool live = k < le;
                const int S = live ? live_node(L, k) : 0;
                const int src = S * K;
                const int x1 = live ? a.x_ptr[S + 1] : 0;
                int x = live ? a.x_ptr[S] : 0;
                if (__any(x < x1 ? 1 : 0))
#pragma unroll 1
                do {
                    const double w = x < x1 ? a.lw[a.n_edges + x] : -INFINITY;
                    int r = 0;
                    bool more;
#pragma unroll 1
                    do {
                        const double v = row[src + r] + w;
                        more = __any(top.beats_last(v) ? 1 : 0) != 0;
                        top.insert(v, (x << kKBestRankBits) | r);
                    } while (++r < K && more);
                } while (++x, __any(x < x1 ? 1 : 0));
            }
            phase_fence();
            clear_row(L);
        }
        // K rounds of wave arg-max over the lanes' heads (a lane without a
        // candidate offers -inf, INT_MAX); the winner pops its head and lane t
        // keeps round t's result
        double mv = -INFINITY;
        int mp = INT_MAX;
        for (int t = 0; t < K; ++t) {
            const bool have = top.p[0] >= 0;
            double bv = top.v[0];
            int bp = have ? top.p[0] : INT_MAX;
            for (int d = kWave / 2; d >= 1; d >>= 1) {
                const double ov = __shfl_xor(bv, d);
                const int op = __shfl_xor(bp, d);
                if (ov > bv || (ov == bv && op < bp)) {
                    bv = ov;
                    bp = op;
                }
            }
            if (lane == t) {
                mv = bv;
                mp = bp;
            }
            if (have && top.p[0] == bp) top.pop();   // (an end edge has one source: p names one lane's entry)
        }
        phase_fence();
        // the slot of `node` among the nodes live at position j >= 1 (ascending nodes)
        auto slot_of = [&](int j, int node) {
            int lo = live_begin(j), hi = live_end(j) - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (W.dst[mid] < node) lo = mid + 1;
                else hi = mid;
            }
            return lo;
        };
        if (lane < K) {   // one lane per output path
            int32_t* out = a.path + (o0 + s) * int64_t(K) + int64_t(lane) * (L + 1);
            bool ok = mp != INT_MAX && mv > -INFINITY;
            if (ok) {
                const int x = mp >> kKBestRankBits;
                int r = mp & kRankMask;
                out[L] = a.n_edges + x;
                int k = 0;
                if (L >= 1) {   // the end edge's source: the last node whose end edges begin at or before x
                    int lo = 0, hi = N - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (a.x_ptr[mid] <= x) lo = mid;
                        else hi = mid - 1;
                    }
                    k = slot_of(L, lo);
                }
                for (int i = L; i >= 1; --i) {
                    const int pb = BP[int64_t(i - 1) * a.max_dst * K + ((k - live_begin(i)) * K + r)];
                    if (pb < 0) {   // (a finite entry always has a back-pointer)
                        ok = false;
                        break;
                    }
                    const int e = pb >> kKBestRankBits;
                    r = pb & kRankMask;
                    out[i - 1] = W.e_g[e];
                    if (i >= 2) k = slot_of(i - 1, W.e_src[e]);
                }
            }
            a.best[int64_t(s) * K + lane] = ok ? mv : -INFINITY;
            if (!ok) out[0] = -1;
        }
    }
}

template <int KC>
void launch_capacity(const KBestArgs& a, int grid, int waves, hipStream_t stream) {
    hipLaunchKernelGGL(kbest_kernel<KC>, dim3(unsigned(grid)), dim3(unsigned(waves * kWave)), 0, stream, a);
}

}  // namespace

hipError_t launch_kbest_paths(const KBestArgs& a, int grid, int waves, hipStream_t stream) {
    const int kc = kbest_capacity(a.k);
    if (grid < 1 || waves < 1 || waves > kKBestWavesPerBlock || kc == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.ctr, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    const int64_t n = int64_t(a.n_edges) + a.n_end;
    if (n > 0) {
        const int blocks = int(n / 256 < 1 ? 1 : (n / 256 > 4096 ? 4096 : n / 256));
        hipLaunchKernelGGL(kbest_edge_lw_kernel, dim3(unsigned(blocks)), dim3(256), 0, stream, a);
    }
    if (a.n_strings > 0) {
        if (kc == 2) launch_capacity<2>(a, grid, waves, stream);
        else if (kc == 4) launch_capacity<4>(a, grid, waves, stream);
        else if (kc == 8) launch_capacity<8>(a, grid, waves, stream);
        else launch_capacity<16>(a, grid, waves, stream);
    }
    return hipGetLastError();
}

}  // namespace wfsa

// The (max, +) trellis passes with back-pointers (decode.hpp): the scalar
// Viterbi kernel, the top-K kernels, and what they share.
#include "decode.hpp"

#include <climits>

#include "decode_device.hpp"

namespace wfsa {

namespace {

constexpr int kRankMask = (1 << kKBestRankBits) - 1;

__device__ __forceinline__ void take_if(bool take, int& mine, int theirs) {
    if (take) mine = theirs;
}

// Wave arg-max by butterfly: every lane ends with the greatest v, among equal
// v the lowest key, and that lane's `carry` (a lane without a candidate offers
// -inf, INT_MAX).  Every lane runs every shuffle.
template <class... Carry>
__device__ __forceinline__ void wave_argmax(double& v, int& key, Carry&... carry) {
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(v, d);
        const int ok = __shfl_xor(key, d);
        const bool take = ov > v || (ov == v && ok < key);
        (take_if(take, carry, __shfl_xor(carry, d)), ...);
        if (take) {
            v = ov;
            key = ok;
        }
    }
}

// lw[g] = sum of the weights of edge g's parameters, in list order (no exp);
// an edge without parameters weighs log 1.  Both decodes launch this kernel,
// so their k = 1 weights agree bit for bit.
__global__ __launch_bounds__(256) void decode_edge_weight_kernel(DecodeArgs a) {
    const int64_t n = int64_t(a.n_edges) + a.n_end;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        double t = 0.0;
        for (int q = a.pptr[g]; q < a.pptr[g + 1]; ++q) t += a.wt[a.pidx[q]];
        a.lw[g] = t;
    }
}

__global__ __launch_bounds__(kDecodeWavesPerBlock* kWave) void best_path_kernel(DecodeArgs a) {
    const WideModel& W = a.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = a.n_nodes;
    double* R = a.score + gw * decode_score_doubles(N, 1);
    int32_t* BP = a.back + gw * decode_back_ints(a.max_len, a.max_dst, 1);
    // both rows hold -inf outside the live nodes: set once, restored behind every position
    for (int k = lane; k < 2 * N; k += kWave) R[k] = -INFINITY;
    phase_fence();
    for (;;) {
        const int s = next_string(a.ctr, lane);
        if (s < 0 || s >= a.n_strings) break;
        const int64_t o0 = a.off[s];
        const int L = int(a.off[s + 1] - o0);
        const LiveSet live{W, a.sym + o0, a.start};
        auto clear_row = [&](int j) {
            double* row = R + int64_t(j & 1) * N;
            for (int k = live.begin(j) + lane; k < live.end(j); k += kWave) row[live.node(j, k)] = -INFINITY;
        };
        if (lane == 0) R[a.start] = 0.0;
        phase_fence();
        int reached = L;   // the last position whose row was written
        for (int i = 0; i < L; ++i) {
            const double* cur = R + int64_t(i & 1) * N;
            double* nxt = R + int64_t((i + 1) & 1) * N;
            const int cb = live.begin(i + 1), ce = live.end(i + 1);
            int32_t* bp = BP + int64_t(i) * a.max_dst;
            bool any = false;
            for (int k = cb + lane; k < ce; k += kWave) {
                double bv = -INFINITY;
                int be = -1;
                for (int e = W.e_ptr[k]; e < W.e_ptr[k + 1]; ++e) {
                    const double v = cur[W.e_src[e]] + a.lw[W.e_g[e]];
                    if (v > bv) {   // strict: the first in-edge keeps a tie, -inf never wins
                        bv = v;
                        be = e;
                    }
                }
                nxt[W.dst[k]] = bv;
                bp[k - cb] = be;
                any = any || be >= 0;
            }
            phase_fence();
            clear_row(i);
            phase_fence();
            if (!__any(any ? 1 : 0)) {   // nothing reachable: row i + 1 is all -inf already
                reached = -1;
                break;
            }
        }
        // the end edges of the nodes live at position L
        double bv = -INFINITY;
        int bk = INT_MAX, bx = -1;
        if (reached == L) {
            const double* row = R + int64_t(L & 1) * N;
            for (int k = live.begin(L) + lane; k < live.end(L); k += kWave) {
                const int S = live.node(L, k);
                const double sc = row[S];
                if (!(sc > -INFINITY)) continue;
                for (int x = a.x_ptr[S]; x < a.x_ptr[S + 1]; ++x) {
                    const double v = sc + a.lw[a.n_edges + x];
                    if (v > bv) {   // a lane's k ascend: the lowest node, then its first end edge, keeps a tie
                        bv = v;
                        bk = k;
                        bx = x;
                    }
                }
            }
            phase_fence();
            clear_row(L);
        }
        wave_argmax(bv, bk, bx);   // ties to the lowest slot k
        phase_fence();
        if (lane == 0) {
            int32_t* out = a.path + o0 + s;
            bool ok = bx >= 0;
            if (ok) {
                out[L] = a.n_edges + bx;
                int k = bk;
                for (int i = L; i >= 1; --i) {
                    const int e = BP[int64_t(i - 1) * a.max_dst + (k - live.begin(i))];
                    if (e < 0) {   // (a node on the best path always has a winning in-edge)
                        ok = false;
                        break;
                    }
                    out[i - 1] = W.e_g[e];
                    if (i >= 2) k = live.slot_of(i - 1, W.e_src[e]);   // the source's entry among the destinations of byte c_{i-2}
                }
            }
            a.best[s] = ok ? bv : -INFINITY;
            if (!ok) out[0] = -1;
        }
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
__global__ __launch_bounds__(kDecodeWavesPerBlock* kWave) void kbest_kernel(DecodeArgs a) {
    static_assert(KC >= 2 && KC <= kKBestMax && KC <= (1 << kKBestRankBits) && KC < kWave, "capacity");
    const WideModel& W = a.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = a.n_nodes;
    const int K = a.k;   // 1 .. KC: the list length in scratch and the paths written
    // (one wave's scratch is below the 1 GiB budget: offsets into it are 32-bit)
    const int row_len = N * K;
    double* R = a.score + gw * decode_score_doubles(N, K);
    int32_t* BP = a.back + gw * decode_back_ints(a.max_len, a.max_dst, K);
    // both rows hold -inf outside the live lists: set once, restored behind every position
    for (int k = lane; k < 2 * row_len; k += kWave) R[k] = -INFINITY;
    phase_fence();
    for (;;) {
        const int s = next_string(a.ctr, lane);
        if (s < 0 || s >= a.n_strings) break;
        const int64_t o0 = a.off[s];
        const int L = int(a.off[s + 1] - o0);
        const LiveSet live{W, a.sym + o0, a.start};
        auto clear_row = [&](int j) {
            double* row = R + (j & 1) * row_len;
            for (int k = live.begin(j) + lane; k < live.end(j); k += kWave) {
                const int list = live.node(j, k) * K;
                for (int r = 0; r < K; ++r) row[list + r] = -INFINITY;
            }
        };
        if (lane == 0) R[a.start * K] = 0.0;   // the empty prefix; ranks 1 .. stay -inf
        phase_fence();
        int reached = L;   // the last position whose row was written
        for (int i = 0; i < L; ++i) {
            const double* cur = R + (i & 1) * row_len;
            double* nxt = R + ((i + 1) & 1) * row_len;
            const int cb = live.begin(i + 1), ce = live.end(i + 1);
            int32_t* bp = BP + int64_t(i) * a.max_dst * K;
            bool any = false;
            // The loops below run wave-uniform trip counts (a lane past its
            // own range offers -inf, which no insertion takes): a lane that
            // left a loop early would need its lists kept apart from the
            // others' still running, which doubles the registers.
            for (int k0 = cb; k0 < ce; k0 += kWave) {
                const int k = k0 + lane;
                const bool live_k = k < ce;
                TopList<KC> top;
                top.reset();
                const int e1 = live_k ? W.e_ptr[k + 1] : 0;
                // (written as a guarded do-while: the compiler does not rotate
                // a loop whose condition is a wave vote, and the unrotated
                // form keeps a second copy of the lists)
                int e = live_k ? W.e_ptr[k] : 0;
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
                if (live_k) {
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
            const int lb = live.begin(L), le = live.end(L);
            for (int k0 = lb; k0 < le; k0 += kWave) {
                const int k = k0 + lane;
                const bool live_k = k < le;
                const int S = live_k ? live.node(L, k) : 0;
                const int src = S * K;
                const int x1 = live_k ? a.x_ptr[S + 1] : 0;
                int x = live_k ? a.x_ptr[S] : 0;
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
        // K rounds of wave arg-max over the lanes' heads, ties to the lowest
        // p; the winner pops its head and lane t keeps round t's result
        double mv = -INFINITY;
        int mp = INT_MAX;
        for (int t = 0; t < K; ++t) {
            const bool have = top.p[0] >= 0;
            double bv = top.v[0];
            int bp = have ? top.p[0] : INT_MAX;
            wave_argmax(bv, bp);
            if (lane == t) {
                mv = bv;
                mp = bp;
            }
            if (have && top.p[0] == bp) top.pop();   // (an end edge has one source: p names one lane's entry)
        }
        phase_fence();
        if (lane < K) {   // one lane per output path
            // (the walk's own view of the string: with the pass's `live` used
            // here as well, kbest_kernel<4>, <8> and <16> take 2, 6 and 3 more
            // VGPRs, and <8> loses a wave of occupancy)
            const LiveSet walk{W, a.sym + o0, a.start};
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
                    k = walk.slot_of(L, lo);
                }
                for (int i = L; i >= 1; --i) {
                    const int pb = BP[int64_t(i - 1) * a.max_dst * K + ((k - walk.begin(i)) * K + r)];
                    if (pb < 0) {   // (a finite entry always has a back-pointer)
                        ok = false;
                        break;
                    }
                    const int e = pb >> kKBestRankBits;
                    r = pb & kRankMask;
                    out[i - 1] = W.e_g[e];
                    if (i >= 2) k = walk.slot_of(i - 1, W.e_src[e]);
                }
            }
            a.best[int64_t(s) * K + lane] = ok ? mv : -INFINITY;
            if (!ok) out[0] = -1;
        }
    }
}

}  // namespace

// what every decode launch starts with: the work counter at zero and the edge
// log-weights of a.wt
hipError_t launch_edge_weights(const DecodeArgs& a, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(a.ctr, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    const int64_t n = int64_t(a.n_edges) + a.n_end;
    if (n > 0) {
        const int blocks = int(n / 256 < 1 ? 1 : (n / 256 > 4096 ? 4096 : n / 256));
        hipLaunchKernelGGL(decode_edge_weight_kernel, dim3(unsigned(blocks)), dim3(256), 0, stream, a);
    }
    return hipSuccess;
}

namespace {

template <class Kernel>
hipError_t launch_decode(Kernel kernel, const DecodeArgs& a, int grid, int waves, hipStream_t stream) {
    if (grid < 1 || waves < 1 || waves > kDecodeWavesPerBlock) return hipErrorInvalidValue;
    if (hipError_t e = launch_edge_weights(a, stream); e != hipSuccess) return e;
    if (a.n_strings > 0) hipLaunchKernelGGL(kernel, dim3(unsigned(grid)), dim3(unsigned(waves * kWave)), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_best_paths(const DecodeArgs& a, int grid, int waves, hipStream_t stream) {
    if (a.k != 1) return hipErrorInvalidValue;
    return launch_decode(best_path_kernel, a, grid, waves, stream);
}

hipError_t launch_kbest_paths(const DecodeArgs& a, int grid, int waves, hipStream_t stream) {
    switch (kbest_capacity(a.k)) {
        case 2: return launch_decode(kbest_kernel<2>, a, grid, waves, stream);
        case 4: return launch_decode(kbest_kernel<4>, a, grid, waves, stream);
        case 8: return launch_decode(kbest_kernel<8>, a, grid, waves, stream);
        case 16: return launch_decode(kbest_kernel<16>, a, grid, waves, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace wfsa

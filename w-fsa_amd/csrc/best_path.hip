// The (max, +) trellis pass with back-pointers (best_path.hpp).
#include "best_path.hpp"

#include <climits>

namespace wfsa {

namespace {

constexpr int kWave = 64;

// A wave's lanes hand values to each other through its global scratch rows:
// a phase's stores are complete, and its loads done, before the next phase
// (the same fence the H_f traversal kernel uses between its phases).
__device__ __forceinline__ void phase_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// lw[g] = sum of the weights of edge g's parameters, in list order (no exp);
// an edge without parameters weighs log 1
__global__ __launch_bounds__(256) void best_edge_weight_kernel(BestPathArgs a) {
    const int64_t n = int64_t(a.n_edges) + a.n_end;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        double t = 0.0;
        for (int q = a.pptr[g]; q < a.pptr[g + 1]; ++q) t += a.wt[a.pidx[q]];
        a.lw[g] = t;
    }
}

__global__ __launch_bounds__(kBestWavesPerBlock* kWave) void best_path_kernel(BestPathArgs a) {
    const WideModel& W = a.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = a.n_nodes;
    double* R = a.score + gw * best_path_score_doubles(N);
    int32_t* BP = a.back + gw * best_path_back_ints(a.max_len, a.max_dst);
    // both rows hold -inf outside the live nodes: set once, restored behind every position
    for (int k = lane; k < 2 * N; k += kWave) R[k] = -INFINITY;
    phase_fence();
    for (;;) {
        // The wave takes the next string: every lane runs the add (lane 0 adds
        // one, the rest nothing), so the loop starts with no branch on the
        // lane.  With "if (lane == 0)" around the add, the compiler threaded
        // the other lanes' path round the loop past it: they parted from lane
        // 0 and decoded string 0 for ever.
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
            double* row = R + int64_t(j & 1) * N;
            for (int k = live_begin(j) + lane; k < live_end(j); k += kWave) row[live_node(j, k)] = -INFINITY;
        };
        if (lane == 0) R[a.start] = 0.0;
        phase_fence();
        int reached = L;   // the last position whose row was written
        for (int i = 0; i < L; ++i) {
            const double* cur = R + int64_t(i & 1) * N;
            double* nxt = R + int64_t((i + 1) & 1) * N;
            const int cb = live_begin(i + 1), ce = live_end(i + 1);
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
            for (int k = live_begin(L) + lane; k < live_end(L); k += kWave) {
                const int S = live_node(L, k);
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
        // wave argmax, ties to the lowest k (a lane without a candidate holds -inf, INT_MAX)
        for (int d = kWave / 2; d >= 1; d >>= 1) {
            const double ov = __shfl_xor(bv, d);
            const int ok = __shfl_xor(bk, d);
            const int ox = __shfl_xor(bx, d);
            if (ov > bv || (ov == bv && ok < bk)) {
                bv = ov;
                bk = ok;
                bx = ox;
            }
        }
        phase_fence();
        if (lane == 0) {
            int32_t* out = a.path + o0 + s;
            bool ok = bx >= 0;
            if (ok) {
                out[L] = a.n_edges + bx;
                int k = bk;
                for (int i = L; i >= 1; --i) {
                    const int cb = live_begin(i);
                    const int e = BP[int64_t(i - 1) * a.max_dst + (k - cb)];
                    if (e < 0) {   // (a node on the best path always has a winning in-edge)
                        ok = false;
                        break;
                    }
                    out[i - 1] = W.e_g[e];
                    if (i >= 2) {   // the source's entry among the destinations of byte c_{i-2} (ascending nodes)
                        const int src = W.e_src[e];
                        int lo = live_begin(i - 1), hi = live_end(i - 1) - 1;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (W.dst[mid] < src) lo = mid + 1;
                            else hi = mid;
                        }
                        k = lo;
                    }
                }
            }
            a.best[s] = ok ? bv : -INFINITY;
            if (!ok) out[0] = -1;
        }
    }
}

}  // namespace

hipError_t launch_best_paths(const BestPathArgs& a, int grid, int waves, hipStream_t stream) {
    if (grid < 1 || waves < 1 || waves > kBestWavesPerBlock) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.ctr, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    const int64_t n = int64_t(a.n_edges) + a.n_end;
    if (n > 0) {
        const int blocks = int(n / 256 < 1 ? 1 : (n / 256 > 4096 ? 4096 : n / 256));
        hipLaunchKernelGGL(best_edge_weight_kernel, dim3(unsigned(blocks)), dim3(256), 0, stream, a);
    }
    if (a.n_strings > 0)
        hipLaunchKernelGGL(best_path_kernel, dim3(unsigned(grid)), dim3(unsigned(waves * kWave)), 0, stream, a);
    return hipGetLastError();
}

}  // namespace wfsa

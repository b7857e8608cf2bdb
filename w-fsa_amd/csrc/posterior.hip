// The log-sum-exp trellis pass with stored rows, the backward pass over node
// posteriors and the row scan (posterior.hpp).
#include "posterior.hpp"

#include "decode_device.hpp"

namespace wfsa {

namespace {

// Fixed-point words (fb_kernels.hip's fix_of, restated): a value rounded once
// to a multiple of 2^-frac.  The gamma and count rows are read, added to and
// reset with agent-scope atomics only, so every access meets the others in L2.
__device__ __forceinline__ unsigned long long fix_of(double v, int frac) { return (unsigned long long)rint(ldexp(v, frac)); }
__device__ __forceinline__ unsigned long long fix_add(unsigned long long* p, unsigned long long v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long fix_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fix_store(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the same bits on every lane: a + b is commutative, so both partners of a step form the same sum
__device__ __forceinline__ double wave_sum(double v) {
    for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(kDecodeWavesPerBlock* kWave) void posterior_counts_kernel(PosteriorArgs a) {
    const DecodeArgs& d = a.d;
    const WideModel& W = d.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = d.n_nodes;
    const int NP = a.n_params;
    const int F = a.count_frac;
    double* R = d.score + gw * (2 * int64_t(N));
    double* H = a.hist + gw * (int64_t(d.max_len > 0 ? d.max_len : 1) * int64_t(d.max_dst > 0 ? d.max_dst : 1));
    unsigned long long* G = a.gamma + gw * (2 * int64_t(N));
    unsigned long long* C = a.count + gw * int64_t(NP > 0 ? NP : 1);
    // the score rows hold -inf and the gamma and count rows 0 outside what a
    // string uses: set once, restored behind every position / by the row scan
    for (int k = lane; k < 2 * N; k += kWave) {
        R[k] = -INFINITY;
        fix_store(G + k, 0ull);
    }
    for (int j = lane; j < NP; j += kWave) fix_store(C + j, 0ull);
    phase_fence();
    for (;;) {
        const int s = next_string(d.ctr, lane);
        if (s < 0 || s >= d.n_strings) break;
        const int64_t o0 = d.off[s];
        const int L = int(d.off[s + 1] - o0);
        const LiveSet live{W, d.sym + o0, d.start};
        auto clear_row = [&](int j) {
            double* row = R + int64_t(j & 1) * N;
            for (int k = live.begin(j) + lane; k < live.end(j); k += kWave) row[live.node(j, k)] = -INFINITY;
        };
        if (lane == 0) R[d.start] = 0.0;
        phase_fence();
        bool alive = true;
        for (int i = 0; i < L; ++i) {
            const double* cur = R + int64_t(i & 1) * N;
            double* nxt = R + int64_t((i + 1) & 1) * N;
            const int cb = live.begin(i + 1), ce = live.end(i + 1);
            double* h = H + int64_t(i) * d.max_dst;
            bool any = false;
            for (int k = cb + lane; k < ce; k += kWave) {
                // log alpha of the destination: the greatest term, then the sum of the terms over it in e_ptr order
                const int e0 = W.e_ptr[k], e1 = W.e_ptr[k + 1];
                double mx = -INFINITY;
                for (int e = e0; e < e1; ++e) {
                    const double v = cur[W.e_src[e]] + d.lw[W.e_g[e]];
                    mx = v > mx ? v : mx;
                }
                double t = -INFINITY;
                if (mx > -INFINITY) {
                    double sum = 0.0;
                    for (int e = e0; e < e1; ++e) sum += exp(cur[W.e_src[e]] + d.lw[W.e_g[e]] - mx);
                    t = mx + log(sum);
                    any = true;
                }
                nxt[W.dst[k]] = t;
                h[k - cb] = t;
            }
            phase_fence();
            clear_row(i);
            phase_fence();
            if (!__any(any ? 1 : 0)) {   // nothing reachable: row i + 1 is all -inf already
                alive = false;
                break;
            }
        }
        if (alive) clear_row(L);   // (the backward pass reads the stored rows, not R)
        phase_fence();
        // log q over the end edges in (live slot, end edge) order, as the
        // sampler's lane 0 forms it; every lane forms the same value
        const int lb = live.begin(L), le = live.end(L);
        const double* hl = H + int64_t(L >= 1 ? L - 1 : 0) * d.max_dst;   // row L by slot (L >= 1)
        double mx = -INFINITY;
        if (alive)
            for (int k = lb; k < le; ++k) {
                const int S = live.node(L, k);
                const double av = L >= 1 ? hl[k - lb] : 0.0;
                for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) {
                    const double v = av + d.lw[d.n_edges + x];
                    mx = v > mx ? v : mx;
                }
            }
        const bool has = mx > -INFINITY;
        double lq = -INFINITY;
        if (has) {
            double total = 0.0;
            for (int k = lb; k < le; ++k) {
                const int S = live.node(L, k);
                const double av = L >= 1 ? hl[k - lb] : 0.0;
                for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) total += exp(av + d.lw[d.n_edges + x] - mx);
            }
            lq = mx + log(total);
        }
        double ent = 0.0;   // this lane's share of the entropy
        int fresh = 0;      // counts this lane's add found at 0
        // mass m > 0 on combined edge g: to the count of every parameter of its list
        auto count_edge = [&](int g, double m) {
            const unsigned long long iv = fix_of(m, F);
            if (iv == 0ull) return;
            for (int q = d.pptr[g]; q < d.pptr[g + 1]; ++q) fresh += fix_add(C + d.pidx[q], iv) == 0ull ? 1 : 0;
        };
        if (has && a.phases >= 2) {
            // position L: the end edges of the live nodes, lanes over the slots
            for (int k = lb + lane; k < le; k += kWave) {
                const int S = live.node(L, k);
                const double av = L >= 1 ? hl[k - lb] : 0.0;
                unsigned long long g = 0ull;
                for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) {
                    const double t = av + d.lw[d.n_edges + x];
                    if (!(t > -INFINITY)) continue;
                    const double dd = fmin(t - lq, 0.0);
                    const double m = exp(dd);
                    if (!(m > 0.0)) continue;
                    ent -= m * dd;
                    g += fix_of(m, kPosteriorGammaFrac);
                    count_edge(d.n_edges + x, m);
                }
                if (L >= 1 && g != 0ull) fix_store(G + int64_t(L & 1) * N + S, g);
            }
            phase_fence();
            for (int i = L; i >= 1; --i) {
                unsigned long long* gi = G + int64_t(i & 1) * N;
                unsigned long long* gp = G + int64_t((i - 1) & 1) * N;
                const int cb = live.begin(i), ce = live.end(i);
                const double* hi = H + int64_t(i - 1) * d.max_dst;                  // row i by slot
                const double* hp = H + int64_t(i >= 2 ? i - 2 : 0) * d.max_dst;     // row i - 1 by slot (i >= 2)
                const int sb = live.begin(i - 1);
                for (int k = cb + lane; k < ce; k += kWave) {
                    const unsigned long long g = fix_load(gi + W.dst[k]);
                    if (g == 0ull) continue;
                    const double gam = ldexp(double(g), -kPosteriorGammaFrac);
                    const double la = hi[k - cb];
                    for (int e = W.e_ptr[k]; e < W.e_ptr[k + 1]; ++e) {
                        const int src = W.e_src[e];
                        double las;   // log alpha of the source at position i - 1
                        if (i < 2) {
                            las = src == d.start ? 0.0 : -INFINITY;
                        } else {
                            const int ks = live.slot_of(i - 1, src);   // its entry among the destinations of byte c_{i-2}, if it is one
                            las = W.dst[ks] == src ? hp[ks - sb] : -INFINITY;
                        }
                        const int eg = W.e_g[e];
                        const double t = las + d.lw[eg];
                        if (!(t > -INFINITY)) continue;
                        const double dd = fmin(t - la, 0.0);
                        const double m = gam * exp(dd);
                        if (!(m > 0.0)) continue;
                        ent -= m * dd;
                        if (i >= 2) {
                            const unsigned long long iv = fix_of(m, kPosteriorGammaFrac);
                            if (iv != 0ull) fix_add(gp + src, iv);
                        }
                        count_edge(eg, m);
                    }
                }
                phase_fence();
                for (int k = cb + lane; k < ce; k += kWave) fix_store(gi + W.dst[k], 0ull);
                phase_fence();
            }
        }
        ent = wave_sum(ent);
        const int nnz = wave_sum(fresh);
        // room for the row: every lane runs the add (lane 0 adds the row's
        // length, the rest nothing), as next_string takes its ticket
        __builtin_amdgcn_wave_barrier();
        const unsigned long long got = fix_add(a.cursor, lane == 0 ? (unsigned long long)nnz : 0ull);
        const int64_t start = int64_t(__builtin_amdgcn_readfirstlane(unsigned(got))) |
                              (int64_t(__builtin_amdgcn_readfirstlane(unsigned(got >> 32))) << 32);
        const bool fits = start + nnz <= a.capacity;
        if (lane == 0) {
            a.logq[s] = lq;
            a.entropy[s] = has ? ent : __builtin_nan("");
            a.row_start[s] = start;
            a.row_len[s] = fits ? nnz : 0;
            if (!fits) fix_store(a.cursor + 1, 1ull);
        }
        if (a.phases >= 3 && nnz > 0) {
            // the non-zero counts in ascending id: a ballot per round of 64 ids
            // and each lane's rank among the round's set bits
            int64_t at = start;
            for (int j0 = 0; j0 < NP; j0 += kWave) {
                const int j = j0 + lane;
                const unsigned long long v = j < NP ? fix_load(C + j) : 0ull;
                const unsigned long long mask = __ballot(v != 0ull ? 1 : 0);
                if (v != 0ull) {
                    const int64_t p = at + __popcll(mask & ((1ull << lane) - 1ull));
                    if (fits && p < start + nnz) {
                        a.out_idx[p] = j;
                        a.out_val[p] = ldexp(double(v), -F);
                    }
                    fix_store(C + j, 0ull);
                }
                at += __popcll(mask);
            }
            phase_fence();
        }
    }
}

}  // namespace

hipError_t launch_posterior_counts(const PosteriorArgs& a, int grid, int waves, hipStream_t stream) {
    if (grid < 1 || waves < 1 || waves > kDecodeWavesPerBlock || a.phases < 1 || a.phases > 3 || a.count_frac < 0 ||
        a.count_frac > kPosteriorGammaFrac)
        return hipErrorInvalidValue;
    if (hipError_t e = launch_edge_weights(a.d, stream); e != hipSuccess) return e;
    if (hipError_t e = hipMemsetAsync(a.cursor, 0, 2 * sizeof(unsigned long long), stream); e != hipSuccess) return e;
    if (a.d.n_strings > 0) hipLaunchKernelGGL(posterior_counts_kernel, dim3(unsigned(grid)), dim3(unsigned(waves * kWave)), 0, stream, a);
    return hipGetLastError();
}

}  // namespace wfsa

// The log-sum-exp trellis pass with stored rows, the backward pass over node
// posteriors folded into per-byte state sums, and the (max, +) pass over those
// sums (marginals.hpp).
#include "marginals.hpp"

#include <algorithm>
#include <climits>
#include <numeric>

#include "decode_device.hpp"

namespace wfsa {

namespace {

constexpr unsigned long long kOneFix = 1ull << kMarginalFrac;   // 1.0 in fixed point

// Fixed-point words (posterior.hip's, restated): a value rounded once to a
// multiple of 2^-62.  The gamma rows are read, added to and reset with
// agent-scope atomics only, so every access meets the others in L2.
__device__ __forceinline__ unsigned long long fix_of(double v) { return (unsigned long long)rint(ldexp(v, kMarginalFrac)); }
__device__ __forceinline__ unsigned long long fix_add(unsigned long long* p, unsigned long long v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long fix_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fix_store(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// integer addition: the same bits on every lane, whatever the order
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ bool finite_weight(double w) { return w > -INFINITY && w < INFINITY; }

// Wave arg-max by butterfly (decode.hip's, restated): every lane ends with the
// greatest v, among equal v the lowest key, and that lane's carry (a lane
// without a candidate offers -inf, INT_MAX).  Every lane runs every shuffle.
__device__ __forceinline__ void wave_argmax(double& v, int& key, int& carry) {
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(v, d);
        const int ok = __shfl_xor(key, d);
        const int oc = __shfl_xor(carry, d);
        if (ov > v || (ov == v && ok < key)) {
            v = ov;
            key = ok;
            carry = oc;
        }
    }
}

__global__ __launch_bounds__(kDecodeWavesPerBlock* kWave) void marginal_rows_kernel(MarginalArgs a) {
    const DecodeArgs& d = a.d;
    const WideModel& W = d.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = d.n_nodes;
    double* R = d.score + gw * (2 * int64_t(N));
    double* H = a.hist + gw * (int64_t(d.max_len > 0 ? d.max_len : 1) * int64_t(d.max_dst > 0 ? d.max_dst : 1));
    unsigned long long* G = a.gamma + gw * (2 * int64_t(N));
    // the score rows hold -inf and the gamma rows 0 outside what a string
    // uses: set once, restored behind every position
    for (int k = lane; k < 2 * N; k += kWave) {
        R[k] = -INFINITY;
        fix_store(G + k, 0ull);
    }
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
        // log q over the end edges in (live slot, end edge) order, as
        // posterior_counts_kernel forms it; every lane forms the same value
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
        if (lane == 0) a.logq[s] = lq;
        if (has) {
            // position L: the end edges of the live nodes, lanes over the slots
            for (int k = lb + lane; k < le; k += kWave) {
                const int S = live.node(L, k);
                const double av = L >= 1 ? hl[k - lb] : 0.0;
                unsigned long long g = 0ull;
                for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) {
                    const double t = av + d.lw[d.n_edges + x];
                    if (!(t > -INFINITY)) continue;
                    const double m = exp(fmin(t - lq, 0.0));
                    if (!(m > 0.0)) continue;
                    g += fix_of(m);
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
                // gamma_i is complete: its state sums, at the byte's fixed
                // address, and the mass on the nodes where an emission ends
                unsigned long long* mrow = a.mass + a.base[o0 + i - 1];
                unsigned long long ends = 0ull;
                for (int j = cb + lane; j < ce; j += kWave) {
                    const int node = W.dst[j];
                    if (node < a.n_states) ends += fix_load(gi + node);
                    const int len = a.seg[j];
                    if (len > 0) {   // the head of a segment of the (owner state, node) order
                        unsigned long long t = 0ull;
                        for (int q = 0; q < len; ++q) t += fix_load(gi + W.dst[a.ord[j + q]]);
                        mrow[a.grp[a.ord[j]]] = t > kOneFix ? kOneFix : t;
                    }
                }
                ends = wave_sum(ends);
                if (lane == 0) a.boundary[o0 + i - 1] = ldexp(double(ends > kOneFix ? kOneFix : ends), -kMarginalFrac);
                for (int k = cb + lane; k < ce; k += kWave) {
                    const unsigned long long g = fix_load(gi + W.dst[k]);
                    if (g == 0ull) continue;
                    const double gam = ldexp(double(g), -kMarginalFrac);
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
                        const double t = las + d.lw[W.e_g[e]];
                        if (!(t > -INFINITY)) continue;
                        const double m = gam * exp(fmin(t - la, 0.0));
                        if (!(m > 0.0)) continue;
                        if (i >= 2) {
                            const unsigned long long iv = fix_of(m);
                            if (iv != 0ull) fix_add(gp + src, iv);
                        }
                    }
                }
                phase_fence();
                for (int k = cb + lane; k < ce; k += kWave) fix_store(gi + W.dst[k], 0ull);
                phase_fence();
            }
        } else {
            // no path of finite weight: the string owns nothing (its state sums stay 0)
            for (int i = lane; i < L; i += kWave) a.boundary[o0 + i] = __builtin_nan("");
        }
    }
}

__global__ __launch_bounds__(kDecodeWavesPerBlock* kWave) void marginal_decode_kernel(MarginalArgs a) {
    const DecodeArgs& d = a.d;
    const WideModel& W = d.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = d.n_nodes;
    double* R = d.score + gw * decode_score_doubles(N, 1);
    int32_t* BP = d.back + gw * decode_back_ints(d.max_len, d.max_dst, 1);
    // both rows hold -inf outside the live nodes: set once, restored behind every position
    for (int k = lane; k < 2 * N; k += kWave) R[k] = -INFINITY;
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
        const bool has = a.logq[s] > -INFINITY;   // (marginal_rows_kernel's: the same on every lane)
        int reached = -1;   // the last position whose row was written
        if (has) {
            if (lane == 0) R[d.start] = 0.0;
            phase_fence();
            reached = L;
            for (int i = 0; i < L; ++i) {
                const double* cur = R + int64_t(i & 1) * N;
                double* nxt = R + int64_t((i + 1) & 1) * N;
                const int cb = live.begin(i + 1), ce = live.end(i + 1);
                int32_t* bp = BP + int64_t(i) * d.max_dst;
                const unsigned long long* mrow = a.mass + a.base[o0 + i];   // the state sums of byte i + 1
                bool any = false;
                for (int k = cb + lane; k < ce; k += kWave) {
                    double bs = -INFINITY, bw = -INFINITY;
                    int be = -1;
                    for (int e = W.e_ptr[k]; e < W.e_ptr[k + 1]; ++e) {
                        const double sv = cur[W.e_src[e]];
                        const double w = d.lw[W.e_g[e]];
                        if (!(sv > -INFINITY) || !finite_weight(w)) continue;
                        if (sv > bs || (sv == bs && w > bw)) {   // strict: the first in-edge keeps a full tie
                            bs = sv;
                            bw = w;
                            be = e;
                        }
                    }
                    // the best eligible source plus the node's own reward: one add per position
                    nxt[W.dst[k]] = be >= 0 ? bs + ldexp(double(mrow[a.grp[k]]), -kMarginalFrac) : -INFINITY;
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
        }
        // the live nodes at position L that have a finite end edge
        double bv = -INFINITY;
        int bk = INT_MAX, bx = -1;
        if (reached == L) {
            const double* row = R + int64_t(L & 1) * N;
            for (int k = live.begin(L) + lane; k < live.end(L); k += kWave) {
                const int S = live.node(L, k);
                const double sc = row[S];
                if (!(sc > -INFINITY)) continue;
                double xw = -INFINITY;
                int x1 = -1;
                for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) {
                    const double w = d.lw[d.n_edges + x];
                    if (finite_weight(w) && w > xw) {   // strict: the first end edge keeps a tie
                        xw = w;
                        x1 = x;
                    }
                }
                if (x1 >= 0 && sc > bv) {   // a lane's k ascend: the lowest node keeps a tie
                    bv = sc;
                    bk = k;
                    bx = x1;
                }
            }
            phase_fence();
            clear_row(L);
        }
        wave_argmax(bv, bk, bx);   // ties to the lowest slot k
        phase_fence();
        if (lane == 0) {
            int32_t* out = d.path + o0 + s;
            bool ok = bx >= 0;
            if (ok) {
                out[L] = d.n_edges + bx;
                int k = bk;
                for (int i = L; i >= 1; --i) {
                    const int e = BP[int64_t(i - 1) * d.max_dst + (k - live.begin(i))];
                    if (e < 0) {   // (a node on the path always has a winning in-edge)
                        ok = false;
                        break;
                    }
                    out[i - 1] = W.e_g[e];
                    if (i >= 2) k = live.slot_of(i - 1, W.e_src[e]);   // the source's entry among the destinations of byte c_{i-2}
                }
            }
            double lw_sum = 0.0;   // the decoders' weight of the path: lw left to right from 0
            if (ok)
                for (int i = 0; i <= L; ++i) lw_sum += d.lw[out[i]];
            d.best[s] = ok ? lw_sum : -INFINITY;
            a.mea_score[s] = ok ? bv : __builtin_nan("");
            if (!ok) out[0] = -1;
        }
    }
}

}  // namespace

MarginalTables build_marginal_tables(const std::vector<int32_t>& c_ptr, const std::vector<int32_t>& dst, const std::vector<int32_t>& owner) {
    MarginalTables t;
    const size_t n_slots = size_t(c_ptr[256]);
    t.ord.assign(n_slots, 0);
    t.seg.assign(n_slots, 0);
    t.grp.assign(n_slots, 0);
    t.g_ptr.assign(257, 0);
    for (int c = 0; c < 256; ++c) {
        const int32_t b = c_ptr[size_t(c)], e = c_ptr[size_t(c) + 1];
        std::iota(t.ord.begin() + b, t.ord.begin() + e, b);
        std::sort(t.ord.begin() + b, t.ord.begin() + e, [&](int32_t x, int32_t y) {
            const int32_t ox = owner[size_t(dst[size_t(x)])], oy = owner[size_t(dst[size_t(y)])];
            return ox != oy ? ox < oy : dst[size_t(x)] < dst[size_t(y)];
        });
        int32_t groups = 0;
        for (int32_t j = b; j < e;) {
            const int32_t own = owner[size_t(dst[size_t(t.ord[size_t(j)])])];
            int32_t j1 = j;
            while (j1 < e && owner[size_t(dst[size_t(t.ord[size_t(j1)])])] == own) t.grp[size_t(t.ord[size_t(j1++)])] = groups;
            t.seg[size_t(j)] = j1 - j;
            t.g_state.push_back(own);
            ++groups;
            j = j1;
        }
        t.g_ptr[size_t(c) + 1] = t.g_ptr[size_t(c)] + groups;
    }
    return t;
}

hipError_t launch_marginal_rows(const MarginalArgs& a, int64_t n_mass, int grid, int waves, hipStream_t stream) {
    if (grid < 1 || waves < 1 || waves > kDecodeWavesPerBlock || n_mass < 0) return hipErrorInvalidValue;
    if (hipError_t e = launch_edge_weights(a.d, stream); e != hipSuccess) return e;
    if (n_mass > 0)
        if (hipError_t e = hipMemsetAsync(a.mass, 0, size_t(n_mass) * sizeof(unsigned long long), stream); e != hipSuccess) return e;
    if (a.d.n_strings > 0) hipLaunchKernelGGL(marginal_rows_kernel, dim3(unsigned(grid)), dim3(unsigned(waves * kWave)), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_marginal_decode(const MarginalArgs& a, int grid, int waves, hipStream_t stream) {
    if (grid < 1 || waves < 1 || waves > kDecodeWavesPerBlock) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(a.d.ctr, 0, sizeof(unsigned), stream); e != hipSuccess) return e;
    if (a.d.n_strings > 0) hipLaunchKernelGGL(marginal_decode_kernel, dim3(unsigned(grid)), dim3(unsigned(waves * kWave)), 0, stream, a);
    return hipGetLastError();
}

}  // namespace wfsa

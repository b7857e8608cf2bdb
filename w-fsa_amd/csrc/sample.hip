// The log-sum-exp trellis pass with stored rows and the sampling walks (sample.hpp).
#include "sample.hpp"

#include "decode_device.hpp"

namespace wfsa {

namespace {

__global__ __launch_bounds__(256) void sample_uniforms_kernel(uint64_t seed, uint64_t string, uint32_t sample, int32_t n_draws, double* out) {
    const int64_t d = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (d < n_draws) out[d] = sample_uniform(seed, string, sample, uint32_t(d));
}

// Lanes 0 .. n-1 of a wave walk one sample each; the rest of the kernel is the
// decoders' wave-per-string pass with log-sum-exp in place of max.
__global__ __launch_bounds__(kDecodeWavesPerBlock* kWave) void sample_path_kernel(SampleArgs a) {
    const DecodeArgs& d = a.d;
    const WideModel& W = d.w;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t gw = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kWave;
    const int N = d.n_nodes;
    const int n = d.k;   // samples per string
    double* R = d.score + gw * sample_score_doubles(N);
    double* H = a.hist + gw * sample_hist_doubles(d.max_len, d.max_dst);
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
        if (alive) clear_row(L);   // (the walks read the stored rows, not R)
        phase_fence();
        if (lane < n) {   // one lane per sample
            const LiveSet walk{W, d.sym + o0, d.start};
            int32_t* out = d.path + (o0 + s) * int64_t(n) + int64_t(lane) * (L + 1);
            const int lb = walk.begin(L), le = walk.end(L);
            const double* hl = H + int64_t(L >= 1 ? L - 1 : 0) * d.max_dst;   // row L by slot (L >= 1)
            // The end edges in (live slot, end edge) order: the greatest term,
            // then the masses over it and their sum.  Every walking lane forms
            // the same values, whatever n is.
            double mx = -INFINITY;
            if (alive)
                for (int k = lb; k < le; ++k) {
                    const int S = walk.node(L, k);
                    const double av = L >= 1 ? hl[k - lb] : 0.0;
                    for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) {
                        const double v = av + d.lw[d.n_edges + x];
                        mx = v > mx ? v : mx;
                    }
                }
            const bool has = mx > -INFINITY;
            bool ok = has;
            if (has) {
                double total = 0.0;
                for (int k = lb; k < le; ++k) {
                    const int S = walk.node(L, k);
                    const double av = L >= 1 ? hl[k - lb] : 0.0;
                    for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) total += exp(av + d.lw[d.n_edges + x] - mx);
                }
                if (lane == 0) a.logq[s] = mx + log(total);
                const uint64_t sid = uint64_t(uint32_t(s));
                // the end choice
                double target = sample_uniform(a.seed, sid, uint32_t(lane), 0u) * total;
                double c = 0.0;
                int k = -1, bx = -1;
                for (int kk = lb; kk < le; ++kk) {
                    const int S = walk.node(L, kk);
                    const double av = L >= 1 ? hl[kk - lb] : 0.0;
                    for (int x = d.x_ptr[S]; x < d.x_ptr[S + 1]; ++x) {
                        const double m = exp(av + d.lw[d.n_edges + x] - mx);
                        c += m;
                        if (m > 0.0) {
                            k = kk;
                            bx = x;
                        }
                        if (c > target) break;
                    }
                    if (c > target) break;
                }
                ok = bx >= 0;
                if (ok) out[L] = d.n_edges + bx;
                // the in-edge into position i, i = L .. 1 (draw L + 1 - i): masses
                // exp(log alpha[src] + lw - log alpha[node]), their sum in e_ptr
                // order, then the choice
                for (int i = L; ok && i >= 1; --i) {
                    const double la = H[int64_t(i - 1) * d.max_dst + (k - walk.begin(i))];
                    const double* hp = H + int64_t(i >= 2 ? i - 2 : 0) * d.max_dst;   // row i - 1 by slot (i >= 2)
                    const int sb = walk.begin(i - 1);
                    const int e0 = W.e_ptr[k], e1 = W.e_ptr[k + 1];
                    // log alpha of in-edge e's source and the source's slot at position i - 1
                    auto source = [&](int e, int& ks) -> double {
                        const int src = W.e_src[e];
                        if (i < 2) {
                            ks = 0;
                            return src == d.start ? 0.0 : -INFINITY;
                        }
                        ks = walk.slot_of(i - 1, src);   // its entry among the destinations of byte c_{i-2}, if it is one
                        return W.dst[ks] == src ? hp[ks - sb] : -INFINITY;
                    };
                    total = 0.0;
                    for (int e = e0; e < e1; ++e) {
                        int ks;
                        total += exp(source(e, ks) + d.lw[W.e_g[e]] - la);
                    }
                    target = sample_uniform(a.seed, sid, uint32_t(lane), uint32_t(L + 1 - i)) * total;
                    c = 0.0;
                    int be = -1, bk = 0;
                    for (int e = e0; e < e1; ++e) {
                        int ks;
                        const double m = exp(source(e, ks) + d.lw[W.e_g[e]] - la);
                        c += m;
                        if (m > 0.0) {
                            be = e;
                            bk = ks;
                        }
                        if (c > target) break;
                    }
                    ok = be >= 0;
                    if (ok) {
                        out[i - 1] = W.e_g[be];
                        k = bk;
                    }
                }
            } else if (lane == 0) {
                a.logq[s] = -INFINITY;
            }
            // the path's weight as the decoders form it: one left-to-right sum
            double v = 0.0;
            if (ok)
                for (int t = 0; t <= L; ++t) v += d.lw[out[t]];
            d.best[int64_t(s) * n + lane] = ok ? v : -INFINITY;
            if (!ok) out[0] = -1;
        }
    }
}

}  // namespace

hipError_t launch_sample_paths(const SampleArgs& a, int grid, int waves, hipStream_t stream) {
    if (grid < 1 || waves < 1 || waves > kDecodeWavesPerBlock || a.d.k < 1 || a.d.k > kSampleMax) return hipErrorInvalidValue;
    if (hipError_t e = launch_edge_weights(a.d, stream); e != hipSuccess) return e;
    if (a.d.n_strings > 0) hipLaunchKernelGGL(sample_path_kernel, dim3(unsigned(grid)), dim3(unsigned(waves * kWave)), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_sample_uniforms(uint64_t seed, uint64_t string, uint32_t sample, int32_t n_draws, double* out, hipStream_t stream) {
    if (n_draws < 0) return hipErrorInvalidValue;
    if (n_draws > 0)
        hipLaunchKernelGGL(sample_uniforms_kernel, dim3(unsigned((n_draws + 255) / 256)), dim3(256), 0, stream, seed, string, sample, n_draws,
                           out);
    return hipGetLastError();
}

}  // namespace wfsa

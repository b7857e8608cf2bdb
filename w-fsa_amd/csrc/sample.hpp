// Posterior path sampling on the device (wfsa_dev_sample_paths): n independent
// draws per loaded string from P(path | string) = exp(w(path)) / q_s.
//
// It is decode.hpp's trellis walk over (log-sum-exp, +) in place of (max, +).
// One wavefront per string runs the forward pass over the in-edges-by-byte
// lists (WideModel): lanes run over the destinations of byte c_i, and each
// forms its destination's log alpha from the terms log alpha[src] + lw[edge]
// over its in-edges -- the greatest term, then the sum of exp(term - greatest)
// in e_ptr order -- with lw the decoders' edge log-weights.  Every node's value
// is relative to its own greatest term, so neither a q_s below the double range
// nor a prefix far below another one at the same position loses anything: a
// string with an accepting path of finite weight always has positive mass.
// The rows are kept per (position, destination slot) where the decoders keep
// back-pointers.  Then lanes 0 .. n-1 walk one sample each from the end: the
// end edge among the end edges of the live nodes, then per position an in-edge
// of the current node, each by inverse CDF with one Philox draw.
//
// Choice rule: among candidates of masses a_i >= 0 the first whose running sum
// exceeds u * total, total their sum in the same order; when rounding leaves
// none, the last of positive mass.  In-edges are candidates in e_ptr order with
// a = exp(log alpha[src] + lw[edge] - log alpha[node]); end edges in (live
// slot, end edge) order with a = exp(log alpha[node] + lw[end edge] - greatest
// such term).  A candidate of mass 0 (an edge of weight -inf, a prefix of mass
// 0) is never taken.  log q is the greatest end term plus the log of that sum.
//
// A sample's weight is one left-to-right sum of lw over its edges, which is
// how the decoders form it: a sampled path carries the bits kbest_paths
// reports for it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "decode.hpp"

namespace wfsa {

constexpr int kSampleMax = 64;   // WFSA_SAMPLE_MAX: one walking lane per sample

struct SampleArgs {
    // The model, the strings, wt / lw, ctr and the outputs as the decoders use
    // them, with k = n samples per string: best[s][t] = the weight of sample t,
    // path as for K-best (first entry -1: the walk failed).  score: per wave
    // two node-indexed rows of n_nodes log alphas, -inf outside the live nodes;
    // back is not used.
    DecodeArgs d;
    double* hist;      // per wave [max_len][max_dst]: row i + 1 by destination slot
    double* logq;      // [n_strings] log q_s; -inf: no path of finite weight, no samples
    uint64_t seed;
};

__host__ __device__ inline int64_t sample_score_doubles(int32_t n_nodes) { return 2 * int64_t(n_nodes); }
__host__ __device__ inline int64_t sample_hist_doubles(int32_t max_len, int32_t max_dst) {
    return int64_t(max_len > 0 ? max_len : 1) * int64_t(max_dst > 0 ? max_dst : 1);
}
inline int64_t sample_wave_bytes(int32_t max_len, int32_t n_nodes, int32_t max_dst) {
    return 8 * (sample_score_doubles(n_nodes) + sample_hist_doubles(max_len, max_dst));
}

// Philox4x32-10 (Salmon et al., SC'11): counter c, key k -> four words.
struct Philox4 {
    uint32_t x[4];
};
__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
        c1 = uint32_t(p1);
        c3 = uint32_t(p0);
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// The uniform of draw d of sample t of string s: key (lo32(seed), hi32(seed)),
// counter (lo32(s), hi32(s), t, d); u = the top 53 bits of words 0 and 1,
// in [0, 1).
__host__ __device__ inline double sample_uniform(uint64_t seed, uint64_t s, uint32_t t, uint32_t d) {
    const Philox4 r = philox4x32_10(uint32_t(s), uint32_t(s >> 32), t, d, uint32_t(seed), uint32_t(seed >> 32));
    return double(((uint64_t(r.x[0]) << 32) | r.x[1]) >> 11) * 0x1.0p-53;
}

// grid blocks of `waves` wavefronts (1 .. kDecodeWavesPerBlock): the counter
// reset and the edge log-weights (launch_edge_weights), then the sampler
hipError_t launch_sample_paths(const SampleArgs& a, int grid, int waves, hipStream_t stream);
// out[d] = sample_uniform(seed, string, sample, d), d < n_draws, on the device
hipError_t launch_sample_uniforms(uint64_t seed, uint64_t string, uint32_t sample, int32_t n_draws, double* out, hipStream_t stream);

}  // namespace wfsa

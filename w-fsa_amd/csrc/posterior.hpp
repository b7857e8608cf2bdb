// Posterior expected counts on the device (wfsa_dev_posterior_counts): for
// every loaded string its log q, the entropy of its path posterior
// P(path | string) = exp(w(path)) / q_s and the sparse row of expected
// parameter counts E_s[count] -- the per-string E-step.
//
// Forward pass.  sample.hpp's, restated: one wavefront per string, lanes over
// the destinations of byte c_i, each forms its destination's log alpha from the
// terms log alpha[src] + lw[edge] over its in-edges -- the greatest term, then
// the sum of exp(term - greatest) in e_ptr order -- with lw the decoders' edge
// log-weights, and the rows are kept per (position, destination slot).  log q
// is the greatest end term plus the log of the sum of exp(term - greatest) over
// the end edges in (live slot, end edge) order: sample_paths' log q bit for bit.
//
// Backward pass, in the linear domain on node posteriors, position L down to 1.
// At L a live node k has gamma_L[k] = sum over its end edges x of
// exp(log alpha_L[k] + lw[E + x] - log q), and each end edge's mass goes to that
// edge's parameters.  At position i the lane that owns destination slot k gives
// every in-edge e the mass
//     m_e = gamma_i[k] * exp(log alpha_{i-1}[src] + lw[e] - log alpha_i[k])
// (the sampler's conditional: its exponent is <= 0 and is clamped there, so
// neither a q_s below the double range nor rounding can lift a mass over its
// node's); the source's log alpha is read at its slot (slot_of), and m_e is
// added to gamma_{i-1}[src] and to the count of every parameter on the edge's
// list, once per occurrence.  A mass of 0 -- an edge at -inf, a source of mass
// 0, a product that underflows -- is skipped: 0 * -inf is never formed.
//
// Fixed point.  Several lanes of the wave can aim both adds at one word, so
// each mass is rounded ONCE to a multiple of 2^-frac and added with a 64-bit
// integer atomic (integer addition is associative: the bits do not depend on
// the order of arrival).  Node posteriors are <= 1: kPosteriorGammaFrac = 62
// fraction bits.  A count is bounded by B = (max_len + 1) x the longest edge
// parameter list; posterior_count_frac(B) = 62 - ceil(log2 B) fraction bits keep
// B x 2^frac <= 2^62 (at B = 1: 62 bits; at B = 258, strings of up to 128
// bytes and lists of two: 53 bits, 1.1e-16).
// A mass below half a unit of its word rounds to 0 and is not added; a
// parameter is "listed" when its accumulated fixed-point count is not 0, and
// its value is that integer times 2^-frac, converted to double once.
//
// Entropy by the chain rule: -sum m_e * (the exponent above) over every in-edge
// taken and likewise over the end edges against log q -- a sum of non-negative
// terms, each lane's in (position descending, slot, in-edge) order, then a
// butterfly sum over the wave (every lane the same bits).
//
// The row.  After position 1 the wave scans its n_params counts lane-strided,
// compacts the non-zero ones with a ballot and a prefix count in ascending
// parameter id, converts them and zeroes them.  Room in the output comes from
// an atomic cursor -- the number of non-zero counts is known before the scan:
// the lane whose add found the word at 0 counted it -- and each string's start
// and length are recorded; the host puts the rows into string order.  A row
// that does not fit `capacity` is counted, not written, and flagged: the cursor
// still ends at the entries all rows need, and the host launches once more at
// that size.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "decode.hpp"

namespace wfsa {

constexpr int kPosteriorGammaFrac = 62;   // node posteriors are <= 1

// fraction bits of a count bounded by `bound` = (max_len + 1) x the longest
// edge parameter list: bound x 2^frac <= 2^62
inline int posterior_count_frac(int64_t bound) {
    int bits = 0;
    while ((int64_t(1) << bits) < bound && bits < 62) ++bits;
    return 62 - bits;
}

struct PosteriorArgs {
    // The model, the strings, wt / lw, ctr and score as the sampler uses them
    // (two node-indexed rows of log alphas per wave, -inf outside the live
    // nodes); k, back, best and path are not used.
    DecodeArgs d;
    double* hist;                 // per wave [max_len][max_dst]: row i + 1 by destination slot
    unsigned long long* gamma;    // per wave two node-indexed rows of node posteriors, 62 fraction bits, 0 outside the live nodes
    unsigned long long* count;    // per wave [n_params] expected counts, count_frac fraction bits, 0 between strings
    int32_t n_params;
    int32_t count_frac;
    int32_t phases;               // 3: everything; timing only: 1 the forward pass and log q alone, 2 no row scan
    double* logq;                 // [n_strings] log q_s; -inf: no path of finite weight
    double* entropy;              // [n_strings] nats; NaN where log q = -inf
    unsigned long long* cursor;   // [2]: entries handed out so far; non-zero: a row did not fit `capacity`
    int64_t capacity;             // entries of out_idx / out_val
    int64_t* row_start;           // [n_strings] where the string's row starts in out_idx / out_val
    int32_t* row_len;             // [n_strings] its entries
    int32_t* out_idx;             // parameter ids, ascending within a row
    double* out_val;
};

// scratch of one wave: the sampler's rows, the two gamma rows, the count row
inline int64_t posterior_wave_bytes(int32_t max_len, int32_t n_nodes, int32_t max_dst, int32_t n_params) {
    const int64_t hist = int64_t(max_len > 0 ? max_len : 1) * int64_t(max_dst > 0 ? max_dst : 1);
    return 8 * (2 * int64_t(n_nodes) + hist + 2 * int64_t(n_nodes) + int64_t(n_params > 0 ? n_params : 1));
}

// grid blocks of `waves` wavefronts (1 .. kDecodeWavesPerBlock): the counter
// reset and the edge log-weights (launch_edge_weights), the cursor at zero,
// then posterior_counts_kernel
hipError_t launch_posterior_counts(const PosteriorArgs& a, int grid, int waves, hipStream_t stream);

}  // namespace wfsa

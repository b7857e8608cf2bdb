// Per-byte state posteriors and the max-expected-accuracy decode on the device
// (wfsa_dev_byte_marginals).  For every loaded string, under
// P(path | string) = exp(w(path)) / q_s:
//   mass[s, i, U]  the posterior probability that byte i lies inside an
//                  emission of Fsa state U,
//   boundary[s, i] the posterior probability that an emission ends with byte i,
// and on request the accepting path of finite weight that maximises
// score = sum_i mass[s, i, state of the path at byte i] (MEA decode).
//
// In trellis terms (trellis_model.hpp): being at node k at position i means, for
// k < n_states, that an emission of state k ended with byte i, and for a chain
// node that byte i lies inside the multi-byte emission the chain spells, which
// belongs to the node's owner state (TrellisModel::owner).  So mass[s, i, U] is
// the sum of the node posteriors gamma_i over the nodes owned by U, and
// boundary[s, i] the sum over the nodes below n_states.
//
// marginal_rows_kernel.  posterior.hpp's forward pass and backward gamma
// recursion, restated line for line without the parameter counts, the count row
// and the row scan: one wavefront per string; log alpha is the greatest term
// plus the log of the sum of exp(term - greatest) in e_ptr order; log q runs over
// the end edges in (live slot, end edge) order (posterior_counts' log q byte for
// byte); in-edge e into node k at position i carries
//     m_e = gamma_i[k] * exp(min(0, log alpha_{i-1}[src] + lw[e] - log alpha_i[k])),
// each mass is rounded ONCE to a multiple of 2^-62 and added to gamma_{i-1}[src]
// with an agent-scope 64-bit integer atomic, and a mass of 0 is skipped (0 * -inf
// is never formed).  When the backward loop reaches position i, gamma_i is
// complete; before its reset the wave folds it into state sums.
//
// The fold.  The nodes live at position i are the destinations of byte c_{i-1}:
// the grouping of a byte's destination slots by owner state is a table of the
// model (MarginalTables, built when the model is loaded).  Per byte c the slots
// [c_ptr[c], c_ptr[c + 1]) are listed in (owner state, node) order; the lane at a
// segment head adds its segment's fixed-point words as integers -- exact, and
// independent of any order -- clamps the sum to 2^62 and stores it at
//     mass[base[off[s] + i - 1] + group index],
// where base is the prefix sum of n_groups[byte] over the corpus bytes (computed
// once per loaded corpus): a fixed address that depends on the corpus alone, so
// the bytes returned cannot depend on which wave took which string.  boundary is
// the integer wave sum of the words of the nodes below n_states, clamped to 2^62
// and converted once to a double.
//
// marginal_decode_kernel.  best_path_kernel's loop -- two node-indexed score
// rows and an int back-pointer per (position, slot) -- with a node reward in
// place of the edge weight: ldexp(double(word), -62) of the state sum of the
// slot's group, read where marginal_rows_kernel stored it.  An in-edge is
// eligible when its lw is finite and its source's score is above -inf; a
// destination's score is the best eligible source score plus its own reward (one
// add per position, left to right: the score is one fixed sum).  Ties, total:
//   in-edges by (source score descending, lw descending, e ascending);
//   at the end by (score descending, node ascending) over the live nodes that
//   have a finite end edge, then that node's end edges by (lw descending, end
//   edge ascending).
// (e and the end edge as decode.hpp defines them: within a destination's e_ptr
// range source node ascending, then the source's out-edge order; the scores
// compared are the sums of the state sums as stored, so two paths that tie in
// exact arithmetic are ordered by the stored words.)
// Lane 0 walks the back-pointers and writes the path's L + 1 combined edge ids,
// as the Viterbi decoder does, and forms the path's log weight as the decoders
// do: one left-to-right sum of lw, so the path carries bit for bit the weight
// kbest_paths reports for it.  A string whose log q is -inf has no path.
//
// The kernels read and write only the buffers named here -- nothing an
// evaluation, rmin, the QN loop, another decode or a captured graph touches.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "decode.hpp"

namespace wfsa {

constexpr int kMarginalFrac = 62;   // node posteriors and state sums are <= 1

// The grouping of every byte's destination slots by owner state.
struct MarginalTables {
    std::vector<int32_t> ord;      // [n_slots] per byte: its slots in (owner state, node) order
    std::vector<int32_t> seg;      // [n_slots] at a segment head of that order: the segment's length; else 0
    std::vector<int32_t> grp;      // [n_slots] by slot: the index of its owner among the byte's distinct owners
    std::vector<int32_t> g_ptr;    // [257] prefix sum of n_groups[c]
    std::vector<int32_t> g_state;  // [g_ptr[256]] the owner state of group g_ptr[c] + group index (ascending within a byte)
    int32_t n_groups(int c) const { return g_ptr[size_t(c) + 1] - g_ptr[size_t(c)]; }
};

// c_ptr[257] / dst[c_ptr[256]]: the destinations by byte (WideModel); owner[n_nodes]
MarginalTables build_marginal_tables(const std::vector<int32_t>& c_ptr, const std::vector<int32_t>& dst, const std::vector<int32_t>& owner);

struct MarginalArgs {
    // The model, the strings, wt / lw, ctr and score as the sampler uses them
    // (two node-indexed rows per wave, -inf outside the live nodes).  The decode
    // kernel also uses back (its back-pointers), best (the path's log weight) and
    // path (Viterbi layout); k is 1.
    DecodeArgs d;
    double* hist;                     // per wave [max_len][max_dst]: row i + 1 by destination slot
    unsigned long long* gamma;        // per wave two node-indexed rows of node posteriors, 62 fraction bits, 0 outside the live nodes
    int32_t n_states;                 // nodes below it are Fsa states
    const int32_t* ord;               // MarginalTables, on the device
    const int32_t* seg;
    const int32_t* grp;
    const int64_t* base;              // [total_symbols + 1] where each corpus byte's state sums start
    unsigned long long* mass;         // [base[total_symbols]] state sums, 62 fraction bits
    double* logq;                     // [n_strings] log q_s; -inf: no path of finite weight
    double* boundary;                 // [total_symbols]; NaN on the bytes of a string whose log q is -inf
    double* mea_score;                // [n_strings] the decode's score; NaN: no path
};

// scratch of one wave: the sampler's rows and the two gamma rows; with the
// decode, its back-pointers too (it reuses the score rows)
inline int64_t marginal_wave_bytes(int32_t max_len, int32_t n_nodes, int32_t max_dst, bool decode) {
    const int64_t hist = int64_t(max_len > 0 ? max_len : 1) * int64_t(max_dst > 0 ? max_dst : 1);
    return 8 * (4 * int64_t(n_nodes) + hist) + (decode ? 4 * hist : 0);
}

// grid blocks of `waves` wavefronts (1 .. kDecodeWavesPerBlock): the counter
// reset and the edge log-weights (launch_edge_weights), the mass buffer of
// `n_mass` words at zero, then marginal_rows_kernel
hipError_t launch_marginal_rows(const MarginalArgs& a, int64_t n_mass, int grid, int waves, hipStream_t stream);
// after launch_marginal_rows on the same stream: the counter at zero again,
// then marginal_decode_kernel
hipError_t launch_marginal_decode(const MarginalArgs& a, int grid, int waves, hipStream_t stream);

}  // namespace wfsa

// Decoding on the device: the most probable accepting path of every loaded
// string (Viterbi, wfsa_dev_best_paths) and its K most probable ones (K-best,
// wfsa_dev_kbest_paths).  One argument block, one scratch layout and one set
// of helpers serve both; k = 1 is the Viterbi decode.
//
// Viterbi.  A (max, +) pass in the log domain over the byte-step trellis, one
// wavefront per string, over the in-edges-by-byte lists (WideModel).  Position
// i + 1 is live only on the destinations of byte c_i; lanes run over those
// destinations, each takes the max over its in-edges of score[src] + lw(edge)
// and keeps the winning in-edge as its back-pointer.  After the last byte the
// wave takes the max over the end edges of the live nodes and one lane walks
// the back-pointers and writes the path's L + 1 combined edge ids.
//
// Ties: a destination keeps the first in-edge in e_ptr order; at the end the
// lowest source node wins, then its first end edge in x_ptr order.  An edge of
// weight -inf, or a source at -inf, never wins (every comparison is a strict
// "greater than" against -inf), so the result is deterministic and a string
// without a finite-weight accepting path reports -inf and no path.
//
// K-best.  The same scheme with lists in place of scalars: every live node
// holds its K best prefix scores in descending order; a lane merges, for its
// destination, the lists of its in-edges' sources (score[src][r] + lw(edge))
// into K register-held candidates and stores with each the back-pointer
// (in-edge, source rank).  After the last byte every lane forms its K best
// candidates over the end edges of its live nodes, the wave extracts the K
// best of those by K rounds of butterfly arg-max, and lanes 0 .. K-1 each walk
// one path back and write its L + 1 combined edge ids.
//
// The order on a node's paths is (weight descending, in-edge ascending, source
// rank ascending); at the end (weight descending, live slot ascending, end edge
// ascending, rank ascending).  "In-edge" is the index into w.e_src / w.e_g,
// which runs through the lists of all bytes; a destination's candidates all
// come from its own e_ptr range of one byte's list, so what decides is the
// order within that range: source node ascending, then the source's out-edge
// order (the table's stable sort by destination).  Nodes are numbered as the
// model description numbers its states (Fsa's container order, not the
// file's), the chain nodes behind them.  "End edge" is the index x of x_ptr,
// which runs through the nodes in ascending order, and the live slots ascend
// by node, so (live slot, end edge) is the end edges' own order.  A source
// rank is compared only behind an equal in-edge, i.e. within one source's list.
// The order is total and defined without reference to K,
// and a path's weight is one left-to-right sum, so the first j paths of a K
// result are the j result bit for bit, and the first path is the Viterbi
// decode's.  A lane therefore merges into a compile-time capacity KC >= K (2,
// 4, 8 or 16 register-held entries, statically indexed) and stores the first K.
//
// An edge of weight -inf, or a prefix at -inf, never enters a list (every
// insertion is a strict "greater than" against entries that start at -inf): a
// string with m < K finite-weight accepting paths gives m paths.
//
// Both decodes take their edge log-weights from one kernel (one sum, in list
// order), so the k = 1 weights agree bit for bit.
//
// The kernels read and write only the buffers named here: their own copy of
// the weights, their own edge log-weights, scratch, counter and outputs --
// nothing an evaluation, rmin, the QN loop, the other decode or a captured
// graph touches.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fb_kernels.hpp"

namespace wfsa {

constexpr int kDecodeWavesPerBlock = 4;
constexpr int kKBestMax = 16;          // the largest capacity (WFSA_KBEST_MAX)
constexpr int kKBestRankBits = 4;      // a K-best back-pointer is (in-edge << 4) | source rank
// in-edges (and end edges) a packed back-pointer can name
constexpr int64_t kKBestMaxEdges = int64_t(1) << (31 - kKBestRankBits);

struct DecodeArgs {
    WideModel w;             // in-edges by byte
    const int32_t* x_ptr;    // [n_nodes + 1] end edges by source node (ids relative to n_edges)
    const int32_t* pptr;     // [n_edges + n_end + 1] parameter list of each combined edge
    const int32_t* pidx;
    int32_t n_nodes;
    int32_t start;
    int32_t n_edges;         // byte-consuming edges E; end edge x has the combined id E + x
    int32_t n_end;
    const uint8_t* sym;
    const int64_t* off;
    int32_t n_strings;
    int32_t max_len;
    int32_t max_dst;         // the most destinations of one byte
    int32_t k;               // paths wanted per string: 1 for Viterbi, 1 .. the launched capacity for K-best
    const double* wt;        // [n_params + 1] weights (GetWeight form, zero slot last)
    double* lw;              // [n_edges + n_end] edge log-weights: the sum over the parameter list
    double* score;           // per wave: two rows of [n_nodes][k], descending, -inf outside the live lists
    int32_t* back;           // per wave: [max_len][max_dst][k]; Viterbi: the winning in-edge (index into
                             // w.e_src / w.e_g), K-best: packed (in-edge, source rank); -1: none
    unsigned* ctr;           // work counter: the next string (zero before the launch)
    double* best;            // [n_strings][k] log weights, descending, -inf past the string's last path
    int32_t* path;           // string s, rank t: L + 1 combined edge ids at (off[s] + s) * k + t * (L + 1)
                             // (Viterbi: first entry -1: no path)
};

// the compile-time capacity that serves k: 2, 4, 8 or 16 (0: k out of range)
inline int kbest_capacity(int k) {
    if (k < 1 || k > kKBestMax) return 0;
    int kc = 2;
    while (kc < k) kc *= 2;
    return kc;
}

// scratch of one wave at list length k: the score rows, then the back-pointers
__host__ __device__ inline int64_t decode_score_doubles(int32_t n_nodes, int k) { return 2 * int64_t(n_nodes) * k; }
__host__ __device__ inline int64_t decode_back_ints(int32_t max_len, int32_t max_dst, int k) {
    return int64_t(max_len > 0 ? max_len : 1) * int64_t(max_dst > 0 ? max_dst : 1) * k;
}
inline int64_t decode_wave_bytes(int32_t max_len, int32_t n_nodes, int32_t max_dst, int k) {
    return 8 * decode_score_doubles(n_nodes, k) + 4 * decode_back_ints(max_len, max_dst, k);
}

// grid blocks of `waves` wavefronts (1 .. kDecodeWavesPerBlock) each.  The
// Viterbi launch wants a.k == 1; the K-best launch runs the kernel of capacity
// kbest_capacity(a.k) (also at k = 1).  The scratch is sized for a.k, and one
// wave's must stay below 1 GiB (the K-best kernel indexes it with 32 bits).
hipError_t launch_best_paths(const DecodeArgs& a, int grid, int waves, hipStream_t stream);
hipError_t launch_kbest_paths(const DecodeArgs& a, int grid, int waves, hipStream_t stream);
// what both start with, and the sampler (sample.hpp) too: the work counter at
// zero and decode_edge_weight_kernel's a.lw from a.wt
hipError_t launch_edge_weights(const DecodeArgs& a, hipStream_t stream);

}  // namespace wfsa

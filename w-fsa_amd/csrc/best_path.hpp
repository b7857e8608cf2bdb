// Viterbi decode on the device: the most probable accepting path of every
// loaded string (wfsa_dev_best_paths).
//
// A (max, +) pass in the log domain over the byte-step trellis, one wavefront
// per string, over the in-edges-by-byte lists (WideModel).  Position i + 1 is
// live only on the destinations of byte c_i; lanes run over those
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
// The kernels read and write only the buffers named here: their own copy of
// the weights, their own edge log-weights, scratch, counter and outputs --
// nothing an evaluation, rmin, the QN loop or a captured graph touches.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fb_kernels.hpp"

namespace wfsa {

constexpr int kBestWavesPerBlock = 4;

struct BestPathArgs {
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
    const double* wt;        // [n_params + 1] weights (GetWeight form, zero slot last)
    double* lw;              // [n_edges + n_end] edge log-weights: the sum over the parameter list
    double* score;           // per wave: two rows of n_nodes (-inf outside the live nodes)
    int32_t* back;           // per wave: [max_len][max_dst] winning in-edge (index into w.e_src / w.e_g), -1: none
    unsigned* ctr;           // work counter: the next string (zero before the launch)
    double* best;            // [n_strings] log weight of the best path (-inf: none)
    int32_t* path;           // [total symbols + n_strings] string s: L + 1 combined edge ids at off[s] + s
                             // (first entry -1: no path)
};

// scratch bytes of one wave: the score rows, then the back-pointers
__host__ __device__ inline int64_t best_path_score_doubles(int32_t n_nodes) { return 2 * int64_t(n_nodes); }
__host__ __device__ inline int64_t best_path_back_ints(int32_t max_len, int32_t max_dst) {
    return int64_t(max_len > 0 ? max_len : 1) * int64_t(max_dst > 0 ? max_dst : 1);
}
inline int64_t best_path_wave_bytes(int32_t max_len, int32_t n_nodes, int32_t max_dst) {
    return 8 * best_path_score_doubles(n_nodes) + 4 * best_path_back_ints(max_len, max_dst);
}

// grid blocks of `waves` wavefronts (1 .. kBestWavesPerBlock) each
hipError_t launch_best_paths(const BestPathArgs& a, int grid, int waves, hipStream_t stream);

}  // namespace wfsa

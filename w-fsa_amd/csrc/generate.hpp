// Unconditional generation on the device (wfsa_dev_generate): n independent
// walks of the automaton itself, start -> (transition, emission)* -> end, each
// state choosing among its transitions and among its emissions with
// probability proportional to exp(weight).  No string is loaded and no trellis
// is built: the walk reads the flattened state graph of wfsa_model_desc, which
// is why it also serves a model on the dense path.
//
// The walk of sample i: U = start, m = 0; per step, draw 2m chooses one of
// tr_ptr[U] .. tr_ptr[U + 1] (target V); V == end completes the sample
// (status 0); otherwise draw 2m + 1 chooses one of em_ptr[V] .. em_ptr[V + 1];
// if its bytes would take the string past max_len the sample is truncated
// (status 1) and that emission is not recorded (the transition into V is);
// else its bytes are appended, U = V, m += 1.  A choice without candidates, or
// whose masses sum to 0, leaves the sample dead (status 2).
//
// Choice rule (the sampler's, sample.hpp): candidates of masses a_k =
// exp(w[param_k]) (1.0 for a single-member group, param -1), running sums left
// to right in the model's order, T the last one; the first k whose running sum
// exceeds u * T; when rounding leaves none, the last candidate of positive
// mass.  The running sums are formed once per call (generate_cdf_kernel), and a
// choice is a binary search in the state's slice of them: the sums do not
// decrease and a candidate of mass 0 repeats its predecessor, so the first
// entry above u * T is the linear rule's answer.
//
// Draw d of sample i is sample_uniform(seed, i, 0xFFFFFFFF, d): the sampler's
// key and counter layout with a sample word that sample_paths (t < 64) never
// uses.  A draw depends neither on n nor on the lane that made it, so the walk
// runs twice -- once to size the outputs, once to fill them -- with the same
// result.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wfsa {

constexpr int kGenerateBlock = 256;                 // threads per block = samples per tile
constexpr uint32_t kGenerateSampleWord = 0xFFFFFFFFu;

// the flattened state graph on the device (wfsa_model_desc's arrays)
struct GenerateModel {
    const int32_t* em_ptr;
    const int64_t* em_off;
    const int32_t* em_len;
    const int32_t* em_param;
    const uint8_t* em_bytes;
    const int32_t* tr_ptr;
    const int32_t* tr_dst;
    const int32_t* tr_param;
    int32_t n_states, start, end, n_params;
};

struct GenerateArgs {
    GenerateModel g;
    const double* w;      // [n_params] GetWeight form
    double* cdf_tr;       // [n_tr] inclusive running sums of exp(w) within each state's transitions
    double* cdf_em;       // [n_em] ... within each state's emissions
    unsigned* flag;       // set to 1 by the running-sum kernel: some weight is NaN or +inf
    int64_t n;            // samples
    int32_t max_len;
    uint32_t max_steps;   // n_states * (max_len + 1): no walk of a model without an epsilon cycle takes more
    uint64_t seed;
    // per sample, written by the sizing pass
    int32_t* len;         // bytes
    int32_t* plen;        // parameter ids
    double* logw;
    double* logp;
    int8_t* status;
    // the scan: per-tile sums ([2][tiles]: bytes, ids), then the exclusive offsets [n + 1]
    int64_t* bsum;
    int64_t* off;
    int64_t* prow;
    // written by the filling pass
    uint8_t* sym;
    int32_t* pidx;
};

__host__ __device__ inline int64_t generate_tiles(int64_t n) { return (n + kGenerateBlock - 1) / kGenerateBlock; }

// the running sums of every state's two groups, and the weights' check
hipError_t launch_generate_cdf(const GenerateArgs& a, hipStream_t stream);
// the walk without output (len, plen, logw, logp, status per sample), then off and prow by an exclusive scan
hipError_t launch_generate_size(const GenerateArgs& a, hipStream_t stream);
// the walk again, writing bytes and parameter ids at off / prow
hipError_t launch_generate_fill(const GenerateArgs& a, hipStream_t stream);

}  // namespace wfsa

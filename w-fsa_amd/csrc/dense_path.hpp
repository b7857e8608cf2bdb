// Dense-automaton path (BASELINE.json configs[4], SURVEY.md 8d "c5"): when the
// transition matrix is dense, one trellis step of many strings at once is a
// GEMM against the N x N matrix exp(w) -- fp64 MFMA (v_mfma_f64_16x16x4f64).
//
// Model (reference semantics, SURVEY.md 8 "Exact semantics"): the start state
// `^` moves to state T and T emits the first byte; each later byte is a
// transition S->T followed by T's 1-byte emission; `$` is entered once the
// string is consumed.  With a[T] = exp(w(^->T)), A[S][T] = exp(w(S->T)),
// E[T][c] = exp(w(T emits c)), e[S] = exp(w(S->$)):
//   alpha_1 = a (.) E[:, s_0],  alpha_{j+1} = (alpha_j A) (.) E[:, s_j],
//   q = alpha_L . e,  beta_L = e,  beta_j = A (E[:, s_j] (.) beta_{j+1}),
// and the gradient of every parameter is minus its p-weighted posterior
// count (src/QuasiNewtonLearner.cpp:93-125): transitions
// A (.) sum_j alpha_j^T (E (.) beta_{j+1}) / q, emissions / start / end edges
// from gamma_j = alpha_j (.) beta_j / q.
//
// Layout in HBM: strings are packed back to back into R row slots (longest
// first, each to the least loaded slot), so trellis step t of the batch is one
// R x Np row block whatever the string lengths are; every GEMM has M = R.
// alpha, gamma and z (the scaled E (.) beta rows the gradient GEMM consumes)
// are kept for all T steps: T x R x Np doubles each.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "wfsa_dev.h"

namespace wfsa {

// Parameter codes of the dense tables: >= 0 Fsa parameter, kCodeNone no
// such edge (weight 0), kCodeOne an unequivocal edge (weight 1).
constexpr int32_t kCodeNone = -1;
constexpr int32_t kCodeOne = -2;
constexpr int kDenseTile = 128;   // GEMM block tile (rows and columns)

struct DenseModel {
    int32_t n_states = 0;          // interior states (not ^, not $)
    int32_t np = 0;                // n_states padded to kDenseTile
    int32_t vocab = 0;             // distinct emitted bytes
    int32_t n_params = 0;          // Fsa parameters (n_full)
    int16_t sym_of_byte[256];      // byte -> symbol index, vocab = not emitted
    std::vector<int32_t> code_a;   // [np][np] S->T
    std::vector<int32_t> code_s;   // [np] ^->T
    std::vector<int32_t> code_e;   // [np] S->$
    std::vector<int32_t> code_em;  // [vocab+1][np] T emits symbol v (row vocab: none)
    int32_t code_se = kCodeNone;   // ^->$ (the empty string)
    int64_t n_transitions = 0;     // interior S->T edges
    std::vector<int32_t> state_id; // [n_states] interior index -> Fsa state id (wfsa_model_desc numbering), ascending
};

// Builds the dense tables when the automaton qualifies: every state other
// than ^ and $ emits single bytes only (no epsilon, no multi-byte emission),
// and -- unless force -- at least a quarter of the interior transition matrix
// is present with >= 64 interior states.  Returns "" when dense, else why not.
std::string dense_model_build(const wfsa_model_desc& d, bool force, DenseModel& out);

class DensePath {
public:
    explicit DensePath(int n_cu) : n_cu_(n_cu > 0 ? n_cu : 256) {}
    ~DensePath();
    DensePath(const DensePath&) = delete;
    DensePath& operator=(const DensePath&) = delete;

    hipError_t load_model(const DenseModel& m, hipStream_t s);
    // packs the strings into row slots and allocates the per-step buffers
    hipError_t load_corpus(const uint8_t* sym, const int64_t* off, const double* p, int64_t n_strings,
                           hipStream_t s);
    // One evaluation: out[0] = sum_s p_s log q_s, out[1 + j] = -sum_s p_s
    // E[count_j | s] for every Fsa parameter (the context's out layout);
    // logq (nullable) per string in load order.  ewp[j] = exp(w_full[j]).
    // structural: all weights 1 and all p 1 (path counts and used
    // parameters, wfsa_dev_recognize).  halted (nullable): nonzero = skip.
    hipError_t enqueue(const double* ewp, bool structural, double* out, double* logq, const unsigned* halted,
                       hipStream_t s);
    // The rmin info column at the weights of the evaluation just enqueued
    // (src/QuasiNewtonLearner.cpp:80-84): res[0] = min over strings and
    // their paths of path probability / q, res[1] = the string holding it
    // (lowest index on ties), by a (min, +) trellis pass in the log domain
    // over the same row slots -- one tiled min-plus product per step on the
    // fp64 VALU (a semiring MFMA does not compute).  Empty strings (one path,
    // relative probability 1) are not candidates.
    hipError_t enqueue_rmin(double* res, const unsigned* halted, hipStream_t s);
    // Viterbi decode at w_full (host, n_params log weights of which -inf is
    // the only non-finite value): a (max, +) pass over the same row slots
    // that keeps every step's scores (T x R x np doubles in the history the
    // sampler shares, allocated by the first call of either since the load
    // at the evaluations' row pitch) and a back-track kernel that recomputes each
    // predecessor from them, ties to the lowest state (dense_decode.hip).
    // Buffers of its own: the evaluations' and the rmin pass's state is not
    // touched.  ev[0..3] are recorded before the table kernel, after it,
    // after the forward steps and after the back-track.
    // hipErrorOutOfMemory: the history (best_paths_history_bytes) does not fit.
    hipError_t enqueue_best_paths(const double* w_full, hipEvent_t const ev[4], hipStream_t s);
    size_t best_paths_history_bytes() const;
    // the last pass's results: logw[S] the paths' weights (-inf: no path) and
    // codes[2 (total_symbols + S)]: string s owns the pairs from 2 (off[s] + s),
    // one (transition code, emission code) per byte and (end code, kCodeOne)
    // last; an empty string has its ^ -> $ code alone
    hipError_t best_paths_download(double* logw, int32_t* codes, hipStream_t s) const;
    const std::vector<int64_t>& string_offsets() const { return off_host_; }
    // Posterior path sampling at w_full (host, as for enqueue_best_paths):
    // forward filter, backward sample (dense_sample.hip).  The forward pass is
    // the evaluation's own -- dense_weights_kernel at exp(w_full), the split-K
    // RAW step GEMM, dense_fwd_epi_kernel per step, dense_final_kernel for
    // log q, whatever engine the evaluations run -- into buffers of the
    // sampler's own, every step's scaled alpha row kept in the history the
    // Viterbi decode keeps its scores in (scratch of both; no result outlives
    // it).  Then one wavefront per (string, sample) walks back from the end:
    // each state by inverse CDF over alpha[S] A[S][T] in ascending S with one
    // Philox draw (sample.hpp), and forward again for the path's parameter
    // codes and its weight as the decoders form it.  n samples per string,
    // 1 .. kSampleMax.  ev[0..2] are recorded before the forward pass, after
    // it and after the backward kernel.
    // hipErrorOutOfMemory: the history (history_bytes) does not fit.
    hipError_t enqueue_sample_paths(const double* w_full, int32_t n, uint64_t seed, hipEvent_t const ev[3], hipStream_t s);
    // bytes of the fixed-size path output of n samples per string
    size_t sample_paths_output_bytes(int32_t n) const;
    // the last pass's results: logq[S], logw[S n] (-inf: no path) and
    // codes[2 n (total_symbols + S)]: sample t of string s owns the pairs from
    // 2 ((off[s] + s) n + t (L + 1)), laid out as best_paths_download's
    hipError_t sample_paths_download(int32_t n, double* logq, double* logw, int32_t* codes, hipStream_t s) const;
    // Per-byte state posteriors and the MEA decode at w_full (host, as for
    // enqueue_best_paths; dense_marginals.hip), in four phases on one stream,
    // buffers of the feature's own except the shared history:
    //   byte_marginals_masses  the evaluation's forward pass (as the sampler
    //                          runs it) and its backward pass with p = 1
    //                          (enqueue_backward_into), gamma written over
    //                          alpha in the history: the history then holds
    //                          alpha beta exp(la + lb - log q) per slot and state
    //   byte_marginals_count   a wavefront per corpus byte counts the interior
    //                          states with min(gamma, 1) > 0; the prefix sum
    //                          is taken on the host (synchronises); returns
    //                          the number of entries
    //   byte_marginals_fill    allocates the rows and fills them: Fsa state
    //                          ids ascending, the clamped masses
    //   byte_marginals_decode  dense_decode_tables_kernel into tables of its
    //                          own, lA turned into a 0 / -inf mask, T reward
    //                          (max, +) steps that write D over gamma in the
    //                          history, and the back-track
    // ev[0..7]: before / after the forward pass, after the backward pass,
    // after the count, before / after the fill, before / after the decode.
    // hipErrorOutOfMemory from _masses: the history does not fit; from _fill:
    // the rows do not.
    hipError_t byte_marginals_masses(const double* w_full, hipEvent_t const ev[8], hipStream_t s);
    hipError_t byte_marginals_count(int64_t* n_entries, hipEvent_t const ev[8], hipStream_t s);
    hipError_t byte_marginals_fill(hipEvent_t const ev[8], hipStream_t s);
    hipError_t byte_marginals_decode(hipEvent_t const ev[8], hipStream_t s);
    // results: logq[S]; the rows (mrow[total_symbols + 1] from the count,
    // midx / mval of its last entry's length); score[S] (NaN: no path),
    // logw[S] and codes as best_paths_download gives them
    hipError_t byte_marginals_logq_download(double* logq, hipStream_t s) const;
    const std::vector<int64_t>& byte_marginals_mrow() const { return bm_mrow_host_; }
    hipError_t byte_marginals_rows_download(int32_t* midx, double* mval, hipStream_t s) const;
    void byte_marginals_rows_release();   // (the rows live on the host after the download)
    hipError_t byte_marginals_paths_download(double* score, double* logw, int32_t* codes, hipStream_t s) const;

    // the last evaluation ran at real weights (not the structural pass)
    bool weighted() const { return weighted_; }
    int64_t n_strings() const { return n_strings_; }
    int32_t rows() const { return R_; }
    int32_t steps() const { return T_; }
    int32_t np() const { return np_; }
    // the GEMM engine the evaluations run: 0 fused MFMA kernels, 1 rocBLAS
    // dgemm + epilogue kernels, 2 split-K MFMA kernels + epilogue kernels,
    // 3 LDS-DMA pipelined MFMA kernels + epilogue kernels
    int engine() const { return engine_ == 1 && !blas_ ? 0 : engine_; }
    int64_t total_symbols() const { return total_sym_; }
    // algorithmic fp64 flops of one evaluation: three GEMMs of 2 np^2 per
    // string position (forward, backward, gradient)
    double gemm_flops() const { return 6.0 * double(np_) * double(np_) * double(total_sym_); }
    // flops the GEMM launches execute (slot padding included)
    double issued_flops() const;

private:
    int n_cu_ = 256;
    int grad_cfg_ = 0;   // gradient GEMM: 4-wave blocks, K slices of 16, two blocks per CU (WFSA_DENSE_GRAD_CFG=1: 8-wave, 32; 65.7 vs 69.8 ms, profiles/r04/gemm_cfg_ab.txt)
    // WFSA_DENSE_STEP_CFG: 5 (default) engine 2's step GEMMs as 8-wave 128 x 128 blocks, 64 x 32 per wave,
    // two blocks per CU (c5 0.797 -> 0.814 of the fp64 peak, profiles/r05/c5_step_gemm_8wave.txt); timing
    // experiments: 0 the 4-wave blocks, 6 the gradient GEMM in 8-wave blocks too (0.80), 1 per-step GEMMs with
    // 4-wave blocks, 2 K slices of 16, 3 engine 2 with K slices of 32, 4 engine 3 with its own gradient GEMM
    int step_cfg_ = 5;
    int32_t n_params_ = 0, np_ = 0, vocab_ = 0, nct_ = 0;
    int32_t n_states_ = 0;             // interior states (np_ without the padding)
    int32_t code_se_ = kCodeNone;
    int16_t sym_of_byte_[256] = {};
    int64_t n_strings_ = 0, total_sym_ = 0;
    int32_t R_ = 0, T_ = 0;
    bool weighted_ = false;
    int32_t ldx_ = 0;                  // row pitch of alpha / gamma / z / Y
    double p0_sum_ = 0.0, n0_ = 0.0;   // sum of p / count of empty strings
    int32_t reduce_chunks_ = 0;
    // model tables
    int32_t* code_a_ = nullptr;
    int32_t* code_s_ = nullptr;
    int32_t* code_e_ = nullptr;
    int32_t* code_em_ = nullptr;
    int32_t* state_id_ = nullptr;  // [n_states] interior index -> Fsa state id
    // per-iteration weights
    double* amat_ = nullptr;   // [np][np]
    double* amat_t_ = nullptr; // [np][np] transposed
    double* et_ = nullptr;     // [vocab+1][np]
    double* a0_ = nullptr;     // [np]
    double* aend_ = nullptr;   // [np]
    double* ones_ = nullptr;   // [n_params + 1] all ones (structural pass)
    // corpus: slots
    int32_t* meta_ = nullptr;  // [T][R] symbol | start << 9 | end << 10 (idle: symbol = vocab)
    int32_t* sid_ = nullptr;   // [T][R] string or -1
    int32_t* end_at_ = nullptr;  // [S] t * R + r of the string's last position, -1 if empty
    double* p_ = nullptr;      // [S]
    double* pones_ = nullptr;  // [S] all ones
    double* logq_ = nullptr;   // [S]
    double* la_ = nullptr;     // [T][R]
    double* lb_ = nullptr;     // [T][R]
    double* alpha_ = nullptr;  // [T][R][np]
    double* gam_ = nullptr;    // [T][R][np]
    double* z_ = nullptr;      // [T][R][np]
    double* y_ = nullptr;      // [2][R][np]
    double* part_ = nullptr;   // [2][nct][R]
    double* ll_part_ = nullptr;
    int32_t n_ll_ = 0;
    double* red_ = nullptr;    // [chunks][vocab+2][np]
    // GEMM engine (WFSA_DENSE_ENGINE=fused|blas|split|dma, default split;
    // WFSA_DENSE_BLAS=0/1 = fused/blas): 1 the GEMMs as plain fp64 library GEMMs (rocBLAS, atomics
    // off: deterministic) with our epilogue kernels; 2 the same flow with our
    // RAW GEMM kernel (K split in two halves: 2 blocks per CU) for the step
    // GEMMs and the fused gradient kernel; 0 the fused MFMA kernels above
    int engine_ = 2;
    void* blas_ = nullptr;     // rocblas_handle
    double* gbuf_ = nullptr;   // [np][np] the gradient GEMM's product (engine 1)
    double* ysplit_ = nullptr; // [R][ldx] the second K half's products (engine 2)
    // rmin pass (allocated by its first call): log tables (+inf: no edge),
    // two row-slot buffers of log min-path weights, per column tile and
    // string the end minima, per block the string minima
    double* lmat_ = nullptr;   // [np][np] log A
    double* let_ = nullptr;    // [vocab+1][np] log E^T
    double* l0_ = nullptr;     // [np] log a
    double* lend_ = nullptr;   // [np] log e
    double* mrow_ = nullptr;   // [2][R][np]
    double* spart_ = nullptr;  // [nct][S]
    double* rpart_ = nullptr;  // [2 * blocks]
    // Viterbi decode (allocated by its first call, freed with the corpus):
    // the weights, log tables (-inf: no edge), the score history, the paths
    std::vector<int64_t> off_host_;   // [S + 1] the strings' offsets
    int64_t* doff_ = nullptr;  // [S + 1]
    double* dw_ = nullptr;     // [n_params]
    double* dla_ = nullptr;    // [np][np] log A
    double* dlat_ = nullptr;   // [np][np] transposed
    double* dle_ = nullptr;    // [vocab+1][np] log E^T
    double* dl0_ = nullptr;    // [np]
    double* dlend_ = nullptr;  // [np]
    double* dhist_ = nullptr;  // [T][R][np]
    int32_t* dstates_ = nullptr;  // [total symbols]
    int32_t* dcodes_ = nullptr;   // [2 (total symbols + S)]
    double* dlogw_ = nullptr;  // [S]
    // Posterior sampling (allocated by its first call, freed with the corpus):
    // the weights and exp of them, the forward pass's tables, scales and
    // log q, the sampled states, codes and weights (fs_n_ samples per string)
    double* fs_w_ = nullptr;       // [n_params]
    double* fs_ewp_ = nullptr;     // [n_params]
    double* fs_amat_ = nullptr;    // [np][np]
    double* fs_amat_t_ = nullptr;  // [np][np] transposed
    double* fs_et_ = nullptr;      // [vocab+1][np]
    double* fs_a0_ = nullptr;      // [np]
    double* fs_aend_ = nullptr;    // [np]
    double* fs_la_ = nullptr;      // [T][R]
    double* fs_sum_ = nullptr;     // [2][R]
    double* fs_ysplit_ = nullptr;  // [R][ldx]
    double* fs_logq_ = nullptr;    // [S]
    double* fs_ll_ = nullptr;      // [blocks of dense_final_kernel]
    int32_t* fs_states_ = nullptr; // [n total symbols]
    int32_t* fs_codes_ = nullptr;  // [2 n (total symbols + S)]
    double* fs_logw_ = nullptr;    // [S n]
    int32_t fs_n_ = 0;
    // the history both passes keep their rows in: [T][R][ldx] doubles
    hipError_t history_alloc();
    // the evaluation's forward pass (engine 2's flow) at ewp into the caller's
    // buffers: the tables, alpha[T][R][ldx], la[T][R], log q
    struct ForwardBufs {
        double *amat, *amat_t, *et, *a0, *aend, *alpha, *la, *sum, *ysplit, *logq, *ll_part;
    };
    hipError_t enqueue_forward_into(const double* ewp, const ForwardBufs& b, hipStream_t s);
    // the evaluation's backward pass (engine 2's flow) with p = 1 behind a
    // forward pass into the same buffers: gam[T][R][ldx] = alpha beta
    // exp(la + lb - log q) (gam may be alpha: a step reads and writes its own
    // elements alone, and the recursion never reads alpha), lb[T][R]; y is
    // [2][R][ldx], z one [R][ldx] block every step overwrites (the gradient
    // GEMM that would read it does not run)
    struct BackwardBufs {
        const double *amat_t, *et, *aend, *alpha, *la, *logq;
        double *gam, *lb, *sum, *y, *ysplit, *z;
    };
    hipError_t enqueue_backward_into(const BackwardBufs& b, hipStream_t s);
    // dense_decode_tables_kernel at w (device) into the caller's log tables
    struct DecodeTables {
        double *la, *lat, *le, *l0, *lend;
    };
    hipError_t enqueue_decode_tables_into(const double* w, const DecodeTables& t, hipStream_t s);
    // Byte marginals and the MEA decode (allocated by its first call, freed
    // with the corpus): the forward and backward passes' tables and scales,
    // the row of every corpus byte, the rows, the decode's tables and paths
    struct ByteMarginalBufs {
        double *w = nullptr, *ewp = nullptr;                                          // [n_params]
        double *amat = nullptr, *amat_t = nullptr;                                    // [np][np]
        double *et = nullptr, *a0 = nullptr, *aend = nullptr;                         // [vocab+1][np], [np], [np]
        double *la = nullptr, *lb = nullptr, *sum = nullptr;                          // [T][R], [T][R], [2][R]
        double *y = nullptr, *ysplit = nullptr, *z = nullptr;                         // [2][R][ldx], [R][ldx], [R][ldx]
        double *logq = nullptr, *ll = nullptr;                                        // [S], [blocks of dense_final_kernel]
        int32_t *rowof = nullptr, *cnt = nullptr;                                     // [total symbols]: t R + r of the byte; its entries
        int64_t* mrow = nullptr;                                                      // [total symbols + 1]
        int32_t* midx = nullptr;                                                      // [entries]
        double* mval = nullptr;                                                       // [entries]
        double *tla = nullptr, *tlat = nullptr, *tle = nullptr, *tl0 = nullptr, *tlend = nullptr;   // the decode's tables
        int32_t *states = nullptr, *codes = nullptr;                                  // [total symbols], [2 (total symbols + S)]
        double *logw = nullptr, *score = nullptr;                                     // [S]
    } bm_;
    std::vector<int64_t> bm_mrow_host_;   // [total symbols + 1] the last count's prefix sum
    hipError_t enqueue_lib(const double* w, const double* p, bool structural, double* out, double* logq,
                           const unsigned* halted, hipStream_t s);
    void free_corpus();
    void free_model();
};

}  // namespace wfsa

/*
 * wfsa_dev.h -- the drop-in device boundary of the MI355X w-fsa path.
 *
 * The reference (gaebor/w-fsa) has no FFI: its hot path is the body of the
 * Learner class hierarchy.  These C entry points replace, one for one, the
 * hot functions a host-side Learner calls:
 *
 *   wfsa_dev_load_model     <- the Fsa graph walked by Recognizer
 *                              (inc/Fsa.h:26-66, inc/Recognize.h:35-96)
 *   wfsa_dev_load_corpus    <- Corpus strings + p (inc/Corpus.h:16-26,
 *                              src/Learner.cpp:297-302)
 *   wfsa_dev_recognize      <- Learner::BuildPaths (src/Learner.cpp:276-348):
 *                              recognized flag, exact path count per string and
 *                              the "used parameter" marks Trim consumes
 *                              (src/Learner.cpp:310, :350-425)
 *   wfsa_dev_objective_grad <- Learner::ComputeModeledProbs + ComputeObjective
 *                              (src/Learner.cpp:515-553) and
 *                              QuasiNewtonLearner::ComputeGrad
 *                              (src/QuasiNewtonLearner.cpp:93-125) ==
 *                              HessianLearner::ComputeGrad
 *                              (src/HessianLearner.cpp:565-597)
 *   wfsa_dev_comm_*         <- (new) one all-reduce per iteration when the
 *                              corpus is sharded over GPUs (RCCL, or an
 *                              in-process group of contexts)
 *
 * Conventions: plain pointers and sizes, host buffers caller-owned and only
 * touched during the call; all device memory belongs to the context.  Every
 * entry point returns WFSA_OK (0) or a negative code and sets a thread-local
 * message readable with wfsa_dev_last_error() -- the reference throws MyError
 * subclasses with a message (inc/Utils.h:130-141); no exception crosses this
 * ABI.  A context is bound to one device and is not re-entrant.
 */
#ifndef WFSA_DEV_H
#define WFSA_DEV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFSA_OK 0
#define WFSA_ERR_ARG (-1)      /* invalid argument / call order            */
#define WFSA_ERR_HIP (-2)      /* HIP runtime failure                       */
#define WFSA_ERR_MODEL (-3)    /* automaton rejected (e.g. epsilon cycle)   */
#define WFSA_ERR_CAPACITY (-4) /* a string's trellis exceeds device limits  */
#define WFSA_ERR_RCCL (-5)     /* collective failure                        */
#define WFSA_ERR_NODEV (-6)    /* no usable gfx950 device / kernels missing */

typedef struct wfsa_dev wfsa_dev;

/* The automaton after Fsa::AssignIndices (src/Fsa.cpp:207-238), flattened.
 * States are 0..n_states-1; per state its emissions (byte strings, possibly
 * empty or multi-byte) and its transitions.  *_param is the Fsa parameter
 * index, or -1 for an unequivocal (single-member) group, whose weight is
 * log 1.  `end` is the end state's id or -1 when nothing transitions to it. */
typedef struct {
    int32_t n_states;
    int32_t start;
    int32_t end;
    int32_t n_params;          /* Fsa::GetNumberOfParameters() ("n_full")   */
    const int32_t* em_ptr;     /* [n_states+1]                              */
    const int64_t* em_off;     /* [n_em] offset of the emission in em_bytes */
    const int32_t* em_len;     /* [n_em]                                    */
    const int32_t* em_param;   /* [n_em]                                    */
    const uint8_t* em_bytes;
    const int32_t* tr_ptr;     /* [n_states+1]                              */
    const int32_t* tr_dst;     /* [n_tr]                                    */
    const int32_t* tr_param;   /* [n_tr]                                    */
} wfsa_model_desc;

typedef struct {
    int64_t n_strings;         /* strings resident on this device           */
    int64_t total_symbols;     /* sum of their lengths                      */
    int32_t max_len;
    int32_t n_nodes;           /* trellis nodes after epsilon removal       */
    int64_t n_edges;           /* byte-consuming composite edges            */
    int64_t n_end_edges;
    int64_t compiled_strings;  /* served by the compiled-stream kernel      */
    int64_t fallback_strings;  /* served by the traversal kernel            */
    int64_t stream_words;      /* compiled main-stream words                */
    int64_t stream_bytes;      /* main-stream bytes incl. chunk padding     */
    int64_t bubble_words;
    int64_t n_bubbles;         /* compiled bubbles (bubble kernel lanes)    */
    int64_t fb_launches;       /* objective_grad calls timed so far         */
    double fb_kernel_ms;       /* sum of their forward-backward kernel time */
    double last_fb_kernel_ms;  /* last call: compiled + traversal kernels   */
    double last_compiled_ms;   /* last call: compiled-stream kernel alone   */
    double last_call_ms;       /* last call, device side, end to end        */
    int64_t last_live_edges;   /* traversal-path trellis edges, last call   */
    int32_t tier1_strings;     /* strings needing the large-slab tier       */
    int32_t waves_per_block;
    double prepare_ms;         /* structural pass + stream compilation      */
    double compiled_kernel_ms; /* sum over calls of the compiled kernel     */
    int32_t graph;             /* last call replayed a captured hipGraph    */
    int32_t dense;             /* the dense fp64 MFMA path serves the model */
    /* filled by wfsa_learner_stats (zero from wfsa_dev_get_stats): host time
     * of the learner's optimization steps, summed over host_steps steps --
     * before the device call is enqueued, overlapped with it, waiting for
     * it, after it (gradient mapping + update) */
    int64_t host_steps;
    double host_begin_ms, host_overlap_ms, host_wait_ms, host_post_ms;
    /* dense path (dense == 1): row slots R and trellis steps T of the packed
     * corpus; each evaluation runs 3 GEMMs of 2 np^2 R flops per step */
    int32_t dense_rows, dense_steps, dense_np;
    int32_t tier2_strings;     /* strings on the global-scratch traversal tier */
    int32_t wave_strings;      /* traversal strings on the wave-per-string pair-table kernel */
    int64_t wave_row_entries;  /* per evaluation: alpha entries it writes (and reads back), sum |D| */
    int64_t wave_pair_edges;   /* per evaluation: pair-list edges one pass walks */
    int32_t comm_ranks;        /* communicator size (1: none) */
    int32_t comm_peer;         /* the one-shot peer all-reduce: 1 on, 0 off / untried, -1 its set-up check failed */
    int64_t slot_chunks;       /* bubble contribution slots, in 16-slot chunks (8 B a slot) */
    int32_t max_group_chunks;  /* chunks of the largest constraint's slot group (one QN block sums it) */
    int32_t wave_pull;         /* the wave kernel pulls (wave_pull_kernel): nodes per lane (4, 6, 8); 0: it pushes (wide2_kernel) */
    int32_t dense_blas;        /* dense path GEMM engine (WFSA_DENSE_ENGINE): 0 our fused MFMA kernels, 1 rocBLAS dgemm + our epilogues, 2 our split-K MFMA kernels + epilogues, 3 our LDS-DMA pipelined MFMA kernels + epilogues */
    int32_t qn_inkernel_waves; /* last device QN run: its update ran inside the stream kernel on this many waves (0: the separate QN step kernel) */
    int32_t qn_batches;        /* ... in this many batches of constraints (at most 64 members each) */
    /* the regime of the per-iteration path, chosen at preparation from the
     * parameter count and the structural counts */
    int32_t stream_block;      /* threads per block of the stream kernel (512 or 1024) */
    int32_t stream_w_lds;      /* it stages the weight table in LDS */
    int32_t stream_wide;       /* 32-bit stream words (n_full >= 0x8000 or >= 0x7fff multi-parameter edges) */
    int32_t stream_multi;      /* some stream word is a multi-parameter composite */
    int32_t stream_delta;      /* it reads the delta format */
    int32_t bubbles_fused;     /* an evaluation without log q runs the bubbles inside the stream kernel */
    int32_t grad_tables;       /* the preparation-time gradient pass accumulates in LDS (0: per-block slabs in HBM) */
    int32_t wave_lgrad;        /* the traversal wave kernel's gradient table is in LDS (1) or global (0); -1: no wave kernel configured */
    int64_t ll_dot_launches;   /* step launches without the stream pass so far: the trivial words' log-likelihood as a dot product (WFSA_LL_DOT=0: none) */
    double best_path_ms;       /* last wfsa_dev_best_paths call: device time of its kernels */
    double kbest_path_ms;      /* last wfsa_dev_kbest_paths call: device time of its kernels */
    double sample_path_ms;     /* last wfsa_dev_sample_paths call: device time of its kernels */
    double posterior_count_ms; /* last wfsa_dev_posterior_counts call: device time of its kernels */
    double byte_marginal_ms;   /* last wfsa_dev_byte_marginals call: device time of its kernels */
    int64_t shaped_bubbles;    /* small bubbles whose structure has compiled-in sweeps (WFSA_BUBBLE_SHAPES=0: none) */
    int64_t mixed_shape_waves; /* small-bubble waves whose lanes carry more than one structure id (several sweep turns) */
    int64_t small_bubbles_a;   /* small bubbles of class A (<= 4 nodes and edges), one lane each */
    int64_t small_bubbles_b;   /* small bubbles of class B (<= 8 nodes and edges); n_bubbles counts the big ones too */
    int64_t big_bubbles;       /* bubbles of neither class (more nodes or edges, or a multi-parameter edge), one wave each */
    int32_t max_bubble_nodes;  /* nodes of the largest compiled bubble (at most 32; 0: no bubble) */
    int32_t max_bubble_edges;  /* edges of the compiled bubble with the most edges (at most 255; 0: no bubble) */
    double generate_ms;        /* last wfsa_dev_generate call: device time of its kernels */
    /* last wfsa_dev_dense_best_paths call (its sum is best_path_ms): the table
     * kernel, the T forward steps, the back-track kernel */
    double dense_bp_tables_ms, dense_bp_forward_ms, dense_bp_backtrack_ms;
    int64_t qn_wave_launches;  /* QN steps so far whose update ran as qn_wave_kernel, a wave per constraint (WFSA_QN_WAVE=0: none; the others launch qn_step_kernel or ride in the stream kernel) */
    /* last wfsa_dev_dense_sample_paths call (its sum is sample_path_ms): the
     * forward pass (tables, the T steps, the final kernel), the backward kernel */
    double dense_sp_forward_ms, dense_sp_backward_ms;
    /* last wfsa_dev_dense_byte_marginals call (its sum is byte_marginal_ms): the
     * forward pass, the backward pass, the count and fill kernels (0 with
     * rows = 0), the tables, reward steps and back-track (0 with decode = 0) */
    double dense_bm_forward_ms, dense_bm_backward_ms, dense_bm_rows_ms, dense_bm_decode_ms;
    int64_t bubble_grid_launches; /* of ll_dot_launches, those launched as a grid of only the waves that have work (step_grid_kernel; WFSA_BUBBLE_GRID=0, the rmin column or the in-kernel QN update: none) */
    int32_t stream_grid;       /* blocks of the stream kernel's geometry (stream_block threads each); the bubble-grid launch's roles are waves of it */
} wfsa_dev_stats;

/* context ---------------------------------------------------------------- */
int wfsa_dev_create(int device, wfsa_dev** out);
void wfsa_dev_destroy(wfsa_dev* ctx);
const char* wfsa_dev_last_error(void);

/* One-time uploads -------------------------------------------------------- */
int wfsa_dev_load_model(wfsa_dev* ctx, const wfsa_model_desc* model);
/* sym: packed bytes, off[n_strings+1] offsets into sym, p[n_strings] weights
 * (the reference's p: corpus weight / sum over ALL strings). */
int wfsa_dev_load_corpus(wfsa_dev* ctx, const uint8_t* sym, const int64_t* off,
                         const double* p, int64_t n_strings);

/* Structural pass (weights ignored) over the loaded strings.  Any output may
 * be NULL.  recognized[s] = 1 iff the string has an accepting path;
 * path_count[s] = number of accepting paths (exact below 2^53);
 * used_param[j] = 1 iff Fsa parameter j lies on an accepting path of some
 * string (OR over ranks when a communicator is attached). */
int wfsa_dev_recognize(wfsa_dev* ctx, uint8_t* recognized, double* path_count,
                       uint8_t* used_param);

/* Dense symmetric-indefinite factorisation in HBM for the HessianLearner's
 * KKT system (MKL DSS in the reference: dss_factor_real / dss_statistics
 * "Inertia", "Determinant" / dss_solve_real, src/HessianLearner.cpp:28-57,
 * 100-113; RealSymmetricLogDet src/Utils.cpp:296-350): Bunch-Kaufman LDL^T
 * (our own right-looking kernels, sym_solver.hip, with LAPACK dsytf2's pivot rule
 * and storage) of a[n*n] (symmetric, either layout); inertia =
 * {positive, negative, zero} pivots of D, log|det| and its sign.  sym_solve
 * overwrites b[n] with A^-1 b (one-workgroup dsytrs kernel). */
int wfsa_dev_sym_factor(wfsa_dev* ctx, int64_t n, const double* a, int64_t inertia[3], double* log_abs_det,
                        int32_t* det_sign);
int wfsa_dev_sym_solve(wfsa_dev* ctx, double* b);
/* The same from the matrix's entries -- upper-triangle coordinates
 * (i[t] <= j[t]; duplicates add), no dense host copy -- assembled in HBM and
 * factored blockwise: Bunch-Kaufman pivots within 128-column diagonal blocks
 * (MKL DSS's supernode-restricted pivoting), the trailing updates as fp64
 * library GEMMs (rocBLAS dsyrkx on MFMA); b (nullable) is solved in place and
 * refined against the entries.  When a block pivot falls under 1e-12 max|A|,
 * L grows past 1e8, or the refined solve misses a backward error of 1e-12,
 * the full Bunch-Kaufman factorisation above is used instead.  *method = 1
 * blocked, 2 full.  sym_solve works after either. */
int wfsa_dev_sym_factor_coo(wfsa_dev* ctx, int64_t n, int64_t nnz, const int32_t* i, const int32_t* j,
                            const double* v, double* b, int64_t inertia[3], double* log_abs_det, int32_t* det_sign,
                            int32_t* method);

/* Matrix-file mode (Learner::LoadMatrices, src/Learner.cpp:125-199; main.cpp
 * -m "<file"): instead of an automaton and strings, the path matrices the
 * reference's BuildPaths builds.  P: n_paths x n_params CSR (prow[n_paths+1],
 * pcol/pdata[prow[n_paths]], parameter counts); M: n_strings x n_paths CSR
 * of ones (mrow[n_strings+1], mcol = path indices); p[n_strings].  M names
 * every path exactly once (a path of two strings or of none: WFSA_ERR_ARG).  Replaces
 * any loaded model and corpus; objective_grad then takes w_full = x
 * (n_params values, no trimming) and computes the reference's SpMV chain
 * (logq = log M exp(P x), grad = -P^T (rpp (.) M^T p)); recognize reports
 * the path counts of M and the parameters P uses; rmin reports the
 * reference's path index.  Leave the mode with wfsa_dev_load_model. */
int wfsa_dev_load_paths(wfsa_dev* ctx, int32_t n_params, int64_t n_paths, const int64_t* prow, const int32_t* pcol,
                        const double* pdata, int64_t n_strings, const int64_t* mrow, const int64_t* mcol,
                        const double* p);

/* The rmin info column (QuasiNewtonLearner::GetOptimizationInfo,
 * src/QuasiNewtonLearner.cpp:80-84; HessianLearner :313-317) at the weights
 * of the last evaluation: *rmin = the smallest relative path probability
 * exp(P x)_path / q_s over all paths of ambiguous strings (path count > 1),
 * exact; *string_index = the loaded string holding that path (-1 when no
 * string is ambiguous).  The reference reports the path's index in its BFS
 * enumeration instead, which has no counterpart without enumerating paths
 * (in matrix-file mode, where paths are given, *string_index is that path
 * index).  On the dense path the candidates are every non-empty string
 * (a (min, +) trellis over its row slots; WFSA_ERR_ARG until an evaluation
 * at real weights has run). */
int wfsa_dev_rmin(wfsa_dev* ctx, double* rmin, int64_t* string_index);

/* Viterbi decode: the most probable accepting path of every loaded string at
 * w_full (GetWeight form, as objective_grad takes it) -- a (max, +) pass with
 * back-pointers over the byte-step trellis, one wavefront per string,
 * whichever tier serves the string in the learning path.
 *   best_logw[s] = max over accepting paths of the sum of the path's weights,
 *                  -inf when the string has none (NULL allowed);
 *   *n_entries   = total length of the paths' parameter lists (NULL allowed).
 * best_paths_get then copies the paths out: pidx[prow[s] .. prow[s + 1]) are
 * the Fsa parameter ids of string s's best path in path order, repeats kept
 * (single-member groups carry no id, as everywhere); an unrecognized string
 * has an empty range.  Ties are broken by a fixed rule (the first in-edge of
 * a node, the lowest end node, its first end edge), so equal weights give
 * equal results.  Valid until the next load or best_paths call.
 * The call is local to the rank (no collective, like logq) and touches no
 * state of the learning path: evaluations, rmin and the QN loop continue as
 * if it had not run.  WFSA_ERR_ARG before a model and a corpus are loaded,
 * while an evaluation is in flight and in matrix-file mode; on the dense path
 * WFSA_ERR_CAPACITY (no trellis is built there: load with WFSA_DENSE=0). */
int wfsa_dev_best_paths(wfsa_dev* ctx, const double* w_full, double* best_logw, int64_t* n_entries);
int wfsa_dev_best_paths_get(wfsa_dev* ctx, int64_t* prow, int32_t* pidx);

/* Viterbi decode on the dense path (stats.dense == 1), where no trellis is
 * built and wfsa_dev_best_paths fails: the most probable accepting path of
 * every loaded string at w_full by a (max, +) pass over the row slots of the
 * dense path (dense_decode.hip).  Outputs in best_paths' layout and
 * conventions: best_logw[s] (-inf without an accepting path of finite weight:
 * a byte no state emits, an empty string without a ^ -> $ edge, every path
 * crossing a -inf weight; NULL allowed), *n_entries (NULL allowed), and
 * dense_best_paths_get's pidx[prow[s] .. prow[s + 1]): Fsa parameter ids in
 * path order, repeats kept, a transition before the emission it leads to, the
 * end transition last; single-member groups carry no id; a string without a
 * path has an empty range; an empty string with a ^ -> $ edge has that edge
 * as its path.
 *
 * Arithmetic, exactly.  Log tables come from w_full and the model's parameter
 * codes directly (never log(exp(w))), a missing edge or padded state -inf, a
 * single-member group 0.0: lA[S][T], its transpose lAT[T][S], lE[v][T], l0[T]
 * (^ -> T), lend[T] (T -> $).  Forward, per row slot r and step t:
 *   D_t[r][T] = l0[T] + lE[sym][T]                          where a string starts,
 *   D_t[r][T] = max_S(D_{t-1}[r][S] + lA[S][T]) + lE[sym][T]  elsewhere
 * (the max first, then one add); every D_t is kept -- T x R x np doubles,
 * the size of one of the three histories of an evaluation, allocated by the
 * first call and freed by the next load.  End: the T that maximises
 * D_end[r][T] + lend[T], ties to the lowest T; a maximum of -inf: no path.
 * Back-track: the predecessor of T is the S that maximises D_{t-1}[r][S] +
 * lAT[T][S], ties to the lowest S, recomputed from the history (no
 * back-pointers are stored); a -inf candidate is never chosen.
 * best_logw is not the search's score but the decoders' weight of the
 * returned path: an edge's weight is the left-to-right sum, from 0.0, of its
 * present parameters' weights (transition, then emission), the path's the
 * left-to-right sum, from 0.0, of its edges' weights, the end edge last -- bit
 * for bit what best_paths / kbest_paths report for that path when the model
 * is loaded with WFSA_DENSE=0.  The search rounds (D + lA) + lE where the
 * trellis decode rounds D + (lA + lE), so the returned path can differ from
 * best_paths' only where a decision on it is closer than that rounding (a
 * few ulp) or at exact ties; there both break ties towards the lowest state
 * (for a model that qualifies for the dense path best_paths' first in-edge is
 * the one from the lowest source state).
 *
 * Needs a loaded model and corpus; no evaluation has to have run.  Local to
 * the rank; leaves the learning path untouched (evaluations, rmin, the QN
 * loop and generate go on as if it had not run).  Valid until the next load
 * or dense_best_paths call.  stats.best_path_ms = device time of its kernels
 * (dense_bp_*_ms its parts).  WFSA_ERR_ARG when the model is not on the dense
 * path (use wfsa_dev_best_paths), before a model and a corpus are loaded, in
 * matrix-file mode, while an evaluation is in flight, for a w_full entry that
 * is NaN or +inf (before any kernel runs), and from _get without a result
 * since the last load; WFSA_ERR_CAPACITY, naming the bytes, when the score
 * history cannot be allocated. */
int wfsa_dev_dense_best_paths(wfsa_dev* ctx, const double* w_full, double* best_logw /* [n_strings], NULL ok */,
                              int64_t* n_entries /* NULL ok */);
int wfsa_dev_dense_best_paths_get(wfsa_dev* ctx, int64_t* prow /* [n_strings + 1] */, int32_t* pidx /* [n_entries] */);

/* K-best decode: the k most probable accepting paths of every loaded string at
 * w_full, 1 <= k <= WFSA_KBEST_MAX -- best_paths' trellis pass with a sorted
 * list of k scores and k (in-edge, source rank) back-pointers per live node, a
 * wave-wide top-k over the end edges and k back-tracks (kbest_path.hip).
 *   *n_paths   = paths found over all strings (NULL allowed);
 *   *n_entries = total length of their parameter lists (NULL allowed).
 * kbest_paths_get copies them out (any pointer may be NULL): string s owns the
 * paths srow[s] .. srow[s + 1], in descending weight; logw[t] is path t's log
 * weight and pidx[prow[t] .. prow[t + 1]) its Fsa parameter ids in path order,
 * repeats kept, as best_paths_get gives them.  A string with m < k accepting
 * paths of finite weight has m paths (an unrecognized string none): a weight
 * of -inf never enters a list.
 * Paths are ordered by (weight descending, in-edge ascending, rank of the
 * prefix at the source ascending) at every node, and by (weight descending,
 * end node ascending, end edge ascending, rank ascending) at the end.  The
 * order is total and does not depend on k, and a weight is one left-to-right
 * sum, so the first j paths of a k result are the j result bit for bit, and
 * the k = 1 result is best_paths' result bit for bit.
 * Valid until the next load or kbest_paths call; a best_paths result and a
 * kbest_paths result do not invalidate each other.  Local to the rank, and
 * leaves the learning path untouched, as best_paths does.  Errors as for
 * best_paths (WFSA_ERR_ARG before a model and a corpus are loaded, while an
 * evaluation is in flight and in matrix-file mode; WFSA_ERR_CAPACITY on the
 * dense path and when one string's scratch exceeds the budget); k outside
 * 1 .. WFSA_KBEST_MAX is WFSA_ERR_ARG. */
#define WFSA_KBEST_MAX 16
int wfsa_dev_kbest_paths(wfsa_dev* ctx, const double* w_full, int32_t k, int64_t* n_paths, int64_t* n_entries);
int wfsa_dev_kbest_paths_get(wfsa_dev* ctx, int64_t* srow /* [n_strings + 1] */, double* logw /* [n_paths] */,
                             int64_t* prow /* [n_paths + 1] */, int32_t* pidx /* [n_entries] */);

/* Posterior path sampling: n independent draws per loaded string from
 * P(path | string) = exp(w(path)) / q_s at w_full, 1 <= n <= WFSA_SAMPLE_MAX --
 * best_paths' trellis walk with log-sum-exp in place of max: a forward pass in
 * the log domain whose rows are kept per position (so a q_s below the double
 * range loses nothing), then n walks back from the end, each choosing its end
 * edge and then its in-edge per position by inverse CDF (sample.hip).
 *   logq[s]    = log q_s from that forward pass, -inf when the string has no
 *                accepting path of finite weight (NULL allowed);
 *   *n_paths   = samples over all strings (NULL allowed);
 *   *n_entries = total length of their parameter lists (NULL allowed).
 * sample_paths_get copies them out in kbest_paths_get's layout (any pointer may
 * be NULL): string s owns the paths srow[s] .. srow[s + 1], logw[t] is path t's
 * log weight and pidx[prow[t] .. prow[t + 1]) its Fsa parameter ids in path
 * order, repeats kept.  A string with an accepting path of finite weight owns
 * exactly n paths, in sample-index order (sample 0 first), unsorted, duplicates
 * possible; any other string owns none.  An edge of weight -inf, or a prefix of
 * mass 0, is never taken.  logw[t] is formed as the decoders form it (one
 * left-to-right sum of decode_edge_weight_kernel's edge log-weights): a sampled
 * path carries bit for bit the weight kbest_paths reports for it, and
 * exp(logw[t] - logq[s]) is the posterior mass of that path.
 *
 * Reproducibility.  The random numbers are Philox4x32-10 (multipliers
 * 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with key
 * (lo32(seed), hi32(seed)) and counter (lo32(s), hi32(s), t, d): s the string's
 * index among the loaded strings, t the sample index, d = 0 the choice of the
 * end edge and d = m (1 .. L) the choice of the in-edge into position
 * L + 1 - m.  One draw per choice: u = (((x0 << 32) | x1) >> 11) * 2^-53 from
 * output words 0 and 1.  A choice among candidates of masses a_i >= 0 takes the
 * first i whose running sum exceeds u * total (total: the sum in the same
 * order); if rounding leaves none, the last candidate of positive mass.  In-edges are candidates in e_ptr order, end
 * edges in (live slot, end edge) order, the decoders' tie order.  Hence two
 * calls with the same weights, n and seed return the same bytes; the first j
 * samples of every string in an n result are the j result byte for byte (a draw
 * depends neither on n nor on which wave or lane made it); to continue a sample
 * set, call again with another seed.
 *
 * Valid until the next load or sample_paths call; best_paths, kbest_paths and
 * sample_paths results do not invalidate each other.  Local to the rank (no
 * collective), and leaves the learning path untouched, as the decoders do.
 * WFSA_ERR_ARG for n outside 1 .. WFSA_SAMPLE_MAX, before a model and a corpus
 * are loaded, while an evaluation is in flight, in matrix-file mode, and from
 * _get without a result since the last load; WFSA_ERR_CAPACITY on the dense
 * path (load with WFSA_DENSE=0) and when one wave's scratch exceeds the 1 GiB
 * budget. */
#define WFSA_SAMPLE_MAX 64
int wfsa_dev_sample_paths(wfsa_dev* ctx, const double* w_full, int32_t n, uint64_t seed,
                          double* logq /* [n_strings], NULL allowed */, int64_t* n_paths, int64_t* n_entries /* NULL allowed */);
int wfsa_dev_sample_paths_get(wfsa_dev* ctx, int64_t* srow /* [n_strings + 1] */, double* logw /* [n_paths] */,
                              int64_t* prow /* [n_paths + 1] */, int32_t* pidx /* [n_entries] */);
/* Posterior path sampling on the dense path (stats.dense == 1), where no
 * trellis is built and wfsa_dev_sample_paths fails: n independent draws per
 * loaded string from P(path | string) at w_full, 1 <= n <= WFSA_SAMPLE_MAX, by
 * forward filter / backward sample over the row slots of the dense path
 * (dense_sample.hip).  Outputs as sample_paths gives them: logq[s] (-inf when
 * the string has no accepting path of finite weight; NULL allowed), *n_paths,
 * *n_entries (NULL allowed), and dense_sample_paths_get in kbest_paths_get's
 * layout (any pointer may be NULL).  A string with an accepting path of finite
 * weight owns exactly n paths, in sample-index order; every other string owns
 * none.  Parameter ids follow dense_best_paths_get's conventions: path order,
 * a transition before the emission it leads to, the end transition last,
 * single-member groups without an id; an empty string with a finite ^ -> $
 * edge has n copies of that edge as its paths.
 *
 * Forward.  The evaluation's own forward arithmetic at exp(w_full) (formed on
 * the device as objective_grad forms it): dense_weights_kernel, the split-K
 * RAW step GEMM and dense_fwd_epi_kernel per step, dense_final_kernel for
 * log q -- this flow whatever WFSA_DENSE_ENGINE says -- into buffers of the
 * sampler's own; the T x R x (np + pad) history of scaled alpha rows shares
 * its allocation with dense_best_paths' score history (scratch of both).  On a
 * context that runs the default engine logq equals objective_grad(w,
 * want_logq)'s log q byte for byte.
 *
 * Backward.  For sample t of string s with L bytes, draw d = 0 chooses the end
 * state among candidates of mass alpha_L[T] aend[T]; draw d = m (1 .. L - 1)
 * the state at byte L - m among candidates of mass alpha_{L-m}[S] A[S][T], T
 * the state chosen at byte L - m + 1; the ^ edge into byte 1 is one candidate
 * and takes no draw.  A row's scale is common to its candidates and cancels.
 * Draws are sample_paths' generator word for word (Philox4x32-10, key the
 * seed, counter (lo32(s), hi32(s), t, d), u from words 0 and 1).
 *
 * A choice.  Candidates in ascending state order over the np padded states
 * (padded states have mass 0), in groups of 64 consecutive states: a group's
 * sum is a fixed butterfly over its 64 members, total the left-to-right sum
 * of the group sums.  The group is the first whose running sum over the
 * group sums exceeds u * total; the state is the first of that group whose
 * running sum -- left to right over the members, from the running sum before
 * the group -- exceeds u * total and exceeds the sum before it.  If rounding
 * leaves none, the last member of positive mass (of the group; without a
 * group, of all candidates).  Left-to-right sums of non-negative terms never
 * decrease and a candidate is taken only where the sum grows, so a mass of 0
 * (an absent edge, a -inf weight, a padded state, an alpha of 0) is never
 * chosen.  If total == 0 (every product underflows) the lowest S with
 * alpha[S] > 0 and A[S][T] > 0 is taken.  The association depends neither on
 * n nor on the wave or lane that holds the sample: the same weights, n and
 * seed give the same bytes on every call, and the first j samples of an n
 * result are the j result byte for byte.
 *
 * logw[t] is the decoders' weight of the returned path, formed as
 * dense_best_paths forms best_logw (an edge: the sum from 0.0 over its present
 * parameters, transition then emission; the path: the sum from 0.0 over its
 * edges, the end edge last) -- bit for bit what kbest_paths reports for that
 * path under WFSA_DENSE=0; exp(logw[t] - logq[s]) is its posterior mass.
 * Against sample_paths under WFSA_DENSE=0: the same uniforms and the same
 * candidate order (in-edges by ascending source state, end nodes by ascending
 * state for a model that qualifies for the dense path), the CDFs equal up to
 * rounding (alpha * A here, exp(log alpha + lw - ...) there): a sample is the
 * same path in both unless one of its choices falls closer to a CDF boundary
 * than the two roundings differ.
 *
 * Needs a loaded model and corpus; no evaluation has to have run.  Local to
 * the rank; leaves evaluations, rmin, the QN loop, generate and the
 * dense_best_paths result untouched.  Valid until the next load or
 * dense_sample_paths call.  stats.sample_path_ms = device time of its kernels
 * (dense_sp_forward_ms + dense_sp_backward_ms).  WFSA_ERR_ARG when the model
 * is not on the dense path (use wfsa_dev_sample_paths), before a model and a
 * corpus are loaded, in matrix-file mode, while an evaluation is in flight,
 * for n outside 1 .. WFSA_SAMPLE_MAX, for a w_full entry that is NaN or +inf
 * (before any kernel runs), and from _get without a result since the last
 * load; WFSA_ERR_CAPACITY, naming the bytes, when the history cannot be
 * allocated or the fixed-size path output (2 n (total bytes + n_strings)
 * int32) exceeds 4 GiB. */
int wfsa_dev_dense_sample_paths(wfsa_dev* ctx, const double* w_full, int32_t n, uint64_t seed,
                                double* logq /* [n_strings], NULL ok */, int64_t* n_paths, int64_t* n_entries /* NULL ok */);
int wfsa_dev_dense_sample_paths_get(wfsa_dev* ctx, int64_t* srow /* [n_strings + 1] */, double* logw /* [n_paths] */,
                                    int64_t* prow /* [n_paths + 1] */, int32_t* pidx /* [n_entries] */);
/* Test entry: the device's generator without an automaton, out[d] = the uniform
 * of draw d = 0 .. n_draws - 1 of sample `sample` of string `string` under
 * `seed` (the counter and key above). */
int wfsa_dev_sample_uniforms(int device, uint64_t seed, int64_t string, int32_t sample, int32_t n_draws, double* out);

/* Posterior expected counts: the per-string E-step.  For every loaded string at
 * w_full, under P(path | string) = exp(w(path)) / q_s:
 *   logq[s]    = log q_s, -inf when the string has no accepting path of finite
 *                weight (NULL allowed);
 *   entropy[s] = -sum_path P log P >= 0 in nats, NaN where logq[s] = -inf (NULL
 *                allowed);
 *   *n_entries = entries of all rows (NULL allowed).
 * posterior_counts_get copies the sparse rows out (any pointer may be NULL): a
 * string of positive mass owns cidx[crow[s] .. crow[s + 1]), Fsa parameter ids
 * in ascending order, each with cval > 0, the expected number of times a path
 * of s uses that parameter (single-member groups carry no id, as everywhere);
 * any other string owns nothing.  sum_s p_s * row_s is minus the gradient of
 * the corpus log-likelihood before the constraints' projection, and
 * entropy[s] = logq[s] - row_s . w.
 *
 * Arithmetic (posterior.hip).  The forward pass is sample_paths': log alpha per
 * live node as the greatest term log alpha[src] + lw[edge] over its in-edges
 * plus the log of the sum of exp(term - greatest) in the model's in-edge order,
 * lw the decoders' edge log-weights; log q likewise over the end edges in (live
 * slot, end edge) order: logq equals sample_paths' logq byte for byte.  The
 * backward pass walks node posteriors from the last position down: in-edge e
 * into node k at position i carries the mass
 *   m_e = gamma_i[k] * exp(min(0, log alpha_{i-1}[src] + lw[e] - log alpha_i[k])),
 * an end edge exp(min(0, log alpha_L[k] + lw[x] - log q)); a mass of 0 (an edge
 * at -inf, a source of mass 0, an underflow) is skipped.  Every mass is rounded
 * ONCE to fixed point and added with integer atomics, so the result does not
 * depend on the order of arrival: node posteriors (<= 1) at 2^-62, counts at
 * 2^-F with F = 62 - ceil(log2((max_len + 1) * longest edge parameter list)),
 * the bound on any count (F = 62 when it is 1; 55 at 100).  A mass below half a
 * unit rounds to 0 and is not added.  A parameter is listed when its
 * accumulated fixed-point count is not 0; cval is that integer times 2^-F.
 * Entropy is the chain-rule sum of -m * (the clamped exponent) over the same
 * edges -- no cancellation -- per lane in a fixed order, then a butterfly sum.
 * A string with exactly one accepting path of finite weight has every mass
 * exp(0) = 1: its integer counts exactly and entropy exactly 0.
 *
 * Reproducibility: the same weights give the same bytes on every call,
 * whatever the number of waves in flight and whichever wave took which string;
 * the learning path's tiers play no part.
 *
 * Valid until the next load or posterior_counts call; best_paths, kbest_paths,
 * sample_paths and posterior_counts results do not invalidate each other.
 * Local to the rank (no collective), and leaves the learning path untouched,
 * as the decoders do.  WFSA_ERR_ARG before a model and a corpus are loaded,
 * while an evaluation is in flight, in matrix-file mode, and from _get without
 * a result since the last load; WFSA_ERR_CAPACITY on the dense path (load with
 * WFSA_DENSE=0), when one wave's scratch (the sampler's rows, two rows of
 * n_nodes posteriors and n_params counts) exceeds the 1 GiB budget, and when
 * the rows' entries exceed 4 GiB at 12 bytes an entry (a row is the union of
 * the parameters over the string's paths, so its length is known only after
 * the pass: the first call sizes the output for (total bytes + n_strings) * the
 * longest edge parameter list entries, a pass whose rows do not fit still
 * counts them, and one more pass at the exact size fills them in).
 * (Environment, for measurements: WFSA_POSTERIOR_WAVES caps
 * the waves in flight; WFSA_POSTERIOR_PHASES=1 runs the forward pass alone, =2
 * leaves out the row scan -- timing only, such a call leaves no result.) */
int wfsa_dev_posterior_counts(wfsa_dev* ctx, const double* w_full, double* logq /* [n_strings], NULL allowed */,
                              double* entropy /* [n_strings], NULL allowed */, int64_t* n_entries /* NULL allowed */);
int wfsa_dev_posterior_counts_get(wfsa_dev* ctx, int64_t* crow /* [n_strings + 1] */, int32_t* cidx /* [n_entries] */,
                                  double* cval /* [n_entries] */);

/* Per-byte state posteriors and the max-expected-accuracy (MEA) decode.  For a
 * loaded string s of L bytes at w_full, under P(path | s) = exp(w(path)) / q_s:
 *   mass[s, i, U], i = 1 .. L: the posterior probability that byte i of s lies
 *     inside an emission of Fsa state U (a state id in wfsa_model_desc
 *     numbering).  States with the empty emission emit no byte and never appear;
 *     for every byte the sum over U is 1.
 *   boundary[s, i]: the posterior probability that an emission ends with byte i;
 *     boundary[s, L] is 1, and a byte strictly inside a multi-byte emission on
 *     every path has boundary 0.
 *   MEA decode (decode != 0): the accepting path of finite weight that maximises
 *     score = sum_i mass[s, i, state of the path at byte i], the expected number
 *     of bytes the returned analysis attributes to the same state as a path drawn
 *     from the posterior; 0 < score <= L.
 * Outputs (every pointer may be NULL):
 *   logq[s]       log q_s, posterior_counts' logq byte for byte;
 *   boundary[b]   for corpus byte b = off[s] + i - 1;
 *   score[s], path_logw[s]  the MEA path's score and log weight (decode != 0
 *                 only; untouched otherwise);
 *   *n_entries    entries of all mass rows; *n_path_entries: total length of
 *                 the paths' parameter lists (0 without decode).
 * byte_marginals_get copies the sparse mass rows out: corpus byte b owns
 * midx[mrow[b] .. mrow[b + 1]), state ids ascending, each with mval > 0.
 * byte_marginals_path_get copies the MEA paths out in best_paths_get's layout
 * (pidx[prow[s] .. prow[s + 1]) the Fsa parameter ids of string s's path in path
 * order); WFSA_ERR_ARG when the last call had decode = 0.
 * A string without an accepting path of finite weight owns nothing: logq = -inf,
 * boundary NaN on its bytes, score NaN, path_logw -inf, empty rows, empty path.
 *
 * Arithmetic (marginals.hip).  posterior_counts' forward pass and backward gamma
 * recursion, restated: log alpha is the greatest term plus the log of the sum of
 * exp(term - greatest) in the model's in-edge order, log q likewise over the end
 * edges in (live slot, end edge) order; in-edge e into node k at position i
 * carries m_e = gamma_i[k] * exp(min(0, log alpha_{i-1}[src] + lw[e] - log
 * alpha_i[k])); every mass is rounded ONCE to a multiple of 2^-62 and added with
 * 64-bit integer atomics; a mass of 0 is skipped.  Being at node k at position i
 * means, for a state, that an emission of it ended with byte i, and for a chain
 * node that byte i lies inside the emission it spells: mass[s, i, U] is the
 * integer sum of the fixed-point gamma_i over the nodes U owns, clamped to 2^62,
 * and boundary[s, i] the integer sum over the state nodes, clamped likewise and
 * converted once.  A state is listed when its fixed-point sum is not 0; mval is
 * that integer times 2^-62.  Each sum is stored at a fixed address, a function
 * of the corpus alone (the prefix sum over the corpus bytes of the number of
 * distinct owner states among the byte's destinations, plus the state's rank
 * among them), so the same weights give the same bytes on every call, whatever
 * the number of waves in flight and whichever wave took which string.
 * The decode is best_paths' (max, +) pass with a node reward in place of the
 * edge weight: the reward of a destination at byte i is mass[s, i, its owner],
 * an in-edge is eligible when its log weight is finite and its source's score is
 * above -inf, and a destination's score is the best eligible source score plus
 * its reward (one add per position, left to right).  Ties: in-edges by (source
 * score descending, log weight descending, in-edge ascending); at the end by
 * (score descending, node ascending) over the nodes with a finite end edge, then
 * that node's end edges by (log weight descending, end edge ascending).
 * path_logw is the decoders' left-to-right sum of the edge log-weights: the path
 * carries bit for bit the weight kbest_paths reports for it.
 * A string with exactly one accepting path of finite weight has every mass
 * exactly 1.0, one entry per byte, boundaries exactly 0.0 or 1.0, score exactly
 * L, and best_paths' path.
 *
 * Valid until the next load or byte_marginals call; best_paths, kbest_paths,
 * sample_paths, posterior_counts and byte_marginals results do not invalidate
 * each other.  Local to the rank (no collective), and leaves the learning path
 * untouched, as the decoders do.  WFSA_ERR_ARG before a model and a corpus are
 * loaded, while an evaluation is in flight, in matrix-file mode, and from _get
 * without a result since the last load; WFSA_ERR_CAPACITY on the dense path
 * (load with WFSA_DENSE=0), when one wave's scratch (the sampler's rows, two
 * rows of n_nodes posteriors and, with decode, max_len x max_dst back-pointers)
 * exceeds the 1 GiB budget, and when the state sums (8 bytes each) exceed 4 GiB.
 * (Environment, for measurements: WFSA_MARGINAL_WAVES caps the waves in
 * flight.) */
int wfsa_dev_byte_marginals(wfsa_dev* ctx, const double* w_full, int32_t decode, double* logq /* [n_strings] */,
                            double* boundary /* [total_symbols] */, double* score /* [n_strings] */,
                            double* path_logw /* [n_strings] */, int64_t* n_entries, int64_t* n_path_entries);
int wfsa_dev_byte_marginals_get(wfsa_dev* ctx, int64_t* mrow /* [total_symbols + 1] */, int32_t* midx /* [n_entries] */,
                                double* mval /* [n_entries] */);
int wfsa_dev_byte_marginals_path_get(wfsa_dev* ctx, int64_t* prow /* [n_strings + 1] */, int32_t* pidx /* [n_path_entries] */);

/* Per-byte state posteriors and the MEA decode on the dense path (stats.dense
 * == 1), where no trellis is built and wfsa_dev_byte_marginals fails
 * (dense_marginals.hip).  On the dense path every interior state emits exactly
 * one byte, so byte i of string s has one state on every path, and
 *   mass[s, i, U] = P(the path is in Fsa state U at byte i | s),
 * summing to 1 over U for every byte; the boundary after every byte is 1 and
 * is not an output.  rows != 0 asks for the mass rows, decode != 0 for the MEA
 * path of every string; at least one must be set.  rows = 0, decode = 1 is the
 * decode alone: no row output, no 4 GiB rule.
 * Outputs (every pointer may be NULL):
 *   logq[s]       log q_s: dense_sample_paths' log q -- the evaluation's forward
 *                 pass (DensePath::enqueue_forward_into, engine 2's flow whatever
 *                 WFSA_DENSE_ENGINE says) into buffers of the call's own, the
 *                 scaled alpha rows in the history dense_best_paths and
 *                 dense_sample_paths share (scratch of all three).  On a context
 *                 that runs the default engine it equals objective_grad(w,
 *                 want_logq)'s log q byte for byte;
 *   score[s], path_logw[s]  the MEA path's score and log weight (decode != 0
 *                 only; untouched otherwise);
 *   *n_entries    entries of all mass rows (0 with rows = 0); *n_path_entries
 *                 the total length of the paths' parameter lists (0 without
 *                 decode).
 * dense_byte_marginals_get copies the rows out in byte_marginals_get's layout:
 * corpus byte b = off[s] + i - 1 owns midx[mrow[b] .. mrow[b + 1]), Fsa state
 * ids in wfsa_model_desc numbering, ascending, each with 0 < mval <= 1;
 * WFSA_ERR_ARG when the last call had rows = 0.  dense_byte_marginals_path_get
 * copies the MEA paths out in dense_best_paths_get's layout and conventions
 * (pidx[prow[s] .. prow[s + 1]): Fsa parameter ids in path order, a transition
 * before the emission it leads to, the end transition last, single-member
 * groups without an id); WFSA_ERR_ARG when the last call had decode = 0.
 *
 * Masses.  Behind the forward pass the evaluation's own backward pass runs with
 * p = 1 (DensePath::enqueue_backward_into: the split-K RAW GEMM against A^T and
 * dense_bwd_epi_kernel per step, no gradient GEMM), so for the byte at step t
 * of row slot r and interior state T
 *   gamma = alpha_t[T] * beta_t[T] * exp(la_t + lb_t - log q_s)
 * in the evaluation's scaled arithmetic, written over alpha in the history (the
 * backward recursion never reads alpha).  The stored mass is min(gamma, 1.0); a
 * state is listed when that value is > 0.  The interior states keep their order
 * (the table from interior index to state id is built at model load), padded
 * states and idle rows never appear.  Exactness for strings with one path is
 * NOT promised, unlike byte_marginals': a mass of 1 comes out as the rounded
 * product above, within 3e-11 * max(1, |log q_s|) * (L_s + 1) of 1.
 * Rows.  One wavefront per corpus byte counts the byte's listed states (ballot
 * and popcount over 64 states at a time), the host takes the prefix sum
 * (mrow), and a second kernel writes every listed state at mrow[b] + the number
 * of listed states below it: the rows do not depend on which wave took which
 * byte.  More than 4 GiB of rows at 12 bytes an entry is refused with
 * WFSA_ERR_CAPACITY and the byte count before the rows are allocated, and the
 * call leaves no result; the caller slices the corpus, as for byte_marginals.
 *
 * MEA decode: the accepting path that maximises score = sum_i reward_i[state at
 * byte i], reward the stored mass (the clamped double; 0.0 for an unlisted
 * state).  Eligibility is read from the log tables dense_decode_tables_kernel
 * writes (into tables of the call's own): an edge, emission, start or end is
 * eligible when its entry is above -inf -- best_paths' notion of a finite
 * weight, no exp involved.
 *   D_1[T] = reward_1[T] where ^ -> T is eligible and T may emit byte 1;
 *   D_j[T] = (max over S with S -> T eligible of D_{j-1}[S]) + reward_j[T]
 *            where T may emit byte j; everything else is -inf.
 * The max is taken first, then one add per byte: score is one left-to-right
 * sum.  The pass is dense_best_paths' tile, T launches, every D_t kept -- over
 * gamma in the history once the rows are out, so the decode needs no second
 * history.  Back-track without back-pointers: the end state is the arg max of
 * D_L over the states with an eligible end edge, each predecessor the arg max
 * of D_{j-1}[S] over the S with S -> T eligible; ties go to the LOWEST state, a
 * -inf candidate is never taken.  score[s] = D_L[end state]; path_logw[s] is
 * the decoders' sum as dense_best_paths forms best_logw, bit for bit what
 * kbest_paths reports for that path under WFSA_DENSE=0.  With rows = 0 the
 * rewards are the same doubles, so paths, scores and weights are the bytes of
 * a rows = 1 call.
 * Ties against byte_marginals (WFSA_DENSE=0): there the order is source score,
 * then log weight descending, then in-edge ascending; here source score, then
 * lowest state.  At exact score ties the two tiers may return different paths
 * of equal score.
 *
 * A string with log q = -inf owns nothing: empty rows, score NaN, path_logw
 * -inf, empty path -- also where the log tables alone would find a route (exp
 * underflow).  The empty string has no rows; with a finite ^ -> $ edge its path
 * is that edge, its score 0.0 and its weight the edge's, as byte_marginals
 * returns them.
 *
 * The rows, paths, scores and weights are copied out of the history during the
 * call: a later dense_best_paths or dense_sample_paths call does not invalidate
 * the result, and this call invalidates neither of theirs.  Evaluations, rmin,
 * the QN loop, generate and captured graphs are untouched; local to the rank.
 * Valid until the next load or dense_byte_marginals call.  stats.byte_marginal_ms
 * = dense_bm_forward_ms + dense_bm_backward_ms + dense_bm_rows_ms +
 * dense_bm_decode_ms.  WFSA_ERR_ARG when the model is not on the dense path
 * (use wfsa_dev_byte_marginals), before a model and a corpus are loaded, in
 * matrix-file mode, while an evaluation is in flight, for rows == 0 && decode
 * == 0, for a w_full entry that is NaN or +inf (before any kernel runs), and
 * from _get / _path_get without a result since the last load;
 * WFSA_ERR_CAPACITY, naming the bytes, when the history or the rows cannot be
 * allocated or the rows exceed 4 GiB. */
int wfsa_dev_dense_byte_marginals(wfsa_dev* ctx, const double* w_full, int32_t rows, int32_t decode,
                                  double* logq /* [n_strings] */, double* score /* [n_strings] */,
                                  double* path_logw /* [n_strings] */, int64_t* n_entries, int64_t* n_path_entries);
int wfsa_dev_dense_byte_marginals_get(wfsa_dev* ctx, int64_t* mrow /* [total_symbols + 1] */, int32_t* midx /* [n_entries] */,
                                      double* mval /* [n_entries] */);
int wfsa_dev_dense_byte_marginals_path_get(wfsa_dev* ctx, int64_t* prow /* [n_strings + 1] */, int32_t* pidx /* [n_path_entries] */);

/* Unconditional generation: n independent strings drawn from the automaton
 * itself at w_full, each with its path and weights.  The call needs a loaded
 * model only, no corpus, and no trellis: it walks the flattened state graph of
 * wfsa_model_desc (generate.hip), so it serves a model on the dense path too.
 *
 * The walk.  Sample i (0 <= i < n) starts at U = start with step m = 0.  Each
 * step makes two choices:
 *   - draw 2m chooses one of U's transitions tr_ptr[U] .. tr_ptr[U + 1], to V;
 *   - if V is `end`, the sample is complete (status 0);
 *   - otherwise draw 2m + 1 chooses one of V's emissions em_ptr[V] ..
 *     em_ptr[V + 1];
 *   - if its bytes would take the string past max_len, the sample is truncated
 *     (status 1) and that emission is not recorded (the transition into V,
 *     chosen before it, is);
 *   - else the bytes are appended, U = V and m += 1.
 * A choice.  The candidates have masses a_k = exp(w_full[param_k]); the member
 * of a single-member group (param = -1) has a_k = 1.0.  The running sums are
 * formed left to right in the model's order (one add per candidate, no fused
 * multiply-add), T is the last of them.  The choice takes the first k whose
 * running sum exceeds u * T; if rounding leaves none, the last candidate of
 * positive mass -- sample_paths' rule word for word.  No candidates, or T == 0,
 * leaves the sample dead (status 2): the model loses that mass.  A dead sample
 * keeps what was recorded before the choice that failed.  (The device finds k
 * by bisection in the running sums, which do not decrease and which a
 * candidate of mass 0 leaves unchanged: the same k.)
 * The draws.  u of draw d of sample i is sample_paths' generator with key
 * (lo32(seed), hi32(seed)) and counter (lo32(i), hi32(i), 0xFFFFFFFF, d): the
 * sample word 0xFFFFFFFF is one sample_paths (t < 64) never uses.
 *
 *   *total_bytes     = bytes of all samples (NULL allowed);
 *   *n_entries       = total length of their parameter lists (NULL allowed);
 *   status_counts[3] = samples complete, truncated, dead (NULL allowed).
 * generate_get copies the samples out (every pointer may be NULL): sample i's
 * bytes are sym[off[i] .. off[i + 1]); pidx[prow[i] .. prow[i + 1]) are the Fsa
 * parameter ids in path order, a transition before the emission it leads to,
 * repeats kept, single-member groups carrying no id (best_paths_get's
 * convention); logw[i] is the left-to-right sum of the chosen parameters'
 * weights, the decoders' path weight; logp[i] is the left-to-right sum of
 * w_k - log T over the choices (0 - log 1 for a single-member group), the log
 * probability of the walk itself, equal to logw when every group sums to 1;
 * status[i] as above.  A truncated or dead sample keeps the bytes, path, logw
 * and logp of the choices recorded before it stopped.
 *
 * Reproducibility.  The same weights, max_len and seed give the same bytes on
 * every call; sample i depends neither on n nor on which wave or lane walked
 * it, so the first j samples of an n result are the j result byte for byte.
 *
 * Valid until the next load or generate call.  It invalidates none of the
 * other results (best_paths, kbest_paths, sample_paths, posterior_counts,
 * byte_marginals) and none of them invalidates it.  Local to the rank (no
 * collective), and leaves the learning path untouched, as the decoders do.
 * WFSA_ERR_ARG before a model is loaded, in matrix-file mode, while an
 * evaluation is in flight, for n < 1, max_len < 0 or
 * 2 * n_states * (max_len + 1) >= 2^32 (the draw index is a 32-bit counter
 * word; a loaded model has no epsilon cycle, so no walk takes more than
 * n_states * (max_len + 1) steps), for a w_full entry that is NaN or +inf
 * (before any walk), and from _get without a result since the last load;
 * WFSA_ERR_CAPACITY when the bytes or the path entries exceed 4 GiB, and for
 * n >= 2^31. */
int wfsa_dev_generate(wfsa_dev* ctx, const double* w_full, int64_t n, int32_t max_len, uint64_t seed,
                      int64_t* total_bytes, int64_t* n_entries, int64_t status_counts[3]);
int wfsa_dev_generate_get(wfsa_dev* ctx, uint8_t* sym, int64_t* off /* [n + 1] */, double* logw /* [n] */, double* logp /* [n] */,
                          int8_t* status /* [n] */, int64_t* prow /* [n + 1] */, int32_t* pidx /* [n_entries] */);

/* Where each loaded string runs (after compilation): tier[s] = -1 compiled
 * stream (trivial words + bubbles), 0 / 1 LDS-slab traversal, 2 wide
 * traversal (global scratch), 3 dense MFMA path, 4 matrix-file mode. */
int wfsa_dev_string_tiers(wfsa_dev* ctx, int8_t* tier);

/* Per-iteration hot path.  w_full[n_params] = Learner::GetWeight(j)
 * (src/Learner.cpp:427-436): x[trim[j]], 0 or -inf.  Outputs:
 *   *loglik        = sum_s p_s log q_s
 *   grad_full[j]   = -sum_s p_s E_{path|s}[count_j]   (NULL allowed)
 *   logq[s]        = log q_s for the loaded strings     (NULL allowed)
 * A loaded string without an accepting path has logq[s] = -inf and makes
 * loglik -inf when p_s > 0; on the dense path it adds nothing to grad_full
 * either way and, with p_s = 0, nothing to loglik, and it does not disturb
 * the string packed behind it in its row slot.
 * With a communicator attached, loglik and grad_full are summed over ranks
 * (one RCCL all-reduce) and logq stays local. */
int wfsa_dev_objective_grad(wfsa_dev* ctx, const double* w_full, double* loglik,
                            double* grad_full, double* logq);
/* The same split in two so host work can overlap the device: _begin copies
 * w_full and enqueues the evaluation (plus the all-reduce) and returns;
 * _end waits and writes the outputs.  Exactly one _end per _begin. */
int wfsa_dev_objective_grad_begin(wfsa_dev* ctx, const double* w_full, int want_logq);
int wfsa_dev_objective_grad_end(wfsa_dev* ctx, double* loglik, double* grad_full, double* logq);
/* The host-mapped area _begin copies w_full into (n_params doubles; NULL
 * before a model is loaded; valid until the next load).  A caller may write
 * the weights there itself and pass w_full = NULL to _begin: one copy of
 * the weights fewer per evaluation (the host QN binding does).  Not while an
 * evaluation is in flight.  _begin accepts w_full = NULL only when this was
 * called since the previous _begin (else WFSA_ERR_ARG). */
double* wfsa_dev_weights_staging(wfsa_dev* ctx);

/* Device-resident QuasiNewton: QuasiNewtonLearner::OptimizationStep
 * (src/QuasiNewtonLearner.cpp:162-201) and the epoch loop (src/main.cpp:276-303)
 * with x, lambda and w_full kept in HBM -- one step = the objective/gradient
 * kernels at x, the (all-reduce), and a one-workgroup KKT-diagonal update that
 * writes the next step's weights; steps are enqueued ahead and the host only
 * reads each step's info row.
 *   qn_setup:     once after Trim: trim[n_full] = Learner::trimmed_weights,
 *                 ccol[n_params] = the constraint of each kept parameter (C),
 *                 plogp = sum p log p (over all ranks), InitCallback flag 32.
 *   qn_set_state: x[n_params], lambda[n_constraints] (after Init).
 *   qn_get_state: x, lambda and the last step's gradient (any may be NULL).
 *   qn_run:       up to max_steps steps; info_rows[7*s ..] gets step s's
 *                 GetOptimizationInfo row (KL, graderr, g_min, g_max, lambda_min,
 *                 rmin, rmin string -- both 0 unless info_rmin); stops after the step whose HaltCondition(tol) holds
 *                 (*status = 1) or whose info is not finite (*status = 2). */
typedef struct {
    int32_t n_params;
    int32_t n_constraints;
    const int32_t* trim;       /* [n_full]                                   */
    const int32_t* ccol;       /* [n_params]                                 */
    double plogp;
    int32_t exponential_lambda;
    int32_t info_rmin;         /* fill the rmin columns (wfsa_dev_rmin per step) */
} wfsa_qn_desc;
int wfsa_dev_qn_setup(wfsa_dev* ctx, const wfsa_qn_desc* desc);
int wfsa_dev_qn_set_state(wfsa_dev* ctx, const double* x, const double* lambda);
int wfsa_dev_qn_get_state(wfsa_dev* ctx, double* x, double* lambda, double* grad);
int wfsa_dev_qn_run(wfsa_dev* ctx, double eta, double tol, int32_t max_steps, double* info_rows,
                    int32_t* steps_done, int32_t* status);

/* Second-order term of the objective's Hessian for HessianLearner
 * (ComputeHf, src/HessianLearner.cpp:498-547; pattern as AssembleH :381-446):
 *   hf_setup: builds the pattern -- the pairs (j, k), j <= k, of Fsa
 *             parameters whose counts vary together on some string -- after the
 *             corpus is compiled (bubbles per bubble, traversal-tier strings
 *             per string over their equivocal parameters); fails
 *             (WFSA_ERR_CAPACITY) when a string has more than 512 equivocal
 *             parameters (on any rank), and on the dense path.  With a
 *             communicator the pattern is the union over the ranks and
 *             hf_eval's values are all-reduced.
 *   hf_pairs: the pattern, pairs[2 t], pairs[2 t + 1] (ascending).
 *   hf_eval:  values[t] = sum_s p_s Cov_s(count_j, count_k) at w_full
 *             (HessianLearner adds -values to H). */
int wfsa_dev_hf_setup(wfsa_dev* ctx, int64_t* n_pairs);
int wfsa_dev_hf_pairs(wfsa_dev* ctx, int32_t* pairs);
int wfsa_dev_hf_eval(wfsa_dev* ctx, const double* w_full, double* values);

/* Multi-GPU: one process per GPU.  Rank 0 creates the id, the launcher
 * broadcasts the 128 bytes, every rank attaches.  wfsa_dev_allreduce sums
 * `count` doubles of a host buffer in place over the ranks.
 * wfsa_dev_comm_local_id makes the id of an in-process group instead: up to
 * 16 contexts of ONE process, each driven by its own thread, on one device
 * or on peer-enabled devices; comm_init with that id attaches a member.  The
 * group combines the same values at the same points as RCCL (rank order,
 * blocking), so one GPU runs every multi-rank branch of the path. */
#define WFSA_COMM_ID_BYTES 128
int wfsa_dev_comm_unique_id(uint8_t id[WFSA_COMM_ID_BYTES]);
int wfsa_dev_comm_local_id(int nranks, uint8_t id[WFSA_COMM_ID_BYTES]);
int wfsa_dev_comm_init(wfsa_dev* ctx, int nranks, int rank, const uint8_t id[WFSA_COMM_ID_BYTES]);
int wfsa_dev_allreduce(wfsa_dev* ctx, double* host_buf, int64_t count);

/* Failure semantics across ranks.  A call that takes part in
 * collectives (recognize, objective_grad_begin/_end, qn_setup, qn_run,
 * hf_setup, hf_eval, rmin, allreduce) and fails on one rank for any reason
 * but a bad argument aborts that rank's communicator.  How the others hear
 * of it depends on the transport:
 *   - in-process group: poisoned -- every waiting member wakes with
 *     WFSA_ERR_RCCL now, a later one fails at entry;
 *   - peer sums (the per-step [LL, grad]): every member's peer area gets its
 *     poison word -- their next peer sum fails at entry;
 *   - host callback (gloo, MPI): a poisoned header exchange -- every member
 *     waiting in, or later entering, any collective fails at once;
 *   - RCCL: the communicator is aborted (ncclCommAbort), which does NOT wake
 *     the other processes' pending RCCL calls: each rank's host watchdog
 *     ends them (an asynchronous error, or no progress within
 *     WFSA_COMM_TIMEOUT_S, default 300 s), unless the peer path carried the
 *     call.
 * A peer sum whose wait gives up (WFSA_PEER_TIMEOUT_S, default 120 s)
 * poisons every area too and is reported as WFSA_ERR_RCCL at the next host
 * sync point, never as a NaN result.  wfsa_dev_comm_abort does the same for
 * a failure outside the library (the caller's own work between
 * collectives). */
int wfsa_dev_comm_abort(wfsa_dev* ctx, const char* why);

/* Test entry: the peer all-reduce kernel on one device, the other members'
 * areas local and written beforehand (no second process, no concurrency
 * needed).  mode 0: every member present, out[0] = max |sum - rank-order
 * sum|; 1: the last member never arrives, out[0] = NaN results (the call
 * must give up after timeout_s); 2: the area poisoned before the call, which
 * must fail at entry.  out[1] = status word, out[2] = poisoned areas,
 * out[3] = seconds the call took. */
int wfsa_dev_peer_selftest(int device, int nranks, int64_t n, double timeout_s, int mode, double out[4]);

/* A communicator over a host callback instead of RCCL (one process per rank,
 * several may share a GPU; e.g. torch.distributed over gloo, or MPI):
 * fn(user, buf, count, op) all-reduces a HOST buffer in place -- op 0: sum
 * of doubles, 1: min of doubles, 2: max of bytes -- and returns 0 on
 * success.  Called from the thread that drives ctx.  (New; the reference
 * has no multi-process path.)
 *
 * Sums of up to 65536 doubles (the per-iteration [LL, grad] and the other
 * small vectors) take the one-shot peer all-reduce when it is on: one
 * kernel stores the rank's vector into every member's receive slot over
 * xGMI (IPC-mapped device memory; the pointer itself in an in-process
 * group), raises a flag per chunk and sums the members' slots in rank
 * order -- stream-ordered, no host step.  On by default over RCCL, off
 * otherwise; WFSA_PEER=1 / 0 overrides.  The first such sum checks the
 * path on every rank and all ranks fall back to the transport when any
 * check fails (stats.comm_peer = -1).  Refused (stats.comm_peer = 0) for an
 * in-process group whose members share a device: nothing guarantees their
 * spinning kernels run concurrently there. */
typedef int (*wfsa_host_allreduce_fn)(void* user, void* buf, int64_t count, int32_t op);
int wfsa_dev_comm_init_host(wfsa_dev* ctx, int nranks, int rank, wfsa_host_allreduce_fn fn, void* user);

int wfsa_dev_get_stats(wfsa_dev* ctx, wfsa_dev_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* WFSA_DEV_H */

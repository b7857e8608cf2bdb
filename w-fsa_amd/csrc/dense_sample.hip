// Posterior path sampling on the dense path (wfsa_dev_dense_sample_paths;
// dense_path.hpp): n draws per loaded string from P(path | string), forward
// filter / backward sample over the row slots the evaluations use.
//
// Per call, on one stream:
//   dense_sample_exp      ewp = exp(w_full) on the device, as the evaluations'
//                         staging kernel forms it
//   the forward pass      DensePath::enqueue_forward_into: the evaluation's own
//                         kernels (weights, transpose, the split-K RAW step
//                         GEMM and dense_fwd_epi_kernel per step,
//                         dense_final_kernel) into the sampler's buffers;
//                         every step's scaled alpha row is kept
//   dense_sample_walk     one wavefront per (string, sample): the end state
//                         among the masses alpha_L[T] aend[T], then per byte
//                         the state S among alpha[S] A[S][T], T the state
//                         chosen one byte later -- row T of the transposed
//                         table, so both operands are read along rows.  A
//                         row's scale is common to its candidates and cancels.
//                         Then forward along the path: the parameter codes and
//                         the weight as the decoders form it (dense_decode.hip)
//
// A choice among np candidates of masses m[S] >= 0 in ascending S, with one
// uniform u (sample.hpp's generator):
//   - groups of 64 consecutive states, one per lane; a group's sum by a fixed
//     xor butterfly; total = the left-to-right sum of the group sums
//   - the group: the first whose running sum P (left to right over the group
//     sums) exceeds x = u total; the state: the first lane of that group
//     whose running sum -- left to right over the lanes, from the P before
//     the group -- exceeds x AND exceeds the sum before it
//   - when rounding leaves no such lane (or group): the last lane of positive
//     mass in the group (of all candidates)
//   - total == 0 (every product underflows): the lowest S with both factors
//     positive; none: the walk fails (at the end state: the string has no path)
// Sums of non-negative terms taken left to right never decrease, and a lane is
// taken only where its sum grows: a candidate of mass 0 -- no edge, a weight of
// -inf, a padded state, an alpha of 0 -- cannot be chosen.  Nothing in the
// association depends on n or on the wavefront that holds the sample.
#include "dense_path.hpp"

#include <algorithm>
#include <climits>

#include "sample.hpp"

namespace wfsa {

namespace {

constexpr int kSwWaves = 4;   // walk: wavefronts per block

__global__ __launch_bounds__(256) void dense_sample_exp_kernel(const double* __restrict__ w, double* __restrict__ ewp,
                                                               int32_t n) {
    for (int32_t i = int32_t(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += int32_t(gridDim.x * blockDim.x))
        ewp[i] = exp(w[i]);
}

struct WalkArgs {
    const double* alpha;      // [T][R][ldx] scaled forward rows
    const double* amat_t;     // [np][np] A^T: row T holds A[S][T] along S
    const double* aend;       // [np]
    const double* w;          // [n_params]
    const int32_t* code_a;    // [np][np]
    const int32_t* code_em;   // [vocab+1][np]
    const int32_t* code_s;    // [np]
    const int32_t* code_e;    // [np]
    const int32_t* meta;      // [T][R]
    const int32_t* end_at;    // [S]
    const int64_t* off;       // [S + 1]
    int32_t* states;          // [n total symbols]: sample t of string s from off[s] n + t L
    int32_t* codes;           // [2 n (total symbols + S)]
    double* logw;             // [S n]
    int64_t n_strings;
    uint64_t seed;
    int32_t n, np, ldx, R, code_se;
};

// the same sum in every lane: level by level the partner's partial is added,
// and a + b == b + a to the bit
__device__ __forceinline__ double wave_sum_butterfly(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One choice (the rule above) among the np products a[S] b[S]; the same value
// in every lane, -1: no candidate with both factors positive.
__device__ __forceinline__ int dense_sample_choose(const double* __restrict__ a, const double* __restrict__ b, int np,
                                                   double u, int lane) {
    // kGroups groups' loads are in flight together (np is a multiple of 128:
    // a batch may end past the row, those groups are skipped); the sums are
    // taken group by group in ascending order whatever the batch
    constexpr int kGroups = 4;
    double total = 0.0;
    int first = INT_MAX, last = -1;   // per lane: its lowest candidate with both factors positive, its highest of positive mass
    for (int c0 = 0; c0 < np; c0 += 64 * kGroups) {
        double av[kGroups], bv[kGroups];
#pragma unroll
        for (int q = 0; q < kGroups; ++q) {
            const int c = min(c0 + 64 * q, np - 64) + lane;
            av[q] = a[c];
            bv[q] = b[c];
        }
#pragma unroll
        for (int q = 0; q < kGroups; ++q) {
            const int g0 = c0 + 64 * q;
            if (g0 >= np) break;
            const double m = av[q] * bv[q];
            total += wave_sum_butterfly(m);
            first = min(first, av[q] > 0.0 && bv[q] > 0.0 ? g0 + lane : INT_MAX);
            last = m > 0.0 ? g0 + lane : last;
        }
    }
    if (!(total > 0.0)) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        return first == INT_MAX ? -1 : first;
    }
    const double x = u * total;
    double P = 0.0, msel = 0.0;
    int gsel = -1;   // the group's first state
    for (int c0 = 0; gsel < 0 && c0 < np; c0 += 64 * kGroups) {
        double m[kGroups];
#pragma unroll
        for (int q = 0; q < kGroups; ++q) {
            const int c = min(c0 + 64 * q, np - 64) + lane;
            m[q] = a[c] * b[c];
        }
#pragma unroll
        for (int q = 0; q < kGroups; ++q) {
            const int g0 = c0 + 64 * q;
            if (g0 >= np || gsel >= 0) break;
            const double P2 = P + wave_sum_butterfly(m[q]);
            if (P2 > x) {
                gsel = g0;
                msel = m[q];
            } else {
                P = P2;
            }
        }
    }
    if (gsel < 0) {   // rounding left no group: the last candidate of positive mass
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
        return last;
    }
    double r = P;
    for (int k = 0; k < 64; ++k) {
        const double r2 = r + __shfl(msel, k, 64);
        if (r2 > x && r2 > r) return gsel + k;
        r = r2;
    }
    // rounding left no member: the group's last of positive mass (P + its sum > P: it has one)
    return gsel + 63 - __clzll(__ballot(msel > 0.0));
}

__global__ __launch_bounds__(kSwWaves * 64) void dense_sample_walk_kernel(WalkArgs a) {
    const int lane = int(threadIdx.x) & 63;
    // (string, sample) items, fewer than 2^31: the entry point caps the output at 4 GiB
    const uint32_t wave0 = blockIdx.x * kSwWaves + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * kSwWaves, n_items = uint32_t(a.n_strings) * uint32_t(a.n);
    const size_t np = size_t(a.np), ldx = size_t(a.ldx);
    for (uint32_t item = wave0; item < n_items; item += n_waves) {
        const int64_t s = int64_t(item / uint32_t(a.n));
        const int32_t t = int32_t(item % uint32_t(a.n));
        const int64_t o0 = a.off[s], L = a.off[s + 1] - o0;
        int32_t* cd = a.codes + 2 * ((o0 + s) * int64_t(a.n) + int64_t(t) * (L + 1));
        int32_t* st = a.states + o0 * int64_t(a.n) + int64_t(t) * L;
        const int32_t at = a.end_at[s];
        if (at < 0) {   // the empty string: the ^ -> $ edge or nothing
            if (lane == 0) {
                double lw = 0.0;
                if (a.code_se >= 0) lw += a.w[a.code_se];
                const double total = 0.0 + lw;
                const bool ok = a.code_se != kCodeNone && total > -INFINITY;
                cd[0] = ok ? a.code_se : kCodeNone;
                cd[1] = kCodeOne;
                a.logw[item] = ok ? total : -INFINITY;
            }
            continue;
        }
        const int64_t t_end = at / a.R, r = at % a.R;
        // backward: draw 0 the state at the last byte (against aend), draw m the state m
        // bytes before it (against row `cur` of A^T); byte j's state is kept by lane
        // j & 63, which alone reads it again
        int cur = 0;
        for (int64_t j = L - 1; j >= 0; --j) {
            const double* row = a.alpha + (size_t(t_end - (L - 1) + j) * size_t(a.R) + size_t(r)) * ldx;   // alpha at byte j
            const double* col = j == L - 1 ? a.aend : a.amat_t + size_t(cur) * np;
            cur = dense_sample_choose(row, col, a.np, sample_uniform(a.seed, uint64_t(s), uint32_t(t), uint32_t(L - 1 - j)), lane);
            if (cur < 0) break;
            if (lane == int(j & 63)) st[j] = cur;
        }
        if (cur < 0) {   // no accepting path of positive mass
            if (lane == 0) {
                cd[0] = kCodeNone;
                a.logw[item] = -INFINITY;
            }
            continue;
        }
        // forward along the path, 64 edges at a time (edge L: the end edge):
        // the codes, and the weight summed left to right over the edges
        double total = 0.0;
        int carry = -1;
        for (int64_t j0 = 0; j0 <= L; j0 += 64) {
            const int64_t j = j0 + lane;
            const int T = j < L ? st[j] : -1;
            int prev = __shfl_up(T, 1, 64);
            if (lane == 0) prev = carry;
            carry = __shfl(T, 63, 64);
            int32_t ct = kCodeNone, ce = kCodeOne;
            if (j < L) {
                const int sym = a.meta[size_t(t_end - L + 1 + j) * size_t(a.R) + size_t(r)] & 0x1ff;
                ct = j == 0 ? a.code_s[T] : a.code_a[size_t(prev) * np + size_t(T)];
                ce = a.code_em[size_t(sym) * np + size_t(T)];
            } else if (j == L) {
                ct = a.code_e[prev];
            }
            double lw = 0.0;
            if (ct >= 0) lw += a.w[ct];
            if (ce >= 0) lw += a.w[ce];
            if (j <= L) {
                cd[2 * j] = ct;
                cd[2 * j + 1] = ce;
            }
            const int cnt = int(L + 1 - j0 < 64 ? L + 1 - j0 : 64);
            for (int k = 0; k < cnt; ++k) total += __shfl(lw, k, 64);
        }
        if (lane == 0) a.logw[item] = total;
    }
}

template <typename T>
hipError_t dalloc(T*& p, size_t n) {
    if (p) (void)hipFree(p);
    p = nullptr;
    return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T));
}

#define DTRY(x)                                     \
    do {                                            \
        const hipError_t e_ = (x);                  \
        if (e_ != hipSuccess) return e_;            \
    } while (0)

}  // namespace

size_t DensePath::sample_paths_output_bytes(int32_t n) const {
    return 2 * size_t(n) * (size_t(total_sym_) + size_t(n_strings_)) * sizeof(int32_t);
}

hipError_t DensePath::enqueue_sample_paths(const double* w_full, int32_t n, uint64_t seed, hipEvent_t const ev[3],
                                           hipStream_t s) {
    const size_t np = size_t(np_), R = size_t(R_), S = size_t(n_strings_), N = size_t(n);
    if (!fs_amat_) {   // first call since the load: the pass's buffers
        DTRY(dalloc(fs_w_, size_t(n_params_)));
        DTRY(dalloc(fs_ewp_, size_t(n_params_)));
        DTRY(dalloc(fs_amat_t_, np * np));
        DTRY(dalloc(fs_et_, size_t(vocab_ + 1) * np));
        DTRY(dalloc(fs_a0_, np));
        DTRY(dalloc(fs_aend_, np));
        DTRY(dalloc(fs_la_, size_t(T_) * R));
        DTRY(dalloc(fs_sum_, 2 * R));
        DTRY(dalloc(fs_ysplit_, R * size_t(ldx_)));
        DTRY(dalloc(fs_logq_, S));
        DTRY(dalloc(fs_ll_, size_t(std::max(n_ll_, 1))));
        DTRY(dalloc(fs_amat_, np * np));
    }
    if (fs_n_ < n) {
        fs_n_ = 0;
        DTRY(dalloc(fs_states_, N * size_t(total_sym_)));
        DTRY(dalloc(fs_codes_, 2 * N * (size_t(total_sym_) + S)));
        DTRY(dalloc(fs_logw_, N * S));
        fs_n_ = n;
    }
    DTRY(history_alloc());
    if (n_params_ > 0) DTRY(hipMemcpyAsync(fs_w_, w_full, size_t(n_params_) * sizeof(double), hipMemcpyHostToDevice, s));
    DTRY(hipEventRecord(ev[0], s));
    if (n_params_ > 0) {
        const unsigned blocks = unsigned(std::min<int32_t>(64, (n_params_ + 255) / 256));
        dense_sample_exp_kernel<<<blocks, 256, 0, s>>>(fs_w_, fs_ewp_, n_params_);
        DTRY(hipGetLastError());
    }
    ForwardBufs b{};
    b.amat = fs_amat_; b.amat_t = fs_amat_t_; b.et = fs_et_; b.a0 = fs_a0_; b.aend = fs_aend_;
    b.alpha = dhist_; b.la = fs_la_; b.sum = fs_sum_; b.ysplit = fs_ysplit_; b.logq = fs_logq_; b.ll_part = fs_ll_;
    DTRY(enqueue_forward_into(fs_ewp_, b, s));
    DTRY(hipEventRecord(ev[1], s));
    if (S > 0) {
        WalkArgs k{};
        k.alpha = dhist_; k.amat_t = fs_amat_t_; k.aend = fs_aend_; k.w = fs_w_;
        k.code_a = code_a_; k.code_em = code_em_; k.code_s = code_s_; k.code_e = code_e_;
        k.meta = meta_; k.end_at = end_at_; k.off = doff_;
        k.states = fs_states_; k.codes = fs_codes_; k.logw = fs_logw_;
        k.n_strings = n_strings_;
        k.seed = seed;
        k.n = n; k.np = np_; k.ldx = ldx_; k.R = R_; k.code_se = code_se_;
        const int64_t want = (int64_t(S) * n + kSwWaves - 1) / kSwWaves;
        const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(want, int64_t(n_cu_) * 8)));
        dense_sample_walk_kernel<<<grid, kSwWaves * 64, 0, s>>>(k);
        DTRY(hipGetLastError());
    }
    return hipEventRecord(ev[2], s);
}

hipError_t DensePath::sample_paths_download(int32_t n, double* logq, double* logw, int32_t* codes, hipStream_t s) const {
    const size_t S = size_t(n_strings_), N = size_t(n);
    if (S == 0) return hipSuccess;
    DTRY(hipMemcpyAsync(logq, fs_logq_, S * sizeof(double), hipMemcpyDeviceToHost, s));
    DTRY(hipMemcpyAsync(logw, fs_logw_, N * S * sizeof(double), hipMemcpyDeviceToHost, s));
    return hipMemcpyAsync(codes, fs_codes_, 2 * N * (size_t(total_sym_) + S) * sizeof(int32_t), hipMemcpyDeviceToHost, s);
}

}  // namespace wfsa

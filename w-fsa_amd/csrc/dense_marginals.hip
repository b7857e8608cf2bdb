// Per-byte state posteriors and the max-expected-accuracy (MEA) decode on the
// dense path (wfsa_dev_dense_byte_marginals; dense_path.hpp), over the row
// slots the evaluations use.
//
// Per call, on one stream:
//   dense_bm_exp          ewp = exp(w_full) on the device, as the evaluations'
//                         staging kernel forms it
//   the forward pass      DensePath::enqueue_forward_into: the evaluation's own
//                         kernels into buffers of the feature's own, every
//                         step's scaled alpha row kept in the shared history
//   the backward pass     DensePath::enqueue_backward_into: the evaluation's
//                         split-K RAW GEMM against A^T and dense_bwd_epi_kernel
//                         per step with p = 1; gamma = alpha beta
//                         exp(la + lb - log q) is written over alpha
//   dense_bm_count        one wavefront per corpus byte: the interior states
//                         whose stored mass min(gamma, 1) is > 0, counted 64 at
//                         a time by ballot and popcount; the prefix sum over
//                         the bytes is the host's
//   dense_bm_fill         the same walk again: a listed state's entry is the
//                         byte's first plus the number of listed states below
//                         it (popcount of the ballot under the lane), so the
//                         rows ascend by state and no address depends on the
//                         wave that took the byte
//   dense_decode_tables   (dense_decode.hip) the log tables into tables of the
//                         feature's own: an edge, emission, start or end is
//                         eligible when its entry is above -inf
//   dense_bm_mask         lA -> 0.0 where eligible, -inf elsewhere
//   dense_bm_maxplus x T  D_t[r][T] = max_S (D_{t-1}[r][S] + mask[S][T]) + reward
//                         where T may emit the byte; 0.0 + reward where a string
//                         starts and ^ -> T is eligible; -inf elsewhere.  Adding
//                         the mask's 0.0 is exact, so the score is one add per
//                         byte.  reward = min(gamma, 1), read from the element
//                         of the history D_t is then written to (the thread
//                         that owns the element reads it first)
//   dense_bm_backtrack    one wavefront per string: the end state maximises
//                         D_L over the states with an eligible end edge, every
//                         predecessor D_{j-1}[S] over the S with S -> T
//                         eligible; ties to the lowest state, a -inf candidate
//                         never taken, no back-pointers; then the codes and the
//                         weight as dense_backtrack_kernel's forward walk forms
//                         them
#include "dense_path.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace wfsa {

namespace {

constexpr int kT = kDenseTile;   // 128
constexpr int kMxK = 16;         // K slice of the max-plus tile
constexpr int kBtWaves = 4;      // back-track: wavefronts per block
constexpr int kRowWaves = 4;     // count / fill: wavefronts per block

__global__ __launch_bounds__(256) void dense_bm_exp_kernel(const double* __restrict__ w, double* __restrict__ ewp, int32_t n) {
    for (int32_t i = int32_t(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += int32_t(gridDim.x * blockDim.x))
        ewp[i] = exp(w[i]);
}

__global__ __launch_bounds__(256) void dense_bm_mask_kernel(double* la, int64_t n) {
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
        la[i] = la[i] > -INFINITY ? 0.0 : -INFINITY;
}

struct RowArgs {
    const double* gam;         // [T][R][ldx] the history: gamma
    const int32_t* rowof;      // [n_bytes] t R + r of the byte
    const int32_t* state_id;   // [n_states]
    const int64_t* mrow;       // [n_bytes + 1] (fill)
    int32_t* cnt;              // [n_bytes] (count)
    int32_t* midx;             // [entries] (fill)
    double* mval;              // [entries] (fill)
    int64_t n_bytes;
    int32_t n_states, ldx;
};

// One wavefront per corpus byte, 64 consecutive states per load (a full
// 512-byte row segment); FILL = false counts the listed states, FILL = true
// writes them from mrow[byte] on in ascending state order.
template <bool FILL>
__global__ __launch_bounds__(kRowWaves * 64) void dense_bm_rows_kernel(RowArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t wave0 = int64_t(blockIdx.x) * kRowWaves + (int(threadIdx.x) >> 6);
    const int64_t n_waves = int64_t(gridDim.x) * kRowWaves;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t b = wave0; b < a.n_bytes; b += n_waves) {
        const double* row = a.gam + size_t(a.rowof[b]) * size_t(a.ldx);
        int64_t at = FILL ? a.mrow[b] : 0;
        for (int c0 = 0; c0 < a.n_states; c0 += 64) {
            const int c = c0 + lane;
            const double m = c < a.n_states ? fmin(row[c], 1.0) : 0.0;   // the stored mass
            const bool listed = m > 0.0;
            const unsigned long long any = __ballot(listed);
            if (FILL && listed) {
                const int64_t o = at + __popcll(any & below);
                a.midx[o] = a.state_id[c];
                a.mval[o] = m;
            }
            at += __popcll(any);
        }
        if (!FILL && lane == 0) a.cnt[b] = int32_t(at);
    }
}

struct RewardArgs {
    const double* x;        // [R][ldx] D_{t-1} (unused at step 0)
    const double* mask;     // [np][np] 0.0: S -> T eligible, -inf: not
    const double* le;       // [vocab+1][np] log tables: eligibility alone is read
    const double* l0;       // [np]
    const int32_t* meta;    // [R] this step
    double* y;              // [R][ldx] gamma_t in, D_t out
    int32_t np, ldx, vocab;
};

// One step of the reward (max, +) trellis for all R row slots:
// dense_maxplus_kernel's tile (dense_decode.hip) -- 128 x 128 per block, 8 x 8
// per thread at stride 16, K staged through 32 KB of LDS in slices of 16 with
// the next slice's loads in registers -- over rows of the evaluations' pitch,
// with the mask in place of lA and the element's own gamma as the reward.
template <bool FIRST>
__global__ __launch_bounds__(256) void dense_bm_maxplus_kernel(RewardArgs a) {
    __shared__ double xs[kMxK][kT + 1];   // [k][row]
    __shared__ double ls[kMxK][kT];       // [k][column]
    const int tid = int(threadIdx.x), tx = tid & 15, ty = tid >> 4;
    const int c0 = int(blockIdx.x) * kT, r0 = int(blockIdx.y) * kT;
    const size_t np = size_t(a.np), ldx = size_t(a.ldx);
    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = -INFINITY;
    if (!FIRST) {
        const int xr = tid >> 1, xk = (tid & 1) * 8, lk = tid >> 4, lc = (tid & 15) * 8;
        const double2* xp = reinterpret_cast<const double2*>(a.x + size_t(r0 + xr) * ldx + size_t(xk));
        const double2* lp = reinterpret_cast<const double2*>(a.mask + size_t(lk) * np + size_t(c0 + lc));
        const size_t lstep = kMxK * np / 2;   // double2 per K slice of the mask
        double2 xv[4], lv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xv[q] = xp[q];
            lv[q] = lp[q];
        }
        for (int k0 = 0; k0 < a.np; k0 += kMxK) {
            __syncthreads();   // the previous slice's reads are done
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                xs[xk + 2 * q][xr] = xv[q].x;
                xs[xk + 2 * q + 1][xr] = xv[q].y;
                ls[lk][lc + 2 * q] = lv[q].x;
                ls[lk][lc + 2 * q + 1] = lv[q].y;
            }
            __syncthreads();
            if (k0 + kMxK < a.np) {
                xp += kMxK / 2;
                lp += lstep;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    xv[q] = xp[q];
                    lv[q] = lp[q];
                }
            }
#pragma unroll 4
            for (int kk = 0; kk < kMxK; ++kk) {
                double xa[8], lb[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) xa[i] = xs[kk][ty + 16 * i];
#pragma unroll
                for (int j = 0; j < 8; ++j) lb[j] = ls[kk][tx + 16 * j];
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[i][j] = fmax(acc[i][j], xa[i] + lb[j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = r0 + ty + 16 * i;
        const int32_t m = a.meta[r];
        const int sym = m & 0x1ff;
        const bool idle = sym >= a.vocab, start = FIRST || ((m >> 9) & 1);
        double* yr = a.y + size_t(r) * ldx;
        const double* le = a.le + size_t(idle ? a.vocab : sym) * np;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int T = c0 + tx + 16 * j;
            const double reward = fmin(yr[T], 1.0);
            const bool ok = !idle && le[T] > -INFINITY && (!start || a.l0[T] > -INFINITY);
            yr[T] = ok ? (start ? 0.0 : acc[i][j]) + reward : -INFINITY;
        }
    }
}

struct BacktrackArgs {
    const double* hist;       // [T][R][ldx] D
    const double* lat;        // [np][np] lAT[T][S]
    const double* lend;       // [np]
    const double* w;          // [n_params]
    const double* logq;       // [S]
    const int32_t* code_a;    // [np][np]
    const int32_t* code_em;   // [vocab+1][np]
    const int32_t* code_s;    // [np]
    const int32_t* code_e;    // [np]
    const int32_t* meta;      // [T][R]
    const int32_t* end_at;    // [S]
    const int64_t* off;       // [S + 1]
    int32_t* states;          // [total symbols]
    int32_t* codes;           // [2 (total symbols + S)]
    double* logw;             // [S]
    double* score;            // [S]
    int64_t n_strings;
    int32_t np, ldx, R, code_se;
};

// the wave's maximum of (v, i): ties to the lower index; i = INT_MAX: no candidate above -inf
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double v2 = __shfl_xor(v, o, 64);
        const int i2 = __shfl_xor(i, o, 64);
        if (v2 > v || (v2 == v && i2 < i)) {
            v = v2;
            i = i2;
        }
    }
}

// arg max over the eligible c (el[c] > -inf) of row[c]
__device__ __forceinline__ void eligible_argmax(const double* __restrict__ row, const double* __restrict__ el, int np, int lane,
                                                double& best, int& arg) {
    best = -INFINITY;
    arg = INT_MAX;
    for (int c = lane; c < np; c += 64) {
        const double v = el[c] > -INFINITY ? row[c] : -INFINITY;
        if (v > best) {
            best = v;
            arg = c;
        }
    }
    wave_argmax(best, arg);
}

__global__ __launch_bounds__(kBtWaves * 64) void dense_bm_backtrack_kernel(BacktrackArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t wave0 = int64_t(blockIdx.x) * kBtWaves + (int(threadIdx.x) >> 6);
    const int64_t n_waves = int64_t(gridDim.x) * kBtWaves;
    const size_t np = size_t(a.np), ldx = size_t(a.ldx);
    const double nan = __builtin_nan("");
    for (int64_t s = wave0; s < a.n_strings; s += n_waves) {
        const int64_t o0 = a.off[s], L = a.off[s + 1] - o0;
        int32_t* cd = a.codes + 2 * (o0 + s);
        const int32_t at = a.end_at[s];
        const bool has = a.logq[s] > -INFINITY;   // a string of mass 0 owns nothing, whatever the mask would find
        if (at < 0 || !has) {   // the empty string: the ^ -> $ edge or nothing, score 0.0
            if (lane == 0) {
                double lw = 0.0;
                if (a.code_se >= 0) lw += a.w[a.code_se];
                const double total = 0.0 + lw;
                const bool ok = has && at < 0 && a.code_se != kCodeNone && total > -INFINITY;
                cd[0] = ok ? a.code_se : kCodeNone;
                cd[1] = kCodeOne;
                a.logw[s] = ok ? total : -INFINITY;
                a.score[s] = ok ? 0.0 : nan;
            }
            continue;
        }
        const int64_t t_end = at / a.R, r = at % a.R;
        double best, end_score;
        int cur;
        eligible_argmax(a.hist + size_t(at) * ldx, a.lend, a.np, lane, end_score, cur);
        for (int64_t j = L - 1; j >= 1 && cur != INT_MAX; --j) {
            if (lane == 0) a.states[o0 + j] = cur;
            const double* row = a.hist + (size_t(t_end - L + j) * size_t(a.R) + size_t(r)) * ldx;   // D at byte j - 1
            eligible_argmax(row, a.lat + size_t(cur) * np, a.np, lane, best, cur);
        }
        if (lane != 0) continue;
        if (cur == INT_MAX) {   // no eligible route (a string with log q above -inf has one)
            cd[0] = kCodeNone;
            a.logw[s] = -INFINITY;
            a.score[s] = nan;
            continue;
        }
        a.states[o0] = cur;
        // forward along the path: the codes and the decoders' weight
        double total = 0.0;
        int prev = -1;
        for (int64_t j = 0; j < L; ++j) {
            const int T = a.states[o0 + j];
            const int sym = a.meta[size_t(t_end - L + 1 + j) * size_t(a.R) + size_t(r)] & 0x1ff;
            const int32_t ct = j == 0 ? a.code_s[T] : a.code_a[size_t(prev) * np + size_t(T)];
            const int32_t ce = a.code_em[size_t(sym) * np + size_t(T)];
            double lw = 0.0;
            if (ct >= 0) lw += a.w[ct];
            if (ce >= 0) lw += a.w[ce];
            total += lw;
            cd[2 * j] = ct;
            cd[2 * j + 1] = ce;
            prev = T;
        }
        const int32_t cx = a.code_e[prev];
        double lw = 0.0;
        if (cx >= 0) lw += a.w[cx];
        total += lw;
        cd[2 * L] = cx;
        cd[2 * L + 1] = kCodeOne;
        a.logw[s] = total;
        a.score[s] = end_score;
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

hipError_t DensePath::byte_marginals_masses(const double* w_full, hipEvent_t const ev[8], hipStream_t s) {
    const size_t np = size_t(np_), R = size_t(R_), S = size_t(n_strings_), TR = size_t(T_) * R, ld = size_t(ldx_);
    ByteMarginalBufs& m = bm_;
    if (!m.amat) {   // first call since the load: the passes' buffers, and where every corpus byte's row lies
        DTRY(dalloc(m.w, size_t(n_params_)));
        DTRY(dalloc(m.ewp, size_t(n_params_)));
        DTRY(dalloc(m.amat_t, np * np));
        DTRY(dalloc(m.et, size_t(vocab_ + 1) * np));
        DTRY(dalloc(m.a0, np));
        DTRY(dalloc(m.aend, np));
        DTRY(dalloc(m.la, TR));
        DTRY(dalloc(m.lb, TR));
        DTRY(dalloc(m.sum, 2 * R));
        DTRY(dalloc(m.y, 2 * R * ld));
        DTRY(dalloc(m.ysplit, R * ld));
        DTRY(dalloc(m.z, R * ld));
        DTRY(dalloc(m.logq, S));
        DTRY(dalloc(m.ll, size_t(std::max(n_ll_, 1))));
        std::vector<int32_t> end_at(std::max<size_t>(S, 1), -1), rowof(std::max<size_t>(size_t(total_sym_), 1), 0);
        if (S > 0) DTRY(hipMemcpyAsync(end_at.data(), end_at_, S * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        DTRY(hipStreamSynchronize(s));
        for (size_t i = 0; i < S; ++i) {
            const int64_t L = off_host_[i + 1] - off_host_[i];
            for (int64_t j = 0; j < L; ++j)   // the string's bytes lie one step apart in its slot
                rowof[size_t(off_host_[i] + j)] = int32_t(int64_t(end_at[i]) - (L - 1 - j) * int64_t(R_));
        }
        DTRY(dalloc(m.rowof, size_t(total_sym_)));
        DTRY(dalloc(m.cnt, size_t(total_sym_)));
        DTRY(dalloc(m.mrow, size_t(total_sym_) + 1));
        if (total_sym_ > 0)
            DTRY(hipMemcpyAsync(m.rowof, rowof.data(), size_t(total_sym_) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        DTRY(hipStreamSynchronize(s));
        DTRY(dalloc(m.amat, np * np));
    }
    DTRY(history_alloc());
    if (n_params_ > 0) DTRY(hipMemcpyAsync(m.w, w_full, size_t(n_params_) * sizeof(double), hipMemcpyHostToDevice, s));
    DTRY(hipEventRecord(ev[0], s));
    if (n_params_ > 0) {
        const unsigned blocks = unsigned(std::min<int32_t>(64, (n_params_ + 255) / 256));
        dense_bm_exp_kernel<<<blocks, 256, 0, s>>>(m.w, m.ewp, n_params_);
        DTRY(hipGetLastError());
    }
    ForwardBufs f{};
    f.amat = m.amat; f.amat_t = m.amat_t; f.et = m.et; f.a0 = m.a0; f.aend = m.aend;
    f.alpha = dhist_; f.la = m.la; f.sum = m.sum; f.ysplit = m.ysplit; f.logq = m.logq; f.ll_part = m.ll;
    DTRY(enqueue_forward_into(m.ewp, f, s));
    DTRY(hipEventRecord(ev[1], s));
    BackwardBufs b{};
    b.amat_t = m.amat_t; b.et = m.et; b.aend = m.aend; b.alpha = dhist_; b.la = m.la; b.logq = m.logq;
    b.gam = dhist_; b.lb = m.lb; b.sum = m.sum; b.y = m.y; b.ysplit = m.ysplit; b.z = m.z;
    DTRY(enqueue_backward_into(b, s));
    return hipEventRecord(ev[2], s);
}

hipError_t DensePath::byte_marginals_count(int64_t* n_entries, hipEvent_t const ev[8], hipStream_t s) {
    const size_t B = size_t(total_sym_);
    bm_mrow_host_.assign(B + 1, 0);
    if (B > 0) {
        RowArgs a{};
        a.gam = dhist_; a.rowof = bm_.rowof; a.state_id = state_id_; a.cnt = bm_.cnt;
        a.n_bytes = total_sym_;
        a.n_states = n_states_; a.ldx = ldx_;
        const int64_t want = (total_sym_ + kRowWaves - 1) / kRowWaves;
        const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(want, int64_t(n_cu_) * 16)));
        dense_bm_rows_kernel<false><<<grid, kRowWaves * 64, 0, s>>>(a);
        DTRY(hipGetLastError());
    }
    DTRY(hipEventRecord(ev[3], s));
    std::vector<int32_t> cnt(std::max<size_t>(B, 1), 0);
    if (B > 0) DTRY(hipMemcpyAsync(cnt.data(), bm_.cnt, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DTRY(hipStreamSynchronize(s));
    for (size_t b = 0; b < B; ++b) bm_mrow_host_[b + 1] = bm_mrow_host_[b] + cnt[b];
    *n_entries = bm_mrow_host_[B];
    return hipSuccess;
}

hipError_t DensePath::byte_marginals_fill(hipEvent_t const ev[8], hipStream_t s) {
    const size_t B = size_t(total_sym_), E = size_t(bm_mrow_host_[B]);
    if (dalloc(bm_.midx, E) != hipSuccess || dalloc(bm_.mval, E) != hipSuccess) {
        (void)hipGetLastError();
        byte_marginals_rows_release();
        return hipErrorOutOfMemory;
    }
    DTRY(hipMemcpyAsync(bm_.mrow, bm_mrow_host_.data(), (B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    DTRY(hipEventRecord(ev[4], s));
    if (B > 0) {
        RowArgs a{};
        a.gam = dhist_; a.rowof = bm_.rowof; a.state_id = state_id_; a.mrow = bm_.mrow; a.midx = bm_.midx; a.mval = bm_.mval;
        a.n_bytes = total_sym_;
        a.n_states = n_states_; a.ldx = ldx_;
        const int64_t want = (total_sym_ + kRowWaves - 1) / kRowWaves;
        const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(want, int64_t(n_cu_) * 16)));
        dense_bm_rows_kernel<true><<<grid, kRowWaves * 64, 0, s>>>(a);
        DTRY(hipGetLastError());
    }
    return hipEventRecord(ev[5], s);
}

void DensePath::byte_marginals_rows_release() {
    if (bm_.midx) (void)hipFree(bm_.midx);
    if (bm_.mval) (void)hipFree(bm_.mval);
    bm_.midx = nullptr;
    bm_.mval = nullptr;
}

hipError_t DensePath::byte_marginals_decode(hipEvent_t const ev[8], hipStream_t s) {
    const size_t np = size_t(np_), R = size_t(R_), S = size_t(n_strings_), ld = size_t(ldx_);
    ByteMarginalBufs& m = bm_;
    if (!m.tla) {   // first decode since the load
        DTRY(dalloc(m.tlat, np * np));
        DTRY(dalloc(m.tle, size_t(vocab_ + 1) * np));
        DTRY(dalloc(m.tl0, np));
        DTRY(dalloc(m.tlend, np));
        DTRY(dalloc(m.states, size_t(total_sym_)));
        DTRY(dalloc(m.codes, 2 * (size_t(total_sym_) + S)));
        DTRY(dalloc(m.logw, S));
        DTRY(dalloc(m.score, S));
        DTRY(dalloc(m.tla, np * np));
    }
    DTRY(hipEventRecord(ev[6], s));
    DTRY(enqueue_decode_tables_into(m.w, DecodeTables{m.tla, m.tlat, m.tle, m.tl0, m.tlend}, s));
    dense_bm_mask_kernel<<<unsigned(std::min<size_t>(1024, (np * np + 255) / 256)), 256, 0, s>>>(m.tla, int64_t(np * np));
    DTRY(hipGetLastError());
    if (total_sym_ > 0) {
        RewardArgs g{};
        g.mask = m.tla; g.le = m.tle; g.l0 = m.tl0;
        g.np = np_; g.ldx = ldx_; g.vocab = vocab_;
        const dim3 grid(unsigned(np / kT), unsigned(R / kT));
        for (int64_t t = 0; t < T_; ++t) {
            RewardArgs f = g;
            f.x = t > 0 ? dhist_ + size_t(t - 1) * R * ld : nullptr;
            f.y = dhist_ + size_t(t) * R * ld;
            f.meta = meta_ + size_t(t) * R;
            if (t == 0) dense_bm_maxplus_kernel<true><<<grid, 256, 0, s>>>(f);
            else dense_bm_maxplus_kernel<false><<<grid, 256, 0, s>>>(f);
            DTRY(hipGetLastError());
        }
    }
    if (S > 0) {
        BacktrackArgs b{};
        b.hist = dhist_; b.lat = m.tlat; b.lend = m.tlend; b.w = m.w; b.logq = m.logq;
        b.code_a = code_a_; b.code_em = code_em_; b.code_s = code_s_; b.code_e = code_e_;
        b.meta = meta_; b.end_at = end_at_; b.off = doff_;
        b.states = m.states; b.codes = m.codes; b.logw = m.logw; b.score = m.score;
        b.n_strings = n_strings_;
        b.np = np_; b.ldx = ldx_; b.R = R_; b.code_se = code_se_;
        const int64_t want = (int64_t(S) + kBtWaves - 1) / kBtWaves;
        const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(want, int64_t(n_cu_) * 8)));
        dense_bm_backtrack_kernel<<<grid, kBtWaves * 64, 0, s>>>(b);
        DTRY(hipGetLastError());
    }
    return hipEventRecord(ev[7], s);
}

hipError_t DensePath::byte_marginals_logq_download(double* logq, hipStream_t s) const {
    if (n_strings_ == 0) return hipSuccess;
    return hipMemcpyAsync(logq, bm_.logq, size_t(n_strings_) * sizeof(double), hipMemcpyDeviceToHost, s);
}

hipError_t DensePath::byte_marginals_rows_download(int32_t* midx, double* mval, hipStream_t s) const {
    const size_t E = size_t(bm_mrow_host_.empty() ? 0 : bm_mrow_host_.back());
    if (E == 0) return hipSuccess;
    DTRY(hipMemcpyAsync(midx, bm_.midx, E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return hipMemcpyAsync(mval, bm_.mval, E * sizeof(double), hipMemcpyDeviceToHost, s);
}

hipError_t DensePath::byte_marginals_paths_download(double* score, double* logw, int32_t* codes, hipStream_t s) const {
    const size_t S = size_t(n_strings_);
    if (S == 0) return hipSuccess;
    DTRY(hipMemcpyAsync(score, bm_.score, S * sizeof(double), hipMemcpyDeviceToHost, s));
    DTRY(hipMemcpyAsync(logw, bm_.logw, S * sizeof(double), hipMemcpyDeviceToHost, s));
    return hipMemcpyAsync(codes, bm_.codes, 2 * (size_t(total_sym_) + S) * sizeof(int32_t), hipMemcpyDeviceToHost, s);
}

}  // namespace wfsa

// Viterbi decode on the dense path (wfsa_dev_dense_best_paths; dense_path.hpp):
// the most probable accepting path of every loaded string by a (max, +) pass
// in the log domain over the row slots the evaluations use.
//
// Per call, on one stream:
//   dense_decode_tables   log tables straight from w_full and the parameter
//                         codes (never log(exp(w))): lA[S][T], its transpose
//                         lAT[T][S], lE[v][T] (row vocab: -inf), l0[T], lend[T];
//                         no edge / padded state -inf, an unequivocal edge 0.0
//   dense_maxplus  x T    D_t[r][T] = max_S (D_{t-1}[r][S] + lA[S][T]) + lE[sym][T]
//                         (max first, then one add); l0[T] + lE[sym][T] where a
//                         string starts, -inf on idle rows.  Every D_t is kept:
//                         T x R x np doubles
//   dense_backtrack       one wavefront per string: the end state maximises
//                         D_end[T] + lend[T], every predecessor is the S that
//                         maximises D_{t-1}[S] + lAT[T][S] -- recomputed from
//                         the history (no back-pointers), ties to the lowest
//                         state, a -inf candidate never chosen; then the path's
//                         parameter codes and its weight as the decoders form it
//                         (decode.hip: an edge's weight is the left-to-right sum,
//                         from 0.0, of its present parameters; the path's the
//                         left-to-right sum, from 0.0, of its edges)
// -inf is the only non-finite value the pass meets (the entry point rejects
// NaN and +inf weights), so fmax never sees a NaN.
#include "dense_path.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace wfsa {

namespace {

constexpr int kT = kDenseTile;   // 128
constexpr int kMxK = 16;         // K slice of the max-plus tile
constexpr int kBtWaves = 4;      // back-track: wavefronts per block

__device__ __forceinline__ double code_logw(const double* w, int32_t c) {
    return c >= 0 ? w[c] : (c == kCodeOne ? 0.0 : -INFINITY);
}

struct DecodeTableArgs {
    const double* w;            // [n_params] w_full
    const int32_t* code_a;      // [np][np]
    const int32_t* code_em;     // [vocab+1][np]
    const int32_t* code_s;      // [np]
    const int32_t* code_e;      // [np]
    double* la;                 // [np][np]
    double* lat;                // [np][np] transposed
    double* le;                 // [vocab+1][np]
    double* l0;                 // [np]
    double* lend;               // [np]
    int64_t n_em;
    int32_t np;
};

// grid (np / 32, np / 32): block (bx, by) fills the 32 x 32 tile of lA at rows
// by, columns bx and its transpose in lAT (through LDS: both stores run along
// rows); the small tables are dealt over all blocks
__global__ __launch_bounds__(256) void dense_decode_tables_kernel(DecodeTableArgs a) {
    __shared__ double tile[32][33];
    const int bx = int(blockIdx.x) * 32, by = int(blockIdx.y) * 32;
    const int tx = int(threadIdx.x) & 31, ty = int(threadIdx.x) >> 5;
    const size_t np = size_t(a.np);
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const size_t o = size_t(by + ty + k) * np + size_t(bx + tx);
        const double v = code_logw(a.w, a.code_a[o]);
        a.la[o] = v;
        tile[ty + k][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) a.lat[size_t(bx + ty + k) * np + size_t(by + tx)] = tile[tx][ty + k];
    const int64_t nblocks = int64_t(gridDim.x) * gridDim.y, stride = nblocks * 256;
    const int64_t t0 = (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    for (int64_t i = t0; i < a.n_em; i += stride) a.le[i] = code_logw(a.w, a.code_em[i]);
    for (int64_t i = t0; i < a.np; i += stride) {
        a.l0[i] = code_logw(a.w, a.code_s[i]);
        a.lend[i] = code_logw(a.w, a.code_e[i]);
    }
}

struct MaxPlusArgs {
    const double* x;        // [R][np] D_{t-1} (unused at step 0)
    const double* la;       // [np][np]
    const double* le;       // [vocab+1][np]
    const double* l0;       // [np]
    const int32_t* meta;    // [R] this step
    double* y;              // [R][np] D_t, a row block of the history
    int32_t np, vocab;
};

// One step of the (max, +) trellis for all R row slots, dense_minplus_kernel's
// tile: 128 x 128 per block (256 threads, 8 x 8 per thread at stride 16: the
// LDS reads of a slice broadcast within each 16-lane row group), K staged
// through LDS in slices of 16 with the next slice's global loads in registers
// during the current one's arithmetic.
template <bool FIRST>
__global__ __launch_bounds__(256) void dense_maxplus_kernel(MaxPlusArgs a) {
    __shared__ double xs[kMxK][kT + 1];   // [k][row]
    __shared__ double ls[kMxK][kT];       // [k][column]
    const int tid = int(threadIdx.x), tx = tid & 15, ty = tid >> 4;
    const int c0 = int(blockIdx.x) * kT, r0 = int(blockIdx.y) * kT;
    const size_t np = size_t(a.np);
    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = -INFINITY;
    if (!FIRST) {
        // loaders: x row tid/2, k half (tid&1)*8; lA k row tid/16, columns (tid&15)*8
        const int xr = tid >> 1, xk = (tid & 1) * 8, lk = tid >> 4, lc = (tid & 15) * 8;
        const double2* xp = reinterpret_cast<const double2*>(a.x + size_t(r0 + xr) * np + size_t(xk));
        const double2* lp = reinterpret_cast<const double2*>(a.la + size_t(lk) * np + size_t(c0 + lc));
        const size_t lstep = kMxK * np / 2;   // double2 per K slice of lA
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
        const bool idle = sym >= a.vocab, start = (m >> 9) & 1;
        double* yr = a.y + size_t(r) * np;
        const double* le = a.le + size_t(idle ? a.vocab : sym) * np;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int T = c0 + tx + 16 * j;
            yr[T] = idle ? -INFINITY : ((start || FIRST) ? a.l0[T] : acc[i][j]) + le[T];
        }
    }
}

struct BacktrackArgs {
    const double* hist;       // [T][R][np]
    const double* lat;        // [np][np] lAT[T][S]
    const double* lend;       // [np]
    const double* w;          // [n_params]
    const int32_t* code_a;    // [np][np]
    const int32_t* code_em;   // [vocab+1][np]
    const int32_t* code_s;    // [np]
    const int32_t* code_e;    // [np]
    const int32_t* meta;      // [T][R]
    const int32_t* end_at;    // [S]
    const int64_t* off;       // [S + 1]
    int32_t* states;          // [total symbols] the path's state at every byte
    int32_t* codes;           // [2 (total symbols + S)] per string and edge: (transition, emission) code
    double* logw;             // [S]
    int64_t n_strings;
    int32_t np, R, code_se;
};

// the wave's maximum of (v, i): ties to the lower index; i = INT_MAX: no finite candidate
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

__global__ __launch_bounds__(kBtWaves * 64) void dense_backtrack_kernel(BacktrackArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t wave0 = int64_t(blockIdx.x) * kBtWaves + (int(threadIdx.x) >> 6);
    const int64_t n_waves = int64_t(gridDim.x) * kBtWaves;
    const size_t np = size_t(a.np);
    for (int64_t s = wave0; s < a.n_strings; s += n_waves) {
        const int64_t o0 = a.off[s], L = a.off[s + 1] - o0;
        int32_t* cd = a.codes + 2 * (o0 + s);
        const int32_t at = a.end_at[s];
        if (at < 0) {   // the empty string: the ^ -> $ edge or nothing
            if (lane == 0) {
                double lw = 0.0;
                if (a.code_se >= 0) lw += a.w[a.code_se];
                const double total = 0.0 + lw;
                const bool ok = a.code_se != kCodeNone && total > -INFINITY;
                cd[0] = ok ? a.code_se : kCodeNone;
                cd[1] = kCodeOne;
                a.logw[s] = ok ? total : -INFINITY;
            }
            continue;
        }
        const int64_t t_end = at / a.R, r = at % a.R;
        int cur;
        {
            const double* row = a.hist + size_t(at) * np;
            double best = -INFINITY;
            int arg = INT_MAX;
            for (int c = lane; c < a.np; c += 64) {
                const double v = row[c] + a.lend[c];
                if (v > best) {
                    best = v;
                    arg = c;
                }
            }
            wave_argmax(best, arg);
            cur = arg;
        }
        for (int64_t j = L - 1; j >= 1 && cur != INT_MAX; --j) {
            if (lane == 0) a.states[o0 + j] = cur;
            const double* row = a.hist + (size_t(t_end - L + j) * size_t(a.R) + size_t(r)) * np;   // D at byte j - 1
            const double* lt = a.lat + size_t(cur) * np;
            double best = -INFINITY;
            int arg = INT_MAX;
            for (int c = lane; c < a.np; c += 64) {
                const double v = row[c] + lt[c];
                if (v > best) {
                    best = v;
                    arg = c;
                }
            }
            wave_argmax(best, arg);
            cur = arg;
        }
        if (lane != 0) continue;
        if (cur == INT_MAX) {   // no accepting path of finite weight
            cd[0] = kCodeNone;
            a.logw[s] = -INFINITY;
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

size_t DensePath::best_paths_history_bytes() const {
    return size_t(T_) * size_t(R_) * size_t(ldx_) * sizeof(double);
}

// the log tables at w (device) into the caller's buffers (the MEA decode reads
// its eligibility from tables of its own: dense_marginals.hip)
hipError_t DensePath::enqueue_decode_tables_into(const double* w, const DecodeTables& t, hipStream_t s) {
    const size_t np = size_t(np_);
    DecodeTableArgs a{};
    a.w = w;
    a.code_a = code_a_; a.code_em = code_em_; a.code_s = code_s_; a.code_e = code_e_;
    a.la = t.la; a.lat = t.lat; a.le = t.le; a.l0 = t.l0; a.lend = t.lend;
    a.n_em = int64_t(size_t(vocab_ + 1) * np);
    a.np = np_;
    const dim3 grid(unsigned(np / 32), unsigned(np / 32));
    dense_decode_tables_kernel<<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t DensePath::enqueue_best_paths(const double* w_full, hipEvent_t const ev[4], hipStream_t s) {
    const size_t np = size_t(np_), R = size_t(R_), S = size_t(n_strings_);
    if (!dla_) {   // first call since the load: the pass's buffers
        DTRY(dalloc(dw_, size_t(n_params_)));
        DTRY(dalloc(dla_, np * np));
        DTRY(dalloc(dlat_, np * np));
        DTRY(dalloc(dle_, size_t(vocab_ + 1) * np));
        DTRY(dalloc(dl0_, np));
        DTRY(dalloc(dlend_, np));
        DTRY(dalloc(dstates_, size_t(total_sym_)));
        DTRY(dalloc(dcodes_, 2 * (size_t(total_sym_) + S)));
        DTRY(dalloc(dlogw_, S));
    }
    DTRY(history_alloc());   // (shared with the sampler's alpha rows: pitch np + pad there, np here)
    if (n_params_ > 0) DTRY(hipMemcpyAsync(dw_, w_full, size_t(n_params_) * sizeof(double), hipMemcpyHostToDevice, s));
    DTRY(hipEventRecord(ev[0], s));
    DTRY(enqueue_decode_tables_into(dw_, DecodeTables{dla_, dlat_, dle_, dl0_, dlend_}, s));
    DTRY(hipEventRecord(ev[1], s));
    if (total_sym_ > 0) {
        MaxPlusArgs g{};
        g.la = dla_; g.le = dle_; g.l0 = dl0_;
        g.np = np_;
        g.vocab = vocab_;
        const dim3 grid(unsigned(np / kT), unsigned(R / kT));
        for (int64_t t = 0; t < T_; ++t) {
            MaxPlusArgs f = g;
            f.x = t > 0 ? dhist_ + size_t(t - 1) * R * np : nullptr;
            f.y = dhist_ + size_t(t) * R * np;
            f.meta = meta_ + size_t(t) * R;
            if (t == 0) dense_maxplus_kernel<true><<<grid, 256, 0, s>>>(f);
            else dense_maxplus_kernel<false><<<grid, 256, 0, s>>>(f);
            DTRY(hipGetLastError());
        }
    }
    DTRY(hipEventRecord(ev[2], s));
    if (S > 0) {
        BacktrackArgs b{};
        b.hist = dhist_; b.lat = dlat_; b.lend = dlend_; b.w = dw_;
        b.code_a = code_a_; b.code_em = code_em_; b.code_s = code_s_; b.code_e = code_e_;
        b.meta = meta_; b.end_at = end_at_; b.off = doff_;
        b.states = dstates_; b.codes = dcodes_; b.logw = dlogw_;
        b.n_strings = n_strings_;
        b.np = np_; b.R = R_; b.code_se = code_se_;
        const int64_t want = (int64_t(S) + kBtWaves - 1) / kBtWaves;
        const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(want, int64_t(n_cu_) * 8)));
        dense_backtrack_kernel<<<grid, kBtWaves * 64, 0, s>>>(b);
        DTRY(hipGetLastError());
    }
    return hipEventRecord(ev[3], s);
}

hipError_t DensePath::best_paths_download(double* logw, int32_t* codes, hipStream_t s) const {
    const size_t S = size_t(n_strings_);
    if (S == 0) return hipSuccess;
    DTRY(hipMemcpyAsync(logw, dlogw_, S * sizeof(double), hipMemcpyDeviceToHost, s));
    return hipMemcpyAsync(codes, dcodes_, 2 * (size_t(total_sym_) + S) * sizeof(int32_t), hipMemcpyDeviceToHost, s);
}

}  // namespace wfsa

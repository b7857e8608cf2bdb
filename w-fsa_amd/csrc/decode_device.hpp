// Device helpers of the wave-per-string trellis walks (decode.hip's (max, +)
// decoders and sample.hip's (+, x) sampler): the fence between a wave's
// phases, the work ticket and the live set of a position.  Include from a
// .hip translation unit only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fb_kernels.hpp"

namespace wfsa {

namespace {

constexpr int kWave = 64;

// A wave's lanes hand values to each other through its global scratch rows:
// a phase's stores are complete, and its loads done, before the next phase
// (the same fence the H_f traversal kernel uses between its phases).
__device__ __forceinline__ void phase_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// The wave takes the next string: every lane runs the add (lane 0 adds one,
// the rest nothing), so the decode loop starts with no branch on the lane.
// With "if (lane == 0)" around the add, the compiler threaded the other lanes'
// path round the loop past it: they parted from lane 0 and decoded string 0
// for ever.
__device__ __forceinline__ int next_string(unsigned* ctr, int lane) {
    __builtin_amdgcn_wave_barrier();
    const unsigned got = __hip_atomic_fetch_add(ctr, lane == 0 ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __builtin_amdgcn_readfirstlane(int(got));   // lane 0's ticket
}

// The nodes live at position j of one string: the destinations of byte
// c_{j-1}, as slots [begin(j), end(j)) of W.dst (ascending nodes); at 0 the
// start node alone.
struct LiveSet {
    const WideModel& W;
    const uint8_t* str;
    int start;
    __device__ __forceinline__ int begin(int j) const { return j == 0 ? 0 : W.c_ptr[str[j - 1]]; }
    __device__ __forceinline__ int end(int j) const { return j == 0 ? 1 : W.c_ptr[str[j - 1] + 1]; }
    __device__ __forceinline__ int node(int j, int k) const { return j == 0 ? start : W.dst[k]; }
    // the slot of `node` among the nodes live at position j >= 1
    __device__ __forceinline__ int slot_of(int j, int node) const {
        int lo = begin(j), hi = end(j) - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (W.dst[mid] < node) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
};

}  // namespace

}  // namespace wfsa

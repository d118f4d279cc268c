// Workgroup and wave collectives: how per-thread values become a sum, a rank or a prefix.  Included by rto_device.hip.h right
// after kWave and kBlock; a kernel of the grid features that sums, ranks or scans calls these and keeps no partials of its own
// (the few that keep their own code, and why: docs/LAB_NOTES.md, "One set of workgroup collectives").
//
// THE CONTRACT
//  * wave_* calls hold no barrier and use no LDS.  Every lane of the wave that is still running must reach them together (they
//    shuffle and vote): call them from wave-uniform control flow.  wave_reduce / wave_sum / wave_min / wave_max give the result
//    to every lane.
//  * block_* calls (block_reduce / block_sum / block_min / block_max, block_rank, block_exclusive_scan) hold exactly ONE
//    __syncthreads().  EVERY thread of the workgroup must reach such a call: it sits outside the kernel's bounds test, and a
//    thread that owns nothing passes the operation's identity (0 for a sum, false for a rank).  THREADS is the workgroup's size
//    (blockDim.x, a multiple of 64).  Every thread folds the waves' partials, so every thread holds the result.
//  * LDS: each block_* call owns a static array of THREADS / 64 partials per value (THREADS / 64 words for an int, twice that
//    for a 64-bit value, THREADS / 64 * sizeof(T) bytes for a struct).  Two calls of the same collective with the same types in
//    one kernel share that array.  Before the same collective is called a SECOND time (a loop, or twice in a row) the caller
//    holds a barrier between the first call's return (its last read of the partials) and the second call (its next write):
//        for (...) { r = block_rank<kBlock>(flag, &all); ...; __syncthreads(); }
//  * Integers only: int, unsigned, long long, unsigned long long, or a struct of them handed to block_reduce / wave_reduce with
//    the caller's own `op(a, b)`: several values then cost one barrier.  The operations must be associative and commutative (the
//    order in which lanes and waves are combined is not promised), which is why no float is reduced here.
#pragma once

namespace rto {

struct OpSum { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct OpMin { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct OpMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; } };

// A bounding box in integer coordinates, the multi-value reduction most kernels here want.
struct IntBox { int lo[3], hi[3]; };
struct OpBoxUnion {
    __device__ __forceinline__ IntBox operator()(IntBox a, const IntBox& b) const {
#pragma unroll
        for (int k = 0; k < 3; k++) { a.lo[k] = min(a.lo[k], b.lo[k]); a.hi[k] = max(a.hi[k], b.hi[k]); }
        return a;
    }
};

// lane l receives v of lane l ^ off: any value made of 32-bit words
template <typename T>
__device__ __forceinline__ T lane_xor(T v, int off) {
    static_assert(sizeof(T) % 4 == 0, "collectives move 32-bit words");
    int w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); k++) w[k] = __shfl_xor(w[k], off);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// ---------------------------------------------------------------- the wave
template <typename T, typename OP>
__device__ __forceinline__ T wave_reduce(T v, OP op) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = op(v, lane_xor(v, off));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, OpSum()); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, OpMin()); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, OpMax()); }

// the sum of v over lanes 0 .. this lane
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = (int)threadIdx.x % kWave;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T up = __shfl_up(v, off);
        if (lane >= off) v += up;
    }
    return v;
}

// Do all lanes that hold a label (have) hold the same one?  first: the label of the lowest holder, -1 when no lane holds any
// (the answer is then false).
__device__ __forceinline__ bool wave_uniform_label(bool have, int label, int& first) {
    const unsigned long long holders = __ballot(have);
    first = -1;
    if (!holders) return false;
    first = __shfl(label, (int)__ffsll((long long)holders) - 1);
    return __ballot(have && label != first) == 0ull;
}

// Appending to a list whose length is *counter, one atomic per wave (none for a wave that appends nothing): the first of this
// lane's n consecutive slots, lanes in order.
template <typename T>
__device__ __forceinline__ T wave_append(T n, T* counter) {
    const int lane = (int)threadIdx.x % kWave;
    const T upto = wave_inclusive_scan(n);
    T base = 0;
    if (lane == kWave - 1 && upto > 0) base = atomicAdd(counter, upto);
    return __shfl(base, kWave - 1) + upto - n;
}

// ---------------------------------------------------------------- the workgroup (one barrier each: see the contract)
template <int THREADS, typename T, typename OP>
__device__ __forceinline__ T block_reduce(T v, OP op) {
    static_assert(THREADS % kWave == 0, "whole waves");
    __shared__ T part[THREADS / kWave];
    v = wave_reduce(v, op);
    if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    T r = part[0];
#pragma unroll
    for (int w = 1; w < THREADS / kWave; w++) r = op(r, part[w]);
    return r;
}
template <int THREADS, typename T> __device__ __forceinline__ T block_sum(T v) { return block_reduce<THREADS>(v, OpSum()); }
template <int THREADS, typename T> __device__ __forceinline__ T block_min(T v) { return block_reduce<THREADS>(v, OpMin()); }
template <int THREADS, typename T> __device__ __forceinline__ T block_max(T v) { return block_reduce<THREADS>(v, OpMax()); }

// the sum of v over the threads before this one; *total (optional): over all threads
template <int THREADS, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* total = nullptr) {
    static_assert(THREADS % kWave == 0, "whole waves");
    __shared__ T part[THREADS / kWave];
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    const T incl = wave_inclusive_scan(v);
    if (lane == kWave - 1) part[wave] = incl;
    __syncthreads();
    T before = incl - v, all = 0;
#pragma unroll 4                                     // by four, not whole: sixteen 64-bit partials at once (1024 threads) cost 72 VGPRs against 32
    for (int w = 0; w < THREADS / kWave; w++) { const T p = part[w]; before += w < wave ? p : T(0); all += p; }
    if (total) *total = all;
    return before;
}

// the number of set flags in the threads before this one; *total (optional): in all threads
template <int THREADS>
__device__ __forceinline__ int block_rank(bool flag, int* total = nullptr) {
    static_assert(THREADS % kWave == 0, "whole waves");
    __shared__ int part[THREADS / kWave];
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
    if (lane == 0) part[wave] = __builtin_popcountll(m);
    __syncthreads();
    int before = __builtin_popcountll(m & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < THREADS / kWave; w++) { const int p = part[w]; before += w < wave ? p : 0; all += p; }
    if (total) *total = all;
    return before;
}

}  // namespace rto

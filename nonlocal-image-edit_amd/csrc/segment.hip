// Automatic regions: the pixel kernels of kernel k-means on the trained affinity (the rule is stated in include/nle.h
// "automatic regions").  Three memory-bound passes over label bytes and fp32 planes:
//   k_segment_init    the start: label = the number of equal-population cuts the pixel's quarter-level bin has reached
//   k_segment_stats   per cluster the member count and the fp64 sum of the members' own spread value q_{label}[i] -- one
//                     gathered float and one byte per pixel (one 16-byte load where four pixels share a label, as they do
//                     inside a segment); per-workgroup partial sums, folded by k_segment_fold in a fixed order (the grid
//                     is a function of n alone), so two runs give the same bits
//   k_segment_assign  label' = the smallest c with the smallest m_c - 2 q_c[i]; the new indicator planes, the new counts
//                     and the number of changed labels (integer atomics: exact in any order)
// Every kernel takes four pixels per thread (16-byte plane accesses, one 4-byte word of labels) where all its pointers and
// strides allow it and one pixel at a time otherwise, as for the last n mod 4 pixels; grid-stride under combine_grid's cap.
// Nothing is handed from one workgroup to another inside a kernel: the steps are dependent launches on one stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <limits>

#include "kernels.h"
#include "launch.h"
#include "nle.h"
#include "plane_combine.h"

// the rule fixes where every rounding happens
#pragma clang fp contract(off)

namespace nlek {

namespace {

constexpr int kSegThreads = 256, kSegWaves = kSegThreads / 64;

// lane 0 receives the sum over the wave, the lanes added in a fixed order
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// a thread's tallies -> the wave's (shuffles) -> the workgroup's (LDS atomics); sh must be zeroed and fenced by the caller,
// and every thread of the workgroup calls this
template <int NV>
__device__ __forceinline__ void block_tally(unsigned* sh, const unsigned (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const unsigned w = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&sh[k], w);
    }
}

__device__ __forceinline__ void unpack4(unsigned w, unsigned (&l)[4]) {
    l[0] = w & 255u, l[1] = (w >> 8) & 255u, l[2] = (w >> 16) & 255u, l[3] = w >> 24;
}

// nle_plane_histogram's bin of x at scale 1, as a bin number: -1 below the range, 4096 above it and for a NaN
__device__ __forceinline__ int segment_bin(float x) {
    const double t = ((double)x + 256.0) * 4.0;
    if (t != t) return NLE_TONE_BINS;
    if (t < 0.0) return -1;
    if (t >= (double)NLE_TONE_BINS) return NLE_TONE_BINS;
    return (int)t;  // t >= 0: the conversion truncates to the floor
}

__device__ __forceinline__ unsigned init_label(float x, int C, const SegmentCuts& cuts) {
    const int b = segment_bin(x);
    unsigned l = 0;
#pragma unroll
    for (int c = 0; c < kRegionMax - 1; ++c)
        if (c < C - 1 && b >= cuts.b[c]) ++l;
    return l;
}

}  // namespace

__global__ __launch_bounds__(kSegThreads) void k_segment_init(const float* __restrict__ x, long long n, int C, const SegmentCuts cuts,
                                                              unsigned char* __restrict__ labels) {
    const bool vec = ((reinterpret_cast<size_t>(x) & 15) | (reinterpret_cast<size_t>(labels) & 3)) == 0;
    const long long n4 = vec ? n >> 2 : 0;
    const long long step = (long long)gridDim.x * kSegThreads, t0 = (long long)blockIdx.x * kSegThreads + threadIdx.x;
    for (long long g = t0; g < n4; g += step) {
        const float4 v = reinterpret_cast<const float4*>(x)[g];
        reinterpret_cast<unsigned*>(labels)[g] = init_label(v.x, C, cuts) | (init_label(v.y, C, cuts) << 8) |
                                                 (init_label(v.z, C, cuts) << 16) | (init_label(v.w, C, cuts) << 24);
    }
    for (long long i = n4 * 4 + t0; i < n; i += step) labels[i] = (unsigned char)init_label(x[i], C, cuts);
}

// partial[blockIdx.x][c] = the workgroup's sum for cluster c; r->count and r->bad are added to
template <int C>
__global__ __launch_bounds__(kSegThreads) void k_segment_stats(const float* __restrict__ q, long long q_stride, long long n,
                                                               const unsigned char* __restrict__ labels,
                                                               double* __restrict__ partial, SegmentResult* __restrict__ r) {
    __shared__ double sh_sum[kSegWaves][C];
    __shared__ unsigned sh_cnt[C + 1];
    const int tid = threadIdx.x;
    if (tid <= C) sh_cnt[tid] = 0u;
    __syncthreads();
    double acc[C];
    unsigned cnt[C + 1];  // cnt[C]: the labels out of range
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0, cnt[c] = 0u;
    cnt[C] = 0u;
    // one gathered value per pixel: the spread of the pixel's own cluster.  A label >= C is counted and indexes nothing.
    auto pixel = [&](long long i, unsigned l) {
        if (l < (unsigned)C) {
            const double v = (double)q[(long long)l * q_stride + i];
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (l == (unsigned)c) acc[c] += v, ++cnt[c];
        } else {
            ++cnt[C];
        }
    };
    const bool vec = (reinterpret_cast<size_t>(labels) & 3) == 0;
    const bool qvec = ((reinterpret_cast<size_t>(q) & 15) | (size_t)(q_stride & 3)) == 0;
    const long long n4 = vec ? n >> 2 : 0;
    const long long step = (long long)gridDim.x * kSegThreads, t0 = (long long)blockIdx.x * kSegThreads + tid;
    for (long long g = t0; g < n4; g += step) {
        const unsigned w = reinterpret_cast<const unsigned*>(labels)[g];
        unsigned l[4];
        unpack4(w, l);
        // inside a segment the four pixels share their label: one 16-byte load from that plane, their sum added once
        if (qvec && w == l[0] * 0x01010101u && l[0] < (unsigned)C) {
            const float4 v = *reinterpret_cast<const float4*>(q + (long long)l[0] * q_stride + g * 4);
            const double s4 = (((double)v.x + (double)v.y) + (double)v.z) + (double)v.w;
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (l[0] == (unsigned)c) acc[c] += s4, cnt[c] += 4u;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) pixel(g * 4 + j, l[j]);
        }
    }
    for (long long i = n4 * 4 + t0; i < n; i += step) pixel(i, labels[i]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double s = wave_sum(acc[c]);
        if ((tid & 63) == 0) sh_sum[tid >> 6][c] = s;
    }
    block_tally(sh_cnt, cnt);
    __syncthreads();
    if (tid < C) {
        double s = sh_sum[0][tid];
#pragma unroll
        for (int w = 1; w < kSegWaves; ++w) s += sh_sum[w][tid];
        partial[(long long)blockIdx.x * kRegionMax + tid] = s;
        if (sh_cnt[tid]) atomicAdd(&r->count[tid], (unsigned long long)sh_cnt[tid]);
    }
    if (tid == C && sh_cnt[C]) atomicAdd(&r->bad, (unsigned long long)sh_cnt[C]);
}

// one workgroup, 32 threads per cluster: thread j of cluster c adds the partials of the workgroups j, j + 32, .. in order,
// then the 32 are folded by shuffles in a fixed order; mean[c] = sum[c] / count[c], +inf for an empty cluster
__global__ __launch_bounds__(kSegThreads) void k_segment_fold(const double* __restrict__ partial, int blocks, int C,
                                                              SegmentResult* __restrict__ r) {
    static_assert(kSegThreads == 32 * kRegionMax, "32 threads for each of kRegionMax clusters");
    const int c = threadIdx.x >> 5, j = threadIdx.x & 31;
    double s = 0.0;
    if (c < C)
        for (int b = j; b < blocks; b += 32) s += partial[(long long)b * kRegionMax + c];
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) s += __shfl_down(s, d, 32);
    if (j == 0 && c < C) {
        const unsigned long long k = r->count[c];
        r->sum[c] = s;
        r->mean[c] = k ? s / (double)k : std::numeric_limits<double>::infinity();
    }
}

namespace {

struct AssignArgs {
    const float* q;  // null: no plane is read and every label stays -- the indicator planes and counts of the labels as they are
    long long q_stride, n;
    unsigned char* labels;
    float* ind;  // null: no indicator planes
    long long ind_stride;
    SegmentResult* r;
};

// the new labels of the P pixels from i on.  score = m_c - 2 q: a NaN never compares smaller and +inf is never smaller than
// the start, so both count as +inf, a tie keeps the smaller c, and a pixel none of whose scores is finite or -inf keeps its
// label.  A label out of range stays as it is (the host refuses the call on tally[C + 1]) and belongs to no cluster.
template <int C, int P>
__device__ __forceinline__ void assign_pixels(const AssignArgs& a, const double (&m)[C], long long i, const unsigned (&old)[P],
                                              unsigned (&lab)[P], unsigned (&tally)[C + 2]) {
    double best[P];
    int arg[P];
#pragma unroll
    for (int j = 0; j < P; ++j) best[j] = std::numeric_limits<double>::infinity(), arg[j] = -1;
    if (a.q) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            Pack<P> v;
            v.load(a.q + (long long)c * a.q_stride + i);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const double s = m[c] - 2.0 * (double)v.v[j];
                if (s < best[j]) best[j] = s, arg[j] = c;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const bool bad = old[j] >= (unsigned)C;
        lab[j] = (arg[j] < 0 || bad) ? old[j] : (unsigned)arg[j];
#pragma unroll
        for (int c = 0; c < C; ++c) tally[c] += lab[j] == (unsigned)c ? 1u : 0u;
        tally[C] += lab[j] != old[j] ? 1u : 0u;
        tally[C + 1] += bad ? 1u : 0u;
    }
}

}  // namespace

template <int C>
__global__ __launch_bounds__(kSegThreads) void k_segment_assign(const AssignArgs a) {
    __shared__ unsigned sh[C + 2];
    const int tid = threadIdx.x;
    if (tid < C + 2) sh[tid] = 0u;
    __syncthreads();
    double m[C];
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = a.r->mean[c];
    unsigned tally[C + 2];  // the new counts, the changed labels, the labels out of range
#pragma unroll
    for (int k = 0; k < C + 2; ++k) tally[k] = 0u;
    const size_t misaligned = (reinterpret_cast<size_t>(a.q) & 15) | (size_t)(a.q_stride & 3) | (reinterpret_cast<size_t>(a.labels) & 3) |
                              (a.ind ? (reinterpret_cast<size_t>(a.ind) & 15) | (size_t)(a.ind_stride & 3) : 0);
    const long long n4 = misaligned ? 0 : a.n >> 2;
    const long long step = (long long)gridDim.x * kSegThreads, t0 = (long long)blockIdx.x * kSegThreads + tid;
    for (long long g = t0; g < n4; g += step) {
        unsigned old[4], lab[4];
        unpack4(reinterpret_cast<const unsigned*>(a.labels)[g], old);
        assign_pixels<C, 4>(a, m, g * 4, old, lab, tally);
        reinterpret_cast<unsigned*>(a.labels)[g] = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
        if (a.ind) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                reinterpret_cast<float4*>(a.ind + (long long)c * a.ind_stride)[g] =
                    make_float4(lab[0] == (unsigned)c ? 1.f : 0.f, lab[1] == (unsigned)c ? 1.f : 0.f,
                                lab[2] == (unsigned)c ? 1.f : 0.f, lab[3] == (unsigned)c ? 1.f : 0.f);
        }
    }
    for (long long i = n4 * 4 + t0; i < a.n; i += step) {
        unsigned old[1] = {a.labels[i]}, lab[1];
        assign_pixels<C, 1>(a, m, i, old, lab, tally);
        a.labels[i] = (unsigned char)lab[0];
        if (a.ind) {
#pragma unroll
            for (int c = 0; c < C; ++c) a.ind[(long long)c * a.ind_stride + i] = lab[0] == (unsigned)c ? 1.f : 0.f;
        }
    }
    block_tally(sh, tally);
    __syncthreads();
    if (tid < C + 2 && sh[tid]) {
        unsigned long long* dst = tid < C ? &a.r->new_count[tid] : tid == C ? &a.r->changed : &a.r->bad_new;
        atomicAdd(dst, (unsigned long long)sh[tid]);
    }
}

// the stats grid: a function of n alone (the partials' order is the result's bits), a quarter of combine_grid's cap -- the
// workgroups make more trips, so fewer partials and fewer tallies reach the fold and the global counters
int segment_stats_blocks(long long n) { return (int)std::min<unsigned>(combine_grid(n), 1024u); }

hipError_t segment_init(hipStream_t s, const float* d_x, long long n, int C, const SegmentCuts& cuts, unsigned char* d_labels) {
    if (C < 1 || C > kRegionMax || n < 1) return hipErrorInvalidValue;
    return launch(k_segment_init, dim3(combine_grid(n)), dim3(kSegThreads), 0, s, d_x, n, C, cuts, d_labels);
}

hipError_t segment_stats(hipStream_t s, const float* d_q, long long q_stride, int C, long long n, const unsigned char* d_labels,
                         double* d_partial, SegmentResult* d_r) {
    if (n < 1 || q_stride < 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_r, 0, offsetof(SegmentResult, sum), s);  // count and bad
    if (e != hipSuccess) return e;
    const int blocks = segment_stats_blocks(n);
    const bool known = dispatch_columns<1, kRegionMax>(C, [&](auto c) {
        e = launch(k_segment_stats<decltype(c)::value>, dim3(blocks), dim3(kSegThreads), 0, s, d_q, q_stride, n, d_labels, d_partial,
                   d_r);
    });
    if (!known) return hipErrorInvalidValue;
    if (e != hipSuccess) return e;
    return launch(k_segment_fold, dim3(1), dim3(kSegThreads), 0, s, d_partial, blocks, C, d_r);
}

hipError_t segment_assign(hipStream_t s, const float* d_q, long long q_stride, int C, long long n, unsigned char* d_labels,
                          float* d_ind, long long ind_stride, SegmentResult* d_r) {
    if (n < 1 || q_stride < 0 || ind_stride < 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(reinterpret_cast<char*>(d_r) + offsetof(SegmentResult, new_count), 0,
                                  sizeof(SegmentResult) - offsetof(SegmentResult, new_count), s);
    if (e != hipSuccess) return e;
    const AssignArgs a{d_q, q_stride, n, d_labels, d_ind, ind_stride, d_r};
    const bool known = dispatch_columns<1, kRegionMax>(C, [&](auto c) {
        e = launch(k_segment_assign<decltype(c)::value>, dim3(combine_grid(n)), dim3(kSegThreads), 0, s, a);
    });
    return known ? e : hipErrorInvalidValue;
}

}  // namespace nlek

// bars.h — the bar layout of the generation kernels (graph.hip, generate.hip, notes.hip, sample.hip), defined once.
//
// A structure tensor is [G,4,32] (bar, track, timestep), cell (g, k, t) at (g * 4 + k) * 32 + t; the nodes of a bar are its
// active cells in that order (data.py:150-160).  Two lane layouts read it:
//   HalfBar   a bar per half-wave, 8 bars per 256-thread block: lane t of the half holds the four cells of timestep t, a
//             track's 32 cells lie across the half and come back as one 32-bit mask (BarMasks) from a ballot.
//   BarLanes  a bar per wave, 4 bars per 256-thread block: lane l holds the cells l and l + 64 of the bar's 128, and each
//             active cell's node number.
// block_scan_1024 is the one-workgroup exclusive scan behind every *_ptr array, pm_bar_node_ptr the host sequence
// "active cells per bar, then node_ptr" (k_bar_cells + k_bar_scan of generate.hip) that opens four entry points.
#pragma once
#include "common.h"

constexpr int PITCH_SOS = 128, PITCH_EOS = 129, PITCH_PAD = 130, DUR_EOS = 97, DUR_PAD = 98;   // constants.py:22-35

// bar_nodes[0..G) = active cells per bar, node_ptr[0..G] = their exclusive scan: two launches on `st` (generate.hip).
// PM_E_INVALID on a null pointer, G <= 0, 4 G beyond int32 or bar_nodes == node_ptr, PM_OK otherwise.
int pm_bar_node_ptr(hipStream_t st, const float* s_tensor, int32_t G, int32_t* bar_nodes, int32_t* node_ptr);

struct BarMasks { uint32_t m[4]; };     // bit t of m[k]: track k active at timestep t

// Coordinates of "a bar per half-wave".  The lanes of a half without a bar (odd G, the last block) have valid = false and
// must still take part in every cross-lane step: mask them out of the predicate, return only after the last ballot / shuffle.
struct HalfBar {
  int lane, half, t;
  int64_t g;
  bool valid;
  __device__ explicit HalfBar(int G) {
    lane = threadIdx.x & 63; half = lane >> 5; t = lane & 31;
    g = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 2 + half;
    valid = g < G;
  }
  __device__ int64_t cell(int k) const { return (g * 4 + k) * 32 + t; }
  // bit t: the predicate of lane t of this half (whole wave: a ballot)
  __device__ uint32_t ballot(bool p) const { return (uint32_t)(__ballot(p) >> (32 * half)); }
  __device__ BarMasks masks(const float* __restrict__ s) const {
    BarMasks b;
#pragma unroll
    for (int k = 0; k < 4; ++k) b.m[k] = ballot(valid && s[cell(k)] != 0.f);
    return b;
  }
  // the four cells of this lane as 0 / 1 into either form of a structure tensor (valid lanes only)
  __device__ void store(const bool (&on)[4], float* __restrict__ s_f32, uint8_t* __restrict__ s_u8) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (s_f32) s_f32[cell(k)] = on[k] ? 1.0f : 0.0f;
      if (s_u8) s_u8[cell(k)] = on[k] ? 1 : 0;
    }
  }
};

// sum over the 32 lanes of a half-wave, in every lane of it
__device__ inline int half_sum(int v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}
// exclusive prefix sum over the 32 lanes of a half-wave (t = lane & 31)
__device__ inline int half_exclusive(int v, int t) {
  int x = v;
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
    const int y = __shfl_up(x, o, 32);
    if (t >= o) x += y;
  }
  return x - v;
}

// "A bar per wave": lane l holds the cells l (track l >> 5) and l + 64 (track 2 + (l >> 5)) of bar g.  Nodes are numbered in
// cell order, so a cell's node is node_ptr[g] + the active cells before it in the bar; on0 / on1: the cell is active and its
// node lies below N.  g is wave-uniform and < G.
struct BarLanes {
  bool on0, on1;
  int64_t n0, n1;
  __device__ BarLanes(const float* __restrict__ s, const int* __restrict__ node_ptr, int g, int lane, int64_t N) {
    const bool a0 = s[(int64_t)g * 128 + lane] != 0.f, a1 = s[(int64_t)g * 128 + 64 + lane] != 0.f;
    const unsigned long long b0 = __ballot(a0), b1 = __ballot(a1), below = (1ull << lane) - 1ull;
    n0 = (int64_t)node_ptr[g] + __popcll(b0 & below);
    n1 = (int64_t)node_ptr[g] + __popcll(b0) + __popcll(b1 & below);
    on0 = a0 && n0 < N;
    on1 = a1 && n1 < N;
  }
};

// Exclusive scan of K int arrays a[k][0..n) by ONE workgroup of 1024 threads: thread i owns the run [lo, hi) of every array
// (ceil(n / 1024) entries, so any n fits), pre[k] is the sum of a[k] in front of the run and total[k] the whole sum.  The caller
// walks its run: ptr[i] = pre, pre += a[i].
template <int K>
struct BlockScan {
  int lo, hi, pre[K], total[K];
  __device__ BlockScan(const int* const (&a)[K], int n) {
    __shared__ int sa[K][1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024;
    lo = min(tid * per, n); hi = min(lo + per, n);
    int x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = 0;
    for (int i = lo; i < hi; ++i)
#pragma unroll
      for (int k = 0; k < K; ++k) x[k] += a[k][i];
#pragma unroll
    for (int k = 0; k < K; ++k) sa[k][tid] = x[k];
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      int y[K];
#pragma unroll
      for (int k = 0; k < K; ++k) y[k] = tid >= o ? sa[k][tid - o] : 0;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < K; ++k) sa[k][tid] += y[k];
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) { pre[k] = sa[k][tid] - x[k]; total[k] = sa[k][1023]; }
  }
};

// generate.hip — the device side of the reference's generation helpers.
//
//   pm_binary_from_logits : `Decoder._binary_from_logits` (model.py:609-623): sigmoid(s_logits) >= thresh, and an
//                           empty bar gets cell [0,0] switched on.  The reference finds the empty bars with
//                           `torch.nonzero` (a host sync); here each bar is one half-wave and a ballot.
//   pm_mtp_from_logits    : `mtp_from_logits` (utils.py:59-79): the dense multitrack pianoroll
//                           [G,4,32,15,230]: an active cell holds its node's logits (nodes are numbered in cell order,
//                           data.py:30,127), an inactive cell the hard silence (row 0 = one-hot pitch EOS, rows 1..14 =
//                           one-hot pitch PAD, duration part all zero).  The reference writes the tensor three times
//                           (zeros, masked put of the logits, masked put of the silence); here every cell is written
//                           once, HBM-write bound: 13.8 KB per cell.
//   pm_mtp_from_tokens    : the same pianoroll with an active cell holding the one-hot rows of its node's sampled tokens
//                           (csrc/sample.hip) instead of its logits: the reference's arg-max decoding then returns the tokens.
//   pm_node_tracks        : the track index of every node, in the same cell order (the per-track rules of chord-aware sampling).
//   pm_node_cells         : the cell index of every node, in the same order (the per-(bar, step) rules of pm_sample_chords_at).
// Byte / index work, bit-exact against the oracle (tests/test_generate_gpu.py, tests/test_sampling_gpu.py).
#include "bars.h"

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int CELL = PM_N_SLOTS * PM_N_TOK;      // 3450 floats per cell

__global__ void __launch_bounds__(256) k_binary_from_logits(const float* __restrict__ s_logits, int G, float thresh,
                                                            float* __restrict__ s_f32, uint8_t* __restrict__ s_u8) {
  const HalfBar h(G);
  bool on[4];
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float x = h.valid ? s_logits[h.cell(k)] : 0.f;
    on[k] = h.valid && !((1.0f / (1.0f + expf(-x))) < thresh);        // model.py:612-615 in fp32 (a NaN ends up True)
    any |= h.ballot(on[k]);
  }
  if (!h.valid) return;
  if (any == 0u && h.t == 0) on[0] = true;                             // model.py:617-621
  h.store(on, s_f32, s_u8);
}

// active cells per bar
__global__ void __launch_bounds__(256) k_bar_cells(const float* __restrict__ s, int G, int* __restrict__ bar_nodes) {
  const HalfBar h(G);
  const BarMasks b = h.masks(s);
  if (h.valid && h.t == 0) bar_nodes[h.g] = __popc(b.m[0]) + __popc(b.m[1]) + __popc(b.m[2]) + __popc(b.m[3]);
}

// exclusive scan over the bars (one workgroup): ptr[0..G]  (a and ptr may not alias)
__global__ void __launch_bounds__(1024) k_bar_scan(const int* __restrict__ a, int G, int* __restrict__ ptr) {
  const int* const in[1] = {a};
  const BlockScan<1> sc(in, G);
  int ra = sc.pre[0];
  for (int i = sc.lo; i < sc.hi; ++i) { ptr[i] = ra; ra += a[i]; }
  if (threadIdx.x == 1023) ptr[G] = sc.total[0];
}

// one workgroup per (bar, track): 32 cells of 13.8 KB, each wave takes 8 of them.  TOK: an active cell holds the one-hot
// rows of its node's tokens [15][2] (pm_mtp_from_tokens) instead of a copy of its logits.
template <bool TOK>
__global__ void __launch_bounds__(256) k_mtp_fill(const float* __restrict__ c_logits, const int* __restrict__ tokens,
                                                  const float* __restrict__ s, const int* __restrict__ node_ptr,
                                                  int64_t N, float* __restrict__ mtp) {
  __shared__ uint32_t masks[4];                                                 // (the numbering of BarLanes, bars.h, per track)
  const int g = blockIdx.x >> 2, k = blockIdx.x & 3;
  if (threadIdx.x < 128) {
    const bool on = s[(int64_t)g * 128 + threadIdx.x] != 0.f;
    const unsigned long long bal = __ballot(on);
    if ((threadIdx.x & 31) == 0) masks[threadIdx.x >> 5] = (uint32_t)(bal >> (threadIdx.x & 32));
  }
  __syncthreads();
  int before = 0;
  for (int j = 0; j < k; ++j) before += __popc(masks[j]);
  const uint32_t m = masks[k];
  const int64_t n0 = (int64_t)node_ptr[g] + before;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wave; t < 32; t += 4) {
    v2f* dst = reinterpret_cast<v2f*>(mtp + ((int64_t)(g * 4 + k) * 32 + t) * CELL);      // 13800 B: 8-byte aligned
    const int64_t n = n0 + __popc(m & ((1u << t) - 1u));
    if (TOK && ((m >> t) & 1u) && n < N) {
      // lane 2 row + head holds that row's token; a token outside its head's range lights no column
      const int tk = lane < 2 * PM_N_SLOTS ? tokens[n * (2 * PM_N_SLOTS) + lane] : -1;
      const int hot_l = (lane & 1) ? ((unsigned)tk < (unsigned)PM_N_DUR ? PM_N_PITCH + tk : -1)
                                   : ((unsigned)tk < (unsigned)PM_N_PITCH ? tk : -1);
      for (int i0 = 0; i0 < CELL / 2; i0 += 64) {                                                 // (whole wave: shuffles)
        const int i = i0 + lane, e = 2 * i, row = min(e / PM_N_TOK, PM_N_SLOTS - 1), col = e - row * PM_N_TOK;
        const int hp = __shfl(hot_l, 2 * row, 64), hd = __shfl(hot_l, 2 * row + 1, 64);
        v2f v;
        v.x = (col == hp || col == hd) ? 1.0f : 0.0f;
        v.y = (col + 1 == hp || col + 1 == hd) ? 1.0f : 0.0f;
        if (i < CELL / 2) __builtin_nontemporal_store(v, dst + i);
      }
    } else if (((m >> t) & 1u) && n < N) {
      const v2f* src = reinterpret_cast<const v2f*>(c_logits + n * CELL);
      for (int i = lane; i < CELL / 2; i += 64) __builtin_nontemporal_store(src[i], dst + i);
    } else {
      for (int i = lane; i < CELL / 2; i += 64) {
        const int e = 2 * i, row = e / PM_N_TOK, col = e - row * PM_N_TOK;                       // 230 is even: a pair never straddles rows
        const int hot = row == 0 ? PITCH_EOS : PITCH_PAD;
        v2f v;
        v.x = col == hot ? 1.0f : 0.0f;
        v.y = col + 1 == hot ? 1.0f : 0.0f;
        __builtin_nontemporal_store(v, dst + i);
      }
    }
  }
}

// the track of every node (pm_node_tracks): one wave per bar (BarLanes).  The tail [active, N) is zeroed by the same launch
// (grid-stride: no cell writes there).
__global__ void __launch_bounds__(256) k_node_tracks(const float* __restrict__ s, const int* __restrict__ node_ptr, int G,
                                                     int64_t N, uint8_t* __restrict__ node_track) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t active = node_ptr[G];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    if (i >= active) node_track[i] = 0;
  if (g >= G) return;                                                           // wave-uniform
  const BarLanes bl(s, node_ptr, g, lane, N);
  if (bl.on0) node_track[bl.n0] = (uint8_t)(lane >> 5);
  if (bl.on1) node_track[bl.n1] = (uint8_t)(2 + (lane >> 5));
}

// the cell of every node (pm_node_cells): k_node_tracks with the whole cell index 128 g + 32 track + step instead of the
// track alone, which is what a rule per (bar, step) needs (pm_sample_chords_at).  Same tail rule.
__global__ void __launch_bounds__(256) k_node_cells(const float* __restrict__ s, const int* __restrict__ node_ptr, int G,
                                                    int64_t N, int32_t* __restrict__ node_cell) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t active = node_ptr[G];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    if (i >= active) node_cell[i] = 0;
  if (g >= G) return;                                                           // wave-uniform
  const BarLanes bl(s, node_ptr, g, lane, N);
  if (bl.on0) node_cell[bl.n0] = g * 128 + lane;                                // 128 G <= 2^31 - 1 (host check)
  if (bl.on1) node_cell[bl.n1] = g * 128 + 64 + lane;
}

}  // namespace

int pm_bar_node_ptr(hipStream_t st, const float* s_tensor, int32_t G, int32_t* bar_nodes, int32_t* node_ptr) {
  if (!s_tensor || !bar_nodes || !node_ptr || G <= 0 || bar_nodes == node_ptr || (int64_t)G * 4 > 0x7fffffffLL)
    return PM_E_INVALID;
  hipLaunchKernelGGL(k_bar_cells, dim3(pm_cdiv(G, 8)), dim3(256), 0, st, s_tensor, G, bar_nodes);
  hipLaunchKernelGGL(k_bar_scan, dim3(1), dim3(1024), 0, st, bar_nodes, G, node_ptr);
  return PM_OK;
}

extern "C" int pm_binary_from_logits(const float* s_logits, int32_t G, float thresh, float* s_f32, uint8_t* s_u8,
                                     pm_stream_t stream) {
  if (!s_logits || (!s_f32 && !s_u8) || G <= 0) return PM_E_INVALID;
  hipLaunchKernelGGL(k_binary_from_logits, dim3(pm_cdiv(G, 8)), dim3(256), 0, (hipStream_t)stream, s_logits, G, thresh,
                     s_f32, s_u8);
  return pm_check_launch();
}

extern "C" int pm_mtp_from_logits(const float* c_logits, const float* s_tensor, int32_t G, int64_t N, int32_t* bar_nodes,
                                  int32_t* node_ptr, float* mtp, pm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if ((!c_logits && N > 0) || !mtp || N < 0 || pm_bar_node_ptr(st, s_tensor, G, bar_nodes, node_ptr) != PM_OK) return PM_E_INVALID;
  hipLaunchKernelGGL(k_mtp_fill<false>, dim3(G * 4), dim3(256), 0, st, c_logits, nullptr, s_tensor, node_ptr, N, mtp);
  return pm_check_launch();
}

extern "C" int pm_mtp_from_tokens(const int32_t* tokens, const float* s_tensor, int32_t G, int64_t N, int32_t* bar_nodes,
                                  int32_t* node_ptr, float* mtp, pm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if ((!tokens && N > 0) || !mtp || N < 0 || pm_bar_node_ptr(st, s_tensor, G, bar_nodes, node_ptr) != PM_OK) return PM_E_INVALID;
  hipLaunchKernelGGL(k_mtp_fill<true>, dim3(G * 4), dim3(256), 0, st, nullptr, tokens, s_tensor, node_ptr, N, mtp);
  return pm_check_launch();
}

extern "C" int pm_node_tracks(const float* s_tensor, int32_t G, int64_t N, int32_t* bar_nodes, int32_t* node_ptr,
                              uint8_t* node_track, pm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if ((!node_track && N > 0) || N < 0 || pm_bar_node_ptr(st, s_tensor, G, bar_nodes, node_ptr) != PM_OK) return PM_E_INVALID;
  hipLaunchKernelGGL(k_node_tracks, dim3(pm_cdiv(G, 4)), dim3(256), 0, st, s_tensor, node_ptr, G, N, node_track);
  return pm_check_launch();
}

extern "C" int pm_node_cells(const float* s_tensor, int32_t G, int64_t N, int32_t* bar_nodes, int32_t* node_ptr,
                             int32_t* node_cell, pm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if ((!node_cell && N > 0) || N < 0 || ((uintptr_t)node_cell & 3) != 0 || (int64_t)G * 128 > 0x7fffffffLL ||
      pm_bar_node_ptr(st, s_tensor, G, bar_nodes, node_ptr) != PM_OK)
    return PM_E_INVALID;
  hipLaunchKernelGGL(k_node_cells, dim3(pm_cdiv(G, 4)), dim3(256), 0, st, s_tensor, node_ptr, G, N, node_cell);
  return pm_check_launch();
}

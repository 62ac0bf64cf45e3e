// notes.hip — generated pieces as ordered note events (pm_notes_from_tokens): what the reference's `muspy_from_mtp`
// (utils.py:83-124) reads out of the pianoroll of pm_mtp_from_tokens, computed from the tokens themselves.  The pianoroll
// (13.8 KB per cell, active or not) is never written: 120 B of tokens are read per node, at most 15 rows of 12 B written.
//
//   cell order  : bar g = i * n_bars + b of piece i, track k, timestep s; an active cell's node is node_ptr[g] + the active
//                 cells before it in the bar (BarLanes of bars.h), its time t = 32 b + s.
//   slot loop   : the 15 (pitch, duration) pairs in order; stop at pitch EOS / PAD or duration EOS / PAD, skip pitch SOS,
//                 otherwise the note (t, pitch, min(duration + 1, 32 n_bars - t)).  The reference never tests for a duration
//                 SOS (utils.py:114-115 tests the pitch twice): token 96 is a note of length 97 before the clamp.  A token
//                 outside its head's range reads as 0, the arg-max of the all-zero head pm_mtp_from_tokens leaves.
//   order       : the reference appends per track, by time, then by slot: the rows of (piece i, track k) are one range, inside
//                 it bar after bar, inside a bar timestep after timestep.  A segment is one (piece, track, bar), numbered
//                 (4 i + k) * n_bars + b; its rows start at the exclusive scan of the segments' note counts.
// Launches: the bars' active cells and their scan (pm_bar_node_ptr), the segments' note counts, their scan (seg_ptr,
// track_ptr, totals), the rows.  The bar per wave (BarLanes), the half-wave sums and the scan are those of bars.h.
// No atomics: every row's position is a function of the inputs.  Integer work, exact.
#include "bars.h"

namespace {

constexpr int TOK_PER_NODE = 2 * PM_N_SLOTS;

// One cell's 15 token pairs in registers (read once, 8-byte loads), read the way the reference reads the cell.
struct Cell {
  int2 tk[PM_N_SLOTS];
  __device__ void load(const int32_t* __restrict__ tokens, int64_t n) {
    const int2* src = reinterpret_cast<const int2*>(tokens + n * TOK_PER_NODE);
#pragma unroll
    for (int j = 0; j < PM_N_SLOTS; ++j) tk[j] = src[j];
#pragma unroll
    for (int j = 0; j < PM_N_SLOTS; ++j) {
      if ((unsigned)tk[j].x >= (unsigned)PM_N_PITCH) tk[j].x = 0;
      if ((unsigned)tk[j].y >= (unsigned)PM_N_DUR) tk[j].y = 0;
    }
  }
  __device__ static bool ends(int2 t) { return t.x == PITCH_EOS || t.x == PITCH_PAD || t.y == DUR_EOS || t.y == DUR_PAD; }
  __device__ int count() const {
    int n = 0;
    bool live = true;
#pragma unroll
    for (int j = 0; j < PM_N_SLOTS; ++j) {
      live = live && !ends(tk[j]);
      n += (live && tk[j].x != PITCH_SOS) ? 1 : 0;
    }
    return n;
  }
  // rows [row, row + count()) of notes; nothing at or beyond `capacity`
  __device__ void emit(int32_t* __restrict__ notes, int64_t row, int64_t capacity, int t, int t_end) const {
    bool live = true;
#pragma unroll
    for (int j = 0; j < PM_N_SLOTS; ++j) {
      live = live && !ends(tk[j]);
      if (live && tk[j].x != PITCH_SOS && row < capacity) {
        int32_t* r = notes + row * 3;
        r[0] = t;
        r[1] = tk[j].x;
        r[2] = min(tk[j].y + 1, t_end - t);
        ++row;
      }
    }
  }
};

// exclusive scan of the segments' note counts into seg_ptr[0..n] (one workgroup); every n_bars-th entry of the scan is a
// track's first row, and the totals are written.
__global__ void __launch_bounds__(1024) k_notes_seg_scan(const int* __restrict__ a, int n, int* __restrict__ ptr, int n_bars,
                                                         int* __restrict__ track_ptr, const int* __restrict__ node_ptr, int G,
                                                         int* __restrict__ totals) {
  const int* const in[1] = {a};
  const BlockScan<1> sc(in, n);
  int ra = sc.pre[0];
  for (int i = sc.lo; i < sc.hi; ++i) {
    ptr[i] = ra;
    if (i % n_bars == 0) track_ptr[i / n_bars] = ra;
    ra += a[i];
  }
  if (threadIdx.x == 1023) {
    ptr[n] = sc.total[0];
    track_ptr[n / n_bars] = sc.total[0];
    totals[0] = sc.total[0];
    totals[1] = node_ptr[G];
  }
}

__global__ void __launch_bounds__(256) k_notes_count(const int32_t* __restrict__ tokens, const float* __restrict__ s,
                                                     const int* __restrict__ node_ptr, int G, int n_bars, int64_t N,
                                                     int* __restrict__ seg_count) {
  const int lane = threadIdx.x & 63, half = lane >> 5, t = lane & 31;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;                                                           // wave-uniform
  const BarLanes bl(s, node_ptr, g, lane, N);
  Cell c;
  int c0 = 0, c1 = 0;
  if (bl.on0) { c.load(tokens, bl.n0); c0 = c.count(); }
  if (bl.on1) { c.load(tokens, bl.n1); c1 = c.count(); }
  c0 = half_sum(c0);
  c1 = half_sum(c1);
  if (t == 0) {
    const int i = g / n_bars, b = g - i * n_bars;
    seg_count[(4 * i + half) * n_bars + b] = c0;
    seg_count[(4 * i + 2 + half) * n_bars + b] = c1;
  }
}

__global__ void __launch_bounds__(256) k_notes_emit(const int32_t* __restrict__ tokens, const float* __restrict__ s,
                                                    const int* __restrict__ node_ptr, const int* __restrict__ seg_ptr, int G,
                                                    int n_bars, int64_t N, int32_t* __restrict__ notes, int64_t capacity) {
  const int lane = threadIdx.x & 63, half = lane >> 5, t = lane & 31;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;                                                           // wave-uniform
  const BarLanes bl(s, node_ptr, g, lane, N);
  const int i = g / n_bars, b = g - i * n_bars, time = 32 * b + t, t_end = 32 * n_bars;
  Cell c;
  {
    int cnt = 0;
    if (bl.on0) { c.load(tokens, bl.n0); cnt = c.count(); }
    const int before = half_exclusive(cnt, t);                                  // (whole wave: shuffles)
    if (bl.on0) c.emit(notes, (int64_t)seg_ptr[(4 * i + half) * n_bars + b] + before, capacity, time, t_end);
  }
  {
    int cnt = 0;
    if (bl.on1) { c.load(tokens, bl.n1); cnt = c.count(); }
    const int before = half_exclusive(cnt, t);
    if (bl.on1) c.emit(notes, (int64_t)seg_ptr[(4 * i + 2 + half) * n_bars + b] + before, capacity, time, t_end);
  }
}

inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {     // int32 ranges [a, a + na), [b, b + nb)
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + 4 * (uintptr_t)nb && pb < pa + 4 * (uintptr_t)na;
}

}  // namespace

extern "C" int pm_notes_from_tokens(const int32_t* tokens, const float* s_tensor, int32_t G, int32_t n_bars, int64_t N,
                                    int32_t* seg_count, int32_t* seg_ptr, int32_t* bar_nodes, int32_t* node_ptr,
                                    int32_t* notes, int64_t capacity, int32_t* track_ptr, int32_t* totals,
                                    pm_stream_t stream) {
  if ((!tokens && N > 0) || !s_tensor || !seg_count || !seg_ptr || !bar_nodes || !node_ptr || (!notes && N > 0) || !track_ptr ||
      !totals || G <= 0 || n_bars <= 0 || N < 0)
    return PM_E_INVALID;
  if (G % n_bars != 0 || (int64_t)G * 128 > 0x7fffffffLL || N > 0x7fffffffLL / PM_N_SLOTS || capacity < PM_N_SLOTS * N)
    return PM_E_INVALID;
  if ((uintptr_t)tokens & 7) return PM_E_INVALID;                               // the token pairs are read as 8-byte words
  const int64_t S = 4 * (int64_t)G;
  const void* buf[7] = {seg_count, seg_ptr, bar_nodes, node_ptr, track_ptr, totals, notes};
  const int64_t len[7] = {S, S + 1, G, (int64_t)G + 1, S / n_bars + 1, 2, 3 * capacity};
  for (int a = 0; a < 7; ++a)
    for (int b = a + 1; b < 7; ++b)
      if (buf[a] && buf[b] && overlap(buf[a], len[a], buf[b], len[b])) return PM_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (pm_bar_node_ptr(st, s_tensor, G, bar_nodes, node_ptr) != PM_OK) return PM_E_INVALID;
  hipLaunchKernelGGL(k_notes_count, dim3(pm_cdiv(G, 4)), dim3(256), 0, st, tokens, s_tensor, node_ptr, G, n_bars, N, seg_count);
  hipLaunchKernelGGL(k_notes_seg_scan, dim3(1), dim3(1024), 0, st, seg_count, (int)S, seg_ptr, n_bars, track_ptr, node_ptr,
                     G, totals);
  hipLaunchKernelGGL(k_notes_emit, dim3(pm_cdiv(G, 4)), dim3(256), 0, st, tokens, s_tensor, node_ptr, seg_ptr, G, n_bars, N,
                     notes, capacity);
  return pm_check_launch();
}

// notes_in.hip — note events read back into bar graphs (pm_tokens_from_notes): the inverse of notes.hip.  What the reference's
// preprocessing (preprocess.py:118-157) does to the notes of one track on the host, plus the empty-bar rule of its graph
// construction (data.py:148-153), for a whole batch of pieces on the device, in the node numbering of every other kernel.
//
//   input       : notes [M,3] (time, pitch, duration) and track_ptr [4B+1], the NoteBatch layout: the rows of (piece i,
//                 track k) are one range, inside it the times do not decrease and lie in [0, 32 n_bars); rows behind the
//                 last range belong to no track (a NoteBatch's notes buffer is sized for the worst case).
//   cell        : (piece i, bar b, track k, timestep s) holds the rows of its track whose time is t = 32 b + s: the range
//                 [first row with time >= t, first row with time >= t + 1), found by binary search inside the track's range.
//                 The track's range is clamped into [0, M] first, so no search leaves `notes` whatever track_ptr holds; rows
//                 out of order make a search land somewhere else inside the same range (counted in `status`, never followed).
//   node        : the first 14 rows of a cell take the slots 1..14 in row order ("lowest position available"), later ones are
//                 dropped (the `continue` of preprocess.py:136-138); pitch token = clamp(pitch, 0, 127), duration token =
//                 clamp(duration, 1, 96) - 1; slot 0 is (SOS, SOS), the slot behind the last kept note (EOS, EOS), the rest
//                 (PAD, PAD).  A cell is active iff it has a row; a bar without one gets cell [0,0] with no note.
//   order       : nodes are the active cells in cell order (BarLanes of bars.h): node = node_ptr[g] + the active cells before
//                 it in the bar, the rows `ops.graph_build` numbers.
// Launches: the input check (a wave per track), the cells' row counts -> s_tensor and the bars' dropped notes (a bar per wave),
// the bars' active cells and their scan (pm_bar_node_ptr), the nodes' 128 B each (a bar per wave, the search repeated), the
// status sums (one wave).  No atomics and no LDS outside the scan: every byte written is a function of the inputs.
#include "bars.h"

namespace {

constexpr int DUR_SOS = 96;                                                     // constants.py:22-35 (bars.h has the others)
constexpr int NODE_SLOTS = PM_N_SLOTS + 1, MAX_NOTES = PM_N_SLOTS - 1;          // 16 slots: SOS, at most 14 notes, EOS
constexpr int MAX_PITCH = 127, MAX_DUR = 96;

// sum over the 64 lanes of a wave, in every lane
__device__ inline int wave_sum(int v) {
  v = half_sum(v);
  return v + __shfl_xor(v, 32, 64);
}

// the rows of track `tr` with 0 <= lo <= hi <= M, whatever track_ptr holds
struct TrackRange {
  int lo, hi;
  __device__ TrackRange(const int32_t* __restrict__ track_ptr, int tr, int M) {
    lo = min(max(track_ptr[tr], 0), M);
    hi = min(max(track_ptr[tr + 1], lo), M);
  }
};

// The rows of the two cells of a lane (BarLanes: cell `lane` of track lane >> 5, cell lane + 64 of track 2 + (lane >> 5), both
// at timestep lane & 31): beg / cnt.  Four binary searches (two times, two tracks) advance together, so their loads overlap;
// every load is inside the track's clamped range.
struct CellRows {
  int beg0, cnt0, beg1, cnt1;
  __device__ CellRows(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr, int M, int piece, int bar,
                      int lane) {
    const TrackRange ra(track_ptr, 4 * piece + (lane >> 5), M), rb(track_ptr, 4 * piece + 2 + (lane >> 5), M);
    const int t = 32 * bar + (lane & 31);
    int lo[4] = {ra.lo, ra.lo, rb.lo, rb.lo}, hi[4] = {ra.hi, ra.hi, rb.hi, rb.hi};
    for (;;) {
      bool live = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool open = lo[q] < hi[q];
        const int mid = lo[q] + ((hi[q] - lo[q]) >> 1);
        const int time = open ? notes[3 * (int64_t)mid] : 0;                    // lo <= mid < hi <= M
        if (open && time < t + (q & 1)) lo[q] = mid + 1;
        else if (open) hi[q] = mid;
        live = live || open;
      }
      if (!live) break;
    }
    beg0 = lo[0]; cnt0 = max(lo[1] - lo[0], 0);                                 // (negative only on rows out of order)
    beg1 = lo[2]; cnt1 = max(lo[3] - lo[2], 0);
  }
};

// one wave per track: rows out of time range, neighbours out of order, bad track_ptr entries -> track_bad[tr][3].  Entry 0 of
// track_ptr is bad unless it is 0; entry j >= 1 is bad when it is outside [0, M] or below entry j - 1.
__global__ void __launch_bounds__(256) k_notes_in_check(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                        int n_bars, int M, int* __restrict__ track_bad) {
  const int lane = threadIdx.x & 63, tr = blockIdx.x * 4 + (threadIdx.x >> 6);  // a block is a piece: tr < 4 B
  const TrackRange r(track_ptr, tr, M);
  const int t_end = 32 * n_bars;
  int range = 0, order = 0;
  for (int i = r.lo + lane; i < r.hi; i += 64) {
    const int t = notes[3 * (int64_t)i];
    range += (unsigned)t >= (unsigned)t_end ? 1 : 0;
    if (i + 1 < r.hi) order += t > notes[3 * (int64_t)(i + 1)] ? 1 : 0;
  }
  range = wave_sum(range);
  order = wave_sum(order);
  if (lane == 0) {
    const int p = track_ptr[tr], q = track_ptr[tr + 1];
    int bad = (q < 0 || q > M || q < p) ? 1 : 0;
    if (tr == 0 && p != 0) ++bad;
    track_bad[3 * tr] = range;
    track_bad[3 * tr + 1] = order;
    track_bad[3 * tr + 2] = bad;
  }
}

// one bar per wave: the cells' activity (fp32 0 / 1, an empty bar's cell [0,0] switched on) and the bar's dropped notes
__global__ void __launch_bounds__(256) k_notes_in_count(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                        int G, int n_bars, int M, float* __restrict__ s,
                                                        int* __restrict__ bar_dropped) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;                                                           // wave-uniform
  const int i = g / n_bars, b = g - i * n_bars;
  const CellRows c(notes, track_ptr, M, i, b, lane);
  bool a0 = c.cnt0 > 0;
  const bool a1 = c.cnt1 > 0;
  const bool empty = (__ballot(a0) | __ballot(a1)) == 0ull;
  if (empty && lane == 0) a0 = true;                                            // data.py:152-153
  s[(int64_t)g * 128 + lane] = a0 ? 1.0f : 0.0f;
  s[(int64_t)g * 128 + 64 + lane] = a1 ? 1.0f : 0.0f;
  const int dropped = wave_sum(max(c.cnt0 - MAX_NOTES, 0) + max(c.cnt1 - MAX_NOTES, 0));
  if (lane == 0) bar_dropped[g] = dropped;
}

// a node's 16 token pairs from the rows [beg, beg + cnt): the rows are read first, then eight 16-byte stores
__device__ inline void emit_node(int32_t* __restrict__ tokens, int64_t n, const int32_t* __restrict__ notes, int beg, int cnt) {
  const int kept = min(cnt, MAX_NOTES);
  int2 tk[NODE_SLOTS];
  tk[0] = make_int2(PITCH_SOS, DUR_SOS);
#pragma unroll
  for (int j = 1; j < NODE_SLOTS; ++j) {
    tk[j] = j == kept + 1 ? make_int2(PITCH_EOS, DUR_EOS) : make_int2(PITCH_PAD, DUR_PAD);
    if (j <= kept) {                                                            // row beg + j - 1 < beg + cnt <= M
      const int32_t* r = notes + 3 * (int64_t)(beg + j - 1);
      tk[j] = make_int2(min(max(r[1], 0), MAX_PITCH), min(max(r[2], 1), MAX_DUR) - 1);
    }
  }
  int4* dst = reinterpret_cast<int4*>(tokens + n * (2 * NODE_SLOTS));
#pragma unroll
  for (int j = 0; j < NODE_SLOTS; j += 2) dst[j >> 1] = make_int4(tk[j].x, tk[j].y, tk[j + 1].x, tk[j + 1].y);
}

// one bar per wave: the nodes of the bar's active cells; nothing at or beyond node `capacity`
__global__ void __launch_bounds__(256) k_notes_in_emit(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                       const float* __restrict__ s, const int* __restrict__ node_ptr, int G,
                                                       int n_bars, int M, int32_t* __restrict__ tokens, int64_t capacity) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;                                                           // wave-uniform
  const BarLanes bl(s, node_ptr, g, lane, capacity);
  const int i = g / n_bars, b = g - i * n_bars;
  const CellRows c(notes, track_ptr, M, i, b, lane);
  if (bl.on0) emit_node(tokens, bl.n0, notes, c.beg0, c.cnt0);
  if (bl.on1) emit_node(tokens, bl.n1, notes, c.beg1, c.cnt1);
}

// one wave: status = {rows out of range, rows out of order, bad track_ptr entries, dropped notes, nodes}
__global__ void __launch_bounds__(64) k_notes_in_status(const int* __restrict__ track_bad, int tracks,
                                                        const int* __restrict__ bar_dropped, const int* __restrict__ node_ptr,
                                                        int G, int* __restrict__ status) {
  const int lane = threadIdx.x;
  int range = 0, order = 0, bad = 0, dropped = 0;
  for (int i = lane; i < tracks; i += 64) {
    range += track_bad[3 * i];
    order += track_bad[3 * i + 1];
    bad += track_bad[3 * i + 2];
  }
  for (int g = lane; g < G; g += 64) dropped += bar_dropped[g];
  range = wave_sum(range);
  order = wave_sum(order);
  bad = wave_sum(bad);
  dropped = wave_sum(dropped);
  if (lane == 0) {
    status[0] = range;
    status[1] = order;
    status[2] = bad;
    status[3] = dropped;
    status[4] = node_ptr[G];
  }
}

inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {     // 4-byte element ranges [a, a + na), [b, b + nb)
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + 4 * (uintptr_t)nb && pb < pa + 4 * (uintptr_t)na;
}

}  // namespace

extern "C" int pm_tokens_from_notes(const int32_t* notes, const int32_t* track_ptr, int32_t B, int32_t n_bars, int64_t M,
                                    float* s_tensor, int32_t* tokens, int64_t capacity, int32_t* scratch, int32_t* status,
                                    pm_stream_t stream) {
  if ((!notes && M > 0) || !track_ptr || !s_tensor || (!tokens && capacity > 0) || !scratch || !status || B <= 0 || n_bars <= 0 ||
      M < 0 || capacity < 0)
    return PM_E_INVALID;
  const int64_t G = (int64_t)B * n_bars;
  if (G * 128 > 0x7fffffffLL || M > 0x7fffffffLL / 3 || capacity > 0x7fffffffLL / (2 * NODE_SLOTS)) return PM_E_INVALID;
  if (((uintptr_t)notes | (uintptr_t)track_ptr | (uintptr_t)s_tensor | (uintptr_t)scratch | (uintptr_t)status) & 3)
    return PM_E_INVALID;
  if ((uintptr_t)tokens & 15) return PM_E_INVALID;                              // a node is written as 16-byte words
  const int64_t tracks = 4 * (int64_t)B;
  const void* buf[6] = {notes, track_ptr, s_tensor, tokens, scratch, status};
  const int64_t len[6] = {3 * M, tracks + 1, 128 * G, 2 * NODE_SLOTS * capacity, PM_NOTES_IN_SCRATCH(B, n_bars), 5};
  for (int a = 0; a < 6; ++a)
    for (int b = (a == 0 ? 2 : a + 1); b < 6; ++b)                              // (the two inputs may share memory)
      if (buf[a] && buf[b] && len[a] > 0 && len[b] > 0 && overlap(buf[a], len[a], buf[b], len[b])) return PM_E_INVALID;
  int32_t *bar_nodes = scratch, *node_ptr = scratch + G, *bar_dropped = scratch + 2 * G + 1, *track_bad = scratch + 3 * G + 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_notes_in_check, dim3(B), dim3(256), 0, st, notes, track_ptr, n_bars, (int)M, track_bad);
  hipLaunchKernelGGL(k_notes_in_count, dim3(pm_cdiv(G, 4)), dim3(256), 0, st, notes, track_ptr, (int)G, n_bars, (int)M, s_tensor,
                     bar_dropped);
  if (pm_bar_node_ptr(st, s_tensor, (int)G, bar_nodes, node_ptr) != PM_OK) return PM_E_INVALID;
  hipLaunchKernelGGL(k_notes_in_emit, dim3(pm_cdiv(G, 4)), dim3(256), 0, st, notes, track_ptr, s_tensor, node_ptr, (int)G, n_bars,
                     (int)M, tokens, capacity);
  hipLaunchKernelGGL(k_notes_in_status, dim3(1), dim3(64), 0, st, track_bad, (int)tracks, bar_dropped, node_ptr, (int)G, status);
  return pm_check_launch();
}

// splice.hip — bar ranges of the pieces of a NoteBatch copied into bar ranges of new pieces (pm_notes_splice): what cuts songs
// into model windows (preprocess.py:165-205: the window by onset time, the silence filters, the transposition) and what puts
// windows behind each other again.
//   segment   : (src_piece, src_bar, out_bar, bars); output piece j owns segments[seg_ptr[j] : seg_ptr[j + 1]] and walks them in
//               that order.  One that breaks a rule (SegWalk below) copies nothing and is counted.
//   layout    : a wave per (output piece, track), the four tracks of a piece per 256-thread workgroup (k_select_len's).  Per
//               segment the wave scans the whole clamped range of the source track (TrackRange, as stats.hip restates it), 64
//               rows at a time; a row goes along iff 32 src_bar <= t < 32 (src_bar + bars), by its onset alone.
//   order     : the rows that go along keep the source's order: a ballot of the chunk, the popcount of the lanes below, and a
//               running base across chunks and segments.  tokens_from_notes assigns slots in row order, so this is part of
//               the result, not a detail.
//   Three launches: counts (rows, cells, the 64-bit mask of bars that hold a row, the segments and seg_ptr entries that were
//   not followed), one workgroup that scans them (BlockScan of bars.h) and decides `keep` from the four masks of a piece, the
//   rows.  No global atomics; every output word but the rows behind the total is written on every call.
#include "bars.h"

namespace {

constexpr int MAX_PITCH = 127, MAX_RULE_BARS = 64;

__device__ inline int wave_sum(int v) {
  v = half_sum(v);
  return v + __shfl_xor(v, 32, 64);
}

// the rows of track `tr` with 0 <= lo <= hi <= M, whatever track_ptr holds (as in notes_in.hip)
struct TrackRange {
  int lo, hi;
  __device__ TrackRange(const int32_t* __restrict__ track_ptr, int64_t tr, int M) {
    lo = min(max(track_ptr[tr], 0), M);
    hi = min(max(track_ptr[tr + 1], lo), M);
  }
};

// The segments of output piece j, one after the other (wave-uniform).  seg_ptr is clamped as TrackRange clamps track_ptr:
// 0 <= lo <= hi <= S.  A segment is followed iff 0 <= src_piece < B, bars >= 1, 0 <= src_bar, src_bar + bars <= src_bars,
// out_bar >= the end of the last followed segment of this piece (0 in front of the first) and out_bar + bars <= out_bars.
struct SegWalk {
  int s, hi, end, B, src_bars, out_bars;
  int piece, src_bar, out_bar, bars;                                            // the segment next() stopped at
  __device__ SegWalk(const int32_t* __restrict__ seg_ptr, int j, int S, int B_, int src_bars_, int out_bars_)
      : end(0), B(B_), src_bars(src_bars_), out_bars(out_bars_) {
    s = min(max(seg_ptr[j], 0), S);
    hi = min(max(seg_ptr[j + 1], s), S);
  }
  // false behind the last segment; else `ok` tells whether the segment is followed
  __device__ bool next(const int32_t* __restrict__ segments, bool& ok) {
    if (s >= hi) return false;
    const int32_t* g = segments + 4 * (int64_t)s;                               // 0 <= s < S
    ++s;
    piece = g[0]; src_bar = g[1]; out_bar = g[2]; bars = g[3];
    ok = piece >= 0 && piece < B && bars >= 1 && src_bar >= 0 && (int64_t)src_bar + bars <= src_bars && out_bar >= end &&
         (int64_t)out_bar + bars <= out_bars;
    if (ok) end = out_bar + bars;
    return true;
  }
};

// a wave per (output piece j, track k): rows and cells of the track, the bars that hold a row; in the entry of track 0 the
// segments that were not followed and the seg_ptr entries that break the contract (entry j + 1, block 0 entry 0 as well)
__global__ void __launch_bounds__(256) k_splice_count(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                      int B, int src_bars, int M, const int32_t* __restrict__ segments,
                                                      const int32_t* __restrict__ seg_ptr, int S, int out_bars, int want_mask,
                                                      int* __restrict__ len, int* __restrict__ cells, int* __restrict__ bad_seg,
                                                      int* __restrict__ bad_ptr, uint32_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6, j = blockIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  SegWalk w(seg_ptr, j, S, B, src_bars, out_bars);
  int n = 0, c = 0, skipped = 0;
  unsigned long long act = 0ull;                                                // bit b: bar b of the output holds a row
  bool ok;
  while (w.next(segments, ok)) {
    if (!ok) { ++skipped; continue; }
    const TrackRange r(track_ptr, 4 * (int64_t)w.piece + k, M);
    const int t0 = 32 * w.src_bar, t1 = 32 * (w.src_bar + w.bars);              // <= 32 src_bars < 2^31
    int last = 0;                                                               // time of the last row taken, if any
    bool any = false;
    for (int base = r.lo; base < r.hi; base += 64) {                            // wave-uniform
      const int i = base + lane;
      const int t = i < r.hi ? notes[3 * (int64_t)i] : 0;                       // lo <= i < hi <= M
      const bool take = i < r.hi && t >= t0 && t < t1;
      const unsigned long long m = __ballot(take);
      if (m == 0ull) continue;
      const unsigned long long before = m & below;
      const int prev_lane = before ? 63 - __clzll(before) : 0;
      const int t_prev = __shfl(t, prev_lane, 64);                              // (every lane takes part)
      if (take) {
        c += before ? (t != t_prev ? 1 : 0) : ((!any || t != last) ? 1 : 0);
        if (want_mask) act |= 1ull << (w.out_bar + ((t - t0) >> 5));            // a bar below out_bars <= 64
      }
      n += __popcll(m);
      last = __shfl(t, 63 - __clzll(m), 64);
      any = true;
    }
  }
  c = wave_sum(c);
  uint32_t a_lo = (uint32_t)act, a_hi = (uint32_t)(act >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a_lo |= (uint32_t)__shfl_xor((int)a_lo, o, 64);
    a_hi |= (uint32_t)__shfl_xor((int)a_hi, o, 64);
  }
  if (lane == 0) {
    const int64_t u = 4 * (int64_t)j + k;
    int bad = 0;
    if (k == 0) {
      const int e = seg_ptr[j + 1];
      bad = (e < 0 || e > S || e < seg_ptr[j]) ? 1 : 0;
      if (j == 0 && (seg_ptr[0] < 0 || seg_ptr[0] > S)) ++bad;
    }
    len[u] = n;
    cells[u] = c;
    bad_seg[u] = k == 0 ? skipped : 0;
    bad_ptr[u] = bad;
    mask[2 * u] = a_lo;
    mask[2 * u + 1] = a_hi;
  }
}

// preprocess.py:176-194 on the four masks of a piece (bit b: the track has a row in bar b), W = out_bars <= 64
__device__ inline int keeps(const uint32_t* __restrict__ m8, int W) {
  unsigned long long act[4], all = 0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    act[k] = (unsigned long long)m8[2 * k] | ((unsigned long long)m8[2 * k + 1] << 32);
    all |= act[k];
  }
  if (W == 1) return (all & 1ull) ? 1 : 0;                                      // all four tracks silent
  const unsigned long long full = W >= 64 ? ~0ull : (1ull << W) - 1ull;
  if (~all & full) return 0;                                                    // a bar silent in every track
  int prev_last = -2;                                                           // the last silent bar met so far
  for (int k = 0; k < 4; ++k) {                                                 // the silent (track, bar) pairs in row-major order
    const unsigned long long silent = ~act[k] & full;
    if (!silent) continue;
    if (silent & (silent >> 1)) return 0;                                       // two consecutive silent bars of one track
    if (__ffsll((long long)silent) - 1 == prev_last + 1) return 0;              // ... or of two tracks that follow each other
    prev_last = 63 - __clzll(silent);
  }
  return 1;
}

// one workgroup: out_track_ptr = the scan of len, totals = (rows, cells), status, keep
__global__ void __launch_bounds__(1024) k_splice_scan(const int* __restrict__ len, const int* __restrict__ cells,
                                                      const int* __restrict__ bad_seg, const int* __restrict__ bad_ptr,
                                                      const uint32_t* __restrict__ mask, int K, int out_bars, int silence_rule,
                                                      int64_t capacity, int32_t* __restrict__ out_track_ptr,
                                                      int32_t* __restrict__ totals, int32_t* __restrict__ keep,
                                                      int32_t* __restrict__ status) {
  const int* const a[4] = {len, cells, bad_seg, bad_ptr};
  const int tracks = 4 * K;
  const BlockScan<4> sc(a, tracks);
  int pre = sc.pre[0];
  for (int i = sc.lo; i < sc.hi; ++i) {
    out_track_ptr[i] = pre;
    pre += len[i];
  }
  for (int j = threadIdx.x; j < K; j += 1024) keep[j] = silence_rule ? keeps(mask + 8 * (int64_t)j, out_bars) : 1;
  if (threadIdx.x == 0) {
    out_track_ptr[tracks] = sc.total[0];
    totals[0] = sc.total[0];
    totals[1] = sc.total[1];
    status[0] = sc.total[2];
    status[1] = sc.total[3];
    status[2] = (int32_t)max((int64_t)sc.total[0] - capacity, (int64_t)0);
    status[3] = 0;
  }
}

// a wave per (output piece, track): the rows, segment by segment, from out_track_ptr[u] on; nothing at or beyond row `capacity`
__global__ void __launch_bounds__(256) k_splice_copy(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                     int B, int src_bars, int M, const int32_t* __restrict__ segments,
                                                     const int32_t* __restrict__ seg_ptr, int S, int out_bars,
                                                     const int32_t* __restrict__ shift, const int* __restrict__ len,
                                                     const int32_t* __restrict__ out_track_ptr, int32_t* __restrict__ out_notes,
                                                     int64_t capacity) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6, j = blockIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t u = 4 * (int64_t)j + k;
  if (len[u] <= 0) return;
  int64_t dst = out_track_ptr[u];
  if (dst < 0) return;                                                          // (a sum beyond int32)
  const bool transpose = shift != nullptr && k > 0;                             // never the drums
  const int sh = transpose ? shift[j] : 0;
  SegWalk w(seg_ptr, j, S, B, src_bars, out_bars);
  bool ok;
  while (w.next(segments, ok)) {
    if (!ok) continue;
    const TrackRange r(track_ptr, 4 * (int64_t)w.piece + k, M);
    const int t0 = 32 * w.src_bar, t1 = 32 * (w.src_bar + w.bars), rebase = 32 * w.out_bar - t0;
    for (int base = r.lo; base < r.hi; base += 64) {
      const int i = base + lane;
      const int32_t* row = notes + 3 * (int64_t)(i < r.hi ? i : r.lo);          // lo <= i < hi <= M, or row lo again
      const int t = row[0];
      const bool take = i < r.hi && t >= t0 && t < t1;
      const unsigned long long m = __ballot(take);
      const int64_t pos = dst + __popcll(m & below);
      if (take && pos < capacity) {                                             // 0 <= pos < capacity
        int p = row[1];
        if (transpose) {                                                        // preprocess.py:196-205 on the pitch token
          const int64_t q = (int64_t)min(max(p, 0), MAX_PITCH) + sh;
          p = (int)min(max(q, (int64_t)0), (int64_t)MAX_PITCH);
        }
        int32_t* out = out_notes + 3 * pos;
        out[0] = t + rebase;
        out[1] = p;
        out[2] = row[2];
      }
      dst += __popcll(m);
    }
  }
}

struct Buf { const void* p; int64_t words; bool written; };

// a buffer that is written may share no byte with any other; two that are only read may
inline bool clash(const Buf* b, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      if (!(b[i].written || b[j].written) || !b[i].p || !b[j].p || b[i].words <= 0 || b[j].words <= 0) continue;
      const uintptr_t pi = (uintptr_t)b[i].p, pj = (uintptr_t)b[j].p;
      if (pi < pj + 4 * (uintptr_t)b[j].words && pj < pi + 4 * (uintptr_t)b[i].words) return true;
    }
  return false;
}

inline bool misaligned(const Buf* b, int n) {
  uintptr_t all = 0;
  for (int i = 0; i < n; ++i) all |= (uintptr_t)b[i].p;
  return (all & 3) != 0;
}

}  // namespace

extern "C" int pm_notes_splice(const int32_t* notes, const int32_t* track_ptr, int32_t B, int32_t src_bars, int64_t M,
                               const int32_t* segments, int32_t S, const int32_t* seg_ptr, int32_t K, int32_t out_bars,
                               const int32_t* shift, int32_t silence_rule, int32_t* out_notes, int64_t capacity,
                               int32_t* out_track_ptr, int32_t* out_totals, int32_t* keep, int32_t* scratch, int32_t* status,
                               pm_stream_t stream) {
  if ((!notes && M > 0) || !track_ptr || (!segments && S > 0) || !seg_ptr || (!out_notes && capacity > 0) || !out_track_ptr ||
      !out_totals || !keep || !scratch || !status || B <= 0 || K < 1 || S < 0 || M < 0 || capacity < 0 || src_bars < 1 ||
      out_bars < 1 || (silence_rule != 0 && silence_rule != 1) || (silence_rule && out_bars > MAX_RULE_BARS))
    return PM_E_INVALID;
  const int64_t tracks = 4 * (int64_t)K, lim = 0x7fffffffLL;
  if (M > lim / 3 || capacity > lim / 3 || 4 * (int64_t)B + 1 > lim || 4 * (int64_t)S > lim || src_bars > lim / 32 ||
      out_bars > lim / 32 || PM_SPLICE_SCRATCH(K, S) > lim)
    return PM_E_INVALID;
  const Buf buf[11] = {{notes, 3 * M, false}, {track_ptr, 4 * (int64_t)B + 1, false}, {segments, 4 * (int64_t)S, false},
                       {seg_ptr, (int64_t)K + 1, false}, {shift, K, false}, {out_notes, 3 * capacity, true},
                       {out_track_ptr, tracks + 1, true}, {out_totals, 2, true}, {keep, K, true},
                       {scratch, PM_SPLICE_SCRATCH(K, S), true}, {status, 4, true}};
  if (misaligned(buf, 11) || clash(buf, 11)) return PM_E_INVALID;
  int32_t *len = scratch, *cells = len + tracks, *bad_seg = cells + tracks, *bad_ptr = bad_seg + tracks;
  uint32_t* mask = (uint32_t*)(bad_ptr + tracks);                               // [4K][2]
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_splice_count, dim3(K), dim3(256), 0, st, notes, track_ptr, B, src_bars, (int)M, segments, seg_ptr, S,
                     out_bars, out_bars <= MAX_RULE_BARS ? 1 : 0, len, cells, bad_seg, bad_ptr, mask);
  hipLaunchKernelGGL(k_splice_scan, dim3(1), dim3(1024), 0, st, len, cells, bad_seg, bad_ptr, mask, K, out_bars, silence_rule,
                     capacity, out_track_ptr, out_totals, keep, status);
  hipLaunchKernelGGL(k_splice_copy, dim3(K), dim3(256), 0, st, notes, track_ptr, B, src_bars, (int)M, segments, seg_ptr, S,
                     out_bars, shift, len, out_track_ptr, out_notes, capacity);
  return pm_check_launch();
}

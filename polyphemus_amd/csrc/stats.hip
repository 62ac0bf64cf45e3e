// stats.hip — what a NoteBatch holds, counted on the device (pm_note_stats, pm_note_chroma), and a subset of its pieces
// (pm_notes_select).
//
// pm_note_stats: the small integer reductions behind the usual objective measures of symbolic music (pitch range, pitches and
// pitch classes used, polyphony, empty beats, groove: muspy.metrics), per (piece, track), from the rows the encoder would see.
//   row       : (t, p, d) of a track is counted iff 0 <= t < L = 32 n_bars, as the note q = clamp(p, 0, 127) of length
//               e = clamp(d, 1, 96) sounding over the steps [t, min(t + e, L)); other rows go to out_of_range only.
//   layout    : a wave per track, the four tracks of a piece per 256-thread workgroup (k_notes_in_check's); the track's range
//               is clamped into [0, M] (TrackRange of notes_in.hip, restated here), lanes stride over its rows.
//   counters  : the wave's slice of LDS holds, per step, the difference array of the sounding count (+1 at t, -1 at the end
//               unless the end is L) and the onset count: 2 L int32, 16 KB per wave at n_bars = 64, the limit.  Integer LDS
//               adds only, so the sums do not depend on the order in which rows arrive.
//   scan      : 64 steps at a time: a wave prefix sum of the difference array gives the notes sounding at every step, ballots
//               give the onset and sounding masks (two 32-bit words per 64 steps) and the step counts, a running maximum the
//               largest chord and polyphony.  Sums, minima, maxima and the 128-bit pitch set end in wave reductions.
//   One launch, no global atomics, no workspace: 12 B read per row, 96 + 8 n_bars B written per track, every word on every call.
//
// pm_note_chroma: the chromagram of a NoteBatch, chroma[track][segment][pitch class] = the (note, step) pairs of that class
// sounding in the segment (segments of 1 .. 32 steps), by the row rule of pm_note_stats.
//   layout    : per-pitch-class difference arrays over a chunk of 16 bars per workgroup (12 x 512 int32 = 24 KB of LDS; the
//               whole piece at n_bars = 64 would need 96 KB per track), grid (4 B tracks, ceil(n_bars / 16) chunks), 256 threads
//               striding over the track's rows and clipping every note to the chunk.  A smaller chunk would read the rows
//               more often (every chunk reads all rows of its track: at most 4 x 12 B per row), a larger one would leave the
//               64 KB budget with less than two workgroups per CU; 16 bars keeps short pieces (n_bars <= 16) at one read.
//   sums      : integer LDS adds, a wave prefix sum per class and xor-shuffle sums per segment: no global atomics, no
//               workspace, every word written by exactly one workgroup on every call, bit-identical from call to call.
//   One launch: 12 B read per row and chunk, 48 B written per segment and track, as coalesced runs.
//
// pm_notes_select: pieces index[0..K) of a NoteBatch as a NoteBatch.  first[b] = lowest position j with index[j] = b (an
// integer minimum, so it does not depend on arrival order); output piece j is piece index[j] iff that is in [0, B) and
// first[index[j]] = j, else empty.  Five launches: first = INT_MAX, the minimum, the chosen tracks' clamped lengths and cells (a
// wave per track), their scan by one workgroup (BlockScan of bars.h) with the totals and the status, the rows.
#include "bars.h"

#include <climits>

namespace {

constexpr int MAX_PITCH = 127, MAX_DUR = 96, MAX_BARS = 64;
constexpr int N_STAT = 12, N_PC = 12;                                           // PM_NOTE_STAT_* of the header

__device__ inline int wave_sum(int v) {
  v = half_sum(v);
  return v + __shfl_xor(v, 32, 64);
}
__device__ inline int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
// inclusive prefix sum over the 64 lanes of a wave
__device__ inline int wave_inclusive(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  return v;
}

// the rows of track `tr` with 0 <= lo <= hi <= M, whatever track_ptr holds (as in notes_in.hip)
struct TrackRange {
  int lo, hi;
  __device__ TrackRange(const int32_t* __restrict__ track_ptr, int64_t tr, int M) {
    lo = min(max(track_ptr[tr], 0), M);
    hi = min(max(track_ptr[tr + 1], lo), M);
  }
};

__global__ void __launch_bounds__(256) k_note_stats(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                    int n_bars, int M, int32_t* __restrict__ track,
                                                    int32_t* __restrict__ pitch_class, int32_t* __restrict__ onsets,
                                                    int32_t* __restrict__ sounding) {
  extern __shared__ int lds[];                                                  // [4 waves][2 L]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = 32 * n_bars;
  const int64_t tr = (int64_t)blockIdx.x * 4 + wave;                            // a block is a piece: tr < 4 B
  int* diff = lds + wave * 2 * L;                                               // sounding count of step s minus that of s - 1
  int* ons = diff + L;                                                          // onsets at step s
  for (int s = lane; s < L; s += 64) diff[s] = ons[s] = 0;
  __syncthreads();

  const TrackRange r(track_ptr, tr, M);
  int n = 0, steps = 0, outside = 0, pmin = 128, pmax = -1, pc[N_PC];
  uint32_t set[4] = {0u, 0u, 0u, 0u};                                           // bit q: pitch q is used
#pragma unroll
  for (int c = 0; c < N_PC; ++c) pc[c] = 0;
  for (int i = r.lo + lane; i < r.hi; i += 64) {                                // lo <= i < hi <= M
    const int32_t* row = notes + 3 * (int64_t)i;
    const int t = row[0], q = min(max(row[1], 0), MAX_PITCH), e = min(max(row[2], 1), MAX_DUR);
    if ((unsigned)t >= (unsigned)L) { ++outside; continue; }
    const int end = min(t + e, L), qc = q % 12;
    ++n;
    steps += end - t;
    pmin = min(pmin, q); pmax = max(pmax, q);
#pragma unroll
    for (int w = 0; w < 4; ++w) set[w] |= (q >> 5) == w ? 1u << (q & 31) : 0u;
#pragma unroll
    for (int c = 0; c < N_PC; ++c) pc[c] += qc == c ? 1 : 0;
    atomicAdd(&ons[t], 1);                                                      // 0 <= t < L
    atomicAdd(&diff[t], 1);
    if (end < L) atomicAdd(&diff[end], -1);                                     // t < end < L
  }
  __syncthreads();

  int carry = 0, n_onsets = 0, n_sound = 0, n_poly = 0, max_poly = 0, max_chord = 0;
  int32_t* on_w = onsets + tr * n_bars;
  int32_t* so_w = sounding + tr * n_bars;
  for (int base = 0; base < L; base += 64) {                                    // wave-uniform; L is a multiple of 32
    const int s = base + lane;
    const int inc = wave_inclusive(s < L ? diff[s] : 0, lane);
    const int cur = s < L ? carry + inc : 0, o = s < L ? ons[s] : 0;            // notes sounding at step s, onsets at it
                                                                                // (a note that ends at L has no -1: mask s >= L)
    carry += __shfl(inc, 63, 64);
    const unsigned long long b_on = __ballot(o > 0), b_so = __ballot(cur > 0);
    n_onsets += __popcll(b_on);
    n_sound += __popcll(b_so);
    n_poly += __popcll(__ballot(cur > 1));
    max_poly = max(max_poly, cur);
    max_chord = max(max_chord, o);
    if (lane == 0 || (lane == 32 && base + 32 < L)) {                           // bars base / 32 and base / 32 + 1
      const int b = (base >> 5) + (lane >> 5);
      on_w[b] = (int32_t)(uint32_t)(b_on >> lane);
      so_w[b] = (int32_t)(uint32_t)(b_so >> lane);
    }
  }

  n = wave_sum(n); steps = wave_sum(steps); outside = wave_sum(outside);
  pmin = -wave_max(-pmin); pmax = wave_max(pmax);
  max_poly = wave_max(max_poly); max_chord = wave_max(max_chord);
  int n_pitches = 0, n_classes = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) n_pitches += __popc(wave_or(set[w]));
#pragma unroll
  for (int c = 0; c < N_PC; ++c) {
    pc[c] = wave_sum(pc[c]);
    n_classes += pc[c] > 0 ? 1 : 0;
  }
  if (lane == 0) {
    int32_t* rec = track + tr * N_STAT;
    rec[PM_NOTE_STAT_N_NOTES] = n;
    rec[PM_NOTE_STAT_N_ONSETS] = n_onsets;
    rec[PM_NOTE_STAT_PITCH_MIN] = pmin;
    rec[PM_NOTE_STAT_PITCH_MAX] = pmax;
    rec[PM_NOTE_STAT_N_PITCHES] = n_pitches;
    rec[PM_NOTE_STAT_N_PITCH_CLASSES] = n_classes;
    rec[PM_NOTE_STAT_NOTE_STEPS] = steps;
    rec[PM_NOTE_STAT_SOUNDING_STEPS] = n_sound;
    rec[PM_NOTE_STAT_POLY_STEPS] = n_poly;
    rec[PM_NOTE_STAT_MAX_POLYPHONY] = max_poly;
    rec[PM_NOTE_STAT_MAX_CHORD] = max_chord;
    rec[PM_NOTE_STAT_OUT_OF_RANGE] = outside;
#pragma unroll
    for (int c = 0; c < N_PC; ++c) pitch_class[tr * N_PC + c] = pc[c];
  }
}

// pm_note_chroma: a workgroup per (track, chunk of CHROMA_BARS bars).  diff[c][x] is the difference array of the notes of
// pitch class c sounding at step x of the chunk; every thread strides over the track's rows and clips a note to the chunk
// (a note that began before the chunk starts at its step 0, so no carry crosses chunks).  Wave w then scans the classes
// w, w + 4, w + 8, 64 steps at a time, sums the counts of every segment with xor shuffles (a segment is an aligned power of
// two of at most 32 lanes) and leaves them in place at diff[c][segment of the chunk]: the segments written in one round lie
// at or below the steps read in it and above those written in the round before.  The whole block stores them as one
// contiguous run of chroma words.
constexpr int CHROMA_BARS = 16;

__global__ void __launch_bounds__(256) k_note_chroma(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                     int n_bars, int M, int seg_steps, int32_t* __restrict__ chroma) {
  extern __shared__ int lds[];                                                  // [12][CH]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = 32 * n_bars;
  const int CH = 32 * min(n_bars, CHROMA_BARS);                                 // steps of a whole chunk
  const int64_t tr = blockIdx.x;                                                // tr < 4 B
  const int c0 = (int)blockIdx.y * CH, c1 = min(c0 + CH, L), len = c1 - c0;     // this chunk: steps [c0, c1), 0 < len <= CH
  for (int i = threadIdx.x; i < N_PC * CH; i += 256) lds[i] = 0;
  __syncthreads();

  const TrackRange r(track_ptr, tr, M);
  for (int i = r.lo + (int)threadIdx.x; i < r.hi; i += 256) {                   // lo <= i < hi <= M
    const int32_t* row = notes + 3 * (int64_t)i;
    const int t = row[0], q = min(max(row[1], 0), MAX_PITCH), e = min(max(row[2], 1), MAX_DUR);
    if ((unsigned)t >= (unsigned)L) continue;
    const int from = max(t, c0), to = min(min(t + e, L), c1);
    if (from >= to) continue;                                                   // the note does not sound in this chunk
    int* diff = lds + (q % 12) * CH;
    atomicAdd(&diff[from - c0], 1);                                             // 0 <= from - c0 < len
    if (to < c1) atomicAdd(&diff[to - c0], -1);                                 // 0 < to - c0 < len
  }
  __syncthreads();

  for (int c = wave; c < N_PC; c += 4) {
    int* diff = lds + c * CH;
    int carry = 0;
    for (int base = 0; base < len; base += 64) {                                // wave-uniform; len is a multiple of 32
      const int x = base + lane;
      const int inc = wave_inclusive(x < len ? diff[x] : 0, lane);
      int cur = x < len ? carry + inc : 0;                                      // notes of class c sounding at step c0 + x
      carry += __shfl(inc, 63, 64);
      for (int o = 1; o < seg_steps; o <<= 1) cur += __shfl_xor(cur, o, 64);
      if (x < len && (lane & (seg_steps - 1)) == 0) diff[x / seg_steps] = cur;
    }
  }
  __syncthreads();

  const int S = L / seg_steps, segs = len / seg_steps;                          // segments of the piece, of this chunk
  int32_t* out = chroma + (tr * S + c0 / seg_steps) * N_PC;
  for (int i = threadIdx.x; i < segs * N_PC; i += 256) out[i] = lds[(i % N_PC) * CH + i / N_PC];
}

__global__ void __launch_bounds__(256) k_select_init(int* __restrict__ first, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) first[b] = INT_MAX;
}

__global__ void __launch_bounds__(256) k_select_mark(const int32_t* __restrict__ index, int K, int B, int* __restrict__ first) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const int b = index[j];
  if (b >= 0 && b < B) atomicMin(&first[b], j);                                 // the lowest position keeps the piece
}

// a wave per chosen track (block j = output piece j): its clamped length and its cells, 0 for a piece that is not followed;
// oor / rep hold the piece's flag in the entry of its track 0, so that one scan sums all four arrays
__global__ void __launch_bounds__(256) k_select_len(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                    int B, int M, const int32_t* __restrict__ index,
                                                    const int* __restrict__ first, int* __restrict__ len,
                                                    int* __restrict__ cells, int* __restrict__ oor, int* __restrict__ rep) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6, j = blockIdx.x;
  const int b = index[j];
  const bool inside = b >= 0 && b < B;
  const bool taken = inside && first[b] == j;                                   // block-uniform
  int n = 0, c = 0;
  if (taken) {
    const TrackRange r(track_ptr, 4 * (int64_t)b + k, M);
    n = r.hi - r.lo;
    for (int i = r.lo + lane; i < r.hi; i += 64)                                // lo <= i - 1 < i < hi <= M behind the first row
      c += (i == r.lo || notes[3 * (int64_t)i] != notes[3 * (int64_t)(i - 1)]) ? 1 : 0;
  }
  c = wave_sum(c);
  if (lane == 0) {
    const int64_t u = 4 * (int64_t)j + k;
    len[u] = n;
    cells[u] = c;
    oor[u] = (k == 0 && !inside) ? 1 : 0;
    rep[u] = (k == 0 && inside && !taken) ? 1 : 0;
  }
}

// one workgroup: out_track_ptr = the scan of len, totals = (rows, cells), status = (entries out of range, repeated)
__global__ void __launch_bounds__(1024) k_select_scan(const int* __restrict__ len, const int* __restrict__ cells,
                                                      const int* __restrict__ oor, const int* __restrict__ rep, int tracks,
                                                      int32_t* __restrict__ out_track_ptr, int32_t* __restrict__ totals,
                                                      int32_t* __restrict__ status) {
  const int* const a[4] = {len, cells, oor, rep};
  const BlockScan<4> sc(a, tracks);
  int pre = sc.pre[0];
  for (int i = sc.lo; i < sc.hi; ++i) {
    out_track_ptr[i] = pre;
    pre += len[i];
  }
  if (threadIdx.x == 0) {
    out_track_ptr[tracks] = sc.total[0];
    totals[0] = sc.total[0];
    totals[1] = sc.total[1];
    status[0] = sc.total[2];
    status[1] = sc.total[3];
  }
}

// a wave per chosen track: its rows, unchanged, to out_track_ptr[u]; nothing at or beyond row `capacity`
__global__ void __launch_bounds__(256) k_select_copy(const int32_t* __restrict__ notes, const int32_t* __restrict__ track_ptr,
                                                     int M, const int32_t* __restrict__ index, const int* __restrict__ len,
                                                     const int32_t* __restrict__ out_track_ptr, int32_t* __restrict__ out_notes,
                                                     int64_t capacity) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6, j = blockIdx.x;
  const int64_t u = 4 * (int64_t)j + k;
  const int n = len[u];
  if (n <= 0) return;                                                           // (index[j] is in [0, B) from here on)
  const TrackRange r(track_ptr, 4 * (int64_t)index[j] + k, M);                  // n = r.hi - r.lo
  const int64_t dst = out_track_ptr[u];
  if (dst < 0) return;                                                          // (a sum beyond int32: only on a bad track_ptr)
  const int64_t words = 3 * min((int64_t)n, max(capacity - dst, (int64_t)0));   // rows dst .. below min(dst + n, capacity)
  const int32_t* src = notes + 3 * (int64_t)r.lo;
  for (int64_t x = lane; x < words; x += 64) out_notes[3 * dst + x] = src[x];
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

extern "C" int pm_note_stats(const int32_t* notes, const int32_t* track_ptr, int32_t B, int32_t n_bars, int64_t M,
                             int32_t* track, int32_t* pitch_class, int32_t* onsets, int32_t* sounding, pm_stream_t stream) {
  if ((!notes && M > 0) || !track_ptr || !track || !pitch_class || !onsets || !sounding || B <= 0 || n_bars < 1 ||
      n_bars > MAX_BARS || M < 0)
    return PM_E_INVALID;
  const int64_t tracks = 4 * (int64_t)B;
  if (M > 0x7fffffffLL / 3 || tracks * n_bars > 0x7fffffffLL || tracks * N_STAT > 0x7fffffffLL) return PM_E_INVALID;
  const Buf buf[6] = {{notes, 3 * M, false}, {track_ptr, tracks + 1, false}, {track, tracks * N_STAT, true},
                      {pitch_class, tracks * N_PC, true}, {onsets, tracks * n_bars, true}, {sounding, tracks * n_bars, true}};
  if (misaligned(buf, 6) || clash(buf, 6)) return PM_E_INVALID;
  const size_t lds = 4 * 2 * 32 * (size_t)n_bars * sizeof(int);                 // at most 64 KB
  hipLaunchKernelGGL(k_note_stats, dim3(B), dim3(256), lds, (hipStream_t)stream, notes, track_ptr, n_bars, (int)M, track,
                     pitch_class, onsets, sounding);
  return pm_check_launch();
}

extern "C" int pm_note_chroma(const int32_t* notes, const int32_t* track_ptr, int32_t B, int64_t M, int32_t n_bars,
                              int32_t seg_steps, int32_t* chroma, pm_stream_t stream) {
  if ((!notes && M > 0) || !track_ptr || !chroma || B <= 0 || n_bars < 1 || n_bars > MAX_BARS || M < 0) return PM_E_INVALID;
  if (seg_steps < 1 || seg_steps > 32 || (seg_steps & (seg_steps - 1)) != 0) return PM_E_INVALID;
  const int64_t tracks = 4 * (int64_t)B, words = tracks * (32 * n_bars / seg_steps) * N_PC;
  if (M > 0x7fffffffLL / 3 || words > 0x7fffffffLL) return PM_E_INVALID;
  const Buf buf[3] = {{notes, 3 * M, false}, {track_ptr, tracks + 1, false}, {chroma, words, true}};
  if (misaligned(buf, 3) || clash(buf, 3)) return PM_E_INVALID;
  const int chunk_bars = n_bars < CHROMA_BARS ? n_bars : CHROMA_BARS;
  const size_t lds = (size_t)N_PC * 32 * chunk_bars * sizeof(int);              // at most 24 KB
  hipLaunchKernelGGL(k_note_chroma, dim3((unsigned)tracks, (unsigned)pm_cdiv(n_bars, CHROMA_BARS)), dim3(256), lds,
                     (hipStream_t)stream, notes, track_ptr, n_bars, (int)M, seg_steps, chroma);
  return pm_check_launch();
}

extern "C" int pm_notes_select(const int32_t* notes, const int32_t* track_ptr, int32_t B, int64_t M, const int32_t* index,
                               int32_t K, int32_t* out_notes, int64_t capacity, int32_t* out_track_ptr, int32_t* out_totals,
                               int32_t* scratch, int32_t* status, pm_stream_t stream) {
  if ((!notes && M > 0) || !track_ptr || !index || (!out_notes && capacity > 0) || !out_track_ptr || !out_totals || !scratch ||
      !status || B <= 0 || K < 1 || M < 0 || capacity < 0)
    return PM_E_INVALID;
  const int64_t tracks = 4 * (int64_t)K;
  if (M > 0x7fffffffLL / 3 || capacity > 0x7fffffffLL / 3 || 4 * (int64_t)B + 1 > 0x7fffffffLL ||
      PM_SELECT_SCRATCH(B, K) > 0x7fffffffLL)
    return PM_E_INVALID;
  const Buf buf[8] = {{notes, 3 * M, false}, {track_ptr, 4 * (int64_t)B + 1, false}, {index, K, false},
                      {out_notes, 3 * capacity, true}, {out_track_ptr, tracks + 1, true}, {out_totals, 2, true},
                      {scratch, PM_SELECT_SCRATCH(B, K), true}, {status, 2, true}};
  if (misaligned(buf, 8) || clash(buf, 8)) return PM_E_INVALID;
  int32_t *first = scratch, *len = scratch + B, *cells = len + tracks, *oor = cells + tracks, *rep = oor + tracks;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_select_init, dim3(pm_cdiv(B, 256)), dim3(256), 0, st, first, B);
  hipLaunchKernelGGL(k_select_mark, dim3(pm_cdiv(K, 256)), dim3(256), 0, st, index, K, B, first);
  hipLaunchKernelGGL(k_select_len, dim3(K), dim3(256), 0, st, notes, track_ptr, B, (int)M, index, first, len, cells, oor, rep);
  hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(1024), 0, st, len, cells, oor, rep, (int)tracks, out_track_ptr, out_totals,
                     status);
  hipLaunchKernelGGL(k_select_copy, dim3(K), dim3(256), 0, st, notes, track_ptr, (int)M, index, len, out_track_ptr, out_notes,
                     capacity);
  return pm_check_launch();
}

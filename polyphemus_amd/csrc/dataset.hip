// dataset.hip — a whole data set resident on the device in compact form, and batches gathered from it by index
// ("Resident data set" in include/polyphemus_hip.h).
//
// The reference's `PolyphemusDataset.__getitem__` (data.py:218-233) opens one `.npz` per sample and re-lays its dense token
// grid out bar by bar on the host, for every batch of every epoch; its random transposition is baked into the files once
// (preprocess.py:196-205).  Here the samples are packed once:
//   s_bits   uint32 [n, n_bars, 4]   bit t of word (bar, track): the cell is active; a bar without a cell has [0,0] (data.py:148-153)
//   rows     uint8  [R, 16, 2]       (pitch id, duration id) of the active cells, in node order (sample, bar, track, step)
//   cell_ptr int64  [n + 1]          the rows of sample i are rows[cell_ptr[i] : cell_ptr[i + 1]]
// and a batch is ONE launch (k_gather): a workgroup per batch entry expands the masks to the fp32 structure tensor and widens
// the byte rows to int32 token rows at out_ptr[j], transposing the pitches of tracks 1..3 on the way.  The output offsets are
// the caller's (host arithmetic on per-sample counts), so there is no device scan and nothing to read back; the only atomics
// are the status counters of entries that were not followed.
//   layout   per workgroup the n_bars * 4 masks and the inclusive prefix of their popcounts sit in LDS; output row r finds its
//            (bar, track) word by a binary search in the prefix.  8 lanes per output row, 16 B per lane: a 128-byte row is one
//            contiguous store of 8 lanes, its source 4 B per lane.  The structure goes out as one float4 per lane.
#include "bars.h"

namespace {

constexpr int MAX_DS_BARS = 64, MAX_WORDS = 4 * MAX_DS_BARS;
constexpr int N_PITCH = 131, N_DUR = 99, MAX_PITCH = 127;

__device__ inline int half_max(int v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 32));
  return v;
}

// The masks of a sample in LDS and the inclusive prefix of their popcounts; returns the cells of the sample.  W = n_bars * 4
// <= MAX_WORDS <= blockDim.x.  Every thread of the block calls it.
__device__ inline int stage_masks(const uint32_t* __restrict__ words, int W, uint32_t* msk, int* inc) {
  const int tid = threadIdx.x;
  if (tid < W) msk[tid] = words[tid];
  __syncthreads();
  if (tid < W) {
    int acc = 0;
    for (int q = 0; q <= tid; ++q) acc += __popc(msk[q]);
    inc[tid] = acc;
  }
  __syncthreads();
  return inc[W - 1];
}

// the word (bar * 4 + track) that holds row r of the sample: the first with inc > r; 0 <= r < inc[W - 1]
__device__ inline int word_of(const int* inc, int W, int r) {
  int lo = 0, hi = W - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (inc[mid] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// A workgroup per sample, a half-wave per bar (8 bars per pass): the masks with the empty-bar rule, the cells, the last live
// token slot (a non-PAD pitch or duration in slots 1..15 of an active cell) and the token ids outside their ranges.
__global__ void __launch_bounds__(256) k_pack_count(const int16_t* __restrict__ tok, const uint8_t* __restrict__ s, int n_bars,
                                                    uint32_t* __restrict__ s_bits, int32_t* __restrict__ cells,
                                                    int32_t* __restrict__ last_slot, int32_t* __restrict__ status) {
  __shared__ int sh[3];
  const int tid = threadIdx.x, hw = tid >> 5, t = tid & 31, half = (tid & 63) >> 5;
  const int64_t i = blockIdx.x;
  if (tid < 3) sh[tid] = 0;
  __syncthreads();
  int n_cells = 0, last = 0, bad = 0;
  for (int b0 = 0; b0 < n_bars; b0 += 8) {                                      // block-uniform: every lane reaches the ballots
    const int b = b0 + hw;
    const bool valid = b < n_bars;
    const int64_t g = i * n_bars + (valid ? b : 0);
    uint32_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = (uint32_t)(__ballot(valid && s[(g * 4 + k) * 32 + t] != 0) >> (32 * half));
    if ((m[0] | m[1] | m[2] | m[3]) == 0u) m[0] = 1u;                           // data.py:152-153
    if (valid && t < 4) s_bits[g * 4 + t] = t == 0 ? m[0] : t == 1 ? m[1] : t == 2 ? m[2] : m[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!valid || !((m[k] >> t) & 1u)) continue;
      ++n_cells;
      const uint4* row = reinterpret_cast<const uint4*>(tok + ((g * 4 + k) * 32 + t) * 32);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 v = row[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                           // slot 4 q + j
          const int pitch = (int16_t)(w[j] & 0xffffu), dur = (int16_t)(w[j] >> 16);
          bad += (pitch < 0 || pitch >= N_PITCH) + (dur < 0 || dur >= N_DUR);
          if (4 * q + j >= 1 && (pitch != PITCH_PAD || dur != DUR_PAD)) last = max(last, 4 * q + j);   // (a lane holds up to four cells)
        }
      }
    }
  }
  n_cells = half_sum(n_cells);
  bad = half_sum(bad);
  last = half_max(last);
  if (t == 0) {
    atomicAdd(&sh[0], n_cells);
    atomicMax(&sh[1], last);
    atomicAdd(&sh[2], bad);
  }
  __syncthreads();
  if (tid == 0) {
    cells[i] = sh[0];
    last_slot[i] = sh[1];
    if (sh[2]) atomicAdd(status, sh[2]);
  }
}

__device__ inline uint32_t narrow2(uint32_t w) { return (w & 0xffu) | ((w >> 8) & 0xff00u); }   // two int16 -> two bytes

// A workgroup per sample, a thread per cell: the byte rows of the active cells at rows[row_base + cell_off[i] + r]; nothing
// at or beyond row R, nothing beyond the sample's span of cell_off.
__global__ void __launch_bounds__(256) k_pack_rows(const int16_t* __restrict__ tok, const uint32_t* __restrict__ s_bits,
                                                   const int64_t* __restrict__ cell_off, int n_bars, uint8_t* __restrict__ rows,
                                                   int64_t row_base, int64_t R) {
  __shared__ uint32_t msk[MAX_WORDS];
  __shared__ int inc[MAX_WORDS];
  const int64_t i = blockIdx.x;
  const int W = 4 * n_bars;
  stage_masks(s_bits + i * W, W, msk, inc);
  const int64_t off = cell_off[i], span = cell_off[i + 1] - off, base = row_base + off;
  if (off < 0 || span <= 0) return;
  for (int c = threadIdx.x; c < 32 * W; c += 256) {
    const int mk = c >> 5, t = c & 31;
    const uint32_t m = msk[mk];
    if (!((m >> t) & 1u)) continue;
    const int64_t r = inc[mk] - __popc(m) + __popc(m & ((1u << t) - 1u));
    if (r >= span || base + r >= R) continue;                                   // 0 <= base + r < R
    const uint4* src = reinterpret_cast<const uint4*>(tok + (i * 32 * W + c) * 32);
    const uint4 a = src[0], b = src[1], e = src[2], f = src[3];
    uint4* dst = reinterpret_cast<uint4*>(rows + (base + r) * 32);
    dst[0] = make_uint4(narrow2(a.x) | (narrow2(a.y) << 16), narrow2(a.z) | (narrow2(a.w) << 16),
                        narrow2(b.x) | (narrow2(b.y) << 16), narrow2(b.z) | (narrow2(b.w) << 16));
    dst[1] = make_uint4(narrow2(e.x) | (narrow2(e.y) << 16), narrow2(e.z) | (narrow2(e.w) << 16),
                        narrow2(f.x) | (narrow2(f.y) << 16), narrow2(f.z) | (narrow2(f.w) << 16));
  }
}

// preprocess.py:196-205 on a pitch id: SOS, EOS and PAD (ids above 127) stay, the rest is shifted and clipped to 0..127
__device__ inline int shifted(int pitch, int sh) { return pitch > MAX_PITCH ? pitch : min(max(pitch + sh, 0), MAX_PITCH); }

// A workgroup per batch entry j.  The entry is followed iff 0 <= index[j] < n and the span of out_ptr equals the sample's
// stored cells and the cells of its masks, inside [0, N] and [0, R]; any other is counted and writes a structure of zeros and
// no row.  Every row store is below out_ptr[j + 1] <= N, every row load below cell_ptr[i + 1] <= R.
__global__ void __launch_bounds__(256) k_gather(const uint32_t* __restrict__ s_bits, const uint8_t* __restrict__ rows,
                                                const int64_t* __restrict__ cell_ptr, int64_t n, int n_bars, int64_t R,
                                                const int32_t* __restrict__ index, const int32_t* __restrict__ out_ptr,
                                                const int32_t* __restrict__ transpose, int64_t N, float* __restrict__ s_tensor,
                                                int32_t* __restrict__ tokens, int32_t* __restrict__ status) {
  __shared__ uint32_t msk[MAX_WORDS];
  __shared__ int inc[MAX_WORDS];
  const int tid = threadIdx.x, W = 4 * n_bars;
  const int64_t j = blockIdx.x, i = index[j];
  float4* s_out = reinterpret_cast<float4*>(s_tensor + j * 32 * W);
  const bool in_range = i >= 0 && i < n;                                        // block-uniform
  int why = in_range ? -1 : 0;
  int64_t o0 = 0, c0 = 0, span = 0;
  if (in_range) {
    o0 = out_ptr[j];
    c0 = cell_ptr[i];
    span = (int64_t)out_ptr[j + 1] - o0;
    const int64_t c1 = cell_ptr[i + 1];
    const int total = stage_masks(s_bits + i * W, W, msk, inc);
    if (o0 < 0 || span < 0 || o0 + span > N || c0 < 0 || c1 > R || c1 - c0 != span || total != span) why = 1;
  }
  if (why >= 0) {
    if (tid == 0) atomicAdd(status + why, 1);
    for (int q = tid; q < 8 * W; q += 256) s_out[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  for (int q = tid; q < 8 * W; q += 256) {                                      // four cells per lane
    const uint32_t b = msk[q >> 3] >> (4 * (q & 7));
    s_out[q] = make_float4((float)(b & 1u), (float)((b >> 1) & 1u), (float)((b >> 2) & 1u), (float)((b >> 3) & 1u));
  }
  const int sh = transpose ? min(max(transpose[j], -128), 128) : 0, sub = tid & 7;   // (beyond +-127 every pitch is clipped)
  const uint32_t* src = reinterpret_cast<const uint32_t*>(rows + c0 * 32);
  int4* dst = reinterpret_cast<int4*>(tokens + o0 * 32);
  for (int r = tid >> 3; r < (int)span; r += 32) {                              // span <= 128 n_bars
    const uint32_t w = src[r * 8 + sub];
    int p0 = (int)(w & 0xffu), p1 = (int)((w >> 16) & 0xffu);
    if (sh != 0 && (word_of(inc, W, r) & 3) != 0) {                             // never the drums
      p0 = shifted(p0, sh);
      p1 = shifted(p1, sh);
    }
    dst[r * 8 + sub] = make_int4(p0, (int)((w >> 8) & 0xffu), p1, (int)(w >> 24));
  }
}

struct Buf { const void* p; int64_t bytes; int align; bool written; };

// a buffer that is written may share no byte with any other; two that are only read may
inline bool clash(const Buf* b, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      if (!(b[i].written || b[j].written) || !b[i].p || !b[j].p || b[i].bytes <= 0 || b[j].bytes <= 0) continue;
      const uintptr_t pi = (uintptr_t)b[i].p, pj = (uintptr_t)b[j].p;
      if (pi < pj + (uintptr_t)b[j].bytes && pj < pi + (uintptr_t)b[i].bytes) return true;
    }
  return false;
}

inline bool misaligned(const Buf* b, int n) {
  for (int i = 0; i < n; ++i)
    if ((uintptr_t)b[i].p & (uintptr_t)(b[i].align - 1)) return true;
  return false;
}

constexpr int64_t LIM32 = 0x7fffffffLL, LIM_ROWS = 1LL << 40;

}  // namespace

extern "C" int pm_dataset_pack_count(const int16_t* token_grid, const uint8_t* s_grid, int64_t n, int32_t n_bars,
                                     uint32_t* s_bits, int32_t* cells, int32_t* last_slot, int32_t* status,
                                     pm_stream_t stream) {
  if (!token_grid || !s_grid || !s_bits || !cells || !last_slot || !status || n < 1 || n_bars < 1 || n_bars > MAX_DS_BARS)
    return PM_E_INVALID;
  if (n > LIM32 / (128 * (int64_t)n_bars)) return PM_E_INVALID;
  const int64_t bars = n * n_bars;
  const Buf buf[6] = {{token_grid, bars * 128 * 64, 16, false}, {s_grid, bars * 128, 1, false}, {s_bits, bars * 16, 4, true},
                      {cells, n * 4, 4, true}, {last_slot, n * 4, 4, true}, {status, 4, 4, true}};
  if (misaligned(buf, 6) || clash(buf, 6)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_pack_count, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, token_grid, s_grid, n_bars, s_bits,
                     cells, last_slot, status);
  return pm_check_launch();
}

extern "C" int pm_dataset_pack_rows(const int16_t* token_grid, const uint32_t* s_bits, const int64_t* cell_off, int64_t n,
                                    int32_t n_bars, uint8_t* rows, int64_t row_base, int64_t R, pm_stream_t stream) {
  if (!token_grid || !s_bits || !cell_off || !rows || n < 1 || n_bars < 1 || n_bars > MAX_DS_BARS || row_base < 0 || R < 1 ||
      R > LIM_ROWS || row_base >= R)
    return PM_E_INVALID;
  if (n > LIM32 / (128 * (int64_t)n_bars)) return PM_E_INVALID;
  const int64_t bars = n * n_bars;
  const Buf buf[4] = {{token_grid, bars * 128 * 64, 16, false}, {s_bits, bars * 16, 4, false}, {cell_off, (n + 1) * 8, 8, false},
                      {rows, R * 32, 16, true}};
  if (misaligned(buf, 4) || clash(buf, 4)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, token_grid, s_bits, cell_off, n_bars,
                     rows, row_base, R);
  return pm_check_launch();
}

extern "C" int pm_dataset_gather(const uint32_t* s_bits, const uint8_t* rows, const int64_t* cell_ptr, int64_t n,
                                 int32_t n_bars, int64_t R, const int32_t* index, const int32_t* out_ptr,
                                 const int32_t* transpose, int32_t B, int64_t N, float* s_tensor, int32_t* tokens,
                                 int32_t* status, pm_stream_t stream) {
  if (!s_bits || !rows || !cell_ptr || !index || !out_ptr || !s_tensor || !tokens || !status || n < 1 || n > LIM32 ||
      n_bars < 1 || n_bars > MAX_DS_BARS || R < 1 || R > LIM_ROWS || B < 1 || N < 1 || N > LIM32)
    return PM_E_INVALID;
  if (B > LIM32 / (128 * (int64_t)n_bars) || N > 128 * (int64_t)n_bars * B) return PM_E_INVALID;
  const Buf buf[9] = {{s_bits, n * n_bars * 16, 4, false}, {rows, R * 32, 16, false}, {cell_ptr, (n + 1) * 8, 8, false},
                      {index, (int64_t)B * 4, 4, false}, {out_ptr, ((int64_t)B + 1) * 4, 4, false},
                      {transpose, (int64_t)B * 4, 4, false}, {s_tensor, (int64_t)B * n_bars * 512, 16, true},
                      {tokens, N * 128, 16, true}, {status, 8, 4, true}};
  if (misaligned(buf, 9) || clash(buf, 9)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_gather, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, s_bits, rows, cell_ptr, n, n_bars, R, index,
                     out_ptr, transpose, N, s_tensor, tokens, status);
  return pm_check_launch();
}

// infill.hip — regenerate chosen tracks, bars and steps of a piece around the notes that are kept (pm_infill_structure,
// pm_infill_tokens).  A region mask [R,4,32] in the cell layout of a structure tensor says which cells the model rewrites;
// bar g reads region row g % R (R = G: a mask per piece and bar; R = n_bars: one mask for every piece).
//
//   structure : a cell is on iff (region ? s_model : s_in); a bar that comes out empty gets cell [0,0] (data.py:152-153, the
//               rule of pm_tokens_from_notes and pm_graph_count), inside the region or not, and bar_forced[g] = 1.  One launch, a
//               bar per half-wave (HalfBar of bars.h), every input read once, every output written once.
//   tokens    : both structures are numbered by BarLanes (a bar per wave), pm_bar_node_ptr once for each.  A node of the merged
//               structure inside the region keeps its drawn row; one outside takes the 15 slots behind the SOS of the input's
//               node of the same cell, or, where the input has no such node (the forced [0,0]; a node at or beyond N_in), the
//               chord of a cell without a note (preprocess.py:118-157): (EOS, EOS), then (PAD, PAD).
//   status    : {active cells of s_out, active cells of s_in, kept nodes, kept nodes without a source, bars forced}, from
//               per-bar counts in scratch summed by one wave.
// A row of `tokens` is 15 pairs = 120 bytes: rows are 8-byte aligned, not 16, and so is the source behind a 128-byte input
// row's SOS pair (byte 8).  k_infill_tokens therefore moves a row as fifteen 8-byte words.
// No atomics and no LDS outside the scan of pm_bar_node_ptr: every byte written is a function of the inputs.
#include "bars.h"

namespace {

constexpr int ROW = PM_N_SLOTS;                                                 // 15 token pairs per node of `tokens`
constexpr int ROW_IN = PM_N_SLOTS + 1;                                          // 16 per node of `tokens_in` (slot 0 = SOS)

__global__ void __launch_bounds__(256) k_infill_structure(const float* __restrict__ s_in, const uint8_t* __restrict__ s_model,
                                                          const uint8_t* __restrict__ region, int G, int R,
                                                          float* __restrict__ s_f32, uint8_t* __restrict__ s_u8,
                                                          int* __restrict__ bar_forced) {
  const HalfBar h(G);
  const int64_t r0 = h.valid ? (h.g % R) * 128 + h.t : 0;                       // region cell of track 0: < 128 R
  bool on[4];
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    on[k] = h.valid && (region[r0 + 32 * k] != 0 ? s_model[h.cell(k)] != 0 : s_in[h.cell(k)] != 0.f);
    any |= h.ballot(on[k]);
  }
  if (!h.valid) return;
  if (h.t == 0) {
    if (any == 0u) on[0] = true;                                                // data.py:152-153
    bar_forced[h.g] = any == 0u ? 1 : 0;
  }
  h.store(on, s_f32, s_u8);
}

// the row of a kept node: fifteen 8-byte loads behind the source's SOS pair, then fifteen 8-byte stores; without a source
// (src == nullptr) the chord of a cell without a note
__device__ inline void keep_node(int32_t* __restrict__ tokens, int64_t n, const int32_t* __restrict__ src) {
  int2 tk[ROW];
#pragma unroll
  for (int j = 0; j < ROW; ++j) {
    tk[j] = j == 0 ? make_int2(PITCH_EOS, DUR_EOS) : make_int2(PITCH_PAD, DUR_PAD);
    if (src) tk[j] = reinterpret_cast<const int2*>(src)[j + 1];
  }
  int2* dst = reinterpret_cast<int2*>(tokens + n * (2 * ROW));
#pragma unroll
  for (int j = 0; j < ROW; ++j) dst[j] = tk[j];
}

// one bar per wave: the rows of the bar's kept nodes; nothing read at or beyond node N_in, nothing written at or beyond N
__global__ void __launch_bounds__(256) k_infill_tokens(const float* __restrict__ s_in, const float* __restrict__ s_out,
                                                       const uint8_t* __restrict__ region, const int* __restrict__ ptr_in,
                                                       const int* __restrict__ ptr_out, int G, int R,
                                                       const int32_t* __restrict__ tokens_in, int64_t N_in,
                                                       int32_t* __restrict__ tokens, int64_t N, int* __restrict__ bar_kept,
                                                       int* __restrict__ bar_lost) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;                                                           // wave-uniform
  const BarLanes out(s_out, ptr_out, g, lane, N), in(s_in, ptr_in, g, lane, N_in);
  const uint8_t* reg = region + (int64_t)(g % R) * 128;
  const bool keep0 = out.on0 && reg[lane] == 0, keep1 = out.on1 && reg[64 + lane] == 0;
  if (keep0) keep_node(tokens, out.n0, in.on0 ? tokens_in + in.n0 * (2 * ROW_IN) : nullptr);
  if (keep1) keep_node(tokens, out.n1, in.on1 ? tokens_in + in.n1 * (2 * ROW_IN) : nullptr);
  const int kept = __popcll(__ballot(keep0)) + __popcll(__ballot(keep1));
  const int lost = __popcll(__ballot(keep0 && !in.on0)) + __popcll(__ballot(keep1 && !in.on1));
  if (lane == 0) {
    bar_kept[g] = kept;
    bar_lost[g] = lost;
  }
}

// one wave: status = {cells of s_out, cells of s_in, kept nodes, kept nodes without a source, bars forced}
__global__ void __launch_bounds__(64) k_infill_status(const int* __restrict__ ptr_in, const int* __restrict__ ptr_out,
                                                      const int* __restrict__ bar_kept, const int* __restrict__ bar_lost,
                                                      const int* __restrict__ bar_forced, int G, int* __restrict__ status) {
  const int lane = threadIdx.x;
  int kept = 0, lost = 0, forced = 0;
  for (int g = lane; g < G; g += 64) {
    kept += bar_kept[g];
    lost += bar_lost[g];
    if (bar_forced) forced += bar_forced[g] != 0 ? 1 : 0;
  }
  kept = half_sum(kept); kept += __shfl_xor(kept, 32, 64);
  lost = half_sum(lost); lost += __shfl_xor(lost, 32, 64);
  forced = half_sum(forced); forced += __shfl_xor(forced, 32, 64);
  if (lane == 0) {
    status[0] = ptr_out[G];
    status[1] = ptr_in[G];
    status[2] = kept;
    status[3] = lost;
    status[4] = forced;
  }
}

struct Buf { const void* p; int64_t bytes; bool written; };

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

inline bool bad_bars(int32_t G, int32_t R) { return G <= 0 || R <= 0 || G % R != 0 || (int64_t)G * 128 > 0x7fffffffLL; }

}  // namespace

extern "C" int pm_infill_structure(const float* s_in, const uint8_t* s_model, const uint8_t* region, int32_t G, int32_t R,
                                   float* s_f32, uint8_t* s_u8, int32_t* bar_forced, pm_stream_t stream) {
  if (!s_in || !s_model || !region || (!s_f32 && !s_u8) || !bar_forced || bad_bars(G, R)) return PM_E_INVALID;
  if (((uintptr_t)s_in | (uintptr_t)s_f32 | (uintptr_t)bar_forced) & 3) return PM_E_INVALID;
  const int64_t cells = 128 * (int64_t)G;
  const Buf buf[6] = {{s_in, 4 * cells, false}, {s_model, cells, false}, {region, 128 * (int64_t)R, false},
                      {s_f32, 4 * cells, true}, {s_u8, cells, true}, {bar_forced, 4 * (int64_t)G, true}};
  if (clash(buf, 6)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_infill_structure, dim3(pm_cdiv(G, 8)), dim3(256), 0, (hipStream_t)stream, s_in, s_model, region, G, R,
                     s_f32, s_u8, bar_forced);
  return pm_check_launch();
}

extern "C" int pm_infill_tokens(const float* s_in, const float* s_out, const uint8_t* region, int32_t G, int32_t R,
                                const int32_t* tokens_in, int64_t N_in, int32_t* tokens, int64_t N, const int32_t* bar_forced,
                                int32_t* scratch, int32_t* status, pm_stream_t stream) {
  if (!s_in || !s_out || !region || !scratch || !status || bad_bars(G, R) || N < 0 || N_in < 0 || (!tokens_in && N_in > 0) ||
      (!tokens && N > 0))
    return PM_E_INVALID;
  if (N > 0x7fffffffLL / (2 * ROW) || N_in > 0x7fffffffLL / (2 * ROW_IN)) return PM_E_INVALID;
  if (((uintptr_t)s_in | (uintptr_t)s_out | (uintptr_t)bar_forced | (uintptr_t)scratch | (uintptr_t)status) & 3)
    return PM_E_INVALID;
  if (((uintptr_t)tokens & 7) || ((uintptr_t)tokens_in & 15)) return PM_E_INVALID;    // rows of 120 B, rows of 128 B
  const int64_t cells = 128 * (int64_t)G;
  const Buf buf[8] = {{s_in, 4 * cells, false}, {s_out, 4 * cells, false}, {region, 128 * (int64_t)R, false},
                      {tokens_in, 8 * ROW_IN * N_in, false}, {bar_forced, 4 * (int64_t)G, false}, {tokens, 8 * ROW * N, true},
                      {scratch, 4 * PM_INFILL_SCRATCH(G), true}, {status, 4 * 5, true}};
  if (clash(buf, 8)) return PM_E_INVALID;
  int32_t *nodes_in = scratch, *ptr_in = scratch + G, *nodes_out = scratch + 2 * (int64_t)G + 1;
  int32_t *ptr_out = scratch + 3 * (int64_t)G + 1, *bar_kept = scratch + 4 * (int64_t)G + 2, *bar_lost = scratch + 5 * (int64_t)G + 2;
  hipStream_t st = (hipStream_t)stream;
  if (pm_bar_node_ptr(st, s_in, G, nodes_in, ptr_in) != PM_OK || pm_bar_node_ptr(st, s_out, G, nodes_out, ptr_out) != PM_OK)
    return PM_E_INVALID;
  hipLaunchKernelGGL(k_infill_tokens, dim3(pm_cdiv(G, 4)), dim3(256), 0, st, s_in, s_out, region, ptr_in, ptr_out, G, R, tokens_in,
                     N_in, tokens, N, bar_kept, bar_lost);
  hipLaunchKernelGGL(k_infill_status, dim3(1), dim3(64), 0, st, ptr_in, ptr_out, bar_kept, bar_lost, bar_forced, G, status);
  return pm_check_launch();
}

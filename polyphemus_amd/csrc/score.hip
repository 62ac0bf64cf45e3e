// score.hip — what the decoder thinks of a piece ("Scores", include/polyphemus_hip.h): the log-likelihood of the piece's own
// tokens and structure under the decoder's logits, per bar and track, with the counts behind the reference's accuracies.
// The terms are those of PolyphemusTrainer._losses (training.py:298-347: cross-entropy with ignore_index = PAD on both heads,
// BCE with logits on the structure) and of its accuracies (training.py:438-468 and 470-497), kept apart per (bar, track)
// instead of averaged over the batch.
//
//   k_score_rows      : one wave per (node, slot) row.  The row's 8-byte target pair is read first; a row whose targets are
//                       both PAD (most of the 15 slots of a real batch) writes its zeros and never touches its 920 B of
//                       logits.  Otherwise the row is held as in sample.hip (load_row of heads.h) and every head with a target
//                       gives logp = (x_t - m) - log sum exp(x - m) in fp32, m the head's max, and whether the head's arg-max
//                       (head_argmax: first index on ties, the rule of k_content_accuracy) is the target.  8 B of row_logp and
//                       one verdict byte per row.
//   k_score_bars      : a bar per wave (BarLanes of bars.h).  A lane sums the 15 rows of each of its (at most two) nodes in slot
//                       order in fp64; the lanes of a track are the 32 lanes of a half-wave, summed by a fixed shuffle tree in
//                       fp64.  135 B read per node, 160 B written per bar, every output word of every bar and track.
//   k_score_structure : a bar per half-wave (HalfBar): lane t holds the four cells of timestep t.  The Bernoulli terms in fp32,
//                       their 32-term sum per track in fp64 by the same tree; the counts are popcounts of ballots.  1 KB read
//                       and 96 B written per bar.
// No atomics and no LDS: two calls write the same bytes, and a bar's words depend on that bar's nodes alone.
#include "bars.h"
#include "heads.h"

namespace {

__device__ static inline float bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// verdict bits of a row
enum { V_PITCH_HIT = 1, V_DUR_HIT = 2, V_PITCH_SET = 4, V_DUR_SET = 8 };

// log softmax of column c (wave-uniform, inside the head) of the head whose columns this lane marks with in[j]
__device__ static inline float head_logp(const float (&v)[4], const bool (&in)[4], int c, int lane) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) m = fmaxf(m, in[j] ? v[j] : -INFINITY);
  m = pm_wave_max(m);
  float z = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) z += in[j] ? expf(v[j] - m) : 0.f;
  z = pm_wave_sum(z);
  const int reg = c >> 6;
  const float mine = reg == 0 ? v[0] : reg == 1 ? v[1] : reg == 2 ? v[2] : v[3];
  return __fsub_rn(__fsub_rn(bcast(mine, c & 63), m), logf(z));
}

// tokens [N, SLOTS, 2]: SLOTS = 16 has the SOS in slot 0, which is no target
__global__ void __launch_bounds__(256) k_score_rows(const float* __restrict__ c_logits, const int2* __restrict__ tokens,
                                                    int tok_slots, int64_t rows, float2* __restrict__ row_logp,
                                                    uint8_t* __restrict__ row_verdict) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                                        // wave-uniform
  const int64_t n = r / PM_N_SLOTS;
  const int slot = (int)(r - n * PM_N_SLOTS) + (tok_slots - PM_N_SLOTS);
  const int2 t = tokens[n * tok_slots + slot];
  const int tp = __builtin_amdgcn_readfirstlane(t.x), td = __builtin_amdgcn_readfirstlane(t.y);
  // a target outside its head (PAD is the head's last token) is no target
  const bool hp = (unsigned)tp < (unsigned)PITCH_PAD, hd = (unsigned)td < (unsigned)DUR_PAD;
  float2 lp = {0.f, 0.f};
  int verdict = 0;
  if (hp || hd) {                                                               // wave-uniform
    float v[4];
    load_row(c_logits + r * PM_N_TOK, lane, v);
    int ip, id;
    head_argmax(v, lane, ip, id);
    const bool p2 = lane < 3;                                                   // register 2: columns 128..130 are pitch
    if (hp) {
      const bool in[4] = {true, true, p2, false};
      lp.x = head_logp(v, in, tp, lane);
      verdict |= V_PITCH_SET | (ip == tp ? V_PITCH_HIT : 0);
    }
    if (hd) {
      const bool in[4] = {false, false, !p2, lane < PM_N_TOK - 192};
      lp.y = head_logp(v, in, PM_N_PITCH + td, lane);
      verdict |= V_DUR_SET | (id == td ? V_DUR_HIT : 0);
    }
  }
  if (lane == 0) {
    row_logp[r] = lp;
    row_verdict[r] = (uint8_t)verdict;
  }
}

// what a node adds to its (bar, track): the two sums in fp64 and the six counts
struct NodeSum { double lp, ld; int c[6]; };

__device__ static inline NodeSum node_sum(bool on, int64_t n, const float2* __restrict__ row_logp,
                                          const uint8_t* __restrict__ row_verdict) {
  NodeSum s = {0.0, 0.0, {0, 0, 0, 0, 0, 0}};
  if (!on) return s;
  s.c[0] = 1;
  const float2* lp = row_logp + n * PM_N_SLOTS;
  const uint8_t* vd = row_verdict + n * PM_N_SLOTS;
#pragma unroll
  for (int j = 0; j < PM_N_SLOTS; ++j) {                                        // slot order
    const float2 x = lp[j];
    const int b = vd[j];
    s.lp += (double)x.x;
    s.ld += (double)x.y;
    s.c[1] += (b & V_PITCH_SET) ? 1 : 0;
    s.c[2] += (b & V_DUR_SET) ? 1 : 0;
    s.c[3] += (b & V_PITCH_HIT) ? 1 : 0;
    s.c[4] += (b & V_DUR_HIT) ? 1 : 0;
    s.c[5] += (b & (V_PITCH_HIT | V_DUR_HIT)) == (V_PITCH_HIT | V_DUR_HIT) ? 1 : 0;   // (a hit implies its target)
  }
  return s;
}
// the sum over the 32 lanes of a half-wave, in every lane of it: one fixed tree
__device__ static inline double half_sum_d(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ static inline void half_reduce(NodeSum& s) {
  s.lp = half_sum_d(s.lp);
  s.ld = half_sum_d(s.ld);
#pragma unroll
  for (int k = 0; k < 6; ++k) s.c[k] = half_sum(s.c[k]);
}

__global__ void __launch_bounds__(256) k_score_bars(const float* __restrict__ s, const int* __restrict__ node_ptr, int G, int64_t N,
                                                    const float2* __restrict__ row_logp, const uint8_t* __restrict__ row_verdict,
                                                    double* __restrict__ logp, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;                                                           // wave-uniform
  const BarLanes bl(s, node_ptr, g, lane, N);
  // cell `lane` lies in track lane >> 5, cell 64 + lane in track 2 + (lane >> 5): a track is a half-wave of either
  NodeSum a = node_sum(bl.on0, bl.n0, row_logp, row_verdict), b = node_sum(bl.on1, bl.n1, row_logp, row_verdict);
  half_reduce(a);
  half_reduce(b);
  if ((lane & 31) == 0) {
    const int half = lane >> 5;
#pragma unroll
    for (int set = 0; set < 2; ++set) {
      const NodeSum& t = set ? b : a;
      const int64_t o = (int64_t)g * 4 + 2 * set + half;
      logp[o * 2] = t.lp;
      logp[o * 2 + 1] = t.ld;
#pragma unroll
      for (int k = 0; k < 6; ++k) counts[o * 6 + k] = t.c[k];
    }
  }
}

__global__ void __launch_bounds__(256) k_score_structure(const float* __restrict__ s_logits, const float* __restrict__ s_tensor,
                                                         int G, double* __restrict__ logp, int* __restrict__ counts) {
  const HalfBar h(G);
  double mine_lp = 0.0;                                                         // lane k < 4 of the half: track k
  int mine_c[4] = {0, 0, 0, 0};
  float x[4], y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                                 // eight loads in flight
    x[k] = h.valid ? s_logits[h.cell(k)] : 0.f;
    y[k] = h.valid ? s_tensor[h.cell(k)] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool on = y[k] != 0.f, pred = structure_pred(x[k]);
    // max(x, 0) - x y + log1p(exp(-|x|)): the first two terms are exact together
    const float term = __fadd_rn(on ? fmaxf(-x[k], 0.f) : fmaxf(x[k], 0.f), log1pf(expf(-fabsf(x[k]))));
    const double sum = half_sum_d((double)term);
    const int n_on = __popc(h.ballot(h.valid && on)), n_pred = __popc(h.ballot(h.valid && pred));
    const int n_tp = __popc(h.ballot(h.valid && on && pred)), n_eq = __popc(h.ballot(h.valid && on == pred));
    if (h.t == k) { mine_lp = -sum; mine_c[0] = n_on; mine_c[1] = n_pred; mine_c[2] = n_tp; mine_c[3] = n_eq; }
  }
  if (!h.valid || h.t >= 4) return;
  logp[h.g * 4 + h.t] = mine_lp;
#pragma unroll
  for (int k = 0; k < 4; ++k) counts[(h.g * 4 + h.t) * 4 + k] = mine_c[k];
}

static inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int pm_score_tokens(const float* c_logits, const int32_t* tokens, int32_t tok_slots, const float* s_tensor, int32_t G,
                               int64_t N, int32_t* bar_nodes, int32_t* node_ptr, float* row_logp, uint8_t* row_verdict,
                               double* logp, int32_t* counts, pm_stream_t stream) {
  if (!s_tensor || !bar_nodes || !node_ptr || !logp || !counts || G <= 0 || N < 0) return PM_E_INVALID;
  if (tok_slots != PM_N_SLOTS && tok_slots != PM_N_SLOTS + 1) return PM_E_INVALID;
  if (N > 0 && (!c_logits || !tokens || !row_logp || !row_verdict)) return PM_E_INVALID;
  if (N * PM_N_SLOTS >= ((int64_t)1 << 31) || bar_nodes == node_ptr || (int64_t)G * 128 > 0x7fffffffLL) return PM_E_INVALID;
  if (!aligned(c_logits, 4) || !aligned(tokens, 8) || !aligned(s_tensor, 4) || !aligned(bar_nodes, 4) || !aligned(node_ptr, 4) ||
      !aligned(row_logp, 8) || !aligned(logp, 8) || !aligned(counts, 4))
    return PM_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (pm_bar_node_ptr(st, s_tensor, G, bar_nodes, node_ptr) != PM_OK) return PM_E_INVALID;
  const int64_t rows = N * PM_N_SLOTS;
  if (rows > 0)
    hipLaunchKernelGGL(k_score_rows, dim3((unsigned)pm_cdiv(rows, 4)), dim3(256), 0, st, c_logits,
                       reinterpret_cast<const int2*>(tokens), tok_slots, rows, reinterpret_cast<float2*>(row_logp), row_verdict);
  hipLaunchKernelGGL(k_score_bars, dim3((unsigned)pm_cdiv(G, 4)), dim3(256), 0, st, s_tensor, node_ptr, G, N,
                     reinterpret_cast<const float2*>(row_logp), row_verdict, logp, counts);
  return pm_check_launch();
}

extern "C" int pm_score_structure(const float* s_logits, const float* s_tensor, int32_t G, double* logp, int32_t* counts,
                                  pm_stream_t stream) {
  if (!s_logits || !s_tensor || !logp || !counts || G <= 0 || (int64_t)G * 128 > 0x7fffffffLL) return PM_E_INVALID;
  if (!aligned(s_logits, 4) || !aligned(s_tensor, 4) || !aligned(logp, 8) || !aligned(counts, 4)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_score_structure, dim3((unsigned)pm_cdiv(G, 8)), dim3(256), 0, (hipStream_t)stream, s_logits, s_tensor, G,
                     logp, counts);
  return pm_check_launch();
}

// sample.hip — stochastic decoding on the device ("sampled generation", include/polyphemus_hip.h): temperature, top-k and
// nucleus (top-p) sampling of the pitch and the duration token of every (node, slot) row of the content logits, and sampling
// of the bar structure from the structure logits.
//
//   the core        : the row layout and the arg-max (load_row, cand_better, cand_wave: heads.h, shared with loss.hip and
//                     score.hip), the noise of the stream (seed, head, row, token) (unit_noise, gumbel) and head_filter, the
//                     top-k / top-p pass of one head of one row over a set of candidate columns.
//   k_sample_tokens : one wave per row of 230 logits (920 B, read once), 8 B of tokens written: both heads at once, every live
//                     column a candidate of its head's head_filter.
//   k_sample_chords : chord-aware sampling (PmChordRules): one wave per node, its 15 slots decided in order as notes, one EOS,
//                     then PAD, under per-track rules (note counts, a pitch mask, no pitch twice): draw_head draws each head
//                     among the candidates of the slot.
//                     CHART (pm_sample_chords_at): the node's cell replaces its track, and a chart of pitch-class sets
//                     per (bar, step) narrows the pitch mask of the tracks it binds: one 4-byte load and two % 12 per
//                     lane in front of the slot loop, nothing inside it.  pm_sample_chords launches CHART = false.
//   k_sample_structure : structure sampling (PmStructureRules): which of the 4 x 32 (track, timestep) cells of every bar are active,
//                     drawn from the structure logits under per-track rules (a bias, the least and the most active cells, the
//                     allowed timesteps).  A bar per half-wave (HalfBar of bars.h, as k_binary_from_logits): lane t of the half
//                     holds the four cells of timestep t, one per track, so a track's 32 cells lie across the 32 lanes of the
//                     half and a bar's logits are four coalesced 128-byte loads.  512 B read and 128 / 512 B (+ 16 B of counts)
//                     written per bar, each once.  The rank of a cell is an all-pairs count inside the half: every allowed
//                     timestep of the track is broadcast once (v_readlane of both halves, a select) and compared with the
//                     lane's own cell; no LDS, no atomics.  The rules are launch constants, so the allowed timesteps are a
//                     scalar loop over the bits of the mask, and a track whose bounds cannot bind (0 .. 32) skips the pass
//                     wave-uniformly.  NOISE = false (temperature 0) compiles the hash and the two logf away.  The lanes of a
//                     half without a bar (odd G, the last wave) take part in every cross-lane step and store nothing.
#include <type_traits>
#include "bars.h"
#include "heads.h"

namespace {

enum { SAMPLE_GREEDY = 0, SAMPLE_PLAIN = 1, SAMPLE_TOPK = 2, SAMPLE_TOPP = 3 };

__device__ static inline float bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// the uniform u in (0, 1) of (key, token): the header's u
__device__ static inline float unit_noise(uint32_t key, uint32_t token) {
  const uint32_t h = pm_group_hash(key, token);
  return ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f;                   // 2^-23: exact, inside (0, 1)
}
// Gumbel noise of (key, token): the header's g
__device__ static inline float gumbel(uint32_t key, uint32_t token) { return -logf(-logf(unit_noise(key, token))); }

// the logit as an unsigned word of the same order; -0 and +0 share one key (they are equal logits)
__device__ static inline unsigned ukey(float x) {
  const unsigned b = __float_as_uint(x + 0.0f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// ---- the sampling core.  The draw is a Gumbel arg-max (gumbel above, cand_better and cand_wave of heads.h), so no cumulative sum and no
// second random number per row, and head_filter is its one top-k / top-p pass.

// One head of one row.  NV registers per lane: v[j] = the logit of this lane's j-th column of the head, cand[j] whether it is a
// candidate, bal[j] = __ballot(cand[j]), live[j] (= cand[j] on entry) whether it stays in the draw.  An all-pairs pass whose
// sources are the candidates alone, taken in index order from the ballots (every one broadcast once with v_readlane and
// compared against the lane's own columns): it counts the candidates that outrank a column (top-k) and sums their softmax mass
// (top-p) in one go, exact under ties, with no LDS and no atomics.  A column that is no candidate takes no rank and adds no
// mass.  MODE 0 greedy and MODE 1 unfiltered have no pass.
template <int MODE, int NV>
__device__ static inline void head_filter(const float (&v)[NV], const bool (&cand)[NV], const unsigned long long (&bal)[NV],
                                          float inv_t, int top_k, float top_p, int lane, bool (&live)[NV]) {
  if (MODE != SAMPLE_TOPK && MODE != SAMPLE_TOPP) return;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) m = fmaxf(m, cand[j] ? v[j] : -INFINITY);
  m = pm_wave_max(m);
  float q[NV], mass[NV];
  unsigned key_[NV];
  int cnt[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    q[j] = cand[j] ? expf((v[j] - m) * inv_t) : 0.f;
    key_[j] = ukey(v[j]);
    cnt[j] = 0;
    mass[j] = 0.f;
  }
  // source (register s, lane l) outranks target (register j, this lane) iff key(source) > thr: the target's key when the
  // source comes later in index order, its key - 1 when it comes earlier (equal logits: the lower index outranks)
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    for (unsigned long long m_s = bal[s]; m_s; m_s &= m_s - 1) {
      const int l = (int)__builtin_ctzll(m_s);
      const unsigned sk = (unsigned)__builtin_amdgcn_readlane((int)key_[s], l);
      const float sq = MODE == SAMPLE_TOPP ? bcast(q[s], l) : 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const bool earlier = s < j || (s == j && l < lane);
        const bool o = sk > key_[j] - (earlier ? 1u : 0u);
        cnt[j] += o ? 1 : 0;
        if (MODE == SAMPLE_TOPP) mass[j] += o ? sq : 0.f;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) live[j] = live[j] && cnt[j] < top_k;
  if (MODE == SAMPLE_TOPP) {
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) z += live[j] ? q[j] : 0.f;
    z = pm_wave_sum(z);
    const float edge = top_p * z;
#pragma unroll
    for (int j = 0; j < NV; ++j) live[j] = live[j] && mass[j] < edge;
  }
}

// One wave per row, both heads at once, every live column a candidate: the head of a column is known per register except for
// register 2, where the lanes 0..2 end the pitch head and the lanes 3..63 begin the duration head.
template <int MODE>
__global__ void __launch_bounds__(256) k_sample_tokens(const float* __restrict__ c_logits, int64_t rows, float inv_t,
                                                       int top_k, float top_p, uint32_t seed, int* __restrict__ tokens) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                                        // wave-uniform
  const bool p2 = lane < 3;                                                     // register 2: columns 128..130 are pitch
  const bool live3 = lane < PM_N_TOK - 192;
  float v[4];
  load_row(c_logits + r * PM_N_TOK, lane, v);
  const int tok[4] = {lane, lane + 64, p2 ? lane + 128 : lane - 3, lane + 192 - PM_N_PITCH};

  bool live[4] = {true, true, true, live3};
  float score[4];
  if (MODE == SAMPLE_GREEDY) {
#pragma unroll
    for (int j = 0; j < 4; ++j) score[j] = v[j];
  } else {
    if (MODE != SAMPLE_PLAIN) {
      const float vp[3] = {v[0], v[1], v[2]}, vd[2] = {v[2], v[3]};
      const bool candp[3] = {true, true, p2}, candd[2] = {!p2, live3};
      const unsigned long long balp[3] = {~0ull, ~0ull, 7ull}, bald[2] = {~7ull, (1ull << (PM_N_TOK - 192)) - 1ull};
      bool livep[3] = {true, true, p2}, lived[2] = {!p2, live3};
      head_filter<MODE, 3>(vp, candp, balp, inv_t, top_k, top_p, lane, livep);
      head_filter<MODE, 2>(vd, candd, bald, inv_t, top_k, top_p, lane, lived);
      live[0] = livep[0]; live[1] = livep[1]; live[2] = p2 ? livep[2] : lived[0]; live[3] = lived[1];
    }
    const uint32_t kp = pm_edge_key(seed, 0u, (uint32_t)r), kd = pm_edge_key(seed, 1u, (uint32_t)r);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool pitch = j < 2 || (j == 2 && p2);
      score[j] = __fadd_rn(__fmul_rn(v[j], inv_t), gumbel(pitch ? kp : kd, (uint32_t)tok[j]));
    }
  }
  // arg-max per head over the surviving columns; a row that leaves none (non-finite logits) gives token 0
  Cand bp = {-INFINITY, 0}, bd = {-INFINITY, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool pitch = j < 2 || (j == 2 && p2);
    const Cand c = {live[j] ? score[j] : -INFINITY, live[j] ? tok[j] : 0x7fffffff};
    if (j < 2) bp = cand_better(bp, c);
    else if (j == 3) bd = cand_better(bd, c);
    else { if (pitch) bp = cand_better(bp, c); else bd = cand_better(bd, c); }
  }
  bp = cand_wave(bp); bd = cand_wave(bd);
  const int tp = min(max(bp.c, 0), PM_N_PITCH - 1), td = min(max(bd.c, 0), PM_N_DUR - 1);
  if (lane < 2) tokens[r * 2 + lane] = lane ? td : tp;
}

// ---- chord-aware sampling ("sampled generation", PmChordRules) -------------------------------------------------------
constexpr int N_DUR_CAND = 96;

// One head of one slot among its candidates (`greedy`: this head at temperature 0).  Returns a candidate whenever there is
// one: where no score wins (non-finite logits) the candidate of the lowest index.
template <int MODE, int NV>
__device__ static inline int draw_head(const float (&v)[NV], const int (&tok)[NV], const bool (&cand)[NV], bool greedy,
                                       float inv_t, int top_k, float top_p, uint32_t key, int lane) {
  unsigned long long bal[NV];
  int ncand = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j) { bal[j] = __ballot(cand[j]); ncand += __popcll(bal[j]); }
  // the candidate of the lowest index: register by register, lane by lane (tok grows that way in both heads)
  int first = 0;
#pragma unroll
  for (int j = NV - 1; j >= 0; --j)
    if (bal[j]) first = __builtin_amdgcn_readlane(tok[j], (int)__builtin_ctzll(bal[j]));
  if (ncand <= 1) return first;                                                 // (wave-uniform) no draw
  bool live[NV];
  float score[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) live[j] = cand[j];
  if (MODE == SAMPLE_GREEDY || greedy) {
#pragma unroll
    for (int j = 0; j < NV; ++j) score[j] = v[j];
  } else {
    head_filter<MODE, NV>(v, cand, bal, inv_t, top_k, top_p, lane, live);
#pragma unroll
    for (int j = 0; j < NV; ++j) score[j] = __fadd_rn(__fmul_rn(v[j], inv_t), gumbel(key, (uint32_t)tok[j]));
  }
  Cand b = {-INFINITY, 0x7fffffff};
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const Cand c = {live[j] ? score[j] : -INFINITY, live[j] ? tok[j] : 0x7fffffff};
    b = cand_better(b, c);
  }
  b = cand_wave(b);
  return b.c == 0x7fffffff ? first : b.c;
}

// One wave per node: the 15 slots in order, the state (count, ended) wave-uniform, `used` and the track's mask bits per-lane
// predicates on the two registers that hold the pitches below 128 (pitch p = lane p & 63, register p >> 6).  The rows'
// addresses depend on no decision: the row of slot s + 1 is in flight while slot s is decided, and nothing is read behind
// the slot that draws the EOS.  Lane l < 30 keeps token l of the node (slot l / 2, head l & 1) and stores it at the end.
// CHART: node_tag[n] is the node's cell 128 g + 32 track + step (int32, pm_node_cells) instead of its track (uint8), and for
// a track with its bit in track_bits a pitch is a candidate only if bit (pitch % 12) of chart[32 g + step] is set as well.
// The chart index is clamped into [0, chart_words), so nothing outside `chart` is read whatever node_tag holds; a set that
// leaves no pitch gives the empty chord by the rule for candidates that run out.  Without CHART the last three arguments are
// not read.
template <int MODE, bool CHART>
__global__ void __launch_bounds__(256) k_sample_chords(const float* __restrict__ c_logits,
                                                       const typename std::conditional<CHART, int32_t, uint8_t>::type* __restrict__ node_tag,
                                                       int64_t N, const PmChordRules R, float inv_tp, float inv_td, int greedy_heads,
                                                       int top_k, uint32_t seed, int* __restrict__ tokens, int* __restrict__ note_count,
                                                       const int32_t* __restrict__ chart, int chart_words, int track_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                                           // wave-uniform
  const int tag = __builtin_amdgcn_readfirstlane((int)node_tag[n]);
  const int t = (CHART ? tag >> 5 : tag) & 3;
  int min_n = 0, max_n = 1;
  uint32_t w0 = 0, w1 = 0;                                                      // this lane's words of the track's mask
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (t == k) {
      min_n = R.min_notes[k]; max_n = R.max_notes[k];
      w0 = R.pitch_mask[k][lane >> 5]; w1 = R.pitch_mask[k][2 + (lane >> 5)];
    }
  bool allow0 = (w0 >> (lane & 31)) & 1u, allow1 = (w1 >> (lane & 31)) & 1u;
  if (CHART && ((track_bits >> t) & 1)) {                                       // (wave-uniform) the chart binds this track
    const int at = min(max((tag >> 7) * 32 + (tag & 31), 0), chart_words - 1);  // bar tag >> 7, step tag & 31
    const uint32_t set = (uint32_t)chart[at];
    allow0 = allow0 && ((set >> (lane % 12)) & 1u);
    allow1 = allow1 && ((set >> ((lane + 64) % 12)) & 1u);
  }
  const float* x = c_logits + n * (PM_N_SLOTS * PM_N_TOK);
  const int tokp[3] = {lane, lane + 64, lane + 128};
  const int tokd[2] = {lane - 3, lane + 192 - PM_N_PITCH};
  const bool candd[2] = {lane >= 3, lane + 192 - PM_N_PITCH < N_DUR_CAND};
  bool used0 = false, used1 = false;
  int count = 0, slot = 0;
  int mine = (lane & 1) ? DUR_PAD : PITCH_PAD;
  float v[4], nx[4] = {0.f, 0.f, 0.f, 0.f};
  load_row(x, lane, v);
  for (; slot < PM_N_SLOTS; ++slot) {
    if (slot + 1 < PM_N_SLOTS) load_row(x + (slot + 1) * PM_N_TOK, lane, nx);
    const uint32_t r = (uint32_t)(n * PM_N_SLOTS + slot);
    const bool room = count < max_n;
    bool candp[3] = {allow0 && !used0 && room, allow1 && !used1 && room, false};
    const bool any = __ballot(candp[0] || candp[1]) != 0ull;
    candp[2] = lane == PITCH_EOS - 128 && (count >= min_n || !any);
    const float vp[3] = {v[0], v[1], v[2]};
    const int p = draw_head<MODE, 3>(vp, tokp, candp, (greedy_heads & 1) != 0, inv_tp, top_k, R.top_p, pm_edge_key(seed, 0u, r), lane);
    if (p >= 128) {                                                             // the EOS (nothing else is a candidate there)
      if (lane == 2 * slot) mine = PITCH_EOS;
      if (lane == 2 * slot + 1) mine = DUR_EOS;
      break;
    }
    const float vd[2] = {v[2], v[3]};
    const int d = draw_head<MODE, 2>(vd, tokd, candd, (greedy_heads & 2) != 0, inv_td, top_k, R.top_p, pm_edge_key(seed, 1u, r), lane);
    if (lane == 2 * slot) mine = p;
    if (lane == 2 * slot + 1) mine = d;
    used0 = used0 || lane == p;
    used1 = used1 || lane + 64 == p;
    ++count;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = nx[j];
  }
  if (lane < 2 * PM_N_SLOTS) tokens[n * (2 * PM_N_SLOTS) + lane] = mine;
  if (note_count && lane == 0) note_count[n] = count;
}

// ---- structure sampling ("Structure sampling", PmStructureRules) -----------------------------------------------------
template <bool NOISE>
__global__ void __launch_bounds__(256) k_sample_structure(const float* __restrict__ s_logits, int G, const PmStructureRules R,
                                                          float inv_t, uint32_t seed, float* __restrict__ s_f32,
                                                          uint8_t* __restrict__ s_u8, int* __restrict__ track_count) {
  const HalfBar h(G);
  const int half = h.half, t = h.t;
  const int64_t g = h.g;
  const bool valid = h.valid;
  const uint32_t key = NOISE ? pm_edge_key(seed, 2u, (uint32_t)g) : 0u;
  bool allow[4], on[4];
  unsigned sk[4];                                                               // ukey(score)
  float x[4];
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = valid ? s_logits[h.cell(k)] : 0.f;         // four loads in flight
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    allow[k] = (R.step_mask[k] >> t) & 1u;
    float score = __fsub_rn(x[k], R.bias[k]);
    if (NOISE) {
      const float u = unit_noise(key, (uint32_t)(32 * k + t));
      score = __fadd_rn(__fmul_rn(score, inv_t), __fsub_rn(logf(u), logf(1.0f - u)));
    }
    sk[k] = ukey(score);
    const bool nonneg = !(score < 0.f);
    const int mn = R.min_active[k], mx = R.max_active[k];
    if (mn == 0 && mx == 32) {                                                  // (wave-uniform) no bound can bind
      on[k] = allow[k] && nonneg;
    } else if (mx == 0) {                                                       // (wave-uniform) muted
      on[k] = false;
    } else {
      // cells of the track that outrank this lane's: a higher key, or the same key at a lower timestep
      int rank = 0;
      for (uint32_t m = R.step_mask[k]; m; m &= m - 1u) {                       // (scalar loop: the allowed timesteps)
        const int l = __builtin_ctz(m);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)sk[k], l);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)sk[k], l + 32);
        const unsigned s = half ? hi : lo;
        rank += (s > sk[k] || (s == sk[k] && l < t)) ? 1 : 0;
      }
      on[k] = allow[k] && (rank < mn || (rank < mx && nonneg));
    }
    any |= h.ballot(valid && on[k]);
  }
  // no empty bar: the best allowed cell of the tracks that are not muted, the lowest cell index on ties
  if (__ballot(valid && any == 0u) != 0ull) {                                   // (wave-uniform)
    unsigned bk = 0u;
    int bc = 0x7fffffff;
#pragma unroll
    for (int k = 3; k >= 0; --k)
      if (allow[k] && R.max_active[k] > 0 && (bc == 0x7fffffff || sk[k] >= bk)) { bk = sk[k]; bc = 32 * k + t; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {                                          // stays inside the half
      const unsigned ok = (unsigned)__shfl_xor((int)bk, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (oc != 0x7fffffff && (bc == 0x7fffffff || ok > bk || (ok == bk && oc < bc))) { bk = ok; bc = oc; }
    }
    if (any == 0u && (bc & 31) == t) {
#pragma unroll
      for (int k = 0; k < 4; ++k) on[k] = on[k] || bc == 32 * k + t;
    }
  }
  int mine = 0;                                                                 // lane k < 4 of the half: the count of track k
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = __popc(h.ballot(valid && on[k]));
    if (t == k) mine = n;
  }
  if (!valid) return;
  h.store(on, s_f32, s_u8);
  if (track_count && t < 4) track_count[g * 4 + t] = mine;
}

}  // namespace

// The kernel form MODE of (every head greedy, top_k, top_p), handed to `launch` as a compile-time constant, and the rank
// bound kk of the filter pass.
template <class F>
static void sample_dispatch(bool all_greedy, int top_k, float top_p, F&& launch) {
  const int kk = top_k == 0 ? 0x7fffffff : top_k;
  if (all_greedy || top_k == 1) launch(std::integral_constant<int, SAMPLE_GREEDY>(), kk);
  else if (top_p < 1.f) launch(std::integral_constant<int, SAMPLE_TOPP>(), kk);
  else if (top_k > 0 && top_k < PM_N_PITCH) launch(std::integral_constant<int, SAMPLE_TOPK>(), kk);
  else launch(std::integral_constant<int, SAMPLE_PLAIN>(), kk);
}

extern "C" uint32_t pm_sample_hash(uint32_t seed, uint32_t row, uint32_t head, uint32_t token) {
  return pm_group_hash(pm_edge_key(seed, head, row), token) >> 9;
}

extern "C" int pm_sample_tokens(const float* c_logits, int64_t rows, float temperature, int32_t top_k, float top_p,
                                uint32_t seed, int32_t* tokens, pm_stream_t stream) {
  if (!c_logits || !tokens || rows <= 0 || rows >= ((int64_t)1 << 32)) return PM_E_INVALID;
  if (!(temperature >= 0.f) || !(temperature <= 3.4028234663852886e38f)) return PM_E_INVALID;      // NaN, inf, negative
  if (top_k < 0 || !(top_p > 0.f) || !(top_p <= 1.f)) return PM_E_INVALID;
  sample_dispatch(temperature == 0.f, top_k, top_p, [&](auto mode, int kk) {
    const float inv_t = decltype(mode)::value == SAMPLE_GREEDY ? 1.f : (float)(1.0 / (double)temperature);
    hipLaunchKernelGGL(k_sample_tokens<decltype(mode)::value>, dim3((unsigned)pm_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                       c_logits, rows, inv_t, kk, top_p, seed, tokens);
  });
  return pm_check_launch();
}

// the rules every chord entry refuses (PM_E_INVALID before any launch)
static bool chord_rules_ok(const PmChordRules& R) {
  for (int h = 0; h < 2; ++h)
    if (!(R.temperature[h] >= 0.f) || !(R.temperature[h] <= 3.4028234663852886e38f)) return false;   // NaN, inf, negative
  if (R.top_k < 0 || !(R.top_p > 0.f) || !(R.top_p <= 1.f)) return false;
  for (int k = 0; k < 4; ++k)
    if (R.min_notes[k] < 0 || R.max_notes[k] < 1 || R.max_notes[k] > PM_N_SLOTS - 1 || R.min_notes[k] > R.max_notes[k])
      return false;
  return true;
}

// the launch of k_sample_chords<MODE, CHART> for checked arguments
template <bool CHART, class Tag>
static int launch_chords(const float* c_logits, const Tag* node_tag, int64_t N, const PmChordRules& R, uint32_t seed,
                         int32_t* tokens, int32_t* note_count, const int32_t* chart, int chart_words, int track_bits,
                         pm_stream_t stream) {
  const int zero_t = (R.temperature[0] == 0.f ? 1 : 0) | (R.temperature[1] == 0.f ? 2 : 0);
  sample_dispatch(zero_t == 3, R.top_k, R.top_p, [&](auto mode, int kk) {
    const int greedy = decltype(mode)::value == SAMPLE_GREEDY ? 3 : zero_t;
    const float inv_tp = (greedy & 1) ? 1.f : (float)(1.0 / (double)R.temperature[0]);
    const float inv_td = (greedy & 2) ? 1.f : (float)(1.0 / (double)R.temperature[1]);
    hipLaunchKernelGGL((k_sample_chords<decltype(mode)::value, CHART>), dim3((unsigned)pm_cdiv(N, 4)), dim3(256), 0,
                       (hipStream_t)stream, c_logits, node_tag, N, R, inv_tp, inv_td, greedy, kk, seed, tokens, note_count, chart,
                       chart_words, track_bits);
  });
  return pm_check_launch();
}

extern "C" int pm_sample_chords(const float* c_logits, const uint8_t* node_track, int64_t N, const PmChordRules* rules,
                                uint32_t seed, int32_t* tokens, int32_t* note_count, pm_stream_t stream) {
  if (!c_logits || !node_track || !rules || !tokens || N <= 0 || N * PM_N_SLOTS >= ((int64_t)1 << 32)) return PM_E_INVALID;
  const PmChordRules R = *rules;
  if (!chord_rules_ok(R)) return PM_E_INVALID;
  return launch_chords<false>(c_logits, node_track, N, R, seed, tokens, note_count, nullptr, 0, 0, stream);
}

extern "C" int pm_sample_chords_at(const float* c_logits, const int32_t* node_cell, int64_t N, const int32_t* chart, int32_t G,
                                   int32_t track_bits, const PmChordRules* rules, uint32_t seed, int32_t* tokens,
                                   int32_t* note_count, pm_stream_t stream) {
  if (!c_logits || !node_cell || !chart || !rules || !tokens || N <= 0 || N * PM_N_SLOTS >= ((int64_t)1 << 32)) return PM_E_INVALID;
  if (G <= 0 || (int64_t)G * 128 > 0x7fffffffLL || track_bits < 0 || track_bits > 15) return PM_E_INVALID;
  if ((((uintptr_t)c_logits | (uintptr_t)node_cell | (uintptr_t)chart | (uintptr_t)tokens | (uintptr_t)note_count) & 3) != 0)
    return PM_E_INVALID;
  const PmChordRules R = *rules;
  if (!chord_rules_ok(R)) return PM_E_INVALID;
  return launch_chords<true>(c_logits, node_cell, N, R, seed, tokens, note_count, chart, 32 * G, track_bits, stream);
}

extern "C" int pm_sample_structure(const float* s_logits, int32_t G, const PmStructureRules* rules, uint32_t seed, float* s_f32,
                                   uint8_t* s_u8, int32_t* track_count, pm_stream_t stream) {
  if (!s_logits || !rules || (!s_f32 && !s_u8) || G <= 0) return PM_E_INVALID;
  const PmStructureRules R = *rules;
  const float FMAX = 3.4028234663852886e38f;
  if (!(R.temperature >= 0.f) || !(R.temperature <= FMAX)) return PM_E_INVALID;                   // NaN, inf, negative
  bool some = false;
  for (int k = 0; k < 4; ++k) {
    if (!(R.bias[k] >= -FMAX) || !(R.bias[k] <= FMAX)) return PM_E_INVALID;
    if (R.min_active[k] < 0 || R.max_active[k] > 32 || R.min_active[k] > R.max_active[k]) return PM_E_INVALID;
    if (R.min_active[k] > __builtin_popcount(R.step_mask[k])) return PM_E_INVALID;
    some = some || (R.max_active[k] > 0 && R.step_mask[k] != 0u);
  }
  if (!some) return PM_E_INVALID;
  const dim3 grid((unsigned)pm_cdiv(G, 8)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (R.temperature == 0.f)
    hipLaunchKernelGGL(k_sample_structure<false>, grid, block, 0, st, s_logits, G, R, 1.f, seed, s_f32, s_u8, track_count);
  else
    hipLaunchKernelGGL(k_sample_structure<true>, grid, block, 0, st, s_logits, G, R, (float)(1.0 / (double)R.temperature), seed,
                       s_f32, s_u8, track_count);
  return pm_check_launch();
}

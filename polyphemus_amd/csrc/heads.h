// heads.h — the two heads of a content-logit row and the structure prediction, defined once for sample.hip (sampled
// generation), loss.hip (the evaluation and training metrics) and score.hip (per-piece scores).
//
//   load_row        the row layout: 230 logits (920 B, read once) across a wave.
//   Cand, cand_better, cand_wave : a candidate of an arg-max (score, then the lower token index) and its wave reduction.
//   head_argmax     the arg-max of both heads of a loaded row: first index on ties (torch.argmax), the rule of the metrics
//                   (`_accuracies`, training.py:349-468).
//   structure_pred  the structure prediction of the metrics (`_structure_accuracy / _precision / _recall`,
//                   training.py:470-497): sigmoid(x) >= 0.5.
#pragma once
#include "common.h"

// a candidate of the arg-max: score, then the lower token index
struct Cand { float s; int c; };
__device__ static inline Cand cand_better(Cand a, Cand b) {
  return (b.s > a.s || (b.s == a.s && b.c < a.c)) ? b : a;
}
__device__ static inline Cand cand_wave(Cand a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Cand b;
    b.s = __shfl_xor(a.s, o, 64);
    b.c = __shfl_xor(a.c, o, 64);
    a = cand_better(a, b);
  }
  return a;
}

// A row of 230 logits (920 B, read once) across the wave: lane l holds the columns l, l + 64, l + 128, l + 192 (four coalesced
// 256-byte wave loads; the last one 38 lanes wide, -inf behind it).  Registers 0, 1 and the lanes 0..2 of register 2 are the
// pitch head (token = column), the lanes 3..63 of register 2 and register 3 the duration head (token = column - 131).
__device__ static inline void load_row(const float* __restrict__ x, int lane, float (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) v[j] = x[lane + 64 * j];
  v[3] = lane < PM_N_TOK - 192 ? x[lane + 192] : -INFINITY;
}

// The arg-max token of the pitch head (ip) and of the duration head (id) of a loaded row, in every lane.  A lane keeps the
// first of its columns that is above -inf and above its earlier ones, the wave takes the best by cand_better: the first index
// among equal maxima.  A head without a value above -inf (all -inf or NaN) gives 0x7fffffff, which is no token.
__device__ static inline void head_argmax(const float (&v)[4], int lane, int& ip, int& id) {
  Cand bp = {-INFINITY, 0x7fffffff}, bd = {-INFINITY, 0x7fffffff};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane + 64 * j;
    if (c < PM_N_PITCH) { if (v[j] > bp.s) { bp.s = v[j]; bp.c = c; } }
    else if (c < PM_N_TOK && v[j] > bd.s) { bd.s = v[j]; bd.c = c - PM_N_PITCH; }
  }
  ip = cand_wave(bp).c;
  id = cand_wave(bd).c;
}

// the structure prediction of the metrics: sigmoid(x) >= 0.5, as the reference takes it
__device__ static inline bool structure_pred(float x) { return 1.0f / (1.0f + expf(-x)) >= 0.5f; }

// optim.hip — fused Adam over one flat fp32 parameter buffer.
//
// Reference: optim.Adam(vae.parameters(), betas=(0.9,0.98), eps=1e-9) (train.py:181,
// training.json:11-18), stepped at training.py:160-166 as 152 per-tensor updates.  Here all
// parameters, gradients and moments live in four flat buffers (also the unit of the data-parallel
// gradient all-reduce), so the step is one HBM-bound pass: 16 B read + 12 B written per parameter (20 B + 16 B with the
// parameter average riding in it).
// Parameters whose gradient has been zero on EVERY step so far (the structure decoder under the
// reference's loss quirk, SURVEY B-1) stay bit-identical: m = v = 0 gives an update of 0 / eps = 0,
// the same end state as torch's `grad is None` skip.  This is not a general skip: a parameter with
// non-zero moments and a zero gradient on one step still moves here (torch.optim.Adam does the same
// for a zero-valued, non-None gradient); the reference never produces that case on this path.
#include "common.h"
#include <math.h>

// Adam's bias-correction scalars at step t, in double: the one formula of the host entry points and of the check's decision
__host__ __device__ static inline void adam_bias_scalars(int64_t t, float lr, float beta1, float beta2, float& step_size,
                                                         float& inv_bc2_sqrt) {
  const double bc1 = 1.0 - pow((double)beta1, (double)t);
  const double bc2 = 1.0 - pow((double)beta2, (double)t);
  step_size = (float)((double)lr / bc1);
  inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
}
// where the update's scalars come from: the host's values, or — read on the device — gscale from the clip block pm_grad_clip_finish
// wrote (CLIP) and the decision with its step_size / inv_bc2_sqrt from the status block of the check (GUARD); ema_w: the weight of
// the fresh parameter in the average (EMA), 1 - decay
struct AdamSources { float step_size, inv_bc2_sqrt, gscale; const double* clip; const unsigned* status; float ema_w; };
// The Adam update over the flat buffers, VT = float4 or float; n counts VTs.  GUARD || CLIP: thread 0 reads the device sources once
// per workgroup; a skipped step returns before any store.  The loop is one text, so with coef == 1 (gscale == grad_scale) and an
// applied decision the plain, the guarded and the clipped steps are bit-identical.  The lanes index the buffers themselves (the
// compiler still moves whole float4s) and the update is these three statements, no locals: which product of m's and of v's update
// the compiler fuses into the FMA depends on such details of the text, and a last bit of m or v with it.  EMA: behind them the
// average moves towards the parameter just stored (the lerp of torch.optim.swa_utils.get_ema_multi_avg_fn; a weight of 1 copies,
// since e + (p - e) is not exactly p in fp32) — 4 B more read and 4 B more written per parameter, and a skipped step leaves it alone.
// ET: how the average is moved, VT or — float4 kernel, an average that is not 16-byte aligned — four floats of element alignment
struct alignas(4) Float4U { float f[4]; };
template <typename VT, bool GUARD, bool CLIP, bool EMA, typename ET = VT>
__global__ void __launch_bounds__(256) k_adam(VT* __restrict__ p, const VT* __restrict__ g, VT* __restrict__ m,
                                              VT* __restrict__ v, ET* __restrict__ ema, int64_t n, float b1, float b2, float eps,
                                              AdamSources a) {
  static_assert(sizeof(ET) == sizeof(VT), "the average moves in steps of one VT");
  float step_size = a.step_size, inv_bc2_sqrt = a.inv_bc2_sqrt, gscale = a.gscale;
  if constexpr (GUARD || CLIP) {
    __shared__ unsigned sh[4];
    if (threadIdx.x == 0) {
      if (CLIP) sh[3] = __float_as_uint((float)a.clip[PM_CLIP_GSCALE]);
      if (GUARD) { sh[0] = a.status[PM_OVF_LAST]; sh[1] = a.status[PM_OVF_STEP_SIZE]; sh[2] = a.status[PM_OVF_INV_BC2]; }
    }
    __syncthreads();
    if (GUARD && sh[0]) return;
    if (GUARD) { step_size = __uint_as_float(sh[1]); inv_bc2_sqrt = __uint_as_float(sh[2]); }
    if (CLIP) gscale = __uint_as_float(sh[3]);
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float* P = reinterpret_cast<float*>(p + i); const float* Gd = reinterpret_cast<const float*>(g + i);
    float* M = reinterpret_cast<float*>(m + i); float* V = reinterpret_cast<float*>(v + i);
    ET avg;                                       // (the average's VT in registers: one whole load in front of the weight test)
    if constexpr (EMA) avg = ema[i];
    float* E = reinterpret_cast<float*>(&avg);
#pragma unroll
    for (int j = 0; j < (int)(sizeof(VT) / 4); ++j) {
      const float gr = Gd[j] * gscale;
      M[j] = b1 * M[j] + (1.f - b1) * gr;
      V[j] = b2 * V[j] + (1.f - b2) * gr * gr;
      P[j] -= step_size * (M[j] / (sqrtf(V[j]) * inv_bc2_sqrt + eps));
      if constexpr (EMA) E[j] = (a.ema_w == 1.f) ? P[j] : E[j] + a.ema_w * (P[j] - E[j]);
    }
    if constexpr (EMA) ema[i] = avg;
  }
}
// the float4 kernel for 16-byte-aligned buffers with n % 4 == 0, the scalar one otherwise; at most 4096 workgroups of 256.  The
// average's own alignment never picks the kernel — the two differ in a last bit of m (see above), and the option must not move
// p, m or v: the float4 kernel moves an average that is not 16-byte aligned as four floats
template <bool GUARD, bool CLIP, bool EMA = false>
static int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float b1, float b2, float eps,
                       const AdamSources& a, pm_stream_t stream, float* ema = nullptr) {
  const bool vec = !(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) && (n % 4) == 0;
  const int64_t nv = vec ? n / 4 : n;
  int64_t nb = pm_cdiv(nv, 256); if (nb > 4096) nb = 4096;
  if constexpr (EMA) {
    if (vec && ((uintptr_t)ema & 15)) {
      hipLaunchKernelGGL((k_adam<float4, GUARD, CLIP, true, Float4U>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                         reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m),
                         reinterpret_cast<float4*>(v), reinterpret_cast<Float4U*>(ema), nv, b1, b2, eps, a);
      return pm_check_launch();
    }
  }
  if (vec)
    hipLaunchKernelGGL((k_adam<float4, GUARD, CLIP, EMA>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m),
                       reinterpret_cast<float4*>(v), reinterpret_cast<float4*>(ema), nv, b1, b2, eps, a);
  else
    hipLaunchKernelGGL((k_adam<float, GUARD, CLIP, EMA>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema,
                       nv, b1, b2, eps, a);
  return pm_check_launch();
}
// acc = (first ? 0 : acc) + scale * g   (gradient accumulation over micro-batches, training.py:149,158)
__global__ void __launch_bounds__(256) k_grad_accumulate(const float* __restrict__ g, float* __restrict__ acc, int64_t n,
                                                         float scale, int first) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = g[i] * scale;
    acc[i] = first ? v : acc[i] + v;
  }
}
extern "C" int pm_grad_accumulate(const float* grads, float* accum, int64_t n, float scale, int32_t first,
                                  pm_stream_t stream) {
  if (!grads || !accum || n <= 0) return PM_E_INVALID;
  int64_t nb = pm_cdiv(n, 256); if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_grad_accumulate, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, grads, accum, n, scale,
                     first);
  return pm_check_launch();
}
extern "C" int pm_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                            float beta1, float beta2, float eps, int32_t step, float grad_scale, pm_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return PM_E_INVALID;
  AdamSources a{0.f, 0.f, grad_scale, nullptr, nullptr};
  adam_bias_scalars(step, lr, beta1, beta2, a.step_size, a.inv_bc2_sqrt);
  return launch_adam<false, false>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream);
}

// ---- guarded step (include/polyphemus_hip.h, "guarded optimizer step"; GradScaler, training.py:160-162)
// non-finite = exponent bits all ones (inf or NaN); a bit test no fast-math flag can fold away, unlike isfinite
__device__ static inline bool nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u; }
// the workgroup's verdict, one atomic per workgroup.  With a decision to make it goes into the ticket word itself — the count of
// finished workgroups in the low 16 bits, of workgroups that saw a non-finite value from bit 16 on — so the last workgroup
// (the one that takes ticket gridDim.x - 1) reads every other verdict from the value its own add returns: read-modify-writes of
// one word are totally ordered, and no fence (an L2 write-back per workgroup: 2048 of them cost 47 us) is needed
struct NonfiniteDecision { int64_t* step; int64_t* skipped; const unsigned* clamp; float lr, beta1, beta2; };
__device__ static inline void check_epilogue(bool bad, unsigned* __restrict__ status, const NonfiniteDecision& d) {
  const bool wg_bad = __syncthreads_or(bad);
  if (threadIdx.x != 0) return;
  if (!d.step) {
    if (wg_bad) atomicOr(status + PM_OVF_PENDING, (unsigned)PM_OVF_NONFINITE_BIT);
    return;
  }
  const unsigned mine = 1u + (wg_bad ? 1u << 16 : 0u);
  const unsigned total = atomicAdd(status + PM_OVF_TICKET, mine) + mine;
  if ((total & 0xffffu) != gridDim.x) return;
  atomicExch(status + PM_OVF_TICKET, 0u);                       // (for the next launch)
  unsigned why = status[PM_OVF_PENDING] | ((total >> 16) ? (unsigned)PM_OVF_NONFINITE_BIT : 0u);
  if (d.clamp && __hip_atomic_load(d.clamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != status[PM_OVF_SNAP])
    why |= PM_OVF_SATURATED_BIT;                               // (any change: a pm_h2_clamp_events reset inside the window too)
  status[PM_OVF_PENDING] = 0;
  status[PM_OVF_LAST] = why;
  if (why) {
    *d.skipped += 1;
    status[(why & PM_OVF_SATURATED_BIT) ? PM_OVF_N_SATURATED : PM_OVF_N_NONFINITE] += 1;
    return;
  }
  const int64_t t = *d.step + 1;
  *d.step = t;
  float step_size, inv_bc2_sqrt;
  adam_bias_scalars(t, d.lr, d.beta1, d.beta2, step_size, inv_bc2_sqrt);
  status[PM_OVF_STEP_SIZE] = __float_as_uint(step_size);
  status[PM_OVF_INV_BC2] = __float_as_uint(inv_bc2_sqrt);
}
// one workgroup of 1024 threads per CU, four loads in flight per thread: the pass runs at the HBM rate with 256 workgroups, so the
// decision word takes 256 same-address atomics, not 2048 (serialised, those cost 26 us)
constexpr int kCheckThreads = 1024, kCheckBlocks = 256;
static_assert(kCheckBlocks <= PM_CLIP_PARTIALS, "one partial slot per workgroup of the check's launch shape");
static_assert(kCheckBlocks < (1 << 16), "the two counts of the decision word must not overflow into each other");

// ---- sum of squares of the gradient (include/polyphemus_hip.h, "gradient clipping by the global norm")
// (double)g * (double)g is exact (24 x 24 significand bits) and cannot overflow or vanish (|g| <= 3.4e38 -> 1.2e77; the
// smallest denormal 1.4e-45 -> 2e-90); every sum below runs in one fixed order, so one gradient gives one set of bits
__device__ static inline double sq4(const uint4& u) {
  const double a = (double)__uint_as_float(u.x), b = (double)__uint_as_float(u.y), c = (double)__uint_as_float(u.z),
               d = (double)__uint_as_float(u.w);
  return (a * a + b * b) + (c * c + d * d);
}
// the workgroup's sum: a shuffle tree per wave, the waves' sums added in wave order by thread 0, one plain store into the
// workgroup's own slot; workgroup 0 zeroes the slots past the grid, so a smaller launch never leaves an earlier launch's there
__device__ static inline void sumsq_epilogue(double acc, double* __restrict__ clip) {
  __shared__ double wsum[kCheckThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  double* partials = clip + PM_CLIP_PARTIALS_AT;
  if (threadIdx.x == 0) {
    double s = wsum[0];
    for (int w = 1; w < kCheckThreads / 64; ++w) s += wsum[w];
    partials[blockIdx.x] = s;
  }
  if (blockIdx.x == 0)
    for (unsigned k = gridDim.x + threadIdx.x; k < (unsigned)PM_CLIP_PARTIALS; k += kCheckThreads) partials[k] = 0.0;
}
// the strided loops of the read, four loads in flight per thread in the uint4 one
template <bool CHECK, bool SUMSQ>
__device__ static inline void grad_pass4(const uint4* __restrict__ g, int64_t n4, int64_t i, int64_t stride, bool& bad,
                                         double& acc) {
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const uint4 u0 = g[i], u1 = g[i + stride], u2 = g[i + 2 * stride], u3 = g[i + 3 * stride];
    if (CHECK)
      bad |= nonfinite_bits(u0.x) | nonfinite_bits(u0.y) | nonfinite_bits(u0.z) | nonfinite_bits(u0.w) |
             nonfinite_bits(u1.x) | nonfinite_bits(u1.y) | nonfinite_bits(u1.z) | nonfinite_bits(u1.w) |
             nonfinite_bits(u2.x) | nonfinite_bits(u2.y) | nonfinite_bits(u2.z) | nonfinite_bits(u2.w) |
             nonfinite_bits(u3.x) | nonfinite_bits(u3.y) | nonfinite_bits(u3.z) | nonfinite_bits(u3.w);
    if (SUMSQ) acc += (sq4(u0) + sq4(u1)) + (sq4(u2) + sq4(u3));
  }
  for (; i < n4; i += stride) {
    const uint4 u = g[i];
    if (CHECK) bad |= nonfinite_bits(u.x) | nonfinite_bits(u.y) | nonfinite_bits(u.z) | nonfinite_bits(u.w);
    if (SUMSQ) acc += sq4(u);
  }
}
template <bool CHECK, bool SUMSQ>
__device__ static inline void grad_pass1(const unsigned* __restrict__ g, int64_t n, int64_t i, int64_t stride, bool& bad,
                                         double& acc) {
  for (; i < n; i += stride) {
    const unsigned u = g[i];
    if (CHECK) bad |= nonfinite_bits(u);
    if (SUMSQ) { const double x = (double)__uint_as_float(u); acc += x * x; }
  }
}
// one read of the gradient for the check (CHECK), the sum of squares (SUMSQ) or both: the sum first, the decision last.  VT = uint4
// or unsigned; n counts VTs.  (The kernel forms the first index and the stride itself: there the compiler reads blockDim.x from the
// dispatch packet without the extra load a device function costs)
template <typename VT, bool CHECK, bool SUMSQ>
__global__ void __launch_bounds__(kCheckThreads) k_grad_pass(const VT* __restrict__ g, int64_t n, unsigned* __restrict__ status,
                                                             NonfiniteDecision d, double* __restrict__ clip) {
  static_assert(CHECK || SUMSQ, "a pass that reads the gradient for nothing");
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  bool bad = false; double acc = 0.0;
  if constexpr (sizeof(VT) == 16) grad_pass4<CHECK, SUMSQ>(g, n, i0, stride, bad, acc);
  else grad_pass1<CHECK, SUMSQ>(g, n, i0, stride, bad, acc);
  if constexpr (SUMSQ) sumsq_epilogue(acc, clip);
  if constexpr (CHECK) check_epilogue(bad, status, d);
}
// the uint4 kernel for a 16-byte-aligned gradient with n % 4 == 0, the scalar one otherwise, in the launch shape above
template <bool CHECK, bool SUMSQ>
static int launch_grad_pass(const float* grads, int64_t n, uint32_t* status, const NonfiniteDecision& d, double* clip,
                            pm_stream_t stream) {
  const bool vec = !((uintptr_t)grads & 15) && (n % 4) == 0;
  const int64_t nv = vec ? n / 4 : n;
  int64_t nb = pm_cdiv(nv, kCheckThreads); if (nb > kCheckBlocks) nb = kCheckBlocks;
  if (vec)
    hipLaunchKernelGGL((k_grad_pass<uint4, CHECK, SUMSQ>), dim3((unsigned)nb), dim3(kCheckThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(grads), nv, status, d, clip);
  else
    hipLaunchKernelGGL((k_grad_pass<unsigned, CHECK, SUMSQ>), dim3((unsigned)nb), dim3(kCheckThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned*>(grads), nv, status, d, clip);
  return pm_check_launch();
}
// the decision the check is to make (none without `step`); false if `window` asks for a clamp word that is not there
static bool make_decision(NonfiniteDecision& d, int64_t* step, int64_t* skipped, float lr, float beta1, float beta2,
                          int32_t window) {
  d = NonfiniteDecision{step, skipped, nullptr, lr, beta1, beta2};
  if (step && window) d.clamp = pm_h2_clamp_word_ready();
  return !(step && window) || d.clamp;
}
// the finish (one workgroup): the partials added in slot order by one thread, then the formula of the header
__global__ void __launch_bounds__(PM_CLIP_PARTIALS) k_grad_clip_finish(double* __restrict__ clip, float grad_scale,
                                                                       float max_norm, double* __restrict__ row) {
  __shared__ double part[PM_CLIP_PARTIALS];
  part[threadIdx.x] = clip[PM_CLIP_PARTIALS_AT + threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sumsq = part[0];
  for (int k = 1; k < PM_CLIP_PARTIALS; ++k) sumsq += part[k];
  const double norm = fabs((double)grad_scale) * sqrt(sumsq);
  const double coef = fmin(1.0, (double)max_norm / (norm + 1e-6));
  const float gscale = (float)((double)grad_scale * coef);
  clip[PM_CLIP_NORM] = norm; clip[PM_CLIP_COEF] = coef; clip[PM_CLIP_GSCALE] = (double)gscale; clip[PM_CLIP_SUMSQ] = sumsq;
  if (row) { row[0] = norm; row[1] = coef; }
}
__global__ void k_adam_bias_scalars(const int64_t* __restrict__ steps, int64_t n, float lr, float beta1, float beta2,
                                    float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    adam_bias_scalars(steps[i], lr, beta1, beta2, out[2 * i], out[2 * i + 1]);
}
extern "C" int pm_grad_nonfinite_check(const float* grads, int64_t n, uint32_t* status, int64_t* step, int64_t* skipped,
                                       float lr, float beta1, float beta2, int32_t window, pm_stream_t stream) {
  NonfiniteDecision d;
  if (!grads || !status || n <= 0 || (step && !skipped) || !make_decision(d, step, skipped, lr, beta1, beta2, window))
    return PM_E_INVALID;
  return launch_grad_pass<true, false>(grads, n, status, d, nullptr, stream);
}
extern "C" int pm_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                    float beta1, float beta2, float eps, float grad_scale, const uint32_t* status,
                                    pm_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !status || n <= 0) return PM_E_INVALID;
  const AdamSources a{0.f, 0.f, grad_scale, nullptr, status};
  return launch_adam<true, false>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream);
}
extern "C" int pm_adam_bias_scalars(const int64_t* steps, int64_t n, float lr, float beta1, float beta2, float* out,
                                    pm_stream_t stream) {
  if (!steps || !out || n <= 0) return PM_E_INVALID;
  int64_t nb = pm_cdiv(n, 256); if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(k_adam_bias_scalars, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, steps, n, lr, beta1,
                     beta2, out);
  return pm_check_launch();
}

// ---- gradient clipping by the global norm (include/polyphemus_hip.h)
extern "C" int pm_grad_sumsq(const float* grads, int64_t n, double* clip, pm_stream_t stream) {
  if (!grads || !clip || n <= 0 || ((uintptr_t)clip & 7)) return PM_E_INVALID;
  return launch_grad_pass<false, true>(grads, n, nullptr, NonfiniteDecision{}, clip, stream);
}
extern "C" int pm_grad_nonfinite_check_sumsq(const float* grads, int64_t n, uint32_t* status, int64_t* step, int64_t* skipped,
                                             float lr, float beta1, float beta2, int32_t window, double* clip,
                                             pm_stream_t stream) {
  NonfiniteDecision d;
  if (!grads || !status || !clip || n <= 0 || (step && !skipped) || ((uintptr_t)clip & 7) ||
      !make_decision(d, step, skipped, lr, beta1, beta2, window))
    return PM_E_INVALID;
  return launch_grad_pass<true, true>(grads, n, status, d, clip, stream);
}
extern "C" int pm_grad_clip_finish(double* clip, float grad_scale, float max_norm, double* row, pm_stream_t stream) {
  if (!clip || ((uintptr_t)clip & 7) || ((uintptr_t)row & 7) || !(max_norm > 0.f)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_grad_clip_finish, dim3(1), dim3(PM_CLIP_PARTIALS), 0, (hipStream_t)stream, clip, grad_scale, max_norm,
                     row);
  return pm_check_launch();
}
extern "C" int pm_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                    float beta1, float beta2, float eps, int32_t step, const double* clip,
                                    const uint32_t* status, pm_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !clip || ((uintptr_t)clip & 7) || n <= 0 || (!status && step <= 0))
    return PM_E_INVALID;
  AdamSources a{0.f, 0.f, 0.f, clip, status};
  if (status) return launch_adam<true, true>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream);
  adam_bias_scalars(step, lr, beta1, beta2, a.step_size, a.inv_bc2_sqrt);       // (unguarded: the host's scalars, as pm_adam_step)
  return launch_adam<false, true>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream);
}

// ---- exponential moving average of the parameters (include/polyphemus_hip.h)
// [a, a + n) and [b, b + n) share an element
static inline bool ranges_overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
  return x < y ? y - x < len : x - y < len;
}
extern "C" int pm_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale, float ema_weight,
                                const double* clip, const uint32_t* status, pm_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !ema || n <= 0 || ((uintptr_t)clip & 7) || (!status && step <= 0) ||
      !(ema_weight > 0.f && ema_weight <= 1.f))                                  // (a NaN weight fails the comparison too)
    return PM_E_INVALID;
  if (ranges_overlap(ema, params, n) || ranges_overlap(ema, grads, n) || ranges_overlap(ema, exp_avg, n) ||
      ranges_overlap(ema, exp_avg_sq, n))
    return PM_E_INVALID;
  AdamSources a{0.f, 0.f, grad_scale, clip, status, ema_weight};
  if (!status) adam_bias_scalars(step, lr, beta1, beta2, a.step_size, a.inv_bc2_sqrt);
  if (status && clip) return launch_adam<true, true, true>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream, ema);
  if (status) return launch_adam<true, false, true>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream, ema);
  if (clip) return launch_adam<false, true, true>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream, ema);
  return launch_adam<false, false, true>(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, a, stream, ema);
}
// a <-> b, VT = float4 or float; n counts VTs
template <typename VT>
__global__ void __launch_bounds__(256) k_buffer_swap(VT* __restrict__ a, VT* __restrict__ b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const VT x = a[i], y = b[i];
    a[i] = y; b[i] = x;
  }
}
extern "C" int pm_buffer_swap(float* a, float* b, int64_t n, pm_stream_t stream) {
  if (!a || !b || n <= 0 || ranges_overlap(a, b, n)) return PM_E_INVALID;
  const bool vec = !(((uintptr_t)a | (uintptr_t)b) & 15) && (n % 4) == 0;
  const int64_t nv = vec ? n / 4 : n;
  int64_t nb = pm_cdiv(nv, 256); if (nb > 4096) nb = 4096;
  if (vec)
    hipLaunchKernelGGL(k_buffer_swap<float4>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(a), reinterpret_cast<float4*>(b), nv);
  else
    hipLaunchKernelGGL(k_buffer_swap<float>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a, b, nv);
  return pm_check_launch();
}

extern "C" int pm_abi_version(void) { return PM_ABI_VERSION; }
extern "C" const char* pm_build_info(void) { return "polyphemus_hip gfx950 (CDNA4) fp32-MFMA build " __DATE__; }

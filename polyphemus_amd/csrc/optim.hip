// optim.hip — fused Adam over one flat fp32 parameter buffer.
//
// Reference: optim.Adam(vae.parameters(), betas=(0.9,0.98), eps=1e-9) (train.py:181,
// training.json:11-18), stepped at training.py:160-166 as 152 per-tensor updates.  Here all
// parameters, gradients and moments live in four flat buffers (also the unit of the data-parallel
// gradient all-reduce), so the step is one HBM-bound pass: 16 B read + 12 B written per parameter.
// Parameters whose gradient has been zero on EVERY step so far (the structure decoder under the
// reference's loss quirk, SURVEY B-1) stay bit-identical: m = v = 0 gives an update of 0 / eps = 0,
// the same end state as torch's `grad is None` skip.  This is not a general skip: a parameter with
// non-zero moments and a zero gradient on one step still moves here (torch.optim.Adam does the same
// for a zero-valued, non-None gradient); the reference never produces that case on this path.
#include "common.h"
#include <math.h>

// The Adam update over the flat buffers, ONE text for the plain, the guarded and the clipped kernels: each names p, g, m, v, the
// count (n4 / n), b1, b2, eps, step_size, inv_bc2_sqrt and gscale, so the three are expression for expression the same loop
#define PM_ADAM4_LOOP \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) { \
    float4 pv = p[i], gv = g[i], mv = m[i], vv = v[i]; \
    float* P = reinterpret_cast<float*>(&pv); float* Gd = reinterpret_cast<float*>(&gv); \
    float* M = reinterpret_cast<float*>(&mv); float* V = reinterpret_cast<float*>(&vv); \
    _Pragma("unroll") \
    for (int j = 0; j < 4; ++j) { \
      const float gr = Gd[j] * gscale; \
      M[j] = b1 * M[j] + (1.f - b1) * gr; \
      V[j] = b2 * V[j] + (1.f - b2) * gr * gr; \
      P[j] -= step_size * (M[j] / (sqrtf(V[j]) * inv_bc2_sqrt + eps)); \
    } \
    p[i] = pv; m[i] = mv; v[i] = vv; \
  }
#define PM_ADAM1_LOOP \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) { \
    const float gr = g[i] * gscale; \
    const float mm = b1 * m[i] + (1.f - b1) * gr; \
    const float vv = b2 * v[i] + (1.f - b2) * gr * gr; \
    m[i] = mm; v[i] = vv; \
    p[i] -= step_size * (mm / (sqrtf(vv) * inv_bc2_sqrt + eps)); \
  }
__global__ void __launch_bounds__(256) k_adam4(float4* __restrict__ p, const float4* __restrict__ g,
                                               float4* __restrict__ m, float4* __restrict__ v, int64_t n4, float b1,
                                               float b2, float step_size, float inv_bc2_sqrt, float eps, float gscale) {
  PM_ADAM4_LOOP
}
__global__ void __launch_bounds__(256) k_adam1(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, int64_t n, float b1, float b2, float step_size,
                                               float inv_bc2_sqrt, float eps, float gscale) {
  PM_ADAM1_LOOP
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
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1);
  const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  hipStream_t st = (hipStream_t)stream;
  const bool al = !(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15);
  if (al && (n % 4) == 0) {
    int64_t nb = pm_cdiv(n / 4, 256); if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_adam4, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<float4*>(params),
                       reinterpret_cast<const float4*>(grads), reinterpret_cast<float4*>(exp_avg),
                       reinterpret_cast<float4*>(exp_avg_sq), n / 4, beta1, beta2, step_size, inv_bc2_sqrt, eps,
                       grad_scale);
  } else {
    int64_t nb = pm_cdiv(n, 256); if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_adam1, dim3((unsigned)nb), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, beta1,
                       beta2, step_size, inv_bc2_sqrt, eps, grad_scale);
  }
  return pm_check_launch();
}

// ---- guarded step (include/polyphemus_hip.h, "guarded optimizer step"; GradScaler, training.py:160-162)
// Adam's bias-correction scalars at step t, in double as pm_adam_step forms them on the host
__device__ static inline void adam_bias_scalars(int64_t t, float lr, float beta1, float beta2, float& step_size,
                                                float& inv_bc2_sqrt) {
  const double bc1 = 1.0 - pow((double)beta1, (double)t);
  const double bc2 = 1.0 - pow((double)beta2, (double)t);
  step_size = (float)((double)lr / bc1);
  inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
}
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
// (the kernels form the first index and the stride themselves: there the compiler reads blockDim.x from the dispatch packet
// without the extra load a device function costs)
#define PM_PASS_INDEX (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x
// the read of the gradient, shared by the check (CHECK), the sum of squares (SUMSQ) and both in one pass
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
__global__ void __launch_bounds__(kCheckThreads) k_nonfinite4(const uint4* __restrict__ g, int64_t n4,
                                                              unsigned* __restrict__ status, NonfiniteDecision d) {
  bool bad = false; double acc = 0.0;
  grad_pass4<true, false>(g, n4, PM_PASS_INDEX, bad, acc);
  check_epilogue(bad, status, d);
}
__global__ void __launch_bounds__(kCheckThreads) k_nonfinite1(const unsigned* __restrict__ g, int64_t n,
                                                              unsigned* __restrict__ status, NonfiniteDecision d) {
  bool bad = false; double acc = 0.0;
  grad_pass1<true, false>(g, n, PM_PASS_INDEX, bad, acc);
  check_epilogue(bad, status, d);
}
// the check and the sum of squares in one read of the gradient
__global__ void __launch_bounds__(kCheckThreads) k_nonfinite4_sumsq(const uint4* __restrict__ g, int64_t n4,
                                                                    unsigned* __restrict__ status, NonfiniteDecision d,
                                                                    double* __restrict__ clip) {
  bool bad = false; double acc = 0.0;
  grad_pass4<true, true>(g, n4, PM_PASS_INDEX, bad, acc);
  sumsq_epilogue(acc, clip);
  check_epilogue(bad, status, d);
}
__global__ void __launch_bounds__(kCheckThreads) k_nonfinite1_sumsq(const unsigned* __restrict__ g, int64_t n,
                                                                    unsigned* __restrict__ status, NonfiniteDecision d,
                                                                    double* __restrict__ clip) {
  bool bad = false; double acc = 0.0;
  grad_pass1<true, true>(g, n, PM_PASS_INDEX, bad, acc);
  sumsq_epilogue(acc, clip);
  check_epilogue(bad, status, d);
}
__global__ void __launch_bounds__(kCheckThreads) k_grad_sumsq4(const uint4* __restrict__ g, int64_t n4,
                                                               double* __restrict__ clip) {
  bool bad = false; double acc = 0.0;
  grad_pass4<false, true>(g, n4, PM_PASS_INDEX, bad, acc);
  sumsq_epilogue(acc, clip);
}
__global__ void __launch_bounds__(kCheckThreads) k_grad_sumsq1(const unsigned* __restrict__ g, int64_t n,
                                                               double* __restrict__ clip) {
  bool bad = false; double acc = 0.0;
  grad_pass1<false, true>(g, n, PM_PASS_INDEX, bad, acc);
  sumsq_epilogue(acc, clip);
}
#undef PM_PASS_INDEX
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
// the workgroup reads the decision and the scalars once; a skipped step stores nothing
#define PM_ADAM_GUARD(status)                                                                         \
  __shared__ unsigned sh[3];                                                                          \
  if (threadIdx.x == 0) {                                                                             \
    sh[0] = status[PM_OVF_LAST]; sh[1] = status[PM_OVF_STEP_SIZE]; sh[2] = status[PM_OVF_INV_BC2];    \
  }                                                                                                   \
  __syncthreads();                                                                                    \
  if (sh[0]) return;                                                                                  \
  const float step_size = __uint_as_float(sh[1]), inv_bc2_sqrt = __uint_as_float(sh[2]);
__global__ void __launch_bounds__(256) k_adam4_guarded(float4* __restrict__ p, const float4* __restrict__ g,
                                                       float4* __restrict__ m, float4* __restrict__ v, int64_t n4, float b1,
                                                       float b2, const unsigned* __restrict__ status, float eps,
                                                       float gscale) {
  PM_ADAM_GUARD(status)
  PM_ADAM4_LOOP
}
__global__ void __launch_bounds__(256) k_adam1_guarded(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n, float b1,
                                                       float b2, const unsigned* __restrict__ status, float eps,
                                                       float gscale) {
  PM_ADAM_GUARD(status)
  PM_ADAM1_LOOP
}
#undef PM_ADAM_GUARD
// ---- Adam with the gradient scale read from the clip block (pm_grad_clip_finish wrote it).  GUARD: behind the decision of the
// check, as k_adam*_guarded; otherwise the scalars come from the host, as in k_adam*.  Thread 0 reads the block once
// thread 0 reads gscale (with coef == 1 it is grad_scale: the step is then bit-identical to pm_adam_step / _guarded) and, GUARD, the
// decision and its scalars once; a skipped step stores nothing
#define PM_ADAM_CLIP_PROLOGUE(clip, status) \
  __shared__ unsigned sh[4]; \
  if (threadIdx.x == 0) { \
    sh[3] = __float_as_uint((float)clip[PM_CLIP_GSCALE]); \
    if (GUARD) { sh[0] = status[PM_OVF_LAST]; sh[1] = status[PM_OVF_STEP_SIZE]; sh[2] = status[PM_OVF_INV_BC2]; } \
  } \
  __syncthreads(); \
  if (GUARD && sh[0]) return; \
  const float step_size = GUARD ? __uint_as_float(sh[1]) : step_size_h; \
  const float inv_bc2_sqrt = GUARD ? __uint_as_float(sh[2]) : inv_bc2_sqrt_h; \
  const float gscale = __uint_as_float(sh[3]);
template <bool GUARD>
__global__ void __launch_bounds__(256) k_adam4_clipped(float4* __restrict__ p, const float4* __restrict__ g,
                                                       float4* __restrict__ m, float4* __restrict__ v, int64_t n4, float b1,
                                                       float b2, float step_size_h, float inv_bc2_sqrt_h, float eps,
                                                       const double* __restrict__ clip, const unsigned* __restrict__ status) {
  PM_ADAM_CLIP_PROLOGUE(clip, status)
  PM_ADAM4_LOOP
}
template <bool GUARD>
__global__ void __launch_bounds__(256) k_adam1_clipped(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n, float b1,
                                                       float b2, float step_size_h, float inv_bc2_sqrt_h, float eps,
                                                       const double* __restrict__ clip, const unsigned* __restrict__ status) {
  PM_ADAM_CLIP_PROLOGUE(clip, status)
  PM_ADAM1_LOOP
}
#undef PM_ADAM_CLIP_PROLOGUE
#undef PM_ADAM4_LOOP
#undef PM_ADAM1_LOOP
__global__ void k_adam_bias_scalars(const int64_t* __restrict__ steps, int64_t n, float lr, float beta1, float beta2,
                                    float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    adam_bias_scalars(steps[i], lr, beta1, beta2, out[2 * i], out[2 * i + 1]);
}
extern "C" int pm_grad_nonfinite_check(const float* grads, int64_t n, uint32_t* status, int64_t* step, int64_t* skipped,
                                       float lr, float beta1, float beta2, int32_t window, pm_stream_t stream) {
  if (!grads || !status || n <= 0 || (step && !skipped)) return PM_E_INVALID;
  NonfiniteDecision d{step, skipped, nullptr, lr, beta1, beta2};
  if (step && window) {
    d.clamp = pm_h2_clamp_word_ready();
    if (!d.clamp) return PM_E_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  // (grid <= 256 < 2^16: the two counts of the decision word cannot overflow into each other)
  if (!((uintptr_t)grads & 15) && (n % 4) == 0) {
    int64_t nb = pm_cdiv(n / 4, kCheckThreads); if (nb > kCheckBlocks) nb = kCheckBlocks;
    hipLaunchKernelGGL(k_nonfinite4, dim3((unsigned)nb), dim3(kCheckThreads), 0, st, reinterpret_cast<const uint4*>(grads),
                       n / 4, status, d);
  } else {
    int64_t nb = pm_cdiv(n, kCheckThreads); if (nb > kCheckBlocks) nb = kCheckBlocks;
    hipLaunchKernelGGL(k_nonfinite1, dim3((unsigned)nb), dim3(kCheckThreads), 0, st, reinterpret_cast<const unsigned*>(grads),
                       n, status, d);
  }
  return pm_check_launch();
}
extern "C" int pm_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                    float beta1, float beta2, float eps, float grad_scale, const uint32_t* status,
                                    pm_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !status || n <= 0) return PM_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const bool al = !(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15);
  if (al && (n % 4) == 0) {
    int64_t nb = pm_cdiv(n / 4, 256); if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_adam4_guarded, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<float4*>(params),
                       reinterpret_cast<const float4*>(grads), reinterpret_cast<float4*>(exp_avg),
                       reinterpret_cast<float4*>(exp_avg_sq), n / 4, beta1, beta2, status, eps, grad_scale);
  } else {
    int64_t nb = pm_cdiv(n, 256); if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_adam1_guarded, dim3((unsigned)nb), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n,
                       beta1, beta2, status, eps, grad_scale);
  }
  return pm_check_launch();
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
template <typename K4, typename K1, typename... A>
static inline void launch_grad_pass(K4 k4, K1 k1, const float* grads, int64_t n, hipStream_t st, A... a) {
  if (!((uintptr_t)grads & 15) && (n % 4) == 0) {
    int64_t nb = pm_cdiv(n / 4, kCheckThreads); if (nb > kCheckBlocks) nb = kCheckBlocks;
    hipLaunchKernelGGL(k4, dim3((unsigned)nb), dim3(kCheckThreads), 0, st, reinterpret_cast<const uint4*>(grads), n / 4, a...);
  } else {
    int64_t nb = pm_cdiv(n, kCheckThreads); if (nb > kCheckBlocks) nb = kCheckBlocks;
    hipLaunchKernelGGL(k1, dim3((unsigned)nb), dim3(kCheckThreads), 0, st, reinterpret_cast<const unsigned*>(grads), n, a...);
  }
}
extern "C" int pm_grad_sumsq(const float* grads, int64_t n, double* clip, pm_stream_t stream) {
  if (!grads || !clip || n <= 0 || ((uintptr_t)clip & 7)) return PM_E_INVALID;
  launch_grad_pass(k_grad_sumsq4, k_grad_sumsq1, grads, n, (hipStream_t)stream, clip);
  return pm_check_launch();
}
extern "C" int pm_grad_nonfinite_check_sumsq(const float* grads, int64_t n, uint32_t* status, int64_t* step, int64_t* skipped,
                                             float lr, float beta1, float beta2, int32_t window, double* clip,
                                             pm_stream_t stream) {
  if (!grads || !status || !clip || n <= 0 || (step && !skipped) || ((uintptr_t)clip & 7)) return PM_E_INVALID;
  NonfiniteDecision d{step, skipped, nullptr, lr, beta1, beta2};
  if (step && window) {
    d.clamp = pm_h2_clamp_word_ready();
    if (!d.clamp) return PM_E_INVALID;
  }
  launch_grad_pass(k_nonfinite4_sumsq, k_nonfinite1_sumsq, grads, n, (hipStream_t)stream, status, d, clip);
  return pm_check_launch();
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
  float step_size = 0.f, inv_bc2_sqrt = 0.f;
  if (!status) {                                  // (pm_adam_step's host scalars; guarded: the decision's, from the device)
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    step_size = (float)((double)lr / bc1);
    inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  }
  hipStream_t st = (hipStream_t)stream;
  const bool al = !(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15);
  if (al && (n % 4) == 0) {
    int64_t nb = pm_cdiv(n / 4, 256); if (nb > 4096) nb = 4096;
    auto k = status ? k_adam4_clipped<true> : k_adam4_clipped<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<float4*>(params),
                       reinterpret_cast<const float4*>(grads), reinterpret_cast<float4*>(exp_avg),
                       reinterpret_cast<float4*>(exp_avg_sq), n / 4, beta1, beta2, step_size, inv_bc2_sqrt, eps, clip, status);
  } else {
    int64_t nb = pm_cdiv(n, 256); if (nb > 4096) nb = 4096;
    auto k = status ? k_adam1_clipped<true> : k_adam1_clipped<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, step_size,
                       inv_bc2_sqrt, eps, clip, status);
  }
  return pm_check_launch();
}

extern "C" int pm_abi_version(void) { return PM_ABI_VERSION; }
extern "C" const char* pm_build_info(void) { return "polyphemus_hip gfx950 (CDNA4) fp32-MFMA build " __DATE__; }

// cnn.hip — structure encoder / decoder convolutions over 4x32 bar grids (NCHW, 3x3, padding 1).
//
// Reference: CNNEncoder.conv / CNNDecoder.conv (model.py:219-230,279-285) = conv2d, max_pool2d((1,4)),
// upsample_nearest2d(scale (1,4)).  ~0.4 MFLOP per bar, a bar's whole CNN state a few KB.  Two kernel sets:
//   * generic direct convolutions, pool and (norm.hip) [O, C, I] BatchNorm: one thread per output element, any
//     shape; 9-10 launches per direction of the model's CNNs.  Eval mode, generation, models without norms, the
//     structure decoder's backward and the Python engine run on these.  `up4` folds the nearest-neighbour
//     upsample into the convolution's reads.
//   * the training step's chains of the model's FIXED shapes with norms on (second half of this file): a workgroup
//     keeps its bars in LDS, the weights are staged once per workgroup, extents are compile-time and indices
//     32-bit.  Training-mode BatchNorm2d needs statistics over all bars, which is the only launch boundary left:
//     structure encoder forward 3 launches (9 before), decoder forward 2 (5), encoder backward 4 (10).  The chains
//     were launch-latency bound (24 launches of 5-50 us for ~100 MMAC), this is what the fused set answers.
#include "common.h"

__global__ void __launch_bounds__(256) k_conv3x3_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ b, int G, int Ci, int Co, int H, int W,
                                                     int up4, float* __restrict__ y) {
  const int64_t total = (int64_t)G * Co * H * W;
  const int Win = up4 ? W / 4 : W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int wq = (int)(i % W), h = (int)((i / W) % H), co = (int)((i / ((int64_t)W * H)) % Co);
    const int g = (int)(i / ((int64_t)W * H * Co));
    float acc = b ? b[co] : 0.f;
    for (int ci = 0; ci < Ci; ++ci) {
      const float* xp = x + ((int64_t)g * Ci + ci) * H * Win;
      const float* wp = w + ((int64_t)co * Ci + ci) * 9;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hh = h + kh - 1;
        if (hh < 0 || hh >= H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = wq + kw - 1;
          if (ww < 0 || ww >= W) continue;
          acc += xp[hh * Win + (up4 ? ww >> 2 : ww)] * wp[kh * 3 + kw];
        }
      }
    }
    y[i] = acc;
  }
}
// dx (w.r.t. the convolution input, before the optional upsample)
__global__ void __launch_bounds__(256) k_conv3x3_bwd_data(const float* __restrict__ dy, const float* __restrict__ w,
                                                          int G, int Ci, int Co, int H, int W, int up4,
                                                          float* __restrict__ dx) {
  const int Win = up4 ? W / 4 : W;
  const int64_t total = (int64_t)G * Ci * H * Win;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int wi = (int)(i % Win), h = (int)((i / Win) % H), ci = (int)((i / ((int64_t)Win * H)) % Ci);
    const int g = (int)(i / ((int64_t)Win * H * Ci));
    float acc = 0.f;
    const int rep = up4 ? 4 : 1;
    for (int u = 0; u < rep; ++u) {
      const int wq = up4 ? wi * 4 + u : wi;
      for (int co = 0; co < Co; ++co) {
        const float* dp = dy + ((int64_t)g * Co + co) * H * W;
        const float* wp = w + ((int64_t)co * Ci + ci) * 9;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int hh = h - kh + 1;
          if (hh < 0 || hh >= H) continue;
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int ww = wq - kw + 1;
            if (ww < 0 || ww >= W) continue;
            acc += dp[hh * W + ww] * wp[kh * 3 + kw];
          }
        }
      }
    }
    dx[i] = acc;
  }
}
// grid = (co*ci, g-chunks): dw[co,ci,:,:] += sum_{g,h,w} dy * x_shifted ; db[co] += sum dy (ci == 0).
// Each workgroup reduces a slice of the bars in fp64 and adds its 9 (+1) partials with float atomics.
__global__ void __launch_bounds__(256) k_conv3x3_bwd_weight(const float* __restrict__ x, const float* __restrict__ dy,
                                                            int G, int Ci, int Co, int H, int W, int up4, float* dw,
                                                            float* db, unsigned* gate) {
  __shared__ double sh[4][10];
  const int co = blockIdx.x / Ci, ci = blockIdx.x % Ci;
  const int Win = up4 ? W / 4 : W;
  double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int gper = (G + gridDim.y - 1) / gridDim.y;
  const int g0 = blockIdx.y * gper, g1 = min(G, g0 + gper);
  const int64_t total = (int64_t)(g1 - g0) * H * W;
  for (int64_t i = threadIdx.x; i < total; i += blockDim.x) {
    const int wq = (int)(i % W), h = (int)((i / W) % H), g = g0 + (int)(i / ((int64_t)W * H));
    const float d = dy[((int64_t)g * Co + co) * H * W + h * W + wq];
    const float* xp = x + ((int64_t)g * Ci + ci) * H * Win;
    acc[9] += d;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int hh = h + kh - 1;
      if (hh < 0 || hh >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ww = wq + kw - 1;
        if (ww < 0 || ww >= W) continue;
        acc[kh * 3 + kw] += (double)d * (double)xp[hh * Win + (up4 ? ww >> 2 : ww)];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    const double s = pm_wave_sum_d(acc[j]);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][j] = s;
  }
  __syncthreads();
  pm_turn_enter_block(gate);                    // (deterministic mode, common.h: the bar slices add in turn)
  if (threadIdx.x < 10) {
    const double s = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (threadIdx.x < 9) atomicAdd(&dw[((int64_t)co * Ci + ci) * 9 + threadIdx.x], (float)s);
    else if (ci == 0 && db) atomicAdd(&db[co], (float)s);
  }
  pm_turn_leave_block(gate);
}
static inline int cgrid(int64_t n) { int64_t g = pm_cdiv(n, 256); return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g)); }

extern "C" int pm_conv3x3_fwd(const float* x, const float* w, const float* b, int32_t G, int32_t Ci, int32_t Co,
                              int32_t H, int32_t W, int up4, float* y, pm_stream_t stream) {
  if (!x || !w || !y || G <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0 || (up4 && (W & 3))) return PM_E_INVALID;
  hipLaunchKernelGGL(k_conv3x3_fwd, dim3(cgrid((int64_t)G * Co * H * W)), dim3(256), 0, (hipStream_t)stream, x, w, b, G,
                     Ci, Co, H, W, up4, y);
  return pm_check_launch();
}
extern "C" int pm_conv3x3_bwd_data(const float* dy, const float* w, int32_t G, int32_t Ci, int32_t Co, int32_t H,
                                   int32_t W, int up4, float* dx, pm_stream_t stream) {
  if (!dy || !w || !dx || G <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0 || (up4 && (W & 3))) return PM_E_INVALID;
  hipLaunchKernelGGL(k_conv3x3_bwd_data, dim3(cgrid((int64_t)G * Ci * H * (up4 ? W / 4 : W))), dim3(256), 0,
                     (hipStream_t)stream, dy, w, G, Ci, Co, H, W, up4, dx);
  return pm_check_launch();
}
extern "C" int pm_conv3x3_bwd_weight(const float* x, const float* dy, int32_t G, int32_t Ci, int32_t Co, int32_t H,
                                     int32_t W, int up4, float* dw, float* db, pm_stream_t stream) {
  if (!x || !dy || !dw || G <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0 || (up4 && (W & 3))) return PM_E_INVALID;
  int chunks = (int)pm_cdiv(1024, Co * Ci);                       // ~1k workgroups in total
  if (chunks > G) chunks = G;
  if (chunks < 1) chunks = 1;
  hipLaunchKernelGGL(k_conv3x3_bwd_weight, dim3(Co * Ci, chunks), dim3(256), 0, (hipStream_t)stream, x, dy, G, Ci, Co,
                     H, W, up4, dw, db, pm_det_gate((hipStream_t)stream));
  return pm_check_launch();
}

// MaxPool2d((1,4), stride (1,4)): the pooled axis is the innermost one, so it is a flat 4 -> 1 max.
__global__ void k_maxpool4_fwd(const float* __restrict__ x, int64_t n_out, float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    y[i] = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
  }
}
__global__ void k_maxpool4_bwd(const float* __restrict__ x, const float* __restrict__ dy, int64_t n_out,
                               float* __restrict__ dx) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    int k = 0; float m = v.x;                                    // first maximum wins (ATen max_pool2d)
    if (v.y > m) { m = v.y; k = 1; }
    if (v.z > m) { m = v.z; k = 2; }
    if (v.w > m) { m = v.w; k = 3; }
    const float d = dy[i];
    reinterpret_cast<float4*>(dx)[i] = make_float4(k == 0 ? d : 0.f, k == 1 ? d : 0.f, k == 2 ? d : 0.f, k == 3 ? d : 0.f);
  }
}
extern "C" int pm_maxpool4_fwd(const float* x, int64_t n_out, float* y, pm_stream_t stream) {
  if (!x || !y || n_out <= 0 || ((uintptr_t)x & 15)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_maxpool4_fwd, dim3(cgrid(n_out)), dim3(256), 0, (hipStream_t)stream, x, n_out, y);
  return pm_check_launch();
}
extern "C" int pm_maxpool4_bwd(const float* x, const float* dy, int64_t n_out, float* dx, pm_stream_t stream) {
  if (!x || !dy || !dx || n_out <= 0 || ((uintptr_t)x & 15) || ((uintptr_t)dx & 15)) return PM_E_INVALID;
  hipLaunchKernelGGL(k_maxpool4_bwd, dim3(cgrid(n_out)), dim3(256), 0, (hipStream_t)stream, x, dy, n_out, dx);
  return pm_check_launch();
}

// ---- the model's CNN chains, bar resident (model.py:219-230, 279-285 with BatchNorm2d in training mode) -------------------
// Shapes: s [G,1,4,32] -conv0-> c0 [G,8,4,32] -BN1,ReLU-> a0 -pool(1,4)-> p0 [G,8,4,8] -conv4-> c1 [G,16,4,8] -BN5,ReLU-> a1;
//         u2 [G,16,4,8] -up(1,4),conv1-> c2 [G,8,4,32] -BN2,ReLU-> a2 -conv4-> s_logits [G,1,4,32].
// Every kernel runs 256 threads and walks bars g = blockIdx.x, blockIdx.x + gridDim.x, ..  A convolution adds in the order of
// k_conv3x3_fwd (bias, then ci outer, kh, kw inner, out-of-range taps skipped), so on the same input its output has the same bits.
// Batch statistics: every workgroup of a producer leaves fp64 partial sums in ITS slot of the caller's scratch
// (partial[slot][NV], plain stores, no atomics); every workgroup of the consumer adds all slots in one fixed order
// (cnn_sum_slots) and forms the norm's constants itself — the same bits in every workgroup, run and mode.  Workgroup 0 of the
// consumer writes mean / var / running statistics (as k_bn_finalize_stats) or dgamma / dbeta (as k_bn_finalize_bwd).
constexpr int kCnnThreads = 256;
constexpr int kCnnMaxSlots = 256;                    // workgroups per launch at most (= slots of the scratch used)
constexpr int kCnnEncFwdSlot = 16 + 32;              // doubles per slot: {sum, sum^2} of c0's 8 and of c1's 16 channels
constexpr int kCnnDecFwdSlot = 16;                   // ... of c2's 8 channels
// backward slot: {sum du, sum du*xhat} of BN5's 16 channels | of BN1's 8 channels | conv4's dw [1152], db [16] | conv0's [8]{dw[9], db}
constexpr int kBwdBn1 = 32, kBwdDw4 = kBwdBn1 + 16, kBwdDw0 = kBwdDw4 + 1168, kCnnEncBwdSlot = kBwdDw0 + 80;

// out[v] (LDS) = sum over k < nslot of partial[k * STRIDE + v], v < NV: sixteen threads per value take slots j, j + 16, .. in order
// and meet in a fixed butterfly.  Ends with a barrier.
template <int NV, int STRIDE>
__device__ static inline void cnn_sum_slots(const double* __restrict__ partial, int nslot, double* out) {
  const int j = threadIdx.x & 15;
  for (int v = threadIdx.x >> 4; v < NV; v += kCnnThreads / 16) {
    double s = 0;
    for (int k = j; k < nslot; k += 16) s += partial[k * STRIDE + v];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    if (j == 0) out[v] = s;
  }
  __syncthreads();
}
// sum over the 32 lanes of a half wave (every lane gets it)
__device__ static inline double cnn_half_sum_d(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// Training-mode constants of channel c from its sums {sum x, sum x^2} (sums[c], sums[C + c]), as k_bn_finalize_stats forms
// them; bn = [4][C] floats in LDS: mean, rsqrt(var + eps), gamma, beta.  `writer`: save mean / var, update the running statistics.
template <int C>
__device__ static inline void cnn_bn_consts(const double* sums, int c, double count, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float eps, float momentum, bool writer,
                                            float* mean, float* var, float* rmean, float* rvar, float* bn) {
  const double mu = sums[c] / count;
  double v = sums[C + c] / count - mu * mu;
  if (v < 0) v = 0;
  const float mf = (float)mu, vf = (float)v;
  bn[c] = mf; bn[C + c] = rsqrtf(vf + eps); bn[2 * C + c] = gamma[c]; bn[3 * C + c] = beta[c];
  if (writer) {
    mean[c] = mf; var[c] = vf;
    if (rmean) {
      const double unb = count > 1 ? v * count / (count - 1) : v;
      rmean[c] = (float)((1.0 - momentum) * rmean[c] + momentum * mu);
      rvar[c] = (float)((1.0 - momentum) * rvar[c] + momentum * unb);
    }
  }
}
// BatchNorm + ReLU of one element, the expression of k_bn_apply1
template <int C>
__device__ static inline float cnn_bn_relu(float x, const float* bn, int c) {
  return fmaxf((x - bn[c]) * bn[C + c] * bn[2 * C + c] + bn[3 * C + c], 0.f);
}

// encoder 1/3: c0 = conv0(s) and the sums of c0.  Thread = (position, 4 of the 8 output channels).
__global__ void __launch_bounds__(kCnnThreads) k_cnn_enc_conv0(const float* __restrict__ s, const float* __restrict__ w,
                                                               const float* __restrict__ b, int G, float* __restrict__ c0,
                                                               double* __restrict__ partial) {
  __shared__ float xs[128];
  __shared__ float ws[80];                                       // [8][9] weights, [8] bias
  __shared__ double red[4][8];
  const int t = threadIdx.x, pos = t & 127, h = pos >> 5, wq = pos & 31, cg = t >> 7;
  if (t < 72) ws[t] = w[t];
  else if (t < 80) ws[t] = b[t - 72];
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    __syncthreads();
    if (t < 128) xs[t] = s[g * 128 + t];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = cg * 4 + j;
      float acc = ws[72 + co];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hh = h + kh - 1;
        if (hh < 0 || hh >= 4) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = wq + kw - 1;
          if (ww < 0 || ww >= 32) continue;
          acc += xs[hh * 32 + ww] * ws[co * 9 + kh * 3 + kw];
        }
      }
      c0[(g * 8 + co) * 128 + pos] = acc;
      s1[j] += (double)acc; s2[j] += (double)acc * (double)acc;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double a = pm_wave_sum_d(s1[j]), q = pm_wave_sum_d(s2[j]);
    if ((t & 63) == 0) { red[t >> 6][j] = a; red[t >> 6][4 + j] = q; }
  }
  __syncthreads();
  if (t < 16) {                                                  // t = a * 8 + channel; waves 2 cg, 2 cg + 1 hold channel group cg
    const int a = t >> 3, c = t & 7, wv = (c >> 2) * 2, j = a * 4 + (c & 3);
    partial[blockIdx.x * kCnnEncFwdSlot + t] = red[wv][j] + red[wv + 1][j];
  }
}
// encoder 2/3: BN1 + ReLU -> a0, pool -> p0, conv4 -> c1 and the sums of c1.  First phase: thread = pooled element (4 of
// c0 / a0); second phase: thread = (position of the 4x8 grid, 2 of the 16 output channels).
__global__ void __launch_bounds__(kCnnThreads) k_cnn_enc_mid(const float* __restrict__ c0, const double* __restrict__ partial_in,
                                                             int nslot, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ w, const float* __restrict__ b, int G, float eps,
                                                             float momentum, float* __restrict__ a0, float* __restrict__ p0,
                                                             float* __restrict__ c1, float* mean, float* var, float* rmean, float* rvar,
                                                             double* __restrict__ partial_out) {
  __shared__ double sums[16];
  __shared__ float bn[4 * 8];
  __shared__ float ws[16 * 8 * 9 + 16];
  __shared__ float ps[256];
  const int t = threadIdx.x;
  cnn_sum_slots<16, kCnnEncFwdSlot>(partial_in, nslot, sums);
  if (t < 8) cnn_bn_consts<8>(sums, t, (double)G * 128.0, gamma, beta, eps, momentum, blockIdx.x == 0, mean, var, rmean, rvar, bn);
  for (int i = t; i < 1152; i += kCnnThreads) ws[i] = w[i];
  if (t < 16) ws[1152 + t] = b[t];
  const int pos = t & 31, h = pos >> 3, wq = pos & 7, cg = t >> 5, ch = t >> 5;
  double s1[2] = {0, 0}, s2[2] = {0, 0};
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    __syncthreads();
    const float4 x = reinterpret_cast<const float4*>(c0)[g * 256 + t];
    const float4 y = make_float4(cnn_bn_relu<8>(x.x, bn, ch), cnn_bn_relu<8>(x.y, bn, ch), cnn_bn_relu<8>(x.z, bn, ch),
                                 cnn_bn_relu<8>(x.w, bn, ch));
    reinterpret_cast<float4*>(a0)[g * 256 + t] = y;
    const float m = fmaxf(fmaxf(y.x, y.y), fmaxf(y.z, y.w));
    ps[t] = m;
    p0[g * 256 + t] = m;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int co = cg * 2 + j;
      float acc = ws[1152 + co];
      for (int ci = 0; ci < 8; ++ci) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int hh = h + kh - 1;
          if (hh < 0 || hh >= 4) continue;
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int ww = wq + kw - 1;
            if (ww < 0 || ww >= 8) continue;
            acc += ps[ci * 32 + hh * 8 + ww] * ws[(co * 8 + ci) * 9 + kh * 3 + kw];
          }
        }
      }
      c1[(g * 16 + co) * 32 + pos] = acc;
      s1[j] += (double)acc; s2[j] += (double)acc * (double)acc;
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double a = cnn_half_sum_d(s1[j]), q = cnn_half_sum_d(s2[j]);
    if (pos == 0) {
      partial_out[blockIdx.x * kCnnEncFwdSlot + 16 + cg * 2 + j] = a;
      partial_out[blockIdx.x * kCnnEncFwdSlot + 32 + cg * 2 + j] = q;
    }
  }
}
// encoder 3/3: BN5 + ReLU -> a1
__global__ void __launch_bounds__(kCnnThreads) k_cnn_enc_out(const float* __restrict__ c1, const double* __restrict__ partial_in,
                                                             int nslot, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             int G, float eps, float momentum, float* __restrict__ a1, float* mean,
                                                             float* var, float* rmean, float* rvar) {
  __shared__ double sums[32];
  __shared__ float bn[4 * 16];
  const int t = threadIdx.x;
  cnn_sum_slots<32, kCnnEncFwdSlot>(partial_in, nslot, sums);
  if (t < 16) cnn_bn_consts<16>(sums, t, (double)G * 32.0, gamma, beta, eps, momentum, blockIdx.x == 0, mean, var, rmean, rvar, bn);
  __syncthreads();
  const int n4 = G * 128;                                        // float4 of [G,16,32]: 8 per channel plane
  for (int i = blockIdx.x * kCnnThreads + t; i < n4; i += gridDim.x * kCnnThreads) {
    const int ch = (i >> 3) & 15;
    const float4 x = reinterpret_cast<const float4*>(c1)[i];
    reinterpret_cast<float4*>(a1)[i] = make_float4(cnn_bn_relu<16>(x.x, bn, ch), cnn_bn_relu<16>(x.y, bn, ch),
                                                   cnn_bn_relu<16>(x.z, bn, ch), cnn_bn_relu<16>(x.w, bn, ch));
  }
}

// decoder 1/2: c2 = conv1(upsample(u2)) and the sums of c2.  Thread = (position of the 4x32 grid, 4 of the 8 output channels).
__global__ void __launch_bounds__(kCnnThreads) k_cnn_dec_conv1(const float* __restrict__ u2, const float* __restrict__ w,
                                                               const float* __restrict__ b, int G, float* __restrict__ c2,
                                                               double* __restrict__ partial) {
  __shared__ float us[512];
  __shared__ float ws[8 * 16 * 9 + 8];
  __shared__ double red[4][8];
  const int t = threadIdx.x, pos = t & 127, h = pos >> 5, wq = pos & 31, cg = t >> 7;
  for (int i = t; i < 1152; i += kCnnThreads) ws[i] = w[i];
  if (t < 8) ws[1152 + t] = b[t];
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    __syncthreads();
    us[t] = u2[g * 512 + t]; us[t + 256] = u2[g * 512 + 256 + t];
    __syncthreads();
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = ws[1152 + cg * 4 + j];
    for (int ci = 0; ci < 16; ++ci) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hh = h + kh - 1;
        if (hh < 0 || hh >= 4) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = wq + kw - 1;
          if (ww < 0 || ww >= 32) continue;
          const float x = us[ci * 32 + hh * 8 + (ww >> 2)];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] += x * ws[((cg * 4 + j) * 16 + ci) * 9 + kh * 3 + kw];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c2[(g * 8 + cg * 4 + j) * 128 + pos] = acc[j];
      s1[j] += (double)acc[j]; s2[j] += (double)acc[j] * (double)acc[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double a = pm_wave_sum_d(s1[j]), q = pm_wave_sum_d(s2[j]);
    if ((t & 63) == 0) { red[t >> 6][j] = a; red[t >> 6][4 + j] = q; }
  }
  __syncthreads();
  if (t < 16) {
    const int a = t >> 3, c = t & 7, wv = (c >> 2) * 2, j = a * 4 + (c & 3);
    partial[blockIdx.x * kCnnDecFwdSlot + t] = red[wv][j] + red[wv + 1][j];
  }
}
// decoder 2/2: BN2 + ReLU -> a2, conv4 -> s_logits.  First phase: thread = 4 elements of c2 / a2; second: thread < 128 = position.
__global__ void __launch_bounds__(kCnnThreads) k_cnn_dec_out(const float* __restrict__ c2, const double* __restrict__ partial_in,
                                                             int nslot, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ w, const float* __restrict__ b, int G, float eps,
                                                             float momentum, float* __restrict__ a2, float* __restrict__ s_logits,
                                                             float* mean, float* var, float* rmean, float* rvar) {
  __shared__ double sums[16];
  __shared__ float bn[4 * 8];
  __shared__ float ws[73];
  __shared__ float as[1024];
  const int t = threadIdx.x, ch = t >> 5;
  cnn_sum_slots<16, kCnnDecFwdSlot>(partial_in, nslot, sums);
  if (t < 8) cnn_bn_consts<8>(sums, t, (double)G * 128.0, gamma, beta, eps, momentum, blockIdx.x == 0, mean, var, rmean, rvar, bn);
  if (t < 72) ws[t] = w[t];
  else if (t == 72) ws[72] = b[0];
  const int h = (t & 127) >> 5, wq = t & 31;
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    __syncthreads();
    const float4 x = reinterpret_cast<const float4*>(c2)[g * 256 + t];
    const float4 y = make_float4(cnn_bn_relu<8>(x.x, bn, ch), cnn_bn_relu<8>(x.y, bn, ch), cnn_bn_relu<8>(x.z, bn, ch),
                                 cnn_bn_relu<8>(x.w, bn, ch));
    reinterpret_cast<float4*>(a2)[g * 256 + t] = y;
    reinterpret_cast<float4*>(as)[t] = y;
    __syncthreads();
    if (t < 128) {
      float acc = ws[72];
      for (int ci = 0; ci < 8; ++ci) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int hh = h + kh - 1;
          if (hh < 0 || hh >= 4) continue;
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int ww = wq + kw - 1;
            if (ww < 0 || ww >= 32) continue;
            acc += as[ci * 128 + hh * 32 + ww] * ws[ci * 9 + kh * 3 + kw];
          }
        }
      }
      s_logits[g * 128 + t] = acc;
    }
  }
}

// One element of the norm's backward: xhat and du = dy * [BN(x) > 0] (bn_acc<1> / k_bn_bwd_apply of norm.hip)
template <int C>
__device__ static inline void cnn_bn_du(float x, float dy, const float* bn, int c, float& xh, float& du) {
  xh = (x - bn[c]) * bn[C + c];
  du = (xh * bn[2 * C + c] + bn[3 * C + c] > 0.f) ? dy : 0.f;
}
template <int C>
__device__ static inline void cnn_bn_saved(int c, const float* __restrict__ mean, const float* __restrict__ var,
                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float* bn) {
  bn[c] = mean[c]; bn[C + c] = rsqrtf(var[c] + eps); bn[2 * C + c] = gamma[c]; bn[3 * C + c] = beta[c];
}
// encoder backward 1/4: the two BN5-backward sums (du, du * xhat) over da1 and c1 [G,16,32].  Thread = elements t, t + 256 of a bar.
__global__ void __launch_bounds__(kCnnThreads) k_cnn_enc_bwd_sums(const float* __restrict__ c1, const float* __restrict__ da1,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  int G, float eps, double* __restrict__ partial) {
  __shared__ float bn[4 * 16];
  const int t = threadIdx.x;
  if (t < 16) cnn_bn_saved<16>(t, mean, var, gamma, beta, eps, bn);
  __syncthreads();
  double acc[2][2] = {{0, 0}, {0, 0}};
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = j * 256 + t;
      float xh, du;
      cnn_bn_du<16>(c1[g * 512 + e], da1[g * 512 + e], bn, e >> 5, xh, du);
      acc[j][0] += (double)du; acc[j][1] += (double)du * (double)xh;
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const double v = cnn_half_sum_d(acc[j][a]);
      if ((t & 31) == 0) partial[blockIdx.x * kCnnEncBwdSlot + a * 16 + j * 8 + (t >> 5)] = v;
    }
}
// encoder backward 2/4: BN5 backward -> dc1 (LDS), conv4's weight / bias gradient, conv4's data gradient, pool backward -> da0
// and the two BN1-backward sums.  Weight gradient: thread = outputs t, t + 256, .. of the 1152; threads 128..143 also a bias;
// fp64 over the workgroup's bars, left in its slot like the statistics and added up by the next launch — one rounding to fp32
// per element and no atomics (k_conv3x3_bwd_weight adds 8 fp32 partials per element; up to 256 here would cost it accuracy and
// the same-address atomics disturb the GCL kernels' own beside it).  p0 sits in LDS with a zero halo, so every output walks all
// 32 positions with compile-time offsets (an out-of-range tap adds dc * 0).
__global__ void __launch_bounds__(kCnnThreads) k_cnn_enc_bwd_mid(
    const float* __restrict__ c1, const float* __restrict__ da1, const float* __restrict__ p0, const float* __restrict__ a0,
    const float* __restrict__ c0, const float* __restrict__ mean5, const float* __restrict__ var5, const float* __restrict__ gamma5,
    const float* __restrict__ beta5, const float* __restrict__ mean1, const float* __restrict__ var1, const float* __restrict__ gamma1,
    const float* __restrict__ beta1, const float* __restrict__ w, const double* __restrict__ partial_in, int nslot, int G, float eps,
    float* dgamma5, float* dbeta5, float* __restrict__ dc1_out, float* __restrict__ da0, double* __restrict__ partial_out) {
  __shared__ double sums[32];
  __shared__ float bn5[4 * 16], mb5[2 * 16], bn1[4 * 8];
  __shared__ float ws[1152], dcs[512], pp[8 * 60];                 // pp: p0 as [8][4 + 2][8 + 2], zero halo
  const int t = threadIdx.x;
  cnn_sum_slots<32, kCnnEncBwdSlot>(partial_in, nslot, sums);
  if (t < 16) {
    cnn_bn_saved<16>(t, mean5, var5, gamma5, beta5, eps, bn5);
    const double count = (double)G * 32.0;
    mb5[t] = (float)(sums[t] / count); mb5[16 + t] = (float)(sums[16 + t] / count);
    if (blockIdx.x == 0) { dbeta5[t] += (float)sums[t]; dgamma5[t] += (float)sums[16 + t]; }
  } else if (t >= 64 && t < 72) cnn_bn_saved<8>(t - 64, mean1, var1, gamma1, beta1, eps, bn1);
  for (int i = t; i < 1152; i += kCnnThreads) ws[i] = w[i];
  for (int i = t; i < 8 * 60; i += kCnnThreads) pp[i] = 0.f;
  // weight-gradient outputs of this thread: o = t + 256 j -> (co, ci, kh, kw) -> its offsets into dcs and pp
  int o_dc[5], o_p[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int o = t + 256 * j, oo = o < 1152 ? o : 0;
    const int co = oo / 72, ci = (oo / 9) % 8, kh = (oo % 9) / 3, kw = oo % 3;
    o_dc[j] = co * 32; o_p[j] = ci * 60 + kh * 10 + kw;
  }
  double gw[5] = {0, 0, 0, 0, 0}, gb = 0;
  double acc[2] = {0, 0};
  const int ch = t >> 5, h = (t >> 3) & 3, wq = t & 7;
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = j * 256 + t, c = e >> 5;
      float xh, du;
      cnn_bn_du<16>(c1[g * 512 + e], da1[g * 512 + e], bn5, c, xh, du);
      const float dc = bn5[32 + c] * bn5[16 + c] * (du - mb5[c] - xh * mb5[16 + c]);
      dcs[e] = dc;
      if (dc1_out) dc1_out[g * 512 + e] = dc;
    }
    pp[ch * 60 + (h + 1) * 10 + wq + 1] = p0[g * 256 + t];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (t + 256 * j >= 1152) continue;                           // (j = 4: waves 2, 3 have no output)
#pragma unroll
      for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x)
          gw[j] += (double)dcs[o_dc[j] + y * 8 + x] * (double)pp[o_p[j] + y * 10 + x];
    }
    if (t >= 128 && t < 144)
      for (int i = 0; i < 32; ++i) gb += (double)dcs[(t - 128) * 32 + i];
    // dp0[ci = ch, h, wq] (thread = pooled element t), then the pool's backward over the four a0 it came from
    float dp = 0.f;
    for (int co = 0; co < 16; ++co) {
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hh = h - kh + 1;
        if (hh < 0 || hh >= 4) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = wq - kw + 1;
          if (ww < 0 || ww >= 8) continue;
          dp += dcs[co * 32 + hh * 8 + ww] * ws[(co * 8 + ch) * 9 + kh * 3 + kw];
        }
      }
    }
    const float4 v = reinterpret_cast<const float4*>(a0)[g * 256 + t];
    int k = 0; float m = v.x;                                    // first maximum wins (k_maxpool4_bwd)
    if (v.y > m) { m = v.y; k = 1; }
    if (v.z > m) { m = v.z; k = 2; }
    if (v.w > m) { m = v.w; k = 3; }
    const float d4[4] = {k == 0 ? dp : 0.f, k == 1 ? dp : 0.f, k == 2 ? dp : 0.f, k == 3 ? dp : 0.f};
    reinterpret_cast<float4*>(da0)[g * 256 + t] = make_float4(d4[0], d4[1], d4[2], d4[3]);
    const float4 xv = reinterpret_cast<const float4*>(c0)[g * 256 + t];
    const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float xh, du;
      cnn_bn_du<8>(x4[i], d4[i], bn1, ch, xh, du);
      acc[0] += (double)du; acc[1] += (double)du * (double)xh;
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const double v = cnn_half_sum_d(acc[a]);
    if ((t & 31) == 0) partial_out[blockIdx.x * kCnnEncBwdSlot + kBwdBn1 + a * 8 + ch] = v;
  }
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (t + 256 * j < 1152) partial_out[blockIdx.x * kCnnEncBwdSlot + kBwdDw4 + t + 256 * j] = gw[j];
  if (t >= 128 && t < 144) partial_out[blockIdx.x * kCnnEncBwdSlot + kBwdDw4 + 1152 + t - 128] = gb;
}
// encoder backward 3/4: conv4's dw / db += the slots' sums (workgroup b owns elements b, b + gridDim.x, ..; gridDim.x = nslot);
// BN1 backward -> dc0 (registers), conv0's weight / bias gradient: fp64 per workgroup into its slot, added up by
// k_cnn_enc_bwd_dw0 behind it (no atomics or fences beside the GCL kernels: profiles/LOG.md).  Thread = (channel, 4 positions).
__global__ void __launch_bounds__(kCnnThreads) k_cnn_enc_bwd_in(const float* __restrict__ s, const float* __restrict__ c0,
                                                                const float* __restrict__ da0, const float* __restrict__ mean,
                                                                const float* __restrict__ var, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const double* __restrict__ partial_in,
                                                                int nslot, int G, float eps, float* dgamma, float* dbeta, float* dw4,
                                                                float* db4, double* partial_out, float* __restrict__ dc0_out) {
  __shared__ double sums[16];
  __shared__ float bn[4 * 8], mb[2 * 8];
  __shared__ float xs[128];
  const int t = threadIdx.x;
  for (int o = blockIdx.x + nslot * (t >> 4); o < 1152 + 16; o += nslot * (kCnnThreads / 16)) {
    double v = 0;
    for (int k = t & 15; k < nslot; k += 16) v += partial_in[k * kCnnEncBwdSlot + kBwdDw4 - kBwdBn1 + o];      // (partial_in = slot + kBwdBn1)
#pragma unroll
    for (int i = 8; i > 0; i >>= 1) v += __shfl_xor(v, i, 16);
    if ((t & 15) == 0) {
      if (o < 1152) dw4[o] += (float)v;
      else db4[o - 1152] += (float)v;
    }
  }
  cnn_sum_slots<16, kCnnEncBwdSlot>(partial_in, nslot, sums);
  if (t < 8) {
    cnn_bn_saved<8>(t, mean, var, gamma, beta, eps, bn);
    const double count = (double)G * 128.0;
    mb[t] = (float)(sums[t] / count); mb[8 + t] = (float)(sums[8 + t] / count);
    if (blockIdx.x == 0) { dbeta[t] += (float)sums[t]; dgamma[t] += (float)sums[8 + t]; }
  }
  const int ch = t >> 5, q = t & 31, h = q >> 3, w0 = (q & 7) * 4;
  double gw[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    __syncthreads();
    if (t < 128) xs[t] = s[g * 128 + t];
    __syncthreads();
    const float4 xv = reinterpret_cast<const float4*>(c0)[g * 256 + t];
    const float4 dv = reinterpret_cast<const float4*>(da0)[g * 256 + t];
    const float x4[4] = {xv.x, xv.y, xv.z, xv.w}, d4[4] = {dv.x, dv.y, dv.z, dv.w};
    float dc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float xh, du;
      cnn_bn_du<8>(x4[i], d4[i], bn, ch, xh, du);
      dc[i] = bn[16 + ch] * bn[8 + ch] * (du - mb[ch] - xh * mb[8 + ch]);
    }
    if (dc0_out) reinterpret_cast<float4*>(dc0_out)[g * 256 + t] = make_float4(dc[0], dc[1], dc[2], dc[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gw[9] += (double)dc[i];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hh = h + kh - 1;
        if (hh < 0 || hh >= 4) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = w0 + i + kw - 1;
          if (ww < 0 || ww >= 32) continue;
          gw[kh * 3 + kw] += (double)dc[i] * (double)xs[hh * 32 + ww];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 10; ++j) gw[j] = cnn_half_sum_d(gw[j]);
  if (q == 0) {
#pragma unroll
    for (int j = 0; j < 10; ++j) partial_out[blockIdx.x * kCnnEncBwdSlot + kBwdDw0 + ch * 10 + j] = gw[j];
  }
}
// encoder backward 4/4 (one workgroup): conv0's dw / db += the slots' sums.  v = channel * 10 + {9 taps, bias}: sixteen threads
// per value and five values per thread, so a thread has five independent chains of loads in flight
__global__ void __launch_bounds__(kCnnThreads) k_cnn_enc_bwd_dw0(const double* __restrict__ partial, int nslot, float* dw, float* db) {
  const int t = threadIdx.x;
  double a5[5] = {0, 0, 0, 0, 0};
  const double* slots = partial + kBwdDw0 + (t >> 4);
  for (int k = t & 15; k < nslot; k += 16)
#pragma unroll
    for (int i = 0; i < 5; ++i) a5[i] += slots[k * kCnnEncBwdSlot + 16 * i];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double a = a5[i];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 16);
    const int v = (t >> 4) + 16 * i;
    if ((t & 15) == 0) {
      if (v % 10 < 9) dw[(v / 10) * 9 + v % 10] += (float)a;
      else db[v / 10] += (float)a;
    }
  }
}

// workgroups (= scratch slots) of a chain's launches: one bar each up to kCnnMaxSlots, and no more than the scratch holds
static inline int cnn_slots(int G, int64_t scratch_len, int per_slot) {
  int64_t n = G < kCnnMaxSlots ? G : kCnnMaxSlots;
  if (n > scratch_len / per_slot) n = scratch_len / per_slot;
  return (int)n;
}
static inline bool cnn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int kCnnMaxBars = 1 << 20;                 // 32-bit element indices: G * 1024 floats

extern "C" int pm_cnn_enc_fwd(const float* s, const float* w0, const float* b0, const float* gamma1, const float* beta1,
                              const float* w4, const float* b4, const float* gamma5, const float* beta5, int32_t G, float eps,
                              float momentum, float* c0, float* a0, float* p0, float* c1, float* a1, float* mean1, float* var1,
                              float* rmean1, float* rvar1, float* mean5, float* var5, float* rmean5, float* rvar5,
                              double* scratch, int64_t scratch_len, pm_stream_t stream) {
  if (!s || !w0 || !b0 || !gamma1 || !beta1 || !w4 || !b4 || !gamma5 || !beta5 || !c0 || !a0 || !p0 || !c1 || !a1 || !mean1 ||
      !var1 || !mean5 || !var5 || !scratch || G <= 0 || G > kCnnMaxBars || !cnn_al16(c0) || !cnn_al16(a0) || !cnn_al16(c1) ||
      !cnn_al16(a1))
    return PM_E_INVALID;
  const int n = cnn_slots(G, scratch_len, kCnnEncFwdSlot);
  if (n < 1) return PM_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cnn_enc_conv0, dim3(n), dim3(kCnnThreads), 0, st, s, w0, b0, G, c0, scratch);
  hipLaunchKernelGGL(k_cnn_enc_mid, dim3(n), dim3(kCnnThreads), 0, st, c0, scratch, n, gamma1, beta1, w4, b4, G, eps, momentum, a0,
                     p0, c1, mean1, var1, rmean1, rvar1, scratch);
  hipLaunchKernelGGL(k_cnn_enc_out, dim3(n), dim3(kCnnThreads), 0, st, c1, scratch + 16, n, gamma5, beta5, G, eps, momentum, a1,
                     mean5, var5, rmean5, rvar5);
  return pm_check_launch();
}
extern "C" int pm_cnn_dec_fwd(const float* u2, const float* w1, const float* b1, const float* gamma2, const float* beta2,
                              const float* w4, const float* b4, int32_t G, float eps, float momentum, float* c2, float* a2,
                              float* s_logits, float* mean2, float* var2, float* rmean2, float* rvar2, double* scratch,
                              int64_t scratch_len, pm_stream_t stream) {
  if (!u2 || !w1 || !b1 || !gamma2 || !beta2 || !w4 || !b4 || !c2 || !a2 || !s_logits || !mean2 || !var2 || !scratch || G <= 0 ||
      G > kCnnMaxBars || !cnn_al16(c2) || !cnn_al16(a2))
    return PM_E_INVALID;
  const int n = cnn_slots(G, scratch_len, kCnnDecFwdSlot);
  if (n < 1) return PM_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cnn_dec_conv1, dim3(n), dim3(kCnnThreads), 0, st, u2, w1, b1, G, c2, scratch);
  hipLaunchKernelGGL(k_cnn_dec_out, dim3(n), dim3(kCnnThreads), 0, st, c2, scratch, n, gamma2, beta2, w4, b4, G, eps, momentum, a2,
                     s_logits, mean2, var2, rmean2, rvar2);
  return pm_check_launch();
}
extern "C" int pm_cnn_enc_bwd(const float* s, const float* c0, const float* a0, const float* p0, const float* c1, const float* da1,
                              const float* mean1, const float* var1, const float* gamma1, const float* beta1, const float* mean5,
                              const float* var5, const float* gamma5, const float* beta5, const float* w4, int32_t G, float eps,
                              float* dw0, float* db0, float* dgamma1, float* dbeta1, float* dw4, float* db4, float* dgamma5,
                              float* dbeta5, float* dc1, float* da0, float* dc0, double* scratch, int64_t scratch_len,
                              pm_stream_t stream) {
  if (!s || !c0 || !a0 || !p0 || !c1 || !da1 || !mean1 || !var1 || !gamma1 || !beta1 || !mean5 || !var5 || !gamma5 || !beta5 ||
      !w4 || !dw0 || !db0 || !dgamma1 || !dbeta1 || !dw4 || !db4 || !dgamma5 || !dbeta5 || !da0 || !scratch || G <= 0 ||
      G > kCnnMaxBars || !cnn_al16(c0) || !cnn_al16(a0) || !cnn_al16(da0) || (dc0 && !cnn_al16(dc0)))
    return PM_E_INVALID;
  const int n = cnn_slots(G, scratch_len, kCnnEncBwdSlot);
  if (n < 1) return PM_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cnn_enc_bwd_sums, dim3(n), dim3(kCnnThreads), 0, st, c1, da1, mean5, var5, gamma5, beta5, G, eps, scratch);
  hipLaunchKernelGGL(k_cnn_enc_bwd_mid, dim3(n), dim3(kCnnThreads), 0, st, c1, da1, p0, a0, c0, mean5, var5, gamma5, beta5, mean1,
                     var1, gamma1, beta1, w4, scratch, n, G, eps, dgamma5, dbeta5, dc1, da0, scratch);
  hipLaunchKernelGGL(k_cnn_enc_bwd_in, dim3(n), dim3(kCnnThreads), 0, st, s, c0, da0, mean1, var1, gamma1, beta1, scratch + kBwdBn1, n, G,
                     eps, dgamma1, dbeta1, dw4, db4, scratch, dc0);
  hipLaunchKernelGGL(k_cnn_enc_bwd_dw0, dim3(1), dim3(kCnnThreads), 0, st, scratch, n, dw0, db0);
  return pm_check_launch();
}

// Keras optimizers (Adam, RMSprop, Nadam, SGD) over a flat fp32 arena, the global gradient norm / clip scale with its overflow guard
// and dynamic loss scaling.  HBM-bound streaming kernels; the gradient-norm reduction is two-stage and fixed-order.
#include "common.h"

// ------------------------------------------------------------------------------------------
// Optimizers (Keras 2.2.4 formulas).  state[0] = iteration t (int), state[1] = lr_t (float bits)
// gscale[0] <= 0 (or NaN) = "skip this step": stp_grad_global_scale found a non-finite gradient (fp16 overflow under loss scaling).
// Every optimizer kernel - the per-step scalar preparation included - returns without touching parameters, moments or the step
// counter, so one overflowing batch cannot poison P / m / v.
__device__ __forceinline__ bool opt_skip(const float* gscale) { return gscale && !(gscale[0] > 0.f); }

__global__ void adam_prep_kernel(int32_t* state, const float* lr, float beta1, float beta2, const float* gscale) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || opt_skip(gscale)) return;
  const int t = state[0] + 1;
  state[0] = t;
  const double lr_t = (double)lr[0] * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t));
  reinterpret_cast<float*>(state)[1] = (float)lr_t;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t count, const int32_t* state, float b1,
                                                   float b2, float eps, const uint8_t* __restrict__ mask,
                                                   const float* gscale, float clipvalue) {
  const float lr_t = reinterpret_cast<const float*>(state)[1];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 mv = load4(m + i * 4), vv = load4(v + i * 4), pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float mn = b1 * mv[e] + (1.f - b1) * gv[e];
      const float vn = b2 * vv[e] + (1.f - b2) * gv[e] * gv[e];
      pv[e] = pv[e] - lr_t * mn / (sqrtf(vn) + eps);
      mv[e] = mn;
      vv[e] = vn;
    }
    store4(m + i * 4, mv);
    store4(v + i * 4, vv);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_adam(float* param, const float* grad, float* m, float* v, int64_t count, const float* lr, float beta1,
                        float beta2, float eps, int32_t* state, const uint8_t* mask, const float* gscale, float clipvalue,
                        void* stream) {
  if (!param || !grad || !m || !v || !lr || !state || count <= 0 || (count & 3)) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(64), 0, s, state, lr, beta1, beta2, gscale);
  STP_LAUNCH_CHECK();
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(adam_kernel, dim3((int)g), dim3(256), 0, s, param, grad, m, v, count, state, beta1, beta2, eps, mask,
                     gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// RMSprop (keras/optimizers.py 2.2.4): a <- rho a + (1-rho) g^2 ; p <- p - lr g / (sqrt(a) + eps)
__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ acc,
                                                      int64_t count, const float* lr, float rho, float eps,
                                                      const uint8_t* __restrict__ mask, const float* gscale, float clipvalue) {
  const float l = lr[0];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 av = load4(acc + i * 4), pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float an = rho * av[e] + (1.f - rho) * gv[e] * gv[e];
      pv[e] = pv[e] - l * gv[e] / (sqrtf(an) + eps);
      av[e] = an;
    }
    store4(acc + i * 4, av);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_rmsprop(float* param, const float* grad, float* acc, int64_t count, const float* lr, float rho, float eps,
                           const uint8_t* mask, const float* gscale, float clipvalue, void* stream) {
  if (!param || !grad || !acc || !lr || count <= 0 || (count & 3)) return STP_E_BADARG;
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(rmsprop_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, param, grad, acc, count, lr, rho, eps, mask,
                     gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// Nadam (keras/optimizers.py 2.2.4, schedule_decay form).  state[0] = iteration t, fstate[0] = m_schedule (starts at 1),
// fstate[1..5] = this step's scalars {1/(1-m_schedule_new), 1/(1-m_schedule_next), 1/(1-beta2^t), 1-mu_t, mu_{t+1}}
__global__ void nadam_prep_kernel(int32_t* state, float* fstate, float beta1, float beta2, float schedule_decay, const float* gscale) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || opt_skip(gscale)) return;
  const int t = state[0] + 1;
  state[0] = t;
  const double mu_t = (double)beta1 * (1.0 - 0.5 * pow(0.96, (double)t * (double)schedule_decay));
  const double mu_t1 = (double)beta1 * (1.0 - 0.5 * pow(0.96, (double)(t + 1) * (double)schedule_decay));
  const double ms_new = (double)fstate[0] * mu_t;
  const double ms_next = ms_new * mu_t1;
  fstate[0] = (float)ms_new;
  fstate[1] = (float)(1.0 / (1.0 - ms_new));
  fstate[2] = (float)(1.0 / (1.0 - ms_next));
  fstate[3] = (float)(1.0 / (1.0 - pow((double)beta2, (double)t)));
  fstate[4] = (float)(1.0 - mu_t);
  fstate[5] = (float)mu_t1;
}

__global__ __launch_bounds__(256) void nadam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t count, const float* lr, const float* fstate,
                                                    float b1, float b2, float eps, const uint8_t* __restrict__ mask,
                                                    const float* gscale, float clipvalue) {
  const float l = lr[0];
  const float ig = fstate[1], im = fstate[2], iv = fstate[3], cg = fstate[4], cm = fstate[5];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 mv = load4(m + i * 4), vv = load4(v + i * 4), pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float mn = b1 * mv[e] + (1.f - b1) * gv[e];
      const float vn = b2 * vv[e] + (1.f - b2) * gv[e] * gv[e];
      const float mbar = cg * (gv[e] * ig) + cm * (mn * im);
      pv[e] = pv[e] - l * mbar / (sqrtf(vn * iv) + eps);
      mv[e] = mn;
      vv[e] = vn;
    }
    store4(m + i * 4, mv);
    store4(v + i * 4, vv);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_nadam(float* param, const float* grad, float* m, float* v, int64_t count, const float* lr, float beta1,
                         float beta2, float eps, float schedule_decay, int32_t* state, float* fstate, const uint8_t* mask,
                         const float* gscale, float clipvalue, void* stream) {
  if (!param || !grad || !m || !v || !lr || !state || !fstate || count <= 0 || (count & 3)) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nadam_prep_kernel, dim3(1), dim3(64), 0, s, state, fstate, beta1, beta2, schedule_decay, gscale);
  STP_LAUNCH_CHECK();
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(nadam_kernel, dim3((int)g), dim3(256), 0, s, param, grad, m, v, count, lr, fstate, beta1, beta2, eps, mask,
                     gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ vel,
                                                  int64_t count, const float* lr, float mu, int nesterov,
                                                  const uint8_t* __restrict__ mask, const float* gscale, float clipvalue) {
  const float l = lr[0];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 vv = vel ? load4(vel + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f}, pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float vn = mu * vv[e] - l * gv[e];
      pv[e] = nesterov ? pv[e] + mu * vn - l * gv[e] : pv[e] + vn;
      vv[e] = vn;
    }
    if (vel) store4(vel + i * 4, vv);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_sgd(float* param, const float* grad, float* vel, int64_t count, const float* lr, float momentum,
                       int32_t nesterov, const uint8_t* mask, const float* gscale, float clipvalue, void* stream) {
  if (!param || !grad || !lr || count <= 0 || (count & 3)) return STP_E_BADARG;
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(sgd_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, param, grad, vel, count, lr, momentum,
                     nesterov, mask, gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ||grad||^2 partials -> gscale = min(1, clipnorm/||base*g||) * base   (base = 1/world_size)
__global__ __launch_bounds__(256) void sqsum_partial_kernel(const float* __restrict__ g, int64_t count, float* partial) {
  float a = 0.f;
  const int64_t per = (count + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < count ? i0 + per : count;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) a += g[i] * g[i];
  __shared__ float red[4];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void gscale_finalize_kernel(const float* partial, int blocks, float clipnorm, float base,
                                                              float* gscale) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) a += (double)partial[b];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double norm = sqrt(sh[0]) * (double)base;  // norm of the (mean) gradient the optimizer will see
  if (!(sh[0] >= 0.0 && sh[0] < 1e300 * 1e300) || !(norm == norm)) {   // inf / NaN somewhere in the arena: the step is skipped (opt_skip)
    gscale[0] = -1.f;
    gscale[1] += 1.f;                              // skipped steps so far (host: HipSegModel.skipped_steps)
    return;
  }
  double k = 1.0;
  if (clipnorm > 0.f && norm > (double)clipnorm) k = (double)clipnorm / norm;
  gscale[0] = (float)(k * (double)base);
}

extern "C" int stp_grad_global_scale(const float* grad, int64_t count, float clipnorm, float base, float* gscale,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!grad || !gscale || !workspace || count <= 0) return STP_E_BADARG;
  if (workspace_bytes < 1024 * sizeof(float)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int64_t b = count / 4096;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  hipLaunchKernelGGL(sqsum_partial_kernel, dim3((int)b), dim3(256), 0, s, grad, count, (float*)workspace);
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gscale_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (int)b, clipnorm, base, gscale);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ---- dynamic loss scaling (fp16 storage).  dls = float[8] on the device: [0] multiplier m of the NEXT backward pass (a power of two, on
// top of the static scale the loss kernels apply), [1] clean steps since the last change, [2] growth interval (steps), [3] smallest m,
// [4] m of the gradients now in the arena (written by stp_scale_by_device when the backward pass is seeded), [5] largest m.  Everything happens on the device, inside the
// captured step: stp_scale_by_device multiplies the loss gradient by m right after the loss kernel seeded it; the _dls form of
// stp_grad_global_scale folds 1/m into gscale, halves m when the step is skipped (non-finite gradient) and doubles it after
// `interval` clean steps - the schedule of torch.cuda.amp.GradScaler / Keras' LossScaleOptimizer.
template <typename T>
__global__ __launch_bounds__(256) void scale_by_device_kernel(T* __restrict__ x, int64_t count, const float* __restrict__ scalar, float* record) {
  const float m = scalar[0];
  if (record && blockIdx.x == 0 && threadIdx.x == 0) record[0] = m;      // (the multiplier this backward pass runs under: dls[4])
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    Elem<T>::store(x + i, Elem<T>::load(x + i) * m);
}
extern "C" int stp_scale_by_device(void* x, int64_t count, int32_t dtype, const float* scalar, float* record, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;
  if (!x || !scalar || count <= 0) return STP_E_BADARG;
  int64_t g = (count + 255) / 256;
  if (g > 8192) g = 8192;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == STP_H16) hipLaunchKernelGGL(scale_by_device_kernel<bf16_t>, dim3((int)g), dim3(256), 0, s, (bf16_t*)x, count, scalar, record);
  else if (dtype == STP_F32) hipLaunchKernelGGL(scale_by_device_kernel<float>, dim3((int)g), dim3(256), 0, s, (float*)x, count, scalar, record);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

__global__ __launch_bounds__(256) void gscale_finalize_dls_kernel(const float* partial, int blocks, float clipnorm, float base,
                                                                  float* gscale, float* dls) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) a += (double)partial[b];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float m = dls[0];
  // the gradients in the arena were produced under dls[4] (recorded by stp_scale_by_device when their backward pass was seeded);
  // dls[0] is the multiplier of the NEXT pass - equal only while every step is one backward pass followed by one optimizer launch
  const double eff = (double)base / (double)dls[4];  // what turns an arena value into the gradient the optimizer sees
  const double norm = sqrt(sh[0]) * eff;
  if (!(sh[0] >= 0.0 && sh[0] < 1e300 * 1e300) || !(norm == norm)) {   // overflow: skip the step, halve the multiplier
    gscale[0] = -1.f;
    gscale[1] += 1.f;
    dls[0] = fmaxf(m * 0.5f, dls[3]);
    dls[1] = 0.f;
    return;
  }
  double k = 1.0;
  if (clipnorm > 0.f && norm > (double)clipnorm) k = (double)clipnorm / norm;
  gscale[0] = (float)(k * eff);
  const float clean = dls[1] + 1.f;
  if (clean >= dls[2]) { dls[0] = fminf(m * 2.f, dls[5]); dls[1] = 0.f; }
  else dls[1] = clean;
}

extern "C" int stp_grad_global_scale_dls(const float* grad, int64_t count, float clipnorm, float base, float* gscale, float* dls,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!grad || !gscale || !dls || !workspace || count <= 0) return STP_E_BADARG;
  if (workspace_bytes < 1024 * sizeof(float)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int64_t b = count / 4096;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  hipLaunchKernelGGL(sqsum_partial_kernel, dim3((int)b), dim3(256), 0, s, grad, count, (float*)workspace);
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gscale_finalize_dls_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (int)b, clipnorm, base, gscale, dls);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

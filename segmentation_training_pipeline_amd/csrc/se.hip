// Channel squeeze-and-excitation (SE-ResNet basic units): x = u * sigmoid(relu(mean_hw(u) W1 + b1) W2 + b2) + shortcut, forward and
// gradient, as self-contained HBM-bound passes next to the convolution kernels.
//
// Every tensor pass works on ITEMS = (image n, chunk of se_rpc consecutive pixels of that image): the gate s[n][c] is constant inside
// an item, an item is one column of a partial-sum table.  A workgroup of 256 threads covers RPB = 256 / (C / VEC) pixels per trip with
// one 16-byte vector per lane (VEC = 8 storage words or 4 floats); lane (r, g) keeps channels [g VEC, g VEC + VEC) of pixels r, r + RPB,
// ... in registers, the RPB rows meet in LDS and are added in row order.  Workgroups stride over the items with a capped grid.
// Reductions are two-stage with a fixed order (partials per item, summed in chunk order by the per-image kernels; parameter gradients
// summed in image order): no float atomics, a replay is bit-identical.
#include "common.h"

#define SE_THREADS 256
#define SE_MAX_C 512
#define SE_MAX_R 32
#define SE_GRID_CAP 1024   // workgroups of the tensor passes (4 per CU): more items than this take further trips of the item loop
#define SE_MAX_CHUNKS 256

// chunks per image: enough items to fill the chip at batch 2, at least 64 pixels each
static int se_chunks(int N, int64_t HW) {
  int64_t target = (1024 + N - 1) / N, by_rows = HW / 64;
  int64_t ch = target < by_rows ? target : by_rows;
  if (ch > SE_MAX_CHUNKS) ch = SE_MAX_CHUNKS;
  if (ch < 1) ch = 1;
  const int64_t rpc = (HW + ch - 1) / ch;
  return (int)((HW + rpc - 1) / rpc);
}
static int se_rpc(int N, int64_t HW) {
  const int ch = se_chunks(N, HW);
  return (int)((HW + ch - 1) / ch);
}
static bool se_shape_ok(int N, int64_t HW, int C) {
  return N > 0 && HW > 0 && HW <= (1 << 30) && C >= 16 && C <= SE_MAX_C && (C & 7) == 0 && (int64_t)N * se_chunks(N, HW) < (1ll << 31);
}

extern "C" int32_t stp_se_chunks(int32_t N, int64_t HW, int32_t C) { return se_shape_ok(N, HW, C) ? se_chunks(N, HW) : 0; }
extern "C" size_t stp_se_workspace_bytes(int32_t N, int64_t HW, int32_t C) {
  return se_shape_ok(N, HW, C) ? (size_t)N * se_chunks(N, HW) * C * sizeof(float) : 0;
}

template <typename T> struct SeVec;
template <> struct SeVec<float> {
  static constexpr int VEC = 4;
  __device__ static __forceinline__ void load(const float* p, float* v) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  }
  // stores v; v becomes the stored values
  __device__ static __forceinline__ void store(float* p, float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct SeVec<bf16_t> {
  static constexpr int VEC = 8;
  __device__ static __forceinline__ void load(const bf16_t* p, float* v) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = h16lo_to_f32(r[e]); v[2 * e + 1] = h16hi_to_f32(r[e]); }
  }
  __device__ static __forceinline__ void store(bf16_t* p, float* v) {
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
    *reinterpret_cast<u32x4*>(p) = r;
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = h16lo_to_f32(r[e]); v[2 * e + 1] = h16hi_to_f32(r[e]); }
  }
};

// ------------------------------------------------------------------------------------------
// squeeze (PROD = false): part[item][c] = sum over the item's pixels of a;  backward reduce (PROD = true): ... of a * b
template <typename T, bool PROD>
__global__ __launch_bounds__(SE_THREADS) void se_reduce_kernel(const T* __restrict__ a, const T* __restrict__ b, float* __restrict__ part,
                                                               int items, int chunks, int rpc, int HW, int C) {
  constexpr int VEC = SeVec<T>::VEC;
  __shared__ float sh[SE_THREADS * VEC];
  const int CG = C / VEC, RPB = SE_THREADS / CG;
  const int r = threadIdx.x / CG, g = threadIdx.x - r * CG;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int n = item / chunks, ch = item - n * chunks;
    const int row0 = ch * rpc, row1 = min(HW, row0 + rpc);
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    if (r < RPB) {
      const size_t base = (size_t)n * HW * C + (size_t)g * VEC;
#pragma unroll 4
      for (int row = row0 + r; row < row1; row += RPB) {
        float va[VEC];
        SeVec<T>::load(a + base + (size_t)row * C, va);
        if (PROD) {
          float vb[VEC];
          SeVec<T>::load(b + base + (size_t)row * C, vb);
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] = fmaf(va[e], vb[e], acc[e]);
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] += va[e];
        }
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) sh[r * C + g * VEC + e] = acc[e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += SE_THREADS) {
      float s = 0.f;
      for (int k = 0; k < RPB; ++k) s += sh[k * C + c];
      part[(size_t)item * C + c] = s;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// scale-add (TENSOR_ADD): y = a * s[n][c] + b[pixel][c], optionally with the per-item sum / sum of squares of the STORED y;
// backward apply (!TENSOR_ADD): y = a * s[n][c] + addv[n][c] * add_scale
template <typename T, bool TENSOR_ADD, bool STATS>
__global__ __launch_bounds__(SE_THREADS) void se_apply_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y,
                                                              const float* __restrict__ s, const float* __restrict__ addv, float add_scale,
                                                              float* __restrict__ stats, int items, int chunks, int rpc, int HW, int C) {
  constexpr int VEC = SeVec<T>::VEC;
  __shared__ float sh[STATS ? 2 * SE_THREADS * VEC : 1];
  const int CG = C / VEC, RPB = SE_THREADS / CG;
  const int r = threadIdx.x / CG, g = threadIdx.x - r * CG;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int n = item / chunks, ch = item - n * chunks;
    const int row0 = ch * rpc, row1 = min(HW, row0 + rpc);
    float sum[VEC], sq[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) sum[e] = sq[e] = 0.f;
    if (r < RPB) {
      float sv[VEC], av[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        sv[e] = s[(size_t)n * C + g * VEC + e];
        av[e] = TENSOR_ADD ? 0.f : addv[(size_t)n * C + g * VEC + e] * add_scale;
      }
      const size_t base = (size_t)n * HW * C + (size_t)g * VEC;
#pragma unroll 4
      for (int row = row0 + r; row < row1; row += RPB) {
        float va[VEC], vb[VEC];
        SeVec<T>::load(a + base + (size_t)row * C, va);
        if (TENSOR_ADD) SeVec<T>::load(b + base + (size_t)row * C, vb);
#pragma unroll
        for (int e = 0; e < VEC; ++e) va[e] = fmaf(va[e], sv[e], TENSOR_ADD ? vb[e] : av[e]);
        SeVec<T>::store(y + base + (size_t)row * C, va);
        if (STATS) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) { sum[e] += va[e]; sq[e] = fmaf(va[e], va[e], sq[e]); }
        }
      }
    }
    if (STATS) {
      if (r < RPB) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          sh[r * C + g * VEC + e] = sum[e];
          sh[SE_THREADS * VEC + r * C + g * VEC + e] = sq[e];
        }
      }
      __syncthreads();
      for (int c = threadIdx.x; c < C; c += SE_THREADS) {
        float t0 = 0.f, t1 = 0.f;
        for (int k = 0; k < RPB; ++k) { t0 += sh[k * C + c]; t1 += sh[SE_THREADS * VEC + k * C + c]; }
        stats[(size_t)c * items + item] = t0;                     // [2][C][items]: the layout stp_bn_finalize reads
        stats[((size_t)C + c) * items + item] = t1;
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------
// The per-image kernels are chains of short dependent steps on 16 workgroups: what they cost is memory latency, so every loop below
// issues its (independent) loads four or eight at a time and adds in a fixed order.

// vs[c] = sum over the chunks of part[n][k][c] for all c < C: with C <= 128 the 256 threads split the chunks into Q = 256 / C
// contiguous runs (each added in chunk order, the runs then in run order); valid after the trailing barrier
__device__ __forceinline__ void se_chunk_sums(const float* __restrict__ part_n, int chunks, int C, float* red, float* vs) {
  const int Q = C <= SE_THREADS / 2 ? SE_THREADS / C : 1;
  const int per = (chunks + Q - 1) / Q;
  for (int c0 = 0; c0 < C; c0 += SE_THREADS) {
    const int q = Q > 1 ? (int)threadIdx.x / C : 0, c = Q > 1 ? (int)threadIdx.x - q * C : c0 + (int)threadIdx.x;
    float a = 0.f;
    if (c < C && q < Q) {
      const int k1 = min(chunks, (q + 1) * per);
      int k = q * per;
      for (; k + 8 <= k1; k += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = part_n[(size_t)(k + i) * C + c];
#pragma unroll
        for (int i = 0; i < 8; ++i) a += v[i];
      }
      for (; k < k1; ++k) a += part_n[(size_t)k * C + c];
      if (Q > 1) red[q * C + c] = a; else vs[c] = a;
    }
  }
  if (Q > 1) {
    __syncthreads();
    if ((int)threadIdx.x < C) {
      float a = 0.f;
      for (int q = 0; q < Q; ++q) a += red[q * C + threadIdx.x];
      vs[threadIdx.x] = a;
    }
  }
  __syncthreads();
}

// out[j] = sum over c < K of v[c] * M[c * ldc + j * ldj] for j < J <= 32; v and out live in LDS.  J a power of two: L = 256 / J lanes per
// output take interleaved c and meet in a shuffle butterfly inside their aligned lane group (fixed order, no LDS).  Otherwise the 256
// threads split K into P = 256 / J interleaved parts that meet in LDS and are added in part order.
__device__ __forceinline__ void se_matvec_small(const float* v, const float* __restrict__ M, int K, int J, int ldc, int ldj, float* red, float* out) {
  if ((J & (J - 1)) == 0) {
    const int L = SE_THREADS / J;                        // 8 .. 256, a power of two
    const int j = (int)threadIdx.x / L, p = (int)threadIdx.x - j * L;
    float a = 0.f;
    int c = p;
    for (; c + 3 * L < K; c += 4 * L) {
      const float m0 = M[(size_t)c * ldc + (size_t)j * ldj], m1 = M[(size_t)(c + L) * ldc + (size_t)j * ldj];
      const float m2 = M[(size_t)(c + 2 * L) * ldc + (size_t)j * ldj], m3 = M[(size_t)(c + 3 * L) * ldc + (size_t)j * ldj];
      a = fmaf(v[c], m0, a); a = fmaf(v[c + L], m1, a); a = fmaf(v[c + 2 * L], m2, a); a = fmaf(v[c + 3 * L], m3, a);
    }
    for (; c < K; c += L) a = fmaf(v[c], M[(size_t)c * ldc + (size_t)j * ldj], a);
    if (L <= 64) {
      for (int o = L >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if (p == 0) out[j] = a;
    } else {                                             // J = 1 or 2: whole waves per output, the waves meet in LDS
      a = wave_sum(a);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
      __syncthreads();
      if ((int)threadIdx.x < J) {
        const int w = L >> 6;
        float t = 0.f;
        for (int k = 0; k < w; ++k) t += red[threadIdx.x * w + k];
        out[threadIdx.x] = t;
      }
    }
    __syncthreads();
    return;
  }
  const int P = SE_THREADS / J;
  const int j = threadIdx.x % J, p = threadIdx.x / J;
  if (p < P) {
    float a = 0.f;
    for (int c = p; c < K; c += P) a = fmaf(v[c], M[(size_t)c * ldc + (size_t)j * ldj], a);
    red[p * J + j] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < J) {
    float a = 0.f;
    for (int k = 0; k < P; ++k) a += red[k * J + threadIdx.x];
    out[threadIdx.x] = a;
  }
  __syncthreads();
}

// acc + sum over j < J of hs[j] * M[j * ld] (M already offset to the thread's column), four loads in flight
__device__ __forceinline__ float se_dot_small(const float* hs, const float* __restrict__ M, int J, size_t ld, float acc) {
  int j = 0;
  for (; j + 4 <= J; j += 4) {
    const float m0 = M[(size_t)j * ld], m1 = M[(size_t)(j + 1) * ld], m2 = M[(size_t)(j + 2) * ld], m3 = M[(size_t)(j + 3) * ld];
    acc = fmaf(hs[j], m0, acc); acc = fmaf(hs[j + 1], m1, acc); acc = fmaf(hs[j + 2], m2, acc); acc = fmaf(hs[j + 3], m3, acc);
  }
  for (; j < J; ++j) acc = fmaf(hs[j], M[(size_t)j * ld], acc);
  return acc;
}

// one workgroup per image: z = (sum of the chunk partials, in a fixed order) / HW, h = relu(z W1 + b1), s = sigmoid(h W2 + b2)
__global__ __launch_bounds__(SE_THREADS) void se_excite_kernel(const float* __restrict__ part, int chunks, float inv_hw, int C, int R,
                                                               const float* __restrict__ W1, const float* __restrict__ b1,
                                                               const float* __restrict__ W2, const float* __restrict__ b2,
                                                               float* __restrict__ z, float* __restrict__ h, float* __restrict__ s) {
  __shared__ float zs[SE_MAX_C], red[SE_THREADS], hs[SE_MAX_R];
  const int n = blockIdx.x;
  se_chunk_sums(part + (size_t)n * chunks * C, chunks, C, red, zs);
  for (int c = threadIdx.x; c < C; c += SE_THREADS) {
    const float a = zs[c] * inv_hw;
    zs[c] = a;
    z[(size_t)n * C + c] = a;
  }
  __syncthreads();
  se_matvec_small(zs, W1, C, R, R, 1, red, hs);             // W1 [C][R]
  if ((int)threadIdx.x < R) {
    const float a = fmaxf(hs[threadIdx.x] + b1[threadIdx.x], 0.f);
    hs[threadIdx.x] = a;
    h[(size_t)n * R + threadIdx.x] = a;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += SE_THREADS) {
    const float a = se_dot_small(hs, W2 + c, R, C, b2[c]);  // W2 [R][C]
    s[(size_t)n * C + c] = 1.f / (1.f + expf(-a));
  }
}

// one workgroup per image: ds = sum of the chunk partials, da2 = ds s (1 - s), dh = da2 W2^T, da1 = dh [h > 0], dz = da1 W1^T
__global__ __launch_bounds__(SE_THREADS) void se_excite_bwd_kernel(const float* __restrict__ part, int chunks, int C, int R,
                                                                   const float* __restrict__ W1, const float* __restrict__ W2,
                                                                   const float* __restrict__ h, const float* __restrict__ s,
                                                                   float* __restrict__ da2, float* __restrict__ da1, float* __restrict__ dz) {
  __shared__ float as[SE_MAX_C], red[SE_THREADS], hs[SE_MAX_R];
  const int n = blockIdx.x;
  se_chunk_sums(part + (size_t)n * chunks * C, chunks, C, red, as);
  for (int c = threadIdx.x; c < C; c += SE_THREADS) {
    const float sv = s[(size_t)n * C + c];
    const float a = as[c] * sv * (1.f - sv);
    as[c] = a;
    da2[(size_t)n * C + c] = a;
  }
  __syncthreads();
  se_matvec_small(as, W2, C, R, 1, C, red, hs);             // dh[j] = sum_c da2[c] W2[j][c]
  if ((int)threadIdx.x < R) {
    const float a = h[(size_t)n * R + threadIdx.x] > 0.f ? hs[threadIdx.x] : 0.f;
    hs[threadIdx.x] = a;
    da1[(size_t)n * R + threadIdx.x] = a;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += SE_THREADS) dz[(size_t)n * C + c] = se_dot_small(hs, W1 + (size_t)c * R, R, 1, 0.f);
}

// sum over n < N of a[n * lda] * b[n * ldb] (b == nullptr: of a alone), in image order, four loads in flight
__device__ __forceinline__ float se_image_sum(const float* __restrict__ a, size_t lda, const float* __restrict__ b, size_t ldb, int N) {
  float acc = 0.f;
  int n = 0;
  for (; n + 4 <= N; n += 4) {
    float x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i] = a[(size_t)(n + i) * lda]; y[i] = b ? b[(size_t)(n + i) * ldb] : 1.f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = b ? fmaf(x[i], y[i], acc) : acc + x[i];
  }
  for (; n < N; ++n) acc = b ? fmaf(a[(size_t)n * lda], b[(size_t)n * ldb], acc) : acc + a[(size_t)n * lda];
  return acc;
}

// parameter gradients, one thread per element, summed over the images in image order and WRITTEN:
// dW1[c][j] = sum_n z[n][c] da1[n][j], dW2[j][c] = sum_n h[n][j] da2[n][c], db1 = sum_n da1, db2 = sum_n da2
__global__ __launch_bounds__(SE_THREADS) void se_param_grad_kernel(const float* __restrict__ z, const float* __restrict__ h,
                                                                   const float* __restrict__ da2, const float* __restrict__ da1, int N, int C, int R,
                                                                   float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2,
                                                                   float* __restrict__ db2) {
  const int CR = C * R, total = 2 * CR + R + C;
  for (int i = blockIdx.x * SE_THREADS + threadIdx.x; i < total; i += gridDim.x * SE_THREADS) {
    if (i < CR) {
      const int c = i / R, j = i - c * R;
      dW1[i] = se_image_sum(z + c, C, da1 + j, R, N);
    } else if (i < 2 * CR) {
      const int k = i - CR, j = k / C, c = k - j * C;
      dW2[k] = se_image_sum(h + j, R, da2 + c, C, N);
    } else if (i < 2 * CR + R) {
      db1[i - 2 * CR] = se_image_sum(da1 + (i - 2 * CR), R, nullptr, 0, N);
    } else {
      db2[i - 2 * CR - R] = se_image_sum(da2 + (i - 2 * CR - R), C, nullptr, 0, N);
    }
  }
}

// ------------------------------------------------------------------------------------------
static int se_grid(int64_t items) { return (int)(items < SE_GRID_CAP ? items : SE_GRID_CAP); }
static bool se_r_ok(int C, int R) { return R >= 1 && R <= SE_MAX_R && R <= C; }

template <bool PROD>
static int se_reduce_launch(const void* a, const void* b, int dtype, int N, int64_t HW, int C, float* ws, size_t ws_bytes, void* stream) {
  if (!a || (PROD && !b) || !ws || !stp_dtype_ok(dtype) || !se_shape_ok(N, HW, C)) return STP_E_BADARG;
  if (ws_bytes < stp_se_workspace_bytes(N, HW, C)) return STP_E_WORKSPACE;
  const int chunks = se_chunks(N, HW), rpc = se_rpc(N, HW), items = N * chunks;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == STP_F32)
    hipLaunchKernelGGL((se_reduce_kernel<float, PROD>), dim3(se_grid(items)), dim3(SE_THREADS), 0, s, (const float*)a, (const float*)b, ws, items,
                       chunks, rpc, (int)HW, C);
  else
    hipLaunchKernelGGL((se_reduce_kernel<bf16_t, PROD>), dim3(se_grid(items)), dim3(SE_THREADS), 0, s, (const bf16_t*)a, (const bf16_t*)b, ws,
                       items, chunks, rpc, (int)HW, C);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_se_squeeze(const void* u, int32_t dtype, int32_t N, int64_t HW, int32_t C, float* workspace, size_t workspace_bytes,
                              void* stream) {
  return se_reduce_launch<false>(u, nullptr, dtype, N, HW, C, workspace, workspace_bytes, stream);
}

extern "C" int stp_se_bwd_reduce(const void* dx, const void* u, int32_t dtype, int32_t N, int64_t HW, int32_t C, float* workspace,
                                 size_t workspace_bytes, void* stream) {
  return se_reduce_launch<true>(dx, u, dtype, N, HW, C, workspace, workspace_bytes, stream);
}

extern "C" int stp_se_excite(const float* workspace, int32_t N, int64_t HW, int32_t C, int32_t R, const float* W1, const float* b1,
                             const float* W2, const float* b2, float* z, float* h, float* s, void* stream) {
  if (!workspace || !W1 || !b1 || !W2 || !b2 || !z || !h || !s || !se_shape_ok(N, HW, C) || !se_r_ok(C, R)) return STP_E_BADARG;
  hipLaunchKernelGGL(se_excite_kernel, dim3(N), dim3(SE_THREADS), 0, (hipStream_t)stream, workspace, se_chunks(N, HW), 1.f / (float)HW, C, R,
                     W1, b1, W2, b2, z, h, s);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_se_scale_add(const void* u, const void* shortcut, void* x, int32_t dtype, int32_t N, int64_t HW, int32_t C, const float* s,
                                float* stats, void* stream) {
  if (!u || !shortcut || !x || !s || !stp_dtype_ok(dtype) || !se_shape_ok(N, HW, C)) return STP_E_BADARG;
  const int chunks = se_chunks(N, HW), rpc = se_rpc(N, HW), items = N * chunks;
  hipStream_t st = (hipStream_t)stream;
#define SE_SA(T, STATS)                                                                                                                  \
  hipLaunchKernelGGL((se_apply_kernel<T, true, STATS>), dim3(se_grid(items)), dim3(SE_THREADS), 0, st, (const T*)u, (const T*)shortcut, \
                     (T*)x, s, (const float*)nullptr, 0.f, stats, items, chunks, rpc, (int)HW, C)
  if (dtype == STP_F32) {
    if (stats) SE_SA(float, true); else SE_SA(float, false);
  } else {
    if (stats) SE_SA(bf16_t, true); else SE_SA(bf16_t, false);
  }
#undef SE_SA
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_se_excite_bwd(const float* workspace, int32_t N, int64_t HW, int32_t C, int32_t R, const float* W1, const float* W2,
                                 const float* z, const float* h, const float* s, float* da2, float* da1, float* dz, float* dW1, float* db1,
                                 float* dW2, float* db2, void* stream) {
  if (!workspace || !W1 || !W2 || !z || !h || !s || !da2 || !da1 || !dz || !dW1 || !db1 || !dW2 || !db2 || !se_shape_ok(N, HW, C) ||
      !se_r_ok(C, R))
    return STP_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(se_excite_bwd_kernel, dim3(N), dim3(SE_THREADS), 0, st, workspace, se_chunks(N, HW), C, R, W1, W2, h, s, da2, da1, dz);
  STP_LAUNCH_CHECK();
  const int total = 2 * C * R + R + C;
  hipLaunchKernelGGL(se_param_grad_kernel, dim3(ceil_div(total, SE_THREADS)), dim3(SE_THREADS), 0, st, z, h, da2, da1, N, C, R, dW1, db1, dW2,
                     db2);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_se_bwd_apply(const void* dx, void* du, int32_t dtype, int32_t N, int64_t HW, int32_t C, const float* s, const float* dz,
                                void* stream) {
  if (!dx || !du || !s || !dz || !stp_dtype_ok(dtype) || !se_shape_ok(N, HW, C)) return STP_E_BADARG;
  const int chunks = se_chunks(N, HW), rpc = se_rpc(N, HW), items = N * chunks;
  hipStream_t st = (hipStream_t)stream;
  const float inv_hw = 1.f / (float)HW;
  if (dtype == STP_F32)
    hipLaunchKernelGGL((se_apply_kernel<float, false, false>), dim3(se_grid(items)), dim3(SE_THREADS), 0, st, (const float*)dx,
                       (const float*)nullptr, (float*)du, s, dz, inv_hw, (float*)nullptr, items, chunks, rpc, (int)HW, C);
  else
    hipLaunchKernelGGL((se_apply_kernel<bf16_t, false, false>), dim3(se_grid(items)), dim3(SE_THREADS), 0, st, (const bf16_t*)dx,
                       (const bf16_t*)nullptr, (bf16_t*)du, s, dz, inv_hw, (float*)nullptr, items, chunks, rpc, (int)HW, C);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

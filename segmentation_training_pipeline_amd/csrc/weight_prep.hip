// Weight-layout preparation (the 16-bit compute copies of the fp32 master weights, forward and data-gradient orientation, the
// class-collapsed copies of convolutions over a nearest-2x upsampled source), the weight-gradient unpadding, the stem beta gradient
// and the wire-format casts.  HBM-bound streaming kernels.
#include "common.h"
#include <cstdlib>

// ------------------------------------------------------------------------------------------
// weight compute copies.  master [Cout][KH][KW][Cin] fp32.
//   fwd [rows_f][KH][KWp][Cinp]  (rows_f = Cout rounded up to 16; zero padded)
//   bwd [rows_b][KH][KW][CoutB]  bwd[ci][kh][kw][co] = master[co][KH-1-kh][KW-1-kw][ci]
//                                (rows_b = Cin rounded up to 16, CoutB >= Cout; zero padded)
template <typename T>
__global__ __launch_bounds__(256) void weight_prepare_kernel(const float* __restrict__ w, T* __restrict__ fwd, T* __restrict__ bwd,
                                                             int Cout, int KH, int KW, int Cin, int KWp, int Cinp, int CoutB,
                                                             int rows_f, int rows_b) {
  const int64_t nf = fwd ? (int64_t)rows_f * KH * KWp * Cinp : 0;
  const int64_t nb = bwd ? (int64_t)rows_b * KH * KW * CoutB : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nf + nb; i += (int64_t)gridDim.x * 256) {
    if (i < nf) {
      int64_t r = i;
      const int ci = (int)(r % Cinp); r /= Cinp;
      const int kw = (int)(r % KWp); r /= KWp;
      const int kh = (int)(r % KH);
      const int co = (int)(r / KH);
      float v = 0.f;
      if (co < Cout && kw < KW && ci < Cin) v = w[(((int64_t)co * KH + kh) * KW + kw) * Cin + ci];
      Elem<T>::store(fwd + i, v);
    } else {
      int64_t r = i - nf;
      const int co = (int)(r % CoutB); r /= CoutB;
      const int kw = (int)(r % KW); r /= KW;
      const int kh = (int)(r % KH);
      const int ci = (int)(r / KH);
      float v = 0.f;
      if (co < Cout && ci < Cin) v = w[(((int64_t)co * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)) * Cin + ci];
      Elem<T>::store(bwd + (i - nf), v);
    }
  }
}

extern "C" int stp_weight_prepare(const float* master, void* fwd, void* bwd, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin,
                                  int32_t KWp, int32_t Cinp, int32_t CoutB, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!master || (!fwd && !bwd) || KWp < KW || Cinp < Cin || CoutB < Cout) return STP_E_BADARG;
  const int rows_f = round_up(Cout, 16), rows_b = round_up(Cin, 16);
  const int64_t total = (fwd ? (int64_t)rows_f * KH * KWp * Cinp : 0) + (bwd ? (int64_t)rows_b * KH * KW * CoutB : 0);
  int64_t g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == STP_H16)
    hipLaunchKernelGGL(weight_prepare_kernel<bf16_t>, dim3((int)g), dim3(256), 0, s, master, (bf16_t*)fwd, (bf16_t*)bwd, Cout, KH,
                       KW, Cin, KWp, Cinp, CoutB, rows_f, rows_b);
  else if (dtype == STP_F32)
    hipLaunchKernelGGL(weight_prepare_kernel<float>, dim3((int)g), dim3(256), 0, s, master, (float*)fwd, (float*)bwd, Cout, KH, KW,
                       Cin, KWp, Cinp, CoutB, rows_f, rows_b);
  else
    return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// All layers in one launch: desc[l] describes layer l, `start` is the running element count (fwd then bwd
// elements of every layer); a thread finds its layer by binary search.  Same arithmetic as the
// per-layer kernel above, 1 launch instead of ~50 per step.
struct WeightPrepDesc {
  const float* master;
  void* fwd;
  void* bwd;
  int64_t start;      // first global element index of this layer
  int32_t Cout, KH, KW, Cin, KWp, Cinp, CoutB, rows_f, rows_b, pad_;
};

// grid.y = layer; the workgroups of a layer stride over its (tap, 32-cout, 32-cin) units.  A unit is read once
// from the fp32 master (cin fastest: coalesced), held in LDS, and written twice: the forward copy in the same
// orientation and the data-gradient copy transposed (cout fastest) with the taps flipped - both coalesced.
// Padding (Cinp > Cin, KWp > KW, row padding to 16, CoutB > Cout) is written as zeros.
// 16-bit layers without padding (Cin a multiple of 64, Cout of 32: every layer that matters by bytes): a unit is (tap, 32 cout,
// 64 cin) - 16-byte loads of the fp32 master, 16-byte stores of BOTH copies (8 consecutive cin of a cout row forward, 8 consecutive
// cout of a cin row transposed).  Same rounding per element as the generic path below: bit-identical copies.
template <typename T>
__device__ __forceinline__ void weight_prepare_fast_layer(const WeightPrepDesc& d, float (*tile)[65]) {
  const int CT = d.Cout >> 5, IT = d.Cin >> 6, taps = d.KH * d.KW;
  const int units = taps * CT * IT;
  const int tid = threadIdx.x;
  T* fwd = reinterpret_cast<T*>(d.fwd);
  T* bwd = reinterpret_cast<T*>(d.bwd);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int it = u % IT, ct = (u / IT) % CT, tap = u / (IT * CT);
    const int kh = tap / d.KW, kw = tap - kh * d.KW;
    const int co0 = ct * 32, ci0 = it * 64;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int r = p * 16 + (tid >> 4), c4 = (tid & 15) * 4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(d.master + (((int64_t)(co0 + r) * d.KH + kh) * d.KW + kw) * d.Cin + ci0 + c4);
      tile[r][c4] = v.x; tile[r][c4 + 1] = v.y; tile[r][c4 + 2] = v.z; tile[r][c4 + 3] = v.w;
    }
    __syncthreads();
    if (fwd) {
      const int r = tid >> 3, c8 = (tid & 7) * 8;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(tile[r][c8 + 2 * e], tile[r][c8 + 2 * e + 1]);
      *reinterpret_cast<u32x4*>(fwd + (((int64_t)(co0 + r) * d.KH + kh) * d.KW + kw) * d.Cin + ci0 + c8) = o;
    }
    if (bwd) {
      const int ci = tid >> 2, c8 = (tid & 3) * 8;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(tile[c8 + 2 * e][ci], tile[c8 + 2 * e + 1][ci]);
      *reinterpret_cast<u32x4*>(bwd + (((int64_t)(ci0 + ci) * d.KH + (d.KH - 1 - kh)) * d.KW + (d.KW - 1 - kw)) * d.Cout + co0 + c8) = o;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void weight_prepare_batched_kernel(const WeightPrepDesc* __restrict__ desc, int nlayers, int64_t total) {
  __shared__ float tile[32][65];
  const WeightPrepDesc d = desc[blockIdx.y];
  if constexpr (sizeof(T) == 2) {
    if (!(d.Cin & 63) && !(d.Cout & 31) && d.Cinp == d.Cin && d.KWp == d.KW && d.CoutB == d.Cout && d.rows_f == d.Cout && d.rows_b == d.Cin &&
        !(reinterpret_cast<uintptr_t>(d.master) & 15) && !(reinterpret_cast<uintptr_t>(d.fwd) & 15) && !(reinterpret_cast<uintptr_t>(d.bwd) & 15)) {
      weight_prepare_fast_layer<T>(d, tile);
      return;
    }
  }
  const int co_ext = d.bwd ? (d.rows_f > d.CoutB ? d.rows_f : d.CoutB) : d.rows_f;
  const int ci_ext = d.bwd ? (d.Cinp > d.rows_b ? d.Cinp : d.rows_b) : d.Cinp;
  const int CT = (co_ext + 31) >> 5, IT = (ci_ext + 31) >> 5, taps = d.KH * d.KWp;
  const int units = taps * CT * IT;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  T* fwd = reinterpret_cast<T*>(d.fwd);
  T* bwd = reinterpret_cast<T*>(d.bwd);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int it = u % IT;
    const int ct = (u / IT) % CT;
    const int tap = u / (IT * CT);
    const int kh = tap / d.KWp, kw = tap - kh * d.KWp;
    const int co0 = ct * 32, ci0 = it * 32;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int co = co0 + ty + 8 * p, ci = ci0 + tx;
      float v = 0.f;
      if (co < d.Cout && kw < d.KW && ci < d.Cin) v = d.master[(((int64_t)co * d.KH + kh) * d.KW + kw) * d.Cin + ci];
      tile[ty + 8 * p][tx] = v;
      if (fwd && co < d.rows_f && ci < d.Cinp) Elem<T>::store(fwd + (((int64_t)co * d.KH + kh) * d.KWp + kw) * d.Cinp + ci, v);
    }
    __syncthreads();
    if (bwd && kw < d.KW) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int ci = ci0 + ty + 8 * p, co = co0 + tx;
        if (ci < d.rows_b && co < d.CoutB)
          Elem<T>::store(bwd + (((int64_t)ci * d.KH + (d.KH - 1 - kh)) * d.KW + (d.KW - 1 - kw)) * d.CoutB + co, tile[tx][ty + 8 * p]);
      }
    }
    __syncthreads();
  }
}

extern "C" size_t stp_weight_prepare_desc_bytes(void) { return sizeof(WeightPrepDesc); }

// Fills one host-side descriptor (the caller uploads the array to the device); returns the element count.
extern "C" int64_t stp_weight_prepare_desc_fill(void* desc_host, int32_t index, int64_t start, const float* master, void* fwd,
                                                void* bwd, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin, int32_t KWp,
                                                int32_t Cinp, int32_t CoutB) {
  WeightPrepDesc* d = reinterpret_cast<WeightPrepDesc*>(desc_host) + index;
  d->master = master; d->fwd = fwd; d->bwd = bwd; d->start = start;
  d->Cout = Cout; d->KH = KH; d->KW = KW; d->Cin = Cin; d->KWp = KWp; d->Cinp = Cinp; d->CoutB = CoutB;
  d->rows_f = round_up(Cout, 16); d->rows_b = round_up(Cin, 16); d->pad_ = 0;
  return (fwd ? (int64_t)d->rows_f * KH * KWp * Cinp : 0) + (bwd ? (int64_t)d->rows_b * KH * KW * CoutB : 0);
}

extern "C" int stp_weight_prepare_batched(const void* desc_dev, int32_t nlayers, int64_t total, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!desc_dev || nlayers <= 0 || total <= 0) return STP_E_BADARG;
  // grid.x workgroups per layer: the big layers (9.4 MB, 2304 units) grid-stride over them, the surplus workgroups of the small
  // layers exit at once (64 -> 256: the launch lasts as long as its largest layer, 130 -> see DESIGN)
  hipStream_t s = (hipStream_t)stream;
  static const int per_layer = getenv("STP_PREP_BLOCKS") ? atoi(getenv("STP_PREP_BLOCKS")) : 512;
  if (dtype == STP_H16)
    hipLaunchKernelGGL(weight_prepare_batched_kernel<bf16_t>, dim3(per_layer, nlayers), dim3(256), 0, s, (const WeightPrepDesc*)desc_dev, nlayers, total);
  else if (dtype == STP_F32)
    hipLaunchKernelGGL(weight_prepare_batched_kernel<float>, dim3(per_layer, nlayers), dim3(256), 0, s, (const WeightPrepDesc*)desc_dev, nlayers, total);
  else
    return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// Class-collapsed weights of a 3x3 convolution over a NEAREST-2x upsampled source (stp_conv_params.weight_up): for output parity
// (py, px) the taps that read the same low-resolution pixel are summed - rows (py, ty): (0,0) {0}, (0,1) {1,2}, (1,0) {0,1}, (1,1) {2}.
// out[row][c = py*2+px][t = ty*2+tx][ci], row < round_up(Cout, 16) (zero rows behind Cout); sums in fp32, one rounding.
struct UpcollapseDesc {     // 32 bytes (the host packs it as two pointers + four int32)
  const float* master;
  void* out;
  int32_t Cout, rows, C0, Ctot;
};

template <typename T>
__device__ __forceinline__ void weight_upcollapse_layer(const UpcollapseDesc& d, int64_t first, int64_t stride) {
  T* out = reinterpret_cast<T*>(d.out);
  if constexpr (sizeof(T) == 2) {
    // 8 consecutive input channels per thread (C0 and Ctot multiples of 8, 16-byte aligned rows): 16-byte loads and stores, 32-bit
    // index arithmetic; same fp32 sums in the same order, one rounding: bit-identical to the element-wise loop below
    if (!(d.C0 & 7) && !(d.Ctot & 7) && !(reinterpret_cast<uintptr_t>(d.master) & 15) && !(reinterpret_cast<uintptr_t>(d.out) & 15) &&
        (int64_t)d.rows * 16 * d.C0 < (1ll << 31)) {
      const uint32_t c8n = (uint32_t)d.C0 >> 3, n8 = (uint32_t)d.rows * 16u * c8n;
      for (uint32_t i = (uint32_t)first; i < n8; i += (uint32_t)stride) {
        const uint32_t q = i / c8n, ci = (i - q * c8n) * 8u, ct = q & 15u, co = q >> 4;
        const int py = ct >> 3, px = (ct >> 2) & 1, ty = (ct >> 1) & 1, tx = ct & 1;
        const int kh0 = (py == 0) ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), kh1 = (py == 0) ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
        const int kw0 = (px == 0) ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kw1 = (px == 0) ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if ((int)co < d.Cout)
          for (int kh = kh0; kh <= kh1; ++kh)
            for (int kw = kw0; kw <= kw1; ++kw) {
              const float* src = d.master + (((int64_t)co * 3 + kh) * 3 + kw) * d.Ctot + ci;
              v0 += *reinterpret_cast<const f32x4*>(src);
              v1 += *reinterpret_cast<const f32x4*>(src + 4);
            }
        *reinterpret_cast<u32x4*>(out + (size_t)i * 8) = u32x4{pack_bf16x2(v0.x, v0.y), pack_bf16x2(v0.z, v0.w), pack_bf16x2(v1.x, v1.y), pack_bf16x2(v1.z, v1.w)};
      }
      return;
    }
  }
  const int64_t n = (int64_t)d.rows * 16 * d.C0;
  for (int64_t i = first; i < n; i += stride) {
    const int ci = (int)(i % d.C0);
    const int ct = (int)((i / d.C0) & 15);
    const int co = (int)(i / ((int64_t)16 * d.C0));
    const int py = ct >> 3, px = (ct >> 2) & 1, ty = (ct >> 1) & 1, tx = ct & 1;
    const int kh0 = (py == 0) ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), kh1 = (py == 0) ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
    const int kw0 = (px == 0) ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kw1 = (px == 0) ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
    float v = 0.f;
    if (co < d.Cout)
      for (int kh = kh0; kh <= kh1; ++kh)
        for (int kw = kw0; kw <= kw1; ++kw) v += d.master[(((int64_t)co * 3 + kh) * 3 + kw) * d.Ctot + ci];
    Elem<T>::store(out + i, v);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void weight_upcollapse_kernel(UpcollapseDesc d) {
  weight_upcollapse_layer<T>(d, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}
// grid.y = layer (descriptor table on the device): ONE launch per step for all decoder stages
template <typename T>
__global__ __launch_bounds__(256) void weight_upcollapse_batched_kernel(const UpcollapseDesc* __restrict__ desc) {
  weight_upcollapse_layer<T>(desc[blockIdx.y], (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}

extern "C" int stp_weight_prepare_upcollapse(const float* master, void* weight_up, int32_t Cout, int32_t C0, int32_t C1, int32_t dtype,
                                             void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!master || !weight_up || Cout <= 0 || C0 <= 0 || C1 < 0) return STP_E_BADARG;
  UpcollapseDesc d;
  d.master = master; d.out = weight_up; d.Cout = Cout; d.rows = round_up(Cout, 16); d.C0 = C0; d.Ctot = C0 + C1;
  int64_t g = ((int64_t)d.rows * 16 * C0 + 255) / 256;
  if (g > 2048) g = 2048;
  if (dtype == STP_H16) hipLaunchKernelGGL(weight_upcollapse_kernel<bf16_t>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, d);
  else if (dtype == STP_F32) hipLaunchKernelGGL(weight_upcollapse_kernel<float>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, d);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" size_t stp_weight_prepare_upcollapse_desc_bytes(void) { return sizeof(UpcollapseDesc); }

// desc_dev: `nlayers` descriptors {const float* master; void* out; int32 Cout, rows (= Cout rounded up to 16), C0, C0 + C1} on the device
extern "C" int stp_weight_prepare_upcollapse_batched(const void* desc_dev, int32_t nlayers, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!desc_dev || nlayers <= 0) return STP_E_BADARG;
  const dim3 grid(256, nlayers);
  if (dtype == STP_H16) hipLaunchKernelGGL(weight_upcollapse_batched_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else if (dtype == STP_F32) hipLaunchKernelGGL(weight_upcollapse_batched_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// The data gradient w.r.t. the LOW-RESOLUTION source of such a convolution is a plain 4x4 / stride 2 / pad 1 convolution of dY:
// dX_lo[i] takes dY rows 2i-1 .. 2i+2 through the row-tap sums {2}, {1,2}, {0,1}, {0} of the 3x3 kernel (columns alike) - 16
// instead of 36 taps per low-resolution pixel, and neither the high-resolution gradient nor its 2x2 fold exist.  out = the weight
// matrix of that convolution, [round_up(C0, 16)][4][4][CoutB] (rows = input channels of the forward layer, zero padding).
// Descriptor: UpcollapseDesc with `rows` holding CoutB.
template <typename T>
__global__ __launch_bounds__(256) void weight_upcollapse_bwd_batched_kernel(const UpcollapseDesc* __restrict__ desc) {
  const UpcollapseDesc d = desc[blockIdx.y];
  const int CoutB = d.rows, rows = (d.C0 + 15) / 16 * 16;
  T* out = reinterpret_cast<T*>(d.out);
  const int64_t n = (int64_t)rows * 16 * CoutB;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int co = (int)(i % CoutB);
    const int rs = (int)((i / CoutB) & 15);
    const int ci = (int)(i / ((int64_t)16 * CoutB));
    const int r = rs >> 2, c = rs & 3;
    const int kh0 = r == 0 ? 2 : r == 1 ? 1 : 0, kh1 = r == 0 ? 2 : r == 1 ? 2 : r == 2 ? 1 : 0;
    const int kw0 = c == 0 ? 2 : c == 1 ? 1 : 0, kw1 = c == 0 ? 2 : c == 1 ? 2 : c == 2 ? 1 : 0;
    float v = 0.f;
    if (co < d.Cout && ci < d.C0)
      for (int kh = kh0; kh <= kh1; ++kh)
        for (int kw = kw0; kw <= kw1; ++kw) v += d.master[(((int64_t)co * 3 + kh) * 3 + kw) * d.Ctot + ci];
    Elem<T>::store(out + i, v);
  }
}

// desc_dev: nlayers records {const float* master; void* out; int32 Cout, CoutB, C0, C0 + C1} (32 bytes each) on the device
extern "C" int stp_weight_prepare_upcollapse_bwd_batched(const void* desc_dev, int32_t nlayers, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!desc_dev || nlayers <= 0) return STP_E_BADARG;
  const dim3 grid(256, nlayers);
  if (dtype == STP_H16) hipLaunchKernelGGL(weight_upcollapse_bwd_batched_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else if (dtype == STP_F32) hipLaunchKernelGGL(weight_upcollapse_bwd_batched_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// padded gradient [CoutP][KH][KWp][Cinp] -> master layout [Cout][KH][KW][Cin]
__global__ void weight_grad_unpad_kernel(const float* __restrict__ padded, float* __restrict__ grad, int Cout, int KH, int KW,
                                         int Cin, int KWp, int Cinp, int accumulate) {
  const int64_t n = (int64_t)Cout * KH * KW * Cin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ci = (int)(r % Cin); r /= Cin;
    const int kw = (int)(r % KW); r /= KW;
    const int kh = (int)(r % KH);
    const int co = (int)(r / KH);
    const float v = padded[(((int64_t)co * KH + kh) * KWp + kw) * Cinp + ci];
    grad[i] = accumulate ? grad[i] + v : v;
  }
}

extern "C" int stp_weight_grad_unpad(const float* padded, float* grad, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin,
                                     int32_t KWp, int32_t Cinp, int32_t accumulate, void* stream) {
  if (!padded || !grad) return STP_E_BADARG;
  int64_t g = ((int64_t)Cout * KH * KW * Cin + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(weight_grad_unpad_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, padded, grad, Cout, KH, KW, Cin,
                     KWp, Cinp, accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// Gradient of the beta of the input BatchNormalization (bn_data, scale=False) without a stem
// data-gradient pass.  The stem input carries a constant-one 4th channel, so the padded stem
// weight gradient holds S[co][kh][kw] = sum over valid taps of dY in channel slot `one_ch`;
//   dbeta[c] = sum_{co,kh,kw} W[co][kh][kw][c] * S[co][kh][kw].
__global__ void stem_beta_grad_kernel(const float* __restrict__ padded_dw, const float* __restrict__ w, float* __restrict__ dbeta,
                                      int Cout, int KH, int KW, int Cin, int KWp, int Cinp, int one_ch) {
  const int c = blockIdx.x;
  float a = 0.f;
  const int n = Cout * KH * KW;
  for (int i = threadIdx.x; i < n; i += 256) {
    int r = i;
    const int kw = r % KW; r /= KW;
    const int kh = r % KH;
    const int co = r / KH;
    a += w[(((int64_t)co * KH + kh) * KW + kw) * Cin + c] * padded_dw[(((int64_t)co * KH + kh) * KWp + kw) * Cinp + one_ch];
  }
  // 4 waves (the kernel is the tail of the backward pass: 3136 products per channel, latency-bound at 64 threads)
  __shared__ float red[4];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) dbeta[c] = ((red[0] + red[1]) + red[2]) + red[3];
}

extern "C" int stp_stem_beta_grad(const float* padded_dw, const float* master, float* dbeta, int32_t Cout, int32_t KH,
                                  int32_t KW, int32_t Cin, int32_t KWp, int32_t Cinp, int32_t one_ch, void* stream) {
  if (!padded_dw || !master || !dbeta || one_ch >= Cinp) return STP_E_BADARG;
  hipLaunchKernelGGL(stem_beta_grad_kernel, dim3(Cin), dim3(256), 0, (hipStream_t)stream, padded_dw, master, dbeta, Cout, KH, KW,
                     Cin, KWp, Cinp, one_ch);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
__global__ void cast_f32_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = f32_to_bf16(src[i]);
}
__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, int64_t count, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = bf16_to_f32(src[i]) * scale;
}
extern "C" int stp_cast_f32_to_bf16(const float* src, void* dst, int64_t count, void* stream) {
  if (!src || !dst || count <= 0) return STP_E_BADARG;
  int64_t g = (count + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, count);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
extern "C" int stp_cast_bf16_to_f32(const void* src, float* dst, int64_t count, float scale, void* stream) {
  if (!src || !dst || count <= 0) return STP_E_BADARG;
  int64_t g = (count + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, dst, count, scale);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_abi_version(void) { return 1; }
extern "C" int stp_storage_dtype(void) { return STP_H16; }

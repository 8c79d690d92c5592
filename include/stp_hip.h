/*
 * stp_hip.h - C-ABI of the MI355X-native segmentation training hot path (libstp_hip.so).
 *
 * Boundary contract (last row): the reference has no native layer at all - its
 * hot loop is Keras `fit_generator` over TF/cuDNN ops reached from
 * segmentation_pipeline/segmentation.py:35 (GenericImageTaskConfig.fit) and :155
 * (`clazz(**cleaned)` -> segmentation_models.Unet graph).  Each entry point below replaces the
 * TF op family named in its comment; the Python host mirror that binds them with ctypes lives
 * in segmentation_training_pipeline_amd/_lib.py, and INTEGRATION.md shows the reference-side
 * stub.
 *
 * Rules for every entry point:
 *   - plain pointers / ints / floats / hipStream_t only (passed as void*); no C++ or torch types;
 *   - the caller owns every buffer (device memory, 16-byte aligned); nothing here allocates;
 *   - stream-ordered, never synchronises, safe to capture into a hipGraph;
 *   - returns 0 on success, <0 on error (STP_E_*); never throws;
 *   - re-entrant on distinct streams/workspaces.
 *
 * Tensors: activations NHWC dense; dtype 0 = fp32, 1 = bf16 (storage of activations and of the
 * compute copies of weights; accumulation is always fp32; master weights/grads/optimizer
 * state are always fp32).
 */
#ifndef STP_HIP_H
#define STP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STP_OK 0
#define STP_E_BADARG (-1)
#define STP_E_LAUNCH (-2)
#define STP_E_WORKSPACE (-3)

#define STP_F32 0
#define STP_BF16 1
/* STP_U8 (2) is defined with the BatchNormalization entry points below. */
#define STP_F16 3   /* IEEE half storage + v_mfma_*_f16 (BASELINE.json configs[3] "fp16 MFMA").  The 16-bit storage format is a
                       BUILD parameter of the kernel set: libstp_hip.so serves STP_F32 and STP_BF16, libstp_hip_f16.so - the
                       same sources compiled with -DSTP_STORAGE_F16=1, same symbols - serves STP_F32 and STP_F16.  Every
                       "dtype" argument documented as bf16 below means "the library's 16-bit format".  fp16 needs loss scaling:
                       the loss entry points' grad_scale and the optimizers' gscale carry it (host: HipSegModel loss_scale). */

/* How src0 is resampled into the virtual input plane of the implicit GEMM gather. */
#define STP_SRC_DIRECT 0     /* virtual (h,w) = src (h,w)                                        */
#define STP_SRC_NEAREST2X 1  /* UpSampling2D(2): virtual (h,w) reads src (h/2,w/2)               */
#define STP_SRC_ZEROINS2X 2  /* zero-insertion: virtual (h,w) reads src (h/2,w/2) iff both even  */
                             /* (data-gradient of a stride-2 convolution)                        */

int stp_abi_version(void);
/* The 16-bit dtype code this library was built for: STP_BF16 (libstp_hip.so) or STP_F16 (libstp_hip_f16.so). */
int stp_storage_dtype(void);

/* ----------------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA.  Replaces keras.layers.Conv2D forward and the
 * Conv2DBackpropInput op of its gradient (reference call site segmentation.py:155 builds the
 * graph; schemas/segmentation.raml:158-178 names the decoder it produces).
 *
 * virtual input  V[n,h,w,c] = concat_c( resample(src0)[.., C0], src1[.., C1] ), h<Hv, w<Wv
 * out[n,ho,wo,co] = sum_{kh,kw,c} V[n, ho*stride - pad + kh, wo*stride - pad + kw, c]
 *                                 * weight[co][(kh*KW + kw)*(C0+C1) + c]
 *                   (+ bias[co]) (+ residual[n,ho,wo,co]) (ReLU if relu)
 * Output channels [0,Cd0) go to dst0 (row stride Cd0), [Cd0,Cout) to dst1 (row stride
 * Cout-Cd0); each destination either overwrites or accumulates (+=).
 * Constraints: C0, C1 multiples of 8 (bf16) / 4 (fp32), or C0 == 4 && C1 == 0 (stem, KW even);
 * Cd0 and Cout-Cd0 multiples of 4 unless Cout < 4 is handled by padding the weight rows
 * (Cout is then the number of valid rows; only those are stored).
 */
typedef struct stp_conv_params {
  const void* src0;     /* [N,Hs0,Ws0,C0]                       */
  const void* src1;     /* [N,Hv,Wv,C1] or NULL                 */
  const void* weight;   /* [Cout_pad][KH*KW*(C0+C1)] dtype      */
  const float* bias;    /* [Cout] or NULL                       */
  const void* residual; /* [N,Ho,Wo,Cout] dtype or NULL         */
  void* dst0;           /* [N,Ho,Wo,Cd0]                        */
  void* dst1;           /* [N,Ho,Wo,Cout-Cd0] or NULL           */
  int32_t N, Hs0, Ws0, Hv, Wv, C0, C1;
  int32_t src0_mode;    /* STP_SRC_*                            */
  int32_t KH, KW, stride, pad;
  int32_t Ho, Wo, Cout, Cd0;
  int32_t accumulate0, accumulate1, relu;
  int32_t dtype;        /* STP_F32 / STP_BF16                   */
  int32_t tile;         /* 0 = auto; else forces a tile config (testing/tuning) */
  int32_t stats_tiles;  /* OUT (written by stp_conv2d when stats_partial != NULL): number of pixel tiles */
  float* stats_partial; /* optional [2][Cout][pixel tiles] fp32: per-tile sum / sum of squares of the stored
                           output per channel (fused BatchNormalization statistics, finalize with
                           stp_bn_finalize); capacity >= stp_conv2d_stats_floats(p) floats */
  /* BatchNormalization-backward fusion for a data-gradient convolution whose destination is dY of a BN(+ReLU)
   * output and which COMPLETES that gradient - the only consumer of the BN output, or the last one to contribute
   * (accumulate0 = 1 on top of what the other consumers wrote): with bnb_x != NULL (the BN INPUT, [N,Ho,Wo,Cout] dtype)
   * the epilogue stores g = dY * [bn(x) > 0] (g = dY when bnb_relu == 0) instead of dY and writes
   * stats_partial = per-tile sum(g) / sum(g * xhat) per channel; finish with stp_bn_backward_fused.  Requires
   * stats_partial, Cd0 == Cout, Cout % 4 == 0, no relu / residual. */
  const void* bnb_x;
  const float* bnb_mean;
  const float* bnb_rstd;
  const float* bnb_gamma; /* NULL: scale=False */
  const float* bnb_beta;  /* NULL: center=False */
  int32_t bnb_relu;
  /* Gradient of UpSampling2D(2) folded into the epilogue of the data-gradient convolution whose (virtual) destination
   * is the upsampled tensor: with dst_sum2x2 != 0, dst0 is [N,Ho/2,Wo/2,Cout] and receives the sum of each 2x2 block
   * (the hi-res gradient is never written); bnb_x / stats_partial / accumulate0 then refer to that low-resolution
   * tensor.  Small-channel kernel (stp_conv2d_sc_eligible), Ho and Wo even, no bias / relu - and, for 64+ channels, the halo kernel
   * in its fused form (bnb_x set, Cd0 a multiple of the variant's channel tile: conv_halo.hip's EP 3, with or without dst1).
   * With a second destination (dst1 != NULL: the data gradient of conv3x3(concat(UpSampling2D(2)(x), skip)), served by the
   * wide-output kernel, stp_conv2d_scw_eligible, or by the halo kernel) only dst0 - the first Cd0 channels - is summed, and bnb_x / stats_partial
   * refer to those Cd0 channels; dst1 stays [N,Ho,Wo,Cout-Cd0]. */
  int32_t dst_sum2x2;
  /* stats_slots > 0 (a power of two <= 64): stats_partial points to PRE-ZEROED int64 fixed-point slots [2][Cout][stats_slots]
   * (2^-24 units) and every pixel tile ADDS its sums atomically into slot (tile % stats_slots) - integer addition, hence
   * order-independent and deterministic - instead of writing a per-tile partial: no finalize kernel; the consumer
   * (stp_bn_apply_slots / stp_bn_backward_slots) sums the few slots of each channel in its prologue. */
  int32_t stats_slots;
  /* Fused PRODUCER BatchNormalization (small-channel kernel and halo kernel only): src_bn_mean != NULL means src0 holds the tensor BEFORE a
   * training-phase BatchNormalization (+ activation src_bn_relu: 0 none, 1 ReLU, 2 ReLU6).  The kernel normalises it while
   * staging its halo tile, with the arithmetic and rounding of stp_bn_apply, so the result equals the unfused pair bit for
   * bit and the normalised tensor is never written to HBM.  Padding stays zero (it pads the NORMALISED tensor). */
  const float* src_bn_mean;
  const float* src_bn_rstd;
  const float* src_bn_gamma; /* may be NULL */
  const float* src_bn_beta;  /* may be NULL */
  int32_t src_bn_relu;
  /* Optional class-collapsed weights for a NEAREST-2x source (uniform-tap kernel, forward of the decoder convolutions over
   * UpSampling2D(2) + concat): for output parity class (py, px) the nine taps over the upsampled src0 read only 2 x 2 distinct
   * low-resolution pixels, so with weight_up = [Cout_pad][4 classes][2][2][C0] (stp_weight_prepare_upcollapse: the 3x3 taps that
   * share a pixel summed) the K loop takes 4 x C0 + 9 x C1 instead of 9 x (C0 + C1) steps.  NULL: the plain gather. */
  const void* weight_up;
  /* Data gradient of a 1x1 / stride-2 SHORTCUT folded into the data gradient of its sibling 3x3 / stride-2 / pad-1 convolution (both
   * read the same tensor, ResNet basic block with a projection shortcut): in the parity-class order of that launch the shortcut
   * touches only the (even, even) class, where it is one more tap - fold_src = dY of the shortcut ([N,Hs0,Ws0,fold_C], fold_C == C0),
   * fold_weight = its data-gradient weight copy [round_up(Cout,16)][fold_C] (rows = channels of the shared input).  The K loop of
   * that class runs fold_C / 64 more tiles; no separate launch reads and rewrites the whole gradient tensor.  Honoured only where
   * stp_conv2d_fold_ok(p) != 0 (STP_E_BADARG otherwise). */
  const void* fold_src;
  const void* fold_weight;
  int32_t fold_C;
  /* GROUP-LEVEL PRE-REDUCTION of the fused sums (round 5).  stats_group = G > 1: the pixel tiles of a channel tile are taken in groups
   * of G consecutive tiles; every workgroup publishes its column of stats_partial write-through and draws an arrival ticket from
   * stats_group_counters[channel tile x groups] (uint32, ZERO before the first launch; the launch leaves them at zero); the workgroup
   * that draws the last ticket of a group sums the group's columns IN TILE ORDER (fixed order: deterministic, replay bit-identical)
   * into stats_group_out = [2][C][ceil(tiles / G)].  The table the BatchNormalization reads then has <= 128 columns, which
   * stp_bn_finalize_apply / the one-launch form of stp_bn_backward_fused reduce in their prologue: no finalize launch on the chain
   * conv -> finalize -> apply -> conv.  G must be stp_conv2d_stats_group_for(p) (0 = this shape's kernel has no such epilogue). */
  float* stats_group_out;
  uint32_t* stats_group_counters;
  int32_t stats_group;
  /* SPACE-TO-DEPTH data gradient of a 3x3 / stride-2 / pad-1 convolution (+ its sibling 1x1 / stride-2 projection shortcut), round 5.
   * s2d_dgrad = 1 describes ONE dense launch for the four output parity classes: src0 = dY of the 3x3 layer [N,Ho,Wo,C0], src1 = dY of
   * the shortcut [N,Ho,Wo,C1] or NULL, KH = KW = 2, stride 1, pad 0 (tap (da, db) reads (a + da, b + db); past the bottom / right
   * edge = zero), Cout = 4 x Cq output channels in parity-class-major order (class cls = py * 2 + px), dst0 = [N,2Ho,2Wo,Cq]: channel
   * cls * Cq + c of pixel (a, b) is
   * stored as channel c of pixel (2a + (cls >> 1), 2b + (cls & 1)).  accumulate0, bnb_x (+ stats_partial = [2][Cq][4 x tiles]: four
   * column blocks per channel, stp_conv2d_stats_floats counts them) refer to that destination.  NO weight copy of its own: weight = the
   * 3x3 layer's ordinary data-gradient copy [Cq^16][3][3][C0] (stp_weight_prepare's `bwd`), fold_weight = the shortcut's [Cq^16][C1]
   * (required when C1 > 0) - the kernel addresses, per output row, the kernel tap its class meets under each of the 2 x 2 taps
   * (9 of the 16 (tap, class) blocks are live; the dead ones move no bytes and issue no MFMAs).  Served by the halo kernel only:
   * stp_conv2d_halo_variant(p) >= 0 tells. */
  int32_t s2d_dgrad;
} stp_conv_params;
/* Group size G (a power of two, >= 2) for which stp_conv2d(p) can pre-reduce its stats_partial columns to <= 128 (see stats_group), or 0
 * when the table is small enough already / the kernel that serves p has no such epilogue.  stp_conv2d_stats_group_counters(p, G) =
 * uint32 words stats_group_counters must hold. */
int stp_conv2d_stats_group_for(const stp_conv_params* p);
size_t stp_conv2d_stats_group_counters(const stp_conv_params* p, int32_t G);
/* 1: stp_conv2d(p) takes the parity-class path that honours fold_src / fold_weight / fold_C for this shape (p->fold_* need not be set). */
int stp_conv2d_fold_ok(const stp_conv_params* p);

int stp_conv2d(const stp_conv_params* p, void* stream);
/* weight_up of stp_conv_params from the fp32 master [Cout][3][3][C0 + C1]: rows = Cout rounded up to 16 (zero rows behind Cout),
 * class c = py * 2 + px, tap t = ty * 2 + tx; row taps of (py, ty): (0,0) {0}, (0,1) {1,2}, (1,0) {0,1}, (1,1) {2}; columns alike. */
int stp_weight_prepare_upcollapse(const float* master, void* weight_up, int32_t Cout, int32_t C0, int32_t C1, int32_t dtype,
                                  void* stream);
/* The same for several layers in ONE launch: desc_dev = nlayers records {const float* master; void* weight_up; int32 Cout, rows
 * (= Cout rounded up to 16), C0, C0 + C1} (stp_weight_prepare_upcollapse_desc_bytes() = 32 bytes each) in device memory. */
size_t stp_weight_prepare_upcollapse_desc_bytes(void);
int stp_weight_prepare_upcollapse_batched(const void* desc_dev, int32_t nlayers, int32_t dtype, void* stream);
/* Data gradient w.r.t. the low-resolution source of such a layer = a 4x4 / stride 2 / pad 1 convolution of dY (stp_conv2d, DIRECT
 * source): this builds its weights [round_up(C0, 16)][4][4][CoutB] from the master - row taps {2}, {1,2}, {0,1}, {0} of the 3x3
 * kernel summed, columns alike.  desc_dev: nlayers records {const float* master; void* out; int32 Cout, CoutB, C0, C0 + C1}. */
int stp_weight_prepare_upcollapse_bwd_batched(const void* desc_dev, int32_t nlayers, int32_t dtype, void* stream);
/* floats needed by stats_partial for this shape (tile choice included) */
size_t stp_conv2d_stats_floats(const stp_conv_params* p);
/* tile configuration stp_conv2d would pick for p (see conv_igemm.hip: 1..6 register-staged tiles, 32*STAGES+t
 * uniform-tap DMA tiles, 256+t per-lane-tap DMA tiles, 512 small-channel kernel, 768 stem kernel, 1024+v halo kernel); used by bench.py. */
int stp_conv2d_tile_for(const stp_conv_params* p);
/* Small-channel path (Cin <= 32, Cout <= 32, 3x3 stride 1 pad 1, single source, optional nearest-2x):
 * an 8x32 output tile per workgroup with the input halo tile staged once in LDS (conv_sc.hip).
 * stp_conv2d uses it automatically when stp_conv2d_sc_eligible(p) != 0 (tile id 512). */
int stp_conv2d_sc_eligible(const stp_conv_params* p);
/* Columns of the [stat][channel][column] partial sums the small-channel kernel writes for p (what stats_tiles will report):
 * one per 8x32 tile, or one per persistent workgroup in the streaming form. */
int stp_conv2d_sc_stats_tiles(const stp_conv_params* p);
int stp_conv2d_sc(const stp_conv_params* p, void* stream);
/* Wide-output form of the small-channel kernel (conv_sc_wide.hip: conv_scw_stream_kernel): 3x3 / stride 1 / pad 1, 32 input channels,
 * 128 output channels split over dst0 (Cd0 channels, a multiple of 32, dst_sum2x2 = 1: low-resolution, optional bnb_x + stats_partial)
 * and dst1 (full resolution); 16-bit storage.  Replaces the generic per-tap data gradient of decoder_stage3_conv1 + stp_upsample2x_bwd
 * (TF: Conv2DBackpropInput + ResizeNearestNeighborGrad + FusedBatchNormGrad's reductions).  stp_conv2d uses it automatically
 * (tile id 640; STP_SCW=0 in the environment switches it off).  stats_tiles = stp_conv2d_scw_stats_tiles(p) columns of [2][Cd0][columns]. */
int stp_conv2d_scw_eligible(const stp_conv_params* p);
int stp_conv2d_scw_stats_tiles(const stp_conv_params* p);
int stp_conv2d_scw(const stp_conv_params* p, void* stream);
/* Narrow-output form (conv_sc_narrow.hip: conv_scn_stream_kernel): the FORWARD of Conv2D(32, 3x3)(Concatenate([UpSampling2D(2)(x), skip])) with 64 + 64
 * input channels (src0 = x at half resolution, src0_mode = STP_SRC_NEAREST2X, src1 = skip), 16-bit storage: both halos resident in LDS (x as its
 * low-resolution pixels), all weights in registers, one wave per SIMD.  Takes `weight` (the plain forward copy [32][3][3][128]); weight_up is
 * ignored.  bias / relu / accumulate0 / stats_partial as for stp_conv2d.  stp_conv2d uses it automatically (tile id 704; STP_SCN=0 switches it
 * off).  stats_tiles = stp_conv2d_scn_stats_tiles(p) columns. */
int stp_conv2d_scn_eligible(const stp_conv_params* p);
int stp_conv2d_scn_stats_tiles(const stp_conv_params* p);
int stp_conv2d_scn(const stp_conv_params* p, void* stream);
/* 64 -> 64 channels, 3x3 / stride 1 / pad 1, 16-bit storage, single source and destination (conv_sc_s64.hip: conv_s64_stream_kernel; ResNet stage 1
 * forward and data gradient): the whole weight matrix in the registers of every wave, the halo double-buffered in LDS.  residual, or stats_partial,
 * or bnb_x + stats_partial; no bias / relu / accumulate.  OPT-IN (tile id 736, or STP_S64=1 in the environment for stp_conv2d's automatic choice
 * when the launch has at least two tiles of 8 x 32 pixels per CU): at the U-Net's batch the halo kernel is as fast (conv_sc_s64.hip has the numbers).
 * stats_tiles = stp_conv2d_s64_stats_tiles(p) columns (one per workgroup). */
int stp_conv2d_s64_eligible(const stp_conv_params* p);
int stp_conv2d_s64_stats_tiles(const stp_conv_params* p);
int stp_conv2d_s64(const stp_conv_params* p, void* stream);
/* The ResNet stem (classification_models conv0: 7x7 / stride 2 / pad 3, 3+1 input channels -> 64, bf16): halo-tile kernel,
 * used by stp_conv2d automatically when eligible (tile id 768); optional fused BatchNormalization sums (stats_partial). */
int stp_conv2d_stem_eligible(const stp_conv_params* p);
int stp_conv2d_stem(const stp_conv_params* p, void* stream);
/* Halo-resident 3x3 kernel (conv_halo.hip; bf16, stride 1, pad 1, one direct source, Cin % 64 == 0, Cout % 16 == 0, Wo % 16 == 0,
 * Ho % 8 == 0): a workgroup keeps the (TH+2) x 18 input pixels of its TH x 16 output block resident in LDS per 64-channel slab and
 * streams only the weights.  Tile ids 1024 + variant (0: 16x16 px x 128 channels, 1: 8x16 x 128, 2: 16x16 x 64, 3: 8x16 x 64);
 * stp_conv2d picks it automatically where it measured faster (stp_conv2d_halo_variant(p) >= 0 with p->tile == 0; the environment
 * variable STP_HALO=0 disables the automatic choice).  It is the one GEMM-class kernel that honours src_bn_*: the producer
 * BatchNormalization (+activation) is applied in LDS, bit-identical to stp_bn_apply.  stp_conv2d_halo_tiles = pixel tiles
 * (= stats_partial columns) of a variant. */
int stp_conv2d_halo_variant(const stp_conv_params* p);
int stp_conv2d_halo_tiles(const stp_conv_params* p, int variant);
int stp_conv2d_halo(const stp_conv_params* p, int variant, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Weight gradient (Conv2DBackpropFilter).  dW[co][(kh*KW+kw)*(C0+C1)+c] =
 *   sum_{n,ho,wo} dY[n,ho,wo,co] * V[n, ho*stride-pad+kh, wo*stride-pad+kw, c]
 * with V gathered exactly as in stp_conv2d.  Pixels are split over `splits` slabs written to
 * `workspace` ([splits][Cout][K] fp32) and reduced in fixed order (deterministic).
 * dW is fp32 [Cout][K]; accumulate != 0 adds to it.
 */
typedef struct stp_wgrad_params {
  const void* src0;
  const void* src1;
  const void* dy;       /* [N,Ho,Wo,Cout] dtype */
  float* dw;            /* [Cout][K] fp32       */
  int32_t N, Hs0, Ws0, Hv, Wv, C0, C1, src0_mode;
  int32_t KH, KW, stride, pad;
  int32_t Ho, Wo, Cout;
  int32_t accumulate;
  int32_t dtype;
  int32_t splits;       /* 0 = auto */
  /* as stp_conv_params.src_bn_*: src0 is the pre-normalisation tensor (small-channel and row-of-taps weight gradients - single-layer
   * and grouped launches -, C1 == 0 only) */
  const float* src_bn_mean;
  const float* src_bn_rstd;
  const float* src_bn_gamma;
  const float* src_bn_beta;
  int32_t src_bn_relu;
} stp_wgrad_params;

size_t stp_conv2d_wgrad_workspace_bytes(const stp_wgrad_params* p);
int stp_conv2d_wgrad(const stp_wgrad_params* p, void* workspace, size_t workspace_bytes, void* stream);
/* The two phases of stp_conv2d_wgrad as separate launches (so that a profiler / the plan can time them
 * individually).  variant: 0 = auto, 1 = register-staged kernel, 2 / 3 = buffer-DMA ring with 2 / 3 stages,
 * 4 = row-of-taps kernel (bf16, 3x3 / stride 1 / pad 1, C0 % 64 == 0 and C1 % 64 == 0, src0 direct or nearest-2x, Wo a multiple
 * of 64 or a power of two >= 16 with Ho * Wo % 64 == 0; STP_E_BADARG otherwise). */
int stp_conv2d_wgrad_partial(const stp_wgrad_params* p, void* workspace, size_t workspace_bytes, int32_t variant, void* stream);
int stp_conv2d_wgrad_reduce(const stp_wgrad_params* p, const void* workspace, int32_t variant, void* stream);
/* Small-channel weight gradient (conv_sc_wgrad.hip): chosen automatically by variant 0 when eligible. */
int stp_wgrad_sc_eligible(const stp_wgrad_params* p);
int stp_wgrad_sc_slabs(const stp_wgrad_params* p);
int stp_wgrad_sc_partial(const stp_wgrad_params* p, void* workspace, void* stream);
/* Which kernel family variant 0 launches for p: 0 = pixel-reduction GEMM (conv_wgrad_kernel / conv_wgrad_dma_kernel),
 * 1 = small-channel halo kernel, 2 / 3 = row-of-taps kernel with 128 / 64 output channels per workgroup. */
int stp_conv2d_wgrad_kernel_id(const stp_wgrad_params* p);

/* Grouped weight gradient (row-of-taps kernel): ONE partial launch + ONE reduce launch for several layers (the 3x3 / stride-1
 * layers of a network stage).  A layer launched alone offers 6-96 output tiles to 512-768 workgroup slots, so its pixel reduction
 * is split 5-85 ways (~12 steps per workgroup, one 96 KB partial slab each); the group's (layer, tile, step) space is cut into one
 * contiguous chunk per workgroup slot instead (fixed partition -> deterministic), a tile is covered by 1-3 partial slabs.
 *   stp_wgrad_group_class        : 0 = the layer cannot join a group; otherwise the class (32 / 64 / 128 output channels per tile) -
 *                                  the layers of one group must share it
 *   stp_wgrad_group_table_bytes  : size of the descriptor table of a group (0: invalid group)
 *   stp_wgrad_group_workspace_bytes : size of the partial slabs
 *   stp_wgrad_group_build        : fills the HOST copy of the table (it holds the layers' device pointers: build it when src0 / src1 /
 *                                  dy / dw are final); the caller copies it to device memory
 *   stp_wgrad_group_partial / _reduce : the two launches; host_table (header read on the host) and its device copy
 * Layers may carry src_bn_* (C1 == 0, directly read src0): the group then runs the kernel instance that normalises those layers' halo
 * tiles in LDS (per-layer switch; header word 14 of the table says which instance the group uses). */
int stp_wgrad_group_class(const stp_wgrad_params* p);
size_t stp_wgrad_group_table_bytes(const stp_wgrad_params* const* layers, int32_t n);
size_t stp_wgrad_group_workspace_bytes(const stp_wgrad_params* const* layers, int32_t n);
int stp_wgrad_group_build(const stp_wgrad_params* const* layers, int32_t n, void* host_table, size_t table_bytes);
int stp_wgrad_group_partial(const void* host_table, const void* dev_table, void* workspace, size_t workspace_bytes, void* stream);
int stp_wgrad_group_reduce(const void* host_table, const void* dev_table, const void* workspace, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Compute copies of a convolution kernel from the fp32 master (layout [Cout][KH][KW][Cin]):
 *   fwd : [Cout_pad16][KH][KWp][Cinp] dtype, zero padded (operand of stp_conv2d / layout of dW)
 *   bwd : [Cin_pad16][KH][KW][CoutB]  dtype, spatially flipped and transposed, zero padded
 *         (operand of the data-gradient GEMM: stp_conv2d over dY with pad' = K-1-pad)
 * Either pointer may be NULL.  stp_weight_grad_unpad copies a padded gradient
 * [Cout..][KH][KWp][Cinp] back to the master layout.  stp_stem_beta_grad: see weight_prep.hip.
 */
int stp_weight_prepare(const float* master, void* fwd, void* bwd, int32_t Cout, int32_t KH, int32_t KW,
                       int32_t Cin, int32_t KWp, int32_t Cinp, int32_t CoutB, int32_t dtype, void* stream);
/* All layers of a network in ONE launch: the caller fills a host array of opaque descriptors
 * (stp_weight_prepare_desc_bytes() each) with stp_weight_prepare_desc_fill - `start` = running sum of the
 * returned element counts - uploads it, and replays stp_weight_prepare_batched every step. */
size_t stp_weight_prepare_desc_bytes(void);
int64_t stp_weight_prepare_desc_fill(void* desc_host, int32_t index, int64_t start, const float* master, void* fwd, void* bwd,
                                     int32_t Cout, int32_t KH, int32_t KW, int32_t Cin, int32_t KWp, int32_t Cinp, int32_t CoutB);
int stp_weight_prepare_batched(const void* desc_dev, int32_t nlayers, int64_t total, int32_t dtype, void* stream);
int stp_weight_grad_unpad(const float* padded, float* grad, int32_t Cout, int32_t KH, int32_t KW,
                          int32_t Cin, int32_t KWp, int32_t Cinp, int32_t accumulate, void* stream);
int stp_stem_beta_grad(const float* padded_dw, const float* master, float* dbeta, int32_t Cout, int32_t KH,
                       int32_t KW, int32_t Cin, int32_t KWp, int32_t Cinp, int32_t one_ch, void* stream);

/* ----------------------------------------------------------------------------------------------
 * BatchNormalization (Keras semantics: biased batch variance for the normalisation, unbiased
 * for the moving variance, momentum on the moving stats).  Replaces keras BatchNormalization /
 * tf.nn.fused_batch_norm + ReLU, forward and gradient.
 *   stp_bn_stats     : per-channel mean and rstd (= 1/sqrt(var+eps)) over `rows` = N*H*W, plus the
 *                      moving-stat update (either may be NULL).  workspace: stp_bn_workspace_bytes.
 *   stp_bn_apply     : y = (x-mean)*rstd*gamma + beta, optional ReLU.  For uint8 input
 *                      (xdtype = STP_U8, C <= 4, the raw image) Cy must be 4 and the padded
 *                      channels are written as pad_value; otherwise Cy == C and xdtype == ydtype.
 *   stp_bn_inference : same with rstd derived from the moving variance.
 *   stp_bn_backward  : dy is the gradient w.r.t. the (post-ReLU) output; the ReLU mask is
 *                      re-derived from x (same single-fma affine as the forward).  Produces dx
 *                      (optionally accumulating) and the raw sums dgamma / dbeta (may be NULL).
 * gamma and beta may be NULL (scale=False / center=False).
 */
#define STP_U8 2
size_t stp_bn_workspace_bytes(int32_t C);
/* The slot forms (stp_conv_params.stats_slots): statistics -> mean / rstd (published for the backward pass), moving statistics
 * and the normalisation + activation in ONE kernel; and the BatchNormalization backward from bnb slots in ONE kernel. */
int stp_bn_apply_slots(const void* x, void* y, int32_t dtype, int64_t rows, int32_t C, const int64_t* slots, int32_t nslots,
                       float eps, float momentum, float* mean, float* rstd, float* moving_mean, float* moving_var,
                       const float* gamma, const float* beta, int32_t relu, void* stream);
int stp_bn_backward_slots(const void* x, const void* g, void* dx, int32_t dtype, int64_t rows, int32_t C, const float* mean,
                          const float* rstd, const float* gamma, const int64_t* slots, int32_t nslots, float* dgamma,
                          float* dbeta, int32_t accumulate_dx, void* stream);
/* zero-fill (the slot arena, once per step); p and bytes 16-byte aligned */
int stp_zero_bytes(void* p, int64_t bytes, void* stream);
/* second half of stp_bn_backward when the partial sums came from a convolution epilogue (stp_conv_params.bnb_x):
 * g is the masked gradient that epilogue stored, partial its [2][C][tiles] sums. */
int stp_bn_backward_fused(const void* x, const void* g, void* dx, int32_t dtype, int64_t rows, int32_t C,
                          const float* mean, const float* rstd, const float* gamma, const float* partial, int32_t tiles,
                          float* dgamma, float* dbeta, int32_t accumulate_dx, void* workspace, size_t workspace_bytes,
                          void* stream);
/* stp_bn_finalize + stp_bn_apply as ONE launch (16-bit dtype, C % 64 == 0, tiles <= 128; stp_bn_finalize_apply_ok tells): every
 * workgroup of the apply pass owns a 64-channel slab x a chunk of rows and reduces the [2][64][tiles] partial sums of its slab
 * itself (fp64, fixed order - all workgroups of a slab normalise with bit-identical constants), the first chunk of a slab also
 * writes mean / rstd / the moving statistics.  stp_bn_backward_fused(_add) takes the same one-launch form where eligible. */
int stp_bn_finalize_apply_ok(int32_t dtype, int64_t rows, int32_t C, int32_t tiles);
int stp_bn_finalize_apply(const float* partial, int32_t tiles, const void* x, void* y, int32_t dtype, int64_t rows, int32_t C,
                          float eps, float momentum, float* mean, float* rstd, float* moving_mean, float* moving_var,
                          const float* gamma, const float* beta, int32_t relu, void* stream);
/* the same with the accumulated addend in ANOTHER buffer: dx = result + dadd when accumulate_dx (dadd is left intact - a residual
 * gradient that a grouped weight gradient, stp_wgrad_group_partial, still reads as its dY); dadd == dx is the in-place form above */
int stp_bn_backward_fused_add(const void* x, const void* g, void* dx, const void* dadd, int32_t dtype, int64_t rows, int32_t C,
                              const float* mean, const float* rstd, const float* gamma, const float* partial, int32_t tiles,
                              float* dgamma, float* dbeta, int32_t accumulate_dx, void* workspace, size_t workspace_bytes,
                              void* stream);
int stp_bn_stats(const void* x, int32_t xdtype, int64_t rows, int32_t C, float eps, float momentum,
                 float* mean, float* rstd, float* moving_mean, float* moving_var,
                 void* workspace, size_t workspace_bytes, void* stream);
/* second half of stp_bn_stats for statistics produced by a convolution epilogue (stats_partial) */
int stp_bn_finalize(const float* partial, int32_t tiles, int64_t rows, int32_t C, float eps, float momentum,
                    float* mean, float* rstd, float* moving_mean, float* moving_var, void* stream);
int stp_bn_apply(const void* x, int32_t xdtype, void* y, int32_t ydtype, int64_t rows, int32_t C, int32_t Cy,
                 const float* mean, const float* rstd, const float* gamma, const float* beta,
                 int32_t relu, float pad_value, void* stream);
int stp_bn_inference(const void* x, int32_t xdtype, void* y, int32_t ydtype, int64_t rows, int32_t C, int32_t Cy,
                     const float* moving_mean, const float* moving_var, float eps,
                     const float* gamma, const float* beta, int32_t relu, float pad_value, void* stream);
int stp_bn_backward(const void* x, const void* dy, void* dx, int32_t dtype, int64_t rows, int32_t C,
                    const float* mean, const float* rstd, const float* gamma, const float* beta,
                    float* dgamma, float* dbeta, int32_t relu, int32_t accumulate_dx,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ZeroPadding2D(1) + MaxPooling2D(3, strides 2, 'valid') (classification_models ResNet stem).
 * idx [N,Ho,Wo,C] uint8 records kh*3+kw of the first maximum (padded taps compete with value 0);
 * the gradient routes dy through it (TF MaxPoolGrad behaviour). */
int stp_maxpool3x3s2(const void* x, void* y, uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C,
                     int32_t dtype, void* stream);
int stp_maxpool3x3s2_bwd(const uint8_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                         int32_t dtype, int32_t accumulate, void* stream);
/* stp_bn_apply (+ activation) and the stp_maxpool3x3s2 that follows it as ONE launch (the ResNet stem: bn0 -> relu0 -> pooling0): x = the
 * tensor before the BatchNormalization, yb = the normalised tensor (written, bit-identical to stp_bn_apply's - other layers read it),
 * y / idx = the pooling outputs.  16-bit storage, H and W even, C % 8 == 0. */
int stp_bn_apply_maxpool3x3s2(const void* x, void* yb, void* y, uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype,
                              const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t relu, void* stream);
/* The same when dx is the gradient of a BatchNormalization(+activation) output that this launch completes (bn0 of the ResNet
 * stem: pooled, and read by a decoder skip): mask + partial sums for stp_bn_backward_fused, as stp_upsample2x_bwd_bn. */
int stp_maxpool3x3s2_bwd_bn_tiles(int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype);
int stp_maxpool3x3s2_bwd_bn(const uint8_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype,
                            int32_t accumulate, const void* bn_x, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, int32_t relu, float* partial, void* stream);
/* MaxPooling2D(2, 2), no padding (keras.applications VGG blocks; H and W even).  idx = 2*dy+dx of the first maximum. */
int stp_maxpool2x2(const void* x, void* y, uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
int stp_maxpool2x2_bwd(const uint8_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype,
                       int32_t accumulate, void* stream);
/* AveragePooling2D(pool = strides = k), H % k == W % k == 0 (PSPNet pyramid pooling) and its gradient dx = dy / k^2.
 * Large windows over few outputs are reduced in two fixed-order stages through `workspace` (fp32 partials; size from the
 * query, 0 = not needed); without it the single-stage kernel runs. */
size_t stp_avgpool_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k);
int stp_avgpool(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t dtype, void* workspace,
                size_t workspace_bytes, void* stream);
int stp_avgpool_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t dtype,
                    int32_t accumulate, void* stream);
/* PSPNet's pyramid pooling (segmentation_models 0.2.1 psp builder: AveragePooling2D(size / level) of ONE feature map for levels 1, 2, 3, 6;
 * schemas/segmentation.raml:225-249) in one pass over the feature map: up to four levels y_i [N][H / k_i][W / k_i][C], k0 the FINEST window
 * (smallest k), every other k_i a multiple of k0 (k_i = 0: level unused) - the means are formed from the fp32 sums of the finest windows, one
 * rounding per output as stp_avgpool.  _bwd: dx (+)= sum_i dy_i / k_i^2 in one pass.  _ok: 1 if the pyramid form serves the shape
 * (STP_POOL_PYRAMID=0: never); workspace >= stp_avgpool_pyramid_workspace_bytes(). */
int stp_avgpool_pyramid_ok(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k0, int32_t k1, int32_t k2, int32_t k3, int32_t dtype);
size_t stp_avgpool_pyramid_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k0, int32_t dtype);
int stp_avgpool_pyramid(const void* x, void* y0, void* y1, void* y2, void* y3, int32_t k0, int32_t k1, int32_t k2, int32_t k3, int32_t N,
                        int32_t H, int32_t W, int32_t C, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);
int stp_avgpool_pyramid_bwd(const void* dy0, const void* dy1, const void* dy2, const void* dy3, int32_t k0, int32_t k1, int32_t k2, int32_t k3,
                            void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t accumulate, void* stream);
/* MaxPooling2D(pool_size = strides = k), any k dividing H and W (PSPNet `psp_pooling_type: max`): idx[N,H/k,W/k,C] int32 = position of the
 * first maximum inside its window (NULL = not wanted); the gradient goes to that position. */
int stp_maxpool_k(const void* x, void* y, int32_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t dtype, void* stream);
int stp_maxpool_k_bwd(const int32_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t dtype,
                      int32_t accumulate, void* stream);
/* dy <- dy * [y > 0] in place (gradient of a ReLU fused into a convolution epilogue); count % 4 == 0 */
int stp_relu_bwd(const void* y, void* dy, int64_t count, int32_t dtype, void* stream);

/* Gradient of UpSampling2D(2): dx[n,h,w,c] (+)= sum of the 2x2 block of dy ([N,2H,2W,ldy]). */
int stp_upsample2x_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldy,
                       int32_t dtype, int32_t accumulate, void* stream);
/* The same when dx is the gradient of a BatchNormalization(+activation) output that this launch completes: the stored value
 * is masked with the activation re-derived from the BN input bn_x and `partial` ([2][C][tiles], tiles from the query; 0 =
 * channel count not supported) receives the sums stp_bn_backward_fused consumes - see stp_conv_params.bnb_x. */
/* Second half of the data gradient of a 1x1 / stride-2 convolution (reference: the projection shortcut `sc` of
 * classification_models' bottleneck ResNets, reached through segmentation.py:109-118): t = W^T dY is computed at LOW resolution by a plain
 * 1x1 / stride-1 stp_conv2d; stp_scatter2x_bwd puts t[n, a, b] at (2a, 2b) of dx [N, H, W, C] (zeros elsewhere; accumulate != 0: dx +=).
 * The _bn form completes the gradient of a BatchNormalization(+activation) output as stp_maxpool3x3s2_bwd_bn does: masked in place,
 * partial[2][C][stp_scatter2x_bwd_bn_tiles] for stp_bn_backward_fused. */
/* Conv2D(3x3, padding 1) with few output channels over many input channels (segmentation_models' class heads `final_conv` of FPN / PSPNet,
 * reached through segmentation.py:109-118) as a 1x1 stp_conv2d into 9 x Cout tap channels (the 3x3 kernel [Cout][3][3][Cin] read as the
 * matrix [9 Cout][Cin]: tap channel (o, t) = o * 9 + t) followed by stp_tapsum_fwd:
 *   y[n, h, w, o] = bias[o] + sum_t z[n, h + t / 3 - 1, w + t % 3 - 1, o * 9 + t]   (taps outside the image contribute zero)
 * stp_tapsum_bwd is its adjoint: dz[n, h, w, o * 9 + t] = dy[n, h - (t / 3 - 1), w - (t % 3 - 1), o]; the padded channels of dz are zeroed. */
int stp_tapsum_fwd(const void* z, void* y, const float* bias, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t Zc, int32_t Cy, int32_t dtype,
                   void* stream);
int stp_tapsum_bwd(const void* dy, void* dz, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t Cdy, int32_t Cdz, int32_t dtype, void* stream);
int stp_scatter2x_bwd(const void* t, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t accumulate, void* stream);
int stp_scatter2x_bwd_bn_tiles(int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype);
int stp_scatter2x_bwd_bn(const void* t, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t accumulate,
                         const void* bn_x, const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t relu,
                         float* partial, void* stream);
int stp_upsample2x_bwd_bn_tiles(int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldy, int32_t dtype);
int stp_upsample2x_bwd_bn(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldy, int32_t dtype,
                          int32_t accumulate, const void* bn_x, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, int32_t relu, float* partial, void* stream);
/* x[n,2h+i,2w+j,c] += m[n,h,w,c] in place (FPN: Add()([lateral, UpSampling2D(2)(m)])); H, W = size of x, even. */
int stp_upsample2x_add(void* x, const void* m, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* tf.image.resize_bilinear(align_corners=False) of TF 1.x by an integer factor (src = dst / factor, no half-pixel offset) -
 * Keras 2.2.4's K.resize_images(interpolation='bilinear').  x [N,H,W,C] -> channels [coff, coff+C) of y [N,H*f,W*f,ldo]
 * (Concatenate of resized maps without a copy; factor 1 = strided copy).  The gradient is a fixed-order gather: one
 * workgroup per input pixel over the (2f)^2 outputs that may read it, split further through `workspace` (fp32 partials,
 * size from the query, 0 = not needed) when a few pixels collect a whole map (PSPNet level 1: 1x1 -> 96x96). */
int stp_resize_bilinear(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo,
                        int32_t coff, int32_t dtype, void* stream);
size_t stp_resize_bilinear_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor);
int stp_resize_bilinear_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo,
                            int32_t coff, int32_t dtype, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Which form of the gradient stp_resize_bilinear_bwd runs for these arguments (csrc/resize_bwd.hip; a plan-time query for callers and
 * tests: launches nothing, needs no device).  The forms are tried in this order: SLICE_COPY (factor 1: the channel slice copied or
 * added back), TINY (maps of <= 16 x 8 pixels, factor >= 8: a separable two-pass reduction; only with a workspace of the queried size
 * and a 16-byte aligned dy), ROWS (output rows of <= 40 KB streamed through LDS: class logits), TILE (16-bit slices of >= 32
 * channels: row pairs), then the workgroup-per-pixel kernel in one pass (BLOCK) or with its tap rows split over the workspace and summed
 * by a second launch (BLOCK_SPLIT; without a large-enough workspace: BLOCK), and GATHER (channel counts or slices that no vector
 * width divides).  STP_E_BADARG under the same checks as the launch; the pointers are only tested for null and alignment. */
#define STP_RESIZE_BWD_GATHER 0
#define STP_RESIZE_BWD_SLICE_COPY 1
#define STP_RESIZE_BWD_TINY 2
#define STP_RESIZE_BWD_ROWS 3
#define STP_RESIZE_BWD_TILE 4
#define STP_RESIZE_BWD_BLOCK 5
#define STP_RESIZE_BWD_BLOCK_SPLIT 6
int stp_resize_bilinear_bwd_form(const void* dy, const void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo,
                                 int32_t coff, int32_t dtype, const void* workspace, size_t workspace_bytes);
/* ResizeImage(factor, interpolation='nearest') (= UpSampling2D(factor)) with the same slice addressing, and its gradient (the sum of
 * the factor x factor outputs of every input pixel). */
int stp_resize_nearest(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo, int32_t coff,
                       int32_t dtype, void* stream);
int stp_resize_nearest_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo, int32_t coff,
                           int32_t dtype, int32_t accumulate, void* stream);

/* Bias gradient: out[c] (+)= sum over rows of x[rows][C]; and the in-place tensor add used where two
 * gradient paths meet outside a GEMM epilogue.  workspace as for stp_bn_stats. */
int stp_channel_sum(const void* x, int32_t dtype, int64_t rows, int32_t C, float* out, int32_t accumulate,
                    void* workspace, size_t workspace_bytes, void* stream);
int stp_add_inplace(void* dst, const void* src, int64_t count, int32_t dtype, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Segmentation head + loss.  logits -> sigmoid -> w_bce*binary_crossentropy + w_dice*dice_loss
 * (Keras TF-backend BCE with the 1e-7 probability clip; musket dice_coef_loss, smooth 1), the
 * metrics (dice at 0.5, binary_accuracy) and dL/dlogits (channel 0 of a [count][dl_channels]
 * tensor, other channels zero, so it can feed the 8-channel-granular gather of the GEMMs).
 * scalars (fp32[10]): loss, bce, dice_loss, dice_metric, binary_accuracy, sum_p, sum_y, sum_py, iou, iot
 *   (iou = (sum_py+1)/(sum_y+sum_p-sum_py+1); iot = the same with p thresholded at 0.5).
 * Two-stage, fixed-order reduction (deterministic).
 */
size_t stp_loss_workspace_bytes(void);
int stp_sigmoid_bce_dice(const void* logits, const uint8_t* target, int64_t count, int32_t dtype,
                         float w_bce, float w_dice, float* scalars, void* dlogits, int32_t dl_channels,
                         float grad_scale, void* workspace, size_t workspace_bytes, void* stream);
/* The rest of the loss registry of segmentation.py:15-22 for the sigmoid head: weights5 (HOST pointer, read at launch)
 * = weights of {binary_crossentropy, dice_loss, iou_loss, jaccard_loss, focal_loss} in the composite `a+w*b` spec
 * (README.md:210-214).  iou_loss = 1 - iou_coef (smooth 1); jaccard_loss = jaccard_distance_loss (smooth 100, per pixel,
 * mean); focal_loss = binary focal loss (gamma 2, alpha 0.25, 1e-7 clip, mean).  scalars (fp32[12]) = the ten of
 * stp_sigmoid_bce_dice + [10] jaccard_loss, [11] focal_loss. */
int stp_sigmoid_loss_ex(const void* logits, const uint8_t* target, int64_t count, int32_t dtype, const float* weights5,
                        float* scalars, void* dlogits, int32_t dl_channels, float grad_scale, void* workspace,
                        size_t workspace_bytes, void* stream);
/* lovasz_loss (segmentation.py:18; README.md:379,411): binary Lovasz hinge per image on the Keras-recovered logits, mean over
 * images.  Runs AFTER stp_sigmoid_bce_dice / stp_sigmoid_loss_ex on the same scalars / dlogits: scalars[12] = lovasz_loss,
 * scalars[0] += weight * lovasz_loss, dlogits channel 0 += weight * gradient (scalars is fp32[16] here).  The workspace holds the
 * sort keys and rocPRIM's temporary storage: stp_lovasz_workspace_bytes(images * per_image, images) (0 = not available). */
size_t stp_lovasz_workspace_bytes(int64_t count, int32_t images);
int stp_lovasz_hinge(const void* logits, const uint8_t* target, int32_t images, int64_t per_image, int32_t dtype, float weight,
                     float* scalars, void* dlogits, int32_t dl_channels, void* workspace, size_t workspace_bytes, void* stream);
/* Bias gradient of the class convolution (= sum of dL/dlogit): stp_sigmoid_bce_dice / stp_sigmoid_loss_ex leave one partial sum
 * per gradient workgroup in their workspace; this adds them up in a fixed order into dbias[0] (instead of a stp_channel_sum pass
 * over the padded gradient tensor).  Same workspace and count as the loss call that wrote dlogits. */
int stp_sigmoid_loss_bias_grad(const void* workspace, int64_t count, float* dbias, int32_t accumulate, void* stream);
int stp_sigmoid(const void* logits, float* probs, int64_t count, int32_t dtype, void* stream);
/* Multi-label sigmoid head (classes: C, activation: sigmoid, H x W x C {0,1} masks): C = 2..8 independent sigmoid channels of
 * logits [pixels][ldc] (the first `classes` channels), target = one uint8 per pixel with bit c = class c.  weights5 (HOST pointer) as
 * stp_sigmoid_loss_ex; every loss is the Keras / musket formula on the [pixels, classes] tensor: binary_crossentropy, binary_accuracy and
 * focal_loss are means over pixels * classes elements, dice / iou ONE soft coefficient over the flattened tensor (smooth 1), jaccard_loss
 * the per-pixel distance over the class axis (smooth 100) averaged over pixels.  scalars (fp32[12]) in the layout of stp_sigmoid_loss_ex;
 * dlogits [pixels][dl_channels] gets the classes gradients x grad_scale and zero padding.  STP_E_BADARG for classes outside 2..8,
 * ldc < classes or dl_channels < classes.  Workspace: stp_loss_workspace_bytes(). */
int stp_sigmoid_multilabel_loss(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc,
                                int32_t dtype, const float* weights5, float* scalars, void* dlogits, int32_t dl_channels,
                                float grad_scale, void* workspace, size_t workspace_bytes, void* stream);
/* Bias gradients of the multi-label class convolution: the gradient pass of stp_sigmoid_multilabel_loss leaves one partial sum per
 * class and workgroup in its workspace; this adds them up in a fixed order into dbias[0 .. classes) (accumulate: +=).  Same workspace,
 * pixels and classes as the loss call that wrote dlogits. */
int stp_sigmoid_multilabel_bias_grad(const void* workspace, int64_t pixels, int32_t classes, float* dbias, int32_t accumulate,
                                     void* stream);
/* Multi-class head (activation: softmax, loss: categorical_crossentropy[+w*dice_loss]; schemas/segmentation.raml:12-21,
 * 62-63): channel softmax over the first `classes` (2..32) channels of logits [pixels][ldc], target = uint8 class index
 * per pixel.  scalars as stp_sigmoid_bce_dice with [1] = categorical_crossentropy and the sums taken over every
 * (pixel, class) element of the one-hot target; dlogits [pixels][dl_channels] gets classes gradients + zero padding. */
int stp_softmax_cce_dice(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc,
                         int32_t dtype, float w_cce, float w_dice, float* scalars, void* dlogits, int32_t dl_channels,
                         float grad_scale, void* workspace, size_t workspace_bytes, void* stream);
/* The multi-class head with the rest of the loss registry (segmentation.py:15-22) but lovasz_loss: weights5 (HOST pointer) =
 * {categorical_crossentropy, dice_loss, iou_loss, jaccard_loss, focal_loss}, every term the Keras / musket formula on p = softmax of the
 * first `classes` (2..32) channels and the one-hot target (uint8 class index per pixel, clamped to classes - 1): iou_loss ONE soft
 * coefficient over the [pixels, classes] tensor (smooth 1), jaccard_loss the per-pixel distance over the class axis (smooth 100) averaged
 * over pixels, focal_loss (gamma 2, alpha 0.25) a mean over pixels * classes elements.  scalars (fp32[12]) in the layout of
 * stp_sigmoid_loss_ex: [1] = categorical_crossentropy, [8] = the soft iou, [10] = jaccard_loss, [11] = focal_loss (0 when its weight is 0: the
 * term's per-class logarithms are then not evaluated), the rest as
 * stp_softmax_cce_dice.  dlogits [pixels][dl_channels] gets the classes gradients x grad_scale and exactly-zero padding (NULL: scalars
 * only).  Deterministic (fixed-order reduction, no atomics).  STP_E_BADARG for classes outside 2..32, ldc < classes, dl_channels <
 * classes or the other build's 16-bit dtype; STP_E_WORKSPACE below stp_loss_workspace_bytes().  Not here: a fused low-resolution
 * (_up) form, a bias-gradient shortcut from workgroup sums.  (The Lovasz term of several classes: stp_lovasz_softmax, below.) */
int stp_softmax_loss_ex(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc,
                        int32_t dtype, const float* weights5, float* scalars, void* dlogits, int32_t dl_channels,
                        float grad_scale, void* workspace, size_t workspace_bytes, void* stream);
/* stp_softmax_loss_ex with an ignore label and class weights (experiment keys ignore_label / class_weights).  The arguments of
 * stp_softmax_loss_ex, then ignore_label (-1: none, else 0..255: a pixel whose STORED target equals it takes no part in the loss, the
 * gradient or the metrics) and class_weights (DEVICE pointer to `classes` floats, NULL: all 1; positive and finite - the host checks
 * them, the kernel cannot).  The arithmetic, fixed HERE (the reference pins none):
 *   t_i the stored target, v_i = [t_i != ignore_label]; the class of a counted pixel is min(t_i, classes - 1); w_c the class weights;
 *   omega_i = v_i w_class(i); n = sum_i v_i, counted on the device (it differs from batch to batch); p = softmax(z), y the one-hot target.
 *   1. per-pixel means (Keras's class_weight / zero sample weight rule: the weight multiplies the per-sample loss, the mean runs over
 *      the samples that count):  categorical_crossentropy = sum_i omega_i ce_i / n,  jaccard_loss = sum_i omega_i jac_i / n,
 *      focal_loss = sum_i omega_i sum_c focal_ic / (n classes) - ce_i, jac_i, focal_ic the per-pixel expressions of stp_softmax_loss_ex,
 *      clips included.
 *   2. region overlaps: dice_loss, iou_loss and the logged dice, iou, iot, binary_accuracy from sums over the counted pixels only
 *      (sum_p, sum_y = n, sum_py and the thresholded sums each times v_i; accuracy over n classes elements); class weights do not enter.
 *   3. loss = the weighted sum of the five terms (weights5).
 *   4. n == 0: the three means are 0 (the divisor is max(n, 1)), the overlap terms take their smooth-term values (dice_loss 0, iou 1),
 *      every gradient element is 0; nothing is NaN.
 *   5. dlogits = the exact derivative of the above through the softmax x grad_scale; the row of an ignored pixel is exactly 0.0 in
 *      every channel and IS stored, padding channels of every row are exactly 0; the 1e-7 clips pass no gradient.
 *   6. ignore_label -1 and weights of 1 (or NULL): the scalars and gradients of stp_softmax_loss_ex on the same inputs.
 * scalars (fp32[14]): [0..11] as stp_softmax_loss_ex ([11] = 0 when focal_loss has no weight), [12] = n, [13] = sum_i omega_i (n is exact
 * in its float up to 2^24 counted pixels; the gradient pass reads it from there).  Deterministic: fixed-order reduction, no atomics.
 * STP_E_BADARG as stp_softmax_loss_ex, and for ignore_label outside -1..255; STP_E_WORKSPACE below stp_loss_workspace_bytes().
 * Not here: a fused low-resolution (_up) form, class weights on dice_loss / iou_loss. */
int stp_softmax_loss_masked(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc,
                            int32_t dtype, const float* weights5, float* scalars, void* dlogits, int32_t dl_channels,
                            float grad_scale, void* workspace, size_t workspace_bytes, int32_t ignore_label,
                            const float* class_weights, void* stream);
/* lovasz_softmax: the Lovasz-Softmax of Berman et al. (the mean-IoU surrogate) on the multi-class head, batch form (per_image=False,
 * classes='present').  Runs AFTER stp_softmax_loss_ex / stp_softmax_loss_masked on the same logits, scalars (fp32[16]) and dlogits and ADDS
 * its term, as stp_lovasz_hinge does for one class.  The arithmetic, fixed HERE (the reference pins none):
 *   p = softmax(z) in fp32 over the first `classes` channels; t_i the stored target, v_i = [t_i != ignore_label] (-1: every pixel counts);
 *   the class of a counted pixel is min(t_i, classes - 1), y_ic its one-hot target.  For each class c over the counted pixels of the batch:
 *     e_ic = y_ic ? 1 - p_ic : p_ic;  G_c = sum_i v_i y_ic, the class is present iff G_c > 0;
 *     the errors ordered by descending e, ties by ascending pixel index (a stable sort of class-major keys);
 *     at 0-based rank r, c1_r / c0_r = positives / negatives among ranks 0..r;  g_r = 1 / (G + c0_r) for a positive,
 *     (G - c1_r) / ((G + c0_r - 1) (G + c0_r)) for a negative (the closed form of the Jaccard increments: sum_r g_r = 1);
 *     loss_c = sum_r e_(r) g_r.
 *   lovasz_softmax = (1 / P) sum over the present classes of loss_c, P = their number; P == 0 (nothing counted): the term is 0, every
 *   gradient element is 0, nothing is NaN.  Class weights do not enter (as they do not enter dice_loss / iou_loss).
 *   Gradient with g held constant (the surrogate's sub-gradient): d_ic = (y_ic ? -1 : +1) g_rank(i,c) / P for counted pixels of present
 *   classes, else 0;  dz_ik = p_ik (d_ik - sum_c p_ic d_ic).
 *   scalars[14] = lovasz_softmax;  scalars[0] += weight * lovasz_softmax (two roundings);  dlogits[i][k] += weight * grad_scale * dz_ik, the
 *   add made in the storage type; rows of ignored pixels and padding channels are not touched (they stay exactly 0).  dlogits NULL: scalars only.
 * Launches: key pass, one chip-wide stable radix sort of (class << 30 | reversed error bits, pixel << 1 | y) pairs (rocPRIM through hipCUB),
 * two scan launches over a grid of (chunk of STP_LOVASZ_SOFTMAX_CHUNK ranks, class) workgroups, a one-workgroup finalize in double, the
 * gradient pass.  Deterministic (fixed-order sums; the only atomics are integer counts), no allocation, no synchronisation: it captures into
 * a hipGraph.  workspace: 16-byte aligned, >= stp_lovasz_softmax_workspace_bytes(pixels, classes) (0 = not available: bad sizes, or no device
 * to size the sort on) - 24 bytes per (pixel, class) for the double-buffered pairs (the coefficient buffer of the gradient lives in the pair
 * buffer the sort leaves free) plus the sort's temporary storage and two words per (chunk, class).
 * STP_E_BADARG before any launch: classes outside 2..32, ldc < classes, dl_channels < classes (with dlogits), pixels <= 0 or pixels * classes >=
 * 2^31, ignore_label outside -1..255, a NULL pointer, the other build's 16-bit dtype; STP_E_WORKSPACE below the queried size.
 * Not here: a per-image variant, class weights on this term, a low-resolution (_up) form. */
#define STP_LOVASZ_SOFTMAX_CHUNK 4096 /* ranks of a class segment one scan workgroup walks */
size_t stp_lovasz_softmax_workspace_bytes(int64_t pixels, int32_t classes);
int stp_lovasz_softmax(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype, float weight,
                       float* scalars, void* dlogits, int32_t dl_channels, float grad_scale, int32_t ignore_label, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The same loss on class logits the network produces at 1 / factor of the mask's resolution and resizes bilinearly (segmentation_models
 * 0.2.1: PSPNet `final_interpolation: bilinear` x downsample_factor, schemas/segmentation.raml:225-249; FPN's last UpSampling2D(4,
 * 'bilinear')) - replaces, in the training step, stp_resize_bilinear of the logits + stp_softmax_cce_dice + stp_scale_by_device +
 * stp_resize_bilinear_bwd of their gradient WITHOUT the resized tensors: low [N][H][W][ldc], target [N][H factor][W factor] (4-byte
 * aligned), dlow [N][H][W][dl_channels] = d loss / d low (classes gradients + zero padding; NULL: scalars only), rounded to the storage
 * type where the unfused chain rounds (the resized logit, the per-pixel gradient).  dev_scale (may be NULL): device multiplier applied to
 * dlow (the dynamic loss scale, stp_scale_by_device), recorded into dev_record[0].  factor 2 / 4 / 8 / 16; workspace >=
 * stp_loss_workspace_bytes(); corners >= stp_softmax_cce_dice_up_corner_bytes() (16-byte aligned; only with dlow).  _ok: 1 if the
 * fused form serves (factor, classes) (STP_UP_LOSS=0: never). */
int stp_softmax_cce_dice_up_ok(int32_t factor, int32_t classes, int32_t dtype);
size_t stp_softmax_cce_dice_up_corner_bytes(int32_t N, int32_t H, int32_t W, int32_t classes);
int stp_softmax_cce_dice_up(const void* low, const uint8_t* target, int32_t N, int32_t H, int32_t W, int32_t factor, int32_t classes,
                            int32_t ldc, int32_t dtype, float w_cce, float w_dice, float* scalars, void* dlow, int32_t dl_channels,
                            float grad_scale, const float* dev_scale, float* dev_record, void* workspace, size_t workspace_bytes,
                            void* corners, size_t corner_bytes, void* stream);
/* probs [pixels][classes] fp32 = softmax of the first `classes` channels */
int stp_softmax(const void* logits, float* probs, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype, void* stream);

/* Confusion matrix of the multi-class head (metrics: categorical_accuracy, mean_iou, iou_class_k - K.argmax against the class-index
 * target).  rows [pixels][ldc] in the storage type, logits or probabilities (only the first `classes` = 2..32 channels are read); target =
 * class index per pixel, clamped to classes - 1 as the loss kernels clamp it.  Predicted class = the FIRST index of the row maximum of
 * the stored values (numpy.argmax); it lies in [0, classes) whatever the values are, NaN included.  counts: dense [classes][classes]
 * int32, counts[t * classes + p]; every call OVERWRITES it (no accumulation), nothing behind entry classes * classes is touched, the
 * entries sum to `pixels`.  Integer sums: two calls and a graph replay give the same counts bit for bit.  pixels in 1 .. 2^31 - 1
 * (argument 2, as in every loss launch: Plan.rerun_loss shortens it); workspace >= stp_class_confusion_workspace_bytes(classes)
 * (0 for classes outside 2..32).  rows / low are 16-byte aligned, as every buffer of this interface: rows whose stride is a multiple of
 * 16 bytes are read as 16-byte vectors without a check.
 * _up: the same matrix for logits low [N][H][W][ldc] held at 1 / factor (2 / 4 / 8 / 16) of the mask's resolution, target
 * [N][H factor][W factor]: each class is interpolated in fp32 with stp_resize_bilinear's expression and rounded to the storage type as
 * its store rounds, so the counts EQUAL those of stp_resize_bilinear followed by stp_class_confusion (no tolerance).  _up_ok: 1 if the
 * form serves (factor, classes, dtype).
 * _ignore: stp_class_confusion with an ignore label (-1: none, else 0..255): pixels whose stored target equals it are not counted, the
 * entries sum to the number of counted pixels; with -1 the counts are stp_class_confusion's.
 * STP_E_BADARG: classes outside 2..32, ldc < classes, null pointers, pixels <= 0 or >= 2^31, an unsupported factor, ignore_label outside -1..255, the other build's
 * 16-bit dtype; STP_E_WORKSPACE: less workspace than the query returns. */
size_t stp_class_confusion_workspace_bytes(int32_t classes);
int stp_class_confusion(const void* rows, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                        int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int stp_class_confusion_ignore(const void* rows, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                               int32_t* counts, void* workspace, size_t workspace_bytes, int32_t ignore_label, void* stream);
int stp_class_confusion_up_ok(int32_t factor, int32_t classes, int32_t dtype);
int stp_class_confusion_up(const void* low, const uint8_t* target, int32_t N, int32_t H, int32_t W, int32_t factor,
                           int32_t classes, int32_t ldc, int32_t dtype, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Optimizers over a flat fp32 arena (Keras 2.2.4 update rules, schemas/segmentation.raml:77-89).
 * `state` is a device int32[2]: [0] = iteration counter (incremented by the launch, so a captured
 * graph advances), [1] = scratch for the bias-corrected step size.  count must be a multiple of 4.
 * lr lives in device memory (lr[0]) so callbacks can change it without re-capturing.
 * mask (uint8, optional) freezes elements where mask[i] == 0 (freeze_encoder).
 * gscale (device float, optional) multiplies the gradient (clipnorm / 1/world_size).
 */
int stp_adam(float* param, const float* grad, float* m, float* v, int64_t count, const float* lr,
             float beta1, float beta2, float eps, int32_t* state, const uint8_t* mask, const float* gscale,
             float clipvalue, void* stream);
int stp_sgd(float* param, const float* grad, float* vel, int64_t count, const float* lr, float momentum,
            int32_t nesterov, const uint8_t* mask, const float* gscale, float clipvalue, void* stream);
/* RMSprop (Keras 2.2.4): a <- rho a + (1-rho) g^2 ; p <- p - lr g / (sqrt(a) + eps).  Same mask / gscale / clipvalue
 * conventions as stp_adam. */
int stp_rmsprop(float* param, const float* grad, float* acc, int64_t count, const float* lr, float rho, float eps,
                const uint8_t* mask, const float* gscale, float clipvalue, void* stream);
/* Nadam (Keras 2.2.4, schedule_decay form; lr default 0.002).  state: int32[2] as stp_adam (state[0] = iteration);
 * fstate: float[8] device scratch whose element 0 is m_schedule and MUST be initialised to 1.0. */
int stp_nadam(float* param, const float* grad, float* m, float* v, int64_t count, const float* lr, float beta1, float beta2,
              float eps, float schedule_decay, int32_t* state, float* fstate, const uint8_t* mask, const float* gscale,
              float clipvalue, void* stream);
/* gscale[0] = min(1, clipnorm / ||base*grad||_2) * base  (base = 1/world_size for summed data-parallel
 * gradients, times 1/loss_scale in fp16 mode; clipnorm <= 0: no clipping; deterministic two-stage reduction).  workspace >= 4 KiB.
 * OVERFLOW GUARD: gscale is float[2]; when the squared norm is not finite (an inf / NaN anywhere in the arena - fp16 overflow
 * under loss scaling) gscale[0] = -1 and gscale[1] is incremented, and every optimizer entry point (stp_adam, stp_sgd,
 * stp_rmsprop, stp_nadam) given that gscale returns without touching parameters, moments or its step counter: the step is skipped. */
int stp_grad_global_scale(const float* grad, int64_t count, float clipnorm, float base, float* gscale,
                          void* workspace, size_t workspace_bytes, void* stream);
/* DYNAMIC LOSS SCALING (fp16 storage; replaces a Keras LossScaleOptimizer / torch GradScaler around the reference's fit()).
 * dls = float[8] on the device: [0] multiplier m of the next backward pass (on top of the static scale of the loss kernels),
 * [1] clean steps, [2] growth interval, [3] smallest m, [4] m of the gradients now in the arena, [5] largest m.
 * stp_scale_by_device: x *= scalar[0] (the loss gradient right after the loss kernel seeded it; record = dls + 4).  stp_grad_global_scale_dls: as
 * stp_grad_global_scale with base / m; a skipped step halves m, `interval` clean steps double it - all on the device (graph-safe). */
int stp_scale_by_device(void* x, int64_t count, int32_t dtype, const float* scalar, float* record /* may be NULL: receives scalar[0] */, void* stream);
int stp_grad_global_scale_dls(const float* grad, int64_t count, float clipnorm, float base, float* gscale, float* dls,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * DeepLabV3+ (the in-tree model, segmentation_pipeline/impl/deeplab/model.py) - the ops nothing else needs.
 *
 * Depthwise convolution (DepthwiseConv2D, model.py:136, 255-259): x [N,H,W,C] dtype, w fp32 [k][k][C] (Keras'
 * (kh,kw,C,1) kernel as stored), explicit top/left padding (TF 'same' is bottom/right heavy), dilation; C % 4 == 0.
 * The weight gradient needs stp_dwconv_wgrad_workspace_bytes(C, k) of workspace (two-stage fixed-order reduction). */
int stp_dwconv(const void* x, const float* w, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride,
               int32_t pad_t, int32_t pad_l, int32_t dilation, int32_t Ho, int32_t Wo, int32_t dtype, void* stream);
int stp_dwconv_dgrad(const void* dy, const float* w, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                     int32_t stride, int32_t pad_t, int32_t pad_l, int32_t dilation, int32_t Ho, int32_t Wo, int32_t dtype,
                     int32_t accumulate, void* stream);
size_t stp_dwconv_wgrad_workspace_bytes(int32_t C, int32_t k);
int stp_dwconv_wgrad(const void* x, const void* dy, float* dw, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                     int32_t stride, int32_t pad_t, int32_t pad_l, int32_t dilation, int32_t Ho, int32_t Wo, int32_t dtype,
                     int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* tf.image.resize_bilinear(align_corners=True) to any output size, larger or smaller than the input (BilinearUpsampling,
 * model.py:94-100) and its gradient (fixed-order gather).  Dense [N,H,W,C] tensors, any C.  Per axis, in fp32:
 * s = float(H-1) / float(Ho-1) (0 when Ho == 1), src = float(yo) * s, y0 = floor(src), y1 = min(y0+1, H-1), f = src - y0.
 * The forward evaluates v0 + (v1 - v0) * f along x for both rows, then along y, and rounds once to the storage dtype; the
 * gradient is the adjoint with weights (1 - f) and f (dx = Ry^T dy Rx, + dx when accumulate), rounded once. */
int stp_resize_bilinear_ac(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo,
                           int32_t dtype, void* stream);
int stp_resize_bilinear_ac_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo,
                               int32_t dtype, int32_t accumulate, void* stream);
/* Inverted dropout (model.py:461): y = mask * x / (1 - rate), mask = counter-based hash of (state[0], salt, index) - the same
 * call with dy gives the gradient; stp_counter_tick advances state[0] (int32 on the device) once per step, so a hipGraph
 * replay draws a fresh mask.  x == y allowed.  A kept element is float(x) * (1.f / (1.f - rate)), rounded once (to nearest
 * even) to the storage dtype; rate = 0 returns x. */
int stp_counter_tick(int32_t* state, void* stream);
int stp_dropout(const void* x, void* y, int64_t count, float rate, const int32_t* state, uint32_t salt, int32_t dtype, void* stream);
/* SpatialDropout2D(rate) on [N][HW][C] (segmentation_models' FPN / PSPNet `dropout`, schemas/segmentation.raml:201-203, 241-243):
 * one keep / drop decision per (sample, channel), mask index n * C + c, same hash, scaling and step counter as stp_dropout. */
int stp_dropout_spatial(const void* x, void* y, int32_t N, int64_t HW, int32_t C, float rate, const int32_t* state, uint32_t salt,
                        int32_t dtype, void* stream);
/* Activation('sigmoid') carried by the last convolution (model.py:485) as a tensor op on the first `channels` columns of
 * [rows][ld] tensors, and dz = dp * p * (1 - p) over [rows][ldg] gradients (padding columns written as 0). */
int stp_sigmoid_act(const void* z, void* p, int64_t rows, int32_t channels, int32_t ldz, int32_t ldp, int32_t dtype, void* stream);
int stp_sigmoid_act_bwd(const void* p, const void* dp, void* dz, int64_t rows, int32_t channels, int32_t ldp, int32_t ldg,
                        int32_t dtype, void* stream);
/* Loss on PROBABILITIES (the model upsamples sigmoid outputs, model.py:485-486): same scalars as stp_sigmoid_bce_dice,
 * gradient w.r.t. the probabilities into column 0 of dprobs [count][dl_channels].  workspace >= stp_loss_workspace_bytes(). */
int stp_prob_bce_dice(const void* probs, const uint8_t* target, int64_t count, int32_t dtype, float w_bce, float w_dice,
                      float* scalars, void* dprobs, int32_t dl_channels, void* workspace, size_t workspace_bytes, void* stream);
/* The multi-class form of the same head (classes 2..32, activation softmax inside the class convolution, model.py:485):
 * Activation('softmax') over the first `classes` columns as a tensor op with its gradient dz_c = p_c (dp_c - sum_k p_k dp_k),
 * and Keras categorical_crossentropy (p / sum p, 1e-7 clip) + w_dice * dice_loss on the RESIZED probabilities
 * [pixels][ldc] against class-index targets; scalars as stp_softmax_cce_dice, dprobs [pixels][dl_channels >= classes]. */
int stp_softmax_act(const void* z, void* p, int64_t rows, int32_t classes, int32_t ldz, int32_t ldp, int32_t dtype, void* stream);
int stp_softmax_act_bwd(const void* p, const void* dp, void* dz, int64_t rows, int32_t classes, int32_t ldp, int32_t ldg,
                        int32_t dtype, void* stream);
int stp_prob_cce_dice(const void* probs, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                      float w_cce, float w_dice, float* scalars, void* dprobs, int32_t dl_channels, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * On-device augmentation (replaces the imgaug worker processes, schemas/augmenters.raml:43-133).
 * One fused pass per batch: inverse affine warp (flips, Affine, crop / pad augmenters and the final Resize composed on
 * the host into a 2x3 matrix per sample), bilinear for the image (constant 0 border, result rounded to uint8 like
 * imgaug), nearest for the mask, then the point operations in the fixed order Add, Multiply, MultiplyElementwise,
 * AddElementwise, AdditiveGaussianNoise, Dropout, Grayscale, Invert (integer / single-rounded float arithmetic: the
 * numpy oracle reproduces them bit for bit; per-pixel randomness is a counter-based hash of seed, pixel, channel, op).
 * params per sample: float[STP_AUG_RECORD] (integers stored as exactly representable floats)
 *   0-5 m00 m01 m02 m10 m11 m12 (output->input pixel map)   6-8 Add per channel   9-11 Multiply per channel
 *   12 flags (1 Invert, 2 noise per channel, 4 dropout per channel, 8 AddElementwise per channel,
 *             16 MultiplyElementwise per channel, 32 AddElementwise on, 64 MultiplyElementwise on)
 *   13 Grayscale alpha * 256   14 noise k = rint(sigma * 65536 / 147.8)   15 dropout threshold rint(p * 2^24)
 *   16-17 AddElementwise [lo, hi] (int)   18-19 MultiplyElementwise [lo, hi]   20 seed (integer < 2^24)   21-23 zero
 */
#define STP_AUG_RECORD 24
int stp_augment_u8(const uint8_t* img, const uint8_t* mask, uint8_t* img_out, uint8_t* mask_out,
                   const float* params, int32_t N, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                   int32_t C, void* stream);
/* Neighbourhood filters of the augmenter catalogue on a uint8 batch [N,H,W,C] (src != dst): per image an
 * int32[STP_FILTER_RECORD] record = K (odd <= 13; 0 = copy), mode (0 = linear K x K filter, 1 = median), 0, 0, K*K weights
 * in 1/16384 units.  Reflect-101 border, integer arithmetic (bit-exact against the oracle).  GaussianBlur, AverageBlur,
 * Sharpen, Emboss and EdgeDetect are linear filters whose weights the host derives; MedianBlur is mode 1. */
#define STP_FILTER_RECORD 173
int stp_filter_u8(const uint8_t* src, uint8_t* dst, const int32_t* params, int32_t N, int32_t H, int32_t W, int32_t C,
                  void* stream);
/* The non-affine geometric augmenters (schemas/augmenters.raml:126-133) as a per-pixel displacement field [N][Hout][Wout]
 * (int32 = two int16 (dx, dy) in 1/64 pixel) that stp_augment_field_u8 adds to the output pixel position before its matrix:
 * out(p) = in(M (p + D(p))), image bilinear / mask nearest as in stp_augment_u8 (field NULL = stp_augment_u8).
 * stp_field_piecewise: PiecewiseAffine - grid int32 [N][rows][cols][2] = control-point jitter in 1/64 pixel at
 * linspace(0, H, rows) x linspace(0, W, cols), affine per triangle.  stp_field_elastic: ElasticTransformation - per image
 * int32[STP_ELASTIC_RECORD] = seed, alpha (1/64 pixel), blur radius r <= 64, 0, one-sided Gaussian weights w[0..r] in 1/32768
 * (full kernel sums to 32768); tmp is a scratch buffer of the field's size.  Integer arithmetic, bit-exact against the oracle. */
#define STP_ELASTIC_RECORD 69
int stp_augment_field_u8(const uint8_t* img, const uint8_t* mask, uint8_t* img_out, uint8_t* mask_out, const float* params,
                         const int32_t* field, int32_t N, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, int32_t C,
                         void* stream);
int stp_field_piecewise(int32_t* field, const int32_t* grid, int32_t N, int32_t H, int32_t W, int32_t rows, int32_t cols,
                        void* stream);
int stp_field_elastic(int32_t* field, int32_t* tmp, const int32_t* params, int32_t N, int32_t H, int32_t W, void* stream);
/* BackgroundReplacer (README.md:270-278, FAQ.md:24-38): out = img inside the mask eroded by a (2*erosion+1)^2 minimum, bg
 * (a background image already resized to H x W, same layout as img) elsewhere; out != img; the mask is not changed. */
int stp_background_replace_u8(const uint8_t* img, const uint8_t* mask, const uint8_t* bg, uint8_t* out, int32_t N, int32_t H,
                              int32_t W, int32_t C, int32_t erosion, void* stream);

/* Gradient-bucket helpers for the RCCL all-reduce (fp32 <-> bf16 wire format). */
int stp_cast_f32_to_bf16(const float* src, void* dst, int64_t count, void* stream);
int stp_cast_bf16_to_f32(const void* src, float* dst, int64_t count, float scale, void* stream);

/* segmentation_models' PSPNet head (schemas/segmentation.raml:226-249: Conv2D(512, 1x1) over Concatenate([feature, the four resized
 * pyramid levels])) WITHOUT the concatenation: a 1x1 convolution commutes with the bilinear resize, so the head is Conv2D(1x1) of the
 * feature with its columns of the kernel + stp_upsample_sum of the 1x1 convolutions of the TINY level maps with theirs (the sum enters
 * the feature convolution as its residual operand).  stp_upsample_sum: y[N][Ho][Wo][C] = sum over the non-NULL sources i of the TF-1.x
 * bilinear resize (align_corners False) of x_i [N][h_i][h_i][C] by Ho / h_i (Ho == Wo, Ho % h_i == 0), one rounding; its gradient is
 * stp_resize_bilinear_bwd per source.  stp_copy_cols_f32: dst[r][0..cols) (+)= src[r][0..cols), fp32 row-major with row pitches ld_* -
 * the column range of the shared kernel as a dense matrix for stp_weight_prepare, and the weight gradient back into the range. */
int stp_upsample_sum(const void* x0, const void* x1, const void* x2, const void* x3, int32_t h0, int32_t h1, int32_t h2, int32_t h3,
                     void* y, int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t dtype, void* stream);
int stp_copy_cols_f32(float* dst, int32_t ld_dst, const float* src, int32_t ld_src, int32_t rows, int32_t cols, int32_t accumulate, void* stream);

/* Batched reduce of lone weight gradients (round 6; the weight gradient of Keras' backward feeds only the optimizer, so its split-K
 * reduction can wait): a layer whose stp_conv2d_wgrad_partial launch (variant 0) wrote plain [splits][Cout * KH * KW * C] slabs into a
 * workspace OF ITS OWN adds a descriptor to a host table (stp_wgrad_reduce_desc_fill: returns the layer's element count, 0 = this layer
 * keeps its own stp_conv2d_wgrad_reduce); the table, copied to the device, is reduced by ONE launch (n layers, max_count = the largest
 * element count).  Deterministic (fixed walk, fixed tree). */
size_t stp_wgrad_reduce_desc_bytes(void);
int64_t stp_wgrad_reduce_desc_fill(void* host_table, int32_t index, const stp_wgrad_params* p, const void* workspace);
int stp_wgrad_reduce_batched(const void* table_dev, int32_t n, int64_t max_count, void* stream);

/* Conv2D(1x1, strides 1) of the bottleneck ResNets (classification_models residual_bottleneck_block conv1 / conv3 / the stride-1 shortcut,
 * segmentation_models' FPN laterals; reached through segmentation.py:109-118) and its data gradient, 16-bit storage, 64 ... 512 channels
 * (stp_conv2d_pw_eligible: the served (C0, Cout) pairs, N * Ho * Wo a multiple of the tile): a pixel-STREAMING kernel - persistent
 * workgroups, the whole weight matrix as register-resident MFMA fragments, pixels double-buffered by LDS-DMA, epilogue (bias | statistics
 * (+ residual) | BatchNormalization backward (+ accumulate)) from the accumulators with 16-byte accesses.  stp_conv2d dispatches to it
 * (STP_PW=0 switches the automatic use off; tile = 800 forces it).  The [2][Cout][columns] table of fused sums has ONE column per
 * workgroup: stp_conv2d_pw_cols (= stp_conv2d_stats_floats / (2 Cout)). */
int stp_conv2d_pw_eligible(const stp_conv_params* p);
int stp_conv2d_pw_cols(const stp_conv_params* p);
int stp_conv2d_pw(const stp_conv_params* p, void* stream);

/* Box calibration probes (bench.py `box_calibration`; no counterpart in the reference - the boxes of one MI355X pool differ by +-2.5 % in
 * sustained clocks, more than one round's gain on the step, so the bench line states what the box it ran on sustains):
 * stp_calib_mfma - `blocks` workgroups of 8 waves, each wave `iters` x 16 back-to-back v_mfma_f32_32x32x16 of the build's 16-bit
 * format on register operands (stp_calib_mfma_flops(blocks, iters) = the FLOP of one launch); out: >= blocks * 512 floats of scratch.
 * stp_calib_copy - device copy with 16-byte accesses (bytes a multiple of 16, both pointers 16-byte aligned). */
int64_t stp_calib_mfma_flops(int32_t blocks, int32_t iters);
int stp_calib_mfma(float* out, int32_t blocks, int32_t iters, void* stream);
int stp_calib_copy(void* dst, const void* src, int64_t bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Channel squeeze-and-excitation of the SE-ResNet basic unit (classification_models `seresnet18/34`: the gate sits on the residual
 * branch, before the Add; reduction 16).  With u = conv2's output and sc the shortcut, both [N, HW, C] in the storage dtype:
 *     z = mean over HW of u;  h = relu(z W1 + b1);  s = sigmoid(h W2 + b2);  x = u * s + sc        (ONE rounding, of x)
 * W1 [C][R], b1 [R], W2 [R][C], b2 [C] are fp32 masters in the Keras Conv2D(1x1) layouts; z, s [N][C] and h [N][R] stay fp32.
 * Served shapes: C % 8 == 0, 16 <= C <= 512, 1 <= R <= 32; anything else is STP_E_BADARG.  The tensor passes work on items =
 * (image, one of stp_se_chunks(N, HW, C) runs of consecutive pixels); every reduction is two-stage in a fixed order (no atomics):
 *   stp_se_squeeze    : per-item channel sums of u into the workspace ([N][chunks][C] fp32, stp_se_workspace_bytes; host-only query).
 *   stp_se_excite     : one workgroup per image adds the chunks in a fixed order, writes z, h, s.
 *   stp_se_scale_add  : x = u * s + sc with 16-byte accesses; stats != NULL: also the per-item sum / sum of squares of the STORED x as a
 *                       [2][C][N * chunks] table for stp_bn_finalize (the next BatchNormalization's batch statistics).  NULL: inference.
 * Gradient, given dx (the shortcut's gradient IS dx):
 *   stp_se_bwd_reduce : per-item channel sums of dx * u (same workspace layout).
 *   stp_se_excite_bwd : per image ds = the chunks in the same fixed order, da2 = ds s (1 - s) [N][C], da1 = (da2 W2^T) [h > 0] [N][R],
 *                       dz = da1 W1^T [N][C]; then dW1 = z^T da1, db1, dW2 = h^T da2, db2 summed over the images IN IMAGE ORDER and
 *                       WRITTEN (not accumulated).  Two launches.
 *   stp_se_bwd_apply  : du = dx * s + dz / HW (ONE rounding). */
int32_t stp_se_chunks(int32_t N, int64_t HW, int32_t C);
size_t stp_se_workspace_bytes(int32_t N, int64_t HW, int32_t C);
int stp_se_squeeze(const void* u, int32_t dtype, int32_t N, int64_t HW, int32_t C, float* workspace, size_t workspace_bytes, void* stream);
int stp_se_excite(const float* workspace, int32_t N, int64_t HW, int32_t C, int32_t R, const float* W1, const float* b1, const float* W2,
                  const float* b2, float* z, float* h, float* s, void* stream);
int stp_se_scale_add(const void* u, const void* shortcut, void* x, int32_t dtype, int32_t N, int64_t HW, int32_t C, const float* s,
                     float* stats, void* stream);
int stp_se_bwd_reduce(const void* dx, const void* u, int32_t dtype, int32_t N, int64_t HW, int32_t C, float* workspace,
                      size_t workspace_bytes, void* stream);
int stp_se_excite_bwd(const float* workspace, int32_t N, int64_t HW, int32_t C, int32_t R, const float* W1, const float* W2, const float* z,
                      const float* h, const float* s, float* da2, float* da1, float* dz, float* dW1, float* db1, float* dW2, float* db2,
                      void* stream);
int stp_se_bwd_apply(const void* dx, void* du, int32_t dtype, int32_t N, int64_t HW, int32_t C, const float* s, const float* dz,
                     void* stream);

/* ----------------------------------------------------------------------------------------------
 * Prediction on the device (csrc/predict.hip): flip test-time augmentation, fold ensembling, the way back to the image's own size and
 * the label map, on the fp32 probabilities an inference plan leaves on the device.  uint8 and fp32 only (both builds export the same
 * code).  Each value comes from the operation numpy applies on the host - one fp32 add, one correctly rounded fp32 division, one fp32
 * multiplication, a truncation - so the results equal the host chain of segmentation_pipeline/segmentation.py (predict_on_batch,
 * _scale_back, `(x * 255).astype(uint8)`, argmax) bit for bit.  No atomics; element indices are int64.  16-byte accesses where the
 * destination rows start on 16-byte boundaries (aligned base, row pitch a multiple of 16 bytes; stp_predict_finish ends such a row with
 * a scalar tail), one element per thread otherwise.  STP_E_BADARG before any launch: a NULL pointer, a size (or k) <= 0, flip outside
 * 0..2, mode outside 0..2, source == destination, out_ld < w, mode 2 with C > 32.
 *
 * flip: 0 = none, 1 = columns reversed (x[:, :, ::-1]), 2 = rows reversed (x[:, ::-1]); whole pixels move, channels keep their order.
 *   stp_flip_u8            : dst[N][H][W][C] = flip(src) - a flipped batch written straight into an inference plan's image buffer.
 *   stp_predict_accumulate : acc[N][H][W][C] += flip(probs) (the un-flip of a map predicted from a flipped input); the caller zeroes acc.
 *   stp_predict_finish     : ONE image.  acc = that image's [H][W][C] sums, k = how many maps were added.  For y < h, x < w:
 *                            value = acc[y * H / h][x * W / w][c] / (float)k (integer division of the coordinates: the nearest gather of
 *                            _scale_back); rows of `out` lie out_ld PIXELS apart (>= w: a `crops` cell is written into its rectangle of
 *                            the full map).  mode 0: out fp32 [h][w][C] = value;  1: out uint8 [h][w][C] = (uint8)(value * 255.f),
 *                            truncating;  2: out uint8 [h][w] = the first index of the largest of the C values (numpy.argmax; 2 <= C <= 32;
 *                            a NaN never wins) or, C == 1, value > 0.5f. */
int stp_flip_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flip, void* stream);
int stp_predict_accumulate(const float* probs, float* acc, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flip, void* stream);
int stp_predict_finish(const float* acc, int32_t H, int32_t W, int32_t C, int32_t k, int32_t mode, void* out, int32_t h, int32_t w,
                       int32_t out_ld, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Dihedral (D4) test-time augmentation on the device (csrc/dihedral.hip; `ttflips="d4"`): all eight symmetries of the square where
 * stp_flip_u8 / stp_predict_accumulate have three.  uint8 and fp32 only (both builds export the same code); values are moved as they
 * are or added with one fp32 add, so the results equal the numpy statement (tests/_dihedral_reference.py) bit for bit.  No atomics;
 * element indices are int64; nothing outside the N * H * W * C elements of the destination is written.
 *
 * op 0..7, on x [N][H][W][C] (whole pixels move, channels keep their order):
 *   g_op(x)   = x.transpose(0, 2, 1, 3) if op & 4, then columns reversed if op & 1, then rows reversed if op & 2
 *               -> [N][H'][W'][C], (H', W') = (W, H) if op & 4 else (H, W)
 *   inv_op(y) = rows reversed if op & 2, then columns reversed if op & 1, then transposed if op & 4: inv_op(g_op(x)) == x.
 * 0, 1, 2 are stp_flip_u8's flips; 3 is the half turn, 4 the transpose, 5 and 6 the quarter turns, 7 the anti-transpose.  H != W is
 * legal here (the layer above offers the transposing ops for square network shapes only).
 *   stp_dihedral_u8                 : dst[N][H'][W'][C] = g_op(src[N][H][W][C]).
 *   stp_predict_accumulate_dihedral : acc[N][H][W][C] += inv_op(probs), probs being [N][H'][W'][C]: one __fadd_rn per element; the
 *                                     caller zeroes acc.
 * The transposing ops move tiles of 8 to 64 pixels a side through LDS (pixels below 256 bytes; rows of the source tile are read and rows
 * of the destination tile are written as contiguous runs) or gather whole pixels (256 bytes and more).  16-byte accesses where both
 * bases are 16-byte aligned and the row pitches are multiples of 16 bytes, one element per thread otherwise.  STP_E_BADARG before any
 * launch: a NULL pointer, a size <= 0, op outside 0..7, source == destination, W * C or H * C above 2^31 - 1. */
int stp_dihedral_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t C, int32_t op, void* stream);
int stp_predict_accumulate_dihedral(const float* probs, float* acc, int32_t N, int32_t H, int32_t W, int32_t C, int32_t op, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Sliding-window prediction on the device (csrc/window.hip): an image larger than the network shape is predicted at its own pixel scale
 * in overlapping H x W windows, cross-faded where they overlap (`windows: <overlap>`, PipelineConfig._predict_windows_device).  Three
 * kernels around the unchanged inference plan and stp_predict_accumulate.  uint8 and fp32 only (both builds export the same code).  A
 * window at origin (y0, x0) weights its pixel (ly, lx) with the INTEGER ry[ly] * rx[lx], r[i] = min(i + 1, L - i, overlap + 1); every
 * fp32 value comes from the operation numpy applies in the host statement (tests/_window_reference.py) - one multiplication and one
 * addition per window in window order, one correctly rounded division, one multiplication by 255, a truncation - so the results equal
 * it bit for bit.  No atomics; element indices are int64.  16-byte accesses where the destination rows start on 16-byte boundaries
 * (aligned base, row pitch a multiple of 16 bytes; stp_window_finish ends such a row with a scalar tail), one element per thread
 * otherwise; sources are read element by element.  STP_E_BADARG before any launch: a NULL pointer, a size (or k) <= 0, n outside
 * 1..64, an origin outside the image (y0 < 0, y0 >= h, x0 < 0, x0 >= w), overlap < 0 or 2 * overlap > min(H, W) (or overlap > 4095:
 * the weight must be an exact fp32 integer), source == destination, out_ld < w, mode outside 0..2, mode 2 with C > 32.
 *
 * `origins` is a HOST pointer to n (y0, x0) int32 pairs, copied into the kernel's arguments; more than 64 windows take several calls, in
 * order.
 *   stp_window_gather_u8  : dst[i][y][x][c] = img[min(y0_i + y, h - 1)][min(x0_i + x, w - 1)][c] for y < H, x < W: the windows of one batch
 *                           cut out of the image [h][w][C] into a batch [n][H][W][C] at the network shape; an image smaller than the
 *                           window is edge-replicated (numpy.pad(mode="edge")).
 *   stp_window_accumulate : acc = the batch's [n][H][W][C] probability sums.  GATHER form: a thread owns elements of the canvas [h][w][C]
 *                           and goes through the n windows in index order; for each window that holds its pixel,
 *                           canvas = canvas + (float)(ry * rx) * acc[i][y - y0][x - x0][c].  No two threads write one element; an
 *                           element is read and written once per call, however many windows cover it.  The launch covers only the rows
 *                           the windows span; the other rows are not touched.  The caller zeroes the canvas once per image
 *                           (stp_zero_bytes).
 *   stp_window_finish     : value = canvas[y][x][c] / ((float)k * sy[y] * sx[x]); k = how many maps each window's sum holds, sy / sx = DEVICE
 *                           fp32 tables [h] / [w] of the per-axis sums of the ramps over the windows that hold the row / column (the
 *                           weight sum of a product grid of windows is separable).  The caller keeps k * max(sy) * max(sx) <= 2^24, so
 *                           the denominator is an exact integer in any order.  mode and out_ld as stp_predict_finish's: 0 fp32 [h][w][C],
 *                           1 uint8 (uint8)(value * 255.f), 2 uint8 [h][w] first index of the largest value (a NaN never wins) or,
 *                           C == 1, value > 0.5f; rows of `out` lie out_ld PIXELS apart. */
int stp_window_gather_u8(const uint8_t* img, int32_t h, int32_t w, int32_t C, const int32_t* origins, int32_t n, uint8_t* dst, int32_t H,
                         int32_t W, void* stream);
int stp_window_accumulate(const float* acc, int32_t H, int32_t W, int32_t C, const int32_t* origins, int32_t n, int32_t overlap,
                          float* canvas, int32_t h, int32_t w, void* stream);
int stp_window_finish(const float* canvas, int32_t h, int32_t w, int32_t C, int32_t k, const float* sy, const float* sx, int32_t mode,
                      void* out, int32_t out_ld, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Masks on the device (csrc/mask.hip): what is done with ONE image's finished fp32 map [h][w][C] (stp_predict_finish mode 0) - threshold,
 * disk erosion / dilation, the run-length code, the counters of a threshold sweep.  uint8, fp32 and integers only (both builds export the
 * same code); all of it exact integer work, equal to the host statement (numpy, scipy.ndimage, segmentation_pipeline/impl/rle.py) bit for
 * bit.  No float atomics; element indices are int64; no result depends on an order.  Masks are uint8 {0, 1} (any non-zero input byte
 * counts as 1).  STP_E_BADARG before any launch: a NULL pointer, a size <= 0, and what each entry lists.
 *
 *   stp_mask_threshold : out[y][x] (rows out_ld >= w bytes apart) = mode 0: map[y][x][channel] > threshold, compared in fp32 (the caller
 *                        rounds its threshold to fp32 once - what `arr > 0.25` does on a float32 array; a NaN is never larger);  mode 1: the
 *                        first index of the largest of the C values == channel (stp_predict_finish mode 2's rule; C <= 32; `threshold`
 *                        unused).  One 16-byte store per 16 pixels where `out` is 16-byte aligned and out_ld % 16 == 0, else one byte per
 *                        thread.  BADARG: channel outside 0..C-1, mode outside 0..1, out_ld < w, mode 1 with C > 32.
 *   stp_mask_morph     : dst[h][w] = binary erosion (op 0) or dilation (op 1) of src[h][w] by the disk dx*dx + dy*dy <= r*r (skimage's
 *                        disk(r)), 1 <= r <= 7, pixels outside the image reading as 0 for BOTH ops; src != dst.  Opening = erode, dilate;
 *                        closing = dilate, erode: the pair equals scipy.ndimage.binary_opening / binary_closing(mask, disk(r)) with scipy's
 *                        DEFAULTS (border_value = 0) - including that such a closing clears a band of r pixels at the image border (an
 *                        all-ones 9 x 11 image closes to 35 ones with r = 2, and opens to 87).  LDS tiles of 64 rows x 256 columns of bits
 *                        with an r-wide halo.  BADARG: r outside 1..7, op outside 0..1, src == dst.
 *   stp_mask_rle       : the reference's run-length code of img[h][w]: pixels numbered 1-based COLUMN-major (x * h + y + 1); a run that
 *                        reaches the bottom of a column and goes on at the top of the next is one run (the flat array decides).
 *                        *count = number of runs, runs[k] = (start, length) int32 pairs for k < count, ascending; pairs past count are
 *                        not written.  h * w < 2^31; capacity (pairs `runs` holds) >= (h*w + 1) / 2, the most an image can have, else
 *                        BADARG; workspace (8-byte aligned) >= stp_mask_rle_workspace_bytes(h, w) (0 for sizes it refuses), else
 *                        STP_E_WORKSPACE.  64 x 64 tiles are transposed through LDS into a column-major bit stream (global loads stay
 *                        row-contiguous); run ends and the last run start are counted per workgroup, one workgroup scans them in order,
 *                        a compacting launch writes the pairs.
 *   stp_threshold_counts : ONE pass over the map for T <= 64 thresholds (a HOST pointer; finite and strictly ascending, else BADARG),
 *                        against target[h][w] (uint8, non-zero = positive):  counts[t][0] = pixels with map[..][channel] > thresholds[t]
 *                        (fp32 compare, a NaN never),  counts[t][1] = those of them with target != 0;  totals[0] = positives of the
 *                        target, totals[1] = h * w.  int64 device outputs.  Per pixel j = #thresholds below the value goes into a
 *                        workgroup's integer LDS table [T + 1][2]; a finalize launch sums the tables and takes the suffix sums.
 *                        h * w < 2^40; workspace >= stp_threshold_counts_workspace_bytes(T) (0 for T outside 1..64), else
 *                        STP_E_WORKSPACE. */
int stp_mask_threshold(const float* map, int32_t h, int32_t w, int32_t C, int32_t channel, int32_t mode, float threshold, uint8_t* out,
                       int32_t out_ld, void* stream);
int stp_mask_morph(const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t r, int32_t op, void* stream);
size_t stp_mask_rle_workspace_bytes(int32_t h, int32_t w);
int stp_mask_rle(const uint8_t* img, int32_t h, int32_t w, int32_t* runs, int32_t* count, int64_t capacity, void* workspace,
                 size_t workspace_bytes, void* stream);
size_t stp_threshold_counts_workspace_bytes(int32_t T);
int stp_threshold_counts(const float* map, const uint8_t* target, int32_t h, int32_t w, int32_t C, int32_t channel, const float* thresholds,
                         int32_t T, int64_t* counts, int64_t* totals, void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Connected components on the device (csrc/components.hip): the objects of ONE uint8 mask [h][w] - what scipy.ndimage.label and
 * skimage's remove_small_objects / remove_small_holes compute - and the run-length code of a label image, one triple per run
 * (segmentation_pipeline/impl/rle.py: multi_rle_encode).  uint8, int32 and int64 only (both builds export the same code); exact integer
 * work, equal to the host statement (tests/_components_reference.py) bit for bit and from run to run.  Only integer atomics (atomicMin on
 * the union-find's parents, atomicAdd on the areas); no workgroup waits for another.  The rules of the mask entries hold: STP_E_BADARG
 * before any launch for a NULL pointer, a size <= 0 and what each entry lists; never a synchronisation or an allocation; h * w < 2^31;
 * workspace 8-byte aligned and >= the entry's *_workspace_bytes(h, w) (0 for sizes it refuses), else STP_E_WORKSPACE.
 *
 *   stp_mask_label       : foreground = (img[y][x] != 0) != (invert != 0).  labels[y * w + x] = 0 off the foreground, else the number
 *                          1..*count of the pixel's component under the 4-neighbourhood (connectivity 1) or the 8-neighbourhood (2);
 *                          components are numbered by their first pixel in row-major order:  root = the smallest pixel index y * w + x
 *                          of the component, label = the number of roots at or before it.  This is scipy.ndimage.label(fg,
 *                          generate_binary_structure(2, connectivity)).  Every cell of `labels` and *count are written (int32, device).
 *                          BADARG: connectivity outside 1..2.
 *   stp_mask_area_filter : area(c) = the pixel count of foreground component c.  invert 0: dst = (src != 0) with the pixels of every
 *                          component of area < min_size cleared (skimage's remove_small_objects(mask, min_size, connectivity): label,
 *                          bincount, sizes < min_size - a strict <).  invert 1, foreground = the ZERO pixels: dst = (src != 0) with the
 *                          pixels of every zero component of area < min_size set (remove_small_holes(mask, area_threshold = min_size,
 *                          connectivity) = ~remove_small_objects(~mask, ...): a small zero component at the image border is filled
 *                          too).  dst is uint8 {0, 1}; min_size = 0 (and 1) gives the binarised source.  src == dst is allowed: the
 *                          FIRST launch is the only one that reads src (it turns it into the parent array: >= 0 on the foreground), the
 *                          LAST is the only one that writes dst, and the one-launch form for min_size <= 1 reads and writes a pixel in
 *                          one thread.  BADARG: connectivity outside 1..2, min_size < 0.
 *   stp_label_rle        : the column-major numbering of stp_mask_rle (1-based x * h + y + 1) on an int32 image with values >= 0 (any
 *                          such image, not only stp_mask_label's).  A run is a maximal stretch of EQUAL NON-ZERO values of the flat
 *                          column-major array: a stretch that leaves the bottom of a column and goes on at the top of the next with the
 *                          same value is one run, with another value two.  runs[k] = (value, start, length) int32 triples for
 *                          k < *count in ascending start; triples past *count are not written.  capacity (triples `runs` holds) >=
 *                          h * w, the most a label image can have, else BADARG.  The triples of one value, in order, are the runs of
 *                          rle_encode(labels == value). */
size_t stp_mask_label_workspace_bytes(int32_t h, int32_t w);
int stp_mask_label(const uint8_t* img, int32_t h, int32_t w, int32_t connectivity, int32_t invert, int32_t* labels, int32_t* count,
                   void* workspace, size_t workspace_bytes, void* stream);
size_t stp_mask_area_filter_workspace_bytes(int32_t h, int32_t w);
int stp_mask_area_filter(const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t connectivity, int32_t invert, int64_t min_size,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t stp_label_rle_workspace_bytes(int32_t h, int32_t w);
int stp_label_rle(const int32_t* labels, int32_t h, int32_t w, int32_t* runs, int32_t* count, int64_t capacity, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Object-level matching of two label images on the device (csrc/object_match.hip): the counters of the per-object competition scores
 * (Airbus ship detection: F2 over IoU thresholds; DSB-2018: TP / (TP + FP + FN)).  int32 and int64 only (both builds export the same
 * code); no float arithmetic; exact integer work, equal to the host statement (tests/_object_match_reference.py) and byte-identical from
 * run to run.  Only integer atomics (a 64-bit atomicCAS on a table key whose return value decides, atomicAdd on counts, areas and
 * counters); no workgroup waits for another.  The rules of the component entries hold: STP_E_BADARG before any launch for a NULL pointer,
 * a size <= 0 and what is listed below; never a synchronisation or an allocation; h * w < 2^31; workspace 8-byte aligned and >= the
 * entry's *_workspace_bytes(h, w) (0 for sizes it refuses), else STP_E_WORKSPACE.
 *
 *   pred, truth : int32 label images [h][w], 0 = background; ANY label images (values need not be contiguous), not only stp_mask_label's.
 *   label_cap   : labels lie in 0..label_cap; 0 <= label_cap <= h * w, else BADARG (stp_mask_label's output: (h * w + 1) / 2 is enough).
 *                 A value outside 0..label_cap (a negative one too) is background in that image - it never becomes an index - and the
 *                 pixel is counted once, in either image or both, as out of range.
 *   arithmetic  : A_p[a], A_g[b] = the pixel counts of the labels;  I[a][b] = the pixels with pred = a and truth = b, both > 0;
 *                 U = A_p[a] + A_g[b] - I.  The thresholds are t_k = iou_num[k] / iou_den (iou_num: a HOST pointer to T int32):
 *                 1 <= T <= 64, 1 <= iou_den <= 1000, iou_den <= 2 * iou_num[k], iou_num[k] <= iou_den, strictly ascending, else BADARG.
 *                 The pair (a, b) matches at t_k iff  I * iou_den > iou_num[k] * U  in int64 - the strict iou > t of the competitions'
 *                 notebooks; t = 1 matches nothing.  As t >= 1/2 a label has at most one partner, so TP_k = the number of matching pairs:
 *                 there is no assignment step.
 *   the table   : row stretches of equal (pred, truth), both non-zero, found with wave ballots, make one insert each into an
 *                 open-addressing table keyed by (a << 32) | b.  It has the smallest power of two >= 2 * h * w slots (12 bytes each)
 *                 and at most h * w keys - every pair owns a pixel -, so the load stays <= 1/2 and every probe sequence ends.  Its clear
 *                 and its final pass cost in proportion to the slots, not to the pairs.
 *
 *   stp_label_match    : out (int64, device, 8-byte aligned, T + 3 entries, all written):  out[k] = TP_k for k < T,  out[T] = the pred
 *                        labels with A_p > 0,  out[T + 1] = the truth labels with A_g > 0,  out[T + 2] = the out-of-range pixels.
 *                        3 launches: clear, count (areas + table), finalize (T comparisons per pair, pre-summed per workgroup).
 *   stp_label_overlaps : the same inputs without thresholds.  triples[k] = (a, b, I) int32 for k < *count, the non-empty pairs in an
 *                        UNSPECIFIED order (sort them); triples past *count are not written.  capacity (triples it holds) >= h * w, else
 *                        BADARG.  area_p, area_g: int32 [label_cap + 1], all written (entry 0 is 0).  *out_of_range: int64, 8-byte
 *                        aligned.  3 launches: clear, count, emit. */
size_t stp_label_match_workspace_bytes(int32_t h, int32_t w);
int stp_label_match(const int32_t* pred, const int32_t* truth, int32_t h, int32_t w, int32_t label_cap, const int32_t* iou_num, int32_t T,
                    int32_t iou_den, int64_t* out, void* workspace, size_t workspace_bytes, void* stream);
size_t stp_label_overlaps_workspace_bytes(int32_t h, int32_t w);
int stp_label_overlaps(const int32_t* pred, const int32_t* truth, int32_t h, int32_t w, int32_t label_cap, int32_t* triples, int32_t* count,
                       int64_t capacity, int32_t* area_p, int32_t* area_g, int64_t* out_of_range, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ----------------------------------------------------------------------------------------------
 * Splitting touching objects on the device (csrc/split.hip): a component of ONE uint8 mask [h][w] is cut at its necks - the cores of the
 * distance transform are numbered and grown back.  uint8 and int32 only (both builds export the same code); exact integer work, equal
 * to the host statement (tests/_split_reference.py) bit for bit and byte-identical from run to run; no atomics, no workgroup waits for
 * another, and within a launch no workgroup reads what another one writes.  The rules of the component entries hold: STP_E_BADARG
 * before any launch for a NULL pointer, h or w < 1 and what is listed below; never a synchronisation or an allocation; workspace
 * 8-byte aligned and >= the entry's *_workspace_bytes(h, w) (0 for sizes it refuses), else STP_E_WORKSPACE.  Sizes: h, w <= 32767 and
 * h * w < 2^31, else BADARG - D2 <= 2 * 32766^2 = 2147221512 then stays below 2147483647 and every product is an int32.
 *
 * The arithmetic.  M = the mask (any non-zero byte is foreground), c2 >= 0 an integer, the squared core distance (a radius r: c2 =
 * floor(r * r); as D2 is an integer, D2 > r^2 is D2 > c2).
 *   1. D2[p] = 0 off the foreground, else min over the background pixels q of the image of |p - q|^2 (int32); what lies outside the image
 *      is not background.  With at least one zero in M this is the exact integer squared distance of scipy.ndimage.distance_transform_edt.
 *      With no zero pixel anywhere every D2 is 2147483647.
 *   2. Cores C = {D2 > c2}, numbered 1..nc by stp_mask_label with connectivity 2.
 *   3. Growth: a foreground pixel outside C takes the label of the core that reaches it first through foreground pixels over the
 *      8-neighbourhood, the smaller label winning a tie: (length of a shortest 8-path inside M, label) is the lexicographically smallest
 *      pair over all cores; equally, the synchronous iteration "every unlabelled foreground pixel with a labelled neighbour takes the
 *      smallest neighbouring label" until nothing changes.  Every resulting object is 8-connected.
 *   4. The foreground pixels still at 0 (components without a core) are numbered 1..nr by stp_mask_label, connectivity 2, and take
 *      nc + that number; nc + nr objects in all.  c2 = 0 makes the whole mask core: the result is stp_mask_label(M, connectivity 2).
 *
 *   stp_mask_edt        : d2[h][w] (int32, all written) = D2 of img.  2 launches: rows (one wave per row, the nearest zero from 64-lane
 *                         ballots, a uint16 distance per pixel in the workspace), columns (a workgroup holds 32 columns of those in LDS
 *                         - h <= 1024, else it reads them from global memory - and each pixel looks at the rows dy = 1, 2, ... above
 *                         and below while dy * dy < its best).
 *   stp_edt_threshold   : out[h][w] (uint8 {0, 1}) = d2 > c2.  BADARG: c2 < 0.  One d2 serves many c2.
 *   stp_label_grow      : labels[h][w] (int32, all written) = seeds[h][w] (int32, 0 = none, else 1..h * w; ANY such image, not only
 *                         cores; a seed off the foreground is dropped) grown through mask by stp_label_grow_rounds() = 32 synchronous
 *                         rounds of rule 3, fewer if the state stops changing (the rounds after that do nothing).  *changed (int32,
 *                         device) = 1 if the last round still changed a pixel - call again with seeds = labels (seeds == labels is
 *                         allowed) until it is 0 -, else 0.  1 + 32 launches that ping-pong between labels and the workspace; a round
 *                         reads the "changed" word the round before it wrote.
 *   stp_label_unclaimed : out[h][w] (uint8 {0, 1}) = mask != 0 and labels == 0.
 *   stp_label_merge     : labels[i] = rest[i] + *nc where rest[i] != 0, else unchanged; *total = *nc + *nr.  nc, nr, total: int32 on the
 *                         device (read there: no host round trip); total is neither nc nor nr and rest is not labels, else BADARG. */
size_t stp_mask_edt_workspace_bytes(int32_t h, int32_t w);
int stp_mask_edt(const uint8_t* img, int32_t h, int32_t w, int32_t* d2, void* workspace, size_t workspace_bytes, void* stream);
int stp_edt_threshold(const int32_t* d2, int32_t h, int32_t w, int32_t c2, uint8_t* out, void* stream);
size_t stp_label_grow_workspace_bytes(int32_t h, int32_t w);
int32_t stp_label_grow_rounds(void);
int stp_label_grow(const uint8_t* mask, const int32_t* seeds, int32_t h, int32_t w, int32_t* labels, int32_t* changed, void* workspace,
                   size_t workspace_bytes, void* stream);
int stp_label_unclaimed(const uint8_t* mask, const int32_t* labels, int32_t h, int32_t w, uint8_t* out, void* stream);
int stp_label_merge(const int32_t* rest, const int32_t* nc, const int32_t* nr, int32_t h, int32_t w, int32_t* labels, int32_t* total,
                    void* stream);

/* ----------------------------------------------------------------------------------------------
 * Per-object measurements of a label image on the device (csrc/measure.hip): area, sums of the coordinates, a fixed-point confidence and
 * the bounding box per label, and the selection of the objects that are large and confident enough.  int32, int64 and fp32 only (both
 * builds export the same code); after the quantisation below everything is exact integer work, equal to the host statement
 * (tests/_measure_reference.py) bit for bit and byte-identical from run to run.  Only integer atomics (64-bit atomicAdd on the sums, int32
 * atomicMin / atomicMax on the boxes, in LDS and in global memory); no workgroup waits for another.  The rules of the component entries
 * hold: STP_E_BADARG before any launch for a NULL pointer, a bad size and what is listed below; never a synchronisation or an allocation;
 * workspace 8-byte aligned and >= stp_label_select_workspace_bytes(label_cap) (0 for label_cap < 0), else STP_E_WORKSPACE.  Sizes:
 * 1 <= h, w <= 32767 (so h * w < 2^31), else BADARG.
 *
 *   labels    : an int32 label image [h][w], 0 = background; ANY label image (values need not be contiguous), not only stp_mask_label's.
 *   label_cap : labels lie in 0..label_cap; 0 <= label_cap <= h * w, else BADARG.  A value outside 0..label_cap (a negative one too) is
 *               background - it never becomes an index - and its pixel is counted in *out_of_range (int64, 8-byte aligned).
 *   probs     : fp32 [h][w][C] or NULL; with probs, C >= 1 and 0 <= channel < C, else BADARG; with NULL, C and channel are ignored.
 *   q         : the fixed-point probability of a pixel, q = (int) (clamp(p, 0, 1) * 65535.0f) with p = probs[y][x][channel]: one fp32
 *               multiply and one truncation, 0..65535, a NaN gives 0 - numpy's (np.clip(p, 0, 1).astype(np.float32) *
 *               np.float32(65535)).astype(np.int64) with NaN set to 0 first.  q = 0 without probs.
 *   the table : for every label k in 0..label_cap (all rows written; sums 8-byte aligned)
 *                 sums[k]  (int64 x 4) = (area = its pixel count, the sum of its y, the sum of its x, the sum of its q)
 *                 boxes[k] (int32 x 4) = (min y, min x, max y, max x), CLOSED; (h, w, -1, -1) for a label without a pixel.
 *               Row 0 is all zero with that empty box.  Derived on the host in float64: cy = sum y / area, cx = sum x / area, confidence =
 *               sum q / (65535 * area), the half-open box (min y, min x, max y + 1, max x + 1) = scipy.ndimage.find_objects' slices.
 *   selection : label k is kept iff  area > 0,  area >= min_area  and  sum q * conf_den >= conf_num * 65535 * area  in int64 (area < 2^31:
 *               both products stay below 2^61).  min_area >= 0, 1 <= conf_den <= 10000, 0 <= conf_num <= conf_den, else BADARG.  The kept
 *               labels keep their order and are renumbered 1..*count.
 *
 *   stp_label_measure : 2 launches: clear (the table, the counter), measure.  A wave owns 64 consecutive pixels of a row; a stretch of
 *                       equal labels contributes once - its length, y * length, the closed-form sum of its x, its sum of q from the
 *                       wave's prefix sum, and y, first x, last x for the box.  A workgroup combines the stretches of up to 128 labels in
 *                       LDS and adds each once to global memory; what does not fit the LDS table goes there directly.
 *   stp_label_select  : out_labels[i] = the new number of labels[i], 0 for a label that is dropped or out of range (out_labels == labels
 *                       is allowed: a pixel is read and written by one thread).  *count (int32, device) = the kept labels.
 *                       out_sums[new], out_boxes[new] = the kept rows in the new numbering; row 0 as above; rows past *count are not
 *                       written (room for label_cap + 1 rows is enough).  out_sums == sums or out_boxes == boxes: BADARG.  4 launches:
 *                       the kept labels per block of 256, one workgroup that scans the blocks in order, the map old -> new with the
 *                       rows' copy, the pass over the image.  workspace: the map and the block counts. */
int stp_label_measure(const int32_t* labels, const float* probs, int32_t h, int32_t w, int32_t C, int32_t channel, int32_t label_cap,
                      int64_t* sums, int32_t* boxes, int64_t* out_of_range, void* stream);
size_t stp_label_select_workspace_bytes(int32_t label_cap);
int stp_label_select(const int32_t* labels, int32_t h, int32_t w, int32_t label_cap, const int64_t* sums, const int32_t* boxes,
                     int64_t min_area, int32_t conf_num, int32_t conf_den, int32_t* out_labels, int32_t* count, int64_t* out_sums,
                     int32_t* out_boxes, void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * U-Net border weight maps on the device (csrc/border_weight.hip) and the one-class loss that takes them (csrc/loss_sigmoid.hip):
 *   w(x) = w_c(x) + w0 * exp(-(d1(x) + d2(x))^2 / (2 sigma^2))      (Ronneberger et al. 2015, eq. 2)
 * with d1, d2 the distances from a background pixel to the nearest and the second-nearest object, truncated to a window.  int32 and fp32
 * only (both builds export the same code); the distances are exact integer work, equal to the host statement
 * (tests/_border_weight_reference.py); no atomics, no workgroup waits for another, byte-identical from run to run.  STP_E_BADARG before any
 * launch for a NULL pointer (d1sq, d2sq may be NULL), N, H or W < 1, N * H * W >= 2^31, radius outside 1..32, w0 < 0, sigma <= 0, b0 or
 * b1 <= 0 or any of them not finite; never a synchronisation or an allocation; workspace 8-byte aligned and >=
 * stp_border_weight_workspace_bytes(N, H, W) (0 for sizes it refuses), else STP_E_WORKSPACE.
 *
 *   labels  : int32 [N][H][W], 0 on the background, > 0 on objects; ANY image with values >= 0, not only stp_mask_label's.  Two pixels
 *             with different non-zero values belong to different objects (neighbours too); equal values are one object.
 *   window  : for a pixel p of sample n, the pixels q of the SAME sample with |qy - py| <= R and |qx - px| <= R (R = radius), clipped to
 *             the image.  It never reaches into the neighbouring sample of the batch.
 *   D1^2(p) : the smallest |p - q|^2 over the labelled pixels of the window (int32); L1 = the label of one such nearest pixel (a tie
 *             between labels may be broken either way: nothing below depends on it).  A foreground pixel is its own nearest: D1^2 = 0.
 *   D2^2(p) : the smallest |p - q|^2 over the labelled pixels of the window whose label differs from L1.
 *             Either is -1 when no such pixel exists.
 *   term(p) = w0 * exp(-(sqrt(D1^2) + sqrt(D2^2))^2 / (2 sigma^2)) on the background where D2^2 >= 0, else 0.
 *   weights[p] = (labels[p] ? b1 : b0) + term(p), evaluated in fp32 (class_balance = (b0, b1)).
 *   The window truncates the usual statement (per label distance_transform_edt, the two smallest): a pixel the window drops has
 *   d2 >= R + 1, so the two differ by less than w0 * exp(-(R + 1)^2 / (2 sigma^2)).
 *   Separable and still exact, 2 launches over the whole batch: rows (per pixel the nearest labelled pixel of its row within +-R as
 *   (dxA, labelA) and the nearest one whose label != labelA as dxB, 8 bytes per pixel in the workspace), columns (dy in -R..R twice:
 *   (D1^2, L1) from the A candidates, then per row dxA if labelA != L1, else dxB).
 *   d1sq, d2sq : int32 [N][H][W] or NULL: D1^2 and D2^2, all written.
 *
 *   stp_sigmoid_bce_dice_weighted : stp_sigmoid_bce_dice with a pixel-weight operand, pixel_weights fp32 [count], every one > 0 (the map
 *             above).  weighted_binary_crossentropy = sum_i w_i * bce_i / count (the Keras sample-weight rule; no zero weights, so its
 *             non-zero-weight normaliser is 1), bce_i the sibling's expression, clip included;
 *             loss = w_bce * weighted_binary_crossentropy + w_dice * dice_loss.  The weights enter neither dice_loss nor any logged
 *             overlap or accuracy.  scalars (fp32[16]): [0..9] as the sibling with [0] the loss above and [1] the UNWEIGHTED
 *             binary_crossentropy, [13] weighted_binary_crossentropy, [15] the mean of the weights; [10..12], [14] are not written.
 *             dlogits: the sibling's, the cross-entropy part multiplied by w_i, then by grad_scale; padding channels exactly 0.
 *             Deterministic (fixed-order reduction, no atomics).  Workspace: stp_loss_workspace_bytes().  It leaves no bias-gradient sums
 *             (stp_sigmoid_loss_bias_grad does not follow it).  BADARG as the sibling, and for NULL pixel_weights. */
size_t stp_border_weight_workspace_bytes(int32_t N, int32_t H, int32_t W);
int stp_border_weight(const int32_t* labels, int32_t N, int32_t H, int32_t W, float w0, float sigma, int32_t radius, float b0, float b1,
                      float* weights, int32_t* d1sq, int32_t* d2sq, void* workspace, size_t workspace_bytes, void* stream);
int stp_sigmoid_bce_dice_weighted(const void* logits, const uint8_t* target, int64_t count, int32_t dtype, float w_bce, float w_dice,
                                  float* scalars, void* dlogits, int32_t dl_channels, float grad_scale, void* workspace,
                                  size_t workspace_bytes, const float* pixel_weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STP_HIP_H */

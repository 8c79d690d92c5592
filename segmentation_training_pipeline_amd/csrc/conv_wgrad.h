// What the translation units of the weight-gradient family share (conv_wgrad.hip: the pixel-reduction GEMM, its reduces and every
// single-layer entry point; conv_wgrad_row.hip: the row-of-taps kernels; conv_wgrad_taps9.hip: the all-taps kernels;
// conv_wgrad_group.hip: the stream-K planner and the entry points of the grouped launch): the kernel argument block, the LDS tile
// address, the group table, and the host decisions every unit has to take the same way - stated here once.
#pragma once
#include "common.h"
#include "launch.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));

struct WgradArgs {
  const char* src0;
  const char* src1;
  const char* dy;
  float* out;  // slabs [splits][Cout][K]
  int N, Hs0, Ws0, Hv, Wv, C0, C1, Ctot, mode;
  int KH, KW, stride, pad, Ho, Wo, Cout;
  int K, P, HoWo;
  int ntile_m, ntile_n, steps_per_split, nsteps;
  int xcd;   // XCD-contiguous block order
  int rowu;  // every pixel step lies inside one image and starts on an output-row boundary pattern (see ROWU)
  uint32_t bytes0, bytes1, bytesdy;
  FastDiv divC, divKW, divHoWo, divWo;
  BnBack pbn;   // row-of-taps kernel: src0 is the tensor BEFORE a BatchNormalization(+activation), normalised in LDS (pbn.x unused)
};

#define STP_OOB 0x80000000u  // buffer voffset beyond any descriptor -> the load returns 0
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// byte address of (row, byte-in-row) in a pixel-major tile whose rows are ROWB bytes
template <int ROWB> __device__ __forceinline__ int tile_addr(int row, int byte) {
  constexpr int U = ROWB / 32;
  constexpr int R = U >= 8 ? 1 : 8 / U;
  constexpr int M = (U >= 8 ? 8 : U) - 1;
  const int s = (row / R) & M;
  return row * ROWB + (byte ^ (s << 5));
}

// the table of a grouped launch (conv_wgrad_group.hip builds it, the kernels of conv_wgrad_row.hip and conv_wgrad_taps9.hip walk it)
struct WgLayer {
  WgradArgs a;
  float* dw;
  int accumulate, tile0, pad0, pad1;
};
struct WgSeg { int layer, tile, step0, step1, slot, pad0, pad1, pad2; };
struct WgTile { int layer, t, list0, nslots; };        // the tile's partial slabs: slot_list[list0 .. list0 + nslots), in line order
struct WgGroupHeader {
  int magic, bm, n_layers, n_segs, n_wg, n_tiles;
  int off_layers, off_segs, off_first, off_tiles;      // byte offsets from the start of the table
  int total_bytes, off_slots;
  int reduce_lanes, xcd, pbn, taps9;                    // lanes per element of the reduce launch (1 or 4); xcd: contiguous line runs per XCD;
};                                                      // pbn: some layer normalises its src0 in LDS (fused producer BatchNormalization);
                                                        // taps9: all-taps tiles (conv_wgrad_taps9_group_kernel) instead of row-of-taps tiles
#define WG_GROUP_MAGIC 0x57474733

// dword-wise copy of a descriptor through the constant address space (scalar, invariant loads)
template <typename T> __device__ __forceinline__ void load_constant(T& dst, const T* src) {
  static_assert(sizeof(T) % 4 == 0, "dwords");
  typedef const __attribute__((address_space(4))) uint32_t* cptr_t;
  const cptr_t q = (cptr_t)(reinterpret_cast<const uint32_t*>(src));
  uint32_t* d = reinterpret_cast<uint32_t*>(&dst);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); ++i) d[i] = q[i];
}

struct WgradPlan {
  int tile, bm, bn, ntile_m, ntile_n, splits, steps_per_split, nsteps;
};

extern "C" int stp_wgrad_sc_eligible(const stp_wgrad_params* p);
extern "C" int stp_wgrad_sc_slabs(const stp_wgrad_params* p);
extern "C" int stp_wgrad_sc_partial(const stp_wgrad_params* p, void* workspace, void* stream);
#define WG_TILE_SC 100  // small-channel halo-tile kernel (conv_sc_wgrad.hip): splits = number of persistent workgroups
#define WG_TILE_ROW128 5  // row-of-taps kernels (conv_wgrad_row.hip); 1-4 are the GEMM tiles of conv_wgrad.hip
#define WG_TILE_ROW64 6

// ---- host side -------------------------------------------------------------------------------------------------------------------
// (hidden: defined in one unit, called from another, nothing added to the library's exported symbols)
#define STP_LIB_HIDDEN __attribute__((visibility("hidden")))

// The kernel family of a single-layer launch.  stp_conv2d_wgrad_partial, _reduce, _kernel_id and stp_wgrad_reduce_desc_fill all ask
// here, so a partial launch and its reduce cannot disagree.  variant: 0 = automatic, 1-3 = the GEMM forms, 4 = row-of-taps.
enum WgradPath { WG_PATH_GEMM, WG_PATH_SC, WG_PATH_ROW };
STP_LIB_HIDDEN WgradPath wgrad_path(const stp_wgrad_params* p, int variant);

// The output-channel class of the row-of-taps and all-taps kernels -> the instance: f(RowClass<BM, WM, WN>{}).  The grouped launches
// have a 32-channel class, the single-layer kernels (WITH32 = false) do not.
template <int BM_, int WM_, int WN_> struct RowClass { static constexpr int BM = BM_, WM = WM_, WN = WN_; };
template <bool WITH32 = true, typename F> static inline int row_class(int bm, F&& f) {
  if (bm == 128) return f(RowClass<128, 2, 2>{});
  if (bm == 64) return f(RowClass<64, 1, 4>{});
  if constexpr (WITH32) {
    if (bm == 32) return f(RowClass<32, 1, 4>{});
  }
  return STP_E_BADARG;
}

// slab sizes in bytes: plain [splits][Cout][K]; row-of-taps, fragment-major whole tiles; one slab per segment of a group
static inline size_t wgrad_slab_bytes(const stp_wgrad_params* p, int splits) {
  return (size_t)splits * p->Cout * p->KH * p->KW * (p->C0 + p->C1) * sizeof(float);
}
static inline size_t wgrad_row_slab_bytes(const WgradPlan& r) { return (size_t)r.splits * r.ntile_m * r.ntile_n * r.bm * 192 * sizeof(float); }
static inline size_t wg_group_slab_bytes(size_t n_segs, int bm, bool taps9) { return n_segs * (size_t)bm * (taps9 ? 576 : 192) * sizeof(float); }

template <typename K>
static int launch_wg(K kern, WgradArgs& a, size_t lds, int splits, hipStream_t s) {
  return stp_launch_lds(kern, dim3(a.ntile_m * a.ntile_n * splits), dim3(256), lds, s, a);
}

// conv_wgrad.hip
STP_LIB_HIDDEN void wgrad_choose_splits(WgradPlan& w, int asked, int target);
STP_LIB_HIDDEN int wgrad_fill(const stp_wgrad_params* p, void* workspace, size_t workspace_bytes, WgradArgs& a, WgradPlan& w, bool* c4_out,
                              bool* dma_out);
// conv_wgrad_row.hip
STP_LIB_HIDDEN bool wgrad_row_eligible(const stp_wgrad_params* p);
STP_LIB_HIDDEN bool wgrad_row_auto(const stp_wgrad_params* p);
STP_LIB_HIDDEN WgradPlan plan_wgrad_row(const stp_wgrad_params* p);
STP_LIB_HIDDEN int wgrad_row_partial(const stp_wgrad_params* p, WgradArgs& a, hipStream_t s);
STP_LIB_HIDDEN int wgrad_row_reduce(const stp_wgrad_params* p, const void* workspace, hipStream_t s);
STP_LIB_HIDDEN int wgrad_row_group_partial(const WgGroupHeader* hd, const void* dev_table, void* workspace, hipStream_t s);
STP_LIB_HIDDEN int wgrad_row_group_reduce(const WgGroupHeader* hd, const void* dev_table, const void* workspace, hipStream_t s);
// conv_wgrad_taps9.hip
STP_LIB_HIDDEN int wgrad_taps9_group_partial(const WgGroupHeader* hd, const void* dev_table, void* workspace, hipStream_t s);
STP_LIB_HIDDEN int wgrad_taps9_group_reduce(const WgGroupHeader* hd, const void* dev_table, const void* workspace, hipStream_t s);

// The grouped weight-gradient launch: the stream-K planner, the table builder and the stp_wgrad_group_* entry points (conv_wgrad.h has
// the table's layout; the kernels that walk it and their launchers are in conv_wgrad_row.hip and conv_wgrad_taps9.hip).
#include "conv_wgrad.h"
#include <cstdlib>
#include <cstring>
#include <vector>

// ------------------------------------------------------------------------------------------------
// GROUPED launch (round 3).  A layer launched alone has 6-96 output tiles for 512-768 workgroup slots, so its pixel reduction was
// split 5-85 ways: ~12 steps per workgroup, a 3-stage pipeline fill and a 96 KB partial slab per 12 steps - the launch ran at
// 520-700 TFLOP/s and the slabs were 3.65x the algorithmic bytes (profiles/r02g_*).  The same kernel body with 130+ steps per
// workgroup reaches 1060-1070 TFLOP/s (scratch/r03_probe.py).  The weight gradients feed nothing but the optimizer, so the plan
// collects the layers of a stage and issues ONE launch for them: the (layer, tile, step) space of the group is laid out as a line
// (layer-major, tile, step), cut into one contiguous chunk per workgroup slot (stream-K), and a workgroup walks the segments of
// its chunk.  Every segment writes one partial slab; a tile is covered by 1-3 segments that `wgrad_group_reduce_kernel` sums in
// line order (fixed partition, fixed order: deterministic, no atomics) and scatters into dW.

// ---- grouped row-of-taps launch: host side -----------------------------------------------------------------------------------
// class of a layer = the output-channel tile of its kernel instance (layers of one group share it); 0 = not eligible
static int wg_group_bm(const stp_wgrad_params* p) {
  if (!p || !wgrad_row_eligible(p) || p->splits != 0) return 0;      // (a fused producer BatchNormalization: wgrad_row_eligible's rules)
  const int64_t lim = 1ll << 31;
  const int64_t P = (int64_t)p->N * p->Ho * p->Wo;
  if ((int64_t)p->N * p->Hs0 * p->Ws0 * p->C0 * 2 >= lim || (int64_t)p->N * p->Hv * p->Wv * p->C1 * 2 >= lim || P * p->Cout * 2 >= lim) return 0;
  return p->Cout <= 32 ? 32 : p->Cout <= 64 ? 64 : 128;
}
extern "C" int stp_wgrad_group_class(const stp_wgrad_params* p) { return wg_group_bm(p); }

struct WgGroupPlan {
  int bm = 0, max_slots_per_tile = 1;
  bool taps9 = false;      // all-taps tiles (BM x 576, one workgroup per CU) instead of row-of-taps tiles (BM x 192)
  std::vector<int> ntile_m, ntile_n, nsteps, tile0;
  std::vector<WgSeg> segs;
  std::vector<int> first;
  std::vector<WgTile> tiles;
  std::vector<int> slot_list;
};

static int wg_group_slots(int bm, bool taps9) {
  const int cus = stp_cu_count();
  static const int target = getenv("STP_WGRAD_GROUP_SLOTS") ? atoi(getenv("STP_WGRAD_GROUP_SLOTS")) : 0;
  if (target > 0) return target;
  if (taps9) return cus;                                 // 512 threads, 120-144 KB of LDS: one workgroup per CU
  return cus * (bm == 128 ? 2 : bm == 64 ? 3 : 4);     // co-resident workgroups: 77 KB of LDS / 224 registers at 128 channels, 52 KB / 144 and 40 KB / 114 below
}
// all-taps tiles for a group: every layer on a 16 / 32 / >= 64 pixel wide map (the kernel's three bodies), none with a fused producer
// BatchNormalization (that stays on the row-of-taps instance).  Default for the 128-channel class (profiles/r04f_*: the three groups
// 265 / 234 / 150 -> 210 / 173 / 117 us, 1150-1230 TFLOP/s, step 6.78 -> 6.64 ms on one box); STP_WGRAD_TAPS9=0 keeps the round-3 kernel.
static bool wg_group_taps9(const stp_wgrad_params* const* L, int n) {
  static const int mode = getenv("STP_WGRAD_TAPS9") ? atoi(getenv("STP_WGRAD_TAPS9")) : 1;      // 0: off; 1 (default): 128-channel class; 2: every class (tests)
  if (!mode) return false;
  // (the 64 / 32-channel classes: 32 / 16 output channels per wave against 9 taps x 16 input channels = 1.2 / 2 transpose reads per
  //  MFMA - LDS-bound, measured 25 % / 45 % slower than their row-of-taps instances, whose fabric traffic is already ~1x algorithmic)
  if (mode != 2 && wg_group_bm(L[0]) != 128) return false;
  for (int l = 0; l < n; ++l)
    if (L[l]->src_bn_mean || !(L[l]->Wo == 16 || L[l]->Wo == 32 || L[l]->Wo % 64 == 0)) return false;
  return true;
}

// The line: layer-major; inside a layer RANGE-major (a range = ~one workgroup chunk of steps), tile-minor - the tiles of a layer over
// the same pixel range are neighbours on the line, i.e. run at the same time on the same XCD (contiguous runs of the line per XCD)
// and share dY / x through its L2.  With the tile-major line of the first build a stage-1 layer (3 tiles x 4096 steps) put 43
// workgroups on 43 different pixel ranges of one tile: every operand byte came from HBM three times (541 TFLOP/s, 5.9 TB/s).
static int wg_group_plan(const stp_wgrad_params* const* L, int n, WgGroupPlan& g) {
  if (!L || n <= 0) return STP_E_BADARG;
  g.bm = wg_group_bm(L[0]);
  if (!g.bm) return STP_E_BADARG;
  g.taps9 = wg_group_taps9(L, n);
  int64_t total = 0;
  int ntiles = 0;
  for (int l = 0; l < n; ++l) {
    if (wg_group_bm(L[l]) != g.bm || !L[l]->src0 || !L[l]->dy || !L[l]->dw) return STP_E_BADARG;
    const int tm = ceil_div(L[l]->Cout, g.bm), tn = (g.taps9 ? 1 : 3) * ((L[l]->C0 + L[l]->C1) / 64);
    const int ns = (int)((int64_t)L[l]->N * L[l]->Ho * L[l]->Wo / 64);
    g.ntile_m.push_back(tm); g.ntile_n.push_back(tn); g.nsteps.push_back(ns); g.tile0.push_back(ntiles);
    ntiles += tm * tn;
    total += (int64_t)tm * tn * ns;
  }
  const int slots = wg_group_slots(g.bm, g.taps9);
  const int MINSEG = 8;       // no segment shorter than this unless its item is (a 3-stage pipeline fill + a slab per segment)
  int64_t chunk = (total + slots - 1) / slots;
  if (chunk < 2 * MINSEG) chunk = 2 * MINSEG;
  std::vector<std::vector<int>> lists;
  for (;; ++chunk) {
    g.segs.clear(); g.first.clear();
    lists.assign(ntiles, std::vector<int>());
    // items of the line: (layer, range, tile) -> steps [r * R, min(ns, (r + 1) * R))
    int l = 0, r = 0, t = 0, s = 0;
    auto ranges_of = [&](int l_) { int64_t nr = (g.nsteps[l_] + chunk / 2) / chunk; return (int)(nr < 1 ? 1 : nr); };
    auto rlen_of = [&](int l_) { return ceil_div(g.nsteps[l_], ranges_of(l_)); };
    while (l < n) {
      g.first.push_back((int)g.segs.size());
      int64_t rem = chunk;
      int mine = 0;
      while (rem > 0 && l < n) {
        const int R = rlen_of(l), i0 = r * R, i1 = (i0 + R < g.nsteps[l]) ? i0 + R : g.nsteps[l];
        const int avail = i1 - i0 - s;
        int take = (int)(rem < avail ? rem : avail);
        if (avail - take > 0 && avail - take < MINSEG) take = avail;             // do not leave a sliver of the item behind
        if (take < MINSEG && take < avail && mine > 0) break;                     // a sliver at the end of the chunk: the next workgroup takes it
        WgSeg sg = {l, t, i0 + s, i0 + s + take, (int)g.segs.size(), 0, 0, 0};
        lists[g.tile0[l] + t].push_back(sg.slot);
        g.segs.push_back(sg);
        ++mine;
        rem -= take; s += take;
        if (s == i1 - i0) {
          s = 0;
          if (++t == g.ntile_m[l] * g.ntile_n[l]) { t = 0; if (++r == ranges_of(l)) { r = 0; ++l; } }
        }
      }
    }
    g.first.push_back((int)g.segs.size());
    if ((int)g.first.size() - 1 <= slots) break;       // (slivers moved between neighbours can cost one workgroup more than the slots)
  }
  g.tiles.clear(); g.slot_list.clear(); g.max_slots_per_tile = 1;
  for (int l = 0; l < n; ++l)
    for (int t = 0; t < g.ntile_m[l] * g.ntile_n[l]; ++t) {
      const std::vector<int>& v = lists[g.tile0[l] + t];
      g.tiles.push_back(WgTile{l, t, (int)g.slot_list.size(), (int)v.size()});
      g.slot_list.insert(g.slot_list.end(), v.begin(), v.end());
      if ((int)v.size() > g.max_slots_per_tile) g.max_slots_per_tile = (int)v.size();
    }
  return STP_OK;
}

static size_t wg_align16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" size_t stp_wgrad_group_table_bytes(const stp_wgrad_params* const* layers, int32_t n) {
  WgGroupPlan g;
  if (wg_group_plan(layers, n, g) != STP_OK) return 0;
  return wg_align16(sizeof(WgGroupHeader)) + wg_align16(sizeof(WgLayer) * n) + wg_align16(sizeof(WgSeg) * g.segs.size()) +
         wg_align16(sizeof(int) * g.first.size()) + wg_align16(sizeof(WgTile) * g.tiles.size()) + wg_align16(sizeof(int) * g.slot_list.size());
}

extern "C" size_t stp_wgrad_group_workspace_bytes(const stp_wgrad_params* const* layers, int32_t n) {
  WgGroupPlan g;
  if (wg_group_plan(layers, n, g) != STP_OK) return 0;
  return wg_group_slab_bytes(g.segs.size(), g.bm, g.taps9);
}

// Fills `host_table` (stp_wgrad_group_table_bytes): the caller copies it to device memory and passes both to the launches
// (the header is read on the host, everything else on the device; the table holds the layers' device pointers).
extern "C" int stp_wgrad_group_build(const stp_wgrad_params* const* layers, int32_t n, void* host_table, size_t table_bytes) {
  WgGroupPlan g;
  int rc = wg_group_plan(layers, n, g);
  if (rc != STP_OK) return rc;
  if (!host_table || table_bytes < stp_wgrad_group_table_bytes(layers, n)) return STP_E_WORKSPACE;
  char* tb = (char*)host_table;
  WgGroupHeader hd = {};
  hd.magic = WG_GROUP_MAGIC; hd.bm = g.bm; hd.n_layers = n; hd.n_segs = (int)g.segs.size(); hd.n_wg = (int)g.first.size() - 1;
  hd.n_tiles = (int)g.tiles.size();
  size_t off = wg_align16(sizeof(WgGroupHeader));
  hd.off_layers = (int)off; off += wg_align16(sizeof(WgLayer) * n);
  hd.off_segs = (int)off; off += wg_align16(sizeof(WgSeg) * g.segs.size());
  hd.off_first = (int)off; off += wg_align16(sizeof(int) * g.first.size());
  hd.off_tiles = (int)off; off += wg_align16(sizeof(WgTile) * g.tiles.size());
  hd.off_slots = (int)off; off += wg_align16(sizeof(int) * g.slot_list.size());
  hd.total_bytes = (int)off;
  hd.reduce_lanes = g.max_slots_per_tile >= 12 ? 4 : 1;
  {
    static const int xcd_env = getenv("STP_WGRAD_GROUP_XCD") ? atoi(getenv("STP_WGRAD_GROUP_XCD")) : -1;
    // measured per group (profiles/r03f_group_xcd_ab.txt, r03g_*): one contiguous run per XCD wins (stage 1: 140 vs 181 us, stage 3: 224
    // vs 244) except where most of the work sits in layers of 64+ tiles over ONE pixel range (the 512-channel layers at 16 x 16 x 16:
    // 96 tiles x 64 steps - an XCD's 64 workgroups then fetch the same lines at the same time: 275 vs 247 us) -> identity there
    int64_t wide = 0, all = 0;
    for (int l = 0; l < n; ++l) {
      const int64_t wk = (int64_t)g.ntile_m[l] * g.ntile_n[l] * g.nsteps[l];
      all += wk;
      if (g.ntile_m[l] * g.ntile_n[l] >= 64) wide += wk;
    }
    hd.xcd = xcd_env >= 0 ? xcd_env : (2 * wide > all ? 0 : 1);
  }
  for (int l = 0; l < n; ++l)
    if (layers[l]->src_bn_mean) hd.pbn = 1;
  {
    // the v_mfma_f32_32x32x16 form of the 128-channel instance: OPT-IN (STP_WGRAD_TAPS9_M32=1) - measured equal to the 16 x 16 x 32 form
    // (profiles/r04j_m32_ab.txt: 7.33 vs 7.33 ms per step; the loop is not bound by the MFMA shape)
    static const bool m32 = getenv("STP_WGRAD_TAPS9_M32") && atoi(getenv("STP_WGRAD_TAPS9_M32")) == 1;
    hd.taps9 = g.taps9 ? ((m32 && g.bm == 128) ? 2 : 1) : 0;
  }
  memset(tb, 0, off);
  memcpy(tb, &hd, sizeof(hd));
  for (int l = 0; l < n; ++l) {
    WgLayer wl = {};
    WgradPlan w;
    bool c4, dma;
    rc = wgrad_fill(layers[l], (void*)tb, ~(size_t)0, wl.a, w, &c4, &dma);     // (workspace arguments: validation only, unused by the group)
    if (rc != STP_OK) return rc;
    if (!dma) return STP_E_BADARG;
    wl.a.out = nullptr;
    wl.a.ntile_m = g.ntile_m[l]; wl.a.ntile_n = g.ntile_n[l]; wl.a.nsteps = g.nsteps[l]; wl.a.steps_per_split = g.nsteps[l];
    wl.a.xcd = 0;
    wl.dw = layers[l]->dw; wl.accumulate = layers[l]->accumulate; wl.tile0 = g.tile0[l];
    memcpy(tb + hd.off_layers + sizeof(WgLayer) * l, &wl, sizeof(wl));
  }
  memcpy(tb + hd.off_segs, g.segs.data(), sizeof(WgSeg) * g.segs.size());
  memcpy(tb + hd.off_first, g.first.data(), sizeof(int) * g.first.size());
  memcpy(tb + hd.off_tiles, g.tiles.data(), sizeof(WgTile) * g.tiles.size());
  memcpy(tb + hd.off_slots, g.slot_list.data(), sizeof(int) * g.slot_list.size());
  return STP_OK;
}

static const WgGroupHeader* wg_group_header(const void* host_table) {
  const WgGroupHeader* hd = (const WgGroupHeader*)host_table;
  return (hd && hd->magic == WG_GROUP_MAGIC && (hd->bm == 32 || hd->bm == 64 || hd->bm == 128) && hd->n_wg > 0 && hd->n_tiles > 0) ? hd : nullptr;
}

extern "C" int stp_wgrad_group_partial(const void* host_table, const void* dev_table, void* workspace, size_t workspace_bytes, void* stream) {
  const WgGroupHeader* hd = wg_group_header(host_table);
  if (!hd || !dev_table || !workspace) return STP_E_BADARG;
  if (wg_group_slab_bytes((size_t)hd->n_segs, hd->bm, hd->taps9 != 0) > workspace_bytes) return STP_E_WORKSPACE;
  return hd->taps9 ? wgrad_taps9_group_partial(hd, dev_table, workspace, (hipStream_t)stream)
                   : wgrad_row_group_partial(hd, dev_table, workspace, (hipStream_t)stream);
}

extern "C" int stp_wgrad_group_reduce(const void* host_table, const void* dev_table, const void* workspace, void* stream) {
  const WgGroupHeader* hd = wg_group_header(host_table);
  if (!hd || !dev_table || !workspace) return STP_E_BADARG;
  return hd->taps9 ? wgrad_taps9_group_reduce(hd, dev_table, workspace, (hipStream_t)stream)
                   : wgrad_row_group_reduce(hd, dev_table, workspace, (hipStream_t)stream);
}

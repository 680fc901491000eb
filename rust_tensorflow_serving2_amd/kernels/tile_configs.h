// The tile configs of the GEMM / conv kernel families: the ONLY place a config
// is written down.  One `cfg` integer selects a row; the launchers' switches,
// the host-side queries (cgemm.h, bindings.cpp) and the tuner's tables
// (ops/tile_table.py parses this file) all derive from the lists below.
//
// Host-only, standard library only (a plain C++ compiler takes it alone).
// Keep the lists regular -- `#define TFSK_<FAMILY>_CONFIGS(X)`, one `X(...)`
// row of plain integers per line, comments in /* */ -- because Python reads
// them too.  Ids are never reused: 124..137 (the 32-deep k-tile and the
// persistent multi-tile cgemm builds) and 144/145 (the ping-pong halo kernel)
// took no picks in the tuned tables and were removed; they stay in git history.
#pragma once

namespace tfsk {

// igemm.hip: X(id, BM, BN, stages, waves_m, BK, base).  `stages` is the DMA
// ring depth: deeper rings hide more memory latency per workgroup but cost
// LDS, i.e. resident workgroups per CU (160 KB), so the tuner picks per layer
// (K = 64 1x1 convs want occupancy, long-K small-grid layers want depth).
// Only the direct-to-LDS operand modes (dense / im2col) build every row; the
// register-staged modes build the rows that are their own `base` (0..3, depth
// always 2) and run any other id as its `base`.
#define TFSK_IGEMM_CONFIGS(X) \
  X(0, 128, 128, 2, 2, 64, 0) \
  X(1, 128, 64, 2, 2, 64, 1) \
  X(2, 64, 128, 2, 2, 64, 2) \
  X(3, 64, 64, 2, 2, 64, 3) \
  X(4, 128, 128, 3, 2, 64, 0) \
  X(5, 64, 64, 4, 2, 64, 3) \
  X(6, 128, 64, 3, 2, 64, 1) \
  X(7, 64, 128, 3, 2, 64, 2) \
  /* wide tiles (one wave row / column): 4x the outputs per workgroup setup */ \
  X(8, 64, 256, 2, 1, 64, 2) \
  X(9, 256, 64, 2, 4, 64, 1) \
  X(10, 128, 256, 2, 2, 64, 0) \
  X(11, 256, 128, 2, 4, 64, 0) \
  /* deep k-tiles: 2-4x the MFMA work per barrier / DMA round trip */ \
  X(12, 64, 64, 2, 2, 128, 3) \
  X(13, 64, 64, 2, 2, 256, 3) \
  X(14, 64, 128, 2, 2, 128, 2) \
  X(15, 128, 64, 2, 2, 128, 1) \
  X(16, 128, 128, 2, 2, 128, 0)

// cgemm.hip (16x16x32 MFMA): X(id, BM, BN, WGM, WGN, S) -- tile, wave grid,
// ring depth.  LDS per workgroup = S * (BM + BN) * 128 B (or the fp32 epilogue
// tile if larger).
#define TFSK_CGEMM_CONFIGS(X) \
  X(32, 128, 128, 2, 2, 3)   /* 96 KB, wave 64x64 */ \
  X(33, 128, 128, 2, 2, 2)   /* 64 KB (2 WG/CU) */ \
  X(34, 64, 128, 2, 2, 4)    /* 96 KB, wave 32x64 */ \
  X(35, 128, 64, 2, 2, 4)    /* 96 KB, wave 64x32 */ \
  X(36, 64, 64, 2, 2, 4)     /* 64 KB, wave 32x32 */ \
  X(37, 256, 128, 4, 2, 3)   /* 144 KB, 8 waves of 64x64 */ \
  X(38, 128, 256, 2, 4, 3)   /* 144 KB, 8 waves of 64x64 */ \
  X(39, 128, 128, 2, 4, 4)   /* 128 KB, 8 waves of 64x32 */ \
  X(40, 64, 256, 1, 4, 3)    /* 120 KB, wave 64x64 */ \
  X(41, 256, 64, 4, 1, 3)    /* 120 KB, wave 64x64 */ \
  /* double-buffered, small LDS: several workgroups per CU overlap each */ \
  /* other's prologue / barrier / epilogue latency */ \
  X(42, 64, 64, 2, 2, 2)     /* 32 KB (5 WG/CU) */ \
  X(43, 64, 128, 2, 2, 2)    /* 48 KB (3 WG/CU) */ \
  X(44, 128, 64, 2, 2, 2)    /* 48 KB (3 WG/CU) */ \
  /* 96-wide tiles: N = 768 (BERT-base hidden) is 8 of them, so an M = 4096 */ \
  /* GEMM is exactly 256 tiles of 128 x 96 -- one per CU -- where 128 x 128 */ \
  /* leaves a quarter of the CUs idle (192 tiles) and 128 x 64 needs 1.5 waves */ \
  X(45, 128, 96, 2, 2, 3)    /* 84 KB, wave 64x48 */ \
  X(46, 128, 96, 2, 2, 4)    /* 112 KB */ \
  X(47, 64, 96, 2, 2, 3)     /* 60 KB, wave 32x48 */ \
  /* two waves per workgroup: a 64x64 tile as two 64x32 wave tiles reads 24 KB */ \
  /* of LDS fragments per k-step instead of the 32 KB four 32x32 waves read */ \
  /* (whose LDS reads take as long as their MFMAs at 256 B/clk) */ \
  X(64, 64, 64, 1, 2, 2)     /* 32 KB, wave 64x32 */ \
  X(65, 64, 64, 1, 2, 3)     /* 48 KB */ \
  X(66, 64, 64, 2, 1, 3)     /* 48 KB, wave 32x64 */ \
  X(67, 128, 64, 2, 1, 2)    /* 48 KB, wave 64x64 */ \
  X(68, 64, 128, 1, 2, 2)    /* 48 KB, wave 64x64 */ \
  X(69, 128, 64, 2, 1, 3)    /* 72 KB, wave 64x64 */ \
  X(70, 64, 128, 1, 2, 3)    /* 72 KB, wave 64x64 */ \
  X(71, 64, 64, 2, 2, 3)     /* 48 KB, wave 32x32 */ \
  /* 8 waves of 64x96 (BERT's 2304 / 3072-wide projections at M = 4096: 192 / */ \
  /* 256 tiles, one per CU); 112 KB ring, epilogue in two 128-row passes */ \
  X(72, 256, 192, 4, 2, 2) \
  /* 8 waves of 32x144: BERT-base's QKV projection (4096 x 2304) is exactly */ \
  /* 256 tiles of 256 x 144, one per CU, where 256 x 192 leaves 64 CUs idle */ \
  /* (192 tiles); 150 KB, a 3-slot ring, the fp32 epilogue in one pass */ \
  X(73, 256, 144, 8, 1, 3) \
  /* 8 waves of 32x48 on the 128 x 96 tile (N = 768 at M = 4096: 256 tiles): */ \
  /* two waves per SIMD to cover the DMA latency the 4-wave 128 x 96 builds */ \
  /* (ids 45 / 46) leave exposed over K = 3072; 4- and 5-slot rings */ \
  X(74, 128, 96, 4, 2, 4)    /* 112 KB */ \
  X(75, 128, 96, 4, 2, 5)    /* 140 KB */

// cgemm.hip, fragment-prefetch (PF) builds: X(id, base_id, BM, BN, WGM, WGN, S),
// the row `base_id` above built with the PF step pipeline (checked below).
// The 8-wave 256 x 128 / 128 x 256 / 256 x 192 tiles spill with two fragment
// sets and are not built.
#define TFSK_CGEMM_PF_CONFIGS(X) \
  X(96, 32, 128, 128, 2, 2, 3) \
  X(97, 34, 64, 128, 2, 2, 4) \
  X(98, 35, 128, 64, 2, 2, 4) \
  X(99, 36, 64, 64, 2, 2, 4) \
  X(100, 39, 128, 128, 2, 4, 4) \
  X(101, 41, 256, 64, 4, 1, 3) \
  X(102, 42, 64, 64, 2, 2, 2) \
  X(103, 43, 64, 128, 2, 2, 2) \
  X(104, 44, 128, 64, 2, 2, 2) \
  X(105, 45, 128, 96, 2, 2, 3) \
  X(106, 71, 64, 64, 2, 2, 3)

// cgemm32.hip (v_mfma_f32_32x32x16_bf16, wave tiles in 32x32 blocks):
// X(id, BM, BN, WGM, WGN, S)
#define TFSK_CGEMM32_CONFIGS(X) \
  X(112, 64, 64, 2, 2, 4)     /* 64 KB, waves 32x32 */ \
  X(113, 64, 64, 1, 2, 3)     /* 48 KB, waves 64x32 */ \
  X(114, 128, 128, 2, 2, 3)   /* 96 KB, waves 64x64 */ \
  X(115, 128, 64, 2, 2, 4)    /* 96 KB, waves 64x32 */ \
  X(116, 64, 128, 2, 2, 4)    /* 96 KB, waves 32x64 */ \
  X(117, 128, 256, 2, 4, 3)   /* 144 KB, 8 waves of 64x64 */ \
  X(118, 256, 128, 4, 2, 3)   /* 144 KB, 8 waves of 64x64 */ \
  X(119, 256, 64, 4, 1, 3)    /* 120 KB, waves 64x64 */ \
  X(120, 128, 128, 2, 4, 4)   /* 128 KB, 8 waves of 64x32 */ \
  X(121, 64, 128, 2, 2, 2)    /* 48 KB (3 WG/CU) */ \
  X(122, 128, 64, 2, 2, 2)    /* 48 KB (3 WG/CU) */ \
  X(123, 256, 192, 4, 2, 2)   /* 112 KB, 8 waves of 64x96 */

// bgemm.hip (big-tile ping-pong, 8 waves of 128 x BN / 4; dense operands, no
// in-kernel split-K fixup): X(id, BM, BN)
#define TFSK_BGEMM_CONFIGS(X) \
  X(140, 256, 256) \
  X(141, 256, 128) \
  X(142, 256, 192)

// halo.hip (3x3 stride-1 conv): X(id, pf_id, BM, BN, WGM, WGN, HR, S) -- BM
// output pixels x BN channels, wave grid, halo rows, B ring depth.  `pf_id`
// is the id of the same tile built with the fragment-prefetch step pipeline,
// 0 where that build does not exist (the 8-wave 256 x 128 tile spills with
// two fragment sets: 84 is not a config).  LDS = 2 halo buffers (HR x 128 B;
// one when C == 64) + S B slots (BN x 128 B).
#define TFSK_HALO_CONFIGS(X) \
  X(48, 80, 256, 64, 4, 1, 320, 3)    /* 104 KB (64 KB for C == 64), waves 64x64 */ \
  X(49, 81, 128, 128, 2, 2, 192, 3)   /* 96 KB, waves 64x64 */ \
  X(50, 82, 128, 64, 2, 2, 192, 3)    /* 72 KB (48 KB), waves 64x32 */ \
  X(51, 83, 64, 64, 2, 2, 128, 3)     /* 56 KB (40 KB), waves 32x32 */ \
  X(52, 0, 256, 128, 4, 2, 320, 3)    /* 135 KB, 8 waves of 64x64 */ \
  X(53, 85, 64, 128, 2, 2, 128, 3)    /* 80 KB, waves 32x64 */ \
  /* 9-slot rings: 8 weight tiles in flight (16 x 1-KB DMAs per wave) */ \
  X(54, 86, 64, 64, 2, 2, 128, 9)     /* 104 KB, waves 32x32 */ \
  X(55, 87, 128, 64, 2, 2, 192, 9)    /* 120 KB, waves 64x32 */ \
  X(56, 88, 256, 64, 4, 1, 320, 9)    /* 152 KB, waves 64x64 */ \
  /* 8 waves of 32x32 on the 128 x 64 tile: two waves per SIMD where the */ \
  /* 4-wave build waits 40 % of its cycles (the stage-2 / 3 3x3 convs, */ \
  /* profiles/round4/s5/pmc_r50_b32_mfma.txt) */ \
  X(57, 89, 128, 64, 4, 2, 192, 3)    /* 72 KB */ \
  X(58, 90, 128, 64, 4, 2, 192, 9)    /* 120 KB */

// halo.hip halo_persist_kernel: X(id, BM, BN, HR) -- 128 pixels x 64 channels,
// C == 64 only, the whole filter resident in LDS, plain bf16 output, no split-K
#define TFSK_HALO_PERSIST_CONFIGS(X) \
  X(146, 128, 64, 192)

enum class TileFamily : int { kIGemm, kCGemm, kCGemmPf, kCGemm32, kBGemm, kHalo, kHaloPf, kHaloPersist };

struct TileConfig {
  int id;
  TileFamily family;
  int bm, bn;
  int hr;     // halo rows (halo families; 0 elsewhere)
  int base;   // the row this one is a variant of (igemm `base`, PF builds); itself otherwise
};

constexpr int kTileIdEnd = 147;   // every id is below this

struct TileTable {
  TileConfig rows[128];
  int n, n_igemm;
  short at[kTileIdEnd];   // id -> index into rows, -1: not a config
  bool ok;                // the lists are consistent (checked below)
};

constexpr TileTable make_tile_table() {
  TileTable t{};
  for (int i = 0; i < kTileIdEnd; ++i) t.at[i] = -1;
  t.ok = true;
  auto add = [&t](int id, TileFamily f, int bm, int bn, int hr, int base) {
    if (id < 0 || id >= kTileIdEnd || t.at[id] >= 0 || t.n >= 128) {
      t.ok = false;
      return;
    }
    t.at[id] = short(t.n);
    t.rows[t.n++] = TileConfig{id, f, bm, bn, hr, base};
  };
#define TFSK_ROW_IGEMM(id, bm, bn, st, wm, bk, base) add(id, TileFamily::kIGemm, bm, bn, 0, base);
#define TFSK_ROW_CGEMM(id, bm, bn, wgm, wgn, s) add(id, TileFamily::kCGemm, bm, bn, 0, id);
#define TFSK_ROW_CGEMM_PF(id, base, bm, bn, wgm, wgn, s) add(id, TileFamily::kCGemmPf, bm, bn, 0, base);
#define TFSK_ROW_CGEMM32(id, bm, bn, wgm, wgn, s) add(id, TileFamily::kCGemm32, bm, bn, 0, id);
#define TFSK_ROW_BGEMM(id, bm, bn) add(id, TileFamily::kBGemm, bm, bn, 0, id);
#define TFSK_ROW_HALO(id, pf, bm, bn, wgm, wgn, hr, s) add(id, TileFamily::kHalo, bm, bn, hr, id);
#define TFSK_ROW_HALO_PF(id, pf, bm, bn, wgm, wgn, hr, s) \
  if (pf != 0) add(pf, TileFamily::kHaloPf, bm, bn, hr, id);
#define TFSK_ROW_HALO_PERSIST(id, bm, bn, hr) add(id, TileFamily::kHaloPersist, bm, bn, hr, id);
  // the order of the rows is the order cgemm_configs() / halo_configs() list them in
  TFSK_IGEMM_CONFIGS(TFSK_ROW_IGEMM)
  TFSK_CGEMM_CONFIGS(TFSK_ROW_CGEMM)
  TFSK_CGEMM_PF_CONFIGS(TFSK_ROW_CGEMM_PF)
  TFSK_CGEMM32_CONFIGS(TFSK_ROW_CGEMM32)
  TFSK_BGEMM_CONFIGS(TFSK_ROW_BGEMM)
  TFSK_HALO_CONFIGS(TFSK_ROW_HALO)
  TFSK_HALO_CONFIGS(TFSK_ROW_HALO_PF)
  TFSK_HALO_PERSIST_CONFIGS(TFSK_ROW_HALO_PERSIST)
#undef TFSK_ROW_IGEMM
#undef TFSK_ROW_CGEMM
#undef TFSK_ROW_CGEMM_PF
#undef TFSK_ROW_CGEMM32
#undef TFSK_ROW_BGEMM
#undef TFSK_ROW_HALO
#undef TFSK_ROW_HALO_PF
#undef TFSK_ROW_HALO_PERSIST
  // every `base` names a row that is its own base; a PF row has its base's
  // tile; the igemm ids are 0 .. n_igemm - 1
  for (int i = 0; i < t.n; ++i) {
    const TileConfig& r = t.rows[i];
    if (r.base < 0 || r.base >= kTileIdEnd || t.at[r.base] < 0) {
      t.ok = false;
      continue;
    }
    const TileConfig& b = t.rows[t.at[r.base]];
    if (b.base != b.id) t.ok = false;
    if (r.family == TileFamily::kIGemm) {
      if (b.family != TileFamily::kIGemm || r.id != t.n_igemm++) t.ok = false;
    } else if (b.bm != r.bm || b.bn != r.bn || b.hr != r.hr) {
      t.ok = false;
    }
  }
  return t;
}

inline constexpr TileTable kTileTable = make_tile_table();
static_assert(kTileTable.ok,
              "tile_configs.h: an id is listed twice or is not below kTileIdEnd, a PF row differs from its base "
              "row's tile, a base is not a base row, or the igemm ids are not 0 .. n - 1");
constexpr int kNumIGemmConfigs = kTileTable.n_igemm;

// The row of config `id`, nullptr for anything that is not one.
constexpr const TileConfig* tile_config(int id) {
  return id >= 0 && id < kTileIdEnd && kTileTable.at[id] >= 0 ? &kTileTable.rows[kTileTable.at[id]] : nullptr;
}

constexpr bool cgemm_family(TileFamily f) {
  return f == TileFamily::kCGemm || f == TileFamily::kCGemmPf || f == TileFamily::kCGemm32 ||
         f == TileFamily::kBGemm;
}
constexpr bool halo_family(TileFamily f) {
  return f == TileFamily::kHalo || f == TileFamily::kHaloPf || f == TileFamily::kHaloPersist;
}

}  // namespace tfsk

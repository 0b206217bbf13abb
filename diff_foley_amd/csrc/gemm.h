// Implicit-GEMM descriptor shared by host launcher and device kernels.
//
//   C[m, n] = epilogue( alpha * sum_k A(m, k) * W[n, k] )
//
// A is a bf16 NHWC activation tensor [rows][lda]; for taps == 9 the k index runs over
// (ky, kx, cin) of a 3x3 window (zero padding 1, stride 1|2, optional nearest x2 upsample of
// the input), i.e. the convolution is evaluated as a GEMM without materialising im2col.
// W is bf16 [N][K] (K contiguous) -- PyTorch Linear layout, conv weights re-packed to
// [Cout][ky][kx][Cin] at load time.  Accumulation is fp32 on the MFMA units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

// Launch constants (gemm_launch_consts, gemm.hip): everything a block's prologue would otherwise derive from GemmParams by dividing by
// constants of the launch -- tile counts, the tile walk, the K range of a split, the halo geometry -- and, for every divisor the
// device still applies, what turns the division into a multiplication.  Computed on the host once per launch, read-only on the
// device: a prologue holds no division, integer or float (tools/check_prologue.py).  Two forms:
//   GemmMagic   x / d == umulhi(x, mul) >> sh for 0 <= x < 2^31 (d == 1: x).  Block-uniform quotients -- the tile walk, the weight
//               matrix of a tile, the first tap of a split -- stay on the scalar unit with it (a float reciprocal would take them,
//               and every address computed from them, through vector registers), and conv rows may pass 2^22.
//   reciprocals the IEEE 1.0f / (float)d of FastDiv (gemm_impl.h), exact for 0 <= x < 2^22: the halo kernels' per-thread quotients.
struct GemmMagic { unsigned mul; int sh; int d; };
struct GemmLaunch {
  // tile walk: blockIdx.x -> logical tile id (XCD remap: xq = nblk / 8, xr = nblk % 8) -> (M tile, N tile)
  int nbm, nbn, nblk, xq, xr;
  int gm;                      // M tiles per row group, normalised to 1 .. nbm (GemmParams::gm <= 0 or >= nbm: one group)
  GemmMagic per, rows, last;   // by gm * nbn (logical tiles of a full row group), by gm, by the M tiles of the last (short) row group
  // K range of a split: split z runs K steps (halo tiles: 64-channel slices) [z * kper, min(nk, (z + 1) * kper))
  int nk, kper;
  // halo tiles' folded skip: its n2tot slices are dealt, per2 each, to the `used` splits that own conv slices (no split-K: used = 1)
  int n2tot, used, per2;
  GemmMagic wrb;               // per-sample weights: by the M tiles per weight matrix (w_rows / BM); d = 0: off
  GemmMagic ohw, ow, cin;      // MODE 1 .. 3: row -> (sample, y, x) by OH OW and OW, first K index of a split -> tap by Cin
  // halo tiles: (TH + 2)(TW + 2), TH TW, patches per block, halo rows, DMA passes of a halo, patches per image row / column / image
  // and in all
  int HWp, PPX, PB, HR, APASS, npx, npy, pimg, npatch;
  float inv_hwp, inv_tw2, inv_pimg, inv_npx, inv_ppx, inv_tw;
};

struct GemmParams {
  // operands
  const uint16_t* A; long a_bs; int lda;
  const uint16_t* W; long w_bs;
  unsigned a_bytes, w_bytes;   // bytes addressable from A / W of ONE batch slice (buffer-load bounds, < 2 GiB)
  int M, N, K;
  GemmLaunch lc;               // set by launch_gemm from the route; beside the operands, which the first requests need with it
  // implicit-conv geometry
  // ResBlock skip connection folded into conv2 (openai_unetmodel.py:234-241, 275: skip(x) + h): a TENTH K range of
  // Cin2 channels read from a second operand tensor at the centre pixel, K = 9*Cin + Cin2, W rows = [conv taps | skip]
  const uint16_t* A2; int lda2; unsigned a2_bytes; int Cin2;
  int taps;    // 1 (linear / 1x1) or 9 (3x3, pad 1)
  int Cin;     // channels per tap, K = taps * Cin, Cin % 64 == 0
  int H, Wd;   // stored input spatial size
  int OH, OW;  // output spatial size (M = batch * OH * OW)
  int stride;  // 1 | 2
  int pad;     // taps == 9, MODE 2 (stride 2 / upsampled input): zero padding in front of row 0 / column 0 -- 1 = the symmetric conv, 0 = the VAE
               // encoder's Downsample (F.pad(x, (0,1,0,1)) + a padding-0 conv: only the bottom row and the right column read zeros)
  int ups;     // 1: conv runs on the nearest-x2 upsampled input
  int zstuff;  // with ups=1: the x2 input is ZERO-stuffed (transposed stride-2 conv, backward of Downsample), not nearest
  int th, tw;  // halo kernels: spatial patch of output pixels owned per block (th*tw divides BM)
  int halo_ring_bytes;   // halo kernels (set by the launcher): LDS bytes of the operand ring; the epilogue row table follows
  // epilogue
  void* C; long c_bs; int ldc; int out_bf16;
  float alpha;
  const float* bias;                 // [N]
  const float* rowbias; int ld_rowbias; int rows_per_sample; int rowbias_mode;  // 1: by sample, 2: by position
  const float* res; long res_bs; int ldr;   // fp32 residual, may alias C
  int relu;                          // max(v, 0) after bias / residual (CAVP encoder ConvModule activation)
  int silu;                          // v * sigmoid(v) after bias (time-embedding MLP layers); LEAN / ANY epilogues
  uint16_t* aux; int ld_aux;         // optional second output: operand-type copy of the stored value, [row][ld_aux]
  int geglu;                         // columns come in (x:32 | gate:32) groups, output width N/2
  // LayerNorm folded into this GEMM (A = raw operand copy of x, W = gamma-scaled weights):
  //   out[m][n] = rstd[m] * (acc[m][n] - mean[m] * ln_cs[n]) + bias[n]      (bias already holds beta.W + b)
  // mean / rstd of row m come from the producer's per-row partials ln_stats[m][0..ln_slots) = (sum, sum of squares)
  // over 64-column slots of the fp32 tensor the operand copy was made from (ln_C columns in total).
  const float2* ln_stats; int ln_slots; int ln_C; float ln_eps;
  const float* ln_cs;                // [N] column sums of the (operand-rounded) gamma-scaled weights
  // The same GEGLU projection in the 320-column packing of the wide tiles (ffn_wide.hip, round 6): weight rows, column sums and
  // folded bias permuted so that every 160-row half of a 320-row tile is [80 x rows | their 80 gate rows].  null = not packed.
  const uint16_t* W_w320; const float* cs_w320; const float* bias_w320;
  // Row-block weights: rows [i*w_rows, (i+1)*w_rows) multiply W + i*w_bs (one weight matrix per SAMPLE in one launch: the
  // cross-attention GEMMs whose "weights" are precomputed from each sample's context).  w_rows % BM == 0.
  int w_rows;
  // Cross-attention score epilogue (with ln_stats): ln_cs and bias are per sample, [M / w_rows][N]; every group of sm_w = 32
  // columns (one head) gets a softmax over its first sm_valid columns (the rest is padding and stores 0); operand-type output.
  int sm_w, sm_valid;
  // per-row partial statistics of the STORED fp32 value (after bias / residual): stats[row][col/64] = (sum, sumsq)
  float2* stats; int stats_slots;
  // columns >= vt_col0 are stored TRANSPOSED per sample into vt[(row/vt_T)*(N-vt_col0) + col-vt_col0][ldvt] at
  // position row%vt_T (attention V^T straight out of the fused QKV projection); vt_col0 % BN == 0 for every tile used
  uint16_t* vt; int vt_col0; int vt_T; int ldvt;
  // Classifier-free-guidance prefix: the two halves of the CFG batch are identical until the first cross-attention, so the
  // ops in front of it run on ONE half (M rows) and the op that feeds the full batch stores every output row twice, at
  // row and row + dup_rows (C / aux / stats alike).  0 = off.  Plain row-major epilogues only (LEAN / PROD / ANY, reduce).
  int dup_rows;
  int no_c_store;   // PROD epilogue: skip the fp32 store of C (nobody reads it); operand copy + row statistics only
  int store_nchw; int hw_out;        // write C as [batch][N][hw_out] instead of [rows][ldc]
  int gm;      // tile walk: each XCD's contiguous tile range runs M-fastest inside row groups of `gm` M-tiles (0 = all rows:
               // plain M-fastest; 1 = N-fastest).  Decides which operand panels an XCD's L2 can share; autotuned in situ.
  int dbg;     // tools only: 1 = every K tile re-reads tile 0 (cache-resident operands; isolates memory latency)
  // split-K
  int splitk; float* partial;
  int defer_reduce;   // split-K only: write the partial slabs and do NOT launch the reduce -- the consumer (GroupNorm) sums them
  // split-K + NCHW store of a CFG batch [uncond ; cond] (UNetModel.out): the reduce launch also forms e_u + cfg_scale (e_c - e_u)
  // and writes THAT, [M / 2 rows][N] as NCHW, to cfg_out (ddim.py:241-245); C is not written.  null = off.
  float* cfg_out; float cfg_scale;
};

#if defined(__HIP_DEVICE_COMPILE__)
// kernel-argument / own-code touch of the GEMM kernels: common.h df_entry_touch
__device__ __forceinline__ DfTouch gemm_kernarg_touch() { return df_entry_touch((int)sizeof(GemmParams)); }
__device__ __forceinline__ void gemm_kernarg_touch_end(const DfTouch& v) { df_entry_touch_end(v); }
#endif

// The tiles: gemm_tiles.def has one row per tile id; the enum and every look-up below are generated from it.
enum GemmTileFamily { DF_FAM_GEN = 0, DF_FAM_HALO = 1, DF_FAM_PS = 2, DF_FAM_PGEGLU = 3, DF_FAM_WGEGLU = 4, DF_FAM_RETIRED = 5 };
enum GemmTile {
#define DF_TILE(ID, NAME, ...) NAME,
#include "gemm_tiles.def"
#undef DF_TILE
  TILE_ALL
};
struct GemmTileInfo {
  const char* name;      // display name (tools)
  int family, part;      // GemmTileFamily; which of the family's two translation units holds it
  int modes;             // bit m: instantiated for MODE m
  int bm, bn, wgm, wgn, ring, ps, lns;
};
inline constexpr GemmTileInfo kGemmTiles[TILE_ALL] = {
#define DF_TILE(ID, NAME, DISP, FAM, PART, M0, M1, M2, M3, BM, BN, WGM, WGN, RING, PS, LNS) \
  {DISP, DF_FAM_##FAM, PART, (M0) | (M1) << 1 | (M2) << 2 | (M3) << 3, BM, BN, WGM, WGN, RING, PS, LNS},
#include "gemm_tiles.def"
#undef DF_TILE
};
#define DF_TILE(ID, NAME, ...) static_assert(NAME == ID, "gemm_tiles.def: a tile id is its row's position (the ids are a file format)");
#include "gemm_tiles.def"
#undef DF_TILE

// Any int may be asked about; an id outside the table is of no family and no MODE.
static inline int gemm_tile_family(int cfg) { return (cfg >= 0 && cfg < TILE_ALL) ? kGemmTiles[cfg].family : -1; }
static inline bool gemm_tile_is_halo(int cfg) { return gemm_tile_family(cfg) == DF_FAM_HALO; }
static inline bool gemm_tile_is_ps(int cfg) { return gemm_tile_family(cfg) == DF_FAM_PS; }
static inline bool gemm_tile_is_pgeglu(int cfg) { return gemm_tile_family(cfg) == DF_FAM_PGEGLU; }
static inline bool gemm_tile_is_wgeglu(int cfg) { return gemm_tile_family(cfg) == DF_FAM_WGEGLU; }
static inline bool gemm_tile_has_mode(int cfg, int mode) { return cfg >= 0 && cfg < TILE_ALL && ((kGemmTiles[cfg].modes >> mode) & 1); }
// MODE 0: linear / 1x1;  1: 3x3 stride 1 (tap offsets are linear, 2 VALU per request);  2: 3x3 stride 2 / upsampled;
// 3: phase-decomposed upsample conv (taps == 4)
static inline int gemm_mode(const GemmParams& p) { return (p.taps == 4) ? 3 : (p.taps != 9) ? 0 : ((p.stride == 1 && !p.ups) ? 1 : 2); }
// 64-column slots of row statistics a LayerNorm-folded GEMM can fold per row (gemm_impl.h LNS): C <= 1280
static inline int gemm_ln_max_slots() { return 20; }

// The look-ups below take an id of the table.
// threads of a halo tile that issue its DMA requests (the LDS staging geometry follows from them: 8 threads per 128-B row)
static inline int gemm_halo_dma_threads(int cfg) {
  const GemmTileInfo& t = kGemmTiles[cfg];
  return 64 * t.wgm * t.wgn * (t.ps ? t.ps : 1);
}
static inline int gemm_halo_ring(int cfg) { return kGemmTiles[cfg].ring; }     // weight ring depth
static inline void gemm_tile_dims(int cfg, int* bm, int* bn) {
  *bm = kGemmTiles[cfg].bm;
  *bn = kGemmTiles[cfg].bn;
}

// Epilogue specialisations.  A kernel carries ONLY the epilogue it runs: the per-launch fixed cost on this chip grows by
// ~1-2 us between a 5 KB and a 45 KB code object (cold instruction fetch at every kernel boundary; tools/icache_probe.py),
// which is 10-20 % of the small GEMMs of the transformer blocks.
//   LEAN   fp32 | operand-type row-major out, bias, per-sample / per-position bias, residual   (the UNet's common case)
//   SPLITK partial slab store (the reduce kernel applies the epilogue)
//   GEGLU  value * gelu(gate) on (32 | 32) column groups, optionally LayerNorm-folded
//   PROD   LEAN + per-row partial statistics + operand-type copy (producers of a LayerNorm-folded consumer)
//   LNC    LayerNorm-folded consumer, optionally with the transposed V^T column range (fused QKV)
//   ANY    everything else: alpha, ReLU, aux copy, NCHW store, unaligned shapes (scalar fallback)
//   XS     cross-attention scores: LayerNorm-folded, softmax over each 32-column head, operand-type out
enum { EPI_LEAN = 0, EPI_SPLITK = 1, EPI_GEGLU = 2, EPI_PROD = 3, EPI_LNC = 4, EPI_ANY = 5, EPI_XS = 6 };

// The vectorised epilogues (in-kernel and split-K reduce alike) move 4 consecutive columns of C, the residual, the row bias and the
// operand copy as one 16-byte (8-byte) access: row-major output, every row stride a multiple of 4 elements.
static inline bool gemm_rows_vec4(const GemmParams& p) {
  return !p.store_nchw && (p.ldc & 3) == 0 && (p.ldr & 3) == 0 && (p.ld_rowbias & 3) == 0 && (p.ld_aux & 3) == 0;
}
// Only the in-kernel epilogues run batched: they step C and the residual by blockIdx.z * c_bs / res_bs, so those strides have to keep
// the alignment too.  The reduce kernels never see a batch (split-K and batch exclude each other) and do not ask this.
static inline bool gemm_batch_vec4(const GemmParams& p) { return (p.res_bs & 3) == 0 && (p.c_bs & 3) == 0; }

// How one (problem, tile, batch, split-K) is launched: gemm_route decides, launch_gemm only dispatches on it.
enum GemmReduce { DF_RED_NONE = 0, DF_RED_VEC, DF_RED_SCALAR, DF_RED_CFG, DF_RED_DEFERRED };      // who sums split-K slabs (MODE 3: of the x2 map)
struct GemmRoute {
  int family, mode, epi, zdim, reduce;         // GemmTileFamily, MODE 0 .. 3, EPI_*, grid z (split-K or batch), GemmReduce
  int th, tw, halo_ring_bytes;                 // halo tiles: the block's patch of output pixels, bytes of its LDS operand ring
  size_t lds;                                  // halo tiles: dynamic LDS of the launch
};
// The launch constants of a problem the route admits (r = what gemm_route said for the same p, tile, splitk): the ONE place that
// derives them; the kernels are their only reader.  Pure host arithmetic.
void gemm_launch_consts(const GemmParams& p, int tile, int splitk, const GemmRoute& r, GemmLaunch* out);
GemmMagic gemm_magic(int d);
// nullptr: the tile can run this problem at this batch and split-K, *out (may be null) says how; else the rule that refuses.
// Every correctness rule of the GEMM stack is here, once; pure host arithmetic, no HIP call.
const char* gemm_route(const GemmParams& p, int tile, int batch, int splitk, GemmRoute* out);
// POLICY, not correctness: the splits of a K loop the tuner bothers to time (every slab keeps at least two K steps; halo tiles: one
// 64-channel chunk).  A finer split runs and is right, it is just never the fastest.
bool gemm_split_worth_tuning(const GemmParams& p, int tile, int splitk);
// What the plan builder and the tuner ask: gemm_route says yes, and the split is inside the tuner's policy.
bool gemm_tile_valid(const GemmParams& p, int tile, int batch, int splitk);

// Calls gemm_route with p.splitk first: a refusal is hipErrorInvalidValue, *why (when given) the rule; nothing is launched.
hipError_t launch_gemm(const GemmParams& p, int tile_cfg, int batch, hipStream_t stream, const char** why = nullptr);
// (32 x | 32 gate) GEGLU packing (rows of K operand values, column sums, folded bias) -> the wide tiles' 320-column packing (ffn_wide.hip)
hipError_t launch_pack_w320(const uint16_t* w, const float* cs, const float* bb, uint16_t* wo, float* cso, float* bbo, int N, int K, hipStream_t s);

// MFMA bf16 implicit-GEMM for gfx950: conv3x3 / conv1x1 / Linear / batched matmul with fused epilogues.
//
// Block = 256 threads = 4 wavefronts (64 lanes) in a WGM x WGN grid; each wavefront owns a
// (BM/WGM) x (BN/WGN) output tile made of 32x32 MFMA tiles (v_mfma_f32_32x32x16_bf16).
// K is walked in steps of 64.  Operand tiles go HBM -> LDS directly (buffer_load_dwordx4 ... lds, no VGPR
// round trip) into an NST-deep LDS ring: tile kt+NST-1 is requested while tile kt is multiplied, so the
// ~1 us load latency of this chip is covered even for the tiny-K GEMMs of the transformer blocks.  One raw
// s_barrier per K step; waits are counted (s_waitcnt vmcnt(N)), never a full drain inside the loop.
// LDS rows are 128 B (64 bf16); the 16-B chunk index is XOR-swizzled with (row>>1)&7 so the ds_read_b128
// fragment reads of a 16-lane group hit 16 distinct slots.  The DMA writes LDS linearly (wave base +
// lane*16), so the swizzle is applied to the per-lane SOURCE chunk instead (rule: both sides or neither).
// Out-of-range rows / conv padding use an out-of-bounds buffer offset: the hardware then writes zeros.
#include <algorithm>
#include <numeric>
#include <stdlib.h>

#include "gemm_impl.h"


hipError_t launch_gemm_m0a(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream);
hipError_t launch_gemm_m0b(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream);
hipError_t launch_gemm_m1(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream);
hipError_t launch_gemm_m2(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream);
hipError_t launch_gemm_halo(int tile_cfg, int epi, const GemmParams& p, int zdim, size_t lds, hipStream_t stream);
hipError_t launch_gemm_m3(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream);
hipError_t launch_gemm_ps(int mode, int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream);
hipError_t launch_gemm_ps_small(int mode, int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream);
hipError_t launch_gemm_pgeglu(int tile_cfg, const GemmParams& p, hipStream_t stream);
hipError_t launch_gemm_wgeglu(int tile_cfg, const GemmParams& p, hipStream_t stream);

namespace {

// Sums the split-K partial slabs and applies the same epilogue.  One thread per output element (scalar fallback:
// GEGLU, NCHW stores, unaligned leading dimensions).
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmParams p) {
  const int nout = p.geglu ? (p.N >> 1) : p.N;
  const long total = (long)p.M * nout;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / nout), oc = (int)(e - (long)row * nout);
    if (p.geglu) {
      const int xcol = (oc >> 5) * 64 + (oc & 31);
      float xs = 0.f, gs = 0.f;
      for (int s = 0; s < p.splitk; ++s) {
        const float* part = p.partial + ((long)s * p.M + row) * p.N;
        xs += part[xcol];
        gs += part[xcol + 32];
      }
      epi_out(p, 0, row, oc, epi_bias(p, row, xcol, xs) * gelu_erf(epi_bias(p, row, xcol + 32, gs)));
    } else {
      float v = 0.f;
      for (int s = 0; s < p.splitk; ++s) v += p.partial[((long)s * p.M + row) * p.N + oc];
      epi_out(p, 0, row, oc, epi_bias(p, row, oc, v));
    }
  }
}

// Split-K reduce of UNetModel.out on a classifier-free-guidance batch (round 5): rows [0, M/2) are the unconditional half, rows
// [M/2, M) the conditional one; both are reduced in slab order, get alpha / bias like the scalar reduce above, and the guided
// eps  e_u + scale (e_c - e_u)  leaves as NCHW -- the arithmetic of splitk_reduce_kernel followed by cfg_combine_kernel, bit for bit,
// in one launch instead of two.
__global__ __launch_bounds__(256) void splitk_reduce_cfg_kernel(GemmParams p) {
  const int half = p.M >> 1;
  const long total = (long)half * p.N;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / p.N), oc = (int)(e - (long)row * p.N);
    float vu = 0.f, vc = 0.f;
    for (int s = 0; s < p.splitk; ++s) {
      vu += p.partial[((long)s * p.M + row) * p.N + oc];
      vc += p.partial[((long)s * p.M + row + half) * p.N + oc];
    }
    const float u = epi_bias(p, row, oc, vu), c = epi_bias(p, row + half, oc, vc);
    const int b = row / p.hw_out, px = row - b * p.hw_out;
    p.cfg_out[((long)b * p.N + oc) * p.hw_out + px] = u + p.cfg_scale * (c - u);
  }
}

// Vectorised reduce: one thread per 4 consecutive output columns; the SK slab loads of a thread are independent and
// issued together (compile-time split count), then alpha / bias / FiLM bias / residual / ReLU and one 16-B (fp32) or
// 8-B (operand type) store.  Summation order s = 0..SK-1 is fixed, so results are deterministic.
template <int SK>
__global__ __launch_bounds__(256) void splitk_reduce_vec_kernel(GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const DfTouch ka = gemm_kernarg_touch();      // kernel-argument lines (and the code behind the pc) into L2 beside the first scalar loads
#endif
  const int n4 = p.N >> 2;
  const long total = (long)p.M * n4;
  const long slab = (long)p.M * p.N;
  const bool has_bias = p.bias != nullptr, has_rb = p.rowbias != nullptr, has_res = p.res != nullptr;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / n4), col = (int)(e - (long)row * n4) * 4;
    const float* src = p.partial + (long)row * p.N + col;
    float4 t[SK];
#pragma unroll
    for (int s = 0; s < SK; ++s) t[s] = *reinterpret_cast<const float4*>(src + s * slab);
    float4 v = t[0];
#pragma unroll
    for (int s = 1; s < SK; ++s) {
      v.x += t[s].x; v.y += t[s].y; v.z += t[s].z; v.w += t[s].w;
    }
    v.x *= p.alpha; v.y *= p.alpha; v.z *= p.alpha; v.w *= p.alpha;
    if (p.ln_stats) {        // LayerNorm folded into the GEMM: row statistics from the producer's per-slot partials
      const float2* sp = p.ln_stats + (long)row * p.ln_slots;
      float s1 = 0.f, s2 = 0.f;
      for (int i = 0; i < p.ln_slots; ++i) {
        const float2 t2 = sp[i];
        s1 += t2.x;
        s2 += t2.y;
      }
      const float inv = 1.0f / (float)p.ln_C;
      const float mean = s1 * inv, rstd = rsqrtf(fmaxf(s2 * inv - mean * mean, 0.f) + p.ln_eps);
      const float4 cs = *reinterpret_cast<const float4*>(&p.ln_cs[col]);
      v.x = rstd * (v.x - mean * cs.x); v.y = rstd * (v.y - mean * cs.y);
      v.z = rstd * (v.z - mean * cs.z); v.w = rstd * (v.w - mean * cs.w);
    }
    if (has_bias) {
      const float4 b = *reinterpret_cast<const float4*>(&p.bias[col]);
      v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    }
    if (has_rb) {
      const int ri = (p.rowbias_mode == 1) ? (row / p.rows_per_sample) : (row % p.rows_per_sample);
      const float4 b = *reinterpret_cast<const float4*>(&p.rowbias[(long)ri * p.ld_rowbias + col]);
      v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    }
    if (has_res) {
      const float4 b = *reinterpret_cast<const float4*>(&p.res[(long)row * p.ldr + col]);
      v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    }
    if (p.silu && !p.ln_stats && !p.stats) {      // same rule as the in-kernel epilogue (gemm_impl.h DF_EPI_LOOP)
      v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w);
    }
    if (p.relu) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    if (p.stats) {           // N % 64 == 0: 16 consecutive threads hold one 64-column slot of one row
      const float s1 = row16_sum((v.x + v.y) + (v.z + v.w));
      const float s2 = row16_sum((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
      if ((threadIdx.x & 15) == 0) {
        p.stats[(long)row * p.stats_slots + (col >> 6)] = make_float2(s1, s2);
        if (p.dup_rows) p.stats[(long)(row + p.dup_rows) * p.stats_slots + (col >> 6)] = make_float2(s1, s2);
      }
    }
    for (int rep = 0; rep < (p.dup_rows ? 2 : 1); ++rep) {      // CFG prefix: every row is stored for both halves of the batch
      const long orow = row + (rep ? p.dup_rows : 0);
      const long idx = orow * p.ldc + col;
      if (p.no_c_store) {       // producer whose fp32 value nobody reads (operand copy + statistics only)
      } else if (p.out_bf16)
        st_wt(reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(p.C) + idx), make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)));
      else
        st_wt(reinterpret_cast<float4*>(reinterpret_cast<float*>(p.C) + idx), v);
      if (p.aux) st_wt(reinterpret_cast<uint2*>(p.aux + orow * p.ld_aux + col), make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)));
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  gemm_kernarg_touch_end(ka);
#endif
}

// split counts the vectorised reduce is built for (the tuner's list); any other count takes the scalar reduce
#define DF_REDUCE_SPLITS(X) X(2) X(3) X(4) X(6) X(8) X(12) X(16) X(24) X(32)
bool reduce_vec_built(int sk) {
#define DF_RED(SK) case SK:
  switch (sk) {
    DF_REDUCE_SPLITS(DF_RED) return true;
    default: return false;
  }
#undef DF_RED
}

// q: the GEMM's parameters (MODE 3: with the x2 map's row count, as one-tap rows)
hipError_t launch_splitk_reduce(const GemmParams& q, int reduce, hipStream_t stream) {
  const bool vec = reduce == DF_RED_VEC, cfg = reduce == DF_RED_CFG;
  const long total = vec ? (long)q.M * (q.N >> 2) : cfg ? (long)(q.M >> 1) * q.N : (long)q.M * (q.geglu ? q.N >> 1 : q.N);     // threads
  const int blocks = (int)std::min<long>((total + 255) / 256, vec ? 4096 : 2048);
#define DF_RED(SK) case SK: hipLaunchKernelGGL(splitk_reduce_vec_kernel<SK>, dim3(blocks), dim3(256), 0, stream, q); break;
  if (vec) switch (q.splitk) { DF_REDUCE_SPLITS(DF_RED) }
  else if (cfg) hipLaunchKernelGGL(splitk_reduce_cfg_kernel, dim3(blocks), dim3(256), 0, stream, q);
  else hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, q);
#undef DF_RED
  return hipGetLastError();
}

// Spatial patch (th x tw output pixels) owned by one block of a halo kernel with BM rows.
bool halo_patch(int H, int W, int BM, int* th, int* tw) {
  const int w = (W % 16 == 0) ? 16 : W;
  if (w <= 0 || H <= 0 || BM % w != 0) return false;
  *th = std::gcd(H, BM / w);     // tallest patch that tiles both the image and the block (192 rows: 3 x 4x16)
  *tw = w;
  return true;
}

// The persistent and the wide GEGLU projection (ffn.hip, ffn_wide.hip): one LayerNorm-folded form each, nothing else.
const char* route_fused_geglu(const GemmParams& p, const GemmTileInfo& t, int batch, int sk) {
  if (!p.geglu || !p.ln_stats) return "the fused GEGLU tiles run the LayerNorm-folded GEGLU projection only";
  if (sk > 1 || batch > 1) return "the fused GEGLU tiles take neither split-K nor a batch";
  if (!p.out_bf16 || !p.C || p.res || p.rowbias || p.aux || p.stats || p.vt || p.w_rows != 0 || p.Cin2 != 0 || p.dup_rows != 0 ||
      p.sm_w != 0 || p.relu || p.silu || p.store_nchw || p.alpha != 1.f)
    return "the fused GEGLU tiles store operand-type value * gelu(gate) and know no other epilogue feature";
  if ((p.K % 64) != 0 || p.K < 128) return "the fused GEGLU tiles need K >= 128 in whole 64-element steps";
  if (p.ln_slots > gemm_ln_max_slots()) return "more than 20 LayerNorm statistics slots";
  if (t.family == DF_FAM_PGEGLU) {
    if (!p.ln_cs || !p.bias) return "the persistent GEGLU kernel needs column sums and the folded bias";
    if ((p.N % 128) != 0) return "the persistent GEGLU kernel needs N % 128 == 0";
    if (p.ln_slots > t.lns) return "more LayerNorm statistics slots than this tile's registers hold (LNS)";
    if ((long)p.M * p.ldc * 2 >= ((long)1 << 31)) return "the persistent GEGLU kernel's output exceeds 2 GiB of buffer addressing";
  } else {
    if (!p.W_w320 || !p.cs_w320 || !p.bias_w320) return "the wide GEGLU tiles need the 320-column packing";
    if ((p.N % 320) != 0 || (p.ln_slots % 5) != 0) return "the wide GEGLU tiles need N % 320 == 0 and ln_slots % 5 == 0";
    if ((p.ldc % 8) != 0 || (p.lda % 8) != 0) return "the wide GEGLU tiles need lda and ldc in whole 16-byte chunks";
  }
  return nullptr;
}

// Halo tiles: the block's patch, its LDS staging (gemm_impl.h conv3x3_halo_kernel) and what must fit
const char* route_halo(const GemmParams& p, int tile, GemmRoute& r) {
  const GemmTileInfo& t = kGemmTiles[tile];
  if (p.geglu) return "halo tiles: no geglu";
  if (!halo_patch(p.H, p.Wd, t.bm, &r.th, &r.tw)) return "halo tile: no patch of this block tiles the map";
  const int rpp = gemm_halo_dma_threads(tile) / 8;             // 128-B LDS rows one DMA pass fills
  const int pb = t.bm / (r.th * r.tw), hr = pb * (r.th + 2) * (r.tw + 2);
  const int apass = (hr + rpp - 1) / rpp, wpass = (t.bn + rpp - 1) / rpp;
  if (apass > 12) return "halo tile: the halo takes more than 12 DMA passes";
  // the folded skip connection is a one-tap K tail of the producer-specialised halo tiles; its three activation slots live in the
  // two halo buffers
  if (p.Cin2 > 0 && !t.ps) return "halo tile: only the producer-specialised ones take the folded skip";
  if (p.Cin2 > 0 && 3 * t.bm > 2 * apass * rpp) return "halo tile: the folded skip's three slots do not fit the two halo buffers";
  if (p.Cin2 > 0 && (p.lda2 & 7) != 0) return "halo tile: lda2 % 8 != 0";
  const size_t ring = ((size_t)2 * apass * rpp + (size_t)t.ring * wpass * rpp) * 128;
  r.halo_ring_bytes = (int)ring;
  r.lds = ring + (size_t)std::max(t.bm, hr) * 4;          // + the prologue's halo-row table / the epilogue's row table
  if (r.lds > 160 * 1024) return "halo tile: the staged patch exceeds 160 KiB of LDS";
  if ((p.lda & 7) != 0) return "halo tile: lda % 8 != 0 (the halo-row table keeps a 3-bit key in the low bits of a byte offset)";
  if ((long)p.M / (r.th * r.tw) + pb > (1 << 22)) return "halo tile: 2^22 patches or more (FastDiv range)";      // patches, rounded up to whole blocks
  return nullptr;
}

}  // namespace

const char* gemm_route(const GemmParams& p, int tile, int batch, int splitk, GemmRoute* out) {
  GemmRoute r{};
  const int sk = splitk > 1 ? splitk : 1;
  if (tile < 0 || tile >= TILE_ALL) return "no such tile";
  const GemmTileInfo& t = kGemmTiles[tile];
  r.family = t.family;
  r.mode = gemm_mode(p);
  r.zdim = sk > 1 ? sk : (batch > 0 ? batch : 1);
  // which (tile, MODE) pairs are built: gemm_tiles.def M0 .. M3 (a retired id: none)
  if (!((t.modes >> r.mode) & 1)) return "this tile is not built for the problem's MODE";
  if (p.taps == 9 && p.pad != 1 && (p.pad != 0 || r.mode != 2 || p.stride != 2 || p.ups))
    return "pad: 1 for every 3x3 conv, 0 only for the stride-2 conv of an asymmetrically padded Downsample";
  if (t.family == DF_FAM_PGEGLU || t.family == DF_FAM_WGEGLU) {
    if (const char* no = route_fused_geglu(p, t, batch, sk)) return no;
    r.epi = EPI_GEGLU;
    if (out) *out = r;
    return nullptr;
  }
  const bool rows4 = gemm_rows_vec4(p) && (p.N & 3) == 0;      // what every vectorised epilogue and the vectorised reduce need
  if (sk > 1 && batch > 1) return "split-K and a batch exclude each other";
  if (sk > 1 && (p.N & 3) != 0) return "split-K with N % 4 != 0 (the slabs are written and reduced as float4)";
  // epilogue features and the forms they exist in
  const bool lnf = p.ln_stats || p.stats || p.vt;
  if (lnf && (!rows4 || (p.N & 63) != 0))
    return "ln_stats / stats / vt exist in the vectorised epilogues only: row-major, N % 64 == 0, leading dimensions % 4 == 0";
  if (lnf && batch > 1) return "ln_stats / stats / vt with a batch";
  if (p.ln_stats && r.mode != 0) return "ln_stats on a conv";
  if (p.ln_stats && p.ln_slots > gemm_ln_max_slots()) return "more than 20 LayerNorm statistics slots";
  if (p.geglu && ((p.N & 63) != 0 || (p.ldc & 3) != 0)) return "geglu needs the vectorised block epilogue: N % 64 == 0, ldc % 4 == 0";
  if (p.vt && (sk > 1 || p.vt_col0 % t.bn != 0)) return "vt: transposed-V tiles are whole tiles (no split-K, vt_col0 % BN == 0)";
  if (p.vt && ((p.M & 3) != 0 || (p.vt_T & 3) != 0 || (p.ldvt & 3) != 0 || r.mode != 0 || !p.ln_stats))
    return "vt: LayerNorm-folded linear GEMM with M, vt_T and ldvt % 4 == 0";
  if (p.w_rows > 0 && (batch > 1 || r.mode != 0 || p.w_rows % t.bm != 0 || p.M % p.w_rows != 0))
    return "w_rows: linear, unbatched, w_rows % BM == 0 and M % w_rows == 0";
  if (p.sm_w > 0 && (p.sm_w != 32 || sk > 1 || !p.ln_stats || !p.out_bf16 || p.w_rows <= 0 || (p.N & 31) != 0 || p.geglu || p.vt || p.res ||
                     p.rowbias || p.aux || p.alpha != 1.f || !p.bias))
    return "sm_w: the score epilogue is 32 columns a head, LayerNorm-folded, per-sample weights, bias, operand-type out, no split-K";
  if (p.dup_rows > 0 && (batch > 1 || p.geglu || p.vt || p.sm_w > 0 || !rows4))
    return "dup_rows: plain row-major vectorised epilogues only, no geglu / vt / sm_w, no batch";
  if (p.Cin2 > 0 && (batch > 1 || (p.Cin2 & 63) != 0 || !p.A2)) return "Cin2: unbatched, whole 64-channel steps from A2";
  if (p.Cin2 > 0 && r.mode != 1 && (r.mode != 0 || p.Cin2 >= p.K))
    return "Cin2: a stride-1 conv's folded 1x1 skip, or the K columns [K - Cin2, K) of a linear GEMM";
  if (r.mode == 3) {     // phase-decomposed upsample conv: plain epilogues on the x2 map
    if (batch > 1 || p.geglu || p.stats || p.res || p.store_nchw) return "MODE 3: plain unbatched row-major epilogues without residual only";
    if (p.OH != p.H || p.OW != p.Wd || p.K != 4 * p.Cin || p.w_bs != (long)p.N * p.K)
      return "MODE 3: OH x OW is the input map, K = 4 Cin, w_bs = N K between the four phases' weights";
  }
  if (t.family == DF_FAM_HALO) {
    if (batch > 1) return "halo tiles with a batch";
    if (const char* no = route_halo(p, tile, r)) return no;
  }
  // the epilogue the kernel carries (gemm_impl.h): only the code it runs
  const bool vec = rows4 && gemm_batch_vec4(p);
  if (sk > 1) r.epi = EPI_SPLITK;
  else if (p.sm_w > 0) r.epi = EPI_XS;
  else if (p.geglu) r.epi = EPI_GEGLU;
  else if (p.ln_stats || p.vt) r.epi = EPI_LNC;
  else if (p.stats) r.epi = EPI_PROD;
  else if (!vec || p.relu || p.aux || p.alpha != 1.f) r.epi = EPI_ANY;
  else r.epi = EPI_LEAN;
  // which (MODE, epilogue) pairs are built (gemm_m0a .. gemm_ps2.hip, gemm_halo.hip): LEAN, SPLITK and ANY for every MODE,
  // the rest for MODE 0 alone
  if (r.epi == EPI_GEGLU || r.epi == EPI_PROD || r.epi == EPI_LNC || r.epi == EPI_XS) {
    if (r.mode != 0) return "the GEGLU / PROD / LNC / XS epilogues are built for MODE 0 (linear) only";
    if (!vec) return "the GEGLU / PROD / LNC / XS epilogues are vectorised: N, leading dimensions and batch strides % 4 == 0";
    if (r.epi != EPI_XS && (p.alpha != 1.f || p.relu || p.silu)) return "alpha / relu / silu with a GEGLU / PROD / LNC epilogue";
    if (r.epi == EPI_LNC && p.aux) return "aux with ln_stats";
  }
  if (sk > 1) {     // who sums the slabs
    const bool vec_red = !p.geglu && rows4 && reduce_vec_built(sk);
    if (!vec_red && (p.ln_stats || p.stats || p.dup_rows > 0 || p.no_c_store))
      return "ln_stats / stats / dup_rows / no_c_store with a split-K only the scalar reduce sums (geglu, or a split count the vectorised one is not built for)";
    if (p.defer_reduce) {
      if (p.dup_rows > 0) return "dup_rows with a deferred split-K reduce";
      r.reduce = DF_RED_DEFERRED;
    } else if (r.mode == 3 && !rows4) {
      return "MODE 3 split-K: the reduce of the x2 map needs aligned rows (leading dimensions % 4 == 0)";
    } else if (vec_red) {
      r.reduce = DF_RED_VEC;
    } else if (p.cfg_out) {
      if (!p.store_nchw || p.geglu || p.res || p.aux || p.silu || p.relu || (p.M & 1) || p.hw_out <= 0 || (p.M >> 1) % p.hw_out != 0)
        return "cfg_out: NCHW store of an even batch of whole samples, bias only";
      r.reduce = DF_RED_CFG;
    } else {
      r.reduce = DF_RED_SCALAR;
    }
  }
  if (out) *out = r;
  return nullptr;
}

GemmMagic gemm_magic(int d) {
  // l = ceil(log2 d); mul = floor(2^(31 + l) / d) + 1 < 2^32 (d > 2^(l - 1)); mul d = 2^(31 + l) + e with 0 < e <= d <= 2^l, so
  // x mul / 2^(31 + l) = x / d + x e / (d 2^(31 + l)) and the excess stays below 1 / d for x < 2^31: the floor is x / d.
  // (d == 1 has no 32-bit multiplier: the device returns x.)
  GemmMagic m{0u, 0, d};
  if (d < 2) return m;
  int l = 1;
  while (l < 31 && (1l << l) < (long)d) ++l;
  m.mul = (unsigned)((((unsigned long)1 << (31 + l)) / (unsigned long)d) + 1);
  m.sh = l - 1;
  return m;
}

void gemm_launch_consts(const GemmParams& p, int tile, int splitk, const GemmRoute& r, GemmLaunch* out) {
  GemmLaunch c{};
  const GemmTileInfo& t = kGemmTiles[tile];
  const auto inv = [](int d) { return 1.0f / (float)std::max(d, 1); };     // FastDiv's reciprocal (gemm_impl.h)
  const int sk = splitk > 1 ? splitk : 1;
  const bool halo = r.family == DF_FAM_HALO;
  if (halo) {
    const int TH = r.th, TW = r.tw;
    c.HWp = (TH + 2) * (TW + 2);
    c.PPX = TH * TW;
    c.PB = t.bm / c.PPX;
    c.HR = c.PB * c.HWp;
    const int rpp = gemm_halo_dma_threads(tile) / 8;
    c.APASS = (c.HR + rpp - 1) / rpp;
    c.npx = p.Wd / TW;
    c.npy = p.H / TH;
    c.pimg = c.npx * c.npy;
    c.npatch = p.M / c.PPX;
    c.inv_hwp = inv(c.HWp); c.inv_tw2 = inv(TW + 2); c.inv_pimg = inv(c.pimg);
    c.inv_npx = inv(c.npx); c.inv_ppx = inv(c.PPX); c.inv_tw = inv(TW);
    c.nbm = (c.npatch + c.PB - 1) / c.PB;
    c.nk = p.Cin / 64;
  } else {
    c.nbm = (p.M + t.bm - 1) / t.bm;
    c.nk = p.K / 64;
  }
  c.nbn = (p.N + t.bn - 1) / t.bn;
  c.nblk = c.nbm * c.nbn;
  c.xq = c.nblk >> 3;
  c.xr = c.nblk & 7;
  c.gm = (p.gm <= 0 || p.gm >= c.nbm) ? std::max(c.nbm, 1) : p.gm;
  const int last = c.nbm % c.gm;
  c.per = gemm_magic(c.gm * c.nbn); c.rows = gemm_magic(c.gm); c.last = gemm_magic(last ? last : c.gm);
  c.kper = (c.nk + sk - 1) / sk;
  c.n2tot = p.Cin2 / 64;
  c.used = c.kper > 0 ? (c.nk + c.kper - 1) / c.kper : 1;
  c.per2 = (c.n2tot + std::max(c.used, 1) - 1) / std::max(c.used, 1);
  c.wrb = gemm_magic(p.w_rows > 0 ? p.w_rows / t.bm : 0);
  c.ohw = gemm_magic(std::max(p.OH * p.OW, 1));
  c.ow = gemm_magic(std::max(p.OW, 1));
  c.cin = gemm_magic(std::max(p.Cin, 1));
  *out = c;
}

bool gemm_split_worth_tuning(const GemmParams& p, int tile, int splitk) {
  if (splitk <= 1) return true;
  return gemm_tile_is_halo(tile) ? p.Cin / 64 / splitk >= 1 : p.K / 64 / splitk >= 2;
}

bool gemm_tile_valid(const GemmParams& p, int tile, int batch, int splitk) {
  return gemm_route(p, tile, batch, splitk, nullptr) == nullptr && gemm_split_worth_tuning(p, tile, splitk);
}

hipError_t launch_gemm(const GemmParams& p, int tile_cfg, int batch, hipStream_t stream, const char** why) {
  GemmRoute r;
  const char* no = gemm_route(p, tile_cfg, batch, p.splitk, &r);
  if (why) *why = no;
  if (no) return hipErrorInvalidValue;
  const int part = kGemmTiles[tile_cfg].part;
  hipError_t e;
  if (r.family == DF_FAM_PGEGLU) return launch_gemm_pgeglu(tile_cfg, p, stream);
  GemmParams q = p;        // what the kernels get: the problem + the launch constants (+ the halo tiles' patch)
  gemm_launch_consts(p, tile_cfg, p.splitk, r, &q.lc);
  if (r.family == DF_FAM_WGEGLU) return launch_gemm_wgeglu(tile_cfg, q, stream);
  if (r.family == DF_FAM_HALO) {
    q.th = r.th; q.tw = r.tw; q.halo_ring_bytes = r.halo_ring_bytes;
    e = launch_gemm_halo(tile_cfg, r.epi, q, r.zdim, r.lds, stream);
  } else if (r.family == DF_FAM_PS) e = part ? launch_gemm_ps_small(r.mode, tile_cfg, r.epi, q, r.zdim, stream) : launch_gemm_ps(r.mode, tile_cfg, r.epi, q, r.zdim, stream);
  else if (r.mode == 0) e = part ? launch_gemm_m0b(tile_cfg, r.epi, q, r.zdim, stream) : launch_gemm_m0a(tile_cfg, r.epi, q, r.zdim, stream);
  else if (r.mode == 1) e = launch_gemm_m1(tile_cfg, r.epi, q, r.zdim, stream);
  else if (r.mode == 2) e = launch_gemm_m2(tile_cfg, r.epi, q, r.zdim, stream);
  else e = launch_gemm_m3(tile_cfg, r.epi, q, r.zdim, stream);
  if (e != hipSuccess || r.reduce == DF_RED_NONE || r.reduce == DF_RED_DEFERRED) return e;
  if (r.mode != 3) return launch_splitk_reduce(p, r.reduce, stream);
  q = p;
  q.M = 4 * p.M;           // the slabs hold the x2 output map
  q.taps = 1;
  return launch_splitk_reduce(q, r.reduce, stream);
}

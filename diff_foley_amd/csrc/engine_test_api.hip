// libdfengine: single-kernel entry points for unit tests and tools (df_test_*; include/df_engine.h).
#include "engine_internal.h"

using namespace dfe;

extern "C" {

// ---- single-kernel entry points for unit tests
// grow-only split-K scratch shared by the test entry points (no allocation inside timed loops)
static float* test_partial(size_t bytes) {
  static float* buf = nullptr;
  static size_t cap = 0;
  if (bytes > cap) {
    if (buf) {
      (void)hipDeviceSynchronize();
      (void)hipFree(buf);
    }
    HIPCHK(hipMalloc((void**)&buf, bytes));
    cap = bytes;
  }
  return buf;
}

// Test input -> GemmParams: every operand form and epilogue feature the plans use.  The one translation; run_test_gemm below is the
// one launch behind the eight single-GEMM entry points.
static void test_gemm_params(const df_test_gemm_desc* d, GemmParams& g) {
  if (!d) fail("df_test_gemm: null descriptor");
  if (d->size != (int64_t)sizeof(df_test_gemm_desc))
    fail("df_test_gemm: descriptor of %lld bytes, this build expects %zu (stale binding of df_test_gemm_desc?)", (long long)d->size,
         sizeof(df_test_gemm_desc));
  const bf16_t* A = (const bf16_t*)d->A;
  const bf16_t* W = (const bf16_t*)d->W;
  if (d->conv == 2) {        // phase-decomposed upsample conv: W is the packed [2][2][N][2][2][Cin] operand
    if (d->ups || d->zstuff || d->stride > 1) fail("df_test_gemm: conv 2 takes neither ups / zstuff nor a stride");
    g = Builder::gp_conv3_ups4(A, d->NB, d->H, d->Wd, d->Cin, W, d->N);
  } else if (d->conv) {
    if (d->conv != 1) fail("df_test_gemm: conv %d", d->conv);
    if (d->stride != 1 && d->stride != 2) fail("df_test_gemm: conv stride %d", d->stride);
    if (d->zstuff && !d->ups) fail("df_test_gemm: zstuff without ups");
    if (d->ups && d->stride != 1) fail("df_test_gemm: ups with stride %d", d->stride);
    g = Builder::gp_conv3(A, d->NB, d->H, d->Wd, d->Cin, W, d->N, d->stride, d->ups ? 1 : 0);
    g.zstuff = d->zstuff ? 1 : 0;
  } else {
    if (d->ups || d->zstuff) fail("df_test_gemm: ups / zstuff on a linear GEMM");
    g = Builder::gp_linear(A, d->M, d->K, W, d->N);
    if (d->lda > 0) {
      g.lda = d->lda;
      g.a_bytes = Builder::op_bytes((size_t)d->M * d->lda * 2);
    }
  }
  if (d->Cin2 > 0 || d->A2) {     // a second operand tensor for the last Cin2 K columns, sized as the builder sizes it
    if (d->Cin2 <= 0 || d->lda2 < d->Cin2) fail("df_test_gemm: A2 with Cin2 %d / lda2 %d", d->Cin2, d->lda2);
    Builder::add_a2(g, (const bf16_t*)d->A2, d->lda2, d->Cin2);
  }
  g.geglu = d->geglu ? 1 : 0;
  g.vt = (bf16_t*)d->vt; g.vt_col0 = d->vt_col0; g.vt_T = d->vt_T; g.ldvt = d->ldvt;
  g.C = d->C; g.ldc = d->ldc > 0 ? d->ldc : (g.geglu ? g.N / 2 : g.N); g.out_bf16 = d->out_operand ? 1 : 0;
  g.a_bs = d->a_bs; g.c_bs = d->c_bs; g.res_bs = d->res_bs;
  if (d->conv != 2) g.w_bs = d->w_bs;      // phase-decomposed: the builder's stride between the four phases' weights stays
  g.alpha = d->alpha;
  g.bias = d->bias;
  g.rowbias = d->rowbias; g.ld_rowbias = d->ld_rowbias; g.rows_per_sample = d->rows_per_sample; g.rowbias_mode = d->rowbias_mode;
  g.res = d->res; g.ldr = d->ldr;
  g.relu = d->relu; g.silu = d->silu;
  g.aux = (bf16_t*)d->aux; g.ld_aux = d->ld_aux;
  g.stats = (float2*)d->stats; g.stats_slots = d->stats_slots;
  g.ln_stats = (const float2*)d->ln_stats; g.ln_slots = d->ln_slots; g.ln_C = d->ln_C; g.ln_eps = d->ln_eps; g.ln_cs = d->ln_cs;
  g.w_rows = d->w_rows; g.sm_w = d->sm_w; g.sm_valid = d->sm_valid;
  g.dup_rows = d->dup_rows; g.no_c_store = d->no_c_store; g.store_nchw = d->store_nchw; g.hw_out = d->hw_out;
  g.cfg_out = d->cfg_out; g.cfg_scale = d->cfg_scale;
  g.defer_reduce = d->defer_reduce;
  g.gm = d->gm;
  g.splitk = d->splitk > 1 ? d->splitk : 1;
  // the wide GEGLU tiles read a 320-column packing that run_test_gemm makes per call; for the host-only queries it is "there"
  // exactly when its three sources are
  if (g.geglu && g.N % 320 == 0) { g.W_w320 = W; g.cs_w320 = g.ln_cs; g.bias_w320 = g.bias; }
}

// 0: launchable and inside the tuner's split policy;  1: launchable, outside the policy;  2: refused, the rule in buf;  -1: bad descriptor
int df_test_gemm_why(const df_test_gemm_desc* d, int tile, int batch, int splitk, char* buf, int n) {
  std::lock_guard<std::recursive_mutex> hold(g_api_lock);
  try {
    GemmParams g;
    test_gemm_params(d, g);
    const char* why = gemm_route(g, tile, batch, splitk, nullptr);
    if (buf && n > 0) snprintf(buf, (size_t)n, "%s", why ? why : "");
    return why ? 2 : (gemm_split_worth_tuning(g, tile, splitk) ? 0 : 1);
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

int df_test_gemm_valid(const df_test_gemm_desc* d, int tile, int batch, int splitk) {
  const int r = df_test_gemm_why(d, tile, batch, splitk, nullptr, 0);
  return r < 0 ? -1 : (r == 0 ? 1 : 0);
}

int df_test_gemm_key(const df_test_gemm_desc* d, int batch, char* buf, int n) {
  std::lock_guard<std::recursive_mutex> hold(g_api_lock);
  try {
    GemmParams g;
    test_gemm_params(d, g);
    const std::string key = tune_key(g, batch > 1 ? batch : 1, d->defer_reduce != 0);
    if (!buf || n <= (int)key.size()) fail("df_test_gemm_key: buffer of %d bytes for a key of %zu", n, key.size());
    memcpy(buf, key.c_str(), key.size() + 1);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

int df_test_gemm_launch_constants(const df_test_gemm_desc* d, int tile, int batch, int splitk, df_test_gemm_launch* out) {
  std::lock_guard<std::recursive_mutex> hold(g_api_lock);
  try {
    if (!out || out->size != (int64_t)sizeof(df_test_gemm_launch)) fail("df_test_gemm_launch_constants: a df_test_gemm_launch of another size");
    GemmParams g;
    test_gemm_params(d, g);
    GemmRoute r;
    if (const char* why = gemm_route(g, tile, batch, splitk, &r)) {
      g_err = std::string("df_test_gemm_launch_constants: launch_gemm refuses this problem (") + why + ")";
      return 2;
    }
    GemmLaunch c;
    gemm_launch_consts(g, tile, splitk, r, &c);
    out->nbm = c.nbm; out->nbn = c.nbn; out->nblk = c.nblk; out->xq = c.xq; out->xr = c.xr; out->gm = c.gm;
    const GemmMagic* mg[7] = {&c.per, &c.rows, &c.last, &c.wrb, &c.ohw, &c.ow, &c.cin};
    for (int i = 0; i < 7; ++i) {
      out->magic[i].mul = mg[i]->mul; out->magic[i].sh = mg[i]->sh; out->magic[i].d = mg[i]->d;
    }
    out->nk = c.nk; out->kper = c.kper; out->n2tot = c.n2tot; out->used = c.used; out->per2 = c.per2;
    out->HWp = c.HWp; out->PPX = c.PPX; out->PB = c.PB; out->HR = c.HR; out->APASS = c.APASS;
    out->npx = c.npx; out->npy = c.npy; out->pimg = c.pimg; out->npatch = c.npatch;
    out->inv_hwp = c.inv_hwp; out->inv_tw2 = c.inv_tw2; out->inv_pimg = c.inv_pimg; out->inv_npx = c.inv_npx;
    out->inv_ppx = c.inv_ppx; out->inv_tw = c.inv_tw;
    out->th = r.th; out->tw = r.tw;
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

int df_test_gemm_tile_info(int tile, df_test_gemm_tile* out) {
  std::lock_guard<std::recursive_mutex> hold(g_api_lock);
  if (tile < 0 || tile >= TILE_ALL || !out || out->size != (int64_t)sizeof(df_test_gemm_tile)) {
    g_err = "df_test_gemm_tile_info: no tile " + std::to_string(tile) + ", or a df_test_gemm_tile of another size";
    return 1;
  }
  const GemmTileInfo& t = kGemmTiles[tile];
  out->name = t.name; out->family = t.family; out->modes = t.modes;
  out->bm = t.bm; out->bn = t.bn; out->dma_threads = gemm_halo_dma_threads(tile); out->ring = t.ring;
  return 0;
}

// The wide GEGLU tiles read the 320-column packing of (W, column sums, bias): permuted here into a grow-only scratch, on every
// call -- unless `keep` (timing tools) and the packing in the scratch was made from this W by the call before.
static void test_pack_w320(GemmParams& g, bool keep, hipStream_t s) {
  static void* buf = nullptr;
  static size_t cap = 0;
  static const void* packed_from = nullptr;
  const size_t wb = ((size_t)g.N * g.K * 2 + 255) & ~(size_t)255, need = wb + (size_t)g.N * 8 + 512;
  if (need > cap) {
    if (buf) {
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipFree(buf));
      buf = nullptr; cap = 0;
    }
    packed_from = nullptr;
    HIPCHK(hipMalloc(&buf, need));
    cap = need;
  }
  uint16_t* w3 = (uint16_t*)buf;
  float* cs3 = (float*)((char*)buf + wb);
  float* bb3 = cs3 + g.N;
  if (!keep || packed_from != (const void*)g.W) HIPCHK(launch_pack_w320(g.W, g.ln_cs, g.bias, w3, cs3, bb3, g.N, g.K, s));
  packed_from = (const void*)g.W;
  g.W_w320 = w3; g.cs_w320 = cs3; g.bias_w320 = bb3;
}

// What the single-GEMM entry points differ in once their descriptor is filled.
struct TestGemmOpts {
  int dbg = 0;                   // GemmParams::dbg (tools: timing switches, bit 6 = per-block clock stamps into the shared scratch)
  bool tuner_policy = false;     // also apply the tuner's split policy (gemm_split_worth_tuning); launch_gemm itself refuses what cannot run
  bool keep_w320 = false;        // wide GEGLU tiles: reuse the packing the previous call made from the same W
};
static int env_gemm_dbg() { return getenv("DF_GEMM_DBG") ? atoi(getenv("DF_GEMM_DBG")) : 0; }

// launch_gemm; its refusal (made on the host, nothing launched) names the rule
static void test_launch_gemm(const GemmParams& g, int tile, int batch, hipStream_t s, const char* role = "") {
  const char* why = nullptr;
  const hipError_t e = launch_gemm(g, tile, batch, s, &why);
  if (e == hipErrorInvalidValue)
    fail("%slaunch_gemm refused tile %d / split-K %d / batch %d (%dx%dx%d): %s (%s)", role, tile, g.splitk, batch, g.M, g.N, g.K,
         hipGetErrorString(e), why ? why : "the launch itself");
  HIPCHK(e);
}

// descriptor -> GemmParams -> launch: everything the eight single-GEMM entry points below do on the device
static void run_test_gemm(const df_test_gemm_desc& d, const TestGemmOpts& o, hipStream_t s) {
  GemmParams g;
  test_gemm_params(&d, g);
  const int batch = d.batch > 1 ? d.batch : 1;
  // as Builder::gemm: the K loop of every kernel walks whole 64-element steps, a ragged K would silently drop its tail
  if (g.K % 64 != 0 || (g.taps != 1 && g.Cin % 64 != 0))
    fail("df_test_gemm (%dx%dx%d, Cin %d): the contraction length must be a multiple of 64", g.M, g.N, g.K, g.Cin);
  if (d.defer_reduce && g.splitk < 2) fail("df_test_gemm: defer_reduce needs split-K");
  g.dbg = o.dbg;
  if (o.tuner_policy && !gemm_split_worth_tuning(g, d.tile, g.splitk)) fail("tile %d / split-K %d refused this problem", d.tile, g.splitk);
  const size_t slab_bytes = (size_t)g.splitk * g.M * g.N * 4 * (g.taps == 4 ? 4 : 1);     // phase-decomposed: four slabs per split
  if (g.splitk > 1) g.partial = test_partial(slab_bytes);
  else if (g.dbg & 64) g.partial = test_partial((size_t)4096 * 32 * 8);      // per-block clock stamps (df_test_scratch_read)
  if (gemm_tile_is_wgeglu(d.tile) && g.geglu) {
    if (g.N % 320 != 0 || !g.ln_cs || !g.bias) fail("tile %d: N = %d is not a multiple of 320, or no column sums / bias", d.tile, g.N);
    test_pack_w320(g, o.keep_w320, s);
  }
  test_launch_gemm(g, d.tile, batch, s);
  if (d.defer_reduce && d.slabs_out) HIPCHK(hipMemcpyAsync(d.slabs_out, g.partial, slab_bytes, hipMemcpyDeviceToDevice, s));
}

int df_test_gemm_ex(const df_test_gemm_desc* d, void* stream) {
  return guard([&] {
    if (!d) fail("df_test_gemm: null descriptor");
    run_test_gemm(*d, TestGemmOpts{}, (hipStream_t)stream);
  });
}

// ---- the fixed-shape entry points: each fills a descriptor and runs it
static df_test_gemm_desc test_desc(const void* A, const void* W, void* C, int tile, int splitk) {
  df_test_gemm_desc d{};
  d.size = sizeof d;
  d.alpha = 1.f;
  d.A = A; d.W = W; d.C = C; d.tile = tile; d.splitk = splitk;
  return d;
}
static df_test_gemm_desc test_desc_conv(const void* A, const void* W, void* C, int tile, int splitk, int conv, int NB, int H, int Wd,
                                        int Cin, int Cout, const float* bias) {
  df_test_gemm_desc d = test_desc(A, W, C, tile, splitk);
  d.conv = conv; d.NB = NB; d.H = H; d.Wd = Wd; d.Cin = Cin; d.N = Cout; d.stride = 1; d.bias = bias;
  return d;
}

// outside the tuner's split policy too, DF_GEMM_DBG from the environment: the tools time (tile, split-K) pairs the tuner would not pick
int df_test_gemm(const uint16_t* A, const uint16_t* W, float* C, int M, int N, int K, int tile, int splitk, void* stream) {
  return guard([&] {
    df_test_gemm_desc d = test_desc(A, W, C, tile, splitk);
    d.M = M; d.N = N; d.K = K;
    run_test_gemm(d, {env_gemm_dbg(), false, false}, (hipStream_t)stream);
  });
}

// bias, residual, activation (1 = SiLU, 2 = ReLU), fp32 or operand-type output
int df_test_gemm_epi(const uint16_t* A, const uint16_t* W, const float* bias, const float* res, void* C, int M, int N, int K,
                     int act, int out_operand, int tile, int splitk, void* stream) {
  return guard([&] {
    df_test_gemm_desc d = test_desc(A, W, C, tile, splitk);
    d.M = M; d.N = N; d.K = K;
    d.bias = bias;
    d.res = res; d.ldr = res ? N : 0;
    d.silu = act == 1; d.relu = act == 2;
    d.out_operand = out_operand;
    run_test_gemm(d, {0, true, false}, (hipStream_t)stream);
  });
}

// C = [A | A2] W^T with the K columns split over two operand tensors (the merged FF2 + proj_out GEMM of the SpatialTransformer)
int df_test_gemm_dual(const uint16_t* A, const uint16_t* A2, const uint16_t* W, float* C, int M, int N, int K1, int K2, int tile,
                      int splitk, void* stream) {
  return guard([&] {
    df_test_gemm_desc d = test_desc(A, W, C, tile, splitk);
    d.M = M; d.N = N; d.K = K1;
    d.A2 = A2; d.lda2 = K2; d.Cin2 = K2;
    run_test_gemm(d, {0, true, false}, (hipStream_t)stream);
  });
}

// as df_test_gemm: no split policy, DF_GEMM_DBG from the environment
int df_test_conv3x3(const uint16_t* A, const uint16_t* W, const float* bias, float* C, int NB, int H, int Wd, int Cin,
                    int Cout, int stride, int ups, int tile, int splitk, void* stream) {
  return guard([&] {
    df_test_gemm_desc d = test_desc_conv(A, W, C, tile, splitk, 1, NB, H, Wd, Cin, Cout, bias);
    d.stride = stride; d.ups = ups;
    run_test_gemm(d, {env_gemm_dbg(), false, false}, (hipStream_t)stream);
  });
}

int df_test_conv3x3_skip(const uint16_t* A, const uint16_t* A2, const uint16_t* W, const float* bias, float* C, int NB, int H,
                         int Wd, int Cin, int Cin2, int Cout, int tile, int splitk, void* stream) {
  return guard([&] {
    df_test_gemm_desc d = test_desc_conv(A, W, C, tile, splitk, 1, NB, H, Wd, Cin, Cout, bias);
    d.A2 = A2; d.lda2 = Cin2; d.Cin2 = Cin2;
    run_test_gemm(d, {0, true, false}, (hipStream_t)stream);
  });
}

// Upsample + conv3x3 through the phase-decomposed form (gemm_m3.hip): W_oihw fp32 [Cout][Cin][3][3] is packed here.
int df_test_conv3x3_ups4(const uint16_t* A, const float* W_oihw, const float* bias, float* C, uint16_t* w4_scratch, int NB, int H,
                         int Wd, int Cin, int Cout, int tile, int splitk, void* stream) {
  return guard([&] {
    HIPCHK(launch_pack_conv_ups4(W_oihw, w4_scratch, Cout, Cin, Cin, (hipStream_t)stream));
    const df_test_gemm_desc d = test_desc_conv(A, w4_scratch, C, tile, splitk, 2, NB, H, Wd, Cin, Cout, bias);
    run_test_gemm(d, {0, true, false}, (hipStream_t)stream);
  });
}

// The LayerNorm-folded GEGLU projection alone, on caller-owned operands (timing probes: tools/pgeglu_probe.py).  stats [M][K/64]
// float2, cs / bias [N1]; dbg = debug switches of the persistent kernel (ffn.hip) or DF_GEMM_DBG of the generic one; its bit 7 is
// this entry's own: keep the wide tiles' packing made from the same W by the previous call.
int df_test_geglu(const uint16_t* A, const uint16_t* W, const void* stats, const float* cs, const float* bias, uint16_t* out, int M,
                  int K, int N1, int tile, int dbg, void* stream) {
  return guard([&] {
    df_test_gemm_desc d = test_desc(A, W, out, tile, 1);
    d.M = M; d.N = N1; d.K = K;
    d.geglu = 1; d.out_operand = 1;
    d.ln_stats = stats; d.ln_slots = K / 64; d.ln_C = K; d.ln_eps = 1e-5f; d.ln_cs = cs;
    d.bias = bias;
    run_test_gemm(d, {dbg & ~128, true, (dbg & 128) != 0}, (hipStream_t)stream);
  });
}

// The folded cross-attention exactly as context_px + the SpatialTransformer plan run it, every intermediate returned:
// ctx.kv (kv = ctx Wkv^T), xattn_expand (Kexp / Vexp), the lnq_t packing of (norm2.gamma, to_q) (WqT), ctx.g (G = Kexp WqT^T),
// xattn_rowstats (cs, bb from bq = Wq beta), the batched ctx.vo (Vo[n] = Wo Vexp[n]^T), then st.xs (probabilities P from the
// operand copy xb of the residual stream x and its per-64-column (sum, sum of squares) statistics) and st.xo (out = x + P Vo^T + bo,
// fp32).  ctx.kv / ctx.g / ctx.vo run on the 64 x 64 tile; st.xs and st.xo on the caller's tiles.
int df_test_xattn_chain(const uint16_t* ctx, const uint16_t* Wkv, const float* Wq, const float* gamma, const float* bq,
                        const uint16_t* Wo, const float* bo, const float* x, const uint16_t* xb, const void* xstats, int NB, int T,
                        int Tc, int Dc, int C, int heads, uint16_t* kv, uint16_t* Kexp, uint16_t* Vexp, uint16_t* WqT, uint16_t* G,
                        float* cs, float* bb, uint16_t* Vo, uint16_t* P, float* out, int tile_xs, int tile_xo, void* stream) {
  return guard([&] {
    hipStream_t s = (hipStream_t)stream;
    const int HT = heads * 32, M = NB * T;
    const float scale = 1.0f / sqrtf((float)(C / heads));
    if (Tc < 1 || Tc > 32 || C % 64 != 0 || C % heads != 0 || (C / heads) % 8 != 0 || HT % 64 != 0 || T % 64 != 0 || Dc % 64 != 0)
      fail("xattn chain: C %d / heads %d / Tc %d / T %d / Dc %d outside what the folded form takes", C, heads, Tc, T, Dc);
    auto run = [&](const GemmParams& g, int tile, int batch, const char* what) { test_launch_gemm(g, tile, batch, s, what); };
    {
      GemmParams g = Builder::gp_linear(ctx, NB * Tc, Dc, Wkv, 2 * C);
      Builder::out_b16(g, kv, 2 * C);
      run(g, TILE_64x64, 1, "xattn chain ctx.kv: ");
    }
    HIPCHK(launch_xattn_expand(kv, Kexp, Vexp, NB, Tc, 32, C, heads, s));
    HIPCHK(launch_pack_lnq_t(Wq, gamma, WqT, C, scale, s));
    {
      GemmParams g = Builder::gp_linear(Kexp, NB * HT, C, WqT, C);
      Builder::out_b16(g, G, C);
      run(g, TILE_64x64, 1, "xattn chain ctx.g: ");
    }
    HIPCHK(launch_xattn_rowstats(G, Kexp, bq, scale, C, (long)NB * HT, cs, bb, s));
    {
      GemmParams g = Builder::gp_linear(Wo, C, C, Vexp, HT);
      g.w_bs = (long)HT * C;
      Builder::out_b16(g, Vo, HT);
      g.c_bs = (long)C * HT;
      run(g, TILE_64x64, NB, "xattn chain ctx.vo: ");
    }
    {
      GemmParams g = Builder::gp_linear(xb, M, C, G, HT);
      g.w_bs = (long)HT * C; g.w_rows = T;
      Builder::out_b16(g, P, HT);
      g.ln_stats = (const float2*)xstats; g.ln_slots = C / 64; g.ln_C = C; g.ln_eps = 1e-5f; g.ln_cs = cs;
      g.bias = bb;
      g.sm_w = 32; g.sm_valid = Tc;
      run(g, tile_xs, 1, "xattn chain st.xs: ");
    }
    {
      GemmParams g = Builder::gp_linear(P, M, HT, Vo, C);
      g.w_bs = (long)C * HT; g.w_rows = T;
      Builder::out_f32(g, out, C);
      g.bias = bo;
      g.res = x; g.ldr = C;
      run(g, tile_xo, 1, "xattn chain st.xo: ");
    }
  });
}

// FeedForward's second Linear merged with proj_out (launch_pack_ffproj): wout [C][F + C] = [Wp W2 | Wp], bout = Wp b2 + bp.
int df_test_pack_ffproj(const float* Wp, const float* bp, const float* W2, const float* b2, uint16_t* wout, float* bout, int C, int F,
                        void* stream) {
  return guard([&] { HIPCHK(launch_pack_ffproj(Wp, bp, W2, b2, wout, bout, C, F, (hipStream_t)stream)); });
}

// Producer GEMM (t0 = A0 W0^T + b0 [+ t0_in], fp32 + operand copy + per-row partial statistics) followed by a
// LayerNorm-folded consumer GEMM (y = LN(t0; gamma, beta) W1^T + b1), exactly the pair the SpatialTransformer plan uses.
// mode 0: y fp32 [M][N1];  mode 1: GEGLU (W1 = [x ; gate] rows, y operand-type [M][N1/2]);  mode 2: fused QKV --
// N1 = 3C, y operand-type [M][2C] and vt operand-type [M/T][C][ldvt] (V columns transposed per sample of T rows).
int df_test_ln_chain(const uint16_t* A0, const uint16_t* W0, const float* b0, const float* res_in, const float* gamma,
                     const float* beta, const float* W1, const float* b1, float* t0, void* y, uint16_t* vt, int M, int C,
                     int N1, int mode, int T, int ldvt, int tile0, int sk0, int tile1, int sk1, void* stream) {
  return guard([&] {
    hipStream_t s = (hipStream_t)stream;
    const int slots = C / 64;
    uint16_t *xb = nullptr, *w1p = nullptr;
    float2* st = nullptr;
    float *cs = nullptr, *bb = nullptr;
    HIPCHK(hipMalloc((void**)&xb, (size_t)M * C * 2));
    HIPCHK(hipMalloc((void**)&st, (size_t)M * slots * sizeof(float2)));
    HIPCHK(hipMalloc((void**)&w1p, (size_t)N1 * C * 2));
    HIPCHK(hipMalloc((void**)&cs, (size_t)N1 * 4));
    HIPCHK(hipMalloc((void**)&bb, (size_t)N1 * 4));
    HIPCHK(hipMemsetAsync(st, 0xFF, (size_t)M * slots * sizeof(float2), s));      // NaN poison: every slot must be written
    HIPCHK(launch_pack_ln_linear(W1, b1, gamma, beta, w1p, cs, bb, N1, C, 0, mode == 1 ? N1 / 2 : 0, s));
    {
      GemmParams g = Builder::gp_linear(A0, M, C, W0, C);
      Builder::out_f32(g, t0, C);
      g.bias = b0;
      if (res_in) { g.res = res_in; g.ldr = C; }
      g.aux = xb; g.ld_aux = C;
      g.stats = st; g.stats_slots = slots;
      g.splitk = sk0;
      if (sk0 > 1) g.partial = test_partial((size_t)sk0 * M * C * 4);
      test_launch_gemm(g, tile0, 1, s, "producer: ");
    }
    {
      GemmParams g = Builder::gp_linear(xb, M, C, w1p, N1);
      g.ln_stats = st; g.ln_slots = slots; g.ln_C = C; g.ln_eps = 1e-5f; g.ln_cs = cs;
      g.bias = bb;
      if (mode == 0) Builder::out_f32(g, (float*)y, N1);
      else if (mode == 1) { Builder::out_b16(g, (bf16_t*)y, N1 / 2); g.geglu = 1; }
      else {
        Builder::out_b16(g, (bf16_t*)y, 2 * C);
        g.vt = vt; g.vt_col0 = 2 * C; g.vt_T = T; g.ldvt = ldvt;
      }
      g.splitk = sk1;
      if (sk1 > 1) g.partial = test_partial((size_t)sk1 * M * N1 * 4);
      test_launch_gemm(g, tile1, 1, s, "consumer: ");
    }
    HIPCHK(hipStreamSynchronize(s));
    for (void* p : {(void*)xb, (void*)st, (void*)w1p, (void*)cs, (void*)bb}) (void)hipFree(p);
  });
}

int df_test_scratch_read(void* host, int64_t bytes) {
  return guard([&] {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host, test_partial((size_t)bytes), (size_t)bytes, hipMemcpyDeviceToHost));
  });
}

int df_test_linear_rows(const float* a, int lda, const uint16_t* W, const float* bias, float* out, int ldo, int M, int N, int K,
                        int act, void* stream) {
  return guard([&] { HIPCHK(launch_linear_rows(a, lda, W, bias, out, ldo, M, N, K, act, (hipStream_t)stream)); });
}

// ONE block of the loaded UNet in isolation, against the reference's per-block tensors (golden G3): the plan builder's
// own resblock / spatial_transformer / Downsample / Upsample code paths on caller-supplied NHWC fp32 activations.
//   kind 0 ResBlock (semb = SiLU(time_embed(t)) [N][4*model_channels]), 1 SpatialTransformer (context [N][T][context_dim]),
//   2 Downsample, 3 Upsample.  x [N*H*W][Cin] -> out [N*OH*OW][Cout], both NHWC fp32.
int df_test_unet_block(df_ctx* c, const char* prefix, int kind, const float* x, const float* semb, const float* context,
                       float* out, int N, int H, int W, int Cin, int Cout, int T, void* stream) {
  return guard([&] {
    if (!c->has_unet || !c->finalized) fail("df_test_unet_block: load and finalize a UNet first");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const df_unet_config& u = c->ucfg;
    const std::string pre = "model.diffusion_model.", p = prefix;
    Plan plan;
    plan.poison = c->poison_on;
    Builder b{c, &plan, pre, 0};
    const int rows = N * H * W, temb = 4 * u.model_channels;
    F32 xin{b.buf<float>((size_t)rows * Cin), rows, Cin, Cin};
    HIPCHK(hipMemcpyAsync(xin.p, x, (size_t)rows * Cin * 4, hipMemcpyDeviceToDevice, s));
    int orow = rows;
    if (kind == 2) orow = rows / 4;
    if (kind == 3) orow = rows * 4;
    F32 dst{b.buf<float>((size_t)orow * Cout), orow, Cout, Cout};
    if (kind == 0) {
      float* E = b.buf<float>((size_t)N * Cout);
      const bf16_t* w = c->w_linear(pre + p + ".emb_layers.1.weight");
      const float* bb = c->f32(pre + p + ".emb_layers.1.bias");
      b.other("t.embproj", [=](hipStream_t st, const RunArgs&) { return launch_linear_rows(semb, temb, w, bb, E, Cout, N, Cout, temb, 0, st); });
      b.resblock(xin, dst, N, H, W, p + ".in_layers.0", p + ".in_layers.2", p + ".out_layers.0", p + ".out_layers.3",
                 p + ".skip_connection", 1e-5f, E, Cout, 0);
    } else if (kind == 1) {
      const int Dc = u.context_dim, ldvtc = rup(T, 32);
      bf16_t* ctxb = b.buf<bf16_t>((size_t)N * T * Dc);
      const long n = (long)N * T * Dc;
      b.other("ctx.cast", [=](hipStream_t st, const RunArgs&) { return launch_cast_bf16(context, ctxb, n, st); });
      if (Builder::px_ok(Cin, u.num_heads, T, H * W)) {     // same choice as build_unet_like
        Builder::PX px = b.context_px(ctxb, N, T, Dc, p, Cin, u.num_heads);
        b.spatial_transformer(xin, dst, N, H * W, p, u.num_heads, nullptr, nullptr, T, ldvtc, &px);
      } else {
        bf16_t *K, *Vt;
        b.context_kv(ctxb, N, T, Dc, p, Cin, &K, &Vt, ldvtc);
        b.spatial_transformer(xin, dst, N, H * W, p, u.num_heads, K, Vt, T, ldvtc);
      }
    } else {
      bf16_t* hb = b.cast2d(xin);
      const std::string wn = pre + p + (kind == 2 ? ".op" : ".conv");
      GemmParams g = kind == 3 ? Builder::gp_conv3_ups4(hb, N, H, W, Cin, c->w_conv3_ups4(wn + ".weight", Cin), Cout)   // as in the plan
                               : Builder::gp_conv3(hb, N, H, W, Cin, c->w_conv3(wn + ".weight", Cin), Cout, kind == 2 ? 2 : 1, 0);
      Builder::out_f32(g, dst.p, Cout);
      g.bias = c->f32(wn + ".bias");
      b.gemm(g, 1, kind == 2 ? "down" : "up");
    }
    finish_plan(c, &plan);
    RunArgs a;
    run_ops(c, &plan, 0, plan.ops.size(), s, a);
    HIPCHK(hipMemcpyAsync(out, dst.p, (size_t)orow * Cout * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
  });
}

// df_debug_poison checked against plans with a planted defect (include/df_engine.h): only Plan::alloc / release and the
// element-wise launchers, every access inside the plan's own blocks.
int df_test_poison_selftest(df_ctx* c, int defect, float* out_dev, void* stream) {
  return guard([&] {
    if (defect < 0 || defect > 2) fail("df_test_poison_selftest: defect %d (0 .. 2)", defect);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    constexpr int n = 1024, h = n / 2;
    Plan plan;
    plan.poison = c->poison_on;
    Builder b{c, &plan, "", 0};
    float* x = b.buf<float>(n);
    {
      std::vector<float> xh(n);
      for (int i = 0; i < n; ++i) xh[i] = (float)(i % 37 - 18) / 8.f;
      HIPCHK(hipMemcpy(x, xh.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
    auto lincomb = [&](const char* tag, float* out, const float* in0, float c0, const float* in1, float c1, long cnt) {
      b.other(tag, [=](hipStream_t st, const RunArgs&) {
        const float* in[2] = {in0, in1};
        const float coef[2] = {c0, c1};
        return launch_lincomb(out, in, coef, in1 ? 2 : 1, cnt, st);
      });
    };
    float* A = b.buf<float>(n);
    lincomb("self.a", A, x, 2.f, nullptr, 0.f, n);
    float* B = b.buf<float>(n);
    lincomb("self.b", B, A, 1.f, x, 1.f, n);
    plan.release(A);
    float* Cc = b.buf<float>(h);      // the freelist hands out A's block: n floats for a tenant of h
    if (Cc != A) fail("df_test_poison_selftest: the freelist did not recycle the released block");
    lincomb("self.c", Cc, B, 0.5f, defect == 2 ? Cc + h : nullptr, 1.f, h);
    float* o = b.buf<float>(h);
    lincomb("self.out", o, Cc, 1.f, defect == 1 ? A + h : B + h, 1.f, h);
    finish_plan(c, &plan);
    run_ops(c, &plan, 0, plan.ops.size(), s, RunArgs{});
    HIPCHK(hipMemcpyAsync(out_dev, o, h * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
  });
}

int df_test_conv3x3_fewout(const uint16_t* A, const uint16_t* W, const float* bias, float* out_nchw, int NB, int H, int Wd, int Cin,
                           int Cout, void* stream) {
  return guard([&] { HIPCHK(launch_conv3x3_fewout(A, W, bias, out_nchw, NB, H, Wd, Cin, Cout, (hipStream_t)stream)); });
}

int df_test_conv3x3_fewin(const float* x, const float* W, const float* bias, float* out, int ldo, int NB, int H, int Wd, int Cin, int Cout,
                          void* stream) {
  return guard([&] {
    if (!conv3x3_fewin_ok(H, Wd, Cin, Cout, ldo) || NB <= 0) fail("conv3x3_fewin: %d -> %d channels on %dx%d, ld %d is refused", Cin, Cout, H, Wd, ldo);
    HIPCHK(launch_conv3x3_fewin(x, W, bias, out, ldo, NB, H, Wd, Cin, Cout, (hipStream_t)stream));
  });
}

// the route conv3x3_fewin replaces: NCHW fp32 -> 64 operand-type channels, weights packed to [Cout][3][3][64], implicit GEMM on the
// tile Builder::gemm would choose (halo where it fits, else the cost model)
int df_test_conv3x3_fewin_gemm(const float* x, const float* W, const float* bias, float* out, uint16_t* xpad, uint16_t* wpad, int NB, int H,
                               int Wd, int Cin, int Cout, void* stream) {
  return guard([&] {
    hipStream_t s = (hipStream_t)stream;
    if (Cin < 1 || Cin > 64 || NB <= 0 || H <= 0 || Wd <= 0) fail("conv3x3_fewin_gemm: bad shape");
    HIPCHK(launch_pack_latent(x, xpad, NB, Cin, H * Wd, 64, 1, 1.0f, nullptr, nullptr, s));
    HIPCHK(launch_pack_conv_weight(W, wpad, Cout, Cin, 3, 3, 64, s));
    Plan pl;
    Builder b{nullptr, &pl, "", 0};
    GemmParams g = Builder::gp_conv3(xpad, NB, H, Wd, 64, wpad, Cout, 1, 0);
    Builder::out_f32(g, out, Cout);
    g.bias = bias;
    const Op& o = b.gemm(g, 1, "conv_in");
    GemmParams gp = o.gp;
    if (gp.splitk > 1) gp.partial = test_partial((size_t)gp.splitk * gp.M * gp.N * 4);
    test_launch_gemm(gp, o.tile, 1, s);
  });
}

int df_test_vae_encode_tap(df_ctx* c, const float* x, float* moments, float* tap_out, int tap, int B, int H, int W, void* stream) {
  return guard([&] {
    if (!c->has_vae_shape || !c->has_vae_enc) fail("vae encoder not configured");
    const int f = 1 << (c->vcfg.n_mult - 1);
    if (B <= 0 || B > 16 || H <= 0 || W <= 0 || H % f || W % f || tap < 0) fail("vae encode tap: bad shape %d x %dx%d / tap %d", B, H, W, tap);
    Plan* p = get_plan(c, keyf("vaeenc_tap%d_%d_%d_%d", tap, B, H, W), [&](Plan* pl) { build_vae_encoder(c, pl, B, H, W, tap); });
    RunArgs a;
    a.x = x;
    a.out = moments;
    a.out2 = tap_out;
    run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
  });
}

int df_test_cavp_spec_tap(df_ctx* c, const float* spec, float* out, void* tap_out, int tap, int B, int n_mels, int T, int normalize,
                          void* stream) {
  return guard([&] {
    if (!c->has_cavp_spec) fail("cavp spectrogram encoder not configured");
    if (B <= 0 || B > 16 || n_mels != c->scfg.n_mels || T < 16 || tap < 1 || tap > 6)
      fail("cavp spec tap: bad shape %d x %d x %d / tap %d", B, n_mels, T, tap);
    Plan* p = get_plan(c, keyf("cavpspec_tap%d_%d_%d_%d", tap, B, T, n_mels), [&](Plan* pl) { build_cavp_spec(c, pl, B, T, n_mels, tap); });
    RunArgs a;
    a.x = spec;
    a.out = out;
    a.out2 = (float*)tap_out;
    a.scale = normalize ? 1.f : 0.f;
    run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
  });
}

static GemmParams test_down_params(const uint16_t* A, const uint16_t* W, const float* bias, float* C, int NB, int H, int Wd, int Cin,
                                   int Cout, int pad, int splitk) {
  if (pad != 0 && pad != 1) fail("conv3x3_down: pad %d", pad);
  if (NB <= 0 || H <= 0 || Wd <= 0 || ((H | Wd) & 1)) fail("conv3x3_down: a positive even map, got %d x %dx%d", NB, H, Wd);
  GemmParams g = pad ? Builder::gp_conv3(A, NB, H, Wd, Cin, W, Cout, 2, 0) : Builder::gp_conv3_down_asym(A, NB, H, Wd, Cin, W, Cout);
  Builder::out_f32(g, C, Cout);
  g.bias = bias;
  g.splitk = splitk > 1 ? splitk : 1;
  return g;
}

int df_test_conv3x3_down(const uint16_t* A, const uint16_t* W, const float* bias, float* C, int NB, int H, int Wd, int Cin, int Cout,
                         int pad, int tile, int splitk, void* stream) {
  return guard([&] {
    GemmParams g = test_down_params(A, W, bias, C, NB, H, Wd, Cin, Cout, pad, splitk);
    if (g.K % 64 != 0 || g.Cin % 64 != 0) fail("conv3x3_down: Cin %d is not a multiple of 64", Cin);
    if (g.splitk > 1) g.partial = test_partial((size_t)g.splitk * g.M * g.N * 4);
    test_launch_gemm(g, tile, 1, (hipStream_t)stream);
  });
}

int df_test_conv3x3_down_valid(int NB, int H, int Wd, int Cin, int Cout, int pad, int tile, int splitk) {
  std::lock_guard<std::recursive_mutex> hold(g_api_lock);
  try {
    const GemmParams g = test_down_params(nullptr, nullptr, nullptr, nullptr, NB, H, Wd, Cin, Cout, pad, splitk);
    if (g.K % 64 != 0 || g.Cin % 64 != 0) return 0;
    return gemm_route(g, tile, 1, splitk, nullptr) ? 0 : 1;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 0;
  }
}

// Which kernel form a shape takes (host only; csrc/kernels.h groupnorm_route / attention_form -- the functions the launchers
// themselves dispatch on): tests/test_kernel_forms_cpu.py asserts that the GPU tests' shape tables reach every form.
int df_test_groupnorm_form(int N, int HW, int C, int nslab) { return groupnorm_form(N, HW, C, nslab); }
int df_test_attention_form(int D, int Tq, int Tk) { return attention_form(D, Tq, Tk); }

// GroupNorm in its three input modes with every leading dimension free: plain (nslab == 0), a split-K producer's slabs
// (nslab > 0: x is the first slab, + bias + rowbias) and the norm's own producer (own_slabs != null: df_test_groupnorm_own_slabs
// with ldo / raw_out).  raw_out rows are ldo wide like out's.  The arguments become the launcher's descriptor as they are.
int df_test_groupnorm_ex(float* x, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps, int silu,
                         uint16_t* out, int ldo, uint16_t* raw_out, int nslab, int64_t slab_stride, const float* bias,
                         const float* rowbias, int ld_rowbias, const float* own_slabs, int c_own, const float* res, int ldr,
                         void* stream) {
  return guard([&] {
    GroupNormArgs a;
    a.x = x; a.ld = ld; a.N = N; a.HW = HW; a.C = C; a.gamma = gamma; a.beta = beta; a.eps = eps; a.silu = silu;
    a.out = out; a.ldo = ldo; a.raw_out = raw_out;
    a.nslab = nslab; a.slab_stride = (long)slab_stride; a.bias = bias; a.rowbias = rowbias; a.ld_rowbias = ld_rowbias;
    a.own_slabs = own_slabs; a.c_own = c_own; a.res = res; a.ldr = ldr;
    a.scratch = test_partial(groupnorm_route(N, HW, C, nslab).scratch_bytes);
    HIPCHK(launch_groupnorm(a, (hipStream_t)stream));
  });
}
int df_test_groupnorm(const float* x, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps,
                      int silu, uint16_t* out, void* stream) {
  return df_test_groupnorm_ex(const_cast<float*>(x), ld, N, HW, C, gamma, beta, eps, silu, out, C, nullptr, 0, 0, nullptr, nullptr, 0,
                              nullptr, 0, nullptr, 0, stream);
}
int df_test_groupnorm_own_slabs(float* x, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps, int silu,
                                uint16_t* out, const float* slabs, int nslab, int c_own, const float* bias, const float* res,
                                int ldr, void* stream) {
  return df_test_groupnorm_ex(x, ld, N, HW, C, gamma, beta, eps, silu, out, C, nullptr, nslab, (int64_t)N * HW * c_own, bias, nullptr, 0,
                              slabs, c_own, res, ldr, stream);
}
int df_test_layernorm_ex(const float* x, int ld, int rows, int C, const float* gamma, const float* beta, uint16_t* out, void* stream) {
  return guard([&] { HIPCHK(launch_layernorm(x, ld, rows, C, gamma, beta, 1e-5f, out, (hipStream_t)stream)); });
}
int df_test_layernorm(const float* x, int rows, int C, const float* gamma, const float* beta, uint16_t* out, void* stream) {
  return df_test_layernorm_ex(x, C, rows, C, gamma, beta, out, stream);
}
int df_test_attention(const uint16_t* Q, int ldq, const uint16_t* K, int ldk, const uint16_t* Vt, int ldvt, uint16_t* O,
                      int ldo, int N, int heads, int D, int Tq, int Tk, float scale, void* stream) {
  return guard([&] { HIPCHK(launch_attention(Q, ldq, K, ldk, Vt, ldvt, O, ldo, N, heads, D, Tq, Tk, scale, (hipStream_t)stream)); });
}

// ---- the classifier's input-gradient kernels (csrc/backward.hip) one at a time
int df_test_groupnorm_bwd(const float* x, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps, int silu,
                          const float* dy, int lddy, const float* addend, int ldadd, float* dx, int lddx, uint16_t* dx_b16,
                          void* stream) {
  return guard([&] {
    HIPCHK(launch_groupnorm_bwd(x, ld, N, HW, C, gamma, beta, eps, silu, dy, lddy, addend, ldadd, dx, lddx, dx_b16,
                                (hipStream_t)stream));
  });
}
int df_test_layernorm_bwd(const float* x, int rows, int C, const float* gamma, float eps, const float* dy, const float* addend,
                          float* dx, uint16_t* dx_b16, void* stream) {
  return guard([&] { HIPCHK(launch_layernorm_bwd(x, rows, C, gamma, eps, dy, addend, dx, dx_b16, (hipStream_t)stream)); });
}
int df_test_geglu_fwd(const uint16_t* u, uint16_t* y, int64_t rows, int H, void* stream) {
  return guard([&] { HIPCHK(launch_geglu_fwd(u, y, (long)rows, H, (hipStream_t)stream)); });
}
int df_test_geglu_bwd(const uint16_t* u, const float* dy, uint16_t* du, int64_t rows, int H, void* stream) {
  return guard([&] { HIPCHK(launch_geglu_bwd(u, dy, du, (long)rows, H, (hipStream_t)stream)); });
}
int df_test_attention_bwd(const uint16_t* Q, int ldq, const uint16_t* K, int ldk, const uint16_t* Vt, int ldvt, const float* dO,
                          int lddo, uint16_t* dQ, int lddq, uint16_t* dK, int lddk, uint16_t* dV, int lddv, int N, int heads, int D,
                          int Tq, int Tk, float scale, int form, void* stream) {
  return guard([&] {
    size_t nws = attention_bwd_ws_floats(N, heads, D, Tq, Tk, lddk, lddv, dK != nullptr);
    if (form == 2 && dK) nws = (size_t)N * heads * Tq * 3;      // the tiled pair forced on a shape a resident form would take
    float* ws = nws ? test_partial(nws * 4) : nullptr;
    HIPCHK(launch_attention_bwd(Q, ldq, K, ldk, Vt, ldvt, dO, lddo, dQ, lddq, dK, lddk, dV, lddv, N, heads, D, Tq, Tk, scale, ws,
                                form, (hipStream_t)stream));
  });
}
int df_test_cls_head_bwd(const float* prob, const float* w, float* dh, uint16_t* dh_b16, int N, int HW, int C, int Cp, void* stream) {
  return guard([&] { HIPCHK(launch_cls_head_bwd(prob, w, dh, dh_b16, N, HW, C, Cp, (hipStream_t)stream)); });
}
int df_test_pack_linear_t(const float* w, uint16_t* out, int O, int I, int ldo, int off, void* stream) {
  return guard([&] { HIPCHK(launch_pack_linear_t(w, out, O, I, ldo, off, (hipStream_t)stream)); });
}
int df_test_pack_conv_bwd(const float* w, uint16_t* out, int O, int I, int Opad, void* stream) {
  return guard([&] { HIPCHK(launch_pack_conv_bwd(w, out, O, I, Opad, (hipStream_t)stream)); });
}
// Backward-data of a 3x3 conv (pad 1) exactly as build_classifier_grad issues it: W_oihw fp32 [O][I][3][3] packed here with
// Opad = O rounded up to 64 (dY: [NB][OH][OW][Opad], pad columns zero); stride 1 = conv of dY with the flipped taps, stride 2 = the
// same over the zero-stuffed x2 grid of dY (Downsample^T).  dX fp32 [NB][H][W][I] (+ the operand-type copy dX_op when given).
int df_test_conv3x3_bwd_data(const uint16_t* dY, const float* W_oihw, uint16_t* w_scratch, float* dX, uint16_t* dX_op, int NB, int H,
                             int Wd, int I, int O, int stride, int tile, int splitk, void* stream) {
  return guard([&] {
    if (stride != 1 && stride != 2) fail("conv3x3 backward-data: stride %d", stride);
    if (stride == 2 && ((H | Wd) & 1)) fail("conv3x3 backward-data: stride 2 needs an even map, got %dx%d", H, Wd);
    const int Opad = (O + 63) / 64 * 64;
    HIPCHK(launch_pack_conv_bwd(W_oihw, w_scratch, O, I, Opad, (hipStream_t)stream));
    GemmParams g = stride == 1 ? Builder::gp_conv3(dY, NB, H, Wd, Opad, w_scratch, I, 1, 0)
                               : Builder::gp_conv3(dY, NB, H / 2, Wd / 2, Opad, w_scratch, I, 1, 1);
    if (stride == 2) g.zstuff = 1;
    Builder::out_f32(g, dX, I);
    if (dX_op) {
      g.aux = dX_op;
      g.ld_aux = I;
    }
    g.splitk = splitk;
    if (splitk > 1) g.partial = test_partial((size_t)splitk * g.M * g.N * 4);
    test_launch_gemm(g, tile, 1, (hipStream_t)stream);
  });
}


// ---- the packing, casting, pooling and data-movement kernels one at a time (tests/test_small_kernels_gpu.py)
#define DF_TEST_LAUNCH(call) return guard([&] { HIPCHK(call); })
int df_test_softmax_rows(const float* s, uint16_t* p, int rows, int T, int ldp, void* stream) {
  DF_TEST_LAUNCH(launch_softmax_rows(s, p, rows, T, ldp, (hipStream_t)stream));
}
int df_test_timestep_embedding(const float* t, float* out, int N, int dim, void* stream) {
  DF_TEST_LAUNCH(launch_timestep_embedding(t, out, N, dim, (hipStream_t)stream));
}
int df_test_timestep_embedding_b16(const float* t, int t_B, uint16_t* out, int N, int dim, void* stream) {
  DF_TEST_LAUNCH(launch_timestep_embedding_b16(t, t_B, out, N, dim, (hipStream_t)stream));
}
int df_test_pack_latent(const float* x, uint16_t* out, int B, int C, int HW, int cpad, int rep, float in_scale, const float* wpq,
                        const float* bpq, void* stream) {
  DF_TEST_LAUNCH(launch_pack_latent(x, out, B, C, HW, cpad, rep, in_scale, wpq, bpq, (hipStream_t)stream));
}
int df_test_pack_latent_bcast(const float* x, uint16_t* out, int B, int C, int HW, int cpad, int rep, const float* src, float* dst,
                              int rows, int n, void* stream) {
  DF_TEST_LAUNCH(launch_pack_latent_bcast(x, out, B, C, HW, cpad, rep, src, dst, rows, n, (hipStream_t)stream));
}
int df_test_bcast_rows(const float* src, float* dst, int rows, int n, void* stream) {
  DF_TEST_LAUNCH(launch_bcast_rows(src, dst, rows, n, (hipStream_t)stream));
}
int df_test_cast_bf16(const float* x, uint16_t* out, int64_t n, void* stream) {
  DF_TEST_LAUNCH(launch_cast_bf16(x, out, (long)n, (hipStream_t)stream));
}
int df_test_cast_bf16_2d(const float* x, int ld, uint16_t* out, int64_t rows, int C, void* stream) {
  DF_TEST_LAUNCH(launch_cast_bf16_2d(x, ld, out, (long)rows, C, (hipStream_t)stream));
}
int df_test_avgpool(const float* x, float* out, int N, int HW, int C, void* stream) {
  DF_TEST_LAUNCH(launch_avgpool(x, out, N, HW, C, (hipStream_t)stream));
}
int df_test_pack_conv_weight(const float* w, uint16_t* out, int O, int I, int KH, int KW, int Ipad, void* stream) {
  DF_TEST_LAUNCH(launch_pack_conv_weight(w, out, O, I, KH, KW, Ipad, (hipStream_t)stream));
}
int df_test_pack_conv_skip(const float* w, const float* ws, uint16_t* out, int O, int I, int I2, void* stream) {
  DF_TEST_LAUNCH(launch_pack_conv_skip(w, ws, out, O, I, I2, (hipStream_t)stream));
}
int df_test_pack_geglu(const float* w, const float* b, uint16_t* wout, float* bout, int half_rows, int K, void* stream) {
  DF_TEST_LAUNCH(launch_pack_geglu(w, b, wout, bout, half_rows, K, (hipStream_t)stream));
}
int df_test_pack_ln_linear(const float* w, const float* bias, const float* gamma, const float* beta, uint16_t* wout, float* cs, float* bb,
                           int rows, int K, int row_off, int geglu_half, void* stream) {
  DF_TEST_LAUNCH(launch_pack_ln_linear(w, bias, gamma, beta, wout, cs, bb, rows, K, row_off, geglu_half, (hipStream_t)stream));
}
int df_test_grad_scale_per_sample(float* x, const float* prob, int N, int64_t per, void* stream) {
  DF_TEST_LAUNCH(launch_grad_scale_per_sample(x, prob, N, (long)per, (hipStream_t)stream));
}
int df_test_stem_im2col(const float* x, uint16_t* out, int F, int H, int W, int OH, int OW, int KP, void* stream) {
  DF_TEST_LAUNCH(launch_stem_im2col(x, out, F, H, W, OH, OW, KP, (hipStream_t)stream));
}
int df_test_maxpool3x3s2(const uint16_t* x, uint16_t* out, int F, int H, int W, int OH, int OW, int C, void* stream) {
  DF_TEST_LAUNCH(launch_maxpool3x3s2(x, out, F, H, W, OH, OW, C, (hipStream_t)stream));
}
int df_test_subsample2(const uint16_t* x, uint16_t* out, int F, int H, int W, int C, void* stream) {
  DF_TEST_LAUNCH(launch_subsample2(x, out, F, H, W, C, (hipStream_t)stream));
}
int df_test_tcat3(const uint16_t* x, uint16_t* out, int F, int T, int HW, int C, void* stream) {
  DF_TEST_LAUNCH(launch_tcat3(x, out, F, T, HW, C, (hipStream_t)stream));
}
int df_test_pack_conv3d_bn(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                           uint16_t* out, float* bias, int O, int I, int KT, int KH, int KW, int KP, void* stream) {
  DF_TEST_LAUNCH(launch_pack_conv3d_bn(w, gamma, beta, mean, var, eps, out, bias, O, I, KT, KH, KW, KP, (hipStream_t)stream));
}
int df_test_maxpool_time(const float* x, float* out, int B, int T, int C, int k, void* stream) {
  DF_TEST_LAUNCH(launch_maxpool_time(x, out, B, T, C, k, (hipStream_t)stream));
}
int df_test_l2norm_rows(float* x, int rows, int C, void* stream) {
  DF_TEST_LAUNCH(launch_l2norm_rows(x, rows, C, (hipStream_t)stream));
}
int df_test_spec_conv_in(const float* spec, const float* const* bn0, const float* w, const float* const* bn1, float eps, uint16_t* out,
                         int ldo, int B, int n_mels, int T, int C1, void* stream) {
  DF_TEST_LAUNCH(launch_spec_conv_in(spec, bn0, w, bn1, eps, out, ldo, B, n_mels, T, C1, (hipStream_t)stream));
}
int df_test_avgpool_nhwc(const float* x, int ldx, uint16_t* out, int ldo, int B, int H, int W, int C, int ph, int pw, void* stream) {
  DF_TEST_LAUNCH(launch_avgpool_nhwc(x, ldx, out, ldo, B, H, W, C, ph, pw, (hipStream_t)stream));
}
int df_test_spec_head_pool(const float* x, int ldx, uint16_t* out, int ldo, int B, int T, int W, int C, void* stream) {
  DF_TEST_LAUNCH(launch_spec_head_pool(x, ldx, out, ldo, B, T, W, C, (hipStream_t)stream));
}
#undef DF_TEST_LAUNCH

}  // extern "C"

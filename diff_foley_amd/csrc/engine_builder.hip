// libdfengine: the tile / split-K cost model and the plan Builder -- GEMM emission, norms, ResBlock, SpatialTransformer and the
// context operands (declarations and data layout: engine_internal.h).
#include "engine_internal.h"

DFE_NAMESPACE {

// ---------------------------------------------------------------------------------------------------------------
// Tile / split-K choice: a small cost model in MFMA cycles (256 CUs, one 32x32x16 MFMA per 8 cycles per CU).
static void choose_tile(int M, int N, int K, int batch, bool geglu, int* tile, int* splitk) {
  static const double eff[] = {1.0, 0.85, 0.85, 0.62, 0.55};      // the cost model knows the first five generic tiles
  constexpr int TILE_COUNT = sizeof(eff) / sizeof(eff[0]);
  static_assert(TILE_COUNT == TILE_32x128 + 1, "one efficiency per tile 128x128 .. 32x128");
  double best = 1e30;
  *tile = TILE_64x64;
  *splitk = 1;
  const int nk = K / 64;
  for (int c = 0; c < TILE_COUNT; ++c) {
    int bm, bn;
    gemm_tile_dims(c, &bm, &bn);
    if (bm > 64 && M <= bm / 2) continue;
    const long tiles = (long)cdiv(M, bm) * cdiv(N, bn) * batch;
    for (int sk = 1; sk <= 16; sk *= 2) {
      if (sk > 1 && (batch > 1 || nk / sk < 4)) break;
      const double work = (double)(bm / 32) * (bn / 32) * (double)cdiv(nk, sk) * 4.0 * 8.0 / eff[c] + 2500.0;
      const double rounds = (double)((tiles * sk + 255) / 256);
      double cost = rounds * work;
      if (sk > 1) cost += 9000.0 + (double)M * N * 8.0 * sk / 2000.0;   // reduce launch + slab traffic
      if (cost < best) {
        best = cost;
        *tile = c;
        *splitk = sk;
      }
    }
  }
}

void Builder::attach_aux(GemmParams& g, int rows, int C) {
  last_aux = nullptr;
  if (!want_aux) return;
  last_aux = buf<bf16_t>((size_t)rows * C);
  g.aux = last_aux;
  g.ld_aux = C;
  want_aux = false;
}

void Builder::forget_pend() {
  pend = Pend{};
  pl->unhold();
}

void Builder::other(const char* tag, std::function<hipError_t(hipStream_t, const RunArgs&)> fn) {
  Op o;
  o.fn = std::move(fn);
  o.tag = tag;
  pl->ops.push_back(std::move(o));
  // behind the push, as in gemm(): a held residual is read by THIS op when it is the GroupNorm that claimed the pending GEMM, so its
  // postponed release takes effect behind the op (the index df_debug_poison fills it at), not in front of it
  forget_pend();
}

void Builder::emits(const bf16_t* p, long rows, int cols, int ld) {
  if (p && !pl->ops.empty()) pl->ops.back().outs.push_back({p, rows, cols, ld});
}

Op& Builder::gemm(GemmParams gp, int batch, const char* tag) {
  Op o;
  o.is_gemm = true;
  o.batch = batch;
  o.tag = tag;
  int sk = 1;
  // the K loop of every GEMM kernel walks whole 64-element steps (gemm_impl.h: nk = K / 64): a ragged K would silently drop its tail
  if (gp.K % 64 != 0 || (gp.taps != 1 && gp.Cin % 64 != 0))
    fail("GEMM %s (%dx%dx%d, Cin %d): the contraction length must be a multiple of 64 (channel counts, context_dim and origin_dim "
         "that are not are outside what libdfengine builds)", tag, gp.M, gp.N, gp.K, gp.Cin);
  // batch-invariant plans (choice_NB): the choice is made for kChoiceBatch samples' rows (batched GEMMs: one matrix per sample)
  int Mc = gp.M, bc = batch;
  if (choice_NB > 0) {
    if (batch == 1 && gp.M % choice_NB == 0) Mc = gp.M / choice_NB * kChoiceBatch;
    if (batch > 1 && batch % choice_NB == 0) bc = batch / choice_NB * kChoiceBatch;
  }
  choose_tile(Mc, gp.N, gp.K, bc, gp.geglu != 0, &o.tile, &sk);
  if (gp.taps == 9 && gemm_tile_valid(gp, TILE_HALO_128x64, batch, 1)) {   // halo reuse beats re-fetching A per tap
    o.tile = TILE_HALO_128x64;
    const long blocks = (long)((Mc + 127) / 128) * ((gp.N + 63) / 64);
    sk = 1;
    while (blocks * sk < 160 && sk < 16 && gp.Cin / 64 / (sk * 2) >= 2) sk *= 2;
  }
  if (!gemm_tile_valid(gp, o.tile, batch, sk)) {   // epilogue features narrow the tile set: 64x64, no split-K always runs
    o.tile = TILE_64x64;
    sk = 1;
    if (!gemm_tile_valid(gp, o.tile, batch, sk)) fail("no valid tile for GEMM %s (%dx%dx%d)", tag, gp.M, gp.N, gp.K);
  }
  gp.splitk = sk;
  if (sk > 1) {
    const size_t need = (size_t)sk * gp.M * gp.N * 4 * (gp.taps == 4 ? 4 : 1);
    if (need > pl->partial_bytes) pl->partial_bytes = need;
  }
  gp.dbg = getenv("DF_GEMM_DBG") ? atoi(getenv("DF_GEMM_DBG")) : 0;   // tools only (timing experiments)
  o.gp = gp;
  pl->gemm_flops += 2.0 * gp.M * (double)gp.N * gp.K * batch * (gp.taps == 4 ? 4 : 1);
  pl->weight_bytes += 2.0 * (double)gp.N * gp.K * (gp.w_bs ? batch : 1);
  pl->ops.push_back(std::move(o));
  forget_pend();
  if (batch == 1 && gp.C && !gp.out_bf16 && !gp.aux && !gp.dup_rows && !gp.stats && !gp.ln_stats && !gp.geglu && !gp.vt &&
      !gp.rowbias && !gp.store_nchw && !gp.relu && !gp.silu && !gp.no_c_store && gp.alpha == 1.f && gp.taps != 4 &&
      gp.sm_w == 0 && (gp.N & 3) == 0)
  {
    pend = Pend{(long)pl->ops.size() - 1, (const float*)gp.C, gp.ldc, gp.N, gp.M};
    pl->held = gp.res;       // the claiming norm reads the residual while it writes its own (freshly allocated) outputs
  }
  return pl->ops.back();
}

unsigned Builder::op_bytes(size_t b) {
  if (b >= ((size_t)1 << 31)) fail("GEMM operand of %zu bytes exceeds the 2 GiB buffer-addressing limit (split the batch)", b);
  return (unsigned)b;
}

GemmParams Builder::gp_linear(const bf16_t* A, int M, int K, const bf16_t* W, int N) {
  GemmParams g{};
  g.A = A; g.lda = K; g.W = W; g.M = M; g.N = N; g.K = K;
  g.taps = 1; g.Cin = K; g.alpha = 1.f; g.stride = 1;
  g.a_bytes = op_bytes((size_t)M * K * 2); g.w_bytes = op_bytes((size_t)N * K * 2);
  return g;
}

GemmParams Builder::gp_conv3(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W, int Cout, int stride,
                             int ups) {
  GemmParams g{};
  g.A = A; g.lda = Cin; g.W = W;
  g.H = H; g.Wd = Wd; g.stride = stride; g.ups = ups;
  g.OH = ups ? 2 * H : (stride == 2 ? H / 2 : H);
  g.OW = ups ? 2 * Wd : (stride == 2 ? Wd / 2 : Wd);
  g.M = NB * g.OH * g.OW; g.N = Cout; g.K = 9 * Cin;
  g.taps = 9; g.Cin = Cin; g.alpha = 1.f; g.pad = 1;
  g.a_bytes = op_bytes((size_t)NB * H * Wd * Cin * 2); g.w_bytes = op_bytes((size_t)Cout * 9 * Cin * 2);
  return g;
}

GemmParams Builder::gp_conv3_down_asym(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W, int Cout) {
  if ((H | Wd) & 1) fail("asymmetric Downsample conv: the %dx%d map is not even", H, Wd);
  GemmParams g = gp_conv3(A, NB, H, Wd, Cin, W, Cout, 2, 0);
  g.pad = 0;
  return g;
}

GemmParams Builder::gp_conv3_ups4(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W4, int Cout) {
  GemmParams g{};
  g.A = A; g.lda = Cin; g.W = W4;
  g.H = H; g.Wd = Wd; g.stride = 1; g.ups = 0;
  g.OH = H; g.OW = Wd;                       // row grid of the GEMM (the output map is 2H x 2W)
  g.M = NB * H * Wd; g.N = Cout; g.K = 4 * Cin;
  g.taps = 4; g.Cin = Cin; g.alpha = 1.f;
  g.w_bs = (long)Cout * 4 * Cin;
  g.a_bytes = op_bytes((size_t)NB * H * Wd * Cin * 2); g.w_bytes = op_bytes((size_t)Cout * 4 * Cin * 2);
  return g;
}

void Builder::add_a2(GemmParams& g, const bf16_t* A2, int lda2, int Cin2) {
  g.A2 = A2; g.lda2 = lda2; g.Cin2 = Cin2;
  g.a2_bytes = op_bytes(((size_t)(g.M - 1) * lda2 + Cin2) * 2);
  g.K += Cin2;
  g.w_bytes = op_bytes((size_t)g.N * g.K * 2);
}

// The one place a plan emits a GroupNorm: asks the route (csrc/kernels.h), allocates the scratch that route wants, pushes the op,
// records its outputs and releases the scratch.  feed != GnFeed::none: the GEMM at ops[prod] may be tuned to split-K AFTER the build,
// so where the register kernels hold this shape its reduce is left to the norm (Op::defer) and every launch looks at the producer
// again: split-K -> the slab fields of its own copy of the descriptor are filled in, otherwise the plain norm runs.
void Builder::emit_groupnorm(GroupNormArgs a, GnFeed feed, size_t prod, const float* rowbias, int ld_rowbias) {
  const size_t sb = groupnorm_route(a.N, a.HW, a.C, 0).scratch_bytes;
  if (feed != GnFeed::none && groupnorm_route(a.N, a.HW, a.C, 1).form == GN_FORM_REFUSED) feed = GnFeed::none;
  if (feed != GnFeed::none) pl->ops[prod].defer = true;
  a.scratch = sb ? (float*)pl->alloc(sb) : nullptr;
  Plan* plp = pl;
  other("groupnorm", [=](hipStream_t s, const RunArgs&) {
    if (feed == GnFeed::none) return launch_groupnorm(a, s);
    const GemmParams& gp = plp->ops[prod].gp;
    if (!plp->ops[prod].defer || gp.splitk <= 1) return launch_groupnorm(a, s);
    GroupNormArgs g = a;
    g.nslab = gp.splitk;
    g.slab_stride = (long)gp.M * gp.N;
    g.bias = gp.bias;
    if (feed == GnFeed::input_slabs) {      // the producer's output has this norm as its ONE reader: it is never written
      g.x = gp.partial;
      g.rowbias = rowbias;
      g.ld_rowbias = ld_rowbias;
    } else {                                // own slabs: this norm finishes x (bias + residual, in the reduce kernel's order) and writes it back
      g.own_slabs = gp.partial;
      g.c_own = gp.N;
      g.res = gp.res;
      g.ldr = gp.ldr;
    }
    return launch_groupnorm(g, s);
  });
  emits(a.out, (long)a.N * a.HW, a.C, a.ldo);
  emits(a.raw_out, (long)a.N * a.HW, a.C, a.ldo);
  pl->release(a.scratch);
}

bf16_t* Builder::groupnorm(const F32& x, int NB, const std::string& p, float eps, int silu, bf16_t** raw) {
  bf16_t* o = buf<bf16_t>((size_t)x.rows * x.C);
  bf16_t* r = raw ? buf<bf16_t>((size_t)x.rows * x.C) : nullptr;
  if (raw) *raw = r;
  GroupNormArgs a;
  a.x = x.p; a.ld = x.ld; a.N = NB; a.HW = x.rows / NB; a.C = x.C;
  a.gamma = c->f32(nm(p + ".weight")); a.beta = c->f32(nm(p + ".bias")); a.eps = eps; a.silu = silu;
  a.out = o; a.ldo = x.C; a.raw_out = r;
  // x straight out of a GEMM that may run split-K (a ResBlock's conv2, a SpatialTransformer's merged FF2 + proj_out, a
  // Downsample conv): this norm is its first reader, so it does the reduce -- sums the slabs, adds bias + residual, writes
  // x back -- in the launch it needs anyway; the producer's reduce launch and one fp32 round trip of x disappear.
  static const bool no_own = getenv("DF_NO_GNOWN") && atoi(getenv("DF_NO_GNOWN"));
  const Pend pd = pend;
  const bool claim = !no_own && pd.op >= 0 && pd.p == x.p && pd.ld == x.ld && pd.rows == x.rows && pd.C <= x.C && (pd.C & 1) == 0 &&
                     (x.ld & 1) == 0;
  emit_groupnorm(a, claim ? GnFeed::own_slabs : GnFeed::none, claim ? (size_t)pd.op : 0, nullptr, 0);
  return o;
}

void Builder::layernorm(const F32& x, const std::string& p, bf16_t* o) {
  const float* g = c->f32(nm(p + ".weight"));
  const float* b = c->f32(nm(p + ".bias"));
  const float* xp = x.p;
  const int ld = x.ld, rows = x.rows, C = x.C;
  other("layernorm", [=](hipStream_t s, const RunArgs&) { return launch_layernorm(xp, ld, rows, C, g, b, 1e-5f, o, s); });
  emits(o, rows, C, C);
}

bf16_t* Builder::cast2d(const F32& x) {
  if (x.b16) return x.b16;      // the producer already wrote the operand copy: no cast launch
  bf16_t* o = buf<bf16_t>((size_t)x.rows * x.C);
  const float* xp = x.p;
  const int ld = x.ld, C = x.C;
  const long rows = x.rows;
  other("cast", [=](hipStream_t s, const RunArgs&) { return launch_cast_bf16_2d(xp, ld, o, rows, C, s); });
  emits(o, rows, C, C);
  return o;
}

void Builder::resblock(const F32& x, const F32& out, int NB, int H, int Wd, const std::string& n1, const std::string& c1,
                       const std::string& n2, const std::string& c2, const std::string& skip, float eps,
                       const float* emb, int emb_ld, int emb_col, int dup_rows) {
  const int cin = x.C, cout = out.C, M = x.rows;
  const bool has_skip = c->has(nm(skip + ".weight"));
  if (!has_skip && cin != cout) fail("resblock %s: channel change without skip conv", nm(c1).c_str());
  bf16_t* xraw = nullptr;
  bf16_t* a1 = groupnorm(x, NB, n1, eps, 1, has_skip ? &xraw : nullptr);
  float* h1 = buf<float>((size_t)M * cout);
  {
    GemmParams g = gp_conv3(a1, NB, H, Wd, cin, c->w_conv3(nm(c1 + ".weight"), cin), cout, 1, 0);
    out_f32(g, h1, cout);
    g.bias = c->f32(nm(c1 + ".bias"));
    if (emb) {
      g.rowbias = emb + emb_col; g.ld_rowbias = emb_ld; g.rows_per_sample = H * Wd; g.rowbias_mode = 1;
    }
    gemm(g, 1, "res.conv1");
  }
  pl->release(a1);
  // h1 has ONE consumer, the second GroupNorm.  When conv1 runs split-K, its reduce launch is dropped: the norm sums
  // the partial slabs while loading and adds the bias / FiLM bias itself (no reduce kernel, no fp32 round trip of h1).
  const size_t ci = pl->ops.size() - 1;
  bf16_t* a2 = buf<bf16_t>((size_t)M * cout);
  {
    GroupNormArgs a;
    a.x = h1; a.ld = cout; a.N = NB; a.HW = H * Wd; a.C = cout;
    a.gamma = c->f32(nm(n2 + ".weight")); a.beta = c->f32(nm(n2 + ".bias")); a.eps = eps; a.silu = 1;
    a.out = a2; a.ldo = cout;
    emit_groupnorm(a, GnFeed::input_slabs, ci, emb ? emb + emb_col : nullptr, emb_ld);
  }
  pl->release(h1);
  {
    GemmParams g = gp_conv3(a2, NB, H, Wd, cout, c->w_conv3(nm(c2 + ".weight"), cout), cout, 1, 0);
    out_f32(g, out.p, out.ld);
    g.bias = c->f32(nm(c2 + ".bias"));
    if (has_skip) {
      // skip(x) + conv2(h) as ONE implicit GEMM: the 1x1 skip conv is a tenth K range over the raw operand copy of x
      const bf16_t* w;
      const float* bsum;
      c->w_conv3_skip(nm(c2), nm(skip), &w, &bsum);
      g.W = w;
      g.bias = bsum;
      add_a2(g, xraw, cin, cin);
    } else { g.res = x.p; g.ldr = x.ld; }
    attach_aux(g, M, cout);
    g.dup_rows = dup_rows;       // CFG prefix: this block ran on one half of the batch, its output feeds both
    gemm(g, 1, "res.conv2");
  }
  if (has_skip) pl->release(xraw);
  pl->release(a2);
}

void Builder::spatial_transformer(const F32& x, const F32& out, int NB, int T, const std::string& p, int heads,
                                  const bf16_t* ctxK, const bf16_t* ctxVt, int Tc, int ldvtc, const PX* px,
                                  bool cfg_prefix) {
  const int C = x.C, M = x.rows, D = C / heads;
  if (cfg_prefix && (T % 4 != 0 || NB % 2 != 0)) fail("cfg prefix needs the fused QKV form");
  const int Mp = cfg_prefix ? M / 2 : M, NBp = cfg_prefix ? NB / 2 : NB;     // rows / samples of the deduplicated prefix
  if (!attention_supported(D)) fail("unsupported attention head dim %d", D);
  const std::string tb = p + ".transformer_blocks.0";
  const float scale = 1.0f / sqrtf((float)D);
  bf16_t* a = groupnorm(F32{x.p, Mp, C, x.ld}, NBp, p + ".norm", 1e-6f, 0, nullptr);
  float* t0 = buf<float>((size_t)M * C);        // fp32 residual stream of the transformer block
  F32 t0v{t0, M, C, C};
  bf16_t* xb = buf<bf16_t>((size_t)M * C);      // its operand-type copy (A operand of the LayerNorm-folded GEMMs)
  const int slots = C / 64;
  float2* st = buf<float2>((size_t)M * slots);  // per-row (sum, sumsq) partials per 64-column slot of t0
  // The three pre-norm LayerNorms (attention_openai.py:211-215) never run as kernels: the producer of t0 emits the
  // row statistics from its epilogue, the consumer GEMM multiplies the RAW operand copy by gamma-scaled weights and
  // its epilogue applies  rstd * (acc - mean * colsum) + (beta.W + b).
  auto produces_t0 = [&](GemmParams& g) {
    out_f32(g, t0, C);
    g.aux = xb; g.ld_aux = C;
    g.stats = st; g.stats_slots = slots;
  };
  auto ln_fold = [&](GemmParams& g, const float* cs, const float* bb) {
    g.ln_stats = st; g.ln_slots = slots; g.ln_C = C; g.ln_eps = 1e-5f; g.ln_cs = cs;
    g.bias = bb;
  };
  {
    GemmParams g = gp_linear(a, Mp, C, c->w_linear(nm(p + ".proj_in.weight")), C);
    produces_t0(g);
    g.bias = c->f32(nm(p + ".proj_in.bias"));
    gemm(g, 1, "st.proj_in");
  }
  // ---- self attention: one GEMM for Q | K | V; the V third leaves transposed (V^T[n][c][t]) from the epilogue
  bf16_t* qk = buf<bf16_t>((size_t)M * 2 * C);
  const int ldvt = rup(T, 32);
  bf16_t* vt = buf<bf16_t>((size_t)NB * C * ldvt);
  const bool fuse_v = (T % 4 == 0);           // the transposed store moves 4 tokens of one sample per lane
  bf16_t* o_own = nullptr;
  if (!fuse_v) {   // 1- or 2-token maps (8x8 / 8x16 latents at ds 8): LayerNorm kernel + separate K|Q and V^T GEMMs
    layernorm(t0v, tb + ".norm1", a);
    {
      const bf16_t* w = c->w_stack(nm(tb + ".attn1.qk"), {nm(tb + ".attn1.to_q.weight"), nm(tb + ".attn1.to_k.weight")});
      GemmParams g = gp_linear(a, M, C, w, 2 * C);
      out_b16(g, qk, 2 * C);
      gemm(g, 1, "st.qk");
    }
    {  // V^T[n] = Wv . a[n]^T  (batched: A = Wv shared, "W" operand = this sample's tokens)
      GemmParams g = gp_linear(c->w_linear(nm(tb + ".attn1.to_v.weight")), C, C, a, T);
      g.w_bs = (long)T * C;
      out_b16(g, vt, ldvt);
      g.c_bs = (long)C * ldvt;
      gemm(g, NB, "st.vT");
    }
    o_own = buf<bf16_t>((size_t)M * C);
  } else {
    const bf16_t* w;
    const float *cs, *bb;
    c->w_ln_stack(nm(tb + ".attn1.qkv"), nm(tb + ".norm1"),
                  {nm(tb + ".attn1.to_q.weight"), nm(tb + ".attn1.to_k.weight"), nm(tb + ".attn1.to_v.weight")}, {}, false,
                  &w, &cs, &bb);
    GemmParams g = gp_linear(xb, Mp, C, w, 3 * C);
    out_b16(g, qk, 2 * C);
    ln_fold(g, cs, bb);
    g.vt = vt; g.vt_col0 = 2 * C; g.vt_T = T; g.ldvt = ldvt;
    gemm(g, 1, "st.qkv");
  }
  bf16_t* o = o_own ? o_own : a;                 // GroupNorm output is dead after proj_in
  other("attn.self", [=](hipStream_t s, const RunArgs&) {
    return launch_attention(qk, 2 * C, qk + C, 2 * C, vt, ldvt, o, C, NBp, heads, D, T, T, scale, s);
  });
  emits(o, Mp, C, C);
  {
    GemmParams g = gp_linear(o, Mp, C, c->w_linear(nm(tb + ".attn1.to_out.0.weight")), C);
    produces_t0(g);
    g.bias = c->f32(nm(tb + ".attn1.to_out.0.bias"));
    g.res = t0; g.ldr = C;
    g.dup_rows = cfg_prefix ? Mp : 0;           // t0 / xb / statistics of BOTH halves of the CFG batch from here on
    gemm(g, 1, "st.attn1.out");
  }
  // ---- cross attention
  if (px && px->G) {
    // the context-dependent half was folded into per-sample operands by set_context (context_px): scores + softmax in one
    // LayerNorm-folded GEMM (N = heads * 32), then probabilities x (Wo V^T) with the residual / statistics epilogue
    const int HT = px->HT;
    bf16_t* pr = qk;                               // [M][HT] probabilities (qk holds M x 2C >= M x HT elements)
    if ((size_t)HT > (size_t)2 * C) fail("cross-attention: %d probability columns do not fit the q|k buffer", HT);
    {
      GemmParams g = gp_linear(xb, M, C, px->G, HT);
      g.w_bs = (long)HT * C; g.w_rows = T;
      g.w_bytes = op_bytes((size_t)HT * C * 2);
      out_b16(g, pr, HT);
      ln_fold(g, px->cs, px->bb);
      g.sm_w = 32; g.sm_valid = Tc;
      gemm(g, 1, "st.xs");
    }
    {
      GemmParams g = gp_linear(pr, M, HT, px->Vo, C);
      g.w_bs = (long)C * HT; g.w_rows = T;
      g.w_bytes = op_bytes((size_t)C * HT * 2);
      produces_t0(g);
      // nobody reads the fp32 residual stream after this op on the merged-FF path (FF1 and ffproj consume the operand
      // copy + row statistics, the block residual is x): the epilogue skips the fp32 store
      g.no_c_store = 1;
      g.bias = c->f32(nm(tb + ".attn2.to_out.0.bias"));
      g.res = t0; g.ldr = C;
      gemm(g, 1, "st.xo");
    }
  } else {
  // (K / V^T of the context were computed by set_context)
  bf16_t* q2 = qk;
  {
    const bf16_t* w;
    const float *cs, *bb;
    c->w_ln_stack(nm(tb + ".attn2.q"), nm(tb + ".norm2"), {nm(tb + ".attn2.to_q.weight")}, {}, false, &w, &cs, &bb);
    GemmParams g = gp_linear(xb, M, C, w, C);
    out_b16(g, q2, C);
    ln_fold(g, cs, bb);
    gemm(g, 1, "st.q2");
  }
  other("attn.cross", [=](hipStream_t s, const RunArgs&) {
    return launch_attention(q2, C, ctxK, C, ctxVt, ldvtc, o, C, NB, heads, D, T, Tc, scale, s);
  });
  emits(o, M, C, C);
  {
    GemmParams g = gp_linear(o, M, C, c->w_linear(nm(tb + ".attn2.to_out.0.weight")), C);
    produces_t0(g);
    g.bias = c->f32(nm(tb + ".attn2.to_out.0.bias"));
    g.res = t0; g.ldr = C;
    gemm(g, 1, "st.attn2.out");
  }
  }
  pl->release(qk);
  pl->release(vt);
  // ---- GEGLU feed-forward
  bf16_t* gl = buf<bf16_t>((size_t)M * 4 * C);
  {
    const bf16_t* w;
    const float *cs, *bb;
    c->w_ln_stack(nm(tb + ".ff.net.0.proj"), nm(tb + ".norm3"), {nm(tb + ".ff.net.0.proj.weight")},
                  {nm(tb + ".ff.net.0.proj.bias")}, true, &w, &cs, &bb);
    GemmParams g = gp_linear(xb, M, C, w, 8 * C);
    out_b16(g, gl, 4 * C);
    ln_fold(g, cs, bb);
    g.geglu = 1;
    if ((8 * C) % 320 == 0) {      // the wide tiles' packing of the same operand (TILE_WGEGLU_*; the tuner decides who runs)
      const bf16_t* w3;
      const float *cs3, *bb3;
      c->w_ln_w320(nm(tb + ".ff.net.0.proj"), 8 * C, C, &w3, &cs3, &bb3);
      g.W_w320 = w3; g.cs_w320 = cs3; g.bias_w320 = bb3;
    }
    gemm(g, 1, "st.ff1");
  }
  {
    // FF's second Linear, the residual add and proj_out are ONE linear map of (h, t): proj_out(t + W2 h + b2) =
    // (Wp W2) h + Wp t + (Wp b2 + bp).  One GEMM with K = 4C + C over two A tensors -- the GEGLU output and the operand
    // copy of the residual stream -- with the same FLOPs as the pair it replaces and one launch fewer per block.
    const bf16_t* w;
    const float* bsum;
    c->w_ffproj(nm(tb + ".ff.net.2"), nm(p + ".proj_out"), &w, &bsum);
    GemmParams g = gp_linear(gl, M, 4 * C, w, C);
    add_a2(g, xb, C, C);
    out_f32(g, out.p, out.ld);
    g.bias = bsum;
    g.res = x.p; g.ldr = x.ld;
    attach_aux(g, M, C);
    gemm(g, 1, "st.ffproj");
  }
  pl->release(gl);
  pl->release(a);
  pl->release(t0);
  pl->release(xb);
  pl->release(st);
  pl->release(o_own);
}

bool Builder::px_ok(int C, int heads, int Tc, int tokens) {
  const bool off = getenv("DF_NO_XPRE") && atoi(getenv("DF_NO_XPRE"));     // read per plan build: tests A/B both forms
  return !off && Tc >= 1 && Tc <= 32 && C % 64 == 0 && C % heads == 0 && (C / heads) % 8 == 0 && (heads * 32) % 64 == 0 &&
         tokens % 64 == 0;
}

// Cross-attention with the context folded into per-sample "weights".  The context is fixed for a whole sample() call while
// the queries change every step, so everything that does not depend on the query is precomputed by set_context:
//   scores_h = LN(t) Wq_h^T K_h^T / sqrt(D) = LN(t) . G_h,   G = [G_0 .. G_H-1]  ([C] x [H*32] per sample, LayerNorm-folded)
//   out      = sum_h P_h V_h Wo_h^T + bo   = P . Vo,          Vo = [Wo_h V_h^T]_h ([H*32] x [C] per sample)
// which turns  q-projection -> attention kernel -> out-projection  (2 M C^2 + 2 M C^2 FLOPs, 3 launches) into two GEMMs
// of 2 M C (32 H) FLOPs each with a softmax in the first one's epilogue (context length <= 32: padded to 32 per head).
Builder::PX Builder::context_px(const bf16_t* ctx, int NB, int Tc, int Dc, const std::string& st_prefix, int C, int heads) {
  const std::string tb = st_prefix + ".transformer_blocks.0", a2 = tb + ".attn2";
  const int HT = heads * 32;
  const float scale = 1.0f / sqrtf((float)(C / heads));
  PX px;
  px.HT = HT;
  bf16_t* kvb = buf<bf16_t>((size_t)NB * Tc * 2 * C);
  {
    const bf16_t* w = c->w_stack(nm(a2 + ".kv"), {nm(a2 + ".to_k.weight"), nm(a2 + ".to_v.weight")});
    GemmParams g = gp_linear(ctx, NB * Tc, Dc, w, 2 * C);
    out_b16(g, kvb, 2 * C);
    gemm(g, 1, "ctx.kv");
  }
  bf16_t* Kexp = buf<bf16_t>((size_t)NB * HT * C);
  bf16_t* Vexp = buf<bf16_t>((size_t)NB * HT * C);
  other("ctx.expand", [=](hipStream_t s, const RunArgs&) { return launch_xattn_expand(kvb, Kexp, Vexp, NB, Tc, 32, C, heads, s); });
  bf16_t* G = buf<bf16_t>((size_t)NB * HT * C);
  {
    GemmParams g = gp_linear(Kexp, NB * HT, C, c->w_lnq_t(nm(a2 + ".to_q.weight"), nm(tb + ".norm2"), scale), C);
    out_b16(g, G, C);
    gemm(g, 1, "ctx.g");
  }
  float* cs = buf<float>((size_t)NB * HT);
  float* bb = buf<float>((size_t)NB * HT);
  {
    const bf16_t* wq;
    const float *csq, *bq;
    c->w_ln_stack(nm(tb + ".attn2.q"), nm(tb + ".norm2"), {nm(a2 + ".to_q.weight")}, {}, false, &wq, &csq, &bq);
    const long rows = (long)NB * HT;
    other("ctx.gstats", [=](hipStream_t s, const RunArgs&) { return launch_xattn_rowstats(G, Kexp, bq, scale, C, rows, cs, bb, s); });
  }
  bf16_t* Vo = buf<bf16_t>((size_t)NB * C * HT);
  {  // Vo[n] = Wo . Vexp[n]^T  (batched: A = Wo shared, "W" operand = this sample's expanded values)
    GemmParams g = gp_linear(c->w_linear(nm(a2 + ".to_out.0.weight")), C, C, Vexp, HT);
    g.w_bs = (long)HT * C;
    out_b16(g, Vo, HT);
    g.c_bs = (long)C * HT;
    gemm(g, NB, "ctx.vo");
  }
  // kvb / Kexp / Vexp stay allocated: set_context re-runs these ops for every new context
  px.G = G; px.cs = cs; px.bb = bb; px.Vo = Vo;
  return px;
}

// context -> per-ST K [NB*Tc][C] and V^T [NB][C][ldvt]
void Builder::context_kv(const bf16_t* ctx, int NB, int Tc, int Dc, const std::string& st_prefix, int C, bf16_t** K,
                         bf16_t** Vt, int ldvt) {
  const std::string a2 = st_prefix + ".transformer_blocks.0.attn2";
  *K = buf<bf16_t>((size_t)NB * Tc * C);
  *Vt = buf<bf16_t>((size_t)NB * C * ldvt);
  {
    GemmParams g = gp_linear(ctx, NB * Tc, Dc, c->w_linear(nm(a2 + ".to_k.weight")), C);
    out_b16(g, *K, C);
    gemm(g, 1, "ctx.k");
  }
  {
    GemmParams g = gp_linear(c->w_linear(nm(a2 + ".to_v.weight")), C, Dc, ctx, Tc);
    g.w_bs = (long)Tc * Dc;
    out_b16(g, *Vt, ldvt);
    g.c_bs = (long)C * ldvt;
    gemm(g, NB, "ctx.vT");
  }
}

// ---- shared front of build_unet_like and build_classifier_grad
// the context cast to the operand type, first op of both plans
bf16_t* Builder::context_cast(int N, int Tc, int Dc) {
  bf16_t* ctxb = buf<bf16_t>((size_t)N * Tc * Dc);
  const long n = (long)N * Tc * Dc;
  other("ctx.cast", [=](hipStream_t s, const RunArgs& a) { return launch_cast_bf16(a.aux, ctxb, n, s); });
  return ctxb;
}
void Builder::context_kv_for(const bf16_t* ctx, int NB, int Tc, int Dc, const BlockDesc& d, int ldvt, KV& kv) {
  bf16_t *K, *Vt;
  context_kv(ctx, NB, Tc, Dc, d.prefix, d.cin, &K, &Vt, ldvt);
  kv[d.prefix] = {K, Vt};
}
// the emb projections of every ResBlock stacked into one operand / one bias (column offsets: build_emb_table)
void Builder::emb_proj_operands(const UNetTopo& topo, const bf16_t** w, const float** bb) {
  std::vector<std::string> wn, bn;
  for (auto& r : topo_resblocks(topo)) {
    wn.push_back(pre + r + ".emb_layers.1.weight");
    bn.push_back(pre + r + ".emb_layers.1.bias");
  }
  *w = c->w_stack(pre + "#embw", wn);
  *bb = c->b_stack(pre + "#embb", bn);
}
int Builder::checked_in_channels(const df_unet_config& u) {
  const int cin = u.in_channels;
  if (cin < 1 || cin > 64) fail("in_channels = %d: the first conv's operand is one 64-channel K step (1 .. 64 input channels)", cin);
  return cin;
}

}  // namespace dfe

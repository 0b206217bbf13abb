// libdfengine: UNet topology and the forward plans of the four networks -- UNet / classifier backbone, VAE decoder, cond stage,
// VAE encoder, CAVP video encoder, CAVP spectrogram encoder (types and the Builder: engine_internal.h).
#include "engine_internal.h"

DFE_NAMESPACE {


UNetTopo make_topo(const df_unet_config& u, bool encoder_only) {
  UNetTopo t;
  const int mc = u.model_channels;
  auto in_attn = [&](int ds) {
    for (int i = 0; i < u.n_attn; ++i)
      if (u.attention_resolutions[i] == ds) return true;
    return false;
  };
  t.input.push_back({{BlockDesc::CONV_IN, "input_blocks.0.0", u.in_channels, mc}});
  t.in_ch.push_back(mc);
  t.in_ds.push_back(1);
  int ch = mc, ds = 1, idx = 1;
  for (int level = 0; level < u.n_mult; ++level) {
    for (int r = 0; r < u.num_res_blocks; ++r) {
      std::vector<BlockDesc> b;
      const int co = u.channel_mult[level] * mc;
      b.push_back({BlockDesc::RES, "input_blocks." + std::to_string(idx) + ".0", ch, co});
      ch = co;
      if (in_attn(ds)) b.push_back({BlockDesc::ST, "input_blocks." + std::to_string(idx) + ".1", ch, ch, ds});
      t.input.push_back(b);
      t.in_ch.push_back(ch);
      t.in_ds.push_back(ds);
      ++idx;
    }
    if (level != u.n_mult - 1) {
      t.input.push_back({{BlockDesc::DOWN, "input_blocks." + std::to_string(idx) + ".0", ch, ch}});
      ds *= 2;
      t.in_ch.push_back(ch);
      t.in_ds.push_back(ds);
      ++idx;
    }
  }
  t.middle = {{BlockDesc::RES, "middle_block.0", ch, ch},
              {BlockDesc::ST, "middle_block.1", ch, ch, ds},
              {BlockDesc::RES, "middle_block.2", ch, ch}};
  t.final_ch = ch;
  if (encoder_only) return t;
  std::vector<int> stack = t.in_ch;
  idx = 0;
  for (int level = u.n_mult - 1; level >= 0; --level) {
    for (int i = 0; i <= u.num_res_blocks; ++i) {
      const int ich = stack.back();
      stack.pop_back();
      std::vector<BlockDesc> b;
      const int co = mc * u.channel_mult[level];
      b.push_back({BlockDesc::RES, "output_blocks." + std::to_string(idx) + ".0", ch + ich, co});
      ch = co;
      int j = 1;
      t.out_ds.push_back(ds);
      if (in_attn(ds)) b.push_back({BlockDesc::ST, "output_blocks." + std::to_string(idx) + "." + std::to_string(j++), ch, ch, ds});
      if (level && i == u.num_res_blocks) {
        b.push_back({BlockDesc::UP, "output_blocks." + std::to_string(idx) + "." + std::to_string(j), ch, ch});
        ds /= 2;
      }
      t.output.push_back(b);
      ++idx;
    }
  }
  t.final_ch = ch;
  return t;
}

std::vector<std::string> topo_resblocks(const UNetTopo& t) {
  std::vector<std::string> r;
  auto scan = [&](const std::vector<BlockDesc>& b) {
    for (auto& d : b)
      if (d.kind == BlockDesc::RES) r.push_back(d.prefix);
  };
  for (auto& b : t.input) scan(b);
  scan(t.middle);
  for (auto& b : t.output) scan(b);
  return r;
}
std::vector<BlockDesc> topo_sts(const UNetTopo& t) {
  std::vector<BlockDesc> r;
  auto scan = [&](const std::vector<BlockDesc>& b) {
    for (auto& d : b)
      if (d.kind == BlockDesc::ST) r.push_back(d);
  };
  for (auto& b : t.input) scan(b);
  scan(t.middle);
  for (auto& b : t.output) scan(b);
  return r;
}

// ---------------------------------------------------------------------------------------------------------------
// UNet / classifier plan.  which: 0 = denoiser UNet, 1 = alignment classifier backbone.
//   cfg_mode (UNet only): external x/t hold B = N/2 rows, the batch is duplicated on the fly and the CFG combine
//   is applied to the output.
void build_unet_like(df_ctx* c, Plan* pl, int which, int N, int H, int W, int Tc, bool cfg_mode) {
  const df_unet_config& u = which ? c->ccfg : c->ucfg;
  const std::string pre = which ? "classifier.model." : "model.diffusion_model.";
  Builder b{c, pl, pre, which};
  UNetTopo topo = make_topo(u, which == 1);
  const int mc = u.model_channels, temb = 4 * mc, HW = H * W, heads = u.num_heads;
  const int Dc = u.context_dim;

  // ---- context K / V^T for every SpatialTransformer (part of this plan: run by set_context or inline)
  std::vector<BlockDesc> sts = topo_sts(topo);
  const int ldvtc = rup(Tc, 32);
  bf16_t* ctxb = b.context_cast(N, Tc, Dc);
  Builder::KV kv;
  std::map<std::string, Builder::PX> pxs;
  for (auto& d : sts) {
    const int tokens = (H / d.ds) * (W / d.ds);
    // the denoiser's context is set once per sample() call: fold it into per-sample operands where the shapes allow;
    // the classifier gets new features with every call and keeps the K / V^T form
    if (which == 0 && Builder::px_ok(d.cin, heads, Tc, tokens)) {
      pxs[d.prefix] = b.context_px(ctxb, N, Tc, Dc, d.prefix, d.cin, heads);
      kv[d.prefix] = {nullptr, nullptr};
      continue;
    }
    b.context_kv_for(ctxb, N, Tc, Dc, d, ldvtc, kv);
  }
  pl->n_ctx = pl->ops.size();

  // ---- time embedding MLP and the fused emb projection of every ResBlock
  const int B_ext = cfg_mode ? N / 2 : N;
  const int etot = c->emb_total[which];
  float* E = b.buf<float>((size_t)N * etot);
  pl->op_t0 = (long)pl->ops.size();
  {
    const bf16_t* w0 = c->w_linear(pre + "time_embed.0.weight");
    const float* b0 = c->f32(pre + "time_embed.0.bias");
    const bf16_t* w2 = c->w_linear(pre + "time_embed.2.weight");
    const float* b2 = c->f32(pre + "time_embed.2.bias");
    const bf16_t* w;
    const float* bb;
    b.emb_proj_operands(topo, &w, &bb);
    // The time-embedding MLP and the stacked emb projections as three MFMA GEMMs (M = N rows, rows beyond M are
    // out-of-bounds zero fill): the 52 MB emb weight stream goes through the LDS-DMA ring of the GEMM kernel at the HBM
    // rate, where the GEMV kernels reach 0.9 TB/s.  Activations take the operand type here (they are O(1) sinusoids /
    // SiLU outputs; the projections' fp32 results E are what the ResBlocks consume).
    bf16_t* teb = b.buf<bf16_t>((size_t)N * mc);
    bf16_t* e1b = b.buf<bf16_t>((size_t)N * temb);
    bf16_t* seb = b.buf<bf16_t>((size_t)N * temb);
    b.other("t.embed", [=](hipStream_t s, const RunArgs& a) { return launch_timestep_embedding_b16(a.t, B_ext, teb, N, mc, s); });
    {
      GemmParams g = Builder::gp_linear(teb, N, mc, w0, temb);
      Builder::out_b16(g, e1b, temb);
      g.bias = b0; g.silu = 1;
      b.gemm(g, 1, "t.mlp0");
    }
    {
      GemmParams g = Builder::gp_linear(e1b, N, temb, w2, temb);
      Builder::out_b16(g, seb, temb);
      g.bias = b2; g.silu = 1;          // emb is only ever consumed through SiLU (emb_layers = SiLU -> Linear)
      b.gemm(g, 1, "t.mlp2");
    }
    {
      GemmParams g = Builder::gp_linear(seb, N, temb, w, etot);
      Builder::out_f32(g, E, etot);
      g.bias = bb;
      b.gemm(g, 1, "t.embproj");
    }
    pl->weight_bytes += 2.0 * etot * temb + 2.0 * (temb * mc + temb * temb);
  }
  // (round 5) a hoisted step's two leading launches -- the table look-up and the latent packing -- are one launch
  const bool step_merge = !which && etot % 4 == 0;
  if (!which && etot % 4 == 0) {
    // the table look-up that replaces the ops above when the caller announced its timesteps (df_unet_set_timesteps): the time
    // embedding depends on t only, so a sampler computes it for all S steps before the loop, like the context operands
    pl->op_tl = (long)pl->ops.size();
    pl->E = E; pl->etot = etot; pl->e_rows = N; pl->t_rows = B_ext;
    pl->tl_merged = step_merge;
    Plan* plp = pl;
    b.other("t.lookup", [=](hipStream_t s, const RunArgs& a) {
      if (a.ts_index < 0) return hipSuccess;
      if (!plp->Etab || a.ts_index >= plp->etab_S) return hipErrorInvalidValue;
      if (step_merge) return hipSuccess;       // the row broadcast rides in x.pack's launch (below)
      return launch_bcast_rows(plp->Etab + (size_t)a.ts_index * etot, E, N, etot, s);
    });
  }

  // ---- input packing: NCHW fp32 -> NHWC bf16 (channels padded to 64), CFG duplication folded in
  const int cin = Builder::checked_in_channels(u);
  // Classifier-free guidance runs the batch [x ; x] with the contexts [uncond ; cond]: everything in front of the first
  // cross-attention -- conv_in, the first ResBlock, and the first SpatialTransformer up to its self-attention out-projection --
  // is identical in both halves.  Those ops run on ONE half; the ops whose outputs the full batch needs (conv_in -> skip +
  // ResBlock, ResBlock -> transformer residual, attn1.out -> residual stream) store every row twice (GemmParams::dup_rows).
  const bool dedup = cfg_mode && !which && N % 2 == 0 && topo.input.size() >= 2 &&
                     topo.input[0].size() == 1 && topo.input[0][0].kind == BlockDesc::CONV_IN && topo.input[1].size() == 2 &&
                     topo.input[1][0].kind == BlockDesc::RES && topo.input[1][1].kind == BlockDesc::ST && (HW % 4) == 0 &&
                     pxs.count(topo.input[1][1].prefix) > 0;
  const int Np = dedup ? N / 2 : N;              // samples the prefix ops run on
  bf16_t* xin = b.buf<bf16_t>((size_t)Np * HW * 64);
  {
    Plan* plp = pl;
    float* Eb = E;
    b.other("x.pack", [=](hipStream_t s, const RunArgs& a) {
      if (step_merge && a.ts_index >= 0 && plp->Etab && a.ts_index < plp->etab_S)
        return launch_pack_latent_bcast(a.x, xin, B_ext, cin, HW, 64, (cfg_mode && !dedup) ? 2 : 1,
                                        plp->Etab + (size_t)a.ts_index * etot, Eb, N, etot, s);
      return launch_pack_latent(a.x, xin, B_ext, cin, HW, 64, (cfg_mode && !dedup) ? 2 : 1, 1.0f, nullptr, nullptr, s);
    });
  }

  // ---- concat buffers of the decoder (skip tensors are produced straight into them)
  const int nin = (int)topo.input.size();
  struct Cat { float* p; int ch, ich, rows, h, w; };
  std::vector<Cat> cats;
  if (!which) {
    // output block j pops input block (nin-1-j)
    int ch = topo.middle.back().cout;
    for (int j = 0; j < (int)topo.output.size(); ++j) {
      const int k = nin - 1 - j;
      const int ich = topo.in_ch[k], ds = topo.in_ds[k];
      const int h = H / ds, w = W / ds, rows = N * h * w;
      float* p = b.buf<float>((size_t)rows * (ch + ich));
      cats.push_back({p, ch, ich, rows, h, w});
      ch = topo.output[j][0].cout;
    }
  }
  auto skip_slot = [&](int k) -> F32 {   // destination of input block k's output
    if (which) return F32{};
    const Cat& ct = cats[nin - 1 - k];
    return F32{ct.p + ct.ch, ct.rows, ct.ich, ct.ch + ct.ich};
  };

  bf16_t* h_aux = nullptr;        // operand-type copy of the current h, when its producer was asked for one
  bool in_prefix = false;         // building input_blocks[0..1] of a deduplicated CFG batch
  auto run_block = [&](const std::vector<BlockDesc>& blk, F32 h, int ds, F32 final_dst, bool tail_aux) -> F32 {
    for (size_t li = 0; li < blk.size(); ++li) {
      const BlockDesc& d = blk[li];
      const bool last = (li + 1 == blk.size());
      int hh = H / ds, ww = W / ds;
      F32 dst;
      // the conv of a following Downsample / Upsample reads the operand-type copy of this op's output
      b.want_aux = (d.kind == BlockDesc::RES || d.kind == BlockDesc::ST) &&
                   (last ? tail_aux : blk[li + 1].kind == BlockDesc::UP);
      bf16_t* in_aux = h_aux;
      h_aux = nullptr;
      auto mk = [&](int rows, int C) {
        if (last && final_dst.p) return final_dst;
        return F32{b.buf<float>((size_t)rows * C), rows, C, C};
      };
      if (d.kind == BlockDesc::CONV_IN) {
        dst = mk(N * HW, d.cout);
        GemmParams g = Builder::gp_conv3(xin, in_prefix ? Np : N, H, W, 64, c->w_conv3(pre + d.prefix + ".weight", 64), d.cout, 1, 0);
        Builder::out_f32(g, dst.p, dst.ld);
        g.bias = c->f32(pre + d.prefix + ".bias");
        g.dup_rows = in_prefix ? Np * HW : 0;
        b.gemm(g, 1, "conv_in");
      } else if (d.kind == BlockDesc::RES) {
        dst = mk(h.rows, d.cout);
        if (in_prefix)
          b.resblock(F32{h.p, h.rows / 2, h.C, h.ld}, dst, Np, hh, ww, d.prefix + ".in_layers.0", d.prefix + ".in_layers.2",
                     d.prefix + ".out_layers.0", d.prefix + ".out_layers.3", d.prefix + ".skip_connection", 1e-5f, E, etot,
                     c->emb_off[which].at(d.prefix), h.rows / 2);
        else
        b.resblock(h, dst, N, hh, ww, d.prefix + ".in_layers.0", d.prefix + ".in_layers.2", d.prefix + ".out_layers.0",
                   d.prefix + ".out_layers.3", d.prefix + ".skip_connection", 1e-5f, E, etot,
                   c->emb_off[which].at(d.prefix));
      } else if (d.kind == BlockDesc::ST) {
        dst = mk(h.rows, d.cout);
        b.spatial_transformer(h, dst, N, hh * ww, d.prefix, heads, kv[d.prefix].first, kv[d.prefix].second, Tc, ldvtc,
                              pxs.count(d.prefix) ? &pxs[d.prefix] : nullptr, in_prefix);
      } else if (d.kind == BlockDesc::DOWN) {
        dst = mk(h.rows / 4, d.cout);
        bf16_t* hb = in_aux ? in_aux : b.cast2d(h);
        GemmParams g = Builder::gp_conv3(hb, N, hh, ww, d.cin, c->w_conv3(pre + d.prefix + ".op.weight", d.cin), d.cout, 2, 0);
        Builder::out_f32(g, dst.p, dst.ld);
        g.bias = c->f32(pre + d.prefix + ".op.bias");
        b.gemm(g, 1, "down");
        pl->release(hb);
      } else {  // UP: nearest x2 then conv3x3 (openai_unetmodel.py:100-119)
        dst = mk(h.rows * 4, d.cout);
        bf16_t* hb = in_aux ? in_aux : b.cast2d(h);
        // Upsample (openai_unetmodel.py:100-119): four 2x2-tap convs on the input-resolution map instead of a 3x3 conv on
        // the x2 map (2.25x fewer multiply-adds, gemm_m3.hip)
        GemmParams g = Builder::gp_conv3_ups4(hb, N, hh, ww, d.cin, c->w_conv3_ups4(pre + d.prefix + ".conv.weight", d.cin), d.cout);
        Builder::out_f32(g, dst.p, dst.ld);
        g.bias = c->f32(pre + d.prefix + ".conv.bias");
        b.gemm(g, 1, "up");
        pl->release(hb);
      }
      if (d.kind == BlockDesc::RES || d.kind == BlockDesc::ST) h_aux = b.last_aux;
      b.last_aux = nullptr;
      b.want_aux = false;
      // the previous intermediate is dead unless it lives in a concat buffer
      bool in_cat = false;
      for (auto& ct : cats)
        if (h.p >= ct.p && h.p < ct.p + (size_t)ct.rows * (ct.ch + ct.ich)) in_cat = true;
      if (h.p && !in_cat) pl->release(h.p);
      h = dst;
    }
    return h;
  };

  F32 h{};
  for (int k = 0; k < nin; ++k) {
    const int ds_run = (topo.input[k][0].kind == BlockDesc::DOWN) ? topo.in_ds[k] / 2 : topo.in_ds[k];
    const bool next_down = (k + 1 < nin) && topo.input[k + 1][0].kind == BlockDesc::DOWN;
    in_prefix = dedup && k <= 1;
    h = run_block(topo.input[k], h, ds_run, skip_slot(k), next_down);
    in_prefix = false;
  }
  const int ds_mid = topo.in_ds.back();
  if (which) {
    h = run_block(topo.middle, h, ds_mid, F32{}, false);
    // classifier head: GN -> SiLU -> conv3x3 -> global avg-pool -> Linear -> sigmoid (alignment_backbone.py:630-638)
    const int hh = H / ds_mid, ww = W / ds_mid, co = topo.final_ch / 2;
    bf16_t* a = b.groupnorm(h, N, "out.0", 1e-5f, 1, nullptr);
    float* ho = b.buf<float>((size_t)h.rows * co);
    GemmParams g = Builder::gp_conv3(a, N, hh, ww, topo.final_ch, c->w_conv3(pre + "out.2.weight", topo.final_ch), co, 1, 0);
    Builder::out_f32(g, ho, co);
    g.bias = c->f32(pre + "out.2.bias");
    b.gemm(g, 1, "cls.out");
    float* pooled = b.buf<float>((size_t)N * rup(co, 8));
    const int hw2 = hh * ww, oc = u.out_channels;
    b.other("cls.pool", [=](hipStream_t s, const RunArgs&) { return launch_avgpool(ho, pooled, N, hw2, co, s); });
    const bf16_t* wc = c->w_linear(pre + "classifier.weight");
    const float* bc = c->f32(pre + "classifier.bias");
    b.other("cls.head", [=](hipStream_t s, const RunArgs& ar) { return launch_linear_rows(pooled, co, wc, bc, ar.out, oc, N, oc, co, 2, s); });
    return;
  }
  // middle block output goes into the first concat buffer's leading columns
  h = run_block(topo.middle, h, ds_mid, F32{cats[0].p, cats[0].rows, cats[0].ch, cats[0].ch + cats[0].ich}, false);
  const int nout = (int)topo.output.size();
  for (int j = 0; j < nout; ++j) {
    F32 cat{cats[j].p, cats[j].rows, cats[j].ch + cats[j].ich, cats[j].ch + cats[j].ich};
    F32 dst{};
    if (j + 1 < nout) dst = F32{cats[j + 1].p, cats[j + 1].rows, cats[j + 1].ch, cats[j + 1].ch + cats[j + 1].ich};
    h = run_block(topo.output[j], cat, topo.out_ds[j], dst, false);
  }
  // ---- out: GN -> SiLU -> conv3x3 -> NCHW fp32 (openai_unetmodel.py:682-686)
  bf16_t* a = b.groupnorm(h, N, "out.0", 1e-5f, 1, nullptr);
  GemmParams g = Builder::gp_conv3(a, N, H, W, mc, c->w_conv3(pre + "out.2.weight", mc), u.out_channels, 1, 0);
  g.bias = c->f32(pre + "out.2.bias");
  g.store_nchw = 1;
  g.hw_out = HW;
  if (cfg_mode) {
    float* e2 = b.buf<float>((size_t)N * u.out_channels * HW);
    Builder::out_f32(g, e2, u.out_channels);
    // (round 5) when the tuner runs out.conv split-K, its reduce launch forms the guided eps as well (gemm.hip
    // splitk_reduce_cfg_kernel: same arithmetic, one launch fewer); cfg.combine then has nothing to do.
    b.gemm(g, 1, "out.conv").cfg_ext = true;
    const size_t oci = pl->ops.size() - 1;
    Plan* plq = pl;
    const long n = (long)(N / 2) * u.out_channels * HW;
    pl->op_outconv = (long)oci;
    pl->op_cfgc = (long)pl->ops.size();
    b.other("cfg.combine", [=](hipStream_t s, const RunArgs& ar) {
      if (plq->ops[oci].cfg_ext && plq->ops[oci].gp.splitk > 1) return hipSuccess;
      return launch_cfg_combine(e2, ar.out, n, ar.scale, s);
    });
  } else {
    Builder::out_f32(g, nullptr, u.out_channels);
    Op& o = b.gemm(g, 1, "out.conv");
    o.c_ext = true;
  }
}

// AttnBlock (stage1_autoencoder/model.py:273-297) of the VAE's mid section, decoder and encoder alike: a single head over T = hh * ww
// tokens with head dim = ch -> GEMM + row-softmax + GEMM.  p: the block's state_dict prefix below b.pre; t: the op tags of the plan it
// is built into.  Consumes h (released) and returns the block's output.
struct VaeAttnTags { const char *q, *k, *vT_pad, *vT, *qk, *softmax, *pv, *proj_out; };
static const VaeAttnTags kVaeDecAttn{"vae.q", "vae.k", "vae.vT.pad", "vae.vT", "vae.qk", "vae.softmax", "vae.pv", "vae.proj_out"};
static const VaeAttnTags kVaeEncAttn{"vaeenc.q", "vaeenc.k", "vaeenc.vT.pad", "vaeenc.vT", "vaeenc.qk", "vaeenc.softmax", "vaeenc.pv",
                                     "vaeenc.proj_out"};
static F32 vae_attn_block(Builder& b, const std::string& p, F32 h, int B, int T, const VaeAttnTags& t) {
  df_ctx* c = b.c;
  Plan* pl = b.pl;
  const std::string& pre = b.pre;
  const int ch = h.C, M = B * T;
  // the P V contraction runs over the tokens: padded to whole 64-element K steps (zero probabilities against zeroed V^T columns)
  // for maps whose token count is not a multiple of 64 (any latent but the 16 x 64 one may be: decode_first_stage takes them all)
  const int Tp = rup(T, 64);
  bf16_t* a = b.groupnorm(h, B, p + ".norm", 1e-6f, 0, nullptr);
  bf16_t* q = b.buf<bf16_t>((size_t)M * ch);
  bf16_t* k = b.buf<bf16_t>((size_t)M * ch);
  bf16_t* vt = b.buf<bf16_t>((size_t)B * ch * Tp);
  {
    GemmParams g = Builder::gp_linear(a, M, ch, c->w_linear(pre + p + ".q.weight"), ch);
    Builder::out_b16(g, q, ch);
    g.bias = c->f32(pre + p + ".q.bias");
    b.gemm(g, 1, t.q);
  }
  {
    GemmParams g = Builder::gp_linear(a, M, ch, c->w_linear(pre + p + ".k.weight"), ch);
    Builder::out_b16(g, k, ch);
    g.bias = c->f32(pre + p + ".k.bias");
    b.gemm(g, 1, t.k);
  }
  {  // V^T without its bias: softmax rows sum to 1, so P(V + 1 b^T) = P V + b^T -> bias added after P V
    if (Tp != T) {
      const size_t nb = (size_t)B * ch * Tp * sizeof(bf16_t);
      b.other(t.vT_pad, [=](hipStream_t s, const RunArgs&) { return hipMemsetAsync(vt, 0, nb, s); });
    }
    GemmParams g = Builder::gp_linear(c->w_linear(pre + p + ".v.weight"), ch, ch, a, T);
    g.w_bs = (long)T * ch;
    Builder::out_b16(g, vt, Tp);
    g.c_bs = (long)ch * Tp;
    b.gemm(g, B, t.vT);
  }
  float* sc = b.buf<float>((size_t)B * T * T);
  {
    GemmParams g = Builder::gp_linear(q, T, ch, k, T);
    g.a_bs = (long)T * ch;
    g.w_bs = (long)T * ch;
    Builder::out_f32(g, sc, T);
    g.c_bs = (long)T * T;
    g.alpha = 1.0f / sqrtf((float)ch);
    b.gemm(g, B, t.qk);
  }
  bf16_t* pr = b.buf<bf16_t>((size_t)B * T * Tp);
  b.other(t.softmax, [=](hipStream_t s, const RunArgs&) { return launch_softmax_rows(sc, pr, B * T, T, Tp, s); });
  bf16_t* o = q;
  {
    GemmParams g = Builder::gp_linear(pr, T, Tp, vt, ch);
    g.a_bs = (long)T * Tp;
    g.w_bs = (long)ch * Tp;
    Builder::out_b16(g, o, ch);
    g.c_bs = (long)T * ch;
    g.bias = c->f32(pre + p + ".v.bias");
    b.gemm(g, B, t.pv);
  }
  F32 ho{b.buf<float>((size_t)M * ch), M, ch, ch};
  {
    GemmParams g = Builder::gp_linear(o, M, ch, c->w_linear(pre + p + ".proj_out.weight"), ch);
    Builder::out_f32(g, ho.p, ch);
    g.bias = c->f32(pre + p + ".proj_out.bias");
    g.res = h.p; g.ldr = h.ld;
    b.gemm(g, 1, t.proj_out);
  }
  for (void* p_ : {(void*)a, (void*)q, (void*)k, (void*)vt, (void*)sc, (void*)pr, (void*)h.p}) pl->release(p_);
  return ho;
}

// VAE decoder plan (autoencoder.py:330-333, stage1_autoencoder/model.py:630-663)
void build_vae(df_ctx* c, Plan* pl, int B, int H, int W) {
  const df_vae_config& v = c->vcfg;
  const std::string pre = "first_stage_model.";
  Builder b{c, pl, pre, 0};
  const int zc = v.z_channels;
  if (zc < 1 || zc > 64 || v.embed_dim != zc)
    fail("vae: z_channels = %d, embed_dim = %d: post_quant_conv is applied as a square 1x1 mix of 1 .. 64 latent channels while the "
         "latent is packed", zc, v.embed_dim);
  int hh = H, ww = W;
  int ch = v.ch * v.ch_mult[v.n_mult - 1];
  bf16_t* zin = b.buf<bf16_t>((size_t)B * hh * ww * 64);
  {
    const float* wpq = c->f32(pre + "post_quant_conv.weight");
    const float* bpq = c->f32(pre + "post_quant_conv.bias");
    const float inv = 1.0f / v.scale_factor;
    const int HW = hh * ww;
    b.other("z.pack", [=](hipStream_t s, const RunArgs& a) { return launch_pack_latent(a.x, zin, B, zc, HW, 64, 1, inv, wpq, bpq, s); });
  }
  F32 h{b.buf<float>((size_t)B * hh * ww * ch), B * hh * ww, ch, ch};
  {
    GemmParams g = Builder::gp_conv3(zin, B, hh, ww, 64, c->w_conv3(pre + "decoder.conv_in.weight", 64), ch, 1, 0);
    Builder::out_f32(g, h.p, ch);
    g.bias = c->f32(pre + "decoder.conv_in.bias");
    b.gemm(g, 1, "vae.conv_in");
  }
  auto res = [&](const std::string& p, F32 x, int cout) {
    F32 o{b.buf<float>((size_t)x.rows * cout), x.rows, cout, cout};
    b.resblock(x, o, B, hh, ww, p + ".norm1", p + ".conv1", p + ".norm2", p + ".conv2", p + ".nin_shortcut", 1e-6f,
               nullptr, 0, 0);
    pl->release(x.p);
    return o;
  };
  h = res("decoder.mid.block_1", h, ch);
  h = vae_attn_block(b, "decoder.mid.attn_1", h, B, hh * ww, kVaeDecAttn);
  h = res("decoder.mid.block_2", h, ch);
  for (int lvl = v.n_mult - 1; lvl >= 0; --lvl) {
    const int co = v.ch * v.ch_mult[lvl];
    for (int ib = 0; ib <= v.num_res_blocks; ++ib)
      h = res("decoder.up." + std::to_string(lvl) + ".block." + std::to_string(ib), h, co);
    if (lvl != 0) {
      bf16_t* hb = b.cast2d(h);
      F32 o{b.buf<float>((size_t)h.rows * 4 * co), h.rows * 4, co, co};
      const std::string p = pre + "decoder.up." + std::to_string(lvl) + ".upsample.conv";
      GemmParams g = Builder::gp_conv3_ups4(hb, B, hh, ww, co, c->w_conv3_ups4(p + ".weight", co), co);
      Builder::out_f32(g, o.p, co);
      g.bias = c->f32(p + ".bias");
      b.gemm(g, 1, "vae.up");
      pl->release(hb);
      pl->release(h.p);
      h = o;
      hh *= 2;
      ww *= 2;
    }
  }
  bf16_t* a = b.groupnorm(h, B, "decoder.norm_out", 1e-6f, 1, nullptr);
  if (conv3x3_fewout_ok(hh, ww, h.C, v.out_ch)) {
    const bf16_t* wp = c->w_conv3(pre + "decoder.conv_out.weight", h.C);
    const float* bo = c->f32(pre + "decoder.conv_out.bias");
    const int H_ = hh, W_ = ww, C_ = h.C, O_ = v.out_ch;
    b.other("vae.conv_out", [=](hipStream_t s, const RunArgs& ra) { return launch_conv3x3_fewout(a, wp, bo, ra.out, B, H_, W_, C_, O_, s); });
    return;
  }
  GemmParams g = Builder::gp_conv3(a, B, hh, ww, h.C, c->w_conv3(pre + "decoder.conv_out.weight", h.C), v.out_ch, 1, 0);
  Builder::out_f32(g, nullptr, v.out_ch);
  g.bias = c->f32(pre + "decoder.conv_out.bias");
  g.store_nchw = 1;
  g.hw_out = hh * ww;
  Op& o = b.gemm(g, 1, "vae.conv_out");
  o.c_ext = true;
}

// VAE encoder plan: quant_conv(encoder(x)) (autoencoder.py:324-328, stage1_autoencoder/model.py:529-554).  The decoder's mirror image:
// conv_in from the <= 4 image channels (conv3x3_fewin), per level num_res_blocks ResnetBlocks and -- on every level but the last -- the
// asymmetrically padded stride-2 Downsample (model.py:167-171, gp_conv3_down_asym), mid block_1 / attn_1 / block_2, norm_out + SiLU,
// conv_out, and quant_conv as a second small fp32 op that writes the moments NCHW.
void build_vae_encoder(df_ctx* c, Plan* pl, int B, int H, int W, int tap) {
  const df_vae_config& v = c->vcfg;
  const std::string pre = "first_stage_model.";
  Builder b{c, pl, pre, 0};
  const int zc = v.z_channels, cin = c->ecfg.in_channels;
  if (zc < 1 || zc > 64 || v.embed_dim != zc)
    fail("vae encoder: z_channels = %d, embed_dim = %d: built for embed_dim == z_channels, 1 .. 64 (as the decoder)", zc, v.embed_dim);
  if (cin < 1 || cin > 4) fail("vae encoder: in_channels = %d: conv_in is built for 1 .. 4 image channels", cin);
  // The latent of a clip must not depend on its batch-mates (x0 of an inpainting call; the decoder's and the UNet's tables are keyed by
  // the row count, so their summation order follows the batch): every GEMM choice is a function of the per-sample problem
  b.choice_NB = B;
  pl->fixed_choices = true;
  int hh = H, ww = W;
  int ch = v.ch;
  F32 h{b.buf<float>((size_t)B * hh * ww * ch), B * hh * ww, ch, ch};
  {
    if (!conv3x3_fewin_ok(hh, ww, cin, ch, ch)) fail("vae encoder: no conv_in kernel for %d -> %d channels", cin, ch);
    const float* wi = c->f32(pre + "encoder.conv_in.weight");
    const float* bi = c->f32(pre + "encoder.conv_in.bias");
    float* o = h.p;
    const int H_ = hh, W_ = ww, C_ = ch;
    pl->ext_hint = std::max(pl->ext_hint, (size_t)B * cin * H * W * 4);
    b.other("vaeenc.conv_in", [=](hipStream_t s, const RunArgs& a) { return launch_conv3x3_fewin(a.x, wi, bi, o, C_, B, H_, W_, cin, C_, s); });
  }
  auto tap_here = [&](int id, const F32& x) {      // tests only: the stage's rows leave the plan as they are at this point
    if (tap != id) return;
    const float* src = x.p;
    const size_t bytes = (size_t)x.rows * x.C * sizeof(float);
    b.other("vaeenc.tap", [=](hipStream_t s, const RunArgs& ra) {
      return ra.out2 ? hipMemcpyAsync(ra.out2, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
    });
  };
  tap_here(0, h);
  auto res = [&](const std::string& p, F32 x, int cout) {
    F32 o{b.buf<float>((size_t)x.rows * cout), x.rows, cout, cout};
    b.resblock(x, o, B, hh, ww, p + ".norm1", p + ".conv1", p + ".norm2", p + ".conv2", p + ".nin_shortcut", 1e-6f,
               nullptr, 0, 0);
    pl->release(x.p);
    return o;
  };
  for (int lvl = 0; lvl < v.n_mult; ++lvl) {
    const int co = v.ch * v.ch_mult[lvl];
    const bool down = lvl != v.n_mult - 1;
    bf16_t* hb = nullptr;
    for (int ib = 0; ib < v.num_res_blocks; ++ib) {
      // the Downsample conv reads the operand-type copy of the level's last ResnetBlock output: written by that block's conv2
      b.want_aux = down && ib == v.num_res_blocks - 1;
      h = res("encoder.down." + std::to_string(lvl) + ".block." + std::to_string(ib), h, co);
      hb = b.last_aux;
      b.last_aux = nullptr;
      b.want_aux = false;
    }
    ch = co;
    if (down) {
      if (!hb) hb = b.cast2d(h);
      F32 o{b.buf<float>((size_t)(h.rows / 4) * co), h.rows / 4, co, co};
      const std::string p = pre + "encoder.down." + std::to_string(lvl) + ".downsample.conv";
      GemmParams g = Builder::gp_conv3_down_asym(hb, B, hh, ww, co, c->w_conv3(p + ".weight", co), co);
      Builder::out_f32(g, o.p, co);
      g.bias = c->f32(p + ".bias");
      b.gemm(g, 1, "vaeenc.down");
      pl->release(hb);
      pl->release(h.p);
      h = o;
      hh /= 2;
      ww /= 2;
      tap_here(1 + lvl, h);
    }
  }
  h = res("encoder.mid.block_1", h, ch);
  h = vae_attn_block(b, "encoder.mid.attn_1", h, B, hh * ww, kVaeEncAttn);
  h = res("encoder.mid.block_2", h, ch);
  tap_here(100, h);
  bf16_t* a = b.groupnorm(h, B, "encoder.norm_out", 1e-6f, 1, nullptr);
  float* m = b.buf<float>((size_t)h.rows * 2 * zc);
  {
    GemmParams g = Builder::gp_conv3(a, B, hh, ww, ch, c->w_conv3(pre + "encoder.conv_out.weight", ch), 2 * zc, 1, 0);
    Builder::out_f32(g, m, 2 * zc);
    g.bias = c->f32(pre + "encoder.conv_out.bias");
    b.gemm(g, 1, "vaeenc.conv_out");
  }
  {
    const float* wq = c->f32(pre + "quant_conv.weight");
    const float* bq = c->f32(pre + "quant_conv.bias");
    const int HW = hh * ww, ci = 2 * zc, co = 2 * v.embed_dim;
    b.other("vaeenc.quant_conv", [=](hipStream_t s, const RunArgs& ra) { return launch_conv1x1_rows_nchw(m, ci, wq, bq, ra.out, B, HW, ci, co, s); });
  }
}

std::vector<std::string> vae_encoder_tensor_names(const df_ctx* c) {
  const df_vae_config& v = c->vcfg;
  std::vector<std::string> r;
  const std::string e = "first_stage_model.encoder.";
  auto wb = [&](const std::string& p) { r.push_back(p + ".weight"); r.push_back(p + ".bias"); };
  auto resn = [&](const std::string& p, int ci, int co) {
    wb(p + ".norm1"); wb(p + ".conv1"); wb(p + ".norm2"); wb(p + ".conv2");
    if (ci != co) wb(p + ".nin_shortcut");
  };
  wb(e + "conv_in");
  int ch = v.ch;
  for (int lvl = 0; lvl < v.n_mult; ++lvl) {
    const int co = v.ch * v.ch_mult[lvl];
    for (int ib = 0; ib < v.num_res_blocks; ++ib) {
      resn(e + "down." + std::to_string(lvl) + ".block." + std::to_string(ib), ch, co);
      ch = co;
    }
    if (lvl != v.n_mult - 1) wb(e + "down." + std::to_string(lvl) + ".downsample.conv");
  }
  resn(e + "mid.block_1", ch, ch);
  wb(e + "mid.attn_1.norm");
  for (const char* n : {"q", "k", "v", "proj_out"}) wb(e + "mid.attn_1." + n);
  resn(e + "mid.block_2", ch, ch);
  wb(e + "norm_out");
  wb(e + "conv_out");
  wb("first_stage_model.quant_conv");
  return r;
}

// cond stage: Linear(origin->embed) + pos_emb[:T]  (video_feat_encoder.py:12-18)
void build_cond(df_ctx* c, Plan* pl, int B, int T) {
  const df_cond_config& k = c->kcfg;
  const std::string pre = "cond_stage_model.";
  Builder b{c, pl, pre, 0};
  if (T > k.seq_len) fail("cond stage: %d frames > pos_emb length %d", T, k.seq_len);
  const long n = (long)B * T * k.origin_dim;
  bf16_t* xb = b.buf<bf16_t>((size_t)n);
  b.other("cond.cast", [=](hipStream_t s, const RunArgs& a) { return launch_cast_bf16(a.x, xb, n, s); });
  GemmParams g = Builder::gp_linear(xb, B * T, k.origin_dim, c->w_linear(pre + "embedder.0.weight"), k.embed_dim);
  Builder::out_f32(g, nullptr, k.embed_dim);
  g.bias = c->f32(pre + "embedder.0.bias");
  g.rowbias = c->f32(pre + "pos_emb.weight");
  g.ld_rowbias = k.embed_dim;
  g.rows_per_sample = T;
  g.rowbias_mode = 2;
  Op& o = b.gemm(g, 1, "cond.embed");
  o.c_ext = true;
}

// CAVP video encoder: SlowOnly-R50 over ONE clip of T frames -> [T][embed] features.
// inference/model/cavp_model.py:47-65 (encode_video, pool=False), cavp_modules.py:757-779 / 837-859 / 167-330.
// Activations are frame-major NHWC; every conv is an MFMA GEMM with the eval BatchNorm folded into weights + bias and
// ReLU in the epilogue: stem = explicit im2col (K 147 -> 192), (1,3,3) convs = implicit GEMM (stride 1|2), (3,1,1)
// temporal convs = one GEMM over the K-concatenation [x[t-1] | x[t] | x[t+1]], 1x1 stride-2 shortcuts = GEMM on the
// subsampled rows.  The residual stream stays fp32 (conv3 epilogue: + identity, ReLU, fp32 out + operand copy).
void build_cavp(df_ctx* c, Plan* pl, int T, int H, int W) {
  const df_cavp_config& k = c->pcfg;
  const std::string pre = "cavp.video_encoder.";
  Builder b{c, pl, pre, 0};
  if (H % 32 || W % 32) fail("cavp: frame size %dx%d must be a multiple of 32", H, W);
  const int F = T;
  const int base = k.base_channels;
  pl->ext_hint = (size_t)F * 3 * H * W * 4;
  // ---- stem
  const int OH = H / 2, OW = W / 2, KP = 192;
  bf16_t* col = b.buf<bf16_t>((size_t)F * OH * OW * KP);
  b.other("cavp.im2col", [=](hipStream_t s, const RunArgs& a) { return launch_stem_im2col(a.x, col, F, H, W, OH, OW, KP, s); });
  const bf16_t* w;
  const float* bias;
  c->w_conv3d_bn(pre + "conv1", KP, &w, &bias);
  bf16_t* s1 = b.buf<bf16_t>((size_t)F * OH * OW * base);
  {
    GemmParams g = Builder::gp_linear(col, F * OH * OW, KP, w, base);
    Builder::out_b16(g, s1, base);
    g.bias = bias;
    g.relu = 1;
    b.gemm(g, 1, "cavp.stem");
  }
  pl->release(col);
  int h = OH / 2, wd = OW / 2;
  bf16_t* xb = b.buf<bf16_t>((size_t)F * h * wd * base);
  b.other("cavp.maxpool", [=](hipStream_t s, const RunArgs&) { return launch_maxpool3x3s2(s1, xb, F, OH, OW, h, wd, base, s); });
  pl->release(s1);
  float* xf = nullptr;          // fp32 residual stream (exists from the first block's output on)
  int cin = base;
  for (int li = 0; li < 4; ++li) {
    const int planes = base << li, cout = planes * 4;
    const bool inflate = li >= 2;
    for (int bi = 0; bi < k.stage_blocks[li]; ++bi) {
      const std::string p = pre + "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      const int stride = (bi == 0 && li > 0) ? 2 : 1;
      const int oh = h / stride, ow = wd / stride;
      const int Min = F * h * wd, Mout = F * oh * ow;
      // conv1: 1x1x1 or (3,1,1)
      bf16_t* h1 = b.buf<bf16_t>((size_t)Min * planes);
      if (inflate) {
        bf16_t* cat = b.buf<bf16_t>((size_t)Min * 3 * cin);
        const bf16_t* xin = xb;
        const int hw = h * wd, ci = cin;
        b.other("cavp.tcat", [=](hipStream_t s, const RunArgs&) { return launch_tcat3(xin, cat, F, T, hw, ci, s); });
        c->w_conv3d_bn(p + ".conv1", 3 * cin, &w, &bias);
        GemmParams g = Builder::gp_linear(cat, Min, 3 * cin, w, planes);
        Builder::out_b16(g, h1, planes);
        g.bias = bias;
        g.relu = 1;
        b.gemm(g, 1, "cavp.conv1t");
        pl->release(cat);
      } else {
        c->w_conv3d_bn(p + ".conv1", cin, &w, &bias);
        GemmParams g = Builder::gp_linear(xb, Min, cin, w, planes);
        Builder::out_b16(g, h1, planes);
        g.bias = bias;
        g.relu = 1;
        b.gemm(g, 1, "cavp.conv1");
      }
      // conv2: (1,3,3), stride on this conv ('pytorch' style)
      bf16_t* h2 = b.buf<bf16_t>((size_t)Mout * planes);
      {
        c->w_conv3d_bn(p + ".conv2", 9 * planes, &w, &bias);
        GemmParams g = Builder::gp_conv3(h1, F, h, wd, planes, w, planes, stride, 0);
        Builder::out_b16(g, h2, planes);
        g.bias = bias;
        g.relu = 1;
        b.gemm(g, 1, "cavp.conv2");
      }
      pl->release(h1);
      // identity / downsample
      const float* idt = xf;
      float* ds = nullptr;
      if (c->has(p + ".downsample.conv.weight")) {
        const bf16_t* src = xb;
        bf16_t* sub = nullptr;
        if (stride == 2) {
          sub = b.buf<bf16_t>((size_t)Mout * cin);
          const bf16_t* xin = xb;
          const int hh = h, ww = wd, ci = cin;
          b.other("cavp.subsample", [=](hipStream_t s, const RunArgs&) { return launch_subsample2(xin, sub, F, hh, ww, ci, s); });
          src = sub;
        }
        ds = b.buf<float>((size_t)Mout * cout);
        c->w_conv3d_bn(p + ".downsample", cin, &w, &bias);
        GemmParams g = Builder::gp_linear(src, Mout, cin, w, cout);
        Builder::out_f32(g, ds, cout);
        g.bias = bias;
        b.gemm(g, 1, "cavp.down");
        if (sub) pl->release(sub);
        idt = ds;
      }
      if (!idt) fail("cavp: block %s has neither a downsample conv nor an fp32 input", p.c_str());
      // conv3: 1x1x1 -> 4*planes, + identity, ReLU; fp32 residual + operand copy for the next block
      float* of = b.buf<float>((size_t)Mout * cout);
      bf16_t* ob = b.buf<bf16_t>((size_t)Mout * cout);
      {
        c->w_conv3d_bn(p + ".conv3", planes, &w, &bias);
        GemmParams g = Builder::gp_linear(h2, Mout, planes, w, cout);
        Builder::out_f32(g, of, cout);
        g.bias = bias;
        g.res = idt;
        g.ldr = cout;
        g.relu = 1;
        g.aux = ob;
        g.ld_aux = cout;
        b.gemm(g, 1, "cavp.conv3");
      }
      pl->release(h2);
      if (ds) pl->release(ds);
      if (xf) pl->release(xf);
      pl->release(xb);
      xf = of;
      xb = ob;
      cin = cout;
      h = oh;
      wd = ow;
    }
  }
  // ---- head: spatial mean -> Linear(4*8*base -> embed) (+ L2 normalisation, applied by the entry point when asked)
  float* pooled = b.buf<float>((size_t)F * cin);
  {
    const float* xin = xf;
    const int hw = h * wd, ci = cin;
    b.other("cavp.pool", [=](hipStream_t s, const RunArgs&) { return launch_avgpool(xin, pooled, F, hw, ci, s); });
  }
  {
    const bf16_t* wp = c->w_linear("cavp.video_project_head.weight");
    const float* bp = c->f32("cavp.video_project_head.bias");
    const int ci = cin, E = k.embed_dim;
    b.other("cavp.proj", [=](hipStream_t s, const RunArgs& a) {
      hipError_t e = launch_linear_rows(pooled, ci, wp, bp, a.out, E, F, E, ci, 0, s);
      if (e != hipSuccess) return e;
      return a.scale != 0.f ? launch_l2norm_rows(a.out, F, E, s) : hipSuccess;     // a.scale doubles as the normalize flag
    });
  }
}

// CAVP spectrogram encoder: Cnn14 over B clips of T frames x n_mels mel bins -> [B*T'][embed] features, T' = T floor-halved four times.
// inference/model/cavp_model.py:68-84 (encode_spec, pool=False), cavp_modules.py:1440-1483 (ConvBlock) / 1516-1546 (Cnn14.forward).
// Activations are NHWC with H = time, W = mel.  conv_block1.conv1 (one input channel, input BatchNorm in front of the padding) is the
// VALU kernel spec_conv_in; the other eleven convs are implicit GEMMs with the eval BatchNorm folded into weights + bias and ReLU in
// the epilogue.  The second conv of a block writes fp32 and the avg-pool behind it rounds to the operand type, so an activation is
// rounded once; block 6's (1, 1) pool is no launch, the head pool reads its fp32 output.  fc1 runs twice on one packed weight
// (cavp_modules.py:1543-1544).  Every GEMM choice is made for the per-sample problem: a clip's features do not depend on its batch.
void build_cavp_spec(df_ctx* c, Plan* pl, int B, int T, int n_mels, int tap) {
  const df_cavp_spec_config& k = c->scfg;
  const std::string pre = "cavp.spec_encoder.";
  Builder b{c, pl, pre, 0};
  b.choice_NB = B;
  pl->fixed_choices = true;
  const int C1 = k.channels[0];
  if (C1 < 8 || C1 % 8 || C1 > 256) fail("cavp spec: channels[0] = %d: the first conv is built for 8 .. 256 channels in steps of 8", C1);
  if (k.fc_dim != k.channels[5])
    fail("cavp spec: fc_dim = %d, channels[5] = %d: fc1 is applied twice (cavp_modules.py:1543-1544), so it must be square", k.fc_dim,
         k.channels[5]);
  if ((int)c->rt(pre + "bn.weight").n != n_mels) fail("cavp spec: the input BatchNorm has %zu bins, the mel has %d", c->rt(pre + "bn.weight").n, n_mels);
  auto bn4 = [&](const std::string& p) {
    return std::array<const float*, 4>{c->f32(p + ".weight"), c->f32(p + ".bias"), c->f32(p + ".running_mean"), c->f32(p + ".running_var")};
  };
  auto tap_here = [&](int id, const void* src, size_t bytes) {      // tests only
    if (tap != id) return;
    b.other("cavpspec.tap", [=](hipStream_t s, const RunArgs& ra) {
      return ra.out2 ? hipMemcpyAsync(ra.out2, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
    });
  };
  int h = T, w = n_mels;
  bf16_t* h1 = b.buf<bf16_t>((size_t)B * h * w * C1);
  {
    const std::array<const float*, 4> bn0 = bn4(pre + "bn"), bn1 = bn4(pre + "conv_block1.bn1");
    const float* wi = c->f32(pre + "conv_block1.conv1.weight");
    if (c->rt(pre + "conv_block1.conv1.weight").n != (size_t)C1 * 9) fail("cavp spec: conv_block1.conv1.weight is not [%d][1][3][3]", C1);
    pl->ext_hint = std::max(pl->ext_hint, (size_t)B * n_mels * T * 4);
    b.other("cavpspec.conv_in", [=](hipStream_t s, const RunArgs& a) {
      return launch_spec_conv_in(a.x, bn0.data(), wi, bn1.data(), 1e-5f, h1, C1, B, n_mels, T, C1, s);
    });
    b.emits(h1, (long)B * h * w, C1, C1);
  }
  const bf16_t* wp;
  const float* bias;
  bf16_t* xb = nullptr;            // operand-type input of the block (blocks 2 .. 6)
  float* f = nullptr;              // fp32 output of the block's second conv
  int cin = 1;
  for (int blk = 0; blk < 6; ++blk) {
    const int co = k.channels[blk];
    const std::string p = pre + "conv_block" + std::to_string(blk + 1);
    if (blk > 0) {
      h1 = b.buf<bf16_t>((size_t)B * h * w * co);
      c->w_conv2d_bn(p + ".conv1", p + ".bn1", 9 * cin, &wp, &bias);
      GemmParams g = Builder::gp_conv3(xb, B, h, w, cin, wp, co, 1, 0);
      Builder::out_b16(g, h1, co);
      g.bias = bias;
      g.relu = 1;
      b.gemm(g, 1, "cavpspec.conv1");
      pl->release(xb);
    }
    f = b.buf<float>((size_t)B * h * w * co);
    {
      c->w_conv2d_bn(p + ".conv2", p + ".bn2", 9 * co, &wp, &bias);
      GemmParams g = Builder::gp_conv3(h1, B, h, w, co, wp, co, 1, 0);
      Builder::out_f32(g, f, co);
      g.bias = bias;
      g.relu = 1;
      b.gemm(g, 1, "cavpspec.conv2");
    }
    pl->release(h1);
    cin = co;
    if (blk == 5) break;           // avg_pool2d((1, 1)) is the identity
    const int ph = blk < 4 ? 2 : 1, pw = 2;
    if (h < ph || w < pw) fail("cavp spec: the %dx%d map of conv_block%d does not survive its (%d, %d) pool (%d frames x %d mels)", h, w, blk + 1, ph, pw, T, n_mels);
    const int oh = h / ph, ow = w / pw;
    xb = b.buf<bf16_t>((size_t)B * oh * ow * co);
    {
      const float* src = f;
      bf16_t* dst = xb;
      const int hh = h, ww = w;
      b.other("cavpspec.pool", [=](hipStream_t s, const RunArgs&) { return launch_avgpool_nhwc(src, co, dst, co, B, hh, ww, co, ph, pw, s); });
      b.emits(xb, (long)B * oh * ow, co, co);
    }
    pl->release(f);
    h = oh;
    w = ow;
    tap_here(blk + 1, xb, (size_t)B * h * w * co * sizeof(bf16_t));
  }
  tap_here(6, f, (size_t)B * h * w * cin * sizeof(float));
  // ---- head: mean over mel, max3 + avg3 over time, relu(fc1) twice, final_project (+ L2 normalisation when asked)
  const int rows = B * h, C6 = cin, E = k.embed_dim;
  bf16_t* pooled = b.buf<bf16_t>((size_t)rows * C6);
  {
    const float* src = f;
    const int hh = h, ww = w;
    b.other("cavpspec.head_pool", [=](hipStream_t s, const RunArgs&) { return launch_spec_head_pool(src, C6, pooled, C6, B, hh, ww, C6, s); });
    b.emits(pooled, rows, C6, C6);
  }
  pl->release(f);
  const bf16_t* wf = c->w_linear(pre + "fc1.weight");
  const float* bf = c->f32(pre + "fc1.bias");
  bf16_t* y1 = b.buf<bf16_t>((size_t)rows * C6);
  bf16_t* y2 = b.buf<bf16_t>((size_t)rows * C6);
  for (int i = 0; i < 2; ++i) {
    GemmParams g = Builder::gp_linear(i ? y1 : pooled, rows, C6, wf, C6);
    Builder::out_b16(g, i ? y2 : y1, C6);
    g.bias = bf;
    g.relu = 1;
    b.gemm(g, 1, i ? "cavpspec.fc1b" : "cavpspec.fc1a");
  }
  {
    GemmParams g = Builder::gp_linear(y2, rows, C6, c->w_linear(pre + "final_project.weight"), E);
    Builder::out_f32(g, nullptr, E);
    g.bias = c->f32(pre + "final_project.bias");
    Op& o = b.gemm(g, 1, "cavpspec.project");
    o.c_ext = true;
  }
  b.other("cavpspec.l2norm", [=](hipStream_t s, const RunArgs& a) {      // a.scale doubles as the normalize flag, as in build_cavp
    return a.scale != 0.f ? launch_l2norm_rows(a.out, rows, E, s) : hipSuccess;
  });
}

void build_emb_table(df_ctx* c, int which) {
  const df_unet_config& u = which ? c->ccfg : c->ucfg;
  UNetTopo t = make_topo(u, which == 1);
  int off = 0;
  const std::string pre = which ? "classifier.model." : "model.diffusion_model.";
  for (auto& r : topo_resblocks(t)) {
    c->emb_off[which][r] = off;
    off += (int)c->rt(pre + r + ".emb_layers.1.weight").shape[0];
  }
  c->emb_total[which] = off;
}

}  // namespace dfe

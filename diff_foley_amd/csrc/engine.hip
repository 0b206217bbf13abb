// libdfengine: the product C ABI (include/df_engine.h) over the plan builders, the plan cache and the autotuner, and the
// packed-operand blob the ABI exports and imports.  Types, the context, the Builder and who defines what: engine_internal.h.
#include "engine_internal.h"

DFE_NAMESPACE {
thread_local std::string g_err;
std::recursive_mutex g_api_lock;
}  // namespace dfe
using namespace dfe;

// ---- packed-operand blob: ONE packing on the root rank, one broadcast, no fp32 masters and no re-pack elsewhere ------
namespace {
struct BlobW {
  std::vector<char> m;
  template <class T> void put(T v) { const char* p = (const char*)&v; m.insert(m.end(), p, p + sizeof(T)); }
  void str(const std::string& s) { put<uint16_t>((uint16_t)s.size()); m.insert(m.end(), s.begin(), s.end()); }
};
struct BlobR {
  const char* p; const char* e;
  template <class T> T get() { if (p + sizeof(T) > e) fail("packed manifest truncated"); T v; memcpy(&v, p, sizeof(T)); p += sizeof(T); return v; }
  std::string str() { const uint16_t n = get<uint16_t>(); if (p + n > e) fail("packed manifest truncated"); std::string s(p, p + n); p += n; return s; }
};
constexpr uint32_t kBlobMagic = 0x44464250u;   // "DFBP"
// fp32 tensors up to this many elements travel as data (biases, norm parameters, pos_emb, post_quant_conv); larger ones as
// shape only.  DF_RAW_DATA_MAX (tests): a smaller bound, so that a tiny model's weight matrices are shape-only as well.
static size_t raw_data_max() {
  static const size_t v = getenv("DF_RAW_DATA_MAX") ? (size_t)atol(getenv("DF_RAW_DATA_MAX")) : 65536;
  return v;
}
#define kRawDataMax raw_data_max()
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// Layout shared by size / export: raw entries (sorted by name) first, then packed entries (sorted by key).
size_t blob_layout(df_ctx* c, BlobW* w) {
  size_t off = 0;
  if (w) {
    w->put<uint32_t>(kBlobMagic); w->put<uint32_t>(1);
#if defined(DF_OPERAND_F16)
    w->put<uint32_t>(1);
#else
    w->put<uint32_t>(0);
#endif
    w->put<uint32_t>((uint32_t)c->raw.size()); w->put<uint32_t>((uint32_t)c->packed.size());
  }
  for (auto& kv : c->raw) {
    const RawT& t = kv.second;
    const bool data = t.d != nullptr && t.n <= kRawDataMax;
    if (w) {
      w->str(kv.first); w->put<uint8_t>((uint8_t)t.shape.size());
      for (int64_t d : t.shape) w->put<int64_t>(d);
      w->put<uint8_t>(data ? 1 : 0); w->put<uint64_t>((uint64_t)off);
    }
    if (data) off += al256(t.n * 4);
  }
  for (auto& kv : c->packed) {
    auto it = c->block_bytes.find(kv.second);
    if (it == c->block_bytes.end()) fail("packed entry '%s' has no recorded size", kv.first.c_str());
    if (w) { w->str(kv.first); w->put<uint64_t>((uint64_t)it->second); w->put<uint64_t>((uint64_t)off); }
    off += al256(it->second);
  }
  return off;
}
}  // namespace

// ================================================================================================== C ABI
extern "C" {

// Sizes that come straight from the caller's tensors: an empty batch / map / sequence has no plan (several builders divide by these)
static void need_positive(const char* what, std::initializer_list<std::pair<const char*, long>> dims) {
  for (auto& d : dims)
    if (d.second <= 0) fail("%s: %s = %ld (empty input: every size must be positive)", what, d.first, d.second);
}
static void need_pointers(const char* what, std::initializer_list<std::pair<const char*, const void*>> ptrs) {
  for (auto& p : ptrs)
    if (!p.second) fail("%s: %s is a null pointer", what, p.first);
}

int df_abi_version(void) { return 1; }
const char* df_operand_dtype(void) {
#if defined(DF_OPERAND_F16)
  return "f16";
#else
  return "bf16";
#endif
}
const char* df_last_error(void) { return g_err.c_str(); }

int df_create(int device, df_ctx** out) {
  return guard([&] {
    HIPCHK(hipSetDevice(device));
    df_ctx* c = new df_ctx();
    c->device = device;
    HIPCHK(hipStreamCreateWithFlags(&c->pack_stream, hipStreamNonBlocking));
    *out = c;
  });
}

void df_destroy(df_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  if (ctx->pack_stream) (void)hipStreamDestroy(ctx->pack_stream);
  delete ctx;
}

int df_config_unet(df_ctx* c, const df_unet_config* cfg) { return guard([&] { c->ucfg = *cfg; c->has_unet = true; }); }
int df_config_vae(df_ctx* c, const df_vae_config* cfg) { return guard([&] { c->vcfg = *cfg; c->has_vae = c->has_vae_shape = true; }); }
int df_config_vae_encoder(df_ctx* c, const df_vae_encoder_config* cfg) {
  return guard([&] {
    c->has_vae_enc = cfg != nullptr;
    c->ecfg = cfg ? *cfg : df_vae_encoder_config{};
  });
}
// A context that encodes and never decodes (the Align-Acc metric model): the encoder's shape comes with the call, the decoder stays
// unconfigured -- df_vae_decode refuses, df_prepack packs no decoder, and no decoder tensor is asked for.
int df_config_vae_encoder_only(df_ctx* c, const df_vae_config* vae, const df_vae_encoder_config* enc) {
  return guard([&] {
    if (!vae || !enc) fail("df_config_vae_encoder_only: null configuration");
    c->vcfg = *vae;
    c->has_vae = false;
    c->has_vae_shape = true;
    c->has_vae_enc = true;
    c->ecfg = *enc;
  });
}
int df_config_cond(df_ctx* c, const df_cond_config* cfg) { return guard([&] { c->kcfg = *cfg; c->has_cond = true; }); }
int df_config_cavp(df_ctx* c, const df_cavp_config* cfg) { return guard([&] { c->pcfg = *cfg; c->has_cavp = true; }); }
int df_config_classifier(df_ctx* c, const df_unet_config* cfg) { return guard([&] { c->ccfg = *cfg; c->has_cls = true; }); }

static void load_common(df_ctx* c, const char* name, const float* src, const int64_t* shape, int ndim, hipMemcpyKind kind) {
  HIPCHK(hipSetDevice(c->device));
  RawT t;
  t.n = 1;
  for (int i = 0; i < ndim; ++i) {
    t.shape.push_back(shape[i]);
    t.n *= (size_t)shape[i];
  }
  auto it = c->raw.find(name);
  if (it != c->raw.end()) {
    HIPCHK(hipDeviceSynchronize());       // plans of the old weights may still be running
    (void)hipFree(it->second.d);
    c->raw.erase(it);
    c->reloaded = true;
  }
  HIPCHK(hipMalloc((void**)&t.d, ((t.n * 4) + 255) & ~(size_t)255));
  HIPCHK(hipMemcpy(t.d, src, t.n * 4, kind));
  c->raw[name] = t;
}

int df_load_tensor(df_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
  return guard([&] { load_common(c, name, host, shape, ndim, hipMemcpyHostToDevice); });
}
int df_load_tensor_dev(df_ctx* c, const char* name, const float* dev, const int64_t* shape, int ndim) {
  return guard([&] { load_common(c, name, dev, shape, ndim, hipMemcpyDeviceToDevice); });
}

int df_finalize(df_ctx* c) {
  return guard([&] {
    HIPCHK(hipSetDevice(c->device));
    if (c->has_unet) build_emb_table(c, 0);
    if (c->has_cls) build_emb_table(c, 1);
    if (c->has_vae_enc) {      // the encoder is configured only by a caller that loads its tensors: every one of them has to be there
      if (!c->has_vae_shape)
        fail("vae encoder configured without df_config_vae / df_config_vae_encoder_only (it shares the decoder's ch / ch_mult / z_channels)");
      for (auto& n : vae_encoder_tensor_names(c)) (void)c->rt(n);
    }
    HIPCHK(hipDeviceSynchronize());
    c->plans.clear();
    if (c->reloaded) {     // every packed operand copy (casts, GEGLU / LN-folded / BN-folded / stacked packings) is rebuilt
      for (void* p : c->packed_blocks) (void)hipFree(p);
      c->packed_blocks.clear();
      c->block_bytes.clear();
      c->packed.clear();
      if (c->ctx_copy) (void)hipFree(c->ctx_copy);
      c->ctx_copy = nullptr;
      c->ctx_copy_bytes = 0;
      c->ctx_N = c->ctx_T = 0;
      c->reloaded = false;
    }
    c->last_unet = nullptr;
    c->finalized = true;
  });
}

int df_autotune(df_ctx* c, int enable) {
  return guard([&] {
    if (enable && c->poison_on) fail("df_autotune: df_debug_poison is on (the tuner re-runs ops out of plan order, which poisoned workspaces do not survive)");
    c->autotune = enable != 0;
  });
}

int df_cavp_encode(df_ctx* c, const float* video, float* out, int B, int T, int H, int W, int normalize, void* stream) {
  return guard([&] {
    if (!c->has_cavp) fail("cavp encoder not configured");
    need_positive("cavp", {{"clips", B}, {"frames", T}, {"H", H}, {"W", W}});
    Plan* p = get_plan(c, keyf("cavp_%d_%d_%d", T, H, W), [&](Plan* pl) { build_cavp(c, pl, T, H, W); });
    for (int i = 0; i < B; ++i) {      // clips are independent (temporal padding is per clip): one plan run each
      RunArgs a;
      a.x = video + (size_t)i * T * 3 * H * W;
      a.out = out + (size_t)i * T * c->pcfg.embed_dim;
      a.scale = normalize ? 1.f : 0.f;
      run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
    }
  });
}

int df_cavp_pool(const float* feat, float* out, int B, int T, int C, int kernel, int normalize, void* stream) {
  return guard([&] {
    need_positive("cavp pool", {{"clips", B}, {"frames", T}, {"channels", C}, {"kernel", kernel}});
    HIPCHK(launch_maxpool_time(feat, out, B, T, C, kernel, (hipStream_t)stream));
    if (normalize) HIPCHK(launch_l2norm_rows(out, B * (T / kernel), C, (hipStream_t)stream));
  });
}

int df_config_cavp_spec(df_ctx* c, const df_cavp_spec_config* cfg) {
  return guard([&] {
    if (!cfg) fail("cavp spec: null configuration");
    c->scfg = *cfg;
    c->has_cavp_spec = true;
  });
}

// T' of a T-frame mel: four floor-halvings (the (2, 2) pools of conv_block1 .. 4)
static int cavp_spec_rows(int T) { return T / 2 / 2 / 2 / 2; }

// clips per plan: the widest operand (conv_block1's full-resolution map) stays far below the 2 GiB operand addressing
static int cavp_spec_chunk(const df_ctx* c, int T, int n_mels) {
  const size_t per_clip = (size_t)T * n_mels * (size_t)std::max(c->scfg.channels[0], 1) * 2;
  const int chunk = (int)std::max<size_t>(1, ((size_t)1 << 30) / std::max<size_t>(per_clip, 1));
  return std::min(chunk, 16);
}

static void cavp_spec_check(df_ctx* c, const char* what, int B, int n_mels, int T) {
  if (!c->has_cavp_spec) fail("cavp spectrogram encoder not configured (df_config_cavp_spec, with the spec_encoder tensors loaded)");
  need_positive(what, {{"clips", B}, {"mel bins", n_mels}, {"frames", T}});
  if (n_mels != c->scfg.n_mels) fail("%s: the mel has %d bins, the encoder is configured for %d", what, n_mels, c->scfg.n_mels);
  if (cavp_spec_rows(T) < 1) fail("%s: %d frames give no output row (16 frames make one)", what, T);
}

int df_cavp_spec_encode(df_ctx* c, const float* spec, float* out, int B, int n_mels, int T, int normalize, void* stream) {
  return guard([&] {
    cavp_spec_check(c, "cavp spec", B, n_mels, T);
    need_pointers("cavp spec", {{"spec", spec}, {"out", out}});
    const int chunk = cavp_spec_chunk(c, T, n_mels), To = cavp_spec_rows(T);
    for (int b0 = 0; b0 < B; b0 += chunk) {
      const int nb = std::min(chunk, B - b0);
      Plan* p = get_plan(c, keyf("cavpspec_%d_%d_%d", nb, T, n_mels), [&](Plan* pl) { build_cavp_spec(c, pl, nb, T, n_mels); });
      RunArgs a;
      a.x = spec + (size_t)b0 * n_mels * T;
      a.out = out + (size_t)b0 * To * c->scfg.embed_dim;
      a.scale = normalize ? 1.f : 0.f;
      run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
    }
  });
}

int df_cavp_similarity(const float* v, const float* s, float* out, int Bv, int Bs, int T, int D, float scale, void* stream) {
  return guard([&] {
    need_positive("cavp similarity", {{"video clips", Bv}, {"audio clips", Bs}, {"frames", T}, {"feature width", D}});
    need_pointers("cavp similarity", {{"v", v}, {"s", s}, {"out", out}});
    if (D % 4) fail("cavp similarity: feature width %d is not a multiple of 4", D);
    HIPCHK(launch_cavp_similarity(v, s, out, Bv, Bs, T, D, scale, (hipStream_t)stream));
  });
}

int df_cond_encode(df_ctx* c, const float* feats, float* out, int B, int T, void* stream) {
  return guard([&] {
    if (!c->has_cond) fail("cond stage not configured");
    need_positive("cond stage", {{"batch", B}, {"sequence length", T}});
    Plan* p = get_plan(c, keyf("cond_%d_%d", B, T), [&](Plan* pl) { build_cond(c, pl, B, T); });
    RunArgs a;
    a.x = feats;
    a.out = out;
    run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
  });
}

static Plan* unet_plan(df_ctx* c, int N, int H, int W, int T, bool cfg) {
  if (!c->has_unet) fail("unet not configured");
  need_positive("unet", {{"batch", N}, {"H", H}, {"W", W}, {"context length", T}});
  if (H % (1 << (c->ucfg.n_mult - 1)) || W % (1 << (c->ucfg.n_mult - 1))) fail("latent %dx%d not divisible by the UNet downsampling", H, W);
  return get_plan(c, keyf("unet_%d_%d_%d_%d_%d", N, H, W, T, (int)cfg),
                  [&](Plan* pl) { build_unet_like(c, pl, 0, N, H, W, T, cfg); });
}

int df_unet_set_context(df_ctx* c, const float* context, int N, int T, void* stream) {
  return guard([&] {
    need_positive("unet context", {{"batch", N}, {"context length", T}});
    c->ctx_N = N;
    c->ctx_T = T;
    // the context K/V live inside each forward plan; remember the pointer and (re)run the context ops lazily
    // for every plan that is used with this context.  Simple and exact: stash the pointer, mark plans stale.
    RunArgs a;
    a.aux = context;
    for (auto& kv : c->plans) {
      if (kv.first.rfind("unet_", 0) != 0) continue;
      int n, h, w, t, g;
      if (sscanf(kv.first.c_str(), "unet_%d_%d_%d_%d_%d", &n, &h, &w, &t, &g) == 5 && n == N && t == T)
        run_ops(c, kv.second.get(), 0, kv.second->n_ctx, (hipStream_t)stream, a);
    }
    // keep a device copy so plans created later can still be primed
    const size_t bytes = (size_t)N * T * c->ucfg.context_dim * 4;
    if (bytes > c->ctx_copy_bytes) {     // grow-only scratch, NOT a packed operand: freed here, never exported
      if (c->ctx_copy) {
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        (void)hipFree(c->ctx_copy);
      }
      HIPCHK(hipMalloc((void**)&c->ctx_copy, (bytes + 255) & ~(size_t)255));
      c->ctx_copy_bytes = bytes;
    }
    HIPCHK(hipMemcpyAsync(c->ctx_copy, context, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  });
}

static void unet_run(df_ctx* c, const float* x, const float* t, float* out, int N, int H, int W, bool cfg, float scale,
                     hipStream_t s, int ts_index = -1) {
  if (c->ctx_N != N) fail("context has %d rows but the UNet batch is %d (call df_unet_set_context first)", c->ctx_N, N);
  const std::string key = keyf("unet_%d_%d_%d_%d_%d", N, H, W, c->ctx_T, (int)cfg);
  const bool fresh = c->plans.count(key) == 0;
  Plan* p = unet_plan(c, N, H, W, c->ctx_T, cfg);
  const size_t nctx = p->n_ctx;
  RunArgs a;
  a.x = x;
  a.t = t;
  a.out = out;
  a.scale = scale;
  if (fresh) {  // plan created after set_context: prime its K/V from the saved context copy
    a.aux = c->ctx_copy;
    run_ops(c, p, 0, nctx, s, a);
  }
  if (ts_index >= 0) {       // announced timestep: one table look-up instead of the time-embedding ops
    if (p->op_tl < 0 || !p->Etab) fail("no timestep table for this UNet plan (call df_unet_set_timesteps after df_unet_set_context)");
    if (ts_index >= p->etab_S) fail("timestep index %d outside the table of %d steps", ts_index, p->etab_S);
    a.ts_index = ts_index;
    run_ops(c, p, (size_t)p->op_tl, p->ops.size(), s, a);
  } else if (p->op_tl >= 0) {
    run_ops(c, p, nctx, (size_t)p->op_tl, s, a);
    run_ops(c, p, (size_t)p->op_tl + 1, p->ops.size(), s, a);
  } else {
    run_ops(c, p, nctx, p->ops.size(), s, a);
  }
  c->last_unet = p;
  c->last_unet_hoisted = ts_index >= 0;
}

// Time embedding of every step of a sample() call, once, before the loop (it depends on t only; the reference
// recomputes it inside every UNet call, openai_unetmodel.py:724).  t_host[S] = the timesteps the sampler is going to visit, the
// same value for every sample of the batch (ddim.py:217 `ts = torch.full((b,), step)`).  Runs the plan's own time-embedding ops
// per step, so a table row is bit-identical to what the step would have computed in place.
static void unet_set_timesteps(df_ctx* c, const float* t_host, int S, int N, int H, int W, bool cfg, hipStream_t s) {
  if (S <= 0) fail("df_unet_set_timesteps: no timesteps");
  if (c->ctx_N != N) fail("context has %d rows but the UNet batch is %d (call df_unet_set_context first)", c->ctx_N, N);
  const std::string key = keyf("unet_%d_%d_%d_%d_%d", N, H, W, c->ctx_T, (int)cfg);
  const bool fresh = c->plans.count(key) == 0;
  Plan* p = unet_plan(c, N, H, W, c->ctx_T, cfg);
  if (p->op_tl < 0) fail("this UNet plan has no hoistable time embedding");
  RunArgs a;
  if (fresh) {
    a.aux = c->ctx_copy;
    run_ops(c, p, 0, p->n_ctx, s, a);
  }
  // The same timesteps as the table already holds (every sample() call of a service announces the same 25 / 50 steps): nothing to do --
  // the table lives with the plan, and a plan does not survive a weight reload (round 6: 7 runs of the time ops + a host
  // synchronisation per sample() call gone).
  if (p->Etab && p->etab_S == S && p->etab_t.size() == (size_t)S && std::equal(p->etab_t.begin(), p->etab_t.end(), t_host)) return;
  p->etab_t.clear();
  if (S > p->etab_cap) {
    HIPCHK(hipStreamSynchronize(s));
    if (p->Etab) (void)hipFree(p->Etab);
    if (p->ttab) (void)hipFree(p->ttab);
    p->Etab = p->ttab = nullptr;
    p->etab_cap = 0;
    HIPCHK(hipMalloc((void**)&p->Etab, (size_t)S * p->etot * 4));
    HIPCHK(hipMalloc((void**)&p->ttab, (size_t)S * p->t_rows * 4));
    p->etab_cap = S;
  }
  std::vector<float> tt((size_t)S * p->t_rows);      // S timesteps, then padding (the last timestep repeated) for the last run
  for (size_t i = 0; i < tt.size(); ++i) tt[i] = t_host[std::min<size_t>(i, (size_t)S - 1)];
  HIPCHK(hipMemcpyAsync(p->ttab, tt.data(), tt.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));       // tt leaves scope
  p->etab_S = 0;
  // The time ops map t_rows timesteps to t_rows rows of E, row by row (the embedding kernel and the three GEMMs are row-independent;
  // with CFG the second half of E repeats the first): one run of them serves t_rows DIFFERENT timesteps, so the table takes
  // ceil(S / t_rows) runs, not S (round 5: 7 instead of 25 for B = 4 -- the 52 MB of emb-projection weights are streamed 7 times per
  // sample() call instead of 25).  Row r of a run is bit-identical to the in-step form's row for that timestep.
  const int tr = std::max(p->t_rows, 1);
  for (int i = 0; i < S; i += tr) {
    const int nrow = std::min(tr, S - i);
    a.t = p->ttab + (size_t)i;          // ttab, read as S consecutive timesteps (the tail of the last run reads into the padding)
    run_ops(c, p, (size_t)p->op_t0, (size_t)p->op_tl, s, a);
    HIPCHK(hipMemcpyAsync(p->Etab + (size_t)i * p->etot, p->E, (size_t)nrow * p->etot * 4, hipMemcpyDeviceToDevice, s));
  }
  p->etab_S = S;
  p->etab_t.assign(t_host, t_host + S);
}

int df_unet_forward(df_ctx* c, const float* x, const float* t, float* out, int N, int H, int W, void* stream) {
  return guard([&] { unet_run(c, x, t, out, N, H, W, false, 1.f, (hipStream_t)stream); });
}

int df_unet_forward_cfg(df_ctx* c, const float* x, const float* t, float* out, int B, int H, int W, float scale,
                        void* stream) {
  return guard([&] { unet_run(c, x, t, out, 2 * B, H, W, true, scale, (hipStream_t)stream); });
}

int df_unet_set_timesteps(df_ctx* c, const float* t_host, int S, int N, int H, int W, int cfg, void* stream) {
  return guard([&] { unet_set_timesteps(c, t_host, S, cfg ? 2 * N : N, H, W, cfg != 0, (hipStream_t)stream); });
}

int df_unet_forward_ts(df_ctx* c, const float* x, int ts_index, float* out, int N, int H, int W, void* stream) {
  return guard([&] {
    if (ts_index < 0) fail("df_unet_forward_ts: negative timestep index");
    unet_run(c, x, nullptr, out, N, H, W, false, 1.f, (hipStream_t)stream, ts_index);
  });
}

int df_unet_forward_cfg_ts(df_ctx* c, const float* x, int ts_index, float* out, int B, int H, int W, float scale, void* stream) {
  return guard([&] {
    if (ts_index < 0) fail("df_unet_forward_cfg_ts: negative timestep index");
    unet_run(c, x, nullptr, out, 2 * B, H, W, true, scale, (hipStream_t)stream, ts_index);
  });
}

// One GEMM operand is addressed with 32-bit buffer offsets (< 2 GiB): the decoder's widest activation is 8H x 8W pixels x
// 2*ch channels per sample, so large batches run as slices of at most this many samples (shared by df_vae_decode / df_prepack).
static int vae_chunk(df_ctx* c, int H, int W) {
  const size_t per_sample = (size_t)(H << (c->vcfg.n_mult - 1)) * (W << (c->vcfg.n_mult - 1)) * (size_t)c->vcfg.ch * 2 * 2;
  const int chunk = (int)std::max<size_t>(1, (((size_t)1 << 31) - 1) / std::max<size_t>(per_sample, 1));
  return std::min(chunk, 16);
}

int df_vae_decode(df_ctx* c, const float* z, float* out, int B, int H, int W, void* stream) {
  return guard([&] {
    if (!c->has_vae) fail("vae not configured");
    need_positive("vae decode", {{"batch", B}, {"H", H}, {"W", W}});
    // One GEMM operand is addressed with 32-bit buffer offsets (< 2 GiB): the decoder's widest activation is
    // 8 x H x 8 x W pixels x 2*ch channels per sample, so large batches run as slices of at most `chunk` samples through
    // the plan of that size (same kernels, same results; no host round trip between slices).
    const int chunk = vae_chunk(c, H, W);
    const int zc = c->vcfg.z_channels, up = 1 << (c->vcfg.n_mult - 1);
    for (int b0 = 0; b0 < B; b0 += chunk) {
      const int nb = std::min(chunk, B - b0);
      Plan* p = get_plan(c, keyf("vae_%d_%d_%d", nb, H, W), [&](Plan* pl) { build_vae(c, pl, nb, H, W); });
      RunArgs a;
      a.x = z + (size_t)b0 * zc * H * W;
      a.out = out + (size_t)b0 * c->vcfg.out_ch * (H * up) * (W * up);
      run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
    }
  });
}

// The encoder's widest operand is the full-resolution map x ch channels (2 ch at half resolution is half of that); the bound below is
// the decoder's (2 ch at full resolution), so both directions slice a batch the same way.
static int vae_encode_chunk(df_ctx* c, int H, int W) {
  const size_t per_sample = (size_t)H * W * (size_t)c->vcfg.ch * 2 * 2;
  const int chunk = (int)std::max<size_t>(1, (((size_t)1 << 31) - 1) / std::max<size_t>(per_sample, 1));
  return std::min(chunk, 16);
}

int df_vae_encode(df_ctx* c, const float* x, float* moments, int B, int H, int W, void* stream) {
  return guard([&] {
    if (!c->has_vae_shape || !c->has_vae_enc) fail("vae encoder not configured (df_config_vae_encoder, with the encoder's tensors loaded)");
    need_positive("vae encode", {{"batch", B}, {"H", H}, {"W", W}});
    const int f = 1 << (c->vcfg.n_mult - 1);
    // torch's padded stride-2 convs floor an odd map; this engine sizes every level as H / 2 and refuses what does not divide
    if (H % f || W % f) fail("vae encode: image %dx%d is not a multiple of the encoder's downsampling (%d)", H, W, f);
    const int chunk = vae_encode_chunk(c, H, W);
    const int cin = c->ecfg.in_channels, mc = 2 * c->vcfg.embed_dim;
    for (int b0 = 0; b0 < B; b0 += chunk) {
      const int nb = std::min(chunk, B - b0);
      Plan* p = get_plan(c, keyf("vaeenc_%d_%d_%d", nb, H, W), [&](Plan* pl) { build_vae_encoder(c, pl, nb, H, W); });
      RunArgs a;
      a.x = x + (size_t)b0 * cin * H * W;
      a.out = moments + (size_t)b0 * mc * (H / f) * (W / f);
      run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
    }
  });
}

// The engine sizes every Downsample output as floor(H / 2) x floor(W / 2) where torch's stride-2 conv gives the ceiling, and its
// backward has no odd-size transposed conv: a map that does not survive the downsampling is refused, as unet_plan does.
static void cls_need_divisible(df_ctx* c, int H, int W) {
  const int ds = 1 << (c->ccfg.n_mult - 1);
  if (H % ds || W % ds) fail("classifier: latent %dx%d not divisible by the classifier's downsampling (%d)", H, W, ds);
}

int df_classifier_forward(df_ctx* c, const float* x, const float* t, const float* feat, float* prob, int B, int H,
                          int W, int T, void* stream) {
  return guard([&] {
    if (!c->has_cls) fail("classifier not configured");
    need_positive("classifier", {{"batch", B}, {"H", H}, {"W", W}, {"video frames", T}});
    cls_need_divisible(c, H, W);
    Plan* p = get_plan(c, keyf("cls_%d_%d_%d_%d", B, H, W, T),
                       [&](Plan* pl) { build_unet_like(c, pl, 1, B, H, W, T, false); });
    RunArgs a;
    a.x = x;
    a.t = t;
    a.aux = feat;
    a.out = prob;
    run_ops(c, p, 0, p->ops.size(), (hipStream_t)stream, a);
  });
}

int df_classifier_grad_cached(df_ctx* c, const float* x, const float* t, const float* feat, float* prob, float* grad, int B,
                              int H, int W, int T, uint64_t feat_token, void* stream) {
  return guard([&] {
    if (!c->has_cls) fail("classifier not configured");
    need_positive("classifier gradient", {{"batch", B}, {"H", H}, {"W", W}, {"video frames", T}});
    cls_need_divisible(c, H, W);
    Plan* p = get_plan(c, keyf("clsgrad_%d_%d_%d_%d", B, H, W, T), [&](Plan* pl) { build_classifier_grad(c, pl, B, H, W, T); });
    RunArgs a;
    a.x = x;
    a.t = t;
    a.aux = feat;
    a.out = grad;
    a.out2 = prob;
    // the plan, not the caller, knows whether its K / V^T buffers hold these features: a plan rebuilt since the last call
    // (other shape, dropped plans, reloaded weights) starts at token 0 and recomputes
    const bool reuse = feat_token != 0 && p->feat_token == feat_token;
    if (!reuse) p->feat_token = 0;        // a failing launch below must not leave a token on half-written buffers
    run_ops(c, p, reuse ? p->n_feat : 0, p->ops.size(), (hipStream_t)stream, a);
    p->feat_token = feat_token;
  });
}

int df_classifier_grad(df_ctx* c, const float* x, const float* t, const float* feat, float* prob, float* grad, int B,
                       int H, int W, int T, void* stream) {
  return df_classifier_grad_cached(c, x, t, feat, prob, grad, B, H, W, T, 0, stream);
}

// ---- packed-operand blob (helpers above the C ABI block)

int df_prepack(df_ctx* c, int B, int H, int W, int T) {
  return guard([&] {
    HIPCHK(hipSetDevice(c->device));
    if (c->has_unet) (void)unet_plan(c, 2 * B, H, W, T, true);
    if (c->has_vae) {     // the plans df_vae_decode will actually run: slices of at most vae_chunk() samples + the remainder
      const int chunk = vae_chunk(c, H, W);
      for (int nb : {std::min(B, chunk), B % chunk})
        if (nb > 0) (void)get_plan(c, keyf("vae_%d_%d_%d", nb, H, W), [&](Plan* pl) { build_vae(c, pl, nb, H, W); });
    }
    if (c->has_cond) (void)get_plan(c, keyf("cond_%d_%d", B, T), [&](Plan* pl) { build_cond(c, pl, B, T); });
    HIPCHK(hipStreamSynchronize(c->pack_stream));
  });
}

int df_packed_size(df_ctx* c, size_t* manifest_bytes, size_t* blob_bytes) {
  return guard([&] {
    BlobW w;
    *blob_bytes = blob_layout(c, &w);
    *manifest_bytes = w.m.size();
  });
}

int df_export_packed(df_ctx* c, void* manifest_host, void* blob_dev, void* stream) {
  return guard([&] {
    HIPCHK(hipSetDevice(c->device));
    BlobW w;
    (void)blob_layout(c, &w);
    memcpy(manifest_host, w.m.data(), w.m.size());
    hipStream_t s = (hipStream_t)stream;
    size_t off = 0;
    for (auto& kv : c->raw) {
      const RawT& t = kv.second;
      if (t.d == nullptr || t.n > kRawDataMax) continue;
      HIPCHK(hipMemcpyAsync((char*)blob_dev + off, t.d, t.n * 4, hipMemcpyDeviceToDevice, s));
      off += al256(t.n * 4);
    }
    for (auto& kv : c->packed) {
      const size_t b = c->block_bytes.at(kv.second);
      HIPCHK(hipMemcpyAsync((char*)blob_dev + off, kv.second, b, hipMemcpyDeviceToDevice, s));
      off += al256(b);
    }
  });
}

int df_import_packed(df_ctx* c, const void* manifest_host, size_t manifest_bytes, const void* blob_dev, size_t blob_bytes,
                     void* stream) {
  return guard([&] {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    BlobR r{(const char*)manifest_host, (const char*)manifest_host + manifest_bytes};
    if (r.get<uint32_t>() != kBlobMagic || r.get<uint32_t>() != 1) fail("not a libdfengine packed manifest");
    const uint32_t op = r.get<uint32_t>();
#if defined(DF_OPERAND_F16)
    if (op != 1) fail("packed blob holds bf16 operands, this library is the fp16 build");
#else
    if (op != 0) fail("packed blob holds fp16 operands, this library is the bf16 build");
#endif
    const uint32_t nraw = r.get<uint32_t>(), npk = r.get<uint32_t>();
    for (uint32_t i = 0; i < nraw; ++i) {
      const std::string name = r.str();
      RawT t;
      t.n = 1;
      const int nd = r.get<uint8_t>();
      for (int k = 0; k < nd; ++k) { t.shape.push_back(r.get<int64_t>()); t.n *= (size_t)t.shape.back(); }
      const bool data = r.get<uint8_t>() != 0;
      const uint64_t off = r.get<uint64_t>();
      auto it = c->raw.find(name);
      if (it != c->raw.end()) { (void)hipFree(it->second.d); c->raw.erase(it); c->reloaded = true; }
      if (data) {
        if (off + t.n * 4 > blob_bytes) fail("packed blob too small for '%s'", name.c_str());
        HIPCHK(hipMalloc((void**)&t.d, al256(t.n * 4)));
        HIPCHK(hipMemcpyAsync(t.d, (const char*)blob_dev + off, t.n * 4, hipMemcpyDeviceToDevice, s));
      }
      c->raw[name] = t;
    }
    if (c->reloaded) fail("df_import_packed into a context that already holds these tensors (create a fresh context)");
    for (uint32_t i = 0; i < npk; ++i) {
      const std::string key = r.str();
      const uint64_t b = r.get<uint64_t>(), off = r.get<uint64_t>();
      if (off + b > blob_bytes) fail("packed blob too small for '%s'", key.c_str());
      void* p = c->pmalloc((size_t)b);
      HIPCHK(hipMemcpyAsync(p, (const char*)blob_dev + off, (size_t)b, hipMemcpyDeviceToDevice, s));
      c->packed[key] = p;
    }
    HIPCHK(hipStreamSynchronize(s));
  });
}

int df_frames_to_tensor(const uint8_t* frames, float* out, uint8_t* tmp, int T, int H, int W, int OH, int OW,
                        const int32_t* bounds_w, const int32_t* coef_w, int ksize_w, const int32_t* bounds_h,
                        const int32_t* coef_h, int ksize_h, void* stream) {
  return guard([&] {
    need_positive("frames_to_tensor", {{"frames", T}, {"H", H}, {"W", W}, {"out H", OH}, {"out W", OW}});
    HIPCHK(launch_frames_to_tensor(frames, out, tmp, T, H, W, OH, OW, bounds_w, coef_w, ksize_w, bounds_h, coef_h, ksize_h,
                                   (hipStream_t)stream));
  });
}

int df_mel_to_stft(const float* mel, int B, int n_mels, int T, const float* A, const float* At, const float* Pt, float inv_L,
                   int iters, float* S, void* stream) {
  return guard([&] {
    need_positive("mel_to_stft", {{"clips", B}, {"mel bins", n_mels}, {"frames", T}});
    if (n_mels > 128) fail("mel_to_stft: n_mels = %d (the kernel's span tables hold at most 128 rows)", n_mels);
    if (iters < 0) fail("mel_to_stft: iters = %d (a count of FISTA iterations, 0 or more)", iters);
    need_pointers("mel_to_stft", {{"mel", mel}, {"A", A}, {"At", At}, {"Pt", Pt}, {"S", S}});
    HIPCHK(launch_mel_to_stft(mel, B, n_mels, T, A, At, Pt, inv_L, iters, S, (hipStream_t)stream));
  });
}
int df_griffinlim(const float* S, const float* phase0, int B, int T, int n_iter, float momentum, const float* twiddles,
                  const float* window, const float* wss, float* angles, float* reb0, float* reb1, float* frames, float* wav,
                  void* stream) {
  return guard([&] {
    need_positive("griffinlim", {{"clips", B}, {"frames", T}});
    if (T < 2) fail("griffinlim: T = %d (one frame is zero hops of audio: at least 2 frames)", T);
    if (n_iter < 0) fail("griffinlim: n_iter = %d (a count of iterations, 0 or more)", n_iter);
    if (!(momentum >= 0.f && momentum < 1.f)) fail("griffinlim: momentum = %g (expected 0 <= momentum < 1)", (double)momentum);
    need_pointers("griffinlim", {{"S", S}, {"phase0", phase0}, {"twiddles", twiddles}, {"window", window}, {"wss", wss},
                                 {"angles", angles}, {"reb0", reb0}, {"reb1", reb1}, {"frames", frames}, {"wav", wav}});
    HIPCHK(launch_griffinlim(S, phase0, B, T, n_iter, momentum, (const float2*)twiddles, window, wss, (float2*)angles,
                             (float2*)reb0, (float2*)reb1, frames, wav, (hipStream_t)stream));
  });
}

int df_wave_to_mel(const float* wav, int64_t wav_stride, int B, int L, const float* A, const int32_t* bands, int n_mels,
                   const float* twiddles, const float* window, float floor, float* mel, void* stream) {
  return guard([&] {
    need_positive("wave_to_mel", {{"clips", B}, {"samples", L}, {"mel bins", n_mels}});
    if (n_mels > 128) fail("wave_to_mel: %d mel bins (the kernel holds at most 128 rows per tile)", n_mels);
    if (wav_stride < L) fail("wave_to_mel: row stride %ld is shorter than a clip of %d samples", (long)wav_stride, L);
    if (!wav || !A || !bands || !twiddles || !window || !mel) fail("wave_to_mel: null pointer argument");
    HIPCHK(launch_wave_to_mel(wav, (long)wav_stride, B, L, A, bands, n_mels, (const float2*)twiddles, window, floor, mel,
                              (hipStream_t)stream));
  });
}
int df_wave_to_mel_tile(void) { return wave_to_mel_tile(); }

int df_cfg_combine(const float* e2, float* e, int64_t n, float scale, void* stream) {
  return guard([&] { HIPCHK(launch_cfg_combine(e2, e, (long)n, scale, (hipStream_t)stream)); });
}
int df_lincomb(float* out, const float* const* in, const float* coef, int nterms, int64_t n, void* stream) {
  return guard([&] { HIPCHK(launch_lincomb(out, in, coef, nterms, (long)n, (hipStream_t)stream)); });
}
int df_posterior_sample(const float* moments, const float* noise, float* z, int B, int zc, int HW, float scale, void* stream) {
  return guard([&] {
    need_positive("posterior sample", {{"batch", B}, {"channels", zc}, {"H*W", HW}});
    HIPCHK(launch_posterior_sample(moments, noise, z, B, zc, (long)HW, scale, (hipStream_t)stream));
  });
}
int df_align_verdict(const float* prob, const float* labels, float* pred, int64_t* counts, int B, void* stream) {
  return guard([&] {
    need_positive("align verdict", {{"batch", B}});
    if (!prob || !pred || !counts) fail("align verdict: null pointer argument");
    HIPCHK(launch_align_verdict(prob, labels, pred, (long long*)counts, B, (hipStream_t)stream));
  });
}
int df_q_sample_blend(const float* img, const float* x0, const float* noise, const float* mask, float* out, int64_t n, int64_t chw,
                      int64_t hw, int mask_c, float sqrt_acp, float sqrt_one_minus_acp, void* stream) {
  return guard([&] {
    HIPCHK(launch_q_sample_blend(img, x0, noise, mask, out, (long)n, (long)chw, (long)hw, mask_c, sqrt_acp, sqrt_one_minus_acp,
                                 (hipStream_t)stream));
  });
}
int df_q_sample(const float* x0, const float* noise, const int64_t* t, const float* A, const float* S, float* out, int B, int64_t n,
                int T, void* stream) {
  return guard([&] {
    need_positive("q_sample", {{"batch", B}, {"table length", T}});
    if (n < 1) fail("q_sample: %ld elements per sample (at least 1)", (long)n);
    if (!x0 || !noise || !t || !A || !S || !out) fail("q_sample: null pointer argument");
    HIPCHK(launch_q_sample(x0, noise, (const long long*)t, A, S, out, B, (long)n, T, (hipStream_t)stream));
  });
}
int df_diffusion_loss(const float* pred, const float* target, const int64_t* t, const float* logvar, const float* lvlb_weights,
                      float* loss_simple, float* scalars, int B, int64_t n, int T, int loss_type, float l_simple_weight,
                      float original_elbo_weight, void* stream) {
  return guard([&] {
    need_positive("diffusion_loss", {{"batch", B}, {"table length", T}});
    if (n < 1) fail("diffusion_loss: %ld elements per sample (at least 1)", (long)n);
    if (loss_type != 0 && loss_type != 1) fail("diffusion_loss: loss_type = %d (0 = l2, 1 = l1)", loss_type);
    if (!pred || !target || !t || !logvar || !lvlb_weights || !loss_simple || !scalars) fail("diffusion_loss: null pointer argument");
    HIPCHK(launch_diffusion_loss(pred, target, (const long long*)t, logvar, lvlb_weights, loss_simple, scalars, B, (long)n, T, loss_type,
                                 l_simple_weight, original_elbo_weight, (hipStream_t)stream));
  });
}
int df_dpm_data_prediction(const float* x, const float* eps, float* out, float* s_out, int B, int64_t n, float alpha, float sigma,
                           int thresholding, float max_val, void* stream) {
  return guard([&] {
    need_positive("dpm_data_prediction", {{"batch", B}});
    if (n < 1) fail("dpm_data_prediction: %ld elements per sample (at least 1)", (long)n);
    if (thresholding && n > ((int64_t)1 << 30)) fail("dpm_data_prediction: %ld elements per sample (thresholding: at most 2^30)", (long)n);
    if (!x || !eps || !out) fail("dpm_data_prediction: null pointer argument");
    HIPCHK(launch_dpm_data_prediction(x, eps, out, s_out, B, (long)n, alpha, sigma, thresholding ? 1 : 0, max_val, (hipStream_t)stream));
  });
}
int df_dpm_adaptive_error(const float* x_hi, const float* x_lo, const float* x_prev, float* norm, float* out, int B, int64_t n,
                          float atol, float rtol, void* stream) {
  return guard([&] {
    need_positive("dpm_adaptive_error", {{"batch", B}});
    if (n < 1) fail("dpm_adaptive_error: %ld elements per sample (at least 1)", (long)n);
    if (!x_hi || !x_lo || !x_prev || !norm || !out) fail("dpm_adaptive_error: null pointer argument");
    HIPCHK(launch_dpm_adaptive_error(x_hi, x_lo, x_prev, norm, out, B, (long)n, atol, rtol, (hipStream_t)stream));
  });
}
// The geometry of df_window_gather / df_window_blend, checked on the host before anything is launched -> its device tables
static WindowTables window_geometry(const char* what, const int32_t* starts, int K, int B, int64_t rows, int Ww, int W) {
  need_positive(what, {{"batch", B}, {"windows", K}, {"window width", Ww}, {"total width", W}});
  if (rows < 1) fail("%s: %ld rows per sample (at least 1)", what, (long)rows);
  if (!starts) fail("%s: null pointer argument", what);
  const char* why = nullptr;
  if (!window_geometry_ok(starts, K, Ww, W, &why)) fail("%s: %d windows of %d columns over %d columns: %s", what, K, Ww, W, why);
  WindowTables t;
  HIPCHK(window_tables(starts, K, Ww, W, &t));
  return t;
}
int df_window_gather(const float* x, float* win, const int32_t* starts, int K, int B, int64_t rows, int Ww, int W, void* stream) {
  return guard([&] {
    const WindowTables t = window_geometry("window_gather", starts, K, B, rows, Ww, W);
    if (!x || !win) fail("window_gather: null pointer argument");
    HIPCHK(launch_window_gather(x, win, t, B, K, (long)rows, Ww, W, (hipStream_t)stream));
  });
}
int df_window_blend(const float* win, float* out, const int32_t* starts, int K, int B, int64_t rows, int Ww, int W, void* stream) {
  return guard([&] {
    const WindowTables t = window_geometry("window_blend", starts, K, B, rows, Ww, W);
    if (!win || !out) fail("window_blend: null pointer argument");
    HIPCHK(launch_window_blend(win, out, t, B, K, (long)rows, Ww, W, (hipStream_t)stream));
  });
}
int df_ddim_update(const float* x, const float* e, const float* noise, float* x_prev, float* pred_x0, int64_t n,
                   float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at, void* stream) {
  return guard([&] {
    const float dir = sqrtf(1.0f - a_prev - sigma_t * sigma_t);
    HIPCHK(launch_ddim_update(x, e, noise, x_prev, pred_x0, (long)n, sqrtf(a_t), sqrt_one_minus_at, sqrtf(a_prev), dir,
                              sigma_t, (hipStream_t)stream));
  });
}

int df_plan_count(df_ctx* c, int64_t* n_plans, int64_t* workspace_bytes) {
  return guard([&] {
    *n_plans = (int64_t)c->plans.size();
    int64_t b = 0;
    for (auto& kv : c->plans) {
      for (auto& blk : kv.second->owned) b += (int64_t)blk.bytes;
      for (auto& blk : kv.second->pinned) b += (int64_t)blk.bytes;
      b += (int64_t)kv.second->partial_bytes;
    }
    *workspace_bytes = b;
  });
}

// The autotuner's choices ("key tile splitk gm" per line) as text: rank 0 tunes, the text travels with the packed blob and
// every other rank configures its plans from it -- identical tiles / split-K (= identical fp32 summation order, bit-equal
// results across ranks) and ONE tuning pass per job instead of one per rank.
int df_tune_cache_export(char* buf, int64_t cap, int64_t* n) {
  return guard([&] {
    std::string t;
    for (auto& kv : tune_cache()) {
      char line[224];
      snprintf(line, sizeof line, "%s %d %d %d\n", kv.first.c_str(), kv.second.tile, kv.second.sk, kv.second.gm);
      t += line;
    }
    *n = (int64_t)t.size();
    if (buf && cap > 0) memcpy(buf, t.data(), std::min((size_t)cap, t.size()));
  });
}

int df_tune_cache_import(const char* text, int64_t n) {
  return guard([&] {
    std::string t(text, text + std::max<int64_t>(n, 0));
    size_t pos = 0;
    while (pos < t.size()) {
      size_t e = t.find('\n', pos);
      if (e == std::string::npos) e = t.size();
      char key[160];
      TuneChoice ch;
      if (sscanf(t.substr(pos, e - pos).c_str(), "%159s %d %d %d", key, &ch.tile, &ch.sk, &ch.gm) == 4) {
        if (ch.tile < 0 || ch.tile >= TILE_ALL || ch.sk < 1 || ch.sk > 64) fail("tune cache line out of range: %s", key);
        tune_cache()[key] = ch;
        g_tune_imported = true;
      }
      pos = e + 1;
    }
  });
}

int df_debug_checksums(df_ctx* c, int enable, int64_t capacity) {
  return guard([&] {
    HIPCHK(hipDeviceSynchronize());
    c->chk_on = enable != 0;
    c->chk_used = 0;
    c->chk_label.clear();
    if (enable) {
      const size_t cap = capacity > 0 ? (size_t)capacity : (size_t)1 << 16;
      if (cap > c->chk_cap) {
        if (c->chk_dev) (void)hipFree(c->chk_dev);
        HIPCHK(hipMalloc((void**)&c->chk_dev, cap * 8));
        c->chk_cap = cap;
      }
      HIPCHK(hipMemset(c->chk_dev, 0, c->chk_cap * 8));
    }
  });
}

int df_debug_checksums_read(df_ctx* c, uint64_t* out, int64_t cap, int64_t* n) {
  return guard([&] {
    HIPCHK(hipDeviceSynchronize());
    *n = (int64_t)c->chk_used;
    const size_t k = std::min((size_t)std::max<int64_t>(cap, 0), c->chk_used);
    if (k) HIPCHK(hipMemcpy(out, c->chk_dev, k * 8, hipMemcpyDeviceToHost));
  });
}

int df_debug_checksum_label(df_ctx* c, int64_t index, char* buf, int64_t len) {
  return guard([&] {
    if (index < 0 || (size_t)index >= c->chk_label.size() || len <= 0) fail("checksum label %lld out of range", (long long)index);
    snprintf(buf, (size_t)len, "%s", c->chk_label[(size_t)index].c_str());
  });
}

int df_debug_saturations(df_ctx* c, int enable, int64_t capacity) {
  return guard([&] {
    HIPCHK(hipDeviceSynchronize());
    c->sat_on = enable != 0;
    c->sat_used = 0;
    c->sat_label.clear();
    if (enable) {
      const size_t cap = capacity > 0 ? (size_t)capacity : (size_t)1 << 16;
      if (cap > c->sat_cap) {
        if (c->sat_dev) (void)hipFree(c->sat_dev);
        HIPCHK(hipMalloc((void**)&c->sat_dev, cap * 8));
        c->sat_cap = cap;
      }
      HIPCHK(hipMemset(c->sat_dev, 0, c->sat_cap * 8));
    }
  });
}

// Comma-separated op-tag prefixes ("*" = every op, "" = off): see df_ctx::rq_prefix.
int df_debug_requant(df_ctx* c, const char* prefixes) {
  return guard([&] {
    HIPCHK(hipDeviceSynchronize());
    c->rq_prefix.clear();
    std::string t = prefixes ? prefixes : "";
    size_t pos = 0;
    while (pos < t.size()) {
      size_t e = t.find(',', pos);
      if (e == std::string::npos) e = t.size();
      if (e > pos) c->rq_prefix.push_back(t.substr(pos, e - pos));
      pos = e + 1;
    }
  });
}

// Plan workspaces are built poisoned and re-poisoned at every release (Plan::poison, run_ops).  What Plan::alloc does at build time
// changes with the switch, so the cached plans go, as they do after a weight reload.
int df_debug_poison(df_ctx* c, int enable) {
  return guard([&] {
    const bool on = enable != 0;
    if (on && c->autotune)
      fail("df_debug_poison: df_autotune is on (the tuner re-runs ops out of plan order, which poisoned workspaces do not survive): "
           "call df_autotune(ctx, 0) first");
    if (on == c->poison_on) return;
    HIPCHK(hipDeviceSynchronize());       // the plans' buffers may still be read by queued launches
    c->plans.clear();
    c->plan_tick.clear();
    c->last_unet = nullptr;
    c->poison_on = on;
  });
}

int df_debug_saturations_read(df_ctx* c, uint64_t* out, int64_t cap, int64_t* n) {
  return guard([&] {
    HIPCHK(hipDeviceSynchronize());
    *n = (int64_t)c->sat_used;
    const size_t k = std::min((size_t)std::max<int64_t>(cap, 0), c->sat_used);
    if (k) HIPCHK(hipMemcpy(out, c->sat_dev, k * 8, hipMemcpyDeviceToHost));
  });
}

int df_debug_saturation_label(df_ctx* c, int64_t index, char* buf, int64_t len) {
  return guard([&] {
    if (index < 0 || (size_t)index >= c->sat_label.size() || len <= 0) fail("saturation label %lld out of range", (long long)index);
    snprintf(buf, (size_t)len, "%s", c->sat_label[(size_t)index].c_str());
  });
}

int df_unet_plan_stats(df_ctx* c, int64_t* n_launches, double* gemm_flops, double* weight_bytes) {
  return guard([&] {
    if (!c->last_unet) fail("no UNet plan has been executed yet");
    const size_t nctx = c->last_unet->n_ctx;
    int64_t n = 0;
    for (size_t i = nctx; i < c->last_unet->ops.size(); ++i) {
      const Plan* lp = c->last_unet;
      // the last run took either the time ops [op_t0, op_tl) or the table look-up op_tl, never both
      if (lp->op_tl >= 0 && (c->last_unet_hoisted ? ((long)i >= lp->op_t0 && (long)i < lp->op_tl) : (long)i == lp->op_tl)) continue;
      if ((long)i == lp->op_tl && lp->tl_merged) continue;      // hoisted: the look-up is part of x.pack's launch
      if ((long)i == lp->op_cfgc && lp->op_outconv >= 0 && lp->ops[lp->op_outconv].cfg_ext && lp->ops[lp->op_outconv].gp.splitk > 1) continue;
      n += 1 + (lp->ops[i].is_gemm && lp->ops[i].gp.splitk > 1 && !lp->ops[i].defer);      // (a deferred reduce runs inside the GroupNorm that follows)
    }
    *n_launches = n;
    *gemm_flops = c->last_unet->gemm_flops;
    *weight_bytes = c->last_unet->weight_bytes;
  });
}

int df_profile_begin(df_ctx* c) {
  return guard([&] {
    c->prof_on = true;
    c->prof_used = 0;
    c->prof_fam.clear();
    c->prof_op.clear();
  });
}

int df_profile_end(df_ctx* c, double* ms_by_family, int64_t* count_by_family) {
  return guard([&] {
    c->prof_on = false;
    HIPCHK(hipDeviceSynchronize());
    for (int f = 0; f < 5; ++f) {
      ms_by_family[f] = 0;
      count_by_family[f] = 0;
    }
    for (size_t i = 0; i < c->prof_fam.size(); ++i) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
      ms_by_family[c->prof_fam[i]] += ms;
      count_by_family[c->prof_fam[i]] += 1;
    }
  });
}

// Per-op CSV of the last profiled region (call between df_profile_begin and df_profile_end's sync is not needed:
// call AFTER df_profile_end).  Columns: tag,M,N,K,taps,stride,ups,batch,tile,splitk,ms,gm
int df_profile_dump(df_ctx* c, const char* path) {
  return guard([&] {
    FILE* f = fopen(path, "w");
    if (!f) fail("cannot open %s", path);
    fprintf(f, "tag,M,N,K,taps,stride,ups,batch,tile,splitk,ms,gm\n");
    for (size_t i = 0; i < c->prof_fam.size(); ++i) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
      const Op* o = (const Op*)c->prof_op[i];
      if (o->is_gemm)
        fprintf(f, "%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%.5f,%d\n", o->tag, o->gp.M, o->gp.N, o->gp.K, o->gp.taps, o->gp.stride,
                o->gp.ups, o->batch, o->tile, o->gp.splitk, ms, o->gp.gm);
      else
        fprintf(f, "%s,0,0,0,0,0,0,0,0,0,%.5f,0\n", o->tag, ms);
    }
    fclose(f);
  });
}

}  // extern "C"

// libdfengine: MI355X engine for the Diff-Foley Stage-2 sampling path (C ABI in include/df_engine.h).
//
// Host side: owns the fp32 checkpoint tensors (device copies), re-packs them to bf16 MFMA layouts, and
// compiles each network (UNet / VAE decoder / cond stage / alignment classifier) for a given batch and
// latent size into a static *plan*: a flat list of kernel launches over pre-allocated HBM buffers.
// Executing a plan is a loop of launches on the caller's stream -- no allocation, no host sync.
//
// Data layout in HBM
//   residual stream / block outputs : fp32 NHWC  [N*H*W][ld]   (skip tensors are written straight into their
//                                     slot of the decoder's concat buffer: concat costs nothing, ld = ctot)
//   MFMA operands                   : bf16 NHWC  [N*H*W][C]    (emitted by the norm kernels)
//   conv weights                    : bf16 [Cout][ky][kx][Cin] ; linear weights bf16 [out][in]
//   attention V                     : bf16 transposed [N][C][T] (produced directly by a batched GEMM)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/df_engine.h"
#include "gemm.h"
#include "kernels.h"

typedef uint16_t bf16_t;

namespace {

thread_local std::string g_err;

[[noreturn]] void fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw std::runtime_error(buf);
}
#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

struct RawT {
  float* d = nullptr;
  std::vector<int64_t> shape;
  size_t n = 0;
};

struct RunArgs {
  const float* x = nullptr;      // external latent input
  const float* t = nullptr;      // external timesteps
  const float* aux = nullptr;    // external context / features
  float* out = nullptr;          // external output
  float* out2 = nullptr;         // optional second external output (classifier probability in the grad plan)
  float scale = 1.f;             // guidance scale
  int ts_index = -1;             // >= 0: row of the plan's hoisted time-embedding table (df_unet_set_timesteps)
};

struct OutBuf { const uint16_t* p; long rows; int cols, ld; };   // operand-type output of a non-GEMM op (df_debug_saturations)

struct Op {
  bool is_gemm = false;
  std::vector<OutBuf> outs;
  GemmParams gp{};
  int tile = 0, batch = 1;
  bool c_ext = false;            // gp.C <- RunArgs.out at run time
  bool cfg_ext = false;          // split-K only: the reduce launch also does the CFG combine into RunArgs.out (GemmParams::cfg_out)
  bool defer = false;            // when tuned to split-K: leave the partial slabs to the next op (a GroupNorm that sums them)
  std::function<hipError_t(hipStream_t, const RunArgs&)> fn;
  const char* tag = "";
};

struct Block {
  void* p;
  size_t bytes;
};

struct Plan {
  std::vector<Op> ops;
  std::vector<Block> owned;      // every hipMalloc'd block (freed with the plan)
  std::vector<Block> freelist;   // build-time reuse
  float* partial = nullptr;      // shared split-K scratch
  size_t partial_bytes = 0;
  double gemm_flops = 0, weight_bytes = 0;
  size_t ext_hint = 0;           // largest external (caller-owned) buffer the plan touches, when above 32 MB (autotune dummies)
  size_t n_ctx = 0;              // UNet plans: ops [0, n_ctx) depend on the context only (run by df_unet_set_context)
  // Classifier-gradient plans: ops [0, n_feat) turn the video features into the cross-attention K / V^T of every transformer
  // block; feat_token != 0 names the features those buffers were last computed from (df_classifier_grad_cached)
  size_t n_feat = 0;
  uint64_t feat_token = 0;
  // Hoisted time embedding: ops [op_t0, op_tl) map the timestep to the stacked emb projections E [N][etot] (they depend on t
  // only); op_tl = "t.lookup" copies row ts_index of Etab [S][etot] to every row of E instead.  df_unet_set_timesteps fills the
  // table by running [op_t0, op_tl) once per timestep of a sample() call; the step loop then runs [op_tl, end).
  long op_t0 = -1, op_tl = -1;
  float* E = nullptr;
  int etot = 0, e_rows = 0, t_rows = 0;
  float* Etab = nullptr;         // [etab_S][etot]
  float* ttab = nullptr;         // [etab_S][t_rows] timesteps as the time ops read them
  int etab_S = 0, etab_cap = 0;
  std::vector<float> etab_t;     // the etab_S timesteps the table was built for (host copy: an identical announcement is a no-op)
  // launch accounting (df_unet_plan_stats): t.lookup launches nothing when its row broadcast rides in x.pack (tl_merged), and
  // cfg.combine (op_cfgc) launches nothing while out.conv (op_outconv) runs split-K with the guided reduce
  bool tl_merged = false;
  long op_cfgc = -1, op_outconv = -1;
  std::string name;              // cache key (debug labels)
  void* chk_list = nullptr;      // debug checksums: device array of (pointer, 32-bit words) of every workspace block
  int chk_n = 0;
  ~Plan() {
    for (auto& b : owned) (void)hipFree(b.p);
    if (partial) (void)hipFree(partial);
    if (chk_list) (void)hipFree(chk_list);
    if (Etab) (void)hipFree(Etab);
    if (ttab) (void)hipFree(ttab);
  }
  void* alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    int best = -1;
    for (int i = 0; i < (int)freelist.size(); ++i)
      if (freelist[i].bytes >= bytes && freelist[i].bytes <= bytes + bytes / 2 + 4096 &&
          (best < 0 || freelist[i].bytes < freelist[best].bytes))
        best = i;
    if (best >= 0) {
      void* p = freelist[best].p;
      freelist.erase(freelist.begin() + best);
      return p;
    }
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    HIPCHK(hipMemset(p, 0, bytes));
    owned.push_back({p, bytes});
    return p;
  }
  // One buffer may be HELD: a release() of it is postponed until unhold() (Builder: the fp32 residual of a GEMM whose split-K
  // reduce is handed to the next op must not be recycled for that op's own outputs).
  const void* held = nullptr;
  bool held_released = false;
  void unhold() {
    const void* h = held;
    const bool rel = held_released;
    held = nullptr;
    held_released = false;
    if (h && rel) release(const_cast<void*>(h));
  }
  void release(void* p) {
    if (!p) return;
    if (p == held) {
      held_released = true;
      return;
    }
    for (auto& b : owned)
      if (b.p == p) {
        freelist.push_back(b);
        return;
      }
  }
};

struct F32 {  // fp32 NHWC activation view
  float* p = nullptr;
  int rows = 0, C = 0, ld = 0;
  uint16_t* b16 = nullptr;      // operand-type copy [rows][C] written by the op that produced the tensor (classifier-gradient tape), or null
};

}  // namespace

struct df_ctx {
  int device = 0;
  std::map<std::string, RawT> raw;
  std::map<std::string, void*> packed;
  std::vector<void*> packed_blocks;
  bool has_unet = false, has_vae = false, has_cond = false, has_cls = false, has_cavp = false, finalized = false;
  df_cavp_config pcfg{};
  df_unet_config ucfg{}, ccfg{};
  df_vae_config vcfg{};
  df_cond_config kcfg{};
  std::map<std::string, int> emb_off[2];   // resblock prefix -> column offset in the fused emb projection
  int emb_total[2] = {0, 0};
  std::map<std::string, std::unique_ptr<Plan>> plans;
  std::map<std::string, uint64_t> plan_tick;     // last use of every plan (least-recently-used eviction, DF_MAX_PLANS)
  uint64_t tick = 0;
  Plan* last_unet = nullptr;
  bool last_unet_hoisted = false;   // the last UNet run looked its time embedding up (df_unet_forward*_ts)
  int ctx_N = 0, ctx_T = 0;
  float* ctx_copy = nullptr;
  size_t ctx_copy_bytes = 0;
  bool autotune = false;
  bool reloaded = false;          // a tensor that already existed was loaded again: packed operand copies are stale
  bool prof_on = false;
  std::vector<hipEvent_t> prof_ev;      // pairs (start, stop) per executed op while profiling
  std::vector<int> prof_fam;
  std::vector<const void*> prof_op;
  size_t prof_used = 0;
  hipStream_t pack_stream = nullptr;
  // debug: after every op, a 64-bit checksum of ALL workspace bytes of the plan (df_debug_checksums): two runs of the same
  // inputs must give the same sequence; the first index that differs names the op whose launch was not reproducible
  bool chk_on = false;
  // debug (df_debug_requant, fp16 build): operand-type outputs of the ops whose tag starts with one of these prefixes are re-rounded
  // to bf16 precision (8 significant bits) right behind the op -- the error budget of the bf16 build, one op family at a time
  std::vector<std::string> rq_prefix;
  unsigned long long* chk_dev = nullptr;
  size_t chk_used = 0, chk_cap = 0;
  std::vector<std::string> chk_label;
  // debug: after every op, the number of operand-type values it stored that sit at the fp16 saturation value +-65504 (fp16
  // build: conversions clamp there instead of overflowing) / are not finite (bf16 build) -- df_debug_saturations
  bool sat_on = false;
  unsigned long long* sat_dev = nullptr;
  size_t sat_used = 0, sat_cap = 0;
  std::vector<std::string> sat_label;

  ~df_ctx() {
    plans.clear();
    for (auto& kv : raw) (void)hipFree(kv.second.d);
    for (void* p : packed_blocks) (void)hipFree(p);
    for (hipEvent_t e : prof_ev) (void)hipEventDestroy(e);
    if (chk_dev) (void)hipFree(chk_dev);
    if (sat_dev) (void)hipFree(sat_dev);
    if (ctx_copy) (void)hipFree(ctx_copy);
  }

  const RawT& rt(const std::string& name) const {
    auto it = raw.find(name);
    if (it == raw.end()) fail("missing tensor '%s'", name.c_str());
    return it->second;
  }
  bool has(const std::string& name) const { return raw.count(name) != 0; }
  const float* f32(const std::string& name) const {
    const RawT& t = rt(name);
    if (!t.d) fail("tensor '%s' was imported shape-only (df_import_packed): its fp32 data is not on this rank", name.c_str());
    return t.d;
  }

  std::map<const void*, size_t> block_bytes;     // size of every packed block (export of the packed blob)
  void* pmalloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, (bytes + 255) & ~(size_t)255));
    packed_blocks.push_back(p);
    block_bytes[p] = bytes;
    return p;
  }
  // Linear / 1x1-conv weight [O][I] -> bf16
  const bf16_t* w_linear(const std::string& name) {
    auto it = packed.find(name);
    if (it != packed.end()) return (const bf16_t*)it->second;
    const RawT& t = rt(name);
    (void)f32(name);
    bf16_t* o = (bf16_t*)pmalloc(t.n * 2);
    HIPCHK(launch_cast_bf16(t.d, o, (long)t.n, pack_stream));
    packed[name] = o;
    return o;
  }
  // rows of several [O_i][I] matrices stacked -> bf16 [sum O_i][I]
  const bf16_t* w_stack(const std::string& key, const std::vector<std::string>& names) {
    auto it = packed.find(key);
    if (it != packed.end()) return (const bf16_t*)it->second;
    size_t tot = 0;
    for (auto& n : names) tot += rt(n).n;
    bf16_t* o = (bf16_t*)pmalloc(tot * 2);
    size_t off = 0;
    for (auto& n : names) {
      const RawT& t = rt(n);
      HIPCHK(launch_cast_bf16(t.d, o + off, (long)t.n, pack_stream));
      off += t.n;
    }
    packed[key] = o;
    return o;
  }
  const float* b_stack(const std::string& key, const std::vector<std::string>& names) {
    auto it = packed.find(key);
    if (it != packed.end()) return (const float*)it->second;
    size_t tot = 0;
    for (auto& n : names) tot += rt(n).n;
    float* o = (float*)pmalloc(tot * 4);
    size_t off = 0;
    for (auto& n : names) {
      const RawT& t = rt(n);
      HIPCHK(hipMemcpyAsync(o + off, t.d, t.n * 4, hipMemcpyDeviceToDevice, pack_stream));
      off += t.n;
    }
    packed[key] = o;
    return o;
  }
  // 3x3 conv weight OIHW -> bf16 [O][3][3][Ipad]
  const bf16_t* w_conv3(const std::string& name, int ipad) {
    const std::string key = name + "#c3";
    auto it = packed.find(key);
    if (it != packed.end()) return (const bf16_t*)it->second;
    const RawT& t = rt(name);
    if (t.shape.size() != 4 || t.shape[2] != 3 || t.shape[3] != 3) fail("'%s' is not a 3x3 conv weight", name.c_str());
    const int O = (int)t.shape[0], I = (int)t.shape[1];
    bf16_t* o = (bf16_t*)pmalloc((size_t)O * 9 * ipad * 2);
    HIPCHK(launch_pack_conv_weight(t.d, o, O, I, 3, 3, ipad, pack_stream));
    packed[key] = o;
    return o;
  }
  // 3x3 conv weight that follows a nearest-x2 Upsample: per-phase 2x2-tap weights [4][O][4][Ipad] (gemm_m3.hip)
  const bf16_t* w_conv3_ups4(const std::string& name, int ipad) {
    const std::string key = name + "#c3ups4";
    auto it = packed.find(key);
    if (it != packed.end()) return (const bf16_t*)it->second;
    const RawT& t = rt(name);
    if (t.shape.size() != 4 || t.shape[2] != 3 || t.shape[3] != 3) fail("'%s' is not a 3x3 conv weight", name.c_str());
    const int O = (int)t.shape[0], I = (int)t.shape[1];
    bf16_t* o = (bf16_t*)pmalloc((size_t)16 * O * ipad * 2);
    HIPCHK(launch_pack_conv_ups4(f32(name), o, O, I, ipad, pack_stream));
    packed[key] = o;
    return o;
  }
  // conv2 + folded 1x1 skip connection: operand [O][9*I + I2] and the summed bias
  void w_conv3_skip(const std::string& conv, const std::string& skip, const bf16_t** w, const float** b) {
    const std::string kw = conv + ".weight#c3skip", kb = conv + ".bias#c3skip";
    if (!packed.count(kw)) {
      const RawT& t = rt(conv + ".weight");
      const RawT& ts = rt(skip + ".weight");
      const int O = (int)t.shape[0], I = (int)t.shape[1], I2 = (int)ts.shape[1];
      bf16_t* wo = (bf16_t*)pmalloc((size_t)O * (9 * I + I2) * 2);
      float* bo = (float*)pmalloc((size_t)O * 4);
      HIPCHK(launch_pack_conv_skip(f32(conv + ".weight"), f32(skip + ".weight"), wo, O, I, I2, pack_stream));
      const float* ins[2] = {f32(conv + ".bias"), f32(skip + ".bias")};
      const float co[2] = {1.f, 1.f};
      HIPCHK(launch_lincomb(bo, ins, co, 2, O, pack_stream));
      packed[kw] = wo;
      packed[kb] = bo;
    }
    *w = (const bf16_t*)packed[kw];
    *b = (const float*)packed[kb];
  }
  // FeedForward's second Linear merged with the SpatialTransformer's proj_out (1x1 conv): operand [C][4C + C], summed bias
  void w_ffproj(const std::string& ff2, const std::string& po, const bf16_t** w, const float** b) {
    const std::string kw = ff2 + ".weight#ffproj", kb = ff2 + ".bias#ffproj";
    if (!packed.count(kw)) {
      const RawT& t2 = rt(ff2 + ".weight");
      const RawT& tp = rt(po + ".weight");
      const int C = (int)t2.shape[0], F = (int)t2.shape[1];
      if ((int)tp.shape[0] != C || (int)tp.shape[1] != C) fail("ffproj: proj_out is not %dx%d", C, C);
      bf16_t* wo = (bf16_t*)pmalloc((size_t)C * (F + C) * 2);
      float* bo = (float*)pmalloc((size_t)C * 4);
      HIPCHK(launch_pack_ffproj(f32(po + ".weight"), f32(po + ".bias"), f32(ff2 + ".weight"), f32(ff2 + ".bias"), wo, bo, C, F,
                                pack_stream));
      packed[kw] = wo;
      packed[kb] = bo;
    }
    *w = (const bf16_t*)packed[kw];
    *b = (const float*)packed[kb];
  }
  // scale * gamma[c] * Wq[j][c] as operand [c][j]: the LayerNorm-folded cross-attention query projection, transposed
  const bf16_t* w_lnq_t(const std::string& wq, const std::string& norm, float scale) {
    const std::string key = wq + "#lnqT";
    auto it = packed.find(key);
    if (it != packed.end()) return (const bf16_t*)it->second;
    const RawT& t = rt(wq);
    const int C = (int)t.shape[0];
    if ((int)t.shape[1] != C) fail("w_lnq_t %s: not square", wq.c_str());
    bf16_t* o = (bf16_t*)pmalloc((size_t)C * C * 2);
    HIPCHK(launch_pack_lnq_t(t.d, f32(norm + ".weight"), o, C, scale, pack_stream));
    packed[key] = o;
    return o;
  }
  // Linear weights [O_j][I] stacked along O and transposed -> bf16 [I][sum O_j]  (backward-data operand)
  const bf16_t* w_stack_t(const std::string& key, const std::vector<std::string>& names) {
    auto it = packed.find(key);
    if (it != packed.end()) return (const bf16_t*)it->second;
    int otot = 0;
    const int I = (int)rt(names[0]).shape[1];
    for (auto& n : names) otot += (int)rt(n).shape[0];
    bf16_t* o = (bf16_t*)pmalloc((size_t)I * otot * 2);
    int off = 0;
    for (auto& n : names) {
      const RawT& t = rt(n);
      HIPCHK(launch_pack_linear_t(t.d, o, (int)t.shape[0], I, otot, off, pack_stream));
      off += (int)t.shape[0];
    }
    packed[key] = o;
    return o;
  }
  // 3x3 conv weight OIHW -> backward-data packing bf16 [I][ky'][kx'][Opad] (flipped taps).  Opad = Cout rounded up to the 64-channel
  // K step with zero rows behind the real ones: the gradient operand of such a conv carries Opad columns, the pad ones zero (the
  // classifier head's conv halves the channels: 64 -> 32, 320 -> 160; every other conv on the tape has Cout % 64 == 0)
  const bf16_t* w_conv3_bwd(const std::string& name) {
    const std::string key = name + "#c3bwd";
    auto it = packed.find(key);
    if (it != packed.end()) return (const bf16_t*)it->second;
    const RawT& t = rt(name);
    const int O = (int)t.shape[0], I = (int)t.shape[1], Opad = (O + 63) / 64 * 64;
    bf16_t* o = (bf16_t*)pmalloc((size_t)I * 9 * Opad * 2);
    HIPCHK(launch_pack_conv_bwd(t.d, o, O, I, Opad, pack_stream));
    packed[key] = o;
    return o;
  }
  // Conv3d + eval BatchNorm3d of an mmcv ConvModule `p` (keys p.conv.weight, p.bn.*): operand [O][kp] with the BN scale
  // folded in (k = tap*I + i, zero padded to kp) and the fp32 bias beta - mean*scale.
  void w_conv3d_bn(const std::string& p, int kp, const bf16_t** w, const float** b) {
    const std::string kw = "c3d:" + p + ":" + std::to_string(kp), kb = kw + ":b";
    if (!packed.count(kw)) {
      const RawT& t = rt(p + ".conv.weight");
      if (t.shape.size() != 5) fail("%s.conv.weight: expected a 5-D Conv3d weight", p.c_str());
      const int O = (int)t.shape[0], I = (int)t.shape[1], KT = (int)t.shape[2], KH = (int)t.shape[3], KW = (int)t.shape[4];
      bf16_t* wo = (bf16_t*)pmalloc((size_t)O * kp * 2);
      float* bo = (float*)pmalloc((size_t)O * 4);
      HIPCHK(launch_pack_conv3d_bn(t.d, f32(p + ".bn.weight"), f32(p + ".bn.bias"), f32(p + ".bn.running_mean"),
                                   f32(p + ".bn.running_var"), 1e-5f, wo, bo, O, I, KT, KH, KW, kp, pack_stream));
      packed[kw] = wo;
      packed[kb] = bo;
    }
    *w = (const bf16_t*)packed[kw];
    *b = (const float*)packed[kb];
  }

  // LayerNorm `norm` folded into the Linear(s) `names` stacked along the output dim (biases[i] may be empty):
  // operand rows gamma*W, their column sums and the folded bias beta.W + b.  geglu: ONE matrix, rows GEGLU-interleaved.
  void w_ln_stack(const std::string& key, const std::string& norm, const std::vector<std::string>& names,
                  const std::vector<std::string>& biases, bool geglu, const bf16_t** w, const float** cs, const float** bb) {
    const std::string kw = key + "#lnw", kc = key + "#lncs", kb = key + "#lnbb";
    if (!packed.count(kw)) {
      int rows = 0;
      const int K = (int)rt(names[0]).shape[1];
      for (auto& n : names) rows += (int)rt(n).shape[0];
      bf16_t* wo = (bf16_t*)pmalloc((size_t)rows * K * 2);
      float* co = (float*)pmalloc((size_t)rows * 4);
      float* bo = (float*)pmalloc((size_t)rows * 4);
      const float* g = f32(norm + ".weight");
      const float* be = f32(norm + ".bias");
      int off = 0;
      for (size_t i = 0; i < names.size(); ++i) {
        const RawT& t = rt(names[i]);
        if ((int)t.shape[1] != K) fail("w_ln_stack %s: input dims differ", key.c_str());
        const float* bias = (i < biases.size() && !biases[i].empty()) ? f32(biases[i]) : nullptr;
        const int r = (int)t.shape[0];
        HIPCHK(launch_pack_ln_linear(t.d, bias, g, be, wo, co, bo, r, K, off, geglu ? r / 2 : 0, pack_stream));
        off += r;
      }
      packed[kw] = wo;
      packed[kc] = co;
      packed[kb] = bo;
    }
    *w = (const bf16_t*)packed[kw];
    *cs = (const float*)packed[kc];
    *bb = (const float*)packed[kb];
  }

  // The LayerNorm-folded GEGLU projection `key` (w_ln_stack with geglu = true: rows in (32 x | 32 gate) groups) once more in the
  // 320-column packing of the wide tiles (ffn_wide.hip): a device-side row permutation of the packed operand -- needs no fp32
  // data, so a rank that imported the packed blob builds it the same way.
  void w_ln_w320(const std::string& key, int rows, int K, const bf16_t** w, const float** cs, const float** bb) {
    const std::string kw = key + "#lnw", kc = key + "#lncs", kb = key + "#lnbb";
    const std::string kw3 = key + "#lnw320", kc3 = key + "#lncs320", kb3 = key + "#lnbb320";
    if (!packed.count(kw3)) {
      if (!packed.count(kw) || !packed.count(kc) || !packed.count(kb)) fail("w_ln_w320 %s: the (32 | 32) packing does not exist", key.c_str());
      bf16_t* wo = (bf16_t*)pmalloc((size_t)rows * K * 2);
      float* co = (float*)pmalloc((size_t)rows * 4);
      float* bo = (float*)pmalloc((size_t)rows * 4);
      HIPCHK(launch_pack_w320((const bf16_t*)packed[kw], (const float*)packed[kc], (const float*)packed[kb], wo, co, bo, rows, K, pack_stream));
      packed[kw3] = wo;
      packed[kc3] = co;
      packed[kb3] = bo;
    }
    *w = (const bf16_t*)packed[kw3];
    *cs = (const float*)packed[kc3];
    *bb = (const float*)packed[kb3];
  }

  void w_geglu(const std::string& prefix, const bf16_t** w, const float** b) {
    const std::string kw = prefix + ".weight#geglu", kb = prefix + ".bias#geglu";
    auto it = packed.find(kw);
    if (it == packed.end()) {
      const RawT& tw = rt(prefix + ".weight");
      const RawT& tb = rt(prefix + ".bias");
      const int rows = (int)tw.shape[0], K = (int)tw.shape[1];
      bf16_t* wo = (bf16_t*)pmalloc((size_t)rows * K * 2);
      float* bo = (float*)pmalloc((size_t)rows * 4);
      HIPCHK(launch_pack_geglu(tw.d, tb.d, wo, bo, rows / 2, K, pack_stream));
      packed[kw] = wo;
      packed[kb] = bo;
    }
    *w = (const bf16_t*)packed[kw];
    *b = (const float*)packed[kb];
  }
};

namespace {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int rup(int a, int b) { return cdiv(a, b) * b; }

// ---------------------------------------------------------------------------------------------------------------
// Tile / split-K choice: a small cost model in MFMA cycles (256 CUs, one 32x32x16 MFMA per 8 cycles per CU).
void choose_tile(int M, int N, int K, int batch, bool geglu, int* tile, int* splitk) {
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

struct Builder {
  df_ctx* c;
  Plan* pl;
  std::string pre;     // state_dict prefix of the module being built
  int which = 0;       // 0 = unet, 1 = classifier (emb offset table)

  std::string nm(const std::string& s) const { return pre + s; }

  struct PX;     // cross-attention operands precomputed from the context (context_px below)

  // A consumer that needs the operand-type copy of a block's fp32 output (Downsample / Upsample convs) sets
  // want_aux before the block is built; the block's last GEMM then writes the copy from its epilogue (no cast pass)
  // and leaves the buffer in last_aux.
  bool want_aux = false;
  bf16_t* last_aux = nullptr;
  void attach_aux(GemmParams& g, int rows, int C) {
    last_aux = nullptr;
    if (!want_aux) return;
    last_aux = buf<bf16_t>((size_t)rows * C);
    g.aux = last_aux;
    g.ld_aux = C;
    want_aux = false;
  }

  template <class T>
  T* buf(size_t n) {
    return (T*)pl->alloc(n * sizeof(T));
  }

  // The last emitted op, when it is a GEMM whose fp32 output could be left as split-K slabs for a GroupNorm that follows
  // IMMEDIATELY (groupnorm() below claims it; any other emission forgets it).
  struct Pend { long op = -1; const float* p = nullptr; int ld = 0, C = 0, rows = 0; };
  Pend pend;

  void forget_pend() {
    pend = Pend{};
    pl->unhold();
  }

  void other(const char* tag, std::function<hipError_t(hipStream_t, const RunArgs&)> fn) {
    forget_pend();
    Op o;
    o.fn = std::move(fn);
    o.tag = tag;
    pl->ops.push_back(std::move(o));
  }
  // operand-type output of the op emitted last (counted by df_debug_saturations)
  void emits(const bf16_t* p, long rows, int cols, int ld) {
    if (p && !pl->ops.empty()) pl->ops.back().outs.push_back({p, rows, cols, ld});
  }

  Op& gemm(GemmParams gp, int batch, const char* tag) {
    Op o;
    o.is_gemm = true;
    o.batch = batch;
    o.tag = tag;
    int sk = 1;
    // the K loop of every GEMM kernel walks whole 64-element steps (gemm_impl.h: nk = K / 64): a ragged K would silently drop its tail
    if (gp.K % 64 != 0 || (gp.taps != 1 && gp.Cin % 64 != 0))
      fail("GEMM %s (%dx%dx%d, Cin %d): the contraction length must be a multiple of 64 (channel counts, context_dim and origin_dim "
           "that are not are outside what libdfengine builds)", tag, gp.M, gp.N, gp.K, gp.Cin);
    choose_tile(gp.M, gp.N, gp.K, batch, gp.geglu != 0, &o.tile, &sk);
    if (gp.taps == 9 && gemm_tile_valid(gp, TILE_HALO_128x64, batch, 1)) {   // halo reuse beats re-fetching A per tap
      o.tile = TILE_HALO_128x64;
      const long blocks = (long)((gp.M + 127) / 128) * ((gp.N + 63) / 64);
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

  // operands are addressed through 32-bit buffer offsets: one operand of one GEMM must stay below 2 GiB
  static unsigned op_bytes(size_t b) {
    if (b >= ((size_t)1 << 31)) fail("GEMM operand of %zu bytes exceeds the 2 GiB buffer-addressing limit (split the batch)", b);
    return (unsigned)b;
  }
  static GemmParams gp_linear(const bf16_t* A, int M, int K, const bf16_t* W, int N) {
    GemmParams g{};
    g.A = A; g.lda = K; g.W = W; g.M = M; g.N = N; g.K = K;
    g.taps = 1; g.Cin = K; g.alpha = 1.f; g.stride = 1;
    g.a_bytes = op_bytes((size_t)M * K * 2); g.w_bytes = op_bytes((size_t)N * K * 2);
    return g;
  }
  static GemmParams gp_conv3(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W, int Cout, int stride,
                             int ups) {
    GemmParams g{};
    g.A = A; g.lda = Cin; g.W = W;
    g.H = H; g.Wd = Wd; g.stride = stride; g.ups = ups;
    g.OH = ups ? 2 * H : (stride == 2 ? H / 2 : H);
    g.OW = ups ? 2 * Wd : (stride == 2 ? Wd / 2 : Wd);
    g.M = NB * g.OH * g.OW; g.N = Cout; g.K = 9 * Cin;
    g.taps = 9; g.Cin = Cin; g.alpha = 1.f;
    g.a_bytes = op_bytes((size_t)NB * H * Wd * Cin * 2); g.w_bytes = op_bytes((size_t)Cout * 9 * Cin * 2);
    return g;
  }
  // nearest-x2 upsample + conv3x3 as four 2x2-tap convs (one per output phase) over the INPUT-resolution map: rows = input
  // pixels, K = 4 Cin, one weight matrix per phase (w_bs), output rows = the x2 map (the kernel scatters by phase)
  static GemmParams gp_conv3_ups4(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W4, int Cout) {
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
  static void out_f32(GemmParams& g, float* C, int ldc) { g.C = C; g.ldc = ldc; g.out_bf16 = 0; }
  static void out_b16(GemmParams& g, bf16_t* C, int ldc) { g.C = C; g.ldc = ldc; g.out_bf16 = 1; }

  // GroupNorm(+SiLU) -> bf16 operand (and optionally the raw bf16 cast)
  bf16_t* groupnorm(const F32& x, int NB, const std::string& p, float eps, int silu, bf16_t** raw) {
    bf16_t* o = buf<bf16_t>((size_t)x.rows * x.C);
    bf16_t* r = raw ? buf<bf16_t>((size_t)x.rows * x.C) : nullptr;
    if (raw) *raw = r;
    const float* g = c->f32(nm(p + ".weight"));
    const float* b = c->f32(nm(p + ".bias"));
    const float* xp = x.p;
    const int ld = x.ld, HW = x.rows / NB, C = x.C;
    const size_t sb = groupnorm_scratch_bytes(NB, HW, C);
    // x straight out of a GEMM that may run split-K (a ResBlock's conv2, a SpatialTransformer's merged FF2 + proj_out, a
    // Downsample conv): this norm is its first reader, so it does the reduce -- sums the slabs, adds bias + residual, writes
    // x back -- in the launch it needs anyway; the producer's reduce launch and one fp32 round trip of x disappear.
    static const bool no_own = getenv("DF_NO_GNOWN") && atoi(getenv("DF_NO_GNOWN"));
    Pend pd = pend;
    if (!no_own && !sb && pd.op >= 0 && pd.p == xp && pd.ld == ld && pd.rows == x.rows && pd.C <= C && (pd.C & 1) == 0 &&
        (ld & 1) == 0 && groupnorm_accepts_slabs(HW, C)) {
      Plan* plp = pl;
      const size_t pi = (size_t)pd.op;
      pl->ops[pi].defer = true;
      float* xw = x.p;
      other("groupnorm", [=](hipStream_t s, const RunArgs&) {
        const Op& po = plp->ops[pi];
        if (po.defer && po.gp.splitk > 1)
          return launch_groupnorm_own_slabs(xw, ld, NB, HW, C, g, b, eps, silu, o, C, r, po.gp.partial, po.gp.splitk,
                                            (long)po.gp.M * po.gp.N, po.gp.N, po.gp.bias, po.gp.res, po.gp.ldr, s);
        return launch_groupnorm(xp, ld, NB, HW, C, g, b, eps, silu, o, C, r, s);
      });
      emits(o, x.rows, C, C);
      emits(r, x.rows, C, C);
      return o;
    }
    if (sb) {          // large slabs (VAE decoder): pixel-chunked, fully coalesced three-launch form
      float* scr = (float*)pl->alloc(sb);
      other("groupnorm", [=](hipStream_t s, const RunArgs&) {
        return launch_groupnorm_chunked(xp, ld, NB, HW, C, g, b, eps, silu, o, C, r, scr, s);
      });
      emits(o, x.rows, C, C);
      emits(r, x.rows, C, C);
      pl->release(scr);
      return o;
    }
    other("groupnorm", [=](hipStream_t s, const RunArgs&) {
      return launch_groupnorm(xp, ld, NB, HW, C, g, b, eps, silu, o, C, r, s);
    });
    emits(o, x.rows, C, C);
    emits(r, x.rows, C, C);
    return o;
  }
  void layernorm(const F32& x, const std::string& p, bf16_t* o) {
    const float* g = c->f32(nm(p + ".weight"));
    const float* b = c->f32(nm(p + ".bias"));
    const float* xp = x.p;
    const int ld = x.ld, rows = x.rows, C = x.C;
    other("layernorm", [=](hipStream_t s, const RunArgs&) { return launch_layernorm(xp, ld, rows, C, g, b, 1e-5f, o, s); });
    emits(o, rows, C, C);
  }
  bf16_t* cast2d(const F32& x) {
    if (x.b16) return x.b16;      // the producer already wrote the operand copy: no cast launch
    bf16_t* o = buf<bf16_t>((size_t)x.rows * x.C);
    const float* xp = x.p;
    const int ld = x.ld, C = x.C;
    const long rows = x.rows;
    other("cast", [=](hipStream_t s, const RunArgs&) { return launch_cast_bf16_2d(xp, ld, o, rows, C, s); });
    emits(o, rows, C, C);
    return o;
  }

  // ResBlock (openai_unetmodel.py:255-275) / VAE ResnetBlock (model.py:216-236, no emb).  `out` may be a slot of a
  // concat buffer.  Names differ between the two families, so they are passed in.
  void resblock(const F32& x, const F32& out, int NB, int H, int Wd, const std::string& n1, const std::string& c1,
                const std::string& n2, const std::string& c2, const std::string& skip, float eps,
                const float* emb, int emb_ld, int emb_col, int dup_rows = 0) {
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
    pl->ops[ci].defer = groupnorm_accepts_slabs(H * Wd, cout);
    bf16_t* a2 = buf<bf16_t>((size_t)M * cout);
    {
      Plan* plp = pl;
      const float* gm = c->f32(nm(n2 + ".weight"));
      const float* bt = c->f32(nm(n2 + ".bias"));
      const float* cb = c->f32(nm(c1 + ".bias"));
      const float* rb = emb ? emb + emb_col : nullptr;
      const int HW = H * Wd;
      const size_t sb = groupnorm_scratch_bytes(NB, HW, cout);
      float* scr = sb ? (float*)pl->alloc(sb) : nullptr;
      other("groupnorm", [=](hipStream_t s, const RunArgs&) {
        const Op& co = plp->ops[ci];
        if (co.defer && co.gp.splitk > 1)
          return launch_groupnorm_slabs(co.gp.partial, cout, NB, HW, cout, gm, bt, eps, 1, a2, cout, nullptr, co.gp.splitk,
                                        (long)M * cout, cb, rb, emb_ld, s);
        if (scr) return launch_groupnorm_chunked(h1, cout, NB, HW, cout, gm, bt, eps, 1, a2, cout, nullptr, scr, s);
        return launch_groupnorm(h1, cout, NB, HW, cout, gm, bt, eps, 1, a2, cout, nullptr, s);
      });
      emits(a2, M, cout, cout);
      pl->release(scr);
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
        g.A2 = xraw; g.lda2 = cin; g.Cin2 = cin; g.a2_bytes = op_bytes((size_t)M * cin * 2);
        g.K = 9 * cout + cin;
        g.w_bytes = op_bytes((size_t)cout * g.K * 2);
      } else { g.res = x.p; g.ldr = x.ld; }
      attach_aux(g, M, cout);
      g.dup_rows = dup_rows;       // CFG prefix: this block ran on one half of the batch, its output feeds both
      gemm(g, 1, "res.conv2");
    }
    if (has_skip) pl->release(xraw);
    pl->release(a2);
  }

  // SpatialTransformer (attention_openai.py:250-261) with one BasicTransformerBlock (:211-215).
  // ctxK [NB*Tc][C] bf16 and ctxVt [NB][C][ldvt] bf16 are the hoisted cross-attention K / V^T.
  // cfg_prefix: the block is the first SpatialTransformer of a classifier-free-guidance batch [x ; x] -- its GroupNorm, proj_in,
  // Q|K|V projection, self-attention and out-projection see identical rows in both halves (no context yet), so they run on the
  // first half only and attn1.out stores every row for both halves (GemmParams::dup_rows); from the cross-attention on, full batch.
  void spatial_transformer(const F32& x, const F32& out, int NB, int T, const std::string& p, int heads,
                           const bf16_t* ctxK, const bf16_t* ctxVt, int Tc, int ldvtc, const PX* px = nullptr,
                           bool cfg_prefix = false) {
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
      g.K = 5 * C;
      g.w_bytes = op_bytes((size_t)C * 5 * C * 2);
      g.A2 = xb; g.lda2 = C; g.Cin2 = C; g.a2_bytes = op_bytes((size_t)M * C * 2);
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

  // context -> per-ST K [NB*Tc][C] and V^T [NB][C][ldvt]
  // Cross-attention with the context folded into per-sample "weights".  The context is fixed for a whole sample() call while
  // the queries change every step, so everything that does not depend on the query is precomputed by set_context:
  //   scores_h = LN(t) Wq_h^T K_h^T / sqrt(D) = LN(t) . G_h,   G = [G_0 .. G_H-1]  ([C] x [H*32] per sample, LayerNorm-folded)
  //   out      = sum_h P_h V_h Wo_h^T + bo   = P . Vo,          Vo = [Wo_h V_h^T]_h ([H*32] x [C] per sample)
  // which turns  q-projection -> attention kernel -> out-projection  (2 M C^2 + 2 M C^2 FLOPs, 3 launches) into two GEMMs
  // of 2 M C (32 H) FLOPs each with a softmax in the first one's epilogue (context length <= 32: padded to 32 per head).
  struct PX {
    const bf16_t* G = nullptr;    // [NB][H*32][C]   operand of the score GEMM (rows = (head, context token))
    const float* cs = nullptr;    // [NB][H*32]      column sums of G (LayerNorm fold)
    const float* bb = nullptr;    // [NB][H*32]      beta . G
    const bf16_t* Vo = nullptr;   // [NB][C][H*32]   operand of the output GEMM
    int HT = 0;                   // H * 32
  };
  static bool px_ok(int C, int heads, int Tc, int tokens) {
    const bool off = getenv("DF_NO_XPRE") && atoi(getenv("DF_NO_XPRE"));     // read per plan build: tests A/B both forms
    return !off && Tc >= 1 && Tc <= 32 && C % 64 == 0 && C % heads == 0 && (C / heads) % 8 == 0 && (heads * 32) % 64 == 0 &&
           tokens % 64 == 0;
  }
  PX context_px(const bf16_t* ctx, int NB, int Tc, int Dc, const std::string& st_prefix, int C, int heads) {
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

  void context_kv(const bf16_t* ctx, int NB, int Tc, int Dc, const std::string& st_prefix, int C, bf16_t** K,
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
};

// ---------------------------------------------------------------------------------------------------------------
// UNet topology (openai_unetmodel.py:516-692), shared by the plan builder and the emb-offset table.
struct BlockDesc {
  enum Kind { CONV_IN, RES, ST, DOWN, UP } kind;
  std::string prefix;
  int cin, cout;
  int ds = 1;           // downsample factor of the feature map the block runs on (filled for ST blocks)
};
struct UNetTopo {
  std::vector<std::vector<BlockDesc>> input, output;
  std::vector<BlockDesc> middle;
  std::vector<int> in_ch;      // output channels of every input block (the skip stack)
  std::vector<int> in_ds;      // downsample factor (1,2,4,8) at the output of every input block
  std::vector<int> out_ds;     // ds at which every output block's ResBlock runs
  int final_ch = 0;
};

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
struct NetState {                 // context-dependent buffers shared between set_context and forward plans
  std::vector<bf16_t*> K, Vt;
  int ldvt = 0;
};

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
  bf16_t* ctxb = b.buf<bf16_t>((size_t)N * Tc * Dc);
  std::map<std::string, std::pair<bf16_t*, bf16_t*>> kv;
  std::map<std::string, Builder::PX> pxs;
  {
    const long n = (long)N * Tc * Dc;
    b.other("ctx.cast", [=](hipStream_t s, const RunArgs& a) { return launch_cast_bf16(a.aux, ctxb, n, s); });
    for (auto& d : sts) {
      const int tokens = (H / d.ds) * (W / d.ds);
      // the denoiser's context is set once per sample() call: fold it into per-sample operands where the shapes allow;
      // the classifier gets new features with every call and keeps the K / V^T form
      if (which == 0 && Builder::px_ok(d.cin, heads, Tc, tokens)) {
        pxs[d.prefix] = b.context_px(ctxb, N, Tc, Dc, d.prefix, d.cin, heads);
        kv[d.prefix] = {nullptr, nullptr};
        continue;
      }
      bf16_t *K, *Vt;
      b.context_kv(ctxb, N, Tc, Dc, d.prefix, d.cin, &K, &Vt, ldvtc);
      kv[d.prefix] = {K, Vt};
    }
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
    std::vector<std::string> wn, bn;
    for (auto& r : topo_resblocks(topo)) {
      wn.push_back(pre + r + ".emb_layers.1.weight");
      bn.push_back(pre + r + ".emb_layers.1.bias");
    }
    const bf16_t* w = c->w_stack(pre + "#embw", wn);
    const float* bb = c->b_stack(pre + "#embb", bn);
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
  const int cin = u.in_channels;
  if (cin < 1 || cin > 64) fail("in_channels = %d: the first conv's operand is one 64-channel K step (1 .. 64 input channels)", cin);
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


// ---------------------------------------------------------------------------------------------------------------
// Alignment classifier: forward + input gradient  g = d sum(log p) / d x   (cal_classifier_loglikelihood_grad,
// ddim.py:333-341; cond_grad_fn_classifier, dpm_solver.py:1340-1349).  The encoder is a chain, so the plan is built
// with a tape: every forward module pushes a closure that, given the gradient w.r.t. its output, appends the
// backward ops and returns the gradient w.r.t. its input.  Nothing is freed during the forward (the saved
// activations are the backward's operands).  Only activation gradients are formed -- weights are constants here.
void build_classifier_grad(df_ctx* c, Plan* pl, int N, int H, int W, int Tc) {
  const df_unet_config& u = c->ccfg;
  const std::string pre = "classifier.model.";
  Builder b{c, pl, pre, 1};
  UNetTopo topo = make_topo(u, true);
  const int mc = u.model_channels, temb = 4 * mc, HW = H * W, heads = u.num_heads, Dc = u.context_dim;
  if (u.out_channels != 1) fail("classifier gradient: out_channels must be 1");

  auto f32buf = [&](int rows, int C) { return F32{b.buf<float>((size_t)rows * C), rows, C, C}; };
  // dX = dY . W  for y = x W^T : plain GEMM against the transposed packing
  auto lin_bwd = [&](const bf16_t* dyb, int M, int O, const bf16_t* wt, int I, const char* tag, bool want_copy = false) {
    F32 dx = f32buf(M, I);
    GemmParams g = Builder::gp_linear(dyb, M, O, wt, I);
    Builder::out_f32(g, dx.p, I);
    if (want_copy) {      // the next backward GEMM reads this gradient as an operand: copy from this epilogue instead of a cast launch
      dx.b16 = b.buf<bf16_t>((size_t)M * I);
      g.aux = dx.b16;
      g.ld_aux = I;
    }
    b.gemm(g, 1, tag);
    return dx;
  };
  // backward-data of a stride-1 3x3 conv: conv of dY with flipped, transposed weights
  auto conv_bwd = [&](const bf16_t* dyb, int hh, int ww, int O, const std::string& wname, int I, const char* tag) {
    F32 dx = f32buf(N * hh * ww, I);
    GemmParams g = Builder::gp_conv3(dyb, N, hh, ww, O, c->w_conv3_bwd(wname), I, 1, 0);
    Builder::out_f32(g, dx.p, I);
    b.gemm(g, 1, tag);
    return dx;
  };
  auto gn_bwd = [&](const F32& x, const std::string& p, float eps, int silu, const F32& dy, const F32* addend,
                    bool want_b16, bf16_t** b16) {
    F32 dx = f32buf(x.rows, x.C);
    bf16_t* db = want_b16 ? b.buf<bf16_t>((size_t)x.rows * x.C) : nullptr;
    if (b16) *b16 = db;
    dx.b16 = db;
    const float* gm = c->f32(pre + p + ".weight");
    const float* bt = c->f32(pre + p + ".bias");
    const float *xp = x.p, *dyp = dy.p, *ap = addend ? addend->p : nullptr;
    const int ld = x.ld, hw = x.rows / N, C = x.C, lddy = dy.ld, ldadd = addend ? addend->ld : 0;
    float* dxp = dx.p;
    b.other("gn.bwd", [=](hipStream_t s, const RunArgs&) {
      return launch_groupnorm_bwd(xp, ld, N, hw, C, gm, bt, eps, silu, dyp, lddy, ap, ldadd, dxp, C, db, s);
    });
    return dx;
  };
  auto ln_bwd = [&](const F32& x, const std::string& p, const F32& dy, const F32& addend, bf16_t** b16) {
    F32 dx = f32buf(x.rows, x.C);
    bf16_t* db = b.buf<bf16_t>((size_t)x.rows * x.C);
    *b16 = db;
    const float* gm = c->f32(pre + p + ".weight");
    const float *xp = x.p, *dyp = dy.p, *ap = addend.p;
    const int rows = x.rows, C = x.C;
    float* dxp = dx.p;
    b.other("ln.bwd", [=](hipStream_t s, const RunArgs&) {
      return launch_layernorm_bwd(xp, rows, C, gm, 1e-5f, dyp, ap, dxp, db, s);
    });
    return dx;
  };

  // ---- context K / V^T (raw CAVP features, recomputed every call), time embedding, input packing
  std::vector<BlockDesc> sts = topo_sts(topo);
  const int ldvtc = rup(Tc, 32);
  bf16_t* ctxb = b.buf<bf16_t>((size_t)N * Tc * Dc);
  std::map<std::string, std::pair<bf16_t*, bf16_t*>> kv;
  {
    const long n = (long)N * Tc * Dc;
    b.other("ctx.cast", [=](hipStream_t s, const RunArgs& a) { return launch_cast_bf16(a.aux, ctxb, n, s); });
    for (auto& d : sts) {
      bf16_t *K, *Vt;
      b.context_kv(ctxb, N, Tc, Dc, d.prefix, d.cin, &K, &Vt, ldvtc);
      kv[d.prefix] = {K, Vt};
    }
  }
  pl->n_feat = pl->ops.size();        // everything above depends on the features only: skipped while the caller's token stands
  float* te = b.buf<float>((size_t)N * mc);
  b.other("t.embed", [=](hipStream_t s, const RunArgs& a) { return launch_timestep_embedding(a.t, te, N, mc, s); });
  float* e1 = b.buf<float>((size_t)N * temb);
  float* semb = b.buf<float>((size_t)N * temb);
  {
    const bf16_t* w0 = c->w_linear(pre + "time_embed.0.weight");
    const float* b0 = c->f32(pre + "time_embed.0.bias");
    const bf16_t* w2 = c->w_linear(pre + "time_embed.2.weight");
    const float* b2 = c->f32(pre + "time_embed.2.bias");
    b.other("t.mlp0", [=](hipStream_t s, const RunArgs&) { return launch_linear_rows(te, mc, w0, b0, e1, temb, N, temb, mc, 1, s); });
    b.other("t.mlp2", [=](hipStream_t s, const RunArgs&) { return launch_linear_rows(e1, temb, w2, b2, semb, temb, N, temb, temb, 1, s); });
  }
  const int etot = c->emb_total[1];
  float* E = b.buf<float>((size_t)N * etot);
  {
    std::vector<std::string> wn, bn;
    for (auto& r : topo_resblocks(topo)) {
      wn.push_back(pre + r + ".emb_layers.1.weight");
      bn.push_back(pre + r + ".emb_layers.1.bias");
    }
    const bf16_t* w = c->w_stack(pre + "#embw", wn);
    const float* bb = c->b_stack(pre + "#embb", bn);
    b.other("t.embproj", [=](hipStream_t s, const RunArgs&) { return launch_linear_rows(semb, temb, w, bb, E, etot, N, etot, temb, 0, s); });
  }
  const int cin = u.in_channels;
  if (cin < 1 || cin > 64) fail("in_channels = %d: the first conv's operand is one 64-channel K step (1 .. 64 input channels)", cin);
  bf16_t* xin = b.buf<bf16_t>((size_t)N * HW * 64);
  b.other("x.pack", [=](hipStream_t s, const RunArgs& a) { return launch_pack_latent(a.x, xin, N, cin, HW, 64, 1, 1.0f, nullptr, nullptr, s); });

  std::vector<std::function<F32(F32)>> tape;

  // ---- forward modules (each pushes its backward)
  auto fwd_conv_in = [&](const BlockDesc& d) {
    F32 h = f32buf(N * HW, d.cout);
    GemmParams g = Builder::gp_conv3(xin, N, H, W, 64, c->w_conv3(pre + d.prefix + ".weight", 64), d.cout, 1, 0);
    Builder::out_f32(g, h.p, h.ld);
    g.bias = c->f32(pre + d.prefix + ".bias");
    b.gemm(g, 1, "conv_in");
    const std::string wname = pre + d.prefix + ".weight";
    const int co = d.cout;
    tape.push_back([=, &b](F32 dh) mutable -> F32 {
      bf16_t* db = b.cast2d(dh);
      GemmParams g2 = Builder::gp_conv3(db, N, H, W, co, c->w_conv3_bwd(wname), cin, 1, 0);
      Builder::out_f32(g2, nullptr, cin);
      g2.store_nchw = 1;
      g2.hw_out = HW;
      Op& o = b.gemm(g2, 1, "conv_in.bwd");
      o.c_ext = true;                      // the final gradient goes straight to the caller's NCHW buffer
      return F32{};
    });
    return h;
  };

  auto fwd_res = [&](const BlockDesc& d, const F32& x, int hh, int ww) {
    const std::string p = d.prefix;
    const int ci = x.C, co = d.cout, M = x.rows;
    const bool has_skip = c->has(pre + p + ".skip_connection.weight");
    bf16_t* xraw = nullptr;
    bf16_t* a1 = b.groupnorm(x, N, p + ".in_layers.0", 1e-5f, 1, has_skip ? &xraw : nullptr);
    F32 h1 = f32buf(M, co);
    {
      GemmParams g = Builder::gp_conv3(a1, N, hh, ww, ci, c->w_conv3(pre + p + ".in_layers.2.weight", ci), co, 1, 0);
      Builder::out_f32(g, h1.p, co);
      g.bias = c->f32(pre + p + ".in_layers.2.bias");
      g.rowbias = E + c->emb_off[1].at(p); g.ld_rowbias = etot; g.rows_per_sample = hh * ww; g.rowbias_mode = 1;
      b.gemm(g, 1, "res.conv1");
    }
    bf16_t* a2 = b.groupnorm(h1, N, p + ".out_layers.0", 1e-5f, 1, nullptr);
    F32 out = f32buf(M, co);
    if (has_skip) {
      GemmParams g = Builder::gp_linear(xraw, M, ci, c->w_linear(pre + p + ".skip_connection.weight"), co);
      Builder::out_f32(g, out.p, co);
      g.bias = c->f32(pre + p + ".skip_connection.bias");
      b.gemm(g, 1, "res.skip");
    }
    {
      GemmParams g = Builder::gp_conv3(a2, N, hh, ww, co, c->w_conv3(pre + p + ".out_layers.3.weight", co), co, 1, 0);
      Builder::out_f32(g, out.p, co);
      g.bias = c->f32(pre + p + ".out_layers.3.bias");
      if (has_skip) { g.res = out.p; g.ldr = co; } else { g.res = x.p; g.ldr = x.ld; }
      b.gemm(g, 1, "res.conv2");
    }
    tape.push_back([=, &b](F32 dout) mutable -> F32 {
      bf16_t* dob = b.cast2d(dout);
      F32 d_a2 = conv_bwd(dob, hh, ww, co, pre + p + ".out_layers.3.weight", co, "res.conv2.bwd");
      bf16_t* d_h1b = nullptr;
      F32 d_h1 = gn_bwd(h1, p + ".out_layers.0", 1e-5f, 1, d_a2, nullptr, true, &d_h1b);
      (void)d_h1;
      F32 d_a1 = conv_bwd(d_h1b, hh, ww, co, pre + p + ".in_layers.2.weight", ci, "res.conv1.bwd");
      F32 ds = dout;
      if (has_skip)
        ds = lin_bwd(dob, M, co, c->w_stack_t(pre + p + ".skip#t", {pre + p + ".skip_connection.weight"}), ci, "res.skip.bwd");
      return gn_bwd(x, p + ".in_layers.0", 1e-5f, 1, d_a1, &ds, true, nullptr);      // + operand copy: the next tape entry's first GEMM reads it
    });
    return out;
  };

  auto fwd_down = [&](const BlockDesc& d, const F32& x, int hh, int ww) {
    bf16_t* hb = b.cast2d(x);
    F32 out = f32buf(x.rows / 4, d.cout);
    GemmParams g = Builder::gp_conv3(hb, N, hh, ww, d.cin, c->w_conv3(pre + d.prefix + ".op.weight", d.cin), d.cout, 2, 0);
    Builder::out_f32(g, out.p, d.cout);
    g.bias = c->f32(pre + d.prefix + ".op.bias");
    b.gemm(g, 1, "down");
    const std::string wname = pre + d.prefix + ".op.weight";
    const int ci = d.cin, co = d.cout;
    tape.push_back([=, &b](F32 dy) mutable -> F32 {
      bf16_t* dyb = b.cast2d(dy);
      F32 dx = f32buf(N * hh * ww, ci);
      // transposed stride-2 conv: conv over the zero-stuffed x2 grid of dY with flipped taps
      GemmParams g2 = Builder::gp_conv3(dyb, N, hh / 2, ww / 2, co, c->w_conv3_bwd(wname), ci, 1, 1);
      g2.zstuff = 1;
      Builder::out_f32(g2, dx.p, ci);
      dx.b16 = b.buf<bf16_t>((size_t)N * hh * ww * ci);      // operand copy for the tape entry in front (its conv2.bwd reads it)
      g2.aux = dx.b16;
      g2.ld_aux = ci;
      b.gemm(g2, 1, "down.bwd");
      return dx;
    });
    return out;
  };

  auto fwd_st = [&](const BlockDesc& d, const F32& x, int T) {
    const std::string p = d.prefix, tb = p + ".transformer_blocks.0";
    const int C = x.C, M = x.rows, D = C / heads;
    if (!attention_supported(D) || !(D == 32 || D == 64)) fail("classifier gradient: head dim %d not supported", D);
    const float scale = 1.0f / sqrtf((float)D);
    const bf16_t* ctxK = kv[p].first;
    const bf16_t* ctxVt = kv[p].second;
    bf16_t* a0 = b.groupnorm(x, N, p + ".norm", 1e-6f, 0, nullptr);
    F32 t0 = f32buf(M, C), t1 = f32buf(M, C), t2 = f32buf(M, C), out = f32buf(M, C);
    bf16_t* a = b.buf<bf16_t>((size_t)M * C);
    {
      GemmParams g = Builder::gp_linear(a0, M, C, c->w_linear(pre + p + ".proj_in.weight"), C);
      Builder::out_f32(g, t0.p, C);
      g.bias = c->f32(pre + p + ".proj_in.bias");
      b.gemm(g, 1, "st.proj_in");
    }
    b.layernorm(t0, tb + ".norm1", a);
    bf16_t* qk = b.buf<bf16_t>((size_t)M * 2 * C);
    {
      const bf16_t* w = c->w_stack(pre + tb + ".attn1.qk", {pre + tb + ".attn1.to_q.weight", pre + tb + ".attn1.to_k.weight"});
      GemmParams g = Builder::gp_linear(a, M, C, w, 2 * C);
      Builder::out_b16(g, qk, 2 * C);
      b.gemm(g, 1, "st.qk");
    }
    const int ldvt = rup(T, 32);
    bf16_t* vt = b.buf<bf16_t>((size_t)N * C * ldvt);
    {
      GemmParams g = Builder::gp_linear(c->w_linear(pre + tb + ".attn1.to_v.weight"), C, C, a, T);
      g.w_bs = (long)T * C;
      Builder::out_b16(g, vt, ldvt);
      g.c_bs = (long)C * ldvt;
      b.gemm(g, N, "st.vT");
    }
    bf16_t* o = b.buf<bf16_t>((size_t)M * C);
    b.other("attn.self", [=](hipStream_t s, const RunArgs&) {
      return launch_attention(qk, 2 * C, qk + C, 2 * C, vt, ldvt, o, C, N, heads, D, T, T, scale, s);
    });
    {
      GemmParams g = Builder::gp_linear(o, M, C, c->w_linear(pre + tb + ".attn1.to_out.0.weight"), C);
      Builder::out_f32(g, t1.p, C);
      g.bias = c->f32(pre + tb + ".attn1.to_out.0.bias");
      g.res = t0.p; g.ldr = C;
      b.gemm(g, 1, "st.attn1.out");
    }
    b.layernorm(t1, tb + ".norm2", a);
    bf16_t* q2 = b.buf<bf16_t>((size_t)M * C);
    {
      GemmParams g = Builder::gp_linear(a, M, C, c->w_linear(pre + tb + ".attn2.to_q.weight"), C);
      Builder::out_b16(g, q2, C);
      b.gemm(g, 1, "st.q2");
    }
    b.other("attn.cross", [=](hipStream_t s, const RunArgs&) {
      return launch_attention(q2, C, ctxK, C, ctxVt, ldvtc, o, C, N, heads, D, T, Tc, scale, s);
    });
    {
      GemmParams g = Builder::gp_linear(o, M, C, c->w_linear(pre + tb + ".attn2.to_out.0.weight"), C);
      Builder::out_f32(g, t2.p, C);
      g.bias = c->f32(pre + tb + ".attn2.to_out.0.bias");
      g.res = t1.p; g.ldr = C;
      b.gemm(g, 1, "st.attn2.out");
    }
    b.layernorm(t2, tb + ".norm3", a);
    bf16_t* uu = b.buf<bf16_t>((size_t)M * 8 * C);       // raw [x | gate] of the GEGLU projection (saved)
    {
      GemmParams g = Builder::gp_linear(a, M, C, c->w_linear(pre + tb + ".ff.net.0.proj.weight"), 8 * C);
      Builder::out_b16(g, uu, 8 * C);
      g.bias = c->f32(pre + tb + ".ff.net.0.proj.bias");
      b.gemm(g, 1, "st.ff1.raw");
    }
    bf16_t* gl = b.buf<bf16_t>((size_t)M * 4 * C);
    b.other("geglu", [=](hipStream_t s, const RunArgs&) { return launch_geglu_fwd(uu, gl, (long)M, 4 * C, s); });
    {
      GemmParams g = Builder::gp_linear(gl, M, 4 * C, c->w_linear(pre + tb + ".ff.net.2.weight"), C);
      Builder::out_b16(g, a, C);
      g.bias = c->f32(pre + tb + ".ff.net.2.bias");
      g.res = t2.p; g.ldr = C;
      b.gemm(g, 1, "st.ff2");
    }
    {
      GemmParams g = Builder::gp_linear(a, M, C, c->w_linear(pre + p + ".proj_out.weight"), C);
      Builder::out_f32(g, out.p, C);
      g.bias = c->f32(pre + p + ".proj_out.bias");
      g.res = x.p; g.ldr = x.ld;
      b.gemm(g, 1, "st.proj_out");
    }
    tape.push_back([=, &b](F32 dout) mutable -> F32 {
      auto wt = [&](const std::string& n) { return c->w_stack_t(pre + n + "#t", {pre + n}); };
      bf16_t* doutb = b.cast2d(dout);
      F32 dt3 = lin_bwd(doutb, M, C, wt(p + ".proj_out.weight"), C, "st.proj_out.bwd", true);
      bf16_t* dt3b = b.cast2d(dt3);
      F32 dgl = lin_bwd(dt3b, M, C, wt(tb + ".ff.net.2.weight"), 4 * C, "st.ff2.bwd");
      bf16_t* du = b.buf<bf16_t>((size_t)M * 8 * C);
      {
        const float* dglp = dgl.p;
        b.other("geglu.bwd", [=](hipStream_t s, const RunArgs&) { return launch_geglu_bwd(uu, dglp, du, (long)M, 4 * C, s); });
      }
      F32 da3 = lin_bwd(du, M, 8 * C, wt(tb + ".ff.net.0.proj.weight"), C, "st.ff1.bwd");
      bf16_t* dt2b = nullptr;
      F32 dt2 = ln_bwd(t2, tb + ".norm3", da3, dt3, &dt2b);
      // cross attention (context is a constant: dQ only)
      F32 do2 = lin_bwd(dt2b, M, C, wt(tb + ".attn2.to_out.0.weight"), C, "st.attn2.out.bwd");
      bf16_t* dq2 = b.buf<bf16_t>((size_t)M * C);
      {
        const float* dop = do2.p;
        b.other("attn.cross.bwd", [=](hipStream_t s, const RunArgs&) {
          return launch_attention_bwd(q2, C, ctxK, C, ctxVt, ldvtc, dop, C, dq2, C, nullptr, 0, nullptr, 0, N, heads, D, T, Tc,
                                      scale, nullptr, s);
        });
      }
      F32 da2 = lin_bwd(dq2, M, C, wt(tb + ".attn2.to_q.weight"), C, "st.q2.bwd");
      bf16_t* dt1b = nullptr;
      F32 dt1 = ln_bwd(t1, tb + ".norm2", da2, dt2, &dt1b);
      // self attention
      F32 do1 = lin_bwd(dt1b, M, C, wt(tb + ".attn1.to_out.0.weight"), C, "st.attn1.out.bwd");
      bf16_t* dqkv = b.buf<bf16_t>((size_t)M * 3 * C);
      {
        const float* dop = do1.p;
        const size_t nws = attention_bwd_ws_floats(N, heads, D, T, T, 3 * C, 3 * C, true);      // > 0: the tiled pair (long maps)
        float* ws = nws ? b.buf<float>(nws) : nullptr;
        b.other("attn.self.bwd", [=](hipStream_t s, const RunArgs&) {
          return launch_attention_bwd(qk, 2 * C, qk + C, 2 * C, vt, ldvt, dop, C, dqkv, 3 * C, dqkv + C, 3 * C, dqkv + 2 * C,
                                      3 * C, N, heads, D, T, T, scale, ws, s);
        });
      }
      const bf16_t* wqkv_t = c->w_stack_t(pre + tb + ".attn1.qkv#t", {pre + tb + ".attn1.to_q.weight", pre + tb + ".attn1.to_k.weight",
                                                                       pre + tb + ".attn1.to_v.weight"});
      F32 da1 = lin_bwd(dqkv, M, 3 * C, wqkv_t, C, "st.qkv.bwd");
      bf16_t* dt0b = nullptr;
      F32 dt0 = ln_bwd(t0, tb + ".norm1", da1, dt1, &dt0b);
      (void)dt0;
      F32 da0 = lin_bwd(dt0b, M, C, wt(p + ".proj_in.weight"), C, "st.proj_in.bwd");
      return gn_bwd(x, p + ".norm", 1e-6f, 0, da0, &dout, true, nullptr);
    });
    return out;
  };

  // ---- forward
  F32 h{};
  const int nin = (int)topo.input.size();
  for (int k = 0; k < nin; ++k) {
    for (auto& d : topo.input[k]) {
      const int ds = (d.kind == BlockDesc::DOWN) ? topo.in_ds[k] / 2 : topo.in_ds[k];
      const int hh = H / ds, ww = W / ds;
      if (d.kind == BlockDesc::CONV_IN) h = fwd_conv_in(d);
      else if (d.kind == BlockDesc::RES) h = fwd_res(d, h, hh, ww);
      else if (d.kind == BlockDesc::ST) h = fwd_st(d, h, hh * ww);
      else if (d.kind == BlockDesc::DOWN) h = fwd_down(d, h, hh, ww);
      else fail("classifier gradient: unexpected block kind");
    }
  }
  const int ds_mid = topo.in_ds.back(), hm = H / ds_mid, wmid = W / ds_mid;
  for (auto& d : topo.middle) {
    if (d.kind == BlockDesc::RES) h = fwd_res(d, h, hm, wmid);
    else h = fwd_st(d, h, hm * wmid);
  }
  // head: GN -> SiLU -> conv3x3 -> global avg-pool -> Linear -> sigmoid (alignment_backbone.py:630-638)
  const int chf = topo.final_ch, co = chf / 2, hw2 = hm * wmid;
  bf16_t* ah = b.groupnorm(h, N, "out.0", 1e-5f, 1, nullptr);
  F32 ho = f32buf(h.rows, co);
  {
    GemmParams g = Builder::gp_conv3(ah, N, hm, wmid, chf, c->w_conv3(pre + "out.2.weight", chf), co, 1, 0);
    Builder::out_f32(g, ho.p, co);
    g.bias = c->f32(pre + "out.2.bias");
    b.gemm(g, 1, "cls.out");
  }
  float* pooled = b.buf<float>((size_t)N * rup(co, 8));
  float* prob = b.buf<float>((size_t)rup(N, 8));
  {
    const float* hop = ho.p;
    b.other("cls.pool", [=](hipStream_t s, const RunArgs&) { return launch_avgpool(hop, pooled, N, hw2, co, s); });
    const bf16_t* wc = c->w_linear(pre + "classifier.weight");
    const float* bc = c->f32(pre + "classifier.bias");
    b.other("cls.head", [=](hipStream_t s, const RunArgs& ar) {
      hipError_t e = launch_linear_rows(pooled, co, wc, bc, prob, 1, N, 1, co, 2, s);
      if (e == hipSuccess && ar.out2) e = hipMemcpyAsync(ar.out2, prob, (size_t)N * 4, hipMemcpyDeviceToDevice, s);
      return e;
    });
  }
  // ---- backward: head, then the tape in reverse
  const int cop = rup(co, 64);          // the gradient operand's row length: co columns + zero pad up to the K step (w_conv3_bwd)
  F32 dho = f32buf(h.rows, co);
  bf16_t* dhob = b.buf<bf16_t>((size_t)h.rows * cop);
  {
    const float* wcls = c->f32(pre + "classifier.weight");
    float* dp = dho.p;
    // the VJP of the logit (cotangent 1); 1 - p_n is applied to the finished gradient in fp32 (cls.grad.scale): folded into the
    // cotangent here it took a confident sample's fp16 gradient operands into the subnormal range
    b.other("cls.head.bwd", [=](hipStream_t s, const RunArgs&) { return launch_cls_head_bwd(nullptr, wcls, dp, dhob, N, hw2, co, cop, s); });
  }
  F32 d_ah = conv_bwd(dhob, hm, wmid, cop, pre + "out.2.weight", chf, "cls.out.bwd");
  F32 g = gn_bwd(h, "out.0", 1e-5f, 1, d_ah, nullptr, true, nullptr);
  for (int i = (int)tape.size() - 1; i >= 0; --i) g = tape[i](g);
  const long per = (long)cin * HW;
  b.other("cls.grad.scale", [=](hipStream_t s, const RunArgs& a) { return launch_grad_scale_per_sample(a.out, prob, N, per, s); });
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
  {  // AttnBlock (model.py:273-297): single head over hh*ww tokens, head dim = ch -> GEMM + row-softmax + GEMM
    const std::string p = "decoder.mid.attn_1";
    const int T = hh * ww, M = B * T;
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
      b.gemm(g, 1, "vae.q");
    }
    {
      GemmParams g = Builder::gp_linear(a, M, ch, c->w_linear(pre + p + ".k.weight"), ch);
      Builder::out_b16(g, k, ch);
      g.bias = c->f32(pre + p + ".k.bias");
      b.gemm(g, 1, "vae.k");
    }
    {  // V^T without its bias: softmax rows sum to 1, so P(V + 1 b^T) = P V + b^T -> bias added after P V
      if (Tp != T) {
        const size_t nb = (size_t)B * ch * Tp * sizeof(bf16_t);
        b.other("vae.vT.pad", [=](hipStream_t s, const RunArgs&) { return hipMemsetAsync(vt, 0, nb, s); });
      }
      GemmParams g = Builder::gp_linear(c->w_linear(pre + p + ".v.weight"), ch, ch, a, T);
      g.w_bs = (long)T * ch;
      Builder::out_b16(g, vt, Tp);
      g.c_bs = (long)ch * Tp;
      b.gemm(g, B, "vae.vT");
    }
    float* sc = b.buf<float>((size_t)B * T * T);
    {
      GemmParams g = Builder::gp_linear(q, T, ch, k, T);
      g.a_bs = (long)T * ch;
      g.w_bs = (long)T * ch;
      Builder::out_f32(g, sc, T);
      g.c_bs = (long)T * T;
      g.alpha = 1.0f / sqrtf((float)ch);
      b.gemm(g, B, "vae.qk");
    }
    bf16_t* pr = b.buf<bf16_t>((size_t)B * T * Tp);
    b.other("vae.softmax", [=](hipStream_t s, const RunArgs&) { return launch_softmax_rows(sc, pr, B * T, T, Tp, s); });
    bf16_t* o = q;
    {
      GemmParams g = Builder::gp_linear(pr, T, Tp, vt, ch);
      g.a_bs = (long)T * Tp;
      g.w_bs = (long)ch * Tp;
      Builder::out_b16(g, o, ch);
      g.c_bs = (long)T * ch;
      g.bias = c->f32(pre + p + ".v.bias");
      b.gemm(g, B, "vae.pv");
    }
    F32 ho{b.buf<float>((size_t)M * ch), M, ch, ch};
    {
      GemmParams g = Builder::gp_linear(o, M, ch, c->w_linear(pre + p + ".proj_out.weight"), ch);
      Builder::out_f32(g, ho.p, ch);
      g.bias = c->f32(pre + p + ".proj_out.bias");
      g.res = h.p; g.ldr = h.ld;
      b.gemm(g, 1, "vae.proj_out");
    }
    for (void* p_ : {(void*)a, (void*)q, (void*)k, (void*)vt, (void*)sc, (void*)pr, (void*)h.p}) pl->release(p_);
    h = ho;
  }
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

void finish_plan(df_ctx* c, Plan* pl) {
  if (pl->partial_bytes) {
    HIPCHK(hipMalloc((void**)&pl->partial, pl->partial_bytes));
    for (auto& o : pl->ops)
      if (o.is_gemm && o.gp.splitk > 1) o.gp.partial = pl->partial;
  }
  HIPCHK(hipStreamSynchronize(c->pack_stream));   // weight packing done before first use
}

int op_family(const Op& o) {
  if (o.is_gemm) return 0;
  if (!strncmp(o.tag, "attn", 4)) return 1;
  if (!strcmp(o.tag, "groupnorm")) return 2;
  if (!strcmp(o.tag, "layernorm")) return 3;
  return 4;
}

struct ChkBuf { const uint32_t* p; unsigned long long words; };
// Order-independent (integer) checksum of a list of buffers: grid (x, buffer), one 64-bit atomic add per wavefront.
__global__ __launch_bounds__(256) void checksum_kernel(const ChkBuf* list, unsigned long long* slot) {
  const ChkBuf b = list[blockIdx.y];
  unsigned long long acc = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < b.words; i += (unsigned long long)gridDim.x * 256)
    acc += (unsigned long long)b.p[i] * (unsigned long long)((i & 1023u) + 1u);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(slot, acc);
}

void checksum_after_op(df_ctx* c, Plan* pl, size_t op_index, hipStream_t s) {
  if (!pl->chk_list) {
    std::vector<ChkBuf> v;
    for (auto& b : pl->owned) v.push_back({(const uint32_t*)b.p, (unsigned long long)(b.bytes / 4)});
    if (pl->partial) v.push_back({(const uint32_t*)pl->partial, (unsigned long long)(pl->partial_bytes / 4)});
    pl->chk_n = (int)v.size();
    if (!v.empty()) {
      HIPCHK(hipMalloc(&pl->chk_list, v.size() * sizeof(ChkBuf)));
      HIPCHK(hipMemcpy(pl->chk_list, v.data(), v.size() * sizeof(ChkBuf), hipMemcpyHostToDevice));
    }
  }
  if (c->chk_used >= c->chk_cap || pl->chk_n == 0) return;
  hipLaunchKernelGGL(checksum_kernel, dim3(64, pl->chk_n), dim3(256), 0, s, (const ChkBuf*)pl->chk_list, c->chk_dev + c->chk_used);
  char lab[160];
  snprintf(lab, sizeof lab, "%s#%zu:%s", pl->name.c_str(), op_index, pl->ops[op_index].tag);
  if (pl->ops[op_index].is_gemm) {
    const Op& o = pl->ops[op_index];
    const size_t n = strlen(lab);
    snprintf(lab + n, sizeof lab - n, " %dx%dx%d taps%d tile%d sk%d", o.gp.M, o.gp.N, o.gp.K, o.gp.taps, o.tile, o.gp.splitk);
  }
  c->chk_label.push_back(lab);
  ++c->chk_used;
}

// Operand-type values at the saturation point of the operand format: fp16 build -- |v| == 65504, where pack_bf2 / f2bf clamp
// (common.h); bf16 build -- non-finite (bf16 keeps the fp32 range and is not clamped).  One 64-bit atomic add per wavefront.
__global__ __launch_bounds__(256) void sat_count_kernel(const uint16_t* p, long rows, int cols, int ld, unsigned long long* slot) {
  const long total = rows * (long)cols;
  unsigned long long acc = 0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / cols;
    const uint16_t v = p[r * ld + (e - r * cols)];
#if defined(DF_OPERAND_F16)
    acc += (v & 0x7FFFu) == 0x7BFFu;
#else
    acc += (v & 0x7F80u) == 0x7F80u;
#endif
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(slot, acc);
}

void saturations_after_op(df_ctx* c, Plan* pl, size_t op_index, hipStream_t s) {
  if (c->sat_used >= c->sat_cap) return;
  const Op& o = pl->ops[op_index];
  std::vector<OutBuf> outs = o.outs;
  if (o.is_gemm) {
    const GemmParams& g = o.gp;
    const long rows = (long)g.M * (g.taps == 4 ? 4 : 1) + g.dup_rows;     // dup_rows: rows [M, M + dup_rows) repeat [0, M)
    const int cols = g.geglu ? g.N / 2 : (g.vt ? g.vt_col0 : g.N);
    if (g.out_bf16 && g.C && !o.c_ext && !g.store_nchw)
      for (int z = 0; z < (g.splitk > 1 ? 1 : o.batch); ++z) outs.push_back({(const uint16_t*)g.C + (long)z * g.c_bs, rows, cols, g.ldc});
    if (g.aux) outs.push_back({g.aux, rows, g.N, g.ld_aux});
    if (g.vt) outs.push_back({g.vt, (long)(g.M / g.vt_T) * (g.N - g.vt_col0), g.vt_T, g.ldvt});
  }
  for (auto& b : outs) {
    const long total = b.rows * (long)b.cols;
    if (total <= 0) continue;
    const int blocks = (int)std::min<long>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(sat_count_kernel, dim3(blocks), dim3(256), 0, s, b.p, b.rows, b.cols, b.ld, c->sat_dev + c->sat_used);
  }
  char lab[160];
  snprintf(lab, sizeof lab, "%s#%zu:%s", pl->name.c_str(), op_index, o.tag);
  c->sat_label.push_back(lab);
  ++c->sat_used;
}

// Operand-type values re-rounded to bf16's 8 significant bits (round to nearest even on the fp16 pattern: 3 of its 10 mantissa bits
// go; values below bf16's fp16-representable range are kept).  fp16 build only; the bf16 build's values are already there.
__global__ __launch_bounds__(256) void requant_bf16_kernel(uint16_t* p, long rows, int cols, int ld) {
#if defined(DF_OPERAND_F16)
  const long total = rows * (long)cols;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / cols;
    uint16_t* q = p + r * ld + (e - r * cols);
    const uint16_t v = *q;
    if ((v & 0x7C00u) == 0x7C00u) continue;             // inf / nan
    const uint16_t lsb = (v >> 3) & 1u;
    *q = (uint16_t)((v + 3u + lsb) & 0xFFF8u);
  }
#endif
}

void requant_after_op(df_ctx* c, Plan* pl, size_t op_index, hipStream_t s) {
  const Op& o = pl->ops[op_index];
  bool hit = false;
  for (auto& pre : c->rq_prefix)
    if (pre == "*" || !strncmp(o.tag, pre.c_str(), pre.size())) hit = true;
  if (!hit) return;
  std::vector<OutBuf> outs = o.outs;
  if (o.is_gemm) {
    const GemmParams& g = o.gp;
    const long rows = (long)g.M * (g.taps == 4 ? 4 : 1) + g.dup_rows;
    const int cols = g.geglu ? g.N / 2 : (g.vt ? g.vt_col0 : g.N);
    if (g.out_bf16 && g.C && !o.c_ext && !g.store_nchw)
      for (int z = 0; z < (g.splitk > 1 ? 1 : o.batch); ++z) outs.push_back({(const uint16_t*)g.C + (long)z * g.c_bs, rows, cols, g.ldc});
    if (g.aux) outs.push_back({g.aux, rows, g.N, g.ld_aux});
    if (g.vt) outs.push_back({g.vt, (long)(g.M / g.vt_T) * (g.N - g.vt_col0), g.vt_T, g.ldvt});
  }
  for (auto& b : outs) {
    const long total = b.rows * (long)b.cols;
    if (total <= 0) continue;
    const int blocks = (int)std::min<long>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(requant_bf16_kernel, dim3(blocks), dim3(256), 0, s, const_cast<uint16_t*>(b.p), b.rows, b.cols, b.ld);
  }
}

void run_ops(df_ctx* c, Plan* pl, size_t begin, size_t end, hipStream_t s, const RunArgs& a) {
  for (size_t i = begin; i < end; ++i) {
    Op& o = pl->ops[i];
    hipError_t e;
    (void)hipGetLastError();     // a stale launch-configuration error (e.g. a refused tuning candidate) is not this op's
    if (c->prof_on) {
      if (c->prof_used + 2 > c->prof_ev.size()) {
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        c->prof_ev.push_back(e0);
        c->prof_ev.push_back(e1);
      }
      HIPCHK(hipEventRecord(c->prof_ev[c->prof_used], s));
    }
    if (o.is_gemm) {
      GemmParams g = o.gp;
      if (o.c_ext) g.C = a.out;
      if (o.cfg_ext && g.splitk > 1) { g.cfg_out = a.out; g.cfg_scale = a.scale; }
      if (o.defer && g.splitk > 1) g.defer_reduce = 1;
      e = launch_gemm(g, o.tile, o.batch, s);
    } else {
      e = o.fn(s, a);
    }
    if (e != hipSuccess) {
      if (o.is_gemm)
        fail("op %zu (%s: GEMM %dx%dx%d taps %d batch %d tile %d split-K %d) failed: %s", i, o.tag, o.gp.M, o.gp.N, o.gp.K,
             o.gp.taps, o.batch, o.tile, o.gp.splitk, hipGetErrorString(e));
      fail("op %zu (%s) failed: %s", i, o.tag, hipGetErrorString(e));
    }
    if (c->prof_on) {
      HIPCHK(hipEventRecord(c->prof_ev[c->prof_used + 1], s));
      c->prof_fam.push_back(op_family(o));
      c->prof_op.push_back(&o);
      c->prof_used += 2;
    }
    if (!c->rq_prefix.empty()) requant_after_op(c, pl, i, s);
    if (c->chk_on) checksum_after_op(c, pl, i, s);
    if (c->sat_on) saturations_after_op(c, pl, i, s);
    static const bool trace = getenv("DF_TRACE_OPS") && atoi(getenv("DF_TRACE_OPS"));     // debug: name + sync every op
    if (trace) {
      fprintf(stderr, "[df] %s#%zu %s%s\n", pl->name.c_str(), i, o.tag, o.is_gemm ? (" tile " + std::to_string(o.tile) + " sk " + std::to_string(o.gp.splitk)).c_str() : "");
      HIPCHK(hipStreamSynchronize(s));
    }
  }
}

// Autotune, stage 1: time every (tile, split-K) candidate of every distinct GEMM of the plan in isolation (3 launches
// back to back, operands cache-warm) and rank them ("measure, don't guess").
// Stage 2 (in situ): the isolated ranking mispredicts layers whose operands arrive cold from HBM/MALL or whose
// neighbours leave the CUs half busy, so the best DF_TUNE_TOPK candidates of every GEMM are re-timed INSIDE the plan:
// round r runs the whole plan with every GEMM on its r-th candidate (HIP events around each op), and each distinct
// GEMM keeps the candidate with the smallest in-plan time summed over its instances.
struct TuneCand { int tile, sk; float iso_ms; double situ_ms; };

static std::string tune_key(const Op& o) {
  const GemmParams& g = o.gp;
  char key[160];
  const int epi = (g.silu ? 128 : 0) | (g.ln_stats ? 1 : 0) | (g.stats ? 2 : 0) | (g.vt ? 4 : 0) | (g.aux ? 8 : 0) | (g.res ? 16 : 0) | (g.Cin2 ? 32 : 0) |
                  (o.defer ? 64 : 0) | (g.dup_rows ? 256 : 0);
  snprintf(key, sizeof key, "%d_%d_%d_%d_%d_%d_%d_%d_e%d", g.M, g.N, g.K, g.taps, g.stride, g.ups, o.batch, g.geglu, epi);
  return key;
}

// Optional persistent tuning results (env DF_TUNE_CACHE=<file>): one line "key tile splitk gm" per distinct GEMM.  A plan
// whose GEMMs are all in the file is configured from it without a single trial launch (profiling runs use this so
// that rocprof sees only the product launches); otherwise the plan is tuned and its results are appended.
struct TuneChoice { int tile, sk, gm; };
static std::map<std::string, TuneChoice>& tune_cache() {
  static std::map<std::string, TuneChoice> m;
  static bool loaded = false;
  if (!loaded) {
    loaded = true;
    if (const char* path = getenv("DF_TUNE_CACHE")) {
      if (FILE* f = fopen(path, "r")) {
        char key[160];
        TuneChoice ch;
        while (fscanf(f, "%159s %d %d %d", key, &ch.tile, &ch.sk, &ch.gm) == 4) m[key] = ch;
        fclose(f);
      }
    }
  }
  return m;
}
static void tune_cache_save() {
  const char* path = getenv("DF_TUNE_CACHE");
  if (!path) return;
  FILE* f = fopen(path, "w");
  if (!f) return;
  for (auto& kv : tune_cache()) fprintf(f, "%s %d %d %d\n", kv.first.c_str(), kv.second.tile, kv.second.sk, kv.second.gm);
  fclose(f);
}

// Set by df_tune_cache_import: another rank's choices were handed to this process.  Plans then take every choice the cache holds
// for their GEMMs whether or not df_autotune is on here -- the ranks of a job must run the SAME tiles and split-K factors
// (identical fp32 summation order, bit-equal results; parallel.broadcast_packed_model), and an importing rank that never asked
// for tuning used to fall back to the heuristic tiles silently.
static bool g_tune_imported = false;

// A GEMM the table does not hold takes the entry of its NEAREST ROW COUNT among the entries that agree in everything else
// (N, K, taps, stride, upsampling, batch count, GEGLU, epilogue class): the table is made at sampler batches 1-8 and 16, and another
// batch size or latent width changes M only -- the tile family that wins at M = 8192 still wins at 10240.  Within a factor of 4 in M;
// the choice is validated for the actual problem like an exact hit.  (Round 6: B = 10 without this ran the cost-model plan.)
static const TuneChoice* nearest_tune_choice(const std::string& key) {
  const size_t us = key.find('_');
  if (us == std::string::npos) return nullptr;
  const std::string suffix = key.substr(us);
  const double m = (double)atol(key.substr(0, us).c_str());
  if (m <= 0) return nullptr;
  const TuneChoice* best = nullptr;
  double bestd = 2.0001;           // |log2(M' / M)| <= 2
  for (auto& kv : tune_cache()) {
    const size_t u2 = kv.first.find('_');
    if (u2 == std::string::npos || kv.first.compare(u2, std::string::npos, suffix) != 0) continue;
    const double m2 = (double)atol(kv.first.substr(0, u2).c_str());
    if (m2 <= 0) continue;
    const double d = fabs(log2(m2 / m));
    if (d < bestd) {
      bestd = d;
      best = &kv.second;
    }
  }
  return best;
}

static void apply_tune_cache(Plan* pl) {
  auto& tc = tune_cache();
  for (auto& o : pl->ops) {
    if (!o.is_gemm || o.c_ext) continue;
    const std::string key = tune_key(o);
    auto it = tc.find(key);
    const TuneChoice* chp = it != tc.end() ? &it->second : nearest_tune_choice(key);
    if (!chp) continue;
    const TuneChoice& ch = *chp;
    const size_t need = (size_t)ch.sk * o.gp.M * o.gp.N * 4 * (o.gp.taps == 4 ? 4 : 1);
    if (!gemm_tile_valid(o.gp, ch.tile, o.batch, ch.sk) || (ch.sk > 1 && need > pl->partial_bytes)) continue;
    o.tile = ch.tile;
    o.gp.splitk = ch.sk;
    o.gp.gm = ch.gm;
    o.gp.partial = pl->partial;
  }
}

void autotune_plan(df_ctx* c, Plan* pl, hipStream_t s) {
  {
    auto& tc = tune_cache();      // in-memory for the life of the process (+ the file when DF_TUNE_CACHE is set)
    bool all = !tc.empty();
    for (auto& o : pl->ops)
      if (o.is_gemm && !o.c_ext && !tc.count(tune_key(o))) all = false;
    if (all) {
      apply_tune_cache(pl);
      tune_cache_save();     // DF_TUNE_CACHE may name a file this process has not written yet
      return;
    }
  }
  struct SaveOnExit {
    Plan* pl;
    ~SaveOnExit() {
      for (auto& o : pl->ops)
        if (o.is_gemm && !o.c_ext) tune_cache()[tune_key(o)] = {o.tile, o.gp.splitk, o.gp.gm};
      tune_cache_save();
    }
  } save_on_exit{pl};
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  std::map<std::string, std::vector<TuneCand>> cands;
  static const int tile_cap = getenv("DF_TILE_CAP") ? atoi(getenv("DF_TILE_CAP")) : TILE_ALL;   // tools: A/B a tile family
  // Candidates per GEMM class that go on to the in-plan stage.  The isolated ranking is a weak predictor of the in-plan time
  // (operands cold, neighbours' traffic): widening 6 -> 12 -> 40 measured 231.2 -> 235.8 and 232.5 -> 233.7 -> 234.5 steps/s on
  // two boxes, for ~1 s more tuning per plan (40 plan runs of 4 ms x 4 repetitions).
  static const int topk = getenv("DF_TUNE_TOPK") ? atoi(getenv("DF_TUNE_TOPK")) : 32;           // 1 = stage 1 only
  for (auto& o : pl->ops) {
    if (!o.is_gemm || o.c_ext) continue;
    const std::string key = tune_key(o);
    if (cands.count(key)) continue;
    GemmParams g = o.gp;
    std::vector<TuneCand>& v = cands[key];
    static const unsigned long tile_skip = getenv("DF_TILE_SKIP") ? strtoul(getenv("DF_TILE_SKIP"), nullptr, 0) : 0ul;   // tools: bit mask
    for (int t = 0; t < TILE_ALL && t < tile_cap; ++t) {
      if ((tile_skip >> t) & 1) continue;
      // 3 * 2^k splits too: 2 M tiles x 20 N tiles x 6 = 240 blocks fill 256 CUs where 4 / 8 give 160 / 320 (tools/cold_probe.py:
      // sk 3 / 6 / 12 are the best factor of most weight-streaming layers)
      static const int sks[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
      for (int si = 0; si < 10; ++si) {
        const int sk = sks[si];
        if (!gemm_tile_valid(g, t, o.batch, sk)) { if (sk > 1) break; else continue; }
        const size_t need = (size_t)sk * g.M * g.N * 4 * (g.taps == 4 ? 4 : 1);
        if (sk > 1 && need > pl->partial_bytes) break;
        GemmParams q = g;
        q.splitk = sk;
        q.partial = pl->partial;
        // res may alias C: results are garbage during tuning but are recomputed by the next real run
        if (launch_gemm(q, t, o.batch, s) != hipSuccess) continue;
        HIPCHK(hipEventRecord(e0, s));
        for (int r = 0; r < 3; ++r) (void)launch_gemm(q, t, o.batch, s);
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        v.push_back({t, sk, ms, 0.0});
      }
    }
    if (v.empty()) v.push_back({o.tile, g.splitk, 0.f, 0.0});
    std::sort(v.begin(), v.end(), [](const TuneCand& a, const TuneCand& b) { return a.iso_ms < b.iso_ms; });
    if ((int)v.size() > topk) v.resize(topk > 0 ? topk : 1);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  auto apply = [&](int round) {   // round < 0: the best in-situ candidate
    for (auto& o : pl->ops) {
      if (!o.is_gemm || o.c_ext) continue;
      const std::vector<TuneCand>& v = cands[tune_key(o)];
      int idx = 0;
      if (round >= 0) idx = std::min(round, (int)v.size() - 1);
      else
        for (int k = 1; k < (int)v.size(); ++k)
          if (v[k].situ_ms < v[idx].situ_ms) idx = k;
      o.tile = v[idx].tile;
      o.gp.splitk = v[idx].sk;
      o.gp.partial = pl->partial;
    }
  };
  size_t rounds = 0;
  for (auto& kv : cands) rounds = std::max(rounds, kv.second.size());
  if (rounds <= 1) { apply(0); return; }
  // stage 2: dummy external buffers (timing does not depend on the values)
  const size_t slab = std::max((size_t)32 << 20, (pl->ext_hint + 4095) & ~(size_t)4095);
  char* ext = nullptr;
  HIPCHK(hipMalloc((void**)&ext, 5 * slab));
  HIPCHK(hipMemsetAsync(ext, 0, 5 * slab, s));
  RunArgs a;
  a.x = (const float*)ext;
  a.t = (const float*)(ext + slab);
  a.aux = (const float*)(ext + 2 * slab);
  a.out = (float*)(ext + 3 * slab);
  a.out2 = (float*)(ext + 4 * slab);
  const bool prof_was = c->prof_on;
  // per-op minimum over `nrep` in-plan runs of the whole plan (a first run warms up)
  auto time_ops = [&](int nrep) {
    std::vector<float> best(pl->ops.size(), 1e30f);
    for (int rep = 0; rep < nrep + 1; ++rep) {
      c->prof_on = true;
      c->prof_used = 0;
      c->prof_fam.clear();
      c->prof_op.clear();
      run_ops(c, pl, 0, pl->ops.size(), s, a);
      c->prof_on = false;
      HIPCHK(hipStreamSynchronize(s));
      if (rep == 0) continue;
      for (size_t i = 0; i < pl->ops.size(); ++i) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        best[i] = std::min(best[i], ms);
      }
    }
    return best;
  };
  // one in-plan pass over candidate ranks [0, nr): every GEMM class runs its r-th candidate, per-op minimum over `nrep` runs
  auto evaluate = [&](size_t nr, int nrep) {
    for (auto& kv : cands)
      for (auto& cd : kv.second) cd.situ_ms = 0.0;
    for (size_t r = 0; r < nr; ++r) {
      apply((int)r);
      const std::vector<float> best = time_ops(nrep);
      for (size_t i = 0; i < pl->ops.size(); ++i) {
        const Op& o = pl->ops[i];
        if (!o.is_gemm || o.c_ext) continue;
        std::vector<TuneCand>& v = cands[tune_key(o)];
        // a deferred split-K reduce is paid by the next op (the GroupNorm sums the slabs): judge the pair.  (round 5) Any consumer
        // that is not a GEMM itself (GroupNorm, attention: their time depends on nothing in this round but where this GEMM's tile
        // walk left their input -- which XCD's L2 holds it) is judged with its producer too.
        const bool pair = i + 1 < pl->ops.size() && (o.defer || !pl->ops[i + 1].is_gemm);
        if (r < v.size()) v[r].situ_ms += best[i] + (pair ? best[i + 1] : 0.f);
      }
    }
  };
  // stage 2a: every surviving candidate, coarse (2 runs); 2b: the four best of each class again, among good neighbours and
  // with 6 runs -- the final choice between near-equal candidates used to flip from run to run (227 .. 234 steps/s for the
  // same build and box), a second, finer round takes most of that variance out
  evaluate(rounds, 2);
  size_t keep = 0;
  for (auto& kv : cands) {
    std::vector<TuneCand>& v = kv.second;
    std::sort(v.begin(), v.end(), [](const TuneCand& x, const TuneCand& y) { return x.situ_ms < y.situ_ms; });
    if (v.size() > 4) v.resize(4);
    keep = std::max(keep, v.size());
  }
  evaluate(keep, 6);
  apply(-1);
  if (getenv("DF_TUNE_LOG") && atoi(getenv("DF_TUNE_LOG"))) {      // tools: the candidates of every GEMM class, both stages
    for (auto& kv : cands) {
      fprintf(stderr, "[df tune] %s:", kv.first.c_str());
      for (auto& cd : kv.second) fprintf(stderr, "  t%d/sk%d iso %.1f situ %.1f", cd.tile, cd.sk, cd.iso_ms * 1e3 / 3, cd.situ_ms * 1e3);
      fprintf(stderr, "\n");
    }
  }
  // stage 3: tile walk order of the chosen tile (GemmParams::gm), again timed inside the plan
  static const int gms[] = {0, 1, 2, 4, 8, 16};
  constexpr int NG = sizeof(gms) / sizeof(gms[0]);
  std::map<std::string, std::vector<double>> score;
  for (int r = 0; r < NG; ++r) {
    for (auto& o : pl->ops)
      if (o.is_gemm && !o.c_ext) o.gp.gm = gms[r];
    const std::vector<float> best = time_ops(3);
    for (size_t i = 0; i < pl->ops.size(); ++i) {
      const Op& o = pl->ops[i];
      if (!o.is_gemm || o.c_ext) continue;
      std::vector<double>& v = score[tune_key(o)];
      v.resize(NG, 0.0);
      v[r] += best[i] + ((i + 1 < pl->ops.size() && !pl->ops[i + 1].is_gemm) ? best[i + 1] : 0.f);
    }
  }
  for (auto& o : pl->ops) {
    if (!o.is_gemm || o.c_ext) continue;
    const std::vector<double>& v = score[tune_key(o)];
    int bi = 0;
    for (int k = 1; k < NG; ++k)
      if (v[k] < v[bi] * 0.99) bi = k;      // keep the default walk unless another is >1 % faster
    o.gp.gm = gms[bi];
  }
  c->prof_on = prof_was;
  c->prof_used = 0;
  c->prof_fam.clear();
  c->prof_op.clear();
  HIPCHK(hipStreamSynchronize(s));
  (void)hipFree(ext);
}

Plan* get_plan(df_ctx* c, const std::string& key, const std::function<void(Plan*)>& build) {
  auto it = c->plans.find(key);
  c->plan_tick[key] = ++c->tick;
  if (it != c->plans.end()) return it->second.get();
  if (!c->finalized) fail("df_finalize() has not been called");
  // Plans own their workspaces (up to a few GB for large batches): a service that sees many (batch, latent, context)
  // shapes must not grow without bound.  Beyond DF_MAX_PLANS (default 32) the least recently used plan is dropped.
  static const size_t max_plans = getenv("DF_MAX_PLANS") ? (size_t)std::max(2, atoi(getenv("DF_MAX_PLANS"))) : 32;
  while (c->plans.size() >= max_plans) {
    auto victim = c->plans.end();
    for (auto p = c->plans.begin(); p != c->plans.end(); ++p)
      if (p->second.get() != c->last_unet && (victim == c->plans.end() || c->plan_tick[p->first] < c->plan_tick[victim->first]))
        victim = p;
    if (victim == c->plans.end()) break;
    HIPCHK(hipDeviceSynchronize());               // the plan's buffers may still be read by queued launches
    c->plan_tick.erase(victim->first);
    c->plans.erase(victim);
  }
  std::unique_ptr<Plan> p(new Plan());
  build(p.get());
  if (c->autotune || g_tune_imported) {
    // tuning may try larger split-K factors than the cost model picked: give the scratch some head-room
    size_t want = 0;
    for (auto& o : p->ops)
      if (o.is_gemm && o.batch == 1) want = std::max(want, (size_t)32 * o.gp.M * o.gp.N * 4 * (o.gp.taps == 4 ? 4 : 1));
    if (want > ((size_t)512 << 20)) want = (size_t)512 << 20;
    if (want > p->partial_bytes) p->partial_bytes = want;
  }
  finish_plan(c, p.get());
  if (c->autotune) {
    autotune_plan(c, p.get(), c->pack_stream);
    HIPCHK(hipStreamSynchronize(c->pack_stream));
  } else if (g_tune_imported) {
    apply_tune_cache(p.get());
  }
  Plan* r = p.get();
  r->name = key;
  c->plans[key] = std::move(p);
  return r;
}

std::string keyf(const char* fmt, ...) {
  char buf[128];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
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

// Every entry point runs under one process-wide lock: contexts share the autotuner's choices, the launchers keep function-attribute
// high-water marks in statics, and a plan build is not re-entrant.  The calls only enqueue work, so the lock is held for microseconds;
// what it buys is that two host threads may drive two models (or one) without corrupting any of that.  Recursive: test hooks nest.
static std::recursive_mutex g_api_lock;

template <class F>
int guard(F&& f) {
  std::lock_guard<std::recursive_mutex> hold(g_api_lock);
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  }
}

}  // namespace

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
int df_config_vae(df_ctx* c, const df_vae_config* cfg) { return guard([&] { c->vcfg = *cfg; c->has_vae = true; }); }
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

int df_autotune(df_ctx* c, int enable) { return guard([&] { c->autotune = enable != 0; }); }

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
    HIPCHK(launch_mel_to_stft(mel, B, n_mels, T, A, At, Pt, inv_L, iters, S, (hipStream_t)stream));
  });
}
int df_griffinlim(const float* S, const float* phase0, int B, int T, int n_iter, float momentum, const float* twiddles,
                  const float* window, const float* wss, float* angles, float* reb0, float* reb1, float* frames, float* wav,
                  void* stream) {
  return guard([&] {
    need_positive("griffinlim", {{"clips", B}, {"frames", T}});
    HIPCHK(launch_griffinlim(S, phase0, B, T, n_iter, momentum, (const float2*)twiddles, window, wss, (float2*)angles,
                             (float2*)reb0, (float2*)reb1, frames, wav, (hipStream_t)stream));
  });
}

int df_cfg_combine(const float* e2, float* e, int64_t n, float scale, void* stream) {
  return guard([&] { HIPCHK(launch_cfg_combine(e2, e, (long)n, scale, (hipStream_t)stream)); });
}
int df_lincomb(float* out, const float* const* in, const float* coef, int nterms, int64_t n, void* stream) {
  return guard([&] { HIPCHK(launch_lincomb(out, in, coef, nterms, (long)n, (hipStream_t)stream)); });
}
int df_q_sample_blend(const float* img, const float* x0, const float* noise, const float* mask, float* out, int64_t n, int64_t chw,
                      int64_t hw, int mask_c, float sqrt_acp, float sqrt_one_minus_acp, void* stream) {
  return guard([&] {
    HIPCHK(launch_q_sample_blend(img, x0, noise, mask, out, (long)n, (long)chw, (long)hw, mask_c, sqrt_acp, sqrt_one_minus_acp,
                                 (hipStream_t)stream));
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

int df_test_gemm(const uint16_t* A, const uint16_t* W, float* C, int M, int N, int K, int tile, int splitk, void* stream) {
  return guard([&] {
    GemmParams g = Builder::gp_linear(A, M, K, W, N);
    Builder::out_f32(g, C, N);
    g.dbg = getenv("DF_GEMM_DBG") ? atoi(getenv("DF_GEMM_DBG")) : 0;
    g.splitk = splitk;
    if (splitk > 1) g.partial = test_partial((size_t)splitk * M * N * 4);
    else if (g.dbg & 64) g.partial = test_partial((size_t)4096 * 32 * 8);      // per-block clock stamps (tools/gemm_stamps.py)
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
  });
}

// The GEMM with its simple epilogue features switched on: bias, residual, activation (1 = SiLU, 2 = ReLU), fp32 or
// operand-type output, with and without split-K -- every tile must give the same answer for every combination.
int df_test_gemm_epi(const uint16_t* A, const uint16_t* W, const float* bias, const float* res, void* C, int M, int N, int K,
                     int act, int out_operand, int tile, int splitk, void* stream) {
  return guard([&] {
    GemmParams g = Builder::gp_linear(A, M, K, W, N);
    if (out_operand) Builder::out_b16(g, (bf16_t*)C, N);
    else Builder::out_f32(g, (float*)C, N);
    g.bias = bias;
    if (res) { g.res = res; g.ldr = N; }
    g.silu = act == 1;
    g.relu = act == 2;
    g.splitk = splitk;
    if (splitk > 1) g.partial = test_partial((size_t)splitk * M * N * 4);
    if (!gemm_tile_valid(g, tile, 1, splitk)) fail("tile %d / split-K %d refused this problem", tile, splitk);
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
  });
}

// C = [A | A2] W^T with the K columns split over two operand tensors (the merged FF2 + proj_out GEMM of the SpatialTransformer).
int df_test_gemm_dual(const uint16_t* A, const uint16_t* A2, const uint16_t* W, float* C, int M, int N, int K1, int K2, int tile,
                      int splitk, void* stream) {
  return guard([&] {
    GemmParams g = Builder::gp_linear(A, M, K1, W, N);
    g.K = K1 + K2;
    g.w_bytes = Builder::op_bytes((size_t)N * (K1 + K2) * 2);
    g.A2 = A2; g.lda2 = K2; g.Cin2 = K2; g.a2_bytes = Builder::op_bytes((size_t)M * K2 * 2);
    Builder::out_f32(g, C, N);
    g.splitk = splitk;
    if (splitk > 1) g.partial = test_partial((size_t)splitk * M * N * 4);
    if (!gemm_tile_valid(g, tile, 1, splitk)) fail("tile %d / split-K %d refused this problem", tile, splitk);
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
  });
}

// Every GemmParams epilogue feature on a caller-chosen (tile, split-K, batch, gm): tests/test_gemm_epilogues_gpu.py walks the
// autotuner's whole search space with it.
static void test_gemm_params(const df_test_gemm_desc* d, GemmParams& g) {
  if (!d) fail("df_test_gemm: null descriptor");
  if (d->size != (int64_t)sizeof(df_test_gemm_desc))
    fail("df_test_gemm: descriptor of %lld bytes, this build expects %zu (stale binding of df_test_gemm_desc?)", (long long)d->size,
         sizeof(df_test_gemm_desc));
  const bf16_t* A = (const bf16_t*)d->A;
  const bf16_t* W = (const bf16_t*)d->W;
  if (d->conv) {
    if (d->stride != 1 && d->stride != 2) fail("df_test_gemm: conv stride %d", d->stride);
    g = Builder::gp_conv3(A, d->NB, d->H, d->Wd, d->Cin, W, d->N, d->stride, 0);
  } else {
    g = Builder::gp_linear(A, d->M, d->K, W, d->N);
    if (d->lda > 0) {
      g.lda = d->lda;
      g.a_bytes = Builder::op_bytes((size_t)d->M * d->lda * 2);
    }
  }
  g.C = d->C; g.ldc = d->ldc > 0 ? d->ldc : g.N; g.out_bf16 = d->out_operand ? 1 : 0;
  g.a_bs = d->a_bs; g.w_bs = d->w_bs; g.c_bs = d->c_bs; g.res_bs = d->res_bs;
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
}

int df_test_gemm_valid(const df_test_gemm_desc* d, int tile, int batch, int splitk) {
  std::lock_guard<std::recursive_mutex> hold(g_api_lock);
  try {
    GemmParams g;
    test_gemm_params(d, g);
    return gemm_tile_valid(g, tile, batch, splitk) ? 1 : 0;
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

int df_test_gemm_ex(const df_test_gemm_desc* d, void* stream) {
  return guard([&] {
    GemmParams g;
    test_gemm_params(d, g);
    const int batch = d->batch > 1 ? d->batch : 1;
    if (g.K % 64 != 0) fail("df_test_gemm: K %d is not a multiple of 64", g.K);
    if (d->defer_reduce && g.splitk < 2) fail("df_test_gemm: defer_reduce needs split-K");
    const size_t slab_bytes = (size_t)g.splitk * g.M * g.N * 4;
    if (g.splitk > 1) g.partial = test_partial(slab_bytes);
    const hipError_t e = launch_gemm(g, d->tile, batch, (hipStream_t)stream);
    if (e == hipErrorInvalidValue)
      fail("launch_gemm refused tile %d / split-K %d / batch %d (%dx%dx%d)", d->tile, g.splitk, batch, g.M, g.N, g.K);
    HIPCHK(e);
    if (d->defer_reduce && d->slabs_out)
      HIPCHK(hipMemcpyAsync(d->slabs_out, g.partial, slab_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
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
    auto run = [&](const GemmParams& g, int tile, int batch, const char* what) {
      if (!gemm_tile_valid(g, tile, batch, 1)) fail("xattn chain: tile %d refused %s", tile, what);
      HIPCHK(launch_gemm(g, tile, batch, s));
    };
    {
      GemmParams g = Builder::gp_linear(ctx, NB * Tc, Dc, Wkv, 2 * C);
      Builder::out_b16(g, kv, 2 * C);
      run(g, TILE_64x64, 1, "ctx.kv");
    }
    HIPCHK(launch_xattn_expand(kv, Kexp, Vexp, NB, Tc, 32, C, heads, s));
    HIPCHK(launch_pack_lnq_t(Wq, gamma, WqT, C, scale, s));
    {
      GemmParams g = Builder::gp_linear(Kexp, NB * HT, C, WqT, C);
      Builder::out_b16(g, G, C);
      run(g, TILE_64x64, 1, "ctx.g");
    }
    HIPCHK(launch_xattn_rowstats(G, Kexp, bq, scale, C, (long)NB * HT, cs, bb, s));
    {
      GemmParams g = Builder::gp_linear(Wo, C, C, Vexp, HT);
      g.w_bs = (long)HT * C;
      Builder::out_b16(g, Vo, HT);
      g.c_bs = (long)C * HT;
      run(g, TILE_64x64, NB, "ctx.vo");
    }
    {
      GemmParams g = Builder::gp_linear(xb, M, C, G, HT);
      g.w_bs = (long)HT * C; g.w_rows = T;
      Builder::out_b16(g, P, HT);
      g.ln_stats = (const float2*)xstats; g.ln_slots = C / 64; g.ln_C = C; g.ln_eps = 1e-5f; g.ln_cs = cs;
      g.bias = bb;
      g.sm_w = 32; g.sm_valid = Tc;
      run(g, tile_xs, 1, "st.xs");
    }
    {
      GemmParams g = Builder::gp_linear(P, M, HT, Vo, C);
      g.w_bs = (long)C * HT; g.w_rows = T;
      Builder::out_f32(g, out, C);
      g.bias = bo;
      g.res = x; g.ldr = C;
      run(g, tile_xo, 1, "st.xo");
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
      if (!gemm_tile_valid(g, tile0, 1, sk0)) fail("producer: tile %d / split-K %d not valid here", tile0, sk0);
      HIPCHK(launch_gemm(g, tile0, 1, s));
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
      if (!gemm_tile_valid(g, tile1, 1, sk1)) fail("consumer: tile %d / split-K %d not valid here", tile1, sk1);
      HIPCHK(launch_gemm(g, tile1, 1, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (void* p : {(void*)xb, (void*)st, (void*)w1p, (void*)cs, (void*)bb}) (void)hipFree(p);
  });
}

// The LayerNorm-folded GEGLU projection alone, on caller-owned operands (timing probes: tools/pgeglu_probe.py).  stats [M][K/64]
// float2, cs / bias [N1]; dbg = debug switches of the persistent kernel (ffn.hip) or DF_GEMM_DBG of the generic one.
int df_test_geglu(const uint16_t* A, const uint16_t* W, const void* stats, const float* cs, const float* bias, uint16_t* out, int M,
                  int K, int N1, int tile, int dbg, void* stream) {
  return guard([&] {
    GemmParams g = Builder::gp_linear(A, M, K, W, N1);
    g.ln_stats = (const float2*)stats; g.ln_slots = K / 64; g.ln_C = K; g.ln_eps = 1e-5f; g.ln_cs = cs;
    g.bias = bias;
    Builder::out_b16(g, out, N1 / 2);
    g.geglu = 1;
    g.splitk = 1;
    g.dbg = dbg;
    if (dbg & 64) g.partial = test_partial((size_t)1024 * 32 * 8);     // per-block clock stamps (read back with df_test_scratch_read)
    if (gemm_tile_is_wgeglu(tile)) {      // the wide tiles read the 320-column packing: permuted here, per call (test entry)
      if (N1 % 320 != 0) fail("tile %d: N = %d is not a multiple of 320", tile, N1);
      static void* buf = nullptr;
      static size_t cap = 0;
      const size_t need = (size_t)N1 * K * 2 + (size_t)N1 * 8 + 512;
      if (need > cap) {
        if (buf) HIPCHK(hipFree(buf));
        HIPCHK(hipMalloc(&buf, need));
        cap = need;
      }
      uint16_t* w3 = (uint16_t*)buf;
      float* cs3 = (float*)((char*)buf + (((size_t)N1 * K * 2 + 255) & ~(size_t)255));
      float* bb3 = cs3 + N1;
      static const void* packed_from = nullptr;
      if (!(dbg & 128) || packed_from != (const void*)W)      // dbg bit 7 (timing tools): keep the packing made from this W by the last call
        HIPCHK(launch_pack_w320(W, cs, bias, w3, cs3, bb3, N1, K, (hipStream_t)stream));
      packed_from = (const void*)W;
      g.dbg = dbg & ~128;
      g.W_w320 = w3; g.cs_w320 = cs3; g.bias_w320 = bb3;
    }
    if (!gemm_tile_valid(g, tile, 1, 1)) fail("tile %d not valid for this GEGLU projection", tile);
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
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

int df_test_conv3x3(const uint16_t* A, const uint16_t* W, const float* bias, float* C, int NB, int H, int Wd, int Cin,
                    int Cout, int stride, int ups, int tile, int splitk, void* stream) {
  return guard([&] {
    GemmParams g = Builder::gp_conv3(A, NB, H, Wd, Cin, W, Cout, stride, ups);
    Builder::out_f32(g, C, Cout);
    g.bias = bias;
    g.splitk = splitk;
    g.dbg = getenv("DF_GEMM_DBG") ? atoi(getenv("DF_GEMM_DBG")) : 0;
    if (splitk > 1) g.partial = test_partial((size_t)splitk * g.M * g.N * 4);
    else if (g.dbg & 64) g.partial = test_partial((size_t)4096 * 32 * 8);      // halo kernels: per-block clock stamps
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
  });
}

int df_test_conv3x3_fewout(const uint16_t* A, const uint16_t* W, const float* bias, float* out_nchw, int NB, int H, int Wd, int Cin,
                           int Cout, void* stream) {
  return guard([&] { HIPCHK(launch_conv3x3_fewout(A, W, bias, out_nchw, NB, H, Wd, Cin, Cout, (hipStream_t)stream)); });
}

int df_test_conv3x3_skip(const uint16_t* A, const uint16_t* A2, const uint16_t* W, const float* bias, float* C, int NB, int H,
                         int Wd, int Cin, int Cin2, int Cout, int tile, int splitk, void* stream) {
  return guard([&] {
    GemmParams g = Builder::gp_conv3(A, NB, H, Wd, Cin, W, Cout, 1, 0);
    Builder::out_f32(g, C, Cout);
    g.bias = bias;
    g.A2 = A2; g.lda2 = Cin2; g.Cin2 = Cin2; g.a2_bytes = Builder::op_bytes((size_t)g.M * Cin2 * 2);
    g.K = 9 * Cin + Cin2;
    g.w_bytes = Builder::op_bytes((size_t)Cout * g.K * 2);
    g.splitk = splitk;
    if (splitk > 1) g.partial = test_partial((size_t)splitk * g.M * g.N * 4);
    if (!gemm_tile_valid(g, tile, 1, splitk)) fail("tile %d / split-K %d refused this problem", tile, splitk);
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
  });
}

// Upsample + conv3x3 through the phase-decomposed form (gemm_m3.hip): W_oihw fp32 [Cout][Cin][3][3] is packed here.
int df_test_conv3x3_ups4(const uint16_t* A, const float* W_oihw, const float* bias, float* C, uint16_t* w4_scratch, int NB, int H,
                         int Wd, int Cin, int Cout, int tile, int splitk, void* stream) {
  return guard([&] {
    HIPCHK(launch_pack_conv_ups4(W_oihw, w4_scratch, Cout, Cin, Cin, (hipStream_t)stream));
    GemmParams g = Builder::gp_conv3_ups4(A, NB, H, Wd, Cin, w4_scratch, Cout);
    Builder::out_f32(g, C, Cout);
    g.bias = bias;
    g.splitk = splitk;
    if (splitk > 1) g.partial = test_partial((size_t)splitk * 4 * g.M * g.N * 4);
    if (!gemm_tile_valid(g, tile, 1, splitk)) fail("tile %d / split-K %d refused this problem", tile, splitk);
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
  });
}

int df_test_groupnorm(const float* x, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps,
                      int silu, uint16_t* out, void* stream) {
  return guard([&] {
    const size_t sb = groupnorm_scratch_bytes(N, HW, C);
    if (sb) {
      float* scr = test_partial(sb);
      HIPCHK(launch_groupnorm_chunked(x, ld, N, HW, C, gamma, beta, eps, silu, out, C, nullptr, scr, (hipStream_t)stream));
    } else {
      HIPCHK(launch_groupnorm(x, ld, N, HW, C, gamma, beta, eps, silu, out, C, nullptr, (hipStream_t)stream));
    }
  });
}
int df_test_groupnorm_own_slabs(float* x, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps, int silu,
                                uint16_t* out, const float* slabs, int nslab, int c_own, const float* bias, const float* res,
                                int ldr, void* stream) {
  return guard([&] {
    if (!groupnorm_accepts_slabs(HW, C)) fail("groupnorm: %d x %d slab does not fit the register kernel", HW, C);
    HIPCHK(launch_groupnorm_own_slabs(x, ld, N, HW, C, gamma, beta, eps, silu, out, C, nullptr, slabs, nslab,
                                      (long)N * HW * c_own, c_own, bias, res, ldr, (hipStream_t)stream));
  });
}
int df_test_layernorm(const float* x, int rows, int C, const float* gamma, const float* beta, uint16_t* out, void* stream) {
  return guard([&] { HIPCHK(launch_layernorm(x, C, rows, C, gamma, beta, 1e-5f, out, (hipStream_t)stream)); });
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
    if (!gemm_tile_valid(g, tile, 1, splitk)) fail("tile %d / split-K %d refused this problem", tile, splitk);
    HIPCHK(launch_gemm(g, tile, 1, (hipStream_t)stream));
  });
}

}  // extern "C"

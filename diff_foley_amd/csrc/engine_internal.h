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
//
// This header is what the engine's translation units share: the plan types, the context with its weight packers, the plan
// Builder, and the prototypes of every function one unit calls in another.  Who defines what:
//   engine_pack.hip      df_ctx packers
//   engine_builder.hip   choose_tile, Builder members
//   engine_nets.hip      UNet topology, build_emb_table, build_unet_like, build_vae, build_vae_encoder, build_cond, build_cavp,
//                        build_cavp_spec
//   engine_cls_grad.hip  build_classifier_grad
//   engine_run.hip       finish_plan, run_ops (+ debug hooks), get_plan, keyf
//   engine_tune.hip      tune cache, apply_tune_cache, autotune_plan
//   engine_test_api.hip  df_test_* entry points
//   engine (this name)   product C ABI with the packed-blob layout / export / import, g_err, g_api_lock
// Everything in namespace dfe is hidden from the dynamic symbol table (DFE_NAMESPACE below); what one unit alone uses stays
// static in that unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
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

// Every unit opens namespace dfe through this macro.  The attribute hides what is DEFINED inside the block it is written on: a
// definition in a plain `namespace dfe {` block is exported unless another unit happens to reference it through this header.
#define DFE_NAMESPACE namespace dfe __attribute__((visibility("hidden")))

DFE_NAMESPACE {

extern thread_local std::string g_err;      // last error of this thread (df_last_error); defined with the C ABI

[[noreturn]] inline void fail(const char* fmt, ...) {
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
    if (e_ != hipSuccess) dfe::fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
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
  std::vector<Block> pinned;     // alloc_zeroed / alloc_index blocks: never recycled, never poisoned (freed with the plan)
  // debug (df_debug_poison): fresh blocks are filled with 0xFF bytes (NaN as fp32 / bf16 / fp16) instead of zeros, and every
  // release is recorded as (ops.size() when it took effect, block): run_ops fills the block again right behind the op in front of
  // that index.  An op that reads what no earlier op of the same run wrote -- build-time zeros, a previous tenant's bytes, its own
  // buffer after the release -- then reads NaN.
  bool poison = false;
  std::vector<std::pair<size_t, Block>> poison_at;      // sorted by op index in finish_plan
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
  // The builder fixed every GEMM's tile and split-K as a function of the PER-SAMPLE problem (Builder::choice_NB): neither the tune
  // table nor the autotuner may replace them (their entries are keyed by the row count, i.e. by the batch) -- VAE encoder plans,
  // whose results must not depend on what else is in the batch
  bool fixed_choices = false;
  std::string name;              // cache key (debug labels)
  void* chk_list = nullptr;      // debug checksums: device array of (pointer, 32-bit words) of every workspace block
  int chk_n = 0;
  ~Plan() {
    for (auto& b : owned) (void)hipFree(b.p);
    for (auto& b : pinned) (void)hipFree(b.p);
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
    HIPCHK(hipMemset(p, poison ? 0xFF : 0, bytes));
    owned.push_back({p, bytes});
    return p;
  }
  // A block of zeros that stays what it is: zeroed here, never on the freelist (release() does not know it), never poisoned.  For
  // regions an op reads but no op ever writes -- the pad columns behind the columns a GEMM stores.  The ops that write INTO such a
  // block write the same elements in every run, so the zeros around them are the build's in every run.
  void* alloc_zeroed(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    HIPCHK(hipMemset(p, 0, bytes));
    pinned.push_back({p, bytes});
    return p;
  }
  // A block whose content is read as an integer, an index or a pointer: pinned and zeroed like alloc_zeroed, and named apart so that
  // the poison pattern can never become an address (no plan builder needs one today)
  void* alloc_index(size_t bytes) { return alloc_zeroed(bytes); }
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
        if (poison) poison_at.push_back({ops.size(), b});
        return;
      }
  }
};

struct F32 {  // fp32 NHWC activation view
  float* p = nullptr;
  int rows = 0, C = 0, ld = 0;
  uint16_t* b16 = nullptr;      // operand-type copy [rows][C] written by the op that produced the tensor (classifier-gradient tape), or null
};

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int rup(int a, int b) { return cdiv(a, b) * b; }

}  // namespace dfe

// (hidden like namespace dfe: the C ABI passes df_ctx* as an opaque handle, its members are the engine's own)
struct __attribute__((visibility("hidden"))) df_ctx {
  int device = 0;
  std::map<std::string, dfe::RawT> raw;
  std::map<std::string, void*> packed;
  std::vector<void*> packed_blocks;
  bool has_unet = false, has_vae = false, has_cond = false, has_cls = false, has_cavp = false, has_vae_enc = false, has_cavp_spec = false,
       finalized = false;
  bool has_vae_shape = false;       // vcfg is set: by df_config_vae (has_vae: the decoder runs) or by df_config_vae_encoder_only (it does not)
  df_cavp_config pcfg{};
  df_cavp_spec_config scfg{};
  df_unet_config ucfg{}, ccfg{};
  df_vae_config vcfg{};
  df_vae_encoder_config ecfg{};
  df_cond_config kcfg{};
  std::map<std::string, int> emb_off[2];   // resblock prefix -> column offset in the fused emb projection
  int emb_total[2] = {0, 0};
  std::map<std::string, std::unique_ptr<dfe::Plan>> plans;
  std::map<std::string, uint64_t> plan_tick;     // last use of every plan (least-recently-used eviction, DF_MAX_PLANS)
  uint64_t tick = 0;
  dfe::Plan* last_unet = nullptr;
  bool last_unet_hoisted = false;   // the last UNet run looked its time embedding up (df_unet_forward*_ts)
  int ctx_N = 0, ctx_T = 0;
  float* ctx_copy = nullptr;
  size_t ctx_copy_bytes = 0;
  bool autotune = false;
  bool poison_on = false;         // df_debug_poison: plans are built with Plan::poison (switching it drops the cached plans)
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

  const dfe::RawT& rt(const std::string& name) const {
    auto it = raw.find(name);
    if (it == raw.end()) dfe::fail("missing tensor '%s'", name.c_str());
    return it->second;
  }
  bool has(const std::string& name) const { return raw.count(name) != 0; }
  const float* f32(const std::string& name) const {
    const dfe::RawT& t = rt(name);
    if (!t.d) dfe::fail("tensor '%s' was imported shape-only (df_import_packed): its fp32 data is not on this rank", name.c_str());
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
  // The frame of every packer below.  The blocks stored under `keys` are looked up in `packed` (the blocks of one packer are made
  // together, so the first key decides); on a miss make() sizes them with pmalloc, fills them on pack_stream and returns them, and
  // they are stored under their keys.
  template <size_t N, class Make>
  std::array<void*, N> pack_once(const std::array<std::string, N>& keys, Make&& make) {
    if (!packed.count(keys[0])) {
      const std::array<void*, N> made = make();
      for (size_t i = 0; i < N; ++i) packed[keys[i]] = made[i];
    }
    std::array<void*, N> blk;
    for (size_t i = 0; i < N; ++i) blk[i] = packed[keys[i]];
    return blk;
  }
  template <class Make>
  void* pack_once(const std::string& key, Make&& make) {      // one block
    return pack_once<1>({key}, [&]() -> std::array<void*, 1> { return {make()}; })[0];
  }
  // Linear / 1x1-conv weight [O][I] -> bf16
  const bf16_t* w_linear(const std::string& name);
  // rows of several [O_i][I] matrices stacked -> bf16 [sum O_i][I]
  const bf16_t* w_stack(const std::string& key, const std::vector<std::string>& names);
  const float* b_stack(const std::string& key, const std::vector<std::string>& names);
  // 3x3 conv weight OIHW -> bf16 [O][3][3][Ipad]
  const bf16_t* w_conv3(const std::string& name, int ipad);
  // 3x3 conv weight that follows a nearest-x2 Upsample: per-phase 2x2-tap weights [4][O][4][Ipad] (gemm_m3.hip)
  const bf16_t* w_conv3_ups4(const std::string& name, int ipad);
  // conv2 + folded 1x1 skip connection: operand [O][9*I + I2] and the summed bias
  void w_conv3_skip(const std::string& conv, const std::string& skip, const bf16_t** w, const float** b);
  // FeedForward's second Linear merged with the SpatialTransformer's proj_out (1x1 conv): operand [C][4C + C], summed bias
  void w_ffproj(const std::string& ff2, const std::string& po, const bf16_t** w, const float** b);
  // scale * gamma[c] * Wq[j][c] as operand [c][j]: the LayerNorm-folded cross-attention query projection, transposed
  const bf16_t* w_lnq_t(const std::string& wq, const std::string& norm, float scale);
  // Linear weights [O_j][I] stacked along O and transposed -> bf16 [I][sum O_j]  (backward-data operand)
  const bf16_t* w_stack_t(const std::string& key, const std::vector<std::string>& names);
  // 3x3 conv weight OIHW -> backward-data packing bf16 [I][ky'][kx'][Opad] (flipped taps).  Opad = Cout rounded up to the 64-channel
  // K step with zero rows behind the real ones: the gradient operand of such a conv carries Opad columns, the pad ones zero (the
  // classifier head's conv halves the channels: 64 -> 32, 320 -> 160; every other conv on the tape has Cout % 64 == 0)
  const bf16_t* w_conv3_bwd(const std::string& name);
  // Conv3d + eval BatchNorm3d of an mmcv ConvModule `p` (keys p.conv.weight, p.bn.*): operand [O][kp] with the BN scale
  // folded in (k = tap*I + i, zero padded to kp) and the fp32 bias beta - mean*scale.
  void w_conv3d_bn(const std::string& p, int kp, const bf16_t** w, const float** b);
  // Conv2d 3x3 (no bias) `conv`.weight + eval BatchNorm2d `bn`.* of a Cnn14 ConvBlock: the same fold, operand [O][9 I] (k = tap*I + i)
  void w_conv2d_bn(const std::string& conv, const std::string& bn, int kp, const bf16_t** w, const float** b);
  // LayerNorm `norm` folded into the Linear(s) `names` stacked along the output dim (biases[i] may be empty):
  // operand rows gamma*W, their column sums and the folded bias beta.W + b.  geglu: ONE matrix, rows GEGLU-interleaved.
  void w_ln_stack(const std::string& key, const std::string& norm, const std::vector<std::string>& names,
                  const std::vector<std::string>& biases, bool geglu, const bf16_t** w, const float** cs, const float** bb);
  // The LayerNorm-folded GEGLU projection `key` (w_ln_stack with geglu = true: rows in (32 x | 32 gate) groups) once more in the
  // 320-column packing of the wide tiles (ffn_wide.hip): a device-side row permutation of the packed operand -- needs no fp32
  // data, so a rank that imported the packed blob builds it the same way.
  void w_ln_w320(const std::string& key, int rows, int K, const bf16_t** w, const float** cs, const float** bb);
  void w_geglu(const std::string& prefix, const bf16_t** w, const float** b);
};

DFE_NAMESPACE {

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

UNetTopo make_topo(const df_unet_config& u, bool encoder_only);
std::vector<std::string> topo_resblocks(const UNetTopo& t);
std::vector<BlockDesc> topo_sts(const UNetTopo& t);

struct Builder {
  df_ctx* c;
  Plan* pl;
  std::string pre;     // state_dict prefix of the module being built
  int which = 0;       // 0 = unet, 1 = classifier (emb offset table)

  std::string nm(const std::string& s) const { return pre + s; }

  struct PX {    // cross-attention operands precomputed from the context (context_px, engine_builder.hip)
    const bf16_t* G = nullptr;    // [NB][H*32][C]   operand of the score GEMM (rows = (head, context token))
    const float* cs = nullptr;    // [NB][H*32]      column sums of G (LayerNorm fold)
    const float* bb = nullptr;    // [NB][H*32]      beta . G
    const bf16_t* Vo = nullptr;   // [NB][C][H*32]   operand of the output GEMM
    int HT = 0;                   // H * 32
  };

  // A consumer that needs the operand-type copy of a block's fp32 output (Downsample / Upsample convs) sets
  // want_aux before the block is built; the block's last GEMM then writes the copy from its epilogue (no cast pass)
  // and leaves the buffer in last_aux.
  bool want_aux = false;
  bf16_t* last_aux = nullptr;
  // > 0: the plan's batch size.  gemm() then chooses tile and split-K for kChoiceBatch samples of the problem whatever the batch is, so
  // every sample's fp32 summation order -- and with it every bit of its result -- is the same in any batch (Plan::fixed_choices).
  int choice_NB = 0;
  static constexpr int kChoiceBatch = 4;
  void attach_aux(GemmParams& g, int rows, int C);

  template <class T>
  T* buf(size_t n) {
    return (T*)pl->alloc(n * sizeof(T));
  }

  // The last emitted op, when it is a GEMM whose fp32 output could be left as split-K slabs for a GroupNorm that follows
  // IMMEDIATELY (groupnorm() below claims it; any other emission forgets it).
  struct Pend { long op = -1; const float* p = nullptr; int ld = 0, C = 0, rows = 0; };
  Pend pend;

  void forget_pend();
  void other(const char* tag, std::function<hipError_t(hipStream_t, const RunArgs&)> fn);
  // operand-type output of the op emitted last (counted by df_debug_saturations)
  void emits(const bf16_t* p, long rows, int cols, int ld);
  Op& gemm(GemmParams gp, int batch, const char* tag);

  // operands are addressed through 32-bit buffer offsets: one operand of one GEMM must stay below 2 GiB
  static unsigned op_bytes(size_t b);
  static GemmParams gp_linear(const bf16_t* A, int M, int K, const bf16_t* W, int N);
  static GemmParams gp_conv3(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W, int Cout, int stride,
                             int ups);
  // the VAE encoder's Downsample (stage1_autoencoder/model.py:167-171): F.pad(x, (0,1,0,1)) + stride-2 conv with padding 0 =
  // gp_conv3(..., stride 2) with GemmParams::pad = 0 (H and Wd even)
  static GemmParams gp_conv3_down_asym(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W, int Cout);
  // nearest-x2 upsample + conv3x3 as four 2x2-tap convs (one per output phase) over the INPUT-resolution map: rows = input
  // pixels, K = 4 Cin, one weight matrix per phase (w_bs), output rows = the x2 map (the kernel scatters by phase)
  static GemmParams gp_conv3_ups4(const bf16_t* A, int NB, int H, int Wd, int Cin, const bf16_t* W4, int Cout);
  // a second operand tensor A2 [M][lda2] for Cin2 more K columns behind g's own (the folded 1x1 skip of a conv, the residual-stream
  // half of st.ffproj): K grows by Cin2, and W -- [N][K] over the whole K -- is sized again
  static void add_a2(GemmParams& g, const bf16_t* A2, int lda2, int Cin2);
  static void out_f32(GemmParams& g, float* C, int ldc) { g.C = C; g.ldc = ldc; g.out_bf16 = 0; }
  static void out_b16(GemmParams& g, bf16_t* C, int ldc) { g.C = C; g.ldc = ldc; g.out_bf16 = 1; }

  // Both norms of a plan go through emit_groupnorm (engine_builder.hip).  A split-K producer at ops[prod] hands its reduce to the norm
  // in one of two ways: input_slabs -- the norm sums the slabs of its INPUT (a ResBlock's conv1 -> second norm; + bias + FiLM row
  // bias); own_slabs -- the norm finishes the slabs of the tensor it normalises and writes it back (the claimed `pend` GEMM).
  enum class GnFeed { none, input_slabs, own_slabs };
  void emit_groupnorm(GroupNormArgs a, GnFeed feed, size_t prod, const float* rowbias, int ld_rowbias);
  // GroupNorm(+SiLU) -> bf16 operand (and optionally the raw bf16 cast)
  bf16_t* groupnorm(const F32& x, int NB, const std::string& p, float eps, int silu, bf16_t** raw);
  void layernorm(const F32& x, const std::string& p, bf16_t* o);
  bf16_t* cast2d(const F32& x);

  // ResBlock (openai_unetmodel.py:255-275) / VAE ResnetBlock (model.py:216-236, no emb).  `out` may be a slot of a
  // concat buffer.  Names differ between the two families, so they are passed in.
  void resblock(const F32& x, const F32& out, int NB, int H, int Wd, const std::string& n1, const std::string& c1,
                const std::string& n2, const std::string& c2, const std::string& skip, float eps,
                const float* emb, int emb_ld, int emb_col, int dup_rows = 0);

  // SpatialTransformer (attention_openai.py:250-261) with one BasicTransformerBlock (:211-215).
  // ctxK [NB*Tc][C] bf16 and ctxVt [NB][C][ldvt] bf16 are the hoisted cross-attention K / V^T.
  // cfg_prefix: the block is the first SpatialTransformer of a classifier-free-guidance batch [x ; x] -- its GroupNorm, proj_in,
  // Q|K|V projection, self-attention and out-projection see identical rows in both halves (no context yet), so they run on the
  // first half only and attn1.out stores every row for both halves (GemmParams::dup_rows); from the cross-attention on, full batch.
  void spatial_transformer(const F32& x, const F32& out, int NB, int T, const std::string& p, int heads,
                           const bf16_t* ctxK, const bf16_t* ctxVt, int Tc, int ldvtc, const PX* px = nullptr,
                           bool cfg_prefix = false);

  static bool px_ok(int C, int heads, int Tc, int tokens);
  PX context_px(const bf16_t* ctx, int NB, int Tc, int Dc, const std::string& st_prefix, int C, int heads);
  void context_kv(const bf16_t* ctx, int NB, int Tc, int Dc, const std::string& st_prefix, int C, bf16_t** K,
                  bf16_t** Vt, int ldvt);

  // ---- what the two UNet-shaped builders (build_unet_like, build_classifier_grad) spell the same way
  typedef std::map<std::string, std::pair<bf16_t*, bf16_t*>> KV;      // SpatialTransformer prefix -> context K, V^T
  bf16_t* context_cast(int N, int Tc, int Dc);
  void context_kv_for(const bf16_t* ctx, int NB, int Tc, int Dc, const BlockDesc& d, int ldvt, KV& kv);
  void emb_proj_operands(const UNetTopo& topo, const bf16_t** w, const float** bb);
  static int checked_in_channels(const df_unet_config& u);
};

// ---- plan builders (engine_nets.hip, engine_cls_grad.hip)
void build_emb_table(df_ctx* c, int which);
void build_unet_like(df_ctx* c, Plan* pl, int which, int N, int H, int W, int Tc, bool cfg_mode);
void build_classifier_grad(df_ctx* c, Plan* pl, int N, int H, int W, int Tc);
void build_vae(df_ctx* c, Plan* pl, int B, int H, int W);
// tap >= 0 (df_test_vae_encode_tap): one stage's fp32 output is also copied to RunArgs.out2 -- 0 conv_in, 1 + l Downsample l, 100 mid
void build_vae_encoder(df_ctx* c, Plan* pl, int B, int H, int W, int tap = -1);
// every state_dict key the encoder plan reads (df_finalize requires them once the encoder is configured)
std::vector<std::string> vae_encoder_tensor_names(const df_ctx* c);
void build_cond(df_ctx* c, Plan* pl, int B, int T);
void build_cavp(df_ctx* c, Plan* pl, int T, int H, int W);
// CAVP spectrogram encoder (Cnn14) over B clips of T frames x n_mels; tap 1 .. 6 (df_test_cavp_spec_tap): that ConvBlock's output is also
// copied to RunArgs.out2 as the plan holds it (operand type behind the pools of blocks 1 .. 5, fp32 for block 6)
void build_cavp_spec(df_ctx* c, Plan* pl, int B, int T, int n_mels, int tap = -1);

// ---- plan execution and the plan cache (engine_run.hip)
void finish_plan(df_ctx* c, Plan* pl);
void run_ops(df_ctx* c, Plan* pl, size_t begin, size_t end, hipStream_t s, const RunArgs& a);
Plan* get_plan(df_ctx* c, const std::string& key, const std::function<void(Plan*)>& build);
std::string keyf(const char* fmt, ...);

// ---- autotuner (engine_tune.hip)
// Optional persistent tuning results (env DF_TUNE_CACHE=<file>): one line "key tile splitk gm" per distinct GEMM.  A plan
// whose GEMMs are all in the file is configured from it without a single trial launch (profiling runs use this so
// that rocprof sees only the product launches); otherwise the plan is tuned and its results are appended.
struct TuneChoice { int tile, sk, gm; };
std::map<std::string, TuneChoice>& tune_cache();
extern bool g_tune_imported;       // set by df_tune_cache_import (see engine_tune.hip)
// "M_N_K_taps_stride_ups_batch_geglu_eEPI": the GEMM class a tuned choice belongs to (defer: the plan leaves its split-K slabs to the
// next GroupNorm).  The only place the EPI bits are assigned; df_test_gemm_key exposes it to the tests.
std::string tune_key(const GemmParams& g, int batch, bool defer);
void apply_tune_cache(Plan* pl);
void autotune_plan(df_ctx* c, Plan* pl, hipStream_t s);

// Every entry point runs under one process-wide lock: contexts share the autotuner's choices, the launchers keep function-attribute
// high-water marks in statics, and a plan build is not re-entrant.  The calls only enqueue work, so the lock is held for microseconds;
// what it buys is that two host threads may drive two models (or one) without corrupting any of that.  Recursive: test hooks nest.
extern std::recursive_mutex g_api_lock;     // defined with the C ABI

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

}  // namespace dfe

// libdfengine: plan execution -- finish_plan, the launch loop run_ops with its four debug hooks (checksums, saturation counts,
// bf16 re-rounding, workspace poisoning), and the plan cache get_plan (types: engine_internal.h).
#include "engine_internal.h"

DFE_NAMESPACE {

void finish_plan(df_ctx* c, Plan* pl) {
  if (pl->partial_bytes) {
    HIPCHK(hipMalloc((void**)&pl->partial, pl->partial_bytes));
    for (auto& o : pl->ops)
      if (o.is_gemm && o.gp.splitk > 1) o.gp.partial = pl->partial;
  }
  std::stable_sort(pl->poison_at.begin(), pl->poison_at.end(),
                   [](const std::pair<size_t, Block>& a, const std::pair<size_t, Block>& b) { return a.first < b.first; });
  HIPCHK(hipStreamSynchronize(c->pack_stream));   // weight packing done before first use
}

namespace {

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
    for (auto& b : pl->pinned) v.push_back({(const uint32_t*)b.p, (unsigned long long)(b.bytes / 4)});
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

// Every operand-type buffer an op stores: what it declared (Builder::emits) and, for a GEMM, what its GemmParams say -- C per
// batch slice, the aux copy, the transposed V (the two debug hooks below walk this list)
std::vector<OutBuf> operand_outputs(const Op& o) {
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
  return outs;
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
  const std::vector<OutBuf> outs = operand_outputs(o);
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
  const std::vector<OutBuf> outs = operand_outputs(o);
  for (auto& b : outs) {
    const long total = b.rows * (long)b.cols;
    if (total <= 0) continue;
    const int blocks = (int)std::min<long>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(requant_bf16_kernel, dim3(blocks), dim3(256), 0, s, const_cast<uint16_t*>(b.p), b.rows, b.cols, b.ld);
  }
}

// df_debug_poison: the blocks whose release took effect right behind op `op_index` are filled with 0xFF bytes -- whoever reads them
// from here on without writing first (the next tenant, or the owner that released too early) reads NaN
void poison_after_op(Plan* pl, size_t op_index, hipStream_t s) {
  auto it = std::lower_bound(pl->poison_at.begin(), pl->poison_at.end(), op_index + 1,
                             [](const std::pair<size_t, Block>& e, size_t v) { return e.first < v; });
  for (; it != pl->poison_at.end() && it->first == op_index + 1; ++it) HIPCHK(hipMemsetAsync(it->second.p, 0xFF, it->second.bytes, s));
}

// ... and the slabs a split-K GEMM may use, in front of its launch: an element that no K slice writes and the reduce (or the
// GroupNorm the reduce was handed to) still sums is NaN
void poison_partial(Plan* pl, const GemmParams& g, hipStream_t s) {
  if (!pl->partial || g.partial != pl->partial) return;
  const size_t need = (size_t)g.splitk * g.M * g.N * 4 * (g.taps == 4 ? 4 : 1);
  HIPCHK(hipMemsetAsync(pl->partial, 0xFF, std::min(need, pl->partial_bytes), s));
}

}  // namespace

void run_ops(df_ctx* c, Plan* pl, size_t begin, size_t end, hipStream_t s, const RunArgs& a) {
  for (size_t i = begin; i < end; ++i) {
    Op& o = pl->ops[i];
    hipError_t e;
    const char* why = nullptr;       // launch_gemm's rule, when it refuses
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
      if (pl->poison && g.splitk > 1) poison_partial(pl, g, s);
      e = launch_gemm(g, o.tile, o.batch, s, &why);
    } else {
      e = o.fn(s, a);
    }
    if (e != hipSuccess) {
      if (o.is_gemm)
        fail("op %zu (%s: GEMM %dx%dx%d taps %d batch %d tile %d split-K %d) failed: %s%s%s%s", i, o.tag, o.gp.M, o.gp.N, o.gp.K,
             o.gp.taps, o.batch, o.tile, o.gp.splitk, hipGetErrorString(e), why ? " (" : "", why ? why : "", why ? ")" : "");
      fail("op %zu (%s) failed: %s", i, o.tag, hipGetErrorString(e));
    }
    if (c->prof_on) {
      HIPCHK(hipEventRecord(c->prof_ev[c->prof_used + 1], s));
      c->prof_fam.push_back(op_family(o));
      c->prof_op.push_back(&o);
      c->prof_used += 2;
    }
    if (pl->poison) poison_after_op(pl, i, s);
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
  p->poison = c->poison_on;
  build(p.get());
  const bool tunable = !p->fixed_choices;
  if (tunable && (c->autotune || g_tune_imported)) {
    // tuning may try larger split-K factors than the cost model picked: give the scratch some head-room
    size_t want = 0;
    for (auto& o : p->ops)
      if (o.is_gemm && o.batch == 1) want = std::max(want, (size_t)32 * o.gp.M * o.gp.N * 4 * (o.gp.taps == 4 ? 4 : 1));
    if (want > ((size_t)512 << 20)) want = (size_t)512 << 20;
    if (want > p->partial_bytes) p->partial_bytes = want;
  }
  finish_plan(c, p.get());
  if (!tunable) {
  } else if (c->autotune) {
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

}  // namespace dfe

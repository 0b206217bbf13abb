// libdfengine: the context's weight packers -- fp32 checkpoint tensors -> MFMA operand layouts, once per key, on pack_stream
// (declarations: engine_internal.h).
#include "engine_internal.h"

using namespace dfe;

const bf16_t* df_ctx::w_linear(const std::string& name) {
  return (const bf16_t*)pack_once(name, [&] {
    const RawT& t = rt(name);
    (void)f32(name);
    bf16_t* o = (bf16_t*)pmalloc(t.n * 2);
    HIPCHK(launch_cast_bf16(t.d, o, (long)t.n, pack_stream));
    return o;
  });
}
const bf16_t* df_ctx::w_stack(const std::string& key, const std::vector<std::string>& names) {
  return (const bf16_t*)pack_once(key, [&] {
    size_t tot = 0;
    for (auto& n : names) tot += rt(n).n;
    bf16_t* o = (bf16_t*)pmalloc(tot * 2);
    size_t off = 0;
    for (auto& n : names) {
      const RawT& t = rt(n);
      HIPCHK(launch_cast_bf16(t.d, o + off, (long)t.n, pack_stream));
      off += t.n;
    }
    return o;
  });
}
const float* df_ctx::b_stack(const std::string& key, const std::vector<std::string>& names) {
  return (const float*)pack_once(key, [&] {
    size_t tot = 0;
    for (auto& n : names) tot += rt(n).n;
    float* o = (float*)pmalloc(tot * 4);
    size_t off = 0;
    for (auto& n : names) {
      const RawT& t = rt(n);
      HIPCHK(hipMemcpyAsync(o + off, t.d, t.n * 4, hipMemcpyDeviceToDevice, pack_stream));
      off += t.n;
    }
    return o;
  });
}
const bf16_t* df_ctx::w_conv3(const std::string& name, int ipad) {
  return (const bf16_t*)pack_once(name + "#c3", [&] {
    const RawT& t = rt(name);
    if (t.shape.size() != 4 || t.shape[2] != 3 || t.shape[3] != 3) fail("'%s' is not a 3x3 conv weight", name.c_str());
    const int O = (int)t.shape[0], I = (int)t.shape[1];
    bf16_t* o = (bf16_t*)pmalloc((size_t)O * 9 * ipad * 2);
    HIPCHK(launch_pack_conv_weight(t.d, o, O, I, 3, 3, ipad, pack_stream));
    return o;
  });
}
const bf16_t* df_ctx::w_conv3_ups4(const std::string& name, int ipad) {
  return (const bf16_t*)pack_once(name + "#c3ups4", [&] {
    const RawT& t = rt(name);
    if (t.shape.size() != 4 || t.shape[2] != 3 || t.shape[3] != 3) fail("'%s' is not a 3x3 conv weight", name.c_str());
    const int O = (int)t.shape[0], I = (int)t.shape[1];
    bf16_t* o = (bf16_t*)pmalloc((size_t)16 * O * ipad * 2);
    HIPCHK(launch_pack_conv_ups4(f32(name), o, O, I, ipad, pack_stream));
    return o;
  });
}
void df_ctx::w_conv3_skip(const std::string& conv, const std::string& skip, const bf16_t** w, const float** b) {
  const auto blk = pack_once<2>({conv + ".weight#c3skip", conv + ".bias#c3skip"}, [&]() -> std::array<void*, 2> {
    const RawT& t = rt(conv + ".weight");
    const RawT& ts = rt(skip + ".weight");
    const int O = (int)t.shape[0], I = (int)t.shape[1], I2 = (int)ts.shape[1];
    bf16_t* wo = (bf16_t*)pmalloc((size_t)O * (9 * I + I2) * 2);
    float* bo = (float*)pmalloc((size_t)O * 4);
    HIPCHK(launch_pack_conv_skip(f32(conv + ".weight"), f32(skip + ".weight"), wo, O, I, I2, pack_stream));
    const float* ins[2] = {f32(conv + ".bias"), f32(skip + ".bias")};
    const float co[2] = {1.f, 1.f};
    HIPCHK(launch_lincomb(bo, ins, co, 2, O, pack_stream));
    return {wo, bo};
  });
  *w = (const bf16_t*)blk[0];
  *b = (const float*)blk[1];
}
void df_ctx::w_ffproj(const std::string& ff2, const std::string& po, const bf16_t** w, const float** b) {
  const auto blk = pack_once<2>({ff2 + ".weight#ffproj", ff2 + ".bias#ffproj"}, [&]() -> std::array<void*, 2> {
    const RawT& t2 = rt(ff2 + ".weight");
    const RawT& tp = rt(po + ".weight");
    const int C = (int)t2.shape[0], F = (int)t2.shape[1];
    if ((int)tp.shape[0] != C || (int)tp.shape[1] != C) fail("ffproj: proj_out is not %dx%d", C, C);
    bf16_t* wo = (bf16_t*)pmalloc((size_t)C * (F + C) * 2);
    float* bo = (float*)pmalloc((size_t)C * 4);
    HIPCHK(launch_pack_ffproj(f32(po + ".weight"), f32(po + ".bias"), f32(ff2 + ".weight"), f32(ff2 + ".bias"), wo, bo, C, F,
                              pack_stream));
    return {wo, bo};
  });
  *w = (const bf16_t*)blk[0];
  *b = (const float*)blk[1];
}
const bf16_t* df_ctx::w_lnq_t(const std::string& wq, const std::string& norm, float scale) {
  return (const bf16_t*)pack_once(wq + "#lnqT", [&] {
    const RawT& t = rt(wq);
    const int C = (int)t.shape[0];
    if ((int)t.shape[1] != C) fail("w_lnq_t %s: not square", wq.c_str());
    bf16_t* o = (bf16_t*)pmalloc((size_t)C * C * 2);
    HIPCHK(launch_pack_lnq_t(t.d, f32(norm + ".weight"), o, C, scale, pack_stream));
    return o;
  });
}
const bf16_t* df_ctx::w_stack_t(const std::string& key, const std::vector<std::string>& names) {
  return (const bf16_t*)pack_once(key, [&] {
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
    return o;
  });
}
const bf16_t* df_ctx::w_conv3_bwd(const std::string& name) {
  return (const bf16_t*)pack_once(name + "#c3bwd", [&] {
    const RawT& t = rt(name);
    const int O = (int)t.shape[0], I = (int)t.shape[1], Opad = (O + 63) / 64 * 64;
    bf16_t* o = (bf16_t*)pmalloc((size_t)I * 9 * Opad * 2);
    HIPCHK(launch_pack_conv_bwd(t.d, o, O, I, Opad, pack_stream));
    return o;
  });
}
void df_ctx::w_conv3d_bn(const std::string& p, int kp, const bf16_t** w, const float** b) {
  const std::string kw = "c3d:" + p + ":" + std::to_string(kp);
  const auto blk = pack_once<2>({kw, kw + ":b"}, [&]() -> std::array<void*, 2> {
    const RawT& t = rt(p + ".conv.weight");
    if (t.shape.size() != 5) fail("%s.conv.weight: expected a 5-D Conv3d weight", p.c_str());
    const int O = (int)t.shape[0], I = (int)t.shape[1], KT = (int)t.shape[2], KH = (int)t.shape[3], KW = (int)t.shape[4];
    bf16_t* wo = (bf16_t*)pmalloc((size_t)O * kp * 2);
    float* bo = (float*)pmalloc((size_t)O * 4);
    HIPCHK(launch_pack_conv3d_bn(t.d, f32(p + ".bn.weight"), f32(p + ".bn.bias"), f32(p + ".bn.running_mean"),
                                 f32(p + ".bn.running_var"), 1e-5f, wo, bo, O, I, KT, KH, KW, kp, pack_stream));
    return {wo, bo};
  });
  *w = (const bf16_t*)blk[0];
  *b = (const float*)blk[1];
}

void df_ctx::w_conv2d_bn(const std::string& conv, const std::string& bn, int kp, const bf16_t** w, const float** b) {
  const std::string kw = "c2d:" + conv + ":" + std::to_string(kp);
  const auto blk = pack_once<2>({kw, kw + ":b"}, [&]() -> std::array<void*, 2> {
    const RawT& t = rt(conv + ".weight");
    if (t.shape.size() != 4 || t.shape[2] != 3 || t.shape[3] != 3) fail("'%s.weight' is not a 3x3 conv weight", conv.c_str());
    const int O = (int)t.shape[0], I = (int)t.shape[1];
    bf16_t* wo = (bf16_t*)pmalloc((size_t)O * kp * 2);
    float* bo = (float*)pmalloc((size_t)O * 4);
    HIPCHK(launch_pack_conv3d_bn(f32(conv + ".weight"), f32(bn + ".weight"), f32(bn + ".bias"), f32(bn + ".running_mean"),
                                 f32(bn + ".running_var"), 1e-5f, wo, bo, O, I, 1, 3, 3, kp, pack_stream));
    return {wo, bo};
  });
  *w = (const bf16_t*)blk[0];
  *b = (const float*)blk[1];
}

void df_ctx::w_ln_stack(const std::string& key, const std::string& norm, const std::vector<std::string>& names,
                        const std::vector<std::string>& biases, bool geglu, const bf16_t** w, const float** cs, const float** bb) {
  const auto blk = pack_once<3>({key + "#lnw", key + "#lncs", key + "#lnbb"}, [&]() -> std::array<void*, 3> {
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
    return {wo, co, bo};
  });
  *w = (const bf16_t*)blk[0];
  *cs = (const float*)blk[1];
  *bb = (const float*)blk[2];
}

void df_ctx::w_ln_w320(const std::string& key, int rows, int K, const bf16_t** w, const float** cs, const float** bb) {
  const std::string kw = key + "#lnw", kc = key + "#lncs", kb = key + "#lnbb";
  const auto blk = pack_once<3>({key + "#lnw320", key + "#lncs320", key + "#lnbb320"}, [&]() -> std::array<void*, 3> {
    if (!packed.count(kw) || !packed.count(kc) || !packed.count(kb)) fail("w_ln_w320 %s: the (32 | 32) packing does not exist", key.c_str());
    bf16_t* wo = (bf16_t*)pmalloc((size_t)rows * K * 2);
    float* co = (float*)pmalloc((size_t)rows * 4);
    float* bo = (float*)pmalloc((size_t)rows * 4);
    HIPCHK(launch_pack_w320((const bf16_t*)packed[kw], (const float*)packed[kc], (const float*)packed[kb], wo, co, bo, rows, K, pack_stream));
    return {wo, co, bo};
  });
  *w = (const bf16_t*)blk[0];
  *cs = (const float*)blk[1];
  *bb = (const float*)blk[2];
}

void df_ctx::w_geglu(const std::string& prefix, const bf16_t** w, const float** b) {
  const auto blk = pack_once<2>({prefix + ".weight#geglu", prefix + ".bias#geglu"}, [&]() -> std::array<void*, 2> {
    const RawT& tw = rt(prefix + ".weight");
    const RawT& tb = rt(prefix + ".bias");
    const int rows = (int)tw.shape[0], K = (int)tw.shape[1];
    bf16_t* wo = (bf16_t*)pmalloc((size_t)rows * K * 2);
    float* bo = (float*)pmalloc((size_t)rows * 4);
    HIPCHK(launch_pack_geglu(tw.d, tb.d, wo, bo, rows / 2, K, pack_stream));
    return {wo, bo};
  });
  *w = (const bf16_t*)blk[0];
  *b = (const float*)blk[1];
}

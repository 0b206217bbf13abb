/* df_engine.h -- C ABI of libdfengine.so, the MI355X (gfx950) engine behind the Diff-Foley
 * Stage-2 sampling path.
 *
 * The reference (luosiallen/Diff-Foley) has NO FFI/plugin boundary: the hot path is a tree of
 * torch.nn modules driven from Python.  Each entry point below replaces one Python-level call
 * of the reference; the reference-side binding a maintainer would add is the ctypes stub shown
 * in INTEGRATION.md (and implemented in diff_foley_amd/engine.py).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; df_last_error() gives the message
 *     (thread-local); nothing throws across the ABI.
 *   - "dev" pointers are device pointers (torch tensor.data_ptr()); the caller owns every I/O buffer,
 *     the library owns packed weights and workspaces for the lifetime of the ctx.
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no internal
 *     synchronisation except in df_load_tensor / df_finalize / df_autotune.
 *   - latents are NCHW fp32 exactly as the reference passes them; internal layout is NHWC.
 *   - one ctx per device per process; a ctx is not re-entrant.
 */
#ifndef DF_ENGINE_H
#define DF_ENGINE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct df_ctx df_ctx;

/* UNetModel / Classifier_Backbone hyper-parameters
 * (diff_foley/modules/diffusionmodules/openai_unetmodel.py:443-468, inference/config/Stage2_LDM.yaml:21-36,
 *  inference/config/Double_Guidance_Classifier.yaml:35-50). */
typedef struct {
  int in_channels, out_channels, model_channels, num_res_blocks;
  int channel_mult[8];
  int n_mult;
  int attention_resolutions[8];
  int n_attn;
  int num_heads;
  int context_dim;
} df_unet_config;

/* AutoencoderKL decoder ddconfig (Stage2_LDM.yaml:38-59) + LatentDiffusion.scale_factor (:17). */
typedef struct {
  int z_channels, embed_dim, ch, num_res_blocks, out_ch;
  int ch_mult[8];
  int n_mult;
  float scale_factor;
} df_vae_config;

/* What AutoencoderKL's Encoder needs beyond the decoder's df_vae_config -- stage1_autoencoder/model.py:463-527, Stage2_LDM.yaml:47: the channels of
 * the image it reads.  ch, ch_mult, num_res_blocks, z_channels and embed_dim are the decoder's (double_z = true). */
typedef struct {
  int in_channels;
} df_vae_encoder_config;

/* Video_Feat_Encoder_Posembed (Stage2_LDM.yaml:62-67). */
typedef struct {
  int origin_dim, embed_dim, seq_len;
} df_cond_config;

/* CAVP video encoder = ResNet3dSlowOnly(depth 50) + video_project_head (inference/model/cavp_model.py:21-29,
 * inference/model/cavp_modules.py:1233-1268): blocks per stage (3,4,6,3), stem width 64, feature width embed_dim. */
typedef struct {
  int stage_blocks[4];
  int base_channels;
  int embed_dim;
} df_cavp_config;

/* CAVP spectrogram encoder = Cnn14 + final_project (inference/model/cavp_model.py:36, inference/model/cavp_modules.py:1487-1546).
 * The reference fixes n_mels 128 (the input BatchNorm2d), channels 64 .. 2048 doubling, fc_dim 2048 (fc1 is applied twice, so
 * fc_dim == channels[5]) and embed_dim 512; carrying them lets a narrow net run the same plan, as stage_blocks does above. */
typedef struct {
  int n_mels;
  int channels[6];
  int fc_dim;
  int embed_dim;
} df_cavp_spec_config;

/* ---- lifetime ------------------------------------------------------------------------------ */
int df_create(int device, df_ctx** out);
void df_destroy(df_ctx* ctx);
const char* df_last_error(void);
int df_abi_version(void);
/* MFMA operand type this build was compiled for: "bf16" (libdfengine.so) or "f16" (libdfengine_f16.so, built from
 * the same sources with -DDF_OPERAND_F16).  2-byte operand buffers passed to the df_test_* entry points use it. */
const char* df_operand_dtype(void);

/* ---- model definition: replaces instantiate_from_config(config.model) + load_state_dict()
 *      (inference/diff_foley_inference.ipynb:80-95; diff_foley/util.py:176-191).
 * `name` is the reference state_dict key (e.g. "model.diffusion_model.input_blocks.1.0.in_layers.2.weight");
 * classifier tensors are loaded under the prefix "classifier." + their own key ("classifier.model....").
 * `host` is fp32, C-contiguous; it is copied before the call returns. */
int df_config_unet(df_ctx* ctx, const df_unet_config* cfg);
int df_config_vae(df_ctx* ctx, const df_vae_config* cfg);
int df_config_cond(df_ctx* ctx, const df_cond_config* cfg);
/* Optional: the VAE encoder + quant_conv ("first_stage_model.encoder.*", "first_stage_model.quant_conv.*"; autoencoder.py:324-328).
 * Configured only by a caller that loads those tensors: df_finalize then requires every one of them.  cfg == NULL takes the encoder
 * out of the configuration again.  in_channels above 4 is refused when a plan is built. */
int df_config_vae_encoder(df_ctx* ctx, const df_vae_encoder_config* cfg);
/* The same encoder in a context that never decodes (the Align-Acc metric model, alignment_classifier_metric.py:196-210): `vae` gives
 * the shape the encoder shares with the decoder (ch, ch_mult, num_res_blocks, z_channels, embed_dim); the decoder itself stays
 * unconfigured, so no post_quant_conv / decoder tensor is loaded or packed and df_vae_decode refuses.  A later df_config_vae
 * configures the decoder as usual. */
int df_config_vae_encoder_only(df_ctx* ctx, const df_vae_config* vae, const df_vae_encoder_config* enc);
int df_config_classifier(df_ctx* ctx, const df_unet_config* cfg);
/* Tensors of the CAVP video branch are loaded under "cavp." + the CAVP_Inference state_dict key
 * ("cavp.video_encoder.conv1.conv.weight", "cavp.video_encoder.layer1.0.conv1.bn.running_var",
 * "cavp.video_project_head.weight", ...). */
int df_config_cavp(df_ctx* ctx, const df_cavp_config* cfg);
int df_load_tensor(df_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
/* Same, but the fp32 source already lives on the device (used after an RCCL weight broadcast). */
int df_load_tensor_dev(df_ctx* ctx, const char* name, const float* dev, const int64_t* shape, int ndim);
/* Checks every tensor the configured modules need is present and re-packs to bf16 MFMA layouts. */
int df_finalize(df_ctx* ctx);
/* Optional: time the candidate tile shapes of every GEMM of the plans built so far and keep the fastest. */
int df_autotune(df_ctx* ctx, int enable);

/* ---- LatentDiffusion.get_learned_conditioning (ddpm.py:568-579 -> video_feat_encoder.py:12-18)
 * feats [B][T][origin_dim] fp32 -> out [B][T][embed_dim] fp32 */
int df_cond_encode(df_ctx* ctx, const float* feats_dev, float* out_dev, int B, int T, void* stream);

/* ---- CAVP_Inference.encode_video(video, normalize, pool=False) (inference/model/cavp_model.py:47-65), as called by
 * Extract_CAVP_Features.forward (inference/demo_util.py:150-167): video [B][T][3][H][W] fp32 RGB in [0,1] (H, W
 * multiples of 32; the reference uses 224) -> out [B][T][embed_dim] fp32, rows L2-normalised when normalize != 0.
 * Clips are independent; the temporal (3,1,1) convolutions zero-pad inside each clip of T frames. */
int df_cavp_encode(df_ctx* ctx, const float* video_dev, float* out_dev, int B, int T, int H, int W, int normalize,
                   void* stream);

/* The pooled form, encode_video(..., pool=True) (cavp_model.py:58-59: nn.MaxPool1d(kernel_size=16) over the frame axis of the
 * projected features, then the optional F.normalize): feat [B][T][C] fp32 (df_cavp_encode with normalize = 0) -> out
 * [B][T / kernel][C], rows L2-normalised when normalize != 0. */
int df_cavp_pool(const float* feat_dev, float* out_dev, int B, int T, int C, int kernel, int normalize, void* stream);

/* ---- CAVP_Inference.encode_spec(spec, normalize, pool=False) (inference/model/cavp_model.py:68-84 -> Cnn14.forward,
 * inference/model/cavp_modules.py:1516-1546).  Tensors are loaded under "cavp." + the CAVP_Inference state_dict key
 * ("cavp.spec_encoder.bn.weight", "cavp.spec_encoder.conv_block3.conv2.weight", "cavp.spec_encoder.fc1.bias", ...); the plan is
 * built from them at the first call, so a context without them fails there.  spec [B][n_mels][T] fp32, the normalised log-mel as the
 * caller holds it (the reference's unsqueeze + permute is an address rule of the first kernel) -> out [B][T'][embed_dim] fp32, T' = T
 * floor-halved four times, rows L2-normalised when normalize != 0.  n_mels must be the configured one and T >= 16 (one output row).
 * A clip's rows do not depend on its batch-mates: every GEMM's tile and split-K is chosen for the per-sample problem and no tune-table
 * entry is taken.  Any B >= 1: large batches run as slices inside this call.  The pooled form is df_cavp_pool on the result. */
int df_config_cavp_spec(df_ctx* ctx, const df_cavp_spec_config* cfg);
int df_cavp_spec_encode(df_ctx* ctx, const float* spec_dev, float* out_dev, int B, int n_mels, int T, int normalize, void* stream);

/* Audio / video agreement of CAVP features (no reference counterpart: the reference forms the contrastive logits in its training
 * loss only; this is the frame-wise form of that product for ranking generated candidates against one video).
 * out[i][j] = scale * mean_t <v[i][t][:], s[j][t][:]>: v [Bv][T][D], s [Bs][T][D], out [Bv][Bs], all fp32, D a multiple of 4.
 * scale: logit_scale.exp() or 1.  Stateless, no atomics: the result is a pure function of the inputs. */
int df_cavp_similarity(const float* v_dev, const float* s_dev, float* out_dev, int Bv, int Bs, int T, int D, float scale,
                       void* stream);

/* ---- UNetModel.forward (openai_unetmodel.py:710-742) through LatentDiffusion.apply_model (ddpm.py:925-1026).
 * The cross-attention context is step-invariant, so it is set once per sample() call: everything of the 16
 * SpatialTransformers' cross-attention that depends on the context only is computed here, not per step -- the K/V
 * projections and, for T <= 32, their products with the (LayerNorm-folded) query and output projections, so that a step
 * runs cross-attention as two GEMMs against per-sample operands.  context [N][T][context_dim] fp32. */
int df_unet_set_context(df_ctx* ctx, const float* context_dev, int N, int T, void* stream);
/* x [N][C][H][W] fp32, t [N] fp32 (integer or fractional timesteps), eps_out [N][C][H][W] fp32. */
int df_unet_forward(df_ctx* ctx, const float* x_dev, const float* t_dev, float* eps_out_dev, int N, int H, int W,
                    void* stream);
/* Classifier-free-guidance step of p_sample_ddim (ddim.py:241-245): runs the UNet on cat([x,x]) against the
 * 2B-row context set before ([uncond ; cond]) and returns e_u + scale*(e_c - e_u).  x, t, eps: B rows.  The ops in front of
 * the first cross-attention see identical rows in both halves and run on one half only. */
int df_unet_forward_cfg(df_ctx* ctx, const float* x_dev, const float* t_dev, float* eps_out_dev, int B, int H, int W,
                        float guidance_scale, void* stream);
/* Time embedding of a whole sample() call, hoisted out of the step loop like the context (timestep_embedding util.py:151-171 ->
 * time_embed openai_unetmodel.py:506-511,724 -> every ResBlock's emb_layers :262: all of it depends on t only, and a sampler
 * knows its S timesteps before the loop -- ddim.py:193-201, plms.py:127-135, dpm_solver.py:1071-1079).  t_host[S]: the
 * timesteps (host memory; integer or fractional), each used for every sample of the batch as the reference samplers do
 * (ddim.py:217).  N, H, W, cfg name the plan (cfg != 0: the CFG plan of df_unet_forward_cfg with B = N).  Call after
 * df_unet_set_context.  The *_ts entry points then take the INDEX of the step's timestep in that table instead of t_dev and
 * replace the four time-embedding launches of a step by one table look-up; results are bit-identical to the t_dev forms.
 * Announcing the timesteps the plan's table already holds returns at once (a service's sample() calls repeat the same 25 / 50). */
int df_unet_set_timesteps(df_ctx* ctx, const float* t_host, int S, int N, int H, int W, int cfg, void* stream);
int df_unet_forward_ts(df_ctx* ctx, const float* x_dev, int ts_index, float* eps_out_dev, int N, int H, int W, void* stream);
int df_unet_forward_cfg_ts(df_ctx* ctx, const float* x_dev, int ts_index, float* eps_out_dev, int B, int H, int W,
                           float guidance_scale, void* stream);

/* ---- LatentDiffusion.decode_first_stage (ddpm.py:739-797 -> autoencoder.py:330-333 -> model.py:630-663)
 * z [B][z_channels][H][W] fp32 -> out [B][out_ch][H*2^(n_mult-1)][W*2^(n_mult-1)] fp32.  Any B: batches whose widest
 * activation would exceed the 2 GiB operand addressing (B > 16 at the full decoder) run as slices inside this call. */
int df_vae_decode(df_ctx* ctx, const float* z_dev, float* out_dev, int B, int H, int W, void* stream);

/* ---- AutoencoderKL.encode up to the posterior's parameters (autoencoder.py:324-328 -> stage1_autoencoder/model.py:529-554, the
 * Downsample of :167-171), as LatentDiffusion.encode_first_stage reaches it (ddpm.py:860-899 without split_input_params).
 * x [B][in_channels][H][W] fp32 -> moments [B][2*embed_dim][H/f][W/f] fp32 = quant_conv(encoder(x)), f = 2^(n_mult-1): the
 * `parameters` of the DiagonalGaussianDistribution (model.py:34-37), mean in the first embed_dim channels, logvar in the rest.
 * H and W must be positive multiples of f (the reference floors odd maps; this engine refuses them).  Any B: batches whose widest
 * operand would pass the 2 GiB operand addressing run as slices inside this call, like df_vae_decode. */
int df_vae_encode(df_ctx* ctx, const float* x_dev, float* moments_dev, int B, int H, int W, void* stream);
/* DiagonalGaussianDistribution.sample() (model.py:38-47) with LatentDiffusion.get_first_stage_encoding's scale_factor (ddpm.py:559-566)
 * folded in: z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise); moments [B][2*zc][HW], noise / z [B][zc][HW] fp32.
 * noise_dev may be NULL: z = scale * mean (mode(), model.py:71-72).  Stateless, like df_lincomb. */
int df_posterior_sample(const float* moments_dev, const float* noise_dev, float* z_dev, int B, int zc, int HW, float scale,
                        void* stream);

/* ---- Align-Acc verdict of one batch (evaluation/align_acc.py:85-86): pred[b] = prob[b] rounded half to even (torch.round: 0.5 -> 0,
 * 1.5 -> 2), counts[0] += #(pred[b] == label[b]), counts[1] += B.  prob / pred [B] fp32, labels [B] fp32 or NULL (all 1, :76),
 * counts int64[2] on the device, zeroed by the caller before the first batch.  One block, one launch, no atomics: calls on one
 * stream accumulate in order, and a dataset loop reads the counters once, after its last batch.  Stateless, like df_lincomb. */
int df_align_verdict(const float* prob_dev, const float* labels_dev, float* pred_dev, int64_t* counts_dev, int B, void* stream);

/* ---- Alignment classifier forward (alignment_classifier.py:269-271 -> alignment_backbone.py:656-686)
 * x [B][C][H][W], t [B], video_feat [B][T][context_dim] (raw CAVP features) -> prob [B][out_channels] */
int df_classifier_forward(df_ctx* ctx, const float* x_dev, const float* t_dev, const float* feat_dev, float* prob_dev,
                          int B, int H, int W, int T, void* stream);

/* Classifier guidance gradient (cal_classifier_loglikelihood_grad, ddim.py:333-341; cond_grad_fn_classifier,
 * dpm_solver.py:1340-1349):  grad = d sum_b log p_b / d x  (UNSCALED), shape of x; prob (optional, may be NULL) [B][1].
 * Forward and hand-written backward-data pass run natively (no autograd). */
int df_classifier_grad(df_ctx* ctx, const float* x_dev, const float* t_dev, const float* feat_dev, float* prob_dev,
                       float* grad_dev, int B, int H, int W, int T, void* stream);

/* The same call for a guidance loop, which hands the classifier the SAME video features at every step (ddim.py:374-380 passes
 * origin_cond unchanged through all S steps; dpm_solver.py:1377-1393 closes over it): feat_token != 0 names the CONTENTS of
 * feat_dev.  While consecutive calls on a plan carry the same token, the feature-only launches (cast + cross-attention K / V^T
 * of every transformer block: 7 of the call's launches at the Stage-2 classifier) are skipped and feat_dev is not read.  The
 * caller changes the token whenever the features change; token 0 = no reuse (df_classifier_grad).  The plan holds the token:
 * a plan that was rebuilt (other shape, reloaded weights) recomputes whatever token it is handed first. */
int df_classifier_grad_cached(df_ctx* ctx, const float* x_dev, const float* t_dev, const float* feat_dev, float* prob_dev,
                              float* grad_dev, int B, int H, int W, int T, uint64_t feat_token, void* stream);

/* ---- video frame pre-processing in front of the CAVP encoder (Extract_CAVP_Features.forward, inference/demo_util.py:
 * 100-104, 150-151): per frame torchvision Resize((OH, OW)) on a PIL image (= PIL.Image.resize BILINEAR: antialiased,
 * 8-bit fixed point, horizontal pass then vertical pass -- vertical pass first on frames with H > 100 W and OH < H, as Pillow does)
 * + ToTensor().  frames uint8 [T][H][W][3] RGB ->
 * out fp32 [T][3][OH][OW] in [0, 1], bit-identical to Pillow.  bounds_* int32 [out][2] = (first input index, taps),
 * coef_* int32 [out][ksize] 22-bit fixed-point filter weights (computed in double precision on the host:
 * diff_foley_amd/video.py); tmp uint8 scratch for the first pass's result: [T][H][OW][3], or [T][OH][W][3] when H > 100 W and OH < H.
 * All pointers device memory. */
int df_frames_to_tensor(const uint8_t* frames_dev, float* out_dev, uint8_t* tmp_dev, int T, int H, int W, int OH, int OW,
                        const int32_t* bounds_w_dev, const int32_t* coef_w_dev, int ksize_w, const int32_t* bounds_h_dev,
                        const int32_t* coef_h_dev, int ksize_h, void* stream);

/* ---- mel -> waveform (inverse_op, inference/demo_util.py:196-211; algorithms of librosa 0.8.0, the
 * reference's pinned dependency).  df_mel_to_stft: undo the log-mel normalisation and invert the mel filterbank by
 * non-negative least squares (librosa.feature.inverse.mel_to_stft, power 1): mel [B][n_mels][T] -> S [B][T][513].
 * A [n_mels][513] = librosa.filters.mel(22050, 1024, n_mels, 125, 7600), At its transpose, Pt [n_mels][513] = pinv(A)^T
 * (the clipped least-squares start of librosa.util.nnls), inv_L = 1 / sigma_max(A)^2, iters FISTA iterations.
 * df_griffinlim: librosa.griffinlim(S, hop_length=256): 32 fast Griffin-Lim iterations, momentum 0.99; phase0
 * [B][513][T] uniform in [0,1) is the random initial phase; twiddles complex [512] exp(-2 pi i k/1024), window [1024]
 * periodic hann, wss [1024 + 256 (T-1)] window sum-square; workspaces: angles / reb0 / reb1 complex [B][T][513], frames
 * [B][T][1024]; wav [B][256 (T-1)].  All pointers device memory, all launches asynchronous on `stream`.
 * Refused before anything is launched (non-zero return, df_last_error() names the argument, no output is touched):
 * df_mel_to_stft -- B, n_mels or T < 1, n_mels > 128 (the size of the kernel's span tables), iters < 0 (0 returns the clipped
 * least-squares start), a null mel / A / At / Pt / S; df_griffinlim -- B < 1, T < 2 (one frame is zero hops of audio), n_iter < 0
 * (0 synthesises from the initial phase), momentum outside [0, 1) or NaN, any null pointer. */
int df_mel_to_stft(const float* mel_dev, int B, int n_mels, int T, const float* A_dev, const float* At_dev,
                   const float* Pt_dev, float inv_L, int iters, float* S_dev, void* stream);
int df_griffinlim(const float* S_dev, const float* phase0_dev, int B, int T, int n_iter, float momentum,
                  const float* twiddles_dev, const float* window_dev, const float* wss_dev, float* angles_dev,
                  float* reb0_dev, float* reb1_dev, float* frames_dev, float* wav_dev, void* stream);

/* ---- waveform -> mel, the forward direction of the above (get_spectrogram / TRANSFORMS, data_preprocess/wav2spec.py:145-155,
 * 170-189; librosa 0.8.0 stft + filters.mel on the CPU there): |stft(y, n_fft 1024, hop 256)| (periodic hann, centred,
 * np.pad reflect by 512 -- also for clips shorter than the pad) -> mel filterbank -> LowerThresh(floor), Log10, *20, -20, +100,
 * /100, Clip(0, 1).  wav fp32 [B][wav_stride >= L] -> mel fp32 [B][n_mels][T], T = 1 + L / 256 (the layout encode_first_stage
 * takes after the channel repeat).  A [n_mels][513] = librosa.filters.mel(sr, 1024, n_mels, fmin, fmax) (sr 16000 in wav2spec.py),
 * bands int32 [n_mels][2] = (first non-zero bin, count of bins up to the last non-zero one) of every row of A -- the kernel
 * walks only those; twiddles complex [512] exp(-2 pi i k/1024), window [1024] periodic hann, floor 1e-5.  1 <= n_mels <= 128,
 * B >= 1, L >= 1; no workspace, no atomics: the result is a pure function of the input.  All pointers device memory, the launch is
 * asynchronous on `stream`.  df_wave_to_mel_tile: frames per block of this build (returns the count, not a status). */
int df_wave_to_mel(const float* wav_dev, int64_t wav_stride, int B, int L, const float* A_dev, const int32_t* bands_dev,
                   int n_mels, const float* twiddles_dev, const float* window_dev, float floor, float* mel_dev, void* stream);
int df_wave_to_mel_tile(void);

/* ---- packed-operand blob (multi-GPU weight distribution; replaces SURVEY's df_bcast_weights: the RCCL
 * communicator belongs to torch.distributed, so the library exports / imports and the host side broadcasts).
 * Root rank: load tensors, df_finalize, df_prepack (builds every operand packing the UNet CFG-batch 2B / VAE / cond plans
 * of this shape use), df_packed_size, df_export_packed.  Other ranks: df_create, df_config_*, df_import_packed(manifest,
 * blob), df_finalize -- no fp32 master copies, no re-packing.  The manifest (host bytes) lists every tensor's shape, the
 * small fp32 tensors that plans read directly (biases, norm parameters, pos_emb) and every packed operand with its
 * offset into the blob (device bytes, 256-B aligned segments).  Operand type (bf16 / fp16 build) is checked on import. */
int df_prepack(df_ctx* ctx, int B, int H, int W, int T);
int df_packed_size(df_ctx* ctx, size_t* manifest_bytes, size_t* blob_bytes);
int df_export_packed(df_ctx* ctx, void* manifest_host, void* blob_dev, void* stream);
int df_import_packed(df_ctx* ctx, const void* manifest_host, size_t manifest_bytes, const void* blob_dev,
                     size_t blob_bytes, void* stream);

/* ---- sampler arithmetic on fp32 latents (n = number of elements) -------------------------------
 * e = e_u + scale*(e_c - e_u), e2 = [e_u ; e_c]                     (ddim.py:245, dpm_solver.py:1386) */
int df_cfg_combine(const float* e2_dev, float* e_dev, int64_t n, float scale, void* stream);
/* out = sum_i coef[i]*in[i], 1..4 terms; out may alias an input  (DPM-Solver++ updates dpm_solver.py:504-549,
 * 755-810; PLMS multistep plms.py:219-232; classifier guidance ddim.py:380) */
int df_lincomb(float* out_dev, const float* const* in_dev, const float* coef, int nterms, int64_t n, void* stream);
/* Inpainting blend of the samplers (reference ddim.py:206-209, plms.py:147-150, ddpm.py:1239-1241 with q_sample ddpm.py:279-282):
 * out = (sqrt_acp * x0 + sqrt_one_minus_acp * noise) * mask + (1 - mask) * img.  All tensors fp32 NCHW [B][C][H][W] (n elements,
 * chw per sample, hw per channel); mask is [B][mask_c][H][W] with mask_c = 1 (broadcast over channels) or C.  out != img. */
int df_q_sample_blend(const float* img_dev, const float* x0_dev, const float* noise_dev, const float* mask_dev, float* out_dev,
                      int64_t n, int64_t chw, int64_t hw, int mask_c, float sqrt_acp, float sqrt_one_minus_acp, void* stream);
/* The forward process at a PER-SAMPLE timestep (LatentDiffusion.q_sample, ddpm.py:279-282; DDIMSampler.stochastic_encode,
 * ddim.py:412-413): out[b] = A[t[b]] * x0[b] + S[t[b]] * noise[b].  x0 / noise / out fp32 [B][n] contiguous, t int64 [B] ON THE
 * DEVICE (a torch.randint result needs no host round trip), A / S fp32 device tables of T entries: the model's sqrt_alphas_cumprod /
 * sqrt_one_minus_alphas_cumprod, or a sampler's sqrt(ddim_alphas) / ddim_sqrt_one_minus_alphas.  A t[b] outside [0, T) never becomes
 * an address: that sample's output is NaN in every element and the tables are not read for it.  float4 loads and stores where the
 * three tensors share an alignment (scalar elements up to the first 16-byte boundary of every sample and behind its last whole
 * float4), scalar otherwise.  out must not alias x0 or noise.  B, n, T >= 1.  Stateless, like df_lincomb. */
int df_q_sample(const float* x0_dev, const float* noise_dev, const int64_t* t_dev, const float* A_dev, const float* S_dev,
                float* out_dev, int B, int64_t n, int T, void* stream);
/* The denoising loss of LatentDiffusion.p_losses behind its UNet call (get_loss ddpm.py:284-297, the reduction ddpm.py:1061-1079).
 * pred / target fp32 [B][n], t int64 [B] and the tables logvar / lvlb_weights fp32 [T] on the device; loss_type 0 = l2, 1 = l1.
 * loss_simple[b] = mean over n of (target - pred)^2 or |target - pred| (:1061), and scalars[5] =
 *   { mean(loss_simple)                                           loss_simple  (:1062)
 *     mean(loss_simple / exp(logvar[t]) + logvar[t])              loss_gamma   (:1067-1070)
 *     mean(lvlb_weights[t] * loss_simple)                         loss_vlb     (:1075-1077)
 *     l_simple_weight * [1] + original_elbo_weight * [2]          loss         (:1073, 1078-1079)
 *     mean(logvar) over the T entries                             logvar       (:1071) }.
 * Two launches: one block per sample (per-lane sums, a DPP tree per wavefront, one LDS step across wavefronts), then one wavefront
 * that adds the B values in a fixed order.  No atomics: equal inputs give equal bits.  A t[b] outside [0, T) reads no table and
 * makes loss_simple[b] and scalars[0..3] NaN.  B, n, T >= 1.  Stateless. */
int df_diffusion_loss(const float* pred_dev, const float* target_dev, const int64_t* t_dev, const float* logvar_dev,
                      const float* lvlb_weights_dev, float* loss_simple_dev, float* scalars_dev, int B, int64_t n, int T,
                      int loss_type, float l_simple_weight, float original_elbo_weight, void* stream);
/* The data prediction of DPM-Solver++ (DPM_Solver.data_prediction_fn, dpm_solver.py:386-399): out = (x - sigma * eps) / alpha over
 * fp32 [B][n], alpha / sigma the schedule's values at the step's time.  thresholding != 0 adds Imagen's dynamic thresholding per
 * sample: s = max(quantile_0.995(|x0|), max_val), out = clamp(x0, -s, s) / s.  The quantile follows torch.quantile's 'linear' rule
 * (rank 0.995 (n - 1) in fp32, linear interpolation between the two neighbouring order statistics) and is an exact selection: a
 * four-pass radix select on the bit patterns of |x0| with 256-bin histograms in LDS, one block per sample, x0 re-evaluated
 * identically in every pass.  s_out (fp32 [B], may be NULL) receives s.  A NaN anywhere in a sample makes s and the whole sample
 * NaN, as torch.quantile does.  Integer LDS atomics only: equal inputs give equal bits.  out must not alias x or eps.  B, n >= 1;
 * with thresholding n <= 2^30.  Stateless, like df_lincomb. */
int df_dpm_data_prediction(const float* x_dev, const float* eps_dev, float* out_dev, float* s_out_dev, int B, int64_t n, float alpha,
                           float sigma, int thresholding, float max_val, void* stream);
/* The error estimate of the adaptive DPM-Solver (dpm_solver_adaptive, dpm_solver.py:952-954):
 * out[0] = max over b of norm[b], norm[b] = sqrt(mean_i(((x_hi - x_lo) / max(atol, rtol * max(|x_lo|, |x_prev|)))^2)); all tensors
 * fp32 [B][n] on the device, norm fp32 [B] and out fp32 [1] on the device (the driver reads out).  One block per sample, then one
 * wavefront over the batch: no atomics, fixed summation order.  A NaN norm makes out NaN.  B, n >= 1.  Stateless. */
int df_dpm_adaptive_error(const float* x_hi_dev, const float* x_lo_dev, const float* x_prev_dev, float* norm_dev, float* out_dev,
                          int B, int64_t n, float atol, float rtol, void* stream);
/* Overlapped windows of a long fp32 tensor x [B][rows][W] (an NCHW latent or image with rows = C * H): K windows of Ww columns,
 * window k at column starts[k] (HOST int32 array).  Both entries check the geometry on the host and launch nothing when it is bad
 * (return 1, df_last_error names the rule): K, B, rows, Ww >= 1, W >= Ww, 0 <= starts[k], starts[k] + Ww <= W, starts ascending, every
 * column of [0, W) covered by a window.  Any integer starts and widths are served (4-byte accesses only).
 *   df_window_gather: win[b * K + k][row][j] = x[b][row][starts[k] + j], win [B * K][rows][Ww] -- a copy.
 *   df_window_blend:  out[b][row][c] = (sum_k w(c - starts[k]) * win[b * K + k][row][c - starts[k]]) * inv_n[c] over the windows that
 *     cover column c in ascending k, w(j) = min(j + 1, Ww - j) (an integer tent), inv_n[c] = fp32(1 / sum_k w(c - starts[k])) with the
 *     reciprocal taken in double on the host.  fp32 accumulation from zero, one fma per window, one multiply: no atomics, no scatter,
 *     equal inputs give equal bits.  out must not alias win.
 * The per-column tables of a geometry are built on the host and uploaded with a blocking copy the first time the geometry is seen on a
 * device, then reused (up to 64 geometries are kept).  Stateless otherwise, like df_lincomb. */
int df_window_gather(const float* x_dev, float* win_dev, const int32_t* starts_host, int K, int B, int64_t rows, int Ww, int W,
                     void* stream);
int df_window_blend(const float* win_dev, float* out_dev, const int32_t* starts_host, int K, int B, int64_t rows, int Ww, int W,
                    void* stream);
/* DDIM update (ddim.py:258-272).  noise may be NULL (eta = 0). */
int df_ddim_update(const float* x_dev, const float* e_dev, const float* noise_dev, float* x_prev_dev,
                   float* pred_x0_dev, int64_t n, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at,
                   void* stream);

/* ---- introspection for bench.py / tests --------------------------------------------------------- */
/* Plans (static launch lists + workspaces, one per (network, batch, latent, context) shape) currently cached and the bytes
 * of HBM they own.  The cache is bounded: beyond DF_MAX_PLANS (env, default 32) the least recently used plan is dropped. */
int df_plan_count(df_ctx* ctx, int64_t* n_plans, int64_t* workspace_bytes);
/* Number of kernel launches of the last UNet plan executed and its algorithmic GEMM FLOPs. */
int df_unet_plan_stats(df_ctx* ctx, int64_t* n_launches, double* gemm_flops, double* weight_bytes);
/* Per-op-family HIP-event timing of everything executed between begin and end (events are recorded on the
 * stream the kernels are launched on).  Families: 0 MFMA implicit-GEMM (conv3x3/1x1/linear/batched, incl. split-K
 * reduce), 1 fused attention, 2 GroupNorm, 3 LayerNorm, 4 other (packing, embeddings, sampler arithmetic).
 * ms_by_family / count_by_family: arrays of 5. */
int df_profile_begin(df_ctx* ctx);
int df_profile_end(df_ctx* ctx, double* ms_by_family, int64_t* count_by_family);
/* CSV (tag,M,N,K,taps,stride,ups,batch,tile,splitk,ms) of every op of the region last closed by df_profile_end. */
int df_profile_dump(df_ctx* ctx, const char* path);
/* The autotuner's choices as text ("key tile splitk gm" per line; process-wide).  Export: *n = bytes needed, at most cap are
 * written to buf (buf may be NULL to query the size).  Import merges the lines into this process's cache: plans built with
 * df_autotune(1) whose GEMMs are all present are configured from it without a trial launch.  parallel.broadcast_packed_model
 * ships rank 0's text with the packed blob: every rank runs rank 0's tiles (identical fp32 summation order). */
int df_tune_cache_export(char* buf, int64_t cap, int64_t* n);
int df_tune_cache_import(const char* text, int64_t n);
/* Debug: while enabled, every op of every plan is followed by a 64-bit (order-independent, integer) checksum over ALL
 * workspace bytes of its plan; the sequence of checksums of two runs on identical inputs must be identical, and the first
 * index that differs names the launch that was not reproducible (tools/chk_probe.py).  capacity = checksum slots. */
int df_debug_checksums(df_ctx* ctx, int enable, int64_t capacity);
int df_debug_checksums_read(df_ctx* ctx, uint64_t* out, int64_t cap, int64_t* n);
int df_debug_checksum_label(df_ctx* ctx, int64_t index, char* buf, int64_t len);
/* Debug: while enabled, every op of every plan is followed by a count of the operand-type values it stored that sit at the
 * saturation point of the operand format -- fp16 build: |v| == 65504, where every fp32 -> fp16 conversion of the kernels
 * clamps instead of overflowing (csrc/common.h op_clamp); bf16 build: non-finite values.  Covers the operand-type outputs of
 * every GEMM epilogue (C, the aux copy, the transposed V) and of the norm / cast / attention ops.  A non-zero count means the
 * fp16 build has lost information in that op (a trained checkpoint's activations left the fp16 range): use the bf16 build.
 * The reference computes in fp32 and has no such limit (openai_unetmodel.py:24-28: convert_module_to_f16 is a stub). */
int df_debug_saturations(df_ctx* ctx, int enable, int64_t capacity);
int df_debug_saturations_read(df_ctx* ctx, uint64_t* out, int64_t cap, int64_t* n);
/* Error budget of the bf16 build (tools/error_budget.py; no reference counterpart): in the fp16 build, re-round the operand-type outputs of
 * every op whose tag starts with one of the comma-separated prefixes ("*" = all, "" = off) to bf16's 8 significant bits right behind
 * the op.  The bf16 build accepts the call and changes nothing. */
int df_debug_requant(df_ctx* ctx, const char* tag_prefixes);
int df_debug_saturation_label(df_ctx* ctx, int64_t index, char* buf, int64_t len);
/* Debug: poisoned plan workspaces.  The rule it enforces: an op may read only bytes written earlier in the same run by an op of
 * its plan, or a pinned zeroed block.  While enabled, (i) a workspace block fresh from the allocator is filled with 0xFF bytes (a NaN as
 * fp32, bf16 and fp16) instead of zeros, (ii) every block is filled with the pattern again right behind the last op in front of its
 * release at plan-build time -- whenever that op is among the ops a call executes -- and (iii) the split-K scratch a GEMM may use
 * (splitk * M * N * 4 bytes, x 4 for the four-phase Upsample conv) is filled in front of every split-K GEMM.  An op that relies on the
 * build-time zeros, on a previous tenant's bytes or on its own buffer after the release then produces NaN instead of a slightly wrong
 * number.  The fills are hipMemsetAsync calls on the stream of the run, in op order.  Off (the default), nothing changes.  Switching
 * drops the context's cached plans (what a block holds when a plan is built changes); refused while df_autotune is on, and
 * df_autotune(1) is refused while this is on: the tuner re-runs ops out of plan order. */
int df_debug_poison(df_ctx* ctx, int enable);
/* Self-test of df_debug_poison (tests/test_plan_poison_gpu.py): a four-op plan of element-wise launches over Plan::alloc / release
 * blocks, on the fixed input x[i] = ((i % 37) - 18) / 8, i < 1024.  out_dev [512] fp32.
 *   ops: A = 2 x [1024] ; B = A + x [1024], A released ; C = B / 2 [512], which recycles A's (twice as large) block ;
 *        out[i] = C[i] + B[512 + i] = 1.5 x[i] + 3 x[512 + i]
 *   defect 0: that plan.  defect 1 (use after release): the last op reads A[512 + i] for B[512 + i] -- the tail of the block that was
 *   released behind op 1 and handed to C.  defect 2 (stale tail): op 2 adds C[512 + i], the tail of its oversized recycled block that
 *   it never wrote, to C[i].  Both defects stay inside A's block, give finite (wrong) numbers with the hook off and NaN with it on. */
int df_test_poison_selftest(df_ctx* ctx, int defect, float* out_dev, void* stream);
/* Run ONE op family in isolation for unit tests (see tests/test_kernels_gpu.py). */
int df_test_scratch_read(void* host, int64_t bytes);     /* the shared scratch of the test entry points (debug stamps) */
/* df_test_gemm, _gemm_epi, _gemm_dual, df_test_conv3x3, _conv3x3_skip, _conv3x3_ups4 and df_test_geglu are fixed-shape fills of
 * the df_test_gemm_desc below, run through the one path of df_test_gemm_ex: K (convs: Cin too) must be a multiple of 64, and a refusal
 * of the launch reads "launch_gemm refused ...: invalid argument (the rule that refuses)": launch_gemm itself refuses whatever cannot
 * run (csrc/gemm.h gemm_route), on the host, before anything is launched.  _gemm_epi, _gemm_dual, _conv3x3_skip, _conv3x3_ups4 and
 * df_test_geglu also apply the tuner's split policy ("tile T / split-K S refused this problem"); df_test_gemm and df_test_conv3x3 do
 * not, like df_test_gemm_ex -- they also take GemmParams::dbg from the environment (DF_GEMM_DBG; bit 6: per-block clock stamps).
 * df_test_geglu: the LayerNorm-folded GEGLU projection (stats [M][K/64] float2, cs / bias [N1], out operand type [M][N1/2]); dbg goes
 * to GemmParams::dbg except bit 7, which keeps the wide tiles' 320-column packing made from the same W by the previous call. */
int df_test_geglu(const uint16_t* A_dev, const uint16_t* W_dev, const void* stats_dev, const float* cs_dev, const float* bias_dev,
                  uint16_t* out_dev, int M, int K, int N1, int tile, int dbg, void* stream);
int df_test_conv3x3_fewout(const uint16_t* A_nhwc_dev, const uint16_t* W_okki_dev, const float* bias_dev, float* out_nchw_dev, int NB,
                           int H, int W, int Cin, int Cout /* <= 4 */, void* stream);
/* The VAE encoder's conv_in kernel alone (csrc/elementwise.hip conv3x3_fewin; model.py:479-483): x NCHW fp32 [NB][Cin <= 4][H][W],
 * W OIHW fp32, out fp32 rows [NB*H*W][ldo >= Cout]. */
int df_test_conv3x3_fewin(const float* x_nchw_dev, const float* W_oihw_dev, const float* bias_dev, float* out_dev, int ldo, int NB,
                          int H, int W, int Cin, int Cout, void* stream);
/* The same conv through the route the dedicated kernel replaces (tools/vae_encode_bench.py): pack to 64 operand-type channels
 * (xpad [NB*H*W][64], wpad [Cout][9][64] scratch), then the implicit GEMM on the builder's own tile choice. */
int df_test_conv3x3_fewin_gemm(const float* x_nchw_dev, const float* W_oihw_dev, const float* bias_dev, float* out_dev,
                               uint16_t* xpad_dev, uint16_t* wpad_dev, int NB, int H, int W, int Cin, int Cout, void* stream);
/* df_vae_encode of B samples with ONE intermediate tensor copied out as it is produced (tests: the hooked stages of the reference's
 * Encoder.forward, model.py:529-554): tap 0 = conv_in's output, tap 1 + l = the Downsample output of level l, tap 100 = mid.block_2's
 * output; tap_out fp32 NHWC rows [B*h*w][C] of that stage.  A plan of its own per tap (the copy stands between a GEMM and the GroupNorm
 * that otherwise takes over its split-K reduce: same arithmetic, possibly another summation order); B within one slice of df_vae_encode. */
int df_test_vae_encode_tap(df_ctx* ctx, const float* x_dev, float* moments_dev, float* tap_out_dev, int tap, int B, int H, int W,
                           void* stream);
/* Stride-2 3x3 conv with GemmParams::pad = pad: 1 = the symmetric Downsample of the UNet (df_test_conv3x3 with stride 2), 0 = the VAE
 * encoder's F.pad(x, (0,1,0,1)) + padding-0 conv (model.py:167-171).  A [NB][H][W][Cin] and W [Cout][3][3][Cin] operand type, C fp32
 * [NB*(H/2)*(W/2)][Cout].  _valid: 1 when gemm_route accepts (tile, splitk) for this problem, else 0 (host only). */
int df_test_conv3x3_down(const uint16_t* A_dev, const uint16_t* W_dev, const float* bias_dev, float* C_dev, int NB, int H, int W,
                         int Cin, int Cout, int pad, int tile, int splitk, void* stream);
int df_test_conv3x3_down_valid(int NB, int H, int W, int Cin, int Cout, int pad, int tile, int splitk);
int df_test_gemm_epi(const uint16_t* A_dev, const uint16_t* W_dev, const float* bias_dev, const float* res_dev, void* C_dev,
                     int M, int N, int K, int act /*0 none, 1 SiLU, 2 ReLU*/, int out_operand, int tile, int splitk,
                     void* stream);
int df_test_gemm_dual(const uint16_t* A_dev, const uint16_t* A2_dev, const uint16_t* W_dev, float* C_dev, int M, int N, int K1,
                      int K2, int tile, int splitk, void* stream);
int df_test_gemm(const uint16_t* A_dev, const uint16_t* W_dev, float* C_dev, int M, int N, int K, int tile, int splitk,
                 void* stream);
/* SpatialTransformer GEMM pair: producer (fp32 t0 + operand copy + per-row partial statistics from the epilogue) and
 * LayerNorm-folded consumer (attention_openai.py:211-215 pre-norms never run as kernels).  mode 0 plain fp32 out,
 * 1 GEGLU, 2 fused QKV with the V third stored transposed per sample of T rows. */
int df_test_ln_chain(const uint16_t* A0_dev, const uint16_t* W0_dev, const float* b0_dev, const float* res_in_dev,
                     const float* gamma_dev, const float* beta_dev, const float* W1_dev, const float* b1_dev,
                     float* t0_dev, void* y_dev, uint16_t* vt_dev, int M, int C, int N1, int mode, int T, int ldvt,
                     int tile0, int sk0, int tile1, int sk1, void* stream);
/* Small-M weight-streaming linear (classifier head, classifier-gradient time MLP, CAVP head): out = act(a W^T + bias),
 * act 0 none, 1 SiLU, 2 sigmoid. */
int df_test_linear_rows(const float* a_dev, int lda, const uint16_t* W_dev, const float* bias_dev, float* out_dev, int ldo,
                        int M, int N, int K, int act, void* stream);
/* ONE block of the loaded UNet in isolation (checked against the reference's per-block tensors, golden G3): kind 0
 * ResBlock (openai_unetmodel.py:255-275; semb = SiLU(time_embed(t))), 1 SpatialTransformer (attention_openai.py:250-261),
 * 2 Downsample, 3 Upsample.  x [N*H*W][Cin] -> out [N*OH*OW][Cout], NHWC fp32; prefix e.g. "input_blocks.1.0". */
int df_test_unet_block(df_ctx* ctx, const char* prefix, int kind, const float* x_dev, const float* semb_dev,
                       const float* context_dev, float* out_dev, int N, int H, int W, int Cin, int Cout, int T, void* stream);
int df_test_conv3x3(const uint16_t* A_dev, const uint16_t* W_dev, const float* bias_dev, float* C_dev, int NB, int H,
                    int W, int Cin, int Cout, int stride, int ups, int tile, int splitk, void* stream);
/* conv3x3 (stride 1) with a folded 1x1 skip connection: C = conv3x3(A; W[:, :9 Cin]) + A2 . W[:, 9 Cin:]^T + bias, one implicit GEMM
 * with K = 9 Cin + Cin2 (A [NB*H*Wd][Cin], A2 [NB*H*Wd][Cin2], W [Cout][9 Cin + Cin2] operand type; Cin, Cin2 multiples of 64). */
int df_test_conv3x3_skip(const uint16_t* A_dev, const uint16_t* A2_dev, const uint16_t* W_dev, const float* bias_dev, float* C_dev,
                         int NB, int H, int W, int Cin, int Cin2, int Cout, int tile, int splitk, void* stream);
/* nearest-x2 upsample + conv3x3 in the phase-decomposed form (four 2x2-tap convs on the input-resolution map, per-phase
 * weights = sums of the 3x3 taps): A [NB*H*Wd][Cin] operand type, W_oihw fp32 [Cout][Cin][3][3], w4_scratch 16*Cout*Cin
 * operand-type elements, C fp32 [NB*2H*2Wd][Cout]. */
int df_test_conv3x3_ups4(const uint16_t* A_dev, const float* W_oihw_dev, const float* bias_dev, float* C_dev, uint16_t* w4_scratch_dev,
                         int NB, int H, int Wd, int Cin, int Cout, int tile, int splitk, void* stream);
int df_test_groupnorm(const float* x_dev, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps,
                      int silu, uint16_t* out_dev, void* stream);
/* GroupNorm whose input is the not-yet-reduced output of its own split-K producer: channels [0, c_own) of x are summed from
 * `nslab` fp32 slabs [N*HW][c_own] (consecutive), + bias[c_own] + res[N*HW][ldr] (either may be NULL), written back to x and
 * normalised together with channels [c_own, C) read from x. */
int df_test_groupnorm_own_slabs(float* x_dev, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps,
                                int silu, uint16_t* out_dev, const float* slabs_dev, int nslab, int c_own,
                                const float* bias_dev, const float* res_dev, int ldr, void* stream);
/* Host only, no GPU work: the kernel form a shape takes, from the function the launcher itself dispatches on.
 * df_test_groupnorm_form: PER of the register kernel (1, 2, 3, 4, 6, 8, 12, 16, 20), -1 streaming kernel, -2 chunked three-launch
 * form, -3 refused; nslab > 0 = either slab mode.  df_test_attention_form: waves * 16 + 32-key sub-tiles per iteration (66 =
 * <D,4,2>, 65 = <D,4>, 33 = <D,2>, 17 = <D,1>), 0 = head dim not supported. */
int df_test_groupnorm_form(int N, int HW, int C, int nslab);
int df_test_attention_form(int D, int Tq, int Tk);
/* GroupNorm with every leading dimension free, in its three input modes.  out / raw_out (nullable: the input cast to the operand
 * type) are [N*HW][ldo].  nslab == 0: plain input x [N*HW][ld].  nslab > 0, own_slabs NULL: x is the first of nslab fp32 slabs
 * [N*HW][ld], slab_stride floats apart, + bias[C] + rowbias[N][ld_rowbias] (nullable).  own_slabs non-NULL: as
 * df_test_groupnorm_own_slabs (slabs [N*HW][c_own], slab_stride apart; res [N*HW][ldr]). */
int df_test_groupnorm_ex(float* x_dev, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps, int silu,
                         uint16_t* out_dev, int ldo, uint16_t* raw_out_dev, int nslab, int64_t slab_stride, const float* bias_dev,
                         const float* rowbias_dev, int ld_rowbias, const float* own_slabs_dev, int c_own, const float* res_dev,
                         int ldr, void* stream);
/* x fp32 [rows][C] -> operand type [rows][C], C = 64 .. 2048 in steps of 64; _ex: x rows are ld >= C floats apart */
int df_test_layernorm(const float* x_dev, int rows, int C, const float* gamma, const float* beta, uint16_t* out_dev,
                      void* stream);
int df_test_layernorm_ex(const float* x_dev, int ld, int rows, int C, const float* gamma, const float* beta, uint16_t* out_dev,
                         void* stream);
int df_test_attention(const uint16_t* Q, int ldq, const uint16_t* K, int ldk, const uint16_t* Vt, int ldvt, uint16_t* O,
                      int ldo, int N, int heads, int D, int Tq, int Tk, float scale, void* stream);
/* The classifier's input-gradient kernels one at a time (csrc/backward.hip).  Nullable: addend, dx_b16 (its rows are C wide). */
int df_test_groupnorm_bwd(const float* x_dev, int ld, int N, int HW, int C, const float* gamma, const float* beta, float eps,
                          int silu, const float* dy_dev, int lddy, const float* addend_dev, int ldadd, float* dx_dev, int lddx,
                          uint16_t* dx_b16_dev, void* stream);
int df_test_layernorm_bwd(const float* x_dev, int rows, int C, const float* gamma, float eps, const float* dy_dev,
                          const float* addend_dev, float* dx_dev, uint16_t* dx_b16_dev, void* stream);
/* u = [x | gate] operand-type [rows][2H]; fwd: y = x * gelu(gate) [rows][H]; bwd: du = [dy gelu(g) | dy x gelu'(g)] [rows][2H] */
int df_test_geglu_fwd(const uint16_t* u_dev, uint16_t* y_dev, int64_t rows, int H, void* stream);
int df_test_geglu_bwd(const uint16_t* u_dev, const float* dy_dev, uint16_t* du_dev, int64_t rows, int H, void* stream);
/* form: -1 the production choice, 0 MFMA, 1 VALU LDS-resident, 2 tiled pair; a forced form that does not take the shape fails.
 * dK == NULL: dQ only (cross attention). */
int df_test_attention_bwd(const uint16_t* Q, int ldq, const uint16_t* K, int ldk, const uint16_t* Vt, int ldvt, const float* dO,
                          int lddo, uint16_t* dQ, int lddq, uint16_t* dK, int lddk, uint16_t* dV, int lddv, int N, int heads, int D,
                          int Tq, int Tk, float scale, int form, void* stream);
int df_test_cls_head_bwd(const float* prob_dev, const float* w_dev, float* dh_dev, uint16_t* dh_b16_dev, int N, int HW, int C, int Cp,
                         void* stream);
int df_test_pack_linear_t(const float* w_dev, uint16_t* out_dev, int O, int I, int ldo, int off, void* stream);
int df_test_pack_conv_bwd(const float* w_dev, uint16_t* out_dev, int O, int I, int Opad, void* stream);
/* Backward-data of a pad-1 3x3 conv as the classifier gradient runs it: dY [NB][OH][OW][rup(O, 64)] (pad columns zero), stride 1
 * or 2 (zero-stuffed); W fp32 OIHW is packed into w_scratch (I * 9 * rup(O, 64) elements); dX fp32 [NB][H][W][I], dX_op nullable. */
int df_test_conv3x3_bwd_data(const uint16_t* dY_dev, const float* W_oihw_dev, uint16_t* w_scratch_dev, float* dX_dev,
                             uint16_t* dX_op_dev, int NB, int H, int Wd, int I, int O, int stride, int tile, int splitk,
                             void* stream);
/* The packing, casting, pooling and data-movement kernels one at a time: each entry is its launcher (csrc/kernels.h documents
 * the layouts).  2-byte buffers hold the build's operand type. */
int df_test_softmax_rows(const float* s_dev, uint16_t* p_dev, int rows, int T, int ldp, void* stream);
int df_test_timestep_embedding(const float* t_dev, float* out_dev, int N, int dim, void* stream);
int df_test_timestep_embedding_b16(const float* t_dev, int t_B, uint16_t* out_dev, int N, int dim, void* stream);
int df_test_pack_latent(const float* x_dev, uint16_t* out_dev, int B, int C, int HW, int cpad, int rep, float in_scale,
                        const float* wpq_dev, const float* bpq_dev, void* stream);
int df_test_pack_latent_bcast(const float* x_dev, uint16_t* out_dev, int B, int C, int HW, int cpad, int rep, const float* src_dev,
                              float* dst_dev, int rows, int n, void* stream);
int df_test_bcast_rows(const float* src_dev, float* dst_dev, int rows, int n, void* stream);
int df_test_cast_bf16(const float* x_dev, uint16_t* out_dev, int64_t n, void* stream);
int df_test_cast_bf16_2d(const float* x_dev, int ld, uint16_t* out_dev, int64_t rows, int C, void* stream);
int df_test_avgpool(const float* x_dev, float* out_dev, int N, int HW, int C, void* stream);
int df_test_pack_conv_weight(const float* w_dev, uint16_t* out_dev, int O, int I, int KH, int KW, int Ipad, void* stream);
int df_test_pack_conv_skip(const float* w_dev, const float* ws_dev, uint16_t* out_dev, int O, int I, int I2, void* stream);
int df_test_pack_geglu(const float* w_dev, const float* b_dev, uint16_t* wout_dev, float* bout_dev, int half_rows, int K, void* stream);
int df_test_pack_ln_linear(const float* w_dev, const float* bias_dev, const float* gamma_dev, const float* beta_dev, uint16_t* wout_dev,
                           float* cs_dev, float* bb_dev, int rows, int K, int row_off, int geglu_half, void* stream);
int df_test_grad_scale_per_sample(float* x_dev, const float* prob_dev, int N, int64_t per, void* stream);
int df_test_stem_im2col(const float* x_dev, uint16_t* out_dev, int F, int H, int W, int OH, int OW, int KP, void* stream);
int df_test_maxpool3x3s2(const uint16_t* x_dev, uint16_t* out_dev, int F, int H, int W, int OH, int OW, int C, void* stream);
int df_test_subsample2(const uint16_t* x_dev, uint16_t* out_dev, int F, int H, int W, int C, void* stream);
int df_test_tcat3(const uint16_t* x_dev, uint16_t* out_dev, int F, int T, int HW, int C, void* stream);
int df_test_pack_conv3d_bn(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev, const float* var_dev,
                           float eps, uint16_t* out_dev, float* bias_dev, int O, int I, int KT, int KH, int KW, int KP, void* stream);
int df_test_maxpool_time(const float* x_dev, float* out_dev, int B, int T, int C, int k, void* stream);
int df_test_l2norm_rows(float* x_dev, int rows, int C, void* stream);
/* The spectrogram tower's own kernels one at a time (csrc/cavp_spec.hip; csrc/kernels.h documents the layouts).  bn0 / bn1: four
 * device pointers each, {weight, bias, running_mean, running_var}, passed as host arrays of pointers. */
int df_test_spec_conv_in(const float* spec_dev, const float* const* bn0, const float* w_dev, const float* const* bn1, float eps,
                         uint16_t* out_dev, int ldo, int B, int n_mels, int T, int C1, void* stream);
int df_test_avgpool_nhwc(const float* x_dev, int ldx, uint16_t* out_dev, int ldo, int B, int H, int W, int C, int ph, int pw,
                         void* stream);
int df_test_spec_head_pool(const float* x_dev, int ldx, uint16_t* out_dev, int ldo, int B, int T, int W, int C, void* stream);
/* df_cavp_spec_encode of B clips (one slice) with ONE ConvBlock's output copied out as the plan holds it (tests: the hooked stages of
 * Cnn14.forward): tap 1 .. 5 = conv_block<tap> behind its pool, operand type NHWC [B][h][w][C]; tap 6 = conv_block6, fp32 NHWC (its
 * (1, 1) pool is the identity).  A plan of its own per tap. */
int df_test_cavp_spec_tap(df_ctx* ctx, const float* spec_dev, float* out_dev, void* tap_out_dev, int tap, int B, int n_mels, int T,
                          int normalize, void* stream);
/* One GEMM with any GemmParams epilogue (csrc/gemm.h) switched on, on a caller-chosen (tile, split-K, batch, gm): the tests of the
 * autotuner's search space.  `size` must be sizeof(df_test_gemm_desc).  Geometry: conv == 0 linear, A [M][lda] (lda 0 = K);
 * conv == 1 a pad-1 3x3 conv, A NHWC [NB][H][Wd][Cin], W [N][9][Cin], M = NB * OH * OW.  Null / zero fields are off.  ldc 0 = N.
 * defer_reduce (split-K only): the slabs are left for a consumer; when slabs_out is given they are copied there,
 * [splitk][M][N] fp32.  Refusals of launch_gemm are reported as "launch_gemm refused ..." through df_last_error. */
typedef struct df_test_gemm_desc {
  int64_t size;
  const void* A; const void* W; void* C;
  int M, N, K, lda, ldc, out_operand;
  int conv, NB, H, Wd, Cin, stride;
  int batch, tile, splitk, gm;
  int64_t a_bs, w_bs, c_bs, res_bs;
  float alpha;
  const float* bias;
  const float* rowbias; int ld_rowbias, rows_per_sample, rowbias_mode;
  const float* res; int ldr;
  int relu, silu;
  void* aux; int ld_aux;
  void* stats; int stats_slots;                 /* float2 [rows][stats_slots] */
  const void* ln_stats; int ln_slots, ln_C; float ln_eps; const float* ln_cs;
  int w_rows, sm_w, sm_valid;
  int dup_rows, no_c_store, store_nchw, hw_out;
  float* cfg_out; float cfg_scale;
  int defer_reduce; float* slabs_out;
  /* operand side.  conv == 1 with ups (+ zstuff): the conv runs on the nearest-x2 (zero-stuffed) input, M = NB * 2H * 2Wd.
   * conv == 2: the phase-decomposed upsample conv, W the packed [2][2][N][2][2][Cin] operand, M = NB * H * Wd rows of the GEMM
   * (C holds the 2H x 2Wd map).  A2 / lda2 / Cin2: a second operand tensor for the last Cin2 K columns -- conv: the folded 1x1
   * skip, K = 9 Cin + Cin2; linear: K = K + Cin2 (d->K counts A's columns only).  geglu: (32 x | 32 gate) column groups, output
   * width N / 2; the wide tiles' 320-column packing is made inside the entry on every call.  vt: columns >= vt_col0 are stored
   * transposed per sample of vt_T rows, [M / vt_T][N - vt_col0][ldvt] operand type. */
  int ups, zstuff;
  const void* A2; int lda2, Cin2;
  int geglu;
  void* vt; int vt_col0, vt_T, ldvt;
} df_test_gemm_desc;
int df_test_gemm_ex(const df_test_gemm_desc* d, void* stream);
/* gemm_tile_valid(d, tile, batch, splitk): 1 / 0, or -1 (message in df_last_error) for a malformed descriptor.  Host only.
 * 1 exactly when df_test_gemm_why returns 0. */
int df_test_gemm_valid(const df_test_gemm_desc* d, int tile, int batch, int splitk);
/* Why: 0 = launch_gemm runs it and the tuner would try it; 1 = it runs, but the split is outside the tuner's policy (too few K steps
 * per slab to be worth timing); 2 = launch_gemm refuses it, the rule NUL-terminated (truncated) into buf[n] (buf may be null);
 * -1 = malformed descriptor (message in df_last_error).  Host only. */
int df_test_gemm_why(const df_test_gemm_desc* d, int tile, int batch, int splitk, char* buf, int n);
/* The tune-cache key of the descriptor's GEMM (csrc/engine_tune.hip tune_key: M_N_K_taps_stride_ups_batch_geglu_eEPI; the deferred-reduce
 * bit from d->defer_reduce), NUL-terminated into buf[n].  Returns 0, or -1 (message in df_last_error).  Host only. */
int df_test_gemm_key(const df_test_gemm_desc* d, int batch, char* buf, int n);
/* Row `tile` of the GEMM tile table (csrc/gemm_tiles.def): what a tile id of the plan tables and tune caches means.  `size` must be
 * sizeof(df_test_gemm_tile).  family: 0 generic, 1 halo conv, 2 producer-specialised, 3 persistent GEGLU, 4 wide GEGLU, 5 retired
 * (id reserved, never valid).  dma_threads: the threads that issue DMA requests; ring: depth of the LDS operand rings (halo: of the
 * weight ring); modes: bit m set = built for MODE m (0 linear, 1 conv s1, 2 conv s2 / upsampled, 3 phase-upsample).  Returns
 * non-zero for an id outside the table (ids are 0 .. count-1 without gaps).  Host only. */
typedef struct df_test_gemm_tile {
  int64_t size;
  const char* name;
  int family, bm, bn, dma_threads, ring, modes;
} df_test_gemm_tile;
int df_test_gemm_tile_info(int tile, df_test_gemm_tile* out);
/* The launch constants launch_gemm hands a GEMM-family kernel for (d, tile, batch, splitk): csrc/gemm.h GemmLaunch (the kernels'
 * prologues divide by nothing; these are the quotients, the multiply-high magic numbers -- x / d == umulhi(x, mul) >> sh, d == 1: x --
 * and the FastDiv reciprocals 1.0f / (float)divisor they read), + the halo tiles' patch th x tw.  magic[]: by the tiles of a full row
 * group (gm nbn), by gm, by the M tiles of the last row group, by w_rows / BM (d 0 = off), by OH OW, by OW, by Cin.  `size` must be
 * sizeof(df_test_gemm_launch).  Returns 0, 2 when launch_gemm refuses the problem, -1 for a malformed descriptor (message in
 * df_last_error either way).  Host only. */
typedef struct df_test_gemm_launch {
  int64_t size;
  int nbm, nbn, nblk, xq, xr, gm;
  struct { uint32_t mul; int sh, d; } magic[7];
  int nk, kper, n2tot, used, per2;
  int HWp, PPX, PB, HR, APASS, npx, npy, pimg, npatch;
  float inv_hwp, inv_tw2, inv_pimg, inv_npx, inv_ppx, inv_tw;
  int th, tw;
} df_test_gemm_launch;
int df_test_gemm_launch_constants(const df_test_gemm_desc* d, int tile, int batch, int splitk, df_test_gemm_launch* out);
/* The folded cross-attention of one SpatialTransformer (engine_builder.hip context_px, st.xs, st.xo), every intermediate out: ctx [NB*Tc][Dc]
 * and Wkv [2C][Dc] (to_k | to_v) operand type; Wq [C][C], gamma (norm2), bq = Wq . beta fp32; Wo [C][C] operand, bo fp32; x fp32
 * [NB*T][C], xb its operand copy, xstats float2 [NB*T][C/64] (sum, sum of squares per 64 columns).  Outputs: kv [NB*Tc][2C],
 * Kexp / Vexp [NB][H*32][C], WqT [C][C], G [NB][H*32][C], cs / bb [NB][H*32], Vo [NB][C][H*32], P [NB*T][H*32], out fp32 [NB*T][C]. */
int df_test_xattn_chain(const uint16_t* ctx_dev, const uint16_t* Wkv_dev, const float* Wq_dev, const float* gamma_dev,
                        const float* bq_dev, const uint16_t* Wo_dev, const float* bo_dev, const float* x_dev, const uint16_t* xb_dev,
                        const void* xstats_dev, int NB, int T, int Tc, int Dc, int C, int heads, uint16_t* kv_dev, uint16_t* Kexp_dev,
                        uint16_t* Vexp_dev, uint16_t* WqT_dev, uint16_t* G_dev, float* cs_dev, float* bb_dev, uint16_t* Vo_dev,
                        uint16_t* P_dev, float* out_dev, int tile_xs, int tile_xo, void* stream);
/* [Wp.W2 | Wp] operand [C][F + C] and bias Wp.b2 + bp (FeedForward's second Linear merged with proj_out). */
int df_test_pack_ffproj(const float* Wp_dev, const float* bp_dev, const float* W2_dev, const float* b2_dev, uint16_t* wout_dev,
                        float* bout_dev, int C, int F, void* stream);
/* Device-peak microbenchmarks (tools/peaks.py; SURVEY.md 8d "peaks measured on the box").  kind 0: MFMA issue peak
 * (n = iterations per wavefront of 4 independent v_mfma_f32_32x32x16_bf16; grid blocks x 256 threads); kind 1:
 * streaming copy of n bytes; kind 2: streaming read of n bytes. */
int df_test_peak(int kind, const void* src_dev, void* dst_dev, size_t n, int blocks, void* stream);
/* L2 -> CU fill-rate probes: kind 3 LDS-DMA, 4 global_load_dwordx4 -> VGPR, 5 global_load + ds_write_b128.  Every block
 * re-reads its span-byte window n times; stride_blk bytes between the windows of consecutive blocks. */
int df_test_fill(int kind, const void* src_dev, void* dst_dev, size_t span, size_t stride_blk, int n, int blocks,
                 void* stream);


#ifdef __cplusplus
}
#endif
#endif /* DF_ENGINE_H */

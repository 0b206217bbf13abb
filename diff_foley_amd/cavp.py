"""CAVPInference (the reference's ``CAVP_Inference``): the video tower that feeds Stage-2 sampling and the spectrogram tower that scores
generated audio against its video.  Also importable from ldm.py, where ``instantiate_from_config`` maps the reference's target path to
it."""
import torch

from .model_base import _EngineModel, _check_shapes


class CAVPInference(_EngineModel):
    """Mirror of the reference ``CAVP_Inference`` (inference/model/cavp_model.py:9-96), both towers in libdfengine.so:
    ``encode_video`` = SlowOnly-R50 backbone + ``video_project_head`` (df_cavp_encode; what Stage-2 inference uses, Extract_CAVP_Features,
    inference/demo_util.py:80-170) and ``encode_spec`` = Cnn14 + ``final_project`` (df_cavp_spec_encode), the tower that reads the
    normalised log-mel ``decode_first_stage(z)[:, 0]`` and ``wave_to_mel`` produce.  The spectrogram tower is kept when the state dict
    holds its complete key set (synth.cavp_audio_spec); ``alignment_scores`` ranks generated candidates against a video with the two."""

    _buffer_names = ()          # no schedule; and no range probe: the operand type is the caller's choice alone
    _not_ready = ("CAVPInference: call load_state_dict() and .cuda() first (the encoder runs in libdfengine.so on a ROCm GPU; there is "
                  "no CPU fallback)")

    def __init__(self, video_encode="Slowonly_pool", spec_encode="cnn14_pool", embed_dim=512, video_pretrained=False,
                 audio_pretrained=False, stage_blocks=(3, 4, 6, 3), spec_channels=(64, 128, 256, 512, 1024, 2048), spec_fc_dim=2048,
                 spec_n_mels=128, precision=None, **ignored):
        if video_encode != "Slowonly_pool":
            raise NotImplementedError("only video_encode='Slowonly_pool' exists in the reference (cavp_model.py:25)")
        if spec_encode != "cnn14_pool":
            raise NotImplementedError("only spec_encode='cnn14_pool' exists in the reference (cavp_model.py:35)")
        if len(spec_channels) != 6:
            raise ValueError(f"spec_channels: Cnn14 has six ConvBlocks, got {len(spec_channels)} widths")
        self.cfg = dict(stage_blocks=[int(v) for v in stage_blocks], base_channels=64, embed_dim=int(embed_dim))
        # the reference builds Cnn14(embed_dim=512) whatever CAVP_Inference's embed_dim is (cavp_model.py:36); the two agree at 512
        self.spec_cfg = dict(n_mels=int(spec_n_mels), channels=[int(v) for v in spec_channels], fc_dim=int(spec_fc_dim),
                             embed_dim=int(embed_dim))
        super().__init__(precision)
        self._spec_state = None           # the spectrogram tower's tensors, when the state dict held all of them
        self._spec_missing = []
        self.logit_scale = None

    def load_state_dict(self, state_dict, strict=False):
        keep = ("video_encoder.", "video_project_head.")
        self._state = {k: v for k, v in state_dict.items() if k.startswith(keep) and "num_batches_tracked" not in k}
        from . import synth
        _check_shapes(self._state, synth.cavp_spec(self.cfg), "CAVPInference")
        # the spectrogram tower is kept when the state dict holds its COMPLETE key set (the rule the VAE encoder follows in
        # LatentDiffusion.load_state_dict); with any key missing it is dropped, and its keys are reported as unexpected, as before
        aspec = synth.cavp_audio_spec(self.spec_cfg)
        self._spec_missing = [k for k in aspec if k not in state_dict]
        has_spec = not self._spec_missing
        self._spec_state = None
        self.logit_scale = None
        if has_spec:
            self._spec_state = {k: state_dict[k] for k in aspec if k != "logit_scale"}
            _check_shapes(self._spec_state, aspec, "CAVPInference")
            self.logit_scale = state_dict["logit_scale"].detach().to(torch.float32).reshape(()).cpu()
        missing = [] if self._state else ["video_encoder.*"]
        unexpected = [k for k in state_dict if not k.startswith(keep) and not (has_spec and k in aspec)
                      and not (has_spec and k.startswith("spec_encoder.") and k.endswith("num_batches_tracked"))]
        if self.engine is not None:
            self._upload()
        return missing, unexpected

    def _upload(self):
        self.engine.config_cavp(self.cfg)
        for k, v in self._state.items():
            self.engine.load_tensor("cavp." + k, v)
        if self._spec_state is not None:
            self.engine.config_cavp_spec(self.spec_cfg)
            for k, v in self._spec_state.items():
                self.engine.load_tensor("cavp." + k, v)
        self.engine.finalize()

    @torch.no_grad()
    def encode_video(self, video, normalize=False, train=False, pool=True):
        """video (B,T,3,H,W) -> (B,T,embed_dim) for pool=False (cavp_model.py:47-65; what Stage-2 inference calls,
        demo_util.py:161); pool=True adds the contrastive head's MaxPool1d(16) over the frames before the optional normalisation
        (cavp_model.py:58-59): (B, embed_dim) for 16..31 frames."""
        if pool:
            return self._require().cavp_encode_pooled(video, normalize=normalize)
        return self._require().cavp_encode(video, normalize=normalize)

    def _require_spec(self):
        eng = self._require()
        if self._spec_state is None:
            miss = self._spec_missing or ["spec_encoder.*"]
            raise NotImplementedError(f"CAVPInference: the spectrogram tower was not loaded -- the state dict lacks {len(miss)} of its "
                                      f"keys ({', '.join(miss[:3])}{' ...' if len(miss) > 3 else ''})")
        return eng

    @torch.no_grad()
    def encode_spec(self, spec, normalize: bool = False, pool=True):
        """spec (B, n_mels, T) normalised log-mel -> (B, T // 16, embed_dim) for pool=False (cavp_model.py:68-84); pool=True adds the
        contrastive head's MaxPool1d(16) over the rows before the optional normalisation, under encode_video's rule (Engine.cavp_pool):
        refused below one 16-row window (T < 256), NotImplementedError for normalize=True over more than one window, (B, embed_dim)
        for one window."""
        eng = self._require_spec()
        if not pool:
            return eng.cavp_spec_encode(spec, normalize=normalize)
        return eng.cavp_pool(eng.cavp_spec_encode(spec, normalize=False), normalize, "encode_spec", "feature rows")

    @torch.no_grad()
    def forward(self, video, spec, output_dict=True):
        """cavp_model.py:87-96: both towers pooled and normalised, and exp(logit_scale)."""
        self._require_spec()
        video_features = self.encode_video(video, normalize=True)
        spec_features = self.encode_spec(spec, normalize=True)
        scale = self.logit_scale.exp().to(video_features.device)
        if output_dict:
            return {"video_features": video_features, "spec_features": spec_features, "logit_scale": scale}
        return video_features, spec_features, scale

    __call__ = forward

    @torch.no_grad()
    def alignment_scores(self, video_feat, spec):
        """(Bv, Bs) agreement of audio candidates with videos: ``video_feat`` (Bv, T', D) frame features (encode_video(normalize=True,
        pool=False)), ``spec`` either mels (Bs, n_mels, T) -- encoded here with normalize=True, pool=False -- or their features
        (Bs, T', D).  scores[i, j] = mean over the frames of <video_feat[i, t], spec_feat[j, t]> (df_cavp_similarity, scale 1): with
        normalised rows, the mean cosine.  ``scores.argmax(1)`` is the best candidate for each video."""
        eng = self._require()
        if video_feat.ndim != 3:
            raise RuntimeError(f"alignment_scores: video_feat must be (Bv, T', D), got shape {tuple(video_feat.shape)}")
        if spec.ndim != 3:
            raise RuntimeError(f"alignment_scores: spec must be mels (Bs, n_mels, T) or features (Bs, T', D), got shape {tuple(spec.shape)}")
        # features have the video features' (T', D); anything else is a mel (a (Bs, 128, 512) mel also has 512 columns, but 128 rows)
        is_feat = tuple(spec.shape[1:]) == tuple(video_feat.shape[1:])
        if not is_feat and spec.shape[1] != self.spec_cfg["n_mels"] and spec.shape[2] == video_feat.shape[2]:
            is_feat = True            # features of another length: the frame-count check below names the mismatch
        sf = spec if is_feat else self.encode_spec(spec, normalize=True, pool=False)
        if sf.shape[1] != video_feat.shape[1]:
            raise RuntimeError(f"alignment_scores: the audio gives {sf.shape[1]} feature rows, the video has {video_feat.shape[1]} frames "
                               "(a 4 fps video pairs with 64 mel frames per video frame)")
        return eng.cavp_similarity(video_feat, sf, 1.0)

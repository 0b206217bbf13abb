#!/usr/bin/env python
"""Score a folder of generated mels with the paper's Align-Acc metric (the reference's evaluation/align_acc.py) on the GPU.

    python tools/align_acc.py --config eval_classifier.yaml --ckpt eval_classifier.ckpt --specs GENERATED_DIR --feats CAVP_FEAT_DIR

--config   evaluation/config/eval_classifier.yaml; its ``model.target`` may name the reference class or diff_foley_amd's.  The dataset's
           fps / truncate / sr are taken from ``data_eval_metric.params.validation.params`` when the file has them (4 / 131072 / 16000).
--ckpt     eval_classifier.ckpt (``state_dict`` inside, or the state dict itself)
--specs    folder of ``*.npy`` one-channel mels (n_mels, T): cut to 512 columns and repeated to 3 channels (evaluation/dataset.py:99-107)
--feats    folder of ``<name>.npz`` with key ``feat`` (rows, 512); <name> is the mel's file name with its last two ``_`` fields
           dropped (dataset.py:36), rows [0, int(fps * truncate / sr)) are kept (:95-96)
--seed     torch.manual_seed in front of the loop (the reference's main() uses 0); the posterior's noise is drawn as the reference
           draws it, batch after batch from the CPU generator, so a run repeats

Host file I/O only; prints the reference's closing line."""
import argparse
import os
import sys

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import diff_foley_amd as P  # noqa: E402
from diff_foley_amd import ldm  # noqa: E402


def load_model(config, ckpt, precision=None):
    with open(config) as f:
        cfg = yaml.safe_load(f)
    model_cfg = dict(cfg["model"])
    if precision is not None:
        model_cfg["params"] = dict(model_cfg["params"], precision=precision)
    model = P.instantiate_from_config(model_cfg)
    if not isinstance(model, P.AlignmentClassifierMetric):
        raise SystemExit(f"{config}: model.target {cfg['model']['target']!r} is not the Align-Acc metric model")
    sd = torch.load(ckpt, map_location="cpu")
    sd = sd["state_dict"] if "state_dict" in sd else sd
    model.load_state_dict(sd, strict=False)
    model.cuda()
    model.eval()
    data = (((cfg.get("data_eval_metric") or {}).get("params") or {}).get("validation") or {}).get("params") or {}
    return model, ldm.align_acc_frames(data.get("fps", 4), data.get("truncate", 131072), data.get("sr", 16000))


def load_clip(specs_dir, feats_dir, file_name, frames):
    spec = np.load(os.path.join(specs_dir, file_name)).astype(np.float32)[:, :512]
    feat = np.load(os.path.join(feats_dir, ldm.align_acc_clip_name(file_name) + ".npz"))["feat"].astype(np.float32)[:frames]
    return torch.from_numpy(spec), torch.from_numpy(feat)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--specs", required=True)
    ap.add_argument("--feats", required=True)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default=None, choices=["fp16", "bf16"])
    a = ap.parse_args(argv)
    model, frames = load_model(a.config, a.ckpt, a.precision)
    files = sorted(f for f in os.listdir(a.specs) if f.endswith(".npy"))
    if not files:
        raise SystemExit(f"{a.specs}: no *.npy mels")
    f = 2 ** (len(model.vae_cfg["ch_mult"]) - 1)
    torch.manual_seed(a.seed)
    correct = total = 0
    chunk = 16 * a.batch_size                    # clips held on the host at a time; one host synchronisation per chunk
    for c0 in range(0, len(files), chunk):
        clips = [load_clip(a.specs, a.feats, name, frames) for name in files[c0:c0 + chunk]]
        specs, feats = torch.stack([s for s, _ in clips]), torch.stack([v for _, v in clips])
        shape = (model.vae_cfg["embed_dim"], specs.shape[1] // f, specs.shape[2] // f)
        noise = torch.cat([torch.randn((min(a.batch_size, len(clips) - i),) + shape) for i in range(0, len(clips), a.batch_size)])
        n_ok, n = model.align_acc(specs, feats, batch_size=a.batch_size, noise=noise)
        correct, total = correct + n_ok, total + n
    avg_acc = correct / total
    print("Metric =====> Avg ACC: {}   Total Num: {}".format(avg_acc, total))
    return avg_acc, total


if __name__ == "__main__":
    main()

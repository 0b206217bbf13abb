"""Float64 restatement of the CAVP spectrogram tower (CAVP_Inference.encode_spec -> Cnn14.forward; inference/model/cavp_model.py:68-84,
inference/model/cavp_modules.py:1440-1483, 1516-1546) as plain functions of a flat state dict with the reference's keys
(``spec_encoder.*``).  It takes any channel widths: the shapes come from the tensors.  Pinned to the reference by
tests/test_cavp_spec_cpu.py against golden G15; the GPU tests compare the engine with it."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
POOLS = ((2, 2), (2, 2), (2, 2), (2, 2), (1, 2), (1, 1))


def out_rows(frames):
    """T' of a T-frame mel: avg_pool2d floors, four times."""
    t = int(frames)
    for ph, _ in POOLS:
        t //= ph
    return t


def _bn(sd, p, x, axis):
    shape = [1] * x.ndim
    shape[axis] = -1
    w, b, m, v = (sd[p + "." + n].to(x.dtype).reshape(shape) for n in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / torch.sqrt(v + BN_EPS) * w + b


def cnn14(sd, spec, taps=None, dtype=torch.float64, pre="spec_encoder."):
    """spec (B, n_mels, T) -> (B, T', embed).  taps: dict filled with every ConvBlock's output, 'conv_block<i>' -> (B, C, t, mel)."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(pre)}
    x = spec.to(dtype).unsqueeze(1).permute(0, 1, 3, 2)              # (B, 1, T, mel)
    x = _bn(sd, pre + "bn", x, 3)                                    # BatchNorm2d over the mel axis (the two transposes)
    for i, pool in enumerate(POOLS):
        p = f"{pre}conv_block{i + 1}"
        x = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"], padding=1), 1))
        x = F.relu(_bn(sd, p + ".bn2", F.conv2d(x, sd[p + ".conv2.weight"], padding=1), 1))
        x = F.avg_pool2d(x, kernel_size=pool)
        if taps is not None:
            taps[f"conv_block{i + 1}"] = x
    x = x.mean(dim=3)                                                # (B, C, T')
    x = F.max_pool1d(x, 3, 1, 1) + F.avg_pool1d(x, 3, 1, 1)          # -inf padding / zero padding, always / 3
    x = x.transpose(1, 2)
    w, b = sd[pre + "fc1.weight"], sd[pre + "fc1.bias"]
    x = F.relu(F.linear(F.relu(F.linear(x, w, b)), w, b))            # fc1 twice (cavp_modules.py:1543-1544)
    return F.linear(x, sd[pre + "final_project.weight"], sd[pre + "final_project.bias"])


def encode_spec(sd, spec, normalize=False, pool=True, taps=None, dtype=torch.float64):
    x = cnn14(sd, spec, taps, dtype)
    if pool:
        x = F.max_pool1d(x.permute(0, 2, 1), 16).squeeze(2)
    if normalize:
        x = F.normalize(x, dim=-1)
    return x


def similarity(v, s, scale=1.0):
    """(Bv, Bs): scale * mean_t <v[i, t], s[j, t]>."""
    return scale * torch.einsum("itd,jtd->ij", v.double(), s.double()) / v.shape[1]

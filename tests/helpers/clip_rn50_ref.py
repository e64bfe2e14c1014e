"""CPU oracles of the frozen CLIP RN50 image trunk (safevla_amd.preproc.ClipResNet), written on a CLIP ``visual`` state dict with
``torch.nn.functional.conv2d`` / ``avg_pool2d`` / ``batch_norm`` in fp32:

  forward_fp32   the published ModifiedResNet forward without its attention pool (the reference's ClipResNet, pool=False), as is
  forward_bf16   the same network the way the kernels evaluate it: every eval-mode BatchNorm folded into its convolution, the folded weights rounded to bf16,
                 fp32 accumulation, the activation rounded to bf16 after every layer (= every launch's output)

The distance between the two on an input is the noise floor of the bf16 arithmetic for that input; the GPU tests gate on twice that distance."""
import torch
import torch.nn.functional as F

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
LAYERS = (3, 4, 6, 3)
EPS = 1e-5


def perturbed_state_dict(sd, seed=0):
    """every BatchNorm's weight / bias / running_mean / running_var moved off its initial 1 / 0 / 0 / 1 so that the folding is exercised"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        v = v.detach().cpu().float().clone()
        if ("bn" in k or ".downsample.1." in k) and v.dim() == 1:
            if k.endswith(".weight"):
                v = 1.0 + 0.2 * (2 * torch.rand(v.shape, generator=g) - 1)
            elif k.endswith("running_var"):
                v = 0.5 + torch.rand(v.shape, generator=g)
            else:                                           # bias, running_mean
                v = 0.1 * torch.randn(v.shape, generator=g)
        out[k] = v
    return out


def normalise(frames_u8):
    x = frames_u8.cpu().permute(0, 3, 1, 2).float() / 255.0
    return (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, EPS)


def _blocks():
    for i, n in enumerate(LAYERS):
        for j in range(n):
            yield f"layer{i + 1}.{j}", (2 if i > 0 and j == 0 else 1)


@torch.no_grad()
def forward_fp32(sd, frames_u8):
    """(B, 2048, H/32, W/32) fp32"""
    x = normalise(frames_u8)
    x = F.relu(_bn(F.conv2d(x, sd["conv1.weight"], stride=2, padding=1), sd, "bn1"))
    x = F.relu(_bn(F.conv2d(x, sd["conv2.weight"], padding=1), sd, "bn2"))
    x = F.relu(_bn(F.conv2d(x, sd["conv3.weight"], padding=1), sd, "bn3"))
    x = F.avg_pool2d(x, 2)
    for p, stride in _blocks():
        out = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"]), sd, p + ".bn1"))
        out = F.relu(_bn(F.conv2d(out, sd[p + ".conv2.weight"], padding=1), sd, p + ".bn2"))
        if stride > 1:
            out = F.avg_pool2d(out, stride)
        out = _bn(F.conv2d(out, sd[p + ".conv3.weight"]), sd, p + ".bn3")
        idn = x
        if p + ".downsample.0.weight" in sd:
            idn = F.avg_pool2d(x, stride) if stride > 1 else x
            idn = _bn(F.conv2d(idn, sd[p + ".downsample.0.weight"]), sd, p + ".downsample.1")
        x = F.relu(out + idn)
    return x


def bf16r(x):
    return x.to(torch.bfloat16).float()


def fold(sd, conv, bn):
    s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + EPS)
    return bf16r(sd[conv + ".weight"] * s[:, None, None, None]), sd[bn + ".bias"] - sd[bn + ".running_mean"] * s


@torch.no_grad()
def forward_bf16(sd, frames_u8):
    """(B, 2048, H/32, W/32) fp32 holding bf16 values"""
    def cv(x, conv, bn, relu, **kw):
        w, b = fold(sd, conv, bn)
        y = F.conv2d(x, w, b, **kw)
        return bf16r(F.relu(y) if relu else y)

    x = cv(normalise(frames_u8), "conv1", "bn1", True, stride=2, padding=1)
    x = cv(x, "conv2", "bn2", True, padding=1)
    x = cv(x, "conv3", "bn3", True, padding=1)
    x = bf16r(F.avg_pool2d(x, 2))
    for p, stride in _blocks():
        out = cv(x, p + ".conv1", p + ".bn1", True)
        out = cv(out, p + ".conv2", p + ".bn2", True, padding=1)
        if stride > 1:
            out = bf16r(F.avg_pool2d(out, stride))
        idn = x
        if p + ".downsample.0.weight" in sd:
            idn = bf16r(F.avg_pool2d(x, stride)) if stride > 1 else x
            idn = cv(idn, p + ".downsample.0", p + ".downsample.1", False)
        w, b = fold(sd, p + ".conv3", p + ".bn3")
        x = bf16r(F.relu(F.conv2d(out, w, b) + idn))
    return x


def frames(B, H, W, seed):
    """smooth-ish random uint8 frames: a low-resolution random image upsampled, plus pixel noise (a camera frame is not white noise)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, max(1, H // 16), max(1, W // 16), generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * 255 + 12 * torch.randn(B, 3, H, W, generator=g)
    return x.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def rel_err(got, want):
    """max-abs error relative to the oracle's max-abs"""
    return float((got.float() - want.float()).abs().max() / want.float().abs().max())

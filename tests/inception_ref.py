"""Plain-torch restatement of torchvision's ``Inception3`` (eval, ``aux_logits=False``) and of the reference's
``FIDInceptionModel`` (models/imagenet_pretrained.py:64-111), from a torchvision-format state dict, in the dtype of the state
dict handed in (the tests use float64 on the CPU, and fp32 to measure the reference's own rounding noise).  ATen calls only:
``F.conv2d``, ``F.batch_norm`` in eval form, ``F.max_pool2d``, ``F.avg_pool2d``, ``F.interpolate``, ``F.linear``.

Written from torchvision's published model definition (torchvision/models/inception.py), independently of the package's layer
table: the geometry of every convolution is spelled out where it is applied."""
import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def cast(sd, dtype):
    return {k: (v.detach().cpu().to(dtype) if v.dtype.is_floating_point else v.detach().cpu()) for k, v in sd.items()}


def bconv(sd, name, x, stride=1, padding=0):
    """BasicConv2d: conv(bias=False) -> BatchNorm2d(eps=1e-3), running statistics -> ReLU."""
    x = F.conv2d(x, sd[name + ".conv.weight"], None, stride=stride, padding=padding)
    x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                     training=False, eps=1e-3)
    return F.relu(x)


def inception_a(sd, p, x):
    b1 = bconv(sd, p + ".branch1x1", x)
    b5 = bconv(sd, p + ".branch5x5_2", bconv(sd, p + ".branch5x5_1", x), padding=2)
    b3 = bconv(sd, p + ".branch3x3dbl_1", x)
    b3 = bconv(sd, p + ".branch3x3dbl_2", b3, padding=1)
    b3 = bconv(sd, p + ".branch3x3dbl_3", b3, padding=1)
    bp = bconv(sd, p + ".branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
    return torch.cat([b1, b5, b3, bp], 1)


def inception_b(sd, p, x):
    b3 = bconv(sd, p + ".branch3x3", x, stride=2)
    bd = bconv(sd, p + ".branch3x3dbl_1", x)
    bd = bconv(sd, p + ".branch3x3dbl_2", bd, padding=1)
    bd = bconv(sd, p + ".branch3x3dbl_3", bd, stride=2)
    return torch.cat([b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def inception_c(sd, p, x):
    b1 = bconv(sd, p + ".branch1x1", x)
    b7 = bconv(sd, p + ".branch7x7_1", x)
    b7 = bconv(sd, p + ".branch7x7_2", b7, padding=(0, 3))
    b7 = bconv(sd, p + ".branch7x7_3", b7, padding=(3, 0))
    bd = bconv(sd, p + ".branch7x7dbl_1", x)
    bd = bconv(sd, p + ".branch7x7dbl_2", bd, padding=(3, 0))
    bd = bconv(sd, p + ".branch7x7dbl_3", bd, padding=(0, 3))
    bd = bconv(sd, p + ".branch7x7dbl_4", bd, padding=(3, 0))
    bd = bconv(sd, p + ".branch7x7dbl_5", bd, padding=(0, 3))
    bp = bconv(sd, p + ".branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
    return torch.cat([b1, b7, bd, bp], 1)


def inception_d(sd, p, x):
    b3 = bconv(sd, p + ".branch3x3_2", bconv(sd, p + ".branch3x3_1", x), stride=2)
    b7 = bconv(sd, p + ".branch7x7x3_1", x)
    b7 = bconv(sd, p + ".branch7x7x3_2", b7, padding=(0, 3))
    b7 = bconv(sd, p + ".branch7x7x3_3", b7, padding=(3, 0))
    b7 = bconv(sd, p + ".branch7x7x3_4", b7, stride=2)
    return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


def inception_e(sd, p, x):
    b1 = bconv(sd, p + ".branch1x1", x)
    b3 = bconv(sd, p + ".branch3x3_1", x)
    b3 = torch.cat([bconv(sd, p + ".branch3x3_2a", b3, padding=(0, 1)), bconv(sd, p + ".branch3x3_2b", b3, padding=(1, 0))], 1)
    bd = bconv(sd, p + ".branch3x3dbl_1", x)
    bd = bconv(sd, p + ".branch3x3dbl_2", bd, padding=1)
    bd = torch.cat([bconv(sd, p + ".branch3x3dbl_3a", bd, padding=(0, 1)), bconv(sd, p + ".branch3x3dbl_3b", bd, padding=(1, 0))], 1)
    bp = bconv(sd, p + ".branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
    return torch.cat([b1, b3, bd, bp], 1)


def transform_input(x):
    """torchvision's Inception3._transform_input."""
    ch = [x[:, c:c + 1] * (STD[c] / 0.5) + (MEAN[c] - 0.5) / 0.5 for c in range(3)]
    return torch.cat(ch, 1)


def features(sd, x, stem_pool="max", transform=False):
    """x [N, 3, H, W] -> the pooled Mixed_7c output [N, 2048]; ``stem_pool="avg"``: F.avg_pool2d(3, 2) where torchvision has its
    two stem max-pools (what FIDInceptionModel's loop over ``_modules`` computes with torchvision 0.4.x)."""
    pool = (lambda t: F.max_pool2d(t, kernel_size=3, stride=2)) if stem_pool == "max" else (lambda t: F.avg_pool2d(t, kernel_size=3, stride=2))
    if transform:
        x = transform_input(x)
    x = bconv(sd, "Conv2d_1a_3x3", x, stride=2)
    x = bconv(sd, "Conv2d_2a_3x3", x)
    x = bconv(sd, "Conv2d_2b_3x3", x, padding=1)
    x = pool(x)
    x = bconv(sd, "Conv2d_3b_1x1", x)
    x = bconv(sd, "Conv2d_4a_3x3", x)
    x = pool(x)
    for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = inception_a(sd, p, x)
    x = inception_b(sd, "Mixed_6a", x)
    for p in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = inception_c(sd, p, x)
    x = inception_d(sd, "Mixed_7a", x)
    x = inception_e(sd, "Mixed_7b", x)
    x = inception_e(sd, "Mixed_7c", x)
    return torch.flatten(F.adaptive_avg_pool2d(x, (1, 1)), 1)


def logits(sd, x, stem_pool="max", transform=False):
    return F.linear(features(sd, x, stem_pool, transform), sd["fc.weight"], sd["fc.bias"])


def fid_input(x):
    """FIDInceptionModel.forward up to the network: nn.Upsample((299, 299), 'bilinear') -> scale_img -> normalise."""
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    x = torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def fid_features(sd, x, stem_pool="avg"):
    return features(sd, fid_input(x), stem_pool)


def resize_formula(x, mode):
    """The input kernel's formula, evaluated with explicit gathers in the dtype of ``x`` (float64 in the tests):
    ``src = max((dst + 0.5) in / 299 - 0.5, 0)``, neighbours clamped at the border; then the affine of ``mode``."""
    n, c, h, w = x.shape
    dt = x.dtype

    def axis(size):
        src = torch.clamp((torch.arange(299, dtype=dt) + 0.5) * (size / 299.0) - 0.5, min=0.0)
        i0 = torch.clamp(src.floor().long(), max=size - 1)
        return i0, torch.clamp(i0 + 1, max=size - 1), src - i0.to(dt)
    y0, y1, ly = axis(h)
    x0, x1, lx = axis(w)
    ly, lx = ly.view(1, 1, 299, 1), lx.view(1, 1, 1, 299)
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    v = (1 - ly) * top + ly * bot
    if mode == "transform":
        v = transform_input(v)
    elif mode == "fid":
        mean = torch.tensor(MEAN, dtype=dt).view(1, 3, 1, 1)
        std = torch.tensor(STD, dtype=dt).view(1, 3, 1, 1)
        v = (torch.clamp((v + 1.0) / 2.0, 0.0, 1.0) - mean) / std
    return v

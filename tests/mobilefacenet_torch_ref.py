"""MobileFaceNet (the network morphganformer_amd/mobilefacenet.py runs) restated functionally in torch from its contract: driven by a
state dict under the reference's key names, generic over dtype, differentiable.  A helper of the tests, not a test module;
tests/test_mobilefacenet_host.py pins it on the reference module's recorded outputs (tests/golden/mobilefacenet.npz).

    ConvBlock = conv (no bias) -> eval BatchNorm (eps 1e-5) -> per-channel PReLU;  LinearBlock = conv -> BatchNorm
    DepthWise(in, out, g, stride) = ConvBlock 1x1 in->g, ConvBlock 3x3 pad 1 groups g at the stride, LinearBlock 1x1 g->out (+ input)
"""
import torch
import torch.nn.functional as F

EPS = 1e-5
# (index in `layers`, groups, stride, number of residual blocks; 0 = one plain DepthWise)
TRUNK = [(2, 128, 2, 0), (3, 128, 1, 4), (4, 256, 2, 0), (5, 256, 1, 6), (6, 512, 2, 0), (7, 256, 1, 2)]


def as_state(sd, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def _bn(x, sd, name):
    shape = (1, -1) + (1,) * (x.ndim - 2)
    g = lambda k: sd[f"{name}.{k}"].reshape(shape)
    return (x - g("running_mean")) / torch.sqrt(g("running_var") + EPS) * g("weight") + g("bias")


def _block(x, sd, name, stride=1, pad=0, groups=1, prelu=True):
    x = _bn(F.conv2d(x, sd[name + ".layers.0.weight"], None, stride, pad, 1, groups), sd, name + ".layers.1")
    return F.prelu(x, sd[name + ".layers.2.weight"]) if prelu else x


def _depthwise(x, sd, name, g, stride, residual):
    h = _block(x, sd, name + ".layers.0")
    h = _block(h, sd, name + ".layers.1", stride, 1, g)
    h = _block(h, sd, name + ".layers.2", prelu=False)
    return x + h if residual else h


def mobilefacenet_torch(sd, x, stages=None):
    """x [n,3,112,112] -> embedding [n,512] in x's dtype (sd: as_state(..., x.dtype)); `stages`: a list that receives the outputs of
    layers.0 .. layers.7 and conv_sep."""
    keep = (lambda t: stages.append(t)) if stages is not None else (lambda t: None)
    x = _block(x, sd, "layers.0", 2, 1); keep(x)
    x = _block(x, sd, "layers.1", 1, 1, 64); keep(x)
    for li, g, stride, nres in TRUNK:
        if nres == 0:
            x = _depthwise(x, sd, f"layers.{li}", g, stride, False)
        else:
            for j in range(nres):
                x = _depthwise(x, sd, f"layers.{li}.layers.{j}", g, 1, True)
        keep(x)
    x = _block(x, sd, "conv_sep"); keep(x)
    x = _block(x, sd, "features.layers.0", 1, 0, 512, prelu=False).flatten(1)
    return _bn(F.linear(x, sd["features.layers.2.weight"]), sd, "features.layers.3")


def embed_image_torch(sd, img):
    """embed_image: bilinear resize (align_corners=False) to 112x112 unless the image already is."""
    if tuple(img.shape[2:]) != (112, 112):
        img = F.interpolate(img, size=(112, 112), mode="bilinear", align_corners=False)
    return mobilefacenet_torch(sd, img)


def embedding_grad(sd, x, v):
    """(embedding, d sum(embedding * v) / d x) by autograd, in x's dtype."""
    x = x.detach().clone().requires_grad_(True)
    e = mobilefacenet_torch(sd, x)
    (g,) = torch.autograd.grad((e * v).sum(), x)
    return e.detach(), g


def biometric_loss_torch(sd, pred, target):
    """MSE(embed_image(pred[i]), embed_image(target)) per sample [n]; target [1,..] or [n,..]."""
    return (embed_image_torch(sd, pred) - embed_image_torch(sd, target)).square().mean(1)


def fixture_gradients(g):
    """(float32 gradient, float64 gradient) of tests/golden/mobilefacenet.npz as numpy arrays: the file stores float32(grad64), the
    float32 remainder of grad64 and the exact float32 difference of the two gradients (tools/make_mobilefacenet_golden.py)."""
    import numpy as np
    hi = g["grad64_hi"]
    return hi + g["grad_delta"], hi.astype(np.float64) + g["grad64_lo"].astype(np.float64)

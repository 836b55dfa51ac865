"""Oracle: torch-CPU fp32 restatement of torchvision 0.16 ``shufflenet_v2_x1_0``
with the ``fc`` head the reference swaps in (``src/tt100k/pipeline/e2e.py:331-333``)
and of ``PyTorchClassifier.predict_batch`` (e2e.py:378-396).

TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED: torchvision is not installed in the
build container and the reference ships no classifier weights or outputs; the
architecture follows the published ShuffleNetV2 x1.0 definition (SURVEY
Appendix B).  Module/parameter names equal torchvision's state_dict keys, so a
real ``shufflenetv2.pth`` loads with ``load_state_dict``.
"""
from __future__ import annotations

import copy
from typing import List, Tuple

import numpy as np
import torch
import torch.nn as nn

from .pil_resize_ref import classifier_input

STAGE_REPEATS = (4, 8, 4)
STAGE_OUT = (24, 116, 232, 464, 1024)


def channel_shuffle(x: torch.Tensor, groups: int) -> torch.Tensor:
    b, c, h, w = x.shape
    return x.view(b, groups, c // groups, h, w).transpose(1, 2).reshape(b, c, h, w)


class InvertedResidual(nn.Module):
    def __init__(self, inp: int, oup: int, stride: int):
        super().__init__()
        self.stride = stride
        bf = oup // 2
        if stride > 1:
            self.branch1 = nn.Sequential(
                nn.Conv2d(inp, inp, 3, stride, 1, groups=inp, bias=False), nn.BatchNorm2d(inp),
                nn.Conv2d(inp, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True))
        else:
            self.branch1 = nn.Sequential()
        self.branch2 = nn.Sequential(
            nn.Conv2d(inp if stride > 1 else bf, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True),
            nn.Conv2d(bf, bf, 3, stride, 1, groups=bf, bias=False), nn.BatchNorm2d(bf),
            nn.Conv2d(bf, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True))

    def forward(self, x):
        if self.stride == 1:
            x1, x2 = x.chunk(2, dim=1)
            out = torch.cat((x1, self.branch2(x2)), dim=1)
        else:
            out = torch.cat((self.branch1(x), self.branch2(x)), dim=1)
        return channel_shuffle(out, 2)


class ShuffleNetV2(nn.Module):
    def __init__(self, num_classes: int = 58):
        super().__init__()
        c = STAGE_OUT
        self.conv1 = nn.Sequential(nn.Conv2d(3, c[0], 3, 2, 1, bias=False), nn.BatchNorm2d(c[0]), nn.ReLU(inplace=True))
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inp = c[0]
        for name, rep, oup in zip(("stage2", "stage3", "stage4"), STAGE_REPEATS, c[1:4]):
            seq = [InvertedResidual(inp, oup, 2)] + [InvertedResidual(oup, oup, 1) for _ in range(rep - 1)]
            setattr(self, name, nn.Sequential(*seq))
            inp = oup
        self.conv5 = nn.Sequential(nn.Conv2d(inp, c[4], 1, 1, 0, bias=False), nn.BatchNorm2d(c[4]), nn.ReLU(inplace=True))
        self.fc = nn.Linear(c[4], num_classes)

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        x = self.stage4(self.stage3(self.stage2(x)))
        x = self.conv5(x).mean([2, 3])
        return self.fc(x)


def seeded_state_dict(num_classes: int, seed: int = 1234, gain: float = 1.7) -> "dict[str, torch.Tensor]":
    """Synthetic weights with non-trivial BN statistics (random-init torchvision
    weights have identity BN, which would not exercise BN folding)."""
    g = torch.Generator().manual_seed(seed)
    model = ShuffleNetV2(num_classes)
    sd = model.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            sd[k] = torch.rand(v.shape, generator=g) * 0.5 + 0.75
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
        elif v.dim() == 1 and k.endswith("weight"):  # BN gamma
            sd[k] = torch.rand(v.shape, generator=g) * 0.5 + 0.75
        elif v.dim() == 1:  # BN beta / fc bias
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
        else:
            fan_in = float(np.prod(v.shape[1:]))
            sd[k] = torch.randn(v.shape, generator=g) * (gain / fan_in) ** 0.5
    return sd


def build(num_classes: int, state_dict=None) -> ShuffleNetV2:
    m = ShuffleNetV2(num_classes)
    if state_dict is not None:
        m.load_state_dict(state_dict)
    return m.eval()


@torch.no_grad()
def predict_batch(model: ShuffleNetV2, rois_bgr: List[np.ndarray], size: int = 64) -> Tuple[np.ndarray, np.ndarray]:
    """e2e.py:378-396."""
    if len(rois_bgr) == 0:
        return np.array([]), np.array([])
    batch = torch.from_numpy(np.stack([classifier_input(r, size) for r in rois_bgr]))
    probs = torch.softmax(model(batch), dim=1).numpy()
    return np.argmax(probs, axis=1), probs


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference, and a folded float64 forward that can emulate the fp16 storage of each GPU path
# ---------------------------------------------------------------------------------------------------------------------
def input_batch(rois_bgr: List[np.ndarray], size: int = 64) -> np.ndarray:
    """classifier_input of every ROI, stacked: fp32 [N,3,size,size] (what the reference's model sees)."""
    return np.stack([classifier_input(r, size) for r in rois_bgr])


def resized_u8(rois_bgr: List[np.ndarray], size: int = 64) -> np.ndarray:
    """The uint8 RGB crops the GPU classifier reads (PIL bilinear of e2e.py:385-389): [N,3,size,size]."""
    from .pil_resize_ref import resize_bilinear_u8
    return np.stack([resize_bilinear_u8(np.ascontiguousarray(r[:, :, ::-1]), size, size).transpose(2, 0, 1) for r in rois_bgr])


@torch.no_grad()
def logp_module(model: nn.Module, x: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """log softmax of ``model`` run in ``dtype`` on the input batch ``x`` (input_batch), as float64 [N, classes]."""
    m = copy.deepcopy(model).to(dtype).eval()
    return torch.log_softmax(m(torch.from_numpy(x).to(dtype)), dim=1).double().numpy()


# One fp16 rounding recipe per GPU path of the fp16 classifier.  Everything not listed stays float64.
#   w16      pointwise (1x1 conv, conv5, fc) weights rounded to fp16: cls_net.hip / cls_fused.hip read them from
#            pack_fused_pw (cls_plan.h), the layer-at-a-time MFMA and naive kernels from ConvLayer::build
#            (conv_kernels.hip, put_elem).  Depthwise weights and every bias stay fp32 (upload_f32, add_dw,
#            classifier.cpp): not rounded.
#   acts     every stored activation rounded: stem output, depthwise outputs, pointwise outputs (both shuffle halves).
#            cls_dev.h: store_relu; cls_net.hip: dwconv, the stage2.0/3.0/4.0 shuffle stores, s1_block (the maxpool and
#            the x_lo copy move stored fp16 values: nothing new to round); the 8 KB hand-off cls_front -> cls_back
#            copies the fp16 LDS image X3, already rounded.  Layer-at-a-time: cls_stem_kernel, dwconv3x3_kernel
#            (cls_kernels.hip), conv_naive_kernel (conv_kernels.hip), the MFMA pointwise epilogues,
#            shuffle_stage_kernel (cls_fused.hip).
#   stem     "u8": cls_net.hip's MFMA stem multiplies the uint8 bytes by fp16(w / 255 / 0.34) and adds
#            bias - 0.18 / 0.34 * (sum of the weights of the taps inside the image) in fp32 (pack_cls_stem, cls_plan.h);
#            "f32": cls_stem_kernel (cls_kernels.hip): fp32 weights on the fp32-normalised input, nothing rounded
#            but its output.
#   conv5    "mean": conv5 + ReLU in fp32, averaged in fp32, only the mean rounded (conv5_mean_store, cls_dev.h, in
#            cls_back and cls_head_fused); "store": conv5's ReLU output stored as fp16 (ConvLayer epilogue), then
#            spatial_mean_kernel averages the rounded values and rounds the mean (cls_kernels.hip).
#   Logits and softmax are fp32 on every path (out_f32 of the fc ConvLayer; LG in cls_back / cls_head_fused): not rounded.
RECIPES = {
    # A: default fp16 path, cls_front + cls_back (cls_net.hip)
    "fused": dict(w16=True, acts=True, stem="u8", conv5="mean"),
    # B: LITEPI_CLS_LAYERWISE=1: cls_stem, maxpool, per-layer stride-2 blocks, shuffle_stage_fused, cls_head_fused
    "layerwise": dict(w16=True, acts=True, stem="f32", conv5="mean"),
    # C: conv_impl = 1 at fp16: every layer its own kernel (conv_naive, dwconv3x3, spatial_mean, softmax_argmax)
    "naive": dict(w16=True, acts=True, stem="f32", conv5="store"),
}


def fold_bn(sd, conv: str, bn: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv (no bias) + BatchNorm(eval, eps 1e-5) -> (weight, bias) in float64, as fold() of csrc/cls_plan.h."""
    w = sd[conv + ".weight"].double()
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
    return w * s.view(-1, 1, 1, 1), sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s


def _f16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(torch.float64)


@torch.no_grad()
def folded_logp(sd, rois_bgr: List[np.ndarray], recipe=None) -> np.ndarray:
    """BN-folded forward in float64 -> log softmax [N, classes].  recipe None: no rounding anywhere (equals the float64
    module); a RECIPES key or dict: fp16 rounding exactly where that GPU path stores fp16 (see RECIPES)."""
    import torch.nn.functional as F
    r = RECIPES[recipe] if isinstance(recipe, str) else (recipe or dict(w16=False, acts=False, stem="f32", conv5="mean"))
    rw = _f16 if r["w16"] else (lambda t: t)
    ra = _f16 if r["acts"] else (lambda t: t)

    def pw(x, w, b, relu=True):
        y = F.conv2d(x, rw(w), b)
        return ra(F.relu(y) if relu else y)

    def dw(x, w, b, stride):
        return ra(F.conv2d(x, w, b, stride, 1, groups=x.shape[1]))

    w1, b1 = fold_bn(sd, "conv1.0", "conv1.1")
    if r["stem"] == "u8":
        u8 = torch.from_numpy(resized_u8(rois_bgr)).double()
        y = F.conv2d(u8, _f16(w1 / 255.0 / 0.34), None, 2, 1)
        inside = F.conv2d(torch.ones_like(u8[:1]), w1, None, 2, 1)   # sum of the weights of the taps inside the image
        y = y + b1.view(1, -1, 1, 1) - (0.18 / 0.34) * inside
    else:
        y = F.conv2d(torch.from_numpy(input_batch(rois_bgr)).double(), w1, b1, 2, 1)
    x = F.max_pool2d(ra(F.relu(y)), 3, 2, 1)
    for name, rep in zip(("stage2", "stage3", "stage4"), STAGE_REPEATS):
        for i in range(rep):
            p = f"{name}.{i}."
            if i == 0:
                x1 = pw(dw(x, *fold_bn(sd, p + "branch1.0", p + "branch1.1"), 2), *fold_bn(sd, p + "branch1.2", p + "branch1.3"))
                x2, stride = x, 2
            else:
                x1, x2 = x.chunk(2, dim=1)
                stride = 1
            t = pw(x2, *fold_bn(sd, p + "branch2.0", p + "branch2.1"))
            t = dw(t, *fold_bn(sd, p + "branch2.3", p + "branch2.4"), stride)
            t = pw(t, *fold_bn(sd, p + "branch2.5", p + "branch2.6"))
            x = channel_shuffle(torch.cat((x1, t), dim=1), 2)
    w5, b5 = fold_bn(sd, "conv5.0", "conv5.1")
    z = F.relu(F.conv2d(x, rw(w5), b5))
    if r["conv5"] == "store":
        z = ra(z)
    m = ra(z.mean([2, 3]))
    logits = m @ rw(sd["fc.weight"].double()).t() + sd["fc.bias"].double()
    return torch.log_softmax(logits, dim=1).numpy()

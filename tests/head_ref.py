"""Float64 restatement of ONE pyramid level of the Detect head, for the tests that pin the fp16 head kernels to their own input
map (test_head_ref_cpu.py, test_gpu_head_float64.py).  Plain torch / NumPy on the CPU; nothing of the package under test is
imported (the tests take the anchor grid from the exporter's ``make_anchors``).

    box tower  : 3x3 (Cin -> 64) + SiLU -> 3x3 (64 -> 64) + SiLU -> 1x1 (64 -> 4 x reg_max)
    class tower: 3x3 (Cin -> c3) + SiLU -> 3x3 (c3 -> c3) + SiLU -> 1x1 (c3 -> nc)
    decode     : softmax over the reg_max bins of a side, expectation with dfl_w, dist2bbox around the anchor, x stride;
                 sigmoid of the class logits

Rounding points (``head_out0`` flags), read off the kernels.  Every sum is fp32 on the device, float64 here.

  weights      fp16, once: a property of the stored model, not an error of the kernel (hplan::pack_head's ``frag`` / ``frag16``
               pack every weight with f32_to_f16, head_plan.h; ConvLayer packs its fragments the same way).  Biases stay
               fp32: they initialise the fp32 accumulators (``bias16`` / ``biasA16``, head_kernels.hip) or are added to them
               (``act4(v, bias)``, conv_kernels.hip).
  round_mid    the two post-SiLU activations of each tower, fp16 round-to-nearest-even.
               fused plan: ``mid_store16`` (A16) / the ``silu_h8`` stores of the 32-pixel stage A write SiLU(first conv) into
               the LDS image MID as half8 (head_kernels.hip, "SiLU, fp16, -> MID"); ``silu_h8(accC[mt][p], 8 * s)`` and
               ``silu_h8(accB[mt][p], 8 * s)`` round SiLU(second conv) to the half8 B operand of the projection's MFMA.
               three-launch plan: ``store_lane`` writes the merged first convs' SiLU output to HBM as half8
               (``q[i] = (half_t)y0[i]``, conv_kernels.hip), ``tail_store`` rounds SiLU(second conv) to the B operand of the
               fused 1x1 (``bq[s][i] = (half_t)y0[i]``: "rounded to T first, as if it had been stored and re-loaded"); v2's
               48-channel class tower stores it through ``store_lane`` and runs the 1x1 as a launch of its own.
  round_logits both projection outputs, fp16: the three-launch plan only.  ``tail_store`` ends in ``store_lane<T, T2, ACT_NONE>``,
               which writes the 64 box logits and the nc class logits to HBM as halfs; ``decode_kernel<half_t>``
               (post_kernels.hip) reads them back (``v[q * G + i] = (float)x[i]``, ``(float)cls[c]``).  The fused kernel decodes
               the fp32 accumulators ``ob[rt]`` / ``oc`` directly ("fp32 logits straight from the accumulators").

Softmax, expectation, dist2bbox and the sigmoid run in fp32 on the device (hardware exp2 / rcp or __expf, relative error ~1e-7)
and are written to out0 as fp32: no flag.

Mutations (``mutate=``; applied to this reference only, never to a kernel): deliberate errors of the kind a tiled kernel makes,
which test_head_ref_cpu.py uses to show that the caps of ``broken_caps`` would catch them.
"""
import numpy as np
import torch
import torch.nn.functional as F

MUTATIONS = (
    "box2_tap02_col15",   # tap (0, 2) of the box tower's second conv dropped on output columns x % 16 == 15 (a tile's last column)
    "box2_tap02_row9",    # the same tap dropped on output rows y % 10 == 9 (the last row of a 10-row tile)
    "cls1_swap01",        # input channels 0 and 1 swapped in the centre tap of the class tower's first conv
    "dfl15",              # dfl_w[15] = 14
    "anchor_shift",       # the level's anchors shifted by one index
    "cls_swap12",         # classes 1 and 2 exchanged (nc >= 3)
    "cls_bias21",         # the class projection's bias of class 2 used for class 1 (nc >= 3)
)


def find_heads(layers):
    """Per pyramid level (graph order: P3, P4, P5) of ``oracle.ncnn_ref.load_model`` output: ``{"feat": blob name of the neck map
    both towers read, "box": [conv3x3, conv3x3, conv1x1], "cls": [conv3x3, conv3x3, conv1x1]}`` (Layer objects)."""
    prod = {o: L for L in layers for o in L.outputs}

    def src(name):   # the blob a Split output is a copy of
        while prod[name].type == "Split":
            name = prod[name].inputs[0]
        return name

    def tower(blob):
        proj = prod[src(blob)]
        s2 = prod[src(proj.inputs[0])]
        c2 = prod[src(s2.inputs[0])]
        s1 = prod[src(c2.inputs[0])]
        c1 = prod[src(s1.inputs[0])]
        assert [L.type for L in (proj, s2, c2, s1, c1)] == ["Convolution", "Swish", "Convolution", "Swish", "Convolution"]
        assert proj.weight.shape[2:] == (1, 1) and c2.weight.shape[2:] == (3, 3) and c1.weight.shape[2:] == (3, 3)
        return src(c1.inputs[0]), [c1, c2, proj]

    heads = []
    for L in layers:
        if L.type != "Concat" or len(L.inputs) != 2 or any(prod[src(i)].type != "Convolution" for i in L.inputs):
            continue
        nxt = [M for M in layers if L.outputs[0] in M.inputs]
        if not nxt or nxt[0].type != "Reshape":
            continue
        fb, box = tower(L.inputs[0])
        fc, cls = tower(L.inputs[1])
        assert fb == fc, "the two towers of a level read one map"
        heads.append({"feat": fb, "box": box, "cls": cls})
    return heads


def round_fp16(t):
    """Round to the nearest fp16 value (ties to even), keep the dtype.  Through NumPy: its float64 -> float16 conversion rounds
    once (a conversion by way of float32 would round twice)."""
    return torch.from_numpy(t.numpy().astype(np.float16).astype(t.numpy().dtype))


def _silu(x):
    return x * torch.sigmoid(x)


def _conv3(x, w, b, tapwise):
    if not tapwise:
        return F.conv2d(x, w, b, padding=1)
    H, W = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    y = b.view(1, -1, 1, 1).expand(x.shape[0], -1, H, W).clone()
    for ky in range(3):
        for kx in range(3):
            y += F.conv2d(xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky:ky + 1, kx:kx + 1])
    return y


def _head(feat, level, anchors, stride, dfl_w, round_mid, round_logits, mutate, round_weights, dtype, tapwise):
    mutate = (mutate,) if isinstance(mutate, str) else tuple(mutate or ())
    assert all(m in MUTATIONS for m in mutate), mutate
    x = torch.as_tensor(np.asarray(feat)).to(dtype)
    N, _, H, W = x.shape

    def wb(L):
        w = torch.from_numpy(L.weight)
        if round_weights:
            w = round_fp16(w)
        return w.to(dtype), torch.from_numpy(L.bias).to(dtype)

    def mid(t):
        return round_fp16(t) if round_mid else t

    def logits(t):
        return round_fp16(t) if round_logits else t

    # ---- box tower
    (w1, b1), (w2, b2), (w3, b3) = (wb(L) for L in level["box"])
    m1 = mid(_silu(_conv3(x, w1, b1, tapwise)))
    y2 = _conv3(m1, w2, b2, tapwise)
    for m, mask in (("box2_tap02_col15", (torch.arange(W) % 16 == 15).view(1, 1, 1, W).expand(1, 1, H, W)),
                    ("box2_tap02_row9", (torch.arange(H) % 10 == 9).view(1, 1, H, 1).expand(1, 1, H, W))):
        if m in mutate:
            tap = F.conv2d(F.pad(m1, (1, 1, 1, 1))[:, :, 0:H, 2:2 + W], w2[:, :, 0:1, 2:3])
            y2 = y2 - tap * mask.to(dtype)
    box = logits(F.conv2d(mid(_silu(y2)), w3, b3))
    # ---- class tower
    (w1, b1), (w2, b2), (w3, b3) = (wb(L) for L in level["cls"])
    if "cls1_swap01" in mutate:
        w1 = w1.clone()
        w1[:, [0, 1], 1, 1] = w1[:, [1, 0], 1, 1]
    if "cls_bias21" in mutate:
        b3 = b3.clone()
        b3[1] = b3[2]
    cls = logits(F.conv2d(mid(_silu(_conv3(mid(_silu(_conv3(x, w1, b1, tapwise))), w2, b2, tapwise))), w3, b3))
    if "cls_swap12" in mutate:
        cls = cls[:, [0, 2, 1] + list(range(3, cls.shape[1]))]
    # ---- decode
    dfl = torch.as_tensor(np.asarray(dfl_w)).to(dtype).clone()
    if "dfl15" in mutate:
        dfl[15] = 14
    anc = torch.as_tensor(np.asarray(anchors)).to(dtype)
    if "anchor_shift" in mutate:
        anc = torch.roll(anc, 1, dims=1)
    R = dfl.numel()
    assert box.shape[1] == 4 * R and anc.shape == (2, H * W)
    dist = (torch.softmax(box.reshape(N, 4, R, H * W), dim=2) * dfl.view(1, 1, R, 1)).sum(dim=2)   # [N, 4, HW]: l, t, r, b
    x1y1, x2y2 = anc - dist[:, :2], anc + dist[:, 2:]
    xywh = torch.cat([(x1y1 + x2y2) / 2, x2y2 - x1y1], dim=1) * stride
    return torch.cat([xywh, torch.sigmoid(cls).reshape(N, -1, H * W)], dim=1).numpy()


@torch.no_grad()
def head_out0(feat, level, anchors, stride, dfl_w, round_mid, round_logits, mutate=(), round_weights=True):
    """out0 of one level, ``[N, 4 + nc, H * W]`` float64, of the map ``feat`` ``[N, Cin, H, W]`` (used as given).  ``level``: one entry
    of ``find_heads``; ``anchors``: ``[2, H * W]`` (grid units); flags and mutations as in the module docstring."""
    return _head(feat, level, anchors, stride, dfl_w, round_mid, round_logits, mutate, round_weights, torch.float64, False)


@torch.no_grad()
def standin_out0(feat, level, anchors, stride, dfl_w, round_logits=False):
    """A stand-in for a correct fp16 kernel: the same head in fp32, the 3x3 convs summed tap by tap (another K order than
    conv2d's), fp16 weights and fp16 intermediates."""
    return _head(feat, level, anchors, stride, dfl_w, True, round_logits, (), True, torch.float32, True).astype(np.float64)


def row_groups(out0, stride):
    """The two row groups of a level's out0: box rows in grid cells, score rows."""
    out0 = np.asarray(out0, np.float64)
    return {"box": out0[:, :4] / stride, "score": out0[:, 4:]}


# mean(d) <= MEAN_CAP * mean(e): see test_gpu_head_float64.py for the measurements it comes from
MEAN_CAP = 0.25
# the cost of fp16 storage must be visible in the reference pair, or the caps below say nothing
MIN_MAX_E = {"box": 1e-4, "score": 1e-5}


def measure(got, r_exact, r_emul, stride):
    """Per row group: e = |r_emul - r_exact| (what fp16 storage itself costs; nothing of the code under test enters) and
    d = |got - r_emul|, as ``{"max_e", "mean_e", "max_d", "mean_d"}``."""
    g, x, m = row_groups(got, stride), row_groups(r_exact, stride), row_groups(r_emul, stride)
    out = {}
    for k in ("box", "score"):
        e, d = np.abs(m[k] - x[k]), np.abs(g[k] - m[k])
        out[k] = {"max_e": float(e.max()), "mean_e": float(e.mean()), "max_d": float(d.max()), "mean_d": float(d.mean())}
    return out


def broken_caps(stats, mean_cap):
    """The caps a measurement breaks, as a list of messages (empty: within both).
    Per element: d <= 2 max(e) -- the code under test differs from the emulation by fp32 summation order, the hardware's
    transcendentals and the roundings these flip; a flipped rounding moves an activation by one fp16 ulp, twice the largest
    single rounding error e is made of.  Mean: mean(d) <= mean_cap * mean(e) -- flips are rare."""
    out = []
    for k, s in stats.items():
        if not (np.isfinite(s["max_d"]) and s["max_d"] <= 2 * s["max_e"]):
            out.append(f"{k}: max d {s['max_d']:.3e} > 2 max e = {2 * s['max_e']:.3e}")
        if not (np.isfinite(s["mean_d"]) and s["mean_d"] <= mean_cap * s["mean_e"]):
            out.append(f"{k}: mean d {s['mean_d']:.3e} > {mean_cap} mean e = {mean_cap * s['mean_e']:.3e}")
    return out


def fmt(stats):
    return "; ".join(f"{k}: e max {s['max_e']:.2e} mean {s['mean_e']:.2e}, d max {s['max_d']:.2e} mean {s['mean_d']:.2e}, "
                     f"d/e max {s['max_d'] / s['max_e']:.3f} mean {s['mean_d'] / s['mean_e']:.4f}" for k, s in stats.items())

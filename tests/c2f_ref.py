"""Float64 restatement of the span of the graph ONE launch of c2f_kernels.hip covers (a whole C2f module with or without the
stride-2 conv in front and the SPPF behind, a stride-2 conv with or without its 1x1 tail, the one-launch SPPF), for the tests
that pin those fp16 launches to their own HBM input (test_c2f_ref_cpu.py, test_gpu_c2f_float64.py).  Plain torch / NumPy on
``oracle.ncnn_ref.load_model`` layers; nothing of the package under test is imported.

    launch_convs(layer_string, layers)   the Convolution layers of a launch, from the profile's ``layer`` field
    span(layers, convs)                  the launch's output blob, its cut blobs (what it reads from HBM) and the layers between
    eval_span / standin_span             cut blobs -> output blob, float64 / fp32 in another summation order

Rounding points (``round_act``), read off the kernels.  Every sum is fp32 on the device (MFMA accumulators), float64 here.

  weights      fp16, once: a property of the stored model (``pack_phase`` of c2f_plan.h packs every fragment as halfs).  Biases stay fp32: they
               are added to the fp32 accumulators (``silu4(acc[t][i], bv[t])``: ``v = v + b``).
  Swish        every Swish output, fp16 round-to-nearest-even.  c2f_kernel: each epilogue converts its SiLU values with
               ``to_half<NT>(v, h)`` before the store -- the entry conv's x (``GlobalEpi``: ``store_h<NT>(base + ..)``), cv1's y0 | y1
               (``store_h<NT>(P0 + (fy * LW + fx) * PS0 + chb * 2, h)`` and the concat buffer), a_k (``epi_a``: ``store_h<NT>(P1
               + ..)``), cv2 (``epi_cv2``: ``store_h<NT>(out + ..)``; the whole-image configurations also put those halfs back
               into the planes: "the output (2c = COUT channels) also replaces y_NB | y_{NB+1} in the planes -- SPPF.cv1's
               input"), SPPF.cv1's s (``store_h<NT>(P0 + ((rg.fy0 + py) * LW + rg.fx0 + px) * PS + chb * 2, h)``) and SPPF.cv2
               (``store_h<NT>(out2 + ..)``).
               s2conv_kernel: the same ``GlobalEpi``, ``to_half<NT>(v, h)`` then ``store_h<NT>(base + ..)``.
               s2lds_kernel: ``for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]); .. to_half<NT>(v, hh);`` and, with
               the 1x1 tail, "out2 = silu(W2 . fp16(silu(conv)) + b2)": ``bq[0][j] = hh[j]`` is the B operand of the tail's
               MFMA, ``v[t] = silu4(o, b2v[t]); .. to_half<NT>(v, hh);`` its output.
               sppf_kernel: cv1 ``to_half<NT>(v, h); if (ok) store_h<NT>(P0 + (py * LW + px) * PS + chb * 2, h);`` and cv2
               ``v[t] = silu4(acc[t][i], bv[t]); .. to_half<NT>(v, h);``.
  add          every BinaryOp add output, fp16: ``epi_b`` computes ``h[4 * t + q] = (half_t)((float)(half_t)v[t][q] +
               (float)r[4 * t + q])`` -- "silu rounded to fp16, shortcut added in fp32, rounded again" (the sum of two halfs is
               exact in fp32 and in float64, so one rounding of the exact sum is the same number).
  no rounding  Slice, Split, Concat (addresses), the nearest-x2 Interp (``pw_phase<.., CFG::UP, ..>`` gathers the half-resolution
               source) and the 5x5 max pools (``pool_inplace``: maxima of halfs are halfs).

Mutations (``mutate=``; applied to this reference only, never to a kernel): errors of the kind a tiled kernel makes, which
test_c2f_ref_cpu.py uses to show that the caps of ``broken_caps`` would catch them.  ``mutations_for`` names those a span has
the layers for.

Budget (``measure`` / ``broken_caps``, as tests/head_ref.py, on activation values, one group per launch):
    e = |R_emul - R_exact|, d = |got - R_emul|;  every d <= 2 max(e);  mean(d) <= MEAN_CAP mean(e);  max(e) >= MIN_MAX_E.
MIN_MAX_E = 2**-11, half an fp16 ulp of a value in [1, 2): the exporter's modules have outputs of absmax 3.5 to 8.3, so the
rounding of the output alone gives max e of 9.8e-4 to 3.3e-3; a smaller max e says the reference pair does not differ by the
output's own rounding and the caps say nothing.
MEAN_CAP = 0.5: see test_c2f_ref_cpu.py for the stand-in's ratios it comes from.
"""
import math
import re

import numpy as np
import torch
import torch.nn.functional as F

from head_ref import broken_caps, round_fp16  # noqa: F401  (broken_caps is re-exported: the caps are the head's)

MUTATIONS = (
    "b2_tap02_col19",    # tap (0, 2) of the last bottleneck's second conv dropped on output columns x % 20 == 19 (a tile's last column)
    "b2_tap20_row15",    # tap (2, 0) of the same conv dropped on output rows y % 16 == 15 (the last row of a 16-row tile)
    "b2_tap20_row9",     # ... and on rows y % 10 == 9 (10-row tiles, half-image tiles of the 20 x 20 map)
    "cat_swap_y1y2",     # segments y1 and y2 exchanged in cv2's concat
    "add_skip_hi",       # the last bottleneck's shortcut add left out on channels >= c / 2
    "up_shift",          # the upsampled segment read at ((y + 1) // 2, (x + 1) // 2)
    "s2_pad_centre",     # the stride-2 conv's top-left padding taps read the centre pixel instead of zero
    "pool2_3x3_border",  # the second pool takes a 3 x 3 window on the border rows
    "cat_img_swap01",    # images 0 and 1 exchanged in the second operand of the concat in front of cv1
)
MEAN_CAP = 0.5
MIN_MAX_E = 2.0 ** -11
WALKED = ("Swish", "BinaryOp", "Pooling", "Concat", "Slice", "Split", "Interp")


def launch_convs(layer_string, layers):
    """The Convolution layers (graph order) a launch covers, from the ``layer`` field of its profile entry: ``a..b`` is a range in
    file order, ``+`` joins pieces, ``+sppf`` stands for the two convolutions that follow in file order, ``pools`` for none."""
    convs = [L for L in layers if L.type == "Convolution"]
    pos = {L.name: i for i, L in enumerate(convs)}
    picked = []
    for piece in layer_string.split("+"):
        if piece == "pools":
            continue
        if piece == "sppf":
            assert picked, layer_string
            picked += [picked[-1] + 1, picked[-1] + 2]
            continue
        m = re.fullmatch(r"(conv_\d+)(?:\.\.(conv_\d+))?", piece)
        assert m and m.group(1) in pos and (m.group(2) is None or m.group(2) in pos), f"cannot parse {layer_string!r}"
        a = pos[m.group(1)]
        b = pos[m.group(2)] if m.group(2) else a
        assert a <= b, layer_string
        picked += list(range(a, b + 1))
    assert picked == sorted(set(picked)) and picked[-1] < len(convs), layer_string
    return [convs[i] for i in picked]


def span(layers, convs):
    """``{"out": blob, "cuts": [blobs, graph order], "inside": [layers between, graph order]}`` of a launch: the output blob is the
    Swish output of the last convolution of the set; walking back from it, Swish, BinaryOp, Pooling, Concat, Slice, Split and Interp
    and the convolutions of the set are walked through, and the Swish output of a convolution outside the set (or the output of an
    add that sums one) is a cut blob -- what the launch reads from HBM."""
    prod = {o: L for L in layers for o in L.outputs}
    order = {id(L): i for i, L in enumerate(layers)}
    inset = {id(L) for L in convs}
    cons = {}
    for L in layers:
        for i in L.inputs:
            cons.setdefault(i, []).append(L)

    def swish_of(conv):
        nxt = cons.get(conv.outputs[0], [])
        assert len(nxt) == 1 and nxt[0].type == "Swish", f"{conv.name}: not followed by one Swish"
        return nxt[0]

    def conv_behind(blob):   # the convolution whose Swish output `blob` is a copy of, or None
        L = prod[blob]
        while L.type == "Split":
            L = prod[L.inputs[0]]
        if L.type != "Swish":
            return None
        c = prod[L.inputs[0]]
        return c if c.type == "Convolution" else None

    def outside(L):   # a Swish or an add that belongs to a launch in front
        if L.type == "Swish":
            return id(prod[L.inputs[0]]) not in inset
        if L.type == "BinaryOp":
            return not any(conv_behind(i) is not None and id(conv_behind(i)) in inset for i in L.inputs)
        return False

    out = swish_of(convs[-1]).outputs[0]
    cuts, inside, seen, todo = {}, {}, set(), [out]
    while todo:
        b = todo.pop()
        if b in seen:
            continue
        seen.add(b)
        L = prod[b]
        if outside(L):
            cuts[b] = order[id(L)]
            continue
        assert L.type in WALKED or (L.type == "Convolution" and id(L) in inset), f"blob {b}: {L.type} {L.name} is not part of a launch's span"
        inside[id(L)] = L
        todo += list(L.inputs)
    missing = [c.name for c in convs if id(c) not in inside]
    assert not missing, f"convolutions {missing} are not reached from blob {out}"
    return {"out": out, "cuts": sorted(cuts, key=cuts.get), "inside": sorted(inside.values(), key=lambda L: order[id(L)])}


def _roles(layers, sp):
    """The layers the mutations name, from the span's structure (None where the span has none)."""
    prod = {o: L for L in layers for o in L.outputs}
    inside = sp["inside"]
    ids = {id(L) for L in inside}

    def through_split(b):
        while prod[b].type == "Split":
            b = prod[b].inputs[0]
        return b

    r = dict(b2=None, add=None, cat=None, interp=None, s2=None, pool2=None, cat_in=None)
    adds = [L for L in inside if L.type == "BinaryOp"]
    if adds:
        r["add"] = adds[-1]
        for i in adds[-1].inputs:   # the operand that is a conv's Swish output: the bottleneck's second conv
            L = prod[through_split(i)]
            if L.type == "Swish" and prod[L.inputs[0]].type == "Convolution" and id(prod[L.inputs[0]]) in ids:
                r["b2"] = prod[L.inputs[0]]
                r["add_short"] = [j for j in adds[-1].inputs if j != i][0]
        # cv2's concat: the one that takes the last add's output
        r["cat"] = [L for L in inside if L.type == "Concat" and any(through_split(i) == adds[-1].outputs[0] for i in L.inputs)][0]
    ups = [L for L in inside if L.type == "Interp"]
    r["interp"] = ups[0] if ups else None
    s2 = [L for L in inside if L.type == "Convolution" and int(L.params.get(3, 1)) == 2]
    r["s2"] = s2[0] if s2 else None
    pools = [L for L in inside if L.type == "Pooling"]
    r["pool2"] = pools[1] if len(pools) >= 2 else None
    cin = [L for L in inside if L.type == "Concat" and len(L.inputs) == 2 and through_split(L.inputs[1]) in sp["cuts"]]
    r["cat_in"] = cin[0] if cin else None
    return r


def mutations_for(layers, convs, width=None):
    """The mutations the span of ``convs`` has the layers for.  ``width``: of the output map; on a map no wider than 20 the tap that
    b2_tap02_col19 drops reads the zero padding (column 19 is the last), so the mutation changes nothing and is left out."""
    r = _roles(layers, span(layers, convs))
    out = []
    if r["b2"] is not None:
        out += ["b2_tap02_col19"] if width is None or width > 20 else []
        out += ["b2_tap20_row15", "b2_tap20_row9", "cat_swap_y1y2", "add_skip_hi"]
    if r["interp"] is not None:
        out.append("up_shift")
    if r["s2"] is not None:
        out.append("s2_pad_centre")
    if r["pool2"] is not None:
        out.append("pool2_3x3_border")
    if r["cat_in"] is not None:
        out.append("cat_img_swap01")
    return out


def _eval(layers, convs, inputs, round_act, keep, mutate, round_weights, dtype, standin):
    mutate = (mutate,) if isinstance(mutate, str) else tuple(mutate or ())
    assert all(m in MUTATIONS for m in mutate), mutate
    sp = span(layers, convs)
    assert set(sp["cuts"]) <= set(inputs), f"cut blobs {sp['cuts']} needed, {sorted(inputs)} given"
    prod = {o: L for L in layers for o in L.outputs}
    roles = _roles(layers, sp) if mutate else {}
    assert all(m in mutations_for(layers, convs) for m in mutate), f"{mutate}: not applicable to this span"
    ids = {id(L) for L in sp["inside"]}
    val = {c: torch.as_tensor(np.asarray(inputs[c])).to(dtype) for c in sp["cuts"]}

    def act(t):
        return round_fp16(t) if round_act else t

    def conv(L, x):
        w = torch.from_numpy(L.weight)
        if round_weights:
            w = round_fp16(w)
        w, b = w.to(dtype), torch.from_numpy(L.bias).to(dtype)
        k, s = int(L.params.get(1, 1)), int(L.params.get(3, 1))
        assert w.shape[2:] == (k, k) and k in (1, 3) and s in (1, 2) and int(L.params.get(4, 0)) == k // 2 and (k == 3 or s == 1), L.name
        N, _, H, W = x.shape
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        if k == 1:
            if not standin:
                return F.conv2d(x, w, b)
            h = w.shape[1] // 2   # the K axis in two halves, second half first
            return (F.conv2d(x[:, h:], w[:, h:]) + F.conv2d(x[:, :h], w[:, :h])) + b.view(1, -1, 1, 1)
        xp = F.pad(x, (1, 1, 1, 1))

        def tap(ky, kx, src=None):
            src = xp if src is None else src
            return F.conv2d(src[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s], w[:, :, ky:ky + 1, kx:kx + 1])

        if standin:
            y = b.view(1, -1, 1, 1).expand(N, -1, Ho, Wo).clone()
            for ky in range(3):
                for kx in range(3):
                    y += tap(ky, kx)
        else:
            y = F.conv2d(x, w, b, stride=s, padding=1)
        if L is roles.get("b2"):
            col = (torch.arange(Wo) % 20 == 19).view(1, 1, 1, Wo).to(dtype)
            for m, (ky, kx), mask in (("b2_tap02_col19", (0, 2), col),
                                      ("b2_tap20_row15", (2, 0), (torch.arange(Ho) % 16 == 15).view(1, 1, Ho, 1).to(dtype)),
                                      ("b2_tap20_row9", (2, 0), (torch.arange(Ho) % 10 == 9).view(1, 1, Ho, 1).to(dtype))):
                if m in mutate:
                    y = y - tap(ky, kx) * mask
        if L is roles.get("s2") and "s2_pad_centre" in mutate:
            # output row 0: the taps of kernel row 0 lie in the padding; output column 0: those of kernel column 0.  Each reads its
            # window's centre pixel x[2 oy, 2 ox] instead of zero (the corner tap belongs to both and is counted once)
            cn = x[:, :, ::2, ::2][:, :, :Ho, :Wo]
            y = y.clone()
            y[:, :, 0, :] += F.conv2d(cn, w[:, :, 0:1, :].sum(3, keepdim=True))[:, :, 0, :]
            y[:, :, :, 0] += F.conv2d(cn, w[:, :, :, 0:1].sum(2, keepdim=True))[:, :, :, 0]
            y[:, :, 0, 0] -= F.conv2d(cn, w[:, :, 0:1, 0:1])[:, :, 0, 0]
        return y

    def silu(x):
        if standin:
            return x / (1 + torch.exp2(-x * math.log2(math.e)))
        return x * torch.sigmoid(x)

    def pool(L, x):
        assert (int(L.params.get(0, 0)), int(L.params.get(1)), int(L.params.get(2, 1)), int(L.params.get(3, 0))) == (0, 5, 1, 2), L.name
        y = F.max_pool2d(x, 5, 1, 2)
        if L is roles.get("pool2") and "pool2_3x3_border" in mutate:
            y3 = F.max_pool2d(x, 3, 1, 1)
            y = y.clone()
            y[:, :, 0], y[:, :, -1] = y3[:, :, 0], y3[:, :, -1]
        return y

    def get(b):
        if b in val:
            return val[b]
        L = prod[b]
        assert id(L) in ids, f"blob {b} lies outside the span"
        ins = [get(i) for i in L.inputs]
        if L.type == "Convolution":
            val[b] = conv(L, ins[0])
        elif L.type == "Swish":
            val[b] = act(silu(ins[0]))
        elif L.type == "Split":
            for o in L.outputs:
                val[o] = ins[0]
        elif L.type == "Slice":
            assert int(L.params.get(1, 0)) == 0 and all(s > 0 for s in L.params[0]), L.name
            for o, part in zip(L.outputs, torch.split(ins[0], list(L.params[0]), dim=1)):
                val[o] = part
        elif L.type == "Concat":
            assert int(L.params.get(0, 0)) == 0, L.name
            if L is roles.get("cat") and "cat_swap_y1y2" in mutate:
                ins[1], ins[2] = ins[2], ins[1]
            if L is roles.get("cat_in") and "cat_img_swap01" in mutate:
                ins[1] = ins[1][[1, 0] + list(range(2, ins[1].shape[0]))]
            val[b] = torch.cat(ins, dim=1)
        elif L.type == "BinaryOp":
            assert int(L.params.get(0, 0)) == 0 and len(ins) == 2 and not int(L.params.get(1, 0)), L.name
            y = ins[0] + ins[1]
            if L is roles.get("add") and "add_skip_hi" in mutate:
                branch = ins[1] if L.inputs[0] == roles["add_short"] else ins[0]
                y = y.clone()
                y[:, y.shape[1] // 2:] = branch[:, y.shape[1] // 2:]
            val[b] = act(y)
        elif L.type == "Pooling":
            val[b] = pool(L, ins[0])
        elif L.type == "Interp":
            assert (int(L.params.get(0, 0)), float(L.params.get(1, 1.0)), float(L.params.get(2, 1.0))) == (1, 2.0, 2.0), L.name
            x = ins[0]
            H, W = x.shape[2:]
            yy, xx = torch.arange(2 * H), torch.arange(2 * W)
            if L is roles.get("interp") and "up_shift" in mutate:
                yy, xx = ((yy + 1) // 2).clamp(max=H - 1), ((xx + 1) // 2).clamp(max=W - 1)
            else:
                yy, xx = yy // 2, xx // 2
            val[b] = x[:, :, yy][:, :, :, xx]
        else:
            raise AssertionError(f"{L.type} {L.name}: not an op of a launch's span")
        return val[b]

    out = get(sp["out"]).to(torch.float64).numpy()
    if not keep:
        return out
    return out, {k: get(k).to(torch.float64).numpy() for k in keep}


@torch.no_grad()
def eval_span(layers, convs, inputs, round_act, keep=(), mutate=(), round_weights=True):
    """The output blob of the span of ``convs``, float64 ``[N, C, H, W]``, from its cut blobs ``inputs`` = ``{blob name: array}`` (used as
    given), demand-driven.  ``round_act``: the kernel's rounding points (module docstring).  With ``keep``: ``(out, {name: blob})``."""
    return _eval(layers, convs, inputs, round_act, tuple(keep), mutate, round_weights, torch.float64, False)


@torch.no_grad()
def standin_span(layers, convs, inputs, keep=()):
    """A stand-in for a correct fp16 kernel: the same span in fp32 with other summation orders -- the 3x3 convs tap by tap, the K axis of
    the 1x1 convs in two halves, second half first, SiLU as x / (1 + exp2(-x log2 e)) -- fp16 weights and the same fp16 rounding points."""
    return _eval(layers, convs, inputs, True, tuple(keep), (), True, torch.float32, True)


def measure(got, r_exact, r_emul):
    """One group, "act": e = |r_emul - r_exact| (what fp16 storage itself costs; nothing of the code under test enters) and
    d = |got - r_emul|, with the share of elements of ``got`` that equal the emulation bit for bit."""
    g, x, m = (np.asarray(a, np.float64) for a in (got, r_exact, r_emul))
    assert g.shape == x.shape == m.shape, (g.shape, x.shape, m.shape)
    e, d = np.abs(m - x), np.abs(g - m)
    return {"act": {"max_e": float(e.max()), "mean_e": float(e.mean()), "max_d": float(d.max()), "mean_d": float(d.mean()),
                    "equal": float((g == m).mean())}}


def check(stats, mean_cap=MEAN_CAP):
    """The messages of ``broken_caps`` plus the floor on max(e) (empty: the measurement is within the budget and the budget says something)."""
    out = list(broken_caps(stats, mean_cap))
    for k, s in stats.items():
        if not s["max_e"] >= MIN_MAX_E:
            out.append(f"{k}: max e {s['max_e']:.2e} < 2**-11: the budget is vacuous")
    return out


def fmt(stats):
    s = stats["act"]
    return (f"max e {s['max_e']:.2e} mean e {s['mean_e']:.2e} max d {s['max_d']:.2e} mean d {s['mean_d']:.2e} "
            f"d/e max {s['max_d'] / s['max_e']:.3f} mean {s['mean_d'] / s['mean_e']:.4f} equal {100 * s['equal']:.2f}%")

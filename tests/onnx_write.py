"""Test helper: write an NCNN detector model as the ONNX file an exporter would have written for it (no `onnx` package).

The graph in front of the Detect tail is translated layer by layer from the NCNN model (``litepi.ncnn_io.read_param_layers``
plus the ``.bin``): Convolution -> Conv, Swish -> Sigmoid + Mul, Slice -> Split, BinaryOp add -> Add, Pooling -> MaxPool,
Interp -> Resize, NCNN's Split layers disappear (an ONNX tensor simply has several readers).  The Detect tail is written the way
the exporter traces ``Detect.forward``: per level Concat -> Reshape, Concat over the anchors, Split into box and class rows, the
DFL (Reshape, Transpose, Softmax, Transpose, Conv, Reshape), the two Slices, Sub / Add / Add / Sub / Div / Concat with the anchor
table as a (1, 2, A) initializer, Mul by the (1, A) stride table, Sigmoid, Concat.  Weights are copied bit for bit.

``opset=12`` writes what the reference's own export holds: ``split`` as an attribute, every constant an initializer in
``raw_data``, ``Softmax`` with its axis.  ``opset=17`` writes what a current exporter leaves: Split sizes, Resize scales and
Reshape shapes come from ``Constant`` nodes, ``Softmax`` relies on the default axis, and biases and integer constants use the
typed repeated fields (``float_data`` / ``int64_data``).

``test_onnx_cpu.test_writer_matches_authentic_export`` keeps this honest: v1's NCNN model written here has the op-type counts
and the attribute names per op type of the reference's ``yolo_plus.onnx``.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from litepi.ncnn_io import read_param_layers

FLOAT, INT64 = 1, 7


# ---- protobuf wire format ---------------------------------------------------------------------------------------------------
def _varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _key(no: int, wt: int) -> bytes:
    return _varint(no << 3 | wt)


def _int(no: int, v: int) -> bytes:
    return _key(no, 0) + _varint(v)


def _bytes(no: int, b: bytes) -> bytes:
    return _key(no, 2) + _varint(len(b)) + b


def _str(no: int, s: str) -> bytes:
    return _bytes(no, s.encode())


def tensor(name: str, arr: np.ndarray, typed: bool = False) -> bytes:
    """TensorProto; typed: values in float_data / int64_data instead of raw_data."""
    arr = np.asarray(arr)
    dt = FLOAT if arr.dtype.kind == "f" else INT64
    out = b"".join(_int(1, int(d)) for d in arr.shape) + _int(2, dt)
    if typed and dt == FLOAT:
        out += _bytes(4, np.ascontiguousarray(arr, "<f4").tobytes())   # packed float_data
    elif typed:
        out += _bytes(7, b"".join(_varint(int(v)) for v in arr.ravel()))
    out += _str(8, name)
    if not typed:
        out += _bytes(9, np.ascontiguousarray(arr, "<f4" if dt == FLOAT else "<i8").tobytes())
    return out


def attr(name: str, value) -> bytes:
    out = _str(1, name)
    if isinstance(value, float):
        return out + _key(2, 5) + struct.pack("<f", value) + _int(20, 1)
    if isinstance(value, int):
        return out + _int(3, value) + _int(20, 2)
    if isinstance(value, str):
        return out + _bytes(4, value.encode()) + _int(20, 3)
    if isinstance(value, bytes):   # a TensorProto
        return out + _bytes(5, value) + _int(20, 4)
    return out + b"".join(_int(8, int(v)) for v in value) + _int(20, 7)


def node(op: str, name: str, inputs: Sequence[str], outputs: Sequence[str], **attrs) -> bytes:
    out = b"".join(_str(1, i) for i in inputs) + b"".join(_str(2, o) for o in outputs)
    if name:
        out += _str(3, name)
    out += _str(4, op)
    for k in sorted(attrs):
        out += _bytes(5, attr(k, attrs[k]))
    return out


def value_info(name: str, shape: Sequence[int]) -> bytes:
    dims = b"".join(_bytes(1, _int(1, int(d))) for d in shape)
    return _str(1, name) + _bytes(2, _bytes(1, _int(1, FLOAT) + _bytes(2, dims)))


def model(nodes: Sequence[bytes], inits: Sequence[bytes], inputs: Sequence[bytes], outputs: Sequence[bytes], opset: int) -> bytes:
    graph = b"".join(_bytes(1, n) for n in nodes) + _str(2, "main_graph") + b"".join(_bytes(5, t) for t in inits)
    graph += b"".join(_bytes(11, i) for i in inputs) + b"".join(_bytes(12, o) for o in outputs)
    return _int(1, 8) + _str(2, "onnx_write") + _bytes(7, graph) + _bytes(8, _str(1, "") + _int(2, opset))


# ---- the NCNN side -------------------------------------------------------------------------------------------------------------
def read_ncnn(param_path: str, bin_path: str) -> List[dict]:
    """read_param_layers plus each layer's weight / bias / data from the .bin."""
    layers = read_param_layers(param_path)
    with open(bin_path, "rb") as f:
        blob = f.read()
    off = 0
    for L in layers:
        p = L["params"]
        if L["type"] in ("Convolution", "ConvolutionDepthWise"):
            off += 4
            n = int(p[6])
            L["weight"] = np.frombuffer(blob, "<f4", n, off).copy()
            off += 4 * n
            if p.get(5, 0):
                L["bias"] = np.frombuffer(blob, "<f4", int(p[0]), off).copy()
                off += 4 * int(p[0])
        elif L["type"] == "MemoryData":
            n = max(int(p.get(0, 0)), 1) * max(int(p.get(1, 0)), 1) * max(int(p.get(2, 0)), 1)
            L["data"] = np.frombuffer(blob, "<f4", n, off).copy()
            off += 4 * n
    assert off == len(blob), (off, len(blob))
    return layers


class _Graph:
    def __init__(self, opset: int):
        self.opset, self.modern = opset, opset >= 13
        self.nodes: List[bytes] = []
        self.inits: List[bytes] = []
        self.n_const = 0

    def add(self, op: str, name: str, ins: Sequence[str], outs: Sequence[str], **attrs) -> None:
        self.nodes.append(node(op, name, ins, outs, **attrs))

    def init(self, name: str, arr: np.ndarray, typed: Optional[bool] = None) -> str:
        self.inits.append(tensor(name, arr, self.modern if typed is None else typed))
        return name

    def const(self, name: str, arr: np.ndarray) -> str:
        """a small constant a node takes as an input: an initializer (opset 12), an unfolded Constant node (opset 17)"""
        if not self.modern:
            return self.init(name, arr, typed=False)
        self.n_const += 1
        self.add("Constant", "", [], [name], value=tensor("", arr, typed=True))   # (nameless: the reader names it Constant_<index>)
        return name


def ncnn_to_onnx(param_path: str, bin_path: str, onnx_path: str, size, opset: int = 12, mutate=None) -> Dict[str, object]:
    """Write the NCNN model as ONNX.  size: the input size the model was exported at, an int or (rows, columns).
    mutate(graph): an optional hook the refusal tests use to spoil the graph before it is serialised."""
    H, W = (size, size) if isinstance(size, int) else size
    layers = read_ncnn(param_path, bin_path)
    producer = {o: L for L in layers for o in L["outputs"]}
    first_tail = next(i for i, L in enumerate(layers) if L["type"] == "Reshape" and producer[L["inputs"][0]]["type"] == "Concat")
    g = _Graph(opset)
    name: Dict[str, str] = {}   # NCNN blob -> ONNX tensor

    def t(blob: str) -> str:
        return name[blob]

    for L in layers[:first_tail]:
        ty, p, ln = L["type"], L["params"], L["name"]
        outs = L["outputs"]
        if ty == "Input":
            name[outs[0]] = "images"
        elif ty == "Split":   # NCNN's fan-out layer: the ONNX tensor just has several readers
            for o in outs:
                name[o] = t(L["inputs"][0])
        elif ty == "MemoryData":
            continue
        elif ty in ("Convolution", "ConvolutionDepthWise"):
            O, kw = int(p[0]), int(p.get(1, 1))
            kh = int(p.get(11, kw))
            group = int(p.get(7, 1))
            w = L["weight"].reshape(O, -1, kh, kw)
            ins = [t(L["inputs"][0]), g.init(ln + ".weight", w, typed=False)]
            if "bias" in L:
                ins.append(g.init(ln + ".bias", L["bias"]))
            name[outs[0]] = f"/{ln}/Conv_output_0"
            sw, pw, dw = int(p.get(3, 1)), int(p.get(4, 0)), int(p.get(2, 1))
            g.add("Conv", f"/{ln}/Conv", ins, [name[outs[0]]], dilations=[int(p.get(12, dw)), dw], group=group, kernel_shape=[kh, kw],
                  pads=[int(p.get(14, pw)), pw, int(p.get(14, pw)), pw], strides=[int(p.get(13, sw)), sw])
        elif ty == "Swish":
            x = t(L["inputs"][0])
            name[outs[0]] = f"/{ln}/Mul_output_0"
            g.add("Sigmoid", f"/{ln}/Sigmoid", [x], [f"/{ln}/Sigmoid_output_0"])
            g.add("Mul", f"/{ln}/Mul", [x, f"/{ln}/Sigmoid_output_0"], [name[outs[0]]])
        elif ty == "Slice":
            sizes = [int(v) for v in p[-23300]]
            for k, o in enumerate(outs):
                name[o] = f"/{ln}/Split_output_{k}"
            if g.modern:
                g.add("Split", f"/{ln}/Split", [t(L["inputs"][0]), g.const(f"/{ln}/Constant_output_0", np.array(sizes, np.int64))],
                      [name[o] for o in outs], axis=int(p.get(1, 0)) + 1)
            else:
                g.add("Split", f"/{ln}/Split", [t(L["inputs"][0])], [name[o] for o in outs], axis=int(p.get(1, 0)) + 1, split=sizes)
        elif ty == "Concat":
            name[outs[0]] = f"/{ln}/Concat_output_0"
            g.add("Concat", f"/{ln}/Concat", [t(i) for i in L["inputs"]], [name[outs[0]]], axis=int(p.get(0, 0)) + 1)
        elif ty == "BinaryOp":
            assert int(p.get(0, 0)) == 0 and len(L["inputs"]) == 2, L
            name[outs[0]] = f"/{ln}/Add_output_0"
            g.add("Add", f"/{ln}/Add", [t(i) for i in L["inputs"]], [name[outs[0]]])
        elif ty == "Pooling":
            assert int(p.get(0, 0)) == 0 and int(p.get(5, 0)) == 1, L
            k, s, pd = int(p[1]), int(p.get(2, 1)), int(p.get(3, 0))
            name[outs[0]] = f"/{ln}/MaxPool_output_0"
            g.add("MaxPool", f"/{ln}/MaxPool", [t(L["inputs"][0])], [name[outs[0]]], ceil_mode=0, dilations=[1, 1],
                  kernel_shape=[int(p.get(11, k)), k], pads=[int(p.get(13, pd)), pd, int(p.get(13, pd)), pd], strides=[int(p.get(12, s)), s])
        elif ty == "Interp":
            assert int(p.get(0, 0)) == 1, L
            name[outs[0]] = f"/{ln}/Resize_output_0"
            scales = g.const(f"/{ln}/Constant_output_0", np.array([1, 1, float(p[1]), float(p[2])], np.float32))
            roi = "" if g.modern else g.const(f"/{ln}/Constant_1_output_0", np.zeros(0, np.float32))
            g.add("Resize", f"/{ln}/Resize", [t(L["inputs"][0]), roi, scales], [name[outs[0]]], coordinate_transformation_mode="asymmetric",
                  cubic_coeff_a=-0.75, mode="nearest", nearest_mode="floor")
        else:
            raise ValueError(f"layer type {ty} in front of the Detect tail")

    # ---- the Detect tail, from what the NCNN tail holds: the level Concats, nc, reg_max, the tables
    tail = layers[first_tail:]
    all_cat = next(L for L in tail if L["type"] == "Concat" and all(producer[i]["type"] == "Reshape" for i in L["inputs"]))
    cats = [t(producer[i]["inputs"][0]) for i in all_cat["inputs"]]
    dfl = next(L for L in tail if L["type"] == "Convolution")
    reg_max = int(dfl["params"][6])
    nc = next(int(L["params"][-23300][1]) for L in tail if L["type"] == "Slice" and int(L["params"][-23300][0]) == 4 * reg_max)
    anchors = next(L["data"] for L in layers if L["type"] == "MemoryData" and int(L["params"].get(1, 0)) == 2)
    strides = next(L["data"] for L in layers if L["type"] == "MemoryData" and int(L["params"].get(1, 0)) == 0)
    A, no = strides.size, 4 * reg_max + nc
    D = "/detect"
    shape = g.const(f"{D}/Constant_output_0", np.array([1, no, -1], np.int64))
    rs = []
    for k, c in enumerate(cats):
        rs.append(f"{D}/Reshape_{k}_output_0")
        g.add("Reshape", f"{D}/Reshape_{k}", [c, shape], [rs[-1]])
    g.add("Concat", f"{D}/Concat_3", rs, [f"{D}/Concat_3_output_0"], axis=2)
    if g.modern:
        g.add("Split", f"{D}/Split", [f"{D}/Concat_3_output_0", g.const(f"{D}/Constant_1_output_0", np.array([4 * reg_max, nc], np.int64))],
              [f"{D}/box", f"{D}/cls"], axis=1)
    else:
        g.add("Split", f"{D}/Split", [f"{D}/Concat_3_output_0"], [f"{D}/box", f"{D}/cls"], axis=1, split=[4 * reg_max, nc])
    g.add("Reshape", f"{D}/dfl/Reshape", [f"{D}/box", g.const(f"{D}/dfl/Constant_output_0", np.array([1, 4, reg_max, A], np.int64))], [f"{D}/dfl/r0"])
    g.add("Sigmoid", f"{D}/Sigmoid", [f"{D}/cls"], [f"{D}/Sigmoid_output_0"])
    g.add("Transpose", f"{D}/dfl/Transpose", [f"{D}/dfl/r0"], [f"{D}/dfl/t0"], perm=[0, 3, 1, 2])
    if g.modern:
        g.add("Softmax", f"{D}/dfl/Softmax", [f"{D}/dfl/t0"], [f"{D}/dfl/s"])   # default axis -1
    else:
        g.add("Softmax", f"{D}/dfl/Softmax", [f"{D}/dfl/t0"], [f"{D}/dfl/s"], axis=3)
    g.add("Transpose", f"{D}/dfl/Transpose_1", [f"{D}/dfl/s"], [f"{D}/dfl/t1"], perm=[0, 3, 2, 1])
    g.add("Conv", f"{D}/dfl/conv/Conv", [f"{D}/dfl/t1", g.init("detect.dfl.conv.weight", dfl["weight"].reshape(1, reg_max, 1, 1), typed=False)],
          [f"{D}/dfl/c"], dilations=[1, 1], group=1, kernel_shape=[1, 1], pads=[0, 0, 0, 0], strides=[1, 1])
    g.add("Reshape", f"{D}/dfl/Reshape_1", [f"{D}/dfl/c", g.const(f"{D}/dfl/Constant_1_output_0", np.array([1, 4, A], np.int64))], [f"{D}/dist"])
    c0, c1, c2, c4 = (g.const(f"{D}/Constant_{k}_output_0", np.array([v], np.int64)) for k, v in ((4, 0), (3, 1), (5, 2), (6, 4)))
    g.add("Slice", f"{D}/Slice", [f"{D}/dist", c0, c2, c1], [f"{D}/lt"])
    g.add("Slice", f"{D}/Slice_1", [f"{D}/dist", c2, c4, c1], [f"{D}/rb"])
    a9 = g.init(f"{D}/Constant_9_output_0", anchors.reshape(1, 2, A), typed=False)
    a10 = g.init(f"{D}/Constant_10_output_0", anchors.reshape(1, 2, A), typed=False)
    g.add("Sub", f"{D}/Sub", [a9, f"{D}/lt"], [f"{D}/x1y1"])
    g.add("Add", f"{D}/Add_1", [a10, f"{D}/rb"], [f"{D}/x2y2"])
    g.add("Add", f"{D}/Add_2", [f"{D}/x1y1", f"{D}/x2y2"], [f"{D}/sum"])
    g.add("Sub", f"{D}/Sub_1", [f"{D}/x2y2", f"{D}/x1y1"], [f"{D}/wh"])
    g.add("Div", f"{D}/Div_1", [f"{D}/sum", g.init(f"{D}/Constant_11_output_0", np.array(2.0, np.float32), typed=False)], [f"{D}/cxy"])
    g.add("Concat", f"{D}/Concat_4", [f"{D}/cxy", f"{D}/wh"], [f"{D}/xywh"], axis=1)
    g.add("Mul", f"{D}/Mul_2", [f"{D}/xywh", g.init(f"{D}/Constant_12_output_0", strides.reshape(1, A), typed=False)], [f"{D}/scaled"])
    g.add("Concat", f"{D}/Concat_5", [f"{D}/scaled", f"{D}/Sigmoid_output_0"], ["output0"], axis=1)
    if mutate is not None:
        mutate(g)
    data = model(g.nodes, g.inits, [value_info("images", [1, 3, H, W])], [value_info("output0", [1, 4 + nc, A])], opset)
    with open(onnx_path, "wb") as f:
        f.write(data)
    return dict(nc=nc, reg_max=reg_max, num_anchors=A, bytes=len(data), constants=g.n_const)

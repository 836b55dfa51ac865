"""The ONNX reader (csrc/onnx_graph.cpp) without a device.

lp_detector_graph_describe prints the layers a model file lowers to, names left out.  An ONNX export and the NCNN export of the
same model must give the same layers in front of the Detect tail -- types, parameters, weight and bias CRCs, as a multiset -- and
the same anchor and stride tables: then the planner, which is structural, sees the same network.  Checked on the reference's own
export of the v1 checkpoint (when build() staged it) and on files tests/onnx_write.py makes from seeded NCNN models; the writer
itself is held to the authentic export (same op counts, same attribute names) and to the oracle's ONNX interpreter.  What the
reader refuses, it refuses with a status and the node's name; tests/native/onnx_parse_replay.cpp runs it over truncated and
corrupted files under AddressSanitizer and UBSan as a stand-alone program."""
import collections
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import onnx_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = os.path.join(ROOT, "oracle", "_ref")
V1_PARAM, V1_BIN, V1_ONNX = (os.path.join(_REF, "yolo_plus_v1." + ext) for ext in ("param", "bin", "onnx"))
needs_v1_onnx = pytest.mark.skipif(not (os.path.exists(V1_PARAM) and os.path.exists(V1_BIN) and os.path.exists(V1_ONNX)),
                                   reason="reference v1 NCNN + ONNX exports not staged (build() stages them when the reference is present)")
# a narrow network of the same topology: the files the refusal tests and the replay program chew on stay near 100 KB
TINY = dict(c=(8, 8, 8, 16, 16), n=(1, 2, 2, 1), f4=16, f3=8, d4conv=8, d4=16, d5conv=16, d5=16, head_box=16, head_cls=8)


def _backend():
    from litepi import _ffi, backend
    if not os.path.exists(_ffi.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return backend


def _split(lines):
    """(the layers in front of the Detect tail, the anchor / stride tables, the number of convolutions, the DFL included) of a description"""
    first = next(i for i, ln in enumerate(lines) if ln.startswith("Reshape "))
    front = collections.Counter(ln for ln in lines[:first] if not ln.startswith("MemoryData "))
    tables = collections.Counter(ln for ln in lines if ln.startswith("MemoryData "))
    return front, tables, sum(ln.startswith("Convolution ") for ln in lines)


def _same_network(onnx_path, param, binf):
    b = _backend()
    got, want = b.detector_graph_describe(onnx_path), b.detector_graph_describe(param, binf)
    (gf, gt, gc), (wf, wt, wc) = _split(got), _split(want)
    assert gf == wf, f"only from ONNX: {sorted((gf - wf).elements())[:6]}; only from NCNN: {sorted((wf - gf).elements())[:6]}"
    assert gt == wt and len(gt) == 2 and sum(gt.values()) == 3   # the anchor table twice (its two readers), the stride table once
    assert gc == wc
    # the planner takes everything from the first head Reshape on as the tail: the DFL convolution must be behind it, and no other
    first = next(i for i, ln in enumerate(got) if ln.startswith("Reshape "))
    assert sum(ln.startswith("Convolution ") for ln in got[first:]) == 1
    return got, gc


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from litepi import ncnn_export
    d = tmp_path_factory.mktemp("tiny")
    p, b = str(d / "tiny.param"), str(d / "tiny.bin")
    ncnn_export.export_detector(p, b, spec=TINY, seed=3, size=64)
    return d, p, b


@needs_v1_onnx
def test_authentic_v1_export_lowers_to_its_ncnn_layers():
    got, convs = _same_network(V1_ONNX, V1_PARAM, V1_BIN)
    assert convs == 64
    # the CRCs are zlib's, of the fp32 bytes: the stem's weight as the oracle's initializer reader sees it
    import zlib
    from oracle import onnx_init
    w = onnx_init.read_initializers(V1_ONNX)["model.0.conv.weight"]
    assert any(ln.startswith("Convolution ") and f" {zlib.crc32(w.tobytes()):08x} " in ln for ln in got)


_models = {}


@pytest.mark.parametrize("opset", [12, 17])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("size", [320, (224, 416)], ids=["320", "224x416"])
@pytest.mark.parametrize("preset", ["v1", "v2"])
def test_writer_made_export_lowers_to_its_ncnn_twin(preset, size, nc, opset, tmp_path_factory):
    from litepi import ncnn_export
    key = (preset, size, nc)
    if key not in _models:
        d = tmp_path_factory.mktemp("m")
        _models[key] = (str(d / "m.param"), str(d / "m.bin"), d)
        ncnn_export.export_detector(*_models[key][:2], preset, seed=11, nc=nc, size=size)
    p, b, d = _models[key]
    o = str(d / f"m{opset}.onnx")
    info = onnx_write.ncnn_to_onnx(p, b, o, size, opset=opset)
    assert info["nc"] == nc and (info["constants"] > 0) == (opset == 17)
    _same_network(o, p, b)


@needs_v1_onnx
def test_writer_matches_authentic_export(tmp_path):
    """v1's NCNN model written by onnx_write has the op-type counts and, per op type, the attribute names of the reference's export"""
    from oracle import onnx_ref

    def stats(path):
        nodes = onnx_ref.read_graph(path)[0]
        names = {}
        for n in nodes:
            names.setdefault(n.op, set()).update(n.attrs)
        return collections.Counter(n.op for n in nodes), names

    o = str(tmp_path / "v1.onnx")
    onnx_write.ncnn_to_onnx(V1_PARAM, V1_BIN, o, 640, opset=12)
    assert stats(o) == stats(V1_ONNX)
    assert stats(V1_ONNX)[0]["Conv"] == 64


def test_writer_made_export_means_what_the_ncnn_model_means(tiny):
    """the oracle's ONNX interpreter (opset 12) on the written file against the oracle's NCNN interpreter on the model it was
    written from: the writer is a translation, not a second opinion of the loader's.  The opset-17 file holds the same network
    in the newer forms: it must lower to the same layers, in the same order."""
    import torch
    from oracle import ncnn_ref, onnx_ref
    d, p, b = tiny
    o, o17 = str(d / "tiny12.onnx"), str(d / "tiny17.onnx")
    onnx_write.ncnn_to_onnx(p, b, o, 64, opset=12)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    want = ncnn_ref.run_graph(ncnn_ref.load_model(p, b), x)["out0"].numpy()
    got = onnx_ref.forward(o, x).numpy()
    assert got.shape == want.shape == (1, 5, 84)
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, float(np.abs(want).max()))   # two fp32 evaluation orders of one network
    onnx_write.ncnn_to_onnx(p, b, o17, 64, opset=17)
    same = [[ln for ln in _backend().detector_graph_describe(f) if not ln.startswith("Softmax ")] for f in (o, o17)]   # (axis 3 and the default, -1)
    assert same[0] == same[1]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refused(path, code, *words):
    from litepi import _ffi
    with pytest.raises(_ffi.LitepiError) as ei:
        _backend().detector_graph_describe(path)
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_truncated_files_are_refused(tiny):
    from litepi import _ffi
    d, p, b = tiny
    o = str(d / "whole.onnx")
    n = onnx_write.ncnn_to_onnx(p, b, o, 64)["bytes"]
    data = open(o, "rb").read()
    assert len(_backend().detector_graph_describe(o)) > 100
    for k, cut in enumerate([0, 1, 7, 100, 1000, n // 3, n // 2, n - 5000, n - 100, n - 1]):
        c = str(d / f"cut{k}.onnx")
        with open(c, "wb") as f:
            f.write(data[:cut])
        _refused(c, _ffi.LP_ERR_GRAPH)


def test_missing_file_is_an_io_error(tmp_path):
    from litepi import _ffi
    _refused(str(tmp_path / "nothing.onnx"), _ffi.LP_ERR_IO, "nothing.onnx")


def test_unknown_operator_is_refused_by_name(tiny):
    from litepi import _ffi
    d, p, b = tiny

    def splice(g):   # ... -> Concat_5 -> Erf -> output0
        g.nodes[-1] = onnx_write.node("Concat", "/detect/Concat_5", ["/detect/scaled", "/detect/Sigmoid_output_0"], ["/detect/pre"], axis=1)
        g.add("Erf", "/spoiled/Erf", ["/detect/pre"], ["output0"])
    o = str(d / "erf.onnx")
    onnx_write.ncnn_to_onnx(p, b, o, 64, mutate=splice)
    _refused(o, _ffi.LP_ERR_GRAPH, "/spoiled/Erf", "op Erf")

    def nameless(g):   # a node without a name is called <op>_<its index in the file>
        splice(g)
        g.nodes[-1] = onnx_write.node("Erf", "", ["/detect/pre"], ["output0"])
        nameless.index = len(g.nodes) - 1
    onnx_write.ncnn_to_onnx(p, b, o, 64, mutate=nameless)
    _refused(o, _ffi.LP_ERR_GRAPH, f"node Erf_{nameless.index} (op Erf)")


def test_dilated_convolution_is_refused_by_name(tiny):
    from litepi import _ffi
    d, p, b = tiny

    def dilate(g):
        g.nodes[0] = onnx_write.node("Conv", "/conv_0/Conv", ["images", "conv_0.weight", "conv_0.bias"], ["/conv_0/Conv_output_0"],
                                     dilations=[2, 2], group=1, kernel_shape=[3, 3], pads=[2, 2, 2, 2], strides=[2, 2])
    o = str(d / "dil.onnx")
    onnx_write.ncnn_to_onnx(p, b, o, 64, mutate=dilate)
    _refused(o, _ffi.LP_ERR_GRAPH, "/conv_0/Conv", "op Conv", "dilation 2x2")

    def lopsided(g):
        g.nodes[0] = onnx_write.node("Conv", "/conv_0/Conv", ["images", "conv_0.weight", "conv_0.bias"], ["/conv_0/Conv_output_0"],
                                     dilations=[1, 1], group=1, kernel_shape=[3, 3], pads=[0, 0, 1, 1], strides=[2, 2])
    onnx_write.ncnn_to_onnx(p, b, o, 64, mutate=lopsided)
    _refused(o, _ffi.LP_ERR_GRAPH, "/conv_0/Conv", "asymmetric pads")


def test_fp16_initializer_is_refused_by_name(tiny):
    from litepi import _ffi
    d, p, b = tiny

    def halve(g):   # the stem's weight as FLOAT16 (data type 10)
        w = np.zeros((8, 3, 3, 3), np.float16)
        t = b"".join(onnx_write._int(1, int(k)) for k in w.shape) + onnx_write._int(2, 10) + onnx_write._str(8, "conv_0.weight")
        g.inits[0] = t + onnx_write._bytes(9, w.tobytes())
    o = str(d / "half.onnx")
    onnx_write.ncnn_to_onnx(p, b, o, 64, mutate=halve)
    _refused(o, _ffi.LP_ERR_GRAPH, "/conv_0/Conv", "element type 10", "fp32")


def test_dynamic_shape_chain_is_refused_by_name(tiny):
    from litepi import _ffi
    d, p, b = tiny
    o = str(d / "shape.onnx")
    onnx_write.ncnn_to_onnx(p, b, o, 64, mutate=lambda g: g.add("Shape", "/detect/Shape", ["images"], ["/detect/Shape_output_0"]))
    _refused(o, _ffi.LP_ERR_GRAPH, "/detect/Shape", "static input shape")


# ---- the reader under the sanitizers, as a stand-alone program ---------------------------------------------------------------------
def test_onnx_parse_replay_native(tiny, tmp_path):
    """tests/native/onnx_parse_replay.cpp: the intact file, every prefix in 997-byte steps and 2000 seeded single-byte corruptions
    through the reader, host code only, under -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d, p, b = tiny
    o = str(d / "replay.onnx")
    onnx_write.ncnn_to_onnx(p, b, o, 64, opset=17)
    exe = str(tmp_path / "onnx_parse_replay")
    csrc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "onnx_parse_replay.cpp"), os.path.join(csrc, "onnx_graph.cpp"), os.path.join(csrc, "ncnn_graph.cpp")]
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    objs = [str(tmp_path / (os.path.basename(c) + ".o")) for c in srcs]
    jobs = [subprocess.Popen(["g++", *flags, "-c", c, "-o", ob]) for c, ob in zip(srcs, objs)]   # the three units side by side
    assert [j.wait(timeout=300) for j in jobs] == [0, 0, 0]
    subprocess.run(["g++", *flags, *objs, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, o], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr and r.stdout.startswith("replay OK"), r.stdout[-2000:] + r.stderr[-2000:]


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def test_python_surface():
    import inspect
    import litepi
    from litepi import _ffi, backend, e2e
    for s in ("lp_load_detector_onnx", "lp_load_detector_onnx_memory", "lp_detector_graph_describe"):
        assert s in _ffi.SYMBOLS
    assert issubclass(litepi.ONNXDetector, litepi.NCNNDetector) and "detect" in dir(litepi.ONNXDetector)
    assert list(inspect.signature(litepi.ONNXDetector.__init__).parameters)[1:3] == ["onnx_path", "input_size"]
    assert inspect.signature(backend.Engine.load_detector).parameters["bin_path"].default is None
    assert hasattr(backend.Engine, "load_detector_onnx")
    a = e2e.build_parser().parse_args(["--detector_onnx", "m.onnx"])
    assert a.detector_onnx == "m.onnx"

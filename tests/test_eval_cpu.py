"""Device-side evaluation, the parts that need no GPU: the matching rule of csrc/eval_match.h through lp_eval_match against
its NumPy restatement (tests/eval_ref.py), against the reference's recorded outputs and against the port where the port is
defined; the refactor of evaluate_predictions; configuration, records, symbols and option handling; the header under
sanitizers in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_SYMBOLS = ("lp_eval_default_config", "lp_eval_config_check", "lp_eval_create", "lp_eval_destroy", "lp_eval_reset", "lp_eval_device",
                "lp_eval", "lp_eval_drain", "lp_eval_match")


def _lib():
    from litepi import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.load_library()


# ---------------------------------------------------------------------------- today's evaluate_predictions, frozen
def _frozen_evaluate_predictions(all_preds, all_gts, num_classes, iou_thresholds=np.arange(0.5, 1.0, 0.05)):
    """evaluate_predictions as it stood before it was split into the matching and evaluate_from_rows"""
    from litepi.e2e import _ap101, _pairwise_iou
    nt = len(iou_thresholds)
    stats = []
    for preds, gts in zip(all_preds, all_gts):
        if len(preds) == 0:
            if len(gts) > 0:
                stats.append((np.zeros((0, nt), bool), np.array([]), np.array([]), np.array(gts)[:, 0]))
            continue
        pb = np.array([p["bbox"] for p in preds])
        pconf = np.array([p["conf"] for p in preds])
        pcls = np.array([p["cls_class"] for p in preds])
        correct = np.zeros((len(preds), nt), bool)
        if len(gts) > 0:
            g = np.array(gts)
            tcls, tb = g[:, 0], g[:, 1:]
            iou = _pairwise_iou(pb, tb)
            for j, thr in enumerate(iou_thresholds):
                pi, gi = np.where(iou >= thr)
                if not len(pi):
                    continue
                m = np.concatenate((np.stack((pi, gi), 1), iou[pi, gi][:, None]), 1)
                if len(pi) > 1:
                    m = m[m[:, 2].argsort()[::-1]]
                    m = m[np.unique(m[:, 0], return_index=True)[1]]
                    m = m[np.unique(m[:, 1], return_index=True)[1]]
                for p_i, g_i, _ in m:
                    if pcls[int(p_i)] == tcls[int(g_i)]:
                        correct[int(p_i), j] = True
        else:
            tcls = np.array([])
        stats.append((correct, pconf, pcls, tcls))
    zeros = lambda: np.zeros(num_classes)  # noqa: E731
    if not stats:
        return {"precision": zeros(), "recall": zeros(), "f1": zeros(), "tp": zeros(), "fp": zeros(), "fn": zeros(),
                "mAP50": 0.0, "mAP50_95": 0.0, "classes_present": np.zeros(num_classes, dtype=bool)}
    tp = np.concatenate([s[0] for s in stats], 0)
    conf = np.concatenate([s[1] for s in stats], 0)
    pcls = np.concatenate([s[2] for s in stats], 0)
    tcls = np.concatenate([s[3] for s in stats], 0)
    order = np.argsort(-conf)
    tp, pcls = tp[order], pcls[order]
    uniq, counts = np.unique(tcls, return_counts=True)
    n_gt_of = dict(zip(uniq, counts))
    ap50, ap5095, pbest, rbest, fbest = zeros(), zeros(), zeros(), zeros(), zeros()
    tpc_, fpc_, fnc_ = zeros(), zeros(), zeros()
    for c in range(num_classes):
        n_gt = n_gt_of.get(c, 0)
        sel = pcls == c
        n_p = sel.sum()
        if n_p == 0 and n_gt == 0:
            continue
        if n_p == 0 or n_gt == 0:
            fnc_[c] = n_gt
            continue
        tpc = tp[sel].cumsum(0)
        fpc = (1 - tp[sel]).cumsum(0)
        rec = tpc / (n_gt + 1e-16)
        prec = tpc / (tpc + fpc + 1e-16)
        aps = [_ap101(rec[:, j], prec[:, j]) for j in range(tp.shape[1])]
        ap50[c], ap5095[c] = aps[0], np.mean(aps)
        f1 = 2 * prec[:, 0] * rec[:, 0] / (prec[:, 0] + rec[:, 0] + 1e-16)
        b = int(np.argmax(f1))
        pbest[c], rbest[c], fbest[c] = prec[b, 0], rec[b, 0], f1[b]
        tpc_[c], fpc_[c] = tpc[b, 0], fpc[b, 0]
        fnc_[c] = n_gt - tpc_[c]
    present = uniq.astype(int)
    return {"precision": pbest, "recall": rbest, "f1": fbest, "tp": tpc_, "fp": fpc_, "fn": fnc_,
            "mAP50": float(np.mean(ap50[present])) if len(present) else 0.0,
            "mAP50_95": float(np.mean(ap5095[present])) if len(present) else 0.0,
            "ap50_per_class": ap50, "classes_present": np.isin(np.arange(num_classes), uniq)}


def _same_metrics(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


def _golden_cases(golden_dir):
    """the four cases of ref_evaluate.npz as ([per image DET_DTYPE], [per image gt tuples], num_classes, the recorded outputs)"""
    g = np.load(os.path.join(golden_dir, "ref_evaluate.npz"))
    for i in range(4):
        nimg, nclass = (int(v) for v in g[f"c{i}_nimg_nclass"])
        P, G = g[f"c{i}_preds"], g[f"c{i}_gts"]
        dets = [R.make_dets(P[P[:, 0] == b][:, 1:5], P[P[:, 0] == b][:, 5], P[P[:, 0] == b][:, 6].astype(int)) for b in range(nimg)]
        gts = [[tuple(int(v) for v in r[1:]) for r in G[G[:, 0] == b]] for b in range(nimg)]
        assert len(np.unique(P[:, 5].astype(np.float32))) == len(P), "the recorded confidences stay distinct as float32"
        yield i, dets, gts, nclass, {k[len(f"c{i}_"):]: g[k] for k in g.files if k.startswith(f"c{i}_")}


def _generator_sets():
    """seeded sets of frames: (name, [(dets, gts)], num_classes)"""
    rng = np.random.default_rng(20240611)
    sets = []
    for name, n, pmax, gmax, nc in (("small", 40, 40, 12, 5), ("dense", 12, 120, 30, 8), ("sparse", 40, 6, 3, 58)):
        frames = [R.scene(rng, int(rng.integers(0, pmax)), int(rng.integers(0, gmax)), nc) for _ in range(n)]
        sets.append((name, frames, nc))
    return sets


@pytest.fixture(scope="module")
def generator_sets():
    return _generator_sets()


# ---------------------------------------------------------------------------- the rule against the reference's recorded outputs
def test_rule_reproduces_the_references_recorded_outputs(golden_dir):
    from litepi import backend
    from litepi.e2e import metrics_from_rows
    _lib()
    for i, dets, gts, nclass, want in _golden_cases(golden_dir):
        assert sum(R.ties(d, g) for d, g in zip(dets, gts)) == 0, i
        rows = []
        for b, (d, g) in enumerate(zip(dets, gts)):
            m = backend.eval_match(d, g)
            r = np.zeros(len(d), dtype=backend._ffi.EVAL_ROW_DTYPE)
            r["conf"], r["cls"], r["correct"], r["frame"] = d["det_conf"], d["cls_class"], m["correct"], b
            rows.append(r)
        got = metrics_from_rows(np.concatenate(rows), R.gt_per_class(list(zip(dets, gts)), nclass), nclass, 10)
        for k in ("precision", "recall", "f1", "tp", "fp", "fn", "ap50_per_class"):
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-12), (i, k)
        assert np.allclose([got["mAP50"], got["mAP50_95"]], want["map"], atol=1e-12), i
        assert np.array_equal(got["classes_present"], want["present"]), i


# ---------------------------------------------------------------------------- lp_eval_match == eval_ref, bit for bit
UNSORTED16 = np.array([0.2 + 0.05 * ((j * 7) % 16) for j in range(16)])


@pytest.mark.parametrize("n_thr", [1, 10, 16])
def test_eval_match_equals_the_numpy_rule_bit_for_bit(n_thr):
    from litepi import backend
    _lib()
    thr = {1: np.array([0.5]), 10: R.THR10, 16: UNSORTED16}[n_thr]
    rng = np.random.default_rng(7 + n_thr)
    for P in (0, 1, 7, 64, 65, 300):
        for G in (0, 1, 4, 64, 256):
            dets, gts = R.scene(rng, P, G, 6, W=2048 if G < 64 else 700)   # a crowded frame: overlapping ground truth
            got, want = backend.eval_match(dets, gts, thr), R.match(dets, gts, thr)
            assert got.dtype.itemsize == 16 and got.tobytes() == want.tobytes(), (P, G, n_thr)


def test_eval_match_default_thresholds_are_numpys_arange():
    from litepi import backend, _ffi
    lib = _lib()
    c = _ffi.LpEvalConfig()
    lib.lp_eval_default_config(C.byref(c))
    assert c.n_thr == 10 and np.array(c.thr[:10]).tobytes() == np.arange(0.5, 1.0, 0.05).tobytes()
    assert (c.max_gt, c.max_rows) == (64, 1 << 20)
    d, g = R.scene(np.random.default_rng(3), 20, 5, 4)
    assert backend.eval_match(d, g).tobytes() == backend.eval_match(d, g, R.THR10).tobytes()


@pytest.mark.parametrize("name", sorted(R.hand_frames()))
def test_hand_built_frames(name):
    from litepi import backend
    _lib()
    dets, gts, thr, want = R.hand_frames()[name]
    got, ref = backend.eval_match(dets, gts, thr), R.match(dets, gts, thr)
    assert got.tobytes() == ref.tobytes()
    for p, (bits, gt) in want.items():
        assert (int(got["correct"][p]), int(got["gt"][p])) == (bits, gt), (name, p, bin(int(got["correct"][p])), int(got["gt"][p]))
    if name == "on_threshold":
        assert got["iou"][0] == 50 / (100 + 1e-7) < 0.5
    if name == "gt_tie_higher_g":
        assert R.ties(dets, gts, thr) == 1


# ---------------------------------------------------------------------------- equal to the port where the port is defined
def test_equal_to_the_port_on_tie_free_frames(generator_sets):
    from litepi import backend
    from litepi.e2e import evaluate_predictions, metrics_from_rows
    _lib()
    n_frames = n_free = 0
    for name, frames, nc in generator_sets:
        set_ties = 0
        rows = []
        for k, (dets, gts) in enumerate(frames):
            t = R.ties(dets, gts)
            n_frames, n_free, set_ties = n_frames + 1, n_free + (t == 0), set_ties + t
            m = backend.eval_match(dets, gts)
            if t == 0:
                assert np.array_equal(R.correct_matrix(m, 10), R.port_correct(dets, gts)), (name, k)
            r = np.zeros(len(dets), dtype=backend._ffi.EVAL_ROW_DTYPE)
            r["conf"], r["cls"], r["correct"], r["frame"] = dets["det_conf"], dets["cls_class"], m["correct"], k
            rows.append(r)
        assert set_ties == 0, f"the set {name} is compared as whole metrics: every frame must be tie-free"
        got = metrics_from_rows(np.concatenate(rows), R.gt_per_class(frames, nc), nc, 10)
        want = evaluate_predictions([R.result_dicts(d) for d, _ in frames], [g for _, g in frames], nc)
        _same_metrics(got, want)
    assert n_free >= 0.95 * n_frames


def test_metrics_from_rows_keeps_the_ports_order_among_equal_confidences():
    from litepi import backend
    from litepi.e2e import evaluate_predictions, metrics_from_rows
    _lib()
    rng = np.random.default_rng(11)
    frames = []
    for _ in range(10):
        dets, gts = R.scene(rng, 30, 6, 3)
        dets["det_conf"] = np.round(dets["det_conf"] * 4) / 4   # many equal confidences
        frames.append((dets, gts))
    assert sum(R.ties(d, g) for d, g in frames) == 0
    rows, _ = R.rows_of(frames)
    rows["correct"] = np.concatenate([backend.eval_match(d, g)["correct"] for d, g in frames])
    _same_metrics(metrics_from_rows(rows, R.gt_per_class(frames, 3), 3, 10),
                  evaluate_predictions([R.result_dicts(d) for d, _ in frames], [g for _, g in frames], 3))


# ---------------------------------------------------------------------------- the refactor
def test_evaluate_predictions_returns_what_it_returned(golden_dir, generator_sets):
    from litepi.e2e import evaluate_predictions
    cases = [([R.result_dicts(d) for d in dets], gts, nclass) for _, dets, gts, nclass, _ in _golden_cases(golden_dir)]
    cases += [([R.result_dicts(d) for d, _ in frames], [g for _, g in frames], nc) for _, frames, nc in generator_sets]
    cases += [([], [], 4), ([[], []], [[], []], 4), ([[]], [[(1, 0, 0, 5, 5)]], 4),
              ([R.result_dicts(R.make_dets([[0, 0, 5, 5]], [0.5], [1]))], [[]], 4),
              # what the old function did with a negative class (it indexed from the end) stays as it was
              ([R.result_dicts(R.make_dets([[0, 0, 5, 5], [9, 9, 20, 20]], [0.5, 0.4], [1, 3]))], [[(-1, 0, 0, 5, 5), (1, 0, 0, 5, 6), (3, 9, 9, 20, 21)]], 4)]
    for preds, gts, nc in cases:
        _same_metrics(evaluate_predictions(preds, gts, nc, 0.45), _frozen_evaluate_predictions(preds, gts, nc))


# ---------------------------------------------------------------------------- configuration, records, symbols, options
def test_eval_config_check_ranges():
    from litepi import backend, _ffi
    _lib()
    ok = backend.eval_config()
    assert backend.eval_config_check(ok) == 0
    assert backend.eval_config_check(None) == _ffi.LP_ERR_ARG
    for field, bad in (("max_gt", 0), ("max_gt", 257), ("max_rows", 0), ("n_thr", 0), ("n_thr", 17), ("reserved0", 1)):
        c = backend.eval_config()
        setattr(c, field, bad)
        assert backend.eval_config_check(c) == _ffi.LP_ERR_ARG, (field, bad)
    for field, good in (("max_gt", 1), ("max_gt", 256), ("max_rows", 1), ("n_thr", 1), ("n_thr", 16)):
        c = backend.eval_config()
        setattr(c, field, good)
        assert backend.eval_config_check(c) == 0, (field, good)
    c = backend.eval_config()
    c.thr[3] = float("nan")
    assert backend.eval_config_check(c) == _ffi.LP_ERR_ARG
    c = backend.eval_config(thr=[0.5, 0.75])
    c.thr[5] = float("nan")   # beyond n_thr: not looked at
    assert c.n_thr == 2 and backend.eval_config_check(c) == 0
    c = backend.eval_config()
    c.reserved[7] = 1
    assert backend.eval_config_check(c) == _ffi.LP_ERR_ARG
    with pytest.raises(TypeError):
        backend.eval_config(n_streams=1)
    with pytest.raises(ValueError):
        backend.eval_config(thr=[])


def test_eval_match_argument_errors():
    from litepi import _ffi
    lib = _lib()
    thr = (C.c_double * 1)(0.5)
    d, g, out = np.zeros(2, _ffi.DET_DTYPE), np.zeros(2, _ffi.GT_DTYPE), np.zeros(2, _ffi.MATCH_DTYPE)
    assert lib.lp_eval_match(d.ctypes.data, 2, g.ctypes.data, 2, thr, 1, out.ctypes.data) == 0
    assert lib.lp_eval_match(None, 0, None, 0, thr, 1, None) == 0
    for args in ((None, 2, g.ctypes.data, 2, thr, 1, out.ctypes.data), (d.ctypes.data, 2, None, 2, thr, 1, out.ctypes.data),
                 (d.ctypes.data, 2, g.ctypes.data, 2, thr, 1, None), (d.ctypes.data, -1, g.ctypes.data, 2, thr, 1, out.ctypes.data),
                 (d.ctypes.data, 2, g.ctypes.data, -1, thr, 1, out.ctypes.data), (d.ctypes.data, 2, g.ctypes.data, 2, thr, 0, out.ctypes.data),
                 (d.ctypes.data, 2, g.ctypes.data, 2, thr, 17, out.ctypes.data), (d.ctypes.data, 2, g.ctypes.data, 2, None, 1, out.ctypes.data)):
        assert lib.lp_eval_match(*args) == _ffi.LP_ERR_ARG


def test_record_layouts_and_symbols():
    from litepi import _ffi
    lib = _lib()
    assert C.sizeof(_ffi.LpMatch) == np.dtype(_ffi.MATCH_DTYPE).itemsize == 16
    assert C.sizeof(_ffi.LpEvalRow) == np.dtype(_ffi.EVAL_ROW_DTYPE).itemsize == 16
    assert C.sizeof(_ffi.LpGt) == np.dtype(_ffi.GT_DTYPE).itemsize == 32
    assert C.sizeof(_ffi.LpEvalConfig) == 16 + 16 * 8 + 32
    for struct, dtype in ((_ffi.LpMatch, _ffi.MATCH_DTYPE), (_ffi.LpEvalRow, _ffi.EVAL_ROW_DTYPE), (_ffi.LpGt, _ffi.GT_DTYPE)):
        dt = np.dtype(dtype)
        for name, *_ in struct._fields_:
            assert getattr(struct, name).offset == dt.fields[name][1], (struct.__name__, name)
    assert [getattr(_ffi.LpMatch, n).offset for n in ("correct", "gt", "iou")] == [0, 4, 8]
    assert [getattr(_ffi.LpEvalRow, n).offset for n in ("conf", "cls", "correct", "frame")] == [0, 4, 8, 12]
    assert [getattr(_ffi.LpGt, n).offset for n in ("cls", "x1", "y1", "x2", "y2", "reserved")] == [0, 4, 8, 12, 16, 20]
    assert _ffi.LpEvalConfig.thr.offset == 16 and _ffi.LpEvalConfig.reserved.offset == 144
    header = open(os.path.join(ROOT, "include", "litepi.h")).read()
    for s in EVAL_SYMBOLS:
        assert s in _ffi.SYMBOLS and hasattr(lib, s) and f"{s}(" in header
        assert getattr(lib, s).restype is (None if s == "lp_eval_default_config" else C.c_int)
    assert lib.lp_version() == _ffi.ABI_VERSION == 310


def test_pipeline_and_cli_options_without_a_device(tmp_path, monkeypatch):
    from litepi import backend, e2e
    _lib()
    with pytest.raises(ValueError, match="gts"):
        backend.check_eval_options(True, None)
    with pytest.raises(ValueError, match="evaluate"):
        backend.check_eval_options(False, [[]])
    with pytest.raises(ValueError, match="one list per image"):
        backend.check_eval_options(True, [[]], 2)
    backend.check_eval_options(True, [[], []], 2)
    backend.check_eval_options(False, None, 2)
    # run_batch applies the rule before it touches the engine
    pipe = object.__new__(backend.HybridPipeline)
    pipe.evaluate, pipe.track = False, False
    with pytest.raises(ValueError, match="evaluate"):
        pipe.run_batch([np.zeros((8, 8, 3), np.uint8)], gts=[[]])
    with pytest.raises(ValueError, match="evaluate"):
        pipe.run_batch([np.zeros((8, 8, 3), np.uint8)], evaluate=True, gts=[[]])
    pipe.evaluate = True
    with pytest.raises(ValueError, match="gts"):
        pipe.run_batch([np.zeros((8, 8, 3), np.uint8)])
    # the constructor refuses a bad configuration and the upload lanes before it creates an engine
    with pytest.raises(ValueError, match="max_gt"):
        backend.HybridPipeline("d.param", "d.bin", "c.pth", "shufflenetv2", evaluate=dict(max_gt=300))
    monkeypatch.setenv("LITEPI_DROPIN_LANES", "2")
    with pytest.raises(ValueError, match="upload lanes"):
        backend.HybridPipeline("d.param", "d.bin", "c.pth", "shufflenetv2", evaluate=True)
    monkeypatch.delenv("LITEPI_DROPIN_LANES")
    # the CLI
    args = e2e.build_parser().parse_args(["--device_eval", "--gpus", "2"])
    with pytest.raises(SystemExit, match="--device_eval and --gpus 2"):
        e2e.check_frame_args(args)
    with pytest.raises(SystemExit, match="device_eval_max_gt"):
        e2e.check_frame_args(e2e.build_parser().parse_args(["--device_eval", "--device_eval_max_gt", "0"]))
    e2e.check_frame_args(e2e.build_parser().parse_args(["--device_eval"]))
    assert e2e.build_parser().parse_args([]).device_eval is False and e2e.build_parser().parse_args([]).device_eval_max_gt == 64
    label = tmp_path / "frame_000001.txt"
    label.write_text("".join(f"{k % 3} 0.5 0.5 0.{k + 1:02d} 0.1\n" for k in range(5)))
    gts = e2e.parse_yolo_label(label, 640, 480)
    assert len(gts) == 5
    e2e.check_device_eval_labels(gts, 5, label)
    with pytest.raises(SystemExit, match="holds 5 boxes, more than --device_eval_max_gt 4"):
        e2e.check_device_eval_labels(gts, 4, label)
    assert "reads image files and gains no time" in " ".join(e2e.build_parser().format_help().split())


# ---------------------------------------------------------------------------- the shared header under sanitizers
def test_eval_match_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "eval_match_check")
    src = os.path.join(ROOT, "tests", "native", "eval_match_check.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK" and lines[-2] == "frames 10 hand-built, 90 swept"

"""CPU suite (-m "not gpu"), part 2: the boundary and the host logic.

* liblitepi_hip.so loads and exports every symbol include/litepi.h declares (no compute calls);
* without a GPU the product fails loudly (no CPU fallback);
* the multi-GPU path (shard + one gather of padded records) with world_size 2 over gloo;
* host-side helpers (synthetic classifier state, record layout, CLI surface).
"""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from litepi import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.load_library()


def test_library_exports_every_declared_symbol():
    from litepi import _ffi
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "litepi.h")).read()
    declared = sorted(set(re.findall(r"\b(lp_[a-z0-9_]+)\s*\(", header)))
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in litepi.h but not exported"
    assert sorted(_ffi.SYMBOLS) == declared
    assert lib.lp_version() == _ffi.ABI_VERSION


def test_struct_layouts_match_header():
    from litepi import _ffi
    assert ctypes.sizeof(_ffi.LpDet) == 32 and np.dtype(_ffi.DET_DTYPE).itemsize == 32
    assert ctypes.sizeof(_ffi.LpConfig) == 16 * 4
    assert ctypes.sizeof(_ffi.LpTiming) == 16
    assert ctypes.sizeof(_ffi.LpKernelTime) == 48 + 32 + 4 + 4 + 16  # name, layer, ms, pad, flops+bytes


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly_never_falls_back():
    from litepi import Engine, _ffi
    _lib()
    with pytest.raises(_ffi.LitepiError) as ei:
        Engine()
    assert ei.value.code == _ffi.LP_ERR_NODEVICE
    assert "no CPU path" in str(ei.value)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "yolo-litepi_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, re.M), f"{f} imports the oracle"


def test_shard_range_partitions_exactly():
    from litepi.distributed import shard_range
    for n in (0, 1, 7, 64, 512, 513):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, q):
    """One rank of the N>1 path on CPU (gloo): uneven image shards (shard_range), one fixed-capacity payload per rank,
    a Gatherer allocated once and used for several steps, max_det overflow (a shard whose images all saturate)."""
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "yolo-litepi_amd"))
    from litepi.distributed import COUNT_WORDS, Gatherer, alloc_result_buffers, records_to_numpy, shard_range
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    total_images, max_det = 4 * world + 3, 5           # not a multiple of world: shards differ by one image
    cap = -(-total_images // world)                    # every rank sends the same fixed-capacity message
    lo, hi = shard_range(total_images, rank, world)

    def fill(buf, step):
        rec = np.zeros((cap, max_det), dtype=records_to_numpy(buf.dets).dtype)
        buf.payload.zero_()
        for b in range(hi - lo):
            g = lo + b                                  # global image id
            n = max_det if g % 4 == 0 else (g + step) % (max_det + 1)   # every 4th image saturates max_det (overflow case)
            buf.counts[b] = n
            buf.counts[cap + b] = min(n + 1, max_det)
            buf.counts[2 * cap + b] = int(np.float32(0.5 + 0.01 * g).view(np.int32))
            for k in range(n):
                rec[b, k] = (g, step, k, 0.5, 0.9 - 0.1 * k, 0, g * 10 + k, 0.75)
        buf.dets.copy_(torch.from_numpy(rec.view(np.uint8).reshape(cap, max_det, 32)))

    buf = alloc_result_buffers(cap, max_det, "cpu")
    gat = Gatherer(buf, dst=0)
    ok = True
    recv_ptr = None
    for step in range(3):
        fill(buf, step)
        out = gat.gather(buf)
        if rank != 0:
            ok = ok and out is None
            continue
        all_dets, all_counts = out
        ok = ok and tuple(all_dets.shape) == (world, cap, max_det, 32) and tuple(all_counts.shape) == (world, COUNT_WORDS * cap)
        ok = ok and all_dets.data_ptr() == gat.recv.data_ptr()      # views of the receive buffer: nothing allocated per step
        recv_ptr = recv_ptr or gat.recv.data_ptr()
        ok = ok and recv_ptr == gat.recv.data_ptr()
        r = records_to_numpy(all_dets)
        seen = 0
        for src in range(world):
            slo, shi = shard_range(total_images, src, world)
            for b in range(shi - slo):
                g = slo + b
                n = max_det if g % 4 == 0 else (g + step) % (max_det + 1)
                ok = ok and int(all_counts[src, b]) == n and int(all_counts[src, cap + b]) == min(n + 1, max_det)
                ok = ok and np.int32(int(all_counts[src, 2 * cap + b])).view(np.float32) == np.float32(0.5 + 0.01 * g)
                for k in range(n):
                    e = r[src, b, k]
                    ok = ok and e["x1"] == g and e["y1"] == step and e["x2"] == k and e["cls_class"] == g * 10 + k
                seen += 1
            for b in range(shi - slo, cap):              # padding slots of a short shard stay empty
                ok = ok and int(all_counts[src, b]) == 0
        ok = ok and seen == total_images
    q.put(bool(ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_multi_rank_gather_of_detection_records_gloo(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(res)


def test_single_process_gather_is_identity():
    from litepi.distributed import alloc_result_buffers, gather_detections
    buf = alloc_result_buffers(2, 4, "cpu")
    d, c = gather_detections(buf)
    assert d.data_ptr() == buf.dets.data_ptr() and d.shape == (1, 2, 4, 32) and c.shape == (1, 6)
    dets, counts = buf
    d, c = gather_detections(dets, counts)
    assert d.data_ptr() == dets.data_ptr() and c.shape == (1, 6)


def test_random_shufflenet_state_matches_torchvision_layout():
    """The product's random-init classifier state has the key names/shapes of the oracle's
    torchvision-compatible module (so real shufflenetv2.pth files are interchangeable)."""
    from litepi.backend import random_shufflenet_state
    from oracle import shufflenet_ref as S
    sd = random_shufflenet_state(49, seed=3)
    ref = {k: v for k, v in S.ShuffleNetV2(49).state_dict().items() if not k.endswith("num_batches_tracked")}
    assert set(sd) == set(ref)
    for k in ref:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
    m = S.ShuffleNetV2(49)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)


def test_shift_cls_bias_touches_only_the_class_projections(tmp_path):
    from litepi import ncnn_export
    from oracle import ncnn_ref
    p, b = str(tmp_path / "m.param"), str(tmp_path / "m.bin")
    ncnn_export.export_detector(p, b, "v1", seed=5, cls_bias=-1.0)
    before = ncnn_ref.load_model(p, b)
    ncnn_export.shift_cls_bias(p, b, 0.75)
    after = ncnn_ref.load_model(p, b)
    changed = 0
    for l0, l1 in zip(ncnn_ref.conv_layers(before), ncnn_ref.conv_layers(after)):
        assert np.array_equal(l0.weight, l1.weight)
        if l0.bias is None:
            continue
        if not np.array_equal(l0.bias, l1.bias):
            changed += 1
            assert l0.weight.shape[0] == 1 and np.allclose(l1.bias - l0.bias, 0.75)
    assert changed == 3


def test_cli_surface_matches_reference_flags():
    """litepi.e2e keeps the reference's argument surface (e2e.py:1017-1048)."""
    from litepi import e2e
    ap = e2e.build_parser()
    flags = {a.option_strings[0] for a in ap._actions if a.option_strings}
    for f in ("--detector_param", "--detector_bin", "--classifier", "--clf_arch", "--input", "--labels", "--classes",
              "--num_samples", "--seed", "--yolo_conf", "--benchmark_conf", "--min_area", "--iou_threshold",
              "--det_input_size", "--cls_input_size", "--detector_threads", "--batch_size", "--device", "--output",
              "--save_viz"):
        assert f in flags, f
    d = ap.parse_args(["--detector_param", "a", "--detector_bin", "b", "--input", "i", "--labels", "l", "--classes", "c"])
    assert (d.seed, d.yolo_conf, d.benchmark_conf, d.min_area, d.iou_threshold) == (42, 0.001, 0.25, 50, 0.45)
    assert (d.det_input_size, d.cls_input_size, d.detector_threads, d.batch_size) == (640, 64, 4, 8)


def test_evaluate_predictions_matches_reference_goldens(golden_dir):
    """litepi.e2e.evaluate_predictions vs outputs of the REFERENCE's evaluate_predictions
    (tools/make_goldens.py ran it on these toy sets in the build container)."""
    from litepi.e2e import evaluate_predictions
    g = np.load(os.path.join(golden_dir, "ref_evaluate.npz"))
    for i in range(4):
        nimg, nclass = g[f"c{i}_nimg_nclass"]
        preds = [[] for _ in range(nimg)]
        gts = [[] for _ in range(nimg)]
        for row in g[f"c{i}_preds"]:
            preds[int(row[0])].append({"bbox": tuple(int(v) for v in row[1:5]), "conf": float(row[5]), "cls_class": int(row[6])})
        for row in g[f"c{i}_gts"]:
            gts[int(row[0])].append(tuple(int(v) for v in row[1:]))
        m = evaluate_predictions(preds, gts, int(nclass), 0.45)
        for k in ("precision", "recall", "f1", "tp", "fp", "fn", "ap50_per_class"):
            assert np.allclose(m[k], g[f"c{i}_{k}"], rtol=0, atol=1e-12), (i, k)
        assert np.allclose([m["mAP50"], m["mAP50_95"]], g[f"c{i}_map"], atol=1e-12)
        assert np.array_equal(m["classes_present"], g[f"c{i}_present"])


# ---- litepi/e2e.py --gpus N: shard + merge under gloo (world 2, CPU, fake engine) --------------------------------------
class _FakeMetrics:
    def __init__(self, t):
        self.t_total = t


class _FakePipeline:
    """Stands in for litepi.backend.HybridPipeline in the CPU tests of the harness: deterministic detections computed from
    the image bytes (so every rank and the single-process run agree on what an image yields), more of them at a lower conf."""

    def __init__(self, *a, **k):
        self.engine = self

    def close(self):
        pass

    def run_batch(self, imgs, conf, iou, min_area):
        out = []
        for im in imgs:
            seed = int(im[:4, :4].astype(np.int64).sum())
            rng = np.random.default_rng(seed)
            n = int(rng.integers(0, 4)) + (3 if conf < 0.01 else 0)
            res = []
            for _ in range(n):
                x1, y1 = int(rng.integers(0, 40)), int(rng.integers(0, 40))
                res.append({"bbox": (x1, y1, x1 + int(rng.integers(8, 20)), y1 + int(rng.integers(8, 20))),
                            "det_conf": float(np.float32(rng.uniform(max(conf, 0.01), 1.0))), "cls_class": int(rng.integers(0, 3)),
                            "det_class": 0, "cls_conf": 0.9})
            out.append((res, _FakeMetrics(1.0 + 0.01 * (seed % 7))))
        return out


def _make_eval_set(root, n):
    from PIL import Image
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels"), exist_ok=True)
    rng = np.random.default_rng(5)
    for i in range(n):
        im = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
        Image.fromarray(im).save(os.path.join(root, "images", f"img_{i:03d}.png"))
        with open(os.path.join(root, "labels", f"img_{i:03d}.txt"), "w") as f:
            for _ in range(int(rng.integers(0, 3))):
                f.write(f"{int(rng.integers(0, 3))} {rng.uniform(0.3, 0.7):.4f} {rng.uniform(0.3, 0.7):.4f} 0.2 0.25\n")
    with open(os.path.join(root, "classes.json"), "w") as f:
        f.write('{"0": "a", "1": "b", "2": "c"}')


def _eval_args(root, out, gpus):
    sys.path.insert(0, os.path.join(ROOT, "yolo-litepi_amd"))
    from litepi import e2e
    return e2e.build_parser().parse_args(["--input", os.path.join(root, "images"), "--labels", os.path.join(root, "labels"),
                                          "--classes", os.path.join(root, "classes.json"), "--output", out, "--batch_images", "3",
                                          "--gpus", str(gpus), "--detector_param", "fake.param"])


def _eval_worker(rank, world, port, root, q):
    sys.path.insert(0, os.path.join(ROOT, "yolo-litepi_amd"))
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "LOCAL_RANK": str(rank),
                       "WORLD_SIZE": str(world), "LITEPI_DIST_BACKEND": "gloo"})
    import litepi.backend as backend
    from litepi import e2e
    backend.HybridPipeline = _FakePipeline
    r = e2e.run_evaluation(_eval_args(root, os.path.join(root, f"out_w{world}"), world))
    if rank == 0:
        q.put({"preds": r["all_preds"], "gts": r["all_gts"], "mAP50": r["metrics"]["mAP50"], "mAP50_95": r["metrics"]["mAP50_95"],
               "times": r["rank_bench_times"], "fps": r["fps"]})
    else:
        q.put({"rank": r["rank"], "n_files": len(r["files"])})
    import torch.distributed as dist
    dist.destroy_process_group()


def test_e2e_harness_shards_and_merges_under_gloo(tmp_path, monkeypatch):
    """`litepi.e2e --gpus 2` on CPU: 11 images (uneven shards of 6 + 5, chunks of 3), a fake engine, backend gloo.  Rank 0's
    merged predictions, ground truths and metric equal the single-process run's exactly; the other rank returns early."""
    import torch.multiprocessing as mp
    root = str(tmp_path)
    _make_eval_set(root, 11)
    # single process
    import litepi.backend as backend
    from litepi import e2e
    monkeypatch.setattr(backend, "HybridPipeline", _FakePipeline)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    one = e2e.run_evaluation(_eval_args(root, os.path.join(root, "out_w1"), 1))
    assert len(one["all_preds"]) == 11 and sum(len(p) for p in one["all_preds"]) > 20
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eval_worker, args=(r, 2, port, root, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    r0 = next(r for r in res if "preds" in r)
    r1 = next(r for r in res if "rank" in r)
    assert r1 == {"rank": 1, "n_files": 5}
    assert r0["preds"] == one["all_preds"] and r0["gts"] == one["all_gts"]
    assert r0["mAP50"] == one["metrics"]["mAP50"] and r0["mAP50_95"] == one["metrics"]["mAP50_95"]
    # the sharded job's FPS: images / the slowest rank's summed benchmark time
    assert len(r0["times"]) == 2 and abs(sum(r0["times"]) - one["rank_bench_times"][0]) < 1e-9
    assert abs(r0["fps"] - 11 / max(r0["times"])) < 1e-9


def test_eval_row_packing_round_trips():
    from litepi.distributed import pack_eval_rows, unpack_eval_rows
    preds = [[{"bbox": (1, 2, 30, 40), "conf": float(np.float32(0.123456789)), "cls_class": 7}], [],
             [{"bbox": (0, 0, 2048, 2047), "conf": float(np.float32(0.001)), "cls_class": -1}] * 2]
    gts = [[(3, 1, 1, 9, 9)], [(0, 5, 6, 7, 8), (1, 0, 0, 1, 1)], []]
    p2, g2 = unpack_eval_rows(pack_eval_rows(preds, gts), 3)
    assert p2 == preds and g2 == gts
    p3, g3 = unpack_eval_rows(pack_eval_rows([[]], [[]]), 1)
    assert p3 == [[]] and g3 == [[]]


def test_copy_pool_stress_native(tmp_path):
    """The copy workers behind the host entry points (csrc/copy_pool.h: pinned-staging uploads of lp_run_batch / lp_detect) on the
    CPU: tests/native/copy_pool_stress.cpp pushes 1500 batches of 1..97 jobs through an 8-thread pool and verifies every byte.
    (A first version kept the batch state in pool members and could double-count a job across two batches -- run() then waited
    forever; the batch now lives on run()'s stack under a serial number, and the harness is clean under -fsanitize=thread.)"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "copy_pool_stress")
    src = os.path.join(ROOT, "tests", "native", "copy_pool_stress.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", inc, src, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_pmc_tool_maps_rocprof_kernel_names_to_the_library_profile_names():
    """bench.py looks its dominant kernel up in profiles/rNN_pmc_traffic*.json by the library's profile name; tools/pmc_traffic.py
    derives the same names from rocprofv3's (demangled or mangled) kernel names.  A mapping that drifts leaves roofline.traffic
    null, so the names of every round-4 kernel are pinned here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmc_traffic", os.path.join(ROOT, "tools", "pmc_traffic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ns, cp = "lp::(anonymous namespace)::", "lp::c2fplan::"   # the kernels of c2f_kernels.hip, the configuration types of c2f_plan.h
    cases = {
        f"void {ns}c2f_kernel<{cp}C2fCfg<24, 2, 0, 48, false, 48, -1, 0, 20, true, 8> >(lp::C2fArgs)": "c2f<24,2,y0y1>_f16",
        f"void {ns}c2f_kernel<{cp}C2fCfg<48, 1, 192, 96, true, 96, 0, 0, 20, false, 0> >(lp::C2fArgs)": "c2f<48,1,up192+96>_f16",
        f"void {ns}c2f_kernel<{cp}C2fCfg<64, 1, 0, 128, false, 128, 2, 64, 20, true, 0> >(lp::C2fArgs)": "c2f<64,1,s2+128,sppf>_f16",
        f"void {ns}s2lds_kernel<{cp}S2LCfg<16, 32, 10, 1, 1, true> >(lp::C2fArgs)": "s2conv+1x1<16,32>_f16",
        f"void {ns}s2lds_kernel<{cp}S2LCfg<96, 192, 10, 4, 2, false> >(lp::C2fArgs)": "s2conv<96,192>_f16",
        f"void {ns}s2conv_kernel<{cp}S2Cfg<32, 64, 20> >(lp::C2fArgs)": "s2conv<32,64>_f16",
        f"void {ns}sppf_kernel<{cp}SpCfg<96, 192, 192, 2> >(lp::C2fArgs)": "sppf<192,96,192>_f16",
        "void lp::stem_block16_kernel<8>(lp::StemBlockArgs)": "stem_block16_f16",
        "lp::stem_block_kernel(lp::StemBlockArgs)": "stem_block_f16",
        "void lp::head_fused_kernel<2, 3, 1, 3, 2, 12, 3, true, true, 18>(lp::HeadArgs)": "head_fused<2,3,1,3,2,12>a16k3_f16",
        "void lp::head_fused_kernel<2, 3, 1, 3, 2, 12, 4, true, true, 27>(lp::HeadArgs)": "head_fused<2,3,1,3,2,12>a16k6_f16",
        "void lp::head_fused_kernel<1, 3, 1, 2, 2, 8, 3, true, true, 9>(lp::HeadArgs)": "head_fused<1,3,1,2,2,8>a16_f16",
    }
    for name, want in cases.items():
        assert mod.family(name) == want, (name, mod.family(name), want)

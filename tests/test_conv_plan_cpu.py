"""The conv kernels' tile and split planner (csrc/conv_plan.h) without a device.

tests/native/conv_plan_replay.cpp includes the header alone, built with a plain g++ under -fsanitize=address,undefined.  It
plans every shape of tests/golden/conv_plans.json -- what ConvLayer::build and BottleneckPair::build computed BEFORE the
arithmetic moved into the header (commit e0a3b0a, recorded on the device: see the file's "about") -- and the planned fields
must be the recorded ones.  From the header alone, every planned (family, NT, tile, tail) must also be an entry of the family's
table of instantiated kernels, and the DISPATCH_CASES of test_gpu_parity.py must plan NT = 2, 3, 4 with at least 160 workgroups."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, FP16 = 0, 1


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("conv_plan") / "conv_plan_replay")
    src = os.path.join(ROOT, "tests", "native", "conv_plan_replay.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", inc, src,
                    "-o", exe], check=True, timeout=300)

    def run(requests):
        r = subprocess.run([exe], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tables(replay):
    t = {"bneck_tile": []}
    for ln in replay(["tables"]):
        name, *vals = ln.split()
        if name == "bneck_tile":
            t[name].append(tuple(int(v) for v in vals))   # th, tw, p1, p2, max_nt, tail, cl
        elif name != "end":
            t[name] = [tuple(int(x) for x in v.split(",")) if "," in v else int(v) for v in vals]
    return t


def _split(fields):
    i = fields.index("|")
    return i, len(fields) - 1 - i


def test_conv_plans_match_the_recording(replay, golden, tables):
    nin, nout = _split(golden["conv_fields"])
    rows = golden["conv"]
    assert nin == 10 and nout == 15 and len(rows) > 600
    got = replay(["conv " + " ".join(str(v) for v in r[:nin]) for r in rows])
    assert len(got) == len(rows)
    seen = set()
    for r, g in zip(rows, got):
        assert g.split() == [str(v) for v in r[nin:]], f"conv {r[:nin]}: planned {g}, recorded {r[nin:]}"
        prec, k, stride, cin, cout, hout, wout, batch, full_n, single = r[:nin]
        direct, nt = r[nin], r[nin + 1]
        if single:
            continue   # weights of a BottleneckPair: launched by the bottleneck kernel (checked below)
        family = "convs2" if direct else "conv3x3" if k == 3 else "conv1x1"
        seen.add((family, nt))
        if family == "conv1x1":
            assert nt in tables[family], r
        elif full_n:   # built for a fused tail: some tail entry, or the plain one, has this NT
            assert any(v[0] == nt for v in tables[family]), r
        else:
            assert (nt, 0) in tables[family], r
    # the recording reaches every NT of every family
    assert {(f, n) for f in ("conv3x3", "convs2", "conv1x1") for n in (1, 2, 3, 4)} <= seen


def test_bottleneck_plans_match_the_recording(replay, golden, tables):
    nin, nout = _split(golden["bneck_fields"])
    rows = golden["bneck"]
    assert nin == 10 and nout == 9 and len(rows) > 100
    got = replay(["bneck " + " ".join(str(v) for v in r[:nin]) for r in rows])
    tiles = {(t[0], t[1]): t for t in tables["bneck_tile"]}
    sg16, sg32 = tables["bneck_max_sg"]
    n_cl = 0
    for r, g in zip(rows, got):
        assert g.split() == ["1"] + [str(v) for v in r[nin:]], f"bneck {r[:nin]}: planned {g}, recorded {r[nin:]}"
        prec, c, has_cv2 = r[0], r[1], r[5]
        th, tw, _, _, cl, _, t2, _, sg = r[nin:]
        nt = (c + 15) // 16
        _, _, p1, p2, max_nt, tail, has_cl = tiles[(th, tw)]
        assert (th + 2) * (tw + 2) <= p1 * 64 and th * tw <= p2 * 64 and nt <= max_nt and nt in tables["bneck_nt"], r
        if has_cv2:
            assert tail and (nt, t2) in tables["bneck_tails"] and 1 <= sg <= (sg16 if prec == FP16 else sg32), r
        if cl:
            n_cl += 1
            assert has_cl and has_cv2 and prec == FP16 and nt == 1 and sg == 1, r
    assert n_cl >= 2   # LITEPI_BNECK_CL=1 loads are part of the recording


def test_plans_without_an_instantiation_are_refused(replay):
    """shapes the parent refused in cv2_shape / plan(): no tail kernel for (NT, T2), too many gathered K steps, more than 64
    channels; and a 3x3 conv with a fused tail that the tables do not hold"""
    ok = lambda ln: ln.split()[0] == "1"
    got = replay(["bneck 1 16 80 80 4 1 32 48 1 0",     # NT 1, T2 3
                  "bneck 1 16 80 80 4 1 104 32 1 0",    # fp16, 13 K groups = 4 gathered steps
                  "bneck 0 16 80 80 4 1 104 32 1 0",    # fp32, 26 K groups = 7 gathered steps
                  "bneck 1 72 40 40 4 0 0 0 0 0",
                  "bneck 1 16 80 80 4 1 32 32 1 0"])
    assert [ok(g) for g in got] == [False, False, False, False, True]


def test_dispatch_cases_plan_every_channel_tile_count(replay, golden):
    """test_gpu_parity.DISPATCH_CASES: N = 8, 80x80 output, Cin 16, Cout 32 / 48 / 64 plan NT = 2 / 3 / 4 in each family, on at
    least 160 workgroups -- so the GPU cases launch the NT 2, 3, 4 entries of the tables and cannot drift onto NT 1"""
    nin, _ = _split(golden["conv_fields"])
    recorded = {tuple(r[:nin]): r[nin:] for r in golden["conv"]}
    for prec in (FP32, FP16):
        for k, stride in ((1, 1), (3, 1), (3, 2)):
            for cout, want_nt in ((32, 2), (48, 3), (64, 4)):
                req = (prec, k, stride, 16, cout, 80, 80, 8, 0, 0)
                assert req in recorded, req
                direct, nt, nsplits, _, _, _, _, _, _, bwh, bww = (int(v) for v in replay(["conv " + " ".join(map(str, req))])[0].split()[:11])
                assert nt == want_nt and direct == (1 if stride == 2 else 0), (req, nt)
                if k == 3 and stride == 1:
                    wgs = 8 * -(-80 // (4 * bwh)) * -(-80 // (20 * bww)) * nsplits
                else:
                    wgs = min(-(-8 * 80 * 80 // 256), 4096) * nsplits
                assert wgs >= 160, (req, wgs)

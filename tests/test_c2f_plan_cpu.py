"""The configurations, predicates and weight packers of c2f_kernels.hip (csrc/c2f_plan.h) without a device.

tests/native/c2f_plan_replay.cpp includes the header alone, built with a plain g++ under -fsanitize=address,undefined, as a stand-alone
program.  It answers every case of tests/golden/c2f_plans.json -- what supported() / tail_supported() / lds_staged() / kernel_name() /
cv2_from_lds() and build() of C2fLayer, S2ConvLayer and SppfLayer computed BEFORE the configuration types, their tables, the K orders
and the fragment packer moved out of c2f_kernels.hip into the header (see the file's "about") -- and every flag, row field, size and
hash must be the recorded one.  From the header alone: every supported case maps to exactly one row, every row is reached by a
recorded case, the rows are the 28 kernel instantiations of that commit's code object, and their profile names are the launches
tests/test_gpu_c2f_float64.py pins on the device."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "c2f_plans.json")

MAPS = ((160, 160), (80, 80), (40, 40), (20, 20), (10, 10), (48, 80), (24, 40), (12, 20), (50, 50))
# the 18 C2f shapes (C, NB, KA, KB, UP, COUT, MODE, KS2) and each shape's own map
SHAPES = (
    (32, 1, 128, 64, 1, 64, 0, 0, 40, 40), (16, 1, 64, 32, 1, 32, 0, 0, 80, 80), (32, 1, 0, 128, 0, 64, 0, 0, 40, 40),
    (64, 1, 0, 256, 0, 128, 1, 64, 20, 20), (64, 1, 0, 128, 0, 128, 2, 64, 20, 20), (16, 2, 0, 32, 0, 32, 0, 0, 80, 80),
    (32, 2, 0, 64, 0, 64, 0, 0, 40, 40), (48, 1, 192, 96, 1, 96, 0, 0, 40, 40), (48, 1, 0, 144, 0, 96, 0, 0, 40, 40),
    (24, 1, 96, 48, 1, 48, 0, 0, 80, 80), (96, 1, 0, 192, 0, 192, 0, 0, 20, 20), (96, 1, 0, 288, 0, 192, 0, 0, 20, 20),
    (24, 2, 0, 48, 0, 48, 0, 0, 80, 80), (48, 2, 0, 96, 0, 96, 0, 0, 40, 40), (64, 1, 0, 256, 0, 128, 0, 0, 20, 20),
    (64, 1, 0, 128, 0, 128, 0, 0, 20, 20), (16, 2, 0, 32, 0, 32, -1, 0, 80, 80), (24, 2, 0, 48, 0, 48, -1, 0, 80, 80),
)
S2_CINS, S2_COUTS = (16, 24, 32, 48, 64, 96), (32, 48, 64, 96, 128, 192)
S2_MAPS = ((80, 80), (40, 40), (20, 20), (10, 10), (24, 40), (50, 60))
SPPF_CASES = ((192, 96, 192, 20, 20), (128, 64, 128, 20, 20), (192, 96, 192, 40, 40), (192, 96, 192, 12, 20))


def perturbed(s):
    """a shape with one key field perturbed: C+8, NB+1, KA+32, UP flipped, COUT+16, MODE replaced by each other value, KS2+32"""
    out = []
    for i, d in ((0, 8), (1, 1), (2, 32), (5, 16), (7, 32)):
        out.append(s[:i] + (s[i] + d,) + s[i + 1:])
    out.append(s[:4] + (1 - s[4],) + s[5:])
    out += [s[:6] + (m,) + s[7:] for m in (-1, 0, 1, 2) if m != s[6]]
    return out


def c2f_req(verb, key, hw):
    return verb + " " + " ".join(str(v) for v in tuple(key) + tuple(hw))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("c2f_plan") / "c2f_plan_replay")
    src = os.path.join(ROOT, "tests", "native", "c2f_plan_replay.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", inc, src,
                    "-o", exe], check=True, timeout=300)

    def run(requests):
        r = subprocess.run([exe], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(requests) or requests in (["rows"], ["table"])
        return out
    return run


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rows(replay):
    """the three tables of the header: [(family, profile name, key, fields)]"""
    out = replay(["rows"])
    assert out[-1] == "end"
    nkey = {"c2f": 8, "s2": 3, "sppf": 3}
    return [(f[0], f[1], tuple(int(v) for v in f[2:2 + nkey[f[0]]]), f[2 + nkey[f[0]]:]) for f in (ln.split() for ln in out[:-1])]


def test_cases_are_the_issue_s_list(golden):
    assert [tuple(m) for m in golden["maps"]] == list(MAPS) and [tuple(s) for s in golden["c2f_shapes"]] == list(SHAPES)
    assert len(SHAPES) == 18 and len(set(SHAPES)) == 18 and len(golden["c2f_flags"]) == 18 and len(golden["c2f_packs"]) == 18
    assert [tuple(p[:10]) for p in golden["c2f_perturbed"]] == [p for s in SHAPES for p in perturbed(s)]
    assert len(golden["c2f_perturbed"]) == 18 * 9
    assert (tuple(golden["s2_cins"]), tuple(golden["s2_couts"]), [tuple(m) for m in golden["s2_maps"]]) == (S2_CINS, S2_COUTS, list(S2_MAPS))
    assert set(golden["s2_flags"]) == {f"{ci},{co},{t}" for ci in S2_CINS for co in S2_COUTS for t in (0, 1)}
    assert len(golden["s2_packs"]) == 9 and set(golden["s2_packs"]) <= set(golden["s2_flags"])
    assert [tuple(c[:5]) for c in golden["sppf"]] == list(SPPF_CASES)
    assert [c[5] != "0" for c in golden["sppf"]] == [True, False, False, False]
    assert "commit" in golden["about"] and os.path.getsize(GOLDEN) < 64 * 1024


def test_c2f_flags_rows_and_packs_match_the_recording(golden, replay):
    got = replay([c2f_req("c2f", s[:8], m) for s in SHAPES for m in MAPS])
    for i, s in enumerate(SHAPES):
        digits, tail = golden["c2f_flags"][i]
        for j, m in enumerate(MAPS):
            assert got[i * len(MAPS) + j] == f"{digits[j]} {tail}", f"{s[:8]} @{m}: {got[i * len(MAPS) + j]}, recorded {digits[j]} {tail}"
        assert digits[MAPS.index(s[8:])] == "1", f"{s}: the parent supported every shape on its own map"
    got = replay([c2f_req("c2fpack", s[:8], s[8:]) for s in SHAPES])
    for s, g, want in zip(SHAPES, got, golden["c2f_packs"]):
        assert want.startswith("1 c2f ") and g == want, f"{s}:\n got      {g}\n recorded {want}"
    got = replay([c2f_req("c2f", p[:8], p[8:10]) for p in golden["c2f_perturbed"]])
    for p, g in zip(golden["c2f_perturbed"], got):
        assert g == p[10], f"perturbed {p[:10]}: {g}, recorded {p[10]}"


def test_stride2_and_sppf_match_the_recording(golden, replay):
    keys = [(ci, co, t) for ci in S2_CINS for co in S2_COUTS for t in (0, 1)]
    got = replay([f"s2 {ci} {co} {co} {t} {m[0]} {m[1]}" for ci, co, t in keys for m in S2_MAPS])
    for i, (ci, co, t) in enumerate(keys):
        digits, staged = golden["s2_flags"][f"{ci},{co},{t}"]
        for j, m in enumerate(S2_MAPS):
            assert got[i * len(S2_MAPS) + j] == f"{digits[j]} {staged}", f"s2 {ci} -> {co} tail {t} @{m}: {got[i * len(S2_MAPS) + j]}"
    got = replay([f"s2pack {ci} {co} {t} 80 80" for ci, co, t in keys])
    for (ci, co, t), g in zip(keys, got):
        assert g == golden["s2_packs"].get(f"{ci},{co},{t}", "0"), f"s2pack {ci} -> {co} tail {t}: {g}"
    other = golden["s2_tail_other_cout2"]
    assert len(other) == 36 and all(o[2] != o[1] for o in other)
    got = replay([f"s2 {o[0]} {o[1]} {o[2]} 1 {o[3]} {o[4]}" for o in other])
    assert got == [o[5] for o in other] and all(g.startswith("0 ") for g in got)
    got = replay(["sppf %d %d %d %d %d" % tuple(c[:5]) for c in golden["sppf"]])
    assert got == [c[5] for c in golden["sppf"]]


def test_every_case_maps_to_one_row_and_every_row_is_reached(golden, rows):
    reached = set()

    def one_row(fam, key):
        hit = [i for i, r in enumerate(rows) if r[0] == fam and r[2] == tuple(key)]
        assert len(hit) == 1, f"{fam} {key}: rows {hit}"
        reached.add(hit[0])
        return rows[hit[0]]

    for s, (digits, tail), pack in zip(SHAPES, golden["c2f_flags"], golden["c2f_packs"]):
        if "1" in digits:
            r = one_row("c2f", s[:8])
            assert r[1] == tail.split()[0] and pack.split(" | ")[0].split()[1:] == ["c2f", r[1]] + [str(v) for v in r[2]] + r[3]
    for p in golden["c2f_perturbed"]:
        if p[10][0] == "1":
            one_row("c2f", p[:8])
    for k, (digits, _) in golden["s2_flags"].items():
        if "1" in digits:
            r = one_row("s2", [int(v) for v in k.split(",")])
            assert golden["s2_packs"][k].split(" | ")[0].split()[1:] == ["s2", r[1]] + [str(v) for v in r[2]] + r[3]
    for c in golden["sppf"]:
        if c[5] != "0":
            one_row("sppf", c[:3])
    assert reached == set(range(len(rows))), f"rows no recorded case reaches: {sorted(set(range(len(rows))) - reached)}"


def test_the_rows_are_the_parents_instantiations(golden, replay, rows):
    """the kernel symbols of the recorded commit's code object: 28, each a type of the lists, each type one of them, one row per type"""
    table = replay(["table"])
    assert table[-1] == "end"
    want = golden["instantiations"]
    assert len(want) == 28 and len(set(want)) == 28
    assert sorted(table[:-1]) == sorted(want)
    assert len(rows) == 28 and [t.split()[1] for t in table[:-1]] == [r[1] for r in rows]


def test_profile_names_are_the_launches_pinned_on_the_device(rows):
    import test_gpu_c2f_float64 as G
    pinned = {n for _, _, launches in list(G.CASES.values()) + [G.CHILD_CASE] for n in launches} | {"s2conv<64,128>"}
    assert {r[1] for r in rows} == pinned

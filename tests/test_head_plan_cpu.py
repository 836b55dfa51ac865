"""The fused Detect head's planner, table of variants and weight-stream packer (csrc/head_plan.h) without a device.

tests/native/head_plan_replay.cpp includes the header alone, built with a plain g++ under -fsanitize=address,undefined.  It plans
and packs every case of tests/golden/head_plans.json -- what HeadLayer::supported and HeadLayer::build computed BEFORE the shapes,
their checks and the packer moved into the header (commit a4a2321: see the file's "about") -- and the plan fields, the chunk tables,
the profile name and the hashes of the packed stream and of the three bias vectors must be the recorded ones; what that commit's
supported() refused must be refused.  From the header alone, every planned case maps to exactly one row of the table, every row
is reached by a recorded case, and the rows are the 20 instantiations of head_fused_kernel in that commit's code object."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("head_plan") / "head_plan_replay")
    src = os.path.join(ROOT, "tests", "native", "head_plan_replay.cpp")
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
    with open(os.path.join(ROOT, "tests", "golden", "head_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed(replay, golden):
    """every case of the recording, planned and packed once: [(case, reply split at '|')]"""
    nin = golden["case_fields"].index("|")
    assert nin == 6
    got = replay(["head " + " ".join(str(v) for v in c[:nin]) for c in golden["cases"]])
    assert len(got) == len(golden["cases"])
    return [(c, [part.split() for part in g.split("|")]) for c, g in zip(golden["cases"], got)]


@pytest.fixture(scope="module")
def table(replay):
    rows = [ln.split() for ln in replay(["table"])]
    assert rows[-1] == ["end"]
    return [(r[0], tuple(int(v) for v in r[1:])) for r in rows[:-1]]   # (profile name, the 14 template arguments)


def test_cases_are_the_issue_s_list(golden):
    nin = golden["case_fields"].index("|")
    ok = {tuple(c[:nin]) for c in golden["cases"] if c[nin + 1]}
    pairs = [(c3, cin) for c3 in (8, 32) for cin in (32, 64, 128)] + [(c3, cin) for c3 in (40, 48, 64) for cin in (48, 96, 192)]
    masks = [0, 1, 2, 4, 8, 3, 12]   # {}, MERGED_A, A32, 2WG, 1WG, A32 + MERGED_A, 1WG + 2WG
    assert golden["switch_bits"] == ["LITEPI_HEAD_MERGED_A", "LITEPI_HEAD_A32", "LITEPI_HEAD_2WG", "LITEPI_HEAD_1WG"]
    assert ok == {(cin, 64, c3, nc, 16, m) for c3, cin in pairs for nc in (1, 3, 32) for m in masks}
    refused = {tuple(c[:nin - 1]) for c in golden["cases"] if not c[nin + 1]}
    assert refused == {(48, 64, 32, 1, 16), (64, 64, 48, 1, 16), (16, 64, 32, 1, 16), (40, 64, 32, 1, 16), (32, 64, 4, 1, 16), (32, 64, 36, 1, 16),
                       (48, 64, 72, 1, 16), (32, 64, 32, 0, 16), (32, 64, 32, 33, 16), (32, 64, 32, 1, 8), (32, 32, 32, 1, 16)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "head_plans.json")) < 40000


def test_plans_and_streams_match_the_recording(golden, replayed):
    nin = golden["case_fields"].index("|")
    assert golden["plan_fields"][0] == "name" and len(golden["plan_fields"]) == 19
    n_ok = 0
    for case, parts in replayed:
        supported = case[nin + 1]
        assert int(parts[0][0]) == supported, f"{case[:nin]}: plan_head ok = {parts[0]}, the parent's supported() = {supported}"
        if not supported:
            continue
        n_ok += 1
        plan, nbytes, h_stream = golden["plans"][case[nin + 2]], case[nin + 3], case[nin + 4]
        assert parts[0][2:] == [str(v) for v in plan["fields"]], f"{case[:nin]}: planned {parts[0][2:]}, recorded {plan['fields']}"
        for key, got in zip(("coff", "csz", "cks"), parts[1:4]):
            assert got == [str(v) for v in plan[key]], f"{case[:nin]}: {key} {got}, recorded {plan[key]}"
        assert int(parts[0][-1]) == len(plan["coff"])   # nchunks is the length of the chunk tables
        slotf = plan["fields"][golden["plan_fields"].index("SLOTF")]
        assert nbytes == (plan["coff"][-1] + 3 * slotf) * 1024   # last chunk's slot image + the two trailing ones
        assert parts[4] == [str(nbytes), h_stream] + golden["bias"][f"{case[2]},{case[3]}"], f"{case[:nin]}: stream / bias hashes {parts[4]}"
    assert n_ok == 15 * 3 * 7


def test_every_case_maps_to_one_row_and_every_row_is_reached(golden, replayed, table):
    nin = golden["case_fields"].index("|")
    names = golden["plan_fields"]
    reached = set()
    for case, parts in replayed:
        if not case[nin + 1]:
            continue
        f = dict(zip(names, golden["plans"][case[nin + 2]]["fields"]))
        # the recorded members against the rows' template arguments (C3T, PA, PB, NPC, KSA, SLOTF, -, OV, A16, -, KSAC, NCAC, KSAB, NCAB) and
        # the profile name; KPT and the remaining arguments are pinned by the name and by test_the_table_is_the_parents_instantiations
        rows = [i for i, (name, t) in enumerate(table)
                if name == f["name"] and t[:6] == (f["C3T"], f["PA"], f["PB"], f["NPC"], f["KSA"], f["SLOTF"]) and t[7:9] == (f["OVL"], f["A16"])
                and t[10:] == (f["KSAC"], f["NCAC"], f["KSAB"], f["NCAB"]) and (t[10] != 0) == bool(f["SPLIT_A"])]
        assert len(rows) == 1, f"{case[:nin]}: rows {rows}"
        assert rows[0] == int(parts[0][1]), f"{case[:nin]}: planned row {parts[0][1]}, the recorded members are row {rows[0]}"
        reached.add(rows[0])
    assert reached == set(range(len(table))), f"rows no recorded case reaches: {sorted(set(range(len(table))) - reached)}"


def test_the_table_is_the_parents_instantiations(golden, table):
    """the kernel symbols of that commit's code object, as template arguments: 20, each a row, each row one of them"""
    want = sorted(tuple(t) for t in golden["instantiations"])
    assert len(want) == 20 and len(set(want)) == 20
    assert sorted(t for _, t in table) == want

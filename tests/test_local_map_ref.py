"""Two restatements of Tracking::UpdateLocalMap agree on every scene of tests/local_map_scenes.py: the plain-Python one the GPU tests are held
to (tests/local_map_ref.py) and the compiled C++ one on flat tables (examples/local_map_host.cpp), built here into a stand-alone program with
g++ - and once more with -fsanitize=address,undefined, which must run clean on the same scenes.  CPU only."""
import copy
import os
import subprocess

import pytest

import local_map_ref as REF
import local_map_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "examples", f) for f in ("local_map_host_check.cpp", "local_map_host.cpp")]
SCENES = SC.all_scenes() + [SC.frame_1000()]          # slots_262144 has no dense text file: its answer is written out by hand


def expected_lines(sc):
    sc = copy.deepcopy(sc)
    m, L, state, lines = sc["map"], sc["limits"], REF.new_state(), []
    for step in sc["steps"]:
        if "bad_points" in step:
            for s in step["bad_points"]: m["points"][s]["bad"] = 1
            continue
        e = REF.update_local_map(state, m, step["frame"], L["max_local_points"], L["max_local_lines"])
        lst = lambda v: [len(v)] + list(v)
        row = [e["status"], e["n_voted"], e["n_bad_cleared"], e["ref_keyframe"], e["vote_empty"]] + lst(e["frame_ids"])
        if not e["status"] & REF.KEYFRAME_OVERFLOW:
            row += lst(e["local_keyframes"]) + lst(e["local_points"]) + lst(e["local_lines"])
        lines.append(row)
    return lines


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("local_map_host") / ("check_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe] + SOURCES)
    return exe


def test_compiled_host_loops_agree_with_the_python_reference(program, tmp_path):
    for sc in SCENES:
        path = str(tmp_path / (sc["name"] + ".txt"))
        SC.write_text(path, sc)
        r = subprocess.run([program, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 0 and not r.stderr, (sc["name"], r.stderr[-2000:])
        got = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert got == expected_lines(sc), sc["name"]


def test_the_scenes_show_what_they_were_made_for():
    by = {sc["name"]: expected_lines(sc) for sc in SCENES}
    assert len(by) == len(SCENES) >= 40
    assert by["voted_1025"][-1][0] == REF.KEYFRAME_OVERFLOW and by["voted_1024"][-1][0] == 0
    assert by["list_full_plus0"][0][0] == 0 and by["list_full_plus1"][0][0] == REF.POINT_OVERFLOW | REF.LINE_OVERFLOW and by["lines_over"][0][0] == REF.LINE_OVERFLOW
    assert by["empty_vote"][1][4] == 1 and by["tie"][0][3] == 3 and by["bad_voted"][0][3] == 1
    # past the kernels' widths
    sc = {s["name"]: s for s in SCENES}
    kfs = lambda name: lists(by[name][-1])[1]
    for n in (33, 96, 97, 161):
        name = "children_%d" % n
        rows = [sc[name]["map"]["keyframes"][v]["child"] for v in range(6)]
        assert all(len(r) == n for r in rows) and rows[0] == rows[1] and len(kfs(name)) == 12
        assert [rows[v].index(kfs(name)[6 + v]) for v in range(4)] == SC.children_winner_positions(n)
        key = lambda s: sc[name]["map"]["keyframes"][s]["key"]
        assert key(kfs(name)[9]) > 2 ** 63 > key(kfs(name)[8]) and min(key(c) for c in rows[3][:SC.CHILD_LDS]) == 1
    for n in (257, 513):
        _, k, p, l = lists(by["row_%d" % n][0])
        L, K = sc["row_%d" % n]["limits"], sc["row_%d" % n]["map"]["keyframes"]
        assert by["row_%d" % n][0][0] == 0 and k == [0, 1] and len(p) == L["max_local_points"] > 3 * n // 4 and len(l) == L["max_local_lines"] > 3 * n // 4
        assert len(K[1]["points"]) == len(K[1]["lines"]) == n and K[1]["lines"][SC.TILE] == K[1]["lines"][200] == 200 and p.count(200) == l.count(200) == 1
        assert (K[1]["points"][SC.TILE] == 200) == (n > 257) and p[:3] == [n + 1, 2, 255] and sum(s > SC.TILE for s in p) > (n - SC.TILE) // 2
        # the second tile writes first occurrences behind the first tile's: a compaction that drops the carry between tiles gives another list
        for rows, objs in (("points", "points"), ("lines", "lines")):
            live = {s for s, o in sc["row_%d" % n]["map"][objs].items() if not o["bad"]}
            tiles = written_per_tile(K[1][rows], K[0][rows], live)
            assert tiles[0] > 200 and (tiles[1] > 0 or (n, rows) == (257, "lines")), (n, rows, tiles)
    assert by["row_257_over"][0][0] == REF.POINT_OVERFLOW | REF.LINE_OVERFLOW
    _, k, p, l = lists(by["prefix_600"][0])
    assert len(k) == 600 and k != sorted(k) and len(p) == 1500 and len(set(p)) == 1500 and len(l) == 86
    assert kfs("voted_40") == list(range(80)) and len(kfs("voted_80")) == 81 and kfs("voted_80")[80] == 80 and kfs("voted_81") == list(range(81))
    assert [r[2] for r in by["frame_1000"]] == [2, 4] and [r[1] for r in by["frame_1000"]] == [6, 2]
    assert [i for i, v in enumerate(lists(by["frame_1000"][0])[0]) if v >= 0] == [255, 257, 512, 999]
    cut = copy.deepcopy(sc["frame_1000"])                            # a vote that stops at the first 256 keypoints gives other counts
    for step in cut["steps"]: step["frame"][256:] = [-1] * 744
    assert [r[1:3] for r in expected_lines(cut)] == [[1, 0], [0, 1]]


def written_per_tile(row, before, live):
    """how many first occurrences each tile of 256 entries of a row adds to the list, after the rows listed before it"""
    seen, out = set(before), []
    for t in range(0, len(row), SC.TILE):
        fresh = [s for s in dict.fromkeys(row[t:t + SC.TILE]) if s in live and s not in seen]
        seen.update(fresh); out.append(len(fresh))
    return out


def lists(row):
    """the lists of one line of expected_lines: frame ids, local keyframes, local points, local lines"""
    out, at = [], 5
    while at < len(row):
        n = row[at]; out.append(row[at + 1:at + 1 + n]); at += 1 + n
    return out


def test_the_hand_written_answer_of_the_slot_scenes():
    for nk in (33, 1 << 18):
        sc = SC.slots_scene(nk)
        e = REF.update_local_map(REF.new_state(), sc["map"], sc["steps"][0]["frame"], sc["limits"]["max_local_points"], sc["limits"]["max_local_lines"])
        want = SC.slots_expected(nk)
        assert {k: e[k] for k in want} == want and sc["limits"]["max_keyframes"] == nk
        words = (nk + 31) // 32
        assert {s >> 5 for s in want["local_keyframes"]} >= {0, 1, words - 1}
        assert {s & 31 for s in want["local_keyframes"] if s >> 5 == words - 1} >= ({0, 31} if nk > 33 else {0})

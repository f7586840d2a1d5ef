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
SCENES = SC.all_scenes()


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
    assert len(by) == len(SCENES) >= 27
    assert by["voted_1025"][-1][0] == REF.KEYFRAME_OVERFLOW and by["voted_1024"][-1][0] == 0
    assert by["list_full_plus0"][0][0] == 0 and by["list_full_plus1"][0][0] == REF.POINT_OVERFLOW | REF.LINE_OVERFLOW and by["lines_over"][0][0] == REF.LINE_OVERFLOW
    assert by["empty_vote"][1][4] == 1 and by["tie"][0][3] == 3 and by["bad_voted"][0][3] == 1

"""The matcher facade (mc_slam_amd/host/ORBmatcher.cpp) without a GPU: tests/host_facade_matcher_check.cpp includes the source, stands
in for the library with stubs that print what reaches them, and drives all thirteen public functions over a small mock map, then
every refusal.  Every line is compared with tests/golden/facade_matcher_lines.txt, which the same harness recorded from the
ORBmatcher.cpp of the commit in front of the refactor (built with -DFACADE_MATCHER_CPP="<that file>"), so the problem structs, the
write-backs and the messages are pinned byte for byte; the refusal texts and the branches the scene has to take are asserted here
once more so that a reader sees them."""
import os
import re

import pytest

import host_check_lib as hc

GOLDEN = os.path.join(hc.ROOT, "tests", "golden", "facade_matcher_lines.txt")


def golden(section):
    parts = re.split(r"^# (.*)\n", open(GOLDEN).read(), flags=re.M)
    return dict(zip(parts[1::2], parts[2::2]))[section].splitlines()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_facade_matcher_check")


@pytest.fixture(scope="module")
def main_lines(checker):
    return hc.run(checker, [])


@pytest.fixture(scope="module")
def refuse_lines(checker):
    return hc.run(checker, ["refuse"])


def calls(lines):
    """the lines of each call of the main mode, by the name behind "call" """
    out, cur = {}, None
    for l in lines:
        if l.startswith("call "):
            cur = out.setdefault(l[5:], [])
        elif cur is not None:
            cur.append(l)
    return out


def stub(lines):
    """the fields of the stubs' "ok <entry point> <problem> key value ..." lines"""
    return [hc.fields(l) for l in lines if l.startswith("ok ")]


def changed(lines, kind):
    """"now <kind> <id> ..." lines: id -> the tokens behind it"""
    return {int(l.split()[2]): l.split()[3:] for l in lines if l.startswith("now " + kind + " ")}


def test_every_line_equals_the_recording(main_lines, refuse_lines):
    assert main_lines == golden("main mode")
    assert refuse_lines == golden("refuse mode")


def test_thirteen_calls_succeed(main_lines):
    c = calls(main_lines)
    assert len(c) == 13
    for name, lines in c.items():
        ret = [l for l in lines if l.startswith("ret ")]
        assert len(ret) == 1 and ret[0].endswith("msg []") and int(ret[0].split()[1]) >= 0, (name, ret)
        assert stub(lines), name


def plans(lines):
    return [dict(zip(l.split()[1::2], map(int, l.split()[2::2]))) for l in lines if l.startswith("plan ")]


def test_fuse_takes_every_branch(main_lines):
    lines = calls(main_lines)["Fuse"]
    hit = [p for p in plans(lines) if p["hit"]]
    pt, kf = changed(lines, "pt"), changed(lines, "kf")[0][1:]
    first = {}
    for p in hit:
        first.setdefault(p["q"], p["i"])
    fresh = [p for p in hit if first[p["q"]] == p["i"]]
    state = lambda i: pt[i]                                      # the tokens behind "pt <id>": bad <b> ... replaced <id> ...
    query_replaced = [p for p in fresh if p["holder"] >= 0 and not p["hbad"] and p["hobs"] > p["qobs"]]
    holder_replaced = [p for p in fresh if p["holder"] >= 0 and not p["hbad"] and p["hobs"] <= p["qobs"]]
    assert query_replaced and holder_replaced
    for p in query_replaced:     # "pt <q> bad 1 ... replaced <holder>"
        assert state(p["q"])[1] == "1" and state(p["q"])[state(p["q"]).index("replaced") + 1] == str(p["holder"])
    for p in holder_replaced:
        assert state(p["holder"])[1] == "1" and state(p["holder"])[state(p["holder"]).index("replaced") + 1] == str(p["q"])
        assert kf[p["key"]] == str(p["q"])
    assert any(p["hbad"] for p in fresh)                          # the keypoint's point is bad: counted, nothing written
    empty = [p for p in fresh if p["holder"] < 0]
    assert empty and all(kf[p["key"]] == str(p["q"]) for p in empty)
    again = [p for p in hit if first[p["q"]] != p["i"]]           # a query a second time: bad or in the keyframe by then
    assert {p["q"] for p in again} & {p["q"] for p in query_replaced} and {p["q"] for p in again} & {p["q"] for p in empty}
    assert all(kf[p["key"]] == str(p["holder"]) for p in again)
    ret = int([l for l in lines if l.startswith("ret ")][0].split()[1])
    assert ret == len(fresh)


def test_fuse_sim3_takes_every_branch(main_lines):
    lines = calls(main_lines)["Fuse (Sim3)"]
    n_list = len([l for l in lines if l.startswith("list ")][0].split()) - 1
    repl = [int(t) for t in [l for l in lines if l.startswith("out vpReplacePoint")][0].split()[2:]]
    assert 0 < len(repl) < n_list                                 # vpReplacePoint is shorter than vpPoints
    hit = [p for p in plans(lines) if p["hit"]]
    assert any(p["i"] >= len(repl) for p in hit)                  # and a match behind its end is left alone
    good = [p for p in hit if p["i"] < len(repl) and p["holder"] >= 0 and not p["hbad"]]
    assert good and all(repl[p["i"]] == p["holder"] for p in good)
    assert sum(r >= 0 for r in repl) == len(good)
    assert any(p["hbad"] for p in hit if p["i"] < len(repl))
    kf = changed(lines, "kf")[1][1:]
    empty = [p for p in hit if p["i"] < len(repl) and p["holder"] < 0]
    assert empty and all(kf[p["key"]] == str(p["q"]) for p in empty)


@pytest.mark.parametrize("call", ["SearchByProjection", "SearchByProjection (last frame)", "SearchByProjection (loop)",
                                  "SearchByProjection (relocalisation)", "SearchLocalMap"])
def test_key_match_of_every_kind_is_applied(main_lines, call):
    """ProjSearch::apply behind both tracking forms, the loop overload and the relocalisation overload each meet key_match >= 0, -1
    and -2"""
    lines = calls(main_lines)[call]
    f = stub(lines)[0]
    assert f["km_pos"] > 0 and f["km_m2"] > 0 and f["km_m1"] > 0
    if call.endswith("(loop)"):
        assert [l for l in lines if l.startswith("out vpMatched")] and int([l for l in lines if l.startswith("ret ")][0].split()[1]) == f["km_pos"]
    else:
        assert changed(lines, "fr")                               # mvpMapPoints of the frame moved


def test_search_local_map_states(main_lines):
    lines = calls(main_lines)["SearchLocalMap"]
    f = stub(lines)[0]
    assert f["st_0"] > 0 and f["st_7up"] > 0 and f["st_other"] > 0
    assert [l for l in lines if l.startswith("out in_view")][0].split()[2] == str(f["st_0"] + f["st_7up"])
    inview = [t[t.index("inview") + 1] for t in changed(lines, "pt").values()]
    assert "1" in inview and "0" in inview


def test_search_by_sim3_agreement(main_lines):
    lines = calls(main_lines)["SearchBySim3"]
    f = stub(lines)[0]
    assert f["agree"] > 0 and f["disagree"] > 0
    assert int([l for l in lines if l.startswith("ret ")][0].split()[1]) == f["agree"]


def test_bow_batches_carry_three_pairs(main_lines):
    c = calls(main_lines)
    for name in ("SearchByBoW (keyframes against a frame)", "SearchByBoW (a keyframe against keyframes)"):
        f = stub(c[name])
        assert len(f) == 3 and all(p["m21_pos"] > 0 and p["m21_m2"] > 0 and p["m21_m1"] > 0 for p in f)
    for name in ("SearchByBoW (frame)", "SearchByBoW (keyframe)"):
        assert len(stub(c[name])) == 1


TARGET = ["N, mvKeysUn, mvuRight, mvpMapPoints and mDescriptors of {the} {noun} disagree",
          "mnScaleLevels and mvScaleFactors of {the} {noun} disagree",
          "{the} {noun} has no grid",
          "{the} {noun} has a stereo keypoint (the backend is monocular)",
          "a keypoint's octave is outside 0 .. 255"]
NO_DEVICE = "no HIP device (the backend has no CPU path)"
BOW = "N, the keypoints, mvpMapPoints and mDescriptors of a keyframe or frame disagree"


def target(the, noun, levels=None):
    t = [m.format(the=the, noun=noun) for m in TARGET]
    if levels:
        t[1] = levels
    return t


# call of the harness -> (the prefix of its messages, the texts its refusals produce): the literal strings of the facade
MESSAGES = {
    "SearchForTriangulation": ("ORBmatcher::SearchForTriangulation", [
        "N, mvKeysUn, mvpMapPoints and mDescriptors of a keyframe disagree",
        "mvLevelSigma2 and mvScaleFactors of keyframe 2 differ in length",
        "a keypoint's octave is outside 0 .. 255", NO_DEVICE, "stub: the backend call failed"]),
    "Fuse": ("ORBmatcher::Fuse", target("the", "keyframe", "mnScaleLevels, mvScaleFactors and mvInvLevelSigma2 of the keyframe disagree") + [NO_DEVICE]),
    "Fuse (Sim3)": ("ORBmatcher::Fuse (Sim3)", target("the", "keyframe", "mnScaleLevels, mvScaleFactors and mvInvLevelSigma2 of the keyframe disagree")),
    "SearchBySim3": ("ORBmatcher::SearchBySim3", target("a", "keyframe") + [NO_DEVICE]),
    "SearchByProjection": ("ORBmatcher::SearchByProjection", target("the", "frame") + [NO_DEVICE]),
    "SearchByProjection (last frame)": ("ORBmatcher::SearchByProjection (last frame)", target("the", "frame") + [
        "N, mvKeys, mvKeysUn, mvpMapPoints and mvbOutlier of the last frame disagree"]),
    "SearchLocalMap": ("Tracking::SearchLocalPoints", target("the", "frame")),
    "SearchByProjection (loop)": ("ORBmatcher::SearchByProjection (loop)", target("the", "keyframe") + [NO_DEVICE]),
    "SearchByProjection (relocalisation)": ("ORBmatcher::SearchByProjection (relocalisation)", target("the", "frame") + [
        "mvKeysUn and mvpMapPoints of the keyframe disagree"]),
    "SearchByBoW (frame)": ("ORBmatcher::SearchByBoW", [BOW, NO_DEVICE]),
    "SearchByBoW (keyframe)": ("ORBmatcher::SearchByBoW", [BOW]),
    "SearchByBoW (keyframes against a frame)": ("ORBmatcher::SearchByBoW (keyframes against a frame)", [BOW]),
    "SearchByBoW (a keyframe against keyframes)": ("ORBmatcher::SearchByBoW (a keyframe against keyframes)", [BOW]),
}
ARGUMENTS = ["ORBmatcher::SearchForTriangulation: bOnlyStereo is not supported (the backend is monocular)",
             "ORBmatcher::SearchByProjection (last frame): bMono is false (the backend is monocular)",
             "ORBmatcher::SearchBySim3: vpMatches12 must have one entry per keypoint of pKF1",
             "ORBmatcher::SearchByProjection (loop): vpMatched does not have one entry per keypoint of the keyframe"]


def test_refusal_messages(refuse_lines):
    seen = {}
    i = 0
    while refuse_lines[i] != "refuse arguments":
        head, ret, kept = refuse_lines[i:i + 3]
        i += 3
        m = re.fullmatch(r"ret -1 msg \[(.*)\]", ret)
        assert head.startswith("refuse ") and m and kept == "map unchanged", (head, ret, kept)
        seen.setdefault(head[7:].split(" / ")[0], []).append(m.group(1))
    assert set(seen) == set(MESSAGES)
    for call, (who, texts) in MESSAGES.items():
        assert set(seen[call]) == {who + ": " + t for t in texts}, call
    assert refuse_lines[i + 1] == "ret -1 -1 -1 -1 pairs 0"       # vMatchedPairs is cleared in front of the refusal
    assert refuse_lines[i + 2:] == ARGUMENTS + ["map unchanged"]

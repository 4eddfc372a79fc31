"""The slice state's transitions on the host (no GPU): tests/cpp/test_ctx_state.cpp walks every state that
better_flow_amd/csrc/bf_ctx_state.h can reach from a fresh context, each transition under the precondition its call sites
guarantee, holds every transition to the block of assignments it replaced and every reached state to the invariants the readers
in the C-ABI files rely on.  And the walk earns its place: a copy of the header with any ONE assignment of any transition taken
out fails it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "better_flow_amd", "csrc", "bf_ctx_state.h")
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_ctx_state.cpp")


def _walk(tmp_path, name, header=None, opt="-O2"):
    exe = str(tmp_path / name)
    cmd = ["g++", opt, "-std=c++14", "-Wall", "-Werror", SOURCE, "-o", exe]
    if header:
        cmd.insert(1, '-DBF_CTX_STATE_HEADER="%s"' % header)
    subprocess.check_call(cmd)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode()


def test_every_reachable_slice_state_keeps_the_readers_invariants(tmp_path):
    rc, out = _walk(tmp_path, "test_ctx_state")
    print(out)
    assert rc == 0 and out.splitlines()[-1] == "ok", out[-4000:]
    reached = int(out.splitlines()[-2].split()[0])
    assert 1000 < reached <= 1 << 20, reached   # (the walk went somewhere, and the flags are the ones it packs)


def _mutants():
    """(transition, assignment, header text without it) for every assignment in the body of every transition."""
    text = open(HEADER).read()
    out = []
    for m in re.finditer(r"\n    void (\w+)\([^)]*\) \{", text):
        depth, end = 1, m.end()
        while depth:   # the body: up to the brace that closes the function
            depth += {"{": 1, "}": -1}.get(text[end], 0)
            end += 1
        for a in re.finditer(r"\b(\w+) (\^?=) [^;=]+;", text[m.end():end]):
            s, e = m.end() + a.start(), m.end() + a.end()
            out.append((m.group(1), a.group(0), text[:s] + text[e:]))
    return out


def test_the_mutants_cover_every_transition():
    text = open(HEADER).read()
    names = set(re.findall(r"\n    void (\w+)\(", text))
    muts = _mutants()
    assert len(names) >= 25 and len(muts) >= 60
    # (a transition made of calls to others alone has no assignment of its own; none is today)
    assert {n for n, _, _ in muts} == names, names - {n for n, _, _ in muts}


# (every mutant of every transition fails it -- 61 of 61 when this was written; the suite compiles those of the composite ones)
@pytest.mark.parametrize("transition", ["run_began", "events_warped", "window_set", "sorted_outside_plan", "tile_run_collected",
                                        "local_tile_run_collected", "grouping_held"])
def test_a_transition_with_one_assignment_removed_fails_the_walk(tmp_path, transition):
    muts = [m for m in _mutants() if m[0] == transition]
    assert muts
    for i, (_, stmt, text) in enumerate(muts):
        broken = tmp_path / ("mutant_%d.h" % i)
        broken.write_text(text)
        rc, out = _walk(tmp_path, "walk_%d" % i, header=str(broken), opt="-O0")
        assert rc == 1 and "ok" not in out.splitlines()[-1:], "%s without `%s` passes the walk:\n%s" % (transition, stmt, out[-1500:])

"""What the readers of a context's slice state return after every ordered pair of the entries that change it
(tests/ctx_sequences.py), against tests/ctx_sequences_expected.txt: the output of scripts/ctx_sequence_table.py at the commit
before the state became one struct with named transitions (bf_ctx_state.h), recorded twice with identical results.  Line for
line: every return code, and the digest of every call's output (ctx_sequences.NO_DIGEST names the call kinds whose digest the two
recordings did not agree on: none)."""
import gc
import os

import pytest

import ctx_sequences as cs

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ctx_sequences_expected.txt")


def test_call_sequences_equal_the_recorded_table(accel_mod):
    with open(TABLE) as f:
        want = f.read().splitlines()
    assert len(want) == len(cs.CASES) * (2 + len(cs.READERS)) and len(cs.CASES) == 144
    gc.collect()   # (a context an earlier test dropped without closing would count as alive)
    got = cs.table(accel_mod)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    for g, w in diff[:40]:
        print("got  %s\nwant %s" % (g, w))
    assert len(got) == len(want) and not diff, "%d of %d lines differ" % (len(diff), len(want))

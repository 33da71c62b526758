"""Regenerates tests/golden/ref_live.npz.  Run where the reference tree is mounted (needs oracle/_ref/libref.so and libref_native.so):

    python tests/golden/make_live_golden.py

Runs every test that holds the oracle to the compiled reference live, once, with the reference wrapped in a
tests/ref_replay.Recorder, and stores what each call of the reference returned and wrote (the bytes it changed in its output
buffers), with a digest of its inputs.  Elsewhere those tests replay these answers (tests/ref_replay.Replay).  The libref_native.so
answers are those of the reference's -march=native build on the host that ran this script.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import binding  # noqa: E402
from tests import ref_replay, test_cache, test_contract, test_estimate, test_oracle  # noqa: E402

# (key, contract, test function, its arguments besides monkeypatch); the key is the one the test passes to ref_replay.reference
LIVE = [("test_contract.live_against_the_compiled_reference[%s]" % c, c, test_contract.test_live_against_the_compiled_reference, (c,))
        for c in binding.CONTRACTS] + \
       [("test_oracle.live_reference_build_agrees", "off", test_oracle.test_live_reference_build_agrees, ()),
        ("test_cache.oracle_live_against_libref", "off", test_cache.test_oracle_live_against_libref, ()),
        ("test_estimate.oracle_matches_reference_functors_live", "off", test_estimate.test_oracle_matches_reference_functors_live, ())]


def main():
    recordings = {}
    for key, contract, fn, args in LIVE:
        lib = binding.load_ref(contract)
        if lib is None:
            raise SystemExit("oracle/_ref: the %s build of the reference is not available (needs the reference tree)" % contract)
        rec = ref_replay.Recorder(lib)
        with pytest.MonkeyPatch.context() as mp:
            mp.setitem(binding._refs, contract, rec)
            fn(*args, mp)
        recordings[key] = rec
        print("%-60s %5d calls" % (key, len(rec.calls)))
    ref_replay.save(recordings)
    print("wrote %s (%d bytes)" % (ref_replay.GOLD, os.path.getsize(ref_replay.GOLD)))


if __name__ == "__main__":
    main()

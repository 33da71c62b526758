"""CPU: the host side of the segment clustering -- refusals on a handle without a device, the BIC choice and the class ids
(amx_segclust_choose) on hand-written tracker lists against tests/segclust_reference.py, and the key-map file byte for byte."""
import numpy as np
import pytest

import rasr_amd
from rasr_amd import _lib
from tests import segclust_reference as sr


@pytest.mark.parametrize("dim", [0, 65])
def test_dimension_outside_the_bound_is_unsupported(dim):
    with pytest.raises(rasr_amd.AmxError, match="dim") as e:
        rasr_amd.SegmentClustering(None, dim)
    assert e.value.status == _lib.AMX_ERR_UNSUPPORTED


def test_host_only_handle_refuses_and_stays_usable():
    sc = rasr_amd.SegmentClustering(None, 3)
    for kw, status, word in [(dict(infile="spk.cl"), _lib.AMX_ERR_UNSUPPORTED, "infile"), (dict(infile=None), _lib.AMX_ERR_INVALID, "no segments"),
                             (dict(amalgamation=2), _lib.AMX_ERR_INVALID, "amalgamation")]:
        with pytest.raises(rasr_amd.AmxError, match=word) as e:
            sc.cluster(**kw)
        assert e.value.status == status
    with pytest.raises(rasr_amd.AmxError, match="host-only") as e:
        sc.accumulate_dev(np.zeros((2, 3), np.float32), [0, 2])
    assert e.value.status == _lib.AMX_ERR_STATE and sc.segments() == 0


# (parent, child, score): a chain 0 <- 1 <- 2 <- 3, a second cluster 4 <- 5, then the two joined
CHAIN = [(2, 3, -5.0), (1, 2, -1.0), (4, 5, 2.0), (0, 1, -3.5), (0, 4, 1.0)]


@pytest.mark.parametrize("tracker, N, mincluster, maxcluster", [
    (CHAIN, 6, 2, 100000),   # the cumulative minimum lies behind a rise: records 0..3
    (CHAIN, 6, 4, 100000),   # mincluster stops the search after two records
    (CHAIN, 6, 2, 3),        # maxcluster < N forces the first three records and restarts the sum behind them
    (CHAIN, 6, 1, 1),        # one cluster
    ([(0, 1, 4.0), (0, 2, 5.0)], 3, 2, 100000),   # nothing below zero: no merge
    ([], 1, 1, 100000),
])
def test_bic_choice_and_class_ids(tracker, N, mincluster, maxcluster):
    want, best, _ = sr.choose(tracker, N, mincluster, maxcluster)
    got, n_clusters, got_best = rasr_amd.SegmentClustering.choose([t[0] for t in tracker], [t[1] for t in tracker], [t[2] for t in tracker], N,
                                                                  mincluster, maxcluster)
    assert got_best == best and np.array_equal(got, want) and n_clusters == len(set(want))


def test_bic_choice_on_the_chain_by_hand():
    got, n_clusters, best = rasr_amd.SegmentClustering.choose(*zip(*CHAIN), 6)
    assert best == 3 and n_clusters == 2 and got.tolist() == [0, 0, 0, 0, 4, 4]
    got, n_clusters, best = rasr_amd.SegmentClustering.choose(*zip(*CHAIN), 6, maxcluster=3)
    assert best == 3 and got.tolist() == [0, 0, 0, 0, 4, 4]   # forced to record 2, then -3.5 < 0 takes record 3


@pytest.mark.parametrize("tracker, kw, status", [(CHAIN, dict(mincluster=7), _lib.AMX_ERR_UNSUPPORTED), (CHAIN, dict(maxcluster=0), _lib.AMX_ERR_INVALID),
                                                 ([(1, 0, 0.0)], dict(), _lib.AMX_ERR_INVALID), ([(0, 1, 0.0), (1, 2, 0.0)], dict(), _lib.AMX_ERR_INVALID)])
def test_bic_choice_refusals(tracker, kw, status):
    with pytest.raises(rasr_amd.AmxError) as e:
        rasr_amd.SegmentClustering.choose(*zip(*tracker), len(tracker) + 1, **kw)
    assert e.value.status == status


def test_key_map_file_byte_for_byte(tmp_path):
    path = str(tmp_path / "cluster.dump")
    rasr_amd.SegmentClustering.write_map(path, ["corpus/rec1/1", "a&b<\"c\">'"], [1, 3], default_ids=["corpus/rec0/7"])
    assert open(path, "rb").read() == (b'<?xml version="1.0" encoding="ISO-8859-1"?>\n<coprus-key-map>\n'
                                       b'<map-item key="corpus/rec0/7" value="0"/>\n<map-item key="corpus/rec1/1" value="1"/>\n'
                                       b'<map-item key="a&amp;b&lt;&quot;c&quot;&gt;&apos;" value="3"/>\n</coprus-key-map>\n')
    rasr_amd.SegmentClustering.write_map(path, [], [])
    assert open(path, "rb").read() == b'<?xml version="1.0" encoding="ISO-8859-1"?>\n<coprus-key-map>\n</coprus-key-map>\n'

import glob
import os
import sys
from collections.abc import Mapping

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


class GoldenArchive(Mapping):
    """The arrays of one fixture, read like np.load's NpzFile (`.files`, a fresh copy per lookup)."""

    def __init__(self, arrays):
        self._arrays = arrays

    @property
    def files(self):
        return list(self._arrays)

    def __getitem__(self, key):
        return self._arrays[key].copy()

    def __iter__(self):
        return iter(self._arrays)

    def __len__(self):
        return len(self._arrays)


def load_golden(name):
    """tests/golden/<name>.npz joined with its <name>_partN.npz files: make_golden.py splits an
    archive that would pass the size limit of a committed file."""
    stem = os.path.join(GOLDEN, name)
    arrays = {}
    for path in [stem + ".npz"] + sorted(glob.glob(stem + "_part*.npz")):
        with np.load(path, allow_pickle=False) as z:
            for k in z.files:
                assert k not in arrays, (path, k)
                arrays[k] = z[k]
    return GoldenArchive(arrays)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


@pytest.fixture(scope="session")
def g_search():
    return load_golden("newref_search")


@pytest.fixture(scope="session")
def g_pipe():
    return load_golden("pipeline")


def ref_dict_from_golden(g):
    """Reference .npz content stored under the 'ref__' prefix in pipeline.npz."""
    return {k[5:]: g[k] for k in g.files if k.startswith("ref__")}


def sample_from_counts(counts, bpc):
    off = np.concatenate(([0], np.cumsum(bpc)))
    return {str(c + 1): counts[off[c]:off[c + 1]].astype(np.int32) for c in range(24)}

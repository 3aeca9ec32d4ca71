import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


class _Golden:
    """A fixture whose repeated arrays are stored once (tests/golden/make_golden.py:save): each `__alias__` row is
    (name of the repeat, name of the array stored), in the order the arrays were written."""

    def __init__(self, z):
        self._z = z
        alias = z["__alias__"]
        self._alias = {a: b for a, b in alias.tolist()}
        order = [str(n) for n in z["__order__"]]
        self.files = order

    def __getitem__(self, key):
        return self._z[self._alias.get(key, key)]

    def __contains__(self, key):
        return key in self.files

    def keys(self):
        return list(self.files)


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return _Golden(z) if "__alias__" in z.files else z


def golden_jpeg(name):
    """Decoded RGB pixels of a JPEG fixture (tests/golden/<name>.jpg), as the reference's predict.py reads an image."""
    from PIL import Image
    with Image.open(os.path.join(GOLDEN, name + ".jpg")) as im:
        return np.array(im.convert("RGB"))


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


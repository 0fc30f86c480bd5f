"""Writes tests/golden/h5lite_writer_70.h5.gz: what h5lite.write_keras_weights makes of many_keras_layers(seed 2, 70 layers),
and - where h5py is importable - checks that libhdf5 reads every layer name, root attribute and weight of that file back intact.
test_cpu_h5lite.py then asks the writer for the same bytes, so a writer change that libhdf5 has not read is caught without h5py.

    python tests/golden/make_h5_writer_fixture.py [--check-only]
"""
import gzip
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import mgr_amd  # noqa: E402,F401
from mgr_amd import h5lite  # noqa: E402
from tests.helpers import many_keras_layers  # noqa: E402

FIXTURE = os.path.join(HERE, "h5lite_writer_70.h5.gz")


def layers():
    return many_keras_layers(np.random.default_rng(2), 70)


def check_with_libhdf5(path, lay):
    import h5py
    exp = {wn: v for _, ws in lay for wn, v in ws}
    with h5py.File(path, "r") as f:
        names = [n.decode() for n in f.attrs["layer_names"]]
        assert names == [n for n, _ in lay], names[:3]
        assert f.attrs["backend"] == b"tensorflow" and f.attrs["keras_version"] == b"2.1.4"
        n = 0
        for ln in names:
            g = f[ln]
            for wn in g.attrs["weight_names"]:
                wn = wn.decode()
                assert np.array_equal(g[wn][()], exp[wn]) and g[wn].dtype == np.float32, wn
                n += 1
    assert n == len(exp)
    return "libhdf5 %s read %d weights back" % (h5py.version.hdf5_version, n)


if __name__ == "__main__":
    lay = layers()
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "w.h5")
        h5lite.write_keras_weights(p, lay)
        try:
            print(check_with_libhdf5(p, lay))
        except ImportError:
            sys.exit("h5py is not importable here: the fixture is only written where libhdf5 can check it")
        if "--check-only" not in sys.argv:
            with open(p, "rb") as src, gzip.GzipFile(FIXTURE, "wb", mtime=0) as dst:
                dst.write(src.read())
            print("wrote", FIXTURE)

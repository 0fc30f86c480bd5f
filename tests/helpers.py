import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.load(open(os.path.join(GOLDEN, name + ".json")))

    def grab(prefix):
        return {k[len(prefix):].replace("__", "/"): z[k] for k in z.files if k.startswith(prefix)}

    return z, meta, grab


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def many_keras_layers(rng, n):
    """n Keras-style (layer name, [(weight name, array)]) entries, 0 - 2 small float32 weights each (h5lite writer tests)."""
    return [("layer_%03d" % i, [("layer_%03d/w_%d:0" % (i, j), rng.standard_normal((3, 2 + j)).astype(np.float32))
                                for j in range(i % 3)]) for i in range(n)]

import json
import math
import multiprocessing as mp
import os
from multiprocessing import forkserver

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


# ----------------------------------------------------------------------------------------
# the network oracle on a whole batch, in a pool of CPU-only processes
# ----------------------------------------------------------------------------------------
ORACLE_CPUS = 16        # what a GPU box grants a test run, whatever os.cpu_count() says: workers x BLAS threads stays within it


def slice_rand(rand, sub):
    """The injected randomness of the samples `sub`: the LSTM input-dropout masks are (4, B, F), everything else is (B, ...)."""
    return {k: (v[:, sub] if (k.endswith("/mask") and k != "head/mask") else v[sub]) for k, v in rand.items()}


def fork_server_running():
    """True once tests/conftest.py has started multiprocessing's fork server (it does so before anything opens the GPU)."""
    return getattr(forkserver._forkserver, "_forkserver_pid", None) is not None


def _oracle_chunk(args):
    """Pool worker: the oracle's loss_and_grads on a slice of the batch in ONE precision.  The gradients come back as float64,
    scaled to the FULL batch's mean (x chunk / B), so that the slices' gradients add up to the batch's.

    precision "32" is numpy float32 throughout; "32c" is the float32 network with only the CTC lattice in fp64 (at T >= 1000 the
    log-likelihood is -3000 ... -6000, where a float32 log-space lattice resolves 2e-4 ... 5e-4 and dominates everything else)."""
    from threadpoolctl import threadpool_limits
    from oracle import keras_ref as kr
    from oracle import network_ref as nr
    sd, w, xs, labels, il, ll, rand, B, precision, threads = args
    n = labels.shape[0]
    dtype = np.float64 if precision == "" else np.float32
    cast = lambda d: {k: (None if v is None else np.asarray(v, dtype)) for k, v in d.items()}
    ctc = kr.ctc_loss_grad

    def ctc_fp64(P, *a, **kw):
        loss, dz = ctc(P.astype(np.float64), *a, **kw)
        return loss.astype(P.dtype), dz.astype(P.dtype)

    try:
        if precision == "32c":
            kr.ctc_loss_grad = ctc_fp64
        with threadpool_limits(limits=threads):                 # (None: the pools as they are)
            _, lb, g, P = nr.loss_and_grads(sd, cast(w), cast(xs), labels, il, ll, cast(rand))
    finally:
        kr.ctc_loss_grad = ctc
    return lb, {k: v.astype(np.float64) * (n / B) for k, v in g.items()}, P


def oracle_by_slices(sd, w, xs, labels, il, ll, rand, chunk=None, start_server=False, precisions=("", "32")):
    """oracle.network_ref.loss_and_grads over the whole batch in fp64 ("") AND in numpy float32 ("32", the error model of
    tests/test_gpu_baseline_configs.py), cut into slices of `chunk` samples (default: 8 slices), every (slice, precision) pair a
    job of a process pool: at most ORACLE_CPUS workers with ONE BLAS thread each (workers x threads <= ORACLE_CPUS).  The oracle's
    products are one (n, H) x (H, 4H) per time step: they stream the weights and cost the same for n = 1 ... 8, and BLAS threads
    do not help them - E at B = 2, T = 1900 on 16 CPUs: 55 s with 4 threads per worker, 36 - 59 s with one; on an 8-core host
    4 threads per worker took three times as long as one (profiles/reference_shapes_parity.txt).

    The workers are forked from the clean fork server and never open the GPU.  A process that has initialised the GPU must not
    start that server itself, so without a running one (and without start_server, for CPU-only callers) the jobs run in line.

    Returns, per precision p, "lb" + p, "g" + p, "P" + p: per-sample losses (B,), gradients of the batch MEAN loss summed over
    the slices in float64, softmax (B, T, C)."""
    B = labels.shape[0]
    chunk = chunk or max(1, math.ceil(B / 8))
    jobs = []
    for p in precisions:
        for i in range(0, B, chunk):
            sub = slice(i, min(B, i + chunk))
            jobs.append([sd, w, {k: v[sub] for k, v in xs.items()}, labels[sub], il[sub], ll[sub], slice_rand(rand, sub), B, p])
    workers = min(ORACLE_CPUS, len(jobs))
    if start_server or fork_server_running():
        with mp.get_context("forkserver").Pool(workers) as pool:
            res = pool.map(_oracle_chunk, [j + [1] for j in jobs], chunksize=1)
    else:
        res = [_oracle_chunk(j + [None]) for j in jobs]
    out = {}
    per = len(jobs) // len(precisions)
    for n, p in enumerate(precisions):
        rs = res[n * per:(n + 1) * per]
        out["lb" + p] = np.concatenate([np.asarray(r[0], np.float64).reshape(-1) for r in rs])
        out["g" + p] = {k: sum(r[1][k] for r in rs) for k in rs[0][1]}
        out["P" + p] = np.concatenate([r[2] for r in rs])
    return out

"""The networks, batches and engine seeds of the device-RNG replay tests, shared by tests/test_cpu_rng_replay.py (which shows on the
oracle alone that the comparison can see a wrong mask) and tests/test_gpu_rng_replay.py (which holds the engine to the oracle).
Everything is built on the CPU; each case is an update case of tests/update_cases.py (its "rands" come from tests/rng_replay.py).

  fusion_tiny     the golden fusion network: frozen encoders, noise on one stream, encoder / fusion / head dropout; B 3, T 12
  unimodal_tiny   the golden all-trainable two-layer network: its encoder masks are read again by the backward pass and both
                  weight-gradient products.  Its engine seed lies above 2^62: seed * 1000003 wraps modulo 2^64.
  split_wide      two trainable layers of 64 units: layer 1 has 128 inputs at p = 0.5, so its projection and its weight gradient
                  are the transposed split-row products, the second reusing the first's kept-feature lists; B 5, T 23 (odd
                  element counts: the last noise pair is half used)
  split_narrow    the same with 32 units: 64 inputs, below the split-row products' range - the other projection call"""
import copy
import functools

import numpy as np

from oracle import network_ref as nr
from tests import rng_replay as rr
from tests import update_cases as uc

NAMES = ["fusion_tiny", "unimodal_tiny", "split_wide", "split_narrow"]
SEEDS = {"fusion_tiny": 11, "unimodal_tiny": (1 << 62) + 20131901, "split_wide": 5, "split_narrow": 5}
STEPS = 4          # replayed steps per case: three for the step counter, four for the pipelined schedule


def _split_case(name, H):
    spec = {"streams": [{"name": "the_input", "F": 7, "noise": 0.5, "residual": True, "trainable": True,
                         "layers": [{"H": H, "dropout": 0.4}, {"H": H, "dropout": 0.5}]}],
            "fusion": None, "head": {"dropout": 0.5, "C": 6}, "ctc": {"skip": 2, "eps": 1e-8},
            "optimizer": {"lr": 1e-4, "decay": 0.0, "clipvalue": 0.5, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "maxnorm": 3.0}}
    B, T, Lmax = 5, 23, 4
    rng = np.random.default_rng(2013 + H)
    w0 = nr.init_weights(spec, rng)
    for k in w0:
        if k.endswith("/b"):          # (non-zero biases: every gradient path carries something)
            w0[k] = w0[k] + rng.uniform(-0.05, 0.05, w0[k].shape)
        elif k.endswith("/W"):        # (kernels at 4 x the init range, like the golden cases': at the init range the posteriors are
            w0[k] = 4.0 * w0[k]       #  near uniform and the loss hardly notices a mask - test_cpu_rng_replay.py's negative control)
    inputs, labels, il, ll = nr.synthetic_batch(spec, B, T, Lmax, rng, lmin=1, lmax=4)
    return dict(name=name, spec=spec, w0=w0, inputs=inputs, labels=labels, il=il, ll=ll, B=B, T=T, Lmax=Lmax, wfinal=None)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("fusion_tiny", "unimodal_tiny"):
        c = uc.golden_case(name)
        c["wfinal"] = None
    else:
        c = _split_case(name, {"split_wide": 64, "split_narrow": 32}[name])
    c["seed"] = SEEDS[name]
    c["rands"] = [rr.replay(c["spec"], c["B"], c["T"], c["seed"], step) for step in range(STEPS)]
    c["name"] = "rng_" + name
    return c


def move_name(name, n):
    """The key of the n-step run of a case in update_cases.MOVE_MEASURED."""
    return "rng_%s_%d" % (name, n)


def steps(c, n):
    """The case cut to its first n steps (what update_cases.run_trainer runs over)."""
    out = dict(c)
    out["rands"] = c["rands"][:n]
    return out


def without_noise(c):
    """A copy of the case whose streams have no GaussianNoise (the two ways to hand an engine its randomness then run the same
    kernels on the same numbers), with the replays of that spec."""
    out = dict(c)
    out["spec"] = copy.deepcopy(c["spec"])
    for s in out["spec"]["streams"]:
        s["noise"] = 0.0
    out["rands"] = [rr.replay(out["spec"], c["B"], c["T"], c["seed"], step) for step in range(STEPS)]
    return out


def covered(c):
    """What a case's spec draws at all: the keys of its replay.  The tests assert on this what they claim to cover."""
    return set(c["rands"][0])


@functools.lru_cache(maxsize=None)
def oracle_step(name, step, train=True):
    """(loss, loss_b, grads, P) of the fp64 oracle at the case's start weights under the replay of `step` (train=False: no
    randomness at all - the learning phase off)."""
    c = case(name)
    return nr.loss_and_grads(c["spec"], c["w0"], c["inputs"], c["labels"], c["il"], c["ll"], c["rands"][step] if train else None)


@functools.lru_cache(maxsize=None)
def oracle_trajectory(name, n):
    """update_cases.run_trainer in float64 over the replays of steps 0 .. n - 1: (start, end, losses)."""
    w0, wf, losses, _ = uc.run_trainer(steps(case(name), n), np.float64)
    return w0, wf, losses

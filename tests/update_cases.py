"""Network-level cases for the optimizer update (Adam + clip + decay + max-norm), shared by tests/test_cpu_update_ref.py (which
measures the error model and shows what the assertion catches) and tests/test_gpu_network.py (which holds the engine to it).

What is compared is the MOVEMENT w_final - w_0 of every trainable weight, not the weight: four steps at lr = 1e-4 move a weight
by 4e-4, so a comparison of the weights themselves to 1e-4 cannot tell an update from none."""
import copy

import numpy as np

from oracle import network_ref as nr
from tests.helpers import load_case, rel_err

# Largest rel_err of the movement between oracle.network_ref.Trainer in float64 and in numpy float32 (the project's error model,
# precision "32" of tests/helpers.py: float32 weights, states and arithmetic from the float32-rounded start), per weight kind,
# measured on the CPU (tests/test_cpu_update_ref.py::test_movement_error_model re-measures them), and the tolerance: 4 x that,
# for the GPU's other summation orders.  An update wrong by 20 % has rel_err 0.2 (same test: the 0.8 x update fails).
MOVE_MEASURED = {
    "fusion_tiny": {"kernel": 3.11e-04, "recurrent": 9.85e-04, "bias": 1.63e-04, "dense": 4.38e-05, "dense_bias": 6.64e-08},
    "unimodal_tiny": {"kernel": 4.52e-04, "recurrent": 9.09e-04, "bias": 4.25e-04, "dense": 4.91e-05, "dense_bias": 1.03e-07},
    "fusion_bite": {"kernel": 3.06e-07, "recurrent": 7.44e-04, "bias": 2.65e-04, "dense": 2.68e-05, "dense_bias": 1.30e-08},
    "unimodal_layer_bound": {"kernel": 5.68e-05, "recurrent": 8.06e-04, "bias": 3.01e-04, "dense": 4.85e-05, "dense_bias": 1.79e-07},
    # the device-RNG replay cases of tests/rng_cases.py over their first 3 (the pipelined one: 4) replayed steps
    # (tests/test_cpu_rng_replay.py::test_movement_error_model re-measures them)
    "rng_fusion_tiny_3": {"kernel": 1.85e-04, "recurrent": 7.43e-04, "bias": 3.74e-04, "dense": 4.92e-05, "dense_bias": 7.57e-08},
    "rng_unimodal_tiny_3": {"kernel": 1.94e-04, "recurrent": 9.66e-04, "bias": 2.73e-04, "dense": 5.69e-05, "dense_bias": 8.31e-08},
    "rng_split_wide_3": {"kernel": 1.45e-03, "recurrent": 9.50e-04, "bias": 5.39e-04, "dense": 6.87e-05, "dense_bias": 1.55e-05},
    "rng_split_narrow_3": {"kernel": 5.47e-04, "recurrent": 1.95e-03, "bias": 4.05e-04, "dense": 5.94e-05, "dense_bias": 3.12e-06},
    "rng_fusion_tiny_4": {"kernel": 1.88e-04, "recurrent": 8.07e-04, "bias": 2.92e-04, "dense": 4.50e-05, "dense_bias": 7.14e-08},
}
MOVE_FACTOR = 4.0


def move_tol(case, kind):
    return MOVE_FACTOR * MOVE_MEASURED[case][kind]


def golden_case(name):
    """A golden case as update case: the committed start, inputs, per-step randomness - and the float64 end state."""
    z, meta, grab = load_case(name)
    return dict(name=name, spec=meta["spec"], w0=grab("w__"), inputs=grab("x__"), labels=z["labels"], il=z["input_length"],
                ll=z["label_length"], rands=[grab("rs%d__" % s) for s in range(meta["steps"])], B=meta["B"], T=meta["T"],
                Lmax=meta["Lmax"], wfinal=grab("wfinal__"))


def fusion_bite_case():
    """fusion_tiny with a max-norm that bites while decay and clipping are active: maxnorm 0.25 (optimizer-wide: the fusion
    layer's own entry is dropped), decay 1e-2, clipvalue 1e-3, six steps of fresh randomness.  The golden kernels are at 4 x the
    init range (column norms 0.39 ... 0.67, all above the bound); every fifth column is shrunk to 0.3 x so that some start, and
    stay, below it."""
    c = golden_case("fusion_tiny")
    spec = copy.deepcopy(c["spec"])
    spec["fusion"].pop("maxnorm")
    spec["optimizer"].update(maxnorm=0.25, decay=1e-2, clipvalue=1e-3)
    w0 = {k: np.array(v, np.float64) for k, v in c["w0"].items()}
    for d in ("fwd", "bwd"):
        w0["fusion/%s/W" % d][:, ::5] *= 0.3
    rng = np.random.default_rng(6)
    rands = [nr.draw_rand(spec, c["B"], c["T"], rng) for _ in range(6)]
    c.update(name="fusion_bite", spec=spec, w0=w0, rands=rands, wfinal=None)
    return c


def unimodal_layer_bound_case():
    """unimodal_tiny with per-layer bounds that differ from the optimizer-wide 3.0 (as a Keras JSON can carry them): layer 0
    unconstrained (0), layer 1 at 0.2 - below the column norms of BOTH layers' kernels, so layer 0 must keep columns above it."""
    c = golden_case("unimodal_tiny")
    spec = copy.deepcopy(c["spec"])
    spec["streams"][0]["layers"][0]["maxnorm"] = 0.0
    spec["streams"][0]["layers"][1]["maxnorm"] = 0.2
    c.update(name="unimodal_layer_bound", spec=spec, wfinal=None)
    return c


def kernel_names(spec):
    return [n for n, _, tr, kind in nr.weight_names(spec) if tr and kind == "kernel"]


def col_norms(W):
    W = np.asarray(W, np.float64)
    return np.sqrt((W * W).sum(0))


def run_trainer(case, dtype=np.float64):
    """oracle Trainer over the case's steps in `dtype` (from the start rounded to it).  Returns (start, end, losses, and per step
    the column norms of every trainable kernel)."""
    cast = lambda d: {k: np.asarray(v, dtype) for k, v in d.items()}
    w0 = cast(case["w0"])
    tr = nr.Trainer(case["spec"], {k: v.copy() for k, v in w0.items()})
    losses, norms = [], []
    for r in case["rands"]:
        losses.append(tr.train_on_batch(cast(case["inputs"]), case["labels"], case["il"], case["ll"], cast(r)))
        norms.append({n: col_norms(tr.w[n]) for n in kernel_names(case["spec"])})
    return w0, tr.w, losses, norms


def movement_errors(spec, w_end, w_start, ref_end, ref_start):
    """Per weight kind the largest rel_err of (w_end - w_start) against (ref_end - ref_start) over the trainable weights of
    that kind, each side's movement taken from its OWN start (the float32 rounding of a start of 2.0 is 3e-4 of a movement),
    and the name of the weight that has it."""
    worst = {}
    for name, _, tr, kind in nr.weight_names(spec):
        if not tr:
            continue
        mv = np.asarray(w_end[name], np.float64) - np.asarray(w_start[name], np.float64)
        ref = np.asarray(ref_end[name], np.float64) - np.asarray(ref_start[name], np.float64)
        assert np.abs(ref).max() > 0, name
        e = rel_err(mv, ref)
        if e >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (e, name)
    return worst


def assert_movement(case_name, spec, w_end, w_start, ref_end, ref_start):
    worst = movement_errors(spec, w_end, w_start, ref_end, ref_start)
    for kind, (e, name) in sorted(worst.items()):
        print("movement %-22s %-10s rel_err %.3e (tolerance %.3e) at %s" % (case_name, kind, e, move_tol(case_name, kind), name))
    for kind, (e, name) in worst.items():
        assert e <= move_tol(case_name, kind), (case_name, kind, name, e, move_tol(case_name, kind))
    return worst

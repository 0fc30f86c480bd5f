"""Per-sample sequence lengths: the reserved key of a batch's input dict and the checks the engine makes on it before
it enqueues anything.  Plain numpy: tests/test_cpu_seqlen.py calls these without a GPU."""
import numpy as np

KEY = "seq_length"


def normalize(seq_length, B, T):
    """seq_length as an int32 array (B,): accepts (B,) or (B, 1) of integers (or floats that hold integers) in [0, T]."""
    a = np.asarray(seq_length)
    if a.shape not in ((B,), (B, 1)):
        raise ValueError("%s: expected shape (%d,) or (%d, 1), got %s" % (KEY, B, B, a.shape))
    a = a.reshape(B)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError("%s: expected integers, got dtype %s" % (KEY, a.dtype))
    if not np.issubdtype(a.dtype, np.integer):
        if not np.all(np.isfinite(a)) or np.any(a != np.round(a)):
            raise ValueError("%s: expected integers, got %s" % (KEY, a))
    a = a.astype(np.int64)
    if np.any(a < 0) or np.any(a > T):
        raise ValueError("%s: values outside [0, T = %d]: %s" % (KEY, T, a))
    return a.astype(np.int32)


def of(inputs, B, T):
    """The lengths an input dict carries, normalized, or None when it has no KEY (or is None itself)."""
    if inputs is None or KEY not in inputs or inputs[KEY] is None:
        return None
    return normalize(inputs[KEY], B, T)


def frames(lens, skip):
    """The CTC input length of each sample: max(0, len - skip)."""
    return np.maximum(0, np.asarray(lens, np.int64) - int(skip)).astype(np.int32)


def check_batch(inputs, B, T, skip, input_length=None, data_parallel=False, frontend=False, augment=False):
    """Everything the engine checks on a batch's lengths, before anything is enqueued.  Returns the lengths (int32 (B,)) or None
    when the batch carries none (then nothing else is looked at).  Raises ValueError on a wrong shape, non-integers, values outside
    [0, T], an input_length[b] above max(0, len[b] - skip), and on lengths given to a data-parallel engine, to a network with a CNN
    front-end, or together with set_augment (the warp and the masks are defined over T)."""
    lens = of(inputs, B, T)
    if lens is None:
        return None
    if data_parallel:
        raise ValueError("%s on an engine with a communicator: data-parallel steps take no per-sample lengths" % KEY)
    if frontend:
        raise ValueError("%s on a network with a CNN front-end is not supported" % KEY)
    if augment:
        raise ValueError("%s together with set_augment: the time warp and the masks are defined over T (set_augment(None) first)" % KEY)
    if input_length is not None:
        il = np.asarray(input_length).reshape(-1)
        if il.shape != (B,):
            raise ValueError("input_length: expected %d values, got shape %s" % (B, np.shape(input_length)))
        room = frames(lens, skip)
        if np.any(il > room):
            b = int(np.argmax(il > room))
            raise ValueError("input_length[%d] = %d above max(0, %s[%d] - skip) = %d" % (b, int(il[b]), KEY, b, int(room[b])))
    return lens

"""numpy restatement of mgr_segment_overlap (no GPU): per class a boolean frame mask for each side, counted."""
import numpy as np


def frame_masks(segments, n_classes, n_frames, ignore=()):
    """segments: [(label, first, last, ...)] inclusive frames -> bool (n_classes, n_frames).  Skipped: a label outside [0, n_classes), an
    ignored one, first < 0; extents are clipped to [0, n_frames)."""
    n = max(int(n_frames), 0)
    m = np.zeros((n_classes, n), bool)
    for s in segments:
        lab, first, last = int(s[0]), int(s[1]), int(s[2])
        if not 0 <= lab < n_classes or lab in ignore or first < 0:
            continue
        m[lab, first:min(last, n - 1) + 1] = True
    return m


def overlap(hyp_segments, ref_segments, n_classes, n_frames, ignore=()):
    """Per sample lists of segments -> (inter, union, hyp_frames, ref_frames), each int32 (B, n_classes)."""
    B = len(hyp_segments)
    n_frames = np.broadcast_to(np.asarray(n_frames), (B,))
    out = np.zeros((4, B, n_classes), np.int32)
    for b in range(B):
        h = frame_masks(hyp_segments[b], n_classes, n_frames[b], ignore)
        r = frame_masks(ref_segments[b], n_classes, n_frames[b], ignore)
        out[:, b] = (h & r).sum(axis=1), (h | r).sum(axis=1), h.sum(axis=1), r.sum(axis=1)
    return tuple(out)


# hand-worked cases, one sample each
HAND = [
    # name, hyp, ref, n_classes, n_frames, ignore, inter, union, hyp_frames, ref_frames
    ("disjoint", [(0, 0, 3)], [(0, 6, 9)], 2, 10, (), [0, 0], [8, 0], [4, 0], [4, 0]),
    ("nested", [(1, 2, 7)], [(1, 4, 5)], 2, 10, (), [0, 2], [0, 6], [0, 6], [0, 2]),
    ("same class united", [(0, 0, 4), (0, 3, 6)], [(0, 2, 9)], 1, 10, (), [5], [10], [7], [8]),
    ("class only in the hypothesis", [(0, 0, 4), (1, 5, 9)], [(0, 0, 4)], 2, 10, (), [5, 0], [5, 5], [5, 5], [5, 0]),
    ("ignored class", [(0, 0, 4), (1, 5, 9)], [(0, 0, 4), (1, 0, 9)], 2, 10, (1,), [5, 0], [5, 0], [5, 0], [5, 0]),
    ("clipped at n_frames", [(0, 5, 20)], [(0, 8, 30), (1, 12, 14)], 2, 10, (), [2, 0], [5, 0], [5, 0], [2, 0]),
    ("empty reference", [(0, 1, 2)], [], 2, 10, (), [0, 0], [2, 0], [2, 0], [0, 0]),
    ("skipped: label out of range, negative first", [(2, 0, 3), (0, -1, 3), (-1, 0, 3)], [(0, 0, 3)], 2, 10, (), [0, 0], [4, 0], [0, 0], [4, 0]),
    ("different classes overlap", [(0, 0, 5), (1, 3, 8)], [(0, 0, 5), (1, 3, 8)], 2, 10, (), [6, 6], [6, 6], [6, 6], [6, 6]),
]

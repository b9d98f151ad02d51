"""Restatements the ensembling path is tested against (test_ensemble_host.py, test_gpu_ensemble.py).

`ensemble`: fp64, built on export_ref.resample_logits -- per member the logits resampled to the common shape, an fp64
softmax, then the mean over the members, its argmax and the top-2 margin of the MEAN PROBABILITIES (which is what decides
whether two channels can swap under the device's fp32 error).
`average_probabilities`: the reference's ensemble.py:17-29 in numpy fp32, same order (avg = p_0; avg += p_m; avg /= M).
"""
import numpy as np

import export_ref as REF


def softmax64(res):
    e = np.exp(res - res.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def ensemble(members, new_shape, full, lo, transpose_backward, separate_z_axes=None):
    """members: list of float32 logits [K, d_m, h_m, w_m] -> (uint8 segmentation, fp64 mean probabilities [K, ...], fp64
    top-2 margin of the mean, bool inside-the-bbox) in the original axis order; outside the bbox: label 0, mean 1 in
    channel 0, margin inf."""
    axes = [None] * len(members) if separate_z_axes is None else list(separate_z_axes)
    mean = None
    for x, ax in zip(members, axes):
        p = softmax64(REF.resample_logits(x, new_shape, ax))
        mean = p if mean is None else mean + p
    mean = mean / len(members)
    seg = mean.argmax(0).astype(np.uint8)
    s = np.sort(mean, 0)
    margin = s[-1] - s[-2]
    segf = REF.paste_transpose(seg, full, lo, transpose_backward)
    meanf = REF.paste_transpose(mean, full, lo, transpose_backward)
    inside = REF.paste_transpose(np.ones(seg.shape, bool), full, lo, transpose_backward)
    meanf[0][~inside] = 1
    marf = REF.paste_transpose(margin, full, lo, transpose_backward, fill=np.inf)
    return segf, meanf, marf, inside


def average_probabilities(list_of_probabilities):
    assert len(list_of_probabilities), 'At least one volume must be given'
    avg = None
    for p in list_of_probabilities:
        if avg is None:
            avg = np.array(p, copy=True)
            if avg.dtype != np.float32:
                avg = avg.astype(np.float32)
        else:
            avg += p
    avg /= len(list_of_probabilities)
    return avg


def merge(list_of_probabilities):
    """(uint8 argmax of the fp32 mean, the mean)"""
    avg = average_probabilities(list_of_probabilities)
    return avg.argmax(0).astype(np.uint8), avg

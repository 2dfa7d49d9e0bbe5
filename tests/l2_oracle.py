"""float64 restatement of the L2 weight penalty of include/dl3.h (dl3_l2_penalty) and of its host-built run table —
numpy and math only, written from the formulas, nothing of the package.

[TF-semantics: Keras 2.2.4 keras/regularizers.py — l2(l) on a weight w adds l * sum(w**2) to the total loss, gradient
2*l*w — restated from memory; the package is not installed.]"""
import math

import numpy as np

TILE = 1024   # elements of one run per tile (the header's contract)


def penalty(p, runs, coef):
    """the truth of out[0]: sum_s coef[s] * sum_{i in run s} p[i]^2.  The squares of floats are exact in double; every
    run's sum is math.fsum (rounded once), times the coefficient (once), and the runs are summed with math.fsum."""
    p = np.asarray(p, np.float32)
    terms = []
    for (first, length), c in zip(runs, coef):
        w = p[first:first + length].astype(np.float64)
        terms.append(float(np.float32(c)) * math.fsum(w * w))
    return math.fsum(terms)


def scale(gs, denom=None, dt=np.float64):
    """sc as dl3_opt_step forms it: gs, or gs / max(denom, 1e-20)"""
    return dt(np.float32(gs)) if denom is None else dt(np.float32(gs)) / np.maximum(dt(np.float32(denom)), dt(1e-20))


def gradient(p, g, runs, coef, gs=1.0, denom=None):
    """g + (2 * coef[s] * p) / sc on the runs, g elsewhere.  -> (expected, magnitude): the magnitude is |g| + |addend| on
    the runs (the terms of the one sum an element is made of)"""
    p, g = np.asarray(p, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    sc = float(scale(gs, denom))
    out, mag = g.copy(), np.abs(g)
    for (first, length), c in zip(runs, coef):
        add = (2.0 * float(np.float32(c)) * p[first:first + length]) / sc
        out[first:first + length] += add
        mag[first:first + length] += np.abs(add)
    return out, mag


def run_index(runs):
    """flat indices of every element on the runs"""
    return np.concatenate([np.arange(f, f + n, dtype=np.int64) for f, n in runs]) if len(runs) else np.zeros(0, np.int64)


def expected_table(slots, table, kind):
    """the run table of one arena, from the slot list: slots = {name: (kind, offset, size, ...)}, table = {name: l}.
    Slots are multiples of 4 floats; a regularised slot that starts where the previous regularised slot's 4-rounded end
    is, with the same float32 l, continues its run.  -> (runs [[first, length, first tile]], coef, tiles)"""
    mine = sorted((v[1], v[2], np.float32(table[n])) for n, v in slots.items() if v[0] == kind and table.get(n, 0) > 0)
    runs, coef = [], []
    for off, size, l in mine:   # noqa: E741
        if runs and coef[-1] == l and -(-(runs[-1][0] + runs[-1][1]) // 4) * 4 == off:
            runs[-1][1] = off + size - runs[-1][0]
        else:
            runs.append([off, size, 0])
            coef.append(l)
    tiles = 0
    for r in runs:
        r[2] = tiles
        tiles += -(-r[1] // TILE)
    return runs, coef, tiles


def model_penalty(weights, table):
    """sum over the table of l * sum(w**2) on host weights {name: array}, the coefficient as the float the device holds"""
    return math.fsum(float(np.float32(l)) * math.fsum((np.asarray(weights[n], np.float32).astype(np.float64) ** 2).ravel())
                     for n, l in sorted(table.items()))

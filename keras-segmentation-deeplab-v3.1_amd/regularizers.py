"""keras.regularizers as far as the path goes: `l2`, the weight decay of DeepLab's training recipe.

[TF-semantics: Keras 2.2.4 keras/regularizers.py, restated from memory: L1L2.__call__ returns l2 * sum(square(x)), and
`l2(l=0.01)` is L1L2(l2=l).]  A layer keyword (`kernel_regularizer=l2(4e-5)`) stores the object; Model.compile() collects
{weight name: l} and the training engine evaluates value and gradient on the device (dl3_l2_penalty).  Host-only module.
"""
import math

import numpy as np

# every regulariser keyword of the layers on the path -> the suffix of the weight it names
KEYWORDS = {"kernel_regularizer": "/kernel:0", "bias_regularizer": "/bias:0", "depthwise_regularizer": "/depthwise_kernel:0",
            "gamma_regularizer": "/gamma:0", "beta_regularizer": "/beta:0"}


class l2:
    """keras.regularizers.l2: the penalty l * sum(w**2) on the weight that carries it"""

    def __init__(self, l=0.01):   # noqa: E741 (Keras' own parameter name)
        if isinstance(l, bool) or not isinstance(l, (int, float, np.integer, np.floating)):
            raise TypeError("l2(l=%r): l must be a number" % (l,))
        if not math.isfinite(float(l)) or float(l) < 0:
            raise ValueError("l2(l=%r): l must be finite and >= 0" % (l,))
        self.l2 = float(l)
        self.l1 = 0.0   # (Keras' L1L2 carries both; l1 is out of scope and always 0)

    def __call__(self, w):
        """the float64 penalty of a host array"""
        w = np.asarray(w, np.float64)
        return float(self.l2 * np.sum(w * w))

    def get_config(self):
        return {"l1": 0.0, "l2": self.l2}

    @classmethod
    def from_config(cls, config):
        if float(config.get("l1", 0.0)) != 0.0:
            raise ValueError("l1 regularisers are not on the path (config %r)" % (config,))
        return cls(config.get("l2", 0.0))

    def __repr__(self):
        return "l2(%r)" % self.l2


def check(reg, what):
    """a layer's regulariser: None or this package's l2.  A foreign object or a bare callable is not silently ignored."""
    if reg is not None and not isinstance(reg, l2):
        raise TypeError("%s=%r: only None or dl3 regularizers.l2(...) is understood (l1 / l1_l2 / callables are not on "
                        "the path)" % (what, reg))
    return reg


def take_keywords(layer, kw, **own):
    """__init__ of a layer: stores its own regulariser keywords (`own`: keyword -> value) as plain attributes and refuses
    the ones in **kw it cannot honour — activity_regularizer (NotImplementedError) and a regulariser that names a weight
    the layer does not have.  Other unknown keywords stay ignored, as before."""
    if kw.get("activity_regularizer") is not None:
        raise NotImplementedError("%s(activity_regularizer=...): activity regularisers are not on the path" % layer.kind)
    for k in KEYWORDS:
        if k not in own and kw.get(k) is not None:
            raise ValueError("%s(%s=...): the layer has no such weight" % (layer.kind, k))
    for k, v in own.items():
        setattr(layer, k, check(v, "%s(%s)" % (layer.kind, k)))


def collect(layers):
    """{weight name: l} over the layers, for l > 0 — Model.compile()'s collection.  Raises TypeError for anything that is
    neither None nor an l2, ValueError for a regulariser that names a weight its layer does not have (bias_regularizer
    on a layer built without bias, kernel_regularizer set on a BatchNormalization...)."""
    table = {}
    for layer in layers:
        if getattr(layer, "activity_regularizer", None) is not None:
            raise NotImplementedError("layer %s: activity regularisers are not on the path" % layer.name)
        for k, suffix in KEYWORDS.items():
            reg = check(getattr(layer, k, None), "layer %s: %s" % (layer.name, k))
            if reg is None:
                continue
            name = layer.name + suffix
            if name not in layer.weights:
                raise ValueError("layer %s: %s names the weight %s, which the layer does not have" % (layer.name, k, name))
            if reg.l2 > 0:
                table[name] = reg.l2
    return table


def normal_form(table):
    """the engine keyword `l2`: a dict or an iterable of (weight name, l) -> the hashable tuple of (name, l) pairs sorted
    by name with l > 0, or None where nothing is regularised (the plain engine key)"""
    if table is None:
        return None
    items = table.items() if isinstance(table, dict) else table
    out = []
    for name, l in items:   # noqa: E741
        l = float(l)   # noqa: E741
        if not math.isfinite(l) or l < 0:
            raise ValueError("l2 table: %s carries l = %r (finite and >= 0 expected)" % (name, l))
        if l > 0:
            out.append((str(name), l))
    return tuple(sorted(out)) or None


TILE = 1024   # elements of one run per tile: L2_TILE of csrc/l2reg.hip


def build_runs(slots, table, kind):
    """dl3_l2_penalty's table over one arena.  slots: Engine.slots ({weight name: (kind, offset, size, ...)}), table: the
    normal form, kind: 'p' (parameter arena) or 's' (state arena).  -> (runs int64 [S,3]: first element, length, first
    tile; coef float32 [S]; tiles).  A slot is a multiple of 4 floats and its padding holds exact zeros, so neighbours
    with the same l merge into one run across the padding between them."""
    known = dict(table or ())
    missing = sorted(n for n in known if n not in slots)
    if missing:
        raise ValueError("l2 table names weights the model does not have: %s" % missing[:4])
    mine = sorted((v[1], v[2], known[n]) for n, v in slots.items() if v[0] == kind and n in known)
    runs = []
    for off, size, l in mine:   # noqa: E741
        if size < 1:
            continue
        if runs and runs[-1][2] == np.float32(l) and (runs[-1][0] + runs[-1][1] + 3) // 4 * 4 == off:
            runs[-1][1] = off + size - runs[-1][0]
        else:
            if runs and runs[-1][0] + runs[-1][1] > off:
                raise ValueError("overlapping arena slots at %d" % off)
            runs.append([int(off), int(size), np.float32(l)])
    out = np.zeros((len(runs), 3), np.int64)
    tiles = 0
    for s, (off, size, _) in enumerate(runs):
        out[s] = (off, size, tiles)
        tiles += (size + TILE - 1) // TILE
    return out, np.asarray([r[2] for r in runs], np.float32), int(tiles)

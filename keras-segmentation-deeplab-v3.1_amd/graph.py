"""Host-side mirror of the small slice of the Keras functional API that the reference's hot path
touches (deeplabv3p.py:29-40 imports; used at :47-206, :260-452; utils.py:181-198).

Pure Python + numpy: layers only DECLARE the graph (names, hyper-parameters, weight shapes and
host master copies of the weights).  All arithmetic happens in libdl3.so through engine.py.
What callers of the reference touch is reproduced: `Model.input/.output/.layers/.name`,
`layer.name/.output/.trainable/.get_weights()/.set_weights()`, `Model(inputs, outputs)` re-wiring
(utils.py:181,:193,:198), Keras 2.2.4 layer ordering (`layers[-5]`) and auto-naming.
"""
import collections
import math
import os

import numpy as np

from . import regularizers

_uids = collections.defaultdict(int)
_rng = np.random.default_rng(0)


def check_mining(mining):
    """(top_k_percent_pixels, hard_example_mining_step) -> (float p, int S), or None where mining is off (None, p == 1);
    ValueError for p outside (0, 1], a negative or non-integer S"""
    if mining is None:
        return None
    p, S = mining
    if isinstance(p, bool) or not isinstance(p, (int, float, np.floating, np.integer)) or not 0.0 < float(p) <= 1.0:
        raise ValueError("top_k_percent_pixels must be a number in (0, 1], got %r" % (p,))
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or int(S) < 0:
        raise ValueError("hard_example_mining_step must be an integer >= 0, got %r" % (S,))
    if float(p) == 1.0:
        return None
    return float(p), int(S)


def check_jaccard(weight):
    """jaccard_weight of the soft-Jaccard loss -> float lambda, or None where the term is off (None, 0); ValueError for
    anything that is not a finite number >= 0"""
    if weight is None:
        return None
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.floating, np.integer)) \
            or not 0.0 <= float(weight) <= float(np.finfo(np.float32).max):   # (the launch takes it as a float)
        raise ValueError("jaccard_weight must be a finite number >= 0, got %r" % (weight,))
    return float(weight) or None


def check_focal(focal):
    """(gamma, alpha) of the focal loss -> (float gamma, tuple alpha or None), or None where the loss is off (None; gamma
    == 0 with alpha None or all ones: the cross-entropy).  alpha: None, one number (broadcast to every class; so is a
    one-element sequence) or one number per class.  ValueError for a gamma that is not a finite number >= 0 and for an
    alpha entry that is not one"""
    if focal is None:
        return None
    gamma, alpha = focal
    fmax = float(np.finfo(np.float32).max)   # (the launch takes gamma as a float, the device holds alpha as floats)

    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.floating, np.integer)) and 0.0 <= float(v) <= fmax
    if not number(gamma):
        raise ValueError("gamma must be a finite number >= 0, got %r" % (gamma,))
    if alpha is not None:
        entries = [alpha] if np.ndim(alpha) == 0 else list(np.asarray(alpha, object).reshape(-1))
        if not entries or not all(number(a) for a in entries):
            raise ValueError("alpha must be None, a finite number >= 0 or one such number per class, got %r" % (alpha,))
        alpha = tuple(float(a) for a in entries)
        if all(a == 1.0 for a in alpha):
            alpha = None
    if float(gamma) == 0.0 and alpha is None:
        return None
    return float(gamma), alpha


def raw_pixels(x):
    """raw 0-255 pixels as the package takes them: a device tensor or a uint8 array (decoded images) as it is, anything
    else as a float32 array (the reference's arrays)"""
    if not hasattr(x, "data_ptr") and not (isinstance(x, np.ndarray) and x.dtype == np.uint8):
        x = np.asarray(x, np.float32)
    return x


def batches(n, batch_size):
    """the slices that cut n samples into forward batches: min(batch_size, n) consecutive samples, a short last one"""
    bs = min(int(batch_size), n)
    return [slice(i, i + bs) for i in range(0, n, bs)]


def clear_session(seed=0):
    """keras.backend.clear_session(): reset auto-naming counters (and the weight-init RNG)."""
    global _rng
    _uids.clear()
    _rng = np.random.default_rng(seed)


def set_seed(seed):
    global _rng
    _rng = np.random.default_rng(seed)


def _auto_name(prefix):
    _uids[prefix] += 1
    return "%s_%d" % (prefix, _uids[prefix])


def glorot_uniform(shape, fan_in, fan_out):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return _rng.uniform(-lim, lim, shape).astype(np.float32)


def glorot_normal(shape, fan_in, fan_out):
    """tf.glorot_normal_initializer (default of icnr_weights, subpixel.py:9): truncated normal,
    stddev = sqrt(2/(fan_in+fan_out))/.87962566 [TF-semantics]; the RNG stream itself is not
    reproducible against TF, only the distribution."""
    std = math.sqrt(2.0 / (fan_in + fan_out)) / 0.87962566103423978
    v = _rng.normal(0.0, std, shape)
    bad = np.abs(v) > 2 * std
    while bad.any():
        v[bad] = _rng.normal(0.0, std, int(bad.sum()))
        bad = np.abs(v) > 2 * std
    return v.astype(np.float32)


class KTensor:
    """Symbolic tensor: static shape without the batch axis, and the layer that produced it."""

    def __init__(self, shape, layer):
        self.shape = tuple(shape)
        self.layer = layer
        self._keras_shape = (None,) + self.shape  # read by the reference at deeplabv3p.py:168

    def __repr__(self):
        return "<KTensor %s from %s>" % (self.shape, self.layer.name)


class Layer:
    kind = "Layer"
    prefix = "layer"

    def __init__(self, name=None, **cfg):
        self.name = name or _auto_name(self.prefix)
        self.cfg = cfg
        self.trainable = True
        self.inbound = []
        self.output = None
        self.weights = collections.OrderedDict()  # "<layer>/<var>:0" -> np.ndarray (host master copy)
        self._engine = None

    # Keras: layer(x) / layer([a, b])
    def __call__(self, x):
        ins = list(x) if isinstance(x, (list, tuple)) else [x]
        assert self.output is None, "layer %s called twice (shared layers are not on the path)" % self.name
        self.inbound = ins
        self.output = KTensor(self.compute_output_shape([t.shape for t in ins]), self)
        self.build([t.shape for t in ins])
        return self.output

    @property
    def input(self):
        return self.inbound[0] if len(self.inbound) == 1 else self.inbound

    def build(self, in_shapes):
        pass

    def compute_output_shape(self, in_shapes):
        return in_shapes[0]

    def weight_names(self):
        return list(self.weights.keys())

    def get_weights(self):
        if self._engine is not None:
            self._engine.sync_layer_to_host(self)
        return [w.copy() for w in self.weights.values()]

    def set_weights(self, ws):
        names = list(self.weights.keys())
        if len(ws) != len(names):
            raise ValueError("layer %s expects %d weight arrays, got %d" % (self.name, len(names), len(ws)))
        for n, w in zip(names, ws):
            w = np.asarray(w, np.float32)
            if w.shape != self.weights[n].shape:
                raise ValueError("layer %s weight %s: shape %s != %s" % (self.name, n, w.shape, self.weights[n].shape))
            self.weights[n] = w.copy()
        if self._engine is not None:
            self._engine.sync_layer_to_device(self)

    def count_params(self):
        return int(sum(w.size for w in self.weights.values()))


class InputLayer(Layer):
    kind = "InputLayer"
    prefix = "input"


def Input(shape=None, tensor=None, name=None):
    """keras.layers.Input (deeplabv3p.py:261,:264).  `tensor` may be a numpy/torch array whose
    trailing dims give the shape; it is remembered as the model's default feed."""
    lyr = InputLayer(name=name)
    if shape is None and tensor is not None:
        shape = tuple(tensor.shape[1:])
    lyr.output = KTensor(shape, lyr)
    lyr.cfg["tensor"] = tensor
    return lyr.output


def _same_out(size, stride):
    return -(-size // stride)


class Conv2D(Layer):
    """keras.layers.Conv2D restricted to what the path uses: k in {1,3}, dilation 1, groups 1."""
    kind = "Conv2D"
    prefix = "conv2d"

    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", use_bias=True, dilation_rate=(1, 1),
                 activation=None, name=None, kernel_initializer="glorot_uniform", kernel_regularizer=None,
                 bias_regularizer=None, **kw):
        super().__init__(name=name)
        # Keras' regulariser keywords (regularizers.py): plain attributes, collected at compile()
        regularizers.take_keywords(self, kw, kernel_regularizer=kernel_regularizer, bias_regularizer=bias_regularizer)
        if bias_regularizer is not None and not use_bias:
            raise ValueError("%s(use_bias=False, bias_regularizer=...): the layer has no bias" % self.kind)
        k = kernel_size[0] if isinstance(kernel_size, (tuple, list)) else kernel_size
        s = strides[0] if isinstance(strides, (tuple, list)) else strides
        r = dilation_rate[0] if isinstance(dilation_rate, (tuple, list)) else dilation_rate
        assert activation is None and r == 1
        self.cfg.update(filters=int(filters), k=int(k), stride=int(s), padding=padding, use_bias=bool(use_bias), rate=1)

    def compute_output_shape(self, in_shapes):
        H, W, _ = in_shapes[0]
        c = self.cfg
        if c["padding"] == "same":
            return (_same_out(H, c["stride"]), _same_out(W, c["stride"]), c["filters"])
        return ((H - c["k"]) // c["stride"] + 1, (W - c["k"]) // c["stride"] + 1, c["filters"])

    def build(self, in_shapes):
        cin, c = in_shapes[0][2], self.cfg
        k, f = c["k"], c["filters"]
        self.weights[self.name + "/kernel:0"] = glorot_uniform((k, k, cin, f), k * k * cin, k * k * f)
        if c["use_bias"]:
            self.weights[self.name + "/bias:0"] = np.zeros((f,), np.float32)


class DepthwiseConv2D(Layer):
    kind = "DepthwiseConv2D"
    prefix = "depthwise_conv2d"

    def __init__(self, kernel_size, strides=(1, 1), padding="valid", use_bias=True, dilation_rate=(1, 1),
                 activation=None, name=None, depthwise_regularizer=None, **kw):
        super().__init__(name=name)
        regularizers.take_keywords(self, kw, depthwise_regularizer=depthwise_regularizer)
        k = kernel_size[0] if isinstance(kernel_size, (tuple, list)) else kernel_size
        s = strides[0] if isinstance(strides, (tuple, list)) else strides
        r = dilation_rate[0] if isinstance(dilation_rate, (tuple, list)) else dilation_rate
        assert k == 3 and not use_bias and activation is None
        self.cfg.update(k=3, stride=int(s), padding=padding, rate=int(r))

    def compute_output_shape(self, in_shapes):
        H, W, C = in_shapes[0]
        c = self.cfg
        if c["padding"] == "same":
            return (_same_out(H, c["stride"]), _same_out(W, c["stride"]), C)
        keff = (c["k"] - 1) * c["rate"] + 1
        return ((H - keff) // c["stride"] + 1, (W - keff) // c["stride"] + 1, C)

    def build(self, in_shapes):
        C = in_shapes[0][2]
        # Keras DepthwiseConv2D glorot fans: fan_in = kh*kw*C, fan_out = kh*kw*depth_multiplier
        self.weights[self.name + "/depthwise_kernel:0"] = glorot_uniform((3, 3, C, 1), 9 * C, 9)


class BatchNormalization(Layer):
    kind = "BatchNormalization"
    prefix = "batch_normalization"

    def __init__(self, epsilon=1e-3, momentum=0.99, name=None, gamma_regularizer=None, beta_regularizer=None, **kw):
        super().__init__(name=name)
        regularizers.take_keywords(self, kw, gamma_regularizer=gamma_regularizer, beta_regularizer=beta_regularizer)
        self.cfg.update(eps=float(epsilon), momentum=float(momentum))

    def build(self, in_shapes):
        C = in_shapes[0][-1]
        n = self.name
        self.weights[n + "/gamma:0"] = np.ones((C,), np.float32)
        self.weights[n + "/beta:0"] = np.zeros((C,), np.float32)
        self.weights[n + "/moving_mean:0"] = np.zeros((C,), np.float32)
        self.weights[n + "/moving_variance:0"] = np.ones((C,), np.float32)


class Activation(Layer):
    """'relu', 'relu6' (the reference's Lambda(relu(x, max_value=6.)), deeplabv3p.py:181) or 'softmax'."""
    kind = "Activation"
    prefix = "activation"

    def __init__(self, fn, name=None):
        super().__init__(name=name)
        assert fn in ("relu", "relu6", "softmax")
        self.cfg["fn"] = fn


class ReLU6(Activation):
    """Lambda(lambda x: relu(x, max_value=6.)) — a Lambda layer in the reference, hence lambda_N auto-names."""
    prefix = "lambda"

    def __init__(self, name=None):
        super().__init__("relu6", name=name)


class Prescale(Layer):
    """Lambda(lambda x: x/127.5 - 1) (deeplabv3p.py:270)"""
    kind = "Prescale"
    prefix = "lambda"


class ResizeBilinear(Layer):
    """Lambda(K.tf.image.resize_bilinear(x, size)) (deeplabv3p.py:382,:418,:439; utils.py:190)"""
    kind = "ResizeBilinear"
    prefix = "lambda"

    def __init__(self, size, name=None):
        super().__init__(name=name)
        self.cfg["size"] = (int(size[0]), int(size[1]))

    def compute_output_shape(self, in_shapes):
        return self.cfg["size"] + (in_shapes[0][2],)


class Add(Layer):
    kind = "Add"
    prefix = "add"

    def compute_output_shape(self, in_shapes):
        assert in_shapes[0] == in_shapes[1], in_shapes
        return in_shapes[0]


class Concatenate(Layer):
    kind = "Concatenate"
    prefix = "concatenate"

    def compute_output_shape(self, in_shapes):
        assert all(s[:2] == in_shapes[0][:2] for s in in_shapes), in_shapes
        return in_shapes[0][:2] + (sum(s[2] for s in in_shapes),)


class AveragePooling2D(Layer):
    kind = "AveragePooling2D"
    prefix = "average_pooling2d"

    def __init__(self, pool_size, name=None):
        super().__init__(name=name)
        self.cfg["pool"] = (int(pool_size[0]), int(pool_size[1]))

    def compute_output_shape(self, in_shapes):
        H, W, C = in_shapes[0]
        ph, pw = self.cfg["pool"]
        if (H // ph, W // pw) != (1, 1):
            raise NotImplementedError("only the global pooling of deeplabv3p.py:375 is on the path")
        return (1, 1, C)


class ZeroPadding2D(Layer):
    kind = "ZeroPadding2D"
    prefix = "zero_padding2d"

    def __init__(self, padding, name=None):
        super().__init__(name=name)
        # Keras reads a 2-tuple of ints as symmetric (height, width) padding (deeplabv3p.py:68,:110)
        ph, pw = padding
        self.cfg["pad"] = ((int(ph), int(ph)), (int(pw), int(pw)))

    def compute_output_shape(self, in_shapes):
        H, W, C = in_shapes[0]
        (pt, pb), (pl, pr) = self.cfg["pad"]
        return (H + pt + pb, W + pl + pr, C)


class Dropout(Layer):
    kind = "Dropout"
    prefix = "dropout"

    def __init__(self, rate, name=None):
        super().__init__(name=name)
        self.cfg["rate"] = float(rate)


class Reshape(Layer):
    kind = "Reshape"
    prefix = "reshape"

    def __init__(self, target_shape, name=None):
        super().__init__(name=name)
        self.cfg["target"] = tuple(target_shape)

    def compute_output_shape(self, in_shapes):
        n = int(np.prod(in_shapes[0]))
        tgt = list(self.cfg["target"])
        if -1 in tgt:
            known = int(np.prod([t for t in tgt if t != -1]))
            tgt[tgt.index(-1)] = n // known
        assert int(np.prod(tgt)) == n, (tgt, in_shapes)
        return tuple(tgt)


# --------------------------------------------------------------------------------------


class Model:
    """keras.models.Model(inputs, outputs, name): the sub-graph between `inputs` and `outputs`."""

    def __init__(self, inputs, outputs, name=None):
        self.name = name or _auto_name("model")
        self.input = inputs
        self.output = outputs
        self._collect()
        self._engines = {}
        self._compiled = None
        self._dp = None          # parallel.DataParallel once distribute() was called
        self._dp_synced = False
        self._train_eng = None   # the engine that holds the live Adam moments / iteration / dropout step
        # callable(input_shape) -> the same graph for another input size, fresh weights: recorded by Deeplabv3() and
        # SegModel.create_seg_model for predict_multiscale's sibling models (tta.py)
        self._tta_rebuild = None

    # -- graph -----------------------------------------------------------------------
    def _collect(self):
        """Keras 2.2.4 Network._init_graph_network ordering: DFS from the output
        assigns visit indices (pre-order, inputs in call order), depth = longest path to the
        output, layers sorted by decreasing depth then increasing visit index."""
        out_layer = self.output.layer
        in_layer = self.input.layer
        index, depth = {}, {}
        finished = set()

        def visit(start):
            # iterative form of Keras' recursive build_map: a layer gets its index when it is first
            # ENTERED (pre-order); inbound layers are entered in call order; finished layers are skipped
            stack = [(start, 0)]
            while stack:
                lyr, i = stack.pop()
                if i == 0:
                    if lyr in finished:
                        continue
                    if lyr not in index:
                        index[lyr] = len(index)
                ins = [] if lyr is in_layer else lyr.inbound
                if i < len(ins):
                    stack.append((lyr, i + 1))
                    stack.append((ins[i].layer, 0))
                else:
                    finished.add(lyr)

        visit(out_layer)
        if in_layer not in index:
            raise ValueError("graph disconnected: the input is not an ancestor of the output")
        # topological (creation) order: every layer's inputs precede it
        topo = []
        seen = set()

        def topo_visit(layer):
            stack = [(layer, 0)]
            while stack:
                lyr, i = stack.pop()
                if lyr in seen:
                    continue
                ins = lyr.inbound if lyr is not in_layer else []
                if i < len(ins):
                    stack.append((lyr, i + 1))
                    if ins[i].layer not in seen:
                        stack.append((ins[i].layer, 0))
                else:
                    seen.add(lyr)
                    topo.append(lyr)

        topo_visit(out_layer)
        self._topo = topo
        # depth = longest path to the output, relaxed in reverse topological order
        for lyr in topo:
            depth[lyr] = 0
        for lyr in reversed(topo):
            ins = lyr.inbound if lyr is not in_layer else []
            for t in ins:
                depth[t.layer] = max(depth[t.layer], depth[lyr] + 1)
        self.layers = sorted(topo, key=lambda l: (-depth[l], index[l]))
        self._by_name = {l.name: l for l in self.layers}

    def get_layer(self, name=None, index=None):
        if index is not None:
            return self.layers[index]
        return self._by_name[name]

    @property
    def weights(self):
        return [n for l in self.layers for n in l.weights]

    def count_params(self):
        return sum(l.count_params() for l in self.layers)

    def trainable_count(self):
        n = 0
        for l in self.layers:
            if not l.trainable:
                continue
            for k, w in l.weights.items():
                if "/moving_" not in k:
                    n += w.size
        return int(n)

    def summary(self, print_fn=print):
        print_fn('Model: "%s"' % self.name)
        for l in self.layers:
            print_fn("%-48s %-22s %-18s %9d" % (l.name, l.kind, l.output.shape, l.count_params()))
        print_fn("Total params: %d   Trainable params: %d" % (self.count_params(), self.trainable_count()))

    # -- weights -----------------------------------------------------------------------
    def get_weights(self):
        return [w for l in self.layers for w in l.get_weights()]

    def set_weights(self, ws):
        i = 0
        for l in self.layers:
            n = len(l.weights)
            if n:
                l.set_weights(ws[i:i + n])
                i += n

    def save_weights(self, path):
        from . import h5io
        h5io.save_weights(self, path)

    def load_weights(self, path, by_name=False):
        from . import h5io
        h5io.load_weights(self, path, by_name=by_name)

    # -- execution (delegated to the HIP engine) ----------------------------------------
    def compile(self, optimizer=None, loss=None, metrics=None, sample_weight_mode=None, **kw):
        """keras Model.compile as used by the notebook (cell 2): remembers the optimizer
        hyper-parameters; the loss on the path is always sparse_crossentropy_ignoring_last_label
        with temporal sample weights (utils.py:127-130)."""
        from .optimizers import compile_optimizer
        # optimizer: None (the notebook's Adam(lr=7e-4, epsilon=1e-8, decay=1e-6)), a dict of overrides, 'adam', an
        # optimizers.Adam / any Keras-style Adam exposing get_config(), or an optimizers.SGD / RMSprop (instances of this
        # package's classes only); anything else raises here, not at the first step.  The rule and the clip settings sit
        # beside the hyper-parameter dict, which for Adam stays the five-key dict it always was
        rule, hyper, clipnorm, clipvalue = compile_optimizer(optimizer)
        self._refuse_jaccard_dp(loss, self._dp)
        # the regularisers in force: {weight name: l} for l > 0.  regularizers.collect raises for anything
        # that is neither None nor this package's l2 — here, before anything of the model changes.  One set after this
        # call takes effect at the next compile()
        l2 = regularizers.collect(self.layers)
        self._compiled = dict(optimizer=hyper, optimizer_object=optimizer, loss=loss, metrics=metrics,
                              sample_weight_mode=sample_weight_mode, rule=rule, clipnorm=clipnorm, clipvalue=clipvalue, l2=l2)
        # Keras 2.2.4 collects the weights the optimizer updates HERE (`_collected_trainable_weights`), and the layers'
        # update ops (BatchNormalization moving statistics) when the train function is first built — the first
        # train_on_batch / fit after compile().  `layer.trainable` flipped in between (segmentation.ipynb: compile in
        # cell 2, the fine-tuning loop in cell 5, no recompile) therefore changes which moving statistics move but NOT
        # which weights train: Keras warns about the discrepancy and trains them all.  Same here.
        self._compile_gen = getattr(self, "_compile_gen", 0) + 1
        self._collected_trainable = {l.name: bool(l.trainable) for l in self.layers}
        self._update_flags = None   # frozen at the first training step after this compile()
        # a new train function starts from fresh optimizer slots (Keras re-creates m / v in get_updates) — but
        # `optimizer.iterations` is a variable of the OPTIMIZER OBJECT: compiling again with the same Adam instance (the
        # notebook's fine-tuning recompile) keeps counting, so the lr decay and the bias-correction exponent continue
        # (ADVICE r5).  A new object, a dict or a string starts at 0.
        prev, prev_obj = self._train_eng, getattr(self, "_opt_object", None)
        keep = prev is not None and optimizer is not None and optimizer is prev_obj and not isinstance(optimizer, (dict, str))
        self._carry_iterations = (int(prev.iteration), prev.drop_step.clone()) if keep else None
        # ... and so does the mining ramp (its device step counter, or the iteration count of an engine that did not mine)
        self._carry_mine_step = (prev.mine_step.clone() if prev.mining else int(prev.iteration)) if keep else None
        self._opt_object = optimizer
        self._train_eng = None

    def distribute(self, dp=None, strict=True):
        """Per-image data parallelism for train_on_batch / fit: this process is one of WORLD_SIZE (one per GPU, launched
        by torch.distributed.run); every call hands over the GLOBAL batch (or, with global_batch=False, this rank's own
        shard), each rank trains on its contiguous shard and the gradients are summed with one RCCL all-reduce
        (parallel.DataParallel).  Stands in for keras.utils.multi_gpu_model (utils.py:209-211), whose towers likewise keep
        per-replica BatchNorm statistics.
        strict (default): an RCCL communicator that cannot be brought up RAISES — a silent fall-back to gloo stages every
        gradient exchange through host memory (10-100x slower); strict=False, or DL3_DIST_BACKEND=gloo asked for explicitly,
        keeps the warning-and-gloo behaviour the functional tests use."""
        from .parallel import DataParallel
        self._refuse_jaccard_dp((getattr(self, "_compiled", None) or {}).get("loss"), True)
        self._dp = dp if dp is not None else DataParallel(strict=strict)
        self._dp_synced = False
        return self

    MAX_ENGINES = int(os.environ.get("DL3_MAX_ENGINES", "4"))

    def _training_flags(self):
        """({layer: does the optimizer update its weights}, {layer: do its update ops run}, cache key) for a training engine.
        Compiled model: the Keras 2.2.4 rule (see compile()).  Never compiled: the live flags, and the key carries them, so a
        plan lowered for one set of flags is never replayed for another."""
        live = {l.name: bool(l.trainable) for l in self.layers}
        if getattr(self, "_collected_trainable", None) is None:
            return live, live, ("live", tuple(sorted(n for n, t in live.items() if not t)))
        if self._update_flags is None:
            self._update_flags = live
            if live != self._collected_trainable:
                import warnings
                warnings.warn("dl3: discrepancy between trainable weights and collected trainable weights — "
                              "`layer.trainable` changed after compile(): as in Keras 2.2.4 the optimizer still updates the "
                              "weights collected at compile(); only the moving statistics of now-frozen BatchNormalization "
                              "layers stop moving.  Call compile() again after setting `trainable` to train the tail only.",
                              UserWarning, stacklevel=4)
        return self._collected_trainable, self._update_flags, ("compiled", self._compile_gen)

    def _mining(self):
        """(p, S) of a compile(loss=utils.sparse_crossentropy_top_k(...)) that mines, else None (any other loss, p == 1)"""
        loss = (getattr(self, "_compiled", None) or {}).get("loss")
        return getattr(loss, "mining", None)

    @staticmethod
    def _refuse_jaccard_dp(loss, dp):
        """compile(loss=utils.sparse_crossentropy_jaccard(...)) and distribute() exclude each other, in either order
        (DESIGN.md §16): host-only, raised before any device call"""
        if dp is not None and getattr(loss, "jaccard", None) is not None:
            raise ValueError("the soft-Jaccard loss does not train under distribute(): a data-parallel engine finishes ONE "
                             "gradient scale in the optimizer from the all-reduced count(w != 0), and the Jaccard term has a "
                             "normaliser of its own; train on one GPU or compile the cross-entropy")

    def _jaccard(self):
        """lambda of a compile(loss=utils.sparse_crossentropy_jaccard(...)) whose term is on, else None (any other loss,
        jaccard_weight == 0)"""
        loss = (getattr(self, "_compiled", None) or {}).get("loss")
        return getattr(loss, "jaccard", None)

    def _focal(self):
        """(gamma, alpha) of a compile(loss=utils.sparse_focal_crossentropy(...)) whose loss is on, else None (any other
        loss; gamma == 0 with alpha None or all ones)"""
        loss = (getattr(self, "_compiled", None) or {}).get("loss")
        return getattr(loss, "focal", None)

    def _engine_key(self, batch, training, kw):
        """(cache key, constructor keywords) of the engine for (batch, mode, keywords): host-only.  A training engine's
        key carries the trainable flags and, through the keywords, the mining settings, the Jaccard weight or the focal
        (gamma, alpha) of the compiled loss — a plan lowered for one setting is never replayed for another; a loss that
        neither mines nor adds the Jaccard term nor modulates adds nothing to either.  The focal loss with mining or with
        the Jaccard term (they are separate loss objects; keywords could still ask for both) raises ValueError.  The L2
        table of compile() rides as the training keyword `l2`, absent where it is empty."""
        kw = dict(kw)
        if training and "mining" not in kw and self._mining() is not None:
            kw["mining"] = self._mining()
        if training and "jaccard" not in kw and self._jaccard() is not None:
            kw["jaccard"] = self._jaccard()
        if training and "focal" not in kw and self._focal() is not None:
            kw["focal"] = self._focal()
        if "focal" in kw:   # the normal form: hashable, and absent where the loss is off (the plain key)
            kw["focal"] = check_focal(kw["focal"]) if training else None
            if kw["focal"] is None:
                del kw["focal"]
        # the L2 table collected at compile(), in its normal form: absent where nothing is regularised (the plain key)
        if training and "l2" not in kw:
            kw["l2"] = (getattr(self, "_compiled", None) or {}).get("l2")
        if "l2" in kw:
            kw["l2"] = regularizers.normal_form(kw["l2"]) if training else None
            if kw["l2"] is None:
                del kw["l2"]
        if training and kw.get("focal") is not None and (
                check_mining(kw.get("mining")) is not None or check_jaccard(kw.get("jaccard")) is not None):
            raise ValueError("the focal loss, hard-example mining and the soft-Jaccard loss are separate losses and cannot "
                             "be combined")
        key = (int(batch), bool(training), tuple(sorted(kw.items())))
        if training:
            flags = self._training_flags()
            kw = dict(kw, opt_trainable=flags[0], bn_update=flags[1])
            key = key + (flags[2],)
        return key, kw

    def _engine(self, batch, training, **kw):
        """engine for (batch, mode); weights travel through the host master copies when the active engine changes, the
        optimizer state (Adam moments, iteration, dropout step) moves device-to-device between training engines, and
        the least recently used engines beyond MAX_ENGINES are dropped (each one owns a full activation arena)."""
        from .engine import Engine
        key, kw = self._engine_key(batch, training, kw)
        eng = self._engines.pop(key, None)
        active = getattr(self, "_active", None)
        if eng is not active and active is not None:
            active.sync_all_to_host()
        if eng is None:
            eng = Engine(self, batch=int(batch), training=training, **kw)
        elif eng is not active:
            eng.sync_all_to_device()
        self._engines[key] = eng  # most recently used last
        if training:
            prev = self._train_eng
            if prev is not None and prev is not eng:
                eng.adopt_optimizer_state(prev)  # e.g. the last, smaller batch of an epoch keeps the same Adam
            elif prev is None and getattr(self, "_carry_iterations", None) is not None:
                # first train function after a compile() that re-used the optimizer object: fresh moments, same clock
                it, drop = self._carry_iterations
                eng.iteration = it
                eng.adam_m.zero_()
                eng.adam_v.zero_()
                eng.drop_step.copy_(drop)
                if isinstance(self._carry_mine_step, int):
                    eng.mine_step.fill_(self._carry_mine_step)
                else:
                    eng.mine_step.copy_(self._carry_mine_step)
                self._carry_iterations = self._carry_mine_step = None
            self._train_eng = eng
        while len(self._engines) > self.MAX_ENGINES:
            k0 = next(iter(self._engines))
            old = self._engines[k0]
            if old is eng or old is self._train_eng:
                self._engines[k0] = self._engines.pop(k0)  # keep; move to the young end
                if all(e is eng or e is self._train_eng for e in self._engines.values()):
                    break
                continue
            del self._engines[k0]
        self._active = eng
        eng.activate()
        return eng

    def predict(self, x, batch_size=32, verbose=0):
        x = raw_pixels(x)
        outs = []
        for s in batches(x.shape[0], batch_size):
            xb = x[s]
            outs.append(self._engine(xb.shape[0], False).predict(xb))
        return np.concatenate(outs, axis=0)

    def predict_mask(self, x, batch_size=32, crf=False, crf_unary="labels"):
        """np.argmax(model.predict(x), -1) (notebook cell 9) without shipping the probabilities to the host: the argmax
        runs on the device (dl3_argmax) and only the int32 masks [B,H,W] cross PCIe — 1 MB instead of 22 MB per
        512x512x21 image.  Not part of the reference's Model API.

        crf=True: the notebook's `do_crf(image, mask)` step on the device as well — every batch's masks go through
        crf.dense_crf with `x` as the image (zero_unsure=True, the reference's default) before they are copied out.

        crf_unary (only looked at with crf=True): "labels" is that path — the unary term rebuilt from the arg-max mask
        with gt_prob; "softmax" hands the CRF the network's own class probabilities (unary_from_softmax, one label per
        class): forward pass, Engine.crf_unary and dl3_crf_inference follow each other on the device and only the int32
        masks are copied out."""
        if crf and crf_unary not in ("labels", "softmax"):
            raise ValueError("predict_mask: crf_unary must be 'labels' or 'softmax', got %r" % (crf_unary,))
        x = raw_pixels(x)
        outs = []
        for s in batches(x.shape[0], batch_size):
            xb = x[s]
            eng = self._engine(xb.shape[0], False)
            eng.set_input(xb)
            if crf and crf_unary == "softmax":
                outs.append(eng.crf_mask(xb).to("cpu").numpy())
                continue
            eng.forward()
            if crf:
                from .crf import dense_crf
                outs.append(dense_crf(xb, eng.argmax(host=False)).to("cpu").numpy().astype(np.int32))
            else:
                outs.append(eng.argmax())
        return np.concatenate(outs, axis=0)

    def predict_multiscale(self, x, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True, batch_size=8, output="probs",
                           crf=False, factory=None):
        """DeepLab's evaluation protocol [deeplab-semantics]: the class probabilities averaged over input
        scales and left-right flips, every step on the device (tta.py).  A pass at scale s runs this graph built for the
        input size tta.scaled_size(H, s) x tta.scaled_size(W, s) — a sibling model, built once and kept (clear_multiscale
        drops them) — on this model's CURRENT weights and moving statistics; the passes run in the order of `scales`, the
        mirrored one behind the plain one.  Not part of the reference's Model API.

        output="probs": numpy float32 in the shape predict() returns; output="mask": int32 [B,H,W], the first-maximum
        argmax of the average (dl3_argmax) — only the masks cross PCIe.  crf=True (with "mask" only): the averaged
        probabilities, still on the device, go through crf.dense_crf_softmax with `x` as the image.
        x: raw 0-255 pixels [B,H,W,3], float32 or uint8, host array or device tensor, as predict() takes them.
        factory: callable(input_shape) -> Model, needed for a Model that neither Deeplabv3() nor
        SegModel.create_seg_model built; without it such a model raises ValueError before any device work."""
        from . import tta
        return tta.predict_multiscale(self, x, scales=scales, flip=flip, batch_size=batch_size, output=output, crf=crf,
                                      factory=factory)

    def clear_multiscale(self):
        """drop predict_multiscale's sibling models and their engines (each owns an activation arena)"""
        from . import tta
        tta.clear_multiscale(self)

    def predict_sliding(self, x, stride=None, blend="uniform", batch_size=8, output="mask", pad_value=127.5):
        """Sliding-window inference: masks or probabilities for images of ANY size at their own resolution.
        Every image is cut into overlapping windows of the model's input size (H, W) — the last window of an axis is
        shifted back to end on the image's edge, an image smaller than the window is padded with `pad_value` (127.5, the
        pixel the pre-scale maps to 0) — the network runs on the windows, their class probabilities are averaged where
        they overlap and the arg-max is taken per image pixel, every step on the device (slide.py).  Not part of the
        reference's Model API.

        x: raw 0-255 pixels, uint8 or float32, host array or device tensor [B,Hi,Wi,3], or a list / tuple of [Hi,Wi,3]
        images of different sizes.  stride: an integer or (sh, sw), 1 <= stride <= window; default two thirds of the
        window.  blend: "uniform" (the plain mean) or "pyramid" (weights min(r+1, H-r) * min(c+1, W-c), which
        down-weight a window's border).  batch_size: windows per forward pass; the windows of all images form one list
        (image-major), so chunks span images.  output="mask": int32 [Hi,Wi], the first-maximum arg-max of the averaged
        probabilities — only the masks cross PCIe; output="probs": float32 [Hi,Wi,C].  Stacked into one array for array
        input, a list for list input.  Bad arguments raise ValueError before any device work.

        Out of scope: combining with predict_multiscale, crf=, training, reading image files."""
        from . import slide
        return slide.predict_sliding(self, x, stride=stride, blend=blend, batch_size=batch_size, output=output,
                                     pad_value=pad_value)

    def evaluate(self, x, y, batch_size=32, sample_weight=None, verbose=0, device=False):
        """keras Model.evaluate for the notebook's metrics (cell 2: metrics=[Jaccard, sparse_accuracy_ignoring_last_label]):
        returns [loss, Jaccard, accuracy].  The argmax mask and the per-image/per-class pixel counts are produced on
        the device (dl3_argmax, dl3_seg_counts); the metric ratios (utils.py:132-157) and the loss (utils.py:127-130,
        Keras weighted mean) are evaluated on the host from those counts / the probabilities.
        device=True: the evaluation plan (Engine.evaluate_batch) — nothing but a small result buffer
        crosses PCIe, once per call — with Keras 2.2.4's averaging [TF-semantics, from memory]: every number is formed per
        BATCH and the call returns the average over batches weighted by batch size.  (The host path pools the counts of
        all batches before it forms the metric ratios; it stays as it is.)"""
        if device:
            return self._with_l2(self._evaluate_device(self._xy_batches(x, y, sample_weight, batch_size))[0])
        from . import utils as U
        x, y = raw_pixels(x), np.asarray(y)
        counts, num, den = [], 0.0, 0.0
        for s in batches(x.shape[0], batch_size):
            xb, yb = x[s], y[s]
            eng = self._engine(xb.shape[0], False)
            probs = eng.predict(xb)
            counts.append(eng.seg_counts(yb))
            C = probs.shape[-1]
            probs = probs.reshape(xb.shape[0], -1, C)
            yb = yb.reshape(xb.shape[0], -1, 1)
            # no sample weights: Keras takes the plain mean over all B*HW pixels (void rows contribute 0 through the
            # one-hot, utils.py:129); with weights: sum(l*w) / count(w != 0)
            w = np.ones(yb.shape[:2], np.float64) if sample_weight is None else \
                np.asarray(sample_weight[s], np.float64).reshape(xb.shape[0], -1)
            ell = U.sparse_crossentropy_ignoring_last_label(yb, probs)
            num += float((ell * w).sum() / max((w != 0).mean(), 1e-30) / w.size) * xb.shape[0]
            den += xb.shape[0]
        counts = np.concatenate(counts, 0)
        return [num / den + self._l2_addend(), U.Jaccard_from_counts(counts), U.accuracy_from_counts(counts)]

    # -- evaluation on the device ------------------------------------------------------------------
    @staticmethod
    def _xy_batches(x, y, sample_weight, batch_size):
        x = raw_pixels(x)
        for s in batches(x.shape[0], batch_size):
            yield x[s], y[s], (None if sample_weight is None else sample_weight[s])

    @staticmethod
    def _generator_batches(generator, steps=None):
        """(X, Y, SW) of a generator's items: (X, Y), (X, Y, SW) or (X, Y, {'pred_mask': SW})"""
        steps = len(generator) if steps is None else int(steps)
        for i in range(steps):
            item = generator[i] if hasattr(generator, "__getitem__") else next(generator)
            SW = item[2] if len(item) > 2 else None
            if isinstance(SW, dict):
                SW = list(SW.values())[0]
            yield item[0], item[1], SW

    def _evaluate_device(self, batches, confusion=None, after_batch=None):
        """one evaluation pass: every batch through Engine.evaluate_batch, the results of the whole pass read once per
        engine (a ragged last batch has an engine of its own).  -> ([loss, Jaccard, accuracy] averaged over the batches
        weighted by batch size, the per-batch triples, the batch sizes).  after_batch: callable(engine, masks) that
        enqueues further device work on the batch's labels (engine.labels) and int32 masks [B,H,W], which stay valid
        until the engine's next batch; the pass then runs the tail with mask=True."""
        from . import utils as U
        used, fresh = [], set()
        for xb, yb, swb in batches:
            eng = self._engine(xb.shape[0], False)
            if id(eng) not in fresh:
                fresh.add(id(eng))
                eng.discard_evaluation()
            if after_batch is None:
                eng.evaluate_batch(xb, yb, swb, confusion=confusion)
            else:
                after_batch(eng, eng.evaluate_batch(xb, yb, swb, confusion=confusion, mask=True))
            used.append(eng)
        if not used:
            raise ValueError("evaluation over zero batches")
        read, per, sizes = {}, [], []
        for eng in used:
            if id(eng) not in read:
                read[id(eng)] = [eng.read_evaluation(), 0]
            (loss, nnz, counts), k = read[id(eng)]
            read[id(eng)][1] += 1
            n = int(nnz[k].sum())
            # sum(l*w) / count(w != 0) of the batch; no weight non-zero: every term is zero (no division)
            per.append([float(loss[k].sum() / n) if n else 0.0, U.Jaccard_from_counts(counts[k]),
                        U.accuracy_from_counts(counts[k])])
            sizes.append(eng.B)
        a, w = np.asarray(per, np.float64), np.asarray(sizes, np.float64)
        return [float(v) for v in (a * w[:, None]).sum(0) / w.sum()], per, sizes

    def _l2_addend(self):
        """the penalty of the compiled regularisers at the current weights: the weights do not move during
        an evaluation pass, so it is added ONCE per call, behind the batch-size-weighted average — value-only launches
        over both arenas of the engine the pass ran on, one double read.  Nothing regularised: 0.0 and no launch."""
        table = regularizers.normal_form((getattr(self, "_compiled", None) or {}).get("l2"))
        return self._active.l2_value(table) if table else 0.0

    def _with_l2(self, vals):
        """[loss, Jaccard, accuracy] of an evaluation pass with the penalty on the loss; the metrics are untouched"""
        return [vals[0] + self._l2_addend()] + list(vals[1:])

    def evaluate_generator(self, generator, steps=None, **kw):
        """keras Model.evaluate_generator on the device: [loss, Jaccard, sparse_accuracy_ignoring_last_label], per-batch
        values averaged with the batch sizes as weights (Keras 2.2.4 [TF-semantics, from memory])"""
        self._check_fit_kw(kw)
        return self._with_l2(self._evaluate_device(self._generator_batches(generator, steps))[0])

    def confusion_matrix(self, x_or_generator, y=None, batch_size=32):
        """int64 [C,C], row = label, column = prediction, void labels skipped — the notebook's calculate_iou loop (cell 10)
        as one device pass: the matrix accumulates on the device across batches and crosses PCIe once"""
        import torch
        C = int(self.output.shape[-1])
        buf = getattr(self, "_confusion_buf", None)
        if buf is None or buf.shape[0] != C:
            buf = self._confusion_buf = torch.zeros(C, C, dtype=torch.int64, device="cuda")
        buf.zero_()
        batches = self._generator_batches(x_or_generator) if y is None else self._xy_batches(x_or_generator, y, None, batch_size)
        self._evaluate_device(batches, confusion=buf)
        return buf.cpu().numpy()

    def confusion_matrix_trimap(self, x_or_generator, y=None, batch_size=32, widths=(1, 2, 4, 8, 16, 32), metric="chebyshev",
                                seeds=("void", "edges")):
        """Confusion matrices restricted to bands around the object boundaries (the trimap experiment of the DeepLabV3+
        paper): int64 [K+1,C,C], CUMULATIVE — slice k is confusion_matrix() over the pixels within
        widths[k] of a boundary seed (trimap.py: a void pixel and / or a pixel with a 4-neighbour of another label;
        metric "chebyshev" or "euclidean"), the last slice over every pixel, equal to confusion_matrix() bit for bit.
        One evaluation pass: behind every batch's tail, dl3_trimap_rings and dl3_trimap_confusion run on the engine's own
        label and mask buffers; the bins accumulate on the device and cross PCIe once.  Bad arguments raise ValueError
        before any device work.  Not part of the reference's Model API."""
        from . import trimap
        ws, m, s = trimap.check_widths(widths), trimap.check_metric(metric), trimap.check_seeds(seeds)
        C = trimap.check_classes(int(self.output.shape[-1]))
        import torch
        band = torch.zeros(len(ws) + 1, C, C, dtype=torch.int64, device="cuda")

        def after_batch(eng, masks):
            trimap.accumulate(masks.reshape(-1), eng.labels, tuple(masks.shape), C, ws, m, s, band)
        batches = self._generator_batches(x_or_generator) if y is None else self._xy_batches(x_or_generator, y, None, batch_size)
        self._evaluate_device(batches, after_batch=after_batch)
        return trimap.cumulative(band).cpu().numpy()

    _KNOWN_METRICS = ("Jaccard", "sparse_accuracy_ignoring_last_label")

    def _metric_names(self):
        """names of compile(metrics=...) — a list or {'pred_mask': [...]} of the two metrics this package knows"""
        m = (self._compiled or {}).get("metrics") or []
        if isinstance(m, dict):
            m = [f for v in m.values() for f in (v if isinstance(v, (list, tuple)) else [v])]
        names = []
        for f in m:
            name = f if isinstance(f, str) else getattr(f, "__name__", None)
            if name not in self._KNOWN_METRICS:
                raise ValueError("validation: metric %r is not one of %s (the metrics the evaluation tail produces)"
                                 % (f, list(self._KNOWN_METRICS)))
            names.append(name)
        return names

    def _validator(self, validation_data, validation_steps, batch_size):
        """() -> {'val_loss': .., 'val_<metric>': ..} for fit / fit_generator.  Under distribute() every rank evaluates
        the whole validation set on its own replica: identical weights give identical logs and identical callback
        decisions without a collective."""
        if validation_data is None:
            return None

        def validate():
            names = self._metric_names()
            if isinstance(validation_data, (tuple, list)):
                sw = validation_data[2] if len(validation_data) > 2 else None
                batches = self._xy_batches(validation_data[0], validation_data[1], sw, batch_size)
            else:
                batches = self._generator_batches(validation_data, validation_steps)
            vals = self._with_l2(self._evaluate_device(batches)[0])
            logs = {"val_loss": vals[0]}
            for name in names:
                logs["val_" + name] = vals[1 + self._KNOWN_METRICS.index(name)]
            return logs
        return validate

    def _opt_desc(self):
        """the compiled optimizer as Engine.opt_step takes it; `hyper` IS the compiled dict, so _set_lr shows at the next
        step.  Nothing compiled: the notebook's Adam."""
        c = self._compiled
        if c is None:
            return dict(rule="adam", hyper={})
        return dict(rule=c.get("rule", "adam"), hyper=c["optimizer"], clipnorm=c.get("clipnorm"), clipvalue=c.get("clipvalue"))

    def _get_lr(self):
        from .engine import Engine
        c = self._compiled or {}
        # (a rule's default where the compiled dict names no lr; Adam's: the notebook's Adam(lr=7e-4))
        return float((c.get("optimizer") or {}).get("lr", Engine._RULES[c.get("rule", "adam")][1]["lr"]))

    def _set_lr(self, lr):
        """a new learning rate from the next step on, whatever the rule: the compiled hyper-parameter dict
        (Engine.opt_step takes it per call — no new engine, the slots and the iteration untouched) and the optimizer
        object's `lr` if there is one"""
        if self._compiled is None:
            self._compiled = dict(optimizer={}, optimizer_object=None, loss=None, metrics=None, sample_weight_mode=None)
        self._compiled["optimizer"]["lr"] = float(lr)
        obj = self._compiled.get("optimizer_object")
        if obj is not None and not isinstance(obj, (dict, str)) and hasattr(obj, "lr"):
            obj.lr = float(lr)

    def _fit_session(self, kw, epochs, steps, batch_size):
        """takes callbacks= / validation_data= / validation_steps= out of kw; None when neither callbacks nor validation
        were asked for (fit then returns its plain list of losses, as before)"""
        callbacks = kw.pop("callbacks", None)
        validation_data = kw.pop("validation_data", None)
        validation_steps = kw.pop("validation_steps", None)
        if not callbacks and validation_data is None:
            return None
        return _FitSession(self, callbacks, self._validator(validation_data, validation_steps, batch_size), epochs, steps)

    def _dp_active(self):
        dp = self._dp
        return dp is not None and (dp.world > 1 or dp.comm is not None)

    def _dp_sync_weights(self, eng):
        """identical weights and moving statistics on every rank before the first data-parallel step"""
        if not self._dp_synced:
            self._dp.broadcast(eng.params)
            self._dp.broadcast(eng.state)
            eng.dirty = True
            self._dp_synced = True

    def train_on_batch(self, x, y, sample_weight=None, lazy_loss=False, global_batch=True, **engine_kw):
        """keras Model.train_on_batch; lazy_loss=True returns an engine.LazyLoss (float() reads it) instead of stalling
        the stream for one scalar every step — fit / fit_generator use it and read once per epoch.
        Under distribute(): global_batch=True (Keras' multi_gpu_model contract, utils.py:209-211) — every rank is handed
        the whole batch and keeps its contiguous shard; global_batch=False — (x, y, sample_weight) ARE this rank's shard
        (a generator sharded by rank: nothing redundant is built or copied on the host)."""
        dp = self._dp
        # the data-parallel step also runs for a communicator of ONE rank (dp.comm set): every launch of the N-rank step —
        # the hipGraph replay, the ONE all-reduce of the arena (gradients + the shard's count and loss sum) behind it, Adam
        # finishing the scale on the device — on one GPU
        multi = dp is not None and (dp.world > 1 or dp.comm is not None)
        if multi:
            n = x.shape[0]
            if global_batch and n < dp.world:
                raise ValueError("global batch of %d images cannot be split over %d ranks" % (n, dp.world))
            # a ragged batch (the last one of a Sequence) gives its remainder to the last rank, like the reference's
            # multi_gpu_model towers; the loss is normalised by the GLOBAL count(w != 0) (Engine.train_step)
            if global_batch:
                lo, hi = dp.shard(n)
                x, y = x[lo:hi], y[lo:hi]
                if sample_weight is not None:
                    sample_weight = sample_weight[lo:hi]
            engine_kw = dict(engine_kw, external_nnz=True)
        eng = self._engine(x.shape[0], True, **engine_kw)
        opt = self._opt_desc()
        if not multi:
            return eng.train_step(x, y, sample_weight, opt, lazy=lazy_loss)
        self._dp_sync_weights(eng)
        # sum_all(l*w) / count_all(w != 0), from the arena tail the one all-reduce summed: the same number on every rank
        return eng.train_step(x, y, sample_weight, opt, comm=dp, lazy=lazy_loss)

    _IGNORED_FIT_KW = ("workers", "use_multiprocessing", "max_queue_size", "shuffle", "initial_epoch")

    def _check_fit_kw(self, kw):
        import warnings
        for k, v in kw.items():
            if k in self._IGNORED_FIT_KW or v is None or (isinstance(v, (list, tuple)) and not v):
                continue
            warnings.warn("dl3: Model.fit/fit_generator does not implement %r: it is IGNORED" % k,
                          RuntimeWarning, stacklevel=3)

    def fit(self, x, y, batch_size=16, epochs=1, sample_weight=None, verbose=0, **kw):
        """Minimal Model.fit (utils.py:244): plain epochs over (x, y) without shuffling.
        validation_data=(x, y[, sw]) and / or callbacks=[...] (callbacks.py): after every epoch the validation set goes
        through the evaluation plan on the device and the callbacks see {'loss', 'val_loss', 'val_<metric>'...}; the call
        then returns a callbacks.History instead of the list of losses."""
        n = x.shape[0]
        ses = self._fit_session(kw, epochs, max(n // batch_size, 0), batch_size)
        self._check_fit_kw(kw)
        hist = []
        for ep in range(epochs):
            if ses:
                ses.epoch_begin(ep)
            for b, i in enumerate(range(0, n - batch_size + 1, batch_size)):
                sw = None if sample_weight is None else sample_weight[i:i + batch_size]
                hist.append(self.train_on_batch(x[i:i + batch_size], y[i:i + batch_size], sw, lazy_loss=True))
                if ses:
                    ses.batch_end(b, batch_size, hist[-1])
            if ses and ses.epoch_end(ep):
                break
        return ses.end() if ses else [float(l) for l in hist]

    def fit_generator(self, generator, steps_per_epoch=None, epochs=1, verbose=0, device_feed=False, n_classes=None,
                      global_batch=True, **kw):
        """Minimal Model.fit_generator (utils.py:233): generator yields (X, Y, {'pred_mask': SW}) or (X, Y, SW).
        device_feed=True (not in Keras): the generator yields (uint8 images [B,H,W,3], raw label maps [B,H,W] uint8 / int32)
        — what cv2 decodes, before SegmentationGenerator.__getitem__ turns it into float tensors (utils.py:375-402): the
        batch crosses PCIe as bytes on a copy stream while the previous step runs, and X / Y / SW are produced on the device
        (feed.BatchFeeder: widening copy + dl3_prepare_targets).  A utils.SegmentationGenerator is read through its
        raw_batch(i): with augmentation on, the feeder runs dl3_augment on the device instead of the widening copy; a
        device_resize generator hands over images of any size and the feeder runs dl3_cv_resize in front of it (one GPU).
        validation_data=generator | (x, y[, sw]), validation_steps=, callbacks=[...]: as in fit(); validation batches come
        from the generator's __getitem__ (also with device_feed=True: the feed serves the training half).
        Under distribute() (utils.py:209-211 + :231-241): global_batch=True — the generator yields the GLOBAL batch and each
        rank stages only its contiguous shard (rows dp.shard(n)) — or global_batch=False — the generator is already sharded
        by rank (e.g. `idx[rank::world]`) and yields this rank's images only.  Either way only the shard crosses PCIe."""
        steps = steps_per_epoch or len(generator)
        ses = self._fit_session(kw, epochs, steps, getattr(generator, "batch_size", 32))
        self._check_fit_kw(kw)
        hist = []
        if device_feed:
            return self._fit_device_feed(generator, steps, epochs, n_classes, global_batch, ses)
        for ep in range(epochs):
            if ses:
                ses.epoch_begin(ep)
            for i in range(steps):
                item = generator[i] if hasattr(generator, "__getitem__") else next(generator)
                X, Y = item[0], item[1]
                SW = item[2] if len(item) > 2 else None
                if isinstance(SW, dict):
                    SW = list(SW.values())[0]
                hist.append(self.train_on_batch(X, Y, SW, lazy_loss=True, global_batch=global_batch))
                if ses:
                    ses.batch_end(i, X.shape[0], hist[-1])
            hist = [float(l) for l in hist]   # one read per epoch
            if ses and ses.epoch_end(ep):
                break
            if hasattr(generator, "on_epoch_end"):
                generator.on_epoch_end()
        return ses.end() if ses else hist

    def _fit_device_feed(self, generator, steps, epochs, n_classes, global_batch=True, ses=None):
        from .feed import BatchFeeder
        dp = self._dp if self._dp_active() else None
        ekw = dict(external_nnz=True) if dp is not None else {}
        C = int(n_classes if n_classes is not None else self.output.shape[-1])
        hist, feeders = [], {}
        # utils.SegmentationGenerator: raw_batch() gives the source bytes (+ augmentation parameters) of a batch
        raw = hasattr(generator, "raw_batch")
        plan = getattr(generator, "plan", None) if raw else None
        # device_resize generators hand over LISTS of images of any size; the feeder packs them (feed.BatchFeeder)
        ragged = bool(getattr(plan, "front", False))
        if ragged and dp is not None:
            raise ValueError("fit_generator(device_feed=True): a device_resize generator (images of any size) cannot be "
                             "sharded under distribute(); resize on the host first or train on one GPU")
        for ep in range(epochs):
            if ses:
                ses.epoch_begin(ep)
            # read every epoch, behind on_epoch_begin: a callback (ReduceLROnPlateau, LearningRateScheduler) may have
            # changed the learning rate
            opt = self._opt_desc()

            def batches():
                for i in range(steps):
                    if raw:
                        # the augmentation parameters of the WHOLE global batch are drawn before a rank keeps its shard:
                        # the global batch is the one a single GPU would train on
                        X, L, P = generator.raw_batch(i)
                    else:
                        item = generator[i] if hasattr(generator, "__getitem__") else next(generator)
                        X, L, P = item[0], item[1], None
                    if ragged:
                        yield (X, L, P)
                        continue
                    X, L = np.asarray(X), np.asarray(L)
                    if dp is not None and global_batch:
                        # the rank's contiguous shard of the global batch (the remainder of a batch that does not divide goes
                        # to the last rank, like multi_gpu_model's last tower): only these rows are staged and copied
                        if X.shape[0] < dp.world:
                            raise ValueError("global batch of %d images cannot be split over %d ranks" % (X.shape[0], dp.world))
                        lo, hi = dp.shard(X.shape[0])
                        X, L, P = X[lo:hi], L[lo:hi], (P[lo:hi] if P is not None else None)
                    yield (X, L) if P is None else (X, L, P)
            losses = []
            it = iter(batches())
            first = next(it, None)
            if first is None:
                break
            eng = self._engine(len(first[0]), True, **ekw)
            if dp is not None:
                self._dp_sync_weights(eng)
            ldt = first[1][0].dtype if ragged else first[1].dtype
            key = (id(eng), ldt.str)
            if key not in feeders:
                feeders[key] = BatchFeeder(eng, C, np.uint8 if ldt == np.uint8 else np.int32, plan=plan,
                                           pool_px=generator.pool_pixels if ragged else None)

            def chain():
                yield first
                for b in it:
                    if len(b[0]) != eng.B:
                        raise ValueError("device_feed needs batches of one size (got %d after %d)" % (len(b[0]), eng.B))
                    yield b

            def step():
                eng.fwd_bwd()
                if dp is not None:
                    # ONE all-reduce of the arena (gradients + the shard's count(w != 0) and loss sum) behind the replayed
                    # graph, the scale finished on the device (Engine.train_step does the same for host-array batches)
                    dp.allreduce_grads(eng.grads)
                eng.l2_penalty()    # (the scale: 1, or the external_nnz engine's own)
                eng.opt_step(opt)   # (norm defaults to the engine's external_nnz)
                losses.append(eng.loss_handle())
                if ses:
                    ses.batch_end(len(losses) - 1, eng.B, losses[-1])

            feeders[key].run(chain(), step)
            hist += [float(l) for l in losses]   # one read per epoch
            if ses and ses.epoch_end(ep):
                break
            if hasattr(generator, "on_epoch_end"):
                generator.on_epoch_end()
        return ses.end() if ses else hist


class _FitSession:
    """callbacks and validation around the epochs of fit / fit_generator (the loop of keras.engine.training_generator):
    on_train_begin | per epoch: on_epoch_begin, on_batch_end per step (logs['loss'] is the step's LazyLoss — nothing is
    read unless a callback converts it), then ONE read of the epoch's losses, the validation pass, on_epoch_end with
    {'loss', 'val_*'} | on_train_end.  Training-batch Jaccard / accuracy are not produced (the fused training tails never
    form a mask)."""

    def __init__(self, model, callbacks, validate, epochs, steps):
        from .callbacks import CallbackList, History
        self.model, self.validate = model, validate
        self.history = History()
        self.cbs = CallbackList(list(callbacks or []) + [self.history])   # History last: it records what the others add
        self.cbs.set_model(model)
        self.cbs.set_params(dict(epochs=epochs, steps=steps, verbose=0, do_validation=validate is not None))
        model.stop_training = False
        self.cbs.on_train_begin()

    def epoch_begin(self, epoch):
        self.losses, self.sizes = [], []
        self.cbs.on_epoch_begin(epoch)

    def batch_end(self, batch, size, loss):
        self.losses.append(loss)
        self.sizes.append(int(size))
        self.cbs.on_batch_end(batch, dict(batch=batch, size=int(size), loss=loss))

    def epoch_end(self, epoch):
        """-> True when a callback asked to stop"""
        vals = np.asarray([float(l) for l in self.losses], np.float64)   # the epoch's one read
        w = np.asarray(self.sizes, np.float64)
        logs = {"loss": float((vals * w).sum() / w.sum()) if len(vals) else float("nan")}
        if self.validate is not None:
            logs.update(self.validate())
        self.cbs.on_epoch_end(epoch, logs)
        return bool(self.model.stop_training)

    def end(self):
        self.cbs.on_train_end()
        return self.history

"""Optimizer objects for Model.compile — the reference's notebook compiles with
`Adam(lr=7e-4, epsilon=1e-8, decay=1e-6)` (segmentation.ipynb cell 2), and its utils.py hands the user
`from keras.optimizers import Adam, SGD, RMSprop` (utils.py:16/31).

The update itself is one launch of libdl3.so over the flat parameter arena (engine.Engine.opt_step: dl3_adam_step for
an unclipped Adam, dl3_opt_step for SGD, RMSprop and any rule with clipping); these classes only carry the
hyper-parameters with Keras 2.2.4's names and defaults [TF-semantics: keras/optimizers.py 2.2.4, restated from memory]:
  Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None -> K.epsilon()=1e-7, decay=0., amsgrad=False)
  SGD(lr=0.01, momentum=0., decay=0., nesterov=False)
  RMSprop(lr=0.001, rho=0.9, epsilon=None -> 1e-7, decay=0.)
All three take clipnorm= / clipvalue= (> 0; Optimizer.get_gradients: the GLOBAL norm over every gradient the optimizer
updates, then the clamp); get_config() names them only when they are set."""

KERAS_EPSILON = 1e-7  # keras.backend.epsilon() default


class _Optimizer:
    """learning_rate spelling, clipnorm / clipvalue, config round trip; a subclass lists its hyper-parameters in _HYPER"""
    _HYPER = ()

    def _common(self, kwargs, lr):
        who = type(self).__name__
        if "learning_rate" in kwargs:  # tf.keras spelling
            lr = kwargs.pop("learning_rate")
        self.clipnorm, self.clipvalue = kwargs.pop("clipnorm", None), kwargs.pop("clipvalue", None)
        if kwargs:
            raise TypeError("%s: unexpected keyword arguments %s" % (who, sorted(kwargs)))
        for k in ("clipnorm", "clipvalue"):
            v = getattr(self, k)
            if v is not None:
                if not float(v) > 0:
                    raise ValueError("%s(%s=%r): must be > 0" % (who, k, v))
                setattr(self, k, float(v))
        return lr

    def get_config(self):
        cfg = {k: getattr(self, k) for k in self._HYPER}
        for k in ("clipnorm", "clipvalue"):
            if getattr(self, k) is not None:
                cfg[k] = getattr(self, k)
        return cfg

    @classmethod
    def from_config(cls, cfg):
        return cls(**cfg)

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join(
            "%s=%s" % (k, v if isinstance(v, bool) else "%g" % v) for k, v in self.get_config().items() if k != "amsgrad"))


class Adam(_Optimizer):
    _HYPER = ("lr", "beta_1", "beta_2", "epsilon", "decay", "amsgrad")

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False, **kwargs):
        lr = self._common(kwargs, lr)
        if amsgrad:
            raise ValueError("Adam(amsgrad=True) is not implemented by dl3_adam_step (the reference never uses it)")
        if not (lr >= 0 and 0 <= beta_1 < 1 and 0 <= beta_2 < 1 and decay >= 0):
            raise ValueError("Adam: lr, decay must be >= 0 and beta_1, beta_2 in [0, 1)")
        self.lr, self.beta_1, self.beta_2 = float(lr), float(beta_1), float(beta_2)
        self.epsilon = KERAS_EPSILON if epsilon is None else float(epsilon)
        self.decay = float(decay)
        self.amsgrad = False


class SGD(_Optimizer):
    _HYPER = ("lr", "momentum", "decay", "nesterov")

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False, **kwargs):
        lr = self._common(kwargs, lr)
        if not (lr >= 0 and momentum >= 0 and decay >= 0):
            raise ValueError("SGD: lr, momentum, decay must be >= 0")
        self.lr, self.momentum, self.decay, self.nesterov = float(lr), float(momentum), float(decay), bool(nesterov)


class RMSprop(_Optimizer):
    _HYPER = ("lr", "rho", "epsilon", "decay")

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0.0, **kwargs):
        lr = self._common(kwargs, lr)
        if not (lr >= 0 and 0 <= rho <= 1 and decay >= 0):
            raise ValueError("RMSprop: lr, decay must be >= 0 and rho in [0, 1]")
        self.lr, self.rho, self.decay = float(lr), float(rho), float(decay)
        self.epsilon = KERAS_EPSILON if epsilon is None else float(epsilon)
        if not self.epsilon >= 0:
            raise ValueError("RMSprop: epsilon must be >= 0")


_KEYS = ("lr", "beta_1", "beta_2", "epsilon", "decay")


def as_adam_dict(optimizer):
    """what Model.compile accepts -> the hyper-parameter dict Engine.adam consumes.
    None: the notebook's values (Engine.adam defaults); dict: partial override of those; 'adam' / Adam(): Keras defaults
    for everything not given; any other object exposing Keras' get_config() with an Adam-shaped config is accepted too."""
    if optimizer is None:
        return {}
    if isinstance(optimizer, dict):
        bad = sorted(set(optimizer) - set(_KEYS))
        if bad:
            raise ValueError("compile(optimizer=dict): unknown keys %s (known: %s)" % (bad, list(_KEYS)))
        return {k: float(v) for k, v in optimizer.items()}
    if isinstance(optimizer, str):
        if optimizer.lower() != "adam":
            raise ValueError("compile(optimizer=%r): the only optimizer taken by name is 'adam'; pass an optimizers.SGD / "
                             "RMSprop object for the other rules" % optimizer)
        optimizer = Adam()
    cfg = getattr(optimizer, "get_config", None)
    if cfg is None:
        raise TypeError("compile(optimizer=%r): expected None, a dict, 'adam' or an Adam object" % (optimizer,))
    cfg = cfg()
    if cfg.get("amsgrad"):
        raise ValueError("Adam(amsgrad=True) is not implemented by dl3_adam_step")
    name = type(optimizer).__name__.lower()
    if "adam" not in name or "adamax" in name or "nadam" in name:
        raise ValueError("compile(optimizer=%s): a foreign optimizer object is taken only when it is Adam-shaped; SGD and "
                         "RMSprop are this package's optimizers.SGD / RMSprop" % type(optimizer).__name__)
    if "learning_rate" in cfg and "lr" not in cfg:
        cfg["lr"] = cfg["learning_rate"]
    out = {k: float(cfg[k]) for k in _KEYS if cfg.get(k) is not None}
    out.setdefault("epsilon", KERAS_EPSILON)
    out.setdefault("decay", 0.0)
    return out


def compile_optimizer(optimizer):
    """what Model.compile accepts -> (rule, hyper-parameter dict, clipnorm, clipvalue), the pieces of the description
    Engine.opt_step consumes.  SGD and RMSprop are accepted as instances of THIS package's classes only: the string
    'sgd', or a foreign object that merely has get_config() and is not Adam-shaped, keeps raising (as_adam_dict), so a
    typo or an optimizer this package does not implement never trains silently as something else.  Everything
    as_adam_dict takes is rule 'adam'; clipping comes from this package's Adam, and a foreign Adam whose config asks for
    clipping is refused rather than trained unclipped."""
    if isinstance(optimizer, (SGD, RMSprop)):
        cfg = optimizer.get_config()
        hyper = {k: (bool(cfg[k]) if k == "nesterov" else float(cfg[k])) for k in optimizer._HYPER}
        return type(optimizer).__name__.lower(), hyper, optimizer.clipnorm, optimizer.clipvalue
    hyper = as_adam_dict(optimizer)
    if isinstance(optimizer, Adam):
        return "adam", hyper, optimizer.clipnorm, optimizer.clipvalue
    if not isinstance(optimizer, (dict, str)) and optimizer is not None:
        cfg = optimizer.get_config()
        if cfg.get("clipnorm") or cfg.get("clipvalue"):
            raise ValueError("compile(optimizer=%s): clipnorm / clipvalue are honoured on this package's optimizers.Adam, "
                             "SGD and RMSprop only" % type(optimizer).__name__)
    return "adam", hyper, None, None

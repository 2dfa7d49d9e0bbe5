"""Host-side mirror of the parts of the reference's utils.py that sit on the hot path:
`SegModel.create_seg_model` head surgery (utils.py:169-214), the loss
`sparse_crossentropy_ignoring_last_label` (utils.py:127-130) — executed on the GPU by
dl3_softmax_xent — and host restatements of the metrics that the north star leaves on the host
(`Jaccard` utils.py:139-157, `sparse_accuracy_ignoring_last_label` utils.py:132-138).
Next-ring rows of SURVEY §8(f): `prepare_targets` (N2, the label half of SegmentationGenerator.__getitem__ on the
device) and `Jaccard_from_counts` / `accuracy_from_counts` (N3, metrics from dl3_seg_counts).
`do_crf` (N4) is the host hook with the reference's parameters (it needs the optional pydensecrf package);
`do_crf(..., backend="device")` runs the exact mean-field inference of the same model on the GPU (crf.py, csrc/crf.hip).
The cv2 augmentation chain (utils.py:319-365) runs on the device (augment.py, dl3_augment) behind
SegmentationGenerator's augmentation keywords and SegModel.create_generators; with device_resize=True so does cv2.resize
over images of any size (dl3_cv_resize).
Out of scope by the SURVEY §8 contract: image file I/O, plotting.
"""
import numpy as np

from . import graph as G
from .deeplabv3p import Deeplabv3
from .graph import Activation, Conv2D, Model, Reshape, ResizeBilinear
from .subpixel import Subpixel, icnr_weights
# the reference's `from utils import *` hands the notebook Keras' callbacks (utils.py: `from keras.callbacks import *`)
from .callbacks import (Callback, EarlyStopping, History, LambdaCallback, LearningRateScheduler,  # noqa: F401
                        ModelCheckpoint, ReduceLROnPlateau, poly_decay)
# ... and Keras' optimizers (utils.py:16/31: `from keras.optimizers import Adam, SGD, RMSprop`)
from .optimizers import SGD, Adam, RMSprop  # noqa: F401
# ... and the weight regulariser (utils.py:24/:39: `from keras.regularizers import l2`)
from .regularizers import l2  # noqa: F401


def sparse_crossentropy_ignoring_last_label(y_true, y_pred):
    """Marker for Model.compile(loss=...): the engine's training step always evaluates this loss
    (utils.py:127-130) on the GPU; calling it on host arrays evaluates the same formula in numpy."""
    y_true = np.asarray(y_true)
    p = np.asarray(y_pred, np.float64)
    C = p.shape[-1]
    t = y_true[:, :, 0].astype(np.int64)
    q = np.clip(p / p.sum(-1, keepdims=True), 1e-7, 1 - 1e-7)
    valid = t < C
    out = np.zeros(t.shape)
    b, i = np.nonzero(valid)
    out[b, i] = -np.log(q[b, i, t[b, i]])
    return out


class sparse_crossentropy_top_k:
    """Loss object for Model.compile(loss=...): sparse_crossentropy_ignoring_last_label with online hard-example mining
    (DeepLab's train_utils, restated from memory).  The step trains on the `top_k_percent_pixels` largest
    per-pixel losses w*l of the batch, chosen on the device; with hard_example_mining_step = S > 0 the share ramps down
    from 100 % to top_k_percent_pixels over the first S optimizer updates.  The loss is the sum of the kept losses over
    the number of kept non-zero ones; ties at the threshold are all kept.  top_k_percent_pixels = 1.0 switches mining
    off (the plain loss, bit for bit).  Calling the object on host arrays returns the per-pixel losses, as the plain
    marker does.  Evaluation and prediction are not mined."""

    def __init__(self, top_k_percent_pixels, hard_example_mining_step=0):
        G.check_mining((top_k_percent_pixels, hard_example_mining_step))   # ValueError
        self.top_k_percent_pixels = float(top_k_percent_pixels)
        self.hard_example_mining_step = int(hard_example_mining_step)
        self.__name__ = "sparse_crossentropy_top_k"

    @property
    def mining(self):
        """(p, S) for the training engine; None where the object does not mine (p == 1)"""
        return G.check_mining((self.top_k_percent_pixels, self.hard_example_mining_step))

    def pixels_kept(self, step, n_pixels):
        """k of the step that follows `step` completed optimizer updates, for a batch of n_pixels = B*H*W pixels: the
        device's schedule (dl3_topk_threshold) restated on the host, every operation one rounded float32 operation —
        pct = p if S == 0 else fl(fl(ratio*p) + fl(1 - ratio)), ratio = min(1, fl32(step)/fl32(S));
        k = min(N, trunc(fl(pct * fl32(N))))"""
        f = np.float32
        p, S, N = f(self.top_k_percent_pixels), self.hard_example_mining_step, int(n_pixels)
        pct = p
        if S > 0:
            ratio = min(f(1), f(f(int(step)) / f(S)))
            pct = f(f(ratio * p) + f(f(1) - ratio))
        return min(N, int(np.trunc(np.float64(f(pct * f(N))))))

    def __call__(self, y_true, y_pred):
        return sparse_crossentropy_ignoring_last_label(y_true, y_pred)

    def __repr__(self):
        return "sparse_crossentropy_top_k(%r, %r)" % (self.top_k_percent_pixels, self.hard_example_mining_step)


class sparse_crossentropy_jaccard:
    """Loss object for Model.compile(loss=...): sparse_crossentropy_ignoring_last_label plus jaccard_weight times a
    differentiable (soft) Jaccard term L_J, evaluated on the device.  L_J is this package's own
    definition, mirroring `Jaccard` above: with u = (sample weight != 0 and label not void) and p the softmax, per image
    and class I = sum u p y, S = sum u p, Y = sum u y, J = I / (S + Y - I) where the class occurs (Y > 0); L_J = 1 - the
    mean over the classes that occur anywhere of the mean of J over the images that hold the class (0 for an all-void
    batch).  The sample weights reach the term as the mask u only; the cross-entropy keeps them as they are.
    jaccard_weight = 0 switches the term off (the plain loss, bit for bit).  Calling the object on host arrays returns the
    per-pixel cross-entropy, as the plain marker does.  Evaluation and prediction do not see the term: val_loss stays the
    cross-entropy.  Not available under Model.distribute() or together with hard-example mining."""

    def __init__(self, jaccard_weight=1.0):
        G.check_jaccard(jaccard_weight)   # ValueError
        self.jaccard_weight = float(jaccard_weight)
        self.__name__ = "sparse_crossentropy_jaccard"

    @property
    def jaccard(self):
        """lambda for the training engine; None where the term is off (jaccard_weight == 0)"""
        return G.check_jaccard(self.jaccard_weight)

    def jaccard_term(self, y_true, y_pred, sample_weight=None):
        """L_J in numpy float64 from host arrays: y_true [B,HW,1] (void = C), y_pred [B,HW,C] probabilities,
        sample_weight [B,HW] or None (w = 1)"""
        p = np.asarray(y_pred, np.float64)
        B, HW, C = p.shape
        t = np.asarray(y_true).reshape(B, HW).astype(np.int64)
        u = (t >= 0) & (t < C)
        if sample_weight is not None:
            u &= np.asarray(sample_weight).reshape(B, HW) != 0
        y = (t[..., None] == np.arange(C)) & u[..., None]
        pu = p * u[..., None]
        I, S, Y = (pu * y).sum(1), pu.sum(1), y.sum(1).astype(np.float64)
        present = Y > 0
        if not present.any():
            return 0.0
        J = np.where(present, I / np.where(present, S + Y - I, 1.0), 0.0)
        n_c = present.sum(0)
        legal = n_c > 0
        return float(1.0 - np.mean(J.sum(0)[legal] / n_c[legal]))

    def __call__(self, y_true, y_pred):
        return sparse_crossentropy_ignoring_last_label(y_true, y_pred)

    def __repr__(self):
        return "sparse_crossentropy_jaccard(%r)" % (self.jaccard_weight,)


class sparse_focal_crossentropy:
    """Loss object for Model.compile(loss=...): the focal loss of Lin et al. 2017 (eq. 5) in softmax form with fixed
    per-class weights, evaluated on the device in every form of the training loss tail.  With p the
    softmax, q = clip(p_t / sum p, 1e-7, 1 - 1e-7) as sparse_crossentropy_ignoring_last_label forms it and t the label, a
    pixel's loss is alpha[t] * (1 - q)**gamma * -log(q); the step loss weights it with the sample weight and divides by
    count(sample weight != 0), as the cross-entropy.  alpha: None (every class 1), one number (every class) or one number
    per class.  gamma = 0 with alpha None or all ones switches the loss off (the plain loss, bit for bit).  Calling the
    object on host arrays returns the per-pixel FOCAL loss in float64 (the siblings return the cross-entropy: here the
    per-pixel loss is the focal one).  Evaluation and prediction do not see it: val_loss stays the cross-entropy.  Trains
    under Model.distribute(); not available together with hard-example mining or the soft-Jaccard term."""

    def __init__(self, gamma=2.0, alpha=None):
        G.check_focal((gamma, alpha))   # ValueError
        self.gamma = float(gamma)
        self.alpha = None if alpha is None else (float(alpha) if np.ndim(alpha) == 0 else tuple(
            float(a) for a in np.asarray(alpha, np.float64).reshape(-1)))
        self.__name__ = "sparse_focal_crossentropy"

    @property
    def focal(self):
        """(gamma, alpha) for the training engine; None where the loss is off"""
        return G.check_focal((self.gamma, self.alpha))

    def __call__(self, y_true, y_pred):
        p = np.asarray(y_pred, np.float64)
        B, HW, C = p.shape
        t = np.asarray(y_true).reshape(B, HW).astype(np.int64)
        alpha = np.ones(C) if self.alpha is None else np.asarray(self.alpha, np.float64).reshape(-1)
        if alpha.size not in (1, C):
            raise ValueError("alpha holds %d class weights, y_pred has %d classes" % (alpha.size, C))
        alpha = np.broadcast_to(alpha, (C,))
        valid = (t >= 0) & (t < C)
        tc = np.where(valid, t, 0)
        q = np.clip(np.take_along_axis(p / p.sum(-1, keepdims=True), tc[..., None], -1)[..., 0], 1e-7, 1 - 1e-7)
        return np.where(valid, alpha[tc] * (1.0 - q) ** self.gamma * -np.log(q), 0.0)

    def __repr__(self):
        return "sparse_focal_crossentropy(%r, %r)" % (self.gamma, self.alpha)


def sparse_accuracy_ignoring_last_label(y_true, y_pred):
    """utils.py:132-138 on host."""
    C = y_pred.shape[-1]
    t = np.asarray(y_true).reshape(-1).astype(np.int64)
    pred = np.asarray(y_pred).reshape(-1, C).argmax(-1)
    legal = t != C
    return float((legal & (t == pred)).sum() / max(legal.sum(), 1))


def Jaccard(y_true, y_pred):
    """utils.py:139-157 on host: per class, IoU per image averaged over images containing the class;
    classes that occur nowhere (NaN) are dropped; mean over the remaining classes."""
    y_true = np.asarray(y_true)
    C = y_pred.shape[-1]
    pred = np.asarray(y_pred).argmax(-1)
    t = y_true[:, :, 0]
    ious = []
    for i in range(C):
        tl, pl = t == i, pred == i
        legal = tl.sum(axis=1) > 0
        if legal.any():
            inter = (tl & pl).sum(axis=1)[legal]
            union = (tl | pl).sum(axis=1)[legal]
            ious.append(float(np.mean(inter / union)))
    return float(np.mean(ious)) if ious else float("nan")


def Jaccard_from_counts(counts):
    """`Jaccard` (utils.py:139-157) from the integer counts of dl3_seg_counts, counts[B][3][C] =
    (#true==c, #pred==c, #both): union = true + pred - inter; same float64 ratios and means as `Jaccard`."""
    counts = np.asarray(counts, np.int64)
    t, p, inter = counts[:, 0], counts[:, 1], counts[:, 2]
    ious = []
    for i in range(counts.shape[2]):
        legal = t[:, i] > 0
        if legal.any():
            union = (t[:, i] + p[:, i] - inter[:, i])[legal]
            ious.append(float(np.mean(inter[:, i][legal] / union)))
    return float(np.mean(ious)) if ious else float("nan")


def accuracy_from_counts(counts):
    """`sparse_accuracy_ignoring_last_label` (utils.py:132-138) from dl3_seg_counts output."""
    counts = np.asarray(counts, np.int64)
    return float(counts[:, 2].sum() / max(counts[:, 0].sum(), 1))


def calculate_iou(model, X, label, nb_classes=21):
    """segmentation.ipynb cell 10 on the device: the notebook walks every pixel in Python and fills
    `conf_m[l - 1, p - 1] += 1` for labels below 255; here Model.confusion_matrix accumulates the matrix in one device
    pass.  Returned in the notebook's own layout, as float: index -1 wraps, so class 0 lands in the LAST row / column
    (np.roll(plain, -1, axis=(0, 1))) — reproduced, not fixed.  X [N,H,W,3] raw 0-255 images, label [N,H,W] with void
    >= nb_classes (255 in VOC)."""
    label = np.asarray(label)
    y = np.where((label >= 0) & (label < nb_classes), label, nb_classes).astype(np.float32).reshape(len(label), -1, 1)
    plain = np.asarray(model.confusion_matrix(X, y))
    return np.roll(plain, -1, axis=(0, 1)).astype(float)


def calculate_iou_multiscale(model, X, label, nb_classes=21, **tta_kwargs):
    """calculate_iou with the masks of Model.predict_multiscale in place of the single-scale argmax: the
    same layout, rolled class 0 included.  The masks come from the device (output="mask"); the matrix is a host bincount
    over label * nb_classes + prediction of the pixels whose label is below nb_classes.  tta_kwargs: scales, flip,
    batch_size, crf, factory."""
    if "output" in tta_kwargs:
        raise ValueError("calculate_iou_multiscale builds its matrix from masks: output= is not an option")
    label = np.asarray(label)
    pred = model.predict_multiscale(X, output="mask", **tta_kwargs).reshape(-1).astype(np.int64)
    lab = label.reshape(-1).astype(np.int64)
    C = int(model.output.shape[-1])   # Model.confusion_matrix's extent: the model's classes
    keep = (lab >= 0) & (lab < min(nb_classes, C))
    plain = np.bincount(lab[keep] * C + pred[keep], minlength=C * C).reshape(C, C)
    return np.roll(plain, -1, axis=(0, 1)).astype(float)


def calculate_iou_sliding(model, X, label, nb_classes=21, **slide_kwargs):
    """calculate_iou with the masks of Model.predict_sliding: images of any size, each judged at its own
    resolution; the same layout, rolled class 0 included.  X and label are arrays [N,Hi,Wi,3] / [N,Hi,Wi] or lists of images
    / label maps of different sizes.  The masks come from the device; the matrix is calculate_iou_multiscale's host
    bincount.  slide_kwargs: stride, blend, batch_size, pad_value."""
    if "output" in slide_kwargs:
        raise ValueError("calculate_iou_sliding builds its matrix from masks: output= is not an option")
    masks = model.predict_sliding(X, output="mask", **slide_kwargs)
    if len(masks) != len(label) or any(np.shape(m) != np.shape(l) for m, l in zip(masks, label)):
        raise ValueError("calculate_iou_sliding: label must hold one [Hi,Wi] map per image")
    pred = np.concatenate([np.asarray(m).reshape(-1) for m in masks]).astype(np.int64)
    lab = np.concatenate([np.asarray(l).reshape(-1) for l in label]).astype(np.int64)
    C = int(model.output.shape[-1])   # Model.confusion_matrix's extent: the model's classes
    keep = (lab >= 0) & (lab < min(nb_classes, C))
    plain = np.bincount(lab[keep] * C + pred[keep], minlength=C * C).reshape(C, C)
    return np.roll(plain, -1, axis=(0, 1)).astype(float)


def iou_from_confusion(conf):
    """(per-class IoU, their mean over the classes that occur) of a confusion matrix [C,C] in the PLAIN layout (row = label,
    column = prediction — Model.confusion_matrix's, not calculate_iou's rolled one): I = diagonal, U = row sum + column sum
    - I, the `I/U` notebook cell 10 computes; NaN where the union is 0, and such classes stay out of the mean (NaN if none
    is left).  Leading axes are kept: [K+1,C,C] -> ([K+1,C], [K+1])."""
    conf = np.asarray(conf, np.float64)
    if conf.ndim < 2 or conf.shape[-1] != conf.shape[-2]:
        raise ValueError("iou_from_confusion: conf must be [...,C,C], got shape %r" % (conf.shape,))
    inter = np.diagonal(conf, axis1=-2, axis2=-1)
    union = conf.sum(-1) + conf.sum(-2) - inter
    iou = np.full(inter.shape, np.nan)
    np.divide(inter, union, out=iou, where=union > 0)
    n = (union > 0).sum(-1)
    mean = np.full(n.shape, np.nan)
    np.divide(np.where(union > 0, iou, 0.0).sum(-1), n, out=mean, where=n > 0)
    return iou, (float(mean) if mean.ndim == 0 else mean)


def _trimap_result(widths, band):
    from . import trimap
    conf = trimap.cumulative(band).cpu().numpy() if hasattr(band, "data_ptr") else np.asarray(band)
    return dict(widths=tuple(widths), confusion=conf, miou=np.asarray(iou_from_confusion(conf)[1], np.float64))


def trimap_iou(model, X, label, nb_classes=21, widths=(1, 2, 4, 8, 16, 32), metric="chebyshev", seeds=("void", "edges"),
               crf=False, crf_unary="labels", batch_size=32):
    """The trimap experiment: mIoU restricted to bands around the object boundaries, where the output heads
    and the dense CRF differ.  X [N,H,W,3] raw 0-255 images, label [N,H,W] with void >= nb_classes (255 in VOC).
    -> dict(widths, confusion = int64 [K+1,C,C] CUMULATIVE plain-layout matrices, slice k over the pixels within widths[k]
    of a boundary and the last slice over every pixel, miou = [K+1], iou_from_confusion's mean of each slice).
    crf=False: Model.confusion_matrix_trimap — one device evaluation pass; crf=True: the masks of
    Model.predict_mask(crf=True, crf_unary=...) judged by trimap.band_confusion."""
    from . import trimap
    ws = trimap.check_widths(widths)
    trimap.check_metric(metric), trimap.check_seeds(seeds)
    C = int(model.output.shape[-1])
    label = np.asarray(label)
    lab = np.where((label >= 0) & (label < min(nb_classes, C)), label, C).astype(np.float32)
    if not crf:
        conf = model.confusion_matrix_trimap(X, lab.reshape(len(lab), -1, 1), batch_size=batch_size, widths=ws, metric=metric,
                                             seeds=seeds)
        return _trimap_result(ws, conf)
    masks = model.predict_mask(X, batch_size=batch_size, crf=True, crf_unary=crf_unary)
    return _trimap_result(ws, trimap.band_confusion(masks, lab, C, ws, metric=metric, seeds=seeds))


def trimap_iou_from_masks(masks, label, nb_classes=21, widths=(1, 2, 4, 8, 16, 32), metric="chebyshev",
                          seeds=("void", "edges")):
    """trimap_iou for masks from anywhere (Model.predict_multiscale(output="mask"), Model.predict_sliding, a file):
    masks and label are arrays [N,H,W] or lists of [Hi,Wi] maps of different sizes; the images of one size share one
    launch pair, the bins of all sizes accumulate in one device array.  Labels outside 0..nb_classes-1 are void."""
    from . import trimap
    ws, C = trimap.check_widths(widths), trimap.check_classes(nb_classes)
    trimap.check_metric(metric), trimap.check_seeds(seeds)
    if len(masks) != len(label) or len(masks) == 0 or any(np.shape(m) != np.shape(l) or np.ndim(m) != 2
                                                          for m, l in zip(masks, label)):
        raise ValueError("trimap_iou_from_masks: masks and label must hold one [Hi,Wi] map per image, of equal shapes")
    by_size = {}
    for i, m in enumerate(masks):
        by_size.setdefault(tuple(np.shape(m)), []).append(i)
    band = None
    for idx in by_size.values():
        m = np.stack([np.asarray(masks[i]) for i in idx])
        l = np.stack([np.asarray(label[i]) for i in idx])
        band = trimap.band_confusion(m, l, C, ws, metric=metric, seeds=seeds, out=band)
    return _trimap_result(ws, band)


def add_weight_decay(model, l2=4e-5, depthwise=0.0, bias=0.0, batchnorm=0.0):
    """DeepLab's weight decay on a built model: sets `kernel_regularizer=l2(l2)` on every Conv2D / Subpixel,
    `depthwise_regularizer=l2(depthwise)` on every DepthwiseConv2D, `bias_regularizer=l2(bias)` on every bias and
    `gamma_regularizer` / `beta_regularizer` = l2(batchnorm) on every BatchNormalization; 0.0 REMOVES the regulariser.
    -> the number of weights that now carry one.  Model.compile() MUST FOLLOW: the regularisers in force are collected
    there, so a model compiled before this call trains unchanged until it is compiled again.
    The defaults: 4e-5 on the convolution kernels is DeepLab's training recipe; none on the depthwise kernels follows the
    MobileNet authors' advice (few parameters per filter) — both restated from memory.  Not part of the reference."""
    from . import regularizers as R   # (the keyword `l2` shadows the imported class in here)

    def reg(l):   # noqa: E741
        r = R.l2(l)   # refuses l < 0 and non-finite l
        return r if r.l2 > 0 else None
    kernel, dw, b, bn = reg(l2), reg(depthwise), reg(bias), reg(batchnorm)
    covered = 0
    for layer in model.layers:
        if layer.kind in ("Conv2D", "Subpixel"):
            layer.kernel_regularizer = kernel
            layer.bias_regularizer = b if layer.cfg["use_bias"] else None
        elif layer.kind == "DepthwiseConv2D":
            layer.depthwise_regularizer = dw
        elif layer.kind == "BatchNormalization":
            layer.gamma_regularizer = layer.beta_regularizer = bn
        covered += sum(getattr(layer, k, None) is not None for k in R.KEYWORDS)
    return covered


def prepare_targets(labels, n_classes=21):
    """Device-side label half of SegmentationGenerator.__getitem__ (utils.py:375-402): raw label maps
    [B,H,W] or [B,HW] (uint8 / int32; numpy array or cuda tensor) -> (Y [B,HW,1], SW [B,HW]) cuda float32 tensors, ready
    for `Model.train_on_batch(X, Y, SW)`.  Runs dl3_prepare_targets; raises if libdl3.so is missing."""
    import torch
    from . import capi
    if isinstance(labels, np.ndarray):
        if labels.dtype not in (np.uint8, np.int32):
            labels = labels.astype(np.int32)
        labels = torch.from_numpy(np.ascontiguousarray(labels)).cuda()
    if labels.dtype not in (torch.uint8, torch.int32):
        labels = labels.to(torch.int32)
    labels = labels.contiguous().reshape(labels.shape[0], -1)
    B, HW = labels.shape
    Y = torch.empty(B, HW, 1, device=labels.device, dtype=torch.float32)
    SW = torch.empty(B, HW, device=labels.device, dtype=torch.float32)
    hist = torch.empty(B, n_classes + 1, device=labels.device, dtype=torch.int32)
    capi.call("dl3_prepare_targets", capi.ptr(labels), capi.LABEL_U8 if labels.dtype == torch.uint8 else capi.LABEL_I32,
              B, HW, n_classes, capi.ptr(Y), capi.ptr(SW), capi.ptr(hist), torch.cuda.current_stream().cuda_stream)
    return Y, SW


# Dense-CRF post-processing: the reference's parameter set (utils.py:74-91), shared by the host hook and
# the device backend.  pydensecrf is not a dependency of this package: the hook imports it on first use.
CRF_PARAMS = dict(gt_prob=0.7, gaussian_sxy=(3, 3), gaussian_compat=3, bilateral_sxy=80, bilateral_srgb=13,
                  bilateral_compat=10, iterations=5)


def restore_crf_labels(MAP, colors):
    """MAP indices -> the mask's original values, exactly as the reference does it (utils.py:86-89): for every index u
    present in MAP, ascending, `np.putmask(MAP, MAP == u, colors[u])` IN PLACE.  The quirk is reproduced, not fixed
    (SURVEY G5): a value written for an earlier index is matched again by a later one — with mask values {0, 2, 15} index
    1 becomes 2 and is then rewritten to 15 together with index 2, so class 2 vanishes from the result.  Masks whose
    values are 0..n-1 (the usual label maps) come back unchanged."""
    for u in np.unique(MAP):
        np.putmask(MAP, MAP == u, colors[u])
    return MAP


def do_crf(im, mask, zero_unsure=True, backend="pydensecrf"):
    """Fully connected CRF refinement of a label mask given the image (reference utils.py:74-91): unary energies from
    the labels with CRF_PARAMS['gt_prob'], a Gaussian (position) and a bilateral (position + colour) pairwise term,
    five mean-field iterations, MAP labels mapped back to the mask's original values by the reference's own in-place
    loop (restore_crf_labels).

    backend="pydensecrf" (the default) is the reference's call sequence on the host and needs that package;
    backend="device" runs the exact mean-field inference of the same model on the GPU (crf.dense_crf, dl3_crf_inference:
    all pixel pairs instead of pydensecrf's lattice approximation) and returns the same type and shape.
    A mask with a single value is returned unchanged by the device backend (pydensecrf's unary divides by
    n_labels - 1)."""
    if backend == "device":
        from .crf import dense_crf
        mask = np.asarray(mask)
        if len(np.unique(mask)) < 2:
            return mask
        return dense_crf(np.asarray(im)[None], mask.reshape((1,) + mask.shape[:2]), zero_unsure=zero_unsure)[0]
    if backend != "pydensecrf":
        raise ValueError("do_crf: backend must be 'pydensecrf' or 'device', got %r" % (backend,))
    try:
        import pydensecrf.densecrf as dcrf
        from pydensecrf.utils import unary_from_labels
    except ImportError as e:  # pragma: no cover - optional host dependency
        raise ImportError("do_crf needs the optional host package pydensecrf (not installed)") from e
    colors, labels = np.unique(mask, return_inverse=True)
    labels = labels.reshape(-1)  # numpy 1.x (the reference's) returns the inverse flat; numpy >= 2 in the mask's shape
    image_size = mask.shape[:2]
    n_labels = len(set(labels.flat))
    crf = dcrf.DenseCRF2D(image_size[1], image_size[0], n_labels)  # width, height, nlabels
    crf.setUnaryEnergy(unary_from_labels(labels, n_labels, gt_prob=CRF_PARAMS["gt_prob"], zero_unsure=zero_unsure))
    crf.addPairwiseGaussian(sxy=CRF_PARAMS["gaussian_sxy"], compat=CRF_PARAMS["gaussian_compat"])
    crf.addPairwiseBilateral(sxy=CRF_PARAMS["bilateral_sxy"], srgb=CRF_PARAMS["bilateral_srgb"],
                             rgbim=np.ascontiguousarray(im.astype("uint8")), compat=CRF_PARAMS["bilateral_compat"])
    q = crf.inference(CRF_PARAMS["iterations"])
    MAP = np.argmax(q, axis=0).reshape(image_size)
    return restore_crf_labels(MAP, colors)


def do_crf_softmax(im, probs, scale=None, clip=1e-5):
    """do_crf with the network's class probabilities as the unary term instead of a label mask (DeepLab's own CRF step;
    pydensecrf.utils.unary_from_softmax): im [H,W,3], probs [H,W,C] or [H*W,C] -> class ids int64 [H,W].  Runs on the
    GPU (crf.dense_crf_softmax) with the kernel parameters and iteration count of CRF_PARAMS."""
    from .crf import dense_crf_softmax
    probs = np.asarray(probs)
    return dense_crf_softmax(np.asarray(im)[None], probs=probs.reshape((1,) + probs.shape), scale=scale, clip=clip)[0]


class SegmentationGenerator:
    """The tensor contract of the reference's `SegmentationGenerator` (utils.py:257-409) over IN-MEMORY arrays:
    `gen[i]` -> `(X [B,H,W,3] float32, Y [B,HW,1], {'pred_mask': SW [B,HW]})`, `len(gen)` batches, `on_epoch_end()`
    reshuffles.  File I/O is out of scope: the caller hands over decoded images (raw 0-255 BGR, as
    `self.X[n] = image`, utils.py:387) and raw label maps; the label half (utils.py:371-400) runs on the device through
    dl3_prepare_targets, so Y and SW are cuda tensors that `Model.fit_generator` / `train_on_batch` consume without a host
    round trip.

    Augmentation (utils.py:319-365): the reference's keywords `resize_shape, crop_shape, horizontal_flip, vertical_flip,
    blur, brightness, rotation, zoom, do_ahisteq` (cv2 (width, height) order for the shapes), all OFF by default.  With
    any of them on, images must be uint8, the per-image parameters come from one `random.Random(seed)` in the
    reference's call order (augment.Plan.draw; `on_epoch_end` shuffles with the same stream, as the reference's global
    `random` does), and the chain runs on the device (dl3_augment): X comes back as host float32, Y / SW stay on the
    device.  `raw_batch(i)` hands the same batch to the device feed before augmentation.

    device_resize=True (off by default): `images` / `labels` may be lists of per-image arrays of different sizes, or arrays
    of any one size.  resize_shape resizes every image as cv2.resize does (INTER_LINEAR, the label map INTER_NEAREST);
    crop_shape follows _random_crop per image (utils.py:411-423): an image larger than the crop both ways is cropped at a
    drawn origin, any other is resized to crop_shape without a draw.  Blur, resize and crop run in dl3_cv_resize, the
    rest of the chain in dl3_augment over the uniform batch; with every other flag off X is the widened resized image."""

    def __init__(self, images, labels, n_classes=21, batch_size=1, seed=7, shuffle=True, resize_shape=None,
                 crop_shape=None, horizontal_flip=False, vertical_flip=False, blur=0, brightness=0.0, rotation=0.0,
                 zoom=0.0, do_ahisteq=False, device_resize=False):
        import random
        from . import augment
        self.n_classes = int(n_classes)
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self._rng = np.random.RandomState(seed)
        self.random = random.Random(seed)
        self.device_resize = bool(device_resize)
        if self.device_resize:
            self._init_any_size(images, labels, resize_shape, crop_shape, horizontal_flip, vertical_flip, blur, brightness,
                                rotation, zoom, do_ahisteq)
            return
        self.images = np.asarray(images)
        self.labels = np.asarray(labels)
        if self.images.ndim != 4 or self.images.shape[-1] != 3 or len(self.images) != len(self.labels):
            raise Exception("images must be [N,H,W,3] and labels [N,H,W]")
        self.order = np.arange(len(self.images))
        self.plan = augment.Plan(self.images.shape[1:3], resize_shape, crop_shape, horizontal_flip, vertical_flip, blur,
                                 brightness, rotation, zoom, do_ahisteq)
        if self.plan.active:
            self._check_dtypes(self.images.dtype, self.labels.dtype)

    def _check_dtypes(self, idt, ldt):
        if idt != np.uint8:
            raise ValueError("augmentation reads decoded uint8 images, got %s" % idt)
        if ldt not in (np.uint8, np.int32):
            raise ValueError("augmentation reads uint8 / int32 label maps, got %s" % ldt)
        if self.plan.warp and ldt != np.uint8:
            raise ValueError("rotation / zoom warp the label map as uint8 (cv2.warpAffine, utils.py:353): "
                             "int32 label maps cannot be warped")

    def _init_any_size(self, images, labels, *opts):
        """device_resize=True: per-image arrays of any size (a list, or a uniform array); cv2.resize / the per-image crop
        of utils.py:322-327 run on the device (dl3_cv_resize) in front of the rest of the chain"""
        from . import augment
        self.images = [np.asarray(i) for i in images]
        self.labels = [np.asarray(l) for l in labels]
        if not self.images or len(self.images) != len(self.labels):
            raise ValueError("device_resize: one label map per image, got %d images and %d maps"
                             % (len(self.images), len(self.labels)))
        for n, (i, l) in enumerate(zip(self.images, self.labels)):
            if i.ndim != 3 or i.shape[2] != 3 or l.shape != i.shape[:2] or not i.size:
                raise ValueError("device_resize: image %d is %r with a label map %r; images are [H,W,3], maps [H,W]"
                                 % (n, i.shape, l.shape))
        self.sizes = [i.shape[:2] for i in self.images]
        self.order = np.arange(len(self.images))
        same = len(set(self.sizes)) == 1
        self.plan = augment.Plan(self.sizes[0] if same else None, *opts, device_resize=True)
        idt, ldt = set(i.dtype for i in self.images), set(l.dtype for l in self.labels)
        if len(idt) != 1 or len(ldt) != 1:
            raise ValueError("device_resize: images and label maps must each have one dtype, got %s / %s"
                             % (sorted(map(str, idt)), sorted(map(str, ldt))))
        self._check_dtypes(idt.pop(), ldt.pop())

    @property
    def pool_pixels(self):
        """device_resize: the pixels a batch can hold at most — the batch_size largest images (what the feeder's slots and
        this generator's own device buffers are sized for)"""
        return int(sum(sorted((h * w for h, w in self.sizes), reverse=True)[:self.batch_size]))

    def __len__(self):
        return len(self.images) // self.batch_size

    def _index(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self.order[i * self.batch_size:(i + 1) * self.batch_size]

    def raw_batch(self, i):
        """(uint8 images [B,Hs,Ws,3], label maps [B,Hs,Ws], params) of batch i before augmentation; params is the list
        of augment.ImageParams drawn for it (None when no augmentation is on)"""
        idx = self._index(i)
        if self.device_resize:    # lists of per-image arrays; each draw sees its image's size
            return ([self.images[j] for j in idx], [self.labels[j] for j in idx],
                    [self.plan.draw(self.random, self.sizes[j]) for j in idx])
        params = [self.plan.draw(self.random) for _ in idx] if self.plan.active else None
        return self.images[idx], self.labels[idx], params

    def _getitem_any_size(self, i):
        import torch
        from . import augment
        images, labels, params = self.raw_batch(i)
        plan, B = self.plan, len(params)
        tab, offs, info = augment.batch_tables(plan, [im.shape[:2] for im in images], params)
        info = info._replace(pool_px=self.pool_pixels)
        ldt = torch.uint8 if labels[0].dtype == np.uint8 else torch.int32
        if getattr(self, "_dev", None) is None:
            n = info.pool_px
            # device buffers of one batch, allocated once and reused by every batch of this generator
            self._dev = dict(img=torch.empty(3 * n, dtype=torch.uint8, device="cuda"),
                             lab=torch.empty(n, dtype=ldt, device="cuda"),
                             fws=torch.empty(augment.front_workspace_bytes(info._replace(blur_any=int(bool(plan.blur)))),
                                             dtype=torch.uint8, device="cuda"),
                             rimg=torch.empty(B, plan.H, plan.W, 3, dtype=torch.uint8, device="cuda"),
                             rlab=torch.empty(B, plan.H, plan.W, dtype=ldt, device="cuda"),
                             present=torch.empty(B, 8, dtype=torch.int32, device="cuda"),
                             X=torch.empty(B, plan.H, plan.W, 3, dtype=torch.float32, device="cuda"),
                             L=torch.empty(B, plan.H * plan.W, dtype=ldt, device="cuda"),
                             ws=torch.empty(augment.workspace_bytes(plan.inner, B), dtype=torch.uint8, device="cuda"))
        d = self._dev
        ipool, lpool = augment.pack_pools(images, labels)
        d["img"][:ipool.size].copy_(torch.from_numpy(ipool))
        d["lab"][:lpool.size].copy_(torch.from_numpy(lpool))
        dtab = torch.from_numpy(tab).cuda()
        augment.launch_front(info, dtab, offs, d["img"], d["lab"], d["rimg"], d["rlab"], d["present"], d["fws"])
        augment.launch(plan.inner, dtab, offs, d["rimg"], d["rlab"], self.n_classes, d["X"], d["L"], d["ws"],
                       present=d["present"])
        Y, SW = prepare_targets(d["L"], self.n_classes)
        return d["X"].cpu().numpy(), Y, {"pred_mask": SW}

    def __getitem__(self, i):
        if self.device_resize:
            return self._getitem_any_size(i)
        if not self.plan.active:
            idx = self._index(i)
            X = np.ascontiguousarray(self.images[idx], dtype=np.float32)
            Y, SW = prepare_targets(self.labels[idx], self.n_classes)
            return X, Y, {"pred_mask": SW}
        import torch
        from . import augment
        images, labels, params = self.raw_batch(i)
        plan, B = self.plan, len(params)
        tab, offs = augment.tables(plan, params)
        ldt = torch.uint8 if labels.dtype == np.uint8 else torch.int32
        if getattr(self, "_dev", None) is None or self._dev[0] != (B, tab.size, ldt):
            # device buffers of one batch, allocated once and reused by every batch of this generator
            self._dev = ((B, tab.size, ldt), torch.empty(tab.size, dtype=torch.int32, device="cuda"),
                         torch.empty(images.shape, dtype=torch.uint8, device="cuda"),
                         torch.empty(labels.shape, dtype=ldt, device="cuda"),
                         torch.empty(B, plan.H, plan.W, 3, dtype=torch.float32, device="cuda"),
                         torch.empty(B, plan.H * plan.W, dtype=ldt, device="cuda"),
                         torch.empty(augment.workspace_bytes(plan, B), dtype=torch.uint8, device="cuda"))
        _, dtab, dimg, dlab, X, L, ws = self._dev
        dtab.copy_(torch.from_numpy(tab))
        dimg.copy_(torch.from_numpy(np.ascontiguousarray(images)))
        dlab.copy_(torch.from_numpy(np.ascontiguousarray(labels)))
        augment.launch(plan, dtab, offs, dimg, dlab, self.n_classes, X, L, ws)
        Y, SW = prepare_targets(L, self.n_classes)
        return X.cpu().numpy(), Y, {"pred_mask": SW}

    def on_epoch_end(self):
        if self.shuffle:
            if self.plan.active:
                self.random.shuffle(self.order)    # utils.py:404-408: the stream the augmentation draws from
            else:
                self._rng.shuffle(self.order)


class SegModel:
    """utils.py:160-254 — model construction, the generators and train_generator."""
    epochs = 20
    batch_size = 16

    def __init__(self, dataset="VOCdevkit/VOC2012", image_size=(320, 320)):
        self.sz = tuple(image_size)
        self.mainpath = dataset
        self.crop = False

    def create_seg_model(self, net, n=21, backbone="mobilenetv2", load_weights=False, multi_gpu=False):
        """net='original': DeepLabV3+ body + conv_upsample 1x1 + bilinear (utils.py:188-193);
        net='subpixel': body + Subpixel(n, 1, scale) with ICNR init (utils.py:194-204).
        The body is Deeplabv3(weights=None, classes=21, OS=16) cut at model.layers[-5] (utils.py:177-181).
        multi_gpu: the reference's in-graph keras.utils.multi_gpu_model (utils.py:209-211) becomes one process per
        GPU + one RCCL all-reduce of the gradients per step: Model.distribute() attaches parallel.DataParallel, which
        reads RANK / WORLD_SIZE (launch with `python -m torch.distributed.run --nproc-per-node <gpus> ...`); every
        train_on_batch then takes the global batch and trains on this rank's shard."""
        model = Deeplabv3(weights=None, input_tensor=None, infer=False, input_shape=self.sz + (3,), classes=21,
                          backbone=backbone, OS=16, alpha=1)
        base_model = Model(model.input, model.layers[-5].output)
        self.net = net
        self.modelpath = "weights/{}_{}.h5".format(backbone, net)
        scale = 4 if backbone == "xception" else 8
        if net == "original":
            x = Conv2D(n, (1, 1), padding="same", name="conv_upsample")(base_model.output)
            x = ResizeBilinear((self.sz[0], self.sz[1]))(x)
            x = Reshape((self.sz[0] * self.sz[1], -1))(x)
            x = Activation("softmax", name="pred_mask")(x)
            model = Model(base_model.input, x, name="deeplabv3p")
        elif net == "subpixel":
            x = Subpixel(n, 1, scale, padding="same")(base_model.output)
            x = Reshape((self.sz[0] * self.sz[1], -1))(x)
            x = Activation("softmax", name="pred_mask")(x)
            model = Model(base_model.input, x, name="deeplabv3p_subpixel")
        else:
            raise ValueError("net must be 'original' or 'subpixel'")
        for layer in model.layers:  # ICNR re-initialisation (utils.py:200-204)
            if type(layer) == Subpixel:
                c, b = layer.get_weights()
                layer.set_weights([icnr_weights(scale=scale, shape=c.shape), b])
        if load_weights:
            model.load_weights(self.modelpath)
        if multi_gpu:
            model.distribute()
            if model._dp.world == 1:
                import warnings
                warnings.warn("multi_gpu=True in a single process: this package runs one process per GPU — launch the "
                              "script with `python -m torch.distributed.run --nproc-per-node <gpus>` to use them",
                              RuntimeWarning, stacklevel=2)
        # the same head for another image size (Model.predict_multiscale's sibling models)
        dataset = self.mainpath
        model._tta_rebuild = lambda shape: SegModel(dataset, image_size=tuple(shape[:2])).create_seg_model(
            net, n=n, backbone=backbone, load_weights=False, multi_gpu=False)
        self.model = model
        return model

    def create_generators(self, crop_shape=False, mode="train", do_ahisteq=True, n_classes=21, horizontal_flip=True,
                          vertical_flip=False, blur=False, with_bg=True, brightness=0.1, rotation=5.0, zoom=0.1,
                          validation_split=.2, seed=7, images=None, labels=None, device_resize=False):
        """utils.py:216-226 over in-memory arrays (this package reads no files): `images` uint8 [N,H,W,3] in cv2's BGR
        order at the model's size (or larger, with crop_shape), `labels` uint8 / int32 [N,H,W].  mode 'train' /
        'validation' split as the reference does (utils.py:268-276): np.random.seed(seed); the first
        round(N * validation_split) of permutation(N) validate, the sorted rest trains.  with_bg is accepted and ignored,
        as in the reference.  device_resize=True: `images` / `labels` are lists of per-image arrays of any sizes (or arrays
        of any one size) and every image is resized to the model's size — or cropped / resized to crop_shape, per image —
        on the device, as the reference's cv2.resize does (utils.py:322-327)."""
        if mode not in ("train", "validation"):
            raise ValueError("create_generators: mode %r is not supported (the reference's 'test' mode reads the test "
                             "JPEG folder; this package reads no files)" % (mode,))
        if images is None or labels is None:
            raise ValueError("create_generators: pass the decoded data as images= (uint8 [N,H,W,3], BGR) and labels= "
                             "(uint8 / int32 [N,H,W]); reading the dataset folder %r (JPEG decode) is out of scope"
                             % (self.mainpath,))
        if not device_resize:
            images, labels = np.asarray(images), np.asarray(labels)
        n = len(images)
        x = np.random.RandomState(seed).permutation(n)[:round(n * validation_split)]
        if mode == "train":
            x = np.setxor1d(x, np.arange(n))
        if device_resize:
            images, labels = [images[j] for j in x], [labels[j] for j in x]
        else:
            images, labels = images[x], labels[x]
        return SegmentationGenerator(images, labels, n_classes=n_classes, batch_size=self.batch_size, seed=seed,
                                     device_resize=device_resize,
                                     resize_shape=self.sz[::-1], crop_shape=crop_shape, horizontal_flip=horizontal_flip,
                                     vertical_flip=vertical_flip, blur=blur, brightness=brightness, rotation=rotation,
                                     zoom=zoom, do_ahisteq=do_ahisteq)

    def load_weights(self, model):
        model.load_weights(self.modelpath)

    def train_generator(self, model, train_generator, valid_generator, callbacks, mp=True, workers=1, max_queue_size=10):
        """utils.py:231-241: one fit_generator call over the two generators with the notebook's callbacks; returns the
        History.  mp / workers / max_queue_size are accepted and ignored (batches are produced on the device).
        `SegModel.train` is not built: as committed it calls a `self.build_callbacks` the class does not have."""
        return model.fit_generator(train_generator, steps_per_epoch=len(train_generator), epochs=self.epochs, verbose=1,
                                   callbacks=callbacks, validation_data=valid_generator,
                                   validation_steps=len(valid_generator), max_queue_size=max_queue_size,
                                   workers=workers, use_multiprocessing=mp)

    @classmethod
    def set_num_epochs(cls, new_epochs):
        cls.epochs = new_epochs

    @classmethod
    def set_batch_size(cls, new_batch_size):
        cls.batch_size = new_batch_size
